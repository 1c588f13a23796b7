#!/usr/bin/env python3
"""Normals for point clouds, measured on one MI355X -> profiles/normals_timing.txt ("Normals for point clouds").

    python tools/normals_timing.py --out normals_timing.txt [--kernel-stats bench_stats.txt cloud_stats.txt]
    rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/normals_timing.py --trace-loop --scene 0   (a run of its own, per scene)
    python tools/rocprof_summary.py DIR > bench_stats.txt

Scenes: the bench scene (the 80 k-voxel generator scene, every voxel's point and two jittered copies: about 92 k voxels and
239 k vertices) and the ~1 M-vertex cloud of profiles/region_timing.txt (the 100 k-voxel scene, ten vertices per voxel).
Library calls: device events around the call alone (its clears included), outputs in the caller's buffers, no host copy;
median / min / max of 30 after 5 warm-up calls.  estimate_normals(): host clock around the session call, which ends in its
one host round trip.  The three stages of a3d_estimate_normals are launches inside one call: their times come from the
kernel trace of a separate run per scene (--trace-loop --scene K: 31 calls) when the summaries are given with --kernel-stats.  For
context, on the 92 k scene: a host numpy recipe -- one covariance per voxel (not per 27-voxel neighbourhood) from a sort of
the vertices, then numpy.linalg.eigh -- by the host clock.  There is no CPU path: the tool needs the GPU.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from agile3d_amd import build_model, default_args, randomize_bn_stats  # noqa: E402
from agile3d_amd import view as V  # noqa: E402
from agile3d_amd.session import InteractiveSession  # noqa: E402
from agile3d_amd.synthetic import make_scene  # noqa: E402

REPS, WARM = 30, 5
KERNELS = ("k_normals_moments", "k_normals_solve", "k_normals_lift", "k_cull_points", "k_render_shade_lit_points")


def scenes():
    rng = np.random.default_rng(0)
    for name, voxels, copies in (("bench scene", 80_000, 2), ("~1 M-vertex cloud", 100_000, 9)):
        sc = make_scene(voxels, seed=0, voxel_size=0.02)
        raw = sc["raw_xyz"]
        xyz = np.concatenate([raw] + [raw + rng.uniform(-0.004, 0.004, raw.shape).astype(np.float32) for _ in range(copies)])
        yield name, xyz.astype(np.float32), np.concatenate([sc["feats"]] * (copies + 1)).astype(np.float32)


def device_us(call):
    for _ in range(WARM):
        call()
    times = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1000.0)
    return float(np.median(times)), min(times), max(times)


def host_ms(call):
    for _ in range(WARM):
        call()
    times = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1000.0)
    return float(np.median(times)), min(times), max(times)


def numpy_recipe(xyz, inv, n):
    """One covariance per voxel from a sort of the vertices, then eigh: (seconds, voxels with >= 3 vertices)."""
    t0 = time.perf_counter()
    order = np.argsort(inv, kind="stable")
    p = xyz[order].astype(np.float64)
    starts = np.flatnonzero(np.r_[True, np.diff(inv[order]) != 0])
    rows = inv[order][starts]
    cnt = np.diff(np.r_[starts, len(p)])
    s = np.add.reduceat(p, starts, axis=0)
    outer = (p[:, :, None] * p[:, None, :]).reshape(-1, 9)
    m = np.add.reduceat(outer, starts, axis=0).reshape(-1, 3, 3)
    mean = s / cnt[:, None]
    cov = m / cnt[:, None, None] - mean[:, :, None] * mean[:, None, :]
    w, v = np.linalg.eigh(cov)
    normals = np.zeros((n, 3))
    normals[rows] = np.where((cnt >= 3)[:, None], v[:, :, 0], 0.0)
    return time.perf_counter() - t0, int((cnt >= 3).sum())


def run(ses, name, lines, trace_only):
    dev = ses.device
    n, n_full = ses.raw_coords_qv.shape[0], ses.coords_full.shape[0]
    origin, quantum, bits = ses._fixed_point_frame()
    scene, xyz, inv = ses._scene_handle(), ses.coords_full, ses.inverse_map
    outs = dict(normal_qv=torch.empty((n, 3), device=dev), variation_qv=torch.empty(n, device=dev),
                count_qv=torch.empty(n, dtype=torch.int32, device=dev), moments_qv=False,
                summary=torch.empty(32, dtype=torch.uint8, device=dev), workspace=V.normals_workspace(n, dev))
    full = torch.empty((n_full, 3), device=dev)
    whole = lambda: V.estimate_normals(scene, xyz, origin, quantum, bits, inv, origin, normal_full=full, **outs)
    no_lift = lambda: V.estimate_normals(scene, xyz, origin, quantum, bits, inv, origin, normal_full=False, **outs)
    res = ses.estimate_normals()
    culled = torch.empty_like(xyz)
    hidden, count = torch.empty(n_full, dtype=torch.uint8, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
    eye = (origin + np.array([30.0, -20.0, 12.0])).astype(np.float32)
    cull = lambda: V.cull_points(xyz, ses.normals, eye, "back", out=culled, hidden=False, count=False)
    cull_counted = lambda: V.cull_points(xyz, ses.normals, eye, "back", out=culled, hidden=hidden, count=count)
    views = []
    for w, h in ((640, 480), (1280, 720)):
        k, e = ses.default_view(w, h)
        r = ses.render(k, e, w, h)
        rgb = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        views.append((w, h, r, rgb))
    if trace_only:
        for _ in range(REPS):
            whole(), cull()
            for w, h, r, rgb in views:
                V.render_shade_lit_points(r.ids, ses.colors_full, ses.normals, r.camera, 0.35, (1, 1, 1), rgb=rgb)
        torch.cuda.synchronize()
        return
    lines.append(f"\n== {name}: {n_full} vertices, {n} voxels (voxel size 0.02), bits = {bits}; {res.valid} voxels with a normal, "
                 f"{res.invalid} without")
    lines.append(f"{'device us, median / min / max of ' + str(REPS):58s}{'median':>10s}{'min':>10s}{'max':>10s}")
    row = lambda what, t: lines.append(f"  {what:56s}{t[0]:10.1f}{t[1]:10.1f}{t[2]:10.1f}")
    row("a3d_estimate_normals, whole call (A, B, the lift)", device_us(whole))
    row("a3d_estimate_normals without the lift (A, B)", device_us(no_lift))
    row("a3d_cull_points (the copy alone)", device_us(cull))
    row("a3d_cull_points with hidden and count", device_us(cull_counted))
    for w, h, r, rgb in views:
        shown = int((r.ids >= 0).sum())
        lines.append(f"  view {w} x {h}: {shown} of {w * h} pixels show a vertex")
        row(f"a3d_render_shade_lit_points {w} x {h}", device_us(lambda: V.render_shade_lit_points(
            r.ids, ses.colors_full, ses.normals, r.camera, 0.35, (1, 1, 1), rgb=rgb)))
        row(f"a3d_render_shade {w} x {h} (flat, for context)", device_us(lambda: V.render_shade(
            r.ids, None, None, None, ses.colors_full, (1, 1, 1), rgb=rgb)))
        row(f"a3d_render_shade_depth {w} x {h} (for context)", device_us(lambda: V.render_shade_depth(
            r.ids, r.t, None, None, None, ses.colors_full, 8.0, (1, 1, 1), rgb=rgb)))
    t = host_ms(lambda: ses.estimate_normals())
    lines.append(f"{'host ms around the session call (one host round trip)':58s}{'median':>10s}{'min':>10s}{'max':>10s}")
    lines.append(f"  {'estimate_normals()':56s}{t[0]:10.3f}{t[1]:10.3f}{t[2]:10.3f}")
    if name == "bench scene":
        secs, rich = numpy_recipe(ses._coords_host, inv.cpu().numpy(), n)
        lines.append(f"host numpy recipe, for context (per-voxel covariance from a sort + numpy.linalg.eigh; {rich} voxels with >= 3 "
                     f"vertices): {secs * 1000.0:.1f} ms, one run")


def kernel_rows(path):
    """The rows of tools/rocprof_summary.py's text for this tool's kernels."""
    out = []
    for line in open(path):
        f = line.split(None, 4)
        if len(f) == 5 and f[0].isdigit() and any(k in f[4] for k in KERNELS):
            out.append(f"  {int(f[0]):7d} calls  {float(f[2]):10.2f} us average  {f[4].strip().split('(')[0].replace('a3d::', '').replace('void ', '')}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="normals_timing.txt")
    ap.add_argument("--kernel-stats", nargs="*", default=[], help="rocprof_summary.py texts of the --trace-loop runs, one per scene")
    ap.add_argument("--trace-loop", action="store_true")
    ap.add_argument("--scene", type=int, default=None, help="only scene 0 (bench) or 1 (the 1 M-vertex cloud)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("normals_timing needs the GPU")
    torch.manual_seed(0)
    model = randomize_bn_stats(build_model(default_args(voxel_size=0.02))).eval().cuda()
    lines = ["Normals for point clouds: a3d_estimate_normals, a3d_cull_points, a3d_render_shade_lit_points (DESIGN.md 4.9, \"Normals "
             "for point clouds\")",
             "One MI355X, one run, as measured; written by tools/normals_timing.py (its docstring says how each number is taken).",
             "Nothing existed before: no speed was promised and no threshold is set."]
    names = []
    for index, (name, xyz, col) in enumerate(scenes()):
        names.append(name)
        if a.scene is not None and index != a.scene:
            continue
        ses = InteractiveSession(model, voxel_size=0.02).load_scene(xyz, col, None, name=name)
        run(ses, name, lines, a.trace_loop)
        del ses
        torch.cuda.empty_cache()
    if a.trace_loop:
        return
    for name, path in zip(names, a.kernel_stats):
        lines.append(f"\n== {name}: per kernel, from the kernel trace of a separate run ({REPS + 1} calls of a3d_estimate_normals, "
                     f"{REPS} of the others; the lit pass at both view sizes together)")
        lines += kernel_rows(path)
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
