#!/usr/bin/env python3
"""The planes of a scan, measured on one MI355X -> profiles/planes_timing.txt ("The planes of a scan").

    python tools/planes_timing.py --out planes_timing.txt [--kernel-stats stats.txt]
    rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/planes_timing.py --trace-loop      (a run of its own)
    python tools/rocprof_summary.py DIR > stats.txt

Scene: the bench scene (the 80 k-voxel generator scene, every voxel's point and two jittered copies: about 92 k voxels and
239 k vertices) with the normals estimate_normals() gives it.  a3d_find_planes at max_planes 1, 6 and 16: device events around
the call alone (its clears and the upload-free table included), outputs in the caller's buffers, no host copy; median / min /
max of 30 after 5 warm-up calls.  planes(): host clock around the session call, which ends in its one host round trip.  The
kernels of a call are launches inside it: their times come from the kernel trace of a separate run (--trace-loop: 31 calls at
max_planes = 16) when its summary is given with --kernel-stats.  There is no CPU path: the tool needs the GPU.
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
VOXEL = 0.02
KERNELS = ("k_plane_vote", "k_plane_peak", "k_plane_sums", "k_plane_step", "k_plane_assign", "k_plane_lift")


def bench_scene():
    rng = np.random.default_rng(0)
    sc = make_scene(80_000, seed=0, voxel_size=VOXEL)
    raw = sc["raw_xyz"]
    xyz = np.concatenate([raw] + [raw + rng.uniform(-0.004, 0.004, raw.shape).astype(np.float32) for _ in range(2)])
    return xyz.astype(np.float32), np.concatenate([sc["feats"]] * 3).astype(np.float32)


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


def kernel_rows(path):
    """The rows of tools/rocprof_summary.py's text for this tool's kernels."""
    out = []
    for line in open(path):
        f = line.split(None, 4)
        if len(f) == 5 and f[0].isdigit() and any(k in f[4] for k in KERNELS):
            out.append(f"  {int(f[0]):7d} calls  {float(f[1]):12.1f} us total  {float(f[2]):10.2f} us average  "
                       f"{f[4].strip().split('(')[0].replace('a3d::', '').replace('void ', '')}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="planes_timing.txt")
    ap.add_argument("--kernel-stats", default=None, help="rocprof_summary.py's text of the --trace-loop run")
    ap.add_argument("--trace-loop", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("planes_timing needs the GPU")
    torch.manual_seed(0)
    model = randomize_bn_stats(build_model(default_args(voxel_size=VOXEL))).eval().cuda()
    xyz, col = bench_scene()
    ses = InteractiveSession(model, voxel_size=VOXEL).load_scene(xyz, col, None, name="bench scene")
    dev = ses.device
    res = ses.estimate_normals()
    n, n_full = ses.raw_coords_qv.shape[0], ses.coords_full.shape[0]
    origin, quantum, bits = ses._fixed_point_frame()
    outs = dict(plane_qv=torch.empty(n, dtype=torch.int32, device=dev), plane_full=torch.empty(n_full, dtype=torch.int32, device=dev),
                out=torch.empty(V.PLANES_OUT_BYTES, dtype=torch.uint8, device=dev), workspace=V.planes_workspace(n, dev),
                table=torch.from_numpy(V.direction_table()).to(dev))
    call = lambda k: V.find_planes(res.normals_qv, ses.raw_coords_qv, origin, quantum, bits, offset_bin=VOXEL, normal_deg=20.0,
                                   dist_tol=1.5 * VOXEL, min_voxels=200, max_planes=k, inverse_map=ses.inverse_map, **outs)
    if a.trace_loop:
        for _ in range(REPS + 1):
            call(16)
        torch.cuda.synchronize()
        return
    lines = ["The planes of a scan: a3d_find_planes (DESIGN.md 4.9, \"The planes of a scan\")",
             "One MI355X, one run, as measured; written by tools/planes_timing.py (its docstring says how each number is taken).",
             "Nothing existed before: no speed was promised and no threshold is set.",
             f"\n== bench scene: {n_full} vertices, {n} voxels (voxel size {VOXEL}), bits = {bits}; {res.valid} voxels with a normal",
             f"{'device us, median / min / max of ' + str(REPS):64s}{'median':>10s}{'min':>10s}{'max':>10s}"]
    for k in (1, 6, 16):
        t = device_us(lambda: call(k))
        _, s = V.read_planes(outs["out"].cpu().numpy())
        launches = 1 + 10 * 2 * k + 1
        lines.append(f"  {'a3d_find_planes max_planes = %2d: %2d planes, %2d rounds (%d spent), %3d launches + 2 clears' % (k, s['n_planes'], s['rounds'], s['spent'], launches):62s}"
                     f"{t[0]:10.1f}{t[1]:10.1f}{t[2]:10.1f}")
    t = host_ms(lambda: ses.planes())
    r = ses.planes()
    lines.append(f"{'host ms around the session call (one host round trip)':64s}{'median':>10s}{'min':>10s}{'max':>10s}")
    lines.append(f"  {'planes(): %d planes %s' % (r.n_planes, r.kinds):62s}{t[0]:10.3f}{t[1]:10.3f}{t[2]:10.3f}")
    lines.append(f"  inliers {r.records['inliers'].tolist()}; admitted {r.admitted}, left out {r.left_out}")
    if a.kernel_stats:
        lines.append(f"\n== per kernel, from the kernel trace of a separate run ({REPS + 1} calls at max_planes = 16)")
        lines += kernel_rows(a.kernel_stats)
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
