#!/usr/bin/env python3
"""Normals oriented by propagation, measured on one MI355X -> profiles/orient_timing.txt ("One sign for a whole
surface").

    python tools/orient_timing.py --out orient_timing.txt [--bench-text bench.txt]

Scenes: the bench scene (the 80 k-voxel generator scene, every voxel's point and two jittered copies: about 92 k voxels and
239 k vertices) and the ~1 M-vertex cloud the other timing tools use (the 100 k-voxel scene, ten vertices per voxel), each with
the normals estimate_normals() gives it and the components a3d_label_pieces finds among the voxels with a normal.
a3d_orient_normals in the NEAREST mode at 26-connectivity, outputs in the caller's buffers, no host copy: device events around
the call alone, median / min / max of 30 after 5 warm-up calls.  The phases are launches inside one call, so they are taken
apart by the number of sweeps asked for: at sweeps = 1 the call is everything BUT the relaxation (edge table, seeds, one sweep,
close, parents, pointer-jumping rounds, finish, conflicts); at the session's 512 it adds the sweeps that work and the launches
that return at once behind them; at S*, the least number of sweeps after which the call reports `converged` (found by
bisection), it adds only the sweeps that work.  The sweeps that did work are S* - 1: the last one finds nothing to lower.
orient_normals(): host clock around the session call, which labels the components and ends in its one host round trip.
--bench-text: a text file appended as it is (the bench.py headline of this commit next to the parent's, taken by the caller in
the same visit).  There is no CPU path: the tool needs the GPU.
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


def scenes():
    rng = np.random.default_rng(0)
    for name, voxels, copies in (("bench scene", 80_000, 2), ("~1 M-vertex cloud", 100_000, 9)):
        sc = make_scene(voxels, seed=0, voxel_size=VOXEL)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="orient_timing.txt")
    ap.add_argument("--bench-text", default=None, help="a text file to append as it is: the bench.py lines of this commit and its parent")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("orient_timing needs the GPU")
    torch.manual_seed(0)
    model = randomize_bn_stats(build_model(default_args(voxel_size=VOXEL))).eval().cuda()
    lines = ["One sign for a whole surface: a3d_orient_normals (DESIGN.md 4.9, \"One sign for a whole surface\")",
             "One MI355X, one run, as measured; written by tools/orient_timing.py (its docstring says how each number is taken).",
             "Nothing existed before: no speed was promised and no threshold is set."]
    row = lambda what, t, unit="%10.1f": f"  {what:78s}" + "".join(unit % x for x in t)
    for name, xyz, col in scenes():
        ses = InteractiveSession(model, voxel_size=VOXEL).load_scene(xyz, col, None, name=name)
        dev = ses.device
        est = ses.estimate_normals()
        n, n_full = ses.raw_coords_qv.shape[0], ses.coords_full.shape[0]
        nrm = est.normals_qv.contiguous()
        has = torch.isfinite(nrm).all(1) & (nrm != 0).any(1)
        keys = has.to(torch.int32) - 1
        pieces = dict(piece_qv=torch.empty(n, dtype=torch.int32, device=dev), records=torch.empty(40, dtype=torch.uint8, device=dev),
                      count=torch.empty(2, dtype=torch.int32, device=dev), workspace=V.pieces_workspace(n, dev))
        label = lambda: V.label_pieces(ses._scene_handle(), keys, 26, **pieces)
        comp = label()[0]
        outs = dict(normal_out_qv=torch.empty(n, 3, device=dev), flipped_qv=torch.empty(n, dtype=torch.uint8, device=dev),
                    dist_qv=torch.empty(n, dtype=torch.int32, device=dev), owner_qv=torch.empty(n, dtype=torch.int32, device=dev),
                    normal_full=torch.empty(n_full, 3, device=dev), summary=torch.empty(64, dtype=torch.uint8, device=dev),
                    workspace=V.orient_workspace(n, dev))
        vp = ses._fixed_point_frame()[0]
        call = lambda sweeps: V.orient_normals(ses._scene_handle(), nrm, components=comp, positions=ses.raw_coords_qv, viewpoint=vp,
                                               connectivity=26, sweeps=sweeps, inverse_map=ses.inverse_map, **outs)
        done = lambda sweeps: (call(sweeps), V.read_orient_summary(outs["summary"].cpu().numpy()))[1]
        lo, hi = 0, V.ORIENT_MAX_SWEEPS                                 # converged(lo) is false, converged(hi) must be true
        s = done(hi)
        if not s["converged"]:
            raise SystemExit(f"{name}: not converged after {hi} sweeps")
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if done(mid)["converged"] else (mid, hi)
        star = hi
        rounds = max(n - 1, 0).bit_length()
        lines += [f"\n== {name}: {n_full} vertices, {n} voxels (voxel size {VOXEL}); {s['admitted']} voxels with a normal, "
                  f"{s['seeds']} components with a seed",
                  f"   reached {s['reached']}, flipped {s['flipped']}, conflicts {s['conflicts']}, largest path cost {s['max_dist']}; "
                  f"sweeps that did work: {star - 1} (converged is reported from {star} sweeps on); {rounds} pointer-jumping rounds",
                  f"  {'device us, median / min / max of ' + str(REPS):78s}{'median':>10s}{'min':>10s}{'max':>10s}"]
        lines.append(row("a3d_label_pieces on the voxels with a normal (the components of \"nearest\")", device_us(label)))
        fixed = device_us(lambda: call(1))
        lines.append(row(f"a3d_orient_normals, sweeps = 1: everything but the relaxation ({9 + rounds} kernels, 4 clears)", fixed))
        exact = device_us(lambda: call(star))
        lines.append(row(f"a3d_orient_normals, sweeps = {star}: + the sweeps that work", exact))
        whole = device_us(lambda: call(512)) if star <= 512 else None
        if whole:
            lines.append(row(f"a3d_orient_normals, sweeps = 512 (the session's): + {512 - star} launches that return at once", whole))
            lines.append(f"    so: the relaxation {exact[0] - fixed[0]:.1f} us = {(exact[0] - fixed[0]) / max(star - 1, 1):.2f} us a working sweep; "
                         f"an idle launch {(whole[0] - exact[0]) / max(512 - star, 1):.2f} us")
        t = host_ms(lambda: ses.orient_normals(normals=est))
        r = ses.orient_normals(normals=est)
        lines.append(f"  {'host ms around the session call':78s}{'median':>10s}{'min':>10s}{'max':>10s}")
        lines.append(row(f"orient_normals(): {r.launched} sweeps launched, {r.launched // 512} host round trip(s)", t, "%10.3f"))
        del ses
        torch.cuda.empty_cache()
    if a.bench_text:
        lines.append("")
        lines.append(open(a.bench_text).read().rstrip("\n"))
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
