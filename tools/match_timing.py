#!/usr/bin/env python3
"""The query by example, measured on one MI355X -> profiles/match_timing.txt ("More objects like this one").

    python tools/match_timing.py --out match_timing.txt [--bench-text bench_lines.txt]

Scene: the bench scene of tools/patches_timing.py (the 80 k-voxel generator scene, every voxel's point and two jittered
copies).  Features: the backbone's own output for that scene (random weights), fp32 [n_voxels, 128].  For k = 1, 20 and 255
prototypes the voxels are cut into k + 1 slabs along x: slab 0 is the background, slab j the examples of object j -- so a
quarter of the rows at least are examples, far more than an annotator labels, which is the prototype kernel's worst case.
Library calls: device events around the call alone (its clears included), outputs in the caller's buffers, no host copy;
median / min / max of 30 after 5 warm-up calls.  GB/s = the 512 bytes of every feature row the call has to read, over the
median: a rate of the whole call, not a kernel's share of peak.  lookalikes(): host clock around the call, which ends in its
host round trips; the labelling is planted (``ses._labels_qv`` and the keys of ``ses.click_idx`` set directly: the click list
does not take 255 objects, and the method reads nothing else of the annotation).  --bench-text: lines to append as they are
(the bench.py headline of this commit next to the parent's, taken by the caller in the same visit).
There is no CPU path: the tool needs the GPU.
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
KS = (1, 20, 255)


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


def slabs(ses, k):
    """int32 [n_voxels] on the device: 0 (background) or the object 1..k of the voxel's slab along x."""
    x = ses.raw_coords_qv[:, 0].cpu().numpy()
    edges = np.quantile(x, np.arange(1, k + 1) / (k + 1))
    return torch.from_numpy(np.searchsorted(edges, x).astype(np.int32)).to(ses.device)


def run(ses, lines):
    dev = ses.device
    feats = ses._backbone[0].F.contiguous()
    n, n_full = feats.shape[0], ses.coords_full.shape[0]
    row_bytes = n * V.MATCH_CHANNELS * 4
    lines.append(f"\n== bench scene: {n_full} vertices, {n} voxels (voxel size 0.02); features fp32 [{n}, 128] = {row_bytes / 1e6:.1f} MB")
    lines.append(f"{'device us, median / min / max of ' + str(REPS):88s}{'median':>10s}{'min':>10s}{'max':>10s}{'GB/s':>9s}")

    def row(what, t, nbytes=None):
        lines.append(f"  {what:86s}{t[0]:10.1f}{t[1]:10.1f}{t[2]:10.1f}" + ("" if nbytes is None else f"{nbytes / t[0] / 1e3:9.0f}"))
    match_qv, best_qv = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    score_qv = torch.empty(n, dtype=torch.float32, device=dev)
    full = dict(inverse_map=ses.inverse_map, match_full=torch.empty(n_full, dtype=torch.int32, device=dev),
                score_full=torch.empty(n_full, dtype=torch.float32, device=dev))
    outs = dict(match_qv=match_qv, best_qv=best_qv, score_qv=score_qv, summary=torch.empty(V.MATCH_SUMMARY.itemsize, dtype=torch.uint8, device=dev))
    planted = {}
    for k in KS:
        labels = slabs(ses, k)
        classes = torch.where(labels > 0, labels, torch.full_like(labels, -1))
        examples = int((classes >= 0).sum())
        sums = torch.empty((k + 1, V.MATCH_CHANNELS), dtype=torch.int64, device=dev)
        count, psum = torch.empty(k + 1, dtype=torch.int32, device=dev), torch.empty(V.PROTOTYPES_SUMMARY.itemsize, dtype=torch.uint8, device=dev)
        row(f"a3d_feature_prototypes, {k} classes, {examples} example rows",
            device_us(lambda: V.feature_prototypes(feats, classes, k + 1, sums=sums, count=count, summary=psum)), examples * 512)
        s = V.read_prototypes_summary(psum.cpu().numpy())
        lines.append(f"    ({s['examples']} rows summed, {s['examples_left_out']} left out)")
        ids = torch.arange(1, k + 1, dtype=torch.int32, device=dev)
        protos = V.prototype_table(sums, count)[1:].contiguous()
        candidate = (labels == 0).to(torch.uint8)
        row(f"a3d_feature_match, {k} prototypes, every voxel a candidate, no lift", device_us(lambda: V.feature_match(feats, protos, ids, 0.9, **outs)), row_bytes)
        row(f"a3d_feature_match, {k} prototypes, the background as candidates, with the lift",
            device_us(lambda: V.feature_match(feats, protos, ids, 0.9, candidate=candidate, **outs, **full)), row_bytes)
        m = V.read_match_summary(outs["summary"].cpu().numpy())
        lines.append(f"    ({int(m['matched'].sum())} of {int(candidate.sum())} candidates matched at cos_min 0.9, {m['rows_nonfinite']} rows not finite)")
        planted[k] = labels
    row("prototype_table on the device (256 classes)", device_us(lambda: V.prototype_table(sums, count)))
    lines.append(f"{'host ms around the session call (with its host round trips)':88s}{'median':>10s}{'min':>10s}{'max':>10s}")
    hrow = lambda what, t: lines.append(f"  {what:86s}{t[0]:10.3f}{t[1]:10.3f}{t[2]:10.3f}")
    for k in KS:
        ses._labels_qv, ses.click_idx = planted[k], {str(j): [] for j in range(k + 1)}
        for cos_min in (0.9, 0.999):
            res = ses.lookalikes(cos_min=cos_min)
            hrow(f"lookalikes(), {k} prototypes, cos_min {cos_min}", host_ms(lambda: ses.lookalikes(cos_min=cos_min)))
            lines.append(f"    ({int((res.match_qv >= 0).sum())} voxels matched, {res.n_regions} regions of 8 voxels or more, {res.n_regions_searched} searched, "
                         f"{len(res.candidates)} candidates)")
    ses._labels_qv, ses.click_idx = planted[1], {"0": [], "1": []}
    hrow("lookalikes(obj=1), 1 prototype", host_ms(lambda: ses.lookalikes(obj=1)))
    hrow("pieces(), for context", host_ms(lambda: ses.pieces()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="match_timing.txt")
    ap.add_argument("--bench-text", default=None, help="a text file to append as it is: the bench.py lines of this commit and its parent")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("match_timing needs the GPU")
    torch.manual_seed(0)
    model = randomize_bn_stats(build_model(default_args(voxel_size=0.02))).eval().cuda()
    lines = ["More objects like this one: a3d_feature_prototypes, a3d_feature_match, lookalikes() (DESIGN.md 4.9, \"More objects like this one\")",
             "One MI355X, one run, as measured; written by tools/match_timing.py (its docstring says how each number is taken).",
             "Nothing existed before: no speed was promised and no threshold is set."]
    rng = np.random.default_rng(0)
    sc = make_scene(80_000, seed=0, voxel_size=0.02)
    raw = sc["raw_xyz"]
    xyz = np.concatenate([raw] + [raw + rng.uniform(-0.004, 0.004, raw.shape).astype(np.float32) for _ in range(2)])
    ses = InteractiveSession(model, voxel_size=0.02).load_scene(xyz.astype(np.float32), np.concatenate([sc["feats"]] * 3).astype(np.float32), None,
                                                              name="bench scene")
    run(ses, lines)
    if a.bench_text:
        lines += ["", ""] + open(a.bench_text).read().rstrip("\n").split("\n")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
