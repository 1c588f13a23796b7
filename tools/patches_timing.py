#!/usr/bin/env python3
"""Smooth patches, the magic wand and the snap, measured on one MI355X -> profiles/patches_timing.txt (DESIGN.md 4.9,
"Smooth patches").

    python tools/patches_timing.py --out patches_timing.txt [--baseline-text parent.txt]
    python tools/patches_timing.py --baseline --out parent.txt        (in a checkout of the PARENT commit: the yardstick)

Scenes: those of tools/normals_timing.py -- the bench scene (the 80 k-voxel generator scene, every voxel's point and two
jittered copies) and the ~1 M-vertex cloud (the 100 k-voxel scene, ten vertices per voxel).  Normals: estimate_normals().
Colours: what load_scene fed the backbone.  Labels for the vote: four slabs along x with 5 % of the voxels relabelled at
random.  Library calls: device events around the call alone (its clears included), outputs in the caller's buffers, no host
copy; median / min / max of 30 after 5 warm-up calls.  Session calls: host clock around the call, which ends in its host
round trips.  --baseline measures only what the parent commit has -- a3d_label_pieces on all-zero keys and on the slab
labels, and pieces() -- with this script's scenes and clocks; its text is appended to the report with --baseline-text.
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


def slab_labels(ses):
    """int32 [n_voxels] on the device: four slabs along x, 5 % of the voxels relabelled at random (0..3)."""
    x = ses.raw_coords_qv[:, 0].cpu().numpy()
    edges = np.quantile(x, [0.25, 0.5, 0.75])
    lab = np.searchsorted(edges, x).astype(np.int32)
    rng = np.random.default_rng(1)
    flip = rng.random(len(lab)) < 0.05
    lab[flip] = rng.integers(0, 4, int(flip.sum()))
    return torch.from_numpy(lab).to(ses.device)


def run(ses, name, lines, baseline):
    dev = ses.device
    n, n_full = ses.raw_coords_qv.shape[0], ses.coords_full.shape[0]
    scene, inv = ses._scene_handle(), ses.inverse_map
    labels = slab_labels(ses)
    zeros = torch.zeros_like(labels)
    outs = dict(piece_qv=torch.empty(n, dtype=torch.int32, device=dev), records=torch.empty(4096 * V.PIECE.itemsize, dtype=torch.uint8, device=dev),
                count=torch.empty(2, dtype=torch.int32, device=dev))
    full = dict(inverse_map=inv, piece_full=torch.empty(n_full, dtype=torch.int32, device=dev))
    lines.append(f"\n== {name}: {n_full} vertices, {n} voxels (voxel size 0.02)")
    lines.append(f"{'device us, median / min / max of ' + str(REPS):88s}{'median':>10s}{'min':>10s}{'max':>10s}")
    row = lambda what, t: lines.append(f"  {what:86s}{t[0]:10.1f}{t[1]:10.1f}{t[2]:10.1f}")
    ws = V.pieces_workspace(n, dev)
    count = lambda: int(outs["count"].cpu()[0])
    row("a3d_label_pieces, keys all 0, with the lift", device_us(lambda: V.label_pieces(scene, zeros, workspace=ws, **outs, **full)))
    lines.append(f"    ({count()} pieces)")
    row("a3d_label_pieces, the slab labels, with the lift", device_us(lambda: V.label_pieces(scene, labels, workspace=ws, **outs, **full)))
    lines.append(f"    ({count()} pieces)")
    row("a3d_label_pieces, keys all 0, no lift", device_us(lambda: V.label_pieces(scene, zeros, workspace=ws, **outs)))
    if not baseline:
        res = ses.estimate_normals()
        normals, feats = res.normals_qv, ses.colors_full[ses._unique_map].contiguous()
        cos_min, tol2 = np.float32(np.cos(np.radians(15.0))), np.float32(0.1) ** 2
        for what, kw in (("neither array (the bytes of a3d_label_pieces)", dict()),
                         ("normals, 15 degrees", dict(normals=normals, cos_min=cos_min)),
                         ("colours, tolerance 0.1", dict(feats=feats, tol2=tol2)),
                         ("normals and colours", dict(normals=normals, feats=feats, cos_min=cos_min, tol2=tol2)),
                         ("normals and colours, the slab labels as keys", dict(keys=labels, normals=normals, feats=feats, cos_min=cos_min, tol2=tol2)),
                         ("normals, and the reference test at 15 degrees", dict(normals=normals, cos_min=cos_min, ref_normal=[0.0, 0.0, 1.0], ref_cos_min=cos_min))):
            row(f"a3d_similar_pieces, {what}, with the lift", device_us(lambda: V.similar_pieces(scene, workspace=ws, **kw, **outs, **full)))
            lines.append(f"    ({count()} pieces)")
        row("a3d_similar_pieces, normals, no lift", device_us(lambda: V.similar_pieces(scene, normals=normals, cos_min=cos_min, workspace=ws, **outs)))
        vote_ws = V.vote_workspace(n, dev, 65536, 256)
        piece = V.similar_pieces(scene, normals=normals, cos_min=cos_min, workspace=vote_ws, **outs)[0].clone()
        labels_out, summary = torch.empty_like(labels), torch.empty(32, dtype=torch.uint8, device=dev)
        vote = lambda: V.vote_pieces(scene, labels, piece, vote_ws, 8, (2, 3), (), 256, 65536, labels_out=labels_out, summary=summary)
        row("a3d_vote_pieces on the normals' partition (capacity 65536, 256 classes)", device_us(vote))
        s = V.read_vote_summary(summary.cpu().numpy())
        lines.append(f"    ({s['eligible_pieces']} eligible pieces, {s['relabelled_pieces']} relabelled, {s['relabelled_voxels']} voxels changed)")
    lines.append(f"{'host ms around the session call (with its host round trips)':88s}{'median':>10s}{'min':>10s}{'max':>10s}")
    hrow = lambda what, t: lines.append(f"  {what:86s}{t[0]:10.3f}{t[1]:10.3f}{t[2]:10.3f}")
    hrow("pieces()", host_ms(lambda: ses.pieces()))
    if not baseline:
        host_labels = labels.cpu().numpy()
        for obj in (1, 2, 3, 0):                                         # a click per slab, then the slab labels replayed as logits
            ses.click(ses._coords_qv_host[np.flatnonzero(host_labels == obj)[0]], obj)
        logits = torch.full((n, 4), -2.0, device=dev)
        logits[torch.arange(n, device=dev), labels.long()] = 3.0
        ses.infer(logits=logits)
        k, e = ses.default_view(640, 480)
        view = ses.render(k, e, 640, 480)
        hit = np.argwhere(view.ids.cpu().numpy() >= 0)
        j, i = (int(a) for a in hit[len(hit) // 2])
        p = ses.patches()
        lines.append(f"    (patches(): {p.n_pieces} patches)")
        hrow("patches()", host_ms(lambda: ses.patches()))
        hrow("patches(color_tol=0.1)", host_ms(lambda: ses.patches(color_tol=0.1)))
        hrow("wand_at(), chain", host_ms(lambda: ses.wand_at(view, i, j)))
        hrow("wand_at(), seed", host_ms(lambda: ses.wand_at(view, i, j, mode="seed")))
        hrow("snap(patches)", host_ms(lambda: ses.snap(p)))
        hrow("snap() with patches() computed in it", host_ms(lambda: ses.snap()))
        hrow("despeckle(), for context", host_ms(lambda: ses.despeckle()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="patches_timing.txt")
    ap.add_argument("--baseline", action="store_true", help="measure only a3d_label_pieces and pieces(): what the parent commit has")
    ap.add_argument("--baseline-text", default=None, help="the text a --baseline run in a checkout of the parent wrote, to append")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("patches_timing needs the GPU")
    torch.manual_seed(0)
    model = randomize_bn_stats(build_model(default_args(voxel_size=0.02))).eval().cuda()
    if a.baseline:
        lines = ["THE YARDSTICK: a3d_label_pieces and pieces() of the parent commit, by this script, same scenes, same device, same day."]
    else:
        lines = ["Smooth patches, the magic wand and the snap: a3d_similar_pieces, a3d_vote_pieces, patches(), wand_at(), snap() "
                 "(DESIGN.md 4.9, \"Smooth patches\")",
                 "One MI355X, one run, as measured; written by tools/patches_timing.py (its docstring says how each number is taken).",
                 "Nothing existed before: no speed was promised and no threshold is set."]
    for name, xyz, col in scenes():
        ses = InteractiveSession(model, voxel_size=0.02).load_scene(xyz, col, None, name=name)
        run(ses, name, lines, a.baseline)
        del ses
        torch.cuda.empty_cache()
    if a.baseline_text:
        lines += ["", ""] + open(a.baseline_text).read().rstrip("\n").split("\n")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
