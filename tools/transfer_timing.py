#!/usr/bin/env python3
"""Labels to and from another point set, measured on one MI355X -> profiles/transfer_timing.txt ("Labels to and
from another point set").

    python tools/transfer_timing.py --out transfer_timing.txt

Scenes: those of tools/normals_timing.py -- the bench scene (the 80 k-voxel generator scene, every voxel's point and two
jittered copies: about 92 k voxels and 239 k vertices) and the ~1 M-vertex cloud (the 100 k-voxel scene, ten vertices per
voxel).  The other point set: 1 M points, the scene's own vertices (repeated as often as it takes) each moved by up to a
quarter voxel per axis.  max_distance = the voxel size 0.02, cells of 0.04.
Library calls: device events around the call alone (its clears included), outputs in the caller's buffers, no host copy;
median / min / max of 30 after 5 warm-up calls.  transfer() and import_labels(): host clock around the session call, which
ends in its host round trip (import_labels builds and drops an index over the 1 M points inside the call, and set_manual adds
a second round trip).  For context: a3d_nearest_rows on the same vertices, 64 queries a call, and what a million queries
would take at that rate -- an EXTRAPOLATION (calls x time per call), not a measurement.  There is no CPU path: the tool
needs the GPU.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from agile3d_amd import build_model, default_args, randomize_bn_stats  # noqa: E402
from agile3d_amd import view as V  # noqa: E402
from agile3d_amd.session import InteractiveSession  # noqa: E402
from normals_timing import REPS, device_us, host_ms, scenes  # noqa: E402

VS, M = 0.02, 1_000_000


def run(ses, name, lines):
    dev = ses.device
    xyz = ses.coords_full
    n = xyz.shape[0]
    rng = np.random.default_rng(1)
    host = ses._coords_host[np.arange(M) % n] + rng.uniform(-VS / 4, VS / 4, (M, 3)).astype(np.float32)
    q = torch.from_numpy(host.astype(np.float32)).to(dev)
    labels = (torch.arange(n, device=dev) % 200).to(torch.int32)
    q_labels = (torch.arange(M, device=dev) % 200).to(torch.int32)
    cell = 2 * VS
    ws = V.point_index_workspace(n, dev)
    made = []

    def create():
        made.append(V.point_index_create(xyz, cell, workspace=ws))
        if len(made) > 1:
            made.pop(0).close()                 # (the handle only: the workspace is this tool's)
    t_create = device_us(create)
    index = made[-1]
    nearest, d2 = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, device=dev)
    out_labels, summary = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(40, dtype=torch.uint8, device=dev)
    plain = lambda: V.point_index_nearest(index, q, VS, nearest=nearest, d2=d2, summary=summary)
    carried = lambda: V.point_index_nearest(index, q, VS, labels_src=labels, nearest=nearest, d2=d2, labels=out_labels, summary=summary)
    t_plain, t_carried = device_us(plain), device_us(carried)
    s = V.read_transfer_summary(summary.cpu().numpy())
    big = V.point_index_create(q, cell)
    back, back_labels = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    t_back = device_us(lambda: V.point_index_nearest(big, xyz, VS, labels_src=q_labels, nearest=back, d2=False, labels=back_labels,
                                                     summary=summary))
    big.close()
    t_big = device_us(lambda: V.point_index_create(q, cell).close())            # (allocates its workspace inside the bracket)
    queries64 = host[:64]
    rows64 = torch.empty((1, 64), dtype=torch.int32, device=dev)
    t_rows = device_us(lambda: V.nearest_rows([xyz], queries64, out=rows64, workspace=ses._ws))
    ses.preview()
    t_transfer = host_ms(lambda: ses.transfer(q))
    t_import = host_ms(lambda: ses.import_labels(q, q_labels, into="manual"))
    lines.append(f"\n== {name}: {n} vertices; the other set: {M} points; max_distance {VS}, cell_size {cell}; of the {M} queries "
                 f"{s['matched']} matched, {s['unmatched']} not")
    lines.append(f"{'device us, median / min / max of ' + str(REPS):72s}{'median':>10s}{'min':>10s}{'max':>10s}")
    row = lambda what, t: lines.append(f"  {what:70s}{t[0]:10.1f}{t[1]:10.1f}{t[2]:10.1f}")
    row(f"a3d_point_index_create over the {n} vertices", t_create)
    row(f"a3d_point_index_nearest, {M} queries: rows and d2", t_plain)
    row(f"a3d_point_index_nearest, {M} queries: rows, d2 and labels", t_carried)
    row(f"a3d_point_index_create over the {M} points (with its allocation)", t_big)
    row(f"a3d_point_index_nearest, the {n} vertices against the {M} points", t_back)
    row("a3d_nearest_rows, 64 queries against the vertices (one call)", t_rows)
    calls = (M + 63) // 64
    lines.append(f"  EXTRAPOLATED, not measured: {calls} such calls for {M} queries = {calls * t_rows[0] / 1e6:.2f} s "
                 f"({calls * t_rows[0] / t_plain[0]:.0f} x the bulk query)")
    lines.append(f"{'host ms around the session call':72s}{'median':>10s}{'min':>10s}{'max':>10s}")
    lines.append(f"  {'transfer(1 M points), the index kept with the scene':70s}{t_transfer[0]:10.3f}{t_transfer[1]:10.3f}{t_transfer[2]:10.3f}")
    lines.append(f"  {'import_labels(1 M points, into=manual): index built and dropped':70s}{t_import[0]:10.3f}{t_import[1]:10.3f}{t_import[2]:10.3f}")
    index.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="transfer_timing.txt")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transfer_timing needs the GPU")
    torch.manual_seed(0)
    model = randomize_bn_stats(build_model(default_args(voxel_size=VS))).eval().cuda()
    lines = ["Labels to and from another point set: a3d_point_index_create, a3d_point_index_nearest (DESIGN.md 4.9, \"Labels to and "
             "from another point set\")",
             "One MI355X, one run, as measured; written by tools/transfer_timing.py (its docstring says how each number is taken).",
             "Nothing existed before: no speed was promised and no threshold is set."]
    for name, xyz, col in scenes():
        ses = InteractiveSession(model, voxel_size=VS).load_scene(xyz, col, None, name=name)
        run(ses, name, lines)
        del ses
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
