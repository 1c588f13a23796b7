#!/usr/bin/env python3
"""Generate the fixtures of the headless interactive session by RUNNING THE REFERENCE's interactive tool.

Like ``make_goldens.py`` (whose MinkowskiEngine stub it installs) this runs only where the reference is checked out; it
imports the reference's ``interactive_tool`` package -- with stub modules for ``open3d`` and ``MinkowskiEngine`` in
``sys.modules``, neither is used by what runs here -- and holds none of its text.  What it RUNS of the reference:

  find_nearest            on the voxel rows and on the vertices, for every scripted click
  mean_iou_scene          on every inference step
  get_obj_color           ids 1..10, normalised: the palette the paint test passes in (a recorded result)
  get_next_click          ``UserInteractiveSegmentationModel.get_next_click`` called unbound on a stand-in ``self``: a model
                          stub that returns recorded logits, the reference's own ``get_colors`` bound to the stand-in,
                          no-op visualizer / data-loader stubs, and a fixed clock in place of ``datetime``.  Its
                          ``object_mask``, the colours it hands the visualizer, the record line and the contents of the
                          mask and click files are the fixtures.

The click state between the model calls (the three dictionaries, the running click count, the relabelled ground truth) is
kept by the GUI's event handler, which needs a window; the script keeps that state itself, by the rule the handler states.

Two scenes of a few thousand vertices: ``near`` (coordinates within 0-6 m) and ``far`` (the same room translated by about
50 m, one axis negative).  CONDITION ON THE CLICKS: every click written is one where the reference's ``find_nearest``
(``torch.cdist``, fp32, matrix-multiply form) equals the float64 brute-force arg-min, on the voxel rows AND on the
vertices -- asserted for every click.  A candidate that fails is dropped and redrawn; the fixture records candidates and
drops, and the script fails if more than half were dropped.

Outputs (tests/golden/): session_case_<name>.npz (arrays) and session_case_<name>.json (strings, dictionaries, counts).
"""
import argparse
import json
import os
import sys
import tempfile
import types
from datetime import datetime

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_goldens import REF, install_me_stub  # noqa: E402

VOXEL = 0.05
CLOCK = datetime(2024, 5, 17, 13, 45, 9)
SCENES = {"near": (0.0, 0.0, 0.0), "far": (50.3, -48.7, 1.2)}
# object of every click (0 = background); new ids appear in order, so no click leaves a gap
SCRIPT = [1, 2, 0, 1, 3, 2, 0, 3, 4, 1, 2, 0, 4, 3]
INFER_AFTER = (3, 6, 10, 14)          # inference runs after this many clicks
# (instance id, box centre, box half size): the vertices of an instance lie on its box's surface; instance 0 = floor
BOXES = [(7, (1.2, 1.0, 0.4), (0.45, 0.35, 0.4)), (12, (3.1, 2.2, 0.5), (0.5, 0.5, 0.5)),
         (30, (4.6, 0.9, 0.3), (0.4, 0.6, 0.3)), (41, (2.0, 3.3, 0.6), (0.3, 0.3, 0.6))]
N_FLOOR, N_BOX = 1400, 450


def install_open3d_stub():
    o3d = types.ModuleType("open3d")
    vis = types.ModuleType("open3d.visualization")
    gui = types.ModuleType("open3d.visualization.gui")
    ren = types.ModuleType("open3d.visualization.rendering")
    o3d.visualization, vis.gui, vis.rendering = vis, gui, ren
    gui.__getattr__ = lambda attr: type(attr, (), {})      # widget base classes the GUI module derives from at import
    for name, m in (("open3d", o3d), ("open3d.visualization", vis), ("open3d.visualization.gui", gui),
                    ("open3d.visualization.rendering", ren)):
        sys.modules[name] = m


def make_vertices(seed, shift):
    """coords float64 [n, 3] (float32-representable, as a scan stored in float32 is), colours float32, instance ids."""
    rng = np.random.default_rng(seed)
    pts = [np.stack([rng.uniform(0, 6, N_FLOOR), rng.uniform(0, 4, N_FLOOR), rng.normal(0, 0.004, N_FLOOR)], 1)]
    ids = [np.zeros(N_FLOOR, np.int32)]
    for inst, c, h in BOXES:
        p = rng.uniform(-1, 1, (N_BOX, 3))
        ax = rng.integers(0, 3, N_BOX)
        p[np.arange(N_BOX), ax] = np.sign(p[np.arange(N_BOX), ax])        # onto a face of the box
        pts.append(np.asarray(c) + p * np.asarray(h))
        ids.append(np.full(N_BOX, inst, np.int32))
    xyz = (np.concatenate(pts, 0) + np.asarray(shift)).astype(np.float32)
    perm = rng.permutation(len(xyz))
    ids = np.concatenate(ids)[perm]
    return xyz[perm].astype(np.float64), rng.random((len(xyz), 3), dtype=np.float32), ids


def f64_argmin(rows32, p32):
    d = ((rows32.astype(np.float64) - np.asarray(p32, np.float64)) ** 2).sum(1)
    return int(d.argmin())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    install_me_stub()
    install_open3d_stub()
    sys.path.insert(0, REF)
    sys.path.insert(0, REPO)
    import interactive_tool.interactive_segmentation_user as ref_user      # the reference
    from interactive_tool.utils import BACKGROUND_CLICK_COLOR, find_nearest, get_obj_color, mean_iou_scene
    from agile3d_amd.sparse import sparse_quantize

    class FixedClock:
        @staticmethod
        def now():
            return CLOCK

    ref_user.datetime = FixedClock
    Ref = ref_user.UserInteractiveSegmentationModel
    palette = [[0.0, 0.0, 0.0]] + [get_obj_color(k, normalize=True) for k in range(1, 11)]

    for si, (name, shift) in enumerate(SCENES.items()):
        coords, colors, inst = make_vertices(100 + si, shift)
        n = len(coords)
        _, unique_map, inverse_map = sparse_quantize(coords, quantization_size=VOXEL, return_index=True, return_inverse=True)
        coords32 = coords.astype(np.float32)
        raw_qv = torch.from_numpy(coords32[unique_map])                    # interactive_segmentation_user.py:188
        ori = torch.from_numpy(coords32)                                   # gui.py:559
        labels_full = torch.from_numpy(inst).float()
        labels_qv = labels_full[unique_map]
        n_qv = len(unique_map)
        rng = np.random.default_rng(7 + si)
        inst_of_obj = {0: 0, 1: 7, 2: 12, 3: 30, 4: 41}

        click_idx, click_time, click_pos = {"0": []}, {"0": []}, {"0": []}
        new_labels = torch.zeros(n)
        num_clicks, candidates, dropped = 0, 0, 0
        points, rows_qv, rows_full, objs = [], [], [], []
        steps = []
        tmp = tempfile.mkdtemp()
        for d in ("masks", "clicks"):
            os.makedirs(os.path.join(tmp, d))
        shown = {}
        me = types.SimpleNamespace(
            pcd_features=None, aux=None, coordinates=None, pos_encodings_pcd=None, inverse_map=torch.from_numpy(inverse_map),
            object_mask=np.zeros([n, 3]), original_colors=colors.astype(np.float64), record_file=os.path.join(tmp, "iou_record.csv"),
            mask_folder=os.path.join(tmp, "masks"), click_folder=os.path.join(tmp, "clicks"), object_name="object",
            visualizer=types.SimpleNamespace(update_colors=lambda colors: shown.__setitem__("colors", colors)),
            dataloader_test=types.SimpleNamespace(update_object=lambda *a_, **k_: None))
        me.get_colors = types.MethodType(Ref.get_colors, me)
        for obj in SCRIPT:
            while True:                                                    # draw until the reference itself is right
                candidates += 1
                v = rng.choice(np.flatnonzero(inst == inst_of_obj[obj]))
                p = (coords32[v] + rng.normal(0, 0.012, 3).astype(np.float32)).astype(np.float32)
                point = [float(x) for x in p]
                r_qv, r_full = find_nearest(raw_qv, point), find_nearest(ori, point)
                if r_qv == f64_argmin(raw_qv.numpy(), p) and r_full == f64_argmin(coords32, p):
                    break
                dropped += 1
                assert candidates < 400
            assert r_qv == f64_argmin(raw_qv.numpy(), p) and r_full == f64_argmin(coords32, p)
            key = str(obj)
            if key not in click_idx:                                       # a new object: the GUI relabels the ground truth
                click_idx[key], click_time[key], click_pos[key] = [], [], []
                new_labels[labels_full == labels_qv[r_qv]] = obj
            click_idx[key].append(r_qv)
            click_time[key].append(num_clicks)
            click_pos[key].append(ori[r_full].tolist())
            num_clicks += 1
            points.append(p), rows_qv.append(r_qv), rows_full.append(r_full), objs.append(obj)
            if num_clicks not in INFER_AFTER:
                continue
            K = len(click_idx) - 1
            g = torch.Generator().manual_seed(1000 * si + num_clicks)
            target = new_labels[unique_map].long().clamp(max=K)
            logits = 2.5 * torch.nn.functional.one_hot(target, K + 1).float() + torch.randn(n_qv, K + 1, generator=g)
            me.model = types.SimpleNamespace(forward_mask=lambda *a_, **k_: {"pred_masks": [logits.clone()]})
            before = set(os.listdir(me.mask_folder)), set(os.listdir(me.click_folder))
            Ref.get_next_click(me, click_idx=click_idx, click_time_idx=click_time, click_positions=click_pos,
                               num_clicks=num_clicks, run_model=True, gt_labels=new_labels, ori_coords=coords, scene_name=name)
            (mask_file,) = set(os.listdir(me.mask_folder)) - before[0]
            (click_file,) = set(os.listdir(me.click_folder)) - before[1]
            saved = np.load(os.path.join(me.click_folder, click_file), allow_pickle=True).item()
            mask = np.load(os.path.join(me.mask_folder, mask_file))
            assert mask.dtype == np.int64 and np.array_equal(mask, me.object_mask[:, 0].astype(np.int64))
            iou, _ = mean_iou_scene(torch.from_numpy(mask), new_labels)
            steps.append(dict(num_clicks=num_clicks, logits=logits.numpy(), mask=mask.astype(np.int32),
                              colors=np.asarray(shown["colors"]).astype(np.float32), new_labels=new_labels.numpy().astype(np.int32),
                              miou=np.float32(iou.item()), mask_file=mask_file, click_file=click_file,
                              click_idx={k: list(map(int, v_)) for k, v_ in saved["click_idx"].items()},
                              click_time={k: list(map(int, v_)) for k, v_ in saved["click_time"].items()}))
        record = open(me.record_file).read().splitlines(keepends=True)
        assert len(record) == len(steps) and 2 * dropped <= candidates, (dropped, candidates)
        arrays = dict(coords_full=coords, colors_full=colors, labels_full=inst, unique_map=unique_map.astype(np.int64),
                      inverse_map=inverse_map.astype(np.int64), click_points=np.stack(points).astype(np.float32),
                      click_rows_qv=np.array(rows_qv, np.int32), click_rows_full=np.array(rows_full, np.int32),
                      click_objs=np.array(objs, np.int32), new_labels=new_labels.numpy().astype(np.int32),
                      palette=np.array(palette, np.float32), background_click_color=np.array(BACKGROUND_CLICK_COLOR, np.float32))
        for j, s in enumerate(steps):
            for k in ("logits", "mask", "colors", "new_labels", "miou"):
                arrays[f"step{j}_{k}"] = s[k]
        np.savez_compressed(os.path.join(a.out, f"session_case_{name}.npz"), **arrays)
        meta = dict(name=name, voxel_size=VOXEL, clock=CLOCK.isoformat(), candidates=candidates, dropped=dropped,
                    click_idx=click_idx, click_time_idx=click_time, click_positions=click_pos, record=record,
                    steps=[{k: s[k] for k in ("num_clicks", "mask_file", "click_file", "click_idx", "click_time")} for s in steps])
        json.dump(meta, open(os.path.join(a.out, f"session_case_{name}.json"), "w"), indent=1, sort_keys=True)
        print(f"{name}: {n} vertices, {n_qv} voxels, {num_clicks} clicks, candidates {candidates}, dropped {dropped}")
        for ln in record:
            print("   ", ln.rstrip())


if __name__ == "__main__":
    main()
