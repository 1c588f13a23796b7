#!/usr/bin/env python3
"""Stage times of one click of the headless interactive session, next to the torch / numpy recipe a user of the model API
would write around the same ``forward_mask`` (the reference's: two ``torch.cdist(...).argmin()``, ``argmax`` + per-object
overwrite, ``pred[inverse_map]``, ``.cpu().numpy()``, the per-object colour loop) -- both in ONE process and run,
alternating, on one synthetic scene (~80 k voxels, ~250 k full-resolution vertices) at 1, 5, 10 and 20 clicks.

    python tools/session_bench.py [--voxels 80000] [--reps 60] [--out profiles/session_bench.json]
                                  [--mesh-only | --render-only | --annotate-only | --edit-only | --guide-only]
                                  [--section-only [--other-lib PATH]] [--pieces-only] [--measure-only]

Every stage is timed twice: with device events around it (what the GPU spent) and with a host clock around a stage that
ends in a synchronisation (what the caller waits).  Medians over ``--reps`` clicks after a warm-up of 10.  The baseline has
no pick stage (the reference renders a depth image) and no IoU; the session's "paint + IoU" stage includes the IoU.  Needs
the GPU; there is no CPU path to time.

A last stage times the MESH pick (``a3d_pick_mesh``) next to the vertex pick (``a3d_pick_ray``) on the same vertices: a
synthetic tessellated height field of about the scene's vertex count, vertices in scan order, two triangles per cell.
Staged like ``pick`` above (the call and its small device-to-host copy, device events and host clock), and back to back
(``--mesh-calls`` calls between two events, no copy: the two kernels of a call alone), with the bytes a call must move
(12 B of indices per face + 12 B per vertex once) and the bytes it requests (12 + 36 B per face).

The RENDER stage (``a3d_render_mesh`` / ``a3d_render_points`` + ``a3d_render_shade``) draws the same height field, as a
mesh and with its vertices as a cloud, at 640 x 480 and 1280 x 720 from two cameras: one above the field looking in, one
40 cm over its middle looking along it (faces all around, across and behind the camera plane).  Per view: device events
and host clock around the render and its header copy, the same around a call whose pair capacity is 1 (it bins, counts
and stops: the cost of the binning passes before the fill), the (tile, primitive) pairs, pairs per tile, and the primitives
that went to the everywhere-list.  What to check: the whole call should cost far more than the binning -- the tile pass,
pixels x mean list length exact tests, is where the time belongs.  Every view is also shaded LIT, next to the flat shade
and on the same images: the mesh with ``a3d_render_shade_lit``, the cloud with ``a3d_render_shade_depth``; the vertex
normals (``a3d_vertex_normals``, once per scene in the session) and the host-side build of their incidence lists are timed
once for the field.  The figure to read: lit shade time against flat shade time per view, with pixels and vertices.

The ANNOTATE stage times the passes that draw the state of the annotation over those views: ``a3d_render_labels`` and
``a3d_render_annotate`` (outlines on) with 0, 20 and 256 markers, next to ``a3d_render_shade`` and the render itself on
the same images.  One launch of these sits at the floor of what a staged call measures, so every figure here is
``--mesh-calls`` calls back to back between two events, median of 5 such windows, after a warm-up window.  The vertices'
labels are stripes of five objects with background between them; the markers are vertices of the field projected by
``view.marker_table``.  The figure to read: annotate at 256 markers against the render of the same view.

The EDIT stage (``--edit-only``, a run of its own) times ``a3d_session_edit`` on the click scene, back to back like the
annotate stage: the relabel with 5, 20 and 255 objects, over the scene's own labels and over labels no object claims (the
whole table walked for every vertex), the remap of the voxel labels, and both in one call; then whole ``undo()`` /
``redo()`` calls at 20 clicks on the host clock, synchronised.  The figure to read: the relabel against 8 bytes per vertex.

The GUIDE stage (``--guide-only``, a run of its own) times ``a3d_session_guide`` on the click scene with random logits of 3, 11
and 21 columns and ten clicks, back to back like the annotate stage: its voxel pass alone (``n_full = 0``; the clear of the
summary record is part of the call) next to ``a3d_argmax_labels`` on the same logits and clicks; both passes in one call,
and the difference of the two as the full-resolution pass, next to ``a3d_session_paint`` without cubes on the same arrays.
Then, with one click on each of C - 1 objects and the model's own logits, whole ``infer()`` and ``guide()`` calls on the host
clock, synchronised.  The figures to read: the voxel pass against the arg-max (it reads the same logits and writes 16
bytes per voxel where the arg-max writes 4), the full-resolution pass against the paint (16 bytes per vertex against 16).

The PIECES stage (``--pieces-only``, a run of its own) times ``a3d_label_pieces`` and ``a3d_absorb_pieces`` on the click scene,
back to back like the annotate stage.  The model is FITTED first (``agile3d_amd.fit``: ``--fit-iters`` iterations on four
5 000-voxel synthetic scenes), three objects and the background are clicked, and the labellings are the arg-max ``infer()``
keeps and that labelling with 5 % of the rows relabelled at random (specks).  The expectation is a memory-bound pass, about
27 x 4 B of table plus the gathered keys per voxel, twice: the figure ``table_gb_s`` is 2 x 27 x 4 B x voxels over the time of
both calls.  Beside it the host time of ``pieces()``, ``despeckle()`` and the two modes of ``guide()``.

The MEASURE stage (``--measure-only``, a run of its own) times ``a3d_measure_objects`` and ``a3d_object_extents`` back to back
like the annotate stage: on the click scene's vertices and voxels with the scene's instance labels (the bench scene's rows are
shuffled, so every wave is mixed: the per-lane LDS atomics), with the same rows sorted by object (every wave carries one label:
the folded path), and with labels drawn at random over 256 ids, and on the render
stage's height field with and without its faces (objects: stripes 40 cm wide).  A vertex is 16 bytes (12 of coordinates, 4 of
label) and a face requests 48 (12 of indices, 36 of corners): the figures to read are the GB/s these give.  Beside them whole
``measure()`` calls on the host clock and what the same table costs when the labels are copied to the host and reduced there
(``measure_numpy_table``).

The SECTION stage (``--section-only``, a run of its own) times ONE view, the render stage's height field as a mesh at 640 x
480 from the outside camera, three ways that alternate call by call in one process: ``a3d_render_mesh``;
``a3d_render_mesh_section`` under ``Section.below(0)`` with back-face culling; and, with ``--other-lib``, ``a3d_render_mesh``
of another build of the library (the commit before the section: an A/B of two shared objects).  ``--reps`` calls per window,
5 windows after a warm-up window; per case the median of the window medians and their spread (largest minus smallest).
The figure to read: the difference between this build and the other one without a section, against the other one's spread."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from agile3d_amd import build_model, clicks as K, default_args, randomize_bn_stats  # noqa: E402
from agile3d_amd import view as V  # noqa: E402
from agile3d_amd.session import InteractiveSession  # noqa: E402
from agile3d_amd.synthetic import make_scene  # noqa: E402

STAGES = ("pick", "nearest", "forward_mask", "argmax", "paint_iou", "round_trip")
BASE_STAGES = ("nearest", "forward_mask", "argmax", "lift", "round_trip", "colour_loop")


class Timer:
    """Device events + host clock per named stage; a stage's host time ends in a stream synchronisation."""

    def __init__(self, names):
        self.dev = {n: [] for n in names}
        self.host = {n: [] for n in names}

    def run(self, name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        out = fn()
        b.record()
        torch.cuda.current_stream().synchronize()
        self.host[name].append(1e3 * (time.perf_counter() - t0))
        self.dev[name].append(a.elapsed_time(b))
        return out

    def medians(self, skip):
        return ({n: float(np.median(v[skip:])) for n, v in self.dev.items()},
                {n: float(np.median(v[skip:])) for n, v in self.host.items()})


def height_field(n_vertices, rng):
    """(xyz fp32, faces int32, lattice coordinates g): a tessellated height field of ~n_vertices vertices 2 cm apart,
    vertices in scan order, two triangles per cell."""
    side = int(round(np.sqrt(n_vertices)))
    g = np.arange(side, dtype=np.float64) * 0.02
    x, y = np.meshgrid(g, g, indexing="ij")
    z = 0.3 * np.sin(0.9 * x) * np.cos(0.7 * y) + rng.uniform(-0.004, 0.004, x.shape)
    xyz = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange(side * side, dtype=np.int32).reshape(side, side)
    q00, q10, q01, q11 = idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:], idx[1:, 1:]
    faces = np.stack([np.stack([q00, q10, q11], -1), np.stack([q00, q11, q01], -1)], 2).reshape(-1, 3)   # cell by cell
    return xyz, np.ascontiguousarray(faces), g


def _look_at(eye, target):
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    ext = np.eye(4)
    ext[:3, :3] = np.stack([x, np.cross(z, x), z])
    ext[:3, 3] = -ext[:3, :3] @ eye
    return ext


def render_stage(ses, n_vertices, reps, warmup):
    """The rendered view of the height field, mesh and cloud, two sizes, two cameras (see the module docstring)."""
    import ctypes as C
    from agile3d_amd import lib as L
    from agile3d_amd.session import camera_from_matrices, vertex_corner_lists
    lib, dev = ses.lib, ses.device
    xyz, faces, g = height_field(n_vertices, np.random.default_rng(1))
    xyz_dev, faces_dev = torch.from_numpy(xyz).to(dev), torch.from_numpy(faces).to(dev)
    col_dev = torch.rand((len(xyz), 3), device=dev)
    n, m = len(xyz), len(faces)
    # the normals of the field: the lists on the host (what load_scene pays once per scene), then the kernel
    t0 = time.perf_counter()
    offsets, corners = vertex_corner_lists(faces, n)
    lists_host_ms = 1e3 * (time.perf_counter() - t0)
    off_dev, cor_dev = torch.from_numpy(offsets).to(dev), torch.from_numpy(corners).to(dev)
    normals_dev = torch.empty((n, 3), dtype=torch.float32, device=dev)
    stream0 = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def normals():
        rc = lib.a3d_vertex_normals(xyz_dev.data_ptr(), n, faces_dev.data_ptr(), m, off_dev.data_ptr(), cor_dev.data_ptr(),
                                    normals_dev.data_ptr(), stream0)
        assert rc == 0, lib.a3d_last_error()

    tn = Timer(("normals",))
    for _ in range(warmup + reps):
        tn.run("normals", normals)
    normals_ms = {"device_ms": tn.medians(warmup)[0]["normals"], "host_ms": tn.medians(warmup)[1]["normals"],
                  "lists_host_ms": lists_host_ms}
    mid = 0.5 * g[-1]
    cameras = {"outside": _look_at(np.array([mid, mid - 1.0, 4.0]), np.array([mid, mid, 0.0])),
               "inside": _look_at(np.array([mid, mid, 0.4]), np.array([mid + 2.0, mid + 0.5, 0.2]))}
    header = ses._small[16:20]
    bg = np.ones(3, np.float32)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out_rows = {}
    print(f"\n== render: {n} vertices, {m} faces; median of {reps} ==")
    print(f"vertex normals {normals_ms['device_ms']:.3f}/{normals_ms['host_ms']:.3f} (device / host ms), once per scene; their "
          f"incidence lists on the host {lists_host_ms:.1f} ms")
    for w, h in ((640, 480), (1280, 720)):
        f = 0.5 * w / np.tan(np.radians(30.0))
        intr = np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1.0]])
        ids = torch.empty((h, w), dtype=torch.int32, device=dev)
        t, u, v = (torch.empty((h, w), dtype=torch.float32, device=dev) for _ in range(3))
        rgb = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        for cam_name, ext in cameras.items():
            cam = camera_from_matrices(intr, ext, w, h)
            for kind in ("mesh", "points"):
                mesh = kind == "mesh"
                n_prim = m if mesh else n
                out = L.RenderOut(ids.data_ptr(), t.data_ptr(), u.data_ptr() if mesh else None, v.data_ptr() if mesh else None,
                                  header.data_ptr())

                def call(ws):
                    if mesh:
                        rc = lib.a3d_render_mesh(xyz_dev.data_ptr(), n, faces_dev.data_ptr(), m, C.byref(cam), C.byref(out),
                                                 ws.data_ptr(), ws.numel(), stream)
                    else:
                        rc = lib.a3d_render_points(xyz_dev.data_ptr(), n, 0.02, C.byref(cam), C.byref(out), ws.data_ptr(),
                                                   ws.numel(), stream)
                    assert rc == 0, lib.a3d_last_error()
                    return header.cpu().numpy()

                def shade():
                    rc = lib.a3d_render_shade(ids.data_ptr(), u.data_ptr() if mesh else None, v.data_ptr() if mesh else None,
                                              faces_dev.data_ptr() if mesh else None, m if mesh else 0, col_dev.data_ptr(), n,
                                              bg.ctypes.data_as(C.POINTER(C.c_float)), rgb.data_ptr(), w, h, stream)
                    assert rc == 0, lib.a3d_last_error()

                def shade_lit():
                    if mesh:
                        rc = lib.a3d_render_shade_lit(ids.data_ptr(), u.data_ptr(), v.data_ptr(), faces_dev.data_ptr(), m,
                                                      col_dev.data_ptr(), n, normals_dev.data_ptr(), C.byref(cam), 0.35,
                                                      bg.ctypes.data_as(C.POINTER(C.c_float)), rgb.data_ptr(), stream)
                    else:
                        rc = lib.a3d_render_shade_depth(ids.data_ptr(), t.data_ptr(), None, None, None, 0, col_dev.data_ptr(),
                                                        n, 8.0, bg.ctypes.data_as(C.POINTER(C.c_float)), rgb.data_ptr(), w, h,
                                                        stream)
                    assert rc == 0, lib.a3d_last_error()

                tiny = torch.empty(lib.a3d_render_workspace_bytes(n_prim, w, h, 1), dtype=torch.uint8, device=dev)
                head = call(tiny)
                pairs, n_every = int(head[2:4].view(np.int64)[0]), int(head[1])
                ws = torch.empty(lib.a3d_render_workspace_bytes(n_prim, w, h, max(pairs, 1)), dtype=torch.uint8, device=dev)
                tm = Timer(("render", "binning", "shade", "shade_lit"))
                for _ in range(warmup + reps):
                    head = tm.run("render", lambda: call(ws))
                    tm.run("binning", lambda: call(tiny))
                    tm.run("shade", shade)
                    tm.run("shade_lit", shade_lit)
                assert not int(head[0]) & L.A3D_RENDER_OVERFLOW
                dev_ms, host_ms = tm.medians(warmup)
                tiles = ((w + 15) // 16) * ((h + 15) // 16)
                shown = int((ids >= 0).sum())
                key = f"{w}x{h} {cam_name} {kind}"
                out_rows[key] = {"device_ms": dev_ms, "host_ms": host_ms, "pairs": pairs, "tiles": tiles,
                                 "pairs_per_tile": pairs / tiles, "everywhere": n_every, "pixels_shown": shown,
                                 "exact_tests": (pairs / tiles + n_every) * w * h, "pixels": w * h,
                                 "lit_kernel": "a3d_render_shade_lit" if mesh else "a3d_render_shade_depth",
                                 "lit_over_flat_device": dev_ms["shade_lit"] / dev_ms["shade"]}
                print(f"{key:28s} render {dev_ms['render']:.3f}/{host_ms['render']:.3f}  binning alone {dev_ms['binning']:.3f}/"
                      f"{host_ms['binning']:.3f}  shade {dev_ms['shade']:.3f}/{host_ms['shade']:.3f}  "
                      f"{'lit' if mesh else 'depth'} shade {dev_ms['shade_lit']:.3f}/{host_ms['shade_lit']:.3f} (device / host ms)   "
                      f"pairs {pairs} = {pairs / tiles:.1f} per tile, everywhere {n_every}, {shown} of {w * h} pixels shown")
    return {"vertices": n, "faces": m, "normals": normals_ms, "views": out_rows}


def annotate_stage(ses, n_vertices, calls):
    """Label image, outlines and markers over the render stage's views (see the module docstring)."""
    import ctypes as C
    from agile3d_amd import lib as L
    from agile3d_amd import view as V
    from agile3d_amd.session import camera_from_matrices
    lib, dev = ses.lib, ses.device
    rng = np.random.default_rng(2)
    xyz, faces, g = height_field(n_vertices, np.random.default_rng(1))
    xyz_dev, faces_dev = torch.from_numpy(xyz).to(dev), torch.from_numpy(faces).to(dev)
    col_dev = torch.rand((len(xyz), 3), device=dev)
    n, m = len(xyz), len(faces)
    stripe = np.floor(xyz[:, 0] / 0.4).astype(np.int64)
    labels = np.where(stripe % 2 == 0, 1 + (stripe // 2) % 5, 0).astype(np.int32)     # objects 40 cm wide, background between
    labels_dev = torch.from_numpy(labels).to(dev)
    mid = 0.5 * g[-1]
    cameras = {"outside": _look_at(np.array([mid, mid - 1.0, 4.0]), np.array([mid, mid, 0.0])),
               "inside": _look_at(np.array([mid, mid, 0.4]), np.array([mid + 2.0, mid + 0.5, 0.2]))}
    header = ses._small[16:20]
    fp = C.POINTER(C.c_float)
    bg, black, white = (np.full(3, c, np.float32) for c in (1.0, 0.0, 1.0))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def back_to_back(fn):
        per_call = []
        for window in range(6):                     # (the first window warms up)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            per_call.append(a.elapsed_time(b) / calls)
        return float(np.median(per_call[1:]))

    rows = {}
    print(f"\n== annotate: {n} vertices, {m} faces; device ms per call, {calls} calls back to back, median of 5 windows ==")
    for w, h in ((640, 480), (1280, 720)):
        f = 0.5 * w / np.tan(np.radians(30.0))
        intr = np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1.0]])
        ids, label_img = (torch.empty((h, w), dtype=torch.int32, device=dev) for _ in range(2))
        t, u, v = (torch.empty((h, w), dtype=torch.float32, device=dev) for _ in range(3))
        rgb, rgb_out = (torch.empty((h, w, 3), dtype=torch.uint8, device=dev) for _ in range(2))
        for cam_name, ext in cameras.items():
            cam = camera_from_matrices(intr, ext, w, h)
            table = V.marker_table(cam, xyz[rng.permutation(n)[:16384]], rng.uniform(0, 1, (16384, 3)))
            table = table[(table[:, 0] >= 0) & (table[:, 0] <= w - 1) & (table[:, 1] >= 0) & (table[:, 1] <= h - 1)][:L.A3D_MAX_CLICKS]
            assert len(table) == L.A3D_MAX_CLICKS, len(table)
            table_dev = torch.from_numpy(table).to(dev)
            for kind in ("mesh", "points"):
                mesh = kind == "mesh"
                n_prim = m if mesh else n
                out = L.RenderOut(ids.data_ptr(), t.data_ptr(), u.data_ptr() if mesh else None, v.data_ptr() if mesh else None,
                                  header.data_ptr())
                up, vp, fcp, mm = (u.data_ptr(), v.data_ptr(), faces_dev.data_ptr(), m) if mesh else (None, None, None, 0)

                def render(ws):
                    if mesh:
                        rc = lib.a3d_render_mesh(xyz_dev.data_ptr(), n, faces_dev.data_ptr(), m, C.byref(cam), C.byref(out),
                                                 ws.data_ptr(), ws.numel(), stream)
                    else:
                        rc = lib.a3d_render_points(xyz_dev.data_ptr(), n, 0.02, C.byref(cam), C.byref(out), ws.data_ptr(),
                                                   ws.numel(), stream)
                    assert rc == 0, lib.a3d_last_error()

                def shade():
                    rc = lib.a3d_render_shade(ids.data_ptr(), up, vp, fcp, mm, col_dev.data_ptr(), n, bg.ctypes.data_as(fp),
                                              rgb.data_ptr(), w, h, stream)
                    assert rc == 0, lib.a3d_last_error()

                def label_image():
                    rc = lib.a3d_render_labels(ids.data_ptr(), up, vp, fcp, mm, labels_dev.data_ptr(), n, label_img.data_ptr(),
                                               w, h, stream)
                    assert rc == 0, lib.a3d_last_error()

                def annotate(k):
                    rc = lib.a3d_render_annotate(rgb.data_ptr(), label_img.data_ptr(), t.data_ptr(), table_dev.data_ptr(), k, 6.0,
                                                 4.5, 0.1, black.ctypes.data_as(fp), white.ctypes.data_as(fp), rgb_out.data_ptr(),
                                                 w, h, stream)
                    assert rc == 0, lib.a3d_last_error()

                tiny = torch.empty(lib.a3d_render_workspace_bytes(n_prim, w, h, 1), dtype=torch.uint8, device=dev)
                render(tiny)
                pairs = int(header.cpu().numpy()[2:4].view(np.int64)[0])
                ws = torch.empty(lib.a3d_render_workspace_bytes(n_prim, w, h, max(pairs, 1)), dtype=torch.uint8, device=dev)
                render(ws)
                assert not int(header.cpu()[0]) & L.A3D_RENDER_OVERFLOW
                shade(), label_image(), annotate(L.A3D_MAX_CLICKS)
                ms = {"render": back_to_back(lambda: render(ws)), "shade": back_to_back(shade), "labels": back_to_back(label_image)}
                for k in (0, 20, L.A3D_MAX_CLICKS):
                    ms[f"annotate_{k}"] = back_to_back(lambda: annotate(k))
                lab = label_img.cpu().numpy()
                drawn = int((rgb_out != rgb).any(-1).sum())
                key = f"{w}x{h} {cam_name} {kind}"
                rows[key] = {"device_ms_per_call": ms, "pixels": w * h, "pixels_labelled": int((lab >= 1).sum()),
                             "pixels_changed_at_256_markers": drawn,
                             "annotate_256_over_render": ms[f"annotate_{L.A3D_MAX_CLICKS}"] / ms["render"],
                             "marker_tests_at_256": L.A3D_MAX_CLICKS * w * h}
                print(f"{key:28s} render {ms['render']:.4f}  shade {ms['shade']:.4f}  labels {ms['labels']:.4f}  annotate with 0 / 20 / "
                      f"256 markers {ms['annotate_0']:.4f} / {ms['annotate_20']:.4f} / {ms['annotate_256']:.4f}   256 markers = "
                      f"{rows[key]['annotate_256_over_render']:.2f} x the render; {drawn} of {w * h} pixels drawn over")
    return {"vertices": n, "faces": m, "calls_back_to_back": calls, "views": rows}


def edit_stage(ses, xyz, lab, inst, calls, reps):
    """``a3d_session_edit`` on the bench scene -- the relabel with 5, 20 and 255 objects over the scene's own instance ids
    (ids the scene does not have fill the table up) and over labels no object claims (every row walks the whole table), the
    remap of the voxel labels, both in one call -- and a whole ``undo()`` / ``redo()`` at 20 clicks on the host clock."""
    import ctypes as C
    from agile3d_amd import lib as L
    lib, dev = ses.lib, ses.device
    rng = np.random.default_rng(3)
    n_full, n_qv = ses.labels_full_ori.shape[0], ses.raw_coords_qv.shape[0]
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    new_labels = torch.empty(n_full, dtype=torch.int32, device=dev)
    unclaimed = torch.full((n_full,), -5, dtype=torch.int32, device=dev)
    labels_qv = torch.from_numpy(rng.integers(0, 256, n_qv).astype(np.int32)).to(dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ids = [int(i) for i in np.unique(lab) if i > 0]
    ids += [10_000 + k for k in range(255 - len(ids))]

    def back_to_back(fn):
        per_call = []
        for window in range(6):                     # (the first window warms up)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            per_call.append(a.elapsed_time(b) / calls)
        return float(np.median(per_call[1:]))

    def launcher(relabel, remap, instances, ori):
        a = L.SessionEditArgs()
        if relabel:
            a.labels_ori_dev, a.instances_dev, a.new_labels_dev = ori.data_ptr(), instances.data_ptr(), new_labels.data_ptr()
            a.n_full, a.n_objects = n_full, instances.shape[0]
        if remap:
            a.labels_dev, a.n_labels, a.err_dev = labels_qv.data_ptr(), n_qv, err.data_ptr()
            C.memmove(a.lut, np.arange(256, dtype=np.uint8).ctypes.data, 256)       # the identity: the labels survive the repeats

        def fn():
            rc = lib.a3d_session_edit(C.byref(a), stream)
            assert rc == 0, lib.a3d_last_error()
        return fn

    print(f"\n== edit: {n_full} vertices, {n_qv} voxels; device ms per call, {calls} calls back to back, median of 5 windows ==")
    out = {"vertices": int(n_full), "voxels": int(n_qv), "calls_back_to_back": calls, "device_ms_per_call": {}}
    never = torch.empty(0)
    out["device_ms_per_call"]["remap"] = back_to_back(launcher(False, True, never, never))
    for k in (5, 20, 255):
        instances = torch.tensor(ids[:k], dtype=torch.int32, device=dev)
        ms = {"relabel": back_to_back(launcher(True, False, instances, ses.labels_full_ori)),
              "relabel_unclaimed": back_to_back(launcher(True, False, instances, unclaimed)),
              "relabel_and_remap": back_to_back(launcher(True, True, instances, ses.labels_full_ori))}
        out["device_ms_per_call"][f"objects_{k}"] = ms
        print(f"{k:3d} objects   relabel {ms['relabel']:.4f}  relabel, no label claimed {ms['relabel_unclaimed']:.4f}  "
              f"relabel + remap {ms['relabel_and_remap']:.4f}")
    print(f"remap alone   {out['device_ms_per_call']['remap']:.4f}")
    # a whole edit: 20 clicks on 5 objects, an inference, then undo() / redo() pairs on the host clock
    ses.reset()
    for k in range(20):
        ses.click(xyz[rng.choice(np.flatnonzero(lab == inst[k % 5]))], 1 + k % 5)
    ses.infer()
    host = {"undo": [], "redo": []}
    for _ in range(reps):
        for name, call in (("undo", ses.undo), ("redo", ses.redo)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assert call() is not None
            torch.cuda.synchronize()
            host[name].append(1e3 * (time.perf_counter() - t0))
    out["host_ms_at_20_clicks"] = {k: float(np.median(v[reps // 4:])) for k, v in host.items()}
    print("a whole edit at 20 clicks (host ms, synchronised): undo {undo:.3f}  redo {redo:.3f}".format(**out["host_ms_at_20_clicks"]))
    ses.reset()
    return out


def guide_stage(ses, xyz, calls, reps):
    """``a3d_session_guide`` beside ``a3d_argmax_labels`` and ``a3d_session_paint``; ``guide()`` beside ``infer()`` (see the
    module docstring)."""
    import ctypes as C
    from agile3d_amd import lib as L
    lib, dev = ses.lib, ses.device
    rng = np.random.default_rng(4)
    n_full, n_qv = ses.coords_full.shape[0], ses.raw_coords_qv.shape[0]
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lab, run, want, pred = (torch.empty(n_qv, dtype=torch.int32, device=dev) for _ in range(4))
    margin = torch.empty(n_qv, dtype=torch.float32, device=dev)
    margin_full, label_full = torch.empty(n_full, dtype=torch.float32, device=dev), torch.empty(n_full, dtype=torch.int32, device=dev)
    colors_out = torch.empty((n_full, 3), dtype=torch.float32, device=dev)
    summary = torch.empty(V.GUIDE_SUMMARY.itemsize, dtype=torch.uint8, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    click_rows = np.ascontiguousarray(rng.choice(n_qv, 10, replace=False), dtype=np.int32)

    def back_to_back(fn):
        per_call = []
        for window in range(6):                     # (the first window warms up)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            per_call.append(a.elapsed_time(b) / calls)
        return float(np.median(per_call[1:]))

    print(f"\n== guide: {n_qv} voxels, {n_full} vertices; device ms per call, {calls} calls back to back, median of 5 windows ==")
    out = {"voxels": int(n_qv), "vertices": int(n_full), "calls_back_to_back": calls, "columns": {}}
    for c in (3, 11, 21):
        logits = torch.from_numpy(rng.normal(0, 2, (n_qv, c)).astype(np.float32)).to(dev)
        click_objs = np.ascontiguousarray(rng.integers(0, c, 10), dtype=np.int32)
        ip = C.POINTER(C.c_int32)

        def argmax():
            rc = lib.a3d_argmax_labels(logits.data_ptr(), n_qv, c, click_rows.ctypes.data_as(ip), click_objs.ctypes.data_as(ip), 10,
                                       pred.data_ptr(), stream)
            assert rc == 0, lib.a3d_last_error()

        def guide_args(full):
            a = L.SessionGuideArgs()
            a.logits_dev, a.n_qv, a.n_classes = logits.data_ptr(), n_qv, c
            a.labels_qv_dev, a.runner_qv_dev, a.margin_qv_dev, a.want_qv_dev = (t.data_ptr() for t in (lab, run, margin, want))
            a.summary_dev, a.threshold, a.full_margin, a.n_clicks = summary.data_ptr(), 1.0, 4.0, 10
            a.doubt[:] = [1.0, 1.0, 1.0]
            for k in range(10):
                a.click_row[k], a.click_obj[k] = int(click_rows[k]), int(click_objs[k])
            if full:
                a.inverse_map_dev, a.n_full, a.colors_full_dev = ses.inverse_map.data_ptr(), n_full, ses.colors_full.data_ptr()
                a.palette_dev, a.n_palette = ses._palette_dev.data_ptr(), ses._palette_dev.shape[0]
                a.margin_full_dev, a.colors_out_dev = margin_full.data_ptr(), colors_out.data_ptr()

            def fn():
                rc = lib.a3d_session_guide(C.byref(a), stream)
                assert rc == 0, lib.a3d_last_error()
            return fn

        def paint():
            V.session_paint(lab, ses.inverse_map, ses.coords_full, ses.colors_full, ses._palette_dev, None, ses.cube_size,
                            labels_out=label_full, colors_out=colors_out, err=err)

        ms = {"argmax_labels": back_to_back(argmax), "guide_voxels": back_to_back(guide_args(False)),
              "guide_both": back_to_back(guide_args(True)), "session_paint": back_to_back(paint)}
        assert torch.equal(pred, lab)                   # the same labels, row for row
        ms["guide_full"] = ms["guide_both"] - ms["guide_voxels"]
        ms["voxels_over_argmax"] = ms["guide_voxels"] / ms["argmax_labels"]
        ms["full_over_paint"] = ms["guide_full"] / ms["session_paint"]
        # whole calls with the model's own logits: one click on each of c - 1 objects
        ses.reset()
        for k, row in enumerate(rng.choice(n_full, c - 1, replace=False)):
            ses.click(xyz[row], k + 1)
        host = {"infer": [], "guide": []}
        for _ in range(reps):
            for name, call in (("infer", ses.infer), ("guide", ses.guide)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                host[name].append(1e3 * (time.perf_counter() - t0))
        ms["host_ms"] = {k: float(np.median(v[reps // 4:])) for k, v in host.items()}
        out["columns"][str(c)] = ms
        print(f"C = {c:2d}   argmax {ms['argmax_labels']:.4f}  guide voxels {ms['guide_voxels']:.4f} (x{ms['voxels_over_argmax']:.2f})  "
              f"guide both {ms['guide_both']:.4f}  full pass {ms['guide_full']:.4f}  paint {ms['session_paint']:.4f} "
              f"(x{ms['full_over_paint']:.2f})   host ms: infer() {ms['host_ms']['infer']:.3f}  guide() {ms['host_ms']['guide']:.3f}")
    ses.reset()
    return out


def pieces_stage(ses, xyz, lab, inst, calls, reps):
    """``a3d_label_pieces`` and ``a3d_absorb_pieces`` on the fitted model's arg-max and on that with 5 % specks (see the module
    docstring)."""
    import ctypes as C
    from agile3d_amd import lib as L
    lib, dev = ses.lib, ses.device
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rng = np.random.default_rng(11)
    n_qv = ses.raw_coords_qv.shape[0]

    def back_to_back(fn):
        per_call = []
        for window in range(6):                     # (the first window warms up)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            per_call.append(a.elapsed_time(b) / calls)
        return float(np.median(per_call[1:]))

    ses.reset()
    for k, i in enumerate(inst[:3]):
        ses.click(xyz[np.flatnonzero(lab == i)[0]], k + 1)
    ses.click(xyz[np.flatnonzero(lab == 0)[0]], 0)
    res = ses.infer()
    argmax = ses._labels_qv.cpu().numpy()
    specks = argmax.copy()
    rows = rng.choice(n_qv, n_qv // 20, replace=False)
    specks[rows] = rng.choice(np.unique(argmax), len(rows))
    scene, clicks = ses._scene_handle(), ses._click_rows()
    capacity = 4096                                 # (what despeckle() starts with)
    ws = V.pieces_workspace(n_qv, dev, capacity, 256)
    records = torch.empty(4096 * V.PIECE.itemsize, dtype=torch.uint8, device=dev)
    count = torch.empty(2, dtype=torch.int32, device=dev)
    piece, out = torch.empty(n_qv, dtype=torch.int32, device=dev), torch.empty(n_qv, dtype=torch.int32, device=dev)
    summary = torch.empty(V.ABSORB_SUMMARY.itemsize, dtype=torch.uint8, device=dev)
    print(f"\n== pieces: {n_qv} voxels, mIoU of the fitted model's inference {res.miou:.3f}; device ms per call, {calls} calls "
          f"back to back, median of 5 windows ==")
    result = {"voxels": int(n_qv), "calls_back_to_back": calls, "miou": res.miou, "labellings": {}}
    for name, host_labels in (("argmax", argmax), ("argmax_5pct_specks", specks)):
        labels = torch.from_numpy(host_labels.astype(np.int32)).to(dev)
        entry = {}
        for c in (6, 26):
            la, ab = L.LabelPiecesArgs(), L.AbsorbPiecesArgs()          # (the arguments built once: the calls are the library's alone)
            la.scene = ab.scene = scene.handle.value
            la.n = ab.n = n_qv
            la.keys_dev = ab.labels_dev = labels.data_ptr()
            la.piece_qv_dev = ab.piece_qv_dev = piece.data_ptr()
            la.out_dev, la.max_out, la.n_out_dev = records.data_ptr(), 4096, count.data_ptr()
            la.workspace_dev = ab.workspace_dev = ws.data_ptr()
            la.workspace_bytes = ab.workspace_bytes = ws.numel()
            la.connectivity = ab.connectivity = c
            la.n_clicks = ab.n_clicks = len(clicks)
            for k, r in enumerate(clicks):
                la.click_row[k] = ab.click_row[k] = r
            ab.labels_out_dev, ab.summary_dev = out.data_ptr(), summary.data_ptr()
            ab.min_voxels, ab.n_classes, ab.capacity = 8, 256, capacity

            def label():
                rc = lib.a3d_label_pieces(C.byref(la), stream)
                assert rc == 0, lib.a3d_last_error()

            def absorb():
                rc = lib.a3d_absorb_pieces(C.byref(ab), stream)
                assert rc == 0, lib.a3d_last_error()
            ms = {"label_pieces": back_to_back(label), "absorb_pieces": back_to_back(absorb)}
            label(), absorb()
            s = V.read_absorb_summary(summary.cpu().numpy())
            assert s["err"] == 0, s
            ms.update(pieces=int(count.cpu()[0]), **{k: s[k] for k in ("small_pieces", "relabelled_pieces", "relabelled_voxels", "kept_isolated")})
            ms["table_gb_s"] = 2 * 27 * 4 * n_qv / (1e6 * (ms["label_pieces"] + ms["absorb_pieces"]))
            entry[str(c)] = ms
            print(f"{name:20s} connectivity {c:2d}   label {ms['label_pieces']:.4f}  absorb {ms['absorb_pieces']:.4f}   {ms['pieces']} pieces, "
                  f"{ms['small_pieces']} small, {ms['relabelled_voxels']} voxels relabelled   2 x 27 x 4 B x voxels = {ms['table_gb_s']:.0f} GB/s")
        result["labellings"][name] = entry
    # whole calls on the inference's own labelling (host ms, synchronised)
    host = {"pieces": [], "despeckle": [], "guide": [], "guide_connected": []}
    for _ in range(reps):
        for key, call in (("pieces", ses.pieces), ("despeckle", ses.despeckle), ("guide", ses.guide),
                          ("guide_connected", lambda: ses.guide(regions="connected"))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = call()
            torch.cuda.synchronize()
            host[key].append(1e3 * (time.perf_counter() - t0))
    result["host_ms"] = {k: float(np.median(v[reps // 4:])) for k, v in host.items()}
    result["spots"] = {"n_spots": got.n_spots, "searched": got.n_spots_searched, "contested": got.n_contested}
    print("whole calls (host ms, synchronised): " + "  ".join(f"{k}() {v:.3f}" for k, v in result["host_ms"].items()) +
          f"   guide(regions='connected'): {got.n_spots} spots over {got.n_contested} contested voxels")
    ses.reset()
    return result


def measure_numpy_table(xyz, labels, n_ids):
    """What a user writes in numpy for the same table once the labels are on the host: counts, centroid, box and covariance
    per object (float64 sums through ``np.bincount`` weights, the box through ``np.minimum.at``)."""
    p = xyz.astype(np.float64)
    count = np.bincount(labels, minlength=n_ids).astype(np.float64)
    mean = np.stack([np.bincount(labels, p[:, a], n_ids) for a in range(3)], 1) / np.maximum(count, 1)[:, None]
    c = p - mean[labels]
    cov = np.stack([np.bincount(labels, c[:, a] * c[:, b], n_ids) for a in range(3) for b in range(3)], 1) / np.maximum(count, 1)[:, None]
    lo, hi = np.full((n_ids, 3), np.inf, np.float32), np.full((n_ids, 3), -np.inf, np.float32)
    np.minimum.at(lo, labels, xyz)
    np.maximum.at(hi, labels, xyz)
    return count, mean, cov.reshape(n_ids, 3, 3), lo, hi


def measure_stage(ses, n_vertices, calls, reps):
    """``a3d_measure_objects`` and ``a3d_object_extents`` back to back on the click scene (a cloud) and on the render stage's
    height field (a mesh); whole ``measure()`` calls next to the numpy recipe (see the module docstring)."""
    lib, dev = ses.lib, ses.device
    rng = np.random.default_rng(12)

    def back_to_back(fn):
        per_call = []
        for window in range(6):                     # (the first window warms up)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            per_call.append(a.elapsed_time(b) / calls)
        return float(np.median(per_call[1:]))

    origin, quantum, bits = ses._fixed_point_frame()
    n_full, n_qv = ses.coords_full.shape[0], ses.raw_coords_qv.shape[0]
    records = torch.empty(256 * V.OBJECT_MOMENTS.itemsize, dtype=torch.uint8, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    extents = torch.empty((256, 3, 2), dtype=torch.float32, device=dev)
    axes = torch.from_numpy(np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(256)]).astype(np.float32)).to(dev)
    truth = ses.labels_full_ori % 256
    by_object = torch.argsort(truth, stable=True)      # the bench scene's rows are shuffled; a scan's are coherent: sorted by object
    labellings = {"instances": (ses.coords_full, truth, truth[ses._unique_map]),
                  "instances_rows_by_object": (ses.coords_full[by_object].contiguous(), truth[by_object].contiguous(), truth[ses._unique_map]),
                  "random_over_256": (ses.coords_full, torch.from_numpy(rng.integers(0, 256, n_full).astype(np.int32)).to(dev),
                                      torch.from_numpy(rng.integers(0, 256, n_qv).astype(np.int32)).to(dev))}
    print(f"\n== measure: {n_full} vertices, {n_qv} voxels, bits = {bits}; device ms per call, {calls} calls back to back, median of 5 "
          f"windows ==")
    out = {"vertices": int(n_full), "voxels": int(n_qv), "bits": bits, "calls_back_to_back": calls, "cloud": {}}
    for name, (coords, labels, labels_qv) in labellings.items():
        ms = {"measure_objects": back_to_back(lambda: V.measure_objects(coords, labels, origin, quantum, bits, 256,
                                                                        labels_qv=labels_qv, records=records, err=err)),
              "object_extents": back_to_back(lambda: V.object_extents(coords, labels, axes, extents=extents, err=err))}
        assert int(err.cpu()[0]) == 0
        host_labels = labels.cpu().numpy()[:n_full // 64 * 64].reshape(-1, 64)
        uniform = float((host_labels == host_labels[:, :1]).all(1).mean())
        ms["gb_s_at_16_bytes_per_vertex"] = 16 * n_full / (1e6 * ms["measure_objects"])
        ms["waves_with_one_label"] = uniform
        out["cloud"][name] = ms
        print(f"{name:24s} measure_objects {ms['measure_objects']:.4f} = {ms['gb_s_at_16_bytes_per_vertex']:.0f} GB/s at 16 B per vertex   "
              f"object_extents {ms['object_extents']:.4f}   waves with one label: {uniform:.2f}")
    # the height field: a mesh of about as many vertices, two faces per cell; objects = stripes 40 cm wide
    xyz, faces, g = height_field(n_vertices, np.random.default_rng(1))
    stripe = (np.floor(xyz[:, 0] / 0.4).astype(np.int64) % 256).astype(np.int32)
    xyz_dev, faces_dev, lab_dev = torch.from_numpy(xyz).to(dev), torch.from_numpy(faces).to(dev), torch.from_numpy(stripe).to(dev)
    centre = 0.5 * (xyz.min(0) + xyz.max(0)).astype(np.float64)
    q = 2.0 ** (int(np.ceil(np.log2(np.abs(xyz - centre).max()))) - bits)
    mesh_ms = {"without_faces": back_to_back(lambda: V.measure_objects(xyz_dev, lab_dev, centre, q, bits, 256, records=records, err=err)),
               "with_faces": back_to_back(lambda: V.measure_objects(xyz_dev, lab_dev, centre, q, bits, 256, faces=faces_dev,
                                                                    records=records, err=err))}
    assert int(err.cpu()[0]) == 0
    mesh_ms["faces_pass"] = mesh_ms["with_faces"] - mesh_ms["without_faces"]
    mesh_ms["faces_gb_s_at_48_bytes_per_face"] = 48 * len(faces) / (1e6 * mesh_ms["faces_pass"])
    waves = stripe[:len(stripe) // 64 * 64].reshape(-1, 64)
    out["mesh"] = dict(mesh_ms, vertices=len(xyz), faces=len(faces), waves_with_one_label=float((waves == waves[:, :1]).all(1).mean()))
    print(f"height field, {len(xyz)} vertices, {len(faces)} faces, waves with one label: {out['mesh']['waves_with_one_label']:.2f}   without faces {mesh_ms['without_faces']:.4f}  with faces "
          f"{mesh_ms['with_faces']:.4f}  the faces' pass {mesh_ms['faces_pass']:.4f} = {mesh_ms['faces_gb_s_at_48_bytes_per_face']:.0f} "
          f"GB/s at 48 B requested per face")
    # whole calls on the host clock, synchronised, next to: copy the labels to the host, reduce in numpy
    host = {"measure": [], "measure_oriented_false": [], "numpy_copy_and_reduce": []}
    coords_host = ses._coords_host
    for _ in range(reps):
        for key, call in (("measure", lambda: ses.measure(labels=truth)), ("measure_oriented_false", lambda: ses.measure(labels=truth, oriented=False)),
                          ("numpy_copy_and_reduce", lambda: measure_numpy_table(coords_host, truth.cpu().numpy().astype(np.int64), 256))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = call()
            torch.cuda.synchronize()
            host[key].append(1e3 * (time.perf_counter() - t0))
    out["host_ms"] = {k: float(np.median(v[reps // 4:])) for k, v in host.items()}
    m = ses.measure(labels=truth, oriented=False)
    live = m.vertices > 0
    assert np.allclose(m.centroid[live], got[1][:len(live)][live], atol=quantum) and np.array_equal(m.lo[live], got[3][:len(live)][live])
    print("whole calls (host ms, synchronised): " + "  ".join(f"{k} {v:.3f}" for k, v in out["host_ms"].items()) +
          f"   {int(live.sum())} objects")
    return out


def section_stage(ses, n_vertices, reps, other_lib):
    """One view, with and without a section, next to another build of the library (see the module docstring)."""
    import ctypes as C
    from agile3d_amd import lib as L
    from agile3d_amd.session import Section, camera_from_matrices
    lib, dev = ses.lib, ses.device
    xyz, faces, g = height_field(n_vertices, np.random.default_rng(1))
    xyz_dev, faces_dev = torch.from_numpy(xyz).to(dev), torch.from_numpy(faces).to(dev)
    n, m, (w, h) = len(xyz), len(faces), (640, 480)
    mid = 0.5 * g[-1]
    f = 0.5 * w / np.tan(np.radians(30.0))
    cam = camera_from_matrices(np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1.0]]),
                               _look_at(np.array([mid, mid - 1.0, 4.0]), np.array([mid, mid, 0.0])), w, h)
    libs = {"this build": lib}
    if other_lib:
        other = C.CDLL(other_lib)
        for name in ("a3d_render_mesh", "a3d_render_workspace_bytes", "a3d_last_error"):
            getattr(other, name).restype, getattr(other, name).argtypes = L.SYMBOLS[name]
        libs["other build"] = other
    section = Section.below(0.0, cull="back").struct()
    header = ses._small[16:20]
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    images = {}

    def images_of(case):
        if case not in images:
            images[case] = (torch.empty((h, w), dtype=torch.int32, device=dev),
                            *(torch.empty((h, w), dtype=torch.float32, device=dev) for _ in range(3)))
        return images[case]

    def call(case, ws):
        ids, t, u, v = images_of(case)
        out = L.RenderOut(ids.data_ptr(), t.data_ptr(), u.data_ptr(), v.data_ptr(), header.data_ptr())
        args = (xyz_dev.data_ptr(), n, faces_dev.data_ptr(), m, C.byref(cam))
        tail = (C.byref(out), ws.data_ptr(), ws.numel(), stream)
        if case == "section":
            rc = lib.a3d_render_mesh_section(*args, C.byref(section), *tail)
        else:
            rc = libs[case].a3d_render_mesh(*args, *tail)
        assert rc == 0, (case, lib.a3d_last_error())
        return header.cpu().numpy()

    tiny = torch.empty(lib.a3d_render_workspace_bytes(m, w, h, 1), dtype=torch.uint8, device=dev)
    pairs = int(call("this build", tiny)[2:4].view(np.int64)[0])
    ws = torch.empty(lib.a3d_render_workspace_bytes(m, w, h, max(pairs, 1)), dtype=torch.uint8, device=dev)
    cases = ["this build", "section"] + (["other build"] if other_lib else [])
    windows = {c: {"device_ms": [], "host_ms": []} for c in cases}
    for window in range(6):                         # (the first one warms up)
        tm = Timer(cases)
        for _ in range(reps):
            for c in cases:
                tm.run(c, lambda: call(c, ws))
        dev_ms, host_ms = tm.medians(0)
        if window:
            for c in cases:
                windows[c]["device_ms"].append(dev_ms[c]), windows[c]["host_ms"].append(host_ms[c])
    res = {"vertices": n, "faces": m, "view": f"{w}x{h} outside mesh", "pairs": pairs, "reps": reps, "cases": {}}
    for c in cases:
        shown = int((images_of(c)[0] >= 0).sum())
        res["cases"][c] = {k: {"median": float(np.median(v)), "spread": float(max(v) - min(v)), "windows": v}
                           for k, v in windows[c].items()}
        res["cases"][c]["pixels_shown"] = shown
    if other_lib:                                   # without a section the two builds must draw the same image
        res["same_bytes_as_other_build"] = all(torch.equal(a, b) for a, b in zip(images_of("this build"), images_of("other build")))
        assert res["same_bytes_as_other_build"]
    print(f"\n== section: {n} vertices, {m} faces, {w} x {h}, {pairs} pairs; 5 windows of {reps} calls, cases alternating ==")
    for c in cases:
        d, hh = res["cases"][c]["device_ms"], res["cases"][c]["host_ms"]
        print(f"{c:12s} device {d['median']:.4f} ms (spread {d['spread']:.4f})   host {hh['median']:.4f} ms (spread "
              f"{hh['spread']:.4f})   {res['cases'][c]['pixels_shown']} pixels shown")
    return res


def mesh_pick_stage(ses, n_vertices, reps, warmup, calls):
    """Mesh pick and vertex pick on one tessellated height field of ~n_vertices vertices (see the module docstring)."""
    import ctypes as C
    lib, dev = ses.lib, ses.device
    rng = np.random.default_rng(1)
    xyz, faces, g = height_field(n_vertices, rng)
    xyz_dev, faces_dev = torch.from_numpy(xyz).to(dev), torch.from_numpy(np.ascontiguousarray(faces)).to(dev)
    n, m = len(xyz), len(faces)
    fp = C.POINTER(C.c_float)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = ses._small

    def ray():
        tgt = np.array([rng.uniform(0.1, g[-1] - 0.1), rng.uniform(0.1, g[-1] - 0.1), 0.0])
        o = np.array([0.5 * g[-1], 0.5 * g[-1], 3.0]) + rng.uniform(-0.5, 0.5, 3)
        d = tgt - o
        return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d / np.linalg.norm(d), np.float32)

    def call_mesh(o, d):
        rc = lib.a3d_pick_mesh(xyz_dev.data_ptr(), n, faces_dev.data_ptr(), m, o.ctypes.data_as(fp), d.ctypes.data_as(fp),
                               out.data_ptr(), ses._ws.data_ptr(), ses._ws.numel(), stream)
        assert rc == 0, lib.a3d_last_error()

    def call_ray(o, d):
        rc = lib.a3d_pick_ray(xyz_dev.data_ptr(), n, o.ctypes.data_as(fp), d.ctypes.data_as(fp), 0.02, out.data_ptr(),
                              ses._ws.data_ptr(), ses._ws.numel(), stream)
        assert rc == 0, lib.a3d_last_error()

    tm = Timer(("pick_mesh", "pick_ray"))
    hits = 0
    for _ in range(warmup + reps):
        o, d = ray()
        hits += int(tm.run("pick_mesh", lambda: (call_mesh(o, d), out[:8].cpu())[1])[0]) >= 0
        tm.run("pick_ray", lambda: (call_ray(o, d), out[:4].cpu())[1])
    dev_ms, host_ms = tm.medians(warmup)
    back = {}
    for name, fn in (("pick_mesh", call_mesh), ("pick_ray", call_ray)):
        o, d = ray()
        per_call = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(calls):
                fn(o, d)
            b.record()
            torch.cuda.synchronize()
            per_call.append(a.elapsed_time(b) / calls)
        back[name] = float(np.median(per_call))
    must = {"pick_mesh": 12 * m + 12 * n, "pick_ray": 12 * n}
    asked = {"pick_mesh": 48 * m, "pick_ray": 12 * n}
    res = {"vertices": n, "faces": m, "rays_hit": hits, "rays": warmup + reps, "staged_device_ms": dev_ms,
           "staged_host_ms": host_ms, "back_to_back_device_ms": back, "calls_back_to_back": calls, "bytes_must_move": must,
           "bytes_requested": asked,
           "gbps_must_move": {k: must[k] / back[k] * 1e-6 for k in back},
           "gbps_requested": {k: asked[k] / back[k] * 1e-6 for k in back}}
    print(f"\n== mesh pick next to vertex pick: {n} vertices, {m} faces, {hits} of {warmup + reps} rays hit ==")
    for k in ("pick_mesh", "pick_ray"):
        print(f"{k}  staged {dev_ms[k]:.3f}/{host_ms[k]:.3f} (device / host ms)   back to back {1e3 * back[k]:.2f} us per call   "
              f"must move {must[k] / 1e6:.2f} MB = {res['gbps_must_move'][k]:.0f} GB/s   requests {asked[k] / 1e6:.2f} MB = "
              f"{res['gbps_requested'][k]:.0f} GB/s")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=80_000)
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mesh-calls", type=int, default=200, help="calls between two events in the mesh-pick stage")
    ap.add_argument("--mesh-only", action="store_true", help="run the mesh-pick stage alone")
    ap.add_argument("--render-only", action="store_true", help="run the render stage alone")
    ap.add_argument("--annotate-only", action="store_true", help="run the annotate stage alone")
    ap.add_argument("--edit-only", action="store_true", help="run the edit stage (a3d_session_edit, undo / redo) alone")
    ap.add_argument("--guide-only", action="store_true", help="run the guide stage (a3d_session_guide, guide()) alone")
    ap.add_argument("--pieces-only", action="store_true", help="run the pieces stage (a3d_label_pieces, a3d_absorb_pieces) alone")
    ap.add_argument("--measure-only", action="store_true", help="run the measure stage (a3d_measure_objects, a3d_object_extents) alone")
    ap.add_argument("--fit-iters", type=int, default=120, help="pieces stage: iterations the model is fitted for first")
    ap.add_argument("--section-only", action="store_true", help="run the section stage (one view with and without a section) alone")
    ap.add_argument("--other-lib", default=None, help="section stage: another build of libagile3d_hip.so to time beside this one")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("session_bench needs the GPU")
    torch.manual_seed(0)
    model = randomize_bn_stats(build_model(default_args(voxel_size=0.02))).eval().cuda()
    if a.pieces_only:
        from agile3d_amd.fit import fit, labelled_scenes
        fit(model, labelled_scenes(4, voxels=5000, objects=3), torch.device("cuda"), iters=a.fit_iters, lr=1e-3, batch=2, seed=7)
        model.eval()
    sc = make_scene(a.voxels, seed=0, voxel_size=0.02)
    rng = np.random.default_rng(0)
    raw = sc["raw_xyz"]
    xyz = np.concatenate([raw] + [raw + rng.uniform(-0.004, 0.004, raw.shape).astype(np.float32) for _ in range(2)]).astype(np.float32)
    col = np.concatenate([sc["feats"]] * 3).astype(np.float32)
    lab = np.concatenate([sc["labels"]] * 3).astype(np.int32)
    ses = InteractiveSession(model, voxel_size=0.02)
    ses.load_scene(xyz, col, lab, name="bench")
    n_full, n_qv = len(xyz), ses.raw_coords_qv.shape[0]
    print(f"scene: {n_qv} voxels, {n_full} vertices")
    inst = [i for i in np.unique(lab) if i > 0 and (lab == i).sum() > 200][:5]
    palette_host = ses.palette
    original = col.copy()
    centre = xyz.mean(0)
    result = {"voxels": int(n_qv), "vertices": int(n_full), "reps": a.reps, "warmup": a.warmup, "clicks": {}}
    alone = a.mesh_only or a.render_only or a.annotate_only or a.edit_only or a.section_only or a.guide_only or a.pieces_only or a.measure_only
    for n_clicks in (() if alone else (1, 5, 10, 20)):
        ses.reset()
        objs = [1 + (k % min(5, n_clicks)) for k in range(n_clicks)]
        targets = [xyz[rng.choice(np.flatnonzero(lab == inst[o - 1]))] for o in objs]
        for p, o in zip(targets[:-1], objs[:-1]):
            ses.click(p, o)
        base_state = ({k: list(v) for k, v in ses.click_idx.items()}, {k: list(v) for k, v in ses.click_time_idx.items()},
                      {k: list(v) for k, v in ses.click_positions.items()}, ses.num_clicks,
                      None if ses.new_labels is None else ses.new_labels.clone())
        last_obj = objs[-1]
        ts, tb = Timer(STAGES), Timer(BASE_STAGES)
        whole_s, whole_b = [], []
        for rep in range(a.warmup + a.reps):
            tgt = xyz[rng.choice(np.flatnonzero(lab == inst[last_obj - 1]))]
            direction = (tgt - (centre + np.array([0, 0, 3.0], np.float32))).astype(np.float64)
            origin = tgt - 0.5 * direction / np.linalg.norm(direction)

            def restore():
                ses.click_idx, ses.click_time_idx, ses.click_positions = ({k: list(v) for k, v in base_state[0].items()},
                                                                          {k: list(v) for k, v in base_state[1].items()},
                                                                          {k: list(v) for k, v in base_state[2].items()})
                ses.num_clicks = base_state[3]
                if base_state[4] is not None:
                    ses.new_labels = base_state[4].clone()

            # ---- the session, stage by stage (the calls click() and infer() make)
            restore()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            point = ts.run("pick", lambda: ses.pick(origin, direction))
            point = tgt if point is None else point
            q = np.asarray(point, np.float32)
            rows = ts.run("nearest", lambda: ses.nearest(q))
            key = str(last_obj)
            if key not in ses.click_idx:
                ses.click_idx[key], ses.click_time_idx[key], ses.click_positions[key] = [], [], []
                first = [ses.click_idx[str(k)][0] for k in range(1, last_obj)] + [rows[0]]      # (click(): the list's relabel)
                V.session_edit(labels_ori=ses.labels_full_ori, new_labels=ses.new_labels,
                               instances=ses.labels_qv_ori[torch.tensor(first, dtype=torch.int64, device=ses.device)])
            ses.click_idx[key].append(rows[0])
            ses.click_time_idx[key].append(ses.num_clicks)
            ses.click_positions[key].append(ses._coords_host[rows[1]].tolist())
            ses.num_clicks += 1
            logits = ts.run("forward_mask", lambda: model.forward_mask(*ses._backbone, click_idx=[ses.click_idx],
                                                                      click_time_idx=[ses.click_time_idx])["pred_masks"][0])
            labels_qv = ts.run("argmax", lambda: K.argmax_labels(logits, ses.click_idx))

            def paint_iou():
                out = ses._launch_paint(labels_qv, False)
                ses.lib.a3d_iou_counts(labels_qv.data_ptr(), labels_qv.shape[0], ses.inverse_map.data_ptr(), ses.new_labels.data_ptr(),
                                       ses.new_labels.shape[0], 256, ses._counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
                return out
            ts.run("paint_iou", paint_iou)
            ts.run("round_trip", lambda: ses._counts_host.copy_(ses._counts, non_blocking=True))
            whole_s.append(1e3 * (time.perf_counter() - t0))

            # ---- the torch / numpy recipe around the same forward_mask
            restore()
            ci = {k: list(v) for k, v in ses.click_idx.items()}
            ct = {k: list(v) for k, v in ses.click_time_idx.items()}
            torch.cuda.synchronize()
            t0 = time.perf_counter()

            def cdist2():
                p = torch.tensor([[float(v) for v in q]]).to(ses.device)
                r0 = torch.cdist(ses.raw_coords_qv, p, p=2).argmin().tolist()
                r1 = torch.cdist(ses.coords_full, p, p=2).argmin().tolist()
                return r0, ses.coords_full[r1].cpu().tolist()
            r0, _pos = tb.run("nearest", cdist2)
            ci.setdefault(key, []).append(r0)
            ct.setdefault(key, []).append(ses.num_clicks)
            blogits = tb.run("forward_mask", lambda: model.forward_mask(*ses._backbone, click_idx=[ci], click_time_idx=[ct])["pred_masks"][0])

            def argmax_overwrite():
                pred = blogits.argmax(1)
                for obj_id, cids in ci.items():
                    pred[cids] = int(obj_id)
                return pred
            pred = tb.run("argmax", argmax_overwrite)
            pred_full = tb.run("lift", lambda: pred[ses.inverse_map])
            host = tb.run("round_trip", lambda: pred_full.cpu().numpy())

            def colour_loop():
                colors = original.copy()
                for obj_id in np.unique(host):
                    if obj_id != 0:
                        colors[host == obj_id] = palette_host[obj_id]
                return colors
            tb.run("colour_loop", colour_loop)
            whole_b.append(1e3 * (time.perf_counter() - t0))
        sd, sh = ts.medians(a.warmup)
        bd, bh = tb.medians(a.warmup)
        entry = {"session_device_ms": sd, "session_host_ms": sh, "baseline_device_ms": bd, "baseline_host_ms": bh,
                 "session_click_ms": float(np.median(whole_s[a.warmup:])), "baseline_click_ms": float(np.median(whole_b[a.warmup:])),
                 "queries": n_clicks + model.num_bg_queries}
        entry["session_outside_forward_mask_host_ms"] = sum(v for k, v in sh.items() if k != "forward_mask")
        entry["baseline_outside_forward_mask_host_ms"] = sum(v for k, v in bh.items() if k != "forward_mask")
        result["clicks"][str(n_clicks)] = entry
        print(f"\n== {n_clicks} click(s), {entry['queries']} queries: median of {a.reps} ==")
        print("session   " + "  ".join(f"{k} {sd[k]:.3f}/{sh[k]:.3f}" for k in STAGES) + "   (device / host ms)")
        print("baseline  " + "  ".join(f"{k} {bd[k]:.3f}/{bh[k]:.3f}" for k in BASE_STAGES))
        print(f"outside forward_mask (host ms): session {entry['session_outside_forward_mask_host_ms']:.3f}  "
              f"baseline {entry['baseline_outside_forward_mask_host_ms']:.3f}   forward_mask {sh['forward_mask']:.3f}")
        print(f"whole click, staged (host ms): session {entry['session_click_ms']:.3f}  baseline {entry['baseline_click_ms']:.3f}")
    if a.edit_only:
        result["edit"] = edit_stage(ses, xyz, lab, inst, a.mesh_calls, a.reps)
    if a.guide_only:
        result["guide"] = guide_stage(ses, xyz, a.mesh_calls, a.reps)
    if a.pieces_only:
        result["pieces"] = pieces_stage(ses, xyz, lab, inst, a.mesh_calls, a.reps)
    if a.measure_only:
        result["measure"] = measure_stage(ses, n_full, a.mesh_calls, a.reps)
    if a.section_only:
        result["section"] = section_stage(ses, n_full, a.reps, a.other_lib)
    if not (a.render_only or a.annotate_only or a.edit_only or a.section_only or a.guide_only or a.pieces_only or a.measure_only):
        result["mesh_pick"] = mesh_pick_stage(ses, n_full, a.reps, a.warmup, a.mesh_calls)
    if not (a.mesh_only or a.annotate_only or a.edit_only or a.section_only or a.guide_only or a.pieces_only or a.measure_only):
        result["render"] = render_stage(ses, n_full, a.reps, a.warmup)
    if not (a.mesh_only or a.render_only or a.edit_only or a.section_only or a.guide_only or a.pieces_only or a.measure_only):
        result["annotate"] = annotate_stage(ses, n_full, a.mesh_calls)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
    print("RESULT " + json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
