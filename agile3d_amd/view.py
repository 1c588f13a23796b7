"""The interactive session's library calls (``csrc/session*.hip``) as functions of device tensors -- the one place where
they are marshalled, as ``clicks.py`` is for ``csrc/clicks.hip``.  ``session.py`` and the tests call these.

Every wrapper takes device tensors (or ``None`` where the C ABI takes a null pointer), checks dtype, device, shape and
contiguity (``ValueError`` naming the argument, before the library is reached), hands a tensor without elements over as a
null pointer, writes into the output tensors the caller passes (``out=``, ``rgb=``, ``header=`` ...; allocated otherwise),
launches on the current stream of the tensors' device and returns device tensors: no synchronisation, no copy to the host.
Three-vectors the C ABI reads on the host (origin, direction, background, queries) are anything ``numpy`` turns into fp32.
The ``read_*`` functions decode a result record from its host copy; ``marker_table`` projects click points to the rows
``render_annotate`` draws, on the host.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import lib as L
from ._args import F32, I32, I64, U8, _device, _out, _ptr

# the result records as numpy sees them (lib.PickResult, lib.PickMeshResult, lib.RenderHeader)
PICK = np.dtype([("index", "<i4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
PICK_MESH = np.dtype([("face", "<i4"), ("flags", "<i4"), ("t", "<f4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("u", "<f4"),
                      ("v", "<f4")])
RENDER_HEADER = np.dtype([("flags", "<i4"), ("n_everywhere", "<i4"), ("pairs_needed", "<i8")])
assert C.sizeof(L.PickResult) == PICK.itemsize == 16
assert C.sizeof(L.PickMeshResult) == PICK_MESH.itemsize == 32
assert C.sizeof(L.RenderHeader) == RENDER_HEADER.itemsize == 16


# ---- decoding: pure functions of a host array ----------------------------------------------------------------------------
def _record(host, dtype):
    """The ``dtype`` record at the front of a host buffer (of those bytes, whatever its own dtype and shape)."""
    return np.ascontiguousarray(host).view(np.uint8).reshape(-1)[:dtype.itemsize].view(dtype)[0]


def _summary_ints(host, dtype):
    """The fields of a summary record as a dict of Python ints (the padding left out)."""
    rec = _record(host, dtype)
    return {k: int(rec[k]) for k in dtype.names if k != "reserved_"}


def read_pick(host):
    """``(index, xyz fp32 [3])`` of the int32 [4] host copy of an ``a3d_pick_result`` (index -1: the ray meets no point)."""
    rec = _record(host, PICK)
    return int(rec["index"]), np.array([rec["x"], rec["y"], rec["z"]], np.float32)


def read_pick_mesh(host):
    """The ``PICK_MESH`` records of the int32 [8 k] host copy of k ``a3d_pick_mesh_result``s."""
    return np.ascontiguousarray(host).view(PICK_MESH)


def read_render_header(host):
    """``(flags, n_everywhere, pairs)`` of the int32 [4] host copy of an ``a3d_render_header``."""
    rec = _record(host, RENDER_HEADER)
    return int(rec["flags"]), int(rec["n_everywhere"]), int(rec["pairs_needed"])


# ---- argument checks (the tensor checkers are _args.py's, shared with decoder_ops.py) --------------------------------------
def _f32p(name, values, shape):
    """(array, pointer) of a small host argument; the array must outlive the call."""
    a = np.ascontiguousarray(values, dtype=np.float32)
    if a.shape != shape:
        raise ValueError(f"{name} must have shape {list(shape)}")
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def _int_in(name, value, lo, hi, message=None):
    """``int(value)`` of an integer (no bool; a float only when it is whole) in lo .. hi, else ``ValueError(message)``."""
    if isinstance(value, bool) or int(value) != value or not lo <= value <= hi:
        raise ValueError(message or f"{name} must be an integer in {lo} .. {hi}")
    return int(value)


def _summary(summary, nbytes, dev, align=8):
    summary = _out("summary", summary, U8, (nbytes,), dev)
    if summary.data_ptr() % align:
        raise ValueError(f"summary must be {align}-byte aligned")
    return summary


def _scratch(nbytes, device, refusal):
    """uint8 [nbytes] of scratch on the device; 0 is the library's "no such workspace": ``ValueError(refusal)``."""
    if nbytes == 0:
        raise ValueError(refusal)
    return torch.empty(nbytes, dtype=U8, device=device)


def _attach(a, workspace, dev, need=None, message=None):
    """The workspace into the argument block ``a``; with ``need`` (bytes) the size and the 256-byte alignment are checked."""
    a.workspace_dev, a.workspace_bytes = _ptr("workspace", workspace, U8, (None,), dev), workspace.shape[0]
    if need is not None and (a.workspace_bytes < need or workspace.data_ptr() % 256):
        raise ValueError(message)


def _wanted(a, dev, outputs):
    """The optional outputs ``(name, tensor, dtype, shape)`` of a call: ``None`` = allocated, ``False`` = not wanted (a null
    pointer, as for one without rows).  Sets ``a.<name>_dev``; returns the tensors, ``None`` for what was not wanted."""
    outs = []
    for name, t, dtype, shape in outputs:
        t = None if t is False else _out(name, t, dtype, shape, dev)
        setattr(a, name + "_dev", t.data_ptr() if t is not None and shape[0] else None)
        outs.append(t)
    return outs


def session_workspace(device):
    """The scratch of ``nearest_rows``, ``pick_ray`` and ``pick_mesh`` (``a3d_session_workspace_bytes``)."""
    return torch.empty(L.load().a3d_session_workspace_bytes(), dtype=U8, device=device)


def _workspace(ws, dev):
    if ws is None:
        return session_workspace(dev)
    _ptr("workspace", ws, U8, (None,), dev)
    return ws


def render_workspace_bytes(n_primitives, width, height, pair_capacity):
    """``a3d_render_workspace_bytes``: 0 for sizes the renders refuse."""
    return L.load().a3d_render_workspace_bytes(n_primitives, width, height, pair_capacity)


# ---- nearest rows, picks -------------------------------------------------------------------------------------------------------
def nearest_rows(sources, queries, out=None, workspace=None):
    """``a3d_nearest_rows``: fp32 [n_s, 3] row sets x host queries [m, 3] -> int32 [len(sources), m] nearest rows."""
    dev = _device("sources[0]", sources[0])
    q, qp = _f32p("queries", queries, (np.shape(queries)[0], 3))
    out = _out("out", out, I32, (len(sources), len(q)), dev)
    ws = _workspace(workspace, dev)
    src = (L.NearestSource * len(sources))()
    for i, s in enumerate(sources):
        src[i].xyz_dev, src[i].n, src[i].rows_out_dev = _ptr(f"sources[{i}]", s, F32, (None, 3), dev), s.shape[0], out[i].data_ptr()
    L.check(L.load().a3d_nearest_rows(src, len(sources), qp, len(q), ws.data_ptr(), ws.numel(), L.stream(dev)), "a3d_nearest_rows")
    return out


# The ``*_section`` calls take a ``lib.Section`` or ``None`` (the C ABI's NULL: no section).  ``_PLAIN`` stands for "the entry
# point without a section": the wrappers that have always been here keep calling exactly that.
_PLAIN = object()


def _section_ptr(section):
    if section is not None and not isinstance(section, L.Section):
        raise ValueError("section must be a lib.Section or None")
    return None if section is None else C.byref(section)


def _pick_ray(xyz, origin, direction, radius, section, out, workspace):
    dev = _device("xyz", xyz)
    xp = _ptr("xyz", xyz, F32, (None, 3), dev)
    (o, op), (d, dp) = _f32p("origin", origin, (3,)), _f32p("direction", direction, (3,))
    out = _out("out", out, I32, (4,), dev)
    ws = _workspace(workspace, dev)
    tail = (out.data_ptr(), ws.data_ptr(), ws.numel(), L.stream(dev))
    if section is _PLAIN:
        L.check(L.load().a3d_pick_ray(xp, xyz.shape[0], op, dp, float(radius), *tail), "a3d_pick_ray")
    else:
        L.check(L.load().a3d_pick_ray_section(xp, xyz.shape[0], op, dp, float(radius), _section_ptr(section), *tail),
                "a3d_pick_ray_section")
    return out


def _pick_mesh(xyz, faces, origin, direction, section, out, workspace):
    dev = _device("xyz", xyz)
    xp, fp = _ptr("xyz", xyz, F32, (None, 3), dev), _ptr("faces", faces, I32, (None, 3), dev)
    (o, op), (d, dp) = _f32p("origin", origin, (3,)), _f32p("direction", direction, (3,))
    out = _out("out", out, I32, (8,), dev)
    ws = _workspace(workspace, dev)
    tail = (out.data_ptr(), ws.data_ptr(), ws.numel(), L.stream(dev))
    if section is _PLAIN:
        L.check(L.load().a3d_pick_mesh(xp, xyz.shape[0], fp, faces.shape[0], op, dp, *tail), "a3d_pick_mesh")
    else:
        L.check(L.load().a3d_pick_mesh_section(xp, xyz.shape[0], fp, faces.shape[0], op, dp, _section_ptr(section), *tail),
                "a3d_pick_mesh_section")
    return out


def pick_ray(xyz, origin, direction, radius, out=None, workspace=None):
    """``a3d_pick_ray``: the first vertex of fp32 [n, 3] along a ray (unit ``direction``) -> int32 [4], see ``read_pick``."""
    return _pick_ray(xyz, origin, direction, radius, _PLAIN, out, workspace)


def pick_mesh(xyz, faces, origin, direction, out=None, workspace=None):
    """``a3d_pick_mesh``: the first face (int32 [m, 3] into ``xyz``) a ray crosses -> int32 [8], see ``read_pick_mesh``."""
    return _pick_mesh(xyz, faces, origin, direction, _PLAIN, out, workspace)


def pick_ray_section(xyz, origin, direction, radius, section, out=None, workspace=None):
    """``a3d_pick_ray_section``: ``pick_ray`` among the vertices on the kept side of every plane of the ``lib.Section``."""
    return _pick_ray(xyz, origin, direction, radius, section, out, workspace)


def pick_mesh_section(xyz, faces, origin, direction, section, out=None, workspace=None):
    """``a3d_pick_mesh_section``: ``pick_mesh`` with the ray cut to the section's interval and its faces culled."""
    return _pick_mesh(xyz, faces, origin, direction, section, out, workspace)


def section_ray(section, origin, direction):
    """``a3d_section_ray`` (host only, no GPU): ``(t_lo, t_hi, empty)`` -- two ``numpy.float32`` and a bool -- of a ray under
    the planes of a ``lib.Section``, by the function the kernels call."""
    (o, op), (d, dp) = _f32p("origin", origin, (3,)), _f32p("direction", direction, (3,))
    out = np.zeros(3, np.float32)
    L.check(L.load().a3d_section_ray(_section_ptr(section), op, dp, out.ctypes.data_as(C.POINTER(C.c_float))), "a3d_section_ray")
    return out[0], out[1], bool(out[2])


# ---- the rendered view -----------------------------------------------------------------------------------------------------------
def _render(xyz, faces, radius, cam, ids, t, u, v, uv, header, workspace, capacity, section=_PLAIN):
    dev = _device("xyz", xyz)
    xp = _ptr("xyz", xyz, F32, (None, 3), dev)
    mesh = faces is not None
    fp = _ptr("faces", faces, I32, (None, 3), dev) if mesh else None
    h, w = cam.height, cam.width
    ids, t = _out("ids", ids, I32, (h, w), dev), _out("t", t, F32, (h, w), dev)
    u, v = (_out("u", u, F32, (h, w), dev), _out("v", v, F32, (h, w), dev)) if uv else (None, None)
    header = _out("header", header, I32, (4,), dev)
    out = L.RenderOut(ids.data_ptr(), t.data_ptr(), u.data_ptr() if uv else None, v.data_ptr() if uv else None, header.data_ptr())
    n, m = xyz.shape[0], faces.shape[0] if mesh else xyz.shape[0]
    if workspace is None:
        workspace = torch.empty(render_workspace_bytes(m, w, h, capacity), dtype=U8, device=dev)
    _ptr("workspace", workspace, U8, (None,), dev)
    lib = L.load()
    tail = (C.byref(out), workspace.data_ptr(), workspace.numel(), L.stream(dev))
    if mesh and section is _PLAIN:
        L.check(lib.a3d_render_mesh(xp, n, fp, m, C.byref(cam), *tail), "a3d_render_mesh")
    elif mesh:
        L.check(lib.a3d_render_mesh_section(xp, n, fp, m, C.byref(cam), _section_ptr(section), *tail), "a3d_render_mesh_section")
    elif section is _PLAIN:
        L.check(lib.a3d_render_points(xp, n, float(radius), C.byref(cam), *tail), "a3d_render_points")
    else:
        L.check(lib.a3d_render_points_section(xp, n, float(radius), C.byref(cam), _section_ptr(section), *tail),
                "a3d_render_points_section")
    return ids, t, u, v, header


def render_mesh(xyz, faces, cam, ids=None, t=None, u=None, v=None, uv=True, header=None, workspace=None, capacity=1 << 16):
    """``a3d_render_mesh``, ONE attempt: ``(ids int32 [h, w], t, u, v fp32 [h, w], header int32 [4])`` for the ``lib.Camera``
    ``cam``; ``uv=False`` leaves the weights out (``u``, ``v`` come back ``None``).  ``workspace``: uint8 scratch whose size is
    the pair capacity (``render_workspace_bytes``), else one for ``capacity`` pairs is allocated.  Whether the capacity
    sufficed is in the header (``read_render_header``); the images are untouched when it did not."""
    return _render(xyz, faces, None, cam, ids, t, u, v, uv, header, workspace, capacity)


def render_points(xyz, radius, cam, ids=None, t=None, header=None, workspace=None, capacity=1 << 16):
    """``a3d_render_points``, one attempt: ``(ids, t, header)`` as ``render_mesh``, ids = vertices within ``radius``."""
    ids, t, _, _, header = _render(xyz, None, radius, cam, ids, t, None, None, False, header, workspace, capacity)
    return ids, t, header


def render_mesh_section(xyz, faces, cam, section, ids=None, t=None, u=None, v=None, uv=True, header=None, workspace=None,
                        capacity=1 << 16):
    """``a3d_render_mesh_section``: ``render_mesh`` under a ``lib.Section`` (``None``: the C ABI's NULL) -- per pixel what
    ``pick_mesh_section`` returns for the pixel's ray."""
    return _render(xyz, faces, None, cam, ids, t, u, v, uv, header, workspace, capacity, section)


def render_points_section(xyz, radius, cam, section, ids=None, t=None, header=None, workspace=None, capacity=1 << 16):
    """``a3d_render_points_section``: ``render_points`` under a ``lib.Section`` -- per pixel ``pick_ray_section``'s vertex."""
    ids, t, _, _, header = _render(xyz, None, radius, cam, ids, t, None, None, False, header, workspace, capacity, section)
    return ids, t, header


def _shade_args(ids, u, v, faces, colors, background, rgb):
    """What the three shading passes share: (device, (h, w), pointers of ids, u, v, faces, colors, m, n, background, rgb)."""
    dev = _device("ids", ids)
    ip = _ptr("ids", ids, I32, (None, None), dev)
    h, w = ids.shape
    mesh = faces is not None
    ptrs = (ip, _ptr("u", u, F32, (h, w), dev, optional=not mesh),
            _ptr("v", v, F32, (h, w), dev, optional=not mesh), _ptr("faces", faces, I32, (None, 3), dev, optional=True),
            _ptr("colors", colors, F32, (None, 3), dev))
    rgb = _out("rgb", rgb, U8, (h, w, 3), dev)
    return dev, (h, w), ptrs, faces.shape[0] if mesh else 0, colors.shape[0], _f32p("background", background, (3,)), rgb


def render_shade(ids, u, v, faces, colors, background, rgb=None):
    """``a3d_render_shade``: uint8 [h, w, 3] flat colours of an id image; ``u``, ``v``, ``faces`` ``None`` on a cloud."""
    dev, (h, w), (ip, up, vp, fp, cp), m, n, (bg, bgp), rgb = _shade_args(ids, u, v, faces, colors, background, rgb)
    L.check(L.load().a3d_render_shade(ip, up, vp, fp, m, cp, n, bgp, rgb.data_ptr(), w, h, L.stream(dev)), "a3d_render_shade")
    return rgb


def render_shade_lit(ids, u, v, faces, colors, normals, cam, ambient, background, rgb=None):
    """``a3d_render_shade_lit``: a mesh's colours lit from the camera by the vertex normals (fp32 [n, 3])."""
    dev, _, (ip, up, vp, fp, cp), m, n, (bg, bgp), rgb = _shade_args(ids, u, v, faces, colors, background, rgb)
    np_ = _ptr("normals", normals, F32, (n, 3), dev)
    L.check(L.load().a3d_render_shade_lit(ip, up, vp, fp, m, cp, n, np_, C.byref(cam), float(ambient), bgp, rgb.data_ptr(),
                                          L.stream(dev)), "a3d_render_shade_lit")
    return rgb


def render_shade_depth(ids, t, u, v, faces, colors, strength, background, rgb=None):
    """``a3d_render_shade_depth``: colours darkened by the depth steps of the ``t`` image to a pixel's four neighbours."""
    dev, (h, w), (ip, up, vp, fp, cp), m, n, (bg, bgp), rgb = _shade_args(ids, u, v, faces, colors, background, rgb)
    tp = _ptr("t", t, F32, (h, w), dev)
    L.check(L.load().a3d_render_shade_depth(ip, tp, up, vp, fp, m, cp, n, float(strength), bgp, rgb.data_ptr(), w, h,
                                            L.stream(dev)), "a3d_render_shade_depth")
    return rgb


def vertex_normals(xyz, faces, offsets, corners, out=None):
    """``a3d_vertex_normals``: fp32 [n, 3] from the incidence lists (``session.vertex_corner_lists``: int64 [n + 1], int32 [3 m])."""
    dev = _device("xyz", xyz)
    xp, fp = _ptr("xyz", xyz, F32, (None, 3), dev), _ptr("faces", faces, I32, (None, 3), dev)
    op, cp = _ptr("offsets", offsets, I64, (None,), dev), _ptr("corners", corners, I32, (None,), dev)
    n, m = xyz.shape[0], faces.shape[0]
    out = _out("out", out, F32, (n, 3), dev)
    L.check(L.load().a3d_vertex_normals(xp, n, fp, m, op, cp, out.data_ptr() if n else None, L.stream(dev)),
            "a3d_vertex_normals")
    return out


# ---- the annotation in the view ----------------------------------------------------------------------------------------------
def render_labels(ids, u, v, faces, labels, out=None):
    """``a3d_render_labels``: int32 [h, w] labels of an id image from per-vertex ``labels`` int32 [n] -- a cloud's vertex
    (``u``, ``v``, ``faces`` ``None``) or the heaviest corner of a mesh's face; -1 where the pixel shows nothing."""
    dev = _device("ids", ids)
    ip = _ptr("ids", ids, I32, (None, None), dev)
    h, w = ids.shape
    mesh = faces is not None
    up, vp = _ptr("u", u, F32, (h, w), dev, optional=not mesh), _ptr("v", v, F32, (h, w), dev, optional=not mesh)
    fp, lp = _ptr("faces", faces, I32, (None, 3), dev, optional=True), _ptr("labels", labels, I32, (None,), dev)
    m = faces.shape[0] if mesh else 0
    n = 0 if mesh and m == 0 else labels.shape[0]       # a mesh without faces: a cloud without vertices, every pixel -1
    out = _out("out", out, I32, (h, w), dev)
    L.check(L.load().a3d_render_labels(ip, up, vp, fp, m, lp, n, out.data_ptr(), w, h, L.stream(dev)), "a3d_render_labels")
    return out


def render_annotate(rgb, label_image, t, markers, radius, inner_radius, depth_slack, outline, border, out=None):
    """``a3d_render_annotate``: uint8 [h, w, 3], ``rgb`` with the objects of ``label_image`` (int32 [h, w]) outlined in
    ``outline`` (``None``: no outlines, ``label_image`` may then be ``None``) and the ``markers`` (fp32 [k, 6] on the device,
    ``marker_table``'s rows; ``None``: none) drawn over the pixels whose ``t`` lies no more than ``depth_slack`` in front of
    them.  ``out`` may be ``rgb`` itself."""
    dev = _device("rgb", rgb)
    rp = _ptr("rgb", rgb, U8, (None, None, 3), dev)
    h, w = rgb.shape[:2]
    lp = _ptr("label_image", label_image, I32, (h, w), dev, optional=outline is None)
    tp = _ptr("t", t, F32, (h, w), dev)
    mp = _ptr("markers", markers, F32, (None, 6), dev, optional=True)
    k = 0 if markers is None else markers.shape[0]
    (oa, op) = (None, None) if outline is None else _f32p("outline", outline, (3,))
    ba, bp = _f32p("border", border, (3,))
    out = _out("out", out, U8, (h, w, 3), dev)
    L.check(L.load().a3d_render_annotate(rp, lp, tp, mp, k, float(radius), float(inner_radius), float(depth_slack), op, bp,
                                         out.data_ptr(), w, h, L.stream(dev)), "a3d_render_annotate")
    return out


def marker_table(camera, points, colors, return_kept=False):
    """The rows ``(x, y, t, r, g, b)`` of ``a3d_render_annotate``'s markers for world ``points`` [k, 3] seen by the
    ``lib.Camera`` ``camera``, with ``colors`` [k, 3]: fp32 [k', 6], in the order given.  From the camera's fp32 fields,
    widened to float64: ``(a, b, c) = solve([du dv d00], p - o)``, the position ``x = a / c``, ``y = b / c`` in pixels (the
    centre of pixel (u, v) is the position (u, v)) and ``t = |p - o|``, the parameter of the pixel's unit ray at the point,
    as the render's ``t`` image holds it.  Rows with ``c <= 0`` (behind the camera) or a value that is not finite are left
    out; each value is rounded to fp32 once.  ``return_kept=True`` returns ``(rows, kept)`` with ``kept`` int64 [k'] the
    indices into ``points`` of the rows that stayed (``session.marker_hit`` names a click by them).  Pure numpy."""
    o, d00, du, dv = (np.array(f[:], np.float64) for f in (camera.o, camera.d00, camera.du, camera.dv))
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    col = np.asarray(colors, dtype=np.float64).reshape(-1, 3)
    if len(col) != len(p):
        raise ValueError("points and colors must both be [k, 3]")
    try:
        abc = np.linalg.solve(np.stack([du, dv, d00], 1), (p - o).T).T
    except np.linalg.LinAlgError:
        raise ValueError("camera: du, dv and d00 must be linearly independent") from None
    with np.errstate(all="ignore"):
        rows = np.concatenate([abc[:, :2] / abc[:, 2:], np.linalg.norm(p - o, axis=1)[:, None], col], 1).astype(np.float32)
    keep = (abc[:, 2] > 0) & np.isfinite(rows).all(1)
    rows = np.ascontiguousarray(rows[keep])
    return (rows, np.flatnonzero(keep)) if return_kept else rows


# ---- paint -------------------------------------------------------------------------------------------------------------------------
def session_paint(labels_qv, inverse_map, xyz, colors, palette, cubes, cube_size, labels_out=None, colors_out=None, err=None):
    """``a3d_session_paint``: ``(labels int32 [n], colours fp32 [n, 3], err int32 [1])`` of the n full-resolution vertices
    from the voxels' labels through ``inverse_map`` (int64 [n]), ``palette`` fp32 [K + 1, 3] and the click ``cubes`` fp32
    [k, 6] (``None``: none).  ``err`` != 0 (on the device): inverse_map or labels out of range."""
    dev = _device("labels_qv", labels_qv)
    n = inverse_map.shape[0] if torch.is_tensor(inverse_map) else 0
    a = L.SessionPaintArgs()
    a.labels_qv_dev, a.n_qv = _ptr("labels_qv", labels_qv, I32, (None,), dev), labels_qv.shape[0]
    a.inverse_map_dev, a.n_full = _ptr("inverse_map", inverse_map, I64, (None,), dev), n
    a.xyz_full_dev, a.colors_full_dev = _ptr("xyz", xyz, F32, (n, 3), dev), _ptr("colors", colors, F32, (n, 3), dev)
    a.palette_dev, a.n_palette = _ptr("palette", palette, F32, (None, 3), dev), palette.shape[0]
    a.cubes_dev, a.n_cubes = _ptr("cubes", cubes, F32, (None, 6), dev, optional=True), 0 if cubes is None else cubes.shape[0]
    a.cube_size = cube_size
    labels_out, colors_out = _out("labels_out", labels_out, I32, (n,), dev), _out("colors_out", colors_out, F32, (n, 3), dev)
    err = _out("err", err, I32, (1,), dev)
    a.label_full_dev, a.colors_out_dev, a.err_dev = labels_out.data_ptr(), colors_out.data_ptr(), err.data_ptr()
    L.check(L.load().a3d_session_paint(C.byref(a), L.stream(dev)), "a3d_session_paint")
    return labels_out, colors_out, err


# ---- edits of the click list -------------------------------------------------------------------------------------------------
def session_edit(labels_ori=None, instances=None, new_labels=None, labels=None, lut=None, err=None):
    """``a3d_session_edit``, either half or both.  Relabel (``labels_ori`` int32 [n] given): ``new_labels`` int32 [n] (``out``
    style: the caller's or a new one) = the largest k with ``instances[k - 1] == labels_ori`` (``instances`` int32 [K] on the
    device, K <= 255; ``None``: no object), else 0.  Remap (``labels`` int32 [m] given): ``labels = lut[labels]`` in place,
    ``lut`` 256 host values in 0..255; ``err`` int32 [1] != 0 (on the device): a label outside 0..255, written as 0.
    Returns ``(new_labels, labels, err)``, ``None`` for what an absent half would have given."""
    if labels_ori is None and labels is None:
        raise ValueError("session_edit: neither labels_ori (relabel) nor labels (remap) given")
    dev = _device("labels_ori" if labels_ori is not None else "labels", labels_ori if labels_ori is not None else labels)
    a = L.SessionEditArgs()
    if labels_ori is not None:
        a.labels_ori_dev, a.n_full = _ptr("labels_ori", labels_ori, I32, (None,), dev), labels_ori.shape[0]
        a.instances_dev = _ptr("instances", instances, I32, (None,), dev, optional=True)
        a.n_objects = 0 if instances is None else instances.shape[0]
        if a.n_objects > 255:
            raise ValueError("instances: at most 255 objects")
        new_labels = _out("new_labels", new_labels, I32, (a.n_full,), dev)
        a.new_labels_dev = new_labels.data_ptr() if a.n_full else None
    elif instances is not None or new_labels is not None:
        raise ValueError("instances and new_labels belong to the relabel half: labels_ori is missing")
    if labels is not None:
        a.labels_dev, a.n_labels = _ptr("labels", labels, I32, (None,), dev), labels.shape[0]
        table = np.asarray(lut)
        if table.shape != (256,) or table.dtype.kind not in "iu" or table.min() < 0 or table.max() > 255:
            raise ValueError("lut must be 256 integers in 0 .. 255")
        C.memmove(a.lut, np.ascontiguousarray(table, dtype=np.uint8).ctypes.data, 256)
        err = _out("err", err, I32, (1,), dev)
        a.err_dev = err.data_ptr()
    elif lut is not None or err is not None:
        raise ValueError("lut and err belong to the remap half: labels is missing")
    L.check(L.load().a3d_session_edit(C.byref(a), L.stream(dev)), "a3d_session_edit")
    return new_labels, labels, err


# ---- the guide: margins, the confidence view, what the cluster search takes ---------------------------------------------------
GUIDE_SUMMARY = np.dtype([("voxels", "<i4", (256,)), ("contested", "<i4", (256,)), ("least_key", "<u8"), ("err", "<i4"),
                          ("reserved_", "<i4")])
assert C.sizeof(L.SessionGuideSummary) == GUIDE_SUMMARY.itemsize == 2064
GUIDE_NAN_MARGIN, GUIDE_BAD_INDEX = 1, 2        # the bits of the summary's error word


def read_guide_summary(host):
    """The host copy of an ``a3d_session_guide_summary`` (uint8 [2064], or anything of those bytes) as a dict: ``voxels``
    and ``contested`` int64 [256] (rows and contested rows per label), ``least`` = ``(row, margin)`` of the least confident
    row -- the smallest finite margin, ties to the lowest row -- or ``None`` when no row has a finite margin, ``err`` (bit
    ``GUIDE_NAN_MARGIN``, bit ``GUIDE_BAD_INDEX``)."""
    rec = _record(host, GUIDE_SUMMARY)
    key = ~int(rec["least_key"]) & ((1 << 64) - 1)       # (stored complemented: the cleared record means "no row")
    least = None
    if key != (1 << 64) - 1:
        least = (key & 0xffffffff, float(np.array([key >> 32], np.uint32).view(np.float32)[0]))
    return {"voxels": rec["voxels"].astype(np.int64), "contested": rec["contested"].astype(np.int64), "least": least,
            "err": int(rec["err"])}


def session_guide(logits, click_rows, click_objs, threshold, inverse_map=None, colors=None, palette=None,
                  doubt_color=(1.0, 1.0, 1.0), full_margin=4.0, labels=None, runner=None, margin=None, want=None,
                  margin_full=None, colors_out=None, summary=None):
    """``a3d_session_guide``: how sure ``logits`` fp32 [n, C] (2 <= C <= 256) are, row by row.  ``click_rows`` /
    ``click_objs``: host sequences of equal length (at most ``A3D_MAX_CLICKS``; objects in 0..255), applied in order.
    ``threshold`` > 0: a row whose margin lies below it is contested.  The vertex half runs when ``colors`` fp32 [m, 3] is
    given: ``inverse_map`` int64 [m] (``None``: the identity), ``palette`` fp32 [K + 1, 3], ``doubt_color`` three numbers,
    ``full_margin`` > 0 (the margin from which a vertex shows its plain colour).  Outputs are the caller's or allocated.
    Returns ``(labels int32 [n], runner int32 [n], margin fp32 [n], want int32 [n], margin_full fp32 [m] or None, colours
    fp32 [m, 3] or None, summary uint8 [2064])`` on the device; ``read_guide_summary`` decodes the summary's host copy."""
    dev = _device("logits", logits)
    a = L.SessionGuideArgs()
    a.logits_dev = _ptr("logits", logits, F32, (None, None), dev)
    n, a.n_classes = logits.shape
    if not 2 <= a.n_classes <= 256:
        raise ValueError(f"logits must have 2 .. 256 columns, not {a.n_classes}")
    a.n_qv = n
    rows, objs = np.asarray(click_rows, dtype=np.int64).reshape(-1), np.asarray(click_objs, dtype=np.int64).reshape(-1)
    if len(rows) != len(objs) or len(rows) > L.A3D_MAX_CLICKS:
        raise ValueError(f"click_rows and click_objs must have one length, at most {L.A3D_MAX_CLICKS}")
    if len(objs) and (objs.min() < 0 or objs.max() > 255):
        raise ValueError("click_objs are object ids in 0 .. 255")
    a.n_clicks = len(rows)
    for k, (r, o) in enumerate(zip(rows.tolist(), objs.tolist())):
        a.click_row[k], a.click_obj[k] = (r if -1 <= r < 1 << 31 else -1), o     # (a row no int32 holds is a row outside)
    threshold, full_margin = float(threshold), float(full_margin)
    f32 = np.float32
    with np.errstate(over="ignore"):
        if not (np.isfinite(f32(threshold)) and f32(threshold) > 0 and np.isfinite(f32(full_margin)) and f32(full_margin) > 0):
            raise ValueError("threshold and full_margin must be finite and > 0 (in fp32)")
    a.threshold, a.full_margin = threshold, full_margin
    labels, runner = _out("labels", labels, I32, (n,), dev), _out("runner", runner, I32, (n,), dev)
    margin, want = _out("margin", margin, F32, (n,), dev), _out("want", want, I32, (n,), dev)
    a.labels_qv_dev, a.runner_qv_dev = labels.data_ptr() if n else None, runner.data_ptr() if n else None
    a.margin_qv_dev, a.want_qv_dev = margin.data_ptr() if n else None, want.data_ptr() if n else None
    if colors is not None:
        m = colors.shape[0] if torch.is_tensor(colors) and colors.dim() == 2 else 0
        a.n_full = m
        a.colors_full_dev = _ptr("colors", colors, F32, (None, 3), dev)
        a.inverse_map_dev = _ptr("inverse_map", inverse_map, I64, (m,), dev, optional=True)
        a.palette_dev = _ptr("palette", palette, F32, (None, 3), dev)
        a.n_palette = palette.shape[0]
        if not 2 <= a.n_palette <= 256:
            raise ValueError("palette must be [K + 1, 3] with 1 <= K <= 255")
        a.doubt[:] = [float(x) for x in _f32p("doubt_color", doubt_color, (3,))[0]]
        margin_full, colors_out = _out("margin_full", margin_full, F32, (m,), dev), _out("colors_out", colors_out, F32, (m, 3), dev)
        a.margin_full_dev, a.colors_out_dev = (margin_full.data_ptr(), colors_out.data_ptr()) if m else (None, None)
    elif inverse_map is not None or margin_full is not None or colors_out is not None:
        raise ValueError("inverse_map, margin_full and colors_out belong to the vertex half: colors is missing")
    summary = _summary(summary, GUIDE_SUMMARY.itemsize, dev)
    a.summary_dev = summary.data_ptr()
    L.check(L.load().a3d_session_guide(C.byref(a), L.stream(dev)), "a3d_session_guide")
    return labels, runner, margin, want, margin_full, colors_out, summary


# ---- the pieces of a labelling, despeckle --------------------------------------------------------------------------------------
PIECE = np.dtype([("root", "<i4"), ("key", "<i4"), ("voxels", "<i4"), ("clicked", "<i4"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,))])
ABSORB_SUMMARY = np.dtype([("small_pieces", "<i4"), ("relabelled_pieces", "<i4"), ("relabelled_voxels", "<i4"),
                           ("kept_isolated", "<i4"), ("err", "<i4"), ("reserved_", "<i4", (3,))])
assert C.sizeof(L.Piece) == PIECE.itemsize == 40
assert C.sizeof(L.AbsorbSummary) == ABSORB_SUMMARY.itemsize == 32
PIECES_BAD_INDEX = 1                            # the bit of a3d_label_pieces' error word
ABSORB_OVERFLOW, ABSORB_BAD_LABEL = 1, 2        # the bits of the absorb summary's error word
CONNECTIVITIES = (6, 18, 26)


def read_pieces(records_host, count_host):
    """``(records, n_pieces, err)`` of the host copies of ``label_pieces``' record buffer (uint8, 40 bytes a record) and its
    int32 [2] count: the ``PIECE`` records that were written (at most the buffer's, in ascending root), the TRUE number of
    pieces, the error word (bit ``PIECES_BAD_INDEX``)."""
    count = np.ascontiguousarray(count_host).view(np.int32).reshape(-1)
    raw = np.ascontiguousarray(records_host).view(np.uint8).reshape(-1)
    n = int(count[0])
    kept = min(n, len(raw) // PIECE.itemsize)
    return raw[:kept * PIECE.itemsize].view(PIECE).copy(), n, int(count[1])


def read_absorb_summary(host):
    """The host copy of an ``a3d_absorb_summary`` (uint8 [32], or anything of those bytes) as a dict of Python ints:
    ``small_pieces`` (on ``ABSORB_OVERFLOW`` the capacity needed), ``relabelled_pieces``, ``relabelled_voxels``,
    ``kept_isolated``, ``err`` (bits ``ABSORB_OVERFLOW``, ``ABSORB_BAD_LABEL``)."""
    return _summary_ints(host, ABSORB_SUMMARY)


def pieces_workspace(n, device, capacity=None, n_classes=256):
    """The scratch of ``label_pieces`` for n voxels (``a3d_pieces_workspace_bytes``); with ``capacity`` also room for
    ``absorb_pieces`` with that many small pieces and ``n_classes`` labels (``a3d_absorb_workspace_bytes``)."""
    lib = L.load()
    nbytes = lib.a3d_pieces_workspace_bytes(n) if capacity is None else lib.a3d_absorb_workspace_bytes(n, capacity, n_classes)
    return _scratch(nbytes, device, f"no pieces workspace for n={n} capacity={capacity} n_classes={n_classes}")


def _scene_rows(scene):
    if getattr(scene, "handle", None) is None or not getattr(scene, "n", None):
        raise ValueError("scene must be an engine.Scene")
    return getattr(scene.handle, "value", scene.handle), scene.n[0]


def _connectivity(connectivity):
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"connectivity must be one of {CONNECTIVITIES}, not {connectivity!r}")
    return int(connectivity)


def _click_rows(dst, click_rows):
    rows = np.asarray(click_rows, dtype=np.int64).reshape(-1)
    if len(rows) > L.A3D_MAX_CLICKS:
        raise ValueError(f"click_rows: at most {L.A3D_MAX_CLICKS}")
    for k, r in enumerate(rows.tolist()):
        dst[k] = r if -1 <= r < 1 << 31 else -1               # (a row no int32 holds is a row outside)
    return len(rows)


def _pieces_outputs(a, n, dev, connectivity, click_rows, inverse_map, piece_qv, piece_full, records, count, workspace):
    """What ``label_pieces`` and ``similar_pieces`` share, written into either argument block: the connectivity, the clicked
    rows, the lift, the outputs (the caller's, checked, or new ones) and the workspace.  Returns ``(piece_qv, piece_full,
    records, count, workspace)``."""
    a.connectivity = _connectivity(connectivity)
    a.n_clicks = _click_rows(a.click_row, click_rows)
    piece_qv = _out("piece_qv", piece_qv, I32, (n,), dev)
    a.piece_qv_dev = piece_qv.data_ptr()
    if inverse_map is not None:
        a.inverse_map_dev = _ptr("inverse_map", inverse_map, I64, (None,), dev)
        a.n_full = inverse_map.shape[0]
        piece_full = _out("piece_full", piece_full, I32, (a.n_full,), dev)
        a.piece_full_dev = piece_full.data_ptr() if a.n_full else None
    elif piece_full is not None:
        raise ValueError("piece_full belongs to the lift: inverse_map is missing")
    if records is None:
        records = torch.empty(1024 * PIECE.itemsize, dtype=U8, device=dev)
    _ptr("records", records, U8, (None,), dev)
    if records.data_ptr() % 4:
        raise ValueError("records must be 4-byte aligned")
    a.max_out = min(records.shape[0] // PIECE.itemsize, (1 << 31) - 1)
    a.out_dev = records.data_ptr() if a.max_out else None
    count = _out("count", count, I32, (2,), dev)
    a.n_out_dev = count.data_ptr()
    if workspace is None:
        workspace = pieces_workspace(n, dev)
    _attach(a, workspace, dev)                  # (the library checks the size: a vote's workspace is one as well)
    return piece_qv, piece_full, records, count, workspace


def label_pieces(scene, keys, connectivity=26, click_rows=(), inverse_map=None, piece_qv=None, piece_full=None, records=None,
                 count=None, workspace=None):
    """``a3d_label_pieces``: the connected pieces of ``keys`` int32 [n] (the rows of ``scene``, an ``engine.Scene``, in the
    caller's order; a negative key belongs to no piece) under ``connectivity`` 6, 18 or 26.  ``click_rows``: a host sequence
    of at most ``A3D_MAX_CLICKS`` rows.  ``inverse_map`` int64 [m]: also lift the pieces to m vertices.  ``records``: a uint8
    buffer of 40 bytes per record the call may write (default: room for 1024); ``count`` int32 [2]; ``workspace``:
    ``pieces_workspace``.  Returns ``(piece_qv int32 [n], piece_full int32 [m] or None, records, count, workspace)`` on the
    device; ``read_pieces`` decodes the host copies of the last two."""
    dev = _device("keys", keys)
    handle, n = _scene_rows(scene)
    a = L.LabelPiecesArgs()
    a.scene, a.n = handle, n
    a.keys_dev = _ptr("keys", keys, I32, (n,), dev)
    outs = _pieces_outputs(a, n, dev, connectivity, click_rows, inverse_map, piece_qv, piece_full, records, count, workspace)
    L.check(L.load().a3d_label_pieces(C.byref(a), L.stream(dev)), "a3d_label_pieces")
    return outs


def absorb_pieces(scene, labels, piece_qv, workspace, min_voxels, connectivity=26, click_rows=(), n_classes=256, capacity=1024,
                  labels_out=None, summary=None):
    """``a3d_absorb_pieces``: one despeckle step on ``labels`` int32 [n] in 0..n_classes-1.  ``piece_qv`` and ``workspace``:
    what ``label_pieces`` returned for ``keys = labels`` under the same ``connectivity`` (the workspace holds the pieces'
    sizes; it must be a ``pieces_workspace(n, device, capacity, n_classes)``).  A piece of fewer than ``min_voxels`` voxels
    without a clicked row takes the label most of its differently labelled neighbour pairs vote for.  Returns ``(labels_out
    int32 [n], summary uint8 [32])`` on the device; ``read_absorb_summary`` decodes the summary's host copy -- on
    ``ABSORB_OVERFLOW`` nothing was written to ``labels_out`` and ``small_pieces`` is the capacity to call again with."""
    dev = _device("labels", labels)
    handle, n = _scene_rows(scene)
    a = L.AbsorbPiecesArgs()
    a.scene, a.n = handle, n
    a.labels_dev = _ptr("labels", labels, I32, (n,), dev)
    a.piece_qv_dev = _ptr("piece_qv", piece_qv, I32, (n,), dev)
    a.connectivity = _connectivity(connectivity)
    a.n_clicks = _click_rows(a.click_row, click_rows)
    a.min_voxels = _int_in("min_voxels", min_voxels, 0, (1 << 31) - 1)
    a.n_classes, a.capacity = _int_in("n_classes", n_classes, 1, 256), _int_in("capacity", capacity, 0, (1 << 31) - 1)
    labels_out = _out("labels_out", labels_out, I32, (n,), dev)
    if n and labels_out.data_ptr() == labels.data_ptr():
        raise ValueError("labels_out may not alias labels")
    a.labels_out_dev = labels_out.data_ptr()
    summary = _summary(summary, ABSORB_SUMMARY.itemsize, dev, 4)
    a.summary_dev = summary.data_ptr()
    _attach(a, workspace, dev, L.load().a3d_absorb_workspace_bytes(n, a.capacity, a.n_classes),
            "workspace too small for this capacity and n_classes (pieces_workspace(n, device, capacity, n_classes))")
    L.check(L.load().a3d_absorb_pieces(C.byref(a), L.stream(dev)), "a3d_absorb_pieces")
    return labels_out, summary


# ---- smooth patches, the magic wand, the snap --------------------------------------------------------------------------------
VOTE_SUMMARY = np.dtype([("eligible_pieces", "<i4"), ("uniform_pieces", "<i4"), ("relabelled_pieces", "<i4"),
                         ("relabelled_voxels", "<i4"), ("blocked_pieces", "<i4"), ("below_share_pieces", "<i4"), ("err", "<i4"),
                         ("reserved_", "<i4")])
assert C.sizeof(L.VoteSummary) == VOTE_SUMMARY.itemsize == 32
assert C.sizeof(L.SimilarPiecesArgs) == 1192 and C.sizeof(L.VotePiecesArgs) == 1112
SIMILAR_REF_NORMAL, SIMILAR_REF_FEAT = L.A3D_SIMILAR_REF_NORMAL, L.A3D_SIMILAR_REF_FEAT
VOTE_OVERFLOW, VOTE_BAD_LABEL = L.A3D_VOTE_OVERFLOW, L.A3D_VOTE_BAD_LABEL      # the bits of the vote summary's error word
VOTE_MAX_DEN = 1 << 16


def read_vote_summary(host):
    """The host copy of an ``a3d_vote_summary`` (uint8 [32], or anything of those bytes) as a dict of Python ints:
    ``eligible_pieces`` (on ``VOTE_OVERFLOW`` the capacity needed), ``uniform_pieces``, ``relabelled_pieces``,
    ``relabelled_voxels``, ``blocked_pieces``, ``below_share_pieces``, ``err`` (bits ``VOTE_OVERFLOW``, ``VOTE_BAD_LABEL``)."""
    return _summary_ints(host, VOTE_SUMMARY)


def vote_workspace(n, device, capacity, n_classes=256):
    """The scratch of ``label_pieces`` / ``similar_pieces`` for n voxels with room behind it for ``vote_pieces`` with
    ``capacity`` eligible pieces and ``n_classes`` labels (``a3d_vote_workspace_bytes``)."""
    return _scratch(L.load().a3d_vote_workspace_bytes(n, capacity, n_classes), device,
                    f"no vote workspace for n={n} capacity={capacity} n_classes={n_classes}")


def _cosine(name, value):
    with np.errstate(over="ignore"):
        value = float(np.float32(value))
    if not (np.isfinite(value) and -1.0 <= value <= 1.0):
        raise ValueError(f"{name} must be a finite cosine in [-1, 1], not {value!r}")
    return value


def _tolerance2(name, value):
    with np.errstate(over="ignore"):
        value = float(np.float32(value))
    if not (np.isfinite(value) and value >= 0.0):
        raise ValueError(f"{name} must be finite and >= 0, not {value!r}")
    return value


def _reference(name, value):
    a = np.asarray(value, dtype=np.float32).reshape(-1)
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError(f"{name} must be three finite values")
    return [float(x) for x in a]


def similar_settings(cos_min=1.0, tol2=0.0, oriented=False, ref_normal=None, ref_cos_min=1.0, ref_feat=None, ref_tol2=0.0):
    """The by-value settings of ``a3d_similar_pieces`` checked on the host as the library checks them: ``(cos_min, tol2,
    oriented, ref_flags, ref_normal, ref_cos_min, ref_feat, ref_tol2)``.  Cosines finite in [-1, 1], squared tolerances
    finite and >= 0 (as fp32), ``oriented`` a bool or 0 / 1, a reference three finite values or ``None`` (its bit of
    ``ref_flags`` then stays clear).  ``ValueError`` naming the argument.  Pure Python."""
    if oriented not in (False, True, 0, 1):
        raise ValueError("oriented must be a bool")
    flags = (SIMILAR_REF_NORMAL if ref_normal is not None else 0) | (SIMILAR_REF_FEAT if ref_feat is not None else 0)
    return (_cosine("cos_min", cos_min), _tolerance2("tol2", tol2), int(bool(oriented)), flags,
            _reference("ref_normal", ref_normal) if ref_normal is not None else [0.0] * 3, _cosine("ref_cos_min", ref_cos_min),
            _reference("ref_feat", ref_feat) if ref_feat is not None else [0.0] * 3, _tolerance2("ref_tol2", ref_tol2))


def similar_pair(normal_a=None, normal_b=None, feat_a=None, feat_b=None, cos_min=1.0, tol2=0.0, oriented=False):
    """``a3d_similar_pair`` (host only, no GPU): whether the pair predicate of ``a3d_similar_pieces`` joins two voxels with
    these normals (fp32 [3] each, or both ``None``: no normal test) and colours (the same) -- evaluated by the function the
    kernel calls.  The admissibility test is the same call with the reference as ``b``.  NaNs and zeros are passed on as
    they are; the thresholds are checked as ``similar_settings`` checks them."""
    cos_min, tol2, oriented = similar_settings(cos_min, tol2, oriented)[:3]
    if (normal_a is None) != (normal_b is None) or (feat_a is None) != (feat_b is None):
        raise ValueError("normal_a / normal_b and feat_a / feat_b are given or left out in pairs")
    keep, ptrs = [], []
    for name, v in (("normal_a", normal_a), ("normal_b", normal_b), ("feat_a", feat_a), ("feat_b", feat_b)):
        a, p = _f32p(name, v, (3,)) if v is not None else (None, None)
        keep.append(a), ptrs.append(p)
    got = L.load().a3d_similar_pair(*ptrs, cos_min, tol2, oriented)
    if got not in (0, 1):
        raise L.A3DError("a3d_similar_pair refused its arguments")
    return bool(got)


def similar_pieces(scene, keys=None, normals=None, feats=None, cos_min=1.0, tol2=0.0, oriented=False, ref_normal=None,
                   ref_cos_min=1.0, ref_feat=None, ref_tol2=0.0, connectivity=26, click_rows=(), inverse_map=None, piece_qv=None,
                   piece_full=None, records=None, count=None, workspace=None):
    """``a3d_similar_pieces``: the connected pieces of the voxels of ``scene`` (an ``engine.Scene``; n rows in the caller's
    order) under a SIMILARITY: two neighbours under ``connectivity`` are joined when they hold the same key (``keys`` int32
    [n], ``None``: all 0; a negative key belongs to no piece), their ``normals`` fp32 [n, 3] have ``|dot| >= cos_min`` (``dot``
    with ``oriented``) and their ``feats`` fp32 [n, 3] a squared distance ``<= tol2`` -- each test only when its array is given.
    ``ref_normal`` / ``ref_feat`` (three values, with ``ref_cos_min`` / ``ref_tol2``): only the rows that pass the same test
    against this reference take part at all; a reference needs its array.  Everything else -- ``click_rows``,
    ``inverse_map``, ``records``, ``count``, ``workspace`` and the return value ``(piece_qv, piece_full, records, count,
    workspace)`` -- is ``label_pieces``'; ``read_pieces`` decodes the host copies of the last two."""
    handle, n = _scene_rows(scene)
    settings = similar_settings(cos_min, tol2, oriented, ref_normal, ref_cos_min, ref_feat, ref_tol2)
    if (ref_normal is not None and normals is None) or (ref_feat is not None and feats is None):
        raise ValueError("a reference needs its array: ref_normal goes with normals, ref_feat with feats")
    connectivity = _connectivity(connectivity)
    first = next((t for t in (keys, normals, feats, piece_qv, workspace) if t is not None), None)
    dev = _device("keys", first) if first is not None else _device("scene", getattr(scene, "workspace", None))
    a = L.SimilarPiecesArgs()
    a.scene, a.n = handle, n
    a.keys_dev = _ptr("keys", keys, I32, (n,), dev, optional=True)
    a.normal_qv_dev = _ptr("normals", normals, F32, (n, 3), dev, optional=True)
    a.feat_qv_dev = _ptr("feats", feats, F32, (n, 3), dev, optional=True)
    a.cos_min, a.tol2, a.oriented, a.ref_flags = settings[:4]
    a.ref_normal[:], a.ref_cos_min, a.ref_feat[:], a.ref_tol2 = settings[4:]
    outs = _pieces_outputs(a, n, dev, connectivity, click_rows, inverse_map, piece_qv, piece_full, records, count, workspace)
    L.check(L.load().a3d_similar_pieces(C.byref(a), L.stream(dev)), "a3d_similar_pieces")
    return outs


def vote_settings(min_voxels, share, n_classes=256, capacity=1024):
    """``(min_voxels, share_num, share_den, n_classes, capacity)`` as ``a3d_vote_pieces`` takes them, checked on the host:
    ``min_voxels`` an integer >= 1, ``share`` a pair of integers with ``1 <= num <= den <= 65536``, ``n_classes`` in 1 .. 256,
    ``capacity`` an integer >= 0.  ``ValueError`` naming the argument.  Pure Python."""
    try:
        num, den = share
    except (TypeError, ValueError):
        raise ValueError("share must be a pair of integers (num, den)") from None
    settings = tuple(_int_in(name, value, lo, hi) for name, value, lo, hi in (
        ("min_voxels", min_voxels, 1, (1 << 31) - 1), ("share numerator", num, 1, VOTE_MAX_DEN),
        ("share denominator", den, 1, VOTE_MAX_DEN), ("n_classes", n_classes, 1, 256), ("capacity", capacity, 0, (1 << 31) - 1)))
    if num > den:
        raise ValueError("share must be at most 1: num <= den")
    return settings


def vote_pieces(scene, labels, piece_qv, workspace, min_voxels=8, share=(2, 3), click_rows=(), n_classes=256, capacity=1024,
                labels_out=None, summary=None):
    """``a3d_vote_pieces``: snaps ``labels`` int32 [n] in 0..n_classes-1 to a partition.  ``piece_qv`` and ``workspace``: what
    ``label_pieces`` or ``similar_pieces`` returned for this scene (the workspace holds the pieces' sizes; it must be a
    ``vote_workspace(n, device, capacity, n_classes)``).  Every piece of at least ``min_voxels`` voxels whose most frequent
    label (ties: the lowest) holds at least ``share = (num, den)`` of its voxels, and which holds no clicked row of another
    label, gives all its voxels that label; everything else is copied.  Returns ``(labels_out int32 [n], summary uint8
    [32])`` on the device; ``read_vote_summary`` decodes the summary's host copy -- on ``VOTE_OVERFLOW`` nothing was written
    to ``labels_out`` and ``eligible_pieces`` is the capacity to call again with."""
    settings = vote_settings(min_voxels, share, n_classes, capacity)
    handle, n = _scene_rows(scene)
    dev = _device("labels", labels)
    a = L.VotePiecesArgs()
    a.scene, a.n = handle, n
    a.labels_dev = _ptr("labels", labels, I32, (n,), dev)
    a.piece_qv_dev = _ptr("piece_qv", piece_qv, I32, (n,), dev)
    a.n_clicks = _click_rows(a.click_row, click_rows)
    a.min_voxels, a.share_num, a.share_den, a.n_classes, a.capacity = settings
    labels_out = _out("labels_out", labels_out, I32, (n,), dev)
    if n and labels_out.data_ptr() == labels.data_ptr():
        raise ValueError("labels_out may not alias labels")
    a.labels_out_dev = labels_out.data_ptr()
    summary = _summary(summary, VOTE_SUMMARY.itemsize, dev, 4)
    a.summary_dev = summary.data_ptr()
    _attach(a, workspace, dev, L.load().a3d_vote_workspace_bytes(n, a.capacity, a.n_classes),
            "workspace too small or not 256-byte aligned (vote_workspace(n, device, capacity, n_classes))")
    L.check(L.load().a3d_vote_pieces(C.byref(a), L.stream(dev)), "a3d_vote_pieces")
    return labels_out, summary


# ---- growing a selection along the surface ------------------------------------------------------------------------------------
GROW_SUMMARY = np.dtype([("seeds", "<i8"), ("reached", "<i8"), ("selected", "<i8"), ("max_dist", "<i4"), ("err", "<i4")])
assert C.sizeof(L.GrowSummary) == GROW_SUMMARY.itemsize == 32
assert C.sizeof(L.GrowVoxelsArgs) == 136
GROW_BAD_INDEX = L.A3D_GROW_BAD_INDEX           # the bit of the grow summary's error word
GROW_MAX_STEPS = L.A3D_GROW_MAX_STEPS
GROW_METRIC_COST = (1024, 1448, 1774)           # round(1024 * (1, sqrt 2, sqrt 3)): face, edge, corner steps in 1/1024 voxel
GROW_MAX_COST, GROW_MAX_LIMIT = 1 << 16, 1 << 30


def read_grow_summary(host):
    """The host copy of an ``a3d_grow_summary`` (uint8 [32], or anything of those bytes) as a dict of Python ints: ``seeds``,
    ``reached`` (voxels), ``selected`` (vertices), ``max_dist``, ``err`` (bit ``GROW_BAD_INDEX``)."""
    return _summary_ints(host, GROW_SUMMARY)


def grow_workspace(n, device):
    """The scratch of ``grow_voxels`` for n voxels (``a3d_grow_workspace_bytes``)."""
    return _scratch(L.load().a3d_grow_workspace_bytes(n), device, f"no grow workspace for n={n}")


def grow_settings(cost, limit, connectivity):
    """``(cost, limit, connectivity)`` as ``a3d_grow_voxels`` takes them, checked on the host: three integer step costs in
    1 .. 65536 (face, edge, corner), an integer limit in 0 .. 2^30 that is at most ``GROW_MAX_STEPS`` steps of the cheapest,
    a connectivity of 6, 18 or 26.  ``ValueError`` naming the argument."""
    connectivity = _connectivity(connectivity)
    try:
        cost = tuple(cost)
    except TypeError:
        cost = ()
    three = f"cost must be three integers in 1 .. {GROW_MAX_COST} (face, edge, corner)"
    if len(cost) != 3:
        raise ValueError(three)
    cost = tuple(_int_in("cost", c, 1, GROW_MAX_COST, three) for c in cost)
    if _int_in("limit", limit, 0, GROW_MAX_LIMIT) // min(cost) > GROW_MAX_STEPS:
        raise ValueError(f"limit = {limit} is more than {GROW_MAX_STEPS} steps of cost {min(cost)}: everything connected is "
                         "what label_pieces answers")
    return cost, int(limit), connectivity


def grow_voxels(scene, n_full, keys=None, seed_qv=None, seed_full=None, inverse_map=None, cost=GROW_METRIC_COST, limit=0,
                connectivity=26, dist_qv=None, owner_qv=None, selected_full=None, dist_full=None, summary=None, workspace=None):
    """``a3d_grow_voxels``: the bounded shortest-path distance from a set of seed voxels over the voxels of ``scene`` (an
    ``engine.Scene``; n rows in the caller's order), and the seed that is nearest.  ``n_full``: the number of vertices the
    result is lifted to (0: none).  ``keys`` int32 [n] or ``None`` (all 0): a key < 0 cannot be walked on, an edge is walkable
    between equal keys.  Seeds: ``seed_qv`` uint8 [n] and / or ``seed_full`` uint8 [n_full] through ``inverse_map`` int64
    [n_full] (``None``: the identity); one of the two at least.  ``cost``: the face, edge and corner step; ``limit``: the
    largest path cost (``grow_settings``).  Outputs: a tensor of the caller's, ``None`` = allocated, ``False`` = not wanted.
    Returns ``(dist_qv int32 [n], owner_qv int32 [n], selected_full uint8 [n_full], dist_full int32 [n_full], summary uint8
    [32], workspace)`` on the device, ``None`` for what was not wanted; ``read_grow_summary`` decodes the summary's host copy."""
    cost, limit, connectivity = grow_settings(cost, limit, connectivity)
    n_full = _int_in("n_full", n_full, 0, (1 << 31) - 1, "n_full must be an integer in 0 .. 2^31 - 1")
    if seed_qv is None and seed_full is None:
        raise ValueError("seed_qv or seed_full: one of the two seed arrays must be given")
    if n_full == 0 and (seed_full is not None or inverse_map is not None):
        raise ValueError("seed_full and inverse_map belong to the vertices: n_full is 0")
    handle, n = _scene_rows(scene)
    dev = _device("seed_qv" if seed_qv is not None else "seed_full", seed_qv if seed_qv is not None else seed_full)
    a = L.GrowVoxelsArgs()
    a.scene, a.n, a.n_full = handle, n, n_full
    a.keys_dev = _ptr("keys", keys, I32, (n,), dev, optional=True)
    a.seed_qv_dev = _ptr("seed_qv", seed_qv, U8, (n,), dev, optional=True)
    a.seed_full_dev = _ptr("seed_full", seed_full, U8, (n_full,), dev, optional=True)
    a.inverse_map_dev = _ptr("inverse_map", inverse_map, I64, (n_full,), dev, optional=True)
    a.connectivity, a.limit = connectivity, limit
    a.cost[:] = cost
    outs = _wanted(a, dev, (("dist_qv", dist_qv, I32, (n,)), ("owner_qv", owner_qv, I32, (n,)),
                            ("selected_full", selected_full, U8, (n_full,)), ("dist_full", dist_full, I32, (n_full,))))
    summary = _summary(summary, GROW_SUMMARY.itemsize, dev)
    a.summary_dev = summary.data_ptr()
    if workspace is None:
        workspace = grow_workspace(n, dev)
    _attach(a, workspace, dev, L.load().a3d_grow_workspace_bytes(n),
            "workspace too small or not 256-byte aligned (grow_workspace(n, device))")
    L.check(L.load().a3d_grow_voxels(C.byref(a), L.stream(dev)), "a3d_grow_voxels")
    return (*outs, summary, workspace)


# ---- measuring the objects of a labelling ---------------------------------------------------------------------------------------
OBJECT_MOMENTS = np.dtype([("vertices", "<i8"), ("voxels", "<i8"), ("sum", "<i8", (3,)), ("mom", "<i8", (6,)),
                           ("area_thirds", "<i8"), ("lo", "<f4", (3,)), ("hi", "<f4", (3,)), ("reserved_", "<i4", (2,))])
assert C.sizeof(L.ObjectMoments) == OBJECT_MOMENTS.itemsize == 128
MEASURE_RANGE, MEASURE_BAD_LABEL = L.A3D_MEASURE_RANGE, L.A3D_MEASURE_BAD_LABEL      # the bits of the two calls' error word


def read_object_moments(host):
    """The ``OBJECT_MOMENTS`` records (one per object id) of the host copy of ``measure_objects``' record buffer (uint8, 128
    bytes a record, or anything of those bytes): ``vertices``, ``voxels``, ``sum`` [3] and ``mom`` [6] (fixed-point, int64),
    ``area_thirds``, ``lo`` / ``hi`` fp32 [3].  A copy."""
    raw = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
    return raw[:len(raw) // OBJECT_MOMENTS.itemsize * OBJECT_MOMENTS.itemsize].view(OBJECT_MOMENTS).copy()


def _power_of_two(name, value):
    value = float(value)
    if not (np.isfinite(value) and value > 0.0 and np.frexp(value)[0] == 0.5):
        raise ValueError(f"{name} must be a positive power of two, not {value!r}")
    return value


def measure_objects(xyz, labels, origin, quantum, bits=L.A3D_MEASURE_MAX_BITS, n_classes=256, labels_qv=None, faces=None,
                    area_quantum=None, records=None, err=None):
    """``a3d_measure_objects``: one record per object id 0..n_classes-1 of ``labels`` int32 [n] over the vertices ``xyz`` fp32
    [n, 3] -- vertices, the exact fp32 box, and the sums of the fixed-point coordinates ``X = rint((x - origin) / quantum)`` and
    of their products; a vertex with ``|X| > 2^bits`` or a label outside counts nowhere and sets a bit of the error word.
    ``origin``: three finite numbers; ``quantum``: a positive power of two; ``bits`` in 0..20 with ``n * 2^(2 bits) <= 2^62``.
    ``labels_qv`` int32 [n_qv]: also count the voxels per object.  ``faces`` int32 [m, 3] (m <= 2^23): also the surface each
    object covers, in thirds of ``area_quantum`` (a positive power of two; default ``quantum^2 * 2^8``).  Returns ``(records
    uint8 [128 n_classes], err int32 [1])`` on the device, the caller's or allocated; ``read_object_moments`` decodes the host
    copy of the first, the second holds ``MEASURE_RANGE`` / ``MEASURE_BAD_LABEL``."""
    dev = _device("xyz", xyz)
    a = L.MeasureArgs()
    a.xyz_dev = _ptr("xyz", xyz, F32, (None, 3), dev)
    a.n = n = xyz.shape[0]
    a.labels_dev = _ptr("labels", labels, I32, (n,), dev)
    a.n_classes = _int_in("n_classes", n_classes, 1, 256)
    a.bits = _int_in("bits", bits, 0, L.A3D_MEASURE_MAX_BITS)
    if n >= 1 << 31 or n << (2 * a.bits) > 1 << 62:
        raise ValueError(f"{n} vertices at bits={a.bits}: the sums could overflow (n * 2^(2 bits) <= 2^62)")
    o = np.asarray(origin, dtype=np.float64).reshape(-1)
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError("origin must be three finite numbers")
    a.origin[:] = o.tolist()
    a.quantum = _power_of_two("quantum", quantum)
    if labels_qv is not None:
        a.labels_qv_dev = _ptr("labels_qv", labels_qv, I32, (None,), dev)
        a.n_qv = labels_qv.shape[0]
    if faces is not None:
        a.faces_dev = _ptr("faces", faces, I32, (None, 3), dev)
        a.m = faces.shape[0]
        if a.m > L.A3D_MEASURE_MAX_FACES:
            raise ValueError(f"at most {L.A3D_MEASURE_MAX_FACES} faces")
        a.area_quantum = _power_of_two("area_quantum", a.quantum * a.quantum * 256.0 if area_quantum is None else area_quantum)
    elif area_quantum is not None:
        raise ValueError("area_quantum belongs to the faces: faces is missing")
    records = _out("records", records, U8, (a.n_classes * OBJECT_MOMENTS.itemsize,), dev)
    if records.data_ptr() % 8:
        raise ValueError("records must be 8-byte aligned")
    err = _out("err", err, I32, (1,), dev)
    a.out_dev, a.err_dev = records.data_ptr(), err.data_ptr()
    L.check(L.load().a3d_measure_objects(C.byref(a), L.stream(dev)), "a3d_measure_objects")
    return records, err


def object_extents(xyz, labels, axes, extents=None, err=None):
    """``a3d_object_extents``: for every object id k of ``labels`` int32 [n] (0..n_classes-1, ``n_classes`` = ``axes.shape[0]``)
    and each of its three axes ``axes`` fp32 [n_classes, 3, 3] (row j of object k = axis j) the smallest and the largest
    projection ``(a_x x + a_y y) + a_z z`` (fp32, one operation at a time) of the object's vertices ``xyz`` fp32 [n, 3].
    Returns ``(extents fp32 [n_classes, 3, 2] = (min, max), err int32 [1])`` on the device, the caller's or allocated; an object
    without a vertex has ``(+inf, -inf)``."""
    dev = _device("xyz", xyz)
    a = L.ExtentsArgs()
    a.xyz_dev = _ptr("xyz", xyz, F32, (None, 3), dev)
    a.n = n = xyz.shape[0]
    a.labels_dev = _ptr("labels", labels, I32, (n,), dev)
    a.axes_dev = _ptr("axes", axes, F32, (None, 3, 3), dev)
    a.n_classes = _int_in("n_classes", axes.shape[0], 1, 256)
    if n >= 1 << 31:
        raise ValueError("at most 2^31 - 1 vertices")
    extents = _out("extents", extents, F32, (a.n_classes, 3, 2), dev)
    err = _out("err", err, I32, (1,), dev)
    a.out_dev, a.err_dev = extents.data_ptr(), err.data_ptr()
    L.check(L.load().a3d_object_extents(C.byref(a), L.stream(dev)), "a3d_object_extents")
    return extents, err


# ---- normals for point clouds: the estimate, the lit pass, the culled copy -------------------------------------------------------
NORMALS_SUMMARY = np.dtype([("counted", "<i8"), ("valid", "<i8"), ("invalid", "<i8"), ("err", "<i4"), ("reserved_", "<i4")])
assert C.sizeof(L.NormalsSummary) == NORMALS_SUMMARY.itemsize == 32
assert C.sizeof(L.EstimateNormalsArgs) == 168
NORMALS_RANGE, NORMALS_BAD_INDEX = L.A3D_NORMALS_RANGE, L.A3D_NORMALS_BAD_INDEX      # the bits of the summary's error word
CULL_MODES = {"back": L.A3D_CULL_BACK, "front": L.A3D_CULL_FRONT}


def read_normals_summary(host):
    """The host copy of an ``a3d_normals_summary`` (uint8 [32], or anything of those bytes) as a dict of Python ints:
    ``counted`` (vertices), ``valid`` / ``invalid`` (voxels with / without a normal), ``err`` (``NORMALS_RANGE``,
    ``NORMALS_BAD_INDEX``)."""
    return _summary_ints(host, NORMALS_SUMMARY)


def normals_workspace(n, device):
    """The scratch of ``estimate_normals`` for n voxels (``a3d_normals_workspace_bytes``)."""
    return _scratch(L.load().a3d_normals_workspace_bytes(n), device, f"no normals workspace for n={n}")


def _three_finite(name, values):
    a = np.asarray(values, dtype=np.float64).reshape(-1)
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError(f"{name} must be three finite numbers")
    return a.tolist()


def estimate_normals(scene, xyz, origin, quantum, bits=L.A3D_MEASURE_MAX_BITS, inverse_map=None, viewpoint=None, normal_qv=None,
                     variation_qv=None, count_qv=None, moments_qv=None, normal_full=None, summary=None, workspace=None):
    """``a3d_estimate_normals``: one unoriented normal per voxel of ``scene`` (an ``engine.Scene``; n rows in the caller's
    order) from the vertices ``xyz`` fp32 [n_full, 3] of its 3 x 3 x 3 neighbourhood -- ``inverse_map`` int64 [n_full] names
    each vertex's voxel (``None``: the identity) -- lifted to the vertices.  ``origin``, ``quantum``, ``bits``: the fixed-point
    frame of ``measure_objects`` (three finite numbers, a positive power of two, 0..20 with ``n_full * 2^(2 bits) <= 2^62``).
    ``viewpoint``: three finite numbers the normals are turned towards, or ``None``: the component of largest magnitude is
    made positive.  Outputs: a tensor of the caller's, ``None`` = allocated, ``False`` = not wanted.  Returns ``(normal_qv fp32
    [n, 3], variation_qv fp32 [n], count_qv int32 [n], moments_qv int64 [n, 10], normal_full fp32 [n_full, 3], summary uint8
    [32], workspace)`` on the device, ``None`` for what was not wanted; ``read_normals_summary`` decodes the summary's host
    copy."""
    handle, n = _scene_rows(scene)
    dev = _device("xyz", xyz)
    a = L.EstimateNormalsArgs()
    a.scene, a.n = handle, n
    a.xyz_dev = _ptr("xyz", xyz, F32, (None, 3), dev)
    a.n_full = n_full = xyz.shape[0]
    a.inverse_map_dev = _ptr("inverse_map", inverse_map, I64, (n_full,), dev, optional=True)
    a.bits = _int_in("bits", bits, 0, L.A3D_MEASURE_MAX_BITS)
    if n_full >= 1 << 31 or n_full << (2 * a.bits) > 1 << 62:
        raise ValueError(f"{n_full} vertices at bits={a.bits}: the sums could overflow (n_full * 2^(2 bits) <= 2^62)")
    a.origin[:] = _three_finite("origin", origin)
    a.quantum = _power_of_two("quantum", quantum)
    a.has_viewpoint = int(viewpoint is not None)
    if viewpoint is not None:
        a.viewpoint[:] = _three_finite("viewpoint", viewpoint)
    outs = _wanted(a, dev, (("normal_qv", normal_qv, F32, (n, 3)), ("variation_qv", variation_qv, F32, (n,)),
                            ("count_qv", count_qv, I32, (n,)), ("moments_qv", moments_qv, I64, (n, 10)),
                            ("normal_full", normal_full, F32, (n_full, 3))))
    summary = _summary(summary, NORMALS_SUMMARY.itemsize, dev)
    a.summary_dev = summary.data_ptr()
    if workspace is None:
        workspace = normals_workspace(n, dev)
    _attach(a, workspace, dev, L.load().a3d_normals_workspace_bytes(n),
            "workspace too small or not 256-byte aligned (normals_workspace(n, device))")
    L.check(L.load().a3d_estimate_normals(C.byref(a), L.stream(dev)), "a3d_estimate_normals")
    return (*outs, summary, workspace)


def normals_solve(count, sums, moments, origin, quantum, viewpoint=None):
    """``a3d_normals_solve`` (host only, no GPU): stage B of ``a3d_estimate_normals`` for ONE neighbourhood from its integer
    sums -- ``count``, ``sums`` [3] (X, Y, Z), ``moments`` [6] (XX, XY, XZ, YY, YZ, ZZ), each an integer an int64 holds -- by the
    function the kernel calls: ``(normal fp32 [3], variation numpy.float32, valid bool)``."""
    s = (C.c_int64 * 3)(*[int(v) for v in sums])
    m = (C.c_int64 * 6)(*[int(v) for v in moments])
    o = (C.c_double * 3)(*_three_finite("origin", origin))
    vp = None if viewpoint is None else (C.c_double * 3)(*_three_finite("viewpoint", viewpoint))
    out = np.zeros(5, np.float32)
    L.check(L.load().a3d_normals_solve(int(count), s, m, o, _power_of_two("quantum", quantum), vp,
                                       out.ctypes.data_as(C.POINTER(C.c_float))), "a3d_normals_solve")
    return out[:3].copy(), out[3], bool(out[4])


def render_shade_lit_points(ids, colors, normals, cam, ambient, background, rgb=None):
    """``a3d_render_shade_lit_points``: a cloud's colours lit from the camera by per-vertex normals fp32 [n, 3] (the
    ``normal_full`` of ``estimate_normals``); a vertex with a zero normal keeps its colour."""
    dev, (h, w), (ip, _, _, _, cp), _, n, (bg, bgp), rgb = _shade_args(ids, None, None, None, colors, background, rgb)
    if (h, w) != (cam.height, cam.width):
        raise ValueError(f"ids must have the camera's shape [{cam.height}, {cam.width}]")
    ambient = float(ambient)
    if not 0.0 <= ambient <= 1.0:                       # (NaN fails both)
        raise ValueError("ambient must lie in [0, 1]")
    np_ = _ptr("normals", normals, F32, (n, 3), dev)
    L.check(L.load().a3d_render_shade_lit_points(ip, cp, n, np_, C.byref(cam), ambient, bgp, rgb.data_ptr(), L.stream(dev)),
            "a3d_render_shade_lit_points")
    return rgb


def cull_points(xyz, normals, eye, mode, out=None, hidden=None, count=None):
    """``a3d_cull_points``: the copy of ``xyz`` fp32 [n, 3] in which the vertices whose normal (``normals`` fp32 [n, 3]) points
    away from ``eye`` (``mode="back"``) or towards it (``"front"``) have NaN coordinates -- what the picks, the renders and
    ``select_vertices`` then do not see.  ``eye``: three finite numbers (rounded to fp32).  ``hidden`` uint8 [n] and ``count``
    int64 [1]: a tensor of the caller's, ``None`` = allocated, ``False`` = not wanted.  Returns ``(out, hidden, count)`` on the
    device."""
    if mode not in CULL_MODES:
        raise ValueError(f"mode must be one of {sorted(CULL_MODES)}, not {mode!r}")
    dev = _device("xyz", xyz)
    xp = _ptr("xyz", xyz, F32, (None, 3), dev)
    n = xyz.shape[0]
    np_ = _ptr("normals", normals, F32, (n, 3), dev)
    if max(abs(c) for c in _three_finite("eye", eye)) > float(np.finfo(np.float32).max):
        raise ValueError("eye must be three finite numbers in fp32")
    e, ep = _f32p("eye", eye, (3,))
    out = _out("out", out, F32, (n, 3), dev)
    hidden = None if hidden is False else _out("hidden", hidden, U8, (n,), dev)
    count = None if count is False else _out("count", count, I64, (1,), dev)
    L.check(L.load().a3d_cull_points(xp, np_, n, ep, CULL_MODES[mode], out.data_ptr() if n else None,
                                     hidden.data_ptr() if hidden is not None and n else None,
                                     count.data_ptr() if count is not None else None, L.stream(dev)), "a3d_cull_points")
    return out, hidden, count


# ---- one sign for a whole surface: normals oriented by propagation ---------------------------------------------------------------
ORIENT_SUMMARY = np.dtype([("admitted", "<i8"), ("seeds", "<i8"), ("reached", "<i8"), ("unreached", "<i8"), ("flipped", "<i8"),
                           ("conflicts", "<i8"), ("max_dist", "<i4"), ("converged", "<i4"), ("err", "<i4"), ("reserved_", "<i4")])
assert C.sizeof(L.OrientSummary) == ORIENT_SUMMARY.itemsize == 64
assert C.sizeof(L.OrientNormalsArgs) == 176
ORIENT_MAX_ROWS, ORIENT_MAX_SWEEPS = L.A3D_ORIENT_MAX_ROWS, L.A3D_ORIENT_MAX_SWEEPS
ORIENT_BAD_INDEX, ORIENT_BAD_COMPONENT = L.A3D_ORIENT_BAD_INDEX, L.A3D_ORIENT_BAD_COMPONENT    # the bits of the error word
ORIENT_MODES = {"given": L.A3D_ORIENT_GIVEN, "nearest": L.A3D_ORIENT_NEAREST}


def read_orient_summary(host):
    """The host copy of an ``a3d_orient_summary`` (uint8 [64], or anything of those bytes) as a dict of Python ints:
    ``admitted``, ``seeds``, ``reached``, ``unreached``, ``flipped`` (voxels), ``conflicts`` (edges), ``max_dist``,
    ``converged`` (1: the last sweep lowered nothing) and ``err`` (``ORIENT_BAD_INDEX``, ``ORIENT_BAD_COMPONENT``)."""
    return _summary_ints(host, ORIENT_SUMMARY)


def orient_workspace(n, device):
    """The scratch of ``orient_normals`` for n voxels (``a3d_orient_workspace_bytes``; at most 2^21 voxels).  A call with
    ``resume=True`` continues from what the call before left in it."""
    return _scratch(L.load().a3d_orient_workspace_bytes(n), device, f"no orient workspace for n={n} (0 .. {ORIENT_MAX_ROWS})")


def orient_edge(a, b):
    """``a3d_orient_edge`` (host only, no GPU): ``(w, flip)`` of the edge between two voxels with the normals ``a`` and ``b``
    (fp32 [3] each) -- the cost in 1 .. 1024 and whether the normals disagree (``dot < 0``) -- by the function the kernel calls.
    NaNs and zeros are passed on as they are."""
    ka, pa = _f32p("a", a, (3,))
    kb, pb = _f32p("b", b, (3,))
    w, flip = C.c_int32(0), C.c_int32(0)
    L.check(L.load().a3d_orient_edge(pa, pb, C.byref(w), C.byref(flip)), "a3d_orient_edge")
    return int(w.value), bool(flip.value)


def orient_normals(scene, normals, seed_qv=None, seed_flip=None, components=None, positions=None, viewpoint=None, connectivity=26,
                   sweeps=512, resume=False, inverse_map=None, n_full=None, normal_out_qv=None, flipped_qv=None, dist_qv=None,
                   owner_qv=None, normal_full=None, summary=None, workspace=None):
    """``a3d_orient_normals``: the ``normals`` fp32 [n, 3] of the voxels of ``scene`` (an ``engine.Scene``; n rows in the
    caller's order) given one consistent sign by propagation from seed voxels along the edges between neighbours under
    ``connectivity`` (the rule: include/agile3d_hip.h).  Seeds, one of two modes: ``seed_qv`` uint8 [n] marks voxels whose sign
    is trusted (``seed_flip`` uint8 [n], optional: negate these first); or ``components`` int32 [n] (``label_pieces`` of the
    rows with a normal), ``positions`` fp32 [n, 3] and ``viewpoint`` (three finite numbers): per component the voxel nearest to
    the viewpoint is the seed and is turned towards it.  ``sweeps`` (1 .. 4096) relaxation sweeps are launched; with
    ``resume`` the call continues from the state ``workspace`` holds (the same arguments otherwise).  The lift: ``inverse_map``
    int64 [n_full], or ``n_full`` alone for the identity.  Outputs: a tensor of the caller's, ``None`` = allocated, ``False`` =
    not wanted.  Returns ``(normal_out_qv fp32 [n, 3], flipped_qv uint8 [n], dist_qv int32 [n], owner_qv int32 [n],
    normal_full fp32 [n_full, 3], summary uint8 [64], workspace)`` on the device, ``None`` for what was not wanted;
    ``read_orient_summary`` decodes the summary's host copy -- while its ``converged`` is 0 the outputs are not final."""
    connectivity = _connectivity(connectivity)
    sweeps = _int_in("sweeps", sweeps, 1, ORIENT_MAX_SWEEPS)
    handle, n = _scene_rows(scene)
    if n > ORIENT_MAX_ROWS:
        raise ValueError(f"{n} voxels: at most {ORIENT_MAX_ROWS} (2^21), so that every path cost fits 31 bits")
    given = seed_qv is not None or seed_flip is not None
    nearest = components is not None or positions is not None or viewpoint is not None
    if given == nearest:
        raise ValueError("seeds: either seed_qv (with seed_flip), or components, positions and viewpoint")
    if given and seed_qv is None:
        raise ValueError("seed_flip belongs to seed_qv, which is missing")
    if nearest and (components is None or positions is None or viewpoint is None):
        raise ValueError("the nearest seeds need components, positions and viewpoint, all three")
    dev = _device("normals", normals)
    a = L.OrientNormalsArgs()
    a.scene, a.n = handle, n
    a.normal_qv_dev = _ptr("normals", normals, F32, (n, 3), dev)
    a.mode = L.A3D_ORIENT_GIVEN if given else L.A3D_ORIENT_NEAREST
    a.seed_qv_dev = _ptr("seed_qv", seed_qv, U8, (n,), dev, optional=True)
    a.seed_flip_dev = _ptr("seed_flip", seed_flip, U8, (n,), dev, optional=True)
    a.component_qv_dev = _ptr("components", components, I32, (n,), dev, optional=True)
    a.position_qv_dev = _ptr("positions", positions, F32, (n, 3), dev, optional=True)
    if nearest:
        a.viewpoint[:] = _three_finite("viewpoint", viewpoint)
    a.connectivity, a.sweeps, a.resume = connectivity, sweeps, int(bool(resume))
    if inverse_map is not None:
        if n_full is not None and n_full != inverse_map.shape[0]:
            raise ValueError("n_full must be the length of inverse_map")
        n_full = inverse_map.shape[0]
    n_full = _int_in("n_full", 0 if n_full is None else n_full, 0, (1 << 31) - 1, "n_full must be an integer in 0 .. 2^31 - 1")
    a.n_full = n_full
    a.inverse_map_dev = _ptr("inverse_map", inverse_map, I64, (n_full,), dev, optional=True)
    outs = _wanted(a, dev, (("normal_out_qv", normal_out_qv, F32, (n, 3)), ("flipped_qv", flipped_qv, U8, (n,)),
                            ("dist_qv", dist_qv, I32, (n,)), ("owner_qv", owner_qv, I32, (n,)),
                            ("normal_full", normal_full, F32, (n_full, 3))))
    if outs[0] is not None and outs[0].data_ptr() == normals.data_ptr():
        raise ValueError("normal_out_qv must not be the input array")
    summary = _summary(summary, ORIENT_SUMMARY.itemsize, dev)
    a.summary_dev = summary.data_ptr()
    if workspace is None:
        if resume:
            raise ValueError("resume continues from a workspace: pass the one the call before returned")
        workspace = orient_workspace(n, dev)
    _attach(a, workspace, dev, L.load().a3d_orient_workspace_bytes(n),
            "workspace too small or not 256-byte aligned (orient_workspace(n, device))")
    L.check(L.load().a3d_orient_normals(C.byref(a), L.stream(dev)), "a3d_orient_normals")
    return (*outs, summary, workspace)


# ---- labels to and from another point set: an index over any point set, the bulk nearest query ---------------------------------
TRANSFER_SUMMARY = np.dtype([("matched", "<i8"), ("unmatched", "<i8"), ("nonfinite", "<i8"), ("source_left_out", "<i8"),
                             ("err", "<i4"), ("reserved_", "<i4")])
assert C.sizeof(L.TransferSummary) == TRANSFER_SUMMARY.itemsize == 40
TRANSFER_UNKEYABLE, TRANSFER_SORT_FAILED = L.A3D_TRANSFER_UNKEYABLE, L.A3D_TRANSFER_SORT_FAILED   # the bits of the error word
POINT_INDEX_MAX_CELLS = 1 << 20                 # a source coordinate lies within this many cells of the origin


def read_transfer_summary(host, check=True):
    """The host copy of an ``a3d_transfer_summary`` (uint8 [40], or anything of those bytes) as a dict of Python ints:
    ``matched``, ``unmatched`` (finite queries without a row in reach), ``nonfinite`` (queries), ``source_left_out`` (source
    rows that are not finite), ``err``.  With ``check`` an index that left rows out because they cannot be keyed raises
    ``ValueError`` (``TRANSFER_UNKEYABLE``: its answers ignore those rows) and one whose sort gave up ``RuntimeError``."""
    s = _summary_ints(host, TRANSFER_SUMMARY)
    if check and s["err"] & TRANSFER_UNKEYABLE:
        raise ValueError(f"a source coordinate lies more than {POINT_INDEX_MAX_CELLS} cells of cell_size from the origin: such "
                         "a point set cannot be indexed (a larger cell_size, or coordinates moved towards the origin)")
    if check and s["err"]:
        raise RuntimeError("a3d_point_index_create: the sort of the build gave up; the index is not usable")
    return s


def _positive_f32(name, value):
    """``value`` rounded to fp32, as the library compares it; finite and > 0 there."""
    with np.errstate(over="ignore"):
        v = float(np.float32(value))
    if not (np.isfinite(v) and v > 0.0):
        raise ValueError(f"{name} must be finite and > 0 in fp32")
    return v


def point_index_workspace(n, device):
    """The memory an index over n points lives in (``a3d_point_index_workspace_bytes``)."""
    return _scratch(L.load().a3d_point_index_workspace_bytes(n), device, f"no point index for n={n}")


class PointIndex:
    """An ``a3d_point_index``: the handle, the workspace it lives in (kept alive here), ``n`` source rows, ``cell_size`` (the
    fp32 value) and the device.  ``close()`` frees the handle and lets go of the workspace; a closed index is refused."""

    def __init__(self, handle, workspace, n, cell_size, device):
        self.handle, self.workspace, self.n, self.cell_size, self.device = handle, workspace, n, cell_size, device

    def close(self):
        if self.handle is not None:
            L.load().a3d_point_index_destroy(self.handle)
        self.handle = self.workspace = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def point_index_create(xyz, cell_size, workspace=None):
    """``a3d_point_index_create``: a ``PointIndex`` over ``xyz`` fp32 [n, 3] (n >= 0) with cubic cells of ``cell_size`` (rounded
    to fp32).  Rows that are not finite are left out and counted in every query's summary.  ``workspace``: uint8, 256-byte
    aligned, ``point_index_workspace(n, device)`` or larger (allocated otherwise).  ``xyz`` is not needed after the call's
    launches have run; nothing is synchronised."""
    dev = _device("xyz", xyz)
    xp = _ptr("xyz", xyz, F32, (None, 3), dev)
    n = xyz.shape[0]
    if n >= 1 << 31:
        raise ValueError(f"xyz: {n} rows, the index takes fewer than 2^31")
    cell = _positive_f32("cell_size", cell_size)
    need = L.load().a3d_point_index_workspace_bytes(n)
    if workspace is None:
        workspace = point_index_workspace(n, dev)
    wp = _ptr("workspace", workspace, U8, (None,), dev)
    if workspace.shape[0] < need or workspace.data_ptr() % 256:
        raise ValueError("workspace too small or not 256-byte aligned (point_index_workspace(n, device))")
    handle = C.c_void_p()
    L.check(L.load().a3d_point_index_create(xp, n, cell, wp, workspace.shape[0], L.stream(dev), C.byref(handle)),
            "a3d_point_index_create")
    return PointIndex(handle, workspace, n, cell, dev)


def point_index_nearest(index, queries, max_distance, labels_src=None, fill=0, nearest=None, d2=None, labels=None, summary=None):
    """``a3d_point_index_nearest``: for every row of ``queries`` fp32 [m, 3] the nearest source row of ``index`` within
    ``max_distance`` (rounded to fp32; 0 < max_distance <= index.cell_size / 2), by the brute-force rule of the header: the
    first arg-min of the fp32 distance among the finite rows in reach, -1 without one.  ``labels_src`` int32 [index.n]: the
    labels to carry, gathered in the same kernel (``fill`` where nothing is in reach).  Outputs: a tensor of the caller's,
    ``None`` = allocated; ``d2=False`` = not wanted; ``labels`` exists exactly with ``labels_src``.  Returns ``(nearest int32
    [m], d2 fp32 [m] or None, labels int32 [m] or None, summary uint8 [40])`` on the device; ``read_transfer_summary`` decodes
    the summary's host copy."""
    if not isinstance(index, PointIndex) or index.handle is None:
        raise ValueError("index must be an open PointIndex (point_index_create)")
    dev = index.device
    if not torch.is_tensor(queries) or queries.device != dev:
        raise ValueError(f"queries must be a tensor on {dev}, the index's device")
    qp = _ptr("queries", queries, F32, (None, 3), dev)
    m = queries.shape[0]
    if m >= 1 << 31:
        raise ValueError(f"queries: {m} rows, a call takes fewer than 2^31")
    r = _positive_f32("max_distance", max_distance)
    if r > float(np.float32(0.5) * np.float32(index.cell_size)):
        raise ValueError(f"max_distance={r} must not exceed half the index's cell_size={index.cell_size}")
    fill = _int_in("fill", fill, -(1 << 31), (1 << 31) - 1)
    lp = _ptr("labels_src", labels_src, I32, (index.n,), dev, optional=True)
    if labels_src is None and labels is not None:
        raise ValueError("labels is written only with labels_src")
    nearest = _out("nearest", nearest, I32, (m,), dev)
    d2 = None if d2 is False else _out("d2", d2, F32, (m,), dev)
    labels = None if labels_src is None else _out("labels", labels, I32, (m,), dev)
    summary = _summary(summary, TRANSFER_SUMMARY.itemsize, dev)
    if labels_src is not None and lp is None:           # (no source rows: a pointer all the same, never followed)
        lp = summary.data_ptr()
    L.check(L.load().a3d_point_index_nearest(index.handle, qp, m, r, lp, fill, nearest.data_ptr() if m else None,
                                             d2.data_ptr() if d2 is not None and m else None,
                                             (labels.data_ptr() if m else summary.data_ptr()) if labels is not None else None,
                                             summary.data_ptr(), L.stream(dev)), "a3d_point_index_nearest")
    return nearest, d2, labels, summary


# ---- correcting by hand: a screen region, the vertices seen inside it, the manual layer ----------------------------------------
SELECT_SUMMARY = np.dtype([("selected", "<i8"), ("in_view", "<i8"), ("flags", "<i4"), ("reserved_", "<i4")])
OVERLAY_SUMMARY = np.dtype([("changed", "<i8"), ("overridden", "<i8"), ("differing", "<i8"), ("err", "<i4"), ("reserved_", "<i4")])
assert C.sizeof(L.SelectSummary) == SELECT_SUMMARY.itemsize == 24
assert C.sizeof(L.OverlaySummary) == OVERLAY_SUMMARY.itemsize == 32
REGION_SHAPES = {"polygon": L.A3D_REGION_POLYGON, "stroke": L.A3D_REGION_STROKE}
REGION_MODES = {"replace": L.A3D_REGION_REPLACE, "add": L.A3D_REGION_ADD, "subtract": L.A3D_REGION_SUBTRACT}
OVERLAY_OPS = {"none": L.A3D_OVERLAY_NONE, "paint": L.A3D_OVERLAY_PAINT, "erase": L.A3D_OVERLAY_ERASE}
SELECT_NOT_FINITE = L.A3D_SELECT_NOT_FINITE     # the bit of the select summary's flags
OVERLAY_BAD_LABEL = 1                           # the bit of the overlay summary's error word


def read_select_summary(host):
    """The host copy of an ``a3d_select_summary`` (uint8 [24], or anything of those bytes) as a dict of Python ints:
    ``selected``, ``in_view``, ``flags`` (bit ``SELECT_NOT_FINITE``)."""
    return _summary_ints(host, SELECT_SUMMARY)


def read_overlay_summary(host):
    """The host copy of an ``a3d_overlay_summary`` (uint8 [32], or anything of those bytes) as a dict of Python ints:
    ``changed``, ``overridden``, ``differing``, ``err`` (bit ``OVERLAY_BAD_LABEL``)."""
    return _summary_ints(host, OVERLAY_SUMMARY)


def camera_rows(camera):
    """fp32 [9] (numpy): the rows of the inverse of the matrix with columns ``du``, ``dv``, ``d00`` of the ``lib.Camera`` as
    ``a3d_render_camera_bounds`` computes them in double (host only, no GPU), each value rounded to fp32 once -- what
    ``select_vertices`` projects with.  ``ValueError`` for a camera the renders refuse."""
    out = (C.c_double * 13)()
    if L.load().a3d_render_camera_bounds(C.byref(camera), out) != 0:
        raise ValueError("camera: a size outside 1 .. 4096, a value that is not finite, or du, dv and d00 close to one plane")
    with np.errstate(over="ignore"):
        return np.array(out[:9], np.float64).astype(np.float32)


def region_mask(shape, points, width, height, radius=None, mode="replace", mask=None, device=None):
    """``a3d_region_mask``: a screen region as uint8 [height, width] on the device, 1 inside.  ``shape``: ``"polygon"``
    (``points`` [k, 2] with 3 <= k <= 256, even-odd; ``radius`` must be ``None``) or ``"stroke"`` (1 <= k <= 256 points joined
    by segments, every pixel within ``radius`` > 0 of one of them).  ``points`` are host numbers ``(x, y)`` in pixels: the
    centre of pixel (u, v) is the position (u, v).  ``mode``: ``"replace"`` writes the region into ``mask`` (allocated on
    ``device`` when ``None``), ``"add"`` / ``"subtract"`` join it to / take it out of the caller's ``mask``, in place."""
    if shape not in REGION_SHAPES or mode not in REGION_MODES:
        raise ValueError(f"shape must be one of {sorted(REGION_SHAPES)} and mode one of {sorted(REGION_MODES)}")
    pts = np.ascontiguousarray(points, dtype=np.float32)
    if pts.ndim != 2 or pts.shape[1] != 2 or not (3 if shape == "polygon" else 1) <= len(pts) <= L.A3D_REGION_MAX_POINTS:
        raise ValueError(f"points must be [k, 2] with k in 3 .. {L.A3D_REGION_MAX_POINTS} (a polygon) or 1 .. "
                         f"{L.A3D_REGION_MAX_POINTS} (a stroke)")
    if not np.isfinite(pts).all():
        raise ValueError("points must be finite (in fp32)")
    if shape == "polygon":
        if radius is not None:
            raise ValueError("radius belongs to a stroke")
        radius = 0.0
    else:
        with np.errstate(over="ignore"):
            r32 = np.float32(np.nan if radius is None else radius)
        if not (np.isfinite(r32) and r32 > 0):
            raise ValueError("a stroke needs a finite radius > 0 (in fp32)")
    width, height = int(width), int(height)
    if not (1 <= width <= L.A3D_RENDER_MAX_SIZE and 1 <= height <= L.A3D_RENDER_MAX_SIZE):
        raise ValueError(f"width and height must lie in 1 .. {L.A3D_RENDER_MAX_SIZE}")
    if mask is None:
        if mode != "replace":
            raise ValueError(f"mode {mode!r} changes a mask: mask is missing")
        if device is None:
            raise ValueError("device is needed to allocate the mask")
        mask = torch.empty((height, width), dtype=U8, device=device)
    dev = _device("mask", mask)
    mp = _ptr("mask", mask, U8, (height, width), dev)
    L.check(L.load().a3d_region_mask(width, height, REGION_SHAPES[shape], pts.ctypes.data_as(C.POINTER(C.c_float)), len(pts),
                                     float(radius), REGION_MODES[mode], mp, L.stream(dev)), "a3d_region_mask")
    return mask


def select_vertices(xyz, cam, mask, t=None, slack=0.0, section=None, rows=None, selected=None, summary=None):
    """``a3d_select_vertices``: which of the vertices ``xyz`` fp32 [n, 3] the ``lib.Camera`` ``cam`` sees inside ``mask`` uint8
    [h, w] -- ``(selected uint8 [n], summary uint8 [24])`` on the device; ``read_select_summary`` decodes the summary's host
    copy.  ``t`` fp32 [h, w]: a render's t image; a vertex then also has to lie no more than ``slack`` >= 0 behind what its
    pixel shows (``None``: select through everything).  ``section``: a ``lib.Section`` or ``None``; a vertex on the cut side
    of a plane is not in view.  ``rows``: fp32 [9] as ``camera_rows(cam)`` gives them (computed when ``None``)."""
    dev = _device("xyz", xyz)
    h, w = cam.height, cam.width
    a = L.SelectArgs()
    a.xyz_dev, a.n = _ptr("xyz", xyz, F32, (None, 3), dev), xyz.shape[0]
    a.camera = cam
    r = camera_rows(cam) if rows is None else np.ascontiguousarray(rows, dtype=np.float32)
    if r.shape != (9,) or not np.isfinite(r).all():
        raise ValueError("rows must be nine finite numbers (in fp32)")
    a.rows[:] = r.tolist()
    with np.errstate(over="ignore"):
        s32 = np.float32(slack)
    if not (np.isfinite(s32) and s32 >= 0):
        raise ValueError("slack must be finite and >= 0 (in fp32)")
    a.slack = float(s32)
    a.mask_dev = _ptr("mask", mask, U8, (h, w), dev)
    a.t_dev = _ptr("t", t, F32, (h, w), dev, optional=True)
    _section_ptr(section)                       # (a lib.Section or None)
    if section is not None:
        a.section = C.pointer(section)
    selected = _out("selected", selected, U8, (a.n,), dev)
    a.selected_dev = selected.data_ptr() if a.n else None
    summary = _summary(summary, SELECT_SUMMARY.itemsize, dev)
    a.summary_dev = summary.data_ptr()
    L.check(L.load().a3d_select_vertices(C.byref(a), L.stream(dev)), "a3d_select_vertices")
    return selected, summary


def session_overlay(labels_in, manual_on, manual_obj, selected=None, op="none", obj=0, colors=None, palette=None,
                    labels_out=None, colors_out=None, summary=None):
    """``a3d_session_overlay``: the manual layer ``(manual_on uint8 [n], manual_obj int32 [n])`` -- updated IN PLACE where
    ``selected`` uint8 [n] is not 0: ``op`` ``"paint"`` sets them to ``obj`` (0..255), ``"erase"`` clears them, ``"none"``
    leaves the layer alone -- laid over the model's labels ``labels_in`` int32 [n].  With ``colors`` fp32 [n, 3] and ``palette``
    fp32 [K + 1, 3] the labels and colours of the result are written (``labels_out``, ``colors_out``: the caller's or
    allocated); without ``colors`` the call is a pure layer update and both come back ``None``.  Returns ``(labels_out,
    colors_out, summary uint8 [32])`` on the device; ``read_overlay_summary`` decodes the summary's host copy."""
    dev = _device("labels_in", labels_in)
    if op not in OVERLAY_OPS:
        raise ValueError(f"op must be one of {sorted(OVERLAY_OPS)}")
    obj = _int_in("obj", obj, 0, 255)
    a = L.SessionOverlayArgs()
    a.labels_in_dev, a.n = _ptr("labels_in", labels_in, I32, (None,), dev), labels_in.shape[0]
    n = a.n
    a.manual_on_dev, a.manual_obj_dev = _ptr("manual_on", manual_on, U8, (n,), dev), _ptr("manual_obj", manual_obj, I32, (n,), dev)
    a.selected_dev = _ptr("selected", selected, U8, (n,), dev, optional=True)
    a.op, a.obj = OVERLAY_OPS[op], obj
    if colors is not None:
        a.colors_full_dev = _ptr("colors", colors, F32, (n, 3), dev)
        a.palette_dev = _ptr("palette", palette, F32, (None, 3), dev)
        a.n_palette = palette.shape[0]
        if not 2 <= a.n_palette <= 256:
            raise ValueError("palette must be [K + 1, 3] with 1 <= K <= 255")
        labels_out, colors_out = _out("labels_out", labels_out, I32, (n,), dev), _out("colors_out", colors_out, F32, (n, 3), dev)
        # (without vertices there is nothing to write: the pointers of empty tensors travel as NULL, a pure layer update)
        a.labels_out_dev, a.colors_out_dev = (labels_out.data_ptr(), colors_out.data_ptr()) if n else (None, None)
    elif palette is not None or labels_out is not None or colors_out is not None:
        raise ValueError("palette, labels_out and colors_out belong to the outputs: colors is missing")
    summary = _summary(summary, OVERLAY_SUMMARY.itemsize, dev)
    a.summary_dev = summary.data_ptr()
    L.check(L.load().a3d_session_overlay(C.byref(a), L.stream(dev)), "a3d_session_overlay")
    return labels_out, colors_out, summary


# ---- more objects like this one: prototypes of example classes, the best prototype per voxel under a cosine threshold ---------
PROTOTYPES_SUMMARY = np.dtype([("examples", "<i8"), ("examples_left_out", "<i8"), ("err", "<i4"), ("reserved_", "<i4")])
MATCH_SUMMARY = np.dtype([("matched", "<i8", (L.A3D_MATCH_MAX_PROTOTYPES,)), ("rows_nonfinite", "<i8"), ("err", "<i4"),
                          ("reserved_", "<i4")])
assert C.sizeof(L.PrototypesSummary) == PROTOTYPES_SUMMARY.itemsize == 24
assert C.sizeof(L.MatchSummary) == MATCH_SUMMARY.itemsize == 2064
MATCH_CHANNELS, MATCH_MAX_PROTOTYPES = L.A3D_MATCH_CHANNELS, L.A3D_MATCH_MAX_PROTOTYPES
MATCH_QUANTUM = 2.0 ** -L.A3D_MATCH_QUANTUM_BITS
MATCH_BAD_CLASS, MATCH_BAD_INDEX, MATCH_BAD_PROTOTYPE = L.A3D_MATCH_BAD_CLASS, L.A3D_MATCH_BAD_INDEX, L.A3D_MATCH_BAD_PROTOTYPE


def read_prototypes_summary(host):
    """The host copy of an ``a3d_prototypes_summary`` (uint8 [24], or anything of those bytes) as a dict of Python ints:
    ``examples``, ``examples_left_out``, ``err`` (bit ``MATCH_BAD_CLASS``)."""
    return _summary_ints(host, PROTOTYPES_SUMMARY)


def read_match_summary(host):
    """The host copy of an ``a3d_match_summary`` (uint8 [2064], or anything of those bytes): ``matched`` (int64 [256], matched
    voxels per class), ``rows_nonfinite`` and ``err`` (bits ``MATCH_BAD_CLASS``, ``MATCH_BAD_INDEX``, ``MATCH_BAD_PROTOTYPE``)."""
    rec = _record(host, MATCH_SUMMARY)
    return dict(matched=rec["matched"].astype(np.int64), rows_nonfinite=int(rec["rows_nonfinite"]), err=int(rec["err"]))


def _features(name, feats, dev=None):
    """(pointer, rows) of a feature table: fp32 [n, 128], contiguous, on the GPU (on ``dev`` when given)."""
    dev = _device(name, feats) if dev is None else dev
    return _ptr(name, feats, F32, (None, MATCH_CHANNELS), dev), feats.shape[0]


def feature_prototypes(feats, classes, n_classes=MATCH_MAX_PROTOTYPES, sums=None, count=None, summary=None):
    """``a3d_feature_prototypes``: the fixed-point sums of the example rows of ``feats`` fp32 [n, 128] per class -- ``classes``
    int32 [n], -1 = no example, 0 .. n_classes-1 = the class; n < 2^22, 1 <= n_classes <= 256.  Returns ``(sums int64
    [n_classes, 128], count int32 [n_classes], summary uint8 [24])`` on the device (the caller's tensors or new ones);
    ``prototype_table`` turns the first two into prototypes, ``read_prototypes_summary`` decodes the summary's host copy."""
    dev = _device("feats", feats)
    a = L.FeaturePrototypesArgs()
    a.feats_dev, a.n = _features("feats", feats)
    if a.n >= L.A3D_MATCH_MAX_EXAMPLE_ROWS:
        raise ValueError(f"feats: {a.n} rows, the prototypes take fewer than 2^22")
    a.classes_dev = _ptr("classes", classes, I32, (a.n,), dev)
    a.n_classes = _int_in("n_classes", n_classes, 1, MATCH_MAX_PROTOTYPES)
    sums = _out("sums", sums, I64, (a.n_classes, MATCH_CHANNELS), dev)
    count = _out("count", count, I32, (a.n_classes,), dev)
    summary = _summary(summary, PROTOTYPES_SUMMARY.itemsize, dev)
    a.sums_dev, a.count_dev, a.summary_dev = sums.data_ptr(), count.data_ptr(), summary.data_ptr()
    L.check(L.load().a3d_feature_prototypes(C.byref(a), L.stream(dev)), "a3d_feature_prototypes")
    return sums, count, summary


def prototype_table(sums, count):
    """The caller's step of the prototype rule: fp32 [n_classes, 128], row c = ``float32((float64(sums[c]) / float64(count[c]))
    * 2^-20)`` -- int64 -> double to nearest even, one division, one exact scaling, one rounding, each an IEEE operation, so
    numpy arrays (the host step; a numpy array comes back) and tensors on any device (a tensor there comes back, nothing is
    synchronised) give the same bits.  A class with ``count == 0`` has no prototype: its row is ZERO, and a zero prototype
    (``pp == 0``) takes part in no match.  ``sums`` int64 [n_classes, 128], ``count`` int32 [n_classes]."""
    if torch.is_tensor(sums) != torch.is_tensor(count):
        raise ValueError("sums and count must both be tensors or both be numpy arrays")
    if torch.is_tensor(sums):
        if sums.dtype is not I64 or sums.dim() != 2 or sums.shape[1] != MATCH_CHANNELS:
            raise ValueError(f"sums must be an int64 [n_classes, {MATCH_CHANNELS}] tensor")
        if count.dtype is not I32 or tuple(count.shape) != (sums.shape[0],) or count.device != sums.device:
            raise ValueError(f"count must be an int32 [{sums.shape[0]}] tensor on sums' device")
        has = (count > 0).unsqueeze(1)
        mean = sums.to(torch.float64) / torch.where(has, count.unsqueeze(1), torch.ones_like(count.unsqueeze(1))).to(torch.float64)
        return torch.where(has, (mean * MATCH_QUANTUM).to(torch.float32), torch.zeros((), dtype=torch.float32, device=sums.device))
    s, c = np.asarray(sums), np.asarray(count)
    if s.dtype != np.int64 or s.ndim != 2 or s.shape[1] != MATCH_CHANNELS:
        raise ValueError(f"sums must be an int64 [n_classes, {MATCH_CHANNELS}] array")
    if c.dtype != np.int32 or c.shape != (s.shape[0],):
        raise ValueError(f"count must be an int32 [{s.shape[0]}] array")
    has = (c > 0)[:, None]
    mean = s.astype(np.float64) / np.where(has, c[:, None], 1).astype(np.float64)
    return np.where(has, (mean * MATCH_QUANTUM).astype(np.float32), np.float32(0.0))


def feature_match(feats, protos, proto_class, cos_min, candidate=None, inverse_map=None, match_qv=None, best_qv=None,
                  score_qv=None, match_full=None, score_full=None, summary=None):
    """``a3d_feature_match``: per row of ``feats`` fp32 [n, 128] the best of the prototypes ``protos`` fp32 [k, 128] (1 <= k <=
    256; ``proto_class`` int32 [k], classes 0..255) whose cosine reaches ``cos_min`` (a finite number in [0, 1]), by the rule
    of include/agile3d_hip.h.  ``candidate`` uint8 [n]: 0 = the voxel matches nothing (``None``: every voxel may).
    ``inverse_map`` int64 [n_full]: also lift the match and the score to the vertices.  ``protos`` on the HOST (a numpy array
    or a CPU tensor) are checked to be finite and uploaded; prototypes already on the device are the caller's word -- one that
    is not finite takes part in nothing and sets ``MATCH_BAD_PROTOTYPE`` in the summary.  Outputs: the caller's tensors or new
    ones.  Returns ``(match_qv int32 [n], best_qv int32 [n], score_qv fp32 [n], match_full int32 [n_full] or None, score_full
    fp32 [n_full] or None, summary uint8 [2064])`` on the device; ``read_match_summary`` decodes the summary's host copy."""
    dev = _device("feats", feats)
    a = L.FeatureMatchArgs()
    a.feats_dev, a.n = _features("feats", feats)
    if a.n >= 1 << 31:
        raise ValueError(f"feats: {a.n} rows, a call takes fewer than 2^31")
    if not (torch.is_tensor(protos) and protos.device.type == "cuda"):
        host = np.asarray(protos.numpy() if torch.is_tensor(protos) else protos)
        if host.dtype != np.float32 or host.ndim != 2 or host.shape[1] != MATCH_CHANNELS:
            raise ValueError(f"protos must be fp32 [k, {MATCH_CHANNELS}]")
        if not np.isfinite(host).all():
            raise ValueError("protos must be finite")
        if not 1 <= host.shape[0] <= MATCH_MAX_PROTOTYPES:
            raise ValueError(f"protos: k = {host.shape[0]} prototypes, a call takes 1 .. {MATCH_MAX_PROTOTYPES}")
        protos = torch.from_numpy(np.ascontiguousarray(host)).to(dev)
    a.protos_dev, a.k = _features("protos", protos, dev)
    if not 1 <= a.k <= MATCH_MAX_PROTOTYPES:
        raise ValueError(f"protos: k = {a.k} prototypes, a call takes 1 .. {MATCH_MAX_PROTOTYPES}")
    a.proto_class_dev = _ptr("proto_class", proto_class, I32, (a.k,), dev)
    try:
        a.cos_min = float(cos_min)
    except (TypeError, ValueError):
        raise ValueError("cos_min must be a finite number in [0, 1]") from None
    if not 0.0 <= a.cos_min <= 1.0:                     # (NaN fails both)
        raise ValueError("cos_min must be a finite number in [0, 1]")
    a.candidate_dev = _ptr("candidate", candidate, U8, (a.n,), dev, optional=True)
    match_qv, best_qv = _out("match_qv", match_qv, I32, (a.n,), dev), _out("best_qv", best_qv, I32, (a.n,), dev)
    score_qv = _out("score_qv", score_qv, F32, (a.n,), dev)
    if a.n:
        a.match_qv_dev, a.best_qv_dev, a.score_qv_dev = match_qv.data_ptr(), best_qv.data_ptr(), score_qv.data_ptr()
    if inverse_map is not None:
        _ptr("inverse_map", inverse_map, I64, (None,), dev)
        a.n_full = inverse_map.shape[0]
        if a.n_full >= 1 << 31:
            raise ValueError(f"inverse_map: {a.n_full} rows, a call takes fewer than 2^31")
        match_full, score_full = _out("match_full", match_full, I32, (a.n_full,), dev), _out("score_full", score_full, F32, (a.n_full,), dev)
        if a.n_full:
            a.inverse_map_dev, a.match_full_dev, a.score_full_dev = inverse_map.data_ptr(), match_full.data_ptr(), score_full.data_ptr()
    elif match_full is not None or score_full is not None:
        raise ValueError("match_full and score_full belong to the lift: inverse_map is missing")
    summary = _summary(summary, MATCH_SUMMARY.itemsize, dev)
    a.summary_dev = summary.data_ptr()
    L.check(L.load().a3d_feature_match(C.byref(a), L.stream(dev)), "a3d_feature_match")
    return match_qv, best_qv, score_qv, match_full, score_full, summary


# ---- the planes of a scan: Hough votes in integers, fits from integer sums ------------------------------------------------------
PLANE = np.dtype([("normal", "<f4", (3,)), ("offset", "<f4"), ("inliers", "<i4"), ("score", "<i4"), ("round", "<i4"), ("bin", "<i4"),
                  ("count", "<i8"), ("sum", "<i8", (3,)), ("mom", "<i8", (6,)), ("off", "<i8"), ("N", "<i4", (3,)), ("rms", "<f4")])
PLANES_SUMMARY = np.dtype([("n_planes", "<i4"), ("rounds", "<i4"), ("spent", "<i4"), ("admitted", "<i4"), ("left_out", "<i4", (5,)),
                           ("err", "<i4"), ("reserved_", "<i4", (2,))])
PLANES_MAX, PLANES_GRID, PLANES_BINS = L.A3D_PLANES_MAX, L.A3D_PLANES_GRID, L.A3D_PLANES_BINS
PLANES_SCALE = 1 << L.A3D_PLANES_SCALE_BITS     # table entries, N and the units of bin_width / dist_tol: 2^-20 (quanta)
PLANES_MAX_UNITS = 1 << 44                      # the largest bin_width and dist_tol, in those units
PLANES_OUT_BYTES = PLANES_MAX * PLANE.itemsize + PLANES_SUMMARY.itemsize
PLANES_BAD_INDEX = L.A3D_PLANES_BAD_INDEX       # the bit of the summary's error word
PLANES_LEFT_OUT = ("candidate", "nonfinite", "zero_normal", "frame", "bins")      # A3D_PLANES_OUT_*, in order
assert C.sizeof(L.Plane) == PLANE.itemsize == 136 and C.sizeof(L.PlanesSummary) == PLANES_SUMMARY.itemsize == 48
assert C.sizeof(L.PlanesOut) == PLANES_OUT_BYTES == 2224 and C.sizeof(L.FindPlanesArgs) == 168


def read_planes(host):
    """``(records, summary)`` of the host copy of an ``a3d_planes_out`` (uint8 [2224], or anything of those bytes): the
    ``PLANE`` records of the planes found, in the order found (a copy), and the summary as a dict -- ``n_planes``, ``rounds``,
    ``spent``, ``admitted``, ``left_out`` (a dict by ``PLANES_LEFT_OUT``), ``err`` (bit ``PLANES_BAD_INDEX``)."""
    raw = np.ascontiguousarray(host).view(np.uint8).reshape(-1)[:PLANES_OUT_BYTES]
    rec = raw[PLANES_MAX * PLANE.itemsize:].view(PLANES_SUMMARY)[0]
    s = {k: int(rec[k]) for k in ("n_planes", "rounds", "spent", "admitted", "err")}
    s["left_out"] = {name: int(v) for name, v in zip(PLANES_LEFT_OUT, rec["left_out"])}
    return raw[:PLANES_MAX * PLANE.itemsize].view(PLANE)[:s["n_planes"]].copy(), s


def planes_workspace(n, device):
    """The scratch of ``find_planes`` for n rows (``a3d_planes_workspace_bytes``)."""
    return _scratch(L.load().a3d_planes_workspace_bytes(n), device, f"no planes workspace for n={n}")


def direction_table():
    """The HOST's table of ``a3d_find_planes``, int32 [3 G G, 3] (numpy, G = 16): for cell ``(a G + iu) G + iv`` the unit vector
    along ``e_a + u e_b + v e_c`` -- b, c = (a + 1, a + 2) mod 3, u = (2 iu + 1 - G) / G, v likewise -- computed in float64 and
    rounded, ``llrint(component * 2^20)``.  The kernels read it and never normalise."""
    G = PLANES_GRID
    centre = (2.0 * np.arange(G) + 1.0 - G) / G
    table = np.zeros((3, G, G, 3), np.float64)
    for a in range(3):
        table[a, :, :, a] = 1.0
        table[a, :, :, (a + 1) % 3] = centre[:, None]
        table[a, :, :, (a + 2) % 3] = centre[None, :]
    table /= np.sqrt((table * table).sum(-1, keepdims=True))
    return np.rint(table * float(PLANES_SCALE)).astype(np.int32).reshape(3 * G * G, 3)


def planes_settings(quantum, offset_bin, normal_deg, dist_tol, min_voxels, max_planes):
    """``(bin_width, dist_tol_units, cos_min, min_voxels, max_planes)`` as ``a3d_find_planes`` takes them, pure Python:
    ``bin_width = llrint(offset_bin / quantum * 2^20)`` and ``dist_tol_units`` likewise (world units -> 2^-20 quanta, float64,
    rounded once each), ``cos_min = cos(radians(normal_deg))`` in float64, rounded once.  ``ValueError`` for a bin of less
    than one unit or more than 2^44, a tolerance that is negative or more than 2^44, an angle outside 0 .. 90 degrees,
    ``min_voxels < 1`` or ``max_planes`` outside 1 .. 16."""
    q = _power_of_two("quantum", quantum)
    units = []
    for name, value, lo in (("offset_bin", offset_bin, 1), ("dist_tol", dist_tol, 0)):
        try:
            x = float(value)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a finite number") from None
        u = np.rint(np.float64(x) / np.float64(q) * np.float64(PLANES_SCALE)) if np.isfinite(x) else np.nan
        if not lo <= u <= PLANES_MAX_UNITS:              # (a NaN fails both)
            raise ValueError(f"{name}={value!r}: {lo} .. 2^44 units of quantum * 2^-20 are taken")
        units.append(int(u))
    try:
        deg = float(normal_deg)
    except (TypeError, ValueError):
        raise ValueError("normal_deg must be an angle in 0 .. 90 degrees") from None
    if not 0.0 <= deg <= 90.0:
        raise ValueError("normal_deg must be an angle in 0 .. 90 degrees")
    cos_min = min(max(float(np.cos(np.radians(np.float64(deg)))), 0.0), 1.0)
    return (units[0], units[1], cos_min, _int_in("min_voxels", min_voxels, 1, (1 << 31) - 1),
            _int_in("max_planes", max_planes, 1, PLANES_MAX))


def find_planes(normals, positions, origin, quantum, bits=L.A3D_MEASURE_MAX_BITS, offset_bin=None, normal_deg=20.0, dist_tol=None,
                min_voxels=200, max_planes=PLANES_MAX, candidate=None, inverse_map=None, table=None, plane_qv=None,
                plane_full=None, out=None, workspace=None):
    """``a3d_find_planes``: the global planes of the rows ``normals`` fp32 [n, 3] (zeros: no normal) at ``positions`` fp32
    [n, 3], by the rule of include/agile3d_hip.h.  ``origin``, ``quantum``, ``bits``: the fixed-point frame of
    ``measure_objects``.  ``offset_bin`` (the width of an offset bin) and ``dist_tol`` (the inlier distance) in world units --
    both must be given: the session passes the voxel size and 1.5 voxels --, ``normal_deg`` in degrees, ``min_voxels`` (the
    smallest recorded plane), ``max_planes`` 1 .. 16: see ``planes_settings``.  ``candidate`` uint8 [n]: 0 = the row takes no
    part.  ``inverse_map`` int64 [n_full]: also lift the ids to the vertices (``plane_full=False``: not wanted, as without
    a map).  ``table``: ``direction_table()`` on the device as int32 [768, 3] (``None``: uploaded here).  Outputs: the caller's
    tensors or new ones.  Returns ``(plane_qv int32 [n], plane_full int32 [n_full] or None, out uint8 [2224], workspace)`` on the
    device; ``read_planes`` decodes the host copy of ``out``."""
    dev = _device("normals", normals)
    a = L.FindPlanesArgs()
    a.normal_dev = _ptr("normals", normals, F32, (None, 3), dev)
    a.n = n = normals.shape[0]
    a.pos_dev = _ptr("positions", positions, F32, (n, 3), dev)
    a.candidate_dev = _ptr("candidate", candidate, U8, (n,), dev, optional=True)
    a.bits = _int_in("bits", bits, 0, L.A3D_MEASURE_MAX_BITS)
    if n >= 1 << 31 or n << (2 * a.bits) > 1 << 62:
        raise ValueError(f"{n} rows at bits={a.bits}: the sums could overflow (n * 2^(2 bits) <= 2^62)")
    a.origin[:] = _three_finite("origin", origin)
    a.quantum = _power_of_two("quantum", quantum)
    if offset_bin is None or dist_tol is None:
        raise ValueError("offset_bin and dist_tol must be given (world units)")
    a.bin_width, a.dist_tol, a.cos_min, a.min_voxels, a.max_planes = planes_settings(a.quantum, offset_bin, normal_deg, dist_tol,
                                                                                      min_voxels, max_planes)
    if table is None:
        table = torch.from_numpy(direction_table()).to(dev)
    a.table_dev = _ptr("table", table, I32, (3 * PLANES_GRID * PLANES_GRID, 3), dev)
    plane_qv = _out("plane_qv", plane_qv, I32, (n,), dev)
    a.plane_qv_dev = plane_qv.data_ptr() if n else None
    if inverse_map is not None and plane_full is not False:
        _ptr("inverse_map", inverse_map, I64, (None,), dev)
        a.n_full = inverse_map.shape[0]
        if a.n_full >= 1 << 31:
            raise ValueError(f"inverse_map: {a.n_full} rows, a call takes fewer than 2^31")
        plane_full = _out("plane_full", plane_full, I32, (a.n_full,), dev)
        if a.n_full:
            a.inverse_map_dev, a.plane_full_dev = inverse_map.data_ptr(), plane_full.data_ptr()
    elif plane_full is not None and plane_full is not False:
        raise ValueError("plane_full belongs to the lift: inverse_map is missing")
    else:
        plane_full = None
    out = _summary(out, PLANES_OUT_BYTES, dev)
    a.out_dev = out.data_ptr()
    if workspace is None:
        workspace = planes_workspace(n, dev)
    _attach(a, workspace, dev, L.load().a3d_planes_workspace_bytes(n),
            "workspace too small or not 256-byte aligned (planes_workspace(n, device))")
    L.check(L.load().a3d_find_planes(C.byref(a), L.stream(dev)), "a3d_find_planes")
    return plane_qv, plane_full, out, workspace
