"""-m gpu: ``agile3d_amd.decoder_ops`` as a marshalling layer -- what the wrappers refuse before the library is reached,
that the caller's outputs and scratch are used and change nothing, and that ``drop`` alone chooses between an entry point
and its ``_dropout`` twin.  What the kernels compute is the business of test_gpu_backward.py, test_gpu_dropout.py,
test_gpu_flash_walk.py and test_gpu_train_primitives.py."""
import re

import pytest
import torch

from agile3d_amd import decoder_ops as ops
from agile3d_amd import lib as L
from attn_kit import DEV, nan, poisoned

pytestmark = pytest.mark.gpu
FAMILY = re.compile(r"a3d_(linear$|flash|attn_|softmax|group_max|next_layer_mask|dropout_rows|dropout_mask|attn_dropout)")
LQ, LK = 3, 5
DROP = L.Dropout(0x5eed, 0.1, 1, 8, 0)


@pytest.fixture
def called():
    """The names of the decoder-training symbols called while the test runs, in order (each call still goes through)."""
    lib, seen = L.load(), []
    orig = {n: getattr(lib, n) for n in L.SYMBOLS if FAMILY.match(n)}
    for n, fn in orig.items():
        setattr(lib, n, lambda *a, _fn=fn, _n=n: (seen.append(_n), _fn(*a))[1])
    yield seen
    for n, fn in orig.items():
        setattr(lib, n, fn)


def launches(seen):
    return [n for n in seen if not n.endswith("_workspace_bytes")]


def test_lib_stream_is_torchs_current_stream():
    side = torch.cuda.Stream()
    for dev in (None, torch.device("cuda"), torch.device("cuda", torch.cuda.current_device())):
        assert (L.stream(dev).value or 0) == torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.stream(side):
            assert (L.stream(dev).value or 0) == side.cuda_stream != 0
    assert L.ptr(None).value is None and L.ptr(side_tensor := torch.zeros(1, device=DEV)).value == side_tensor.data_ptr()
    with pytest.raises((ValueError, RuntimeError)):
        L.stream(torch.device("cpu"))


# ---------------------------------------------------------------------------------------------------- refusals
def z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device=DEV)


def _flash(kind, backward):
    q, k, v = z(LQ, 128), z(LK, 128), z(LK, 128)
    stats, other = ((2, 8, LQ), (LQ, 8, 2)) if kind == "c2s" else ((LQ, 8, 2), (2, 8, LQ))
    a = {("qs" if kind == "c2s" else "q"): q, ("k" if kind == "c2s" else "ks"): k, "v": v}
    bad = {("k" if kind == "c2s" else "ks"): (LK, 64), "v": (LK + 1, 128), "o": (LQ - 1, 128), "stats": other}
    if kind == "c2s":
        a["mask"], bad["mask"] = z(LQ, LK, dtype=torch.uint8), (LQ, LK + 1)
    a.update(o=z(LQ, 128), stats=z(*stats))
    if backward:
        a.update(do=z(LQ, 128), dq=z(LQ, 128), dk=z(LK, 128), dv=z(LK, 128))
        bad.update(do=(LQ + 1, 128), dq=(LQ - 1, 128), dk=(LK - 1, 128), dv=(LK, 127))
    if backward or kind == "c2s":
        a["workspace"], bad["workspace"] = z(1 << 20, dtype=torch.uint8), (1,)
    return getattr(ops, f"flash_{kind}_{'backward' if backward else 'forward'}"), a, bad


def _cases():
    """name -> (wrapper, its good keyword arguments, {tensor argument: a shape it must refuse}).  Every tensor argument is
    also refused as another dtype, non-contiguous and on the CPU; arguments that set the sizes have no wrong extent."""
    G, Q, N = 2, 4, 6
    packed = ops.pack_linear(z(128, 128))
    P = lambda: z(8, LQ, LK)
    i32 = lambda *s: z(*s, dtype=torch.int32)
    c = {
        "linear": (ops.linear, dict(x=z(LQ, 128), packed=packed, bias=z(128), out=z(LQ, 128), res=z(LQ, 128)),
                   dict(x=(LQ, 64), bias=(127,), out=(LQ - 1, 128), res=(LQ, 129))),
        "linear acc": (ops.linear, dict(x=z(LQ, 128), packed=packed, acc=z(LQ, 128)), dict(acc=(LQ + 1, 128))),
        "attn_scores": (ops.attn_scores, dict(a=z(LQ, 128), b=z(LK, 128), scale=0.25, mask=z(LQ, LK, dtype=torch.uint8), out=P()),
                        dict(b=(LK, 64), mask=(LQ, LK + 1), out=(8, LQ - 1, LK))),
        "softmax_rows": (ops.softmax_rows, dict(S=P()), {}),
        "softmax_rows_backward": (ops.softmax_rows_backward, dict(P=P(), dP=P()), dict(dP=(8, LQ, LK + 1))),
        "softmax_cols": (ops.softmax_cols, dict(S=P()), dict(S=(8 * LQ, LK))),
        "softmax_cols_backward": (ops.softmax_cols_backward, dict(P=P(), dP=P()), dict(dP=(8, LQ + 1, LK))),
        "attn_apply": (ops.attn_apply, dict(P=P(), V=z(LK, 128), transposed=False, scale=1.0, out=z(LQ, 128),
                                            workspace=z(1 << 20, dtype=torch.uint8)),
                       dict(V=(LQ, 128), out=(LK, 128),
                            workspace=(0,) if ops.attn_apply_workspace_bytes(LQ, LK, 8, 16, 0) else None)),
        "attn_apply transposed": (ops.attn_apply, dict(P=P(), V=z(LQ, 128), transposed=True, scale=1.0, out=z(LK, 128)),
                                  dict(V=(LK, 128), out=(LQ, 128))),
        "attn_dropout": (ops.attn_dropout, dict(P=P(), transposed=False, drop=DROP, out=P()), dict(out=(8, LK, LQ))),
        "group_max": (ops.group_max, dict(lq=z(N, Q), q_begin=i32(G), q_end=i32(G) + Q, out=z(N, G), arg=i32(N, G)),
                      dict(q_end=(G + 1,), out=(N, G + 1), arg=(N - 1, G))),
        "group_max_backward": (ops.group_max_backward, dict(dy=z(N, G), arg=i32(N, G), n_cols=Q, out=z(N, Q)),
                               dict(arg=(N, G + 1), out=(N, Q + 1))),
        "next_layer_mask": (ops.next_layer_mask, dict(logits=z(N, G), grp_of_query=i32(Q), out=z(Q, N, dtype=torch.uint8),
                                                      workspace=z(1 << 20, dtype=torch.uint8)),
                            dict(out=(N, Q), workspace=(1,))),
        "dropout_rows_forward": (ops.dropout_rows_forward, dict(x=z(LQ, 128), res=z(LQ, 128), relu=True, drop=DROP, out=z(LQ, 128)),
                                 dict(res=(LQ, 64), out=(LQ + 1, 128))),
        "dropout_rows_backward": (ops.dropout_rows_backward, dict(dy=z(LQ, 128), x_pre=z(LQ, 128), drop=DROP, out=z(LQ, 128)),
                                  dict(x_pre=(LQ - 1, 128), out=(LQ, 64))),
        "dropout_mask": (ops.dropout_mask, dict(seed=7, sample=0, site=3, p=0.1, heads=8, rows=LQ, cols=LK,
                                                out=z(8, LQ, LK, dtype=torch.uint8)), dict(out=(8, LK, LQ))),
    }
    for kind in ("c2s", "s2c"):
        for backward in (False, True):
            c[f"flash_{kind}_{'backward' if backward else 'forward'}"] = _flash(kind, backward)
    return c


def _strided(t):
    """``t``'s shape and dtype, every other element of a buffer twice as long: not contiguous."""
    wide = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
    return wide[..., ::2]


@pytest.fixture(scope="module")
def cases():
    return _cases()


CASE_NAMES = ["linear", "linear acc", "attn_scores", "softmax_rows", "softmax_rows_backward", "softmax_cols",
              "softmax_cols_backward", "attn_apply", "attn_apply transposed", "attn_dropout", "group_max", "group_max_backward", "next_layer_mask",
              "dropout_rows_forward", "dropout_rows_backward", "dropout_mask", "flash_c2s_forward", "flash_c2s_backward",
              "flash_s2c_forward", "flash_s2c_backward"]


def test_every_wrapper_has_a_refusal_case(cases):
    assert sorted(cases) == sorted(CASE_NAMES)
    wrapped = {fn.__name__ for fn, _, _ in cases.values()}
    public = {n for n, f in vars(ops).items() if callable(f) and getattr(f, "__module__", "") == ops.__name__ and
              not n.startswith("_")}
    # no tensor of their own to check: built on the wrappers, or sizes in and a byte count out
    composed = {"pack_linear", "dense_forward", "dense_backward", "c2s_forward", "c2s_backward", "s2c_forward", "s2c_backward",
                "flash_c2s_workspace_bytes", "flash_s2c_workspace_bytes", "attn_apply_workspace_bytes"}
    assert public - composed == wrapped


@pytest.mark.parametrize("name", CASE_NAMES)
def test_wrapper_refuses_a_bad_tensor_before_the_library(cases, called, name):
    """A wrong extent, another dtype, a non-contiguous tensor and a CPU tensor, for every tensor argument: ``ValueError`` that
    names the argument, and no entry point was called.  The good arguments do go through (once, at the end)."""
    fn, good, extents = cases[name]
    tried = 0
    for arg, t in good.items():
        if not torch.is_tensor(t):
            continue
        bads = {"dtype": t.double() if t.dtype == torch.float32 else t.float(), "cpu": t.cpu()}
        if not (fn is ops.linear and arg == "x"):          # linear has always taken any x and made it contiguous
            bads["strided"] = _strided(t)
            assert bads["strided"].shape == t.shape and not bads["strided"].is_contiguous()
        if extents.get(arg) is not None:
            bads["extent"] = torch.zeros(extents[arg], dtype=t.dtype, device=DEV)
        for kind, bad in bads.items():
            with pytest.raises(ValueError, match=rf"^{arg} must"):
                fn(**{**good, arg: bad})
            tried += 1
            assert launches(called) == [], (name, arg, kind)
    assert tried >= 3 and set(extents) <= set(good)
    fn(**good)
    assert len(launches(called)) == 1, called


def test_drop_must_be_a_dropout_struct(called):
    x = z(LQ, 128)
    for call in (lambda: ops.dropout_rows_forward(x, None, False, None), lambda: ops.dropout_rows_backward(x, None, None),
                 lambda: ops.attn_dropout(z(8, LQ, LK), False, None),
                 lambda: ops.flash_s2c_forward(z(LQ, 128), z(LK, 128), z(LK, 128), drop=0.1)):
        with pytest.raises(ValueError, match="drop"):
            call()
    assert launches(called) == []


# ---------------------------------------------------------------------------------------------------- the twin is chosen by drop
def test_drop_chooses_the_dropout_twin(called):
    q, k, v, do = (torch.randn(n, 128, device=DEV) for n in (LQ, LK, LK, LQ))
    mask = z(LQ, LK, dtype=torch.uint8)
    want = []
    for drop, tail in ((None, ""), (DROP, "_dropout")):
        o, stats = ops.flash_c2s_forward(q, k, v, mask, drop=drop)
        ops.flash_c2s_backward(q, k, v, mask, o, stats, do, drop=drop)
        o, stats = ops.flash_s2c_forward(q, k, v, drop=drop)
        ops.flash_s2c_backward(q, k, v, o, stats, do, drop=drop)
        want += [f"a3d_flash_{kind}_{way}{tail}" for kind in ("c2s", "s2c") for way in ("forward", "backward")]
    y = ops.dropout_rows_forward(q, None, True, DROP)
    ops.dropout_rows_backward(y, q, DROP)
    assert launches(called) == want + ["a3d_dropout_rows_forward", "a3d_dropout_rows_backward"]


# ---------------------------------------------------------------------------------------------------- caller's outputs
def _qkvw(Lq, Lk):
    g = torch.Generator().manual_seed(100 * Lq + Lk)
    q, k, v, w = (torch.randn(n, 128, generator=g).to(DEV) for n in (Lq, Lk, Lk, Lq))
    mask = torch.rand(Lq, Lk, generator=g) < 0.5
    mask[:, 0] = False                                               # no row fully blocked
    return q, k, v, w, mask.to(torch.uint8).to(DEV)


def _same(a, b):
    for x, y in zip(a, b):
        assert not torch.isnan(x).any() and torch.equal(x, y)


@pytest.mark.parametrize("drop", [None, DROP], ids=["plain", "dropout"])
def test_flash_c2s_into_the_callers_tensors(drop):
    """(Lq, Lk) = (3, 65): one 64-key chunk plus one key.  NaN-filled outputs and a 0xff-filled workspace give the bits of
    the call that allocates everything itself."""
    Lq, Lk = 3, 65
    q, k, v, w, mask = _qkvw(Lq, Lk)
    o0, s0 = ops.flash_c2s_forward(q, k, v, mask, drop=drop)
    g0 = ops.flash_c2s_backward(q, k, v, mask, o0, s0, w, drop=drop)
    ws = poisoned(ops.flash_c2s_workspace_bytes(Lq, Lk))
    o, stats = nan(Lq, 128), nan(2, 8, Lq)
    got = ops.flash_c2s_forward(q, k, v, mask, o=o, stats=stats, workspace=ws, drop=drop)
    assert got[0] is o and got[1] is stats
    _same((o, stats), (o0, s0))
    ws.fill_(255)
    outs = nan(Lq, 128), nan(Lk, 128), nan(Lk, 128)
    got = ops.flash_c2s_backward(q, k, v, mask, o, stats, w, dq=outs[0], dk=outs[1], dv=outs[2], workspace=ws, drop=drop)
    assert all(a is b for a, b in zip(got, outs))
    _same(outs, g0)


@pytest.mark.parametrize("drop", [None, DROP], ids=["plain", "dropout"])
def test_flash_s2c_into_the_callers_tensors(drop):
    """(Lq, Lk) = (65, 3): one 64-point chunk plus one point."""
    Lq, Lk = 65, 3
    q, k, v, w, _ = _qkvw(Lq, Lk)
    o0, s0 = ops.flash_s2c_forward(q, k, v, drop=drop)
    g0 = ops.flash_s2c_backward(q, k, v, o0, s0, w, drop=drop)
    o, stats = nan(Lq, 128), nan(Lq, 8, 2)
    got = ops.flash_s2c_forward(q, k, v, o=o, stats=stats, drop=drop)
    assert got[0] is o and got[1] is stats
    _same((o, stats), (o0, s0))
    outs = nan(Lq, 128), nan(Lk, 128), nan(Lk, 128)
    got = ops.flash_s2c_backward(q, k, v, o, stats, w, dq=outs[0], dk=outs[1], dv=outs[2],
                                 workspace=poisoned(ops.flash_s2c_workspace_bytes(Lq, Lk)), drop=drop)
    assert all(a is b for a, b in zip(got, outs))
    _same(outs, g0)


@pytest.mark.parametrize("drop", [None, DROP], ids=["plain", "dropout"])
def test_dense_pair_into_the_callers_tensors(drop):
    q, k, v, w, mask = _qkvw(LQ, LK)
    o0, saved0 = ops.dense_forward(q, k, v, mask, drop=drop)
    g0 = ops.dense_backward(q, k, v, mask, o0, saved0, w, drop=drop)
    o = nan(LQ, 128)
    got, saved = ops.dense_forward(q, k, v, mask, o, drop)
    assert got is o and saved[1] is False
    _same((o, saved[0]), (o0, saved0[0]))
    outs = nan(LQ, 128), nan(LK, 128), nan(LK, 128)
    got = ops.dense_backward(q, k, v, mask, o, saved, w, *outs, drop)
    assert all(a is b for a, b in zip(got, outs))
    _same(outs, g0)
    # the pieces with a poisoned workspace: attn_apply both ways
    for transposed, V, rows in ((False, v, LQ), (True, q, LK)):
        ws = poisoned(max(1, ops.attn_apply_workspace_bytes(LQ, LK, 8, 16, transposed)))
        _same([ops.attn_apply(saved[0], V, transposed, 0.5, nan(rows, 128), workspace=ws)],
              [ops.attn_apply(saved[0], V, transposed, 0.5)])

