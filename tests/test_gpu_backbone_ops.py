"""-m gpu: ``agile3d_amd.backward`` as a marshalling layer -- what the wrappers refuse before the library is reached, that a
column slice of a wider buffer is still served in place, that an input in a layout the kernels cannot read is copied, and
that ``stem_forward`` computes what ``train_backbone._run_stem`` did.  What the kernels compute is the business of
test_gpu_backward.py and test_gpu_train_primitives.py."""
import hashlib
import re

import pytest
import torch

from agile3d_amd import backward as B
from agile3d_amd import lib as L
from agile3d_amd.engine import Scene
from agile3d_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FAMILY = re.compile(r"a3d_(conv_|bn_|stem_|program_|pack_conv)")
KIND, LEVEL, C32 = L.OP_CONV3, 1, 32
SENTINEL = -7.5
# sha256 of what train_backbone._run_stem returned on the seeded scene below before stem_forward replaced it
# (tools/backbone_tape_digest.py prints them; profiles/backbone_ops_bits.txt)
STEM_SHA256 = {125: "891e74b54e9c78ce01b5e503f29c04a05c217df1d16d526a987cac158352f606",
               27: "e7acfe7d17e600ad3eeb59ae5bf6f71f349ac4a4ca8f85f003b2bf0ab68dfa7c"}


@pytest.fixture(scope="module")
def world():
    """One seeded 3000-voxel scene, the caller-ordered colours of its voxels, and a seeded generator's tensors."""
    scn = make_scene(3000, seed=1)
    sc = Scene(torch.from_numpy(scn["coords"]).cuda())
    feats3 = torch.rand(len(scn["coords"]), 3, generator=torch.Generator().manual_seed(2)).cuda()
    sc.prepare_wgrad()
    return sc, feats3


@pytest.fixture
def called():
    """The names of the backbone-training symbols called while the test runs, in order (each call still goes through)."""
    lib, seen = L.load(), []
    orig = {n: getattr(lib, n) for n in L.SYMBOLS if FAMILY.match(n)}
    for n, fn in orig.items():
        setattr(lib, n, lambda *a, _fn=fn, _n=n: (seen.append(_n), _fn(*a))[1])
    yield seen
    for n, fn in orig.items():
        setattr(lib, n, fn)


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def rows_with_zero_row(seed, n, C_):
    t = randn(seed, n + 1, C_)
    t[n] = 0
    return t


def weight(seed, K, cin, cout):
    return randn(seed, K, cin, cout) / (cin * 4) ** 0.5


# ---------------------------------------------------------------------------------------------------- refusals
def _cases(sc):
    """name -> (call taking the tensor under test, a good tensor for it): every wrapper that writes into a caller's tensor,
    on the 3^3 conv 32 -> 32 of level 1 and the BatchNorm behind it."""
    n = sc.n[LEVEL]
    W = weight(1, 27, C32, C32)
    wf, parts = B.pack_weight(W), B.packed_input_grad_weights(KIND, W)
    x, dy = rows_with_zero_row(2, n, C32), rows_with_zero_row(3, n, C32)
    gamma, beta = torch.rand(C32, device=DEV) + 0.5, torch.zeros(C32, device=DEV)
    raw = randn(4, n, C32)
    act, mean, rstd = B.bn_train_forward(raw, gamma, beta, 1e-5, None, True, zero_row=True)
    sums = torch.zeros(2, C32, dtype=torch.float64, device=DEV)
    good = lambda: torch.zeros(n + 1, C32, device=DEV)
    return {
        "conv_apply_acc y": (lambda t: B.conv_apply_acc(sc, KIND, LEVEL, wf, x, C32, C32, t), good()),
        "conv_input_grad_into out": (lambda t: B.conv_input_grad_into(sc, KIND, LEVEL, parts, dy, C32, C32, t), good()),
        "conv_bn_train_forward y": (lambda t: B.conv_bn_train_forward(sc, KIND, LEVEL, wf, x, C32, C32, gamma, beta, 1e-5, None,
                                                                       True, t, None, None, 0.1), good()),
        "conv_dgrad_bn out": (lambda t: B.conv_dgrad_bn(sc, KIND, LEVEL, parts[0], dy, C32, t, False, act, raw, mean, rstd, True),
                              good()),
        "bn_backward_from_sums dx": (lambda t: B.bn_backward_from_sums(raw, dy, gamma, mean, rstd, sums, t), good()),
        "bn_train_backward_into dx": (lambda t: B.bn_train_backward_into(raw, act, dy, gamma, mean, rstd, True, t, good()), good()),
        "bn_train_backward_into dres": (lambda t: B.bn_train_backward_into(raw, act, dy, gamma, mean, rstd, True, good(), t),
                                        good()),
    }


CASE_NAMES = ["conv_apply_acc y", "conv_input_grad_into out", "conv_bn_train_forward y", "conv_dgrad_bn out",
              "bn_backward_from_sums dx", "bn_train_backward_into dx", "bn_train_backward_into dres"]


@pytest.fixture(scope="module")
def cases(world):
    return _cases(world[0])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_wrapper_refuses_a_bad_output_before_the_library(cases, called, name):
    """A float64 tensor, a CPU tensor, one row too few and a channel-strided view as a caller's output: ``ValueError`` that
    names the argument, and no library symbol was reached -- not even a workspace query.  The good tensor goes through."""
    call, good = cases[name]
    arg = name.split()[1]
    wide = torch.zeros(good.shape[0], 2 * good.shape[1], device=DEV)
    bads = {"float64": good.double(), "cpu": good.cpu(), "one row too few": good[:-1], "channel-strided": wide[:, ::2]}
    assert bads["channel-strided"].shape == good.shape and bads["channel-strided"].stride(1) == 2
    for kind, bad in bads.items():
        with pytest.raises(ValueError, match=rf"^{arg} must"):
            call(bad)
        assert called == [], (name, kind)
    call(good)
    assert len([n for n in called if not n.endswith("_workspace_bytes")]) == 1, called
    assert not torch.isnan(good).any()


def test_every_case_is_parametrised(cases):
    assert sorted(cases) == sorted(CASE_NAMES)


# ---------------------------------------------------------------------------------------------------- views served in place
def _in_place(run, rows, total, c0, width):
    """``run(out)`` into columns [c0, c0 + width) of a sentinel-filled [rows, total] buffer against ``run`` into a new
    contiguous tensor: the same bits there, the sentinel everywhere else."""
    fresh = torch.full((rows, width), SENTINEL, device=DEV)
    run(fresh)
    buf = torch.full((rows, total), SENTINEL, device=DEV)
    run(buf[:, c0:c0 + width])
    assert not torch.isnan(fresh).any() and not (fresh == SENTINEL).all()
    assert torch.equal(buf[:, c0:c0 + width], fresh)
    keep = torch.ones(total, dtype=torch.bool, device=DEV)
    keep[c0:c0 + width] = False
    assert (buf[:, keep] == SENTINEL).all()


def test_conv_apply_acc_writes_a_column_slice_in_place(world):
    """96 -> 32 at level 1 into columns [64, 96) of a [n + 1, 96] buffer."""
    sc, n = world[0], world[0].n[LEVEL]
    wf, x = B.pack_weight(weight(5, 27, 96, 32)), rows_with_zero_row(6, n, 96)
    _in_place(lambda out: B.conv_apply_acc(sc, KIND, LEVEL, wf, x, 96, 32, out), n + 1, 96, 64, 32)


def test_conv_input_grad_into_writes_a_column_slice_in_place(world):
    """The input gradient of a 32 -> 96 conv at level 1 (its launch reads 96 channels and writes 32) into columns [64, 96) of
    a [n + 1, 96] buffer."""
    sc, n = world[0], world[0].n[LEVEL]
    parts, dy = B.packed_input_grad_weights(KIND, weight(7, 27, 32, 96)), rows_with_zero_row(8, n, 96)
    assert [(c0, w) for c0, w, _ in parts] == [(0, 32)]
    _in_place(lambda out: B.conv_input_grad_into(sc, KIND, LEVEL, parts, dy, 32, 96, out), n + 1, 96, 64, 32)


def test_conv_input_grad_into_two_slices_in_place(world):
    """cin = 192 at level 2: the smallest case where the slice rule gives more than one launch (128 + 64 columns), into
    columns [32, 224) of a [n + 1, 256] buffer."""
    sc, n = world[0], world[0].n[2]
    parts, dy = B.packed_input_grad_weights(KIND, weight(9, 27, 192, 32)), rows_with_zero_row(10, n, 32)
    assert [(c0, w) for c0, w, _ in parts] == [(0, 128), (128, 64)]
    _in_place(lambda out: B.conv_input_grad_into(sc, KIND, 2, parts, dy, 192, 32, out), n + 1, 256, 32, 192)


def test_an_input_with_a_bad_row_stride_is_copied_not_refused(world):
    """x as the first 32 columns of a [n + 1, 33] buffer (row stride 33 floats: the kernels' vector loads need a multiple of
    4) gives the bits of its contiguous copy."""
    sc, n = world[0], world[0].n[LEVEL]
    wf = B.pack_weight(weight(11, 27, C32, C32))
    x = torch.zeros(n + 1, 33, device=DEV)
    x[:n] = randn(12, n, 33)
    view = x[:, :C32]
    assert view.stride() == (33, 1)
    want = B.conv_apply_acc(sc, KIND, LEVEL, wf, view.contiguous(), C32, C32, torch.empty(n + 1, C32, device=DEV))
    got = B.conv_apply_acc(sc, KIND, LEVEL, wf, view, C32, C32, torch.empty(n + 1, C32, device=DEV))
    assert not torch.isnan(want).any() and torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------- the input convolution
@pytest.mark.parametrize("kvol", [125, 27])
def test_stem_forward_gives_the_bits_run_stem_gave(world, kvol):
    sc, feats3 = world
    w = (torch.randn(kvol, 3, 32, generator=torch.Generator().manual_seed(kvol)) / 6.0).cuda()
    y = B.stem_forward(sc, w, feats3, kvol)
    assert y.shape == (sc.n[0] + 1, 32) and (y[sc.n[0]] == 0).all()
    assert hashlib.sha256(y.contiguous().cpu().numpy().tobytes()).hexdigest() == STEM_SHA256[kvol]
    for bad, arg in ((feats3[:-1], "feats3"), (feats3.double(), "feats3"), (w[:, :, :16], "w"), (w.cpu(), "w")):
        with pytest.raises(ValueError, match=rf"^{arg} must"):
            B.stem_forward(sc, w if arg == "feats3" else bad, bad if arg == "feats3" else feats3, kvol)


# ---------------------------------------------------------------------------------------------------- the library's refusal
def test_a_workspace_query_that_answers_0_raises_the_librarys_message(world, called):
    """The weight gradient's work lists serve channel counts that are multiples of 32: for 48 -> 32
    a3d_conv_wgrad_workspace_bytes answers 0, and the wrapper raises what the library says about it without launching."""
    sc, n = world[0], world[0].n[LEVEL]
    with pytest.raises(L.A3DError, match=r"a3d_conv_wgrad: channels must be multiples of 32 \(got 48 -> 32\)"):
        B.conv_weight_grad(sc, KIND, LEVEL, randn(13, n, 48), randn(14, n, C32))
    assert called == ["a3d_conv_wgrad_workspace_bytes"]
