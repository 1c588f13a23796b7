"""The training primitives on their own, at the shapes where their kernels change path: the nn.Linear weight / bias
gradient (csrc/wgrad.hip), the dense attention pieces (csrc/attn_train.hip), LayerNorm and BatchNorm(train)
(csrc/bnorm.hip).  The whole-network gradient tests reach these kernels at one scene and one click layout, with
tolerances scaled by a parameter's largest gradient; a tail, one template instantiation or one output layout can be wrong
there without a test noticing.

Every reference is float64 torch / numpy on the CPU from seeded generators.  Quantities the project already bounds reuse
that bound (named at the assertion).  Softmax, softmax backward and BatchNorm on offset data have no project bound: there
the kernel is allowed FOUR times the error torch's own float32 CPU implementation of the same expression makes against
the float64 reference on the same inputs, plus 1e-7 (an exact float32 result must not make the bound zero; the factor of
four covers a different but valid summation order) -- ``_derived_bound``.
"""
import numpy as np
import pytest
import torch

from agile3d_amd import backward as B
from agile3d_amd import decoder_ops as ops
from agile3d_amd import lib as L
from agile3d_amd.lib import ptr as _ptr

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _err(got, ref):
    return (got.detach().cpu().double() - ref.detach().double()).abs().max().item()


def _derived_bound(name, kernel, f32, ref):
    """-> (kernel error, bound) with bound = 4 x (error of torch's float32 CPU result) + 1e-7; prints the figures."""
    e32, ek = _err(f32, ref), _err(kernel, ref)
    print(f"[derived] {name}: float32-CPU error {e32:.3e}  kernel error {ek:.3e}  ratio " + (f"{ek / e32:.2f}" if e32 > 0 else "-"))
    return ek, 4.0 * e32 + 1e-7


def _scratch(nbytes):
    """Workspace that starts out as NaN patterns: a kernel that reads scratch nothing wrote shows up in the result."""
    return torch.full((int(nbytes),), 255, dtype=torch.uint8, device="cuda")


# ------------------------------------------------------------------------------------------------------------------
# 1. a3d_linear_wgrad_into / a3d_linear_wgrad
# ------------------------------------------------------------------------------------------------------------------
# all 16 pairs of {32, 64, 96, 128}: 13 of them select the 13 builds of k_wgrad, (96,128), (128,96) and (128,128) repeat a
# build with two channel blocks, the FFN shapes (128,1024) / (1024,128) with sixteen -- the table is pinned by
# test_wgrad_plan_host.py::test_the_build_table_of_the_gpu_modules
PAIRS = [(ci, co) for ci in (32, 64, 96, 128) for co in (32, 64, 96, 128)] + [(128, 1024), (1024, 128)]
BUILD_PAIRS = [p for p in PAIRS[:16] if p not in ((96, 128), (128, 96), (128, 128))]
# one partial group, exactly one group, a group plus one row, fewer groups than the four waves, several segments
ROW_EDGES = [(ci, co, n) for ci, co in ((128, 128), (96, 128)) for n in (1, 15, 16, 17, 63, 65, 4099)]
# EXACT cases: x and dy are integers in [-3, 3], the seeded dW / db integers in [-8, 8], so every sum in any order is an integer
# below 2^24 (the largest: 4099 x 9 + 8) and float32 arithmetic is exact: the assertion is bit equality with float64
EXACT_CASES = ROW_EDGES + [(ci, co, 65) for ci, co in BUILD_PAIRS]
WGRAD_CASES = ([pytest.param(ci, co, n, False, id=f"{ci}-{co}-{n}") for ci, co, n in [(ci, co, 1000) for ci, co in PAIRS] + ROW_EDGES] +
               [pytest.param(ci, co, n, True, id=f"exact-{ci}-{co}-{n}") for ci, co, n in EXACT_CASES])
LAYOUT_PAIRS = [(128, 128), (96, 64), (32, 96)]


def _wgrad_inputs(cin, cout, n, exact=False):
    g = torch.Generator().manual_seed(1000 * cin + cout + 7 * n)
    if exact:
        x, dy = (torch.randint(-3, 4, (n, c), generator=g).float() for c in (cin, cout))
        old_w, old_b = torch.randint(-8, 9, (cin, cout), generator=g).float(), torch.randint(-8, 9, (cout,), generator=g).float()
        assert n * 9 + 8 < 2 ** 24
        return x, dy, old_w, old_b, x.double().t() @ dy.double(), dy.double().sum(0)
    x = torch.randn(n, cin, generator=g)
    dy = torch.randn(n, cout, generator=g)
    old_w = torch.randn(cin, cout, generator=g) * 3 + 0.5      # what an accumulating call finds ([cin, cout] orientation)
    old_b = torch.randn(cout, generator=g) * 3 - 0.5
    return x, dy, old_w, old_b, x.double().t() @ dy.double(), dy.double().sum(0)


def _wgrad_into(x, dy, n, cin, cout, dw, ld_dw, transposed, accumulate, db, db_accumulate):
    """The entry point itself: x / dy / dw are views with unit channel stride, leading dimensions taken from them."""
    lib = L.load()
    nbytes = lib.a3d_linear_wgrad_into_workspace_bytes(n, cin, cout)
    assert nbytes, lib.a3d_last_error().decode()
    ws = _scratch(nbytes)
    L.check(lib.a3d_linear_wgrad_into(_ptr(x), x.stride(0), _ptr(dy), dy.stride(0), n, cin, cout, _ptr(dw), ld_dw,
                                      transposed, accumulate, _ptr(db), db_accumulate, _ptr(ws), nbytes, None),
            "a3d_linear_wgrad_into")


def _wgrad_plain(x, dy, n, cin, cout):
    lib = L.load()
    nbytes = lib.a3d_linear_wgrad_workspace_bytes(n, cin, cout)
    assert nbytes, lib.a3d_last_error().decode()
    ws = _scratch(nbytes)
    dw = torch.full((cin, cout), NAN, device="cuda")
    L.check(lib.a3d_linear_wgrad(_ptr(x), x.stride(0), _ptr(dy), dy.stride(0), n, cin, cout, _ptr(dw), _ptr(ws), nbytes,
                                 None), "a3d_linear_wgrad")
    return dw


@pytest.mark.parametrize("cin,cout,n,exact", WGRAD_CASES)
def test_linear_wgrad_into_every_output_mode(cin, cout, n, exact):
    """dW = x^T dy and db = sum_rows dy against float64, for transposed x accumulate x db in {absent, assigned, added}.
    An assigning call finds NaN in its destination, an accumulating one seeded values (expected: old + new).  Bound: the
    project's linear-weight-gradient bound 2e-4 max(1, |ref|max), for db (a sum over the same n rows, produced by the same
    pass) with its own reference's scale; the EXACT cases (integer operands) allow no error at all, in both entry points and
    every output mode.  The plain a3d_linear_wgrad must agree with ``_into`` (transposed = 0, accumulate = 0) within the same
    bound, and a repeated call must reproduce dW and db bit for bit."""
    x, dy, old_w, old_b, ref_w, ref_b = _wgrad_inputs(cin, cout, n, exact)
    xd, dyd = x.cuda(), dy.cuda()
    tol_w = 0.0 if exact else 2e-4 * max(1.0, ref_w.abs().max().item())
    tol_b = 0.0 if exact else 2e-4 * max(1.0, ref_b.abs().max().item())
    plain_into = None
    for transposed in (0, 1):
        for accumulate in (0, 1):
            for db_mode in ("absent", "assign", "accumulate"):
                start = old_w if accumulate else torch.full((cin, cout), NAN)
                dw = (start.t() if transposed else start).contiguous().cuda()
                want_w = ref_w + old_w.double() if accumulate else ref_w
                db = None
                if db_mode != "absent":
                    db = (old_b.clone() if db_mode == "accumulate" else torch.full((cout,), NAN)).cuda()
                _wgrad_into(xd, dyd, n, cin, cout, dw, cin if transposed else cout, transposed, accumulate, db,
                            int(db_mode == "accumulate"))
                got = dw.t() if transposed else dw
                where = (cin, cout, n, transposed, accumulate, db_mode)
                assert _err(got, want_w) <= tol_w, where
                if db is not None:
                    want_b = ref_b + old_b.double() if db_mode == "accumulate" else ref_b
                    assert _err(db, want_b) <= tol_b, where
                if not transposed and not accumulate and db_mode == "absent":
                    plain_into = dw
    plain = _wgrad_plain(xd, dyd, n, cin, cout)
    assert _err(plain, ref_w) <= tol_w
    assert _err(plain, plain_into.cpu()) <= tol_w
    twice = []
    for _ in range(2):
        dw, db = torch.full((cout, cin), NAN, device="cuda"), torch.full((cout,), NAN, device="cuda")
        _wgrad_into(xd, dyd, n, cin, cout, dw, cin, 1, 0, db, 0)
        twice.append((dw, db))
    assert torch.equal(twice[0][0], twice[1][0]) and torch.equal(twice[0][1], twice[1][1])
    assert torch.equal(_wgrad_plain(xd, dyd, n, cin, cout), plain)


@pytest.mark.parametrize("cin,cout", LAYOUT_PAIRS)
@pytest.mark.parametrize("transposed", [0, 1])
def test_linear_wgrad_into_writes_only_its_block_of_a_wider_matrix(cin, cout, transposed):
    """ld_dw wider than a row (a row slice of a packed in_proj matrix, a column slice here): dW is a [rows, cols] block
    at column 32 of a NaN-filled [rows, cols + 64] buffer.  The block is right and every element outside it is still NaN,
    assigned and accumulated."""
    n = 1000
    x, dy, old_w, old_b, ref_w, ref_b = _wgrad_inputs(cin, cout, n)
    rows, cols = (cout, cin) if transposed else (cin, cout)
    tol_w = 2e-4 * max(1.0, ref_w.abs().max().item())
    for accumulate in (0, 1):
        wide = torch.full((rows, cols + 64), NAN)
        if accumulate:
            wide[:, 32:32 + cols] = old_w.t() if transposed else old_w
        wide = wide.cuda()
        block = wide[:, 32:32 + cols]
        db = torch.full((cout,), NAN, device="cuda")
        _wgrad_into(x.cuda(), dy.cuda(), n, cin, cout, block, cols + 64, transposed, accumulate, db, 0)
        got = block.t() if transposed else block
        assert _err(got, ref_w + old_w.double() if accumulate else ref_w) <= tol_w, accumulate
        assert _err(db, ref_b) <= 2e-4 * max(1.0, ref_b.abs().max().item())
        assert torch.isnan(wide[:, :32]).all() and torch.isnan(wide[:, 32 + cols:]).all(), accumulate


@pytest.mark.parametrize("cin,cout", LAYOUT_PAIRS)
def test_linear_wgrad_reads_column_slices_of_wider_operands(cin, cout):
    """ldx / ldy wider than the channel count (even, the documented requirement): x = [:, 32:] of [n, cin + 32], dy =
    [:, 2:cout + 2] of [n, cout + 6]; everything outside the slices is NaN, so a read outside them poisons the result."""
    n = 65
    x, dy, _, _, ref_w, ref_b = _wgrad_inputs(cin, cout, n)
    xw, dyw = torch.full((n, cin + 32), NAN), torch.full((n, cout + 6), NAN)
    xw[:, 32:], dyw[:, 2:cout + 2] = x, dy
    xw, dyw = xw.cuda(), dyw.cuda()
    xs, dys = xw[:, 32:], dyw[:, 2:cout + 2]
    tol_w = 2e-4 * max(1.0, ref_w.abs().max().item())
    dw, db = torch.full((cout, cin), NAN, device="cuda"), torch.full((cout,), NAN, device="cuda")
    _wgrad_into(xs, dys, n, cin, cout, dw, cin, 1, 0, db, 0)
    assert _err(dw.t(), ref_w) <= tol_w
    assert _err(db, ref_b) <= 2e-4 * max(1.0, ref_b.abs().max().item())
    assert _err(_wgrad_plain(xs, dys, n, cin, cout), ref_w) <= tol_w


# ------------------------------------------------------------------------------------------------------------------
# 2. dense attention primitives
# ------------------------------------------------------------------------------------------------------------------
def _keep_one_finite(mask, dim):
    """Unblock the first position of every fully blocked row: such a row is NaN in torch too and is not what these tests
    are about."""
    full = mask.all(dim=dim, keepdim=True)
    first = torch.zeros_like(mask)
    first.select(dim, 0).fill_(True)
    return mask & ~(full & first)


def _softmax_inputs(shape, dim, masked, seed):
    g = torch.Generator().manual_seed(seed)
    S = torch.randn(shape, generator=g) * 4        # probabilities over several orders of magnitude
    dP = torch.randn(shape, generator=g)
    blocked = None
    if masked:
        blocked = _keep_one_finite(torch.rand(shape, generator=g) < 0.5, dim)
        assert (~blocked).any(dim=dim).all()       # every row keeps a finite entry
        S = S.masked_fill(blocked, float("-inf"))
    return S, dP, blocked


def _softmax_check(name, S, dP, blocked, dim, forward, backward):
    ref = torch.softmax(S.double(), dim)
    assert torch.isfinite(ref).all()
    got = forward(S.cuda())
    ek, bound = _derived_bound(name + " softmax", got, torch.softmax(S, dim), ref)
    assert ek <= bound, (name, ek, bound)
    if blocked is not None:
        assert (got.cpu()[blocked] == 0).all()
    # backward on the float64 probabilities rounded to float32: dS = P (dP - sum P dP)
    P = ref.float()
    ref_b = P.double() * (dP.double() - (P.double() * dP.double()).sum(dim, keepdim=True))
    f32_b = P * (dP - (P * dP).sum(dim, keepdim=True))
    got_b = backward(P.cuda(), dP.cuda())
    ek, bound = _derived_bound(name + " softmax backward", got_b, f32_b, ref_b)
    assert ek <= bound, (name, ek, bound)
    if blocked is not None:
        assert (got_b.cpu()[blocked] == 0).all()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Lk", [1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025])
def test_softmax_rows_and_backward_around_the_lane_strides_and_the_512_switch(Lk, masked):
    """a3d_softmax_rows / _backward on 24 rows (8 heads x 3): one wave per row below L = 512 (lanes stride over the row,
    ``per`` = ceil(L / 64) values per lane), one workgroup per row from 512.  ``masked``: about half of each row is -inf
    and must come out exactly 0, forward and backward.  Bound: ``_derived_bound``.

    Measured on an MI355X, largest over the 24 cases (float32-CPU error / kernel error; largest ratio of a single case):
      softmax            2.96e-07 / 2.13e-07   ratio <= 2.31 (L = 63: 7.2e-08 / 1.67e-07)
      softmax backward   1.90e-07 / 2.73e-07   ratio <= 2.04 (L = 128 masked: 6.9e-08 / 1.40e-07)"""
    S, dP, blocked = _softmax_inputs((24, Lk), 1, masked, 31 * Lk + masked)
    _softmax_check(f"rows L={Lk} masked={masked}", S, dP, blocked, 1, ops.softmax_rows, ops.softmax_rows_backward)


@pytest.mark.parametrize("Lq", [1, 3, 20])
@pytest.mark.parametrize("Lk", [1, 255, 257, 3000])
def test_softmax_cols_and_backward(Lq, Lk):
    """a3d_softmax_cols / _backward: the softmax over the MIDDLE dimension of [H, Lq, Lk] (scene-to-click attention keeps
    its scores transposed), one thread per (head, column), around the 256-thread workgroup edge.  Bound:
    ``_derived_bound``.

    Measured on an MI355X, largest over the 12 cases (float32-CPU error / kernel error; largest ratio of a single case):
      softmax            4.91e-07 / 4.91e-07   ratio <= 1.00
      softmax backward   7.64e-07 / 9.73e-07   ratio <= 1.36 (Lq = 20, Lk = 255)"""
    S, dP, _ = _softmax_inputs((8, Lq, Lk), 1, False, 97 * Lq + Lk)
    _softmax_check(f"cols Lq={Lq} Lk={Lk}", S, dP, None, 1, ops.softmax_cols, ops.softmax_cols_backward)


VALUE_FAMILIES = ("pm80", "peak60")


def _far_from_zero(S, blocked, dim, family, seed):
    """Scores of a peaked attention instead of 4 randn.  pm80: every entry within a few units of +80 or of -80 (half of the
    softmax underflows to exactly 0); peak60: the LAST unblocked entry along ``dim`` 60 above the largest other one (its
    weight is 1 to float32, every other one about e^-60)."""
    g = torch.Generator().manual_seed(seed + 7)
    opened = torch.ones_like(S, dtype=torch.bool) if blocked is None else ~blocked
    if family == "pm80":
        T = (torch.rand(S.shape, generator=g) < 0.5).float() * 160.0 - 80.0 + torch.randn(S.shape, generator=g)
    else:
        assert family == "peak60"
        T = torch.randn(S.shape, generator=g) * 4
        shape = [1] * S.dim()
        shape[dim] = S.shape[dim]
        last = (opened * torch.arange(S.shape[dim]).view(shape)).max(dim, keepdim=True)[1]
        top = T.masked_fill(~opened, float("-inf")).max(dim, keepdim=True)[0]
        T.scatter_(dim, last, top + 60.0)
        assert bool(opened.gather(dim, last).all())
    return T if blocked is None else T.masked_fill(blocked, float("-inf"))


@pytest.mark.parametrize("family", VALUE_FAMILIES)
@pytest.mark.parametrize("Lk", [129, 513])
def test_softmax_rows_and_backward_far_from_zero(Lk, family):
    """a3d_softmax_rows / _backward, masked, on both sides of the 512 switch, on the score families of ``_far_from_zero``
    (the other cases: 4 randn).  Bound: ``_derived_bound``, as there.

    Measured on an MI355X over the 4 cases: kernel error / float32-CPU error <= 1.06 (L = 513 pm80 backward: 7.1e-09 /
    6.7e-09); peak60 is exact to the reference's 1.7e-32."""
    S, dP, blocked = _softmax_inputs((24, Lk), 1, True, 31 * Lk + 1)
    S = _far_from_zero(S, blocked, 1, family, 31 * Lk + 1)
    _softmax_check(f"rows L={Lk} {family}", S, dP, blocked, 1, ops.softmax_rows, ops.softmax_rows_backward)


@pytest.mark.parametrize("family", VALUE_FAMILIES)
@pytest.mark.parametrize("Lq,Lk", [(20, 255), (3, 3000)])
def test_softmax_cols_and_backward_far_from_zero(Lq, Lk, family):
    """a3d_softmax_cols / _backward on the score families of ``_far_from_zero``.  Bound: ``_derived_bound``.

    Measured on an MI355X over the 4 cases: kernel error / float32-CPU error <= 1.02 (Lq = 20, Lk = 255 pm80: 9.2e-08 /
    9.1e-08)."""
    S, dP, _ = _softmax_inputs((8, Lq, Lk), 1, False, 97 * Lq + Lk)
    S = _far_from_zero(S, None, 1, family, 97 * Lq + Lk)
    _softmax_check(f"cols Lq={Lq} Lk={Lk} {family}", S, dP, None, 1, ops.softmax_cols, ops.softmax_cols_backward)


@pytest.mark.parametrize("family", VALUE_FAMILIES)
@pytest.mark.parametrize("Lq,Lk,H,dh", [(20, 1500, 8, 16), (1500, 7, 8, 16)])
def test_attn_scores_far_from_zero(Lq, Lk, H, dh, family):
    """a3d_attn_scores (k_tr_scores_long by key and by query) on operands whose scores reach +-80 (pm80: q scaled), or
    whose last key scores 60 above every other key of its row (peak60: channel 0 of every head is a for the queries, b for
    that key and 0 for the others).  The bars of test_attn_scores_with_a_mask: 1e-4 absolute, blocked entries -inf.

    Measured on an MI355X: max|diff| 1.1e-05 / 9.7e-06 (pm80), 2.1e-05 / 3.2e-05 (peak60, scores up to 71)."""
    g = torch.Generator().manual_seed(Lq * 7 + Lk)
    q, k = torch.randn(Lq, H * dh, generator=g), torch.randn(Lk, H * dh, generator=g)
    mask = (torch.rand(Lq, Lk, generator=g) < 0.3)
    scale = dh ** -0.5

    def scores():
        return scale * torch.einsum("ihd,jhd->hij", q.double().view(Lq, H, dh), k.double().view(Lk, H, dh))
    if family == "pm80":
        q *= 80.0 / scores().abs().max().item()
        assert 79.0 <= scores().abs().max().item() <= 81.0
    else:
        q[:, 0::dh], k[:, 0::dh] = 0.0, 0.0
        ref = scores()
        lead = (ref.max(-1)[0] - ref[:, :, -1]).max().item() + 60.01
        q[:, 0::dh], k[-1, 0::dh] = (lead / scale) ** 0.5, (lead / scale) ** 0.5
        ref = scores()
        assert (ref[:, :, -1] - ref[:, :, :-1].max(-1)[0]).min().item() >= 60.0
    S = torch.full((H, Lq, Lk), NAN, device="cuda")
    ops.attn_scores(q.cuda(), k.cuda(), scale, mask.to(torch.uint8).cuda(), out=S, heads=H)
    ref = scores()
    S = S.cpu()
    blocked = mask.expand(H, Lq, Lk)
    err = (S[~blocked].double() - ref[~blocked]).abs().max().item()
    print(f"attn_scores {Lq}x{Lk} {family}: max|score| {ref.abs().max().item():.0f}, max|diff| {err:.2e}")
    assert (S[blocked] == float("-inf")).all()
    assert err <= 1e-4


@pytest.mark.parametrize("Lq,Lk,H,dh", [(20, 20, 8, 16), (5, 300, 8, 16), (20, 1500, 8, 16), (1500, 7, 8, 16),
                                        (1100, 9, 1, 128)])
def test_attn_scores_with_a_mask(Lq, Lk, H, dh):
    """a3d_attn_scores with its uint8 mask (~30 % blocked): the thread-per-element kernel, k_tr_scores_long by key and by
    query, and its dh = 128 build.  Unblocked entries against float64 einsum to the project's 1e-4, blocked ones are -inf."""
    g = torch.Generator().manual_seed(Lq * 7 + Lk)
    q, k = torch.randn(Lq, H * dh, generator=g), torch.randn(Lk, H * dh, generator=g)
    mask = (torch.rand(Lq, Lk, generator=g) < 0.3)
    scale = dh ** -0.5
    S = torch.full((H, Lq, Lk), NAN, device="cuda")
    q_d, k_d, mask_d = q.cuda(), k.cuda(), mask.to(torch.uint8).cuda()
    ops.attn_scores(q_d, k_d, scale, mask_d, out=S, heads=H)
    ref = scale * torch.einsum("ihd,jhd->hij", q.double().view(Lq, H, dh), k.double().view(Lk, H, dh))
    S = S.cpu()
    blocked = mask.expand(H, Lq, Lk)
    assert (S[blocked] == float("-inf")).all()
    assert (S[~blocked].double() - ref[~blocked]).abs().max().item() <= 1e-4


@pytest.mark.parametrize("Lq,Lk,H,dh,transposed", [(1, 1, 8, 16, 0), (1, 1, 8, 16, 1), (17, 17, 8, 16, 0), (17, 17, 8, 16, 1),
                                                   (200, 200, 8, 16, 0), (200, 200, 8, 16, 1), (30, 1100, 1, 128, 1)])
def test_attn_apply_at_the_self_attention_sizes(Lq, Lk, H, dh, transposed):
    """a3d_attn_apply where nothing is split: k_tr_apply / k_tr_apply_t at the click-to-click sizes and
    k_tr_apply_t_head<128>, against float64 einsum to the project's 2e-5 max(1, |ref|max)."""
    g = torch.Generator().manual_seed(Lq + 3 * Lk + transposed)
    P = torch.softmax(torch.randn(H, Lq, Lk, generator=g) * 2, -1)
    rows_in, rows_out = (Lq, Lk) if transposed else (Lk, Lq)
    V = torch.randn(rows_in, H * dh, generator=g)
    out = torch.full((rows_out, H * dh), NAN, device="cuda")
    ops.attn_apply(P.cuda(), V.cuda(), transposed, 0.5, out,
                   workspace=_scratch(ops.attn_apply_workspace_bytes(Lq, Lk, H, dh, transposed)))
    eq = "hij,ihd->jhd" if transposed else "hij,jhd->ihd"
    ref = 0.5 * torch.einsum(eq, P.double(), V.double().view(rows_in, H, dh)).reshape(rows_out, H * dh)
    assert _err(out, ref) <= 2e-5 * max(1.0, ref.abs().max().item())


def _group_max_inputs(N):
    """-> (lq [N, 12], qbeg, qend, expected max [N, 4], expected first arg max [N, 4]) with tied maxima (CPU only)."""
    Q, sizes = 12, (1, 1, 3, 7)
    qbeg = np.cumsum((0,) + sizes[:-1]).astype(np.int32)
    qend = (qbeg + np.array(sizes)).astype(np.int32)
    G = len(sizes)
    rng = np.random.default_rng(N)
    lq = rng.standard_normal((N, Q)).astype(np.float32)
    tied = rng.random(N) < 0.1
    tied[0] = True
    for g in range(G):
        if sizes[g] < 2:
            continue
        seg = lq[:, qbeg[g]:qend[g]]                    # a view
        top = seg.argmax(1)
        other = (top + rng.integers(1, sizes[g], N)) % sizes[g]
        rows = np.nonzero(tied)[0]
        seg[rows, other[rows]] = seg[rows, top[rows]]
        assert ((seg == seg.max(1, keepdims=True)).sum(1) >= 2).any()      # the group has a tied maximum
    ref_out = np.stack([lq[:, qbeg[g]:qend[g]].max(1) for g in range(G)], 1)
    ref_arg = np.stack([qbeg[g] + lq[:, qbeg[g]:qend[g]].argmax(1) for g in range(G)], 1).astype(np.int32)
    return lq, qbeg, qend, ref_out, ref_arg


@pytest.mark.parametrize("N", [1, 255, 4097])
def test_group_max_and_its_backward_pick_the_first_maximum(N):
    """a3d_group_max / _backward: Q = 12 queries in contiguous groups of 1, 1, 3 and 7 (all non-empty).  At about a tenth
    of the points (point 0 always) the group's largest value is copied to another query of the group, so the maximum is
    tied; values and indices must equal numpy's max / argmax (first occurrence) exactly, and the backward must put every
    dout on that index and exact zeros elsewhere."""
    lq, qbeg, qend, ref_out, ref_arg = _group_max_inputs(N)
    Q, G = lq.shape[1], len(qbeg)
    rng = np.random.default_rng(N + 1)
    lq_d = torch.from_numpy(lq).cuda()
    out = torch.full((N, G), NAN, device="cuda")
    arg = torch.full((N, G), -1, dtype=torch.int32, device="cuda")
    qbeg_d, qend_d = torch.from_numpy(qbeg).cuda(), torch.from_numpy(qend).cuda()
    ops.group_max(lq_d, qbeg_d, qend_d, out=out, arg=arg)
    assert np.array_equal(out.cpu().numpy(), ref_out) and np.array_equal(arg.cpu().numpy(), ref_arg)
    dout = rng.standard_normal((N, G)).astype(np.float32)
    ref_dlq = np.zeros((N, Q), np.float32)
    np.put_along_axis(ref_dlq, ref_arg.astype(np.int64), dout, 1)
    dlq = torch.full((N, Q), NAN, device="cuda")
    dout_d = torch.from_numpy(dout).cuda()
    ops.group_max_backward(dout_d, arg, Q, out=dlq)
    assert np.array_equal(dlq.cpu().numpy(), ref_dlq)


# ------------------------------------------------------------------------------------------------------------------
# 3. LayerNorm beyond C = 128 contiguous
# ------------------------------------------------------------------------------------------------------------------
def _wide(t, ld, off):
    """t [n, C] as columns off .. off + C of a NaN-filled [n, ld] buffer on the GPU -> (buffer, view)."""
    buf = torch.full((t.shape[0], ld), NAN)
    buf[:, off:off + t.shape[1]] = t
    buf = buf.cuda()
    return buf, buf[:, off:off + t.shape[1]]


def _untouched(buf, off, width):
    return bool(torch.isnan(buf[:, :off]).all() and torch.isnan(buf[:, off + width:]).all())


# (C, ld of x / dx, column offset, ld of y, offset, ld of dy, offset)
_LN_GENERIC = [(C_, C_ + 6, 3, C_ + 2, 1, C_ + 10, 5) for C_ in (64, 192, 256, 512)]
_LN_130 = (128, 130, 1, 130, 1, 130, 1)             # the generic kernels at the decoder's width
_LN_132 = (128, 132, 4, 132, 4, 132, 4)             # the 128 kernels on strided rows
_LN_DENSE = (128, 128, 0, 128, 0, 128, 0)
LN_CASES = ([(lay, n) for lay in _LN_GENERIC + [_LN_130] for n in (1, 3, 4, 5, 1000)] +
            [(_LN_132, n) for n in (1, 3, 4, 5, 17, 1000)] +
            [(_LN_DENSE, n) for n in (1, 15, 16, 17, 511, 513)])


@pytest.mark.parametrize("layout,n", LN_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_layernorm_generic_widths_and_strided_rows(layout, n):
    """a3d_layernorm_forward / _backward against float64 layer_norm and autograd, to the project's bounds (y 1e-5, dx 2e-5
    of scale, dgamma / dbeta 1e-4 of scale): the generic kernels at C = 64 .. 512 and at C = 128 with a leading dimension
    that is no multiple of 4, the C = 128 kernels on strided rows and at their 16-rows-per-workgroup / 512-row-block edges.
    x, y, dy and dx are column slices of NaN-filled buffers: nothing outside the slices of y and dx may be written."""
    lib = L.load()
    C_, ldx, ox, ldy, oy, lddy, ody = layout
    g = torch.Generator().manual_seed(C_ * 13 + n + ldx)
    x = torch.randn(n, C_, generator=g) * 1.7 + 0.3
    gamma, beta = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g)
    dy = torch.randn(n, C_, generator=g)
    xd, gd, bd = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    y_ref = torch.nn.functional.layer_norm(xd, (C_,), gd, bd, 1e-5)
    y_ref.backward(dy.double())
    _, xv = _wide(x, ldx, ox)
    _, dyv = _wide(dy, lddy, ody)
    ybuf, yv = _wide(torch.full((n, C_), NAN), ldy, oy)
    dxbuf, dxv = _wide(torch.full((n, C_), NAN), ldx, ox)          # dx has the layout of x
    gam, bet = gamma.cuda(), beta.cuda()
    L.check(lib.a3d_layernorm_forward(_ptr(xv), ldx, n, C_, _ptr(gam), _ptr(bet), 1e-5, _ptr(yv), ldy, None),
            "a3d_layernorm_forward")
    assert _err(yv, y_ref) <= 1e-5
    assert _untouched(ybuf, oy, C_)
    dgamma, dbeta = torch.full((C_,), NAN, device="cuda"), torch.full((C_,), NAN, device="cuda")
    nbytes = lib.a3d_bn_workspace_bytes(n, C_)
    ws = _scratch(nbytes)
    L.check(lib.a3d_layernorm_backward(_ptr(xv), ldx, _ptr(dyv), lddy, n, C_, _ptr(gam), 1e-5, _ptr(dxv), _ptr(dgamma),
                                       _ptr(dbeta), _ptr(ws), nbytes, None), "a3d_layernorm_backward")
    assert _err(dxv, xd.grad) <= 2e-5 * max(1.0, xd.grad.abs().max().item())
    assert _untouched(dxbuf, ox, C_)
    assert _err(dgamma, gd.grad) <= 1e-4 * max(1.0, gd.grad.abs().max().item())
    assert _err(dbeta, bd.grad) <= 1e-4 * max(1.0, bd.grad.abs().max().item())


# ------------------------------------------------------------------------------------------------------------------
# 4. BatchNorm (train) at row-block edges and on offset data
# ------------------------------------------------------------------------------------------------------------------
def _bn_inputs(n, C_):
    """Seeded inputs of a BatchNorm case.  Any float32 BatchNorm loses eps_f32 |x| rstd in y (more in dx), without limit
    as a column's variance goes to zero, so the project's fixed bounds presuppose columns that are not nearly constant;
    with two rows a random column is one a few times in a hundred.  The first seed n + C + 1000 k whose smallest column
    variance is at least 1e-3 is used -- a property of the input alone (k = 0 for every n >= 511 here)."""
    for k in range(200):
        g = torch.Generator().manual_seed(n + C_ + 1000 * k)
        x = (torch.randn(n, C_, generator=g) * 2 + 0.5)
        if x.double().var(0, unbiased=False).min().item() < 1e-3:
            continue
        res = torch.randn(n, C_, generator=g)
        gamma, beta = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g)
        rm, rv = torch.randn(C_, generator=g) * 0.1, torch.rand(C_, generator=g) + 0.5
        return x, res, gamma, beta, rm, rv, torch.randn(n, C_, generator=g)
    raise AssertionError("no well-conditioned seed")


@pytest.mark.parametrize("n,C_", [(n, C_) for C_ in (32, 96) for n in (2, 3, 511, 512, 513, 1025)] + [(524_289 + 1024, 32)])
def test_batchnorm_training_at_row_block_edges(n, C_):
    """BatchNorm(train) + residual + ReLU and its backward where the row blocks of bn_blocks end (512 rows per block), at
    two and three rows (the unbiased running variance divides by n - 1), and past the 1024-block cap, where a block has
    more than 512 rows and the last one is short.  Reference and bounds: those of
    test_batchnorm_training_forward_backward_vs_torch (float64 batch_norm + autograd on the CPU)."""
    x, res, gamma, beta, rm, rv, dy = _bn_inputs(n, C_)
    xd, gd, bd = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    rd = res.double().requires_grad_()
    rm_ref, rv_ref = rm.double().clone(), rv.double().clone()
    y_ref = torch.relu(torch.nn.functional.batch_norm(xd, rm_ref, rv_ref, gd, bd, training=True, momentum=0.02, eps=1e-5) + rd)
    y_ref.backward(dy.double())
    rm_d, rv_d = rm.cuda(), rv.cuda()
    x_d, dy_d, gam = x.cuda(), dy.cuda(), gamma.cuda()
    y, mean, rstd = B.bn_train_forward(x_d, gam, beta.cuda(), 1e-5, res.cuda(), True, rm_d, rv_d, 0.02)
    assert _err(y, y_ref) <= 2e-5
    assert _err(rm_d, rm_ref) <= 1e-6 and _err(rv_d, rv_ref) <= 1e-5
    dx, dgamma, dbeta, dres = B.bn_train_backward(x_d, y, dy_d, gam, mean, rstd, True, True)
    assert _err(dx, xd.grad) <= 5e-5 * max(1.0, xd.grad.abs().max().item())
    assert _err(dgamma, gd.grad) <= 2e-4 * max(1.0, gd.grad.abs().max().item())
    assert _err(dbeta, bd.grad) <= 2e-4 * max(1.0, bd.grad.abs().max().item())
    assert _err(dres, rd.grad) <= 1e-6


@pytest.mark.parametrize("n,C_", [(5000, 64), (513, 32)])
def test_batchnorm_training_on_data_far_from_zero(n, C_):
    """x = 100 + 0.05 randn: a column mean 2000 times its spread, what the merge of per-block (count, mean, M2) in
    k_bn_combine exists for (E[x^2] - E[x]^2 has no correct digit here).  save_mean, save_rstd sqrt(var + eps) (1 in exact
    arithmetic) and y against float64; bound: ``_derived_bound`` with torch's float32 CPU batch norm on the same input.

    This test found a first-order loss in the merge: with the block sums taken of x itself, an fp32 sum of 500 values
    near 100 is off by 1e-2, and Chan's between-block term carries that error into the variance.  Measured on an MI355X
    before the fix, float32-CPU error / kernel error: (5000, 64) save_mean 2.14e-5 / 7.56e-6, save_rstd sqrt(var + eps)
    3.30e-7 / 3.83e-6 (ratio 11.6, over the bound).  k_bn_block_stats now sums x - row 0; a float32 emulation of the
    kernel's arithmetic on the CPU, which reproduces the figures above to the last bit, then gives (5000, 64) save_mean
    3.71e-6, save_rstd 1.11e-7 (ratio 0.34), y 5.0e-4 / 9.6e-5; (513, 32) save_mean 1.04e-5 / 3.72e-6, save_rstd 1.19e-7 /
    9.5e-8 (before: 1.34e-5), y 3.4e-4 / 9.6e-5.  Figures are printed with ``pytest -s``."""
    g = torch.Generator().manual_seed(n * 3 + C_)
    x = 100 + 0.05 * torch.randn(n, C_, generator=g)
    gamma, beta = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g)
    xd = x.double()
    mean_ref = xd.mean(0)
    var_ref = ((xd - mean_ref) ** 2).mean(0)
    y_ref = (xd - mean_ref) / torch.sqrt(var_ref + 1e-5) * gamma.double() + beta.double()
    y32, mean32, rstd32 = torch.native_batch_norm(x, gamma, beta, None, None, True, 0.1, 1e-5)
    y, mean, rstd = B.bn_train_forward(x.cuda(), gamma.cuda(), beta.cuda(), 1e-5)
    sd = torch.sqrt(var_ref + 1e-5)
    one = torch.ones(C_, dtype=torch.float64)
    for name, got, f32, ref in (("save_mean", mean, mean32, mean_ref),
                                ("save_rstd sqrt(var + eps)", rstd.cpu().double() * sd, rstd32.double() * sd, one),
                                ("y", y, y32, y_ref)):
        ek, bound = _derived_bound(f"batchnorm offset n={n} C={C_} {name}", got, f32, ref)
        assert ek <= bound, (name, ek, bound)


def test_batchnorm_zero_row_adds_one_zero_row_and_changes_nothing_else():
    """zero_row = True (what feeds a3d_conv_apply): y, dx and dres get row n, exactly zero; rows 0 .. n - 1 are those of
    the call without it, bit for bit."""
    n, C_ = 513, 96
    g = torch.Generator().manual_seed(5)
    x, res = (torch.randn(n, C_, generator=g) * 2 + 0.5).cuda(), torch.randn(n, C_, generator=g).cuda()
    gamma, beta = (torch.rand(C_, generator=g) + 0.5).cuda(), torch.randn(C_, generator=g).cuda()
    dy = torch.randn(n, C_, generator=g).cuda()
    y0, mean0, rstd0 = B.bn_train_forward(x, gamma, beta, 1e-5, res, True)
    y1, mean1, rstd1 = B.bn_train_forward(x, gamma, beta, 1e-5, res, True, zero_row=True)
    assert y1.shape == (n + 1, C_) and (y1[n] == 0).all() and torch.equal(y1[:n], y0)
    assert torch.equal(mean0, mean1) and torch.equal(rstd0, rstd1)
    dx0, dg0, db0, dres0 = B.bn_train_backward(x, y0, dy, gamma, mean0, rstd0, True, True)
    dx1, dg1, db1, dres1 = B.bn_train_backward(x, y1, dy, gamma, mean1, rstd1, True, True, zero_row=True)
    assert dx1.shape == (n + 1, C_) and (dx1[n] == 0).all() and torch.equal(dx1[:n], dx0)
    assert dres1.shape == (n + 1, C_) and (dres1[n] == 0).all() and torch.equal(dres1[:n], dres0)
    assert torch.equal(dg0, dg1) and torch.equal(db0, db1)


# the four SyncBN pieces on one GPU, no process group: two rows, one row past a 512-row block, three blocks + a one-row tail
SYNCBN_CASES = [(n, C_) for C_ in (32, 96) for n in (2, 513, 1025)]
# 4 x the largest error measured over SYNCBN_CASES (see the docstring below), relative to max(1, |ref|max)
SYNCBN_MEAN_TOL, SYNCBN_M2_TOL = 4 * 6.326e-08, 4 * 1.409e-07


def _syncbn_backward_apply(lib, x, y, dy, n, C_, gamma, mean, rstd, glob, n_global, local, zero_row):
    """a3d_bn_backward_apply (ReLU on, residual gradient wanted) into NaN-filled outputs -> (dx, dres, dgamma, dbeta)."""
    dx, dres = (torch.full((n + zero_row, C_), NAN, device="cuda") for _ in range(2))
    dgamma, dbeta = torch.full((C_,), NAN, device="cuda"), torch.full((C_,), NAN, device="cuda")
    L.check(lib.a3d_bn_backward_apply(_ptr(x), C_, _ptr(y), C_, _ptr(dy), C_, n, C_, _ptr(gamma), _ptr(mean), _ptr(rstd), 1,
                                      _ptr(glob), n_global, _ptr(local), _ptr(dx), C_, _ptr(dres), C_, _ptr(dgamma),
                                      _ptr(dbeta), zero_row, None), "a3d_bn_backward_apply")
    return dx, dres, dgamma, dbeta


@pytest.mark.parametrize("n,C_", SYNCBN_CASES)
def test_syncbn_pieces_on_one_gpu(n, C_):
    """a3d_bn_local_stats, a3d_bn_apply, a3d_bn_backward_sums and a3d_bn_backward_apply called through the library with
    no process group (the two-rank run of test_gpu_distributed.py is the only other GPU test that reaches them), on
    ``_bn_inputs``, with residual and ReLU.

    Forward: local statistics, the host combination of bn_sync_forward for one rank, then a3d_bn_apply.  y against float64
    batch_norm to the 2e-5 of test_batchnorm_training_at_row_block_edges.  stats[0:C] / stats[C:2C] against the float64
    mean / sum of squared deviations: no project bound, so 4 x the largest error measured on an MI355X over these six
    cases, relative to max(1, |ref|max) (the margin covers seed-to-seed variation of an fp32 block sum).  Measured:
      (n, C)      mean       M2            (n, C)      mean       M2
      (2, 32)     2.674e-08  6.849e-08     (2, 96)     5.099e-08  1.178e-07
      (513, 32)   5.670e-08  1.409e-07     (513, 96)   6.326e-08  9.154e-08
      (1025, 32)  5.007e-08  8.369e-08     (1025, 96)  5.545e-08  1.273e-07
    so the bounds are 4 x 6.326e-08 for the mean and 4 x 1.409e-07 for the sum of squared deviations (``pytest -s`` prints
    the figures).
    Backward with n_global = n: dx, dres, dgamma and dbeta equal a3d_bn_train_backward's bit for bit (the same three
    kernels in the same order).  Backward with n_global = 2 n and twice the local sums (two identical ranks): dx against
    float64 gamma rstd (g - sum g / 2n - xhat sum g xhat / 2n) to the 5e-5 max(1, |dx|max) of the test above, dgamma /
    dbeta the local sums.  zero_row = 1: row n of y, dx and dres is zero, the rows before it unchanged bit for bit."""
    lib = L.load()
    x, res, gamma, beta, _, _, dy = _bn_inputs(n, C_)
    xd = x.double()
    mean_ref = xd.mean(0)
    m2_ref = ((xd - mean_ref) ** 2).sum(0)
    y_ref = torch.relu(torch.nn.functional.batch_norm(xd, None, None, gamma.double(), beta.double(), training=True, eps=1e-5) +
                       res.double())
    x_d, res_d, dy_d, gam, bet = x.cuda(), res.cuda(), dy.cuda(), gamma.cuda(), beta.cuda()
    nbytes = lib.a3d_bn_workspace_bytes(n, C_)

    # forward
    st = torch.full((2 * C_ + 1,), NAN, dtype=torch.float64, device="cuda")
    ws = _scratch(nbytes)
    L.check(lib.a3d_bn_local_stats(_ptr(x_d), C_, n, C_, _ptr(st), _ptr(ws), nbytes, None), "a3d_bn_local_stats")
    e_mean = _err(st[:C_], mean_ref) / max(1.0, mean_ref.abs().max().item())
    e_m2 = _err(st[C_:2 * C_], m2_ref) / max(1.0, m2_ref.abs().max().item())
    print(f"[syncbn] n={n} C={C_}: local_stats mean error {e_mean:.3e}  M2 error {e_m2:.3e}  (relative to max(1, |ref|max))")
    assert e_mean <= SYNCBN_MEAN_TOL and e_m2 <= SYNCBN_M2_TOL, (e_mean, e_m2)
    st[2 * C_] = float(n)
    allst = st[None]                                             # bn_sync_forward's combination, world = 1
    cnt = allst[:, 2 * C_:2 * C_ + 1]
    n_glob = cnt.sum()
    mean = (allst[:, :C_] * cnt).sum(0) / n_glob
    m2 = (allst[:, C_:2 * C_] + cnt * (allst[:, :C_] - mean) ** 2).sum(0)
    mean_f = mean.to(torch.float32)
    rstd = 1.0 / torch.sqrt((m2 / n_glob).to(torch.float32) + 1e-5)
    ys = []
    for zero_row in (0, 1):
        y = torch.full((n + zero_row, C_), NAN, device="cuda")
        L.check(lib.a3d_bn_apply(_ptr(x_d), C_, n, C_, _ptr(gam), _ptr(bet), _ptr(mean_f), _ptr(rstd), _ptr(res_d), C_, 1,
                                 _ptr(y), C_, zero_row, None), "a3d_bn_apply")
        ys.append(y)
    y = ys[0]
    assert _err(y, y_ref) <= 2e-5
    assert (ys[1][n] == 0).all() and torch.equal(ys[1][:n], y)

    # backward, n_global = n: the pieces against the one-call entry point
    local = torch.full((2 * C_,), NAN, dtype=torch.float64, device="cuda")
    ws = _scratch(nbytes)
    L.check(lib.a3d_bn_backward_sums(_ptr(x_d), C_, _ptr(y), C_, _ptr(dy_d), C_, n, C_, _ptr(mean_f), _ptr(rstd), 1, _ptr(local),
                                     _ptr(ws), nbytes, None), "a3d_bn_backward_sums")
    pieces = _syncbn_backward_apply(lib, x_d, y, dy_d, n, C_, gam, mean_f, rstd, local, n, local, 0)
    whole = [torch.full((n, C_), NAN, device="cuda") for _ in range(2)] + [torch.full((C_,), NAN, device="cuda") for _ in range(2)]
    ws = _scratch(nbytes)
    L.check(lib.a3d_bn_train_backward(_ptr(x_d), C_, _ptr(y), C_, _ptr(dy_d), C_, n, C_, _ptr(gam), _ptr(mean_f), _ptr(rstd), 1,
                                      _ptr(whole[0]), C_, _ptr(whole[1]), C_, _ptr(whole[2]), _ptr(whole[3]), 0, _ptr(ws), nbytes,
                                      None), "a3d_bn_train_backward")
    for name, a, b in zip(("dx", "dres", "dgamma", "dbeta"), pieces, whole):
        assert torch.equal(a, b), name
    with_row = _syncbn_backward_apply(lib, x_d, y, dy_d, n, C_, gam, mean_f, rstd, local, n, local, 1)
    for name, a, b in zip(("dx", "dres"), with_row, pieces):
        assert (a[n] == 0).all() and torch.equal(a[:n], b), name
    assert torch.equal(with_row[2], pieces[2]) and torch.equal(with_row[3], pieces[3])

    # backward, n_global = 2 n: two identical ranks
    dx2, dres2, dgamma2, dbeta2 = _syncbn_backward_apply(lib, x_d, y, dy_d, n, C_, gam, mean_f, rstd, 2.0 * local, 2 * n, local, 0)
    rstd_ref = 1.0 / torch.sqrt(m2_ref / n + 1e-5)
    g = dy.double() * (y_ref > 0)
    xhat = (xd - mean_ref) * rstd_ref
    dx_ref = gamma.double() * rstd_ref * (g - 2.0 * g.sum(0) / (2 * n) - xhat * (2.0 * (g * xhat).sum(0)) / (2 * n))
    assert _err(dx2, dx_ref) <= 5e-5 * max(1.0, dx_ref.abs().max().item())
    assert torch.equal(dres2, pieces[1])
    assert torch.equal(dbeta2, local[:C_].float()) and torch.equal(dgamma2, local[C_:].float())


@pytest.mark.parametrize("n", [1, 512, 513])
def test_column_sums_at_row_block_edges(n):
    """a3d_column_sums against the float64 sum to the project's 1e-3, bit-equal when repeated."""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, 96, generator=g)
    s = B.column_sums(x.cuda())
    assert _err(s, x.double().sum(0)) <= 1e-3
    assert torch.equal(B.column_sums(x.cuda()), s)
