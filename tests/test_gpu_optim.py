"""-m gpu: the last steps of a training iteration -- the gradient-norm clip and the AdamW update (csrc/optim.hip,
agile3d_amd/optim.py) -- against tests/optim_ref.py's float64 restatement, at the chunk / table / block edges of the
multi-tensor kernels and through the single-tensor entry points of include/agile3d_hip.h.

Every AdamW comparison is over ONE step: the fp32 state before the step goes into adamw_step64 as it is, so drift never
enters a bound.  Bounds (from a numpy fp32 emulation of the kernels' arithmetic against adamw_step64 over 200k elements,
t in {1, 2, 3, 10, 1000}, lr in {1e-4, 1e-3, 2e-3}, gradient scales 1e-12 .. 100: worst 3.5 units, 1.6e-7, 2.8e-7;
2-4 x headroom for FMA contraction on the device):
    p           |p_dev - p64| <= P_UNITS * (ulp32(|p_before|) + 1e-6 * |delta|), delta the float64 update term
    exp_avg     <= M_REL * (b1 * |m_before| + (1 - b1) * |g * scale|)
    exp_avg_sq  <= V_REL * v64
The norm: 1e-12 relative to sum_squares64 of the same fp32 values (fp64 accumulation in a fixed order)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from agile3d_amd import lib as L
from agile3d_amd.optim import MT_CHUNK, AdamW, _mt_layout, _to_device, clip_grad_norm_, total_grad_norm
from optim_ref import adamw_step64, clip_coef, sum_squares64, ulp32

pytestmark = pytest.mark.gpu

P_UNITS = 8.0     # worst on the MI355X over this module: 2.05 (error / (ulp32 + 1e-6 |delta|))
M_REL = 1e-6      # worst on the MI355X: 1.85e-7
V_REL = 1e-6      # worst on the MI355X: 2.99e-7 (1.30e-5 while the kernels formed 1.f - beta2 from the fp32 beta2)
NORM_REL = 1e-12  # worst on the MI355X: 5.98e-15

HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
GUARD = 64
SENTINEL = -12345.678
WORST = {"p": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0, "norm": 0.0}    # over the module's run, printed at its end (-s)


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    print(f"\nworst over test_gpu_optim: p {WORST['p']:.2f} units (<= {P_UNITS:g}), exp_avg {WORST['exp_avg']:.2e} "
          f"(<= {M_REL:g}), exp_avg_sq {WORST['exp_avg_sq']:.2e} (<= {V_REL:g}), norm {WORST['norm']:.2e} (<= {NORM_REL:g})")


def _np(t):
    return t.detach().cpu().numpy().copy()


def _check_step(before, g, after, t, hp, scale, what):
    """before / after: (p, m, v) fp32 numpy arrays around one step of number ``t``; g: the fp32 gradient as the kernel
    read it.  Asserts the three bounds, -> the worst (p units, m relative, v relative)."""
    p64, m64, v64, delta = adamw_step64(before[0], g, before[1], before[2], t, hp["lr"], hp["betas"], hp["eps"],
                                        hp["weight_decay"], scale)
    b1 = hp["betas"][0]
    g64 = np.asarray(g, np.float64) * scale
    bound = (ulp32(before[0]) + 1e-6 * np.abs(delta),
             b1 * np.abs(before[1].astype(np.float64)) + (1.0 - b1) * np.abs(g64),
             v64)
    limit = (P_UNITS, M_REL, V_REL)
    worst = []
    for name, got, ref, b, lim in zip(("p", "exp_avg", "exp_avg_sq"), after, (p64, m64, v64), bound, limit):
        err = np.abs(got.astype(np.float64) - ref).ravel()
        b = b.ravel()
        ratio = float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0), initial=0.0))
        worst.append(ratio)
        WORST[name] = max(WORST[name], ratio)
        bad = err > lim * b
        assert not bad.any(), (what, name, t, f"{int(bad.sum())} of {err.size} outside the bound, worst ratio {ratio:.3e} "
                               f"(limit {lim:g}), max |err| {float(err.max()):.3e}")
    return tuple(worst)


def _carve(sizes, fill):
    """One flat buffer holding a slice per entry of ``sizes`` with GUARD sentinel floats before, between and after:
    -> (buffer, list of slices (views), boolean mask of the guard positions)."""
    total = GUARD + sum(n + GUARD for n in sizes)
    buf = torch.full((total,), SENTINEL, dtype=torch.float32, device="cuda")
    guard = torch.ones(total, dtype=torch.bool)
    views, off = [], GUARD
    for n in sizes:
        views.append(buf[off:off + n])
        guard[off:off + n] = False
        off += n + GUARD
    for view in views:
        view.copy_(fill(view.numel()))
    return buf, views, guard.cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sizes_270():
    rng = np.random.default_rng(270)
    sizes = [1, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 3 * 4096]
    sizes += rng.choice([1, 96, 128, 27 * 32 * 32, 4096, 4097], size=259).tolist()
    rng.shuffle(sizes)
    return [int(n) for n in sizes]


@pytest.fixture(scope="module")
def world270():
    """270 tensors as slices of four guarded flat buffers, two warm-up steps taken (so both moments are non-zero)."""
    gen = torch.Generator().manual_seed(270)
    sizes = _sizes_270()
    names = [f"t{i:03d}" for i in range(len(sizes))]
    pbuf, ps, guard = _carve(sizes, lambda n: torch.randn(n, generator=gen))
    mbuf, ms, _ = _carve(sizes, lambda n: torch.zeros(n))
    vbuf, vs, _ = _carve(sizes, lambda n: torch.zeros(n))
    gbuf, gs, _ = _carve(sizes, lambda n: torch.zeros(n))
    opt = AdamW(zip(names, ps), **HP)
    for k, m, v in zip(names, ms, vs):
        opt.state[k] = (m, v)                 # AdamW.step only creates the state that is missing
    for _ in range(2):
        for g in gs:
            g.copy_(torch.randn(g.numel(), generator=gen) * 10.0 ** float(torch.randint(-4, 2, (1,), generator=gen)))
        opt.step(dict(zip(names, gs)), 0.5)
    torch.cuda.synchronize()
    assert all(opt.state[k][0].data_ptr() == m.data_ptr() for k, m in zip(names, ms))
    return dict(sizes=sizes, names=names, opt=opt, gen=gen, guard=guard,
                bufs=dict(p=pbuf, m=mbuf, v=vbuf, g=gbuf), views=dict(p=ps, m=ms, v=vs, g=gs))


def test_adamw_chunk_and_table_edges(world270):
    """(a) one launch over 270 interleaved one-chunk and multi-chunk tensors (mt_find 8-9 levels deep), sizes at every
    edge of the 4096-element chunk and the 256-thread stride: every tensor inside the bounds, nothing written outside
    the tensors, the gradients untouched."""
    w = world270
    sizes, names, opt, gen = w["sizes"], w["names"], w["opt"], w["gen"]
    assert len(sizes) == 270 and sum((n + MT_CHUNK - 1) // MT_CHUNK > 1 for n in sizes) > 20
    for g in w["views"]["g"]:
        g.copy_(torch.randn(g.numel(), generator=gen) * 10.0 ** float(torch.randint(-4, 2, (1,), generator=gen)))
    before = {q: [_np(x) for x in w["views"][q]] for q in "pmv"}
    flat_before = {q: w["bufs"][q].clone() for q in "pmvg"}
    scale = 0.37
    opt.step(dict(zip(names, w["views"]["g"])), scale)
    torch.cuda.synchronize()
    worst = np.zeros(3)
    for i, k in enumerate(names):
        assert opt.steps[k] == 3
        after = tuple(_np(w["views"][q][i]) for q in "pmv")
        got = _check_step(tuple(before[q][i] for q in "pmv"), _np(w["views"]["g"][i]), after, 3, HP, scale, (k, sizes[i]))
        worst = np.maximum(worst, got)
        assert not np.array_equal(after[0], before["p"][i])
    print(f"\n270 tensors, worst p {worst[0]:.2f} units (<= {P_UNITS}), exp_avg {worst[1]:.2e} (<= {M_REL}), "
          f"exp_avg_sq {worst[2]:.2e} (<= {V_REL})")
    for q in "pmv":
        assert torch.equal(_bits(w["bufs"][q])[w["guard"]], _bits(flat_before[q])[w["guard"]]), f"guard zone of {q} written"
    assert torch.equal(_bits(w["bufs"]["g"]), _bits(flat_before["g"])), "the gradient buffer was written"


def test_per_parameter_step_counts():
    """(b) parameters that skip steps count their own updates (torch's state['step']); the gradient dict comes in reverse
    order of the parameters."""
    gen = torch.Generator().manual_seed(6)
    shapes = [(5000,), (96,), (3, 4097), (1,), (128, 96), (4096,)]
    names = [f"p{i}" for i in range(6)]
    ref_p = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in shapes]
    dev_p = {k: r.detach().clone().cuda() for k, r in zip(names, ref_p)}
    ref_opt = torch.optim.AdamW(ref_p, **HP)
    opt = AdamW(dev_p.items(), **HP)
    skipped = {1: {5}, 2: {2}, 4: {2}}
    for step in range(1, 6):
        skip = skipped.get(step, set())
        grads = {}
        for i in reversed(range(6)):
            g = torch.randn(shapes[i], generator=gen) * 0.1
            ref_p[i].grad = None if i in skip else g
            if i not in skip:
                grads[names[i]] = g.cuda()
        frozen = {i: [_bits(x).clone() for x in (dev_p[names[i]],) + tuple(opt.state.get(names[i], ()))] for i in skip}
        ref_opt.step()
        opt.step(grads)
        torch.cuda.synchronize()
        for i, k in enumerate(names):
            want = int(float(ref_opt.state[ref_p[i]]["step"])) if ref_opt.state[ref_p[i]] else 0
            assert opt.steps.get(k, 0) == want, (step, k)
            assert (dev_p[k].cpu() - ref_p[i].detach()).abs().max().item() <= 1e-6, (step, k)
        for i, old in frozen.items():
            now = (dev_p[names[i]],) + tuple(opt.state.get(names[i], ()))
            assert len(now) == len(old) and all(torch.equal(_bits(a), b) for a, b in zip(now, old)), (step, i)
    assert [opt.steps[k] for k in names] == [5, 5, 3, 5, 5, 4]
    assert opt.step_count == 5


def _warm(shapes, gen, hp=HP, steps=2):
    names = [f"w{i}" for i in range(len(shapes))]
    params = {k: torch.randn(s, generator=gen).cuda() for k, s in zip(names, shapes)}
    opt = AdamW(params.items(), **hp)
    for _ in range(steps):
        opt.step({k: (torch.randn(s, generator=gen) * 0.3).cuda() for k, s in zip(names, shapes)})
    return names, params, opt


def _snapshot(opt, k):
    return (_np(opt.params[k]),) + tuple(_np(x) for x in opt.state[k])


def test_gradient_forms():
    """(c) a (1, 128) gradient for a (128,) parameter, a transposed view as gradient (through the clip and without it),
    a zero-element parameter."""
    gen = torch.Generator().manual_seed(12)
    shapes = [(128,), (96, 130), (0,), (257,)]
    names, params, opt = _warm(shapes, gen)
    assert names[2] not in opt.state and opt.steps.get(names[2], 0) == 0
    for use_clip in (True, False):
        raw = {names[0]: torch.randn(1, 128, generator=gen).cuda(),
               names[1]: torch.randn(130, 96, generator=gen).cuda().t(),
               names[2]: torch.zeros(0).cuda(),
               names[3]: torch.randn(257, generator=gen).cuda()}
        assert not raw[names[1]].is_contiguous()
        dense = {k: _np(g).reshape(params[k].shape) for k, g in raw.items()}
        before = {k: _snapshot(opt, k) for k in names if k != names[2]}
        grads = dict(raw)
        coef = 1.0
        if use_clip:
            norm, coef = clip_grad_norm_(grads, 0.1)
            want = math.sqrt(sum_squares64(*dense.values()))
            assert abs(norm - want) <= NORM_REL * want
            assert coef == clip_coef(norm, 0.1) and coef < 1.0
        t = opt.steps[names[0]] + 1
        opt.step(grads, coef)
        torch.cuda.synchronize()
        for k in before:
            assert opt.steps[k] == t
            _check_step(before[k], dense[k], _snapshot(opt, k), t, HP, coef, (k, use_clip))
        assert names[2] not in opt.state and names[2] not in opt.steps
    only_empty = {names[2]: torch.zeros(0).cuda()}
    assert total_grad_norm(only_empty) == 0.0
    opt.step(only_empty)


def test_layout_cache_follows_parameters_and_state():
    """(d) the cached table is rebuilt when a parameter moves, and dropped by load_state_dict."""
    gen = torch.Generator().manual_seed(13)
    shapes = [(4097,), (96,), (27, 32, 32)]
    names, params, opt = _warm(shapes, gen, steps=1)
    k = names[0]
    old = opt.params[k]
    opt.params[k] = old.clone()
    assert opt.params[k].data_ptr() != old.data_ptr()
    old_bits = _bits(old).clone()
    grads = {n: (torch.randn(s, generator=gen) * 0.3).cuda() for n, s in zip(names, shapes)}
    before = {n: _snapshot(opt, n) for n in names}
    opt.step(grads)
    torch.cuda.synchronize()
    for n in names:
        _check_step(before[n], _np(grads[n]), _snapshot(opt, n), 2, HP, 1.0, n)
    assert torch.equal(_bits(old), old_bits), "the tensor that left the optimiser was written"

    twin = AdamW({n: p.clone() for n, p in opt.params.items()}.items(), lr=9.0, betas=(0.5, 0.5), eps=1.0, weight_decay=9.0)
    twin.load_state_dict(opt.state_dict())
    assert (twin.lr, twin.betas, twin.eps, twin.weight_decay) == (opt.lr, tuple(opt.betas), opt.eps, opt.weight_decay)
    assert twin.steps == opt.steps
    grads = {n: (torch.randn(s, generator=gen) * 0.3).cuda() for n, s in zip(names, shapes)}
    opt.step(grads, 0.7)
    twin.step({n: g.clone() for n, g in grads.items()}, 0.7)
    torch.cuda.synchronize()
    for n in names:
        assert twin.steps[n] == opt.steps[n] == 3
        assert torch.equal(twin.params[n], opt.params[n]), n
        assert torch.equal(twin.state[n][0], opt.state[n][0]) and torch.equal(twin.state[n][1], opt.state[n][1]), n
        assert twin.params[n].data_ptr() != opt.params[n].data_ptr()


def _norm_case(grads):
    want = math.sqrt(sum_squares64(*[_np(g) for g in grads.values()]))
    got = total_grad_norm(grads)
    again = total_grad_norm(grads)
    assert math.isfinite(got) and got == again, (got, again)
    rel = abs(got - want) / want
    WORST["norm"] = max(WORST["norm"], rel)
    assert rel <= NORM_REL, (got, want, rel)
    return got


def test_norm_of_270_tensors(world270):
    """(e.1) the gradients of (a): every chunk edge, tensors interleaved."""
    _norm_case(dict(zip(world270["names"], world270["views"]["g"])))


def test_norm_more_than_1024_chunks():
    """(e.2) 1030 chunks: the final reduction's per-thread loop runs twice for the first threads."""
    n = 1029 * 4096 + 5
    g = torch.randn(n, generator=torch.Generator().manual_seed(14)).cuda()
    assert _mt_layout([n])[1] == 1030
    _norm_case({"g": g})


def test_norm_of_huge_values_stays_finite():
    """(e.3) squares of 1e50 overflow an fp32 accumulator, not the fp64 one."""
    g = torch.randn(5000, generator=torch.Generator().manual_seed(15))
    g[[0, 77, 4097, 4999]] = torch.tensor([1e25, -1e25, 1e25, -1e25])
    norm = _norm_case({"a": g[:4100].cuda(), "b": g[4100:].cuda()})
    assert 1.9e25 < norm < 2.1e25


def test_norm_zero_and_no_clipping():
    """(e.4, e.5) all-zero gradients; max_norm <= 0 switches the clip off."""
    zeros = {"a": torch.zeros(4097).cuda(), "b": torch.zeros(3, 5).cuda()}
    assert total_grad_norm(zeros) == 0.0
    assert clip_grad_norm_(zeros, 0.1) == (0.0, 1.0)
    g = {"a": torch.full((300,), 2.0).cuda()}
    for max_norm in (0.0, -1.0):
        norm, coef = clip_grad_norm_(g, max_norm)
        assert coef == 1.0 and abs(norm - math.sqrt(1200.0)) <= NORM_REL * norm


# ---- the single-tensor entry points of the header, through the bound library
def _ws():
    lib = L.load()
    return torch.empty(lib.a3d_sum_squares_workspace_bytes(), dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 512 * 2048, 512 * 2048 + 1, 3 * 512 * 2048 + 7])
def test_sum_squares_single_tensor(n):
    """(f) a3d_sum_squares / a3d_sum_squares_accumulate at the 2048-element block edge and past the 512-block cap, where
    the grid-stride loop takes over; _accumulate adds to what *acc_dev holds."""
    lib = L.load()
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3.0
    want = sum_squares64(g.numpy())
    gd, ws = g.cuda(), _ws()
    out = C.c_double(-1.0)
    L.check(lib.a3d_sum_squares(L.ptr(gd), n, C.byref(out), L.ptr(ws), ws.numel(), L.stream(gd.device)), "a3d_sum_squares")
    assert abs(out.value - want) <= NORM_REL * want, (out.value, want)
    prior = 1234.5
    acc = torch.full((1,), prior, dtype=torch.float64, device="cuda")
    for rep in (1, 2):
        L.check(lib.a3d_sum_squares_accumulate(L.ptr(gd), n, L.ptr(acc), L.ptr(ws), ws.numel(), L.stream(gd.device)),
                "a3d_sum_squares_accumulate")
        got = float(acc.item())
        assert abs(got - (prior + rep * want)) <= NORM_REL * (prior + rep * want), (rep, got, want)


@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097])
def test_adamw_single_tensor_meets_bounds_and_equals_multi(n, step):
    """(f) a3d_adamw_step inside the bounds, and a3d_adamw_step_multi on copies of the same inputs bit-equal to it (the
    header's promise)."""
    lib = L.load()
    gen = torch.Generator().manual_seed(1000 * step + n)
    p, g, m = (torch.randn(n + 2 * GUARD, generator=gen) for _ in range(3))
    v = torch.rand(n + 2 * GUARD, generator=gen) * 0.01
    scale = 0.81
    one = [x.cuda() for x in (p, g, m, v)]
    many = [x.cuda() for x in (p, g, m, v)]
    inner = slice(GUARD, GUARD + n)
    args = (HP["lr"], HP["betas"][0], HP["betas"][1], HP["eps"], HP["weight_decay"], scale)
    L.check(lib.a3d_adamw_step(L.ptr(one[0][inner]), L.ptr(one[1][inner]), L.ptr(one[2][inner]), L.ptr(one[3][inner]), n, step,
                               *args, L.stream(one[0].device)), "a3d_adamw_step")
    tab, nchunks = _mt_layout([n])
    for q, x in zip("pgmv", many):
        tab[q] = x[inner].data_ptr()
    tab["bias1"] = 1.0 - HP["betas"][0] ** step
    tab["bias2_sqrt"] = math.sqrt(1.0 - HP["betas"][1] ** step)
    tabd = _to_device(tab, many[0].device)
    L.check(lib.a3d_adamw_step_multi(L.ptr(tabd), 1, nchunks, *args, L.stream(many[0].device)), "a3d_adamw_step_multi")
    torch.cuda.synchronize()
    _check_step(tuple(x[inner].numpy() for x in (p, m, v)), g[inner].numpy(), tuple(_np(one[i][inner]) for i in (0, 2, 3)),
                step, HP, scale, "a3d_adamw_step")
    for q, a, b, orig in zip("pgmv", one, many, (p, g, m, v)):
        assert torch.equal(_bits(a), _bits(b)), f"single- and multi-tensor {q} differ"
        outside = torch.ones(n + 2 * GUARD, dtype=torch.bool)
        outside[inner] = q == "g"
        assert torch.equal(_bits(a.cpu())[outside], _bits(orig)[outside]), f"{q} written outside the tensor"


def test_refusals_before_any_launch():
    """(g) argument checks: A3D_ERR_INVALID (-1), a3d_last_error names the function, nothing is launched."""
    lib = L.load()
    x = torch.ones(512, device="cuda")
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.a3d_sum_squares_workspace_bytes() + 8, dtype=torch.uint8, device="cuda")
    need = lib.a3d_sum_squares_workspace_bytes()
    assert ws.data_ptr() % 8 == 0
    out = C.c_double(-3.0)
    st = L.stream(x.device)
    px, pw, pa, null = L.ptr(x), L.ptr(ws), L.ptr(acc), C.c_void_p(0)
    pw4 = C.c_void_p(ws.data_ptr() + 4)
    hp = (1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0)
    tab, nchunks = _mt_layout([512])
    for q in "pgmv":
        tab[q] = x.data_ptr()
    tabd = _to_device(tab, x.device)
    pt = L.ptr(tabd)
    mws = torch.empty(lib.a3d_mt_workspace_bytes(1) + 8, dtype=torch.uint8, device="cuda")
    mneed = lib.a3d_mt_workspace_bytes(1)
    pm, pm4 = L.ptr(mws), C.c_void_p(mws.data_ptr() + 4)
    cases = []
    for fn, name, dst in ((lib.a3d_sum_squares, "a3d_sum_squares", C.byref(out)),
                          (lib.a3d_sum_squares_accumulate, "a3d_sum_squares_accumulate", pa)):
        cases += [(name, "n = 0", lambda fn=fn, dst=dst: fn(px, 0, dst, pw, need, st)),
                  (name, "null gradient", lambda fn=fn, dst=dst: fn(null, 512, dst, pw, need, st)),
                  (name, "null result", lambda fn=fn: fn(px, 512, None, pw, need, st)),
                  (name, "null workspace", lambda fn=fn, dst=dst: fn(px, 512, dst, null, need, st)),
                  (name, "workspace one byte short", lambda fn=fn, dst=dst: fn(px, 512, dst, pw, need - 1, st)),
                  (name, "workspace misaligned by 4", lambda fn=fn, dst=dst: fn(px, 512, dst, pw4, need, st))]
    step1 = lib.a3d_adamw_step
    cases += [("a3d_adamw_step", "n = 0", lambda: step1(px, px, px, px, 0, 1, *hp, st)),
              ("a3d_adamw_step", "step = 0", lambda: step1(px, px, px, px, 512, 0, *hp, st))]
    for i in range(4):
        ptrs = [px] * 4
        ptrs[i] = null
        cases.append(("a3d_adamw_step", f"null pointer {i}", lambda ptrs=ptrs: step1(*ptrs, 512, 1, *hp, st)))
    ssm, asm_ = lib.a3d_sum_squares_multi, lib.a3d_adamw_step_multi
    cases += [("a3d_sum_squares_multi", "null table", lambda: ssm(null, 1, 1, pa, pm, mneed, st)),
              ("a3d_sum_squares_multi", "n_tensors = 0", lambda: ssm(pt, 0, 1, pa, pm, mneed, st)),
              ("a3d_sum_squares_multi", "n_chunks = 0", lambda: ssm(pt, 1, 0, pa, pm, mneed, st)),
              ("a3d_sum_squares_multi", "n_chunks = 2^31", lambda: ssm(pt, 1, 2 ** 31, pa, pm, mneed, st)),
              ("a3d_sum_squares_multi", "null result", lambda: ssm(pt, 1, 1, null, pm, mneed, st)),
              ("a3d_sum_squares_multi", "null workspace", lambda: ssm(pt, 1, 1, pa, null, mneed, st)),
              ("a3d_sum_squares_multi", "workspace one byte short", lambda: ssm(pt, 1, 1, pa, pm, mneed - 1, st)),
              ("a3d_sum_squares_multi", "workspace misaligned by 4", lambda: ssm(pt, 1, 1, pa, pm4, mneed, st)),
              ("a3d_adamw_step_multi", "null table", lambda: asm_(null, 1, 1, *hp, st)),
              ("a3d_adamw_step_multi", "n_tensors = 0", lambda: asm_(pt, 0, 1, *hp, st)),
              ("a3d_adamw_step_multi", "n_chunks = 0", lambda: asm_(pt, 1, 0, *hp, st)),
              ("a3d_adamw_step_multi", "n_chunks = 2^31", lambda: asm_(pt, 1, 2 ** 31, *hp, st))]
    for name, what, call in cases:
        assert call() == -1, (name, what)                          # A3D_ERR_INVALID
        msg = lib.a3d_last_error().decode()
        assert msg.startswith(name + ":"), (name, what, msg)
    torch.cuda.synchronize()
    assert torch.equal(x, torch.ones_like(x)) and float(acc.item()) == 0.0 and out.value == -3.0
