"""tests/optimizer_reference.py against torch's own optimizer and clipping in float64, and the fairness of every input family of
tests/optimizer_inputs.py -- what tests/test_hip_optimizer_range.py asks of the kernels must be satisfiable: the float32
restatement is finite, d32 > 0 wherever a bound is a multiple of d32 alone, and the kernels' expressions evaluated in float32 on
the CPU (once with every operation rounded, once with the fused multiply-adds a compiler may form) sit inside the bounds.  No GPU."""
import math

import numpy as np
import pytest
import torch

import optimizer_inputs as I
import optimizer_reference as R

NO_GRAD = True


@pytest.mark.parametrize("betas", I.BETAS)
@pytest.mark.parametrize("wd", [0.0, 4.5e-2])
def test_float64_adamw_is_torch_optim_adamw(betas, wd):
    n, lr = 1000, R.f32(3e-3)
    b1, b2, eps, wd = R.f32(betas[0]), R.f32(betas[1]), R.f32(I.EPS), R.f32(wd)
    with torch.enable_grad():
        ref = I.unit((n,), "host.p").double().requires_grad_(True)
        opt = torch.optim.AdamW([ref], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
        p, m, v = ref.detach().clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        for step in range(1, 6):
            g = (I.unit((n,), "host.g%d" % step) * 10.0 ** (step - 3)).double()
            ref.grad = g.clone()
            opt.step()
            R.adamw_step(p, g, m, v, lr, b1, b2, eps, wd, *R.bias_corrections(betas[0], betas[1], step))
            st = opt.state[ref]
            for got, want in ((p, ref.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
                assert float((got - want).abs().max()) <= 1e-14 * float(want.abs().max()), step


@pytest.mark.parametrize("max_norm", [0.5, 1e9, 1e-3])
def test_float64_norm_and_coefficient_are_clip_grad_norm(max_norm):
    ts = [t.double() for t in I.norm_table_case(65, False).ts]
    want = I.norm_table_case(65, False).n64
    gs = [t.clone() for t in ts]
    for t, g in zip(ts, gs):
        t.grad = g
    total = float(torch.nn.utils.clip_grad_norm_(ts, max_norm, foreach=False))
    assert abs(total - want) <= 1e-14 * want
    coef = R.clip_coef(want, max_norm)
    for t in ts[:8]:
        assert float((t.grad - t * coef).abs().max()) <= 1e-14 * float(t.abs().max())
    assert R.clip_coef(want, 0.0) == 1.0 and R.clip_coef(want, -1.0) == 1.0


def kernel_f32(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2s, gs, contract=False):
    """aw_update of csrc/pack.hip in float32 tensor ops.  contract=False: every operation rounded; contract=True: with the fused
    multiply-adds a compiler may form (a b + c rounded once: the double product of two float32 values is exact)"""
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    fma = (lambda a, b, c: (a.double() * b.double() + c.double()).float()) if contract else (lambda a, b, c: a * b + c)
    gi = g * f(gs)
    mi = fma(f(b1), m, (1 - f(b1)) * gi)
    vi = fma((1 - f(b2)) * gi, gi, f(b2) * v)
    upd = (f(lr) / f(bc1)) * mi / (vi.sqrt() / f(bc2s) + f(eps))
    pi = fma(p, fma(-f(lr), f(wd), f(1.0)), -upd)
    return pi, mi, vi


def inside(errs, what):
    worst = 0.0
    for i, (err, d32, ulp) in enumerate(errs):
        assert err <= 4 * d32 + ulp, "%s tensor %d: err %.3e, d32 %.3e, ulp %.3e" % (what, i, err, d32, ulp)
        worst = max(worst, err / d32 if d32 > 0 else 0.0)
    return worst


@pytest.mark.parametrize("contract", [False, True])
@pytest.mark.parametrize("idx", range(len(I.A_CASES)), ids=I.A_IDS)
def test_adam_scale_family_is_fair(idx, contract):
    d = I.adam_case(idx)
    c = d["c"]
    b1, b2, lr, wd, eps = R.f32(c.betas[0]), R.f32(c.betas[1]), R.f32(c.lr), R.f32(c.wd), R.f32(I.EPS)
    assert float((d["g"][:, :I.A_SIZES[0]].abs().double() * R.f32(c.gs)).max()) <= I.DECADES[0] * 1.001
    st = [d["p0"].clone(), d["m0"].clone(), d["v0"].clone()]
    worst = 0.0
    for s in range(1, I.A_STEPS[-1] + 1):
        h = d["hyper"][s - 1]
        st = list(kernel_f32(st[0], d["g"][s - 1], st[1], st[2], lr, b1, b2, eps, wd, h[1], h[2], h[3], contract))
        if s not in I.A_STEPS:
            continue
        for form in ("hyper", "step"):
            y = d["snap"][form][s]
            for k, name in enumerate("pmv"):
                assert bool(torch.isfinite(y[3 + k]).all()), (form, s, name)
                errs = I.per_tensor(y[3 + k], y[k], y[3 + k], I.A_SIZES)
                for j, (_, d32, _) in enumerate(errs):          # (the g = 0 tensor from the zero state: m = v = 0 exactly, d32 = 0)
                    assert d32 > 0 or j == I.A_ZERO, (form, s, name, j)
        y = d["snap"]["hyper"][s]
        for k, name in enumerate("pmv"):
            worst = max(worst, inside(I.per_tensor(st[k], y[k], y[3 + k], I.A_SIZES), "step %d %s" % (s, name)))
        o = sum(I.A_SIZES[:I.A_ZERO])
        n = I.A_SIZES[I.A_ZERO]
        assert bool((y[1][o:o + n] == 0).all()) and bool((y[2][o:o + n] == 0).all())       # g = 0 from the zero state: m = v = 0
    print("%s: float32 emulation of the kernel's expression (contract=%s), worst err / d32 = %.2f" % (I.A_IDS[idx], contract, worst))


@pytest.mark.parametrize("betas", I.BETAS)
@pytest.mark.parametrize("step", I.B_STEPS)
def test_bias_correction_family_is_fair(betas, step):
    d = I.bias_case(betas, step)
    y = d["y"]
    for k in range(3):
        assert bool(torch.isfinite(y[3 + k]).all()) and float((y[3 + k].double() - y[k]).abs().max()) > 0
    bc1, bc2s = R.bias_corrections(betas[0], betas[1], step)
    got = kernel_f32(torch.zeros(I.B_N), d["g"], d["m0"], d["v0"], R.f32(I.B_LR), R.f32(betas[0]), R.f32(betas[1]), R.f32(I.EPS),
                     R.f32(I.B_WD), R.f32(bc1), R.f32(bc2s), 1.0)
    for k in range(3):
        inside(I.per_tensor(got[k], y[k], y[3 + k], [I.B_N]), "pmv"[k])
    # what the test is there to catch: the corrections formed through float32 powf are NOT inside the bound at beta2 = 0.999, step 2
    if step == 2 and betas[1] == 0.999:
        bad1 = float(np.float32(1) - np.power(np.float32(betas[0]), np.float32(step)))
        bad2 = float(np.sqrt(np.float32(1) - np.power(np.float32(betas[1]), np.float32(step))))
        gotb = kernel_f32(torch.zeros(I.B_N), d["g"], d["m0"], d["v0"], R.f32(I.B_LR), R.f32(betas[0]), R.f32(betas[1]), R.f32(I.EPS),
                          R.f32(I.B_WD), bad1, bad2, 1.0)
        err, d32, ulp = I.per_tensor(gotb[0], y[0], y[3], [I.B_N])[0]
        print("float32 powf corrections at step 2, betas %s: err %.3e, d32 %.3e (ratio %.1f)" % (betas, err, d32, err / d32))
        assert err > 4 * d32 + ulp


@pytest.mark.parametrize("count,ones", [(c, False) for c in I.C_ADAM_COUNTS] + [(70, True)])
def test_adam_table_family_is_fair(count, ones):
    d = I.table_adam_case(count, ones)
    y, h = d["y"], d["hyper"]
    got = kernel_f32(d["p0"], d["g"], d["m0"], d["v0"], R.f32(I.C_LR), R.f32(I.C_BETAS[0]), R.f32(I.C_BETAS[1]), R.f32(I.EPS),
                     R.f32(I.C_WD), h[1], h[2], h[3])
    for k in range(3):
        assert bool(torch.isfinite(y[3 + k]).all())
        inside(I.per_tensor(got[k], y[k], y[3 + k], d["sizes"]), "pmv"[k])
    if not ones:                # every size meets every misaligned array (and none)
        seen = {(n, I.misaligned_role(i, 4)) for i, n in enumerate(d["sizes"])}
        assert len(seen) == len(I.SIZES) * 5


def test_arena_layout_guards_and_alignment():
    sizes = I.table_sizes(65)
    shifted = [i % 3 == 1 for i in range(65)]
    flat = I.unit((sum(sizes),), "host.arena")
    a, offs = I.arena(flat, sizes, shifted)
    assert torch.equal(I.gather(a, sizes, offs), flat) and I.guards_intact(a, sizes, offs)
    prev_end = 0
    for n, o, sh in zip(sizes, offs, shifted):
        assert o % 4 == (1 if sh else 0) and o - prev_end >= 4
        prev_end = o + n
    assert a.numel() - prev_end >= 4
    a[offs[7] - 1] = 0.0
    assert not I.guards_intact(a, sizes, offs)


@pytest.mark.parametrize("name", I.NORM_SCALES)
def test_norm_scale_family_is_fair(name):
    c = I.norm_case(name)
    flat = torch.cat(c.ts)
    nz = flat[flat != 0].abs()
    assert float(nz.min()) >= I.NORM_LO and float(nz.max()) < I.NORM_HI              # inside the documented domain
    assert math.isfinite(c.n32) and c.n32 > 0
    assert abs(c.n32 - c.n64) <= I.norm_bound(c)
    for mn in I.max_norms(c.n64):
        want, bound = I.coef_bound(c, mn)
        c32 = 1.0 if mn <= 0 else float(torch.clamp(torch.tensor(mn, dtype=torch.float32) / (torch.tensor(c.n32) + 1e-6), max=1.0))
        assert abs(c32 - want) <= bound, (mn, c32, want, bound)
    # the kernel's own order (16 float32 squares, then double) is inside the bound too
    sq = [float((t * t).double().sum()) for t in c.ts]          # float32 squares, double sums: an upper class of the kernel's
    assert abs(R.f32(math.sqrt(sum(sq))) - c.n64) <= I.norm_bound(c)


def test_norm_outside_the_domain_is_what_the_header_says():
    hi = torch.full((5,), 2.0 ** 64)                           # g^2 = 2^128: +inf in float32
    assert math.isinf(float((hi * hi).sum()))
    lo = torch.full((4096,), 2.0 ** -76)                       # g^2 = 2^-152: 0 in float32 -- understated, the true norm is 2^-70
    assert float((lo * lo).sum()) == 0.0 and R.grad_norm([lo]) == 2.0 ** -70
    near = (I.unit((4096,), "norm.out.lo") * 2.0 ** -64).float()        # [2^-65, 2^-64): denormal squares, 2^-150 off at most each
    n64 = R.grad_norm([near])
    got = R.f32(math.sqrt(float((near * near).double().sum())))
    assert 0.0 < got <= n64 * (1 + 2.0 ** -20)


@pytest.mark.parametrize("decay", [0.99, 0.9999])
def test_ema_drift_family_is_fair(decay):
    d = I.ema_drift_case(decay)
    assert bool(torch.isfinite(d["y"][1]).all())
    for _, d32, _ in I.per_tensor(d["y"][1], d["y"][0], d["y"][1], I.G_SIZES):
        assert d32 > 0
    assert d["w"] != 1.0 - d["decay"]                           # the entry's (1 - decay) is the host's float32, not 1.f - decay


@pytest.mark.parametrize("contract", [False, True])
def test_chain_family_is_fair(contract):
    d = I.chain_case()
    sizes = d["sizes"]
    clipped = sum(c < 1.0 for c in d["coefs"])
    assert 8 <= clipped <= 12, clipped
    assert set(sizes) == set(I.H_SIZES) and len(sizes) == I.H_COUNT
    for k in range(3):
        assert bool(torch.isfinite(d["y"][3 + k]).all())
        for _, d32, _ in I.per_tensor(d["y"][3 + k], d["y"][k], d["y"][3 + k], sizes):
            assert d32 > 0
    # the chain in float32 as the kernels run it: 16 float32 squares then double, the coefficient's float32 division, aw_update
    st = [d["p0"].clone(), torch.zeros(sum(sizes)), torch.zeros(sum(sizes))]
    for s in range(I.H_ITERS):
        h = d["hyper"][s]
        total = torch.tensor(math.sqrt(float((d["g"][s] * d["g"][s]).double().sum())), dtype=torch.float32)
        c = float(torch.clamp(torch.tensor(I.H_MAX_NORM) / (total + torch.tensor(1e-6)), max=1.0))
        st = list(kernel_f32(st[0], d["g"][s], st[1], st[2], R.f32(I.H_LR), R.f32(I.H_BETAS[0]), R.f32(I.H_BETAS[1]), R.f32(I.EPS),
                             R.f32(I.H_WD), h[1], h[2], c, contract))
    worst = max(inside(I.per_tensor(st[k], d["y"][k], d["y"][3 + k], sizes), "pmv"[k]) for k in range(3))
    print("chain, float32 emulation (contract=%s): worst err / d32 %.2f" % (contract, worst))


def test_amax_reference_rules():
    x = torch.tensor([0.5, float("nan"), -3.0, 2.0])
    assert R.amax(x) == 3.0 and R.amax(x, 7.0) == 7.0
    assert R.amax(torch.tensor([float("nan")])) == 0.0
    assert R.amax(torch.tensor([1.0, float("-inf")])) == math.inf
    assert R.amax(torch.tensor([-0.0])) == 0.0 and math.copysign(1.0, R.amax(torch.tensor([-0.0]))) == 1.0
    for n in I.AMAX_SIZES + [I.AMAX_BIG]:
        pos = I.amax_positions(n)
        assert pos[0] == 0 and pos[-1] == n - 1 and all(0 <= q < n for q in pos)
    assert I.amax_positions(4097) == [0, 4095, 4096] and I.amax_positions(7) == [0, 3, 4, 6] and I.amax_positions(3) == [0, 2]
