"""The last stage of a training iteration -- global gradient norm, clip coefficient, AdamW, EMA, and the max |x| that chooses every
loss scale (ds_grad_norm_multi, ds_adamw / ds_adamw_dev / ds_adamw_multi, ds_ema_multi, ds_amax: csrc/pack.hip, csrc/train.hip) --
against the FLOAT64 yardstick of tests/optimizer_reference.py on the input families of tests/optimizer_inputs.py (whose fairness
tests/test_optimizer_host.py asserts without a GPU).

The bound, PER TENSOR (each tensor carries one gradient magnitude, so a maximum cannot hide small entries behind large ones):
    max |kernel - f64| <= 4 d32 + one float32 ulp of the tensor's largest |f64 value|,   d32 = max |torch's float32 expression - f64|
(the factor 4 is DESIGN.md section 4's).  The norm likewise (4 d32 + 1 ulp, d32 from torch's float32 _foreach_norm path), the
coefficient to the norm's own relative bound (4 d32 + ulp) / norm; ds_amax and every "untouched" claim are exact.  No
bound comes from a kernel's output.
  a. AdamW across |g grad_scale| = 1e-12 .. 1e6 (around and far from eps), p in {0, 1e-3, 1}, grad_scale in {1, 0.37, 2^-12}, lr in
     {3e-3, 3e-6}, wd in {0, 4.5e-2}, both beta pairs, g = 0 from the zero state and on a non-zero one: p, m, v of all three entry
     points after steps 1, 2, 50, 400, `hyper` refreshed per step;
  b. ds_adamw's own bias corrections at steps 1 .. 10^6;
  c. the three multi-tensor kernels over sizes around 4, 1024 and 4096 elements, tensor counts around their descriptor batches, a
     table of 1-element tensors, each array misaligned by 4 bytes in turn; the guard elements between tensors keep their bits;
  d. the norm over |g| = 2^-40 .. 2^40, at both ends of its documented domain (2^-63 <= |g| < 2^62) and just outside;
  e. +inf and NaN gradients: total and coef are what include/diffsound_hip.h says;
  f. ds_amax: sizes 1 .. 2^21 + 7, both alignments, the maximum at every seam, negative / denormal / -0 / NaN / inf, a start value;
  g. 300 EMA updates at decay 0.99 and 0.9999;
  h. 20 iterations of norm -> coefficient -> AdamW on 150 tensors, half of them clipping.

Measured on an MI355X, worst err / d32 over a family's tensors (the table of DESIGN.md section 7.2):
  a. ds_adamw 2.00 .. 2.40, ds_adamw_dev 1.35 .. 2.04, ds_adamw_multi 1.94 .. 2.30 over the 12 cases;
  b. 1.08 .. 1.33 over the steps and both beta pairs;
  c. ds_adamw_multi 3.35 .. 4.22 (7.32 on the table of 1-element tensors: d32 is a fraction of an ulp there and the ulp term carries
     the bound), ds_ema_multi 1.00, ds_grad_norm_multi 0.15 .. 1.00;
  d. 0.14 .. 1.00;   g. 1.00 (the kernel is torch's expression to the bit);   h. 2.26, 10 of 20 iterations clipping.
The chain of (h) takes the size list from 1023 elements up: tests/optimizer_inputs.py H_SIZES says why.
The bound found ds_adamw forming 1 - beta^step through float32 powf (beta2 = 0.999, step 2: 1.5e-5 relative on 1 - beta2^2, p at
more than 20 d32); it now forms the corrections in double.  The NaN clip coefficient was 1 and is NaN now (include/diffsound_hip.h).
GPU only (-m gpu)."""
import ctypes
import math

import pytest
import torch

import optimizer_inputs as I
import optimizer_reference as R
from conftest import parity_line
from text_to_sound_synthesis_amd import _lib

pytestmark = pytest.mark.gpu
NO_GRAD = True


def lib():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _lib.lib()


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_error():
    """a kernel fault surfaces at the next synchronisation: the session ends there instead of launching the remaining tests on a
    device in that state"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:          # noqa: BLE001
        pytest.exit("the GPU reported an error (%s): no further test is run on it" % e, returncode=3)


def records(cols, sizes):
    """HOST table of descriptors: per tensor the device addresses of `cols` (lists of int addresses) and its element count"""
    k = len(cols) + 1
    rec = (ctypes.c_int64 * (k * len(sizes)))()
    for i, n in enumerate(sizes):
        rec[k * i:k * i + k] = [c[i] for c in cols] + [n]
    return ctypes.cast(rec, ctypes.c_void_p), rec


def addrs(t, sizes, offs=None):
    """device addresses of the tensors of a flat device array (offs: element offsets; default: packed back to back).  The caller
    keeps `t` alive until the kernel has run: addresses hold no reference."""
    if offs is None:
        offs = [sum(sizes[:i]) for i in range(len(sizes))]
    return [t.data_ptr() + 4 * o for o in offs]


def adamw_multi(p, g, m, v, sizes, hyper, betas, wd):
    tab, keep = records([p, g, m, v], sizes)
    _lib.check(lib().ds_adamw_multi(tab, len(sizes), _lib.ptr(hyper), betas[0], betas[1], I.EPS, wd, _lib.stream()))


def grad_norm_multi(g, sizes, max_norm, coef_ptr="own"):
    """-> (total, coef) device tensors of one element (coef_ptr: "own", None, or a device address)"""
    tab, keep = records([g], sizes)
    chunks = sum((n + 4095) // 4096 for n in sizes)
    part = torch.full((chunks,), float("nan"), dtype=torch.float64, device="cuda")
    total, coef = torch.full((1,), -7.0, device="cuda"), torch.full((1,), -7.0, device="cuda")
    cp = _lib.ptr(coef) if coef_ptr == "own" else coef_ptr
    _lib.check(lib().ds_grad_norm_multi(tab, len(sizes), _lib.ptr(part), chunks, max_norm, _lib.ptr(total), cp, _lib.stream()))
    return total, coef


def check(got, y64, y32, sizes, what):
    """the per-tensor bound; -> (err / d32, err, d32) of the tensor with the worst ratio"""
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % what
    worst = (0.0, 0.0, 0.0)
    for i, (err, d32, ulp) in enumerate(I.per_tensor(got, y64, y32, sizes)):
        assert err <= 4 * d32 + ulp, "%s, tensor %d (%d elements): err %.3e, d32 %.3e, ulp %.3e" % (what, i, sizes[i], err, d32, ulp)
        if d32 > 0:
            worst = max(worst, (err / d32, err, d32))
    return worst


def fmt(w):
    return "err %.3e, d32 %.3e, ratio %.2f" % (w[1], w[2], w[0])


# ---- a ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(I.A_CASES)), ids=I.A_IDS)
def test_adamw_across_gradient_scale(idx):
    d = I.adam_case(idx)
    c = d["c"]
    sizes, N = I.A_SIZES, I.A_N
    g, gpre = d["g"].cuda(), d["gpre"].cuda()
    hyper_all = torch.tensor(d["hyper"], dtype=torch.float32).cuda()
    hyper = torch.zeros(4, device="cuda")
    state = {e: [d[k].cuda() for k in ("p0", "m0", "v0")] for e in ("adamw", "dev", "multi")}
    offs = [sum(sizes[:i]) for i in range(len(sizes))]
    L = lib()
    b1, b2, wd, lr = c.betas[0], c.betas[1], c.wd, c.lr
    worst = {e: (0.0, 0.0, 0.0) for e in state}
    for s in range(1, I.A_STEPS[-1] + 1):
        hyper.copy_(hyper_all[s - 1])                                   # refreshed per step, as GraphedIteration does
        gp, gpp = g[s - 1], gpre[s - 1]
        p, m, v = state["multi"]
        adamw_multi(addrs(p, sizes), addrs(gp, sizes), addrs(m, sizes), addrs(v, sizes), sizes, hyper, c.betas, wd)
        for o, n in zip(offs, sizes):
            p, m, v = state["dev"]
            _lib.check(L.ds_adamw_dev(_lib.ptr_off(p, o), _lib.ptr_off(gp, o), _lib.ptr_off(m, o), _lib.ptr_off(v, o), n, _lib.ptr(hyper),
                                      b1, b2, I.EPS, wd, _lib.stream()))
            p, m, v = state["adamw"]
            _lib.check(L.ds_adamw(_lib.ptr_off(p, o), _lib.ptr_off(gpp, o), _lib.ptr_off(m, o), _lib.ptr_off(v, o), n, lr, b1, b2, I.EPS,
                                  wd, s, _lib.stream()))
        if s not in I.A_STEPS:
            continue
        for e in state:
            y = d["snap"]["step" if e == "adamw" else "hyper"][s]
            for k, name in enumerate("pmv"):
                got = state[e][k].cpu()
                worst[e] = max(worst[e], check(got, y[k], y[3 + k], sizes, "%s step %d %s" % (e, s, name)))
                if name in "mv":                                        # g = 0 from the zero state: m = v = 0, p only decays
                    z = got[offs[I.A_ZERO]:offs[I.A_ZERO] + sizes[I.A_ZERO]]
                    assert bool((z == 0).all()), "%s step %d: %s of the g = 0 tensor is not 0" % (e, s, name)
    line = "adamw across scale, %s: worst tensor %s" % (I.A_IDS[idx], "; ".join("%s %s" % (e, fmt(worst[e])) for e in worst))
    print(line)
    parity_line(line)


# ---- b ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", I.BETAS, ids=["b2-0.96", "b2-0.999"])
def test_adamw_own_bias_corrections(betas):
    worst = {}
    for step in I.B_STEPS:
        d = I.bias_case(betas, step)
        p, g, m, v = torch.zeros(I.B_N, device="cuda"), d["g"].cuda(), d["m0"].cuda(), d["v0"].cuda()
        _lib.check(lib().ds_adamw(_lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), I.B_N, I.B_LR, betas[0], betas[1], I.EPS, I.B_WD, step,
                                  _lib.stream()))
        y = d["y"]
        worst[step] = max(check(t.cpu(), y[k], y[3 + k], [I.B_N], "step %d %s" % (step, "pmv"[k])) for k, t in enumerate((p, m, v)))
    line = "ds_adamw bias corrections, betas %s: per step %s" % (betas, "; ".join("%d: %s" % (k, fmt(w)) for k, w in worst.items()))
    print(line)
    parity_line(line)


# ---- c ------------------------------------------------------------------------------------------------------------------------
def arenas(flats, sizes, roles):
    """one guarded arena per array of `flats`; array r + 1 of tensor i is shifted by 4 bytes where misaligned_role(i) == r + 1"""
    out = []
    for r, flat in enumerate(flats):
        a, offs = I.arena(flat, sizes, [I.misaligned_role(i, roles) == r + 1 for i in range(len(sizes))])
        out.append((a.cuda(), offs))
    return out


@pytest.mark.parametrize("count,ones", [(c, False) for c in I.C_ADAM_COUNTS] + [(70, True)])
def test_adamw_multi_paths_and_neighbours(count, ones):
    d = I.table_adam_case(count, ones)
    sizes, y = d["sizes"], d["y"]
    ar = arenas([d["p0"], d["g"], d["m0"], d["v0"]], sizes, 4)
    hyper = torch.tensor(d["hyper"], dtype=torch.float32).cuda()
    adamw_multi(*[addrs(a, sizes, offs) for a, offs in ar], sizes, hyper, I.C_BETAS, I.C_WD)
    worst = (0.0, 0.0, 0.0)
    for k, name in ((0, "p"), (2, "m"), (3, "v")):
        a, offs = ar[k][0].cpu(), ar[k][1]
        j = {0: 0, 2: 1, 3: 2}[k]
        worst = max(worst, check(I.gather(a, sizes, offs), y[j], y[3 + j], sizes, name))
        assert I.guards_intact(a, sizes, offs), "elements next to a tensor of %s were written" % name
    a, offs = ar[1][0].cpu(), ar[1][1]
    assert I.guards_intact(a, sizes, offs) and torch.equal(I.gather(a, sizes, offs), d["g"])
    line = "adamw_multi table of %d%s: worst tensor %s" % (count, " 1-element tensors" if ones else "", fmt(worst))
    print(line)
    parity_line(line)


@pytest.mark.parametrize("count,ones", [(c, False) for c in I.C_EMA_COUNTS] + [(100, True)])
def test_ema_multi_paths_and_neighbours(count, ones):
    d = I.table_ema_case(count, ones)
    sizes, y = d["sizes"], d["y"]
    ar = arenas([d["e0"], d["cur"]], sizes, 2)
    tab, keep = records([addrs(a, sizes, offs) for a, offs in ar], sizes)
    _lib.check(lib().ds_ema_multi(tab, len(sizes), d["decay"], d["w"], _lib.stream()))
    a, offs = ar[0][0].cpu(), ar[0][1]
    worst = check(I.gather(a, sizes, offs), y[0], y[1], sizes, "ema")
    assert I.guards_intact(a, sizes, offs), "elements next to an average were written"
    a, offs = ar[1][0].cpu(), ar[1][1]
    assert I.guards_intact(a, sizes, offs) and torch.equal(I.gather(a, sizes, offs), d["cur"])
    line = "ema_multi table of %d%s: worst tensor %s" % (count, " 1-element tensors" if ones else "", fmt(worst))
    print(line)
    parity_line(line)


def norm_checks(c, ts_addr, sizes, what):
    """total and coef of a case under their bounds for the four thresholds; two calls agree bit for bit.  -> (err / d32, err, d32)"""
    ratio = (0.0, 0.0, 0.0)
    for mn in I.max_norms(c.n64):
        total, coef = grad_norm_multi(ts_addr, sizes, mn)
        t, k = float(total), float(coef)
        err, d32 = abs(t - c.n64), abs(c.n32 - c.n64)
        print("%s, max_norm %.6g: total %.9g (f64 %.12g): err %.3e, d32 %.3e; coef %.9g" % (what, mn, t, c.n64, err, d32, k))
        assert err <= I.norm_bound(c), "%s: total %.9g, f64 %.12g: err %.3e, bound %.3e" % (what, t, c.n64, err, I.norm_bound(c))
        want, bound = I.coef_bound(c, mn)
        assert abs(k - want) <= bound and k <= 1.0, "%s, max_norm %g: coef %.9g, f64 %.12g, bound %.3e" % (what, mn, k, want, bound)
        ratio = max(ratio, (err / d32 if d32 > 0 else 0.0, err, d32))
    total2, coef2 = grad_norm_multi(ts_addr, sizes, mn, coef_ptr=None)
    assert float(total2) == t and float(coef2) == -7.0                      # fixed-order sums: bit-reproducible; coef is optional
    return ratio


@pytest.mark.parametrize("count,ones", [(c, False) for c in I.C_NORM_COUNTS] + [(130, True)])
def test_grad_norm_multi_paths(count, ones):
    c = I.norm_table_case(count, ones)
    sizes = [t.numel() for t in c.ts]
    (a, offs), = arenas([torch.cat(c.ts)], sizes, 1)
    ratio = norm_checks(c, addrs(a, sizes, offs), sizes, "table of %d" % count)
    assert I.guards_intact(a.cpu(), sizes, offs)
    line = "grad_norm_multi table of %d%s: %s" % (count, " 1-element tensors" if ones else "", fmt(ratio))
    print(line)
    parity_line(line)


# ---- d, e ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", I.NORM_SCALES)
def test_grad_norm_across_scale(name):
    c = I.norm_case(name)
    sizes = [t.numel() for t in c.ts]
    flat = torch.cat(c.ts).cuda()
    ratio = norm_checks(c, addrs(flat, sizes), sizes, name)
    line = "grad norm, |g| %s: %s" % (name, fmt(ratio))
    print(line)
    parity_line(line)


def test_grad_norm_outside_its_domain():
    """What include/diffsound_hip.h promises outside 2^-63 <= |g| < 2^62: above, total is +inf (or right) -- never finite and wrong;
    below, the squares are denormal: total stays finite, never more than 2^-20 relative above the norm, and goes down to 0."""
    hi = (I.unit((4096,), "norm.out.hi") * 2.0 ** 63).float()                      # [2^62, 2^63): a thread's 16 squares overflow
    dev = hi.cuda()
    total, coef = grad_norm_multi(addrs(dev, [4096]), [4096], 0.5)
    n64 = R.grad_norm([hi])
    print("|g| in [2^62, 2^63): total %r (f64 %.6g), coef %r" % (float(total), n64, float(coef)))
    assert math.isinf(float(total)) or abs(float(total) - n64) <= 2.0 ** -22 * n64
    assert float(coef) == 0.0 or not math.isinf(float(total))
    top = torch.full((5,), 2.0 ** 64)                                              # every square overflows
    dev = top.cuda()
    total, coef = grad_norm_multi(addrs(dev, [5]), [5], 0.5)
    assert float(total) == math.inf and float(coef) == 0.0
    near = (I.unit((4096,), "norm.out.lo") * 2.0 ** -64).float()                   # [2^-65, 2^-64): every square is denormal
    dev = near.cuda()
    total, coef = grad_norm_multi(addrs(dev, [4096]), [4096], 0.5)
    n64 = R.grad_norm([near])
    print("|g| in [2^-65, 2^-64): total %r (f64 %r): %+.3e relative, coef %r" % (float(total), n64, float(total) / n64 - 1, float(coef)))
    # a denormal square is at most 2^-150 from g^2 >= 2^-130: never more than 2^-20 relative above (flushed to 0: understated)
    assert 0.0 <= float(total) <= n64 * (1 + 2.0 ** -20) and float(coef) == 1.0
    lo = torch.full((4096,), 2.0 ** -76)                                           # g^2 = 2^-152 is 0 in float32; the norm is 2^-70
    dev = lo.cuda()
    total, coef = grad_norm_multi(addrs(dev, [4096]), [4096], 0.5)
    print("|g| = 2^-76: total %r (f64 %.6g), coef %r" % (float(total), 2.0 ** -70, float(coef)))
    assert 0.0 <= float(total) <= 2.0 ** -70 and float(coef) == 1.0


@pytest.mark.parametrize("bad,want_total,want_coef", [(math.inf, math.inf, 0.0), (-math.inf, math.inf, 0.0), (math.nan, math.nan, math.nan)])
def test_grad_norm_of_non_finite_gradients(bad, want_total, want_coef):
    """one +-inf: total = +inf, coef = 0; one NaN: total = NaN, coef = NaN (as torch's clamp gives); without clipping (max_norm <= 0)
    coef = 1 whatever the gradients hold"""
    c = I.norm_table_case(65, False)
    sizes = [t.numel() for t in c.ts]
    flat = torch.cat(c.ts).clone()
    flat[sum(sizes[:40]) + 17] = bad
    dev = flat.cuda()
    same = (lambda a, b: math.isnan(a) if math.isnan(b) else a == b)
    for mn in (0.5, 1e9):
        total, coef = grad_norm_multi(addrs(dev, sizes), sizes, mn)
        assert same(float(total), want_total) and same(float(coef), want_coef), (mn, float(total), float(coef))
    total, coef = grad_norm_multi(addrs(dev, sizes), sizes, 0.0)
    assert same(float(total), want_total) and float(coef) == 1.0


# ---- f ------------------------------------------------------------------------------------------------------------------------
def amax_run(x_dev, n, start=0.0):
    out = torch.full((1,), start, device="cuda")
    _lib.check(lib().ds_amax(_lib.ptr(x_dev), n, _lib.ptr(out), _lib.stream()))
    return out.cpu()


def bits(t):
    return int(t.view(torch.int32))


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "4-byte offset"])
@pytest.mark.parametrize("n", I.AMAX_SIZES + [I.AMAX_BIG])
def test_amax_exact_at_every_seam(n, shift):
    base = I.amax_base(n)
    buf = torch.zeros(n + 4, device="cuda")
    x = buf[shift:shift + n]
    assert x.data_ptr() % 16 == 4 * shift
    x.copy_(base)
    launches = 0
    for pos in I.amax_positions(n):
        for val in (3.5, -3.5):                                                    # the maximum at the seam, either sign
            x[pos] = val
            got = amax_run(x, n)
            assert float(got) == 3.5, "n %d, maximum %g at %d: %r" % (n, val, pos, float(got))
            launches += 1
        x[pos] = float(base[pos])
    want = R.amax(base)
    assert float(amax_run(x, n)) == want
    assert float(amax_run(x, n, 2.0 * want)) == 2.0 * want and float(amax_run(x, n, 0.5 * want)) == want     # max with what is there
    if n > 8192:
        return
    for pos in I.amax_positions(n):
        # NaNs are ignored, wherever they lie; +-inf wins
        y = base.clone()
        y[pos] = math.nan
        assert float(amax_run(buf[shift:shift + n].copy_(y), n)) == R.amax(y)
        for inf in (math.inf, -math.inf):
            y[pos] = inf
            assert float(amax_run(buf[shift:shift + n].copy_(y), n)) == math.inf, "n %d, %r at %d" % (n, inf, pos)
        # a denormal maximum among zeros; -0.0 leaves the result +0
        y = torch.zeros(n)
        y[pos] = -1e-40
        assert float(y[pos]) != 0.0
        got = amax_run(buf[shift:shift + n].copy_(y), n)
        assert bits(got) == bits(y[pos].abs()), "denormal maximum at %d: %r" % (pos, float(got))
    y = torch.full((n,), -0.0)
    assert bits(amax_run(buf[shift:shift + n].copy_(y), n)) == 0
    y = torch.full((n,), math.nan)
    assert bits(amax_run(buf[shift:shift + n].copy_(y), n)) == 0 and float(amax_run(x, n, 1.5)) == 1.5


# ---- g ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [0.99, 0.9999])
def test_ema_drift_over_300_updates(decay):
    d = I.ema_drift_case(decay)
    sizes = I.G_SIZES
    cur, e = d["cur"].cuda(), d["e0"].cuda()
    for s in range(I.G_UPDATES):
        tab, keep = records([addrs(e, sizes), addrs(cur[s], sizes)], sizes)
        _lib.check(lib().ds_ema_multi(tab, len(sizes), d["decay"], d["w"], _lib.stream()))
    got = e.cpu()
    worst = (0.0, 0.0, 0.0)
    for i, (err, d32, _) in enumerate(I.per_tensor(got, d["y"][0], d["y"][1], sizes)):
        assert err <= 4 * d32, "tensor %d: err %.3e, d32 %.3e" % (i, err, d32)
        worst = max(worst, (err / d32, err, d32))
    line = "ema drift, 300 updates at decay %g: worst tensor %s" % (decay, fmt(worst))
    print(line)
    parity_line(line)


# ---- h ------------------------------------------------------------------------------------------------------------------------
def test_norm_clip_adamw_chain():
    d = I.chain_case()
    sizes, y = d["sizes"], d["y"]
    N = sum(sizes)
    g = d["g"].cuda()
    hyper_all = torch.tensor(d["hyper"], dtype=torch.float32).cuda()
    hyper = torch.zeros(4, device="cuda")
    p, m, v = d["p0"].cuda(), torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    coefs = []
    for s in range(I.H_ITERS):
        hyper[:3].copy_(hyper_all[s][:3])
        ga = addrs(g[s], sizes)
        grad_norm_multi(ga, sizes, I.H_MAX_NORM, coef_ptr=_lib.ptr_off(hyper, 3))      # the coefficient goes straight into hyper[3]
        coefs.append(hyper[3:4].clone())
        adamw_multi(addrs(p, sizes), ga, addrs(m, sizes), addrs(v, sizes), sizes, hyper, I.H_BETAS, I.H_WD)
    coefs = [float(c) for c in coefs]
    assert [c < 1.0 for c in coefs] == [c < 1.0 for c in d["coefs"]]
    assert max(abs(a - b) for a, b in zip(coefs, d["coefs"])) <= 2.0 ** -22
    worst = max(check(t.cpu(), y[k], y[3 + k], sizes, "pmv"[k]) for k, t in enumerate((p, m, v)))
    line = "norm -> clip -> adamw, 20 iterations on 150 tensors (%d clip): worst tensor %s" % (sum(c < 1.0 for c in coefs), fmt(worst))
    print(line)
    parity_line(line)
