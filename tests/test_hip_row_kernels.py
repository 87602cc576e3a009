"""The row-wise kernels of the diffusion transformer (csrc/norm.hip on the forward path, csrc/train.hip on the backward path)
against float64 at their edges, each through its raw C entry: ds_adaln, ds_layernorm, ds_adaln_split, ds_layernorm_split,
ds_layernorm_bwd, ds_layernorm_bwd_sums, ds_gelu2, ds_softmax_bwd_rows, ds_colsum, ds_colsum_ws, ds_embed.

Inputs: tests/rows_inputs.py; float64 and float32 restatements: tests/rows_reference.py; tests/test_rows_host.py checks on the CPU
that the inputs are what they claim, that the restatements hold the bounds and the regime caps, and that wrong kernels do not.

Bounds.  A fixed-order fp32 chain without a multiply (the three column-sum forms, ds_embed) must match
its float32 restatement bit for bit.  A split-plane output must equal the split of the fp32-output kernel bit for bit.
Everything else, on every element:  |kernel - f64| <= 4 max(d32, 1 ulp), d32 = the float32 restatement's own distance from
float64 on the element's row, the ulp taken at the largest term added or subtracted to form the element.

Every output is pre-filled with NaN (the split planes with a bit pattern) and carries a 64-element guard that must come back
untouched.  Measured on an MI355X: every test's docstring carries its own figures."""
import pytest
import torch

import rows_inputs as I
import rows_reference as R
from conftest import parity_line

pytestmark = pytest.mark.gpu
NO_GRAD = True          # tests/conftest.py: every test of this module runs under torch.no_grad()
F64, F32 = torch.float64, torch.float32
D = I.D
GUARD = 64              # elements behind every output
NAN = float("nan")
SENT_H = 0x5A5A         # the split planes' sentinel (as int16 bits)
SENT_F = -12345.0


@pytest.fixture(scope="module")
def L():
    from text_to_sound_synthesis_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _lib.lib()
    return _lib


def _out(n, fill=NAN, dtype=F32):
    return torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")


def _untouched(buf, n, fill=NAN):
    g = buf[n:].cpu()
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


def _refused(L, rc, entry):
    return rc != 0 and entry in L.lib().ds_last_error_string().decode()


def _ceil16(m):
    return (m + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------ 1. the forward norms
def _norm_fp32(L, form, x, M, operands):
    """ds_layernorm (gamma, beta) or ds_adaln (table, t; L = ADA_L) into a NaN-filled buffer -> [M][D] on the host"""
    out = _out(M * D)
    xc = x.cuda()
    a, b = operands
    if form == "ln":
        L.check(L.lib().ds_layernorm(L.ptr(xc), L.ptr(out), M, D, L.ptr(a), L.ptr(b), L.stream()))
    else:
        L.check(L.lib().ds_adaln(L.ptr(xc), L.ptr(out), M, I.ADA_L, D, L.ptr(a), L.ptr(b), L.stream()))
    assert _untouched(out, M * D)
    return out[:M * D].cpu().view(M, D)


def _norm_operands(form):
    if form == "ln":
        g, b = I.ln_affine()
        return g.cuda(), b.cuda()
    _, _, tab, t = I.ada_operands(I.MAX_ROWS, I.ADA_L)
    return tab.cuda(), t.cuda()


def _norm_reference(regime, form):
    x = I.ln_rows(regime, I.MAX_ROWS, "fwd", form)
    scale, shift = I.ln_operands(I.MAX_ROWS) if form == "ln" else I.ada_operands(I.MAX_ROWS, I.ADA_L)[:2]
    y64, _, term = R.norm_forward(x, scale, shift, F64, form == "ada")
    y32, _, _ = R.norm_forward(x, scale, shift, F32, form == "ada")
    return x, shift, y64, y32, term


@pytest.mark.parametrize("regime", I.REGIMES)
def test_layernorm_and_adaln(L, regime):
    """ds_layernorm at M = 1, 3, 4, 5, 17, 33 and ds_adaln at the same M and at M = 15 (L = 5: three samples on the first, the
    last and a middle row of the table, a workgroup straddling two of them); gains +-(0.1 .. 3), AdaLN scales whose 1 + scale
    cancels.  Every element within 4 max(d32 of its row, 1 ulp at |x - mean| rstd |s|) of float64; on the constant
    row the output is the shift, bit for bit.
    Measured, worst error / bound (ds_layernorm | ds_adaln): zero_mean 0.340 | 0.283, mean_1e2 0.360 | 0.371, hot3 0.288 | 0.283,
    scale 2^-14 0.273 | 0.268, scale 2^14 0.331 | 0.307; the constant row exact (0 | 0)."""
    worst = {}
    for form in ("ln", "ada"):
        x, shift, y64, y32, term = _norm_reference(regime, form)
        ops = _norm_operands(form)
        for M in I.LN_M + ((I.ADA_L * I.ADA_B,) if form == "ada" else ()):
            k = _norm_fp32(L, form, x[:M].contiguous(), M, ops)
            rep = R.bound_report(k, y64[:M], y32[:M], term[:M])
            print("%s %s M %d: %.3f of the bound (d32 %.3g)" % (form, regime, M, rep["worst"], rep["d32"]))
            assert rep["ok"], (form, regime, M, rep)
            if regime == "const":
                assert torch.equal(k, shift[:M].contiguous()), "the constant row's output is not the shift"
            worst[form] = max(worst.get(form, 0.0), rep["worst"])
    parity_line("ds_layernorm | ds_adaln %s: worst error %.3f | %.3f of 4 max(d32, ulp)" % (regime, worst["ln"], worst["ada"]))


@pytest.mark.parametrize("regime", I.REGIMES)
def test_split_norms_equal_the_split_of_the_fp32_kernels(L, regime):
    """ds_layernorm_split / ds_adaln_split at M = 1, 15, 16, 17, 33 (the lo plane sits ceil16(M) D halves behind the hi plane):
    both planes, unpacked, equal torch_split of the fp32-output kernel's result bit for bit; the padding rows M .. ceil16(M) - 1
    of both planes and the guard keep the caller's bit pattern (the kernel stores rows < M only).
    Measured: 0 of 335 872 halves differ in every regime, every padding row untouched."""
    diff = halves = 0
    for form in ("ln", "ada"):
        x = _norm_reference(regime, form)[0]
        ops = _norm_operands(form)
        for M in I.SPLIT_M:
            xm = x[:M].contiguous()
            y = _norm_fp32(L, form, xm, M, ops)
            R16 = _ceil16(M)
            yh = _out(2 * R16 * D, SENT_H, torch.int16)
            xc = xm.cuda()
            if form == "ln":
                L.check(L.lib().ds_layernorm_split(L.ptr(xc), L.ptr(yh), M, D, L.ptr(ops[0]), L.ptr(ops[1]), L.stream()))
            else:
                L.check(L.lib().ds_adaln_split(L.ptr(xc), L.ptr(yh), M, I.ADA_L, D, L.ptr(ops[0]), L.ptr(ops[1]), L.stream()))
            assert _untouched(yh, 2 * R16 * D, SENT_H)
            planes = L.unpack_planes(yh[:2 * R16 * D].cpu(), R16, D)             # [2][R16][D] int16 bits
            want = R.torch_split(y).view(torch.int16)
            bad = int((planes[:, :M] != want).sum())
            assert bad == 0, (form, regime, M, bad)
            assert bool((planes[:, M:] == SENT_H).all()), "a padding row of a split plane was written"
            diff, halves = diff + bad, halves + 2 * M * D
    parity_line("ds_layernorm_split | ds_adaln_split %s: %d of %d halves differ from the split of the fp32 kernels; padding rows "
                "untouched" % (regime, diff, halves))


# ------------------------------------------------------------------------------------------------ 2. the backward norms
def _bwd_run(L, kind, x, dy, prev, mode, n, ops, accumulate=0, with_dyxn=True):
    """kind 'plain': ds_layernorm_bwd -> dx, dyxn;  'sums': ds_layernorm_bwd_sums -> dx, part [G cpg][2][D]"""
    M = x.shape[0]
    Lr = n if mode == 0 else 1
    dx = _out(M * D)
    if accumulate:
        dx[:M * D] = prev.cuda().view(-1)
    xc, dc = x.cuda(), dy.cuda()
    tab, t, gamma = (ops[0], ops[1], None) if mode == 0 else (None, None, ops)
    if kind == "plain":
        px = _out(M * D) if with_dyxn else None
        L.check(L.lib().ds_layernorm_bwd(L.ptr(xc), L.ptr(dc), L.ptr(dx), L.ptr(px), M, Lr, D, mode, L.ptr(tab), L.ptr(t), L.ptr(gamma),
                                         L.stream()))
        assert _untouched(dx, M * D) and (px is None or _untouched(px, M * D))
        return dx[:M * D].cpu().view(M, D), None if px is None else px[:M * D].cpu().view(M, D)
    G = M // n if mode == 0 else 1
    cpg = L.lib().ds_layernorm_bwd_chunks(M, Lr, mode)
    assert cpg == R.chunking(n)[0]
    part = _out(G * cpg * 2 * D)
    L.check(L.lib().ds_layernorm_bwd_sums(L.ptr(xc), L.ptr(dc), L.ptr(dx), L.ptr(part), M, Lr, D, mode, L.ptr(tab), L.ptr(t),
                                          L.ptr(gamma), accumulate, L.stream()))
    assert _untouched(dx, M * D) and _untouched(part, G * cpg * 2 * D)
    return dx[:M * D].cpu().view(M, D), part[:G * cpg * 2 * D]


def _grad_sums(L, part, G, cpg):
    """ds_colsum over the chunks of part -> [G][2][D]"""
    out = _out(G * 2 * D)
    L.check(L.lib().ds_colsum(L.ptr(part), L.ptr(out), G, cpg, 2 * D, 2 * D, cpg * 2 * D, 0, L.stream()))
    assert _untouched(out, G * 2 * D)
    return out[:G * 2 * D].cpu().view(G, 2, D)


@pytest.mark.parametrize("regime", I.REGIMES)
def test_layernorm_backward(L, regime):
    """ds_layernorm_bwd (with and without dyxn) and ds_layernorm_bwd_sums (accumulate 0 and 1) on every row regime x dy scaled by
    2^-40, 1, 2^20; mode 1 at M = 1, 3, 15, 16, 17, 33, mode 0 at L = 1, 5, 16, 17, 33 x three samples (one and several chunks, a
    shorter last chunk, waves that own no row and still store their zero partial).  dx of both kernels and dyxn on every element
    within 4 max(d32 of the row, 1 ulp at rstd max(|g|, |mg|, |xn mgx|)) of float64; the scale and shift gradients after ds_colsum
    of part within the bound per element; part fully written, guards intact; a second run bit-equal; on the constant row dyxn
    and the scale gradient are exactly 0.
    Measured, worst error / bound (dx | dyxn | gradient sums): zero_mean 0.535 | 0.600 | 0.334, mean_1e2 0.380 | 0.400 | 0.318,
    hot3 0.479 | 0.505 | 0.733, scale 2^-14 0.450 | 0.486 | 0.457, scale 2^14 0.472 | 0.563 | 0.409, const 0.250 | 0 | 0.250."""
    worst = {"dx": 0.0, "dyxn": 0.0, "sums": 0.0}
    for dy_name in I.DY_SCALES:
        for mode, sizes in ((1, I.BWD_M), (0, I.BWD_L)):
            for n in sizes:
                x, dy, prev, scale, ops = I.bwd_case(regime, dy_name, mode, n)
                ops = tuple(o.cuda() for o in ops) if mode == 0 else ops.cuda()
                G = 1 if mode == 1 else I.BWD_B
                dx64, px64, term, xn64 = R.norm_backward(x, dy, scale, F64, mode == 0)
                dx32, px32, _, xn32 = R.norm_backward(x, dy, scale, F32, mode == 0)
                tag = (regime, dy_name, mode, n)
                dx_a, px = _bwd_run(L, "plain", x, dy, prev, mode, n, ops)
                dx_b, _ = _bwd_run(L, "plain", x, dy, prev, mode, n, ops, with_dyxn=False)
                dx_c, part = _bwd_run(L, "sums", x, dy, prev, mode, n, ops)
                dx_d, part_d = _bwd_run(L, "sums", x, dy, prev, mode, n, ops, accumulate=1)
                for name, k in (("bwd", dx_a), ("bwd, no dyxn", dx_b), ("bwd_sums", dx_c)):
                    rep = R.bound_report(k, dx64, dx32, term)
                    assert rep["ok"], (tag, name, rep)
                    worst["dx"] = max(worst["dx"], rep["worst"])
                p = prev.double()
                rep = R.bound_report(dx_d, dx64 + p, dx32 + prev, torch.maximum(term, p.abs()))
                assert rep["ok"], (tag, "bwd_sums accumulate", rep)
                worst["dx"] = max(worst["dx"], rep["worst"])
                rep = R.bound_report(px, px64, px32)
                assert rep["ok"], (tag, "dyxn", rep)
                worst["dyxn"] = max(worst["dyxn"], rep["worst"])
                assert not torch.isnan(part).any(), "a partial of ds_layernorm_bwd_sums was not stored"
                assert torch.equal(part, part_d), "part depends on accumulate"
                cpg = R.chunking(n)[0]
                sums = _grad_sums(L, part, G, cpg)
                s64, sterm = R.bwd_sums(dy, xn64, G, n, F64)
                s32, _ = R.bwd_sums(dy, xn32, G, n, F32)
                rep = R.bound_report(sums.view(-1, D), s64.view(-1, D), s32.view(-1, D), sterm.view(-1, D))
                assert rep["ok"], (tag, "sums", rep)
                worst["sums"] = max(worst["sums"], rep["worst"])
                dx_c2, part2 = _bwd_run(L, "sums", x, dy, prev, mode, n, ops)
                assert torch.equal(dx_c, dx_c2) and torch.equal(part, part2), "a second run differs"
                if regime == "const":
                    assert (px == 0).all() and (sums[:, 0] == 0).all()
        print("layernorm backward %s dy %s: %s" % (regime, dy_name, worst))
    parity_line("ds_layernorm_bwd | _bwd_sums %s: worst error dx %.3f, dyxn %.3f, scale / shift gradients %.3f of 4 max(d32, ulp)"
                % (regime, worst["dx"], worst["dyxn"], worst["sums"]))


# ------------------------------------------------------------------------------------------------ 3. GELU2
def _gelu(L, x, dy):
    n = x.numel()
    out = _out(n)
    xc, dc = x.cuda(), None if dy is None else dy.cuda()
    L.check(L.lib().ds_gelu2(L.ptr(xc), L.ptr(dc), L.ptr(out), n, L.stream()))
    assert _untouched(out, n)
    return out[:n].cpu()


@pytest.mark.parametrize("n", I.GELU_N)
def test_gelu2(L, n):
    """n = 4, 1020, 1024, 1028 (one workgroup covers 1024 elements) of a grid over [-100, 100] with +-0, the fp32 neighbours of the
    derivative's zero (-0.75115), +-52 and +-53 (where expf(1.702 |x|) passes fp32's range), the smallest normal and a
    denormal; forward, and backward with dy scaled by 2^-40, 1, 2^20.  Every element within 4 max(d32 of the element, 1 ulp at
    |dy| max(sg, |1.702 x sg (1 - sg)|)) of float64, outputs that are denormal in float64 within 2^-126.
    Measured, worst error / bound (forward | backward): n = 4 0.241 | 0.222; n = 1020, 1024, 1028 0.426 | 0.475, the same at the
    three dy scales."""
    x = I.gelu_grid()[:n]
    worst = {}
    for dy_name in (None,) + tuple(I.DY_SCALES):
        dy = None if dy_name is None else I.gelu_dy(n, dy_name)
        k = _gelu(L, x, dy)
        y64, term = R.gelu2(x, dy, F64)
        y32, _ = R.gelu2(x, dy, F32)
        rep = R.bound_report(k[None], y64[None], y32[None], term[None], dim=None, floor_denormal=True)
        print("ds_gelu2 n %d dy %s: %.3f of the bound" % (n, dy_name, rep["worst"]))
        assert rep["ok"], (n, dy_name, rep)
        key = "fwd" if dy is None else "bwd"
        worst[key] = max(worst.get(key, 0.0), rep["worst"])
    parity_line("ds_gelu2 n %d: worst error forward %.3f, backward %.3f of 4 max(d32, ulp)" % (n, worst["fwd"], worst["bwd"]))


def test_gelu2_nonfinite(L):
    """x = +inf, -inf, NaN, 1: the expectation is torch's x sigmoid(1.702 x) and its autograd derivative in float64 -- NaN where
    torch gives NaN (forward at -inf and NaN; backward at +-inf and NaN), +inf forward at +inf, the bound at 1.
    Measured: NaN and inf in the same places, the finite element (x = 1) at 0.064 (forward) and 0.225 (backward) of the bound."""
    x = I.gelu_nonfinite()
    with torch.enable_grad():
        x64 = x.double().requires_grad_(True)
        want = x64 * torch.sigmoid(1.702 * x64)
        dwant, = torch.autograd.grad(want.sum(), x64)
    for dy, w in ((None, want.detach()), (torch.ones(4), dwant)):
        k = _gelu(L, x, dy)
        assert torch.equal(torch.isnan(k), torch.isnan(w)), (k, w)
        inf = torch.isinf(w)
        assert torch.equal(k[inf].double(), w[inf])
        fin = torch.isfinite(w)
        y64, term = R.gelu2(x[fin], None if dy is None else dy[fin], F64)
        y32, _ = R.gelu2(x[fin], None if dy is None else dy[fin], F32)
        assert float((y64 - w[fin]).abs().max()) < 1e-15
        rep = R.bound_report(k[fin][None], y64[None], y32[None], term[None], dim=None)
        assert rep["ok"], rep
        parity_line("ds_gelu2 %s at +inf, -inf, NaN, 1: NaN / inf where torch has them; x = 1 at %.3f of 4 max(d32, ulp)"
                    % ("forward" if dy is None else "backward", rep["worst"]))


# ------------------------------------------------------------------------------------------------ 4. softmax backward
@pytest.mark.parametrize("n", I.SB_N)
def test_softmax_backward_rows(L, n):
    """rows 1, 3, 4, 5; ld = n, n + 1, 288; P from scores of spread 4, of spread 40 (nearly one-hot), exactly one-hot, uniform; dP
    of order 1, 1e4 + order 1 (the cancellation in dP - s), scaled by 2^-40; scale 0.125.  Every element within 4 max(d32 of the
    row, 1 ulp at scale P max(|dP|, |s|)) of float64; one-hot rows: dS exactly 0 where P is 0; columns n .. ld - 1 come back
    exactly 0 (they held 777 against P = 0.5: a sum over ld would show), the guard untouched.
    Measured, worst error / bound: 0.250 at every n but 1 (n = 1: dS = 0 exactly) -- the kernel's error is its restatement's."""
    worst = 0.0
    for p_regime in I.SB_P:
        for dp_regime in I.SB_DP:
            P, dP = I.sb_case(p_regime, dp_regime, n)
            y64, term = R.softmax_bwd(P, dP, n, I.SB_SCALE, F64)
            y32, _ = R.softmax_bwd(P, dP, n, I.SB_SCALE, F32)
            for ld in I.sb_ld(n):
                for rows in I.SB_ROWS:
                    Pb = torch.full((rows, ld), I.SB_PAD_P)
                    Pb[:, :n] = P[:rows]
                    buf = _out(rows * ld)
                    v = buf[:rows * ld].view(rows, ld)
                    v[:] = I.SB_PAD_DP
                    v[:, :n] = dP[:rows].cuda()
                    pc = Pb.cuda()
                    L.check(L.lib().ds_softmax_bwd_rows(L.ptr(pc), L.ptr(buf), rows, n, ld, I.SB_SCALE, L.stream()))
                    assert _untouched(buf, rows * ld)
                    got = v.cpu()
                    assert (got[:, n:] == 0).all(), "padding columns"
                    k = got[:, :n]
                    rep = R.bound_report(k, y64[:rows], y32[:rows], term[:rows])
                    assert rep["ok"], (p_regime, dp_regime, ld, rows, rep)
                    if p_regime == "one_hot":
                        assert (k[P[:rows] == 0] == 0).all()
                    worst = max(worst, rep["worst"])
            print("ds_softmax_bwd_rows n %d %s %s: worst so far %.3f" % (n, p_regime, dp_regime, worst))
    parity_line("ds_softmax_bwd_rows n %d: worst error %.3f of 4 max(d32, ulp); padding columns 0" % (n, worst))


# ------------------------------------------------------------------------------------------------ 5. column sums
def _colsum(L, xs, G, R_, C, ld, gstride, start, ws=None):
    """xs: the device tensor the kernel reads; start None: accumulate 0 into NaN, else accumulate 1 onto start [G][C].
    ws = (work buffer or None, work_floats): ds_colsum_ws."""
    out = _out(G * C)
    if start is not None:
        out[:G * C] = start.cuda().view(-1)
    acc = int(start is not None)
    if ws is None:
        L.check(L.lib().ds_colsum(L.ptr(xs), L.ptr(out), G, R_, C, ld, gstride, acc, L.stream()))
    else:
        L.check(L.lib().ds_colsum_ws(L.ptr(xs), L.ptr(out), G, R_, C, ld, gstride, acc, L.ptr(ws[0]), ws[1], L.stream()))
    assert _untouched(out, G * C)
    return out[:G * C].cpu().view(G, C)


def _cs_device(x, extra=7):
    """x [G][R][ld] (NaN past column C) -> the device buffer with `extra` NaN floats between the groups, and its gstride"""
    G, R_, ld = x.shape
    xs = torch.full((G, R_ * ld + extra), NAN)
    xs[:, :R_ * ld] = x.reshape(G, -1)
    return xs.cuda(), R_ * ld + extra


def _cs_check(k, x, C, start, y32):
    diff = R.differing(k, y32)
    xr = x[:, :, :C]
    term = R.colsum_term(xr) if start is None else torch.maximum(R.colsum_term(xr), start.double().abs())
    rep = R.bound_report(k, R.colsum(xr, F64, start), y32, term)
    return diff, rep


@pytest.mark.parametrize("G", I.CS_G)
def test_colsum_both_kernels_bit_exact(L, G):
    """R = 1, 3, 4, 5, 15, 16, 17, 19, 67, 83 (the 16-, 4- and 1-row batch seams of the four-chain loop, the R % 4 tail) x C = 1, 63,
    64, 65, 257, ld = C + 3, NaN in the columns past C and between the groups, accumulate 0 and 1 onto a non-zero start; by the
    entry's rule the four-chain kernel runs from R = 16, the one-thread kernel below, and for (1, 19, 65537) and (1, 4, 70001).
    Also the position gradient's interleaved layout (gstride = D < ld = G D, Lx 5, B 3, D 64).  Data spread over 2^+-20 with
    mixed signs.  Bit-equal to the fp32 restatement of the documented order (four chains interleaved by row, tail rows on chain
    0, (s0 + s1) + (s2 + s3)) and within 4 max(d32, ulp) of float64 per element.
    Measured: 0 elements differ in every case."""
    cases = diff = 0
    sides = set()
    shapes = [(G, R_, C) for R_ in I.CS_R for C in I.CS_C] + ([c for c in I.CS_WIDE] if G == 1 else [])
    for g, R_, C in shapes:
        sides.add((I.cs_four_chain(g, R_, C), R_ >= 16))
        x, start = I.cs_case(g, R_, C)
        xs, gstride = _cs_device(x)
        for st in (None, start):
            y32 = R.colsum(x[:, :, :C], F32, st)
            k = _colsum(L, xs, g, R_, C, C + 3, gstride, st)
            d, rep = _cs_check(k, x, C, st, y32)
            assert d == 0, ((g, R_, C), st is not None, d, "four-chain" if I.cs_four_chain(g, R_, C) else "one-thread")
            assert rep["ok"], rep
            cases, diff = cases + 1, diff + d
    assert (True, True) in sides and (False, False) in sides and (G > 1 or (False, True) in sides)
    if G == 3:
        Lx, B, Dp = I.CS_POS                                       # train.py: ds_colsum(dx, dpos, Lx, B, D, Lx D, D, ...)
        dx = I.cs_data((B, Lx, Dp), "pos")
        dc = dx.cuda()
        for st in (None, I.cs_data((Lx, Dp), "pos.start")):
            k = _colsum(L, dc, Lx, B, Dp, Lx * Dp, Dp, st)
            d = R.differing(k, R.colsum(dx.transpose(0, 1), F32, st))
            assert d == 0, ("position layout", d)
            cases, diff = cases + 1, diff + d
    parity_line("ds_colsum G %d: %d cases (both kernels), %d elements differ from the fp32 restatement" % (G, cases, diff))


@pytest.mark.parametrize("shape", I.CS_WS, ids=lambda s: "x".join(map(str, s)))
def test_colsum_ws_chunked_order(L, shape):
    """(G, R, C) = (1, 1025, 256): 64 chunks of 17 rows, the last three empty (exact zeros); (1, 33, 300) and (3, 40, 257): three
    chunks, the last shorter; (2, 16, 65): one chunk, falls through to ds_colsum.  Bit-equal to the restatement (chunks summed
    from their own first row, then added in index order), accumulate 0 and 1; with work = NULL the plain order; a workspace one
    float short is refused under the entry's name and nothing is written; the workspace's guard is untouched.
    Measured: 0 elements differ in every form."""
    G, R_, C = shape
    rs = I.cs_chunks(G, R_, C)
    x, start = I.cs_case(G, R_, C)
    xs, gstride = _cs_device(x)
    xr = x[:, :, :C]
    diff = 0
    for st in (None, start):
        work = _out(G * rs * C)
        k = _colsum(L, xs, G, R_, C, C + 3, gstride, st, ws=(work, G * rs * C))
        assert _untouched(work, G * rs * C)
        y32 = R.colsum_ws(xr, rs, F32, st) if rs > 1 else R.colsum(xr, F32, st)
        d, rep = _cs_check(k, x, C, st, y32)
        assert d == 0 and rep["ok"], (shape, st is not None, d, rep)
        if rs > 1:
            assert not torch.isnan(work[:G * rs * C]).any()
            if shape == (1, 1025, 256):
                assert (work[:G * rs * C].view(rs, C)[61:] == 0).all(), "an empty trailing chunk is not an exact zero"
        k0 = _colsum(L, xs, G, R_, C, C + 3, gstride, st, ws=(None, 0))
        d0 = R.differing(k0, R.colsum(xr, F32, st))
        assert d0 == 0, (shape, "work = NULL", d0)
        diff += d + d0
    if rs > 1:
        out, work = _out(G * C), _out(G * rs * C)
        rc = L.lib().ds_colsum_ws(L.ptr(xs), L.ptr(out), G, R_, C, C + 3, gstride, 0, L.ptr(work), G * rs * C - 1, L.stream())
        assert _refused(L, rc, "ds_colsum_ws"), (rc, L.lib().ds_last_error_string())
        torch.cuda.synchronize()
        assert _untouched(out, 0) and _untouched(work, 0)
    parity_line("ds_colsum_ws %s: %d chunks, %d elements differ from the fp32 restatement" % ("x".join(map(str, shape)), rs, diff))


# ------------------------------------------------------------------------------------------------ 6. ds_embed
def test_embed_edges(L):
    """M = 1, 5, 7 with L = 5 and L = 7; tokens 0, the last table row and a negative id (reads row 0): torch.equal with
    emb[tok] + pos in fp32.  No token at or past the table's size: the kernel has no bound to check against.
    Measured: 0 elements differ."""
    diff = 0
    for M, Lr in I.EMB_CASES:
        tok, emb, pos = I.embed_case(M, Lr)
        out = _out(M * D)
        tc, ec, pc = tok.cuda(), emb.cuda(), pos.cuda()
        L.check(L.lib().ds_embed(L.ptr(tc), L.ptr(ec), L.ptr(pc), L.ptr(out), M, Lr, D, L.stream()))
        assert _untouched(out, M * D)
        k = out[:M * D].cpu().view(M, D)
        want = R.embed(tok, emb, pos, Lr)
        assert torch.equal(k, want), (M, Lr)
        diff += R.differing(k, want)
    parity_line("ds_embed M 1, 5, 7 x L 5, 7: %d elements differ from emb[tok] + pos" % diff)


# ------------------------------------------------------------------------------------------------ 7. arguments
def test_argument_errors_launch_nothing(L):
    """D != 1024, n % 4 != 0, ld < n, ld < C, M % L != 0 (sums form, mode 0), null pointers, and M <= 0 / L <= 0 of the four
    forward norms (accepted before: an empty grid, or a division by zero in the kernel): a non-zero return, ds_last_error_string
    names the entry (ds_layernorm_bwd's refusals named a static helper, ln_bwd_launch, before), no output is written."""
    lib, p, st = L.lib(), L.ptr, L.stream()
    f = lambda n, fill=SENT_F, dtype=F32: torch.full((n,), fill, dtype=dtype, device="cuda")
    src, tt, tok = f(8 * 2 * D, 0.5), torch.zeros(8, dtype=torch.int64, device="cuda"), torch.zeros(64, dtype=torch.int64, device="cuda")
    o1, o2, oh = f(8 * D), f(8 * 2 * D), f(2 * 16 * D, SENT_H, torch.int16)
    entries = {
        "ds_adaln": (dict(x=p(src), y=p(o1), M=4, L=2, D=D, tab=p(src), t=p(tt)),
                     lambda a: lib.ds_adaln(a["x"], a["y"], a["M"], a["L"], a["D"], a["tab"], a["t"], st),
                     [dict(x=None), dict(y=None), dict(tab=None), dict(t=None), dict(D=512), dict(D=1028), dict(M=0), dict(M=-1),
                      dict(L=0), dict(L=-2)]),
        "ds_layernorm": (dict(x=p(src), y=p(o1), M=4, D=D, g=p(src), b=p(src)),
                         lambda a: lib.ds_layernorm(a["x"], a["y"], a["M"], a["D"], a["g"], a["b"], st),
                         [dict(x=None), dict(y=None), dict(g=None), dict(b=None), dict(D=512), dict(M=0), dict(M=-1)]),
        "ds_adaln_split": (dict(x=p(src), y=p(oh), M=4, L=2, D=D, tab=p(src), t=p(tt)),
                           lambda a: lib.ds_adaln_split(a["x"], a["y"], a["M"], a["L"], a["D"], a["tab"], a["t"], st),
                           [dict(x=None), dict(y=None), dict(tab=None), dict(t=None), dict(D=512), dict(M=0), dict(M=-1), dict(L=0),
                            dict(L=-2)]),
        "ds_layernorm_split": (dict(x=p(src), y=p(oh), M=4, D=D, g=p(src), b=p(src)),
                               lambda a: lib.ds_layernorm_split(a["x"], a["y"], a["M"], a["D"], a["g"], a["b"], st),
                               [dict(x=None), dict(y=None), dict(g=None), dict(b=None), dict(D=512), dict(M=0), dict(M=-1)]),
        "ds_layernorm_bwd": (dict(x=p(src), dy=p(src), dx=p(o1), px=p(o2), M=4, L=2, D=D, mode=0, tab=p(src), t=p(tt), g=p(src)),
                             lambda a: lib.ds_layernorm_bwd(a["x"], a["dy"], a["dx"], a["px"], a["M"], a["L"], a["D"], a["mode"], a["tab"],
                                                            a["t"], a["g"], st),
                             [dict(x=None), dict(dy=None), dict(dx=None), dict(tab=None), dict(t=None), dict(mode=1, g=None), dict(D=512),
                              dict(M=0), dict(L=0), dict(mode=2)]),
        "ds_layernorm_bwd_sums": (dict(x=p(src), dy=p(src), dx=p(o1), part=p(o2), M=4, L=2, D=D, mode=0, tab=p(src), t=p(tt), g=p(src)),
                                  lambda a: lib.ds_layernorm_bwd_sums(a["x"], a["dy"], a["dx"], a["part"], a["M"], a["L"], a["D"], a["mode"],
                                                                      a["tab"], a["t"], a["g"], 0, st),
                                  [dict(x=None), dict(dy=None), dict(dx=None), dict(part=None), dict(tab=None), dict(t=None),
                                   dict(mode=1, g=None), dict(D=512), dict(M=0), dict(L=0), dict(L=3), dict(mode=2)]),
        "ds_gelu2": (dict(x=p(src), out=p(o1), n=8), lambda a: lib.ds_gelu2(a["x"], None, a["out"], a["n"], st),
                     [dict(x=None), dict(out=None), dict(n=0), dict(n=-4), dict(n=6), dict(n=1)]),
        "ds_softmax_bwd_rows": (dict(P=p(src), dP=p(o1), rows=4, n=8, ld=8),
                                lambda a: lib.ds_softmax_bwd_rows(a["P"], a["dP"], a["rows"], a["n"], a["ld"], 1.0, st),
                                [dict(P=None), dict(dP=None), dict(rows=0), dict(n=0), dict(ld=7), dict(rows=-1)]),
        "ds_colsum": (dict(x=p(src), out=p(o1), G=2, R=3, C=8, ld=8),
                      lambda a: lib.ds_colsum(a["x"], a["out"], a["G"], a["R"], a["C"], a["ld"], 24, 0, st),
                      [dict(x=None), dict(out=None), dict(G=0), dict(R=0), dict(C=0), dict(ld=7)]),
        "ds_colsum_ws": (dict(x=p(src), out=p(o1), G=2, R=3, C=8, ld=8),
                         lambda a: lib.ds_colsum_ws(a["x"], a["out"], a["G"], a["R"], a["C"], a["ld"], 24, 0, p(o2), 8 * 2 * D, st),
                         [dict(x=None), dict(out=None), dict(G=0), dict(R=0), dict(C=0), dict(ld=7)]),
        "ds_embed": (dict(tok=p(tok), emb=p(src), pos=p(src), out=p(o1), M=4, L=2, D=D),
                     lambda a: lib.ds_embed(a["tok"], a["emb"], a["pos"], a["out"], a["M"], a["L"], a["D"], st),
                     [dict(tok=None), dict(emb=None), dict(pos=None), dict(out=None), dict(M=0), dict(L=0), dict(D=1022)]),
    }
    for name, (ok, call, bads) in entries.items():
        for bad in bads:
            rc = call(dict(ok, **bad))
            assert _refused(L, rc, name), (name, bad, rc, lib.ds_last_error_string())
            with pytest.raises(L.DiffsoundHipError):
                L.check(rc)
    torch.cuda.synchronize()
    for o, fill in ((o1, SENT_F), (o2, SENT_F), (oh, SENT_H)):
        assert bool((o.cpu() == fill).all()), "a refused call wrote to an output"
    for name, (ok, call, _) in entries.items():                               # the table's own calls are valid ones
        assert call(ok) == 0, (name, lib.ds_last_error_string())
    torch.cuda.synchronize()
