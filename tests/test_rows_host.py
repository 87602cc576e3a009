"""CPU checks behind tests/test_hip_row_kernels.py: the inputs of tests/rows_inputs.py are what they claim to be, the float32
restatements of tests/rows_reference.py hold every bound and every regime cap, the regimes left out cannot hold a cap, and each
deliberately wrong kernel (`variant`) breaks its bound on at least one case.  Nothing here needs a GPU."""
import math

import pytest
import torch

import rows_inputs as I
import rows_reference as R

F64, F32 = R.F64, R.F32
D = I.D


def _holds(y32, y64, term=None, **kw):
    return R.bound_report(y32, y64, y32, term, **kw)


def _breaks(wrong, y64, y32, term=None, **kw):
    return not R.bound_report(wrong, y64, y32, term, **kw)["ok"]


# ------------------------------------------------------------------------------------------------ the regimes
def test_row_regimes_are_what_they_claim():
    for regime in I.REGIMES + I.LEFT_OUT:
        x = I.ln_rows(regime, 33, "claim").double()
        mean, sd = x.mean(1), x.std(1, unbiased=False)
        if regime == "zero_mean":
            assert (mean.abs() < 1e-7).all() and ((sd - 1).abs() < 0.05).all()
        elif regime == "mean_1e2":
            assert ((mean / sd - 100).abs() < 5).all()
        elif regime == "mean_1e4":
            assert ((mean / sd / 1e4 - 1).abs() < 0.05).all()
        elif regime == "hot3":
            rest = torch.ones(D, dtype=torch.bool)
            rest[list(I.HOT)] = False
            assert float(x[:, list(I.HOT)].abs().median()) > 100 * float(x[:, rest].abs().max()) / 10
            assert float(x[:, rest].abs().max()) < 2 and float(x[:, list(I.HOT)].abs().max()) > 1e3
        elif regime == "scale_2^-14":
            assert ((sd * 2.0 ** 14 - 1).abs() < 0.05).all() and float((sd ** 2).max()) < I.EPS / 1000   # eps rules rstd
        elif regime == "scale_2^14":
            assert ((sd * 2.0 ** -14 - 1).abs() < 0.05).all()
        elif regime == "const":
            assert (x == I.CONST).all()
        elif regime == "near_const":
            assert int((x != I.CONST).sum()) == 33
    k = torch.arange(1, D + 1, dtype=F64) * I.CONST               # every partial sum of the constant row is an fp32 number
    assert torch.equal(k.float().double(), k)
    g, b = I.ln_affine()
    assert 0.1 <= float(g.abs().min()) and float(g.abs().max()) <= 3.0 and float(g.abs().max() / g.abs().min()) > 10 and (g < 0).any()
    tab = I.adaln_table()
    s = 1.0 + tab[:, :D].double()
    assert float(s[:, :64].abs().max()) <= 2.0 ** -10 and 0.09 < float(s[:, 64:].abs().min()) and float(s.abs().max()) < 3.01
    assert I.adaln_t(3).tolist() == [0, I.ADA_T - 1, 3] and len(set(I.adaln_t(3).tolist())) == 3
    assert (I.ADA_L * I.ADA_B) % 4 != 0 and I.ADA_L % 4 != 0      # a workgroup of four rows straddles two samples


@pytest.mark.parametrize("form", ("ln", "ada"))
def test_constant_row_is_exact(form):
    """mean = 3.75 and x - mean = 0 exactly, so xn = +-0 and y is the shift, bit for bit -- in the restatement as in any order"""
    M = 15
    x = I.ln_rows("const", M)
    scale, shift = I.ln_operands(M) if form == "ln" else I.ada_operands(M, I.ADA_L)[:2]
    mean, rstd = R.row_stats(x, F32)
    assert (mean == I.CONST).all() and R.same_floats(rstd, torch.full_like(rstd, 1.0) / torch.sqrt(torch.tensor(1e-5, dtype=F32)))
    y, xn, _ = R.norm_forward(x, scale, shift, F32, form == "ada")
    assert (xn == 0).all() and torch.equal(y, shift.contiguous())
    dx, dyxn, _, _ = R.norm_backward(x, I.dy_rows(M, "1", "c"), scale, F32, form == "ada")
    assert (dyxn == 0).all() and torch.isfinite(dx).all()


# ------------------------------------------------------------------------------------------------ forward norms
def _forward(regime, form, variant=None, dtype=F32):
    M = 33 if form == "ln" else I.ADA_L * I.ADA_B
    x = I.ln_rows(regime, M, "fwd", form)
    scale, shift = I.ln_operands(M) if form == "ln" else I.ada_operands(M, I.ADA_L)[:2]
    return R.norm_forward(x, scale, shift, dtype, form == "ada", variant)


@pytest.mark.parametrize("form", ("ln", "ada"))
@pytest.mark.parametrize("regime", I.REGIMES)
def test_forward_restatement_holds_bound_and_cap(regime, form):
    y64, _, term = _forward(regime, form, dtype=F64)
    y32, _, _ = _forward(regime, form)
    rep = _holds(y32, y64, term)
    print("forward %s %s: d32 %.3g, cap figure %.3g" % (form, regime, rep["d32"], rep["cap"]))
    assert rep["ok"] and torch.isfinite(y64).all()
    if regime != "const":                                          # (the constant row: y = shift, checked exactly above)
        assert rep["cap"] <= I.CAP[regime], rep


def test_forward_mutants_break_the_bound():
    broke = {"var_keeps_mean": 0, "scale_without_one": 0}
    for regime in I.REGIMES:
        for form in ("ln", "ada"):
            y64, _, term = _forward(regime, form, dtype=F64)
            y32, _, _ = _forward(regime, form)
            for v in broke:
                broke[v] += _breaks(_forward(regime, form, v)[0], y64, y32, term)
    assert broke["var_keeps_mean"] >= 2 and broke["scale_without_one"] >= 5, broke
    y64, _, term = _forward("mean_1e2", "ln", dtype=F64)          # E[x^2] on a mean of 1e2 sd: xn is 100 x too small
    assert _breaks(_forward("mean_1e2", "ln", "var_keeps_mean")[0], y64, _forward("mean_1e2", "ln")[0], term)


# ------------------------------------------------------------------------------------------------ backward norms
def _backward(regime, dy_name, mode, variant=None, dtype=F32, n=17):
    x, dy, prev, scale, _ = I.bwd_case(regime, dy_name, mode, n)
    return R.norm_backward(x, dy, scale, dtype, mode == 0, variant)


@pytest.mark.parametrize("dy_name", list(I.DY_SCALES))
@pytest.mark.parametrize("regime", I.REGIMES + I.LEFT_OUT)
def test_backward_restatement_holds_bound_and_cap(regime, dy_name):
    """dx and dyxn of both modes; the gradient sums after the chunk partials and ds_colsum's order.  Measured cap figures (d32 / the
    row's largest |value|, the larger of dx and dyxn): <= 2.2e-7 on zero_mean, hot3, the scaled rows and the constant row (dx),
    4.8e-6 on mean_1e2; mean_1e4 reaches 5.7e-4 and near_const 1.4e-3 (both in dyxn, through xn): they hold no cap and are not
    GPU cases."""
    worst = 0.0
    for mode in (1, 0):
        dx64, px64, term, xn64 = _backward(regime, dy_name, mode, dtype=F64)
        dx32, px32, _, xn32 = _backward(regime, dy_name, mode)
        rep, rep_p = _holds(dx32, dx64, term), _holds(px32, px64)
        print("backward mode %d %s dy %s: dx cap figure %.3g, dyxn %.3g" % (mode, regime, dy_name, rep["cap"], rep_p["cap"]))
        assert rep["ok"] and rep_p["ok"] and torch.isfinite(dx64).all()
        worst = max(worst, rep["cap"], rep_p["cap"])
        if regime in I.LEFT_OUT:
            continue
        assert rep["cap"] <= I.CAP[regime], rep
        if regime == "const":
            assert (px32 == 0).all() and (px64 == 0).all()
        else:
            assert rep_p["cap"] <= I.CAP[regime], rep_p
        x, dy, _, _, _ = I.bwd_case(regime, dy_name, mode, 17)
        G = 1 if mode == 1 else I.BWD_B
        s64, sterm = R.bwd_sums(dy, xn64, G, 17, F64)
        s32, _ = R.bwd_sums(dy, xn32, G, 17, F32)
        assert _holds(s32.view(-1, D), s64.view(-1, D), sterm.view(-1, D))["ok"]
        if regime == "const":
            assert (s32[:, 0] == 0).all()
    assert regime not in I.LEFT_OUT or worst > 2.0 ** -16, worst


def test_backward_mutants_break_the_bound():
    broke = {"no_mg": 0, "no_xn_mgx": 0, "mean_g_short": 0}
    for regime in I.REGIMES:
        for dy_name in I.DY_SCALES:
            for mode in (1, 0):
                dx64, _, term, _ = _backward(regime, dy_name, mode, dtype=F64)
                dx32 = _backward(regime, dy_name, mode)[0]
                for v in broke:
                    broke[v] += _breaks(_backward(regime, dy_name, mode, v)[0], dx64, dx32, term)
    # the constant row has xn = 0: dropping xn mgx changes nothing there, every other regime shows it
    assert broke["no_mg"] == 36 and broke["mean_g_short"] == 36 and broke["no_xn_mgx"] == 30, broke


def test_backward_chunking_of_the_cases():
    """one and several chunks, a last chunk shorter than the rest, waves that own no row"""
    seen = set()
    for rows in sorted(set(I.BWD_M + I.BWD_L)):
        cpg, rpc = R.chunking(rows)
        assert cpg * rpc >= rows and rpc <= 16
        last = rows - (cpg - 1) * rpc
        seen |= {"one"} if cpg == 1 else {"several"}
        seen |= {"short_last"} if cpg > 1 and last < rpc else set()
        seen |= {"idle_wave"} if min(last, rpc) < 4 else set()
    assert seen == {"one", "several", "short_last", "idle_wave"}, seen


# ------------------------------------------------------------------------------------------------ column sums
def test_colsum_cases_and_rule():
    sides = {(I.cs_four_chain(G, R, C), R >= 16) for G in I.CS_G for R in I.CS_R for C in I.CS_C}
    sides |= {(I.cs_four_chain(*c), c[1] >= 16) for c in I.CS_WIDE}
    assert sides == {(True, True), (False, False), (False, True)}      # both kernels, the one-thread one below and above R = 16
    assert not I.cs_four_chain(1, 15, 64) and I.cs_four_chain(1, 16, 64) and not I.cs_four_chain(1, 19, 65537)
    Lx, B, Dp = I.CS_POS
    assert I.cs_four_chain(Lx, B, Dp) is False
    assert [I.cs_chunks(*c) for c in I.CS_WS] == [64, 3, 3, 1]
    chunk = (1025 + 63) // 64
    assert chunk == 17 and [k for k in range(64) if k * chunk >= 1025] == [61, 62, 63]   # three empty trailing chunks
    x = I.cs_data((1, 83, 257), "claim").double().abs()
    assert float(x.max() / x[x > 0].min()) > 2.0 ** 30 and (I.cs_data((1, 83, 257), "claim") < 0).any()


def test_colsum_restatement_and_mutants():
    tail = first = rev = 0
    for G in I.CS_G:
        for R_ in I.CS_R:
            for C in I.CS_C:
                x, start = I.cs_case(G, R_, C)
                x = x[:, :, :C]
                for st in (None, start):
                    y64, y32 = R.colsum(x, F64, st), R.colsum(x, F32, st)
                    term = R.colsum_term(x) if st is None else torch.maximum(R.colsum_term(x), st.double().abs())
                    assert _holds(y32, y64, term)["ok"]
                if R_ % 4 and R_ >= 4:
                    tail += R.differing(R.colsum(x, F32, variant="tail_chain3"), R.colsum(x, F32))
    assert tail > 0                                                # the chain the tail rows join shows in the bits
    for G, R_, C in I.CS_WS:
        rs = I.cs_chunks(G, R_, C)
        x = I.cs_case(G, R_, C)[0][:, :, :C]
        y32 = R.colsum_ws(x, rs, F32)
        assert _holds(y32, R.colsum(x, F64), R.colsum_term(x))["ok"]
        if rs > 1:
            first += _breaks(R.colsum_ws(x, rs, F32, variant="first_chunk_only"), R.colsum(x, F64), y32, R.colsum_term(x))
            rev += R.differing(R.colsum_ws(x, rs, F32, variant="chunks_reversed"), y32)
            assert R.differing(R.colsum(x, F32), y32) > 0          # the chunked order is not the plain one
    assert first == 3 and rev > 0
    Lx, B, Dp = I.CS_POS                                           # the position gradient: the interleaved view is a transpose
    dx = I.cs_data((B, Lx, Dp), "pos")
    assert torch.equal(R.colsum(dx.transpose(0, 1), F32), R.colsum(dx.transpose(0, 1).contiguous(), F32))


# ------------------------------------------------------------------------------------------------ GELU2
def test_gelu_grid_and_bound():
    z = I.gelu2_zero()
    assert abs(z + 0.7512) < 1e-4          # (1 + 1.702 z (1 - sigmoid(1.702 z)) = 0)
    x = I.gelu_grid()
    assert x.shape == (1028,) and float(x.min()) == -100 and float(x.max()) == 100
    head = x[:1020].tolist()
    for v in (52.0, -52.0, 53.0, -53.0, I.TINY, 1e-40):
        assert float(torch.tensor(v, dtype=F32)) in head
    assert x[0] == 0 and x[1] == 0 and not torch.signbit(x[0]) and torch.signbit(x[1])
    assert float(x[2]) < z < float(x[3]) and x[3] == torch.nextafter(x[2], torch.tensor(0.0))     # the zero's two fp32 neighbours
    one = torch.ones(4, dtype=F32)
    d64 = R.gelu2(x[:4], one, F64)[0]
    assert float(d64[2]) < 0 < float(d64[3]) and float(d64[0]) == 0.5
    assert math.isinf(float(torch.exp(torch.tensor(1.702 * 53, dtype=F32)))) and math.isfinite(float(torch.exp(torch.tensor(1.702 * 52, dtype=F32))))
    assert 0 < abs(float(x[15])) < I.TINY
    for dy_name in (None,) + tuple(I.DY_SCALES):
        dy = None if dy_name is None else I.gelu_dy(1028, dy_name)
        y64, term = R.gelu2(x, dy, F64)
        y32, _ = R.gelu2(x, dy, F32)
        rep = _holds(y32[None], y64[None], term[None], dim=None, floor_denormal=True)
        assert rep["ok"] and torch.isfinite(y64).all()
        wrong = R.gelu2(x, dy, F32, c=1.7)[0]                      # the mutant: 1.7 for 1.702
        assert _breaks(wrong[None], y64[None], y32[None], term[None], dim=None, floor_denormal=True)
    nf = I.gelu_nonfinite().double()
    want = nf * torch.sigmoid(1.702 * nf)
    assert math.isinf(float(want[0])) and torch.isnan(want[1:3]).all()


# ------------------------------------------------------------------------------------------------ softmax backward
def test_softmax_backward_cases_and_mutants():
    broke = {"no_scale": 0, "sum_over_ld": 0}
    for n in I.SB_N:
        for p_regime in I.SB_P:
            for dp_regime in I.SB_DP:
                P, dP = I.sb_case(p_regime, dp_regime, n)
                assert (P.double().sum(1) - 1).abs().max() < n * 2.0 ** -23
                if p_regime == "one_hot":
                    assert int((P == 1).sum()) == 5 and int((P == 0).sum()) == 5 * (n - 1)
                if p_regime == "spread40" and n >= 63:
                    assert float(P.max(1).values.min()) > 0.8 and float(P.median(1).values.max()) < 1e-5
                y64, term = R.softmax_bwd(P, dP, n, I.SB_SCALE, F64)
                y32, _ = R.softmax_bwd(P, dP, n, I.SB_SCALE, F32)
                assert _holds(y32, y64, term)["ok"]
                if p_regime == "one_hot":
                    assert (y32 == 0).all()                        # the one live column: dP - s = 0 exactly
                Pl = torch.nn.functional.pad(P, (0, 1), value=I.SB_PAD_P)
                dPl = torch.nn.functional.pad(dP, (0, 1), value=I.SB_PAD_DP)
                for v in broke:
                    broke[v] += _breaks(R.softmax_bwd(Pl, dPl, n, I.SB_SCALE, F32, v)[0], y64, y32, term)
    assert broke["sum_over_ld"] >= 40 and broke["no_scale"] >= 30, broke      # (one-hot rows and n = 1: dS = 0 either way)


# ------------------------------------------------------------------------------------------------ ds_embed
def test_embed_cases():
    seen = set()
    for M, L in I.EMB_CASES:
        tok, emb, pos = I.embed_case(M, L)
        assert tok.shape == (M,) and int(tok.max()) < I.EMB_ROWS and emb.shape == (I.EMB_ROWS, D) and pos.shape == (L, D)
        seen |= set(tok.tolist())
        y = R.embed(tok, emb, pos, L)
        assert torch.equal(y[M - 1], emb[max(int(tok[M - 1]), 0)] + pos[(M - 1) % L])
    assert {0, I.EMB_ROWS - 1, -3} <= seen
