"""The small kernels between the contractions of the SpecVQGAN codec and the MelGAN vocoder (csrc/misc.hip, csrc/norm.hip)
against float64 at their edges, each through its raw C entry: ds_vq_argmin, ds_groupnorm_stats / ds_groupnorm_finish and the
statistics ds_conv3x3_c1 hands them, ds_softmax_rows, ds_stencil9, ds_stencil7_tanh, ds_mel_to_cl, ds_codebook_gather.

Inputs: tests/glue_inputs.py; float64 and float32 restatements: tests/glue_reference.py; tests/test_glue_host.py checks on the
CPU that the inputs are what they claim and that the references hold the bounds (and a wrong kernel does not).

Bounds.  A fixed-order fp32 chain without a multiply (ds_stencil9, the layout of ds_mel_to_cl, ds_codebook_gather, ds_vq_argmin
on exactly representable distances) must be met bit for bit.  GroupNorm's scale / shift: 2^-22 relative (sums in double, one
rounding to fp32, the factor 4).  Everything else, on every element:  |kernel - f64| <= 4 * max(d32, 1 ulp of fp32 at the f64
value), d32 = the float32 restatement's own distance from float64 on the case (per row for the softmax).

Every output buffer is pre-filled with NaN (a sentinel where NaN is a legitimate output, and for integers) and carries a guard
region behind it that must come back untouched.  The non-finite rows of ds_vq_argmin go through the raw entry ONLY: its addresses
depend on row, lane and k, never on a value, and its output is read back on the host -- no consumer ever indexes with it.

Measured on an MI355X: every test's docstring carries its own figures."""
import pytest
import torch

import glue_inputs as I
import glue_reference as R
from conftest import parity_line

pytestmark = pytest.mark.gpu
NO_GRAD = True          # tests/conftest.py: every test of this module runs under torch.no_grad()
F64, F32 = torch.float64, torch.float32
GUARD = 64              # elements behind every output
SENT_F, SENT_I = -12345.0, -7


@pytest.fixture(scope="module")
def L():
    from text_to_sound_synthesis_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _lib.lib()
    return _lib


def _out(n, fill=float("nan"), dtype=F32):
    return torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")


def _untouched(buf, n, fill=float("nan")):
    g = buf[n:].cpu()
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


def _refused(L, rc, entry):
    return rc != 0 and entry in L.lib().ds_last_error_string().decode()


# ------------------------------------------------------------------------------------------------ 1. ds_vq_argmin
def _vq(L, z, ze, ee, with_dmin):
    M, K = ze.shape
    idx = _out(M, SENT_I, torch.int64)
    dmin = _out(M, SENT_F) if with_dmin else None         # NaN is a legitimate winning distance: a finite sentinel here
    zc, zec, eec = z.cuda(), ze.cuda(), ee.cuda()
    L.check(L.lib().ds_vq_argmin(L.ptr(zc), L.ptr(zec), L.ptr(eec), L.ptr(idx), L.ptr(dmin), M, z.shape[1], K, L.stream()))
    assert _untouched(idx, M, SENT_I) and (dmin is None or _untouched(dmin, M, SENT_F))
    return idx[:M].cpu(), None if dmin is None else dmin[:M].cpu()


@pytest.mark.parametrize("K", I.VQ_K)
def test_vq_argmin_equals_torch_argmin(L, K):
    """C = 1, 64, 100, 256 x M = 1 .. 5, 795 at every K: the unique minimum at 0, K - 1 and every lane of the first and last pass;
    the same minimum at k, k + 1, k + 64, k + 65; an all-equal row; one NaN, NaN at K - 1 only, all NaN, all +inf, -inf, NaN
    beside -inf, NaN in z; dmin given and NULL -- torch.equal with torch.argmin of the same fp32 row, dmin bit for bit.  Then
    z = 0 with arbitrary fp32 ee, ze (one rounding per distance).  Before the fix the all-NaN, all-+inf and NaN-in-z rows
    returned 2 147 483 647 (no d < best ever held) and a NaN among finite values was passed over.
    Measured: 0 of 7 290 rows differ at every K (3 240 with dmin, 3 240 without, 810 rounded), every dmin bit-equal."""
    rows = 0
    for C in I.VQ_C:
        for M in I.VQ_M:
            z, ze, ee, names = I.vq_case(K, C, M)
            want, want_d, _ = R.vq_argmin(z, ze, ee)
            for with_dmin in (True, False):
                idx, dmin = _vq(L, z, ze, ee, with_dmin)
                assert int(idx.min()) >= 0 and int(idx.max()) < K, "index outside [0, K)"
                bad = (idx != want).nonzero().view(-1).tolist()
                assert not bad, "K %d C %d M %d: rows %s differ" % (K, C, M, [(r, names[r], int(idx[r]), int(want[r])) for r in bad[:8]])
                assert dmin is None or R.same_floats(dmin, want_d)
                rows += M
    for M in I.VQ_M:
        z, ze, ee = I.vq_rounded_case(K, M)
        want, want_d, _ = R.vq_argmin(z, ze, ee)
        idx, dmin = _vq(L, z, ze, ee, True)
        assert torch.equal(idx, want) and R.same_floats(dmin, want_d)
        rows += M
    parity_line("ds_vq_argmin K %d: %d rows (finite, tied, NaN, +-inf), 0 differ from torch.argmin" % (K, rows))


# ------------------------------------------------------------------------------------------------ 2. GroupNorm statistics
def _gn_stats(L, x, groups, gamma, beta):
    B, P, C = x.shape
    work = _out(B * ((P + 255) // 256) * 2 * C, dtype=F64)
    sc, sh = _out(B * C), _out(B * C)
    xc, gc, bc = x.cuda(), gamma.cuda(), beta.cuda()
    L.check(L.lib().ds_groupnorm_stats(L.ptr(xc), B, P, C, groups, L.ptr(gc), L.ptr(bc), I.GN_EPS, L.ptr(work), L.ptr(sc),
                                       L.ptr(sh), L.stream()))
    assert _untouched(work, work.numel() - GUARD) and _untouched(sc, B * C) and _untouched(sh, B * C)
    return sc[:B * C].cpu().view(B, C), sh[:B * C].cpu().view(B, C)


@pytest.mark.parametrize("shape", I.GN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_stats_vs_two_pass_float64(L, shape):
    """scale and shift themselves (not the normalised tensor) against a two-pass float64 group_norm, 2^-22 relative; zero-mean
    data, channel means of 1e2 and 1e4 standard deviations, a constant group (rstd = 1 / sqrt(eps)), a group of +-6e4, a
    group of 1e-6; a second run is bit-equal.
    Measured, error / bound over the 6 kinds: 0.23 .. 0.25 in every shape (the one fp32 rounding is 0.25).  With plain sums
    (before the kernel summed x - pivot) means of 1e4 standard deviations were at 1.74 in 1 x 300 x 1024, 0.86 in 1 x 265 x 512
    and 0.25 .. 0.43 elsewhere: the fewer pixel lanes a channel has, the longer a thread's chain of double adds."""
    worst = 0.0
    for kind in I.GN_DATA:
        x, gamma, beta = I.gn_case(shape, kind)
        sc, sh = _gn_stats(L, x, shape[3], gamma, beta)
        rep = R.groupnorm_report(sc, sh, R.groupnorm_affine(x, shape[3], gamma, beta, I.GN_EPS), beta)
        print("ds_groupnorm_stats %s %s: scale %.3f shift %.3f of the bound" % (shape, kind, rep["scale"], rep["shift"]))
        assert rep["ok"], (kind, rep)
        sc2, sh2 = _gn_stats(L, x, shape[3], gamma, beta)
        assert torch.equal(sc, sc2) and torch.equal(sh, sh2)
        worst = max(worst, rep["worst"])
    parity_line("ds_groupnorm_stats %s, 6 kinds of data: worst error %.3f of 2^-22 relative" % ("x".join(map(str, shape)), worst))


def _gn_finish(L, part, P, C, groups, gamma, beta):
    B, nchunk = part.shape[:2]
    sc, sh = _out(B * C), _out(B * C)
    pc, gc, bc = part.cuda(), gamma.cuda(), beta.cuda()
    L.check(L.lib().ds_groupnorm_finish(L.ptr(pc), B, nchunk, P, C, groups, L.ptr(gc), L.ptr(bc), I.GN_EPS, L.ptr(sc), L.ptr(sh),
                                        L.stream()))
    assert _untouched(sc, B * C) and _untouched(sh, B * C)
    return sc[:B * C].cpu().view(B, C), sh[:B * C].cpu().view(B, C)


@pytest.mark.parametrize("nchunk", I.GN_FINISH_CHUNKS)
def test_groupnorm_finish_on_exact_partials(L, nchunk):
    """Hand-built partial sums with integer values (exact in double in any order), C 128 / 32 groups and C 64 / 64 groups;
    nchunk * C / groups runs past the 256 threads from nchunk = 83 on.  Within 1 fp32 ulp of the float64 formula, and
    identical under a permutation of the chunks.  Measured: at most 0.5 ulp (the one rounding), all permutations bit-equal."""
    worst = 0.0
    for C, groups in ((128, 32), (64, 64)):
        part, P, gamma, beta = I.gn_finish_case(nchunk, C, groups)
        sc, sh = _gn_finish(L, part, P, C, groups, gamma, beta)
        rs, rh, _ = R.groupnorm_affine_from_sums(part[:, :, 0].sum(1), part[:, :, 1].sum(1), P * C // groups, groups, gamma, beta,
                                                 I.GN_EPS)
        es, eh = (sc.double() - rs).abs() / R.ulp32(rs), (sh.double() - rh).abs() / R.ulp32(rh)
        worst = max(worst, float(es.max()), float(eh.max()))
        assert float(es.max()) <= 1.0 and float(eh.max()) <= 1.0, (float(es.max()), float(eh.max()))
        perm = torch.randperm(nchunk, generator=torch.Generator().manual_seed(nchunk))
        sc2, sh2 = _gn_finish(L, part[:, perm].contiguous(), P, C, groups, gamma, beta)
        assert torch.equal(sc, sc2) and torch.equal(sh, sh2)
    parity_line("ds_groupnorm_finish nchunk %d, integer partial sums: %.2f ulp from float64, chunk order irrelevant" % (nchunk, worst))


@pytest.mark.parametrize("mel", I.CHAIN_MELS)
@pytest.mark.parametrize("shape", I.CHAIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_in_statistics_through_groupnorm(L, shape, mel):
    """ds_conv3x3_c1's per-row sums -> ds_groupnorm_finish, against ds_groupnorm_stats on the stored conv output and against
    the two-pass float64 GroupNorm of that output: scale / shift within 2^-22 relative of both.
    Measured, error / bound (80 x 848 x 128 | 2 x 16 x 33 x 64): with the kernel's sums in fp32 (as it was first written)
    uniform 0.24 | 0.24, silent 26.7 | 0.79, silent past column 300 12.0 | 0.25; with the sums in double 0.22 .. 0.24 in all six,
    and scale / shift bit-equal to ds_groupnorm_stats' on the stored output."""
    B, H, W, C = shape
    x, w, bias, gamma, beta = I.chain_case(shape, mel)
    nch = L.lib().ds_conv3x3_c1_chunks(H, W)
    out, part = _out(B * H * W * C), _out(B * nch * 2 * C, dtype=F64)
    xc, wc, bc = x.cuda(), w.cuda(), bias.cuda()
    L.check(L.lib().ds_conv3x3_c1(L.ptr(xc), L.ptr(wc), L.ptr(bc), L.ptr(out), B, H, W, C, L.ptr(part), L.stream()))
    assert _untouched(out, B * H * W * C) and _untouched(part, B * nch * 2 * C)
    y = out[:B * H * W * C].cpu().view(B, H * W, C)
    assert torch.isfinite(y).all()
    sc, sh = _gn_finish(L, part[:B * nch * 2 * C].cpu().view(B, nch, 2, C), H * W, C, 32, gamma, beta)
    ref = R.groupnorm_affine(y, 32, gamma, beta, I.GN_EPS)
    rep = R.groupnorm_report(sc, sh, ref, beta)
    sc_s, sh_s = _gn_stats(L, y, 32, gamma, beta)
    rep_s = R.groupnorm_report(sc_s, sh_s, ref, beta)
    rep_cs = R.groupnorm_report(sc, sh, (sc_s.double(), sh_s.double(), ref[2]), beta)
    line = ("ds_conv3x3_c1 -> ds_groupnorm_finish %s %s: %.3f of 2^-22 relative from float64, %.3f from ds_groupnorm_stats "
            "(itself %.3f from float64)" % ("x".join(map(str, shape)), mel, rep["worst"], rep_cs["worst"], rep_s["worst"]))
    print(line)
    parity_line(line)
    assert rep_s["ok"], rep_s
    assert rep["ok"], rep
    assert rep_cs["ok"], rep_cs


# ------------------------------------------------------------------------------------------------ 3. ds_softmax_rows
@pytest.mark.parametrize("n", I.SM_N)
def test_softmax_rows(L, n):
    """ld = n and n rounded up to 32; rows 1, 2, 3, 5, 530; scale 0.044, 1, -1, 0; flat, unit, sharp (a one-hot at scale 1),
    +-30 spread, rows with -inf entries.  Every element within 4 max(d32 of its row, 1 ulp) of float64, padding columns
    exactly 0, -inf entries and the sharp rows' losers exactly 0, row sums within n 2^-23 of 1.
    Measured: worst error / bound 0.66 .. 0.76 for n >= 2 (n = 1: exact), row sums within 0.38 n 2^-23 (n = 2) .. 0.001 n 2^-23
    (n = 1000)."""
    worst, worst_sum = 0.0, 0.0
    for regime, scales in I.SM_REGIMES.items():
        x = I.sm_case(regime, n)
        for scale in scales:
            y64, y32 = R.softmax_rows(x, scale, F64), R.softmax_rows(x, scale, F32)
            for ld in I.sm_ld(n):
                for rows in I.SM_ROWS:
                    buf = _out(rows * ld)
                    v = buf[:rows * ld].view(rows, ld)
                    v[:] = 777.0                                              # what the padding columns hold before
                    v[:, :n] = x[:rows].cuda()
                    L.check(L.lib().ds_softmax_rows(L.ptr(buf), rows, n, ld, scale, L.stream()))
                    assert _untouched(buf, rows * ld)
                    got = v.cpu()
                    k = got[:, :n]
                    assert (got[:, n:] == 0).all(), "padding columns"
                    rep = R.bound_report(k, y64[:rows], y32[:rows], dim=1)
                    assert rep["ok"], (regime, scale, ld, rows, rep)
                    dev = float((k.double().sum(1) - 1).abs().max()) / (n * 2.0 ** -23)
                    assert dev <= 1.0, (regime, scale, ld, rows, dev)
                    if regime == "neg_inf":
                        assert (k[torch.isinf(x[:rows])] == 0).all()
                    if regime == "sharp":
                        assert torch.equal(k, y64[:rows].float()) and int((k == 1).sum()) == rows and int((k == 0).sum()) == rows * (n - 1)
                    worst, worst_sum = max(worst, rep["worst"]), max(worst_sum, dev)
    parity_line("ds_softmax_rows n %d: worst error %.3f of 4 max(d32, ulp); row sums within %.3f n 2^-23 of 1" % (n, worst, worst_sum))


# ------------------------------------------------------------------------------------------------ 4. stencils and layout
@pytest.mark.parametrize("shape", I.S9_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stencil9(L, shape):
    """ldt 9 and 16, taps at scale 1 and 1e4: bit-equal to the fp32 chain bias + taps in (ky, kx) order, and within the bound of
    float64.  Measured: bit-equal in all 20 cases; error / bound at most 0.25."""
    B, H, W = shape
    worst = 0.0
    for ldt in I.S9_LDT:
        for scale in I.S9_SCALES:
            taps, bias = I.s9_case(shape, ldt, scale)
            out = _out(B * H * W)
            tc = taps.cuda()
            L.check(L.lib().ds_stencil9(L.ptr(tc), ldt, bias, L.ptr(out), B, H, W, L.stream()))
            assert _untouched(out, B * H * W)
            k = out[:B * H * W].cpu().view(B, H, W)
            y32, y64 = R.stencil9(taps, bias, F32), R.stencil9(taps, bias, F64)
            assert torch.equal(k, y32), (ldt, scale, float((k - y32).abs().max()))
            rep = R.bound_report(k, y64, y32)
            assert rep["ok"], rep
            worst = max(worst, rep["worst"])
    parity_line("ds_stencil9 %s: bit-equal to the fp32 chain; %.3f of 4 max(d32, ulp) from float64" % ("x".join(map(str, shape)), worst))


@pytest.mark.parametrize("N", I.S7_N)
def test_stencil7_tanh(L, N):
    """B 1 and 3, ldt 7 and 8, pre-activations to +-20: within the bound of float64, and the first and last three outputs of
    every clip (the reflecting ones) within the bound taken on them alone.
    Measured: error / bound 0.25 (one ulp at a saturated output) at every N but 7, where it is 0.39, on the whole clips and on
    the reflecting outputs alike."""
    worst, worst_edge = 0.0, 0.0
    edge = torch.tensor(sorted(set([0, 1, 2, N - 3, N - 2, N - 1])))
    for B in I.S7_B:
        for ldt in I.S7_LDT:
            taps, bias = I.s7_case(B, N, ldt)
            out = _out(B * N)
            tc = taps.cuda()
            L.check(L.lib().ds_stencil7_tanh(L.ptr(tc), ldt, bias, L.ptr(out), B, N, L.stream()))
            assert _untouched(out, B * N)
            k = out[:B * N].cpu().view(B, N)
            y64, y32 = R.stencil7_tanh(taps, bias, F64), R.stencil7_tanh(taps, bias, F32)
            rep, rep_e = R.bound_report(k, y64, y32), R.bound_report(k[:, edge], y64[:, edge], y32[:, edge])
            assert rep["ok"], rep
            assert rep_e["ok"], rep_e
            worst, worst_edge = max(worst, rep["worst"]), max(worst_edge, rep_e["worst"])
    parity_line("ds_stencil7_tanh N %d: %.3f of 4 max(d32, ulp) from float64; reflecting outputs alone %.3f" % (N, worst, worst_edge))


def test_stencil7_tanh_refuses_short_clips(L):
    """N < 4: ReflectionPad1d(3) needs more than one bounce (N = 1, 2, 3: 6, 4, 1 taps outside [0, N) with the kernel's one) --
    the entry returns an error and the output buffer is untouched."""
    taps = torch.zeros(3, 4, 8).cuda()
    for N in (3, 2, 1, 0, -1):
        out = _out(16)
        rc = L.lib().ds_stencil7_tanh(L.ptr(taps), 8, 0.0, L.ptr(out), 3, N, L.stream())
        assert _refused(L, rc, "ds_stencil7_tanh"), N
        with pytest.raises(L.DiffsoundHipError):
            L.check(rc)
        torch.cuda.synchronize()
        assert _untouched(out, 0)
    out = _out(12)
    L.check(L.lib().ds_stencil7_tanh(L.ptr(taps), 8, 0.0, L.ptr(out), 3, 4, L.stream()))
    assert (out[:12].cpu() == 0).all() and _untouched(out, 12)


@pytest.mark.parametrize("shape", I.MEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mel_to_cl(L, shape):
    """a = 1, b = 0: torch.equal with the permuted input plus zero padding; (0.5, 0.5) and (2, -1): within 1 ulp of |a x| + |b|,
    padding exactly 0.  Measured: at most 0.5 ulp."""
    B, C, T, Cpad = shape
    mel = I.mel_case(shape)
    mc = mel.cuda()
    worst = 0.0
    for a, b in I.MEL_AB:
        out = _out(B * T * Cpad)
        L.check(L.lib().ds_mel_to_cl(L.ptr(mc), L.ptr(out), B, C, T, Cpad, a, b, L.stream()))
        assert _untouched(out, B * T * Cpad)
        k = out[:B * T * Cpad].cpu().view(B, T, Cpad)
        y64, mag = R.mel_to_cl(mel, Cpad, a, b, F64)
        assert (k[..., C:] == 0).all()
        if (a, b) == (1.0, 0.0):
            assert torch.equal(k, y64.float())
        err = (k.double() - y64).abs()[..., :C] / R.ulp32(mag[..., :C])
        assert float(err.max()) <= 1.0, float(err.max())
        worst = max(worst, float(err.max()))
    parity_line("ds_mel_to_cl %s: identity exact; affine forms within %.2f ulp of |a x| + |b|" % ("x".join(map(str, shape)), worst))


@pytest.mark.parametrize("shape", I.CB_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_codebook_gather(L, shape):
    """torch.equal with the gather in ColumnMajor order; tokens -1 and K (a leftover [MASK]) read rows 0 and K - 1: the clamp
    precedes the address computation."""
    B, H, W, C, K = shape
    tok, E = I.cb_case(shape)
    out = _out(B * H * W * C)
    tc, ec = tok.cuda(), E.cuda()
    L.check(L.lib().ds_codebook_gather(L.ptr(tc), L.ptr(ec), L.ptr(out), B, H, W, C, K, L.stream()))
    assert _untouched(out, B * H * W * C)
    assert torch.equal(out[:B * H * W * C].cpu().view(B, H, W, C), R.codebook_gather(tok, E, H, W))


# ------------------------------------------------------------------------------------------------ 5. arguments
def test_argument_errors_launch_nothing(L):
    """Null pointers and sizes <= 0: a non-zero return, ds_last_error_string names the entry, no output is written."""
    lib, p, st = L.lib(), L.ptr, L.stream()
    f = lambda n, fill=SENT_F, dtype=F32: torch.full((n,), fill, dtype=dtype, device="cuda")
    src, src64, tok = f(4096, 0.5), f(4096, 0.5, F64), torch.zeros(64, dtype=torch.int64, device="cuda")
    o1, o2, oi, od = f(4096), f(4096), f(64, SENT_I, torch.int64), f(4096, SENT_F, F64)
    entries = {
        "ds_vq_argmin": (dict(z=p(src), ze=p(src), ee=p(src), idx=p(oi), dmin=p(o1), M=4, C=8, K=16),
                         lambda a: lib.ds_vq_argmin(a["z"], a["ze"], a["ee"], a["idx"], a["dmin"], a["M"], a["C"], a["K"], st),
                         [dict(z=None), dict(ze=None), dict(ee=None), dict(idx=None), dict(M=0), dict(C=0), dict(K=0), dict(M=-1), dict(K=-1)]),
        "ds_groupnorm_stats": (dict(x=p(src), B=2, P=8, C=8, g=2, ga=p(src), be=p(src), w=p(od), sc=p(o1), sh=p(o2)),
                               lambda a: lib.ds_groupnorm_stats(a["x"], a["B"], a["P"], a["C"], a["g"], a["ga"], a["be"], 1e-6, a["w"], a["sc"],
                                                                a["sh"], st),
                               [dict(x=None), dict(ga=None), dict(be=None), dict(w=None), dict(sc=None), dict(sh=None), dict(B=0), dict(B=-1),
                                dict(P=0), dict(P=-1), dict(C=0), dict(g=0), dict(C=-8)]),
        "ds_groupnorm_finish": (dict(part=p(src64), B=2, n=2, P=8, C=8, g=2, ga=p(src), be=p(src), sc=p(o1), sh=p(o2)),
                                lambda a: lib.ds_groupnorm_finish(a["part"], a["B"], a["n"], a["P"], a["C"], a["g"], a["ga"], a["be"], 1e-6,
                                                                  a["sc"], a["sh"], st),
                                [dict(part=None), dict(ga=None), dict(be=None), dict(sc=None), dict(sh=None), dict(B=0), dict(n=0), dict(P=0),
                                 dict(C=0), dict(g=0), dict(n=-1)]),
        "ds_softmax_rows": (dict(x=p(o1), rows=4, n=8, ld=8), lambda a: lib.ds_softmax_rows(a["x"], a["rows"], a["n"], a["ld"], 1.0, st),
                            [dict(x=None), dict(rows=0), dict(n=0), dict(rows=-1), dict(n=-1), dict(ld=7)]),
        "ds_stencil9": (dict(t=p(src), ldt=9, out=p(o1), B=2, H=3, W=4),
                        lambda a: lib.ds_stencil9(a["t"], a["ldt"], 0.0, a["out"], a["B"], a["H"], a["W"], st),
                        [dict(t=None), dict(out=None), dict(ldt=8), dict(B=0), dict(H=0), dict(W=0), dict(B=-1), dict(H=-1), dict(W=-1)]),
        "ds_stencil7_tanh": (dict(t=p(src), ldt=7, out=p(o1), B=2, N=8),
                             lambda a: lib.ds_stencil7_tanh(a["t"], a["ldt"], 0.0, a["out"], a["B"], a["N"], st),
                             [dict(t=None), dict(out=None), dict(ldt=6), dict(B=0), dict(B=-1), dict(N=0), dict(N=3), dict(N=-4)]),
        "ds_mel_to_cl": (dict(mel=p(src), out=p(o1), B=2, C=3, T=4, Cp=8),
                         lambda a: lib.ds_mel_to_cl(a["mel"], a["out"], a["B"], a["C"], a["T"], a["Cp"], 1.0, 0.0, st),
                         [dict(mel=None), dict(out=None), dict(B=0), dict(C=0), dict(T=0), dict(Cp=2), dict(B=-1), dict(T=-1), dict(C=-1, Cp=0)]),
        "ds_codebook_gather": (dict(tok=p(tok), E=p(src), out=p(o1), B=2, H=2, W=3, C=8, K=16),
                               lambda a: lib.ds_codebook_gather(a["tok"], a["E"], a["out"], a["B"], a["H"], a["W"], a["C"], a["K"], st),
                               [dict(tok=None), dict(E=None), dict(out=None), dict(B=0), dict(H=0), dict(W=0), dict(C=0), dict(K=0),
                                dict(B=-1), dict(C=6)]),
    }
    for name, (ok, call, bads) in entries.items():
        for bad in bads:
            rc = call(dict(ok, **bad))
            assert _refused(L, rc, name), (name, bad, rc, lib.ds_last_error_string())
            with pytest.raises(L.DiffsoundHipError):
                L.check(rc)
    torch.cuda.synchronize()
    for o, fill in ((o1, SENT_F), (o2, SENT_F), (oi, SENT_I), (od, SENT_F)):
        assert bool((o.cpu() == fill).all()), "a refused call wrote to an output"
    for name, (ok, call, _) in entries.items():                               # the table's own calls are valid ones
        assert call(ok) == 0, (name, lib.ds_last_error_string())
    torch.cuda.synchronize()
