"""The conditions that keep tests/test_hip_codec_glue.py honest, checked on the CPU alone (tests/glue_inputs.py,
tests/glue_reference.py): the inputs are what their names say, the references are the operations they restate, the bounds are
met by a correct evaluation at the kernel's precision and missed by the mistakes they are there to catch -- the first version of
ds_vq_argmin's lane loop (emulated here from its source) on all-NaN / all-+inf rows, a one-bounce reflection at N <= 3, fp32
accumulators under the GroupNorm statistics of a silent mel, a stencil that adds its taps in another order."""
import pytest
import torch
import torch.nn.functional as F

import glue_inputs as I
import glue_reference as R

F64, F32 = torch.float64, torch.float32
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------ ds_vq_argmin
def test_torch_argmin_semantics_the_kernel_must_have():
    rows = torch.tensor([[3, NAN, 1, NAN], [INF] * 4, [NAN] * 4, [2, -INF, -INF, 0]])
    assert torch.argmin(rows, dim=1).tolist() == [1, 0, 0, 1]


def _ahead_first_version(a, ia, b, ib, in_lane):
    return a < b if in_lane else (a < b or (a == b and ia < ib))


def _ahead(a, ia, b, ib, in_lane):
    na, nb = a != a, b != b
    if na or nb:
        return na and (not nb or ia < ib)
    return a < b or (a == b and ia < ib)


def _lane_argmin(d, ahead):
    """the kernel's search: 64 lanes walk k = lane, lane + 64, ... from (+inf, 0x7fffffff), then a butterfly over the lanes"""
    K = len(d)
    best, bi = [INF] * 64, [0x7fffffff] * 64
    for lane in range(64):
        for k in range(lane, K, 64):
            if ahead(d[k], k, best[lane], bi[lane], True):
                best[lane], bi[lane] = d[k], k
    o = 32
    while o:
        nb, ni = list(best), list(bi)
        for lane in range(64):
            if ahead(best[lane ^ o], bi[lane ^ o], best[lane], bi[lane], False):
                nb[lane], ni[lane] = best[lane ^ o], bi[lane ^ o]
        best, bi, o = nb, ni, o >> 1
    return bi[0]


@pytest.mark.parametrize("K", [1, 65, 256])
def test_vq_patterns_separate_the_first_version_from_the_fix(K):
    """On every pattern the new order equals torch.argmin; the first version's equals it on the finite rows (bit-identical
    tokens) and on the rows with -inf, passes over a NaN among finite values, and leaves the sentinel on rows that are all NaN
    or all +inf (the two the issue names; NaN in z makes the row all NaN)."""
    pats = I.vq_patterns(K)
    assert set(I.VQ_NONFINITE) <= {n for n, _, _ in pats}
    for name, d, nan_in_z in pats:
        row = torch.full((K,), NAN) if nan_in_z else d
        want = int(torch.argmin(row))
        assert _lane_argmin(row.tolist(), _ahead) == want, name
        old = _lane_argmin(row.tolist(), _ahead_first_version)
        if name in ("all_nan", "all_inf", "nan_in_z"):
            assert old == 0x7fffffff, name
        elif torch.isnan(row).any():
            assert old != want or K == 1, name
        else:
            assert old == want, name


@pytest.mark.parametrize("K", I.VQ_K)
def test_vq_cases_dictate_exact_distances(K):
    pats = I.vq_patterns(K)
    where = {int(n[4:]) for n, _, _ in pats if n.startswith("min@")}
    assert {0, K - 1} | set(range(min(64, K))) | set(range(64 * ((K - 1) // 64), K)) <= where
    for n, d, _ in pats:
        if n.startswith("tie@"):
            k0 = int(n[4:])
            assert all(float(d[j]) == 1.0 for j in (k0, k0 + 1, k0 + 64, k0 + 65) if j < K) and int(torch.argmin(d)) == k0
    for C in I.VQ_C:
        for M in I.VQ_M:
            z, ze, ee, names = I.vq_case(K, C, M)
            assert z.shape == (M, C) and ze.shape == (M, K) and len(names) == M
            if M == 5:
                assert set(names) <= set(I.VQ_NONFINITE), (K, C, M)     # five of the non-finite rows in one short call
            if M > 5:
                assert {n for n, _, _ in pats} == set(names), (K, C, M)    # every pattern
            assert torch.isfinite(ze[[i for i, n in enumerate(names) if n == "nan_in_z"]]).all()
            d32 = R.vq_distances(z, ze, ee)
            d64 = R.vq_distances(z.double(), ze.double(), ee.double())
            assert R.same_floats(d32.double(), d64)                    # exact: nothing was rounded, in any order
            fin = torch.isfinite(d32)
            assert torch.equal(d32[fin], d32[fin].round())
            idx, dm, _ = R.vq_argmin(z, ze, ee)
            for r, n in enumerate(names):
                if n in ("all_nan", "all_inf", "nan_in_z"):
                    assert int(idx[r]) == 0
                if n.startswith("min@"):
                    assert int(idx[r]) == int(n[4:]) and float(dm[r]) == 1.0 + float((z[r] ** 2).sum()) * 0
    z, ze, ee = I.vq_rounded_case(K, 5)
    assert (z == 0).all() and torch.equal(2 * ze / 2, ze)
    one = (ee.double()[None] - 2 * ze.double()).float()                 # ONE rounding of the exact value
    assert torch.equal(R.vq_distances(z, ze, ee), one)
    assert torch.equal(torch.addcmul(ee[None].expand_as(ze), ze, torch.tensor(-2.0)), one)        # and contraction changes nothing


# ------------------------------------------------------------------------------------------------ stencil7's reflection
def test_one_bounce_reflection_leaves_the_clip_only_below_four():
    assert [R.one_bounce_out_of_range(N) for N in (1, 2, 3)] == [6, 4, 1]
    for N in I.S7_N:
        assert N >= 4 and R.one_bounce_out_of_range(N) == 0
        t = torch.arange(N)
        for k in range(7):                                              # the reference's map is ReflectionPad1d's
            pad = F.pad(t.double()[None, None], (3, 3), mode="reflect")[0, 0].long()
            assert torch.equal(R.reflect(t + k - 3, N), pad[k:k + N])


@pytest.mark.parametrize("N", I.S7_N)
def test_stencil7_cases_and_chain(N):
    eye = torch.zeros(1, 7, 7, dtype=F64)
    for k in range(7):
        eye[0, k, k] = 1.0
    for B in I.S7_B:
        for ldt in I.S7_LDT:
            taps, bias = I.s7_case(B, N, ldt)
            pre = R.stencil7_pre(taps, bias, F64)
            conv = F.conv1d(F.pad(taps[..., :7].double().permute(0, 2, 1), (3, 3), mode="reflect"), eye)[:, 0] + float(torch.tensor(bias))
            assert (pre - conv).abs().max() < 1e-12
            assert float(pre.min()) < -20                               # on output 1, which reflects
            if N >= 255:                                                # (below, the two planted outputs share taps)
                assert float(pre.max()) > 20 and float(pre.abs().min()) < 0.1             # and tanh's linear range
            y64, y32 = R.stencil7_tanh(taps, bias, F64), R.stencil7_tanh(taps, bias, F32)
            assert R.bound_report(y32, y64, y32)["ok"]
            wrong = torch.tanh(pre - taps[:, :, 0].double() + taps[:, R.reflect(torch.arange(N) - 2, N), 0].double())   # tap 0 one off
            assert not R.bound_report(wrong, y64, y32)["ok"]


# ------------------------------------------------------------------------------------------------ GroupNorm
@pytest.mark.parametrize("shape", I.GN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_cases_and_bound(shape):
    """The kernel's formula (E[x^2] - mean^2 in double, one rounding to fp32) holds the 2^-22 bound on every case with room to
    spare; fp32 sums do not at a mean of 1e4 standard deviations."""
    B, P, C, groups = shape
    cpg = C // groups
    for kind in I.GN_DATA:
        x, gamma, beta = I.gn_case(shape, kind)
        assert x.shape == (B, P, C) and float(gamma.min()) >= 0.2
        xg = x.double().view(B, P, groups, cpg)
        mean, std = xg.mean((1, 3)), xg.var((1, 3), unbiased=False).sqrt()
        g0 = groups // 2
        if kind in ("mean_1e2", "mean_1e4") and P * cpg >= 40:
            Rr = 1e2 if kind == "mean_1e2" else 1e4
            ratio = mean.abs() / std
            assert float(ratio.min()) > Rr / 4 and float(ratio.max()) < 4 * Rr, (float(ratio.min()), float(ratio.max()))
        if kind == "constant":
            assert float(std[:, g0].max()) == 0.0
        if kind == "big":
            assert float(xg[:, :, g0].abs().max()) > (5e4 if P * cpg >= 40 else 0) and float(xg.abs().max()) <= 6e4
        if kind == "tiny" and P * cpg >= 40:
            assert 1e-7 < float(std[:, g0].min()) and float(std[:, g0].max()) < 1e-5
        ref = R.groupnorm_affine(x, groups, gamma, beta, I.GN_EPS)
        if kind == "constant":                                           # rstd = 1 / sqrt(eps) on the constant group
            want = gamma.double()[g0 * cpg:(g0 + 1) * cpg] / float(torch.tensor(I.GN_EPS, dtype=F32)) ** 0.5
            assert torch.allclose(ref[0][0, g0 * cpg:(g0 + 1) * cpg], want, rtol=1e-12, atol=0)
        s, q = x.double().sum(1), x.double().pow(2).sum(1)
        ks, kh, _ = R.groupnorm_affine_from_sums(s, q, P * cpg, groups, gamma, beta, I.GN_EPS)
        rep = R.groupnorm_report(ks.float(), kh.float(), ref, beta)
        assert rep["worst"] <= 0.5, (kind, rep)                          # one fp32 rounding is 0.25 of the bound
        if P * cpg > 1:                                                  # (torch refuses a group of one value)
            normed = F.group_norm(x.double().permute(0, 2, 1), groups, gamma.double(), beta.double(),
                                  eps=float(torch.tensor(I.GN_EPS, dtype=F32))).permute(0, 2, 1)
            mine = x.double() * ref[0][:, None] + ref[1][:, None]
            assert float((mine - normed).abs().max()) <= 1e-9 * max(1.0, float(normed.abs().max()))
        if kind == "mean_1e4" and P * cpg >= 255:
            s32, q32 = x.sum(1).double(), x.pow(2).sum(1).double()
            bad = R.groupnorm_affine_from_sums(s32, q32, P * cpg, groups, gamma, beta, I.GN_EPS)
            assert not R.groupnorm_report(bad[0].float(), bad[1].float(), ref, beta)["ok"]


@pytest.mark.parametrize("nchunk", I.GN_FINISH_CHUNKS)
def test_groupnorm_finish_partials_are_exact(nchunk):
    for C, groups in ((128, 32), (64, 64)):
        part, P, gamma, beta = I.gn_finish_case(nchunk, C, groups)
        assert part.shape == (2, nchunk, 2, C) and part.dtype == F64 and P == 3 * nchunk
        assert torch.equal(part, part.round()) and float(part.abs().sum()) < 2.0 ** 52
        assert (nchunk * (C // groups) > 256) == (nchunk >= 83 and C // groups == 4 or nchunk * (C // groups) > 256)
        s, q = part[:, :, 0].sum(1), part[:, :, 1].sum(1)
        perm = torch.randperm(nchunk, generator=torch.Generator().manual_seed(nchunk))
        assert torch.equal(s, part[:, perm, 0].sum(1)) and torch.equal(q, part[:, perm, 1].sum(1))
        rs, rh, _ = R.groupnorm_affine_from_sums(s, q, P * C // groups, groups, gamma, beta, I.GN_EPS)
        assert torch.isfinite(rs).all() and torch.isfinite(rh).all()
        # rounding the float64 value to fp32 is within half an ulp: "within 1 ulp" leaves the kernel its one rounding
        assert float(((rs.float().double() - rs).abs() / R.ulp32(rs)).max()) <= 0.5


@pytest.mark.parametrize("mel", I.CHAIN_MELS)
@pytest.mark.parametrize("shape", I.CHAIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_in_statistics_scheme(shape, mel):
    """fp32 accumulators over a thread's W / slots pixels, as ds_conv3x3_c1 first had them, against double sums of the same
    stored values, through the float64 finish.  Prints the error / bound of both; double always holds the bound; fp32 misses it
    on the silent 80 x 848 mel (the same rounding 106 times)."""
    B, H, W, C = shape
    x, w, bias, gamma, beta = I.chain_case(shape, mel)
    assert float(x.min()) >= -1 and float(x.max()) <= 1
    if mel == "silent":
        assert (x == -1).all()
    if mel == "silent_past_300":
        assert (x[:, :, (300 if W > 300 else 12):] == -1).all() and not (x[:, :, :12] == -1).all()
    y = F.conv2d(x[:, None], w.view(C, 1, 3, 3), bias, padding=1).permute(0, 2, 3, 1).contiguous()      # fp32, [B][H][W][C]
    ref = R.groupnorm_affine(y.view(B, H * W, C), 32, gamma, beta, I.GN_EPS)
    n = H * W * (C // 32)
    s, q = y.double().sum((1, 2)), y.double().pow(2).sum((1, 2))
    dbl = R.groupnorm_affine_from_sums(s, q, n, 32, gamma, beta, I.GN_EPS)
    s32, q32 = R.conv3x3_c1_stats_fp32_scheme(y, 256 // (C // 4))
    f32 = R.groupnorm_affine_from_sums(s32, q32, n, 32, gamma, beta, I.GN_EPS)
    rep_d = R.groupnorm_report(dbl[0].float(), dbl[1].float(), ref, beta)
    rep_f = R.groupnorm_report(f32[0].float(), f32[1].float(), ref, beta)
    print("%s %s: double sums %.3f of the bound, fp32 accumulators %.3f" % (shape, mel, rep_d["worst"], rep_f["worst"]))
    assert rep_d["worst"] <= 0.3
    if mel == "silent" and W == 848:
        assert not rep_f["ok"]


# ------------------------------------------------------------------------------------------------ softmax
@pytest.mark.parametrize("n", I.SM_N)
def test_softmax_cases(n):
    assert I.sm_ld(n)[0] == n and I.sm_ld(n)[1] % 32 == 0 and 0 <= I.sm_ld(n)[1] - n < 32
    for regime, scales in I.SM_REGIMES.items():
        x = I.sm_case(regime, n)
        assert x.shape == (530, n) and torch.isfinite(x).any(1).all()
        for scale in scales:
            y64, y32 = R.softmax_rows(x, scale, F64), R.softmax_rows(x, scale, F32)
            assert torch.isfinite(y64).all() and (y64.sum(1) - 1).abs().max() < 1e-12
            assert R.bound_report(y32, y64, y32, dim=1)["ok"]
            assert float((y32.double().sum(1) - 1).abs().max()) <= n * 2.0 ** -23
            if regime == "flat" or scale == 0.0:
                assert (y64 - 1.0 / n).abs().max() <= 2.0 ** -50 and torch.equal(y32, torch.full_like(y32, 1.0 / n))
            if regime == "sharp":
                assert scale == 1.0 and int((y64 == 1).sum()) == 530 and int((y64 == 0).sum()) == 530 * (n - 1)
            if regime == "neg_inf" and n > 1:
                assert torch.isinf(x).any() and (y64[torch.isinf(x)] == 0).all()
            if regime == "spread" and scale == 1.0 and n >= 63:
                assert float(x.max() - x.min()) > 55
                unscaled = R.softmax_rows(x, 0.044, F32)                 # a kernel that uses another scale is far outside
                assert not R.bound_report(unscaled, y64, y32, dim=1)["ok"]


# ------------------------------------------------------------------------------------------------ stencil9, layout
@pytest.mark.parametrize("shape", I.S9_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stencil9_chain(shape):
    B, H, W = shape
    eye = torch.zeros(1, 9, 3, 3, dtype=F64)
    for k in range(9):
        eye[0, k, k // 3, k % 3] = 1.0
    other = 0
    for ldt in I.S9_LDT:
        for scale in I.S9_SCALES:
            taps, bias = I.s9_case(shape, ldt, scale)
            assert taps.shape == (B, H, W, ldt) and float(taps[..., :9].abs().max()) <= scale
            y64, y32 = R.stencil9(taps, bias, F64), R.stencil9(taps, bias, F32)
            conv = F.conv2d(taps[..., :9].double().permute(0, 3, 1, 2), eye, padding=1)[:, 0] + float(torch.tensor(bias, dtype=F32))
            assert float((y64 - conv).abs().max()) <= 1e-12 * scale
            assert R.bound_report(y32, y64, y32)["ok"]
            rev = R.stencil9(taps[..., [8, 7, 6, 5, 4, 3, 2, 1, 0]].flip((1, 2)), bias, F32).flip((1, 2))      # the taps in reverse order
            assert float((rev.double() - y64).abs().max()) <= 1e-5 * scale
            other += int((rev != y32).sum())
    if H * W >= 100:
        assert other > 0                                                # bit equality tells the order of the chain


def test_layout_cases():
    for shape in I.MEL_SHAPES:
        B, C, T, Cpad = shape
        mel = I.mel_case(shape)
        y, mag = R.mel_to_cl(mel, Cpad, 1.0, 0.0)
        assert y.shape == (B, T, Cpad) and torch.equal(y[..., :C].float(), mel.permute(0, 2, 1)) and (y[..., C:] == 0).all()
        for a, b in I.MEL_AB[1:]:
            y64, mag = R.mel_to_cl(mel, Cpad, a, b, F64)
            y32, _ = R.mel_to_cl(mel, Cpad, a, b, F32)
            assert float(((y32.double() - y64).abs()[..., :C] / R.ulp32(mag[..., :C])).max()) <= 0.5
    seen = set()
    for shape in I.CB_SHAPES:
        B, H, W, C, K = shape
        tok, E = I.cb_case(shape)
        assert tok.shape == (B, H * W) and E.shape == (K, C) and C % 4 == 0
        seen |= {"low"} if int(tok.min()) == -1 else set()
        assert int(tok.max()) == K
        g = R.codebook_gather(tok, E, H, W)
        for b, h, w_ in ((0, 0, 0), (B - 1, H - 1, W - 1), (0, H // 2, W // 2)):
            assert torch.equal(g[b, h, w_], E[int(tok[b, w_ * H + h].clamp(0, K - 1))])
    assert "low" in seen
