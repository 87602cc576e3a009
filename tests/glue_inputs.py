"""Named inputs of tests/test_hip_codec_glue.py (GPU) and tests/test_glue_host.py (CPU): shapes, regimes and the seeded tensors
of every case.  No code under test is imported here; everything is a function of its arguments (torch.Generator seeds), so the
GPU test and the host test see the same tensors."""
import torch

F32 = torch.float32
NAN, INF = float("nan"), float("inf")


def _gen(*key):
    s = 0
    for c in repr(key):                                       # a stable seed (Python's hash() is salted per process)
        s = (s * 131 + ord(c)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _uniform(shape, g, lo=-1.0, hi=1.0):
    return torch.rand(shape, generator=g, dtype=torch.float64).mul(hi - lo).add(lo).float()


# ------------------------------------------------------------------------------------------------ ds_vq_argmin
VQ_K = (1, 63, 64, 65, 256, 1000, 2048)
VQ_M = (1, 2, 3, 4, 5, 265 * 3)
VQ_C = (1, 64, 100, 256)
VQ_NONFINITE = ("one_nan", "nan_last", "all_nan", "all_inf", "neg_inf", "two_neg_inf", "nan_and_neg_inf", "nan_in_z")


def vq_patterns(K):
    """The distance rows d[K] a codebook of K entries is searched on: a list of (name, d f32[K], nan_in_z).  Finite rows hold
    small integers (exact however they are computed): base values 10 .. 20, minima 1.
      min@p      the unique minimum at p: 0, K - 1, every lane of the first pass (k < 64) and of the last (k >= 64 ((K - 1) / 64))
      tie@k      the same minimum at k, k + 1, k + 64, k + 65 (those below K): the lowest wins across lanes and within one
      equal      an all-equal row
    and the non-finite rows of VQ_NONFINITE."""
    k = torch.arange(K)
    base = (10 + (k * 37) % 11).float()
    rows = []
    last0 = 64 * ((K - 1) // 64)
    for p in sorted(set([0, K - 1] + list(range(min(64, K))) + list(range(last0, K)))):
        d = base.clone()
        d[p] = 1.0
        rows.append(("min@%d" % p, d, False))
    for k0 in sorted(set(x for x in (0, 1, 62, 63, 64, K - 66, K - 65, K - 2) if 0 <= x < K)):
        d = base.clone()
        for j in (k0 + 65, k0 + 64, k0 + 1, k0):
            if j < K:
                d[j] = 1.0
        rows.append(("tie@%d" % k0, d, False))
    rows.append(("equal", torch.full((K,), 7.0), False))
    mid = K // 2
    for name in VQ_NONFINITE:
        d = base.clone()
        if name == "one_nan":
            d[mid] = NAN
            d[0] = 1.0 if K > 1 else d[0]
        elif name == "nan_last":
            d[K - 1] = NAN
        elif name == "all_nan":
            d[:] = NAN
        elif name == "all_inf":
            d[:] = INF
        elif name == "neg_inf":
            d[mid] = -INF
        elif name == "two_neg_inf":
            d[mid] = -INF
            d[K - 1] = -INF
        elif name == "nan_and_neg_inf":
            d[0] = -INF
            d[K - 1] = NAN
        rows.append((name, d, name == "nan_in_z"))
    return rows


def vq_case(K, C, M):
    """Integer family: M rows drawn from vq_patterns(K) (all of them, cycled, when M allows; a window that moves with (K, C, M)
    otherwise, the non-finite rows first for M = 5), odd rows with a small-integer z, even rows with z = 0.
    Returns z [M][C], ze [M][K], ee [K] (fp32, all finite entries integers or half-integers), names."""
    pats = vq_patterns(K)
    if M >= len(pats):
        pick = [i % len(pats) for i in range(M)]
    else:
        first = len(pats) - len(VQ_NONFINITE) if M == 5 else (7 * K + 3 * C + M) % len(pats)
        pick = [(first + (K + C) % 3 * (M == 5) + i) % len(pats) for i in range(M)]
    g = _gen("vq", K, C, M)
    ee = torch.randint(0, 6, (K,), generator=g).float()
    z = torch.zeros(M, C)
    z[1::2] = torch.randint(-2, 3, (z[1::2].shape[0], C), generator=g).float()
    D = torch.stack([pats[i][1] for i in pick])
    for r, i in enumerate(pick):
        if pats[i][2]:
            z[r, (r * 5) % C] = NAN
    zz = torch.nan_to_num(z, nan=0.0).pow(2).sum(1, keepdim=True)
    # d = (zz + ee) - 2 ze  <=>  ze = (zz + ee - d) / 2:  NaN -> NaN, +inf -> -inf, -inf -> +inf, integers -> half-integers
    ze = (zz + ee[None, :] - D) / 2
    return z, ze.contiguous(), ee, [pats[i][0] for i in pick]


def vq_rounded_case(K, M):
    """z = 0 and arbitrary fp32 ee, ze on a coarse grid (so equal distances are common): d = ee - 2 ze is ONE fp32 rounding,
    the same on the host whether or not a compiler contracts it."""
    g = _gen("vqr", K, M)
    ee = (torch.randint(0, 64, (K,), generator=g).float() * 0.1)
    ze = (torch.randint(-32, 32, (M, K), generator=g).float() * 0.05)
    return torch.zeros(M, 1), ze, ee


# ------------------------------------------------------------------------------------------------ GroupNorm
GN_SHAPES = ((1, 1, 32, 32), (2, 255, 128, 32), (2, 256, 128, 32), (2, 257, 128, 32), (1, 265, 512, 32), (3, 1060, 96, 32),
             (1, 300, 1024, 32), (2, 64, 64, 64), (1, 513, 8, 1), (1, 40, 4, 4))
GN_DATA = ("zero_mean", "mean_1e2", "mean_1e4", "constant", "big", "tiny")
GN_EPS = 1e-6
GN_FINISH_CHUNKS = (1, 2, 83, 540, 1000)


def gn_case(shape, kind):
    """x [B][P][C], gamma, beta.  zero_mean: unit noise.  mean_1e2 / mean_1e4: every channel gets a mean of that many standard
    deviations -- one sign and size per group (times 1 .. 2 from group to group) plus a jitter of one standard deviation per
    channel, so that |group mean| / (group std) stays of that size: the regime where E[x^2] - mean^2 cancels.  constant /
    big / tiny: group (groups // 2) is the constant 0.75 (variance 0: rstd = 1 / sqrt(eps)) / uniform in +-6e4 / of size 1e-6."""
    B, P, C, groups = shape
    g = _gen("gn", shape, kind)
    x = torch.randn(B, P, C, generator=g, dtype=torch.float64)
    cpg = C // groups
    if kind in ("mean_1e2", "mean_1e4"):
        R = 1e2 if kind == "mean_1e2" else 1e4
        gm = R * (1 + torch.rand(groups, generator=g, dtype=torch.float64)) * (1 - 2 * (torch.arange(groups) % 2))
        x = x + gm.repeat_interleave(cpg)[None, None, :] + torch.randn(C, generator=g, dtype=torch.float64)[None, None, :]
    sel = slice((groups // 2) * cpg, (groups // 2 + 1) * cpg)
    if kind == "constant":
        x[:, :, sel] = 0.75
    if kind == "big":
        x[:, :, sel] = (torch.rand(B, P, cpg, generator=g, dtype=torch.float64) * 2 - 1) * 6e4
    if kind == "tiny":
        x[:, :, sel] = x[:, :, sel] * 1e-6
    gamma = _uniform((C,), g, 0.2, 2.2)
    beta = _uniform((C,), g)
    return x.float(), gamma, beta


def gn_finish_case(nchunk, C=128, groups=32, B=2, ppc=3):
    """Hand-built partial sums with integer values (exact in double in any order): integers in -8 .. 8 at P = nchunk * ppc
    pixels, summed per chunk.  Returns part f64[B][nchunk][2][C], P, gamma, beta."""
    g = _gen("gnf", nchunk, C, groups)
    x = torch.randint(-8, 9, (B, nchunk, ppc, C), generator=g).double()
    x[0, :, :, :C // groups] += 40.0                          # one group far from zero mean
    part = torch.stack((x.sum(2), x.pow(2).sum(2)), dim=2).contiguous()
    return part, nchunk * ppc, _uniform((C,), g, 0.2, 2.2), _uniform((C,), g)


CHAIN_SHAPES = ((1, 80, 848, 128), (2, 16, 33, 64))
CHAIN_MELS = ("uniform", "silent", "silent_past_300")


def chain_case(shape, mel):
    """Encoder.conv_in on a mel in [-1, 1]: x [B][H][W], w [Cout][9], bias [Cout] (init-like: uniform +-1/3, the bound of
    Conv2d's default init at fan-in 9), gamma, beta.  silent = all -1 (a zero-extended clip); silent_past_300 = that from
    column 300 on (from column 12 at W = 33)."""
    B, H, W, C = shape
    g = _gen("chain", shape)
    x = _uniform((B, H, W), g)
    if mel == "silent":
        x[:] = -1.0
    if mel == "silent_past_300":
        x[:, :, (300 if W > 300 else 12):] = -1.0
    w = _uniform((C, 9), g, -1 / 3, 1 / 3)
    bias = _uniform((C,), g, -1 / 3, 1 / 3)
    return x, w, bias, _uniform((C,), g, 0.2, 2.2), _uniform((C,), g)


# ------------------------------------------------------------------------------------------------ ds_softmax_rows
SM_N = (1, 2, 63, 64, 65, 265, 1000)
SM_ROWS = (1, 2, 3, 5, 530)
SM_SCALES = (0.044, 1.0, -1.0, 0.0)
SM_REGIMES = {"flat": SM_SCALES, "unit": SM_SCALES, "sharp": (1.0,), "spread": SM_SCALES, "neg_inf": (0.044, 1.0)}


def sm_ld(n):
    return (n, (n + 31) // 32 * 32)


def sm_case(regime, n, rows=max(SM_ROWS)):
    """x [rows][n] (rows are independent: a call on fewer rows takes the first ones).  flat: all equal (a different value per
    row); unit: uniform +-1; sharp: one entry 1e4 above the rest (at scale 1 the others underflow to exactly 0); spread: uniform
    +-30; neg_inf: unit with every third entry -inf (never the whole row)."""
    g = _gen("sm", regime, n)
    if regime == "flat":
        return (_uniform((rows, 1), g) * 5).expand(rows, n).contiguous()
    x = _uniform((rows, n), g, -30.0, 30.0) if regime == "spread" else _uniform((rows, n), g)
    r = torch.arange(rows)
    if regime == "sharp":
        x[r, (r * 7) % n] += 1e4
    if regime == "neg_inf" and n > 1:                         # (n = 1: nothing to take away, the case is "unit")
        k = torch.arange(n)
        x[(k[None, :] + r[:, None]) % 3 == 1] = -INF
    return x


# ------------------------------------------------------------------------------------------------ stencils and layout
S9_SHAPES = ((1, 1, 1), (1, 1, 5), (2, 3, 1), (2, 20, 33), (1, 5, 53))
S9_LDT = (9, 16)
S9_SCALES = (1.0, 1e4)
S7_N = (4, 5, 7, 255, 256, 257, 500)
S7_B = (1, 3)
S7_LDT = (7, 8)
MEL_SHAPES = ((1, 80, 53, 96), (3, 80, 1, 80), (2, 1, 7, 32), (1, 80, 1712, 96))
MEL_AB = ((1.0, 0.0), (0.5, 0.5), (2.0, -1.0))
CB_SHAPES = ((1, 1, 1, 4, 2), (2, 5, 53, 256, 256), (3, 5, 53, 256, 512), (1, 3, 7, 1024, 16))


def s9_case(shape, ldt, scale):
    """taps [B][H][W][ldt] uniform in +-scale (the columns past 9 hold 1e30: reading one shows), bias"""
    g = _gen("s9", shape, ldt, scale)
    taps = _uniform(tuple(shape) + (ldt,), g) * scale
    taps[..., 9:] = 1e30
    return taps, 0.25 * scale


def s7_case(B, N, ldt):
    """taps [B][N][ldt]: uniform with an amplitude that runs from 0.05 to 3 along the clip and back, so the pre-activations
    cover the linear range of tanh and reach well into its saturation at both (reflecting) ends of a clip; in clip 0 the seven
    taps of output N // 2 are 2.9 and those of output 1 (which reflects) are -2.9: pre-activations of +20.2 and -20.4 (at
    N <= 7 the two outputs share taps; the second one is written last and keeps its -20.4).  Columns past 7 hold 1e30."""
    g = _gen("s7", B, N, ldt)
    t = torch.arange(N, dtype=torch.float64) / max(N - 1, 1)
    amp = 0.05 + 2.95 * (2 * t - 1).abs()
    taps = _uniform((B, N, ldt), g) * amp.float()[None, :, None]
    for t0, v in ((N // 2, 2.9), (1, -2.9)):
        for k in range(7):
            s = abs(t0 + k - 3)
            s = 2 * (N - 1) - s if s >= N else s
            taps[0, s, k] = v
    taps[..., 7:] = 1e30
    return taps, -0.1


def mel_case(shape):
    B, C, T, _ = shape
    return _uniform((B, C, T), _gen("mel", shape), -1.0, 1.0)


def cb_case(shape):
    """tokens [B][H W] in 0 .. K - 1 with a -1 and a K (a leftover [MASK]) planted, codebook [K][C]"""
    B, H, W, C, K = shape
    g = _gen("cb", shape)
    tok = torch.randint(0, K, (B, H * W), generator=g)
    tok[0, 0] = -1
    tok[B - 1, H * W - 1] = K
    if H * W > 2:
        tok[0, 1], tok[0, 2] = 0, K - 1
    return tok, _uniform((K, C), g)
