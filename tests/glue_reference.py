"""float64 restatements of the codec's and the vocoder's glue kernels (csrc/misc.hip, csrc/norm.hip), stock torch on the CPU, for
tests/test_hip_codec_glue.py and tests/test_glue_host.py.  Every formula takes a dtype: in float64 it is the yardstick, in
float32 it is the same formula at the kernel's precision, and the distance of the two on an input is that input's d32.  No code
under test is imported here.

The one bound of the suite (DESIGN.md section 4's factor):   |kernel - y64| <= 4 * max(d32, 1 ulp of fp32 at y64)."""
import torch

F64, F32 = torch.float64, torch.float32
FACTOR = 4.0
GN_REL = 2.0 ** -22          # ds_groupnorm_*: sums in double, ONE rounding to fp32 (2^-24) -- a factor 4 on top, as everywhere


def ulp32(y):
    """spacing of fp32 at |y| (y finite, any dtype): 2^(e - 23) for 2^e <= |y| < 2^(e+1), 2^-149 below the normal range"""
    y = y.to(F64).abs()
    _, e = torch.frexp(y)                                   # |y| = m 2^e, m in [0.5, 1)
    e = torch.where(y == 0, torch.full_like(e, -125), e).clamp(min=-125)
    return torch.ldexp(torch.ones_like(y), e - 24)


def bound_report(k, y64, y32, dim=None):
    """The bound on every element.  d32 = max |y32 - y64| over the whole case (dim=None) or over `dim` of each row."""
    k, y64, y32 = k.to(F64), y64.to(F64), y32.to(F64)
    gap = (y32 - y64).abs()
    d32 = gap.max() if dim is None else gap.amax(dim, keepdim=True)
    bound = FACTOR * torch.maximum(d32.expand_as(y64), ulp32(y64))
    err = (k - y64).abs()
    bad = ~(err <= bound)                                    # a NaN in k is outside
    return {"worst": float((err / bound).nan_to_num(nan=float("inf")).max()), "d32": float(gap.max()), "bad": int(bad.sum()),
            "ok": not bool(bad.any()), "n": k.numel()}


# ------------------------------------------------------------------------------------------------ ds_vq_argmin
def vq_distances(z, ze, ee):
    """d[m][k] = (sum_c z[m][c]^2 + ee[k]) - 2 ze[m][k] in fp32, the kernel's association.  With z = 0 this is ONE rounding of
    ee - 2 ze (2 ze is exact); with small-integer operands it is exact in any order."""
    zz = (z * z).sum(1, keepdim=True)
    return (zz + ee[None, :]) - 2.0 * ze


def vq_argmin(z, ze, ee):
    d = vq_distances(z.float(), ze.float(), ee.float())
    idx = torch.argmin(d, dim=1)                              # first NaN, else first minimum (test_glue_host.py pins this)
    return idx, d.gather(1, idx[:, None])[:, 0], d


def same_floats(a, b):
    """bit-for-bit up to the payload of a NaN"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(a[~na], b[~nb]))


# ------------------------------------------------------------------------------------------------ GroupNorm
def groupnorm_affine(x, groups, gamma, beta, eps, dtype=F64):
    """x [B][P][C] channels-last -> (scale, shift) [B][C] with x * scale + shift == group_norm(x): two-pass mean / biased
    variance per (sample, group) in `dtype`; eps is the fp32 value the C ABI passes."""
    B, P, C = x.shape
    eps = float(torch.tensor(eps, dtype=F32))
    xg = x.to(dtype).view(B, P, groups, C // groups)
    mean = xg.mean((1, 3), keepdim=True)
    var = (xg - mean).pow(2).mean((1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return _affine(mean, rstd, gamma, beta, B, C, groups, dtype)


def groupnorm_affine_from_sums(s, q, n, groups, gamma, beta, eps, dtype=F64):
    """the same from per-channel sums s, q [B][C] (sum, sum of squares over P pixels), n = P * C / groups: the kernel's formula
    var = E[x^2] - mean^2, clamped at 0"""
    B, C = s.shape
    eps = float(torch.tensor(eps, dtype=F32))
    mean = s.to(dtype).view(B, 1, groups, -1).sum(3, keepdim=True) / n
    var = (q.to(dtype).view(B, 1, groups, -1).sum(3, keepdim=True) / n - mean * mean).clamp(min=0)
    rstd = 1.0 / torch.sqrt(var + eps)
    return _affine(mean, rstd, gamma, beta, B, C, groups, dtype)


def _affine(mean, rstd, gamma, beta, B, C, groups, dtype):
    g, b = gamma.to(dtype).view(1, 1, groups, -1), beta.to(dtype).view(1, 1, groups, -1)
    scale = (rstd * g).expand(B, 1, groups, C // groups).reshape(B, C)
    mrg = (mean * rstd * g).expand(B, 1, groups, C // groups).reshape(B, C)
    return scale, b.expand(B, 1, groups, C // groups).reshape(B, C) - mrg, mrg


def groupnorm_report(scale, shift, ref, beta, rel=GN_REL):
    """|scale - ref| <= rel |ref|,  |shift - ref| <= rel (|beta| + |mean rstd gamma|); ref = groupnorm_affine*(...)"""
    rs, rh, mrg = ref
    es = (scale.to(F64) - rs).abs() / (rel * rs.abs())
    eh = (shift.to(F64) - rh).abs() / (rel * (beta.to(F64).abs()[None, :] + mrg.abs()))
    worst = max(float(es.nan_to_num(nan=float("inf")).max()), float(eh.nan_to_num(nan=float("inf")).max()))
    return {"scale": float(es.max()), "shift": float(eh.max()), "worst": worst, "ok": worst <= 1.0}


# ------------------------------------------------------------------------------------------------ ds_softmax_rows
def softmax_rows(x, scale, dtype=F64):
    """softmax(scale * x) per row; scale is the fp32 value the C ABI passes"""
    s = torch.tensor(scale, dtype=F32).to(dtype)
    return torch.softmax(x.to(dtype) * s, dim=1)


# ------------------------------------------------------------------------------------------------ stencils
def stencil9(taps, bias, dtype=F64):
    """taps [B][H][W][>=9] -> [B][H][W]: bias + the taps in (ky, kx) order, zero padding 1, one add after the other in `dtype`
    (in float32: the kernel's chain, to be met bit for bit; a skipped tap and an added +0 are the same)"""
    B, H, W, _ = taps.shape
    t = torch.zeros(B, H + 2, W + 2, 9, dtype=dtype)
    t[:, 1:-1, 1:-1] = taps[..., :9].to(dtype)
    acc = torch.full((B, H, W), float(torch.tensor(bias, dtype=F32)), dtype=dtype)
    for ky in range(3):
        for kx in range(3):
            acc = acc + t[:, ky:ky + H, kx:kx + W, ky * 3 + kx]
    return acc


def reflect(s, N):
    """ReflectionPad1d's index map, as many bounces as it takes (period 2 (N - 1)); N >= 2"""
    period = 2 * (N - 1)
    s = s % period
    return torch.where(s >= N, period - s, s)


def stencil7_pre(taps, bias, dtype=F64):
    """taps [B][N][>=7] -> [B][N]: bias + sum_k taps[b][reflect(t + k - 3)][k], k ascending, in `dtype`"""
    B, N, _ = taps.shape
    t = torch.arange(N)
    acc = torch.full((B, N), float(torch.tensor(bias, dtype=F32)), dtype=dtype)
    for k in range(7):
        acc = acc + taps[:, reflect(t + k - 3, N), k].to(dtype)
    return acc


def stencil7_tanh(taps, bias, dtype=F64):
    return torch.tanh(stencil7_pre(taps, bias, dtype))


def one_bounce_out_of_range(N):
    """taps of the kernel's ONE-bounce reflection (s = -s below 0, then 2 (N - 1) - s past N - 1) that land outside [0, N)"""
    n = 0
    for t in range(N):
        for k in range(7):
            s = t + k - 3
            s = -s if s < 0 else s
            s = 2 * (N - 1) - s if s >= N else s
            n += not 0 <= s < N
    return n


# ------------------------------------------------------------------------------------------------ layout
def mel_to_cl(mel, Cpad, a, b, dtype=F64):
    """mel [B][C][T] -> [B][T][Cpad]: a x + b on the C real channels, zeros behind; also |a x| + |b| (the scale of its rounding)"""
    B, C, T = mel.shape
    a, b = torch.tensor(a, dtype=F32).to(dtype), torch.tensor(b, dtype=F32).to(dtype)
    x = mel.to(dtype).permute(0, 2, 1)
    out = torch.zeros(B, T, Cpad, dtype=dtype)
    mag = torch.zeros(B, T, Cpad, dtype=dtype)
    out[..., :C] = a * x + b
    mag[..., :C] = (a * x).abs() + b.abs()
    return out, mag


def codebook_gather(tokens, E, H, W):
    """tokens [B][H W] in ColumnMajor order (position w H + h), E [K][C] -> [B][H][W][C]; ids clamped to [0, K - 1]"""
    B = tokens.shape[0]
    t = tokens.view(B, W, H).permute(0, 2, 1).clamp(0, E.shape[0] - 1)
    return E[t]


def conv3x3_c1_stats_fp32_scheme(out, slots):
    """What fp32 accumulators do to the statistics ds_conv3x3_c1 hands to ds_groupnorm_finish: out [B][H][W][C] (the stored conv
    output); a thread owns the pixels xx = slot, slot + slots, ... of one image row and adds o and o * o to two fp32 sums;
    the slots' sums, then the rows', are added in double.  Returns per-channel (sum, sum of squares) [B][C] in float64."""
    B, H, W, C = out.shape
    s = torch.zeros(B, C, dtype=F64)
    q = torch.zeros(B, C, dtype=F64)
    for slot in range(slots):
        px = out[:, :, slot::slots]                          # [B][H][n][C]
        a1 = torch.zeros(B, H, C, dtype=F32)
        a2 = torch.zeros(B, H, C, dtype=F32)
        for i in range(px.shape[2]):
            a1 = a1 + px[:, :, i]
            a2 = a2 + px[:, :, i] * px[:, :, i]
        s += a1.to(F64).sum(1)
        q += a2.to(F64).sum(1)
    return s, q
