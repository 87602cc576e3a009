"""Restatements of the transformer's row kernels (csrc/norm.hip, csrc/train.hip) in stock torch on the CPU, for
tests/test_hip_row_kernels.py and tests/test_rows_host.py.  Every formula takes a dtype: in float64 it is the yardstick, in
float32 it is the same formula operation by operation at the kernel's precision and, where the kernel fixes an order, in the
kernel's order (a lane's serial sums, the wave butterfly, the four interleaved chains of the column sums, chunks in index order).
The distance of the two on an input is that input's d32.  No code under test is imported here.

The bounds (DESIGN.md section 4's convention):
  * a fixed-order fp32 chain without a multiply (the column sums, ds_embed): the float32 restatement, bit for bit;
  * everything else, on every element:  |kernel - y64| <= 4 max(d32, 1 ulp of fp32 at `term`), d32 per row (per element for
    the elementwise GELU2), `term` = the largest quantity added or subtracted to form the element -- a cancellation leaves
    an error of that term's ulp, not of the result's.  Each `term` stands next to its expression below.
`variant` names a deliberately wrong kernel (tests/test_rows_host.py shows that each one breaks its bound)."""
import torch

F64, F32 = torch.float64, torch.float32
FACTOR = 4.0
D = 1024
TINY = 2.0 ** -126
_LANE = torch.arange(64)


def f32const(v, dtype):
    """the fp32 value a C `float` argument or literal carries, in `dtype`"""
    return torch.tensor(v, dtype=F32).to(dtype)


def ulp32(y):
    """spacing of fp32 at |y| (y finite, any dtype): 2^(e - 23) for 2^e <= |y| < 2^(e+1), 2^-149 below the normal range"""
    y = y.to(F64).abs()
    _, e = torch.frexp(y)                                   # |y| = m 2^e, m in [0.5, 1)
    e = torch.where(y == 0, torch.full_like(e, -125), e).clamp(min=-125)
    return torch.ldexp(torch.ones_like(y), e - 24)


def bound_report(k, y64, y32, term=None, dim=1, floor_denormal=False):
    """The bound on every element.  d32 = max |y32 - y64| over `dim` of each row (dim=None: the element's own); the ulp is
    taken at `term` (default: at y64).  floor_denormal: where y64 is below the normal range the bound is at least 2^-126.
    Also the row-wise cap figure: d32 / the row's largest |y64| (0 where the row is all zero)."""
    k, y64, y32 = k.to(F64), y64.to(F64), y32.to(F64)
    gap = (y32 - y64).abs()
    d32 = gap if dim is None else gap.amax(dim, keepdim=True).expand_as(y64)
    bound = FACTOR * torch.maximum(d32, ulp32(y64 if term is None else term))
    if floor_denormal:
        bound = torch.where(y64.abs() < TINY, bound.clamp(min=TINY), bound)
    err = (k - y64).abs()
    bad = ~(err <= bound)                                    # a NaN in k is outside
    big = y64.abs() if dim is None else y64.abs().amax(dim, keepdim=True).expand_as(y64)
    cap = torch.where(big > 0, d32 / big.clamp(min=1e-300), torch.zeros_like(d32))
    return {"worst": float((err / bound).nan_to_num(nan=float("inf")).max()), "d32": float(gap.max()), "bad": int(bad.sum()),
            "ok": not bool(bad.any()), "n": k.numel(), "cap": float(cap.max())}


def same_floats(a, b):
    """bit-for-bit (+0 and -0 are different) up to the payload of a NaN"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32)))


def differing(a, b):
    """number of elements whose bits differ (fp32)"""
    return int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum())


def torch_split(a):
    """ds_split_hi / ds_split_lo (csrc/common.h) in torch: hi = fp16(clamp(a)), lo = fp16(clamp(a - hi)) -> [2][...] fp16"""
    hi = a.clamp(-65504.0, 65504.0).half()
    lo = (a - hi.float()).clamp(-65504.0, 65504.0).half()
    return torch.stack((hi, lo)).contiguous()


# ------------------------------------------------------------------------------------------------ the wave's view of a row
def lanes(x):
    """[M][D] -> [M][D / 256][64][4]: lane l holds the float4 at columns (j 64 + l) 4 .. + 3, j = 0 .. D / 256 - 1"""
    return x.reshape(x.shape[0], -1, 64, 4)


def butterfly(s):
    """[..., 64] -> [...]: v += v[lane ^ o] for o = 32 .. 1 (tr_wsum / wave_sum); every lane ends with the same bits"""
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., _LANE ^ o]
    return s[..., 0]


def row_stats(x, dtype, eps=1e-5, variant=None):
    """mean and rstd per row [M], the kernels' way: a lane adds (v0 + v1) + (v2 + v3) per float4, the wave butterfly, times
    1 / D; then the squares of x - mean one after the other, the butterfly, biased variance, 1 / sqrt(var + eps)."""
    v = lanes(x.to(dtype))
    s = torch.zeros(v.shape[0], 64, dtype=dtype)
    for j in range(v.shape[1]):
        s = s + ((v[:, j, :, 0] + v[:, j, :, 1]) + (v[:, j, :, 2] + v[:, j, :, 3]))
    mean = butterfly(s) * (1.0 / D)
    q = torch.zeros_like(s)
    for j in range(v.shape[1]):
        for k in range(4):
            d = v[:, j, :, k] - (0.0 if variant == "var_keeps_mean" else mean[:, None])     # the mutant: E[x^2]
            q = q + d * d
    rstd = 1.0 / torch.sqrt(butterfly(q) * (1.0 / D) + f32const(eps, dtype))
    return mean, rstd


# ------------------------------------------------------------------------------------------------ ds_adaln / ds_layernorm
def norm_forward(x, scale, shift, dtype, ada, variant=None):
    """x, scale, shift [M][D] (scale / shift already gathered per row: the table row of the sample, or gamma / beta).
    y = xn s + shift,  s = 1 + scale (AdaLN) or scale;  xn = (x - mean) rstd.
    term = |x - mean| rstd |s|: the product that x - mean (a cancellation at a large mean) and 1 + scale enter."""
    mean, rstd = row_stats(x, dtype, variant=variant)
    xn = (x.to(dtype) - mean[:, None]) * rstd[:, None]
    s = scale.to(dtype)
    if ada and variant != "scale_without_one":
        s = 1.0 + s
    sh = shift.to(dtype)
    y = xn * s + sh
    return y, xn, (xn * s).abs()


# ------------------------------------------------------------------------------------------------ ds_layernorm_bwd(_sums)
def norm_backward(x, dy, scale, dtype, ada, variant=None):
    """g = dy s;  dx = rstd (g - mean(g) - xn mean(g xn));  dyxn = dy xn.  A lane adds its 16 g and g xn one after the other
    (j, then k), the butterfly, times 1 / D.
    term of dx = rstd max(|g|, |mg|, |xn mgx|);  dyxn is one product: its term is itself.  Returns dx, dyxn, term, xn."""
    mean, rstd = row_stats(x, dtype)
    xn = (x.to(dtype) - mean[:, None]) * rstd[:, None]
    s = 1.0 + scale.to(dtype) if ada else scale.to(dtype)
    d = dy.to(dtype)
    g = d * s
    gl, xl = lanes(g), lanes(xn)
    sg = torch.zeros(x.shape[0], 64, dtype=dtype)
    sgx = torch.zeros_like(sg)
    for j in range(gl.shape[1]):
        for k in range(4):
            gk = gl[:, j, :, k]
            if variant == "mean_g_short" and j == gl.shape[1] - 1 and k == 3:         # the mutant: D - 1 of the D elements
                gk = gk * (_LANE < 63).to(dtype)                                      #   (column D - 1 is left out)
            sg = sg + gk
            sgx = sgx + gl[:, j, :, k] * xl[:, j, :, k]
    mg, mgx = butterfly(sg) * (1.0 / D), butterfly(sgx) * (1.0 / D)
    if variant == "no_mg":
        mg = torch.zeros_like(mg)
    if variant == "no_xn_mgx":
        mgx = torch.zeros_like(mgx)
    r = rstd[:, None]
    dx = r * (g - mg[:, None] - xn * mgx[:, None])
    term = r * torch.maximum(torch.maximum(g.abs(), mg.abs()[:, None].expand_as(g)), (xn * mgx[:, None]).abs())
    return dx, d * xn, term, xn


def chunking(rows):
    """ds_layernorm_bwd_sums: chunks per group = ceil(rows / 16), rows per chunk = ceil(rows / chunks)"""
    cpg = (rows + 15) // 16
    return cpg, (rows + cpg - 1) // cpg


def bwd_sums_parts(dy, xn, G, rows, dtype):
    """part [G cpg][2][D] of ds_layernorm_bwd_sums: wave w of a chunk adds dy xn and dy of rows r_lo + w, + 4, ... one after the
    other (a wave without a row holds zeros), the four waves are joined as ((w0 + w1) + w2) + w3."""
    cpg, rpc = chunking(rows)
    d, n = dy.to(dtype), xn.to(dtype)
    part = torch.zeros(G * cpg, 2, D, dtype=dtype)
    for grp in range(G):
        for ck in range(cpg):
            lo = grp * rows + ck * rpc
            hi = min(lo + rpc, (grp + 1) * rows)
            w = torch.zeros(4, 2, D, dtype=dtype)
            for wave in range(4):
                for r in range(lo + wave, hi, 4):
                    w[wave, 0] = w[wave, 0] + d[r] * n[r]
                    w[wave, 1] = w[wave, 1] + d[r]
            part[grp * cpg + ck] = ((w[0] + w[1]) + w[2]) + w[3]
    return part


def bwd_sums(dy, xn, G, rows, dtype):
    """[G][2][D]: d scale = column sums of dy xn, d shift = column sums of dy per group, the way the training step forms them --
    ds_colsum over the chunks of `part` (float64: plain sums).  term [G][2][D] = the largest |dy xn|, |dy| of the column."""
    d, n = dy.to(F64).view(G, rows, D), xn.to(F64).view(G, rows, D)
    term = torch.stack(((d * n).abs().amax(1), d.abs().amax(1)), 1)
    if dtype == F64:
        return torch.stack(((d * n).sum(1), d.sum(1)), 1), term
    cpg, _ = chunking(rows)
    part = bwd_sums_parts(dy, xn, G, rows, dtype)
    return colsum(part.view(G, cpg, 2 * D), dtype).view(G, 2, D), term


# ------------------------------------------------------------------------------------------------ ds_colsum / ds_colsum_ws
def colsum(x, dtype, start=None, variant=None):
    """x [G][R][C] -> [G][C], the order written in both kernels: chains s0 .. s3 take rows r = 0, 1, 2, 3 (mod 4) below R & ~3
    in row order, the R % 4 tail rows join chain 0, then (s0 + s1) + (s2 + s3); accumulate: start + that."""
    G, R, C = x.shape
    x = x.to(dtype)
    if dtype == F64:
        t = x.sum(1)
    else:
        s = [torch.zeros(G, C, dtype=dtype) for _ in range(4)]
        R4 = R & ~3
        for r in range(R4):
            s[r & 3] = s[r & 3] + x[:, r]
        tail = 3 if variant == "tail_chain3" else 0              # the mutant: the tail rows on chain 3
        for r in range(R4, R):
            s[tail] = s[tail] + x[:, r]
        t = (s[0] + s[1]) + (s[2] + s[3])
    return t if start is None else start.to(dtype) + t


def colsum_ws(x, rs, dtype, start=None, variant=None):
    """The chunked form: rs chunks of ceil(R / rs) rows, each summed as above from its own first row (an empty chunk gives an
    exact zero), the chunks then added as above in index order."""
    G, R, C = x.shape
    chunk = (R + rs - 1) // rs
    work = torch.zeros(G, rs, C, dtype=dtype)
    for k in range(rs):
        r0, r1 = k * chunk, min((k + 1) * chunk, R)
        if r1 > r0:
            work[:, k] = colsum(x[:, r0:r1], dtype)
    if variant == "first_chunk_only":
        work[:, 1:] = 0
    if variant == "chunks_reversed":
        work = work.flip(1)
    return colsum(work, dtype, start)


def colsum_term(x):
    """the largest |x| of each column [G][C]"""
    return x.to(F64).abs().amax(1)


# ------------------------------------------------------------------------------------------------ ds_gelu2
def gelu2(x, dy, dtype, c=1.702):
    """forward (dy None): x / (1 + exp(-1.702 x)), one quotient: its term is itself.
    backward: dy (sg + 1.702 x sg (1 - sg)), sg = 1 / (1 + exp(-1.702 x));  term = |dy| max(sg, |1.702 x sg (1 - sg)|): the two
    cancel at x = -0.7524.  float64 uses 1.702 itself, float32 the kernel's 1.702f."""
    v = x.to(dtype)
    cc = f32const(c, dtype) if dtype == F32 else torch.tensor(c, dtype=dtype)
    e = torch.exp(-cc * v)
    if dy is None:
        y = v / (1.0 + e)
        return y, y.abs()
    sg = 1.0 / (1.0 + e)
    b = cc * v * sg * (1.0 - sg)
    d = dy.to(dtype)
    return d * (sg + b), d.abs() * torch.maximum(sg, b.abs())


# ------------------------------------------------------------------------------------------------ ds_softmax_bwd_rows
def softmax_bwd(P, dP, n, scale, dtype, variant=None):
    """P, dP [rows][>= n]: dS = scale P (dP - s), s = sum_j dP_j P_j over the first n columns -- lane l adds columns l, l + 64,
    ... one after the other, then the butterfly.  term = scale P max(|dP|, |s|).  Returns dS [rows][n], term."""
    m = P.shape[1] if variant == "sum_over_ld" else n            # the mutant: the sum runs over the padding too
    p, d = P[:, :m].to(dtype), dP[:, :m].to(dtype)
    pad = (-m) % 64
    pr = torch.nn.functional.pad(p * d, (0, pad)).view(P.shape[0], -1, 64)      # (a lane past n adds nothing)
    s = torch.zeros(P.shape[0], 64, dtype=dtype)
    for k in range(pr.shape[1]):
        s = s + pr[:, k]
    s = butterfly(s)[:, None]
    sc = 1.0 if variant == "no_scale" else f32const(scale, dtype)
    p, d = p[:, :n], d[:, :n]
    return sc * p * (d - s), (sc * p).abs() * torch.maximum(d.abs(), s.abs().expand_as(d))


# ------------------------------------------------------------------------------------------------ ds_embed
def embed(tok, emb, pos, L):
    """x[m] = emb[max(tok[m], 0)] + pos[m % L]: one fp32 add per element"""
    return emb[tok.clamp(min=0)] + pos[torch.arange(tok.shape[0]) % L]
