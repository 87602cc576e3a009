"""CPU references for the CLIP text tower (modeling/clip_text.py) and for each kernel it calls: stock torch only, never the code
under test.

* `tower64`: the tower's formula in float64 on the fp16-valued weights that convert_weights produces (Linear / attention
  weights and biases, the token and position rows as the tower adds them), LayerNorm gains in fp32, NO rounding of activations.
  It is what the fp16 tower approximates; `oracle.clip_text_embed` (stock torch fp16) is the reference's own arithmetic.
* One function per kernel with the kernel's documented rounding chain, evaluated in the dtype it is given (float64 or
  float32).  Each returns the chain's value BEFORE the final rounding to fp16: the bound below adds what that rounding costs.
* `ulp16`, `r16` (exact round-to-nearest-even onto the fp16 grid in either dtype; float64 -> fp16 through torch would round
  twice) and `bound_report`, the one bound of every kernel-level comparison:

      |k - y| <= ulp16(max(|k|, |y|)) / 2 + 4 * d32,      d32 = max |chain32 - chain64| before the final rounding

  with y the float64 chain before its final rounding.  Where y rounds to +-inf the kernel must give that inf, unless |y| lies
  within 4 * d32 of 65520 (the tie between 65504 and the overflow).
"""
import torch
import torch.nn.functional as F

PFX = "transformer.condition_emb."
F16_MAX, F16_TIE = 65504.0, 65520.0


def ulp16(v):
    """fp16's spacing at |v| (float64): 2^(floor(log2 |v|) - 10), and 2^-24 below 2^-14 (the subnormal grid)."""
    a = v.detach().double().abs()
    fin = torch.where(torch.isfinite(a), a, torch.full_like(a, 65536.0))
    _, e = torch.frexp(fin)
    u = torch.ldexp(torch.ones_like(fin), (e - 11).clamp(min=-24))
    return torch.where(fin < 2.0 ** -14, torch.full_like(fin, 2.0 ** -24), u)


def r16(t):
    """Round to the nearest fp16 value (ties to even, overflow to inf at 65520, subnormals kept), staying in t's dtype."""
    if t.dtype != torch.float64:
        return t.half().to(t.dtype)                                     # one rounding
    u = ulp16(t)
    y = torch.round(t / u) * u                                          # t / u is exact; torch.round is half-to-even
    y = torch.where(y.abs() > F16_MAX, torch.sign(t) * float("inf"), y)
    return torch.where(torch.isfinite(t), y, t)


# ---------------------------------------------------------------------------------------------- kernel chains
def embed(table, pos, ids, T):
    """ds_embed_f16: r16(r16(a) + r16(b)), negative ids read row 0.  Exact in fp32 (two fp16 values add exactly), so this
    is the kernel's output itself, float32."""
    ids = ids.reshape(-1).clamp(min=0)
    p = torch.arange(ids.numel()) % T
    return (table[ids].half().float() + pos[p].half().float()).half().float()


def layernorm_pre(x, g, b, dt, eps=1e-5):
    """ds_layernorm_f16: LayerNorm in the working precision (biased variance, eps inside the root), then ONE rounding."""
    return F.layer_norm(x.to(dt), (x.shape[-1],), g.to(dt), b.to(dt), eps)


def layernorm_no_mean_pre(x, g, b, dt, eps=1e-5):
    """A wrong LayerNorm: the variance taken about 0 (the mean is still subtracted from x)."""
    x = x.to(dt)
    m = x.mean(-1, keepdim=True)
    return (x - m) / ((x * x).mean(-1, keepdim=True) + eps).sqrt() * g.to(dt) + b.to(dt)


def l2norm_pre(x, dt):
    """ds_l2norm_rows_f16: the row norm is rounded to fp16 (inf past 65504, the quotients are then 0), then the quotient is."""
    x = x.to(dt)
    return x / r16(x.norm(dim=-1, keepdim=True))


def attention_probs(qkv, B, T, H, dt, scale=0.125, f16=True, mask_shift=1):
    """(probabilities before their rounding [B][H][T][T], kept-key mask [T][T]) of attention_pre below."""
    D = H * 64
    q, k = [qkv[:, i * D:(i + 1) * D].to(dt).reshape(B, T, H, 64).transpose(1, 2) for i in range(2)]
    s = (q @ k.transpose(-2, -1)) * scale
    if f16:
        s = r16(s)
    i = torch.arange(T)
    keep = i[None, :] < i[:, None] + mask_shift
    p = torch.softmax(s.masked_fill(~keep, float("-inf")), -1)
    return torch.where(keep.expand_as(p), p, torch.zeros_like(p)), keep  # a row without keys (mask_shift = 0) gives 0


def attention_pre(qkv, B, T, H, dt, scale=0.125, f16=True, mask_shift=1, drop_tile=None):
    """ds_attention_ex(causal = 1) on a fused [B*T][3*H*64] buffer: the scaled score is rounded, keys > query are masked,
    the probabilities are rounded, the output is (the final rounding is left to the caller).  mask_shift: key < query +
    mask_shift is kept (1 is right).  drop_tile: the keys of that 32-key tile contribute nothing to the output."""
    D = H * 64
    v = qkv[:, 2 * D:].to(dt).reshape(B, T, H, 64).transpose(1, 2)
    p, _ = attention_probs(qkv, B, T, H, dt, scale, f16, mask_shift)
    if f16:
        p = r16(p)
    if drop_tile is not None:
        p = p.clone()
        p[..., 32 * drop_tile:32 * drop_tile + 32] = 0
    return (p @ v).transpose(1, 2).reshape(B * T, D)


def tie_margin(p):
    """Distance of p (float64) from the nearest fp16 rounding tie, relative to p (inf where p is 0)."""
    p = p.double()
    u = ulp16(p)
    frac = p / u - torch.floor(p / u)
    return torch.where(p > 0, (frac - 0.5).abs() * u / p.clamp(min=1e-300), torch.full_like(p, float("inf")))


def attention_scores(qkv, B, T, H, scale=0.125):
    """The kept scaled scores (float64, masked ones set to 0): what the softmax sees."""
    D = H * 64
    q, k = [qkv[:, i * D:(i + 1) * D].double().reshape(B, T, H, 64).transpose(1, 2) for i in range(2)]
    return ((q @ k.transpose(-2, -1)) * scale).tril()


def gemm_pre(A, W, bias, dt, act=False, R=None):
    """ds_gemm(f16_round = 1): bias, then round; QuickGELU with three roundings (1.702 x, the sigmoid, the product); residual
    add, then round.  Returns the value before the LAST of these roundings."""
    v = A.to(dt) @ W.to(dt).t() + bias.to(dt)
    if act:
        v = r16(v)
        c = torch.tensor(1.702, dtype=torch.float32).to(dt)              # the kernel multiplies by the fp32 constant
        v = v * r16(1.0 / (1.0 + torch.exp(-r16(c * v))))
    if R is not None:
        v = r16(v) + R.to(dt)
    return v


# ---------------------------------------------------------------------------------------------- the bound
def bound_report(k, y64, y32):
    """k: kernel output (or anything claiming to be it); y64 / y32: the chain before its final rounding in float64 / float32.
    Returns {ok, bad (elements outside the bound), worst (largest error / bound), d32, used (the largest error beyond the
    half spacing, in units of d32: the bound allows 4), differ (share of elements that are not the rounded float64 chain)}."""
    k, y64, y32 = k.detach().double().cpu(), y64.double(), y32.double()
    assert k.shape == y64.shape == y32.shape
    both = torch.isfinite(y64) & torch.isfinite(y32)
    d32 = float((y64 - y32)[both].abs().max()) if both.any() else 0.0
    yr = r16(y64)
    over = torch.isinf(yr)
    near = (y64.abs() - F16_TIE).abs() <= 4 * d32
    tol = 0.5 * ulp16(torch.maximum(k.abs(), y64.abs())) + 4 * d32
    err = (k - y64).abs()
    err = torch.where(torch.isinf(k) & (k == yr), torch.zeros_like(err), err)      # the same inf is no error
    fine = torch.where(over & ~near, k == yr, (err <= tol) | (near & (k == yr)))
    fine &= ~torch.isnan(k)
    ratio = torch.where(torch.isfinite(err) & (fine | (err > tol)), err / tol, torch.full_like(err, float("inf")))
    over_half = (err - 0.5 * ulp16(torch.maximum(k.abs(), y64.abs()))).clamp(min=0)
    used = float(over_half[torch.isfinite(over_half)].max() / d32) if d32 > 0 and torch.isfinite(over_half).any() else 0.0
    return {"ok": bool(fine.all()), "bad": int((~fine).sum()), "worst": float(ratio.max()), "d32": d32, "used": used,
            "differ": float((k != yr).double().mean())}


# ---------------------------------------------------------------------------------------------- the tower
def tower64(sd, tokens, mask_shift=1, scale=0.125, heads=8, pfx=PFX, want_scores=False):
    """CLIPTextEmbedding.forward (pick_last_embedding False) in float64: token + position rows, 12 x [x += MHA(ln_1 x,
    causal); x += c_proj(QuickGELU(c_fc(ln_2 x)))], ln_final, rows l2-normalised.  Weights carry the values convert_weights
    leaves (fp16 for Linear / attention / the embedding rows as they enter the sum, fp32 LayerNorm), activations are never
    rounded.  mask_shift / scale: the wrong variants of test_clip_host.py.  want_scores: also return the largest kept
    |score| of the last layer."""
    h = lambda n: sd[pfx + n].half().double()
    f = lambda n: sd[pfx + n].float().double()
    B, T = tokens.shape
    d = sd[pfx + "ln_final.weight"].shape[0]
    ln = lambda x, n: F.layer_norm(x, (d,), f(n + ".weight"), f(n + ".bias"), 1e-5)
    x = sd[pfx + "token_embedding.weight"][tokens.clamp(min=0)].half().double() + h("positional_embedding")[:T]
    x = x.reshape(B * T, d)
    top, i = 0.0, 0
    while (pfx + "transformer.resblocks.%d.ln_1.weight" % i) in sd:
        b = "transformer.resblocks.%d." % i
        qkv = ln(x, b + "ln_1") @ h(b + "attn.in_proj_weight").t() + h(b + "attn.in_proj_bias")
        top = float(attention_scores(qkv, B, T, heads, scale).abs().max())
        a = attention_pre(qkv, B, T, heads, torch.float64, scale=scale, f16=False, mask_shift=mask_shift)
        x = x + a @ h(b + "attn.out_proj.weight").t() + h(b + "attn.out_proj.bias")
        y = ln(x, b + "ln_2") @ h(b + "mlp.c_fc.weight").t() + h(b + "mlp.c_fc.bias")
        y = y * torch.sigmoid(1.702 * y)
        x = x + y @ h(b + "mlp.c_proj.weight").t() + h(b + "mlp.c_proj.bias")
        i += 1
    x = ln(x, "ln_final")
    x = (x / x.norm(dim=-1, keepdim=True)).reshape(B, T, d)
    return (x, top) if want_scores else x
