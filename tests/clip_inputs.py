"""Seeded operands for the kernel-level tests of the CLIP text tower (tests/test_clip_host.py on the references alone,
tests/test_hip_clip_range.py on the GPU).  Every activation is on the fp16 grid, as the tower hands it from kernel to kernel;
LayerNorm gains and biases are fp32, as convert_weights leaves them.  Shapes are the smallest that reach each edge: rows that
are no multiple of the 4 per workgroup, sequence lengths on both sides of the 32-row tiles and of the 96-key switch between the
two attention instantiations, and the tower's own GEMM shapes under every block tile."""
import math

import torch

from text_to_sound_synthesis_amd.synth import _gen

VOCAB, WIDTH = 49408, 512


def h16(t):
    return t.float().half().float()


def _g(name):
    return _gen(0, "clip_inputs." + name)


def _randn(shape, name):
    return torch.randn(tuple(shape), generator=_g(name))


def _rand(shape, name):
    return torch.rand(tuple(shape), generator=_g(name))


# ------------------------------------------------------------------------------------------------ embedding
EMBED_ROWS = (77, 154, 5)                    # 5: not a multiple of the 4 rows per workgroup
EMBED_T = 77

_EMBED_TABLES = []


def embed_tables():
    """Token table [49408][512] and position table [77][512], fp16 grid, column scales over four decades so that most sums
    need the final rounding."""
    if not _EMBED_TABLES:
        col = 10.0 ** (_rand((WIDTH,), "embed.col") * 4 - 2)
        _EMBED_TABLES.append((h16(_randn((VOCAB, WIDTH), "embed.tab") * 0.02 * col),
                              h16(_randn((EMBED_T, WIDTH), "embed.pos") * 0.02 * col.flip(0))))
    return _EMBED_TABLES[0]


def embed_ids(M):
    ids = torch.randint(0, VOCAB, (M,), generator=_g("embed.ids.%d" % M))
    ids[0], ids[1], ids[2], ids[-1] = 0, VOCAB - 1, -3, VOCAB - 1      # first row, last row, a negative id (reads row 0)
    return ids.long()


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_DIMS = (512, 1024)
LN_ROWS = (1, 3, 77, 155)
LN_KINDS = ("plain", "hot", "offset", "tight", "gains", "big")


def layernorm_case(kind, M, D):
    """(x [M][D] on the fp16 grid, gamma, beta).  plain: N(0, 3).  hot: three channels x 300.  offset: 200 + N(0, 0.5).
    tight: 1 + N(0, 2e-3), a variance of the size of eps.  gains: gamma log-uniform over a decade.  big: a row that
    reaches 6e4."""
    n = "ln.%s.%d.%d" % (kind, M, D)
    z = _randn((M, D), n + ".x")
    g = 1.0 + 0.1 * _randn((D,), n + ".g")
    b = 0.1 * _randn((D,), n + ".b")
    if kind == "plain":
        x = 3.0 * z
    elif kind == "hot":
        x = z.clone()
        x[:, [31, 255, D - 32]] *= 300.0
    elif kind == "offset":
        x = 200.0 + 0.5 * z
    elif kind == "tight":
        x = 1.0 + 2e-3 * z
    elif kind == "gains":
        x = 3.0 * z
        g = 10.0 ** (_rand((D,), n + ".lg") - 0.5)
    elif kind == "big":
        x = 3.0 * z
        x[0, 7] = 6e4
        x[M - 1, D - 1] = -6e4
    else:
        raise KeyError(kind)
    return h16(x), g, b


# ------------------------------------------------------------------------------------------------ l2norm
L2_ROWS = (1, 77)
L2_KINDS = ("ordinary", "over", "subnormal")


def l2norm_case(kind, M, D=WIDTH):
    """ordinary: N(0, 1) rows.  over: N(0, 4000) rows, norm about 9e4 > 65504: the rounded norm is inf, the quotients 0.
    subnormal: 16 entries of 25 (norm 100) among entries of about 1e-3: quotients of about 1e-5, below 2^-14."""
    z = _randn((M, D), "l2.%s.%d" % (kind, M))
    if kind == "ordinary":
        x = z
    elif kind == "over":
        x = 4000.0 * z
    elif kind == "subnormal":
        x = 1e-3 * z
        x[:, 5::32] = 25.0
    else:
        raise KeyError(kind)
    return h16(x)


# ------------------------------------------------------------------------------------------------ attention
ATT_SHAPES = ((8, 1), (8, 2), (1, 1))        # (heads, batch)
ATT_T = (1, 32, 33, 77, 96, 97, 288)         # 96: the last T of the 3-tile instantiation; 97 and 288 take the 9-tile one
ATT_REGIMES = ("flat", "peaked")
ATT_FP32_CASE = ("flat", 8, 2, 77)           # the one f16_round = 0 case, on the same strided buffer


ATT_GRID = 2.0 ** -5                         # q and k sit on this grid: every score is exact in fp32, in any summation order
TIE_MARGIN, P_FLOOR = 2.0 ** -19, 2.0 ** -20  # no probability >= P_FLOOR lies within TIE_MARGIN (relative) of an fp16 tie


def attention_case(regime, H, B, T):
    """The fused buffer [B*T][3*H*64] = (q | k | v) the tower hands to ds_attention_ex, fp16 grid.
    flat: q, k ~ N(0, 1): scores N(0, 1), |s| <= 8.  peaked: per (sample, head) a sign direction u; k_j = kappa_j u + noise with
    kappa_j ~ U(-2, 2), key 0 = 2 (u + noise) the sink; q_i = b_i u + noise, b_i ~ U(2.4, 3.5): the sink scores
    16 b_i = 38 .. 56, the other keys spread over +-56 with a few within a unit or two of the sink.

    The chain rounds twice before its output, and a rounding that sits on a tie falls either way under ANY fp32 evaluation: the
    bound of clip_reference.bound_report would then measure a coin, not the kernel.  So the intermediate roundings are made
    decidable: q and k lie on the 2^-5 grid (products are multiples of 2^-10 below 2^5, a head's 64 of them sum exactly in
    fp32), and a query row is drawn again, from the same seeded stream, while one of its float64 probabilities >= 2^-20 lies
    within 2^-19 (relative; about 30 fp32 roundings) of an fp16 tie.  tests/test_clip_host.py asserts both properties."""
    import clip_reference as R
    n = "att.%s.%d.%d.%d" % (regime, H, B, T)
    grid = lambda t: torch.round(t / ATT_GRID) * ATT_GRID
    gen = _g(n + ".q")
    k, v = [_randn((B, T, H, 64), n + "." + c) for c in "kv"]
    if regime == "peaked":
        u = (_rand((B, 1, H, 64), n + ".u") < 0.5).float() * 2 - 1
        kappa = _rand((B, T, H, 1), n + ".kappa") * 4 - 2
        kappa[:, 0] = 1.0
        k = kappa * u + 0.25 * k
        k[:, 0] *= 2.0
        draw = lambda: grid((2.4 + 1.1 * torch.rand((B, T, H, 1), generator=gen)) * u
                            + 0.25 * torch.randn((B, T, H, 64), generator=gen))
    elif regime == "flat":
        draw = lambda: grid(torch.randn((B, T, H, 64), generator=gen))
    else:
        raise KeyError(regime)
    k = grid(k)
    q = draw()
    pack = lambda: h16(torch.cat([t.reshape(B * T, H * 64) for t in (q, k, v)], dim=1)).contiguous()
    for _ in range(400):
        p, _keep = R.attention_probs(pack(), B, T, H, torch.float64)
        bad = ((R.tie_margin(p) < TIE_MARGIN) & (p >= P_FLOOR)).any(-1).transpose(1, 2)          # [B][T][H]
        if not bad.any():
            return pack()
        q = torch.where(bad[..., None], draw(), q)
    raise RuntimeError("no tie-free draw for %s" % n)


# ------------------------------------------------------------------------------------------------ GEMM, f16_round = 1
GEMM_ROWS = (1, 77, 154)
GEMM_FORMS = {"bias": (1536, 512, False, False), "gelu": (2048, 512, True, False),       # N, K, QuickGELU, residual
              "res512": (512, 512, False, True), "res2048": (512, 2048, False, True), "inf": (512, 512, False, True)}
GEMM_TILES = (-1, 0, 1, 2)                   # the default and every tile ds_gemm_force_tile accepts
INF_AT = (0, 100)                            # (row, column) of the output the "inf" form pushes past 65504


def gemm_case(form, M):
    """(A [M][K], W [N][K], bias [N], R [M][N] or None, act), fp16 grid.  A ~ N(0, 1) with column 9 x 300, W ~ N(0, 0.02)
    with row 33 x 8, the residual about 30.  "inf": row 0 of A is 16 and row 100 of W is 8 - 2^-7, so that bias + product is
    65472 exactly, finite in fp16, and the residual 64 carries it to 65536: only the rounding AFTER the residual add
    overflows."""
    N, K, act, res = GEMM_FORMS[form]
    n = "gemm.%s.%d" % (form, M)
    A = _randn((M, K), n + ".A")
    A[:, 9] *= 300.0
    W = 0.02 * _randn((N, K), n + ".W")
    W[33] *= 8.0
    bias = 0.1 * _randn((N,), n + ".b")
    R = 30.0 + _randn((M, N), n + ".R") if res else None
    if form == "inf":
        r, c = INF_AT
        A[r] = 16.0
        W[c] = 8.0 - 2.0 ** -7
        bias[c] = 0.0
        R[r, c] = 64.0
        assert math.isclose(float(A[r] @ W[c]), 65472.0)
    return h16(A), h16(W), h16(bias), (h16(R) if res else None), act


# ------------------------------------------------------------------------------------------------ the tower end to end
def tower_tokens():
    """i64[11][77]: the 8 golden captions (punctuation, an HTML entity, the truncated full-length one), 2 rows of
    synth_caption_tokens and one of those again with a negative id in its padding."""
    from conftest import golden
    from text_to_sound_synthesis_amd.synth import synth_caption_tokens
    extra = synth_caption_tokens(3, seed=11)
    extra[2, 40] = -1
    return torch.cat([golden("text_stage")["tokens"].long(), extra], 0)
