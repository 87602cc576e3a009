"""The CLIP text tower (modeling/clip_text.py) and each kernel it calls against float64, off the initialiser manifold.

Kernel level (tests/clip_inputs.py, chains in tests/clip_reference.py): ds_embed_f16 must equal its exact chain; every other
kernel output k must hold, on every element,

    |k - y| <= ulp16(max(|k|, |y|)) / 2 + 4 * d32

with y the float64 evaluation of the kernel's documented rounding chain before its final rounding and d32 the largest distance
between the float32 and the float64 evaluation of that chain on the case; where y rounds to +-inf the kernel must give that inf.
tests/test_clip_host.py shows on the CPU that a variance that keeps the mean, a mask off by one, a lost 32-key tile and a
skipped residual rounding break this bound on the same cases.

End to end, on the "init" and the "trained_clip" profile (synth.py; last-layer scores up to 39, three hot channels, LayerNorm
gains over a decade): max |kernel - tower64| <= 4 * d16 and rms(kernel - tower64) <= 2 * rms(oracle - tower64), with d16 the
distance of stock torch's fp16 tower (oracle.clip_text_embed) from tower64, measured by the test itself.

Attention is the one chain that rounds twice before its output on values no input can pin down (the probabilities); its
operands are drawn so that those roundings are decidable (tests/clip_inputs.py: exact scores, no probability within 2^-19 of an
fp16 tie), so d32 there is accumulation error alone (1.6e-7 .. 1.2e-6) and the bound is half a spacing plus about 1e-6.

Measured on an MI355X (every test's docstring carries its own figures; "beyond" is the largest error in excess of the half
spacing, in units of d32, of which the bound allows 4): all 41 tests pass, no element outside the bound."""
import json
import os

import pytest
import torch

import clip_inputs as I
import clip_reference as R
import diffsound_oracle as O
from conftest import GOLDEN, parity_line
from text_to_sound_synthesis_amd import synth

pytestmark = pytest.mark.gpu
NO_GRAD = True          # tests/conftest.py: every test of this module runs under torch.no_grad()
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def L():
    from text_to_sound_synthesis_amd import _lib
    _lib.lib()
    return _lib


def _check(name, k, y64, y32):
    rep = R.bound_report(k.cpu(), y64, y32)
    print("%s: worst error / bound %.3f, beyond the half spacing %.2f d32, d32 %.3e, %.4f of the elements differ from the "
          "rounded float64 chain, %d outside" % (name, rep["worst"], rep["used"], rep["d32"], rep["differ"], rep["bad"]))
    return rep


# ------------------------------------------------------------------------------------------------ kernel level
def test_embed_is_exact(L):
    """ds_embed_f16 at M = 77, 154, 5 with ids 0, 49407 and a negative one: torch.equal with r16(r16(a) + r16(b))."""
    tab, pos = I.embed_tables()
    tc, pc = tab.cuda(), pos.cuda()
    for M in I.EMBED_ROWS:
        ids = I.embed_ids(M)
        out = torch.full((M + 1, I.WIDTH), float("nan"), device="cuda")                 # one guard row behind the output
        ic = ids.cuda()
        L.check(L.lib().ds_embed_f16(L.ptr(ic), L.ptr(tc), L.ptr(pc), L.ptr(out), M, I.EMBED_T, I.WIDTH, L.stream()))
        assert torch.equal(out[:M].cpu(), R.embed(tab, pos, ids, I.EMBED_T))
        assert torch.isnan(out[M]).all()


@pytest.mark.parametrize("kind", I.LN_KINDS)
def test_layernorm_f16(L, kind):
    """ds_layernorm_f16, D = 512 and 1024, M = 1, 3, 77, 155.  Measured, worst of the 8 shapes: beyond 0.27 (plain), 0.00 (hot),
    0.01 (offset), 0.00 (tight), 0.10 (gains), 0.11 (big); d32 2.2e-7 .. 4.9e-5; at most 3e-4 of the elements differ from the
    rounded float64 value."""
    worst = 0.0
    for D in I.LN_DIMS:
        for M in I.LN_ROWS:
            x, g, b = I.layernorm_case(kind, M, D)
            y = torch.full((M + 1, D), float("nan"), device="cuda")
            xc, gc, bc = x.cuda(), g.cuda(), b.cuda()
            L.check(L.lib().ds_layernorm_f16(L.ptr(xc), L.ptr(y), M, D, L.ptr(gc), L.ptr(bc), L.stream()))
            rep = _check("ds_layernorm_f16 %s M %d D %d" % (kind, M, D), y[:M], R.layernorm_pre(x, g, b, F64),
                         R.layernorm_pre(x, g, b, F32))
            assert rep["ok"], rep
            assert torch.isnan(y[M]).all()
            worst = max(worst, rep["used"])
    parity_line("ds_layernorm_f16 %s, 8 shapes: largest error beyond ulp16/2 = %.2f d32 (bound 4)" % (kind, worst))


@pytest.mark.parametrize("kind", I.L2_KINDS)
def test_l2norm_rows_f16(L, kind):
    """ds_l2norm_rows_f16, M = 1 and 77: ordinary rows; norm past 65504 (inf, quotients 0); quotients on the subnormal grid.
    Measured: beyond 0.00 in all three kinds; "over" is 0 everywhere, every "subnormal" quotient is a non-zero multiple of 2^-24 or
    a correctly rounded 0, and no element differs from the rounded float64 value."""
    worst = 0.0
    for M in I.L2_ROWS:
        x = I.l2norm_case(kind, M)
        y = torch.full((M + 1, I.WIDTH), float("nan"), device="cuda")
        xc = x.cuda()
        L.check(L.lib().ds_l2norm_rows_f16(L.ptr(xc), L.ptr(y), M, I.WIDTH, L.stream()))
        y64 = R.l2norm_pre(x, F64)
        rep = _check("ds_l2norm_rows_f16 %s M %d" % (kind, M), y[:M], y64, R.l2norm_pre(x, F32))
        assert rep["ok"], rep
        assert torch.isnan(y[M]).all()
        out = y[:M].cpu().double()
        if kind == "over":
            assert (out == 0).all()
        if kind == "subnormal":
            small = y64.abs() < 2.0 ** -14
            assert (out[small] != 0).float().mean() > 0.5                               # not flushed ...
            assert torch.equal(out[small] / 2.0 ** -24, torch.round(out[small] / 2.0 ** -24))       # ... and on the 2^-24 grid
        worst = max(worst, rep["used"])
    parity_line("ds_l2norm_rows_f16 %s: largest error beyond ulp16/2 = %.2f d32 (bound 4)" % (kind, worst))


def _attention(L, qkv, B, T, H, f16):
    D = H * 64
    buf = qkv.cuda()
    out = torch.full((B * T + 1, D), float("nan"), device="cuda")
    p = buf.data_ptr()
    L.check(L.lib().ds_attention_ex(p, 3 * D, p + 4 * D, 3 * D, p + 8 * D, 3 * D, L.ptr(out), D, B, H, T, T, 0.125, 1, f16,
                                    L.stream()))
    assert torch.isnan(out[B * T]).all()
    return out[:B * T]


@pytest.mark.parametrize("regime", I.ATT_REGIMES)
@pytest.mark.parametrize("H,B", I.ATT_SHAPES)
def test_causal_attention_f16(L, regime, H, B):
    """ds_attention_ex(causal = 1, f16_round = 1) on the fused QKV buffer, T = 1, 32, 33, 77, 96, 97, 288.
    Measured over the 42 cases: beyond 0.00 .. 0.54, d32 1.6e-7 .. 1.2e-6, at most 9e-4 of the elements differ from the rounded
    float64 chain (each by one fp16 spacing, the final rounding falling the other way)."""
    for T in I.ATT_T:
        qkv = I.attention_case(regime, H, B, T)
        out = _attention(L, qkv, B, T, H, 1)
        rep = _check("ds_attention_ex %s H %d B %d T %d" % (regime, H, B, T), out, R.attention_pre(qkv, B, T, H, F64),
                     R.attention_pre(qkv, B, T, H, F32))
        parity_line("ds_attention_ex causal f16 %s H %d B %d T %d: %.4f of the elements differ from the float64 chain, "
                    "largest error beyond ulp16/2 = %.2f d32 (bound 4)" % (regime, H, B, T, rep["differ"], rep["used"]))
        assert rep["ok"], rep


def test_causal_attention_fp32_on_the_strided_buffer(L):
    """f16_round = 0 on the same fused buffer (H 8, B 2, T 77): within 4 * d32 + one fp32 rounding of the float64 value.
    Measured: max error 4.1e-7, d32 3.6e-7."""
    regime, H, B, T = I.ATT_FP32_CASE
    qkv = I.attention_case(regime, H, B, T)
    out = _attention(L, qkv, B, T, H, 0).cpu().double()
    y64 = R.attention_pre(qkv, B, T, H, F64, f16=False)
    d32 = float((R.attention_pre(qkv, B, T, H, F32, f16=False).double() - y64).abs().max())
    err = (out - y64).abs()
    parity_line("ds_attention_ex causal fp32 on the fused buffer: max error %.3e, d32 %.3e" % (float(err.max()), d32))
    assert (err <= 4 * d32 + 2.0 ** -24 * y64.abs()).all()


@pytest.mark.parametrize("tile", I.GEMM_TILES)
@pytest.mark.parametrize("form", list(I.GEMM_FORMS))
def test_gemm_f16_round(L, form, tile):
    """ds_gemm(f16_round = 1) at the tower's shapes, M = 1, 77, 154, under every block tile: bias only, bias + QuickGELU, bias +
    residual written in place (K = 512 and 2048), and one output carried past 65504 by the residual add.
    Measured, the same under all four tile settings: beyond 0.45 (bias), 1.00 (gelu), 1.00 (res512), 1.75 (res2048), 1.50 (inf); the
    overflowing output is +inf and the only inf.  d32 is 3e-5 (bias) and 7.8e-3 .. 2.0 in the forms that round before their last
    op: there it is one fp16 spacing of an intermediate that the float32 chain itself rounds the other way."""
    N, K, _, _ = I.GEMM_FORMS[form]
    worst = 0.0
    for M in I.GEMM_ROWS:
        A, W, bias, Rs, act = I.gemm_case(form, M)
        x = (Rs.cuda() if Rs is not None else torch.full((M, N), float("nan"), device="cuda"))
        L.lib().ds_gemm_force_tile(tile)
        try:
            L.gemm(A.cuda(), W.cuda(), x, M, N, K, bias=bias.cuda(), R=x if Rs is not None else None,
                   act=L.ACT_GELU2 if act else L.ACT_NONE, f16_round=1)
        finally:
            L.lib().ds_gemm_force_tile(-1)
        y64 = R.gemm_pre(A, W, bias, F64, act, Rs)
        rep = _check("ds_gemm f16 %s tile %d M %d" % (form, tile, M), x, y64, R.gemm_pre(A, W, bias, F32, act, Rs))
        assert rep["ok"], rep
        if form == "inf":
            assert float(x[I.INF_AT]) == float("inf") and int(torch.isinf(x).sum()) == 1
        worst = max(worst, rep["used"])
    parity_line("ds_gemm f16_round %s tile %d: largest error beyond ulp16/2 = %.2f d32 (bound 4)" % (form, tile, worst))


# ------------------------------------------------------------------------------------------------ the tower
def clip_sd(profile):
    with open(os.path.join(GOLDEN, "state_dict_keys_clip.json")) as f:
        return synth.synth_state_dict(json.load(f), 0, profile)


_TOWER = {}


def tower(profile):
    """Kernel output, tower64 and the fp16 oracle on the 11 token rows, computed once per profile."""
    if profile not in _TOWER:
        from text_to_sound_synthesis_amd.config import build_model, default_config
        sd, tok = clip_sd(profile), I.tower_tokens()
        m = build_model(default_config(n_layer=1, with_clip=True))
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected
        emb = m.transformer.condition_emb.cuda().eval()
        _TOWER[profile] = {"tok": tok, "out": emb(tok.cuda()).cpu().double(), "alone": emb(tok[:1].cuda()).cpu().double(),
                           "y": R.tower64(sd, tok), "o16": O.clip_text_embed(sd, tok).double()}
    return _TOWER[profile]


def _rms(t):
    return float(t.pow(2).mean().sqrt())


@pytest.mark.parametrize("profile", ["init", "trained_clip"])
def test_tower_vs_float64(profile):
    """11 token rows (8 golden captions, 2 synthetic, one with a negative id).  Measured, kernel / stock fp16: init max 3.71e-4 / 4.10e-4, rms 4.26e-5 / 4.23e-5 (largest entry 0.150); trained_clip max
    2.71e-3 / 1.90e-3, rms 6.26e-5 / 5.91e-5 (largest entry 0.657)."""
    t = tower(profile)
    assert int(t["tok"].min()) < 0 and t["out"].shape == (11, 77, 512)
    d16, dk = float((t["o16"] - t["y"]).abs().max()), float((t["out"] - t["y"]).abs().max())
    r16, rk = _rms(t["o16"] - t["y"]), _rms(t["out"] - t["y"])
    parity_line("CLIP text tower vs float64, %s: kernel max %.3e rms %.3e; stock fp16 (d16) max %.3e rms %.3e; largest "
                "entry %.3f" % (profile, dk, rk, d16, r16, float(t["y"].abs().max())))
    assert torch.isfinite(t["out"]).all() and torch.isfinite(t["o16"]).all()
    assert dk <= 4 * d16
    assert rk <= 2 * r16
    assert (t["out"].norm(dim=-1) - 1).abs().max() < 2e-3


@pytest.mark.parametrize("profile", ["init", "trained_clip"])
def test_caption_alone_vs_in_the_batch(profile):
    """Caption 0 run alone holds the same bound as in the batch of 11.  Measured: init 3.29e-4, trained_clip 1.84e-3; bit-equal to the same
    caption in the batch on both profiles."""
    t = tower(profile)
    d16 = float((t["o16"] - t["y"]).abs().max())
    da = float((t["alone"][0] - t["y"][0]).abs().max())
    same = torch.equal(t["alone"][0], t["out"][0])
    parity_line("CLIP text tower, %s: caption 0 alone vs float64 %.3e (4 d16 = %.3e); alone and in the batch of 11 are %s"
                % (profile, da, 4 * d16, "bit-equal" if same else
                   "not bit-equal (max %.3e)" % float((t["alone"][0] - t["out"][0]).abs().max())))
    assert da <= 4 * d16
    assert _rms(t["alone"][0] - t["y"][0]) <= 2 * _rms(t["o16"][0] - t["y"][0])
