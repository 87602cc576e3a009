"""Which edges of the un-scaled fp16 split the denoiser's real operands reach (CPU only).

The f16x2 kernels split an activation a into fp16(a) + fp16(a - fp16(a)) without scaling it: fp32-class for |a| in about
[2^-3, 65504]; below 2^-3 the lo plane is subnormal (2^-25 of absolute precision), above 65504 the split saturates
(csrc/gemm_f16x2.hip).  The oracle records (max, median) of |operand| at every such site of the transformer -- the A operands of
the seven GEMMs of a block and of the logits GEMM, and q, k, v and the pre-softmax scores of both attentions -- on the 2-layer
initialiser-like weights and on the 19-layer trained-like profile behind tests/test_hip_trained_like.py.  The table is in
DESIGN.md section 4.2; tests/test_hip_denoiser_range.py holds the kernels to their error model on both sides of 2^-3."""
import pytest
import torch

import diffsound_oracle as O
from conftest import synth_sd
from text_to_sound_synthesis_amd import synth

SPLIT_LIMIT = 65504.0
HEADROOM = 2.0 ** 3
# site -> True: the median |operand| sits above 2^-3 in every block of both weight sets, False: below it in every block
MEDIAN_ABOVE = {"attn1.qkv": True, "attn1.q": True, "attn1.k": True, "attn1.v": True, "attn1.scores": True, "attn1.proj": True,
                "attn2.query": True, "attn2.kv": False, "attn2.q": True, "attn2.k": False, "attn2.v": False,
                "attn2.scores": False, "attn2.proj": False, "mlp.0": True, "mlp.2": True, "to_logits.1": True}
# The sites that the product guards at run time, so that they need not keep the factor 2^3 by themselves: FC2's operand, the GELU2
# outputs (Text2ImageTransformer.range_exceeded; tests/test_hip_denoiser_range.py test_denoiser_range_guard runs the guard)
GUARDED = {"mlp.2"}


def _record(n_layer, profile, tok_key, cond_key, mask_frac, ts):
    sd = synth_sd("dalle", n_layer, profile=profile)
    tok = synth.synth_tokens(2, mask_frac=mask_frac, key=tok_key)
    cond = synth.synth_cond_emb(2, key=cond_key)
    rec = {}
    with torch.no_grad():
        logits = O.transformer_forward(sd, tok, cond, torch.tensor(ts), record=rec)
        if n_layer == 2:
            assert torch.equal(logits, O.transformer_forward(sd, tok, cond, torch.tensor(ts)))      # recording changes nothing
    sites = {}
    for k, v in rec.items():
        site = k.split(".blocks.")[1].split(".", 1)[1] if ".blocks." in k else k.rsplit("transformer.", 1)[1]
        sites.setdefault(site, []).append(v)
    assert set(sites) == set(MEDIAN_ABOVE) and all(len(v) == (1 if s == "to_logits.1" else n_layer) for s, v in sites.items())
    return sites


@pytest.mark.parametrize("n_layer,profile,tok_key,cond_key,mask_frac,ts", [
    (2, "init", "tf2.tokens", "tf2.cond", 0.3, [37, 80]),            # the inputs of the 2-layer logits golden
    (19, "trained", "tl19.tokens", "tl19.cond", 0.5, [63, 7]),       # the inputs of tests/test_hip_trained_like.py
])
def test_denoiser_split_operands_reach_which_edges(n_layer, profile, tok_key, cond_key, mask_frac, ts):
    """Per site, over the blocks: the largest |operand| keeps a factor 2^3 to 65504, and the median sits on the side of 2^-3 that
    MEDIAN_ABOVE names, in every block.

    Measured: the whole cross-attention K / V side runs BELOW 2^-3 -- the l2-normalised caption embedding (median 0.030, max
    0.22), the K and V it projects to (median 0.019 / 0.07), the scores (0.014 / 0.06) and the attention output that feeds
    attn2.proj (0.013 / 0.07) -- so those three GEMMs and the cross-attention work in the 2^-25-absolute regime of the split, not
    the fp32-class one.  Everything else has its median above 2^-3 (0.14 .. 0.7).
    One site does not keep the factor 2^3: FC2's operand (the GELU2 outputs) reaches 1.44e4 = 65504 / 4.5 on the trained-like
    weights, by construction of that profile (2.7 on the initialiser-like ones).  That site is guarded at run time, and only a
    guarded site may come that close: it must still be below 65504 here, and the weights-only bound that switches the guard's
    monitor on (gelu2_operand_bound x 2^3 > 65504) must hold for the recorded maximum of every block, so that the monitor is on
    wherever the site is within 2^3."""
    from text_to_sound_synthesis_amd.modeling.transformer import RANGE_HEADROOM, SPLIT_LIMIT as LIMIT, gelu2_operand_bound
    assert (RANGE_HEADROOM, LIMIT) == (HEADROOM, SPLIT_LIMIT)
    sites = _record(n_layer, profile, tok_key, cond_key, mask_frac, ts)
    for site, v in sites.items():
        mx, md_lo, md_hi = max(a for a, _ in v), min(b for _, b in v), max(b for _, b in v)
        print("%-13s max %9.3g   median %.3g .. %.3g" % (site, mx, md_lo, md_hi))
        assert mx < SPLIT_LIMIT, site
        if site not in GUARDED:
            assert mx * HEADROOM <= SPLIT_LIMIT, site
        if MEDIAN_ABOVE[site]:
            assert md_lo > 2.0 ** -3, site
        else:
            assert md_hi < 2.0 ** -3, site
    sd = synth_sd("dalle", n_layer, profile=profile)
    monitored = False
    for l, (mx, _) in enumerate(sites["mlp.2"]):
        pfx = "transformer.transformer.blocks.%d." % l
        bound = gelu2_operand_bound(sd[pfx + "mlp.0.weight"], sd[pfx + "mlp.0.bias"], sd[pfx + "ln2.weight"], sd[pfx + "ln2.bias"])
        print("block %2d: FC2 operand max %9.3g, weights-only bound %9.3g" % (l, mx, bound))
        assert mx <= bound
        monitored |= bound * HEADROOM > SPLIT_LIMIT
    assert monitored == (profile == "trained")          # (off on the initialiser-like weights: nothing is paid there)
