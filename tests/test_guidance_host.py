"""Classifier-free guidance, the parts that need no GPU:
  * the inputs of tests/test_hip_guidance.py are fair: on each of them the float32 and float64 restatements of the yardstick
    (tests/guidance_reference.py) agree in every kept set and every token, the smallest Gumbel gap is >= 1e-3 and the -70
    clamp is not reached -- so the yardstick itself excuses no column there;
  * at s = 0 / s = 1 the restatement gives the tokens of the plain oracle tail on zu / zc;
  * the float32 and float64 guided_loop chains of the GPU chain test agree on every recorded token with gap >= 1e-3;
  * DiffusionTransformer._guide: shape and broadcast rules of the null condition; DALLE.null_condition without a text stage;
  * condition dropout draws against a CPU generator."""
import pytest
import torch

import guidance_inputs as I
import guidance_reference as R
from text_to_sound_synthesis_amd import synth

NO_GRAD = True


@pytest.mark.parametrize("K", [256, 512])
@pytest.mark.parametrize("idx,trunc_k", [(0, None), (1, None), (2, None), (3, None), (0, 30)])
def test_tail_inputs_are_fair(K, idx, trunc_k):
    c = I.tail_case(K, idx, trunc_k)
    a, b = c["ref32"], c["ref64"]
    assert torch.equal(I.kept(a["trunc"]), I.kept(b["trunc"]))
    assert torch.equal(a["tokens"], b["tokens"])
    gap = min(float(a["gap"].min()), float(b["gap"].min()))
    assert gap >= 1e-3, gap
    assert float(b["log_pred"][:, :-1].min()) > -70.0 and float(a["log_pred"][:, :-1].min()) > -70.0
    d32 = float((a["log_pred"].double() - b["log_pred"]).abs().max())
    print("K=%d case %d: gap %.2e, min log-prob %.1f, d32 %.2e" % (K, idx, gap, float(b["log_pred"][:, :-1].min()), d32))
    assert 0.0 < d32 < 1e-4


@pytest.mark.parametrize("K", [256, 512])
def test_clamp_case_reaches_the_clamp(K):
    c = I.tail_case(K, 4)
    a, b = c["ref32"], c["ref64"]
    assert float(b["log_pred"][:, :-1].min()) == -70.0
    assert torch.equal(I.kept(a["trunc"]), I.kept(b["trunc"]))


@pytest.mark.parametrize("K", [256, 512])
def test_scale_zero_and_one_are_the_plain_tail(K):
    for idx in range(4):
        c = I.tail_case(K, idx)
        for s, z in ((0.0, c["zu"]), (1.0, c["zc"])):
            d = R.guided_step(c["sched"], c["zc"], c["zu"], s, c["log_z"], c["t"], c["u"], trunc_r=I.TRUNC_R)
            assert torch.equal(d["tokens"], R.plain_step(c["sched"], z, c["log_z"], c["t"], c["u"], I.TRUNC_R)), (idx, s)


@pytest.mark.parametrize("name", list(I.CHAINS))
def test_chain_inputs_are_fair(name):
    r32, g32 = I.chain_reference(name)
    r64, g64 = I.chain_reference(name, torch.float64)
    assert r32.shape[0] == (4 if I.CHAINS[name]["skip_step"] else I.T_CHAIN)
    assert torch.equal(r32, r64)
    assert min(g32, g64) >= 1e-3, (g32, g64)
    if I.CHAINS[name]["held"]:
        _, _, known, keep = I.chain_inputs()
        assert bool((r32[:, keep] == known[keep]).all()) and not keep.all(1).any()


def test_null_condition_shape_and_broadcast_rules():
    from text_to_sound_synthesis_amd.config import build_model, default_config
    m = build_model(default_config(n_layer=1))
    dt = m.transformer
    cond = synth.synth_cond_emb(3, key="guid.h.cond")
    null = synth.synth_cond_emb(3, key="guid.h.null")
    assert dt._guide(None, None, cond) is None and dt._guide(1.0, None, cond) is None and dt._guide(1, null, cond) is None
    n, s = dt._guide(3, null[0], cond)
    assert s == 3.0 and tuple(n.shape) == (3, 77, 512) and bool((n == null[0][None]).all())
    n, _ = dt._guide(0.0, null, cond)                      # s = 0 is a guided call (the null prediction), not the plain path
    assert torch.equal(n, null)
    for bad in (null[:2], null[0, :5], null[0, :, :8], null[None]):
        with pytest.raises(ValueError):
            dt._guide(3.0, bad, cond)
    with pytest.raises(ValueError):
        dt._guide(3.0, None, cond)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            dt._guide(bad, null, cond)
    # a model without a text stage takes the null embedding from the batch, and says so when it has neither
    assert m.condition_codec is None
    assert torch.equal(m.null_condition(batch={"null_condition_embed_token": null[0]}), null[0])
    with pytest.raises(ValueError, match="null_condition_embed_token"):
        m.null_condition()
    with pytest.raises(ValueError):
        m.null_condition("silence", batch={"null_condition_embed_token": null[0]})
    assert m._guidance({}, None, 1) == {} and m._guidance({}, 1.0, 2) == {}
    kw = m._guidance({"null_condition_embed_token": null[:2]}, 2.5, 3)
    assert kw["guidance_scale"] == 2.5 and tuple(kw["null_condition_embed"].shape) == (6, 77, 512)


class _Model:
    """what training_draws reads of the model"""
    class transformer:
        device = torch.device("cpu")
        num_classes, content_seq_len, num_timesteps = 257, 265, 100

        @staticmethod
        def sample_time(b, device, method, generator=None):
            t = torch.randint(0, 100, (b,), generator=generator)
            return t, torch.ones(b) / 100


def test_condition_dropout_draws():
    from text_to_sound_synthesis_amd.modeling import train
    B = 16
    x0 = synth.synth_tokens(B, mask_frac=0.0, key="guid.h.x0")
    cond = synth.synth_cond_emb(B, key="guid.h.dcond")
    null = synth.synth_cond_emb(1, key="guid.null")[0]
    gen = lambda: torch.Generator().manual_seed(11)
    g0, g1 = gen(), gen()
    base = train.training_draws(_Model, x0, cond, generator=g0)
    same = train.training_draws(_Model, x0, cond, generator=g1, cond_drop_prob=0.0, null_cond=null)
    assert all(torch.equal(a, b) for a, b in zip(base, same)) and same[1] is cond
    assert torch.equal(g0.get_state(), g1.get_state())                   # p = 0 makes no draw
    g2 = gen()
    full = train.training_draws(_Model, x0, cond, generator=g2, cond_drop_prob=1.0, null_cond=null)
    assert bool((full[1] == null[None]).all()) and all(torch.equal(a, b) for a, b in zip(base[2:], full[2:]))
    assert not torch.equal(g2.get_state(), g0.get_state())               # ... p > 0 one, after t and the noise
    g3 = gen()
    h1 = train.training_draws(_Model, x0, cond, generator=g3, cond_drop_prob=0.5, null_cond=null)
    h2 = train.training_draws(_Model, x0, cond, generator=gen(), cond_drop_prob=0.5, null_cond=null)
    assert torch.equal(h1[1], h2[1]) and torch.equal(g3.get_state(), g2.get_state())
    # the draw is the one a caller can reproduce: after t and the noise, torch.rand(B) < p
    g4 = gen()
    train.training_draws(_Model, x0, cond, generator=g4)
    drop = torch.rand(B, generator=g4) < 0.5
    assert bool(drop.any()) and not bool(drop.all())
    assert bool((h1[1][drop] == null[None]).all()) and torch.equal(h1[1][~drop], cond[~drop])
    with pytest.raises(ValueError):
        train.training_draws(_Model, x0, cond, generator=gen(), cond_drop_prob=0.5)
