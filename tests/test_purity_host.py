"""Host side of purity-prior sampling (no GPU): purity_plan, the sample_type mini-language, the argument rules, the drivers'
keywords, and the facts that make tests/purity_inputs.py fair inputs for tests/test_hip_purity.py -- the float32 and float64
restatements of the yardstick (tests/purity_reference.py) alone stay inside that test's caps, and the float32 one obeys the
exact invariants the kernels are held to."""
import inspect

import numpy as np
import pytest
import torch

import purity_inputs as I
import purity_reference as R
from conftest import golden
from text_to_sound_synthesis_amd import pipeline
from text_to_sound_synthesis_amd.modeling.dalle import DALLE
from text_to_sound_synthesis_amd.modeling.diffusion import purity_plan

NO_GRAD = True
L = 265


def schedule(T):
    return golden("schedule")["T%d_log_cumprod_ct" % T].numpy()


# ---- purity_plan ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [10, 100])
@pytest.mark.parametrize("S", [1, 2, 4, 10, 25, 100, 265])
def test_plan_counts_and_timesteps(S, T):
    lc = schedule(T)
    plan = purity_plan(S, L, lc)
    assert plan == R.plan(S, L, lc), "purity_plan differs from the yardstick's restatement of the rule"
    assert len(plan) == S
    remain = [L] + [r for _, r in plan]
    reveal = [a - b for a, b in zip(remain[:-1], remain[1:])]
    assert remain[-1] == 0 and sum(reveal) == L and min(reveal) >= 1 and max(reveal) - min(reveal) <= 1
    assert [r for _, r in plan] == [((S - 1 - k) * L) // S for k in range(S)]
    ts = [t for t, _ in plan]
    assert ts[0] == T - 1 and all(a >= b for a, b in zip(ts[:-1], ts[1:])) and min(ts) >= 0
    assert purity_plan(S, L, torch.from_numpy(lc)) == plan            # the model's buffer is a tensor


def test_plan_at_S_equal_T_on_the_shipped_schedule():
    """One might expect t_k = 99 - k for S = T = 100.  That does NOT hold for the shipped schedule, and the rule is
    kept: the schedule's expected [MASK] share exp(log_cumprod_ct[t]) rises linearly from 9e-6 at t = 0 to 0.9 (not 1) at
    t = 99, so the share (100 - k) / 100 that is still masked before step k is reached at t ~ 1.1 (99 - k) + 1.1: the plan
    stays at t = 99 for the first eleven steps, runs ahead of 99 - k throughout and ends at t = 1."""
    lc = schedule(100)
    plan = purity_plan(100, L, lc)
    gamma = np.exp(lc.astype(np.float64))[:100]
    assert abs(gamma[99] - 0.9) < 1e-6 and abs(gamma[0] - 9e-6) < 1e-9
    ts = [t for t, _ in plan]
    assert ts[:11] == [99] * 11 and ts[11] == 98 and ts[-1] == 1
    assert all(t >= 99 - k for k, t in enumerate(ts))
    assert sum(t == 99 - k for k, t in enumerate(ts)) == 1           # only k = 0
    # ... and each t_k is the nearest timestep to the share still masked (the rule, restated once more)
    remain = [L] + [r for _, r in plan]
    for k in range(1, 100):
        assert ts[k] == min(ts[k - 1], int(np.abs(gamma - remain[k] / L).argmin()))


def test_plan_ties_go_to_the_larger_timestep_and_errors():
    lc = np.log(np.array([0.25, 0.75, 0.75, 1e-30]))                 # T = 3; shares 0.25, 0.75, 0.75
    assert purity_plan(2, 4, lc) == [(2, 2), (2, 0)]                 # share 2/4 is as far from 0.25 as from 0.75: the larger t
    lc = np.log(np.array([0.2, 0.4, 0.6, 0.6, 0.9, 1e-30]))          # T = 5
    plan = purity_plan(5, 10, lc)                                    # shares before the steps: 1, .8, .6, .4, .2
    assert [t for t, _ in plan] == [4, 4, 3, 1, 0]                   # 0.8: 0.9 is nearest; 0.6: t = 2 and 3 tie -> 3
    for bad in (0, -1, L + 1):
        with pytest.raises(ValueError):
            purity_plan(bad, L, schedule(100))
    assert len(purity_plan(L, L, schedule(100))) == L


# ---- the mini-language and the argument rules -------------------------------------------------------------------------------------
def test_purity_part_of_the_sample_type():
    assert DALLE._purity_part("top0.85r") is None and DALLE._purity_part("top0.85r,fast3") is None
    assert DALLE._purity_part("top0.85r,q0.3") is None and DALLE._purity_part("normal") is None
    assert DALLE._purity_part("top0.85r,purity25") == (25, 0.0)
    assert DALLE._purity_part("top10p,purity4w1.5") == (4, 1.5)
    assert DALLE._purity_part("normal,purity100w0") == (100, 0.0)
    for bad in ("top0.85r,fast3,purity25", "top0.85r,purity25,fast3", "top0.85r,q0.3,purity25", "top0.85r,purity25,q0.3",
                "top0.85r,purity", "top0.85r,purityx", "top0.85r,purity4w", "top0.85r,purity4,purity5"):
        with pytest.raises(ValueError):
            DALLE._purity_part(bad)
    with pytest.raises(ValueError):
        DALLE._purity_part("top0.85r,purity25", keep_mode="renoise")
    assert pipeline.purity_sample_type("top0.85r", None, 3.0) == "top0.85r"
    assert pipeline.purity_sample_type("top0.85r", 25) == "top0.85r,purity25"
    assert DALLE._purity_part(pipeline.purity_sample_type("top0.85r", 8, 0.75)) == (8, 0.75)


def test_the_three_combinations_raise_before_anything_runs():
    """renoise, fast and q together with purity: ValueError on a machine without a GPU, i.e. before anything is enqueued"""
    from text_to_sound_synthesis_amd.config import build_model, default_config
    m = build_model(default_config(n_layer=1))
    tr = m.transformer
    cond = torch.zeros(2, 77, 512)
    batch = {"condition_embed_token": cond, "content_token": torch.zeros(2, L, dtype=torch.long)}
    keep = torch.zeros(2, L, dtype=torch.bool)
    for st in ("top0.85r,fast1,purity8", "top0.85r,q0.5,purity8"):
        with pytest.raises(ValueError):
            m.generate_content(batch=batch, filter_ratio=0, sample_type=st)
        with pytest.raises(ValueError):
            m.generate_long_content(batch=batch, windows=2, overlap_cols=13, sample_type=st)
    assert tr.repeat_rate is None and tr.truncation_r is None and not m.truncation_forward     # nothing was installed
    with pytest.raises(ValueError):
        m.inpaint_content(batch=batch, keep_mask=keep, keep_mode="renoise", sample_type="top0.85r,purity8")
    with pytest.raises(ValueError):
        m.generate_long_content(batch=batch, windows=2, overlap_cols=13, keep_mode="renoise", sample_type="top0.85r,purity8")
    kw = dict(condition_token=None, condition_mask=None, condition_embed=cond)
    with pytest.raises(ValueError):
        tr.sample_purity(steps=8, keep_mask=keep, keep_mode="renoise", content_token=batch["content_token"], **kw)
    tr.repeat_rate = 0.5
    with pytest.raises(ValueError):
        tr.sample_purity(steps=8, **kw)
    tr.repeat_rate = None
    for bad in (dict(steps=0), dict(steps=L + 1), dict(steps=8, purity_weight=-1.0), dict(steps=8, purity_weight=float("nan")),
                dict(steps=8, purity_weight=float("inf")), dict(steps=8, filter_ratio=0.5)):
        with pytest.raises(ValueError):
            tr.sample_purity(**dict(kw, **bad))


EXISTING = {        # the drivers' keywords before purity_steps / purity_weight, in order
    "generate_sample_with_condition": ["cond", "truncation_rate", "replicate", "fast", "caption_ids", "seed", "sample_rate",
                                       "guidance_scale", "negative_text"],
    "inpaint_audio": ["audio", "text", "spans", "keep_mode", "truncation_rate", "save_root", "audio_rate", "caption_ids", "seed",
                      "sample_rate", "guidance_scale", "negative_text"],
    "continue_audio": ["audio", "text", "keep_seconds", "keep_mode", "truncation_rate", "save_root", "audio_rate", "caption_ids",
                       "seed", "sample_rate", "guidance_scale", "negative_text"],
    "generate_long": ["text", "seconds", "overlap_seconds", "truncation_rate", "keep_mode", "caption_ids", "seed", "sample_rate",
                      "guidance_scale", "negative_text", "save_root"],
    "extend_audio": ["audio", "text", "seconds", "overlap_seconds", "truncation_rate", "keep_mode", "caption_ids", "seed",
                     "sample_rate", "guidance_scale", "negative_text", "save_root", "audio_rate"],
    "inference_generate_sample_with_condition": ["text", "truncation_rate", "save_root", "batch_size", "fast", "guidance_scale",
                                                 "negative_text"],
    "generate_sample": ["val_path", "truncation_rate", "save_root", "fast", "replicate", "sample_rate", "guidance_scale"],
}


PASTES = ["keep_original", "fade_seconds", "match_gain"]
KEYWORD_ONLY = {    # the drivers' keyword-only tails, written out in their def lines
    "generate_sample_with_condition": ["level"], "inpaint_audio": ["level"] + PASTES, "continue_audio": ["level"] + PASTES,
    "generate_long": ["joint", "level"], "extend_audio": ["joint", "level"] + PASTES,
    "inference_generate_sample_with_condition": ["level"], "generate_sample": ["level"],
}


@pytest.mark.parametrize("name", sorted(EXISTING))
def test_driver_keywords_come_after_the_existing_ones(name):
    fn = getattr(pipeline.Diffsound, name)
    every = list(inspect.signature(getattr(fn, "__wrapped__", fn)).parameters.values())[1:]
    ps = [p for p in every if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert [p.name for p in ps] == EXISTING[name] + ["purity_steps", "purity_weight"]
    assert ps[-2].default is None and ps[-1].default == 0.0
    assert [p.name for p in every[len(ps):]] == KEYWORD_ONLY[name]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in every[len(ps):])


def test_signatures_json_is_still_satisfied():
    import test_contract
    test_contract.test_boundary_signatures_match_reference()


# ---- the inputs are fair, and the float32 yardstick obeys the invariants ---------------------------------------------------------
@pytest.mark.parametrize("c", I.TAIL_CASES, ids=I.case_id)
def test_tail_inputs_are_fair(c):
    d = I.tail_case(c)
    r32, r64, K, x, remain = d["ref32"], d["ref64"], d["K"], d["x"], d["remain"]
    d_sharp, cand_margin, sel_margin, exc, exs = I.tail_margins(c)
    assert torch.equal(r32["sharp"] > -70.0, r64["sharp"] > -70.0), "the two restatements keep different classes"
    assert d_sharp < 1e-4
    if d["trunc_k"]:
        # no float32 tie at the top-k cut: which of two equal classes survives is the implementation's choice (the kernels keep
        # the smaller index, torch.topk does not say), so an input with one is no fair input
        srt = torch.sort(r32["log_pred"][:, :-1], dim=1, descending=True).values
        assert not bool((srt[:, d["trunc_k"] - 1] == srt[:, d["trunc_k"]]).any())
    # the caps of tests/test_hip_purity.py hold for the float32-float64 pair alone
    assert int(exc.sum()) * 200 <= exc.numel() and int(exs.sum()) * 50 <= exs.numel()
    assert torch.equal(r32["cand"][~exc], r64["cand"][~exc])
    ok = ~exs
    assert torch.equal(r32["reveal"][ok], r64["reveal"][ok])
    pos_ok = ok[:, None] & ~(exc & r64["reveal"])
    assert torch.equal(r32["tokens"][pos_ok], r64["tokens"][pos_ok])
    # the exact invariants, on the float32 restatement
    m = (x == K).sum(1)
    assert int(m[0]) == d["L"] and int(m[2]) <= remain < int(m[1])            # all-[MASK]; reveals; m <= R reveals nothing
    out = r32["tokens"]
    assert torch.equal((out == K).sum(1), torch.clamp(m, max=remain))
    assert torch.equal(out[x != K], x[x != K]) and torch.equal(out[2], x[2])
    assert bool((out[r32["reveal"]] < K).all()) and bool((r32["cand"] < K).all())
    if d["weight"] == 0.0 and d["trunc_k"] == 0 and d["trunc_r"] < 0 and d["zu"] is None:
        import diffsound_oracle as O
        assert torch.equal(r32["sharp"], O.predict_start(d["z"]))              # r = 0, no truncation: sh is predict_start


def test_reference_identity_and_full_reveal():
    c = I.TAIL_CASES[0]
    d = I.tail_case(c)
    K, x = d["K"], d["x"]
    kw = dict(trunc_r=I.TRUNC_R)
    full = R.purity_step(x, d["z"], d["u"], 0, 1.0, **kw)
    assert not bool((full["tokens"] == K).any()) and torch.equal(full["tokens"][x != K], x[x != K])
    same = R.purity_step(x, d["z"], d["u"], L, 1.0, **kw)
    assert torch.equal(same["tokens"], x) and not bool(same["reveal"].any())
    free = torch.randint(0, K, x.shape, generator=torch.Generator().manual_seed(1))
    assert torch.equal(R.purity_step(free, d["z"], d["u"], 0, 1.0, **kw)["tokens"], free)


@pytest.mark.parametrize("name", list(I.CHAINS))
def test_chain_inputs_are_fair(name):
    c = I.CHAINS[name]
    rec, cand_gap, sel_gap = I.chain_reference(name)
    assert cand_gap >= I.CHAIN_MIN_GAP and sel_gap >= I.CHAIN_MIN_GAP, (cand_gap, sel_gap)
    K, S = 256, c["S"]
    cond, null, known, keep = I.chain_inputs(name)
    plan = R.plan(S, L, schedule(I.T_CHAIN))
    free = (~keep if c["held"] else torch.ones_like(keep)).sum(1)
    for k, (_, r_k) in enumerate(plan):
        assert torch.equal((rec[k] == K).sum(1), torch.clamp(free, max=r_k))
    assert not bool((rec[-1] == K).any())
    if c["held"]:
        assert all(torch.equal(r[keep], known[keep]) for r in rec)
    for a, b in zip(rec[:-1], rec[1:]):                              # frozen once revealed
        assert torch.equal(b[a != K], a[a != K])
