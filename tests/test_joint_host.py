"""Joint-window sampling, host side (no GPU):
  * pipeline.joint_map / joint_canvas_cols / joint_window_positions against a brute-force enumeration of every window's columns
    (tests/joint_reference.py: cover) for every n in 1 .. 26, W in {1, 2, 3, 16}, line and ring: every column covered once or
    twice, the two weights summing to 1, the ring's wrap;
  * loop_plan's edges and loop_cut, the rate rule of generate_loop, as a pure function;
  * the inputs of tests/test_hip_joint.py are fair: on every tail case the float32 twin of the yardstick against its float64
    form differs in the kept sets of at most 1 column in 200 and only where the cut is within 4e-7 of r, and agrees on every
    token elsewhere (the rules of tests/test_hip_guidance.py); the chains' twins agree on every token with a Gumbel gap >= 1e-3;
  * one window, and a position under one window, are the plain / guided yardsticks themselves;
  * every rejected argument of the joint entries returns -1 and names the entry before any HIP call."""
import numpy as np
import pytest
import torch

import diffsound_oracle as O
import guidance_reference as G
import joint_inputs as I
import joint_reference as R
from text_to_sound_synthesis_amd import audio, pipeline

NO_GRAD = True


# ---- geometry --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("W", [1, 2, 3, 16])
def test_joint_map_against_enumeration(W, ring):
    for n in range(1, 27):
        if ring and W < 2:
            with pytest.raises(ValueError):
                pipeline.joint_map(W, n, ring)
            continue
        cov = R.cover(W, n, ring)
        m = pipeline.joint_map(W, n, ring)
        C, h = len(cov), 53 - n
        assert m["columns"] == C == pipeline.joint_canvas_cols(W, n, ring) == (W * h if ring else 53 + (W - 1) * h)
        fade = audio.fade_table(n).numpy()
        assert torch.equal(audio.fade_table(n), R.fade(n))
        assert np.all((fade > 0) & (fade < 1)) and np.allclose(fade + fade[::-1], 1.0, atol=1e-7)
        seen = np.zeros((W, 53), dtype=int)
        for c in range(C):
            w1, o1 = cov[c][0]
            assert (int(m["later"][c]), int(m["later_offset"][c])) == (w1, o1)
            seen[w1, o1] += 1
            if len(cov[c]) == 2:
                w0, o0 = cov[c][1]
                assert (int(m["earlier"][c]), int(m["earlier_offset"][c])) == (w0, o0) and w0 == (w1 - 1) % W
                assert m["weight"][c] == fade[o1] and 0.0 < m["weight"][c] < 1.0
                assert abs(float(np.float32(1.0) - m["weight"][c]) + float(m["weight"][c]) - 1.0) < 1e-7
                seen[w0, o0] += 1
            else:
                assert int(m["earlier"][c]) == -1 and int(m["earlier_offset"][c]) == -1 and m["weight"][c] == 1.0
        assert np.all(seen == 1)                                   # every (window, offset) lies on exactly one column
        two = sum(len(v) == 2 for v in cov)
        assert two == (W * n if ring else (W - 1) * n)
        if ring:                                                   # the wrap: the last window's tail is the first window's head
            for o in range(n):
                assert cov[o] == [(0, o), (W - 1, o + h)]
        pos = pipeline.joint_window_positions(W, n, ring)
        assert torch.equal(pos, R.window_positions(W, n, ring))
    assert 5 * pipeline.joint_canvas_cols(16, 1, False) == 4165


def test_geometry_errors():
    for bad in ((0, 13, False), (1, 13, True), (3, 0, False), (3, 27, False), (-1, 5, True)):
        with pytest.raises(ValueError):
            pipeline.joint_canvas_cols(*bad)


# ---- loops -----------------------------------------------------------------------------------------------------------------
def test_loop_plan_edges():
    assert pipeline.loop_plan(10.03) == (2, 13, 80, 80 * 4096)                       # 54 columns asked, two windows of hop 40
    with pytest.raises(ValueError):
        pipeline.loop_plan(53 * 4096 / 22050)                                        # fits one window: no ring under 54 columns
    with pytest.raises(ValueError):
        pipeline.loop_plan(5.0)
    h = 40
    exact = 3 * h * 4096 / 22050                                                     # a multiple of the hop: made as asked
    assert pipeline.loop_plan(exact) == (3, 13, 120, 120 * 4096)
    assert pipeline.loop_plan((3 * h * 4096 + 1) / 22050) == (4, 13, 160, 160 * 4096)   # one sample over: snaps up a hop
    assert pipeline.loop_plan((2 * h * 4096 + 1) / 22050, 0.1) == (2, 1, 104, 104 * 4096)
    assert pipeline.loop_plan(16 * h * 4096 / 22050)[0] == 16
    with pytest.raises(ValueError, match="17 windows"):
        pipeline.loop_plan((16 * h * 4096 + 1) / 22050)
    with pytest.raises(ValueError):
        pipeline.loop_plan(20.0, overlap_seconds=6.0)
    W, n, C, samples = pipeline.loop_plan(33.3)
    assert C == W * (53 - n) and samples == 4096 * C and samples >= round(33.3 * 22050) > 4096 * (C - (53 - n))


def test_loop_cut_rate_rule():
    assert pipeline.loop_cut(80, 40) == (2 * 40 * 4096, 80 * 4096)
    assert pipeline.loop_cut(80, 40, 22050) == pipeline.loop_cut(80, 40)
    assert pipeline.loop_cut(80, 40, 44100) == (4 * 40 * 4096, 160 * 4096)
    assert pipeline.loop_cut(104, 52, 11025) == (52 * 4096, 52 * 4096)
    for C, h in ((80, 40), (104, 52), (147, 49)):
        with pytest.raises(ValueError, match="period of %d samples" % (C * 4096)):
            pipeline.loop_cut(C, h, 48000)
    with pytest.raises(ValueError):
        pipeline.loop_cut(80, 40, 16000)
    # exactness: whole samples at the output rate, in the ratio of the rates
    for rate in (44100, 11025, 88200):
        off, per = pipeline.loop_cut(120, 40, rate)
        assert off * 22050 == 2 * 40 * 4096 * rate and per * 22050 == 120 * 4096 * rate


# ---- the yardstick's own identities ----------------------------------------------------------------------------------------
def test_one_window_is_the_plain_and_the_guided_yardstick():
    K, B = 256, 2
    g = torch.Generator().manual_seed(5)
    zc, zu = torch.randn(B, 1, K, I.L, generator=g) * 4, torch.randn(B, 1, K, I.L, generator=g) * 4
    xt = torch.randint(0, K + 1, (B, I.L), generator=g)
    u = torch.rand(B, K + 1, I.L, generator=g)
    t = torch.tensor([40, 7])
    sched, log_z = O.make_schedule(100, K + 1), O.log_onehot(xt, K + 1)
    a = R.joint_step(sched, zc, None, 0.0, 1, 13, False, log_z, t, u)
    assert torch.equal(a["tokens"], G.plain_step(sched, zc[:, 0], log_z, t, u))
    b = R.joint_step(sched, zc, zu, 3.0, 1, 13, False, log_z, t, u)
    want = G.guided_step(sched, zc[:, 0], zu[:, 0], 3.0, log_z, t, u)
    assert torch.equal(b["tokens"], want["tokens"]) and torch.equal(b["log_pred"], want["log_pred"])


def test_positions_under_one_window_carry_that_windows_prediction():
    c = I.tail_case(256, 13, False)
    lw = O.predict_start(c["zc"].flatten(0, 1)).view(c["B"], c["W"], 257, I.L)
    cov = R.cover(c["W"], 13, False)
    lp = c["ref32"]["log_pred"]
    for col in (0, 39, 53, 79, 132):
        assert len(cov[col]) == 1
        w, o = cov[col][0]
        assert torch.equal(lp[:, :, 5 * col:5 * col + 5], lw[:, w, :, 5 * o:5 * o + 5])
    col = 40                                                       # under windows 0 and 1: the guided mix at scale fade[0]
    (w1, o1), (w0, o0) = cov[col]
    mix = G.guided_log_pred(lw[:, w1, :, 5 * o1:5 * o1 + 5], lw[:, w0, :, 5 * o0:5 * o0 + 5], float(R.fade(13)[o1]))
    assert torch.equal(lp[:, :, 5 * col:5 * col + 5], mix)


# ---- fairness of the GPU tests' inputs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,n,ring,trunc_k,guided", I.TAIL_CASES)
def test_tail_inputs_are_fair(K, n, ring, trunc_k, guided):
    c = I.tail_case(K, n, ring, trunc_k, guided)
    a, b = c["ref32"], c["ref64"]
    same = (I.kept(a["trunc"]) == I.kept(b["trunc"])).all(1)
    if not bool(same.all()):
        assert not trunc_k, "top-k kept sets of the twin differ in %d columns" % int((~same).sum())
        assert bool(I.near_cut(b)[~same].all()), "the twin's kept sets differ where the cut is not within 4e-7 of r"
        assert int((~same).sum()) * 200 <= same.numel()
    assert torch.equal(a["tokens"][same], b["tokens"][same]), "%d tokens differ" % int((a["tokens"] != b["tokens"])[same].sum())
    d32 = float((a["log_pred"].double() - b["log_pred"]).abs().max())
    assert 0 < d32 < 1e-5
    assert int((c["xt"] == K).sum()) > 0                           # the canvas holds [MASK] and revealed positions
    assert c["t"][0] != c["t"][1]


@pytest.mark.parametrize("name", list(I.CHAINS))
def test_chain_inputs_are_fair(name):
    a, gap_a = I.chain_reference(name, torch.float32)
    b, gap_b = I.chain_reference(name, torch.float64)
    assert torch.equal(a, b), "%d tokens differ between the float32 and the float64 chain" % int((a != b).sum())
    assert min(gap_a, gap_b) >= 1e-3, (gap_a, gap_b)
    c = I.CHAINS[name]
    pos = R.window_positions(c["W"], c["n"], c["ring"])
    assert int(a[-1].max()) < 256                                  # no [MASK] left
    if c["held"]:
        _, _, known, keep = I.chain_inputs(name)
        assert torch.equal(a[-1][keep], known[keep])
    assert tuple(a[-1][:, pos].shape) == (2, c["W"], 265)


# ---- argument checks: -1, the entry named, no HIP call ---------------------------------------------------------------------
_PTR = 4096
_TAIL_U = "logits logits_u canvas t u sched out dbg dbg dbg B W n ring fade lrows K T initial trunc_r trunc_k scale keep known " \
          "mode stream"
_TAIL_R = "logits logits_u canvas t gids seed call sched out dbg dbg dbg B W n ring fade lrows K T initial trunc_r trunc_k scale " \
          "keep known mode stream"
_STEP_U = "h canvas_in t t_post kv u B W n ring n_cond fade initial trunc_r trunc_k scale keep known mode tokensN workspace " \
          "canvas_out stream"
_STEP_R = "h canvas_in t t_post kv gids seed call B W n ring n_cond fade initial trunc_r trunc_k scale keep known mode tokensN " \
          "workspace canvas_out stream"
_CHAIN = "h canvas canvas_tmp t_steps n_calls kv gids seed call B W n ring n_cond fade initial trunc_r trunc_k scale keep known " \
         "mode tokensN workspace stream"
_ENTRIES = {"ds_sample_tail_joint": _TAIL_U, "ds_sample_tail_joint_rng": _TAIL_R, "ds_denoiser_step_joint": _STEP_U,
            "ds_denoiser_step_joint_rng": _STEP_R, "ds_denoiser_sample_joint_rng": _CHAIN}
_VALID = dict(B=2, W=3, n=13, ring=0, n_cond=2, lrows=265, K=256, T=100, initial=0, trunc_r=-1.0, trunc_k=0, scale=3.0, seed=7,
              call=0, mode=0, n_calls=3, stream=None, dbg=None, t_post=None, keep=None, known=None)


def test_joint_entries_reject_bad_arguments_before_any_hip_call():
    import ctypes as C

    from text_to_sound_synthesis_amd import _lib as Lb
    lib = Lb.lib()
    assert sorted(set(_ENTRIES) | {"ds_joint_gather"}) == sorted(Lb._PROTOS_JOINT) and set(Lb._PROTOS_JOINT) <= set(Lb.EXPORTED)
    d = Lb.DenoiserDesc()
    d.n_layer, d.n_embd, d.n_head, d.seq_len, d.cond_len, d.cond_dim = 2, 1024, 16, 265, 77, 512
    d.n_codes, d.n_steps, d.mlp_mult = 256, 100, 4
    dummy = torch.zeros(64)
    for f in ("tok_emb", "pos_emb", "lnf_g", "lnf_b", "w_logits", "b_logits", "sched"):
        setattr(d, f, dummy.data_ptr())
    n = 2 * Lb.LP_COUNT
    ptrs = (C.c_void_p * n)(*([dummy.data_ptr()] * n))
    h = C.c_void_p()
    Lb.check(lib.ds_denoiser_create(C.byref(d), ptrs, C.byref(h)))
    problems, total = [], 0
    try:
        for name, spec in _ENTRIES.items():
            names = spec.split()
            assert len(names) == len(Lb._PROTOS_JOINT[name][1]), name
            tail = name.startswith("ds_sample_tail")
            cases = [dict(W=0), dict(W=-2), dict(n=0), dict(n=27), dict(ring=1, W=1), dict(W=300, n=1), dict(fade=None),
                     dict(mode=1), dict(mode=1, keep=_PTR, known=_PTR), dict(mode=2), dict(keep=_PTR, known=None),
                     dict(trunc_k=5, trunc_r=0.85), dict(trunc_k=-1), dict(scale=float("nan")), dict(scale=float("inf")),
                     dict(u=None) if "u" in names else dict(gids=None), dict(B=0)]
            if tail:
                cases += [dict(lrows=264), dict(K=300), dict(T=0), dict(logits=None), dict(canvas=None), dict(t=None),
                          dict(sched=None), dict(out=None)]
            else:
                cases += [dict(h=None), dict(kv=None), dict(workspace=None), dict(tokensN=None), dict(n_cond=0), dict(n_cond=3)]
                cases += [dict(canvas=None), dict(t_steps=None), dict(n_calls=-1)] if "t_steps" in names else \
                    [dict(canvas_in=None), dict(t=None), dict(canvas_out=None)]
            for over in cases:
                vals = dict(_VALID, h=h)
                vals.update(over)
                rc = getattr(lib, name)(*[vals.get(p, _PTR) for p in names])
                msg = lib.ds_last_error_string().decode()
                total += 1
                if rc != -1 or (name + ":") not in msg:
                    problems.append("%s %r -> rc %d, %r" % (name, over, rc, msg))
        for over in (dict(W=0), dict(n=27), dict(ring=1, W=1), dict(copies=0), dict(copies=3), dict(canvas=None), dict(win=None),
                     dict(B=0)):
            vals = dict(canvas=_PTR, win=_PTR, B=2, W=3, n=13, ring=0, copies=1, stream=None)
            vals.update(over)
            rc = lib.ds_joint_gather(*[vals[p] for p in "canvas win B W n ring copies stream".split()])
            total += 1
            if rc != -1 or "ds_joint_gather:" not in lib.ds_last_error_string().decode():
                problems.append("ds_joint_gather %r -> rc %d" % (over, rc))
    finally:
        lib.ds_denoiser_destroy(h)
    assert not problems, "\n".join(problems)
    assert total > 100


# ---- the Python surface's rules (no GPU: they are checked before anything runs) -------------------------------------------
def test_signatures():
    import inspect
    from text_to_sound_synthesis_amd.modeling.dalle import DALLE
    from text_to_sound_synthesis_amd.modeling.diffusion import DiffusionTransformer
    p = inspect.signature(DiffusionTransformer.sample_joint).parameters
    assert list(p)[1:5] == ["condition_embed", "windows", "overlap_cols", "ring"]
    for k in ("skip_step", "caption_ids", "seed", "keep_mask", "content_token", "guidance_scale", "null_condition_embed", "noise_fn"):
        assert k in p
    p = inspect.signature(DALLE.generate_long_content).parameters
    assert p["joint"].default is False and p["ring"].default is False
    for name in ("generate_long", "extend_audio"):
        q = inspect.signature(getattr(pipeline.Diffsound, name)).parameters["joint"]
        assert q.default is False and q.kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(pipeline.Diffsound.generate_loop).parameters
    assert list(p)[1:] == ["text", "seconds", "overlap_seconds", "truncation_rate", "fast", "caption_ids", "seed", "guidance_scale",
                           "negative_text", "sample_rate", "save_root", "level"]
    assert p["overlap_seconds"].default == 2.4 and p["truncation_rate"].default == 0.85
