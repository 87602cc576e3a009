"""Classifier-free guidance on the GPU: the guided sampling tail, the guided step / chain entries and the drivers.
  * the tail kernels against tests/guidance_reference.py on the inputs of tests/guidance_inputs.py (whose fairness
    tests/test_guidance_host.py asserts): log_pred within 4 x d32 of the float64 yardstick (d32 = the distance between its
    float32 and float64 restatements, computed here), kept sets equal except at cuts within 4e-7 of r (at most 1 column in
    200), post within 5e-5 and tokens equal where the kept sets agree -- the rules of tests/test_hip_kernels.py::
    test_sample_tail;
  * held + guided, argument checks, whole chains against guided_loop (0 mismatches), the one-call Philox chain against the
    stepped path, batch independence, guidance_scale None / 1 == today's path, full size once, drivers, condition dropout.
GPU only (-m gpu)."""
import os
import random

import pytest
import torch

import guidance_inputs as I
from conftest import GOLDEN, parity_line, synth_sd
from text_to_sound_synthesis_amd import _lib, shard, synth

pytestmark = pytest.mark.gpu
NO_GRAD = True

SEED = (0x5eed << 32) | 20261017
L = 265


def build(n_layer=2, T=10, mode="f16x2", codes=256):
    from text_to_sound_synthesis_amd.config import build_model, default_config
    m = build_model(default_config(n_layer=n_layer, diffusion_step=T, n_embed=codes))
    sd = dict(synth_sd("dalle", n_layer))
    if T != 100:
        sd = {k: (v[:T] if k.endswith(("ln1.emb.weight", "ln1_1.emb.weight")) else v) for k, v in sd.items()}
    if codes == 256:
        m.load_state_dict(sd, strict=False)
    else:
        synth.synth_init_(m, seed=0)
    m.transformer.transformer.precision = mode
    m = m.cuda().eval()
    m.transformer.truncation_r = 0.85
    return m


def philox_u(ids, call, K=256, stream=0, seed=SEED):
    gids = torch.tensor(list(ids), dtype=torch.long, device="cuda")
    u = torch.empty(len(ids), K + 1, L, device="cuda")
    _lib.check(_lib.lib().ds_philox_uniforms(_lib.ptr(gids), seed, call, stream, _lib.ptr(u), len(ids), L, K, _lib.stream()))
    return u


def sample(dt, cond, **kw):
    return dt.sample(condition_token=None, condition_mask=None, condition_embed=cond, filter_ratio=0, **kw)["content_token"]


def rows(z):
    """logits [B, K, L] -> the kernel's row-major [B * L][K] on the device"""
    return z.permute(0, 2, 1).reshape(-1, z.shape[1]).contiguous().cuda()


def tail_u(K, c, u, sched, trunc_r, trunc_k, scale=None, keep=None, known=None, mode=0, dumps=False, zu="zu"):
    """ds_sample_tail_guided on a case of guidance_inputs -> (rc, tokens, {log_pred, trunc, post})"""
    B = c["B"]
    zc_, zu_ = rows(c["zc"]), (None if zu is None else rows(c[zu]))
    xt, t = c["xt"].cuda(), c["t"].cuda()
    out = torch.full((B, L), -1, dtype=torch.long, device="cuda")
    d = {k: torch.empty(B, K + 1, L, device="cuda") for k in (("log_pred", "trunc", "post") if dumps else ())}
    rc = _lib.lib().ds_sample_tail_guided(
        _lib.ptr(zc_), _lib.ptr(zu_), _lib.ptr(xt), _lib.ptr(t), _lib.ptr(u), _lib.ptr(sched), _lib.ptr(out),
        _lib.ptr(d.get("log_pred")), _lib.ptr(d.get("trunc")), _lib.ptr(d.get("post")), B, L, K, I.T_TAIL, c["initial"],
        trunc_r, trunc_k, c["s"] if scale is None else scale, _lib.ptr(keep), _lib.ptr(known), mode, _lib.stream())
    torch.cuda.synchronize()
    return rc, out, d


def tail_rng(K, c, gids, call, sched, trunc_r, trunc_k, keep=None, known=None, mode=0, t=None):
    B = c["B"]
    zc_, zu_ = rows(c["zc"]), rows(c["zu"])
    xt, t = c["xt"].cuda(), (c["t"] if t is None else t).cuda()
    out = torch.full((B, L), -1, dtype=torch.long, device="cuda")
    rc = _lib.lib().ds_sample_tail_guided_rng(
        _lib.ptr(zc_), _lib.ptr(zu_), _lib.ptr(xt), _lib.ptr(t), _lib.ptr(gids), SEED, call, _lib.ptr(sched), _lib.ptr(out),
        B, L, K, I.T_TAIL, c["initial"], trunc_r, trunc_k, c["s"], _lib.ptr(keep), _lib.ptr(known), mode, _lib.stream())
    torch.cuda.synchronize()
    return rc, out


_SCHED = {}


def sched_table(K):
    if K not in _SCHED:
        _SCHED[K] = build(1, T=I.T_TAIL, codes=K).transformer._schedule_table().clone()
    return _SCHED[K]


# ---- 1. the tail kernel against the yardstick ------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 512])
@pytest.mark.parametrize("idx,trunc_k", [(0, None), (1, None), (2, None), (3, None), (4, None), (0, 30)])
def test_tail_kernel_vs_yardstick(K, idx, trunc_k):
    c = I.tail_case(K, idx, trunc_k)
    r32, r64 = c["ref32"], c["ref64"]
    sched = sched_table(K)
    tr, tk = (-1.0, trunc_k) if trunc_k else (I.TRUNC_R, 0)
    rc, tok, d = tail_u(K, c, c["u"].cuda(), sched, tr, tk, dumps=True)
    assert rc == 0, _lib.lib().ds_last_error_string()
    lp, trunc, post, tok = d["log_pred"].cpu(), d["trunc"].cpu(), d["post"].cpu(), tok.cpu()
    d32 = float((r32["log_pred"].double() - r64["log_pred"]).abs().max())
    err = float((lp.double() - r64["log_pred"]).abs().max())
    print("guided tail K=%d case %d%s: log_pred err %.3e vs f64 (d32 %.3e)" % (K, idx, " top-k" if trunc_k else "", err, d32))
    assert err <= 4 * d32, "log_pred %.3e from the float64 yardstick, 4 x d32 = %.3e" % (err, 4 * d32)
    assert bool((lp[:, -1] == -70.0).all())
    same = (I.kept(trunc) == I.kept(r32["trunc"])).all(1)                      # [B, L]: columns whose kept sets agree
    if not bool(same.all()):
        # a differing column must be one whose cut sits within 4e-7 of r (the inclusive mass at the yardstick's last kept
        # rank or the one before it), and such columns may be at most 1 in 200
        assert not trunc_k, "top-k kept sets differ in %d columns" % int((~same).sum())
        srt = torch.sort(r64["log_pred"], dim=1, descending=True).values
        inc = torch.exp(srt).cumsum(1)
        near = ((inc - I.TRUNC_R).abs() < 4e-7).any(1)
        assert bool(near[~same].all()), "kept sets differ in columns whose cut is not within 4e-7 of r"
        assert int((~same).sum()) * 200 <= same.numel()
    sel = same[:, None, :].expand_as(trunc)
    kept_vals = torch.where(torch.cat((I.kept(trunc), torch.zeros_like(same)[:, None, :]), 1), lp, torch.full_like(lp, -70.0))
    assert torch.equal(trunc, kept_vals), "the truncated prediction is not log_pred on the kept set and -70 elsewhere"
    if idx == 4:
        assert float(lp[:, :-1].min()) == -70.0          # the clamp case reaches the clamp; log_pred and kept sets only
        return
    perr = float((post - r32["post"])[sel].abs().max())
    assert perr <= 5e-5, "post %.3e" % perr
    assert torch.equal(tok[same], r32["tokens"][same]), "%d tokens differ" % int((tok != r32["tokens"])[same].sum())
    parity_line("guided tail K=%d case %d%s: log_pred %.2e (4 d32 = %.2e), post %.2e, tokens equal, %d excused columns"
                % (K, idx, " top-k" if trunc_k else "", err, 4 * d32, perr, int((~same).sum())))
    # the _rng entry == the u entry fed with the stream ds_philox_uniforms writes out, bit for bit
    ids = [7, 123456, 2 ** 31 + 5][:c["B"]]
    gids = torch.tensor(ids, dtype=torch.long, device="cuda")
    rc, a = tail_rng(K, c, gids, 11, sched, tr, tk)
    assert rc == 0
    rc, b, _ = tail_u(K, c, philox_u(ids, 11, K), sched, tr, tk)
    assert rc == 0 and torch.equal(a, b)


# ---- 2. held + guided; 3. argument checks ----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 512])
def test_held_guided_and_argument_checks(K):
    c = I.tail_case(K, 0)
    B, sched = c["B"], sched_table(K)
    g = torch.Generator().manual_seed(K + 3)
    known = torch.randint(0, K, (B, L), generator=g).cuda()
    some = (torch.rand(B, L, generator=g) < 0.4).to(torch.uint8).cuda()
    some[-1, -1] = 1                                                            # the column the dead waves shadow
    ids = [3, 99, 70000][:B]
    gids = torch.tensor(ids, dtype=torch.long, device="cuda")
    u = c["u"].cuda()
    call, tr = 5, I.TRUNC_R
    _, base_u, _ = tail_u(K, c, u, sched, tr, 0)
    _, base_r = tail_rng(K, c, gids, call, sched, tr, 0)
    assert torch.equal(base_u.cpu(), c["ref32"]["tokens"])
    for keep in (some, torch.zeros_like(some), torch.ones_like(some)):
        kb = keep.bool()
        rc, out, _ = tail_u(K, c, u, sched, tr, 0, keep=keep, known=known)
        assert rc == 0 and torch.equal(out[kb], known[kb]) and torch.equal(out[~kb], base_u[~kb])
        rc, out = tail_rng(K, c, gids, call, sched, tr, 0, keep=keep, known=known)
        assert rc == 0 and torch.equal(out[kb], known[kb]) and torch.equal(out[~kb], base_r[~kb])
    # renoise: held columns = q_sample of known at t - 1 on stream 1 of the same call; t_post = 0: known itself
    sb = some.bool()
    rc, out = tail_rng(K, c, gids, call, sched, tr, 0, keep=some, known=known, mode=1)
    dt = build(1, T=I.T_TAIL, codes=K).transformer
    want = dt.q_sample_tokens(known, c["t"].cuda() - 1, shard.caption_uniforms(ids, call, K, L, SEED, rng_stream=1).cuda())
    assert rc == 0 and torch.equal(out[sb], want[sb]) and torch.equal(out[~sb], base_r[~sb])
    rc, out0 = tail_rng(K, c, gids, call, sched, tr, 0, keep=some, known=known, mode=1, t=torch.zeros_like(c["t"]))
    assert rc == 0 and torch.equal(out0[sb], known[sb])
    # argument checks: -1, the message names the entry, nothing is launched (the output keeps its fill)
    lib = _lib.lib()
    bad = [tail_u(K, c, u, sched, tr, 0, zu=None), tail_u(K, c, u, sched, tr, 0, scale=float("nan")),
           tail_u(K, c, u, sched, tr, 0, scale=float("inf")), tail_u(K, c, u, sched, tr, 0, keep=some, known=known, mode=2),
           tail_u(K, c, u, sched, tr, 0, keep=some, known=known, mode=1), tail_u(K, c, u, sched, tr, 0, keep=some),
           tail_u(K, c, u, sched, tr, 30)]
    for rc, out, _ in bad:
        assert rc == -1 and bool((out == -1).all())
        assert b"ds_sample_tail_guided" in lib.ds_last_error_string()
    rc, out = tail_rng(K, c, gids, call, sched, tr, 0, keep=some, known=None)
    assert rc == -1 and bool((out == -1).all()) and b"ds_sample_tail_guided_rng" in lib.ds_last_error_string()


def test_denoiser_entries_reject_before_enqueuing():
    m = build(2, T=10)
    dt = m.transformer
    B = 2
    cond, null, known, keep = [v.cuda() for v in I.chain_inputs()]
    sched = dt._schedule_table()
    kv2, scale, tokens2 = dt._guide_start((null, 3.0), cond, sched)
    lib, p = _lib.lib(), dt.transformer.packed(sched)
    ws = dt.transformer.workspace(2 * B, sched, 0)
    x = torch.full((B, L), 256, dtype=torch.long, device="cuda")
    t2 = torch.full((2 * B,), 5, dtype=torch.long, device="cuda")
    u = torch.rand(B, 257, L, device="cuda")
    gids = torch.arange(B, device="cuda")
    k8 = keep.to(torch.uint8).contiguous()
    tokens2.fill_(-7)
    out = torch.full_like(x, -1)
    step = lambda sc, kp, kn, md: lib.ds_denoiser_step_guided(
        p["handle"], _lib.ptr(x), _lib.ptr(t2), None, _lib.ptr(kv2), _lib.ptr(u), B, 0, 0.85, 0, sc, _lib.ptr(kp), _lib.ptr(kn),
        md, _lib.ptr(tokens2), _lib.ptr(ws), _lib.ptr(out), _lib.stream())
    step_r = lambda sc, kp, kn, md: lib.ds_denoiser_step_guided_rng(
        p["handle"], _lib.ptr(x), _lib.ptr(t2), None, _lib.ptr(kv2), _lib.ptr(gids), SEED, 0, B, 0, 0.85, 0, sc, _lib.ptr(kp),
        _lib.ptr(kn), md, _lib.ptr(tokens2), _lib.ptr(ws), _lib.ptr(out), _lib.stream())
    tmp = torch.empty_like(x)
    t_steps = torch.zeros(1, 2, 2 * B, dtype=torch.long, device="cuda")
    chain = lambda sc, kp, kn, md: lib.ds_denoiser_sample_guided_rng(
        p["handle"], _lib.ptr(x), _lib.ptr(tmp), _lib.ptr(t_steps), 1, _lib.ptr(kv2), _lib.ptr(gids), SEED, 0, B, 0, 0.85, 0, sc,
        _lib.ptr(kp), _lib.ptr(kn), md, _lib.ptr(tokens2), _lib.ptr(ws), _lib.stream())
    for fn, name in ((step, b"ds_denoiser_step_guided"), (step_r, b"ds_denoiser_step_guided_rng"),
                     (chain, b"ds_denoiser_sample_guided_rng")):
        for args in ((float("nan"), None, None, 0), (3.0, k8, known, 3), (3.0, k8, None, 0)):
            assert fn(*args) == -1 and name in lib.ds_last_error_string()
    assert step(3.0, k8, known, 1) == -1                  # renoise on caller uniforms
    torch.cuda.synchronize()
    assert bool((tokens2 == -7).all()) and bool((out == -1).all()), "a rejected call enqueued work"
    assert step(3.0, None, None, 0) == 0 and step_r(3.0, k8, known, 1) == 0
    torch.cuda.synchronize()
    assert bool((tokens2[:B] == x).all()) and bool((tokens2[B:] == x).all())


# ---- 4. chains against guided_loop -----------------------------------------------------------------------------------------
def first_difference(name, rec, want):
    for k, got in enumerate(rec):
        d = torch.nonzero(got.cpu() != want[k])
        if d.numel():
            return "%s: %d tokens differ after call %d; first at clip %d position %d (the yardstick's smallest gap of the " \
                   "whole chain: %.3e)" % (name, d.shape[0], k, int(d[0, 0]), int(d[0, 1]), I.chain_reference(name)[1])
    return "%s: every recorded call agrees" % name


@pytest.mark.parametrize("mode", ["f16x2", "fp32"])
@pytest.mark.parametrize("name", list(I.CHAINS))
def test_chain_vs_guided_loop(name, mode):
    want, gap = I.chain_reference(name)
    m = build(2, T=10, mode=mode)
    dt = m.transformer
    cond, null, known, keep = [v.cuda() for v in I.chain_inputs()]
    c = I.CHAINS[name]
    order = {t: k for k, (t, _) in enumerate(I.R.chain_steps(I.T_CHAIN, c["skip_step"]))}
    noise = I.chain_noise(name)
    rec, inner = [], dt.p_sample_tokens

    def spy(*a, **k):
        out = inner(*a, **k)
        rec.append(out.clone())
        return out
    dt.p_sample_tokens = spy
    try:
        fn = dt.sample_fast if c["skip_step"] else dt.sample
        kw = {"skip_step": c["skip_step"]} if c["skip_step"] else {}
        if c["held"]:
            kw.update(content_token=known, keep_mask=keep)
        tok = fn(condition_token=None, condition_mask=None, condition_embed=cond, filter_ratio=0,
                 noise_fn=lambda t, shp: noise(order[t], shp), guidance_scale=I.CHAIN_SCALE, null_condition_embed=null[0],
                 **kw)["content_token"]
    finally:
        del dt.p_sample_tokens
    n = int((tok.cpu() != want[-1]).sum())
    print("guided chain %s (%s): %d token mismatches (yardstick min gap %.2e)" % (name, mode, n, gap))
    parity_line("guided T=10 chain %-7s %-5s: %d token mismatches vs guided_loop" % (name, mode, n))
    assert n == 0, first_difference(name, rec, want)
    assert len(rec) == want.shape[0] and torch.equal(torch.stack(rec).cpu(), want)
    if c["held"]:
        assert torch.equal(tok[keep], known[keep])


# ---- 5. the one-call Philox chain == the stepped path; 6. batch independence; 7. None / 1.0 --------------------------------
def test_one_call_philox_chain_equals_the_stepped_path():
    m = build(2, T=10)
    dt = m.transformer
    B, ids = 3, [12, 500, 13]
    cond = synth.synth_cond_emb(B, key="guid.p.cond").cuda()
    null = synth.synth_cond_emb(1, key="guid.null")[0].cuda()
    known = synth.synth_tokens(B, mask_frac=0.0, key="guid.p.known").cuda()
    keep = torch.zeros(B, L, dtype=torch.bool, device="cuda")
    keep[:, 40:120] = True
    g = dict(guidance_scale=3.0, null_condition_embed=null)
    stepped = []
    dt.p_sample_tokens = lambda *a, **k: stepped.append(1)           # the chain must not come back to Python between steps
    try:
        a = sample(dt, cond, caption_ids=ids, seed=SEED, **g)
    finally:
        del dt.p_sample_tokens
    assert not stepped
    b = sample(dt, cond, noise_fn=lambda t, shp: philox_u(ids, 9 - t), **g)
    assert torch.equal(a, b) and int(a.max()) < 256
    assert not torch.equal(a, sample(dt, cond, caption_ids=ids, seed=SEED))
    order = {9: 0, 6: 1, 3: 2, 0: 3}
    fkw = dict(condition_token=None, condition_mask=None, condition_embed=cond, filter_ratio=0, skip_step=2, **g)
    assert torch.equal(dt.sample_fast(caption_ids=ids, seed=SEED, **fkw)["content_token"],
                       dt.sample_fast(noise_fn=lambda t, shp: philox_u(ids, order[t]), **fkw)["content_token"])
    dt.repeat_rate = 0.5                                   # 'q': noise_fn's argument is the running call index
    try:
        random.seed(5)
        qa = sample(dt, cond, caption_ids=ids, seed=SEED, **g)
        random.seed(5)
        qb = sample(dt, cond, noise_fn=lambda c, shp: philox_u(ids, c), **g)
        assert torch.equal(qa, qb) and not torch.equal(qa, a)
    finally:
        dt.repeat_rate = None
    dt.truncation_r, dt.truncation_k = None, 100           # top{k}p
    try:
        assert torch.equal(sample(dt, cond, caption_ids=ids, seed=SEED, **g),
                           sample(dt, cond, noise_fn=lambda t, shp: philox_u(ids, 9 - t), **g))
    finally:
        dt.truncation_r, dt.truncation_k = 0.85, None
    # region-held, both keep modes
    hk = dict(content_token=known, keep_mask=keep, **g)
    ha = sample(dt, cond, caption_ids=ids, seed=SEED, **hk)
    hb = sample(dt, cond, noise_fn=lambda t, shp: philox_u(ids, 9 - t), **hk)
    assert torch.equal(ha, hb) and torch.equal(ha[keep], known[keep]) and not torch.equal(ha, a)
    hr = sample(dt, cond, caption_ids=ids, seed=SEED, keep_mode="renoise", **hk)
    assert torch.equal(hr[keep], known[keep]) and not torch.equal(hr, ha)
    # the interface's errors
    with pytest.raises(ValueError):
        sample(dt, cond, guidance_scale=3.0)
    with pytest.raises(ValueError):
        sample(dt, cond, guidance_scale=float("nan"), null_condition_embed=null)
    with pytest.raises(ValueError):
        sample(dt, cond, guidance_scale=3.0, null_condition_embed=null[:5])


def test_a_caption_alone_equals_the_caption_in_a_batch():
    m = build(2, T=10)
    dt = m.transformer
    ids = torch.tensor([40, 1000, 7])
    cond = synth.synth_cond_emb(3, key="guid.b.cond").cuda()
    nulls = synth.synth_cond_emb(3, key="guid.b.null").cuda()          # a null condition per caption ([B, 77, 512])
    run = lambda sel: sample(dt, cond[sel].contiguous(), caption_ids=ids[sel], seed=SEED, guidance_scale=3.0,
                             null_condition_embed=nulls[sel].contiguous()).cpu()
    whole = run([0, 1, 2])
    for i in range(3):
        assert torch.equal(run([i])[0], whole[i]), "caption %d alone differs from the batch of 3" % i


def test_scale_none_and_one_are_the_unguided_path():
    m = build(2, T=10)
    dt = m.transformer
    ids = [4, 5]
    cond, null, _, _ = [v.cuda() for v in I.chain_inputs()]
    lib = _lib.lib()
    called = []

    class Spy:
        def __getattr__(self, name):
            if "guided" in name:
                called.append(name)
            return getattr(lib, name)
    plain_p = sample(dt, cond, caption_ids=ids, seed=SEED)
    nf = lambda t, shp: philox_u(ids, 9 - t)
    plain_u = sample(dt, cond, noise_fn=nf)
    from text_to_sound_synthesis_amd.modeling import diffusion
    real = _lib.lib
    _lib.lib = lambda: Spy()
    try:
        assert diffusion._lib.lib is _lib.lib
        for kw in (dict(guidance_scale=None), dict(guidance_scale=1.0), dict(guidance_scale=1.0, null_condition_embed=null),
                   dict(guidance_scale=None, null_condition_embed=null)):
            assert torch.equal(sample(dt, cond, caption_ids=ids, seed=SEED, **kw), plain_p)
            assert torch.equal(sample(dt, cond, noise_fn=nf, **kw), plain_u)
        assert not called
        sample(dt, cond, caption_ids=ids, seed=SEED, guidance_scale=2.0, null_condition_embed=null)
        assert called == ["ds_denoiser_sample_guided_rng"]
    finally:
        _lib.lib = real


# ---- 8. full size, once ----------------------------------------------------------------------------------------------------
def test_full_size_19_layers_100_steps():
    m = build(19, T=100)
    dt = m.transformer
    ids = torch.tensor([300, 301])
    cond = synth.synth_cond_emb(2, key="guid.full.cond").cuda()
    null = synth.synth_cond_emb(1, key="guid.null")[0].cuda()
    kw = dict(caption_ids=ids, seed=SEED, guidance_scale=3.0, null_condition_embed=null)
    a = sample(dt, cond, **kw)
    assert int(a.min()) >= 0 and int(a.max()) < 256
    assert torch.equal(sample(dt, cond, **kw), a)
    assert not torch.equal(sample(dt, cond, caption_ids=ids, seed=SEED), a)


# ---- 9. drivers ------------------------------------------------------------------------------------------------------------
def test_drivers_on_synthetic_weights():
    from text_to_sound_synthesis_amd import pipeline
    from text_to_sound_synthesis_amd.config import default_config
    # the package's closed merge table covers the synthetic captions' words only: the fixture adds "silence" with the full
    # table's ranks and ids (tools/make_guidance_vocab.py)
    vocab = os.path.join(GOLDEN, "bpe_closed_vocab_guidance.json")
    ds = pipeline.Diffsound(config=default_config(n_layer=2, diffusion_step=100, with_clip=True, bpe_path=vocab), random_vocoder=True)
    model, dt = ds.model, ds.model.transformer
    captions = synth.synth_captions(2, seed=4)
    mel01, wave, tokens = ds.generate_sample_with_condition(captions, caption_ids=[0, 1], seed=3, guidance_scale=3,
                                                            negative_text="silence")
    assert tuple(mel01.shape) == (2, 80, 848) and tuple(wave.shape) == (2, 1, 217088) and tuple(tokens.shape) == (2, 265)
    assert bool(torch.isfinite(wave).all()) and int(tokens.max()) < 256
    # ... the tokens of the model-level call
    null = model.null_condition("silence")
    assert tuple(null.shape) == (77, 512) and tuple(model.null_condition().shape) == (77, 512)
    assert model.null_condition() is model.null_condition() and not torch.equal(null, model.null_condition())
    assert tuple(model.null_condition(["silence", "music"]).shape) == (2, 77, 512)
    cond = model.prepare_condition({"text": captions})
    dt.truncation_r = 0.85
    want = dt.sample(condition_token=cond["condition_token"], condition_mask=None, condition_embed=None, filter_ratio=0,
                     caption_ids=[0, 1], seed=3, guidance_scale=3.0, null_condition_embed=null)["content_token"]
    assert torch.equal(tokens, want)
    plain = ds.generate_sample_with_condition(captions, caption_ids=[0, 1], seed=3)[2]
    assert not torch.equal(plain, tokens)
    assert torch.equal(ds.generate_sample_with_condition(captions, caption_ids=[0, 1], seed=3, guidance_scale=1.0)[2], plain)
    # replicate: the null embedding follows the captions
    rep = model.generate_content(batch={"text": captions, "caption_ids": [0, 1], "seed": 3, "negative_text": ["silence", "silence"]},
                                 filter_ratio=0, replicate=2, guidance_scale=3.0)["content_token"]
    assert tuple(rep.shape) == (4, 265) and int(rep.max()) < 256 and not torch.equal(rep[2:], rep[:2])
    # inpainting keeps the held tokens exactly
    g = torch.Generator().manual_seed(33)
    w22 = (0.2 * torch.randn(2, 217088, generator=g)).cuda()
    spans = [[(4.0, 7.0)], [(0.0, 1.5)]]
    keep = pipeline.spans_to_keep_mask(spans, 2, "cuda")
    input_tokens = model.prepare_content({"audio": w22})["content_token"]
    t_in = ds.inpaint_audio(w22, captions, spans, caption_ids=[0, 1], seed=3, guidance_scale=3)[2]
    assert torch.equal(t_in[keep], input_tokens[keep]) and int(t_in.max()) < 256
    assert not torch.equal(t_in, ds.inpaint_audio(w22, captions, spans, caption_ids=[0, 1], seed=3)[2])


# ---- 10. condition dropout on the device -----------------------------------------------------------------------------------
def test_condition_dropout_on_the_device():
    from text_to_sound_synthesis_amd.modeling import train
    m = build(2, T=100)
    B = 16                      # (both outcomes occur among 16 rows at p = 0.5 except with probability 2^-15)
    cond = synth.synth_cond_emb(B, key="guid.drop.cond").cuda()
    null = synth.synth_cond_emb(1, key="guid.null")[0].cuda()
    batch = {"condition_embed_token": cond, "content_token": synth.synth_tokens(B, mask_frac=0.0, key="guid.drop.x0").cuda()}
    gen = lambda: torch.Generator(device="cuda").manual_seed(77)
    g0, g1 = gen(), gen()
    base = train.training_inputs(m, batch, generator=g0)
    same = train.training_inputs(m, batch, generator=g1, cond_drop_prob=0.0, null_cond=null)
    assert all(torch.equal(a, b) for a, b in zip(base, same)) and torch.equal(g0.get_state(), g1.get_state())
    full = train.training_inputs(m, batch, generator=gen(), cond_drop_prob=1.0, null_cond=null)
    assert bool((full[1] == null[None]).all()) and all(torch.equal(a, b) for a, b in zip(base[2:], full[2:]))
    h1 = train.training_inputs(m, batch, generator=gen(), cond_drop_prob=0.5, null_cond=null)
    h2 = train.training_inputs(m, batch, generator=gen(), cond_drop_prob=0.5, null_cond=null)
    assert torch.equal(h1[1], h2[1])
    is_null, is_orig = (h1[1] == null[None]).flatten(1).all(1), (h1[1] == cond).flatten(1).all(1)
    assert bool((is_null ^ is_orig).all()) and bool(is_null.any()) and bool(is_orig.any())
    with pytest.raises(ValueError):
        train.training_inputs(m, batch, generator=gen(), cond_drop_prob=0.5)


def test_solver_step_with_condition_dropout():
    import math
    from text_to_sound_synthesis_amd import tokenizer as tz
    from text_to_sound_synthesis_amd.config import build_model, default_config
    from text_to_sound_synthesis_amd.modeling import solver, train
    m = build_model(default_config(n_layer=2, diffusion_step=100, with_clip=True, bpe_path=tz.CLOSED_VOCAB_PATH))
    synth.synth_init_(m, seed=0)
    m = m.cuda().eval()
    s = solver.Solver(train.TrainStep(m.transformer, precision="f16x2"), lr=1e-4, model=m,
                      generator=torch.Generator(device="cuda").manual_seed(5), cond_drop_prob=0.5)
    assert s.cond_drop_prob == 0.5 and tuple(s.null_cond.shape) == (77, 512)
    assert torch.equal(s.null_cond, m.null_condition())
    out = s.step({"text": synth.synth_captions(4, seed=2),
                  "content_token": synth.synth_tokens(4, mask_frac=0.0, key="guid.solver.x0").cuda()})
    assert math.isfinite(float(out["loss"]))
    plain = solver.Solver(train.TrainStep(m.transformer, precision="f16x2"), model=m)
    assert plain.cond_drop_prob == 0.0 and plain.null_cond is None
    with pytest.raises(ValueError):
        solver.Solver(train.TrainStep(m.transformer, precision="f16x2"), cond_drop_prob=0.5)      # needs the model's null condition
