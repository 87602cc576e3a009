"""Region-held sampling on the GPU (inpainting / continuation): positions of a keep mask carry given tokens through the
reverse chain, inside the sampler kernel and inside the one-call chain.
  * the tail kernels: held columns == known, free columns == the unheld entry bit for bit, both noise sources, K = 256 / 512;
  * whole chains against tests/golden/inpaint_T10_L2.npz -- the reference's p_sample / q_sample loop with the hold applied
    between calls (tools/make_inpaint_golden.py); every free decision of the fixture clears a 1e-4 margin, so 0 tokens may
    differ;
  * the one-call Philox chain == the host-stepped `u` path; a caption alone == inside a batch; the renoise invariants;
  * once at full size (19 layers, T = 100, B = 8); the drivers on synthetic audio.
GPU only (-m gpu)."""
import os
import random

import pytest
import torch

from conftest import golden, parity_line, synth_sd
from text_to_sound_synthesis_amd import _lib, shard, synth

pytestmark = pytest.mark.gpu
NO_GRAD = True

SEED = (0x1a2b << 32) | 20261017
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
    """the device's own stream written out (ds_philox_uniforms): u f32[B, K+1, L]"""
    gids = torch.tensor(list(ids), dtype=torch.long, device="cuda")
    u = torch.empty(len(ids), K + 1, L, device="cuda")
    _lib.check(_lib.lib().ds_philox_uniforms(_lib.ptr(gids), seed, call, stream, _lib.ptr(u), len(ids), L, K, _lib.stream()))
    return u


def sample(dt, cond, **kw):
    return dt.sample(condition_token=None, condition_mask=None, condition_embed=cond, filter_ratio=0, **kw)["content_token"]


# ---- the tail kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 512])
def test_tail_kernel_holds_and_leaves_free_columns_alone(K):
    T = 100
    m = build(1, T=T, codes=K)
    sched = m.transformer._schedule_table()
    lib = _lib.lib()
    g = torch.Generator().manual_seed(K + 1)
    call = 23
    for B, tr, tk in ((3, 0.85, 0), (5, -1.0, 30), (2, -1.0, 0), (1, 0.85, 0)):     # ragged last workgroup, top-r / top-k / none
        logits = (torch.randn(B * L, K, generator=g) * 2.0).cuda()
        xt = torch.randint(0, K + 1, (B, L), generator=g).cuda()
        known = torch.randint(0, K, (B, L), generator=g).cuda()
        t = torch.randint(1, T, (B,), generator=g).cuda()
        ids = [int(v) for v in torch.randint(0, 2 ** 31, (B,), generator=g)]
        gids = torch.tensor(ids, dtype=torch.long, device="cuda")
        u = torch.rand(B, K + 1, L, generator=g).cuda()
        base_u, base_r = torch.empty_like(xt), torch.empty_like(xt)
        _lib.check(lib.ds_sample_tail_ex(_lib.ptr(logits), _lib.ptr(xt), _lib.ptr(t), _lib.ptr(u), _lib.ptr(sched),
                                         _lib.ptr(base_u), None, None, None, B, L, K, T, 0, tr, tk, _lib.stream()))
        _lib.check(lib.ds_sample_tail_rng(_lib.ptr(logits), _lib.ptr(xt), _lib.ptr(t), _lib.ptr(gids), SEED, call,
                                          _lib.ptr(sched), _lib.ptr(base_r), B, L, K, T, 0, tr, tk, _lib.stream()))

        def hold_u(keep, mode=0, known_=known):
            out = torch.full_like(xt, -1)
            rc = lib.ds_sample_tail_hold(_lib.ptr(logits), _lib.ptr(xt), _lib.ptr(t), _lib.ptr(u), _lib.ptr(sched), _lib.ptr(out),
                                         None, None, None, B, L, K, T, 0, tr, tk, _lib.ptr(keep), _lib.ptr(known_), mode,
                                         _lib.stream())
            return rc, out

        def hold_r(keep, mode=0, known_=known):
            out = torch.full_like(xt, -1)
            rc = lib.ds_sample_tail_hold_rng(_lib.ptr(logits), _lib.ptr(xt), _lib.ptr(t), _lib.ptr(gids), SEED, call,
                                             _lib.ptr(sched), _lib.ptr(out), B, L, K, T, 0, tr, tk, _lib.ptr(keep),
                                             _lib.ptr(known_), mode, _lib.stream())
            return rc, out
        some = (torch.rand(B, L, generator=g) < 0.4).to(torch.uint8).cuda()
        some[-1, -1] = 1                                      # the column the last workgroup's dead waves shadow
        for keep in (some, torch.zeros_like(some), torch.ones_like(some)):
            kb = keep.bool()
            for name, fn, base in (("u", hold_u, base_u), ("philox", hold_r, base_r)):
                rc, out = fn(keep)
                assert rc == 0, _lib.lib().ds_last_error_string()
                assert torch.equal(out[kb], known[kb]), "%s: a held column does not carry its token" % name
                assert torch.equal(out[~kb], base[~kb]), "%s: a free column differs from the unheld entry" % name
        # renoise (Philox only): held columns = q_sample of known at t - 1 on stream 1 of the same call; free ones untouched
        rc, out = hold_r(some, mode=1)
        assert rc == 0
        want = m.transformer.q_sample_tokens(known, t - 1, shard.caption_uniforms(ids, call, K, L, SEED, rng_stream=1).cuda())
        sb = some.bool()
        assert torch.equal(out[sb], want[sb]) and torch.equal(out[~sb], base_r[~sb])
        t0 = torch.zeros_like(t)                              # t_post = 0: known itself
        out0 = torch.empty_like(xt)
        _lib.check(lib.ds_sample_tail_hold_rng(_lib.ptr(logits), _lib.ptr(xt), _lib.ptr(t0), _lib.ptr(gids), SEED, call,
                                               _lib.ptr(sched), _lib.ptr(out0), B, L, K, T, 0, tr, tk, _lib.ptr(some),
                                               _lib.ptr(known), 1, _lib.stream()))
        assert torch.equal(out0[sb], known[sb])
        # a null keep is the unheld kernel
        rc, out = hold_u(None, known_=None)
        assert rc == 0 and torch.equal(out, base_u)
        # argument checks: nothing is launched, the error code comes back
        for rc, _ in (hold_u(some, mode=2), hold_r(some, mode=-1), hold_u(some, mode=1), hold_u(some, known_=None),
                      hold_r(some, known_=None)):
            assert rc == -1
        assert b"ds_sample_tail" in lib.ds_last_error_string()
    torch.cuda.synchronize()


# ---- chains against the reference-made fixture -----------------------------------------------------------------------------
def first_difference(g, name, rec):
    """message for a chain that left the fixture: where first, and the fixture's margins of that decision"""
    want = g[name + "_step_tokens"].long()
    for k, got in enumerate(rec):
        d = torch.nonzero(got.cpu() != want[k])
        if d.numel():
            b, p = int(d[0, 0]), int(d[0, 1])
            return ("%s: %d tokens differ after call %d; first at clip %d position %d (held: %s): fixture gap %.3e, cut margin "
                    "%.3e" % (name, d.shape[0], k, b, p, bool(g[name + "_keep"][b, p]), float(g[name + "_gap"][k, b, p]),
                              float(g[name + "_tmargin"][k, b, p])))
    return "%s: every recorded call agrees" % name


@pytest.mark.parametrize("mode", ["f16x2", "fp32"])
@pytest.mark.parametrize("name", ["middle", "prefix", "scattered", "fast2"])
def test_clamp_chains_vs_reference_fixture(name, mode):
    g = golden("inpaint_T10_L2")
    m = build(2, T=10, mode=mode)
    dt = m.transformer
    cond = synth.synth_cond_emb(2, key="traj.cond").cuda()
    keep, known, key = g[name + "_keep"].cuda(), g["known"].long().cuda(), str(g[name + "_noise_key"])
    order = {9: 0, 6: 1, 3: 2, 0: 3} if name == "fast2" else {t: 9 - t for t in range(10)}
    rec, inner = [], dt.p_sample_tokens

    def spy(*a, **k):
        out = inner(*a, **k)
        rec.append(out.clone())
        return out
    dt.p_sample_tokens = spy
    try:
        fn = dt.sample_fast if name == "fast2" else dt.sample
        kw = {"skip_step": 2} if name == "fast2" else {}
        tok = fn(condition_token=None, condition_mask=None, condition_embed=cond, content_token=known, filter_ratio=0,
                 keep_mask=keep, noise_fn=lambda t, shp: synth.synth_uniform(shp, key="%s.u%d" % (key, order[t])), **kw)["content_token"]
    finally:
        del dt.p_sample_tokens
    n = int((tok.cpu() != g[name + "_tokens"].long()).sum())
    print("inpaint chain %s (%s): %d token mismatches (fixture min gap %.2e)" % (name, mode, n, float(g[name + "_min_gap"])))
    parity_line("inpaint T=10 chain %-9s %-5s: %d token mismatches vs the reference's held loop" % (name, mode, n))
    assert n == 0, first_difference(g, name, rec)
    assert len(rec) == g[name + "_step_tokens"].shape[0]
    assert torch.equal(torch.stack(rec).cpu(), g[name + "_step_tokens"].long())


@pytest.mark.parametrize("mode", ["f16x2", "fp32"])
def test_renoise_chain_vs_reference_fixture_in_one_call(mode):
    g = golden("inpaint_T10_L2")
    m = build(2, T=10, mode=mode)
    dt = m.transformer
    cond = synth.synth_cond_emb(2, key="traj.cond").cuda()
    keep, known = g["renoise_keep"].cuda(), g["known"].long().cuda()
    ids, seed = g["caption_ids"].tolist(), int(g["renoise_seed"])
    stepped = []
    dt.p_sample_tokens = lambda *a, **k: stepped.append(1)           # the chain must not come back to Python between steps
    try:
        tok = sample(dt, cond, content_token=known, keep_mask=keep, keep_mode="renoise", caption_ids=ids, seed=seed)
    finally:
        del dt.p_sample_tokens
    assert not stepped
    n = int((tok.cpu() != g["renoise_tokens"].long()).sum())
    print("inpaint chain renoise (%s): %d token mismatches (fixture min gap %.2e)" % (mode, n, float(g["renoise_min_gap"])))
    parity_line("inpaint T=10 chain renoise   %-5s: %d token mismatches vs the reference's held loop" % (mode, n))
    if n:                                                            # locate it: the same chain, one step per call
        gids = torch.tensor(ids, dtype=torch.long, device="cuda")
        kv = dt.transformer.condition_kv(cond, dt._schedule_table())
        hold = (keep.to(torch.uint8).contiguous(), known, 1)
        x = torch.where(keep, dt.q_sample_tokens(known, torch.full((2,), 9, device="cuda"),
                                                 shard.caption_uniforms(ids, 0, 256, L, seed, rng_stream=1).cuda()),
                        torch.full_like(known, 256))
        rec = []
        for k in range(10):
            x = dt.p_sample_tokens_rng(x, kv, torch.full((2,), 9 - k, device="cuda"), gids, k + 1, False, seed=seed, hold=hold)
            rec.append(x.clone())
        assert False, first_difference(g, "renoise", rec)
    assert torch.equal(tok[keep], known[keep])


# ---- the one-call chain == the stepped path; batch independence; renoise invariants ----------------------------------------
def _case(B, key):
    cond = synth.synth_cond_emb(B, key=key + ".cond").cuda()
    known = synth.synth_tokens(B, mask_frac=0.0, key=key + ".known").cuda()
    keep = torch.zeros(B, 53, dtype=torch.bool)
    for b in range(B):
        keep[b, : 4 + 3 * b] = True                       # a prefix per clip ...
        keep[b, 50 - 2 * b:] = True                       # ... and a suffix
    return cond, known, keep[:, :, None].expand(B, 53, 5).reshape(B, L).contiguous().cuda()


def test_one_call_philox_chain_equals_the_stepped_u_path():
    m = build(2, T=10)
    dt = m.transformer
    B, ids = 3, [12, 500, 13]
    cond, known, keep = _case(B, "inp.chain")
    kw = dict(content_token=known, keep_mask=keep)
    a = sample(dt, cond, caption_ids=ids, seed=SEED, **kw)
    b = sample(dt, cond, noise_fn=lambda t, shp: philox_u(ids, 9 - t), **kw)
    assert torch.equal(a, b) and torch.equal(a[keep], known[keep])
    assert not torch.equal(a, sample(dt, cond, caption_ids=ids, seed=SEED))      # the held context matters to the free positions
    order = {9: 0, 6: 1, 3: 2, 0: 3}
    fa = dt.sample_fast(condition_token=None, condition_mask=None, condition_embed=cond, filter_ratio=0, skip_step=2,
                        caption_ids=ids, seed=SEED, **kw)["content_token"]
    fb = dt.sample_fast(condition_token=None, condition_mask=None, condition_embed=cond, filter_ratio=0, skip_step=2,
                        noise_fn=lambda t, shp: philox_u(ids, order[t]), **kw)["content_token"]
    assert torch.equal(fa, fb) and torch.equal(fa[keep], known[keep])
    dt.repeat_rate = 0.5                                   # 'q': with it noise_fn's argument is the running call index
    try:
        random.seed(5)
        qa = sample(dt, cond, caption_ids=ids, seed=SEED, **kw)
        random.seed(5)
        qb = sample(dt, cond, noise_fn=lambda c, shp: philox_u(ids, c), **kw)
        assert torch.equal(qa, qb) and torch.equal(qa[keep], known[keep])
    finally:
        dt.repeat_rate = None
    dt.truncation_r, dt.truncation_k = None, 100           # top{k}p
    try:
        ka = sample(dt, cond, caption_ids=ids, seed=SEED, **kw)
        kb = sample(dt, cond, noise_fn=lambda t, shp: philox_u(ids, 9 - t), **kw)
        assert torch.equal(ka, kb) and torch.equal(ka[keep], known[keep]) and not torch.equal(ka, a)
    finally:
        dt.truncation_r, dt.truncation_k = 0.85, None
    # keep all zero: today's chain, bit for bit, on both noise sources
    none = torch.zeros_like(keep)
    assert torch.equal(sample(dt, cond, caption_ids=ids, seed=SEED, content_token=known, keep_mask=none),
                       sample(dt, cond, caption_ids=ids, seed=SEED))
    nf = lambda t, shp: philox_u(ids, 9 - t)
    assert torch.equal(sample(dt, cond, noise_fn=nf, content_token=known, keep_mask=none), sample(dt, cond, noise_fn=nf))
    # the interface's errors
    with pytest.raises(ValueError):
        dt.sample(condition_token=None, condition_mask=None, condition_embed=cond, filter_ratio=0.5, **kw)
    with pytest.raises(ValueError):
        sample(dt, cond, content_token=known, keep_mask=keep[:, :-1])
    with pytest.raises(ValueError):
        sample(dt, cond, keep_mask=keep)
    with pytest.raises(ValueError):
        sample(dt, cond, keep_mode="renoise", noise_fn=nf, **kw)
    with pytest.raises(ValueError):
        sample(dt, cond, keep_mode="blend", **kw)


@pytest.mark.parametrize("keep_mode", ["clamp", "renoise"])
def test_a_caption_alone_equals_the_caption_in_a_batch(keep_mode):
    m = build(2, T=10)
    dt = m.transformer
    ids = torch.tensor([40, 1000, 7, 99999])
    cond, known, keep = _case(4, "inp.batch")

    def run(sel):
        sel = list(sel)
        return sample(dt, cond[sel].contiguous(), content_token=known[sel].contiguous(), keep_mask=keep[sel].contiguous(),
                      keep_mode=keep_mode, caption_ids=ids[sel], seed=SEED).cpu()
    whole = run(range(4))
    assert int(whole.max()) < 256 and torch.equal(whole[keep.cpu()], known.cpu()[keep.cpu()])
    for i in range(4):
        assert torch.equal(run([i])[0], whole[i]), "caption %d alone differs from the batch of 4 (%s)" % (i, keep_mode)
    assert torch.equal(run([2, 0]), whole[[2, 0]])


def test_renoise_invariants():
    m = build(2, T=10)
    dt = m.transformer
    B, ids = 3, [5, 6, 70000]
    cond, known, keep = _case(B, "inp.renoise")
    gids = torch.tensor(ids, dtype=torch.long, device="cuda")
    kw = dict(content_token=known, keep_mask=keep, keep_mode="renoise", caption_ids=ids, seed=SEED)
    a = sample(dt, cond, **kw)
    assert torch.equal(a[keep], known[keep]) and int(a.max()) < 256
    assert not torch.equal(a, sample(dt, cond, **dict(kw, keep_mode="clamp")))
    f = dt.sample_fast(condition_token=None, condition_mask=None, condition_embed=cond, filter_ratio=0, skip_step=2, **kw)["content_token"]
    assert torch.equal(f[keep], known[keep])
    dt.repeat_rate = 1.0                                   # every call repeated, the last one (t_post = 0) too
    try:
        q = sample(dt, cond, **kw)
        assert torch.equal(q[keep], known[keep])
    finally:
        dt.repeat_rate = None
    # single steps: at t_post > 0 the held positions are the stream-1 draw at t_post - 1; at t_post = 0 they are known, and
    # a repeated call leaves them so
    kv = dt.transformer.condition_kv(cond, dt._schedule_table())
    hold = (keep.to(torch.uint8).contiguous(), known, 1)
    x = torch.where(keep, known, torch.full_like(known, 256))
    t5 = torch.full((B,), 5, device="cuda")
    y = dt.p_sample_tokens_rng(x, kv, t5, gids, 3, False, seed=SEED, hold=hold)
    want = dt.q_sample_tokens(known, t5 - 1, shard.caption_uniforms(ids, 3, 256, L, SEED, rng_stream=1).cuda())
    assert torch.equal(y[keep], want[keep]) and not torch.equal(y[keep], known[keep])
    t0 = torch.zeros(B, dtype=torch.long, device="cuda")
    z1 = dt.p_sample_tokens_rng(y, kv, t0, gids, 4, False, seed=SEED, hold=hold)
    z2 = dt.p_sample_tokens_rng(z1, kv, t0, gids, 5, False, seed=SEED, hold=hold)
    assert torch.equal(z1[keep], known[keep]) and torch.equal(z2[keep], known[keep])
    # the step entries reject what the tail rejects, before anything is enqueued
    lib, p = _lib.lib(), dt.transformer.packed(dt._schedule_table())
    ws = dt.transformer.workspace(B, dt._schedule_table(), 0)
    u = torch.rand(B, 257, L, device="cuda")
    out = torch.empty_like(x)
    assert lib.ds_denoiser_step_hold(p["handle"], _lib.ptr(x), _lib.ptr(t5), None, _lib.ptr(kv), _lib.ptr(u), B, 0, 0.85, 0,
                                     _lib.ptr(hold[0]), _lib.ptr(known), 1, _lib.ptr(ws), _lib.ptr(out), _lib.stream()) == -1
    assert lib.ds_denoiser_step_hold_rng(p["handle"], _lib.ptr(x), _lib.ptr(t5), None, _lib.ptr(kv), _lib.ptr(gids), SEED, 0, B, 0,
                                         0.85, 0, _lib.ptr(hold[0]), None, 0, _lib.ptr(ws), _lib.ptr(out), _lib.stream()) == -1
    tmp = torch.empty_like(x)
    t_steps = torch.zeros(1, 2, B, dtype=torch.long, device="cuda")
    assert lib.ds_denoiser_sample_hold_rng(p["handle"], _lib.ptr(x), _lib.ptr(tmp), _lib.ptr(t_steps), 1, _lib.ptr(kv),
                                           _lib.ptr(gids), SEED, 0, B, 0, 0.85, 0, _lib.ptr(hold[0]), _lib.ptr(known), 3,
                                           _lib.ptr(ws), _lib.stream()) == -1
    torch.cuda.synchronize()


# ---- full size, once -------------------------------------------------------------------------------------------------------
def test_full_size_19_layers_100_steps_batch_8():
    m = build(19, T=100)
    dt = m.transformer
    B = 8
    ids = torch.arange(300, 300 + B)
    cond, known, keep = _case(B, "inp.full")
    kw = dict(content_token=known, caption_ids=ids, seed=SEED)
    a = sample(dt, cond, keep_mask=keep, **kw)
    assert torch.equal(a[keep], known[keep]) and int(a.max()) < 256
    free_same_as_known = float((a[~keep] == known[~keep]).float().mean())
    assert free_same_as_known < 0.05                       # the free positions were generated, not copied
    other = keep.clone()
    other[0] = ~keep[0]                                    # another mask for clip 0 only
    b = sample(dt, cond, keep_mask=other, **kw)
    assert torch.equal(b[1:], a[1:]), "the free positions of a clip depend on another clip's mask"
    assert not torch.equal(b[0], a[0]) and torch.equal(b[0][other[0]], known[0][other[0]])
    r = sample(dt, cond, keep_mask=keep, keep_mode="renoise", **kw)
    assert torch.equal(r[keep], known[keep]) and not torch.equal(r, a)
    plain = sample(dt, cond, caption_ids=ids, seed=SEED)
    assert torch.equal(sample(dt, cond, keep_mask=torch.zeros_like(keep), **kw), plain), \
        "keep all zero must reproduce sample() of the same seed exactly"


# ---- drivers ---------------------------------------------------------------------------------------------------------------
def test_drivers_on_synthetic_audio(tmp_path):
    from text_to_sound_synthesis_amd import audio, pipeline
    from text_to_sound_synthesis_amd import tokenizer as tz
    from text_to_sound_synthesis_amd.config import default_config
    ds = pipeline.Diffsound(config=default_config(n_layer=2, diffusion_step=100, with_clip=True, bpe_path=tz.CLOSED_VOCAB_PATH),
                            random_vocoder=True)
    g = torch.Generator().manual_seed(33)
    tt = torch.arange(217088) / 22050.0
    w22 = torch.stack([0.3 * torch.sin(2 * torch.pi * 440.0 * tt) + 0.05 * torch.randn(217088, generator=g),
                       0.2 * torch.randn(217088, generator=g) * (1.0 + torch.sin(2 * torch.pi * 3.0 * tt))]).cuda()
    captions = synth.synth_captions(2, seed=4)
    input_tokens = ds.model.prepare_content({"audio": w22})["content_token"]
    spans = [[(4.0, 7.0)], [(0.0, 1.5), (8.0, 217088 / 22050)]]
    keep = pipeline.spans_to_keep_mask(spans, 2, "cuda")
    out_dir = str(tmp_path / "inpaint")
    mel01, wave, tokens = ds.inpaint_audio(w22, captions, spans, save_root=out_dir, caption_ids=[0, 1], seed=3)
    assert tuple(mel01.shape) == (2, 80, 848) and tuple(wave.shape) == (2, 1, 217088) and tuple(tokens.shape) == (2, 265)
    assert bool(torch.isfinite(wave).all()) and bool(torch.isfinite(mel01).all())
    assert torch.equal(tokens[keep], input_tokens[keep]) and int(tokens.max()) < 256
    assert not torch.equal(tokens[~keep], input_tokens[~keep])
    assert sorted(os.listdir(out_dir)) == ["000000.npy", "000000.wav", "000001.npy", "000001.wav"]
    x, sr = audio.read_wav(os.path.join(out_dir, "000001.wav"))
    assert sr == 22050 and x.numel() == 217088
    # the truncation rate of the call does not stick to the model, and the same seed gives the same clip
    assert ds.model.transformer.truncation_r is None and not ds.model.truncation_forward
    again = ds.inpaint_audio(w22, captions, spans, caption_ids=[0, 1], seed=3)[2]
    assert torch.equal(again, tokens)
    # from a 48 kHz input, out at 16 kHz: the same tokens are held (the resampled input encodes to them) ...
    w48 = audio.resample(w22, 22050, 48000)
    in48 = ds.model.prepare_content({"audio": w48, "audio_rate": 48000})["content_token"]
    out48 = str(tmp_path / "inpaint48")
    m48, wv48, t48 = ds.inpaint_audio(w48, captions, spans, keep_mode="renoise", audio_rate=48000, sample_rate=16000,
                                      save_root=out48, caption_ids=[0, 1], seed=3)
    assert torch.equal(t48[keep], in48[keep]) and tuple(m48.shape) == (2, 80, 848)
    n16 = -(-217088 * 320 // 441)
    assert tuple(wv48.shape) == (2, 1, n16)
    x, sr = audio.read_wav(os.path.join(out48, "000000.wav"))
    assert sr == 16000 and x.numel() == n16
    # continuation: the recording's last 3 s (17 columns) open the new clip
    mc, wc, tc = ds.continue_audio(w22, captions, 3.0, caption_ids=[0, 1], seed=3, save_root=str(tmp_path / "cont"))
    assert tuple(tc.shape) == (2, 265) and tuple(wc.shape) == (2, 1, 217088) and int(tc.max()) < 256
    assert torch.equal(tc[:, :5 * 17], input_tokens[:, 5 * (53 - 17):])
    assert sorted(os.listdir(str(tmp_path / "cont"))) == ["000000.npy", "000000.wav", "000001.npy", "000001.wav"]
    # the facade, replicate = 2: both replicas hold the input's tokens and differ in what they generate
    out = ds.model.inpaint_content(batch={"text": captions, "audio": w22, "caption_ids": [0, 1], "seed": 3}, keep_mask=keep,
                                   replicate=2, sample_type="top0.85r")
    assert tuple(out["content"].shape) == (4, 1, 80, 848) and tuple(out["content_token"].shape) == (4, 265)
    k2, in2 = torch.cat([keep, keep]), torch.cat([input_tokens, input_tokens])
    assert torch.equal(out["content_token"][k2], in2[k2])
    assert torch.equal(out["content_token"][:2], tokens)             # replica 0 is the un-replicated clip
    assert not torch.equal(out["content_token"][2:], tokens)
    ds.model.truncation_forward = False
    fast = ds.model.inpaint_content(batch={"condition_token": ds.model.prepare_condition({"text": captions})["condition_token"],
                                           "content_token": input_tokens}, keep_mask=keep, sample_type="top0.85r,fast2")
    assert torch.equal(fast["content_token"][keep], input_tokens[keep])
