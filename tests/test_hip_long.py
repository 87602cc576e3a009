"""Long-form generation on the GPU: clips longer than one 5 x 53 token grid.
  * ds_mel_stitch against the float64 yardstick of tests/long_reference.py: bit-identical outside the overlaps, within
    4 x d32 inside them (d32 = the distance of the formula's float32 evaluation from float64 on the same input: the rule of
    the audio and resampler tests), its argument errors;
  * the token carry of DALLE.generate_long_content: every window opens with its predecessor's last columns, window 0 is
    generate_content, window w is inpaint_content on the continuation, batch independence, seeds, start_token, guidance;
  * the drivers Diffsound.generate_long / extend_audio: lengths, the mel is the stitch of the windows' decodes, the waveform is
    ONE vocoder pass over it, sample rates, files;
  * the vocoder at a length no other test runs (1712 frames) against the CPU oracle.
GPU only (-m gpu)."""
import math
import os

import numpy as np
import pytest
import torch

import diffsound_oracle as O
import long_reference as LR
from conftest import parity_line, synth_sd
from text_to_sound_synthesis_amd import _lib, audio, pipeline, synth

pytestmark = pytest.mark.gpu
NO_GRAD = True

WAVE_RMS_TOL = 1e-4           # BASELINE.json north_star: RMS on waveform (tests/test_hip_models.py)
FACTOR = 4                    # |kernel - float64| <= 4 x d32
SEED = (0x3c4d << 32) | 20261019
L = 265


# ---- the stitch kernel -----------------------------------------------------------------------------------------------------
def _stitch_case(B, W, C, F, S, seed):
    g = torch.Generator().manual_seed(seed)
    win = torch.randn(B, W, C, F, generator=g)
    fade = audio.fade_table(F - S).numpy()
    return win, fade


def _check_stitch(tag, win, fade, S, a, b):
    """the kernel against the yardstick; returns (err inside the overlaps, d32)"""
    B, W, C, F = win.shape
    got = audio.stitch_mel(win.cuda(), S, a, b).cpu().numpy()
    r64 = LR.stitch(win.numpy(), fade, S, a, b)
    r32 = LR.stitch(win.numpy(), fade, S, a, b, dtype=np.float32)
    assert got.shape == r64.shape == (B, C, F + (W - 1) * S) and got.dtype == np.float32
    ov = LR.overlap_mask(W, F, S)
    if (a, b) == (1.0, 0.0):
        assert np.array_equal(got[:, :, ~ov], r64[:, :, ~ov].astype(np.float32)), "%s: a frame outside the overlaps is not the input's" % tag
        assert np.array_equal(got[:, :, ~ov].view(np.uint32), r32[:, :, ~ov].view(np.uint32))
        sel = ov
    else:
        sel = np.ones_like(ov)                   # the fold rounds everywhere
    if not sel.any():
        return 0.0, 0.0
    err = float(np.abs(got.astype(np.float64) - r64)[:, :, sel].max())
    d32 = float(np.abs(r32.astype(np.float64) - r64)[:, :, sel].max())
    line = "mel stitch %s a=%g b=%g: |kernel - f64| %.2e, bound %.2e = 4 x d32 %.2e" % (tag, a, b, err, FACTOR * d32, d32)
    print(line)
    parity_line(line)
    assert err <= FACTOR * d32, line
    return err, d32


@pytest.mark.parametrize("shape", [(1, 1, 80, 848, 848), (3, 2, 80, 848, 832), (2, 3, 80, 848, 432), (1, 4, 5, 32, 20)],
                         ids=["copy", "V16", "V416", "ragged"])
def test_stitch_kernel_vs_float64(shape):
    B, W, C, F, S = shape
    win, fade = _stitch_case(B, W, C, F, S, seed=F + S + W)
    err, d32 = _check_stitch("B%d W%d C%d F%d S%d" % shape, win, fade, S, 1.0, 0.0)
    if W == 1:
        assert torch.equal(audio.stitch_mel(win.cuda(), S).cpu(), win[:, 0])          # a pure copy
    else:
        assert d32 > 0.0                                                               # the overlaps were really blended


def test_stitch_kernel_folds_scale_and_shift():
    B, W, C, F, S = 2, 3, 80, 848, 432
    win, fade = _stitch_case(B, W, C, F, S, seed=11)
    _check_stitch("B%d W%d C%d F%d S%d" % (B, W, C, F, S), win, fade, S, 0.5, 0.5)
    one = torch.randn(2, 1, 80, 848, generator=torch.Generator().manual_seed(12))
    assert torch.equal(audio.stitch_mel(one.cuda(), 848, 0.5, 0.5).cpu(), 0.5 * one[:, 0] + 0.5)   # W = 1: a scaled copy


def test_stitch_kernel_refuses_bad_shapes_without_a_launch():
    lib = _lib.lib()
    for B, W, C, F, S in ((1, 2, 4, 30, 20), (1, 2, 4, 32, 18), (1, 2, 4, 32, 12), (1, 2, 4, 32, 36), (1, 0, 4, 32, 32)):
        win = torch.randn(B, max(W, 1), C, F).cuda()
        fade = torch.rand(64).cuda()
        out = torch.full((B, C, F + max(W - 1, 0) * S + 8), -7.0).cuda()
        rc = lib.ds_mel_stitch(_lib.ptr(win), _lib.ptr(fade), _lib.ptr(out), B, W, C, F, S, 1.0, 0.0, _lib.stream())
        torch.cuda.synchronize()
        assert rc == -1 and b"ds_mel_stitch" in lib.ds_last_error_string(), (F, S)
        assert bool((out == -7.0).all()), "out was written"
    with pytest.raises(_lib.DiffsoundHipError):
        audio.stitch_mel(torch.zeros(1, 2, 4, 32).cuda(), 12)             # V = 20 > S
    with pytest.raises(_lib.DiffsoundHipError):
        audio.stitch_mel(torch.zeros(1, 2, 4, 32), 20)                    # a host tensor: no CPU path


# ---- the token carry -------------------------------------------------------------------------------------------------------
def build(n_layer=2, T=10, mode="f16x2"):
    """the model of tests/test_hip_inpaint.py::build"""
    from text_to_sound_synthesis_amd.config import build_model, default_config
    m = build_model(default_config(n_layer=n_layer, diffusion_step=T))
    sd = dict(synth_sd("dalle", n_layer))
    if T != 100:
        sd = {k: (v[:T] if k.endswith(("ln1.emb.weight", "ln1_1.emb.weight")) else v) for k, v in sd.items()}
    m.load_state_dict(sd, strict=False)
    m.transformer.transformer.precision = mode
    m = m.cuda().eval()
    m.transformer.truncation_r = 0.85
    return m


@pytest.fixture(scope="module")
def carry():
    """(model, cond, ids, the B = 2, W = 3 run) -- computed once, never modified"""
    m = build(2, T=10)
    cond = synth.synth_cond_emb(2, key="long.cond").cuda()
    ids = [7, 300000]
    out = m.generate_long_content(batch={"condition_embed_token": cond, "caption_ids": ids, "seed": SEED}, windows=3, overlap_cols=13)
    return m, cond, ids, out


def test_token_carry_between_windows(carry):
    m, cond, ids, out = carry
    tok = out["content_token"]
    assert tuple(tok.shape) == (2, 3, L) and tok.dtype == torch.long and int(tok.max()) < 256 and int(tok.min()) >= 0
    assert tuple(out["content"].shape) == (6, 1, 80, 848)
    for w in (1, 2):
        assert torch.equal(tok[:, w, :65], tok[:, w - 1, 200:]), "window %d does not open with its predecessor's tail" % w
        assert not torch.equal(tok[:, w], tok[:, w - 1])
    # the truncation settings of the call did not stick or get lost
    assert m.transformer.truncation_r == 0.85 and m.transformer.truncation_k is None and not m.truncation_forward
    # the mel is the decode of the flattened windows, clip-major
    assert torch.equal(out["content"], m.decode_to_img(tok.view(6, L), (6, 256, 5, 53)))


def test_windows_are_the_existing_chains(carry):
    m, cond, ids, out = carry
    tok = out["content_token"]
    keep_tf = m.truncation_forward
    try:
        m.truncation_forward = True                         # (the fixture's truncation_r = 0.85 stays installed)
        w0 = m.generate_content(batch={"condition_embed_token": cond, "caption_ids": ids, "seed": SEED}, filter_ratio=0,
                                content_ratio=1, sample_type="top0.85r")["content_token"]
        assert torch.equal(tok[:, 0], w0), "window 0 is not generate_content's clip"
        for w in (1, 2):
            known, keep = pipeline.continuation_tokens(tok[:, w - 1], 13)
            wid = [i + w * (1 << 20) for i in ids]
            direct = m.inpaint_content(batch={"condition_embed_token": cond, "content_token": known, "caption_ids": wid,
                                              "seed": SEED}, keep_mask=keep, sample_type="top0.85r")["content_token"]
            assert torch.equal(tok[:, w], direct), "window %d is not inpaint_content on the continuation" % w
    finally:
        m.truncation_forward = keep_tf


def test_a_caption_alone_a_second_call_and_another_seed(carry):
    m, cond, ids, out = carry
    tok = out["content_token"]
    run = lambda **kw: m.generate_long_content(batch=dict({"condition_embed_token": cond, "caption_ids": ids, "seed": SEED}, **kw),
                                               windows=3, overlap_cols=13)["content_token"]
    alone = run(condition_embed_token=cond[1:].contiguous(), caption_ids=ids[1:])
    assert torch.equal(alone[0], tok[1]), "caption 1 alone differs from its row in the batch"
    assert torch.equal(run(), tok)
    other = run(seed=SEED + 1)
    assert not torch.equal(other[:, 0], tok[:, 0]) and not torch.equal(other[:, 2], tok[:, 2])
    renoise = m.generate_long_content(batch={"condition_embed_token": cond, "caption_ids": ids, "seed": SEED}, windows=2,
                                      overlap_cols=13, keep_mode="renoise")["content_token"]
    assert torch.equal(renoise[:, 0], tok[:, 0]) and torch.equal(renoise[:, 1, :65], renoise[:, 0, 200:])
    assert not torch.equal(renoise[:, 1], tok[:, 1])


def test_start_token_and_guidance(carry):
    m, cond, ids, out = carry
    start = synth.synth_tokens(2, mask_frac=0.0, key="long.start").cuda()
    batch = {"condition_embed_token": cond, "caption_ids": ids, "seed": SEED}
    calls = []
    inner = m.transformer.sample
    m.transformer.sample = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    try:
        got = m.generate_long_content(batch=batch, windows=3, overlap_cols=5, start_token=start)["content_token"]
    finally:
        del m.transformer.sample
    assert len(calls) == 2, "a chain ran for the given window"
    assert torch.equal(got[:, 0], start)
    for w in (1, 2):
        assert torch.equal(got[:, w, :25], got[:, w - 1, 240:])
    with pytest.raises(ValueError):
        m.generate_long_content(batch=batch, windows=2, overlap_cols=13, start_token=start[:1])
    null = synth.synth_cond_emb(1, key="long.null")[0].cuda()
    guided = m.generate_long_content(batch=dict(batch, null_condition_embed_token=null), windows=3, overlap_cols=13,
                                     guidance_scale=2.0)["content_token"]
    assert tuple(guided.shape) == (2, 3, L) and int(guided.max()) < 256
    for w in (1, 2):
        assert torch.equal(guided[:, w, :65], guided[:, w - 1, 200:])
    assert not torch.equal(guided, out["content_token"])


# ---- the drivers -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ds():
    from text_to_sound_synthesis_amd import tokenizer as tz
    from text_to_sound_synthesis_amd.config import default_config
    return pipeline.Diffsound(config=default_config(n_layer=2, diffusion_step=10, with_clip=True, bpe_path=tz.CLOSED_VOCAB_PATH),
                              random_vocoder=True)


def test_generate_long_25_seconds(ds, tmp_path):
    captions = synth.synth_captions(2, seed=4)
    samples, frames = 551250, math.ceil(551250 / 256)
    out_dir = str(tmp_path / "long")
    mel01, wave, tokens = ds.generate_long(captions, 25, caption_ids=[0, 1], seed=3, save_root=out_dir)
    W, n, total, s_ = pipeline.long_plan(25)
    assert (W, n, s_) == (4, 13, samples)
    assert tuple(wave.shape) == (2, 1, samples) and tuple(mel01.shape) == (2, 80, frames) and tuple(tokens.shape) == (2, W, L)
    assert bool(torch.isfinite(wave).all()) and bool(torch.isfinite(mel01).all()) and int(tokens.max()) < 256
    for w in range(1, W):
        assert torch.equal(tokens[:, w, :65], tokens[:, w - 1, 200:])
    # the mel is the stitch of the windows' decodes, the waveform ONE vocoder pass over it; both cut after the vocoder
    win = ds.model.decode_to_img(tokens.view(2 * W, L), (2 * W, 256, 5, 53)).view(2, W, 80, 848)
    st = audio.stitch_mel(win, (53 - n) * 16)
    assert st.shape[-1] == total * 16
    assert torch.equal(mel01, ((st + 1) / 2)[:, :, :frames])
    assert torch.equal(mel01, audio.stitch_mel(win, (53 - n) * 16, 0.5, 0.5)[:, :, :frames])
    assert torch.equal(wave, ds.vocoder(st, scale=0.5, shift=0.5)[:, :, :samples])
    assert ds.model.transformer.truncation_r is None and not ds.model.truncation_forward
    assert sorted(os.listdir(out_dir)) == ["000000.npy", "000000.wav", "000001.npy", "000001.wav"]
    x, sr = audio.read_wav(os.path.join(out_dir, "000001.wav"))
    assert sr == 22050 and x.numel() == samples
    assert np.load(os.path.join(out_dir, "000000.npy")).shape == (80, frames)
    # at 48 kHz: the same clip, resampled after the cut
    n48 = math.ceil(samples * 48000 / 22050)
    out48 = str(tmp_path / "long48")
    m48, w48, t48 = ds.generate_long(captions, 25, caption_ids=[0, 1], seed=3, sample_rate=48000, save_root=out48)
    assert torch.equal(t48, tokens) and torch.equal(m48, mel01) and tuple(w48.shape) == (2, 1, n48)
    x, sr = audio.read_wav(os.path.join(out48, "000000.wav"))
    assert sr == 48000 and x.numel() == n48


def test_generate_long_within_one_grid(ds):
    captions = synth.synth_captions(2, seed=4)
    mel01, wave, tokens = ds.generate_long(captions, 5, caption_ids=[0, 1], seed=3)
    assert tuple(tokens.shape) == (2, 1, L) and tuple(wave.shape) == (2, 1, 110250) and tuple(mel01.shape) == (2, 80, 431)
    # the same tokens as the one-grid driver, and its mel up to the cut
    tr = ds.model.transformer
    saved = tr.truncation_r, tr.truncation_k, ds.model.truncation_forward      # that driver installs its rate for good
    try:
        m1, _, t1 = ds.generate_sample_with_condition(captions, caption_ids=[0, 1], seed=3)
    finally:
        tr.truncation_r, tr.truncation_k, ds.model.truncation_forward = saved
    assert torch.equal(tokens[:, 0], t1) and torch.equal(mel01, m1[:, :, :431])


def test_extend_audio(ds, tmp_path):
    g = torch.Generator().manual_seed(33)
    tt = torch.arange(220500) / 22050.0
    rec = torch.stack([0.3 * torch.sin(2 * torch.pi * 440.0 * tt) + 0.05 * torch.randn(220500, generator=g),
                       0.2 * torch.randn(220500, generator=g) * (1.0 + torch.sin(2 * torch.pi * 3.0 * tt))]).cuda()
    captions = synth.synth_captions(2, seed=5)
    want0 = ds.model.prepare_content({"audio": rec})["content_token"]
    out_dir = str(tmp_path / "ext")
    mel01, wave, tokens = ds.extend_audio(rec, captions, 18, caption_ids=[0, 1], seed=3, save_root=out_dir)
    W, n, _, samples = pipeline.long_plan(18)
    assert W == 3 and samples == 396900
    assert tuple(tokens.shape) == (2, W, L) and torch.equal(tokens[:, 0], want0)
    for w in range(1, W):
        assert torch.equal(tokens[:, w, :65], tokens[:, w - 1, 200:])
    assert tuple(wave.shape) == (2, 1, samples) and tuple(mel01.shape) == (2, 80, math.ceil(samples / 256))
    x, sr = audio.read_wav(os.path.join(out_dir, "000000.wav"))
    assert sr == 22050 and x.numel() == samples
    with pytest.raises(ValueError):
        ds.extend_audio(rec, captions, 9.0)


# ---- the vocoder at a long length -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_wave_ref():
    mel = synth.synth_uniform((1, 80, 1712), key="long.voc")
    return mel, O.melgan_generator(synth_sd("generator"), mel)


@pytest.mark.parametrize("precision", ["f16x2", "fp32"])
def test_vocoder_at_1712_frames(long_wave_ref, precision):
    """The other vocoder tests run 53 and 848 frames; a stitched mel of W windows is 848 + (W - 1) 640 frames long (1712 =
    848 + 864: the longest two-window clip, no multiple of any tile of the stack)."""
    from text_to_sound_synthesis_amd.modeling.vocoder import Generator
    mel, ref = long_wave_ref
    voc = Generator(80, 32, 3)
    voc.load_state_dict(synth_sd("generator"))
    voc = voc.cuda().eval()
    voc.conv_precision = precision
    got = voc(mel.cuda()).cpu()
    assert got.shape == ref.shape == (1, 1, 1712 * 256)
    rms = (got - ref).pow(2).mean().sqrt().item()
    line = "vocoder %s at 1712 frames: wave RMS vs oracle %.2e, max %.2e" % (precision, rms, float((got - ref).abs().max()))
    print(line)
    parity_line(line)
    assert rms < WAVE_RMS_TOL
