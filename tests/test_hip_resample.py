"""The resampler on the GPU: ds_resample (csrc/resample.hip) behind audio.resample, melspec.mel_image_from_audio(rate=),
batch['audio_rate'] and the drivers' sample_rate.  GPU only (-m gpu).

Yardstick (tests/resample_reference.py, never the code under test): the defining sum with numpy in float64; beside it the
same sum in float32 (f32 table, f32 products, f32 running sum), whose distance to float64 on a case is that case's d32.

Bound per case:  |kernel - float64|_max <= 4 x d32 of that case (the margin the front-end tests give a different summation
order) and never above 1e-4, the project's waveform tolerance applied to the largest element.  No element is left out;
silence has d32 = 0 and must come out as exact zeros."""
import json
import math
import os

import numpy as np
import pytest
import torch

import audio_reference as R
import resample_reference as RR
from conftest import GOLDEN, golden, parity_line, synth_sd
from text_to_sound_synthesis_amd import synth

pytestmark = pytest.mark.gpu
NO_GRAD = True

FACTOR = 4.0
WAVE_TOL = 1e-4
MEL_TOL = 1e-3
RATIOS = [(48000, 22050), (44100, 22050), (32000, 22050), (24000, 22050), (16000, 22050), (8000, 22050),
          (22050, 16000), (22050, 32000), (22050, 44100), (22050, 48000)]
INPUT_NAMES = ["noise_0.3", "noise_1e-3", "bursts", "chirp", "tone_440", "silence"]


def _check(tag, got, x, src, dst, n_out=None):
    """got (device, [n]) against the yardstick of host x; asserts the bound on every element; returns (err, d32)"""
    x = np.asarray(x, dtype=np.float32)
    r64 = RR.resample(x, src, dst, np.float64, n_out)
    r32 = RR.resample(x, src, dst, np.float32, n_out)
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == r64.shape, (got.shape, r64.shape)
    assert np.isfinite(got).all()
    d32 = float(np.abs(r32.astype(np.float64) - r64).max()) if r64.size else 0.0
    err = float(np.abs(got - r64).max()) if r64.size else 0.0
    line = "%s: |kernel - f64| %.2e, bound %.2e = 4 x d32 %.2e, peak %.2e" % (tag, err, FACTOR * d32, d32, float(np.abs(r64).max()) if r64.size else 0.0)
    print(line)
    parity_line("resample " + line)
    assert err <= FACTOR * d32, line
    assert err <= WAVE_TOL, line
    return err, d32


@pytest.mark.parametrize("name", INPUT_NAMES)
@pytest.mark.parametrize("src,dst", RATIOS)
def test_six_inputs_vs_float64(src, dst, name):
    """10 s of every input of audio_reference.make_inputs generated at the source rate, every ratio.
    The measured figures are in DESIGN.md section 8 (resampler parity)."""
    from text_to_sound_synthesis_amd import audio
    x = R.make_inputs(n=10 * src)[name]
    got = audio.resample(x[None].cuda(), src, dst)
    assert tuple(got.shape) == (1, RR.out_length(10 * src, src, dst))
    _check("%d -> %d %s" % (src, dst, name), got[0], x.numpy(), src, dst)
    if name == "silence":
        assert float(got.abs().max()) == 0.0


def test_generated_clips_up_and_down():
    """wave_full of the committed chain golden, 22 050 -> 48 000 -> 22 050, each stage against the yardstick of its own input"""
    from text_to_sound_synthesis_amd import audio
    w = golden("traj_T100_L19")["wave_full"].float()
    assert tuple(w.shape) == (2, 217088)
    up = audio.resample(w.cuda(), 22050, 48000)
    assert tuple(up.shape) == (2, 472573)
    down = audio.resample(up, 48000, 22050)
    assert tuple(down.shape) == (2, RR.out_length(472573, 48000, 22050))
    for i in range(2):
        _check("wave_full[%d] 22050 -> 48000" % i, up[i], w[i].numpy(), 22050, 48000)
        _check("wave_full[%d] 48000 -> 22050" % i, down[i], up[i].cpu().numpy(), 48000, 22050)
    # the round trip keeps the band below 0.9475 x 11 025 Hz: away from the ends it is the clip again
    rt = float((down[:, 2000:215000].cpu() - w[:, 2000:215000]).abs().max())
    parity_line("resample wave_full 22050 -> 48000 -> 22050 vs itself (samples 2000..215000): max %.2e, peak %.2f" % (rt, float(w.abs().max())))


@pytest.mark.parametrize("src,dst", [(48000, 22050), (22050, 16000)])
def test_stop_band_on_the_device(src, dst):
    """a 2 s tone of amplitude 0.5 at 1.1 x the lower Nyquist: what is left of it (RMS of the middle 80 %, relative to the
    tone) may be at most the float32 yardstick's own level for the same tone + 6 dB (a factor 2 for the summation order).
    The measured levels are in DESIGN.md section 1 (the `ds_resample` row)."""
    from text_to_sound_synthesis_amd import audio
    x = RR.tone(1.1 * min(src, dst) / 2.0, src).astype(np.float32)
    lv64 = RR.level_db(RR.resample(x, src, dst, np.float64))
    lv32 = RR.level_db(RR.resample(x, src, dst, np.float32))
    got = audio.resample(torch.from_numpy(x)[None].cuda(), src, dst)[0].cpu().numpy()
    lv = RR.level_db(got)
    line = "%d -> %d stop band at 1.1 x Nyquist: kernel %.1f dB, float32 yardstick %.1f dB, float64 %.1f dB" % (src, dst, lv, lv32, lv64)
    print(line)
    parity_line("resample " + line)
    assert lv <= lv32 + 6.0, line


def test_lengths_and_n_out():
    """rows of different length in one launch = the same rows alone, bit for bit; exact zeros past ceil(len L / M); n_out
    smaller and larger than N"""
    from text_to_sound_synthesis_amd import audio
    g = torch.Generator().manual_seed(5)
    src, dst = 48000, 22050
    T = 100000
    x = (0.3 * torch.randn(4, T, generator=g)).cuda()
    lens = [T, 1, 37777, 0]
    N = RR.out_length(T, src, dst)
    full = audio.resample(x, src, dst, lengths=lens)
    assert tuple(full.shape) == (4, N)
    for i, n in enumerate(lens):
        ni = RR.out_length(n, src, dst)
        alone = audio.resample(x[i:i + 1, :n].contiguous(), src, dst, n_out=N) if n else torch.zeros(1, N).cuda()
        assert torch.equal(alone[0], full[i]), "row %d (length %d)" % (i, n)
        if ni < N:
            assert float(full[i, ni:].abs().max()) == 0.0
        _check("48000 -> 22050 length %d of %d" % (n, T), full[i], x[i, :n].cpu().numpy(), src, dst, n_out=N)
    for n_out in (1, 1000, N - 1, N + 1, 220500):
        y = audio.resample(x, src, dst, lengths=torch.tensor(lens, dtype=torch.int32).cuda(), n_out=n_out)
        assert tuple(y.shape) == (4, n_out)
        m = min(n_out, N)
        assert torch.equal(y[:, :m], full[:, :m])
        if n_out > N:
            assert float(y[:, N:].abs().max()) == 0.0
    # equal rates: nothing is filtered; n_out / lengths zero-extend or cut
    same = audio.resample(x, 22050, 22050, lengths=lens, n_out=T + 5)
    assert torch.equal(same[0, :T], x[0]) and float(same[0, T:].abs().max()) == 0.0 and float(same[3].abs().max()) == 0.0
    assert torch.equal(same[2, :37777], x[2, :37777]) and float(same[2, 37777:].abs().max()) == 0.0
    assert audio.resample(x, 48000, 48000) is x


def test_argument_errors_launch_nothing():
    from text_to_sound_synthesis_amd import _lib, audio
    x, y = torch.zeros(2, 1000).cuda(), torch.zeros(2, 500).cuda()
    taps = audio.resample_taps(44100, 22050)[0].cuda()
    L_ = _lib.lib()
    ok = lambda **k: dict(dict(x=_lib.ptr(x), B=2, T=1000, lengths=None, L=1, M=2, taps=_lib.ptr(taps), W=68, y=_lib.ptr(y), n_out=500), **k)
    call = lambda a: L_.ds_resample(a["x"], a["B"], a["T"], a["lengths"], a["L"], a["M"], a["taps"], a["W"], a["y"], a["n_out"], _lib.stream())
    assert call(ok()) == 0 and call(ok(n_out=0)) == 0
    for bad in (dict(L=0), dict(M=0), dict(L=2, M=4), dict(W=0), dict(n_out=-1), dict(x=None), dict(taps=None), dict(y=None), dict(B=0)):
        assert call(ok(**bad)) != 0, bad
        with pytest.raises(_lib.DiffsoundHipError):
            _lib.check(call(ok(**bad)))
    with pytest.raises(_lib.DiffsoundHipError):
        audio.resample(torch.zeros(1, 100), 48000, 22050)
    torch.cuda.synchronize()


@pytest.mark.parametrize("B", [1, 3, 64])
def test_batch_position_and_run_invariance(B):
    """clip i of a batch is bit-equal to the same clip run alone, and two runs are bit-equal"""
    from text_to_sound_synthesis_amd import audio
    g = torch.Generator().manual_seed(100 + B)
    for src, dst, T in ((48000, 22050, 480000), (22050, 48000, 217088), (44100, 22050, 100001)):
        w = (0.2 * torch.randn(B, T, generator=g)).cuda()
        if B > 1:
            w[1] *= 1e-3
            w[B - 1, T // 4:] = 0
        full, again = audio.resample(w, src, dst), audio.resample(w, src, dst)
        assert torch.equal(full, again)
        for i in sorted({0, 1 % B, B // 2, B - 1}):
            assert torch.equal(audio.resample(w[i:i + 1], src, dst)[0], full[i]), "clip %d of %d, %d -> %d" % (i, B, src, dst)


def _quantise24(x):
    """what write_wav_pcm24 + read_wav do to a float waveform"""
    return (torch.clamp(torch.round(x.double() * 8388608.0), -8388608, 8388607) / 8388608.0).float()


def _mel_refs(x, src, bank):
    """host x f32[T] at `src` Hz -> (float64 route, float32 route) of the codec image: the yardstick resampler to 220 500
    samples at 22 050 Hz, then the front end's formula, each in its own precision"""
    y64 = torch.from_numpy(RR.resample(x.numpy(), src, 22050, np.float64, n_out=220500))
    y32 = torch.from_numpy(RR.resample(x.numpy(), src, 22050, np.float32, n_out=220500))
    return R.codec_image(y64[None], torch.float64, 6, bank), R.codec_image(y32[None], torch.float32, 6, bank)


def test_mel_from_audio_at_other_rates(tmp_path):
    """mel_image_from_audio of 48 kHz and 16 kHz renderings -- a device tensor + rate=, and `.wav` files of mixed rates in
    one list -- against codec_image(float64 yardstick resample(x)): per input within 4 x max(the float32 route's own
    distance on it, on the broadband inputs) and the 1e-3 mel tolerance; broadband inputs and the chirp, as
    test_hip_audio.py does (the chirp's own float32 distance is large: the cap binds there)."""
    from text_to_sound_synthesis_amd.modeling.melspec import WaveToMel, mel_image_from_audio
    from text_to_sound_synthesis_amd.pipeline import write_wav_pcm24
    bank = R.slaney_bank64(fmin=125.0, fmax=7600.0)
    names = ["noise_0.3", "noise_1e-3", "chirp"]
    paths, file_refs = [], []
    for src in (48000, 16000):
        ins = R.make_inputs(n=10 * src)
        refs = {n: _mel_refs(ins[n], src, bank) for n in names}
        d32 = {n: float((refs[n][1].double() - refs[n][0]).abs().max()) for n in names}
        bb = max(d32[n] for n in R.BROADBAND)
        got = mel_image_from_audio(torch.stack([ins[n] for n in names]).cuda(), "cuda", rate=src)
        assert tuple(got.shape) == (3, 1, 80, 848)
        for i, n in enumerate(names):
            err = float((got[i:i + 1].cpu().double() - refs[n][0]).abs().max())
            bound = FACTOR * max(d32[n], bb)
            line = "mel of %d Hz %s: |kernel - f64| %.2e, bound %.2e = 4 x max(d32 %.2e, broadband %.2e)" % (src, n, err, bound, d32[n], bb)
            print(line)
            parity_line("resample " + line)
            assert err <= bound and err <= MEL_TOL, line
        # the same clips as PCM_24 files: the reference sees the quantised samples
        for n in names[:2]:
            paths.append(str(tmp_path / ("%s_%d.wav" % (n, src))))
            write_wav_pcm24(paths[-1], ins[n].numpy(), src)
            r64, r32 = _mel_refs(_quantise24(ins[n]), src, bank)
            file_refs.append((r64, max(float((r32.double() - r64).abs().max()), bb), "%d Hz %s" % (src, n)))
    w22 = R.make_inputs()["noise_0.3"]
    paths.append(str(tmp_path / "noise_22050.wav"))
    write_wav_pcm24(paths[-1], w22.numpy(), 22050)
    r64 = R.codec_image(_quantise24(w22)[None], torch.float64, 6, bank)
    r32 = R.codec_image(_quantise24(w22)[None], torch.float32, 6, bank)
    file_refs.append((r64, float((r32.double() - r64).abs().max()), "22050 Hz noise_0.3"))
    got = mel_image_from_audio(paths, "cuda")
    assert tuple(got.shape) == (len(paths), 1, 80, 848)
    for i, (r64, d, tag) in enumerate(file_refs):
        err = float((got[i:i + 1].cpu().double() - r64).abs().max())
        line = "mel of a .wav file, %s, in a list of mixed rates: |kernel - f64| %.2e, bound %.2e" % (tag, err, FACTOR * d)
        print(line)
        parity_line("resample " + line)
        assert err <= FACTOR * d and err <= MEL_TOL, line
    # a 22 050 Hz batch through the new arguments is the front end as it was, bit for bit
    w = torch.stack([w22, R.make_inputs()["chirp"]]).cuda()
    want = WaveToMel().cuda()(w)
    assert torch.equal(mel_image_from_audio(w, "cuda", rate=22050), want)
    assert torch.equal(mel_image_from_audio(w, "cuda", rate=[22050, 22050]), want)
    assert torch.equal(mel_image_from_audio(w, "cuda"), want)
    assert torch.equal(mel_image_from_audio([x for x in w.cpu()], "cuda", rate=22050), want)


def _build_model():
    from text_to_sound_synthesis_amd import tokenizer as tz
    from text_to_sound_synthesis_amd.config import build_model, default_config
    m = build_model(default_config(n_layer=2, diffusion_step=100, with_clip=True, bpe_path=tz.CLOSED_VOCAB_PATH))
    with open(os.path.join(GOLDEN, "state_dict_keys_clip.json")) as f:
        clip_sd = synth.synth_state_dict(json.load(f))
    sd = {**synth_sd("dalle", 2), **synth_sd("encoder"), **clip_sd}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected
    m = m.cuda().eval()
    dt = m.transformer
    dt.auxiliary_loss_weight, dt.adaptive_auxiliary_loss, dt.mask_weight = 5.0e-4, True, [1, 1]
    return m


@pytest.fixture(scope="module")
def model():
    return _build_model()


def _clips_48k(B=3):
    """B clips at 48 kHz: the golden's generated waves resampled up on the device, and noise"""
    from text_to_sound_synthesis_amd import audio
    w = golden("traj_T100_L19")["wave_full"].float()
    g = torch.Generator().manual_seed(21)
    clips = torch.stack([w[0], w[1], 0.1 * torch.randn(217088, generator=g)][:B])
    return audio.resample(clips.cuda(), 22050, 48000)


def test_entry_points_accept_a_rate(model, tmp_path):
    from text_to_sound_synthesis_amd import audio
    from text_to_sound_synthesis_amd.modeling.melspec import mel_image_from_audio
    from text_to_sound_synthesis_amd.modeling.train import training_inputs
    from text_to_sound_synthesis_amd.pipeline import write_wav_pcm24
    w48 = _clips_48k()
    w22 = audio.resample(w48, 48000, 22050)
    a = model.prepare_content({"audio": w22})
    b = model.prepare_content({"audio": w48, "audio_rate": 48000})
    c = model.prepare_content({"audio": w48, "audio_rate": [48000, 48000, 48000]})
    for o in (b, c):
        assert torch.equal(o["content_token"], a["content_token"]) and torch.equal(o["content_quant"], a["content_quant"])
    assert torch.equal(model.content_image({"audio": w48, "audio_rate": 48000}), mel_image_from_audio(w48, "cuda", rate=48000))
    # 48 kHz files, read with their own header rate, against the same (quantised) clips resampled by audio.resample
    paths = []
    for i, x in enumerate(w48.cpu()):
        paths.append(str(tmp_path / ("c%d.wav" % i)))
        write_wav_pcm24(paths[-1], x.numpy(), 48000)
    d = model.prepare_content({"audio": paths})
    q22 = audio.resample(_quantise24(w48.cpu()).cuda(), 48000, 22050)
    e = model.prepare_content({"audio": q22})
    assert torch.equal(d["content_token"], e["content_token"])
    # mixed rates in one device batch
    mixed = torch.zeros(2, w48.shape[1]).cuda()
    mixed[0], mixed[1, :w22.shape[1]] = w48[0], w22[1]
    f = model.prepare_content({"audio": mixed, "audio_rate": [48000, 22050]})
    assert torch.equal(f["content_token"], a["content_token"][:2])
    captions = synth.synth_captions(3, seed=1)
    g1, g2 = (torch.Generator(device="cuda").manual_seed(7) for _ in range(2))
    x_a = training_inputs(model, {"audio": w48, "audio_rate": 48000, "text": captions}, generator=g1)
    x_i = training_inputs(model, {"audio": w22, "text": captions}, generator=g2)
    for u, v in zip(x_a, x_i):
        assert torch.equal(u, v)
    out = model.sample({"audio": w48[:1], "audio_rate": 48000, "text": captions[:1]}, filter_ratio=[0.1], return_rec=True)
    assert torch.equal(out["input_image"], mel_image_from_audio(w22[:1], "cuda"))


def test_solver_step_with_a_rate(model):
    from text_to_sound_synthesis_amd import audio
    from text_to_sound_synthesis_amd.modeling.solver import GradClipWindow, Solver
    from text_to_sound_synthesis_amd.modeling.train import TrainStep
    dt = model.transformer
    keep = {k: v.detach().clone() for k, v in dt.state_dict().items()}
    w48 = _clips_48k()
    w22 = audio.resample(w48, 48000, 22050)
    captions = synth.synth_captions(3, seed=2)
    losses = []
    try:
        for batch in ({"audio": w48, "audio_rate": 48000, "text": captions}, {"audio": w22, "text": captions}):
            gen = torch.Generator(device="cuda").manual_seed(99)
            solver = Solver(TrainStep(dt, precision="f16x2"), lr=1e-4, clip_grad_norm=GradClipWindow(0, 5000, 0.5), model=model,
                            generator=gen)
            losses.append(float(solver.step(batch)["loss"]))
            dt.load_state_dict(keep)
            dt.transformer.invalidate()
    finally:
        dt.load_state_dict(keep)
        dt.transformer.invalidate()
    assert math.isfinite(losses[0]) and losses[0] > 0 and losses[0] == losses[1], losses


def test_drivers_at_other_rates(tmp_path):
    from text_to_sound_synthesis_amd import audio
    from text_to_sound_synthesis_amd import tokenizer as tz
    from text_to_sound_synthesis_amd.config import default_config
    from text_to_sound_synthesis_amd.pipeline import Diffsound
    ds = Diffsound(config=default_config(n_layer=2, diffusion_step=100, with_clip=True, bpe_path=tz.CLOSED_VOCAB_PATH),
                   random_vocoder=True)
    captions = synth.synth_captions(2, seed=3)
    w16 = audio.resample(_clips_48k(2), 48000, 16000)
    mel01, wave, tokens = ds.generate_sample_from_audio(w16, captions, filter_ratio=0.2, audio_rate=16000)
    assert tuple(mel01.shape) == (2, 80, 848) and tuple(wave.shape) == (2, 1, 217088) and tuple(tokens.shape) == (2, 265)
    assert bool(torch.isfinite(wave).all())
    # caption ids select the in-kernel per-caption noise: with them the seed fixes the clips
    m0, wv0, t0 = ds.generate_sample_with_condition(captions, caption_ids=[0, 1], seed=11)
    m1, wv1, t1 = ds.generate_sample_with_condition(captions, caption_ids=[0, 1], seed=11, sample_rate=48000)
    assert tuple(wv0.shape) == (2, 1, 217088) and tuple(wv1.shape) == (2, 1, 472573)
    assert torch.equal(t0, t1) and torch.equal(m0, m1)
    assert torch.equal(wv1[:, 0], audio.resample(wv0[:, 0], 22050, 48000))
    m2, wv2, _ = ds.generate_sample_with_condition(captions, caption_ids=[0, 1], seed=11, sample_rate=22050)
    assert torch.equal(wv2, wv0)
    tsv = str(tmp_path / "val.csv")
    with open(tsv, "w") as f:
        f.write("file_name,caption\nclip_a.wav,%s\n" % captions[0].replace(",", " "))
    out = str(tmp_path / "out")
    written = ds.generate_sample(tsv, 0.85, out, replicate=1, sample_rate=16000)
    assert len(written) == 1
    x, sr = audio.read_wav(written[0] + ".wav")
    assert sr == 16000 and x.numel() == math.ceil(217088 * 320 / 441) == RR.out_length(217088, 22050, 16000)
    assert np.load(written[0] + ".npy").shape == (80, 848)
