"""Host side of the audio front end (text_to_sound_synthesis_amd/audio.py, modeling/melspec.py, vocoder.Audio2Mel): the
Slaney filterbank against an independent float64 construction and known answers, the RIFF reader against files written
here, the drop-in's signature and buffers, loud failure on host tensors.  No kernel is launched."""
import inspect
import os
import struct
import sys
import wave as wave_mod

import numpy as np
import pytest
import torch

import audio_reference as R
from conftest import ROOT, parity_line


def test_filterbank_matches_an_independent_float64_construction():
    from text_to_sound_synthesis_amd import audio
    for kw in (dict(fmin=125.0, fmax=7600.0), dict(fmin=0.0, fmax=None)):     # the codec's bank, Audio2Mel's bank
        ours = audio.mel_filterbank(22050, 1024, 80, **kw)
        ref = R.slaney_bank64(22050, 1024, 80, **kw)
        assert ours.dtype == torch.float32 and tuple(ours.shape) == (80, 513)
        # f32 rounding of a float64 value: half an ulp, |x| 2^-24; the two float64 constructions differ by a few 1e-16 relative
        err = (ours.double() - ref).abs()
        assert bool((err <= ref.abs() * 2.0 ** -24 + 1e-12).all()), float(err.max())
        assert bool((ours >= 0).all())
        assert int((ours != 0).sum(0).max()) <= 2, "a bin feeds more than two rows"
        assert bool((ours != 0).any(1).all()), "an empty band"


def test_filterbank_known_answers():
    from text_to_sound_synthesis_amd import audio
    assert float(audio.hz_to_mel(1000.0)) == pytest.approx(15.0, abs=1e-12)
    assert float(audio.mel_to_hz(15.0)) == pytest.approx(1000.0, abs=1e-9)
    assert float(audio.hz_to_mel(500.0)) == pytest.approx(7.5, abs=1e-12)                 # linear part: 200 / 3 Hz per mel
    assert float(audio.mel_to_hz(15.0 + 27.0)) == pytest.approx(6400.0, rel=1e-12)         # 27 log steps = a factor 6.4
    bank = audio.mel_filterbank(22050, 1024, 80, 125.0, 7600.0).double()
    area = bank.sum(1) * (22050 / 1024)          # unit area per band, up to the sampling of a triangle by the FFT bins
    parity_line("mel filterbank 125..7600 Hz: row area x (sr / n_fft) min %.3f (band %d), max %.3f, mean %.4f"
                % (float(area.min()), int(area.argmin()), float(area.max()), float(area.mean())))
    assert 0.90 < float(area.min()) and float(area.max()) < 1.10
    assert abs(float(area[20:].mean()) - 1.0) < 0.01
    # the peak of band j sits at corner j + 1: the first band's at mel(125 Hz) + one step
    step = (float(audio.hz_to_mel(7600.0)) - float(audio.hz_to_mel(125.0))) / 81
    f1 = float(audio.mel_to_hz(float(audio.hz_to_mel(125.0)) + step))
    assert abs(int(bank[0].argmax()) * 22050 / 1024 - f1) <= 22050 / 1024
    rr = audio.row_ranges(bank)
    for j in (0, 40, 79):
        nz = torch.nonzero(bank[j]).flatten()
        assert rr[j].tolist() == [int(nz[0]), int(nz[-1]) + 1]
    assert audio.row_ranges(torch.zeros(2, 513)).tolist() == [[0, 0], [0, 0]]


def test_fft_tables_and_window():
    from text_to_sound_synthesis_amd import audio
    tw = audio.fft_tables()
    assert tuple(tw.shape) == (769, 2) and tw.dtype == torch.float64
    assert tw[0].tolist() == [1.0, 0.0] and tw[128].tolist()[1] == -1.0 and tw[512].tolist() == [1.0, 0.0]
    assert tw[512 + 256].tolist()[1] == -1.0 and abs(tw[512 + 256].tolist()[0]) < 1e-15
    assert torch.equal(audio.hann_window(), torch.hann_window(1024, periodic=True, dtype=torch.float64).float())
    assert audio.n_frames(220500, 512) == 862 and audio.n_frames(217088, 384) == 848 and audio.n_frames(5120, 384) == 20


def _write_wav(path, code, bits, channels, rate, payload):
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(payload)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, code, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits))
        f.write(b"data" + struct.pack("<I", len(payload)) + payload)


def test_read_wav_round_trips(tmp_path):
    from text_to_sound_synthesis_amd import audio
    from text_to_sound_synthesis_amd.pipeline import write_wav_pcm24
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(5000, generator=g) * 1.9 - 0.95).numpy()
    p = str(tmp_path / "a24.wav")
    write_wav_pcm24(p, x, 22050)
    y, sr = audio.read_wav(p)
    assert sr == 22050 and y.dtype == torch.float32 and y.shape == (5000,)
    assert float(np.abs(y.numpy().astype(np.float64) - x.astype(np.float64)).max()) <= 2.0 ** -23
    # PCM_16 written by the standard library's wave module, two channels: averaged
    q = np.round(x[:4000].reshape(-1, 2) * 32767).astype("<i2")
    p16 = str(tmp_path / "a16.wav")
    with wave_mod.open(p16, "wb") as w:
        w.setnchannels(2), w.setsampwidth(2), w.setframerate(16000)
        w.writeframes(q.tobytes())
    y, sr = audio.read_wav(p16)
    assert sr == 16000 and y.shape == (2000,)
    assert np.array_equal(y.numpy(), (q.astype(np.float64) / 32768.0).mean(1).astype(np.float32))
    with pytest.raises(ValueError):
        audio.read_wav(p16, rate=22050)          # no resampling: another rate than the model's raises
    # IEEE float32 and PCM_32 written with struct
    pf = str(tmp_path / "af.wav")
    _write_wav(pf, 3, 32, 1, 22050, x.astype("<f4").tobytes())
    assert np.array_equal(audio.read_wav(pf, rate=22050)[0].numpy(), x.astype(np.float32))
    p32 = str(tmp_path / "a32.wav")
    q32 = np.round(x.astype(np.float64) * (2 ** 31 - 1)).astype("<i4")
    _write_wav(p32, 1, 32, 1, 22050, q32.tobytes())
    assert np.array_equal(audio.read_wav(p32)[0].numpy(), (q32.astype(np.float64) / 2 ** 31).astype(np.float32))
    with pytest.raises(ValueError):
        _write_wav(pf, 1, 8, 1, 22050, b"\0" * 16)
        audio.read_wav(pf)
    bad = str(tmp_path / "bad.wav")
    with open(bad, "wb") as f:
        f.write(b"not a wave file")
    with pytest.raises(ValueError):
        audio.read_wav(bad)


REFERENCE_SIGNATURE = [("n_fft", 1024), ("hop_length", 256), ("win_length", 1024), ("sampling_rate", 22050),
                       ("n_mel_channels", 80), ("mel_fmin", 0.0), ("mel_fmax", None)]


def test_audio2mel_signature_and_buffers():
    from text_to_sound_synthesis_amd.modeling.vocoder import Audio2Mel
    want, names = REFERENCE_SIGNATURE, ["mel_basis", "window"]
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_harness
    if ref_harness.available():       # the reference's own class, where its tree is present: imported, never constructed
        import importlib.util
        import types
        # librosa is the one import of vocoder/modules.py that is not installed; a local stand-in, removed again
        # (ref_harness.install() would also patch Tensor.cuda process-wide, which GPU tests of the same run must not see)
        saved = {n: sys.modules.get(n) for n in ("librosa", "librosa.filters")}
        filt = types.ModuleType("librosa.filters")
        filt.mel = None
        lib_mod = types.ModuleType("librosa")
        lib_mod.filters = filt
        sys.modules.setdefault("librosa", lib_mod)
        sys.modules.setdefault("librosa.filters", filt)
        try:
            spec = importlib.util.spec_from_file_location("_ref_vocoder_modules",
                                                          os.path.join(ref_harness.REF_ROOT, "vocoder", "modules.py"))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            got = [(p.name, p.default) for p in list(inspect.signature(mod.Audio2Mel.__init__).parameters.values())[1:]]
            assert got == REFERENCE_SIGNATURE, got
            src = inspect.getsource(mod.Audio2Mel.__init__)
            assert [n for n in names if 'register_buffer("%s"' % n in src] == names
        finally:
            for name, old in saved.items():
                if old is None:
                    sys.modules.pop(name, None)
    ours = [(p.name, p.default) for p in list(inspect.signature(Audio2Mel.__init__).parameters.values())[1:]]
    assert ours == want
    m = Audio2Mel()
    sd = m.state_dict()
    assert list(sd) == names
    assert tuple(sd["mel_basis"].shape) == (80, 513) and tuple(sd["window"].shape) == (1024,)
    assert sd["mel_basis"].dtype == sd["window"].dtype == torch.float32
    assert torch.equal(sd["window"], torch.hann_window(1024, dtype=torch.float64).float())      # float64, rounded once
    for attr, val in (("n_fft", 1024), ("hop_length", 256), ("win_length", 1024), ("sampling_rate", 22050), ("n_mel_channels", 80)):
        assert getattr(m, attr) == val
    with pytest.raises(NotImplementedError):
        Audio2Mel(n_fft=2048)


def test_host_tensors_raise():
    from text_to_sound_synthesis_amd import _lib
    from text_to_sound_synthesis_amd.modeling.melspec import WaveToMel
    from text_to_sound_synthesis_amd.modeling.vocoder import Audio2Mel
    with pytest.raises(_lib.DiffsoundHipError):
        Audio2Mel()(torch.zeros(1, 1, 5120))
    w2m = WaveToMel()
    assert list(w2m.state_dict()) == []            # nothing of it enters a checkpoint
    with pytest.raises(_lib.DiffsoundHipError):
        w2m.spec01(torch.zeros(1, 220500))
    with pytest.raises(_lib.DiffsoundHipError):
        w2m(torch.zeros(1, 220500))
    with pytest.raises(ValueError):
        w2m(torch.zeros(1, 220500), crop=13)


def test_model_state_dict_is_untouched_by_the_front_end():
    """the audio entry points add no parameter or buffer to the DALLE drop-in"""
    from text_to_sound_synthesis_amd.config import build_model, default_config
    m = build_model(default_config(n_layer=1))
    assert hasattr(m, "content_image")
    assert not any("mel_basis" in k or "window" in k for k in m.state_dict())
    with pytest.raises(KeyError):
        m.content_image({"text": ["x"]})           # neither the content key nor 'audio'
