"""Host side of the resampler (no GPU): the polyphase table of audio.resample_taps against the float64 yardstick
(tests/resample_reference.py), the yardstick against scipy's upfirdn, the filter's design properties, lengths and the
argument errors that must be raised before any library call."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import resample_reference as RR

TO_MODEL = [(48000, 22050), (44100, 22050), (32000, 22050), (24000, 22050), (16000, 22050), (8000, 22050)]
FROM_MODEL = [(22050, 16000), (22050, 32000), (22050, 44100), (22050, 48000)]
RATIOS = TO_MODEL + FROM_MODEL
# L, M, taps per row as the filter's definition gives them (Z = 32, rho = 0.94759...)
SHAPES = {(48000, 22050): (147, 320, 149), (44100, 22050): (1, 2, 137), (32000, 22050): (441, 640, 101),
          (24000, 22050): (147, 160, 75), (16000, 22050): (441, 320, 69), (8000, 22050): (441, 160, 69),
          (22050, 16000): (320, 441, 95), (22050, 32000): (640, 441, 69), (22050, 44100): (2, 1, 69),
          (22050, 48000): (320, 147, 69)}


@pytest.mark.parametrize("src,dst", RATIOS)
def test_table_is_the_float64_formula_rounded_once(src, dst):
    from text_to_sound_synthesis_amd import audio
    taps, L, M, W = audio.resample_taps(src, dst)
    want = RR.table64(src, dst)
    assert (L, M, 2 * W + 1) == SHAPES[(src, dst)]
    assert (L, M) == RR.ratio(src, dst) and W == RR.half_width(src, dst)
    assert taps.dtype == torch.float32 and tuple(taps.shape) == (L, 2 * W + 1) == want.shape
    assert np.array_equal(taps.numpy(), want.astype(np.float32)), "table differs from the float64 formula rounded to f32"
    # DC gain 1 at every phase: the float64 rows' own deviation from 1 + the f32 rounding of 2W+1 terms (each at most half an
    # ulp of its magnitude, summed in float64 here)
    dev64 = float(np.abs(want.sum(1) - 1.0).max())
    rounding = float((np.abs(want) * 2.0 ** -24).sum(1).max())
    dev32 = float(np.abs(taps.numpy().astype(np.float64).sum(1) - 1.0).max())
    print("%d -> %d: L %d M %d W %d, %.0f KB; |row sum - 1| f64 %.2e, f32 %.2e (allowed %.2e)"
          % (src, dst, L, M, W, taps.numel() * 4 / 1024, dev64, dev32, dev64 + rounding))
    assert dev32 <= dev64 + rounding
    assert dev64 < 1e-6


@pytest.mark.parametrize("src,dst", [(44100, 22050), (48000, 22050), (22050, 16000), (22050, 48000), (16000, 22050)])
def test_yardstick_equals_upfirdn(src, dst):
    signal = pytest.importorskip("scipy.signal", reason="scipy is not installed: no second implementation to compare the yardstick to")
    L, M = RR.ratio(src, dst)
    W = RR.half_width(src, dst)
    g = np.random.default_rng(3)
    x = 0.3 * g.standard_normal(6000)
    # the prototype sampled at rate src L: h(m / L), m = -W L .. W L; front-padded so that its delay W L is a whole number of
    # outputs: with d = W L + pad, upfirdn's output q + d / M is y[q]
    proto = RR.h(np.arange(-W * L, W * L + 1), L, RR.cutoff(src, dst))
    pad = (-W * L) % M
    full = signal.upfirdn(np.concatenate([np.zeros(pad), proto]), x, up=L, down=M)
    d = (W * L + pad) // M
    y = RR.resample(x, src, dst)
    assert y.shape[0] == RR.out_length(x.shape[0], src, dst)
    got = full[d:d + y.shape[0]]
    assert got.shape == y.shape
    err = float(np.abs(got - y).max())
    print("%d -> %d: |yardstick - upfirdn| %.2e" % (src, dst, err))
    assert err <= 1e-12


@pytest.mark.parametrize("src,dst", [(48000, 22050), (44100, 22050), (32000, 22050), (22050, 16000)])
def test_design_properties(src, dst):
    """2 s tones through the float64 yardstick: flat to 0.8 x the lower Nyquist, -142 dB at 1.1 x (0.05 dB / 6 dB of margin
    for the 2 s window's own leakage)"""
    ny = min(src, dst) / 2.0
    lv = {f: RR.level_db(RR.resample(RR.tone(f * ny if f > 0 else 440.0, src), src, dst)) for f in (0.0, 0.8, 0.9, 1.1, 1.3)}
    print("%d -> %d: 440 Hz %+.3f dB, 0.8 x %+.3f, 0.9 x %+.3f, 1.1 x %.1f, 1.3 x %.1f" % (src, dst, lv[0.0], lv[0.8], lv[0.9], lv[1.1], lv[1.3]))
    assert abs(lv[0.0]) <= 0.05 and abs(lv[0.8]) <= 0.05
    assert lv[1.1] <= -136.0


def test_lengths_and_identity():
    from text_to_sound_synthesis_amd import audio
    for src, dst in RATIOS:
        L, M = RR.ratio(src, dst)
        W = RR.half_width(src, dst)
        for T in (0, 1, W, 220499, 220500, 480000):
            assert audio.resample_length(T, src, dst) == math.ceil(Fraction(T * L, M)) == RR.out_length(T, src, dst)
    x = torch.zeros(2, 100)
    assert audio.resample(x, 22050, 22050) is x and audio.resample(x, 48000, 48000) is x      # nothing to do, nothing launched
    assert RR.out_length(217088, 22050, 48000) == 472573 and RR.out_length(217088, 22050, 16000) == math.ceil(217088 * 320 / 441)


def test_errors_are_raised_before_any_library_call(monkeypatch):
    from text_to_sound_synthesis_amd import _lib, audio

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    x = torch.zeros(2, 100)
    with pytest.raises(_lib.DiffsoundHipError):          # a host tensor: there is no CPU path
        audio.resample(x, 48000, 22050)
    with pytest.raises(_lib.DiffsoundHipError):
        audio.resample(x, 22050, 22050, n_out=50)
    for bad in ((0, 22050), (22050, -1), (22050.0, 16000), (44100, 22050.5), ("48000", 22050), (True, 22050)):
        with pytest.raises(ValueError):
            audio.resample(x, *bad)
        with pytest.raises(ValueError):
            audio.resample_taps(*bad)
    with pytest.raises(ValueError):
        audio.resample(torch.zeros(100), 48000, 22050)
    with pytest.raises(ValueError):
        audio.resample(x, 48000, 22050, n_out=-1)


def test_read_wav_keeps_its_rate_check(tmp_path):
    from text_to_sound_synthesis_amd import audio
    from text_to_sound_synthesis_amd.pipeline import write_wav_pcm24
    p16 = str(tmp_path / "k16.wav")
    write_wav_pcm24(p16, np.zeros(1600), 16000)
    with pytest.raises(ValueError, match="resample the file first"):
        audio.read_wav(p16, rate=22050)
    x, sr = audio.read_wav(p16)
    assert sr == 16000 and x.numel() == 1600


def test_rate_list_of_the_wrong_length_raises():
    from text_to_sound_synthesis_amd.modeling.melspec import mel_image_from_audio
    clips = [torch.zeros(1000), torch.zeros(1000), torch.zeros(1000)]
    with pytest.raises(ValueError):
        mel_image_from_audio(clips, "cpu", rate=[48000, 16000])
    with pytest.raises(ValueError):
        mel_image_from_audio(clips, "cpu", rate=[48000] * 4)
    for bad in (22050.0, 0, -48000, True):          # a single rate that is not a positive integer
        with pytest.raises(ValueError):
            mel_image_from_audio(clips, "cpu", rate=bad)


def test_a_stated_rate_must_match_the_header(tmp_path):
    from text_to_sound_synthesis_amd.modeling.melspec import mel_image_from_audio
    from text_to_sound_synthesis_amd.pipeline import write_wav_pcm24
    p = str(tmp_path / "k48.wav")
    write_wav_pcm24(p, np.zeros(4800), 48000)
    with pytest.raises(ValueError):
        mel_image_from_audio([p], "cpu", rate=16000)


def test_state_dict_gains_no_key():
    """the resampling table is a cache beside the model, not a buffer of it"""
    from conftest import key_contract
    from text_to_sound_synthesis_amd.config import build_model, default_config
    ref = key_contract()
    sd = set(build_model(default_config(n_layer=19)).state_dict())
    want = set(ref["dalle"]["params"]) | set(ref["dalle"]["buffers"]) | set(ref["encoder"]["params"]) | set(ref["encoder"]["buffers"])
    assert sd == want, sd ^ want
