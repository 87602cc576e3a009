"""Host side of output levelling: the K-weighting coefficients and the segment plan of audio.py against BS.1770-4's own
table, the yardstick (tests/level_reference.py) against the standard's figures, and the argument errors.  No GPU."""
import math

import numpy as np
import pytest
import torch

import level_reference as LR

RATES = [8000, 16000, 22050, 44100, 48000]


def test_kweight_coeffs_reproduce_the_bs1770_table():
    from text_to_sound_synthesis_amd import audio
    c = audio.kweight_coeffs(48000)
    got = list(c["shelf"][0]) + list(c["shelf"][1][1:]) + list(c["highpass"][1][1:])
    err = max(abs(g - w) for g, w in zip(got, LR.BS1770_48K))
    print("kweight_coeffs(48000) vs the seven BS.1770-4 table values: max |diff| %.2e" % err)
    assert err <= 1e-12
    assert c["shelf"][1][0] == 1.0 and list(c["highpass"][0]) == [1.0, -2.0, 1.0] and c["highpass"][1][0] == 1.0
    for rate in RATES:                                  # and the yardstick's own coefficients are the same numbers
        c = audio.kweight_coeffs(rate)
        shelf, hp = LR.kweight(rate)
        assert np.allclose(list(c["shelf"][0]) + list(c["shelf"][1][1:]), shelf, rtol=1e-15, atol=0)
        assert np.allclose(c["highpass"][1][1:], hp, rtol=1e-15, atol=0)
        assert all(v.dtype == np.float64 for pair in c.values() for v in pair)


def test_reference_full_scale_sine_is_minus_3_01():
    y = LR.kweighted(LR.sine(997.0, 48000, 10.0), 48000)
    L = LR.loudness_from(y, 48000)
    print("997 Hz full scale, 10 s at 48 kHz: %.4f LUFS" % L)
    assert abs(L - (-3.01)) <= 0.01
    L22 = LR.loudness_from(LR.kweighted(LR.sine(997.0, 22050, 3.0), 22050), 22050)
    assert abs(L22 - (-2.981)) <= 0.01


def test_reference_gating_case():
    fs = 22050
    clip, loud = LR.gating_clip(fs)
    S = LR.segment_samples(fs)
    y = LR.kweighted(clip, fs)
    z = LR.blocks(LR.segment_energies(y, S), S)
    L, A, G, rel = LR.gate(z)
    ungated = LR.ungated_loudness(y, fs)
    alone = LR.loudness_from(LR.kweighted(loud, fs), fs)
    print("gating case: gated %.3f, ungated %.3f, the loud third alone %.3f LUFS; |A| %d, |G| %d of %d blocks"
          % (L, ungated, alone, int(A.sum()), int(G.sum()), z.size))
    assert abs(L - (-17.45)) <= 0.01 and abs(ungated - (-21.98)) <= 0.01 and abs(alone - (-17.11)) <= 0.01
    assert abs(L - ungated) > 0.3 and abs(L - alone) > 0.3 and abs(ungated - alone) > 0.3
    assert 0 < int(G.sum()) < int(A.sum()) < z.size                  # both gates take blocks away
    for thr in (LR.GAMMA_ABS, rel):                                     # no block sits on a threshold
        assert float(np.min(np.abs(z - thr) / thr)) > 1e-6


@pytest.mark.parametrize("rate", RATES)
def test_level_plan(rate):
    from text_to_sound_synthesis_amd import audio
    plan = audio.level_plan(rate)
    S = plan["S"]
    assert S == int(math.floor(0.1 * rate + 0.5)) == LR.segment_samples(rate) and plan["block"] == 4 * S
    assert S == {8000: 800, 16000: 1600, 22050: 2205, 44100: 4410, 48000: 4800}[rate]
    P = plan["transition"]
    assert P.shape == (4, 4) and P.dtype == np.float64 and np.isfinite(P).all()
    # P carries the state over a segment: the filter run over 2 S samples = run over S, then over S more from the carried state
    rng = np.random.default_rng(rate)
    x = rng.standard_normal(2 * S)
    (b0, b1, b2, a1, a2), (c1, c2) = LR.kweight(rate)

    def run(x, s):
        s1, s2, t1, t2 = s
        for xv in x.tolist():
            y1 = b0 * xv + s1
            s1 = b1 * xv - a1 * y1 + s2
            s2 = b2 * xv - a2 * y1
            y2 = y1 + t1
            t1 = t2 - 2.0 * y1 - c1 * y2
            t2 = y1 - c2 * y2
        return np.array([s1, s2, t1, t2])

    zero = (0.0, 0.0, 0.0, 0.0)
    whole = run(x, zero)
    first, second = run(x[:S], zero), run(x[S:], zero)
    carried = P @ first + second
    assert np.abs(carried - whole).max() <= 1e-9 * max(1.0, np.abs(whole).max())
    assert np.abs(P).max() < 1e-3                                       # a segment forgets nearly all of its start state


def test_strategy_and_argument_errors():
    from text_to_sound_synthesis_amd import _lib, audio
    x = torch.zeros(2, 22050)
    for bad_rate in (22050.0, 0, -1, True, "22050", None):
        with pytest.raises(ValueError):
            audio.kweight_coeffs(bad_rate)
        with pytest.raises(ValueError):
            audio.level_plan(bad_rate)
        with pytest.raises(ValueError):
            audio.measure_level(x, bad_rate)
        with pytest.raises(ValueError):
            audio.level(x, bad_rate, "peak")
    with pytest.raises(ValueError):
        audio.level(x, 22050, "lufs")
    with pytest.raises(ValueError):
        audio.level(x, 22050, "match")                                  # no reference
    with pytest.raises(ValueError):
        audio.level(x, 22050, "peak", reference=(x, 22050))             # a reference without "match"
    with pytest.raises(ValueError):
        audio.level(x, 22050, "peak", target=float("nan"))
    with pytest.raises(ValueError):
        audio.level(x, 22050, "peak", ceiling_db=float("inf"))
    with pytest.raises(ValueError):
        audio.level(torch.zeros(22050), 22050, "peak")                  # not [B, T]
    with pytest.raises(_lib.DiffsoundHipError):                         # a host tensor: there is no CPU path
        audio.level(x, 22050, "peak")
    with pytest.raises(_lib.DiffsoundHipError):
        audio.measure_level(x, 22050)
    assert set(audio.LEVEL_STRATEGIES) == {"peak", "rms", "loudness", "match"}
    assert (audio.LEVEL_STRATEGIES["peak"], audio.LEVEL_STRATEGIES["rms"], audio.LEVEL_STRATEGIES["loudness"]) == (-1.0, -20.0, -23.0)


def test_driver_level_keyword_is_checked_before_anything_runs():
    from text_to_sound_synthesis_amd import pipeline
    assert pipeline.level_spec(None, False) is None
    assert pipeline.level_spec("loudness", False) == {"strategy": "loudness", "target": None, "ceiling_db": -1.0}
    assert pipeline.level_spec({"strategy": "rms", "target": -18}, False) == {"strategy": "rms", "target": -18.0, "ceiling_db": -1.0}
    assert pipeline.level_spec("match", True)["strategy"] == "match"
    for bad in ("match", "loud", {"target": -3.0}, {"strategy": "peak", "gain": 2.0}, 3, {"strategy": "match", "target": -20.0}):
        with pytest.raises(ValueError):
            pipeline.level_spec(bad, False)
