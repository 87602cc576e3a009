"""Host side of the look-ahead limiter: audio.limit_plan, the `limit` key of the drivers' level keyword, and the yardstick's
(tests/limit_reference.py) own properties on the cases the definition was prototyped on.  No GPU."""
import math

import numpy as np
import pytest
import torch

import level_reference as LR
import limit_reference as MR

FS = 22050
CASES = [("click_tone", 12.0), ("noise_0.3", 6.0), ("bursts", 12.0), ("tone_fs4", 6.0), ("tone_60", 6.0), ("noise_0.3", 12.0)]


def test_limit_plan():
    from text_to_sound_synthesis_amd import audio
    for rate, L in ((16000, 24), (22050, 33), (48000, 72)):
        p = audio.limit_plan(rate)
        assert set(p) == {"L", "a", "w"} and p["L"] == L == MR.plan(rate)[0]
        w = p["w"]
        assert w.dtype == np.float64 and w.shape == (L + 1,) and (w >= 0.0).all() and (w > 0.0).all()
        assert np.array_equal(w, w[::-1]) and abs(float(np.sum(w)) - 1.0) <= 1e-15 and abs(math.fsum(w) - 1.0) <= 1e-15
        assert np.array_equal(w, MR.plan(rate)[2])
        assert isinstance(p["a"], float) and p["a"] == math.exp(-1000.0 / (50.0 * rate)) == MR.plan(rate)[1]
    p = audio.limit_plan(22050, lookahead_ms=5.0, release_ms=200.0)
    assert p["L"] == 110 and p["a"] == math.exp(-1000.0 / (200.0 * 22050))
    assert audio.limit_plan(22050, lookahead_ms=9.97)["L"] == 220        # = floor(0.01 fs): the last one allowed
    with pytest.raises(ValueError):
        audio.limit_plan(22050, lookahead_ms=10.0)                       # rounds to 221 > 0.01 fs
    assert audio.limit_plan(48000, lookahead_ms=10.0)["L"] == 480
    assert audio.LIMIT_BLOCK == 1024
    for bad in (dict(lookahead_ms=0.0), dict(lookahead_ms=0.01), dict(lookahead_ms=10.1), dict(lookahead_ms=-1.0),
                dict(lookahead_ms=float("nan")), dict(release_ms=0.0), dict(release_ms=-5.0), dict(release_ms=float("inf"))):
        with pytest.raises(ValueError):
            audio.limit_plan(22050, **bad)
    with pytest.raises(ValueError):
        audio.limit_plan(200000, lookahead_ms=10.0)                      # 2000 samples: past the kernels' block
    for bad_rate in (22050.0, 0, -1, True, None):
        with pytest.raises(ValueError):
            audio.limit_plan(bad_rate)


def test_limit_and_level_argument_errors():
    from text_to_sound_synthesis_amd import _lib, audio
    x = torch.zeros(2, 22050)
    with pytest.raises(_lib.DiffsoundHipError):                         # a host tensor: there is no CPU path
        audio.limit(x, 22050)
    with pytest.raises(_lib.DiffsoundHipError):
        audio.level(x, 22050, "loudness", limit=True)
    with pytest.raises(ValueError):
        audio.limit(x, 22050, ceiling_db=float("inf"))
    with pytest.raises(ValueError):
        audio.limit(x, 22050, lookahead_ms=20.0)
    with pytest.raises(ValueError):
        audio.limit(torch.zeros(22050), 22050)
    for bad in ("yes", 1.5, {"lookahead": 1.0}, {"lookahead_ms": 1.0, "attack_ms": 2.0}):
        with pytest.raises(ValueError):
            audio.level(x, 22050, "peak", limit=bad)
    with pytest.raises(ValueError):
        audio.level(x, 22050, "peak", limit={"lookahead_ms": 50.0})


def test_level_spec_with_and_without_limit():
    from text_to_sound_synthesis_amd import pipeline
    assert pipeline.level_spec("loudness", False) == {"strategy": "loudness", "target": None, "ceiling_db": -1.0}
    assert pipeline.level_spec({"strategy": "rms", "target": -18}, False) == {"strategy": "rms", "target": -18.0, "ceiling_db": -1.0}
    assert pipeline.level_spec({"strategy": "loudness", "target": -14, "limit": True}, False) == {
        "strategy": "loudness", "target": -14.0, "ceiling_db": -1.0, "limit": True}
    d = {"lookahead_ms": 3.0, "release_ms": 100.0}
    assert pipeline.level_spec({"strategy": "match", "limit": d}, True) == {
        "strategy": "match", "target": None, "ceiling_db": -1.0, "limit": d}
    assert pipeline.level_spec({"strategy": "peak", "limit": None}, False)["limit"] is None
    for bad in ({"strategy": "peak", "limit": "hard"}, {"strategy": "peak", "limit": {"knee": 1.0}}, {"strategy": "peak", "gain": 2.0},
                {"limit": True}):
        with pytest.raises(ValueError):
            pipeline.level_spec(bad, False)


@pytest.mark.parametrize("name,over_db", CASES)
def test_yardstick_properties(name, over_db):
    """the definition's own promises, on the float64 yardstick: the smoothed reduction is never below the wanted one, the
    sample peak lands on or under the ceiling, the x4 true peak overshoots by a fraction of a per cent before the trim and
    not at all after it"""
    x = MR.inputs(FS, FS)[name]
    g0 = MR.pre_gain(x, FS, over_db)
    r = MR.limit(x, FS, g0)
    c = r["c"]
    assert (r["s"] >= r["d"] - 2.0 ** -52).all()
    assert (r["g"] <= 1.0).all() and (r["g"] >= 0.0).all() and float(r["g"].min()) < 1.0
    assert float(np.abs(r["pre"]).max()) <= c * (1.0 + 2.0 ** -21)      # four fp32 roundings: g0, g, g0 g and the product
    assert r["true_peak"] <= c * 1.002 and r["trim"] <= 1.0
    assert float(np.abs(r["out"]).max()) <= c * (1.0 + 2.0 ** -22)      # two: the trim and the product
    assert LR.true_peak(r["out"], FS) <= c * (1.0 + 2.0 ** -22)
    print("%s +%g dB: min g %.4f, true peak before the trim / c - 1 = %+.2e, trim %.6f"
          % (name, over_db, float(r["g"].min()), r["true_peak"] / c - 1.0, r["trim"]))


def test_yardstick_leaves_a_row_under_the_ceiling_alone():
    for name in ("noise_0.3", "click_tone", "tone_fs4"):
        x = MR.inputs(FS, 4000)[name]
        g0 = MR.pre_gain(x, FS, -0.01)                                   # the true peak a hair under the ceiling
        r = MR.limit(x, FS, g0)
        assert (r["g"] == 1.0).all() and (r["d"] == 0.0).all() and r["trim"] == 1.0
        assert np.array_equal(r["out"], np.float32(g0) * x)
    r = MR.limit(np.zeros(500, np.float32), FS, 3.0)
    assert (r["g"] == 1.0).all() and not r["out"].any()


def test_a_peak_at_the_first_sample_is_met_fully_smoothed():
    """the hold starts at -L: at sample 0 the curve already stands where the peak needs it"""
    x = np.zeros(3000, np.float32)
    x[0] = 0.9
    g0 = MR.pre_gain(x, FS, 12.0)
    r = MR.limit(x, FS, g0)
    assert abs(float(r["g"][0]) - (1.0 - float(r["d"].max()))) <= 1e-12
    assert float(np.abs(r["pre"]).max()) <= r["c"] * (1.0 + 2.0 ** -21)


def test_click_case_shortfall():
    """a 0.9 click over a 0.05 tone, its true peak 12 dB over the ceiling: the limiter keeps the loudness within 1 LU of the
    unlimited g0 x (measured here: 0.79 LU under it, 0.40 dB of RMS), the static cut leaves it 12.0 LU under"""
    x = MR.inputs(FS, FS)["click_tone"]
    g0 = MR.pre_gain(x, FS, 12.0)
    r = MR.limit(x, FS, g0)
    L_free = MR.loudness(g0 * x.astype(np.float64), FS)
    L_lim = MR.loudness(r["out"], FS)
    L_cut = MR.loudness(x.astype(np.float64) * (r["c"] / LR.true_peak(x, FS)), FS)
    rms = lambda v: 10.0 * math.log10(float(np.mean(np.asarray(v, dtype=np.float64) ** 2)))
    print("click case: unlimited %.2f LUFS, limited %.2f, static cut %.2f; RMS lost %.2f dB limited, %.2f dB cut"
          % (L_free, L_lim, L_cut, rms(g0 * x) - rms(r["out"]), rms(g0 * x) - rms(x * (r["c"] / LR.true_peak(x, FS)))))
    assert abs(L_lim - L_free) <= 1.0
    assert L_free - L_cut > 10.0
    assert abs((rms(g0 * x) - rms(r["out"])) - 0.41) <= 0.05
