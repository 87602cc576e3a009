"""Host side of pasting a recording back (keep_original=): pipeline.paste_plan for the four drivers, the keywords the drivers
gained, and the invariants of the float64 yardstick (tests/paste_reference.py).  No kernel is launched."""
import inspect
import math

import numpy as np
import pytest
import torch

import paste_reference as PR
from text_to_sound_synthesis_amd import pipeline

SPANS = [[(4.0, 7.0)], [(0.0, 1.5), (8.0, 217088 / 22050)]]


def test_recording_offset_follows_from_the_two_front_ends():
    from text_to_sound_synthesis_amd import audio
    from text_to_sound_synthesis_amd.modeling import melspec
    crop = (melspec.SPEC_FRAMES - melspec.CROP_FRAMES) // 2                    # content-image frame j = front-end frame j + 6
    centre_in_recording = lambda j: audio.HOP * (j + crop) + melspec.PAD - audio.N_FFT // 2          # centred frames
    centre_in_rendering = lambda j: audio.HOP * j - (audio.N_FFT - audio.HOP) // 2 + audio.N_FFT // 2  # Audio2Mel's padding
    for j in (0, 1, 500, 847):
        assert centre_in_recording(j) - centre_in_rendering(j) == pipeline.RECORDING_OFFSET == 1408
    assert [pipeline.recording_offset(r) for r in (None, 22050, 44100, 48000, 16000)] == [1408, 1408, 2816, 3065, 1022]
    for r in (8000, 16000, 44100, 48000, 96000):
        assert pipeline.recording_offset(r) == math.floor(1408 * r / 22050 + 0.5)


@pytest.mark.parametrize("driver", ["inpaint_audio", "inpaint_scene"])
def test_plan_of_the_inpainting_drivers(driver):
    p = pipeline.paste_plan(driver, "audio", batch=2, spans=SPANS)
    keep = pipeline.spans_to_keep_mask(SPANS, 2).view(2, 53, 5)
    assert p["mode"] == "audio" and p["match_gain"] is True
    assert p["keep_cols"].dtype == torch.uint8 and tuple(p["keep_cols"].shape) == (2, 53)
    assert torch.equal(p["keep_cols"].bool(), keep[:, :, 0]) and bool((keep == keep[:, :, :1]).all())
    assert p["keep_cols"][0].tolist() == [1] * 21 + [0] * 17 + [1] * 15
    assert p["keep_cols"][1].tolist() == [0] * 9 + [1] * 34 + [0] * 10
    assert p["mel"] == {"off": 0, "col_num": 16, "col_den": 1, "fade_len": 4.0}
    assert p["audio"] == {"off": 1408, "col_num": 4096, "col_den": 1, "fade_len": 1024.0, "rate": 22050}
    for rate, off in ((44100, 2816), (48000, 3065), (16000, 1022)):
        a = pipeline.paste_plan(driver, "mel", batch=2, spans=SPANS, sample_rate=rate, fade_seconds=0.0, match_gain=False)
        assert a["mode"] == "mel" and a["match_gain"] is False
        assert a["audio"]["off"] == off and a["audio"]["rate"] == rate and a["audio"]["fade_len"] == 0.0 == a["mel"]["fade_len"]
        assert a["audio"]["col_num"] * 22050 == 4096 * rate * a["audio"]["col_den"]
        assert math.gcd(a["audio"]["col_num"], a["audio"]["col_den"]) == 1
    assert pipeline.paste_plan(driver, None, batch=2, spans=SPANS) is None


def test_plan_of_continue_audio():
    p = pipeline.paste_plan("continue_audio", "audio", batch=3, keep_seconds=3.0)
    assert pipeline.continuation_columns(3.0) == 17
    assert p["keep_cols"].tolist() == [[1] * 17 + [0] * 36] * 3
    assert p["mel"]["off"] == 16 * 36 and p["audio"]["off"] == 4096 * 36 + 1408
    for rate in (16000, 44100, 48000):
        a = pipeline.paste_plan("continue_audio", "audio", batch=1, keep_seconds=3.0, sample_rate=rate)
        assert a["audio"]["off"] == math.floor((1408 + 4096 * 36) * rate / 22050 + 0.5)      # scaled and rounded once
    with pytest.raises(ValueError):
        pipeline.paste_plan("continue_audio", "audio", batch=1, keep_seconds=0.0)


def test_plan_of_extend_audio():
    p = pipeline.paste_plan("extend_audio", "mel", batch=2, seconds=15.0)
    n_cols = -(-round(15.0 * 22050) // 4096)
    assert tuple(p["keep_cols"].shape) == (2, n_cols) and n_cols == 81
    assert p["keep_cols"][0].tolist() == [1] * 53 + [0] * (n_cols - 53)
    assert p["mel"]["off"] == 0 and p["audio"]["off"] == 1408
    with pytest.raises(ValueError):
        pipeline.paste_plan("extend_audio", "mel", batch=2, seconds=9.0)


def test_plan_value_errors():
    kw = dict(batch=2, spans=SPANS)
    for bad in ("wave", "Mel", True, 1):
        with pytest.raises(ValueError):
            pipeline.paste_plan("inpaint_audio", bad, **kw)
    with pytest.raises(ValueError):
        pipeline.paste_plan("inpaint_audio", "audio", has_vocoder=False, **kw)
    assert pipeline.paste_plan("inpaint_audio", "mel", has_vocoder=False, **kw)["mode"] == "mel"
    for fade in (-1e-9, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pipeline.paste_plan("inpaint_audio", "mel", fade_seconds=fade, **kw)
    with pytest.raises(ValueError):
        pipeline.paste_plan("generate_long", "mel", batch=2)


def test_drivers_gained_keyword_only_defaults():
    for name in ("inpaint_audio", "inpaint_scene", "continue_audio", "extend_audio"):
        ps = inspect.signature(getattr(pipeline.Diffsound, name)).parameters
        tail = list(ps.values())[-4:]
        assert [p.name for p in tail] == ["level", "keep_original", "fade_seconds", "match_gain"]
        assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in tail)
        assert [p.default for p in tail] == [None, None, 1024 / 22050, True]
    for name in ("generate_sample_with_condition", "generate_long", "generate_scene", "generate_sample_from_audio"):
        assert "keep_original" not in inspect.signature(getattr(pipeline.Diffsound, name)).parameters


def test_drivers_refuse_bad_keywords_before_any_work():
    class NoVocoder:                       # the checks run before the driver's body: nothing of the model is touched
        vocoder = None
    with pytest.raises(ValueError):
        pipeline.Diffsound.inpaint_audio(NoVocoder(), None, None, SPANS, keep_original="audio")
    with pytest.raises(ValueError):
        pipeline.Diffsound.continue_audio(NoVocoder(), None, None, 3.0, keep_original="samples")
    with pytest.raises(ValueError):
        pipeline.Diffsound.extend_audio(NoVocoder(), None, None, 15.0, keep_original="mel", fade_seconds=-0.1)
    with pytest.raises(TypeError):
        pipeline.Diffsound.generate_long(NoVocoder(), None, 15.0, keep_original="mel")


# ---- the yardstick's own invariants ------------------------------------------------------------------------------------------
def test_reference_curves():
    u = np.linspace(0.0, 1.0, 4097)
    wr, wo = PR.curve(u, "equal_power")
    assert np.abs(wr * wr + wo * wo - 1.0).max() <= 4 * 2.0 ** -53
    assert wr[0] == 0.0 and wo[0] == 1.0 and wr[-1] == 1.0 and abs(wo[-1]) < 1e-16
    lr, lo = PR.curve(u, "linear")
    assert np.abs(lr + lo - 1.0).max() <= 2.0 ** -53 and lr[0] == 0.0 and lo[-1] == 0.0


@pytest.mark.parametrize("col", [(4096, 1), (4096 * 48000 // 150, 22050 // 150), (4096 * 16000 // 50, 22050 // 50), (16, 1)])
def test_reference_columns_and_weights(col):
    col_num, col_den = col
    n_cols = 5
    T = -(-n_cols * col_num // col_den) + 40                                    # past the last column: the index clamps
    c = PR.columns(T, n_cols, col_num, col_den)
    n = np.arange(T)
    assert c[0] == 0 and c[-1] == n_cols - 1 and bool((np.diff(c) >= 0).all())
    inside = c < n_cols - 1
    assert bool((c[inside] * col_num <= n[inside] * col_den).all()) and bool((n[inside] * col_den < (c[inside] + 1) * col_num).all())
    fade = 0.25 * col_num / col_den
    u, kept = PR.weight(T, [1, 0, 1, 0, 0], col_num, col_den, fade)
    assert bool((u[kept] == 0.0).all()) and bool((kept == np.isin(c, (0, 2))).all())
    assert bool((u[c == 4] == 1.0).all())                                       # no kept neighbour, and none at the clip's end
    mid = u[c == 1]
    assert mid.max() == 1.0 and mid.min() < 0.01 and bool((mid[: len(mid) // 2 - 1] <= mid[1: len(mid) // 2]).all())
    tail3 = u[c == 3]
    assert bool((np.diff(tail3) >= 0).all()) and tail3[-1] == 1.0             # fades in from column 2 only
    u0, _ = PR.weight(T, [1, 0, 1, 0, 0], col_num, col_den, 0.0)
    assert bool((u0[~kept] == 1.0).all())                                       # a hard cut
    ua, ka = PR.weight(T, [1] * 5, col_num, col_den, fade)
    un, kn = PR.weight(T, [0] * 5, col_num, col_den, fade)
    assert bool(ka.all()) and not kn.any() and bool((ua == 0).all()) and bool((un == 1).all())


def test_reference_kept_and_u0_are_the_recording():
    g = np.random.default_rng(5)
    T, off = 5 * 4096, 3
    ren = g.standard_normal(T).astype(np.float32)
    ren[::7] = np.nan
    rec = g.standard_normal(T // 2).astype(np.float32)                        # ends inside the clip
    r = PR.paste(ren, rec, [1, 0, 1, 0, 1], off, rec.shape[0], 4096, 1, 1024.0, "equal_power", g=1.7)
    assert r["copy"].sum() == 3 * 4096 + 2                      # the kept columns + the first sample (dl = 0) of columns 1 and 3
    assert r["copy"][3 * 4096] and r["u"][3 * 4096] == 0.0 and r["copy"][4096] and not r["copy"][4097]
    assert np.array_equal(r["ref"][r["copy"]], r["x"][r["copy"]].astype(np.float64))
    assert np.array_equal(r["x"][: T // 2 - off], rec[off:]) and not r["x"][T // 2 - off:].any()
    so, sr = PR.sums(np.nan_to_num(ren), rec, [1, 0, 1, 0, 1], off, rec.shape[0], 4096, 1)
    assert so > 0 and sr > 0 and 0.25 <= PR.gain(so, sr) <= 4.0
    assert PR.gain(0.0, 1.0) == PR.gain(1.0, 0.0) == PR.gain(float("nan"), 1.0) == PR.gain(1.0, float("inf")) == 1.0
    assert PR.gain(1.0, 1e6) == 0.25 and PR.gain(1e6, 1.0) == 4.0


# ---- the C entries refuse bad arguments before any device call: checked here without a GPU -------------------------------------
def test_entries_refuse_bad_arguments_without_a_launch():
    from text_to_sound_synthesis_amd import _lib
    L = _lib.lib()
    fake = 4096                                        # a non-null address that is never dereferenced: every call below is refused
    good = [fake, fake, fake, 3, 1, 1024, 1100, fake, None, fake, 5, 4096, 1, 16.0, _lib.PASTE_EQUAL_POWER, None, None]
    names = ["ren", "rec", "out", "B", "C", "T", "Tr", "off", "rec_len", "keep_cols", "n_cols", "col_num", "col_den", "fade_len",
             "curve", "sums", "stream"]
    assert len(good) == len(names) == len(_lib._PROTOS["ds_paste"][1])
    bads = [("ren", None), ("rec", None), ("out", None), ("off", None), ("keep_cols", None), ("T", 0), ("T", -1), ("B", 0), ("C", 0),
            ("n_cols", 0), ("col_num", 0), ("col_den", 0), ("col_num", -1), ("col_num", 2 ** 31), ("fade_len", -1.0),
            ("fade_len", float("nan")), ("fade_len", float("inf")), ("curve", 2), ("Tr", -1)]
    for name, value in bads:
        args = list(good)
        args[names.index(name)] = value
        assert L.ds_paste(*args) == -1, (name, value)
        assert L.ds_last_error_string().startswith(b"ds_paste:"), (name, value)
    args = list(good)
    args[names.index("curve")], args[names.index("sums")] = _lib.PASTE_LINEAR, fake
    assert L.ds_paste(*args) == -1                     # a gain goes with the equal-power curve
    good_s = [fake, fake, 3, 1024, 1100, fake, None, fake, 5, 4096, 1, fake, 48, fake, None]
    names_s = ["ren", "rec", "B", "T", "Tr", "off", "rec_len", "keep_cols", "n_cols", "col_num", "col_den", "scratch", "bytes",
               "sums", "stream"]
    assert len(good_s) == len(names_s) == len(_lib._PROTOS["ds_paste_sums"][1])
    for name, value in [("ren", None), ("rec", None), ("off", None), ("keep_cols", None), ("scratch", None), ("sums", None), ("T", 0),
                        ("B", 0), ("n_cols", 0), ("col_num", 0), ("col_den", 0), ("bytes", 40), ("scratch", 4100)]:
        args = list(good_s)
        args[names_s.index(name)] = value
        assert L.ds_paste_sums(*args) == -1, (name, value)
        assert L.ds_last_error_string().startswith(b"ds_paste_sums:"), (name, value)
    assert L.ds_paste_scratch_bytes(3, 1024) == 48 and L.ds_paste_scratch_bytes(3, 8193) == 96
    assert L.ds_paste_scratch_bytes(0, 1024) == -1 and L.ds_paste_scratch_bytes(3, 0) == -1
