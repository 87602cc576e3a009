"""Output levelling on the GPU: the ds_level_* kernels (csrc/loudness.hip) behind audio.measure_level / audio.level and the
drivers' `level` keyword.  GPU only (-m gpu).

Yardstick (tests/level_reference.py, never the code under test): the K-weighting recurrence walked over the whole row in
float64, the segment, block and gating sums of BS.1770 in float64; beside it the same in float32 (coefficients, state and sums),
whose distance to float64 on a case is that case's d32.

Bound per case: |kernel - float64| <= 4 x d32 of that case (the factor the front-end and resampler tests use), for the segment
energies (relative, per segment), the loudness (LU), the peak and the root mean square (relative).  The sample peak is a maximum
of the inputs: d32 = 0, and the kernel must return it exactly.  Silence has d32 = 0 everywhere and comes out as -inf LUFS, gain 1
and exact zeros.  Segments whose float64 energy is below SEG_FLOOR are the filter ringing down into digital silence (the bursts
input); float32 underflows there, so they are held to 4 x SEG_FLOOR absolutely instead of relatively."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import audio_reference as R
import level_reference as LR
from conftest import GOLDEN, parity_line, synth_sd
from text_to_sound_synthesis_amd import synth

pytestmark = pytest.mark.gpu
NO_GRAD = True

FACTOR = 4.0
SEG_FLOOR = 1e-30
FS = 22050
S = 2205
CLIP = 217088
LENGTHS = [4 * S, 4 * S + 1, 5 * S - 1, 10 * S + 1234, CLIP]
INPUT_NAMES = ["noise_0.3", "noise_1e-3", "bursts", "chirp", "tone_440", "silence", "dc_sine"]
ULP_DB = 20.0 * math.log10(1.0 + 2.0 ** -24)        # one fp32 rounding of a gain, in dB / LU


@functools.lru_cache(maxsize=None)
def _inputs(n=CLIP, rate=FS):
    """name -> f32[n] (host): audio_reference.make_inputs + 0.2 + 0.5 sin(2 pi 40 t), whose level hangs on the carried state"""
    ins = dict(R.make_inputs(n=n))
    t = torch.arange(n, dtype=torch.float64) / rate
    ins["dc_sine"] = (0.2 + 0.5 * torch.sin(2 * math.pi * 40.0 * t)).float()
    return ins


@functools.lru_cache(maxsize=None)
def _weighted(name, n=CLIP, rate=FS):
    """(y64, y32) of input `name`, computed once: the filter is causal, so a prefix of y is the K-weighted prefix of x"""
    x = _inputs(n, rate)[name].numpy()
    return LR.kweighted(x, rate, np.float64), LR.kweighted(x, rate, np.float32)


def _reference(x, y64, y32, rate, n):
    """float64 and float32 measures of the first n samples -> dict"""
    Sr = LR.segment_samples(rate)
    seg64, seg32 = LR.segment_energies(y64, Sr, n), LR.segment_energies(y32, Sr, n)
    z64 = LR.blocks(seg64, Sr)
    L64, A, G, rel = LR.gate(z64)
    L32 = LR.gate(LR.blocks(seg32, Sr))[0]
    return {"seg64": seg64, "seg32": seg32.astype(np.float64), "z64": z64, "L64": L64, "L32": L32, "A": A, "G": G,
            "peak": LR.sample_peak(x[:n]), "ms64": LR.mean_square(x[:n]), "ms32": LR.mean_square(x[:n], np.float32)}


def _check_measures(tag, m, row, ref):
    """the kernel's measures of row `row` against `ref`; asserts the bounds; one parity line"""
    seg = m["seg"][row].cpu().numpy()
    n_seg = ref["seg64"].shape[0]
    assert np.isfinite(seg).all() and (seg[n_seg:] == 0).all()
    seg = seg[:n_seg]
    big = ref["seg64"] > SEG_FLOOR
    rel = lambda a: float(np.max(np.abs(a[big] - ref["seg64"][big]) / ref["seg64"][big])) if big.any() else 0.0
    e_seg, d_seg = rel(seg), rel(ref["seg32"])
    small = float(np.max(np.abs(seg[~big] - ref["seg64"][~big]))) if (~big).any() else 0.0
    L = float(m["lufs"][row])
    peak, tp, rms = float(m["sample_peak"][row]), float(m["true_peak"][row]), float(m["rms"][row])
    assert all(math.isfinite(v) for v in (peak, tp, rms)) and tp >= peak
    rms64, rms32 = math.sqrt(ref["ms64"]), math.sqrt(ref["ms32"])
    e_rms = abs(rms - rms64) / rms64 if rms64 > 0 else abs(rms)
    d_rms = abs(rms32 - rms64) / rms64 if rms64 > 0 else 0.0
    if ref["L64"] == -math.inf:
        e_L, d_L = (0.0 if L == -math.inf else math.inf), 0.0
    else:
        e_L, d_L = abs(L - ref["L64"]), abs(ref["L32"] - ref["L64"])
    line = ("%s: L %.4f LUFS, |L - L64| %.2e LU (4 x d32 %.2e); seg rel %.2e (4 x d32 %.2e); rms rel %.2e (4 x d32 %.2e); "
            "peak %.6g" % (tag, L, e_L, FACTOR * d_L, e_seg, FACTOR * d_seg, e_rms, FACTOR * d_rms, peak))
    print(line)
    parity_line("level " + line)
    assert e_L <= FACTOR * d_L, line
    assert e_seg <= FACTOR * d_seg and small <= FACTOR * SEG_FLOOR, line
    assert e_rms <= FACTOR * d_rms, line
    assert peak == ref["peak"], line
    return L


# ---- 1. segment energies, loudness, peak and rms against float64 --------------------------------------------------------
@pytest.mark.parametrize("name", INPUT_NAMES)
def test_measures_vs_float64(name):
    """every input at the five lengths (one block, one sample more, one short of five segments, an odd length, a whole clip)"""
    from text_to_sound_synthesis_amd import audio
    x = _inputs()[name]
    y64, y32 = _weighted(name)
    xd = x.cuda()
    for n in LENGTHS:
        m = audio.measure_level(xd[None, :n].contiguous(), FS, segments=True)
        assert tuple(m["seg"].shape) == (1, n // S) and m["lufs"].dtype == torch.float64
        L = _check_measures("%s, %d samples" % (name, n), m, 0, _reference(x.numpy(), y64, y32, FS, n))
        if name == "silence":
            out, g = audio.level(xd[None, :n].contiguous(), FS, "loudness")
            assert L == -math.inf and float(g[0]) == 1.0 and float(out.abs().max()) == 0.0
            assert float(m["sample_peak"][0]) == 0.0 and float(m["true_peak"][0]) == 0.0 and float(m["rms"][0]) == 0.0
            for strategy in ("peak", "rms"):
                out, g = audio.level(xd[None, :n].contiguous(), FS, strategy)
                assert float(g[0]) == 1.0 and bool(torch.isfinite(out).all()) and float(out.abs().max()) == 0.0


def test_restart_per_segment_would_be_caught():
    """the dc_sine input is there for the carried state: a filter restarted at every segment is further from float64 than
    the bound of that case allows (so test_measures_vs_float64 fails without the carry)"""
    n = 10 * S + 1234
    x = _inputs()["dc_sine"].numpy()[:n]
    y64, y32 = _weighted("dc_sine")
    ref = _reference(x, y64, y32, FS, n)
    restarted = np.concatenate([LR.kweighted(x[i:i + S], FS) for i in range(0, n, S)])
    off = abs(LR.loudness_from(restarted, FS) - ref["L64"])
    print("dc_sine: a per-segment restart is %.3f LU off, the bound is %.2e" % (off, FACTOR * abs(ref["L32"] - ref["L64"])))
    assert off > 0.05 and off > 10 * FACTOR * abs(ref["L32"] - ref["L64"])


def test_long_row_past_one_token_grid():
    from text_to_sound_synthesis_amd import audio
    n = 600000
    x = _inputs(n)["noise_0.3"]
    y64, y32 = _weighted("noise_0.3", n)
    m = audio.measure_level(x[None].cuda(), FS, segments=True)
    _check_measures("noise_0.3, %d samples" % n, m, 0, _reference(x.numpy(), y64, y32, FS, n))


@pytest.mark.parametrize("rate", [16000, 48000])
def test_other_rates(rate):
    from text_to_sound_synthesis_amd import audio
    Sr = LR.segment_samples(rate)
    n = 10 * Sr + 1234
    ins = _inputs(n, rate)
    xd = torch.stack([ins[k] for k in INPUT_NAMES]).cuda()
    m = audio.measure_level(xd, rate, segments=True)
    up = audio.resample(xd, rate, 4 * rate).abs().amax(1)
    assert torch.equal(m["true_peak"], torch.maximum(up, m["sample_peak"]))
    for i, name in enumerate(INPUT_NAMES):
        y64, y32 = _weighted(name, n, rate)
        _check_measures("%d Hz %s, %d samples" % (rate, name, n), m, i, _reference(ins[name].numpy(), y64, y32, rate, n))


# ---- 2. gating ------------------------------------------------------------------------------------------------------------
def test_gating_case():
    from text_to_sound_synthesis_amd import audio
    clip, _ = LR.gating_clip(FS)
    y64, y32 = LR.kweighted(clip, FS), LR.kweighted(clip, FS, np.float32)
    ref = _reference(clip, y64, y32, FS, clip.shape[0])
    assert abs(ref["L64"] - (-17.45)) <= 0.01
    m = audio.measure_level(torch.from_numpy(clip)[None].cuda(), FS, segments=True)
    L = _check_measures("gating case", m, 0, ref)
    assert abs(L - (-17.45)) <= 0.01
    z = LR.blocks(m["seg"][0].cpu().numpy(), S)
    _, A, G, _ = LR.gate(z)
    assert np.array_equal(A, ref["A"]) and np.array_equal(G, ref["G"])
    assert m["gate_counts"][0].tolist() == [int(ref["A"].sum()), int(ref["G"].sum())]
    assert 0 < int(ref["G"].sum()) < int(ref["A"].sum()) < z.size


# ---- 3. lengths -----------------------------------------------------------------------------------------------------------
def _same(a, b, keys):
    return all(torch.equal(a[k], b[k]) for k in keys)


def test_rows_of_different_length_in_one_stride():
    from text_to_sound_synthesis_amd import audio
    lens = [10 * S + 1234, 4 * S, 5 * S - 1]
    T = max(lens) + 777
    ins = _inputs()
    x = torch.full((3, T), float("nan"))
    for i, (k, n) in enumerate(zip(("noise_0.3", "dc_sine", "chirp"), lens)):
        x[i, :n] = ins[k][:n]
    x = x.cuda()
    for lengths in (lens, torch.tensor(lens, dtype=torch.int32).cuda()):
        m = audio.measure_level(x, FS, lengths=lengths, segments=True)
        out, g = audio.level(x, FS, "loudness", lengths=lengths)
        assert bool(torch.isfinite(m["lufs"]).all()) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(g).all())
        for i, n in enumerate(lens):
            alone = x[i:i + 1, :n].contiguous()
            a = audio.measure_level(alone, FS, segments=True)
            for k in ("lufs", "sample_peak", "true_peak", "rms", "gate_counts"):
                assert torch.equal(a[k][0], m[k][i]), (k, i)
            assert torch.equal(a["seg"][0], m["seg"][i, :n // S]) and float(m["seg"][i, n // S:].abs().sum()) == 0.0
            oa, ga = audio.level(alone, FS, "loudness")
            assert torch.equal(ga[0], g[i]) and torch.equal(oa[0], out[i, :n]) and float(out[i, n:].abs().max()) == 0.0


# ---- 4. batch invariance --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 64])
def test_batch_position_and_run_invariance(B):
    from text_to_sound_synthesis_amd import audio
    g = torch.Generator().manual_seed(300 + B)
    T = 10 * S + 1234
    w = (0.2 * torch.randn(B, T, generator=g)).cuda()
    row = _inputs()["dc_sine"][:T].cuda()
    keys = ("lufs", "sample_peak", "true_peak", "rms", "seg", "gate_counts")
    alone = audio.measure_level(row[None], FS, segments=True)
    out_alone, g_alone = audio.level(row[None], FS, "loudness")
    for pos in sorted({0, B // 2, B - 1}):
        batch = w.clone()
        batch[pos] = row
        m, again = audio.measure_level(batch, FS, segments=True), audio.measure_level(batch, FS, segments=True)
        assert _same(m, again, keys)
        for k in keys:
            assert torch.equal(m[k][pos], alone[k][0]), (k, pos, B)
        out, gg = audio.level(batch, FS, "loudness")
        assert torch.equal(gg[pos], g_alone[0]) and torch.equal(out[pos], out_alone[0])


# ---- 5. / 6. true peak ----------------------------------------------------------------------------------------------------
def test_true_peak_between_the_samples():
    """sin(2 pi (fs / 4) t + pi / 4): every sample is +-0.70711, the curve between them reaches 1"""
    from text_to_sound_synthesis_amd import audio
    x = LR.sine(FS / 4.0, FS, 1.0, 1.0, math.pi / 4.0).astype(np.float32)
    m = audio.measure_level(torch.from_numpy(x)[None].cuda(), FS)
    sp, tp = float(m["sample_peak"][0]), float(m["true_peak"][0])
    tp64, tp32 = LR.true_peak(x, FS), LR.true_peak(x, FS, np.float32)
    line = "inter-sample case: sample peak %.5f, true peak %.8f (float64 yardstick %.8f, float32 %.8f)" % (sp, tp, tp64, tp32)
    print(line)
    parity_line("level " + line)
    assert abs(sp - 0.70711) < 1e-5 and tp > 1.4 * sp
    assert abs(tp - tp64) <= FACTOR * abs(tp32 - tp64), line


@pytest.mark.parametrize("n", [10 * S + 1234, CLIP])
def test_true_peak_is_the_resampler_s(n):
    from text_to_sound_synthesis_amd import audio
    xd = torch.stack([_inputs()[k][:n] for k in INPUT_NAMES]).cuda()
    m = audio.measure_level(xd, FS)
    up = audio.resample(xd, FS, 4 * FS)
    assert tuple(up.shape) == (len(INPUT_NAMES), 4 * n)
    assert torch.equal(m["true_peak"], torch.maximum(up.abs().amax(1), m["sample_peak"]))
    assert torch.equal(m["sample_peak"], xd.abs().amax(1))
    lens = torch.tensor([n - 3 * i for i in range(len(INPUT_NAMES))], dtype=torch.int32).cuda()
    ml = audio.measure_level(xd, FS, lengths=lens)
    upl = audio.resample(xd, FS, 4 * FS, lengths=lens)
    mask = torch.arange(n, device="cuda")[None, :] < lens[:, None]
    assert torch.equal(ml["sample_peak"], (xd.abs() * mask).amax(1))
    assert torch.equal(ml["true_peak"], torch.maximum(upl.abs().amax(1), ml["sample_peak"]))


# ---- 7. gain --------------------------------------------------------------------------------------------------------------
def _ref_measure(x, rate):
    y = LR.kweighted(x, rate)
    return LR.loudness_from(y, rate), LR.sample_peak(x), LR.mean_square(x)


@pytest.mark.parametrize("name", ["noise_0.3", "noise_1e-3", "dc_sine"])
def test_gain_lands_on_target(name):
    """no ceiling in the way (+40 dB): the yardstick's measure of `out` is the target, within test 1's bound for that input
    plus one fp32 rounding of the gain.  For the peak, where test 1's bound is 0, that holds for the exact product g32 x; `out`
    is the product rounded to fp32 once more (the definition of out), which the second assertion allows for."""
    from text_to_sound_synthesis_amd import audio
    n = 10 * S + 1234
    x = _inputs()[name][:n].contiguous()
    y64, y32 = _weighted(name)
    ref = _reference(x.numpy(), y64, y32, FS, n)
    d_L = abs(ref["L32"] - ref["L64"])
    d_rms = abs(math.sqrt(ref["ms32"]) - math.sqrt(ref["ms64"])) / math.sqrt(ref["ms64"])
    xd = x[None].cuda()
    rec = _inputs(10 * 4800 + 1234, 48000)["noise_0.3"]
    L_rec = LR.loudness_from(LR.kweighted(rec.numpy(), 48000), 48000)
    cases = [("peak", -3.0, None), ("rms", -20.0, None), ("loudness", -23.0, None), ("loudness", -16.5, None),
             ("match", L_rec, (rec[None].cuda(), 48000))]
    for strategy, target, reference in cases:
        out, g = audio.level(xd, FS, strategy, target=None if strategy == "match" else target, ceiling_db=40.0, reference=reference)
        assert out.dtype == torch.float32 and tuple(out.shape) == (1, n) and tuple(g.shape) == (1,)
        assert torch.equal(out, g[:, None] * xd)
        o = out[0].cpu().numpy()
        L, peak, ms = _ref_measure(o, FS)
        if strategy == "peak":
            exact = float(g[0].double()) * ref["peak"]
            e0 = abs(20.0 * math.log10(exact) - target)
            err, bound = abs(20.0 * math.log10(peak) - target), 2.0 * ULP_DB
            assert e0 <= ULP_DB, (e0, ULP_DB)
        elif strategy == "rms":
            err, bound = abs(10.0 * math.log10(ms) - target), 20.0 * math.log10(1.0 + FACTOR * d_rms) + ULP_DB
        else:
            err, bound = abs(L - target), FACTOR * d_L + ULP_DB
        line = "%s -> %s %.3f: the yardstick measures out %.2e off, bound %.2e" % (name, strategy, target, err, bound)
        print(line)
        parity_line("level " + line)
        assert err <= bound, line


def test_default_targets_and_in_place_layout():
    """the defaults (-1 dBFS peak, -20 dBFS rms, -23 LUFS, ceiling -1 dBFS) against the yardstick's float64 gain, within the
    measures' own bounds (4 x d32 of the true peak, the rms and the loudness, as a relative gain) plus two fp32 steps (the
    rounding of g and the step down under the ceiling); a stride that is no multiple of 4 takes the other store path: the same
    bits"""
    from text_to_sound_synthesis_amd import audio
    n = 10 * S + 1234                                                    # 23284 = 4 x 5821
    x = _inputs()["noise_0.3"][:n + 1].contiguous()
    y64, y32 = _weighted("noise_0.3")
    for m_ in (n, n + 1):
        xs = x[:m_].numpy()
        ref = _reference(xs, y64, y32, FS, m_)
        tp64, tp32 = LR.true_peak(xs, FS), LR.true_peak(xs, FS, np.float32)
        d = (abs(tp32 - tp64) / tp64 + abs(math.sqrt(ref["ms32"] / ref["ms64"]) - 1.0)
             + math.log(10.0) / 20.0 * abs(ref["L32"] - ref["L64"]))
        xd = x[None, :m_].contiguous().cuda()
        for strategy in ("peak", "rms", "loudness"):
            out, g = audio.level(xd, FS, strategy)
            want = LR.gain(strategy, LR.DEFAULT_TARGET[strategy], -1.0, ref["L64"], ref["peak"], ref["ms64"], tp64)
            err, bound = abs(float(g[0]) / want - 1.0), FACTOR * d + 2.0 ** -22
            print("default %s, %d samples: gain %.6f, yardstick %.6f, rel %.2e (bound %.2e)" % (strategy, m_, float(g[0]), want, err, bound))
            assert err <= bound, (strategy, m_, float(g[0]), want)
            assert torch.equal(out, g[:, None] * xd)
            inplace = xd.clone()
            _lib_apply_in_place(inplace, g)
            assert torch.equal(inplace, out)


def _lib_apply_in_place(x, g):
    from text_to_sound_synthesis_amd import _lib
    _lib.check(_lib.lib().ds_level_apply(_lib.ptr(x), _lib.ptr(g), _lib.ptr(x), x.shape[0], x.shape[1], None, _lib.stream()))


def test_ceiling_binds():
    """target 0 dBFS peak on the inter-sample case: the gain is cut so that the TRUE peak meets the ceiling"""
    from text_to_sound_synthesis_amd import audio
    x = LR.sine(FS / 4.0, FS, 1.0, 1.0, math.pi / 4.0).astype(np.float32)
    xd = torch.from_numpy(x)[None].cuda()
    for ceiling_db in (-1.0, -3.0):
        c = 10.0 ** (ceiling_db / 20.0)
        out, g = audio.level(xd, FS, "peak", target=0.0, ceiling_db=ceiling_db)
        assert torch.equal(out, g[:, None] * xd)
        o = out[0].cpu().numpy()
        tp_out = LR.true_peak(o, FS)
        line = "ceiling %.0f dBFS on the inter-sample case: gain %.6f, float64 true peak of out / c = 1 %+.2e" % (ceiling_db, float(g[0]), tp_out / c - 1.0)
        print(line)
        parity_line("level " + line)
        assert float(g[0]) < 1.0 / LR.sample_peak(x)                    # the peak target alone would have asked for 1.414
        assert tp_out <= c * (1.0 + 2.0 ** -22), line
        assert tp_out >= c * (1.0 - 1e-5), line                          # a cut to the ceiling, not below it
        assert float(audio.measure_level(out, FS)["true_peak"][0]) <= c


# ---- 8. no synchronisation ------------------------------------------------------------------------------------------------
def test_no_host_synchronisation():
    """measure_level and level under torch.cuda.set_sync_debug_mode("error") (tables uploaded by a first call); where this
    torch build has no such mode on ROCm: captured into a graph without parallel branches and replayed, bits compared"""
    from text_to_sound_synthesis_amd import audio
    n = 10 * S + 1234
    x = torch.stack([_inputs()["noise_0.3"][:n], _inputs()["chirp"][:n]]).cuda()
    lens = torch.tensor([n, n - 999], dtype=torch.int32).cuda()
    ref48 = _inputs(10 * 4800 + 1234, 48000)["noise_0.3"][None].cuda()
    want_m = audio.measure_level(x, FS, lengths=lens, segments=True)
    want_o, want_g = audio.level(x, FS, "match", lengths=lens, reference=(ref48, 48000))
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
        used = "sync debug mode"
    except Exception:                                                    # noqa: BLE001 -- not built for this platform
        used = None
    if used:
        try:
            m = audio.measure_level(x, FS, lengths=lens, segments=True)
            o, g = audio.level(x, FS, "match", lengths=lens, reference=(ref48, 48000))
            o2, g2 = audio.level(x, FS, "loudness", target=-20.0, lengths=lens)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    else:
        used = "graph capture"
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                m = audio.measure_level(x, FS, lengths=lens, segments=True)
                o, g = audio.level(x, FS, "match", lengths=lens, reference=(ref48, 48000))
        graph.replay()
    torch.cuda.synchronize()
    parity_line("level no-synchronisation check ran under: %s" % used)
    assert all(torch.equal(m[k], want_m[k]) for k in want_m) and torch.equal(o, want_o) and torch.equal(g, want_g)


def test_argument_errors_launch_nothing():
    from text_to_sound_synthesis_amd import _lib, audio
    L_ = _lib.lib()
    B, T = 2, 10 * S
    x = torch.zeros(B, T).cuda()
    S_, kw, taps = audio._level_tables(FS, x.device)
    nb = int(L_.ds_level_scratch_bytes(B, T, S_))
    assert nb > 0 and L_.ds_level_scratch_bytes(0, T, S_) < 0 and L_.ds_level_scratch_bytes(B, T, 0) < 0
    sc = torch.zeros(nb // 8 + 1, dtype=torch.float64).cuda()
    seg = torch.zeros(B, 10, dtype=torch.float64).cuda()
    lufs, ms = torch.zeros(B, dtype=torch.float64).cuda(), torch.zeros(B, dtype=torch.float64).cuda()
    pk, g, out = torch.zeros(B, 2).cuda(), torch.zeros(B).cuda(), torch.zeros(B, T).cuda()
    p, st = _lib.ptr, _lib.stream()
    seg_ok = dict(x=p(x), B=B, T=T, lengths=None, S=S_, kw=p(kw), seg=p(seg), n=10, sc=p(sc), nb=nb)
    seg_call = lambda a: L_.ds_level_segments(a["x"], a["B"], a["T"], a["lengths"], a["S"], a["kw"], a["seg"], a["n"], a["sc"], a["nb"], st)
    tp_call = lambda a: L_.ds_level_true_peak(a["x"], a["B"], a["T"], a["lengths"], a["S"], p(taps), a["sc"], a["nb"], st)
    assert seg_call(seg_ok) == 0 and tp_call(seg_ok) == 0
    for bad in (dict(x=None), dict(kw=None), dict(seg=None), dict(sc=None), dict(B=0), dict(T=-1), dict(S=0), dict(n=9), dict(nb=nb - 16)):
        assert seg_call(dict(seg_ok, **bad)) == -1, bad
    for bad in (dict(x=None), dict(sc=None), dict(B=0), dict(S=0), dict(nb=nb - 16)):
        assert tp_call(dict(seg_ok, **bad)) == -1, bad
    gain_ok = dict(seg=p(seg), n=10, B=B, T=T, S=S_, strategy=3, target=-23.0, tdev=None, tn=0, c=-1.0, sc=p(sc), nb=nb, lufs=p(lufs),
                   pk=p(pk), ms=p(ms), g=p(g))
    gain_call = lambda a: L_.ds_level_gain(a["seg"], a["n"], a["B"], a["T"], None, a["S"], a["strategy"], a["target"], a["tdev"], a["tn"],
                                           a["c"], a["sc"], a["nb"], a["lufs"], a["pk"], a["ms"], None, a["g"], st)
    assert gain_call(gain_ok) == 0
    for bad in (dict(seg=None), dict(g=None), dict(lufs=None), dict(strategy=4), dict(strategy=-1), dict(target=float("nan")),
                dict(c=float("inf")), dict(tdev=p(lufs), tn=3), dict(tdev=p(lufs), tn=B, strategy=1), dict(n=9), dict(nb=0)):
        assert gain_call(dict(gain_ok, **bad)) == -1, bad
        with pytest.raises(_lib.DiffsoundHipError):
            _lib.check(gain_call(dict(gain_ok, **bad)))
    assert L_.ds_level_apply(p(x), p(g), p(out), B, T, None, st) == 0
    for args in ((None, p(g), p(out), B, T), (p(x), None, p(out), B, T), (p(x), p(g), None, B, T), (p(x), p(g), p(out), 0, T)):
        assert L_.ds_level_apply(*args, None, st) == -1
    with pytest.raises(ValueError):                                      # shorter than one block, lengths known on the host
        audio.level(x[:, :4 * S - 1].contiguous(), FS, "loudness")
    with pytest.raises(ValueError):
        audio.level(x, FS, "match", lengths=[T, 100], reference=(x, FS))
    torch.cuda.synchronize()


# ---- 9. drivers -----------------------------------------------------------------------------------------------------------
# fp32 roundings between the yardstick's measure of a levelled driver output and its target: the gain's and the product's;
# the kernels' own sums are float64 (test 1 measures their distance, ~1e-12 LU)
DRIVER_LU = 2.0 * ULP_DB + 1e-9


@pytest.fixture(scope="module")
def ds():
    """the 2-layer model with synthetic weights and a random vocoder (as tests/test_hip_resample.py builds them)"""
    from text_to_sound_synthesis_amd import tokenizer as tz
    from text_to_sound_synthesis_amd.config import default_config
    from text_to_sound_synthesis_amd.pipeline import Diffsound
    d = Diffsound(config=default_config(n_layer=2, diffusion_step=100, with_clip=True, bpe_path=tz.CLOSED_VOCAB_PATH),
                  random_vocoder=True)
    with open(os.path.join(GOLDEN, "state_dict_keys_clip.json")) as f:
        clip_sd = synth.synth_state_dict(json.load(f))
    sd = {**synth_sd("dalle", 2), **synth_sd("encoder"), **clip_sd}
    missing, unexpected = d.model.load_state_dict(sd, strict=False)
    assert not unexpected
    d.model = d.model.cuda().eval()
    dt = d.model.transformer
    dt.auxiliary_loss_weight, dt.adaptive_auxiliary_loss, dt.mask_weight = 5.0e-4, True, [1, 1]
    return d


def _on_target(tag, plain, levelled, rate, target):
    """row 0 of `levelled` (f32[B,1,T]) is `plain` brought to `target` LUFS -- or to the -1 dBFS ceiling where that binds: then
    the gain hangs on the kernel's fp32 true peak, held to 4 x its d32 like every other measure, and may sit one fp32 step
    lower (include/diffsound_hip.h)"""
    x, o = plain[0, 0].cpu().numpy(), levelled[0, 0].cpu().numpy()
    L_x = LR.loudness_from(LR.kweighted(x, rate), rate)
    L_o = LR.loudness_from(LR.kweighted(o, rate), rate)
    tp64, tp32 = LR.true_peak(x, rate), LR.true_peak(x, rate, np.float32)
    g = LR.gain("loudness", target, -1.0, L_x, LR.sample_peak(x), LR.mean_square(x), tp64)
    cut = g < 10.0 ** ((target - L_x) / 20.0)
    want = L_x + 20.0 * math.log10(g)
    bound = DRIVER_LU + (20.0 * math.log10(1.0 + FACTOR * abs(tp32 - tp64) / tp64) + ULP_DB if cut else 0.0)
    line = "%s: %.3f LUFS -> %.3f, target %.3f%s, off %.2e LU (bound %.2e)" % (
        tag, L_x, L_o, target, " (cut by the ceiling)" if cut else "", abs(L_o - want), bound)
    print(line)
    parity_line("level " + line)
    assert abs(L_o - want) <= bound, line
    applied = float(np.abs(o).max()) / LR.sample_peak(x)                 # the gain, to one fp32 rounding
    assert applied * tp64 <= 10.0 ** (-1.0 / 20.0) * (1.0 + 2.0 ** -22), line


def test_driver_generate_sample_with_condition(ds):
    captions = synth.synth_captions(1, seed=3)
    kw = dict(caption_ids=[0], seed=11)
    m0, w0, t0 = ds.generate_sample_with_condition(captions, **kw)
    m1, w1, t1 = ds.generate_sample_with_condition(captions, level=None, **kw)
    assert torch.equal(w0, w1) and torch.equal(m0, m1) and torch.equal(t0, t1)
    m2, w2, t2 = ds.generate_sample_with_condition(captions, level="loudness", **kw)
    assert torch.equal(m2, m0) and torch.equal(t2, t0) and tuple(w2.shape) == tuple(w0.shape)
    _on_target("generate_sample_with_condition", w0, w2, 22050, -23.0)
    m3, w3, t3 = ds.generate_sample_with_condition(captions, sample_rate=48000, **kw)
    m4, w4, t4 = ds.generate_sample_with_condition(captions, sample_rate=48000, level={"strategy": "loudness", "target": -18.0}, **kw)
    assert torch.equal(m4, m0) and torch.equal(t4, t0) and tuple(w4.shape) == tuple(w3.shape) == (1, 1, 472573)
    _on_target("generate_sample_with_condition at 48 kHz", w3, w4, 48000, -18.0)
    with pytest.raises(ValueError):
        ds.generate_sample_with_condition(captions, level="match", **kw)
    with pytest.raises(ValueError):
        ds.generate_sample_with_condition(captions, level="louder", **kw)


def test_driver_inpaint_audio(ds, tmp_path):
    from text_to_sound_synthesis_amd import audio
    captions = synth.synth_captions(1, seed=4)
    rec = (0.05 * torch.randn(1, 300000, generator=torch.Generator().manual_seed(9))).cuda()      # a recording at 32 kHz
    kw = dict(audio_rate=32000, caption_ids=[0], seed=5)
    spans = [(2.0, 4.0)]
    m0, w0, t0 = ds.inpaint_audio(rec, captions, spans, **kw)
    m1, w1, t1 = ds.inpaint_audio(rec, captions, spans, level=None, **kw)
    assert torch.equal(w0, w1) and torch.equal(m0, m1) and torch.equal(t0, t1)
    m2, w2, t2 = ds.inpaint_audio(rec, captions, spans, level="loudness", save_root=str(tmp_path / "a"), **kw)
    assert torch.equal(m2, m0) and torch.equal(t2, t0)
    _on_target("inpaint_audio", w0, w2, 22050, -23.0)
    L_rec = LR.loudness_from(LR.kweighted(rec[0].cpu().numpy(), 32000), 32000)
    m3, w3, t3 = ds.inpaint_audio(rec, captions, spans, level="match", sample_rate=48000, save_root=str(tmp_path / "b"), **kw)
    m4, w4, t4 = ds.inpaint_audio(rec, captions, spans, sample_rate=48000, **kw)
    assert torch.equal(m3, m0) and torch.equal(t3, t0)
    _on_target("inpaint_audio, match at 48 kHz", w4, w3, 48000, L_rec)
    for sub, rate, wave in (("a", 22050, w2), ("b", 48000, w3)):
        x, sr = audio.read_wav(str(tmp_path / sub / "000000.wav"))
        q = torch.round(x.double() * 8388608.0)
        assert sr == rate and x.numel() == wave.shape[2]
        assert int(q.max()) < 8388607 and int(q.min()) > -8388608      # nothing at the PCM-24 rails


def test_driver_generate_long(ds, tmp_path):
    from text_to_sound_synthesis_amd import audio
    captions = synth.synth_captions(1, seed=6)
    kw = dict(caption_ids=[0], seed=7)
    m0, w0, t0 = ds.generate_long(captions, 15.0, **kw)
    assert tuple(t0.shape) == (1, 2, 265)
    m1, w1, t1 = ds.generate_long(captions, 15.0, level=None, **kw)
    assert torch.equal(w0, w1) and torch.equal(m0, m1) and torch.equal(t0, t1)
    m2, w2, t2 = ds.generate_long(captions, 15.0, level="loudness", save_root=str(tmp_path / "l"), **kw)
    assert torch.equal(m2, m0) and torch.equal(t2, t0)
    _on_target("generate_long, 2 windows", w0, w2, 22050, -23.0)
    m3, w3, t3 = ds.generate_long(captions, 15.0, sample_rate=48000, **kw)
    m4, w4, t4 = ds.generate_long(captions, 15.0, sample_rate=48000, level="loudness", **kw)
    assert torch.equal(m4, m0) and torch.equal(t4, t0)
    _on_target("generate_long at 48 kHz", w3, w4, 48000, -23.0)
    x, sr = audio.read_wav(str(tmp_path / "l" / "000000.wav"))
    q = torch.round(x.double() * 8388608.0)
    assert sr == 22050 and int(q.max()) < 8388607 and int(q.min()) > -8388608
    with pytest.raises(ValueError):
        ds.generate_long(captions, 15.0, level="match", **kw)


# ---- 10. the drivers that level through another driver's tail -----------------------------------------------------------------
# both sides of every comparison run the same kernels on the same input: bit for bit
def _wav_bytes(tmp_path, row, rate=22050):
    from text_to_sound_synthesis_amd.pipeline import write_wav_pcm24
    path = str(tmp_path / "expected.wav")
    write_wav_pcm24(path, row.cpu().numpy(), rate)
    with open(path, "rb") as f:
        return f.read()


def test_driver_generate_sample_levels_once_through_the_inner_driver(ds, tmp_path):
    import csv
    captions = synth.synth_captions(1, seed=12)
    with open(str(tmp_path / "val.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["file_name", "caption"])
        w.writerow(["clip.wav", captions[0]])
    tr = ds.model.transformer
    mode, tr.rng_mode = tr.rng_mode, "philox"
    try:
        written = ds.generate_sample(str(tmp_path / "val.csv"), 0.85, str(tmp_path / "out"), fast=10, replicate=1, level="peak")
        _, wave, _ = ds.generate_sample_with_condition(captions, 0.85, 1, fast=10, caption_ids=[0], level="peak")
        _, plain, _ = ds.generate_sample_with_condition(captions, 0.85, 1, fast=10, caption_ids=[0])
    finally:
        tr.rng_mode = mode
    assert written == [str(tmp_path / "out" / "clip_mel_sample_0")] and tuple(wave.shape) == (1, 1, CLIP)
    with open(written[0] + ".wav", "rb") as f:
        assert f.read() == _wav_bytes(tmp_path, wave[0, 0])
    assert not torch.equal(wave, plain)                                   # and the level did reach the waveform


def test_driver_inference_generate_sample_with_condition_levels_once(ds, tmp_path):
    text = synth.synth_captions(1, seed=13)[0]
    torch.manual_seed(21)
    written = ds.inference_generate_sample_with_condition(text, 0.85, str(tmp_path / "out"), 4, fast=10, level="loudness")
    torch.manual_seed(21)
    _, wave, _ = ds.generate_sample_with_condition([text], 0.85, replicate=10, fast=10, level="loudness")
    torch.manual_seed(21)
    _, plain, _ = ds.generate_sample_with_condition([text], 0.85, replicate=10, fast=10)
    assert written == [str(tmp_path / "out" / text / ("%06d" % i)) for i in range(10)] and tuple(wave.shape) == (10, 1, CLIP)
    for i, stem in enumerate(written):
        with open(stem + ".wav", "rb") as f:
            assert f.read() == _wav_bytes(tmp_path, wave[i, 0]), i
    assert not torch.equal(wave, plain)


def test_driver_generate_best_of_levels_the_winners_once(ds):
    from text_to_sound_synthesis_amd import audio
    captions = synth.synth_captions(1, seed=14)
    kw = dict(n=2, fast=10, score_timesteps=2, caption_ids=[0], seed=3)
    mel0, plain, tok0, sc0 = ds.generate_best_of(captions, **kw)
    mel1, wave, tok1, sc1 = ds.generate_best_of(captions, level="rms", **kw)
    assert torch.equal(tok1, tok0) and torch.equal(mel1, mel0) and torch.equal(sc1, sc0)
    assert torch.equal(wave, audio.level(plain[:, 0], 22050, "rms")[0][:, None]) and not torch.equal(wave, plain)
