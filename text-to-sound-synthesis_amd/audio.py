"""Host side of the audio front end: the mel filterbank, the FFT tables of `ds_wave_to_mel`, a RIFF reader, and the thin
launcher of the kernel (csrc/stft_mel.hip) that `modeling.vocoder.Audio2Mel` and `modeling.melspec.WaveToMel` share; the
polyphase table of `ds_resample` (csrc/resample.hip) and its launcher: audio at any integer sample rate in and out; the
cross-fade table of `ds_mel_stitch` (csrc/misc.hip) and its launcher: window mels joined into one long mel; the K-weighting
coefficients and segment plan of the `ds_level_*` entries (csrc/loudness.hip) and their launchers: loudness, true peak, gain;
the plan and the launchers of the `ds_limit_*` entries (csrc/limiter.hip): a look-ahead true-peak limiter behind that gain;
the launchers of `ds_paste_sums` / `ds_paste` (csrc/paste.hip): a recording pasted back over a rendering of it; the region
rules, window table and launchers of the `ds_compare_*` entries (csrc/compare.hip): two waveforms side by side -- lag, SI-SDR,
multi-resolution STFT and log-mel distances.

The reference extracts mels with librosa on the host (Diffsound/vocoder/mel2wav/extract_mel_spectrogram.py:15-38,141-187)
and reads audio with `librosa.load(path, sr=None)` (:167); its data preparation resamples with `librosa.load(path, sr=22050)`
(Codebook/feature_extraction/extract_mel_spectrogram.py:167).  Nothing here needs librosa, resampy or soundfile."""
import math
import struct

import numpy as np
import torch

from . import _lib

N_FFT, HOP = 1024, 256          # the sizes ds_wave_to_mel is built for


def hz_to_mel(f):
    """Slaney's auditory-toolbox scale: linear (200/3 Hz per mel) below 1 kHz, logarithmic above with 27 steps per
    factor 6.4 -- so 1000 Hz is mel 15."""
    f = np.asarray(f, dtype=np.float64)
    lin = f * 3.0 / 200.0
    log = 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) * (27.0 / math.log(6.4))
    return np.where(f >= 1000.0, log, lin)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((m - 15.0) * (math.log(6.4) / 27.0)), m * 200.0 / 3.0)


def mel_filterbank(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """f32[n_mels, 1 + n_fft // 2]: triangular filters with corners equally spaced on the Slaney mel scale between fmin and
    fmax (None: sr / 2), each scaled by 2 / (f_{j+2} - f_j) (unit area per band, "Slaney normalisation") -- what librosa 0.8's
    `filters.mel(sr, n_fft, n_mels, fmin, fmax)` defaults give (extract_mel_spectrogram.py:26, vocoder/modules.py:42-44).
    Built in float64, rounded once."""
    fmax = sr / 2.0 if fmax is None else float(fmax)
    corners = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))          # f_0 .. f_{n_mels + 1}
    bins = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    lo, mid, hi = corners[:-2, None], corners[1:-1, None], corners[2:, None]
    rise = (bins[None, :] - lo) / (mid - lo)
    fall = (hi - bins[None, :]) / (hi - mid)
    tri = np.maximum(0.0, np.minimum(rise, fall))
    return torch.from_numpy((tri * (2.0 / (hi - lo))).astype(np.float32))


def hann_window(n=N_FFT):
    """periodic Hann (torch.hann_window's default, scipy's fftbins=True), float64 -> f32"""
    k = np.arange(n, dtype=np.float64)
    return torch.from_numpy((0.5 - 0.5 * np.cos(2.0 * np.pi * k / n)).astype(np.float32))


def fft_tables():
    """f64[769, 2]: (cos, -sin) of 2 pi m / 512 for m < 512 (the radix-8 passes), then of 2 pi k / 1024 for k <= 256 (the
    real-input split): the kernel's FFT runs in double (include/diffsound_hip.h: ds_wave_to_mel's `twiddle`)."""
    ang = np.concatenate([np.arange(512, dtype=np.float64) / 512.0, np.arange(257, dtype=np.float64) / 1024.0]) * 2.0 * np.pi
    return torch.from_numpy(np.stack([np.cos(ang), -np.sin(ang)], axis=1))


def row_ranges(mel_basis):
    """i32[n_mels, 2]: [k0, k1) of every filterbank row's non-zero entries ((0, 0) for an all-zero row).  Pack-time: one
    host copy of the matrix."""
    nz = mel_basis.detach().cpu() != 0
    n = nz.shape[1]
    any_ = nz.any(1)
    k0 = torch.where(any_, nz.float().argmax(1), torch.zeros(nz.shape[0], dtype=torch.long))
    k1 = torch.where(any_, n - nz.flip(1).float().argmax(1), torch.zeros(nz.shape[0], dtype=torch.long))
    return torch.stack([k0, k1], 1).to(torch.int32).contiguous()


def n_frames(length, pad):
    return 1 + (length + 2 * pad - N_FFT) // HOP


_TABLES = {}


def _twiddle(device):
    key = (device.type, device.index)
    if key not in _TABLES:
        _TABLES[key] = fft_tables().to(device)
    return _TABLES[key]


def wave_to_mel(wave, window, mel_basis, krange, *, pad, length=0, f0=0, n_out=None, a=1.0, c=0.0, lo=-math.inf,
                hi=math.inf, floor=1e-5):
    """ds_wave_to_mel on wave f32[B, T] (device) -> f32[B, n_mels, n_out]; see include/diffsound_hip.h for the formula.
    A host tensor raises (there is no CPU path), and so does a wave too short to reflect -- before anything is launched."""
    if not torch.is_tensor(wave) or wave.dim() != 2:
        raise ValueError("wave must be a tensor f32[B, T]")
    if not wave.is_cuda:
        raise _lib.DiffsoundHipError("wave is not on a GPU: the HIP path has no CPU fallback")
    wave = wave.float().contiguous()
    B, T = wave.shape
    L = length if length else T
    if n_out is None:
        n_out = n_frames(L, pad) - f0
    n_mels = mel_basis.shape[0]
    out = torch.empty(B, n_mels, max(n_out, 0), device=wave.device, dtype=torch.float32)
    _lib.check(_lib.lib().ds_wave_to_mel(_lib.ptr(wave), B, T, int(length), int(pad), _lib.ptr(window),
                                         _lib.ptr(_twiddle(wave.device)), _lib.ptr(mel_basis), _lib.ptr(krange), n_mels,
                                         N_FFT, HOP, int(f0), int(n_out), a, c, lo, hi, floor, _lib.ptr(out), _lib.stream()))
    return out


# the resampling filter: Kaiser-windowed sinc, Z zero crossings a side; beta and rho are the published "kaiser_best" constants
RESAMPLE_ZEROS = 32
RESAMPLE_BETA = 14.769656459379492
RESAMPLE_ROLLOFF = 0.9475937167399596


def _rates(src, dst):
    for r in (src, dst):
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or r < 1:
            raise ValueError("sample rates must be positive integers, got %r" % (r,))
    g = math.gcd(int(src), int(dst))
    return int(dst) // g, int(src) // g


def resample_length(n, src, dst):
    """ceil(n dst / src): the samples `n` input samples give"""
    L, M = _rates(src, dst)
    return (int(n) * L + M - 1) // M


def resample_half_width(src, dst):
    """W = ceil(Z / s): input samples on either side of an output's position that the filter reaches"""
    L, M = _rates(src, dst)
    return int(math.ceil(RESAMPLE_ZEROS / (RESAMPLE_ROLLOFF * min(1.0, L / M))))


def resample_taps(src, dst):
    """(f32[L, 2W+1], L, M, W): row p holds h(p / L - j), j = -W..W, of
        h(t) = s sinc(s t) I0(beta sqrt(1 - (s t / Z)^2)) / I0(beta)  for |s t| < Z, else 0,    s = rho min(1, L / M),
    L / M = dst / src in lowest terms, W = ceil(Z / s) (include/diffsound_hip.h: ds_resample).  Built in float64, rounded
    once."""
    L, M = _rates(src, dst)
    s = RESAMPLE_ROLLOFF * min(1.0, L / M)
    W = resample_half_width(src, dst)
    p = np.arange(L, dtype=np.int64)[:, None]
    j = np.arange(-W, W + 1, dtype=np.int64)[None, :]
    u = s * ((p - j * L).astype(np.float64) / L)                     # s t, t = p / L - j
    inside = np.abs(u) < RESAMPLE_ZEROS
    arg = np.sqrt(np.where(inside, 1.0 - (u / RESAMPLE_ZEROS) ** 2, 0.0))
    h = np.where(inside, s * np.sinc(u) * np.i0(RESAMPLE_BETA * arg) / np.i0(RESAMPLE_BETA), 0.0)
    return torch.from_numpy(h.astype(np.float32)), L, M, W


_RESAMPLE_TABLES = {}


def _resample_table(src, dst, device):
    L, M = _rates(src, dst)
    key = (L, M, device.type, device.index)
    if key not in _RESAMPLE_TABLES:
        taps, _, _, W = resample_taps(src, dst)
        _RESAMPLE_TABLES[key] = (taps.to(device), W)
    return (L, M) + _RESAMPLE_TABLES[key]


def resample(wave, src, dst, *, lengths=None, n_out=None):
    """ds_resample on wave f32[B, T] (device) at `src` Hz -> f32[B, n_out] at `dst` Hz (default n_out = ceil(T dst / src)).
    lengths: per-row sample counts (i32[B] on the device, or a list): row b is x[b, :len_b], zero outside, and its output
    past ceil(len_b dst / src) is zero.  src == dst returns the input without a launch (zero-extended or cut if n_out or
    lengths ask for it).  A host tensor raises (there is no CPU path)."""
    L, M = _rates(src, dst)
    if not torch.is_tensor(wave) or wave.dim() != 2:
        raise ValueError("wave must be a tensor f32[B, T]")
    if n_out is not None and n_out < 0:
        raise ValueError("n_out must be >= 0")
    if L == M and lengths is None and n_out is None:
        return wave
    if not wave.is_cuda:
        raise _lib.DiffsoundHipError("wave is not on a GPU: the HIP path has no CPU fallback")
    wave = wave.float().contiguous()
    B, T = wave.shape
    if lengths is not None:
        lengths = torch.as_tensor(lengths, dtype=torch.int32).to(wave.device).contiguous()
        if lengths.shape != (B,):
            raise ValueError("lengths must hold one count per row")
    if n_out is None:
        n_out = (T * L + M - 1) // M
    if L == M or B == 0 or T == 0 or n_out == 0:          # nothing to filter: the rows as they are, zero-extended or cut
        out = torch.zeros(B, n_out, device=wave.device, dtype=torch.float32)
        n = min(T, n_out) if L == M else 0
        out[:, :n] = wave[:, :n]
        if lengths is not None and n:
            out *= (torch.arange(n_out, device=wave.device)[None, :] < lengths[:, None])
        return out
    out = torch.empty(B, n_out, device=wave.device, dtype=torch.float32)
    _, _, taps, W = _resample_table(src, dst, wave.device)
    _lib.check(_lib.lib().ds_resample(_lib.ptr(wave), B, T, _lib.ptr(lengths), L, M, _lib.ptr(taps), W, _lib.ptr(out),
                                      int(n_out), _lib.stream()))
    return out


# ---- output levelling: BS.1770 loudness, true peak and gain (csrc/loudness.hip) -------------------------------------------------
KW_SHELF = (1681.974450955533, 3.999843853973347, 0.7071752369554196)      # f0 Hz, gain dB, Q of the analogue prototype
KW_SHELF_VB_EXP = 0.4996667741545416
KW_HIGHPASS = (38.13547087602444, 0.5003270373238773)                      # f0 Hz, Q
LEVEL_STRATEGIES = {"peak": -1.0, "rms": -20.0, "loudness": -23.0, "match": None}     # name -> default target (dBFS / LUFS)


def _level_rate(rate):
    if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)) or rate < 1:
        raise ValueError("the sample rate must be a positive integer, got %r" % (rate,))
    return int(rate)


def kweight_coeffs(rate):
    """The K-weighting of ITU-R BS.1770 at any integer rate, from the analogue prototypes, in float64:
    {"shelf": (b f64[3], a f64[3]), "highpass": (b f64[3], a f64[3])} with a[0] = 1 (include/diffsound_hip.h: ds_level_segments).
    At 48 000 Hz these are the seven table values of BS.1770-4."""
    fs = float(_level_rate(rate))
    f0, G, Q = KW_SHELF
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** KW_SHELF_VB_EXP
    a0 = 1.0 + K / Q + K * K
    shelf = (np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]),
             np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    f0, Q = KW_HIGHPASS
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    highpass = (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    return {"shelf": shelf, "highpass": highpass}


def level_plan(rate):
    """{"S": samples per 100-ms segment = floor(0.1 rate + 0.5), "block": 4 S (a 400-ms gating block, hop S), "transition":
    f64[4, 4] = A^S, A the state transition of the two biquads in series in transposed direct form II on (s1, s2, t1, t2) --
    what carries a row's filter state from one segment's start to the next (csrc/loudness.hip)."""
    rate = _level_rate(rate)
    c = kweight_coeffs(rate)
    (_, a), (_, d) = c["shelf"], c["highpass"]
    S = int(math.floor(0.1 * rate + 0.5))
    if S < 1:
        raise ValueError("the sample rate %d is too low for a 100-ms segment" % rate)
    A = np.array([[-a[1], 1.0, 0.0, 0.0],
                  [-a[2], 0.0, 0.0, 0.0],
                  [-2.0 - d[1], 0.0, -d[1], 1.0],
                  [1.0 - d[2], 0.0, -d[2], 0.0]])
    return {"S": S, "block": 4 * S, "transition": np.linalg.matrix_power(A, S)}


_LEVEL_TABLES = {}


def _level_tables(rate, device):
    """(S, kw f64[26] on the device, x4 taps f32[4, 69] on the device)"""
    key = (rate, device.type, device.index)
    if key not in _LEVEL_TABLES:
        c, plan = kweight_coeffs(rate), level_plan(rate)
        kw = np.concatenate([c["shelf"][0], c["shelf"][1][1:], c["highpass"][0], c["highpass"][1][1:],
                             plan["transition"].reshape(-1)])
        taps, L, M, W = resample_taps(1, 4)                    # the table depends on the ratio alone
        assert (L, M, W) == (4, 1, 34) and kw.shape == (26,)
        _LEVEL_TABLES[key] = (plan["S"], torch.from_numpy(kw).to(device), taps.contiguous().to(device))
    return _LEVEL_TABLES[key]


def _level_rows(wave, lengths):
    if not torch.is_tensor(wave) or wave.dim() != 2:
        raise ValueError("wave must be a tensor f32[B, T]")
    if not wave.is_cuda:
        raise _lib.DiffsoundHipError("wave is not on a GPU: the HIP path has no CPU fallback")
    wave = wave.float().contiguous()
    host_lens = None
    if lengths is None:
        host_lens = [wave.shape[1]] * wave.shape[0]
    elif not (torch.is_tensor(lengths) and lengths.is_cuda):
        host_lens = [int(n) for n in torch.as_tensor(lengths).reshape(-1).tolist()]
    if lengths is not None:
        lengths = torch.as_tensor(lengths, dtype=torch.int32).to(wave.device).contiguous()
        if lengths.shape != (wave.shape[0],):
            raise ValueError("lengths must hold one count per row")
    return wave, lengths, host_lens


def _level_run(wave, rate, lengths, strategy, target, target_dev, ceiling_db, counts=False):
    """the three measuring launches and the gain launch on rows already checked -> dict of device tensors (+ 'gain')"""
    B, T = wave.shape
    dev = wave.device
    S, kw, taps = _level_tables(rate, dev)
    n_seg_max = T // S
    L = _lib.lib()
    nbytes = int(L.ds_level_scratch_bytes(B, T, S))
    scratch = torch.empty(nbytes // 8 + 1, device=dev, dtype=torch.float64)
    seg = torch.empty(B, max(n_seg_max, 1), device=dev, dtype=torch.float64)
    lufs = torch.empty(B, device=dev, dtype=torch.float64)
    mean_sq = torch.empty(B, device=dev, dtype=torch.float64)
    peaks = torch.empty(B, 2, device=dev, dtype=torch.float32)
    gain = torch.empty(B, device=dev, dtype=torch.float32)
    cnt = torch.empty(B, 2, device=dev, dtype=torch.int32) if counts else None
    st = _lib.stream()
    _lib.check(L.ds_level_segments(_lib.ptr(wave), B, T, _lib.ptr(lengths), S, _lib.ptr(kw), _lib.ptr(seg), max(n_seg_max, 1),
                                   _lib.ptr(scratch), nbytes, st))
    _lib.check(L.ds_level_true_peak(_lib.ptr(wave), B, T, _lib.ptr(lengths), S, _lib.ptr(taps), _lib.ptr(scratch), nbytes, st))
    _lib.check(L.ds_level_gain(_lib.ptr(seg), max(n_seg_max, 1), B, T, _lib.ptr(lengths), S, int(strategy), float(target),
                               _lib.ptr(target_dev), 0 if target_dev is None else int(target_dev.numel()), float(ceiling_db),
                               _lib.ptr(scratch), nbytes, _lib.ptr(lufs), _lib.ptr(peaks), _lib.ptr(mean_sq), _lib.ptr(cnt),
                               _lib.ptr(gain), st))
    out = {"lufs": lufs, "sample_peak": peaks[:, 0], "true_peak": peaks[:, 1], "rms": mean_sq.sqrt(), "gain": gain,
           "seg": seg[:, :n_seg_max], "peaks": peaks}
    if counts:
        out["gate_counts"] = cnt
    return out


def measure_level(wave, rate, lengths=None, segments=False):
    """The level of wave f32[B, T] (device) at `rate` Hz, row b being wave[b, :lengths[b]] (lengths: i32[B] on the device or a
    list; None = T) -> a dict of device tensors: 'lufs' f64[B] (integrated loudness after BS.1770-4, -inf for silence and
    for rows shorter than four segments), 'sample_peak' f32[B], 'true_peak' f32[B] (x4 through the resampler's own filter,
    never below the sample peak) and 'rms' f64[B].  segments=True adds 'seg' f64[B, T // S], the K-weighted energy of every
    100-ms segment, and 'gate_counts' i32[B, 2], the blocks that pass the absolute gate and both gates.  Four launches, no
    host synchronisation; the formulas are in include/diffsound_hip.h (ds_level_segments).  A host tensor raises."""
    rate = _level_rate(rate)
    wave, lengths, _ = _level_rows(wave, lengths)
    if wave.shape[0] == 0:
        raise ValueError("wave holds no rows")
    r = _level_run(wave, rate, lengths, _lib.LEVEL_MEASURE, 0.0, None, 0.0, counts=segments)
    keys = ("lufs", "sample_peak", "true_peak", "rms") + (("seg", "gate_counts") if segments else ())
    return {k: r[k] for k in keys}


def level(wave, rate, strategy, target=None, ceiling_db=-1.0, lengths=None, reference=None, limit=None):
    """Bring wave f32[B, T] (device, `rate` Hz; lengths as in measure_level) to a level -> (out f32[B, T], gain f32[B]):
    one gain per row, out = gain x in fp32, exact zeros past a row's length.  strategy "peak": the sample peak to `target`
    dBFS (default -1); "rms": the root mean square to `target` dBFS (-20); "loudness": the integrated loudness to `target`
    LUFS (-23); "match": to the integrated loudness of `reference` = (wave, rate, lengths) -- one row, or one per row of
    `wave` --, measured by the same kernels (or an f64 device tensor of 1 or B loudness values such a measurement gave).
    Then the ceiling: a gain that would lift the x4 true peak above ceiling_db dBFS is cut to reach exactly that -- a static
    cut of the whole row, its shape untouched.  A silent row, and under "loudness" / "match" a row shorter than 0.4 s, has
    nothing to scale by and keeps gain 1; where the lengths are known on the host such a short row raises ValueError instead.
    limit=True, or a dict {lookahead_ms, release_ms}: the strategy's gain is NOT cut; it goes to the look-ahead limiter
    (`limit`, same ceiling_db), which takes the row down around the peaks that would cross the ceiling and leaves the rest at
    the gain asked for.  The returned gain is then that uncut gain g0.  Limiting lowers loudness, so a limited clip lands under
    its target by what was limited; `limit` reports the loudness reached, and nothing iterates towards the target.
    limit=None: the static cut, the launches and the bits of before.  Everything stays on the device and nothing synchronises."""
    rate = _level_rate(rate)
    limit = _limit_spec(limit)
    plan = None if limit is None else limit_plan(rate, **limit)     # raises on a look-ahead or a release this rate cannot take
    if strategy not in LEVEL_STRATEGIES:
        raise ValueError("strategy must be one of %s, got %r" % (", ".join(sorted(LEVEL_STRATEGIES)), strategy))
    if (strategy == "match") != (reference is not None):
        raise ValueError('reference goes with strategy "match" and "match" needs one')
    if strategy == "match" and target is not None:
        raise ValueError('"match" takes its target from the reference')
    target = LEVEL_STRATEGIES[strategy] if target is None else float(target)
    ceiling_db = float(ceiling_db)
    if strategy != "match" and not math.isfinite(target) or not math.isfinite(ceiling_db):
        raise ValueError("target and ceiling_db must be finite")
    wave, lengths, host_lens = _level_rows(wave, lengths)
    if wave.shape[0] == 0:
        raise ValueError("wave holds no rows")
    block = level_plan(rate)["block"]
    if strategy in ("loudness", "match") and host_lens is not None and min(host_lens) < block:
        raise ValueError("loudness needs at least one 400-ms block (%d samples at %d Hz); a row has %d"
                         % (block, rate, min(host_lens)))
    target_dev = None
    if strategy == "match":
        if torch.is_tensor(reference):
            target_dev = reference
            if not target_dev.is_cuda:
                raise _lib.DiffsoundHipError("the reference loudness is not on a GPU: the HIP path has no CPU fallback")
            target_dev = target_dev.to(torch.float64).reshape(-1).contiguous()
        else:
            ref = tuple(reference)
            if len(ref) not in (2, 3):
                raise ValueError("reference is (wave, rate) or (wave, rate, lengths)")
            rwave, rlens, rhost = _level_rows(ref[0], ref[2] if len(ref) == 3 else None)
            rrate = _level_rate(ref[1])
            if rhost is not None and rwave.shape[0] and min(rhost) < level_plan(rrate)["block"]:
                raise ValueError("the reference is shorter than one 400-ms block")
            target_dev = measure_level(rwave, rrate, rlens)["lufs"]
        if target_dev.numel() not in (1, wave.shape[0]):
            raise ValueError("the reference holds %d rows for %d clips" % (target_dev.numel(), wave.shape[0]))
    code = {"peak": _lib.LEVEL_PEAK, "rms": _lib.LEVEL_RMS, "loudness": _lib.LEVEL_LOUDNESS, "match": _lib.LEVEL_LOUDNESS}[strategy]
    if plan is not None:                                 # the gain as the strategy gives it: no ceiling is in its way
        r = _level_run(wave, rate, lengths, code, 0.0 if target is None else target, target_dev, _NO_CEILING_DB)
        out, _ = _limit_run(wave, rate, lengths, r["gain"], ceiling_db, plan, False)
        return out, r["gain"]
    r = _level_run(wave, rate, lengths, code, 0.0 if target is None else target, target_dev, ceiling_db)
    out = torch.empty_like(wave)
    _lib.check(_lib.lib().ds_level_apply(_lib.ptr(wave), _lib.ptr(r["gain"]), _lib.ptr(out), wave.shape[0], wave.shape[1],
                                         _lib.ptr(lengths), _lib.stream()))
    return out, r["gain"]


# ---- the look-ahead true-peak limiter behind a levelling gain (csrc/limiter.hip) ---------------------------------------------
LIMIT_LOOKAHEAD_MS = 1.5
LIMIT_RELEASE_MS = 50.0
LIMIT_BLOCK = 1024             # = ds_limit_block(), checked where the library is used: the look-ahead may not exceed it
_NO_CEILING_DB = 1000.0        # a ceiling no fp32 gain times an fp32 peak reaches: ds_level_gain then returns the strategy's own gain


def limit_plan(rate, lookahead_ms=LIMIT_LOOKAHEAD_MS, release_ms=LIMIT_RELEASE_MS):
    """{"L": look-ahead in samples = round(lookahead_ms rate / 1000), 1 <= L <= 0.01 rate; "a": the release coefficient per
    sample exp(-1000 / (release_ms rate)), float64; "w": f64[L + 1], the smoothing weights -- a Hann shape without its zero
    ends (np.hanning(L + 3)[1:-1]), normalised to sum 1} (include/diffsound_hip.h: ds_limit_envelope).  The kernels' block
    holds ds_limit_block() = 1024 samples and L may not exceed it: up to 10 ms at 102 400 Hz."""
    rate = _level_rate(rate)
    lookahead_ms, release_ms = float(lookahead_ms), float(release_ms)
    if not (math.isfinite(lookahead_ms) and lookahead_ms > 0.0):
        raise ValueError("lookahead_ms must be positive and finite, got %r" % (lookahead_ms,))
    if not (math.isfinite(release_ms) and release_ms > 0.0):
        raise ValueError("release_ms must be positive and finite, got %r" % (release_ms,))
    L = int(math.floor(lookahead_ms * rate / 1000.0 + 0.5))
    if L < 1 or L > 0.01 * rate:
        raise ValueError("the look-ahead of %g ms is %d samples at %d Hz; it must be 1 .. %d" % (lookahead_ms, L, rate, int(0.01 * rate)))
    if L > LIMIT_BLOCK:
        raise ValueError("the look-ahead of %d samples exceeds the limiter's block of %d" % (L, LIMIT_BLOCK))
    a = math.exp(-1000.0 / (release_ms * rate))
    if not a < 1.0:
        raise ValueError("release_ms = %g does not release at %d Hz" % (release_ms, rate))
    w = np.hanning(L + 3)[1:-1].astype(np.float64)
    return {"L": L, "a": a, "w": w / w.sum()}


_LIMIT_TABLES = {}


def _limit_spec(limit):
    """level's `limit` keyword -> None or the keyword arguments of limit_plan"""
    if limit is None or limit is False:
        return None
    if limit is True:
        return {}
    if not isinstance(limit, dict) or set(limit) - {"lookahead_ms", "release_ms"}:
        raise ValueError("limit is None, True or a dict {lookahead_ms, release_ms}, got %r" % (limit,))
    return {k: float(v) for k, v in limit.items()}


def _limit_run(wave, rate, lengths, gain, ceiling_db, plan, return_curve):
    """the limiter's launches on rows already checked -> (out, info)"""
    B, T = wave.shape
    dev = wave.device
    lib = _lib.lib()
    if int(lib.ds_limit_block()) != LIMIT_BLOCK:
        raise RuntimeError("libdiffsound_hip's limiter block is %d, audio.LIMIT_BLOCK is %d" % (lib.ds_limit_block(), LIMIT_BLOCK))
    S, kw, taps = _level_tables(rate, dev)
    L, a = plan["L"], plan["a"]
    key = (rate, L, dev.type, dev.index)
    if key not in _LIMIT_TABLES:
        _LIMIT_TABLES[key] = torch.from_numpy(np.ascontiguousarray(plan["w"])).to(dev)
    w = _LIMIT_TABLES[key]
    nbytes = int(lib.ds_limit_scratch_bytes(B, T, L))
    scratch = torch.empty(nbytes // 8 + 1, device=dev, dtype=torch.float64)
    out = torch.empty_like(wave)
    curve = torch.empty_like(wave) if return_curve else None
    st = _lib.stream()
    _lib.check(lib.ds_limit_envelope(_lib.ptr(wave), B, T, _lib.ptr(lengths), _lib.ptr(taps), _lib.ptr(gain), ceiling_db, L, a,
                                     _lib.ptr(scratch), nbytes, st))
    _lib.check(lib.ds_limit_carry(B, T, _lib.ptr(lengths), L, a, _lib.ptr(scratch), nbytes, st))
    _lib.check(lib.ds_limit_apply(_lib.ptr(wave), B, T, _lib.ptr(lengths), _lib.ptr(gain), L, a, _lib.ptr(w), _lib.ptr(out),
                                  _lib.ptr(curve), _lib.ptr(scratch), nbytes, st))
    m = _level_run(out, rate, lengths, _lib.LEVEL_MEASURE, 0.0, None, 0.0)          # a varying gain moves the x4 peaks: measure again
    trim = torch.empty(B, device=dev, dtype=torch.float32)
    true_peak, max_red = torch.empty_like(trim), torch.empty_like(trim)
    lufs = torch.empty(B, device=dev, dtype=torch.float64)
    _lib.check(lib.ds_limit_finish(B, T, L, ceiling_db, _lib.ptr(m["lufs"]), _lib.ptr(m["peaks"]), _lib.ptr(scratch), nbytes,
                                   _lib.ptr(trim), _lib.ptr(lufs), _lib.ptr(true_peak), _lib.ptr(max_red), st))
    _lib.check(lib.ds_level_apply(_lib.ptr(out), _lib.ptr(trim), _lib.ptr(out), B, T, _lib.ptr(lengths), st))
    info = {"gain": gain, "trim": trim, "max_reduction": max_red, "lufs": lufs, "true_peak": true_peak}
    if return_curve:
        info["curve"] = curve
    return out, info


def limit(wave, rate, ceiling_db=-1.0, gain=None, lookahead_ms=LIMIT_LOOKAHEAD_MS, release_ms=LIMIT_RELEASE_MS, lengths=None,
          return_curve=False):
    """A look-ahead true-peak limiter on wave f32[B, T] (device, `rate` Hz; lengths as in measure_level) -> (out f32[B, T], info).
    gain: f32[B] on the device, the gain g0 each row is to get (None: 1).  Where g0 would lift the x4 true peak above
    ceiling_db dBFS, a gain curve g <= 1 -- the reduction every peak asks for, seen lookahead_ms ahead, held, released
    exponentially over release_ms and smoothed by a Hann shape over the look-ahead -- takes the row down around those peaks:
    out = (g0 g) x in fp32, exact zeros past a row's length (include/diffsound_hip.h: ds_limit_envelope has the formulas).
    `out` is then measured again and cut statically by `trim` <= 1 (1 where nothing is left above the ceiling), so its x4 true
    peak and its sample peak are at or under the ceiling.  info holds device tensors: 'gain' f32[B] = g0, 'trim' f32[B],
    'max_reduction' f32[B] = 1 - min g, 'lufs' f64[B] and 'true_peak' f32[B] of `out` as returned, and with return_curve
    'curve' f32[B, T] = g (1 past a row's length).  Limiting lowers loudness: a row limited after a loudness gain lands under
    that target by what was limited -- 'lufs' reports where, nothing iterates.  Eight entries, no host synchronisation; a row
    that needs no limiting comes out as ds_level_apply would give it, bit for bit.  A host tensor raises."""
    rate = _level_rate(rate)
    ceiling_db = float(ceiling_db)
    if not math.isfinite(ceiling_db):
        raise ValueError("ceiling_db must be finite")
    plan = limit_plan(rate, lookahead_ms, release_ms)
    wave, lengths, _ = _level_rows(wave, lengths)
    B, T = wave.shape
    if B == 0 or T == 0:
        raise ValueError("wave holds no rows or no samples")
    if gain is None:
        gain = torch.ones(B, device=wave.device, dtype=torch.float32)
    else:
        if not torch.is_tensor(gain):
            raise ValueError("gain must be a tensor f32[B] on the device")
        if not gain.is_cuda:
            raise _lib.DiffsoundHipError("gain is not on a GPU: the HIP path has no CPU fallback")
        gain = gain.float().reshape(-1).contiguous()
        if gain.shape != (B,):
            raise ValueError("gain must hold one value per row")
    return _limit_run(wave, rate, lengths, gain, ceiling_db, plan, bool(return_curve))


def fade_table(V):
    """f32[V]: the weight of the LATER window over the V frames two neighbouring windows share (ds_mel_stitch),
        fade[f] = sin^2(pi (f + 1/2) / (2 V)):
    strictly increasing from ~0 to ~1 and symmetric, fade[f] + fade[V-1-f] = 1; the earlier window's weight is 1 - fade[f].
    Built in float64, rounded once (like the resampler's polyphase table)."""
    V = int(V)
    if V < 0:
        raise ValueError("the overlap must be >= 0 frames, got %d" % V)
    f = np.arange(V, dtype=np.float64)
    return torch.from_numpy((np.sin(np.pi * (f + 0.5) / (2.0 * max(V, 1))) ** 2).astype(np.float32))


_FADE_TABLES = {}


def _fade_table(V, device):
    key = (int(V), device.type, device.index)
    if key not in _FADE_TABLES:
        _FADE_TABLES[key] = fade_table(V).to(device)
    return _FADE_TABLES[key]


def stitch_mel(win, hop_frames, scale=1.0, shift=0.0):
    """ds_mel_stitch on win f32[B, W, C, F] (device): window w starts at frame w hop_frames; the F - hop_frames frames two
    neighbours share are cross-faded with fade_table -> f32[B, C, F + (W - 1) hop_frames], then scale x + shift.  W = 1 is a
    scaled copy.  F and hop_frames must be multiples of 4 and F / 2 <= hop_frames <= F (at most two windows cover a frame):
    otherwise the library's argument error is raised and nothing is launched.  A host tensor raises (there is no CPU path)."""
    if not torch.is_tensor(win) or win.dim() != 4:
        raise ValueError("win must be a tensor f32[B, W, C, F]")
    if not win.is_cuda:
        raise _lib.DiffsoundHipError("win is not on a GPU: the HIP path has no CPU fallback")
    win = win.float().contiguous()
    B, W, C, F = win.shape
    S = int(hop_frames)
    V = F - S
    fade = _fade_table(V, win.device) if 0 < V <= S else None        # (an overlap out of range is the library's to refuse)
    out = torch.empty(B, C, max(F + (W - 1) * S, 0), device=win.device, dtype=torch.float32)
    _lib.check(_lib.lib().ds_mel_stitch(_lib.ptr(win), _lib.ptr(fade), _lib.ptr(out), B, W, C, F, S, float(scale), float(shift),
                                        _lib.stream()))
    return out


# ---- pasting a recording back over a rendering of it (csrc/paste.hip) ----------------------------------------------------------
PASTE_CURVES = {"equal_power": _lib.PASTE_EQUAL_POWER, "linear": _lib.PASTE_LINEAR}


def _paste_rows(ren, rec, keep_cols, off, rec_len, col_num, col_den):
    """the checked, contiguous device operands the two paste entries share"""
    if not torch.is_tensor(ren) or not torch.is_tensor(rec) or ren.dim() not in (2, 3) or rec.dim() != ren.dim():
        raise ValueError("ren and rec must be tensors f32[B, T] or f32[B, C, T] of the same rank")
    if not ren.is_cuda or not rec.is_cuda:
        raise _lib.DiffsoundHipError("ren / rec is not on a GPU: the HIP path has no CPU fallback")
    if ren.shape[:-1] != rec.shape[:-1]:
        raise ValueError("ren %s and rec %s differ in rows" % (tuple(ren.shape), tuple(rec.shape)))
    ren, rec = ren.float().contiguous(), rec.float().contiguous()
    B = ren.shape[0]
    keep_cols = torch.as_tensor(keep_cols)
    if keep_cols.dim() != 2 or keep_cols.shape[0] != B or keep_cols.shape[1] < 1:
        raise ValueError("keep_cols must be u8[B, n_cols] with n_cols >= 1")
    keep_cols = (keep_cols != 0).to(torch.uint8).to(ren.device).contiguous()
    off = torch.as_tensor(off, dtype=torch.int64).reshape(-1)
    off = (off.expand(B) if off.numel() == 1 else off).to(ren.device).contiguous()
    if off.shape != (B,):
        raise ValueError("off must hold one offset, or one per clip")
    if rec_len is not None:
        rec_len = torch.as_tensor(rec_len, dtype=torch.int32).to(ren.device).contiguous()
        if rec_len.shape != (B,):
            raise ValueError("rec_len must hold one length per clip")
    for v in (col_num, col_den):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("col_num and col_den must be integers, got %r" % (v,))
    return ren, rec, keep_cols, off, rec_len


def paste_sums(ren, rec, keep_cols, *, off=0, col_num, col_den=1, rec_len=None):
    """ds_paste_sums on ren f32[B, T] and rec f32[B, Tr] (device) -> sums f64[B, 2] on the device: over the positions of kept
    columns whose recording index n + off[b] is inside the recording, S_o = sum rec^2 and S_r = sum ren^2 in float64, in a
    fixed order (include/diffsound_hip.h: ds_paste).  Two launches, no host synchronisation."""
    ren, rec, keep_cols, off, rec_len = _paste_rows(ren, rec, keep_cols, off, rec_len, col_num, col_den)
    if ren.dim() != 2:
        raise ValueError("the sums are taken over waveforms f32[B, T]")
    B, T = ren.shape
    L = _lib.lib()
    nbytes = max(int(L.ds_paste_scratch_bytes(B, T)), 8)
    scratch = torch.empty(nbytes // 8, device=ren.device, dtype=torch.float64)
    sums = torch.empty(B, 2, device=ren.device, dtype=torch.float64)
    _lib.check(L.ds_paste_sums(_lib.ptr(ren), _lib.ptr(rec), B, T, rec.shape[1], _lib.ptr(off), _lib.ptr(rec_len),
                               _lib.ptr(keep_cols), keep_cols.shape[1], int(col_num), int(col_den), _lib.ptr(scratch), nbytes,
                               _lib.ptr(sums), _lib.stream()))
    return sums


def paste(ren, rec, keep_cols, *, off=0, col_num, col_den=1, fade_len=0.0, curve="equal_power", rec_len=None, sums=None,
          match_gain=False):
    """ds_paste: the recording `rec` over its rendering `ren` (both on the device, f32[B, T] / f32[B, Tr] waveforms or
    f32[B, C, T] / f32[B, C, Tr] mel images) -> out like ren.  keep_cols u8[B, n_cols]: the kept columns, each col_num / col_den
    positions long; position n reads the recording at n + off[b] (off: one offset or one per clip; outside [0, rec_len[b]) the
    recording is 0).  In kept columns out is a bit copy of the recording; the rest is the rendering, cross-faded into the
    recording over fade_len positions at the edge of a kept column, inside the regenerated column (curve "equal_power":
    sin / cos, for waveforms; "linear": for mel images).  sums (paste_sums) or match_gain=True (waveforms, "equal_power"): the
    rendering is scaled by g = sqrt(S_o / S_r) clamped to [1/4, 4].  The formula is in include/diffsound_hip.h (ds_paste).
    No host synchronisation; a host tensor raises (there is no CPU path)."""
    if curve not in PASTE_CURVES:
        raise ValueError("curve must be one of %s, got %r" % (", ".join(sorted(PASTE_CURVES)), curve))
    ren, rec, keep_cols, off, rec_len = _paste_rows(ren, rec, keep_cols, off, rec_len, col_num, col_den)
    if match_gain and sums is None:
        sums = paste_sums(ren, rec, keep_cols, off=off, col_num=col_num, col_den=col_den, rec_len=rec_len)
    if sums is not None:
        if not (torch.is_tensor(sums) and sums.is_cuda and sums.dtype == torch.float64 and tuple(sums.shape) == (ren.shape[0], 2)):
            raise ValueError("sums must be f64[B, 2] on the device (paste_sums)")
        sums = sums.contiguous()
    B, T = ren.shape[0], ren.shape[-1]
    C = ren.shape[1] if ren.dim() == 3 else 1
    out = torch.empty_like(ren)
    _lib.check(_lib.lib().ds_paste(_lib.ptr(ren), _lib.ptr(rec), _lib.ptr(out), B, C, T, rec.shape[-1], _lib.ptr(off),
                                   _lib.ptr(rec_len), _lib.ptr(keep_cols), keep_cols.shape[1], int(col_num), int(col_den),
                                   float(fade_len), PASTE_CURVES[curve], _lib.ptr(sums), _lib.stream()))
    return out


# ---- two waveforms side by side: lag, SI-SDR / SNR, multi-resolution STFT and log-mel distances (csrc/compare.hip) --------------
COMPARE_MAX_LAG = 4096          # = ds_compare_max_lag(): one token column.  A design choice, not a limit of the method
# (window, hop) of the three STFT resolutions, all through the one 1024-point FFT the tree has (windows zero-padded to it).
# Parallel WaveGAN's resolutions are FFT 512 / 1024 / 2048; these are this project's own and numbers are not comparable.
COMPARE_RESOLUTIONS = ((256, 64), (512, 128), (1024, 256))
COMPARE_MEL_RATE = 22050        # the one rate the log-mel distance is defined at (Audio2Mel's filterbank)

_COMPARE_TABLES = {}


def _compare_windows(device):
    key = (device.type, device.index)
    if key not in _COMPARE_TABLES:
        win = torch.zeros(len(COMPARE_RESOLUTIONS), N_FFT)
        for i, (w, _) in enumerate(COMPARE_RESOLUTIONS):
            win[i, :w] = hann_window(w)
        _COMPARE_TABLES[key] = win.to(device)
    return _COMPARE_TABLES[key]


def compare_region(n_a, n_b, max_lag=0, lag=None, region=None, min_len=1):
    """The region [s0, s1) of b that align / compare work on, checked on the host -> (s0, s1).  Default: every sample of b whose
    partner in a exists at every lag in question -- [max_lag, min(n_a, n_b) - max_lag) for a search, [max(0, -lag),
    min(n_b, n_a - lag)) at a host integer lag, [0, min(n_a, n_b)) at a lag on the device.  A region must be non-empty (compare:
    at least 1024 samples), inside b, and keep s0 - max_lag >= 0 and s1 + max_lag <= n_a (at an integer lag: s0 + lag >= 0 and
    s1 + lag <= n_a); anything else raises ValueError.  The region is the same for every row: per-row lengths are not built."""
    max_lag = _compare_max_lag(max_lag)
    host_lag = lag if isinstance(lag, (int, np.integer)) and not isinstance(lag, bool) else None
    if region is None:
        if host_lag is not None:
            s0, s1 = max(0, -int(host_lag)), min(n_b, n_a - int(host_lag))
        else:
            s0, s1 = max_lag, min(n_a, n_b) - max_lag
    else:
        try:
            s0, s1 = region
        except (TypeError, ValueError):
            raise ValueError("region is a pair (s0, s1) of sample indices of b, got %r" % (region,))
        for v in (s0, s1):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("region is a pair of integers, got %r" % (region,))
        s0, s1 = int(s0), int(s1)
    if not (0 <= s0 < s1 <= n_b):
        raise ValueError("the region [%d, %d) must be non-empty and inside b's %d samples" % (s0, s1, n_b))
    if s1 - s0 < min_len:
        raise ValueError("the region [%d, %d) holds %d samples; at least %d are needed" % (s0, s1, s1 - s0, min_len))
    lo, hi = (s0 + int(host_lag), s1 + int(host_lag)) if host_lag is not None else (s0 - max_lag, s1 + max_lag)
    if lo < 0 or hi > n_a:
        raise ValueError("the region [%d, %d) reaches samples [%d, %d) of a, which holds %d" % (s0, s1, lo, hi, n_a))
    return s0, s1


def _compare_max_lag(max_lag):
    if isinstance(max_lag, bool) or not isinstance(max_lag, (int, np.integer)) or not 0 <= max_lag <= COMPARE_MAX_LAG:
        raise ValueError("max_lag must be an integer in 0..%d, got %r" % (COMPARE_MAX_LAG, max_lag))
    return int(max_lag)


def _compare_rows(a, b):
    """the checks of the two inputs that need no device: ValueError; then the device check"""
    for name, x in (("a", a), ("b", b)):
        if not torch.is_tensor(x) or x.dim() != 2 or x.dtype != torch.float32:
            raise ValueError("%s must be a tensor f32[B, N]" % name)
        if not x.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
    if a.shape[0] != b.shape[0] or a.shape[0] < 1:
        raise ValueError("a holds %d rows and b %d: one row of each per comparison, at least one" % (a.shape[0], b.shape[0]))
    if a.shape[1] < 1 or b.shape[1] < 1:
        raise ValueError("a and b must hold samples")


def _compare_device(a, b):
    if not a.is_cuda or not b.is_cuda:
        raise _lib.DiffsoundHipError("a / b is not on a GPU: the HIP path has no CPU fallback")
    if int(_lib.lib().ds_compare_max_lag()) != COMPARE_MAX_LAG:
        raise RuntimeError("libdiffsound_hip's lag cap is %d, audio.COMPARE_MAX_LAG is %d" % (_lib.lib().ds_compare_max_lag(), COMPARE_MAX_LAG))


def _compare_align(a, b, s0, s1, max_lag, lag):
    """ds_compare_align -> (lag i32[B], rho f64[B], sums f64[B, 3], scratch, its bytes); lag: None (search), int, or i32[B]"""
    B, dev = a.shape[0], a.device
    L = _lib.lib()
    nbytes = int(L.ds_compare_scratch_bytes(B, s1 - s0, max_lag))
    scratch = torch.empty(nbytes // 8 + 1, device=dev, dtype=torch.float64)
    lag_out = torch.empty(B, device=dev, dtype=torch.int32)
    rho = torch.empty(B, device=dev, dtype=torch.float64)
    sums = torch.empty(B, 3, device=dev, dtype=torch.float64)
    lag_dev = lag if torch.is_tensor(lag) else None
    _lib.check(L.ds_compare_align(_lib.ptr(a), _lib.ptr(b), B, a.shape[1], b.shape[1], s0, s1, max_lag, _lib.ptr(lag_dev),
                                  0 if lag is None or lag_dev is not None else int(lag), _lib.ptr(scratch), nbytes,
                                  _lib.ptr(lag_out), _lib.ptr(rho), _lib.ptr(sums), _lib.stream()))
    return lag_out, rho, sums, scratch, nbytes


def align(a, b, max_lag, region=None):
    """The lag at which b f32[B, Nb] lines up with its reference a f32[B, Na] (device, contiguous, same rate) -> (lag i32[B],
    rho f64[B]) on the device: lag l pairs b[n] with a[n + l]; over |l| <= max_lag <= 4096 the normalised correlation
    rho(l) = sum b[n] a[n+l] / sqrt(sum a[n+l]^2 sum b[n]^2) over the region (compare_region) is formed in float64 and the l of
    largest rho is chosen on the device -- among bit-equal rho the smallest |l|, then the negative one.  rho is exactly 0 where
    either energy is 0.  Two launches, no host synchronisation; a row's bits do not depend on the batch around it.  The formulas
    are in include/diffsound_hip.h (ds_compare_align).  A host tensor raises (there is no CPU path)."""
    max_lag = _compare_max_lag(max_lag)
    _compare_rows(a, b)
    s0, s1 = compare_region(a.shape[1], b.shape[1], max_lag, None, region)
    _compare_device(a, b)
    lag, rho, _, _, _ = _compare_align(a, b, s0, s1, max_lag, None)
    return lag, rho


def compare(a, b, *, max_lag=0, lag=None, region=None, rate=22050):
    """b f32[B, Nb], the waveform under test, against its reference a f32[B, Na] (device, contiguous, both at `rate` Hz) -> a
    dict of device tensors:
      'lag' i32[B], 'rho' f64[B]   align's search over |l| <= max_lag; or lag= an int or an i32[B] device tensor, which skips
                                   the search (rho is then the correlation at that lag; samples a device lag reaches outside a
                                   count as 0)
      'si_sdr_db' f64[B]           10 log10(alpha^2 ea / sum (b - alpha a)^2), alpha = r / ea: +inf for a zero residual, else -inf
                                   where alpha^2 ea is 0.  The residual is summed directly, sample by sample
      'snr_db' f64[B]              10 log10(ea / sum (b - a)^2), same two rules
      'sc', 'logmag' f64[B, 3]     per resolution of COMPARE_RESOLUTIONS: spectral convergence |A - B|_F / |A|_F and the mean of
                                   |ln max(A, 1e-5) - ln max(B, 1e-5)| over the frames lying wholly inside the region (no
                                   reflection) and bins 0..512 of a 1024-point FFT
      'mel_l1' f64[B]              the mean |difference| of Audio2Mel's log10 mel (ds_wave_to_mel) of the two aligned cuts
                                   a[s0 + l : s1 + l] and b[s0 : s1], reduced in float64 -- only at rate == 22050, the rate
                                   that filterbank is defined at: at another rate the key is absent, not approximated.
    region (compare_region) is the same for every row and holds at least 1024 samples.  Everything is float64 over fixed
    partitions in a fixed order; nothing synchronises.  What these numbers say about a trained model is unmeasured.  The formulas
    are in include/diffsound_hip.h (ds_compare_align).  A host tensor raises (there is no CPU path)."""
    rate = _level_rate(rate)
    max_lag = _compare_max_lag(max_lag)
    _compare_rows(a, b)
    B = a.shape[0]
    if lag is not None:
        if max_lag != 0:
            raise ValueError("lag= skips the search: max_lag must be 0 with it")
        if torch.is_tensor(lag):
            if lag.dtype != torch.int32 or tuple(lag.shape) != (B,) or not lag.is_contiguous():
                raise ValueError("a lag tensor must be i32[B], contiguous, on the device")
        elif isinstance(lag, bool) or not isinstance(lag, (int, np.integer)):
            raise ValueError("lag must be None, an int or an i32[B] device tensor, got %r" % (lag,))
    s0, s1 = compare_region(a.shape[1], b.shape[1], max_lag, lag, region, min_len=N_FFT)
    _compare_device(a, b)
    if torch.is_tensor(lag) and not lag.is_cuda:
        raise _lib.DiffsoundHipError("lag is not on a GPU: the HIP path has no CPU fallback")
    dev = a.device
    L = _lib.lib()
    lag_out, rho, sums, scratch, nbytes = _compare_align(a, b, s0, s1, max_lag, lag)
    st = _lib.stream()
    Na, Nb = a.shape[1], b.shape[1]
    _lib.check(L.ds_compare_residual(_lib.ptr(a), _lib.ptr(b), B, Na, Nb, s0, s1, max_lag, _lib.ptr(lag_out), _lib.ptr(sums),
                                     _lib.ptr(scratch), nbytes, st))
    _lib.check(L.ds_compare_stft(_lib.ptr(a), _lib.ptr(b), B, Na, Nb, s0, s1, max_lag, _lib.ptr(lag_out),
                                 _lib.ptr(_compare_windows(dev)), _lib.ptr(_twiddle(dev)), _lib.ptr(scratch), nbytes, st))
    out = {"lag": lag_out, "rho": rho,
           "si_sdr_db": torch.empty(B, device=dev, dtype=torch.float64), "snr_db": torch.empty(B, device=dev, dtype=torch.float64),
           "sc": torch.empty(B, 3, device=dev, dtype=torch.float64), "logmag": torch.empty(B, 3, device=dev, dtype=torch.float64)}
    _lib.check(L.ds_compare_finish(B, s0, s1, max_lag, _lib.ptr(sums), _lib.ptr(scratch), nbytes, _lib.ptr(out["si_sdr_db"]),
                                   _lib.ptr(out["snr_db"]), _lib.ptr(out["sc"]), _lib.ptr(out["logmag"]), st))
    if rate == COMPARE_MEL_RATE:
        key = ("mel", dev.type, dev.index)
        if key not in _COMPARE_TABLES:
            basis = mel_filterbank(COMPARE_MEL_RATE, N_FFT, 80)
            _COMPARE_TABLES[key] = (hann_window(N_FFT).to(dev), basis.to(dev), row_ranges(basis).to(dev))
        window, basis, krange = _COMPARE_TABLES[key]
        pad = (N_FFT - HOP) // 2
        idx = torch.arange(s0, s1, device=dev)[None, :] + lag_out[:, None].long()       # the cut of a, by the device's own lag
        cut = torch.where((idx >= 0) & (idx < Na), a.gather(1, idx.clamp(0, Na - 1)), torch.zeros((), device=dev))
        ma = wave_to_mel(cut, window, basis, krange, pad=pad)
        mb = wave_to_mel(b[:, s0:s1].contiguous(), window, basis, krange, pad=pad)
        out["mel_l1"] = torch.empty(B, device=dev, dtype=torch.float64)
        _lib.check(L.ds_compare_l1(_lib.ptr(ma), _lib.ptr(mb), B, ma.shape[1] * ma.shape[2], _lib.ptr(out["mel_l1"]), st))
    return out


def read_wav(path, rate=None):
    """RIFF/WAVE file -> (f32[T] mono in [-1, 1), sample rate): PCM_16 / PCM_24 / PCM_32 and IEEE float32, channels
    averaged; the inverse of pipeline.write_wav_pcm24.  rate: the rate the caller needs -- another one raises (the
    reference's `librosa.load(sr=None)` does not resample either, extract_mel_spectrogram.py:167)."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError("%s: not a RIFF/WAVE file" % path)
    fmt, raw, pos = None, None, 12
    while pos + 8 <= len(data):
        tag, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if tag == b"fmt ":
            fmt = body
        elif tag == b"data":
            raw = body
        pos += 8 + size + (size & 1)          # chunks are word-aligned
    if fmt is None or raw is None or len(fmt) < 16:
        raise ValueError("%s: no fmt / data chunk" % path)
    code, channels, sr, _, _, bits = struct.unpack("<HHIIHH", fmt[:16])
    if code == 0xFFFE and len(fmt) >= 26:     # WAVE_FORMAT_EXTENSIBLE: the real code leads the sub-format GUID
        code = struct.unpack("<H", fmt[24:26])[0]
    if channels < 1:
        raise ValueError("%s: no channels" % path)
    step = channels * (bits // 8)
    raw = raw[:len(raw) // step * step]
    if code == 1 and bits == 16:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float64) / 32768.0
    elif code == 1 and bits == 24:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = (v - ((v & 0x800000) << 1)).astype(np.float64) / 8388608.0
    elif code == 1 and bits == 32:
        x = np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0
    elif code == 3 and bits == 32:
        x = np.frombuffer(raw, dtype="<f4").astype(np.float64)
    else:
        raise ValueError("%s: unsupported sample format (code %d, %d bits)" % (path, code, bits))
    x = x.reshape(-1, channels).mean(1).astype(np.float32)
    if rate is not None and sr != rate:
        raise ValueError("%s: sample rate %d, the model needs %d (resample the file first)" % (path, sr, rate))
    return torch.from_numpy(x), sr
