"""The yardstick of the tests of audio.align / audio.compare: the definitions of include/diffsound_hip.h (ds_compare_align)
evaluated with numpy on the host, in float64 (the reference value) and -- the same text with another dtype -- in float32 (the
"twin": products, sums, FFT, logarithms and ratios all in float32), whose distance to float64 on a case is that case's d32.
The three sums rho is made of are exactly rounded in the float64 evaluation (math.fsum): where rho is within a few roundings of
1 a pairwise sum's own error would be as large as the float32 twin's distance.
The log-mel distance is DEFINED on the project's Audio2Mel (fp32, ds_wave_to_mel) and reduced in float64, so its yardstick is
the float64 mean over fp32 mels that `mel_fn` supplies for the two cuts this module makes on the host: on the GPU the project's
existing Audio2Mel module (tests/test_hip_audio.py holds it to the float64 formula), without a device the float32 formula of
tests/audio_reference.py.  Never the code under test: not the cut, not the reduction.

A lag l pairs b[n] with a[n + l]; the region [s0, s1) of b must keep every sample it pairs inside a."""
import math

import numpy as np
import torch

import audio_reference as AR

RESOLUTIONS = ((256, 64), (512, 128), (1024, 256))      # (window, hop), all zero-padded to one 1024-point FFT
N_FFT = 1024
BINS = 513
FLOOR = 1e-5
MAX_LAG = 4096
KEYS = ("rho", "si_sdr_db", "snr_db", "sc", "logmag", "mel_l1")


def default_region(n_a, n_b, max_lag):
    return max_lag, min(n_a, n_b) - max_lag


def check_region(n_a, n_b, s0, s1, max_lag):
    assert 0 <= s0 < s1 <= n_b and s0 - max_lag >= 0 and s1 + max_lag <= n_a, (n_a, n_b, s0, s1, max_lag)


def hann(w):
    """periodic Hann in float64, rounded to float32 once: the window values the definition names"""
    k = np.arange(w, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * k / w)).astype(np.float32)


def correlations(a, b, s0, s1, max_lag, dtype=np.float64):
    """(lags i64[2M+1], r, ea, eb) of one row pair: r(l) = sum b[n] a[n+l], ea(l) = sum a[n+l]^2, eb = sum b[n]^2 over the region"""
    check_region(a.shape[0], b.shape[0], s0, s1, max_lag)
    bb = b[s0:s1].astype(dtype)
    win = np.lib.stride_tricks.sliding_window_view(a[s0 - max_lag:s1 + max_lag].astype(dtype), s1 - s0)     # row i: lag i - M
    r = np.array([np.sum(row * bb, dtype=dtype) for row in win], dtype=dtype)
    ea = np.array([np.sum(row * row, dtype=dtype) for row in win], dtype=dtype)
    return np.arange(-max_lag, max_lag + 1), r, ea, np.sum(bb * bb, dtype=dtype)


def rho_of(r, ea, eb):
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = r / np.sqrt(ea * eb)
    return np.where((ea == 0) | (eb == 0), np.zeros_like(rho), rho)


def pick_lag(lags, rho):
    """the l of largest rho; among equal rho the smallest |l|, then the negative one -> (l, rho(l), index)"""
    order = np.lexsort((lags, np.abs(lags), -rho))
    i = int(order[0])
    return int(lags[i]), rho[i], i


def search(a, b, s0, s1, max_lag):
    """float64 lag search of one row pair -> (lag, rho at it, the margin of the best rho over the best rho at any other lag)"""
    lags, r, ea, eb = correlations(a, b, s0, s1, max_lag)
    rho = rho_of(r, ea, eb)
    lag, best, i = pick_lag(lags, rho)
    rest = np.delete(rho, i)
    return lag, float(best), float(best - rest.max()) if rest.size else math.inf


def _ratio_db(num, den, dtype):
    if den == 0:
        return dtype(math.inf)
    if num == 0:
        return dtype(-math.inf)
    return dtype(10.0) * np.log10(num / den)


def frames(x, w, hop, dtype):
    """the frames lying wholly inside x, windowed, zero-padded to 1024 -> |rfft| [F, 513] in dtype"""
    win = hann(w).astype(dtype)
    fr = np.lib.stride_tricks.sliding_window_view(x, w)[::hop] * win
    assert fr.shape[0] == (x.shape[0] - w) // hop + 1
    pad = np.zeros((fr.shape[0], N_FFT), dtype=dtype)
    pad[:, :w] = fr
    spec = np.fft.rfft(pad, axis=1)
    assert spec.dtype == (np.complex128 if dtype == np.float64 else np.complex64)
    return np.abs(spec)


def _sum(x, dtype):
    """the sum of x in dtype: exactly rounded in float64, numpy's pairwise sum in float32"""
    return np.float64(math.fsum(x)) if dtype == np.float64 else np.sum(x, dtype=dtype)


def formula_mel32(x):
    """Audio2Mel's formula in float32 on one host row -> f32[80, F]: the stand-in for the project's module where there is no device"""
    return AR.audio2mel(torch.from_numpy(np.ascontiguousarray(x))[None], torch.float32, _bank())[0].numpy()


def measures(a, b, s0, s1, lag, dtype=np.float64, mel=True, mel_fn=None):
    """every number audio.compare reports for one row pair at a given lag, in `dtype` -> dict (sc, logmag: arrays of 3);
    mel_fn: one host row f32[n] -> its fp32 log-mel [80, F] (None: formula_mel32)"""
    check_region(a.shape[0], b.shape[0], s0, s1, abs(lag))
    aa, bb = a[s0 + lag:s1 + lag].astype(dtype), b[s0:s1].astype(dtype)
    r, ea, eb = _sum(bb * aa, dtype), _sum(aa * aa, dtype), _sum(bb * bb, dtype)
    out = {"rho": rho_of(np.asarray(r), np.asarray(ea), np.asarray(eb))[()]}
    alpha = r / ea if ea != 0 else dtype(0)
    res, dif = bb - alpha * aa, bb - aa
    ea_p = np.sum(aa * aa, dtype=dtype)                  # the ratios divide sums taken in one order: b = 0 gives 0 dB exactly
    out["si_sdr_db"] = _ratio_db(alpha * alpha * ea_p, np.sum(res * res, dtype=dtype), dtype)
    out["snr_db"] = _ratio_db(ea_p, np.sum(dif * dif, dtype=dtype), dtype)
    sc, lm = [], []
    for w, hop in RESOLUTIONS:
        A, B = frames(aa, w, hop, dtype), frames(bb, w, hop, dtype)
        d = A - B
        num, den = np.sum(d * d, dtype=dtype), np.sum(A * A, dtype=dtype)
        sc.append(dtype(0) if num == 0 else (dtype(math.inf) if den == 0 else np.sqrt(num) / np.sqrt(den)))
        fl = dtype(FLOOR)
        lm.append(np.mean(np.abs(np.log(np.maximum(A, fl)) - np.log(np.maximum(B, fl))), dtype=dtype))
    out["sc"], out["logmag"] = np.array(sc, dtype=dtype), np.array(lm, dtype=dtype)
    if mel:
        fn = formula_mel32 if mel_fn is None else mel_fn
        ma, mb = fn(np.ascontiguousarray(a[s0 + lag:s1 + lag])), fn(np.ascontiguousarray(b[s0:s1]))
        assert ma.dtype == mb.dtype == np.float32 and ma.shape == mb.shape and ma.shape[0] == 80
        out["mel_l1"] = np.mean(np.abs(ma.astype(dtype) - mb.astype(dtype)), dtype=dtype)
    return out


_BANK = []


def _bank():
    if not _BANK:
        _BANK.append(AR.slaney_bank64())
    return _BANK[0]


def distance(x, ref):
    """|x - ref| element-wise as float64, for values that may be infinite: 0 where both are the same infinity, inf where one is
    infinite and the other is not (or the other infinity) -> the largest"""
    x, ref = np.atleast_1d(np.asarray(x, dtype=np.float64)), np.atleast_1d(np.asarray(ref, dtype=np.float64))
    assert not np.isnan(ref).any()
    out = np.empty(ref.shape)
    for i, (u, v) in enumerate(zip(x, ref)):
        out[i] = 0.0 if u == v else (math.inf if (math.isinf(u) or math.isinf(v) or math.isnan(u)) else abs(u - v))
    return float(out.max())
