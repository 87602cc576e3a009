"""Seeded inputs of the tests of audio.align / audio.compare (tests/test_compare_host.py, tests/test_hip_compare.py): pairs
(a, b) of float32 numpy rows -- a the reference, b the one under test, a lag l pairing b[n] with a[n + l]."""
import functools
import math

import numpy as np

import audio_reference as AR

FS = 22050
N = 8999                        # samples of a values pair: the default region spans two tiles of 8192, the second ending on 3 odd samples


def noise(n, seed, amp=0.3):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def shifted(a, lag, n_b, seed=None, snr_db=None):
    """b[n] = a[n + lag] where a has that sample, fresh noise elsewhere; with snr_db, plus independent noise that far below a"""
    n = np.arange(n_b) + lag
    ok = (n >= 0) & (n < a.shape[0])
    b = noise(n_b, 7 if seed is None else seed + 1000)
    b[ok] = a[n[ok]]
    if snr_db is not None:
        rms = math.sqrt(float(np.mean(a.astype(np.float64) ** 2)))
        b = (b + noise(n_b, seed + 2000, rms * 10.0 ** (-snr_db / 20.0))).astype(np.float32)
    return b


def periodic(n, period=50, seed=5):
    """an integer-valued signal (samples in {-3..3}) of exact period: every product and sum over it is exact in float64"""
    p = np.random.default_rng(seed).integers(-3, 4, period)
    assert np.abs(p).max() > 0
    return np.tile(p, n // period + 1)[:n].astype(np.float32)


@functools.lru_cache(maxsize=None)
def value_pairs():
    """name -> (a, b), both f32[N]: the pairs whose every reported number is held to 4 x d32"""
    a = noise(N, 11)
    t = np.arange(N, dtype=np.float64) / FS
    chirp = AR.make_inputs(n=N)["chirp"].numpy()
    quiet = noise(N, 12, 1e-3)
    out = {
        "gain_0.5": (a, (np.float32(0.5) * a).astype(np.float32)),
        "gain_1.001": (a, (np.float32(1.001) * a).astype(np.float32)),
        "noise_1e-3": (a, (a + noise(N, 13, 1e-3)).astype(np.float32)),
        "noise_1e-2": (a, (a + noise(N, 14, 1e-2)).astype(np.float32)),
        "noise_0.1": (a, (a + noise(N, 15, 0.1)).astype(np.float32)),
        "tone_440_441": ((0.5 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32),
                         (0.5 * np.sin(2 * np.pi * 441.0 * t)).astype(np.float32)),
        "chirp_0.9": (chirp, (np.float32(0.9) * chirp).astype(np.float32)),
        "quiet_1e-3": (quiet, (quiet + noise(N, 16, 1e-4)).astype(np.float32)),
    }
    return out


# (max_lag, region length or None = the default region) the value pairs cycle through; the region starts at max_lag
VALUE_CONFIGS = ((0, None), (1, 1024), (64, 1025), (300, 1087), (0, 1088), (64, 4096), (1, None), (300, 4096))
REGION_LENGTHS = (1024, 1025, 1087, 1088, 4096)
MAX_LAGS = (0, 1, 64, 300)


# ---- the C entries' argument lists (good values on fake addresses) and what each must refuse ---------------------------------
FAKE = 4096                                                          # a non-null address that is never dereferenced
ENTRIES = {
    "ds_compare_align": (["a", "b", "B", "Na", "Nb", "s0", "s1", "max_lag", "lag_dev", "lag", "scratch", "bytes", "lag_out", "rho",
                          "sums", "stream"],
                         [FAKE, FAKE, 2, 9000, 8000, 300, 7700, 300, None, 0, FAKE, 1 << 30, FAKE, FAKE, FAKE, None]),
    "ds_compare_residual": (["a", "b", "B", "Na", "Nb", "s0", "s1", "max_lag", "lag", "sums", "scratch", "bytes", "stream"],
                            [FAKE, FAKE, 2, 9000, 8000, 300, 7700, 300, FAKE, FAKE, FAKE, 1 << 30, None]),
    "ds_compare_stft": (["a", "b", "B", "Na", "Nb", "s0", "s1", "max_lag", "lag", "windows", "twiddle", "scratch", "bytes",
                         "stream"],
                        [FAKE, FAKE, 2, 9000, 8000, 300, 7700, 300, FAKE, FAKE, FAKE, FAKE, 1 << 30, None]),
    "ds_compare_finish": (["B", "s0", "s1", "max_lag", "sums", "scratch", "bytes", "si_sdr_db", "snr_db", "sc", "logmag", "stream"],
                          [2, 300, 7700, 300, FAKE, FAKE, 1 << 30, FAKE, FAKE, FAKE, FAKE, None]),
}
REGION_BADS = [("max_lag", -1), ("max_lag", 4097), ("s0", 299), ("s1", 8701), ("s1", 8001), ("Na", 7999), ("s0", -1), ("s1", 300),
               ("s1", 200), ("B", 0), ("Na", 0), ("Nb", 0), ("bytes", 64), ("scratch", None), ("scratch", 4100)]


def bad_arguments(name):
    """the (argument, value) replacements entry `name` must refuse with -1 -> list; shared with the GPU test, which makes the
    same calls on real buffers and checks that nothing was written"""
    names = ENTRIES[name][0]
    bads = [(n, None) for n in names if n not in ("lag_dev", "stream") and isinstance(ENTRIES[name][1][names.index(n)], int)
            and ENTRIES[name][1][names.index(n)] == FAKE]
    # (ds_compare_finish is given neither row length: what it can check of the region is its order and its 1024 samples)
    bads += [(n, v) for n, v in REGION_BADS if n in names and not (name == "ds_compare_finish" and (n, v) in (("s1", 8701), ("s1", 8001), ("s0", 299)))]
    if name == "ds_compare_align":
        bads += [("lag", 5), ("lag_dev", FAKE)]                      # a given lag goes with max_lag == 0
    if name in ("ds_compare_stft", "ds_compare_finish"):
        bads += [("s1", 300 + 1023)]                                  # a region under 1024 samples
    return bads
