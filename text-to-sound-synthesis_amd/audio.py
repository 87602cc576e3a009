"""Host side of the audio front end: the mel filterbank, the FFT tables of `ds_wave_to_mel`, a RIFF reader, and the thin
launcher of the kernel (csrc/stft_mel.hip) that `modeling.vocoder.Audio2Mel` and `modeling.melspec.WaveToMel` share.

The reference extracts mels with librosa on the host (Diffsound/vocoder/mel2wav/extract_mel_spectrogram.py:15-38,141-187)
and reads audio with `librosa.load(path, sr=None)` (:167).  Nothing here needs librosa or soundfile."""
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
