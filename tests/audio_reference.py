"""The yardstick of the audio front end's tests: the transform's formula with stock torch on the CPU, in float64 (the
reference value) and in float32 (the arithmetic class of the reference's own code: librosa 0.8 works in complex64,
Audio2Mel in fp32), with a Slaney filterbank built here -- independently of text_to_sound_synthesis_amd/audio.py -- and
the test inputs.  Never the code under test."""
import math

import torch
import torch.nn.functional as F

SR = 22050
CLIP = 220500


def slaney_bank64(sr=SR, n_fft=1024, n_mels=80, fmin=0.0, fmax=None):
    """float64 [n_mels, n_fft / 2 + 1], element by element from the published definition: mel = f / (200 / 3) below 1 kHz,
    15 + ln(f / 1000) / (ln(6.4) / 27) above; n_mels + 2 corner frequencies equally spaced in mel; triangle j rises over
    [f_j, f_j+1], falls over [f_j+1, f_j+2] and is scaled by 2 / (f_j+2 - f_j)."""
    fmax = sr / 2.0 if fmax is None else fmax
    step = math.log(6.4) / 27.0

    def h2m(f):
        return f / (200.0 / 3.0) if f < 1000.0 else 15.0 + math.log(f / 1000.0) / step

    def m2h(m):
        return m * (200.0 / 3.0) if m < 15.0 else 1000.0 * math.exp((m - 15.0) * step)

    m0, m1 = h2m(fmin), h2m(fmax)
    pts = [m2h(m0 + (m1 - m0) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    W = torch.zeros(n_mels, n_fft // 2 + 1, dtype=torch.float64)
    for j in range(n_mels):
        for k in range(n_fft // 2 + 1):
            f = k * sr / n_fft
            up = (f - pts[j]) / (pts[j + 1] - pts[j])
            down = (pts[j + 2] - f) / (pts[j + 2] - pts[j + 1])
            W[j, k] = max(0.0, min(up, down)) * 2.0 / (pts[j + 2] - pts[j])
    return W


def mel_magnitudes(wave, basis64, pad, length, dtype):
    """wave [B, T] -> mel_basis |STFT| [B, n_mels, frames] in `dtype`: zero-extend / cut to `length` (0: as is), reflect-pad,
    periodic Hann, torch.stft(center=False, return_complex=True), abs, matmul."""
    x = wave.to(dtype)
    if length:
        y = torch.zeros(x.shape[0], length, dtype=dtype)
        n = min(length, x.shape[1])
        y[:, :n] = x[:, :n]
        x = y
    xp = F.pad(x[:, None], (pad, pad), mode="reflect")[:, 0]
    win = torch.hann_window(1024, periodic=True, dtype=torch.float64).to(dtype)
    S = torch.stft(xp, 1024, hop_length=256, win_length=1024, window=win, center=False, return_complex=True).abs()
    return torch.matmul(basis64.to(dtype), S)


def log_affine(m, a, c, lo, hi, floor=1e-5):
    y = a * torch.log10(torch.clamp(m, min=floor)) + c
    return torch.clamp(y, lo, hi)


def codec_spec01(wave, dtype, bank=None):
    """extract_mel_spectrogram.py's TRANSFORMS on a 220 500-sample clip: [B, 80, 860] in [0, 1]"""
    bank = slaney_bank64(fmin=125.0, fmax=7600.0) if bank is None else bank
    m = mel_magnitudes(wave, bank, 512, CLIP, dtype)
    assert m.shape[-1] == 862
    return log_affine(m, 0.2, 0.8, 0.0, 1.0)[..., :860]


def codec_image(wave, dtype, crop=6, bank=None):
    """... + the dataset's crop and 2 x - 1: [B, 1, 80, 848] in [-1, 1]"""
    return (2.0 * codec_spec01(wave, dtype, bank)[..., crop:crop + 848] - 1.0)[:, None]


def audio2mel(wave, dtype, bank=None):
    """vocoder/modules.py:54-69 on wave [B, T]: log10(clamp(mel_basis |STFT|, 1e-5)), pad 384"""
    bank = slaney_bank64() if bank is None else bank
    return log_affine(mel_magnitudes(wave, bank, 384, 0, dtype), 1.0, 0.0, -math.inf, math.inf)


def make_inputs(n=CLIP, seed=0):
    """name -> f32[n]; the first two are the broadband ones"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / SR
    noise = torch.randn(n, generator=g)
    gate = ((torch.arange(n) // (SR // 4)) % 3 == 0).float()                   # 0.25 s of noise, 0.5 s of exact zeros
    dur = n / SR
    chirp = 0.8 * torch.sin(2 * math.pi * (100.0 * t + 0.5 * (7100.0 - 100.0) / dur * t * t))
    return {
        "noise_0.3": 0.3 * noise,
        "noise_1e-3": 1e-3 * torch.randn(n, generator=g),
        "bursts": 0.3 * torch.randn(n, generator=g) * gate,
        "chirp": chirp.float(),
        "tone_440": (0.9 * torch.sin(2 * math.pi * 440.0 * t)).float(),
        "silence": torch.zeros(n),
    }


BROADBAND = ("noise_0.3", "noise_1e-3")
