"""The codec's audio front end: waveform -> the mel image the VQ encoder consumes, in one HIP launch (ds_wave_to_mel).

Replaces the reference's offline feature extraction and the dataset's last steps:
  Diffsound/vocoder/mel2wav/extract_mel_spectrogram.py:141-151   TRANSFORMS: |STFT| (n_fft 1024, hop 256, centred frames) ->
                                                                 80 Slaney mels 125..7600 Hz at 22 050 Hz -> max(., 1e-5) ->
                                                                 log10 -> * 20 - 20 + 100 -> / 100 -> clip [0, 1] -> 860 frames
  :166-173, :195                                                 the wave zero-extended or cut to 220 500 samples
  sound_synthesis/data/caps_dataset.py:22-23,34,62               crop to 848 frames (centre crop for validation), 2 x - 1
The constants below are those settings; the crop and both affine maps are kernel arguments, not extra passes."""
import os

import numpy as np
import torch
from torch import nn

from .. import audio

SAMPLE_RATE = 22050
CLIP_SAMPLES = 220500          # 10 s
N_MELS, FMIN, FMAX = 80, 125.0, 7600.0
PAD = audio.N_FFT // 2         # centred frames (librosa.stft's center=True, reflect)
SPEC_FRAMES = 860              # TrimSpec(860) of the 862 frames
CROP_FRAMES = 848              # spec_crop_len
LOG_A, LOG_C = 0.2, 0.8        # (20 log10(m) - 20 + 100) / 100
FLOOR = 1e-5


class WaveToMel(nn.Module):
    """spec01(wave f32[B, T]) -> f32[B, 80, 860] in [0, 1]: what the reference stores as `*_mel.npy`.
    forward(wave, crop="center" | int) -> f32[B, 1, 80, 848] in [-1, 1]: the dataset item ('image') -- frames
    [crop, crop + 848), "center" = 6 (the validation crop).  wave is a device tensor at 22 050 Hz; any T (zero-extended or
    cut to 220 500 samples).  Host tensors raise: there is no CPU path."""

    def __init__(self):
        super().__init__()
        self.register_buffer("mel_basis", audio.mel_filterbank(SAMPLE_RATE, audio.N_FFT, N_MELS, FMIN, FMAX), persistent=False)
        self.register_buffer("window", audio.hann_window(), persistent=False)
        self.register_buffer("krange", audio.row_ranges(self.mel_basis), persistent=False)

    def spec01(self, wave):
        return audio.wave_to_mel(wave, self.window, self.mel_basis, self.krange, pad=PAD, length=CLIP_SAMPLES, f0=0,
                                 n_out=SPEC_FRAMES, a=LOG_A, c=LOG_C, lo=0.0, hi=1.0, floor=FLOOR)

    def forward(self, wave, crop="center"):
        f0 = (SPEC_FRAMES - CROP_FRAMES) // 2 if crop == "center" else int(crop)
        if not 0 <= f0 <= SPEC_FRAMES - CROP_FRAMES:
            raise ValueError("crop must be 'center' or a first frame in 0..%d" % (SPEC_FRAMES - CROP_FRAMES))
        # 2 * clip(a log10 m + c, 0, 1) - 1 = clip(2 a log10 m + 2 c - 1, -1, 1)
        out = audio.wave_to_mel(wave, self.window, self.mel_basis, self.krange, pad=PAD, length=CLIP_SAMPLES, f0=f0,
                                n_out=CROP_FRAMES, a=2 * LOG_A, c=2 * LOG_C - 1.0, lo=-1.0, hi=1.0, floor=FLOOR)
        return out[:, None]


_FRONT_ENDS = {}


def _front_end(device):
    key = (device.type, device.index)
    if key not in _FRONT_ENDS:
        _FRONT_ENDS[key] = WaveToMel().to(device)
    return _FRONT_ENDS[key]


def _clip_rates(rate, n):
    """`rate` (None, one rate, or one per clip) -> a list of n entries (None = not stated)"""
    if rate is None or isinstance(rate, (int, float, np.number)):
        if rate is not None and (isinstance(rate, bool) or not isinstance(rate, (int, np.integer)) or rate < 1):
            raise ValueError("sample rates must be positive integers, got %r" % (rate,))
        return [rate] * n
    if torch.is_tensor(rate):
        rate = rate.tolist()
    rate = list(rate)
    if len(rate) != n:
        raise ValueError("%d sample rates for %d clips" % (len(rate), n))
    return rate


def mel_image_from_audio(item, device, crop="center", rate=None):
    """batch['audio'] -> the content image f32[B, 1, 80, 848] on `device`: the one helper behind every entry point that
    accepts audio (DALLE.prepare_content / sample, modeling.train.training_prologue and so the solvers,
    pipeline.Diffsound.generate_sample_from_audio).  `item`: f32[B, T] (or [T]) already on the device, or a list of
    `.wav` paths / host arrays / host tensors -- read, zero-extended or cut to 220 500 samples on the host and copied once.
    `rate` (batch['audio_rate']): the sample rate of a tensor / of all host arrays, or a list, one per clip; None = 22 050 Hz
    for tensors and arrays, the header's rate for paths.  Clips at another rate than 22 050 Hz are resampled on the device
    (audio.resample: one copy and one ds_resample launch per distinct rate, written into the [B, 220 500] buffer)."""
    device = torch.device(device)
    if torch.is_tensor(item) and item.is_cuda:
        wave = item[None] if item.dim() == 1 else item
        rates = _clip_rates(rate, wave.shape[0])
        if any(r not in (None, SAMPLE_RATE) for r in rates):
            rates = [SAMPLE_RATE if r is None else r for r in rates]
            if len(set(rates)) == 1:          # one rate for the batch: the launch writes the buffer WaveToMel consumes
                wave = audio.resample(wave, rates[0], SAMPLE_RATE, n_out=CLIP_SAMPLES)
            else:
                buf = torch.empty(wave.shape[0], CLIP_SAMPLES, device=wave.device)
                for r in sorted(set(rates)):
                    rows = [i for i, q in enumerate(rates) if q == r]
                    buf[rows] = audio.resample(wave[rows], r, SAMPLE_RATE, n_out=CLIP_SAMPLES)
                wave = buf
        return _front_end(wave.device)(wave, crop=crop)
    clips = [item] if isinstance(item, (str, os.PathLike)) or (torch.is_tensor(item) and item.dim() == 1) else list(item)
    rates = _clip_rates(rate, len(clips))
    waves = []
    for i, clip in enumerate(clips):
        if isinstance(clip, (str, os.PathLike)):
            x, sr = audio.read_wav(clip)
            if rates[i] is not None and rates[i] != sr:
                raise ValueError("%s: sample rate %d in the header, %d stated" % (clip, sr, rates[i]))
            rates[i] = sr
        else:
            x = torch.as_tensor(clip).float().reshape(-1)
            rates[i] = SAMPLE_RATE if rates[i] is None else rates[i]
        waves.append(x)
    front = _front_end(device)
    if all(r == SAMPLE_RATE for r in rates):
        host = torch.zeros(len(clips), CLIP_SAMPLES)
        for i, x in enumerate(waves):
            n = min(x.numel(), CLIP_SAMPLES)
            host[i, :n] = x[:n]
        return front(host.to(device), crop=crop)
    buf = torch.empty(len(clips), CLIP_SAMPLES, device=device)
    for r in sorted(set(rates)):
        rows = [i for i, q in enumerate(rates) if q == r]
        need = -(-CLIP_SAMPLES * r // SAMPLE_RATE) + audio.resample_half_width(r, SAMPLE_RATE) + 1    # what the last output reaches
        lens = [min(waves[i].numel(), need) for i in rows]
        host = torch.zeros(len(rows), max(max(lens), 1))
        for k, i in enumerate(rows):
            host[k, :lens[k]] = waves[i][:lens[k]]
        part = audio.resample(host.to(device), r, SAMPLE_RATE, lengths=lens, n_out=CLIP_SAMPLES)
        if len(rows) == len(clips):
            buf = part
        else:
            buf[rows] = part
    return front(buf, crop=crop)
