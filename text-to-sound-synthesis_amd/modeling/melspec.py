"""The codec's audio front end: waveform -> the mel image the VQ encoder consumes, in one HIP launch (ds_wave_to_mel).

Replaces the reference's offline feature extraction and the dataset's last steps:
  Diffsound/vocoder/mel2wav/extract_mel_spectrogram.py:141-151   TRANSFORMS: |STFT| (n_fft 1024, hop 256, centred frames) ->
                                                                 80 Slaney mels 125..7600 Hz at 22 050 Hz -> max(., 1e-5) ->
                                                                 log10 -> * 20 - 20 + 100 -> / 100 -> clip [0, 1] -> 860 frames
  :166-173, :195                                                 the wave zero-extended or cut to 220 500 samples
  sound_synthesis/data/caps_dataset.py:22-23,34,62               crop to 848 frames (centre crop for validation), 2 x - 1
The constants below are those settings; the crop and both affine maps are kernel arguments, not extra passes."""
import os

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


def mel_image_from_audio(item, device, crop="center"):
    """batch['audio'] -> the content image f32[B, 1, 80, 848] on `device`: the one helper behind every entry point that
    accepts audio (DALLE.prepare_content / sample, modeling.train.training_prologue and so the solvers,
    pipeline.Diffsound.generate_sample_from_audio).  `item`: f32[B, T] (or [T]) already on the device, or a list of
    `.wav` paths / host arrays / host tensors -- read, zero-extended or cut to 220 500 samples on the host and copied once."""
    device = torch.device(device)
    if torch.is_tensor(item) and item.is_cuda:
        wave = item[None] if item.dim() == 1 else item
    else:
        clips = [item] if isinstance(item, (str, os.PathLike)) or (torch.is_tensor(item) and item.dim() == 1) else list(item)
        host = torch.zeros(len(clips), CLIP_SAMPLES)
        for i, clip in enumerate(clips):
            x = audio.read_wav(clip, rate=SAMPLE_RATE)[0] if isinstance(clip, (str, os.PathLike)) else torch.as_tensor(clip).float().reshape(-1)
            n = min(x.numel(), CLIP_SAMPLES)
            host[i, :n] = x[:n]
        wave = host.to(device)
    key = (wave.device.type, wave.device.index)
    if key not in _FRONT_ENDS:
        _FRONT_ENDS[key] = WaveToMel().to(wave.device)
    return _FRONT_ENDS[key](wave, crop=crop)
