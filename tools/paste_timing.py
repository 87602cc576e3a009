"""Time of pasting a recording back on one GPU: ds_paste_sums and ds_paste alone, and the whole of audio.paste(match_gain=True),
beside the vocoder pass that produces the same batch, in one run.

    python tools/paste_timing.py [--iters 30] [--out profiles/NAME.json]

The batch is the one the drivers return: 64 x 217 088 samples at 22 050 Hz, 53 columns of 4096 samples, recording offset 1408
(so the recording is read off the 16-byte grid), cross-fade 1024 samples.  Masks:
  inpaint   columns 21..37 regenerated (4 s .. 7 s): 36 of 53 columns kept
  all       every column kept: the paste is a copy of the recording, the sums run over every position
  none      nothing kept: the paste is the rendering (times the gain), the sums have nothing to add
and the mel paste of the same batch (f32[64, 80, 848], 16 frames a column, fade 4, linear) under the inpaint mask.
Milliseconds: median (min .. max) of --iters calls after 5 untimed ones, a device event pair around each call.  The traffic
floor is 12 bytes a position for the paste (rendering and recording read, result written) and 8 for the sums, at the 6.3 TB/s
a streaming kernel reaches on this part; the kernels skip the operand a group of four positions does not need, so a call can
move less than that.  Prints one JSON line; asserts nothing about the times."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from text_to_sound_synthesis_amd import _lib, audio, synth                    # noqa: E402
from text_to_sound_synthesis_amd.modeling.vocoder import Generator            # noqa: E402

RATE = 22050
HBM_ACHIEVABLE = 6.3e12
B, T, N_COLS, OFF, FADE = 64, 217088, 53, 1408, 1024.0
MASKS = {"inpaint": [0 if 21 <= c <= 37 else 1 for c in range(N_COLS)], "all": [1] * N_COLS, "none": [0] * N_COLS}


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "paste_timing.py measures on the GPU: there is no other path"
    torch.set_grad_enabled(False)
    voc = Generator(80, 32, 3)
    synth.synth_init_(voc, seed=0)
    voc = voc.cuda().eval()
    g = torch.Generator().manual_seed(0)
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream()
    ren = (0.1 * torch.randn(B, T, generator=g)).cuda()
    rec = (0.1 * torch.randn(B, 220500, generator=g)).cuda()
    out = torch.empty_like(ren)
    off = torch.full((B,), OFF, dtype=torch.int64).cuda()
    nbytes = int(L.ds_paste_scratch_bytes(B, T))
    scratch = torch.empty(nbytes // 8, dtype=torch.float64).cuda()
    sums = torch.empty(B, 2, dtype=torch.float64).cuda()
    res = {"device": torch.cuda.get_device_name(0), "rate": RATE, "iters": a.iters, "rows": B, "samples": T,
           "megabytes": round(B * T * 4 / 1e6, 2), "cases": {}}
    for name, mask in MASKS.items():
        keep = torch.tensor([mask] * B, dtype=torch.uint8).cuda()
        case = {"kept_columns": sum(mask)}
        case["ds_paste_sums"] = timed(lambda: _lib.check(L.ds_paste_sums(p(ren), p(rec), B, T, rec.shape[1], p(off), None, p(keep),
                                                                         N_COLS, 4096, 1, p(scratch), nbytes, p(sums), st)), a.iters)
        case["ds_paste"] = timed(lambda: _lib.check(L.ds_paste(p(ren), p(rec), p(out), B, 1, T, rec.shape[1], p(off), None, p(keep),
                                                               N_COLS, 4096, 1, FADE, _lib.PASTE_EQUAL_POWER, p(sums), st)), a.iters)
        case["paste_match_gain"] = timed(lambda: audio.paste(ren, rec, keep, off=off, col_num=4096, fade_len=FADE, match_gain=True),
                                         a.iters)
        res["cases"][name] = case
    res["traffic_floor_ms"] = {"ds_paste": round(12 * B * T / HBM_ACHIEVABLE * 1e3, 4),
                               "ds_paste_sums": round(8 * B * T / HBM_ACHIEVABLE * 1e3, 4)}
    mel = synth.synth_uniform((B, 80, T // 256), key="paste_time.mel").cuda() * 2 - 1
    image = synth.synth_uniform((B, 80, T // 256), key="paste_time.image").cuda() * 2 - 1
    keep = torch.tensor([MASKS["inpaint"]] * B, dtype=torch.uint8).cuda()
    res["mel_paste"] = timed(lambda: audio.paste(mel, image, keep, col_num=16, fade_len=4.0, curve="linear"), a.iters)
    res["mel_traffic_floor_ms"] = round(12 * mel.numel() / HBM_ACHIEVABLE * 1e3, 4)
    res["vocoder"] = timed(lambda: voc(mel, scale=0.5, shift=0.5), max(a.iters // 3, 3), warmup=2)
    res["paste_share_of_vocoder"] = round((res["cases"]["inpaint"]["paste_match_gain"]["median_ms"] + res["mel_paste"]["median_ms"])
                                          / res["vocoder"]["median_ms"], 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
