"""Time of ds_conv3x3_c1 (Encoder.conv_in: one input channel -> 128, with the GroupNorm partial sums of its output) on one GPU.

    python tools/conv_in_timing.py [--label NAME] [--out profiles/NAME.json]

20 mels of 80 x 848 (the encoder's batch), 128 output channels, with and without the statistics.  Milliseconds: median
(min .. max) of 100 calls after 20 untimed ones, a device event pair around each call.  The library is the one
text_to_sound_synthesis_amd/_lib.py loads (DIFFSOUND_LIB selects another build for an A/B of two of them: run the parent's
build twice to learn the run-to-run spread, then the new one).  The floor is the 434 MB store of the output at the 6.3 TB/s
a streaming kernel reaches on this part.  Prints one JSON line; asserts nothing about the times."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from text_to_sound_synthesis_amd import _lib, synth                    # noqa: E402

B, H, W, C = 20, 80, 848, 128
WARMUP, ITERS = 20, 100
HBM_ACHIEVABLE = 6.3e12


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ITERS)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "conv_in_timing.py measures on the GPU: there is no other path"
    torch.set_grad_enabled(False)
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream()
    x = (synth.synth_uniform((B, H, W), key="conv_in_time.x") * 2 - 1).cuda()
    w = ((synth.synth_uniform((C, 9), key="conv_in_time.w") * 2 - 1) / 3).cuda()
    bias = ((synth.synth_uniform((C,), key="conv_in_time.b") * 2 - 1) / 3).cuda()
    out = torch.empty(B, H, W, C, device="cuda")
    part = torch.empty(B, L.ds_conv3x3_c1_chunks(H, W), 2, C, dtype=torch.float64, device="cuda")
    res = {"label": a.label, "device": torch.cuda.get_device_name(0), "shape": [B, H, W, C], "warmup": WARMUP, "iters": ITERS,
           "with_statistics": timed(lambda: _lib.check(L.ds_conv3x3_c1(p(x), p(w), p(bias), p(out), B, H, W, C, p(part), st))),
           "without_statistics": timed(lambda: _lib.check(L.ds_conv3x3_c1(p(x), p(w), p(bias), p(out), B, H, W, C, None, st))),
           "store_floor_ms": round(out.numel() * 4 / HBM_ACHIEVABLE * 1e3, 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
