"""Time of audio.compare on one GPU: every ds_compare_* entry alone and the whole call, beside the vocoder pass that produces the
same batch, in one run.

    python tools/audio_compare_timing.py [--iters 20] [--max-lag 2048] [--out profiles/NAME.json]

Case: 64 x 217 088 samples at 22 050 Hz (the batch the drivers return; a = noise at 0.1, b = a moved by 37 samples plus noise
at -20 dB), the lag searched over +- max_lag on the default region.  Milliseconds: median (min .. max) of --iters calls after 3
untimed ones, a device event pair around each call.  ds_compare_align is its three kernels together (the partial sums; one wave
per row that adds them and picks the lag; the double-double sums at that lag).  Beside the times, two floors of the lag search:
  fma      B n (2 max_lag + 1) float64 fma for r and as many for ea, at 64 fma per clock and CU (v_fma_f64 at the fp32 rate: 16
           lanes per clock and SIMD) x the device's CU count and its clock as the runtime reports it (where it reports none:
           the part's nominal 2 400 MHz, and the record says so)
  traffic  the two inputs read once and the partial sums written once, at the 6.3 TB/s a streaming kernel reaches on this part
Prints one JSON line; asserts nothing about the times."""
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
NOMINAL_CLOCK_HZ = 2.4e9
B, T = 64, 217088


def timed(fn, iters, warmup=3):
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


def entries(a, b, M):
    """the entries on buffers made once -> (name -> callable, scratch bytes, region)"""
    L = _lib.lib()
    dev = a.device
    s0, s1 = audio.compare_region(a.shape[1], b.shape[1], M)
    nbytes = int(L.ds_compare_scratch_bytes(B, s1 - s0, M))
    scratch = torch.empty(nbytes // 8 + 1, device=dev, dtype=torch.float64)
    lag = torch.empty(B, device=dev, dtype=torch.int32)
    rho, si, snr = (torch.empty(B, device=dev, dtype=torch.float64) for _ in range(3))
    sums, sc, lm = (torch.empty(B, 3, device=dev, dtype=torch.float64) for _ in range(3))
    win, tw = audio._compare_windows(dev), audio._twiddle(dev)
    p, st = _lib.ptr, _lib.stream()
    Na, Nb = a.shape[1], b.shape[1]
    fns = {
        "ds_compare_align": lambda: _lib.check(L.ds_compare_align(p(a), p(b), B, Na, Nb, s0, s1, M, None, 0, p(scratch), nbytes,
                                                                  p(lag), p(rho), p(sums), st)),
        "ds_compare_residual": lambda: _lib.check(L.ds_compare_residual(p(a), p(b), B, Na, Nb, s0, s1, M, p(lag), p(sums), p(scratch),
                                                                        nbytes, st)),
        "ds_compare_stft": lambda: _lib.check(L.ds_compare_stft(p(a), p(b), B, Na, Nb, s0, s1, M, p(lag), p(win), p(tw), p(scratch),
                                                                nbytes, st)),
        "ds_compare_finish": lambda: _lib.check(L.ds_compare_finish(B, s0, s1, M, p(sums), p(scratch), nbytes, p(si), p(snr), p(sc),
                                                                    p(lm), st)),
    }
    return fns, nbytes, (s0, s1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--max-lag", type=int, default=2048)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "audio_compare_timing.py measures on the GPU: there is no other path"
    torch.set_grad_enabled(False)
    M = args.max_lag
    g = torch.Generator().manual_seed(0)
    a = (0.1 * torch.randn(B, T, generator=g)).cuda()
    b = torch.roll(a, -37, 1) + (0.01 * torch.randn(B, T, generator=g)).cuda()          # b[n] = a[n + 37] + noise
    fns, nbytes, (s0, s1) = entries(a, b, M)
    prop = torch.cuda.get_device_properties(0)
    n = s1 - s0
    fma = 2.0 * B * n * (2 * M + 1)
    clock_hz = float(getattr(prop, "clock_rate", 0) or 0) * 1e3
    clock_source = "runtime" if clock_hz > 0 else "nominal"
    clock_hz = clock_hz if clock_hz > 0 else NOMINAL_CLOCK_HZ
    res = {"device": torch.cuda.get_device_name(0), "rate": RATE, "iters": args.iters, "rows": B, "samples": T, "max_lag": M,
           "region": [s0, s1], "scratch_megabytes": round(nbytes / 1e6, 2), "compute_units": prop.multi_processor_count,
           "clock_mhz": round(clock_hz / 1e6, 1), "clock_source": clock_source}
    for k, fn in fns.items():
        res[k] = timed(fn, args.iters)
    res["audio_compare"] = timed(lambda: audio.compare(a, b, max_lag=M), args.iters)
    out = audio.compare(a, b, max_lag=M)
    res["lags_found"] = sorted(set(out["lag"].tolist()))
    res["audio_compare_given_lag"] = timed(lambda: audio.compare(a, b, lag=out["lag"], region=(s0, s1)), args.iters)
    res["fma_count"] = fma
    res["fma_floor_ms"] = round(fma / (64.0 * prop.multi_processor_count * clock_hz) * 1e3, 4)
    res["traffic_floor_ms"] = round((2.0 * B * T * 4 + nbytes) / HBM_ACHIEVABLE * 1e3, 4)
    voc = Generator(80, 32, 3)
    synth.synth_init_(voc, seed=0)
    voc = voc.cuda().eval()
    mel = synth.synth_uniform((B, 80, T // 256), key="compare_time.mel").cuda()
    res["vocoder"] = timed(lambda: voc(mel, scale=0.5, shift=0.5), max(args.iters // 3, 3), warmup=2)
    res["compare_share_of_vocoder"] = round(res["audio_compare"]["median_ms"] / res["vocoder"]["median_ms"], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
