"""Time of the resampler at B = 64 x 10 s on one GPU, per ratio: (a) ds_resample (one launch, audio.resample), (b) the
stock-torch route on the same device -- one strided F.conv1d with the polyphase bank, the form torchaudio's resample runs:
channel c at stride position q reads x[q M + k - W], so row (c M) mod L of the [L, 2W+1] table sits at column floor(c M / L) of a
[L, 1, 2W + 1 + floor((L - 1) M / L)] kernel -- and (c) the traffic floor: bytes in + out over the HBM rate a streaming
kernel reaches on this part (6.3 TB/s).  Device events over `--iters` launches after warm-up, same process.

    python tools/resample_time.py [--batch 64] [--iters 30] [--out profiles/NAME.txt]"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_ACHIEVABLE = 6.3e12
RATIOS = [(48000, 22050), (44100, 22050), (16000, 22050), (22050, 48000)]


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
    return ms[len(ms) // 2], ms[0], ms[-1]


def conv_bank(taps, L, M, W):
    """channel c = n mod L of stride position q = n div L: i0 = q M + floor(c M / L), phase (c M) mod L"""
    shift = [(c * M) // L for c in range(L)]
    bank = torch.zeros(L, 1, 2 * W + 1 + shift[-1])
    for c in range(L):
        bank[c, 0, shift[c]:shift[c] + 2 * W + 1] = taps[(c * M) % L]
    return bank


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--no-stock", action="store_true", help="time ds_resample only (profiling runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from text_to_sound_synthesis_amd import audio
    torch.set_grad_enabled(False)
    B = args.batch
    g = torch.Generator().manual_seed(0)
    lines = ["device: %s   batch %d x %.0f s   %d timed launches each (median / min / max, device events)"
             % (torch.cuda.get_device_name(0), B, args.seconds, args.iters)]
    for src, dst in RATIOS:
        T = int(round(args.seconds * src))
        wave = (0.3 * torch.randn(B, T, generator=g)).cuda()
        taps, L, M, W = audio.resample_taps(src, dst)
        N = audio.resample_length(T, src, dst)
        floor_us = B * (T + N) * 4 / HBM_ACHIEVABLE * 1e6
        ours = audio.resample(wave, src, dst)
        med, lo, hi = timed(lambda: audio.resample(wave, src, dst), args.iters)
        lines.append("%d -> %d  (L %d, M %d, %d taps)  [%d,%d] -> [%d,%d]" % (src, dst, L, M, 2 * W + 1, B, T, B, N))
        lines.append("  (a) ds_resample            %9.1f us  (%.1f .. %.1f)   %.2f x the floor" % (med * 1e3, lo * 1e3, hi * 1e3, med * 1e3 / floor_us))
        if not args.no_stock:
            bank = conv_bank(taps, L, M, W).cuda()
            Q = (N + L - 1) // L
            need = (Q - 1) * M + bank.shape[-1]                      # padded samples the last stride position reads
            xp = F.pad(wave, (W, max(need - T - W, 0)))[:, None]     # the copy is made once, outside the timed region

            def stock():
                return F.conv1d(xp, bank, stride=M).transpose(1, 2).reshape(B, -1)[:, :N]
            try:
                diff = float((stock() - ours).abs().max())
                smed, slo, shi = timed(stock, args.iters)
                lines.append("  (b) stock torch F.conv1d   %9.1f us  (%.1f .. %.1f)   %.1f x (a); max |a - b| %.2e"
                             % (smed * 1e3, slo * 1e3, shi * 1e3, smed / med, diff))
            except Exception as e:      # the vendor library may have no kernel for such a shape: say so, keep timing (a)
                lines.append("  (b) stock torch F.conv1d   failed: %s" % str(e).splitlines()[0][:120])
            del bank, xp
        lines.append("  (c) traffic floor          %9.1f us  (%.1f MB at 6.3 TB/s)" % (floor_us, B * (T + N) * 4 / 1e6))
        del wave, ours
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
