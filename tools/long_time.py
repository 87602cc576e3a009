"""Time long-form generation (Diffsound.generate_long: 19 layers, T = 100, top-r 0.85, synthetic weights, random vocoder).

    python tools/long_time.py --batch 8 --seconds 24          W = 3 windows at the default overlap
    python tools/long_time.py --batch 8 --baseline             generate_sample_with_condition only (runs on an older tree too)

Prints one JSON line.  Per stage, milliseconds of the median of --repeats timed calls after --warmup untimed ones (hipEvent
pairs around the stage's calls inside generate_long): the W sampling chains, the one decode at batch B W, the mel stitch, the
vocoder; the whole call; generate_sample_with_condition at the same B (one grid: chain + decode + vocoder), to set the whole
call beside W of those.  Then ds_mel_stitch alone over --stitch-iters back-to-back launches, at the call's shape and at a
shape large enough to leave the caches (B = 64, W = 16): microseconds per launch and GB/s against the bytes it must move
(every window value read once, every output value written once)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from text_to_sound_synthesis_amd import pipeline, synth                        # noqa: E402
from text_to_sound_synthesis_amd.config import default_config                 # noqa: E402


class Stage:
    """wraps a callable: every call is bracketed by a hipEvent pair; ms() sums and clears them"""

    def __init__(self, fn):
        self.fn, self.events = fn, []

    def __call__(self, *a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = self.fn(*a, **k)
        e1.record()
        self.events.append((e0, e1))
        return out

    def ms(self):
        torch.cuda.synchronize()
        t = sum(a.elapsed_time(b) for a, b in self.events)
        self.events = []
        return t


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def stitch_alone(audio, B, W, iters):
    hop = (53 - 13) * 16
    win = torch.randn(B, W, 80, 848, device="cuda")
    audio.stitch_mel(win, hop)
    ms = timed(lambda: [audio.stitch_mel(win, hop) for _ in range(iters)]) / iters
    moved = 4 * (win.numel() + B * 80 * (848 + (W - 1) * hop))
    return {"B": B, "W": W, "us_per_launch": round(ms * 1e3, 2), "bytes": moved, "GB_per_s": round(moved / (ms * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=24.0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--stitch-iters", type=int, default=200)
    ap.add_argument("--baseline", action="store_true", help="only generate_sample_with_condition at --batch")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    ds = pipeline.Diffsound(config=default_config(n_layer=19, diffusion_step=100), random_vocoder=True)
    synth.synth_init_(ds.model, seed=0)
    synth.synth_init_(ds.vocoder, seed=0)
    B = a.batch
    cond = synth.synth_cond_emb(B, key="time.cond").cuda()
    ids = list(range(B))
    res = {"batch": B, "repeats": a.repeats}
    one = [timed(lambda: ds.generate_sample_with_condition(cond, caption_ids=ids, seed=1)) for _ in range(a.warmup + a.repeats)]
    res["one_grid_ms"] = round(median(one[a.warmup:]), 2)
    ds.model.truncation_forward = False
    if not a.baseline:
        from text_to_sound_synthesis_amd import audio
        W = pipeline.long_plan(a.seconds)[0]
        chains, decode = Stage(ds.model._run_chain), Stage(ds.model.decode_to_img)
        stitch, vocode = Stage(audio.stitch_mel), Stage(ds.vocoder.forward)
        ds.model._run_chain, ds.model.decode_to_img, ds.vocoder.forward = chains, decode, vocode
        real_stitch, audio.stitch_mel = audio.stitch_mel, stitch
        rows = []
        for i in range(a.warmup + a.repeats):
            whole = timed(lambda: ds.generate_long(cond, a.seconds, caption_ids=ids, seed=1))
            rows.append((whole, chains.ms(), decode.ms(), stitch.ms(), vocode.ms()))
        audio.stitch_mel = real_stitch
        rows = rows[a.warmup:]
        names = ("whole_ms", "chains_ms", "decode_ms", "stitch_ms", "vocoder_ms")
        res.update({"seconds": a.seconds, "windows": W})
        res.update({n: round(median([r[k] for r in rows]), 3) for k, n in enumerate(names)})
        res["whole_over_W_one_grid"] = round(res["whole_ms"] / (W * res["one_grid_ms"]), 3)
        res["stitch_alone"] = [stitch_alone(audio, B, W, a.stitch_iters), stitch_alone(audio, 64, 16, a.stitch_iters)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
