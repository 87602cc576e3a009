"""Time the one-call Philox sampling chain (19 layers, T = 100, top-r 0.85, synthetic weights), unguided or guided.

    python tools/guidance_time.py --batch 64 --scale 3        guided: one forward at batch 128 per step
    python tools/guidance_time.py --batch 128                 unguided (runs on a tree without guidance too)

Prints one JSON line: clips/s over --repeats timed chains after --warmup untimed ones (hipEvent timing around each chain,
median and min..max), so that the guided chain at batch B can be set beside the unguided chain at 2B and at B."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from text_to_sound_synthesis_amd import synth                                  # noqa: E402
from text_to_sound_synthesis_amd.config import build_model, default_config     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--scale", type=float, default=None, help="guidance scale; omitted: the unguided chain")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    m = build_model(default_config(n_layer=19, diffusion_step=100))
    synth.synth_init_(m, seed=0)
    dt = m.cuda().eval().transformer
    dt.truncation_r = 0.85
    B = a.batch
    cond = synth.synth_cond_emb(B, key="time.cond").cuda()
    ids = torch.arange(B, device="cuda")
    kw = dict(condition_token=None, condition_mask=None, condition_embed=cond, filter_ratio=0, caption_ids=ids, seed=1)
    if a.scale is not None:
        kw.update(guidance_scale=a.scale, null_condition_embed=synth.synth_cond_emb(1, key="time.null")[0].cuda())
    secs = []
    for i in range(a.warmup + a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dt.sample(**kw)
        e1.record()
        e1.synchronize()
        if i >= a.warmup:
            secs.append(e0.elapsed_time(e1) / 1e3)
    secs.sort()
    rate = [B / s for s in secs]
    print(json.dumps({"batch": B, "guidance_scale": a.scale, "repeats": a.repeats, "clips_per_s_median": round(B / secs[len(secs) // 2], 3),
                      "clips_per_s_min": round(min(rate), 3), "clips_per_s_max": round(max(rate), 3),
                      "seconds_per_chain_median": round(secs[len(secs) // 2], 4)}))


if __name__ == "__main__":
    main()
