"""Time the caption-track chain against the guided chain (19 layers, T = 100, synthetic weights, B = 16).

    python tools/compose_timing.py [--out profiles/NAME.json]

All chains are one C call of 100 steps (top-r 0.85, per-caption in-kernel noise): the guided chain (ds_denoiser_sample_guided_rng,
forward at batch 2B) and the composed chain (ds_denoiser_sample_composed_rng, forward at batch (C+1)B) at C = 1, 2, 3 with
dense constant weights, alternating within a repeat.  Milliseconds of the median of --repeats timed calls after --warmup
untimed ones, a device event pair around each call; the guided chain's spread (max - min over its repeats) is reported with
it, since composed C = 1 against guided is the one comparison with an expectation (the same forward, the same tail
arithmetic).  The zero-weight skip is measured on the tail alone: ds_sample_tail_composed_rng at C = 3 on synthetic logits,
with dense weights against weights where exactly one track is live per position, and the C = 1 tail against the guided
tail on the same two rows.  Prints one JSON line; asserts nothing about the times."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from text_to_sound_synthesis_amd import _lib, synth                           # noqa: E402
from text_to_sound_synthesis_amd.config import build_model, default_config    # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--layers", type=int, default=19)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tail-repeats", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "compose_timing.py measures on the GPU: there is no other path"
    torch.set_grad_enabled(False)
    T, L, K, CMAX = 100, 265, 256, 3
    m = build_model(default_config(n_layer=a.layers, diffusion_step=T))
    synth.synth_init_(m, seed=0)
    m = m.cuda().eval()
    dt = m.transformer
    dt.truncation_r = 0.85
    B = a.batch
    conds = torch.stack([synth.synth_cond_emb(B, key="time.cond%d" % i) for i in range(CMAX)], 0).cuda()
    null = synth.synth_cond_emb(1, key="time.null")[0].cuda()
    ids = torch.arange(B, device="cuda")
    kw = dict(condition_token=None, condition_mask=None, caption_ids=ids, seed=1, filter_ratio=0, null_condition_embed=null)
    guided = lambda: dt.sample(condition_embed=conds[0], guidance_scale=3.0, **kw)["content_token"]
    composed = lambda C: dt.sample(condition_embed=None, track_embed=conds[:C].contiguous(),
                                   track_weight=torch.full((B, C, L), 3.0 / C, device="cuda"), **kw)["content_token"]
    times = {"guided": [], 1: [], 2: [], 3: []}
    same = None
    for i in range(a.warmup + a.repeats):
        ms, g = timed(guided)
        times["guided"].append(ms)
        for C in (1, 2, 3):
            ms, c = timed(lambda: composed(C))
            times[C].append(ms)
            if C == 1:                                            # one track of weight 3: the guided chain's tokens
                same = bool(torch.equal(c, g)) and same is not False
    res = {"batch": B, "layers": a.layers, "T": T, "repeats": a.repeats}
    gt = times["guided"][a.warmup:]
    res["guided_chain_ms"] = round(median(gt), 2)
    res["guided_chain_spread_ms"] = round(max(gt) - min(gt), 2)
    for C in (1, 2, 3):
        res["composed_c%d_chain_ms" % C] = round(median(times[C][a.warmup:]), 2)
        res["composed_c%d_over_guided" % C] = round(median(times[C][a.warmup:]) / median(gt), 4)
    res["composed_c1_weight3_tokens_equal_guided"] = same

    # ---- the tails alone (the tail entries take L rows per sample), on synthetic logits
    lib, sched = _lib.lib(), dt._schedule_table()
    C = CMAX
    x = synth.synth_tokens(B, mask_frac=0.5, key="time.xt").cuda()
    out = torch.empty_like(x)
    dense = torch.full((B, C, L), 1.0, device="cuda")
    sparse = torch.zeros(B, C, L, device="cuda")
    owner = (torch.arange(L, device="cuda") // 5 * C // 53).clamp(max=C - 1)                # a third of the columns per track
    sparse.scatter_(1, owner[None, None, :].expand(B, 1, L), 3.0)
    assert bool(((sparse != 0).sum(1) == 1).all())
    z = (torch.randn(C + 1, B * L, K, device="cuda") * 4).contiguous()
    t = torch.full((B,), 50, dtype=torch.long, device="cuda")

    one = torch.full((B, 1, L), 3.0, device="cuda")
    z1 = z[C - 1:]                                        # [2][B L][K]: one track and the null condition -- the guided tail's rows

    def tail(w, zz=z):
        return timed(lambda: _lib.check(lib.ds_sample_tail_composed_rng(
            _lib.ptr(zz), _lib.ptr(x), _lib.ptr(t), _lib.ptr(ids), 1, 0, _lib.ptr(sched), _lib.ptr(out), B, L, K, T, 0, 0.85, 0,
            w.shape[1], _lib.ptr(w), None, None, 0, _lib.stream())))[0]

    def tail_guided():
        return timed(lambda: _lib.check(lib.ds_sample_tail_guided_rng(
            _lib.ptr(z1[0]), _lib.ptr(z1[1]), _lib.ptr(x), _lib.ptr(t), _lib.ptr(ids), 1, 0, _lib.ptr(sched), _lib.ptr(out), B, L, K, T,
            0, 0.85, 0, 3.0, None, None, 0, _lib.stream())))[0]
    tail(dense), tail(sparse), tail(one, z1), tail_guided()
    td, ts, t1, tg = [], [], [], []
    for _ in range(a.tail_repeats):
        td.append(tail(dense))
        ts.append(tail(sparse))
        t1.append(tail(one, z1))
        tg.append(tail_guided())
    res["tail_c3_dense_us"] = round(1e3 * median(td), 1)
    res["tail_c3_one_live_us"] = round(1e3 * median(ts), 1)
    res["tail_c1_us"] = round(1e3 * median(t1), 1)
    res["tail_guided_us"] = round(1e3 * median(tg), 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
