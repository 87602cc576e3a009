"""Time the token stage of a long clip, chained against joint (19 layers, T = 100, synthetic weights, one process).

    python tools/joint_timing.py [--out profiles/NAME.json]

chained: what generate_long runs today -- window 0's chain, then one region-held chain per later window with its predecessor's
last n columns held (W chains of 100 steps at batch B, each one C call).  joint: DiffusionTransformer.sample_joint -- ONE chain of
100 steps at batch B W on the shared canvas (one C call: gather, forward, joint tail per step).  Cases: B = 1 with W = 2, 4, 8,
16, and B = 16 with W = 4, at n = 13 overlap columns, top-r 0.85, per-caption in-kernel noise.  Beside every joint chain the
plain chain (ds_denoiser_sample_rng) at the same forward batch B W: the ratio is the price of the gather and the joint tail.
The three alternate within a repeat; milliseconds of the median of --repeats timed calls after --warmup untimed ones, a device
event pair around each call, and the spread (max - min) of the joint chain's repeats.  The tails alone, on synthetic logits, at
the same number of window rows (16 x 265): the joint tail on one clip of 16 windows (3 265 canvas positions, 975 of them under
two windows), the guided tail and the plain tail on 16 clips of one grid (4 240 positions).  Prints one JSON line; asserts
nothing about the times."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from text_to_sound_synthesis_amd import _lib, audio, pipeline, synth          # noqa: E402
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
    ap.add_argument("--layers", type=int, default=19)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--overlap", type=int, default=13)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tail-repeats", type=int, default=200)
    ap.add_argument("--cases", default="1x2,1x4,1x8,1x16,16x4")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "joint_timing.py measures on the GPU: there is no other path"
    torch.set_grad_enabled(False)
    T, L, K, n = a.steps, 265, 256, a.overlap
    m = build_model(default_config(n_layer=a.layers, diffusion_step=T))
    synth.synth_init_(m, seed=0)
    m = m.cuda().eval()
    dt = m.transformer
    dt.truncation_r = 0.85
    res = {"layers": a.layers, "T": T, "overlap_cols": n, "warmup": a.warmup, "repeats": a.repeats, "cases": []}
    for case in a.cases.split(","):
        B, W = (int(v) for v in case.split("x"))
        cond = synth.synth_cond_emb(B, key="time.joint.cond").cuda()
        ids = torch.arange(B)
        kw = dict(condition_token=None, condition_mask=None, condition_embed=cond, filter_ratio=0, seed=1)

        def chained():
            cur = dt.sample(caption_ids=ids, **kw)["content_token"]
            toks = [cur]
            for w in range(1, W):
                known, keep = pipeline.continuation_tokens(cur, n)
                cur = dt.sample(caption_ids=pipeline.window_caption_ids(ids, w), content_token=known, keep_mask=keep,
                                **kw)["content_token"]
                toks.append(cur)
            return torch.stack(toks, 1)

        joint = lambda: dt.sample_joint(cond, W, n, caption_ids=ids, seed=1)
        wide = cond.repeat_interleave(W, 0).contiguous()
        wide_ids = torch.arange(B * W)
        plain = lambda: dt.sample(condition_token=None, condition_mask=None, condition_embed=wide, filter_ratio=0, seed=1,
                                  caption_ids=wide_ids)["content_token"]
        tc, tj, tp = [], [], []
        for _ in range(a.warmup + a.repeats):
            tc.append(timed(chained)[0])
            ms, canvas = timed(joint)
            tj.append(ms)
            tp.append(timed(plain)[0])
        tc, tj, tp = tc[a.warmup:], tj[a.warmup:], tp[a.warmup:]
        tok = canvas[:, pipeline.joint_window_positions(W, n).cuda()]
        shared = all(bool(torch.equal(tok[:, w, 5 * (53 - n):], tok[:, w + 1, :5 * n])) for w in range(W - 1))
        res["cases"].append({"B": B, "W": W, "canvas_positions": int(canvas.shape[1]), "forward_rows": B * W,
                             "chained_ms": round(median(tc), 1), "joint_ms": round(median(tj), 1),
                             "joint_spread_ms": round(max(tj) - min(tj), 1), "plain_chain_same_batch_ms": round(median(tp), 1),
                             "chained_over_joint": round(median(tc) / median(tj), 3),
                             "joint_over_plain_same_batch": round(median(tj) / median(tp), 4),
                             "neighbours_share_tokens": shared, "no_mask_left": bool(int(canvas.max()) < K)})

    # ---- the tails alone, on synthetic logits: 16 x 265 window rows each
    lib, sched = _lib.lib(), dt._schedule_table()
    W = 16
    Lc = 5 * pipeline.joint_canvas_cols(W, n)
    z = (torch.randn(2, W * L, K, device="cuda") * 4).contiguous()
    fade = audio.fade_table(n).cuda()
    canvas = torch.randint(0, K + 1, (1, Lc), device="cuda")
    grid = torch.randint(0, K + 1, (W, L), device="cuda")
    out_c, out_g = torch.empty_like(canvas), torch.empty_like(grid)
    t1 = torch.full((1,), T // 2, dtype=torch.long, device="cuda")
    tw = torch.full((W,), T // 2, dtype=torch.long, device="cuda")
    id1, idw = torch.arange(1, device="cuda"), torch.arange(W, device="cuda")

    def tail_joint(guided):
        return timed(lambda: _lib.check(lib.ds_sample_tail_joint_rng(
            _lib.ptr(z[0]), _lib.ptr(z[1]) if guided else None, _lib.ptr(canvas), _lib.ptr(t1), _lib.ptr(id1), 1, 0, _lib.ptr(sched),
            _lib.ptr(out_c), None, None, None, 1, W, n, 0, _lib.ptr(fade), L, K, T, 0, 0.85, 0, 3.0, None, None, 0,
            _lib.stream())))[0]

    def tail_guided():
        return timed(lambda: _lib.check(lib.ds_sample_tail_guided_rng(
            _lib.ptr(z[0]), _lib.ptr(z[1]), _lib.ptr(grid), _lib.ptr(tw), _lib.ptr(idw), 1, 0, _lib.ptr(sched), _lib.ptr(out_g), W, L,
            K, T, 0, 0.85, 0, 3.0, None, None, 0, _lib.stream())))[0]

    def tail_plain():
        return timed(lambda: _lib.check(lib.ds_sample_tail_rng(
            _lib.ptr(z[0]), _lib.ptr(grid), _lib.ptr(tw), _lib.ptr(idw), 1, 0, _lib.ptr(sched), _lib.ptr(out_g), W, L, K, T, 0, 0.85,
            0, _lib.stream())))[0]

    def gather():
        win = torch.empty(2 * W, L, dtype=torch.long, device="cuda")
        return timed(lambda: _lib.check(lib.ds_joint_gather(_lib.ptr(canvas), _lib.ptr(win), 1, W, n, 0, 2, _lib.stream())))[0]
    for _ in range(10):
        tail_joint(False), tail_joint(True), tail_guided(), tail_plain(), gather()
    tj, tjg, tg, tp, tga = [], [], [], [], []
    for _ in range(a.tail_repeats):
        tj.append(tail_joint(False))
        tjg.append(tail_joint(True))
        tg.append(tail_guided())
        tp.append(tail_plain())
        tga.append(gather())
    res["tail_joint_us"] = round(1e3 * median(tj), 1)
    res["tail_joint_guided_us"] = round(1e3 * median(tjg), 1)
    res["tail_guided_us"] = round(1e3 * median(tg), 1)
    res["tail_plain_us"] = round(1e3 * median(tp), 1)
    res["gather_2_copies_us"] = round(1e3 * median(tga), 1)
    res["tail_positions"] = {"joint": Lc, "joint_two_window": 5 * (W - 1) * n, "guided_and_plain": W * L}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
