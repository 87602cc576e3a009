"""Time of the look-ahead limiter on one GPU: every ds_limit_* entry alone, the whole of audio.limit, the levelling tail with
limit=True and with today's static cut on the same batch and target, and the vocoder pass that produces that batch, in one run.

    python tools/limit_timing.py [--iters 30] [--out profiles/NAME.json]

Cases (22 050 Hz, noise at 0.1; the loudness target asks for a gain that puts the clip's true peak 6 dB over the -1 dBFS ceiling,
so the limiter works on the blocks that hold the noise's highest peaks and passes the others through):
  batch   64 x 217 088 samples: the batch the drivers return (the vocoder on mel f32[64, 80, 848])
  long     1 x 2 646 000 samples: one two-minute clip (the vocoder on f32[1, 80, 10 335])
Milliseconds: median (min .. max) of --iters calls after 5 untimed ones, a device event pair around each call.  The traffic
floor counts the bytes each pass must move, at the 6.3 TB/s a streaming kernel reaches on this part, per sample of 4 bytes:
envelope 2 (x in, d out), apply 3 (d and x in, out out), the re-measurement 3 (two segment passes, the true peak), the trim 2
= 10 passes for audio.limit; the gain before it 3 more (13 for the limit=True tail); the static-cut tail 5.  Prints one JSON
line; asserts nothing about the times."""
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
OVER_DB = 6.0
CEILING_DB = -1.0
CASES = [("batch", 64, 217088), ("long", 1, 2646000)]


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


def entries(wave, gain):
    """the four new entries on buffers made once (run once in order first, so each finds what the one before it leaves)"""
    L = _lib.lib()
    B, T = wave.shape
    _, _, taps = audio._level_tables(RATE, wave.device)
    plan = audio.limit_plan(RATE)
    La, a = plan["L"], plan["a"]
    w = torch.from_numpy(plan["w"]).to(wave.device)
    nbytes = int(L.ds_limit_scratch_bytes(B, T, La))
    scratch = torch.empty(nbytes // 8 + 1, device=wave.device, dtype=torch.float64)
    out = torch.empty_like(wave)
    m = audio.measure_level(wave, RATE)
    peaks = torch.stack([m["sample_peak"], m["true_peak"]], 1).contiguous()
    trim, tp, red = (torch.empty(B, device=wave.device) for _ in range(3))
    lufs = torch.empty(B, device=wave.device, dtype=torch.float64)
    p, st = _lib.ptr, _lib.stream()
    fns = {
        "ds_limit_envelope": lambda: _lib.check(L.ds_limit_envelope(p(wave), B, T, None, p(taps), p(gain), CEILING_DB, La, a, p(scratch), nbytes, st)),
        "ds_limit_carry": lambda: _lib.check(L.ds_limit_carry(B, T, None, La, a, p(scratch), nbytes, st)),
        "ds_limit_apply": lambda: _lib.check(L.ds_limit_apply(p(wave), B, T, None, p(gain), La, a, p(w), p(out), None, p(scratch), nbytes, st)),
        "ds_limit_finish": lambda: _lib.check(L.ds_limit_finish(B, T, La, CEILING_DB, p(m["lufs"]), p(peaks), p(scratch), nbytes, p(trim),
                                                                p(lufs), p(tp), p(red), st)),
    }
    for fn in fns.values():
        fn()
    return fns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "limit_timing.py measures on the GPU: there is no other path"
    torch.set_grad_enabled(False)
    voc = Generator(80, 32, 3)
    synth.synth_init_(voc, seed=0)
    voc = voc.cuda().eval()
    g = torch.Generator().manual_seed(0)
    c = 10.0 ** (CEILING_DB / 20.0)
    res = {"device": torch.cuda.get_device_name(0), "rate": RATE, "iters": a.iters, "over_db": OVER_DB, "cases": {}}
    for name, B, T in CASES:
        wave = (0.1 * torch.randn(B, T, generator=g)).cuda()
        m = audio.measure_level(wave, RATE)
        # one target for the batch: the quietest-peaked row lands OVER_DB over the ceiling, the others above that
        target = float((m["lufs"] + 20.0 * torch.log10(c * 10.0 ** (OVER_DB / 20.0) / m["true_peak"].double())).max())
        _, gain = audio.level(wave, RATE, "loudness", target=target, ceiling_db=audio._NO_CEILING_DB)
        case = {"rows": B, "samples": T, "megabytes": round(B * T * 4 / 1e6, 2), "target_lufs": round(target, 3)}
        for k, fn in entries(wave, gain).items():
            case[k] = timed(fn, a.iters)
        case["limit"] = timed(lambda: audio.limit(wave, RATE, CEILING_DB, gain=gain), a.iters)
        case["level_limit_tail"] = timed(lambda: audio.level(wave, RATE, "loudness", target=target, limit=True), a.iters)
        case["level_static_tail"] = timed(lambda: audio.level(wave, RATE, "loudness", target=target), a.iters)
        out, info = audio.limit(wave, RATE, CEILING_DB, gain=gain)
        cut, _ = audio.level(wave, RATE, "loudness", target=target)
        case["max_reduction"] = round(float(info["max_reduction"].max()), 4)
        case["min_trim"] = round(float(info["trim"].min()), 6)
        case["lufs_limited_mean"] = round(float(info["lufs"].mean()), 3)
        case["lufs_static_mean"] = round(float(audio.measure_level(cut, RATE)["lufs"].mean()), 3)
        for key, passes in (("limit", 10), ("level_limit_tail", 13), ("level_static_tail", 5)):
            case[key + "_traffic_floor_ms"] = round(passes * B * T * 4 / HBM_ACHIEVABLE * 1e3, 4)
        mel = synth.synth_uniform((B, 80, T // 256), key="limit_time.mel." + name).cuda()
        case["vocoder"] = timed(lambda: voc(mel, scale=0.5, shift=0.5), max(a.iters // 3, 3), warmup=2)
        case["limit_tail_share_of_vocoder"] = round(case["level_limit_tail"]["median_ms"] / case["vocoder"]["median_ms"], 4)
        case["static_tail_share_of_vocoder"] = round(case["level_static_tail"]["median_ms"] / case["vocoder"]["median_ms"], 4)
        case["limit_tail_over_static_tail"] = round(case["level_limit_tail"]["median_ms"] / case["level_static_tail"]["median_ms"], 3)
        res["cases"][name] = case
        del wave, out, cut
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
