"""Drop-in for Diffsound/evaluation/generate_samples_batch.py:class Diffsound (:42-187).

Same constructor (config, path, ckpt_vocoder) and checkpoint conventions: ckpt['model'] ->
DALLE.load_state_dict(strict=False), ckpt['ema'] overlaid on model.get_ema_model() (:69-85); the
vocoder is Generator(n_mel_channels, ngf, n_residual_layers) as `<ckpt_vocoder>/args.yml` says + best_netG.pt
(:29-40), and NO vocoder (.npy only, no .wav) when ckpt_vocoder is falsy (:53-56).  `generate_sample_with_condition` is the
tensor-returning form of the reference's file-writing drivers: mel and waveform stay on the GPU and
the vocoder runs on the whole batch.
"""
import contextlib
import os
from collections import namedtuple

import torch

from .config import build_model, default_config, load_yaml_config
from .modeling.vocoder import Generator


def read_vocoder_args(path):
    """(n_mel_channels, ngf, n_residual_layers) from a MelGAN `args.yml` (generate_samples_batch.py:34-36).  The reference
    unpickles the training script's argparse.Namespace with yaml.UnsafeLoader; this reads only the three integer fields it
    uses, as plain `key: int` lines (the `!!python/object:argparse.Namespace` tag line is skipped, nothing is executed).
    A missing field keeps the reference configuration's value (80, 32, 3)."""
    import re
    vals = {"n_mel_channels": 80, "ngf": 32, "n_residual_layers": 3}
    with open(path, "r") as f:
        for line in f:
            m = re.match(r"^\s*(n_mel_channels|ngf|n_residual_layers)\s*:\s*(\d+)\s*(#.*)?$", line)
            if m:
                vals[m.group(1)] = int(m.group(2))
    return vals["n_mel_channels"], vals["ngf"], vals["n_residual_layers"]


def load_vocoder(ckpt_vocoder, eval_mode=True):
    """generate_samples_batch.py:29-40: `<ckpt_vocoder>/best_netG.pt` into the Generator `<ckpt_vocoder>/args.yml`
    describes (no args.yml: the reference configuration 80 / 32 / 3).  A wrong directory raises."""
    d = str(ckpt_vocoder)
    f = os.path.join(d, "best_netG.pt")
    if not os.path.exists(f):
        raise FileNotFoundError("vocoder checkpoint not found: %s" % f)
    a = os.path.join(d, "args.yml")
    g = Generator(*(read_vocoder_args(a) if os.path.exists(a) else (80, 32, 3)))
    g.load_state_dict(torch.load(f, map_location="cpu", weights_only=False))
    return {"model": g.eval() if eval_mode else g}


VOCODER_RATE = 22050          # the rate the vocoder generates at
GRID_ROWS, GRID_COLS = 5, 53  # the token grid of one clip; content_token is time-major: position 5 column + row
COLUMN_SAMPLES = 4096         # a column covers 16 mel frames = 4096 samples at 22 050 Hz (217 088 / 53)
CLIP_SAMPLES = GRID_COLS * COLUMN_SAMPLES


def _seconds_to_samples(t):
    """seconds -> samples at 22 050 Hz; a value within 1e-6 of a whole sample IS that sample (a column edge spelled as
    4096 c / 22050 must not fall to either side of it by the rounding of the division)"""
    s = float(t) * VOCODER_RATE
    return float(round(s)) if abs(s - round(s)) < 1e-6 else s


def spans_to_keep_mask(spans, batch, device="cpu"):
    """The keep mask of DALLE.inpaint_content from the time spans to REGENERATE.  spans: a list of (t0, t1) in seconds
    shared by the `batch` clips, or a list of `batch` such lists, one per clip.  Column c (all five rows of it) is regenerated
    iff [4096 c, 4096 (c + 1)) intersects a half-open span [t0, t1) in samples at 22 050 Hz.  Returns bool[batch, 265], True =
    held, in content_token's time-major order.  A span outside [0, 217088 / 22050] or with t1 <= t0 raises ValueError."""
    is_seq = lambda x: isinstance(x, (list, tuple))
    spans = list(spans)
    per_clip = len(spans) > 0 and all(is_seq(s) and (len(s) == 0 or is_seq(s[0])) for s in spans)
    if per_clip and len(spans) != batch:
        raise ValueError("per-clip spans: %d lists for a batch of %d" % (len(spans), batch))
    keep = torch.ones(batch, GRID_COLS, dtype=torch.bool)
    for b in range(batch):
        for span in (spans[b] if per_clip else spans):
            if not is_seq(span) or len(span) != 2:
                raise ValueError("a span is (t0, t1) in seconds, got %r" % (span,))
            s0, s1 = _seconds_to_samples(span[0]), _seconds_to_samples(span[1])
            if not (0.0 <= s0 and s1 <= CLIP_SAMPLES):
                raise ValueError("span %r is outside the clip [0, %d / %d s]" % (span, CLIP_SAMPLES, VOCODER_RATE))
            if not s1 > s0:
                raise ValueError("span %r is empty: t1 must be greater than t0" % (span,))
            for c in range(GRID_COLS):
                if s0 < COLUMN_SAMPLES * (c + 1) and s1 > COLUMN_SAMPLES * c:
                    keep[b, c] = False
    return keep[:, :, None].expand(batch, GRID_COLS, GRID_ROWS).reshape(batch, GRID_COLS * GRID_ROWS).to(device)


def continuation_columns(keep_seconds):
    """columns of a recording's tail that continue_audio carries over: ceil(keep_seconds 22050 / 4096), in 1 .. 52"""
    import math
    n = int(math.ceil(_seconds_to_samples(keep_seconds) / COLUMN_SAMPLES))
    if not 0 < n < GRID_COLS:
        raise ValueError("keep_seconds must cover 1 .. %d columns of %d samples, got %r" % (GRID_COLS - 1, COLUMN_SAMPLES, keep_seconds))
    return n


def continuation_tokens(tokens, n_cols):
    """tokens i64[B, 265] of a recording -> (tokens of the next clip, keep mask): the last n_cols columns become the first
    ones (a shift by 5 (53 - n_cols) tokens), held; the rest (zeros here) is to be generated."""
    n = GRID_ROWS * n_cols
    out = torch.zeros_like(tokens)
    out[:, :n] = tokens[:, tokens.shape[1] - n:]
    keep = torch.zeros(tokens.shape, dtype=torch.bool, device=tokens.device)
    keep[:, :n] = True
    return out, keep


WINDOW_ID_STRIDE = 1 << 20    # window w of a long clip draws its noise as caption id + w * 2^20 (replicates: + r * 2^24)
MAX_WINDOWS = 16              # about two minutes at the default overlap
COLUMN_FRAMES = 16            # mel frames per grid column (4096 / 256)


def long_plan(seconds, overlap_seconds=2.4):
    """The window plan of a clip longer than one 5 x 53 token grid (Diffsound.generate_long): -> (windows W, overlap columns
    n, total columns, samples).  samples = round(seconds 22050) (whole samples snapped as in spans_to_keep_mask);
    n = ceil(overlap_seconds 22050 / 4096) columns are shared by two neighbouring windows, 1 <= n <= 26 (the hop 53 - n is
    then at least n: at most two windows cover a frame); W = 1 while ceil(samples / 4096) <= 53 columns, else
    1 + ceil((columns - 53) / (53 - n)) -- the fewest windows that cover the clip -- and total = 53 + (W - 1)(53 - n).
    More than 16 windows, an overlap outside 1 .. 26 columns or a length of no samples raise ValueError.

    The default overlap (2.4 s = 13 columns) is a design choice: the later window is generated with those columns of the
    earlier one held as context, and their mel frames are cross-faded.  No trained checkpoint has been available to this
    project, so how the seams SOUND at this or any other overlap has not been measured."""
    import math
    samples = int(round(_seconds_to_samples(seconds)))
    if samples < 1:
        raise ValueError("seconds must cover at least one sample, got %r" % (seconds,))
    n = int(math.ceil(_seconds_to_samples(overlap_seconds) / COLUMN_SAMPLES))
    if not 1 <= n <= GRID_COLS // 2:
        raise ValueError("overlap_seconds must cover 1 .. %d columns of %d samples, got %r (%d columns)"
                         % (GRID_COLS // 2, COLUMN_SAMPLES, overlap_seconds, n))
    needed = -(-samples // COLUMN_SAMPLES)
    hop = GRID_COLS - n
    windows = 1 if needed <= GRID_COLS else 1 + -(-(needed - GRID_COLS) // hop)
    if windows > MAX_WINDOWS:
        raise ValueError("%r s needs %d windows at an overlap of %d columns: at most %d (%.1f s)"
                         % (seconds, windows, n, MAX_WINDOWS, (GRID_COLS + (MAX_WINDOWS - 1) * hop) * COLUMN_SAMPLES / VOCODER_RATE))
    return windows, n, GRID_COLS + (windows - 1) * hop, samples


def joint_canvas_cols(windows, overlap_cols, ring=False):
    """Columns C of the token canvas of joint-window sampling: `windows` = W grids of 53 columns, neighbours sharing n =
    overlap_cols of them (hop h = 53 - n).  line: C = 53 + (W - 1) h, W >= 1; ring: C = W h, W >= 2 (window w covers columns
    (w h + o) mod C).  1 <= n <= 26, so n <= h and at most two windows cover a column.  Anything else raises ValueError."""
    W, n = int(windows), int(overlap_cols)
    if not 1 <= n <= GRID_COLS // 2:
        raise ValueError("overlap_cols must be in 1 .. %d, got %r" % (GRID_COLS // 2, overlap_cols))
    if W < (2 if ring else 1):
        raise ValueError("%s needs at least %d window%s, got %r" % ((("a ring", 2, "s") if ring else ("a canvas", 1, "")) + (windows,)))
    h = GRID_COLS - n
    return W * h if ring else GRID_COLS + (W - 1) * h


def joint_map(windows, overlap_cols, ring=False):
    """The host mirror of the joint tail's geometry (csrc/sampler.hip SampleJoint): for every canvas column c
    -> dict of numpy arrays of length C = joint_canvas_cols(...):
        'later' / 'later_offset'      w1 = min(c // h, W - 1) (ring: c // h) and o1 = c - w1 h
        'earlier' / 'earlier_offset'  w0 = (w1 - 1) mod W and o1 + h where o1 < n and (w1 >= 1 or ring); -1 elsewhere
        'weight'                      f32: the later window's weight -- audio.fade_table(n)[o1] under two windows (sin^2, in
                                      (0, 1); the earlier window's is 1 - weight), 1 under one
    and 'columns' = C.  Canvas positions are time-major, q = 5 c + r, as in content_token."""
    import numpy as np
    from .audio import fade_table
    W, n = int(windows), int(overlap_cols)
    C = joint_canvas_cols(W, n, ring)
    h = GRID_COLS - n
    c = np.arange(C)
    w1 = c // h if ring else np.minimum(c // h, W - 1)
    o1 = c - w1 * h
    two = (o1 < n) & ((w1 >= 1) | bool(ring))
    fade = fade_table(n).numpy()
    return {"columns": C, "later": w1, "later_offset": o1, "earlier": np.where(two, (w1 - 1) % W, -1),
            "earlier_offset": np.where(two, o1 + h, -1),
            "weight": np.where(two, fade[np.minimum(o1, n - 1)], np.float32(1.0)).astype(np.float32)}


def joint_window_positions(windows, overlap_cols, ring=False):
    """i64[W, 265]: the canvas position of every token of every window (window w, offset o, row r -> 5 ((w h + o) mod C) + r):
    canvas[:, joint_window_positions(...)] cuts the windows from a canvas, as ds_joint_gather does on the device."""
    W, n = int(windows), int(overlap_cols)
    C = joint_canvas_cols(W, n, ring)
    h = GRID_COLS - n
    col = (torch.arange(W)[:, None] * h + torch.arange(GRID_COLS)[None, :]) % C                 # [W, 53]
    return (GRID_ROWS * col[:, :, None] + torch.arange(GRID_ROWS)[None, None, :]).reshape(W, GRID_ROWS * GRID_COLS)


def loop_plan(seconds, overlap_seconds=2.4):
    """The window plan of a seamless loop (Diffsound.generate_loop): -> (windows W, overlap columns n, ring columns C, samples).
    n as in long_plan; W is the smallest W >= 2 with W h >= ceil(round(seconds 22050) / 4096), h = 53 - n, and the loop that
    is made is C = W h WHOLE columns -- a loop's length snaps UP to a multiple of h columns -- of samples = 4096 C samples:
    the length made, not the one asked for.  A ring under 54 columns (10.03 s) would need a window that overlaps itself and is
    not built: a length that fits one window (<= 53 columns) raises ValueError, and so do more than 16 windows."""
    import math
    asked = int(round(_seconds_to_samples(seconds)))
    if asked < 1:
        raise ValueError("seconds must cover at least one sample, got %r" % (seconds,))
    n = int(math.ceil(_seconds_to_samples(overlap_seconds) / COLUMN_SAMPLES))
    if not 1 <= n <= GRID_COLS // 2:
        raise ValueError("overlap_seconds must cover 1 .. %d columns of %d samples, got %r (%d columns)"
                         % (GRID_COLS // 2, COLUMN_SAMPLES, overlap_seconds, n))
    hop = GRID_COLS - n
    needed = -(-asked // COLUMN_SAMPLES)
    if needed <= GRID_COLS:
        raise ValueError("a loop of %r s fits one window (%d columns): the shortest ring is two windows, %d columns (%.2f s)"
                         % (seconds, needed, GRID_COLS + 1, (GRID_COLS * COLUMN_SAMPLES + 1) / VOCODER_RATE))
    windows = max(2, -(-needed // hop))
    if windows > MAX_WINDOWS:
        raise ValueError("a loop of %r s needs %d windows at an overlap of %d columns: at most %d (%.1f s)"
                         % (seconds, windows, n, MAX_WINDOWS, MAX_WINDOWS * hop * COLUMN_SAMPLES / VOCODER_RATE))
    return windows, n, windows * hop, windows * hop * COLUMN_SAMPLES


LOOP_LEAD_HOPS = 2            # hops of the ring's own content rendered ahead of the loop that is cut out (generate_loop)


def loop_cut(columns, hop_cols, sample_rate=None):
    """Where generate_loop cuts the loop out of its rendering, at the output rate -> (offset, period) in whole samples.  At
    22 050 Hz the rendering starts LOOP_LEAD_HOPS hops ahead of the ring (offset = 2 hop_cols 4096) and the period is 4096
    columns samples; at another rate both are multiplied by sample_rate / 22 050 and must stay WHOLE: a loop point is exact or
    it is not emitted.  44 100 and 11 025 Hz always work; 48 000 Hz needs 147 to divide both column counts.  Otherwise
    ValueError, naming the period."""
    rate = VOCODER_RATE if sample_rate is None else int(sample_rate)
    if rate <= 0:
        raise ValueError("sample_rate must be positive, got %r" % (sample_rate,))
    off, period = LOOP_LEAD_HOPS * int(hop_cols) * COLUMN_SAMPLES, int(columns) * COLUMN_SAMPLES
    if (off * rate) % VOCODER_RATE or (period * rate) % VOCODER_RATE:
        raise ValueError("a loop of %d columns has a period of %d samples at %d Hz = %s samples at %d Hz (offset %s): not whole, "
                         "and no approximate loop point is emitted -- use 44100, 11025 or 22050 Hz"
                         % (columns, period, VOCODER_RATE, "%d/%d" % (period * rate, VOCODER_RATE), rate,
                            "%d/%d" % (off * rate, VOCODER_RATE)))
    return off * rate // VOCODER_RATE, period * rate // VOCODER_RATE


def window_caption_ids(caption_ids, window):
    """The caption ids window `window` of a long clip draws its noise under: ids + window 2^20 (i64 tensor).  Ids must be in
    0 .. 2^20 - 1, which keeps the windows apart from each other and from the replicate stride 2^24; else ValueError."""
    ids = torch.as_tensor(caption_ids, dtype=torch.long).reshape(-1)
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= WINDOW_ID_STRIDE):
        raise ValueError("caption ids of a long clip must be in 0 .. %d (window w draws as id + w 2^20)" % (WINDOW_ID_STRIDE - 1))
    if not 0 <= int(window) < MAX_WINDOWS:
        raise ValueError("window must be in 0 .. %d, got %r" % (MAX_WINDOWS - 1, window))
    return ids + int(window) * WINDOW_ID_STRIDE


MAX_TRACKS = 4                # caption tracks per scene (DS_MAX_TRACKS, include/diffsound_hip.h)


def track_weights(tracks, total_cols=GRID_COLS, batch=None):
    """The caption tracks of a scene (DALLE.generate_content: tracks) from seconds.  A track is (text, t0, t1) or
    (text, t0, t1, scale): the caption applies over the half-open span [t0, t1) seconds with weight `scale` (default 1;
    Diffsound.generate_scene fills in its own default); t1 None: to the end of the clip.  `tracks` is one scene -- a list of
    tracks, shared by `batch` clips (default 1) -- or a list of B scenes.  Column c of a track gets scale x the fraction of the
    column's 4096 samples [4096 c, 4096 (c + 1)) the span covers (seconds -> samples snapped as in spans_to_keep_mask): scale
    inside the span, exactly 0 outside, the proportional value in an edge column -- the ramp, with no further parameter --
    and all five rows of a column share it.  Scenes with fewer tracks are padded with zero-weight tracks of the empty caption
    up to the largest C.  More than 4 tracks, a span outside [0, 4096 total_cols / 22050], an empty span or a non-finite
    scale raise ValueError.  Returns (C lists of B captions, f32[B, C, 5 total_cols] time-major like content_token)."""
    import math
    is_seq = lambda x: isinstance(x, (list, tuple))
    is_track = lambda x: is_seq(x) and len(x) in (3, 4) and isinstance(x[0], str)
    tracks = list(tracks)
    if all(is_track(t) for t in tracks):
        scenes = [tracks] * (1 if batch is None else int(batch))
    elif all(is_seq(sc) and all(is_track(t) for t in sc) for sc in tracks):
        scenes = [list(sc) for sc in tracks]
        if batch is not None and len(scenes) != batch:
            raise ValueError("per-clip scenes: %d lists for a batch of %d" % (len(scenes), batch))
    else:
        raise ValueError("a track is (text, t0, t1) or (text, t0, t1, scale); tracks is one scene or a list of scenes")
    total_cols = int(total_cols)
    C = max((len(sc) for sc in scenes), default=0)
    if not 1 <= C <= MAX_TRACKS or not scenes:
        raise ValueError("a scene has 1 .. %d tracks, got %d" % (MAX_TRACKS, C))
    end = total_cols * COLUMN_SAMPLES
    texts = [["" for _ in scenes] for _ in range(C)]
    weight = torch.zeros(len(scenes), C, total_cols)
    for b, sc in enumerate(scenes):
        for i, trk in enumerate(sc):
            scale = float(trk[3]) if len(trk) == 4 else 1.0
            if not math.isfinite(scale):
                raise ValueError("track %r: the scale must be finite" % (trk,))
            s0, s1 = _seconds_to_samples(trk[1]), float(end) if trk[2] is None else _seconds_to_samples(trk[2])
            if not (0.0 <= s0 and s1 <= end):
                raise ValueError("track %r is outside the clip [0, %d / %d s]" % (trk, end, VOCODER_RATE))
            if not s1 > s0:
                raise ValueError("track %r is empty: t1 must be greater than t0" % (trk,))
            texts[i][b] = trk[0]
            for c in range(total_cols):
                cover = min(s1, COLUMN_SAMPLES * (c + 1)) - max(s0, COLUMN_SAMPLES * c)
                if cover > 0:
                    weight[b, i, c] = scale * (cover / COLUMN_SAMPLES)
    weight = weight[:, :, :, None].expand(-1, -1, -1, GRID_ROWS).reshape(len(scenes), C, total_cols * GRID_ROWS)
    return texts, weight.contiguous()


def purity_sample_type(sample_type, purity_steps, purity_weight=0.0):
    """sample_type + the ",purity{S}" / ",purity{S}w{r}" part the drivers' purity_steps / purity_weight keywords stand for
    (DALLE._purity_part); purity_steps None: sample_type as it is -- purity_weight is not looked at."""
    if purity_steps is None:
        return sample_type
    w = float(purity_weight)
    return "%s,purity%d%s" % (sample_type, int(purity_steps), "" if w == 0.0 else "w%r" % w)


def level_spec(level, takes_recording):
    """The drivers' `level` keyword -> None or {"strategy", "target", "ceiling_db"}: a strategy name of audio.level ("peak",
    "rms", "loudness", "match") or a dict {strategy[, target][, ceiling_db][, limit]}.  "match" -- the result takes the loudness
    of the recording the driver was given -- only where there is one (takes_recording).  limit (True, or a dict {lookahead_ms,
    release_ms}; audio.level) puts the look-ahead limiter in place of the static cut under the ceiling; the returned dict
    carries the key only where the caller gave it.  Anything else raises ValueError."""
    from . import audio
    if level is None:
        return None
    spec = {"strategy": level} if isinstance(level, str) else level
    if not isinstance(spec, dict) or "strategy" not in spec or set(spec) - {"strategy", "target", "ceiling_db", "limit"}:
        raise ValueError("level is a strategy name or a dict {strategy, target, ceiling_db, limit}, got %r" % (level,))
    strategy, target = spec["strategy"], spec.get("target")
    if strategy not in audio.LEVEL_STRATEGIES:
        raise ValueError("level: strategy must be one of %s, got %r" % (", ".join(sorted(audio.LEVEL_STRATEGIES)), strategy))
    if strategy == "match" and not takes_recording:
        raise ValueError('level="match" needs a recording to match: this driver takes none')
    if strategy == "match" and target is not None:
        raise ValueError('level="match" takes its target from the recording')
    out = {"strategy": strategy, "target": None if target is None else float(target),
           "ceiling_db": float(spec.get("ceiling_db", -1.0))}
    if "limit" in spec:
        audio._limit_spec(spec["limit"])                 # its form is checked here, before anything runs
        out["limit"] = spec["limit"]
    return out


def recording_loudness(item, rate=None, device="cuda"):
    """Integrated loudness f64[B] (device) of the recordings a driver was given (`audio` / `audio_rate` as in
    melspec.mel_image_from_audio), each measured at its own rate and over its own length by audio.measure_level."""
    from . import audio
    from .modeling.melspec import SAMPLE_RATE, _clip_rates
    if torch.is_tensor(item) and item.is_cuda:
        wave = item[None] if item.dim() == 1 else item
        rates = [SAMPLE_RATE if r is None else r for r in _clip_rates(rate, wave.shape[0])]
        if len(set(rates)) == 1:
            return audio.measure_level(wave, rates[0])["lufs"]
        return torch.cat([audio.measure_level(wave[i:i + 1], r)["lufs"] for i, r in enumerate(rates)])
    clips = [item] if isinstance(item, (str, os.PathLike)) or (torch.is_tensor(item) and item.dim() == 1) else list(item)
    rates = _clip_rates(rate, len(clips))
    out = []
    for i, clip in enumerate(clips):
        if isinstance(clip, (str, os.PathLike)):
            x, sr = audio.read_wav(clip)
        else:
            x, sr = torch.as_tensor(clip).float().reshape(-1), SAMPLE_RATE if rates[i] is None else rates[i]
        out.append(audio.measure_level(x[None].to(device), int(sr))["lufs"])
    return torch.cat(out)


# Where the recording lies under the rendering -- a definition, from the two front ends in the code.  Content-image frame j is
# front-end frame j + 6 (the centre crop of melspec.WaveToMel: (860 - 848) / 2), and that frame is centred on recording sample
# 256 (j + 6) (frames are centred: PAD = N_FFT / 2).  The vocoder renders frame j into output samples [256 j, 256 j + 256), and
# under the MelGAN Audio2Mel convention (pad (1024 - 256) / 2, no centring) frame j is centred on sample 256 j + 128.  So output
# sample n at 22 050 Hz is recording sample n + 6 * 256 - 128: a constant shift, no drift.
RECORDING_OFFSET = 6 * 256 - 128          # 1408
FADE_SECONDS = 1024 / VOCODER_RATE        # the default cross-fade at the edge of a kept column: 4 mel frames
KEEP_ORIGINAL = (None, "mel", "audio")


def recording_offset(rate=None, shift_columns=0):
    """The recording sample under output sample 0 at `rate` Hz (None: 22 050): floor((1408 + 4096 shift_columns) rate / 22050
    + 0.5) -- 1408, 2816 at 44 100, 3065 at 48 000, 1022 at 16 000; shift_columns: the columns continue_audio skips."""
    rate = VOCODER_RATE if rate is None else int(rate)
    at_22k = RECORDING_OFFSET + COLUMN_SAMPLES * int(shift_columns)
    return (2 * at_22k * rate + VOCODER_RATE) // (2 * VOCODER_RATE)


def _check_keep_original(keep_original, fade_seconds, has_vocoder):
    """the ValueErrors of the `keep_original` / `fade_seconds` keywords -> fade_seconds as a float"""
    import math
    if keep_original not in KEEP_ORIGINAL:
        raise ValueError('keep_original must be None, "mel" or "audio", got %r' % (keep_original,))
    if keep_original == "audio" and not has_vocoder:
        raise ValueError('keep_original="audio" needs a vocoder: there is no waveform to paste into')
    fade_seconds = float(fade_seconds)
    if keep_original is not None and not (math.isfinite(fade_seconds) and fade_seconds >= 0.0):
        raise ValueError("fade_seconds must be finite and >= 0, got %r" % (fade_seconds,))
    return fade_seconds


def paste_plan(driver, keep_original, *, batch, spans=None, keep_seconds=None, seconds=None, sample_rate=None,
               fade_seconds=FADE_SECONDS, match_gain=True, has_vocoder=True):
    """What `keep_original` means for one driver call, on the host: None for keep_original None, else
      {"mode": "mel" | "audio", "keep_cols": u8[batch, n_cols] (1 = the recording's column is kept), "match_gain",
       "mel":   {"off", "col_num": 16, "col_den": 1, "fade_len"}   in mel frames,
       "audio": {"off", "col_num", "col_den", "fade_len", "rate"}  in samples at the output rate; col_num / col_den =
                4096 rate / 22050 in lowest terms}.
    driver "inpaint_audio" / "inpaint_scene": the columns spans_to_keep_mask(spans) holds; "continue_audio": the first
    n = continuation_columns(keep_seconds) columns, which are the recording's last n -- the offsets grow by 53 - n columns
    (16 (53 - n) frames; 4096 (53 - n) samples at 22 050 Hz, scaled with the 1408 and rounded once); "extend_audio": the first
    53 of the ceil(samples / 4096) columns of a clip of `seconds`.  fade_len = fade_seconds x 22050 / 256 frames and
    fade_seconds x rate samples.  An unknown keep_original, "audio" without a vocoder and a negative or non-finite
    fade_seconds raise ValueError."""
    import math
    fade_seconds = _check_keep_original(keep_original, fade_seconds, has_vocoder)
    if keep_original is None:
        return None
    batch, shift = int(batch), 0
    if driver in ("inpaint_audio", "inpaint_scene"):
        keep_cols = spans_to_keep_mask(spans, batch).view(batch, GRID_COLS, GRID_ROWS)[:, :, 0]
    elif driver == "continue_audio":
        n = continuation_columns(keep_seconds)
        keep_cols = torch.zeros(batch, GRID_COLS, dtype=torch.bool)
        keep_cols[:, :n] = True
        shift = GRID_COLS - n
    elif driver == "extend_audio":
        n_cols = -(-int(round(_seconds_to_samples(seconds))) // COLUMN_SAMPLES)       # long_plan's samples
        if n_cols <= GRID_COLS:
            raise ValueError("extend_audio: seconds must exceed one grid, got %r" % (seconds,))
        keep_cols = torch.zeros(batch, n_cols, dtype=torch.bool)
        keep_cols[:, :GRID_COLS] = True
    else:
        raise ValueError("paste_plan: no driver %r" % (driver,))
    rate = VOCODER_RATE if sample_rate is None else int(sample_rate)
    g = math.gcd(COLUMN_SAMPLES * rate, VOCODER_RATE)
    return {"mode": keep_original, "keep_cols": keep_cols.to(torch.uint8).contiguous(), "match_gain": bool(match_gain),
            "mel": {"off": COLUMN_FRAMES * shift, "col_num": COLUMN_FRAMES, "col_den": 1,
                    "fade_len": fade_seconds * VOCODER_RATE / 256},
            "audio": {"off": recording_offset(rate, shift), "col_num": COLUMN_SAMPLES * rate // g, "col_den": VOCODER_RATE // g,
                      "fade_len": fade_seconds * rate, "rate": rate}}


def recording_at_rate(item, rate, out_rate, device="cuda"):
    """The recordings a driver was given (`audio` / `audio_rate` as in melspec.mel_image_from_audio: a device tensor, host
    arrays or `.wav` paths; one rate or one per clip) at `out_rate` Hz -> (f32[B, Tr] on the device, lengths i32[B] on the
    device).  Rows are grouped by rate, one audio.resample per distinct rate; a clip whose rate already is out_rate is NOT
    resampled: its samples go through untouched."""
    from . import audio
    from .modeling.melspec import SAMPLE_RATE, _clip_rates
    out_rate = int(out_rate)
    if torch.is_tensor(item) and item.is_cuda:
        wave = (item[None] if item.dim() == 1 else item).float()
        rates = [SAMPLE_RATE if r is None else int(r) for r in _clip_rates(rate, wave.shape[0])]
        clips, lens_in, device = None, [wave.shape[1]] * wave.shape[0], wave.device
        if len(set(rates)) == 1:
            out = wave.contiguous() if rates[0] == out_rate else audio.resample(wave, rates[0], out_rate)
            return out, torch.full((out.shape[0],), out.shape[1], dtype=torch.int32, device=device)
    else:
        clips = [item] if isinstance(item, (str, os.PathLike)) or (torch.is_tensor(item) and item.dim() == 1) else list(item)
        rates = _clip_rates(rate, len(clips))
        waves = []
        for i, clip in enumerate(clips):
            if isinstance(clip, (str, os.PathLike)):
                x, rates[i] = audio.read_wav(clip)
            else:
                x, rates[i] = torch.as_tensor(clip).float().reshape(-1), SAMPLE_RATE if rates[i] is None else int(rates[i])
            waves.append(x)
        lens_in = [x.numel() for x in waves]
    lens = [audio.resample_length(n, r, out_rate) for n, r in zip(lens_in, rates)]
    buf = torch.zeros(len(lens), max(max(lens), 1), device=device)
    for r in sorted(set(rates)):
        rows = [i for i, q in enumerate(rates) if q == r]
        if clips is None:
            part = wave[rows]
        else:
            part = torch.zeros(len(rows), max(max(lens_in[i] for i in rows), 1))
            for k, i in enumerate(rows):
                part[k, :lens_in[i]] = waves[i]
            part = part.to(device)
        if r != out_rate:
            part = audio.resample(part, r, out_rate, lengths=[lens_in[i] for i in rows])
        buf[rows, :part.shape[1]] = part[:, :buf.shape[1]]
    return buf, torch.tensor(lens, dtype=torch.int32).to(device)


_Request = namedtuple("_Request", "level recording paste")      # what one driver call asks of the tail the drivers share


def _request(self, level, recording=None, keep_original=None, fade_seconds=FADE_SECONDS, match_gain=True):
    """A driver's `level` (level_spec) and `keep_original` / `fade_seconds` / `match_gain` (paste_plan) keywords, checked ->
    the _Request its tail is given: (the level spec or None, the recording (audio, audio_rate) the driver takes or None, the
    paste_plan keywords or None).  The first statement of every driver: a bad keyword raises ValueError before any work."""
    spec = level_spec(level, recording is not None)
    _check_keep_original(keep_original, fade_seconds, self.vocoder is not None)
    paste = dict(keep_original=keep_original, fade_seconds=fade_seconds, match_gain=match_gain)
    return _Request(spec, recording, None if keep_original is None else paste)


def _sample_type(truncation_rate, fast=False, purity_steps=None, purity_weight=0.0):
    """the drivers' truncation_rate / fast / purity_steps / purity_weight -> DALLE's sample_type "top{rate}r[,fast{n - 1}][,purity..]";
    fast=n is skip_step n - 1, spelled like the reference's drivers"""
    skip = ",fast" + str(fast - 1) if fast else ""
    return purity_sample_type("top" + str(truncation_rate) + "r" + skip, purity_steps, purity_weight)


def _numbered_stems(root, n):
    """`root` (made where missing) -> the n path stems root/000000, root/000001, ..."""
    os.makedirs(root, exist_ok=True)
    return [os.path.join(root, str(i).zfill(6)) for i in range(n)]


def _write_clips(mel01, wave, rate, stems):
    """clip i of mel01 f32[B, 80, F] -> `{stems[i]}.npy` and, with a waveform f32[B, 1, T] at `rate` (None: 22 050 Hz), of wave ->
    `{stems[i]}.wav` (PCM_24), clip by clip -> stems"""
    import numpy as np
    m_, w_ = mel01.cpu().numpy(), None if wave is None else wave[:, 0].cpu().numpy()
    for i, stem in enumerate(stems):
        np.save(stem + ".npy", m_[i])
        if w_ is not None:
            write_wav_pcm24(stem + ".wav", w_[i], VOCODER_RATE if rate is None else int(rate))
    return stems


class Diffsound:
    def __init__(self, config=None, path=None, ckpt_vocoder=None, device="cuda", random_vocoder=False):
        """ckpt_vocoder falsy: `self.vocoder = None` and the drivers write `.npy` only, as the reference does (:53-56).
        random_vocoder=True (tests / benchmarks without a checkpoint) builds a random-weight Generator(80, 32, 3) instead."""
        cfg = default_config(with_clip=True) if config is None else (load_yaml_config(config) if isinstance(config, str) else config)
        self.model = build_model(cfg)
        self.epoch = 0
        if path is not None:       # path=None: seeded / random weights on purpose (tests, bench); a wrong path raises
            if not os.path.exists(path):
                raise FileNotFoundError("Diffsound checkpoint not found: %s" % path)
            ckpt = torch.load(path, map_location="cpu", weights_only=False)
            self.epoch = ckpt.get("last_epoch", ckpt.get("epoch", 0))
            self.model.load_state_dict(ckpt["model"], strict=False)
            if "ema" in ckpt:
                self.model.get_ema_model().load_state_dict(ckpt["ema"], strict=False)
        self.model = self.model.to(device).eval()
        for p in self.model.parameters():
            p.requires_grad = False
        if ckpt_vocoder:
            self.vocoder = load_vocoder(ckpt_vocoder)["model"].to(device)
        elif random_vocoder:
            self.vocoder = Generator(80, 32, 3).eval().to(device)
        else:
            self.vocoder = None
        if self.vocoder is not None:
            for p in self.vocoder.parameters():
                p.requires_grad = False

    @torch.no_grad()
    def generate_sample_with_condition(self, cond, truncation_rate=0.85, replicate=1, fast=False, caption_ids=None,
                                       seed=None, sample_rate=None, guidance_scale=None, negative_text=None, purity_steps=None,
                                       purity_weight=0.0, *, level=None):
        """Captions -> (mel01 f32[B,80,848], wave f32[B,1,217088] -- None without a vocoder --, tokens), everything left on the GPU.
        `cond` is a list of caption strings (needs the text stage: tokenizer + CLIP in the config),
        token ids i64[B,77], or caption embeddings f32[B,77,512].  fast=n selects the skip-step sampler with
        skip_step n-1, spelled like the reference's drivers (generate_samples_batch.py:100-103,148-151).
        caption_ids (one global index per caption) switches the sampler to per-caption in-kernel noise: a caption's clip
        then does not depend on the batch it is generated in (DiffusionTransformer.rng_mode); replicate r of caption i
        draws as caption id ids[i] + r * 2^24.  sample_rate: the rate of the returned waveform; another one than 22 050 Hz is the
        vocoder's output resampled on the device (audio.resample): f32[B,1,ceil(217088 sample_rate / 22050)].
        guidance_scale: classifier-free guidance (DALLE.generate_content) against the empty caption or negative_text (a
        caption, or one per caption); None or 1: unguided.
        purity_steps = S: an S-step purity-prior chain instead of the reference's 100-step loop (DiffusionTransformer.
        sample_purity: 1 <= S <= 265 forwards, confident positions first, no [MASK] left at any S), purity_weight its
        sharpening weight; None: today's path, untouched.  Not together with fast.  Its effect on audio quality is unmeasured.
        level= (keyword-only, on this and every driver that returns or writes a waveform; level_spec): bring every
        clip to a level on the device, at the output rate -- "peak" (-1 dBFS), "rms" (-20 dBFS), "loudness" (-23 LUFS, BS.1770-4)
        or a dict {strategy, target, ceiling_db, limit}, under a true-peak ceiling of -1 dBFS (audio.level: a static cut, or
        with limit=True the look-ahead limiter); the drivers that take a recording also accept "match": the recording's own
        loudness.  None: the vocoder's own level, no launch.  Mel and tokens are never affected; generate_best_of levels the
        winners only."""
        request = _request(self, level)
        out = self.model.generate_content(batch=self._batch(cond, caption_ids, seed, negative_text), filter_ratio=0,
                                          replicate=replicate, content_ratio=1, return_att_weight=False,
                                          guidance_scale=guidance_scale,
                                          sample_type=_sample_type(truncation_rate, fast, purity_steps, purity_weight))
        mel = out["content"]                                   # [B,1,80,848] in ~[-1,1]
        wave = None if self.vocoder is None else self.vocoder(mel[:, 0], scale=0.5, shift=0.5)   # spec = (x+1)/2, :182
        return (mel[:, 0] + 1) / 2, self._finish(wave, sample_rate, request), out["content_token"]

    @staticmethod
    def _batch(text, caption_ids=None, seed=None, negative_text=None):
        """The batch dict of a model call: the caption(s) -- strings, token ids i64[B,77] or embeddings f32[B,77,512]; None: no
        caption, the tracks of a scene carry them -- and those of the noise / guidance keywords that were given."""
        if text is None:
            batch = {}
        elif isinstance(text, (list, tuple, str)):
            batch = {"text": [text] if isinstance(text, str) else list(text)}
        else:
            batch = {"condition_token": text} if text.dtype == torch.long else {"condition_embed_token": text}
        for key, value in (("caption_ids", caption_ids), ("seed", seed), ("negative_text", negative_text)):
            if value is not None:
                batch[key] = value
        return batch

    @staticmethod
    def _at_rate(wave, sample_rate):
        """the vocoder's f32[B,1,T] at 22 050 Hz -> at `sample_rate` (None / 22 050: as it is)"""
        if wave is None or sample_rate is None or sample_rate == VOCODER_RATE:
            return wave
        from . import audio
        return audio.resample(wave[:, 0], VOCODER_RATE, sample_rate)[:, None]

    def _paste_plan(self, request, driver, batch, **where):
        """paste_plan for the `keep_original` of a driver call's request (None without one) + the recording the driver was given"""
        if request.paste is None:
            return None
        plan = paste_plan(driver, batch=batch, has_vocoder=self.vocoder is not None, **request.paste, **where)
        return dict(plan, recording=request.recording)

    @staticmethod
    def _paste_mel(mel, plan):
        """the decoder's mel f32[B,80,F] in [-1,1] -> with the recording's own content image in the kept columns (plan None:
        as it is)"""
        if plan is None:
            return mel
        from . import audio
        from .modeling.melspec import mel_image_from_audio
        image = mel_image_from_audio(plan["recording"][0], mel.device, rate=plan["recording"][1])[:, 0]
        p = plan["mel"]
        return audio.paste(mel, image, plan["keep_cols"], off=p["off"], col_num=p["col_num"], col_den=p["col_den"],
                           fade_len=p["fade_len"], curve="linear")

    @staticmethod
    def _paste_audio(wave, plan):
        """the rendering f32[B,1,T] at the output rate -> with the recording's own samples in the kept columns (mode "audio")"""
        if wave is None or plan is None or plan["mode"] != "audio":
            return wave
        from . import audio
        p = plan["audio"]
        rec, lens = recording_at_rate(plan["recording"][0], plan["recording"][1], p["rate"], wave.device)
        return audio.paste(wave[:, 0], rec, plan["keep_cols"], off=p["off"], col_num=p["col_num"], col_den=p["col_den"],
                           fade_len=p["fade_len"], curve="equal_power", rec_len=lens, match_gain=plan["match_gain"])[:, None]

    @staticmethod
    def _finish(wave, sample_rate, request, paste=None):
        """The tail every driver shares: the vocoder's f32[B,1,T] -> at `sample_rate` (_at_rate) -> the recording's samples
        pasted over it (paste = a paste_plan of mode "audio") -> brought to the level the driver call asked for (request =
        its _Request), at that rate, on the device (audio.level).  No plan and no `level`: no launch, the waveform as it is."""
        return Diffsound._level(Diffsound._paste_audio(Diffsound._at_rate(wave, sample_rate), paste), sample_rate, request)

    @staticmethod
    def _level(wave, sample_rate, request):
        """_finish's last step on a waveform that is already at `sample_rate`"""
        spec, recording = request.level, request.recording
        if wave is None or spec is None:
            return wave
        from . import audio
        rate = VOCODER_RATE if sample_rate is None else int(sample_rate)
        ref = recording_loudness(recording[0], recording[1], wave.device) if spec["strategy"] == "match" else None
        out, _ = audio.level(wave[:, 0], rate, spec["strategy"], target=spec["target"], ceiling_db=spec["ceiling_db"],
                             reference=ref, limit=spec.get("limit"))
        return out[:, None]

    @torch.no_grad()
    def generate_sample_from_audio(self, audio, text, filter_ratio=0.5, truncation_rate=0.85, save_root=None, audio_rate=None,
                                   *, level=None):
        """Re-sample given recordings under new captions: audio (f32[B, T] on the device, or a list of `.wav` paths / host
        arrays; audio_rate = their sample rate, one or a list, None = 22 050 Hz / the files' own: another rate is resampled on
        the device first) -> mel (modeling/melspec.py, one HIP launch) -> VQ tokens -> diffused forward to
        t = int(T * filter_ratio) - 1 and denoised from there under `text` (a list of B captions, token ids or embeddings, as in
        generate_sample_with_condition) -> decode -> vocoder.  Returns (mel01 f32[B,80,848], wave f32[B,1,217088] or None,
        tokens); with save_root also writes `{i:06d}.npy` and, with a vocoder, `{i:06d}.wav` like the other drivers."""
        request = _request(self, level, (audio, audio_rate))
        model = self.model
        cond = model.prepare_condition(self._batch(text))
        content = model.prepare_content({"audio": audio, "audio_rate": audio_rate})
        with self._truncation(truncation_rate):
            out = model.transformer.sample(condition_token=cond.get("condition_token"), condition_mask=cond.get("condition_mask"),
                                           condition_embed=cond.get("condition_embed_token"),
                                           content_token=content["content_token"], filter_ratio=filter_ratio, print_log=False)
        return self._render(request, out["content_token"], content["content_quant"].shape, save_root)

    @contextlib.contextmanager
    def _truncation(self, truncation_rate, forward=False):
        """The model's truncation state at this call's rate inside the block (forward: with truncation_forward on, as a chain
        through DALLE needs it) and what it was after it, also when the block raises: the facade installs a rate once and
        keeps it."""
        model, tr = self.model, self.model.transformer
        saved = tr.truncation_r, tr.truncation_k, tr.repeat_rate, model.truncation_forward
        tr.truncation_r, tr.truncation_k = float(truncation_rate), None
        if forward:
            model.truncation_forward = True
        try:
            yield
        finally:
            tr.truncation_r, tr.truncation_k, tr.repeat_rate, model.truncation_forward = saved

    def _render(self, request, tokens, zshape, save_root=None, sample_rate=None, paste=None):
        """tokens -> decode (-> the recording's mel pasted: paste = a paste_plan) -> vocoder (-> sample_rate -> the recording's
        samples pasted -> level, as the driver call's request says: _finish): the tail the audio-in drivers share.  Returns
        (mel01, wave or None, tokens); with save_root also writes `{i:06d}.npy` and, with a vocoder, `{i:06d}.wav`."""
        mel = self.model.decode_to_img(tokens, zshape)
        if paste is not None:
            mel = self._paste_mel(mel[:, 0], paste)[:, None]
        wave = None if self.vocoder is None else self.vocoder(mel[:, 0], scale=0.5, shift=0.5)
        wave = self._finish(wave, sample_rate, request, paste)
        mel01 = (mel[:, 0] + 1) / 2
        if save_root is not None:
            _write_clips(mel01, wave, sample_rate, _numbered_stems(save_root, mel01.shape[0]))
        return mel01, wave, tokens

    def _inpaint_tokens(self, tokens, keep, text, keep_mode, truncation_rate, caption_ids, seed, guidance_scale=None,
                        negative_text=None, purity_steps=None, purity_weight=0.0, tracks=None):
        """DALLE.inpaint_content at this call's truncation rate (_truncation); text None: the captions are the tracks'."""
        batch = dict(self._batch(text, caption_ids, seed, negative_text), content_token=tokens)
        with self._truncation(truncation_rate, forward=True):
            out = self.model.inpaint_content(batch=batch, keep_mask=keep, keep_mode=keep_mode, guidance_scale=guidance_scale,
                                             **({} if tracks is None else {"tracks": tracks}),
                                             sample_type=_sample_type(truncation_rate, False, purity_steps, purity_weight))
        return out["content_token"]

    @torch.no_grad()
    def inpaint_audio(self, audio, text, spans, keep_mode="clamp", truncation_rate=0.85, save_root=None, audio_rate=None,
                      caption_ids=None, seed=None, sample_rate=None, guidance_scale=None, negative_text=None, purity_steps=None,
                      purity_weight=0.0, *, level=None, keep_original=None, fade_seconds=FADE_SECONDS, match_gain=True):
        """Regenerate time spans of given recordings under a caption and keep the rest: audio / audio_rate / text as in
        generate_sample_from_audio; spans = the (t0, t1) seconds to regenerate, shared or one list per clip
        (spans_to_keep_mask: whole grid columns of 4096 samples at 22 050 Hz).  The recording is encoded to its 5 x 53 tokens,
        the tokens outside the spans are held through the whole reverse chain (keep_mode "clamp": clean; "renoise": following
        the forward process, per-caption in-kernel noise) and the spans are generated from [MASK] with them as context.
        caption_ids / seed / sample_rate / guidance_scale / negative_text / purity_steps / purity_weight as in
        generate_sample_with_condition (a purity chain holds positions clean: keep_mode "clamp" only).  Returns
        (mel01, wave or None, tokens) and writes the files generate_sample_from_audio writes.
        inpaint_scene regenerates the spans under a scene (caption tracks) instead of one caption.

        What is kept is the TOKENS: exact.  By default (keep_original=None) the returned audio is the codec's and the vocoder's
        rendering everywhere -- the held region is not the input's samples (the decoder's lowest level attends over all 265
        positions).  keep_original= (keyword-only, on the four drivers that hold a recording; paste_plan) puts the recording
        itself back outside the spans:
          "mel":   the recording's own content image (melspec.mel_image_from_audio) replaces the decoder's mel in the kept
                   columns, cross-faded linearly into it over fade_seconds inside the regenerated columns; the vocoder renders
                   the pasted mel, and the returned mel01 is the pasted mel.  The waveform is the vocoder's everywhere.
          "audio": all of "mel", and the recording's own samples -- at the output rate; a recording already at that rate is not
                   resampled -- replace the vocoder's in the kept columns: bit-equal to the input at sample n + RECORDING_OFFSET
                   (scaled to the rate; recording_offset), with an equal-power cross-fade of fade_seconds inside the regenerated
                   columns and, under match_gain=True, one gain per clip on the rendering, sqrt of the ratio of the two signals'
                   energies over the kept region, clamped to [1/4, 4].  Needs a vocoder (ValueError without).
        fade_seconds (default 1024 / 22050, >= 0; 0: a hard cut) and match_gain apply only with keep_original.  Tokens are
        never affected; the order of the tail is vocoder -> sample_rate -> paste -> level.  The alignment is a definition taken
        from the code's two front ends (RECORDING_OFFSET), not a measurement on a trained vocoder; there is no phase alignment
        of the rendering to the recording and no limiter.
        level= as in generate_sample_with_condition; "match": the result is brought to the integrated loudness of the
        recording, measured at the recording's own rate and length."""
        request = _request(self, level, (audio, audio_rate), keep_original, fade_seconds, match_gain)
        content = self.model.prepare_content({"audio": audio, "audio_rate": audio_rate})
        known = content["content_token"]
        keep = spans_to_keep_mask(spans, known.shape[0], known.device)
        tokens = self._inpaint_tokens(known, keep, text, keep_mode, truncation_rate, caption_ids, seed, guidance_scale,
                                      negative_text, purity_steps, purity_weight)
        return self._render(request, tokens, content["content_quant"].shape, save_root, sample_rate,
                            self._paste_plan(request, "inpaint_audio", known.shape[0], spans=spans, sample_rate=sample_rate))

    @torch.no_grad()
    def inpaint_scene(self, audio, tracks, spans, scale=3.0, keep_mode="clamp", truncation_rate=0.85, save_root=None,
                      audio_rate=None, caption_ids=None, seed=None, sample_rate=None, negative_text=None,
                      *, level=None, keep_original=None, fade_seconds=FADE_SECONDS, match_gain=True):
        """inpaint_audio under a scene instead of one caption: the spans are regenerated under `tracks` -- caption tracks as
        in generate_scene, [(text, t0, t1[, scale]), ...] in the clip's own seconds, one scene or one per clip; a track that
        names no scale gets `scale` -- and the rest of the recording is kept, as tokens, exactly (keep_original= as in
        inpaint_audio: also as its own mel, or its own samples).  The other arguments and the return are inpaint_audio's.  (A method of its own: inpaint_audio's keywords are what they were.)"""
        request = _request(self, level, (audio, audio_rate), keep_original, fade_seconds, match_gain)
        content = self.model.prepare_content({"audio": audio, "audio_rate": audio_rate})
        known = content["content_token"]
        keep = spans_to_keep_mask(spans, known.shape[0], known.device)
        tokens = self._inpaint_tokens(known, keep, None, keep_mode, truncation_rate, caption_ids, seed, None, negative_text,
                                      tracks=self._scene(tracks, GRID_COLS, known.shape[0], scale))
        return self._render(request, tokens, content["content_quant"].shape, save_root, sample_rate,
                            self._paste_plan(request, "inpaint_scene", known.shape[0], spans=spans, sample_rate=sample_rate))

    @torch.no_grad()
    def continue_audio(self, audio, text, keep_seconds, keep_mode="clamp", truncation_rate=0.85, save_root=None,
                       audio_rate=None, caption_ids=None, seed=None, sample_rate=None, guidance_scale=None, negative_text=None,
                       purity_steps=None, purity_weight=0.0, *, level=None, keep_original=None, fade_seconds=FADE_SECONDS,
                       match_gain=True):
        """Generate the clip that follows given recordings: the last ceil(keep_seconds 22050 / 4096) token columns of the
        recording become the first columns of a new 10-s clip (a shift by 5 (53 - n) tokens), held, and the remaining columns
        are generated under `text`.  Arguments and return as inpaint_audio.  By default the new clip's head is the codec's
        rendering of the kept tail (exact tokens, not the input's samples); keep_original="mel" / "audio" (inpaint_audio) makes
        it the recording's own mel frames from 16 (53 - n) on / its own samples from 4096 (53 - n) + RECORDING_OFFSET on (at
        22 050 Hz; scaled and rounded once at another output rate).  This returns the NEW clip only; extend_audio returns the
        recording and what follows it as one clip, joined in the mel domain."""
        request = _request(self, level, (audio, audio_rate), keep_original, fade_seconds, match_gain)
        content = self.model.prepare_content({"audio": audio, "audio_rate": audio_rate})
        known, keep = continuation_tokens(content["content_token"], continuation_columns(keep_seconds))
        tokens = self._inpaint_tokens(known, keep, text, keep_mode, truncation_rate, caption_ids, seed, guidance_scale,
                                      negative_text, purity_steps, purity_weight)
        return self._render(request, tokens, content["content_quant"].shape, save_root, sample_rate,
                            self._paste_plan(request, "continue_audio", known.shape[0], keep_seconds=keep_seconds,
                                             sample_rate=sample_rate))

    def _long_tokens(self, text, windows, overlap_cols, keep_mode, sample_type, caption_ids, seed, guidance_scale, negative_text,
                     start_token=None, tracks=None, joint=False, ring=False):
        """DALLE.generate_long_content under this call's caption / noise keywords and sample type (the model saves and restores
        its own); text None: the captions are the tracks'."""
        kw = {} if tracks is None else {"tracks": tracks}       # (without tracks: the call as it always was)
        if joint:
            kw.update(joint=True, ring=ring)                    # (likewise)
        return self.model.generate_long_content(batch=self._batch(text, caption_ids, seed, negative_text), windows=windows,
                                                overlap_cols=overlap_cols, keep_mode=keep_mode, sample_type=sample_type,
                                                guidance_scale=guidance_scale, start_token=start_token, **kw)

    VOCODER_CHUNK_FRAMES = 64 * 848       # mel frames per vocoder call of a long clip: the largest call the benchmarks run

    def _vocode_long(self, mel):
        """ONE vocoder pass per clip over its whole stitched mel f32[B, 80, F] -> f32[B, 1, 256 F] (None without a vocoder).
        Clips go through the vocoder in batch chunks of at most VOCODER_CHUNK_FRAMES mel frames; a clip is never split."""
        if self.vocoder is None:
            return None
        step = max(1, self.VOCODER_CHUNK_FRAMES // mel.shape[2])
        return torch.cat([self.vocoder(mel[i:i + step], scale=0.5, shift=0.5) for i in range(0, mel.shape[0], step)], 0)

    def _render_long(self, request, out, windows, overlap_cols, samples, save_root, sample_rate, paste=None):
        """window mels -> ds_mel_stitch (codec domain) (-> the recording's mel pasted: paste = a paste_plan; its samples
        pasted in _finish) -> the vocoder (_vocode_long) -> both cut to `samples` (the vocoder's reflection at the far end lies
        past the cut) -> sample_rate -> paste -> level, as the driver call's request says (_finish), files."""
        from . import audio
        win = out["content"]                                          # [B W, 1, 80, 848], clip-major: index b W + w
        B = win.shape[0] // windows
        mel = audio.stitch_mel(win.reshape(B, windows, win.shape[2], win.shape[3]), (GRID_COLS - overlap_cols) * COLUMN_FRAMES)
        mel = self._paste_mel(mel, paste)
        wave = self._vocode_long(mel)
        if wave is not None:
            wave = self._finish(wave[:, :, :samples].contiguous(), sample_rate, request, paste)
        mel01 = ((mel + 1) / 2)[:, :, :-(-samples // 256)].contiguous()
        if save_root is not None:
            _write_clips(mel01, wave, sample_rate, _numbered_stems(save_root, B))
        return mel01, wave, out["content_token"]

    @torch.no_grad()
    def generate_long(self, text, seconds, overlap_seconds=2.4, truncation_rate=0.85, keep_mode="clamp", caption_ids=None,
                      seed=None, sample_rate=None, guidance_scale=None, negative_text=None, save_root=None, purity_steps=None,
                      purity_weight=0.0, *, joint=False, level=None):
        """Captions -> clips of `seconds` (up to 16 windows, about two minutes): (mel01 f32[B, 80, ceil(samples / 256)], wave
        f32[B, 1, samples] -- None without a vocoder --, tokens i64[B, W, 265]), samples = round(seconds 22050).  The clip is
        generated as W overlapping windows of one 5 x 53 grid each (long_plan): window 0 like generate_sample_with_condition
        with per-caption in-kernel noise, every later window by region-held sampling with the last ceil(overlap_seconds
        22050 / 4096) token columns of its predecessor held as its first columns (keep_mode as in inpaint_audio), under the
        same caption, seed and guidance, drawing as caption id + w 2^20 (caption_ids default 0 .. B-1, each below 2^20).  All
        windows are decoded in one batch; their mels are cross-faded over the shared frames on the device (audio.stitch_mel)
        and the vocoder renders the whole long mel at once, so the waveform has no seam of its own -- it reflects only at the
        clip's two ends, and the far end's reflection is cut away with the frames past `samples`.  sample_rate / save_root as
        in the other drivers; purity_steps / purity_weight: every window's chain is a purity-prior chain
        (generate_sample_with_condition; keep_mode "clamp" only).  seconds up to one grid (217 088 samples): W = 1, the same path without a held chain.

        joint=True (keyword-only, like level=) switches the TOKEN stage to joint-window sampling
        (DALLE.generate_long_content: one chain at batch B W on a shared canvas instead of W chains at batch B, every window
        seeing both neighbours); the rendering is unchanged.  purity_steps and keep_mode "renoise" are not built for it.

        The overlap is a design choice whose audible quality is unmeasured (long_plan); so is how joint clips sound."""
        request = _request(self, level)
        windows, n, _, samples = long_plan(seconds, overlap_seconds)
        out = self._long_tokens(text, windows, n, keep_mode, _sample_type(truncation_rate, False, purity_steps, purity_weight),
                                caption_ids, seed, guidance_scale, negative_text, joint=joint)
        return self._render_long(request, out, windows, n, samples, save_root, sample_rate)

    def _loop_rendering(self, win, windows, overlap_cols, sample_rate=None):
        """The UNCUT rendering of a ring: the decoded windows win f32[B W, 1, 80, 848] (clip-major) stitched as
        [w_{W-2}, w_{W-1}, w_0 .. w_{W-1}, w_0, w_1] (indices mod W; audio.stitch_mel at hop 16 h frames) -> (mel f32[B, 80,
        848 + (W + 3) 16 h] in the codec's [-1, 1], wave f32[B, 1, .] at sample_rate -- the vocoder over the whole stitched mel,
        resampled as a whole -- or None without a vocoder).  The ring's frame f is stitched frame 2 16 h + f; the stitched mel
        is the ring's periodic continuation from frame 16 n (the first window's head has no predecessor to blend with) to frame
        (W + 4) 16 h (the last window's tail has no successor)."""
        from . import audio
        B = win.shape[0] // windows
        order = [(w - LOOP_LEAD_HOPS) % windows for w in range(windows + 2 * LOOP_LEAD_HOPS)]
        mel = audio.stitch_mel(win.reshape(B, windows, win.shape[2], win.shape[3])[:, order].contiguous(),
                               (GRID_COLS - overlap_cols) * COLUMN_FRAMES)
        return mel, self._at_rate(self._vocode_long(mel), sample_rate)

    @torch.no_grad()
    def generate_loop(self, text, seconds, overlap_seconds=2.4, truncation_rate=0.85, fast=False, caption_ids=None, seed=None,
                      guidance_scale=None, negative_text=None, sample_rate=None, save_root=None, *, level=None):
        """Captions -> seamless loops of about `seconds` (ambiences, engines, room tone): (mel01 f32[B, 80, 16 C], wave
        f32[B, 1, 4096 C rate / 22050] -- None without a vocoder --, tokens i64[B, W, 265], seconds_made).  loop_plan picks
        W >= 2 windows and the ring of C = W h whole columns (the length snaps UP to a multiple of the hop h = 53 - n columns;
        seconds_made = 4096 C / 22050 says what was made).  The tokens are ONE joint chain on the canvas closed into a ring
        (DALLE.generate_long_content(joint=True, ring=True)): window W - 1 flows into window 0 as every window flows into
        the next.  Rendering: the W decoded windows are stitched as [w_{W-2}, w_{W-1}, w_0 .. w_{W-1}, w_0, w_1] (indices
        mod W; audio.stitch_mel, hop 16 h frames), so the ring's frame f is stitched frame 2 16 h + f and the frames ahead of
        and behind the ring are the ring's own content, one hop of it fully blended on either side; the vocoder renders the
        WHOLE stitched mel and the waveform is cut to the ring's samples.  A convolutional vocoder on a periodic mel gives a
        periodic waveform wherever its receptive field stays inside the periodic part (DESIGN.md section 4 derives the field),
        so the loop's last sample flows into its first as any sample flows into the next: no cross-fade in the audio domain.
        sample_rate: the uncut rendering is resampled and cut at the converted offsets, which must be whole samples
        (loop_cut: 44 100 and 11 025 always are; otherwise ValueError -- no approximate loop point is emitted).
        level=: the static strategies measure and scale the one period; with limit it raises (a periodic gain curve is not
        built).  fast / caption_ids / seed / guidance_scale / negative_text / save_root as in the other drivers.

        How loops SOUND is unmeasured: no trained checkpoint has been available to this project."""
        request = _request(self, level)
        if request.level is not None and request.level.get("limit"):
            raise ValueError("generate_loop: level= with limit is not built for loops (the limiter's gain curve is not periodic)")
        windows, n, cols, samples = loop_plan(seconds, overlap_seconds)
        hop = GRID_COLS - n
        off, period = loop_cut(cols, hop, sample_rate)                 # the rate rule, before anything runs
        out = self._long_tokens(text, windows, n, "clamp", _sample_type(truncation_rate, fast), caption_ids, seed, guidance_scale,
                                negative_text, joint=True, ring=True)
        mel, wave = self._loop_rendering(out["content"], windows, n, sample_rate)
        lead = LOOP_LEAD_HOPS * hop * COLUMN_FRAMES
        if wave is not None:
            wave = self._level(wave[:, :, off:off + period].contiguous(), sample_rate, request)
        mel01 = ((mel + 1) / 2)[:, :, lead:lead + cols * COLUMN_FRAMES].contiguous()
        if save_root is not None:
            _write_clips(mel01, wave, sample_rate, _numbered_stems(save_root, mel01.shape[0]))
        return mel01, wave, out["content_token"], samples / VOCODER_RATE

    SCENE_SCALE = 3.0     # generate_scene's default track weight: the scale the guidance tests run at; a design choice

    @staticmethod
    def _scene(tracks, total_cols=GRID_COLS, batch=None, scale=None):
        """tracks of generate_scene / inpaint_scene -> the dict DALLE's `tracks` keyword takes (None stays None); a track that
        names no scale gets `scale` (default SCENE_SCALE).  batch: the clips ONE scene is shared by; a list of scenes brings
        its own count and batch is not looked at."""
        if tracks is None:
            return None
        is_seq = lambda x: isinstance(x, (list, tuple))
        if len(tracks) > 0 and is_seq(tracks[0]) and len(tracks[0]) > 0 and is_seq(tracks[0][0]):      # a list of scenes
            batch = None
        scale = Diffsound.SCENE_SCALE if scale is None else float(scale)
        fill = lambda t: tuple(t) + (scale,) if is_seq(t) and len(t) == 3 and isinstance(t[0], str) else t
        tracks = [fill(t) if not (is_seq(t) and t and is_seq(t[0])) else [fill(q) for q in t] for t in tracks]
        text, weight = track_weights(tracks, total_cols, batch)
        return {"text": text, "weight": weight}

    @torch.no_grad()
    def generate_scene(self, tracks, seconds=None, scale=3.0, overlap_seconds=2.4, truncation_rate=0.85, keep_mode="clamp",
                       fast=False, caption_ids=None, seed=None, negative_text=None, sample_rate=None, save_root=None,
                       *, level=None):
        """A scene instead of one caption: tracks = [(text, t0, t1[, scale]), ...] in seconds (track_weights: t1 None = to the
        end; at most 4 tracks), one scene or a list of B scenes -> what generate_long returns: (mel01, wave or None, tokens
        i64[B, W, 265]).  Every sampler step evaluates the denoiser under each track's caption and under the null condition
        (the empty caption, or negative_text) and samples each grid position from
            log p_null + sum_i w_i(pos) (log p_i - log p_null),   renormalised
        (csrc/sampler.hip SampleCompose) -- the conjunction of Liu et al. 2022 with weights that vary over the token grid;
        w_i is the track's scale inside its span, 0 outside, proportional in an edge column.  scale: the default for tracks
        that name none (3.0: the scale the guidance tests run at -- a design choice, not a measured optimum).  seconds None
        or at most one grid (217 088 samples): one window; longer: the windows of generate_long (long_plan, overlap_seconds,
        keep_mode), each under the slice of the weights over its own columns.  fast / caption_ids / seed / sample_rate /
        save_root as in the other drivers; a scene is repeated by calling again under other caption_ids.

        No trained checkpoint has been available to this project: what scenes SOUND like, and whether event order and
        placement improve over one caption, is unmeasured."""
        request = _request(self, level)
        windows, n, total, samples = long_plan(CLIP_SAMPLES / VOCODER_RATE if seconds is None else seconds, overlap_seconds)
        out = self._long_tokens(None, windows, n, keep_mode, _sample_type(truncation_rate, fast), caption_ids, seed, None,
                                negative_text, tracks=self._scene(tracks, total, 1, scale))
        return self._render_long(request, out, windows, n, samples, save_root, sample_rate)

    @torch.no_grad()
    def extend_audio(self, audio, text, seconds, overlap_seconds=2.4, truncation_rate=0.85, keep_mode="clamp", caption_ids=None,
                     seed=None, sample_rate=None, guidance_scale=None, negative_text=None, save_root=None, audio_rate=None,
                     purity_steps=None, purity_weight=0.0, *, joint=False, level=None, keep_original=None,
                     fade_seconds=FADE_SECONDS, match_gain=True):
        """Extend given recordings to `seconds` in total (more than one grid, 217 088 / 22 050 s): audio / audio_rate as in
        continue_audio; the recording is encoded to its 5 x 53 tokens, which become window 0, and the windows after it are
        generated under `text` as in generate_long.  Returns what generate_long returns; tokens[:, 0] are the recording's.
        By default the head of the result is the codec's and the vocoder's rendering of the recording's tokens, not the
        input's samples; keep_original="mel" / "audio" (inpaint_audio) keeps columns 0 .. 52 of the long clip as the recording's
        own mel / samples, with the cross-fade inside column 53.  joint=True (keyword-only, as on generate_long): the windows after the recording are ONE joint
        chain with the recording's grid held as the canvas head (generate_long); tokens[:, 0] stay the recording's."""
        request = _request(self, level, (audio, audio_rate), keep_original, fade_seconds, match_gain)
        windows, n, _, samples = long_plan(seconds, overlap_seconds)
        if windows < 2:
            raise ValueError("extend_audio: seconds must exceed one grid (%d samples at %d Hz), got %r"
                             % (CLIP_SAMPLES, VOCODER_RATE, seconds))
        start = self.model.prepare_content({"audio": audio, "audio_rate": audio_rate})["content_token"]
        out = self._long_tokens(text, windows, n, keep_mode, _sample_type(truncation_rate, False, purity_steps, purity_weight),
                                caption_ids, seed, guidance_scale, negative_text, start_token=start, joint=joint)
        return self._render_long(request, out, windows, n, samples, save_root, sample_rate,
                                 self._paste_plan(request, "extend_audio", start.shape[0], seconds=seconds, sample_rate=sample_rate))

    # ---- likelihood scoring (DiffusionTransformer.score_tokens) -------------------------------------------
    @torch.no_grad()
    def score_audio(self, audio, text, audio_rate=None, timesteps=None, draws=1, caption_ids=None, seed=None):
        """How well recordings fit captions: audio / audio_rate as in generate_sample_from_audio (encoded to their 5 x 53
        tokens), text = one caption per recording (strings, token ids or embeddings).  Returns DALLE.score_content's
        {'nats' f64[B] -- the variational bound, lower = better fit --, 'bits_per_token', 'terms'}; timesteps / draws /
        caption_ids / seed as in DiffusionTransformer.score_tokens."""
        batch = dict(self._batch(text, caption_ids, seed), audio=audio, audio_rate=audio_rate)
        return self.model.score_content(batch, timesteps=timesteps, draws=draws)

    # ---- two waveforms side by side (audio.compare) -------------------------------------------------------
    @staticmethod
    def _rows_at_22k(item, rate, device):
        """recordings as the drivers take them (or a driver's own f32[B,1,T] output) -> f32[B, T'] at 22 050 Hz on the device, rows
        zero-extended to the longest"""
        if torch.is_tensor(item) and item.dim() == 3 and item.shape[1] == 1:
            item = item[:, 0]
        rows, _ = recording_at_rate(item, rate, VOCODER_RATE, device)
        return rows.float().contiguous()

    @torch.no_grad()
    def compare_audio(self, a, b, audio_rate=None, **kw):
        """b, the waveforms under test, against their references a: each a device tensor f32[B, T] (or a driver's f32[B, 1, T]),
        host arrays or `.wav` paths, as the other drivers take recordings; audio_rate the sample rate of both (one or one per clip,
        None = 22 050 Hz / the files' own; two tensors at different rates: audio.resample one first).  Both are brought to 22 050 Hz on the
        device (audio.resample; a clip already there is not touched) and handed to audio.compare with the remaining keywords
        (max_lag, lag, region -- in samples at 22 050 Hz) -> its dict of device tensors: lag, rho, si_sdr_db, snr_db, sc,
        logmag, mel_l1.  Rows of different length are zero-extended to the longest: the region is one for the whole batch
        (per-row lengths are not built), so name a region that every row fills.  What these numbers say about a trained model
        is unmeasured; on seeded weights they measure the code."""
        from . import audio
        if "rate" in kw:
            raise ValueError("compare_audio compares at 22 050 Hz: give the inputs' rate as audio_rate")
        device = next(self.model.parameters()).device
        rows_a = self._rows_at_22k(a, audio_rate, device)
        rows_b = self._rows_at_22k(b, audio_rate, device)
        return audio.compare(rows_a, rows_b, rate=VOCODER_RATE, **kw)

    @torch.no_grad()
    def round_trip(self, audio, audio_rate=None, max_lag=2048):
        """What the codec and the vocoder do to a recording: audio / audio_rate as in generate_sample_from_audio -> its 5 x 53
        tokens (prepare_content) -> decode -> vocoder, nothing sampled -> (mel01 f32[B,80,848], wave f32[B,1,217088], tokens,
        report).  report = audio.compare of the rendering against the recording at 22 050 Hz, the lag searched over
        RECORDING_OFFSET +- max_lag (the search is centred on the alignment the code defines, so it lies inside for any
        max_lag) over the default region; report['lag'] is the full lag, RECORDING_OFFSET where the definition holds.  Needs a
        vocoder (ValueError without).  How lossy the round trip is with TRAINED weights is unmeasured: no checkpoint is in
        the tree; on seeded weights the report measures the code, not a model."""
        from . import audio as A
        if self.vocoder is None:
            raise ValueError("round_trip needs a vocoder: there is no waveform to compare")
        content = self.model.prepare_content({"audio": audio, "audio_rate": audio_rate})
        mel01, wave, tokens = self._render(_Request(None, None, None), content["content_token"], content["content_quant"].shape)
        rec = self._rows_at_22k(audio, audio_rate, wave.device)
        if rec.shape[1] <= RECORDING_OFFSET:
            raise ValueError("the recording holds %d samples at 22 050 Hz: too short to compare" % rec.shape[1])
        report = A.compare(rec[:, RECORDING_OFFSET:].contiguous(), wave[:, 0].contiguous(), max_lag=max_lag, rate=VOCODER_RATE)
        report["lag"] = report["lag"] + RECORDING_OFFSET
        return mel01, wave, tokens, report

    @torch.no_grad()
    def generate_best_of(self, cond, n, score_timesteps=None, truncation_rate=0.85, fast=False, caption_ids=None, seed=None,
                         sample_rate=None, guidance_scale=None, negative_text=None, purity_steps=None, purity_weight=0.0,
                         score_draws=1, *, level=None):
        """Best-of-n generation: n candidates per caption, the one that fits its caption best is rendered.  cond and the
        keywords as in generate_sample_with_condition, whose `replicate` is n here; the candidates are its tokens at
        replicate = n with per-caption in-kernel noise (caption_ids default 0 .. B-1; replicate r of caption i draws as id
        ids[i] + r 2^24).  Candidate r of caption i is scored by DiffusionTransformer.score_tokens under the caption, on the
        caption's own id ids[i] and `seed` -- all n candidates of a caption see the same forward-diffusion uniforms --
        with score_timesteps / score_draws as its timesteps / draws (None: the full bound, T forwards per candidate).  The
        lowest score wins, ties go to the lowest replicate; only the winners are decoded and vocoded.
        Returns (mel01 f32[B,80,848], wave or None, tokens i64[B,265], scores f64[B, n] in nats)."""
        request = _request(self, level)
        n = int(n)
        if n < 1:
            raise ValueError("generate_best_of needs at least one candidate per caption, got n = %r" % (n,))
        model = self.model
        condition = model.prepare_condition(batch=self._batch(cond))
        B = next(v.shape[0] for v in condition.values() if torch.is_tensor(v))
        ids = torch.arange(B) if caption_ids is None else torch.as_tensor(caption_ids, dtype=torch.long).reshape(-1)
        batch = self._batch(cond, ids, seed, negative_text)
        sample_type = _sample_type(truncation_rate, fast, purity_steps, purity_weight)
        model.eval()
        replicated = {k: (torch.cat([v for _ in range(n)], dim=0) if torch.is_tensor(v) else v) for k, v in condition.items()}
        tokens = model._run_chain(batch, replicated, model._free_keywords(0, 1.0, False, sample_type), n, sample_type,
                                  guidance_scale)                                   # [n B, 265], replicate-major
        model.train()
        kw = {} if seed is None else {"seed": int(seed)}
        scores = model.transformer.score_tokens(tokens, condition_token=replicated.get("condition_token"),
                                                condition_embed=replicated.get("condition_embed_token"),
                                                timesteps=score_timesteps, draws=score_draws, caption_ids=ids.repeat(n), **kw)
        scores = scores.view(n, B).t().contiguous()                                # [B, n]
        import numpy as np
        best = torch.from_numpy(np.argmin(scores.cpu().numpy(), axis=1)).to(tokens.device)   # first minimum: the lowest replicate
        winners = tokens.view(n, B, -1)[best, torch.arange(B, device=tokens.device)].contiguous()
        mel01, wave, winners = self._render(request, winners, (B, 256, 5, 53), None, sample_rate)
        return mel01, wave, winners, scores

    @torch.no_grad()
    def inference_generate_sample_with_condition(self, text, truncation_rate, save_root, batch_size, fast=False,
                                                 guidance_scale=None, negative_text=None, purity_steps=None, purity_weight=0.0,
                                                 *, level=None):
        """The reference's single-caption driver, same signature and behaviour (generate_samples_batch.py:89-123):
        ONE caption `text`, sampled `replicate = 10` times (hard-coded there, :111; `batch_size` is accepted and
        unused, as in the reference), results written under `save_root/str(text)/` as `000000`, `000001`, ...
        The reference writes `.png` through an image-era uint8 cast that cannot represent a [-1,1] spectrogram
        (`Image.fromarray` rejects the [80,848,1] array); this drop-in writes what the batch driver writes instead:
        `{n:06d}.npy` (mel in [0,1], f32[80,848]) and, with a vocoder, `{n:06d}.wav` (22 050 Hz PCM_24).  Returns the paths."""
        _request(self, level)                     # a bad level raises here, before a directory is made; the inner driver applies it
        replicate = 10
        stems = _numbered_stems(os.path.join(save_root, str(text)), replicate)
        mel01, wave, _ = self.generate_sample_with_condition([text], truncation_rate, replicate=replicate, fast=fast,
                                                             guidance_scale=guidance_scale, negative_text=negative_text,
                                                             purity_steps=purity_steps, purity_weight=purity_weight, level=level)
        return _write_clips(mel01, wave, None, stems)

    @staticmethod
    def read_tsv(val_path):
        """file_name,caption CSV -> {file_name: [captions]} (generate_samples_batch.py:125-141)."""
        import csv
        caps = {}
        with open(val_path, newline="") as f:
            for row in csv.DictReader(f):
                caps.setdefault(row["file_name"], []).append(row["caption"])
        return caps

    @torch.no_grad()
    def generate_sample(self, val_path, truncation_rate, save_root, fast=False, replicate=2, sample_rate=None,
                        guidance_scale=None, purity_steps=None, purity_weight=0.0, *, level=None):
        """The reference's file-writing driver (generate_samples_batch.py:143-187): per audio file, all of
        its captions x `replicate` are sampled in one batch; every sample is written as
        `{base}_mel_sample_{i}.npy` (mel in [0,1], f32[80,848]) and -- if there is a vocoder (:183) --
        `{base}_mel_sample_{i}.wav` (22 050 Hz or `sample_rate`, PCM_24).  Unlike the reference the vocoder runs on the whole
        batch at once."""
        _request(self, level)                     # a bad level raises here, before a directory is made; the inner driver applies it
        os.makedirs(save_root, exist_ok=True)
        written = []
        n_seen = 0                       # running caption index over the whole table = the global caption id
        philox = self.model.transformer.rng_mode == "philox"
        for key, captions in self.read_tsv(val_path).items():
            base = os.path.join(save_root, key.split(".")[0] + "_mel_sample_")
            ids = list(range(n_seen, n_seen + len(captions))) if philox else None
            n_seen += len(captions)
            mel01, wave, _ = self.generate_sample_with_condition(list(captions), truncation_rate, replicate, fast=fast,
                                                                 caption_ids=ids, sample_rate=sample_rate,
                                                                 guidance_scale=guidance_scale, purity_steps=purity_steps,
                                                                 purity_weight=purity_weight, level=level)
            written += _write_clips(mel01, wave, sample_rate, [base + str(i) for i in range(mel01.shape[0])])
        return written


def write_wav_pcm24(path, samples, rate):
    """Mono float waveform in [-1, 1] -> RIFF/WAVE with 24-bit little-endian PCM, as
    soundfile.write(path, x, rate, 'PCM_24') produces (generate_samples_batch.py:186)."""
    import struct

    import numpy as np
    x = np.asarray(samples, dtype=np.float64).reshape(-1)
    q = np.clip(np.rint(x * 8388608.0), -8388608, 8388607).astype("<i4")   # libsndfile: scale 2^23, clip
    raw = q.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, rate, rate * 3, 3, 24))
        f.write(b"data" + struct.pack("<I", len(raw)))
        f.write(raw)
