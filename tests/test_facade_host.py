"""The Diffsound drivers' plumbing, on the host: what each of the twelve drivers hands to the model, which steps of the shared tail
(vocoder -> sample_rate -> paste -> level) run, in what order, how often and with what arguments, and which files are written.
The model, the vocoder and every device helper are recorders that return zero-filled tensors of the right shapes, so no kernel is
launched.  Each step of the tail adds its own mark to what flows through it (vocoder 1 + the mel's value, resample +10, the
waveform paste +100, level +1000, the mel paste +0.5), so the returned values say that every step ran once on the result of the
step before it.  Expected paste arguments come from pipeline.paste_plan itself, never from a second run of a driver."""
import os

import pytest
import torch

from text_to_sound_synthesis_amd import audio as audio_mod
from text_to_sound_synthesis_amd import pipeline
from text_to_sound_synthesis_amd.modeling import melspec

NO_GRAD = True
CLIP = 217088
TAIL = ("vocoder", "resample", "paste_mel", "paste_audio", "level")
SPANS = [(2.0, 4.0)]
TRACKS = [("rain", 0.0, None), ("thunder", 2.0, 5.0, 1.5)]
RATES = [None, 48000]


class StubTransformer:
    def __init__(self, rig):
        self.rig = rig
        self.truncation_r, self.truncation_k, self.repeat_rate, self.rng_mode = 0.7, 5, 0.25, "torch"

    def state(self):
        return self.truncation_r, self.truncation_k, self.repeat_rate

    def sample(self, **kw):
        self.rig.model_call("sample", kw)
        return {"content_token": torch.zeros(kw["content_token"].shape, dtype=torch.long)}

    def score_tokens(self, tokens, **kw):
        self.rig.model_call("score_tokens", dict(kw, tokens=tokens))
        return -torch.arange(tokens.shape[0], dtype=torch.float64)          # the last replicate of every caption wins


class StubModel:
    def __init__(self, rig):
        self.rig, self.truncation_forward, self.transformer = rig, False, StubTransformer(rig)

    def state(self):
        return self.transformer.state() + (self.truncation_forward,)

    def eval(self):
        return self

    def train(self):
        return self

    @staticmethod
    def _rows(batch):
        for k in ("text", "condition_token", "condition_embed_token", "content_token", "caption_ids"):
            if k in batch:
                return len(batch[k])
        return 1

    def generate_content(self, **kw):
        self.rig.model_call("generate_content", kw)
        n = self._rows(kw["batch"]) * kw["replicate"]
        return {"content": torch.zeros(n, 1, 80, 848), "content_token": torch.zeros(n, 265, dtype=torch.long)}

    def inpaint_content(self, **kw):
        self.rig.model_call("inpaint_content", kw)
        return {"content_token": torch.zeros(kw["batch"]["content_token"].shape, dtype=torch.long)}

    def generate_long_content(self, **kw):
        self.rig.model_call("generate_long_content", kw)
        start, trk = kw.get("start_token"), kw.get("tracks")
        B = start.shape[0] if start is not None else trk["weight"].shape[0] if trk is not None else self._rows(kw["batch"])
        W = kw["windows"]
        return {"content": torch.zeros(B * W, 1, 80, 848), "content_token": torch.zeros(B, W, 265, dtype=torch.long)}

    def prepare_content(self, batch):
        self.rig.model_call("prepare_content", {"batch": batch})
        B = batch["audio"].shape[0]
        return {"content_token": torch.zeros(B, 265, dtype=torch.long), "content_quant": torch.zeros(B, 256, 5, 53)}

    def prepare_condition(self, batch):
        self.rig.model_call("prepare_condition", {"batch": dict(batch)})
        return {"condition_embed_token": torch.zeros(self._rows(batch), 3, 4)}

    def decode_to_img(self, tokens, zshape):
        self.rig.model_call("decode_to_img", {"tokens": tokens, "zshape": tuple(zshape)})
        return torch.zeros(tokens.shape[0], 1, 80, 848)

    def _free_keywords(self, *args):
        self.rig.model_call("_free_keywords", {"args": args})
        return {"free": args}

    def _run_chain(self, batch, condition, keywords, replicate, sample_type, guidance_scale):
        self.rig.model_call("_run_chain", dict(batch=batch, condition=condition, keywords=keywords, replicate=replicate,
                                               sample_type=sample_type, guidance_scale=guidance_scale))
        n = condition["condition_embed_token"].shape[0]
        return torch.arange(n)[:, None].expand(n, 265).contiguous()          # row i is all i: replicate-major candidates


class Rig:
    """a Diffsound made with object.__new__ over the stubs + the ordered log of everything that was called"""

    def __init__(self, monkeypatch, vocoder=True):
        self.log, self.fail = [], None
        self.ds = object.__new__(pipeline.Diffsound)
        self.ds.model = StubModel(self)
        self.ds.vocoder = self.vocoder if vocoder else None
        self.lufs = torch.zeros(1, dtype=torch.float64)
        monkeypatch.setattr(audio_mod, "level", self.level)
        monkeypatch.setattr(audio_mod, "paste", self.paste)
        monkeypatch.setattr(audio_mod, "resample", self.resample)
        monkeypatch.setattr(audio_mod, "stitch_mel", self.stitch_mel)
        monkeypatch.setattr(melspec, "mel_image_from_audio", self.mel_image_from_audio)
        monkeypatch.setattr(pipeline, "recording_at_rate", self.recording_at_rate)
        monkeypatch.setattr(pipeline, "recording_loudness", self.recording_loudness)
        monkeypatch.setattr(pipeline, "write_wav_pcm24", self.write_wav)

    # -- the log
    def model_call(self, name, kw):
        self.log.append((name, dict(kw, state=self.ds.model.state())))
        if self.fail == name:
            raise RuntimeError("the stub's " + name + " fails")

    def calls(self, name):
        return [kw for n, kw in self.log if n == name]

    def one(self, name):
        got = self.calls(name)
        assert len(got) == 1, (name, len(got))
        return got[0]

    def tail(self):
        return [n for n, _ in self.log if n in TAIL]

    # -- the recorders
    def vocoder(self, mel, scale, shift):
        assert (scale, shift) == (0.5, 0.5) and mel.dim() == 3 and mel.shape[1] == 80
        self.log.append(("vocoder", {"shape": tuple(mel.shape)}))
        return torch.full((mel.shape[0], 1, 256 * mel.shape[2]), 1.0 + float(mel[0, 0, 0]))

    def resample(self, wave, src, dst, **kw):
        assert wave.dim() == 2 and not kw
        self.log.append(("resample", {"src": src, "dst": dst}))
        return torch.full((wave.shape[0], -(-wave.shape[1] * dst // src)), float(wave[0, 0]) + 10.0)

    def level(self, wave, rate, strategy, **kw):
        assert wave.dim() == 2
        self.log.append(("level", dict(kw, rate=rate, strategy=strategy, samples=wave.shape[1])))
        return wave + 1000.0, torch.ones(wave.shape[0])

    def paste(self, ren, rec, keep_cols, **kw):
        name = "paste_mel" if ren.dim() == 3 else "paste_audio"
        self.log.append((name, dict(kw, rec=rec, keep_cols=keep_cols)))
        return ren + (0.5 if ren.dim() == 3 else 100.0)

    def stitch_mel(self, win, hop, *args):
        assert not args and win.dim() == 4 and win.is_contiguous()
        self.log.append(("stitch_mel", {"windows": win.shape[1], "hop": hop}))
        return torch.zeros(win.shape[0], win.shape[2], win.shape[3] + (win.shape[1] - 1) * hop)

    def mel_image_from_audio(self, item, device, rate=None):
        self.log.append(("mel_image_from_audio", {"item": item, "rate": rate}))
        return torch.zeros(item.shape[0], 1, 80, 848)

    def recording_at_rate(self, item, rate, out_rate, device="cuda"):
        self.log.append(("recording_at_rate", {"item": item, "rate": rate, "out_rate": out_rate}))
        self.rec = torch.zeros(item.shape[0], 7)
        self.rec_len = torch.full((item.shape[0],), 7, dtype=torch.int32)
        return self.rec, self.rec_len

    def recording_loudness(self, item, rate=None, device="cuda"):
        self.log.append(("recording_loudness", {"item": item, "rate": rate}))
        return self.lufs

    def write_wav(self, path, samples, rate):
        self.log.append(("wav", {"path": path, "samples": len(samples), "value": float(samples[0]), "rate": rate}))


@pytest.fixture
def rig(monkeypatch):
    return Rig(monkeypatch)


def _recording(B=2):
    return torch.zeros(B, 1000)


def _tsv(tmp_path):
    path = tmp_path / "val.csv"
    path.write_text("file_name,caption\na.wav,a dog\na.wav,a cat\nb.wav,rain\n")
    return str(path)


# every driver: how it is called here (B = 2 wherever a batch is given) and what its tail and its files look like
#   takes: the recording's (audio, audio_rate) it takes, or None;  pastes / joint: whether it has those keywords
#   rate: whether it has sample_rate;  stitched: whether its mel is stitched from windows;  samples: the waveform at 22 050 Hz
DRIVERS = {
    "generate_sample_with_condition": dict(args=lambda c: ((["a", "b"], 0.8), dict(fast=10, caption_ids=[4, 5], seed=3)), samples=CLIP),
    "generate_sample_from_audio": dict(args=lambda c: ((c["audio"], ["a", "b"]), dict(truncation_rate=0.8, save_root=c["root"], audio_rate=32000)),
                                       takes=32000, rate=False, files="index", samples=CLIP),
    "generate_loop": dict(args=lambda c: ((["a", "b"], 15.0), dict(truncation_rate=0.8, fast=10, caption_ids=[4, 5], seed=3, save_root=c["root"])),
                          stitched=True, files="index", samples=120 * 4096, rates=[None, 44100]),
    "generate_scene": dict(args=lambda c: ((TRACKS, 15.0), dict(truncation_rate=0.8, fast=10, caption_ids=[4], seed=3, save_root=c["root"])),
                           stitched=True, files="index", samples=330750, B=1),
    "generate_best_of": dict(args=lambda c: ((["a", "b"], 3), dict(score_timesteps=2, truncation_rate=0.8, fast=10, seed=3, guidance_scale=2.0)),
                             samples=CLIP),
    "inference_generate_sample_with_condition": dict(args=lambda c: (("a dog", 0.8, c["root"], 4), dict(fast=10, guidance_scale=2.0)),
                                                     rate=False, files="caption", samples=CLIP, B=10),
    "generate_sample": dict(args=lambda c: ((c["tsv"], 0.8, c["root"]), dict(fast=10, replicate=2, guidance_scale=2.0)),
                            files="table", samples=CLIP),
    "inpaint_audio": dict(args=lambda c: ((c["audio"], ["a", "b"], SPANS), dict(truncation_rate=0.8, save_root=c["root"], audio_rate=32000,
                                                                                  caption_ids=[4, 5], seed=3, guidance_scale=2.0)),
                          takes=32000, pastes=dict(spans=SPANS), files="index", samples=CLIP),
    "inpaint_scene": dict(args=lambda c: ((c["audio"], TRACKS, SPANS), dict(truncation_rate=0.8, save_root=c["root"], audio_rate=32000,
                                                                             caption_ids=[4, 5], seed=3)),
                          takes=32000, pastes=dict(spans=SPANS), files="index", samples=CLIP),
    "continue_audio": dict(args=lambda c: ((c["audio"], ["a", "b"], 3.0), dict(truncation_rate=0.8, save_root=c["root"], audio_rate=32000,
                                                                                caption_ids=[4, 5], seed=3, guidance_scale=2.0)),
                           takes=32000, pastes=dict(keep_seconds=3.0), files="index", samples=CLIP),
    "generate_long": dict(args=lambda c: ((["a", "b"], 15.0), dict(truncation_rate=0.8, caption_ids=[4, 5], seed=3, guidance_scale=2.0,
                                                                   save_root=c["root"])),
                          joint=True, stitched=True, files="index", samples=330750),
    "extend_audio": dict(args=lambda c: ((c["audio"], ["a", "b"], 15.0), dict(truncation_rate=0.8, caption_ids=[4, 5], seed=3, guidance_scale=2.0,
                                                                               save_root=c["root"], audio_rate=32000)),
                         takes=32000, pastes=dict(seconds=15.0), joint=True, stitched=True, files="index", samples=330750),
}
assert len(DRIVERS) == 12


def _requests(d):
    """the keyword-only requests a driver is run under"""
    out = [{}, {"level": "peak"}]
    if d.get("takes"):
        out.append({"level": "match"})
    if d.get("pastes"):
        out += [{"keep_original": "mel"}, {"keep_original": "audio", "level": "rms"}]
    if d.get("joint"):
        out.append({"joint": True})
    return out


CASES = [(name, req, rate) for name, d in DRIVERS.items() for req in _requests(d)
         for rate in (d.get("rates", RATES) if d.get("rate", True) else [None])]


def _case_id(v):
    if isinstance(v, dict):
        return "-".join("%s=%s" % kv for kv in sorted(v.items())) or "plain"
    return str(v)


def _run(rig, name, req, rate, tmp_path, **more):
    d = DRIVERS[name]
    os.makedirs(str(tmp_path), exist_ok=True)
    ctx = {"audio": _recording(), "root": str(tmp_path / "out"), "tsv": _tsv(tmp_path)}
    args, kw = d["args"](ctx)
    if d.get("rate", True) and rate is not None:
        kw["sample_rate"] = rate
    before = rig.ds.model.state()
    out = getattr(rig.ds, name)(*args, **dict(kw, **req, **more))
    assert rig.ds.model.state() == before
    return ctx, out


@pytest.mark.parametrize("name,req,rate", CASES, ids=_case_id)
def test_tail_and_files(rig, name, req, rate, tmp_path):
    d = DRIVERS[name]
    ctx, out = _run(rig, name, req, rate, tmp_path)
    B, out_rate = d.get("B", 2), 22050 if rate is None else rate
    keep, level = req.get("keep_original"), req.get("level")
    batches = [4, 2] if name == "generate_sample" else [B]                   # generate_sample: one tail per file of the table

    # ---- which steps ran, in what order, how often
    want = (["paste_mel"] if keep else []) + ["vocoder"] + (["resample"] if rate else []) \
        + (["paste_audio"] if keep == "audio" else []) + (["level"] if level else [])
    assert rig.tail() == want * len(batches)
    assert len(rig.calls("stitch_mel")) == (1 if d.get("stitched") else 0)
    value = 1.0 + (0.5 if keep else 0.0) + (10.0 if rate else 0.0) + (100.0 if keep == "audio" else 0.0) + (1000.0 if level else 0.0)
    samples = d["samples"] if rate is None else -(-d["samples"] * rate // 22050)
    if name == "generate_loop" and rate:
        samples = d["samples"] * rate // 22050
    for r in rig.calls("resample"):
        assert (r["src"], r["dst"]) == (22050, rate)

    # ---- the returned tensors
    if d.get("files") not in ("caption", "table"):
        mel01, wave = out[0], out[1]
        assert tuple(wave.shape) == (B, 1, samples) and bool((wave == value).all())
        assert mel01.shape[0] == B and mel01.shape[1] == 80 and bool((mel01 == (0.75 if keep else 0.5)).all())
        assert mel01.shape[2] == (-(-d["samples"] // 256))
        assert out[2].dtype == torch.long

    # ---- what audio.level was given
    for n, lv in zip(batches, rig.calls("level")):
        assert lv["rate"] == out_rate and type(lv["rate"]) is int and lv["samples"] == samples
        assert lv["strategy"] == level and lv["target"] is None and lv["ceiling_db"] == -1.0 and lv["limit"] is None
        assert (lv["reference"] is rig.lufs) if level == "match" else (lv["reference"] is None)
    heard = rig.calls("recording_loudness")
    assert len(heard) == (1 if level == "match" else 0)
    for h in heard:
        assert h["item"] is ctx["audio"] and h["rate"] == d["takes"]

    # ---- what audio.paste was given
    if keep:
        plan = pipeline.paste_plan(name, keep, batch=B, sample_rate=rate, **d["pastes"])
        pm, image = rig.one("paste_mel"), rig.one("mel_image_from_audio")
        assert image["item"] is ctx["audio"] and image["rate"] == d["takes"]
        assert torch.equal(pm["keep_cols"], plan["keep_cols"]) and pm["keep_cols"].dtype == torch.uint8
        assert {k: pm[k] for k in ("off", "col_num", "col_den", "fade_len", "curve")} == dict(
            {k: plan["mel"][k] for k in ("off", "col_num", "col_den", "fade_len")}, curve="linear")
        assert "match_gain" not in pm and "rec_len" not in pm
        if keep == "audio":
            pa, at = rig.one("paste_audio"), rig.one("recording_at_rate")
            assert at["item"] is ctx["audio"] and at["rate"] == d["takes"] and at["out_rate"] == out_rate == plan["audio"]["rate"]
            assert pa["rec"] is rig.rec and pa["rec_len"] is rig.rec_len and torch.equal(pa["keep_cols"], plan["keep_cols"])
            assert {k: pa[k] for k in ("off", "col_num", "col_den", "fade_len", "curve", "match_gain")} == dict(
                {k: plan["audio"][k] for k in ("off", "col_num", "col_den", "fade_len")}, curve="equal_power", match_gain=True)
    else:
        assert not rig.calls("mel_image_from_audio") and not rig.calls("recording_at_rate")

    # ---- the files: stems, their order, the rates; the returned paths
    root = ctx["root"]
    if d.get("files") == "index":
        stems = [os.path.join(root, "%06d" % i) for i in range(B)]
    elif d.get("files") == "caption":
        stems = [os.path.join(root, "a dog", "%06d" % i) for i in range(10)]
        assert out == stems
    elif d.get("files") == "table":
        stems = [os.path.join(root, "a_mel_sample_%d" % i) for i in range(4)] + [os.path.join(root, "b_mel_sample_%d" % i) for i in range(2)]
        assert out == stems
    else:
        stems = []
        assert not os.path.exists(root)
    wavs = rig.calls("wav")
    assert [w["path"] for w in wavs] == [s + ".wav" for s in stems]
    for w in wavs:
        assert (w["samples"], w["value"], w["rate"]) == (samples, value, out_rate) and type(w["rate"]) is int
    if stems:                                                                # the .npy files are really written; nothing else is
        assert sorted(os.listdir(os.path.dirname(stems[0]))) == sorted(os.path.basename(s) + ".npy" for s in stems)


# ---- what reaches the model -----------------------------------------------------------------------------------------------
def test_model_generate_sample_with_condition(rig, tmp_path):
    _run(rig, "generate_sample_with_condition", {"level": "peak"}, None, tmp_path, negative_text="noise", guidance_scale=2.0)
    g = rig.one("generate_content")
    assert g["sample_type"] == "top0.8r,fast9" and g["guidance_scale"] == 2.0 and g["replicate"] == 1
    assert (g["filter_ratio"], g["content_ratio"], g["return_att_weight"]) == (0, 1, False)
    assert g["batch"] == {"text": ["a", "b"], "caption_ids": [4, 5], "seed": 3, "negative_text": "noise"}
    rig.log.clear()
    tokens = torch.zeros(2, 77, dtype=torch.long)
    rig.ds.generate_sample_with_condition(tokens, purity_steps=8, purity_weight=0.5)
    g = rig.one("generate_content")
    assert g["sample_type"] == "top0.85r,purity8w0.5" and g["guidance_scale"] is None
    assert list(g["batch"]) == ["condition_token"] and g["batch"]["condition_token"] is tokens
    rig.log.clear()
    embed = torch.zeros(2, 77, 512)
    rig.ds.generate_sample_with_condition(embed, level="rms")
    g = rig.one("generate_content")
    assert g["sample_type"] == "top0.85r" and list(g["batch"]) == ["condition_embed_token"] and g["batch"]["condition_embed_token"] is embed
    rig.log.clear()
    rig.ds.generate_sample_with_condition("one caption")
    assert rig.one("generate_content")["batch"] == {"text": ["one caption"]}


@pytest.mark.parametrize("req", [{}, {"level": "match"}], ids=_case_id)
def test_model_generate_sample_from_audio(rig, req, tmp_path):
    ctx, _ = _run(rig, "generate_sample_from_audio", req, None, tmp_path, filter_ratio=0.25)
    assert rig.one("prepare_condition")["batch"] == {"text": ["a", "b"]}
    pc = rig.one("prepare_content")["batch"]
    assert pc["audio"] is ctx["audio"] and pc["audio_rate"] == 32000 and list(pc) == ["audio", "audio_rate"]
    s = rig.one("sample")
    assert s["state"][:2] == (0.8, None) and s["filter_ratio"] == 0.25 and s["print_log"] is False
    assert s["condition_token"] is None and s["condition_mask"] is None and tuple(s["condition_embed"].shape) == (2, 3, 4)
    assert rig.one("decode_to_img")["zshape"] == (2, 256, 5, 53)


@pytest.mark.parametrize("name", ["inpaint_audio", "continue_audio", "inpaint_scene"])
@pytest.mark.parametrize("req", [{}, {"keep_original": "audio", "level": "match"}], ids=_case_id)
def test_model_inpainting_drivers(rig, name, req, tmp_path):
    more = dict(negative_text="noise", keep_mode="clamp")
    if name != "inpaint_scene":
        more.update(purity_steps=8)
    ctx, _ = _run(rig, name, req, None, tmp_path, **more)
    pc = rig.one("prepare_content")["batch"]
    assert pc["audio"] is ctx["audio"] and pc["audio_rate"] == 32000
    c = rig.one("inpaint_content")
    assert c["state"] == (0.8, None, 0.25, True)                              # this call's rate, installed around the call
    assert c["keep_mode"] == "clamp" and tuple(c["keep_mask"].shape) == (2, 265)
    want = {"caption_ids": [4, 5], "seed": 3, "negative_text": "noise"}
    if name == "inpaint_scene":
        assert c["sample_type"] == "top0.8r" and c["guidance_scale"] is None
        assert c["tracks"]["text"] == [["rain", "rain"], ["thunder", "thunder"]] and tuple(c["tracks"]["weight"].shape) == (2, 2, 265)
        assert float(c["tracks"]["weight"][0, 0].max()) == 3.0 and float(c["tracks"]["weight"][0, 1].max()) == 1.5
        assert torch.equal(c["keep_mask"], pipeline.spans_to_keep_mask(SPANS, 2))
    else:
        assert c["sample_type"] == "top0.8r,purity8" and c["guidance_scale"] == 2.0 and "tracks" not in c
        want["text"] = ["a", "b"]
        if name == "continue_audio":
            assert int(c["keep_mask"][0].sum()) == 5 * pipeline.continuation_columns(3.0) and bool(c["keep_mask"][0, 0])
    assert {k: v for k, v in c["batch"].items() if k != "content_token"} == want
    assert tuple(c["batch"]["content_token"].shape) == (2, 265)
    assert rig.one("decode_to_img")["zshape"] == (2, 256, 5, 53)


def test_model_inpaint_scene_takes_a_scene_per_clip(rig, tmp_path):
    scenes = [[("rain", 0.0, None)], [("wind", 1.0, 2.0), ("birds", 3.0, 4.0, 2.0)]]
    rig.ds.inpaint_scene(_recording(), scenes, SPANS, scale=2.5)
    trk = rig.one("inpaint_content")["tracks"]
    assert trk["text"] == [["rain", "wind"], ["", "birds"]] and float(trk["weight"][0, 0].max()) == 2.5
    rig.log.clear()
    rig.ds.generate_scene(scenes)
    c = rig.one("generate_long_content")
    assert c["tracks"]["text"] == [["rain", "wind"], ["", "birds"]] and float(c["tracks"]["weight"][1, 1].max()) == 2.0
    assert c["windows"] == 1 and c["sample_type"] == "top0.85r" and c["batch"] == {}


@pytest.mark.parametrize("name", ["generate_long", "extend_audio"])
@pytest.mark.parametrize("joint", [False, True])
def test_model_long_drivers(rig, name, joint, tmp_path):
    req = {"joint": True, "level": "peak"} if joint else {}
    ctx, out = _run(rig, name, req, None, tmp_path, negative_text="noise", keep_mode="clamp", purity_steps=None if joint else 8)
    c = rig.one("generate_long_content")
    assert (c["windows"], c["overlap_cols"], c["keep_mode"], c["guidance_scale"]) == (2, 13, "clamp", 2.0)
    assert c["sample_type"] == ("top0.8r" if joint else "top0.8r,purity8")
    assert c["batch"] == {"text": ["a", "b"], "caption_ids": [4, 5], "seed": 3, "negative_text": "noise"}
    assert "tracks" not in c
    if joint:
        assert c["joint"] is True and c["ring"] is False
    else:
        assert "joint" not in c and "ring" not in c
    if name == "extend_audio":
        pc = rig.one("prepare_content")["batch"]
        assert pc["audio"] is ctx["audio"] and pc["audio_rate"] == 32000 and tuple(c["start_token"].shape) == (2, 265)
    else:
        assert c["start_token"] is None
    assert rig.one("stitch_mel") == {"windows": 2, "hop": 640} and tuple(out[2].shape) == (2, 2, 265)


def test_model_generate_loop_and_scene(rig, tmp_path):
    _, out = _run(rig, "generate_loop", {"level": "peak"}, None, tmp_path, negative_text="noise", guidance_scale=2.0)
    c = rig.one("generate_long_content")
    assert (c["windows"], c["overlap_cols"], c["keep_mode"], c["guidance_scale"]) == (3, 13, "clamp", 2.0)
    assert c["sample_type"] == "top0.8r,fast9" and c["joint"] is True and c["ring"] is True and c["start_token"] is None
    assert c["batch"] == {"text": ["a", "b"], "caption_ids": [4, 5], "seed": 3, "negative_text": "noise"}
    assert rig.one("stitch_mel") == {"windows": 7, "hop": 640} and out[3] == 120 * 4096 / 22050
    assert rig.one("vocoder")["shape"] == (2, 80, 848 + 6 * 640)
    rig.log.clear()
    _run(rig, "generate_scene", {}, None, tmp_path, negative_text="noise")
    c = rig.one("generate_long_content")
    assert (c["windows"], c["overlap_cols"], c["keep_mode"], c["guidance_scale"]) == (2, 13, "clamp", None)
    assert c["sample_type"] == "top0.8r,fast9" and "joint" not in c and c["start_token"] is None
    assert c["batch"] == {"caption_ids": [4], "seed": 3, "negative_text": "noise"}
    assert c["tracks"]["text"] == [["rain"], ["thunder"]] and tuple(c["tracks"]["weight"].shape) == (1, 2, 5 * 93)


@pytest.mark.parametrize("req", [{}, {"level": "peak"}], ids=_case_id)
def test_model_generate_best_of(rig, req, tmp_path):
    _, (mel01, wave, winners, scores) = _run(rig, "generate_best_of", req, None, tmp_path, negative_text="noise", purity_steps=8)
    assert rig.one("prepare_condition")["batch"] == {"text": ["a", "b"]}
    c = rig.one("_run_chain")
    assert c["sample_type"] == "top0.8r,fast9,purity8" and c["replicate"] == 3 and c["guidance_scale"] == 2.0
    assert rig.one("_free_keywords")["args"] == (0, 1.0, False, "top0.8r,fast9,purity8") and c["keywords"] == {"free": (0, 1.0, False, c["sample_type"])}
    assert sorted(c["batch"]) == ["caption_ids", "negative_text", "seed", "text"] and c["batch"]["caption_ids"].tolist() == [0, 1]
    assert (c["batch"]["text"], c["batch"]["seed"], c["batch"]["negative_text"]) == (["a", "b"], 3, "noise")
    assert tuple(c["condition"]["condition_embed_token"].shape) == (6, 3, 4)
    s = rig.one("score_tokens")
    assert (s["timesteps"], s["draws"], s["seed"]) == (2, 1, 3) and s["caption_ids"].tolist() == [0, 1, 0, 1, 0, 1]
    assert s["condition_token"] is None and tuple(s["condition_embed"].shape) == (6, 3, 4) and tuple(s["tokens"].shape) == (6, 265)
    assert scores.tolist() == [[0.0, -2.0, -4.0], [-1.0, -3.0, -5.0]]
    assert winners[:, 0].tolist() == [4, 5] and rig.one("decode_to_img")["zshape"] == (2, 256, 5, 53)
    assert torch.equal(rig.one("decode_to_img")["tokens"], winners)


@pytest.mark.parametrize("req", [{}, {"level": "loudness"}], ids=_case_id)
def test_model_reference_file_drivers(rig, req, tmp_path):
    _run(rig, "inference_generate_sample_with_condition", req, None, tmp_path, negative_text="noise", purity_steps=8, purity_weight=0.5)
    g = rig.one("generate_content")
    assert g["sample_type"] == "top0.8r,fast9,purity8w0.5" and g["replicate"] == 10 and g["guidance_scale"] == 2.0
    assert g["batch"] == {"text": ["a dog"], "negative_text": "noise"}
    for mode, ids in (("torch", [None, None]), ("philox", [[0, 1], [2]])):
        rig.log.clear()
        rig.ds.model.transformer.rng_mode = mode
        _run(rig, "generate_sample", req, 48000, tmp_path, purity_steps=8)
        first, second = rig.calls("generate_content")
        assert first["sample_type"] == second["sample_type"] == "top0.8r,fast9,purity8" and first["replicate"] == 2
        assert first["guidance_scale"] == 2.0
        assert first["batch"] == dict({"text": ["a dog", "a cat"]}, **({} if ids[0] is None else {"caption_ids": ids[0]}))
        assert second["batch"] == dict({"text": ["rain"]}, **({} if ids[1] is None else {"caption_ids": ids[1]}))


# ---- the level request in full; where it is refused -----------------------------------------------------------------------
def test_level_dict_reaches_audio_level_as_given(rig, tmp_path):
    spec = {"strategy": "loudness", "target": -18, "ceiling_db": -2, "limit": {"lookahead_ms": 2.0}}
    for name in ("generate_sample_with_condition", "inpaint_audio", "generate_long", "generate_best_of", "generate_sample"):
        rig.log.clear()
        _run(rig, name, {"level": spec}, 48000, tmp_path)
        for lv in rig.calls("level"):
            assert (lv["rate"], lv["strategy"], lv["target"], lv["ceiling_db"]) == (48000, "loudness", -18.0, -2.0)
            assert lv["limit"] is spec["limit"] and lv["reference"] is None
        assert len(rig.calls("level")) == (2 if name == "generate_sample" else 1)


def test_refusals_come_before_any_work(rig, tmp_path):
    ds, rec = rig.ds, _recording()
    with pytest.raises(ValueError, match="limit"):                           # before loop_plan, which refuses 5 s itself
        ds.generate_loop(["a"], 5.0, level={"strategy": "peak", "limit": True})
    with pytest.raises(ValueError, match="whole"):
        ds.generate_loop(["a"], 15.0, sample_rate=48000)
    for name, d in DRIVERS.items():
        args, kw = d["args"]({"audio": rec, "root": str(tmp_path / "out"), "tsv": _tsv(tmp_path)})
        with pytest.raises(ValueError):
            getattr(ds, name)(*args, level="louder", **kw)
        with pytest.raises(ValueError):
            getattr(ds, name)(*args, level={"strategy": "match", "target": -20.0}, **kw)
        if not d.get("takes"):
            with pytest.raises(ValueError, match="recording"):
                getattr(ds, name)(*args, level="match", **kw)
        if d.get("pastes"):
            with pytest.raises(ValueError):
                getattr(ds, name)(*args, keep_original="samples", **kw)
            with pytest.raises(ValueError):
                getattr(ds, name)(*args, keep_original="mel", fade_seconds=float("nan"), **kw)
        else:
            with pytest.raises(TypeError):
                getattr(ds, name)(*args, keep_original="mel", **kw)
        if not d.get("joint"):
            with pytest.raises(TypeError):
                getattr(ds, name)(*args, joint=True, **kw)
    assert rig.log == [] and not os.path.exists(str(tmp_path / "out"))


def test_without_a_vocoder(monkeypatch, tmp_path):
    rig = Rig(monkeypatch, vocoder=False)
    for name, d in DRIVERS.items():
        for req in ({"level": "peak"}, {"keep_original": "mel"} if d.get("pastes") else {}):
            rig.log.clear()
            _, out = _run(rig, name, req, None, tmp_path / name / _case_id(req))
            assert rig.tail() == (["paste_mel"] if req.get("keep_original") else []) and not rig.calls("wav")
            if d.get("files") not in ("caption", "table"):
                assert out[1] is None
        if d.get("pastes"):
            with pytest.raises(ValueError, match="vocoder"):
                _run(rig, name, {"keep_original": "audio"}, None, tmp_path)


# ---- fade_seconds / match_gain; the chunked vocoder pass ---------------------------------------------------------------
def test_paste_keywords_reach_the_plan(rig, tmp_path):
    for name in ("inpaint_audio", "extend_audio"):
        rig.log.clear()
        _run(rig, name, {"keep_original": "audio", "fade_seconds": 0.25, "match_gain": False}, 44100, tmp_path)
        plan = pipeline.paste_plan(name, "audio", batch=2, sample_rate=44100, fade_seconds=0.25, match_gain=False, **DRIVERS[name]["pastes"])
        assert rig.one("paste_mel")["fade_len"] == plan["mel"]["fade_len"] == 0.25 * 22050 / 256
        pa = rig.one("paste_audio")
        assert pa["fade_len"] == plan["audio"]["fade_len"] == 0.25 * 44100 and pa["match_gain"] is False
        assert pa["off"] == plan["audio"]["off"] == 2816


@pytest.mark.parametrize("name", ["generate_long", "generate_loop"])
def test_a_long_mel_goes_through_the_vocoder_in_chunks_of_whole_clips(rig, name, tmp_path):
    rig.ds.VOCODER_CHUNK_FRAMES = 1                                          # every clip is a chunk of its own
    _, out = _run(rig, name, {"level": "peak"}, None, tmp_path)
    frames = 848 + (1 if name == "generate_long" else 6) * 640
    assert rig.tail() == ["vocoder", "vocoder", "level"]
    assert [v["shape"] for v in rig.calls("vocoder")] == [(1, 80, frames)] * 2
    assert tuple(out[1].shape) == (2, 1, DRIVERS[name]["samples"]) and bool((out[1] == 1001.0).all())


# ---- the transformer's truncation state -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fails", [("generate_sample_from_audio", "sample"), ("inpaint_audio", "inpaint_content"),
                                        ("inpaint_scene", "inpaint_content"), ("continue_audio", "inpaint_content")])
def test_truncation_state_is_restored_when_the_model_raises(rig, name, fails, tmp_path):
    rig.fail = fails
    before = rig.ds.model.state()
    with pytest.raises(RuntimeError, match="stub"):
        _run(rig, name, {"level": "peak"}, None, tmp_path)
    assert rig.ds.model.state() == before == (0.7, 5, 0.25, False)
    assert rig.calls(fails)[0]["state"][:2] == (0.8, None) and rig.tail() == []
