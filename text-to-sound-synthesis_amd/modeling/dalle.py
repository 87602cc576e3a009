"""Drop-in for sound_synthesis/modeling/models/dalle_spec.py:DALLE (generation side).

generate_content() keeps the reference's keyword signature and `sample_type` mini-language
(:179-247): "top{r}r" installs top-r truncation -- natively, as a kernel argument, instead of the
reference's monkey-patched predict_start wrapper (:208-210).  The caption conditioning is either text
(`batch['text']`: BPE tokenizer + the HIP CLIP text tower, when the config builds them), already tokenised
captions (`condition_token` i64[B, 77]) or the embedding itself (`condition_embed_token` f32[B, 77, 512], what
CLIPTextEmbedding.forward returns), in `batch` or as `condition=`.
"""
import torch
from torch import nn

from ..config import instantiate_from_config


class DALLE(nn.Module):
    def __init__(self, *, content_info={"key": "image"}, condition_info={"key": "text"}, content_codec_config,
                 condition_codec_config, first_stage_permuter_config, diffusion_config):
        super().__init__()
        self.content_info = content_info
        self.condition_info = condition_info
        self.content_codec = instantiate_from_config(content_codec_config)
        self.condition_codec = instantiate_from_config(condition_codec_config)  # Tokenize: section 8f-1
        self.transformer = instantiate_from_config(diffusion_config)
        self.first_stage_permuter = instantiate_from_config(first_stage_permuter_config)
        self.truncation_forward = False

    @property
    def device(self):
        return self.transformer.device

    def get_ema_model(self):
        return self.transformer

    @torch.no_grad()
    def get_tokens(self, spec):
        """mel image [B, 1, 80, 848] -> (quant_z, token ids [B, 265] in sequence order) (dalle_spec.py:70-77)."""
        quant_z, _, info = self.content_codec.encode(spec)
        indices = self.first_stage_permuter(info[2].view(quant_z.shape[0], -1))
        self.zshape = quant_z.shape
        return quant_z, indices

    @torch.no_grad()
    def content_image(self, batch):
        """batch[content key] on the model's device; a batch without it that carries 'audio' (f32[B, T] on the device, or a
        list of .wav paths / host arrays) gets the mel image from the HIP front end (modeling/melspec.py: the reference's
        offline extract_mel_spectrogram.py + the dataset's crop and 2 x - 1).  batch['audio_rate'] (an int, or a list with one
        rate per clip) states the sample rate; absent = 22 050 Hz for tensors and arrays, the header's rate for paths.  Another
        rate than 22 050 Hz is resampled on the device first (audio.resample)."""
        key = self.content_info["key"]
        if key not in batch and batch.get("audio") is not None:
            from .melspec import mel_image_from_audio
            return mel_image_from_audio(batch["audio"], self.device, rate=batch.get("audio_rate"))
        cont = batch[key]
        return cont.to(self.device) if torch.is_tensor(cont) else cont

    @torch.no_grad()
    def prepare_content(self, batch, with_mask=False):
        """batch[content key] (or batch['audio']) -> {'content_token', 'content_quant'} (dalle_spec.py:107-126, with_mask=False
        branch)."""
        if with_mask:
            raise NotImplementedError("masked content encoding is not part of the sound pipeline (:118-120)")
        quant_z, indices = self.get_tokens(self.content_image(batch))
        return {"content_token": indices, "content_quant": quant_z}

    @torch.no_grad()
    def prepare_input(self, batch):
        """condition + content of a training batch (dalle_spec.py:128-133)"""
        inp = self.prepare_condition(batch)
        inp.update(self.prepare_content(batch))
        return inp

    @torch.no_grad()
    def forward(self, batch, name="none", **kwargs):
        """batch {'image': mel f32[B,1,80,848], 'text' | 'condition_embed_token': ...} -> the transformer's
        {'logits', 'loss'} (dalle_spec.py:389-400).  A forward value (no autograd through the HIP path): training enters
        through `Solver.step(batch)` / `TrainStep` (modeling/solver.py, modeling/train.py), which has its own backward."""
        return self.transformer(self.prepare_input(batch), **kwargs)

    def decode_to_img(self, index, zshape, stage="first"):
        """tokens (sequence order) -> mel image [B, 1, 80, 848] (:80-91)."""
        assert stage == "first"
        return self.content_codec.decode_tokens(index, zshape[2], zshape[3])

    @torch.no_grad()
    def prepare_condition(self, batch, condition=None):
        cond = {}
        src = batch if condition is None else condition
        if torch.is_tensor(src):
            src = {"condition_embed_token": src}
        emb = src.get("condition_embed_token", src.get("embed_token"))
        tok = src.get("condition_token", src.get("token"))
        if emb is not None:
            cond["condition_embed_token"] = emb.to(self.device)
            cond["condition_token"] = None
        elif tok is not None:      # already tokenised captions i64[B, 77]
            cond["condition_token"] = tok.to(self.device)
        elif self.condition_codec is not None:
            for k, v in self.condition_codec.get_tokens(src[self.condition_info["key"]]).items():
                cond["condition_" + k] = v.to(self.device) if torch.is_tensor(v) else v
        else:
            raise NotImplementedError(
                "this model was built without a text codec (condition_codec_config = None): pass "
                "batch={'condition_embed_token': f32[B,77,512]} or {'condition_token': i64[B,77]}")
        return cond

    @torch.no_grad()
    def null_condition(self, negative=None, batch=None):
        """The null condition of classifier-free guidance (DiffusionTransformer.sample: guidance_scale): the CLIP embedding
        of the empty caption "" -- f32[77, 512], computed once per device and cached -- or of `negative`, a caption
        (f32[77, 512]) or a list of B captions (f32[B, 77, 512]); through condition_codec + transformer.condition_emb.  A
        model built without a text stage takes batch['null_condition_embed_token'] (f32[77, 512] or [B, 77, 512]) instead."""
        tr = self.transformer
        if self.condition_codec is None or tr.condition_emb is None:
            emb = None if batch is None else batch.get("null_condition_embed_token")
            if emb is None:
                raise ValueError("classifier-free guidance needs a null condition: this model has no text stage "
                                 "(condition_codec / condition_emb), so pass batch['null_condition_embed_token'] "
                                 "f32[77,512] or [B,77,512]")
            if negative is not None:
                raise ValueError("negative_text needs the text stage (condition_codec + condition_emb) this model lacks")
            return torch.as_tensor(emb).float().to(self.device)
        if negative is None:
            cache = self.__dict__.setdefault("_null_condition", {})
            key = str(self.device)
            if key not in cache:
                cache[key] = self._embed_captions([""])[0]
            return cache[key]
        if isinstance(negative, str):
            return self._embed_captions([negative])[0]
        return self._embed_captions(list(negative))

    def _embed_captions(self, captions):
        tok = self.condition_codec.get_tokens(captions)["token"]
        return self.transformer.condition_emb(tok.to(self.device)).float()

    def _guidance(self, batch, guidance_scale, replicate):
        """sample()'s guidance keywords: the null embedding from batch['negative_text'] (or the empty caption), replicated
        with the captions.  guidance_scale None or exactly 1: no keywords, today's path."""
        if guidance_scale is None or float(guidance_scale) == 1.0:
            return {}
        null = self.null_condition(batch.get("negative_text"), batch=batch)
        if null.dim() == 3 and replicate != 1:
            null = torch.cat([null for _ in range(replicate)], dim=0)
        return {"guidance_scale": float(guidance_scale), "null_condition_embed": null}

    def _track_keywords(self, batch, tracks, replicate, sample_type, total_cols=None):
        """sample()'s caption-track keywords (DiffusionTransformer.sample: track_embed, track_weight) from `tracks`, a dict:
        'text' -- C captions (each for the whole batch) or C lists of B captions, each track through prepare_condition's text
        stage once; 'weight' -- f32[B, C, 265] (time-major like content_token; pipeline.track_weights builds it from
        seconds), or f32[B, C, 5 total_cols] for the long form.  A model without a text stage takes 'embed' f32[C, B, 77, 512]
        instead of 'text', mirroring null_condition_embed_token.  The null condition is batch['negative_text'] or the empty
        caption, as for guidance.  None: no keywords, today's path.  The rules are checked before anything runs."""
        if tracks is None:
            return None
        if replicate != 1:
            raise ValueError("replicate must be 1 with tracks: repeat the scene under different caption_ids instead")
        if self._purity_part(sample_type) is not None:
            raise ValueError("caption tracks have no purity form: sample type %r" % (sample_type,))
        if tracks.get("weight") is None:
            raise ValueError("tracks needs 'weight': f32[B, C, 265]")
        tr = self.transformer
        w = torch.as_tensor(tracks["weight"]).float()
        L = tr.content_seq_len if total_cols is None else 5 * int(total_cols)
        if w.dim() != 3 or w.shape[2] != L or not 1 <= w.shape[1] <= tr.MAX_TRACKS:
            raise ValueError("tracks['weight'] must be f32[B, C, %d] with 1 <= C <= %d, got %s" % (L, tr.MAX_TRACKS, tuple(w.shape)))
        if not bool(torch.isfinite(w).all()):
            raise ValueError("tracks['weight'] must be finite")
        B, C = w.shape[0], w.shape[1]
        if self.condition_codec is None or tr.condition_emb is None:
            if tracks.get("embed") is None:
                raise ValueError("this model has no text stage (condition_codec / condition_emb): pass tracks['embed'] "
                                 "f32[C, B, 77, 512]")
            emb = torch.as_tensor(tracks["embed"]).float().to(self.device)
        else:
            text = tracks.get("text")
            if text is None or isinstance(text, str) or len(text) != C:
                raise ValueError("tracks['text'] must hold one caption (or one list of B captions) per track: %d" % C)
            embs = []
            for caps in text:
                caps = [caps] * B if isinstance(caps, str) else list(caps)
                if len(caps) != B:
                    raise ValueError("a track's caption list must have B = %d entries, got %d" % (B, len(caps)))
                cond = self.prepare_condition({self.condition_info["key"]: caps})
                embs.append(tr._cond(cond.get("condition_token"), cond.get("condition_embed_token")).to(self.device))
            emb = torch.stack(embs, 0)
        if tuple(emb.shape[:2]) != (C, B):
            raise ValueError("tracks['embed'] must be f32[C, B, 77, 512] = [%d, %d, ...], got %s" % (C, B, tuple(emb.shape)))
        return {"track_embed": emb, "track_weight": w, "null_condition_embed": self.null_condition(batch.get("negative_text"), batch=batch)}

    @staticmethod
    def _window_tracks(kw, w, overlap_cols):
        """the track keywords of window w of the long form: the weight's slice over the window's own global columns
        [w (53 - n), w (53 - n) + 53), time-major"""
        from ..pipeline import GRID_COLS
        if kw is None:
            return None
        wt = kw["track_weight"]
        c0 = w * (GRID_COLS - overlap_cols)
        return dict(kw, track_weight=wt[:, :, 5 * c0:5 * (c0 + GRID_COLS)].contiguous())

    def _install_sample_type(self, sample_type):
        """The `sample_type` mini-language (:179-247) applied to the transformer; returns its comma-separated parts."""
        parts = sample_type.split(",")
        tr = self.transformer
        if len(parts) > 1 and parts[1][:1] == "q":           # repeat-step sampler (:135-143, :205-206)
            tr.repeat_rate = float(parts[1].replace("q", ""))
        if parts[0][:3] == "top" and not self.truncation_forward:
            # installed once and sticky, like the reference's predict_start wrapper (:207-209)
            if parts[0][-1] == "p":
                tr.truncation_k, tr.truncation_r = int(parts[0][:-1].replace("top", "")), None
            elif parts[0][-1] == "r":
                tr.truncation_r, tr.truncation_k = float(parts[0][:-1].replace("top", "")), None
            else:
                print("wrong sample type")                    # the reference's reaction (:176-177)
            self.truncation_forward = True
        return parts

    @staticmethod
    def _purity_part(sample_type, keep_mode="clamp"):
        """The purity part of a sample type (not in the reference): ",purity{S}" or ",purity{S}w{r}" -- an S-step purity-prior
        chain (DiffusionTransformer.sample_purity), r = the sharpening weight (default 0) -> (S, r), or None without one.
        Together with ",fast{n}", ",q{rate}" or keep_mode "renoise" it raises ValueError: before anything is installed or run."""
        parts = sample_type.split(",")
        pur = [q for q in parts[1:] if q[:6] == "purity"]
        if not pur:
            return None
        if len(pur) > 1:
            raise ValueError("one purity part per sample type, got %r" % (sample_type,))
        for q in parts[1:]:
            if q[:4] == "fast" or q[:1] == "q":
                raise ValueError("purity sampling has its own chain: %r cannot be combined with it (%r)" % (q, sample_type))
        if keep_mode != "clamp":
            raise ValueError("purity sampling holds positions clean: keep_mode=%r cannot be combined with it" % (keep_mode,))
        body = pur[0][6:]
        try:
            steps, sep, weight = body.partition("w")
            return int(steps), (float(weight) if sep else 0.0)
        except ValueError:
            raise ValueError("a purity part is 'purity{S}' or 'purity{S}w{r}', got %r" % (pur[0],)) from None

    @staticmethod
    def _replicated_caption_ids(batch, replicate):
        ids = torch.as_tensor(batch["caption_ids"], dtype=torch.long)
        return torch.cat([ids for _ in range(replicate)]) + \
            torch.arange(replicate).repeat_interleave(ids.numel()) * int(batch.get("caption_id_stride", 1 << 24))

    @staticmethod
    def _free_keywords(filter_ratio, temperature, return_att_weight, sample_type):
        """the chain keywords of generate_content: everything is generated"""
        return dict(content_token=None, filter_ratio=filter_ratio, temperature=temperature, return_att_weight=return_att_weight,
                    return_logits=False, print_log=False, sample_type=sample_type)

    @staticmethod
    def _hold_keywords(tokens, keep, keep_mode):
        """the chain keywords of inpaint_content: the positions of `keep` carry `tokens`"""
        return dict(content_token=tokens, filter_ratio=0, return_logits=False, print_log=False, keep_mask=keep, keep_mode=keep_mode)

    def _run_chain(self, batch, condition, kw, replicate, sample_type, guidance_scale, tracks=None):
        """What generate_content, inpaint_content and generate_long_content share once the chain's own keywords `kw` are set:
        install the sample type, add the (replicated) condition, the guidance and the noise keywords of `batch`, run sample(),
        sample_fast() or -- for a sample type with a ",purity{S}" part (_purity_part) -- sample_purity() -> tokens i64[B r, 265]."""
        purity = self._purity_part(sample_type, kw.get("keep_mode", "clamp"))
        parts = self._install_sample_type(sample_type)
        tr = self.transformer
        kw = dict(kw, condition_token=condition.get("condition_token"), condition_mask=condition.get("condition_mask"),
                  condition_embed=condition.get("condition_embed_token"))
        kw.update(self._guidance(batch, guidance_scale, replicate))
        if tracks is not None:                               # caption tracks (_track_keywords): guidance_scale must be None
            kw.update(tracks, guidance_scale=guidance_scale)
        if batch.get("caption_ids") is not None:             # per-caption in-kernel noise (diffusion.py rng_mode)
            kw["caption_ids"] = self._replicated_caption_ids(batch, replicate)
        if batch.get("seed") is not None:
            kw["seed"] = int(batch["seed"])
        if purity is not None:                               # purity-prior chain: ",purity{S}" / ",purity{S}w{r}"
            return tr.sample_purity(steps=purity[0], purity_weight=purity[1], **kw)["content_token"]
        if len(parts) == 2 and parts[1][:4] == "fast":       # skip-step sampler (:211-222)
            return tr.sample_fast(skip_step=int(parts[1][4:]), **kw)["content_token"]
        return tr.sample(**kw)["content_token"]

    @torch.no_grad()
    def inpaint_content(self, *, batch, keep_mask, keep_mode="clamp", replicate=1, sample_type="top0.85r", guidance_scale=None,
                        tracks=None):
        """Region-held generation (not in the reference, whose content_ratio slices the token vector and cannot run for any
        value but 1): the positions of `keep_mask` (bool[B, 265], True = held, time-major like content_token;
        pipeline.spans_to_keep_mask builds it from seconds) keep the tokens of the batch's content, the others are generated
        from [MASK] under the batch's caption with the held ones as context of the denoiser.  batch: the caption as in
        prepare_condition ('text', 'condition_token' or 'condition_embed_token') and the content as in prepare_content
        ('image', or 'audio' with 'audio_rate') or already encoded ('content_token' i64[B, 265]); 'caption_ids' / 'seed' as in
        generate_content.  keep_mode "clamp" | "renoise": DiffusionTransformer.sample.  Every sample_type of generate_content
        works.  guidance_scale: classifier-free guidance as in generate_content.  Returns {'content': mel image [B r, 1, 80, 848], 'content_token'}.

        The held TOKENS of the result are exactly the input's.  The mel is the codec's rendering of the whole grid, held
        region included: not the input's samples (the decoder's lowest level attends over all 265 positions), and the
        original mel or audio is not pasted back.
        tracks: caption tracks as in generate_content -- the free positions are generated under the scene."""
        trk = self._track_keywords(batch, tracks, replicate, sample_type)
        self.eval()
        condition = self.prepare_condition(batch=batch) if trk is None else {}
        tokens = batch.get("content_token")
        if tokens is None:
            tokens = self.prepare_content(batch)["content_token"]
        tokens = tokens.to(self.device)
        keep = torch.as_tensor(keep_mask).to(self.device)
        if replicate != 1:
            for k in condition:
                if torch.is_tensor(condition[k]):
                    condition[k] = torch.cat([condition[k] for _ in range(replicate)], dim=0)
            tokens = torch.cat([tokens for _ in range(replicate)], dim=0)
            keep = torch.cat([keep for _ in range(replicate)], dim=0)
        out_tokens = self._run_chain(batch, condition, self._hold_keywords(tokens, keep, keep_mode), replicate, sample_type,
                                     guidance_scale, trk)
        content = self.decode_to_img(out_tokens, (out_tokens.shape[0], 256, 5, 53))
        self.train()
        return {"content": content, "content_token": out_tokens}

    @torch.no_grad()
    def generate_content(self, *, batch, condition=None, filter_ratio=0.5, temperature=1.0, content_ratio=0.0,
                         replicate=1, return_att_weight=False, sample_type="top0.85r", guidance_scale=None,
                         tracks=None):
        """guidance_scale (not in the reference): classifier-free guidance of every sampler step against the null condition
        -- the empty caption, or batch['negative_text'] (a caption or a list of B) -- see DiffusionTransformer.sample and
        null_condition; None or exactly 1 is the unguided path.
        sample_type (beyond the reference's forms): a ",purity{S}" or ",purity{S}w{r}" part, e.g. "top0.85r,purity25", runs an
        S-step purity-prior chain instead (_purity_part, DiffusionTransformer.sample_purity; filter_ratio must resolve to 0).
        tracks (not in the reference): caption tracks, a scene instead of one caption -- {'text': C captions or C lists of B,
        'weight': f32[B, C, 265]} (_track_keywords; pipeline.track_weights builds both from (caption, start, end) triples).
        The batch then needs no caption; replicate must be 1 and guidance_scale None."""
        trk = self._track_keywords(batch, tracks, replicate, sample_type)
        self.eval()
        condition = self.prepare_condition(batch=batch, condition=condition) if trk is None else {}
        if replicate != 1:
            for k in condition:
                if condition[k] is not None:
                    condition[k] = torch.cat([condition[k] for _ in range(replicate)], dim=0)
        tokens = self._run_chain(batch, condition, self._free_keywords(filter_ratio, temperature, return_att_weight, sample_type),
                                 replicate, sample_type, guidance_scale, trk)
        zshape = (tokens.shape[0], 256, 5, 53)   # hard-coded in the reference too (:236)
        content = self.decode_to_img(tokens, zshape)
        self.train()
        return {"content": content, "content_token": tokens}

    @torch.no_grad()
    def _joint_long_content(self, batch, windows, n, ring, keep_mode, sample_type, guidance_scale, start_token, tracks):
        """generate_long_content(joint=True): the token stage as ONE joint chain (DiffusionTransformer.sample_joint)."""
        from ..pipeline import GRID_COLS, GRID_ROWS, joint_canvas_cols, joint_window_positions
        if tracks is not None:
            raise ValueError("caption tracks are not built for joint sampling (joint=True)")
        if keep_mode != "clamp":
            raise ValueError("joint sampling holds positions clean: keep_mode=%r is not built for it (joint=True)" % (keep_mode,))
        if self._purity_part(sample_type, keep_mode) is not None:
            raise ValueError("a purity part is not built for joint sampling (joint=True): sample type %r" % (sample_type,))
        parts = sample_type.split(",")
        skip = 0
        for q in parts[1:]:
            if q[:4] != "fast":
                raise ValueError("joint sampling takes 'top{r}r' / 'top{k}p' and ',fast{n}': %r is not built for it" % (q,))
            skip = int(q[4:])
        Lc = GRID_ROWS * joint_canvas_cols(windows, n, ring)
        self.eval()
        condition = self.prepare_condition(batch=batch)
        tr = self.transformer
        cond_emb = tr._cond(condition.get("condition_token"), condition.get("condition_embed_token"))
        B = cond_emb.shape[0]
        ids = batch.get("caption_ids")
        ids = torch.arange(B) if ids is None else torch.as_tensor(ids, dtype=torch.long).reshape(-1)
        if ids.numel() != B:
            raise ValueError("%d caption ids for %d captions" % (ids.numel(), B))
        kw = dict(self._guidance(batch, guidance_scale, 1), caption_ids=ids)
        if batch.get("seed") is not None:
            kw["seed"] = int(batch["seed"])
        if start_token is not None:                           # the recording's grid: a held canvas head
            head = torch.as_tensor(start_token).to(self.device).long().contiguous()
            if tuple(head.shape) != (B, tr.content_seq_len):
                raise ValueError("start_token must be i64[%d, %d], got %s" % (B, tr.content_seq_len, tuple(head.shape)))
            known = torch.zeros(B, Lc, dtype=torch.long, device=self.device)
            known[:, :GRID_ROWS * GRID_COLS] = head
            keep = torch.zeros(B, Lc, dtype=torch.bool, device=self.device)
            keep[:, :GRID_ROWS * GRID_COLS] = True
            kw.update(keep_mask=keep, content_token=known)
        saved = tr.truncation_r, tr.truncation_k, tr.repeat_rate, self.truncation_forward
        self.truncation_forward = False                       # install THIS call's sample type
        try:
            self._install_sample_type(parts[0])
            canvas = tr.sample_joint(cond_emb, windows, n, ring=ring, skip_step=skip, **kw)
        finally:
            tr.truncation_r, tr.truncation_k, tr.repeat_rate, self.truncation_forward = saved
        tokens = canvas[:, joint_window_positions(windows, n, ring).to(canvas.device)].contiguous()       # [B, W, 265]
        flat = tokens.view(B * windows, tokens.shape[2])
        content = self.decode_to_img(flat, (flat.shape[0], 256, 5, 53))
        self.train()
        return {"content": content, "content_token": tokens, "canvas_token": canvas}

    @torch.no_grad()
    def generate_long_content(self, *, batch, windows, overlap_cols, keep_mode="clamp", sample_type="top0.85r",
                              guidance_scale=None, start_token=None, tracks=None, joint=False, ring=False):
        """A clip longer than one token grid as `windows` overlapping 5 x 53 grids (not in the reference; the plan comes from
        pipeline.long_plan).  Window 0 is what generate_content(filter_ratio=0, content_ratio=1) generates with per-caption
        in-kernel noise (batch['caption_ids'], default 0 .. B-1; batch['seed']) -- or start_token (i64[B, 265], e.g. a
        recording's tokens), and then no chain runs for it.  Window w >= 1 is inpaint_content's chain on
        pipeline.continuation_tokens(window w-1, overlap_cols): the last overlap_cols columns of its predecessor, held as its
        first ones (keep_mode "clamp" | "renoise"), the rest generated under the same caption, seed, sample_type and guidance
        with the caption ids + w 2^20 (pipeline.window_caption_ids: ids must be below 2^20, which keeps the windows apart from
        each other and from the replicate stride 2^24).  All windows are decoded in ONE decode_to_img call at batch B W.
        The model's truncation settings are this call's only: saved before and restored after.
        tracks: caption tracks as in generate_content with 'weight' f32[B, C, 5 total columns], total columns =
        53 + (W - 1)(53 - overlap_cols); window w runs under the slice over its own global columns (_window_tracks).
        Returns {'content_token': i64[B, W, 265], 'content': mel image [B W, 1, 80, 848], clip-major (index b W + w)}.

        joint=True: the token stage is ONE joint chain instead -- all windows on one token canvas, one denoiser forward per
        step at batch B W, one token drawn per canvas position from the fusion of the windows that cover it
        (DiffusionTransformer.sample_joint) under the clips' own caption ids; start_token becomes a held canvas head.  ring=True
        (joint only, W >= 2) closes the canvas into a ring.  Also returns 'canvas_token' i64[B, 5 C]; content_token holds the
        windows cut from the canvas, so two neighbours carry the SAME tokens in the columns they share.  tracks, a purity part
        and keep_mode "renoise" are not built for joint sampling and raise ValueError.  joint=False: today's path."""
        from ..pipeline import GRID_COLS, MAX_WINDOWS, continuation_tokens, window_caption_ids
        windows, n = int(windows), int(overlap_cols)
        if not 1 <= windows <= MAX_WINDOWS:
            raise ValueError("windows must be in 1 .. %d, got %r" % (MAX_WINDOWS, windows))
        if not 1 <= n <= GRID_COLS // 2:
            raise ValueError("overlap_cols must be in 1 .. %d, got %r" % (GRID_COLS // 2, overlap_cols))
        if ring and not joint:
            raise ValueError("a ring exists under joint sampling only: pass joint=True with ring=True")
        if joint:
            return self._joint_long_content(batch, windows, n, bool(ring), keep_mode, sample_type, guidance_scale, start_token,
                                            tracks)
        trk = self._track_keywords(batch, tracks, 1, sample_type, GRID_COLS + (windows - 1) * (GRID_COLS - n))
        self.eval()
        condition = self.prepare_condition(batch=batch) if trk is None else {}
        B = next(v.shape[0] for v in condition.values() if torch.is_tensor(v)) if trk is None else trk["track_weight"].shape[0]
        ids = batch.get("caption_ids")
        ids = torch.arange(B) if ids is None else torch.as_tensor(ids, dtype=torch.long).reshape(-1)
        if ids.numel() != B:
            raise ValueError("%d caption ids for %d captions" % (ids.numel(), B))
        window_caption_ids(ids, windows - 1)                  # the range check, before anything runs
        self._purity_part(sample_type, keep_mode)             # ... and the purity part's rules (window 0 holds nothing)
        tr = self.transformer
        saved = tr.truncation_r, tr.truncation_k, tr.repeat_rate, self.truncation_forward
        self.truncation_forward = False                       # install THIS call's sample type
        try:
            if start_token is not None:
                cur = torch.as_tensor(start_token).to(self.device).long().contiguous()
                if tuple(cur.shape) != (B, tr.content_seq_len):
                    raise ValueError("start_token must be i64[%d, %d], got %s" % (B, tr.content_seq_len, tuple(cur.shape)))
            else:
                cur = self._run_chain(dict(batch, caption_ids=ids), condition, self._free_keywords(0, 1.0, False, sample_type), 1,
                                      sample_type, guidance_scale, self._window_tracks(trk, 0, n))
            toks = [cur]
            for w in range(1, windows):
                known, keep = continuation_tokens(cur, n)
                cur = self._run_chain(dict(batch, caption_ids=window_caption_ids(ids, w)), condition,
                                      self._hold_keywords(known, keep, keep_mode), 1, sample_type, guidance_scale,
                                      self._window_tracks(trk, w, n))
                toks.append(cur)
        finally:
            tr.truncation_r, tr.truncation_k, tr.repeat_rate, self.truncation_forward = saved
        tokens = torch.stack(toks, 1).contiguous()
        flat = tokens.view(B * windows, tokens.shape[2])
        content = self.decode_to_img(flat, (flat.shape[0], 256, 5, 53))
        self.train()
        return {"content": content, "content_token": tokens}

    # ---- likelihood scoring (not in the reference; DiffusionTransformer.score_tokens) ---------------------
    def _score_keywords(self, batch, condition):
        kw = dict(condition_token=condition.get("condition_token"), condition_embed=condition.get("condition_embed_token"))
        if batch.get("caption_ids") is not None:
            kw["caption_ids"] = batch["caption_ids"]
        if batch.get("seed") is not None:
            kw["seed"] = int(batch["seed"])
        return kw

    def _content_tokens(self, batch):
        """batch['content_token'], or the batch's content ('image', or 'audio' with 'audio_rate') through prepare_content"""
        tokens = batch.get("content_token")
        if tokens is None:
            tokens = self.prepare_content(batch)["content_token"]
        return torch.as_tensor(tokens).to(self.device).long()

    @torch.no_grad()
    def score_content(self, batch, timesteps=None, draws=1):
        """How well the batch's clips fit its captions: the variational bound of each clip's tokens under its caption.  batch:
        the caption as in prepare_condition and the content as 'content_token' i64[B, 265], 'image' or 'audio' (+ 'audio_rate');
        'caption_ids' / 'seed' select the noise of the forward diffusion as in generate_content (default ids 0 .. B-1).
        timesteps / draws: DiffusionTransformer.score_tokens.  Returns {'nats' f64[B] (lower = better fit), 'bits_per_token'
        f64[B] = nats / (265 ln 2), 'terms' f64[B, n_t]}."""
        import math
        condition = self.prepare_condition(batch=batch)
        tokens = self._content_tokens(batch)
        nats, terms = self.transformer.score_tokens(tokens, timesteps=timesteps, draws=draws, return_terms=True,
                                                    **self._score_keywords(batch, condition))
        return {"nats": nats, "bits_per_token": nats / (tokens.shape[1] * math.log(2.0)), "terms": terms}

    @torch.no_grad()
    def rank_captions(self, batch, captions, timesteps=None, draws=1):
        """Generative zero-shot tagging: every clip of the batch (content as in score_content; the batch needs no caption)
        scored under each of the C `captions` (a list of strings, token ids i64[C, 77] or embeddings f32[C, 77, 512]) ->
        f64[N, C] nats, lower = better fit.  Every caption of a clip is scored on the clip's own id (batch['caption_ids'],
        default 0 .. N-1) and seed: the same forward-diffused states, so a row's entries differ by the captions alone."""
        tokens = self._content_tokens(batch)
        N = tokens.shape[0]
        if isinstance(captions, (list, tuple, str)):
            condition = self.prepare_condition({self.condition_info["key"]: [captions] if isinstance(captions, str) else list(captions)})
        else:
            condition = self.prepare_condition(batch={}, condition=captions if captions.dtype != torch.long else {"condition_token": captions})
        cond_emb = self.transformer._cond(condition.get("condition_token"), condition.get("condition_embed_token"))
        C = cond_emb.shape[0]
        ids = batch.get("caption_ids")
        ids = torch.arange(N) if ids is None else torch.as_tensor(ids, dtype=torch.long).reshape(-1)
        kw = {} if batch.get("seed") is None else {"seed": int(batch["seed"])}
        nats = self.transformer.score_tokens(tokens.repeat_interleave(C, 0), condition_embed=cond_emb.repeat(N, 1, 1),
                                             timesteps=timesteps, draws=draws, caption_ids=ids.repeat_interleave(C), **kw)
        return nats.view(N, C)

    @torch.no_grad()
    def sample(self, batch, clip=None, temperature=1., return_rec=True, filter_ratio=[0, 0.5, 1.0], content_ratio=[1],
               return_att_weight=False, return_logits=False, sample_type="normal", **kwargs):
        """The trainer's logging sampler (dalle_spec.py:264-343): encode the batch's mel to tokens, optionally decode
        them back ('reconstruction_image'), and for every filter_ratio fr re-sample from those tokens diffused to
        t = int(T * fr) - 1 (fr = 0: from the all-[MASK] state) -> 'cond1_cont{cr}_fr{fr}_image'.  Only
        content_ratio = 1 is meaningful for the fixed 265-token grid (the reference slices the token sequence, which
        its own q_sample cannot take either)."""
        if return_att_weight:
            raise NotImplementedError("attention weights are never materialised on the HIP path")
        if sample_type == "debug":
            raise NotImplementedError("sample_debug is not part of the sound pipeline")
        self.eval()
        condition = self.prepare_condition(batch)
        if self.content_info["key"] not in batch and batch.get("audio") is not None:     # encode the audio once
            batch = dict(batch, **{self.content_info["key"]: self.content_image(batch)})
        content = self.prepare_content(batch)
        out = {"input_image": batch[self.content_info["key"]]}
        zshape = content["content_quant"].shape
        if return_rec:
            out["reconstruction_image"] = self.decode_to_img(content["content_token"], zshape)
        for fr in filter_ratio:
            for cr in content_ratio:
                n_tok = int(content["content_token"].shape[1] * cr)
                if n_tok < 0:
                    continue
                if n_tok != content["content_token"].shape[1] and int(self.transformer.num_timesteps * fr) > 0:
                    raise ValueError("content_ratio < 1 cannot be re-sampled: q_sample needs the whole token grid")
                trans_out = self.transformer.sample(
                    condition_token=condition.get("condition_token"), condition_mask=condition.get("condition_mask"),
                    condition_embed=condition.get("condition_embed_token"), content_token=content["content_token"][:, :n_tok],
                    filter_ratio=fr, temperature=temperature, return_att_weight=False, return_logits=return_logits,
                    content_logits=None, sample_type=sample_type, **kwargs)
                out["cond1_cont{}_fr{}_image".format(cr, fr)] = self.decode_to_img(trans_out["content_token"], zshape)
                if return_logits:
                    out["logits"] = trans_out["logits"]
        self.train()
        res = {"condition": batch.get(self.condition_info["key"])}
        res.update(out)
        return res

