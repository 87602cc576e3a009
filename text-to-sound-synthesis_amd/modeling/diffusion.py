"""Drop-in for sound_synthesis/modeling/transformers/diffusion_transformer.py:DiffusionTransformer
(sampling side), HIP-backed.

State-dict keys (log_at ... Lt_count, transformer.*), constructor keywords and the
sample()/p_sample()/predict_start() signatures follow the reference (:153-234, :269-291, :342-357,
:587-659).  The reverse loop carries token indices; one step = ds_denoiser_step (19-block denoiser +
the fused predict_start / top-r truncation / q_posterior / Gumbel-argmax tail).  The uniform noise is
drawn with torch.rand on the reference's [B, K+1, L] shape so that the same seed consumes the same
Philox stream as the reference's torch.rand_like(logits) (:360).
"""
import numpy as np

import torch
from torch import nn

from .. import _lib
from ..config import instantiate_from_config


def alpha_schedule(time_step, N=100, att_1=0.99999, att_T=0.000009, ctt_1=0.000009, ctt_T=0.9):
    """Mask-and-uniform schedule (:122-151); float64 numpy, as the reference."""
    lin = np.arange(0, time_step) / (time_step - 1)
    att = np.concatenate(([1], lin * (att_T - att_1) + att_1))
    ctt = np.concatenate(([0], lin * (ctt_T - ctt_1) + ctt_1))
    at = att[1:] / att[:-1]
    ct = 1 - (1 - ctt[1:]) / (1 - ctt[:-1])
    bt = (1 - at - ct) / N
    att = np.concatenate((att[1:], [1]))
    ctt = np.concatenate((ctt[1:], [0]))
    btt = (1 - att - ctt) / N
    return at, bt, ct, att, btt, ctt


def purity_plan(S, L, log_cumprod_ct):
    """The host-side plan of an S-step purity chain over a grid of L positions: [(t_k, R_k)], k = 0 .. S-1.
    R_k = floor((S-1-k) L / S) is the number of [MASK] positions a sample may still have after step k (R_{S-1} = 0; the reveal
    counts R_{k-1} - R_k differ by at most one).  t_k, the timestep the network is told, is the one at which the forward process
    has masked, in expectation, the share of the grid that is still masked: argmin_t |exp(log_cumprod_ct[t]) - R_{k-1} / L|
    with R_{-1} = L, ties to the larger t, forced non-increasing, t_0 = T - 1.  log_cumprod_ct: the model's buffer of T + 1
    entries (tensor, array or list); entry T is the wrap-around slot of t = -1, not a timestep, and is not searched.
    1 <= S <= L, else ValueError.  Pure host arithmetic in float64."""
    S, L = int(S), int(L)
    if S < 1:
        raise ValueError("a purity chain has at least one step, got S = %d" % S)
    if S > L:
        raise ValueError("a purity chain reveals at least one position per step: S = %d exceeds the %d grid positions" % (S, L))
    lc = log_cumprod_ct.detach().cpu().numpy() if torch.is_tensor(log_cumprod_ct) else log_cumprod_ct
    gamma = np.exp(np.asarray(lc, dtype=np.float64).reshape(-1)[:-1])
    T = gamma.shape[0]
    if T < 1:
        raise ValueError("log_cumprod_ct must have T + 1 entries with T >= 1")
    plan, prev_r, prev_t = [], L, T - 1
    for k in range(S):
        d = np.abs(gamma - prev_r / L)
        t = T - 1 if k == 0 else min(prev_t, int(np.nonzero(d == d.min())[0].max()))
        r = ((S - 1 - k) * L) // S
        plan.append((t, r))
        prev_r, prev_t = r, t
    return plan


def score_plan(T, n=None):
    """The timesteps and weights of a likelihood score -> (timesteps, weights), two lists.
    n None or T: every timestep 0 .. T-1 with weight 1 -- the full variational bound, T forwards per clip.
    2 <= n < T: t = 0 with weight 1 (the decoder term is not interpolated) and n - 1 distinct timesteps, the midpoints of n - 1
    equal strata of 1 .. T-1 (t_k = 1 + floor((2k + 1)(T - 1) / (2(n - 1)))), each with weight (T - 1) / (n - 1): the weights
    sum to T.  Anything else raises ValueError.  Pure host arithmetic."""
    T = int(T)
    if T < 1:
        raise ValueError("a diffusion has at least one timestep, got T = %r" % (T,))
    if n is None or (not isinstance(n, bool) and isinstance(n, (int, np.integer)) and int(n) == T):
        return list(range(T)), [1.0] * T
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 2 <= int(n) < T:
        raise ValueError("timesteps must be None, T = %d, or an integer in 2 .. %d, got %r" % (T, T - 1, n))
    n = int(n)
    ts = [0] + [1 + ((2 * k + 1) * (T - 1)) // (2 * (n - 1)) for k in range(n - 1)]
    return ts, [1.0] + [(T - 1) / (n - 1)] * (n - 1)


def _log_1_min_a(a):
    return torch.log(1 - a.exp() + 1e-40)


class DiffusionTransformer(nn.Module):
    def __init__(self, *, content_emb_config=None, condition_emb_config=None, transformer_config=None,
                 diffusion_step=100, alpha_init_type="cos", auxiliary_loss_weight=0,
                 adaptive_auxiliary_loss=False, mask_weight=[1, 1]):
        super().__init__()
        self.condition_emb = instantiate_from_config(condition_emb_config)  # CLIP text: SURVEY 8(f)-1
        transformer_config = dict(transformer_config)
        transformer_config["params"] = dict(transformer_config["params"])
        transformer_config["params"]["diffusion_step"] = diffusion_step
        transformer_config["params"]["content_emb_config"] = content_emb_config
        self.transformer = instantiate_from_config(transformer_config)
        self.content_seq_len = transformer_config["params"]["content_seq_len"]
        self.num_classes = self.transformer.content_emb.num_embed  # K + 1
        self.shape = self.content_seq_len
        self.num_timesteps = diffusion_step
        self.parametrization = "x0"
        self.loss_type = "vb_stochastic"
        self.auxiliary_loss_weight = auxiliary_loss_weight
        self.adaptive_auxiliary_loss = adaptive_auxiliary_loss
        self.mask_weight = mask_weight
        self.truncation_r = None  # set by DALLE.generate_content from sample_type "top{r}r"
        self.truncation_k = None  # ... or "top{k}p" (top-k, dalle_spec.py:147-157); exclusive with truncation_r
        self.repeat_rate = None   # "q{rate}": repeat a step with this probability (dalle_spec.py:135-143)
        # Noise source of the samplers.  "torch" (default): torch.rand((B, K+1, L)) per call on the model's device, the
        # reference's own draw (log_sample_categorical, :359-368) -- same seed, same device => same stream, but what a
        # caption draws depends on the batch around it.  "philox" (or passing caption_ids to sample()): the uniforms are
        # drawn inside the sampler kernel from a counter-based stream keyed by (sample_seed, global caption id, call,
        # position, class) -- a caption's NOISE no longer depends on batch size, batch position or rank (SURVEY.md
        # section 8e), no noise tensor exists, and the whole chain is enqueued by one C call (ds_denoiser_sample_rng).
        # Its tokens are identical across batches as long as the same GEMM program serves the local batch size (the
        # per-sample, half-tile and 4-wave programs agree to ~1e-7 relative on rows 256..264, not bit for bit -- csrc/api.hip
        # rows_per_sample -- so a near-tie can fall differently between, say, one batch of 64 and 8 shards of 8).
        self.rng_mode = "torch"
        self.sample_seed = 1234
        assert alpha_init_type == "alpha1", "Diffsound uses alpha_init_type='alpha1'"
        at, bt, ct, att, btt, ctt = alpha_schedule(self.num_timesteps, N=self.num_classes)
        f64 = lambda x: torch.tensor(x.astype("float64"))
        log_at, log_bt, log_ct = torch.log(f64(at)), torch.log(f64(bt)), torch.log(f64(ct))
        log_cat, log_cbt, log_cct = torch.log(f64(att)), torch.log(f64(btt)), torch.log(f64(ctt))
        for name, v in (("log_at", log_at), ("log_bt", log_bt), ("log_ct", log_ct),
                        ("log_cumprod_at", log_cat), ("log_cumprod_bt", log_cbt), ("log_cumprod_ct", log_cct),
                        ("log_1_min_ct", _log_1_min_a(log_ct)),
                        ("log_1_min_cumprod_ct", _log_1_min_a(log_cct))):
            self.register_buffer(name, v.float())
        self.register_buffer("Lt_history", torch.zeros(self.num_timesteps))
        self.register_buffer("Lt_count", torch.zeros(self.num_timesteps))
        self._sched = None

    @property
    def device(self):
        return self.log_at.device

    def _schedule_table(self):
        """[8][T+1] table consumed by ds_sample_tail (rows: log_at, log_bt, log_ct, log_1_min_ct,
        log_cumprod_at, log_cumprod_bt, log_cumprod_ct, log_1_min_cumprod_ct)."""
        if self._sched is None or self._sched.device != self.log_at.device:
            T = self.num_timesteps
            tab = torch.zeros(8, T + 1, device=self.log_at.device, dtype=torch.float32)
            for i, n in enumerate(("log_at", "log_bt", "log_ct", "log_1_min_ct")):
                tab[i, :T] = getattr(self, n)
            for i, n in enumerate(("log_cumprod_at", "log_cumprod_bt", "log_cumprod_ct", "log_1_min_cumprod_ct")):
                tab[4 + i] = getattr(self, n)
            self._sched = tab
        return self._sched

    # ---- pieces with the reference's signatures (log-one-hot in / out) ------------------------------
    @torch.no_grad()
    def _tail(self, logits_rows, x_t, t, u, initial, want):
        """Run ds_sample_tail on row-major logits; `want` selects debug dumps."""
        B, L, K = x_t.shape[0], self.content_seq_len, self.num_classes - 1
        dev = logits_rows.device
        dump = {k: torch.empty(B, K + 1, L, device=dev) for k in want}
        out = torch.empty(B, L, device=dev, dtype=torch.long)
        r, k = self._truncation()
        _lib.check(_lib.lib().ds_sample_tail_ex(
            _lib.ptr(logits_rows), _lib.ptr(x_t), _lib.ptr(t), _lib.ptr(u), _lib.ptr(self._schedule_table()),
            _lib.ptr(out), _lib.ptr(dump.get("log_pred")), _lib.ptr(dump.get("trunc")), _lib.ptr(dump.get("post")),
            B, L, K, self.num_timesteps, int(initial), r, k, _lib.stream()))
        return out, dump

    def _truncation(self):
        """(trunc_r, trunc_k) for the C ABI: top-k wins if set (the reference installs exactly one wrapper)."""
        if self.truncation_k is not None:
            return -1.0, int(self.truncation_k)
        return (-1.0 if self.truncation_r is None else float(self.truncation_r)), 0

    @staticmethod
    def _is_initial(log_x):
        return bool(torch.isinf(log_x[:, :-1]).all().item())

    @torch.no_grad()
    def step_detail(self, x_t, cond_emb, t, u, initial):
        """Teacher-forced single step on token indices: returns (tokens, {log_pred, trunc, post})."""
        tr = self.transformer
        p = tr.packed(self._schedule_table())
        B = x_t.shape[0]
        x_t, t, u = x_t.contiguous(), t.to(x_t.device).contiguous(), u.contiguous()
        kv = tr.condition_kv(cond_emb, self._schedule_table())
        logits = torch.empty(B * self.content_seq_len, self.num_classes - 1, device=x_t.device)
        _lib.check(_lib.lib().ds_denoiser_forward(p["handle"], _lib.ptr(x_t), _lib.ptr(t), _lib.ptr(kv), B,
                                                  _lib.ptr(tr.workspace(B, self._schedule_table())),
                                                  _lib.ptr(logits), 0, _lib.stream()))
        return self._tail(logits, x_t, t, u, initial, ("log_pred", "trunc", "post"))

    @torch.no_grad()
    def predict_start(self, log_x_t, cond_emb, t):
        """p(x0 | xt) as clamped log-probs [B, K+1, L] (:269-291); with truncation_r set this is the
        reference's truncation-wrapped predict_start (dalle_spec.py:158-174)."""
        x_t = log_x_t.argmax(1)
        u = torch.full((x_t.shape[0], self.num_classes, self.content_seq_len), 0.5, device=x_t.device)
        _, d = self.step_detail(x_t, cond_emb, t, u, self._is_initial(log_x_t))
        return d["trunc"] if (self.truncation_r is not None or self.truncation_k is not None) else d["log_pred"]

    @torch.no_grad()
    def p_sample(self, log_x, cond_emb, t):
        """One reverse step on the reference's log-one-hot state (:353-357)."""
        x_t = log_x.argmax(1)
        u = torch.rand((x_t.shape[0], self.num_classes, self.content_seq_len), device=x_t.device)
        tok = self.p_sample_tokens(x_t, self.transformer.condition_kv(cond_emb, self._schedule_table()), t, u,
                                   self._is_initial(log_x))
        oh = torch.nn.functional.one_hot(tok, self.num_classes).permute(0, 2, 1).float()
        return torch.log(oh.clamp(min=1e-30))

    def _seed(self, seed):
        return int(self.sample_seed if seed is None else seed)

    def _result(self, x, return_logits):
        out = {"content_token": x}
        if return_logits:
            out["logits"] = torch.nn.functional.one_hot(x, self.num_classes).permute(0, 2, 1).float()
        return out

    def _step_entry(self, chain, noise, B, initial, hold, guide, slot=0):
        """The C entry of one reverse step (chain False: ds_denoiser_step_*) or of a whole chain (True: ds_denoiser_sample_*)
        and the arguments its forms share.  noise: the uniforms u, or (caption_ids, call, seed) for the in-kernel Philox draw;
        hold: None or (keep, known, mode) -- plain and held are different entries; guide: None, (kv2, scale, tokens2), or
        the composed form (kvN, None, tokensN, weights, C) of caption tracks (_guide_start).
        Returns (entry, the noise arguments, the arguments from B to the workspace); the caller's part is what comes
        before (handle, tokens, timesteps, kv) and after (the step's output tokens, the stream)."""
        rng = isinstance(noise, tuple)
        composed = guide is not None and len(guide) == 5
        family = "_composed" if composed else "_guided" if guide is not None else "_hold" if hold is not None else ""
        name = "ds_denoiser_%s%s%s" % ("sample" if chain else "step", family, "_rng" if rng else "" if family else "_ex")
        r, k = self._truncation()
        args = [B, 0 if hold is not None else int(initial), r, k]
        if composed:
            args += [int(guide[4]), _lib.ptr(guide[3])]
        elif guide is not None:
            args.append(float(guide[1]))
        if family:
            keep, known, mode = hold if hold is not None else (None, None, 0)
            args += [_lib.ptr(keep), _lib.ptr(known), int(mode)]
        if guide is not None:
            args.append(_lib.ptr(guide[2]))
        args.append(_lib.ptr(self.transformer.workspace(self._n_cond(guide) * B, self._schedule_table(), slot)))
        noise = [_lib.ptr(noise[0]), self._seed(noise[2]), int(noise[1])] if rng else [_lib.ptr(noise)]
        return getattr(_lib.lib(), name), noise, args

    @staticmethod
    def _n_cond(guide):
        """conditions per clip of a step: 1 unguided, 2 guided, C + 1 with C caption tracks"""
        return 1 if guide is None else guide[4] + 1 if len(guide) == 5 else 2

    def _p_sample(self, x_t, kv, t, noise, initial, out, t_post, slot, hold, guide):
        p = self.transformer.packed(self._schedule_table())
        if out is None:
            out = torch.empty_like(x_t)
        if guide is not None:                        # (named: alive until the launch is enqueued)
            n = self._n_cond(guide)
            kv, t, t_post = guide[0], t.repeat(n), None if t_post is None else t_post.repeat(n)
        entry, noise, args = self._step_entry(False, noise, x_t.shape[0], initial, hold, guide, slot)
        _lib.check(entry(p["handle"], _lib.ptr(x_t), _lib.ptr(t), _lib.ptr(t_post), _lib.ptr(kv), *noise, *args, _lib.ptr(out),
                         _lib.stream()))
        return out

    @torch.no_grad()
    def p_sample_tokens(self, x_t, kv, t, u, initial, out=None, t_post=None, slot=0, hold=None, guide=None):
        """x_t i64[B,L] -> x_{t-1} i64[B,L]; kv from transformer.condition_kv().  t_post: the posterior's timestep
        vector when it differs from the network's (sample_fast).  hold: (keep u8[B,L], known i64[B,L], mode) of the
        region-held step (_hold_start); on caller uniforms only mode 0 (clamp) exists.  guide: (kv2, scale, tokens2) of
        the guided step (_guide_start: the K/V of captions + null conditions at batch 2B, the guidance scale, an
        i64[2B,L] scratch) or its composed form (kvN, None, tokensN, weights, C) for C caption tracks; kv is not read then."""
        return self._p_sample(x_t, kv, t, u, initial, out, t_post, slot, hold, guide)

    @torch.no_grad()
    def p_sample_tokens_rng(self, x_t, kv, t, caption_ids, call, initial, out=None, t_post=None, slot=0, seed=None,
                            hold=None, guide=None):
        """p_sample_tokens with the noise drawn in the kernel: Philox stream of (seed, caption_ids[b], call).  hold and
        guide as in p_sample_tokens, mode 1 (renoise) included."""
        return self._p_sample(x_t, kv, t, (caption_ids, call, seed), initial, out, t_post, slot, hold, guide)

    def _caption_ids(self, caption_ids, B, device):
        """i64[B] global caption ids on the device (default: 0 .. B-1)."""
        if caption_ids is None:
            return torch.arange(B, device=device, dtype=torch.long)
        on_device = torch.is_tensor(caption_ids) and caption_ids.device.type == device.type == "cuda"
        ids = torch.as_tensor(caption_ids, dtype=torch.long)
        if ids.shape != (B,):
            raise ValueError("caption_ids must have one entry per caption: got %s for a batch of %d" % (tuple(ids.shape), B))
        # The range is checked on host lists / CPU tensors every time (it costs nothing there), and on a DEVICE tensor the
        # first time that very tensor OBJECT is seen at its current version (one host synchronisation; remembered through a
        # weak reference to the object, so an id tensor re-used across sample() calls -- bench.py's timed loop -- is checked
        # once, a modified one again, and a NEW tensor that the caching allocator happens to put at the same address is not
        # mistaken for the checked one).  An id outside [0, 2^32) would be truncated into the Philox counter and could share
        # a noise stream with another caption.
        seen = getattr(self, "_gids_checked", None)
        known = on_device and seen is not None and seen[0]() is caption_ids and seen[1] == caption_ids._version
        if B > 0 and not known:
            if int(ids.min()) < 0 or int(ids.max()) >= 2 ** 32:
                raise ValueError("caption ids must be in [0, 2^32)")
            if on_device:
                import weakref
                self._gids_checked = (weakref.ref(caption_ids), caption_ids._version)
        return ids.to(device).contiguous()

    def _cond(self, condition_token, condition_embed):
        if self.condition_emb is not None and condition_token is not None:
            return self.condition_emb(condition_token).float()          # CLIP text tower (:619-621)
        if condition_embed is None:
            raise ValueError("pass condition_token (with a condition_emb module) or condition_embed [B,77,512]")
        return condition_embed.float()

    # ---- training loss: the forward value (the step with gradients is modeling/train.py) ----
    def sample_time(self, b, device, method="uniform", generator=None):
        """Timesteps for a batch and their sampling probabilities (:379-406): importance sampling by sqrt(Lt_history)
        once every timestep has been seen more than 10 times, uniform before.  generator: optional torch.Generator of
        `device` (the reference draws from the global one)."""
        if method == "importance":
            # (Lt_count only grows -- scatter_add of ones --, so once every timestep has been seen 11 times the test stays
            # true: it is read from the device until then, one host synchronisation per call, and never again.  A state-dict
            # load or a manual reset of the statistics clears the memo: _load_from_state_dict / reset_time_statistics.)
            if not getattr(self, "_lt_all_seen", False):
                if not (self.Lt_count > 10).all():
                    return self.sample_time(b, device, method="uniform", generator=generator)
                self._lt_all_seen = True
            lt_sqrt = torch.sqrt(self.Lt_history + 1e-10) + 0.0001
            lt_sqrt[0] = lt_sqrt[1]
            pt_all = lt_sqrt / lt_sqrt.sum()
            t = torch.multinomial(pt_all, num_samples=b, replacement=True, generator=generator)
            return t, pt_all.gather(dim=0, index=t)
        if method == "uniform":
            t = torch.randint(0, self.num_timesteps, (b,), device=device, generator=generator).long()
            return t, torch.ones_like(t).float() / self.num_timesteps
        raise ValueError(method)

    def reset_time_statistics(self):
        """Zero the importance-sampling statistics (:88-89) and forget that every timestep had been seen."""
        self.Lt_history.zero_()
        self.Lt_count.zero_()
        self._lt_all_seen = False

    def _load_from_state_dict(self, *args, **kwargs):
        self._lt_all_seen = False
        return super()._load_from_state_dict(*args, **kwargs)

    @torch.no_grad()
    def _train_loss(self, x, cond_emb, is_train=True, noise=None):
        """(log_model_prob [B, K+1, L], vb_loss [B]) of :408-476, computed forward-only on the HIP path: ds_q_sample,
        the denoiser, and ds_loss_tail for the per-position KL / NLL / auxiliary-KL terms.  Updates Lt_history /
        Lt_count like the reference (the accuracy bookkeeping lists :425-436 are logging only and not kept).
        noise: optional f32[B, K+1, L] uniforms for q_sample (tests)."""
        B, L, K1, T = x.shape[0], self.content_seq_len, self.num_classes, self.num_timesteps
        dev = x.device
        t, pt = self.sample_time(B, dev, "importance")
        t, pt = t.to(dev), pt.to(dev)
        u = torch.rand((B, K1, L), device=dev) if noise is None else noise.to(dev)
        x = x.contiguous()
        xt = self.q_sample_tokens(x, t, u)
        tr = self.transformer
        sched = self._schedule_table()
        p = tr.packed(sched)
        kv = tr.condition_kv(cond_emb, sched)
        logits = torch.empty(B * L, K1 - 1, device=dev)
        _lib.check(_lib.lib().ds_denoiser_forward(p["handle"], _lib.ptr(xt), _lib.ptr(t), _lib.ptr(kv), B,
                                                  _lib.ptr(tr.workspace(B, sched)), _lib.ptr(logits), 0, _lib.stream()))
        kl, nll, kl_aux = (torch.empty(B, L, device=dev) for _ in range(3))
        log_model_prob = torch.empty(B, K1, L, device=dev)
        _lib.check(_lib.lib().ds_loss_tail(_lib.ptr(logits), _lib.ptr(x), _lib.ptr(xt), _lib.ptr(t),
                                           _lib.ptr(sched), _lib.ptr(kl), _lib.ptr(nll), _lib.ptr(kl_aux),
                                           _lib.ptr(log_model_prob), B, L, K1 - 1, T, _lib.stream()))
        mask_region = (xt == K1 - 1).float()
        weight = mask_region * self.mask_weight[0] + (1.0 - mask_region) * self.mask_weight[1]
        is0 = (t == 0).float()
        decoder_nll = nll.sum(-1)
        kl_loss = is0 * decoder_nll + (1.0 - is0) * (kl * weight).sum(-1)
        lt2 = kl_loss.pow(2)
        self.Lt_history.scatter_(dim=0, index=t, src=(0.1 * lt2 + 0.9 * self.Lt_history.gather(dim=0, index=t)))
        self.Lt_count.scatter_add_(dim=0, index=t, src=torch.ones_like(lt2))
        vb_loss = kl_loss / pt
        if self.auxiliary_loss_weight != 0 and is_train:
            kl_aux_loss = is0 * decoder_nll + (1.0 - is0) * (kl_aux * weight).sum(-1)
            w = t.float() / T + 1.0 if self.adaptive_auxiliary_loss else 1.0
            vb_loss = vb_loss + w * self.auxiliary_loss_weight * kl_aux_loss / pt
        return log_model_prob, vb_loss

    @torch.no_grad()
    def forward(self, input, return_loss=False, return_logits=True, return_att_weight=False, is_train=True, **kwargs):
        """{'logits': exp(log_model_prob), 'loss': scalar} as :539-577.  The loss is a forward value for evaluation / loss
        parity; optimisation enters through `Solver.step(batch)` / `TrainStep` (modeling/train.py: the hand-written backward)."""
        x = input["content_token"]
        cond_emb = self._cond(input.get("condition_token"), input.get("condition_embed_token")).to(x.device)
        out = {}
        if is_train:
            log_model_prob, loss = self._train_loss(x, cond_emb, noise=kwargs.get("noise"))
            loss = loss.sum() / (x.shape[0] * x.shape[1])
            if return_logits:
                out["logits"] = torch.exp(log_model_prob)
            if return_loss:
                out["loss"] = loss
        return out

    @torch.no_grad()
    def q_sample_tokens(self, x0, t, u):
        """x_t ~ q(x_t | x_0) on token ids (q_sample, :370-377); u f32[B, K+1, L] uniforms."""
        x0_c, t_c, u_c = x0.contiguous(), t.contiguous(), u.contiguous()   # named: alive until the launch is enqueued
        out = torch.empty_like(x0_c)
        _lib.check(_lib.lib().ds_q_sample(_lib.ptr(x0_c), _lib.ptr(t_c), _lib.ptr(u_c),
                                          _lib.ptr(self._schedule_table()), _lib.ptr(out), x0_c.shape[0],
                                          self.content_seq_len, self.num_classes - 1, self.num_timesteps,
                                          _lib.stream()))
        return out

    @torch.no_grad()
    def q_sample(self, log_x_start, t):
        """The reference's log-one-hot form of the forward diffusion (:370-377): log_x_start f32[B, K+1, L] one-hot in
        log space -> a log-one-hot sample of q(x_t | x_0), drawing torch.rand of the same shape as the reference."""
        x0 = log_x_start.argmax(1)
        u = torch.rand(tuple(log_x_start.shape), device=x0.device)
        xt = self.q_sample_tokens(x0, t.to(x0.device), u)
        oh = torch.nn.functional.one_hot(xt, self.num_classes).permute(0, 2, 1).float()
        return torch.log(oh.clamp(min=1e-30))

    KEEP_MODES = {"clamp": 0, "renoise": 1}

    def _hold_start(self, keep_mask, keep_mode, content_token, B, noise_fn, caption_ids, seed):
        """Region-held sampling (inpainting / continuation): keep_mask bool[B, L] (True = held), content_token supplies the
        held tokens.  Returns (hold, start tokens, caption ids): hold = (keep u8, known i64, mode) for the *_hold entries.
        clamp: the start state is known where held, [MASK] elsewhere.  renoise: the held positions follow the forward
        process -- they start from q_sample(known, T - 1) on stream 1 of the caption's Philox draws (call 0), and reverse
        call k (Philox call k + 1 on both streams) re-draws them at that call's posterior timestep minus one; this mode
        exists with in-kernel noise only, so it always samples per caption (caption_ids default 0 .. B-1)."""
        if keep_mode not in self.KEEP_MODES:
            raise ValueError("keep_mode is 'clamp' or 'renoise', got %r" % (keep_mode,))
        if content_token is None:
            raise ValueError("keep_mask holds positions of given content: pass content_token i64[B, %d]" % self.content_seq_len)
        device, L, K = self.device, self.content_seq_len, self.num_classes - 1
        known = content_token.to(device).long().contiguous()
        keep = torch.as_tensor(keep_mask).to(device)
        if tuple(known.shape) != (B, L) or tuple(keep.shape) != (B, L):
            raise ValueError("keep_mask and content_token must be [%d, %d]: got %s and %s"
                             % (B, L, tuple(keep.shape), tuple(known.shape)))
        keep = keep != 0
        mode = self.KEEP_MODES[keep_mode]
        if mode == 0:
            x = torch.where(keep, known, torch.full_like(known, K))
        else:
            if noise_fn is not None:
                raise ValueError("keep_mode='renoise' draws the held positions' noise inside the kernel: not with noise_fn")
            caption_ids = self._caption_ids(caption_ids, B, device)
            t = torch.full((B,), self.num_timesteps - 1, device=device, dtype=torch.long)
            xs = torch.empty_like(known)
            _lib.check(_lib.lib().ds_q_sample_rng(_lib.ptr(known), _lib.ptr(t), _lib.ptr(caption_ids),
                                                  self._seed(seed), 0,
                                                  _lib.ptr(self._schedule_table()), _lib.ptr(xs), B, L, K,
                                                  self.num_timesteps, _lib.stream()))
            x = torch.where(keep, xs, torch.full_like(known, K))
        return (keep.to(torch.uint8).contiguous(), known, mode), x, caption_ids

    def _guide(self, guidance_scale, null_condition_embed, cond_emb):
        """Classifier-free guidance of sample() / sample_fast(): None (today's path, no null forward) for a scale of None
        or exactly 1, else (null embeddings f32[B,77,512] on the model's device, scale).  null_condition_embed is
        f32[77,512], broadcast over the batch, or f32[B,77,512] (DALLE.null_condition)."""
        if guidance_scale is None or float(guidance_scale) == 1.0:
            return None
        scale = float(guidance_scale)
        if scale != scale or scale in (float("inf"), float("-inf")):
            raise ValueError("guidance_scale must be finite, got %r" % (guidance_scale,))
        if null_condition_embed is None:
            raise ValueError("guidance_scale = %g needs the null condition: pass null_condition_embed f32[77,512] or "
                             "[B,77,512] (DALLE.null_condition())" % scale)
        null = torch.as_tensor(null_condition_embed).float()
        want = tuple(cond_emb.shape)
        if null.dim() == 2:
            null = null[None].expand(want[0], -1, -1)
        if tuple(null.shape) != want:
            raise ValueError("null_condition_embed must be %s or %s: got %s"
                             % (want[1:], want, tuple(torch.as_tensor(null_condition_embed).shape)))
        return null.to(self.device), scale

    MAX_TRACKS = 4       # DS_MAX_TRACKS (include/diffsound_hip.h)

    def _tracks(self, track_embed, track_weight, null_condition_embed, guidance_scale):
        """Caption tracks of sample() / sample_fast(): None when both keywords are None (today's path), else
        (null f32[B,77,512], weights f32[B,C,L], embeds f32[C,B,77,512]) on the model's device -- the `guide` of the composed
        entries.  Every rule that can be checked on the host is, before anything runs; the weights' finiteness is one of
        them (the C layer cannot see device values without a synchronisation)."""
        if track_embed is None and track_weight is None:
            return None
        if track_embed is None or track_weight is None:
            raise ValueError("caption tracks need both track_embed f32[C,B,77,512] and track_weight f32[B,C,%d]"
                             % self.content_seq_len)
        if guidance_scale is not None:
            raise ValueError("caption tracks carry their own weights: guidance_scale must be None with track_embed")
        emb, w = torch.as_tensor(track_embed).float(), torch.as_tensor(track_weight).float()
        if emb.dim() != 4 or not 1 <= emb.shape[0] <= self.MAX_TRACKS:
            raise ValueError("track_embed must be f32[C,B,77,512] with 1 <= C <= %d: got %s" % (self.MAX_TRACKS, tuple(emb.shape)))
        C, B = emb.shape[0], emb.shape[1]
        if tuple(w.shape) != (B, C, self.content_seq_len):
            raise ValueError("track_weight must be f32[B,C,%d] = %s for track_embed %s: got %s"
                             % (self.content_seq_len, (B, C, self.content_seq_len), tuple(emb.shape), tuple(w.shape)))
        if not bool(torch.isfinite(w).all()):
            raise ValueError("track_weight must be finite")
        if null_condition_embed is None:
            raise ValueError("caption tracks need the null condition: pass null_condition_embed f32[77,512] or [B,77,512] "
                             "(DALLE.null_condition())")
        null, _ = self._guide(0.0, null_condition_embed, emb[0])
        return null, w.to(self.device).contiguous(), emb.to(self.device)

    def _cond_guide(self, condition_token, condition_embed, guidance_scale, null_condition_embed, track_embed, track_weight):
        """(cond_emb, guide) of sample() / sample_fast(): with caption tracks the guide is _tracks' and cond_emb, which then
        only gives the batch its size, is track 0's embeddings (condition_embed may be None)."""
        tracks = self._tracks(track_embed, track_weight, null_condition_embed, guidance_scale)
        if tracks is not None:
            return tracks[2][0], tracks
        cond_emb = self._cond(condition_token, condition_embed)
        return cond_emb, self._guide(guidance_scale, null_condition_embed, cond_emb)

    def _guide_start(self, guide, cond_emb, sched):
        """(kv2, scale, tokens2) of the guided entries: the cross-attention K/V at batch 2B of the captions followed by the
        null conditions, and the scratch that receives the duplicated tokens of every step.  A 3-tuple of _tracks gives the
        composed entries' (kvN, None, tokensN, weights, C): K/V at batch (C+1)B, track-major, the null conditions last."""
        B = cond_emb.shape[0]
        if len(guide) == 3:
            null, weights, emb = guide
            C = emb.shape[0]
            kvn = self.transformer.condition_kv(torch.cat((emb.reshape(C * B, *emb.shape[2:]), null), 0).contiguous(), sched)
            return kvn, None, torch.empty((C + 1) * B, self.content_seq_len, device=self.device, dtype=torch.long), weights, C
        null, scale = guide
        kv2 = self.transformer.condition_kv(torch.cat((cond_emb.float(), null), 0).contiguous(), sched)
        return kv2, scale, torch.empty(2 * B, self.content_seq_len, device=self.device, dtype=torch.long)

    def _reverse(self, *args, **kwargs):
        """_reverse_once under the denoiser's range guard (Text2ImageTransformer.range_exceeded): a chain during which FC2's
        split operand saturated is run again from its start in the fp32 mode, with the state of Python's `random` (the repeat
        sampler) and of the device's generator (the torch.rand noise) put back first; the Philox noise needs neither."""
        return self._guarded(self._reverse_once, *args, **kwargs)

    def _guarded(self, chain, *args, **kwargs):
        """chain(*args, **kwargs) under the range guard described in _reverse"""
        import random
        tr = self.transformer
        tr.packed(self._schedule_table())
        if tr._packed.get("range_peak") is None:
            return chain(*args, **kwargs)
        state, gen = random.getstate(), torch.cuda.get_rng_state(self.device)
        tr.range_exceeded()                                 # clear what earlier calls left
        out = chain(*args, **kwargs)
        if not tr.range_exceeded():
            return out
        random.setstate(state)
        torch.cuda.set_rng_state(gen, self.device)
        with tr.strict_mode():
            return chain(*args, **kwargs)

    def _reverse_once(self, cond_emb, steps, noise_fn, return_logits, start_tokens=None, caption_ids=None, seed=None, hold=None,
                      guide=None):
        """guide: (null embeddings, scale) of _guide -- every call then runs one forward at batch 2B and the guided tail.
        steps: list of (t, t_post) pairs, first one from the all-[MASK] state (or from start_tokens, already
        diffused to the first t).  hold: (keep, known, mode) of _hold_start -- every call then runs the region-held
        kernels and start_tokens is the mixed start state.  The 'q' repeat sampler
        (dalle_spec.py:135-143: with probability `repeat_rate` a step is applied twice at the same t) draws from
        Python's `random` exactly like the reference's wrapper: one random.random() per step."""
        import random
        device = self.device
        B = cond_emb.shape[0]
        K1, L = self.num_classes, self.content_seq_len
        cond_emb = cond_emb.to(device)
        if start_tokens is None:
            x = torch.full((B, L), K1 - 1, device=device, dtype=torch.long)  # all [MASK]
        else:
            x = start_tokens.to(device).clone()
        sched = self._schedule_table()
        if guide is not None:
            kv, guide = None, self._guide_start(guide, cond_emb, sched)
        else:
            kv = self.transformer.condition_kv(cond_emb.contiguous(), sched)
        nxt = torch.empty_like(x)
        if noise_fn is None and (caption_ids is not None or self.rng_mode == "philox"):
            # in-kernel noise: the whole chain is one C call, nothing returns to Python between steps
            calls = []
            for step, step_post in steps:
                reps = 2 if (self.repeat_rate is not None and random.random() < self.repeat_rate) else 1
                calls += [(step, step_post)] * reps
            p = self.transformer.packed(sched)
            gids = self._caption_ids(caption_ids, B, device)
            t_steps = torch.tensor(calls, dtype=torch.long, device=device).view(-1, 2, 1)
            t_steps = t_steps.expand(-1, 2, self._n_cond(guide) * B).contiguous()
            call0 = 1 if hold is not None and hold[2] == 1 else 0   # renoise: stream-1 call 0 was the start state's q_sample
            entry, noise, args = self._step_entry(True, (gids, call0, seed), B, start_tokens is None, hold, guide)
            _lib.check(entry(p["handle"], _lib.ptr(x), _lib.ptr(nxt), _lib.ptr(t_steps), len(calls),
                             _lib.ptr(kv if guide is None else guide[0]), *noise, *args, _lib.stream()))
            return self._result(x, return_logits)
        calls = 0
        for i, (step, step_post) in enumerate(steps):
            repeats = 2 if (self.repeat_rate is not None and random.random() < self.repeat_rate) else 1
            for rep in range(repeats):
                # the reference's draw: torch.rand_like(logits) on a [B, K+1, L] fp32 tensor of the model's device
                # (diffusion_transformer.py:359-368) -- torch.rand of that shape consumes the generator identically
                u = noise_fn(step if self.repeat_rate is None else calls, (B, K1, L)).to(device) \
                    if noise_fn is not None else torch.rand((B, K1, L), device=device)
                u = u.contiguous()
                calls += 1
                t = torch.full((B,), step, device=device, dtype=torch.long)
                tp = None if step_post == step else torch.full((B,), step_post, device=device, dtype=torch.long)
                kw = {} if guide is None else {"guide": guide}      # (unguided: the call as it always was)
                self.p_sample_tokens(x, kv, t, u, initial=(start_tokens is None and i == 0 and rep == 0), out=nxt, t_post=tp,
                                     hold=hold, **kw)
                x, nxt = nxt, x
        return self._result(x, return_logits)

    @torch.no_grad()
    def sample(self, condition_token, condition_mask, condition_embed, content_token=None, filter_ratio=0.5,
               temperature=1.0, return_att_weight=False, return_logits=False, content_logits=None,
               print_log=True, noise_fn=None, caption_ids=None, seed=None, keep_mask=None, keep_mode="clamp",
               guidance_scale=None, null_condition_embed=None, track_embed=None, track_weight=None, **kwargs):
        """Reverse diffusion from the all-[MASK] state (:587-659, filter_ratio == 0 branch).

        noise_fn(step, shape) may supply the uniforms (tests inject the oracle's noise; with the 'q' repeat sampler
        active the first argument is the running p_sample call index instead of the timestep).  caption_ids (i64[B],
        global caption indices) selects the in-kernel per-caption noise (see rng_mode); seed overrides sample_seed.

        keep_mask (bool[B, L], True = held; not in the reference): region-held sampling -- the held positions carry
        content_token's tokens through the whole chain as context of the denoiser, the others are generated from [MASK]
        (filter_ratio must resolve to step 0).  keep_mode "clamp" keeps them clean, "renoise" lets them follow the forward
        process (_hold_start).  The held TOKENS of the result are exactly content_token's.

        guidance_scale (not in the reference): classifier-free guidance -- every step evaluates the denoiser under the
        caption and under null_condition_embed (f32[77,512] or [B,77,512]) in one forward at batch 2B and samples from
        the renormalised mix  log p_null + scale (log p_caption - log p_null)  (csrc/sampler.hip SampleGuide).  None or
        exactly 1: today's path, untouched, no null forward.

        track_embed f32[C,B,77,512] / track_weight f32[B,C,L] (not in the reference): caption tracks -- C <= 4 captions per
        clip, each weighted per grid position; every step evaluates the denoiser under each of them and under
        null_condition_embed in one forward at batch (C+1)B and samples from the renormalised mix
        log p_null + sum_i w_i(pos) (log p_i - log p_null)  (csrc/sampler.hip SampleCompose).  guidance_scale must be None,
        condition_embed may be; both None: today's path, untouched."""
        cond_emb, guide = self._cond_guide(condition_token, condition_embed, guidance_scale, null_condition_embed, track_embed,
                                           track_weight)
        T = self.num_timesteps
        start_step = int(T * filter_ratio)
        if keep_mask is not None:
            if start_step != 0:
                raise ValueError("keep_mask samples the free positions from [MASK]: filter_ratio must resolve to step 0")
            hold, x, caption_ids = self._hold_start(keep_mask, keep_mode, content_token, cond_emb.shape[0], noise_fn,
                                                    caption_ids, seed)
            return self._reverse(cond_emb, [(s_, s_) for s_ in range(T - 1, -1, -1)], noise_fn, return_logits,
                                 start_tokens=x, caption_ids=caption_ids, seed=seed, hold=hold, guide=guide)
        if start_step == 0:
            return self._reverse(cond_emb, [(s_, s_) for s_ in range(T - 1, -1, -1)], noise_fn, return_logits,
                                 caption_ids=caption_ids, seed=seed, guide=guide)
        # partial re-sampling (:643-651): diffuse the given tokens (e.g. DALLE.get_tokens of a mel) forward to
        # t = start_step - 1, then run the reverse chain from there.  With noise_fn, call 0 is q_sample's draw and
        # the reverse steps get the running call index 1.. instead of the timestep.
        if content_token is None:
            raise ValueError("filter_ratio > 0 re-samples given content: pass content_token i64[B, 265]")
        device, B = self.device, cond_emb.shape[0]
        shape = (B, self.num_classes, self.content_seq_len)
        t = torch.full((B,), start_step - 1, device=device, dtype=torch.long)
        steps = list(range(start_step - 1, -1, -1))
        if noise_fn is None and (caption_ids is not None or self.rng_mode == "philox"):
            # forward diffusion on stream 1 of each caption's Philox draws (call 0), the reverse chain on stream 0
            x0 = content_token.to(device).contiguous()
            gids = self._caption_ids(caption_ids, B, device)
            x = torch.empty_like(x0)
            _lib.check(_lib.lib().ds_q_sample_rng(_lib.ptr(x0), _lib.ptr(t), _lib.ptr(gids),
                                                  self._seed(seed), 0,
                                                  _lib.ptr(self._schedule_table()), _lib.ptr(x), B, self.content_seq_len,
                                                  self.num_classes - 1, self.num_timesteps, _lib.stream()))
            return self._reverse(cond_emb, [(s_, s_) for s_ in steps], None, return_logits, start_tokens=x,
                                 caption_ids=gids, seed=seed, guide=guide)
        u = noise_fn(0, shape).to(device) if noise_fn is not None else torch.rand(shape, device=device)
        x = self.q_sample_tokens(content_token.to(device), t, u)
        nf = None if noise_fn is None else (lambda st, shp: noise_fn(1 + steps.index(st), shp)) \
            if self.repeat_rate is None else (lambda c, shp: noise_fn(1 + c, shp))
        return self._reverse(cond_emb, [(s_, s_) for s_ in steps], nf, return_logits, start_tokens=x, guide=guide)

    @torch.no_grad()
    def sample_fast(self, condition_token, condition_mask, condition_embed, content_token=None, filter_ratio=0.5,
                    temperature=1.0, return_att_weight=False, return_logits=False, content_logits=None,
                    print_log=True, skip_step=1, noise_fn=None, caption_ids=None, seed=None, keep_mask=None,
                    keep_mode="clamp", guidance_scale=None, null_condition_embed=None, track_embed=None, track_weight=None,
                    **kwargs):
        """Skip-step sampler (:748-812): timesteps T-1, T-2-skip, ... (0 appended), the network sees t, the
        posterior t - skip_step while t > skip_step.  The reference calls p_pred's pieces directly, so the 'q'
        wrapper on p_sample never applies here.  keep_mask / keep_mode: region-held sampling as in sample(); the
        posterior's timestep governs what a renoised position is drawn at.  guidance_scale / null_condition_embed:
        classifier-free guidance as in sample().  track_embed / track_weight: caption tracks as in sample()."""
        cond_emb, guide = self._cond_guide(condition_token, condition_embed, guidance_scale, null_condition_embed, track_embed,
                                           track_weight)
        if keep_mask is not None and int(self.num_timesteps * filter_ratio) != 0:
            raise ValueError("keep_mask samples the free positions from [MASK]: filter_ratio must resolve to step 0")
        assert int(self.num_timesteps * filter_ratio) == 0     # the reference asserts start_step == 0 (:787)
        lst = list(range(self.num_timesteps - 1, -1, -1 - skip_step))
        if lst[-1] != 0:
            lst.append(0)
        hold = x = None
        if keep_mask is not None:
            hold, x, caption_ids = self._hold_start(keep_mask, keep_mode, content_token, cond_emb.shape[0], noise_fn,
                                                    caption_ids, seed)
        keep, self.repeat_rate = self.repeat_rate, None
        try:
            return self._reverse(cond_emb, [(s_, s_ - skip_step if s_ > skip_step else s_) for s_ in lst], noise_fn,
                                 return_logits, start_tokens=x, caption_ids=caption_ids, seed=seed, hold=hold, guide=guide)
        finally:
            self.repeat_rate = keep

    # ---- joint-window sampling (csrc/sampler.hip SampleJoint) ----------------------------------------------
    JOINT_MAX_ROWS = 128      # the largest forward of a joint step: the largest batch the project has measured

    def _joint_once(self, cond_emb, geometry, calls, noise_fn, gids, seed, hold, guide):
        """One joint chain on a chunk of clips -> canvas i64[B, Lc].  calls: [(t, t_post)]; noise_fn None: the one-call chain
        with in-kernel noise (ds_denoiser_sample_joint_rng), else the stepped entry per call (ds_denoiser_step_joint)."""
        from ..audio import _fade_table
        W, n, ring, Lc = geometry
        device = self.device
        B, K1, L = cond_emb.shape[0], self.num_classes, self.content_seq_len
        sched = self._schedule_table()
        tr = self.transformer
        p = tr.packed(sched)
        lib = _lib.lib()
        r, k = self._truncation()
        n_cond = 1 if guide is None else 2
        Bf = n_cond * B * W
        emb = cond_emb.to(device).float().repeat_interleave(W, 0)               # row b W + w: clip b's caption
        scale = 1.0
        if guide is not None:
            emb, scale = torch.cat((emb, guide[0].repeat_interleave(W, 0)), 0), guide[1]
        kv = tr.condition_kv(emb.contiguous(), sched)
        fade = _fade_table(n, device)
        keep, known = (None, None) if hold is None else hold
        x = torch.full((B, Lc), K1 - 1, device=device, dtype=torch.long) if hold is None \
            else torch.where(keep != 0, known, torch.full_like(known, K1 - 1))
        tmp = torch.empty_like(x)
        tokens_n = torch.empty(Bf, L, device=device, dtype=torch.long)
        ws = tr.workspace(Bf, sched, 0)
        geo = [B, W, n, int(bool(ring)), n_cond, _lib.ptr(fade)]
        tail = [r, k, float(scale), _lib.ptr(keep), _lib.ptr(known), 0, _lib.ptr(tokens_n), _lib.ptr(ws)]
        if noise_fn is None:
            t_steps = torch.tensor(calls, dtype=torch.long, device=device).view(-1, 2, 1).expand(-1, 2, Bf).contiguous()
            _lib.check(lib.ds_denoiser_sample_joint_rng(p["handle"], _lib.ptr(x), _lib.ptr(tmp), _lib.ptr(t_steps), len(calls),
                                                        _lib.ptr(kv), _lib.ptr(gids), self._seed(seed), 0, *geo,
                                                        int(hold is None), *tail, _lib.stream()))
            return x
        for i, (step, step_post) in enumerate(calls):
            u = noise_fn(step, (B, K1, Lc)).to(device).float().contiguous()
            t = torch.full((Bf,), step, device=device, dtype=torch.long)
            tp = None if step_post == step else torch.full((Bf,), step_post, device=device, dtype=torch.long)
            _lib.check(lib.ds_denoiser_step_joint(p["handle"], _lib.ptr(x), _lib.ptr(t), _lib.ptr(tp), _lib.ptr(kv), _lib.ptr(u),
                                                  *geo, int(hold is None and i == 0), *tail, _lib.ptr(tmp), _lib.stream()))
            x, tmp = tmp, x
        return x

    @torch.no_grad()
    def sample_joint(self, condition_embed, windows, overlap_cols, ring=False, skip_step=0, caption_ids=None, seed=None,
                     keep_mask=None, content_token=None, guidance_scale=None, null_condition_embed=None, noise_fn=None):
        """Joint-window sampling (not in the reference; the discrete-diffusion counterpart of MultiDiffusion, Bar-Tal et al.
        2023): all `windows` = W overlapping 5 x 53 windows of a long clip live on one token canvas of
        C = pipeline.joint_canvas_cols(W, overlap_cols, ring) columns, every diffusion step runs the denoiser ONCE on all
        windows at batch B W (2 B W with guidance) and the joint tail draws one token per canvas position -- from the fusion
        of the two windows' predictions where two windows cover it (csrc/sampler.hip SampleJoint).  ring=True closes the
        canvas into a ring (W >= 2): the last window flows into the first.  -> canvas tokens i64[B, 5 C], time-major.

        condition_embed f32[B, 77, 512].  skip_step: the skip-step plan of sample_fast (0: all T steps).  Noise: in-kernel
        Philox per clip (caption_ids, default 0 .. B-1; seed) at the canvas position, the whole chain one C call -- or
        noise_fn(t, (B', K+1, 5 C)), the stepped entry.  keep_mask bool[B, 5 C] / content_token i64[B, 5 C]: held canvas
        positions (clean: there is no renoise mode).  guidance_scale / null_condition_embed as in sample().  Clips are
        independent; the batch is cut into chunks whose forward has at most JOINT_MAX_ROWS rows (noise_fn is then called
        per chunk, with the chunk's B').  How joint clips sound is unmeasured: no trained checkpoint has been available."""
        from ..pipeline import GRID_ROWS, joint_canvas_cols
        W, n = int(windows), int(overlap_cols)
        Lc = GRID_ROWS * joint_canvas_cols(W, n, ring)
        if self.content_seq_len != 265:
            raise ValueError("joint sampling is built for the 5 x 53 grid, this model's is %d tokens" % self.content_seq_len)
        if self.repeat_rate is not None:
            raise ValueError("the repeat sampler (',q{rate}') is not built for joint sampling")
        cond_emb = self._cond(None, condition_embed)
        guide = self._guide(guidance_scale, null_condition_embed, cond_emb)
        device, B, T = self.device, cond_emb.shape[0], self.num_timesteps
        skip = int(skip_step)
        lst = list(range(T - 1, -1, -1 - skip))
        if lst[-1] != 0:
            lst.append(0)
        calls = [(s_, s_ - skip if s_ > skip else s_) for s_ in lst]
        hold = None
        if keep_mask is not None:
            if content_token is None:
                raise ValueError("keep_mask holds canvas positions of given content: pass content_token i64[B, %d]" % Lc)
            known = torch.as_tensor(content_token).to(device).long().contiguous()
            keep = torch.as_tensor(keep_mask).to(device)
            if tuple(known.shape) != (B, Lc) or tuple(keep.shape) != (B, Lc):
                raise ValueError("keep_mask and content_token of joint sampling are on the canvas, [%d, %d]: got %s and %s"
                                 % (B, Lc, tuple(keep.shape), tuple(known.shape)))
            hold = ((keep != 0).to(torch.uint8).contiguous(), known)
        gids = None if noise_fn is not None else self._caption_ids(caption_ids, B, device)
        n_cond = 1 if guide is None else 2
        if n_cond * W > self.JOINT_MAX_ROWS:
            raise ValueError("%d windows%s exceed the largest forward of joint sampling (%d rows)"
                             % (W, " with guidance" if guide is not None else "", self.JOINT_MAX_ROWS))
        chunk = max(1, self.JOINT_MAX_ROWS // (n_cond * W))
        out = []
        for a in range(0, B, chunk):
            sl = slice(a, min(B, a + chunk))
            out.append(self._guarded(self._joint_once, cond_emb[sl], (W, n, bool(ring), Lc), calls, noise_fn,
                                     None if gids is None else gids[sl].contiguous(), seed,
                                     None if hold is None else (hold[0][sl].contiguous(), hold[1][sl].contiguous()),
                                     None if guide is None else (guide[0][sl], guide[1])))
        return out[0] if len(out) == 1 else torch.cat(out, 0)

    # ---- purity-prior sampling (csrc/sampler.hip SamplePurity) ---------------------------------------------
    def _purity_check(self, steps, purity_weight, keep_mode, filter_ratio):
        """The argument rules of sample_purity, before anything is enqueued -> (S, weight)."""
        if keep_mode != "clamp":
            raise ValueError("purity sampling holds positions clean (keep_mode='clamp'): a revealed token is never re-drawn, "
                             "so keep_mode=%r does not exist here" % (keep_mode,))
        if self.repeat_rate is not None:
            raise ValueError("the repeat sampler (',q{rate}') re-applies a posterior step: not with purity sampling")
        if int(self.num_timesteps * filter_ratio) != 0:
            raise ValueError("purity sampling generates from [MASK]: filter_ratio must resolve to step 0")
        S = self.num_timesteps if steps is None else int(steps)
        w = float(purity_weight)
        if not (w >= 0.0 and w != float("inf")):
            raise ValueError("purity_weight must be finite and >= 0, got %r" % (purity_weight,))
        if not 1 <= S <= self.content_seq_len:
            raise ValueError("steps must be in 1 .. %d (a step reveals at least one position), got %r" % (self.content_seq_len, steps))
        return S, w

    def _purity_once(self, cond_emb, plan, weight, noise_fn, return_logits, start_tokens=None, caption_ids=None, seed=None,
                     guide=None):
        """The purity chain of `plan` (purity_plan).  In-kernel noise: one C call (ds_denoiser_sample_purity_rng), nothing
        returns to Python between steps; caller noise: noise_fn(k, shape) per call k, or torch.rand."""
        import ctypes
        device = self.device
        B, K1, L = cond_emb.shape[0], self.num_classes, self.content_seq_len
        cond_emb = cond_emb.to(device)
        x = torch.full((B, L), K1 - 1, device=device, dtype=torch.long) if start_tokens is None else start_tokens.to(device).clone()
        sched = self._schedule_table()
        tr = self.transformer
        p = tr.packed(sched)
        lib = _lib.lib()
        r, k = self._truncation()
        scratch = torch.empty(int(lib.ds_purity_scratch_bytes(B, L)), device=device, dtype=torch.uint8)
        tmp = torch.empty_like(x)
        if guide is not None:
            kv, scale, tokens2 = self._guide_start(guide, cond_emb, sched)
            Bf = 2 * B
        else:
            kv, scale, tokens2, Bf = tr.condition_kv(cond_emb.contiguous(), sched), 1.0, None, B
        ws = tr.workspace(Bf, sched, 0)
        if noise_fn is None and (caption_ids is not None or self.rng_mode == "philox"):
            gids = self._caption_ids(caption_ids, B, device)
            t_steps = torch.tensor([t for t, _ in plan], dtype=torch.long, device=device).view(-1, 1).expand(-1, Bf).contiguous()
            remain = (ctypes.c_int * len(plan))(*[rk for _, rk in plan])
            _lib.check(lib.ds_denoiser_sample_purity_rng(
                p["handle"], _lib.ptr(x), _lib.ptr(tmp), _lib.ptr(t_steps), remain, len(plan), _lib.ptr(kv), _lib.ptr(gids),
                self._seed(seed), 0, B, weight, r, k, float(scale), _lib.ptr(tokens2),
                _lib.ptr(ws), _lib.ptr(scratch), _lib.stream()))
        else:
            for call, (t_k, r_k) in enumerate(plan):
                u = (noise_fn(call, (B, K1, L)).to(device) if noise_fn is not None else torch.rand((B, K1, L), device=device))
                u = u.contiguous()
                t = torch.full((Bf,), t_k, device=device, dtype=torch.long)
                _lib.check(lib.ds_denoiser_step_purity(
                    p["handle"], _lib.ptr(x), _lib.ptr(t), _lib.ptr(kv), _lib.ptr(u), B, int(r_k), weight, r, k, float(scale),
                    _lib.ptr(tokens2), _lib.ptr(ws), _lib.ptr(scratch), _lib.ptr(tmp), _lib.stream()))
                x, tmp = tmp, x
        return self._result(x, return_logits)

    @torch.no_grad()
    def sample_purity(self, condition_token, condition_mask, condition_embed, content_token=None, filter_ratio=0,
                      temperature=1.0, return_att_weight=False, return_logits=False, content_logits=None, print_log=True,
                      steps=None, purity_weight=0.0, noise_fn=None, caption_ids=None, seed=None, keep_mask=None,
                      keep_mode="clamp", guidance_scale=None, null_condition_embed=None, **kwargs):
        """Purity-prior sampling (not in the reference; the high-quality inference strategy of Tang et al. 2022, specified in
        DESIGN.md section 4): a chain of `steps` = S denoiser forwards (1 <= S <= 265, default T) from the all-[MASK] state.
        Step k reveals exactly R_{k-1} - R_k positions per sample (purity_plan) -- those where the predicted x0 distribution
        is most certain, drawn without replacement in proportion to their purity -- with a token drawn from the truncated
        prediction, sharpened by purity_weight r >= 0 (exponent 1 + r purity; 0: not sharpened).  A revealed token is never
        re-sampled, and the chain ends with no [MASK] at any S.  No posterior is involved; the timestep only tells the
        network how much of the grid is still masked.

        keep_mask / content_token: region-held sampling -- the held positions enter as their known tokens, i.e. as already
        revealed, and come out bit-exact (clamp mode only: keep_mode='renoise' raises ValueError, as do the ',q{rate}'
        repeat sampler and a filter_ratio that does not resolve to step 0).  guidance_scale / null_condition_embed,
        caption_ids / seed as in sample(); noise_fn(k, shape) gets the call index k = 0 .. S-1.  What this sampler does to
        audio quality is unmeasured: no trained checkpoint has been available to this project."""
        if kwargs.get("track_embed") is not None or kwargs.get("track_weight") is not None:
            raise ValueError("caption tracks have no purity form: track_embed / track_weight go to sample() or sample_fast()")
        S, weight = self._purity_check(steps, purity_weight, keep_mode, filter_ratio)
        cond_emb = self._cond(condition_token, condition_embed)
        guide = self._guide(guidance_scale, null_condition_embed, cond_emb)
        x = None
        if keep_mask is not None:
            _, x, _ = self._hold_start(keep_mask, "clamp", content_token, cond_emb.shape[0], noise_fn, caption_ids, seed)
        plan = purity_plan(S, self.content_seq_len, self.log_cumprod_ct)
        return self._guarded(self._purity_once, cond_emb, plan, weight, noise_fn, return_logits, start_tokens=x,
                             caption_ids=caption_ids, seed=seed, guide=guide)

    # ---- likelihood scoring (csrc/sampler.hip ds_score_tail_kernel) ---------------------------------------
    def _score_once(self, x0, cond_emb, ts, draws, gids, seed, rows_per_launch, want_map):
        """The rows of a score: per draw r, row k N + n is clip n at timestep ts[k] (timestep-major, so consecutive launches of
        a batch of clips see the same clips and share one caption K/V), cut into launches of at most rows_per_launch rows; a
        launch never spans two draws (the draw index is the launch's Philox call).  -> (terms f64[draws, n_t, N], per-position
        values f32[draws, n_t, N, L] or None)."""
        device = self.device
        N, L = x0.shape
        n_t, rows = len(ts), len(ts) * N
        sched = self._schedule_table()
        tr = self.transformer
        p = tr.packed(sched)
        lib = _lib.lib()
        t_rows = torch.tensor(ts, dtype=torch.long, device=device).repeat_interleave(N).contiguous()
        terms = torch.full((draws, rows), float("nan"), dtype=torch.float64, device=device)
        pos = torch.full((draws, rows, L), float("nan"), dtype=torch.float32, device=device) if want_map else None
        kv_of = {}                                        # (first clip, rows) of a launch -> its replicated inputs
        for r in range(draws):
            for a in range(0, rows, rows_per_launch):
                B = min(rows, a + rows_per_launch) - a
                key = (a % N, B)
                if key not in kv_of:
                    clip = (torch.arange(a, a + B, device=device) % N)
                    kv_of.clear()                         # one launch shape alive at a time: the K/V of 64 rows is large
                    kv_of[key] = (x0[clip].contiguous(), gids[clip].contiguous(),
                                  tr.condition_kv(cond_emb[clip].contiguous(), sched))
                x_rows, g_rows, kv = kv_of[key]
                xt = torch.empty_like(x_rows)
                t_l, term_l = t_rows[a:a + B], terms[r, a:a + B]
                pos_l = None if pos is None else pos[r, a:a + B]
                _lib.check(lib.ds_denoiser_score_rng(p["handle"], _lib.ptr(x_rows), _lib.ptr(t_l), _lib.ptr(kv), _lib.ptr(g_rows),
                                                     self._seed(seed), r, B, _lib.ptr(tr.workspace(B, sched)), _lib.ptr(xt),
                                                     _lib.ptr(term_l), _lib.ptr(pos_l), _lib.stream()))
        return terms.view(draws, n_t, N), None if pos is None else pos.view(draws, n_t, N, L)

    @torch.no_grad()
    def score_tokens(self, content_token, condition_token=None, condition_embed=None, timesteps=None, draws=1,
                     caption_ids=None, seed=None, rows_per_launch=64, return_terms=False, return_map=False):
        """How well clips fit their captions: the variational bound of content_token i64[N, L] (every value < K) under the
        captions (condition_token i64[N, 77] or condition_embed f32[N, 77, 512]), in nats, f64[N] -- lower is a better fit.
            score = (1 / draws) sum_r sum_k w_k term(x0, c, t_k, r),   (t_k, w_k) = score_plan(T, timesteps)
        term: the decoder NLL at t = 0, the KL between the true and the modelled posterior at t > 0, summed over the grid, on
        x_t = q_sample(x0, t_k) drawn from stream 1 of (caption_ids[n], seed) at Philox call r -- the same uniforms at every
        t and in every batch, so a score does not depend on how its rows are cut into launches, and one clip scored under
        several captions with one id sees common random numbers.  The prior term KL(q(x_T | x0) || p(x_T)) is left out, as the
        reference's loss leaves it out; mask weights are (1, 1) and there is no auxiliary term: this is the bound, not the
        training loss.  timesteps None (or T): the full bound, T forwards per clip; an integer n in 2 .. T-1: t = 0 and n - 1
        evenly spread timesteps, re-weighted.  The (clip, timestep) rows run draws x ceil(N n_t / rows_per_launch) launches of
        ds_denoiser_score_rng (64 rows: the batch the per-sample GEMM program is tuned for), under the range guard of the
        sampling chains.  return_terms: also terms f64[N, n_t] (unweighted, mean over draws); return_map: also f32[N, L], the
        weighted per-position sum (mean over draws) -- returned as a tuple in that order."""
        L, K, T = self.content_seq_len, self.num_classes - 1, self.num_timesteps
        device = self.device
        x0 = torch.as_tensor(content_token).to(device).long().contiguous()
        if x0.dim() != 2 or x0.shape[1] != L or x0.shape[0] < 1:
            raise ValueError("content_token must be i64[N, %d] with N >= 1, got %s" % (L, tuple(x0.shape)))
        if int(x0.max()) >= K or int(x0.min()) < 0:
            raise ValueError("content_token holds values outside 0 .. %d ([MASK] = %d is not a valid x0)" % (K - 1, K))
        draws, rows_per_launch = int(draws), int(rows_per_launch)
        if draws < 1 or rows_per_launch < 1:
            raise ValueError("draws and rows_per_launch must be at least 1, got %d and %d" % (draws, rows_per_launch))
        ts, weights = score_plan(T, timesteps)
        N = x0.shape[0]
        cond_emb = self._cond(condition_token, condition_embed).to(device)
        if cond_emb.shape[0] != N:
            raise ValueError("%d conditions for %d clips" % (cond_emb.shape[0], N))
        gids = self._caption_ids(caption_ids, N, device)
        terms, pos = self._guarded(self._score_once, x0, cond_emb, ts, draws, gids, seed, rows_per_launch, return_map)
        w = torch.tensor(weights, dtype=torch.float64, device=device)
        terms = terms.mean(0)                                        # [n_t, N]
        out = [(terms * w[:, None]).sum(0)]
        if return_terms:
            out.append(terms.t().contiguous())
        if return_map:
            out.append((pos.double() * w[None, :, None, None]).sum(1).mean(0).float())
        return out[0] if len(out) == 1 else tuple(out)
