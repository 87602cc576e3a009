"""Training step of the denoiser on the HIP kernels (scope row 8f-3).

    loss, grads = TrainStep(model.transformer).loss_and_grads(x0, cond_emb, t, pt, noise)

follows DiffusionTransformer._train_loss / forward (diffusion_transformer.py:408-476,539-577) and what
`loss.backward()` produces for every parameter of `Text2ImageTransformer` (engine/solver_spec.py:308-331 back-propagates
exactly this), without an autograd graph: the forward keeps the activations the backward needs, every nn.Linear
contributes three GEMMs (y = x W^T, dX = dY W, dW = dY^T X -- 98 % of the step's flops), the row / elementwise
pieces run on csrc/train.hip, norm.hip and sampler.hip.  The self-attention Q | K | V projections and the
cross-attention K | V projections are fused into one linear each (one GEMM of N = 3D / 2D instead of three / two).

Two GEMM backends (`TrainStep(precision=...)`; modeling/train_gemm.py), both behind the same step:

  "fp32"   exact-fp32 MFMA (`ds_gemm`); transposed / padded operands are made by torch.  The reference arithmetic.
  "f16x2"  the fp32-class 3-pass fp16 split GEMM with PACKED split planes on both operands of all three GEMMs (LDS-DMA
           staging, gemm_f16x2.hip AMODE 2: 1.2-1.4x the loader-split program on the step's shapes) and NOTHING on the host
           between two launches.  Every matrix that enters a GEMM goes through `ds_pack_operand` exactly once (csrc/pack.hip):
             * an activation x -> its row form (A of y = x W^T) and its transposed form (X^T, W operand of dW = dY^T X);
             * a gradient dY  -> its row form (A of dX = dY W), its transposed form (A of dW), the per-tile column sums that
               become the bias gradient, and max |dY| for the loss-scale monitor -- one read of dY instead of four;
             * a weight W     -> row form (forward) and transposed form (dX), with a per-matrix power-of-two pre-scale
               refreshed every `rescale_interval` steps (weights move slowly);
             * GELU2 rides in the pack's prologue in both directions (fc2's input from fc1's output; d fc1-output from
               d gelu-output), so the MLP's activation and its gradient never exist in fp32.
           dW runs as a split-K launch on the packed planes (`groups` K-ranges fill the chip: a 1024 x 1024 dW is only 64
           tiles) whose partial sums `ds_colsum` adds in a fixed order.  The gradients' magnitude (|dY| ~ 1e-12 .. 1e-2, far
           below fp16's range, and spread over 2^25 between the sites of one backward) is handled by a loss scale 2^k -- d
           logits is multiplied by it, every dX carries it, the dW GEMMs' epilogue and one multiply over the small gradients
           take it out again -- PLUS one power of two per site (every linear's dY, every attention backward's dO; round 6): the
           operand times 2^e is what is split to fp16 and 2^-e goes into the consuming epilogues / stores, exact.  k and the e
           come from a two-pass calibration (`calibrate`: max |operand| per site, two host syncs; the policy around them -- where a
           calibration aims, when it is dropped -- is modeling/loss_scale.py).  A split value keeps an
           absolute precision of 2^-25, so anything above 2^-3 after scaling is fp32-class; the calibration puts every site's
           largest value at 2^6..2^7 under a saturation monitor whose window ends at 2^15.  The FORWARD operands (LayerNorm and
           attention outputs, gelu2(u)) are split as they are while they stay under 2^13; a linear whose input has outgrown
           that (fc2's is the candidate: 1.4e4 on trained-like weights) is packed under 2^f = 2^(12 - floor(log2 max)) from the
           first calibration pass, 2^-f goes into its forward and dW epilogues, and a second monitor scalar takes max |x 2^f|
           of every pass (LossScalePolicy.fwd_exponents / check_loss_scale; tests/test_hip_train_range.py).  The step has no host
           synchronisation at all and is captured in a hipGraph (`capture`): one graph launch per iteration instead of ~2000
           kernel launches from Python.

Attention: `attention="fused"` (default) = a fused forward + a backward by tile-wise recomputation that reads Q | K | V and
writes dQ | dK | dV in place in the fused projection buffers and never stores the probabilities -- `ds_attention` +
`ds_attention_bwd` on the exact-fp32 MFMA in the "fp32" backend, `ds_attention_f16x2` + `ds_attention_bwd_f16x2` (every tile
product on the fp16 matrix cores, 3-pass split, fp32-class) in the "f16x2" backend; `attention="composed"` = grouped fp32
GEMMs + row softmax with materialised probabilities and torch head split / merge / transposes (the first version, kept as a
cross-check).  The norms and the loss tail are exact fp32.  Worst per-tensor gradient error against autograd through the oracle, all 63 tensors of the
2-layer test model: see tests/test_hip_train_kernels.py.
"""
import math

import torch

from .. import _lib
from .loss_scale import LossScalePolicy
from .train_gemm import (PACK_GELU2, PACK_GELU2_BWD, PACK_PLAIN, _ceil, _colsum, _Fp32Gemm, _Linear, _Packed, _pack,  # noqa: F401
                         _pack_parts, _SplitGemm)

L_ = _lib


_ROWS_MAX = 32      # rows per launch of ds_rows_outer / ds_rows_times_matrix


def _rows_outer(a, s):
    """out[g] = a[g]^T s[g] for a [G][B][N], s [G][B][D] (contiguous) by ds_rows_outer; past 32 samples, one launch per 32 and
    the partial results added in chunk order (bit-reproducible)"""
    G, B, N = a.shape
    D = s.shape[2]
    out = torch.empty(G, N, D, device=a.device)
    tmp = None
    for b0 in range(0, B, _ROWS_MAX):
        nb = min(B - b0, _ROWS_MAX)
        ab = a if nb == B else a[:, b0:b0 + nb].contiguous()
        sb = s if nb == B else s[:, b0:b0 + nb].contiguous()
        if b0 and tmp is None:
            tmp = torch.empty_like(out)
        L_.check(L_.lib().ds_rows_outer(L_.ptr(ab), L_.ptr(sb), L_.ptr(tmp if b0 else out), G, nb, N, D, L_.stream()))
        if b0:
            out += tmp
    return out


def _norm_fwd(x, mode, L, table=None, t=None, gamma=None, beta=None):
    M, D = x.shape
    y = torch.empty_like(x)
    if mode == 0:
        L_.check(L_.lib().ds_adaln(L_.ptr(x), L_.ptr(y), M, L, D, L_.ptr(table), L_.ptr(t), L_.stream()))
    else:
        L_.check(L_.lib().ds_layernorm(L_.ptr(x), L_.ptr(y), M, D, L_.ptr(gamma), L_.ptr(beta), L_.stream()))
    return y


def _norm_bwd(x, dy, mode, L, table=None, t=None, gamma=None, add_to=None):
    """-> (dx, [d scale | d shift]): the sums per sample [B][2D] (AdaLN, mode 0) or over all rows [1][2D] (LayerNorm, mode 1).
    One kernel computes dx and per-chunk column sums of dy * xn and dy (ds_layernorm_bwd_sums), one ds_colsum adds the chunks.
    add_to: the residual stream's gradient -- the norm-input gradient is ADDED to it in place instead of being returned."""
    M, D = x.shape
    dx = torch.empty_like(x) if add_to is None else add_to
    G = M // L if mode == 0 else 1
    chunks = L_.lib().ds_layernorm_bwd_chunks(M, L, mode)
    part = torch.empty(G * chunks, 2 * D, device=x.device)
    L_.check(L_.lib().ds_layernorm_bwd_sums(L_.ptr(x), L_.ptr(dy), L_.ptr(dx), L_.ptr(part), M, L, D, mode, L_.ptr(table), L_.ptr(t),
                                            L_.ptr(gamma), int(add_to is not None), L_.stream()))
    sums = torch.empty(G, 2 * D, device=x.device)
    L_.check(L_.lib().ds_colsum(L_.ptr(part), L_.ptr(sums), G, chunks, 2 * D, 2 * D, chunks * 2 * D, 0, L_.stream()))
    return dx, sums


def _heads(x, B, Lx, H, Lp):
    """[B*Lx, H*64] (a column range of a fused projection is fine: any row stride) -> [B*H, Lp, 64] zero-padded"""
    out = torch.zeros(B * H, Lp, 64, device=x.device)
    out.view(B, H, Lp, 64)[:, :, :Lx].copy_(x.view(B, Lx, H, 64).permute(0, 2, 1, 3))
    return out


def _merge_into(out, x4, B, Lx, H):
    """[B*H, Lp, 64] -> out [B*Lx, H*64] (any row stride)"""
    out.view(B, Lx, H, 64).copy_(x4.view(B, H, -1, 64)[:, :, :Lx].permute(0, 2, 1, 3))   # .view: never a silent copy
    return out


# The two attention classes share one surface: an operand is (tensor, first column, row stride) -- a column range of a fused
# projection buffer, read or written where it lies -- `out` is the forward's [B*Lq][H*64] result, and
# backward(dO, dq, dk, dv, amax, do_scale) writes the three gradients into their operands.  `site`: whether the backward splits
# dO to fp16 under a power of two of its own, i.e. is a site of the loss-scale calibration (TrainStep.calibrate).

class _Attn:
    """softmax(q k^T / 8) v per head (FullAttention / CrossAttention cores, transformer_utils.py:43-58,91-109), composed:
    grouped exact-fp32 GEMMs + row softmax with stored probabilities; torch slices the operands' column ranges and splits /
    merges the heads.  The first version, kept as a cross-check of the fused kernels."""
    site = False

    def __init__(self, q, k, v, B, Lq, Lk, H, split=False):
        """split: ignored (every product is exact fp32 here)"""
        q, k, v = (x[:, c:c + H * 64] for x, c, _ in (q, k, v))
        self.B, self.Lq, self.Lk, self.H = B, Lq, Lk, H
        self.Lqp, self.Lkp = _ceil(Lq, 32), _ceil(Lk, 32)
        G = B * H
        self.q4, self.k4, self.v4 = _heads(q, B, Lq, H, self.Lqp), _heads(k, B, Lk, H, self.Lkp), _heads(v, B, Lk, H, self.Lkp)
        S = torch.empty(G, self.Lqp, self.Lkp, device=q.device)
        L_.gemm(self.q4, self.k4, S, self.Lqp, self.Lkp, 64, groups=G, a_gstride=self.Lqp * 64, w_gstride=self.Lkp * 64,
                c_gstride=self.Lqp * self.Lkp)
        L_.check(L_.lib().ds_softmax_rows(L_.ptr(S), G * self.Lqp, Lk, self.Lkp, 0.125, L_.stream()))
        self.P = S
        vT = self.v4.transpose(1, 2).contiguous()                                  # [G, 64, Lkp]
        o4 = torch.empty(G, self.Lqp, 64, device=q.device)
        L_.gemm(self.P, vT, o4, self.Lqp, 64, self.Lkp, groups=G, a_gstride=self.Lqp * self.Lkp, w_gstride=64 * self.Lkp,
                c_gstride=self.Lqp * 64)
        self.out = _merge_into(torch.empty(B * Lq, H * 64, device=q.device), o4, B, Lq, H)

    def backward(self, dO, dq, dk, dv, amax=None, do_scale=1.0):
        """dO [B*Lq, H*64] -> dQ / dK / dV into the column ranges dq / dk / dv of the fused gradient buffers.  amax, do_scale:
        ignored (nothing is split to fp16 here)"""
        B, Lq, Lk, H, Lqp, Lkp = self.B, self.Lq, self.Lk, self.H, self.Lqp, self.Lkp
        G = B * H
        dO4 = _heads(dO, B, Lq, H, Lqp)
        dev = dO.device
        dV4 = torch.empty(G, Lkp, 64, device=dev)                                   # dV = P^T dO
        L_.gemm(self.P.transpose(1, 2).contiguous(), dO4.transpose(1, 2).contiguous(), dV4, Lkp, 64, Lqp, groups=G,
                a_gstride=Lkp * Lqp, w_gstride=64 * Lqp, c_gstride=Lkp * 64)
        dP = torch.empty(G, Lqp, Lkp, device=dev)                                   # dP = dO V^T
        L_.gemm(dO4, self.v4, dP, Lqp, Lkp, 64, groups=G, a_gstride=Lqp * 64, w_gstride=Lkp * 64, c_gstride=Lqp * Lkp)
        L_.check(L_.lib().ds_softmax_bwd_rows(L_.ptr(self.P), L_.ptr(dP), G * Lqp, Lk, Lkp, 0.125, L_.stream()))
        dS = dP
        dQ4 = torch.empty(G, Lqp, 64, device=dev)                                   # dQ = dS K
        L_.gemm(dS, self.k4.transpose(1, 2).contiguous(), dQ4, Lqp, 64, Lkp, groups=G, a_gstride=Lqp * Lkp,
                w_gstride=64 * Lkp, c_gstride=Lqp * 64)
        dK4 = torch.empty(G, Lkp, 64, device=dev)                                   # dK = dS^T Q
        L_.gemm(dS.transpose(1, 2).contiguous(), self.q4.transpose(1, 2).contiguous(), dK4, Lkp, 64, Lqp, groups=G,
                a_gstride=Lkp * Lqp, w_gstride=64 * Lqp, c_gstride=Lkp * 64)
        for (x, c, _), x4, Lx in ((dq, dQ4, Lq), (dk, dK4, Lk), (dv, dV4, Lk)):
            _merge_into(x[:, c:c + H * 64], x4, B, Lx, H)


class _FusedAttn:
    """The same attention cores on the fused kernels: `ds_attention` forward and `ds_attention_bwd` (tile-wise
    recomputation: the probabilities are never stored), reading Q / K / V and writing dQ / dK / dV IN PLACE in the fused
    projection buffers.  Exact-fp32 MFMA, like the composed version."""
    site = True

    def __init__(self, q, k, v, B, Lq, Lk, H, split=False):
        """split: the forward on the streamed fp16-split attention kernel of the sampling path (ds_attention_f16x2: fp32-class,
        2e-5 max-abs against float64 where the exact-fp32 kernel has 1e-6; 3-4x faster) -- the "f16x2" backend's choice; the
        backward recomputes the probabilities in exact fp32 either way."""
        self.q, self.k, self.v, self.B, self.Lq, self.Lk, self.H, self.split = q, k, v, B, Lq, Lk, H, split
        self.out = torch.empty(B * Lq, H * 64, device=q[0].device)
        fn = L_.lib().ds_attention_f16x2 if split else L_.lib().ds_attention
        L_.check(fn(L_.ptr_off(q[0], q[1]), q[2], L_.ptr_off(k[0], k[1]), k[2], L_.ptr_off(v[0], v[1]), v[2],
                    L_.ptr(self.out), H * 64, B, H, Lq, Lk, 0.125, L_.stream()))

    def backward(self, dO, dq, dk, dv, amax=None, do_scale=1.0):
        """split: the tile products of the recomputation on the fp16 matrix cores too (ds_attention_bwd_f16x2_mon); dO enters
        them as an fp16-split operand under the step's loss scale AND this call's own power of two `do_scale` (the kernel
        splits dO * do_scale and takes it out again at its stores), and the kernel folds max |dO * do_scale| into the saturation
        monitor (`amax`) itself; the in-register dS is normalised per wave inside the kernel (csrc/attention_bwd.hip)."""
        q, k, v, B, Lq, Lk, H = self.q, self.k, self.v, self.B, self.Lq, self.Lk, self.H
        stats = torch.empty(2 * B * H * _ceil(Lq, 32), device=dO.device)
        args = (L_.ptr_off(q[0], q[1]), q[2], L_.ptr_off(k[0], k[1]), k[2], L_.ptr_off(v[0], v[1]), v[2], L_.ptr(self.out), H * 64,
                L_.ptr(dO), H * 64, L_.ptr_off(dq[0], dq[1]), dq[2], L_.ptr_off(dk[0], dk[1]), dk[2], L_.ptr_off(dv[0], dv[1]), dv[2],
                L_.ptr(stats), B, H, Lq, Lk, 0.125)
        if self.split and amax is not None:
            L_.check(L_.lib().ds_attention_bwd_f16x2_mon(*args, float(do_scale), L_.ptr(amax), L_.stream()))
        else:
            L_.check((L_.lib().ds_attention_bwd_f16x2 if self.split else L_.lib().ds_attention_bwd)(*args, L_.stream()))


@torch.no_grad()
def training_inputs(model, batch, generator=None, cond_drop_prob=0.0, null_cond=None):
    """The reference's training batch -> the five tensors of `TrainStep.loss_and_grads`: what happens between
    `self.model(batch, return_loss=True)` (engine/solver_spec.py:308-331) and the loss arithmetic.

        batch {'image': mel f32[B,1,80,848], 'text': list of B captions}
          -> DALLE.prepare_input (dalle_spec.py:93-133): Tokenize (BPE ids i64[B,77], host) and VQModel.encode + argmin +
             ColumnMajor of the mel -> content_token i64[B,265]                       (HIP: vqgan.py, ds_vq_argmin)
          -> DiffusionTransformer.forward (diffusion_transformer.py:552-566): CLIPTextEmbedding of the ids -> f32[B,77,512]
          -> _train_loss (:408-421): sample_time(b, device, 'importance') -> (t, pt); the uniforms q_sample's
             log_sample_categorical draws as torch.rand_like(logits [B, K+1, L]) (:359-368)

    `model` is the DALLE drop-in (`condition_codec` + `transformer.condition_emb` built: config.default_config(with_clip=True)).
    A batch that already carries 'condition_embed_token' / 'condition_token' (DALLE.prepare_condition's other forms) or
    'content_token' skips the respective stage; one that carries 'audio' (waveforms at 22 050 Hz, or at batch['audio_rate']) instead of 'image' gets the mel
    from the HIP front end first (DALLE.content_image -> modeling/melspec.py).  generator: torch.Generator of the model's device for t and the noise.
    Everything is enqueued on the current stream; the only host synchronisation is sample_time's Lt_count test while it
    is still false.  cond_drop_prob / null_cond: condition dropout, see training_draws."""
    x0, cond_emb = training_prologue(model, batch)
    return training_draws(model, x0, cond_emb, generator=generator, cond_drop_prob=cond_drop_prob, null_cond=null_cond)


@torch.no_grad()
def training_prologue(model, batch):
    """The part of `training_inputs` that depends on the batch and on FROZEN weights only (BPE, the CLIP text tower, the VQ
    encoder): (x0 i64[B,265], cond_emb f32[B,77,512]).  Nothing the optimiser touches is read, so it may run ahead of the
    previous iteration -- GraphSolver.prefetch enqueues it on a side stream."""
    dt = model.transformer
    dev = dt.device
    cond = model.prepare_condition(batch)
    if batch.get("content_token") is not None:
        x0 = batch["content_token"].to(dev)
    else:
        x0 = model.prepare_content(batch)["content_token"]
    cond_emb = dt._cond(cond.get("condition_token"), cond.get("condition_embed_token")).to(dev)
    return x0.contiguous(), cond_emb.contiguous()


@torch.no_grad()
def training_draws(model, x0, cond_emb, generator=None, cond_drop_prob=0.0, null_cond=None):
    """... and the part that depends on the training state: sample_time reads the importance-sampling statistics the previous
    iteration updated.  -> (x0, cond_emb, t, pt, noise)

    cond_drop_prob > 0: condition dropout, what makes a model usable with classifier-free guidance -- after the draws of t and
    the noise, one uniform per sample from `generator`; the samples below cond_drop_prob get null_cond (f32[77,512], DALLE.
    null_condition()) as their condition.  With probability 0 no draw is made: the generator's state and every returned tensor
    are those of a call without the keywords."""
    dt = model.transformer
    dev = dt.device
    B = x0.shape[0]
    t, pt = dt.sample_time(B, dev, "importance", generator=generator)
    noise = torch.rand((B, dt.num_classes, dt.content_seq_len), device=dev, generator=generator)
    if cond_drop_prob > 0:
        if null_cond is None:
            raise ValueError("cond_drop_prob > 0 needs null_cond f32[77,512] (DALLE.null_condition())")
        drop = torch.rand((B,), device=dev, generator=generator) < cond_drop_prob
        null = torch.as_tensor(null_cond).to(device=cond_emb.device, dtype=cond_emb.dtype).expand_as(cond_emb)
        cond_emb = torch.where(drop.to(cond_emb.device)[:, None, None], null, cond_emb).contiguous()
    return x0, cond_emb, t.to(dev), pt.to(dev), noise


class _BlockActs:
    """What the forward of one block keeps for its backward: the residual stream at the three norm inputs (x0, x1, x2), the
    operand handles of the seven linears' inputs (h1: qkv1, o1: proj1, h2: q2, o2: proj2, h3: fc1, g: fc2 -- gelu2(u); the
    caption handle of kv2 is the pass's), the two attention objects, and fc1's output u."""
    __slots__ = ("x0", "h1", "att1", "o1", "x1", "h2", "att2", "o2", "x2", "h3", "u", "g")


_BLOCK_WEIGHTS = ("mlp.2.weight", "mlp.0.weight", "attn2.proj.weight", "attn2.query.weight", "attn2.key.weight",
                  "attn2.value.weight", "attn1.proj.weight", "attn1.query.weight", "attn1.key.weight", "attn1.value.weight")


class _Pass:
    """One walk of the network -- forward keeping activations, loss, backward -- for `TrainStep`: the normal step and the two
    calibration passes are this one code path (`calibrating`, `amax`, `site_amax`).  Every d* of the backward carries the loss
    scale; `small` collects what one multiply un-scales at the end (the weight gradients lose it in their GEMM's epilogue).

    site_amax: second calibration pass -- a zeroed f32[>= number of sites] whose slot i takes max |operand| of the i-th site
    (a linear's dY, a fused attention backward's dO) IN THE ORDER THE BACKWARD VISITS THEM; `site_index` receives the keys.
    fwd_amax: first calibration pass -- the same for the FORWARD operands: slot i takes max |x| of the i-th linear input the
    forward packs (`fwd_index`: the keys), every one packed unscaled.  Every other pass packs a linear's input under its
    calibrated 2^f (LossScalePolicy.fwd_exp) and folds max |x 2^f| into the forward monitor (`_fwd_live`)."""

    def __init__(self, step, x0, cond_emb, t, pt, noise, calibrating, amax=None, on_grads=None, site_amax=None, fwd_amax=None):
        self.step, self.dt, self.tr, self.gemm, self.policy = step, step.dt, step.tr, step.gemm, step.policy
        self.x0, self.cond_emb, self.t, self.pt, self.noise = x0, cond_emb, t, pt, noise
        self.calibrating, self.amax, self.site_amax = calibrating, amax, site_amax
        self.on_grads = None if calibrating else on_grads
        self.site_exp = {} if (calibrating or self.policy._site_exp is None) else self.policy._site_exp
        self.site_index = {}                    # site key -> slot of site_amax, in visiting order
        self.fwd_amax, self.fwd_index = fwd_amax, {}
        self.fwd_exp = {} if (fwd_amax is not None or self.policy.fwd_exp is None) else self.policy.fwd_exp
        self.fwd_live = None
        self.dev = x0.device
        self.B, self.Lx = x0.shape
        self.Lc = cond_emb.shape[1]
        self.D, self.H, self.K = self.tr.n_embd, self.tr.n_head, self.tr.num_codes
        self.M = self.B * self.Lx
        self.T = self.dt.num_timesteps
        self.loss_scale = 2.0 ** self.policy.loss_scale_exp
        self.inv = 1.0 / self.loss_scale
        self.g, self.small = {}, []             # {parameter name: gradient}; the tensors the closing multiply un-scales
        self.pending_dw, self.pending_names = [], []     # weight-gradient work not launched yet; names not handed over yet
        self.ada = [None] * (2 * len(self.tr.blocks))    # [d scale | d shift] [B][2D] per AdaLN module, forward order

    # ---- the walk --------------------------------------------------------------------------------------------------------
    def run(self):
        step, G_ = self.step, self.gemm
        G_.rows_per_sample = self.Lx
        self.blocks, self.lin_logits = step._linears()
        all_lins = [l for b in self.blocks for l in b.values()] + [self.lin_logits]
        if step.precision == "f16x2" and (not G_.wexp or (step._steps % step.rescale_interval == 0 and not self.calibrating
                                                           and not step._capturing)):
            G_.refresh_scales(all_lins)
        for l in all_lins:
            G_.prepare(l)
        if self.amax is None and step.precision == "f16x2":     # the saturation monitor (LossScalePolicy.check_loss_scale)
            if self.policy._amax_live is None or self.policy._amax_live.device != self.dev:
                self.policy._amax_live = torch.zeros(1, device=self.dev)
            self.amax = self.policy._amax_live
        if step.precision == "f16x2":
            if self.policy._fwd_live is None or self.policy._fwd_live.device != self.dev:
                self.policy._fwd_live = torch.zeros(1, device=self.dev)
            self.fwd_live = self.policy._fwd_live
        x = self.embed()
        self.adaln_tables()
        saved = []
        for li in range(len(self.blocks)):
            s, x = self.block_fwd(li, x)
            saved.append(s)
        lnf = self.tr.to_logits[0]
        hf = self.prep_x(self.lin_logits, _norm_fwd(x, 1, self.Lx, gamma=lnf.weight, beta=lnf.bias))
        logits = G_.fwd(self.lin_logits, hf)                                        # [M, K]
        loss, dlog = self.loss_and_dlogits(logits)
        g = self.g
        dh, g["transformer.to_logits.1.weight"], g["transformer.to_logits.1.bias"] = self.lin_bwd(self.lin_logits, hf, dlog)
        self.hand_over(["transformer.to_logits.1.weight"])
        dx, sums = _norm_bwd(x, dh, 1, self.Lx, gamma=lnf.weight)
        self.norm_gain_grads("transformer.to_logits.0", sums)
        for li in reversed(range(len(saved))):
            self.block_bwd(li, saved[li], dx)
            self.hand_over(["transformer.blocks.%d.%s" % (li, n) for n in _BLOCK_WEIGHTS], now=False)
        self.hand_over([])                       # the blocks still waiting
        self.adaln_param_grads_all()
        # the AdaLN parameter gradients (17 MB per block, 22 % of the gradient bytes) are final here: hand them to the
        # overlapped reduction before the embedding backward and the closing un-scale instead of leaving them to finish()
        self.hand_over([pfx + sfx for pfx in self.adaln_prefixes() for sfx in (".linear.weight", ".emb.weight")])
        self.embed_bwd(dx)
        if self.inv != 1.0:
            torch._foreach_mul_(self.small, self.inv)
        return loss, g

    def embed(self):
        """q_sample of the clean tokens, then token + position embedding -> x [M][D]; the caption rows' operand handle"""
        dt, emb = self.dt, self.tr.content_emb
        self.sched = dt._schedule_table()
        self.xt = dt.q_sample_tokens(self.x0.contiguous(), self.t, self.noise)
        pos = emb.position_table()
        x = torch.empty(self.M, self.D, device=self.dev)
        L_.check(L_.lib().ds_embed(L_.ptr(self.xt), L_.ptr(emb.emb.weight), L_.ptr(pos), L_.ptr(x), self.M, self.Lx, self.D,
                                   L_.stream()))
        cond = self.cond_emb.reshape(-1, self.cond_emb.shape[-1]).float().contiguous()
        # operand handles (gemm.prep_x): the forward's GEMM input AND the X^T of the same layer's dW, made in one pass; the
        # caption embedding feeds every block's cross K | V projection (same K, same padded contraction: one handle)
        self.cond_h = self.prep_x(self.blocks[0]["kv2"], cond)
        return x

    def adaln_tables(self):
        """The 2 n_layer AdaLN modulations  Linear(SiLU(Emb(t_b)))  (transformer_utils.py:145-147) as ONE grouped exact-fp32 GEMM
        over the batch's OWN timesteps -- B rows per module, as the reference computes them (the sampling loop tabulates all T
        rows once; here the weights change every iteration and a table of 100 rows was 5x the work: 416 -> 90 us, and as much
        again in the backward).  The AdaLN kernels index the [B][2D] rows with sample_rows = 0 .. B-1."""
        B, D = self.B, self.D
        lns = [ln for blk in self.tr.blocks for ln in (blk.ln1, blk.ln1_1)]
        self.ada_E = torch.stack([ln.emb.weight.detach() for ln in lns]).index_select(1, self.t)     # [G][B][D] = Emb(t_b)
        self.ada_W = torch.stack([ln.linear.weight.detach() for ln in lns])                        # [G][2D][D]
        self.sample_rows = torch.arange(B, device=self.dev)
        self.tabs = torch.empty(len(lns), B, 2 * D, device=self.dev)
        L_.gemm(torch.nn.functional.silu(self.ada_E), self.ada_W, self.tabs, B, 2 * D, D, groups=len(lns), a_gstride=B * D,
                w_gstride=2 * D * D, c_gstride=B * 2 * D)
        self.tabs += torch.stack([ln.linear.bias.detach() for ln in lns])[:, None, :]

    def adaln_prefixes(self):
        return ["transformer.blocks.%d.%s" % (li, n) for li in range(len(self.tr.blocks)) for n in ("ln1", "ln1_1")]

    def prep_x(self, lin, x, pro=PACK_PLAIN):
        """gemm.prep_x under the linear's forward power of two, with max |x 2^f| folded into the first calibration pass's slot
        of this linear or into the forward monitor (the "fp32" backend: no scale, no monitor)"""
        if self.fwd_amax is not None:
            slot = self.fwd_amax[self.fwd_index.setdefault(lin.key, len(self.fwd_index))]
        else:
            slot = self.fwd_live
        return self.gemm.prep_x(lin, x, pro=pro, scale=2.0 ** self.fwd_exp.get(lin.key, 0), amax=slot)

    # ---- one block: forward, and its backward right below ----------------------------------------------------------------
    def block_fwd(self, li, x):
        """x -> x + proj1(attn1(qkv1(ln1 x))) -> + proj2(attn2(q2(ln1_1 .), kv2(caption))) -> + fc2(gelu2(fc1(ln2 .)))"""
        G_, blk, ls = self.gemm, self.tr.blocks[li], self.blocks[li]
        B, Lx, Lc, D, H, rows = self.B, self.Lx, self.Lc, self.D, self.H, self.sample_rows
        attn, split = self.step.attn_cls, self.step.split_attention
        s = _BlockActs()
        s.x0 = x
        s.h1 = self.prep_x(ls["qkv1"], _norm_fwd(x, 0, Lx, table=self.tabs[2 * li], t=rows))
        qkv = G_.fwd(ls["qkv1"], s.h1)                                            # [M][3D]: q | k | v
        s.att1 = attn((qkv, 0, 3 * D), (qkv, D, 3 * D), (qkv, 2 * D, 3 * D), B, Lx, Lx, H, split=split)
        s.o1 = self.prep_x(ls["proj1"], s.att1.out)
        s.x1 = x = G_.fwd(ls["proj1"], s.o1, R=x)
        s.h2 = self.prep_x(ls["q2"], _norm_fwd(x, 0, Lx, table=self.tabs[2 * li + 1], t=rows))
        q = G_.fwd(ls["q2"], s.h2)
        kv = G_.fwd(ls["kv2"], self.cond_h)                                       # [B*Lc][2D]: k | v
        s.att2 = attn((q, 0, D), (kv, 0, 2 * D), (kv, D, 2 * D), B, Lx, Lc, H, split=split)
        s.o2 = self.prep_x(ls["proj2"], s.att2.out)
        s.x2 = x = G_.fwd(ls["proj2"], s.o2, R=x)
        s.h3 = self.prep_x(ls["fc1"], _norm_fwd(x, 1, Lx, gamma=blk.ln2.weight, beta=blk.ln2.bias))
        s.u = G_.fwd(ls["fc1"], s.h3)
        s.g = self.prep_x(ls["fc2"], s.u, pro=PACK_GELU2)                           # gelu2(u): the f16x2 backend never stores it in fp32
        return s, G_.fwd(ls["fc2"], s.g, R=x)

    def block_bwd(self, li, s, dx):
        """dx: the gradient of the block's output, turned IN PLACE into that of its input (the residual stream's gradient: every
        branch adds its norm-input gradient to it)"""
        g, blk, ls = self.g, self.tr.blocks[li], self.blocks[li]
        B, Lx, Lc, D, M, rows, dev = self.B, self.Lx, self.Lc, self.D, self.M, self.sample_rows, self.dev
        p = "transformer.blocks.%d." % li
        # x3 = x2 + fc2(gelu(fc1(ln2(x2))))
        dgact, g[p + "mlp.2.weight"], g[p + "mlp.2.bias"] = self.lin_bwd(ls["fc2"], s.g, dx)
        # d fc1-output = dgact * gelu2'(u): the prologue of fc1's gradient pack
        dh, g[p + "mlp.0.weight"], g[p + "mlp.0.bias"] = self.lin_bwd(ls["fc1"], s.h3, dgact, pro=PACK_GELU2_BWD, aux=s.u)
        _, sums = _norm_bwd(s.x2, dh, 1, Lx, gamma=blk.ln2.weight, add_to=dx)
        self.norm_gain_grads(p + "ln2", sums)
        # x2 = x1 + proj2(attn2(q(ln1_1(x1)), kv(cond)))
        dao, g[p + "attn2.proj.weight"], g[p + "attn2.proj.bias"] = self.lin_bwd(ls["proj2"], s.o2, dx)
        dq = torch.empty(M, D, device=dev)
        dkv = torch.empty(B * Lc, 2 * D, device=dev)
        slot, dsc = self.att_site("b%d.att2" % li, s.att2)
        s.att2.backward(dao, (dq, 0, D), (dkv, 0, 2 * D), (dkv, D, 2 * D), amax=slot, do_scale=dsc)
        dh, g[p + "attn2.query.weight"], g[p + "attn2.query.bias"] = self.lin_bwd(ls["q2"], s.h2, dq)
        _, dWkv, dbkv = self.lin_bwd(ls["kv2"], self.cond_h, dkv, need_dx=False)
        g[p + "attn2.key.weight"], g[p + "attn2.value.weight"] = dWkv[:D], dWkv[D:]
        g[p + "attn2.key.bias"], g[p + "attn2.value.bias"] = dbkv[:D], dbkv[D:]
        _, self.ada[2 * li + 1] = _norm_bwd(s.x1, dh, 0, Lx, table=self.tabs[2 * li + 1], t=rows, add_to=dx)
        # x1 = x0 + proj1(attn1(qkv(ln1(x0))))
        dao, g[p + "attn1.proj.weight"], g[p + "attn1.proj.bias"] = self.lin_bwd(ls["proj1"], s.o1, dx)
        dqkv = torch.empty(M, 3 * D, device=dev)
        slot, dsc = self.att_site("b%d.att1" % li, s.att1)
        s.att1.backward(dao, (dqkv, 0, 3 * D), (dqkv, D, 3 * D), (dqkv, 2 * D, 3 * D), amax=slot, do_scale=dsc)
        dh, dWqkv, dbqkv = self.lin_bwd(ls["qkv1"], s.h1, dqkv)
        for j, nm in enumerate(("query", "key", "value")):
            g[p + "attn1.%s.weight" % nm], g[p + "attn1.%s.bias" % nm] = dWqkv[j * D:(j + 1) * D], dbqkv[j * D:(j + 1) * D]
        _, self.ada[2 * li] = _norm_bwd(s.x0, dh, 0, Lx, table=self.tabs[2 * li], t=rows, add_to=dx)

    # ---- the pieces of the backward --------------------------------------------------------------------------------------
    def site_slot(self, key):
        """where max |operand| of this site goes: its own slot in the second calibration pass, the monitor's scalar otherwise
        (every gradient that enters a GEMM passes gemm.prep_dy, whose pack folds max |dY 2^e| into it)"""
        if self.site_amax is None:
            return self.amax
        return self.site_amax[self.site_index.setdefault(key, len(self.site_index))]

    def att_site(self, key, att):
        """(monitor slot, this attention backward's own power of two); the composed attention splits nothing: no site"""
        if not att.site:
            return None, 1.0
        return self.site_slot(key), 1.0 if self.site_amax is not None else 2.0 ** self.site_exp.get(key, 0)

    def lin_bwd(self, lin, xh, dy, need_dx=True, pro=PACK_PLAIN, aux=None):
        """The three products of one linear layer for its output gradient dy (fp32; with pro = PACK_GELU2_BWD the
        gradient of the layer's output is dy * gelu2'(aux)).  dy is packed ONCE (gemm.prep_dy: row form, transposed form,
        bias column sums, max |dY|), then dX, dW and db.  (Rounds 2-4 could put dW / db on a second HIP stream; measured
        slower in both rounds it was tried -- 15.6 vs 15.9 and 16.2 vs 16.6 it/s, the GEMMs fill the power-capped chip -- and
        removed in round 5.)"""
        G_ = self.gemm
        # the site's own power of two on top of the loss scale (module docstring; 1 while calibrating)
        e = self.site_exp.get(lin.key, 0)
        up, down = 2.0 ** e, 2.0 ** -e
        dyh = G_.prep_dy(lin, dy, pro=pro, aux=aux, amax=self.site_slot(lin.key), need_row=need_dx, scale=up)
        dxo = G_.dx(lin, dyh, unscale=down) if need_dx else None
        # dW is off the critical path: a backend that pairs products (pairs_dw) gets them collected, side by side (flush_dw)
        dW = torch.empty(lin.N, lin.K, device=self.dev)
        # (... and 2^-f of a forward operand that was packed as x 2^f: the handle knows it; fp32 handles are plain tensors)
        self.pending_dw.append((lin, xh, dyh, self.inv * down * getattr(xh, "unscale", 1.0), dW))
        if not G_.pairs_dw:
            self.flush_dw()
        db = G_.db(lin, dyh)
        self.small.append(db)
        return dxo, dW, db

    def flush_dw(self):
        if self.pending_dw:
            self.gemm.dw_many(self.pending_dw)
            self.pending_dw.clear()

    def hand_over(self, names, now=True):
        """Give the named gradients, final from here on, to on_grads.  now=False: the names wait until the weight gradients of
        TWO blocks are collected (their products then pair up: two qkv gradients in one grid, four MLP ones, ...) -- the
        overlapped reduction gets them one block later.  (A backend that collects nothing never reaches two blocks: the "fp32"
        backend's block gradients all go out in the call after the block loop.)"""
        self.pending_names.extend(names)
        if not now and len(self.pending_dw) < 14:
            return
        self.flush_dw()                          # (the gradients handed over must be final)
        if self.on_grads is not None:
            self.on_grads({n: self.g[n] for n in self.pending_names}, ())
        self.pending_names.clear()

    def norm_gain_grads(self, prefix, sums):
        """LayerNorm's d weight | d bias: the two halves of _norm_bwd's [1][2D] sums (un-scaled at the end)"""
        dgam, dbet = sums[:, :self.D], sums[:, self.D:]
        self.g[prefix + ".weight"], self.g[prefix + ".bias"] = dgam[0], dbet[0]
        self.small += [dgam, dbet]

    def loss_and_dlogits(self, logits):
        """-> (loss as forward() reports it, d loss / d logits [M][K] times the loss scale); the importance-sampling statistics
        of sample_time are updated unless calibrating"""
        dt, x0, xt, t, pt, sched = self.dt, self.x0, self.xt, self.t, self.pt, self.sched
        B, Lx, K, T, dev = self.B, self.Lx, self.K, self.T, self.dev
        kl, nll, kl_aux = (torch.empty(B, Lx, device=dev) for _ in range(3))
        L_.check(L_.lib().ds_loss_tail(L_.ptr(logits), L_.ptr(x0), L_.ptr(xt), L_.ptr(t), L_.ptr(sched), L_.ptr(kl), L_.ptr(nll),
                                       L_.ptr(kl_aux), None, B, Lx, K, T, L_.stream()))
        mask_region = (xt == K).float()
        weight = mask_region * dt.mask_weight[0] + (1.0 - mask_region) * dt.mask_weight[1]
        is0 = (t == 0).float()
        kl_loss = is0 * nll.sum(-1) + (1.0 - is0) * (kl * weight).sum(-1)
        if not self.calibrating:
            lt2 = kl_loss.pow(2)                     # importance-sampling statistics of sample_time (:452-455)
            dt.Lt_history.scatter_(dim=0, index=t, src=(0.1 * lt2 + 0.9 * dt.Lt_history.gather(dim=0, index=t)))
            dt.Lt_count.scatter_add_(dim=0, index=t, src=torch.ones_like(lt2))
        vb = kl_loss / pt
        if dt.auxiliary_loss_weight != 0:
            wa = t.float() / T + 1.0 if dt.adaptive_auxiliary_loss else 1.0
            vb = vb + wa * dt.auxiliary_loss_weight * (is0 * nll.sum(-1) + (1.0 - is0) * (kl_aux * weight).sum(-1)) / pt
        norm = 1.0 / (B * Lx)
        loss = vb.sum() * norm
        dlog = torch.empty(self.M, K, device=dev)
        L_.check(L_.lib().ds_loss_tail_bwd(L_.ptr(logits), L_.ptr(x0), L_.ptr(xt), L_.ptr(t), L_.ptr(pt.contiguous()),
                                           L_.ptr(sched), L_.ptr(dlog), B, Lx, K, T, float(dt.mask_weight[0]),
                                           float(dt.mask_weight[1]), float(dt.auxiliary_loss_weight),
                                           int(bool(dt.adaptive_auxiliary_loss)), L_.stream()))
        dlog.mul_(norm * self.loss_scale)                                                # loss = sum(vb) / (B L); x loss scale
        return loss, dlog

    def adaln_param_grads_all(self):
        """d modulation rows [B][2D] -> emb.weight / linear.{weight, bias} through  mod_b = Linear(SiLU(emb[t_b]))  (AdaLayerNorm,
        transformer_utils.py:134-149) for ALL 2 n_layer AdaLN modules at once: dW = dmod^T silu(e_b) (ds_rows_outer), db = column
        sums of dmod, de[t_b] += (dmod_b W) silu'(e_b) (ds_rows_times_matrix): two passes over the B samples for all modules
        instead of two small GEMMs, three transposing copies and a dozen elementwise launches per module (4 ms of an 82 ms
        iteration in round 4; grouped GEMMs over all T table rows until round 6).  self.ada, ada_E and ada_W are all in forward
        order: the stacked parameters of the forward are used as they are."""
        G, B, D, T, dev, g = len(self.ada), self.B, self.D, self.T, self.dev, self.g
        if G == 0:
            return
        dmod = torch.stack(self.ada) * self.inv                                                # [G][B][2D]
        E = self.ada_E                                                                         # [G][B][D]
        sg = torch.sigmoid(E)
        silu_e = (E * sg).contiguous()                                                         # dW[g] = dmod[g]^T silu(e_b[g]):
        dw = _rows_outer(dmod, silu_e)                                                         # B outer products per module
        # dmod[g] W[g]: B rows against the row-major weights where they lie (ds_rows_times_matrix: no transposed copy of the
        # 38 matrices -- 0.38 ms per iteration -- and no tile program that is mostly padding rows)
        KS = (2 * D) // 256
        ds_ = torch.empty(G, B, D, device=dev)
        for b0 in range(0, B, _ROWS_MAX):               # (the kernel takes <= 32 rows; every row's result is its own)
            nb = min(B - b0, _ROWS_MAX)
            xb = dmod if nb == B else dmod[:, b0:b0 + nb].contiguous()
            part = torch.empty(KS, G, nb, D, device=dev)
            L_.check(L_.lib().ds_rows_times_matrix(L_.ptr(xb), L_.ptr(self.ada_W), L_.ptr(part), G, nb, 2 * D, D, L_.stream()))
            ob = ds_ if nb == B else torch.empty(G, nb, D, device=dev)
            L_.check(L_.lib().ds_colsum(L_.ptr(part), L_.ptr(ob), 1, KS, G * nb * D, G * nb * D, 0, 0, L_.stream()))
            if nb != B:
                ds_[:, b0:b0 + nb] = ob
        # de[g][tau] = sum over the b with t_b = tau of ds_[g][b] silu'(e_b): the same sum of outer products with one-hot rows
        # (samples that share a timestep add up in sample order -- index_add_'s atomics made that order the hardware's)
        onehot = (self.t[:, None] == torch.arange(T, device=dev)).float().expand(G, B, T).contiguous()   # [G][B][T]
        de = _rows_outer(onehot, (ds_ * (sg * (1.0 + E * (1.0 - sg)))).contiguous())
        dbias = dmod.sum(1)                                                                    # [G][2D]
        for i, pfx in enumerate(self.adaln_prefixes()):
            g[pfx + ".emb.weight"], g[pfx + ".linear.weight"], g[pfx + ".linear.bias"] = de[i], dw[i], dbias[i]

    def embed_bwd(self, dx):
        """dx [M][D] -> the token table's gradient (scatter-add over the noised tokens) and the two position tables' (sums of
        dx over the batch, then over the other spatial axis)"""
        emb, g, dev = self.tr.content_emb, self.g, self.dev
        B, Lx, D, M = self.B, self.Lx, self.D, self.M
        demb = torch.zeros_like(emb.emb.weight)
        nw = L_.lib().ds_embed_bwd_work_floats(M, D, demb.shape[0])
        ework = torch.empty(nw, device=dev)
        L_.check(L_.lib().ds_embed_bwd_ws(L_.ptr(dx), L_.ptr(self.xt), L_.ptr(demb), M, D, demb.shape[0], L_.ptr(ework), nw,
                                          L_.stream()))
        g["transformer.content_emb.emb.weight"] = demb
        dpos = torch.empty(Lx, D, device=dev)
        L_.check(L_.lib().ds_colsum(L_.ptr(dx), L_.ptr(dpos), Lx, B, D, Lx * D, D, 0, L_.stream()))
        Hh, Ww = emb.spatial_size
        dhh = _colsum(dpos.view(Hh, Ww, D).reshape(Hh * Ww, D), Hh)                                     # sum over w
        g["transformer.content_emb.height_emb.weight"] = dhh
        dw = torch.empty(Ww, D, device=dev)
        L_.check(L_.lib().ds_colsum(L_.ptr(dpos), L_.ptr(dw), Ww, Hh, D, Ww * D, D, 0, L_.stream()))   # sum over h
        g["transformer.content_emb.width_emb.weight"] = dw
        self.small += [demb, dhh, dw]


class TrainStep:
    def __init__(self, diffusion_transformer, precision="fp32", rescale_interval=100, attention="fused"):
        assert precision in ("f16x2", "fp32") and attention in ("fused", "composed")
        self.attention = attention
        self.attn_cls = _FusedAttn if attention == "fused" else _Attn
        # fused attention FORWARD on the streamed fp16-split kernel of the sampling path (ds_attention_f16x2) in the "f16x2"
        # backend: 122 -> ~35 us per self-attention launch at B = 20; gradient parity unchanged (tests/test_hip_train_kernels.py)
        self.split_attention = precision == "f16x2"
        self.dt = diffusion_transformer
        self.tr = diffusion_transformer.transformer
        self.precision = precision
        self.gemm = _SplitGemm() if precision == "f16x2" else _Fp32Gemm()
        self.rescale_interval = rescale_interval
        # the loss scale, the per-site exponents and the monitors that guard them (modeling/loss_scale.py); the "fp32" backend
        # scales nothing: loss_scale_exp is 0 and every check answers False
        self.policy = LossScalePolicy(enabled=precision == "f16x2")
        self.calibrated_amax = None
        self._steps = 0
        self._capturing = False     # set by GraphedIteration while a hipGraph records the step: no host syncs then
        # weight swaps outside this class (checkpoint / EMA loads: solver._invalidate) must drop the cached pre-scales
        import weakref
        diffusion_transformer.__dict__.setdefault("_scale_clients", []).append(weakref.ref(self))

    # ---- the loss-scale policy's public face (solver.py, train_bench.py and the tests address the step) -------------------
    loss_scale_exp = property(lambda self: self.policy.loss_scale_exp, lambda self, v: setattr(self.policy, "loss_scale_exp", v))
    calib_log2 = property(lambda self: self.policy.calib_log2, lambda self, v: setattr(self.policy, "calib_log2", v))
    monitor_window = property(lambda self: self.policy.monitor_window, lambda self, v: setattr(self.policy, "monitor_window", v))
    monitor_log = property(lambda self: self.policy.monitor_log)
    last_trip = property(lambda self: self.policy.last_trip)

    def check_loss_scale(self, force=False):
        """The saturation monitor's host check (LossScalePolicy.check_loss_scale): True when the next step must re-calibrate"""
        return self.policy.check_loss_scale(force=force)

    def observe_grad_norm(self, norm):
        """The gradient-norm guard (LossScalePolicy.observe_grad_norm): True when the next step must re-calibrate"""
        return self.policy.observe_grad_norm(norm)

    def reset_scales(self, weights_replaced=True):
        """Forget the per-matrix weight pre-scales 2^s and the loss scale: the next step re-derives both (one calibration
        backward).  Called after the weights were replaced behind this object's back (solver._invalidate) -- then what the
        saturation monitor had learnt about the OLD weights' gradients (`_target_drop`) goes too -- and, with
        weights_replaced=False, by a re-capture of the same run (the bound is exactly what that re-calibration needs)."""
        self.policy.reset(weights_replaced)
        if self.precision == "f16x2":
            self.gemm.wexp.clear()
        # a captured iteration (GraphedIteration) has the OLD pre-scales and loss scale baked into its graph: it must be
        # re-captured BEFORE its next replay (swapped-in weights a few times larger would saturate the fp16 planes silently)
        self._scales_epoch = getattr(self, "_scales_epoch", 0) + 1

    @torch.no_grad()
    def prescales_drifted(self):
        """Host check of the weight pre-scales 2^s a CAPTURED iteration froze (the eager step simply refreshes them every
        `rescale_interval` steps): one host sync over max |W| of every matrix.  True when a matrix has outgrown its place --
        max |W| 2^s has reached 2^14, one bit of fp16's range left for the replays until the next check -- or has fallen more
        than two bits under it (2 of the split's 22 bits lost), or when there are no pre-scales at all (weights were swapped)."""
        if self.precision != "f16x2":
            return False
        old = self.gemm.wexp
        if not old:
            return True
        blocks, lin_logits = self._linears()
        new = self.gemm.scales_of([l for b in blocks for l in b.values()] + [lin_logits])
        return any(k not in old or s < old[k] or s > old[k] + 2 for k, s in new.items())

    # ---- the step's linears ------------------------------------------------------------------------------------------
    def _linears(self):
        """[(per-block dict), ..., logits]: fused weights are concatenated here once per step (query | key | value rows)."""
        tr = self.tr
        out = []
        for li, blk in enumerate(tr.blocks):
            a1, a2 = blk.attn1, blk.attn2
            p = "b%d." % li
            out.append({
                "qkv1": _Linear(p + "qkv1", (a1.query.weight, a1.key.weight, a1.value.weight),
                                (a1.query.bias, a1.key.bias, a1.value.bias)),
                "proj1": _Linear(p + "proj1", a1.proj.weight.detach(), a1.proj.bias.detach()),
                "q2": _Linear(p + "q2", a2.query.weight.detach(), a2.query.bias.detach()),
                "kv2": _Linear(p + "kv2", (a2.key.weight, a2.value.weight), (a2.key.bias, a2.value.bias)),
                "proj2": _Linear(p + "proj2", a2.proj.weight.detach(), a2.proj.bias.detach()),
                "fc1": _Linear(p + "fc1", blk.mlp[0].weight.detach(), blk.mlp[0].bias.detach()),
                "fc2": _Linear(p + "fc2", blk.mlp[2].weight.detach(), blk.mlp[2].bias.detach()),
            })
        lin = tr.to_logits[1]
        return out, _Linear("logits", lin.weight.detach(), lin.bias.detach())

    @torch.no_grad()
    def loss_and_grads(self, x0, cond_emb, t, pt, noise, on_grads=None):
        """x0 i64[B, L] clean tokens, cond_emb f32[B, 77, 512], t i64[B], pt f32[B] (sample_time's output), noise
        f32[B, K+1, L] uniforms for q_sample.  Returns (loss scalar as forward() reports it, {parameter name relative to
        the DiffusionTransformer: gradient}).  Gradients are those of that loss.
        on_grads(named, streams): called during the backward -- after the logits layer and after every transformer block,
        last block first -- with the WEIGHT-matrix gradients that are final at that point (76 % of the bytes), then once
        after the block loop with the AdaLN tables' parameter gradients (22 %: they come out of two grouped GEMMs over all
        modules); biases and norm gains are un-scaled in one multiply at the very end and stay with finish().  `streams`:
        the streams that wrote them.  The hook of the overlapped data-parallel reduction (shard.GradientReducer.ready)."""
        if self.loss_scale_exp is None:
            self.calibrate(x0, cond_emb, t, pt, noise)
        return self._run(x0, cond_emb, t, pt, noise, on_grads=on_grads)

    @torch.no_grad()
    def calibrate(self, x0, cond_emb, t, pt, noise):
        """Loss scale of the "f16x2" backend from one unscaled backward on this batch: the largest |dY| that enters a GEMM
        is put at 2^12..2^13 (fp16 overflows at 2^16; a split value keeps 2^-25 absolutely).  One host sync.  The
        importance-sampling statistics (Lt_history / Lt_count) are not touched."""
        if self.precision != "f16x2":
            return 0
        pol, batch = self.policy, (x0, cond_emb, t, pt, noise)
        pol.begin_calibration()
        # (the forward operands ride along in the same pass and the same host sync: max |x| of every linear's input -> the
        #  power of two 2^f <= 1 that keeps it under 2^13, LossScalePolicy.fwd_exponents; slot 0 is the gradients' maximum)
        n_lin = 6 * len(self.tr.blocks) + 2                                  # 6 per block + the caption rows (kv2) + the logits layer
        probe = torch.zeros(1 + n_lin, device=x0.device)
        first = _Pass(self, *batch, calibrating=True, amax=probe[0], fwd_amax=probe[1:])
        first.run()
        m, *per_lin = probe.tolist()
        assert len(first.fwd_index) == n_lin, (len(first.fwd_index), n_lin)
        pol.fwd_exp = pol.fwd_exponents(list(first.fwd_index), per_lin)
        self.calibrated_amax = m
        # Second pass, under that provisional scale (unscaled, the deep sites' operands flush to 0): the largest value of EVERY
        # operand the backward splits to fp16 under the loss scale -- max |dY| per linear (its dY feeds the dX and dW GEMMs)
        # and max |dO| over the attention backwards -- in one more host sync.  One scale for the whole backward leaves the small gradients
        # behind: against the reference at 19 layers / B = 20 (tests/test_hip_train_batch.py) the cross-attention query
        # projections -- whose dY is a softmax gradient of near-uniform probabilities, 2^-14 of the largest dY -- came out with
        # 1e-2 relative error, their fp16 lo plane under the subnormal range (the reference's own fp32: 6e-7).  So
        # every SITE gets its own power of two on top of the loss scale (the fp32 tensors in between carry the loss scale without
        # harm, whatever it is): a linear's dY 2^e is what is split (ds_pack_operand `scale`) and 2^-e goes into its dX / dW
        # epilogues; an attention backward's dO 2^e is what its kernels split and their stores take 2^-e out again (they
        # normalise their in-register dS by themselves) -- all exact.
        pol.loss_scale_exp = pol._exp_from_amax(m)
        n_sites = 9 * len(self.tr.blocks) + 1                                # 7 linears + 2 attentions per block, + the logits layer
        sites = torch.zeros(n_sites, device=x0.device)                       # in the order the backward visits them
        second = _Pass(self, *batch, calibrating=True, amax=torch.zeros(1, device=x0.device), site_amax=sites)
        second.run()
        per_site = sites.tolist()
        assert len(second.site_index) == n_sites or self.attention != "fused", (len(second.site_index), n_sites)
        pol._site_exp = pol.site_exponents(list(second.site_index), per_site)
        return pol.loss_scale_exp

    def _run(self, x0, cond_emb, t, pt, noise, on_grads=None):
        """One training step under the calibrated scales (eager, or while a hipGraph records it: GraphedIteration)"""
        loss, grads = _Pass(self, x0, cond_emb, t, pt, noise, calibrating=False, on_grads=on_grads).run()
        self._steps += 1
        self.policy._last_loss = loss       # (device scalar; a captured iteration keeps updating this very tensor)
        return loss, grads

    # ---- optimizer -------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def adamw_step(self, grads, state, step, lr, betas=(0.9, 0.96), eps=1e-8, weight_decay=4.5e-2, hyper=None):
        """In-place AdamW on the parameters that have a gradient (state: dict name -> (m, v), created on first use).
        hyper: optional f32[4] device tensor { lr, 1 - beta1^step, sqrt(1 - beta2^step), grad_scale } -- then `step` / `lr`
        are ignored and the launch arguments do not depend on the iteration (captured graphs: `capture`)."""
        params = dict(self.dt.named_parameters())
        if hyper is not None:
            # one batched launch per 64 tensors (ds_adamw_multi: descriptors by value in the kernel arguments -- capturable)
            import ctypes
            names = list(grads)
            rec = (ctypes.c_int64 * (5 * len(names)))()
            keep = []
            for i, name in enumerate(names):
                p_ = params[name]
                if name not in state:
                    state[name] = (torch.zeros_like(p_), torch.zeros_like(p_))
                m, v = state[name]
                gr = grads[name].contiguous()
                keep.append(gr)
                assert gr.numel() == p_.numel() and p_.data.is_contiguous() and m.is_contiguous() and v.is_contiguous()
                rec[5 * i:5 * i + 5] = [p_.data.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), p_.numel()]
            L_.check(L_.lib().ds_adamw_multi(ctypes.cast(rec, ctypes.c_void_p), len(names), L_.ptr(hyper), betas[0], betas[1], eps,
                                             weight_decay, L_.stream()))
            self.tr.invalidate()
            return
        for name, gr in grads.items():
            p_ = params[name]
            if name not in state:
                state[name] = (torch.zeros_like(p_), torch.zeros_like(p_))
            m, v = state[name]
            gr = gr.contiguous()
            L_.check(L_.lib().ds_adamw(L_.ptr(p_.data), L_.ptr(gr), L_.ptr(m), L_.ptr(v), p_.numel(), lr, betas[0], betas[1],
                                       eps, weight_decay, step, L_.stream()))
        self.tr.invalidate()       # cached weight packs / AdaLN tables are stale now (frees the native handle too)

    # ---- the whole iteration as ONE hipGraph -----------------------------------------------------------------------------
    def capture(self, x0, cond_emb, t, pt, noise, betas=(0.9, 0.96), eps=1e-8, weight_decay=4.5e-2, max_norm=None,
                reduce=None):
        """Capture  loss_and_grads -> global-norm clip -> AdamW  (engine/solver_spec.py:308-331's order) on static copies of
        the batch tensors into one hipGraph and return a `GraphedIteration`: `it(x0, cond_emb, t, pt, noise, lr)` copies
        the batch in, refreshes the 4 device scalars of the update and replays -- one graph launch per training iteration.
        Data-parallel form: `reduce(grads)` (e.g. shard.allreduce_gradients: averages the gradient tensors over the
        ranks, in place, on the current stream) makes it TWO graphs per rank -- gradients | clip + AdamW -- with the
        reduction enqueued between the two replays (engine/solver_spec.py:109: DDP reduces before the optimizer step).
        The loss scale and the weight pre-scales are the calibrated constants of capture time; `recapture()` refreshes them."""
        return GraphedIteration(self, (x0, cond_emb, t, pt, noise), betas, eps, weight_decay, max_norm, reduce=reduce)


class GraphedIteration:
    def __init__(self, step, batch, betas, eps, weight_decay, max_norm, reduce=None):
        self.step, self.betas, self.eps, self.weight_decay, self.max_norm = step, betas, eps, weight_decay, max_norm
        self.reduce = reduce                 # None: one graph; callable(grads): gradients graph | reduce | update graph
        self.static = [b.clone() for b in batch]
        self.hyper = torch.zeros(4, device=batch[0].device)
        self.opt_state = {}
        self.iteration = 0
        self.graph = None
        self.update_graph = None
        self._capture()

    @torch.no_grad()
    def _capture(self):
        st = self.step
        dev = self.static[0].device
        if st.loss_scale_exp is None:
            st.calibrate(*self.static)
        # warm-up on a side stream (lazy initialisation inside the library, allocator pools), with lr = 0 and every
        # statistic restored afterwards so that the warm-up leaves no trace in the training state
        dt = st.dt
        keep = (dt.Lt_history.clone(), dt.Lt_count.clone(), st._steps)
        self.hyper.copy_(torch.tensor([0.0, 1.0, 1.0, 0.0]))
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._body()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        for name, (m, v) in self.opt_state.items():
            m.zero_()
            v.zero_()
        self.graph = torch.cuda.CUDAGraph()
        self.update_graph = None
        self._scales_epoch = getattr(st, "_scales_epoch", 0)     # the scales this graph bakes in (TrainStep.reset_scales bumps it)
        st._capturing = True
        try:
            if self.reduce is None:
                with torch.cuda.graph(self.graph):
                    self._body()
            else:       # two segments sharing one memory pool: the gradient tensors of the first are the second's inputs
                with torch.cuda.graph(self.graph):
                    self._body_grads()
                self.update_graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.update_graph, pool=self.graph.pool()):
                    self._body_update()
        finally:
            st._capturing = False
        dt.Lt_history.copy_(keep[0])
        dt.Lt_count.copy_(keep[1])
        st._steps = keep[2]

    def _body(self):                       # (the warm-up runs it un-reduced on every rank alike: lr = 0, state restored)
        self._body_grads()
        self._body_update()

    def _body_grads(self):
        self.loss, self.grads = self.step._run(*self.static)

    def _body_update(self):
        st, loss, grads = self.step, self.loss, self.grads
        # global gradient norm + clip coefficient (torch.nn.utils.clip_grad_norm_: coef = max_norm / (norm + 1e-6), <= 1) in two
        # launches, the coefficient written straight into the AdamW kernel's hyper[3] (ds_grad_norm_multi)
        import ctypes
        tensors = [g_.contiguous() for g_ in grads.values()]
        assert all(g_.dtype == torch.float32 for g_ in tensors)
        rec = (ctypes.c_int64 * (2 * len(tensors)))()
        chunks = 0
        for i, g_ in enumerate(tensors):
            rec[2 * i:2 * i + 2] = [g_.data_ptr(), g_.numel()]
            chunks += (g_.numel() + 4095) // 4096
        part = torch.empty(chunks, dtype=torch.float64, device=self.hyper.device)
        total1 = torch.empty(1, device=self.hyper.device)
        L_.check(L_.lib().ds_grad_norm_multi(ctypes.cast(rec, ctypes.c_void_p), len(tensors), L_.ptr(part), chunks,
                                             float(self.max_norm) if self.max_norm is not None else 0.0, L_.ptr(total1),
                                             L_.ptr_off(self.hyper, 3) if self.max_norm is not None else None, L_.stream()))
        self._norm_keep = (tensors, part)              # alive until the launches are enqueued / for the life of the captured graph
        total = total1.reshape(())
        st.adamw_step(grads, self.opt_state, 0, 0.0, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay,
                      hyper=self.hyper)
        self.loss, self.grad_norm, self.grads = loss, total, grads

    def recapture(self, static=None, reason="requested"):
        """New calibration of the loss scale / weight pre-scales on the current static batch (or `static`, the batch about
        to run), then a new graph.  `reason` is kept (recapture_reasons: what a long run's log shows next to its rate)."""
        if static is not None:
            for dst, src in zip(self.static, static):
                dst.copy_(src)
        self.recaptures = getattr(self, "recaptures", 0) + 1
        self.recapture_reasons = getattr(self, "recapture_reasons", []) + ["iteration %d: %s" % (self.iteration, reason)]
        self.step.reset_scales(weights_replaced=False)
        keep_state = {k: (m.clone(), v.clone()) for k, (m, v) in self.opt_state.items()}
        self._capture()
        for k, (m, v) in keep_state.items():
            self.opt_state[k][0].copy_(m)
            self.opt_state[k][1].copy_(v)
        self._replays = 0

    def state_dict(self):
        """What a resumed run needs of the captured iteration: the AdamW moments (they live in the graph's static tensors)
        and the bias-correction counter."""
        return {"iteration": self.iteration, "optimizer": {k: (m.clone(), v.clone()) for k, (m, v) in self.opt_state.items()}}

    @torch.no_grad()
    def load_state_dict(self, state):
        """In place into the tensors the graph updates (no re-capture needed)."""
        self.iteration = int(state["iteration"])
        missing = [k for k in self.opt_state if k not in state["optimizer"]]
        extra = [k for k in state["optimizer"] if k not in self.opt_state]
        if missing or extra:
            raise RuntimeError("GraphedIteration.load_state_dict: missing %s, unexpected %s" % (missing, extra))
        for k, (m, v) in state["optimizer"].items():
            self.opt_state[k][0].copy_(m)
            self.opt_state[k][1].copy_(v)

    @torch.no_grad()
    def __call__(self, x0, cond_emb, t, pt, noise, lr):
        if getattr(self.step, "_scales_epoch", 0) != self._scales_epoch:
            # the weights were replaced behind the graph (checkpoint / EMA load -> TrainStep.reset_scales): its frozen
            # pre-scales belong to the old weights.  Re-capture on THIS batch before anything is replayed.
            self.recapture(static=(x0, cond_emb, t, pt, noise), reason="weights replaced (reset_scales)")
        for dst, src in zip(self.static, (x0, cond_emb, t, pt, noise)):
            dst.copy_(src)
        self.iteration += 1
        b1, b2 = self.betas
        self.hyper[:3].copy_(torch.tensor([lr, 1.0 - b1 ** self.iteration, math.sqrt(1.0 - b2 ** self.iteration)]))
        if self.max_norm is None:
            self.hyper[3:4].fill_(1.0)
        self.graph.replay()
        if self.update_graph is not None:
            self.reduce(self.grads)        # in place on the graph's own gradient tensors, stream-ordered between the replays
            self.update_graph.replay()
        self.step._steps += 1
        self._replays = getattr(self, "_replays", 0) + 1
        self.step.tr.invalidate()          # the replay updated the weights: cached inference packs are stale
        return {"loss": self.loss, "grad_norm": self.grad_norm, "lr": lr}

    def check_loss_scale(self):
        """Host-side guards of the frozen constants of a captured iteration.  (1) The weight pre-scales 2^s are those of
        capture time -- the eager step refreshes them every `rescale_interval` steps, a replay cannot: after that many
        replays the weights are looked at (TrainStep.prescales_drifted, one host sync) and the iteration is re-captured only
        if a matrix has left its place.  (Until round 5 this re-captured unconditionally: ~1.9 s per 100 replays of 57 ms,
        a quarter of a long run -- profiles/r05last_monitor_ab.txt.)  (2) The saturation monitor (max |scaled dY|,
        TrainStep.check_loss_scale) is read every `monitor_interval` replays -- one host sync then, none in between -- and
        re-captures when the gradients have left the calibrated window."""
        st = self.step
        if getattr(self, "_replays", 0) >= max(1, st.rescale_interval):
            self._replays = 0
            if st.prescales_drifted():
                self.recapture(reason="a weight pre-scale 2^s left its place")
                return True
        if st.check_loss_scale():
            self.recapture(reason=getattr(st, "last_trip", None) or "saturation monitor")
            return True
        return False
