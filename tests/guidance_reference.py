"""The yardstick of the classifier-free guidance tests: the guided tail and the guided reverse chain, composed on the CPU
from the oracle's pieces (oracle/diffsound_oracle.py: predict_start, truncate_top_r / truncate_top_k, q_posterior,
gumbel_sample, transformer_forward, log_onehot, make_schedule) -- never importing the package's sampler.

    lc = predict_start(zc), lu = predict_start(zu)      zc: logits under the caption, zu: under the null condition
    g  = lu + s (lc - lu),  g <- g - logsumexp(g)        float64, max-shifted; over the K real classes
    log_pred = clamp(round(g), -70, 0), [MASK] row -70   -> truncation, q_posterior, Gumbel-argmax as in the oracle

dtype = float32 is the arithmetic as specified (the kernel's: predict_start and the mix computed in float64 and rounded to
float32, everything after it in float32); dtype = float64 rounds nowhere.  The distance between the two is the rounding
error the specification itself allows, and the tests' tolerances are multiples of it."""
import torch

import diffsound_oracle as O
from inpaint_reference import chain_steps

L = 265


def guided_log_pred(lc, lu, s, dtype=torch.float32):
    """lc, lu: predict_start(z, dtype) of the two logit tensors, [B, K+1, L] -> the guided log_pred [B, K+1, L] in dtype"""
    c, u = lc[:, :-1].double(), lu[:, :-1].double()
    g = u + float(s) * (c - u)
    m = g.max(dim=1, keepdim=True).values
    g = (g - m) - torch.log(torch.exp(g - m).sum(dim=1, keepdim=True))
    g = g.to(dtype)
    g = torch.cat((g, torch.full_like(g[:, :1, :], -70.0)), dim=1)
    return g.clamp(-70.0, 0.0)


def guided_step(sched, zc, zu, s, log_z, t, u, trunc_r=0.85, trunc_k=None, t_post=None, dtype=torch.float32):
    """One guided tail on given logits zc, zu [B, K, L] and state log_z [B, K+1, L].  Returns a dict: log_pred, trunc, post
    [B, K+1, L], tokens i64[B, L] and gap [B, L] (best minus second-best Gumbel score of every decision)."""
    log_pred = guided_log_pred(O.predict_start(zc, dtype), O.predict_start(zu, dtype), s, dtype)
    if trunc_k is not None:
        trunc = O.truncate_top_k(log_pred, trunc_k)
    else:
        trunc = O.truncate_top_r(log_pred, trunc_r) if trunc_r is not None else log_pred
    post = O.q_posterior(sched, trunc, log_z, t if t_post is None else t_post)
    score = -torch.log(-torch.log(u + 1e-30) + 1e-30) + post
    top2 = score.topk(2, dim=1).values
    tokens = O.gumbel_sample(post, u)
    assert torch.equal(tokens, score.argmax(1))
    return dict(log_pred=log_pred, trunc=trunc, post=post, tokens=tokens, gap=top2[:, 0] - top2[:, 1])


def plain_step(sched, z, log_z, t, u, trunc_r=0.85):
    """the oracle's own (unguided) tail on logits z: tokens i64[B, L]"""
    trunc = O.truncate_top_r(O.predict_start(z), trunc_r)
    return O.gumbel_sample(O.q_posterior(sched, trunc, log_z, t), u)


def guided_loop(sd, cond, null, s, noise_fn, T=100, trunc_r=0.85, skip_step=0, keep=None, known=None, record=None,
                dtype=torch.float32, n_head=16):
    """The guided reverse chain: cond, null f32[B, 77, 512]; noise_fn(call index, shape) -> uniforms.  keep bool[B, L] /
    known i64[B, L]: positions held clean between the calls (the clamp mode of tests/inpaint_reference.py).  Returns
    (tokens i64[B, L], the smallest Gumbel gap over all free decisions of the chain); record: the tokens after every call.
    dtype = float64 runs the denoiser, the guidance and the tail in float64."""
    K = sd["transformer.transformer.to_logits.1.weight"].shape[0]
    B = cond.shape[0]
    shape = (B, K + 1, L)
    sched = O.make_schedule(T, K + 1)
    if dtype != torch.float32:
        sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        cond, null = cond.to(dtype), null.to(dtype)
    log_z = O.initial_log_z(B, K + 1, L)
    free = torch.ones(B, L, dtype=torch.bool)
    if keep is not None:
        log_known = O.log_onehot(known, K + 1)
        log_z = torch.where(keep[:, None, :], log_known, log_z)
        free = ~keep
    min_gap = float("inf")
    for k, (st, sp) in enumerate(chain_steps(T, skip_step)):
        t = torch.full((B,), st, dtype=torch.long)
        x_t = log_z.argmax(1)
        zc = O.transformer_forward(sd, x_t, cond, t, n_head=n_head)
        zu = O.transformer_forward(sd, x_t, null, t, n_head=n_head)
        d = guided_step(sched, zc, zu, s, log_z, t, noise_fn(k, shape), trunc_r, t_post=torch.full((B,), sp, dtype=torch.long),
                        dtype=dtype)
        min_gap = min(min_gap, float(d["gap"][free].min()))
        log_z = O.log_onehot(d["tokens"], K + 1)
        if keep is not None:
            log_z = torch.where(keep[:, None, :], log_known, log_z)
        if record is not None:
            record.append(log_z.argmax(1).clone())
    return log_z.argmax(1), min_gap
