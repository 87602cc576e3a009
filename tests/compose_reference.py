"""The yardstick of the caption-track tests: the composed tail and the composed reverse chain, restated on the CPU from the
oracle's pieces (oracle/diffsound_oracle.py: predict_start, truncate_top_r / truncate_top_k, q_posterior, gumbel_sample,
transformer_forward, log_onehot, make_schedule) -- never importing the package's sampler.

    lu = predict_start(z_null), l_i = predict_start(z_i)       z_i: logits under track i's caption, i = 0 .. C-1
    g  = lu;  for i in index order: g = g + w_i (l_i - lu)     float64; w f[B, C, L], one weight per grid position
    g <- g - logsumexp(g)                                      max-shifted; over the K real classes
    log_pred = clamp(round(g), -70, 0), [MASK] row -70         -> truncation, q_posterior, Gumbel-argmax as in the oracle

A track whose weight is 0 at a position contributes exactly 0 there whatever its logits hold: the restatement selects the
term away (torch.where), as the kernel does not read the row.  dtype = float32 is the arithmetic as specified (predict_start
and the mix computed in float64 and rounded to float32, everything after it in float32); dtype = float64 rounds nowhere.  The
distance between the two is the rounding error the specification itself allows, and the tests' tolerances are multiples of it."""
import torch

import diffsound_oracle as O
from inpaint_reference import chain_steps

L = 265


def composed_log_pred(lt, lu, w, dtype=torch.float32):
    """lt: list of C predict_start(z_i, dtype) [B, K+1, L]; lu: predict_start(z_null, dtype); w [B, C, L] -> the composed
    log_pred [B, K+1, L] in dtype"""
    u = lu[:, :-1].double()
    g = u.clone()
    for i, li in enumerate(lt):
        wi = w[:, i].double()[:, None, :]
        g = g + torch.where(wi != 0, wi * (li[:, :-1].double() - u), torch.zeros_like(u))
    m = g.max(dim=1, keepdim=True).values
    g = (g - m) - torch.log(torch.exp(g - m).sum(dim=1, keepdim=True))
    g = g.to(dtype)
    g = torch.cat((g, torch.full_like(g[:, :1, :], -70.0)), dim=1)
    return g.clamp(-70.0, 0.0)


def composed_step(sched, zt, zu, w, log_z, t, u, trunc_r=0.85, trunc_k=None, t_post=None, dtype=torch.float32):
    """One composed tail on given logits zt (list of C [B, K, L]), zu [B, K, L], weights w [B, C, L] and state log_z
    [B, K+1, L].  Returns a dict: log_pred, trunc, post [B, K+1, L], tokens i64[B, L] and gap [B, L] (best minus second-best
    Gumbel score of every decision)."""
    log_pred = composed_log_pred([O.predict_start(z, dtype) for z in zt], O.predict_start(zu, dtype), w, dtype)
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


def composed_loop(sd, conds, null, w, noise_fn, T=100, trunc_r=0.85, skip_step=0, keep=None, known=None, record=None,
                  dtype=torch.float32, n_head=16):
    """The composed reverse chain: conds f32[C, B, 77, 512], null f32[B, 77, 512], w f32[B, C, L]; noise_fn(call index, shape)
    -> uniforms.  keep bool[B, L] / known i64[B, L]: positions held clean between the calls (the clamp mode of
    tests/inpaint_reference.py).  Returns (tokens i64[B, L], the smallest Gumbel gap over all free decisions of the chain);
    record: the tokens after every call.  dtype = float64 runs the denoiser, the mix and the tail in float64."""
    K = sd["transformer.transformer.to_logits.1.weight"].shape[0]
    B = null.shape[0]
    shape = (B, K + 1, L)
    sched = O.make_schedule(T, K + 1)
    if dtype != torch.float32:
        sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        conds, null = conds.to(dtype), null.to(dtype)
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
        zt = [O.transformer_forward(sd, x_t, c, t, n_head=n_head) for c in conds]
        zu = O.transformer_forward(sd, x_t, null, t, n_head=n_head)
        d = composed_step(sched, zt, zu, w, log_z, t, noise_fn(k, shape), trunc_r, t_post=torch.full((B,), sp, dtype=torch.long),
                          dtype=dtype)
        min_gap = min(min_gap, float(d["gap"][free].min()))
        log_z = O.log_onehot(d["tokens"], K + 1)
        if keep is not None:
            log_z = torch.where(keep[:, None, :], log_known, log_z)
        if record is not None:
            record.append(log_z.argmax(1).clone())
    return log_z.argmax(1), min_gap
