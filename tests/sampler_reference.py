"""The yardstick of the plain sampling tail and of q_sample (tests/test_sampler_host.py, tests/test_hip_sampler_edges.py),
composed on the CPU from the oracle's pieces (oracle/diffsound_oracle.py: predict_start, q_posterior, _q_pred, log_onehot,
make_schedule) -- never importing the package's sampler.

    log_pred = clamp(round(log_softmax_f64(z)), -70, 0), [MASK] row -70
    trunc    = top-r (mass ranked before a class < r), top-k (rank < k) or log_pred itself
    post     = q_posterior(trunc, log_z, t);  token = argmax(-log(-log(u + 1e-30) + 1e-30) + post)

dtype = float32 is the arithmetic as specified (the kernel's: the log-softmax in float64 rounded to float32, everything
after it in float32); dtype = float64 rounds nowhere: the float32 schedule buffers, the state and the uniforms are cast up
and every operation after the logits runs in double.  The distance between the two is the rounding error the specification
itself allows, and the tests' tolerances are multiples of it.

Three differences from the oracle's own functions, on purpose:
  * a STABLE ranking in both truncations (torch.sort(..., descending=True, stable=True)).  The reference's unstable sort
    and topk leave the survivor among exactly equal log-probabilities unspecified; the kernel's documented rule is "lower
    class index first", which is what a stable descending sort gives.
  * the rate as float32: the mass is compared with numpy.float32(r) in both dtypes, as the kernel holds it.
  * the float64 log-softmax as log n + log1p(rest / n) (n: the classes at the column's maximum, rest: the sum of
    exp(z - max) over the others).  F.log_softmax forms log(1 + rest), whose ABSOLUTE error of 1e-16 is a relative error of
    1e-16 / rest in the dominant class's entry -rest: more than a float32 ulp once that class holds all but 2e-9 of the
    mass.  The yardstick has to resolve one float32 ulp at every entry's magnitude, so it must not lose it there; the
    float32 form stays the oracle's predict_start, the arithmetic as specified."""
import numpy as np
import torch

import diffsound_oracle as O

SCHED_ROWS = ("log_at", "log_bt", "log_ct", "log_1_min_ct", "log_cumprod_at", "log_cumprod_bt", "log_cumprod_ct",
              "log_1_min_cumprod_ct")


def sched_table(sched):
    """the kernels' [8][T + 1] table of a schedule dict (the per-step rows have T entries, the cumulative ones T + 1)"""
    T = sched["log_at"].numel()
    tab = torch.zeros(8, T + 1)
    for i, n in enumerate(SCHED_ROWS):
        tab[i, :sched[n].numel()] = sched[n]
    return tab


def truncate_top_r(log_pred, r):
    """rank i of a stable descending sort survives iff the mass of ranks 0 .. i-1 is < float32(r) (rank 0 always)"""
    srt, idx = torch.sort(log_pred, dim=1, descending=True, stable=True)
    inc = torch.exp(srt).cumsum(dim=1)
    ks = torch.cat((torch.ones_like(inc[:, :1, :], dtype=torch.bool), (inc < float(np.float32(r)))[:, :-1, :]), dim=1)
    keep = torch.zeros_like(ks).scatter(1, idx, ks)
    return torch.where(keep, log_pred, torch.full_like(log_pred, -70.0))


def truncate_top_k(log_pred, k):
    """the first k ranks of a stable descending sort keep their value, every other row becomes -70"""
    idx = torch.sort(log_pred, dim=1, descending=True, stable=True)[1][:, :k, :]
    keep = torch.zeros_like(log_pred, dtype=torch.bool).scatter(1, idx, torch.ones_like(idx, dtype=torch.bool))
    return torch.where(keep, log_pred, torch.full_like(log_pred, -70.0))


def predict_start(z, dtype=torch.float32):
    """float32: the oracle's predict_start.  float64: the same quantity from log n + log1p(rest / n) (module docstring)."""
    if dtype != torch.float64:
        return O.predict_start(z, dtype)
    z = z.double()
    mx = z.max(dim=1, keepdim=True).values
    top = z == mx
    n = top.sum(dim=1, keepdim=True).double()
    rest = torch.where(top, torch.zeros_like(z), torch.exp(z - mx)).sum(dim=1, keepdim=True)
    lp = (z - mx) - (torch.log(n) + torch.log1p(rest / n))
    lp = torch.cat((lp, torch.full_like(lp[:, :1, :], -70.0)), dim=1)
    return lp.clamp(-70.0, 0.0)


def truncated(z, trunc_r=None, trunc_k=None, dtype=torch.float32):
    """logits z [B, K, L] -> (log_pred, trunc) [B, K+1, L] in dtype"""
    log_pred = predict_start(z, dtype)
    if trunc_k is not None:
        return log_pred, truncate_top_k(log_pred, trunc_k)
    return log_pred, (truncate_top_r(log_pred, trunc_r) if trunc_r is not None else log_pred)


def _decide(post, u, dtype):
    score = -torch.log(-torch.log(u.to(dtype) + 1e-30) + 1e-30) + post
    top2 = score.topk(2, dim=1).values
    return score.argmax(1), top2[:, 0] - top2[:, 1]


def plain_step(sched, z, log_z, t, u, trunc_r=None, trunc_k=None, dtype=torch.float32):
    """One plain tail on logits z [B, K, L], state log_z [B, K+1, L], timesteps t i64[B] and uniforms u [B, K+1, L].
    Returns a dict: log_pred, trunc, post [B, K+1, L] in dtype, tokens i64[B, L] (the first index among equal scores) and
    gap [B, L] (best minus second-best Gumbel score of every decision)."""
    sched = {k: v.to(dtype) for k, v in sched.items()}
    log_pred, trunc = truncated(z, trunc_r, trunc_k, dtype)
    post = O.q_posterior(sched, trunc, log_z.to(dtype), t)
    tokens, gap = _decide(post, u, dtype)
    return dict(log_pred=log_pred, trunc=trunc, post=post, tokens=tokens, gap=gap)


def q_sample_step(sched, x0, t, u, dtype=torch.float32):
    """x_t ~ q(x_t | x_0) for tokens x0 i64[B, L] (the [MASK] id included): the same dict, post = log q(x_t | x_0) and
    log_pred = trunc = the log one-hot of x0"""
    K1 = u.shape[1]
    sched = {k: v.to(dtype) for k, v in sched.items()}
    log_x0 = O.log_onehot(x0, K1).to(dtype)
    post = O._q_pred(sched, log_x0, t, sched["log_at"].numel())
    tokens, gap = _decide(post, u, dtype)
    return dict(log_pred=log_x0, trunc=log_x0, post=post, tokens=tokens, gap=gap)
