"""The yardstick of the purity-prior sampling tests: one purity step and the S-step purity chain,
composed on the CPU from the oracle's pieces (oracle/diffsound_oracle.py: predict_start, truncate_top_r / truncate_top_k,
transformer_forward, log_onehot, make_schedule) and guidance_reference.guided_log_pred -- never importing the package's
sampler, plan included (plan() below restates the rule on its own).

    lp   = predict_start(z)                     (+ the guided mix with predict_start(zu) when zu is given)
    tr   = truncation of lp                     dropped classes at -70
    lmax = max_c lp[c]                          before truncation: the log of the purity
    sh   = tr                                   weight r == 0
         = a tr - logsumexp(a tr), a = 1 + r exp(lmax)      r > 0; float64, max-shifted, over the K real classes
    cand = argmax_c sh[c] + G(u_c)              over the K real classes, G(u) = -log(-log(u + 1e-30) + 1e-30)
    key  = lmax + G(u_K) where x == K           u_K: the [MASK] slot's uniform
    per sample: m masked positions, n = max(0, m - R): the n largest keys (equal keys: smaller position first) take cand

dtype = float32 is the arithmetic as specified (predict_start, the mix and the sharpening computed in float64 and rounded to
float32, a and the Gumbel scores in float32); dtype = float64 rounds nowhere.  The distance between the two is the rounding
error the specification itself allows, and the tests' tolerances and margins are multiples of it."""
import numpy as np
import torch

import diffsound_oracle as O
from guidance_reference import guided_log_pred

L = 265
INF = float("inf")


def plan(S, n_pos, log_cumprod_ct):
    """[(t_k, R_k)]: R_k = floor((S-1-k) n_pos / S); t_k = the t in 0 .. T-1 whose exp(log_cumprod_ct[t]) is nearest to
    R_{k-1} / n_pos (R_{-1} = n_pos; ties to the larger t), forced non-increasing, t_0 = T - 1.  log_cumprod_ct has T + 1
    entries (the last is the wrap-around slot)."""
    g = np.exp(np.asarray(log_cumprod_ct, dtype=np.float64))[:-1]
    T = len(g)
    out, prev_r = [], n_pos
    for k in range(S):
        share = prev_r / n_pos
        best = min(abs(float(x) - share) for x in g)
        t = max(i for i in range(T) if abs(float(g[i]) - share) == best)
        if k == 0:
            t = T - 1
        else:
            t = min(t, out[-1][0])
        prev_r = ((S - 1 - k) * n_pos) // S
        out.append((t, prev_r))
    return out


def gumbel(u):
    return -torch.log(-torch.log(u + 1e-30) + 1e-30)


def purity_step(x, z, u, remain, weight, trunc_r=0.85, trunc_k=None, zu=None, scale=None, dtype=torch.float32):
    """One purity step.  x i64[B, n]; z (and zu) logits [B, K, n]; u uniforms [B, K+1, n]; remain R; weight r.  Returns a dict:
    log_pred (lp) and sharp [B, K+1, n] ([MASK] row -70), score [B, K, n] (sh + G), cand i64[B, n], cand_gap [B, n] (best minus second-best
    score), key [B, n] (-inf off [MASK]), reveal bool[B, n], tokens i64[B, n], sel_gap [B] (the n-th minus the (n+1)-th largest
    key of the sample; inf when nothing or everything masked is revealed)."""
    B, K, n_pos = z.shape
    lp = O.predict_start(z, dtype)
    if zu is not None:
        lp = guided_log_pred(lp, O.predict_start(zu, dtype), scale, dtype)
    if trunc_k is not None:
        tr = O.truncate_top_k(lp, trunc_k)
    else:
        tr = O.truncate_top_r(lp, trunc_r) if trunc_r is not None else lp
    lmax = lp[:, :-1].max(dim=1).values
    if weight == 0:
        sh = tr
    else:
        if dtype == torch.float32:
            a = (1.0 + torch.tensor(weight, dtype=torch.float32) * torch.exp(lmax)).double()
        else:
            a = 1.0 + float(weight) * torch.exp(lmax.double())
        av = a[:, None, :] * tr[:, :-1].double()
        m = av.max(dim=1, keepdim=True).values
        s = ((av - m) - torch.log(torch.exp(av - m).sum(dim=1, keepdim=True))).to(dtype).clamp(-70.0, 0.0)
        sh = torch.cat((s, torch.full_like(s[:, :1, :], -70.0)), dim=1)
    g = gumbel(u.to(dtype))
    score = sh[:, :-1] + g[:, :-1]
    top2 = score.topk(2, dim=1).values
    cand = score.argmax(1)
    mask = x == K
    key = torch.where(mask, lmax + g[:, K], torch.full_like(lmax, -INF))
    order = torch.sort(key, dim=1, descending=True, stable=True).indices       # equal keys: the smaller position first
    reveal = torch.zeros(B, n_pos, dtype=torch.bool)
    sel_gap = torch.full((B,), INF, dtype=torch.float64)
    for b in range(B):
        m_b = int(mask[b].sum())
        n_b = max(0, m_b - int(remain))
        reveal[b, order[b, :n_b]] = True
        if 0 < n_b < m_b:
            sel_gap[b] = float(key[b, order[b, n_b - 1]]) - float(key[b, order[b, n_b]])
    tokens = torch.where(reveal, cand, x)
    return dict(log_pred=lp, sharp=sh, score=score, cand=cand, cand_gap=top2[:, 0] - top2[:, 1], key=key, reveal=reveal, tokens=tokens,
                sel_gap=sel_gap)


def purity_loop(sd, cond, S, weight, noise_fn, T=100, trunc_r=0.85, null=None, scale=None, keep=None, known=None, record=None,
                dtype=torch.float32, n_head=16):
    """The S-step purity chain: cond (and null, for guidance) f32[B, 77, 512]; noise_fn(call index, shape) -> uniforms.
    keep bool[B, L] / known i64[B, L]: held positions enter as their known tokens.  Returns (tokens i64[B, L], the smallest
    candidate gap over all revealed decisions, the smallest selection gap); record: the tokens after every call."""
    K = sd["transformer.transformer.to_logits.1.weight"].shape[0]
    B = cond.shape[0]
    sched = O.make_schedule(T, K + 1)
    if dtype != torch.float32:
        sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        cond = cond.to(dtype)
        null = None if null is None else null.to(dtype)
    x = torch.full((B, L), K, dtype=torch.long)
    if keep is not None:
        x = torch.where(keep, known, x)
    cand_gap, sel_gap = INF, INF
    for k, (t_k, r_k) in enumerate(plan(S, L, sched["log_cumprod_ct"].numpy())):
        t = torch.full((B,), t_k, dtype=torch.long)
        z = O.transformer_forward(sd, x, cond, t, n_head=n_head)
        zu = None if null is None else O.transformer_forward(sd, x, null, t, n_head=n_head)
        d = purity_step(x, z, noise_fn(k, (B, K + 1, L)), r_k, weight, trunc_r=trunc_r, zu=zu, scale=scale, dtype=dtype)
        if bool(d["reveal"].any()):
            cand_gap = min(cand_gap, float(d["cand_gap"][d["reveal"]].min()))
        sel_gap = min(sel_gap, float(d["sel_gap"].min()))
        x = d["tokens"]
        if record is not None:
            record.append(x.clone())
    return x, cand_gap, sel_gap
