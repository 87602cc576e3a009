"""The yardstick of the joint-window tests: the joint tail and the joint reverse chain, restated on the CPU from the oracle's
pieces (oracle/diffsound_oracle.py: predict_start, truncate_top_r / truncate_top_k, q_posterior, gumbel_sample,
transformer_forward, log_onehot, make_schedule) -- never importing the package's sampler or its geometry.

Geometry, restated by enumeration: W windows of G = 53 columns, neighbours sharing n of them (hop h = G - n), on a canvas of
C columns -- line: C = G + (W - 1) h, ring: C = W h, window w covering columns (w h + o) mod C.  A column is covered by one
window or by two; under two, the LATER one is the window that reaches it at the smaller offset o (< n) and its weight is
fade[o] = sin^2(pi (o + 1/2) / (2 n)), built in float64 and rounded to float32 once; the earlier one's is 1 - fade[o].

    l_w = the log_pred window w's row gets from the plain tail -- predict_start(z_w) -- or, with a null condition, from the
          guided tail (tests/guidance_reference.py: guided_log_pred)
    one window:   log_pred = l_w
    two windows:  g = l0 + f (l1 - l0),  g <- g - logsumexp(g)      float64, max-shifted, over the K real classes
                  log_pred = clamp(round(g), -70, 0), [MASK] row -70
    -> truncation, q_posterior, Gumbel-argmax as in the oracle, on the canvas

dtype = float32 is the arithmetic as specified (every predict_start and every mix computed in float64 and rounded to
float32, everything after in float32); dtype = float64 rounds nowhere.  The distance between the two is the rounding error the
specification itself allows, and the tests' tolerances are multiples of it."""
import math

import torch

import diffsound_oracle as O
from guidance_reference import guided_log_pred
from inpaint_reference import chain_steps

R, G = 5, 53
L = R * G


def canvas_cols(W, n, ring):
    h = G - n
    return W * h if ring else G + (W - 1) * h


def fade(n):
    """f32[n], the later window's weight per overlap column"""
    return torch.tensor([math.sin(math.pi * (o + 0.5) / (2.0 * n)) ** 2 for o in range(n)], dtype=torch.float64).float()


def cover(W, n, ring):
    """per canvas column the list of (window, offset) that cover it, by enumerating every window's columns; the later window
    (smaller offset) first"""
    C, h = canvas_cols(W, n, ring), G - n
    cov = [[] for _ in range(C)]
    for w in range(W):
        for o in range(G):
            c = w * h + o
            if ring:
                c %= C
            cov[c].append((w, o))
    for c in range(C):
        assert 1 <= len(cov[c]) <= 2
        cov[c].sort(key=lambda wo: wo[1])
        if len(cov[c]) == 2:
            assert cov[c][0][1] < n and cov[c][1][1] == cov[c][0][1] + h
    return cov


def window_positions(W, n, ring):
    """i64[W, 265]: the canvas position of every token of every window"""
    C, h = canvas_cols(W, n, ring), G - n
    pos = torch.empty(W, L, dtype=torch.long)
    for w in range(W):
        for o in range(G):
            c = (w * h + o) % C if ring else w * h + o
            for r in range(R):
                pos[w, R * o + r] = R * c + r
    return pos


def joint_log_pred(lw, W, n, ring, dtype=torch.float32):
    """lw [B, W, K+1, 265]: every window's own log_pred in dtype -> the canvas's log_pred [B, K+1, R C] in dtype"""
    cov, f = cover(W, n, ring), fade(n)
    B, K1 = lw.shape[0], lw.shape[2]
    C = len(cov)
    l1 = torch.empty(B, K1, R * C, dtype=dtype)
    l0 = torch.empty(B, K1, R * C, dtype=dtype)
    wt = torch.ones(R * C, dtype=torch.float64)
    two = torch.zeros(R * C, dtype=torch.bool)
    for c in range(C):
        (w1, o1) = cov[c][0]
        l1[:, :, R * c:R * c + R] = lw[:, w1, :, R * o1:R * o1 + R]
        if len(cov[c]) == 2:
            (w0, o0) = cov[c][1]
            l0[:, :, R * c:R * c + R] = lw[:, w0, :, R * o0:R * o0 + R]
            wt[R * c:R * c + R] = float(f[o1])
            two[R * c:R * c + R] = True
        else:
            l0[:, :, R * c:R * c + R] = l1[:, :, R * c:R * c + R]
    a, b = l0[:, :-1].double(), l1[:, :-1].double()
    g = a + wt[None, None, :] * (b - a)
    m = g.max(dim=1, keepdim=True).values
    g = (g - m) - torch.log(torch.exp(g - m).sum(dim=1, keepdim=True))
    g = g.to(dtype)
    g = torch.cat((g, torch.full_like(g[:, :1, :], -70.0)), dim=1).clamp(-70.0, 0.0)
    return torch.where(two[None, None, :], g, l1)


def joint_step(sched, zc, zu, s, W, n, ring, log_z, t, u, trunc_r=0.85, trunc_k=None, t_post=None, dtype=torch.float32):
    """One joint tail on given logits zc [B, W, K, 265] (zu likewise, or None: unguided), canvas state log_z [B, K+1, R C],
    t i64[B], uniforms u [B, K+1, R C].  Returns a dict: log_pred, trunc, post [B, K+1, R C], tokens i64[B, R C] and gap."""
    B = zc.shape[0]
    lw = O.predict_start(zc.flatten(0, 1), dtype)
    if zu is not None:
        lw = guided_log_pred(lw, O.predict_start(zu.flatten(0, 1), dtype), s, dtype)
    log_pred = joint_log_pred(lw.view(B, W, *lw.shape[1:]), W, n, ring, dtype)
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


def joint_loop(sd, cond, null, s, W, n, ring, noise_fn, T=100, trunc_r=0.85, skip_step=0, keep=None, known=None, record=None,
               dtype=torch.float32, n_head=16):
    """The joint reverse chain: cond f32[B, 77, 512], null likewise or None (unguided); noise_fn(call index, shape) -> the
    canvas's uniforms.  keep bool[B, R C] / known i64[B, R C]: canvas positions held clean between the calls.  Returns (canvas
    i64[B, R C], the smallest Gumbel gap over all free decisions of the chain); record: the canvas after every call."""
    K = sd["transformer.transformer.to_logits.1.weight"].shape[0]
    B, Lc = cond.shape[0], R * canvas_cols(W, n, ring)
    pos = window_positions(W, n, ring)
    sched = O.make_schedule(T, K + 1)
    if dtype != torch.float32:
        sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        cond, null = cond.to(dtype), (None if null is None else null.to(dtype))
    log_z = O.initial_log_z(B, K + 1, Lc)
    free = torch.ones(B, Lc, dtype=torch.bool)
    if keep is not None:
        log_known = O.log_onehot(known, K + 1)
        log_z = torch.where(keep[:, None, :], log_known, log_z)
        free = ~keep
    cw = cond.repeat_interleave(W, 0)
    nw = None if null is None else null.repeat_interleave(W, 0)
    min_gap = float("inf")
    for k, (st, sp) in enumerate(chain_steps(T, skip_step)):
        t = torch.full((B,), st, dtype=torch.long)
        tw = torch.full((B * W,), st, dtype=torch.long)
        xw = log_z.argmax(1)[:, pos].reshape(B * W, L)
        zc = O.transformer_forward(sd, xw, cw, tw, n_head=n_head).view(B, W, K, L)
        zu = None if nw is None else O.transformer_forward(sd, xw, nw, tw, n_head=n_head).view(B, W, K, L)
        d = joint_step(sched, zc, zu, s, W, n, ring, log_z, t, noise_fn(k, (B, K + 1, Lc)), trunc_r,
                       t_post=torch.full((B,), sp, dtype=torch.long), dtype=dtype)
        min_gap = min(min_gap, float(d["gap"][free].min()))
        log_z = O.log_onehot(d["tokens"], K + 1)
        if keep is not None:
            log_z = torch.where(keep[:, None, :], log_known, log_z)
        if record is not None:
            record.append(log_z.argmax(1).clone())
    return log_z.argmax(1), min_gap
