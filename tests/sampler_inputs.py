"""Inputs of the sampling-tail edge tests, shared by tests/test_sampler_host.py (which asserts that they are fair: the
yardstick alone meets what the GPU test demands of the kernel) and tests/test_hip_sampler_edges.py (which runs the kernels
on them).  Everything comes from torch.Generator seeds; the yardstick's float32 and float64 results
(tests/sampler_reference.py) are computed once per process and never modified.

Shapes: L = 37 with B = 2 and 3 (74 and 111 columns: 2 and 1 dead waves in the last workgroup of 4), (B, L) = (1, 1), (5, 1)
and (1, 3) (3, 3 and 1 dead waves), K = 256 and 512 (both NPL instantiations), T = 100 and one case at T = 10."""
import collections
import functools

import numpy as np
import torch

import diffsound_oracle as O
import sampler_reference as R

FAMILIES = ("normal4", "spread40", "flat", "const", "tied_half", "onehot", "two_level", "asc", "desc", "neg_inf")
FULL_RANGE = ("normal4", "const", "tied_half", "onehot")             # the families every r and every k run on
RATES = (0.0, 1e-6, 0.5, 0.85, 0.999, 1.0)
T_POOL = (0, 1, 50, 98, 99)
EDGE_U = (1.0 - 2.0 ** -24, 1.0 - 2.0 ** -12, 2.0 ** -24, 0.0)
NEAR_CUT = 4e-7                 # a kept set may differ only where the cut sits this close to r (tests/test_hip_guidance.py)
# generator seeds per case id, where the default (derived from the id) breaks a cap of test_sampler_host.py or puts a
# cut within NEAR_CUT of r that another seed avoids (chosen on the yardstick alone: its float32 and float64 forms)
# normal4 at r = 1.0: the float32 running mass rounds to float32(1.0) once less than 2^-25 of it is left and the classes
# ranked after that point are dropped, which float64 keeps: on Gaussian logits the two yardsticks differ in 62 of 74
# columns whatever the seed.  The case runs on three columns, one seed each (a tuple), in which the
# float32 mass before the last class stays >= 8e-8 below that point, so that both keep all K classes.
SEEDS = {"normal4-K256-B1L3-r1": (14419, 17787, 9937), "normal4-K512-B1L3-r1": (9848, 7191, 18077),
         "tied_half-K256-B3L37-r0.999": 8, "tied_half-K256-B2L37-r1": 11, "flat-K512-B2L37-r0.85": 1,
         "normal4-K512-B3L37-r0.999": 5, "tied_half-K512-B3L37-r0.999": 2, "tied_half-K512-B2L37-r1": 3}

Case = collections.namedtuple("Case", "id family K B L T trunc_r trunc_k xt_kind u_kind t")


def _cases():
    out, n_fam = [], collections.Counter()

    def add(family, K, B, L, trunc, xt_kind="random", u_kind="random", T=100, t=None, tag=""):
        r, k = (trunc[1], None) if trunc and trunc[0] == "r" else (None, trunc[1] if trunc else None)
        if t is None:       # per sample, different within a batch; the offset walks with the family's case count
            n = n_fam[family]
            n_fam[family] += 1
            pool = T_POOL if T == 100 else (0, 1, T // 2, T - 2, T - 1)
            t = tuple(pool[(n + 2 * b) % 5] for b in range(B))
        name = "%s-K%d-B%dL%d-%s%s" % (family, K, B, L, "none" if not trunc else "%s%g" % trunc, tag)
        out.append(Case(name, family, K, B, L, T, r, k, xt_kind, u_kind, t))

    for K in (256, 512):
        for i, f in enumerate(FAMILIES):                             # every family at r = 0.85, no truncation and k = 30
            for j, trunc in enumerate((("r", 0.85), None, ("k", 30))):
                add(f, K, 2 + (i + j) % 2, 37, trunc)
        for i, f in enumerate(FULL_RANGE):                           # every r and every k
            for j, trunc in enumerate([("r", r) for r in RATES if r != 0.85] + [("k", 1), ("k", K)]):
                if (f, trunc) == ("normal4", ("r", 1.0)):            # three chosen columns: see SEEDS
                    add(f, K, 1, 3, trunc)
                else:
                    add(f, K, 2 + (i + j) % 2, 37, trunc)
        for B, L in ((1, 1), (5, 1), (1, 3)):                        # the ragged grids: 1, 5 and 3 columns
            for f, trunc in (("normal4", ("r", 0.85)), ("tied_half", ("k", 30)), ("spread40", None)):
                add(f, K, B, L, trunc)
        add("normal4", K, 2, 37, ("r", 0.85), xt_kind="all_mask", tag="-allmask")       # initial = 1
        add("tied_half", K, 3, 37, ("k", 30), xt_kind="all_mask", tag="-allmask")
        add("normal4", K, 3, 37, ("r", 0.85), xt_kind="no_mask", tag="-nomask")
        add("spread40", K, 2, 37, None, xt_kind="no_mask", tag="-nomask")
        for f, trunc in (("normal4", None), ("normal4", ("r", 0.85)), ("spread40", ("r", 0.85)), ("spread40", None),
                         ("onehot", ("r", 0.85)), ("onehot", ("k", 30)), ("neg_inf", None), ("tied_half", ("k", 30))):
            add(f, K, 3, 37, trunc, u_kind="edge", tag="-edge")
        add("normal4", K, 5, 1, ("r", 0.85), u_kind="edge", tag="-edge")
        # every kept class scores the same: all-[MASK] x_t, one shared t at which [MASK] is not the likeliest successor
        for f, t in (("const", 1), ("two_level", 0)):
            for trunc in (("r", 0.85), None, ("k", 100 if f == "const" else 30)):   # (k = 100: the tie spans two j slots)
                add(f, K, 2, 37, trunc, xt_kind="all_mask", u_kind="const_u", t=(t, t), tag="-constu")
    add("normal4", 256, 3, 37, ("r", 0.85), T=10, tag="-T10")        # tm1 wraps to T at t = 0 whatever T is; a second T
    add("tied_half", 512, 2, 37, ("k", 30), T=10, tag="-T10")
    return out


CASES = _cases()
CASE_IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def _seed(cid):
    return SEEDS.get(cid, sum((i + 1) * ord(ch) for i, ch in enumerate(cid)) % 100003)


def logits(family, B, K, L, g):
    """one of the logit families, [B, K, L]"""
    n = lambda: torch.randn(B, K, L, generator=g)
    if family == "normal4":
        return n() * 4
    if family == "spread40":
        return n() * 40
    if family == "flat":
        return n() * 0.01
    if family == "const":
        return torch.zeros(B, K, L)
    if family == "tied_half":
        return (n() * 4).round() / 2
    if family == "onehot":
        hot = torch.randint(0, K, (B, 1, L), generator=g)
        return torch.full((B, K, L), -100.0).scatter(1, hot, 50.0)
    if family == "two_level":
        # about 3 % of the classes at 6.0; the last of them is moved 64 above the first, so that two of the tying classes
        # always share a lane (class = 64 j + lane) in different j slots
        m = max(2, round(0.03 * K))
        order = torch.rand(B, K, L, generator=g).argsort(1)[:, :m, :]
        order[:, m - 1, :] = (order[:, 0, :] + 64) % K
        return torch.zeros(B, K, L).scatter(1, order, 6.0)
    if family in ("asc", "desc"):
        ramp = 0.05 * torch.arange(K, dtype=torch.float32).view(1, K, 1).expand(B, K, L)
        return (ramp if family == "asc" else -ramp).contiguous()
    if family == "neg_inf":
        z = n() * 4
        masked = torch.rand(B, K, L, generator=g).argsort(1) < K // 4      # a quarter of every column, never a whole one
        return z.masked_fill(masked, float("-inf"))
    raise ValueError(family)


def kept(trunc):
    """the kept set of a truncated prediction: bool[B, K, L] over the real classes"""
    return trunc[:, :-1] > -70.0


def edge_uniforms(c, log_pred64, trunc64):
    """u = 0.5 everywhere but four classes per column.  Column n gives EDGE_U[n % 4] to its likeliest class and the three
    other values to its least likely kept classes (where fewer than four are kept, to the least likely classes of all), so
    that over the columns every edge value is the one the winner holds."""
    B, K, L = c.B, c.K, c.L
    u = torch.full((B, K + 1, L), 0.5)
    order = torch.sort(log_pred64[:, :-1], dim=1, descending=True, stable=True)[1]          # [B, K, L]
    n_keep = kept(trunc64).sum(1)                                                            # [B, L]
    for b in range(B):
        for pos in range(L):
            col, m = b * L + pos, max(int(n_keep[b, pos]), 1)
            others = [int(order[b, m - 1 - i, pos]) for i in range(3)] if m >= 4 else \
                     [int(order[b, i, pos]) for i in range(1, m)] + [int(order[b, K - 1 - i, pos]) for i in range(4 - m)]
            vals = [EDGE_U[(col + 1 + i) % 4] for i in range(3)]
            u[b, int(order[b, 0, pos]), pos] = EDGE_U[col % 4]
            for cls, v in zip(others, vals):
                u[b, cls, pos] = v
    return u


@functools.lru_cache(maxsize=None)
def schedule(T, K):
    return O.make_schedule(T, K + 1)


def compare(r32, r64, trunc_r):
    """the float32 yardstick against the float64 one: same [B, L] (columns whose kept sets agree), near [B, L] (columns
    with a cut within NEAR_CUT of r), d32 (the largest posterior distance over the agreeing columns) and thr (the Gumbel
    gap from which a token must agree: 2 (4 d32 + 1e-6 + 4e-6); 4e-6 = 2 ulp of the largest Gumbel term, 16.6)"""
    same = (kept(r32["trunc"]) == kept(r64["trunc"])).all(1)
    if trunc_r is None:
        near = torch.zeros_like(same)
    else:
        # rank i >= 1 of the K real classes looks at the mass of ranks 0 .. i-1: K - 1 partial sums decide a column
        inc = torch.exp(torch.sort(r64["log_pred"][:, :-1], dim=1, descending=True, stable=True)[0]).cumsum(1)[:, :-1]
        near = ((inc - float(np.float32(trunc_r))).abs() < NEAR_CUT).any(1)
    sel = same[:, None, :].expand_as(r64["post"])
    d32 = float((r32["post"].double() - r64["post"])[sel].abs().max()) if bool(same.any()) else 0.0
    return same, near, d32, 2 * (4 * d32 + 1e-6 + 4e-6)


@functools.lru_cache(maxsize=None)
def case(cid):
    """the inputs of a case (z [B, K, L]; xt i64[B, L]; t i64[B]; u [B, K+1, L]; initial; log_z) and the yardstick's
    results: ref32, ref64 (plain_step's dicts), same, near, d32, thr (compare above)"""
    c = BY_ID[cid]
    B, K, L = c.B, c.K, c.L
    seed, z = _seed(cid), None
    if isinstance(seed, tuple):             # one seed per column
        z = torch.cat([logits(c.family, B, K, 1, torch.Generator().manual_seed(s)) for s in seed], dim=2)
        seed = seed[0]
    g = torch.Generator().manual_seed(seed)
    if z is None:
        z = logits(c.family, B, K, L, g)
    initial = 0
    if c.xt_kind == "all_mask":
        xt = torch.full((B, L), K, dtype=torch.long)
        initial = int(c.u_kind != "const_u" or c.trunc_k is None)       # both forms of the all-[MASK] state occur
    else:
        xt = torch.randint(0, K + (c.xt_kind == "random"), (B, L), generator=g)
    log_z = O.initial_log_z(B, K + 1, L) if initial else O.log_onehot(xt, K + 1)
    t = torch.tensor(c.t, dtype=torch.long)
    sched = schedule(c.T, K)
    if c.u_kind == "random":
        u = torch.rand(B, K + 1, L, generator=g)
    elif c.u_kind == "const_u":
        u = torch.full((B, K + 1, L), 0.5)
    else:
        u = edge_uniforms(c, *R.truncated(z, c.trunc_r, c.trunc_k, torch.float64))
    kw = dict(trunc_r=c.trunc_r, trunc_k=c.trunc_k)
    r32 = R.plain_step(sched, z, log_z, t, u, dtype=torch.float32, **kw)
    r64 = R.plain_step(sched, z, log_z, t, u, dtype=torch.float64, **kw)
    same, near, d32, thr = compare(r32, r64, c.trunc_r)
    return dict(c=c, z=z, xt=xt, t=t, u=u, initial=initial, log_z=log_z, sched=sched, ref32=r32, ref64=r64, same=same,
                near=near, d32=d32, thr=thr)


def tying_classes(d):
    """const_u cases: per column the classes that hold the float32 yardstick's best score -> bool[B, K+1, L]"""
    r = d["ref32"]
    score = -torch.log(-torch.log(d["u"] + 1e-30) + 1e-30) + r["post"]
    return score == score.max(1, keepdim=True).values


# ---- q_sample ---------------------------------------------------------------------------------------------------------------
QCase = collections.namedtuple("QCase", "id K B L u_kind t")
Q_CASES = [QCase("q-K%d-B%dL%d-%s" % (K, B, L, uk), K, B, L, uk, tuple((0, 1, 50, 99, 1)[(i + b) % 5] for b in range(B)))
           for K in (256, 512) for i, (B, L) in enumerate(((1, 1), (5, 1), (3, 37))) for uk in ("random", "edge")]
Q_IDS = [c.id for c in Q_CASES]
Q_BY_ID = {c.id: c for c in Q_CASES}


@functools.lru_cache(maxsize=None)
def q_case(cid):
    """x0 i64[B, L] (the [MASK] id included), t i64[B], u and the yardstick's q_sample_step in both dtypes.  The edge
    uniforms: column n gives EDGE_U[(n + i) % 4] to x0's class, [MASK] and two other classes (i = 0 .. 3)."""
    c = Q_BY_ID[cid]
    B, K, L = c.B, c.K, c.L
    g = torch.Generator().manual_seed(_seed(cid))
    x0 = torch.randint(0, K + 1, (B, L), generator=g)
    x0[0, 0] = K
    if B * L > 1:
        x0[-1, -1] = 3
    t = torch.tensor(c.t, dtype=torch.long)
    if c.u_kind == "random":
        u = torch.rand(B, K + 1, L, generator=g)
    else:
        u = torch.full((B, K + 1, L), 0.5)
        extra = torch.randint(1, K - 1, (B, L, 2), generator=g)
        for b in range(B):
            for pos in range(L):
                x, col = int(x0[b, pos]), b * L + pos
                cls = [x, K if x != K else 0] + [int((x + e) % K) if x != K else int(e) for e in extra[b, pos]]
                if cls[2] == cls[3]:
                    cls[3] = (cls[3] + 1) % K if (cls[3] + 1) % K != x else (cls[3] + 2) % K
                for i, k in enumerate(cls):
                    u[b, k, pos] = EDGE_U[(col + i) % 4]
    sched = schedule(100, K)
    r32 = R.q_sample_step(sched, x0, t, u, torch.float32)
    r64 = R.q_sample_step(sched, x0, t, u, torch.float64)
    d32 = float((r32["post"].double() - r64["post"]).abs().max())
    return dict(c=c, x0=x0, t=t, u=u, sched=sched, ref32=r32, ref64=r64, d32=d32, thr=2 * (4 * d32 + 1e-6 + 4e-6))


# ---- the frequency test through the in-kernel noise -----------------------------------------------------------------------
FREQ = dict(K=256, B=16, L=265, T=100, calls=(0, 1, 2, 3), seed=(0x51ed << 32) | 20261018, trunc_r=0.85, t=2, q_t=50, q_x0=17,
            ids=(0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 100000, 2 ** 31 + 7, 2 ** 32 - 1))
CHI2_TAIL = 1e-9


def freq_row():
    """the logits row every column of the frequency test carries: eight classes hold 0.22 .. 0.05 of the mass (top-r 0.85
    keeps seven of them), the other 248 share 0.05; x_t = [MASK] at t = 2, where staying [MASK] has probability ~ 1/2"""
    K = FREQ["K"]
    p = torch.full((K,), 0.05 / (K - 8), dtype=torch.float64)
    p[torch.tensor([3, 40, 64, 65, 129, 200, 254, 255])] = torch.tensor([0.22, 0.18, 0.14, 0.12, 0.10, 0.08, 0.06, 0.05], dtype=torch.float64)
    return torch.log(p).float()


@functools.lru_cache(maxsize=None)
def freq_tail():
    """(z [1, K, 1], xt, t, the yardstick's float32 post [K+1], its float64 class probabilities exp(post64) / sum [K+1]).
    Gumbel-argmax draws class c with probability exp(post[c]) / sum exp(post): the truncated posterior is not renormalised."""
    K = FREQ["K"]
    z = freq_row().view(1, K, 1)
    xt = torch.full((1, 1), K, dtype=torch.long)
    t = torch.tensor([FREQ["t"]])
    u = torch.full((1, K + 1, 1), 0.5)
    sched = schedule(FREQ["T"], K)
    kw = dict(trunc_r=FREQ["trunc_r"])
    r32 = R.plain_step(sched, z, O.log_onehot(xt, K + 1), t, u, dtype=torch.float32, **kw)
    r64 = R.plain_step(sched, z, O.log_onehot(xt, K + 1), t, u, dtype=torch.float64, **kw)
    p = torch.exp(r64["post"][0, :, 0])
    return z, xt, t, r32["post"][0, :, 0], p / p.sum()


@functools.lru_cache(maxsize=None)
def freq_q():
    """q_sample at t = 50 of x0 = 17: (float32 log q [K+1], float64 probabilities of the three cells: stay, [MASK], other)"""
    K = FREQ["K"]
    x0 = torch.full((1, 1), FREQ["q_x0"], dtype=torch.long)
    t = torch.tensor([FREQ["q_t"]])
    u = torch.full((1, K + 1, 1), 0.5)
    sched = schedule(FREQ["T"], K)
    lq32 = R.q_sample_step(sched, x0, t, u, torch.float32)["post"][0, :, 0]
    p = torch.exp(R.q_sample_step(sched, x0, t, u, torch.float64)["post"][0, :, 0])
    p = p / p.sum()
    stay, mask = p[FREQ["q_x0"]], p[K]
    return lq32, torch.stack((stay, mask, 1.0 - stay - mask))


def pearson(counts, prob, min_expected=20.0):
    """counts i64[n], prob f64[n] -> (Pearson's statistic, cells): classes whose expected count is below min_expected are
    pooled into one cell, and that cell joins the smallest other one if it is still below it"""
    N = float(counts.sum())
    exp = prob.double() * N
    big = exp >= min_expected
    o, e = counts[big].double().tolist(), exp[big].tolist()
    po, pe = float(counts[~big].sum()), float(exp[~big].sum())
    if pe >= min_expected:
        o.append(po)
        e.append(pe)
    elif (~big).any():
        i = e.index(min(e))
        o[i] += po
        e[i] += pe
    return sum((a - b) ** 2 / b for a, b in zip(o, e)), len(e)


def chi2_threshold(cells):
    from scipy.stats import chi2
    return float(chi2.isf(CHI2_TAIL, cells - 1))


def host_tokens(log_prob32, rng_stream):
    """the float32 yardstick's tokens for all B x calls x L columns of the frequency test, fed the host mirror of the
    in-kernel Philox stream: i64[calls, B, L]"""
    from text_to_sound_synthesis_amd import shard
    out = []
    for call in FREQ["calls"]:
        u = shard.caption_uniforms(FREQ["ids"], call, FREQ["K"], FREQ["L"], FREQ["seed"], rng_stream=rng_stream)
        out.append((-torch.log(-torch.log(u + 1e-30) + 1e-30) + log_prob32.view(1, -1, 1)).argmax(1))
    return torch.stack(out)
