"""Inputs of the purity-prior sampling tests, shared by tests/test_purity_host.py (which asserts the facts that make them fair
inputs) and tests/test_hip_purity.py (which runs the kernels on them), with the yardstick's results computed once per
process (tests/purity_reference.py)."""
import functools

import torch

import purity_reference as R
from conftest import synth_sd
from text_to_sound_synthesis_amd import shard, synth

B = 3
TRUNC_R, TRUNC_K, GUIDE_SCALE = 0.85, 10, 3.0
LOGITS = ("flat", "ordinary", "dominant")       # near-flat, ordinary, one class dominant
TRUNCS = ("r", "k", "none")
# (K, L, logits, truncation, weight r, guided): the full cross at L = 265, and the smallest grid (one column, L = 5) under top-r
TAIL_CASES = [(K, 265, lg, tr, w, gd) for K in (256, 512) for lg in LOGITS for tr in TRUNCS for w in (0.0, 1.0)
              for gd in (False, True)] + \
             [(K, 5, lg, "r", 1.0, gd) for K in (256, 512) for lg in LOGITS for gd in (False, True)]
# generator seeds of the cases whose default seed (tail_seed) does not give a fair input: chosen so that the float32 and float64
# restatements alone stay inside the tests' caps (asserted by test_purity_host.py)
TAIL_SEEDS = {(512, 265, "flat", "r", 0.0, False): 9001, (512, 265, "flat", "k", 1.0, False): 9103}
# a decision of the float64 yardstick counts only if its gap exceeds MARGIN_MULT x the measured float32-float64 distance of the
# quantity it compares: the device's libm may be as far from the host's float32 as that is from float64, so a score may be off
# by twice the distance and a gap -- a difference of two scores -- by four times
MARGIN_MULT = 4.0
TOL_MULT = 4.0                                   # dbg_sharp against the float64 yardstick, in units of the same distance


def case_id(c):
    K, n_pos, lg, tr, w, gd = c
    return "K%d-L%d-%s-top%s-r%g-%s" % (K, n_pos, lg, tr, w, "guided" if gd else "plain")


def tail_seed(c):
    return TAIL_SEEDS.get(c, 7000 + TAIL_CASES.index(c))


def tail_state(K, n_pos, g):
    """x i64[3, n_pos]: sample 0 all [MASK], sample 1 about half, sample 2 few -- and the target R between the counts of the
    last two, so that one step reveals from samples 0 and 1 and leaves sample 2 (m <= R) alone"""
    x = torch.randint(0, K, (B, n_pos), generator=g)
    x[0] = K
    if n_pos == 5:
        x[1, 0::2] = K
        x[2, 4] = K
        return x, 1
    x[1][torch.rand(n_pos, generator=g) < 0.5] = K
    x[2][torch.rand(n_pos, generator=g) < 0.08] = K
    m1, m2 = int((x[1] == K).sum()), int((x[2] == K).sum())
    assert m2 < m1 // 2
    return x, m1 // 2


def tail_logits(K, n_pos, kind, g):
    if kind == "flat":
        return torch.randn(B, K, n_pos, generator=g) * 0.05
    z = torch.randn(B, K, n_pos, generator=g) * 4.0
    if kind == "dominant":
        top = torch.randint(0, K, (B, 1, n_pos), generator=g)
        z.scatter_add_(1, top, torch.full((B, 1, n_pos), 25.0))
    return z


@functools.lru_cache(maxsize=None)
def tail_case(c):
    """Inputs (x, R, z, zu or None, u) of a TAIL_CASES entry and the yardstick's float32 / float64 restatements (ref32, ref64:
    purity_step's dicts)."""
    K, n_pos, kind, trunc, weight, guided = c
    g = torch.Generator().manual_seed(tail_seed(c))
    z = tail_logits(K, n_pos, kind, g)
    zu = z + torch.randn(B, K, n_pos, generator=g) if guided else None
    x, remain = tail_state(K, n_pos, g)
    u = torch.rand(B, K + 1, n_pos, generator=g)
    kw = dict(trunc_r=TRUNC_R if trunc == "r" else None, trunc_k=TRUNC_K if trunc == "k" else None, zu=zu,
              scale=GUIDE_SCALE if guided else None)
    ref32 = R.purity_step(x, z, u, remain, weight, dtype=torch.float32, **kw)
    ref64 = R.purity_step(x, z, u, remain, weight, dtype=torch.float64, **kw)
    return dict(K=K, L=n_pos, x=x, remain=remain, z=z, zu=zu, u=u, weight=weight, trunc_r=TRUNC_R if trunc == "r" else -1.0,
                trunc_k=TRUNC_K if trunc == "k" else 0, scale=GUIDE_SCALE, ref32=ref32, ref64=ref64)


def tail_margins(c):
    """(d_sharp, cand margin, selection margin, excluded candidate draws bool[B, L], excluded selections bool[B]) of a case:
    the measured float32-float64 distances of the yardstick and the decisions its float64 form takes by less than the margin"""
    d = tail_case(c)
    r32, r64 = d["ref32"], d["ref64"]
    d_sharp = float((r32["sharp"].double() - r64["sharp"]).abs().max())
    d_score = float((r32["score"].double() - r64["score"]).abs().max())
    fin = torch.isfinite(r64["key"])
    d_key = float((r32["key"].double() - r64["key"])[fin].abs().max()) if bool(fin.any()) else 0.0
    cand_margin, sel_margin = MARGIN_MULT * d_score, MARGIN_MULT * d_key
    return d_sharp, cand_margin, sel_margin, r64["cand_gap"] <= cand_margin, r64["sel_gap"] <= sel_margin


# ---- chains: the 2-layer T = 10 model of the small-model tests -----------------------------------------------------------------
T_CHAIN = 10
CHAIN_SEED = (0x5eed << 32) | 20261019
CHAIN_MIN_GAP = 1e-3        # a chain is a fair input if the yardstick takes every decision of it by at least this much: the
                            # bound the guided-chain tests use for a denoiser whose logits agree with the oracle's to ~1e-4
# ids: the captions' global ids = the Philox streams the chain draws from, chosen for CHAIN_MIN_GAP (test_purity_host.py)
CHAINS = {
    "s4": dict(S=4, weight=1.0, held=False, guided=False, ids=(211, 212)),
    "s10": dict(S=10, weight=0.0, held=False, guided=False, ids=(21, 22)),
    "s4_held": dict(S=4, weight=1.0, held=True, guided=False, ids=(31, 32)),
    "s10_guided": dict(S=10, weight=1.0, held=False, guided=True, ids=(241, 242)),
    "s4_guided_held": dict(S=4, weight=0.0, held=True, guided=True, ids=(51, 52)),
    "s10_b1": dict(S=10, weight=1.0, held=False, guided=False, ids=(361,)),
    "s4_b1_guided": dict(S=4, weight=0.0, held=False, guided=True, ids=(171,)),
}


def chain_sd():
    sd = dict(synth_sd("dalle", 2))
    return {k: (v[:T_CHAIN] if k.endswith(("ln1.emb.weight", "ln1_1.emb.weight")) else v) for k, v in sd.items()}


def chain_inputs(name):
    """cond, null f32[B, 77, 512] (one null embedding, broadcast), known i64[B, L], keep bool[B, L] (a held middle span)"""
    n = len(CHAINS[name]["ids"])
    cond = synth.synth_cond_emb(2, key="purity.cond")[:n].contiguous()
    null = synth.synth_cond_emb(1, key="purity.null").expand(n, -1, -1).contiguous()
    known = synth.synth_tokens(2, mask_frac=0.0, key="purity.known")[:n].contiguous()
    keep = torch.zeros(2, 53, dtype=torch.bool)
    keep[0, 8:45] = True
    keep[1, 10:30] = True
    return cond, null, known, keep[:n, :, None].expand(n, 53, 5).reshape(n, R.L).contiguous()


def chain_noise(name, K=256):
    ids = CHAINS[name]["ids"]
    return lambda k, shp: shard.caption_uniforms(ids, k, K, R.L, CHAIN_SEED)


@functools.lru_cache(maxsize=None)
def chain_reference(name, dtype=torch.float32):
    """(tokens after every call [S, B, L], smallest candidate gap, smallest selection gap) of the yardstick's purity_loop"""
    c = CHAINS[name]
    cond, null, known, keep = chain_inputs(name)
    rec = []
    _, cg, sg = R.purity_loop(chain_sd(), cond, c["S"], c["weight"], chain_noise(name), T=T_CHAIN, trunc_r=TRUNC_R,
                              null=null if c["guided"] else None, scale=GUIDE_SCALE if c["guided"] else None,
                              keep=keep if c["held"] else None, known=known if c["held"] else None, record=rec, dtype=dtype)
    return torch.stack(rec), cg, sg
