"""Inputs of the joint-window tests, shared by tests/test_joint_host.py (which asserts the facts that make them fair inputs)
and tests/test_hip_joint.py (which runs the kernels on them), with the yardstick's results computed once per process
(tests/joint_reference.py)."""
import functools

import torch

import diffsound_oracle as O
import joint_reference as R
from conftest import synth_sd
from text_to_sound_synthesis_amd import synth

L, T_TAIL, T_CHAIN = 265, 100, 10
TRUNC_R, TRUNC_K = 0.85, 30
SCALE = 3.0                       # the guidance scale of the guided cases
B_TAIL, W_TAIL = 2, 3             # 2 clips of 3 windows; the canvas lengths (665 .. 785, 405 .. 780) leave ragged last workgroups
OVERLAPS = (1, 13, 26)
# every tail case: (K, n, ring, trunc_k, guided)
TAIL_CASES = [(K, n, ring, tk, gd) for K in (256, 512) for n in OVERLAPS for ring in (False, True) for tk in (None, TRUNC_K)
              for gd in (False, True)]
# generator seeds of the tail inputs per case: chosen so that the float32 and float64 restatements agree in every kept set
# outside cuts within 4e-7 of r and in every token there (asserted by test_joint_host.py); default below
TAIL_SEEDS = {}


def tail_seed(K, n, ring, trunc_k, guided):
    return TAIL_SEEDS.get((K, n, ring, trunc_k, guided), 7000 + 100 * n + 10 * int(ring) + 2 * int(bool(trunc_k)) + int(guided) + K)


@functools.lru_cache(maxsize=None)
def tail_case(K, n, ring, trunc_k=None, guided=False):
    """Inputs (zc, zu: [B, W, K, 265] window logits, zu None unguided; canvas xt i64[B, Lc], t i64[B] -- a timestep per clip --,
    u [B, K+1, Lc]) and the yardstick's float32 and float64 restatements (ref32, ref64: joint_step's dicts)."""
    B, W = B_TAIL, W_TAIL
    Lc = R.R * R.canvas_cols(W, n, ring)
    g = torch.Generator().manual_seed(tail_seed(K, n, ring, trunc_k, guided))
    z0 = torch.randn(B, 1, K, L, generator=g) * 4.0
    zc = z0 + torch.randn(B, W, K, L, generator=g)
    zu = z0 + torch.randn(B, W, K, L, generator=g) if guided else None
    xt = torch.randint(0, K + 1, (B, Lc), generator=g)
    xt[:, ::7] = K                                   # [MASK] and revealed positions side by side, under one window and under two
    u = torch.rand(B, K + 1, Lc, generator=g)
    t = torch.tensor([60, 30][:B], dtype=torch.long)
    sched = O.make_schedule(T_TAIL, K + 1)
    log_z = O.log_onehot(xt, K + 1)
    kw = dict(trunc_r=None if trunc_k else TRUNC_R, trunc_k=trunc_k)
    ref32 = R.joint_step(sched, zc, zu, SCALE, W, n, ring, log_z, t, u, dtype=torch.float32, **kw)
    ref64 = R.joint_step(sched, zc, zu, SCALE, W, n, ring, log_z, t, u, dtype=torch.float64, **kw)
    return dict(B=B, W=W, n=n, ring=ring, Lc=Lc, zc=zc, zu=zu, xt=xt, t=t, u=u, s=SCALE, ref32=ref32, ref64=ref64)


def kept(trunc):
    """the kept set of a truncated prediction: bool[B, K, Lc] over the real classes"""
    return trunc[:, :-1] > -70.0


def near_cut(ref64, r=TRUNC_R):
    """bool[B, Lc]: columns whose top-r cut sits within 4e-7 of r (the inclusive mass at some rank of the yardstick)"""
    inc = torch.exp(torch.sort(ref64["log_pred"], dim=1, descending=True).values).cumsum(1)
    return ((inc - r).abs() < 4e-7).any(1)


# ---- chains: the 2-layer, T = 10 model, B = 2 --------------------------------------------------------------------------------
# noise: the synth key of the chain's uniforms -- chosen so that the yardstick's smallest free Gumbel gap is >= 1e-3 and its
# float32 and float64 chains agree on every token (a choice of input: test_joint_host.py asserts it)
CHAINS = {"line": dict(W=2, n=13, ring=False, skip_step=0, guided=True, held=False, noise="joint.line.v287"),
          "ring_fast2": dict(W=3, n=26, ring=True, skip_step=2, guided=False, held=False, noise="joint.ring.v12"),
          "held": dict(W=2, n=1, ring=False, skip_step=0, guided=False, held=True, noise="joint.held.v34")}


def chain_sd():
    sd = dict(synth_sd("dalle", 2))
    return {k: (v[:T_CHAIN] if k.endswith(("ln1.emb.weight", "ln1_1.emb.weight")) else v) for k, v in sd.items()}


def chain_inputs(name):
    """cond f32[2, 77, 512], null f32[2, 77, 512] (one null embedding, broadcast), known i64[2, Lc], keep bool[2, Lc]: the
    canvas head (window 0's 265 positions) held, as extend_audio holds a recording"""
    c = CHAINS[name]
    Lc = R.R * R.canvas_cols(c["W"], c["n"], c["ring"])
    cond = synth.synth_cond_emb(2, key="joint.cond")
    null = synth.synth_cond_emb(1, key="joint.null").expand(2, -1, -1).contiguous()
    g = torch.Generator().manual_seed(41)
    known = torch.randint(0, 256, (2, Lc), generator=g)
    keep = torch.zeros(2, Lc, dtype=torch.bool)
    keep[:, :L] = True
    return cond, null, known, keep


def chain_noise(name):
    return lambda k, shp: synth.synth_uniform(shp, key="%s.u%d" % (CHAINS[name]["noise"], k))


@functools.lru_cache(maxsize=None)
def chain_reference(name, dtype=torch.float32):
    """(the canvas after every call [n_calls, 2, Lc], the chain's smallest free Gumbel gap) of the yardstick's joint_loop"""
    c = CHAINS[name]
    cond, null, known, keep = chain_inputs(name)
    rec = []
    _, gap = R.joint_loop(chain_sd(), cond, null if c["guided"] else None, SCALE, c["W"], c["n"], c["ring"], chain_noise(name),
                          T=T_CHAIN, trunc_r=TRUNC_R, skip_step=c["skip_step"], keep=keep if c["held"] else None,
                          known=known if c["held"] else None, record=rec, dtype=dtype)
    return torch.stack(rec), gap
