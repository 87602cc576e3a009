"""Inputs of the classifier-free guidance tests, shared by tests/test_guidance_host.py (which asserts the facts that make
them fair inputs) and tests/test_hip_guidance.py (which runs the kernels on them), with the yardstick's results computed
once per process (tests/guidance_reference.py)."""
import functools

import torch

import diffsound_oracle as O
import guidance_reference as R
from conftest import synth_sd
from text_to_sound_synthesis_amd import synth

L, T_TAIL, T_CHAIN = 265, 100, 10
TRUNC_R = 0.85
# (B, guidance scale, t, logit scale): B = 3, 2, 1 with L = 265 leave ragged last workgroups (4 columns per workgroup);
# t = 99 starts from the all-[MASK] state (initial = 1)
TAIL_CASES = ((3, 3.0, 60, 4.0), (2, 7.5, 99, 4.0), (1, 0.0, 1, 4.0), (2, 1.5, 30, 2.0))
CLAMP_CASE = (2, 7.5, 50, 8.0)          # reaches the -70 clamp: compared on log_pred and kept sets only
CHAIN_SCALE = 3.0
# noise: the synth key of the chain's uniforms -- chosen so that the yardstick's smallest free Gumbel gap is >= 1e-3 (a choice
# of input: test_guidance_host.py asserts it)
CHAINS = {"plain": dict(skip_step=0, held=False, noise="guid.plain.v78"), "fast2": dict(skip_step=2, held=False, noise="guid.fast2.v2"),
          "middle": dict(skip_step=0, held=True, noise="guid.middle.v0")}
# generator seeds of the tail inputs per (K, case): chosen so that the float32 and float64 restatements agree in every kept set
# and token with a Gumbel gap >= 1e-3 (asserted by test_guidance_host.py)
TAIL_SEEDS = {(256, 1): 7266}


@functools.lru_cache(maxsize=None)
def tail_case(K, idx, trunc_k=None):
    """idx 0 .. 3: TAIL_CASES, 4: CLAMP_CASE.  Inputs (zc, zu [B, K, L]; xt, t, u, initial) and the yardstick's float32 and
    float64 restatements (ref32, ref64: guided_step's dicts)."""
    B, s, t, scale = TAIL_CASES[idx] if idx < 4 else CLAMP_CASE
    g = torch.Generator().manual_seed(TAIL_SEEDS.get((K, idx), 1000 * K + idx))
    zc = torch.randn(B, K, L, generator=g) * scale
    zu = zc + torch.randn(B, K, L, generator=g)
    initial = t == T_TAIL - 1
    xt = torch.full((B, L), K, dtype=torch.long) if initial else torch.randint(0, K + 1, (B, L), generator=g)
    u = torch.rand(B, K + 1, L, generator=g)
    tt = torch.full((B,), t, dtype=torch.long)
    sched = O.make_schedule(T_TAIL, K + 1)
    log_z = O.initial_log_z(B, K + 1, L) if initial else O.log_onehot(xt, K + 1)
    kw = dict(trunc_r=None if trunc_k else TRUNC_R, trunc_k=trunc_k)
    ref32 = R.guided_step(sched, zc, zu, s, log_z, tt, u, dtype=torch.float32, **kw)
    ref64 = R.guided_step(sched, zc, zu, s, log_z, tt, u, dtype=torch.float64, **kw)
    return dict(B=B, s=s, t=tt, zc=zc, zu=zu, xt=xt, u=u, initial=int(initial), sched=sched, log_z=log_z, ref32=ref32,
                ref64=ref64)


def kept(trunc):
    """the kept set of a truncated prediction: bool[B, K, L] over the real classes"""
    return trunc[:, :-1] > -70.0


def chain_sd():
    sd = dict(synth_sd("dalle", 2))
    return {k: (v[:T_CHAIN] if k.endswith(("ln1.emb.weight", "ln1_1.emb.weight")) else v) for k, v in sd.items()}


def chain_inputs():
    """cond, null f32[2, 77, 512] (one null embedding, broadcast), known i64[2, L], keep bool[2, L] (a held middle span)"""
    cond = synth.synth_cond_emb(2, key="guid.cond")
    null = synth.synth_cond_emb(1, key="guid.null").expand(2, -1, -1).contiguous()
    known = synth.synth_tokens(2, mask_frac=0.0, key="guid.known")
    keep = torch.zeros(2, 53, dtype=torch.bool)
    keep[0, 8:45] = True
    keep[1, 10:47] = True
    return cond, null, known, keep[:, :, None].expand(2, 53, 5).reshape(2, L).contiguous()


def chain_noise(name):
    return lambda k, shp: synth.synth_uniform(shp, key="%s.u%d" % (CHAINS[name]["noise"], k))


@functools.lru_cache(maxsize=None)
def chain_reference(name, dtype=torch.float32):
    """(tokens after every call [n_calls, 2, L], the chain's smallest free Gumbel gap) of the yardstick's guided_loop"""
    cond, null, known, keep = chain_inputs()
    c = CHAINS[name]
    rec = []
    _, gap = R.guided_loop(chain_sd(), cond, null, CHAIN_SCALE, chain_noise(name), T=T_CHAIN, trunc_r=TRUNC_R,
                           skip_step=c["skip_step"], keep=keep if c["held"] else None, known=known if c["held"] else None,
                           record=rec, dtype=dtype)
    return torch.stack(rec), gap
