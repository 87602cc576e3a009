"""The inputs of the score-tail tests (tests/test_score_host.py asserts their fairness, tests/test_hip_score.py runs them on the
GPU) and the yardstick's answers on them, computed once per case and shared.  A case is (K, L, B, x_t form, logit form):
  K        256 | 512
  L        265 (the grid) | 7 (not a multiple of anything a workgroup or a wave owns)
  B        5: rows at t = 0, 1, T-2, T-1 and T/2 in ONE call | 1: one row, t cycling over 1, T-2, T-1 (t = 0 alone with
           saturated logits is exactly 70 per position in every precision: no distance to measure; B = 5 covers t = 0)
  x_t      "mask": all [MASK] | "clean": nothing masked, x_t == x0 | "mixed": a third of the positions substituted by ANOTHER
           real token, a third masked, the rest equal to x0
  logits   "pm30": Gaussian scaled to +-30 | "right": confidently right, 40 on x0's class (terms near 0) | "wrong":
           confidently wrong, 200 on another class (x0's log-probability clamps at -70)
Host only: no GPU is touched here."""
import functools

import torch

import score_reference as R

T = 100
TOL_MULT = 4.0            # the project's multiplier (tests/purity_inputs.py): GPU error <= TOL_MULT x d32 on the same case
XT_FORMS = ("mask", "clean", "mixed")
LOGIT_FORMS = ("pm30", "right", "wrong")
CASES = [(K, L, B, xf, lf) for K in (256, 512) for L in (265, 7) for B in (5, 1) for xf in XT_FORMS for lf in LOGIT_FORMS]


def case_id(c):
    return "K%d-L%d-B%d-%s-%s" % c


def timesteps(B, index):
    return torch.tensor([0, 1, T - 2, T - 1, T // 2][:B] if B > 1 else [(1, T - 2, T - 1)[index % 3]], dtype=torch.long)


def logits_of(form, x0, K, g):
    B, L = x0.shape
    z = torch.randn(B, K, L, generator=g)
    if form == "pm30":
        return (z * (30.0 / z.abs().max())).contiguous()
    if form == "uniform":
        return torch.zeros(B, K, L)
    hot = x0 if form == "right" else (x0 + 1 + torch.randint(0, K - 1, x0.shape, generator=g)) % K
    return (z + (40.0 if form == "right" else 200.0) * torch.nn.functional.one_hot(hot, K).permute(0, 2, 1).float()).contiguous()


@functools.lru_cache(maxsize=None)
def case(c):
    """-> dict: K, L, B, t i64[B], x0, xt i64[B, L], z f32[B, K, L], pos32 / pos64 (the yardstick's positions in both
    precisions), term32 / term64 f64[B], d32 = max_b |term32 - term64|.  Cached: computed once, shared, never modified."""
    K, L, B, xf, lf = c
    index = CASES.index(c)
    g = torch.Generator().manual_seed(7000 + index)
    x0 = torch.randint(0, K, (B, L), generator=g)
    if xf == "mask":
        xt = torch.full((B, L), K)
    elif xf == "clean":
        xt = x0.clone()
    else:
        r = (torch.arange(L)[None, :] + torch.arange(B)[:, None]) % 3        # every row holds all three kinds, at L = 7 too
        other = (x0 + 1 + torch.randint(0, K - 1, (B, L), generator=g)) % K
        xt = torch.where(r == 0, other, torch.where(r == 1, torch.full((B, L), K), x0))
    t = timesteps(B, index)
    z = logits_of(lf, x0, K, g)
    pos32, term32 = R.score_terms(z, x0, xt, t, T, torch.float32)
    pos64, term64 = R.score_terms(z, x0, xt, t, T, torch.float64)
    return dict(K=K, L=L, B=B, t=t, x0=x0, xt=xt, z=z, pos32=pos32, pos64=pos64, term32=term32, term64=term64,
                d32=float((term32 - term64).abs().max()))


def terms_with(c, form):
    """the float64 row terms of case c's (x0, x_t, t) under another logit form ("uniform": all zeros)"""
    d = case(c)
    g = torch.Generator().manual_seed(8000 + CASES.index(c))
    return R.score_terms(logits_of(form, d["x0"], d["K"], g), d["x0"], d["xt"], d["t"], T, torch.float64)[1]
