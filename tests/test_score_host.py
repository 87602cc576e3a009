"""Likelihood scoring, host side: score_plan, and the fairness of the inputs the GPU tests (tests/test_hip_score.py) measure the
score tail on -- the yardstick (tests/score_reference.py) separates its two precisions on every case, every listed x_t form
really occurs, and the bound orders a confidently right, an uninformed and a confidently wrong prediction.  No GPU."""
import math

import pytest
import torch

import score_inputs as I
from text_to_sound_synthesis_amd.modeling.diffusion import score_plan

NO_GRAD = True


@pytest.mark.parametrize("T", [10, 100, 3])
def test_score_plan(T):
    for n in (None, T):
        ts, w = score_plan(T, n)
        assert ts == list(range(T)) and w == [1.0] * T
    for n in range(2, T):
        ts, w = score_plan(T, n)
        assert len(ts) == len(w) == n
        assert ts.count(0) == 1 and ts[0] == 0 and w[0] == 1.0
        assert len(set(ts)) == n and all(0 <= t < T for t in ts) and ts == sorted(ts)
        assert all(x == (T - 1) / (n - 1) for x in w[1:])
        assert math.isclose(math.fsum(w), T, rel_tol=1e-12)
    for bad in (0, 1, -3, T + 1, 2.5, "all", True):
        with pytest.raises(ValueError):
            score_plan(T, bad)
    with pytest.raises(ValueError):
        score_plan(0)


def test_score_plan_spreads_evenly():
    ts, _ = score_plan(100, 12)
    gaps = [b - a for a, b in zip(ts[1:], ts[2:])]
    assert max(gaps) - min(gaps) <= 1 and ts[1] >= 1 and ts[-1] <= 99


@pytest.mark.parametrize("c", I.CASES, ids=I.case_id)
def test_inputs_are_fair(c):
    d = I.case(c)
    K, L, B, xf, lf = c
    x0, xt, t = d["x0"], d["xt"], d["t"]
    assert tuple(x0.shape) == tuple(xt.shape) == (B, L) and int(x0.min()) >= 0 and int(x0.max()) < K
    assert int(xt.min()) >= 0 and int(xt.max()) <= K and int(t.min()) >= 0 and int(t.max()) < I.T
    if B == 5:
        assert t.tolist() == [0, 1, I.T - 2, I.T - 1, I.T // 2]
    # the x_t form the case names really occurs
    if xf == "mask":
        assert bool((xt == K).all())
    elif xf == "clean":
        assert torch.equal(xt, x0)
    else:
        subst = (xt != x0) & (xt != K)
        assert bool(subst.any(1).all()) and bool((xt == K).any(1).all()) and bool((xt == x0).any(1).all())
    # the two precisions of the yardstick are apart, and finitely so: d32 is a usable unit
    assert math.isfinite(d["d32"]) and d["d32"] > 0.0, d["d32"]
    assert bool(torch.isfinite(d["pos64"]).all()) and bool(torch.isfinite(d["pos32"]).all())
    assert d["d32"] <= 1e-4 * max(1.0, float(d["term64"].abs().max()))
    assert bool((d["pos64"] > -1e-9).all()), "a KL or an NLL below zero"
    # the logit form does what its name says
    z = d["z"]
    if lf == "pm30":
        assert abs(float(z.abs().max()) - 30.0) < 1e-4
    elif lf == "right":
        assert torch.equal(z.argmax(1), x0)
    else:
        assert not bool((z.argmax(1) == x0).any())
        t0 = t == 0
        if bool(t0.any()) and xf == "clean":         # the clamp: -log p(x0 | x1) is exactly 70 at every position
            assert bool((d["pos64"][t0] == 70.0).all()) and bool((d["pos32"][t0] == 70.0).all())


@pytest.mark.parametrize("c", [c for c in I.CASES if c[4] == "pm30"], ids=I.case_id)
def test_bound_orders_right_uninformed_wrong(c):
    right, uniform, wrong = (I.terms_with(c, f) for f in ("right", "uniform", "wrong"))
    assert bool((right < uniform).all()) and bool((uniform < wrong).all()), (right, uniform, wrong)
