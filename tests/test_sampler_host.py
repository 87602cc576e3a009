"""The inputs of tests/test_hip_sampler_edges.py are fair: on every case of tests/sampler_inputs.py the yardstick ALONE
(tests/sampler_reference.py, float32 against float64) meets what the GPU test demands of the kernel, and every logit family
does what its name says.  No GPU.
  * kept sets: equal, except in columns whose cut lies within 4e-7 of r, at most 1 column in 200 (both figures are those of
    tests/test_hip_guidance.py);
  * tokens: equal wherever the float64 Gumbel gap is at least 2 (4 d32 + 1e-6 + 4e-6) (d32: the case's largest posterior
    distance between the two yardsticks); at most 1 decision in 50 is below that gap;
  * the frequency test's yardstick, fed the host mirror of the in-kernel Philox stream, passes its own chi-square threshold.

normal4 at r = 1.0 runs on three chosen columns (tests/sampler_inputs.py SEEDS): the float32 running mass rounds to
float32(1.0) once less than 2^-25 (3e-8) of it is left and every class ranked after that point is dropped, while in float64
the mass stays below 1 to the last class.  On Gaussian logits about a tenth of a column's classes lie in that tail, and the
two yardsticks differ in 62 of 74 columns whatever the seed; in the chosen columns the float32 mass stays 8e-8 below the
point, and both keep all K classes.  The other families at r = 1.0 have no class that small (tied_half: >= 1e-7) or only
exact sums (const, onehot)."""
import pytest
import torch

import sampler_inputs as I

NO_GRAD = True


@pytest.mark.parametrize("cid", I.CASE_IDS)
def test_case_is_fair(cid):
    d = I.case(cid)
    c, r32, r64, same = d["c"], d["ref32"], d["ref64"], d["same"]
    cols = same.numel()
    differ = int((~same).sum())
    excused = (r64["gap"] < d["thr"]) & same
    wrong = (r32["tokens"] != r64["tokens"]) & same & ~excused
    print("%s: t %s, d32 %.2e, gap threshold %.2e, %d of %d kept sets differ, %d decisions below the gap, min log_pred %.1f"
          % (cid, c.t, d["d32"], d["thr"], differ, cols, int(excused.sum()), float(r64["log_pred"][:, :-1].min())))
    if differ:
        assert c.trunc_k is None, "top-k kept sets differ between the float32 and the float64 yardstick"
        assert bool(d["near"][~same].all()), "kept sets differ in columns whose cut is not within 4e-7 of r"
        assert differ * 200 <= cols, "%d of %d columns differ" % (differ, cols)
    if c.u_kind == "const_u":
        assert not bool(wrong.any() | (r32["tokens"] != r64["tokens"]).any())
    else:
        assert not bool(wrong.any()), "%d tokens differ above the gap threshold" % int(wrong.sum())
        assert int(excused.sum()) * 50 <= cols, "%d of %d decisions are below the gap threshold" % (int(excused.sum()), cols)
    assert len(set(c.t)) == len(c.t) or c.u_kind == "const_u"          # timesteps differ within a batch


@pytest.mark.parametrize("family", I.FAMILIES)
def test_family_does_what_its_name_says(family):
    cases = [I.case(c.id) for c in I.CASES if c.family == family]
    ts = set(t for d in cases for t in d["c"].t if d["c"].T == 100)
    assert {0, 99} <= ts, ts
    for d in cases:
        c, r32, r64 = d["c"], d["ref32"], d["ref64"]
        lp = r64["log_pred"][:, :-1]
        if family in ("spread40", "onehot", "neg_inf"):
            assert float(lp.min()) == -70.0 and float(r32["log_pred"][:, :-1].min()) == -70.0
        if family == "onehot" and c.trunc_k is None:
            want = c.K if c.trunc_r is None else 1
            assert bool((I.kept(r64["trunc"]).sum(1) == want).all()) or c.trunc_r is None
            assert bool(((lp > -70.0).sum(1) == 1).all())
        if family == "flat" and c.trunc_r == 1.0:
            assert bool(I.kept(r64["trunc"]).all()) and bool(I.kept(r32["trunc"]).all())
        if family in ("const", "tied_half") and (c.trunc_k not in (None, c.K) or c.trunc_r not in (None, 0.0, 1e-6, 1.0)) \
                and c.u_kind == "random" and c.B * c.L >= 74 and not bool(I.kept(r32["trunc"]).all()):
            # in at least one column the last kept and the first dropped rank hold the same log_pred (float32, as the kernel)
            lp32 = r32["log_pred"][:, :-1]
            k32 = I.kept(r32["trunc"])
            last_kept = torch.where(k32, lp32, torch.full_like(lp32, float("inf"))).min(1).values
            first_dropped = torch.where(~k32, lp32, torch.full_like(lp32, float("-inf"))).max(1).values
            assert bool((last_kept == first_dropped).any()), c.id


def test_flat_at_r_one_keeps_all():
    """flat at r = 1.0 is no case of the GPU matrix (every r runs on four other families): the property on its own"""
    import sampler_reference as R
    for K in (256, 512):
        z = I.logits("flat", 2, K, 37, torch.Generator().manual_seed(K))
        for dt in (torch.float32, torch.float64):
            assert bool(I.kept(R.truncated(z, 1.0, None, dt)[1]).all())


@pytest.mark.parametrize("K", [256, 512])
def test_edge_uniforms_decide_tokens(K):
    """over the edge cases of one K, every edge value is held by the winner of at least one decision, and sits on kept
    classes wherever the column keeps four or more"""
    won = {v: 0 for v in I.EDGE_U}
    for c in I.CASES:
        if c.u_kind != "edge" or c.K != K:
            continue
        d = I.case(c.id)
        r64, u = d["ref64"], d["u"]
        uw = u.gather(1, r64["tokens"][:, None, :])[:, 0]
        line = []
        for v in I.EDGE_U:
            assert bool(((u == v).sum(1) == 1).all()), "every column holds every edge value once"
            n = int((uw == torch.tensor(v, dtype=torch.float32)).sum())
            won[v] += n
            line.append(n)
        k64 = I.kept(r64["trunc"])
        four = k64.sum(1) >= 4
        on_kept = ((u[:, :-1] != 0.5) & ~k64).sum(1) == 0
        assert bool(on_kept[four].all())
        print("%s: decisions won by u = 1-2^-24, 1-2^-12, 2^-24, 0: %s" % (c.id, line))
    assert all(n > 0 for n in won.values()), won


@pytest.mark.parametrize("cid", [c.id for c in I.CASES if c.u_kind == "const_u"])
def test_const_u_columns_tie_exactly(cid):
    d = I.case(cid)
    c, r32 = d["c"], d["ref32"]
    tie = I.tying_classes(d)                                                     # [B, K+1, L]
    assert not bool(tie[:, -1].any()), "[MASK] is among the best scores"
    n_tie = tie.sum(1)
    assert int(n_tie.min()) >= 2
    first = tie.float().argmax(1)
    assert torch.equal(r32["tokens"], first) and torch.equal(d["ref64"]["tokens"], first)
    k32 = I.kept(r32["trunc"])
    lp = r32["log_pred"][:, :-1]
    best_kept = (lp == torch.where(k32, lp, torch.full_like(lp, -70.0)).max(1, keepdim=True).values) & k32
    assert torch.equal(tie[:, :-1], best_kept)                                   # the kept classes with the best log_pred
    if c.family == "const":
        assert torch.equal(first, k32.float().argmax(1))                         # = the lowest kept class index
    for b, pos in ((0, 0), (c.B - 1, c.L - 1)):
        cls = torch.nonzero(tie[b, :, pos]).flatten().tolist()
        lanes, slots = [k & 63 for k in cls], [k >> 6 for k in cls]
        shown = cls if len(cls) <= 16 else cls[:8] + ["..."] + cls[-4:]
        print("%s column (%d, %d): %d classes tie %s; lanes %s, j slots %s; expected token %d"
              % (cid, b, pos, len(cls), shown, sorted(set(lanes))[:8], sorted(set(slots)), int(first[b, pos])))
        assert len(set(lanes)) >= 2, "the tying classes sit in one lane"
        assert any(lanes[i] == lanes[j] and slots[i] != slots[j] for i in range(len(cls)) for j in range(i)), \
            "no two tying classes share a lane in different j slots"


@pytest.mark.parametrize("cid", I.Q_IDS)
def test_q_sample_case_is_fair(cid):
    d = I.q_case(cid)
    r32, r64 = d["ref32"], d["ref64"]
    excused = r64["gap"] < d["thr"]
    n = excused.numel()
    print("%s: d32 %.2e, %d of %d decisions below the gap" % (cid, d["d32"], int(excused.sum()), n))
    assert torch.equal(r32["tokens"][~excused], r64["tokens"][~excused])
    assert int(excused.sum()) * 50 <= n
    assert bool((d["x0"] == d["c"].K).any())


def test_frequency_yardstick_passes_its_own_threshold():
    K = I.FREQ["K"]
    _, _, _, post32, prob = I.freq_tail()
    likely = prob >= 0.02
    assert 6 <= int(likely.sum()) <= 10 and bool(likely[K]), prob[likely]
    tok = I.host_tokens(post32, 0)
    stat, cells = I.pearson(torch.bincount(tok.flatten(), minlength=K + 1), prob)
    thr = I.chi2_threshold(cells)
    print("tail: %d decisions, %d cells, Pearson %.2f, threshold %.2f" % (tok.numel(), cells, stat, thr))
    assert tok.numel() == 16960 and stat < thr
    lq32, p3 = I.freq_q()
    assert float(p3.min()) >= 0.02, p3
    tok = I.host_tokens(lq32, 1)
    x0 = I.FREQ["q_x0"]
    counts = torch.tensor([int((tok == x0).sum()), int((tok == K).sum()), int(((tok != x0) & (tok != K)).sum())])
    stat, cells = I.pearson(counts, p3)
    print("q_sample: cells %s of %d, expected %s, Pearson %.2f, threshold %.2f"
          % (counts.tolist(), tok.numel(), (p3 * tok.numel()).tolist(), stat, I.chi2_threshold(cells)))
    assert cells == 3 and stat < I.chi2_threshold(cells)
