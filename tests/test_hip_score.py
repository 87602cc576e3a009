"""Likelihood scoring on the GPU: the score tail (ds_score_tail), the one-call driver (ds_denoiser_score_rng), the module
methods and the drivers.
  * per position the tail is ds_loss_tail's kl (t > 0) / nll (t == 0) bit for bit, on every case of tests/score_inputs.py
    (whose fairness tests/test_score_host.py asserts);
  * row terms within TOL_MULT x d32 of the float64 yardstick (tests/score_reference.py; d32 = the distance of its float32
    restatement from it on the same case), and within L 2^-52 sum |pos| of math.fsum over the dumped positions;
  * padded rows (lrows = 272, the rest filled with 37.0 and with NaN) and batch independence, bit for bit; argument checks;
  * on the 2-layer T = 10 model: the one-call driver == its three stages composed by hand, bit for bit; score_tokens' full
    bound against the oracle's float64 forward on the kernel's own x_t, in both precision modes; launch tiling, timesteps = T,
    draws; rank_captions, generate_best_of and score_audio.
GPU only (-m gpu)."""
import math

import pytest
import torch

import diffsound_oracle as O
import score_inputs as I
import score_reference as R
from conftest import parity_line, synth_sd
from text_to_sound_synthesis_amd import _lib, synth

pytestmark = pytest.mark.gpu
NO_GRAD = True

SEED = (0x5eed << 32) | 20261019
PAD_FILL = 37.0
NAN = float("nan")


def rows(z, lrows, fill=PAD_FILL):
    """logits [B, K, n] -> the kernel's row-major [B * lrows][K] on the device; rows n .. lrows-1 of a sample hold `fill`"""
    B, K, n = z.shape
    out = torch.full((B, lrows, K), fill)
    out[:, :n] = z.permute(0, 2, 1)
    return out.reshape(B * lrows, K).contiguous().cuda()


_SCHED = {}


def sched_table(K, T=I.T):
    if (K, T) not in _SCHED:
        s = O.make_schedule(T, K + 1)
        tab = torch.zeros(8, T + 1)
        for i, name in enumerate(("log_at", "log_bt", "log_ct", "log_1_min_ct")):
            tab[i, :T] = s[name]
        for i, name in enumerate(("log_cumprod_at", "log_cumprod_bt", "log_cumprod_ct", "log_1_min_cumprod_ct")):
            tab[4 + i] = s[name]
        _SCHED[(K, T)] = tab.cuda()
    return _SCHED[(K, T)]


def score_tail(d, sel=None, lrows=None, fill=PAD_FILL, claim=None, null=()):
    """ds_score_tail on a case of score_inputs (sel: the rows to take, in that order) -> (rc, term f64[B], pos f32[B, L]),
    both pre-filled with NaN.  claim: arguments to misstate (lrows, B, L, K); null: names of pointers to pass as NULL."""
    K, L = d["K"], d["L"]
    sel = list(range(d["B"])) if sel is None else sel
    B = len(sel)
    lrows = L if lrows is None else lrows
    a = dict(logits=rows(d["z"][sel], lrows, fill), x0=d["x0"][sel].contiguous().cuda(), xt=d["xt"][sel].contiguous().cuda(),
             t=d["t"][sel].contiguous().cuda(), sched=sched_table(K))
    term = torch.full((B,), NAN, dtype=torch.float64, device="cuda")
    pos = torch.full((B, L), NAN, device="cuda")
    a.update(term=term, pos=pos)
    p = {k: (None if k in null else _lib.ptr(v)) for k, v in a.items()}
    n = dict(lrows=lrows, B=B, L=L, K=K)
    n.update(claim or {})
    rc = _lib.lib().ds_score_tail(p["logits"], p["x0"], p["xt"], p["t"], p["sched"], p["term"], p["pos"], n["lrows"], n["B"],
                                  n["L"], n["K"], I.T, _lib.stream())
    torch.cuda.synchronize()
    return rc, term, pos


_RUN = {}


def run(c):
    """the plain call of case c (lrows = L), once per session, never modified"""
    if c not in _RUN:
        rc, term, pos = score_tail(I.case(c))
        assert rc == 0, _lib.lib().ds_last_error_string()
        _RUN[c] = (term.cpu(), pos.cpu())
    return _RUN[c]


# ---- 1. per position: ds_loss_tail's arithmetic, bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("c", I.CASES, ids=I.case_id)
def test_positions_are_the_loss_tails(c):
    d = I.case(c)
    K, L, B = d["K"], d["L"], d["B"]
    z, x0, xt, t = rows(d["z"], L), d["x0"].cuda(), d["xt"].cuda(), d["t"].cuda()
    kl, nll, aux = (torch.full((B, L), NAN, device="cuda") for _ in range(3))
    _lib.check(_lib.lib().ds_loss_tail(_lib.ptr(z), _lib.ptr(x0), _lib.ptr(xt), _lib.ptr(t), _lib.ptr(sched_table(K)),
                                       _lib.ptr(kl), _lib.ptr(nll), _lib.ptr(aux), None, B, L, K, I.T, _lib.stream()))
    torch.cuda.synchronize()
    want = torch.where((t == 0)[:, None], nll, kl).cpu()
    _, pos = run(c)
    assert bool(torch.isfinite(pos).all())
    assert torch.equal(pos.view(torch.int32), want.view(torch.int32)), \
        "%d positions differ from ds_loss_tail, max %.3e" % (int((pos != want).sum()), float((pos - want).abs().max()))


# ---- 2. row terms against the float64 yardstick -----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", I.CASES, ids=I.case_id)
def test_terms_vs_yardstick(c):
    d = I.case(c)
    term, pos = run(c)
    err = float((term - d["term64"]).abs().max())
    perr = float((pos.double() - d["pos64"]).abs().max())
    print("score tail %s: term err %.3e vs f64 (d32 %.3e, bound %.3e), position err %.3e, |term| max %.4g"
          % (I.case_id(c), err, d["d32"], I.TOL_MULT * d["d32"], perr, float(d["term64"].abs().max())))
    parity_line("score tail %-28s term %.2e (%g d32 = %.2e)" % (I.case_id(c), err, I.TOL_MULT, I.TOL_MULT * d["d32"]))
    for b in range(d["B"]):
        vals = [float(v) for v in pos[b]]
        exact = math.fsum(vals)
        assert abs(float(term[b]) - exact) <= d["L"] * 2.0 ** -52 * math.fsum(abs(v) for v in vals), (b, float(term[b]), exact)
    assert err <= I.TOL_MULT * d["d32"], "row terms %.3e from the float64 yardstick, %g x d32 = %.3e" % (err, I.TOL_MULT,
                                                                                                    I.TOL_MULT * d["d32"])


# ---- 3. padded rows; batch independence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", I.CASES, ids=I.case_id)
def test_padded_rows_are_never_read(c):
    d = I.case(c)
    term, pos = run(c)
    for fill in (PAD_FILL, NAN):
        rc, term_p, pos_p = score_tail(d, lrows=272, fill=fill)
        assert rc == 0
        assert torch.equal(term_p.cpu().view(torch.int64), term.view(torch.int64)), "terms differ at lrows = 272, fill %r" % fill
        assert torch.equal(pos_p.cpu().view(torch.int32), pos.view(torch.int32)), "the map differs at lrows = 272, fill %r" % fill


@pytest.mark.parametrize("c", [c for c in I.CASES if c[2] == 5], ids=I.case_id)
def test_a_row_does_not_depend_on_its_batch(c):
    d = I.case(c)
    term, pos = run(c)
    perm = [3, 0, 4, 2, 1]
    rc, term_p, pos_p = score_tail(d, sel=perm)
    assert rc == 0 and torch.equal(term_p.cpu().view(torch.int64), term[perm].view(torch.int64))
    assert torch.equal(pos_p.cpu().view(torch.int32), pos[perm].view(torch.int32))
    for b in (0, 3):
        rc, one, pos_1 = score_tail(d, sel=[b])
        assert rc == 0 and torch.equal(one.cpu().view(torch.int64), term[b:b + 1].view(torch.int64))
        assert torch.equal(pos_1.cpu().view(torch.int32), pos[b:b + 1].view(torch.int32))


# ---- 4. argument checks -------------------------------------------------------------------------------------------------------------
def test_tail_argument_checks():
    d = I.case((256, 265, 5, "mixed", "pm30"))
    lib = _lib.lib()
    bad = [dict(null=(name,)) for name in ("logits", "x0", "xt", "t", "sched", "term")]
    bad += [dict(claim={"K": 300}), dict(claim={"K": 1024}), dict(claim={"lrows": 264}), dict(claim={"L": 289, "lrows": 289}),
            dict(claim={"B": 0}), dict(claim={"B": -2})]
    for kw in bad:
        rc, term, pos = score_tail(d, **kw)
        assert rc == -1, kw
        assert b"ds_score_tail" in lib.ds_last_error_string(), (kw, lib.ds_last_error_string())
        assert bool(torch.isnan(term).all()) and bool(torch.isnan(pos).all()), "a rejected call wrote: %r" % (kw,)
    rc, term, pos = score_tail(d, null=("pos",))                         # the map is optional
    assert rc == 0 and torch.equal(term.cpu().view(torch.int64), run((256, 265, 5, "mixed", "pm30"))[0].view(torch.int64))
    assert bool(torch.isnan(pos).all())


# ---- 5. the 2-layer T = 10 model -----------------------------------------------------------------------------------------------------
T10, L, K = 10, 265, 256


def build(mode):
    from text_to_sound_synthesis_amd.config import build_model, default_config
    m = build_model(default_config(n_layer=2, diffusion_step=T10, n_embed=256))
    m.load_state_dict(chain_sd(), strict=False)
    m.transformer.transformer.precision = mode
    return m.cuda().eval()


def chain_sd(dtype=torch.float32):
    sd = dict(synth_sd("dalle", 2))
    sd = {k: (v[:T10] if k.endswith(("ln1.emb.weight", "ln1_1.emb.weight")) else v) for k, v in sd.items()}
    return sd if dtype == torch.float32 else {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


_MODEL = {}


def model(mode="f16x2"):
    if mode not in _MODEL:
        _MODEL[mode] = build(mode)
    return _MODEL[mode]


def clips(n, key="score"):
    return synth.synth_tokens(n, mask_frac=0.0, key=key + ".x0"), synth.synth_cond_emb(n, key=key + ".cond")


def q_sample_rng(dt, x0, t, gids, call, seed=SEED):
    xt = torch.empty_like(x0)
    _lib.check(_lib.lib().ds_q_sample_rng(_lib.ptr(x0), _lib.ptr(t), _lib.ptr(gids), seed, call, _lib.ptr(dt._schedule_table()),
                                          _lib.ptr(xt), x0.shape[0], L, K, T10, _lib.stream()))
    return xt


def score_rows(dt, x0, t, cond, gids, call, want_map=True, seed=SEED):
    """one ds_denoiser_score_rng launch on rows given as they are -> (rc, term, map, x_t scratch), outputs pre-filled"""
    B = x0.shape[0]
    sched = dt._schedule_table()
    tr = dt.transformer
    p = tr.packed(sched)
    kv = tr.condition_kv(cond.contiguous(), sched)
    term = torch.full((B,), NAN, dtype=torch.float64, device="cuda")
    pos = torch.full((B, L), NAN, device="cuda") if want_map else None
    xt = torch.full_like(x0, -1)
    rc = _lib.lib().ds_denoiser_score_rng(p["handle"], _lib.ptr(x0), _lib.ptr(t), _lib.ptr(kv), _lib.ptr(gids), seed, call, B,
                                          _lib.ptr(tr.workspace(B, sched)), _lib.ptr(xt), _lib.ptr(term), _lib.ptr(pos),
                                          _lib.stream())
    torch.cuda.synchronize()
    return rc, term, pos, xt


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
def test_one_call_driver_is_its_stages_composed(mode):
    dt = model(mode).transformer
    x0, cond = (v.cuda() for v in clips(5))
    t = torch.tensor([0, 1, T10 - 2, T10 - 1, 4], device="cuda")
    gids = torch.tensor([7, 123456, 2 ** 31 + 5, 0, 9], device="cuda")
    sched = dt._schedule_table()
    tr = dt.transformer
    p = tr.packed(sched)
    assert int(_lib.lib().ds_denoiser_rows_per_sample(p["handle"], 5)) == L
    rc, term, pos, xt = score_rows(dt, x0, t, cond, gids, call=3)
    assert rc == 0, _lib.lib().ds_last_error_string()
    xt_h = q_sample_rng(dt, x0, t, gids, 3)
    kv = tr.condition_kv(cond.contiguous(), sched)
    logits = torch.empty(5 * L, K, device="cuda")
    _lib.check(_lib.lib().ds_denoiser_forward(p["handle"], _lib.ptr(xt_h), _lib.ptr(t), _lib.ptr(kv), 5,
                                              _lib.ptr(tr.workspace(5, sched)), _lib.ptr(logits), 0, _lib.stream()))
    term_h = torch.full((5,), NAN, dtype=torch.float64, device="cuda")
    pos_h = torch.full((5, L), NAN, device="cuda")
    _lib.check(_lib.lib().ds_score_tail(_lib.ptr(logits), _lib.ptr(x0), _lib.ptr(xt_h), _lib.ptr(t), _lib.ptr(sched),
                                        _lib.ptr(term_h), _lib.ptr(pos_h), L, 5, L, K, T10, _lib.stream()))
    torch.cuda.synchronize()
    assert torch.equal(xt, xt_h) and bool(torch.isfinite(term).all())
    assert torch.equal(term.view(torch.int64), term_h.view(torch.int64)) and torch.equal(pos.view(torch.int32), pos_h.view(torch.int32))


def test_driver_rejects_before_enqueuing():
    dt = model().transformer
    x0, cond = (v.cuda() for v in clips(2))
    t = torch.tensor([0, 5], device="cuda")
    gids = torch.arange(2, device="cuda")
    sched = dt._schedule_table()
    tr = dt.transformer
    p = tr.packed(sched)
    kv, ws = tr.condition_kv(cond.contiguous(), sched), tr.workspace(2, sched)
    term = torch.full((2,), NAN, dtype=torch.float64, device="cuda")
    xt = torch.full_like(x0, -1)
    lib = _lib.lib()
    full = [p["handle"], _lib.ptr(x0), _lib.ptr(t), _lib.ptr(kv), _lib.ptr(gids), SEED, 0, 2, _lib.ptr(ws), _lib.ptr(xt),
            _lib.ptr(term), None, _lib.stream()]
    for i in (0, 1, 2, 3, 4, 8, 9, 10):
        a = list(full)
        a[i] = None
        assert lib.ds_denoiser_score_rng(*a) == -1 and b"ds_denoiser_score_rng" in lib.ds_last_error_string(), i
    for B in (0, -1):
        a = list(full)
        a[7] = B
        assert lib.ds_denoiser_score_rng(*a) == -1 and b"ds_denoiser_score_rng" in lib.ds_last_error_string()
    torch.cuda.synchronize()
    assert bool((xt == -1).all()) and bool(torch.isnan(term).all()), "a rejected call enqueued work"
    assert lib.ds_denoiser_score_rng(*full) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(term).all()) and not bool((xt == -1).any())


_ORACLE = {}


def oracle_bound(ids=(11, 500)):
    """The full bound of two clips by the oracle's float64 and float32 forwards, on the KERNEL's x_t (oracle.train_loss
    documents why: a float64 Gumbel argmax can resolve a near-tie differently) -> (score64 f64[2], d32, x0, cond)."""
    if ids not in _ORACLE:
        dt = model("fp32").transformer
        x0, cond = clips(2)
        N = 2
        t = torch.arange(T10).repeat_interleave(N)                                      # timestep-major rows
        x_rows, c_rows = x0.repeat(T10, 1), cond.repeat(T10, 1, 1)
        g_rows = torch.tensor(ids).repeat(T10)
        xt = q_sample_rng(dt, x_rows.cuda(), t.cuda(), g_rows.cuda(), 0).cpu()
        s = {}
        for dtype in (torch.float64, torch.float32):
            _, term = R.forward_terms(chain_sd(dtype), x_rows, xt, c_rows, t, T10)
            s[dtype] = term.view(T10, N).sum(0)
        _ORACLE[ids] = (s[torch.float64], float((s[torch.float32] - s[torch.float64]).abs().max()), x0, cond, xt)
    return _ORACLE[ids]


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
def test_full_bound_vs_float64_oracle(mode):
    ids = (11, 500)
    want, d32, x0, cond, xt = oracle_bound(ids)
    assert d32 > 0.0 and bool((xt == K).any()) and bool((xt != K).any())
    dt = model(mode).transformer
    kw = dict(condition_embed=cond.cuda(), caption_ids=list(ids), seed=SEED)
    got, terms, amap = dt.score_tokens(x0.cuda(), return_terms=True, return_map=True, **kw)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2,) and tuple(terms.shape) == (2, T10) and tuple(amap.shape) == (2, L)
    err = float((got.cpu() - want).abs().max())
    print("score_tokens %s: full bound %s nats, err %.3e vs float64 oracle (d32 %.3e, bound %.3e, relative %.2e)"
          % (mode, [round(float(v), 4) for v in got], err, d32, I.TOL_MULT * d32, err / float(want.abs().max())))
    parity_line("score_tokens T=10 %-5s: full bound err %.2e vs f64 oracle (%g d32 = %.2e)" % (mode, err, I.TOL_MULT, I.TOL_MULT * d32))
    assert torch.allclose(terms.sum(1), got, rtol=1e-12, atol=0) and torch.allclose(amap.double().sum(1), got, rtol=1e-6, atol=0)
    assert err <= I.TOL_MULT * d32
    # launch tiling: 20 rows as one launch and as launches of 7, 7, 6 -- other GEMM programs, the same bound
    by7 = dt.score_tokens(x0.cuda(), rows_per_launch=7, **kw)
    e7, gap = float((by7.cpu() - want).abs().max()), float((by7 - got).abs().max())
    print("score_tokens %s: rows_per_launch 7 err %.3e, 64 vs 7 %.3e" % (mode, e7, gap))
    assert e7 <= I.TOL_MULT * d32 and gap <= I.TOL_MULT * d32
    for rpl in (64, 7):
        again = dt.score_tokens(x0.cuda(), rows_per_launch=rpl, **kw)
        assert torch.equal(again.view(torch.int64), (got if rpl == 64 else by7).view(torch.int64)), "two equal calls differ"
    assert torch.equal(dt.score_tokens(x0.cuda(), timesteps=T10, **kw).view(torch.int64), got.view(torch.int64))


def test_draws_and_subsampled_timesteps():
    from text_to_sound_synthesis_amd.modeling.diffusion import score_plan
    dt = model().transformer
    x0, cond = (v.cuda() for v in clips(2))
    ids = [11, 500]
    kw = dict(condition_embed=cond, caption_ids=ids, seed=SEED)
    two, terms2 = dt.score_tokens(x0, draws=2, return_terms=True, **kw)
    t = torch.arange(T10, device="cuda").repeat_interleave(2)
    gids = torch.tensor(ids, device="cuda").repeat(T10)
    per_draw = []
    for r in (0, 1):
        rc, term, _, _ = score_rows(dt, x0.repeat(T10, 1), t, cond.repeat(T10, 1, 1), gids, call=r, want_map=False)
        assert rc == 0
        per_draw.append(term.view(T10, 2).t())
    assert not torch.equal(per_draw[0], per_draw[1])
    assert torch.equal(terms2, (per_draw[0] + per_draw[1]) / 2)
    assert torch.allclose(two, ((per_draw[0] + per_draw[1]) / 2).sum(1), rtol=1e-13, atol=0)
    one, terms1 = dt.score_tokens(x0, return_terms=True, **kw)
    assert torch.equal(terms1, per_draw[0])
    # a sub-sampled bound: the planned timesteps' terms of the full bound, re-weighted
    ts, w = score_plan(T10, 4)
    sub, terms_s = dt.score_tokens(x0, timesteps=4, return_terms=True, **kw)
    assert tuple(terms_s.shape) == (2, 4)
    want = (terms_s * torch.tensor(w, dtype=torch.float64, device="cuda")).sum(1)
    assert torch.allclose(sub, want, rtol=1e-13, atol=0)
    # (8 rows in one launch, not 20: another GEMM program may serve them -- fp32-class agreement, not bits)
    assert torch.allclose(terms_s, terms1[:, ts], rtol=1e-4, atol=1e-6)
    with pytest.raises(ValueError):
        dt.score_tokens(torch.full_like(x0, K), **kw)
    with pytest.raises(ValueError):
        dt.score_tokens(x0, timesteps=1, **kw)
    with pytest.raises(ValueError):
        dt.score_tokens(x0, draws=0, **kw)


# ---- 6. the drivers ------------------------------------------------------------------------------------------------------------------
def test_rank_captions_pairs_clips_and_captions():
    m = model()
    dt = m.transformer
    x0, _ = (v.cuda() for v in clips(2))
    base = synth.synth_cond_emb(1, key="score.rank")
    caps = torch.cat((16.0 * base, -16.0 * base, torch.zeros_like(base))).cuda()   # three captions the network tells apart
    ids, seed = [3, 8], 11
    r = m.rank_captions({"content_token": x0, "caption_ids": ids, "seed": seed}, caps, timesteps=4)
    assert r.dtype == torch.float64 and tuple(r.shape) == (2, 3) and bool(torch.isfinite(r).all())
    flat = dt.score_tokens(x0.repeat_interleave(3, 0), condition_embed=caps.repeat(2, 1, 1), timesteps=4,
                           caption_ids=[3, 3, 3, 8, 8, 8], seed=seed)
    assert torch.equal(r.view(-1), flat)
    # Every pair on its own: one clip under one caption, the clip's id and the seed.  That is a launch of 4 rows instead of
    # 24, so possibly another GEMM program: the programs agree to ~1e-7 relative on the logits (csrc/api.hip rows_per_sample)
    # and a score is a sum of 4 x 265 non-negative terms of fp32 arithmetic on them, so 1e-6 relative -- ten times the
    # logits' agreement, 17 fp32 epsilons -- bounds the difference.  The input is fair if the captions move a clip's score
    # by more than twice that: then a pair's own score is nearer to its entry of the matrix than to any other.
    PAIR_TOL = 1e-6
    gap = min(abs(float(r[n, a] - r[n, b])) / abs(float(r[n, a])) for n in range(2) for a in range(3) for b in range(a))
    pair_err = 0.0
    for n in range(2):
        for c in range(3):
            s = float(dt.score_tokens(x0[n:n + 1], condition_embed=caps[c:c + 1], timesteps=4, caption_ids=[ids[n]], seed=seed))
            pair_err = max(pair_err, abs(s - float(r[n, c])) / abs(float(r[n, c])))
            assert int((r - s).abs().argmin()) == 3 * n + c, "pair (%d, %d) is nearest to another entry" % (n, c)
    print("rank_captions: pairs alone differ by %.2e relative from the matrix, captions move a score by >= %.2e" % (pair_err, gap))
    assert gap > 2 * PAIR_TOL, "the captions do not tell the pairs apart: unfair input"
    assert pair_err <= PAIR_TOL


_DS = {}


def diffsound():
    if "ds" not in _DS:
        from text_to_sound_synthesis_amd import pipeline
        from text_to_sound_synthesis_amd.config import default_config
        ds = pipeline.Diffsound(config=default_config(n_layer=2, diffusion_step=T10), random_vocoder=True)
        synth.synth_init_(ds.model, seed=0)                  # seeded weights, before anything is packed from them
        synth.synth_init_(ds.vocoder, seed=0)
        _DS["ds"] = ds
    return _DS["ds"]


def test_generate_best_of_and_score_audio():
    ds = diffsound()
    dt = ds.model.transformer
    cond = synth.synth_cond_emb(2, key="score.best").cuda()
    ids, seed = [4, 9], 5
    mel01, wave, tokens, scores = ds.generate_best_of(cond, 3, caption_ids=ids, seed=seed)
    assert tuple(mel01.shape) == (2, 80, 848) and tuple(wave.shape) == (2, 1, 217088) and tuple(tokens.shape) == (2, L)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (2, 3) and bool(torch.isfinite(scores).all())
    cand = ds.generate_sample_with_condition(cond, replicate=3, caption_ids=ids, seed=seed)[2]         # [3 x 2, 265]
    want = dt.score_tokens(cand, condition_embed=cond.repeat(3, 1, 1), caption_ids=ids * 3, seed=seed).view(3, 2).t()
    assert torch.equal(scores, want)
    cand = cand.view(3, 2, L)
    for b in range(2):
        best = min(range(3), key=lambda r: (float(scores[b, r]), r))
        assert torch.equal(tokens[b], cand[best, b]), "caption %d: not the replicate of lowest score" % b
    assert not torch.equal(cand[0], cand[1])
    # a rendered clip, scored from its audio: the tokens the encoder gives it, scored as score_content scores them
    audio = wave[:, 0].contiguous()
    out = ds.score_audio(audio, cond, timesteps=3, caption_ids=ids, seed=seed)
    toks = ds.model.prepare_content({"audio": audio})["content_token"]
    ref = ds.model.score_content({"condition_embed_token": cond, "content_token": toks, "caption_ids": ids, "seed": seed}, timesteps=3)
    assert tuple(out["nats"].shape) == (2,) and tuple(out["terms"].shape) == (2, 3) and bool(torch.isfinite(out["nats"]).all())
    assert torch.equal(out["nats"], ref["nats"]) and torch.equal(out["terms"], ref["terms"])
    assert torch.equal(out["bits_per_token"], out["nats"] / (L * math.log(2.0)))
