"""Purity-prior sampling on the GPU: the two purity kernels, the step / chain entries, the module methods and the drivers.
  * the tail (ds_sample_tail_purity) against tests/purity_reference.py on the inputs of tests/purity_inputs.py (whose fairness
    tests/test_purity_host.py asserts): dbg_sharp within TOL_MULT x d32 of the float64 yardstick (d32 = the distance between
    its float32 and float64 restatements, computed here); candidates, revealed sets and tokens equal to the float32 yardstick
    wherever the float64 one decides by more than MARGIN_MULT x the same kind of distance, with at most 0.5 % of the candidate
    draws and one selection in 50 samples excused; the exact invariants; padded rows; the _rng entry == the caller-uniform
    entry fed shard.caption_uniforms;
  * weight 0 == the plain tails' truncated prediction bit for bit, batch independence, argument checks;
  * chains on the 2-layer T = 10 model: the one-call chain == S single steps bit for bit == the float32 yardstick's chain,
    held tokens exact, guided, B = 1;
  * the sample_type mini-language and the drivers.
GPU only (-m gpu)."""
import os

import pytest
import torch

import diffsound_oracle as O
import purity_inputs as I
import purity_reference as R
from conftest import GOLDEN, parity_line, synth_sd
from text_to_sound_synthesis_amd import _lib, shard, synth
from text_to_sound_synthesis_amd.modeling.diffusion import purity_plan

pytestmark = pytest.mark.gpu
NO_GRAD = True

SEED = (0x5eed << 32) | 20261019
L = 265
PAD_FILL = 37.0          # what the rows of the padded-row layout that no position owns are filled with


def rows(z, lrows):
    """logits [B, K, n] -> the kernel's row-major [B * lrows][K] on the device; rows n .. lrows-1 of a sample hold PAD_FILL"""
    B, K, n = z.shape
    out = torch.full((B, lrows, K), PAD_FILL)
    out[:, :n] = z.permute(0, 2, 1)
    return out.reshape(B * lrows, K).contiguous().cuda()


def scratch_for(B, n):
    nbytes = int(_lib.lib().ds_purity_scratch_bytes(B, n))
    assert nbytes == 8 * B * n
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda")


def tail(d, u=None, gids=None, call=0, x=None, remain=None, weight=None, lrows=None, dumps=True, scale=None, trunc=None,
         guided=None, K=None, scratch="own", claim_lrows=None):
    """ds_sample_tail_purity (u) / ds_sample_tail_purity_rng (gids) on a case of purity_inputs -> (rc, tokens, sharp, key, cand)"""
    K, n = d["K"] if K is None else K, d["L"]
    x = (d["x"] if x is None else x).cuda().contiguous()
    B = x.shape[0]
    lrows = n if lrows is None else lrows
    z = rows(d["z"][:B], lrows)
    guided = (d["zu"] is not None) if guided is None else guided
    zu = rows(d["zu"][:B], lrows) if guided else None
    out = torch.full((B, n), -1, dtype=torch.long, device="cuda")
    sharp = torch.full((B, d["K"] + 1, n), float("nan"), device="cuda") if dumps else None
    key = torch.full((B, n), float("nan"), device="cuda") if dumps else None
    cand = torch.full((B, n), -1, dtype=torch.int32, device="cuda") if dumps else None
    sc = scratch_for(B, n) if scratch == "own" else scratch
    tr, tk = (d["trunc_r"], d["trunc_k"]) if trunc is None else trunc
    common = (d["remain"] if remain is None else remain, d["weight"] if weight is None else weight, tr, tk,
              lrows if claim_lrows is None else claim_lrows, _lib.ptr(sc),
              _lib.ptr(out), _lib.ptr(sharp), _lib.ptr(key), _lib.ptr(cand), B, n, K, _lib.stream())
    s = d["scale"] if scale is None else scale
    if gids is None:
        u = (d["u"] if u is None else u)[:B].cuda().contiguous()
        rc = _lib.lib().ds_sample_tail_purity(_lib.ptr(z), _lib.ptr(zu), s, _lib.ptr(x), _lib.ptr(u), *common)
    else:
        rc = _lib.lib().ds_sample_tail_purity_rng(_lib.ptr(z), _lib.ptr(zu), s, _lib.ptr(x), _lib.ptr(gids), SEED, call, *common)
    torch.cuda.synchronize()
    return rc, out, sharp, key, cand


def check_invariants(x, out, remain, K):
    """the exact rules of a purity step, whatever the arithmetic: x, out i64[B, n] on the host"""
    m = (x == K).sum(1)
    assert torch.equal((out == K).sum(1), torch.clamp(m, max=remain)), "masks after the step != min(m, R)"
    assert torch.equal(out[x != K], x[x != K]), "a non-[MASK] token changed"
    assert int(out.min()) >= 0 and int(out.max()) <= K
    for b in range(x.shape[0]):
        if remain >= int(m[b]):
            assert torch.equal(out[b], x[b]), "R >= m is the identity"
    if remain == 0:
        assert not bool((out == K).any())


# ---- 1. the tail against the yardstick --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", I.TAIL_CASES, ids=I.case_id)
def test_tail_vs_yardstick(c):
    d = I.tail_case(c)
    K, n, x, remain = d["K"], d["L"], d["x"], d["remain"]
    r32, r64 = d["ref32"], d["ref64"]
    d_sharp, cand_margin, sel_margin, exc, exs = I.tail_margins(c)
    rc, tok, sharp, key, cand = tail(d)
    assert rc == 0, _lib.lib().ds_last_error_string()
    tok, sharp, key, cand = tok.cpu(), sharp.cpu(), key.cpu(), cand.cpu().long()
    err = float((sharp.double() - r64["sharp"]).abs().max())
    print("purity tail %s: sharp err %.3e vs f64 (d32 %.3e), cand margin %.2e (%d excused), selection margin %.2e (%d excused)"
          % (I.case_id(c), err, d_sharp, cand_margin, int(exc.sum()), sel_margin, int(exs.sum())))
    assert err <= I.TOL_MULT * d_sharp, "dbg_sharp %.3e from the float64 yardstick, %g x d32 = %.3e" % (err, I.TOL_MULT,
                                                                                                      I.TOL_MULT * d_sharp)
    assert bool((sharp[:, -1] == -70.0).all())
    # candidates: every position draws one, [MASK] or not
    assert int(exc.sum()) * 200 <= exc.numel() and int(exs.sum()) * 50 <= exs.numel()
    assert int(cand.min()) >= 0 and int(cand.max()) < K
    assert torch.equal(cand[~exc], r32["cand"][~exc]), "%d candidates differ" % int((cand != r32["cand"])[~exc].sum())
    # keys: the sentinel off [MASK], a finite value on it
    mask = x == K
    assert bool((key[~mask] == -float("inf")).all()) and bool(torch.isfinite(key[mask]).all())
    kerr = float((key.double() - r64["key"])[mask].abs().max())
    assert kerr <= sel_margin, "key %.3e from the float64 yardstick, margin %.3e" % (kerr, sel_margin)
    # the revealed set and the tokens
    check_invariants(x, tok, remain, K)
    reveal = mask & (tok != K)
    ok = ~exs
    assert torch.equal(reveal[ok], r32["reveal"][ok]), "the revealed sets differ"
    pos_ok = ok[:, None] & ~(exc & r64["reveal"])
    assert torch.equal(tok[pos_ok], r32["tokens"][pos_ok]), "%d tokens differ" % int((tok != r32["tokens"])[pos_ok].sum())
    assert torch.equal(tok[reveal], cand[reveal])
    parity_line("purity tail %-40s sharp %.2e (%g d32 = %.2e), candidates / revealed set / tokens equal, %d + %d excused"
                % (I.case_id(c), err, I.TOL_MULT, I.TOL_MULT * d_sharp, int(exc.sum()), int(exs.sum())))
    # padded rows: the same logits at lrows > L (the denoiser's 272-row layout; 8 rows for the one-column grid)
    rc, tok_p, sharp_p, key_p, cand_p = tail(d, lrows=272 if n == L else 8)
    assert rc == 0 and torch.equal(tok_p.cpu(), tok) and torch.equal(sharp_p.cpu(), sharp) and torch.equal(key_p.cpu(), key)
    # the _rng entry == the caller-uniform entry fed with the host mirror of the Philox stream, bit for bit
    ids = [7, 123456, 2 ** 31 + 5]
    gids = torch.tensor(ids, dtype=torch.long, device="cuda")
    rc, a, sharp_a, key_a, cand_a = tail(d, gids=gids, call=11)
    assert rc == 0
    rc, b, sharp_b, key_b, cand_b = tail(d, u=shard.caption_uniforms(ids, 11, K, n, SEED))
    assert rc == 0 and torch.equal(a, b) and torch.equal(key_a, key_b) and torch.equal(cand_a, cand_b)
    assert torch.equal(sharp_a, sharp_b)
    check_invariants(x, a.cpu(), remain, K)


# ---- 2. weight 0 is the plain tails' truncated prediction, bit for bit ---------------------------------------------------------------
def sched_table(K, T=100):
    s = O.make_schedule(T, K + 1)
    tab = torch.zeros(8, T + 1)
    for i, name in enumerate(("log_at", "log_bt", "log_ct", "log_1_min_ct")):
        tab[i, :T] = s[name]
    for i, name in enumerate(("log_cumprod_at", "log_cumprod_bt", "log_cumprod_ct", "log_1_min_cumprod_ct")):
        tab[4 + i] = s[name]
    return tab.cuda()


@pytest.mark.parametrize("c", [c for c in I.TAIL_CASES if c[1] == L and c[4] == 0.0 and c[2] == "ordinary"], ids=I.case_id)
def test_weight_zero_is_the_plain_tails_truncation(c):
    d = I.tail_case(c)
    K, x = d["K"], d["x"].cuda()
    rc, _, sharp, _, _ = tail(d)
    assert rc == 0
    t = torch.full((I.B,), 50, dtype=torch.long, device="cuda")
    u, z, out = d["u"].cuda(), rows(d["z"], L), torch.empty_like(x)
    trunc = torch.empty(I.B, K + 1, L, device="cuda")
    lib = _lib.lib()
    if d["zu"] is None:
        rc = lib.ds_sample_tail_ex(_lib.ptr(z), _lib.ptr(x), _lib.ptr(t), _lib.ptr(u), _lib.ptr(sched_table(K)), _lib.ptr(out),
                                   None, _lib.ptr(trunc), None, I.B, L, K, 100, 0, d["trunc_r"], d["trunc_k"], _lib.stream())
    else:
        zu = rows(d["zu"], L)
        rc = lib.ds_sample_tail_guided(_lib.ptr(z), _lib.ptr(zu), _lib.ptr(x), _lib.ptr(t), _lib.ptr(u),
                                       _lib.ptr(sched_table(K)), _lib.ptr(out), None, _lib.ptr(trunc), None, I.B, L, K, 100, 0,
                                       d["trunc_r"], d["trunc_k"], d["scale"], None, None, 0, _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(sharp, trunc), "weight 0: dbg_sharp is not the plain tail's truncated prediction"


# ---- 3. the exact invariants over states and targets; 4. batch independence ------------------------------------------------------
@pytest.mark.parametrize("K", [256, 512])
@pytest.mark.parametrize("n", [L, 5])
def test_exact_invariants_over_states_and_targets(K, n):
    d = I.tail_case((K, n, "ordinary", "r", 1.0, False))
    g = torch.Generator().manual_seed(K + n)
    gids = torch.tensor([3, 99, 70000], dtype=torch.long, device="cuda")
    free = torch.randint(0, K, (I.B, n), generator=g)
    states = {"mixed": d["x"], "all [MASK]": torch.full((I.B, n), K), "no [MASK]": free}
    one = free.clone()
    one[0, n - 1] = K                                   # a single [MASK], in the column the dead waves shadow
    one[2, 0] = K
    states["one [MASK]"] = one
    for name, x in states.items():
        m = (x == K).sum(1)
        for remain in sorted({0, 1, int(m.max()) // 2, int(m.max()) - 1, int(m.max()), n, 10 * n} - {-1}):
            rc, out, _, _, _ = tail(d, gids=gids, call=2, x=x, remain=remain, dumps=False)
            assert rc == 0, (name, remain)
            check_invariants(x, out.cpu(), remain, K)
    # a chain of single steps over decreasing targets ends without [MASK] and never touches a revealed token
    x = states["all [MASK]"]
    for call, remain in enumerate([(3 * n) // 4, n // 2, n // 4, 0]):
        rc, out, _, _, _ = tail(d, gids=gids, call=call, x=x, remain=remain, dumps=False)
        check_invariants(x, out.cpu(), remain, K)
        x = out.cpu()
    assert not bool((x == K).any())


@pytest.mark.parametrize("guided", [False, True])
def test_a_sample_does_not_depend_on_its_batch_position(guided):
    d = I.tail_case((256, L, "ordinary", "r", 1.0, guided))
    ids = torch.tensor([40, 1000, 7])
    perm = [2, 0, 1]
    rc, a, _, key_a, _ = tail(d, gids=ids.cuda(), call=4)
    dp = dict(d, x=d["x"][perm], z=d["z"][perm], zu=None if d["zu"] is None else d["zu"][perm])
    rc2, b, _, key_b, _ = tail(dp, gids=ids[perm].cuda(), call=4)
    assert rc == 0 and rc2 == 0 and torch.equal(a[perm], b) and torch.equal(key_a[perm], key_b)
    rc1, one, _, _, _ = tail(dict(d, x=d["x"][1:2], z=d["z"][1:2], zu=None if d["zu"] is None else d["zu"][1:2]),
                             gids=ids[1:2].cuda(), call=4)
    assert rc1 == 0 and torch.equal(one[0], a[1])


# ---- 5. argument checks -------------------------------------------------------------------------------------------------------------
def test_tail_argument_checks():
    d = I.tail_case((256, L, "ordinary", "r", 1.0, True))
    lib = _lib.lib()
    bad = [tail(d, remain=-1), tail(d, weight=-0.5), tail(d, weight=float("nan")), tail(d, weight=float("inf")),
           tail(d, scale=float("nan")), tail(d, trunc=(0.85, 10)), tail(d, trunc=(-1.0, -3)), tail(d, claim_lrows=L - 1),
           tail(d, K=300), tail(d, scratch=None)]
    for rc, out, sharp, _, _ in bad:
        assert rc == -1 and bool((out == -1).all()) and bool(torch.isnan(sharp).all())
        assert b"ds_sample_tail_purity" in lib.ds_last_error_string()
    assert tail(d, scale=float("nan"), guided=False)[0] == 0            # the scale is not read without logits_u
    assert int(lib.ds_purity_scratch_bytes(0, L)) == -1 and int(lib.ds_purity_scratch_bytes(64, L)) == 64 * L * 8
    gids = torch.arange(3, device="cuda")
    rc, out, _, _, _ = tail(d, gids=gids, remain=-1)
    assert rc == -1 and bool((out == -1).all()) and b"ds_sample_tail_purity_rng" in lib.ds_last_error_string()


# ---- 6. chains -----------------------------------------------------------------------------------------------------------------------
def build(n_layer=2, T=10, mode="f16x2"):
    from text_to_sound_synthesis_amd.config import build_model, default_config
    m = build_model(default_config(n_layer=n_layer, diffusion_step=T, n_embed=256))
    sd = dict(synth_sd("dalle", n_layer))
    if T != 100:
        sd = {k: (v[:T] if k.endswith(("ln1.emb.weight", "ln1_1.emb.weight")) else v) for k, v in sd.items()}
    m.load_state_dict(sd, strict=False)
    m.transformer.transformer.precision = mode
    m = m.cuda().eval()
    m.transformer.truncation_r = I.TRUNC_R
    return m


_MODEL = {}


def model():
    if "m" not in _MODEL:
        _MODEL["m"] = build()
    return _MODEL["m"]


def philox_u(ids, call, K=256):
    gids = torch.tensor(list(ids), dtype=torch.long, device="cuda")
    u = torch.empty(len(ids), K + 1, L, device="cuda")
    _lib.check(_lib.lib().ds_philox_uniforms(_lib.ptr(gids), I.CHAIN_SEED, call, 0, _lib.ptr(u), len(ids), L, K, _lib.stream()))
    return u


def stepped_chain(dt, name):
    """the chain as S single ds_denoiser_step_purity_rng calls -> the tokens after every call"""
    c = I.CHAINS[name]
    cond, null, known, keep = [v.cuda() for v in I.chain_inputs(name)]
    B = cond.shape[0]
    sched = dt._schedule_table()
    tr = dt.transformer
    p = tr.packed(sched)
    if c["guided"]:
        kv, scale, tokens2 = dt._guide_start((null, I.GUIDE_SCALE), cond, sched)
    else:
        kv, scale, tokens2 = tr.condition_kv(cond.contiguous(), sched), 1.0, None
    Bf = 2 * B if c["guided"] else B
    ws = tr.workspace(Bf, sched, 0)
    sc = scratch_for(B, L)
    gids = torch.tensor(list(c["ids"]), dtype=torch.long, device="cuda")
    x = torch.full((B, L), 256, dtype=torch.long, device="cuda")
    if c["held"]:
        x = torch.where(keep, known, x)
    rec = []
    for k, (t_k, r_k) in enumerate(purity_plan(c["S"], L, dt.log_cumprod_ct)):
        t = torch.full((Bf,), t_k, dtype=torch.long, device="cuda")
        out = torch.empty_like(x)
        _lib.check(_lib.lib().ds_denoiser_step_purity_rng(
            p["handle"], _lib.ptr(x), _lib.ptr(t), _lib.ptr(kv), _lib.ptr(gids), I.CHAIN_SEED, k, B, r_k, c["weight"],
            I.TRUNC_R, 0, scale, _lib.ptr(tokens2), _lib.ptr(ws), _lib.ptr(sc), _lib.ptr(out), _lib.stream()))
        rec.append(out)
        x = out
    torch.cuda.synchronize()
    return torch.stack(rec).cpu()


@pytest.mark.parametrize("name", list(I.CHAINS))
def test_chain(name):
    c = I.CHAINS[name]
    want, cand_gap, sel_gap = I.chain_reference(name)
    assert min(cand_gap, sel_gap) >= I.CHAIN_MIN_GAP
    dt = model().transformer
    cond, null, known, keep = [v.cuda() for v in I.chain_inputs(name)]
    kw = dict(condition_token=None, condition_mask=None, condition_embed=cond, steps=c["S"], purity_weight=c["weight"])
    if c["held"]:
        kw.update(content_token=known, keep_mask=keep)
    if c["guided"]:
        kw.update(guidance_scale=I.GUIDE_SCALE, null_condition_embed=null)
    one_call = dt.sample_purity(caption_ids=list(c["ids"]), seed=I.CHAIN_SEED, **kw)["content_token"].cpu()
    rec = stepped_chain(dt, name)
    assert torch.equal(one_call, rec[-1]), "the one-call chain differs from %d single steps" % c["S"]
    n = int((rec != want).sum())
    print("purity chain %s: %d token mismatches over %d calls (yardstick gaps: candidate %.2e, selection %.2e)"
          % (name, n, c["S"], cand_gap, sel_gap))
    parity_line("purity T=10 chain %-15s: %d token mismatches vs purity_loop" % (name, n))
    assert n == 0
    assert not bool((one_call == 256).any())
    if c["held"]:
        assert torch.equal(one_call[keep.cpu()], known.cpu()[keep.cpu()])
    # caller uniforms (ds_denoiser_step_purity): the same chain fed with the stream written out
    by_u = dt.sample_purity(noise_fn=lambda k, shp: philox_u(c["ids"], k), **kw)["content_token"].cpu()
    assert torch.equal(by_u, one_call)


def test_denoiser_entries_reject_before_enqueuing():
    dt = model().transformer
    name = "s4_guided_held"
    cond, null, known, keep = [v.cuda() for v in I.chain_inputs(name)]
    B = 2
    sched = dt._schedule_table()
    tr = dt.transformer
    p = tr.packed(sched)
    kv2, scale, tokens2 = dt._guide_start((null, I.GUIDE_SCALE), cond, sched)
    ws, sc = tr.workspace(2 * B, sched, 0), scratch_for(B, L)
    lib = _lib.lib()
    x = torch.full((B, L), 256, dtype=torch.long, device="cuda")
    tmp = torch.empty_like(x)
    out = torch.full_like(x, -1)
    t2 = torch.full((2 * B,), 5, dtype=torch.long, device="cuda")
    u = torch.rand(B, 257, L, device="cuda")
    gids = torch.arange(B, device="cuda")
    tokens2.fill_(-7)
    import ctypes
    step = lambda remain, w, sc_=scale: lib.ds_denoiser_step_purity(
        p["handle"], _lib.ptr(x), _lib.ptr(t2), _lib.ptr(kv2), _lib.ptr(u), B, remain, w, 0.85, 0, sc_, _lib.ptr(tokens2),
        _lib.ptr(ws), _lib.ptr(sc), _lib.ptr(out), _lib.stream())
    step_r = lambda remain, w, sc_=scale: lib.ds_denoiser_step_purity_rng(
        p["handle"], _lib.ptr(x), _lib.ptr(t2), _lib.ptr(kv2), _lib.ptr(gids), SEED, 0, B, remain, w, 0.85, 0, sc_,
        _lib.ptr(tokens2), _lib.ptr(ws), _lib.ptr(sc), _lib.ptr(out), _lib.stream())
    t_steps = torch.full((2, 2 * B), 5, dtype=torch.long, device="cuda")

    def chain(remain, w, sc_=scale):
        return lib.ds_denoiser_sample_purity_rng(
            p["handle"], _lib.ptr(x), _lib.ptr(tmp), _lib.ptr(t_steps), (ctypes.c_int * 2)(100, remain), 2, _lib.ptr(kv2),
            _lib.ptr(gids), SEED, 0, B, w, 0.85, 0, sc_, _lib.ptr(tokens2), _lib.ptr(ws), _lib.ptr(sc), _lib.stream())
    for fn, who in ((step, b"ds_denoiser_step_purity"), (step_r, b"ds_denoiser_step_purity_rng"),
                    (chain, b"ds_denoiser_sample_purity_rng")):
        for args in ((-1, 1.0), (0, -1.0), (0, float("nan")), (0, 1.0, float("inf"))):
            assert fn(*args) == -1 and who in lib.ds_last_error_string()
    torch.cuda.synchronize()
    assert bool((tokens2 == -7).all()) and bool((out == -1).all()) and bool((x == 256).all()), "a rejected call enqueued work"
    assert step(100, 1.0) == 0 and step_r(0, 1.0) == 0
    torch.cuda.synchronize()
    assert bool((tokens2[:B] == x).all()) and bool((tokens2[B:] == x).all()) and not bool((out == 256).any())


# ---- 7. the mini-language and the drivers -----------------------------------------------------------------------------------------
def test_sample_type_runs_the_purity_chain():
    m = model()
    dt = m.transformer
    cond = synth.synth_cond_emb(2, key="purity.cond").cuda()
    saved = dt.truncation_r, dt.truncation_k, m.truncation_forward
    try:
        m.truncation_forward = False
        batch = {"condition_embed_token": cond, "caption_ids": [5, 6], "seed": 9}
        a = m.generate_content(batch=batch, filter_ratio=0, sample_type="top0.85r,purity4w1")["content_token"]
        want = dt.sample_purity(condition_token=None, condition_mask=None, condition_embed=cond, steps=4, purity_weight=1.0,
                                caption_ids=[5, 6], seed=9)["content_token"]
        assert torch.equal(a, want) and not bool((a == 256).any())
        b = m.generate_content(batch=batch, filter_ratio=0, sample_type="top0.85r,purity10")["content_token"]
        assert not bool((b == 256).any()) and not torch.equal(a, b)
        known = synth.synth_tokens(2, mask_frac=0.0, key="purity.known").cuda()
        keep = torch.zeros(2, L, dtype=torch.bool, device="cuda")
        keep[:, 40:120] = True
        h = m.inpaint_content(batch=dict(batch, content_token=known), keep_mask=keep, sample_type="top0.85r,purity4")
        assert torch.equal(h["content_token"][keep], known[keep]) and not bool((h["content_token"] == 256).any())
    finally:
        dt.truncation_r, dt.truncation_k, m.truncation_forward = saved


def test_driver_on_random_weights():
    from text_to_sound_synthesis_amd import pipeline
    from text_to_sound_synthesis_amd.config import default_config
    vocab = os.path.join(GOLDEN, "bpe_closed_vocab_guidance.json")
    ds = pipeline.Diffsound(config=default_config(n_layer=2, diffusion_step=100, with_clip=True, bpe_path=vocab), random_vocoder=True)
    captions = synth.synth_captions(2, seed=4)
    kw = dict(caption_ids=[0, 1], seed=3)
    mel01, wave, tokens = ds.generate_sample_with_condition(captions, purity_steps=8, **kw)
    assert tuple(mel01.shape) == (2, 80, 848) and tuple(wave.shape) == (2, 1, 217088) and tuple(tokens.shape) == (2, 265)
    assert bool(torch.isfinite(wave).all()) and int(tokens.min()) >= 0 and int(tokens.max()) < 256
    plain = ds.generate_sample_with_condition(captions, **kw)
    none = ds.generate_sample_with_condition(captions, purity_steps=None, purity_weight=2.0, **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, none)), "purity_steps=None is not today's path"
    assert not torch.equal(plain[2], tokens)
    sharper = ds.generate_sample_with_condition(captions, purity_steps=8, purity_weight=1.0, **kw)[2]
    assert int(sharper.max()) < 256 and not torch.equal(sharper, tokens)
    with pytest.raises(ValueError):
        ds.generate_sample_with_condition(captions, fast=2, purity_steps=8, **kw)
    with pytest.raises(ValueError):
        ds.generate_sample_with_condition(captions, purity_steps=266, **kw)
