"""Caption tracks on the GPU: the composed sampling tail, the composed step / chain entries and the Python surface.
  * the tail kernels against tests/compose_reference.py on the inputs of tests/compose_inputs.py (whose fairness
    tests/test_compose_host.py asserts): log_pred within 4 x d32 of the float64 yardstick (d32 = the distance between its
    float32 and float64 restatements, computed here), kept sets equal except at cuts within 4e-7 of r (at most 1 column in
    200), post within 5e-5 and tokens equal where the kept sets agree -- the rules of tests/test_hip_guidance.py;
  * one track of constant weight s == ds_sample_tail_guided at scale s, bit for bit; zero-weight tracks are not read;
  * held + composed, argument checks, whole chains against composed_loop (0 mismatches), the one-call Philox chain against
    the stepped path, batch independence, track_* = None == today's path, the long form's windows, drivers, full size once.
GPU only (-m gpu)."""
import pytest
import torch

import compose_inputs as I
from conftest import parity_line, synth_sd
from text_to_sound_synthesis_amd import _lib, pipeline, synth

pytestmark = pytest.mark.gpu
NO_GRAD = True

SEED = (0x5eed << 32) | 20261020
L = 265


def build(n_layer=2, T=10, mode="f16x2", codes=256):
    from text_to_sound_synthesis_amd.config import build_model, default_config
    m = build_model(default_config(n_layer=n_layer, diffusion_step=T, n_embed=codes))
    sd = dict(synth_sd("dalle", n_layer))
    if T != 100:
        sd = {k: (v[:T] if k.endswith(("ln1.emb.weight", "ln1_1.emb.weight")) else v) for k, v in sd.items()}
    if codes == 256:
        m.load_state_dict(sd, strict=False)
    else:
        synth.synth_init_(m, seed=0)
    m.transformer.transformer.precision = mode
    m = m.cuda().eval()
    m.transformer.truncation_r = 0.85
    return m


def philox_u(ids, call, K=256, stream=0, seed=SEED):
    gids = torch.tensor(list(ids), dtype=torch.long, device="cuda")
    u = torch.empty(len(ids), K + 1, L, device="cuda")
    _lib.check(_lib.lib().ds_philox_uniforms(_lib.ptr(gids), seed, call, stream, _lib.ptr(u), len(ids), L, K, _lib.stream()))
    return u


def sample(dt, cond=None, **kw):
    return dt.sample(condition_token=None, condition_mask=None, condition_embed=cond, filter_ratio=0, **kw)["content_token"]


def rows(z):
    """logits [B, K, L] -> the kernel's row-major [B * L][K]"""
    return z.permute(0, 2, 1).reshape(-1, z.shape[1])


def slabs(zt, zu):
    """the composed tail's logits [C + 1][B * L][K] on the device: the tracks, then the null condition"""
    return torch.stack([rows(z) for z in list(zt) + [zu]], 0).contiguous().cuda()


def tail_u(K, c, u, sched, trunc_r, trunc_k, keep=None, known=None, mode=0, dumps=False, zt=None, w="w", n_tracks=None):
    """ds_sample_tail_composed on a case of compose_inputs -> (rc, tokens, {log_pred, trunc, post})"""
    B = c["B"]
    zt = c["zt"] if zt is None else zt
    z = slabs(zt, c["zu"])
    wt = None if w is None else (c["w"] if isinstance(w, str) else w).contiguous().cuda()
    xt, t = c["xt"].cuda(), c["t"].cuda()
    out = torch.full((B, L), -1, dtype=torch.long, device="cuda")
    d = {k: torch.full((B, K + 1, L), -7.0, device="cuda") for k in (("log_pred", "trunc", "post") if dumps else ())}
    rc = _lib.lib().ds_sample_tail_composed(
        _lib.ptr(z), _lib.ptr(xt), _lib.ptr(t), _lib.ptr(u), _lib.ptr(sched), _lib.ptr(out), _lib.ptr(d.get("log_pred")),
        _lib.ptr(d.get("trunc")), _lib.ptr(d.get("post")), B, L, K, I.T_TAIL, c["initial"], trunc_r, trunc_k,
        len(zt) if n_tracks is None else n_tracks, _lib.ptr(wt), _lib.ptr(keep), _lib.ptr(known), mode, _lib.stream())
    torch.cuda.synchronize()
    return rc, out, d


def tail_rng(K, c, gids, call, sched, trunc_r, trunc_k, keep=None, known=None, mode=0, t=None, zt=None, w="w", n_tracks=None):
    B = c["B"]
    zt = c["zt"] if zt is None else zt
    z = slabs(zt, c["zu"])
    wt = None if w is None else (c["w"] if isinstance(w, str) else w).contiguous().cuda()
    xt, t = c["xt"].cuda(), (c["t"] if t is None else t).cuda()
    out = torch.full((B, L), -1, dtype=torch.long, device="cuda")
    rc = _lib.lib().ds_sample_tail_composed_rng(
        _lib.ptr(z), _lib.ptr(xt), _lib.ptr(t), _lib.ptr(gids), SEED, call, _lib.ptr(sched), _lib.ptr(out), B, L, K, I.T_TAIL,
        c["initial"], trunc_r, trunc_k, len(zt) if n_tracks is None else n_tracks, _lib.ptr(wt), _lib.ptr(keep), _lib.ptr(known),
        mode, _lib.stream())
    torch.cuda.synchronize()
    return rc, out


_SCHED = {}


def sched_table(K):
    if K not in _SCHED:
        _SCHED[K] = build(1, T=I.T_TAIL, codes=K).transformer._schedule_table().clone()
    return _SCHED[K]


# ---- 1. the tail kernel against the yardstick ------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 512])
@pytest.mark.parametrize("idx,trunc_k", [(0, None), (1, None), (2, None), (3, None), (4, None), (0, 30)])
def test_tail_kernel_vs_yardstick(K, idx, trunc_k):
    c = I.tail_case(K, idx, trunc_k)
    r32, r64 = c["ref32"], c["ref64"]
    sched = sched_table(K)
    tr, tk = (-1.0, trunc_k) if trunc_k else (I.TRUNC_R, 0)
    rc, tok, d = tail_u(K, c, c["u"].cuda(), sched, tr, tk, dumps=True)
    assert rc == 0, _lib.lib().ds_last_error_string()
    lp, trunc, post, tok = d["log_pred"].cpu(), d["trunc"].cpu(), d["post"].cpu(), tok.cpu()
    d32 = float((r32["log_pred"].double() - r64["log_pred"]).abs().max())
    err = float((lp.double() - r64["log_pred"]).abs().max())
    print("composed tail K=%d case %d%s: log_pred err %.3e vs f64 (d32 %.3e)" % (K, idx, " top-k" if trunc_k else "", err, d32))
    assert err <= 4 * d32, "log_pred %.3e from the float64 yardstick, 4 x d32 = %.3e" % (err, 4 * d32)
    assert bool((lp[:, -1] == -70.0).all())
    same = (I.kept(trunc) == I.kept(r32["trunc"])).all(1)                      # [B, L]: columns whose kept sets agree
    if not bool(same.all()):
        # a differing column must be one whose cut sits within 4e-7 of r (the inclusive mass at the yardstick's last kept
        # rank or the one before it), and such columns may be at most 1 in 200
        assert not trunc_k, "top-k kept sets differ in %d columns" % int((~same).sum())
        srt = torch.sort(r64["log_pred"], dim=1, descending=True).values
        inc = torch.exp(srt).cumsum(1)
        near = ((inc - I.TRUNC_R).abs() < 4e-7).any(1)
        assert bool(near[~same].all()), "kept sets differ in columns whose cut is not within 4e-7 of r"
        assert int((~same).sum()) * 200 <= same.numel()
    sel = same[:, None, :].expand_as(trunc)
    kept_vals = torch.where(torch.cat((I.kept(trunc), torch.zeros_like(same)[:, None, :]), 1), lp, torch.full_like(lp, -70.0))
    assert torch.equal(trunc, kept_vals), "the truncated prediction is not log_pred on the kept set and -70 elsewhere"
    if idx == 4:
        assert float(lp[:, :-1].min()) == -70.0          # the clamp case reaches the clamp; log_pred and kept sets only
        return
    perr = float((post - r32["post"])[sel].abs().max())
    print("composed tail K=%d case %d: post err %.3e, %d excused columns" % (K, idx, perr, int((~same).sum())))
    assert perr <= 5e-5, "post %.3e" % perr
    assert torch.equal(tok[same], r32["tokens"][same]), "%d tokens differ" % int((tok != r32["tokens"])[same].sum())
    parity_line("composed tail K=%d case %d%s: log_pred %.2e (4 d32 = %.2e), post %.2e, tokens equal, %d excused columns"
                % (K, idx, " top-k" if trunc_k else "", err, 4 * d32, perr, int((~same).sum())))
    # the _rng entry == the u entry fed with the stream ds_philox_uniforms writes out, bit for bit
    ids = [7, 123456, 2 ** 31 + 5][:c["B"]]
    gids = torch.tensor(ids, dtype=torch.long, device="cuda")
    rc, a = tail_rng(K, c, gids, 11, sched, tr, tk)
    assert rc == 0
    rc, b, _ = tail_u(K, c, philox_u(ids, 11, K), sched, tr, tk)
    assert rc == 0 and torch.equal(a, b)


# ---- 2. one track of constant weight s is the guided tail at scale s, bit for bit -------------------------------------------
@pytest.mark.parametrize("K", [256, 512])
def test_one_constant_track_is_the_guided_tail_bit_for_bit(K):
    lib, sched = _lib.lib(), sched_table(K)
    for idx, s in ((0, 3.0), (1, 7.5), (2, 0.0), (3, 1.5), (4, 7.5), (0, -1.0)):
        c = I.tail_case(K, idx)
        B = c["B"]
        zc, zu = c["zt"][0], c["zu"]
        w = torch.full((B, 1, L), s)
        u = c["u"].cuda()
        rc, tok, d = tail_u(K, c, u, sched, I.TRUNC_R, 0, dumps=True, zt=[zc], w=w)
        assert rc == 0, lib.ds_last_error_string()
        zc_, zu_ = rows(zc).contiguous().cuda(), rows(zu).contiguous().cuda()
        xt, t = c["xt"].cuda(), c["t"].cuda()
        gtok = torch.full((B, L), -1, dtype=torch.long, device="cuda")
        g = {k: torch.full((B, K + 1, L), -7.0, device="cuda") for k in ("log_pred", "trunc", "post")}
        assert lib.ds_sample_tail_guided(
            _lib.ptr(zc_), _lib.ptr(zu_), _lib.ptr(xt), _lib.ptr(t), _lib.ptr(u), _lib.ptr(sched), _lib.ptr(gtok),
            _lib.ptr(g["log_pred"]), _lib.ptr(g["trunc"]), _lib.ptr(g["post"]), B, L, K, I.T_TAIL, c["initial"], I.TRUNC_R, 0, s,
            None, None, 0, _lib.stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(tok, gtok), (idx, s)
        for k in g:
            assert torch.equal(d[k].view(torch.int32), g[k].view(torch.int32)), "%s differs in bits (case %d, s = %g)" % (k, idx, s)
        ids = [7, 123456, 2 ** 31 + 5][:B]
        gids = torch.tensor(ids, dtype=torch.long, device="cuda")
        rc, a = tail_rng(K, c, gids, 4, sched, I.TRUNC_R, 0, zt=[zc], w=w)
        gr = torch.full((B, L), -1, dtype=torch.long, device="cuda")
        assert rc == 0 and lib.ds_sample_tail_guided_rng(
            _lib.ptr(zc_), _lib.ptr(zu_), _lib.ptr(xt), _lib.ptr(t), _lib.ptr(gids), SEED, 4, _lib.ptr(sched), _lib.ptr(gr), B, L, K,
            I.T_TAIL, c["initial"], I.TRUNC_R, 0, s, None, None, 0, _lib.stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(a, gr), (idx, s)


# ---- 3. zero-weight tracks are not read ------------------------------------------------------------------------------------
def _same(a, b):
    return torch.equal(a[1], b[1]) and all(torch.equal(a[2][k].view(torch.int32), b[2][k].view(torch.int32)) for k in a[2])


@pytest.mark.parametrize("K", [256, 512])
def test_zero_weight_tracks_are_not_read(K):
    sched = sched_table(K)
    for idx in (0, 1):                                                         # ramps (C = 2) and mixed (C = 4)
        c = I.tail_case(K, idx)
        u = c["u"].cuda()
        base = tail_u(K, c, u, sched, I.TRUNC_R, 0, dumps=True)
        assert base[0] == 0
        # NaN wherever a track's weight is 0: the same bits
        holes = [torch.where((c["w"][:, i] == 0)[:, None, :], torch.full_like(z, float("nan")), z) for i, z in enumerate(c["zt"])]
        assert any(bool(torch.isnan(h).any()) for h in holes)
        got = tail_u(K, c, u, sched, I.TRUNC_R, 0, dumps=True, zt=holes)
        assert got[0] == 0 and _same(got, base), "a zero-weight track was read (case %d)" % idx
        assert not bool(torch.isnan(got[2]["log_pred"]).any())
    # the mixed case's last track is 0 everywhere: the call without it (C = 3) gives the same bits, and so does appending an
    # all-zero track of NaN logits to a C - 1 call
    c = I.tail_case(K, 1)
    u = c["u"].cuda()
    assert bool((c["w"][:, 3] == 0).all())
    full = tail_u(K, c, u, sched, I.TRUNC_R, 0, dumps=True)
    less = tail_u(K, c, u, sched, I.TRUNC_R, 0, dumps=True, zt=c["zt"][:3], w=c["w"][:, :3])
    assert less[0] == 0 and _same(full, less)
    c2 = I.tail_case(K, 3)                                                     # constant, C = 2
    u2 = c2["u"].cuda()
    two = tail_u(K, c2, u2, sched, I.TRUNC_R, 0, dumps=True)
    nan = torch.full_like(c2["zu"], float("nan"))
    for at in (0, 1, 2):                                                       # the zero track first, in the middle, last
        zt = list(c2["zt"])
        zt.insert(at, nan)
        w3 = torch.cat((c2["w"][:, :at], torch.zeros(c2["B"], 1, L), c2["w"][:, at:]), 1)
        three = tail_u(K, c2, u2, sched, I.TRUNC_R, 0, dumps=True, zt=zt, w=w3)
        assert three[0] == 0 and _same(two, three), "an appended all-zero track changed the result (slot %d)" % at


# ---- 4. held + composed; argument checks -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 512])
def test_held_composed_and_argument_checks(K):
    c = I.tail_case(K, 0)
    B, sched = c["B"], sched_table(K)
    g = torch.Generator().manual_seed(K + 3)
    known = torch.randint(0, K, (B, L), generator=g).cuda()
    some = (torch.rand(B, L, generator=g) < 0.4).to(torch.uint8).cuda()
    some[-1, -1] = 1                                                            # the column the dead waves shadow
    ids = [3, 99, 70000][:B]
    gids = torch.tensor(ids, dtype=torch.long, device="cuda")
    u = c["u"].cuda()
    call, tr = 5, I.TRUNC_R
    _, base_u, _ = tail_u(K, c, u, sched, tr, 0)
    _, base_r = tail_rng(K, c, gids, call, sched, tr, 0)
    assert torch.equal(base_u.cpu(), c["ref32"]["tokens"])                      # free columns: the unheld yardstick
    for keep in (some, torch.zeros_like(some), torch.ones_like(some)):
        kb = keep.bool()
        rc, out, _ = tail_u(K, c, u, sched, tr, 0, keep=keep, known=known)
        assert rc == 0 and torch.equal(out[kb], known[kb]) and torch.equal(out[~kb], base_u[~kb])
        rc, out = tail_rng(K, c, gids, call, sched, tr, 0, keep=keep, known=known)
        assert rc == 0 and torch.equal(out[kb], known[kb]) and torch.equal(out[~kb], base_r[~kb])
    # argument checks: -1, the message names the entry, nothing is launched (the output and the dumps keep their fill)
    lib = _lib.lib()
    w5 = torch.ones(B, 5, L)
    for kw, word in ((dict(n_tracks=0), b"n_tracks"), (dict(n_tracks=5, w=w5), b"n_tracks"), (dict(n_tracks=-1), b"n_tracks"),
                     (dict(w=None), b"weights"), (dict(keep=some, known=known, mode=2), b"mode"),
                     (dict(keep=some, known=known, mode=1), b"renoise"), (dict(keep=some), b"known"),
                     (dict(trunc_k=30), b"exclusive")):
        tk = kw.pop("trunc_k", 0)
        rc, out, d = tail_u(K, c, u, sched, tr, tk, dumps=True, **kw)
        msg = lib.ds_last_error_string()
        assert rc == -1 and bool((out == -1).all()) and all(bool((v == -7.0).all()) for v in d.values())
        assert b"ds_sample_tail_composed:" in msg and word in msg, msg
        if word == b"renoise":
            continue                                                            # (the _rng form has renoise)
        rc, out = tail_rng(K, c, gids, call, sched, tr, tk, **kw)
        msg = lib.ds_last_error_string()
        assert rc == -1 and bool((out == -1).all()) and b"ds_sample_tail_composed_rng:" in msg and word in msg, msg


def test_denoiser_entries_reject_before_enqueuing():
    m = build(2, T=10)
    dt = m.transformer
    B, C = 2, 2
    conds, null, w, known, keep = [v.cuda() for v in I.chain_inputs()]
    sched = dt._schedule_table()
    kvn, _, tokens_n, wd, n = dt._guide_start((null, w.contiguous(), conds), conds[0], sched)
    assert n == C and tuple(tokens_n.shape) == ((C + 1) * B, L)
    lib, p = _lib.lib(), dt.transformer.packed(sched)
    ws = dt.transformer.workspace((C + 1) * B, sched, 0)
    x = torch.full((B, L), 256, dtype=torch.long, device="cuda")
    tn = torch.full(((C + 1) * B,), 5, dtype=torch.long, device="cuda")
    u = torch.rand(B, 257, L, device="cuda")
    gids = torch.arange(B, device="cuda")
    k8 = keep.to(torch.uint8).contiguous()
    tokens_n.fill_(-7)
    out = torch.full_like(x, -1)
    step = lambda nt, wt, kp, kn, md: lib.ds_denoiser_step_composed(
        p["handle"], _lib.ptr(x), _lib.ptr(tn), None, _lib.ptr(kvn), _lib.ptr(u), B, 0, 0.85, 0, nt, _lib.ptr(wt), _lib.ptr(kp),
        _lib.ptr(kn), md, _lib.ptr(tokens_n), _lib.ptr(ws), _lib.ptr(out), _lib.stream())
    step_r = lambda nt, wt, kp, kn, md: lib.ds_denoiser_step_composed_rng(
        p["handle"], _lib.ptr(x), _lib.ptr(tn), None, _lib.ptr(kvn), _lib.ptr(gids), SEED, 0, B, 0, 0.85, 0, nt, _lib.ptr(wt),
        _lib.ptr(kp), _lib.ptr(kn), md, _lib.ptr(tokens_n), _lib.ptr(ws), _lib.ptr(out), _lib.stream())
    tmp = torch.empty_like(x)
    t_steps = torch.zeros(1, 2, (C + 1) * B, dtype=torch.long, device="cuda")
    chain = lambda nt, wt, kp, kn, md: lib.ds_denoiser_sample_composed_rng(
        p["handle"], _lib.ptr(x), _lib.ptr(tmp), _lib.ptr(t_steps), 1, _lib.ptr(kvn), _lib.ptr(gids), SEED, 0, B, 0, 0.85, 0, nt,
        _lib.ptr(wt), _lib.ptr(kp), _lib.ptr(kn), md, _lib.ptr(tokens_n), _lib.ptr(ws), _lib.stream())
    for fn, name in ((step, b"ds_denoiser_step_composed"), (step_r, b"ds_denoiser_step_composed_rng"),
                     (chain, b"ds_denoiser_sample_composed_rng")):
        for args in ((0, wd, None, None, 0), (5, wd, None, None, 0), (C, None, None, None, 0), (C, wd, k8, known, 3),
                     (C, wd, k8, None, 0)):
            assert fn(*args) == -1 and name + b":" in lib.ds_last_error_string(), (name, args)
    assert step(C, wd, k8, known, 1) == -1                # renoise on caller uniforms
    torch.cuda.synchronize()
    assert bool((tokens_n == -7).all()) and bool((out == -1).all()), "a rejected call enqueued work"
    assert step(C, wd, None, None, 0) == 0 and step_r(C, wd, k8, known, 1) == 0
    torch.cuda.synchronize()
    assert all(bool((tokens_n[i * B:(i + 1) * B] == x).all()) for i in range(C + 1))


# ---- 5. chains against composed_loop ---------------------------------------------------------------------------------------
def first_difference(name, rec, want):
    for k, got in enumerate(rec):
        d = torch.nonzero(got.cpu() != want[k])
        if d.numel():
            return "%s: %d tokens differ after call %d; first at clip %d position %d (the yardstick's smallest gap of the " \
                   "whole chain: %.3e)" % (name, d.shape[0], k, int(d[0, 0]), int(d[0, 1]), I.chain_reference(name)[1])
    return "%s: every recorded call agrees" % name


@pytest.mark.parametrize("mode", ["f16x2", "fp32"])
@pytest.mark.parametrize("name", list(I.CHAINS))
def test_chain_vs_composed_loop(name, mode):
    want, gap = I.chain_reference(name)
    m = build(2, T=10, mode=mode)
    dt = m.transformer
    conds, null, w, known, keep = [v.cuda() for v in I.chain_inputs()]
    c = I.CHAINS[name]
    order = {t: k for k, (t, _) in enumerate(I.R.chain_steps(I.T_CHAIN, c["skip_step"]))}
    noise = I.chain_noise(name)
    rec, inner = [], dt.p_sample_tokens

    def spy(*a, **k):
        out = inner(*a, **k)
        rec.append(out.clone())
        return out
    dt.p_sample_tokens = spy
    try:
        fn = dt.sample_fast if c["skip_step"] else dt.sample
        kw = {"skip_step": c["skip_step"]} if c["skip_step"] else {}
        if c["held"]:
            kw.update(content_token=known, keep_mask=keep)
        tok = fn(condition_token=None, condition_mask=None, condition_embed=None, filter_ratio=0,
                 noise_fn=lambda t, shp: noise(order[t], shp), track_embed=conds, track_weight=w, null_condition_embed=null[0],
                 **kw)["content_token"]
    finally:
        del dt.p_sample_tokens
    n = int((tok.cpu() != want[-1]).sum())
    print("composed chain %s (%s): %d token mismatches (yardstick min gap %.2e)" % (name, mode, n, gap))
    parity_line("composed T=10 chain %-7s %-5s: %d token mismatches vs composed_loop" % (name, mode, n))
    assert n == 0, first_difference(name, rec, want)
    assert len(rec) == want.shape[0] and torch.equal(torch.stack(rec).cpu(), want)
    if c["held"]:
        assert torch.equal(tok[keep], known[keep])


def _scene_inputs(B, key):
    conds = torch.stack([synth.synth_cond_emb(B, key="%s.c%d" % (key, i)) for i in range(2)], 0).cuda()
    null = synth.synth_cond_emb(1, key="comp.null")[0].cuda()
    scenes = [[("a", 0.0, None, 3.0), ("b", 2.9, 6.2, 3.0)], [("a", 0.0, 4.0, 2.0), ("b", 5.0, None, 3.0)],
              [("a", 1.0, 7.0, 2.5), ("b", 3.3, 4.4, -1.0)]]
    return conds, null, pipeline.track_weights(scenes[:B], 53)[1].cuda()


def test_one_call_philox_chain_equals_the_stepped_path():
    m = build(2, T=10)
    dt = m.transformer
    B, ids = 3, [12, 500, 13]
    conds, null, w = _scene_inputs(B, "comp.p")
    known = synth.synth_tokens(B, mask_frac=0.0, key="comp.p.known").cuda()
    keep = torch.zeros(B, L, dtype=torch.bool, device="cuda")
    keep[:, 40:120] = True
    g = dict(track_embed=conds, track_weight=w, null_condition_embed=null)
    stepped = []
    dt.p_sample_tokens = lambda *a, **k: stepped.append(1)           # the chain must not come back to Python between steps
    try:
        a = sample(dt, caption_ids=ids, seed=SEED, **g)
    finally:
        del dt.p_sample_tokens
    assert not stepped
    b = sample(dt, noise_fn=lambda t, shp: philox_u(ids, 9 - t), **g)
    assert torch.equal(a, b) and int(a.max()) < 256
    assert not torch.equal(a, sample(dt, conds[0], caption_ids=ids, seed=SEED))
    order = {9: 0, 6: 1, 3: 2, 0: 3}
    fkw = dict(condition_token=None, condition_mask=None, condition_embed=None, filter_ratio=0, skip_step=2, **g)
    assert torch.equal(dt.sample_fast(caption_ids=ids, seed=SEED, **fkw)["content_token"],
                       dt.sample_fast(noise_fn=lambda t, shp: philox_u(ids, order[t]), **fkw)["content_token"])
    # region-held, both keep modes
    hk = dict(content_token=known, keep_mask=keep, **g)
    ha = sample(dt, caption_ids=ids, seed=SEED, **hk)
    hb = sample(dt, noise_fn=lambda t, shp: philox_u(ids, 9 - t), **hk)
    assert torch.equal(ha, hb) and torch.equal(ha[keep], known[keep]) and not torch.equal(ha, a)
    hr = sample(dt, caption_ids=ids, seed=SEED, keep_mode="renoise", **hk)
    assert torch.equal(hr[keep], known[keep]) and not torch.equal(hr, ha)
    # one track of constant weight: the guided chain
    one = dict(track_embed=conds[:1], track_weight=torch.full((B, 1, L), 3.0, device="cuda"), null_condition_embed=null)
    assert torch.equal(sample(dt, caption_ids=ids, seed=SEED, **one),
                       sample(dt, conds[0], caption_ids=ids, seed=SEED, guidance_scale=3.0, null_condition_embed=null))


def test_a_scene_alone_equals_the_scene_in_a_batch():
    m = build(2, T=10)
    dt = m.transformer
    ids = torch.tensor([40, 1000, 7])
    conds, null, w = _scene_inputs(3, "comp.b")
    run = lambda sel: sample(dt, caption_ids=ids[sel], seed=SEED, track_embed=conds[:, sel].contiguous(),
                             track_weight=w[sel].contiguous(), null_condition_embed=null).cpu()
    whole = run([0, 1, 2])
    for i in range(3):
        assert torch.equal(run([i])[0], whole[i]), "scene %d alone differs from the batch of 3" % i


# ---- 6. the Python surface -------------------------------------------------------------------------------------------------
def test_no_tracks_is_the_path_as_it_was():
    m = build(2, T=10)
    dt = m.transformer
    ids = [4, 5]
    conds, null, w = _scene_inputs(2, "comp.n")
    cond = conds[0]
    lib = _lib.lib()
    called = []

    class Spy:
        def __getattr__(self, name):
            if "composed" in name:
                called.append(name)
            return getattr(lib, name)
    plain_p = sample(dt, cond, caption_ids=ids, seed=SEED)
    guided_p = sample(dt, cond, caption_ids=ids, seed=SEED, guidance_scale=2.0, null_condition_embed=null)
    nf = lambda t, shp: philox_u(ids, 9 - t)
    plain_u = sample(dt, cond, noise_fn=nf)
    real = _lib.lib
    _lib.lib = lambda: Spy()
    try:
        kw = dict(track_embed=None, track_weight=None)
        assert torch.equal(sample(dt, cond, caption_ids=ids, seed=SEED, **kw), plain_p)
        assert torch.equal(sample(dt, cond, noise_fn=nf, **kw), plain_u)
        assert torch.equal(sample(dt, cond, caption_ids=ids, seed=SEED, guidance_scale=2.0, null_condition_embed=null, **kw), guided_p)
        assert not called
        sample(dt, caption_ids=ids, seed=SEED, track_embed=conds, track_weight=w, null_condition_embed=null)
        assert called == ["ds_denoiser_sample_composed_rng"]
    finally:
        _lib.lib = real


def test_long_form_windows_are_inpaint_content_under_the_sliced_weights():
    m = build(2, T=10)
    B, n, ids = 2, 13, [7, 300000]
    total = 53 + (53 - n)
    conds = torch.stack([synth.synth_cond_emb(B, key="comp.l.c%d" % i) for i in range(2)], 0).cuda()
    null = synth.synth_cond_emb(1, key="comp.null")[0].cuda()
    w = pipeline.track_weights([("a", 0.0, None, 3.0), ("b", 9.0, 12.5, 3.0)], total, batch=B)[1]
    batch = {"null_condition_embed_token": null, "caption_ids": ids, "seed": SEED}
    tok = m.generate_long_content(batch=batch, windows=2, overlap_cols=n, tracks={"embed": conds, "weight": w})["content_token"]
    assert tuple(tok.shape) == (B, 2, L) and int(tok.max()) < 256 and torch.equal(tok[:, 1, :5 * n], tok[:, 0, L - 5 * n:])
    assert m.transformer.truncation_r == 0.85 and not m.truncation_forward
    keep_tf = m.truncation_forward
    try:
        m.truncation_forward = True
        w0 = m.generate_content(batch=batch, filter_ratio=0, content_ratio=1, sample_type="top0.85r",
                                tracks={"embed": conds, "weight": w[:, :, :L].contiguous()})["content_token"]
        assert torch.equal(tok[:, 0], w0), "window 0 is not generate_content's clip under the first 53 columns' weights"
        known, keep = pipeline.continuation_tokens(tok[:, 0], n)
        c0 = 53 - n
        direct = m.inpaint_content(batch=dict(batch, content_token=known, caption_ids=pipeline.window_caption_ids(ids, 1)),
                                   keep_mask=keep, sample_type="top0.85r",
                                   tracks={"embed": conds, "weight": w[:, :, 5 * c0:5 * (c0 + 53)].contiguous()})["content_token"]
        assert torch.equal(tok[:, 1], direct), "window 1 is not inpaint_content under the sliced weights"
        # ... and the slice matters: under window 0's weights the window differs
        other = m.inpaint_content(batch=dict(batch, content_token=known, caption_ids=pipeline.window_caption_ids(ids, 1)),
                                  keep_mask=keep, sample_type="top0.85r",
                                  tracks={"embed": conds, "weight": w[:, :, :L].contiguous()})["content_token"]
        assert not torch.equal(other, direct)
    finally:
        m.truncation_forward = keep_tf


@pytest.fixture(scope="module")
def ds():
    from text_to_sound_synthesis_amd import tokenizer as tz
    from text_to_sound_synthesis_amd.config import default_config
    return pipeline.Diffsound(config=default_config(n_layer=2, diffusion_step=10, with_clip=True, bpe_path=tz.CLOSED_VOCAB_PATH),
                              random_vocoder=True)


def test_generate_scene_and_inpaint_scene(ds):
    caps = synth.synth_captions(3, seed=4)
    scene = [(caps[0], 0, None), (caps[1], 3.0, 4.5, 2.0), (caps[2], 7.0, 8.0, -1.0)]
    # one window
    mel01, wave, tokens = ds.generate_scene(scene, caption_ids=[5], seed=3)
    assert tuple(tokens.shape) == (1, 1, L) and tuple(mel01.shape) == (1, 80, 848) and tuple(wave.shape) == (1, 1, 217088)
    assert bool(torch.isfinite(wave).all()) and bool(torch.isfinite(mel01).all()) and 0 <= int(tokens.min()) and int(tokens.max()) < 256
    assert torch.equal(ds.generate_scene(scene, caption_ids=[5], seed=3)[2], tokens)
    assert not torch.equal(ds.generate_scene(scene, caption_ids=[5], seed=3, scale=1.0)[2], tokens)     # the default scale is used
    assert not torch.equal(ds.generate_scene(scene[:1], caption_ids=[5], seed=3)[2], tokens)           # ... and so are the tracks
    # ... the tokens of the model-level call on track_weights' output
    text, w = pipeline.track_weights([(caps[0], 0, None, 3.0)] + scene[1:], 53)
    model, dt = ds.model, ds.model.transformer
    keep_state = dt.truncation_r, model.truncation_forward
    try:
        dt.truncation_r, model.truncation_forward = 0.85, True
        want = model.generate_content(batch={"caption_ids": [5], "seed": 3}, filter_ratio=0, content_ratio=1,
                                      tracks={"text": text, "weight": w})["content_token"]
    finally:
        dt.truncation_r, model.truncation_forward = keep_state
    assert torch.equal(tokens[:, 0], want)
    # two windows, a scene per clip: the second window opens with the first one's tail
    scenes = [[(caps[0], 0, None), (caps[1], 11.0, 14.0)], [(caps[2], 2.0, 15.5, 2.0)]]
    windows, n, total, samples = pipeline.long_plan(16.0)
    assert windows == 2
    mel01, wave, tokens = ds.generate_scene(scenes, seconds=16.0, caption_ids=[0, 1], seed=3)
    assert tuple(tokens.shape) == (2, 2, L) and tuple(wave.shape) == (2, 1, samples) and tuple(mel01.shape) == (2, 80, -(-samples // 256))
    assert bool(torch.isfinite(wave).all()) and int(tokens.max()) < 256
    assert torch.equal(tokens[:, 1, :5 * n], tokens[:, 0, L - 5 * n:])
    # inpainting under a scene keeps the held tokens exactly
    g = torch.Generator().manual_seed(33)
    w22 = (0.2 * torch.randn(2, 217088, generator=g)).cuda()
    spans = [[(4.0, 7.0)], [(0.0, 1.5)]]
    keep = pipeline.spans_to_keep_mask(spans, 2, "cuda")
    input_tokens = ds.model.prepare_content({"audio": w22})["content_token"]
    t_in = ds.inpaint_scene(w22, scene, spans, caption_ids=[0, 1], seed=3)[2]
    assert torch.equal(t_in[keep], input_tokens[keep]) and int(t_in.max()) < 256 and not torch.equal(t_in, input_tokens)
    assert not torch.equal(t_in, ds.inpaint_audio(w22, [caps[0]] * 2, spans, caption_ids=[0, 1], seed=3)[2])
    assert not torch.equal(t_in, ds.inpaint_scene(w22, scene, spans, caption_ids=[0, 1], seed=3, scale=1.0)[2])
    with pytest.raises(ValueError):
        ds.inpaint_scene(w22, [("a", 0, 1)] * 5, spans)


# ---- 7. full size, once ----------------------------------------------------------------------------------------------------
def test_full_size_19_layers_100_steps():
    m = build(19, T=100)
    dt = m.transformer
    ids = torch.tensor([300, 301])
    conds, null, w = _scene_inputs(2, "comp.full")
    a = sample(dt, caption_ids=ids, seed=SEED, track_embed=conds, track_weight=w, null_condition_embed=null)
    assert tuple(a.shape) == (2, L) and int(a.min()) >= 0 and int(a.max()) < 256              # in range, no [MASK] left
