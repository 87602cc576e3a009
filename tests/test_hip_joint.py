"""Joint-window sampling on the GPU: the joint sampling tail, the window gather, the joint step / chain entries, the drivers
and seamless loops.
  * the tail kernels against tests/joint_reference.py on the inputs of tests/joint_inputs.py (whose fairness
    tests/test_joint_host.py asserts), under the rules of tests/test_hip_guidance.py: log_pred within 4 x d32 of the float64
    yardstick (d32 = the distance between its float32 twin and its float64 form, computed here), kept sets equal except at
    cuts within 4e-7 of r (at most 1 column in 200), post within 5e-5 and tokens equal where the kept sets agree;
  * bit-equalities with the plain and the guided tail, held canvas positions, argument checks, the gather;
  * whole chains: the one-call chain == the stepped entry == the yardstick's joint_loop (0 mismatches), batch independence,
    fast plans; the drivers; loops; the longest canvas once.
GPU only (-m gpu)."""
import math

import pytest
import torch

import joint_inputs as I
import joint_reference as R
from conftest import parity_line, synth_sd
from text_to_sound_synthesis_amd import _lib, audio, pipeline, synth

pytestmark = pytest.mark.gpu
NO_GRAD = True

SEED = (0x5eed << 32) | 20261021
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


_SCHED = {}


def sched_table(K):
    if K not in _SCHED:
        _SCHED[K] = build(1, T=I.T_TAIL, codes=K).transformer._schedule_table().clone()
    return _SCHED[K]


def philox_u(ids, call, Lc, K=256, seed=SEED):
    gids = torch.tensor(list(ids), dtype=torch.long, device="cuda")
    u = torch.empty(len(ids), K + 1, Lc, device="cuda")
    _lib.check(_lib.lib().ds_philox_uniforms(_lib.ptr(gids), seed, call, 0, _lib.ptr(u), len(ids), Lc, K, _lib.stream()))
    return u


def win_rows(z):
    """window logits [B, W, K, 265] -> the kernel's [B W 265][K] on the device"""
    return z.permute(0, 1, 3, 2).reshape(-1, z.shape[2]).contiguous().cuda()


def rows(z):
    """logits [B, K, L'] -> row-major [B L'][K] on the device"""
    return z.permute(0, 2, 1).reshape(-1, z.shape[1]).contiguous().cuda()


def fade_dev(n):
    return audio.fade_table(n).cuda()


def joint_tail(K, c, sched, trunc_r, trunc_k, u=None, gids=None, call=0, dumps=False, **over):
    """ds_sample_tail_joint (u) or ds_sample_tail_joint_rng (gids) on a case of joint_inputs -> (rc, canvas, dumps); `over`
    replaces arguments by name"""
    B, W, n, ring, Lc = c["B"], c["W"], c["n"], c["ring"], c["Lc"]
    a = dict(logits=win_rows(c["zc"]), logits_u=None if c["zu"] is None else win_rows(c["zu"]), canvas=c["xt"].cuda(),
             t=c["t"].cuda(), sched=sched, B=B, W=W, n=n, ring=int(ring), fade=fade_dev(n), lrows=L, K=K, T=I.T_TAIL, initial=0,
             trunc_r=trunc_r, trunc_k=trunc_k, scale=c["s"], keep=None, known=None, mode=0)
    a.update(over)
    Lc = over.get("Lc", Lc)
    out = torch.full((a["B"] if a["B"] > 0 else B, Lc), -1, dtype=torch.long, device="cuda")
    d = {k: torch.empty(B, K + 1, Lc, device="cuda") for k in (("log_pred", "trunc", "post") if dumps else ())}
    head = [_lib.ptr(a["logits"]), _lib.ptr(a["logits_u"]), _lib.ptr(a["canvas"]), _lib.ptr(a["t"])]
    geo = [a["B"], a["W"], a["n"], a["ring"], _lib.ptr(a["fade"]), a["lrows"], a["K"], a["T"], a["initial"], a["trunc_r"],
           a["trunc_k"], a["scale"], _lib.ptr(a["keep"]), _lib.ptr(a["known"]), a["mode"], _lib.stream()]
    dbg = [_lib.ptr(d.get("log_pred")), _lib.ptr(d.get("trunc")), _lib.ptr(d.get("post"))]
    if gids is None:
        rc = _lib.lib().ds_sample_tail_joint(*head, _lib.ptr(u), _lib.ptr(a["sched"]), _lib.ptr(out), *dbg, *geo)
    else:
        rc = _lib.lib().ds_sample_tail_joint_rng(*head, _lib.ptr(gids), SEED, call, _lib.ptr(a["sched"]), _lib.ptr(out), *dbg, *geo)
    torch.cuda.synchronize()
    return rc, out, d


def trunc_args(trunc_k):
    return (-1.0, trunc_k) if trunc_k else (I.TRUNC_R, 0)


# ---- 1. the tail kernel against the yardstick ------------------------------------------------------------------------------
@pytest.mark.parametrize("K,n,ring,trunc_k,guided", I.TAIL_CASES)
def test_tail_kernel_vs_yardstick(K, n, ring, trunc_k, guided):
    c = I.tail_case(K, n, ring, trunc_k, guided)
    r32, r64 = c["ref32"], c["ref64"]
    sched = sched_table(K)
    tr, tk = trunc_args(trunc_k)
    rc, tok, d = joint_tail(K, c, sched, tr, tk, u=c["u"].cuda(), dumps=True)
    assert rc == 0, _lib.lib().ds_last_error_string()
    lp, trunc, post, tok = d["log_pred"].cpu(), d["trunc"].cpu(), d["post"].cpu(), tok.cpu()
    d32 = float((r32["log_pred"].double() - r64["log_pred"]).abs().max())
    err = float((lp.double() - r64["log_pred"]).abs().max())
    tag = "joint tail K=%d n=%d %s%s%s" % (K, n, "ring" if ring else "line", " top-k" if trunc_k else "", " guided" if guided else "")
    print("%s: log_pred err %.3e vs f64 (d32 %.3e)" % (tag, err, d32))
    assert err <= 4 * d32, "log_pred %.3e from the float64 yardstick, 4 x d32 = %.3e" % (err, 4 * d32)
    assert bool((lp[:, -1] == -70.0).all())
    same = (I.kept(trunc) == I.kept(r32["trunc"])).all(1)                      # [B, Lc]: positions whose kept sets agree
    if not bool(same.all()):
        assert not trunc_k, "top-k kept sets differ in %d columns" % int((~same).sum())
        assert bool(I.near_cut(r64)[~same].all()), "kept sets differ in columns whose cut is not within 4e-7 of r"
        assert int((~same).sum()) * 200 <= same.numel()
    sel = same[:, None, :].expand_as(trunc)
    kept_vals = torch.where(torch.cat((I.kept(trunc), torch.zeros_like(same)[:, None, :]), 1), lp, torch.full_like(lp, -70.0))
    assert torch.equal(trunc, kept_vals), "the truncated prediction is not log_pred on the kept set and -70 elsewhere"
    perr = float((post - r32["post"])[sel].abs().max())
    print("%s: post err %.3e" % (tag, perr))
    assert perr <= 5e-5, "post %.3e" % perr
    assert torch.equal(tok[same], r32["tokens"][same]), "%d tokens differ" % int((tok != r32["tokens"])[same].sum())
    parity_line("%s: log_pred %.2e (4 d32 = %.2e), post %.2e, tokens equal, %d excused columns"
                % (tag, err, 4 * d32, perr, int((~same).sum())))
    # the _rng entry == the u entry fed with the stream ds_philox_uniforms writes out at the canvas length, bit for bit
    ids = [7, 2 ** 31 + 5]
    gids = torch.tensor(ids, dtype=torch.long, device="cuda")
    rc, a, _ = joint_tail(K, c, sched, tr, tk, gids=gids, call=11)
    assert rc == 0
    rc, b, _ = joint_tail(K, c, sched, tr, tk, u=philox_u(ids, 11, c["Lc"], K))
    assert rc == 0 and torch.equal(a, b)


# ---- 2. bit-equalities -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 512])
def test_one_window_line_is_the_plain_and_the_guided_tail(K):
    lib, sched = _lib.lib(), sched_table(K)
    gids = torch.tensor([5, 70000], dtype=torch.long, device="cuda")
    for guided in (False, True):
        c = I.tail_case(K, 13, False, None, guided)
        one = dict(c, W=1, Lc=L, zc=c["zc"][:, :1], zu=None if c["zu"] is None else c["zu"][:, :1], xt=c["xt"][:, :L].contiguous())
        for tr, tk in ((I.TRUNC_R, 0), (-1.0, I.TRUNC_K)):
            rc, got, _ = joint_tail(K, one, sched, tr, tk, gids=gids, call=4)
            assert rc == 0, lib.ds_last_error_string()
            want = torch.full((2, L), -1, dtype=torch.long, device="cuda")
            zc, xt, t = rows(one["zc"][:, 0]), one["xt"].cuda(), c["t"].cuda()
            if guided:
                zu = rows(one["zu"][:, 0])
                rc = lib.ds_sample_tail_guided_rng(_lib.ptr(zc), _lib.ptr(zu), _lib.ptr(xt), _lib.ptr(t), _lib.ptr(gids), SEED, 4,
                                                   _lib.ptr(sched), _lib.ptr(want), 2, L, K, I.T_TAIL, 0, tr, tk, c["s"], None, None,
                                                   0, _lib.stream())
            else:
                rc = lib.ds_sample_tail_rng(_lib.ptr(zc), _lib.ptr(xt), _lib.ptr(t), _lib.ptr(gids), SEED, 4, _lib.ptr(sched),
                                            _lib.ptr(want), 2, L, K, I.T_TAIL, 0, tr, tk, _lib.stream())
            assert rc == 0
            torch.cuda.synchronize()
            assert torch.equal(got, want), "%d tokens differ (guided %s)" % (int((got != want).sum()), guided)


@pytest.mark.parametrize("K", [256, 512])
@pytest.mark.parametrize("n,ring", [(13, True), (26, False), (1, True)])
def test_positions_are_the_guided_and_the_plain_tail_on_their_rows(K, n, ring):
    """A two-window position == ds_sample_tail_guided fed the two windows' rows at scale fade[o]; a one-window position == the
    plain tail on its row; both with the canvas position's uniforms (caller uniforms), dumps included."""
    lib, sched = _lib.lib(), sched_table(K)
    c = I.tail_case(K, n, ring)
    B, W, Lc = c["B"], c["W"], c["Lc"]
    u = c["u"].cuda()
    rc, got, gd = joint_tail(K, c, sched, I.TRUNC_R, 0, u=u, dumps=True)
    assert rc == 0
    cov, fade = R.cover(W, n, ring), R.fade(n)
    # per canvas position the later and the earlier window's logits row (the later one's again under one window)
    later = torch.empty(B, K, Lc)
    earlier = torch.empty(B, K, Lc)
    off = torch.full((Lc,), -1, dtype=torch.long)
    for col, cv in enumerate(cov):
        (w1, o1) = cv[0]
        (w0, o0) = cv[1] if len(cv) == 2 else cv[0]
        later[:, :, 5 * col:5 * col + 5] = c["zc"][:, w1, :, 5 * o1:5 * o1 + 5]
        earlier[:, :, 5 * col:5 * col + 5] = c["zc"][:, w0, :, 5 * o0:5 * o0 + 5]
        if len(cv) == 2:
            off[5 * col:5 * col + 5] = o1
    zl, ze, xt, t = rows(later), rows(earlier), c["xt"].cuda(), c["t"].cuda()

    def dumps():
        return {k: torch.empty(B, K + 1, Lc, device="cuda") for k in ("log_pred", "trunc", "post")}
    want, d = torch.full((B, Lc), -1, dtype=torch.long, device="cuda"), dumps()
    rc = lib.ds_sample_tail_ex(_lib.ptr(zl), _lib.ptr(xt), _lib.ptr(t), _lib.ptr(u), _lib.ptr(sched), _lib.ptr(want),
                               _lib.ptr(d["log_pred"]), _lib.ptr(d["trunc"]), _lib.ptr(d["post"]), B, Lc, K, I.T_TAIL, 0, I.TRUNC_R,
                               0, _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    single = (off < 0).cuda()
    assert int(single.sum()) > 0 and torch.equal(got[:, single], want[:, single])
    for k in d:
        assert torch.equal(gd[k][:, :, single], d[k][:, :, single]), k
    checked = 0
    for o in sorted({0, n // 2, n - 1}):
        want, d = torch.full((B, Lc), -1, dtype=torch.long, device="cuda"), dumps()
        rc = lib.ds_sample_tail_guided(_lib.ptr(zl), _lib.ptr(ze), _lib.ptr(xt), _lib.ptr(t), _lib.ptr(u), _lib.ptr(sched),
                                       _lib.ptr(want), _lib.ptr(d["log_pred"]), _lib.ptr(d["trunc"]), _lib.ptr(d["post"]), B, Lc, K,
                                       I.T_TAIL, 0, I.TRUNC_R, 0, float(fade[o]), None, None, 0, _lib.stream())
        assert rc == 0, lib.ds_last_error_string()
        torch.cuda.synchronize()
        at = (off == o).cuda()
        assert int(at.sum()) == 5 * (W if ring else W - 1)
        assert torch.equal(got[:, at], want[:, at]), "offset %d: %d tokens differ" % (o, int((got != want)[:, at].sum()))
        for k in d:
            assert torch.equal(gd[k][:, :, at], d[k][:, :, at]), (o, k)
        checked += int(at.sum())
    assert checked > 0


@pytest.mark.parametrize("K", [256, 512])
def test_held_canvas_positions_and_keep_all_zero(K):
    sched = sched_table(K)
    for guided in (False, True):
        c = I.tail_case(K, 13, True, None, guided)
        B, W, Lc = c["B"], c["W"], c["Lc"]
        g = torch.Generator().manual_seed(K + 9)
        known = torch.randint(0, K, (B, Lc), generator=g).cuda()
        some = (torch.rand(B, Lc, generator=g) < 0.4)
        some[-1, -1] = True                                                      # the position the dead waves shadow
        gids = torch.tensor([3, 99], dtype=torch.long, device="cuda")
        u = c["u"].cuda()
        _, base_u, _ = joint_tail(K, c, sched, I.TRUNC_R, 0, u=u)
        _, base_r, _ = joint_tail(K, c, sched, I.TRUNC_R, 0, gids=gids, call=5)
        zero = torch.zeros(B, Lc, dtype=torch.uint8, device="cuda")
        rc, out, _ = joint_tail(K, c, sched, I.TRUNC_R, 0, u=u, keep=zero, known=known)
        assert rc == 0 and torch.equal(out, base_u)                              # keep all zero == unheld
        rc, out, _ = joint_tail(K, c, sched, I.TRUNC_R, 0, gids=gids, call=5, keep=zero, known=known)
        assert rc == 0 and torch.equal(out, base_r)
        # held positions come out as known whatever the logits hold there: every window row that covers one is NaN
        pos = R.window_positions(W, 13, True)                                    # [W, 265] canvas positions
        zc = c["zc"].clone()
        zu = None if c["zu"] is None else c["zu"].clone()
        hit = some[:, pos]                                                       # [B, W, 265]
        zc[hit[:, :, None, :].expand_as(zc)] = float("nan")
        if zu is not None:
            zu[hit[:, :, None, :].expand_as(zu)] = float("nan")
        keep = some.to(torch.uint8).cuda()
        kb = some.cuda()
        poisoned = dict(c, zc=zc, zu=zu)
        rc, out, _ = joint_tail(K, poisoned, sched, I.TRUNC_R, 0, u=u, keep=keep, known=known)
        assert rc == 0 and torch.equal(out[kb], known[kb]) and torch.equal(out[~kb], base_u[~kb])
        rc, out, _ = joint_tail(K, poisoned, sched, I.TRUNC_R, 0, gids=gids, call=5, keep=keep, known=known)
        assert rc == 0 and torch.equal(out[kb], known[kb]) and torch.equal(out[~kb], base_r[~kb])
        ones = torch.ones_like(keep)
        rc, out, _ = joint_tail(K, poisoned, sched, I.TRUNC_R, 0, u=u, keep=ones, known=known)
        assert rc == 0 and torch.equal(out, known)


# ---- 4. argument checks ----------------------------------------------------------------------------------------------------
def test_rejected_arguments_write_nothing_and_name_the_entry():
    K = 256
    sched, lib = sched_table(K), _lib.lib()
    c = I.tail_case(K, 13, False, None, True)
    u = c["u"].cuda()
    gids = torch.tensor([1, 2], dtype=torch.long, device="cuda")
    some = torch.ones(c["B"], c["Lc"], dtype=torch.uint8, device="cuda")
    known = torch.zeros(c["B"], c["Lc"], dtype=torch.long, device="cuda")
    bad = [dict(W=0), dict(n=0), dict(n=27), dict(ring=1, W=1), dict(W=300, n=1), dict(lrows=264), dict(mode=1),
           dict(mode=1, keep=some, known=known), dict(keep=some), dict(trunc_k=30), dict(scale=float("nan")),
           dict(scale=float("inf")), dict(fade=None), dict(logits=None), dict(canvas=None), dict(t=None), dict(sched=None)]
    for over in bad:
        over = dict(over)
        tk = over.pop("trunc_k", 0)                                            # (top-k beside top-r 0.85: both truncations)
        sc = over.pop("sched", sched)
        rc, out, _ = joint_tail(K, c, sc, I.TRUNC_R, tk, u=u, **over)
        assert rc == -1 and bool((out == -1).all()), over
        assert b"ds_sample_tail_joint:" in lib.ds_last_error_string(), (over, lib.ds_last_error_string())
        rc, out, _ = joint_tail(K, c, sc, I.TRUNC_R, tk, gids=gids, **over)
        assert rc == -1 and bool((out == -1).all()), over
        assert b"ds_sample_tail_joint_rng:" in lib.ds_last_error_string()
    rc, out, _ = joint_tail(K, c, sched, I.TRUNC_R, 0, u=None)
    assert rc == -1 and bool((out == -1).all()) and b"ds_sample_tail_joint:" in lib.ds_last_error_string()


def test_denoiser_entries_reject_before_enqueuing():
    m = build(2, T=10)
    dt = m.transformer
    B, W, n = 2, 2, 13
    Lc = 5 * pipeline.joint_canvas_cols(W, n)
    sched = dt._schedule_table()
    cond = synth.synth_cond_emb(B, key="joint.rej.cond").cuda()
    kv = dt.transformer.condition_kv(cond.repeat_interleave(W, 0).repeat(2, 1, 1).contiguous(), sched)
    lib, p = _lib.lib(), dt.transformer.packed(sched)
    Bf = 2 * B * W
    ws = dt.transformer.workspace(Bf, sched, 0)
    x = torch.full((B, Lc), 256, dtype=torch.long, device="cuda")
    out = torch.full_like(x, -1)
    tmp = torch.empty_like(x)
    tokens_n = torch.full((Bf, L), -7, dtype=torch.long, device="cuda")
    t = torch.full((Bf,), 5, dtype=torch.long, device="cuda")
    t_steps = torch.zeros(1, 2, Bf, dtype=torch.long, device="cuda")
    u = torch.rand(B, 257, Lc, device="cuda")
    gids = torch.arange(B, device="cuda")
    fade = fade_dev(n)
    k8 = torch.ones(B, Lc, dtype=torch.uint8, device="cuda")

    def geo(o):
        return [o.get("B", B), o.get("W", W), o.get("n", n), o.get("ring", 0), o.get("n_cond", 2),
                _lib.ptr(o.get("fade", fade)), 0, 0.85, o.get("trunc_k", 0), o.get("scale", 3.0), _lib.ptr(o.get("keep")),
                _lib.ptr(o.get("known")), o.get("mode", 0), _lib.ptr(tokens_n), _lib.ptr(ws)]
    step = lambda o: lib.ds_denoiser_step_joint(p["handle"], _lib.ptr(x), _lib.ptr(t), None, _lib.ptr(kv), _lib.ptr(u), *geo(o),
                                                _lib.ptr(out), _lib.stream())
    step_r = lambda o: lib.ds_denoiser_step_joint_rng(p["handle"], _lib.ptr(x), _lib.ptr(t), None, _lib.ptr(kv), _lib.ptr(gids),
                                                      SEED, 0, *geo(o), _lib.ptr(out), _lib.stream())
    chain = lambda o: lib.ds_denoiser_sample_joint_rng(p["handle"], _lib.ptr(x), _lib.ptr(tmp), _lib.ptr(t_steps), 1, _lib.ptr(kv),
                                                       _lib.ptr(gids), SEED, 0, *geo(o), _lib.stream())
    for fn, name in ((step, b"ds_denoiser_step_joint:"), (step_r, b"ds_denoiser_step_joint_rng:"),
                     (chain, b"ds_denoiser_sample_joint_rng:")):
        for o in (dict(W=0), dict(n=27), dict(ring=1, W=1), dict(n_cond=3), dict(fade=None), dict(mode=1), dict(keep=k8),
                  dict(trunc_k=30), dict(scale=float("nan")), dict(B=0)):
            assert fn(o) == -1 and name in lib.ds_last_error_string(), (name, o, lib.ds_last_error_string())
    torch.cuda.synchronize()
    assert bool((tokens_n == -7).all()) and bool((out == -1).all()), "a rejected call enqueued work"
    assert step({}) == 0, lib.ds_last_error_string()
    torch.cuda.synchronize()
    pos = pipeline.joint_window_positions(W, n).cuda()
    want = x[:, pos].reshape(B * W, L)
    assert torch.equal(tokens_n[:B * W], want) and torch.equal(tokens_n[B * W:], want)
    assert int(out.min()) >= 0 and int(out.max()) <= 256


# ---- 5. the gather ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,n,ring", [(1, 13, False), (3, 1, False), (3, 26, True), (2, 13, True), (16, 1, False)])
def test_gather_is_torch_indexing(W, n, ring):
    B = 3
    Lc = 5 * pipeline.joint_canvas_cols(W, n, ring)
    g = torch.Generator().manual_seed(W * 100 + n)
    canvas = torch.randint(0, 2 ** 40, (B, Lc), generator=g).cuda()
    pos = R.window_positions(W, n, ring).cuda()
    for copies in (1, 2):
        win = torch.full((copies * B * W + 1, L), -1, dtype=torch.long, device="cuda")       # (a guard row behind the target)
        _lib.check(_lib.lib().ds_joint_gather(_lib.ptr(canvas), _lib.ptr(win), B, W, n, int(ring), copies, _lib.stream()))
        torch.cuda.synchronize()
        want = canvas[:, pos].reshape(B * W, L)
        for k in range(copies):
            assert torch.equal(win[k * B * W:(k + 1) * B * W], want)
        assert bool((win[-1] == -1).all())


# ---- 6. chains -------------------------------------------------------------------------------------------------------------
def joint(dt, cond, c, **kw):
    return dt.sample_joint(cond, c["W"], c["n"], ring=c["ring"], skip_step=c["skip_step"], **kw)


@pytest.mark.parametrize("name", list(I.CHAINS))
def test_chain_vs_joint_loop(name):
    want, gap = I.chain_reference(name)
    c = I.CHAINS[name]
    m = build(2, T=10)
    dt = m.transformer
    cond, null, known, keep = [v.cuda() for v in I.chain_inputs(name)]
    order = {t: k for k, (t, _) in enumerate(R.chain_steps(I.T_CHAIN, c["skip_step"]))}
    noise = I.chain_noise(name)
    kw = {}
    if c["guided"]:
        kw.update(guidance_scale=I.SCALE, null_condition_embed=null[0])
    if c["held"]:
        kw.update(keep_mask=keep, content_token=known)
    tok = joint(dt, cond, c, noise_fn=lambda t, shp: noise(order[t], shp), **kw)
    n_bad = int((tok.cpu() != want[-1]).sum())
    print("joint chain %s: %d token mismatches (yardstick min gap %.2e)" % (name, n_bad, gap))
    parity_line("joint T=10 chain %-10s: %d token mismatches vs joint_loop" % (name, n_bad))
    assert n_bad == 0
    if c["held"]:
        assert torch.equal(tok[keep], known[keep])
    # the one-call chain == the stepped entry called from Python, on the Philox stream of the canvas positions
    ids = [12, 500]
    Lc = tok.shape[1]
    calls = len(order)
    a = joint(dt, cond, c, caption_ids=ids, seed=SEED, **kw)
    b = joint(dt, cond, c, noise_fn=lambda t, shp: philox_u(ids, order[t], Lc), **kw)
    assert calls == want.shape[0] and torch.equal(a, b) and int(a.max()) < 256


def test_a_clip_alone_equals_the_clip_in_a_batch():
    m = build(2, T=10)
    dt = m.transformer
    ids = torch.tensor([40, 1000, 7])
    cond = synth.synth_cond_emb(3, key="joint.b.cond").cuda()
    null = synth.synth_cond_emb(1, key="joint.null")[0].cuda()
    for kw in (dict(ring=False), dict(ring=True, guidance_scale=3.0, null_condition_embed=null)):
        run = lambda sel: dt.sample_joint(cond[sel].contiguous(), 2, 13, caption_ids=ids[sel], seed=SEED, **kw).cpu()
        whole = run([0, 1, 2])
        assert torch.equal(run([2, 0, 1]), whole[[2, 0, 1]])
        for i in range(3):
            assert torch.equal(run([i])[0], whole[i]), "clip %d alone differs from the batch of 3" % i
        # ... and from a batch that is cut into chunks of one clip per forward
        dt.JOINT_MAX_ROWS = 2 * (2 if "guidance_scale" in kw else 1)
        try:
            assert torch.equal(run([0, 1, 2]), whole)
        finally:
            del dt.JOINT_MAX_ROWS


# ---- 7. drivers ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ds():
    from text_to_sound_synthesis_amd import tokenizer as tz
    from text_to_sound_synthesis_amd.config import default_config
    return pipeline.Diffsound(config=default_config(n_layer=2, diffusion_step=10, with_clip=True, bpe_path=tz.CLOSED_VOCAB_PATH),
                              random_vocoder=True)


def shared_columns_agree(tokens, n, ring=False):
    W = tokens.shape[1]
    for w in range(W if ring else W - 1):
        if not torch.equal(tokens[:, w, 5 * (53 - n):], tokens[:, (w + 1) % W, :5 * n]):
            return False
    return True


def test_generate_long_joint(ds):
    captions = synth.synth_captions(2, seed=4)
    W, n, total, samples = pipeline.long_plan(25)
    mel01, wave, tokens = ds.generate_long(captions, 25, caption_ids=[0, 1], seed=3, joint=True)
    assert tuple(tokens.shape) == (2, W, 265) and int(tokens.max()) < 256 and W >= 3
    assert tuple(mel01.shape) == (2, 80, math.ceil(samples / 256)) and tuple(wave.shape) == (2, 1, samples)
    assert bool(torch.isfinite(wave).all())
    assert shared_columns_agree(tokens, n)
    out = ds.model.generate_long_content(batch={"text": captions, "caption_ids": [0, 1], "seed": 3}, windows=W, overlap_cols=n,
                                         joint=True)
    assert torch.equal(out["content_token"], tokens) and tuple(out["canvas_token"].shape) == (2, 5 * total)
    assert torch.equal(out["canvas_token"][:, pipeline.joint_window_positions(W, n).cuda()], tokens)
    assert tuple(out["content"].shape) == (2 * W, 1, 80, 848)
    fast = ds.model.generate_long_content(batch={"text": captions, "caption_ids": [0, 1], "seed": 3}, windows=W, overlap_cols=n,
                                          joint=True, sample_type="top0.85r,fast2")["content_token"]
    assert shared_columns_agree(fast, n) and int(fast.max()) < 256 and not torch.equal(fast, tokens)
    guided = ds.generate_long(captions, 25, caption_ids=[0, 1], seed=3, joint=True, guidance_scale=3.0,
                              negative_text=synth.synth_captions(1, seed=9)[0])[2]
    assert shared_columns_agree(guided, n) and not torch.equal(guided, tokens)
    # joint=False and no keyword at all: today's path, the same tokens and waves
    a = ds.generate_long(captions, 25, caption_ids=[0, 1], seed=3)
    b = ds.generate_long(captions, 25, caption_ids=[0, 1], seed=3, joint=False)
    assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    assert not torch.equal(a[2], tokens)


def test_extend_audio_joint_and_the_errors(ds):
    captions = synth.synth_captions(2, seed=4)
    g = torch.Generator().manual_seed(33)
    rec = (0.2 * torch.randn(2, 217088, generator=g)).cuda()
    start = ds.model.prepare_content({"audio": rec})["content_token"]
    mel01, wave, tokens = ds.extend_audio(rec, captions, 18, caption_ids=[0, 1], seed=3, joint=True)
    W, n, _, samples = pipeline.long_plan(18)
    assert tuple(tokens.shape) == (2, W, 265) and torch.equal(tokens[:, 0], start) and shared_columns_agree(tokens, n)
    assert tuple(wave.shape) == (2, 1, samples) and int(tokens.max()) < 256
    a = ds.extend_audio(rec, captions, 18, caption_ids=[0, 1], seed=3)
    b = ds.extend_audio(rec, captions, 18, caption_ids=[0, 1], seed=3, joint=False)
    assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1])
    batch = {"text": captions}
    glc = ds.model.generate_long_content
    with pytest.raises(ValueError, match="joint sampling"):
        glc(batch=batch, windows=2, overlap_cols=13, joint=True, tracks={"text": ["a"], "weight": torch.ones(2, 1, 5 * 93)})
    with pytest.raises(ValueError, match="joint sampling"):
        glc(batch=batch, windows=2, overlap_cols=13, joint=True, sample_type="top0.85r,purity25")
    with pytest.raises(ValueError, match="joint sampling"):
        glc(batch=batch, windows=2, overlap_cols=13, joint=True, keep_mode="renoise")
    with pytest.raises(ValueError):
        glc(batch=batch, windows=2, overlap_cols=13, ring=True)
    with pytest.raises(ValueError):
        glc(batch=batch, windows=1, overlap_cols=13, joint=True, ring=True)
    with pytest.raises(ValueError, match="joint sampling"):
        ds.generate_long(captions, 25, joint=True, keep_mode="renoise")
    with pytest.raises(ValueError, match="joint sampling"):
        ds.generate_long(captions, 25, joint=True, purity_steps=10)


# ---- 8. loops --------------------------------------------------------------------------------------------------------------
def test_generate_loop(ds, tmp_path):
    captions = synth.synth_captions(2, seed=4)
    W, n, C, samples = pipeline.loop_plan(12)
    h = 53 - n
    assert (W, C) == (2, 2 * h)
    mel01, wave, tokens, made = ds.generate_loop(captions, 12, caption_ids=[0, 1], seed=3, save_root=str(tmp_path / "loop"))
    assert made == samples / 22050 and tuple(tokens.shape) == (2, W, 265) and int(tokens.max()) < 256
    assert tuple(mel01.shape) == (2, 80, 16 * C) and tuple(wave.shape) == (2, 1, 4096 * C)
    assert bool(torch.isfinite(wave).all()) and (tmp_path / "loop" / "000001.wav").exists()
    assert shared_columns_agree(tokens, n, ring=True)                 # the ring identity: the last window flows into the first
    # the uncut rendering: periodic wherever it is fully blended
    out = ds.model.generate_long_content(batch={"text": captions, "caption_ids": [0, 1], "seed": 3}, windows=W, overlap_cols=n,
                                         joint=True, ring=True)
    assert torch.equal(out["content_token"], tokens)
    mel, uncut = ds._loop_rendering(out["content"], W, n)
    P, lo, hi = 16 * C, 16 * n, (W + 4) * 16 * h
    assert mel.shape[2] == 848 + (W + 3) * 16 * h and hi - P > lo
    assert torch.equal(mel[:, :, lo:hi - P], mel[:, :, lo + P:hi])    # frames f and f + 16 C, bit for bit
    assert torch.equal(((mel + 1) / 2)[:, :, 2 * 16 * h:2 * 16 * h + P], mel01)
    off, period = pipeline.loop_cut(C, h)
    assert torch.equal(uncut[:, :, off:off + period], wave)
    m_ = 4096
    dist = float((uncut[:, :, off - m_:off] - wave[:, :, -m_:]).abs().max())
    parity_line("loop W=%d C=%d: the %d samples ahead of the loop vs its last %d: max |diff| %.3e (peak %.3f)"
                % (W, C, m_, m_, dist, float(wave.abs().max())))
    assert dist <= 1e-4, dist
    dist_after = float((uncut[:, :, off + period:off + period + m_] - wave[:, :, :m_]).abs().max())
    assert dist_after <= 1e-4, dist_after
    # rates: 44 100 Hz is exact, 48 000 Hz has no whole period; levelling: static strategies only
    w44 = ds.generate_loop(captions, 12, caption_ids=[0, 1], seed=3, sample_rate=44100)[1]
    assert tuple(w44.shape) == (2, 1, 2 * 4096 * C)
    with pytest.raises(ValueError, match="period"):
        ds.generate_loop(captions, 12, sample_rate=48000)
    with pytest.raises(ValueError, match="limit"):
        ds.generate_loop(captions, 12, level={"strategy": "loudness", "limit": True})
    lev = ds.generate_loop(captions, 12, caption_ids=[0, 1], seed=3, level="peak")[1]
    assert tuple(lev.shape) == tuple(wave.shape) and float(lev.abs().amax()) <= 10 ** (-1 / 20) + 1e-3
    assert not torch.equal(lev, wave)
    with pytest.raises(ValueError):
        ds.generate_loop(captions, 5)


# ---- 9. the longest canvas, once -------------------------------------------------------------------------------------------
def test_sixteen_windows_one_column_overlap():
    m = build(2, T=10)
    dt = m.transformer
    cond = synth.synth_cond_emb(1, key="joint.long.cond").cuda()
    canvas = dt.sample_joint(cond, 16, 1, caption_ids=[9], seed=SEED)
    assert tuple(canvas.shape) == (1, 4165) and int(canvas.min()) >= 0 and int(canvas.max()) < 256
    tokens = canvas[:, pipeline.joint_window_positions(16, 1).cuda()]
    assert tuple(tokens.shape) == (1, 16, 265) and shared_columns_agree(tokens, 1)
    assert torch.equal(dt.sample_joint(cond, 16, 1, caption_ids=[9], seed=SEED), canvas)
