"""The training step away from the two shapes the other modules pin (2 layers / B = 3 / K = 256 and 19 layers / B = 20): the
512-entry codebook (BASELINE configs[3], caps_512.yaml: 513 classes, N = 512 logits, a 513-row embedding), one sample, the
32-row limit of the AdaLN backward's row kernels and past it, shared timesteps -- against the oracle's loss + autograd run in
FLOAT64 on the same x_t, next to the same oracle in fp32 (the yardstick's own distance).  Then the kernels those shapes lean on
at their edges (ds_embed_bwd / _ws, ds_rows_outer / ds_rows_times_matrix, ds_loss_tail / ds_loss_tail_bwd against float64), and
bit-reproducibility of the whole step: the backward sums in a fixed order everywhere, so two identical steps must give
identical gradients.  GPU only."""
import pytest
import torch

from conftest import parity_line, synth_sd
from text_to_sound_synthesis_amd import synth

pytestmark = pytest.mark.gpu
NO_GRAD = True

T = 100
LOSS_TOL = 2e-5         # relative, against float64
GRAD_NORM_TOL = 5e-5    # per-tensor |norm - float64 norm| / float64 norm (test_hip_train_batch.py) ...
REF_FACTOR = 4.0        # ... or this many times the oracle's own fp32 distance for the tensor, if larger
ELEM_TOL = 2e-3         # elementwise max-abs error, relative to the tensor's largest element
ZERO_GRAD = 1e-7        # float64 |g|max under this: an analytically zero gradient (the attention key biases)

MIXED = [0, 99, 42, 42, 1, 98, 57, 12, 12, 12]
CASES = {               # K, B, t
    "k512": (512, 3, [57, 0, 93]),
    "b1_t0": (256, 1, [0]),
    "b1_t99": (256, 1, [99]),
    "b32_shared": (256, 32, [42] * 32),
    "b40_mixed": (256, 40, MIXED * 4),
    "k512_b40": (512, 40, MIXED[::-1] * 4),
}


def rnd(shape, key, scale=1.0):
    return (synth.synth_uniform(shape, key=key) * 2 - 1) * scale


@pytest.fixture(scope="module")
def L():
    from text_to_sound_synthesis_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _lib.lib()
    return _lib


def sd_of(K):
    return synth_sd("dalle" if K == 256 else "dalle_k512", 2)


def inputs(case):
    K, B, t = CASES[case]
    x0 = synth.synth_tokens(B, 265, K, mask_frac=0.0, key="ts.x0.%s" % case)
    cond = synth.synth_cond_emb(B, key="ts.c.%s" % case)
    pt = torch.full((B,), 0.01)
    u = synth.synth_uniform((B, K + 1, 265), key="ts.u.%s" % case)
    return x0, cond, torch.tensor(t), pt, u


_ORACLE = {}


def oracle(case):
    """(x_t, {dtype: (loss, {parameter name relative to the DiffusionTransformer: gradient as float64})}) for float32 and
    float64 runs of the oracle's train_loss + backward() on the same x_t (the fp32 q_sample's)"""
    if case not in _ORACLE:
        import diffsound_oracle as O
        K = CASES[case][0]
        x0, cond, t, pt, u = inputs(case)
        xt = O.q_sample(O.make_schedule(T, K + 1), x0, t, u, K + 1).argmax(1)
        runs = {}
        for dtype in (torch.float32, torch.float64):
            sd = {k: (v.detach().to(dtype, copy=True).requires_grad_(True)
                      if v.is_floating_point() and k.startswith("transformer.transformer.") else v) for k, v in sd_of(K).items()}
            with torch.enable_grad():
                _, _, loss, _ = O.train_loss(sd, x0, cond.to(dtype), t, pt.to(dtype), u, xt=xt)
                loss.backward()
            runs[dtype] = (loss.item(), {k[len("transformer."):]: v.grad.double() for k, v in sd.items()
                                         if v.requires_grad and v.grad is not None})
        _ORACLE[case] = (xt, runs)
    return _ORACLE[case]


def model_of(K):
    from text_to_sound_synthesis_amd.config import build_model, default_config
    m = build_model(default_config(n_layer=2, diffusion_step=T, n_embed=K))
    _, unexpected = m.load_state_dict(dict(sd_of(K)), strict=False)
    assert not unexpected
    m = m.cuda().eval()
    dt = m.transformer
    dt.auxiliary_loss_weight, dt.adaptive_auxiliary_loss, dt.mask_weight = 5.0e-4, True, [1, 1]
    return dt


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
@pytest.mark.parametrize("case", list(CASES))
def test_training_step_vs_float64_oracle(case, precision):
    """TrainStep.loss_and_grads (attention "fused") against the float64 oracle: x_t of the product's q_sample equals the
    oracle's fp32 one (which both sides then use), loss within LOSS_TOL, every gradient's norm within max(GRAD_NORM_TOL,
    REF_FACTOR x the fp32 oracle's distance) and elementwise within ELEM_TOL of its largest element; no gradient missing."""
    from text_to_sound_synthesis_amd.modeling.train import TrainStep
    K, B, tl = CASES[case]
    x0, cond, t, pt, u = inputs(case)
    xt, runs = oracle(case)
    dt = model_of(K)
    xt_hip = dt.q_sample_tokens(x0.cuda(), t.cuda(), u.cuda()).cpu()
    assert torch.equal(xt_hip, xt), "q_sample: %d tokens differ" % int((xt_hip != xt).sum())
    step = TrainStep(dt, precision=precision, attention="fused")
    loss, grads = step.loss_and_grads(x0.cuda(), cond.cuda(), t.cuda(), pt.cuda(), u.cuda())
    loss64, g64 = runs[torch.float64]
    loss32, g32 = runs[torch.float32]
    loss_err = abs(float(loss) - loss64) / abs(loss64)
    worst, missing = [], []
    for name, want in g64.items():
        amax = want.abs().max().item()
        if name not in grads:
            if amax > 0:
                missing.append(name)
            continue
        got = grads[name].cpu().double()
        assert got.shape == want.shape, name
        if amax < ZERO_GRAD:
            # the key biases have an analytically ZERO gradient (softmax is invariant to them): rounding noise on both sides
            assert got.abs().max().item() < 1e-6, name
            continue
        n64 = want.norm().item()
        ref = abs(g32[name].norm().item() - n64) / n64
        err = abs(got.norm().item() - n64) / n64
        elem = (got - want).abs().max().item() / amax
        worst.append((err, name, ref, elem))
    worst.sort(reverse=True)
    over = [w for w in worst if w[0] > max(GRAD_NORM_TOL, REF_FACTOR * w[2])]
    elem_over = [w for w in worst if w[3] > ELEM_TOL]
    e, n, r, el = worst[0]
    parity_line("train shapes %s %s (K %d, B %d): loss rel %.1e (oracle fp32 %.1e), worst of %d per-tensor norms %.1e (%s; the "
                "oracle's fp32 %.1e), worst elementwise %.1e, %d over the norm bound, %d over the elementwise bound"
                % (case, precision, K, B, loss_err, abs(loss32 - loss64) / abs(loss64), len(worst), e, n, r,
                   max(w[3] for w in worst), len(over), len(elem_over)))
    for w in worst[:6]:
        print("  norm rel err %.2e (oracle fp32 %.2e)  elementwise %.2e  %s" % (w[0], w[2], w[3], w[1]))
    assert not missing, missing
    assert len(worst) >= 50
    assert loss_err < LOSS_TOL, (float(loss), loss64)
    assert not over, over[:4]
    assert not elem_over, elem_over[:4]


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
@pytest.mark.parametrize("tcase", ["all_t99", "shared_t"])
def test_training_step_is_bit_reproducible(precision, tcase):
    """Three loss_and_grads calls on identical inputs (2 layers, B = 20; the first one calibrates the f16x2 scales): the
    second and third give the same loss and the same bits in EVERY gradient.  A race or an uninitialised read in any
    kernel of the step, or an order-dependent sum (float atomics), shows up here."""
    from text_to_sound_synthesis_amd.modeling.train import TrainStep
    B = 20
    t = [99] * B if tcase == "all_t99" else [5, 5, 17, 17, 17, 0, 0, 63, 99, 99, 42, 42, 42, 42, 8, 71, 71, 1, 98, 98]
    dt = model_of(256)
    x0 = synth.synth_tokens(B, 265, 256, mask_frac=0.0, key="tr.x0").cuda()
    cond = synth.synth_cond_emb(B, key="tr.c").cuda()
    u = synth.synth_uniform((B, 257, 265), key="tr.u").cuda()
    tt, pt = torch.tensor(t).cuda(), torch.full((B,), 0.01).cuda()
    step = TrainStep(dt, precision=precision, attention="fused")
    runs = []
    for _ in range(3):
        loss, grads = step.loss_and_grads(x0, cond, tt, pt, u)
        runs.append((loss.cpu().clone(), {k: v.cpu().clone() for k, v in grads.items()}))
    (l2, g2), (l3, g3) = runs[1], runs[2]
    assert torch.equal(l2, l3), (float(l2), float(l3))
    assert g2.keys() == g3.keys() and len(g2) >= 50
    differ = [k for k in g2 if not torch.equal(g2[k], g3[k])]
    assert not differ, differ[:8]


# ---- kernel edges -----------------------------------------------------------------------------------------------------------
def embed_bwd(L, dx, tok, rows, base=None, ws=True):
    M, D = dx.shape
    demb = torch.zeros(rows, D, device="cuda") if base is None else base.clone().cuda()
    dxc, tokc = dx.cuda(), tok.cuda()
    if ws:
        work = torch.full((L.lib().ds_embed_bwd_work_floats(M, D, rows),), float("nan"), device="cuda")
        L.check(L.lib().ds_embed_bwd_ws(L.ptr(dxc), L.ptr(tokc), L.ptr(demb), M, D, rows, L.ptr(work), work.numel(), L.stream()))
    else:
        L.check(L.lib().ds_embed_bwd(L.ptr(dxc), L.ptr(tokc), L.ptr(demb), M, D, rows, L.stream()))
    return demb.cpu()


@pytest.mark.parametrize("ws", [True, False], ids=["chunked", "no_workspace"])
@pytest.mark.parametrize("case", ["rows513", "all_mask_b40", "mask_share_0.9", "out_of_range"])
def test_embedding_backward_edges(L, case, ws):
    """ds_embed_bwd_ws (the training step's entry) and ds_embed_bwd (no workspace) against float64 index_add_: the K = 512
    table (513 rows); 40 x 265 positions all on the [MASK] row (the longest list there is); a mixed grid with a 0.9 [MASK]
    share accumulated onto a non-zero table; tokens outside [0, rows) skipped.  Two runs bit-identical."""
    D = 1024
    if case == "rows513":
        rows, tok = 513, synth.synth_tokens(3, 265, 512, mask_frac=0.3, key="eb5.t").view(-1)
    elif case == "all_mask_b40":
        rows, tok = 257, torch.full((40 * 265,), 256, dtype=torch.long)
    elif case == "mask_share_0.9":
        rows, tok = 257, synth.synth_tokens(20, 265, 256, mask_frac=0.9, key="eb9.t").view(-1)
        share = float((tok == 256).float().mean())
        assert 0.85 < share < 0.95, share
    else:
        rows, tok = 257, synth.synth_tokens(4, 265, 256, mask_frac=0.3, key="ebo.t").view(-1)
        tok[::7], tok[3::11], tok[5::13] = -1, 257, 1 << 40
    M = tok.numel()
    dx = rnd((M, D), "eb.dx.%s" % case)
    base = rnd((rows, D), "eb.base") if case == "mask_share_0.9" else None
    keep = (tok >= 0) & (tok < rows)
    ref = torch.zeros(rows, D, dtype=torch.float64) if base is None else base.double()
    ref = ref.index_add(0, tok[keep], dx[keep].double())
    a, b = embed_bwd(L, dx, tok, rows, base, ws), embed_bwd(L, dx, tok, rows, base, ws)
    assert torch.equal(a, b)
    err = (a.double() - ref).abs().max().item() / ref.abs().max().item()
    print("%s: max-abs error %.2e of the largest element %.2e" % (case, err, ref.abs().max().item()))
    assert err < 2e-6


def test_embedding_backward_rejects_short_work(L):
    M, D, rows = 530, 1024, 257
    dx, tok = torch.zeros(M, D, device="cuda"), torch.zeros(M, dtype=torch.long, device="cuda")
    demb = torch.zeros(rows, D, device="cuda")
    n = L.lib().ds_embed_bwd_work_floats(M, D, rows)
    assert n == 3 * rows * D
    work = torch.empty(n, device="cuda")
    assert L.lib().ds_embed_bwd_ws(L.ptr(dx), L.ptr(tok), L.ptr(demb), M, D, rows, L.ptr(work), n - 1, L.stream()) != 0
    assert L.lib().ds_embed_bwd_ws(L.ptr(dx), L.ptr(tok), L.ptr(demb), M, D - 2, rows, L.ptr(work), n, L.stream()) != 0
    assert L.lib().ds_embed_bwd(L.ptr(dx), L.ptr(tok), L.ptr(demb), M, D - 2, rows, L.stream()) != 0


def test_rows_kernels_at_32_rows_and_38_modules(L):
    """ds_rows_outer / ds_rows_times_matrix at their 32-row limit with G = 38 (the 19-layer model's AdaLN module count)."""
    G, B, N, D = 38, 32, 512, 256
    a, s_ = rnd((G, B, N), "r32.a", 2.0), rnd((G, B, D), "r32.s", 0.5)
    ref = torch.einsum("gbn,gbd->gnd", a.double(), s_.double())
    ac, sc = a.cuda(), s_.cuda()
    out = torch.full((G, N, D), float("nan"), device="cuda")
    L.check(L.lib().ds_rows_outer(L.ptr(ac), L.ptr(sc), L.ptr(out), G, B, N, D, L.stream()))
    assert (out.cpu().double() - ref).abs().max().item() < 2e-6 * ref.abs().max().item()
    W = rnd((G, N, D), "r32.w", 0.5)
    ref = torch.einsum("gbk,gkd->gbd", a.double(), W.double())
    Wc = W.cuda()
    KS = N // 256
    part = torch.full((KS, G, B, D), float("nan"), device="cuda")
    L.check(L.lib().ds_rows_times_matrix(L.ptr(ac), L.ptr(Wc), L.ptr(part), G, B, N, D, L.stream()))
    got = part.double().sum(0).cpu()
    assert (got - ref).abs().max().item() < 2e-6 * ref.abs().max().item()


@pytest.mark.parametrize("B", [32, 40, 65])
def test_rows_outer_past_32_samples(L, B):
    """modeling/train.py _rows_outer: one ds_rows_outer launch per 32 samples, the partial results added in chunk order --
    against float64, and bit-identical twice."""
    from text_to_sound_synthesis_amd.modeling.train import _rows_outer
    G, N, D = 4, 300, 512
    a, s_ = rnd((G, B, N), "rp.a%d" % B, 2.0), rnd((G, B, D), "rp.s%d" % B, 0.5)
    ref = torch.einsum("gbn,gbd->gnd", a.double(), s_.double())
    ac, sc = a.cuda(), s_.cuda()
    o1, o2 = _rows_outer(ac, sc).cpu(), _rows_outer(ac, sc).cpu()
    assert torch.equal(o1, o2)
    assert (o1.double() - ref).abs().max().item() < 2e-6 * ref.abs().max().item()


def _tail_ref(K, logits, x0, xt, t, pt, mask_weight, adaptive, aux=5.0e-4):
    """float64 restatement of the loss tail (oracle pieces): per-position kl / nll / kl_aux and the autograd gradient of
    sum_b vb_loss_b with respect to the logits [B, K, L]"""
    import diffsound_oracle as O
    sched = {k: v.double() for k, v in O.make_schedule(T, K + 1).items()}
    lg = logits.double().requires_grad_(True)
    with torch.enable_grad():
        log_x0 = O.log_onehot(x0, K + 1).double()
        log_xt = O.log_onehot(xt, K + 1).double()
        recon = O.predict_start(lg, torch.float64)
        model = O.q_posterior(sched, recon, log_xt, t)
        true = O.q_posterior(sched, log_x0, log_xt, t)
        kl = (true.exp() * (true - model)).sum(1)
        nll = -(log_x0.exp() * model).sum(1)
        kl_aux = (log_x0[:, :-1].exp() * (log_x0[:, :-1] - recon[:, :-1])).sum(1)
        m = (xt == K).double()
        w = m * mask_weight[0] + (1.0 - m) * mask_weight[1]
        is0 = (t == 0).double()
        vb = (is0 * nll.sum(-1) + (1.0 - is0) * (kl * w).sum(-1)) / pt.double()
        wa = t.double() / T + 1.0 if adaptive else 1.0
        vb = vb + wa * aux * (is0 * nll.sum(-1) + (1.0 - is0) * (kl_aux * w).sum(-1)) / pt.double()
        vb.sum().backward()
    return kl.detach(), nll.detach(), kl_aux.detach(), lg.grad


def _tail_inputs(K):
    import diffsound_oracle as O
    B = 4
    t = torch.tensor([0, 1, 98, 99])
    x0 = synth.synth_tokens(B, 265, K, mask_frac=0.0, key="lt.x0.%d" % K)
    xt = O.q_sample(O.make_schedule(T, K + 1), x0, t, synth.synth_uniform((B, K + 1, 265), key="lt.u.%d" % K), K + 1).argmax(1)
    logits = rnd((B, K, 265), "lt.z.%d" % K, 30.0)                      # spread to +-30: the log-sum-exp tails
    tab = torch.zeros(8, T + 1)
    sched = O.make_schedule(T, K + 1)
    for i, n in enumerate(("log_at", "log_bt", "log_ct", "log_1_min_ct", "log_cumprod_at", "log_cumprod_bt", "log_cumprod_ct",
                           "log_1_min_cumprod_ct")):
        tab[i, :sched[n].numel()] = sched[n]
    return B, t, x0, xt, logits, tab


@pytest.mark.parametrize("K", [256, 512])
def test_loss_tail_forward_terms_vs_float64(L, K):
    """ds_loss_tail per position (kl, nll, kl_aux) against float64 at t = 0, 1, 98, 99 with logits spread to +-30."""
    B, t, x0, xt, logits, tab = _tail_inputs(K)
    assert int((xt[3] == K).sum()) > 200                               # t = 99: mostly [MASK]
    kl, nll, kla, _ = _tail_ref(K, logits, x0, xt, t, torch.ones(B), (1.0, 1.0), True)
    rows = logits.permute(0, 2, 1).reshape(B * 265, K).contiguous().cuda()
    out = [torch.full((B, 265), float("nan"), device="cuda") for _ in range(3)]
    x0c, xtc, tc, tabc = x0.cuda(), xt.cuda(), t.cuda(), tab.cuda()
    L.check(L.lib().ds_loss_tail(L.ptr(rows), L.ptr(x0c), L.ptr(xtc), L.ptr(tc), L.ptr(tabc), L.ptr(out[0]), L.ptr(out[1]),
                                 L.ptr(out[2]), None, B, 265, K, T, L.stream()))
    for name, got, want in zip(("kl", "nll", "kl_aux"), out, (kl, nll, kla)):
        err = (got.cpu().double() - want).abs().max().item()
        print("K %d %s: max-abs error %.2e, |ref|max %.2e" % (K, name, err, want.abs().max().item()))
        assert err <= 1e-4 * want.abs().max().item() + 1e-5, (name, err)


@pytest.mark.parametrize("mask_weight,adaptive", [((1.0, 1.0), 1), ((0.7, 1.3), 0)])
@pytest.mark.parametrize("K", [256, 512])
def test_loss_tail_backward_extremes_vs_float64(L, K, mask_weight, adaptive):
    """ds_loss_tail_bwd against float64 autograd of the same loss: logits spread to +-30, t = 0, 1, 98, 99, mask weights
    other than (1, 1) and the auxiliary weight not adaptive."""
    B, t, x0, xt, logits, tab = _tail_inputs(K)
    pt = torch.tensor([0.01, 0.02, 0.005, 0.01])
    _, _, _, ref = _tail_ref(K, logits, x0, xt, t, pt, mask_weight, adaptive)
    rows = logits.permute(0, 2, 1).reshape(B * 265, K).contiguous().cuda()
    out = torch.full((B * 265, K), float("nan"), device="cuda")
    x0c, xtc, tc, ptc, tabc = x0.cuda(), xt.cuda(), t.cuda(), pt.cuda(), tab.cuda()
    L.check(L.lib().ds_loss_tail_bwd(L.ptr(rows), L.ptr(x0c), L.ptr(xtc), L.ptr(tc), L.ptr(ptc), L.ptr(tabc), L.ptr(out),
                                     B, 265, K, T, mask_weight[0], mask_weight[1], 5.0e-4, adaptive, L.stream()))
    got = out.view(B, 265, K).permute(0, 2, 1).cpu().double()
    for b in range(B):
        err = (got[b] - ref[b]).abs().max().item() / ref[b].abs().max().item()
        print("K %d t %d: max-abs error %.2e of |ref|max %.2e" % (K, int(t[b]), err, ref[b].abs().max().item()))
        assert err < 5e-4, (int(t[b]), err)
