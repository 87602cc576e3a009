"""BASELINE configs[4] as the reference runs it: the training iteration FROM THE REFERENCE'S BATCH
{'image': mel f32[20,1,80,848], 'text': 20 captions} at the benchmarked shape -- 19 layers, B = 20 -- against
tests/golden/train_batch_L19_b20{,_trainedlike}.npz, which oracle/make_golden.py train_batch() produced by calling the
UNMODIFIED reference's `DALLE.forward(batch, return_loss=True)` (dalle_spec.py:389-400 -> prepare_input :93-133 ->
diffusion_transformer.py:539-577, 408-476) and `loss.backward()` (engine/solver_spec.py:308-331) with the timesteps and the
q_sample noise injected.  The golden keeps what every stage hands to the next, the loss, the norm and the largest element
of EVERY parameter gradient (539 tensors), the global norm and three gradient slices.  GPU only (-m gpu).

Two weight profiles: "init" (N(0, 0.02)-like) and "trained" (synth.py: heavy-tailed weights, hot residual channels, GELU2
outputs in the 1e4s) -- the second is where ONE 2^k loss scale for the whole backward and the saturation monitor meet a
heavy-tailed dY."""
import json
import math
import os

import pytest
import torch

from conftest import GOLDEN, golden, parity_line, synth_sd
from text_to_sound_synthesis_amd import synth

pytestmark = pytest.mark.gpu
NO_GRAD = True

B = 20
GRAD_NORM_TOL = 5e-5        # per-tensor |norm - exact norm| / exact norm, exact = the reference's modules run in float64
REF_FACTOR = 4.0            # ... or this many times the reference's own fp32-vs-float64 distance for the same tensor, if larger
SLICE_TOL = 2e-4            # elementwise, relative to the slice's largest element
LOSS_TOL = 2e-5             # relative
VQ_TIE = 2e-4               # nearest-code margin (squared distance) under which the argmin is a rounding-level tie


def names(profile):
    tag = "train_batch_L19_b20" + ("_trainedlike" if profile == "trained" else "")
    with open(os.path.join(GOLDEN, tag + "_names.json")) as f:
        return tag, json.load(f)


def build(profile):
    from text_to_sound_synthesis_amd import tokenizer as tz
    from text_to_sound_synthesis_amd.config import build_model, default_config
    m = build_model(default_config(n_layer=19, diffusion_step=100, with_clip=True, bpe_path=tz.CLOSED_VOCAB_PATH))
    with open(os.path.join(GOLDEN, "state_dict_keys_clip.json")) as f:
        clip_sd = synth.synth_state_dict(json.load(f))
    sd = {**synth_sd("dalle", 19, profile=profile), **synth_sd("encoder"), **clip_sd}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected
    m = m.cuda().eval()
    dt = m.transformer
    dt.auxiliary_loss_weight, dt.adaptive_auxiliary_loss, dt.mask_weight = 5.0e-4, True, [1, 1]     # caps_text.yaml:46-48
    return m


def batch_of(meta):
    mel = synth.synth_uniform((B, 1, 80, 848), key="tb.mel") * 2 - 1
    return {"image": mel.cuda(), "text": meta["captions"]}


def injected(g):
    return g["t"].long().cuda(), (torch.ones(B) / 100).cuda(), synth.synth_uniform((B, 257, 265), key="tb.u").cuda()


@pytest.fixture(scope="module")
def model_init():
    return build("init")


def test_prologue_stages_vs_reference(model_init):
    """mel + captions -> BPE ids (exact), CLIP embedding (fp16 tower: 5e-4 on unit-norm rows), VQ token ids (exact except
    where the reference's own nearest-code margin is a rounding-level tie)."""
    from text_to_sound_synthesis_amd.modeling.train import training_inputs
    tag, meta = names("init")
    g = golden(tag)
    m = model_init
    gen = torch.Generator(device="cuda").manual_seed(5)
    x0, cond, t, pt, u = training_inputs(m, batch_of(meta), generator=gen)
    ids = m.prepare_condition(batch_of(meta))["condition_token"]
    assert torch.equal(ids.cpu().long(), g["caption_tokens"].long()), "BPE ids differ from the reference's"
    cond_err = float((cond.cpu() - g["cond_emb"].float()).abs().max())
    diff = x0.cpu() != g["tokens"].long()
    gaps = g["vq_gap"][diff]
    assert x0.shape == (B, 265) and cond.shape == (B, 77, 512) and t.shape == pt.shape == (B,) and u.shape == (B, 257, 265)
    assert x0.dtype == torch.long and int(x0.min()) >= 0 and int(x0.max()) < 256
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0 and torch.equal(pt.cpu(), torch.full((B,), 0.01))     # uniform branch: Lt_count is empty
    parity_line("train batch prologue: BPE ids identical, CLIP max-abs %.2e, VQ tokens %d of %d differ (largest reference margin there %.1e; "
                "%d reference margins are under %.0e)" % (cond_err, int(diff.sum()), diff.numel(), float(gaps.max()) if gaps.numel() else 0.0,
                                                          int((g["vq_gap"] < VQ_TIE).sum()), VQ_TIE))
    assert cond_err < 5e-4
    assert bool((gaps < VQ_TIE).all()), "a VQ code differs away from a near-tie: margins %s" % gaps[gaps >= VQ_TIE][:4]
    assert int(diff.sum()) <= int((g["vq_gap"] < VQ_TIE).sum())


def check_grads(g, meta, loss, grads, what, floor=None):
    """Every gradient norm against the reference's -- measured against the FLOAT64 run of the reference (grad_norms64: the exact
    values), next to what the reference's own fp32 run (grad_norms) is away from them: the product may not be further from
    exact than GRAD_NORM_TOL, whatever the tensor's magnitude (the smallest norms here are 1e-8 of the largest)."""
    ref_names = meta["grad_names"]
    got_norm = {k: float(v.double().norm()) for k, v in grads.items()}
    missing = [n for n in ref_names if n not in grads]
    assert not missing, missing[:4]
    worst, ref_worst = [], 0.0
    for n, n32, n64, amax in zip(ref_names, g["grad_norms"].tolist(), g["grad_norms64"].tolist(), g["grad_amax"].tolist()):
        if amax < 1e-7:      # analytically zero (the attention key biases: softmax is invariant to them): rounding noise on both
            assert got_norm[n] < 1e-6 * float(g["grad_total64"]), (n, got_norm[n])      # sides -- 1e-6 of the global norm at most
            continue
        ref_err = abs(n32 - n64) / n64
        worst.append((abs(got_norm[n] - n64) / n64, n, n64, ref_err))
        ref_worst = max(ref_worst, ref_err)
    worst.sort(reverse=True)
    # the bound per tensor: GRAD_NORM_TOL, or -- where the reference's own fp32 is further than that from exact (trained-like
    # weights: GELU2 outputs in the 1e4s make fp32 itself lose three digits in the first blocks) -- REF_FACTOR times the
    # reference's own distance (a split product carries 22 bits where an fp32 FMA carries 24: measured 1.2x .. 3.1x there)
    floor = GRAD_NORM_TOL if floor is None else floor
    over = [(e, n, mag, r) for e, n, mag, r in worst if e > max(floor, REF_FACTOR * r)]
    beyond = [(e, n, mag, r) for e, n, mag, r in worst if e > max(GRAD_NORM_TOL, REF_FACTOR * r)]
    ref_tot = abs(float(g["grad_total"]) - float(g["grad_total64"])) / float(g["grad_total64"])
    total = math.sqrt(sum(v * v for v in got_norm.values()))
    loss_err = abs(float(loss) - float(g["loss64"])) / float(g["loss64"])
    tot_err = abs(total - float(g["grad_total64"])) / float(g["grad_total64"])
    sl = []
    for key, name, idx in (("grad_logits_w_sample", "transformer.to_logits.1.weight", (slice(None, None, 37), slice(None, None, 53))),
                           ("grad_first_q_sample", "transformer.blocks.0.attn1.query.weight", (slice(None, None, 97), slice(None, None, 89))),
                           ("grad_last_fc1_sample", "transformer.blocks.18.mlp.0.weight", (slice(None, None, 211), slice(None, None, 89)))):
        got, want = grads[name][idx].cpu().double(), g[key].double()
        sl.append(float((got - want).abs().max() / want.abs().max()))
    parity_line("%s: loss rel %.1e (%.6f vs the reference's float64 %.6f; its fp32: %.6f), global grad norm rel %.1e, worst of %d "
                "per-tensor norms %.1e (%s, |g| %.1e; the reference's own fp32 is at most %.1e from its float64), %d tensors beyond "
                "max(%.0e, %g x the reference's own distance)%s, slices vs its fp32 %s"
                % (what, loss_err, float(loss), float(g["loss64"]), float(g["loss"]), tot_err, len(worst), worst[0][0], worst[0][1],
                   worst[0][2], ref_worst, len(beyond), GRAD_NORM_TOL, REF_FACTOR,
                   (": worst %.1e vs %.1e (%s)" % (max(beyond)[0], max(beyond)[3], max(beyond)[1])) if beyond else "",
                   ["%.1e" % e for e in sl]))
    for err, n, want, r in worst[:6]:
        print("  grad-norm rel err %.2e (the reference's fp32: %.2e)  |g| %.3e  %s" % (err, r, want, n))
    assert loss_err < LOSS_TOL
    assert tot_err < max(GRAD_NORM_TOL, REF_FACTOR * ref_tot), (tot_err, ref_tot)
    assert not over, over[:4]
    assert max(sl) < max(SLICE_TOL, REF_FACTOR * ref_worst), sl


@pytest.mark.parametrize("profile", ["init", "trained"])
def test_loss_and_gradients_L19_b20_vs_reference(model_init, profile):
    """The loss and every parameter gradient of the benchmarked training shape against the reference's own loss.backward(),
    entered at what the reference's prologue produced (its VQ token ids and its CLIP embedding, so that the comparison is
    the denoiser's alone) -- at the default calibration target (2^6) and at 2^8 / 2^10 (on init-like weights the policy
    constant `calib_log2` is not what the precision hangs on: 2^2 .. 2^10 all pass; on heavy-tailed operands it is a dial,
    see below)."""
    from text_to_sound_synthesis_amd.modeling.train import TrainStep
    tag, meta = names(profile)
    g = golden(tag)
    m = model_init if profile == "init" else build("trained")
    dt = m.transformer
    t, pt, u = injected(g)
    x0, cond = g["tokens"].long().cuda(), g["cond_emb"].float().cuda()
    # init-like weights: every tensor within GRAD_NORM_TOL at every target.  Trained-like weights (Student-t matrices, one MLP unit
    # x 2000: dY whose typical elements sit 2^12 and more under the tensor's largest): the lo planes of those typical elements
    # run out of fp16's range first, so a handful of small / mid-size tensors are further from exact than 4 x the reference's own
    # fp32 (itself up to 1.9e-3 off on these weights) -- bounded at 1e-3 of their own norm, reported, and shrinking with the target
    floor = None if profile == "init" else 1e-3
    for calib in (None, 8, 10):
        dt.reset_time_statistics()
        step = TrainStep(dt, precision="f16x2")
        if calib is not None:
            step.calib_log2 = calib
        loss, grads = step.loss_and_grads(x0, cond, t, pt, u)
        check_grads(g, meta, loss, grads, "train L19 B20 %s (operand maxima calibrated to 2^%d, loss scale 2^%d, site exponents %d..%d)"
                    % (profile, step.calib_log2, step.loss_scale_exp, min(step.policy._site_exp.values()), max(step.policy._site_exp.values())),
                    floor=floor)
        if calib is None:
            # what ONE scale for the whole backward (rounds 2-5) does to the small gradients, for the record: the same step
            # with the per-site exponents dropped
            keep = step.policy._site_exp
            step.policy._site_exp = None
            _, g1 = step.loss_and_grads(x0, cond, t, pt, u)
            step.policy._site_exp = keep
            n1 = {k: float(v.double().norm()) for k, v in g1.items()}
            w1 = max((abs(n1[n] - n64) / n64, n) for n, n64, am in zip(meta["grad_names"], g["grad_norms64"].tolist(), g["grad_amax"].tolist())
                     if am >= 1e-7)
            parity_line("train L19 B20 %s WITHOUT the per-site scales (one loss scale, as in rounds 2-5): worst per-tensor norm %.1e (%s)"
                        % (profile, w1[0], w1[1]))
            del g1
            dt.reset_time_statistics()
            loss, grads = step.loss_and_grads(x0, cond, t, pt, u)           # (the statistics checked below: one step's worth)
            assert torch.allclose(dt.Lt_history.cpu(), g["Lt_history"], rtol=5e-4, atol=1e-6)
            assert torch.equal(dt.Lt_count.cpu(), g["Lt_count"])
            # the saturation monitor saw this backward: its reading sits where the calibration aimed, and every linear's dY
            # carries its own power of two on top of the loss scale (the small ones many bits)
            assert step.check_loss_scale(force=True) is False
            assert step.calib_log2 - 1 <= step.monitor_log[-1] < step.calib_log2 + 3, step.monitor_log
            ex = step.policy._site_exp
            assert len(ex) == 19 * 9 + 1                            # 7 linears + 2 attention backwards per block, + the logits layer
            print("site exponents: logits %d, block 18 %s, block 0 %s" % (ex["logits"], {k[4:]: v for k, v in ex.items() if k.startswith("b18.")},
                                                                        {k[3:]: v for k, v in ex.items() if k.startswith("b0.")}))
        del step, grads
    if profile != "init":
        del m
    torch.cuda.empty_cache()


def test_exact_fp32_backend_L19_b20_vs_reference(model_init):
    """The strict backend (every GEMM and both attention passes on the exact-fp32 MFMA, no fp16 anywhere, no scales) on the same
    golden: the yardstick for what the split backend's numbers above are worth."""
    from text_to_sound_synthesis_amd.modeling.train import TrainStep
    tag, meta = names("init")
    g = golden(tag)
    dt = model_init.transformer
    dt.reset_time_statistics()
    t, pt, u = injected(g)
    step = TrainStep(dt, precision="fp32")
    loss, grads = step.loss_and_grads(g["tokens"].long().cuda(), g["cond_emb"].float().cuda(), t, pt, u)
    check_grads(g, meta, loss, grads, "train L19 B20 init, exact-fp32 backend")
    dt.reset_time_statistics()


def test_solver_step_from_the_reference_batch(model_init):
    """`Solver(model=dalle).step({'image', 'text'})` = the reference's `self.model(batch, return_loss=True)` entry
    (engine/solver_spec.py:308-331): BPE -> CLIP -> VQ encode -> sample_time -> q_sample noise -> loss + backward -> clip ->
    AdamW, against the golden with the product's OWN prologue (its CLIP embedding is 4e-4 from the reference's and a few VQ
    codes sit on the other side of a tie: the loss agrees to that, not to 1e-5), and bit-for-bit against the same step fed
    with the tensors `training_inputs` returns for the same generator state."""
    from text_to_sound_synthesis_amd.modeling.solver import GradClipWindow, Solver
    from text_to_sound_synthesis_amd.modeling.train import TrainStep, training_inputs
    tag, meta = names("init")
    g = golden(tag)
    m = model_init
    dt = m.transformer
    dt.reset_time_statistics()
    t_g, pt_g, u_g = injected(g)
    # (1) the product's own prologue + the golden's timesteps / noise: loss within what the prologue's tolerance allows
    x0, cond, _, _, _ = training_inputs(m, batch_of(meta))
    step = TrainStep(dt, precision="f16x2")
    loss, grads = step.loss_and_grads(x0, cond, t_g, pt_g, u_g)
    total = math.sqrt(sum(float(v.double().pow(2).sum()) for v in grads.values()))
    e_loss = abs(float(loss) - float(g["loss"])) / float(g["loss"])
    e_tot = abs(total - float(g["grad_total"])) / float(g["grad_total"])
    parity_line("train L19 B20 from mel + captions (own CLIP + VQ encode): loss rel %.1e, global grad norm rel %.1e" % (e_loss, e_tot))
    assert e_loss < 5e-3 and e_tot < 2e-2
    # (2) Solver.step(batch dict) == Solver.step(*training_inputs(batch)) for the same generator state, weights and statistics
    keep = {k: v.detach().clone() for k, v in dt.state_dict().items()}

    def run(as_dict):
        dt.load_state_dict(keep)
        dt.transformer.invalidate()
        gen = torch.Generator(device="cuda").manual_seed(99)
        solver = Solver(TrainStep(dt, precision="f16x2"), lr=1e-4, clip_grad_norm=GradClipWindow(0, 5000, 0.5), model=m, generator=gen)
        if as_dict:
            out = solver.step(batch_of(meta))
        else:
            out = solver.step(*training_inputs(m, batch_of(meta), generator=gen))
        w = dict(dt.named_parameters())["transformer.blocks.7.mlp.0.weight"].detach().clone()
        return float(out["loss"]), float(out["grad_norm"]), w
    a, b = run(True), run(False)
    assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2])
    assert not torch.equal(a[2], keep["transformer.blocks.7.mlp.0.weight"])         # the update happened
    dt.load_state_dict(keep)
    dt.transformer.invalidate()
    with pytest.raises(ValueError):
        Solver(TrainStep(dt, precision="f16x2")).step(batch_of(meta))                # a batch dict needs the model


def test_graph_solver_from_the_reference_batch_three_iterations(model_init):
    """GraphSolver.step(batch dict): the prologue runs eagerly on the stream, the captured iteration replays on its output --
    three iterations with new mel + captions each equal the eager Solver's (same generator, same weights) to rounding; with the
    next batch's prologue PREFETCHED on a side stream (GraphSolver.prefetch) the numbers are the graphed ones (to the last bit
    but for the atomically summed token-embedding gradient)."""
    from text_to_sound_synthesis_amd.modeling.solver import GradClipWindow, GraphSolver, Solver
    from text_to_sound_synthesis_amd.modeling.train import TrainStep
    m = model_init
    dt = m.transformer
    dt.reset_time_statistics()
    keep = {k: v.detach().clone() for k, v in dt.state_dict().items()}

    mels = [torch.rand((B, 1, 80, 848), device="cuda", generator=torch.Generator(device="cuda").manual_seed(70 + i)) * 2 - 1 for i in range(3)]
    torch.cuda.synchronize()

    def run(cls, prefetch=False):
        dt.load_state_dict(keep)
        dt.transformer.invalidate()
        gen = torch.Generator(device="cuda").manual_seed(7)
        solver = cls(TrainStep(dt, precision="f16x2"), lr=1e-4, clip_grad_norm=GradClipWindow(0, 5000, 0.5), model=m, generator=gen)
        batches = [{"image": mels[it], "text": synth.synth_captions(B, seed=40 + it)} for it in range(3)]
        outs = []
        for it in range(3):
            out = solver.step(batches[it])
            if prefetch and it + 1 < 3:        # the next batch's BPE / CLIP / VQ encode on a side stream, beside this replay
                solver.prefetch(batches[it + 1])
            outs.append((float(out["loss"]), float(out["grad_norm"])))
        return outs, getattr(getattr(solver, "iteration_graph", None), "recaptures", 0)
    eager, _ = run(Solver)
    graphed, rec = run(GraphSolver)
    ahead, rec2 = run(GraphSolver, prefetch=True)
    print("eager %s\ngraph %s\ngraph + prefetch %s" % (eager, graphed, ahead))
    for (le, ne), (lg, ng) in zip(eager, graphed):
        assert abs(le - lg) < 1e-5 * abs(le) and abs(ne - ng) < 1e-4 * abs(ne)
    for (lg, ng), (la, na) in zip(graphed, ahead):      # the same kernels on the same inputs, only enqueued earlier (the token
        assert abs(lg - la) <= 1e-6 * abs(lg) and abs(ng - na) <= 1e-6 * abs(ng)     # embedding's gradient is summed with atomics)
    assert rec == 0 and rec2 == 0
    dt.load_state_dict(keep)
    dt.transformer.invalidate()
