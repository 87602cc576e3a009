"""The training step's fp16-split sites across the operand range, against float64: (a) one linear through the GEMM backend's own
surface (modeling/train_gemm.py: prepare / prep_x / prep_dy / fwd / dx / dw_many / db of `_SplitGemm`, with `_Fp32Gemm` behind the
same surface as the fp32-class yardstick), with the scales composed the way the step composes them -- the weight's 2^s (`wexp`),
the site's 2^e from LossScalePolicy._exp_from_amax, 2^-e in the dX epilogue, inv 2^-e in the dW epilogue across split-K partials
and ds_gemm_f16x2_multi grouping, the bias column sums taken before the scale; (b) ds_attention_bwd_f16x2_mon in the softmax
regimes of the inference attention crossed with V and dO scales, with ds_attention_bwd (exact fp32) as the yardstick kernel;
(c) a whole TrainStep whose FC2 operand gelu2(u) exceeds 65504, against the float64 oracle.

The error model (csrc/common.h ds_split_hi / ds_split_lo): a value a is used as fp16(a) + fp16(a - fp16(a)); fp32-class for |a| in
about [2^-3, 65504]; below 2^-3 the lo plane is subnormal and a keeps 2^-25 of absolute precision; above 65504 the split saturates.
The constants EPS32, LO_ABS, C_LO, RMS_LO, IN_RANGE, SCALES / SETS, `torch_split` and the per-block assertion form `judge` are
copied from tests/test_hip_denoiser_range.py (which copied them from tests/test_hip_codec_vocoder_range.py).  The float64 emulation
of the kernels (`emu_*`: torch_split of both operands, hi hi + hi lo + lo hi in float64, then the epilogue scales) needs no GPU:
`check_bounds_on_emulation()` reruns the check that every bound of (a) and (b) holds for it with a margin of 2 or more
(python tests/test_hip_train_range.py).  GPU only (-m gpu)."""
import math
import os
import sys

import pytest
import torch

if __name__ == "__main__":                       # the emulation check, run as a script: the paths tests/conftest.py sets up
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "oracle"), os.path.join(_root, "tests")]

import diffsound_oracle as O
from conftest import parity_line, synth_sd
from text_to_sound_synthesis_amd import synth

pytestmark = pytest.mark.gpu
NO_GRAD = True

# ---- copied from tests/test_hip_denoiser_range.py (see there and tests/test_hip_codec_vocoder_range.py for RMS_LO) ----
EPS32 = 2.0 ** -24
LO_ABS = 2.0 ** -25          # absolute precision of a subnormal fp16 lo plane (half its spacing, 2^-24)
C_LO = 1.0                   # the documented bound:  |err| <= C_LO * 2^-25 * sum |w|  per split (+ the fp32-class term)
RMS_LO = 2.0 ** -25
SCALES = ["2^-12", "2^-6", "1", "2^14", "6e4", "hot6e4"]
SCALE = {"2^-12": 2.0 ** -12, "2^-6": 2.0 ** -6, "1": 1.0, "2^14": 2.0 ** 14, "6e4": 6e4, "hot6e4": 1.0}
HOT = 5
SETS = SCALES + ["mixed"]    # "mixed": even rows at 2^-12, odd rows at 1 (one launch, both sides of 2^-3)
IN_RANGE = 2.0 ** -3         # at and above it no lo-plane allowance at all


def rnd(shape, key, scale=1.0):
    return (synth.synth_uniform(shape, key=key) * 2 - 1) * scale


def torch_split(a):
    """ds_split_hi / ds_split_lo (csrc/common.h) in torch: hi = fp16(clamp(a)), lo = fp16(clamp(a - hi))"""
    hi = a.clamp(-65504.0, 65504.0).half()
    lo = (a - hi.float()).clamp(-65504.0, 65504.0).half()
    return torch.stack((hi, lo)).contiguous()


def gelu2(y):
    return y * torch.sigmoid(1.702 * y)


@pytest.fixture(scope="module")
def L():
    from text_to_sound_synthesis_amd import _lib
    _lib.lib()
    return _lib


# ============================== (a) one linear through the training GEMM backend's surface ==============================
# name -> (M, N, K, parts of the fused weight): ragged M with rows_pad padding and 2 K-ranges; two samples' rows; the 192-tile
# unsplit rule on the 96 x 128 tile; a two-part fused weight (ds_pack_operand's sub-range form), need_dx=False as kv2 runs it
LIN_SHAPES = {"70x96x64": (70, 96, 64, 1), "530x256x1024": (530, 256, 1024, 1), "265x3072x1024": (265, 3072, 1024, 1),
              "77x2048x512.fused": (77, 2048, 512, 2)}
# W: flat; one row x 2^10; max |W| exactly a power of two / one ulp under one (the two edges of s = 13 - floor(log2 max|W|))
WKINDS = ["flat", "wide", "pow2", "under_pow2"]
XFORMS = [(s, pro) for pro in ("plain", "gelu2") for s in SETS]        # gelu2: u through PACK_GELU2, gelu2(u) spanning the same sets
# dY: raw magnitudes under the policy's own exponent; the scaled maximum AT the monitor window's floor 2^0 and just under its
# ceiling 2^15 (exponents placed by hand: that is what the window promises to be fp32-class); rows of two scales 2^14 apart
DYSETS = ["2^-30", "2^-14", "1", "2^10", "floor", "ceiling", "rows2^14"]
DYMAG = {"2^-30": 2.0 ** -30, "2^-14": 2.0 ** -14, "1": 1.0, "2^10": 2.0 ** 10}
INV = 2.0 ** -7               # the inverse loss scale that rides in the dW epilogue with 2^-e
_LIN = {}


def row_scales(M, sname):
    """per-row operand scale [M]"""
    if sname == "mixed":
        s = torch.ones(M, dtype=torch.float64)
        s[0::2] = 2.0 ** -12
        return s
    return torch.full((M,), SCALE[sname], dtype=torch.float64)


def make_w(N, K, wkind, parts):
    ck = ("w", N, K, wkind, parts)
    if ck not in _LIN:
        W = rnd((N, K), "tr.W", 0.1)
        if wkind == "wide":
            W[3] *= 2.0 ** 10
        elif wkind == "pow2":
            W[1, 2] = 0.125
        elif wkind == "under_pow2":
            W[1, 2] = float(torch.nextafter(torch.tensor(0.125), torch.tensor(0.0)))
        m = float(W.abs().max())
        s = 13 - math.floor(math.log2(m))
        assert 2.0 ** 13 <= m * 2.0 ** s < 2.0 ** 14
        if wkind == "pow2":
            assert m == 0.125 and s == 16 and m * 2.0 ** s == 2.0 ** 13
        elif wkind == "under_pow2":
            assert m < 0.125 and s == 17 and m * 2.0 ** s > 2.0 ** 14 * (1 - 2.0 ** -23)
        _LIN[ck] = dict(W=W, b=rnd((N,), "tr.b"), s=s, wkind=wkind, parts=parts)
    return _LIN[ck]


def make_x(M, K, sname, pro):
    """the forward operand: `src` is what prep_x gets (x itself, or u with x = gelu2(u)), `x64` the operand in float64"""
    ck = ("x", M, K, sname, pro)
    if ck not in _LIN:
        rs = row_scales(M, sname)
        src = rnd((M, K), "tr.X") * rs.float()[:, None]
        if sname == "hot6e4":
            src[:, HOT] *= 6e4
        if pro == "gelu2":
            src = src * torch.where(rs < 1.0, 2.0, 1.0).float()[:, None]      # gelu2(u) ~ u / 2 for small u, ~ u for large u > 0
        x64 = gelu2(src.double()) if pro == "gelu2" else src.double()
        assert float(x64.abs().max()) < 65504.0
        _LIN[ck] = dict(src=src, x64=x64, rs=rs, sname=sname, pro=pro)
    return _LIN[ck]


def make_dy(M, N, dname):
    """dY (fp32), the site's exponent e, and the row classes [M] (1 everywhere but for the rows-2^14-apart set)"""
    from text_to_sound_synthesis_amd.modeling.loss_scale import LossScalePolicy
    ck = ("dy", M, N, dname)
    if ck not in _LIN:
        rc = torch.ones(M, dtype=torch.float64)
        if dname in DYMAG:
            dy = rnd((M, N), "tr.dY", DYMAG[dname])
        elif dname == "rows2^14":
            rc[1::2] = 2.0 ** -14
            dy = rnd((M, N), "tr.dY") * rc.float()[:, None]
        else:
            dy = rnd((M, N), "tr.dY", 0.99 * 2.0 ** -14)
            dy[0, 0] = 2.0 ** -14 if dname == "floor" else float(torch.nextafter(torch.tensor(2.0 ** -14), torch.tensor(0.0)))
        top = float(dy.abs().max())
        e = {"floor": 14, "ceiling": 29}.get(dname)
        if e is None:
            e = LossScalePolicy()._exp_from_amax(top)            # the policy's own choice: max |dY 2^e| in [2^6, 2^7)
            assert 2.0 ** 6 <= top * 2.0 ** e < 2.0 ** 7
        elif dname == "floor":
            assert top * 2.0 ** e == 1.0
        else:
            assert 2.0 ** 15 * (1 - 2.0 ** -23) < top * 2.0 ** e < 2.0 ** 15
        _LIN[ck] = dict(dy=dy, e=e, rc=rc, dname=dname)
    return _LIN[ck]


def below(a):
    """where a split value has a subnormal lo plane: 0 < |a| < 2^-3 (an exact zero splits exactly)"""
    return ((a.abs() < IN_RANGE) & (a != 0)).double()


def fwd_ref(x, w, dev):
    """what `judge` wants of one forward case: float64 x W^T + b and the row sums of |W|, ||W||_2"""
    W = w["W"].to(dev).double()
    return dict(ref=(x["x64"].to(dev) @ W.t() + w["b"].to(dev).double()).cpu(), rs=x["rs"], l1=W.abs().sum(1).cpu(), l2=W.norm(dim=1).cpu())


def dx_ref(d, w, dev):
    """float64 dY W, and the documented allowance per output [M][K] (issue / module docstring):
    2^-25 (2^-e sum_{n: 0 < |dY 2^e| < 2^-3} |W[n,k]|  +  2^-s sum_{n: 0 < |W 2^s| < 2^-3} |dY[m,n]|)  and its square-sum form"""
    dy, W, e, s = d["dy"].to(dev).double(), w["W"].to(dev).double(), d["e"], w["s"]
    my, mw = below(dy * 2.0 ** e), below(W * 2.0 ** s)
    lo = LO_ABS * (2.0 ** -e * (my @ W.abs()) + 2.0 ** -s * (dy.abs() @ mw))
    l2sq = 4.0 ** -e * (my @ W.pow(2)) + 4.0 ** -s * (dy.pow(2) @ mw)
    return dict(ref=(dy @ W).cpu(), lo=lo.cpu(), l2sq=l2sq.cpu())


def dw_ref(d, x, dev, inv=INV):
    """float64 inv dY^T X and the same allowance over the contraction index m: the dY side carries 2^-e, the X side is unscaled"""
    dy, X, e = d["dy"].to(dev).double(), x["x64"].to(dev), d["e"]
    my, mx = below(dy * 2.0 ** e), below(X)
    lo = inv * LO_ABS * (2.0 ** -e * (my.t() @ X.abs()) + dy.abs().t() @ mx)
    l2sq = inv * inv * (4.0 ** -e * (my.t() @ X.pow(2)) + dy.pow(2).t() @ mx)
    return dict(ref=(inv * (dy.t() @ X)).cpu(), lo=lo.cpu(), l2sq=l2sq.cpu())


# ---- the float64 emulation of the split kernels (no GPU) ----
def emu_product(a, w):
    """a [M][K], w [N][K] (fp32, already scaled as the kernel's operands are) -> hi hi + hi lo + lo hi of their splits, float64"""
    (ah, al), (wh, wl) = torch_split(a).double(), torch_split(w).double()
    return ah @ wh.t() + ah @ wl.t() + al @ wh.t()


def emu_x(x):
    return gelu2(x["src"]) if x["pro"] == "gelu2" else x["src"]


def emu_fwd(x, w):
    return emu_product(emu_x(x), w["W"] * 2.0 ** w["s"]) * 2.0 ** -w["s"] + w["b"].double()


def emu_dx(d, w):
    return emu_product(d["dy"] * 2.0 ** d["e"], (w["W"] * 2.0 ** w["s"]).t().contiguous()) * 2.0 ** -w["s"] * 2.0 ** -d["e"]


def emu_dw(d, x, inv=INV):
    return emu_product((d["dy"] * 2.0 ** d["e"]).t().contiguous(), emu_x(x).t().contiguous()) * (inv * 2.0 ** -d["e"])


# ---- the assertion forms ----
def blocks_of(c, wkind):
    """(label, row mask, column mask, operand scale of those rows): mixed rows and the wide weight's big row are judged apart,
    each against its own largest |ref|, so that neither hides the other"""
    M, N = c["ref"].shape
    cols = [("", torch.ones(N, dtype=torch.bool))]
    if wkind == "wide":
        big = torch.zeros(N, dtype=torch.bool)
        big[3] = True
        cols = [(" big row", big), (" other rows", ~big)]
    out = []
    for s in sorted(set(c["rs"].tolist())):
        rm = c["rs"] == s
        for cl, cm in cols:
            out.append((("rows@%.3g" % s if len(set(c["rs"].tolist())) > 1 else "") + cl, rm, cm, s))
    return out


def judge(name, y, y32, c, wkind, lip=1.0, extra=None, rms_scale=1.0):
    """The assertion forms of test_hip_denoiser_range.py's judge (test_split_kernel_across_operand_range of the codec's file), per
    block, unchanged.  Operand scale >= 2^-3: relative max error vs float64 within max(3e-6, 1.2 x the exact-fp32 kernel's), no
    lo-plane allowance.  Below: per output within C_LO 2^-25 sum_k |w| + the fp32-class term max(3e-6 max|ref|, 1.2 x the fp32
    kernel's max error), and RMS over outputs of err / ||w||_2 within RMS_LO + 1.2 x the fp32 kernel's.
    rms_scale: 1 in every GPU test; the emulation check alone passes another factor for the RMS figures (see there).
    Returns the figures (rel, rel32, worst-of-bound or None, rms / 2^-25 or None) of the worst block."""
    y, y32, ref = y.cpu().double(), y32.cpu().double(), c["ref"]
    assert torch.isfinite(y).all(), name
    fig = [0.0, 0.0, None, None]
    dist = (y - ref).abs() if extra is None else ((y - ref).abs() - extra).clamp(min=0)
    for label, rm, cm, s in blocks_of(c, wkind):
        err, err32, rf = dist[rm][:, cm], (y32 - ref)[rm][:, cm].abs(), ref[rm][:, cm]
        top = float(rf.abs().max())
        e, e32 = float(err.max()) / top, float(err32.max()) / top
        if e >= fig[0]:
            fig[0], fig[1] = e, e32
        if s >= IN_RANGE:
            assert e <= max(3e-6, 1.2 * e32), "%s %s: %.3g vs fp32 %.3g" % (name, label, e, e32)
        else:
            fp32_term = max(3e-6 * top, 1.2 * float(err32.max()))
            worst = float((err / (C_LO * LO_ABS * lip * c["l1"][cm][None, :] + fp32_term)).max())
            l2 = c["l2"][cm][None, :]
            r, r32 = rms_scale * float((err / l2).pow(2).mean().sqrt()), float((err32 / l2).pow(2).mean().sqrt())
            fig[2], fig[3] = max(fig[2] or 0.0, worst), max(fig[3] or 0.0, r / RMS_LO)
            assert worst <= 1.0, "%s %s: %.3g of the documented bound" % (name, label, worst)
            assert r <= RMS_LO * lip + 1.2 * r32, "%s %s: RMS %.3g x 2^-25 (fp32 %.3g)" % (name, label, r / RMS_LO, r32 / RMS_LO)
    return fig


def judge_bwd(name, y, y32, c, blocks, rms_scale=1.0):
    """dX and dW: per output within C_LO x the allowance of dx_ref / dw_ref + the fp32-class term max(3e-6 max|ref|, 1.2 x the
    `_Fp32Gemm` error), per block (label, row mask, column mask), each against its own largest |ref|; and the RMS form: the
    sub-2^-3 roundings are independent, so over a block RMS(err) <= RMS_LO sqrt(mean of the allowance's square-sum form) + the
    fp32-class term in RMS, max(1e-6 max|ref|, 1.2 x RMS of the `_Fp32Gemm` error) -- 1e-6: a third of the max form's 3e-6, the
    least a maximum over this many outputs stands above their RMS.  -> (rel, rel32, worst-of-bound, RMS(err) / its bound)"""
    y, y32, ref = y.cpu().double(), y32.cpu().double(), c["ref"]
    assert torch.isfinite(y).all(), name
    fig = [0.0, 0.0, 0.0, 0.0]
    for label, rm, cm in blocks:
        sub = lambda a: a[rm][:, cm]
        err, err32, rf = sub((y - ref).abs()), sub((y32 - ref).abs()), sub(ref)
        top = float(rf.abs().max())
        e, e32 = float(err.max()) / top, float(err32.max()) / top
        if e >= fig[0]:
            fig[0], fig[1] = e, e32
        worst = float((err / (C_LO * sub(c["lo"]) + max(3e-6 * top, 1.2 * float(err32.max())))).max())
        r = rms_scale * float(err.pow(2).mean().sqrt())
        r_bound = RMS_LO * float(sub(c["l2sq"]).mean().sqrt()) + max(1e-6 * top, 1.2 * float(err32.pow(2).mean().sqrt()))
        fig[2], fig[3] = max(fig[2], worst), max(fig[3], r / r_bound)
        assert worst <= 1.0, "%s %s: %.3g of the documented bound (rel %.3g, fp32 %.3g)" % (name, label, worst, e, e32)
        assert r <= r_bound, "%s %s: RMS %.3g of its bound" % (name, label, r / r_bound)
    return fig


def row_blocks(rc, ncol):
    cm = torch.ones(ncol, dtype=torch.bool)
    cls = sorted(set(rc.tolist()))
    return [("rows@%.3g" % s if len(cls) > 1 else "", rc == s, cm) for s in cls]


def dw_blocks(x, N, K):
    """dW [N][K]: the contraction mixes the rows; a hot feature column of X is a column of dW and is judged apart"""
    rm, hot = torch.ones(N, dtype=torch.bool), torch.zeros(K, dtype=torch.bool)
    hot[HOT] = True
    return [(" hot column", rm, hot), (" other columns", rm, ~hot)] if x["sname"] == "hot6e4" else [("", rm, ~torch.zeros_like(hot))]


def report_lin(title, figs, bwd=False):
    rel, rel32 = max(f[0] for f in figs.values()), max(f[1] for f in figs.values())
    line = "%s: %d products, worst rel max err vs float64 %.2e (_Fp32Gemm %.2e)" % (title, len(figs), rel, rel32)
    lo = [f for f in figs.values() if f[2] is not None]
    if lo:
        line += "; worst |err| / (lo allowance + fp32 term) %.3f, RMS %.3f %s" % (
            max(f[2] for f in lo), max(f[3] for f in lo), "of its bound" if bwd else "x 2^-25 ||w||_2")
    print(line)
    parity_line(line)


# ---- the backends behind their surface ----
def backends(L, w, wexp_check=True):
    """(_SplitGemm, its _Linear prepared under refresh_scales' own exponent), (_Fp32Gemm, its _Linear) for one weight"""
    from text_to_sound_synthesis_amd.modeling.train_gemm import _Fp32Gemm, _Linear, _SplitGemm
    W, b, parts = w["W"].cuda(), w["b"].cuda(), w["parts"]
    N = W.shape[0]

    def lin():
        if parts == 1:
            return _Linear("site", W, b)
        step = N // parts
        return _Linear("site", [W[i * step:(i + 1) * step].contiguous() for i in range(parts)],
                       [b[i * step:(i + 1) * step].contiguous() for i in range(parts)])
    G, G32, l, l32 = _SplitGemm(), _Fp32Gemm(), lin(), lin()
    G.refresh_scales([l])
    assert G.wexp["site"] == w["s"]
    G.prepare(l)
    G32.prepare(l32)
    return (G, l), (G32, l32)


def prep_x_of(G, l, x):
    from text_to_sound_synthesis_amd.modeling.train_gemm import PACK_GELU2, PACK_PLAIN
    return G.prep_x(l, x["src"].cuda(), pro=PACK_GELU2 if x["pro"] == "gelu2" else PACK_PLAIN)


@pytest.mark.parametrize("sname,pro", XFORMS)
@pytest.mark.parametrize("shape", list(LIN_SHAPES))
def test_train_linear_forward_across_operand_range(L, shape, sname, pro):
    """_SplitGemm.fwd (bias epilogue, split2 = 2^-s) on every X form against float64 x W^T + b, for the four weight kinds, under
    the unchanged `judge` forms with `_Fp32Gemm.fwd` as the fp32 kernel.  The 530-row shape runs as two samples of 265 rows (the
    step's rows_per_sample dispatch)."""
    M, N, K, parts = LIN_SHAPES[shape]
    x = make_x(M, K, sname, pro)
    figs = {}
    for wkind in WKINDS:
        w = make_w(N, K, wkind, parts)
        (G, l), (G32, l32) = backends(L, w)
        G.rows_per_sample = 265 if M % 265 == 0 else 0
        c = fwd_ref(x, w, "cuda")
        y = G.fwd(l, prep_x_of(G, l, x))
        y32 = G32.fwd(l32, prep_x_of(G32, l32, x))
        figs[wkind] = judge("fwd %s X %s/%s W %s" % (shape, sname, pro, wkind), y, y32, c, wkind)
    report_lin("train linear fwd %s, X %s (%s)" % (shape, sname, pro), figs)


def run_bwd(L, G, l, G32, l32, d, x, need_dx):
    """prep_dy(scale = 2^e) -> dx(unscale = 2^-e), dw_many([inv 2^-e]), db on the split backend; the same surface on _Fp32Gemm
    (which scales nothing: its item carries inv alone) -> {dx, dw, db, amax}, {dx, dw, db}"""
    N, K = l.N, l.K
    dyc, e = d["dy"].cuda(), d["e"]
    amax = torch.zeros(1, device="cuda")
    dyh = G.prep_dy(l, dyc, amax=amax, need_row=need_dx, scale=2.0 ** e)
    out = dict(dx=G.dx(l, dyh, unscale=2.0 ** -e) if need_dx else None, db=G.db(l, dyh), amax=float(amax.item()), dyh=dyh)
    out32 = {}
    if x is not None:
        dW, dW32 = torch.full((N, K), float("nan"), device="cuda"), torch.full((N, K), float("nan"), device="cuda")
        G.dw_many([(l, prep_x_of(G, l, x), dyh, INV * 2.0 ** -e, dW)])
        G32.dw_many([(l32, prep_x_of(G32, l32, x), G32.prep_dy(l32, dyc), INV, dW32)])
        out["dw"], out32["dw"] = dW, dW32
    out32["dx"] = G32.dx(l32, G32.prep_dy(l32, dyc)) if need_dx else None
    out32["db"] = G32.db(l32, G32.prep_dy(l32, dyc))
    return out, out32


def small_rows_line(what, y, c, rc):
    """the rows-2^14-apart finding: how far the SMALL rows are from float64, relative to their own largest element"""
    small = rc < 1.0
    ref = c["ref"][small]
    return "%s small rows: max err %.2e of their own max |ref| (allowance %.2e)" % (
        what, float((y.cpu().double()[small] - ref).abs().max() / ref.abs().max()), float(c["lo"][small].max() / ref.abs().max()))


@pytest.mark.parametrize("dname", DYSETS)
@pytest.mark.parametrize("shape", list(LIN_SHAPES))
def test_train_linear_backward_across_operand_range(L, shape, dname):
    """prep_dy(scale = 2^e) / dx(unscale = 2^-e) / dw_many([inv 2^-e]) / db of `_SplitGemm` for one dY set: dX against float64 dY W
    for the four weight kinds, dW against float64 inv dY^T X for every X form (plain and through PACK_GELU2), the bias gradient
    against float64 column sums (within 1e-5 sum_m |dY|: the colsum bound of tests/test_hip_train_kernels.py), and the monitor's
    slot = max |dY 2^e| exactly.  The split-K partial layouts (2 K-ranges; unsplit at 192 tiles) are judged through the summed result.

    The rows-2^14-apart set is the one place where the result is NOT fp32-class, by the documented model: one power of two per site
    puts the site's maximum at 2^T (T = 6 here), and an element 2^-14 under it is split at 2^(T-14) < 2^-3, where it keeps 2^-25
    absolutely -- 2^-(25+T) of the site's maximum, i.e. 2^(14-25-T) = 2^-17 of its OWN size.  The allowance of dx_ref carries
    exactly that (the small rows are their own block); the measured distance of the small rows is printed and recorded in
    DESIGN.md section 7 as a finding -- dW is not affected beyond the large rows' fp32 term (the contraction mixes the rows)."""
    M, N, K, parts = LIN_SHAPES[shape]
    need_dx = parts == 1
    d = make_dy(M, N, dname)
    figs_dx, figs_dw, notes = {}, {}, []
    dy64 = d["dy"].double()
    for wkind in WKINDS:
        w = make_w(N, K, wkind, parts)
        (G, l), (G32, l32) = backends(L, w)
        G.rows_per_sample = 265 if M % 265 == 0 else 0
        out, out32 = run_bwd(L, G, l, G32, l32, d, None, need_dx)
        assert out["amax"] == float(d["dy"].abs().max()) * 2.0 ** d["e"]
        db = out["db"].cpu().double()
        assert torch.isfinite(db).all() and bool(((db - dy64.sum(0)).abs() <= 1e-5 * dy64.abs().sum(0)).all()), (shape, dname, wkind)
        if need_dx:
            c = dx_ref(d, w, "cuda")
            figs_dx[wkind] = judge_bwd("dx %s dY %s W %s" % (shape, dname, wkind), out["dx"], out32["dx"], c, row_blocks(d["rc"], K))
            if dname == "rows2^14" and wkind == "flat":
                notes.append(small_rows_line("dX", out["dx"], c, d["rc"]))
    w = make_w(N, K, "flat", parts)
    (G, l), (G32, l32) = backends(L, w)
    for sname, pro in XFORMS:
        x = make_x(M, K, sname, pro)
        out, out32 = run_bwd(L, G, l, G32, l32, d, x, False)
        c = dw_ref(d, x, "cuda")
        figs_dw[(sname, pro)] = judge_bwd("dw %s dY %s X %s/%s" % (shape, dname, sname, pro), out["dw"], out32["dw"], c, dw_blocks(x, N, K))
    if figs_dx:
        report_lin("train linear dX %s, dY %s (e = %d)" % (shape, dname, d["e"]), figs_dx, bwd=True)
    report_lin("train linear dW %s, dY %s (e = %d)" % (shape, dname, d["e"]), figs_dw, bwd=True)
    for n in notes:
        print(n)
        parity_line("train linear %s, dY rows 2^14 apart (FINDING, not fp32-class by the documented 2^-(25+T) form): %s" % (shape, n))


def test_train_linear_bias_gradient_ignores_the_site_scale(L):
    """The bias gradient's column sums are taken BEFORE ds_pack_operand applies `scale`: bit-identical for e = 0 and e = 20, finite
    and within the colsum bound of float64 although dY 2^20 is far past 65504 (the planes saturate -- nothing reads them here).
    Sums taken after the scale would come out 2^20 times too large."""
    M, N, K, parts = LIN_SHAPES["530x256x1024"]
    d = make_dy(M, N, "1")
    (G, l), _ = backends(L, make_w(N, K, "flat", parts))
    dyc, dy64 = d["dy"].cuda(), d["dy"].double()
    assert float(d["dy"].abs().max()) * 2.0 ** 20 > 65504.0
    db = {e: G.db(l, G.prep_dy(l, dyc, scale=2.0 ** e)).cpu() for e in (0, 20)}
    assert torch.equal(db[0], db[20]) and torch.isfinite(db[20]).all()
    worst = float(((db[20].double() - dy64.sum(0)).abs() / dy64.abs().sum(0)).max())
    parity_line("train linear db under e = 0 / 20: bit-identical, worst |err| / sum_m |dY| %.2e" % worst)
    assert worst <= 1e-5


def test_train_linear_monitor_reads_a_dy_past_the_ceiling(L):
    """A scaled dY pushed past 2^16 saturates the planes: nothing is claimed about accuracy, but the slot the pack folds
    max |dY 2^e| into reads >= 2^15 -- what makes LossScalePolicy.check_loss_scale drop the calibration -- and it does."""
    from text_to_sound_synthesis_amd.modeling.loss_scale import LossScalePolicy
    M, N, K, parts = LIN_SHAPES["70x96x64"]
    d = make_dy(M, N, "1")
    (G, l), _ = backends(L, make_w(N, K, "flat", parts))
    pol = LossScalePolicy()
    pol._amax_live, pol.loss_scale_exp = torch.zeros(1, device="cuda"), 0
    G.prep_dy(l, d["dy"].cuda(), amax=pol._amax_live, scale=2.0 ** 17)
    seen = float(pol._amax_live.item())
    assert seen >= 2.0 ** 16 > 2.0 ** 15 and seen == float(d["dy"].abs().max()) * 2.0 ** 17
    assert pol.check_loss_scale(force=True) and pol.loss_scale_exp is None and "monitor high" in pol.last_trip


def test_train_linear_dw_many_grouping(L):
    """One dw_many call with five products of one tile configuration (530 x 256 x 1024, 2 K-ranges each: one four-wide
    ds_gemm_f16x2_multi grid + the single-launch remainder, five finish() reductions) and one of another (265 x 3072 x 1024: the
    96 x 128 tile, unsplit), every item with its own dY set, exponent and X form: each result against float64 under judge_bwd's
    bounds, and bit-identical to the same product handed in alone."""
    items, alone, meta = [], [], []
    cases = [("530x256x1024", dn, xf) for dn, xf in zip(["2^-30", "1", "floor", "ceiling", "2^10"],
                                                         [("1", "plain"), ("2^-12", "plain"), ("mixed", "gelu2"), ("6e4", "plain"), ("hot6e4", "plain")])]
    cases.append(("265x3072x1024", "2^-14", ("2^14", "gelu2")))
    keep = []
    for shape, dname, (sname, pro) in cases:
        M, N, K, parts = LIN_SHAPES[shape]
        w, d, x = make_w(N, K, "flat", parts), make_dy(M, N, dname), make_x(M, K, sname, pro)
        (G, l), (G32, l32) = backends(L, w)
        dyh = G.prep_dy(l, d["dy"].cuda(), scale=2.0 ** d["e"])
        xh = prep_x_of(G, l, x)
        dW, dW1, dW32 = (torch.full((N, K), float("nan"), device="cuda") for _ in range(3))
        items.append((l, xh, dyh, INV * 2.0 ** -d["e"], dW))
        G.dw_many([(l, xh, dyh, INV * 2.0 ** -d["e"], dW1)])
        G32.dw_many([(l32, prep_x_of(G32, l32, x), G32.prep_dy(l32, d["dy"].cuda()), INV, dW32)])
        alone.append(dW1)
        meta.append((shape, dname, sname, pro, d, x, dW32, N, K))
        keep.append(G)
    G = keep[0]
    assert len({(L.lib().ds_gemm_f16x2_auto_tile(it[0].N, it[0].K, G.split_k(it[0].N, it[0].K, it[2].rows)),
                 G.split_k(it[0].N, it[0].K, it[2].rows)) for it in items}) == 2
    assert [G.split_k(it[0].N, it[0].K, it[2].rows) for it in items] == [2] * 5 + [1]
    G.dw_many(items)
    figs = {}
    for it, one, (shape, dname, sname, pro, d, x, dW32, N, K) in zip(items, alone, meta):
        assert torch.equal(it[4], one), (shape, dname)
        figs[(shape, dname)] = judge_bwd("dw_many %s dY %s X %s/%s" % (shape, dname, sname, pro), it[4], dW32, dw_ref(d, x, "cuda"),
                                         dw_blocks(x, N, K))
    report_lin("train linear dw_many, 5 + 1 products in one call (bit-identical to single calls)", figs, bwd=True)


# ============================================= (b) the attention backward ==============================================
ATT_SHAPES = [(1, 2, 72, 77), (1, 2, 40, 33)]
REGIMES = ["flat", "unit", "sharp", "winner", "cross"]       # the named regimes of tests/test_hip_denoiser_range.py
VSCALES = ["2^-12", "1", "6e4"]
DO_PLACES = ["2^0", "2^6", "under 2^15"]                     # where max |dO do_scale| sits: the window's floor, the target, the ceiling
DO_RAW = 2.0 ** -10                                          # max |dO| itself (a gradient under some loss scale)
DO_SCALE = {"2^0": 2.0 ** 10, "2^6": 2.0 ** 16, "under 2^15": 2.0 ** 25}
# A gradient passes when its max-abs distance to float64 autograd is within F x d32 + the lo-term.  d32: the max-abs distance of a
# plain fp32 torch autograd evaluation of the same case, floored at fp32's own rounding, EPS32 max |want|.  In the sharp and
# winner regimes the floor is EPS32 x the gradient's magnitude BEFORE the softmax backward's cancellation instead (`mag`: dS = P
# (dP - delta) with every product taken over absolute values): there dQ and dK cancel to ~1e-20 of their terms, torch's fp32
# softmax returns the leading probability as exactly 1 and its backward an exact 0, and no kernel that forms dP - delta from two
# rounded numbers can be asked for digits 2^-24 under them.  (Stated per regime, before any measurement.)
# F = the next integer above 1.5 x the worst measured kernel / d32 ratio (net of the lo-term) over every case below on an MI355X,
# capped at the 20 that test_attention_backward_dS_is_normalised_per_wave grants; DESIGN.md section 7 has the measured table:
# worst 2.31 for dQ / dK; dV 1.65 outside the sharp regimes, 9.36 in the sharp one, 14.26 and 22.41 in the winner regime --
# 1.5 x 14.26 = 21.4, so the cap decides, and the 22.41 is a finding (_DV_WINNER below), not a reason to raise it.
F_ATT = 20
ATT_RATIOS = {}


def att_case(B, H, Lq, Lk, regime):
    """q [B*Lq][D], kv [B*Lk][2D] (fused k | v addressing; v filled per V scale by att_values) of the named regime, with the
    regime's label asserted on the float64 scores as tests/test_hip_denoiser_range.py does.  A lead of x in the score is built on
    head dimension 0: q[.., 0] = 4 in every head and 2 x added to that dimension of the leading key (score = q . k / 8)."""
    D = H * 64
    q, k = rnd((B * Lq, D), "tr.at.q"), rnd((B * Lk, D), "tr.at.k")
    d0 = torch.arange(H) * 64
    lead_key = {"sharp": Lk // 2, "winner": Lk // 3}.get(regime)
    if regime == "flat":
        k *= 2.0 ** -9
    elif regime in ("sharp", "winner"):
        q[:, d0] = 4.0
        k.view(B, Lk, D)[:, lead_key, d0] += 2.0 * (60.0 if regime == "sharp" else 125.0)
    elif regime == "cross":
        cond = synth.synth_cond_emb(B, seq=Lk, dim=512, key="tr.at.cond").double().reshape(B * Lk, 512)
        k = (cond @ rnd((D, 512), "tr.at.wk", 0.035).double().t()).float()
    else:
        assert regime == "unit"
    heads = lambda t, Lx: t.reshape(B, Lx, H, 64).permute(0, 2, 1, 3).double()
    s = 0.125 * heads(q, Lq) @ heads(k, Lk).transpose(-1, -2)
    p = torch.softmax(s, -1)
    top2 = s.topk(2, dim=-1).values
    if regime == "flat":
        assert float(s.abs().max()) <= 2.0 ** -6 and float((-(p * p.log()).sum(-1) - math.log(Lk)).abs().max()) < 1e-3
    elif regime == "sharp":
        assert bool((s.argmax(-1) == lead_key).all()) and 50.0 < float((top2[..., 0] - top2[..., 1]).min())
        assert float((top2[..., 0] - top2[..., 1]).max()) < 75.0
    elif regime == "winner":
        assert bool((s.argmax(-1) == lead_key).all()) and float((top2[..., 0] - top2[..., 1]).min()) > 110.0
    elif regime == "cross":
        assert float(k.abs().max()) < IN_RANGE and 0.01 < float(k.abs().median()) < 0.1
    return q, k


def att_values(B, H, Lk, regime, vname):
    D = H * 64
    if regime == "cross":             # V from the same kind of map as K: below 2^-3 at its natural scale
        cond = synth.synth_cond_emb(B, seq=Lk, dim=512, key="tr.at.cond").double().reshape(B * Lk, 512)
        v = (cond @ rnd((D, 512), "tr.at.wv", 0.035).double().t()).float()
        if vname == "1":
            assert float(v.abs().max()) < IN_RANGE
        return v * SCALE[vname]
    return rnd((B * Lk, D), "tr.at.v", SCALE[vname])


def att_do(B, H, Lq, place):
    """dO [B*Lq][D] with max |dO| = 2^-10 exactly (one ulp under it for the ceiling case) -> max |dO do_scale| = 2^0, 2^6, or one ulp
    under 2^15"""
    dO = rnd((B * Lq, H * 64), "tr.at.do", 0.99 * DO_RAW)
    dO[0, 0] = DO_RAW if place != "under 2^15" else float(torch.nextafter(torch.tensor(DO_RAW), torch.tensor(0.0)))
    m = float(dO.abs().max()) * DO_SCALE[place]
    assert m == {"2^0": 1.0, "2^6": 64.0}.get(place, m) and (place != "under 2^15" or 2.0 ** 15 * (1 - 2.0 ** -23) < m < 2.0 ** 15)
    return dO


def att_autograd(q, k, v, dO, B, H, Lq, Lk, dtype):
    """autograd of softmax(q k^T / 8) v in `dtype` -> {dq, dk, dv} as [B*L][D] float64, plus (P, dS, dP, delta) of that evaluation"""
    heads = lambda t, Lx: t.reshape(B, Lx, H, 64).permute(0, 2, 1, 3).to(dtype)
    unheads = lambda t, Lx: t.permute(0, 2, 1, 3).reshape(B * Lx, H * 64).double()
    Q, K, V = (heads(t, Lx).clone().requires_grad_(True) for t, Lx in ((q, Lq), (k, Lk), (v, Lk)))
    dOh = heads(dO, Lq)
    with torch.enable_grad():
        P = torch.softmax(0.125 * (Q @ K.transpose(-1, -2)), dim=-1)
        out = P @ V
        out.backward(dOh)
    P, out = P.detach(), out.detach()
    dP = dOh @ V.detach().transpose(-1, -2)
    delta = (dOh * out).sum(-1, keepdim=True)
    return dict(dq=unheads(Q.grad, Lq), dk=unheads(K.grad, Lk), dv=unheads(V.grad, Lk)), (P, dP, delta)


def att_lo_terms(q, k, v, dO, B, H, Lq, Lk, P, dP, delta):
    """The lo-terms [B*L][D] per gradient, from the float64 evaluation.  Q, K and V are split UNSCALED (csrc/attention_bwd.hip:
    ab_stage_split / ab_load_frag; only dO carries do_scale, P carries 2^10 and dS is normalised per wave), so every entry of them
    with 0 < |.| < 2^-3 is off by up to 2^-25 absolutely.  With dS = P (dP - delta) / 8:
      K's lo plane into dQ = dS K:     |d dQ[q,d]| <= 2^-25 sum_{j: |K[j,d]| < 2^-3} |dS[q,j]|
      Q's lo plane into dK = dS^T Q:   |d dK[j,d]| <= 2^-25 sum_{q: |Q[q,d]| < 2^-3} |dS[q,j]|
      V's lo plane into dP = dO V^T:   |d dP[q,j]| <= 2^-25 sum_{d: |V[j,d]| < 2^-3} |dO[q,d]| =: EP[q,j], hence |d dS| <= P EP / 8
        (delta comes from dO . O in fp32, not from the split V), and from there into dQ: (P EP / 8) |K|, into dK: (P EP / 8)^T |Q|.
    dV = P^T dO has no lo-term: P is split as P 2^10 (2^-35 absolute) and dO under its own power of two.  The same model for the
    scores (Q, K lo planes into S, through the softmax) is not needed: no case comes near F without it."""
    heads = lambda t, Lx: t.reshape(B, Lx, H, 64).permute(0, 2, 1, 3).double()
    unheads = lambda t, Lx: t.permute(0, 2, 1, 3).reshape(B * Lx, H * 64)
    Q, K, V, dOh = heads(q, Lq), heads(k, Lk), heads(v, Lk), heads(dO, Lq)
    dS = (0.125 * P * (dP - delta)).abs()
    dS_v = 0.125 * P * (LO_ABS * (dOh.abs() @ below(V).transpose(-1, -2)))
    lo_dq = LO_ABS * (dS @ below(K)) + dS_v @ K.abs()
    lo_dk = LO_ABS * (dS.transpose(-1, -2) @ below(Q)) + dS_v.transpose(-1, -2) @ Q.abs()
    # the gradients' magnitude before any cancellation (module comment at F_ATT): every product over absolute values
    raw = 0.125 * P * (dOh.abs() @ V.abs().transpose(-1, -2) + (dOh.abs() * (P @ V.abs())).sum(-1, keepdim=True))
    mag = dict(dq=float((raw @ K.abs()).max()), dk=float((raw.transpose(-1, -2) @ Q.abs()).max()), dv=0.0)
    return dict(dq=unheads(lo_dq, Lq), dk=unheads(lo_dk, Lk), dv=torch.zeros(B * Lk, H * 64, dtype=torch.float64)), mag


def emu_attention_bwd(q, k, v, dO, do_scale, B, H, Lq, Lk):
    """float64 emulation of ds_attention_bwd_f16x2: every tile product as hi hi + hi lo + lo hi of the operands' splits (Q, K, V
    unscaled; dO do_scale; P 2^10; dS normalised to [2^8, 2^9) by a power of two -- per head here, per wave in the kernel), exact
    float64 in between -> {dq, dk, dv} [B*L][D]"""
    heads = lambda t, Lx: t.reshape(B, Lx, H, 64).permute(0, 2, 1, 3)
    unheads = lambda t, Lx: t.permute(0, 2, 1, 3).reshape(B * Lx, H * 64)
    out = {n: torch.zeros(B, H, Lx, 64, dtype=torch.float64) for n, Lx in (("dq", Lq), ("dk", Lk), ("dv", Lk))}
    Qa, Ka, Va, dOa = heads(q, Lq), heads(k, Lk), heads(v, Lk), heads(dO * do_scale, Lq)
    for b in range(B):
        for h in range(H):
            Q, K, V, dOs = Qa[b, h].contiguous(), Ka[b, h].contiguous(), Va[b, h].contiguous(), dOa[b, h].contiguous()
            P = torch.softmax(0.125 * emu_product(Q, K), -1)
            O_ = P @ V.double()
            delta = (dOs.double() * O_).sum(-1, keepdim=True)
            Ps = (P * 1024.0).float()
            out["dv"][b, h] = emu_product(Ps.t().contiguous(), dOs.t().contiguous()) / 1024.0 / do_scale
            dS = 0.125 * P * (emu_product(dOs, V) - delta)
            m = float(dS.abs().max())
            up = 2.0 ** (8 - math.floor(math.log2(m))) if m > 0 else 1.0
            dSn = (dS * up).float()
            out["dq"][b, h] = emu_product(dSn, K.t().contiguous()) / up / do_scale
            out["dk"][b, h] = emu_product(dSn.t().contiguous(), Q.t().contiguous()) / up / do_scale
    return {"dq": unheads(out["dq"], Lq), "dk": unheads(out["dk"], Lk), "dv": unheads(out["dv"], Lk)}


def att_cases(B, H, Lq, Lk, regime):
    """every (V scale, dO place) of one shape and regime: inputs, float64 and fp32 autograd, lo-terms"""
    ck = ("att", B, H, Lq, Lk, regime)
    if ck not in _LIN:
        q, k = att_case(B, H, Lq, Lk, regime)
        out = []
        for vname in VSCALES:
            v = att_values(B, H, Lk, regime, vname)
            for place in DO_PLACES:
                dO = att_do(B, H, Lq, place)
                want, (P, dP, delta) = att_autograd(q, k, v, dO, B, H, Lq, Lk, torch.float64)
                got32, _ = att_autograd(q, k, v, dO, B, H, Lq, Lk, torch.float32)
                lo, mag = att_lo_terms(q, k, v, dO, B, H, Lq, Lk, P, dP, delta)
                top = {n: float(want[n].abs().max()) for n in want}
                floor = {n: EPS32 * max(top[n], mag[n] if regime in ("sharp", "winner") else 0.0) for n in want}
                d32 = {n: max(float((got32[n] - want[n]).abs().max()), floor[n]) for n in want}       # absolute
                out.append(dict(vname=vname, place=place, q=q, k=k, v=v, dO=dO, want=want, lo=lo, top=top, d32=d32))
        _LIN[ck] = out
    return _LIN[ck]


def att_judge(name, got, c, F, margin=1.0):
    """-> {gradient: (max-abs err, kernel / d32 raw, net of the lo-term)}; asserts net <= F when F is given"""
    fig = {}
    for n, want in c["want"].items():
        g = got[n].double()
        assert torch.isfinite(g).all(), (name, n)
        err = margin * (g - want).abs()
        raw = float(err.max()) / c["d32"][n]
        net = float((err - c["lo"][n]).clamp(min=0).max()) / c["d32"][n]
        fig[n] = (float(err.max()), raw, net)
        if F is not None:
            assert net <= F, "%s %s: %.2f x the fp32 yardstick (%.2e of max |want|; raw %.2f)" % (name, n, net, c["d32"][n] / c["top"][n], raw)
    return fig


def check_attention_bounds_on_emulation():
    """(b)'s bound on the float64 emulation with its error doubled: F_ATT x d32 + the lo-term must hold for every case; returns
    the worst net ratio (the emulation has no fp32 accumulation error: what remains beyond the lo-term is the splits' own 2^-22)"""
    worst = 0.0
    for B, H, Lq, Lk in ATT_SHAPES:
        for regime in REGIMES:
            for c in att_cases(B, H, Lq, Lk, regime):
                got = emu_attention_bwd(c["q"], c["k"], c["v"], c["dO"], DO_SCALE[c["place"]], B, H, Lq, Lk)
                fig = att_judge("emulated bwd (%d, %d) %s V %s dO %s" % (Lq, Lk, regime, c["vname"], c["place"]), got, c, F_ATT, margin=2.0)
                worst = max(worst, max(f[2] for f in fig.values()))
        print("emulation, attention backward (%d, %d): worst 2 x net ratio so far %.2f (F = %d)" % (Lq, Lk, worst, F_ATT), flush=True)
    return worst


@pytest.fixture(scope="module", autouse=True)
def _att_ratio_table():
    """after the module's tests: the worst measured kernel / d32 ratio per regime and gradient (the table of DESIGN.md section 7)"""
    yield
    for kern in ("f16x2_mon raw", "f16x2_mon net", "exact fp32"):
        row = ["%s %s" % (r, "/".join("%.2f" % ATT_RATIOS.get((kern, r, n), 0.0) for n in ("dq", "dk", "dv"))) for r in REGIMES
               if (kern, r, "dq") in ATT_RATIOS]
        if row:
            parity_line("attention backward vs float64, kernel / d32 (dq/dk/dv) %-13s: %s | worst %.2f"
                        % (kern, " ".join(row), max(v for (k_, _, _), v in ATT_RATIOS.items() if k_ == kern)))


# FINDING (kernel arithmetic, not repaired here): dV of the winner regime at (40, 33) is 3.66e-06 of its
# largest element = 22.41 x torch fp32's 1.63e-07, above the cap of 20 (14.26 x at (72, 77); 9.36 x in the sharp regime).  The
# backward recomputes P = exp(s - lse) with s from the kv kernel's product and lse from the dq kernel's: two summation orders of
# a score of ~130, whose fp32 ulp is 7.6e-06 -- the leading probability comes out 1 +- a few 1e-6 instead of 1, and dV = P^T dO
# carries it.  ds_attention_bwd (exact fp32) is at 1.79e-07 on the same case.  strict: it cannot start passing unnoticed.
_DV_WINNER = pytest.mark.xfail(strict=True, reason="dV, winner regime (40, 33): 22.41 x the torch-fp32 distance (3.66e-06 of max |dV|), "
                               "cap 20: P recomputed from two summation orders of a ~130 score")
ATT_PARAMS = [pytest.param(*sh, r, g, marks=[_DV_WINNER] if (sh[2:], r, g) == ((40, 33), "winner", "dv") else [],
                           id="%dx%d-%s-%s" % (sh[2], sh[3], r, g)) for sh in ATT_SHAPES for r in REGIMES for g in ("dq.dk", "dv")]


@pytest.mark.parametrize("B,H,Lq,Lk,regime,grads", ATT_PARAMS)
def test_attention_backward_across_regimes(L, B, H, Lq, Lk, regime, grads):
    """ds_attention_bwd_f16x2_mon (fused k | v addressing, gradients written in place into fused buffers) against float64 autograd
    in one softmax regime, crossed with V at 2^-12, 1, 6e4 and dO do_scale at the monitor window's floor, at the calibration
    target and one ulp under its ceiling: every gradient within F_ATT x d32 + its lo-term (att_lo_terms), the monitor's scalar =
    max |dO do_scale| through the fp16 hi plane; and ds_attention_bwd, the exact-fp32 kernel on the same cases (dO unscaled),
    within max(2e-5 max |want|, 3 x d32) with no lo-term.  The forward both differentiate is ds_attention on the same operands.
    grads: the gradients this case judges (dQ and dK, or dV: the same launches, so that a finding on one does not hide the others)."""
    D = H * 64
    failures = []
    for c in att_cases(B, H, Lq, Lk, regime):
        qc, kvc, dOc = c["q"].cuda(), torch.cat((c["k"], c["v"]), 1).contiguous().cuda(), c["dO"].cuda()
        o = torch.empty(B * Lq, D, device="cuda")
        L.check(L.lib().ds_attention(L.ptr(qc), D, L.ptr(kvc), 2 * D, L.ptr_off(kvc, D), 2 * D, L.ptr(o), D, B, H, Lq, Lk, 0.125, L.stream()))
        stats = torch.empty(2 * B * H * ((Lq + 31) // 32 * 32), device="cuda")
        got = {}
        for kern in ("f16x2_mon", "exact fp32"):
            dq, dkv = torch.full_like(qc, float("nan")), torch.full_like(kvc, float("nan"))
            args = (L.ptr(qc), D, L.ptr(kvc), 2 * D, L.ptr_off(kvc, D), 2 * D, L.ptr(o), D, L.ptr(dOc), D, L.ptr(dq), D, L.ptr(dkv), 2 * D,
                    L.ptr_off(dkv, D), 2 * D, L.ptr(stats), B, H, Lq, Lk, 0.125)
            if kern == "f16x2_mon":
                amax = torch.zeros(1, device="cuda")
                L.check(L.lib().ds_attention_bwd_f16x2_mon(*args, DO_SCALE[c["place"]], L.ptr(amax), L.stream()))
                want_m = float(c["dO"].abs().max()) * DO_SCALE[c["place"]]
                assert abs(float(amax.item()) - want_m) <= 1e-3 * want_m
            else:
                L.check(L.lib().ds_attention_bwd(*args, L.stream()))
            got[kern] = dict(dq=dq.cpu(), dk=dkv.cpu()[:, :D], dv=dkv.cpu()[:, D:])
        name = "(%d, %d) %s V %s dO %s" % (Lq, Lk, regime, c["vname"], c["place"])
        fig = att_judge(name, got["f16x2_mon"], c, None)
        fig32 = att_judge(name, got["exact fp32"], c, None)
        for n in grads.split("."):
            for kern, val in (("f16x2_mon raw", fig[n][1]), ("f16x2_mon net", fig[n][2]), ("exact fp32", fig32[n][1])):
                ATT_RATIOS[(kern, regime, n)] = max(ATT_RATIOS.get((kern, regime, n), 0.0), val)
            t_ = c["top"][n]
            print("attention bwd %s %s: f16x2 rel %.2e = %.2f x d32 raw, %.2f net of the lo-term (lo-term up to %.2e); exact fp32 rel "
                  "%.2e; d32 %.2e (of max |want| = %.2e)" % (name, n, fig[n][0] / t_, fig[n][1], fig[n][2], float(c["lo"][n].max()) / t_,
                                                            fig32[n][0] / t_, c["d32"][n] / t_, t_))
            if fig[n][2] > F_ATT:
                failures.append("f16x2_mon %s %s: %.2f x d32 net of the lo-term" % (name, n, fig[n][2]))
            if fig32[n][0] > max(2e-5 * t_, 3 * c["d32"][n]):
                failures.append("ds_attention_bwd %s %s: %.2e vs d32 %.2e (of max |want|)" % (name, n, fig32[n][0] / t_, c["d32"][n] / t_))
    assert not failures, failures


# ======================================= (c) a whole step with a hot forward operand =======================================
HOT_ROW = "transformer.transformer.blocks.1.mlp.0"
_STEP_REF = {}


def hot_step_case(factor):
    """The 2-layer synthetic model at B = 2 with mlp.0 weight and bias of the last block times `factor` (FC2's operand gelu2(u)
    grows by about that factor), its batch, and the float64 oracle's loss and gradients -- computed once per factor and shared.
    The oracle gets the noised tokens the fp32 q_sample draws (a float64 Gumbel argmax can resolve a near-tie differently)."""
    if factor not in _STEP_REF:
        sd = dict(synth_sd("dalle", 2))
        for sfx in (".weight", ".bias"):
            sd[HOT_ROW + sfx] = sd[HOT_ROW + sfx] * factor
        x0 = synth.synth_tokens(2, mask_frac=0.0, key="tr.hot.x0")
        cond = synth.synth_cond_emb(2, key="tr.hot.c")
        t, pt = torch.tensor([57, 93]), torch.ones(2) / 100
        u = synth.synth_uniform((2, 257, 265), key="tr.hot.u")
        K = sd["transformer.transformer.to_logits.1.weight"].shape[0]
        xt = O.q_sample(O.make_schedule(100, K + 1), x0, t, u, K + 1).argmax(1)
        sd64 = {k: (v.double().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
        seen, rec_plain = {}, O._rec

        def rec_keep(record, name, a):
            if name == HOT_ROW[:-1] + "2":             # FC2's operand of the hot block
                seen["g"] = a.detach()
            return rec_plain(record, name, a)
        O._rec = rec_keep
        try:
            with torch.enable_grad():
                _, _, loss, _ = O.train_loss(sd64, x0, cond.double(), t, pt.double(), u, xt=xt)
                loss.backward()
        finally:
            O._rec = rec_plain
        grads = {k[len("transformer."):]: v.grad for k, v in sd64.items()
                 if k.startswith("transformer.transformer.") and v.is_floating_point() and v.grad is not None}
        _STEP_REF[factor] = dict(sd=sd, batch=(x0, cond, t, pt, u), loss=float(loss.detach()), grads=grads, g=seen["g"])
    return _STEP_REF[factor]


@pytest.mark.parametrize("factor,lo,hi,n_over", [(2.76e4, 65504.0, 7.0e4, (5, 40)), (1.2e5, 2.9e5, 3.1e5, (400000, 460000)), (1.2e4, 2.0 ** 12, 3.2e4, (0, 0))])
def test_training_step_with_a_hot_forward_operand(factor, lo, hi, n_over):
    """TrainStep("f16x2").loss_and_grads with mlp.0 weight and bias of the last block scaled so that FC2's operand gelu2(u) is
    (1) past fp16's range at a handful of positions -- asserted on the host in float64: max 6.93e4, 24 of the 2 x 265 x 4096
    positions above 65504; (2) far past it: max 3.0e5, 20 % of the positions above 65504; (3) at 3e4, inside the range but above
    2^12 -- against the float64 oracle under the tolerances of test_training_step_gradients_vs_oracle_autograd (loss 2e-4, every
    gradient tensor 2e-3 of its largest element).  Every forward operand used to be packed with scale 1 and no monitor: the split
    saturated at 65504 without a trace.  Measured on the parent commit: (2) loss off by 2.81e-4, worst gradient tensor 4.4e-1
    (mlp.2.weight) -- it fails; (1) does NOT move the parent's figures (loss 3.2e-6, worst tensor 8.1e-4, the same as after the
    fix: 24 entries clipped by at most 6 % are far inside the tolerance), so on the parent it fails only where it asks for the
    policy's exponents and monitor.  Now the first calibration pass measures max |operand| per linear and the
    policy packs the hot one under 2^f = 2^(12 - floor(log2 max)) (f = -4 / -6 / -2 here, asserted); 2^-f goes into the forward
    epilogue and the dW epilogue, exact, and the forward monitor reads the scaled maximum in [2^12, 2^13)."""
    from text_to_sound_synthesis_amd.config import build_model, default_config
    from text_to_sound_synthesis_amd.modeling.train import TrainStep
    c = hot_step_case(factor)
    g64 = c["g"]
    top, over = float(g64.abs().max()), int((g64.abs() > 65504.0).sum())
    assert lo < top < hi, top
    assert n_over[0] <= over <= n_over[1], over
    m = build_model(default_config(n_layer=2, diffusion_step=100))
    m.load_state_dict({**c["sd"], **synth_sd("encoder")}, strict=False)
    m = m.cuda().eval()
    dt = m.transformer
    dt.auxiliary_loss_weight, dt.adaptive_auxiliary_loss, dt.mask_weight = 5.0e-4, True, [1, 1]
    step = TrainStep(dt, precision="f16x2")
    loss, grads = step.loss_and_grads(*(b.cuda() for b in c["batch"]))
    fexp = getattr(step.policy, "fwd_exp", None)
    seen_fwd = float(getattr(step.policy, "_fwd_live", None) or 0.0)       # max |operand 2^f| the forward packs folded in
    worst, missing = [], []
    for name, want in c["grads"].items():
        if name not in grads:
            if want.abs().max() > 0:
                missing.append(name)
            continue
        got = grads[name].cpu().double()
        if want.abs().max().item() < 1e-7:         # (the key biases: analytically zero, see the test this one follows)
            assert got.abs().max().item() < 1e-6, name
            continue
        worst.append(((got - want).abs().max().item() / want.abs().max().item(), name))
    worst.sort(reverse=True)
    rel_loss = abs(loss.item() - c["loss"]) / c["loss"]
    line = "training step, FC2 operand up to %.3g (%d positions > 65504), forward exponents %s: loss rel err %.2e, worst gradient " \
        "tensor %.2e (%s) vs float64 oracle" % (top, over, {k: v for k, v in (fexp or {}).items() if v}, rel_loss, worst[0][0],
                                                worst[0][1])
    print(line)
    parity_line(line)
    for err, name in worst[:8]:
        print("  grad rel err %.2e  %s" % (err, name))
    assert not missing, missing
    assert rel_loss < 2e-4, (loss.item(), c["loss"])
    assert len(worst) >= 50 and worst[0][0] < 2e-3, worst[:5]
    assert {k: v for k, v in fexp.items() if v} == {"b1.fc2": 12 - math.floor(math.log2(top))}
    # the forward monitor saw the scaled operand, three bits under its limit: nothing trips
    assert 2.0 ** 12 <= seen_fwd < 2.0 ** 13, seen_fwd
    assert not step.check_loss_scale(force=True), step.last_trip


# ================================= the bounds against the float64 emulation (no GPU) =================================
def _doubled(y, ref, margin=2.0):
    """the emulation's result with its error doubled: a bound that holds for it holds for the emulation with a margin of 2"""
    return ref + margin * (y - ref)


def check_bounds_on_emulation(shapes=None, attention=True):
    """Every bound of (a) and (b) on the float64 emulation of the kernels (torch_split of both operands, hi hi + hi lo + lo hi in
    float64, the epilogue scales), with the emulation's error DOUBLED before it is judged: a bound the emulation cannot meet with
    that margin is a wrong bound, not a kernel bug.  The RMS forms get a margin of 1.5 instead (rms_scale = 0.75 on the doubled
    error): RMS_LO = 2^-25 bounds roundings that are uniform in +-2^-25, whose RMS is 2^-25 / sqrt(3) -- the emulation measures
    0.58 .. 0.60 x 2^-25 -- so a margin of 2 cannot exist for them; 1.5 is what sqrt(3) leaves.  dX with the wide weight is held to
    the bound itself (margin 1): there ONE term |W[3,k]| ~ 100 is 95 % of sum_n |W[n,k]|, the allowance is the worst case of that
    one rounding, and a worst case is attained (measured 0.55 .. 0.95 of it on the rows 2^-14 under their site's maximum).  The fp32 kernel's place is taken by a plain fp32 torch product on the CPU.
    Run it with  python tests/test_hip_train_range.py ; prints the worst figures."""
    worst = {"fwd": 0.0, "dx": 0.0, "dw": 0.0}
    for shape in shapes or LIN_SHAPES:
        M, N, K, parts = LIN_SHAPES[shape]
        ws = {k: make_w(N, K, k, parts) for k in WKINDS}
        for sname, pro in XFORMS:
            x = make_x(M, K, sname, pro)
            for wkind, w in ws.items():
                c = fwd_ref(x, w, "cpu")
                f = judge("emulated fwd %s X %s/%s W %s" % (shape, sname, pro, wkind), _doubled(emu_fwd(x, w), c["ref"]),
                          emu_x(x) @ w["W"].t() + w["b"], c, wkind, rms_scale=0.75)
                worst["fwd"] = max(worst["fwd"], f[2] or 0.0)
        for dname in DYSETS:
            d = make_dy(M, N, dname)
            for wkind, w in ws.items():
                if parts == 1:
                    c = dx_ref(d, w, "cpu")
                    f = judge_bwd("emulated dx %s dY %s W %s" % (shape, dname, wkind), _doubled(emu_dx(d, w), c["ref"], 1.0 if wkind == "wide" else 2.0),
                                  d["dy"] @ w["W"],
                                  c, row_blocks(d["rc"], K), rms_scale=0.75)
                    worst["dx"] = max(worst["dx"], f[2])
            for sname, pro in XFORMS:
                x = make_x(M, K, sname, pro)
                c = dw_ref(d, x, "cpu")
                f = judge_bwd("emulated dw %s dY %s X %s/%s" % (shape, dname, sname, pro), _doubled(emu_dw(d, x), c["ref"]),
                              INV * (d["dy"].t() @ emu_x(x)), c, dw_blocks(x, N, K), rms_scale=0.75)
                worst["dw"] = max(worst["dw"], f[2])
        print("emulation, %s: worst 2 x |err| / bound so far %s" % (shape, {k: "%.3f" % v for k, v in worst.items()}), flush=True)
    if attention:
        worst["attention_bwd"] = check_attention_bounds_on_emulation()
    return worst


if __name__ == "__main__":
    with torch.no_grad():
        print(check_bounds_on_emulation())
