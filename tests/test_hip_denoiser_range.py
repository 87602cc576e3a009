"""The denoiser's split-fp16 GEMM (ds_gemm_f16x2) and every inference form of its attention across the operand range, against
float64, at the C-ABI entries.

The f16x2 kernels use an fp32 operand a as fp16(a) + fp16(a - fp16(a)) without scaling it (csrc/common.h ds_split_hi / ds_split_lo;
only the weights carry a power of two): fp32-class for |a| in about [2^-3, 65504]; below 2^-3 the lo plane is subnormal and a keeps
2^-25 of absolute precision, so a dot product carries up to 2^-25 * sum |w| of extra absolute error; above 65504 the split saturates.
(a) the dense GEMM on every A path of the denoiser (fp32 A split by the loader, packed planes made on the host and by
ds_pack_operand, the per-sample and half-tile programs), auto and forced tiles, at whole-operand scales 2^-12 .. 6e4, with one hot
feature column at 6e4 and with rows of two scales, and its epilogues (GELU2, split store, in-place residual, attention-ready store);
(b) ds_attention, ds_attention_f16x2 / _split / _ready and causal ds_attention_ex in named softmax regimes (flat, unit, sharp,
winner-takes-all, the running maximum moving late / never, twin maxima in two chunks, a diffuse mass under a peak, the
cross-attention operating point) crossed with V at 2^-12, 1, 6e4 and one hot column.  The bounds come from the documented error
model and, for the attention, from the distance of a plain fp32 torch evaluation to float64 on the same case.
The constants SCALES, LO_ABS, C_LO, RMS_LO and the assertion forms of (a) are those of tests/test_hip_codec_vocoder_range.py (the
codec's and the vocoder's file for the same question); the oracle's record of which edges the real operands reach is the non-GPU
tests/test_denoiser_operand_record.py.  GPU only (-m gpu)."""
import math
import warnings

import pytest
import torch

import diffsound_oracle as O
from conftest import parity_line, synth_sd
from text_to_sound_synthesis_amd import synth

pytestmark = pytest.mark.gpu
NO_GRAD = True

# ---- copied from tests/test_hip_codec_vocoder_range.py (see there for how RMS_LO follows from independent rounding errors) ----
EPS32 = 2.0 ** -24
LO_ABS = 2.0 ** -25          # absolute precision of a subnormal fp16 lo plane (half its spacing, 2^-24)
C_LO = 1.0                   # the documented bound:  |err| <= C_LO * 2^-25 * sum |w|  per split (+ the fp32-class term)
RMS_LO = 2.0 ** -25
SCALES = ["2^-12", "2^-6", "1", "2^14", "6e4", "hot6e4"]
SCALE = {"2^-12": 2.0 ** -12, "2^-6": 2.0 ** -6, "1": 1.0, "2^14": 2.0 ** 14, "6e4": 6e4, "hot6e4": 1.0}
HOT = 5
# ---- this file's own ----
SETS = SCALES + ["mixed"]    # "mixed": even rows at 2^-12, odd rows at 1 (one launch, both sides of 2^-3)
IN_RANGE = 2.0 ** -3         # at and above it no lo-plane allowance at all
GELU2_LIP = 1.1              # max |d/dx x sigmoid(1.702 x)| = 1.0998: an operand-side error passes the activation at most x 1.1
PS, HALF = 9, 10             # ds_gemm_f16x2_force_tile: the per-sample and the half-tile program (tests/test_hip_widening.py)


@pytest.fixture(scope="module")
def L():
    from text_to_sound_synthesis_amd import _lib
    _lib.lib()
    return _lib


def rnd(shape, key, scale=1.0):
    return (synth.synth_uniform(shape, key=key) * 2 - 1) * scale


def torch_split(a):
    """ds_split_hi / ds_split_lo (csrc/common.h) in torch: hi = fp16(clamp(a)), lo = fp16(clamp(a - hi))"""
    hi = a.clamp(-65504.0, 65504.0).half()
    lo = (a - hi.float()).clamp(-65504.0, 65504.0).half()
    return torch.stack((hi, lo)).contiguous()


def gelu2(y):
    return y * torch.sigmoid(1.702 * y)


# =================================================== (a) the dense GEMM ===================================================
def row_scales(M, sname):
    """per-row operand scale [M]"""
    if sname == "mixed":
        s = torch.ones(M, dtype=torch.float64)
        s[0::2] = 2.0 ** -12
        return s
    return torch.full((M,), SCALE[sname], dtype=torch.float64)


_CASES = {}


def gemm_case(M, N, K, sname, wkind, act=False):
    """Seeded inputs and the float64 result, computed once per (shape, operand set, weight kind) and shared (never modified).
    wkind "flat": W from rnd(.., 0.1); "wide": the same with row 3 x 2^10, so that every other weight sits 2^10 down in the
    scaled fp16 range of split_f16x2.  Bias and residual at the operand's scale (mixed rows: the bias at the smaller one)."""
    ck = (M, N, K, sname, wkind, act)
    if ck not in _CASES:
        rs = row_scales(M, sname)
        A = rnd((M, K), "dr.A") * rs.float()[:, None]
        if sname == "hot6e4":
            A[:, HOT] *= 6e4
        W = rnd((N, K), "dr.W", 0.1)
        if wkind == "wide":
            W[3] *= 2.0 ** 10
        b = rnd((N,), "dr.b", float(rs.min()))
        R = None if act else rnd((M, N), "dr.R") * rs.float()[:, None]
        ref = A.double() @ W.double().t() + b.double()
        ref = gelu2(ref) if act else ref + R.double()
        _CASES[ck] = dict(A=A, W=W, b=b, R=R, ref=ref, rs=rs, l1=W.double().abs().sum(1), l2=W.double().norm(dim=1))
    return _CASES[ck]


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


def judge(name, y, y32, c, wkind, lip=1.0, extra=None):
    """The assertion forms of test_split_kernel_across_operand_range (tests/test_hip_codec_vocoder_range.py), per block.
    Operand scale >= 2^-3: relative max error vs float64 within max(3e-6, 1.2 x the exact-fp32 ds_gemm's), no lo-plane allowance.
    Below: per output within C_LO 2^-25 sum_k |w| (x lip through an activation) + the fp32-class term max(3e-6 max|ref|, 1.2 x the
    fp32 kernel's max error), and RMS over outputs of err / ||w||_2 within RMS_LO (x lip) + 1.2 x the fp32 kernel's.
    extra (float64 [M][N], may hold inf): a further absolute allowance per output, taken off the error before it is judged.
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
            r, r32 = float((err / l2).pow(2).mean().sqrt()), float((err32 / l2).pow(2).mean().sqrt())
            fig[2], fig[3] = max(fig[2] or 0.0, worst), max(fig[3] or 0.0, r / RMS_LO)
            assert worst <= 1.0, "%s %s: %.3g of the documented bound" % (name, label, worst)
            assert r <= RMS_LO * lip + 1.2 * r32, "%s %s: RMS %.3g x 2^-25 (fp32 %.3g)" % (name, label, r / RMS_LO, r32 / RMS_LO)
    return fig


def report(title, figs):
    """one parity line per test: the worst figure over the paths / tiles it ran"""
    rel, rel32 = max(f[0] for f in figs.values()), max(f[1] for f in figs.values())
    line = "%s: %d launches, worst rel max err vs float64 %.2e (exact-fp32 ds_gemm %.2e)" % (title, len(figs), rel, rel32)
    lo = [f for f in figs.values() if f[2] is not None]
    if lo:
        line += "; below 2^-3: worst |err| / (2^-25 sum|w| + fp32 term) %.3f, RMS err / ||w||_2 %.3f x 2^-25" \
            % (max(f[2] for f in lo), max(f[3] for f in lo))
    print(line)
    parity_line(line)


def a_forms(L, Ac):
    """the packed split planes of A made on the host (pack_planes of the host split) and by ds_pack_operand: the same bits"""
    M, K = Ac.shape
    M16 = (M + 15) // 16 * 16
    host = L.pack_planes(torch_split(Ac))
    dev = torch.zeros(2, M16 * K, device="cuda", dtype=torch.float16)
    L.check(L.lib().ds_pack_operand(L.ptr(Ac), M, K, K, 1.0, 0, None, 0, L.ptr(dev), M16 * K, None, 0, 0, 0, 0, None, None,
                                    L.stream()))
    assert torch.equal(dev.view(-1), host.view(-1))
    return {"packed.host": host, "packed.pack_operand": dev}, M16 * K


def fp32_gemm(L, c, M, N, K, act=0):
    y32 = torch.empty(M, N, device="cuda")
    L.gemm(c["A"].cuda(), c["W"].cuda(), y32, M, N, K, bias=c["b"].cuda(), R=None if c["R"] is None else c["R"].cuda(), act=act)
    return y32


@pytest.mark.parametrize("wkind", ["flat", "wide"])
@pytest.mark.parametrize("sname", SETS)
@pytest.mark.parametrize("M,N,K", [(70, 96, 64), (265, 256, 1024), (33, 128, 4096)])
def test_gemm_f16x2_across_operand_range(L, M, N, K, sname, wkind):
    """ds_gemm_f16x2 with bias + residual on the 4-wave programs: fp32 A split by the loader (auto, 128x128, 128x64, 64x64 tiles)
    and packed planes from the host split and from ds_pack_operand (the same and the 96x128 tile).  (70, 96, 64): ragged in M, one
    k-tile pair; (265, 256, 1024): one sample's rows; (33, 128, 4096): FC2's contraction."""
    c = gemm_case(M, N, K, sname, wkind)
    Ac, Wc, bc, Rc = c["A"].cuda(), c["W"].cuda(), c["b"].cuda(), c["R"].cuda()
    y32 = fp32_gemm(L, c, M, N, K)
    W2, sc = L.split_f16x2(Wc)
    W2p, scp = L.split_f16x2(Wc, packed=True)
    assert sc == scp
    packed, a_plane = a_forms(L, Ac)
    figs = {}
    try:
        for tile in (-1, 0, 1, 2, 3):
            L.lib().ds_gemm_f16x2_force_tile(tile)
            runs = {} if tile == 3 else {"loader": lambda y: L.gemm(Ac, W2, y, M, N, K, bias=bc, R=Rc, split2=sc)}
            for k, A2p in packed.items():
                runs[k] = lambda y, A2p=A2p: L.gemm(A2p, W2p, y, M, N, K, bias=bc, R=Rc, split2=sc, a_plane=a_plane)
            for path, run in runs.items():
                y = torch.full((M, N), float("nan"), device="cuda")
                run(y)
                figs[(path, tile)] = judge("gemm %s tile %d (%d, %d, %d) @ %s W %s" % (path, tile, M, N, K, sname, wkind), y, y32, c,
                                           wkind)
    finally:
        L.lib().ds_gemm_f16x2_force_tile(-1)
    report("ds_gemm_f16x2 (%d, %d, %d) @ %s, W %s" % (M, N, K, sname, wkind), figs)


@pytest.mark.parametrize("wkind", ["flat", "wide"])
@pytest.mark.parametrize("sname", SETS)
@pytest.mark.parametrize("prog,B,Lp,N,K", [(PS, 17, 265, 256, 64), (PS, 4, 272, 512, 64), (HALF, 4, 272, 512, 64)])
def test_gemm_f16x2_per_sample_programs_across_operand_range(L, prog, B, Lp, N, K, sname, wkind):
    """The per-sample ping-pong program on 265- and 272-row samples and the half-tile program on 272-row samples (the smallest
    shapes tests/test_hip_widening.py runs them on), packed operands, bias + residual: the same bounds against float64."""
    M = B * Lp
    c = gemm_case(M, N, K, sname, wkind)
    Ac, Wc, bc, Rc = c["A"].cuda(), c["W"].cuda(), c["b"].cuda(), c["R"].cuda()
    y32 = fp32_gemm(L, c, M, N, K)
    W2p, sc = L.split_f16x2(Wc, packed=True)
    packed, a_plane = a_forms(L, Ac)
    figs = {}
    try:
        L.lib().ds_gemm_f16x2_force_tile(prog)
        for path, A2p in packed.items():
            y = torch.full((M, N), float("nan"), device="cuda")
            L.gemm(A2p, W2p, y, M, N, K, bias=bc, R=Rc, split2=sc, a_plane=a_plane, rows_per_sample=Lp)
            figs[path] = judge("gemm program %d %s B%d x %d @ %s W %s" % (prog, path, B, Lp, sname, wkind), y, y32, c, wkind)
    finally:
        L.lib().ds_gemm_f16x2_force_tile(-1)
    report("ds_gemm_f16x2 program %d, %d x %d rows, N %d K %d @ %s, W %s" % (prog, B, Lp, N, K, sname, wkind), figs)


@pytest.mark.parametrize("sname", SETS)
def test_gemm_f16x2_gelu2_and_split_store_across_operand_range(L, sname):
    """The FC1 site: bias + GELU2, compared after the activation (its outputs span both edges whatever the operand's scale: the
    negative branch decays to zero), written as fp32 and as packed split planes (c_plane > 0), on the auto program (loader-split and
    packed A) and on the per-sample program with 272-row samples.  The planes equal the split of the fp32-store output bit for bit,
    so hi + lo is within the split's own precision of it (2^-22 relative, 2^-25 absolute below 2^-3) wherever it is in range."""
    B, Lp, N, K = 4, 272, 512, 64
    M = B * Lp
    c = gemm_case(M, N, K, sname, "flat", act=True)
    Ac, Wc, bc = c["A"].cuda(), c["W"].cuda(), c["b"].cuda()
    y32 = fp32_gemm(L, c, M, N, K, act=L.ACT_GELU2)
    W2, sc = L.split_f16x2(Wc)
    W2p, _ = L.split_f16x2(Wc, packed=True)
    packed, a_plane = a_forms(L, Ac)
    A2p = packed["packed.pack_operand"]
    figs = {}
    try:
        for prog in (-1, PS):
            L.lib().ds_gemm_f16x2_force_tile(prog)
            kw = dict(rows_per_sample=Lp) if prog == PS else {}
            runs = {"packed": lambda y, **k: L.gemm(A2p, W2p, y, M, N, K, bias=bc, act=L.ACT_GELU2, split2=sc, a_plane=a_plane, **kw, **k)}
            if prog == -1:
                runs["loader"] = lambda y, **k: L.gemm(Ac, W2, y, M, N, K, bias=bc, act=L.ACT_GELU2, split2=sc, **k)
            for path, run in runs.items():
                name = "gemm GELU2 %s program %d @ %s" % (path, prog, sname)
                y = torch.full((M, N), float("nan"), device="cuda")
                run(y)
                figs[(path, prog)] = judge(name, y, y32, c, "flat", lip=GELU2_LIP)
                if path == "packed":
                    planes = torch.zeros(2, M * N, device="cuda", dtype=torch.float16)           # M = 4 x 272 is a multiple of 16
                    run(planes, c_plane=M * N)
                    got = L.unpack_planes(planes, M, N)
                    # (both launches are the same program: the planes are the split of THIS program's fp32 store, also in the
                    # 16-row block that the per-sample program sums in another order than the 4-wave programs)
                    assert torch.equal(got, torch_split(y)), name
                    # hi + lo against float64 under the same bounds + what the split itself keeps (2^-22 relative, 2^-25 absolute
                    # below 2^-3), wherever the result is representable (past 65504 the planes saturate: no claim there)
                    ref = c["ref"]
                    keeps = (2.0 ** -22 * ref.abs()).clamp(min=LO_ABS)
                    keeps[ref.abs() > 65000.0] = float("inf")
                    assert float((ref.abs() <= 65000.0).double().mean()) > 0.5
                    judge(name + " hi + lo", got[0].double() + got[1].double(), y32, c, "flat", lip=GELU2_LIP, extra=keeps)
    finally:
        L.lib().ds_gemm_f16x2_force_tile(-1)
    report("ds_gemm_f16x2 + GELU2 (fp32 and split store), %d x %d rows, N %d K %d @ %s" % (B, Lp, N, K, sname), figs)


@pytest.mark.parametrize("sname", SETS)
def test_gemm_f16x2_in_place_residual_across_operand_range(L, sname):
    """C aliases R (the denoiser's projections add into the residual stream in place): the bits of the launch with a separate R,
    and the same bounds against float64."""
    M, N, K = 265, 256, 1024
    c = gemm_case(M, N, K, sname, "flat")
    Ac, Wc, bc, Rc = c["A"].cuda(), c["W"].cuda(), c["b"].cuda(), c["R"].cuda()
    y32 = fp32_gemm(L, c, M, N, K)
    W2, sc = L.split_f16x2(Wc)
    W2p, _ = L.split_f16x2(Wc, packed=True)
    packed, a_plane = a_forms(L, Ac)
    A2p = packed["packed.pack_operand"]
    figs = {}
    for path, run in (("loader", lambda y, R: L.gemm(Ac, W2, y, M, N, K, bias=bc, R=R, split2=sc)),
                      ("packed", lambda y, R: L.gemm(A2p, W2p, y, M, N, K, bias=bc, R=R, split2=sc, a_plane=a_plane))):
        apart = torch.full((M, N), float("nan"), device="cuda")
        run(apart, Rc)
        y = Rc.clone()
        run(y, y)
        assert torch.equal(y, apart), path
        figs[path] = judge("gemm in-place residual %s @ %s" % (path, sname), y, y32, c, "flat")
    report("ds_gemm_f16x2 in-place residual (265, 256, 1024) @ %s" % sname, figs)


@pytest.mark.parametrize("sname", ["2^-12", "1", "6e4"])
def test_gemm_f16x2_attention_store_across_operand_range(L, sname):
    """STORE_ATTN (the arguments of test_gemm_attention_store_bit_identical, tests/test_hip_split_gemm.py): the Q planes and the
    K / V^T images written by the epilogue equal attn_images / the head-major split of the fp32-store result of the same GEMM, with
    the projection's outputs far below 2^-3 (subnormal lo planes, some hi planes too), O(1), and past 65504 (both planes saturate
    the same way); the fp32-store result itself is held to the bounds against float64."""
    B, Lq, H, D = 3, 265, 16, 1024
    M, N, K = B * Lq, 3 * D, D
    s = SCALE[sname]
    A, W, b = rnd((M, K), "dr.as.A", s), rnd((N, K), "dr.as.W", 0.05), rnd((N,), "dr.as.b", s)
    c = dict(A=A, W=W, b=b, R=None, ref=A.double() @ W.double().t() + b.double(), rs=row_scales(M, sname),
             l1=W.double().abs().sum(1), l2=W.double().norm(dim=1))
    Ac, Wc, bc = A.cuda(), W.cuda(), b.cuda()
    W2p, sc = L.split_f16x2(Wc, packed=True)
    packed, a_plane = a_forms(L, Ac)
    A2p = packed["packed.pack_operand"]
    y = torch.full((M, N), float("nan"), device="cuda")
    L.gemm(A2p, W2p, y, M, N, K, bias=bc, split2=sc, a_plane=a_plane)
    fig = judge("gemm for the attention store @ %s" % sname, y, fp32_gemm(L, c, M, N, K), c, "flat")
    heads = lambda x: torch_split(x.contiguous()).view(2, B, Lq, H, 64).permute(0, 1, 3, 2, 4).contiguous()
    q_ref = heads(y[:, :D])
    img_ref = L.attn_images(heads(y[:, D:2 * D]), heads(y[:, 2 * D:]), 288)
    if sname == "6e4":
        assert float(y.abs().max()) > 65504.0              # the saturating side is exercised
    qh = torch.full((2, B, H, Lq, 64), float("nan"), device="cuda", dtype=torch.float16)
    img = torch.zeros(B, H, 4, 288 * 64, device="cuda", dtype=torch.float16)
    L.gemm(A2p, W2p, qh, M, N, K, bias=bc, split2=sc, a_plane=a_plane, store=L.STORE_ATTN, rows_per_sample=Lq,
           attn=(img, H, 288, B * H * Lq * 64))
    assert torch.equal(qh, q_ref)
    assert torch.equal(img[:, :, :2], img_ref[:, :, :2])          # K image
    assert torch.equal(img[:, :, 2:], img_ref[:, :, 2:])          # V^T image
    report("ds_gemm_f16x2 STORE_ATTN (795, 3072, 1024) @ %s: Q planes, K / V^T images bit-identical" % sname, {"": fig})


# ================================================= (b) attention forward ==================================================
B_, H_, LQ = 2, 2, 40
D_ = H_ * 64
SM_SCALE = 0.125
LKS = [33, 77, 96, 97, 265]       # one chunk (33, 77, the full 96), the first key of a second chunk, 288 slots with 23 of padding
VSCALES = ["2^-12", "1", "6e4", "hot6e4"]
FORMS = ["ds_attention", "ds_attention_f16x2", "ds_attention_f16x2_split", "ds_attention_f16x2_ready", "ds_attention_ex.causal"]
# A kernel passes when its distance to float64 is within F x d32 + the lo-term: d32 = the distance of a plain fp32 torch
# evaluation of the same attention (O._mha in float32 on the CPU) to float64, max-abs relative to max |ref| and RMS; the lo-term
# (lo_term(), f16x2 forms only) is zero where no probability and no V entry is below 2^-3.  Departure from the issue, stated:
# d32 is floored at fp32's own rounding (yardstick()), because in the sharp regimes the fp32 evaluation is exact.
# F per form = twice the worst kernel / d32 ratio measured on an MI355X over every case below (net of the lo-term), rounded up;
# DESIGN.md section 3 has the tables, raw and net.  The condition of this file is F <= 8 (the training tests live within 3.1 of
# the same yardstick); with V >= 2^-3 even the RAW ratios (worst 3.83) would meet it.
F_FORM = {"ds_attention": 5, "ds_attention_f16x2": 3, "ds_attention_f16x2_split": 4, "ds_attention_f16x2_ready": 4,
          "ds_attention_ex.causal": 3}       # measured worst ratios: 2.20, 1.43, 1.55, 1.55, 1.45
assert max(F_FORM.values()) <= 8
# (form, regime) -> worst measured kernel / d32 ratio of this session: raw with V at 1, 6e4 and the hot column; raw with V below
# 2^-3 (2^-12, the cross-attention point); net of the lo-term over all of them
RAW, RAW_SMALL_V, RATIOS = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _ratio_table():
    """after the module's tests: the worst measured kernel / yardstick ratio per form and regime (the table of DESIGN.md section 3)"""
    yield
    regimes = list(dict.fromkeys(r for _, r in RATIOS))
    for title, tab in (("raw, V >= 2^-3", RAW), ("raw, V < 2^-3", RAW_SMALL_V), ("net of the lo-term", RATIOS)):
        for form in FORMS:
            row = [(r, tab[(form, r)]) for r in regimes if (form, r) in tab]
            if row:
                parity_line("attention vs float64, kernel / d32 %s: %-26s %s | worst %.2f, F = %d"
                            % (title, form, " ".join("%s %.2f" % x for x in row), max(x for _, x in row), F_FORM[form]))


def heads_of(x):
    """[B][L][H * 64] -> [B][H][L][64]"""
    return x.view(x.shape[0], x.shape[1], H_, 64).transpose(1, 2)


def attention64(q, k, v, causal=False, dtype=torch.float64):
    """softmax(q k^T / 8) v per head, written out: (out [B][Lq][H * 64], scores [B][H][Lq][Lk], probabilities)"""
    qh, kh, vh = heads_of(q.to(dtype)), heads_of(k.to(dtype)), heads_of(v.to(dtype))
    s = (qh @ kh.transpose(-2, -1)) * SM_SCALE
    if causal:
        s = s + torch.full(s.shape[-2:], float("-inf"), dtype=dtype).triu_(1)
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    p = p / p.sum(-1, keepdim=True)
    return (p @ vh).transpose(1, 2).reshape(q.shape[0], q.shape[1], -1), s, p


def regime_inputs(regime, Lk):
    """q, k (fp32, [B][L][H * 64]) of the named regime from seeded rnd inputs, with the regime's own label asserted on the float64
    scores, so that a case cannot drift out of the regime it claims.  A lead of x in the score is built on one head dimension:
    q[.., 0] = 4 in every head and 2 x added to that dimension of the leading key (score = q . k / 8)."""
    q, k = rnd((B_, LQ, D_), "dr.at.q"), rnd((B_, Lk, D_), "dr.at.k")
    d0 = torch.arange(H_) * 64

    def lead(j, x):
        """key j leads by x in the score of every query"""
        q[:, :, d0] = 4.0
        k[:, j, d0] += 2.0 * x
    if regime == "flat":
        k *= 2.0 ** -9
    elif regime == "sharp":
        lead(Lk // 2, 60.0)
    elif regime == "winner":
        lead(Lk // 3, 125.0)
    elif regime == "late_max":
        lead(Lk - 1, 8.0)
    elif regime == "early_max":
        lead(0, 8.0)
    elif regime == "twin":
        lead(5, 8.0)
        k[:, Lk - 1] = k[:, 5]                    # key Lk - 1 (second / third chunk) is key 5 (first chunk) again
    elif regime == "diffuse":
        k *= 2.0 ** -9
        lead(Lk // 2, 7.0 * math.log(2.0))
    elif regime == "cross":
        # the cross-attention operating point: K rows = a float64 linear map (N(0, 0.02)-sized weights, like the caption K/V
        # projection) of rows with unit l2 norm in 512 dimensions -- every entry far below 2^-3
        cond = synth.synth_cond_emb(B_, seq=Lk, dim=512, key="dr.at.cond").double()
        k = (cond @ rnd((D_, 512), "dr.at.wk", 0.035).double().t()).float()
    else:
        assert regime == "unit"
    _, s, p = attention64(q, k, torch.zeros(B_, Lk, D_))
    top2 = s.topk(2, dim=-1).values
    if regime in ("flat",):
        assert float(s.abs().max()) <= 2.0 ** -6
        ent = -(p * p.log()).sum(-1)
        assert float((ent - math.log(Lk)).abs().max()) < 1e-3
    elif regime == "sharp":
        # p_lead > 1 - 1e-20 is not representable in float64 (p_lead rounds to 1): stated on the others' weight relative to the
        # leading key, sum_{j != lead} exp(s_j - s_lead) = (1 - p_lead) / p_lead
        rest = (torch.exp(s - s.max(-1, keepdim=True).values) * (torch.arange(Lk) != Lk // 2)).sum(-1)
        assert bool((s.argmax(-1) == Lk // 2).all()) and 0.0 < float(rest.min()) and float(rest.max()) < 1e-20 and float(p.min()) > 0.0
        assert 50.0 < float((top2[..., 0] - top2[..., 1]).min()) and float((top2[..., 0] - top2[..., 1]).max()) < 75.0
    elif regime == "winner":
        assert bool((s.argmax(-1) == Lk // 3).all()) and float((top2[..., 0] - top2[..., 1]).min()) > 110.0
    elif regime in ("late_max", "early_max"):
        j = Lk - 1 if regime == "late_max" else 0
        assert bool((s.argmax(-1) == j).all()) and float(p[..., j].min()) > 0.5 and float(p[..., j].max()) < 1 - 1e-4
    elif regime == "twin":
        assert 5 < 96 <= Lk - 1 and bool((s[..., 5] == s[..., Lk - 1]).all()) and bool((s.max(-1).values == s[..., 5]).all())
        assert float(p[..., 5].max()) < 0.5
    elif regime == "diffuse":
        rel = torch.exp(s - s.max(-1, keepdim=True).values)
        others = torch.ones(Lk, dtype=torch.bool)
        others[Lk // 2] = False
        assert bool((s.argmax(-1) == Lk // 2).all())
        assert float(rel[..., others].min()) > 2.0 ** -7.5 and float(rel[..., others].max()) < 2.0 ** -6.5
        assert float(rel[..., others].sum(-1).min()) > 1.0            # together they hold most of the mass
    elif regime == "cross":
        assert float(k.abs().max()) < IN_RANGE and 0.01 < float(k.abs().median()) < 0.1
    return q, k


def values(regime, Lk, vname):
    if regime == "cross":
        cond = synth.synth_cond_emb(B_, seq=Lk, dim=512, key="dr.at.cond").double()
        v = (cond @ rnd((D_, 512), "dr.at.wv", 0.035).double().t()).float() * SCALE[vname]
    else:
        v = rnd((B_, Lk, D_), "dr.at.v", SCALE[vname])
    if vname == "hot6e4":
        v[:, :, torch.arange(H_) * 64 + HOT] *= 6e4
    return v


def run_forms(L, q, k, v, Lk):
    """every inference form on the same fp32 q, k, v -> {form: [B * Lq][D] fp32 on the host}; the split and the ready form must
    equal ds_attention_f16x2 bit for bit (their planes = the split of its output)"""
    qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
    M = B_ * LQ
    M16 = (M + 15) // 16 * 16
    qkv = (L.ptr(qc), D_, L.ptr(kc), D_, L.ptr(vc), D_)
    out = {}
    for form in ("ds_attention", "ds_attention_f16x2"):
        o = torch.full((M, D_), float("nan"), device="cuda")
        L.check(getattr(L.lib(), form)(*qkv, L.ptr(o), D_, B_, H_, LQ, Lk, SM_SCALE, L.stream()))
        out[form] = o
    o = torch.full((M, D_), float("nan"), device="cuda")
    L.check(L.lib().ds_attention_ex(*qkv, L.ptr(o), D_, B_, H_, LQ, Lk, SM_SCALE, 1, 0, L.stream()))
    out["ds_attention_ex.causal"] = o
    sp = torch.zeros(2, M16 * D_, device="cuda", dtype=torch.float16)
    L.check(L.lib().ds_attention_f16x2_split(*qkv, L.ptr(sp), D_, B_, H_, LQ, Lk, SM_SCALE, L.stream()))
    qh = torch_split(qc).view(2, B_, LQ, H_, 64).permute(0, 1, 3, 2, 4).contiguous()
    nkey = L.lib().ds_attn_nkey(Lk)
    img = torch.full((B_, H_, 4, nkey * 64), float("nan"), device="cuda", dtype=torch.float16)
    kv = torch.cat((kc, vc), dim=2).contiguous()
    L.check(L.lib().ds_attn_pack_kv(L.ptr(kv), 2 * D_, D_, L.ptr(img), B_, H_, Lk, L.stream()))
    rd = torch.zeros_like(sp)
    L.check(L.lib().ds_attention_f16x2_ready(L.ptr(qh), B_ * H_ * LQ * 64, L.ptr(img), L.ptr(rd), D_, B_, H_, LQ, Lk, SM_SCALE,
                                             L.stream()))
    want = torch_split(out["ds_attention_f16x2"])
    assert torch.equal(L.unpack_planes(sp, M, D_), want), "ds_attention_f16x2_split is not the split of ds_attention_f16x2"
    assert torch.equal(rd, sp), "ds_attention_f16x2_ready differs from ds_attention_f16x2_split"
    for form, pl in (("ds_attention_f16x2_split", sp), ("ds_attention_f16x2_ready", rd)):
        u = L.unpack_planes(pl, M, D_)
        out[form] = u[0].float() + u[1].float()
    torch.cuda.synchronize()
    return {f: o.cpu().double().view(B_, LQ, D_) for f, o in out.items()}


def lo_term(v, s, causal):
    """The lo-term of the bound, 2^-25 sum_key |v| / rowsum: the documented error model of the un-scaled split (2^-25 absolute per
    operand below 2^-3) carried through P V, per output element [B][Lq][D], from the float64 scores.  With e_j = exp(s_j - max) (the
    un-normalised probabilities the kernel splits) and rowsum = sum_j e_j:
    P side 2^-25 sum_{j: e_j < 2^-3} |v_jd| / rowsum  (each such probability is off by up to 2^-25 absolute, whatever its size);
    V side, the same model with the operands' roles exchanged, 2^-25 sum_{j: |v_jd| < 2^-3} e_j / rowsum.
    Both vanish where no probability and no V entry is below 2^-3.  (The same model for Q K^T -- sub-2^-3 entries of q and k move a
    score by up to 2^-28 sum |.| -- was measured and is NOT needed: no case comes near F without it.)"""
    if causal:
        s = s + torch.full(s.shape[-2:], float("-inf"), dtype=s.dtype).triu_(1)
    e = torch.exp(s - s.max(-1, keepdim=True).values)                     # [B][H][Lq][Lk]
    rowsum = e.sum(-1, keepdim=True)
    vh = heads_of(v.double())
    p_side = ((e < IN_RANGE) & (e > 0)).double() @ vh.abs() / rowsum      # (e = 0: a masked key, never loaded)
    v_side = e @ (vh.abs() < IN_RANGE).double() / rowsum
    return (LO_ABS * (p_side + v_side)).transpose(1, 2).reshape(v.shape[0], s.shape[2], -1)


def yardstick(o32, ref, cm):
    """d32 of column block cm: (max |o32 - ref| / max |ref|, RMS(o32 - ref) / RMS(ref)) of the plain fp32 torch evaluation,
    floored at what storing the exact result in fp32 costs (half an ulp: 2^-24 relative at the largest element; 2^-25 in RMS) --
    in the sharp regimes the fp32 evaluation returns a V row exactly, and no fp32 output can be asked to beat fp32's rounding"""
    d, r = (o32 - ref)[..., cm], ref[..., cm]
    return (max(float(d.abs().max()) / float(r.abs().max()), EPS32),
            max(float(d.pow(2).mean().sqrt()) / float(r.pow(2).mean().sqrt()), EPS32 / 2))


ATT_CASES = [(r, lk) for r in ("flat", "unit", "sharp", "winner") for lk in LKS] \
    + [(r, lk) for r in ("late_max", "early_max", "twin") for lk in (97, 265)] + [("diffuse", 265), ("cross", 77)]


@pytest.mark.parametrize("regime,Lk", ATT_CASES)
def test_attention_forms_vs_float64(L, regime, Lk):
    """Every inference form in one softmax regime at one key count, crossed with V at 2^-12, 1, 6e4 and with one hot head-dimension
    column at 6e4 (the cross-attention point: V from the same kind of map as K, at its natural scale and with the hot column).
    late_max / early_max: the dominant key is the last / the first one, so the streamed kernel rescales by exp(m_old - m_new) in
    its last chunk / never; twin: two equal maxima in different chunks; diffuse: needs (Lk - 1) 2^-7 > 1, i.e. the 265-key shape.
    winner: the output row must be the leading key's V row to the rounding of the format (2^-23 relative: one fp32 ulp, and what the
    split keeps of V from 2^-2 up; 2^-25 absolute below; twice that for the forms whose output is split again; three more fp32
    roundings and the split of the leading probability in the f16x2 kernel, where that probability is not exactly 1)."""
    q, k = regime_inputs(regime, Lk)
    failures = []
    for vname in (["1", "hot6e4"] if regime == "cross" else VSCALES):
        v = values(regime, Lk, vname)
        refs = {c: attention64(q, k, v, causal=c) for c in (False, True)}
        assert float(refs[False][0].abs().max()) < 65504.0 and float(refs[True][0].abs().max()) < 65504.0
        o32 = {False: O._mha(q, k, v, H_).double(), True: attention64(q, k, v, causal=True, dtype=torch.float32)[0].double()}
        outs = run_forms(L, q, k, v, Lk)
        hot = torch.zeros(D_, dtype=torch.bool)
        hot[torch.arange(H_) * 64 + HOT] = True
        blocks = [("hot column", hot), ("other columns", ~hot)] if vname == "hot6e4" else [("", torch.ones(D_, dtype=torch.bool))]
        for form in FORMS:
            causal = form.endswith("causal")
            ref, s, _ = refs[causal]
            o = outs[form]
            assert torch.isfinite(o).all(), (form, regime, Lk, vname)
            lo = lo_term(v, s, causal) if "f16x2" in form else torch.zeros_like(ref)
            # FINDING (a departure from the issue's lo-term, needed and explained by the same error model): the split and the ready
            # form store their OUTPUT as un-scaled split planes, so an output below 2^-3 keeps 2^-25 absolute like any other split
            # operand.  With V at 2^-12 the outputs are ~2^-14 and that is 2^-11 relative: measured 45 .. 530 x the yardstick
            # beyond the P V lo-term, 0 beyond this one.  The fp32-store form does not get it.
            resplit = LO_ABS * (ref.abs() < IN_RANGE) if "split" in form or "ready" in form else torch.zeros_like(ref)
            for label, cm in blocks:
                dmax, drms = yardstick(o32[causal], ref, cm)
                err = (o - ref)[..., cm].abs()
                top, rr = float(ref[..., cm].abs().max()), float(ref[..., cm].pow(2).mean().sqrt())

                def ratio_net(allow):
                    """the part of the error that `allow` does not explain, in units of the yardstick (max-abs and RMS)"""
                    d = (err - allow[..., cm]).clamp(min=0)
                    return max(float(d.max()) / top / dmax, float(d.pow(2).mean().sqrt()) / rr / drms)
                raw, net = ratio_net(torch.zeros_like(ref)), ratio_net(lo + resplit)
                tab = RAW_SMALL_V if vname == "2^-12" or regime == "cross" else RAW
                tab[(form, regime)] = max(tab.get((form, regime), 0.0), raw)
                RATIOS[(form, regime)] = max(RATIOS.get((form, regime), 0.0), net)
                print("%s %s Lk %d V %s %s: max %.2e rms %.2e of |ref|; fp32 torch %.2e / %.2e; kernel / d32 raw %.2f, net of the "
                      "lo-term %.2f (lo-term up to %.2e); net of the P V lo-term alone %.2f"
                      % (form, regime, Lk, vname, label, float(err.max()) / top, float(err.pow(2).mean().sqrt()) / rr, dmax, drms,
                         raw, net, float((lo + resplit)[..., cm].max()) / top, ratio_net(lo)))
                if net > F_FORM[form]:
                    failures.append("%s %s Lk %d V %s %s: %.2f x the fp32 yardstick" % (form, regime, Lk, vname, label, net))
            if regime == "winner":
                # FINDING: the fp32 kernels return the leading key's V row to fp32 rounding (one ulp, 2^-23 |v|; measured: exactly),
                # the f16x2 forms do not -- they are allowed, and need, up to 2.75 ulp (5.5 where the output is split again).
                # What the formats keep of v: hi + lo is one fp32 ulp from 2^-2 up and, below, 2^-25 absolute (lo = fp16(v - hi) is
                # subnormal as soon as |v - hi| < 2^-14, which is every |v| < 2^-2: at 2^-3 that is the 22 bits the header
                # promises); the forms whose output is split again pay it twice.  The f16x2 kernel folds the softmax scale into
                # exp2(fma(s, c, -m c)), so its leading probability is 2^(rounding residual of m c), not 1: p v, the sum and the
                # division by the row sum each round once more in fp32 (3 x 2^-24 |v|), and that probability 1 + d is itself split
                # with a subnormal lo plane (2^-25 relative to it).  The causal form: the queries that can see the leading key.
                sees = torch.arange(LQ) >= (Lk // 3 if causal else 0)
                vrow = v.double()[:, Lk // 3][:, None, :].expand_as(ref)
                n = 2 if "split" in form or "ready" in form else 1
                tol = 2.0 ** -23 * vrow.abs()
                if "f16x2" in form:
                    tol = n * tol.clamp(min=LO_ABS) + (3 * EPS32 + LO_ABS) * vrow.abs()
                if bool(sees.any()):
                    worst = float(((o - vrow).abs() / tol.clamp(min=1e-300))[:, sees].max())
                    print("%s winner Lk %d V %s: worst |out - v_lead| / tolerance %.3f, in ulp of v %.3f" % (
                        form, Lk, vname, worst, float(((o - vrow).abs() / (2.0 ** -23 * vrow.abs()).clamp(min=1e-300))[:, sees].max())))
                    assert worst <= 1.0, (form, Lk, vname, worst)
    assert not failures, failures


# =============================================== (d) the denoiser's range guard ===============================================
GUARD_ROW = "transformer.transformer.blocks.1.mlp.0.weight"


def _hot_denoiser(factor, mode):
    """2-layer trained-like denoiser with the hot hidden unit of the LAST block's FC1 (row 5, synth.py) boosted: FC2's operand
    there reaches ~factor x 1.6e3 on the inputs below -> (model, state dict)"""
    from text_to_sound_synthesis_amd.config import build_model, default_config
    sd = dict(synth_sd("dalle", 2, profile="trained"))
    w = sd[GUARD_ROW].clone()
    w[5] *= factor
    sd[GUARD_ROW] = w
    m = build_model(default_config(n_layer=2, diffusion_step=100))
    _, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected
    m.transformer.transformer.precision = mode
    return m.cuda().eval(), sd


@pytest.mark.parametrize("factor,lo,hi,falls_back", [(35.0, 5.5e4, 65504, False), (60.0, 9e4, 1.5e5, True)])
def test_denoiser_range_guard(factor, lo, hi, falls_back):
    """The GELU2 output of one hidden unit into FC2 (the one split site of the denoiser that DESIGN.md 4.2 finds within 2^3 of
    65504): at ~5.6e4 the f16x2 mode runs (the monitor is on, nothing falls back) and is as close to float64 as the fp32 mode; at
    ~9.6e4, where the split saturates, the guard recomputes the call in the fp32 mode -- the logits ARE the fp32 mode's, and a
    3-step sampling chain from the same tokens returns the fp32 mode's tokens.  The style of test_decode_range_guard
    (tests/test_hip_codec_vocoder_range.py)."""
    tok = synth.synth_tokens(2, mask_frac=0.5, key="dr.guard.tokens")
    cond = synth.synth_cond_emb(2, key="dr.guard.cond")
    t = torch.tensor([63, 7])
    out, chain, fallbacks = {}, {}, {}
    for mode in ("f16x2", "fp32"):
        m, sd = _hot_denoiser(factor, mode)
        dt, tr = m.transformer, m.transformer.transformer
        dt.rng_mode = "philox"
        with warnings.catch_warnings(record=True):
            warnings.simplefilter("always")
            out[mode] = tr(tok.cuda(), cond.cuda(), t.cuda()).cpu().double()
            after_forward = tr.range_fallbacks
            chain[mode] = dt._reverse(cond.cuda(), [(7, 7), (6, 6), (5, 5)], None, False, start_tokens=tok)["content_token"].cpu()
        fallbacks[mode] = (after_forward, tr.range_fallbacks - after_forward)
        assert tr.precision == mode                                   # the strict recompute leaves the mode as it was
        assert (tr.packed()["range_peak"] is not None) == (mode == "f16x2")
        del m
        torch.cuda.empty_cache()
    rec = {}
    with torch.no_grad():
        ref = O.transformer_forward({k: v.double() for k, v in sd.items() if k.startswith("transformer.transformer.")},
                                    tok, cond.double(), t, record=rec)
    amax = max(v[0] for k, v in rec.items() if k.endswith("mlp.2"))
    assert lo < amax < hi
    e = {mode: float((o - ref).abs().max()) for mode, o in out.items()}
    floor = EPS32 * float(ref.abs().max())
    line = "denoiser guard: hot FC2 operand %.3g -> range_fallbacks (forward, chain) %s; logits vs float64 f16x2 %.2e, fp32 mode " \
        "%.2e (max-abs; floor %.1e)" % (amax, fallbacks["f16x2"], e["f16x2"], e["fp32"], floor)
    print(line)
    parity_line(line)
    assert fallbacks["fp32"] == (0, 0)
    assert all(torch.isfinite(o).all() for o in out.values())
    assert e["f16x2"] <= max(2 * e["fp32"], floor)                    # the strict yardstick of the codec's guard tests
    if falls_back:
        assert fallbacks["f16x2"] == (1, 1)
        assert torch.equal(out["f16x2"], out["fp32"])                 # the same fp32-mode computation, not an f16x2 result
        assert torch.equal(chain["f16x2"], chain["fp32"])
    else:
        assert fallbacks["f16x2"][0] == 0
