"""The split-fp16 convolutions of the SpecVQGAN codec and the MelGAN vocoder across the operand range, against float64.

The f16x2 kernels split an UN-scaled fp32 operand a into fp16 hi + lo (csrc/common.h ds_split_hi / ds_split_lo): fp32-class for
|a| in about [2^-3, 65504]; below 2^-3 the lo plane is subnormal and keeps 2^-25 of absolute precision; above 65504 the split
saturates.  (a) every split-conv entry at whole-tensor operand scales 2^-12 .. 6e4 and with one hot channel at 6e4, against
float64 and against the exact-fp32 gather-GEMM on the same inputs; (b) VQModel.decode / encode and the Generator on the "init"
and the trained-like "trained_conv" weights (synth.py) in both arithmetic modes against the project's float64 oracle; (c) proof
from the oracle's operand record that the trained-like weights reach both edges; (d) the range guard of decode() and of the
Generator: operands past 65504 are recomputed in the strict mode, and nothing below falls back.  GPU only (-m gpu)."""
import warnings

import pytest
import torch
import torch.nn.functional as F

import diffsound_oracle as O
from conftest import parity_line, synth_sd
from text_to_sound_synthesis_amd import synth

pytestmark = pytest.mark.gpu
NO_GRAD = True

EPS32 = 2.0 ** -24
LO_ABS = 2.0 ** -25          # absolute precision of a subnormal fp16 lo plane (half its spacing, 2^-24)
C_LO = 1.0                   # the documented bound:  |err| <= C_LO * 2^-25 * sum |w|  per split (+ the fp32-class term)
# ... a worst case.  With independent rounding errors (uniform, |e| <= 2^-25: standard deviation 2^-25 / sqrt 3 per operand) the
# RMS over outputs of err / ||w||_2 is ~0.58 x 2^-25; RMS_LO (1.7x that) is the statistical bound the small cases also meet
RMS_LO = 2.0 ** -25
SCALES = ["2^-12", "2^-6", "1", "2^14", "6e4", "hot6e4"]
SCALE = {"2^-12": 2.0 ** -12, "2^-6": 2.0 ** -6, "1": 1.0, "2^14": 2.0 ** 14, "6e4": 6e4, "hot6e4": 1.0}
HOT = 5


@pytest.fixture(scope="module")
def L():
    from text_to_sound_synthesis_amd import _lib
    _lib.lib()
    return _lib


def rnd(shape, key, scale=1.0):
    return (synth.synth_uniform(shape, key=key) * 2 - 1) * scale


def operand(shape, key, sname):
    """channels-last operand at the named scale; "hot6e4": O(1) everywhere but channel HOT, which runs at up to 6e4"""
    x = rnd(shape, key, SCALE[sname])
    if sname == "hot6e4":
        x[..., HOT] *= 6e4
    return x


def l1_rows(w):
    """(sum |w|, ||w||_2) per output row of a [N][K] matrix (float64)"""
    w = w.double().reshape(w.shape[0], -1)
    return w.abs().sum(1), w.norm(dim=1)


def _c3(L, sname, mode):
    B, H, W, Cin, Cout = (1, 8, 64, 32, 128) if mode == "up" else (1, 6, 40, 32, 128)
    up = 1 if mode == "up" else 0
    hs, ws = (H // 2, W // 2) if up else (H, W)
    s = SCALE[sname]
    w, bias = rnd((Cout, Cin, 3, 3), "rg.c3.w", 0.1), rnd((Cout,), "rg.c3.b", s)
    R = rnd((B, H, W, Cout), "rg.c3.r", s)
    if mode == "gn":        # operand swish(x sc + sh) at the named scale
        x = rnd((B, hs, ws, Cin), "rg.c3.x")
        sc = (rnd((B, Cin), "rg.c3.s") * 0.25 + 0.75) * 0.9 * s
        sh = rnd((B, Cin), "rg.c3.o", 0.05 * s)
        if sname == "hot6e4":
            sc[:, HOT] *= 0.9 * 6e4
        xin = x.permute(0, 3, 1, 2).double() * sc.double()[:, :, None, None] + sh.double()[:, :, None, None]
        xin = xin * torch.sigmoid(xin)
    else:
        x = operand((B, hs, ws, Cin), "rg.c3.x", sname)
        sc = sh = None
        xin = x.permute(0, 3, 1, 2).double()
    if up:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xin, w.double(), bias.double(), padding=1).permute(0, 2, 3, 1) + R.double()
    wp = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous().cuda()
    w2, osc = L.split_f16x2(wp)
    wq = L.pack_conv3x3_weights(w2, Cout, Cin)
    xc, Rc, bc = x.cuda(), R.cuda(), bias.cuda()
    scc, shc = (sc.cuda(), sh.cuda()) if sc is not None else (None, None)
    y = torch.full((B, H, W, Cout), float("nan"), device="cuda")
    part = torch.empty(B, L.lib().ds_conv3x3_tiles(H, W), 2, Cout, device="cuda", dtype=torch.float64)
    L.check(L.lib().ds_conv3x3_f16x2(L.ptr(xc), L.ptr(wq), wq.numel(), osc, L.ptr(bc), L.ptr(Rc), L.ptr(y), B, H, W, Cin, Cout,
                                     up, L.ptr(scc), L.ptr(shc), L.ptr(part), L.stream()))
    y32 = torch.empty(B, H, W, Cout, device="cuda")
    L.gemm(xc, wp, y32, B * H * W, Cout, 9 * Cin, bias=bc, R=Rc, loader=L.LOAD_CONV2D,
           pro=L.PRO_AFFINE_SWISH if sc is not None else L.PRO_NONE, pro_scale=scc, pro_shift=shc, Cin=Cin, H=H, Wd=W, up=up)
    l1, l2 = l1_rows(wp)
    # nearest-2x: up to four taps of a window read the same source pixel, so their rounding errors add coherently
    return y, y32, ref, (l1, l2 * (2.0 if up else 1.0))


def _gather2d(L, sname, stride2):
    """the tap-by-tap gather kernel with conv_split (conv_f16x2.hip, CONV2D loader): stride 1 and the encoder's stride-2
    Downsample (zero pad right / bottom)"""
    B, H, W, Cin, Cout = 1, 5, 53, 64, 128            # output grid; the stride-2 input is 2H x 2W
    hi, wi = (2 * H, 2 * W) if stride2 else (H, W)
    s = SCALE[sname]
    x = operand((B, hi, wi, Cin), "rg.g2.x%d" % stride2, sname)
    w, bias = rnd((Cout, Cin, 3, 3), "rg.g2.w", 0.1), rnd((Cout,), "rg.g2.b", s)
    xin = x.permute(0, 3, 1, 2).double()
    if stride2:
        ref = F.conv2d(F.pad(xin, (0, 1, 0, 1)), w.double(), bias.double(), stride=2)
    else:
        ref = F.conv2d(xin, w.double(), bias.double(), padding=1)
    ref = ref.permute(0, 2, 3, 1)
    wp = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous().cuda()
    w2, osc = L.split_f16x2(wp)
    xc, bc = x.cuda(), bias.cuda()
    kw = dict(bias=bc, loader=L.LOAD_CONV2D, Cin=Cin, H=H, Wd=W, up=2 if stride2 else 0)
    y = torch.full((B, H, W, Cout), float("nan"), device="cuda")
    L.gemm(xc, w2, y, B * H * W, Cout, 9 * Cin, split2=osc, conv_split=True, **kw)
    y32 = torch.empty(B, H, W, Cout, device="cuda")
    L.gemm(xc, wp, y32, B * H * W, Cout, 9 * Cin, **kw)
    return y, y32, ref, l1_rows(wp)


def _gather1d(L, sname):
    """the first MelGAN layer's form: k7 Conv1d with ReflectionPad1d(3), CONV1D loader"""
    B, T, Cin, Cout = 2, 150, 96, 128
    s = SCALE[sname]
    x = operand((B, T, Cin), "rg.g1.x", sname)
    w, bias = rnd((Cout, Cin, 7), "rg.g1.w", 0.05), rnd((Cout,), "rg.g1.b", s)
    ref = F.conv1d(F.pad(x.double().permute(0, 2, 1), (3, 3), mode="reflect"), w.double(), bias.double()).permute(0, 2, 1)
    wp = w.permute(0, 2, 1).reshape(Cout, -1).contiguous().cuda()
    w2, osc = L.split_f16x2(wp)
    xc, bc = x.cuda(), bias.cuda()
    kw = dict(bias=bc, loader=L.LOAD_CONV1D, Cin=Cin, Wd=T, taps=7, dil=1)
    y = torch.full((B, T, Cout), float("nan"), device="cuda")
    L.gemm(xc, w2, y, B * T, Cout, 7 * Cin, split2=osc, conv_split=True, **kw)
    y32 = torch.empty(B, T, Cout, device="cuda")
    L.gemm(xc, wp, y32, B * T, Cout, 7 * Cin, **kw)
    return y, y32, ref, l1_rows(wp)


def _convt_setup(sname, cin, cout, T, r, key):
    B, pad = 2, r // 2 + r % 2
    s = SCALE[sname]
    x = operand((B, T, cin), key + ".x", sname)
    w, bias = rnd((cin, cout, 2 * r), key + ".w", 0.05), rnd((cout,), key + ".b", s)
    ref = F.conv_transpose1d(F.leaky_relu(x.double().permute(0, 2, 1), 0.2), w.double(), bias.double(), stride=r, padding=pad,
                             output_padding=r % 2).permute(0, 2, 1)
    wph = w.permute(2, 1, 0).reshape(2, r, cout, cin).permute(1, 2, 0, 3).reshape(r, cout, 2 * cin).contiguous()
    return B, pad, x, bias, ref, wph


def _convt_fp32(L, xc, wph, bc, B, T, cin, cout, r, pad):
    y32 = torch.empty(B, T * r, cout, device="cuda")
    L.gemm(xc, wph.reshape(-1, 2 * cin).contiguous().cuda(), y32, B * T, cout, 2 * cin, bias=bc, ldc=cout, loader=L.LOAD_CONVT1D,
           pro=L.PRO_LRELU, store=L.STORE_CONVT, groups=r, w_gstride=cout * 2 * cin, Cin=cin, Wd=T, ct_r=r, ct_p=pad, ct_tin=T)
    return y32


def _convt_l1(wph):
    """per output channel: the largest over the output phases of sum |w| and of ||w||_2 (each output sample is one phase's dot
    product)"""
    w = wph.double()
    return w.abs().sum(2).max(0).values, w.norm(dim=2).max(0).values


def _gather_convt(L, sname):
    cin, cout, T, r = 256, 128, 40, 8
    B, pad, x, bias, ref, wph = _convt_setup(sname, cin, cout, T, r, "rg.gt")
    planes, osc = L.split_f16x2(wph.reshape(-1, 2 * cin).cuda())
    xc, bc = x.cuda(), bias.cuda()
    y = torch.full((B, T * r, cout), float("nan"), device="cuda")
    L.gemm(xc, planes, y, B * T, cout, 2 * cin, split2=osc, conv_split=True, bias=bc, ldc=cout, loader=L.LOAD_CONVT1D,
           pro=L.PRO_LRELU, store=L.STORE_CONVT, groups=r, w_gstride=cout * 2 * cin, Cin=cin, Wd=T, ct_r=r, ct_p=pad, ct_tin=T)
    return y, _convt_fp32(L, xc, wph, bc, B, T, cin, cout, r, pad), ref, _convt_l1(wph)


def _halo_convt(L, sname):
    cin, cout, T, r = 256, 128, 53, 8
    B, pad, x, bias, ref, wph = _convt_setup(sname, cin, cout, T, r, "rg.ht")
    planes, osc = L.split_f16x2(wph.reshape(-1, 2 * cin).cuda())
    pl = planes.view(2, r, cout, 2 * cin)
    wq = torch.cat([L.pack_conv_weights(pl[:, g].contiguous(), cout, cin, 2) for g in range(r)])
    xc, bc = x.cuda(), bias.cuda()
    y = torch.full((B, T * r, cout), float("nan"), device="cuda")
    L.check(L.lib().ds_convt1d_f16x2(L.ptr(xc), L.ptr(wq), wq.numel(), osc, L.ptr(bc), L.ptr(y), B, T, cin, cout, r, pad, 1,
                                     L.stream()))
    return y, _convt_fp32(L, xc, wph, bc, B, T, cin, cout, r, pad), ref, _convt_l1(wph)


def _convt2(L, sname, cin, cout):
    T, r = 300, 2
    B, pad, x, bias, ref, wph = _convt_setup(sname, cin, cout, T, r, "rg.c2.%d" % cin)
    planes, osc = L.split_f16x2(wph.reshape(-1, 2 * cin).cuda())
    xc, bc = x.cuda(), bias.cuda()
    y = torch.full((B, T * r, cout), float("nan"), device="cuda")
    L.check(L.lib().ds_melgan_convt2(L.ptr(xc), L.ptr(planes), 2 * cout * 2 * cin, osc, L.ptr(bc), L.ptr(y), B, T, cin, cout,
                                     L.stream()))
    return y, _convt_fp32(L, xc, wph, bc, B, T, cin, cout, r, pad), ref, _convt_l1(wph)


def _k3(L, sname):
    B, T, C, dil = 2, 300, 128, 3
    s = SCALE[sname]
    x = operand((B, T, C), "rg.k3.x", sname)
    w, bias = rnd((C, C, 3), "rg.k3.w", 0.1), rnd((C,), "rg.k3.b", s)
    ref = F.conv1d(F.pad(F.leaky_relu(x.double().permute(0, 2, 1), 0.2), (dil, dil), mode="reflect"), w.double(), bias.double(),
                   dilation=dil).permute(0, 2, 1)
    wp = w.permute(0, 2, 1).reshape(C, 3 * C).contiguous().cuda()
    planes, osc = L.split_f16x2(wp)
    wq = L.pack_conv_weights(planes, C, C, 3)
    xc, bc = x.cuda(), bias.cuda()
    y = torch.full((B, T, C), float("nan"), device="cuda")
    L.check(L.lib().ds_conv1d_k3_f16x2(L.ptr(xc), L.ptr(wq), wq.numel(), osc, L.ptr(bc), L.ptr(y), B, T, C, C, dil, 1, L.stream()))
    y32 = torch.empty(B, T, C, device="cuda")
    L.gemm(xc, wp, y32, B * T, C, 3 * C, bias=bc, loader=L.LOAD_CONV1D, pro=L.PRO_LRELU, Cin=C, Wd=T, taps=3, dil=dil)
    return y, y32, ref, l1_rows(wp)


def _block_weights(C, key, s):
    # the k3 rows are normalised to sum |w| = 0.9, so that h1 (which the single-pass kernel splits in registers) stays within
    # the operand's own range: every operand of the block then sits at the named scale
    w3 = rnd((C, C, 3), key + ".w3", 0.15)
    w3 = w3 * (0.9 / w3.abs().sum((1, 2), keepdim=True))
    w2, ws = rnd((C, C), key + ".w2", 0.2), rnd((C, C), key + ".ws", 0.2)
    b3, b2, bs = rnd((C,), key + ".b3", 0.05 * s), rnd((C,), key + ".b2", s), rnd((C,), key + ".bs", s)
    return w3, w2, ws, b3, b2, bs


def _block_fp32(L, xc, w3, b3, w2, b2, ws, bs, B, T, C, dil):
    """the strict Generator's three gather-GEMMs for one ResnetBlock"""
    h1 = torch.empty(B, T, C, device="cuda")
    L.gemm(xc, w3.permute(0, 2, 1).reshape(C, 3 * C).contiguous().cuda(), h1, B * T, C, 3 * C, bias=b3.cuda(), loader=L.LOAD_CONV1D,
           pro=L.PRO_LRELU, Cin=C, Wd=T, taps=3, dil=dil)
    y = torch.empty(B, T, C, device="cuda")
    L.gemm(xc, ws.contiguous().cuda(), y, B * T, C, C, bias=bs.cuda())
    L.gemm(h1, w2.contiguous().cuda(), y, B * T, C, C, bias=b2.cuda(), R=y, pro=L.PRO_LRELU)
    return y


def _resblock(L, sname, C, T, dil, fused):
    B = 3 if fused else 2
    s = SCALE[sname]
    x = operand((B, T, C), "rg.rb.x%d" % C, sname)
    w3, w2, ws, b3, b2, bs = _block_weights(C, "rg.rb%d" % C, s)
    xd = x.double().permute(0, 2, 1)
    h = F.conv1d(F.pad(F.leaky_relu(xd, 0.2), (dil, dil), mode="reflect"), w3.double(), b3.double(), dilation=dil)
    ref = (F.conv1d(F.leaky_relu(h, 0.2), w2.double()[:, :, None], b2.double())
           + F.conv1d(xd, ws.double()[:, :, None], bs.double())).permute(0, 2, 1)
    p3, s3 = L.split_f16x2(w3.permute(0, 2, 1).reshape(C, 3 * C).contiguous().cuda())
    pt, st = L.split_f16x2(torch.cat((w2, ws), 1).contiguous().cuda())
    xc, b3c, btc = x.cuda(), b3.cuda(), (b2 + bs).cuda()
    if fused:
        assert L.lib().ds_melgan_resblock_fused_ok(T, C, dil) == 1
    hbuf = None if fused else torch.empty(B, T, C, device="cuda")
    y = torch.full((B, T, C), float("nan"), device="cuda")
    L.check(L.lib().ds_melgan_resblock(L.ptr(xc), L.ptr(p3), C * 3 * C, s3, L.ptr(b3c), L.ptr(pt), C * 2 * C, st, L.ptr(btc),
                                       L.ptr(hbuf), L.ptr(y), B, T, C, dil, L.stream()))
    y32 = _block_fp32(L, xc, w3, b3, w2, b2, ws, bs, B, T, C, dil)
    # two splits in a chain: the tail's own operands, and h1's error carried through |W2|
    w2d, wsd, w3d = w2.double(), ws.double(), w3.double()
    l1 = w2d.abs().sum(1) + wsd.abs().sum(1) + w2d.abs() @ w3d.abs().sum((1, 2))
    l2 = (w2d.pow(2).sum(1) + wsd.pow(2).sum(1) + w2d.pow(2) @ w3d.pow(2).sum((1, 2))).sqrt()
    return y, y32, ref, (l1, l2)


def _tail(L, sname):
    M, C = 1000, 128
    s = SCALE[sname]
    h, x = operand((M, C), "rg.tl.h", sname), operand((M, C), "rg.tl.x", sname)
    w2, ws = rnd((C, C), "rg.tl.w2", 0.2), rnd((C, C), "rg.tl.ws", 0.2)
    b = rnd((C,), "rg.tl.b", s)
    ref = F.leaky_relu(h.double(), 0.2) @ w2.double().t() + x.double() @ ws.double().t() + b.double()
    planes, osc = L.split_f16x2(torch.cat((w2, ws), 1).contiguous().cuda())
    hc, xc, bc = h.cuda(), x.cuda(), b.cuda()
    y = torch.full((M, C), float("nan"), device="cuda")
    L.check(L.lib().ds_melgan_resblock_tail(L.ptr(hc), L.ptr(xc), L.ptr(planes), C * 2 * C, osc, L.ptr(bc), L.ptr(y), M, C,
                                            L.stream()))
    y32 = torch.empty(M, C, device="cuda")
    L.gemm(xc, ws.contiguous().cuda(), y32, M, C, C, bias=bc)
    L.gemm(hc, w2.contiguous().cuda(), y32, M, C, C, R=y32, pro=L.PRO_LRELU)
    return y, y32, ref, l1_rows(torch.cat((w2, ws), 1))


KERNELS = {
    "conv3x3_f16x2.plain": lambda L, s: _c3(L, s, "plain"),
    "conv3x3_f16x2.gn": lambda L, s: _c3(L, s, "gn"),
    "conv3x3_f16x2.up": lambda L, s: _c3(L, s, "up"),
    "gather.conv2d": lambda L, s: _gather2d(L, s, False),
    "gather.conv2d_stride2": lambda L, s: _gather2d(L, s, True),
    "gather.conv1d_k7": _gather1d,
    "gather.convt1d_r8": _gather_convt,
    "conv1d_k3_f16x2": _k3,
    "convt1d_f16x2_r8": _halo_convt,
    "melgan_convt2.128_64": lambda L, s: _convt2(L, s, 128, 64),
    "melgan_convt2.64_32": lambda L, s: _convt2(L, s, 64, 32),
    "melgan_resblock.32_fused": lambda L, s: _resblock(L, s, 32, 640, 3, True),
    "melgan_resblock.64_fused": lambda L, s: _resblock(L, s, 64, 768, 9, True),
    "melgan_resblock.64_two_launch": lambda L, s: _resblock(L, s, 64, 500, 3, False),
    "melgan_resblock_tail.128": _tail,
}


@pytest.mark.parametrize("sname", SCALES)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_split_kernel_across_operand_range(L, kernel, sname):
    """In range (|a| from 2^-3 to 65504, the O(1), 2^14, 6e4 and hot-channel cases): relative max error vs float64 within
    max(3e-6, 1.2 x the exact-fp32 gather-GEMM's).  Below 2^-3 (the 2^-12 and 2^-6 cases): per output element within
    C_LO * 2^-25 * sum |w| of that output (the subnormal lo plane's absolute precision) + the fp32-class term, and in RMS
    over the outputs of err / ||w||_2 within RMS_LO + the fp32 gather's.  The worst-case bound alone would not notice a kernel
    that drops the lo plane at these scales (the random-sign error of dropping it stays below it); the RMS bound does at 2^-6,
    where lo holds ~11 bits of a.  At 2^-12 lo holds only 1-3 bits, and it is the in-range cases that catch a missing lo."""
    y, y32, ref, (l1, l2) = KERNELS[kernel](L, sname)
    torch.cuda.synchronize()
    y, y32, ref = y.cpu().double(), y32.cpu().double(), ref.double()
    assert torch.isfinite(y).all()
    top = float(ref.abs().max())
    err, err32 = (y - ref).abs(), (y32 - ref).abs()
    e, e32 = float(err.max()) / top, float(err32.max()) / top
    print("%s @ %s: split %.2e, exact-fp32 gather %.2e (relative max error vs float64; max |ref| %.3g)" % (kernel, sname, e, e32, top))
    if SCALE[sname] >= 1.0:
        assert e <= max(3e-6, 1.2 * e32), "%s @ %s: %.3g vs fp32 %.3g" % (kernel, sname, e, e32)
    else:
        fp32_term = max(3e-6 * top, 1.2 * float(err32.max()))
        bound = C_LO * LO_ABS * l1.cpu().double().view(*([1] * (y.dim() - 1)), -1) + fp32_term
        worst = float((err / bound).max())
        shape = [1] * (y.dim() - 1) + [-1]
        l2 = l2.cpu().double().view(*shape)
        r, r32 = float((err / l2).pow(2).mean().sqrt()), float((err32 / l2).pow(2).mean().sqrt())
        print("   below 2^-3: worst |err| / (2^-25 sum|w| + fp32 term) = %.3f; RMS err / ||w||_2 = %.3f x 2^-25 (fp32 gather %.3f)"
              % (worst, r / RMS_LO, r32 / RMS_LO))
        assert worst <= 1.0, "%s @ %s: %.3g of the documented bound" % (kernel, sname, worst)
        assert r <= RMS_LO + 1.2 * r32, "%s @ %s: RMS %.3g x 2^-25" % (kernel, sname, r / RMS_LO)


@pytest.mark.parametrize("sname", SCALES)
def test_melgan_final_is_exact_fp32_at_every_scale(L, sname):
    """control: ds_melgan_final does not split (an exact fp32 FMA chain of 7 x 32 terms), so at every scale its error stays
    within the fp32-class term 8 eps32 sum |w a| of each output (tanh is 1-Lipschitz) -- no 2^-25 floor, no saturation"""
    B, T, C = 2, 1000, 32
    x = operand((B, T, C), "rg.fin.x", sname)
    w, bias = rnd((7, C), "rg.fin.w", 0.1), 0.05 * min(SCALE[sname], 1.0)
    a = F.pad(F.leaky_relu(x.double().permute(0, 2, 1), 0.2), (3, 3), mode="reflect")
    ref = torch.tanh(F.conv1d(a, w.double().t()[None], torch.tensor([bias], dtype=torch.float64))[:, 0])
    wa = F.conv1d(a.abs(), w.double().abs().t()[None])[:, 0] + abs(bias)
    xc, wc = x.cuda(), w.cuda()
    out = torch.full((B, T), float("nan"), device="cuda")
    L.check(L.lib().ds_melgan_final(L.ptr(xc), L.ptr(wc), bias, L.ptr(out), B, T, C, L.stream()))
    err = (out.cpu().double() - ref).abs()
    worst = float((err / (8 * EPS32 * wa + 2 * EPS32 * ref.abs() + 1e-30)).max())
    print("melgan_final @ %s: worst |err| / (8 eps32 sum|w a| + 2 eps32 |tanh|) = %.3f" % (sname, worst))
    assert worst <= 1.0


# ---- (b) / (c) / (d): modules against the float64 oracle ------------------------------------------------------------------
def _codec_sd(profile):
    sd = {k: v for k, v in synth_sd("dalle", 1, profile=profile).items() if k.startswith("content_codec.")}
    sd.update(synth_sd("encoder", profile=profile))
    return {k[len("content_codec."):]: v for k, v in sd.items()}


def _vqmodel(sd):
    from text_to_sound_synthesis_amd.config import default_config
    from text_to_sound_synthesis_amd.modeling.vqgan import VQModel
    p = default_config(n_layer=1)["model"]["params"]["content_codec_config"]["params"]
    m = VQModel(p["ddconfig"], n_embed=p["n_embed"], embed_dim=p["embed_dim"])
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def _generator(sd):
    from text_to_sound_synthesis_amd.modeling.vocoder import Generator
    g = Generator(80, 32, 3)
    g.load_state_dict(sd)
    return g.cuda().eval()


def _both_modes(mod, fn):
    out = {}
    for mode in ("f16x2", "fp32"):
        mod.conv_precision = mode
        out[mode] = fn().cpu().double()
    mod.conv_precision = "f16x2"
    return out


def _yardstick(name, out, ref, north_star, metric):
    e = {m: metric(o - ref) for m, o in out.items()}
    floor = EPS32 * float(ref.abs().max())
    parity_line("%s: vs float64 f16x2 %.2e, strict fp32 %.2e (%s; floor %.1e)" % (name, e["f16x2"], e["fp32"], metric.__doc__, floor))
    print(name, e, "floor", floor)
    for m in out:
        assert torch.isfinite(out[m]).all()
        assert e[m] <= north_star, (name, m, e[m])
    assert e["f16x2"] <= max(2 * e["fp32"], floor), (name, e)
    return e


def maxabs(d):
    """max-abs"""
    return float(d.abs().max())


def rms(d):
    """RMS"""
    return float(d.pow(2).mean().sqrt())


@pytest.mark.parametrize("profile", ["init", "trained_conv"])
def test_decode_vs_float64_both_modes(profile):
    """VQModel.decode, B = 2 at the full 80 x 848, against the oracle in float64; the guard must not fire"""
    sd = _codec_sd(profile)
    m = _vqmodel(sd)
    tok = synth.synth_tokens(2, mask_frac=0.0, key="rg.dec.codes")
    quant = O.codebook_gather(sd, tok, pfx="")
    rec = {}
    ref = O.vq_decode({k: v.double() for k, v in sd.items()}, quant.double(), pfx="", record=rec)
    out = _both_modes(m, lambda: m.decode(quant.cuda()))
    _yardstick("decode %s B2 80x848" % profile, out, ref, 1e-3, maxabs)
    assert m.range_fallbacks == 0
    raw = {k: v[0] for k, v in rec.items() if "upsample" in k or k.endswith("conv_in")}
    parity_line("decode %s: split operands max |a| %.3g (raw stream %.3g), min of the per-layer max %.3g"
                % (profile, max(v[0] for v in rec.values()), max(raw.values()), min(v[0] for v in rec.values())))
    if profile == "trained_conv":        # (c) the trained-like weights reach the top of the split's range, below 65504
        assert 2 ** 13 < max(raw.values()) < 65504


@pytest.mark.parametrize("profile", ["init", "trained_conv"])
def test_encode_tokens_vs_float64_both_modes(profile):
    """VQModel.encode -> token ids equal the float64 argmin except where the float64 margin between the best two codes is
    below what the measured latent error can move: 2 |dz| max|e_i - e_j| + 1e-5 (|z|^2 + max |e|^2)"""
    sd = _codec_sd(profile)
    m = _vqmodel(sd)
    mel = rnd((2, 1, 80, 848), "rg.enc.mel")
    sd64 = {k: v.double() for k, v in sd.items()}
    rec = {}
    h64 = O.vq_encoder(sd64, mel.double(), pfx="", record=rec)
    idx64, d64 = O.vq_quantize(sd64, h64, pfx="")
    E = sd64["quantize.embedding.weight"]
    spread = float(torch.cdist(E, E).max())
    ds = d64.sort(1).values
    margin = (ds[:, 1] - ds[:, 0])
    lat = {}
    for mode in ("f16x2", "fp32"):
        m.conv_precision = mode
        h = lat[mode] = m.encode_latent(mel.cuda()).cpu().double()
        _, _, info = m.encode(mel.cuda())
        idx = info[2].view(-1).cpu()
        dz = (h - h64).permute(0, 2, 3, 1).reshape(-1, h.shape[1]).norm(dim=1)
        z2 = h64.permute(0, 2, 3, 1).reshape(-1, h.shape[1]).pow(2).sum(1)
        band = 2 * dz * spread + 1e-5 * (z2 + float(E.pow(2).sum(1).max()))
        diff = idx != idx64.view(-1)
        parity_line("encode %s %s: %d of %d tokens differ from float64 (all inside the near-tie band: %s), %d positions inside "
                    "the band, min margin %.2e" % (profile, mode, int(diff.sum()), diff.numel(),
                                                   bool((margin[diff] < band[diff]).all()), int((margin < band).sum()),
                                                   float(margin.min())))
        assert bool((margin[diff] < band[diff]).all()), "a token outside the near-tie band differs"
    _yardstick("encode latent %s B2" % profile, lat, h64, 1e-3, maxabs)
    m.conv_precision = "f16x2"
    if profile == "trained_conv":
        assert 2 ** 13 < max(v[0] for k, v in rec.items() if "downsample" in k) < 65504


@pytest.mark.parametrize("profile", ["init", "trained_conv"])
@pytest.mark.parametrize("B,T", [(1, 848), (3, 53)])
def test_generator_vs_float64_both_modes(profile, B, T):
    sd = synth_sd("generator", profile=profile)
    g = _generator(sd)
    mel = synth.synth_uniform((B, 80, T), key="rg.voc.mel%d" % T)
    rec = {}
    ref = O.melgan_generator({k: v.double() for k, v in sd.items()}, mel.double(), record=rec)
    out = _both_modes(g, lambda: g(mel.cuda()))
    _yardstick("MelGAN %s B%d T%d" % (profile, B, T), out, ref, 1e-4, rms)
    assert g.range_fallbacks == 0
    # the quiet last stage of the trained-like weights is carried at 2^k (exact; chosen at pack time), nothing else is scaled
    k = g._packed()["stage_log2"]
    parity_line("MelGAN %s: stage scales 2^%s" % (profile, k))
    assert k == ([0, 0, 0, k[3]] if profile == "trained_conv" else [0, 0, 0, 0])
    assert profile == "init" or k[3] >= 4
    parity_line("MelGAN %s B%d T%d: split operands max |a| %.3g" % (profile, B, T, max(v[0] for v in rec.values())))
    if profile == "trained_conv":        # (c) one stage whose every split operand sits below 2^-3
        quiet = [k for k in rec if k.startswith(("model.19.", "model.20.", "model.21."))]
        assert len(quiet) == 9 and max(rec[k][0] for k in quiet) < 2 ** -3


def _hot_decoder_sd(factor):
    """trained-like codec with the hot stream channels of level 1 boosted: they reach the up.1 upsample conv at ~factor x 1.56e4"""
    sd = dict(_codec_sd("trained_conv"))
    for b in range(3):
        k = "decoder.up.1.block.%d.conv2.weight" % b
        w = sd[k].clone()
        w[list(synth.CODEC_HOT)] *= factor
        sd[k] = w
    return sd


@pytest.mark.parametrize("factor,lo,hi,falls_back", [(3.8, 5.5e4, 65504, False), (6.4, 9e4, 1.5e5, True)])
def test_decode_range_guard(factor, lo, hi, falls_back):
    """A hot stream channel into decoder.up.1.upsample.conv: at ~6e4 the split mode runs (no fallback) and matches float64; at
    ~1e5 the guard recomputes the chunk in the strict mode, and the result matches float64 within the strict yardstick."""
    sd = _hot_decoder_sd(factor)
    m = _vqmodel(sd)
    tok = synth.synth_tokens(1, mask_frac=0.0, key="range.over.codes")
    quant = O.codebook_gather(sd, tok, pfx="")
    rec = {}
    ref = O.vq_decode({k: v.double() for k, v in sd.items()}, quant.double(), pfx="", record=rec)
    amax = rec["decoder.up.1.upsample.conv"][0]
    assert lo < amax < hi
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        out = _both_modes(m, lambda: m.decode(quant.cuda()))
    _yardstick("decode hot channel %.3g into up.1.upsample" % amax, out, ref, 1e-3, maxabs)
    assert m.range_fallbacks == (1 if falls_back else 0)
    parity_line("decode guard: hot operand %.3g -> range_fallbacks %d" % (amax, m.range_fallbacks))


@pytest.mark.parametrize("val", [2e5, 1e5])
def test_generator_range_guard(val):
    """A vocoder stream channel at val (> 65504) going into the second stage's ResnetBlocks: the guard recomputes the call in
    the strict mode; the waveform matches float64 within the strict yardstick."""
    sd = {k: v.clone() for k, v in synth_sd("generator").items()}
    sd["model.8.bias"][5] = val
    g = _generator(sd)
    mel = synth.synth_uniform((2, 80, 53), key="range.vmel")
    ref = O.melgan_generator({k: v.double() for k, v in sd.items()}, mel.double())
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        out = _both_modes(g, lambda: g(mel.cuda()))
    _yardstick("MelGAN hot channel %.3g" % val, out, ref, 1e-4, rms)
    assert g.range_fallbacks == 1
    parity_line("MelGAN guard: hot stream channel %.3g -> range_fallbacks %d" % (val, g.range_fallbacks))



def test_codebook_search_at_near_ties():
    """ds_vq_argmin on the trained-like codebook's near-duplicate pairs (codes 2j, 2j + 1, j < 8): latents at the pair's midpoint
    moved by delta (e_2j - e_2j+1) (|e_2j - e_2j+1| ~ 1e-3, so the float64 margin is 2 delta |e_2j - e_2j+1|^2) for delta from
    1e-4 to 300, plus a small component orthogonal to the pair.  The margin then runs from far inside to far outside the band
    1e-5 (|z|^2 + max |e|^2) in which fp32 distances may order either way: outside it the GPU's code equals float64's, and
    both sides of the band are populated."""
    from text_to_sound_synthesis_amd.modeling.vqgan import VectorQuantizer
    E = _codec_sd("trained_conv")["quantize.embedding.weight"]
    n, D = E.shape
    g = torch.Generator().manual_seed(7)
    zs = []
    for j in range(8):
        a, b = E[2 * j].double(), E[2 * j + 1].double()
        u = torch.randn(D, generator=g, dtype=torch.float64) * 0.01
        u -= (u @ (a - b)) / (a - b).pow(2).sum() * (a - b)
        for delta in (1e-4, 1e-2, 1.0, 10.0, 100.0, 300.0):
            for sign in (1, -1):
                zs.append((a + b) / 2 + sign * delta * (a - b) + u)
    z = torch.stack(zs).float()                                         # the fp32 latents both sides see
    d = z.double().pow(2).sum(1, keepdim=True) + E.double().pow(2).sum(1) - 2 * z.double() @ E.double().t()
    ds = d.sort(1).values
    margin = ds[:, 1] - ds[:, 0]
    band = 1e-5 * (z.double().pow(2).sum(1) + float(E.double().pow(2).sum(1).max()))
    q = VectorQuantizer(n, D).cuda()
    q.embedding.weight.data.copy_(E)
    _, _, info = q(z.view(-1, D, 1, 1).cuda())
    idx = info[2].view(-1).cpu()
    diff = idx != d.argmin(1)
    inside = margin < band
    parity_line("codebook near ties: %d of %d latents inside the fp32 band, %d differ from float64 (all inside: %s)"
                % (int(inside.sum()), len(zs), int(diff.sum()), bool(inside[diff].all())))
    assert int(inside.sum()) >= 16 and int((~inside).sum()) >= 16
    assert bool((d.argmin(1).view(8, 12) // 2 == torch.arange(8)[:, None]).all())     # the pair's codes are the two best
    assert bool(inside[diff].all()), "a code outside the near-tie band differs"


def test_decode_gn_bound_past_the_limit_goes_strict_directly():
    """GroupNorm gains x 200 at the full-resolution level: the weight-only operand bound (max|gamma| sqrt(n - 1) + max|beta|)
    exceeds 65504, so every chunk is decoded in the strict mode -- counted once per chunk -- and matches float64 there."""
    sd = dict(_codec_sd("init"))
    for k in [k for k in sd if k.startswith("decoder.up.0.block.") and k.endswith(("norm1.weight", "norm2.weight"))]:
        sd[k] = sd[k] * 200.0
    m = _vqmodel(sd)
    assert m.gn_operand_bound(5, 53) > 65504
    tok = synth.synth_tokens(2, mask_frac=0.0, key="rg.gnb.codes")
    quant = O.codebook_gather(sd, tok, pfx="")
    ref = O.vq_decode({k: v.double() for k, v in sd.items()}, quant.double(), pfx="")
    m.decode_chunk = 1
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        out = _both_modes(m, lambda: m.decode(quant.cuda()))
    assert m.range_fallbacks == 2
    assert torch.equal(out["f16x2"], out["fp32"])          # the same strict computation, not an f16x2 result
    _yardstick("decode GroupNorm gains x200 (strict directly)", out, ref, 1e-3, maxabs)
