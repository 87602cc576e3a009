"""The yardstick of the optimizer tail's tests (global gradient norm, clip coefficient, AdamW, EMA, max |x|): every formula
written once with torch on the CPU, parametrised by dtype -- float64 is the reference value, float32 the arithmetic class a
kernel is allowed; the distance between the two on an input is its d32.  Never imports the package.

What the formulas take as inputs are the numbers the C entry points really RECEIVE: the API's contract is `float beta1, beta2,
eps, weight_decay` (and `float lr` for ds_adamw), so beta, eps, lr, weight decay and grad_scale enter as their float32
roundings (f32() below), and for the `hyper` forms (ds_adamw_dev, ds_adamw_multi) the bias corrections are the float32
values stored in hyper[1], hyper[2] -- the yardstick does not second-guess how the caller formed them.  For ds_adamw(step)
the yardstick forms 1 - beta^step in double from the float32 beta.  (1.f - beta is exact in float32 for beta in [0.5, 1), so
the kernels' `1.f - b1` is the double 1 - beta of the same float32 beta.)

AdamW is torch.optim.AdamW's single-tensor path expression for expression: the Python scalars are formed in double and
rounded once where they meet a tensor, as torch does:
    p.mul_(1 - lr wd);  m.lerp_(g, 1 - beta1);  v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    p.addcdiv_(m, sqrt(v) / sqrt(bc2) + eps, value=-(lr / bc1))"""
import math

import numpy as np
import torch


def f32(x):
    """the float32 rounding of a Python number, as a Python float (what a C `float` argument or a float32 tensor entry holds)"""
    return float(np.float32(x))


def hyper_values(lr, beta1, beta2, step, grad_scale=1.0):
    """the four float32 values GraphedIteration stores in `hyper` for this step (modeling/train.py: the bias corrections formed
    in double from the Python betas, then stored as float32)"""
    return [f32(lr), f32(1.0 - beta1 ** step), f32(math.sqrt(1.0 - beta2 ** step)), f32(grad_scale)]


def bias_corrections(beta1, beta2, step):
    """(1 - beta1^step, sqrt(1 - beta2^step)) in double from the float32 betas: ds_adamw(step)'s yardstick"""
    return 1.0 - f32(beta1) ** step, math.sqrt(1.0 - f32(beta2) ** step)


def adamw_step(p, g, m, v, lr, beta1, beta2, eps, wd, bc1, bc2s, grad_scale=1.0):
    """One update IN PLACE on p, m, v (tensors of one dtype: float64 or float32).  lr, beta1, beta2, eps, wd, grad_scale: the
    float32 values the entry receives (as Python floats); bc1 = 1 - beta1^step, bc2s = sqrt(1 - beta2^step) as the entry holds
    them (hyper forms: the float32 values of hyper; ds_adamw: bias_corrections())."""
    g = g * grad_scale
    p.mul_(1 - lr * wd)
    m.lerp_(g, 1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    denom = (v.sqrt() / bc2s).add_(eps)
    p.addcdiv_(m, denom, value=-(lr / bc1))


def grad_norm(ts, dtype=torch.float64):
    """the global L2 norm of a list of tensors.  float64: sqrt(sum g^2); float32: torch's clip_grad_norm_ path, _foreach_norm ->
    stack -> vector_norm on the float32 tensors.  Returns a Python float."""
    if dtype == torch.float64:
        return math.sqrt(sum(float(t.double().pow(2).sum()) for t in ts))
    ts = [t.float() for t in ts]
    return float(torch.linalg.vector_norm(torch.stack(torch._foreach_norm(ts))))


def clip_coef(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)); 1 when max_norm <= 0 (no clipping asked for)"""
    if max_norm <= 0:
        return 1.0
    return min(1.0, max_norm / (norm + 1e-6))


def ema_step(ema, cur, decay, w):
    """ema * decay + cur * w IN PLACE on ema (w: the float32 the entry receives for 1 - decay): two products and a sum"""
    ema.mul_(decay).add_(cur * w)


def amax(x, start=0.0):
    """max(start, max |x| over the entries that are not NaN) as a Python float"""
    a = x.abs()
    a = a[~torch.isnan(a)]
    return max(float(start), float(a.max())) if a.numel() else float(start)


def ulp32(x):
    """the float32 spacing at |x| (a Python float; the smallest subnormal at 0)"""
    a = np.float32(abs(x))
    return float(np.nextafter(a, np.float32(np.inf)) - a)
