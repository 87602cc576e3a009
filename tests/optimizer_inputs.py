"""The input families of the optimizer tail's tests (tests/test_hip_optimizer_range.py runs the kernels on them,
tests/test_optimizer_host.py asserts their fairness without a GPU) with both yardsticks of tests/optimizer_reference.py on each.
Everything is seeded torch on the CPU; nothing here touches the package or a GPU."""
import collections
import functools

import torch

import optimizer_reference as R

SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193]     # around the 16-byte group, the 1024-element sweep, the 4096 chunk
DECADES = [1e-12, 1e-10, 1e-8, 1e-6, 1e-3, 1.0, 1e3, 1e6]                 # |g * grad_scale|: around and far from eps = 1e-8
EPS = 1e-8
BETAS = [(0.9, 0.96), (0.9, 0.999)]


def gen(key):
    return torch.Generator().manual_seed(sum((i + 1) * b for i, b in enumerate(key.encode())) % (2 ** 31))


def unit(shape, key):
    """+-[0.5, 1): one magnitude per tensor, both signs"""
    g = gen(key)
    mag = 0.5 + 0.5 * torch.rand(shape, generator=g)
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).float()


def split(flat, sizes):
    return list(torch.split(flat, sizes))


def per_tensor(got, y64, y32, sizes):
    """[(err, d32, ulp)] per tensor of a flat comparison: err = max |got - f64|, d32 = max |f32 - f64|, ulp = one float32 ulp of
    the tensor's largest |yardstick value|"""
    out = []
    for g_, a, b in zip(split(got.double(), sizes), split(y64, sizes), split(y32.double(), sizes)):
        out.append((float((g_ - a).abs().max()), float((b - a).abs().max()), R.ulp32(float(a.abs().max()))))
    return out


# ---- (a) AdamW across gradient scale -------------------------------------------------------------------------------------
# one launch = ten tensors: the eight decades of |g grad_scale|, g = 0 from the zero state, g = 0 on a non-zero state.  Sizes
# of at least 64 elements (a tensor's d32 is a maximum over its elements: it is representative only over enough of them), odd
# ones, and one above the 4096 chunk.
A_SIZES = [4097, 257, 129, 1023, 64, 1025, 515, 300, 2049, 1000]
A_STEPS = (1, 2, 50, 400)
A_N = sum(A_SIZES)
A_ZERO, A_ZERO_STATE = 8, 9                      # tensor indices of the two g = 0 tensors
AdamCase = collections.namedtuple("AdamCase", "p_kind gs lr wd betas")
# every (p, lr, betas) combination; grad_scale and weight decay cycle against them so that each value meets each p kind, both
# learning rates and both beta pairs (12 cases instead of the 72 of the full product: the factors act on separate terms of the
# update -- grad_scale on g, wd on the decay factor, lr on both -- and the product below pairs each with every other twice)
A_CASES = [AdamCase(p, [1.0, 0.37, 2.0 ** -12][(i + j + 2 * k) % 3], lr, [0.0, 4.5e-2][(i + j + k) % 2], b)
           for i, p in enumerate(("zero", "milli", "one")) for j, lr in enumerate((3e-3, 3e-6)) for k, b in enumerate(BETAS)]
A_IDS = ["p-%s,gs%.3g,lr%g,wd%g,b2-%g" % (c.p_kind, c.gs, c.lr, c.wd, c.betas[1]) for c in A_CASES]


@functools.lru_cache(None)
def a_units():
    return unit((A_STEPS[-1], A_N), "adam.units")


@functools.lru_cache(None)
def adam_case(idx):
    """-> dict: g [400, N] float32 (what ds_adamw_dev / _multi receive), gpre = g * gs in float32 (what ds_adamw receives), p0, m0,
    v0 float32 [N], hyper [400][4], and snap[form][step] = (p64, m64, v64, p32, m32, v32) for form in ("hyper", "step")."""
    c = A_CASES[idx]
    gs = R.f32(c.gs)
    scale = torch.cat([torch.full((n,), (DECADES[j] / gs) if j < len(DECADES) else 0.0, dtype=torch.float64)
                       for j, n in enumerate(A_SIZES)])
    g = (a_units().double() * scale).float()
    gpre = g * gs                                                            # one float32 product, as the kernel's g * hyper[3]
    p0 = {"zero": torch.zeros(A_N), "milli": 1e-3 * unit((A_N,), "adam.p"), "one": unit((A_N,), "adam.p")}[c.p_kind]
    m0, v0 = torch.zeros(A_N), torch.zeros(A_N)
    o = sum(A_SIZES[:A_ZERO_STATE])
    m0[o:] = 1e-3 * unit((A_SIZES[A_ZERO_STATE],), "adam.m0")
    v0[o:] = 1e-6 * unit((A_SIZES[A_ZERO_STATE],), "adam.v0").abs()
    b1, b2, lr, wd, eps = R.f32(c.betas[0]), R.f32(c.betas[1]), R.f32(c.lr), R.f32(c.wd), R.f32(EPS)
    hyper = [R.hyper_values(c.lr, c.betas[0], c.betas[1], s, c.gs) for s in range(1, A_STEPS[-1] + 1)]
    snap = {}
    for form in ("hyper", "step"):
        st = [t.to(dt).clone() for dt in (torch.float64, torch.float32) for t in (p0, m0, v0)]
        snap[form] = {}
        for s in range(1, A_STEPS[-1] + 1):
            if form == "hyper":
                bc1, bc2s, gin, scale_ = hyper[s - 1][1], hyper[s - 1][2], g[s - 1], gs
            else:
                (bc1, bc2s), gin, scale_ = R.bias_corrections(c.betas[0], c.betas[1], s), gpre[s - 1], 1.0
            R.adamw_step(st[0], gin.double(), st[1], st[2], lr, b1, b2, eps, wd, bc1, bc2s, scale_)
            R.adamw_step(st[3], gin, st[4], st[5], lr, b1, b2, eps, wd, bc1, bc2s, scale_)
            if s in A_STEPS:
                snap[form][s] = tuple(t.clone() for t in st)
    return dict(c=c, g=g, gpre=gpre, p0=p0, m0=m0, v0=v0, hyper=hyper, snap=snap)


# ---- (b) ds_adamw's own bias corrections ------------------------------------------------------------------------------------
B_STEPS = (1, 2, 3, 10, 1000, 10 ** 6)
B_N = 1025
B_LR, B_WD = 3e-3, 4.5e-2


@functools.lru_cache(None)
def bias_case(betas, step):
    """one ds_adamw(step) call from a given non-zero state, p = 0 (the new p is the update itself)"""
    g, m0, v0 = 1e-3 * unit((B_N,), "bias.g"), 1e-3 * unit((B_N,), "bias.m"), 1e-6 * unit((B_N,), "bias.v").abs()
    bc1, bc2s = R.bias_corrections(betas[0], betas[1], step)
    out = []
    for dt in (torch.float64, torch.float32):
        p, m, v = torch.zeros(B_N, dtype=dt), m0.to(dt).clone(), v0.to(dt).clone()
        R.adamw_step(p, g.to(dt), m, v, R.f32(B_LR), R.f32(betas[0]), R.f32(betas[1]), R.f32(EPS), R.f32(B_WD), bc1, bc2s)
        out += [p, m, v]
    return dict(g=g, m0=m0, v0=v0, y=tuple(out))


# ---- (c) tables of tensors in guarded arenas --------------------------------------------------------------------------------
GUARD = -12345.5                                   # every element of an arena that belongs to no tensor holds this bit pattern


def table_sizes(count, ones=False):
    return [1] * count if ones else [SIZES[i % len(SIZES)] for i in range(count)]


def misaligned_role(i, roles):
    """which of `roles` arrays of tensor i starts 4 bytes past a 16-byte boundary (0: none).  Over any 12 * (roles + 1)
    consecutive tensors every size meets every choice."""
    return (i + i // len(SIZES)) % (roles + 1)


def arena_layout(sizes, shifted):
    """element offsets of the tensors in an arena: each starts at a 16-byte boundary (+ 1 element where shifted[i]) with at
    least 4 guard elements before and after it.  -> (offsets, arena length)"""
    offs, cur = [], 0
    for n, sh in zip(sizes, shifted):
        cur = (cur + 3) // 4 * 4 + 4
        offs.append(cur + (1 if sh else 0))
        cur = offs[-1] + n
    return offs, (cur + 3) // 4 * 4 + 8


def arena(flat, sizes, shifted):
    """-> (arena tensor float32 on the CPU, offsets): `flat`'s tensors laid out with guards between them"""
    offs, total = arena_layout(sizes, shifted)
    a = torch.full((total,), GUARD)
    for t, o in zip(split(flat, sizes), offs):
        a[o:o + t.numel()] = t
    return a, offs


def gather(a, sizes, offs):
    return torch.cat([a[o:o + n] for n, o in zip(sizes, offs)])


def guards_intact(a, sizes, offs):
    mask = torch.ones(a.numel(), dtype=torch.bool)
    for n, o in zip(sizes, offs):
        mask[o:o + n] = False
    return bool((a[mask].view(torch.int32) == torch.tensor(GUARD).view(torch.int32)).all())


C_ADAM_COUNTS, C_EMA_COUNTS, C_NORM_COUNTS = (63, 64, 65, 129), (95, 96, 97), (127, 128, 129)
C_STEP, C_GS, C_LR, C_WD, C_BETAS = 3, 0.37, 3e-3, 4.5e-2, (0.9, 0.96)


@functools.lru_cache(None)
def table_adam_case(count, ones):
    """One update of a whole table from a non-zero state (p ~ 1, |m| ~ 1e-2, v ~ 1e-4, |g gs| ~ 1e-6 .. 1e-3: the state dominates
    the increment -- no cancellation between 0.9 m and 0.1 g -- so every element's result is one or two roundings from the
    float64 value whatever its tensor's size: a 1-element tensor has no other elements to make its d32 representative)."""
    sizes = table_sizes(count, ones)
    N = sum(sizes)
    key = "tab.%d.%d" % (count, ones)
    dec = torch.cat([torch.full((n,), 10.0 ** -(3 + i % 4)) for i, n in enumerate(sizes)])
    g = (unit((N,), key + "g") * dec / R.f32(C_GS)).float()
    p0, m0, v0 = unit((N,), key + "p"), 1e-2 * unit((N,), key + "m"), 1e-4 * unit((N,), key + "v").abs()
    hyper = R.hyper_values(C_LR, C_BETAS[0], C_BETAS[1], C_STEP, C_GS)
    out = []
    for dt in (torch.float64, torch.float32):
        p, m, v = (t.to(dt).clone() for t in (p0, m0, v0))
        R.adamw_step(p, g.to(dt), m, v, R.f32(C_LR), R.f32(C_BETAS[0]), R.f32(C_BETAS[1]), R.f32(EPS), R.f32(C_WD), hyper[1], hyper[2],
                     hyper[3])
        out += [p, m, v]
    return dict(sizes=sizes, g=g, p0=p0, m0=m0, v0=v0, hyper=hyper, y=tuple(out))


@functools.lru_cache(None)
def table_ema_case(count, ones, decay=0.99):
    sizes = table_sizes(count, ones)
    N = sum(sizes)
    key = "tabe.%d.%d" % (count, ones)
    e0, cur = unit((N,), key + "e"), unit((N,), key + "c")
    d, w = R.f32(decay), R.f32(1 - decay)
    out = []
    for dt in (torch.float64, torch.float32):
        e = e0.to(dt).clone()
        R.ema_step(e, cur.to(dt), d, w)
        out.append(e)
    return dict(sizes=sizes, e0=e0, cur=cur, decay=d, w=w, y=tuple(out))


# ---- (d), (e) the gradient norm across scale -----------------------------------------------------------------------------------
# The domain of ds_grad_norm_multi: a thread adds 16 squares in float32 before the double sums, so 2^-63 <= |g| (g^2 is a normal
# float32) and |g| < 2^62 (16 g^2 < 2^128), zeros aside.
NORM_LO, NORM_HI = 2.0 ** -63, 2.0 ** 62
NormCase = collections.namedtuple("NormCase", "ts n64 n32")


def _norm_case(ts, rescale=0):
    """rescale: the float32 restatement runs on the tensors times 2^-rescale and its result is scaled back (exact: the norm is
    homogeneous and powers of two move no mantissa) -- torch's float32 path adds ALL of a tensor's squares in float32 and
    overflows long before the kernel's 16 do, so at the domain's ends it is taken on the same mantissas at a harmless exponent"""
    n32 = R.grad_norm([t * 2.0 ** -rescale for t in ts], torch.float32) * 2.0 ** rescale
    return NormCase(ts, R.grad_norm(ts), n32)


@functools.lru_cache(None)
def norm_case(name):
    sizes = table_sizes(40)
    N = sum(sizes)
    if name.startswith("2^"):
        flat = unit((N,), "norm." + name) * 2.0 ** int(name[2:])
    elif name == "mixed":                                                       # most tensors at 1e-6, one at 1e3
        flat = unit((N,), "norm.mixed") * torch.cat([torch.full((n,), 1e3 if i == 17 else 1e-6) for i, n in enumerate(sizes)])
    elif name == "spike":                                                       # one 1e4 among 1e-4 values
        sizes = [8193]
        flat = unit((8193,), "norm.spike") * 1e-4
        flat[4711] = 1e4
    elif name == "lo-edge":                                                     # the documented domain's ends themselves
        flat = unit((N,), "norm.lo") * 2.0 * NORM_LO                            # |g| in [2^-63, 2^-62)
    elif name == "hi-edge":
        flat = unit((N,), "norm.hi") * NORM_HI                                  # |g| in [2^61, 2^62)
    return _norm_case(split(flat.float(), sizes), {"lo-edge": -62, "hi-edge": 62}.get(name, 0))


NORM_SCALES = ["2^-40", "2^-20", "2^0", "2^20", "2^40", "mixed", "spike", "lo-edge", "hi-edge"]


@functools.lru_cache(None)
def norm_table_case(count, ones):
    sizes = table_sizes(count, ones)
    flat = unit((sum(sizes),), "normt.%d.%d" % (count, ones)) * torch.cat([torch.full((n,), 10.0 ** -(i % 4)) for i, n in enumerate(sizes)])
    return _norm_case(split(flat.float(), sizes))


def max_norms(n64):
    """the four clip thresholds of a case: clipping, far from clipping, none, and one within 1e-6 relative of the norm"""
    return (0.5, 1e9, 0.0, R.f32(n64 * (1 + 5e-7)))              # (float32 values: what the entry's `float max_norm` receives)


def norm_bound(c):
    return 4 * abs(c.n32 - c.n64) + R.ulp32(c.n64)


def coef_bound(c, max_norm):
    """The coefficient follows from the yardstick's norm to the norm's own relative bound, (4 d32 + ulp) / norm, and nothing more;
    min(1, .) does not stretch a distance."""
    want = R.clip_coef(c.n64, max_norm)
    return want, norm_bound(c) / c.n64 * want


# ---- (g) EMA drift ---------------------------------------------------------------------------------------------------------------
G_SIZES, G_UPDATES = [4097, 1025, 300], 300


@functools.lru_cache(None)
def ema_drift_case(decay):
    """300 updates towards a `current` that moves by a small random walk -> cur [300, N] float32, e0, and the two yardsticks"""
    N = sum(G_SIZES)
    walk = torch.randn((G_UPDATES, N), generator=gen("ema.walk")) * 1e-3
    cur = (unit((N,), "ema.c0")[None] + walk.cumsum(0)).float()
    e0 = unit((N,), "ema.e0")
    d, w = R.f32(decay), R.f32(1 - decay)
    out = []
    for dt in (torch.float64, torch.float32):
        e = e0.to(dt).clone()
        for s in range(G_UPDATES):
            R.ema_step(e, cur[s].to(dt), d, w)
        out.append(e)
    return dict(cur=cur, e0=e0, decay=d, w=w, y=tuple(out))


# ---- (h) the pieces together -------------------------------------------------------------------------------------------------------
H_COUNT, H_ITERS, H_MAX_NORM, H_LR, H_WD, H_BETAS = 150, 20, 0.5, 3e-3, 4.5e-2, (0.9, 0.96)
# The toy model takes the list's sizes from 1023 elements up.  Over 20 iterations an element's distance from float64 is a random
# walk of roundings, and two float32 evaluations that round at different places (torch's op-by-op expression, a kernel's fused
# multiply-adds) walk independently: a tensor's d32 -- a maximum over its elements -- bounds another such walk only over enough
# elements.  The reason rests on a CPU emulation, not on a kernel: with the sizes 1 .. 5 in the model the float32 emulation of
# tests/test_optimizer_host.py itself misses the per-tensor bound (m of a 1-element tensor: 1.4 x the bound).  Those sizes are held one update at a time by the tables of (c).
H_SIZES = [n for n in SIZES if n >= 1023]


@functools.lru_cache(None)
def chain_case():
    """20 iterations of norm -> clip coefficient -> AdamW on a toy model of 150 tensors; the gradients' norm alternates between
    about 2 max_norm (clips) and about max_norm / 2 (does not).  float64: clip_grad_norm_'s formulas + AdamW in double; float32:
    torch's float32 path (_foreach_norm, the coefficient as a float32 tensor op, AdamW in float32)."""
    sizes = [H_SIZES[i % len(H_SIZES)] for i in range(H_COUNT)]
    N = sum(sizes)
    u = unit((H_ITERS, N), "chain.g")
    target = torch.tensor([H_MAX_NORM * (2.0 if s % 2 == 0 else 0.5) * (1 + 0.03 * s) for s in range(H_ITERS)], dtype=torch.float64)
    g = (u.double() * (target / u.double().norm(dim=1))[:, None]).float()
    p0 = unit((N,), "chain.p")
    b1, b2, lr, wd, eps = R.f32(H_BETAS[0]), R.f32(H_BETAS[1]), R.f32(H_LR), R.f32(H_WD), R.f32(EPS)
    st = [t.to(dt).clone() for dt in (torch.float64, torch.float32) for t in (p0, torch.zeros(N), torch.zeros(N))]
    hyper, norms, coefs = [], [], []
    for s in range(H_ITERS):
        h = R.hyper_values(H_LR, H_BETAS[0], H_BETAS[1], s + 1)
        ts = split(g[s], sizes)
        n64, n32 = R.grad_norm(ts), R.grad_norm(ts, torch.float32)
        c64 = R.clip_coef(n64, H_MAX_NORM)
        c32 = float(torch.clamp(torch.tensor(H_MAX_NORM) / (torch.tensor(n32) + 1e-6), max=1.0))
        R.adamw_step(st[0], g[s].double(), st[1], st[2], lr, b1, b2, eps, wd, h[1], h[2], c64)
        R.adamw_step(st[3], g[s], st[4], st[5], lr, b1, b2, eps, wd, h[1], h[2], c32)
        hyper.append(h)
        norms.append(n64)
        coefs.append(c64)
    return dict(sizes=sizes, g=g, p0=p0, hyper=hyper, norms=norms, coefs=coefs, y=tuple(st))


# ---- (f) ds_amax -----------------------------------------------------------------------------------------------------------------------
AMAX_SIZES = [1, 2, 3, 4, 5, 7, 4096, 4097]
AMAX_BIG = 2097152 + 7                  # above 512 workgroups x 4096 elements: the grid-stride loop's second round, with a 3-element tail


def amax_positions(n):
    """first, last, last of the 16-byte body, first of the tail (those that exist and differ)"""
    n4 = n // 4
    return sorted({0, n - 1} | ({4 * n4 - 1} if n4 else set()) | ({4 * n4} if 4 * n4 < n else set()))


@functools.lru_cache(None)
def amax_base(n):
    return (2 * torch.rand((n,), generator=gen("amax.%d" % n)) - 1).float()          # |x| < 1
