"""GEMM backends of the training step (modeling/train.py): the three products of every linear layer -- y = x W^T,
dX = dY W, dW = dY^T X -- behind one surface, `_Fp32Gemm` (exact-fp32 MFMA, the reference arithmetic) and `_SplitGemm` (3-pass
fp16 split on packed planes), plus the `ds_pack_operand` helpers the second one lives on.

The surface: prepare(lin) once per step and weight; prep_x / prep_dy turn an fp32 matrix into the backend's operand handle --
each under a power of two of the caller's (`scale`; prep_x: the forward operand's 2^f, which `fwd` takes out again by itself and
the dW item's 1 / scale must carry as `x handle.unscale`; prep_dy: the site's 2^e, which dx's `unscale` and the dW item take
out) and with max |operand * scale| folded into `amax`; fwd, dx, db launch at once; dw_many(items) takes weight-gradient work [(lin, x handle, dY handle, 1 / scale, dW out)] --
`pairs_dw` says whether the step should collect that work over two blocks first (the split backend groups equal products
into one grid) or hand every product in as it arises.
"""
import math

import torch

from .. import _lib

L_ = _lib


def _ceil(a, b):
    return (a + b - 1) // b * b


def _colsum(x, G=1, R=None, accumulate_into=None):
    """out[g][c] = sum over the R rows of group g (tall inputs: chunked two-stage sum, ds_colsum_ws)"""
    M, C_ = x.shape
    R = M // G if R is None else R
    out = torch.empty(G, C_, device=x.device) if accumulate_into is None else accumulate_into
    if R >= 64:
        work = torch.empty(G * 64 * C_, device=x.device)
        L_.check(L_.lib().ds_colsum_ws(L_.ptr(x), L_.ptr(out), G, R, C_, C_, R * C_, int(accumulate_into is not None),
                                       L_.ptr(work), work.numel(), L_.stream()))
    else:
        L_.check(L_.lib().ds_colsum(L_.ptr(x), L_.ptr(out), G, R, C_, C_, R * C_, int(accumulate_into is not None), L_.stream()))
    return out


PACK_PLAIN, PACK_GELU2, PACK_GELU2_BWD = 0, 1, 2


class _Linear:
    """One (possibly fused) nn.Linear of the step: the weights of its parts (each [N_i][K] fp32; query | key | value of a fused
    projection), bias [N], plus what the GEMM backend derived from them.  `W` (the concatenated fp32 matrix) is only built
    when somebody asks for it -- the "fp32" backend; the "f16x2" backend packs every part straight into its range of the
    fused operand (ds_pack_operand's sub-range form)."""

    def __init__(self, key, W, b):
        self.key = key
        self.parts = [w.detach() for w in W] if isinstance(W, (list, tuple)) else [W.detach()]
        self.b = torch.cat([x.detach() for x in b]) if isinstance(b, (list, tuple)) else b.detach()
        self.N, self.K = sum(w.shape[0] for w in self.parts), self.parts[0].shape[1]
        self._W = self.parts[0] if len(self.parts) == 1 else None
        self.extra = {}

    @property
    def W(self):
        if self._W is None:
            self._W = torch.cat(self.parts)
        return self._W


def _gelu2(x, dy=None):
    out = torch.empty_like(x)
    L_.check(L_.lib().ds_gelu2(L_.ptr(x), L_.ptr(dy), L_.ptr(out), x.numel(), L_.stream()))
    return out


class _Fp32Gemm:
    """Backend "fp32": every GEMM on the exact-fp32 MFMA kernel; transposes and zero padding by torch.  An operand handle is
    the fp32 matrix itself (after the elementwise prologue, if any)."""
    name = "fp32"
    pairs_dw = False

    def prepare(self, lin):
        pass

    def prep_x(self, lin, x, pro=PACK_PLAIN, scale=1.0, amax=None):
        """scale, amax: ignored (nothing is split to fp16 here)"""
        return _gelu2(x) if pro == PACK_GELU2 else x

    def prep_dy(self, lin, dy, pro=PACK_PLAIN, aux=None, amax=None, need_row=True, scale=1.0):
        return _gelu2(aux, dy) if pro == PACK_GELU2_BWD else dy

    def fwd(self, lin, x, R=None):
        M = x.shape[0]
        y = torch.empty(M, lin.N, device=x.device)
        return L_.gemm(x, lin.W, y, M, lin.N, lin.K, bias=lin.b, R=R)

    def dx(self, lin, dy, unscale=1.0):
        M, N, K = dy.shape[0], lin.N, lin.K
        Np = _ceil(N, 32)
        Wt = lin.extra.get("Wt")
        if Wt is None:                                  # [K][Np]: rows are K-contiguous operands of the GEMM
            Wt = torch.zeros(K, Np, device=dy.device)
            Wt[:, :N] = lin.W.t()
            lin.extra["Wt"] = Wt
        dyp = dy if Np == N else torch.nn.functional.pad(dy, (0, Np - N))
        out = torch.empty(M, K, device=dy.device)
        return L_.gemm(dyp.contiguous(), Wt, out, M, K, Np)

    def dw_many(self, items):
        for lin, x, dy, inv_scale, dW in items:
            M = x.shape[0]
            Mp = _ceil(M, 32)

            def pad_t(a):                               # a [M][C] -> a^T zero-padded to [C][Mp]
                out = torch.zeros(a.shape[1], Mp, device=a.device)
                out[:, :M] = a.t()
                return out
            L_.gemm(pad_t(dy), pad_t(x), dW, lin.N, lin.K, Mp)
            if inv_scale != 1.0:
                dW.mul_(inv_scale)

    def db(self, lin, dy):
        return _colsum(dy)[0]


class _Packed:
    """What ds_pack_operand made of one fp32 matrix [rows][cols]: `row` = packed planes of the matrix (int16 [2][plane]),
    `t` = packed planes of its transpose with the contraction index padded to rows_pad, `part` = per-64-row column sums,
    `unscale` = 2^-f of a forward operand whose planes hold x 2^f (prep_x; 1.0 everywhere else)."""
    __slots__ = ("rows", "cols", "row", "row_plane", "t", "t_plane", "rows_pad", "part", "unscale")


def _pack(src, rows, cols, *, scale=1.0, pro=PACK_PLAIN, aux=None, want_row=True, rows_pad=0, colsum=False, amax=None, ld=None):
    """One ds_pack_operand launch (csrc/pack.hip) over src [rows][ld >= cols]."""
    dev = src.device
    o = _Packed()
    o.rows, o.cols, o.rows_pad = rows, cols, rows_pad
    o.row = o.t = o.part = None
    o.unscale = 1.0
    o.row_plane = _ceil(rows, 16) * cols
    o.t_plane = _ceil(cols, 16) * rows_pad
    if want_row:
        o.row = torch.empty(2, o.row_plane, dtype=torch.int16, device=dev)
    if rows_pad:
        o.t = torch.empty(2, o.t_plane, dtype=torch.int16, device=dev)
    if colsum:
        o.part = torch.empty(L_.lib().ds_pack_operand_tile_rows(rows, rows_pad), cols, device=dev)
    L_.check(L_.lib().ds_pack_operand(L_.ptr(src), rows, cols, cols if ld is None else ld, float(scale), int(pro), L_.ptr(aux),
                                      cols, L_.ptr(o.row), o.row_plane, L_.ptr(o.t), o.t_plane, rows_pad, 0, 0, L_.ptr(o.part),
                                      L_.ptr(amax), L_.stream()))
    return o


def _pack_parts(parts, K, scale):
    """The parts [N_i][K] of a fused weight (N = sum N_i, every N_i % 32 == 0) -> ONE _Packed of the fused matrix [N][K]: part i
    goes to the row groups [n0 / 16, ..) of the row form and to the k-range [n0, n0 + N_i) of the transposed form [K][N]."""
    dev = parts[0].device
    N = sum(w.shape[0] for w in parts)
    assert all(w.shape[0] % 32 == 0 and w.shape[1] == K and w.is_contiguous() for w in parts)
    o = _Packed()
    o.rows, o.cols, o.rows_pad, o.part, o.unscale = N, K, N, None, 1.0
    o.row_plane, o.t_plane = N * K, _ceil(K, 16) * N
    o.row = torch.empty(2, o.row_plane, dtype=torch.int16, device=dev)
    o.t = torch.empty(2, o.t_plane, dtype=torch.int16, device=dev)
    n0 = 0
    for w in parts:
        Ni = w.shape[0]
        L_.check(L_.lib().ds_pack_operand(L_.ptr(w), Ni, K, K, float(scale), PACK_PLAIN, None, 0,
                                          L_.ptr_off(o.row, n0 * K), o.row_plane,       # row group n0 / 16: (n0 / 16) * (K / 32) * 512 halves
                                          L_.ptr(o.t), o.t_plane, Ni, n0, N, None, None, L_.stream()))
        n0 += Ni
    return o


class _SplitGemm:
    """Backend "f16x2": every linear-layer GEMM on the 3-pass fp16 split kernel with packed split planes on both operands
    (module docstring).  Operand handles are `_Packed` objects."""
    name = "f16x2"
    pairs_dw = True

    def __init__(self):
        self.wexp = {}              # key -> s: the weight is split as W * 2^s (max |W| 2^s in [2^13, 2^14))
        self.rows_per_sample = 0    # token rows per sample of the activations (set by the step; 0: unknown)

    @staticmethod
    def scales_of(lins):
        """{key: s} with s = 13 - floor(log2 max|W|) for every matrix; one host sync for all of them"""
        mx = torch.stack([torch.stack([w.abs().max() for w in l.parts]).max() for l in lins]).tolist()
        return {l.key: 0 if (m == 0.0 or not math.isfinite(m)) else 13 - math.floor(math.log2(m)) for l, m in zip(lins, mx)}

    def refresh_scales(self, lins):
        self.wexp.update(self.scales_of(lins))

    @staticmethod
    def split_k(N, K, M=4096):
        """K-ranges of a dW = dY^T X launch over M rows, from the measured sweep of the packed kernel INCLUDING the fixed-order
        reduction of the partial results (tools/train_gemm_ab.py -> profiles/r05g_train_gemm_packed_sweep.txt, M = 5300 / 1540):
        >= 256 tiles of 128 x 128 (fc1 / fc2: half a round of the chip) run unsplit -- the partials' write + re-read costs more
        than the idle slots (133 vs 148 us); so does 3072 x 1024 since round 6 (256 tiles of 96 x 128, one per CU: 111 us against
        118 in 4 ranges, profiles/r06x_train_gemm_tile_sweep.txt); smaller products take 4 ranges (1024 x 1024: 48 us against 52
        at 8, 83 unsplit), 2 when the contraction itself is short (the caption rows: 22 us against 31 at 8)."""
        tiles = ((N + 127) // 128) * ((K + 127) // 128)
        if tiles >= 192:
            return 1
        return 4 if M >= 4096 else 2

    def rows_pad(self, lin, M):
        """the padded contraction length of this layer's dW = dY^T X over M rows: a multiple of 32 per K-range"""
        return _ceil(M, 32 * self.split_k(lin.N, lin.K, M))

    def prepare(self, lin):
        """W * 2^s -> row form [N][K] (forward) and transposed form [K][ceil32(N)] (dX), one pass"""
        s = self.wexp[lin.key]
        lin.extra["osc"] = 2.0 ** (-s)
        if len(lin.parts) > 1 or lin.N % 32 == 0:
            lin.extra["Wp"] = _pack_parts(lin.parts, lin.K, 2.0 ** s)
        else:
            lin.extra["Wp"] = _pack(lin.W, lin.N, lin.K, scale=2.0 ** s, rows_pad=_ceil(lin.N, 32))

    def prep_x(self, lin, x, pro=PACK_PLAIN, scale=1.0, amax=None):
        """scale: the forward operand's own power of two 2^f (LossScalePolicy.fwd_exp; applied after the prologue): the planes
        hold x * scale, the handle remembers 1 / scale for `fwd` and for the dW item; `amax` takes max |x * scale|"""
        M = x.shape[0]
        o = _pack(x, M, lin.K, scale=scale, pro=pro, rows_pad=self.rows_pad(lin, M), amax=amax)
        o.unscale = 1.0 / scale
        return o

    def prep_dy(self, lin, dy, pro=PACK_PLAIN, aux=None, amax=None, need_row=True, scale=1.0):
        """scale: the site's own power of two (LossScalePolicy._site_exp): the planes hold dY * scale, the column sums (bias
        gradient) are those of dY itself, `amax` takes max |dY * scale|"""
        M = dy.shape[0]
        return _pack(dy, M, lin.N, scale=scale, pro=pro, aux=aux, want_row=need_row, rows_pad=self.rows_pad(lin, M), colsum=True,
                     amax=amax)

    def fwd(self, lin, xp, R=None):
        M = xp.rows
        y = torch.empty(M, lin.N, device=xp.row.device)
        Wp = lin.extra["Wp"]
        # (rows_per_sample: lets the dispatcher take the sampling loop's per-sample 272 x 256 program where its grid pays --
        #  the 20 x 12 tiles of the QKV projection, 91 us against 101; same bits, tests/test_hip_widening.py)
        return L_.gemm(xp.row, Wp.row, y, M, lin.N, lin.K, bias=lin.b, R=R, split2=lin.extra["osc"] * xp.unscale, a_plane=xp.row_plane,
                       w_plane=Wp.row_plane, rows_per_sample=self.rows_per_sample if M % max(1, self.rows_per_sample) == 0 else 0)

    def dx(self, lin, dyp, unscale=1.0):
        """unscale: 2^-e of the site's own scale, folded into the epilogue's output scale (exact: powers of two)"""
        M = dyp.rows
        Wp = lin.extra["Wp"]
        out = torch.empty(M, lin.K, device=dyp.row.device)
        Np = Wp.rows_pad                                       # contraction length of dX = dY W (N, a multiple of 32 here)
        assert Np == lin.N, "dX needs N % 32 == 0 (true for every linear of this network)"
        return L_.gemm(dyp.row, Wp.t, out, M, lin.K, Np, split2=lin.extra["osc"] * unscale, a_plane=dyp.row_plane,
                       w_plane=Wp.t_plane, rows_per_sample=self.rows_per_sample if M % max(1, self.rows_per_sample) == 0 else 0)

    def _dw(self, item, S, desc_only=False):
        """One dW = dY^T X on the packed planes, straight into dW (S = 1) or as S K-ranges into partial results.  -> (what
        L_.gemm returned: the descriptor when desc_only, `finish`): finish() adds the partial results in a fixed order."""
        lin, xp, dyp, inv_scale, dW = item
        N, K, Mp = lin.N, lin.K, dyp.rows_pad
        assert xp.rows_pad == Mp and xp.cols == K and dyp.cols == N
        if S == 1:
            return L_.gemm(dyp.t, xp.t, dW, N, K, Mp, split2=inv_scale, a_plane=dyp.t_plane, w_plane=xp.t_plane,
                           desc_only=desc_only), None
        part = torch.empty(S, N * K, device=dW.device)
        Kc = Mp // S
        d = L_.gemm(dyp.t, xp.t, part, N, K, Kc, lda=Mp, ldw=Mp, ldc=K, groups=S, a_gstride=Kc * 16, w_gstride=Kc * 16,
                    c_gstride=N * K, split2=inv_scale, a_plane=dyp.t_plane, w_plane=xp.t_plane, desc_only=desc_only)
        return d, lambda: L_.check(L_.lib().ds_colsum(L_.ptr(part), L_.ptr(dW), 1, S, N * K, N * K, 0, 0, L_.stream()))

    def dw_many(self, items):
        """items: [(lin, xp, dyp, inv_scale, dW)] -- the weight gradients of several layers whose operands are all packed, into
        the pre-allocated dW tensors.  Every dW launch is sized to about one workgroup per CU, and a workgroup alone on a CU
        runs its tile in ~0.6 of the time two co-resident ones take: products of equal tile configuration and K-range count go
        out as ONE grid (ds_gemm_f16x2_multi, up to four), the same bits as one launch each."""
        groups = {}
        for it in items:
            lin, dyp = it[0], it[2]
            S = self.split_k(lin.N, lin.K, dyp.rows)
            cfg = L_.lib().ds_gemm_f16x2_auto_tile(lin.N, lin.K, S)
            groups.setdefault((cfg, S), []).append(it)
        for (cfg, S), its in groups.items():
            for c0 in range(0, len(its), 4):
                chunk = its[c0:c0 + 4]
                if cfg == 2 or len(chunk) == 1:                # one launch each, every one finished before the next
                    for it in chunk:
                        finish = self._dw(it, S)[1]
                        if finish is not None:
                            finish()
                    continue
                made = [self._dw(it, S, desc_only=True) for it in chunk]
                L_.gemm_multi([d for d, _ in made], cfg)
                for _, finish in made:
                    if finish is not None:
                        finish()

    def db(self, lin, dyp):
        out = torch.empty(1, dyp.cols, device=dyp.part.device)
        R = (dyp.rows + 63) // 64                              # tile rows that hold data (the rest pad the contraction)
        L_.check(L_.lib().ds_colsum(L_.ptr(dyp.part), L_.ptr(out), 1, R, dyp.cols, dyp.cols, 0, 0, L_.stream()))
        return out[0]

