// A look-ahead true-peak limiter behind output levelling (include/diffsound_hip.h: ds_limit_*): where a row's gain g0 would lift
// the x4 true peak above the ceiling c, a gain curve g[i] <= 1 takes the signal down around the peaks only.
//
//   e[i] = max(|x[i]|, |y4[4i .. 4i+3]|)               the envelope: the sample and the four x4 outputs of ds_level_true_peak
//   d[i] = max(0, 1 - c / (|g0| e[i]))                 the reduction sample i asks for (fp32; 0 where e = 0 and outside the row)
//   H[i] = max(d[i], a H[i-1])                         its causal decaying maximum (float64, H = 0 before the row)
//   h[i] = max(H[i], max d[i+1 .. i+L])                hold over the look-ahead L, exponential release a
//   s[i] = sum_k w[k] h[i-k], k = 0..L                 smoothing (float64 fma over k ascending, sum w = 1)
//   g[i] = fl32(1 - s[i]),  out[i] = fl32(fl32(g0 g[i]) x[i])
//
// Only H crosses block boundaries, and it composes: a stretch of n samples acts on the state before it as
// H_end = max(a^n H_start, M), M its own decaying maximum from the zero state.  So the row splits as ds_level_segments splits
// the K-weighting: the envelope pass leaves M of every block, one wave per row carries the state over the blocks, and the apply
// pass runs every block again from its true start state.  A block of the apply pass writes samples [k N, (k+1) N) and needs h
// from k N - L on, so the cut of H is shifted by L: envelope block k owns samples [k N - L, (k+1) N - L), and the carried state
// sigma_k = H[k N - L - 1] is exactly what apply block k starts from (sigma_0 = 0: before sample -L nothing has happened).
//
// Every result of a row depends on that row's samples alone; blocks are cut by position in the row and every scan, sum and
// maximum has a fixed order: bit-identical whatever the batch, the row's position in it, the row stride T and the launch.
// Samples at or past len_b are never loaded.
#include <hip/hip_runtime.h>

#include "common.h"
#include "diffsound_hip.h"

#define LM_N 1024                   // samples per workgroup of both passes (256 threads x 4)
#define LM_W 34                     // half width of the x4 filter (audio.resample_taps(fs, 4 fs)), as in loudness.hip
#define LM_NTAP (2 * LM_W + 1)
#define LM_LMAX LM_N                // the shifted cut needs L <= N
#define LM_TRIM_MARGIN 3.0517578125e-05     // 2^-15, see ds_limit_finish_kernel

struct LmLayout {                   // the scratch buffer shared by the ds_limit_* entries
    long long nblk_e;               // envelope blocks per row: ceil((T + L) / N)
    long long nblk_a;               // apply blocks per row: ceil(T / N), at least 1
    long long off_m, off_s, off_d, off_g, bytes;
};

static LmLayout lm_layout(int B, int T, int L) {
    LmLayout l;
    l.nblk_e = ((long long)T + L + LM_N - 1) / LM_N;
    l.nblk_a = ((long long)T + LM_N - 1) / LM_N;
    if (l.nblk_a < 1) l.nblk_a = 1;
    l.off_m = 0;
    l.off_s = l.off_m + (long long)B * l.nblk_e * sizeof(double);
    l.off_d = l.off_s + (long long)B * l.nblk_e * sizeof(double);
    l.off_g = l.off_d + (long long)B * T * sizeof(float);
    l.bytes = l.off_g + (long long)B * l.nblk_a * sizeof(float);
    l.bytes = (l.bytes + 15) / 16 * 16;
    return l;
}

__device__ __forceinline__ int lm_len(const int* lengths, int b, int T) {
    return lengths ? min(max(lengths[b], 0), T) : T;
}

// a^n by squaring, the same products in every thread
__device__ __forceinline__ double lm_pow(double a, int n) {
    double p = 1.0;
    for (; n > 0; n >>= 1) {
        if (n & 1) p *= a;
        a *= a;
    }
    return p;
}

// The decaying maximum across the 256 threads of a block.  Thread t holds m = the state its chunk of c consecutive samples
// ends in when it starts from zero (thread 0: from the carried state), Ac = a^c.  Returns the state thread t's chunk really
// starts from, max over t' < t of Ac^(t-1-t') m_t', and in `total` the state after thread 255.  A shuffle scan in each wave
// (the decay over 2^j chunks is Ac squared j times: uniform), then the four wave totals in order.
__device__ __forceinline__ double lm_block_scan(double m, double Ac, double* sh, double& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double A = Ac, inc = m;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(inc, off);
        if (lane >= off) inc = fmax(A * o, inc);
        A *= A;
    }                                                                    // A = Ac^64: the decay over a wave
    double before = __shfl_up(inc, 1);
    if (lane == 0) before = 0.0;
    __syncthreads();
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    double E = 0.0, tot = 0.0;                                           // the state entering this wave / leaving the block
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        if (v < wave) E = fmax(A * E, sh[v]);
        tot = fmax(A * tot, sh[v]);
    }
    total = tot;
    return fmax(lm_pow(Ac, lane) * E, before);
}

// d of the block's samples and the block's M.  The staging and the sixteen fma chains are ds_level_true_peak_kernel's: a
// thread takes positions tid, tid + 256, .. of the block and all four phases of each.
__global__ __launch_bounds__(256) void ds_limit_envelope_kernel(const float* __restrict__ x, int T, const int* __restrict__ lengths,
                                                               const float* __restrict__ taps, const float* __restrict__ gain,
                                                               float c32, int L, double a, float* __restrict__ d, int nblk_e,
                                                               double* __restrict__ M) {
    __shared__ float xs[LM_N + 2 * LM_W];
    __shared__ __attribute__((aligned(16))) float dl[LM_N];
    __shared__ double sh[4];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int len = lm_len(lengths, b, T);
    const long long i_base = (long long)blockIdx.x * LM_N - L;
    if (i_base >= len || i_base + LM_N <= 0) {                           // nothing of this row here
        if (tid == 0) M[(size_t)b * nblk_e + blockIdx.x] = 0.0;
        return;
    }
    const float* xb = x + (size_t)b * T;
    for (int i = tid; i < LM_N + 2 * LM_W; i += 256) {
        const long long gi = i_base - LM_W + i;
        xs[i] = (gi >= 0 && gi < len) ? xb[gi] : 0.f;
    }
    __syncthreads();
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[r][p] = 0.f;
    const float* xp = xs + tid;                                          // xp[256 r + j] = x[i0 - W + j], i0 = i_base + tid + 256 r
    for (int j = 0; j < LM_NTAP; ++j) {
        const float c0 = taps[j], c1 = taps[LM_NTAP + j], c2 = taps[2 * LM_NTAP + j], c3 = taps[3 * LM_NTAP + j];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float xv = xp[256 * r + j];
            acc[r][0] = fmaf(xv, c0, acc[r][0]);
            acc[r][1] = fmaf(xv, c1, acc[r][1]);
            acc[r][2] = fmaf(xv, c2, acc[r][2]);
            acc[r][3] = fmaf(xv, c3, acc[r][3]);
        }
    }
    const float g0 = fabsf(gain[b]);
    float* db = d + (size_t)b * T;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long i = i_base + tid + 256 * r;
        float dv = 0.f;
        if (i >= 0 && i < len) {
            const float e = fmaxf(fmaxf(fabsf(xp[256 * r + LM_W]), fmaxf(fabsf(acc[r][0]), fabsf(acc[r][1]))),
                                  fmaxf(fabsf(acc[r][2]), fabsf(acc[r][3])));
            const float p = g0 * e;
            if (p > 0.f) dv = fmaxf(0.f, 1.f - c32 / p);
            db[i] = dv;
        }
        dl[tid + 256 * r] = dv;
    }
    __syncthreads();
    const f32x4 mine = *(const f32x4*)(dl + 4 * tid);                    // thread t: samples 4 t .. 4 t + 3 of the block
    double m = (double)mine.x;
    m = fmax(a * m, (double)mine.y);
    m = fmax(a * m, (double)mine.z);
    m = fmax(a * m, (double)mine.w);
    const double a2 = a * a;
    double total;
    lm_block_scan(m, a2 * a2, sh, total);
    if (tid == 0) M[(size_t)b * nblk_e + blockIdx.x] = total;
}

__device__ __forceinline__ double lm_bcast(double v, int k) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, k), hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), k);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// sigma_0 = 0, sigma_{k+1} = max(a^N sigma_k, M_k): one wave per row, as ds_level_carry_kernel walks its segments -- lane l
// holds M of block base + l, every lane runs the recurrence on the broadcast M_k and lane k keeps the state it saw before step k.
__global__ __launch_bounds__(64) void ds_limit_carry_kernel(int T, const int* __restrict__ lengths, double a, int nblk_e,
                                                           const double* __restrict__ M, double* __restrict__ sigma) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int len = lm_len(lengths, b, T);
    const int n_need = min((len + LM_N - 1) / LM_N, nblk_e);             // apply blocks that hold a sample of this row
    const double aN = lm_pow(a, LM_N);
    const double* Mb = M + (size_t)b * nblk_e;
    double* sb = sigma + (size_t)b * nblk_e;
    double s = 0.0;
    for (int base = 0; base < n_need; base += 64) {
        const int j = base + lane;
        const double mj = j < nblk_e ? Mb[j] : 0.0;
        double mine = 0.0;
        for (int k = 0; k < 64; ++k) {
            if (lane == k) mine = s;
            s = fmax(aN * s, lm_bcast(mj, k));
        }
        if (j < n_need) sb[j] = mine;
    }
}

// Samples [k N, (k+1) N) of a row: d over [k N - L, (k+1) N + L) staged, H scanned from the carried state, the hold, the
// smoothing, the gain.  Dynamic LDS: hs f64[N + L] (H, then h), df f32[N + 2 L] (d, then its window maxima, then g).
template <bool VEC>
__global__ __launch_bounds__(256) void ds_limit_apply_kernel(const float* x, int T, const int* __restrict__ lengths,
                                                            const float* __restrict__ gain, int L, double a,
                                                            const double* __restrict__ w, const float* __restrict__ d, int nblk_e,
                                                            const double* __restrict__ sigma, float* out, float* curve,
                                                            int nblk_a, float* __restrict__ gmin) {
    extern __shared__ __attribute__((aligned(16))) double lm_dyn[];
    __shared__ double sh[4];
    __shared__ float red[4];
    const int tid = threadIdx.x, b = blockIdx.y, blk = blockIdx.x;
    const int len = lm_len(lengths, b, T);
    const int s0 = blk * LM_N;
    const int n_h = LM_N + L, n_d = LM_N + 2 * L;
    double* hs = lm_dyn;
    float* df = (float*)(lm_dyn + ((n_h + 1) & ~1));                     // 16-byte aligned: g is read back four at a time
    const float* xb = x + (size_t)b * T;
    float* ob = out + (size_t)b * T;
    float* cb = curve ? curve + (size_t)b * T : nullptr;
    const int i4 = s0 + 4 * tid;                                         // this thread's four outputs
    if (s0 >= len) {                                                     // past the row: zeros, a curve of ones
        if (VEC) {
            if (i4 < T) {
                *(f32x4*)(ob + i4) = f32x4{0.f, 0.f, 0.f, 0.f};
                if (cb) *(f32x4*)(cb + i4) = f32x4{1.f, 1.f, 1.f, 1.f};
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (i4 + q < T) {
                    ob[i4 + q] = 0.f;
                    if (cb) cb[i4 + q] = 1.f;
                }
        }
        if (tid == 0) gmin[(size_t)b * nblk_a + blk] = 1.f;
        return;
    }
    const float* db = d + (size_t)b * T;
    const double sg = sigma[(size_t)b * nblk_e + blk];
    int any = sg != 0.0;
    for (int v = tid; v < n_d; v += 256) {
        const int j = s0 - L + v;
        const float dv = (j >= 0 && j < len) ? db[j] : 0.f;
        df[v] = dv;
        any |= dv != 0.f;
    }
    float g[4] = {1.f, 1.f, 1.f, 1.f};                                   // of samples s0 + tid + 256 r
    if (__syncthreads_or(any)) {                                         // (also the barrier behind the staging)
        // H over [s0 - L, s0 + N): thread t walks c consecutive samples (c odd: the lanes' LDS reads fall on distinct banks)
        const int c = ((n_h + 255) / 256) | 1;
        const int u0 = tid * c;
        double m = tid == 0 ? sg : 0.0;
        for (int q = 0; q < c; ++q)
            if (u0 + q < n_h) m = fmax(a * m, (double)df[u0 + q]);
        double total;
        double st = lm_block_scan(m, lm_pow(a, c), sh, total);
        if (tid == 0) st = sg;
        for (int q = 0; q < c; ++q)
            if (u0 + q < n_h) {
                st = fmax(a * st, (double)df[u0 + q]);
                hs[u0 + q] = st;
            }
        __syncthreads();
        // df[v] <- max d[v .. v + P - 1], P doubling up to the largest power of two <= L (what lies past n_d is never used)
        int P = 1;
        float reg[12];                                                   // n_d <= 3 N = 12 x 256
        for (; 2 * P <= L; P *= 2) {
#pragma unroll
            for (int e = 0; e < 12; ++e) {
                const int v = tid + 256 * e;
                reg[e] = v < n_d ? fmaxf(df[v], v + P < n_d ? df[v + P] : 0.f) : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 12; ++e) {
                const int v = tid + 256 * e;
                if (v < n_d) df[v] = reg[e];
            }
            __syncthreads();
        }
        for (int u = tid; u < n_h; u += 256)                             // h[u] = max(H[u], max d[u + 1 .. u + L])
            hs[u] = fmax(hs[u], (double)fmaxf(df[u + 1], df[u + 1 + L - P]));
        __syncthreads();
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        const double* hp = hs + tid + L;                                 // hp[256 r - k] = h[s0 + tid + 256 r - k]
        for (int k = 0; k <= L; ++k) {
            const double wk = w[k];
#pragma unroll
            for (int r = 0; r < 4; ++r) s[r] = fma(wk, hp[256 * r - k], s[r]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) g[r] = (float)(1.0 - s[r]);
    }
    float* gs = df;                                                      // the four gains of a thread's consecutive outputs
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) gs[tid + 256 * r] = g[r];
    __syncthreads();
    const f32x4 gv = *(const f32x4*)(gs + 4 * tid);
    const float g4[4] = {gv.x, gv.y, gv.z, gv.w};
    const float g0 = gain[b];
    float mn = 1.f;
    if (VEC && i4 + 4 <= len) {
        const f32x4 xv = *(const f32x4*)(xb + i4);
        f32x4 o;
        o.x = (g0 * g4[0]) * xv.x, o.y = (g0 * g4[1]) * xv.y, o.z = (g0 * g4[2]) * xv.z, o.w = (g0 * g4[3]) * xv.w;
        *(f32x4*)(ob + i4) = o;
        if (cb) *(f32x4*)(cb + i4) = gv;
        mn = fminf(fminf(g4[0], g4[1]), fminf(g4[2], g4[3]));
    } else {
        float o[4], cv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool in = i4 + q < len;
            o[q] = in ? (g0 * g4[q]) * xb[i4 + q] : 0.f;
            cv[q] = in ? g4[q] : 1.f;
            mn = fminf(mn, cv[q]);
        }
        if (VEC) {
            if (i4 < T) {
                *(f32x4*)(ob + i4) = f32x4{o[0], o[1], o[2], o[3]};
                if (cb) *(f32x4*)(cb + i4) = f32x4{cv[0], cv[1], cv[2], cv[3]};
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (i4 + q < T) {
                    ob[i4 + q] = o[q];
                    if (cb) cb[i4 + q] = cv[q];
                }
        }
    }
    for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o));
    if ((tid & 63) == 0) red[tid >> 6] = mn;
    __syncthreads();
    if (tid == 0) gmin[(size_t)b * nblk_a + blk] = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
}

// The trim and the report of a row, one wave per row.  tp is the x4 true peak of the limited row as ds_level_gain measured it
// (never below the sample peak).  t = 1 where tp <= c; else t = (c / tp)(1 - 2^-15), rounded to fp32 and one step further down
// where that rounding lifted t tp above c(1 - 2^-15).  The margin is what makes the ceiling hold for the row that is stored, fl32(t out), not only for
// t out: an x4 output of the scaled row is 69 fp32 fmas over samples that were each rounded once more, so it can differ from
// t times the unscaled one by (1 + 2 x 69) 2^-24 sum_j |taps[p][j]| max |out| at the very worst; sum_j |taps[p][j]| < 2.4 for
// every phase and max |out| <= tp, so by less than 2.0e-5 tp < 2^-15 tp.
__global__ __launch_bounds__(64) void ds_limit_finish_kernel(int T, int nblk_a, const float* __restrict__ gmin,
                                                            const double* __restrict__ lufs_in, const float* __restrict__ peaks,
                                                            double ceiling, float* __restrict__ trim, double* __restrict__ lufs,
                                                            float* __restrict__ true_peak, float* __restrict__ max_reduction) {
    const int lane = threadIdx.x, b = blockIdx.x;
    float mn = 1.f;
    for (int j = lane; j < nblk_a; j += 64) mn = fminf(mn, gmin[(size_t)b * nblk_a + j]);
    for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o));
    if (lane != 0) return;
    const double tp = (double)peaks[2 * b + 1];
    float t = 1.f;
    if (tp > ceiling) {
        const double want = ceiling * (1.0 - LM_TRIM_MARGIN);
        t = (float)(want / tp);
        if (!(t > 0.f)) t = 1.f;                                         // tp = inf or NaN: nothing a gain could mend
        else if ((double)t * tp > want) t = __uint_as_float(__float_as_uint(t) - 1u);
    }
    const double p = (double)t * tp;
    float p32 = (float)p;
    if ((double)p32 > p) p32 = __uint_as_float(__float_as_uint(p32) - 1u);       // rounded towards zero: never above t tp
    trim[b] = t;
    lufs[b] = lufs_in[b] + 20.0 * log10((double)t);
    true_peak[b] = p32;
    max_reduction[b] = 1.f - mn;
}

extern "C" int ds_limit_block(void) { return LM_N; }

extern "C" int64_t ds_limit_scratch_bytes(int B, int T, int L) {
    if (B < 1 || T < 0 || L < 1 || L > LM_LMAX) return -1;
    return lm_layout(B, T, L).bytes;
}

#define LM_CHECK_COMMON()                                                                                       \
    DS_CHECK_ARG(B >= 1 && B <= 65535 && T >= 0, "bad sizes");                                                  \
    DS_CHECK_ARG(L >= 1 && L <= LM_LMAX, "the look-ahead L must be in 1 .. ds_limit_block()");                  \
    const LmLayout l = lm_layout(B, T, L);                                                                      \
    DS_CHECK_ARG(scratch_bytes >= l.bytes, "scratch is smaller than ds_limit_scratch_bytes(B, T, L)");          \
    DS_CHECK_ARG(((uintptr_t)scratch & 7) == 0, "scratch must be 8-byte aligned")

extern "C" int ds_limit_envelope(const float* x, int B, int T, const int32_t* lengths, const float* taps, const float* gain,
                                 double ceiling_db, int L, double a, void* scratch, int64_t scratch_bytes, ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(x && taps && gain && scratch, "null pointer");
    LM_CHECK_COMMON();
    DS_CHECK_ARG(ceiling_db == ceiling_db && ceiling_db < INFINITY && ceiling_db > -INFINITY, "ceiling_db must be finite");
    DS_CHECK_ARG(a >= 0.0 && a < 1.0, "the release coefficient a must be in [0, 1)");
    char* sc = (char*)scratch;
    hipLaunchKernelGGL(ds_limit_envelope_kernel, dim3((unsigned)l.nblk_e, B), dim3(256), 0, stream, x, T, lengths, taps, gain,
                       (float)pow(10.0, ceiling_db / 20.0), L, a, (float*)(sc + l.off_d), (int)l.nblk_e, (double*)(sc + l.off_m));
    DS_CHECK_LAUNCH();
    return 0;
}

extern "C" int ds_limit_carry(int B, int T, const int32_t* lengths, int L, double a, void* scratch, int64_t scratch_bytes,
                              ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(scratch, "null pointer");
    LM_CHECK_COMMON();
    DS_CHECK_ARG(a >= 0.0 && a < 1.0, "the release coefficient a must be in [0, 1)");
    char* sc = (char*)scratch;
    hipLaunchKernelGGL(ds_limit_carry_kernel, dim3(B), dim3(64), 0, stream, T, lengths, a, (int)l.nblk_e,
                       (const double*)(sc + l.off_m), (double*)(sc + l.off_s));
    DS_CHECK_LAUNCH();
    return 0;
}

extern "C" int ds_limit_apply(const float* x, int B, int T, const int32_t* lengths, const float* gain, int L, double a,
                              const double* w, float* out, float* curve, void* scratch, int64_t scratch_bytes,
                              ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(x && gain && w && out && scratch, "null pointer");
    LM_CHECK_COMMON();
    DS_CHECK_ARG(a >= 0.0 && a < 1.0, "the release coefficient a must be in [0, 1)");
    if (T == 0) return 0;
    char* sc = (char*)scratch;
    const dim3 grid((unsigned)l.nblk_a, B);
    const size_t lds = (size_t)((LM_N + L + 1) & ~1) * sizeof(double) + (size_t)(LM_N + 2 * L) * sizeof(float);
    const bool vec = T % 4 == 0 && (((uintptr_t)x | (uintptr_t)out | (uintptr_t)curve) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(ds_limit_apply_kernel<true>, grid, dim3(256), lds, stream, x, T, lengths, gain, L, a, w,
                           (const float*)(sc + l.off_d), (int)l.nblk_e, (const double*)(sc + l.off_s), out, curve, (int)l.nblk_a,
                           (float*)(sc + l.off_g));
    else
        hipLaunchKernelGGL(ds_limit_apply_kernel<false>, grid, dim3(256), lds, stream, x, T, lengths, gain, L, a, w,
                           (const float*)(sc + l.off_d), (int)l.nblk_e, (const double*)(sc + l.off_s), out, curve, (int)l.nblk_a,
                           (float*)(sc + l.off_g));
    DS_CHECK_LAUNCH();
    return 0;
}

extern "C" int ds_limit_finish(int B, int T, int L, double ceiling_db, const double* lufs_in, const float* peaks,
                               const void* scratch, int64_t scratch_bytes, float* trim, double* lufs, float* true_peak,
                               float* max_reduction, ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(lufs_in && peaks && scratch && trim && lufs && true_peak && max_reduction, "null pointer");
    LM_CHECK_COMMON();
    DS_CHECK_ARG(ceiling_db == ceiling_db && ceiling_db < INFINITY && ceiling_db > -INFINITY, "ceiling_db must be finite");
    const char* sc = (const char*)scratch;
    hipLaunchKernelGGL(ds_limit_finish_kernel, dim3(B), dim3(64), 0, stream, T, T > 0 ? (int)l.nblk_a : 0, (const float*)(sc + l.off_g),
                       lufs_in, peaks, pow(10.0, ceiling_db / 20.0), trim, lufs, true_peak, max_reduction);
    DS_CHECK_LAUNCH();
    return 0;
}
