// Output levelling on the device: ITU-R BS.1770 K-weighted gated loudness, sample peak, mean square and x4 true peak of a
// batch of mono clips, the gain a strategy asks for, and the gain itself (include/diffsound_hip.h: ds_level_*).
//
// K-weighting is two biquads in series; both run in the transposed direct form II in float64, so a row's filter is the linear
// system  s' = A s + B x,  y = C s + D x  on the 4-vector s = (s1, s2, t1, t2):
//     y1 = b0 x + s1;   s1' = b1 x - a1 y1 + s2;   s2' = b2 x - a2 y1          (shelf)
//     y2 =    y1 + t1;  t1' = -2 y1 - c1 y2 + t2;  t2' =    y1 - c2 y2          (high-pass, b = [1, -2, 1])
// The recurrence is never walked along a whole clip.  The cut is the 100-ms segment of S samples (ds_level_segments):
//   1. every segment is run from the zero state and leaves its end state e_j                        (one lane per segment)
//   2. the true start states follow from the segment transition P = A^S (float64, from the host):
//          sigma_0 = 0,  sigma_{j+1} = P sigma_j + e_j              (one wave per row, n_seg register-only steps of 16 fma)
//   3. every segment is run again from sigma_j and sums y2^2 in sample order -> seg[b][j]; the same pass takes max |x| and
//      sum x^2 of the segment (and of the partial segment that trails the row, which has no energy of its own).
// A workgroup is ONE wave that owns 64 consecutive segments of a row.  Lane-per-segment reads are S floats apart, so the
// wave stages 64 samples of each of its 64 segments through LDS: per segment one coalesced 256-byte read (4 bytes a lane:
// S is odd at 22 050 Hz and the row stride is the caller's, so segment starts have no 16-byte alignment to build wider reads
// on), written to a [64][65] tile whose rows the lanes then read without a bank conflict.  The reads of the next 64 samples
// are issued before the current 64 are filtered, so what bounds the kernel is the float64 work of a sample (a dozen
// dependent operations issued by one wave), not memory: 2 passes x S steps per lane, whatever the clip length.
//
// Every result of a row depends on that row's samples alone and is produced by a fixed order of operations: bit-identical
// whatever the batch, the row's position in it, the row stride T and the launch.  Samples at or past len_b are never loaded.
#include <hip/hip_runtime.h>

#include "common.h"
#include "diffsound_hip.h"

#define LV_TILE 64                  // samples of a segment staged at a time = lanes of the wave
#define LV_PAD 65                   // tile row stride in floats: lane l reads row l, bank (l * 65 + i) % 32 -- no conflict
#define TP_BLOCK 1024               // input samples per workgroup of the true-peak kernel (4096 outputs)
#define TP_W 34                     // half width of the x4 filter (audio.resample_taps(fs, 4 fs))
#define TP_NTAP (2 * TP_W + 1)

struct LvLayout {                   // the scratch buffer shared by the ds_level_* entries
    long long slots;                // segments a row can hold + 1 (the trailing partial one)
    long long chunks;               // true-peak workgroups per row
    long long off_end, off_start, off_sx, off_px, off_tp, bytes;
};

static LvLayout lv_layout(int B, int T, int S) {
    LvLayout l;
    l.slots = (long long)T / S + 1;
    l.chunks = ((long long)T + TP_BLOCK - 1) / TP_BLOCK;
    if (l.chunks < 1) l.chunks = 1;
    l.off_end = 0;
    l.off_start = l.off_end + (long long)B * l.slots * 4 * sizeof(double);
    l.off_sx = l.off_start + (long long)B * l.slots * 4 * sizeof(double);
    l.off_px = l.off_sx + (long long)B * l.slots * sizeof(double);
    l.off_tp = l.off_px + (long long)B * l.slots * sizeof(float);
    l.bytes = l.off_tp + (long long)B * l.chunks * sizeof(float);
    l.bytes = (l.bytes + 15) / 16 * 16;
    return l;
}

__device__ __forceinline__ int lv_len(const int* lengths, int b, int T) {
    return lengths ? min(max(lengths[b], 0), T) : T;
}

// ENERGY = false: from the zero state, writes the end state.  ENERGY = true: from start[b][slot], writes seg / sx / px.
template <bool ENERGY>
__global__ __launch_bounds__(64) void ds_level_segments_kernel(const float* __restrict__ x, int T, const int* __restrict__ lengths,
                                                              int S, const double* __restrict__ kw, int slots,
                                                              double* __restrict__ end, const double* __restrict__ start,
                                                              double* __restrict__ seg, int n_seg_max, double* __restrict__ sx,
                                                              float* __restrict__ px) {
    __shared__ float tile[LV_TILE * LV_PAD];
    const int lane = threadIdx.x, b = blockIdx.y;
    const int slot0 = blockIdx.x * LV_TILE;
    const int len = lv_len(lengths, b, T);
    const int n_seg = len / S;
    if (slot0 > n_seg) {                                                // nothing of this row here: zero what is ours of seg
        if (ENERGY && slot0 + lane < n_seg_max) seg[(size_t)b * n_seg_max + slot0 + lane] = 0.0;
        return;
    }
    if (len == 0) {                                                      // an empty row: no sample of it may be loaded
        if (ENERGY) {
            if (lane < n_seg_max) seg[(size_t)b * n_seg_max + lane] = 0.0;
            if (lane == 0) sx[(size_t)b * slots] = 0.0, px[(size_t)b * slots] = 0.f;
        }
        return;
    }
    const float* xb = x + (size_t)b * T;
    const double b0 = kw[0], b1 = kw[1], b2 = kw[2], a1 = kw[3], a2 = kw[4], c1 = kw[8], c2 = kw[9];
    const int slot = slot0 + lane;
    double s1 = 0.0, s2 = 0.0, t1 = 0.0, t2 = 0.0;
    if (ENERGY && slot <= n_seg) {
        const double* st = start + ((size_t)b * slots + slot) * 4;
        s1 = st[0], s2 = st[1], t1 = st[2], t2 = st[3];
    }
    double e = 0.0, q = 0.0;
    float pk = 0.f;
    // 64 samples of each of the 64 segments, one coalesced 256-byte read per segment, held in registers: the reads of chunk
    // c + 1 are in flight while chunk c is filtered.  A read is unconditional -- its address clamped into [0, len) -- so the 64
    // of them issue back to back; what lies outside the segment or the row becomes zero when the registers go to LDS.
    float nxt[LV_TILE];
    const long long last = (long long)len - 1;
    auto fetch = [&](int c0) {
#pragma unroll
        for (int r = 0; r < LV_TILE; ++r) {
            const long long gi = (long long)(slot0 + r) * S + c0 + lane;
            nxt[r] = xb[gi < last ? gi : last];
        }
    };
    auto step = [&](float xf) {
        const double xv = (double)xf;
        const double y1 = b0 * xv + s1;
        s1 = b1 * xv - a1 * y1 + s2;
        s2 = b2 * xv - a2 * y1;
        const double y2 = y1 + t1;
        t1 = -2.0 * y1 - c1 * y2 + t2;
        t2 = y1 - c2 * y2;
        if (ENERGY) {
            e += y2 * y2;
            q += xv * xv;
            pk = fmaxf(pk, fabsf(xf));
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < S; c0 += LV_TILE) {
        const int n_i = min(LV_TILE, S - c0);
        __syncthreads();                                                 // the tile's last readers are done
#pragma unroll
        for (int r = 0; r < LV_TILE; ++r) {
            const long long left = (long long)len - (long long)(slot0 + r) * S - c0;      // samples of the row from this chunk on
            tile[r * LV_PAD + lane] = (lane < n_i && lane < left) ? nxt[r] : 0.f;
        }
        __syncthreads();
        if (c0 + LV_TILE < S) fetch(c0 + LV_TILE);
        const float* mine = tile + lane * LV_PAD;
        if (n_i == LV_TILE) {
#pragma unroll 8
            for (int i = 0; i < LV_TILE; ++i) step(mine[i]);
        } else {
            for (int i = 0; i < n_i; ++i) step(mine[i]);
        }
    }
    if (ENERGY) {
        if (slot < n_seg_max) seg[(size_t)b * n_seg_max + slot] = slot < n_seg ? e : 0.0;
        if (slot < slots) {
            sx[(size_t)b * slots + slot] = slot <= n_seg ? q : 0.0;      // samples past len were staged as zeros
            px[(size_t)b * slots + slot] = slot <= n_seg ? pk : 0.f;
        }
    } else if (slot < n_seg) {
        double* en = end + ((size_t)b * slots + slot) * 4;
        en[0] = s1, en[1] = s2, en[2] = t1, en[3] = t2;
    }
}

// sigma_0 = 0, sigma_{j+1} = P sigma_j + e_j: one wave per row.  Lane l holds e of segment base + l (read coalesced); the
// recurrence itself is uniform -- every lane runs it on the broadcast e_k -- and lane k keeps the state it saw before step k,
// so nothing in the serial chain waits for memory: n_seg steps of 16 float64 operations.
__device__ __forceinline__ double lv_bcast(double v, int k) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, k), hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), k);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

__global__ __launch_bounds__(64) void ds_level_carry_kernel(int T, const int* __restrict__ lengths, int S,
                                                           const double* __restrict__ kw, int slots,
                                                           const double* __restrict__ end, double* __restrict__ start) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int n_seg = lv_len(lengths, b, T) / S;
    double P[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) P[i] = kw[10 + i];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const double* en = end + (size_t)b * slots * 4;
    double* st = start + (size_t)b * slots * 4;
    for (int base = 0; base <= n_seg; base += 64) {
        const int j = base + lane;
        double e[4], mine[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) e[i] = j < n_seg ? en[(size_t)j * 4 + i] : 0.0, mine[i] = 0.0;
        for (int k = 0; k < 64; ++k) {
            double n[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (lane == k) mine[i] = s[i];
                n[i] = ((P[4 * i] * s[0] + P[4 * i + 1] * s[1]) + (P[4 * i + 2] * s[2] + P[4 * i + 3] * s[3])) + lv_bcast(e[i], k);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) s[i] = n[i];
        }
        if (j <= n_seg) {
#pragma unroll
            for (int i = 0; i < 4; ++i) st[(size_t)j * 4 + i] = mine[i];
        }
    }
}

// max |y| of the row resampled x4 with the project's own filter: the sum of ds_resample (L = 4, M = 1), fp32 fma over j
// ascending, one partial maximum per workgroup; the x4 signal is never stored.  A thread takes the four input positions
// tid, tid + 256, .. of the block and all four phases of each: 16 chains share every tap (wave-uniform: scalar loads) and
// every staged sample serves four of them.
__global__ __launch_bounds__(256) void ds_level_true_peak_kernel(const float* __restrict__ x, int T, const int* __restrict__ lengths,
                                                                const float* __restrict__ taps, int chunks,
                                                                float* __restrict__ part) {
    __shared__ float xs[TP_BLOCK + 2 * TP_W];
    __shared__ float red[4];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int len = lv_len(lengths, b, T);
    const long long i_base = (long long)blockIdx.x * TP_BLOCK;
    if (i_base >= len) {                                                 // (a row of no samples has the partial of chunk 0 only)
        if (tid == 0) part[(size_t)b * chunks + blockIdx.x] = 0.f;
        return;
    }
    const float* xb = x + (size_t)b * T;
    for (int i = tid; i < TP_BLOCK + 2 * TP_W; i += 256) {
        const long long gi = i_base - TP_W + i;
        xs[i] = (gi >= 0 && gi < len) ? xb[gi] : 0.f;
    }
    __syncthreads();
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[r][p] = 0.f;
    const float* xp = xs + tid;                                          // xp[256 r + j] = x[i0 - W + j], i0 = i_base + tid + 256 r
    for (int j = 0; j < TP_NTAP; ++j) {
        const float c0 = taps[j], c1 = taps[TP_NTAP + j], c2 = taps[2 * TP_NTAP + j], c3 = taps[3 * TP_NTAP + j];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float xv = xp[256 * r + j];
            acc[r][0] = fmaf(xv, c0, acc[r][0]);
            acc[r][1] = fmaf(xv, c1, acc[r][1]);
            acc[r][2] = fmaf(xv, c2, acc[r][2]);
            acc[r][3] = fmaf(xv, c3, acc[r][3]);
        }
    }
    float m = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r)                                          // outputs at and past 4 len are zero in ds_resample
        if (i_base + tid + 256 * r < len)
            m = fmaxf(fmaxf(m, fmaxf(fabsf(acc[r][0]), fabsf(acc[r][1]))), fmaxf(fabsf(acc[r][2]), fabsf(acc[r][3])));
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) part[(size_t)b * chunks + blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// the 64 lanes' partial sums, added in lane order by every lane: a fixed order whatever the launch
__device__ __forceinline__ double lv_sum64(double v, double* sh) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < 64; ++i) s += sh[i];
    return s;
}

// gate, loudness, peaks and the gain of a row: one wave per row
__global__ __launch_bounds__(64) void ds_level_gain_kernel(const double* __restrict__ seg, int n_seg_max, int T,
                                                          const int* __restrict__ lengths, int S, int slots, int chunks,
                                                          const double* __restrict__ sx, const float* __restrict__ px,
                                                          const float* __restrict__ tp, int strategy, double target,
                                                          const double* __restrict__ target_dev, int target_n, double ceiling,
                                                          double* __restrict__ lufs, float* __restrict__ peaks,
                                                          double* __restrict__ mean_sq, int* __restrict__ counts,
                                                          float* __restrict__ gain) {
    __shared__ double sh[64];
    const int lane = threadIdx.x, b = blockIdx.x;
    const int len = lv_len(lengths, b, T);
    const int n_seg = len / S, n_blk = n_seg >= 4 ? n_seg - 3 : 0;
    const double* sg = seg + (size_t)b * n_seg_max;
    const double g_abs = 1.1724653045822964e-07;                         // 10^((-70 + 0.691) / 10)
    const double den = 4.0 * (double)S;
    // pass 1: blocks over the absolute threshold
    double sum = 0.0, cnt = 0.0;
    for (int j = lane; j < n_blk; j += 64) {
        const double z = (((sg[j] + sg[j + 1]) + sg[j + 2]) + sg[j + 3]) / den;
        if (z > g_abs) sum += z, cnt += 1.0;
    }
    const double sum_a = lv_sum64(sum, sh), cnt_a = lv_sum64(cnt, sh);
    double L = -INFINITY, cnt_g = 0.0;
    if (cnt_a > 0.0) {
        const double g_rel = 0.1 * (sum_a / cnt_a);
        sum = 0.0, cnt = 0.0;
        for (int j = lane; j < n_blk; j += 64) {
            const double z = (((sg[j] + sg[j + 1]) + sg[j + 2]) + sg[j + 3]) / den;
            if (z > g_abs && z > g_rel) sum += z, cnt += 1.0;
        }
        const double sum_g = lv_sum64(sum, sh);
        cnt_g = lv_sum64(cnt, sh);
        if (cnt_g > 0.0) L = -0.691 + 10.0 * log10(sum_g / cnt_g);
    }
    // sample peak, sum x^2, true peak
    double q = 0.0;
    float pk = 0.f, tpk = 0.f;
    for (int j = lane; j <= n_seg; j += 64) {
        q += sx[(size_t)b * slots + j];
        pk = fmaxf(pk, px[(size_t)b * slots + j]);
    }
    const int n_chunk = (len + TP_BLOCK - 1) / TP_BLOCK;
    for (int j = lane; j < n_chunk; j += 64) tpk = fmaxf(tpk, tp[(size_t)b * chunks + j]);
    const double q_all = lv_sum64(q, sh);
    for (int o = 32; o > 0; o >>= 1) {
        pk = fmaxf(pk, __shfl_xor(pk, o));
        tpk = fmaxf(tpk, __shfl_xor(tpk, o));
    }
    tpk = fmaxf(tpk, pk);
    if (lane != 0) return;
    const double ms = len > 0 ? q_all / (double)len : 0.0;
    double g = 1.0;
    if (strategy == DS_LEVEL_PEAK) {
        if (pk > 0.f) g = pow(10.0, target / 20.0) / (double)pk;
    } else if (strategy == DS_LEVEL_RMS) {
        if (ms > 0.0) g = pow(10.0, target / 20.0) / sqrt(ms);
    } else if (strategy == DS_LEVEL_LOUDNESS) {
        const double tg = target_dev ? target_dev[target_n > 1 ? b : 0] : target;
        if (L > -INFINITY && tg > -INFINITY && tg < INFINITY && tg == tg) g = pow(10.0, (tg - L) / 20.0);
    }
    if (strategy != DS_LEVEL_MEASURE && g * (double)tpk > ceiling) g = ceiling / (double)tpk;
    float g32 = (float)g;
    if (!(g32 > 0.f) || !(g32 < INFINITY)) g32 = 1.f;                    // never a NaN, an inf or a zero gain
    if (strategy != DS_LEVEL_MEASURE && (double)g32 * (double)tpk > ceiling)
        g32 = __uint_as_float(__float_as_uint(g32) - 1u);                // the rounding to fp32 went up: one step down
    lufs[b] = L;
    peaks[2 * b] = pk;
    peaks[2 * b + 1] = tpk;
    mean_sq[b] = ms;
    if (counts) counts[2 * b] = (int)cnt_a, counts[2 * b + 1] = (int)cnt_g;
    gain[b] = g32;
}

// out[b][i] = g[b] x[b][i] for i < len_b, 0 past it.  VEC: 16-byte accesses (T % 4 == 0, 16-byte aligned pointers)
template <bool VEC>
__global__ __launch_bounds__(256) void ds_level_apply_kernel(const float* x, const float* __restrict__ gain, float* out, int T,
                                                            const int* __restrict__ lengths) {
    const int b = blockIdx.y;
    const int len = lv_len(lengths, b, T);
    const float g = gain[b];
    const float* xb = x + (size_t)b * T;
    float* ob = out + (size_t)b * T;
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= T) return;
    if (VEC && i + 4 <= len) {
        f32x4 v = *(const f32x4*)(xb + i);
        v.x *= g, v.y *= g, v.z *= g, v.w *= g;
        *(f32x4*)(ob + i) = v;
    } else {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (i + k < len) ? g * xb[i + k] : 0.f;
        if (VEC) {
            *(f32x4*)(ob + i) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i + k < T) ob[i + k] = v[k];
        }
    }
}

extern "C" int64_t ds_level_scratch_bytes(int B, int T, int S) {
    if (B < 1 || T < 0 || S < 1) return -1;
    return lv_layout(B, T, S).bytes;
}

extern "C" int ds_level_segments(const float* x, int B, int T, const int32_t* lengths, int S, const double* kw, double* seg,
                                 int n_seg_max, void* scratch, int64_t scratch_bytes, ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(x && kw && seg && scratch, "null pointer");
    DS_CHECK_ARG(B >= 1 && B <= 65535 && T >= 0, "bad sizes");
    DS_CHECK_ARG(S >= 1, "S must be >= 1");
    DS_CHECK_ARG(n_seg_max >= T / S, "n_seg_max must hold floor(T / S) segments");
    const LvLayout l = lv_layout(B, T, S);
    DS_CHECK_ARG(scratch_bytes >= l.bytes, "scratch is smaller than ds_level_scratch_bytes(B, T, S)");
    DS_CHECK_ARG(((uintptr_t)scratch & 7) == 0, "scratch must be 8-byte aligned");
    char* sc = (char*)scratch;
    double* end = (double*)(sc + l.off_end);
    double* start = (double*)(sc + l.off_start);
    double* sx = (double*)(sc + l.off_sx);
    float* px = (float*)(sc + l.off_px);
    const int slots = (int)l.slots;
    const int cover = max(slots, n_seg_max);                             // seg is zeroed up to n_seg_max
    const dim3 grid((cover + LV_TILE - 1) / LV_TILE, B);
    hipLaunchKernelGGL(ds_level_segments_kernel<false>, grid, dim3(64), 0, stream, x, T, lengths, S, kw, slots, end, start, seg,
                       n_seg_max, sx, px);
    hipLaunchKernelGGL(ds_level_carry_kernel, dim3(B), dim3(64), 0, stream, T, lengths, S, kw, slots, end, start);
    hipLaunchKernelGGL(ds_level_segments_kernel<true>, grid, dim3(64), 0, stream, x, T, lengths, S, kw, slots, end, start, seg,
                       n_seg_max, sx, px);
    DS_CHECK_LAUNCH();
    return 0;
}

extern "C" int ds_level_true_peak(const float* x, int B, int T, const int32_t* lengths, int S, const float* taps, void* scratch,
                                  int64_t scratch_bytes, ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(x && taps && scratch, "null pointer");
    DS_CHECK_ARG(B >= 1 && B <= 65535 && T >= 0, "bad sizes");
    DS_CHECK_ARG(S >= 1, "S must be >= 1");
    const LvLayout l = lv_layout(B, T, S);
    DS_CHECK_ARG(scratch_bytes >= l.bytes, "scratch is smaller than ds_level_scratch_bytes(B, T, S)");
    DS_CHECK_ARG(((uintptr_t)scratch & 7) == 0, "scratch must be 8-byte aligned");
    float* tp = (float*)((char*)scratch + l.off_tp);
    hipLaunchKernelGGL(ds_level_true_peak_kernel, dim3((int)l.chunks, B), dim3(256), 0, stream, x, T, lengths, taps,
                       (int)l.chunks, tp);
    DS_CHECK_LAUNCH();
    return 0;
}

extern "C" int ds_level_gain(const double* seg, int n_seg_max, int B, int T, const int32_t* lengths, int S, int strategy,
                             double target, const double* target_dev, int target_n, double ceiling_db, const void* scratch,
                             int64_t scratch_bytes, double* lufs, float* peaks, double* mean_sq, int32_t* counts, float* gain,
                             ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(seg && scratch && lufs && peaks && mean_sq && gain, "null pointer");
    DS_CHECK_ARG(B >= 1 && B <= 65535 && T >= 0, "bad sizes");
    DS_CHECK_ARG(S >= 1, "S must be >= 1");
    DS_CHECK_ARG(n_seg_max >= T / S, "n_seg_max must hold floor(T / S) segments");
    DS_CHECK_ARG(strategy >= DS_LEVEL_MEASURE && strategy <= DS_LEVEL_LOUDNESS, "unknown strategy");
    DS_CHECK_ARG(target == target && target < INFINITY && target > -INFINITY, "target must be finite");
    DS_CHECK_ARG(ceiling_db == ceiling_db && ceiling_db < INFINITY && ceiling_db > -INFINITY, "ceiling_db must be finite");
    DS_CHECK_ARG(!target_dev || (strategy == DS_LEVEL_LOUDNESS && (target_n == 1 || target_n == B)),
                 "target_dev goes with the loudness strategy and holds 1 or B values");
    const LvLayout l = lv_layout(B, T, S);
    DS_CHECK_ARG(scratch_bytes >= l.bytes, "scratch is smaller than ds_level_scratch_bytes(B, T, S)");
    DS_CHECK_ARG(((uintptr_t)scratch & 7) == 0, "scratch must be 8-byte aligned");
    const char* sc = (const char*)scratch;
    hipLaunchKernelGGL(ds_level_gain_kernel, dim3(B), dim3(64), 0, stream, seg, n_seg_max, T, lengths, S, (int)l.slots,
                       (int)l.chunks, (const double*)(sc + l.off_sx), (const float*)(sc + l.off_px),
                       (const float*)(sc + l.off_tp), strategy, target, target_dev, target_n, pow(10.0, ceiling_db / 20.0), lufs,
                       peaks, mean_sq, counts, gain);
    DS_CHECK_LAUNCH();
    return 0;
}

extern "C" int ds_level_apply(const float* x, const float* gain, float* out, int B, int T, const int32_t* lengths,
                              ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(x && gain && out, "null pointer");
    DS_CHECK_ARG(B >= 1 && B <= 65535 && T >= 0, "bad sizes");
    if (T == 0) return 0;
    const dim3 grid((unsigned)(((long long)T + 1023) / 1024), B);
    const bool vec = T % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(ds_level_apply_kernel<true>, grid, dim3(256), 0, stream, x, gain, out, T, lengths);
    else
        hipLaunchKernelGGL(ds_level_apply_kernel<false>, grid, dim3(256), 0, stream, x, gain, out, T, lengths);
    DS_CHECK_LAUNCH();
    return 0;
}
