// Band-limited rational resampling in ONE launch (ds_resample): y[n] = sum_j x[i0 + j] C[p][j + W], p = (n M) mod L,
// i0 = (n M) div L, C = the Kaiser-windowed sinc sampled per phase (f32[L][2W+1], built in float64 on the host:
// audio.resample_taps).  Stands in for `librosa.load(path, sr=22050)` of the reference's data preparation
// (Codebook/feature_extraction/extract_mel_spectrogram.py:167) and the 32 kHz resampling of its captioning metric
// (Codebook/AudiocaptionLoss/data_handling/audiocaps_dataset.py:246-260).
//
// A workgroup (256 threads) takes a contiguous block of outputs of one clip:
//   1. the input span the block needs (block * M / L + 2 W samples) is staged in LDS once; zeros outside [0, len_b) are index
//      arithmetic in this loader, so the zero extension / the cut to n_out needs no host pass.  The block's first input
//      index and phase are computed in 64 bits once (n M exceeds 32 bits for long recordings); everything else is an offset.
//   2. Consecutive outputs walk through DIFFERENT table rows, and the table can exceed LDS (174 KB at 441/640), so it is read
//      through L1 / L2.  To pay each table read once for several multiply-adds the block is RS_R x (k L) outputs long, and
//      a thread takes the RS_R outputs s, s + k L, s + 2 k L, ..: they share the phase, so one C[p][j] serves RS_R
//      accumulators and their inputs sit k M samples apart in LDS.  k is chosen by the launcher so that the k L slots fill
//      whole passes of the 256 threads as well as possible within 60 KB of LDS.
//   3. Ratios whose k = 1 block does not fit (M large) take the one-output-per-thread form of the same loop (RS_R = 1, 1024
//      outputs per block): the same sum in the same order.
// Every output is one thread's fp32 fma chain over j ascending -- no atomics, no workspace --, so a clip's result is
// bit-identical whatever the batch, its position in it, n_out and the launch it is part of.
#include <hip/hip_runtime.h>

#include "common.h"
#include "diffsound_hip.h"

#ifndef RS_R
#define RS_R 8                      // outputs per thread that share a table row (A/B: 1 = every output reads its own row)
#endif
#define RS_MAX_FLOATS 15360         // staged input samples per workgroup: 60 KB, so at least two workgroups per CU
#define RS_PLAIN_BLOCK 1024         // outputs per workgroup of the one-output-per-thread form

template <int R>
__global__ __launch_bounds__(256) void ds_resample_kernel(const float* __restrict__ x, int T, const int* __restrict__ lengths,
                                                         int L, int M, const float* __restrict__ taps, int W,
                                                         float* __restrict__ y, int n_out, int slots, int span) {
    extern __shared__ __attribute__((aligned(16))) float xs[];          // [span]: x[b][i0_base - W ..]
    const int tid = threadIdx.x, b = blockIdx.y;
    const int block = R * slots;                                        // outputs of this workgroup
    const long long n0 = (long long)blockIdx.x * block;
    int len = T;
    if (lengths) len = min(max(lengths[b], 0), T);
    const long long n_valid = ((long long)len * L + M - 1) / M;         // outputs at and past it are zero
    float* yb = y + (size_t)b * n_out;
    if (n0 >= n_valid) {
        for (int o = tid; o < block; o += 256)
            if (n0 + o < n_out) yb[n0 + o] = 0.f;
        return;
    }
    const long long base = n0 * M;                                      // 64-bit once
    const long long i0_base = base / L;
    const int p_base = (int)(base - i0_base * L);
    const float* xb = x + (size_t)b * T;
    const long long first = i0_base - W;
    for (int i = tid; i < span; i += 256) {
        const long long gi = first + i;
        xs[i] = (gi >= 0 && gi < len) ? xb[gi] : 0.f;
    }
    __syncthreads();

    const int ntap = 2 * W + 1;
    const int d_in = (int)((long long)slots * M / L);                   // R > 1: slots = k L, the step is k M exactly
    for (int s = tid; s < slots; s += 256) {
        const int q = s * M + p_base;
        const int i_off = q / L, p = q - i_off * L;
        const float* c = taps + (size_t)p * ntap;
        const float* xp = xs + i_off;
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.f;
        for (int j = 0; j < ntap; ++j) {
            const float cj = c[j];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = fmaf(xp[r * d_in + j], cj, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const long long n = n0 + s + (long long)r * slots;
            if (n < n_out) yb[n] = n < n_valid ? acc[r] : 0.f;
        }
    }
}

static long long ds_gcd(long long a, long long b) {
    while (b) {
        const long long t = a % b;
        a = b;
        b = t;
    }
    return a;
}

extern "C" int ds_resample(const float* x, int B, int T, const int32_t* lengths, int L, int M, const float* taps, int W,
                           float* y, int n_out, ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(x && taps && y, "null pointer");
    DS_CHECK_ARG(B >= 1 && B <= 65535 && T >= 0, "bad sizes");
    DS_CHECK_ARG(L >= 1 && M >= 1 && L < (1 << 20) && M < (1 << 20), "L and M must be in 1 .. 2^20");
    DS_CHECK_ARG(ds_gcd(L, M) == 1, "L / M must be in lowest terms");
    DS_CHECK_ARG(W >= 1 && W < (1 << 20), "W must be in 1 .. 2^20");
    DS_CHECK_ARG(n_out >= 0, "n_out must be >= 0");
    if (n_out == 0) return 0;
    // the block: RS_R x (k L) outputs, k = the one whose k L slots waste the fewest lanes of whole 256-thread passes
    int slots = 0;
    if (RS_R > 1) {
        double best = 0.0;
        for (long long k = 1; k * L <= 4096 && (long long)RS_R * k * M + 2 * W + 2 <= RS_MAX_FLOATS; ++k) {
            const long long kl = k * L;
            const double util = (double)kl / (double)((kl + 255) / 256 * 256);
            if (util > best + 1e-9) {
                best = util;
                slots = (int)kl;
            }
        }
    }
    const int grid_y = B;
    if (slots) {
        const int block = RS_R * slots;
        const int span = (int)((long long)block * M / L) + 2 * W + 2;
        hipLaunchKernelGGL(ds_resample_kernel<RS_R>, dim3((n_out + block - 1) / block, grid_y), dim3(256), span * sizeof(float),
                           stream, x, T, lengths, L, M, taps, W, y, n_out, slots, span);
    } else {
        const long long span = (long long)RS_PLAIN_BLOCK * M / L + 2 * W + 2;
        DS_CHECK_ARG(span <= RS_MAX_FLOATS, "M / L or W too large for the built block (1024 M / L + 2 W + 2 <= 15360)");
        hipLaunchKernelGGL(ds_resample_kernel<1>, dim3((n_out + RS_PLAIN_BLOCK - 1) / RS_PLAIN_BLOCK, grid_y), dim3(256),
                           (size_t)span * sizeof(float), stream, x, T, lengths, L, M, taps, W, y, n_out, RS_PLAIN_BLOCK,
                           (int)span);
    }
    DS_CHECK_LAUNCH();
    return 0;
}
