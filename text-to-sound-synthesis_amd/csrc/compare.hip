// Two waveforms side by side on the device (include/diffsound_hip.h: ds_compare_*): the lag at which a rendering b lines up
// with its reference a, the time-domain distances at that lag (SI-SDR, SNR), and the spectral-convergence and log-magnitude
// distances of three STFT resolutions.  Every sum is float64, taken over a partition that depends on the region alone and added
// in a fixed order without atomics: a row's every result has the same bits whatever the batch and the row's position in it.
//
//   ds_xcorr_partials  r(l) = sum b[n] a[n+l], ea(l) = sum a[n+l]^2, eb = sum b[n]^2 per (row, tile of CP_TILE samples, lag).
//       A workgroup owns CP_LAGS = 1024 lags of a tile: thread t the FOUR CONSECUTIVE lags 4t .. 4t+3, so the a samples of four
//       steps of n are a window of seven values that slides by four -- per four samples a lane reads four new a values and
//       four (broadcast) b values from LDS and issues 32 fma: the kernel is bound by v_fma_f64, which gfx950 issues at the
//       fp32 rate (stft_mel.hip relies on the same).  The tile is staged CP_SUB samples at a time, as doubles (the loop has no
//       conversions): b's CP_SUB and a's CP_SUB + CP_LAGS, i.e. 2x the tile's own bytes whatever max_lag.  A lane's four values
//       are 32 bytes apart: 8-byte LDS reads of a 32-lane group then fall on 32 distinct bank pairs twice over -- a 2-way
//       conflict on reads that are a quarter of the fma issue time.  The accumulators stay in registers over the whole tile.
//       r, ea and eb add the same (exact) products in the same order, so b[n] == a[n+l] on the region gives r == ea == eb to
//       the bit, rho within a rounding of 1 and alpha == 1.
//   ds_xcorr_select    one wave per row: tiles added in order, rho, argmax under the tie rule (smallest |l|, then negative).
//   ds_xcorr_refine    r, ea, eb at the chosen lag once more in double-double: the rho and the sums that are reported.  A lag
//       given by the caller goes straight here: no search kernel is launched for it.
//       A workgroup of the search always works 1 024 lags, so 2 M + 1 lags are padded to a multiple of that: at M = 2 048,
//       5 120 lags for 4 097 -- a quarter more fma than the stated floor counts.
//   ds_compare_residual  e_res = sum (b - alpha a)^2 and e_dif = sum (b - a)^2 at the row's lag (read from device memory),
//       summed directly -- never as eb - 2 alpha r + alpha^2 ea, which cancels at high rho -- and ea once more in this pass's
//       own order, so that the two ratios divide sums of the same order (b = 0 gives e_dif == ea to the bit: 0 dB exactly).
//   ds_stft_compare    a wave transforms a frame of b, then the same frame of a, through the SAME instructions (one loop body,
//       not unrolled): the double 1024-point FFT of stft_mel_fft.h with the magnitudes kept in double; identical samples give
//       identical magnitudes and exact zeros.  One partial per workgroup (16 frames) and resolution.
//   ds_compare_finish  one wave per row: the partials added in order, the ratios, the logarithms.
//   ds_compare_l1      mean |x - y| of two fp32 rows in float64 (the log-mel distance of audio.compare).
// Samples of a that a lag would reach outside [0, Na) are never loaded and count as zero.
#include <hip/hip_runtime.h>

#include "common.h"
#include "diffsound_hip.h"
#include "stft_mel_fft.h"

DS_FFT_DEV float ds_fft_sqrt(float x) { return __fsqrt_rn(x); }       // (the header's fp32 split declares it; unused here)

#define CP_MAX_LAG 4096            // one token column: a design choice, not a limit of the method
#define CP_TILE 8192                // samples of the region per partial sum
#define CP_SUB 1024                 // samples staged at a time
#define CP_LAGS 1024                // lags per workgroup = 256 threads x 4
#define CP_AS (CP_SUB + CP_LAGS + 8)
#define CP_FR 16                    // frames per workgroup of the STFT kernel (4 per wave)
#define CP_NFFT 1024
#define CP_BINS 513
#define CP_FLOOR 1e-5               // Audio2Mel's floor under the logarithm

__constant__ int cp_win[3] = {256, 512, 1024};
__constant__ int cp_hop[3] = {64, 128, 256};
static const int cp_win_h[3] = {256, 512, 1024};
static const int cp_hop_h[3] = {64, 128, 256};

struct CpLayout {
    long long tiles, chunks, lp, groups;        // lp: padded lags per (row, tile); groups: STFT workgroups of resolution 0
    long long frames[3];
    long long off_part, off_eb, off_res, off_st, bytes;
};

static CpLayout cp_layout(int B, long long n, int M) {
    CpLayout l;
    l.tiles = (n + CP_TILE - 1) / CP_TILE;
    if (l.tiles < 1) l.tiles = 1;
    l.chunks = (2ll * M + 1 + CP_LAGS - 1) / CP_LAGS;
    l.lp = l.chunks * CP_LAGS;
    for (int i = 0; i < 3; ++i) l.frames[i] = n >= CP_NFFT ? (n - cp_win_h[i]) / cp_hop_h[i] + 1 : 0;
    l.groups = (l.frames[0] + CP_FR - 1) / CP_FR;
    if (l.groups < 1) l.groups = 1;
    l.off_part = 0;
    l.off_eb = l.off_part + (long long)B * l.tiles * 2 * l.lp * sizeof(double);
    l.off_res = l.off_eb + (long long)B * l.tiles * sizeof(double);
    l.off_st = l.off_res + (long long)B * l.tiles * 3 * sizeof(double);
    l.bytes = l.off_st + (long long)B * 3 * l.groups * 3 * sizeof(double);
    return l;
}

// the 64 lanes' values added as a butterfly, then the four waves' sums in wave order: a fixed order whatever the launch
__device__ __forceinline__ double cp_block_sum(double v, double* sh4) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh4[0] + sh4[1]) + sh4[2]) + sh4[3];
}

__global__ __launch_bounds__(256) void ds_xcorr_partials_kernel(const float* __restrict__ a, const float* __restrict__ b, int Na,
                                                               int Nb, int s0, int s1, int M, const int* __restrict__ lag_dev,
                                                               int lag, int tiles, int lp, double* __restrict__ part,
                                                               double* __restrict__ eb_part) {
    __shared__ double as_[CP_AS];
    __shared__ double bs[CP_SUB];
    const int tid = threadIdx.x, tile = blockIdx.x, chunk = blockIdx.y, row = blockIdx.z;
    const float* ar = a + (size_t)row * Na;
    const float* br = b + (size_t)row * Nb;
    const long long centre = lag_dev ? lag_dev[row] : lag;
    const long long t0 = (long long)s0 + (long long)tile * CP_TILE;
    const long long t1 = min(t0 + CP_TILE, (long long)s1);
    const long long shift = centre - M + (long long)chunk * CP_LAGS;            // a index of (sample n, lag 0 of the chunk) = n + shift
    const int q = 4 * tid;
    const bool do_eb = chunk == 0;
    double r[4] = {0.0, 0.0, 0.0, 0.0}, e[4] = {0.0, 0.0, 0.0, 0.0}, eb = 0.0;
    for (long long n0 = t0; n0 < t1; n0 += CP_SUB) {
        const int nv = (int)min((long long)CP_SUB, t1 - n0);
        __syncthreads();                                                         // the last readers of the stage are done
        for (int i = tid; i < CP_AS; i += 256) {
            const long long gi = n0 + shift + i;
            as_[i] = (gi >= 0 && gi < Na) ? (double)ar[gi] : 0.0;
        }
        for (int i = tid; i < CP_SUB; i += 256) bs[i] = i < nv ? (double)br[n0 + i] : 0.0;
        __syncthreads();
        const double* wp = as_ + q;
        double w[7];
        w[0] = wp[0], w[1] = wp[1], w[2] = wp[2];
        int i0 = 0;
        for (; i0 + 4 <= nv; i0 += 4) {
#pragma unroll
            for (int k = 3; k < 7; ++k) w[k] = wp[i0 + k];
            double bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) bv[i] = bs[i0 + i];
#pragma unroll
            for (int i = 0; i < 4; ++i) {                                        // sample i0 + i: lag k pairs it with w[i + k]
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    r[k] = fma(bv[i], w[i + k], r[k]);
                    e[k] = fma(w[i + k], w[i + k], e[k]);
                }
                if (do_eb) eb = fma(bv[i], bv[i], eb);
            }
            w[0] = w[4], w[1] = w[5], w[2] = w[6];
        }
        for (int i = i0; i < nv; ++i) {                                          // the region's last one to three samples
            const double bv = bs[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double wv = wp[i + k];
                r[k] = fma(bv, wv, r[k]);
                e[k] = fma(wv, wv, e[k]);
            }
            if (do_eb) eb = fma(bv, bv, eb);
        }
    }
    double* pr = part + (((size_t)row * tiles + tile) * 2) * lp + (size_t)chunk * CP_LAGS + q;
#pragma unroll
    for (int k = 0; k < 4; ++k) pr[k] = r[k], pr[lp + k] = e[k];
    if (do_eb && tid == 0) eb_part[(size_t)row * tiles + tile] = eb;
}

// is candidate (key, l) better than (bkey, bl)?  key: rho, a NaN counted as -inf; distances are taken from the centre
__device__ __forceinline__ bool cp_better(double key, long long d, double bkey, long long bd) {
    if (key != bkey) return key > bkey;
    const long long ad = d < 0 ? -d : d, abd = bd < 0 ? -bd : bd;
    if (ad != abd) return ad < abd;
    return d < bd;
}

__global__ __launch_bounds__(64) void ds_xcorr_select_kernel(int M, const int* __restrict__ lag_dev, int lag, int tiles, int lp,
                                                            const double* __restrict__ part, const double* __restrict__ eb_part,
                                                            int* __restrict__ lag_out, double* __restrict__ rho_out,
                                                            double* __restrict__ sums) {
    const int lane = threadIdx.x, row = blockIdx.x;
    const int centre = lag_dev ? lag_dev[row] : lag;
    double eb = 0.0;
    for (int t = 0; t < tiles; ++t) eb += eb_part[(size_t)row * tiles + t];
    double bkey = -INFINITY, brho = 0.0, br = 0.0, be = 0.0;
    long long bd = 1ll << 40;                                                    // no candidate yet: loses every tie
    for (int li = lane; li <= 2 * M; li += 64) {
        const double* p = part + (size_t)row * tiles * 2 * lp + li;
        double r = 0.0, ea = 0.0;
        for (int t = 0; t < tiles; ++t) {
            r += p[(size_t)t * 2 * lp];
            ea += p[(size_t)t * 2 * lp + lp];
        }
        const double rho = (ea == 0.0 || eb == 0.0) ? 0.0 : r / sqrt(ea * eb);
        const double key = rho == rho ? rho : -INFINITY;
        const long long d = li - M;
        if (cp_better(key, d, bkey, bd)) bkey = key, bd = d, brho = rho, br = r, be = ea;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double okey = __shfl_xor(bkey, o), orho = __shfl_xor(brho, o), orr = __shfl_xor(br, o), oe = __shfl_xor(be, o);
        const long long od = __shfl_xor(bd, o);
        if (cp_better(okey, od, bkey, bd)) bkey = okey, bd = od, brho = orho, br = orr, be = oe;
    }
    if (lane == 0) {
        lag_out[row] = centre + (int)bd;
        rho_out[row] = brho;
        sums[3 * row] = br, sums[3 * row + 1] = be, sums[3 * row + 2] = eb;
    }
}

// a given lag: nothing to search, the row's lag is written as it came
__global__ void ds_xcorr_given_kernel(int B, const int* __restrict__ lag_dev, int lag, int* __restrict__ lag_out) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row < B) lag_out[row] = lag_dev ? lag_dev[row] : lag;
}

// (hi, lo) += p in double-double: hi + lo carries the running sum to about twice the precision of a double (Knuth's two-sum)
__device__ __forceinline__ void cp_dd_add(double& hi, double& lo, double p, double plo = 0.0) {
    const double s = hi + p, bb = s - hi;
    lo += ((hi - (s - bb)) + (p - bb)) + plo;
    hi = s;
}

// The three sums at the chosen lag once more, in double-double, and rho and sums from them: the search adds up to 8192 products
// in sequence, which leaves rho some 1e-14 from its float64 value -- nothing to a search, but more than the distance of a
// float32 evaluation from it where rho is within a few roundings of 1 (a scaled copy).  One workgroup per row: lane t takes the
// samples s0 + t, s0 + t + 256, ..; the lanes' (hi, lo) pairs are added as a butterfly, then the four waves' in wave order.  The
// three sums add the same products in the same order, so b[n] == a[n+l] still gives r == ea == eb to the bit.
__global__ __launch_bounds__(256) void ds_xcorr_refine_kernel(const float* __restrict__ a, const float* __restrict__ b, int Na,
                                                             int Nb, int s0, int s1, const int* __restrict__ lag_dev,
                                                             double* __restrict__ rho_out, double* __restrict__ sums) {
    __shared__ double sh[4][6];
    const int tid = threadIdx.x, row = blockIdx.x;
    const float* ar = a + (size_t)row * Na;
    const float* br = b + (size_t)row * Nb;
    const long long lag = lag_dev[row];
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                               // (hi, lo) of r, ea, eb
    for (long long n = (long long)s0 + tid; n < s1; n += 256) {
        const long long gi = n + lag;
        const double av = (gi >= 0 && gi < Na) ? (double)ar[gi] : 0.0, bv = (double)br[n];
        cp_dd_add(v[0], v[1], bv * av);                                          // the products of two fp32 values are exact
        cp_dd_add(v[2], v[3], av * av);
        cp_dd_add(v[4], v[5], bv * bv);
    }
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double ohi = __shfl_xor(v[2 * j], o), olo = __shfl_xor(v[2 * j + 1], o);
            cp_dd_add(v[2 * j], v[2 * j + 1], ohi, olo);
        }
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 6; ++j) sh[tid >> 6][j] = v[j];
    }
    __syncthreads();
    if (tid != 0) return;
    double t[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double hi = sh[0][2 * j], lo = sh[0][2 * j + 1];
        for (int w = 1; w < 4; ++w) cp_dd_add(hi, lo, sh[w][2 * j], sh[w][2 * j + 1]);
        t[j] = hi + lo;
    }
    rho_out[row] = (t[1] == 0.0 || t[2] == 0.0) ? 0.0 : t[0] / sqrt(t[1] * t[2]);
    sums[3 * row] = t[0], sums[3 * row + 1] = t[1], sums[3 * row + 2] = t[2];
}

__global__ __launch_bounds__(256) void ds_compare_residual_kernel(const float* __restrict__ a, const float* __restrict__ b, int Na,
                                                                 int Nb, int s0, int s1, const int* __restrict__ lag_dev,
                                                                 const double* __restrict__ sums, int tiles,
                                                                 double* __restrict__ res_part) {
    __shared__ double sh[4];
    const int tid = threadIdx.x, tile = blockIdx.x, row = blockIdx.y;
    const float* ar = a + (size_t)row * Na;
    const float* br = b + (size_t)row * Nb;
    const long long lag = lag_dev[row];
    const double rr = sums[3 * row], ea = sums[3 * row + 1];
    const double alpha = ea == 0.0 ? 0.0 : rr / ea;
    const long long t0 = (long long)s0 + (long long)tile * CP_TILE;
    const long long t1 = min(t0 + CP_TILE, (long long)s1);
    double q = 0.0, p = 0.0, ea2 = 0.0;
    for (long long n = t0 + tid; n < t1; n += 256) {
        const long long gi = n + lag;
        const double av = (gi >= 0 && gi < Na) ? (double)ar[gi] : 0.0, bv = (double)br[n];
        const double d = bv - alpha * av, f = bv - av;
        q = fma(d, d, q);
        p = fma(f, f, p);
        ea2 = fma(av, av, ea2);
    }
    const double qs = cp_block_sum(q, sh), ps = cp_block_sum(p, sh), es = cp_block_sum(ea2, sh);
    if (tid == 0) {
        double* o = res_part + ((size_t)row * tiles + tile) * 3;
        o[0] = qs, o[1] = ps, o[2] = es;
    }
}

// the real-input split of stft_mel_fft.h with the magnitudes left in double: m[i] = |X[lane + 64 i]|, m[4 + i] = |X[512 - lane - 64 i]|,
// m[8] = |X[256]| on lane 0 (0 on the others)
__device__ __forceinline__ void cp_split_mag(const ds_cf* S, const ds_cf* tw4, ds_cf w256, int lane, double* m) {
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int k = i < 4 ? lane + 64 * i : 256;
        const ds_cf w = i < 4 ? tw4[i] : w256;
        const ds_cf A = S[DS_FFT_ZP(k)];
        const ds_cf Zm = S[DS_FFT_ZP((512 - k) & 511)];
        const ds_cf E = ds_cf{A.x + Zm.x, A.y - Zm.y};
        const ds_cf D = ds_cf{A.x - Zm.x, A.y + Zm.y};
        const ds_cf wO = ds_cf_mul(w, ds_cf_mul_mi(D));
        const ds_cf p = ds_cf_add(E, wO), mm = ds_cf_sub(E, wO);
        const double mk = 0.5 * sqrt(p.x * p.x + p.y * p.y), mn = 0.5 * sqrt(mm.x * mm.x + mm.y * mm.y);
        if (i < 4)
            m[i] = mk, m[4 + i] = mn;
        else
            m[8] = lane == 0 ? mk : 0.0;
    }
}

__global__ __launch_bounds__(256) void ds_stft_compare_kernel(const float* __restrict__ a, const float* __restrict__ b, int Na,
                                                             int Nb, int s0, int s1, const int* __restrict__ lag_dev,
                                                             const float* __restrict__ windows, const ds_cf* __restrict__ tw,
                                                             int groups, double* __restrict__ st_part) {
    __shared__ __attribute__((aligned(16))) ds_cf scratch[4 * DS_FFT_SCRATCH];
    __shared__ double sh[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int group = blockIdx.x, res = blockIdx.y, row = blockIdx.z;
    const int w_len = cp_win[res], hop = cp_hop[res];
    const int n_frames = (s1 - s0 - w_len) / hop + 1;
    if (group * CP_FR >= n_frames) return;                                       // (the whole workgroup: before any barrier)
    ds_cf* S = scratch + wid * DS_FFT_SCRATCH;
    const float* ar = a + (size_t)row * Na;
    const float* br = b + (size_t)row * Nb;
    const long long lag = lag_dev[row];
    const float* window = windows + res * CP_NFFT;
    float win[16];
    ds_cf tw1[7], tw2[7], tw4[4];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        win[2 * r] = window[2 * (lane + 64 * r)];
        win[2 * r + 1] = window[2 * (lane + 64 * r) + 1];
    }
#pragma unroll
    for (int r = 1; r < 8; ++r) {
        tw1[r - 1] = tw[(lane & 7) * r * 8];
        tw2[r - 1] = tw[lane * r];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) tw4[i] = tw[512 + lane + 64 * i];
    const ds_cf w256 = tw[512 + 256];
    double num = 0.0, den = 0.0, lg = 0.0;
    for (int it = 0; it < CP_FR / 4; ++it) {                                     // every wave runs every iteration: the barriers
        const int f = group * CP_FR + it * 4 + wid;
        const bool valid = f < n_frames;
        const long long fs = (long long)s0 + (long long)f * hop;
        double mb[9];
#pragma unroll 1
        for (int side = 0; side < 2; ++side) {                                   // 0: the frame of b, 1: the frame of a, lag later
            const float* src = side ? ar : br;
            const long long lim = side ? Na : Nb, start = side ? fs + lag : fs;
            ds_cf v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int j = 2 * (lane + 64 * r);                               // w_len is even: j and j + 1 are inside together
                const long long g0 = start + j;
                const float x0 = (valid && j < w_len && g0 >= 0 && g0 < lim) ? src[g0] : 0.f;
                const float x1 = (valid && j < w_len && g0 + 1 >= 0 && g0 + 1 < lim) ? src[g0 + 1] : 0.f;
                v[r] = ds_cf{(double)x0 * (double)win[2 * r], (double)x1 * (double)win[2 * r + 1]};
            }
            ds_dft8(v);
            ds_fft_store(S, lane, 1, v);
            __syncthreads();
            ds_fft_load(S, tw1, lane, v);
            __syncthreads();
            ds_dft8(v);
            ds_fft_store(S, lane, 8, v);
            __syncthreads();
            ds_fft_load(S, tw2, lane, v);
            __syncthreads();
            ds_dft8(v);
            ds_fft_store(S, lane, 64, v);
            __syncthreads();
            double m[9];
            cp_split_mag(S, tw4, w256, lane, m);
            __syncthreads();
            if (side == 0) {
#pragma unroll
                for (int i = 0; i < 9; ++i) mb[i] = m[i];
            } else if (valid) {
#pragma unroll
                for (int i = 0; i < 9; ++i) {
                    if (i == 8 && lane != 0) break;
                    const double A = m[i], Bv = mb[i], d = A - Bv;
                    num = fma(d, d, num);
                    den = fma(A, A, den);
                    lg += fabs(log(fmax(A, CP_FLOOR)) - log(fmax(Bv, CP_FLOOR)));
                }
            }
        }
    }
    const double n_ = cp_block_sum(num, sh), d_ = cp_block_sum(den, sh), l_ = cp_block_sum(lg, sh);
    if (tid == 0) {
        double* o = st_part + (((size_t)row * 3 + res) * groups + group) * 3;
        o[0] = n_, o[1] = d_, o[2] = l_;
    }
}

__device__ __forceinline__ double cp_ratio_db(double num, double den) {         // 10 log10(num / den): +inf when den == 0, else -inf when num == 0
    if (den == 0.0) return INFINITY;
    if (num == 0.0) return -INFINITY;
    return 10.0 * log10(num / den);
}

// lanes 0..8: the (resolution, sum) pairs of the STFT partials; lanes 9..11: e_res, e_dif, ea.  Each adds its partials in order.
__global__ __launch_bounds__(64) void ds_compare_finish_kernel(int s0, int s1, int tiles, int groups, const double* __restrict__ sums,
                                                              const double* __restrict__ res_part,
                                                              const double* __restrict__ st_part, double* __restrict__ si_sdr_db,
                                                              double* __restrict__ snr_db, double* __restrict__ sc,
                                                              double* __restrict__ logmag) {
    __shared__ double tot[12];
    const int lane = threadIdx.x, row = blockIdx.x;
    if (lane < 9) {
        const int res = lane / 3, which = lane % 3;
        const int n_frames = (s1 - s0 - cp_win[res]) / cp_hop[res] + 1;
        const int n_groups = (n_frames + CP_FR - 1) / CP_FR;
        const double* p = st_part + ((size_t)row * 3 + res) * groups * 3 + which;
        double s = 0.0;
        for (int g = 0; g < n_groups; ++g) s += p[(size_t)g * 3];
        tot[lane] = s;
    } else if (lane < 12) {
        const double* p = res_part + (size_t)row * tiles * 3 + (lane - 9);
        double s = 0.0;
        for (int t = 0; t < tiles; ++t) s += p[(size_t)t * 3];
        tot[lane] = s;
    }
    __syncthreads();
    if (lane < 3) {
        const int n_frames = (s1 - s0 - cp_win[lane]) / cp_hop[lane] + 1;
        const double num = tot[3 * lane], den = tot[3 * lane + 1];
        sc[3 * row + lane] = num == 0.0 ? 0.0 : (den == 0.0 ? (double)INFINITY : sqrt(num) / sqrt(den));
        logmag[3 * row + lane] = tot[3 * lane + 2] / ((double)n_frames * (double)CP_BINS);
    } else if (lane == 3) {
        const double r = sums[3 * row], ea = sums[3 * row + 1];
        const double alpha = ea == 0.0 ? 0.0 : r / ea;
        si_sdr_db[row] = cp_ratio_db(alpha * alpha * tot[11], tot[9]);
        snr_db[row] = cp_ratio_db(tot[11], tot[10]);
    }
}

__global__ __launch_bounds__(256) void ds_compare_l1_kernel(const float* __restrict__ x, const float* __restrict__ y, long long n,
                                                           double* __restrict__ out) {
    __shared__ double sh[4];
    const int row = blockIdx.x;
    const float* xr = x + (size_t)row * n;
    const float* yr = y + (size_t)row * n;
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) s += fabs((double)xr[i] - (double)yr[i]);
    const double t = cp_block_sum(s, sh);
    if (threadIdx.x == 0) out[row] = t / (double)n;
}

// ---- entries ---------------------------------------------------------------------------------------------------------------
#define CP_CHECK_COMMON()                                                                                                  \
    DS_CHECK_ARG(B >= 1 && B <= 65535 && Na >= 1 && Nb >= 1, "bad sizes");                                                 \
    DS_CHECK_ARG(max_lag >= 0 && max_lag <= CP_MAX_LAG, "max_lag must be in 0..4096");                                     \
    DS_CHECK_ARG(s0 >= 0 && s0 < s1 && s1 <= Nb, "the region [s0, s1) must be non-empty and inside b");                    \
    DS_CHECK_ARG(max_lag == 0 || (s0 - max_lag >= 0 && (long long)s1 + max_lag <= Na),                                     \
                 "the region must leave max_lag samples of a on either side")

#define CP_CHECK_SCRATCH()                                                                                                 \
    const CpLayout l = cp_layout(B, (long long)s1 - s0, max_lag);                                                          \
    DS_CHECK_ARG(scratch_bytes >= l.bytes, "scratch is smaller than ds_compare_scratch_bytes(B, s1 - s0, max_lag)");       \
    DS_CHECK_ARG(((uintptr_t)scratch & 7) == 0, "scratch must be 8-byte aligned")

extern "C" int ds_compare_max_lag(void) { return CP_MAX_LAG; }

extern "C" int64_t ds_compare_scratch_bytes(int B, int n_region, int max_lag) {
    if (B < 1 || n_region < 1 || max_lag < 0 || max_lag > CP_MAX_LAG) return -1;
    return cp_layout(B, n_region, max_lag).bytes;
}

extern "C" int ds_compare_align(const float* a, const float* b, int B, int Na, int Nb, int s0, int s1, int max_lag,
                                const int32_t* lag_dev, int lag, void* scratch, int64_t scratch_bytes, int32_t* lag_out,
                                double* rho, double* sums, ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(a && b && scratch && lag_out && rho && sums, "null pointer");
    CP_CHECK_COMMON();
    DS_CHECK_ARG(max_lag == 0 || (!lag_dev && lag == 0), "a given lag skips the search: max_lag must be 0 with it");
    DS_CHECK_ARG(lag_dev || ((long long)s0 + lag >= 0 && (long long)s1 + lag <= Na), "the region shifted by lag must be inside a");
    CP_CHECK_SCRATCH();
    char* sc = (char*)scratch;
    double* part = (double*)(sc + l.off_part);
    double* eb_part = (double*)(sc + l.off_eb);
    if (lag_dev || lag != 0) {                                                   // a given lag (max_lag == 0): no search is launched
        hipLaunchKernelGGL(ds_xcorr_given_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, B, lag_dev, lag, lag_out);
    } else {
        hipLaunchKernelGGL(ds_xcorr_partials_kernel, dim3((unsigned)l.tiles, (unsigned)l.chunks, B), dim3(256), 0, stream, a, b, Na,
                           Nb, s0, s1, max_lag, lag_dev, lag, (int)l.tiles, (int)l.lp, part, eb_part);
        hipLaunchKernelGGL(ds_xcorr_select_kernel, dim3(B), dim3(64), 0, stream, max_lag, lag_dev, lag, (int)l.tiles, (int)l.lp,
                           part, eb_part, lag_out, rho, sums);
    }
    hipLaunchKernelGGL(ds_xcorr_refine_kernel, dim3(B), dim3(256), 0, stream, a, b, Na, Nb, s0, s1, lag_out, rho, sums);
    DS_CHECK_LAUNCH();
    return 0;
}

extern "C" int ds_compare_residual(const float* a, const float* b, int B, int Na, int Nb, int s0, int s1, int max_lag,
                                   const int32_t* lag, const double* sums, void* scratch, int64_t scratch_bytes,
                                   ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(a && b && lag && sums && scratch, "null pointer");
    CP_CHECK_COMMON();
    CP_CHECK_SCRATCH();
    hipLaunchKernelGGL(ds_compare_residual_kernel, dim3((unsigned)l.tiles, B), dim3(256), 0, stream, a, b, Na, Nb, s0, s1, lag, sums,
                       (int)l.tiles, (double*)((char*)scratch + l.off_res));
    DS_CHECK_LAUNCH();
    return 0;
}

extern "C" int ds_compare_stft(const float* a, const float* b, int B, int Na, int Nb, int s0, int s1, int max_lag,
                               const int32_t* lag, const float* windows, const double* twiddle, void* scratch,
                               int64_t scratch_bytes, ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(a && b && lag && windows && twiddle && scratch, "null pointer");
    CP_CHECK_COMMON();
    DS_CHECK_ARG(s1 - s0 >= CP_NFFT, "the region must hold at least 1024 samples");
    CP_CHECK_SCRATCH();
    hipLaunchKernelGGL(ds_stft_compare_kernel, dim3((unsigned)l.groups, 3, B), dim3(256), 0, stream, a, b, Na, Nb, s0, s1, lag,
                       windows, reinterpret_cast<const ds_cf*>(twiddle), (int)l.groups, (double*)((char*)scratch + l.off_st));
    DS_CHECK_LAUNCH();
    return 0;
}

extern "C" int ds_compare_finish(int B, int s0, int s1, int max_lag, const double* sums, const void* scratch,
                                 int64_t scratch_bytes, double* si_sdr_db, double* snr_db, double* sc, double* logmag,
                                 ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(sums && scratch && si_sdr_db && snr_db && sc && logmag, "null pointer");
    DS_CHECK_ARG(B >= 1 && B <= 65535, "bad sizes");
    DS_CHECK_ARG(max_lag >= 0 && max_lag <= CP_MAX_LAG, "max_lag must be in 0..4096");
    DS_CHECK_ARG(s0 >= 0 && s0 < s1, "the region [s0, s1) must be non-empty");
    DS_CHECK_ARG(s1 - s0 >= CP_NFFT, "the region must hold at least 1024 samples");
    CP_CHECK_SCRATCH();
    const char* sc_ = (const char*)scratch;
    hipLaunchKernelGGL(ds_compare_finish_kernel, dim3(B), dim3(64), 0, stream, s0, s1, (int)l.tiles, (int)l.groups, sums,
                       (const double*)(sc_ + l.off_res), (const double*)(sc_ + l.off_st), si_sdr_db, snr_db, sc, logmag);
    DS_CHECK_LAUNCH();
    return 0;
}

extern "C" int ds_compare_l1(const float* x, const float* y, int B, int64_t n, double* out, ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(x && y && out, "null pointer");
    DS_CHECK_ARG(B >= 1 && B <= 65535 && n >= 1, "bad sizes");
    hipLaunchKernelGGL(ds_compare_l1_kernel, dim3(B), dim3(256), 0, stream, x, y, (long long)n, out);
    DS_CHECK_LAUNCH();
    return 0;
}
