// Pasting a recording back over a rendering of it (include/diffsound_hip.h: ds_paste_*): outside the regenerated spans the
// recording's own values -- waveform samples, or frames of its mel image -- replace the decoder's / the vocoder's, with a
// cross-fade that lies wholly inside the regenerated columns, and one gain per clip on the rendering, taken from the kept
// region where both signals describe the same sound.
//
// Both kernels stream: ds_paste reads 4 + 4 bytes and writes 4 per position at most (a group of four positions that is all
// kept never loads the rendering, one that is all regenerated never loads the recording), ds_paste_sums reads 8 per kept
// position.  A thread owns four consecutive positions.  ds_paste lays its groups on the 16-byte grid of the OUTPUT row's
// address, so every full group is one 16-byte store whatever the row stride (T is odd at 48 kHz); the ragged positions at a
// row's two ends are stored one by one.  The recording is read at n + off and the offset is arbitrary (1408, 3065, ..), so
// its address has no alignment to build on: a group's four values are taken from the two ALIGNED 16-byte chunks that hold
// them and picked by the shift (address / 4) mod 4 -- two wide coalesced loads of which the second is a neighbour lane's
// first, instead of four 4-byte loads --, and only where both chunks lie inside the row's valid range [0, len); the few
// groups at a row's ends, and everything outside the recording (which reads as +0), go element by element with bounds.
// Values are moved as 32-bit words: a kept position is a COPY of the recording's bits, NaN payloads included.
//
// The column of position n is c = min(n col_den div col_num, n_cols - 1) in int64 (one division per group, then exact
// comparisons), so kept / regenerated is classified exactly; distances to a column edge are (integer numerator) / col_den in
// float64, the numerator exact.  sin / cos are evaluated only where 0 < u < 1 (as sinpi / cospi of u / 2: no reduction).
//
// The sums are float64 over a fixed partition: a workgroup owns PS_CHUNK consecutive positions, a thread adds its own in
// index order, the 256 threads are joined by a fixed tree, and one wave adds a row's chunk sums in a fixed order.  Nothing is
// atomic; a row's sums depend on that row alone and have the same bits whatever the batch, the row stride and the launch.
#include <hip/hip_runtime.h>

#include <math.h>

#include "common.h"
#include "diffsound_hip.h"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

#define PS_CHUNK 8192               // positions per workgroup of the sums kernel: 256 threads x 8 groups of 4

// v[0..4) = row[i0 .. i0 + 4) as 32-bit words; an index outside [0, len) reads as +0 and is never loaded
__device__ __forceinline__ void ps_load4(const unsigned* __restrict__ row, long long i0, long long len, unsigned v[4]) {
    const unsigned* p = row + i0;
    const int s = (int)(((uintptr_t)p >> 2) & 3);
    if (i0 - s >= 0 && i0 - s + (s ? 8 : 4) <= len) {                   // the aligned chunk(s) lie inside the row
        const u32x4 a = *(const u32x4*)(p - s);
        if (s == 0) {
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
        } else {
            const u32x4 b = *(const u32x4*)(p - s + 4);
            v[0] = s == 1 ? a.y : s == 2 ? a.z : a.w;
            v[1] = s == 1 ? a.z : s == 2 ? a.w : b.x;
            v[2] = s == 1 ? a.w : s == 2 ? b.x : b.y;
            v[3] = s == 1 ? b.x : s == 2 ? b.y : b.z;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (i0 + k >= 0 && i0 + k < len) ? p[k] : 0u;
    }
}

// the column of position n, walked on from a column c that is not past it
__device__ __forceinline__ long long ps_column(long long c, long long n, int n_cols, long long col_num, long long col_den) {
    while (c < n_cols - 1 && n * col_den >= (c + 1) * col_num) ++c;
    return c;
}

// u of position n in column c: 0 in a kept column, 1 outside every fade, else min(1, distance to the nearest kept neighbour's
// edge / fade_len)
__device__ __forceinline__ double ps_weight(const unsigned char* __restrict__ kp, int n_cols, long long c, long long n,
                                            long long col_num, long long col_den, double fade_len) {
    if (kp[c]) return 0.0;
    if (fade_len == 0.0) return 1.0;
    const bool left = c > 0 && kp[c - 1], right = c < n_cols - 1 && kp[c + 1];
    if (!left && !right) return 1.0;
    double d = INFINITY;
    if (left) d = (double)(n * col_den - c * col_num) / (double)col_den;
    if (right) d = fmin(d, (double)((c + 1) * col_num - n * col_den) / (double)col_den);
    return fmin(1.0, d / fade_len);
}

__device__ __forceinline__ double ps_gain(const double* __restrict__ sums, int b) {
    if (!sums) return 1.0;
    const double so = sums[2 * b], sr = sums[2 * b + 1];
    if (!(so > 0.0) || !(sr > 0.0) || !(so < INFINITY) || !(sr < INFINITY)) return 1.0;
    return fmin(fmax(sqrt(so / sr), 0.25), 4.0);
}

__global__ __launch_bounds__(256) void ds_paste_kernel(const unsigned* ren, const unsigned* __restrict__ rec, unsigned* out, int C,
                                                      int T, int Tr, const long long* __restrict__ off,
                                                      const int* __restrict__ rec_len, const unsigned char* __restrict__ keep,
                                                      int n_cols, long long col_num, long long col_den, double fade_len,
                                                      int curve, const double* __restrict__ sums) {
    const int row = blockIdx.y, b = row / C;
    const unsigned* renr = ren + (size_t)row * T;
    const unsigned* recr = rec + (size_t)row * Tr;
    unsigned* outr = out + (size_t)row * T;
    const int s_out = (int)(((uintptr_t)outr >> 2) & 3);
    const long long n0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4 - s_out;   // outr + n0 is 16-byte aligned
    if (n0 >= T) return;
    const long long o = off[b];
    const long long len = rec_len ? min(max(rec_len[b], 0), Tr) : Tr;
    const unsigned char* kp = keep + (size_t)b * n_cols;
    const long long nf = n0 > 0 ? n0 : 0;
    long long c = min(nf * col_den / col_num, (long long)n_cols - 1);
    double u[4];
    bool need_rec = false, need_ren = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long n = n0 + k;
        u[k] = 0.0;
        if (n < 0 || n >= T) continue;
        c = ps_column(c, n, n_cols, col_num, col_den);
        u[k] = ps_weight(kp, n_cols, c, n, col_num, col_den, fade_len);
        need_rec |= u[k] < 1.0;
        need_ren |= u[k] > 0.0;
    }
    unsigned r[4] = {0u, 0u, 0u, 0u}, x[4] = {0u, 0u, 0u, 0u}, y[4];
    if (need_ren) ps_load4(renr, n0, T, r);
    if (need_rec) ps_load4(recr, n0 + o, len, x);
    const double g = ps_gain(sums, b);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (u[k] == 0.0) {
            y[k] = x[k];                                                 // a copy, whatever the rendering holds
        } else if (u[k] == 1.0) {
            y[k] = sums ? __float_as_uint((float)(g * (double)__uint_as_float(r[k]))) : r[k];
        } else {
            const double gr = g * (double)__uint_as_float(r[k]), xo = (double)__uint_as_float(x[k]);
            const double wr = curve == DS_PASTE_EQUAL_POWER ? sinpi(0.5 * u[k]) : u[k];
            const double wo = curve == DS_PASTE_EQUAL_POWER ? cospi(0.5 * u[k]) : 1.0 - u[k];
            y[k] = __float_as_uint((float)(gr * wr + xo * wo));
        }
    }
    if (n0 >= 0 && n0 + 4 <= T) {
        *(u32x4*)(outr + n0) = u32x4{y[0], y[1], y[2], y[3]};
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (n0 + k >= 0 && n0 + k < T) outr[n0 + k] = y[k];
    }
}

// part[b][chunk] = { sum rec^2, sum ren^2 } over the chunk's kept positions whose recording index is in range
__global__ __launch_bounds__(256) void ds_paste_partial_kernel(const unsigned* __restrict__ ren, const unsigned* __restrict__ rec,
                                                              int T, int Tr, const long long* __restrict__ off,
                                                              const int* __restrict__ rec_len,
                                                              const unsigned char* __restrict__ keep, int n_cols,
                                                              long long col_num, long long col_den, int chunks,
                                                              double* __restrict__ part) {
    __shared__ double sh[2][256];
    const int tid = threadIdx.x, b = blockIdx.y;
    const unsigned* renr = ren + (size_t)b * T;
    const unsigned* recr = rec + (size_t)b * Tr;
    const long long o = off[b];
    const long long len = rec_len ? min(max(rec_len[b], 0), Tr) : Tr;
    const unsigned char* kp = keep + (size_t)b * n_cols;
    double so = 0.0, sr = 0.0;
    for (int j = 0; j < PS_CHUNK / 1024; ++j) {
        const long long n0 = (long long)blockIdx.x * PS_CHUNK + ((long long)j * 256 + tid) * 4;
        if (n0 >= T) break;
        long long c = min(n0 * col_den / col_num, (long long)n_cols - 1);
        bool in[4], any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long n = n0 + k;
            c = ps_column(c, n, n_cols, col_num, col_den);
            in[k] = n < T && kp[c] && n + o >= 0 && n + o < len;
            any |= in[k];
        }
        if (!any) continue;
        unsigned r[4], x[4];
        ps_load4(renr, n0, T, r);
        ps_load4(recr, n0 + o, len, x);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!in[k]) continue;
            const double xv = (double)__uint_as_float(x[k]), rv = (double)__uint_as_float(r[k]);
            so += xv * xv;                                               // exact products: only the additions round
            sr += rv * rv;
        }
    }
    sh[0][tid] = so, sh[1][tid] = sr;
    for (int s = 128; s > 0; s >>= 1) {                                  // a fixed tree
        __syncthreads();
        if (tid < s) sh[0][tid] += sh[0][tid + s], sh[1][tid] += sh[1][tid + s];
    }
    if (tid == 0) {
        double* p = part + ((size_t)b * chunks + blockIdx.x) * 2;
        p[0] = sh[0][0], p[1] = sh[1][0];
    }
}

// sums[b] = a row's chunk sums: lane l adds chunks l, l + 64, .. in order, then the 64 lanes are added in lane order
__global__ __launch_bounds__(64) void ds_paste_finish_kernel(const double* __restrict__ part, int chunks, double* __restrict__ sums) {
    __shared__ double sh[2][64];
    const int lane = threadIdx.x, b = blockIdx.x;
    double so = 0.0, sr = 0.0;
    for (int j = lane; j < chunks; j += 64) {
        const double* p = part + ((size_t)b * chunks + j) * 2;
        so += p[0], sr += p[1];
    }
    sh[0][lane] = so, sh[1][lane] = sr;
    __syncthreads();
    if (lane == 0) {
        so = 0.0, sr = 0.0;
        for (int i = 0; i < 64; ++i) so += sh[0][i], sr += sh[1][i];
        sums[2 * b] = so, sums[2 * b + 1] = sr;
    }
}

static int ps_chunks(int T) {
    return (int)(((long long)T + PS_CHUNK - 1) / PS_CHUNK);
}

extern "C" int64_t ds_paste_scratch_bytes(int B, int T) {
    if (B < 1 || T < 1) return -1;
    return (int64_t)B * ps_chunks(T) * 2 * (int64_t)sizeof(double);
}

extern "C" int ds_paste_sums(const float* ren, const float* rec, int B, int T, int Tr, const int64_t* off, const int32_t* rec_len,
                             const uint8_t* keep_cols, int n_cols, int64_t col_num, int64_t col_den, void* scratch,
                             int64_t scratch_bytes, double* sums, ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(ren && rec && off && keep_cols && scratch && sums, "null pointer");
    DS_CHECK_ARG(B >= 1 && B <= 65535 && T > 0 && Tr >= 0, "bad sizes");
    DS_CHECK_ARG(n_cols >= 1, "n_cols must be >= 1");
    DS_CHECK_ARG(col_num >= 1 && col_den >= 1 && col_num <= INT32_MAX && col_den <= INT32_MAX,
                 "col_num and col_den must be in 1 .. 2^31 - 1");
    DS_CHECK_ARG(scratch_bytes >= ds_paste_scratch_bytes(B, T), "scratch is smaller than ds_paste_scratch_bytes(B, T)");
    DS_CHECK_ARG(((uintptr_t)scratch & 7) == 0, "scratch must be 8-byte aligned");
    const int chunks = ps_chunks(T);
    hipLaunchKernelGGL(ds_paste_partial_kernel, dim3(chunks, B), dim3(256), 0, stream, (const unsigned*)ren, (const unsigned*)rec,
                       T, Tr, (const long long*)off, rec_len, keep_cols, n_cols, (long long)col_num, (long long)col_den, chunks,
                       (double*)scratch);
    hipLaunchKernelGGL(ds_paste_finish_kernel, dim3(B), dim3(64), 0, stream, (const double*)scratch, chunks, sums);
    DS_CHECK_LAUNCH();
    return 0;
}

extern "C" int ds_paste(const float* ren, const float* rec, float* out, int B, int C, int T, int Tr, const int64_t* off,
                        const int32_t* rec_len, const uint8_t* keep_cols, int n_cols, int64_t col_num, int64_t col_den,
                        double fade_len, int curve, const double* sums, ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(ren && rec && out && off && keep_cols, "null pointer");
    DS_CHECK_ARG(B >= 1 && C >= 1 && (long long)B * C <= 65535 && T > 0 && Tr >= 0, "bad sizes");
    DS_CHECK_ARG(n_cols >= 1, "n_cols must be >= 1");
    DS_CHECK_ARG(col_num >= 1 && col_den >= 1 && col_num <= INT32_MAX && col_den <= INT32_MAX,
                 "col_num and col_den must be in 1 .. 2^31 - 1");
    DS_CHECK_ARG(fade_len >= 0.0 && fade_len < INFINITY, "fade_len must be finite and >= 0");
    DS_CHECK_ARG(curve == DS_PASTE_EQUAL_POWER || curve == DS_PASTE_LINEAR, "unknown curve");
    DS_CHECK_ARG(!sums || curve == DS_PASTE_EQUAL_POWER, "sums (a gain) go with the equal-power curve");
    DS_CHECK_ARG(rec != out, "out must not be rec");
    const unsigned gx = (unsigned)(((long long)T + 3 + 1023) / 1024);      // groups start up to 3 positions before the row
    hipLaunchKernelGGL(ds_paste_kernel, dim3(gx, B * C), dim3(256), 0, stream, (const unsigned*)ren, (const unsigned*)rec,
                       (unsigned*)out, C, T, Tr, (const long long*)off, rec_len, keep_cols, n_cols, (long long)col_num,
                       (long long)col_den, fade_len, curve, sums);
    DS_CHECK_LAUNCH();
    return 0;
}
