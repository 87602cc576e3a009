// Waveform -> log-mel spectrogram in ONE launch (ds_wave_to_mel): reflect padding, Hann-windowed 1024-point STFT at hop 256,
// magnitude, mel filterbank, log10, affine and clip, frame crop.  Replaces the host-side librosa chain of
// vocoder/mel2wav/extract_mel_spectrogram.py:15-38,141-187 and the torch chain of vocoder/modules.py:54-69 (Audio2Mel.forward).
//
// A workgroup (4 waves) takes SM_FR consecutive frames of one clip:
//   1. the (SM_FR - 1) * 256 + 1024 samples they cover are staged in LDS once -- reflection, zero extension and truncation are
//      index arithmetic in this loader, the 4x frame overlap is served from LDS;
//   2. each wave transforms SM_FR / 4 frames, one at a time: real-input FFT = 512-point complex radix-8 Stockham in LDS + split
//      (stft_mel_fft.h), twiddles and window from float64-built tables held in registers; 513 fp32 magnitudes per frame -> LDS;
//   3. thread (mel group g = tid / SM_FR, frame = tid % SM_FR) accumulates rows g, g + 256 / SM_FR, .. of the filterbank over the
//      row's non-zero range [k0, k1) in ascending k -- a fixed order, so a clip's result does not depend on the batch around
//      it -- and stores out[b][j][frame]: SM_FR consecutive frames = one segment per row.
// Nothing but the input and the output touches HBM.
//
// The FFT runs in DOUBLE.  An fp32 FFT leaves an absolute error of ~eps x (the largest line of the frame) in EVERY bin, and
// log10 turns that into a large error wherever a band sits far below a line of the same frame: Audio2Mel on a 0.8-amplitude
// chirp is 3.7e-3 from the float64 formula with an fp32 FFT (stock torch in fp32: 4.4e-3), against a tolerance of 1e-3.  In
// double the FFT's own error vanishes and what remains is the fp32 rounding of the inputs (the f32 window buffer: 3e-4 on
// that chirp).  gfx950 issues v_fma_f64 / v_add_f64 at the rate of the unpacked fp32 forms, so the cost is LDS bytes and
// registers, not arithmetic.  The squared magnitude is rounded to fp32 once (a relative error, harmless under the log); the
// filterbank sum, log10, affine and clip are fp32.
#include <hip/hip_runtime.h>

#include "common.h"
#include "diffsound_hip.h"
#include "stft_mel_fft.h"

#ifndef SM_FR
#define SM_FR 8                                // frames per workgroup (8 or 16; measured at B = 64: 207 us against 288 us)
#endif
#define SM_NS ((SM_FR - 1) * 256 + 1024)       // staged samples
#define SM_MP 513                              // magnitude row pitch: = 1 mod 64, so SM_FR frames x one k hit SM_FR banks
#define SM_SCRATCH_BYTES (4 * DS_FFT_SCRATCH * (int)sizeof(ds_cf))
#define SM_LDS_BYTES (SM_SCRATCH_BYTES + (SM_NS + SM_FR * SM_MP) * 4)
static_assert(SM_FR == 8 || SM_FR == 16, "a wave transforms SM_FR / 4 frames; the store mapping needs a power of two");

DS_FFT_DEV float ds_fft_sqrt(float x) { return __fsqrt_rn(x); }

__global__ __launch_bounds__(256) void ds_wave_to_mel_kernel(
    const float* __restrict__ wave, int T, int L, int pad, const float* __restrict__ window, const ds_cf* __restrict__ tw,
    const float* __restrict__ basis, const int* __restrict__ krange, int n_mels, float* __restrict__ out, int f0, int n_out,
    float a, float c, float lo, float hi, float floor_) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    ds_cf* S = reinterpret_cast<ds_cf*>(smem) + wid * DS_FFT_SCRATCH;  // [4 waves][DS_FFT_SCRATCH]
    float* xs = reinterpret_cast<float*>(smem + SM_SCRATCH_BYTES);     // [SM_NS]
    float* mag = xs + SM_NS;                                           // [SM_FR][SM_MP]
    const int b = blockIdx.y;
    const int fbase = f0 + blockIdx.x * SM_FR;                         // first frame of this tile

    // 1. stage: padded index i -> source sample s (numpy "reflect": the edge sample is not repeated); pad < L, so one fold
    //    suffices.  Past the clip's T samples the wave is zero-extended to L; past the padded wave (frames of the last tile
    //    that do not exist) zeros too.
    const float* wb = wave + (size_t)b * T;
    const int start = fbase * 256, padded = L + 2 * pad;
    for (int i = tid; i < SM_NS; i += 256) {
        const int gi = start + i;
        float val = 0.f;
        if (gi < padded) {
            int s = gi - pad;
            if (s < 0) s = -s;
            if (s >= L) s = 2 * (L - 1) - s;
            if (s < T) val = wb[s];
        }
        xs[i] = val;
    }

    // the lane's constants: 16 window values, 7 + 7 pass twiddles (tw[0..512) = e^{-2 pi i m / 512}), 4 split twiddles
    // (tw[512 + k] = e^{-2 pi i k / 1024}, k <= 256)
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
    __syncthreads();

    // 2. SM_FR / 4 frames per wave.  The scratch S is private to the wave; the workgroup barriers order its loads and stores
    //    (every wave runs the same iterations).
    for (int it = 0; it < SM_FR / 4; ++it) {
        const int fl = it * 4 + wid;
        ds_cf v[8];
        ds_fft_load_frame(xs + fl * 256, win, lane, v);
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
        ds_fft_split_mag(S, tw4, w256, lane, mag + fl * SM_MP);
        __syncthreads();
    }

    // 3. filterbank, log, affine, clip, store
    const int fl = tid & (SM_FR - 1), g = tid / SM_FR;
    const int fo = blockIdx.x * SM_FR + fl;                            // output frame index (f - f0)
    const float* mrow = mag + fl * SM_MP;
    for (int j = g; j < n_mels; j += 256 / SM_FR) {
        int k0 = 0, k1 = 513;
        if (krange) {
            k0 = max(krange[2 * j], 0);
            k1 = min(krange[2 * j + 1], 513);
        }
        const float* brow = basis + (size_t)j * 513;
        float acc = 0.f;
        for (int k = k0; k < k1; ++k) acc = fmaf(brow[k], mrow[k], acc);
        const float y = fminf(fmaxf(fmaf(a, log10f(fmaxf(acc, floor_)), c), lo), hi);
        if (fo < n_out) out[((size_t)b * n_mels + j) * n_out + fo] = y;
    }
}

extern "C" int ds_wave_to_mel(const float* wave, int B, int T, int length, int pad, const float* window, const double* twiddle,
                              const float* mel_basis, const int32_t* krange, int n_mels, int n_fft, int hop, int f0, int n_out,
                              float a, float c, float lo, float hi, float floor, float* out, ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(wave && window && twiddle && mel_basis && out, "null pointer");
    DS_CHECK_ARG(n_fft == 1024 && hop == 256, "only n_fft = 1024, hop = 256 is built");
    DS_CHECK_ARG(n_mels >= 1 && n_mels <= 128, "n_mels must be in 1..128");
    DS_CHECK_ARG(B >= 1 && B <= 65535 && T >= 1 && length >= 0 && pad >= 0, "bad sizes");
    const long long L = length ? length : T;
    DS_CHECK_ARG(pad < L, "wave too short to reflect (pad must be < its length)");
    DS_CHECK_ARG(L + 2ll * pad >= 1024 && L + 2ll * pad + SM_NS < (1ll << 31), "padded length must be in 1024 .. 2^31");
    const long long frames = 1 + (L + 2ll * pad - 1024) / 256;
    DS_CHECK_ARG(f0 >= 0 && n_out >= 1 && (long long)f0 + n_out <= frames, "frame crop [f0, f0 + n_out) out of range");
    DS_CHECK_ARG(floor > 0.f && lo <= hi, "floor must be > 0 and lo <= hi");
    static DsOnce attr_set;
    if (attr_set.need()) {
        hipError_t e = hipFuncSetAttribute((const void*)ds_wave_to_mel_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           SM_LDS_BYTES);
        if (e != hipSuccess) {
            ds_set_error("ds_wave_to_mel: hipFuncSetAttribute: %s", hipGetErrorString(e));
            return -2;
        }
        attr_set.done();
    }
    hipLaunchKernelGGL(ds_wave_to_mel_kernel, dim3((n_out + SM_FR - 1) / SM_FR, B), dim3(256), SM_LDS_BYTES, stream, wave, T,
                       (int)L, pad, window, reinterpret_cast<const ds_cf*>(twiddle), mel_basis, krange, n_mels, out, f0, n_out,
                       a, c, lo, hi, floor);
    DS_CHECK_LAUNCH();
    return 0;
}
