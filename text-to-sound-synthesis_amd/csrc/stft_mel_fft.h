// Per-lane arithmetic of the 1024-point real-input FFT of stft_mel.hip, in double (stft_mel.hip says why): one wave (64
// lanes) transforms one frame as a 512-point complex FFT of z[n] = x[2n] + i x[2n+1] -- three radix-8 Stockham passes, lane j owning butterfly j of each --
// followed by the real-input split.  Plain C++ on purpose (no HIP types): the same text compiles for the host, where a loop
// over 64 "lanes" checks it against a float64 DFT.
//
// Pass with stride Ns (1, 8, 64), butterfly j:   v[r] = in[j + 64 r] * W512^((j mod Ns) r (64 / Ns)),  V = DFT8(v),
//                                                out[(j / Ns) 8 Ns + (j mod Ns) + q Ns] = V[q]
// so the twiddles of a lane are the same for every frame (held in registers), and pass 0 has none.
#ifndef DS_STFT_MEL_FFT_H
#define DS_STFT_MEL_FFT_H

#ifndef DS_FFT_DEV
#define DS_FFT_DEV __device__ __forceinline__
#endif

template <typename T>
struct alignas(2 * sizeof(T)) ds_cx {
    T x, y;
};
typedef ds_cx<double> ds_cf;   // the kernel's working precision (stft_mel.hip says why it is not float)
typedef double ds_fs;

// LDS image of the 512 complex points (16 bytes each): one pad slot after every 8, so that the stride-8 stores of pass 0
// (lane j writes points 8 j + q: 9 slots between lanes instead of 8) spread over the banks like the stride-1 loads do.
#define DS_FFT_ZP(p) ((p) + ((p) >> 3))
#define DS_FFT_SCRATCH 576   // ds_cf slots (16 bytes each) per wave: DS_FFT_ZP(511) + 1 = 575, rounded up

DS_FFT_DEV ds_cf ds_cf_add(ds_cf a, ds_cf b) { return ds_cf{a.x + b.x, a.y + b.y}; }
DS_FFT_DEV ds_cf ds_cf_sub(ds_cf a, ds_cf b) { return ds_cf{a.x - b.x, a.y - b.y}; }
DS_FFT_DEV ds_cf ds_cf_mul(ds_cf a, ds_cf b) { return ds_cf{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
DS_FFT_DEV ds_cf ds_cf_mul_mi(ds_cf a) { return ds_cf{a.y, -a.x}; }   // a * (-i)

// V[q] = sum_r v[r] e^{-2 pi i r q / 8}, in place: two DFT4 (even / odd inputs) and the last radix-2 stage
DS_FFT_DEV void ds_dft8(ds_cf* v) {
    const ds_fs h = 0.70710678118654752440;
    const ds_cf a0 = ds_cf_add(v[0], v[4]), a1 = ds_cf_sub(v[0], v[4]);
    const ds_cf a2 = ds_cf_add(v[2], v[6]), a3 = ds_cf_mul_mi(ds_cf_sub(v[2], v[6]));
    const ds_cf a4 = ds_cf_add(v[1], v[5]), a5 = ds_cf_sub(v[1], v[5]);
    const ds_cf a6 = ds_cf_add(v[3], v[7]), a7 = ds_cf_mul_mi(ds_cf_sub(v[3], v[7]));
    const ds_cf b0 = ds_cf_add(a0, a2), b2 = ds_cf_sub(a0, a2), b1 = ds_cf_add(a1, a3), b3 = ds_cf_sub(a1, a3);
    const ds_cf b4 = ds_cf_add(a4, a6), b6 = ds_cf_mul_mi(ds_cf_sub(a4, a6));
    const ds_cf s5 = ds_cf_add(a5, a7), d7 = ds_cf_sub(a5, a7);
    const ds_cf b5 = ds_cf{(s5.x + s5.y) * h, (s5.y - s5.x) * h};      // * e^{-i pi / 4}
    const ds_cf b7 = ds_cf{(d7.y - d7.x) * h, -(d7.x + d7.y) * h};     // * e^{-3 i pi / 4}
    v[0] = ds_cf_add(b0, b4); v[4] = ds_cf_sub(b0, b4);
    v[1] = ds_cf_add(b1, b5); v[5] = ds_cf_sub(b1, b5);
    v[2] = ds_cf_add(b2, b6); v[6] = ds_cf_sub(b2, b6);
    v[3] = ds_cf_add(b3, b7); v[7] = ds_cf_sub(b3, b7);
}

// pass 0 input: the frame's 1024 staged samples times the lane's 16 window values (win[2 r], win[2 r + 1] = window[2 (lane + 64 r)],
// window[2 (lane + 64 r) + 1]); 8-byte loads, consecutive over the lanes
DS_FFT_DEV void ds_fft_load_frame(const float* frame, const float* win, int lane, ds_cf* v) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const ds_cx<float> s = *reinterpret_cast<const ds_cx<float>*>(frame + 2 * (lane + 64 * r));
        v[r] = ds_cf{(ds_fs)s.x * (ds_fs)win[2 * r], (ds_fs)s.y * (ds_fs)win[2 * r + 1]};   // exact products in double
    }
}

// input of passes 1 and 2: tw[r - 1] = W512^((lane mod Ns) r (64 / Ns))
DS_FFT_DEV void ds_fft_load(const ds_cf* S, const ds_cf* tw, int lane, ds_cf* v) {
    v[0] = S[DS_FFT_ZP(lane)];
#pragma unroll
    for (int r = 1; r < 8; ++r) v[r] = ds_cf_mul(S[DS_FFT_ZP(lane + 64 * r)], tw[r - 1]);
}

DS_FFT_DEV void ds_fft_store(ds_cf* S, int lane, int Ns, const ds_cf* v) {
    const int j0 = (lane / Ns) * Ns * 8 + (lane % Ns);
#pragma unroll
    for (int q = 0; q < 8; ++q) S[DS_FFT_ZP(j0 + q * Ns)] = v[q];
}

DS_FFT_DEV float ds_fft_sqrt(float x);   // correctly rounded fp32 square root (the kernel: __fsqrt_rn; the host check: sqrtf)

// Real-input split: with A = Z[k], B = conj(Z[512 - k]), E = A + B, O = -i (A - B) and w = e^{-2 pi i k / 1024}:
// |X[k]| = |E + w O| / 2 and |X[512 - k]| = |E - w O| / 2.  The lane takes k = lane + 64 i (tw4[i] = w, i < 4), lane 0
// also k = 256 (w256).  mag: the frame's 513 magnitudes.
DS_FFT_DEV void ds_fft_split_mag(const ds_cf* S, const ds_cf* tw4, ds_cf w256, int lane, float* mag) {
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        if (i == 4 && lane != 0) break;
        const int k = i < 4 ? lane + 64 * i : 256;
        const ds_cf w = i < 4 ? tw4[i] : w256;
        const ds_cf A = S[DS_FFT_ZP(k)];
        const ds_cf Zm = S[DS_FFT_ZP((512 - k) & 511)];
        const ds_cf E = ds_cf{A.x + Zm.x, A.y - Zm.y};
        const ds_cf D = ds_cf{A.x - Zm.x, A.y + Zm.y};      // A - B
        const ds_cf wO = ds_cf_mul(w, ds_cf_mul_mi(D));
        const ds_cf p = ds_cf_add(E, wO), m = ds_cf_sub(E, wO);
        // the squared magnitude is rounded to fp32 once; its root then carries fp32's RELATIVE error, which the log keeps small
        mag[k] = 0.5f * ds_fft_sqrt((float)(p.x * p.x + p.y * p.y));
        mag[512 - k] = 0.5f * ds_fft_sqrt((float)(m.x * m.x + m.y * m.y));
    }
}

#endif
