// The per-column tail of one reverse-diffusion step, fused into one kernel (one wavefront per
// grid position (b, pos); K codes = NPL*64 so each lane owns NPL classes; [MASK] is class K):
//
//   predict_start      diffusion_transformer.py:285-289   log_softmax in float64 -> f32, -70 row, clamp
//   top-r truncation   models/dalle_spec.py:158-174       keep class iff mass ranked before it < r
//   q_posterior        diffusion_transformer.py:293-339   (+ q_pred :253-267, q_pred_one_timestep
//                                                          :241-251, log_add_exp :28-30)
//   log_sample_categorical  :359-368                      Gumbel-argmax with the caller's uniforms
//
// State between steps is the token index, not the reference's 272 KB/sample log-one-hot: the
// log-one-hot is only ever consumed through argmax / q_pred / q_pred_one_timestep, which need
// {0 at x_t, log(1e-30) elsewhere}; the all-[MASK] start state is {0, -inf} (:633-636) and is
// flagged by `initial`.
//
// The reference sorts each column (2 sorts + cumsum + gather); here the "mass ranked before me"
// is an O(K^2/64) compare-and-add per lane against an LDS copy of the column -- 66k flops per
// column, nothing next to the 155 GFLOP transformer step, and no sort network.
// Noise is read in the reference's own [B, K+1, L] layout so that torch.rand_like on the same
// shape reproduces the reference's RNG stream -- or (the *_rng entries) drawn inside the kernel from a counter-based
// Philox4x32-10 stream keyed by (seed; global caption id, sampler call, grid position, class): the draw of a caption
// then depends neither on the batch it is in, nor on its position in it, nor on the rank that runs it (SURVEY.md
// section 8e: "generate the noise per sample, seeded by global caption index"), no [B][K+1][L] tensor of uniforms
// exists, and a whole reverse chain can be enqueued without returning to the host (api.hip ds_denoiser_sample_rng).
#include "sampler.h"

// ---- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants) ----
// counter (c0, c1, c2, c3), key (k0, k1) -> four 32-bit words.  Host mirror: text_to_sound_synthesis_amd/shard.py
// philox4x32_10 / caption_uniforms (numpy), checked against the published known-answer vectors in tests/.
typedef unsigned ds_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ ds_u32x4 ds_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                                      unsigned k1) {
    asm volatile("" : "+v"(k0), "+v"(k1), "+v"(c1), "+v"(c2), "+v"(c3));   // everything in VGPRs: scalar rounds push the sampler kernel past its SGPRs
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const unsigned lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return ds_u32x4{c0, c1, c2, c3};
}
// The uniform of class c = 64 j + lane (j = c >> 6; the [MASK] class K is j = K / 64, lane 0) at grid position pos of
// caption gid in sampler call `call` of stream `sid` (0: reverse steps, 1: q_sample) is word (j & 3) of
//   Philox(counter = (64 (j >> 2) + lane, pos | sid << 16, call, gid), key = seed)  ->  (word >> 8) * 2^-24  in [0, 1):
// the lane that owns classes 64 j + lane runs one Philox per four of them and uses every word.
__device__ __forceinline__ float ds_u01(unsigned w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }

#define LOG_ZERO_F (-69.07755278982137f)  // logf(1e-30f)

__device__ __forceinline__ float lae(float a, float b) {  // log(exp a + exp b)
    const float m = fmaxf(a, b);
    return m + logf(expf(a - m) + expf(b - m));
}
__device__ __forceinline__ float wmaxf(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wsumf(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wsumd(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

struct SampleParams {
    const float* logits;      // [B*L][K]  (row-major, class contiguous)
    const int64_t* xt;        // [B][L] current tokens
    const int64_t* t;         // [B]
    const float* u;           // [B][K+1][L] uniforms in [0,1)
    const float* sched;       // 8 rows of (T+1) floats: log_at, log_bt, log_ct, log_1_min_ct,
                              //   log_cumprod_at, log_cumprod_bt, log_cumprod_ct, log_1_min_cumprod_ct
    int64_t* out_tokens;      // [B][L]
    float* dbg_log_pred;      // optional [B][K+1][L]
    float* dbg_trunc;         // optional
    float* dbg_post;          // optional
    int B, L, T;
    int initial;              // 1: x_t is the all-[MASK] start state (log one-hot = 0 / -inf)
    float trunc_r;            // < 0: no top-r truncation
    int trunc_k;              // > 0: top-k truncation instead ('top{k}p', dalle_spec.py:147-157)
    int lrows;                // rows of `logits` per sample (>= L: the denoiser's padded-row mode), L by default
};
// u == nullptr: the uniforms come from the Philox stream of (seed; gid[b], call) instead (see ds_u01 above).  (A separate
// kernel argument: with these fields inside SampleParams hipcc reserves 68 bytes of -- unused -- private segment.)
struct SampleRng {
    const int64_t* gid;       // [B] global caption ids (< 2^32)
    unsigned seed_lo, seed_hi;
    int call;
};

// REGION-HELD form (inpainting / continuation: the *_hold entries).  keep[b][pos] != 0: the position is held and carries
// known[b][pos]; positions in content_token's time-major order (5 column + row).  A held column's wave writes its token and
// exits before the log-softmax; a free column runs the body below unchanged -- same logits, same uniforms (the [B][K+1][L]
// tensor keeps its shape, the Philox counters are positional), so with keep all zero the tokens are those of the unheld
// kernels bit for bit.  mode 0 (clamp): a held column writes known.  mode 1 (renoise, in-kernel noise only): the call's
// output is x_{t_post - 1} (t_post = p.t), and a held column draws q(x_{t_post-1} | x_0 = known) -- ds_q_sample_column, on
// stream 1 of the caption with the (pos, call, gid) counters of this call -- or writes known when t_post = 0.
// `initial` has no per-position form and callers pass 0 with keep: it is read for a non-[MASK] x_t only (`off` below; every
// is_mask branch ignores it), and a mixed start state only adds non-[MASK] positions with the ordinary 0 / log 1e-30 one-hot.
// A separate kernel argument and separate __global__ wrappers over one body: the unheld kernels keep their arguments,
// registers and (zero) private segment.
struct SampleHold {
    const unsigned char* keep;   // [B][L]
    const int64_t* known;        // [B][L]
    int mode;                    // 0: clamp, 1: renoise
};

__device__ __forceinline__ int ds_q_sample_column(int x, int tt, const float* __restrict__ sched, int T1, int K, int lane,
                                                  const float* up, int L, int pos, unsigned gid, unsigned seed_lo,
                                                  unsigned seed_hi, int call);

// GUIDED form (classifier-free guidance: the *_guided entries).  Every column has two logit rows: p.logits from the denoiser
// run with the caption (zc), logits_u -- same row layout, same lrows -- from the run with the null condition (zu), both on
// the same x_t and t.  After predict_start of each row (lc, lu: the f64 log-softmax rounded to f32 and clamped, as above)
//   g = lu + scale (lc - lu),  g <- g - logsumexp(g)   in float64 (max-shifted),
// rounded to f32 and clamped to [-70, 0], is the log_pred that truncation, posterior and Gumbel-argmax consume unchanged
// (VQ-Diffusion's improved sampler on this kernel's f64 conventions).  scale 0: the null prediction, 1: the captioned one.
// A separate kernel argument and ONE separate __global__ wrapper per (K, noise source), which takes SampleHold with
// keep == nullptr meaning unheld (one wave-uniform pointer test): the unguided kernels keep their arguments and registers.
struct SampleGuide {
    const float* logits_u;       // [B * lrows][K]
    float scale;
};

// PURITY form (purity-prior sampling: the *_purity entries; specification: DESIGN.md section 4).  The column's wave runs the
// prediction, the guidance and the truncation of the body below -- the same code, not a copy -- and then, instead of the posterior,
// sharpens the truncated prediction (weight r > 0: a = 1 + r expf(lmax), sh = a tr - logsumexp(a tr) in float64; r == 0: sh = tr,
// no arithmetic), draws the candidate token c* = argmax over the K real classes of sh + Gumbel with the uniforms the plain tail
// uses for those classes, and writes (c*, key) to the caller's scratch: key = lmax + Gumbel([MASK] slot's uniform) at a [MASK]
// position, -INFINITY elsewhere; lmax = max_c lp[c] before truncation is the log of the purity.  Which positions take their
// candidate is decided per sample by ds_sample_purity_select_kernel.  A separate kernel argument and separate __global__
// wrappers, as for SampleHold and SampleGuide: the other kernels keep their arguments, registers and code.
struct SamplePurity {
    int* cand;                   // [B][L]
    float* key;                  // [B][L]
    float* dbg_sharp;            // optional [B][K+1][L]
    float weight;                // r >= 0
};

// COMPOSED form (caption tracks: the *_composed entries).  The general form of the guided mix: C = n_tracks captions per clip,
// each with its own weight at every grid position.  p.logits holds C + 1 slabs, track_stride floats apart, each in the row
// layout of the plain tail (same lrows): tracks 0 .. C-1, the null condition LAST.  Per column, in float64,
//   g = lu;  for i = 0 .. C-1 in index order:  g = g + w[b][i][pos] (l_i - lu);   g <- g - logsumexp(g)  (max-shifted),
// with lu, l_i the predict_start of the null row and of track i's row; rounded to f32 and clamped to [-70, 0] it is the log_pred
// that truncation, posterior and Gumbel-argmax consume unchanged.  C = 1 with a constant weight s is the guided kernel's own
// expression (lu + s (lc - lu): the same f64 operations in the same order), so its results are the guided tail's bit for bit.
// A track whose weight at the position is exactly 0 is NOT READ there: the weight is wave-uniform (one per column), so one
// scalar branch skips its predict_start; its term is exactly 0, so no bit changes.  All weights zero: the null prediction.
// Negative weights push away from a caption.  A separate kernel argument and ONE separate __global__ wrapper per (K, noise
// source), taking SampleHold with keep == nullptr meaning unheld, as the guided wrapper does: the other kernels keep their
// arguments, registers and code.
struct SampleCompose {
    const float* weights;        // [B][n_tracks][L]
    size_t track_stride;         // floats between two slabs of p.logits
    int n_tracks;                // 1 .. DS_MAX_TRACKS
};

// JOINT form (joint-window sampling of a long clip: the *_joint entries; geometry: DESIGN.md section 4).  All W windows of a
// clip live on one token canvas of C columns -- line: C = G + (W - 1) h, ring: C = W h, hop h = G - n, n overlap columns --
// and one wave handles one CANVAS position q = R c + r: p.L is the canvas length R C, p.xt / p.out_tokens / keep / known / the
// uniforms and the Philox position are the canvas's, p.B counts clips.  p.logits holds one slab of lrows rows per WINDOW, row
// ((b W + w) lrows + R o + r) for offset o of window w.  The later window of column c is w1 = min(c / h, W - 1) (ring: c / h)
// at offset o1 = c - w1 h; with o1 < n and (w1 >= 1 or ring) the earlier window w0 = (w1 - 1) mod W covers the column too, at
// offset o1 + h.  A position under one window gets that row's log_pred -- the plain tail's, or with gd.logits_u (here a
// run-time test, one wave-uniform branch) the guided tail's.  A position under two windows: l0, l1 = those log_preds (each
// rounded to f32 and clamped), then the GUIDED expression with (lu, lc, scale) = (l0, l1, fade[o1]) -- the same macro, the
// same f64 operations in the same order -- and its renormalisation give the log_pred that truncation, posterior and
// Gumbel-argmax consume unchanged.  The posterior's timestep is p.t[b t_stride]: 1 for the tail entries (t i64[B]), W where
// the step driver hands over the network's vector (one entry per window row).  A separate kernel argument and ONE separate
// __global__ wrapper per (K, noise source), keep == nullptr meaning unheld: the other kernels keep their arguments,
// registers and code.
struct SampleJoint {
    const float* fade;           // f32[n]: the later window's weight at overlap offset o (audio.fade_table(n))
    int W, n, ring;
    int t_stride;
};

__device__ __forceinline__ double wmaxd(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// predict_start of one column (diffusion_transformer.py:285-289) into float lp[NPL]: float64 log-softmax over the K real classes
// of the row at lg_, rounded to f32 and clamped to [-70, 0]; the lane owns classes 64 j + lane.  A macro, not a function: the
// guided kernel runs it on both rows, and through a function taking lp by reference the unguided kernels' device code changed
// (register allocation and schedule); expanded in place it is the code they always had, instruction for instruction.
#define DS_PREDICT_START_ROW(lg_, lp_)                                                   \
    {                                                                                    \
        float v[NPL];                                                                    \
        const float* lg = (lg_);                                                         \
        _Pragma("unroll") for (int j = 0; j < NPL; ++j) v[j] = lg[j * 64 + lane];        \
        float mx = v[0];                                                                 \
        _Pragma("unroll") for (int j = 1; j < NPL; ++j) mx = fmaxf(mx, v[j]);            \
        mx = wmaxf(mx);                                                                  \
        /* log(n + rest) as log n + log1p(rest / n), n: the classes at the maximum (their exp is exactly 1), rest: the  \
           others' sum.  log(1 + rest) has an ABSOLUTE error of 1e-16: in the dominant class's entry, -rest, that is     \
           more than a float ulp once the class holds all but 2e-9 of the mass (tests/test_hip_sampler_edges.py). */    \
        double se = 0.0;                                                                 \
        int nmx = 0;                                                                     \
        _Pragma("unroll") for (int j = 0; j < NPL; ++j) {                                \
            const bool top = v[j] == mx;                                                 \
            nmx += __popcll(__ballot(top));                                              \
            se += top ? 0.0 : exp((double)v[j] - (double)mx);                            \
        }                                                                                \
        se = wsumd(se);                                                                  \
        const double lse64 = nmx == 1 ? log1p(se) : log((double)nmx) + log1p(se / (double)nmx); \
        _Pragma("unroll") for (int j = 0; j < NPL; ++j) {                                \
            float x = (float)(((double)v[j] - (double)mx) - lse64);                      \
            lp_[j] = fminf(fmaxf(x, -70.f), 0.f);                                        \
        }                                                                                \
    }

// The guided mix of two predictions, gv = lu + s (lc - lu) in float64, and the renormalisation of a mix, lp = f32(gv - logsumexp(gv))
// (max-shifted) clamped to [-70, 0]: macros for the reason above, expanded by the guided, the composed and the joint form.
#define DS_GUIDE_MIX(gv_, lu_, lc_, s_) \
    _Pragma("unroll") for (int j = 0; j < NPL; ++j) gv_[j] = (double)lu_[j] + s_ * ((double)lc_[j] - (double)lu_[j]);
#define DS_GUIDE_RENORM(gv_, lp_)                                                        \
    {                                                                                    \
        double gm = gv_[0];                                                              \
        _Pragma("unroll") for (int j = 1; j < NPL; ++j) gm = fmax(gm, gv_[j]);           \
        gm = wmaxd(gm);                                                                  \
        double gs = 0.0;                                                                 \
        _Pragma("unroll") for (int j = 0; j < NPL; ++j) gs += exp(gv_[j] - gm);          \
        const double glse = log(wsumd(gs));                                              \
        _Pragma("unroll") for (int j = 0; j < NPL; ++j)                                  \
            lp_[j] = fminf(fmaxf((float)((gv_[j] - gm) - glse), -70.f), 0.f);            \
    }

template <int NPL, bool RNG, bool HOLD, bool GUIDED = false, bool PURITY = false, bool COMPOSED = false, bool JOINT = false>
__device__ __forceinline__ void ds_sample_tail_body(const SampleParams& p, const SampleRng& g, const SampleHold& h,
                                                    const SampleGuide& gd = SampleGuide{nullptr, 1.f},
                                                    const SamplePurity& pu = SamplePurity{nullptr, nullptr, nullptr, 0.f},
                                                    const SampleCompose& cp = SampleCompose{nullptr, 0, 0},
                                                    const SampleJoint& jt = SampleJoint{nullptr, 1, 1, 0, 1}) {
    constexpr int K = NPL * 64;
    __shared__ float s_lp[4][K];
    __shared__ __attribute__((aligned(16))) float s_pr[4][K];
    __shared__ unsigned long long s_key[4][K];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int col = blockIdx.x * 4 + w;
    const bool live = col < p.B * p.L;  // a dead wave shadows the last column and writes nothing
    if (!live) col = p.B * p.L - 1;
    const int b = col / p.L, pos = col - b * p.L;
    if constexpr (HOLD) {
        if ((!(GUIDED || COMPOSED || JOINT) || h.keep) && h.keep[col]) {       // wave-uniform: the whole wave leaves (no block-wide barrier below in this form)
            int tok = (int)h.known[col];
            if constexpr (RNG) {
                const int tp = (int)p.t[b];
                if (h.mode == 1 && tp > 0)
                    tok = ds_q_sample_column(tok, tp - 1, p.sched, p.T + 1, K, lane, nullptr, p.L, pos, (unsigned)g.gid[b],
                                             g.seed_lo, g.seed_hi, g.call);
            }
            if (lane == 0 && live) p.out_tokens[col] = tok;
            return;
        }
    }

    // ---- predict_start: float64 log-softmax over the K real classes ----
    float lp[NPL];
    if constexpr (JOINT) {
        // ---- joint windows (see SampleJoint): the later window's log_pred in lp, the earlier one's -- if there is one -- in l0 ----
        const int hop = DS_GRID_COLS - jt.n;
        const int cc = pos / DS_GRID_ROWS, rr = pos - cc * DS_GRID_ROWS;
        int w1 = cc / hop;
        if (!jt.ring && w1 > jt.W - 1) w1 = jt.W - 1;
        const int o1 = cc - w1 * hop;
        const bool two = o1 < jt.n && (w1 >= 1 || jt.ring);
        const int w0 = w1 >= 1 ? w1 - 1 : jt.W - 1;
        float l0[NPL];
#pragma unroll
        for (int j = 0; j < NPL; ++j) l0[j] = 0.f;
        for (int k = two ? 0 : 1; k < 2; ++k) {
            const size_t row = k ? ((size_t)b * jt.W + w1) * p.lrows + DS_GRID_ROWS * o1 + rr
                                 : ((size_t)b * jt.W + w0) * p.lrows + DS_GRID_ROWS * (o1 + hop) + rr;
            float lw[NPL];
            DS_PREDICT_START_ROW(p.logits + row * K, lw)
            if (gd.logits_u) {
                float lu[NPL];
                DS_PREDICT_START_ROW(gd.logits_u + row * K, lu)
                const double s = (double)gd.scale;
                double gv[NPL];
                DS_GUIDE_MIX(gv, lu, lw, s)
                DS_GUIDE_RENORM(gv, lw)
            }
#pragma unroll
            for (int j = 0; j < NPL; ++j) {
                if (k == 0) l0[j] = lw[j];
                lp[j] = lw[j];
            }
        }
        if (two) {
            const double s = (double)jt.fade[o1];
            double gv[NPL];
            DS_GUIDE_MIX(gv, l0, lp, s)
            DS_GUIDE_RENORM(gv, lp)
        }
    } else if constexpr (COMPOSED) {    // the null condition's row (the last slab) first: lp is lu until the mix below replaces it
        DS_PREDICT_START_ROW(p.logits + (size_t)cp.n_tracks * cp.track_stride + ((size_t)b * p.lrows + pos) * K, lp)
    } else {
    DS_PREDICT_START_ROW(p.logits + ((size_t)b * p.lrows + pos) * K, lp)
    }
    if constexpr (GUIDED || COMPOSED) {
        // ---- guidance: lc (in lp), then lu, then the f64 mix and its renormalisation; lp becomes the guided log_pred ----
        double gv[NPL];
        if constexpr (COMPOSED) {
            // ---- caption tracks: g = lu + sum_i w_i (l_i - lu), one track at a time in index order; weight 0: track not read ----
#pragma unroll
            for (int j = 0; j < NPL; ++j) gv[j] = (double)lp[j];
            const float* wp = cp.weights + (size_t)b * cp.n_tracks * p.L + pos;
            const float* lt = p.logits + ((size_t)b * p.lrows + pos) * K;
            for (int i = 0; i < cp.n_tracks; ++i) {
                // one weight per column: made scalar, so the test is one scalar branch of the whole wave
                const float wi = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(wp[(size_t)i * p.L])));
                if (wi != 0.f) {
                    float li[NPL];
                    DS_PREDICT_START_ROW(lt + (size_t)i * cp.track_stride, li)
                    const double s = (double)wi;
#pragma unroll
                    for (int j = 0; j < NPL; ++j) gv[j] = gv[j] + s * ((double)li[j] - (double)lp[j]);
                }
            }
        } else {
            float lu[NPL];
            DS_PREDICT_START_ROW(gd.logits_u + ((size_t)b * p.lrows + pos) * K, lu)
            const double s = (double)gd.scale;
            DS_GUIDE_MIX(gv, lu, lp, s)
        }
        DS_GUIDE_RENORM(gv, lp)
    }
    const size_t dbg_base = (size_t)b * (K + 1) * p.L + pos;
    if (p.dbg_log_pred && live) {
#pragma unroll
        for (int j = 0; j < NPL; ++j) p.dbg_log_pred[dbg_base + (size_t)(j * 64 + lane) * p.L] = lp[j];
        if (lane == 0) p.dbg_log_pred[dbg_base + (size_t)K * p.L] = -70.f;
    }

    // ---- truncation: top-r (probability mass ranked ahead < r) or top-k (rank < k) ----
    // top-k, dalle_spec.py:147-157: topk over the K+1 rows, everything else -70.  The [MASK] row is -70 and a
    // kept -70 is indistinguishable from a dropped one, so ranking the K real classes is equivalent.
    float tr[NPL];
    if (p.trunc_k > 0) {
#pragma unroll
        for (int j = 0; j < NPL; ++j) s_lp[w][j * 64 + lane] = lp[j];
        if constexpr (HOLD) __builtin_amdgcn_wave_barrier();   // s_lp[w] is this wave's own; held waves have left
        else __syncthreads();
        int rank[NPL];
#pragma unroll
        for (int j = 0; j < NPL; ++j) rank[j] = 0;
        for (int c = 0; c < K; ++c) {
            const float ol = s_lp[w][c];
#pragma unroll
            for (int j = 0; j < NPL; ++j) {
                const int me = j * 64 + lane;
                rank[j] += (ol > lp[j] || (ol == lp[j] && c < me)) ? 1 : 0;
            }
        }
#pragma unroll
        for (int j = 0; j < NPL; ++j) tr[j] = rank[j] < p.trunc_k ? lp[j] : -70.f;
    } else if (p.trunc_r >= 0.f) {
        // dalle_spec.py:159-172: sort descending, exp, cumsum; rank i is kept iff the mass of ranks 0 .. i-1 is < r (rank 0 always).
        // Round 4: the ranks come from a bitonic sort of the column in LDS (one wave per column, 64-bit keys = order-preserving
        // image of the log-probability | inverted class index: descending value, ascending index among ties) and the mass from
        // the sum in rank order, accumulated the way torch's CPU cumsum does, instead of 65 536 pair tests per column
        // (the kernel's 173 us per step were 160 us of those: the largest item of a sampling step after the transformer).
        // The kept set is a prefix of the rank order (the masses are non-negative), so the scan only has to find its length.
        unsigned long long* key = s_key[w];
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            const unsigned bits = __float_as_uint(lp[j] + 0.f);                         // (+ 0: -0 and +0 are one key)
            const unsigned u = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);      // unsigned order = float order
            key[j * 64 + lane] = ((unsigned long long)u << 32) | (unsigned)(0xffffffffu - (unsigned)(j * 64 + lane));
        }
        __builtin_amdgcn_wave_barrier();
        for (int k = 2; k <= K; k <<= 1)
            for (int jj = k >> 1; jj > 0; jj >>= 1) {
#pragma unroll
                for (int h = 0; h < K / 128; ++h) {
                    const int tq = lane + 64 * h;
                    const int i = ((tq & ~(jj - 1)) << 1) | (tq & (jj - 1)), l = i | jj;
                    const unsigned long long a = key[i], bq = key[l];
                    const bool sw = ((i & k) == 0) ? (a < bq) : (a > bq);                // descending blocks where (i & k) == 0
                    if (sw) { key[i] = bq; key[l] = a; }
                }
                __builtin_amdgcn_wave_barrier();       // (a wave's LDS operations execute in order: no hardware barrier needed)
            }
        // probabilities in rank order (this lane: ranks 4 lane' .. for the scan's 16-byte reads)
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            const int rk = j * 64 + lane;
            const unsigned u = (unsigned)(key[rk] >> 32);
            const unsigned bits = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
            s_pr[w][rk] = expf(__uint_as_float(bits));
        }
        __builtin_amdgcn_wave_barrier();
        // n_keep = 1 + #{ i >= 1 : p[0] + .. + p[i-1] < r }, every lane runs the same sequential sum (uniform early exit)
        int n_keep = 1;
        {
            // torch's CPU cumsum of a float tensor accumulates in DOUBLE and rounds every partial sum to float: the same here
            // (tests/test_sampler_sort_emulation.py: with this accumulator the restated algorithm equals the reference's
            // truncation AS EXECUTED ON THE CPU bit for bit -- the goldens are CPU runs; a plain fp32 chain differs in the
            // last place of some partial sums, and so does a CUDA execution of dalle_spec.py:163-165, whose cumsum is a
            // parallel fp32 scan: against a GPU run of the reference a cut at a rounding-level near-tie can differ)
            // float(c) < r, tested on the double: float(c) <= pf = the float below r  <=>  c below the midpoint of pf and r (at the
            // midpoint itself round-to-nearest-even goes to pf iff pf's last mantissa bit is 0)
            double cum = 0.0;
            const float r_ = p.trunc_r;
            const float pf = __uint_as_float(__float_as_uint(r_) - 1u);      // r > 0 (top-r rates are in (0, 1])
            const double mid = 0.5 * ((double)pf + (double)r_);
            const bool tie_low = (__float_as_uint(pf) & 1u) == 0u;
            // c <= mid as ONE comparison: c < the double after mid (mid > 0: its bit pattern + 1)
            const double lim = tie_low ? __longlong_as_double(__double_as_longlong(mid) + 1) : mid;
            auto below = [&](double c) { return c < lim; };
            if (r_ > 0.f)            // (r = 0: no partial sum is below it, rank 0 alone survives)
            for (int i = 0; i < K; i += 4) {
                const f32x4 p4 = *(const f32x4*)(&s_pr[w][i]);
                const double c0 = cum + (double)p4[0], c1 = c0 + (double)p4[1], c2 = c1 + (double)p4[2], c3 = c2 + (double)p4[3];
                // rank i + e + 1 is kept iff float(c_e) < r; the sums do not decrease, so the tests fail from some e on
                const bool b3 = below(c3);
                n_keep += (below(c0) ? 1 : 0) + (below(c1) ? 1 : 0) + (below(c2) ? 1 : 0) + ((b3 && i + 4 < K) ? 1 : 0);
                cum = c3;
                if (!b3) break;
            }
        }
        // back to class order: the class at rank rk is kept iff rk < n_keep
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            const int rk = j * 64 + lane;
            const unsigned cls = 0xffffffffu - (unsigned)(key[rk] & 0xffffffffull);
            s_lp[w][cls] = rk < n_keep ? 1.f : 0.f;
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < NPL; ++j) tr[j] = s_lp[w][j * 64 + lane] != 0.f ? lp[j] : -70.f;
    } else {
#pragma unroll
        for (int j = 0; j < NPL; ++j) tr[j] = lp[j];
    }
    if (p.dbg_trunc && live) {
#pragma unroll
        for (int j = 0; j < NPL; ++j) p.dbg_trunc[dbg_base + (size_t)(j * 64 + lane) * p.L] = tr[j];
        if (lane == 0) p.dbg_trunc[dbg_base + (size_t)K * p.L] = -70.f;
    }

    float post[NPL];
    float post_m;
    [[maybe_unused]] float lmax = 0.f;
    if constexpr (PURITY) {
        // ---- purity and sharpening: `post` becomes sh, the distribution the candidate is drawn from ----
        lmax = lp[0];
#pragma unroll
        for (int j = 1; j < NPL; ++j) lmax = fmaxf(lmax, lp[j]);
        lmax = wmaxf(lmax);
        if (pu.weight > 0.f) {
            const double a = (double)(1.f + pu.weight * expf(lmax));
            double av[NPL];
#pragma unroll
            for (int j = 0; j < NPL; ++j) av[j] = a * (double)tr[j];
            double am = av[0];
#pragma unroll
            for (int j = 1; j < NPL; ++j) am = fmax(am, av[j]);
            am = wmaxd(am);
            double as = 0.0;
#pragma unroll
            for (int j = 0; j < NPL; ++j) as += exp(av[j] - am);
            const double alse = log(wsumd(as));
#pragma unroll
            for (int j = 0; j < NPL; ++j) post[j] = fminf(fmaxf((float)((av[j] - am) - alse), -70.f), 0.f);
        } else {
#pragma unroll
            for (int j = 0; j < NPL; ++j) post[j] = tr[j];
        }
        post_m = -70.f;                  // (dumped only: the [MASK] class is no candidate)
        if (pu.dbg_sharp && live) {
#pragma unroll
            for (int j = 0; j < NPL; ++j) pu.dbg_sharp[dbg_base + (size_t)(j * 64 + lane) * p.L] = post[j];
            if (lane == 0) pu.dbg_sharp[dbg_base + (size_t)K * p.L] = post_m;
        }
    } else {
    // ---- q_posterior ----
    const int T1 = p.T + 1;
    const int t = (int)p.t[JOINT ? b * jt.t_stride : b];
    const int tm1 = (t - 1 + T1) % T1;
    const float* S = p.sched;
    const float lat = S[0 * T1 + t], lbt = S[1 * T1 + t], lct = S[2 * T1 + t];
    const float lcat = S[4 * T1 + t], lcbt = S[5 * T1 + t], lcct = S[6 * T1 + t];
    const float lcat1 = S[4 * T1 + tm1], lcbt1 = S[5 * T1 + tm1], lcct1 = S[6 * T1 + tm1], l1mcct1 = S[7 * T1 + tm1];
    const int xt = (int)p.xt[col];
    const bool is_mask = xt == K;
    const float off = p.initial ? -INFINITY : LOG_ZERO_F;  // log one-hot value away from x_t
    // log q(x_t | x_0 = c) and log q(x_t | x_{t-1} = c) take two values per column: c == x_t or not
    const float qt_hit = is_mask ? lcct : lae(0.f + lcat, lcbt);
    const float qt_off = is_mask ? lcct : lae(off + lcat, lcbt);
    const float q1_hit = is_mask ? lct : lae(0.f + lat, lbt);
    const float q1_off = is_mask ? lct : lae(off + lat, lbt);
    const float qt_m = is_mask ? 0.f : LOG_ZERO_F;  // [MASK] row
    const float q1_m = qt_m;

    float q[NPL];
    float qmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        const int c = j * 64 + lane;
        q[j] = tr[j] - (c == xt ? qt_hit : qt_off);
        qmax = fmaxf(qmax, q[j]);
    }
    const float q_m = -70.f - qt_m;
    qmax = fmaxf(wmaxf(qmax), q_m);
    float es = 0.f;
#pragma unroll
    for (int j = 0; j < NPL; ++j) es += expf(q[j] - qmax);
    es = wsumf(es) + expf(q_m - qmax);
    const float lse = logf(es) + qmax;  // torch.logsumexp

#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        const int c = j * 64 + lane;
        const float ev = lae((q[j] - lse) + lcat1, lcbt1);
        const float o = ev + (c == xt ? q1_hit : q1_off) + lse;
        post[j] = fminf(fmaxf(o, -70.f), 0.f);
    }
    {
        const float ev = lae((q_m - lse) + l1mcct1, lcct1);
        post_m = fminf(fmaxf(ev + q1_m + lse, -70.f), 0.f);
    }
    if (p.dbg_post && live) {
#pragma unroll
        for (int j = 0; j < NPL; ++j) p.dbg_post[dbg_base + (size_t)(j * 64 + lane) * p.L] = post[j];
        if (lane == 0) p.dbg_post[dbg_base + (size_t)K * p.L] = post_m;
    }
    }

    // ---- Gumbel-argmax (first index wins ties, as torch.argmax) ----
    float un[NPL], un_m;            // this lane's uniforms (classes 64 j + lane) and the [MASK] class's
    if (!RNG) {
        const float* up = p.u + dbg_base;
#pragma unroll
        for (int j = 0; j < NPL; ++j) un[j] = up[(size_t)(j * 64 + lane) * p.L];
        un_m = up[(size_t)K * p.L];
    } else {
        const unsigned gid = (unsigned)g.gid[b];
#pragma unroll
        for (int q = 0; q < NPL / 4; ++q) {
            const ds_u32x4 w4 = ds_philox4x32_10(q * 64 + lane, pos, g.call, gid, g.seed_lo, g.seed_hi);
            un[4 * q + 0] = ds_u01(w4.x); un[4 * q + 1] = ds_u01(w4.y);
            un[4 * q + 2] = ds_u01(w4.z); un[4 * q + 3] = ds_u01(w4.w);
        }
        un_m = ds_u01(ds_philox4x32_10((NPL / 4) * 64, pos, g.call, gid, g.seed_lo, g.seed_hi).x);
    }
    float best = -INFINITY;
    int bidx = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        const int c = j * 64 + lane;
        const float gsc = -logf(-logf(un[j] + 1e-30f) + 1e-30f) + post[j];
        if (gsc > best) { best = gsc; bidx = c; }  // ascending c within a lane keeps the first max
    }
    if (!PURITY && lane == 0) {
        const float gsc = -logf(-logf(un_m + 1e-30f) + 1e-30f) + post_m;
        if (gsc > best) { best = gsc; bidx = K; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bidx, o);
        if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    if constexpr (PURITY) {
        if (lane == 0 && live) {
            pu.cand[col] = bidx;
            pu.key[col] = (int)p.xt[col] == K ? lmax + -logf(-logf(un_m + 1e-30f) + 1e-30f) : -INFINITY;
        }
    } else if (lane == 0 && live) p.out_tokens[col] = bidx;
}

template <int NPL, bool RNG>
__global__ __launch_bounds__(256) void ds_sample_tail_kernel(const SampleParams p, const SampleRng g) {
    ds_sample_tail_body<NPL, RNG, false>(p, g, SampleHold{nullptr, nullptr, 0});
}
template <int NPL, bool RNG>
__global__ __launch_bounds__(256) void ds_sample_tail_hold_kernel(const SampleParams p, const SampleRng g, const SampleHold h) {
    ds_sample_tail_body<NPL, RNG, true>(p, g, h);
}

#undef DS_PREDICT_START_ROW
#undef DS_GUIDE_MIX
#undef DS_GUIDE_RENORM

template <int NPL, bool RNG>
__global__ __launch_bounds__(256) void ds_sample_tail_guided_kernel(const SampleParams p, const SampleRng g, const SampleHold h,
                                                                    const SampleGuide gd) {
    ds_sample_tail_body<NPL, RNG, true, true>(p, g, h, gd);
}

// steps 1-5 of a purity step (see SamplePurity): one wave per grid position -> (candidate, key) in the caller's scratch
template <int NPL, bool RNG, bool GUIDED>
__global__ __launch_bounds__(256) void ds_sample_purity_rows_kernel(const SampleParams p, const SampleRng g, const SampleGuide gd,
                                                                    const SamplePurity pu) {
    ds_sample_tail_body<NPL, RNG, false, GUIDED, true>(p, g, SampleHold{nullptr, nullptr, 0}, gd, pu);
}

// the composed tail (see SampleCompose): the posterior tail on the mix of n_tracks captions and the null condition
template <int NPL, bool RNG>
__global__ __launch_bounds__(256) void ds_sample_tail_composed_kernel(const SampleParams p, const SampleRng g, const SampleHold h,
                                                                      const SampleCompose cp) {
    ds_sample_tail_body<NPL, RNG, true, false, false, true>(p, g, h, SampleGuide{nullptr, 1.f},
                                                            SamplePurity{nullptr, nullptr, nullptr, 0.f}, cp);
}

// the joint tail (see SampleJoint): one wave per canvas position; guided iff gd.logits_u
template <int NPL, bool RNG>
__global__ __launch_bounds__(256) void ds_sample_tail_joint_kernel(const SampleParams p, const SampleRng g, const SampleHold h,
                                                                   const SampleGuide gd, const SampleJoint jt) {
    ds_sample_tail_body<NPL, RNG, true, false, false, false, true>(p, g, h, gd, SamplePurity{nullptr, nullptr, nullptr, 0.f},
                                                                   SampleCompose{nullptr, 0, 0}, jt);
}

// The window rows of a canvas (see SampleJoint), as the denoiser reads them: win[(k B W + b W + w)][R o + r] =
// canvas[b][R ((w h + o) mod C) + r] for k < copies -- condition-major, the layout of StepCall::tokens2.  One thread per
// token of one copy: a whole int64 loaded once and stored `copies` times.
__global__ __launch_bounds__(256) void ds_joint_gather_kernel(const int64_t* __restrict__ canvas, int64_t* __restrict__ win,
                                                              int B, int W, int hop, int C, int copies) {
    constexpr int L = DS_GRID_ROWS * DS_GRID_COLS;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, n = (long long)B * W * L;
    if (i >= n) return;
    const int e = (int)(i % L), bw = (int)(i / L);
    const int b = bw / W, w = bw - b * W;
    const int o = e / DS_GRID_ROWS, r = e - o * DS_GRID_ROWS;
    const int64_t v = canvas[(size_t)b * DS_GRID_ROWS * C + (size_t)DS_GRID_ROWS * ((w * hop + o) % C) + r];
    for (int k = 0; k < copies; ++k) win[(size_t)k * n + i] = v;
}

// step 6: one workgroup per sample.  m = its [MASK] positions, n = max(0, m - remain); the n masked positions of largest key
// take their candidate, every other position keeps its token.  Rank by counting over the keys in LDS -- position i is revealed
// iff #{j : key_j > key_i or (key_j == key_i and j < i)} < n (a non-[MASK] j carries -INFINITY and never counts against a
// finite key) -- so the result depends on no order of execution: no atomics, no data-dependent launch.
#define DS_PURITY_MAX_L 288
__global__ __launch_bounds__(256) void ds_sample_purity_select_kernel(const int64_t* __restrict__ xt, const int* __restrict__ cand,
                                                                      const float* __restrict__ key, int64_t* __restrict__ out,
                                                                      int L, int K, int remain) {
    __shared__ float s_k[DS_PURITY_MAX_L];
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * L;
    int mine = 0;
    for (int i = tid; i < L; i += 256) {
        s_k[i] = key[base + i];
        mine += (int)xt[base + i] == K ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = mine;
    __syncthreads();
    const int m = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    const int n = m > remain ? m - remain : 0;
    for (int i = tid; i < L; i += 256) {
        const int64_t x = xt[base + i];
        bool reveal = false;
        if ((int)x == K && n > 0) {
            const float ki = s_k[i];
            int rank = 0;
            for (int j = 0; j < L; ++j) {
                const float kj = s_k[j];
                rank += (kj > ki || (kj == ki && j < i)) ? 1 : 0;
            }
            reveal = rank < n;
        }
        out[base + i] = reveal ? (int64_t)cand[base + i] : x;
    }
}

// ---- training-loss terms (DiffusionTransformer._train_loss, diffusion_transformer.py:408-476), forward only ----
// q_posterior (:293-339) of a per-column distribution lx0[] over the K classes (+ its [MASK] row lx0_m) given
// x_t and t: the same arithmetic as the sampling tail above, factored out for the two posteriors of the loss.
template <int NPL>
__device__ __forceinline__ void ds_posterior(const float (&lx0)[NPL], float lx0_m, int xt, int K, int lane,
                                             const float* __restrict__ S, int T1, int t, float (&post)[NPL],
                                             float& post_m) {
    const int tm1 = (t - 1 + T1) % T1;
    const float lat = S[0 * T1 + t], lbt = S[1 * T1 + t], lct = S[2 * T1 + t];
    const float lcat = S[4 * T1 + t], lcbt = S[5 * T1 + t], lcct = S[6 * T1 + t];
    const float lcat1 = S[4 * T1 + tm1], lcbt1 = S[5 * T1 + tm1], lcct1 = S[6 * T1 + tm1], l1mcct1 = S[7 * T1 + tm1];
    const bool is_mask = xt == K;
    const float qt_hit = is_mask ? lcct : lae(0.f + lcat, lcbt), qt_off = is_mask ? lcct : lae(LOG_ZERO_F + lcat, lcbt);
    const float q1_hit = is_mask ? lct : lae(0.f + lat, lbt), q1_off = is_mask ? lct : lae(LOG_ZERO_F + lat, lbt);
    const float qt_m = is_mask ? 0.f : LOG_ZERO_F, q1_m = qt_m;
    float q[NPL];
    float qmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        const int c = j * 64 + lane;
        q[j] = lx0[j] - (c == xt ? qt_hit : qt_off);
        qmax = fmaxf(qmax, q[j]);
    }
    const float q_m = lx0_m - qt_m;
    qmax = fmaxf(wmaxf(qmax), q_m);
    float es = 0.f;
#pragma unroll
    for (int j = 0; j < NPL; ++j) es += expf(q[j] - qmax);
    es = wsumf(es) + expf(q_m - qmax);
    const float lse = logf(es) + qmax;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        const int c = j * 64 + lane;
        const float ev = lae((q[j] - lse) + lcat1, lcbt1);
        post[j] = fminf(fmaxf(ev + (c == xt ? q1_hit : q1_off) + lse, -70.f), 0.f);
    }
    const float evm = lae((q_m - lse) + l1mcct1, lcct1);
    post_m = fminf(fmaxf(evm + q1_m + lse, -70.f), 0.f);
}

// Per grid position: kl = KL(q(x_{t-1}|x_t,x_0) || p_theta(x_{t-1}|x_t)) (:439-440), decoder_nll =
// -log p_theta(x_0|...) (:446), kl_aux = KL(x_0 || p_theta(x_0|x_t)) over the K real classes (:462).  The mask
// weights, the t == 0 switch, 1/pt and the sums over positions are a few tiny torch ops on the [B][L] outputs.
template <int NPL>
__global__ __launch_bounds__(256) void ds_loss_tail_kernel(const float* __restrict__ logits,
                                                           const int64_t* __restrict__ x0, const int64_t* __restrict__ xt,
                                                           const int64_t* __restrict__ t, const float* __restrict__ sched,
                                                           float* __restrict__ kl, float* __restrict__ nll,
                                                           float* __restrict__ kl_aux, float* __restrict__ dbg_model,
                                                           int B, int L, int T) {
    constexpr int K = NPL * 64;
    const int lane = threadIdx.x & 63;
    const int col = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= B * L) return;
    const int b = col / L, pos = col - b * L;
    float v[NPL];
    const float* lg = logits + (size_t)col * K;
#pragma unroll
    for (int j = 0; j < NPL; ++j) v[j] = lg[j * 64 + lane];
    float mx = v[0];
#pragma unroll
    for (int j = 1; j < NPL; ++j) mx = fmaxf(mx, v[j]);
    mx = wmaxf(mx);
    double se = 0.0;
#pragma unroll
    for (int j = 0; j < NPL; ++j) se += exp((double)v[j] - (double)mx);
    const double lse64 = log(wsumd(se));
    float lp[NPL], ls[NPL];
    const int x0c = (int)x0[col], xtc = (int)xt[col], tt = (int)t[b];
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        lp[j] = fminf(fmaxf((float)(((double)v[j] - (double)mx) - lse64), -70.f), 0.f);   // log p_theta(x_0 | x_t)
        ls[j] = (j * 64 + lane) == x0c ? 0.f : LOG_ZERO_F;                                 // log one-hot of x_0
    }
    const float ls_m = x0c == K ? 0.f : LOG_ZERO_F;
    float pm[NPL], pr[NPL], pm_m, pr_m;
    ds_posterior<NPL>(lp, -70.f, xtc, K, lane, sched, T + 1, tt, pm, pm_m);    // model posterior
    ds_posterior<NPL>(ls, ls_m, xtc, K, lane, sched, T + 1, tt, pr, pr_m);     // true posterior
    float a = 0.f, n = 0.f, x = 0.f;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        a += expf(pr[j]) * (pr[j] - pm[j]);
        n += expf(ls[j]) * pm[j];
        x += expf(ls[j]) * (ls[j] - lp[j]);
    }
    a = wsumf(a) + expf(pr_m) * (pr_m - pm_m);
    n = wsumf(n) + expf(ls_m) * pm_m;
    x = wsumf(x);
    if (lane == 0) {
        kl[col] = a;
        nll[col] = -n;
        kl_aux[col] = x;
    }
    if (dbg_model) {
        const size_t base = (size_t)b * (K + 1) * L + pos;
#pragma unroll
        for (int j = 0; j < NPL; ++j) dbg_model[base + (size_t)(j * 64 + lane) * L] = pm[j];
        if (lane == 0) dbg_model[base + (size_t)K * L] = pm_m;
    }
}

// d(sum_b vb_loss_b) / d logits of the training loss: the first backward kernel of scope row 8f-3 (closed form and
// derivation: oracle/diffsound_oracle.py loss_tail_backward).  Same thread mapping as the forward tail.
template <int NPL>
__global__ __launch_bounds__(256) void ds_loss_tail_bwd_kernel(const float* __restrict__ logits,
                                                               const int64_t* __restrict__ x0, const int64_t* __restrict__ xt,
                                                               const int64_t* __restrict__ t, const float* __restrict__ pt,
                                                               const float* __restrict__ sched, float* __restrict__ dlogits,
                                                               int B, int L, int T, float mw_mask, float mw_other,
                                                               float aux_weight, int adaptive) {
    constexpr int K = NPL * 64;
    const int lane = threadIdx.x & 63;
    const int col = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= B * L) return;
    const int b = col / L;
    float v[NPL];
    const float* lg = logits + (size_t)col * K;
#pragma unroll
    for (int j = 0; j < NPL; ++j) v[j] = lg[j * 64 + lane];
    float mx = v[0];
#pragma unroll
    for (int j = 1; j < NPL; ++j) mx = fmaxf(mx, v[j]);
    mx = wmaxf(mx);
    double se = 0.0;
#pragma unroll
    for (int j = 0; j < NPL; ++j) se += exp((double)v[j] - (double)mx);
    const double lse64 = log(wsumd(se));
    const int x0c = (int)x0[col], xtc = (int)xt[col], tt = (int)t[b];
    const int T1 = T + 1, tm1 = (tt - 1 + T1) % T1;
    const float* S = sched;
    float lp[NPL], ls[NPL], sm[NPL];
    bool lp_live[NPL];
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        const float l = (float)(((double)v[j] - (double)mx) - lse64);
        sm[j] = expf(l);
        lp_live[j] = l > -70.f && l < 0.f;
        lp[j] = fminf(fmaxf(l, -70.f), 0.f);
        ls[j] = (j * 64 + lane) == x0c ? 0.f : LOG_ZERO_F;
    }
    const float ls_m = x0c == K ? 0.f : LOG_ZERO_F;
    // true posterior (forward code)
    float pr[NPL], pr_m;
    ds_posterior<NPL>(ls, ls_m, xtc, K, lane, S, T1, tt, pr, pr_m);
    // model posterior with the quantities its derivative needs
    const float lat = S[0 * T1 + tt], lbt = S[1 * T1 + tt], lct = S[2 * T1 + tt];
    const float lcat = S[4 * T1 + tt], lcbt = S[5 * T1 + tt], lcct = S[6 * T1 + tt];
    const float lcat1 = S[4 * T1 + tm1], lcbt1 = S[5 * T1 + tm1], lcct1 = S[6 * T1 + tm1], l1mcct1 = S[7 * T1 + tm1];
    const bool is_mask = xtc == K;
    const float qt_hit = is_mask ? lcct : lae(0.f + lcat, lcbt), qt_off = is_mask ? lcct : lae(LOG_ZERO_F + lcat, lcbt);
    const float q1_hit = is_mask ? lct : lae(0.f + lat, lbt), q1_off = is_mask ? lct : lae(LOG_ZERO_F + lat, lbt);
    const float qt_m = is_mask ? 0.f : LOG_ZERO_F, q1_m = qt_m;
    float q[NPL];
    float qmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        q[j] = lp[j] - ((j * 64 + lane) == xtc ? qt_hit : qt_off);
        qmax = fmaxf(qmax, q[j]);
    }
    const float q_m = -70.f - qt_m;
    qmax = fmaxf(wmaxf(qmax), q_m);
    float es = 0.f;
#pragma unroll
    for (int j = 0; j < NPL; ++j) es += expf(q[j] - qmax);
    es = wsumf(es) + expf(q_m - qmax);
    const float lse = logf(es) + qmax;
    const float is0 = tt == 0 ? 1.f : 0.f, ipt = 1.f / pt[b];
    const float wgt = is_mask ? mw_mask : mw_other;
    const float wa = adaptive ? (float)tt / (float)T + 1.f : 1.f;
    const float nll_scale = ipt + (aux_weight != 0.f ? wa * aux_weight * ipt : 0.f);
    float w[NPL], sg[NPL], pp[NPL];
    float ssum = 0.f;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        const float A = lae((q[j] - lse) + lcat1, lcbt1);
        const float raw = A + ((j * 64 + lane) == xtc ? q1_hit : q1_off) + lse;
        sg[j] = expf((q[j] - lse) + lcat1 - A);
        pp[j] = expf(q[j] - lse);
        const bool live = raw > -70.f && raw < 0.f;
        w[j] = live ? -(1.f - is0) * expf(pr[j]) * wgt * ipt - is0 * expf(ls[j]) * nll_scale : 0.f;
        ssum += w[j] * (1.f - sg[j]);
    }
    {   // [MASK] row
        const float A = lae((q_m - lse) + l1mcct1, lcct1);
        const float raw = A + q1_m + lse;
        const float sgm = expf((q_m - lse) + l1mcct1 - A);
        const bool live = raw > -70.f && raw < 0.f;
        const float wm = live ? -(1.f - is0) * expf(pr_m) * wgt * ipt - is0 * expf(ls_m) * nll_scale : 0.f;
        ssum = wsumf(ssum) + wm * (1.f - sgm);
    }
    float glp[NPL];
    float G = 0.f;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        float gq = w[j] * sg[j] + pp[j] * ssum;
        if (aux_weight != 0.f) gq -= (1.f - is0) * wa * aux_weight * ipt * wgt * expf(ls[j]);
        glp[j] = lp_live[j] ? gq : 0.f;
        G += glp[j];
    }
    G = wsumf(G);
    float* dz = dlogits + (size_t)col * K;
#pragma unroll
    for (int j = 0; j < NPL; ++j) dz[j * 64 + lane] = glp[j] - sm[j] * G;
}

extern "C" int ds_loss_tail_bwd(const float* logits, const int64_t* x0, const int64_t* xt, const int64_t* t,
                                const float* pt, const float* sched, float* dlogits, int B, int L, int K, int T,
                                float mask_weight_masked, float mask_weight_other, float aux_weight, int adaptive,
                                ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(logits && x0 && xt && t && pt && sched && dlogits && B > 0 && L > 0 && T > 0, "bad arguments");
    DS_CHECK_ARG(K == 256 || K == 512, "codebook size must be 256 or 512");
    const int cols = B * L;
    if (K == 256)
        hipLaunchKernelGGL((ds_loss_tail_bwd_kernel<4>), dim3((cols + 3) / 4), dim3(256), 0, stream, logits, x0, xt, t, pt,
                           sched, dlogits, B, L, T, mask_weight_masked, mask_weight_other, aux_weight, adaptive);
    else
        hipLaunchKernelGGL((ds_loss_tail_bwd_kernel<8>), dim3((cols + 3) / 4), dim3(256), 0, stream, logits, x0, xt, t, pt,
                           sched, dlogits, B, L, T, mask_weight_masked, mask_weight_other, aux_weight, adaptive);
    DS_CHECK_LAUNCH();
    return 0;
}

extern "C" int ds_loss_tail(const float* logits, const int64_t* x0, const int64_t* xt, const int64_t* t,
                            const float* sched, float* kl, float* nll, float* kl_aux, float* dbg_model_log_prob, int B,
                            int L, int K, int T, ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(logits && x0 && xt && t && sched && kl && nll && kl_aux && B > 0 && L > 0 && T > 0, "bad arguments");
    DS_CHECK_ARG(K == 256 || K == 512, "codebook size must be 256 or 512");
    const int cols = B * L;
    if (K == 256)
        hipLaunchKernelGGL((ds_loss_tail_kernel<4>), dim3((cols + 3) / 4), dim3(256), 0, stream, logits, x0, xt, t, sched,
                           kl, nll, kl_aux, dbg_model_log_prob, B, L, T);
    else
        hipLaunchKernelGGL((ds_loss_tail_kernel<8>), dim3((cols + 3) / 4), dim3(256), 0, stream, logits, x0, xt, t, sched,
                           kl, nll, kl_aux, dbg_model_log_prob, B, L, T);
    DS_CHECK_LAUNCH();
    return 0;
}

// ---- q_sample (diffusion_transformer.py:370-377): x_t ~ q(x_t | x_0) for token ids, Gumbel-argmax ----------
// log q(x_t = c | x_0) = log_add_exp(log_onehot(x_0)[c] + log_cumprod_at[t], log_cumprod_bt[t]) for the K classes,
// log_add_exp(log_onehot(x_0)[K] + log_1_min_cumprod_ct[t], log_cumprod_ct[t]) for [MASK]  (q_pred, :253-267)
// One column, one wavefront: the draw for x_0 = x at timestep tt, every lane returns the token.  up != nullptr: the column's
// uniforms in the [B][K+1][L] layout (up = u + b (K+1) L + pos); else stream 1 of caption gid's Philox draws (ds_u01 above).
// Shared by ds_q_sample_kernel and the renoise mode of the region-held sampling tail.
__device__ __forceinline__ int ds_q_sample_column(int x, int tt, const float* __restrict__ sched, int T1, int K, int lane,
                                                  const float* up, int L, int pos, unsigned gid, unsigned seed_lo,
                                                  unsigned seed_hi, int call) {
    const float lcat = sched[4 * T1 + tt], lcbt = sched[5 * T1 + tt], lcct = sched[6 * T1 + tt],
                l1mcct = sched[7 * T1 + tt];
    const float hit = lae(0.f + lcat, lcbt), off = lae(LOG_ZERO_F + lcat, lcbt);
    float best = -INFINITY;
    int bi = 0x7fffffff;
    ds_u32x4 w4 = {0u, 0u, 0u, 0u};
    for (int c = lane; c <= K; c += 64) {
        const float lq = c < K ? (c == x ? hit : off) : lae((x == K ? 0.f : LOG_ZERO_F) + l1mcct, lcct);
        float uu;
        if (up) {
            uu = up[(size_t)c * L];
        } else {
            const int j = c >> 6;
            if ((j & 3) == 0) w4 = ds_philox4x32_10((j >> 2) * 64 + (c & 63), pos | (1u << 16), call, gid, seed_lo, seed_hi);
            uu = ds_u01((j & 3) == 0 ? w4.x : (j & 3) == 1 ? w4.y : (j & 3) == 2 ? w4.z : w4.w);
        }
        const float g = -logf(-logf(uu + 1e-30f) + 1e-30f) + lq;
        if (g > best) { best = g; bi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    return bi;
}

__global__ __launch_bounds__(256) void ds_q_sample_kernel(const int64_t* __restrict__ x0, const int64_t* __restrict__ t,
                                                          const float* __restrict__ u, const float* __restrict__ sched,
                                                          int64_t* __restrict__ out, int B, int L, int K, int T,
                                                          const int64_t* __restrict__ gid, unsigned seed_lo,
                                                          unsigned seed_hi, int call) {
    const int col = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= B * L) return;
    const int lane = threadIdx.x & 63;
    const int b = col / L, pos = col - b * L;
    const float* up = u ? u + (size_t)b * (K + 1) * L + pos : nullptr;
    const int bi = ds_q_sample_column((int)x0[col], (int)t[b], sched, T + 1, K, lane, up, L, pos, u ? 0u : (unsigned)gid[b],
                                      seed_lo, seed_hi, call);
    if (lane == 0) out[col] = bi;
}

extern "C" int ds_q_sample(const int64_t* x0, const int64_t* t, const float* u, const float* sched, int64_t* out,
                           int B, int L, int K, int T, ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(x0 && t && u && sched && out && B > 0 && L > 0 && K > 0 && T > 0, "bad arguments");
    hipLaunchKernelGGL(ds_q_sample_kernel, dim3((B * L + 3) / 4), dim3(256), 0, stream, x0, t, u, sched, out, B, L, K, T,
                       (const int64_t*)nullptr, 0u, 0u, 0);
    DS_CHECK_LAUNCH();
    return 0;
}

extern "C" int ds_q_sample_rng(const int64_t* x0, const int64_t* t, const int64_t* gids, unsigned long long seed, int call,
                               const float* sched, int64_t* out, int B, int L, int K, int T, ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(x0 && t && gids && sched && out && B > 0 && L > 0 && K > 0 && T > 0, "bad arguments");
    DS_CHECK_ARG(K % 256 == 0 && L < 65536, "codebook size must be a multiple of 256, L < 65536");
    hipLaunchKernelGGL(ds_q_sample_kernel, dim3((B * L + 3) / 4), dim3(256), 0, stream, x0, t, (const float*)nullptr, sched,
                       out, B, L, K, T, gids, (unsigned)seed, (unsigned)(seed >> 32), call);
    DS_CHECK_LAUNCH();
    return 0;
}

// the uniforms the *_rng entries draw, written out in the reference's [B][K+1][L] layout (tests; same-noise comparisons
// of the two paths).  rng_stream 0: reverse steps, 1: q_sample.
__global__ __launch_bounds__(256) void ds_philox_uniforms_kernel(const int64_t* __restrict__ gid, unsigned seed_lo,
                                                                 unsigned seed_hi, int call, unsigned sid,
                                                                 float* __restrict__ u, int B, int L, int K) {
    const int col = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= B * L) return;
    const int lane = threadIdx.x & 63;
    const int b = col / L, pos = col - b * L;
    float* up = u + (size_t)b * (K + 1) * L + pos;
    for (int g = 0; g <= K / 256; ++g) {
        const ds_u32x4 w4 = ds_philox4x32_10(g * 64 + lane, pos | (sid << 16), call, (unsigned)gid[b], seed_lo, seed_hi);
        const unsigned w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = (4 * g + e) * 64 + lane;
            if (c <= K) up[(size_t)c * L] = ds_u01(w[e]);
        }
    }
}
extern "C" int ds_philox_uniforms(const int64_t* gids, unsigned long long seed, int call, int rng_stream, float* u, int B,
                                  int L, int K, ds_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DS_CHECK_ARG(gids && u && B > 0 && L > 0 && L < 65536 && K > 0 && K % 256 == 0, "bad arguments");
    DS_CHECK_ARG(rng_stream == 0 || rng_stream == 1, "rng_stream is 0 (reverse steps) or 1 (q_sample)");
    hipLaunchKernelGGL(ds_philox_uniforms_kernel, dim3((B * L + 3) / 4), dim3(256), 0, stream, gids, (unsigned)seed,
                       (unsigned)(seed >> 32), call, (unsigned)rng_stream, u, B, L, K);
    DS_CHECK_LAUNCH();
    return 0;
}

// ---- the tails' host side: one description of a call (sampler.h TailCall), one checker, one launcher ----------------------
// Every rule of every tail, stated once.  A field a form does not have stays zero in the TailCall and passes its rule.
// positions of the canvas of W windows sharing n columns (see SampleJoint), 0 where the geometry does not exist
long long ds_joint_canvas_len(int W, int n, int ring) {
    if (W < 1 || n < 1 || n > DS_GRID_COLS / 2 || (ring && W < 2)) return 0;
    const long long hop = DS_GRID_COLS - n;
    return DS_GRID_ROWS * (ring ? W * hop : DS_GRID_COLS + (W - 1) * hop);
}

int ds_sample_tail_check(const TailCall& c) {
    const bool purity = c.kind == DS_TAIL_PURITY, guided = c.logits_u != nullptr;
    const bool composed = c.weights != nullptr || c.n_tracks != 0;        // a composed entry; its rules are the guided form's plus:
    const bool joint = c.joint;                                           // a joint entry: c.L is the canvas length, 0 if it has none
    const char* msg =
        (composed && !c.weights)                                          ? "null pointer (weights: the track weights)"
        : (composed && !(c.n_tracks >= 1 && c.n_tracks <= DS_MAX_TRACKS)) ? "n_tracks must be in 1 .. 4"
        : (composed && guided)  ? "caption tracks carry their own null condition: not together with logits_u"
        : (composed && purity)                                            ? "caption tracks have no purity form"
        : !(c.logits && c.xt && (c.u || c.gids) && c.out_tokens && (purity ? c.scratch && c.B > 0 : c.t && c.sched))
                                                                         ? "null pointer"
        : (joint && !c.fade)                                              ? "null pointer (fade: the overlap's column weights)"
        : (joint && c.windows < 1)                                        ? "windows must be at least 1"
        : (joint && !(c.overlap_cols >= 1 && c.overlap_cols <= DS_GRID_COLS / 2)) ? "overlap_cols must be in 1 .. 26"
        : (joint && c.ring && c.windows < 2)                              ? "a ring needs at least 2 windows"
        : (joint && ds_joint_canvas_len(c.windows, c.overlap_cols, c.ring) >= 65536)
                                                                          ? "the canvas must be shorter than 65536 positions"
        : (joint && c.mode != 0)                   ? "joint sampling holds positions clean (mode 0): it has no renoise mode"
        // (the unguided posterior tails never tested these three, and which calls are accepted is part of the ABI)
        : (!purity && (guided || composed || joint) && !(c.B > 0 && c.L > 0 && c.T > 0)) ? "B, L and T must be positive"
        : !(c.K == 256 || c.K == 512)                                     ? "codebook size must be 256 or 512"
        : (purity && !(c.L > 0 && c.L <= DS_PURITY_MAX_L))                ? "L must be in 1 .. 288"
        : !(c.logits_rows >= (joint ? DS_GRID_ROWS * DS_GRID_COLS : c.L) && c.L < 65536) ? "logits rows per sample"
        : (composed && c.track_stride < (size_t)c.B * c.logits_rows * c.K) ? "track_stride is smaller than one slab of logits"
        : (purity && c.remain < 0)                                        ? "remain must be >= 0"
        : (purity && !(c.weight >= 0.f && c.weight - c.weight == 0.f))    ? "the purity weight must be finite and >= 0"
        : (guided && !(c.scale - c.scale == 0.f))                         ? "the guidance scale must be finite"
        : !(c.trunc_k >= 0 && !(c.trunc_k > 0 && c.trunc_r >= 0.f))       ? "top-k and top-r truncation are exclusive"
        : !(c.mode == 0 || c.mode == 1)                                   ? "mode is 0 (clamp) or 1 (renoise)"
        : (c.mode == 1 && c.u) ? "renoise draws from the caption's Philox stream: not with caller uniforms"
        : (c.keep && !c.known)                                            ? "keep without known"
                                                                          : nullptr;
    if (!msg) return 0;
    ds_set_error("%s: %s", c.who, msg);
    return -1;
}

// The (K, noise source) ladder, once: LAUNCH_(NPL, RNG) launches that instantiation of the call's kernel family.  The families
// stand in the order held, plain, guided, purity, composed because hipcc emits the kernels in the order of their first mention: it
// is the order the code object has always had, which keeps its device code comparable byte for byte across host-side edits.
#define DS_TAIL_LADDER(LAUNCH_)                   \
    do {                                          \
        if (c.K == 256 && c.u) LAUNCH_(4, false); \
        else if (c.K == 256) LAUNCH_(4, true);    \
        else if (c.u) LAUNCH_(8, false);          \
        else LAUNCH_(8, true);                    \
    } while (0)
#define DS_TAIL_HOLD(NPL_, RNG_) hipLaunchKernelGGL((ds_sample_tail_hold_kernel<NPL_, RNG_>), grid, block, 0, stream, p, g, h)
#define DS_TAIL_PLAIN(NPL_, RNG_) hipLaunchKernelGGL((ds_sample_tail_kernel<NPL_, RNG_>), grid, block, 0, stream, p, g)
#define DS_TAIL_GUIDED(NPL_, RNG_) \
    hipLaunchKernelGGL((ds_sample_tail_guided_kernel<NPL_, RNG_>), grid, block, 0, stream, p, g, h, gd)
#define DS_TAIL_COMPOSED(NPL_, RNG_) \
    hipLaunchKernelGGL((ds_sample_tail_composed_kernel<NPL_, RNG_>), grid, block, 0, stream, p, g, h, cp)
#define DS_TAIL_JOINT(NPL_, RNG_) \
    hipLaunchKernelGGL((ds_sample_tail_joint_kernel<NPL_, RNG_>), grid, block, 0, stream, p, g, h, gd, jt)
#define DS_TAIL_PURITY(NPL_, RNG_)                                                                                           \
    do {                                                                                                                     \
        if (guided) hipLaunchKernelGGL((ds_sample_purity_rows_kernel<NPL_, RNG_, true>), grid, block, 0, stream, p, g, gd, pu); \
        else hipLaunchKernelGGL((ds_sample_purity_rows_kernel<NPL_, RNG_, false>), grid, block, 0, stream, p, g, gd, pu);   \
    } while (0)

int ds_sample_tail_launch(const TailCall& c) {
    hipStream_t stream = (hipStream_t)c.stream;
    const bool purity = c.kind == DS_TAIL_PURITY, guided = c.logits_u != nullptr, composed = c.weights != nullptr;
    const bool joint = c.joint;
    const long long cols = (long long)c.B * c.L;
    int* cand = (int*)c.scratch;                             // purity: the rows kernel leaves (candidate, key) per grid position
    float* key = purity ? (float*)(cand + cols) : nullptr;   //   here, and the select kernel writes the tokens
    const SampleParams p{c.logits, c.xt, c.t, c.u, c.sched, purity ? nullptr : c.out_tokens, c.dbg_log_pred, c.dbg_trunc,
                         c.dbg_post, c.B, c.L, c.T, c.initial, c.trunc_r, c.trunc_k, c.logits_rows};
    const SampleRng g{c.gids, (unsigned)c.seed, (unsigned)(c.seed >> 32), c.call};
    const SampleHold h{c.keep, c.known, c.mode};             // the guided kernels take it with keep == nullptr: unheld
    const SampleGuide gd{c.logits_u, c.scale};
    const SamplePurity pu{cand, key, c.dbg_sharp, c.weight};
    const SampleCompose cp{c.weights, c.track_stride, c.n_tracks};
    const SampleJoint jt{c.fade, c.windows, c.overlap_cols, c.ring, c.t_stride};
    const dim3 grid((unsigned)((cols + 3) / 4)), block(256);
    if (!joint && !purity && !guided && !composed && c.keep) DS_TAIL_LADDER(DS_TAIL_HOLD);
    else if (!joint && !purity && !guided && !composed) DS_TAIL_LADDER(DS_TAIL_PLAIN);
    else if (!joint && !purity && !composed) DS_TAIL_LADDER(DS_TAIL_GUIDED);
    else if (!joint && purity) DS_TAIL_LADDER(DS_TAIL_PURITY);
    else if (!joint) DS_TAIL_LADDER(DS_TAIL_COMPOSED);
    else DS_TAIL_LADDER(DS_TAIL_JOINT);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && purity) {
        hipLaunchKernelGGL(ds_sample_purity_select_kernel, dim3(c.B), dim3(256), 0, stream, c.xt, (const int*)cand,
                           (const float*)key, c.out_tokens, c.L, c.K, c.remain);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        ds_set_error("%s: launch failed: %s", c.who, hipGetErrorString(e));
        return -2;
    }
    if (c.dbg_key) e = hipMemcpyAsync(c.dbg_key, key, cols * sizeof(float), hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess && c.dbg_cand) e = hipMemcpyAsync(c.dbg_cand, cand, cols * sizeof(int), hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess) {
        ds_set_error("%s: hipMemcpyAsync: %s", c.who, hipGetErrorString(e));
        return -2;
    }
    return 0;
}
#undef DS_TAIL_LADDER
#undef DS_TAIL_HOLD
#undef DS_TAIL_PLAIN
#undef DS_TAIL_GUIDED
#undef DS_TAIL_PURITY
#undef DS_TAIL_COMPOSED
#undef DS_TAIL_JOINT

static int tail_run(const TailCall& c) {
    const int rc = ds_sample_tail_check(c);
    return rc ? rc : ds_sample_tail_launch(c);
}

// ---- the public tail entries: fill a TailCall, the entry's own null test (u for the uniform forms, gids for the _rng
// forms, logits_u for the guided ones: in a TailCall a null logits_u means unguided), check and launch
extern "C" int ds_sample_tail_ex(const float* logits, const int64_t* xt, const int64_t* t, const float* u,
                                 const float* sched, int64_t* out_tokens, float* dbg_log_pred, float* dbg_trunc,
                                 float* dbg_post, int B, int L, int K, int T, int initial, float trunc_r,
                                 int trunc_k, ds_stream_t stream) {
    DS_CHECK_ARG(u, "null pointer");
    TailCall c{__func__, DS_TAIL_POSTERIOR, stream};
    c.logits = logits; c.logits_rows = L; c.xt = xt; c.t = t; c.u = u; c.sched = sched; c.out_tokens = out_tokens;
    c.dbg_log_pred = dbg_log_pred; c.dbg_trunc = dbg_trunc; c.dbg_post = dbg_post;
    c.B = B; c.L = L; c.K = K; c.T = T; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    return tail_run(c);
}

extern "C" int ds_sample_tail(const float* logits, const int64_t* xt, const int64_t* t, const float* u,
                              const float* sched, int64_t* out_tokens, float* dbg_log_pred, float* dbg_trunc,
                              float* dbg_post, int B, int L, int K, int T, int initial, float trunc_r,
                              ds_stream_t stream) {
    return ds_sample_tail_ex(logits, xt, t, u, sched, out_tokens, dbg_log_pred, dbg_trunc, dbg_post, B, L, K, T, initial,
                             trunc_r, 0, stream);
}

extern "C" int ds_sample_tail_rng(const float* logits, const int64_t* xt, const int64_t* t, const int64_t* gids,
                                  unsigned long long seed, int call, const float* sched, int64_t* out_tokens, int B,
                                  int L, int K, int T, int initial, float trunc_r, int trunc_k, ds_stream_t stream) {
    DS_CHECK_ARG(gids, "null pointer");
    TailCall c{__func__, DS_TAIL_POSTERIOR, stream};
    c.logits = logits; c.logits_rows = L; c.xt = xt; c.t = t; c.sched = sched; c.out_tokens = out_tokens;
    c.gids = gids; c.seed = seed; c.call = call;
    c.B = B; c.L = L; c.K = K; c.T = T; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    return tail_run(c);
}

// region-held tails (see SampleHold): ds_sample_tail_ex / ds_sample_tail_rng + keep, known, mode
extern "C" int ds_sample_tail_hold(const float* logits, const int64_t* xt, const int64_t* t, const float* u,
                                   const float* sched, int64_t* out_tokens, float* dbg_log_pred, float* dbg_trunc,
                                   float* dbg_post, int B, int L, int K, int T, int initial, float trunc_r, int trunc_k,
                                   const unsigned char* keep, const int64_t* known, int mode, ds_stream_t stream) {
    DS_CHECK_ARG(u, "null pointer");
    TailCall c{__func__, DS_TAIL_POSTERIOR, stream};
    c.logits = logits; c.logits_rows = L; c.xt = xt; c.t = t; c.u = u; c.sched = sched; c.out_tokens = out_tokens;
    c.dbg_log_pred = dbg_log_pred; c.dbg_trunc = dbg_trunc; c.dbg_post = dbg_post;
    c.B = B; c.L = L; c.K = K; c.T = T; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.keep = keep; c.known = known; c.mode = mode;
    return tail_run(c);
}

extern "C" int ds_sample_tail_hold_rng(const float* logits, const int64_t* xt, const int64_t* t, const int64_t* gids,
                                       unsigned long long seed, int call, const float* sched, int64_t* out_tokens, int B,
                                       int L, int K, int T, int initial, float trunc_r, int trunc_k,
                                       const unsigned char* keep, const int64_t* known, int mode, ds_stream_t stream) {
    DS_CHECK_ARG(gids, "null pointer");
    TailCall c{__func__, DS_TAIL_POSTERIOR, stream};
    c.logits = logits; c.logits_rows = L; c.xt = xt; c.t = t; c.sched = sched; c.out_tokens = out_tokens;
    c.gids = gids; c.seed = seed; c.call = call;
    c.B = B; c.L = L; c.K = K; c.T = T; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.keep = keep; c.known = known; c.mode = mode;
    return tail_run(c);
}

// the guided tails (see SampleGuide): logits_u has the rows of logits_c; keep == nullptr: unheld
extern "C" int ds_sample_tail_guided(const float* logits_c, const float* logits_u, const int64_t* xt, const int64_t* t,
                                     const float* u, const float* sched, int64_t* out_tokens, float* dbg_log_pred,
                                     float* dbg_trunc, float* dbg_post, int B, int L, int K, int T, int initial,
                                     float trunc_r, int trunc_k, float scale, const unsigned char* keep,
                                     const int64_t* known, int mode, ds_stream_t stream) {
    DS_CHECK_ARG(u && logits_u, "null pointer (logits_u: the null-condition logits)");
    TailCall c{__func__, DS_TAIL_POSTERIOR, stream};
    c.logits = logits_c; c.logits_u = logits_u; c.scale = scale; c.logits_rows = L;
    c.xt = xt; c.t = t; c.u = u; c.sched = sched; c.out_tokens = out_tokens;
    c.dbg_log_pred = dbg_log_pred; c.dbg_trunc = dbg_trunc; c.dbg_post = dbg_post;
    c.B = B; c.L = L; c.K = K; c.T = T; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.keep = keep; c.known = known; c.mode = mode;
    return tail_run(c);
}

extern "C" int ds_sample_tail_guided_rng(const float* logits_c, const float* logits_u, const int64_t* xt, const int64_t* t,
                                         const int64_t* gids, unsigned long long seed, int call, const float* sched,
                                         int64_t* out_tokens, int B, int L, int K, int T, int initial, float trunc_r,
                                         int trunc_k, float scale, const unsigned char* keep, const int64_t* known, int mode,
                                         ds_stream_t stream) {
    DS_CHECK_ARG(gids && logits_u, "null pointer (logits_u: the null-condition logits)");
    TailCall c{__func__, DS_TAIL_POSTERIOR, stream};
    c.logits = logits_c; c.logits_u = logits_u; c.scale = scale; c.logits_rows = L;
    c.xt = xt; c.t = t; c.sched = sched; c.out_tokens = out_tokens;
    c.gids = gids; c.seed = seed; c.call = call;
    c.B = B; c.L = L; c.K = K; c.T = T; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.keep = keep; c.known = known; c.mode = mode;
    return tail_run(c);
}

// the composed tails (see SampleCompose): logits f32[n_tracks + 1][B * L][K], tracks first, the null condition last;
// weights f32[B][n_tracks][L] (finite: not checked here, see the header); keep == nullptr: unheld
extern "C" int ds_sample_tail_composed(const float* logits, const int64_t* xt, const int64_t* t, const float* u,
                                       const float* sched, int64_t* out_tokens, float* dbg_log_pred, float* dbg_trunc,
                                       float* dbg_post, int B, int L, int K, int T, int initial, float trunc_r, int trunc_k,
                                       int n_tracks, const float* weights, const unsigned char* keep, const int64_t* known,
                                       int mode, ds_stream_t stream) {
    DS_CHECK_ARG(u && weights, "null pointer (weights: the track weights)");
    TailCall c{__func__, DS_TAIL_POSTERIOR, stream};
    c.logits = logits; c.logits_rows = L; c.weights = weights; c.n_tracks = n_tracks;
    c.track_stride = B > 0 && L > 0 && K > 0 ? (size_t)B * L * K : 0;
    c.xt = xt; c.t = t; c.u = u; c.sched = sched; c.out_tokens = out_tokens;
    c.dbg_log_pred = dbg_log_pred; c.dbg_trunc = dbg_trunc; c.dbg_post = dbg_post;
    c.B = B; c.L = L; c.K = K; c.T = T; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.keep = keep; c.known = known; c.mode = mode;
    return tail_run(c);
}

extern "C" int ds_sample_tail_composed_rng(const float* logits, const int64_t* xt, const int64_t* t, const int64_t* gids,
                                           unsigned long long seed, int call, const float* sched, int64_t* out_tokens, int B,
                                           int L, int K, int T, int initial, float trunc_r, int trunc_k, int n_tracks,
                                           const float* weights, const unsigned char* keep, const int64_t* known, int mode,
                                           ds_stream_t stream) {
    DS_CHECK_ARG(gids && weights, "null pointer (weights: the track weights)");
    TailCall c{__func__, DS_TAIL_POSTERIOR, stream};
    c.logits = logits; c.logits_rows = L; c.weights = weights; c.n_tracks = n_tracks;
    c.track_stride = B > 0 && L > 0 && K > 0 ? (size_t)B * L * K : 0;
    c.xt = xt; c.t = t; c.sched = sched; c.out_tokens = out_tokens;
    c.gids = gids; c.seed = seed; c.call = call;
    c.B = B; c.L = L; c.K = K; c.T = T; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.keep = keep; c.known = known; c.mode = mode;
    return tail_run(c);
}

// the joint tails (see SampleJoint): logits (and logits_u, NULL: unguided) f32[B W lrows][K], one slab of lrows >= 265 rows per
// window; everything else on the canvas of ds_joint_canvas_len(W, n, ring) positions; keep == nullptr: unheld
static void joint_fields(TailCall& c, int B, int W, int n, int ring, const float* fade, int lrows) {
    c.joint = true; c.windows = W; c.overlap_cols = n; c.ring = ring != 0; c.fade = fade; c.t_stride = 1;
    c.B = B; c.logits_rows = lrows;
    const long long Lc = ds_joint_canvas_len(W, n, ring);
    c.L = Lc < 65536 ? (int)Lc : 0;       // (the checker refuses a canvas that does not exist or is too long before it reads L)
}

extern "C" int ds_sample_tail_joint(const float* logits, const float* logits_u, const int64_t* canvas, const int64_t* t,
                                    const float* u, const float* sched, int64_t* out_canvas, float* dbg_log_pred,
                                    float* dbg_trunc, float* dbg_post, int B, int W, int overlap_cols, int ring,
                                    const float* fade, int lrows, int K, int T, int initial, float trunc_r, int trunc_k,
                                    float scale, const unsigned char* keep, const int64_t* known, int mode,
                                    ds_stream_t stream) {
    DS_CHECK_ARG(u, "null pointer");
    TailCall c{__func__, DS_TAIL_POSTERIOR, stream};
    joint_fields(c, B, W, overlap_cols, ring, fade, lrows);
    c.logits = logits; c.logits_u = logits_u; c.scale = scale;
    c.xt = canvas; c.t = t; c.u = u; c.sched = sched; c.out_tokens = out_canvas;
    c.dbg_log_pred = dbg_log_pred; c.dbg_trunc = dbg_trunc; c.dbg_post = dbg_post;
    c.K = K; c.T = T; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.keep = keep; c.known = known; c.mode = mode;
    return tail_run(c);
}

extern "C" int ds_sample_tail_joint_rng(const float* logits, const float* logits_u, const int64_t* canvas, const int64_t* t,
                                        const int64_t* gids, unsigned long long seed, int call, const float* sched,
                                        int64_t* out_canvas, float* dbg_log_pred, float* dbg_trunc, float* dbg_post, int B,
                                        int W, int overlap_cols, int ring, const float* fade, int lrows, int K, int T,
                                        int initial, float trunc_r, int trunc_k, float scale, const unsigned char* keep,
                                        const int64_t* known, int mode, ds_stream_t stream) {
    DS_CHECK_ARG(gids, "null pointer");
    TailCall c{__func__, DS_TAIL_POSTERIOR, stream};
    joint_fields(c, B, W, overlap_cols, ring, fade, lrows);
    c.logits = logits; c.logits_u = logits_u; c.scale = scale;
    c.xt = canvas; c.t = t; c.sched = sched; c.out_tokens = out_canvas;
    c.gids = gids; c.seed = seed; c.call = call;
    c.dbg_log_pred = dbg_log_pred; c.dbg_trunc = dbg_trunc; c.dbg_post = dbg_post;
    c.K = K; c.T = T; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.keep = keep; c.known = known; c.mode = mode;
    return tail_run(c);
}

// the window rows of a canvas (ds_joint_gather_kernel): every rule checked before the launch
int ds_joint_gather_check(const char* who, const int64_t* canvas, const int64_t* win, int B, int W, int n, int ring, int copies) {
    const char* msg = !(canvas && win)                                    ? "null pointer"
                      : !(B > 0)                                          ? "B must be positive"
                      : W < 1                                             ? "windows must be at least 1"
                      : !(n >= 1 && n <= DS_GRID_COLS / 2)                ? "overlap_cols must be in 1 .. 26"
                      : (ring && W < 2)                                   ? "a ring needs at least 2 windows"
                      : !(copies >= 1 && copies <= 2)                     ? "copies is 1 or 2"
                                                                          : nullptr;
    if (!msg) return 0;
    ds_set_error("%s: %s", who, msg);
    return -1;
}
int ds_joint_gather_launch(const char* who, const int64_t* canvas, int64_t* win, int B, int W, int n, int ring, int copies,
                           ds_stream_t stream) {
    const int hop = DS_GRID_COLS - n, C = (int)(ds_joint_canvas_len(W, n, ring) / DS_GRID_ROWS);
    const long long total = (long long)B * W * DS_GRID_ROWS * DS_GRID_COLS;
    hipLaunchKernelGGL(ds_joint_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, canvas,
                       win, B, W, hop, C, copies);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        ds_set_error("%s: launch failed: %s", who, hipGetErrorString(e));
        return -2;
    }
    return 0;
}
extern "C" int ds_joint_gather(const int64_t* canvas, int64_t* win, int B, int W, int overlap_cols, int ring, int copies,
                               ds_stream_t stream) {
    const int rc = ds_joint_gather_check(__func__, canvas, win, B, W, overlap_cols, ring, copies);
    return rc ? rc : ds_joint_gather_launch(__func__, canvas, win, B, W, overlap_cols, ring, copies, stream);
}

// ---- purity-prior tails (see SamplePurity)
extern "C" int64_t ds_purity_scratch_bytes(int B, int L) {
    return B > 0 && L > 0 ? (int64_t)B * L * (int64_t)(sizeof(int) + sizeof(float)) : -1;
}

extern "C" int ds_sample_tail_purity(const float* logits, const float* logits_u, float scale, const int64_t* xt, const float* u,
                                     int remain, float weight, float trunc_r, int trunc_k, int lrows, void* scratch,
                                     int64_t* out_tokens, float* dbg_sharp, float* dbg_key, int32_t* dbg_cand, int B, int L,
                                     int K, ds_stream_t stream) {
    DS_CHECK_ARG(u, "null pointer");
    TailCall c{__func__, DS_TAIL_PURITY, stream};
    c.logits = logits; c.logits_u = logits_u; c.scale = scale; c.logits_rows = lrows;
    c.xt = xt; c.u = u; c.out_tokens = out_tokens;
    c.B = B; c.L = L; c.K = K; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.remain = remain; c.weight = weight; c.scratch = scratch;
    c.dbg_sharp = dbg_sharp; c.dbg_key = dbg_key; c.dbg_cand = dbg_cand;
    return tail_run(c);
}

extern "C" int ds_sample_tail_purity_rng(const float* logits, const float* logits_u, float scale, const int64_t* xt,
                                         const int64_t* gids, unsigned long long seed, int call, int remain, float weight,
                                         float trunc_r, int trunc_k, int lrows, void* scratch, int64_t* out_tokens,
                                         float* dbg_sharp, float* dbg_key, int32_t* dbg_cand, int B, int L, int K,
                                         ds_stream_t stream) {
    DS_CHECK_ARG(gids, "null pointer");
    TailCall c{__func__, DS_TAIL_PURITY, stream};
    c.logits = logits; c.logits_u = logits_u; c.scale = scale; c.logits_rows = lrows;
    c.xt = xt; c.out_tokens = out_tokens;
    c.gids = gids; c.seed = seed; c.call = call;
    c.B = B; c.L = L; c.K = K; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.remain = remain; c.weight = weight; c.scratch = scratch;
    c.dbg_sharp = dbg_sharp; c.dbg_key = dbg_key; c.dbg_cand = dbg_cand;
    return tail_run(c);
}

// ---- likelihood scoring: one term of a clip's variational bound per row -------------------------------
// Row b is a (clip, timestep) pair: x0[b] the clip's tokens, xt[b] its forward-diffused state at t[b], logits the denoiser's
// output on (xt[b], t[b]) in the [B * lrows][K] layout of the step driver (lrows >= L: rows >= L of a sample are never read).
// Per grid position -- one wavefront, the thread mapping and the expressions of ds_loss_tail_kernel, so the value is that
// kernel's bit for bit -- only the term t[b] selects is computed:
//   t == 0: nll = -log p_theta(x_0 | x_1)                                    (no true posterior is formed)
//   t >  0: kl  = KL(q(x_{t-1} | x_t, x_0) || p_theta(x_{t-1} | x_t))
// and never the auxiliary KL.  One workgroup per row: its 16 waves walk the positions (wave w takes w, w + 16, ...), leave the
// f32 values in LDS, and wave 0 widens them to double and adds them in a fixed order -- lane l sums positions l, l + 64, ...
// ascending, then the xor butterfly -- so term[b] depends on nothing but row b's own inputs: not on B, not on b, and no
// floating-point atomics.  A timestep outside [0, T) reads no table: the row's term (and map) is NaN.
// The two accumulations are spelled fmaf: ds_loss_tail_kernel's `acc += e * d` chains are contracted to fma by the compiler,
// while here, with fewer accumulators alive, it pairs the products into packed multiplies followed by separate adds -- one
// rounding more per product, values a last place apart (tests/test_hip_score.py holds the two kernels together).
#define DS_SCORE_WAVES 16
template <int NPL>
__global__ __launch_bounds__(64 * DS_SCORE_WAVES) void ds_score_tail_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ x0, const int64_t* __restrict__ xt,
    const int64_t* __restrict__ t, const float* __restrict__ sched, double* __restrict__ term, float* __restrict__ dbg_pos,
    int lrows, int L, int T) {
    constexpr int K = NPL * 64;
    __shared__ float s_pos[DS_PURITY_MAX_L];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const int tt = (int)t[b];
    const bool t_ok = tt >= 0 && tt < T;
    for (int pos = w; pos < L; pos += DS_SCORE_WAVES) {
        const size_t col = (size_t)b * L + pos;
        float val = __builtin_nanf("");
        if (t_ok) {
            float v[NPL];
            const float* lg = logits + ((size_t)b * lrows + pos) * K;
#pragma unroll
            for (int j = 0; j < NPL; ++j) v[j] = lg[j * 64 + lane];
            float mx = v[0];
#pragma unroll
            for (int j = 1; j < NPL; ++j) mx = fmaxf(mx, v[j]);
            mx = wmaxf(mx);
            double se = 0.0;
#pragma unroll
            for (int j = 0; j < NPL; ++j) se += exp((double)v[j] - (double)mx);
            const double lse64 = log(wsumd(se));
            float lp[NPL], ls[NPL];
            const int x0c = (int)x0[col], xtc = (int)xt[col];
#pragma unroll
            for (int j = 0; j < NPL; ++j) {
                lp[j] = fminf(fmaxf((float)(((double)v[j] - (double)mx) - lse64), -70.f), 0.f);   // log p_theta(x_0 | x_t)
                ls[j] = (j * 64 + lane) == x0c ? 0.f : LOG_ZERO_F;                                 // log one-hot of x_0
            }
            const float ls_m = x0c == K ? 0.f : LOG_ZERO_F;
            float pm[NPL], pm_m;
            ds_posterior<NPL>(lp, -70.f, xtc, K, lane, sched, T + 1, tt, pm, pm_m);    // model posterior
            if (tt == 0) {
                float n = 0.f;
#pragma unroll
                for (int j = 0; j < NPL; ++j) n = fmaf(expf(ls[j]), pm[j], n);
                n = fmaf(expf(ls_m), pm_m, wsumf(n));
                val = -n;
            } else {
                float pr[NPL], pr_m;
                ds_posterior<NPL>(ls, ls_m, xtc, K, lane, sched, T + 1, tt, pr, pr_m);     // true posterior
                float a = 0.f;
#pragma unroll
                for (int j = 0; j < NPL; ++j) a = fmaf(expf(pr[j]), pr[j] - pm[j], a);
                a = fmaf(expf(pr_m), pr_m - pm_m, wsumf(a));
                val = a;
            }
        }
        if (lane == 0) {
            s_pos[pos] = val;
            if (dbg_pos) dbg_pos[col] = val;
        }
    }
    __syncthreads();
    if (w == 0) {
        double acc = 0.0;
        for (int pos = lane; pos < L; pos += 64) acc += (double)s_pos[pos];
        acc = wsumd(acc);
        if (lane == 0) term[b] = acc;
    }
}

int ds_score_tail_check(const ScoreCall& c) {
    const char* msg = !(c.logits && c.x0 && c.xt && c.t && c.sched && c.term) ? "null pointer"
                      : !(c.K == 256 || c.K == 512)                          ? "codebook size must be 256 or 512"
                      : !(c.L > 0 && c.L <= DS_PURITY_MAX_L)                  ? "L must be in 1 .. 288"
                      : !(c.lrows >= c.L)                                     ? "logits rows per sample"
                      : !(c.B >= 1)                                           ? "B must be at least 1"
                      : !(c.T > 0)                                            ? "T must be positive"
                                                                              : nullptr;
    if (!msg) return 0;
    ds_set_error("%s: %s", c.who, msg);
    return -1;
}

int ds_score_tail_launch(const ScoreCall& c) {
    hipStream_t stream = (hipStream_t)c.stream;
    const dim3 grid((unsigned)c.B), block(64 * DS_SCORE_WAVES);
    if (c.K == 256)
        hipLaunchKernelGGL((ds_score_tail_kernel<4>), grid, block, 0, stream, c.logits, c.x0, c.xt, c.t, c.sched, c.term,
                           c.dbg_pos, c.lrows, c.L, c.T);
    else
        hipLaunchKernelGGL((ds_score_tail_kernel<8>), grid, block, 0, stream, c.logits, c.x0, c.xt, c.t, c.sched, c.term,
                           c.dbg_pos, c.lrows, c.L, c.T);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        ds_set_error("%s: launch failed: %s", c.who, hipGetErrorString(e));
        return -2;
    }
    return 0;
}

extern "C" int ds_score_tail(const float* logits, const int64_t* x0, const int64_t* xt, const int64_t* t, const float* sched,
                             double* term, float* dbg_pos, int lrows, int B, int L, int K, int T, ds_stream_t stream) {
    const ScoreCall c{__func__, stream, logits, x0, xt, t, sched, term, dbg_pos, lrows, B, L, K, T};
    const int rc = ds_score_tail_check(c);
    return rc ? rc : ds_score_tail_launch(c);
}
