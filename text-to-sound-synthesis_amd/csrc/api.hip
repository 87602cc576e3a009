// C ABI glue: error strings, the public gather-GEMM entry, and the native denoiser driver that
// enqueues the whole Text2ImageTransformer forward (transformer_utils.py:421-443) -- 19 blocks x 11
// launches -- from C++ on one HIP stream (no Python in the per-layer loop).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "sampler.h"

static thread_local char g_err[512] = "";

void ds_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" int ds_version(void) { return 100; }
extern "C" const char* ds_last_error_string(void) { return g_err; }

static void fill(GemmParams& p, const ds_gemm_desc* d) {
    p.A = d->A; p.W = d->W; p.bias = d->bias; p.R = d->R; p.C = d->C;
    p.M = d->M; p.N = d->N; p.K = d->K;
    p.lda = d->lda; p.ldw = d->ldw > 0 ? d->ldw : d->K; p.ldc = d->ldc; p.ldr = d->ldr;
    p.groups = d->groups > 0 ? d->groups : 1;
    p.a_gstride = d->a_gstride; p.w_gstride = d->w_gstride; p.c_gstride = d->c_gstride;
    p.pro = d->pro; p.act = d->act; p.store = d->store; p.f16_round = d->f16_round;
    p.w3_plane = d->w3_plane;
    p.out_scale = d->out_scale;
    p.a_split = d->a_split; p.c_split = d->c_split; p.a_plane = d->a_plane; p.c_plane = d->c_plane;
    p.attn_kv = d->attn_kv; p.attn_heads = d->attn_heads; p.attn_nkey = d->attn_nkey; p.attn_qplane = d->attn_qplane;
    p.row_off = 0;
    p.pro_scale = d->pro_scale; p.pro_shift = d->pro_shift;
    p.rows_per_sample = d->rows_per_sample;
    p.Cin = d->Cin; p.H = d->H; p.W_ = d->Wd; p.up = d->up; p.taps = d->taps; p.dil = d->dil;
    p.ct_r = d->ct_r; p.ct_p = d->ct_p; p.ct_tin = d->ct_tin;
}

extern "C" int ds_gemm(const ds_gemm_desc* d, ds_stream_t stream) {
    DS_CHECK_ARG(d && d->A && d->W && d->C, "null pointer");
    DS_CHECK_ARG(d->pro == DS_PRO_NONE || d->pro == DS_PRO_LRELU || (d->pro_scale && d->pro_shift && d->Cin > 0),
                 "affine prologue needs pro_scale/pro_shift/Cin");
    DS_CHECK_ARG(d->store != DS_STORE_BATCH_T || d->rows_per_sample > 0, "BATCH_T store needs rows_per_sample");
    DS_CHECK_ARG(d->R == nullptr || d->store == DS_STORE_ROW, "residual only with row-major store");
    GemmParams p;
    memset(&p, 0, sizeof(p));
    fill(p, d);
    return ds_launch_gemm(p, (hipStream_t)stream, d->loader);
}

// the conv-family loaders of the descriptor (DS_LOAD_CONV2D / CONV1D / CONVT1D / DENSE) on the fp16 matrix cores; W =
// split_f16x2 planes.  loader 0 (DS_LOAD_DENSE) in the descriptor of a caller that predates the other loaders meant the
// 3x3 conv: the conv2d geometry fields (H > 0 and K == 9 Cin) select it.
extern "C" int ds_conv2d_f16x2(const ds_gemm_desc* d, ds_stream_t stream) {
    DS_CHECK_ARG(d && d->A && d->W && d->C, "null pointer");
    DS_CHECK_ARG(d->w3_plane > 0, "w3_plane (plane stride of the split weights) is required");
    GemmParams p;
    memset(&p, 0, sizeof(p));
    fill(p, d);
    const int loader = (d->loader == DS_LOAD_DENSE && d->H > 0 && d->Cin > 0 && d->K == 9 * d->Cin) ? DS_LOAD_CONV2D : d->loader;
    return ds_launch_conv2d_f16x2(p, (hipStream_t)stream, loader);
}

extern "C" int ds_gemm_f16x2(const ds_gemm_desc* d, ds_stream_t stream) {
    DS_CHECK_ARG(d && d->A && d->W && d->C, "null pointer");
    DS_CHECK_ARG(d->loader == DS_LOAD_DENSE && d->pro == DS_PRO_NONE && !d->f16_round,
                 "f16x2 is the dense, no-prologue kernel (groups: see ds_launch_gemm_f16x2)");
    DS_CHECK_ARG(d->w3_plane > 0, "w3_plane (plane stride of the split weights) is required");
    DS_CHECK_ARG(d->store != DS_STORE_BATCH_T || d->rows_per_sample > 0, "BATCH_T store needs rows_per_sample");
    DS_CHECK_ARG(d->R == nullptr || d->store == DS_STORE_ROW, "residual only with row-major store");
    GemmParams p;
    memset(&p, 0, sizeof(p));
    fill(p, d);
    return ds_launch_gemm_f16x2(p, (hipStream_t)stream);
}

int ds_launch_gemm_f16x2_multi(const GemmParams* ps, int n, int cfg, hipStream_t stream);   // gemm_f16x2.hip
extern "C" int ds_gemm_f16x2_multi(const ds_gemm_desc* descs, int n, int cfg, ds_stream_t stream) {
    DS_CHECK_ARG(descs && n >= 1 && n <= 4, "1 .. 4 descriptors");
    GemmParams ps[4];
    memset(ps, 0, sizeof(ps));
    for (int i = 0; i < n; ++i) {
        const ds_gemm_desc* d = descs + i;
        DS_CHECK_ARG(d->A && d->W && d->C, "null pointer");
        DS_CHECK_ARG(d->loader == DS_LOAD_DENSE && d->pro == DS_PRO_NONE && !d->f16_round && d->w3_plane > 0,
                     "f16x2 is the dense, no-prologue kernel; w3_plane is required");
        fill(ps[i], d);
    }
    return ds_launch_gemm_f16x2_multi(ps, n, cfg, (hipStream_t)stream);
}

// ---- denoiser ---------------------------------------------------------------------------------------
struct ds_denoiser {
    ds_denoiser_desc d;
    std::vector<const float*> lp;  // [n_layer][DS_LP_COUNT]
    std::vector<const void*> lp3;  // split weights (same indexing), empty = fp32-MFMA mode
    std::vector<float> osc;        // f16x2: 2^-s per weight
    const void* w_logits3 = nullptr;
    float logits_osc = 1.f;
    int split_mode = DS_SPLIT_NONE;
    int pad_rows = 1;              // padded-row mode allowed (ds_denoiser_set_row_padding; see rows_per_sample())
    float* range_peak = nullptr;   // f16x2 range monitor (ds_denoiser_set_range_monitor): max |GELU2 output| of every forward
    float S3(int layer, int slot) const { return osc.empty() ? 1.f : osc[(size_t)layer * DS_LP_COUNT + slot]; }
    const float* P(int layer, int slot) const { return lp[(size_t)layer * DS_LP_COUNT + slot]; }
    const void* P3(int layer, int slot) const { return lp3.empty() ? nullptr : lp3[(size_t)layer * DS_LP_COUNT + slot]; }
};

extern "C" int ds_denoiser_set_split_weights(ds_denoiser* h, int mode, const void* const* split3,
                                             const float* out_scales, const void* w_logits3, float logits_scale) {
    DS_CHECK_ARG(h, "null handle");
    if (mode == DS_SPLIT_NONE || !split3) {
        h->lp3.clear();
        h->osc.clear();
        h->w_logits3 = nullptr;
        h->split_mode = DS_SPLIT_NONE;
        return 0;
    }
    DS_CHECK_ARG(mode == DS_SPLIT_F16X2, "unknown split mode");
    DS_CHECK_ARG(out_scales && logits_scale > 0.f, "f16x2 needs the output scales");
    static const int need[6] = {DS_LP_W_QKV, DS_LP_W_PROJ1, DS_LP_W_Q2, DS_LP_W_PROJ2, DS_LP_W_FC1, DS_LP_W_FC2};
    for (int l = 0; l < h->d.n_layer; ++l)
        for (int s : need) DS_CHECK_ARG(split3[(size_t)l * DS_LP_COUNT + s], "missing split weight");
    DS_CHECK_ARG(w_logits3, "missing split logits weight");
    h->lp3.assign(split3, split3 + (size_t)h->d.n_layer * DS_LP_COUNT);
    h->osc.assign(out_scales, out_scales + (size_t)h->d.n_layer * DS_LP_COUNT);
    h->w_logits3 = w_logits3;
    h->logits_osc = logits_scale;
    h->split_mode = mode;
    return 0;
}

extern "C" int ds_denoiser_create(const ds_denoiser_desc* desc, const void* const* layer_ptrs, ds_denoiser** out) {
    DS_CHECK_ARG(desc && layer_ptrs && out, "null pointer");
    DS_CHECK_ARG(desc->n_embd == 1024 && desc->n_embd == desc->n_head * 64, "built for n_embd 1024, head dim 64");
    DS_CHECK_ARG(desc->n_codes == 256 || desc->n_codes == 512, "codebook size must be 256 or 512");
    DS_CHECK_ARG(desc->cond_dim % 32 == 0 && desc->cond_len <= 96 && desc->seq_len <= 288, "unsupported lengths");
    DS_CHECK_ARG(desc->tok_emb && desc->pos_emb && desc->lnf_g && desc->lnf_b && desc->w_logits && desc->b_logits &&
                     desc->sched,
                 "null weight pointer");
    for (int i = 0; i < desc->n_layer * DS_LP_COUNT; ++i) DS_CHECK_ARG(layer_ptrs[i], "null layer pointer");
    ds_denoiser* h = new ds_denoiser;
    h->d = *desc;
    h->lp.resize((size_t)desc->n_layer * DS_LP_COUNT);
    for (size_t i = 0; i < h->lp.size(); ++i) h->lp[i] = (const float*)layer_ptrs[i];
    *out = h;
    return 0;
}

extern "C" void ds_denoiser_destroy(ds_denoiser* h) { delete h; }

// workspace carve (floats): x, hn, qkv, att, fc, logits
struct Carve {
    float *x, *hn, *qkv, *att, *fc, *logits;
    float* kvimg;   // f16x2 mode: self-attention K / V^T images, inside the qkv region after the Q planes
};
// floats occupied by the K / V^T images of one attention over Lk keys (4 fp16 planes of nkey*64 per sample and head)
static size_t attn_img_floats(int B, int heads, int Lk) { return (size_t)B * heads * 4 * ds_attn_nkey(Lk) * 64 / 2; }
// Rows per sample of the activation matrices.  PADDED-ROW MODE (sampling steps in f16x2 mode at batch sizes whose GEMMs
// take the per-sample program, i.e. B = 64): every sample occupies PS_ROWS = 272 rows = 17 packed 16-row groups instead
// of L = 265, so a sample's tile starts on a packed group, and the tile's ninth block row is the 16 rows 256..271 on the
// 16x16x32 MFMA instead of 32 rows (gemm_f16x2_ps.hip NB16: -5 % MFMA work).  The 7 extra rows per sample start as zeros
// (ds_embed_rows), stay finite through every layer (LayerNorm of a constant row = its shift), are extra QUERIES of the
// attention (the ninth query tile exists anyway) but never keys (Lk = L masks them), and the sampler reads the L real
// rows of each sample (TailCall::logits_rows).  Rows 256..264 of a sample are then summed in another order than by the
// 4-wave programs (same products): equal to ~1e-7 relative, not bit-identical across batch sizes.
static const int PS_ROWS = 272;
bool ds_gemm_f16x2_ps_taken(int B, int N);   // gemm_f16x2.hip: the dispatch rule of the per-sample program, forced tile included
static int rows_per_sample(const ds_denoiser* h, int B) {
    const int L = h->d.seq_len;
    if (!h->pad_rows || h->split_mode != DS_SPLIT_F16X2 || L > PS_ROWS || L <= PS_ROWS - 16) return L;
    return ds_gemm_f16x2_ps_taken(B, h->d.n_embd) ? PS_ROWS : L;    // the N = 1024 GEMMs' grid decides (gemm_f16x2.hip)
}
extern "C" int ds_denoiser_rows_per_sample(const ds_denoiser* h, int B) { return h && B > 0 ? rows_per_sample(h, B) : -1; }
extern "C" int ds_denoiser_set_row_padding(ds_denoiser* h, int on) {
    DS_CHECK_ARG(h, "null handle");
    h->pad_rows = on != 0;
    return 0;
}

// Range monitor of the f16x2 mode.  FC2's operand, the GELU2 outputs, is the one split site of the denoiser that is not
// bounded by a normalisation, and it exists only as packed planes inside a forward: with `peak` set (a device float the
// caller zeroes), every forward folds max |hi plane| of every layer's GELU2 output into it (one small launch per layer).
// The hi plane clamps at 65504, so a peak of 65504 says the split saturated; the caller then recomputes in the fp32 mode
// (modeling/transformer.py range_exceeded).  nullptr switches it off; the fp32 mode never looks at it.
int ds_amax_packed_hi(const void* plane, int M, int K, float* out, ds_stream_t stream);   // misc.hip
extern "C" int ds_denoiser_set_range_monitor(ds_denoiser* h, float* peak) {
    DS_CHECK_ARG(h, "null handle");
    h->range_peak = peak;
    return 0;
}

static size_t carve(const ds_denoiser* h, int B, void* ws, Carve* c, int Lp = 0) {
    const size_t M = (size_t)B * (Lp > 0 ? Lp : PS_ROWS > h->d.seq_len ? PS_ROWS : h->d.seq_len), D = h->d.n_embd;
    const size_t M16 = (M + 15) & ~(size_t)15;   // hn / att / fc double as packed split planes (rows padded to 16)
    size_t off = 0;
    auto take = [&](size_t n) {
        float* p = ws ? (float*)ws + off : nullptr;
        off += (n + 63) & ~(size_t)63;
        return p;
    };
    Carve t;
    t.x = take(M * D);
    t.hn = take(M16 * D);
    // fp32 modes: [M][3D] rows.  f16x2 mode: Q planes (M*D floats) + the K / V^T images (padded to nkey key slots)
    const size_t qkv_ready = M * D + attn_img_floats(B, h->d.n_head, h->d.seq_len);   // (nkey covers 272 rows too)
    t.qkv = take(qkv_ready > M * 3 * D ? qkv_ready : M * 3 * D);
    t.kvimg = t.qkv ? t.qkv + M * D : nullptr;
    t.att = take(M16 * D);
    t.fc = take(M16 * D * h->d.mlp_mult);
    t.logits = take(M * h->d.n_codes);
    if (c) *c = t;
    return off * sizeof(float);
}

extern "C" int64_t ds_denoiser_workspace_bytes(const ds_denoiser* h, int B) {
    return h && B > 0 ? (int64_t)carve(h, B, nullptr, nullptr) : -1;
}
// caption K/V cache: fp32 modes [n_layer][B*cond_len][2D]; f16x2 mode [n_layer] K / V^T images + one layer of fp32
// rows as scratch for ds_denoiser_cond_kv.  The buffer is sized for either.
static size_t kv_layer_img_floats(const ds_denoiser* h, int B) { return attn_img_floats(B, h->d.n_head, h->d.cond_len); }
extern "C" int64_t ds_denoiser_kv_bytes(const ds_denoiser* h, int B) {
    if (!h || B <= 0) return -1;
    const size_t rows = (size_t)B * h->d.cond_len * 2 * h->d.n_embd;
    const size_t f32 = (size_t)h->d.n_layer * rows, img = (size_t)h->d.n_layer * kv_layer_img_floats(h, B) + rows;
    return (int64_t)((f32 > img ? f32 : img) * sizeof(float));
}

// ---- optional per-launch timing of the denoiser's GEMMs (bench.py's roofline leg) ---------------
struct ProfRec { hipEvent_t a, b; double flops; int tile; };
extern int g_last_tile;  // gemm_f32.hip
static bool g_prof = false;
static double g_prof_row_frac = 1.0;   // real rows / launched rows of the GEMMs being recorded (padded-row mode: 265 / 272)
static std::vector<ProfRec> g_recs;

extern "C" int ds_profile_enable(int on) {
    g_prof = on != 0;
    return 0;
}
// Waits for the recorded launches; per GEMM program c (0: 128x128, 1: 128x64, 2: 64x64 tiles, 3: the per-sample
// ping-pong program on full tiles, 4: on half tiles -- each is its own kernel symbol) returns summed duration ms[c],
// algorithmic flops[c] (2MNK) and launches[c] for the first n <= 5 programs; the four-program form folds 4 into 3.
extern "C" int ds_profile_collect_n(double* ms, double* flops, int64_t* launches, int n) {
    DS_CHECK_ARG(ms && flops && launches && n >= 4 && n <= 5, "bad arguments");
    for (int c = 0; c < n; ++c) { ms[c] = 0.0; flops[c] = 0.0; launches[c] = 0; }
    for (auto& r : g_recs) {
        const int c = r.tile < n ? r.tile : n - 1;
        float e = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&e, r.a, r.b) == hipSuccess) ms[c] += e;
        flops[c] += r.flops;
        launches[c] += 1;
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    g_recs.clear();
    return 0;
}
extern "C" int ds_profile_collect(double* ms, double* flops, int64_t* launches) {
    return ds_profile_collect_n(ms, flops, launches, 4);
}

static int dense(const float* A, int lda, const float* W, const float* bias, const float* R, float* C, int ldc,
                 int M, int N, int K, int act, hipStream_t s, int store = DS_STORE_ROW, int rps = 0,
                 const void* W3 = nullptr, int split_mode = DS_SPLIT_NONE, float osc = 1.f,
                 long long a_plane = 0, long long c_plane = 0, void* attn_kv = nullptr, int attn_heads = 0,
                 int attn_nkey = 0, long long attn_qplane = 0, long long w_plane = 0) {
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.A = A; p.W = W; p.bias = bias; p.R = R; p.C = C;
    p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldw = K; p.ldc = ldc; p.ldr = ldc;
    p.groups = 1; p.act = act; p.store = store; p.rows_per_sample = rps;
    if (W3) {  // fp32-class GEMM on the fp16 matrix cores
        p.W = (const float*)W3;
        p.w3_plane = (long long)N * K;
        p.out_scale = osc;
        p.a_split = a_plane > 0; p.a_plane = a_plane;   // f16x2 only: A and W are packed split planes
        if (a_plane > 0) p.w3_plane = (long long)((N + 15) & ~15) * K;
        p.c_split = c_plane > 0; p.c_plane = c_plane;
        p.attn_kv = attn_kv; p.attn_heads = attn_heads; p.attn_nkey = attn_nkey; p.attn_qplane = attn_qplane;
        if (w_plane > 0) p.w3_plane = w_plane;   // a row range of a larger packed weight keeps that weight's stride
    }
    auto launch = [&]() {
        if (!W3) return ds_launch_gemm(p, s, DS_LOAD_DENSE);
        return ds_launch_gemm_f16x2(p, s);
    };
    if (!g_prof) return launch();
    ProfRec r;
    r.flops = 2.0 * M * N * K * g_prof_row_frac;   // algorithmic: the padding rows of the padded-row mode do not count
    if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) {
        ds_set_error("profile: hipEventCreate failed");
        return -2;
    }
    (void)hipEventRecord(r.a, s);
    const int rc = launch();
    (void)hipEventRecord(r.b, s);
    r.tile = g_last_tile;
    g_recs.push_back(r);
    return rc;
}

#define TRY(x)            \
    do {                  \
        int rc_ = (x);    \
        if (rc_) return rc_; \
    } while (0)

extern "C" int ds_denoiser_cond_kv(const ds_denoiser* h, const float* cond, int B, float* kv, ds_stream_t stream) {
    DS_CHECK_ARG(h && cond && kv && B > 0, "bad arguments");
    const int D = h->d.n_embd, Mc = B * h->d.cond_len;
    if (h->split_mode == DS_SPLIT_F16X2) {   // attention-ready K / V^T images per layer (see ds_denoiser_kv_bytes)
        const size_t per = kv_layer_img_floats(h, B);
        float* rows = kv + (size_t)h->d.n_layer * per;
        for (int l = 0; l < h->d.n_layer; ++l) {
            TRY(dense(cond, h->d.cond_dim, h->P(l, DS_LP_W_KV2), h->P(l, DS_LP_B_KV2), nullptr, rows, 2 * D, Mc, 2 * D,
                      h->d.cond_dim, DS_ACT_NONE, (hipStream_t)stream));
            TRY(ds_attn_pack_kv(rows, 2 * D, D, kv + (size_t)l * per, B, h->d.n_head, h->d.cond_len, stream));
        }
        return 0;
    }
    for (int l = 0; l < h->d.n_layer; ++l)
        TRY(dense(cond, h->d.cond_dim, h->P(l, DS_LP_W_KV2), h->P(l, DS_LP_B_KV2), nullptr,
                  kv + (size_t)l * Mc * 2 * D, 2 * D, Mc, 2 * D, h->d.cond_dim, DS_ACT_NONE, (hipStream_t)stream));
    return 0;
}

// Lp: rows per sample of every activation matrix (d.seq_len, or PS_ROWS in padded-row mode: layout 0 only)
static int forward_impl(const ds_denoiser* h, const int64_t* tokens, const int64_t* t, const float* kv, int B,
                        const Carve& w, float* logits, int layout, hipStream_t s, int Lp, bool zero_kv_pad = true) {
    const ds_denoiser_desc& d = h->d;
    const int D = d.n_embd, Lv = d.seq_len, L = Lp, M = B * L, Mc = B * d.cond_len, F = D * d.mlp_mult;
    DS_CHECK_ARG(Lp == Lv || (layout == 0 && Lp > Lv), "padded rows need the row-major logits layout");
    g_prof_row_frac = (double)Lv / Lp;
    const float scale = 0.125f;  // 1/sqrt(64), transformer_utils.py:48
    // f16x2 mode: attention follows the GEMM arithmetic, and every GEMM input is produced as PACKED SPLIT PLANES
    // (common.h ds_packed_off; two fp16 planes in the bytes of the fp32 buffer, rows padded to 16) by the kernel
    // before it, with the same ds_split_hi/lo code the GEMM loader would run -- results are bit-identical to
    // splitting in the loader, and the GEMM stages its tiles by LDS-DMA.
    const bool f16 = h->split_mode == DS_SPLIT_F16X2;
    const long long M16 = (M + 15) & ~15;
    const long long pD = f16 ? M16 * D : 0, pF = f16 ? M16 * F : 0;
    auto adaln = [&](int l, int slot) {
        return f16 ? ds_adaln_split(w.x, w.hn, M, L, D, h->P(l, slot), t, s)
                   : ds_adaln(w.x, w.hn, M, L, D, h->P(l, slot), t, s);
    };
    auto lnorm = [&](const float* g, const float* b_) {
        return f16 ? ds_layernorm_split(w.x, w.hn, M, D, g, b_, s) : ds_layernorm(w.x, w.hn, M, D, g, b_, s);
    };
    auto attn = [&](const float* q, int ldq, const float* k, const float* v, int ldkv, int Lk) {
        return ds_attention(q, ldq, k, ldkv, v, ldkv, w.att, D, B, d.n_head, L, Lk, scale, s);
    };
    // f16x2 mode: the QKV / cross-Q GEMMs write attention-ready operands (Q planes at w.qkv, K / V^T images at
    // w.kvimg; the caption images come from ds_denoiser_cond_kv) and the attention kernel stages them by LDS-DMA
    const long long qpl = (long long)M * D;   // halves per Q plane ([B][heads][L][64])
    const int nkS = ds_attn_nkey(L);
    auto lin_attn = [&](int l, int slot, int bslot, int N, int n_weight, void* imgs) {
        return dense(w.hn, D, h->P(l, slot), h->P(l, bslot), nullptr, w.qkv, N, M, N, D, DS_ACT_NONE, s, DS_STORE_ATTN, L,
                     h->P3(l, slot), h->split_mode, h->S3(l, slot), pD, 0, imgs, d.n_head, nkS, qpl,
                     (long long)n_weight * D);
    };
    auto attn_ready = [&](const void* imgs, int Lk) {
        return ds_attention_f16x2_ready(w.qkv, qpl, imgs, w.att, D, B, d.n_head, L, Lk, scale, s);
    };
    // key slots L..nkey-1 of the self-attention images are never written: they must read as zero (a chain of steps over one
    // workspace zeroes them in its first step only: nothing between two of its steps touches the workspace)
    if (f16 && zero_kv_pad) {
        hipError_t e = hipMemsetAsync(w.kvimg, 0, attn_img_floats(B, d.n_head, L) * sizeof(float), s);
        if (e != hipSuccess) {
            ds_set_error("forward: hipMemsetAsync: %s", hipGetErrorString(e));
            return -2;
        }
    }
    // y = act(A W^T + b) (+ R) for layer-l weight `slot`; A (and optionally C) pre-split in f16x2 mode
    auto lin = [&](int l, int slot, int bslot, const float* A, int lda, long long ap, const float* R, float* C, int N,
                   int K, int act, long long cp) {
        return dense(A, lda, h->P(l, slot), h->P(l, bslot), R, C, N, M, N, K, act, s, DS_STORE_ROW, L, h->P3(l, slot),
                     h->split_mode, h->S3(l, slot), ap, cp);
    };
    TRY(ds_embed_rows(tokens, d.tok_emb, d.pos_emb, w.x, B, Lv, L, D, s));
    for (int l = 0; l < d.n_layer; ++l) {
        // x += attn1(ln1(x, t))
        TRY(adaln(l, DS_LP_ADALN1));
        if (f16) {
            TRY(lin_attn(l, DS_LP_W_QKV, DS_LP_B_QKV, 3 * D, 3 * D, w.kvimg));   // Q planes + K / V^T images
            TRY(attn_ready(w.kvimg, Lv));                                          // padded rows are queries, never keys
        } else {
            TRY(lin(l, DS_LP_W_QKV, DS_LP_B_QKV, w.hn, D, pD, nullptr, w.qkv, 3 * D, D, DS_ACT_NONE, 0));
            TRY(attn(w.qkv, 3 * D, w.qkv + D, w.qkv + 2 * D, 3 * D, Lv));
        }
        TRY(lin(l, DS_LP_W_PROJ1, DS_LP_B_PROJ1, w.att, D, pD, w.x, w.x, D, D, DS_ACT_NONE, 0));
        // x += attn2(ln1_1(x, t), cond)
        TRY(adaln(l, DS_LP_ADALN2));
        if (f16) {
            TRY(lin_attn(l, DS_LP_W_Q2, DS_LP_B_Q2, D, D, nullptr));
            TRY(attn_ready(kv + (size_t)l * kv_layer_img_floats(h, B), d.cond_len));
        } else {
            TRY(lin(l, DS_LP_W_Q2, DS_LP_B_Q2, w.hn, D, pD, nullptr, w.qkv, D, D, DS_ACT_NONE, 0));
            const float* kvl = kv + (size_t)l * Mc * 2 * D;
            TRY(attn(w.qkv, D, kvl, kvl + D, 2 * D, d.cond_len));
        }
        TRY(lin(l, DS_LP_W_PROJ2, DS_LP_B_PROJ2, w.att, D, pD, w.x, w.x, D, D, DS_ACT_NONE, 0));
        // x += mlp(ln2(x))
        TRY(lnorm(h->P(l, DS_LP_LN2_G), h->P(l, DS_LP_LN2_B)));
        TRY(lin(l, DS_LP_W_FC1, DS_LP_B_FC1, w.hn, D, pD, nullptr, w.fc, F, D, DS_ACT_GELU2, pF));
        if (f16 && h->range_peak) TRY(ds_amax_packed_hi(w.fc, M, F, h->range_peak, s));
        TRY(lin(l, DS_LP_W_FC2, DS_LP_B_FC2, w.fc, F, pF, w.x, w.x, D, F, DS_ACT_NONE, 0));
    }
    TRY(lnorm(d.lnf_g, d.lnf_b));
    if (layout == 0)
        TRY(dense(w.hn, D, d.w_logits, d.b_logits, nullptr, logits, d.n_codes, M, d.n_codes, D, DS_ACT_NONE, s,
                  DS_STORE_ROW, 0, h->w_logits3, h->split_mode, h->logits_osc, pD));
    else
        TRY(dense(w.hn, D, d.w_logits, d.b_logits, nullptr, logits, L, M, d.n_codes, D, DS_ACT_NONE, s,
                  DS_STORE_BATCH_T, L, h->w_logits3, h->split_mode, h->logits_osc, pD));
    return 0;
}

extern "C" int ds_denoiser_forward(const ds_denoiser* h, const int64_t* tokens, const int64_t* t, const float* kv,
                                   int B, void* workspace, float* logits, int logits_layout, ds_stream_t stream) {
    DS_CHECK_ARG(h && tokens && t && kv && workspace && logits && B > 0, "bad arguments");
    Carve w;
    carve(h, B, workspace, &w, h->d.seq_len);
    return forward_impl(h, tokens, t, kv, B, w, logits, logits_layout, (hipStream_t)stream, h->d.seq_len);
}

// ---- sampling steps and chains: forward + sampling tail (sampler.h TailCall) -------------------------------------------------
// One step, as every ds_denoiser_step* / ds_denoiser_sample* entry describes it.  The entry fills the tail's who, stream, B,
// noise source, truncation, `initial` and its hold / guidance / purity fields; aim_tail adds what the handle and the workspace
// give.  kv and workspace are at the forward's batch: B, or n_cond B with tokens2.
struct StepCall {
    TailCall tail;
    const int64_t* tokens_in = nullptr;
    int64_t* tokens_out = nullptr;
    const int64_t* t = nullptr;        // drives the network (AdaLN)
    const int64_t* t_post = nullptr;   // drives the posterior, nullptr: t.  They differ only for the skip-step sampler
                                       //   (sample_fast, diffusion_transformer.py:796-803: q_posterior with t - skip_step)
    const float* kv = nullptr;
    void* workspace = nullptr;
    // non-null: classifier-free guidance (sampler.hip SampleGuide) -- ONE forward at batch 2B on the tokens duplicated into this
    // i64[2B][seq_len] scratch (two async copies on the call's stream), rows 0 .. B-1 under the captions, rows B .. 2B-1 under
    // the null condition (kv: ds_denoiser_cond_kv of the caption embeddings followed by the null embeddings; t, t_post: the
    // caller's B entries repeated, the posterior reads the first B), and the tail mixes the two halves of the logits
    int64_t* tokens2 = nullptr;
    // conditions per clip with tokens2: 2 guided; n_tracks + 1 composed (sampler.hip SampleCompose: tokens2 is
    // i64[n_cond B][seq_len], kv is track-major with the null condition last, and the tail reads n_cond slabs of the logits)
    int n_cond = 2;
    // joint-window sampling (tail.joint; sampler.hip SampleJoint): tokens_in / tokens_out are canvases i64[B][tail.L], tokens2 is
    // the gather's target i64[n_cond B W][seq_len] -- always given, n_cond 1 (unguided) or 2 -- the forward runs at batch
    // n_cond B W, and the posterior reads entry b W of its timestep vector (one per window row, like the network's)
    bool zero_kv_pad = true;           // forward_impl: false in the later steps of a chain
};

static int step_error(const StepCall& s, int rc, const char* what, const char* detail) {
    ds_set_error("%s: %s%s", s.tail.who, what, detail);
    return rc;
}

// Completes s.tail: the logits where the forward will leave them, the tokens, and the handle's constants.  Host arithmetic
// only.  The purity tail reads no timestep and no schedule table: t, sched and T stay zero.  Returns the rows per sample.
static int aim_tail(const ds_denoiser* h, StepCall& s, Carve* w) {
    TailCall& c = s.tail;
    const int Bw = c.joint ? c.B * c.windows : c.B;      // rows of one condition
    const int Bf = s.tokens2 ? s.n_cond * Bw : Bw, Lp = rows_per_sample(h, Bf);
    carve(h, Bf, s.workspace, w, Lp);
    if (!c.joint) c.L = h->d.seq_len;                    // (joint: the canvas length, set by the entry)
    c.K = h->d.n_codes;
    c.logits = w->logits; c.logits_rows = Lp;
    const bool composed = c.weights != nullptr;
    c.logits_u = s.tokens2 && !composed && !(c.joint && s.n_cond == 1) ? w->logits + (size_t)Bw * Lp * c.K : nullptr;
    c.track_stride = composed ? (size_t)c.B * Lp * c.K : 0;
    c.xt = s.tokens_in; c.out_tokens = s.tokens_out;
    if (c.kind == DS_TAIL_POSTERIOR) {
        c.t = s.t_post ? s.t_post : s.t; c.sched = h->d.sched; c.T = h->d.n_steps;
    }
    return Lp;
}

// the driver's pointer rules, then every rule of the tail on the call as run_step will launch it: before anything is enqueued
static int step_check(const ds_denoiser* h, StepCall s) {
    if (!(h && s.tokens_in && s.t && s.kv && s.workspace && s.tokens_out && s.tail.B > 0))
        return step_error(s, -1, "bad arguments", "");
    Carve w;
    aim_tail(h, s, &w);
    return ds_sample_tail_check(s.tail);
}

static int run_step(const ds_denoiser* h, StepCall& s) {
    hipStream_t stream = (hipStream_t)s.tail.stream;
    const size_t n_tok = (size_t)s.tail.B * h->d.seq_len;
    const bool joint = s.tail.joint;
    if (joint)
        TRY(ds_joint_gather_launch(s.tail.who, s.tokens_in, s.tokens2, s.tail.B, s.tail.windows, s.tail.overlap_cols, s.tail.ring,
                                   s.n_cond, s.tail.stream));
    for (int half = 0; !joint && s.tokens2 && half < s.n_cond; ++half) {
        hipError_t e = hipMemcpyAsync(s.tokens2 + half * n_tok, s.tokens_in, n_tok * sizeof(int64_t), hipMemcpyDeviceToDevice,
                                      stream);
        if (e != hipSuccess) return step_error(s, -2, "hipMemcpyAsync: ", hipGetErrorString(e));
    }
    Carve w;
    const int Lp = aim_tail(h, s, &w);
    const int Bw = joint ? s.tail.B * s.tail.windows : s.tail.B;
    TRY(forward_impl(h, s.tokens2 ? s.tokens2 : s.tokens_in, s.t, s.kv, s.tokens2 ? s.n_cond * Bw : Bw, w, w.logits, 0,
                     stream, Lp, s.zero_kv_pad));
    return ds_sample_tail_launch(s.tail);
}

static int step(const ds_denoiser* h, StepCall& s) {
    TRY(step_check(h, s));
    return run_step(h, s);
}

// A whole chain enqueued from C++ (DiffusionTransformer.sample's loop, diffusion_transformer.py:639-641, and sample_fast's,
// :790-804): nothing returns to the host between steps.  What differs between the chain entries is data: t_steps, a DEVICE
// array, holds t_stride entries per call -- the network's timestep vector first, the posterior's at post_off (0: none).
struct ChainCall {
    int64_t* tokens;          // in: the start state, out: the result; [B][seq_len] like tokens_tmp, the other end of the ping-pong
    int64_t* tokens_tmp;
    const int64_t* t_steps;
    int n_calls;
    size_t t_stride, post_off;
    const int* remain;        // purity: HOST int[n_calls], read before the entry returns; nullptr otherwise
};

// `first` describes call 0 (tail.call = call0; tail.initial: the start state is all-[MASK]).  Call k draws Philox call index
// call0 + k, only call 0 can be `initial`, and only call 0 zeroes the self-attention images' padding (nothing between two steps
// of a chain touches the workspace).  The result lands in `tokens` after an even number of calls and is copied there after an
// odd one.  Every call's arguments are checked before the first is enqueued.
static int run_chain(const ds_denoiser* h, const StepCall& first, const ChainCall& ch) {
    StepCall s = first;
    if (!(ch.tokens && ch.tokens_tmp && ch.t_steps && ch.n_calls >= 0)) return step_error(s, -1, "bad arguments", "");
    s.tokens_in = ch.tokens; s.tokens_out = ch.tokens_tmp; s.t = ch.t_steps;
    TRY(step_check(h, s));
    for (int k = 0; ch.remain && k < ch.n_calls; ++k) {
        s.tail.remain = ch.remain[k];
        TRY(step_check(h, s));
    }
    int64_t *cur = ch.tokens, *nxt = ch.tokens_tmp;
    for (int k = 0; k < ch.n_calls; ++k) {
        s.tokens_in = cur; s.tokens_out = nxt;
        s.t = ch.t_steps + k * ch.t_stride;
        s.t_post = ch.post_off ? s.t + ch.post_off : nullptr;
        s.zero_kv_pad = k == 0;
        s.tail.initial = first.tail.initial && k == 0;
        s.tail.call = first.tail.call + k;
        if (ch.remain) s.tail.remain = ch.remain[k];
        TRY(run_step(h, s));
        int64_t* sw = cur; cur = nxt; nxt = sw;
    }
    if (cur != ch.tokens) {
        hipError_t e = hipMemcpyAsync(ch.tokens, cur, (size_t)s.tail.B * s.tail.L * sizeof(int64_t), hipMemcpyDeviceToDevice,
                                      (hipStream_t)s.tail.stream);
        if (e != hipSuccess) return step_error(s, -2, "hipMemcpyAsync: ", hipGetErrorString(e));
    }
    return 0;
}

// ---- the public entries: fill a StepCall (and a ChainCall), the entry's own null test -- u for the uniform forms, gids for
// the _rng forms, and what only this family requires -- then step() or run_chain()
extern "C" int ds_denoiser_step_ex(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t,
                                   const int64_t* t_post, const float* kv, const float* u, int B, int initial,
                                   float trunc_r, int trunc_k, void* workspace, int64_t* tokens_out,
                                   ds_stream_t stream) {
    DS_CHECK_ARG(u, "bad arguments");
    StepCall s{{__func__, DS_TAIL_POSTERIOR, stream}};
    TailCall& c = s.tail;
    c.B = B; c.u = u; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    s.tokens_in = tokens_in; s.tokens_out = tokens_out; s.t = t; s.t_post = t_post; s.kv = kv; s.workspace = workspace;
    return step(h, s);
}

extern "C" int ds_denoiser_step(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t, const float* kv,
                                const float* u, int B, int initial, float trunc_r, void* workspace,
                                int64_t* tokens_out, ds_stream_t stream) {
    return ds_denoiser_step_ex(h, tokens_in, t, nullptr, kv, u, B, initial, trunc_r, 0, workspace, tokens_out, stream);
}

// the same step with the noise drawn inside the sampler kernel (sampler.hip: Philox keyed by seed, counter = global
// caption id gids[b], sampler call index, grid position, class): what a caption draws does not depend on the batch it is
// in, on its position in it, or on the rank that runs it
extern "C" int ds_denoiser_step_rng(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t,
                                    const int64_t* t_post, const float* kv, const int64_t* gids,
                                    unsigned long long seed, int call, int B, int initial, float trunc_r, int trunc_k,
                                    void* workspace, int64_t* tokens_out, ds_stream_t stream) {
    DS_CHECK_ARG(gids, "bad arguments");
    StepCall s{{__func__, DS_TAIL_POSTERIOR, stream}};
    TailCall& c = s.tail;
    c.B = B; c.gids = gids; c.seed = seed; c.call = call; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    s.tokens_in = tokens_in; s.tokens_out = tokens_out; s.t = t; s.t_post = t_post; s.kv = kv; s.workspace = workspace;
    return step(h, s);
}

// the chain of ds_denoiser_step_rng: t_steps is i64[n_calls][2][B] -- per call the network's timestep vector and the
// posterior's (equal except for the skip-step sampler)
extern "C" int ds_denoiser_sample_rng(const ds_denoiser* h, int64_t* tokens, int64_t* tokens_tmp, const int64_t* t_steps,
                                      int n_calls, const float* kv, const int64_t* gids, unsigned long long seed,
                                      int call0, int B, int initial, float trunc_r, int trunc_k, void* workspace,
                                      ds_stream_t stream) {
    DS_CHECK_ARG(gids, "bad arguments");
    StepCall s{{__func__, DS_TAIL_POSTERIOR, stream}};
    TailCall& c = s.tail;
    c.B = B; c.gids = gids; c.seed = seed; c.call = call0; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    s.kv = kv; s.workspace = workspace;
    return run_chain(h, s, ChainCall{tokens, tokens_tmp, t_steps, n_calls, 2 * (size_t)B, (size_t)B, nullptr});
}

// ---- region-held sampling (inpainting / continuation; sampler.hip SampleHold): the three entries above with keep u8[B][seq_len]
// (non-zero: the position is held), known i64[B][seq_len] (its token) and mode (0 clamp, 1 renoise: in-kernel noise only).
// keep == NULL runs the unheld kernels.
extern "C" int ds_denoiser_step_hold(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t,
                                     const int64_t* t_post, const float* kv, const float* u, int B, int initial,
                                     float trunc_r, int trunc_k, const unsigned char* keep, const int64_t* known, int mode,
                                     void* workspace, int64_t* tokens_out, ds_stream_t stream) {
    DS_CHECK_ARG(u, "bad arguments");
    StepCall s{{__func__, DS_TAIL_POSTERIOR, stream}};
    TailCall& c = s.tail;
    c.B = B; c.u = u; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.keep = keep; c.known = known; c.mode = mode;
    s.tokens_in = tokens_in; s.tokens_out = tokens_out; s.t = t; s.t_post = t_post; s.kv = kv; s.workspace = workspace;
    return step(h, s);
}

extern "C" int ds_denoiser_step_hold_rng(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t,
                                         const int64_t* t_post, const float* kv, const int64_t* gids,
                                         unsigned long long seed, int call, int B, int initial, float trunc_r, int trunc_k,
                                         const unsigned char* keep, const int64_t* known, int mode, void* workspace,
                                         int64_t* tokens_out, ds_stream_t stream) {
    DS_CHECK_ARG(gids, "bad arguments");
    StepCall s{{__func__, DS_TAIL_POSTERIOR, stream}};
    TailCall& c = s.tail;
    c.B = B; c.gids = gids; c.seed = seed; c.call = call; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.keep = keep; c.known = known; c.mode = mode;
    s.tokens_in = tokens_in; s.tokens_out = tokens_out; s.t = t; s.t_post = t_post; s.kv = kv; s.workspace = workspace;
    return step(h, s);
}

// the whole chain: `tokens` holds the caller's start state (held positions included), known stays constant over the calls;
// in renoise mode call k re-draws the held positions at the posterior timestep of that call minus one (stream 1, call
// call0 + k: the counters of the reverse step itself)
extern "C" int ds_denoiser_sample_hold_rng(const ds_denoiser* h, int64_t* tokens, int64_t* tokens_tmp,
                                           const int64_t* t_steps, int n_calls, const float* kv, const int64_t* gids,
                                           unsigned long long seed, int call0, int B, int initial, float trunc_r,
                                           int trunc_k, const unsigned char* keep, const int64_t* known, int mode,
                                           void* workspace, ds_stream_t stream) {
    DS_CHECK_ARG(gids, "bad arguments");
    StepCall s{{__func__, DS_TAIL_POSTERIOR, stream}};
    TailCall& c = s.tail;
    c.B = B; c.gids = gids; c.seed = seed; c.call = call0; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.keep = keep; c.known = known; c.mode = mode;
    s.kv = kv; s.workspace = workspace;
    return run_chain(h, s, ChainCall{tokens, tokens_tmp, t_steps, n_calls, 2 * (size_t)B, (size_t)B, nullptr});
}

// ---- classifier-free guidance (StepCall::tokens2, which these entries require); workspace: ds_denoiser_workspace_bytes(h, 2B);
// keep == NULL: unheld
extern "C" int ds_denoiser_step_guided(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t,
                                       const int64_t* t_post, const float* kv, const float* u, int B, int initial,
                                       float trunc_r, int trunc_k, float scale, const unsigned char* keep,
                                       const int64_t* known, int mode, int64_t* tokens2, void* workspace,
                                       int64_t* tokens_out, ds_stream_t stream) {
    DS_CHECK_ARG(u && tokens2, "bad arguments");
    StepCall s{{__func__, DS_TAIL_POSTERIOR, stream}};
    TailCall& c = s.tail;
    c.B = B; c.u = u; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.keep = keep; c.known = known; c.mode = mode; c.scale = scale;
    s.tokens_in = tokens_in; s.tokens_out = tokens_out; s.t = t; s.t_post = t_post; s.kv = kv; s.workspace = workspace;
    s.tokens2 = tokens2;
    return step(h, s);
}

extern "C" int ds_denoiser_step_guided_rng(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t,
                                           const int64_t* t_post, const float* kv, const int64_t* gids,
                                           unsigned long long seed, int call, int B, int initial, float trunc_r, int trunc_k,
                                           float scale, const unsigned char* keep, const int64_t* known, int mode,
                                           int64_t* tokens2, void* workspace, int64_t* tokens_out, ds_stream_t stream) {
    DS_CHECK_ARG(gids && tokens2, "bad arguments");
    StepCall s{{__func__, DS_TAIL_POSTERIOR, stream}};
    TailCall& c = s.tail;
    c.B = B; c.gids = gids; c.seed = seed; c.call = call; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.keep = keep; c.known = known; c.mode = mode; c.scale = scale;
    s.tokens_in = tokens_in; s.tokens_out = tokens_out; s.t = t; s.t_post = t_post; s.kv = kv; s.workspace = workspace;
    s.tokens2 = tokens2;
    return step(h, s);
}

// the whole guided chain: t_steps is i64[n_calls][2][2B]
extern "C" int ds_denoiser_sample_guided_rng(const ds_denoiser* h, int64_t* tokens, int64_t* tokens_tmp,
                                             const int64_t* t_steps, int n_calls, const float* kv, const int64_t* gids,
                                             unsigned long long seed, int call0, int B, int initial, float trunc_r,
                                             int trunc_k, float scale, const unsigned char* keep, const int64_t* known,
                                             int mode, int64_t* tokens2, void* workspace, ds_stream_t stream) {
    DS_CHECK_ARG(gids && tokens2, "bad arguments");
    StepCall s{{__func__, DS_TAIL_POSTERIOR, stream}};
    TailCall& c = s.tail;
    c.B = B; c.gids = gids; c.seed = seed; c.call = call0; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.keep = keep; c.known = known; c.mode = mode; c.scale = scale;
    s.kv = kv; s.workspace = workspace; s.tokens2 = tokens2;
    return run_chain(h, s, ChainCall{tokens, tokens_tmp, t_steps, n_calls, 4 * (size_t)B, 2 * (size_t)B, nullptr});
}

// ---- caption tracks (sampler.hip SampleCompose; StepCall::tokens2 with n_cond = n_tracks + 1, which these entries require);
// workspace: ds_denoiser_workspace_bytes(h, (n_tracks + 1) B); keep == NULL: unheld.  n_tracks sizes the forward, so its range
// is the entry's own test; the tail's checker states it again for the tail entries.
#define DS_COMPOSED_ARGS(noise_) \
    DS_CHECK_ARG((noise_) && tokensN && weights, "bad arguments (null noise source, tokensN or weights)"); \
    DS_CHECK_ARG(n_tracks >= 1 && n_tracks <= DS_MAX_TRACKS, "n_tracks must be in 1 .. 4")
extern "C" int ds_denoiser_step_composed(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t,
                                         const int64_t* t_post, const float* kv, const float* u, int B, int initial,
                                         float trunc_r, int trunc_k, int n_tracks, const float* weights,
                                         const unsigned char* keep, const int64_t* known, int mode, int64_t* tokensN,
                                         void* workspace, int64_t* tokens_out, ds_stream_t stream) {
    DS_COMPOSED_ARGS(u);
    StepCall s{{__func__, DS_TAIL_POSTERIOR, stream}};
    TailCall& c = s.tail;
    c.B = B; c.u = u; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.keep = keep; c.known = known; c.mode = mode; c.weights = weights; c.n_tracks = n_tracks;
    s.tokens_in = tokens_in; s.tokens_out = tokens_out; s.t = t; s.t_post = t_post; s.kv = kv; s.workspace = workspace;
    s.tokens2 = tokensN; s.n_cond = n_tracks + 1;
    return step(h, s);
}

extern "C" int ds_denoiser_step_composed_rng(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t,
                                             const int64_t* t_post, const float* kv, const int64_t* gids,
                                             unsigned long long seed, int call, int B, int initial, float trunc_r,
                                             int trunc_k, int n_tracks, const float* weights, const unsigned char* keep,
                                             const int64_t* known, int mode, int64_t* tokensN, void* workspace,
                                             int64_t* tokens_out, ds_stream_t stream) {
    DS_COMPOSED_ARGS(gids);
    StepCall s{{__func__, DS_TAIL_POSTERIOR, stream}};
    TailCall& c = s.tail;
    c.B = B; c.gids = gids; c.seed = seed; c.call = call; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.keep = keep; c.known = known; c.mode = mode; c.weights = weights; c.n_tracks = n_tracks;
    s.tokens_in = tokens_in; s.tokens_out = tokens_out; s.t = t; s.t_post = t_post; s.kv = kv; s.workspace = workspace;
    s.tokens2 = tokensN; s.n_cond = n_tracks + 1;
    return step(h, s);
}

// the whole composed chain: t_steps is i64[n_calls][2][(n_tracks + 1) B]
extern "C" int ds_denoiser_sample_composed_rng(const ds_denoiser* h, int64_t* tokens, int64_t* tokens_tmp,
                                               const int64_t* t_steps, int n_calls, const float* kv, const int64_t* gids,
                                               unsigned long long seed, int call0, int B, int initial, float trunc_r,
                                               int trunc_k, int n_tracks, const float* weights, const unsigned char* keep,
                                               const int64_t* known, int mode, int64_t* tokensN, void* workspace,
                                               ds_stream_t stream) {
    DS_COMPOSED_ARGS(gids);
    StepCall s{{__func__, DS_TAIL_POSTERIOR, stream}};
    TailCall& c = s.tail;
    c.B = B; c.gids = gids; c.seed = seed; c.call = call0; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    c.keep = keep; c.known = known; c.mode = mode; c.weights = weights; c.n_tracks = n_tracks;
    s.kv = kv; s.workspace = workspace; s.tokens2 = tokensN; s.n_cond = n_tracks + 1;
    const size_t Bf = (size_t)(n_tracks + 1) * B;
    return run_chain(h, s, ChainCall{tokens, tokens_tmp, t_steps, n_calls, 2 * Bf, Bf, nullptr});
}
#undef DS_COMPOSED_ARGS

// ---- joint-window sampling (sampler.hip SampleJoint): every step gathers the W window rows of each clip's canvas into tokensN
// (ds_joint_gather, n_cond copies), runs ONE forward at batch n_cond B W and the joint tail onto the canvas.  n_cond 1: unguided,
// 2: guided at `scale`.  What sizes the forward -- B, W, overlap_cols, ring, n_cond, the handle's grid -- is the entries' own
// test; the tail's checker states the geometry again for the tail entries.
static int joint_args(const ds_denoiser* h, StepCall& s, const void* noise, int B, int W, int n, int ring, int n_cond,
                      const float* fade, float scale, const unsigned char* keep, const int64_t* known, int mode,
                      int64_t* tokensN) {
    const char* msg = !(h && noise && tokensN && fade) ? "bad arguments (null handle, noise source, tokensN or fade)"
                      : h->d.seq_len != DS_GRID_ROWS * DS_GRID_COLS ? "joint sampling is built for the 5 x 53 grid (seq_len 265)"
                      : !(B > 0)                        ? "B must be positive"
                      : W < 1                           ? "windows must be at least 1"
                      : !(n >= 1 && n <= DS_GRID_COLS / 2) ? "overlap_cols must be in 1 .. 26"
                      : (ring && W < 2)                 ? "a ring needs at least 2 windows"
                      : !(n_cond == 1 || n_cond == 2)   ? "n_cond is 1 (unguided) or 2 (guided)"
                      : ds_joint_canvas_len(W, n, ring) >= 65536 ? "the canvas must be shorter than 65536 positions"
                                                        : nullptr;
    if (msg) return step_error(s, -1, msg, "");
    TailCall& c = s.tail;
    c.joint = true; c.windows = W; c.overlap_cols = n; c.ring = ring != 0; c.fade = fade; c.t_stride = W;
    c.B = B; c.L = (int)ds_joint_canvas_len(W, n, ring);
    c.scale = scale; c.keep = keep; c.known = known; c.mode = mode;
    s.tokens2 = tokensN; s.n_cond = n_cond;
    return 0;
}

extern "C" int ds_denoiser_step_joint(const ds_denoiser* h, const int64_t* canvas_in, const int64_t* t, const int64_t* t_post,
                                      const float* kv, const float* u, int B, int W, int overlap_cols, int ring, int n_cond,
                                      const float* fade, int initial, float trunc_r, int trunc_k, float scale,
                                      const unsigned char* keep, const int64_t* known, int mode, int64_t* tokensN,
                                      void* workspace, int64_t* canvas_out, ds_stream_t stream) {
    StepCall s{{__func__, DS_TAIL_POSTERIOR, stream}};
    TRY(joint_args(h, s, u, B, W, overlap_cols, ring, n_cond, fade, scale, keep, known, mode, tokensN));
    TailCall& c = s.tail;
    c.u = u; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    s.tokens_in = canvas_in; s.tokens_out = canvas_out; s.t = t; s.t_post = t_post; s.kv = kv; s.workspace = workspace;
    return step(h, s);
}

extern "C" int ds_denoiser_step_joint_rng(const ds_denoiser* h, const int64_t* canvas_in, const int64_t* t,
                                          const int64_t* t_post, const float* kv, const int64_t* gids, unsigned long long seed,
                                          int call, int B, int W, int overlap_cols, int ring, int n_cond, const float* fade,
                                          int initial, float trunc_r, int trunc_k, float scale, const unsigned char* keep,
                                          const int64_t* known, int mode, int64_t* tokensN, void* workspace,
                                          int64_t* canvas_out, ds_stream_t stream) {
    StepCall s{{__func__, DS_TAIL_POSTERIOR, stream}};
    TRY(joint_args(h, s, gids, B, W, overlap_cols, ring, n_cond, fade, scale, keep, known, mode, tokensN));
    TailCall& c = s.tail;
    c.gids = gids; c.seed = seed; c.call = call; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    s.tokens_in = canvas_in; s.tokens_out = canvas_out; s.t = t; s.t_post = t_post; s.kv = kv; s.workspace = workspace;
    return step(h, s);
}

// the whole joint chain: canvas / canvas_tmp i64[B][Lc] are the two ends of the ping-pong, t_steps is i64[n_calls][2][n_cond B W]
extern "C" int ds_denoiser_sample_joint_rng(const ds_denoiser* h, int64_t* canvas, int64_t* canvas_tmp, const int64_t* t_steps,
                                            int n_calls, const float* kv, const int64_t* gids, unsigned long long seed,
                                            int call0, int B, int W, int overlap_cols, int ring, int n_cond, const float* fade,
                                            int initial, float trunc_r, int trunc_k, float scale, const unsigned char* keep,
                                            const int64_t* known, int mode, int64_t* tokensN, void* workspace,
                                            ds_stream_t stream) {
    StepCall s{{__func__, DS_TAIL_POSTERIOR, stream}};
    TRY(joint_args(h, s, gids, B, W, overlap_cols, ring, n_cond, fade, scale, keep, known, mode, tokensN));
    TailCall& c = s.tail;
    c.gids = gids; c.seed = seed; c.call = call0; c.initial = initial; c.trunc_r = trunc_r; c.trunc_k = trunc_k;
    s.kv = kv; s.workspace = workspace;
    const size_t Bf = (size_t)n_cond * B * W;
    return run_chain(h, s, ChainCall{canvas, canvas_tmp, t_steps, n_calls, 2 * Bf, Bf, nullptr});
}

// ---- purity-prior sampling (sampler.hip SamplePurity): forward + purity tail.  tokens2 == NULL: the forward at batch B; else
// the guided forward at batch 2B, the tail mixing the two halves of the logits.  scratch: ds_purity_scratch_bytes, a pointer
// of its own.
extern "C" int ds_denoiser_step_purity(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t, const float* kv,
                                       const float* u, int B, int remain, float weight, float trunc_r, int trunc_k, float scale,
                                       int64_t* tokens2, void* workspace, void* scratch, int64_t* tokens_out,
                                       ds_stream_t stream) {
    DS_CHECK_ARG(u, "bad arguments");
    StepCall s{{__func__, DS_TAIL_PURITY, stream}};
    TailCall& c = s.tail;
    c.B = B; c.u = u; c.scale = scale;
    c.trunc_r = trunc_r; c.trunc_k = trunc_k; c.remain = remain; c.weight = weight; c.scratch = scratch;
    s.tokens_in = tokens_in; s.tokens_out = tokens_out; s.t = t; s.kv = kv; s.workspace = workspace; s.tokens2 = tokens2;
    return step(h, s);
}

extern "C" int ds_denoiser_step_purity_rng(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t, const float* kv,
                                           const int64_t* gids, unsigned long long seed, int call, int B, int remain,
                                           float weight, float trunc_r, int trunc_k, float scale, int64_t* tokens2,
                                           void* workspace, void* scratch, int64_t* tokens_out, ds_stream_t stream) {
    DS_CHECK_ARG(gids, "bad arguments");
    StepCall s{{__func__, DS_TAIL_PURITY, stream}};
    TailCall& c = s.tail;
    c.B = B; c.gids = gids; c.seed = seed; c.call = call;
    c.scale = scale; c.trunc_r = trunc_r; c.trunc_k = trunc_k; c.remain = remain; c.weight = weight; c.scratch = scratch;
    s.tokens_in = tokens_in; s.tokens_out = tokens_out; s.t = t; s.kv = kv; s.workspace = workspace; s.tokens2 = tokens2;
    return step(h, s);
}

// the whole purity chain: t_steps is i64[n_calls][B] (guided: [n_calls][2B]), remain a HOST array read here
extern "C" int ds_denoiser_sample_purity_rng(const ds_denoiser* h, int64_t* tokens, int64_t* tokens_tmp, const int64_t* t_steps,
                                             const int* remain, int n_calls, const float* kv, const int64_t* gids,
                                             unsigned long long seed, int call0, int B, float weight, float trunc_r,
                                             int trunc_k, float scale, int64_t* tokens2, void* workspace, void* scratch,
                                             ds_stream_t stream) {
    DS_CHECK_ARG(gids && remain, "bad arguments");
    StepCall s{{__func__, DS_TAIL_PURITY, stream}};
    TailCall& c = s.tail;
    c.B = B; c.gids = gids; c.seed = seed; c.call = call0;
    c.scale = scale; c.trunc_r = trunc_r; c.trunc_k = trunc_k; c.weight = weight; c.scratch = scratch;
    s.kv = kv; s.workspace = workspace; s.tokens2 = tokens2;
    return run_chain(h, s, ChainCall{tokens, tokens_tmp, t_steps, n_calls, (tokens2 ? 2 : 1) * (size_t)B, 0, remain});
}

// ---- likelihood scoring (sampler.hip ds_score_tail_kernel): B independent (clip, timestep) rows -- x_t = ds_q_sample_rng(x0, t;
// stream 1 of gids[b], call), the forward on the step driver's activation layout (padded rows where rows_per_sample says so),
// the score tail on the logits where the forward left them.  Every rule is checked before anything is enqueued.
extern "C" int ds_denoiser_score_rng(const ds_denoiser* h, const int64_t* x0, const int64_t* t, const float* kv,
                                     const int64_t* gids, unsigned long long seed, int call, int B, void* workspace,
                                     int64_t* xt_scratch, double* term, float* dbg_pos, ds_stream_t stream) {
    DS_CHECK_ARG(h && x0 && t && kv && gids && workspace && xt_scratch && term, "null pointer");
    DS_CHECK_ARG(B >= 1, "B must be at least 1");
    const int Lp = rows_per_sample(h, B);
    Carve w;
    carve(h, B, workspace, &w, Lp);
    const ScoreCall c{__func__, stream, w.logits, x0, xt_scratch, t, h->d.sched, term, dbg_pos, Lp, B, h->d.seq_len,
                      h->d.n_codes, h->d.n_steps};
    TRY(ds_score_tail_check(c));
    TRY(ds_q_sample_rng(x0, t, gids, seed, call, h->d.sched, xt_scratch, B, c.L, c.K, c.T, stream));
    TRY(forward_impl(h, xt_scratch, t, kv, B, w, w.logits, 0, (hipStream_t)stream, Lp));
    return ds_score_tail_launch(c);
}
