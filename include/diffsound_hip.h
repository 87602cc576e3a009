/* C ABI of libdiffsound_hip.so -- the MI355X (gfx950) kernels of the Diffsound generation path.
 *
 * The reference (yangdongchao/Text-to-sound-Synthesis) has no FFI / plugin boundary: its hot path
 * is stock torch ops called from Python nn.Modules.  This header therefore
 * defines the boundary a maintainer would bind instead of those op chains; each entry cites the
 * reference lines it replaces (paths relative to Diffsound/).  INTEGRATION.md shows the ctypes
 * binding and the module-level drop-ins.
 *
 * Conventions: every pointer is a DEVICE pointer to fp32 / int64 data unless stated otherwise;
 * callers own all memory (outputs and workspaces included); calls are asynchronous on `stream`
 * (a hipStream_t, passed as void*); the return value is 0 on success, -1 for a rejected argument,
 * -2 for a failed launch, and ds_last_error_string() describes the last failure of the calling
 * thread.  No function allocates, frees or synchronises.  Activations are channels-last.
 * Compute entries keep no state between calls (a ds_denoiser handle only holds the caller's weight pointers).  The
 * exceptions are the TEST / MEASUREMENT switches -- ds_gemm*_force_tile, ds_gemm_f16x2_set_balance_slots, ds_profile_* --
 * which are process-global and must not be flipped while another thread or stream of the process is launching.
 */
#ifndef DIFFSOUND_HIP_H
#define DIFFSOUND_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* ds_stream_t; /* hipStream_t */

int ds_version(void);
const char* ds_last_error_string(void);

/* ---- gather-GEMM (fp32 MFMA): C = store(act(A(m,k) * W[n][k] + bias) + R) ----------------------
 * replaces nn.Linear (sound_synthesis/modeling/transformers/transformer_utils.py:31-36,75-82,
 * 248-253,345-348), Conv2d 1x1/3x3 (specvqgan/modules/diffusionmodules/model.py:92-226,570-671) and
 * Conv1d / ConvTranspose1d (vocoder/modules.py:72-127). */
enum { DS_LOAD_DENSE = 0, DS_LOAD_CONV2D = 1, DS_LOAD_CONV1D = 2, DS_LOAD_CONVT1D = 3 };
enum { DS_PRO_NONE = 0, DS_PRO_AFFINE = 1, DS_PRO_AFFINE_SWISH = 2, DS_PRO_LRELU = 3 };
enum { DS_ACT_NONE = 0, DS_ACT_GELU2 = 1, DS_ACT_TANH = 2 };
enum { DS_STORE_ROW = 0, DS_STORE_BATCH_T = 1, DS_STORE_CONVT = 2, DS_STORE_ATTN = 3 };

typedef struct ds_gemm_desc {
    const float* A;        /* activation base */
    const float* W;        /* [groups][N][ldw], K contiguous */
    const float* bias;     /* [N] or NULL */
    const float* R;        /* residual [M][ldr] (row-major store only) or NULL; may alias C */
    float* C;
    int32_t M, N, K;       /* per group; K % 32 == 0 */
    int32_t lda, ldw, ldc, ldr;
    int32_t groups;        /* >= 1; A/W/C advance by the strides below per group */
    int64_t a_gstride, w_gstride, c_gstride;
    int32_t loader, pro, act, store;
    const float* pro_scale; /* [samples][Cin] for DS_PRO_AFFINE* (GroupNorm folded to a*s + o) */
    const float* pro_shift;
    int32_t rows_per_sample; /* dense prologue / DS_STORE_BATCH_T: rows of one sample; ds_gemm_f16x2 with packed operands: lets
                                the dispatcher take the per-sample programs (see ds_gemm_f16x2_force_tile), 0 = never */
    int32_t Cin;             /* channels per tap (conv loaders; dense prologue: = K) */
    int32_t H, Wd;           /* conv2d: output H, W; conv1d / convT1d: Wd = output length / phase rows */
    int32_t up;              /* conv2d: 1 = source is (H/2, W/2), nearest-upsampled on the fly; 2 = stride-2 conv over a
                                (2H, 2W) source zero-padded right/bottom only (Downsample, model.py:60-77) */
    int32_t taps, dil;       /* conv1d (reflect padding) */
    int32_t ct_r, ct_p, ct_tin; /* convT1d polyphase: stride, padding, input length; groups = r */
    int32_t f16_round;       /* 1: round outputs (and GELU2 intermediates) to the fp16 grid (CLIP text tower) */
    int64_t w3_plane;        /* split kernels only: W holds 3 bf16 / 2 fp16 planes [N][ldw], w3_plane elements apart */
    float out_scale;         /* ds_gemm_f16x2 only: 2^-s undoing the exact power-of-two pre-scale of W */
    /* ds_gemm_f16x2 only -- "packed split planes" of X[R][K] (K % 32 == 0): two fp16 planes (hi, lo), each
       [ceil(R/16)][K/32][16 rows][4 chunks][8 halves] with 16-byte chunk c of row r stored at chunk c ^ ((r>>2)&3);
       element (r,k) at ((r/16)*(K/32) + k/32)*512 + (r%16)*32 + (((k/8)%4) ^ ((r/4)%4))*8 + k%8.
       a_split: A AND W are given in that layout (lda = ldw = K; planes a_plane / w3_plane halves apart), staged by
       LDS-DMA.  c_split: C is written in that layout with row length ldc (planes c_plane halves apart). */
    int32_t a_split, c_split;
    int64_t a_plane, c_plane;
    /* ds_gemm_f16x2, store = DS_STORE_ATTN (packed operands only): column n = which*heads*64 + head*64 + d (which 0 Q,
       1 K, 2 V; N = 1..3 times heads*64), row = sample*rows_per_sample + position (rows_per_sample >= 128).
       C = the Q planes (attn_qplane halves apart), attn_kv = the K / V^T images with attn_nkey key slots
       (see ds_attention_f16x2_ready). */
    void* attn_kv;
    int32_t attn_heads, attn_nkey;
    int64_t attn_qplane;
} ds_gemm_desc;

int ds_gemm(const ds_gemm_desc* d, ds_stream_t stream);
void ds_gemm_force_tile(int cfg); /* test hook: 0..2 pins the block tile, -1 = auto */
/* The same dense contraction (DS_LOAD_DENSE, DS_PRO_NONE) on the fp16 matrix cores with fp32-class accuracy:
 * W*2^s and A are split into two fp16 planes each (22 significant bits), three fp16 MFMA passes
 * a0b0 + a0b1 + a1b0 per k-step, epilogue multiplies by out_scale = 2^-s.  |A| must stay below 65504
 * (gemm_f16x2.hip).  groups > 1 (plain row store, no bias / residual): group g computes
 * A + g a_gstride (floats; HALVES for packed operands) times W + g w_gstride (halves, both planes) into C + g c_gstride
 * -- with a_gstride = w_gstride = K (row-major operands) resp. 16 K (packed operands: K / 32 k-tiles of 512 halves, and
 * lda = ldw = the FULL contraction length the planes were packed with) this is a split-K launch whose partial results the
 * caller sums (ds_colsum). */
int ds_gemm_f16x2(const ds_gemm_desc* d, ds_stream_t stream);
/* n <= 4 INDEPENDENT packed-operand products (a_split = 1, row store, no bias / residual / activation, the same `groups` each)
 * as ONE grid of tile configuration cfg (0: 128x128, 1: 128x64, 3: 96x128): the weight gradients dW = dY^T X of several
 * nn.Linear layers of a block (transformer_utils.py:31-36,75-82,248-253 under loss.backward()), each sized to one workgroup per
 * CU, side by side instead of back to back.  Every product gets the bits ds_gemm_f16x2 gives it with that tile forced. */
int ds_gemm_f16x2_multi(const ds_gemm_desc* descs, int n, int cfg, ds_stream_t stream);
/* the conv-family loaders in the same fp32-class 3-pass formulation: A fp32 (split while it is staged), W = the two fp16
   planes [groups][N][ldw] of W * 2^s from split_f16x2 (w3_plane halves apart, groups w_gstride apart), out_scale = 2^-s.
   d->loader: DS_LOAD_CONV2D (3x3 conv over a channels-last image: Cin, H, Wd, up; prologue none or GroupNorm affine +
   swish), DS_LOAD_CONV1D (taps, dil, reflect padding; prologue none / LeakyReLU), DS_LOAD_CONVT1D (groups = ct_r
   phases, DS_STORE_CONVT; vocoder/modules.py:104-111), DS_LOAD_DENSE (1x1 convs).  Bias, residual, row store; Cin % 32
   == 0, N % 4 == 0.  (A descriptor with loader 0 and the conv2d geometry H > 0, K == 9 Cin is taken as DS_LOAD_CONV2D.) */
int ds_conv2d_f16x2(const ds_gemm_desc* d, ds_stream_t stream);
/* cfg: -1 automatic (default): the per-sample ping-pong program (gemm_f16x2_ps.hip: one 288 x 256 tile of an 8-wave
   workgroup per (sample, 256 columns)) when the problem has packed operands, rows_per_sample in (240, 273] with
   M % rows_per_sample == 0, N % 256 == 0, K % 64 == 0, a row / packed / attention store and a grid that fills whole
   rounds of the 256 CUs (the denoiser's GEMMs at batch 64) -- or, for a row-major store, its LEADING samples that do, the
   rest following as a second launch (20 samples x 4096 columns: 16 + 4); else 128x128 (balanced launch for packed
   operands) / 128x64 / 64x64 / 96x128 (packed operands only: four waves side by side) tiles of a 4-wave workgroup by grid
   size (the rule for packed operands: gemm_f16x2.hip).  0 / 1 / 2 / 3 pin those four; 9 pins the per-sample program, 10 its
   half-tile form, for every problem they can compute, whatever the grid (tests).  Every cfg produces the same bits.
   PROCESS-GLOBAL test / measurement switch, like every *_force_tile, *_set_balance_slots and ds_profile_* entry:
   not for use while another thread or stream of the process is launching GEMMs. */
void ds_gemm_f16x2_force_tile(int cfg);
/* the tile configuration (0 .. 3 as above) an M x N packed-operand product in `groups` K-ranges takes when nothing is forced
   (pure arithmetic; the training step groups its weight gradients by it for ds_gemm_f16x2_multi) */
int ds_gemm_f16x2_auto_tile(int M, int N, int groups);
/* packed-operand launches that pick the 128x128 tile are balanced: 128x128 tiles over the leading rows that fill
   whole rounds of `slots` resident workgroups (default 512 = 256 CUs x 2), 64x64 tiles over the rest.  Test hook
   (process-global). */
void ds_gemm_f16x2_set_balance_slots(int slots);
/* The row partition a packed-operand launch of cfg 0 uses for an M x N product with the given store mode: rows
   [0, m_off) -> nbig main tiles, rows [m_off, M) -> nsmall tail tiles (0: one program over all rows).
   Pure arithmetic, no device work: the CPU test-suite checks the partition with it. */
int ds_gemm_f16x2_plan(int cfg, int M, int N, int store, int* m_off, int* nbig, int* nsmall);

/* ---- row kernels of the denoiser -------------------------------------------------------------- */
/* DalleMaskImageEmbedding.forward, sound_synthesis/modeling/embeddings/dalle_mask_image_embedding.py:36-58
 * out[m] = emb[tokens[m]] + pos[m % L]   (pos = height_emb[p // W] + width_emb[p % W], precombined) */
int ds_embed(const int64_t* tokens, const float* emb, const float* pos, float* out, int M, int L, int D,
             ds_stream_t stream);
/* AdaLayerNorm.forward, transformer_utils.py:145-149, with Linear(SiLU(Emb[t])) tabulated: table [T][2D] */
int ds_adaln(const float* x, float* y, int M, int L, int D, const float* table, const int64_t* t,
             ds_stream_t stream);
/* nn.LayerNorm(D) eps 1e-5 with affine, transformer_utils.py:205,346 */
int ds_layernorm(const float* x, float* y, int M, int D, const float* gamma, const float* beta,
                 ds_stream_t stream);
/* FullAttention / CrossAttention core, transformer_utils.py:43-58, 91-109 (head dim 64, Lk <= 288) */
int ds_attention(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo,
                 int B, int heads, int Lq, int Lk, float scale, ds_stream_t stream);

/* causal = 1: key j visible to query i iff j <= i; f16_round = 1: scores, probabilities and outputs are
 * rounded to the fp16 grid (CLIP's nn.MultiheadAttention in fp16, clip/model.py:166-186) */
int ds_attention_ex(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo,
                    int B, int heads, int Lq, int Lk, float scale, int causal, int f16_round, ds_stream_t stream);
/* the same attention (no mask, head dim 64) on the fp16 matrix cores with the f16x2 split: fp32-class results,
 * ~5x fewer MFMA cycles (attention_f16x2.hip); used by the denoiser in f16x2 mode */
int ds_attention_f16x2(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo,
                       int B, int heads, int Lq, int Lk, float scale, ds_stream_t stream);
/* producers that write packed split planes for ds_gemm_f16x2 (a_split): yh / oh = 2 planes of ceil16(rows) * (D or
   ldo) halves, layout as described at ds_gemm_desc.a_split */
int ds_adaln_split(const float* x, void* yh, int M, int L, int D, const float* table, const int64_t* t,
                   ds_stream_t stream);
int ds_layernorm_split(const float* x, void* yh, int M, int D, const float* gamma, const float* beta,
                       ds_stream_t stream);
int ds_attention_f16x2_split(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, void* oh,
                             int ldo, int B, int heads, int Lq, int Lk, float scale, ds_stream_t stream);
/* Attention on "attention-ready" operands, the denoiser's default path: Q as two fp16 planes [B][heads][Lq][64]
 * (q_plane halves apart), K and V^T as per-(sample, head) LDS images  K hi | K lo | V^T hi | V^T lo  of nkey*64 halves
 * each (nkey = ds_attn_nkey(Lk); K[key][64] with 16-byte chunk c at c ^ ((key>>1)&7), V^T[d][nkey] with the 16-byte
 * chunk of keys 8c..8c+7 at c ^ ((d>>2)&3): csrc/common.h ds_attn_k_off / ds_attn_vt_off; rows of keys >= Lk zero).
 * Producers: ds_gemm_f16x2 with store = DS_STORE_ATTN (Q | K | V columns of the fused QKV projection, or Q alone),
 * ds_attn_pack_kv (fp32 K | V rows, e.g. the caption K/V).  Output: packed split planes as ds_attention_f16x2_split. */
int ds_attn_nkey(int Lk);
int ds_attention_f16x2_ready(const void* qh, long long q_plane, const void* kv_img, void* oh, int ldo, int B, int heads,
                             int Lq, int Lk, float scale, ds_stream_t stream);
int ds_attn_pack_kv(const float* kv, int ld, int v_col, void* img, int B, int heads, int Lk, ds_stream_t stream);
/* fp16-semantics row kernels of the CLIP text tower (sound_synthesis/modeling/modules/clip/model.py:150-157,
 * 341-354; embeddings/clip_text_embedding.py:46-88): fp32 storage, outputs rounded to the fp16 grid */
int ds_embed_f16(const int64_t* tokens, const float* emb, const float* pos, float* out, int M, int L, int D,
                 ds_stream_t stream);
int ds_layernorm_f16(const float* x, float* y, int M, int D, const float* gamma, const float* beta,
                     ds_stream_t stream);
int ds_l2norm_rows_f16(const float* x, float* y, int M, int D, ds_stream_t stream);

/* ---- one reverse-diffusion step's per-column tail --------------------------------------------
 * predict_start (diffusion_transformer.py:285-289) + top-r truncation (models/dalle_spec.py:158-174)
 * + q_posterior (:293-339) + log_sample_categorical (:359-368).
 * logits [B*L][K]; xt [B][L]; t [B]; u [B][K+1][L] uniforms; sched [8][T+1];
 * dbg_* optional [B][K+1][L] dumps (NULL to skip); trunc_r < 0 disables truncation. */
int ds_sample_tail(const float* logits, const int64_t* xt, const int64_t* t, const float* u, const float* sched,
                   int64_t* out_tokens, float* dbg_log_pred, float* dbg_trunc, float* dbg_post, int B, int L,
                   int K, int T, int initial, float trunc_r, ds_stream_t stream);

/* + top-k truncation ('top{k}p', dalle_spec.py:147-157): trunc_k > 0 keeps the k largest log-probs of a column
 * (exclusive with trunc_r >= 0) */
int ds_sample_tail_ex(const float* logits, const int64_t* xt, const int64_t* t, const float* u, const float* sched,
                      int64_t* out_tokens, float* dbg_log_pred, float* dbg_trunc, float* dbg_post, int B, int L,
                      int K, int T, int initial, float trunc_r, int trunc_k, ds_stream_t stream);

/* q_sample (diffusion_transformer.py:370-377): x_t ~ q(x_t | x_0) on token ids, u [B][K+1][L] uniforms; used by
 * sample()'s filter_ratio > 0 branch (:643-651) */
int ds_q_sample(const int64_t* x0, const int64_t* t, const float* u, const float* sched, int64_t* out_tokens, int B,
                int L, int K, int T, ds_stream_t stream);

/* ---- the same samplers with the noise drawn INSIDE the kernel -----------------------------------------------------
 * The reference draws torch.rand_like(logits) per step (log_sample_categorical, diffusion_transformer.py:359-368), so
 * what a caption draws depends on the batch it is in.  SURVEY.md section 8(e) asks for per-sample noise keyed by the
 * global caption index so that a shard reproduces the single-GPU draw (pattern: Codebook/evaluation/
 * generate_samples_caps.py:153,306 -- rank-sharded sampler, nothing collective in the loop).  These entries draw from a
 * counter-based Philox4x32-10 stream: the uniform of class c = 64 j + lane (the [MASK] class K is j = K / 64, lane 0)
 * at grid position pos of caption gids[b] in sampler call `call` is word (j & 3) of
 *     Philox(counter = (64 (j >> 2) + lane, pos | rng_stream << 16, call, gids[b]), key = (seed lo, seed hi))
 * mapped to [0, 1) as (word >> 8) * 2^-24; rng_stream = 0 for reverse steps, 1 for q_sample.  gids [B] (device, each
 * < 2^32), L < 65536.  ds_philox_uniforms writes that stream out as u [B][K+1][L] (tests: *_rng(...) == the u-path fed
 * with it).  Host mirror (numpy): text_to_sound_synthesis_amd.shard.caption_uniforms. */
int ds_philox_uniforms(const int64_t* gids, unsigned long long seed, int call, int rng_stream, float* u, int B, int L,
                       int K, ds_stream_t stream);
int ds_sample_tail_rng(const float* logits, const int64_t* xt, const int64_t* t, const int64_t* gids,
                       unsigned long long seed, int call, const float* sched, int64_t* out_tokens, int B, int L, int K,
                       int T, int initial, float trunc_r, int trunc_k, ds_stream_t stream);
int ds_q_sample_rng(const int64_t* x0, const int64_t* t, const int64_t* gids, unsigned long long seed, int call,
                    const float* sched, int64_t* out_tokens, int B, int L, int K, int T, ds_stream_t stream);

/* ---- region-held tails (inpainting / continuation) -----------------------------------------------------------------
 * ds_sample_tail_ex / ds_sample_tail_rng with keep u8[B][L] (non-zero: the position is held), known i64[B][L] (the token a
 * held position carries) and mode.  Positions in content_token's time-major order (5 column + row).
 *   mode 0 (clamp):   a held column writes known; a free column computes what the unheld entry computes from the same
 *                     logits and the same uniforms (the noise is not re-indexed), so keep all zero == the unheld entry.
 *   mode 1 (renoise): t is the posterior's timestep and the output x_{t-1}: a held column draws q(x_{t-1} | x_0 = known)
 *                     (ds_q_sample's arithmetic, rng_stream 1, the call's own (pos, call, gid) counters), or writes known
 *                     at t = 0.  In-kernel noise only: rejected by the entry on caller uniforms.
 * keep == NULL runs the unheld kernel; keep without known is rejected.  Pass initial = 0 with keep: `initial` only affects
 * non-[MASK] positions, and those of a mixed start state carry the ordinary log-one-hot. */
int ds_sample_tail_hold(const float* logits, const int64_t* xt, const int64_t* t, const float* u, const float* sched,
                        int64_t* out_tokens, float* dbg_log_pred, float* dbg_trunc, float* dbg_post, int B, int L, int K,
                        int T, int initial, float trunc_r, int trunc_k, const unsigned char* keep, const int64_t* known,
                        int mode, ds_stream_t stream);
int ds_sample_tail_hold_rng(const float* logits, const int64_t* xt, const int64_t* t, const int64_t* gids,
                            unsigned long long seed, int call, const float* sched, int64_t* out_tokens, int B, int L,
                            int K, int T, int initial, float trunc_r, int trunc_k, const unsigned char* keep,
                            const int64_t* known, int mode, ds_stream_t stream);

/* Classifier-free guidance in the tail.  Two logit rows per grid position: logits_c from the denoiser run with the caption,
 * logits_u from the run with the null condition (both [B*L][K], same x_t and t).  With lc / lu = predict_start of each row
 * (float64 log-softmax, rounded to f32, clamped to [-70, 0]):
 *     g = lu + scale (lc - lu),   g <- g - logsumexp(g)      in float64, max-shifted,
 * rounded to f32 and clamped to [-70, 0] ([MASK] row -70) is the log_pred that truncation, posterior and Gumbel-argmax
 * consume unchanged; dbg_log_pred dumps it.  scale 0: the null prediction, 1: the captioned one.  keep / known / mode as in
 * ds_sample_tail_hold (a held column leaves before any of this); keep == NULL: unheld.  Rejected (-1, nothing launched):
 * a null logits_u, a non-finite scale, and what ds_sample_tail_hold rejects. */
int ds_sample_tail_guided(const float* logits_c, const float* logits_u, const int64_t* xt, const int64_t* t, const float* u,
                          const float* sched, int64_t* out_tokens, float* dbg_log_pred, float* dbg_trunc, float* dbg_post,
                          int B, int L, int K, int T, int initial, float trunc_r, int trunc_k, float scale,
                          const unsigned char* keep, const int64_t* known, int mode, ds_stream_t stream);
int ds_sample_tail_guided_rng(const float* logits_c, const float* logits_u, const int64_t* xt, const int64_t* t,
                              const int64_t* gids, unsigned long long seed, int call, const float* sched,
                              int64_t* out_tokens, int B, int L, int K, int T, int initial, float trunc_r, int trunc_k,
                              float scale, const unsigned char* keep, const int64_t* known, int mode, ds_stream_t stream);

/* Joint-window sampling in the tail: the W windows of a long clip live on one token CANVAS and a position that two windows
 * cover is drawn once, from the fusion of their predictions (the discrete counterpart of MultiDiffusion, Bar-Tal et al. 2023).
 * Geometry: R = 5 grid rows, G = 53 grid columns, n = overlap_cols in 1 .. 26, hop h = G - n; the canvas has C columns --
 * line (ring == 0): C = G + (W - 1) h, W >= 1; ring: C = W h, W >= 2, window w covering columns (w h + o) mod C -- and
 * Lc = R C positions q = R c + r, time-major.  For column c the later window is w1 = min(c / h, W - 1) (ring: c / h) at offset
 * o1 = c - w1 h; if o1 < n and (w1 >= 1 or ring) the earlier window w0 = (w1 - 1) mod W covers it too, at offset o1 + h.
 *   logits / logits_u  f32[B W lrows][K], row (b W + w) lrows + R o + r for offset o of window w; lrows >= R G;
 *                      logits_u NULL: unguided, else the null condition's rows and `scale` as in ds_sample_tail_guided
 *   canvas / out_canvas / keep / known  [B][Lc];  t i64[B];  u f32[B][K+1][Lc], or gids i64[B] (Philox position q)
 *   fade               f32[n] on the device: the later window's weight at overlap offset o1, in (0, 1)
 * One wave per canvas position.  Under one window it is the plain (or guided) tail on that window's row.  Under two, l0 / l1 =
 * the log_pred the plain (or guided) tail gives rows w0 / w1 (rounded to f32, clamped), and in float64
 *     g = l0 + fade[o1] (l1 - l0),   g <- g - logsumexp(g)   (max-shifted),
 * the guided expression with (lu, lc, scale) = (l0, l1, fade[o1]), rounded to f32 and clamped to [-70, 0], is the log_pred that
 * truncation, posterior and Gumbel-argmax consume unchanged; the dbg_* dumps are f32[B][K+1][Lc].  keep / known: clamp mode
 * only (mode 0), keep == NULL: unheld.  Rejected (-1, nothing launched): null pointers (fade included), W < 1, n outside
 * 1 .. 26, a ring with W < 2, Lc >= 65536, lrows < R G, mode != 0, keep without known, both truncations, a non-finite scale
 * with logits_u. */
int ds_sample_tail_joint(const float* logits, const float* logits_u, const int64_t* canvas, const int64_t* t, const float* u,
                         const float* sched, int64_t* out_canvas, float* dbg_log_pred, float* dbg_trunc, float* dbg_post,
                         int B, int W, int overlap_cols, int ring, const float* fade, int lrows, int K, int T, int initial,
                         float trunc_r, int trunc_k, float scale, const unsigned char* keep, const int64_t* known, int mode,
                         ds_stream_t stream);
int ds_sample_tail_joint_rng(const float* logits, const float* logits_u, const int64_t* canvas, const int64_t* t,
                             const int64_t* gids, unsigned long long seed, int call, const float* sched, int64_t* out_canvas,
                             float* dbg_log_pred, float* dbg_trunc, float* dbg_post, int B, int W, int overlap_cols, int ring,
                             const float* fade, int lrows, int K, int T, int initial, float trunc_r, int trunc_k, float scale,
                             const unsigned char* keep, const int64_t* known, int mode, ds_stream_t stream);
/* The window rows of a canvas, as the denoiser reads them: win[(k B W + b W + w)][R o + r] = canvas[b][R ((w h + o) mod C) + r]
 * for k < copies (1 or 2), condition-major.  canvas i64[B][Lc], win i64[copies B W][265].  The geometry rules above. */
int ds_joint_gather(const int64_t* canvas, int64_t* win, int B, int W, int overlap_cols, int ring, int copies,
                    ds_stream_t stream);

/* Caption tracks in the tail: several captions per clip, each weighted per grid position (the conjunction of Liu et al.,
 * "Compositional Visual Generation with Composable Diffusion Models", 2022, with weights that vary over the token grid;
 * guidance is its one-track, constant-weight case).  C = n_tracks, 1 <= C <= DS_MAX_TRACKS.
 *   logits   f32[C + 1][B*L][K]: the denoiser's logits under track 0 .. C-1's captions, the null condition's LAST; all on
 *            the same x_t and t
 *   weights  f32[B][C][L]
 * With lu / l_i = predict_start of the null row and of track i's row (as in ds_sample_tail_guided), in float64:
 *     g = lu;   for i = 0 .. C-1 in this order:  g = g + weights[b][i][pos] (l_i - lu);   g <- g - logsumexp(g)  (max-shifted),
 * rounded to f32 and clamped to [-70, 0] ([MASK] row -70) is the log_pred that truncation, posterior and Gumbel-argmax
 * consume unchanged; dbg_log_pred dumps it.  One track of constant weight s gives ds_sample_tail_guided's results at scale
 * s bit for bit.  A track whose weight at a position is exactly 0 is not read at that position (its logits may hold
 * anything there); all weights 0: the null prediction.  Negative weights push away from a caption.  The noise is the plain
 * tail's: one stream per clip (gids[b], call).  keep / known / mode as in ds_sample_tail_guided; keep == NULL: unheld.
 * Rejected (-1, nothing launched): null weights, n_tracks outside 1 .. DS_MAX_TRACKS, and what ds_sample_tail_guided
 * rejects.  The VALUES of weights are on the device and are not checked (that would take a synchronisation): the caller
 * passes finite weights -- the Python layer checks them -- and a non-finite weight gives a non-finite prediction. */
#define DS_MAX_TRACKS 4
int ds_sample_tail_composed(const float* logits, const int64_t* xt, const int64_t* t, const float* u, const float* sched,
                            int64_t* out_tokens, float* dbg_log_pred, float* dbg_trunc, float* dbg_post, int B, int L,
                            int K, int T, int initial, float trunc_r, int trunc_k, int n_tracks, const float* weights,
                            const unsigned char* keep, const int64_t* known, int mode, ds_stream_t stream);
int ds_sample_tail_composed_rng(const float* logits, const int64_t* xt, const int64_t* t, const int64_t* gids,
                                unsigned long long seed, int call, const float* sched, int64_t* out_tokens, int B, int L,
                                int K, int T, int initial, float trunc_r, int trunc_k, int n_tracks, const float* weights,
                                const unsigned char* keep, const int64_t* known, int mode, ds_stream_t stream);

/* Purity-prior sampling in the tail (the high-quality inference strategy of Tang et al., "Improved Vector Quantized
 * Diffusion Models", 2022; specification: DESIGN.md section 4).  One step reveals an exact number of [MASK] positions per
 * sample, the most confident first, and never re-samples a revealed token; it uses no posterior and no schedule table.
 * Per grid position (one wavefront, ds_sample_purity_rows_kernel):
 *     lp    predict_start of the row; with logits_u != NULL the guided mix of ds_sample_tail_guided (scale) comes next
 *     tr    the truncation of lp (trunc_r / trunc_k as in ds_sample_tail_ex; dropped classes at -70)
 *     lmax  max_c lp[c], before truncation: the log of the purity
 *     sh    weight == 0: tr, bit for bit; weight > 0: with a = 1 + weight expf(lmax),
 *           a tr - logsumexp(a tr) in float64, max-shifted, rounded to f32, clamped to [-70, 0]
 *     cand  argmax over the K real classes of sh[c] + G(u_c), G(u) = -logf(-logf(u + 1e-30f) + 1e-30f), first index wins
 *     key   lmax + G(u_K) where xt == K ([MASK]), -INFINITY elsewhere; u_K is the [MASK] slot's uniform
 * and per sample (one workgroup, ds_sample_purity_select_kernel): with m [MASK] positions and n = max(0, m - remain), the
 * n masked positions of largest key (equal keys: the smaller position first) get out = cand, every other position keeps xt.
 * The uniforms are the plain tail's: u [B][K+1][L], or the Philox words of (gids, seed, call) (ds_sample_tail_rng).
 *   lrows    rows of logits (and logits_u) per sample, >= L: [B * lrows][K] (the denoiser's padded-row mode)
 *   scratch  ds_purity_scratch_bytes(B, L) bytes of device memory: cand i32[B][L], then key f32[B][L]
 *   dbg_*    optional: dbg_sharp f32[B][K+1][L] (sh, [MASK] row -70), dbg_key f32[B][L], dbg_cand i32[B][L]
 * Rejected (-1, nothing launched): null pointers, K other than 256 / 512, remain < 0, a negative or non-finite weight, a
 * non-finite scale with logits_u, both truncations, lrows < L, L > 288. */
int64_t ds_purity_scratch_bytes(int B, int L);
int ds_sample_tail_purity(const float* logits, const float* logits_u, float scale, const int64_t* xt, const float* u,
                          int remain, float weight, float trunc_r, int trunc_k, int lrows, void* scratch,
                          int64_t* out_tokens, float* dbg_sharp, float* dbg_key, int32_t* dbg_cand, int B, int L, int K,
                          ds_stream_t stream);
int ds_sample_tail_purity_rng(const float* logits, const float* logits_u, float scale, const int64_t* xt,
                              const int64_t* gids, unsigned long long seed, int call, int remain, float weight,
                              float trunc_r, int trunc_k, int lrows, void* scratch, int64_t* out_tokens, float* dbg_sharp,
                              float* dbg_key, int32_t* dbg_cand, int B, int L, int K, ds_stream_t stream);

/* forward terms of the training loss (DiffusionTransformer._train_loss, diffusion_transformer.py:408-476), one value
 * per grid position [B][L]: kl = KL(true posterior || model posterior) (:439-440), nll = the t == 0 decoder term
 * (:446), kl_aux = KL(x_0 || p(x_0|x_t)) over the K classes (:462); logits [B*L][K] of the network at (x_t, t),
 * dbg_model_log_prob optional [B][K+1][L].  Forward value only; its gradient is ds_loss_tail_bwd below. */
int ds_loss_tail(const float* logits, const int64_t* x0, const int64_t* xt, const int64_t* t, const float* sched,
                 float* kl, float* nll, float* kl_aux, float* dbg_model_log_prob, int B, int L, int K, int T,
                 ds_stream_t stream);

/* Likelihood scoring: one term of a clip's variational bound per row (definition: DESIGN.md section 4).  Row b is a
 * (clip, timestep) pair -- x0 i64[B][L] the clip's tokens (each < K), xt i64[B][L] its diffused state, t i64[B] (each in
 * [0, T): rows at different timesteps share a launch; a row outside that range gets NaN), logits [B * lrows][K] the
 * network's output on (xt, t) with lrows >= L rows per sample (the denoiser's padded-row mode; rows >= L are never read).
 * Per grid position, exactly what ds_loss_tail writes there, bit for bit -- nll where t[b] == 0, kl where t[b] > 0 -- and
 * only that term is computed (no true posterior at t == 0, never the auxiliary KL).  term f64[B]: the row's positions
 * widened to double and summed in a fixed order, no atomics, so a row's result depends neither on B nor on its row index.
 * dbg_pos optional f32[B][L]: the per-position values.  Mask weights are (1, 1): this is the bound, not the training loss.
 * Rejected (-1, nothing launched): null pointers (except dbg_pos), K other than 256 / 512, lrows < L, L > 288, B < 1. */
int ds_score_tail(const float* logits, const int64_t* x0, const int64_t* xt, const int64_t* t, const float* sched,
                  double* term, float* dbg_pos, int lrows, int B, int L, int K, int T, ds_stream_t stream);

/* d(sum over samples of vb_loss) / d logits for the loss above (pt [B] = the sampling probabilities of t; mask
 * weights for masked / unmasked x_t positions; auxiliary loss weight and its adaptive flag): dlogits [B*L][K].  The
 * first kernel of the training step's backward (modeling/train.py composes the rest from the entries below, the GEMMs
 * and ds_attention_bwd). */
int ds_loss_tail_bwd(const float* logits, const int64_t* x0, const int64_t* xt, const int64_t* t, const float* pt,
                     const float* sched, float* dlogits, int B, int L, int K, int T, float mask_weight_masked,
                     float mask_weight_other, float aux_weight, int adaptive, ds_stream_t stream);

/* ---- row / elementwise kernels of the training step (csrc/train.hip; scope row 8f-3, building blocks) --------
 * AdaLN (mode 0: table [T][2D], t [M/L]) / LayerNorm (mode 1: gamma) backward: dx, and dyxn = dy * xn for the scale
 * gradient (NULL to skip); D = 1024 */
int ds_layernorm_bwd(const float* x, const float* dy, float* dx, float* dyxn, int M, int L, int D, int mode,
                     const float* table, const int64_t* t, const float* gamma, ds_stream_t stream);
/* The backward with the scale / shift gradient sums folded in: part[G * chunks][2][D] receives, per chunk of <= 16 rows of a
 * group (G = M / L samples for mode 0, one group for mode 1; chunks = ds_layernorm_bwd_chunks(M, L, mode)), the column sums of
 * dy * xn and of dy; ds_colsum over a group's chunks (R = chunks, C = 2 D) gives [d scale | d shift].  No [M][D] dyxn matrix. */
int ds_layernorm_bwd_chunks(int M, int L, int mode);
int ds_layernorm_bwd_sums(const float* x, const float* dy, float* dx, float* part, int M, int L, int D, int mode,
                          const float* table, const int64_t* t, const float* gamma, int accumulate, ds_stream_t stream);
/* out[g][c] (+)= sum over R rows of x[(g*gstride) + r*ld + c]: bias / scale / per-sample AdaLN gradients */
int ds_colsum(const float* x, float* out, int G, int R, int C, long long ld, long long gstride, int accumulate,
              ds_stream_t stream);
/* the same sums for tall inputs (R in the thousands): rows are summed in up to 64 chunks by separate workgroups into
 * `work` (>= G * 64 * C floats is always enough), then the chunks are added in a fixed order -- deterministic */
int ds_colsum_ws(const float* x, float* out, int G, int R, int C, long long ld, long long gstride, int accumulate,
                 float* work, long long work_floats, ds_stream_t stream);
/* GELU2: dy == NULL -> out = x * sigmoid(1.702 x); else out = dy * d/dx of that */
int ds_gelu2(const float* x, const float* dy, float* out, long long n, ds_stream_t stream);
/* in place dS = scale * P * (dP - rowsum(dP * P)) over the first n columns of each row (attention backward) */
int ds_softmax_bwd_rows(const float* P, float* dP, int rows, int n, int ld, float scale, ds_stream_t stream);
/* Backward of ds_attention (FullAttention / CrossAttention cores, transformer_utils.py:43-58, :91-109) by tile-wise
 * recomputation -- the probabilities are never stored: given Q, K, V, the forward's O and dO it writes dQ, dK, dV.
 * Same addressing as ds_attention (rows b*L + pos, head h at columns h*64.., any row strides: column ranges of fused
 * projections work in place); exact-fp32 MFMA; Lq, Lk <= 288.  stats: 2 * B * heads * ceil32(Lq) floats of workspace
 * (per query: log-sum-exp of its scaled scores and delta = dO . O). */
int ds_attention_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o, int ldo,
                     const float* d_o, int lddo, float* dq, int lddq, float* dk, int lddk, float* dv, int lddv,
                     float* stats, int B, int heads, int Lq, int Lk, float scale, ds_stream_t stream);
/* The same backward with every tile product on the fp16 matrix cores (operands split into fp16 hi + lo on the fly, three
 * v_mfma_f32_32x32x16_f16 passes, fp32 accumulate: fp32-class, 5.3x less matrix-pipe time than the exact-fp32 MFMA); |dO|
 * must stay below 65504 (the training step's loss scale puts it at <= 2^13).  The "f16x2" training backend's choice. */
int ds_attention_bwd_f16x2(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o, int ldo,
                           const float* d_o, int lddo, float* dq, int lddq, float* dk, int lddk, float* dv, int lddv,
                           float* stats, int B, int heads, int Lq, int Lk, float scale, ds_stream_t stream);
/* ... with the training step's saturation monitor folded in (round 6): *amax -- a device float the caller zeroes when it
 * reads it; the kernels only ever raise it -- takes max |dO * do_scale|, the operand that carries the step's loss scale into
 * these kernels' fp16 splits (replaces the separate ds_amax over dO of rounds 3-5).  do_scale: a positive power of two, this
 * call's own scale on top of the loss scale: dO * do_scale is what is split, the dQ / dK / dV stores take it out again (exact).  dS = scale P (dP - delta), which exists only
 * in registers and has no fixed relation to dO (it can exceed it by |V| x 8, or sit 2^-20 under it where the probabilities
 * are near-uniform), is normalised per wave by an exact power of two before ITS split in all three entry points of the f16x2
 * form -- it can neither saturate nor fall into fp16's subnormal range.  Reference: the same loss.backward() lines as above. */
int ds_attention_bwd_f16x2_mon(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o, int ldo,
                               const float* d_o, int lddo, float* dq, int lddq, float* dk, int lddk, float* dv, int lddv,
                               float* stats, int B, int heads, int Lq, int Lk, float scale, float do_scale, float* amax,
                               ds_stream_t stream);
/* part[ks][g][b][d] = sum over k in [256 ks, 256 ks + 256) of x[g][b][k] * W[g][k][d]:  B <= 32 rows times G ROW-MAJOR matrices
 * [K][D] (K % 256 == 0), read once from where they lie -- the AdaLN backward's (d modulation) x linear.weight for all modules
 * (what autograd computes for AdaLayerNorm.linear's input, transformer_utils.py:145-147).  The caller adds the K / 256 partial
 * results in a fixed order (ds_colsum over part as [K / 256][G * B * D]). */
int ds_rows_times_matrix(const float* x, const float* W, float* part, int G, int B, int K, int D, ds_stream_t stream);
/* out[g][n][d] = sum over b < B of a[g][b][n] * s[g][b][d]  (a [G][B][N], s [G][B][D], out [G][N][D]; B <= 32, D % 4 == 0):
 * the AdaLN backward's d linear.weight = (d modulation)^T silu(emb(t_b)) for all modules in one output-bound pass (what
 * autograd computes for AdaLayerNorm.linear.weight, transformer_utils.py:145-147). */
int ds_rows_outer(const float* a, const float* s, float* out, int G, int B, int N, int D, ds_stream_t stream);
/* d emb[r] += sum over the m with tokens[m] == r of dx[m], in a fixed order (bit-reproducible; no atomics); tokens outside
 * [0, rows) are skipped.  D % 4 == 0, 16-byte aligned dx / demb.  One workgroup per row and 256 columns walks all positions. */
int ds_embed_bwd(const float* dx, const int64_t* tokens, float* demb, int M, int D, int rows, ds_stream_t stream);
/* The same sum with the positions split into chunks of 256 whose partial tables (work: ds_embed_bwd_work_floats(M, D, rows)
 * floats, 16-byte aligned) ds_colsum adds in chunk order: a long list (the [MASK] row at high t) spread over many workgroups.
 * The training step's entry. */
long long ds_embed_bwd_work_floats(int M, int D, int rows);
int ds_embed_bwd_ws(const float* dx, const int64_t* tokens, float* demb, int M, int D, int rows, float* work, long long work_floats,
                    ds_stream_t stream);
/* fused AdamW update (torch.optim.AdamW semantics), step >= 1.  The contract is FLOAT lr, beta, eps, weight_decay: the update is
 * torch's single-tensor expression on those float32 values -- m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, p = p (1 - lr wd) -
 * (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps), eps OUTSIDE the root, the NEW m and v -- with 1 - beta^step formed in double from
 * the float betas and rounded once (any step up to INT_MAX).  p, m and v stay within 4 x the distance of torch's own float32
 * path from float64 (+ 1 ulp) for |g| from 1e-12 to 1e6, over 400 steps, from p = 0 as from p ~ 1; g = 0 from the zero state
 * leaves m = v = 0 and only decays p (nothing divides by zero: the denominator is eps) (tests/test_hip_optimizer_range.py). */
int ds_adamw(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
             float weight_decay, int step, ds_stream_t stream);
/* The same update with the iteration's scalars in device memory, hyper = { lr, 1 - beta1^step, sqrt(1 - beta2^step),
 * grad_scale } (g is multiplied by grad_scale first: the clip coefficient / the inverse loss scale): a captured
 * hipGraph replays fixed kernel arguments, so what changes per iteration is read through this pointer.  The bias corrections
 * are taken as stored (the caller forms them, in double); the same bounds as ds_adamw for |g grad_scale| from 1e-12 to 1e6. */
int ds_adamw_dev(float* p, const float* g, float* m, float* v, long long n, const float* hyper, float beta1, float beta2,
                 float eps, float weight_decay, ds_stream_t stream);
/* *out = max(*out, max_i |x[i]|)  (the caller zeroes *out; calibration of the training step's loss scale).  Exact for every n >= 1
 * and any 4-byte aligned x: *out must hold a non-negative float; NaN entries are ignored (all NaN: *out is left as it is), +-inf
 * gives +inf, denormals count, -0.0 leaves +0. */
int ds_amax(const float* x, long long n, float* out, ds_stream_t stream);
/* ONE pass over fp32 X[rows][ld_src] (cols valid, cols % 32 == 0) that writes everything the three GEMMs of an nn.Linear
 * in the training step (y = x W^T, dX = dY W, dW = dY^T X: engine/solver_spec.py:308-331 over
 * diffusion_transformer.py:408-476) need of it -- any subset of:
 *   dst_row      packed split planes (hi | lo, plane_row halves apart) of scale * X as a [rows][cols] GEMM operand;
 *   dst_t        packed split planes (plane_t apart) of scale * X^T as a [cols][rows_pad] operand: the contraction index
 *                (X's rows) zero-padded to rows_pad (% 32 == 0; split-K launches need a multiple of 32 * groups); with
 *                t_cols > 0 the destination is [cols][t_cols] and this matrix fills its k-range [t_col0, t_col0 + rows_pad)
 *                (t_col0, t_cols % 32 == 0; 0, 0 = the matrix is the whole destination) -- row ranges of the ROW form are
 *                reached by offsetting dst_row by whole 16-row groups: the parts of a fused projection weight need no
 *                concatenated copy;
 *   colsum_part  [ds_pack_operand_tile_rows(rows, rows_pad)][cols] per-64-row column sums of X (after the prologue, BEFORE
 *                `scale`: a gradient's scale is its site's own power of two, which the bias gradient does not carry), the
 *                first ceil(rows / 64) rows of which ds_colsum adds up in a fixed order (bias gradients; no atomics);
 *   amax         *amax = max(*amax, max |scale * X|) (atomicMax on the bit pattern; the caller zeroes it);
 * with an elementwise prologue: DS_PACK_GELU2 (X := gelu2(X): GELU2 of transformer_utils.py:111-115 between the MLP's
 * linears) or DS_PACK_GELU2_BWD (X := X * gelu2'(aux), aux fp32 [rows][ld_aux]: its backward).  scale: a power of two. */
enum { DS_PACK_PLAIN = 0, DS_PACK_GELU2 = 1, DS_PACK_GELU2_BWD = 2 };
int ds_pack_operand(const float* src, int rows, int cols, long long ld_src, float scale, int pro, const float* aux,
                    long long ld_aux, void* dst_row, long long plane_row, void* dst_t, long long plane_t, int rows_pad,
                    int t_col0, int t_cols, float* colsum_part, float* amax, ds_stream_t stream);
int ds_pack_operand_tile_rows(int rows, int rows_pad);
/* torch.optim.AdamW (configs/caps.yaml:111-115) on many parameter tensors at once: `tensors` = HOST array of n_tensors
 * records { p, g, m, v (device pointers), n (int64 element count) } = 5 x 8 bytes each; 64 tensors per launch, their
 * descriptors passed by value in the kernel arguments (graph-capturable, no table in device memory); hyper and the
 * arithmetic as for ds_adamw_dev, with its bounds.  Any element count >= 1 and any 4-byte alignment of each of p, g, m, v (16-byte
 * accesses only where all four allow); a tensor's neighbours in memory are not touched. */
int ds_adamw_multi(const void* tensors, int n_tensors, const float* hyper, float beta1, float beta2, float eps,
                   float weight_decay, ds_stream_t stream);
/* engine/clip_grad_norm.py:8-29 -> torch.nn.utils.clip_grad_norm_: total = the L2 norm over ALL gradient tensors and coef =
 * min(1, max_norm / (total + 1e-6)) in device memory (ds_adamw_multi reads it as hyper[3]; nothing comes back to the host):
 * `tensors` = HOST array of n_tensors records { g (device pointer, fp32), n (int64 element count) }; part = workspace of at
 * least sum ceil(n_i / 4096) doubles; partial sums per 4096-element chunk, added in a fixed order in double (bit-reproducible).
 * Domain: a thread adds 16 squares in float32 before the doubles, so total is float32-class (within 4 x torch's float32
 * _foreach_norm path of float64, + 1 ulp) for 2^-63 <= |g| < 2^62, zeros aside.  Above, a thread's sum overflows and total = +inf,
 * never a finite wrong value; below, the squares are denormal and keep 2^-149 absolutely each: total stays finite, is never more
 * than 2^-20 relative above the true norm, is more and more understated and reaches 0 for |g| < 2^-75.
 * coef = 1 if max_norm <= 0, whatever the gradients hold.  Otherwise: one +-inf gradient -> total = +inf, coef = 0 (AdamW then sees
 * g coef = 0 everywhere but at the inf itself, which turns NaN); one NaN gradient -> total = NaN and coef = NaN, as torch's clamp
 * gives, so every parameter of that step turns NaN and the next loss shows it. */
int ds_grad_norm_multi(const void* tensors, int n_tensors, double* part, long long part_len, float max_norm, float* total,
                       float* coef, ds_stream_t stream);
/* engine/ema.py:40-56 (EMA.update: ema = ema * decay + current * (1 - decay) for every entry of the state dict) as one pass:
 * `tensors` = HOST array of n_tensors records { ema, current (device pointers, fp32), n (int64 element count) } = 3 x 8 bytes
 * each; 96 tensors per launch, descriptors by value (graph-capturable).  The reference's expression term for term: two
 * products and a sum, each rounded to fp32; one_minus_decay = the host's (1 - decay), which is what the reference multiplies by.
 * Any element count >= 1 and any 4-byte alignment of ema and current; neighbours in memory are not touched; after 300 updates the
 * average is within 4 x the distance of torch's float32 expression from float64 (decay 0.99 and 0.9999; measured: at it). */
int ds_ema_multi(const void* tensors, int n_tensors, float decay, float one_minus_decay, ds_stream_t stream);

/* ---- the whole denoiser (Text2ImageTransformer.forward, transformer_utils.py:421-443) ---------- */
enum {  /* per-layer device pointers, layer-major: ptrs[layer * DS_LP_COUNT + slot] */
    DS_LP_ADALN1 = 0,  /* [T][2D]  ln1 table   */
    DS_LP_W_QKV,       /* [3D][D]  attn1 query|key|value */
    DS_LP_B_QKV,       /* [3D] */
    DS_LP_W_PROJ1, DS_LP_B_PROJ1,
    DS_LP_ADALN2,      /* [T][2D]  ln1_1 table */
    DS_LP_W_Q2, DS_LP_B_Q2,
    DS_LP_W_KV2,       /* [2D][Dc] attn2 key|value */
    DS_LP_B_KV2,
    DS_LP_W_PROJ2, DS_LP_B_PROJ2,
    DS_LP_LN2_G, DS_LP_LN2_B,
    DS_LP_W_FC1, DS_LP_B_FC1, DS_LP_W_FC2, DS_LP_B_FC2,
    DS_LP_COUNT
};
typedef struct ds_denoiser_desc {
    int32_t n_layer, n_embd, n_head, seq_len, cond_len, cond_dim, n_codes, n_steps, mlp_mult;
    const float* tok_emb;   /* [n_codes+1][D] */
    const float* pos_emb;   /* [L][D] */
    const float* lnf_g;     /* to_logits.0 */
    const float* lnf_b;
    const float* w_logits;  /* [n_codes][D] */
    const float* b_logits;
    const float* sched;     /* [8][n_steps+1] */
} ds_denoiser_desc;
typedef struct ds_denoiser ds_denoiser;

int ds_denoiser_create(const ds_denoiser_desc* desc, const void* const* layer_ptrs, ds_denoiser** out);
void ds_denoiser_destroy(ds_denoiser* h);
int64_t ds_denoiser_workspace_bytes(const ds_denoiser* h, int B);
int64_t ds_denoiser_kv_bytes(const ds_denoiser* h, int B);
/* Switch the denoiser's per-step GEMMs to the split kernel.  mode DS_SPLIT_F16X2 = f16x2, DS_SPLIT_NONE = back to fp32
 * MFMA (the strict mode).  split[layer*DS_LP_COUNT + slot] holds the packed plane-split of that slot's weight for the
 * DS_LP_W_* slots QKV, PROJ1, Q2, PROJ2, FC1, FC2 (other slots NULL), out_scales[same index] its 2^-s;
 * w_logits_split / logits_scale likewise for to_logits.1.  (Value 1 was the 6-pass bf16 split of rounds 1-4: removed.) */
enum { DS_SPLIT_NONE = 0, DS_SPLIT_F16X2 = 2 };
int ds_denoiser_set_split_weights(ds_denoiser* h, int mode, const void* const* split, const float* out_scales,
                                  const void* w_logits_split, float logits_scale);
/* Padded-row mode of ds_denoiser_step(_ex) (default on): in f16x2 mode, at batch sizes whose GEMMs run the per-sample
 * program (B = 64), every sample occupies 272 rows = 17 packed row groups of the step's activation matrices instead of
 * seq_len = 265 -- tiles start on a group boundary and their ninth block row is 16 rows on the 16x16x32 MFMA (-5 % MFMA
 * work).  The 7 extra rows per sample are zero embeddings that stay finite, are never attention keys, and are skipped by
 * the sampler.  Tokens agree with the unpadded step except on exact near-ties (rows 256..264 of a sample are summed in
 * another order: ~1e-7 relative).  0 switches it off (A/B, bit-for-bit comparisons across batch sizes). */
int ds_denoiser_set_row_padding(ds_denoiser* h, int on);
/* f16x2 range monitor.  FC2's operand (the GELU2 outputs) is the one split site of the denoiser that no normalisation
 * bounds.  With `peak` set (one device float, zeroed by the caller) every forward, step and chain folds max |hi plane| of
 * every layer's GELU2 output into it; the hi plane clamps at 65504, so a peak >= 65504 means the split saturated and the
 * result should be recomputed in the fp32 mode.  NULL (the default) switches the monitor off. */
int ds_denoiser_set_range_monitor(ds_denoiser* h, float* peak);
/* rows per sample of the activation matrices ds_denoiser_step(_ex) would use at batch B: seq_len, or 272 in padded-row mode */
int ds_denoiser_rows_per_sample(const ds_denoiser* h, int B);
/* cross-attention K/V depend only on the caption: computed once per batch (CrossAttention.key/value,
 * transformer_utils.py:96,98).  cond [B][Lc][Dc] -> kv [n_layer][B*Lc][2D] */
int ds_denoiser_cond_kv(const ds_denoiser* h, const float* cond, int B, float* kv, ds_stream_t stream);
/* logits_layout 0: [B*L][K]; 1: [B][K][L] (the reference's output layout) */
int ds_denoiser_forward(const ds_denoiser* h, const int64_t* tokens, const int64_t* t, const float* kv, int B,
                        void* workspace, float* logits, int logits_layout, ds_stream_t stream);
/* forward + ds_sample_tail: tokens_in -> tokens_out for timestep vector t */
int ds_denoiser_step(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t, const float* kv,
                     const float* u, int B, int initial, float trunc_r, void* workspace, int64_t* tokens_out,
                     ds_stream_t stream);

/* the same with the posterior's own timestep vector t_post (NULL = t; sample_fast's skip-step sampler,
 * diffusion_transformer.py:796-803) and top-k truncation */
int ds_denoiser_step_ex(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t, const int64_t* t_post,
                        const float* kv, const float* u, int B, int initial, float trunc_r, int trunc_k,
                        void* workspace, int64_t* tokens_out, ds_stream_t stream);

/* ds_denoiser_step_ex with the noise drawn in the sampler kernel (ds_sample_tail_rng): Philox call index `call` */
int ds_denoiser_step_rng(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t, const int64_t* t_post,
                         const float* kv, const int64_t* gids, unsigned long long seed, int call, int B, int initial,
                         float trunc_r, int trunc_k, void* workspace, int64_t* tokens_out, ds_stream_t stream);

/* A whole reverse chain (DiffusionTransformer.sample's loop, diffusion_transformer.py:639-641; sample_fast's, :790-804)
 * enqueued without returning to the host: n_calls steps, t_steps = DEVICE i64[n_calls][2][B] (per call the network's
 * timestep vector, then the posterior's), tokens [B][seq_len] in: start state / out: result, tokens_tmp same size,
 * call k draws Philox call index call0 + k, initial != 0: the start state is all-[MASK]. */
int ds_denoiser_sample_rng(const ds_denoiser* h, int64_t* tokens, int64_t* tokens_tmp, const int64_t* t_steps,
                           int n_calls, const float* kv, const int64_t* gids, unsigned long long seed, int call0, int B,
                           int initial, float trunc_r, int trunc_k, void* workspace, ds_stream_t stream);

/* Region-held forms of ds_denoiser_step_ex, ds_denoiser_step_rng and ds_denoiser_sample_rng (see ds_sample_tail_hold):
 * keep / known [B][seq_len], mode 0 clamp / 1 renoise (the *_rng entries only).  For the chain the caller supplies the
 * start state in `tokens` (clamp: known where held, [MASK] elsewhere; renoise: held positions diffused to the first
 * timestep), known stays constant over the calls, and call k uses Philox call index call0 + k on both streams. */
int ds_denoiser_step_hold(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t, const int64_t* t_post,
                          const float* kv, const float* u, int B, int initial, float trunc_r, int trunc_k,
                          const unsigned char* keep, const int64_t* known, int mode, void* workspace,
                          int64_t* tokens_out, ds_stream_t stream);
int ds_denoiser_step_hold_rng(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t, const int64_t* t_post,
                              const float* kv, const int64_t* gids, unsigned long long seed, int call, int B,
                              int initial, float trunc_r, int trunc_k, const unsigned char* keep, const int64_t* known,
                              int mode, void* workspace, int64_t* tokens_out, ds_stream_t stream);
int ds_denoiser_sample_hold_rng(const ds_denoiser* h, int64_t* tokens, int64_t* tokens_tmp, const int64_t* t_steps,
                                int n_calls, const float* kv, const int64_t* gids, unsigned long long seed, int call0,
                                int B, int initial, float trunc_r, int trunc_k, const unsigned char* keep,
                                const int64_t* known, int mode, void* workspace, ds_stream_t stream);

/* Guided forms (see ds_sample_tail_guided) of ds_denoiser_step_hold, ds_denoiser_step_hold_rng and
 * ds_denoiser_sample_hold_rng: one forward at batch 2B and the guided tail on the two halves of its logits.
 *   kv         ds_denoiser_cond_kv at batch 2B of the B caption embeddings followed by the B null embeddings
 *   workspace  ds_denoiser_workspace_bytes(h, 2B)
 *   tokens2    i64[2B][seq_len] scratch of the caller: receives the duplicated tokens of every step (on the call's stream)
 *   t, t_post  2B entries, the caller's B repeated (the posterior reads the first B); for the chain t_steps is
 *              i64[n_calls][2][2B]
 * tokens_in / tokens_out / tokens / tokens_tmp / keep / known stay [B][seq_len]; keep == NULL: unheld.  Argument checks
 * (a non-finite scale, the mode / keep / known rules) come before anything is enqueued. */
int ds_denoiser_step_guided(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t, const int64_t* t_post,
                            const float* kv, const float* u, int B, int initial, float trunc_r, int trunc_k, float scale,
                            const unsigned char* keep, const int64_t* known, int mode, int64_t* tokens2, void* workspace,
                            int64_t* tokens_out, ds_stream_t stream);
int ds_denoiser_step_guided_rng(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t, const int64_t* t_post,
                                const float* kv, const int64_t* gids, unsigned long long seed, int call, int B,
                                int initial, float trunc_r, int trunc_k, float scale, const unsigned char* keep,
                                const int64_t* known, int mode, int64_t* tokens2, void* workspace, int64_t* tokens_out,
                                ds_stream_t stream);
int ds_denoiser_sample_guided_rng(const ds_denoiser* h, int64_t* tokens, int64_t* tokens_tmp, const int64_t* t_steps,
                                  int n_calls, const float* kv, const int64_t* gids, unsigned long long seed, int call0,
                                  int B, int initial, float trunc_r, int trunc_k, float scale, const unsigned char* keep,
                                  const int64_t* known, int mode, int64_t* tokens2, void* workspace, ds_stream_t stream);

/* Joint forms (see ds_sample_tail_joint) of the three guided entries: per step ds_joint_gather into tokensN, ONE forward at
 * batch n_cond B W (n_cond 1: unguided, 2: guided at `scale`), the joint tail onto the canvas.
 *   canvas_in / canvas_out / canvas / canvas_tmp / keep / known   [B][Lc]
 *   tokensN    i64[n_cond B W][265] scratch
 *   kv, workspace   at batch n_cond B W; kv: each clip's caption embedding W times (row b W + w), then the B W null ones
 *   t, t_post  i64[n_cond B W], one entry per forward row; the posterior reads entry b W of its vector
 *   t_steps    i64[n_calls][2][n_cond B W]
 *   fade       f32[overlap_cols] on the device
 * Every call is checked before the first is enqueued; the handle's seq_len must be 265. */
int ds_denoiser_step_joint(const ds_denoiser* h, const int64_t* canvas_in, const int64_t* t, const int64_t* t_post,
                           const float* kv, const float* u, int B, int W, int overlap_cols, int ring, int n_cond,
                           const float* fade, int initial, float trunc_r, int trunc_k, float scale, const unsigned char* keep,
                           const int64_t* known, int mode, int64_t* tokensN, void* workspace, int64_t* canvas_out,
                           ds_stream_t stream);
int ds_denoiser_step_joint_rng(const ds_denoiser* h, const int64_t* canvas_in, const int64_t* t, const int64_t* t_post,
                               const float* kv, const int64_t* gids, unsigned long long seed, int call, int B, int W,
                               int overlap_cols, int ring, int n_cond, const float* fade, int initial, float trunc_r,
                               int trunc_k, float scale, const unsigned char* keep, const int64_t* known, int mode,
                               int64_t* tokensN, void* workspace, int64_t* canvas_out, ds_stream_t stream);
int ds_denoiser_sample_joint_rng(const ds_denoiser* h, int64_t* canvas, int64_t* canvas_tmp, const int64_t* t_steps,
                                 int n_calls, const float* kv, const int64_t* gids, unsigned long long seed, int call0, int B,
                                 int W, int overlap_cols, int ring, int n_cond, const float* fade, int initial, float trunc_r,
                                 int trunc_k, float scale, const unsigned char* keep, const int64_t* known, int mode,
                                 int64_t* tokensN, void* workspace, ds_stream_t stream);

/* Composed forms (caption tracks, see ds_sample_tail_composed) of the three guided entries: one forward at batch (C+1)B,
 * C = n_tracks, and the composed tail on the C + 1 slabs of its logits.
 *   kv         ds_denoiser_cond_kv at batch (C+1)B, track-major: track 0's B embeddings, ..., track C-1's, then the B null
 *              embeddings
 *   workspace  ds_denoiser_workspace_bytes(h, (C+1)B)
 *   tokensN    i64[(C+1)B][seq_len] scratch of the caller: receives the tokens of every step copied C + 1 times (on the
 *              call's stream)
 *   t, t_post  (C+1)B entries, the caller's B repeated (the posterior reads the first B); for the chain t_steps is
 *              i64[n_calls][2][(C+1)B]
 *   weights    f32[B][C][seq_len], finite (see ds_sample_tail_composed)
 * tokens_in / tokens_out / tokens / tokens_tmp / keep / known stay [B][seq_len]; keep == NULL: unheld.  The rows per sample
 * are those of the forward's batch, ds_denoiser_rows_per_sample(h, (C+1)B): the padded-row mode may switch on at a smaller
 * B than unguided.  Argument checks (n_tracks, null weights, the mode / keep / known rules) come before anything is
 * enqueued. */
int ds_denoiser_step_composed(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t, const int64_t* t_post,
                              const float* kv, const float* u, int B, int initial, float trunc_r, int trunc_k,
                              int n_tracks, const float* weights, const unsigned char* keep, const int64_t* known, int mode,
                              int64_t* tokensN, void* workspace, int64_t* tokens_out, ds_stream_t stream);
int ds_denoiser_step_composed_rng(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t, const int64_t* t_post,
                                  const float* kv, const int64_t* gids, unsigned long long seed, int call, int B,
                                  int initial, float trunc_r, int trunc_k, int n_tracks, const float* weights,
                                  const unsigned char* keep, const int64_t* known, int mode, int64_t* tokensN,
                                  void* workspace, int64_t* tokens_out, ds_stream_t stream);
int ds_denoiser_sample_composed_rng(const ds_denoiser* h, int64_t* tokens, int64_t* tokens_tmp, const int64_t* t_steps,
                                    int n_calls, const float* kv, const int64_t* gids, unsigned long long seed, int call0,
                                    int B, int initial, float trunc_r, int trunc_k, int n_tracks, const float* weights,
                                    const unsigned char* keep, const int64_t* known, int mode, int64_t* tokensN,
                                    void* workspace, ds_stream_t stream);

/* Purity-prior steps and chains (see ds_sample_tail_purity): forward + purity tail.  t drives the network only (AdaLN);
 * remain = the [MASK] positions a sample may still have after the step; weight = the sharpening weight r.  Region-held
 * sampling needs no further argument: a held position enters as its known token, which no step changes.
 *   tokens2   NULL: unguided -- kv, workspace and t are those of ds_denoiser_step_rng at batch B, scale is not read.
 *             i64[2B][seq_len]: guided with `scale`, on ds_denoiser_step_guided's conventions -- kv and workspace at batch
 *             2B, t with 2B entries (the caller's B repeated), tokens2 receives the duplicated tokens of every step
 *   scratch   ds_purity_scratch_bytes(B, seq_len) bytes; a pointer of its own, the workspace keeps its size
 * The chain runs n_calls steps without returning to the host: t_steps = DEVICE i64[n_calls][B] (guided: [n_calls][2B]),
 * remain = HOST int[n_calls] (read before the call returns), tokens in: the start state / out: the result, tokens_tmp the
 * other end of the ping-pong, call k draws Philox call index call0 + k.  Argument checks come before anything is enqueued. */
int ds_denoiser_step_purity(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t, const float* kv, const float* u,
                            int B, int remain, float weight, float trunc_r, int trunc_k, float scale, int64_t* tokens2,
                            void* workspace, void* scratch, int64_t* tokens_out, ds_stream_t stream);
int ds_denoiser_step_purity_rng(const ds_denoiser* h, const int64_t* tokens_in, const int64_t* t, const float* kv,
                                const int64_t* gids, unsigned long long seed, int call, int B, int remain, float weight,
                                float trunc_r, int trunc_k, float scale, int64_t* tokens2, void* workspace, void* scratch,
                                int64_t* tokens_out, ds_stream_t stream);
int ds_denoiser_sample_purity_rng(const ds_denoiser* h, int64_t* tokens, int64_t* tokens_tmp, const int64_t* t_steps,
                                  const int* remain, int n_calls, const float* kv, const int64_t* gids,
                                  unsigned long long seed, int call0, int B, float weight, float trunc_r, int trunc_k,
                                  float scale, int64_t* tokens2, void* workspace, void* scratch, ds_stream_t stream);

/* Likelihood scoring of B independent (clip, timestep) rows in one call (see ds_score_tail): x_t = ds_q_sample_rng(x0, t) on
 * rng_stream 1 of (gids[b], seed, call) into xt_scratch i64[B][seq_len], the forward at batch B on the step driver's own
 * activation layout (ds_denoiser_rows_per_sample), the score tail on the logits where the forward left them.  kv and
 * workspace as for ds_denoiser_step_rng at batch B; term f64[B]; dbg_pos optional f32[B][seq_len].  t[b] in [0, n_steps) is
 * the caller's to guarantee.  Argument checks come before anything is enqueued. */
int ds_denoiser_score_rng(const ds_denoiser* h, const int64_t* x0, const int64_t* t, const float* kv, const int64_t* gids,
                          unsigned long long seed, int call, int B, void* workspace, int64_t* xt_scratch, double* term,
                          float* dbg_pos, ds_stream_t stream);

/* per-launch HIP-event timing of the denoiser's GEMM launches (measurement only, bench.py) */
int ds_profile_enable(int on);
/* arrays of 4, indexed by GEMM program (0: 128x128, 1: 128x64, 2: 64x64 tiles; 3: the per-sample 288x256 ping-pong
   program of the f16x2 mode) */
int ds_profile_collect(double* ms, double* flops, int64_t* launches);
/* the same for the first n <= 5 programs: 4 = the per-sample program on HALF tiles (144 | 128 x 256: the grids full tiles
   cannot fill, e.g. batch 32); ds_profile_collect folds it into entry 3 */
int ds_profile_collect_n(double* ms, double* flops, int64_t* launches, int n);

/* ---- SpecVQGAN decoder / MelGAN helpers ------------------------------------------------------- */
/* ColumnMajor(reverse) + get_codebook_entry (permuter.py:31-55, quantize.py:88-103) -> [B][H][W][C] */
int ds_codebook_gather(const int64_t* tokens, const float* codebook, float* out, int B, int H, int W, int C,
                       int K, ds_stream_t stream);
/* VectorQuantizer.forward's nearest-code search (vqvae/quantize.py:46-53): z [M][C] encoder output rows,
 * ze [M][K] = z E^T (ds_gemm), ee [K] = row norms^2 of the codebook -> idx [M], dmin [M] optional (may be NULL).
 * d[k] = (sum_c z[c]^2 + ee[k]) - 2 ze[k] in fp32; idx = torch.argmin(d) on EVERY row: a NaN distance is the minimum and
 * the first NaN wins, among equal values the lowest index wins, a row of +inf gives 0 -- so 0 <= idx < K whatever the
 * inputs hold (a non-finite latent, an overflowing |z|^2); dmin = the winning distance, NaN included.  M, C, K > 0. */
int ds_vq_argmin(const float* z, const float* ze, const float* ee, int64_t* idx, float* dmin, int M, int C, int K,
                 ds_stream_t stream);
/* GroupNorm(groups, C, eps) statistics of x [B][P][C] folded into per-(b,c) scale/shift
 * (model.py:34-35); work >= B*ceil(P/256)*2*C doubles.  Sums in double of x minus a per-(sample, group) pivot (the group's
 * first value), one rounding to fp32: scale within 2^-22 relative of the two-pass float64 value, shift within 2^-22 (|beta| +
 * |mean rstd gamma|), for group means up to 1e4 standard deviations.  B, P, C > 0; C % 4 == 0, C <= 1024, groups <= 64. */
int ds_groupnorm_stats(const float* x, int B, int P, int C, int groups, const float* gamma, const float* beta,
                       float eps, double* work, float* scale, float* shift, ds_stream_t stream);
/* its second half alone: part = [B][nchunk][2][C] double partial sums (sum | sum of squares per channel over a chunk of
 * the P pixels) produced elsewhere -- ds_conv3x3_f16x2 writes them per output tile (nchunk = ds_conv3x3_tiles(H, W)) */
int ds_groupnorm_finish(const double* part, int B, int nchunk, int P, int C, int groups, const float* gamma,
                        const float* beta, float eps, float* scale, float* shift, ds_stream_t stream);
/* The decoder's hot 3x3 convolutions as ONE halo-tiled kernel (csrc/conv3x3_f16x2.hip): ResnetBlock conv1 / conv2 with
 * the preceding GroupNorm + swish as a prologue (specvqgan/modules/diffusionmodules/model.py:92-151) and the Upsample
 * conv (:37-52: nearest-2x, then conv).  x [B][H][W][Cin] channels-last fp32 ([B][H/2][W/2][Cin] when up = 1); w2 = the
 * two fp16 planes of W * 2^s (split_f16x2 of W[Cout][9 Cin], K ordered [tap][channel]) in the fragment-packed layout
 * [Cout/128][Cin/32][9][2 planes][2][2][2][64 lanes][8]: lane (hh = lane >> 5, l = lane & 31) of fragment (wn, j, ks) holds
 * W[128 nt + 64 wn + 32 j + l][tap][32 slab + 16 ks + 8 hh + 0..7] (_lib.pack_conv3x3_weights), w_halves = 2 Cout 9 Cin halves
 * in all; out_scale = 2^-s; y = conv(act(x)) + bias (+ residual) [B][H][W][Cout]; stride 1, zero padding 1 (in the activated domain, as
 * the reference pads after the activation).  pro_scale / pro_shift [B][Cin]: GroupNorm folded to a * s + o, followed by
 * swish; NULL = no prologue.  gn_part != NULL: also writes the GroupNorm partial sums of y, [B][ds_conv3x3_tiles(H, W)]
 * [2][Cout] doubles, for ds_groupnorm_finish.  Cin % 32 == 0, Cout % 128 == 0; 3-pass fp16 split, fp32 accumulate. */
int ds_conv3x3_f16x2(const float* x, const void* w2, long long w_halves, float out_scale, const float* bias,
                     const float* residual, float* y, int B, int H, int W, int Cin, int Cout, int up,
                     const float* pro_scale, const float* pro_shift, double* gn_part, ds_stream_t stream);
int ds_conv3x3_tiles(int H, int W);   /* 4 x 32 pixel tiles per image */
/* Dilated k = 3 Conv1d with ReflectionPad1d(dil) (MelGAN ResnetBlock's first conv, vocoder/modules.py:75-78), halo-tiled like
 * ds_conv3x3_f16x2:  y[b][t][n] = bias[n] + 2^-s sum_{j<3} sum_c W[n][j][c] act(x[b][reflect(t + (j - 1) dil)][c]),  act =
 * LeakyReLU(0.2) if lrelu.  x [B][T][Cin], y [B][T][Cout] channels-last fp32; w2 = the fp16 planes of W * 2^s fragment-packed
 * (_lib.pack_conv_weights(.., taps = 3); w_halves = 2 * Cout * 3 * Cin); out_scale = 2^-s.  Cin % 32 == 0, Cout % 128 == 0,
 * 0 < dil <= 27. */
int ds_conv1d_k3_f16x2(const float* x, const void* w2, long long w_halves, float out_scale, const float* bias, float* y, int B,
                       int T, int Cin, int Cout, int dil, int lrelu, ds_stream_t stream);
/* MelGAN ResnetBlock tail (vocoder/modules.py:72-85) in one contraction over K = 2 C: y = W2 LReLU(h) + Ws x + bias, h = the
 * block's dilated k3 conv output [M][C], x = the block input [M][C] (channels-last rows), w = the two fp16 planes of
 * [W2 | Ws] * 2^s ([C][2 C] row-major, w_plane halves apart, split_f16x2), out_scale = 2^-s, bias = b2 + bs.  Replaces the
 * shortcut GEMM + the 1x1 GEMM with residual: the shortcut tensor never goes through HBM.  C % 32 == 0. */
int ds_melgan_resblock_tail(const float* h, const float* x, const void* w, long long w_plane, float out_scale,
                            const float* bias, float* y, int M, int C, ds_stream_t stream);
/* The whole ResnetBlock behind one entry (SURVEY.md section 8b's `ds_melgan_resblock`): y = shortcut(x) +
 * conv1x1(LReLU(conv_k3_dil(reflect_pad_dil(LReLU(x))))).  x, y [B][T][C] channels-last fp32; w3 = the fp16 planes of the
 * weight-norm-folded k3 weights * 2^s ([C][3 C], K ordered [tap][channel]; w3_plane halves apart; w3_scale = 2^-s), b3 [C];
 * wt / wt_plane / wt_scale / bt = ds_melgan_resblock_tail's operands.  C % 32 == 0, 0 < dil < T.
 *   h != NULL: two launches -- the dilated k3 conv into the scratch tensor h ([B][T][C], caller-owned), then
 *              ds_melgan_resblock_tail;
 *   h == NULL: ONE single-pass kernel (x read once, y written once; the intermediate stays in registers) -- built for the
 *              shapes ds_melgan_resblock_fused_ok() accepts (C = 32: T % 128 == 0, dil <= 16; C = 64: T % 256 == 0, dil <= 9), an
 *              error elsewhere. */
int ds_melgan_resblock(const float* x, const void* w3, long long w3_plane, float w3_scale, const float* b3, const void* wt,
                       long long wt_plane, float wt_scale, const float* bt, float* h, float* y, int B, int T, int C,
                       int dil, ds_stream_t stream);
int ds_melgan_resblock_fused_ok(int T, int C, int dil);   /* 1: ds_melgan_resblock(h = NULL) is available for this block */
/* ConvTranspose1d(k = 2 r, stride r, padding pad) in polyphase form on the halo-tiled kernel (MelGAN's stride-8 upsampling layers,
 * vocoder/modules.py:104-113):  y[b][(q + e_p) r + p - pad][n] = bias[n] + 2^-s sum_c (W[p][n][0][c] act(x[b][q + e_p][c]) +
 * W[p][n][1][c] act(x[b][q + e_p - 1][c])),  e_p = p < pad, source rows outside [0, T) zero, act = LeakyReLU(0.2) if lrelu.
 * x [B][T][Cin], y [B][T r][Cout] channels-last fp32; w2 = the r phases' weights [Cout][2 Cin] (tap 0 = W[:, :, p], tap 1 =
 * W[:, :, p + r]), each split (one scale) and fragment-packed (_lib.pack_conv_weights(.., taps = 2)), concatenated;
 * w_halves = r * 2 * Cout * 2 * Cin.  Cin % 32 == 0, Cout % 128 == 0. */
int ds_convt1d_f16x2(const float* x, const void* w2, long long w_halves, float out_scale, const float* bias, float* y, int B, int T,
                     int Cin, int Cout, int r, int pad, int lrelu, ds_stream_t stream);
/* MelGAN's two last upsampling layers in one pass each (vocoder/modules.py:104-113): y [B][2 Tin][Cout] =
 * ConvTranspose1d(k = 4, stride 2, padding 1)(LeakyReLU_0.2(x [B][Tin][Cin])), channels-last fp32.  w = the fp16 planes of the
 * polyphase weights * 2^s, [2 phases][Cout][2 taps][Cin] (phase p: W[:, :, p] on x[s0], W[:, :, p + 2] on x[s0 - 1]), w_plane
 * halves apart; out_scale = 2^-s.  (Cin, Cout) = (128, 64) and (64, 32) are built (ds_melgan_convt2_ok), an error elsewhere. */
int ds_melgan_convt2(const float* x, const void* w, long long w_plane, float out_scale, const float* bias, float* y, int B, int Tin,
                     int Cin, int Cout, ds_stream_t stream);
int ds_melgan_convt2_ok(int Cin, int Cout);
/* Generator tail (vocoder/modules.py:119-124) in one pass: out[b][t] = tanh(bias + sum_j sum_c w[j][c] *
 * LReLU_0.2(x[b][reflect(t + j - 3)][c])), x [B][T][C] channels-last fp32, w [7][C] fp32 (tap-major), out [B][T].
 * C = 32 (ngf = 32) is built; other widths use the 7-column GEMM + ds_stencil7_tanh. */
int ds_melgan_final(const float* x, const float* w, float bias, float* out, int B, int T, int C, ds_stream_t stream);
/* AttnBlock softmax (model.py:214-216): x[row][0..n) <- softmax(scale*x), x[row][n..ld) <- 0 */
int ds_softmax_rows(float* x, int rows, int n, int ld, float scale, ds_stream_t stream);
/* Encoder.conv_in (specvqgan/modules/diffusionmodules/model.py:423-427, :480): Conv2d(1, Cout, 3, stride 1, padding 1) on a
 * ONE-channel image x f32[B][H][W], w [Cout][9] (= weight [Cout][1][3][3]), bias [Cout] -> out f32[B][H][W][Cout]
 * (channels-last).  Direct fp32 multiply-adds, taps in the conv's order; store-bound.  Cout % 4 == 0, divides 1024.  gn_part
 * (may be null): [B][ds_conv3x3_c1_chunks(H, W)][2][Cout] doubles = per-channel sum / sum of squares of the output per row
 * (one chunk per image row), summed in double from the first value; what ds_groupnorm_finish reads (the GroupNorm that
 * follows needs no pass of its own over the output).  W <= 2046. */
int ds_conv3x3_c1(const float* x, const float* w, const float* bias, float* out, int B, int H, int W, int Cout,
                  double* gn_part, ds_stream_t stream);
int ds_conv3x3_c1_chunks(int H, int W);
/* tap-sum for single-output-channel convs fed by a GEMM with N = taps: out[b][y][x] = bias + sum over (ky, kx) in that order
 * of taps[b][y + ky - 1][x + kx - 1][3 ky + kx] (zero padding 1; an fp32 chain), taps [B][H][W][ldt], ldt >= 9; B, H, W > 0 */
int ds_stencil9(const float* taps, int ldt, float bias, float* out, int B, int H, int W, ds_stream_t stream);
/* out[b][t] = tanh(bias + sum_{k<7} taps[b][reflect(t + k - 3)][k]), ReflectionPad1d(3): reflect(s) = -s below 0 and
 * 2 (N - 1) - s past N - 1, ONE bounce -- so N >= 4, like ds_melgan_final's T (PyTorch's ReflectionPad1d(3) refuses N <= 3
 * too); taps [B][N][ldt], ldt >= 7, B > 0.  N < 4 returns -1 and launches nothing. */
int ds_stencil7_tanh(const float* taps, int ldt, float bias, float* out, int B, int N, ds_stream_t stream);
/* mel [B][C][T] -> [B][T][Cpad], y = a*x + b (generate_samples_batch.py:181-182 uses a = b = 0.5) */
int ds_mel_to_cl(const float* mel, float* out, int B, int C, int T, int Cpad, float a, float b,
                 ds_stream_t stream);
/* Join W overlapping window mels into one long mel (csrc/misc.hip).  win f32[B][W][C][F]: window w starts at output frame
 * w S; fade f32[V], V = F - S: the weight of the LATER window over the V frames two neighbours share; out f32[B][C][F + (W-1) S].
 * For output frame tau: w = min(tau / S, W - 1), f = tau - w S;
 *     w >= 1 and f < V:  out = (1 - fade[f]) win[w-1][f + S] + fade[f] win[w][f],     otherwise  out = win[w][f];
 * then out = a out + b (fp32, each operation rounded; a = 1, b = 0 leaves the value as it is).  Requires 0 <= V <= S (at most two
 * windows cover a frame), F % 4 == 0, S % 4 == 0 and 16-byte aligned pointers (fade may be NULL when V == 0); anything else
 * returns -1 and launches nothing. */
int ds_mel_stitch(const float* win, const float* fade, float* out, int B, int W, int C, int F, int S, float a, float b,
                  ds_stream_t stream);
/* Audio front end: waveform -> log-mel spectrogram in one launch (csrc/stft_mel.hip).  Replaces the librosa chain of
 * vocoder/mel2wav/extract_mel_spectrogram.py:15-38,141-187 (= Codebook/feature_extraction/extract_mel_spectrogram.py) and
 * Audio2Mel.forward (vocoder/modules.py:54-69).  Per clip b and frame f:
 *   x      = wave[b] (f32[B][T]) laid on a zero-extended / truncated length `length` (0: T as it is)
 *   xp[i]  = x reflected by `pad` samples at both ends (numpy / torch "reflect": the edge sample is not repeated; pad < length)
 *   S[k]   = | sum_n window[n] xp[256 f + n] e^{-2 pi i k n / 1024} |,  k = 0..512    (FFT in double, |.|^2 rounded to fp32 once,
 *                                                                                    correctly rounded fp32 sqrt; the rest fp32)
 *   m[j]   = sum_k mel_basis[j][k] S[k]  over k ascending in [krange[j][0], krange[j][1])
 *   out[b][j][f - f0] = min(max(a log10(max(m[j], floor)) + c, lo), hi)   for f in [f0, f0 + n_out);  out f32[B][n_mels][n_out]
 * window f32[1024]; twiddle f64[769][2] = (cos, -sin) of 2 pi m / 512 for m < 512, then of 2 pi k / 1024 for k <= 256; mel_basis f32[n_mels][513], any dense matrix; krange i32[n_mels][2] = a range of each row outside
 * which it is zero, or NULL (every row is summed over all 513 bins).  n_fft = 1024 and hop = 256 are the only built sizes;
 * 1 <= n_mels <= 128; floor > 0; lo / hi may be -inf / +inf.  A clip's result is bit-identical whatever the batch around it. */
int ds_wave_to_mel(const float* wave, int B, int T, int length, int pad, const float* window, const double* twiddle,
                   const float* mel_basis, const int32_t* krange, int n_mels, int n_fft, int hop, int f0, int n_out,
                   float a, float c, float lo, float hi, float floor, float* out, ds_stream_t stream);
/* Band-limited rational resampling, one launch for the batch (csrc/resample.hip).  Stands in for `librosa.load(path, sr=22050)`
 * of the reference's data preparation (Codebook/feature_extraction/extract_mel_spectrogram.py:167) and the 32 kHz resampling
 * of its captioning metric (Codebook/AudiocaptionLoss/data_handling/audiocaps_dataset.py:246-260).  With g = gcd(src, dst),
 * L = dst / g, M = src / g, input x[k], k in [0, len_b), zero outside:
 *   N    = ceil(len_b L / M)                                  valid outputs of row b
 *   s    = rho min(1, L / M)                                  cutoff relative to the input Nyquist
 *   h(t) = s sinc(s t) I0(beta sqrt(1 - (s t / Z)^2)) / I0(beta)   for |s t| < Z, else 0       (sinc(u) = sin(pi u) / (pi u))
 *   y[b][n] = sum_k x[b][k] h(n M / L - k) = sum_{j = -W..W} x[b][i0 + j] taps[p][j + W],   p = (n M) mod L, i0 = (n M) div L
 *   Z = 32, beta = 14.769656459379492, rho = 0.9475937167399596, W = ceil(Z / s), taps[p][j + W] = h(p / L - j)
 * taps f32[L][2W+1] is built in float64 on the host and rounded once (audio.resample_taps).  x f32[B][T] (T = row stride);
 * lengths i32[B] on the device (clamped to 0..T) or NULL (= T); y f32[B][n_out], y[b][n] = 0 for n >= N.  fp32 fma over
 * j ascending by one thread per output: a clip's result is bit-identical whatever the batch, its position in it, n_out and the
 * launch.  L / M in lowest terms, both < 2^20; 1024 M / L + 2 W + 2 <= 15360 (M / L up to ~13); n_out == 0 is a no-op. */
int ds_resample(const float* x, int B, int T, const int32_t* lengths, int L, int M, const float* taps, int W,
                float* y, int n_out, ds_stream_t stream);
/* Output levelling (csrc/loudness.hip): gated loudness after ITU-R BS.1770-4, sample peak, mean square and x4 true peak of
 * a batch of mono rows, the gain a strategy asks for, and the gain applied.  x f32[B][T] (T = row stride), lengths i32[B] on
 * the device (clamped to 0..T) or NULL (= T); row b is x[b][0 .. len_b), and a sample at or past len_b is never loaded.
 * S = floor(0.1 fs + 0.5) samples per segment.  kw f64[26], built in float64 on the host (audio.kweight_coeffs, audio.level_plan):
 *   kw[0..4] = b0 b1 b2 a1 a2 of the shelf, kw[5..9] = 1 -2 1 a1 a2 of the high-pass, both from the analogue prototypes
 *       K = tan(pi f0 / fs), a0 = 1 + K/Q + K^2, a1 = 2 (K^2 - 1) / a0, a2 = (1 - K/Q + K^2) / a0,
 *       shelf b = [Vh + Vb K/Q + K^2, 2 (K^2 - Vh), Vh - Vb K/Q + K^2] / a0,  Vh = 10^(G/20), Vb = Vh^0.4996667741545416,
 *       shelf f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; high-pass f0 = 38.13547087602444,
 *       Q = 0.5003270373238773;
 *   kw[10..25] = P = A^S row-major, A the 4x4 state transition of the two biquads in series in transposed direct form II.
 * All filter state and every sum is float64.  With y the K-weighted row (zero state at sample 0):
 *   n_seg  = floor(len_b / S),   seg[b][j] = sum of y^2 over samples [j S, (j+1) S) in sample order, 0 for j >= n_seg
 *   z_j    = (((seg[j] + seg[j+1]) + seg[j+2]) + seg[j+3]) / (4 S),   j = 0 .. n_seg - 4          (400-ms blocks, 75 % overlap)
 *   A      = { j : z_j > 10^((-70 + 0.691)/10) },   G = { j in A : z_j > 0.1 mean_A z }
 *   lufs   = -0.691 + 10 log10(mean_G z),   -inf when A is empty (silence, or len_b < 4 S)
 *   peaks[b] = { max |x|,  max(max |x|, max_n |r[n]|) },  r = the row through the ds_resample sum with L = 4, M = 1 and
 *              taps f32[4][69] = audio.resample_taps(fs, 4 fs) (W = 34; fp32 fma over j ascending; n < 4 len_b); r is never stored
 *   mean_sq  = sum x^2 / len_b (0 for an empty row)
 * Gain of row b, in float64:  DS_LEVEL_PEAK g = 10^(target/20) / max |x|;  DS_LEVEL_RMS g = 10^(target/20) / sqrt(mean_sq);
 * DS_LEVEL_LOUDNESS g = 10^((target - lufs)/20), the target being target_dev[b] (target_n == B) or target_dev[0] (target_n == 1)
 * where target_dev (f64 on the device, e.g. the lufs another call wrote) is not NULL;  DS_LEVEL_MEASURE g = 1.  A measure that is
 * 0 or -inf, or a target that is not finite, gives g = 1.  Then the ceiling c = 10^(ceiling_db/20): if g true_peak > c,
 * g = c / true_peak -- a static cut, not a limiter.  g is rounded to fp32 once, one step further down where that rounding lifted
 * g true_peak above c.  counts (may be NULL) i32[B][2] = |A|, |G|.  ds_level_apply: out[b][i] = fl32(gain[b] x[b][i]) for
 * i < len_b, 0 past it; out may be x; 16-byte accesses where T % 4 == 0 and both pointers are 16-byte aligned.
 * No entry allocates or synchronises: `scratch` (ds_level_scratch_bytes bytes for the same B, T, S; 8-byte aligned) carries the
 * segment states and the partial peaks from ds_level_segments and ds_level_true_peak to ds_level_gain, which runs after both on
 * the same stream.  n_seg_max >= floor(T / S) is the row stride of seg.  A row's every result is bit-identical whatever the batch,
 * its position in it, T and the launch.  Bad arguments return -1 and launch nothing. */
enum { DS_LEVEL_MEASURE = 0, DS_LEVEL_PEAK = 1, DS_LEVEL_RMS = 2, DS_LEVEL_LOUDNESS = 3 };
int64_t ds_level_scratch_bytes(int B, int T, int S);
int ds_level_segments(const float* x, int B, int T, const int32_t* lengths, int S, const double* kw, double* seg,
                      int n_seg_max, void* scratch, int64_t scratch_bytes, ds_stream_t stream);
int ds_level_true_peak(const float* x, int B, int T, const int32_t* lengths, int S, const float* taps, void* scratch,
                       int64_t scratch_bytes, ds_stream_t stream);
int ds_level_gain(const double* seg, int n_seg_max, int B, int T, const int32_t* lengths, int S, int strategy, double target,
                  const double* target_dev, int target_n, double ceiling_db, const void* scratch, int64_t scratch_bytes,
                  double* lufs, float* peaks, double* mean_sq, int32_t* counts, float* gain, ds_stream_t stream);
int ds_level_apply(const float* x, const float* gain, float* out, int B, int T, const int32_t* lengths, ds_stream_t stream);
/* A look-ahead true-peak limiter behind the levelling gain (csrc/limiter.hip): where gain[b] = g0 would lift the x4 true peak of
 * row b above c = 10^(ceiling_db/20), a gain curve takes the row down around its peaks and leaves the rest at g0 -- instead of
 * the static cut of ds_level_gain, which turns the whole row down.  x, lengths, T and taps as for ds_level_true_peak; gain f32[B]
 * on the device (never read on the host).  L = the look-ahead in samples, 1 <= L <= ds_limit_block() = N; a in [0, 1) the release
 * coefficient per sample, exp(-1000 / (release_ms fs)); w f64[L + 1] on the device, non-negative, sum 1 (audio.limit_plan: a
 * Hann shape).  Per row, n = len_b, y4 the x4 signal ds_level_true_peak forms (same taps, fp32 fma over j ascending):
 *   e[i] = max(|x[i]|, |y4[4i + p]|, p = 0..3)                                  fp32
 *   d[i] = max(0, 1 - fl32(c) / (|g0| e[i])),  0 where g0 e[i] = 0, for i < 0 and for i >= n     fp32
 *   m[i] = max d[i .. i + L],  -L <= i < n                                      the hold: a peak is seen L samples ahead
 *   h[i] = max(m[i], a h[i-1]),  h[-L-1] = 0                                    float64: exponential release
 *   s[i] = sum_{k = 0..L} w[k] h[i-k]                                           float64 fma over k ascending; s[i] >= d[i]
 *   g[i] = fl32(1 - s[i]),   out[b][i] = fl32(fl32(g0 g[i]) x[b][i]) for i < n, 0 for n <= i < T;   curve[b][i] = g[i], 1 past n
 * h is evaluated as max(H[i], max d[i+1 .. i+L]) with H[i] = max(d[i], a H[i-1]); a stretch of n' samples acts on H as
 * H -> max(a^n' H, M), so ds_limit_envelope leaves d and M of every block of N samples (cut at k N - L), ds_limit_carry walks
 * H over a row's blocks with one wave (a^N by squaring), and ds_limit_apply runs each block again from its true start state.
 * curve (may be NULL) f32[B][T].  ds_limit_apply also leaves each block's minimum of g in the scratch buffer.  The entries run in
 * this order on one stream, with the same B, T, L, a and scratch (ds_limit_scratch_bytes(B, T, L) bytes, 8-byte aligned; it
 * holds d f32[B][T]).  A time-varying gain does not commute with the x4 interpolation, so `out` is then measured again
 * (ds_level_segments, ds_level_true_peak, ds_level_gain with DS_LEVEL_MEASURE: lufs_in f64[B], peaks f32[B][2]) and
 * ds_limit_finish forms, per row,  tp = peaks[b][1],  trim t = 1 where tp <= c, else fl32((c / tp)(1 - 2^-15)), one fp32 step
 * further down where the rounding lifted t tp above c (1 - 2^-15);  lufs = lufs_in + 20 log10 t;  true_peak = t tp rounded
 * towards zero;  max_reduction = 1 - min_i g[i].  ds_level_apply(out, trim, out) then applies t in place.  The margin 2^-15
 * covers what rounding the scaled samples and their 69 fmas can add to an x4 output (csrc/limiter.hip), so the x4 true peak
 * of the stored row, measured by ds_level_true_peak, is <= c.  No entry allocates or synchronises; 16-byte accesses where
 * T % 4 == 0 and x, out and curve are 16-byte aligned; a row's every result is bit-identical whatever the batch, its position in
 * it, T and the launch.  Bad arguments (a null pointer, L outside 1..N, a outside [0, 1), a ceiling that is not finite, a
 * scratch that is too small) return -1 and launch nothing. */
int ds_limit_block(void);
int64_t ds_limit_scratch_bytes(int B, int T, int L);
int ds_limit_envelope(const float* x, int B, int T, const int32_t* lengths, const float* taps, const float* gain,
                      double ceiling_db, int L, double a, void* scratch, int64_t scratch_bytes, ds_stream_t stream);
int ds_limit_carry(int B, int T, const int32_t* lengths, int L, double a, void* scratch, int64_t scratch_bytes,
                   ds_stream_t stream);
int ds_limit_apply(const float* x, int B, int T, const int32_t* lengths, const float* gain, int L, double a, const double* w,
                   float* out, float* curve, void* scratch, int64_t scratch_bytes, ds_stream_t stream);
int ds_limit_finish(int B, int T, int L, double ceiling_db, const double* lufs_in, const float* peaks, const void* scratch,
                    int64_t scratch_bytes, float* trim, double* lufs, float* true_peak, float* max_reduction,
                    ds_stream_t stream);
/* Pasting a recording back over a rendering of it (csrc/paste.hip): outside the regenerated columns the recording's own values
 * replace the rendering's, cross-faded inside the regenerated columns, with one gain per clip on the rendering.
 * ren / out f32[B C][T] (rows of clip b: b C .. b C + C - 1; C = 1 for waveforms, the mel channels for mel images), rec f32[B C][Tr];
 * off i64[B], rec_len i32[B] (clamped to 0..Tr; NULL = Tr) and keep_cols u8[B][n_cols] on the device.  Position n of a row of
 * clip b reads the recording at i = n + off[b]:  x = rec[row][i] for 0 <= i < rec_len[b], +0 outside (never loaded).
 * A column is col_num / col_den positions long (1 <= both < 2^31):  c = min(n col_den div col_num, n_cols - 1) in int64, and
 *   kept column (keep_cols[b][c] != 0):  out = x, a copy of its 32 bits whatever ren holds;  otherwise, in float64,
 *   dl = (n col_den - c col_num) / col_den        if c > 0 and column c - 1 is kept, else +inf      (numerators exact in int64)
 *   dr = ((c + 1) col_num - n col_den) / col_den  if c < n_cols - 1 and column c + 1 is kept, else +inf
 *   u  = 1 if fade_len == 0 or dl = dr = +inf, else min(1, min(dl, dr) / fade_len)
 *   u == 0: out = x (a copy);   u == 1: out = fl32(g ren) (a copy of ren where sums == NULL);
 *   else out = fl32(g ren wr + x wo),   DS_PASTE_EQUAL_POWER: wr = sin(pi u / 2), wo = cos(pi u / 2);   DS_PASTE_LINEAR: wr = u,
 *   wo = 1 - u.  The fade lies inside the regenerated columns; a clip boundary has none.
 * g = 1 where sums == NULL; else sums f64[B][2] = { S_o, S_r } (what the sums entry below wrote) and g = sqrt(S_o / S_r) clamped
 * to [1/4, 4], g = 1 where either sum is 0 or not finite; sums go with DS_PASTE_EQUAL_POWER only.  out may be ren itself, not rec.
 * Full groups of four positions are stored with 16-byte stores whatever T and the pointers' alignment.
 * The sums entry (C = 1):  S_o = sum x^2, S_r = sum ren^2 over the positions n < T of kept columns with 0 <= n + off[b] <
 * rec_len[b], in float64 (the products are exact) over a fixed partition in a fixed order, without atomics: a row's sums have the
 * same bits whatever the batch, T's padding and the launch.  scratch: ds_paste_scratch_bytes(B, T) bytes, 8-byte aligned.
 * No entry allocates or synchronises.  A null pointer, T <= 0, n_cols < 1, col_num or col_den < 1, a negative or non-finite
 * fade_len or an unknown curve return -1 and launch nothing. */
enum { DS_PASTE_EQUAL_POWER = 0, DS_PASTE_LINEAR = 1 };
int64_t ds_paste_scratch_bytes(int B, int T);
int ds_paste_sums(const float* ren, const float* rec, int B, int T, int Tr, const int64_t* off, const int32_t* rec_len,
                  const uint8_t* keep_cols, int n_cols, int64_t col_num, int64_t col_den, void* scratch, int64_t scratch_bytes,
                  double* sums, ds_stream_t stream);
int ds_paste(const float* ren, const float* rec, float* out, int B, int C, int T, int Tr, const int64_t* off,
             const int32_t* rec_len, const uint8_t* keep_cols, int n_cols, int64_t col_num, int64_t col_den, double fade_len,
             int curve, const double* sums, ds_stream_t stream);
/* Two waveforms side by side (csrc/compare.hip): a the reference f32[B][Na], b the one under test f32[B][Nb], mono, same rate.
 * A lag l pairs b[n] with a[n + l].  The region [s0, s1) of b is the same for every row (per-row lengths and regions are not
 * built): 0 <= s0 < s1 <= Nb, s0 - max_lag >= 0, s1 + max_lag <= Na.  A sample of a outside [0, Na) -- reachable only through a
 * lag given on the device -- is never loaded and counts as 0.  Every product and sum is float64 (the products of two fp32 values
 * are exact); sums run over the region cut into tiles of 8192 samples, n ascending inside a tile, tiles added in order, nothing
 * atomic: a row's bits do not depend on the batch around it or on its position in it.
 * ds_compare_align, for |l - c| <= M = max_lag, 0 <= M <= ds_compare_max_lag() = 4096 (one token column: a design choice):
 *   r(l) = sum_{n in region} b[n] a[n+l],   ea(l) = sum a[n+l]^2,   eb = sum b[n]^2
 *   rho(l) = r / sqrt(ea(l) eb), exactly 0 where ea(l) or eb is 0
 *   lag_out[b] = the l of largest rho (a NaN counts as -inf); among bit-equal rho the smallest |l - c| wins, then the smaller l;
 *   rho[b] = rho(lag_out[b]);  sums[b] = { r, ea, eb } at that lag (f64[B][3]) -- these three once more in double-double over
 *   lanes striding the region (a fixed order), so the reported rho is within a few roundings of its float64 value also where
 *   it is within a few roundings of 1; the search itself compares the plain float64 sums.  Chosen on the device: no host
 *   synchronisation.
 *   The centre c is 0 for a search.  A given lag skips the search: max_lag == 0 and c = lag_dev[b] (i32[B] on the device) or,
 *   with lag_dev NULL, a host integer lag != 0 (then s0 + lag >= 0 and s1 + lag <= Na); lag_out[b] = c and only the
 *   double-double pass runs.  (max_lag == 0 with lag_dev NULL and lag == 0 is a search over the one lag 0: the same numbers.)
 * ds_compare_residual, at lag[b] (i32[B] on the device) with sums[b] as ds_compare_align wrote them for that lag:
 *   alpha = r / ea (0 where ea is 0),  e_res = sum (b[n] - alpha a[n+l])^2,  e_dif = sum (b[n] - a[n+l])^2 -- summed directly --
 *   and ea again in this pass's own order of addition, which is the ea of the two ratios below.
 * ds_compare_stft: three resolutions through the 1024-point double FFT of ds_wave_to_mel (`twiddle` as there): Hann windows
 *   of w = 256, 512, 1024 samples zero-padded to 1024 (windows f32[3][1024] on the device: audio.hann_window(w), then zeros),
 *   hops 64, 128, 256; frame f of b starts at s0 + f hop, f < F = (s1 - s0 - w) div hop + 1, the frame of a lag[b] later; no
 *   reflection, so s1 - s0 >= 1024.  With A, B the magnitudes of a's and b's frames over bins 0..512, in double, it leaves
 *   sum (A - B)^2, sum A^2 and sum |ln max(A, 1e-5) - ln max(B, 1e-5)| per workgroup of 16 frames.  Both transforms are the
 *   same instructions: identical samples give identical magnitudes and exact zeros.
 * ds_compare_finish adds the partials in order and writes, per row,
 *   si_sdr_db = 10 log10(alpha^2 ea / e_res): +inf when e_res == 0, else -inf when alpha^2 ea == 0
 *   snr_db    = 10 log10(ea / e_dif), by the same two rules
 *   sc[b][i]     = sqrt(sum (A - B)^2) / sqrt(sum A^2): 0 when the numerator is 0, +inf when only the denominator is
 *   logmag[b][i] = sum |ln max(A, 1e-5) - ln max(B, 1e-5)| / (513 F)              (f64[B][3] each, i = the resolution)
 * The entries run in this order on one stream with the same B, s0, s1, max_lag and scratch (ds_compare_scratch_bytes(B,
 * s1 - s0, max_lag) bytes, 8-byte aligned; -1 for sizes out of range).  ds_compare_l1: out[b] = sum |x[b][i] - y[b][i]| / n in
 * float64 over fp32 rows of n values, i strided over 256 lanes, the lanes' sums added in a fixed order (the log-mel distance).
 * No entry allocates or synchronises.  A null pointer, max_lag outside 0..4096, a region outside its rules, a region under 1024
 * samples (ds_compare_stft, ds_compare_finish) or a scratch that is too small return -1 and launch nothing. */
int ds_compare_max_lag(void);
int64_t ds_compare_scratch_bytes(int B, int n_region, int max_lag);
int ds_compare_align(const float* a, const float* b, int B, int Na, int Nb, int s0, int s1, int max_lag, const int32_t* lag_dev,
                     int lag, void* scratch, int64_t scratch_bytes, int32_t* lag_out, double* rho, double* sums,
                     ds_stream_t stream);
int ds_compare_residual(const float* a, const float* b, int B, int Na, int Nb, int s0, int s1, int max_lag, const int32_t* lag,
                        const double* sums, void* scratch, int64_t scratch_bytes, ds_stream_t stream);
int ds_compare_stft(const float* a, const float* b, int B, int Na, int Nb, int s0, int s1, int max_lag, const int32_t* lag,
                    const float* windows, const double* twiddle, void* scratch, int64_t scratch_bytes, ds_stream_t stream);
int ds_compare_finish(int B, int s0, int s1, int max_lag, const double* sums, const void* scratch, int64_t scratch_bytes,
                      double* si_sdr_db, double* snr_db, double* sc, double* logmag, ds_stream_t stream);
int ds_compare_l1(const float* x, const float* y, int B, int64_t n, double* out, ds_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
