// One sampling-tail launch (sampler.hip), host side: what every ds_sample_tail* entry and the denoiser's step driver
// (api.hip run_step) hand to the one checker and the one launcher.  The caller names the fields it has, the rest stay zero;
// the launcher sorts them into the kernels' argument structs.  (Not in common.h: that file's code is fingerprinted with the
// dominant GEMM kernel, build.source_fingerprint.)
#pragma once
#include "common.h"

enum TailKind { DS_TAIL_POSTERIOR, DS_TAIL_PURITY };

struct TailCall {
    const char* who = nullptr;               // the public entry: every message names it
    TailKind kind = DS_TAIL_POSTERIOR;
    ds_stream_t stream = nullptr;
    const float* logits = nullptr;           // [B * logits_rows][K]
    const float* logits_u = nullptr;         // non-null: guided; the null-condition logits, same layout
    int logits_rows = 0;                     // rows of the logits per sample, >= L (the denoiser's padded-row mode)
    const int64_t* xt = nullptr;
    const int64_t* t = nullptr;              // posterior only, like sched and T
    const float* u = nullptr;                // caller uniforms [B][K+1][L]; nullptr: drawn in the kernel from the Philox
    const int64_t* gids = nullptr;           //   stream of (seed; gids[b], call)
    unsigned long long seed = 0;
    int call = 0;
    const float* sched = nullptr;
    int64_t* out_tokens = nullptr;
    float* dbg_log_pred = nullptr;           // the posterior tail's optional dumps
    float* dbg_trunc = nullptr;
    float* dbg_post = nullptr;
    int B = 0, L = 0, K = 0, T = 0, initial = 0;
    float trunc_r = 0.f;
    int trunc_k = 0;
    const unsigned char* keep = nullptr;     // non-null: region-held, with known and mode (0 clamp, 1 renoise)
    const int64_t* known = nullptr;
    int mode = 0;
    float scale = 0.f;                       // the guidance scale, read with logits_u
    const float* weights = nullptr;          // non-null: composed (caption tracks); f32[B][n_tracks][L] track weights, and
    int n_tracks = 0;                        //   logits holds n_tracks + 1 slabs (tracks, then the null condition),
    size_t track_stride = 0;                 //   track_stride floats apart.  Not with logits_u, not with DS_TAIL_PURITY.
    bool joint = false;                      // true: joint-window sampling (sampler.hip SampleJoint) -- B counts clips, L is the
    int windows = 0, overlap_cols = 0;       //   canvas length, logits (and logits_u) hold one slab of logits_rows rows per
    int ring = 0;                            //   window, xt / out_tokens / keep / known / u are the canvas's
    const float* fade = nullptr;             //   f32[overlap_cols], the later window's weight per overlap column (device)
    int t_stride = 1;                        //   the posterior reads t[b t_stride]
    int remain = 0;                          // purity only, from here on
    float weight = 0.f;
    void* scratch = nullptr;                 // ds_purity_scratch_bytes
    float* dbg_sharp = nullptr;
    float* dbg_key = nullptr;
    int32_t* dbg_cand = nullptr;
};

// (The VALUES of weights live on the device: checking that they are finite would take a synchronisation, so it is the
// caller's job -- the Python layer does it, DiffusionTransformer._tracks.  A non-finite weight gives a non-finite prediction.)
// the token grid of one window, and the canvas of W windows sharing n columns (line or ring): its positions, 0 if none exists
#define DS_GRID_ROWS 5
#define DS_GRID_COLS 53
long long ds_joint_canvas_len(int W, int n, int ring);
int ds_joint_gather_check(const char* who, const int64_t* canvas, const int64_t* win, int B, int W, int n, int ring, int copies);
int ds_joint_gather_launch(const char* who, const int64_t* canvas, int64_t* win, int B, int W, int n, int ring, int copies,
                           ds_stream_t stream);

int ds_sample_tail_check(const TailCall& c);    // every argument rule, once: -1 and a message naming c.who, no HIP call
int ds_sample_tail_launch(const TailCall& c);   // a checked call: fills the kernel arguments, selects the kernel

// One score-tail launch (sampler.hip ds_score_tail_kernel): ds_score_tail and the denoiser's score driver (api.hip) share the
// checker and the launcher, like the sampling tails above.
struct ScoreCall {
    const char* who;
    ds_stream_t stream;
    const float* logits;                     // [B * lrows][K]
    const int64_t* x0;                       // [B][L]
    const int64_t* xt;                       // [B][L]
    const int64_t* t;                        // [B], each row its own timestep
    const float* sched;
    double* term;                            // [B]
    float* dbg_pos;                          // optional [B][L]
    int lrows, B, L, K, T;
};

int ds_score_tail_check(const ScoreCall& c);    // -1 and a message naming c.who, no HIP call
int ds_score_tail_launch(const ScoreCall& c);
