// The epilogue of the per-sample GEMM programs, included INSIDE the kernel bodies of gemm_f16x2_ps.hip (full tiles:
// ds_gemm_f16x2_ps_kernel; half tiles: ds_gemm_f16x2_ph_kernel).  It expects, in scope: p, smem_raw, tid, EPI, NB16, BN,
// acc[..][2], acc8, acc9[2], row_lo / m0 / n0 / L / tm_ (the sample) and the tile geometry
//   WROW       tile rows per wave row (128 / 64);  EROW0  first tile row of the ninth block row (256 / 128)
//   HALF_TILE  compile time: two block rows per wave instead of four;  hasE  the tile has a ninth block row
//   pos0       position of tile row `off` inside the sample (0, or 144 for the second half tile)
//   tile_rows  rows of the sample this tile stores, from tile row `off` on (L; 144 / 128 for half tiles)
    // ---- epilogue -------------------------------------------------------------------------------------------------
    // One workgroup per CU: nothing else runs on the CU while a tile is written out, so the epilogue is on the critical
    // path, and round 3 (tools/probe/probe_ceiling.hip, profiles/r03b_*) found it bound inside the CU, not by HBM: most of it
    // was staging the accumulators through LDS one ds_write_b32 at a time, the slowest data path of the CU, to turn "lane =
    // column, registers run down rows" into 16-byte row pieces.  The main loop multiplies with the operands exchanged
    // (weights first, same products in the same order: same bits), so the accumulators arrive TRANSPOSED:
    //   * a lane owns ONE tile row of a 32 x 32 block, row l31 = lane & 31, and its 16 registers are the columns
    //     (r & 3) + 8 (r >> 2) + 4 hh (hh = lane >> 5): register quad qd = r >> 2 is four consecutive columns 8 qd + 4 hh;
    //   * in the 16 x 16 tiles of the ninth block row (NB16) lane (q = lane >> 4, n = lane & 15) owns tile row
    //     4 PS_SIG(n >> 2) + (n & 3) and the four consecutive columns 4 PS_SIG(q) .. + 3 (see PS_SIG).
    // A register quad is therefore already a 16-byte piece of a row.  The store families (profiles/r11_ps_epilogue_*,
    // NOTEBOOK.md "Round 11"):
    //   * packed planes (EPI_SPLIT: FC1): DIRECT, PS_DIRECT_SPLIT.  Per register quad a lane computes and splits its four
    //     values; lanes l and l + 32 hold the two halves of one 8-column chunk, so one v_permlane32_swap per 32-bit word
    //     hands a PAIR of quads over -- the low wave half ends up with the whole chunk of the even quad, the high half with
    //     the odd quad's -- and the chunk leaves as one 16-byte store per plane.  No LDS, no barrier after the one that ends
    //     the main loop; the row-validity test of the 265-row form is one test per lane and block (a lane is a row).  The
    //     16 x 16 tiles pair lanes that are not 32 apart; their two quads leave as 8-byte stores (16 of 272 rows).  The bias
    //     quads of a lane's columns are requested once, after the main loop.
    //   * the STAGED families share one form.  Steps: step s = 0..3 is block row s of BOTH wave rows, step 4 the ninth block
    //     row; step s writes its quads to LDS buffer s & 1 UNTOUCHED, one ds_write_b128 each, in rows of BN + 4 words (the
    //     odd stride of 65 16-byte slots spreads the rows of a write's service group over all banks); ONE barrier; then all
    //     512 threads read the step back and only now scale, add the bias, activate and split -- a thread's columns are the
    //     same in every step, so its bias values are loaded once -- and store 16 bytes per plane.  The stores of step s run
    //     under the staging of step s + 1 (a buffer is re-written two steps later, behind the barrier in between).
    //       - Q planes / K images of EPI_ATTN (PS_DIRECT_QK = 0): the direct form was measured slower for them -- a store
    //         instruction of the direct form is 16-byte pieces of 32 different rows, of the staged form whole 64- / 128-byte
    //         runs, and these tiles have no GELU to hide the longer store phase behind;
    //       - V^T images (EPI_ATTN, which == 2) need a transposition across rows, which is what LDS is for: a thread gathers
    //         the 8 keys of its 16-byte store with eight ds_read_b32 (PS_VT_W), consecutive lanes write consecutive 16-byte
    //         pieces of one d;
    //       - row-major fp32 + residual (EPI_ROW): read back as whole rows and stored with 16-byte stores next to 16-byte
    //         residual loads that were requested a step ahead.
    // Nothing of the epilogue is held across the main loop, which runs at the 256-register cap: the lane / wave indices are
    // re-derived from an opaque copy of the thread id.  GELU2 by v_exp / v_rcp (ds_gelu2_fast, shared with gemm_f16x2.hip so
    // both programs stay bit-identical).
    int tid_e = tid;
    asm volatile("" : "+v"(tid_e));
    const int l31e = tid_e & 31, hhe = (tid_e >> 5) & 1, wre = tid_e >> 8, wce = (tid_e >> 6) & 3;
    // valid tile rows [off, vhi): the sample's rows (and not past the matrix)
    const int off = row_lo - m0;
    int vhi = off + tile_rows;
    if (vhi > p.M - m0) vhi = p.M - m0;
    const float osc = p.out_scale;
    // 272-row samples (NB16; every half tile): off == 0 and every row of the tile is a row of the sample (M is a whole number
    // of samples), so the per-row validity tests -- per-lane branches around every load and store, behind each of which
    // hipcc waits out vmcnt(0) -- drop out at compile time.
    constexpr bool ALLV = NB16;
    const int qe = (tid_e >> 4) & 3, ne = tid_e & 15;
    // first tile column of the wave's two 32-column blocks and of its block of the ninth block row; the row this lane
    // owns inside the ninth block row; the lane's column inside a block is 8 qd + cq (NB16 tiles: 16 tt + cq9)
    const int cb0 = (wce * 2 + 0) * 32, cb1 = (wce * 2 + 1) * 32, cb9 = (wce * 2 + wre) * 32;
    const int cq = 4 * hhe, cq9 = NB16 ? 4 * PS_SIG(qe) : cq;
    const int r9 = NB16 ? 4 * PS_SIG(ne >> 2) + (ne & 3) : l31e;
    // no bias: the loads read (and discard) the weight plane instead, so that no branch stands around them
    const bool hasb = p.bias != nullptr;
    const float* bsrc = (hasb ? p.bias : (const float*)p.W) + n0;
#define PS_BIAS4(col_) (hasb ? *(const f32x4*)(bsrc + (col_)) : f32x4{0.f, 0.f, 0.f, 0.f})
#define PS_BIAS1(col_) (hasb ? bsrc[col_] : 0.f)
    // what becomes of an accumulator x_ in column bias b_ (ONE expression for every family: the same fma, the same bits)
#define PS_FIN(x_, b_, GELU, t_)                                                                     \
    do {                                                                                             \
        t_ = (x_) * osc + (b_);                                                                      \
        if (GELU) t_ = ds_gelu2_fast(t_);                                                            \
    } while (0)
    constexpr int ELD = BN + 4, EBUF = 64 * ELD;  // staging: words per row / per buffer (64 rows: 65 KB)
    // the tile row of step-local row `rs` (0..63: two groups of 32; step 4: 0..15 / 0..31)
#define PS_TROW(S, rs_) ((S) < 4 ? ((rs_) >> 5) * WROW + (S) * 32 + ((rs_) & 31) : EROW0 + (rs_))
    // every register quad of this wave in step S, as it comes out of the MFMAs: STORE4(step-local row, first tile column,
    // registers).  The staged families write them to LDS untouched -- one ds_write_b128 each, no arithmetic in front of the
    // barrier -- and scale, add the bias and activate AFTER the read-back, where a thread's columns are the same in every
    // step, so that its bias values are loaded once.
#define PS_STEP_QUADS(S, STORE4)                                                                     \
    do {                                                                                             \
        if ((S) < 4) {                                                                               \
            _Pragma("unroll") for (int j = 0; j < 2; ++j)                                            \
                _Pragma("unroll") for (int qd = 0; qd < 4; ++qd) {                                   \
                    const f32x16& A_ = acc[(S) < 4 ? (S) : 0][j];                                    \
                    STORE4(wre * 32 + l31e, (j ? cb1 : cb0) + 8 * qd + cq,                           \
                           (f32x4{A_[4 * qd], A_[4 * qd + 1], A_[4 * qd + 2], A_[4 * qd + 3]}));     \
                }                                                                                    \
        } else if (NB16) {                                                                           \
            _Pragma("unroll") for (int tt = 0; tt < 2; ++tt) STORE4(r9, cb9 + 16 * tt + cq9, acc9[tt]); \
        } else {                                                                                     \
            _Pragma("unroll") for (int qd = 0; qd < 4; ++qd)                                         \
                STORE4(r9, cb9 + 8 * qd + cq9,                                                       \
                       (f32x4{acc8[4 * qd], acc8[4 * qd + 1], acc8[4 * qd + 2], acc8[4 * qd + 3]})); \
        }                                                                                            \
    } while (0)
#define PS_ST_RAW(rs_, cl_, v_) *(f32x4*)(Tf + (rs_) * ELD + (cl_)) = (v_)
    const bool gelu = p.act == DS_ACT_GELU2;
    __syncthreads();                               // every wave is out of the main loop: the operand stages are free

    if constexpr (EPI == PS_EPI_ROW) {
        // row-major fp32 (+ residual): 16-byte residual loads and stores, one row of the tile per wave and iteration.
        // The residual of step S is requested a whole step ahead (PS_ROW_LOAD(S) before the store phase of step S - 2 ...
        // i.e. two steps of residual, 64 registers, are in flight or held at any time): requested just before its own
        // staging -- the first form of this epilogue -- every step waited out a full memory latency (~1.5 us x 5 per tile;
        // the write-only families took half the time of this one).
#define PS_ROW_ITERS(S) (((S) < 4 ? 64 : (NB16 ? 16 : 32)) / 8)       /* 8, or 2 / 4 */
        // tile row of iteration `it` of step S for this thread = PS_ROW_CONST + (tid >> 6): with every row valid (ALLV) the
        // address is a block-uniform row base (SGPRs) + ONE per-thread 32-bit offset for all 34 loads / stores
#define PS_ROW_CONST(S, it) ((S) < 4 ? ((it) >> 2) * WROW + (S) * 32 + 8 * ((it) & 3) : EROW0 + 8 * (it))
#define PS_ROW_LOAD(S, res_, HASR)                                                                   \
    do {                                                                                             \
        _Pragma("unroll") for (int it = 0; it < PS_ROW_ITERS(S); ++it) {                             \
            res_[it] = f32x4{0.f, 0.f, 0.f, 0.f};                                                    \
            if (ALLV) {                                                                              \
                if (HASR) res_[it] = *(const f32x4*)(p.R + (size_t)(m0 + PS_ROW_CONST(S, it)) * p.ldr + n0 + voR); \
            } else {                                                                                 \
                const int trow = PS_TROW(S, (tid_e >> 6) + 8 * it);                                  \
                if ((HASR) && trow >= off && trow < vhi)                                             \
                    res_[it] = *(const f32x4*)(p.R + (size_t)(m0 + trow) * p.ldr + n0 + (tid_e & 63) * 4); \
            }                                                                                        \
        }                                                                                            \
    } while (0)
#define PS_ROW_STAGE(S, res_, HASR)                                                                  \
    do {                                                                                             \
        float* Tf = (float*)smem_raw + ((S) & 1) * EBUF;                                             \
        if (!AHEAD) PS_ROW_LOAD(S, res_, HASR);                                                      \
        PS_STEP_QUADS(S, PS_ST_RAW);                                                                 \
    } while (0)
#define PS_ROW_STORE(S, res_, HASR)                                                                  \
    do {                                                                                             \
        const float* Tf = (const float*)smem_raw + ((S) & 1) * EBUF;                                 \
        const int cc = tid_e & 63, col = n0 + cc * 4;                                                \
        __syncthreads();                                                                             \
        _Pragma("unroll") for (int it = 0; it < PS_ROW_ITERS(S); ++it) {                             \
            const int rs = (tid_e >> 6) + 8 * it, trow = PS_TROW(S, rs);                             \
            if (ALLV || (trow >= off && trow < vhi)) {                                               \
                const f32x4 xx_ = *(const f32x4*)(Tf + rs * ELD + cc * 4);                           \
                f32x4 vv_;                                                                           \
                if (gelu) { _Pragma("unroll") for (int e = 0; e < 4; ++e) PS_FIN(xx_[e], bias4[e], true, vv_[e]); } \
                else { _Pragma("unroll") for (int e = 0; e < 4; ++e) PS_FIN(xx_[e], bias4[e], false, vv_[e]); }    \
                if (HASR) vv_ += res_[it];              /* (no residual: no + 0.f, which would turn -0 into +0) */ \
                if (ALLV) *(f32x4*)(p.C + (size_t)(m0 + PS_ROW_CONST(S, it)) * p.ldc + n0 + voC) = vv_; \
                else *(f32x4*)(p.C + (size_t)(m0 + trow) * p.ldc + col) = vv_;                       \
            }                                                                                        \
        }                                                                                            \
    } while (0)
#define PS_ROW_STEP(S, res_, HASR) do { PS_ROW_STAGE(S, res_, HASR); PS_ROW_STORE(S, res_, HASR); } while (0)
        // (the second request goes out after the first staging: before it, the 144 accumulators + 64 residual registers do
        // not fit the 256-register budget -- hipcc demoted two registers to scratch).  The residual pointer is tested ONCE,
        // around two copies of the sequence: tested per load it is a branch per load again.
        f32x4 resA[8], resB[8];
        const f32x4 bias4 = PS_BIAS4((tid_e & 63) * 4);        // this thread's four columns, the same in every step
        constexpr bool AHEAD = ALLV;                           // (265-row tiles keep the first form: their row tests need the registers)
        const unsigned voR = (unsigned)(tid_e >> 6) * (unsigned)p.ldr + (unsigned)(tid_e & 63) * 4u;
        const unsigned voC = (unsigned)(tid_e >> 6) * (unsigned)p.ldc + (unsigned)(tid_e & 63) * 4u;
#define PS_ROW_ALL(HASR)                                                                             \
    do {                                                                                             \
        if constexpr (!HALF_TILE) {                                                                  \
            if (AHEAD) PS_ROW_LOAD(0, resA, HASR);                                                   \
            PS_ROW_STAGE(0, resA, HASR);                                                             \
            if (AHEAD) PS_ROW_LOAD(1, resB, HASR);                                                   \
            PS_ROW_STORE(0, resA, HASR);                                                             \
            if (AHEAD) PS_ROW_LOAD(2, resA, HASR);                                                   \
            PS_ROW_STEP(1, resB, HASR);                                                              \
            if (AHEAD) PS_ROW_LOAD(3, resB, HASR);                                                   \
            PS_ROW_STEP(2, resA, HASR);                                                              \
            if (AHEAD) PS_ROW_LOAD(4, resA, HASR);                                                   \
            PS_ROW_STEP(3, resB, HASR);                                                              \
            PS_ROW_STEP(4, resA, HASR);                                                              \
        } else {                                                                                     \
            if (AHEAD) PS_ROW_LOAD(0, resA, HASR);                                                   \
            PS_ROW_STAGE(0, resA, HASR);                                                             \
            if (AHEAD) PS_ROW_LOAD(1, resB, HASR);                                                   \
            PS_ROW_STORE(0, resA, HASR);                                                             \
            if (hasE) {                                                                              \
                if (AHEAD) PS_ROW_LOAD(4, resA, HASR);                                               \
                PS_ROW_STEP(1, resB, HASR);                                                          \
                PS_ROW_STEP(4, resA, HASR);                                                          \
            } else {                                                                                 \
                PS_ROW_STEP(1, resB, HASR);                                                          \
            }                                                                                        \
        }                                                                                            \
    } while (0)
        if constexpr (ALLV) {
            if (p.R) PS_ROW_ALL(true); else PS_ROW_ALL(false);
        } else {
            PS_ROW_ALL(p.R != nullptr);
        }
    } else {
        // fp16 split outputs
#define PS_PACK(v_, dst_) do { dst_ = ds_split_pack(v_); } while (0)
        // 8 packed values -> the 8 halves of plane 0 (low halves) and of plane 1 (high halves)
#define PS_UNZIP(x_, hi_, lo_)                                                                       \
    do {                                                                                             \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) {        /* one v_perm_b32 per output word */   \
            hi_[e] = __builtin_amdgcn_perm((x_)[2 * e + 1], (x_)[2 * e], 0x05040100u);               \
            lo_[e] = __builtin_amdgcn_perm((x_)[2 * e + 1], (x_)[2 * e], 0x07060302u);               \
        }                                                                                            \
    } while (0)
        const int hw = p.attn_heads * 64;
        const int which = EPI == PS_EPI_ATTN ? n0 / hw : 0;            // block-uniform: Q, K or V columns
        const int b = tm_;                                               // the sample of this tile
        // a quad, split: the two words of plane 0 (h_) and of plane 1 (l_)
#define PS_QUAD_SPLIT(A_, r0_, bq_, GELU, h_, l_)                                                    \
    do {                                                                                             \
        unsigned x_[4];                                                                              \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                              \
            float t_;                                                                                \
            PS_FIN((A_)[(r0_) + e], (bq_)[e], GELU, t_);                                             \
            PS_PACK(t_, x_[e]);                                                                      \
        }                                                                                            \
        h_[0] = __builtin_amdgcn_perm(x_[1], x_[0], 0x05040100u);                                    \
        h_[1] = __builtin_amdgcn_perm(x_[3], x_[2], 0x05040100u);                                    \
        l_[0] = __builtin_amdgcn_perm(x_[1], x_[0], 0x07060302u);                                    \
        l_[1] = __builtin_amdgcn_perm(x_[3], x_[2], 0x07060302u);                                    \
    } while (0)
        // v_permlane32_swap: the high wave half of a_ and the low wave half of b_ change places
#define PS_SWAP(a_, b_, o0_, o1_)                                                                    \
    do {                                                                                             \
        const auto sw_ = __builtin_amdgcn_permlane32_swap(a_, b_, false, false);                     \
        o0_ = sw_[0];                                                                                \
        o1_ = sw_[1];                                                                                \
    } while (0)
        // where tile row trow_, tile column tcol_ (a multiple of 4) lives: packed planes (EPI_SPLIT), or the Q planes / K
        // images of the attention-ready store
#define PS_DST(trow_, tcol_, d0_, d1_)                                                               \
    do {                                                                                             \
        const int row = m0 + (trow_), col = n0 + (tcol_);                                            \
        if (EPI == PS_EPI_SPLIT) {                                                                   \
            d0_ = (_Float16*)p.C + ds_packed_off(row, col, p.ldc >> 5);                              \
            d1_ = d0_ + p.c_plane;                                                                   \
        } else {                                                                                     \
            const int pos = (trow_) - off + pos0;                                                    \
            const int hc = col - which * hw, head = hc >> 6, d = hc & 63;                            \
            const size_t bh = (size_t)b * p.attn_heads + head;                                       \
            if (which == 0) {                                                                        \
                d0_ = (_Float16*)p.C + (bh * L + pos) * 64 + d;                                      \
                d1_ = d0_ + p.attn_qplane;                                                           \
            } else {                                                                                 \
                d0_ = (_Float16*)p.attn_kv + (bh * 4) * ((size_t)p.attn_nkey * 64) + ds_attn_k_off(pos, d); \
                d1_ = d0_ + (size_t)p.attn_nkey * 64;                                                \
            }                                                                                        \
        }                                                                                            \
    } while (0)
        // one 32 x 32 block from the registers: quads 2 m (columns 16 m + cq ..) and 2 m + 1 (16 m + 8 + cq ..) are
        // exchanged between the wave halves -- every lane takes part, whether its row is valid or not -- after which this
        // lane holds the 8-column chunk at column 16 m + 8 hh of its row in both planes
#define PS_DIRECT_BLOCK(A_, trow_, cb_, bqs_, GELU)                                                  \
    do {                                                                                             \
        const int trw_ = (trow_);                                                                    \
        const bool ok_ = ALLV || (trw_ >= off && trw_ < vhi);                                        \
        _Pragma("unroll") for (int m = 0; m < 2; ++m) {                                              \
            unsigned hA[2], lA[2], hB[2], lB[2];                                                     \
            u32x4 vh, vl;                                                                            \
            PS_QUAD_SPLIT(A_, 8 * m, (bqs_)[2 * m], GELU, hA, lA);                                   \
            PS_QUAD_SPLIT(A_, 8 * m + 4, (bqs_)[2 * m + 1], GELU, hB, lB);                           \
            PS_SWAP(hA[0], hB[0], vh[0], vh[2]);                                                     \
            PS_SWAP(hA[1], hB[1], vh[1], vh[3]);                                                     \
            PS_SWAP(lA[0], lB[0], vl[0], vl[2]);                                                     \
            PS_SWAP(lA[1], lB[1], vl[1], vl[3]);                                                     \
            if (ok_) {                                                                               \
                _Float16 *d0, *d1;                                                                   \
                PS_DST(trw_, (cb_) + 16 * m + 8 * hhe, d0, d1);                                      \
                *(u32x4*)d0 = vh;                                                                    \
                *(u32x4*)d1 = vl;                                                                    \
            }                                                                                        \
        }                                                                                            \
    } while (0)
#define PS_DIRECT_STEP_G(S, GELU)                                                                    \
    do {                                                                                             \
        if ((S) < 4) {                                                                               \
            PS_DIRECT_BLOCK(acc[(S) < 4 ? (S) : 0][0], wre * WROW + (S) * 32 + l31e, cb0, bqd[0], GELU); \
            PS_DIRECT_BLOCK(acc[(S) < 4 ? (S) : 0][1], wre * WROW + (S) * 32 + l31e, cb1, bqd[1], GELU); \
        } else if (NB16) {                                  /* every row of a 272-row sample is valid */ \
            _Pragma("unroll") for (int tt = 0; tt < 2; ++tt) {                                       \
                unsigned h9[2], l9[2];                                                               \
                _Float16 *d0, *d1;                                                                   \
                PS_QUAD_SPLIT(acc9[tt], 0, bqd[2][tt], GELU, h9, l9);                                \
                PS_DST(EROW0 + r9, cb9 + 16 * tt + cq9, d0, d1);                                     \
                *(u32x2*)d0 = u32x2{h9[0], h9[1]};                                                   \
                *(u32x2*)d1 = u32x2{l9[0], l9[1]};                                                   \
            }                                                                                        \
        } else {                                                                                     \
            PS_DIRECT_BLOCK(acc8, EROW0 + r9, cb9, bqd[2], GELU);                                    \
        }                                                                                            \
    } while (0)
#define PS_DIRECT_STEP(S) do { if (gelu) PS_DIRECT_STEP_G(S, true); else PS_DIRECT_STEP_G(S, false); } while (0)
        // the bias quads of this lane's columns (the same in every block row), requested once: [block][quad], [2] = the
        // ninth block row (NB16: its two 16 x 16 tiles)
#define PS_DIRECT_BIAS()                                                                             \
    f32x4 bqd[3][4];                                                                                 \
    _Pragma("unroll") for (int qd = 0; qd < 4; ++qd) {                                               \
        bqd[0][qd] = PS_BIAS4(cb0 + 8 * qd + cq);                                                    \
        bqd[1][qd] = PS_BIAS4(cb1 + 8 * qd + cq);                                                    \
        bqd[2][qd] = NB16 ? PS_BIAS4(cb9 + 16 * (qd & 1) + cq9) : PS_BIAS4(cb9 + 8 * qd + cq9);      \
    }
        // the same tiles STAGED (raw accumulators, PS_STEP_QUADS): a thread reads 8 of them = 32 bytes, finishes and splits
        // them and writes one 16-byte store per plane
#define PS_FIN_SPLIT8(xf_, b8_, x_)                                                                  \
    do {                                                                                             \
        _Pragma("unroll") for (int e = 0; e < 8; ++e) {                                              \
            float t_;                                                                                \
            if (gelu) PS_FIN((xf_)[e], (b8_)[e], true, t_); else PS_FIN((xf_)[e], (b8_)[e], false, t_); \
            PS_PACK(t_, x_[e]);                                                                      \
        }                                                                                            \
    } while (0)
#define PS_SPLIT_STEP(S)                                                                             \
    do {                                                                                             \
        constexpr int rows_ = (S) < 4 ? 64 : (NB16 ? 16 : 32);                                       \
        constexpr int iters_ = rows_ / 16;                      /* 4, or 1 / 2 */                    \
        float* Tf = (float*)smem_raw + ((S) & 1) * EBUF;                                             \
        PS_STEP_QUADS(S, PS_ST_RAW);                                                                 \
        __syncthreads();                                                                             \
        const int cc = tid_e & 31;                                                                   \
        _Pragma("unroll") for (int it = 0; it < iters_; ++it) {                                      \
            const int rs = (tid_e >> 5) + 16 * it, trow = PS_TROW(S, rs);                            \
            if (ALLV || (trow >= off && trow < vhi)) {                                               \
                float xf[8];                                                                         \
                unsigned x[8];                                                                       \
                u32x4 vh, vl;                                                                        \
                *(f32x4*)(xf) = *(const f32x4*)(Tf + rs * ELD + cc * 8);                             \
                *(f32x4*)(xf + 4) = *(const f32x4*)(Tf + rs * ELD + cc * 8 + 4);                     \
                PS_FIN_SPLIT8(xf, bias8, x);                                                         \
                PS_UNZIP(x, vh, vl);                                                                 \
                _Float16 *d0, *d1;                                                                   \
                PS_DST(trow, cc * 8, d0, d1);                                                        \
                *(u32x4*)d0 = vh;                                                                    \
                *(u32x4*)d1 = vl;                                                                    \
            }                                                                                        \
        }                                                                                            \
    } while (0)
        // V^T step: staged ROW-MAJOR like the others (a quad = four d of one key = one ds_write_b128, rows of ELD words) and
        // transposed on the way out: a thread gathers the 8 keys of its 16-byte store with eight ds_read_b32.  Consecutive
        // lanes read 4 units (of 8 keys) x 16 columns: 8 keys x ELD words is half a turn of the 64 banks, so units 0 / 2 and
        // 1 / 3 would meet in the same banks -- rows 16..31 of a group therefore sit with column bit 4 flipped, which moves
        // units 2 and 3 into the 32 banks the others leave free (and moves the 16 rows of a write's service group together).
#define PS_VT_W(g_, r_, cl_) T2[((g_) * 32 + (r_)) * ELD + ((cl_) ^ ((((r_) >> 4) & 1) << 4))]
#define PS_ST_VT(rs_, cl_, v_) *(f32x4*)&PS_VT_W(0, rs_, cl_) = (v_)
        // the 8 keys 8 u_ .. of column cl_ in group g_, finished and split
#define PS_VT_UNIT(g_, r0_, cl_, bv_, x_)                                                            \
    do {                                                                                             \
        float xf_[8], b8_[8];                                                                        \
        _Pragma("unroll") for (int e = 0; e < 8; ++e) { xf_[e] = PS_VT_W(g_, (r0_) + e, cl_); b8_[e] = (bv_); } \
        PS_FIN_SPLIT8(xf_, b8_, x_);                                                                 \
    } while (0)
        // ... and its stores: per group, the valid tile rows [lo, hi) are keys [lo - off, hi - off); 16-byte units of 8
        // keys are aligned in the sample's own key index.  A group whose rows are whole units (the padded-row mode: off = 0)
        // is written 4 units per column with consecutive lanes on consecutive units; otherwise a unit that straddles the
        // group's edge is written in parts (2-byte stores), one column per thread as the first version did.
#define PS_VT_STEP(S)                                                                                \
    do {                                                                                             \
        constexpr int ngrp_ = (S) < 4 ? 2 : 1;                                                       \
        constexpr int grows_ = (S) < 4 ? 32 : (NB16 ? 16 : 32);                                      \
        float* T2 = (float*)smem_raw + ((S) & 1) * EBUF;                                             \
        PS_STEP_QUADS(S, PS_ST_VT);                                                                  \
        __syncthreads();                                                                             \
        const int pln = p.attn_nkey * 64;                                                            \
        _Pragma("unroll") for (int g = 0; g < ngrp_; ++g) {                                          \
            const int G0 = (S) < 4 ? g * WROW + (S) * 32 : EROW0;   /* first tile row of the group */ \
            const int lo = ALLV || G0 > off ? G0 : off;                                              \
            const int hi = ALLV || G0 + grows_ < vhi ? G0 + grows_ : vhi;                            \
            if (!ALLV && lo >= hi) continue;                                                         \
            if (ALLV || (lo == G0 && hi == G0 + grows_ && ((G0 - off) & 7) == 0)) {                  \
                constexpr int upc_ = grows_ / 8;                    /* units per column: 4 (2) */    \
                constexpr int iters_ = BN * upc_ / 512;             /* 2 (1) */                      \
                _Pragma("unroll") for (int it = 0; it < iters_; ++it) {                              \
                    const int task = tid_e + 512 * it, cl = task / upc_, u = task % upc_;            \
                    const int hc = n0 + cl - 2 * hw, head = hc >> 6, d = hc & 63;                    \
                    _Float16* img = (_Float16*)p.attn_kv + (((size_t)b * p.attn_heads + head) * 4 + 2) * (size_t)pln; \
                    unsigned x[8];                                                                   \
                    PS_VT_UNIT(g, 8 * u, cl, upc_ == 4 ? bvt[it] : bvt[2], x);                                    \
                    u32x4 vh, vl;                                                                    \
                    PS_UNZIP(x, vh, vl);                                                             \
                    _Float16* dst = img + ds_attn_vt_off(G0 - off + pos0 + 8 * u, d, p.attn_nkey);   \
                    *(u32x4*)dst = vh;                                                               \
                    *(u32x4*)(dst + pln) = vl;                                                       \
                }                                                                                    \
            } else {                                                                                 \
                const int u_first = (lo - off) >> 3, units = ((hi - off + 7) >> 3) - u_first;        \
                const int cl = tid_e & (BN - 1);                                                     \
                const int hc = n0 + cl - 2 * hw, head = hc >> 6, d = hc & 63;                        \
                _Float16* img = (_Float16*)p.attn_kv + (((size_t)b * p.attn_heads + head) * 4 + 2) * (size_t)pln; \
                for (int u = tid_e >> 8; u < units; u += 2) {                                        \
                    const int k0 = (u_first + u) * 8;               /* first key of the unit */      \
                    const int r0 = k0 + off - G0;                   /* its group-local row (may be < 0) */ \
                    _Float16* dst = img + ds_attn_vt_off(k0 + pos0, d, p.attn_nkey);                 \
                    if (r0 >= lo - G0 && r0 + 8 <= hi - G0) {       /* a whole unit inside the group */ \
                        unsigned x[8];                                                               \
                        PS_VT_UNIT(g, r0, cl, bvt[3], x);                                    \
                        u32x4 vh, vl;                                                                \
                        PS_UNZIP(x, vh, vl);                                                         \
                        *(u32x4*)dst = vh;                                                           \
                        *(u32x4*)(dst + pln) = vl;                                                   \
                    } else {                                                                         \
                        _Pragma("unroll") for (int e = 0; e < 8; ++e)                                \
                            if (r0 + e >= lo - G0 && r0 + e < hi - G0) {                             \
                                float t1;                                                            \
                                if (gelu) PS_FIN(PS_VT_W(g, r0 + e, cl), bvt[3], true, t1);   \
                                else PS_FIN(PS_VT_W(g, r0 + e, cl), bvt[3], false, t1);       \
                                const unsigned x1 = ds_split_pack(t1);                               \
                                dst[e] = __builtin_bit_cast(_Float16, (unsigned short)(x1 & 0xffffu)); \
                                dst[pln + e] = __builtin_bit_cast(_Float16, (unsigned short)(x1 >> 16)); \
                            }                                                                        \
                    }                                                                                \
                }                                                                                    \
            }                                                                                        \
        }                                                                                            \
    } while (0)
        if (EPI == PS_EPI_ATTN && which == 2) {
            // the bias of this thread's columns, requested once: column task / 4 of the two passes over a 32-row group,
            // task / 2 of the 16-row group, and the column of the part-unit path
            const float bvt[4] = {PS_BIAS1(tid_e >> 2), PS_BIAS1((tid_e >> 2) + 128), PS_BIAS1(tid_e >> 1),
                                  PS_BIAS1(tid_e & (BN - 1))};
            if constexpr (!HALF_TILE) {
                PS_VT_STEP(0); PS_VT_STEP(1); PS_VT_STEP(2); PS_VT_STEP(3); PS_VT_STEP(4);
            } else {
                PS_VT_STEP(0); PS_VT_STEP(1);
                if (hasE) PS_VT_STEP(4);
            }
        } else {
            constexpr bool DIRECT = EPI == PS_EPI_SPLIT ? PS_DIRECT_SPLIT : PS_DIRECT_QK;
            if constexpr (DIRECT) {
                PS_DIRECT_BIAS();
                if constexpr (!HALF_TILE) {
                    PS_DIRECT_STEP(0); PS_DIRECT_STEP(1); PS_DIRECT_STEP(2); PS_DIRECT_STEP(3); PS_DIRECT_STEP(4);
                } else {
                    PS_DIRECT_STEP(0); PS_DIRECT_STEP(1);
                    if (hasE) PS_DIRECT_STEP(4);
                }
            } else {
                float bias8[8];                                  // this thread's eight columns, the same in every step
                *(f32x4*)bias8 = PS_BIAS4((tid_e & 31) * 8);
                *(f32x4*)(bias8 + 4) = PS_BIAS4((tid_e & 31) * 8 + 4);
                if constexpr (!HALF_TILE) {
                    PS_SPLIT_STEP(0); PS_SPLIT_STEP(1); PS_SPLIT_STEP(2); PS_SPLIT_STEP(3); PS_SPLIT_STEP(4);
                } else {
                    PS_SPLIT_STEP(0); PS_SPLIT_STEP(1);
                    if (hasE) PS_SPLIT_STEP(4);
                }
            }
        }
    }
#undef PS_TROW
#undef PS_STEP_QUADS
#undef PS_BIAS4
#undef PS_BIAS1
#undef PS_FIN
#undef PS_ST_RAW
#undef PS_FIN_SPLIT8
#undef PS_VT_UNIT
#undef PS_DIRECT_BIAS
#undef PS_ROW_STEP
#undef PS_ROW_ALL
#undef PS_ROW_STAGE
#undef PS_ROW_STORE
#undef PS_ROW_LOAD
#undef PS_ROW_ITERS
#undef PS_ROW_CONST
#undef PS_PACK
#undef PS_QUAD_SPLIT
#undef PS_SWAP
#undef PS_DST
#undef PS_DIRECT_BLOCK
#undef PS_DIRECT_STEP_G
#undef PS_ST_VT
#undef PS_UNZIP
#undef PS_DIRECT_STEP
#undef PS_SPLIT_STEP
#undef PS_VT_W
#undef PS_VT_STEP
