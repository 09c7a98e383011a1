// Where the KV-cached decode step decides its route: which kernels serve a call of omlm_decode_step, in which order, on which grids, with how
// much LDS and with which per-launch scalars -- or why the call is refused -- as a pure host function of the call.  Every limit, every
// scratch size and every LDS size of the step is stated here once.  No HIP here: the host c++ compiles this header
// (tests/test_decode_plan_host.py checks it against the launches recorded on an MI355X, tests/decode_routes.json, and pins decode.py's
// mirror to it), and both copies of decode.hip execute what it returns.
#pragma once
#include <stdio.h>
#include <string.h>

// ---- geometry of the step kernels (decode.hip's kernels are written against these) ---------------------------------------------------------
#define DEC_T 256
#define DEC_BMAX 8             // samples of the first-generation and of the vector kernels
#define DEC_ROWS 16            // first generation: weight rows per workgroup (4 per wave)
#define DEC_KS 64              // keys per attention split
#define DEC_AT2 512            // workgroup of dec_attn2_kernel
#define DEC2_ROWS 4            // dec2_kernel: weight rows per workgroup
#define DEC4_T 256
#define DEC4_ROWS 16
#define DEC4_NB 16             // samples of a group of the matrix-core step kernels (one MFMA column tile)
#define DEC4_GMAX 4            // groups of DEC4_NB samples per call
#define DEC4_IMG(NS) ((((NS) + 7) / 8) == 1 ? 16 : 8)

namespace omlm_plan __attribute__((visibility("hidden"))) {
// (static: the objects that include this header export nothing of it)

enum { DEC2_QKV = 0, DEC2_OUT = 1, DEC2_FFIN = 2, DEC2_LNGEMV = 3 };       // MODE of dec2_kernel / dec3_kernel / dec4_kernel

constexpr int DEC_ERR_ARG = -1;                 // common.h: OMLM_ERR_ARG
constexpr long long DEC_LDS_CAP = 160 * 1024;   // per workgroup, opted in to once per kernel instantiation
constexpr long long DEC_GEN1_LDS = 150 * 1024;  // what the first-generation kernels budget for their B * Fp staged floats (+ 1 KiB)

// ---- limits ---------------------------------------------------------------------------------------------------------------------------------
// the dec2 / dec3 / dec4 step kernels serve dim 1024 only; everything else runs on the first-generation kernels
static inline bool decode_second_generation(int D, int H, int Fp) {
    return D == 1024 && H * 64 <= 1024 && Fp <= 4096 && Fp % 2 == 0 && (H * 64 + 128) % DEC2_ROWS == 0;
}
// the matrix-core step kernels (dec4_*) serve 16-bit weights with D, H * 64, Fp multiples of 32 and k-loops of at most 4 x 24 steps.
// B > 8: every LayerNorm in front of a matrix-core kernel must find its statistics in the producers' partials (the own-reduction path stages
// fp32 rows for at most 8 samples): ln_parts given
static inline bool decode_matrix_core(int B, int D, int H, int Fp, bool w16, bool ln_parts) {
    return w16 && B >= 2 && B <= DEC4_GMAX * DEC4_NB && (B <= DEC_BMAX || ln_parts) && D % 32 == 0 && D <= 1024 && (H * 64) % 32 == 0 &&
           H * 64 <= 1024 && Fp % 32 == 0 && Fp <= 3072 && Fp % 8 == 0;
}
// whether the step takes the lo planes of FF-in / FF-out / head ("fp16ff"; all three families given): everywhere on the first generation;
// on the second with 16-bit weights and Fp <= 3072, at B >= 2 on the matrix-core kernels with the LayerNorm partials
static inline bool decode_lo_planes_ok(int B, int D, int H, int Fp, bool w16, bool ln_parts) {
    if (!decode_second_generation(D, H, Fp)) return true;
    return w16 && Fp <= 3072 && (B == 1 || (decode_matrix_core(B, D, H, Fp, w16, ln_parts) && ln_parts));
}
// first generation (and every call of at most 8 samples): B * Fp staged floats
static inline bool decode_gen1_lds_ok(int B, int Fp) { return (long long)B * Fp * 4 + 1024 <= DEC_GEN1_LDS; }
// samples one call holds with every scratch pointer given: 16 (wide: 64) where the matrix-core kernels serve the geometry; otherwise 8, or
// fewer where B * Fp floats exceed the LDS budget
static inline int decode_max_batch(int D, int H, int Fp, bool w16, bool wide) {
    if (Fp > 0 && decode_second_generation(D, H, Fp) && decode_matrix_core(2, D, H, Fp, w16, true)) return wide ? DEC4_GMAX * DEC4_NB : DEC4_NB;
    const long long fit = (DEC_GEN1_LDS - 1024) / (4ll * (Fp > 1 ? Fp : 1));
    return (int)(fit < DEC_BMAX ? (fit > 0 ? fit : 0) : DEC_BMAX);
}

// ---- scratch (include/omlm.h: OMLM_DECODE_LN_PARTS_B, OMLM_DECODE_SPLITK_FLOATS_B, OMLM_DECODE_SPLITK_CNT_B) ----------------------------------
static inline int decode_groups(int B) { return (B + DEC4_NB - 1) / DEC4_NB; }                    // groups of 16 samples
static inline int decode_npd(int D) { return (D + DEC4_ROWS - 1) / DEC4_ROWS; }                   // partials of a D-wide output: one per 16 rows
static inline int decode_npf(int Fp) { return (Fp + 7) / 8; }                                     // partials of u: one per 8 channels
// floats of one family's region of one group: [partial][16 samples][2]
static inline int decode_region(int D, int Fp) { const int a = decode_npd(D), b = decode_npf(Fp); return (a > b ? a : b) * 2 * DEC4_NB; }
static inline long long decode_ln_parts_floats(int B, int D, int Fp) { return 3ll * decode_groups(B) * decode_region(D, Fp); }      // [family][group]
static inline long long decode_splitk_floats(int B, int D) { return (long long)decode_groups(B) * 4 * decode_npd(D) * 256; }       // [group][tile][slice][16][16]
// FF-out takes its tickets per (group, tile), the attention combine per sample, in the same array
static inline long long decode_splitk_cnt(int B, int D) {
    const long long t = (long long)decode_groups(B) * decode_npd(D), s = B > DEC4_NB ? B : DEC4_NB;
    return t > s ? t : s;
}

// ---- LDS bytes per workgroup -------------------------------------------------------------------------------------------------------------------
// first generation: the B activation rows of width K + the reduction tail; attention: a 64-key tile pair + q and o of every head
static inline long long dec1_row_lds(int B, int K) { return (long long)B * K * 4 + (DEC_ROWS * DEC_BMAX + 16) * 4; }
static inline long long dec1_attn_lds(int H) { return (long long)(64 * 65 + 64 * 64 + 2 * H * 64) * 4; }
static inline long long dec_attn2_lds(int H) { return (long long)(64 * 65 + 64 * 64 + H * 64 + 8 * 64) * 4; }
static inline long long dec2_lds(int B, int K) { return ((long long)B * K + DEC_BMAX * 8 + DEC_BMAX * 2 + 4 * DEC_BMAX) * 4; }
// dec4_kernel: the 16-bit activation image (PL: hi and lo images of DEC4_IMG rows) of the longest k-range of a workgroup, the reduction
// scratch, and -- own-reduction path only (a LayerNorm without the producers' partials, B <= 8) -- an fp32 staging copy
static inline long long dec4_lds(int NS, bool PL, int B, int K, int nsl, bool gamma, bool stat_in) {
    const int kmax = nsl > 1 ? 32 * (((K >> 5) + nsl - 1) / nsl) : K;
    const int nb = B < DEC4_NB ? B : DEC4_NB;                                          // samples of a workgroup
    return (((long long)(PL ? 2 * DEC4_IMG(NS) : nb) * (kmax + 8) * 2 + 15) & ~15ll) + (long long)(DEC4_NB * 8 + DEC4_NB * 2 + 4 * 256 + 256) * 4 +
           ((gamma && !stat_in) ? (long long)nb * kmax * 4 : 0);
}

// ---- the call, and what it runs --------------------------------------------------------------------------------------------------------------
struct DecodeCall {
    int B, D, H, L, Fp, Nmax, nsplit, V1;
    int w_dtype;            // as the copy sees it: 0 fp32, else its 16-bit type (decode_to_fp16_copy below)
    bool fp16_copy;         // the fp16 copy of decode.hip: it builds no fp32-weight kernels
    bool round_bf16, kv16;
    // which of the optional pointers are there
    bool pos_dev, parts, ids, emb_table, head_W, ln_parts, splitk_ws, splitk_cnt, W1p_lo, W2p_lo, head_W_lo, k_new, advance_pos;
    // omlm_decode_step_masked: the attention launches are the masked kernels, which read key_live[B, Nmax]; everything else of the plan --
    // route, grids, LDS bytes, every other launch -- is the unmasked call's
    bool masked, key_live;
};
// The bf16 copy holds the public entries and hands a call whose weights are fp16 (w_dtype code 2) to the fp16 copy, which sees its 16-bit
// type as code 1.
inline bool decode_to_fp16_copy(DecodeCall& c) {
    if (c.w_dtype != 2) return false;
    c.w_dtype = 1;
    return true;
}
enum DecodeRoute { DEC_GEN1, DEC_DEC3, DEC_DEC2, DEC_DEC4 };      // first generation; second: row kernels (B = 1), vector kernels, matrix-core kernels
enum DecodeKernel {
    DK_EMBED, DK_ROWSTAT,                               // dec_embed_kernel, dec_rowstat_kernel
    DK_QKV1, DK_ATTN1, DK_GEMV1, DK_FFIN1,              // first generation: dec_qkv_kernel, dec_attn_kernel, dec_gemv_kernel, dec_ffin_kernel
    DK_ATTN2, DK_COMBINE,                               // dec_attn2_kernel, dec_attn_combine_kernel
    DK_DEC2, DK_DEC3, DK_DEC3_FFIN, DK_DEC4,            // dec2_kernel, dec3_kernel, dec3_ffin_kernel, dec4_kernel
    DK_ADVANCE,                                         // omlm_decode_advance, after the step's own launches have been checked
    DK_ATTN1_MASKED, DK_ATTN2_MASKED                    // dec_attn_masked_kernel, dec_attn2_masked_kernel (DecodeCall::masked)
};
enum DecodePhase { DP_PROLOGUE, DP_QKV, DP_ATTN, DP_COMBINE, DP_OUT, DP_FFIN, DP_FFOUT, DP_HEAD, DP_ADVANCE };
struct DecodeLaunch {
    DecodeKernel kernel;
    DecodePhase phase;
    bool w16;               // TW: the weights' type (16-bit / float) of the kernels that have one
    bool c16;               // TC of the attention kernels: the cache's type
    int n;                  // NI (dec2, dec3), CPW (dec3_ffin), NS (dec4)
    int mode;               // MODE (DEC2_*)
    bool pl, grp;           // PL: W = hi + lo; GRP: groups of 16 samples along gridDim.y
    int gx, gy, threads;
    long long lds;
    int nsl;                // dec4 FF-out: k-slices per tile (0: whole rows)
    int nstat_in;           // LayerNorm partials to add up (0: the kernel reduces the rows itself)
    int gtiles;             // GRP: the launch's tiles (gridDim.x is padded to a multiple of 8 so that a tile's groups share an XCD)
    bool unrounded;         // a lo-plane launch: round_bf16 cleared
};
struct DecodePlan {
    int rc;                 // 0, or the refusal's return code with msg set; nothing is launched then
    char msg[320];
    DecodeRoute route;
    int G, region, npd, npf;                // groups; floats of one family's region of a group; partials of a D-wide / an Fp-wide output
    bool stat_x, stat_x1, stat_u;           // the live LayerNorm-partial families: x (embed / row sums / FF-out -> q rows, head), x1 (to_out -> FF-in), u (FF-in -> FF-out)
    bool split, comb_in_attn;               // FF-out rows in four k-slices; the attention kernel's last workgroup of a sample combines its partials
    bool rowstat;                           // the caller embedded the ids itself at B > 8: one launch leaves the rows' sums for the first q rows
    int advance;                            // 0: none, 1: rides in the head launch, 2: a launch of its own
    // l[0, layer): prologue; l[layer, tail): ONE layer, launched L times; l[tail, n): head and advance.  The q rows of layers >= 1 are q_rest
    // in place of l[layer]: the same kernel on the same grid, its LayerNorm statistics from the previous layer's FF-out
    int n, layer, tail;
    DecodeLaunch l[10], q_rest;
};

static inline DecodePlan& decode_refuse(DecodePlan& p, const char* text) {
    p.rc = DEC_ERR_ARG; p.n = p.layer = p.tail = 0;
    snprintf(p.msg, sizeof(p.msg), "bad argument: %s", text);
    return p;
}
static inline DecodeLaunch& decode_push(DecodePlan& p, DecodeKernel k, DecodePhase ph, const DecodeCall& c, int gx, int gy, int threads, long long lds) {
    DecodeLaunch& l = p.l[p.n++];
    memset(&l, 0, sizeof(l));
    l.kernel = k; l.phase = ph; l.w16 = c.w_dtype != 0; l.c16 = c.kv16; l.gx = gx; l.gy = gy; l.threads = threads; l.lds = lds;
    return l;
}
// a second-generation weight-row launch: the row kernels at B = 1 (no LDS), else the matrix-core or the vector kernels
static inline DecodeLaunch& decode_push_rows(DecodePlan& p, DecodePhase ph, const DecodeCall& c, DecodeKernel k, int n, int mode, bool pl, int tiles, int K,
                                      bool gamma, int nstat_in, int nsl = 0) {
    const bool grp = k == DK_DEC4 && c.B > DEC4_NB;
    const long long lds = k == DK_DEC4 ? dec4_lds(n, pl, c.B, K, nsl, gamma, nstat_in > 0) : k == DK_DEC2 ? dec2_lds(c.B, K) : 0;
    const int threads = k == DK_DEC4 ? DEC4_T : DEC_T;
    DecodeLaunch& l = decode_push(p, k, ph, c, grp ? (tiles + 7) & ~7 : tiles, grp ? p.G : 1, threads, lds);
    l.n = n; l.mode = mode; l.pl = pl; l.grp = grp; l.nsl = nsl; l.nstat_in = nstat_in; l.gtiles = grp ? tiles : 0; l.unrounded = pl;
    return l;
}

// The refusals carry the texts omlm_decode_step has always returned: the reason, then in brackets the rule as its check was first written.
#define DEC_REFUSE_UNLESS(cond, text) do { if (!(cond)) return decode_refuse(p, text); } while (0)

static inline DecodePlan decode_plan(const DecodeCall& c) {
    DecodePlan p;
    memset(&p, 0, sizeof(p));
    const int B = c.B, D = c.D, H = c.H, Fp = c.Fp, HD = H * 64, V1 = c.V1;
    const bool w16 = c.w_dtype != 0, pl = c.W1p_lo;
    const bool mfma = decode_matrix_core(B, D, H, Fp, w16, c.ln_parts);
    DEC_REFUSE_UNLESS(!c.fp16_copy || c.w_dtype == 1, "the fp16 copy serves fp16 weights only [a->w_dtype == 1]");
    DEC_REFUSE_UNLESS(B >= 1 && B <= DEC4_GMAX * DEC4_NB, "decode batch must be 1..64 [a->B >= 1 && a->B <= DEC4_GMAX * DEC4_NB]");
    DEC_REFUSE_UNLESS(B <= DEC_BMAX || (D == 1024 && mfma),
                      "decode batches of 9..64 run on the matrix-core kernels only (else at most 8): 16-bit weights, D = 1024, ln_parts given "
                      "[a->B <= DEC_BMAX || (a->w_dtype != 0 && a->D == 1024 && dec4_ok(*a))]");
    DEC_REFUSE_UNLESS(B <= DEC4_NB || (c.splitk_ws && c.splitk_cnt),
                      "decode batches of 17..64 need splitk_ws and splitk_cnt (else at most 16) [a->B <= DEC4_NB || (a->splitk_ws && a->splitk_cnt)]");
    DEC_REFUSE_UNLESS(D % 8 == 0 && Fp % 8 == 0 && c.pos_dev && c.parts, "decode geometry [a->D % 8 == 0 && a->Fp % 8 == 0 && a->pos_dev && a->parts]");
    DEC_REFUSE_UNLESS(H >= 1 && H <= 16 && (HD + 128) % DEC_ROWS == 0, "heads [a->H >= 1 && a->H <= 16 && (a->H * 64 + 128) % DEC_ROWS == 0]");
    DEC_REFUSE_UNLESS((long long)c.nsplit * DEC_KS >= c.Nmax, "nsplit must cover Nmax keys [a->nsplit * DEC_KS >= a->Nmax]");
    DEC_REFUSE_UNLESS(B > DEC_BMAX || decode_gen1_lds_ok(B, Fp),
                      "B * Fp exceeds the LDS budget [a->B > DEC_BMAX || (size_t)a->B * a->Fp * sizeof(float) + 1024 <= 150 * 1024]");
    DEC_REFUSE_UNLESS(!c.emb_table || c.ids, "ids required with an embedding table [!a->emb_table || ids]");
    // a 16-bit cache holds the fp32 cache's numbers only where the steps round every key and value to the operand type anyway
    DEC_REFUSE_UNLESS(!c.kv16 || (w16 && c.round_bf16 && c.k_new),
                      "kv16 (16-bit K/V cache) needs 16-bit weights, round_bf16 and the k_new staging row "
                      "[!a->kv16 || (a->w_dtype != 0 && a->round_bf16 != 0 && a->k_new)]");
    DEC_REFUSE_UNLESS(!c.masked || c.key_live, "null key_live [key_live]");
    // (a batch above 8 has passed the matrix-core rule, which implies the second generation: the first-generation kernels never see one)
    const bool gen2 = decode_second_generation(D, H, Fp);
    if (!gen2) {
        // ---- first generation: the advance is always a launch of its own ----
        DEC_REFUSE_UNLESS(!pl || (c.W2p_lo && (!c.head_W || c.head_W_lo)), "lo planes: all three families [a.W2p_lo && (!a.head_W || a.head_W_lo)]");
        p.route = DEC_GEN1;
        if (c.emb_table) decode_push(p, DK_EMBED, DP_PROLOGUE, c, B, 1, DEC_T, 0);
        p.layer = p.n;
        if (c.L > 0) {
            decode_push(p, DK_QKV1, DP_QKV, c, (HD + 128) / DEC_ROWS, 1, DEC_T, dec1_row_lds(B, D));
            decode_push(p, c.masked ? DK_ATTN1_MASKED : DK_ATTN1, DP_ATTN, c, c.nsplit, B, DEC_T, dec1_attn_lds(H));
            decode_push(p, DK_GEMV1, DP_OUT, c, (D + DEC_ROWS - 1) / DEC_ROWS, 1, DEC_T, dec1_row_lds(B, HD));
            decode_push(p, DK_FFIN1, DP_FFIN, c, Fp / 8, 1, DEC_T, dec1_row_lds(B, D)).unrounded = pl;
            decode_push(p, DK_GEMV1, DP_FFOUT, c, (D + DEC_ROWS - 1) / DEC_ROWS, 1, DEC_T, dec1_row_lds(B, Fp)).unrounded = pl;
            p.q_rest = p.l[p.layer];
        }
        p.tail = p.n;
        if (c.head_W) decode_push(p, DK_GEMV1, DP_HEAD, c, (V1 + DEC_ROWS - 1) / DEC_ROWS, 1, DEC_T, dec1_row_lds(B, D)).unrounded = pl;
        p.advance = c.advance_pos ? 2 : 0;
        if (p.advance) decode_push(p, DK_ADVANCE, DP_ADVANCE, c, 1, 1, 64, 0);
        return p;
    }
    // ---- second generation ----
    // LayerNorm partial sums of the matrix-core kernels (dec2_args::stat_in): three regions of ln_parts per group
    const bool stats = mfma && c.ln_parts;
    p.route = B == 1 ? DEC_DEC3 : mfma ? DEC_DEC4 : DEC_DEC2;
    p.G = decode_groups(B); p.npd = decode_npd(D); p.npf = decode_npf(Fp); p.region = decode_region(D, Fp);
    p.stat_x = stats; p.stat_x1 = p.stat_u = stats && c.L > 0;
    // FF-out rows cut into four k-slices: the matrix-core kernels with the producers' partials, scratch given
    p.split = stats && c.splitk_ws && c.splitk_cnt && (Fp >> 5) >= 8;
    p.comb_in_attn = mfma && c.splitk_cnt;
    p.rowstat = !c.emb_table && stats && B > DEC_BMAX;
    // "fp16ff": FF-in / FF-out / head read W = hi + lo and keep their activations and h1 un-rounded
    if (pl) {
        DEC_REFUSE_UNLESS(w16 && c.W2p_lo && (!c.head_W || c.head_W_lo),
                          "lo planes: 16-bit weights, all three families [sizeof(TW) == 2 && a.W2p_lo && (!a.head_W || a.head_W_lo)]");
        DEC_REFUSE_UNLESS(B == 1 || stats, "lo planes at B >= 2 run on the matrix-core step kernels (ln_parts given) [B == 1 || (mfma && st_x)]");
        DEC_REFUSE_UNLESS(Fp <= 3072, "lo planes: feed-forward width <= 3072 [Fp <= 3072]");
    }
    // partials of x that are valid: one per sample behind the prologue, npd behind an FF-out launch
    const int n_x0 = stats && (c.emb_table || p.rowstat) ? 1 : 0, n_xL = stats ? p.npd : 0, n_head = c.L > 0 ? n_xL : n_x0;
    DEC_REFUSE_UNLESS(!(pl && c.head_W) || B == 1 || n_head > 0,
                      "lo planes: the head needs the LayerNorm partials of the last FF-out launch (L >= 1) [B == 1 || h.stat_in]");
    if (c.emb_table) decode_push(p, DK_EMBED, DP_PROLOGUE, c, B, 1, DEC_T, 0);
    else if (p.rowstat) decode_push(p, DK_ROWSTAT, DP_PROLOGUE, c, B, 1, DEC_T, 0);
    p.layer = p.n;
    if (c.L > 0) {
        // q / k / v rows of the new token
        for (int rest = 0; rest < 2; ++rest) {
            const int ns = rest ? n_xL : n_x0;
            if (B == 1) decode_push_rows(p, DP_QKV, c, DK_DEC3, 2, DEC2_QKV, false, (HD + 128 + 3) / 4, D, true, ns);
            else if (mfma) decode_push_rows(p, DP_QKV, c, DK_DEC4, 8, DEC2_QKV, false, (HD + 128) / DEC4_ROWS, D, true, ns);
            else decode_push_rows(p, DP_QKV, c, DK_DEC2, 2, DEC2_QKV, false, (HD + 128) / DEC2_ROWS, D, true, ns);
            if (rest) p.q_rest = p.l[--p.n];
        }
        decode_push(p, c.masked ? DK_ATTN2_MASKED : DK_ATTN2, DP_ATTN, c, c.nsplit, B, DEC_AT2, dec_attn2_lds(H));
        // x1 = x + attn Wo^T.  Matrix cores: combine once (in the attention kernel, or by a launch), then a plain row product
        if (mfma && !p.comb_in_attn) decode_push(p, DK_COMBINE, DP_COMBINE, c, H, B, 64, 0);
        if (mfma) decode_push_rows(p, DP_OUT, c, DK_DEC4, 8, DEC2_LNGEMV, false, p.npd, HD, false, 0);
        else decode_push_rows(p, DP_OUT, c, DK_DEC2, HD <= 512 ? 1 : 2, DEC2_OUT, false, (D + DEC2_ROWS - 1) / DEC2_ROWS, HD, false, 0);
        // FF-in rows + conv + GEGLU
        if (B == 1) decode_push_rows(p, DP_FFIN, c, DK_DEC3_FFIN, pl ? 2 : 4, DEC2_FFIN, pl, pl ? (Fp + 7) / 8 : (Fp + 15) / 16, D, true, 0);
        else if (mfma) decode_push_rows(p, DP_FFIN, c, DK_DEC4, 8, DEC2_FFIN, pl, (Fp + 7) / 8, D, true, stats ? p.npd : 0);
        else decode_push_rows(p, DP_FFIN, c, DK_DEC2, 2, DEC2_FFIN, false, Fp / 2, D, true, 0);
        // x = x1 + LN(u) W2^T
        const int nu = stats ? p.npf : 0;
        if (B == 1 && Fp <= 3072) decode_push_rows(p, DP_FFOUT, c, DK_DEC3, 6, DEC2_LNGEMV, pl, (D + 3) / 4, Fp, true, 0);
        else if (mfma && p.split) decode_push_rows(p, DP_FFOUT, c, DK_DEC4, 6, DEC2_LNGEMV, pl, 4 * p.npd, Fp, true, nu, 4);
        else if (mfma) decode_push_rows(p, DP_FFOUT, c, DK_DEC4, 24, DEC2_LNGEMV, pl, p.npd, Fp, true, nu);
        else decode_push_rows(p, DP_FFOUT, c, DK_DEC2, Fp <= 3072 ? 6 : 8, DEC2_LNGEMV, false, (D + DEC2_ROWS - 1) / DEC2_ROWS, Fp, true, 0);
    }
    p.tail = p.n;
    if (c.head_W) {
        if (B == 1) decode_push_rows(p, DP_HEAD, c, DK_DEC3, 2, DEC2_LNGEMV, pl, (V1 + 3) / 4, D, true, 0);
        else if (mfma) decode_push_rows(p, DP_HEAD, c, DK_DEC4, 8, DEC2_LNGEMV, pl, (V1 + DEC4_ROWS - 1) / DEC4_ROWS, D, true, n_head);
        else decode_push_rows(p, DP_HEAD, c, DK_DEC2, 2, DEC2_LNGEMV, false, (V1 + DEC2_ROWS - 1) / DEC2_ROWS, D, true, 0);
    }
    // the head's workgroup 0 moves the counters on; without a head the advance is a launch of its own
    p.advance = !c.advance_pos ? 0 : c.head_W ? 1 : 2;
    if (p.advance == 2) decode_push(p, DK_ADVANCE, DP_ADVANCE, c, 1, 1, 64, 0);
    return p;
}
#undef DEC_REFUSE_UNLESS

}   // namespace omlm_plan

#ifdef OMLM_PLAN_TEST_ABI       /* tests/test_decode_plan_host.py: the plan behind a flat C interface, built by the host c++ */
// call: B D H L Fp Nmax nsplit V1 w_dtype copy round_bf16 kv16, then one flag per pointer: pos_dev parts ids emb_table head_W ln_parts
// splitk_ws splitk_cnt W1p_lo W2p_lo head_W_lo k_new advance_pos.
//   copy: 0 / 1 the call as the bf16 / fp16 copy sees it; 2 a call of the public entry (decode_to_fp16_copy decides).
// out: rc route G region npd npf stat_x stat_x1 stat_u split comb_in_attn rowstat advance n layer tail, then 16 values per launch (l[0 .. n),
// then q_rest): kernel phase w16 c16 n mode pl grp gx gy threads lds nsl nstat_in gtiles unrounded.  msg: 320 bytes.
// omlm_plan_decode_fp16_copy: whether the fp16 copy serves the call.  omlm_plan_decode: masked off.  omlm_plan_decode_masked: the plan of omlm_decode_step_masked for
// the same 25 values, key_live given or not; same output format.
static omlm_plan::DecodeCall omlm_plan_decode_call(const int* v, bool masked, bool key_live) {
    omlm_plan::DecodeCall c = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9] == 1, v[10] != 0, v[11] != 0, v[12] != 0, v[13] != 0, v[14] != 0,
                               v[15] != 0, v[16] != 0, v[17] != 0, v[18] != 0, v[19] != 0, v[20] != 0, v[21] != 0, v[22] != 0, v[23] != 0, v[24] != 0, masked, key_live};
    if (v[9] == 2) c.fp16_copy = omlm_plan::decode_to_fp16_copy(c);
    return c;
}
static void omlm_plan_decode_out(const omlm_plan::DecodePlan& p, long long* out, char* msg) {
    const long long h[16] = {p.rc, p.route, p.G, p.region, p.npd, p.npf, p.stat_x, p.stat_x1, p.stat_u, p.split, p.comb_in_attn, p.rowstat,
                             p.advance, p.n, p.layer, p.tail};
    memcpy(out, h, sizeof(h));
    for (int i = 0; i <= p.n; ++i) {
        const omlm_plan::DecodeLaunch& l = i < p.n ? p.l[i] : p.q_rest;
        const long long w[16] = {l.kernel, l.phase, l.w16, l.c16, l.n, l.mode, l.pl, l.grp, l.gx, l.gy, l.threads, l.lds, l.nsl, l.nstat_in, l.gtiles, l.unrounded};
        memcpy(out + 16 + 16 * i, w, sizeof(w));
    }
    memcpy(msg, p.msg, sizeof(p.msg));
}
extern "C" int omlm_plan_decode_fp16_copy(const int* v) { return omlm_plan_decode_call(v, false, false).fp16_copy; }
extern "C" void omlm_plan_decode(const int* v, long long* out, char* msg) { omlm_plan_decode_out(omlm_plan::decode_plan(omlm_plan_decode_call(v, false, false)), out, msg); }
extern "C" void omlm_plan_decode_masked(const int* v, int key_live, long long* out, char* msg) {
    omlm_plan_decode_out(omlm_plan::decode_plan(omlm_plan_decode_call(v, true, key_live != 0)), out, msg);
}
extern "C" int omlm_plan_decode_second_generation(int D, int H, int Fp) { return omlm_plan::decode_second_generation(D, H, Fp); }
extern "C" int omlm_plan_decode_matrix_core(int B, int D, int H, int Fp, int w16, int ln_parts) { return omlm_plan::decode_matrix_core(B, D, H, Fp, w16 != 0, ln_parts != 0); }
extern "C" int omlm_plan_decode_lo_planes_ok(int B, int D, int H, int Fp, int w16, int ln_parts) { return omlm_plan::decode_lo_planes_ok(B, D, H, Fp, w16 != 0, ln_parts != 0); }
extern "C" int omlm_plan_decode_max_batch(int D, int H, int Fp, int w16, int wide) { return omlm_plan::decode_max_batch(D, H, Fp, w16 != 0, wide != 0); }
extern "C" void omlm_plan_decode_scratch(int B, int D, int Fp, long long* out) {
    out[0] = omlm_plan::decode_ln_parts_floats(B, D, Fp); out[1] = omlm_plan::decode_splitk_floats(B, D); out[2] = omlm_plan::decode_splitk_cnt(B, D);
}
#endif
