// Where the attention family decides its routes: which kernels serve a call of omlm_mqa_attn_fwd / omlm_mqa_attn_bwd, on which grids, with
// how much LDS -- or why the call is refused -- as pure host functions of the call.  The layout of the prepared table and of the backward's
// workspace, every LDS size and every limit are stated here once.  No HIP here: the host c++ compiles this header
// (tests/test_attn_plan_host.py checks it against the launches recorded on an MI355X, tests/attn_routes.json), and both copies of
// attention.hip, attention2.hip and attention3.hip execute what it returns.
#pragma once
#include <stdio.h>
#include <string.h>

// most positions per sample of causal attention with 16-bit operands (the long forms of attention2.hip / attention3.hip serve 4096 < N <= this);
// reported by omlm_attn_max_positions.  Bounds: the dropout row key holds the key pair index in 15 bits (N < 65536); the dQ kernel's LDS
// grows by one byte per position (108 KiB here).
#define OMLM_ATTN_NL 16384

#ifdef __HIPCC__
#define OMLM_PLAN_HD __host__ __device__ __forceinline__
#else
#define OMLM_PLAN_HD inline
#endif

namespace omlm_plan __attribute__((visibility("hidden"))) {

constexpr int ATTN_UNSUPPORTED = -3;           // common.h: OMLM_ERR_UNSUPPORTED
constexpr long long ATTN_LDS_CAP = 160 * 1024; // per workgroup, opted in to once per kernel instantiation (common.h: launch_lds_cap)
constexpr int ATTN_SHORT = 4096;               // most positions of the short forms

// ---- layout of the prepared table (omlm_attn_bias_prepare: transposed, zero-padded, x log2 e) and of the backward's workspace --------------
constexpr int ATTN_PAD = 64;                   // zero entries in front of each row (rel >= -64)
constexpr int ATTN_BWIN = 128;                 // floats per head in a tile's bias window
inline int attn_prefix_rows(int N, int P) { return P < N ? P : N; }                        // Pn: 0 is causal
inline int attn_prefix_off(int N, int P) { return P > 0 ? attn_prefix_rows(N, P) - 1 : 0; }  // negative distances in front of the causal layout
inline int attn_ldT(int N, int P) { return (ATTN_PAD + attn_prefix_off(N, P) + N + 2 * ATTN_BWIN + 3) / 4 * 4; }   // the table's pitch
// the prepared table of a prefix of P rows (0: causal): the min(P, N) - 1 negative distances in front of the causal layout
inline long long attn_bias_table_floats(int N, int H, int P) { return (long long)((H + 7) / 8 * 8) * attn_ldT(N, P); }
// d(bias) partial rows: one fp32 row of nqt * 32 bins per (sample, head, query tile); the dK / dV slots of N > 4096 start behind them
inline long long attn_dbias_rows_floats(int B, int N, int H) { const long long nqt = (N + 31) / 32; return (long long)B * H * nqt * nqt * 32; }

// ---- attention3.hip's work split -------------------------------------------------------------------------------------------------------------
constexpr int A3_KEYS = 128;                   // keys per workgroup
// PFX: a key range r with 128 r < Pn walks the query tiles from 0 instead of 4 r
OMLM_PLAN_HD int a3_range_start(int r, int Pn) { return 128 * r < Pn ? 0 : 4 * r; }
inline int a3_chunk(int B, int N) {
    const int nqt = (N + 31) / 32, nr = (N + A3_KEYS - 1) / A3_KEYS;
    long long units = 0;
    for (int r = 0; r < nr; ++r) units += nqt - 4 * r;
    long long ch = ((long long)B * units + 1399) / 1400;      // ~5 workgroups per CU (measured: B = 32, N = 1116: CH 4 -> 505 us per layer, 8 -> 522, 2 -> 528)
    if (ch < 2) ch = 2;
    if (ch > 16) ch = 16;
    return (int)ch;
}
// workgroups per sample: key range r is cut into ceil((nqt - start(r)) / CH) chunks of CH query tiles
inline int a3_wg_per_sample(int N, int CH, int Pn) {
    const int nqt = (N + 31) / 32, nr = (N + A3_KEYS - 1) / A3_KEYS;
    int wps = 0;
    for (int r = 0; r < nr; ++r) wps += (nqt - a3_range_start(r, Pn) + CH - 1) / CH;
    return wps;
}
// fp32 elements of the slots attn3_bwd_dkv_part_kernel writes at (B, N): the dK / dV part of the backward's workspace for N > 4096
inline long long a3_part_floats(int B, int N) { return (long long)B * a3_wg_per_sample(N, a3_chunk(B, N), 0) * 2 * A3_KEYS * 64; }
// N <= 4096: the d(bias) rows.  N > 4096: the same rows, then the slots of the dK / dV kernel (a3_part_floats: B x workgroups per sample x
// 64 KiB), which make dK / dV sums of a fixed order there.
inline long long attn_bwd_workspace_bytes(int B, int N, int H) {
    if (B <= 0 || N <= 0 || H <= 0) return 0;
    return (attn_dbias_rows_floats(B, N, H) + (N > ATTN_SHORT ? a3_part_floats(B, N) : 0)) * 4;
}
// the dK / dV kernel addresses q and dout with 32-bit byte offsets, and its plan needs one whole query tile
inline bool a3_serves(int B, int N, int H) { return N >= 32 && (long long)B * N * H * 128 < (1ll << 32); }

// ---- LDS bytes per workgroup ------------------------------------------------------------------------------------------------------------------
inline int attn_ceil(int n, int m) { return (n + m - 1) / m * m; }
// first generation (attention.hip; 32-query x 64-key tiles): K / V tiles (precise: hi / lo planes) + the bias table of 4 heads (dQ: + their
// d(bias) bins, + the key mask words)
inline long long a1_fwd_lds(int N, bool precise, int off) { return (long long)(precise ? 4 : 2) * 64 * 128 + 4ll * (attn_ceil(N, 32) + off) * 4; }
inline long long a1_dq_lds(int N, bool precise, int off) { return (long long)(precise ? 5 : 3) * 64 * 128 + 8ll * (attn_ceil(N, 32) + off) * 4 + 8ll * ((N + 63) / 64 + 1); }
// first-generation dK / dV: every head's bias column is staged in LDS (a prefix: with up to 31 negative distances in front; see
// attn_bwd_dkv_kernel).  The causal kernel reads the prepared table by windows instead where staging would cost occupancy (> 80 KiB: one
// workgroup per CU): below that the staged form measured 2 % faster (B=32, N=1116, H=8: 656 vs 670 us), above it 16 % slower (B=8, N=1817, H=16)
inline long long a1_dkv_staged_lds(int N, int H, bool pfx) { return 32 * 1024 + (long long)H * (attn_ceil(N, 32) + (pfx ? 31 : 0)) * 4 + 1024; }
constexpr long long A1_DKV_WIN_LDS = 32 * 1024 + 4 * 128 * 4;
inline bool a1_dkv_windowed(int N, int H, int Pn, bool biasT) { return Pn == 0 && biasT && a1_dkv_staged_lds(N, H, false) > 80 * 1024; }
// second generation (attention2.hip): a 3-stage ring of 64-key tiles (the kernels static_assert these against their own stage layout)
constexpr long long A4_RING = 3 * (8192 + 8192 + 8 * ATTN_BWIN * 4);       // K rows | V blocked | bias window
constexpr long long A2Q_RING = 3 * (3 * 8192 + 8 * ATTN_BWIN * 4);         // K rows | K blocked | V rows | bias window
constexpr int A2Q_BINW = 128;                                              // d(bias) bins per wave of the long form's ring
// forward: the ring + the sample's liveness (short: 16-bit per key + 64 ballot words; long: per 64 keys 64 x 16-bit + one ballot word) + zeros
inline long long a4_fwd_lds(int N, bool lng) { return A4_RING + (lng ? (long long)((N + 63) / 64) * (64 * 2 + 8) : (long long)attn_ceil(N, 64) * 2 + 64 * 8) + 128; }
// dQ: the ring + 4 KiB scratch + (short) the additive key mask and 8 waves of bins for every distance, the prefix's negative ones included
// (long) 8 bin rings and one mask byte per key
inline long long a2_dq_lds(int N, int off, bool lng) {
    if (lng) return A2Q_RING + 4096 + 8 * A2Q_BINW * 4 + (long long)attn_ceil(N, 64);
    return A2Q_RING + 4096 + (long long)attn_ceil(N, 64) * 4 + 8ll * ((N + 31) / 32 * 32 + off) * 4;
}
// third generation (attention3.hip): 3 stages of two [32][64] blocked images and four per-wave aux pieces (the final transposes reuse it: 4 x 8448 B)
constexpr long long A3_LDS = 3 * (2 * (4096 + 256) + 4 * 2048);

// ---- limits -----------------------------------------------------------------------------------------------------------------------------------
// 16-bit operands, causal, with the prepared table or no bias: OMLM_ATTN_NL (4096 < N runs the long forms of attention2.hip / attention3.hip).
// Everything else past N = 4096 -- fp32 operands ("bf16x3") at any N, a non-causal prefix, a raw table without its prepared form -- runs the
// first-generation kernels, which keep the bias table in LDS: the largest N that fits the forward / the dQ kernel (the dK / dV kernel stages
// H columns where it has no prepared table to read by windows: H (ceil32(N) + 31) floats + 33 KiB, checked per call).
inline int attn1_limit(bool precise, bool backward, int P) {
    int n = 32;
    for (int N = 32; N <= 4 * OMLM_ATTN_NL; N += 32) {
        const int off = attn_prefix_off(N, P);
        if ((backward ? a1_dq_lds(N, precise, off) : a1_fwd_lds(N, precise, off)) > ATTN_LDS_CAP) break;
        n = N;
    }
    return n;
}
// dtype: the public codes (0 fp32, 1 bf16, 2 fp16)
inline int attn_max_positions(int dtype, int P) {
    if (P < 0) return 0;
    if (dtype == 0) return attn1_limit(true, true, P);
    if (dtype != 1 && dtype != 2) return 0;
    if (P == 0) return OMLM_ATTN_NL;
    const int l1 = attn1_limit(false, true, P);
    return l1 > ATTN_SHORT ? l1 : ATTN_SHORT;
}
// the non-causal prefix runs forward and backward on the second-generation kernels (prepared table) iff their plans fit: the dQ kernel's LDS
// (it grows by the Pn - 1 negative-distance bins), the forward's N <= 4096 and the dK / dV kernel's N >= 32; else on attention.hip's
inline bool attn2_prefix_fits(int N, int Pn) { return N >= 32 && N <= ATTN_SHORT && a2_dq_lds(N, Pn - 1, false) <= ATTN_LDS_CAP; }

// ---- the call, and what it runs ------------------------------------------------------------------------------------------------------------
struct AttnCall {
    bool backward;
    int dtype;              // as the copy sees it: 0 fp32 operands ("bf16x3"), anything else its 16-bit type (attn_to_fp16_copy below)
    bool fp16_copy;         // the fp16 copy of the three files: it builds no fp32 kernels
    int B, N, H, P;
    bool bias, biasT, dbias, ws;     // which of the raw table, the prepared table, d(bias) and the workspace are there
    bool drop;              // dropout p > 0
    bool dkv_adjacent;      // dv == dk + B N 64: one zero fill instead of two
};
// The bf16 copy holds the public entries and hands a call that names fp16 (dtype code 2) to the fp16 copy, which sees its 16-bit type as code 1.
inline bool attn_to_fp16_copy(AttnCall& c) {
    if (c.dtype != 2) return false;
    c.dtype = 1;
    return true;
}
// what the launch loops of attention.hip take next to the plan: the entry's pointers and scalars, filled once (host only: no kernel takes it)
struct AttnArgs {
    const void *q, *k, *v, *dout;
    const float *bias, *biasT;
    const unsigned char* keymask;
    void* out;                       // (the backward reads it, and lse)
    float *lse, *delta, *dq, *dk, *dv, *dbias, *dbias_ws;
    float scale, p;                  // p, seed, seed_dev: dropout
    int bias_ld;
    unsigned long long seed;
    const unsigned long long* seed_dev;
    void* stream;
};
enum AttnFamily {
    ATTN_A1_FWD, ATTN_A1_DQ, ATTN_A1_DKV,      // attention.hip: attn_fwd_kernel, attn_bwd_dq_kernel / attn_bwd_dq_precise_kernel, attn_bwd_dkv_kernel
    ATTN_A4_FWD, ATTN_A2_DQ, ATTN_DBIAS_REDUCE, // attention2.hip: attn4_fwd_kernel, attn2_bwd_dq_kernel (and their long forms), attn_dbias_reduce_kernel
    ATTN_A3_ZERO, ATTN_A3_DKV, ATTN_A3_REDUCE   // attention3.hip: a3_zero_kernel, attn3_bwd_dkv_kernel (and its part form), a3_part_reduce_kernel
};
enum AttnForm { ATTN_FORM_SHORT, ATTN_FORM_LONG, ATTN_FORM_PART };
struct AttnLaunch {
    AttnFamily family;
    AttnForm form;
    bool precise;           // the fp32 instantiation (first generation only)
    bool pfx, drop, fixed;  // template arguments PFX, DROP, FIXED (attn4_fwd: fixed-reference softmax; the online form follows it)
    bool win;               // ATTN_A1_DKV: reads the prepared table by windows
    int gx, gy, gz, threads;
    long long lds;
    int CH, wps;            // attention3.hip: query tiles per chunk, workgroups per sample
    int which;              // ATTN_A3_ZERO: 0 = from dk, 1 = from dv
    long long floats;       // ATTN_A3_ZERO: elements to fill
};
struct AttnPlan {
    int rc;                 // 0, or the refusal's return code with msg set; nothing is launched then
    char msg[480];
    int n;
    AttnLaunch l[5];
    int ldT;                // pitch of the prepared table
    long long dkv_slots;    // offset (floats) of the dK / dV slots in the workspace, -1: no slot form
};

inline void attn_push(AttnPlan& p, AttnFamily f, AttnForm form, const AttnCall& c, int gx, int gy, int gz, int threads, long long lds) {
    AttnLaunch& l = p.l[p.n++];
    memset(&l, 0, sizeof(l));
    l.family = f; l.form = form; l.precise = c.dtype == 0 && f <= ATTN_A1_DKV; l.pfx = c.P > 0; l.drop = c.drop;
    l.gx = gx; l.gy = gy; l.gz = gz; l.threads = threads; l.lds = lds;
}
inline AttnPlan& attn_refuse(AttnPlan& p) { p.rc = ATTN_UNSUPPORTED; p.n = 0; return p; }

// Refusals that name their reason, before anything is launched.
inline bool attn_positions_ok(const AttnCall& c, const char* what, AttnPlan& p) {
    const int N = c.N, P = c.P, H = c.H;
    const char* dir = c.backward ? "backward" : "forward alone";
    if (c.dtype == 0) {
        const int lim = attn1_limit(true, c.backward, P);
        if (N <= lim) return true;
        snprintf(p.msg, sizeof(p.msg), "%s: N = %d positions per sample with fp32 operands (bf16x3): their kernels keep the bias table in LDS and take "
                 "N <= %d (%s; omlm_attn_max_positions); bf16 / fp16 operands take N <= %d", what, N, lim, dir, OMLM_ATTN_NL);
        return false;
    }
    if (N <= ATTN_SHORT) return true;
    if (P > 0 || (c.bias && !c.biasT)) {                       // first-generation kernels, as far as they reach
        const int lim = attn1_limit(false, c.backward, P);
        if (N <= lim && (!c.backward || a1_dkv_staged_lds(N, H, P > 0) <= ATTN_LDS_CAP)) return true;
        if (P > 0)
            snprintf(p.msg, sizeof(p.msg), "%s: N = %d positions per sample with a non-causal prefix (P = %d): past N = 4096 a prefix runs the "
                     "first-generation kernels, whose LDS-resident bias tables take N <= %d (%s) and, in the backward, H (N + 31) <= 31000 "
                     "(H = %d); the long forms (4096 < N <= %d) are causal", what, N, P, lim, dir, H, OMLM_ATTN_NL);
        else
            snprintf(p.msg, sizeof(p.msg), "%s: N = %d > 4096 positions per sample needs the prepared table (biasT, omlm_attn_bias_prepare) next "
                     "to bias; with the raw table alone N <= %d (%s) and, in the backward, H N <= 31000 (H = %d)", what, N, lim, dir, H);
        return false;
    }
    if (N <= OMLM_ATTN_NL) return true;
    snprintf(p.msg, sizeof(p.msg), "%s: N = %d positions per sample is past the limit of %d (omlm_attn_max_positions)", what, N, OMLM_ATTN_NL);
    return false;
}
inline bool attn_lds_ok(long long bytes, AttnPlan& p) {
    if (bytes <= ATTN_LDS_CAP) return true;
    snprintf(p.msg, sizeof(p.msg), "attention: sequence too long for the LDS-resident bias table");
    return false;
}

// 16-bit operands with the prepared table, or without any bias: attention2.hip / attention3.hip (a prefix only while attn2_prefix_fits -- the
// SAME test forward and backward, whose lse is relative to the table's reference point there)
inline bool attn_second_generation(const AttnCall& c) {
    const int Pn = attn_prefix_rows(c.N, c.P);
    return c.dtype != 0 && (c.biasT || !c.bias) && (Pn == 0 || attn2_prefix_fits(c.N, Pn));
}

inline AttnPlan attn_plan(const AttnCall& c) {
    AttnPlan p;
    memset(&p, 0, sizeof(p));
    p.dkv_slots = -1;
    const char* what = c.backward ? "omlm_mqa_attn_bwd" : "omlm_mqa_attn_fwd";
    const int B = c.B, N = c.N, H = c.H, Pn = attn_prefix_rows(N, c.P), off = attn_prefix_off(N, c.P);
    if (!attn_positions_ok(c, what, p)) return attn_refuse(p);
    if (c.dtype == 0 && c.fp16_copy) {
        snprintf(p.msg, sizeof(p.msg), "%s: fp32 operands are served by the bf16 copy of the library", what);
        return attn_refuse(p);
    }
    const bool gen2 = attn_second_generation(c);
    const bool lng = N > ATTN_SHORT;                           // (gen2: the long forms; the positions check has refused a prefix there)
    const int nqt = (N + 31) / 32;
    p.ldT = gen2 || Pn == 0 ? attn_ldT(N, c.P) : 0;
    if (!c.backward) {
        if (gen2) {
            // both softmax forms: the one the table's flag does not name returns at its first instruction (no table: online only)
            const long long lds = a4_fwd_lds(N, lng);
            for (int fixed = c.biasT ? 1 : 0; fixed >= 0; --fixed) {
                attn_push(p, ATTN_A4_FWD, lng ? ATTN_FORM_LONG : ATTN_FORM_SHORT, c, nqt * ((H + 7) / 8) * B, 1, 1, 256, lds);
                p.l[p.n - 1].fixed = fixed != 0;
            }
            return p;
        }
        const long long lds = a1_fwd_lds(N, c.dtype == 0, off);
        if (!attn_lds_ok(lds, p)) return attn_refuse(p);
        attn_push(p, ATTN_A1_FWD, ATTN_FORM_SHORT, c, nqt, (H + 3) / 4, B, 256, lds);
        return p;
    }
    // ---- backward: dQ (+ delta, d(bias)), the d(bias) reduction where a workspace holds its partial rows, dK / dV ----
    // The prepared table (or no bias): attention2.hip's dQ kernel (8 heads per workgroup sharing LDS-DMA-staged K / V tiles) and attention3.hip's
    // dK / dV kernel (128 keys per workgroup, Q / dO staged once per workgroup by LDS-DMA).  With the Horner diagonal sums and the d(bias)
    // workspace the dQ kernel is the faster one at both bench shapes (B=32, N=1116, H=8: whole backward 432 against 456 us; before those two
    // changes both kernels spent ~160 us per layer in d(bias) and the first-generation kernel led 316 : 334).  Causal: each falls back to
    // its first-generation kernel where its plan does not fit.  A prefix runs them iff attn2_prefix_fits -- the forward's test -- so a
    // "does not fit" is an error there, not a fallback.
    const bool win = a1_dkv_windowed(N, H, Pn, c.biasT);
    const bool dq2 = gen2 && (lng || a2_dq_lds(N, off, false) <= ATTN_LDS_CAP);
    const bool dkv3 = gen2 && a3_serves(B, N, H);
    const long long ldsq = a1_dq_lds(N, c.dtype == 0, off), ldsk = win ? A1_DKV_WIN_LDS : a1_dkv_staged_lds(N, H, Pn > 0);
    // N > 4096, causal, with the prepared table or no bias: the long dQ kernel, and with a workspace the dK / dV kernel's slot form -- its slots
    // follow the d(bias) rows in the workspace.  Where the dK / dV kernel's 32-bit offsets refuse the shape, the first-generation kernel takes
    // over in its windowed mode, which needs the prepared table.
    if (gen2 && lng && !win && !dkv3) {
        snprintf(p.msg, sizeof(p.msg), "%s: B N H >= 2^25 with N > 4096 and no prepared table (biasT) is not served: the dK / dV kernel addresses q "
                 "and dout with 32-bit byte offsets (B N H 128 < 2^32), and the windowed first-generation kernel behind it reads biasT -- "
                 "pass the prepared table (an all-zero one, omlm_attn_bias_prepare with bias = NULL, where there is no bias) or split the batch", what);
        return attn_refuse(p);
    }
    if (gen2 && Pn > 0 && !dkv3) {
        snprintf(p.msg, sizeof(p.msg), "%s: B N H >= 2^25 with a non-causal prefix on the prepared table is not served: the dK / dV kernel addresses q "
                 "and dout with 32-bit byte offsets (B N H 128 < 2^32), and the first-generation kernel behind it would not share the "
                 "forward's reference point -- split the batch", what);
        return attn_refuse(p);
    }
    // As found: the first-generation dK / dV kernel's LDS is checked for every causal call below the long forms, also where attention3.hip
    // serves the call and that kernel never runs (no table at all, H (N + 31) > 31000: refused although servable).
    const bool dkv1_checked = c.dtype == 0 || (!(gen2 && lng && !win) && (Pn == 0 || !gen2));
    if ((!dq2 && !attn_lds_ok(ldsq, p)) || (dkv1_checked && !attn_lds_ok(ldsk, p))) return attn_refuse(p);
    if (dq2) attn_push(p, ATTN_A2_DQ, lng ? ATTN_FORM_LONG : ATTN_FORM_SHORT, c, nqt * ((H + 7) / 8) * B, 1, 1, 512, a2_dq_lds(N, off, lng));
    else attn_push(p, ATTN_A1_DQ, ATTN_FORM_SHORT, c, nqt, (H + 3) / 4, B, 256, ldsq);
    if (c.dbias && c.ws) attn_push(p, ATTN_DBIAS_REDUCE, ATTN_FORM_SHORT, c, (N + 255) / 256, H, B < 8 ? B : 8, 256, 0);
    if (!dkv3) {
        attn_push(p, ATTN_A1_DKV, ATTN_FORM_SHORT, c, nqt, 1, B, 256, ldsk);
        p.l[p.n - 1].win = win;
        return p;
    }
    const int CH = a3_chunk(B, N), wps = a3_wg_per_sample(N, CH, Pn);
    const bool part = lng && c.ws;                             // slots, then their sums in a fixed order; else zero fill + atomics
    if (part) p.dkv_slots = attn_dbias_rows_floats(B, N, H);
    else for (int which = 0; which < (c.dkv_adjacent ? 1 : 2); ++which) {
        const long long floats = (long long)B * N * 64 * (c.dkv_adjacent ? 2 : 1), blocks = (floats / 4 + 255) / 256;
        attn_push(p, ATTN_A3_ZERO, ATTN_FORM_SHORT, c, (int)(blocks > 8192 ? 8192 : blocks), 1, 1, 256, 0);
        p.l[p.n - 1].which = which; p.l[p.n - 1].floats = floats;
    }
    attn_push(p, ATTN_A3_DKV, part ? ATTN_FORM_PART : ATTN_FORM_SHORT, c, B * wps, 1, 1, 256, A3_LDS);
    p.l[p.n - 1].CH = CH; p.l[p.n - 1].wps = wps;
    if (part) {
        attn_push(p, ATTN_A3_REDUCE, ATTN_FORM_PART, c, (N + A3_KEYS - 1) / A3_KEYS, B, 2, 256, 0);
        p.l[p.n - 1].CH = CH; p.l[p.n - 1].wps = wps;
    }
    return p;
}

}   // namespace omlm_plan

#ifdef OMLM_PLAN_TEST_ABI       /* tests/test_attn_plan_host.py: the plan behind a flat C interface, built by the host c++ */
// call: backward operands copy B N H P bias biasT dbias ws drop dkv_adjacent.
//   copy: 0 / 1 the call as the bf16 / fp16 copy sees it, operands != 0: fp32; 2 a call of the public entry: operands is its dtype code
//   (attn_to_fp16_copy decides; omlm_plan_attn_fp16_copy: whether the fp16 copy serves the call).
// out: rc, n, ldT, dkv_slots, then 16 values per launch: family form precise pfx drop fixed win gx gy gz threads lds CH wps which floats.
// msg: 480 bytes.
static omlm_plan::AttnCall omlm_plan_attn_call(const int* v) {
    omlm_plan::AttnCall c = {v[0] != 0, v[2] == 2 ? v[1] : v[1] ? 0 : 1, v[2] == 1, v[3], v[4], v[5], v[6], v[7] != 0, v[8] != 0, v[9] != 0, v[10] != 0, v[11] != 0, v[12] != 0};
    if (v[2] == 2) c.fp16_copy = omlm_plan::attn_to_fp16_copy(c);
    return c;
}
extern "C" void omlm_plan_attn(const int* v, long long* out, char* msg) {
    const omlm_plan::AttnCall c = omlm_plan_attn_call(v);
    const omlm_plan::AttnPlan p = omlm_plan::attn_plan(c);
    out[0] = p.rc; out[1] = p.n; out[2] = p.ldT; out[3] = p.dkv_slots;
    for (int i = 0; i < p.n; ++i) {
        const omlm_plan::AttnLaunch& l = p.l[i];
        const long long w[16] = {l.family, l.form, l.precise, l.pfx, l.drop, l.fixed, l.win, l.gx, l.gy, l.gz, l.threads, l.lds, l.CH, l.wps, l.which, l.floats};
        memcpy(out + 4 + 16 * i, w, sizeof(w));
    }
    memcpy(msg, p.msg, sizeof(p.msg));
}
extern "C" int omlm_plan_attn_fp16_copy(const int* v) { return omlm_plan_attn_call(v).fp16_copy; }
extern "C" long long omlm_plan_attn_table_floats(int N, int H, int P) { return omlm_plan::attn_bias_table_floats(N, H, P); }
extern "C" long long omlm_plan_attn_workspace_bytes(int B, int N, int H) { return omlm_plan::attn_bwd_workspace_bytes(B, N, H); }
extern "C" int omlm_plan_attn_max_positions(int dtype, int P) { return omlm_plan::attn_max_positions(dtype, P); }
extern "C" int omlm_plan_attn_second_generation(const int* v) { return omlm_plan::attn_second_generation(omlm_plan_attn_call(v)); }
#endif
