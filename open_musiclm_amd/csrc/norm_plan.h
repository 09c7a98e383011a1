// Where the LayerNorm and q/k-norm entries decide their route: which kernel instantiation serves a call of omlm_layernorm_fwd / _fwd_planes /
// _fwd_mx / _bwd2 (plain and `_seg`) or omlm_qk_norm_fwd / _bwd / _bwd2, on which grid, with which column sum behind it -- or why the call is
// refused -- as a pure host function of the call.  Every limit, grid cap and the workspace size are stated here once.  No HIP here: the host
// c++ compiles this header (tests/test_norm_plan_host.py checks it against the launches recorded on an MI355X, tests/norm_routes.json, and
// pins ops.py's / engine.py's mirrors to it), and norm.hip (both copies) executes what it returns.
#pragma once
#include <stdio.h>
#include <string.h>
#include "ffmid_plan.h"         // colsum_ysplit: the column sum behind a LayerNorm backward is the middle's

// ---- geometry of the kernels (the kernels of norm.hip are written against these) --------------------------------------------------------------
#define LN_THREADS 256
#define LN_MAXV 4               // float4 pieces per thread  -> D <= 4096
#define QKB_BLOCKS 512          // qk_norm_bwd_kernel: each workgroup ends with 128 atomics into the two scale gradients (2048 workgroups: 69 us, 512: 51 us)
#define QKB2_THREADS 1024       // qk_norm_bwd2_kernel, 16 waves per workgroup: a quarter of the atomics of 256-thread workgroups at the same waves per CU
                                // (1024 workgroups x 128 atomics onto 128 addresses were ~10 us of serialised tail)
#define QKB2_BLOCKS 256         // ... and at most so many workgroups (128 atomics per workgroup at the end)

namespace omlm_plan __attribute__((visibility("hidden"))) {
// (static: the objects that include this header export nothing of it)

constexpr int NORM_ERR_ARG = -1;                    // common.h: OMLM_ERR_ARG

// ---- limits and grids ----------------------------------------------------------------------------------------------------------------------
constexpr int LN_MAX_D = 4 * LN_THREADS * LN_MAXV;  // 4096: a thread holds LN_MAXV float4 pieces of a row
constexpr int LN_ROW1_D = 4 * LN_THREADS;           // 1024: the row-pair kernels hold a row as ONE float4 per thread (next-row prefetch, fewer barriers)
// Each row is a dependent chain (load -> two block reductions -> load dres -> store), so the rate is set by the rows in flight: 2048 workgroups,
// a row each.  The backward leaves one partial dgamma row per workgroup in its workspace for the column sum; without a workspace dgamma is
// accumulated with atomics, which only scale to 512 workgroups (2048: 194 -> 273 us).
constexpr int LN_GRID = 2048;
constexpr int LN_GRID_ATOMICS = 512;
constexpr int QK_THREADS = 256;                     // qk_norm_fwd_kernel / qk_norm_bwd_kernel: four waves, four 64-wide vectors per wave and trip
constexpr int QK_VECS = 16;                         // ... so 16 vectors per workgroup and trip
constexpr int QK_FWD_BLOCKS = 4096;

static inline bool ln_d_ok(int D) { return D % 4 == 0 && D <= LN_MAX_D; }
#define LN_D_TEXT "D must be a multiple of 4 and <= 4096 [D % 4 == 0 && D <= 4 * LN_THREADS * LN_MAXV]"
static inline int ln_grid(int M, int cap) { return M < cap ? M : cap; }
// the partial rows a two-level backward leaves (one per workgroup): what the column sum behind it -- the call's own, or the caller's grouped one -- reads
static inline int ln_bwd_partial_rows(int M) { return ln_grid(M, LN_GRID); }
static inline long long ln_bwd_workspace_bytes(int D) { return (long long)LN_GRID * D * 4; }
// A row segment (include/omlm.h, "Row segments"): rows [p0, n_full) of every sample, compact.
static inline bool ln_seg_ok(int M, int n_full, int p0, int n_live) { return p0 > 0 && n_live > 0 && p0 + n_live == n_full && M % n_live == 0; }
#define LN_SEG_TEXT "row segment: n_full = p0 + n_live, p0 > 0, M a multiple of n_live [(p0) > 0 && (n_live) > 0 && (p0) + (n_live) == (n_full) && (M) % (n_live) == 0]"
// the kernels index 64-wide vectors with 32 bits
static inline bool qk_vectors_ok(long long nvec) { return nvec < (1ll << 31); }

// ---- the call, and what it runs --------------------------------------------------------------------------------------------------------------
// LN_FWD, LN_FWD_PLANES and LN_BWD stand for the plain entry and its `_seg` twin: n_full == 0 is "no segment", which is all the plain entries
// pass.  omlm_layernorm_fwd_mx_seg always carries a segment (n_full == 0 is refused there): an op of its own.
enum NormOp { LN_FWD, LN_FWD_PLANES, LN_FWD_MX, LN_FWD_MX_SEG, LN_BWD, QK_FWD, QK_BWD, QK_BWD2 };
struct NormCall {
    NormOp op;
    int M, D, ldy, H;
    int dtype;              // out_dtype / cast_dtype / dtype as the copy sees it: 0 fp32, 1 its 16-bit type (norm_to_fp16_copy below)
    int dy_dtype;           // LN_BWD
    bool fp16_copy;         // the fp16 copy: it builds no fp32 kernels
    bool operands;          // every pointer the entry requires is there
    bool xcast, stats, xc;  // forward: cast copy of x, mean AND rstd, the compact fp32 source rows of a segment (no route depends on xc)
    bool dres, dres2, dxcast, dgamma, workspace;        // backward
    int n_full, p0, n_live; // row segment
    long long y8_stride;    // fwd_mx
};
enum NormKernel {
    NK_LN_FWD, NK_LN_FWD_ROW1, NK_LN_FWD_MX, NK_LN_BWD, NK_LN_BWD_ROW1,        // ln_fwd_kernel, ln_fwd_row1_kernel, ln_fwd_mx_kernel, ln_bwd_kernel, ln_bwd_row1_kernel
    NK_QK_FWD, NK_QK_BWD, NK_QK_BWD2,                                          // qk_norm_fwd_kernel, qk_norm_bwd_kernel, qk_norm_bwd2_kernel
    NK_COLSUM                                                                  // omlm_colsum_accumulate over the partial rows, into dgamma
};
struct NormLaunch {
    NormKernel kernel;
    bool t16, tdy16;        // T, TDY: the 16-bit type of the copy / float
    bool xc, lo, seg;       // XC (row-pair forward), LO (forwards: the second output is y's lo plane), SEG
    int fl;                 // FL (row-pair backward): bit 0 = dres, bit 1 = dres2, bit 2 = dxcast present
    int maxv;               // MAXV (mx forward)
    int gx, gy, threads;
    int rows;               // column sum: the partial rows the kernel in front of it left
};
struct NormPlan {
    int rc;                 // 0, or the refusal's return code with msg set; nothing is launched then
    char msg[384];
    const char* label;      // what a failed launch of the call's own kernel is reported under
    int n;
    NormLaunch l[2];
};

// The bf16 copy holds the public entries and hands a call that names fp16 (dtype code 2) to the fp16 copy, which sees its 16-bit type as
// code 1.  (A backward with one fp16 and one bf16 code goes there too and is run as fp16: the entries have always taken it.)  The mx forward
// exists in the fp16 copy only.
static inline bool norm_to_fp16_copy(NormCall& c) {
    const bool mx = c.op == LN_FWD_MX || c.op == LN_FWD_MX_SEG;
    if (!mx && c.dtype != 2 && !(c.op == LN_BWD && c.dy_dtype == 2)) return false;
    if (c.dtype == 2) c.dtype = 1;
    if (c.dy_dtype == 2) c.dy_dtype = 1;
    return true;
}

static inline NormPlan& norm_refuse(NormPlan& p, const char* text) {
    p.rc = NORM_ERR_ARG; p.n = 0;
    snprintf(p.msg, sizeof(p.msg), "bad argument: %s", text);
    return p;
}
static inline NormLaunch& norm_push(NormPlan& p, NormKernel k, int gx, int gy, int threads) {
    NormLaunch& l = p.l[p.n++];
    memset(&l, 0, sizeof(l));
    l.kernel = k; l.gx = gx; l.gy = gy; l.threads = threads;
    return l;
}

// The refusals carry the texts the entries have always returned: the reason, then in brackets the rule as its check was first written.
#define NORM_REFUSE_UNLESS(cond, text) do { if (!(cond)) return norm_refuse(p, text); } while (0)
// (not reachable through the C entries: the bf16 copy hands over fp16 calls only, as code 1)
#define NORM_FP16_COPY_TEXT "the fp16 copy serves fp16 operands only [dtype == 1]"

// omlm_layernorm_fwd / _fwd_planes / _fwd_mx and their `_seg` twins
static inline NormPlan& ln_fwd_plan(const NormCall& c, NormPlan& p) {
    const bool planes = c.op == LN_FWD_PLANES, mx = c.op == LN_FWD_MX || c.op == LN_FWD_MX_SEG, plain = !planes && !mx;
    const bool seg = mx ? c.op == LN_FWD_MX_SEG : c.n_full != 0;
    // a failed launch of the mx `_seg` entry is reported under the plain entry's name (the two share their runner)
    p.label = mx ? "omlm_layernorm_fwd_mx" : planes ? (seg ? "omlm_layernorm_fwd_planes_seg" : "omlm_layernorm_fwd_planes")
                                                    : (seg ? "omlm_layernorm_fwd_seg" : "omlm_layernorm_fwd");
    if (plain) NORM_REFUSE_UNLESS(!c.fp16_copy || c.dtype == 1, NORM_FP16_COPY_TEXT);
    if (mx) NORM_REFUSE_UNLESS(c.fp16_copy, "the mx forward exists in the fp16 copy only [fp16_copy]");       // (norm_to_fp16_copy sends every such call there)
    if (c.M <= 0) return p;
    if (c.op == LN_FWD_MX_SEG) NORM_REFUSE_UNLESS(ln_seg_ok(c.M, c.n_full, c.p0, c.n_live), LN_SEG_TEXT);
    if (planes) NORM_REFUSE_UNLESS(c.dtype == 1, "layernorm_fwd_planes: out_dtype 1 (bf16) or 2 (fp16) [out_dtype == 1]");
    NORM_REFUSE_UNLESS(c.operands, plain ? "null pointer [x && gamma && y]" : planes ? "null pointer [x && gamma && y && y_lo && mean && rstd]"
                                                                                       : "null pointer [x && gamma && y && y8 && scale8 && mean && rstd]");
    NORM_REFUSE_UNLESS(ln_d_ok(c.D), LN_D_TEXT);
    if (mx) {
        // fp8 plane rows have the pitch of the half plane in bytes (2 ldy), the lo8 plane y8_stride bytes behind the hi8 plane
        NORM_REFUSE_UNLESS(c.ldy >= c.D && c.ldy % 4 == 0 && c.y8_stride >= (long long)c.M * 2 * c.ldy,
                           "ldy / plane stride [ldy >= D && ldy % 4 == 0 && y8_stride >= (long long)M * 2 * ldy]");
        // the kernel zeroes every fp8 row out to a whole 128-byte k-tile: the row pitch must hold it (else the tail runs into the next row)
        NORM_REFUSE_UNLESS(2 * c.ldy >= (c.D + 127) / 128 * 128,
                           "an fp8 plane row (pitch 2 * ldy bytes) must hold D rounded up to 128 bytes [2 * ldy >= (D + 127) / 128 * 128]");
    } else if (planes) {
        NORM_REFUSE_UNLESS(c.ldy >= c.D && c.ldy % 4 == 0, "ldy < D [ldy >= D && ldy % 4 == 0]");
    } else {
        NORM_REFUSE_UNLESS(c.ldy >= c.D, "ldy < D [ldy >= D]");
    }
    if (seg && !mx) NORM_REFUSE_UNLESS(ln_seg_ok(c.M, c.n_full, c.p0, c.n_live), LN_SEG_TEXT);
    if (seg && plain)
        NORM_REFUSE_UNLESS(c.stats && !c.xcast && c.dtype == 1,
                           "layernorm_fwd_seg: statistics wanted, no cast copy of x, 16-bit output [mean && rstd && !xcast && out_dtype == 1]");
    const int grid = ln_grid(c.M, LN_GRID);
    if (mx) {
        NormLaunch& l = norm_push(p, NK_LN_FWD_MX, grid, 1, LN_THREADS);
        l.t16 = true; l.maxv = c.D <= LN_ROW1_D ? 1 : LN_MAXV; l.seg = seg;
        return p;
    }
    // the row-pair kernel stores the statistics unconditionally: the plain forward takes it only with both there (the others require them)
    const bool row1 = c.D == LN_ROW1_D && c.stats;
    NormLaunch& l = norm_push(p, row1 ? NK_LN_FWD_ROW1 : NK_LN_FWD, grid, 1, LN_THREADS);
    l.t16 = !plain || c.dtype != 0;         // (any other code than 0 is taken as the 16-bit type)
    l.xc = row1 && plain && c.xcast;
    l.lo = planes; l.seg = seg;
    return p;
}

// omlm_layernorm_bwd2 / _seg.  With a workspace (ln_bwd_workspace_bytes) every workgroup leaves one partial dgamma row and the column sum
// follows; dgamma null WITH a workspace: the partial rows are left there ([ln_bwd_partial_rows(M), D]) and the caller sums them later --
// engine.trunk_backward folds the column sums of all LayerNorms of a backward pass into one omlm_colsum_group launch.
static inline NormPlan& ln_bwd_plan(const NormCall& c, NormPlan& p) {
    const bool seg = c.n_full != 0;
    p.label = "omlm_layernorm_bwd2";        // (the `_seg` entry too)
    NORM_REFUSE_UNLESS(!c.fp16_copy || c.dtype != 0 || c.dy_dtype != 0, NORM_FP16_COPY_TEXT);
    if (c.M <= 0) return p;
    NORM_REFUSE_UNLESS(c.operands, "null pointer [dy && x && gamma && mean && rstd && dx]");
    NORM_REFUSE_UNLESS(ln_d_ok(c.D), LN_D_TEXT);
    NORM_REFUSE_UNLESS(c.dy_dtype == 0 || c.dy_dtype == 1,
                       "dy_dtype: 0 = fp32, 1 = bf16, 2 = fp16 (same 16-bit type as the cast output) [dy_dtype == 0 || dy_dtype == 1]");
    if (seg) {
        NORM_REFUSE_UNLESS(ln_seg_ok(c.M, c.n_full, c.p0, c.n_live), LN_SEG_TEXT);
        // the one form the trunk uses: 16-bit dy and cast copy (the type is named by cast_dtype even where dxcast is null)
        NORM_REFUSE_UNLESS(!c.dres2 && c.dtype == 1 && c.dy_dtype == 1,
                           "layernorm_bwd2_seg: 16-bit dy and cast type, no dres2 [!dres2 && cast_dtype == 1 && dy_dtype == 1]");
    }
    const int blocks = c.workspace ? ln_bwd_partial_rows(c.M) : ln_grid(c.M, LN_GRID_ATOMICS);
    const bool row1 = c.D == LN_ROW1_D;
    NormLaunch& l = norm_push(p, row1 ? NK_LN_BWD_ROW1 : NK_LN_BWD, blocks, 1, LN_THREADS);
    l.t16 = c.dtype != 0;                   // (any other cast_dtype than 0 is taken as the 16-bit type)
    l.tdy16 = c.dy_dtype != 0; l.seg = seg;
    if (row1) l.fl = (c.dres ? 1 : 0) | (c.dres2 ? 2 : 0) | (c.dxcast ? 4 : 0);
    if (c.workspace && c.dgamma) norm_push(p, NK_COLSUM, (c.D + 255) / 256, colsum_ysplit(blocks), 256).rows = blocks;
    return p;
}

// omlm_qk_norm_fwd / _bwd / _bwd2: M rows of H q vectors, one k and one v vector, 64 wide
static inline NormPlan& qk_plan(const NormCall& c, NormPlan& p) {
    p.label = c.op == QK_FWD ? "omlm_qk_norm_fwd" : c.op == QK_BWD ? "omlm_qk_norm_bwd" : "omlm_qk_norm_bwd2";
    if (c.op != QK_BWD2) NORM_REFUSE_UNLESS(!c.fp16_copy || c.dtype == 1, NORM_FP16_COPY_TEXT);
    if (c.M <= 0) return p;
    if (c.op == QK_BWD2) NORM_REFUSE_UNLESS(c.dtype == 1, "qk_norm_bwd2: 16-bit operand types only (1 = bf16, 2 = fp16) [dtype == 1]");
    NORM_REFUSE_UNLESS(c.operands, c.op == QK_FWD ? "null pointer [q_raw && kv_raw && q_scale && k_scale && q && k && v]" :
                                   c.op == QK_BWD ? "null pointer [dq && dk && dv && q_raw && kv_raw && dq_raw && dkv_raw && dq_scale && dk_scale]" :
                                                    "null pointer [dq && dk && dv && q && k && qn && kn && dq_raw && dkv_raw && dq_scale && dk_scale]");
    const long long nvec = (long long)c.M * (c.H + 2), trips = (nvec + QK_VECS - 1) / QK_VECS;
    if (c.op == QK_FWD) {                   // (64-bit vector index: no limit)
        norm_push(p, NK_QK_FWD, (int)(trips < QK_FWD_BLOCKS ? trips : QK_FWD_BLOCKS), 1, QK_THREADS).t16 = c.dtype != 0;
        return p;
    }
    if (c.op == QK_BWD) {
        NORM_REFUSE_UNLESS(qk_vectors_ok(nvec), "qk_norm_bwd: M * (H + 2) must stay below 2^31 (32-bit vector index) [nvec < (1ll << 31)]");
        norm_push(p, NK_QK_BWD, (int)(trips < QKB_BLOCKS ? trips : QKB_BLOCKS), 1, QK_THREADS).t16 = c.dtype != 0;
        return p;
    }
    NORM_REFUSE_UNLESS(qk_vectors_ok(nvec), "qk_norm_bwd2: M * (H + 2) must stay below 2^31 (32-bit vector index) [nvec < (1ll << 31)]");
    // units of 8 q vectors, ~2 units per wave at least
    const int waves = QKB2_THREADS / 64;
    const long long want = ((long long)c.M * c.H / 8 + 2 * waves - 1) / (2 * waves);
    norm_push(p, NK_QK_BWD2, want > QKB2_BLOCKS ? QKB2_BLOCKS : (want < 1 ? 1 : (int)want), 1, QKB2_THREADS).t16 = true;
    return p;
}
#undef NORM_REFUSE_UNLESS

static inline NormPlan norm_plan(const NormCall& c) {
    NormPlan p;
    memset(&p, 0, sizeof(p));
    switch (c.op) {
    case LN_FWD: case LN_FWD_PLANES: case LN_FWD_MX: case LN_FWD_MX_SEG: return ln_fwd_plan(c, p);
    case LN_BWD: return ln_bwd_plan(c, p);
    default: return qk_plan(c, p);
    }
}

// the fp32-only instantiations: the ones the fp16 copy does not build, and norm_plan never names with fp16_copy set
static inline bool norm_fp32_only(const NormLaunch& l) {
    switch (l.kernel) {
    case NK_LN_FWD: case NK_LN_FWD_ROW1: case NK_QK_FWD: case NK_QK_BWD: return !l.t16;
    case NK_LN_BWD: case NK_LN_BWD_ROW1: return !l.t16 && !l.tdy16;
    default: return false;
    }
}

// ---- what the launchers of norm.hip take next to a launch of the plan: the entry's pointers and scalars, filled once ---------------------------
struct NormArgs {
    // LayerNorm.  y2: the forward's second output -- the cast copy of x, or y's lo plane
    const float *x, *gamma;
    void *y, *y2, *y8;
    unsigned char* scale8;
    float *mean, *rstd, *xc;
    const void *dy, *dres2;
    const float* dres;
    float* dx;
    void* dxcast;
    float *dgamma, *workspace;
    int M, D, ldy;
    float eps, dx_scale;
    int n_full, p0, n_live;
    long long y8_stride;
    // q/k-norm.  q, k: the forward's outputs with v, the inputs of bwd2
    const float *dq, *dk, *dv, *q_raw, *kv_raw, *q_scale, *k_scale, *qn, *kn;
    void *q, *k, *v, *dq_raw, *dkv_raw;
    float *dq_scale, *dk_scale;
    int H;
    void* stream;
};

}   // namespace omlm_plan

#ifdef OMLM_PLAN_TEST_ABI       /* tests/test_norm_plan_host.py: the plan behind a flat C interface, built by the host c++ */
// call: op M D ldy H dtype dy_dtype copy operands xcast stats xc dres dres2 dxcast dgamma workspace n_full p0 n_live; y8_stride apart.
//   copy: 0 / 1 the call as the bf16 / fp16 copy sees it; 2 a call of the public entry (norm_to_fp16_copy decides).
// out: rc n fp16_copy, then 12 values per launch: kernel t16 tdy16 xc lo seg fl maxv gx gy threads rows, and whether the launch is one of the
// fp32-only instantiations.  msg: 384 bytes, label: 64.
extern "C" void omlm_plan_norm(const int* v, long long y8_stride, long long* out, char* msg, char* label) {
    omlm_plan::NormCall c = {(omlm_plan::NormOp)v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7] == 1, v[8] != 0, v[9] != 0, v[10] != 0, v[11] != 0,
                             v[12] != 0, v[13] != 0, v[14] != 0, v[15] != 0, v[16] != 0, v[17], v[18], v[19], y8_stride};
    if (v[7] == 2) c.fp16_copy = omlm_plan::norm_to_fp16_copy(c);
    const omlm_plan::NormPlan q = omlm_plan::norm_plan(c);
    out[0] = q.rc; out[1] = q.n; out[2] = c.fp16_copy;
    for (int i = 0; i < q.n; ++i) {
        const omlm_plan::NormLaunch& l = q.l[i];
        const long long w[13] = {l.kernel, l.t16, l.tdy16, l.xc, l.lo, l.seg, l.fl, l.maxv, l.gx, l.gy, l.threads, l.rows, omlm_plan::norm_fp32_only(l)};
        memcpy(out + 3 + 13 * i, w, sizeof(w));
    }
    memcpy(msg, q.msg, sizeof(q.msg));
    snprintf(label, 64, "%s", q.label);
}
// limits: LN_MAX_D LN_ROW1_D LN_GRID LN_GRID_ATOMICS QK_FWD_BLOCKS QKB_BLOCKS QKB2_BLOCKS QKB2_THREADS LN_THREADS
extern "C" void omlm_plan_norm_limits(int* out) {
    const int v[9] = {omlm_plan::LN_MAX_D, omlm_plan::LN_ROW1_D, omlm_plan::LN_GRID, omlm_plan::LN_GRID_ATOMICS, omlm_plan::QK_FWD_BLOCKS, QKB_BLOCKS,
                      QKB2_BLOCKS, QKB2_THREADS, LN_THREADS};
    memcpy(out, v, sizeof(v));
}
extern "C" long long omlm_plan_ln_bwd_workspace_bytes(int D) { return omlm_plan::ln_bwd_workspace_bytes(D); }
extern "C" int omlm_plan_ln_bwd_partial_rows(int M) { return omlm_plan::ln_bwd_partial_rows(M); }
#endif
