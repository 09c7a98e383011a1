// Where the ConvFeedForward middle decides its route: which kernels serve a call of omlm_ffmid_fwd / _fwd_planes / _fwd_mx / _bwd, in which
// order, on which grids, with how much LDS and with which per-launch scalars -- or why the call is refused -- as a pure host function of the
// call.  Every limit, the workspace size and its split are stated here once.  No HIP here: the host c++ compiles this header
// (tests/test_ffmid_plan_host.py checks it against the launches recorded on an MI355X, tests/ffmid_routes.json, and pins engine.py's
// mirrors to it), and ffmid.hip / ffmid2.hip (both copies of each) execute what it returns.
#pragma once
#include <stdio.h>
#include <string.h>

// ---- geometry of the kernels (the kernels of ffmid.hip / ffmid2.hip are written against these) ------------------------------------------------
#define FF_THREADS 256          // wave-per-row kernels (first generation): four rows per workgroup
#define FF_MAXC_LIMIT 16        // ... with at most 16 chunks of 8 channels per lane
#define FF_BWD1_BLOCKS 1024     // workspace rows of d(gamma) partials
#define FF_BWD2_STRIPS 512      // workspace rows of d(conv taps) partials

namespace omlm_plan __attribute__((visibility("hidden"))) {
// (static: the objects that include this header export nothing of it)

constexpr int FF_ERR_ARG = -1;                      // common.h: OMLM_ERR_ARG
constexpr long long FF_LDS_CAP = 160 * 1024;        // per workgroup; a launch above FF_LDS_OPT_IN opts its instantiation in to it
constexpr long long FF_LDS_OPT_IN = 48 * 1024;

// ---- limits ---------------------------------------------------------------------------------------------------------------------------------
constexpr int FF_MAX_FP = 8 * 64 * FF_MAXC_LIMIT;   // 8192: a wave holds a row, and 5 * Fp floats are the 160 KiB of LDS
constexpr int FF_STRIP_MAX_FP = 8 * 512;            // 4096: the column-strip kernels run one thread per chunk of 8 channels, at most 512
constexpr int FF_ONE_PASS_MAX_FP = 4 * 768;         // 3072: the one-pass backward runs one thread per 4 channels, at most 768
constexpr int FF_ROWSUM_MC = 8;                     // chunks per lane of the two-pass backward's row sums: it runs at Fp in 3080..4096, 7 or 8 chunks
static inline bool ffmid_fp_ok(int F, int Fp) { return Fp % 8 == 0 && Fp >= F && Fp >= 0 && Fp <= FF_MAX_FP; }
// the second generation (column strips; both plane forwards know no other)
static inline bool ffmid_strip_ok(int Fp) { return Fp % 8 == 0 && Fp / 8 <= FF_STRIP_MAX_FP / 8; }
static inline bool ffmid_one_pass(int Fp) { return Fp / 4 <= FF_ONE_PASS_MAX_FP / 4; }

// ---- workspace of the backward: [FF_BWD1_BLOCKS][Fp] partial rows of d(gamma), then [FF_BWD2_STRIPS][2F * 3] of d(conv taps) ------------------
static inline long long ffmid_ws_dconv_at(int Fp) { return (long long)FF_BWD1_BLOCKS * Fp; }                   // floats
static inline long long ffmid_bwd_workspace_bytes(int F, int Fp) { return 4 * (ffmid_ws_dconv_at(Fp) + (long long)FF_BWD2_STRIPS * 2 * F * 3); }

// ---- shared arithmetic --------------------------------------------------------------------------------------------------------------------------
// rows of a strip: nseq cut into the fewest strips of at most `target` rows, evenly
static inline int ffmid_strip_rows(int nseq, int target) {
    const int n = (nseq + target - 1) / target;
    return (nseq + n - 1) / n;
}
static inline int ffmid_chunks_per_lane(int Fp) { return (Fp / 8 + 63) / 64; }
static inline int ffmid_maxc(int Fp) { const int mc = ffmid_chunks_per_lane(Fp); return mc <= 2 ? 2 : mc <= 6 ? 6 : mc <= 8 ? 8 : 16; }
static inline long long ffmid_row_lds(int Fp) { return 4ll * Fp * 4; }                // four fp32 rows (fwd1, bwd1, rowsum)
// omlm_colsum_accumulate / omlm_colsum_group: slices of the P partial rows along gridDim.y (enough workgroups to stream a [2048, D] buffer)
static inline int colsum_ysplit(int P) { return P >= 1024 ? 128 : (P >= 64 ? 16 : 1); }

// ---- the call, and what it runs --------------------------------------------------------------------------------------------------------------
enum FfOp { FF_FWD, FF_FWD_PLANES, FF_FWD_MX, FF_BWD };
struct FfmidCall {
    FfOp op;
    int M, nseq, F, Fp;
    int dtype;              // as the copy sees it: 0 fp32, 1 its 16-bit type (ffmid_to_fp16_copy below)
    bool fp16_copy;         // the fp16 copy: it builds no fp32 kernels
    float p;                // dropout: the route depends on p > 0 only; the forwards check the range
    bool operands;          // every pointer the entry requires is there (the lo / fp8 planes and the workspace among them)
    bool drop_bits, gh, dgamma, dconv;      // which of the optional pointers are there
    int n_full, p0;         // row segment (n_full == 0: none)
    long long h2_8_stride;  // fwd_mx
    bool planes_aligned;    // the plane forwards: every plane at a multiple of 16 bytes
    bool du_aligned;        // bwd: du_tmp at a multiple of 8 bytes
    int impl;               // omlm_ffmid_set_impl (tests): 0 keeps every call on the first generation
};
enum FfKernel {
    FK_FWD1, FK_BWD1, FK_BWD2,                                      // ffmid.hip: ffmid_fwd_kernel, ffmid_bwd1_kernel, ffmid_bwd2_kernel
    FK_STRIP_FWD, FK_STRIP_FWD_SEG, FK_ROWSUM, FK_STRIP_BWD, FK_BWD3,       // ffmid2.hip: ffmid2_fwd_kernel, ffmid2_fwd_seg_kernel, ffmid2_rowsum_kernel, ffmid2_bwd_kernel, ffmid3_bwd_kernel
    FK_COLSUM_G, FK_COLSUM_C, FK_COLSUM_GROUP                       // omlm_colsum_accumulate into dgamma / into dconv; omlm_colsum_group into both
};
struct FfmidLaunch {
    FfKernel kernel;
    bool t16;               // T: the 16-bit type of the copy / float
    int n;                  // MAXC (fwd1, bwd1), NT (strip_fwd, strip_fwd_seg, bwd3), MC (rowsum)
    bool train, pl, mx, gh; // TRAIN, PL, MX (strip forwards), GH (bwd1)
    int gx, gy, threads;
    long long lds;
    int RB, strips, total;  // strip kernels: rows per strip, strips per sample, strips of the call
    int g_rows, c_rows;     // column sums: the partial rows of d(gamma) / of d(conv taps) the kernels in front of them left
};
struct FfmidPlan {
    int rc;                 // 0, or the refusal's return code with msg set; nothing is launched then
    char msg[384];
    bool strips;            // the second generation serves the call
    int n;
    FfmidLaunch l[4];
};

// The bf16 copy holds the public entries and hands a call that names fp16 (dtype code 2) to the fp16 copy, which sees its 16-bit type as
// code 1.  The mx forward exists in the fp16 copy only.
static inline bool ffmid_to_fp16_copy(FfmidCall& c) {
    if (c.op != FF_FWD_MX && c.dtype != 2) return false;
    if (c.dtype == 2) c.dtype = 1;
    return true;
}

static inline FfmidPlan& ffmid_refuse(FfmidPlan& p, const char* text) {
    p.rc = FF_ERR_ARG; p.n = 0;
    snprintf(p.msg, sizeof(p.msg), "bad argument: %s", text);
    return p;
}
static inline FfmidLaunch& ffmid_push(FfmidPlan& p, FfKernel k, const FfmidCall& c, int n, int gx, int gy, int threads, long long lds) {
    FfmidLaunch& l = p.l[p.n++];
    memset(&l, 0, sizeof(l));
    l.kernel = k; l.t16 = c.dtype != 0; l.n = n; l.gx = gx; l.gy = gy; l.threads = threads; l.lds = lds;
    return l;
}
// the column sums behind a backward: one grouped launch where both sums are wanted
static inline void ffmid_push_colsums(FfmidPlan& p, const FfmidCall& c, int g_rows, int c_rows) {
    const int cg = c.F, cc = 2 * c.F * 3;
    if (c.dgamma && c.dconv) {
        FfmidLaunch& l = ffmid_push(p, FK_COLSUM_GROUP, c, 0, (cc + 255) / 256, colsum_ysplit(g_rows > c_rows ? g_rows : c_rows), 256, 0);
        l.g_rows = g_rows; l.c_rows = c_rows;
        return;
    }
    if (c.dgamma) ffmid_push(p, FK_COLSUM_G, c, 0, (cg + 255) / 256, colsum_ysplit(g_rows), 256, 0).g_rows = g_rows;
    if (c.dconv) ffmid_push(p, FK_COLSUM_C, c, 0, (cc + 255) / 256, colsum_ysplit(c_rows), 256, 0).c_rows = c_rows;
}

// The refusals carry the texts the entries have always returned: the reason, then in brackets the rule as its check was first written.
#define FF_REFUSE_UNLESS(cond, text) do { if (!(cond)) return ffmid_refuse(p, text); } while (0)

static inline FfmidPlan ffmid_plan(const FfmidCall& c) {
    FfmidPlan p;
    memset(&p, 0, sizeof(p));
    const int M = c.M, nseq = c.nseq, F = c.F, Fp = c.Fp;
    const bool fwd = c.op != FF_BWD, planes = c.op == FF_FWD_PLANES || c.op == FF_FWD_MX;
    const bool keep_ok = c.p == 0.f || c.drop_bits;                 // the strip kernels' mask travels as keep bits
    if (c.op == FF_FWD_PLANES) FF_REFUSE_UNLESS(c.dtype == 1, "ffmid_fwd_planes: dtype 1 (bf16) or 2 (fp16) [dtype == 1]");
    else if (c.op != FF_FWD_MX) FF_REFUSE_UNLESS(!c.fp16_copy || c.dtype == 1, "the fp16 copy serves fp16 operands only [dtype == 1]");
    if (M <= 0) return p;
    if (fwd) FF_REFUSE_UNLESS(c.n_full == 0 || (c.p0 > 0 && c.p0 + nseq == c.n_full),
                              "row segment: nseq must be n_full - p0, p0 > 0 [(n_full) == 0 || ((p0) > 0 && (p0) + (nseq) == (n_full))]");
    FF_REFUSE_UNLESS(c.operands, c.op == FF_FWD ? "null pointer [h1 && convw && gamma && h2 && mean && rstd]" :
                                 c.op == FF_FWD_PLANES ? "null pointer [h1 && h1_lo && convw && convw_lo && gamma && gamma_lo && h2 && h2_lo && mean && rstd]" :
                                 c.op == FF_FWD_MX ? "null pointer [h1 && h1_lo && convw && convw_lo && gamma && gamma_lo && h2 && h2_8 && scale8 && mean && rstd]" :
                                                     "null pointer [dh2 && h1 && convw && gamma && mean && rstd && du_tmp && dh1 && workspace]");
    if (c.op == FF_FWD_PLANES)
        FF_REFUSE_UNLESS(Fp >= F && ffmid_strip_ok(Fp), "ffmid_fwd_planes: Fp must be F rounded up to 8 and <= 4096 [Fp % 8 == 0 && Fp >= F && ffmid2_supported(Fp)]");
    else if (c.op == FF_FWD_MX)
        FF_REFUSE_UNLESS(Fp >= F && ffmid_strip_ok(Fp), "ffmid_fwd_mx: Fp must be F rounded up to 8 and <= 4096 [Fp % 8 == 0 && Fp >= F && ffmid2_supported(Fp)]");
    else
        FF_REFUSE_UNLESS(ffmid_fp_ok(F, Fp), "Fp must be F rounded up to 8 and <= 8192 [Fp % 8 == 0 && Fp >= F && Fp <= 8192 && (size_t)5 * Fp * sizeof(float) <= 160 * 1024]");
    FF_REFUSE_UNLESS(nseq > 0 && M % nseq == 0, "M must be batch * nseq [nseq > 0 && M % nseq == 0]");
    if (planes) FF_REFUSE_UNLESS(c.p >= 0.f && c.p < 1.f && keep_ok, "dropout p (keep bits required when p > 0) [p >= 0.f && p < 1.f && (p == 0.f || drop_bits)]");
    else if (fwd) FF_REFUSE_UNLESS(c.p >= 0.f && c.p < 1.f, "dropout p [p >= 0.f && p < 1.f]");
    if (c.op == FF_FWD_MX) {
        FF_REFUSE_UNLESS(c.h2_8_stride >= (long long)M * 2 * Fp && c.h2_8_stride % 16 == 0,
                         "ffmid_fwd_mx: fp8 plane stride [h2_8_stride >= (long long)M * 2 * Fp && h2_8_stride % 16 == 0]");
        // the kernel zeroes every fp8 row out to a whole 128-byte k-tile: the row pitch 2 Fp must hold it (Fp >= 64)
        FF_REFUSE_UNLESS(2 * Fp >= (Fp + 127) / 128 * 128,
                         "ffmid_fwd_mx: an fp8 plane row (pitch 2 * Fp bytes) must hold Fp rounded up to 128 bytes [2 * Fp >= (Fp + 127) / 128 * 128]");
        FF_REFUSE_UNLESS(c.planes_aligned, "ffmid_fwd_mx: 16-byte aligned planes [(((uintptr_t)h1 | (uintptr_t)h1_lo | (uintptr_t)convw | (uintptr_t)convw_lo | "
                                           "(uintptr_t)gamma | (uintptr_t)gamma_lo | (uintptr_t)h2 | (uintptr_t)h2_8) % 16) == 0]");
    } else if (c.op == FF_FWD_PLANES) {
        FF_REFUSE_UNLESS(c.planes_aligned, "ffmid_fwd_planes: 16-byte aligned planes [(((uintptr_t)h1 | (uintptr_t)h1_lo | (uintptr_t)convw | (uintptr_t)convw_lo | "
                                           "(uintptr_t)gamma | (uintptr_t)gamma_lo | (uintptr_t)h2 | (uintptr_t)h2_lo) % 16) == 0]");
    }
    // the generation: the strip kernels where they hold the row, the mask reaches them as keep bits and -- backward -- gh is there
    p.strips = planes || (c.impl == 1 && ffmid_strip_ok(Fp) && keep_ok && (fwd || c.gh));
    const int B = M / nseq, rows4 = (M + 3) / 4;
    if (fwd && p.strips) {
        // one workgroup per strip of a sample, one thread per chunk (the instantiation: whole waves).  A segment changes nothing but the
        // keep bits drawn: without dropout the plain kernel serves it
        const int RB = ffmid_strip_rows(nseq, 36), strips = (nseq + RB - 1) / RB, nt = ffmid_chunks_per_lane(Fp) * 64;
        const bool segd = c.n_full > 0 && c.p > 0.f;
        FfmidLaunch& l = ffmid_push(p, segd ? FK_STRIP_FWD_SEG : FK_STRIP_FWD, c, nt >= 64 && nt < 512 ? nt : 512, B * strips, 1, Fp / 8, 0);
        l.train = c.p > 0.f && c.drop_bits && c.gh;         // the training call: all three row stores are unconditional
        l.pl = planes; l.mx = c.op == FF_FWD_MX; l.RB = RB; l.strips = strips;
        return p;
    }
    if (fwd) {
        // (the wave-per-row kernels know no segment: their mask is a function of the compact row -- still one mask for forward and backward)
        ffmid_push(p, FK_FWD1, c, ffmid_maxc(Fp), rows4 < 4096 ? rows4 : 4096, 1, FF_THREADS, ffmid_row_lds(Fp));
        return p;
    }
    if (!p.strips) {
        const int b1 = rows4 < FF_BWD1_BLOCKS ? rows4 : FF_BWD1_BLOCKS, strips = M < FF_BWD2_STRIPS ? M : FF_BWD2_STRIPS;
        ffmid_push(p, FK_BWD1, c, ffmid_maxc(Fp), b1, 1, FF_THREADS, ffmid_row_lds(Fp)).gh = c.gh;
        ffmid_push(p, FK_BWD2, c, 0, (2 * Fp / 8 + FF_THREADS - 1) / FF_THREADS, strips, FF_THREADS, 0);
        ffmid_push_colsums(p, c, b1, strips);
        return p;
    }
    // du_tmp is not needed by the fused kernels: its first M * 2 floats carry the per-row LayerNorm^T sums of the two-pass form
    FF_REFUSE_UNLESS(c.du_aligned, "du_tmp must be 8-byte aligned [((uintptr_t)du_tmp % 8) == 0]");
    const int RB = ffmid_strip_rows(nseq, 35), strips = (nseq + RB - 1) / RB, total = B * strips;
    const int per = (total + 255) / 256;                    // strips per workgroup: about one workgroup (row of workgroups) per CU
    int ny = (total + per - 1) / per, g_rows;
    if (ny > FF_BWD2_STRIPS) ny = FF_BWD2_STRIPS;
    if (ffmid_one_pass(Fp)) {
        // a workgroup covers all channels of its rows and leaves both partial rows
        const int nthr = (Fp / 4 + 63) / 64 * 64, nt = nthr <= 128 ? 128 : nthr <= 256 ? 256 : nthr <= 512 ? 512 : 768;
        FfmidLaunch& l = ffmid_push(p, FK_BWD3, c, nt, 1, ny, nt, 0);
        l.RB = RB; l.strips = strips; l.total = total;
        g_rows = ny;
    } else {
        g_rows = rows4 < FF_BWD1_BLOCKS ? rows4 : FF_BWD1_BLOCKS;
        ffmid_push(p, FK_ROWSUM, c, FF_ROWSUM_MC, g_rows, 1, 256, ffmid_row_lds(Fp));
        FfmidLaunch& l = ffmid_push(p, FK_STRIP_BWD, c, 0, (Fp / 4 + 255) / 256, ny, 256, 0);
        l.RB = RB; l.strips = strips; l.total = total;
    }
    ffmid_push_colsums(p, c, g_rows, ny);
    return p;
}
#undef FF_REFUSE_UNLESS

// ---- what the launchers of ffmid.hip / ffmid2.hip take next to a launch of the plan: the entry's pointers and scalars, filled once -------------
struct FfmidArgs {
    const void *h1, *convw, *gamma, *h1_lo, *convw_lo, *gamma_lo;      // (*_lo: the plane forwards; fwd_mx: h1_lo holds bf8 bytes)
    void *h2, *h2_lo, *h2_8;
    unsigned char* scale8;
    float *mean, *rstd;
    const void* dh2;
    void *du_tmp, *dh1;
    float *dgamma, *dconv, *workspace;
    int M, nseq, F, Fp;
    float eps, p;
    unsigned long long seed;
    const unsigned long long* seed_dev;
    unsigned char* drop_bits;
    void* gh;
    int n_full, p0;
    long long h2_8_stride;
    void* stream;
};

}   // namespace omlm_plan

#ifdef OMLM_PLAN_TEST_ABI       /* tests/test_ffmid_plan_host.py: the plan behind a flat C interface, built by the host c++ */
// call: op M nseq F Fp dtype copy operands drop_bits gh dgamma dconv n_full p0 planes_aligned du_aligned impl; p and h2_8_stride apart.
//   copy: 0 / 1 the call as the bf16 / fp16 copy sees it; 2 a call of the public entry (ffmid_to_fp16_copy decides).
// out: rc strips n, then 16 values per launch: kernel t16 n train pl mx gh gx gy threads lds RB strips total g_rows c_rows.  msg: 384 bytes.
// omlm_plan_ffmid_fp16_copy: whether the fp16 copy serves the call.
static omlm_plan::FfmidCall omlm_plan_ffmid_call(const int* v, double p, long long h2_8_stride) {
    omlm_plan::FfmidCall c = {(omlm_plan::FfOp)v[0], v[1], v[2], v[3], v[4], v[5], v[6] == 1, (float)p, v[7] != 0, v[8] != 0, v[9] != 0, v[10] != 0,
                              v[11] != 0, v[12], v[13], h2_8_stride, v[14] != 0, v[15] != 0, v[16]};
    if (v[6] == 2) c.fp16_copy = omlm_plan::ffmid_to_fp16_copy(c);
    return c;
}
extern "C" int omlm_plan_ffmid_fp16_copy(const int* v) { return omlm_plan_ffmid_call(v, 0, 0).fp16_copy; }
extern "C" void omlm_plan_ffmid(const int* v, double p, long long h2_8_stride, long long* out, char* msg) {
    const omlm_plan::FfmidPlan q = omlm_plan::ffmid_plan(omlm_plan_ffmid_call(v, p, h2_8_stride));
    out[0] = q.rc; out[1] = q.strips; out[2] = q.n;
    for (int i = 0; i < q.n; ++i) {
        const omlm_plan::FfmidLaunch& l = q.l[i];
        const long long w[16] = {l.kernel, l.t16, l.n, l.train, l.pl, l.mx, l.gh, l.gx, l.gy, l.threads, l.lds, l.RB, l.strips, l.total, l.g_rows, l.c_rows};
        memcpy(out + 3 + 16 * i, w, sizeof(w));
    }
    memcpy(msg, q.msg, sizeof(q.msg));
}
// limits: FF_MAX_FP FF_STRIP_MAX_FP FF_ONE_PASS_MAX_FP FF_BWD1_BLOCKS FF_BWD2_STRIPS
extern "C" void omlm_plan_ffmid_limits(int* out) {
    const int v[5] = {omlm_plan::FF_MAX_FP, omlm_plan::FF_STRIP_MAX_FP, omlm_plan::FF_ONE_PASS_MAX_FP, FF_BWD1_BLOCKS, FF_BWD2_STRIPS};
    memcpy(out, v, sizeof(v));
}
extern "C" int omlm_plan_ffmid_fp_ok(int F, int Fp) { return omlm_plan::ffmid_fp_ok(F, Fp); }
extern "C" int omlm_plan_ffmid_strip_ok(int Fp) { return omlm_plan::ffmid_strip_ok(Fp); }
extern "C" int omlm_plan_ffmid_one_pass(int Fp) { return omlm_plan::ffmid_one_pass(Fp); }
extern "C" long long omlm_plan_ffmid_bwd_workspace_bytes(int F, int Fp) { return omlm_plan::ffmid_bwd_workspace_bytes(F, Fp); }
extern "C" long long omlm_plan_ffmid_ws_dconv_at(int Fp) { return omlm_plan::ffmid_ws_dconv_at(Fp); }
#endif
