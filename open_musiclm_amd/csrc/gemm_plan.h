// Where the GEMM family decides its routes: which kernel form runs, on which tile, with how many K-splits and which peeled tail, as pure host
// functions of the shape, the CU count and the test hooks.  No HIP here: the host c++ compiles this header (tests/test_gemm_plan_host.py checks it
// against the launches recorded on an MI355X, tests/gemm_routes.json), and both copies of gemm.hip and gemm_mx.hip execute what it returns.
#pragma once
#include <stdlib.h>
#include <string.h>

#define OMLM_GEMM_T8_DEFAULT 2     // round 5: gemm_tile8_body for the 256 x 256 tiles (see GemmHooks::ring): 2 = where it measured faster

namespace omlm_plan __attribute__((visibility("hidden"))) {

constexpr int KT = 64;             // k-tile depth (gemm_common.h: BK)

// The five test hooks, read per library call (tests and tools/lib_ab toggle them inside one process); gemm_hooks_from_env is their only reader.
struct GemmHooks {
    bool persist;        // OMLM_GEMM_PERSIST=0 keeps the one-tile grid
    // OMLM_GEMM_T8: the half-tile-ring schedule (gemm_tile8_body) for the 256 x 256 tiles: 0 = off, 1 = every eligible launch, 2 (default) =
    // where it measured faster (profiles/r05b_gemm_t8_ab.md, same box, bit-identical results): the grouped weight gradients (557 k-tiles per
    // tile: +6 %) and multi-round launches with K >= 2048 (d(xn2), K = 5504: +3 %; FF-out, K = 2752: +2 %; 8192^3: +15 %).  Short contractions
    // (K = 1024: 16 k-tiles per tile) stay on the persistent walk of the rotated loop, which hides the per-tile prologue / epilogue that this
    // one-tile-per-workgroup form exposes (FF-in 373 vs 399 us).
    int ring;
    bool tile_set;       // OMLM_GEMM_TILE non-empty: no tail peel, whatever it names
    int force_bm, force_bn;      // "256x256" / "256x128": that tile; anything else forces nothing (0, 0)
    bool tail_split;     // OMLM_GEMM_TAIL_SPLIT=0 keeps the one-launch tail
    bool mx_fuse_tail;   // OMLM_MX_FUSE_TAIL=0: always two launches
};
inline GemmHooks gemm_hooks_from_env() {
    auto off = [](const char* name) { const char* e = getenv(name); return e && e[0] == '0'; };
    GemmHooks h;
    h.persist = !off("OMLM_GEMM_PERSIST");
    const char* t8 = getenv("OMLM_GEMM_T8");
    h.ring = t8 ? atoi(t8) : OMLM_GEMM_T8_DEFAULT;
    const char* force = getenv("OMLM_GEMM_TILE");
    h.tile_set = force && force[0];
    h.force_bm = h.force_bn = 0;
    if (h.tile_set && !strcmp(force, "256x256")) { h.force_bm = 256; h.force_bn = 256; }
    else if (h.tile_set && !strcmp(force, "256x128")) { h.force_bm = 256; h.force_bn = 128; }
    h.tail_split = !off("OMLM_GEMM_TAIL_SPLIT");
    h.mx_fuse_tail = !off("OMLM_MX_FUSE_TAIL");
    return h;
}

// what the decisions of omlm_gemm / omlm_gemm_planes / omlm_gemm_planes16 depend on
struct GemmShape {
    int M, N, K;
    bool a_kmajor, b_kmajor;
    bool a_map, b_map, c_map;    // which row maps are present
    int in_dtype, out_dtype;     // 0 = fp32, 1 = the copy's 16-bit type
    bool split3;                 // three products on hi/lo planes (3 x the k-tiles)
    bool planes16;               // the omlm_gemm_planes16 route (launch_tile_s3 of old): built in both copies
    bool fp16_copy;              // the fp16 copy of gemm.hip: no three-product instantiations outside the planes16 route
    bool accumulates;            // Cin == C
    bool cin;                    // any Cin (Cin == C, or a separate residual)
    bool alpha_one;
    long long ws_bytes;          // tail workspace (0: none)
};

// The bf16 copy of gemm.hip holds the public entries and hands a call whose operands are fp16 (code 2) to the fp16 copy, which sees its
// 16-bit type as code 1 -- as output type too.  (omlm_gemm_qknorm, omlm_gemm_planes16 and omlm_gemm_wgrad_group name one type: `dtype`.)
inline bool gemm_to_fp16_copy(int& in_dtype, int& out_dtype) {
    if (in_dtype != 2) return false;
    in_dtype = 1;
    if (out_dtype == 2) out_dtype = 1;
    return true;
}

// k-loop forms
enum GemmForm { FORM_FP32_STAGED, FORM_ROT_GENERAL, FORM_ROT_FASTK, FORM_ROT_KMAP, FORM_ROT_SPLIT3, FORM_PERSIST, FORM_RING };

struct GemmLaunch {               // one kernel launch over rows M of the shape
    int M, bm, bn;
    GemmForm form;
    int splits, kt_per_split;
    int grid_x, grid_y, threads, lds;
    bool kmap_unbuilt;            // a k-row map on a tile other than 128 x 128: an error of the call
};
struct GemmPlan {
    GemmLaunch main;              // the whole problem, or rows [0, M1) of a peeled one
    int M1;                       // 0: no peel
    GemmLaunch tail;              // rows [M1, M): one 128 x 128 launch, or tail_slices k-slices through the workspace
    int tail_slices;              // 0: the one-launch tail; >= 2: slices of tail.kt_per_split k-tiles + a reduce
    int reduce_kind, reduce_blocks;      // gemm_tail_reduce_kernel<kind>: 0 = fp32, 1 = 16-bit, 2 = 16-bit hi/lo planes
};

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// One launch of the 16-bit tile kernels over `M` rows of `s` on a bm x bn tile.
inline GemmLaunch gemm_tile_launch(const GemmShape& s, int M, int bm, int bn, int splits, int kt_per_split, int ncu, int persist_slots, const GemmHooks& h) {
    const int wm = bm == 256 && bn == 256 ? 128 : 64, wn = 64;
    GemmLaunch l;
    l.M = M; l.bm = bm; l.bn = bn; l.splits = splits; l.kt_per_split = kt_per_split; l.kmap_unbuilt = false;
    l.threads = (bm / wm) * (bn / wn) * 64;
    l.lds = 2 * (bm + bn) * KT * 2;
    const int tiles = ceil_div(M, bm) * ceil_div(s.N, bn);
    l.grid_x = tiles; l.grid_y = splits;
    const bool whole_kt = s.K % KT == 0;
    if (s.planes16) {
        // The hi/lo-plane route of omlm_gemm_planes16 (row-major A [M, K] and B [N, K], no maps, no split-K): the half-tile-ring kernel for the
        // 256 x 256 tiles (whole k-tiles), the rotated-loop SPLIT3 kernel otherwise.
        l.form = (bm == 256 && bn == 256 && h.ring > 0 && whole_kt && !s.a_map && splits == 1) ? FORM_RING : FORM_ROT_SPLIT3;
        return l;
    }
    if (bm == 256 && bn == 256) {
        // more than one round of one-workgroup-per-CU tiles (whatever OMLM_GEMM_PERSIST says)
        const int keff = s.split3 ? 3 * s.K : s.K;
        const bool wanted = h.ring == 1 || (h.ring > 1 && splits == 1 && keff >= 2048 && tiles > ncu);
        // whole k-tiles, no maps on the operand side (a scatter map of C and split-K are fine)
        // (the hi/lo-plane route runs a 3x k-loop: K >= 704 already is a long contraction for it; its instantiations exist in the bf16 copy only)
        if (wanted && whole_kt && !s.a_map && !s.b_map && (!s.split3 || !s.fp16_copy)) { l.form = FORM_RING; return l; }
    }
    const bool need_kmap = (s.a_kmajor && s.a_map) || (s.b_kmajor && s.b_map);       // host routes these to the 128x128 tile
    if (need_kmap && bm != 128) { l.kmap_unbuilt = true; l.form = FORM_ROT_KMAP; return l; }
    // Persistent walk (gemm_bf16_tile_persist_kernel) for the wide tile when the problem is more than one round of the machine:
    // whole k-tiles, k-contiguous A, no maps on the k side, no split, no plane mode.  OMLM_GEMM_PERSIST=0 keeps the one-tile grid.
    if ((bm == 256 && bn == 256) || (bm == 128 && bn == 128)) {
        const int slots = (h.persist ? persist_slots : 0) * (bm == 128 ? 2 : 1);             // 64 KiB tiles: two workgroups per CU
        if (slots > 0 && !s.a_kmajor && splits == 1 && !s.split3 && !s.a_map && !s.b_map && !s.c_map && whole_kt && tiles > slots) {
            l.form = FORM_PERSIST; l.grid_x = slots; l.grid_y = 1; l.lds += 32 * (wn + 4) * 4;
            return l;
        }
    }
    // The fp16 copy of gemm.hip (common.h: OMLM_FP16) instantiates only the production kernel and its k-row-map form: the hi/lo-plane
    // (SPLIT3) instantiations exist once, in the bf16 copy.
    l.form = (s.split3 && !s.fp16_copy) ? FORM_ROT_SPLIT3 : need_kmap ? FORM_ROT_KMAP : whole_kt ? FORM_ROT_FASTK : FORM_ROT_GENERAL;
    return l;
}

inline GemmPlan gemm_plan(const GemmShape& s, int ncu, int persist_slots, const GemmHooks& h) {
    const int M = s.M, N = s.N, K = s.K;
    const int pslots = h.persist ? persist_slots : 0;
    // tile shape (bf16 path): 256x256 when both output dims are wide, 256x128 for tall-narrow outputs, else 128x128
    int bm = 128, bn = 128;
    const bool need_kmap = (s.a_kmajor && s.a_map) || (s.b_kmajor && s.b_map);
    if (s.in_dtype == 1 && !need_kmap) {
        if (h.tile_set) { if (h.force_bm) { bm = h.force_bm; bn = h.force_bn; } }
        // Short contractions onto narrow outputs (to_out, d(xn), d(x) of k | v: K <= 512, N <= 1024): with the persistent walk the 128x128
        // tiles (two walkers per CU, 4 x the tiles to balance) beat the wide ones -- to_out 103 -> 92 us, d(xn) 57 -> 50 us (round 4 probe).
        else if (K <= 512 && N <= 1024 && K % KT == 0 && !s.a_kmajor && !s.a_map && !s.b_map && !s.c_map && !s.split3 && !s.accumulates &&
                 ceil_div(M, 128) * ceil_div(N, 128) > 2 * pslots && pslots > 0) { bm = 128; bn = 128; }
        else if (M >= 1024 && N >= 1024) { bm = 256; bn = 256; }   // measured (probe, N = 1024): 256x256 514 us, 128x128 543, 256x128 657
        // N = 512 outputs (q-proj, d(o)): 128x128 (two workgroups per CU) measured 54 / 54 us against 60 / 59 for 256x128 (round 4 tile probe)
        else if (M >= 2048 && N > 512) { bm = 256; bn = 128; }
        else if (N >= 2048 && M >= 256) { bm = 256; bn = 256; }
    }
    // split-K only for accumulate-into-C GEMMs with few output tiles (the weight-gradient contractions).  The 256-wide
    // tiles run one workgroup per CU, so the split count is chosen for whole rounds of the machine: e.g. dW1 has 88 tiles;
    // 12 splits = 1056 workgroups = 4.1 rounds (82 % of the last 5 used), 11 splits = 968 = 3.8 rounds (95 %).
    const int nk = ceil_div(K, KT) * (s.split3 ? 3 : 1);     // k-tiles of the loop (three plane pairs per real k-tile when split3)
    const int tiles = ceil_div(M, bm) * ceil_div(N, bn);
    int splits = 1;
    // fp32 operands (register-staged kernel: the rel-pos MLP's 0.3-GFLOP GEMMs, 36 / 16 output tiles) are latency-bound per k-tile, not per byte:
    // they split down to TWO k-tiles per workgroup (54 -> ~20 us per launch; round 4), the 16-bit tile kernels keep their >= 8 k-tiles per split
    const bool fine = s.in_dtype == 0 && !s.split3;
    if (s.accumulates && s.out_dtype == 0 && tiles < 512 && nk >= (fine ? 4 : 16)) {
        const int slots = (bm == 256 ? 1 : 2) * ncu;              // co-resident workgroups (LDS: 128 KiB tiles 1 / CU, 64 KiB 2 / CU)
        int smax = fine ? nk / 2 : nk / 8; if (smax > 32) smax = 32; if (smax < 1) smax = 1;
        int smin = (slots + tiles - 1) / tiles; if (smin > smax) smin = smax; if (smin < 1) smin = 1;      // at least one full round
        float best = -1.f;
        for (int sp = smin; sp <= smax; ++sp) {
            const int total = tiles * sp, rounds = (total + slots - 1) / slots;
            // every split adds one atomic pass over C.  Re-measured after the k-major DMA fix (tools/splitk_probe.py): with the k-loop
            // faster the atomics weigh more -- 44 tiles (dW2): 5 / 11 splits = 233 / 267 us; 88 tiles (dW1): 5 / 8 / 11 = 479 / 478 / 515 us;
            // 128x128 tiles (dWq, dWkv: 64 KiB partials) keep the old weight: 16 / 32 splits stay best there.
            const float util = (float)total / (float)(rounds * slots) - (bm == 256 ? 0.02f : 0.012f) * (float)sp;
            if (util > best) { best = util; splits = sp; }
        }
    }
    const int ktps = (nk + splits - 1) / splits;
    splits = (nk + ktps - 1) / ktps;
    // (A balanced split-K grid -- every workgroup the same number of k-tiles -- measured slower on dW1: 665 against 642 us; the k-major
    // main loop, not the partial last round or the atomic volume, is what holds these GEMMs at ~620 TFLOP/s.)
    GemmPlan p;
    memset(&p, 0, sizeof(p));
    if (s.in_dtype == 0) {            // register-staged fp32 kernel: 128 x 128 x 64 per workgroup of 4 waves, 4 LDS planes (A/B x hi/lo)
        GemmLaunch& l = p.main;
        l.M = M; l.bm = 128; l.bn = 128; l.form = FORM_FP32_STAGED; l.splits = splits; l.kt_per_split = ktps;
        l.grid_x = tiles; l.grid_y = splits; l.threads = 256; l.lds = 4 * (128 * KT * 2);
        return p;
    }
    // Tail peeling for the one-workgroup-per-CU 256x256 tiles: dX-type GEMMs have 560 tiles = 2.19 rounds of 256 CUs, i.e. a
    // third round that is 19 % full.  The m-tile rows that fill whole rounds keep the 256x256 kernel; the remaining rows go to
    // the 128x128 kernel (2 workgroups per CU, ~1/3 of the time per tile).
    // (omlm_gemm_mx16 peels by its own rule: mx_plan below, the two side by side there)
    if (bm == 256 && bn == 256 && splits == 1 && !s.a_kmajor && !s.a_map && !s.c_map && !h.tile_set && tiles > ncu) {
        const int tiles_n = (N + 255) / 256, tiles_m = (M + 255) / 256;
        const int rem = tiles % ncu;
        const int m_full = ((tiles / ncu) * ncu) / tiles_n;
        if (rem > 0 && rem < ncu / 2 && m_full >= 1 && m_full < tiles_m) {
            p.M1 = m_full * 256;
            const int Mt = M - p.M1;
            p.main = gemm_tile_launch(s, p.M1, 256, 256, 1, ktps, ncu, persist_slots, h);
            // the tail: deterministic split-K through the workspace when it pays (see gemm_tail_reduce_kernel)
            if (s.ws_bytes > 0 && h.tail_split && s.alpha_one) {
                const int Nw = (N + 3) / 4 * 4;
                const int tiles_t = ((Mt + 127) / 128) * ((N + 127) / 128);
                int S = (2 * ncu) / tiles_t;
                if (S > nk / 8) S = nk / 8;
                if (S > 8) S = 8;
                if (S >= 2) {
                    const int kt = (nk + S - 1) / S;
                    S = (nk + kt - 1) / kt;
                    const long long slice = (long long)Mt * Nw;
                    if (S >= 2 && (long long)S * slice * 4 <= s.ws_bytes) {
                        GemmShape w = s;                       // the slices: fp32 into the workspace, no residual
                        w.out_dtype = 0; w.cin = false; w.accumulates = false;
                        p.tail = gemm_tile_launch(w, Mt, 128, 128, S, kt, ncu, persist_slots, h);
                        p.tail_slices = S;
                        const long long quads = (long long)Mt * (Nw / 4);
                        p.reduce_blocks = (int)((quads + 255) / 256 > 4096 ? 4096 : (quads + 255) / 256);
                        p.reduce_kind = s.out_dtype == 0 ? 0 : (s.planes16 ? 2 : 1);     // (16-bit planes leave the planes16 route only)
                        return p;
                    }
                }
            }
            p.tail = gemm_tile_launch(s, Mt, 128, 128, 1, ktps, ncu, persist_slots, h);
            return p;
        }
    }
    p.main = gemm_tile_launch(s, M, bm, bn, splits, ktps, ncu, persist_slots, h);
    return p;
}

// Workspace of the peeled tail's deterministic split-K: an upper bound of what an M x N output needs (8 fp32 slices of the at most
// one-machine-round tail).
inline long long gemm_tail_workspace_bytes(int M, int N, int ncu) {
    if (M <= 0 || N <= 0) return 0;
    const long long tiles_n = (N + 255) / 256, tiles_m = (M + 255) / 256;
    if (tiles_m * tiles_n <= ncu) return 0;
    long long tail_rows = ((long long)(ncu / 2) / tiles_n + 1) * 256;        // fewer than half a round of tiles ever go to the tail
    if (tail_rows > M) tail_rows = M;
    return 8ll * tail_rows * ((N + 3) / 4 * 4) * 4;
}

// ---- omlm_gemm_mx16 ----------------------------------------------------------------------------------------------------------------
// how the launch is cut: rows [0, M1) as whole machine rounds of 256 x 256 tiles, rows [M1, M) as S k-slices through the workspace.
// The same peel as gemm_plan's, as found, with these differences (none of them reconciled here):
//   - no `rem < ncu / 2` bound: any partial last round peels;
//   - the tail runs on 256-row tiles over ncu slots (gemm_plan: 128 x 128 tiles over 2 * ncu slots);
//   - slices start at even loop tiles (gemm_mx_body's two loops);
//   - without at least two slices that fit the workspace there is no peel at all (gemm_plan: the one-launch 128 x 128 tail).
struct MxPlan {
    int nk_all;        // loop tiles: K / 64 half tiles padded to even, then 2 x ceil(K / 128) fp8 tiles
    int M1, S, ktps;   // S < 2: one launch of all rows
    bool fused;        // full-round tiles and tail slices in one grid
    int main_tiles, tail_tiles, reduce_blocks;
};
inline MxPlan mx_plan(int M, int N, int K, long long ws_bytes, int ncu, const GemmHooks& h) {
    MxPlan p;
    const int tiles_n = (N + 255) / 256, tiles_m = (M + 255) / 256, tiles = tiles_m * tiles_n;
    const int nk_all = ((K / KT + 1) & ~1) + 2 * ((K + 127) / 128);
    p.nk_all = nk_all; p.M1 = M; p.S = 1; p.ktps = nk_all; p.fused = false; p.main_tiles = tiles; p.tail_tiles = 0; p.reduce_blocks = 0;
    if (tiles <= ncu) return p;
    const int rem = tiles % ncu;
    const int m_full = ((tiles / ncu) * ncu) / tiles_n;
    if (rem == 0 || m_full < 1 || m_full >= tiles_m) return p;
    const int Mt = M - m_full * 256, Nw = (N + 3) / 4 * 4;
    const int tiles_t = ((Mt + 255) / 256) * tiles_n;
    int s = ncu / tiles_t;
    if (s > nk_all / 8) s = nk_all / 8;
    if (s > 8) s = 8;
    if (s < 2) return p;
    const int per = ((nk_all + s - 1) / s + 1) & ~1;           // slices start at even loop tiles (gemm_mx_body's two loops)
    s = (nk_all + per - 1) / per;
    if (s < 2 || (long long)s * Mt * Nw * 4 > ws_bytes) return p;
    p.M1 = m_full * 256; p.S = s; p.ktps = per;
    p.main_tiles = m_full * tiles_n; p.tail_tiles = tiles_t;
    // one grid where the last round of the full tiles leaves CUs idle (FF-in at B = 32: 3058 tiles = 11.95 rounds; the tail's 88 slices start on the
    // 14 idle CUs and finish ~20 us behind the round instead of 41 us as their own launch: 804 -> 781 us).  A main part of WHOLE rounds (FF-out:
    // 512 tiles) gains nothing from it (381 -> 392 us measured): two launches.  OMLM_MX_FUSE_TAIL=0: always two launches.
    p.fused = h.mx_fuse_tail && p.main_tiles % ncu != 0;
    const long long quads = (long long)Mt * (Nw / 4);
    p.reduce_blocks = (int)((quads + 255) / 256 > 4096 ? 4096 : (quads + 255) / 256);
    return p;
}
// Workspace the tail of an M x N x K launch wants (0: none)
inline long long mx16_workspace_bytes(int M, int N, int K, int ncu) {
    const MxPlan p = mx_plan(M, N, K, (long long)1 << 62, ncu, GemmHooks());
    return p.S >= 2 ? (long long)p.S * (M - p.M1) * ((N + 3) / 4 * 4) * 4 : 0;
}

// ---- omlm_gemm_qknorm: 128 x 128 tiles, l2-norm epilogue ---------------------------------------------------------------------------
inline GemmLaunch qknorm_plan(int M, int N, int K, int persist_slots, const GemmHooks& h) {
    GemmLaunch l;
    l.M = M; l.bm = 128; l.bn = 128; l.splits = 1; l.kt_per_split = ceil_div(K, KT); l.kmap_unbuilt = false;
    l.threads = 256; l.lds = 2 * (128 + 128) * KT * 2;
    const int tiles = ceil_div(M, 128) * ceil_div(N, 128);
    l.grid_x = tiles; l.grid_y = 1;
    const int slots = 2 * (h.persist ? persist_slots : 0);                    // persistent walk, two workgroups per CU (see gemm_bf16_tile_persist_kernel)
    if (slots > 0 && tiles > slots && K % KT == 0) { l.form = FORM_PERSIST; l.grid_x = slots; l.lds += 32 * (64 + 4) * 4; }
    else l.form = K % KT == 0 ? FORM_ROT_FASTK : FORM_ROT_GENERAL;
    return l;
}

// ---- omlm_gemm_wgrad_group: one launch of 256 x 256 full-K (or lightly split) tiles over up to 48 problems -------------------------
struct WgradDims { int M, N, K; };
struct WgradPlan { int splits; GemmForm form; int total; };       // total: workgroups of the launch (512 threads, 128 KiB LDS)
// splits_arg: K-splits per tile for every problem (0 = chosen here for whole machine rounds); kt_per_split / start: per problem, n entries each
inline WgradPlan wgrad_group_plan(const WgradDims* d, int n, int splits_arg, int ncu, const GemmHooks& h, int* kt_per_split, int* start) {
    long long units = 0;
    int nk_min = 1 << 30;
    bool fastk = true;                                    // every problem's K a multiple of the k-tile depth: SGPR-offset DMA form
    for (int i = 0; i < n; ++i) {
        if (d[i].K % KT != 0) fastk = false;
        units += (long long)((d[i].M + 255) / 256) * ((d[i].N + 255) / 256);
        const int nk = ceil_div(d[i].K, KT);
        if (nk < nk_min) nk_min = nk;
    }
    int sp = splits_arg;
    if (sp <= 0) {
        // a unit = one full-K tile; s splits cut it into s workgroups of 1/s the work and add s atomic passes over C
        float best = -1.f;
        sp = 1;
        for (int s = 1; s <= 4; ++s) {
            const long long wgs = units * s, rounds = (wgs + ncu - 1) / ncu;
            const float util = (float)wgs / (float)(rounds * ncu) - 0.02f * (float)(s - 1);
            if (util > best) { best = util; sp = s; }
        }
    }
    if (sp > nk_min / 8) sp = nk_min / 8 > 0 ? nk_min / 8 : 1;
    int at = 0;
    for (int i = 0; i < n; ++i) {
        const int nk = ceil_div(d[i].K, KT);
        kt_per_split[i] = (nk + sp - 1) / sp;
        const int s_eff = (nk + kt_per_split[i] - 1) / kt_per_split[i];
        start[i] = at;
        at += ((d[i].M + 255) / 256) * ((d[i].N + 255) / 256) * s_eff;
    }
    WgradPlan p;
    p.splits = sp; p.total = at;
    p.form = fastk && h.ring > 0 ? FORM_RING : fastk ? FORM_ROT_FASTK : FORM_ROT_GENERAL;      // (the ring for any mode above 0)
    return p;
}

// ---- executing a peel: the argument blocks of the two parts (G: GemmArgs or omlm_gemm_mx16's GemmMxArgs; row-major A, no a_map / c_map) -----
// g1 = rows [0, M1), g2 = rows [M1, M) of g.  c_sz / lo_sz: bytes per element of C / C_lo.  Planes beside A (A_lo; the fp8 planes and row
// scales of the MX route) are the caller's to move.
template <typename G>
inline void peel_rows(const G& g, long long M1, size_t c_sz, size_t lo_sz, G& g1, G& g2) {
    g1 = g; g2 = g;
    g1.M = (int)M1;
    g2.M = g.M - (int)M1;
    g2.A = (const char*)g.A + (size_t)M1 * g.lda * 2;
    g2.a_rows = g.a_rows - M1;
    g2.C = (char*)g.C + (size_t)M1 * g.ldc * c_sz;
    if (g.C_lo) g2.C_lo = (char*)g.C_lo + (size_t)M1 * g.ldc * lo_sz;
    if (g.Cin) g2.Cin = g.Cin + (size_t)M1 * g.ldcin;
}
// the tail g2 as k-slices: every slice stores its fp32 partial [M, N padded to 4] to its own plane of the workspace
template <typename G>
inline G slice_args(const G& g2, void* ws) {
    G gw = g2;
    gw.C = ws; gw.C_lo = nullptr; gw.Cin = nullptr; gw.ldc = (g2.N + 3) / 4 * 4; gw.ldcin = 0;
    gw.c_split_stride = (long long)g2.M * gw.ldc;
    return gw;
}

}   // namespace omlm_plan

#ifdef OMLM_PLAN_TEST_ABI       /* tests/test_gemm_plan_host.py: the planners behind a flat C interface, built by the host c++ */
using namespace omlm_plan;
static GemmHooks hooks_of(const int* v) { GemmHooks h = {v[0] != 0, v[1], v[2] != 0, v[3], v[4], v[5] != 0, v[6] != 0}; return h; }
static int put(int* o, const GemmLaunch& l) {
    const int v[] = {l.form, l.bm, l.bn, l.grid_x, l.grid_y, l.threads, l.lds, l.splits, l.kt_per_split, l.kmap_unbuilt};
    memcpy(o, v, sizeof(v));
    return 10;
}
// sh: M N K a_kmajor b_kmajor a_map b_map c_map in_dtype out_dtype split3 planes16 copy accumulates cin alpha_one.
//   copy: 0 / 1 the call as the bf16 / fp16 copy sees it; 2 a call of the public entry (gemm_to_fp16_copy decides).
// out: M1, tail_slices, reduce_kind, reduce_blocks, then main and tail as put() writes them.  omlm_plan_gemm_fp16_copy: whether the fp16 copy
// serves the call.
static GemmShape shape_of(const int* sh, long long ws_bytes) {
    GemmShape s = {sh[0], sh[1], sh[2], sh[3] != 0, sh[4] != 0, sh[5] != 0, sh[6] != 0, sh[7] != 0, sh[8], sh[9], sh[10] != 0, sh[11] != 0,
                   sh[12] == 1, sh[13] != 0, sh[14] != 0, sh[15] != 0, ws_bytes};
    if (sh[12] == 2) s.fp16_copy = gemm_to_fp16_copy(s.in_dtype, s.out_dtype);
    return s;
}
extern "C" int omlm_plan_gemm_fp16_copy(const int* sh) { return shape_of(sh, 0).fp16_copy; }
extern "C" void omlm_plan_gemm(const int* sh, long long ws_bytes, int ncu, int persist_slots, const int* hooks, int* out) {
    const GemmPlan p = gemm_plan(shape_of(sh, ws_bytes), ncu, persist_slots, hooks_of(hooks));
    out[0] = p.M1; out[1] = p.tail_slices; out[2] = p.reduce_kind; out[3] = p.reduce_blocks;
    put(out + 4 + put(out + 4, p.main), p.tail);
}
// the copy that serves an entry that names one type (omlm_gemm_qknorm, omlm_gemm_planes16, omlm_gemm_wgrad_group), and the code it sees
extern "C" int omlm_plan_gemm_copy_of(int* dtype) { int out = *dtype; return gemm_to_fp16_copy(*dtype, out); }
extern "C" void omlm_plan_mx(int M, int N, int K, long long ws_bytes, int ncu, const int* hooks, int* out) {
    const MxPlan p = mx_plan(M, N, K, ws_bytes, ncu, hooks_of(hooks));
    const int v[] = {p.nk_all, p.M1, p.S, p.ktps, p.fused, p.main_tiles, p.tail_tiles, p.reduce_blocks};
    memcpy(out, v, sizeof(v));
}
extern "C" void omlm_plan_qknorm(int M, int N, int K, int persist_slots, const int* hooks, int* out) { put(out, qknorm_plan(M, N, K, persist_slots, hooks_of(hooks))); }
extern "C" void omlm_plan_wgrad(const int* mnk, int n, int splits, int ncu, const int* hooks, int* out, int* kt_per_split, int* start) {
    const WgradPlan p = wgrad_group_plan((const WgradDims*)mnk, n, splits, ncu, hooks_of(hooks), kt_per_split, start);
    out[0] = p.splits; out[1] = p.form; out[2] = p.total;
}
extern "C" long long omlm_plan_tail_ws(int M, int N, int ncu) { return gemm_tail_workspace_bytes(M, N, ncu); }
extern "C" long long omlm_plan_mx_ws(int M, int N, int K, int ncu) { return mx16_workspace_bytes(M, N, K, ncu); }
#endif
