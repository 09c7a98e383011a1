// MFMA GEMM for every dense contraction of the TokenConditionedTransformer path
// (to_q / to_kv / to_out, FF in/out, per-quantizer logit heads, and all their backward GEMMs).
//
//   C[m, n] = alpha * sum_k A(m, k) * B(n, k)  (+ Cin[m, n])
//
// A is either row-major [M, K] ("normal", k contiguous) or k-major [K, M] (A_KMAJ);
// B is either [N, K] (nn.Linear weight layout, k contiguous) or k-major [K, N] (B_KMAJ).
// With those two switches the forward (x W^T), the input-gradient (dY W) and the
// weight-gradient (dY^T X) contractions all read their operands exactly as the
// autograd graph leaves them in HBM -- no transposed copies are ever materialised.
// k-major tiles are staged row-for-row into LDS and fed to the matrix cores through the
// gfx950 hardware transpose read (ds_read_b64_tr_b16).
//
// Element type T selects the arithmetic:
//   T = bf16  : operands are bf16 in HBM, one v_mfma_f32_32x32x16_bf16 per k16 step  ("bf16")
//   T = float : operands are fp32 in HBM and are split on the fly into bf16 hi + bf16 lo
//               while being staged into LDS; hi*hi + hi*lo + lo*hi on the matrix cores
//               ("bf16x3": fp32-grade products at 1/3 of the bf16 MFMA rate, still ~5x the
//               fp32-MFMA rate).  Accumulation is fp32 in both modes.
//
// fp32 path (gemm_kernel): 128 x 128 x 64 per workgroup of 4 waves (2x2), each wave 64x64 = 2x2 MFMA 32x32 tiles;
// staging global -> registers (issued before the MFMA phase of the previous tile) -> split -> LDS after the barrier.
// LDS images are XOR-swizzled so that both ds_read_b128 (normal) and ds_read_b64_tr_b16 (k-major) fragment reads
// are conflict-free.
// Out-of-range rows/columns are read through a buffer descriptor with an out-of-bounds offset
// (hardware returns 0), so M, N and K may be ragged at 8-element granularity.
// Optional row maps (int32) gather A rows / k rows and scatter C rows: this is how the
// per-quantizer logit heads read the positions p = q (mod Q) of the hidden states in place.
//
// bf16 operands take the LDS-DMA path (gemm_bf16_tile_kernel: 256x256 / 256x128 / 128x128 tiles): tiles go HBM -> LDS directly with
// buffer_load_dwordx4 ... lds (no VGPR staging, no ds_write pass), the swizzle is applied on the
// per-lane SOURCE address (the DMA destination is lane-linear), LDS is double-buffered and there
// is ONE barrier per k-tile: the DMA of tile t+1 is in flight while tile t is on the matrix cores.
// fp32 operands (bf16x3) keep the register-staged path because they are split on the way in.
//
// Split-K: weight-gradient GEMMs have M x N = (out x in features) tiles only (32 tiles for to_q) but
// K = all tokens of the batch; gridDim.y splits K and the epilogue accumulates with fp32 atomics
// into C (these GEMMs are "C += ..." by construction: gradients accumulate over micro-batches).
#include "common.h"
#include "gemm_common.h"
#include "gemm_plan.h"

namespace OMLM_NS {

// One workgroup's share of C = alpha A B^T (+ Cin).  lg: logical workgroup id inside this problem's (tiles x K-splits, split-major)
// space; split: partial sums are added to fp32 C with atomics.
// FASTK: K is a multiple of the k-tile depth (host-checked): the DMA pieces take their k offset from an SGPR (DmaStagerT::issue_one)
template <int BM_, int BN_, int WM_, int WN_, bool A_KMAJ, bool B_KMAJ, typename TOUT, bool KMAP, bool SPLIT3 = false, bool FASTK = false, int EPI = 0>
__device__ __forceinline__ void gemm_tile_body(const GemmArgs& g, const int lg, const bool split, char* smem) {
    constexpr int NWN = BN_ / WN_, NWAVES = (BM_ / WM_) * NWN;
    constexpr int MI = WM_ / 32, NJ = WN_ / 32;
    constexpr int A_BYTES = BM_ * BK * 2, B_BYTES = BN_ * BK * 2, STAGE = A_BYTES + B_BYTES;
    constexpr int UA = (BM_ / 8) / NWAVES, UB = (BN_ / 8) / NWAVES;   // DMA wave-instructions per k-tile per wave

    const int tiles_m = (g.M + BM_ - 1) / BM_, tiles_n = (g.N + BN_ - 1) / BN_;
    const int nwg = tiles_m * tiles_n;
    const int nk1 = (g.K + BK - 1) / BK;
    const int nk_all = SPLIT3 ? 3 * nk1 : nk1;            // split3: k-tile t reads planes (t / nk1) at k = (t % nk1) * BK
    constexpr int GROUP = OMLM_SUPER_ROWS / BM_;                       // tile rows per super-tile (same footprint as the 128 kernel's 8)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = (wave / NWN) * WM_, wn = (wave % NWN) * WN_;
    const dma_rsrc rsA = make_dma_rsrc(g.A, (unsigned long long)g.a_rows * g.lda * 2);
    const dma_rsrc rsB = make_dma_rsrc(g.B, (unsigned long long)g.b_rows * g.ldb * 2);
    const dma_rsrc rsAl = make_dma_rsrc(SPLIT3 ? g.A_lo : g.A, (unsigned long long)g.a_rows * g.lda * 2);      // (plain kernels: never used)
    const dma_rsrc rsBl = make_dma_rsrc(SPLIT3 ? g.B_lo : g.B, (unsigned long long)g.b_rows * g.ldb * 2);

    {
        const int ksplit_id = lg / nwg;
        const int bid = lg - ksplit_id * nwg;
        const int kt0 = ksplit_id * g.kt_per_split;
        const int kt1 = min(nk_all, kt0 + g.kt_per_split);
        const int gsz = GROUP * tiles_n;
        const int grp = bid / gsz, first_m = grp * GROUP;
        const int rows_in = min(GROUP, tiles_m - first_m);
        const int tm = first_m + (bid - grp * gsz) % rows_in, tn = (bid - grp * gsz) / rows_in;
        const int m0 = tm * BM_, n0 = tn * BN_;

        DmaStagerT<A_KMAJ, BM_, NWAVES> sa;
        DmaStagerT<B_KMAJ, BN_, NWAVES> sb;
        sa.init(g.a_map, g.lda, g.M, m0, wave, lane);
        sb.init(g.b_map, g.ldb, g.N, n0, wave, lane);

        f32x16 acc[MI][NJ];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

        // k-tile index -> contraction offset and operand planes
        // (SPLIT3 is its own instantiation: the plain kernels keep the code and register allocation they were measured with)
        // pa / pb: the k-tile reads A's / B's lo plane (uniform: the descriptor is chosen by scalar selects)
        auto tile_at = [&](int t, bool& pa, bool& pb) -> int {
            if constexpr (SPLIT3) {
                const int which = t >= 2 * nk1 ? 2 : (t >= nk1 ? 1 : 0);
                pa = which == 2;
                pb = which == 1;
                return (t - which * nk1) * BK;
            } else {
                pa = false; pb = false;
                return t * BK;
            }
        };
        if (kt0 < kt1) {
            bool pa, pb;
            const int k00 = tile_at(kt0, pa, pb);
            sa.template issue<KMAP, FASTK>(SPLIT3 && pa ? rsAl : rsA, g.a_map, g.lda, k00, g.K, smem, wave);
            sb.template issue<KMAP, FASTK>(SPLIT3 && pb ? rsBl : rsB, g.b_map, g.ldb, k00, g.K, smem + A_BYTES, wave);
        }
        // Rotated k-loop: the MFMAs of a tile's LAST k16 step run AFTER the next tile's barrier and first fragment reads (their
        // operands are in registers), so the matrix pipe has work while the barrier releases and the first LDS reads of the new
        // tile are in flight; the next tile's DMA issue is spread over that deferred step and steps 0, 1, and step 2 covers its
        // latency.  Same products in the same order per accumulator.
        {
            h16x8 a[2][MI], b[2][NJ];
            bool pending = false;                                                  // a[1], b[1] hold an unmultiplied last step
            constexpr int MPS = MI * NJ, NLOAD = UA + UB;
            constexpr int SPREAD = 2;          // phases (of 4) over which the next tile's DMA issue is spread: 2 measured best (1: -5 %, 3: -1..+3 %, 4: worse)
            constexpr int STRIDE = (SPREAD * MPS) / NLOAD > 0 ? (SPREAD * MPS) / NLOAD : 1;
            for (int kt = kt0; kt < kt1; ++kt) {
                const int cur = (kt - kt0) & 1;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();      // tile kt landed everywhere; every wave's reads of the other stage (incl. its last step) are complete
                const bool live = kt + 1 < kt1;
                char* nxt = smem + (cur ^ 1) * STAGE;
                bool pan, pbn;
                const int knext = tile_at(kt + 1, pan, pbn);
                const dma_rsrc rsAn = SPLIT3 && pan ? rsAl : rsA, rsBn = SPLIT3 && pbn ? rsBl : rsB;
                const char* As = smem + cur * STAGE;
                const char* Bs = As + A_BYTES;
                // phase ph in 0..3 = (deferred last step of tile kt-1, step 0, step 1, step 2) of this iteration; fi = fragment set
                auto phase = [&](const int ph, const int fi, const bool mul) {
#pragma unroll
                    for (int i = 0; i < MI; ++i)
#pragma unroll
                        for (int j = 0; j < NJ; ++j) {
                            if (mul) acc[i][j] = OMLM_MFMA_32x32x16(a[fi][i], b[fi][j], acc[i][j]);
                            else if (mul) asm volatile("" :: "v"(a[fi][i]), "v"(b[fi][j]));
                            const int midx = ph * MPS + i * NJ + j;
                            if (midx % STRIDE == 0 && midx / STRIDE < NLOAD) {
                                const int l = midx / STRIDE;
                                __builtin_amdgcn_sched_barrier(0);
                                if (l < UA) sa.template issue_one<KMAP, FASTK>(l, rsAn, g.a_map, g.lda, knext, g.K, nxt, wave, live);
                                else        sb.template issue_one<KMAP, FASTK>(l - UA, rsBn, g.b_map, g.ldb, knext, g.K, nxt + A_BYTES, wave, live);
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                };
#pragma unroll
                for (int i = 0; i < MI; ++i) a[0][i] = read_frag<A_KMAJ>(As, wm + 32 * i, 0, lane);
#pragma unroll
                for (int j = 0; j < NJ; ++j) b[0][j] = read_frag<B_KMAJ>(Bs, wn + 32 * j, 0, lane);
                __builtin_amdgcn_sched_barrier(0);
                phase(0, 1, pending);                                              // last step of the previous tile (registers only)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int st = 0; st < 3; ++st) {
#pragma unroll
                    for (int i = 0; i < MI; ++i) a[(st + 1) & 1][i] = read_frag<A_KMAJ>(As, wm + 32 * i, st + 1, lane);
#pragma unroll
                    for (int j = 0; j < NJ; ++j) b[(st + 1) & 1][j] = read_frag<B_KMAJ>(Bs, wn + 32 * j, st + 1, lane);
                    __builtin_amdgcn_sched_barrier(0);
                    phase(st + 1, st & 1, true);
                    __builtin_amdgcn_sched_barrier(0);
                }
                pending = true;
            }
            if (pending) {
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) acc[i][j] = OMLM_MFMA_32x32x16(a[1][i], b[1][j], acc[i][j]);
            }
        }
        // The last iteration issued its "next tile" DMA pieces with out-of-bounds offsets (`live` false): no memory traffic, but the
        // hardware still writes their ZEROS into the other LDS stage -- the stage the epilogue below re-uses as its transpose patch
        // (smem + 0 .. for an even k-tile count, e.g. K = 1024 / 512).  They are inline asm, i.e. invisible to hipcc's vmcnt
        // bookkeeping, so without this wait nothing orders them before the epilogue's ds_writes: a late zero-fill wiped staged output
        // values (round 3: intermittent 30-70 % error in the rel-pos MLP's gradient -- its GEMMs run on the second stream next to the
        // trunk's HBM-bound kernels, whose traffic delays the pieces past the ~500 cycles the remaining MFMAs of a 128x128 tile take).
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        constexpr bool SLICE = BM_ == 128 && BN_ == 128 && std::is_same<TOUT, float>::value && EPI == 0;
        tile_epilogue<MI, NJ, WN_, TOUT, EPI, (MI * NJ <= 4), SLICE>(g, acc, smem, m0, n0, wm, wn, wave, lane, split, nullptr,
                                                                     SLICE ? ksplit_id : 0);
    }
}

// For split-K GEMMs the split-major XCD order puts all co-resident workgroups of an XCD on the SAME K range (they share A and B
// panels through its L2); with a tile-only remap an XCD held 3 unrelated K ranges at a time (measured L2 hit 48 % on the dW1 GEMM).
template <int BM_, int BN_, int WM_, int WN_, bool A_KMAJ, bool B_KMAJ, typename TOUT, bool KMAP, bool SPLIT3 = false, bool FASTK = false, int EPI = 0>
__global__ __launch_bounds__((BM_ / WM_) * (BN_ / WN_) * 64) void gemm_bf16_tile_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 stages][A | B]
    const int nwg = gridDim.x;                                     // tiles
    const int total = nwg * (int)gridDim.y;
    const int lg = xcd_logical_id(blockIdx.y * nwg + blockIdx.x, total);
    gemm_tile_body<BM_, BN_, WM_, WN_, A_KMAJ, B_KMAJ, TOUT, KMAP, SPLIT3, FASTK, EPI>(g, lg, gridDim.y > 1, smem);
}


// ---- persistent form of the wide tile kernel -----------------------------------------------------------------------------
// The 256x256 tiles run ONE workgroup per CU (128 KiB of LDS), so nothing overlaps a workgroup's prologue (first k-tile: a full L2 / HBM
// round trip), its epilogue and the dispatch of its successor: ~12 % of a K = 1024 tile (16 k-tiles), 32.5 us per tile against 28.6 us
// at the rate of the k-loop (round 4).  Here G = gridDim.x workgroups (one per CU, G a multiple of 8) each walk the tiles
// lin, lin + G, lin + 2G, ... of the XCD-aware order (lin & 7 is constant, so the walk stays inside its XCD's chunk and the 32 workgroups
// of an XCD move through consecutive super-tile patches together), and the LAST k-iteration of a tile requests the FIRST k-tile of the
// next one -- in the slots where the one-tile kernel issues its dead pieces -- so that tile's first round trip runs under this tile's
// epilogue.  The request lands in the stage the last k-tile did not use; the epilogue's transpose patches therefore live in the
// stage of the last k-tile (seven waves) and in 8.5 KiB behind the two stages (the eighth), never under a landing DMA piece.
// Order: [k-loop ... last iteration: DMA(next tile, k-tile 0) -> stage X] barrier [epilogue: patches in stage X^1 / behind] [next
// tile, iteration 0: vmcnt wait + barrier, DMA(k-tile 1) -> stage X^1, multiply from stage X].  The barrier of iteration 0 is what
// orders every wave's patch traffic before the first piece of k-tile 1 lands in stage X^1.
// Only the shape the host sends here is built: whole k-tiles (K % 64 == 0), no row / k-row / scatter maps, no split-K, plain epilogue.
// Iteration 0 of a follow-up tile waits for its DMA pieces only (counted), not for the epilogue's stores behind them.
// CIN: the epilogue adds a residual.  It is a template switch because the residual loads are what hipcc has to protect in the NEXT
// tile's first iteration (their registers are re-used; paths that skip a row leave a load unconsumed): with them in the code,
// iteration 0 carries compiler waits that drain the epilogue's stores whatever the run-time pointer is (seen in the ISA).
template <int BM_, int BN_, int WM_, int WN_, bool A_KMAJ, bool B_KMAJ, typename TOUT, bool CIN, int EPI = 0>
__global__ __launch_bounds__((BM_ / WM_) * (BN_ / WN_) * 64) void gemm_bf16_tile_persist_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 stages][A | B] + one transpose patch
    constexpr int NWN = BN_ / WN_, NWAVES = (BM_ / WM_) * NWN;
    constexpr int MI = WM_ / 32, NJ = WN_ / 32;
    constexpr int A_BYTES = BM_ * BK * 2, B_BYTES = BN_ * BK * 2, STAGE = A_BYTES + B_BYTES;
    constexpr int UA = (BM_ / 8) / NWAVES, UB = (BN_ / 8) / NWAVES;
    constexpr int PATCH = 32 * (WN_ + 4) * 4;                      // one wave's transpose patch (tile_epilogue: 32 rows x SROW floats)
    static_assert((NWAVES - 1) * PATCH <= STAGE, "all but the last wave's patch must fit inside one stage");
    constexpr int GROUP = OMLM_SUPER_ROWS / BM_;
    constexpr int VEC = sizeof(TOUT) == 2 ? 8 : 4, NSTORE = MI * (32 / (64 / (WN_ / VEC)));   // 16-byte stores per wave of a full tile's epilogue

    const int tiles_m = (g.M + BM_ - 1) / BM_, tiles_n = (g.N + BN_ - 1) / BN_;
    const int total = tiles_m * tiles_n;
    const int nk = g.K / BK;                                       // host: K % 64 == 0, K > 0
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = (wave / NWN) * WM_, wn = (wave % NWN) * WN_;
    const dma_rsrc rsA = make_dma_rsrc(g.A, (unsigned long long)g.a_rows * g.lda * 2);
    const dma_rsrc rsB = make_dma_rsrc(g.B, (unsigned long long)g.b_rows * g.ldb * 2);
    const unsigned smem_lds = (unsigned)(size_t)LDS_PTR(char, smem);

    auto origin = [&](int lin, int& m0, int& n0) {                 // the one-tile kernel's order (xcd_logical_id + super-tiles)
        const int bid = xcd_logical_id(lin, total);
        const int gsz = GROUP * tiles_n;
        const int grp = bid / gsz, first_m = grp * GROUP;
        const int rows_in = min(GROUP, tiles_m - first_m);
        m0 = (first_m + (bid - grp * gsz) % rows_in) * BM_;
        n0 = ((bid - grp * gsz) / rows_in) * BN_;
    };
    // one 1-KiB piece of k-tile k0 (same address form as DmaStagerT::issue_one<false, true>)
    auto piece = [&](int l, const unsigned (&va)[UA], const unsigned (&vb)[UB], int k0, unsigned stage_lds, bool live) {
        if (l < UA) {
            const int b = wave + NWAVES * l;
            dma_issue_s(rsA, stage_lds + (unsigned)(b * 1024), live ? va[l] : OOB_OFF,
                        A_KMAJ ? (unsigned)k0 * (unsigned)(g.lda * 2) : (unsigned)(k0 * 2));
        } else {
            const int b = wave + NWAVES * (l - UA);
            dma_issue_s(rsB, stage_lds + (unsigned)A_BYTES + (unsigned)(b * 1024), live ? vb[l - UA] : OOB_OFF,
                        B_KMAJ ? (unsigned)k0 * (unsigned)(g.ldb * 2) : (unsigned)(k0 * 2));
        }
    };

    int lin = blockIdx.x;
    const int G = gridDim.x;
    if (lin >= total) return;
    int m0, n0;
    origin(lin, m0, n0);
    unsigned va[UA], vb[UB];                                       // per-lane byte offsets of this tile's pieces at k = 0
    {
        DmaStagerT<A_KMAJ, BM_, NWAVES> sa;
        DmaStagerT<B_KMAJ, BN_, NWAVES> sb;
        sa.init(nullptr, g.lda, g.M, m0, wave, lane);
        sb.init(nullptr, g.ldb, g.N, n0, wave, lane);
#pragma unroll
        for (int i = 0; i < UA; ++i) va[i] = sa.vfast[i];
#pragma unroll
        for (int i = 0; i < UB; ++i) vb[i] = sb.vfast[i];
    }
    int par = 0;                                                   // stage of the current tile's k-tile 0
#pragma unroll
    for (int l = 0; l < UA + UB; ++l) piece(l, va, vb, 0, smem_lds, true);
    bool counted = false;                                          // the pieces of k-tile 0 are older than >= NSTORE stores of the previous epilogue

    for (;;) {
        const int lin_n = lin + G;
        const bool has_next = lin_n < total;
        int m0n = m0, n0n = n0;
        if (has_next) origin(lin_n, m0n, n0n);
        unsigned van[UA], vbn[UB];
        {
            DmaStagerT<A_KMAJ, BM_, NWAVES> sa;
            DmaStagerT<B_KMAJ, BN_, NWAVES> sb;
            sa.init(nullptr, g.lda, g.M, m0n, wave, lane);
            sb.init(nullptr, g.ldb, g.N, n0n, wave, lane);
#pragma unroll
            for (int i = 0; i < UA; ++i) van[i] = sa.vfast[i];
#pragma unroll
            for (int i = 0; i < UB; ++i) vbn[i] = sb.vfast[i];
        }
        f32x16 acc[MI][NJ];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        {   // the rotated k-loop of gemm_tile_body (same products in the same order per accumulator)
            h16x8 a[2][MI], b[2][NJ];
            bool pending = false;
            constexpr int MPS = MI * NJ, NLOAD = UA + UB;
            constexpr int SPREAD = 2;
            constexpr int STRIDE = (SPREAD * MPS) / NLOAD > 0 ? (SPREAD * MPS) / NLOAD : 1;
            for (int kt = 0; kt < nk; ++kt) {
                const int cur = (par + kt) & 1;
                if (kt == 0 && counted) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NSTORE) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                const bool last = kt + 1 == nk;
                const bool live = !last || has_next;
                const unsigned nxt = smem_lds + (unsigned)((cur ^ 1) * STAGE);
                const int knext = last ? 0 : (kt + 1) * BK;
                const char* As = smem + cur * STAGE;
                const char* Bs = As + A_BYTES;
                auto phase = [&](const int ph, const int fi, const bool mul) {
#pragma unroll
                    for (int i = 0; i < MI; ++i)
#pragma unroll
                        for (int j = 0; j < NJ; ++j) {
                            if (mul) acc[i][j] = OMLM_MFMA_32x32x16(a[fi][i], b[fi][j], acc[i][j]);
                            const int midx = ph * MPS + i * NJ + j;
                            if (midx % STRIDE == 0 && midx / STRIDE < NLOAD) {
                                const int l = midx / STRIDE;
                                __builtin_amdgcn_sched_barrier(0);
                                unsigned v;
                                if (l < UA) v = last ? van[l] : va[l]; else v = last ? vbn[l - UA] : vb[l - UA];
                                {
                                    unsigned one_a[UA], one_b[UB];
#pragma unroll
                                    for (int x = 0; x < UA; ++x) one_a[x] = v;
#pragma unroll
                                    for (int x = 0; x < UB; ++x) one_b[x] = v;
                                    piece(l, one_a, one_b, knext, nxt, live);
                                }
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                };
#pragma unroll
                for (int i = 0; i < MI; ++i) a[0][i] = read_frag<A_KMAJ>(As, wm + 32 * i, 0, lane);
#pragma unroll
                for (int j = 0; j < NJ; ++j) b[0][j] = read_frag<B_KMAJ>(Bs, wn + 32 * j, 0, lane);
                __builtin_amdgcn_sched_barrier(0);
                phase(0, 1, pending);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int st = 0; st < 3; ++st) {
#pragma unroll
                    for (int i = 0; i < MI; ++i) a[(st + 1) & 1][i] = read_frag<A_KMAJ>(As, wm + 32 * i, st + 1, lane);
#pragma unroll
                    for (int j = 0; j < NJ; ++j) b[(st + 1) & 1][j] = read_frag<B_KMAJ>(Bs, wn + 32 * j, st + 1, lane);
                    __builtin_amdgcn_sched_barrier(0);
                    phase(st + 1, st & 1, true);
                    __builtin_amdgcn_sched_barrier(0);
                }
                pending = true;
            }
            if (pending) {
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) acc[i][j] = OMLM_MFMA_32x32x16(a[1][i], b[1][j], acc[i][j]);
            }
        }
        const int cur_last = (par + nk - 1) & 1;
        // Last tile of the walk: its final iteration issued dead pieces (zeros) into the other stage, which nothing reads or patches again;
        // they are waited for all the same, so that the kernel never ends with LDS writes in flight.
        if (!has_next) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                           // every wave's fragment reads of the last k-tile's stage are complete
        float* patch = wave < NWAVES - 1 ? (float*)(smem + cur_last * STAGE + wave * PATCH) : (float*)(smem + 2 * STAGE);
        GemmArgs ge = g;
        ge.c_map = nullptr;                                        // host: no scatter map on this route
        if constexpr (!CIN) ge.Cin = nullptr;
        tile_epilogue<MI, NJ, WN_, TOUT, EPI, false>(ge, acc, smem, m0, n0, wm, wn, wave, lane, false, patch);    // (no second residual set: registers)
        if (!has_next) break;
        // a full interior tile's epilogue issued exactly NSTORE 16-byte stores per wave behind the next tile's pieces (more on the scalar
        // path): `vmcnt(NSTORE)` then covers the pieces; an edge tile skips stores, so its successor drains everything
        counted = m0 + BM_ <= g.M && n0 + BN_ <= g.N;
        par = (par + nk) & 1;
        lin = lin_n; m0 = m0n; n0 = n0n;
#pragma unroll
        for (int i = 0; i < UA; ++i) va[i] = van[i];
#pragma unroll
        for (int i = 0; i < UB; ++i) vb[i] = vbn[i];
    }
}


// ---- round 5: the wide tile on a half-tile ring with counted waits (two staggered wave groups) ----------------------------------
// What the k-loops above still pay (rounds 1-4): ONE barrier and a full `s_waitcnt vmcnt(0)` per k-tile with ONE tile of DMA in flight -- the
// youngest piece of k-tile t + 1 has ~1.5 of tile t's 4 k16 steps to land, so every L2 miss (and, under load, many hits) is exposed, and
// after each barrier all eight waves of the one workgroup per CU wait for their first fragments together (MFMA pipe busy 47 %).
// This body keeps the 256 x 256 x 64 tile, the LDS images and the fragment reads, and changes the schedule:
//   * the unit of staging is a HALF-tile (128 rows or columns x 64 k = 16 KiB = two 1-KiB DMA pieces per wave); LDS holds two k-tiles =
//     8 half-tile slots, and a slot is re-requested two phases after its last fragment read -- FIVE half-tiles (80 KiB) are in flight
//     behind a counted `s_waitcnt vmcnt(10)` per phase, never 0: every piece has ~5 phases (~1300 MFMA cycles) to land;
//   * a k-tile is four PHASES, one 64 x 32 quadrant of the wave's output per phase (8 MFMAs = 256 matrix-pipe cycles): the wave owns
//     rows ha * 128 + wr * 64 + [0, 64) and columns hb * 128 + wc * 32 + [0, 32) for ha, hb in {0, 1}, so quadrant (ha, hb) needs exactly
//     half-tiles A_ha and B_hb; quadrant order (0,0) (0,1) (1,1) (1,0): a phase reads ONE new half (A0: 8 ds_read_b128, B1: 4, A1: 8, and
//     in the last phase B0 of the NEXT k-tile: 4 -- the B fragments rotate through three register sets), requests one half-tile, waits
//     (counted) for the half the next phase reads, `s_barrier`, multiplies, `s_barrier`;
//   * waves 4-7 run ONE barrier behind waves 0-3: on every SIMD one wave is on the matrix pipe while its partner reads fragments and
//     issues DMA -- the fragment latency is covered by the partner's MFMAs instead of by a rotated loop.
// Event order (e_n: 4T = B0(T), 4T+1 = A0(T), 4T+2 = B1(T), 4T+3 = A1(T)): e_n is read in phase n - 1 and requested in phase n - 7
// (prologue: e_0 .. e_6); at the wait of phase g, e_(g+2) must have landed and e_(g+3) .. e_(g+7) stay in flight: vmcnt(10).
//   RAW: a wave's own pieces are covered by its counted wait, the other waves' by the barrier(s) behind their waits -- group 1's wait of
//        phase g sits one barrier later than group 0's, still in front of the barrier that opens group 0's phase g + 1 reads;
//   WAR: e_(g+7) overwrites the slot last read in phase g - 2 (A0: 4T -> requested in 4T + 2, etc.): both groups' reads of that phase have
//        been retired by their `lgkmcnt(0)` behind the phase's first barrier, two and one barriers before the request respectively.
// Requests past the last k-tile are issued dead (out-of-bounds offset: zeros, no traffic) so that the counts stay uniform; they are
// drained in front of the epilogue (the tail race of round 4).  Whole k-tiles only (K % 64 == 0), no row maps on the operands.
template <bool A_KMAJ, bool B_KMAJ, typename TOUT, bool SPLIT3 = false>
__device__ __forceinline__ void gemm_tile8_body(const GemmArgs& g, const int m0, const int n0, const int kt0, const int kt1, const bool split, char* smem) {
    constexpr int A_BYTES = 256 * BK * 2, STAGE = 2 * A_BYTES;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const dma_rsrc rsA = make_dma_rsrc(g.A, (unsigned long long)g.a_rows * g.lda * 2);
    const dma_rsrc rsB = make_dma_rsrc(g.B, (unsigned long long)g.b_rows * g.ldb * 2);
    const dma_rsrc rsAl = make_dma_rsrc(SPLIT3 ? g.A_lo : g.A, (unsigned long long)g.a_rows * g.lda * 2);      // (plain kernels: never used)
    const dma_rsrc rsBl = make_dma_rsrc(SPLIT3 ? g.B_lo : g.B, (unsigned long long)g.b_rows * g.ldb * 2);
    DmaStagerT<A_KMAJ, 256, 8> sa;          // unit i of a wave is 1-KiB unit b = wave + 8 i of the tile image: i < 2 -> rows / columns [0, 128) = half 0
    DmaStagerT<B_KMAJ, 256, 8> sb;
    sa.init(nullptr, g.lda, g.M, m0, wave, lane);
    sb.init(nullptr, g.ldb, g.N, n0, wave, lane);
    const int nk = kt1 - kt0;
    const unsigned smem_lds = (unsigned)(size_t)LDS_PTR(char, smem);

    f32x16 acc[2][2][2];                    // [ha][hb][i]: rows ha * 128 + wr * 64 + 32 i, columns hb * 128 + wc * 32
#pragma unroll
    for (int x = 0; x < 8; ++x)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[x >> 2][(x >> 1) & 1][x & 1][e] = 0.f;

    // request event e_n, n = 4 T + J (J a compile-time constant): two pieces per wave
    auto stage = [&](auto JC, const int T) {
        constexpr int J = decltype(JC)::value;
        constexpr bool isA = (J & 1) != 0;
        constexpr int h = J >> 1;
        const bool live = T < nk;
        unsigned k0 = (unsigned)(kt0 + T) * BK;
        bool lo = false;                        // this event reads its operand's lo plane (uniform)
        if constexpr (SPLIT3) {
            // hi/lo operand planes ("bf16x3"): loop tile t reads planes (A_hi, B_hi), (A_hi, B_lo), (A_lo, B_hi) at k = (t mod nk1) * 64 -- gemm_tile_body's tile_at
            const int t = kt0 + T, nk1 = g.K / BK;
            const int which = t >= 2 * nk1 ? 2 : (t >= nk1 ? 1 : 0);
            k0 = (unsigned)(t - which * nk1) * BK;
            lo = isA ? which == 2 : which == 1;
        }
        const dma_rsrc rs = isA ? (SPLIT3 && lo ? rsAl : rsA) : (SPLIT3 && lo ? rsBl : rsB);
        if constexpr (SPLIT3) k0 = (unsigned)__builtin_amdgcn_readfirstlane((int)k0);      // (hipcc keeps the plane arithmetic on the VALU: the offset must reach the DMA in an SGPR)
        const unsigned base = smem_lds + (unsigned)((T & 1) * STAGE) + (isA ? 0u : (unsigned)A_BYTES);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = 2 * h + u;
            const int b = wave + 8 * i;
            if constexpr (isA) dma_issue_s(rs, base + (unsigned)(b * 1024), live ? sa.vfast[i] : OOB_OFF, A_KMAJ ? k0 * (unsigned)(g.lda * 2) : k0 * 2u);
            else               dma_issue_s(rs, base + (unsigned)(b * 1024), live ? sb.vfast[i] : OOB_OFF, B_KMAJ ? k0 * (unsigned)(g.ldb * 2) : k0 * 2u);
        }
    };
    using J0 = std::integral_constant<int, 0>; using J1 = std::integral_constant<int, 1>;
    using J2 = std::integral_constant<int, 2>; using J3 = std::integral_constant<int, 3>;

    h16x8 a[2][4], bX[4], bY[4], bZ[4];
    auto read_a = [&](const int T, const int ha) {
        const char* As = smem + (T & 1) * STAGE;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int st = 0; st < 4; ++st) a[i][st] = read_frag<A_KMAJ>(As, ha * 128 + wr * 64 + 32 * i, st, lane);
    };
    auto read_b = [&](h16x8 (&b)[4], const int T, const int hb) {
        const char* Bs = smem + (T & 1) * STAGE + A_BYTES;
#pragma unroll
        for (int st = 0; st < 4; ++st) b[st] = read_frag<B_KMAJ>(Bs, hb * 128 + wc * 32, st, lane);
    };
    auto mma = [&](f32x16 (&c)[2], const h16x8 (&b)[4]) {
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int i = 0; i < 2; ++i) c[i] = OMLM_MFMA_32x32x16(a[i][st], b[st], c[i]);
        __builtin_amdgcn_s_setprio(0);
    };
    // the synchronisation of one phase: (reads and the request were just issued) counted wait -> barrier -> fragments in -> MFMAs -> barrier
#define T8_SYNC_IN()                                                           \
    do {                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                     \
        asm volatile("s_waitcnt vmcnt(10)" ::: "memory");                      \
        __builtin_amdgcn_s_barrier();                                          \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                     \
        __builtin_amdgcn_sched_barrier(0);                                     \
    } while (0)
#define T8_SYNC_OUT()                                                          \
    do {                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                     \
        __builtin_amdgcn_s_barrier();                                          \
        __builtin_amdgcn_sched_barrier(0);                                     \
    } while (0)

    // prologue: e_0 .. e_6 = all of k-tile 0 and B0, A0, B1 of k-tile 1
    stage(J0{}, 0); stage(J1{}, 0); stage(J2{}, 0); stage(J3{}, 0);
    stage(J0{}, 1); stage(J1{}, 1); stage(J2{}, 1);
    asm volatile("s_waitcnt vmcnt(10)" ::: "memory");                          // e_0 (B0 of k-tile 0) and e_1 (A0) are in
    __builtin_amdgcn_s_barrier();
    read_b(bX, 0, 0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                         // (retired before anyone may re-request that slot: phase 1)
    __builtin_amdgcn_sched_barrier(0);
    if (wr == 1) __builtin_amdgcn_s_barrier();                                 // waves 4-7 run one barrier behind from here on

    // one k-tile: b0 holds B0 of this tile (read in the previous tile's last phase), bn receives B0 of the next tile
    auto ktile = [&](h16x8 (&b0)[4], h16x8 (&bn)[4], const int T) {
        read_a(T, 0);             stage(J3{}, T + 1);  T8_SYNC_IN();  mma(acc[0][0], b0);  T8_SYNC_OUT();     // phase 0: A0 -> (0, 0); request A1(T + 1)
        read_b(bY, T, 1);         stage(J0{}, T + 2);  T8_SYNC_IN();  mma(acc[0][1], bY);  T8_SYNC_OUT();     // phase 1: B1 -> (0, 1); request B0(T + 2)
        read_a(T, 1);             stage(J1{}, T + 2);  T8_SYNC_IN();  mma(acc[1][1], bY);  T8_SYNC_OUT();     // phase 2: A1 -> (1, 1); request A0(T + 2)
        read_b(bn, T + 1, 0);     stage(J2{}, T + 2);  T8_SYNC_IN();  mma(acc[1][0], b0);  T8_SYNC_OUT();     // phase 3: B0(T + 1) for later; (1, 0); request B1(T + 2)
    };
    for (int T = 0; T < nk; T += 2) {
        ktile(bX, bZ, T);
        if (T + 1 < nk) ktile(bZ, bX, T + 1);
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();                                 // waves 0-3 wait for the others' last phase
#undef T8_SYNC_IN
#undef T8_SYNC_OUT
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                           // the dead requests of the last phases (zeros into LDS) are drained
    __syncthreads();
    // epilogue: the wave's four 64 x 32 quadrants through its LDS patch (tile_epilogue, 32-column form)
#pragma unroll
    for (int ha = 0; ha < 2; ++ha)
#pragma unroll
        for (int hb = 0; hb < 2; ++hb)
            tile_epilogue<2, 1, 32, TOUT>(g, reinterpret_cast<f32x16 (&)[2][1]>(acc[ha][hb]), smem, m0, n0, ha * 128 + wr * 64, hb * 128 + wc * 32,
                                          wave, lane, split);
}

// one output tile per workgroup, the tile / split order of gemm_bf16_tile_kernel
template <bool A_KMAJ, bool B_KMAJ, typename TOUT, bool SPLIT3 = false>
__global__ __launch_bounds__(512) void gemm_tile8_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 k-tiles][A | B]
    const int nwg = gridDim.x;
    const int lg = xcd_logical_id(blockIdx.y * nwg + blockIdx.x, nwg * (int)gridDim.y);
    const int tiles_m = (g.M + 255) / 256, tiles_n = (g.N + 255) / 256;
    const int ksplit = lg / nwg, bid = lg - ksplit * nwg;
    const int nk_all = (SPLIT3 ? 3 : 1) * (g.K / BK);
    const int kt0 = ksplit * g.kt_per_split, kt1 = min(nk_all, kt0 + g.kt_per_split);
    constexpr int GROUP = OMLM_SUPER_ROWS / 256;
    const int gsz = GROUP * tiles_n;
    const int grp = bid / gsz, first_m = grp * GROUP;
    const int rows_in = min(GROUP, tiles_m - first_m);
    const int tm = first_m + (bid - grp * gsz) % rows_in, tn = (bid - grp * gsz) / rows_in;
    if (kt0 >= kt1) return;
    gemm_tile8_body<A_KMAJ, B_KMAJ, TOUT, SPLIT3>(g, tm * 256, tn * 256, kt0, kt1, gridDim.y > 1, smem);
}


// ---- grouped weight-gradient GEMM ------------------------------------------------------------------------------------
// All dW += dY^T X contractions of a backward pass (same K = tokens, small outputs) as ONE launch: the 30 separate GEMMs of a
// coarse-small step each had too few output tiles for 256 CUs and were split 5..31 ways along K with fp32 atomics
// (dW2: 44 tiles x 11 splits, 640 TFLOP/s); together they are ~900 full-K tiles, i.e. 3-4 machine rounds with few or no atomics.
// Nothing consumes a weight gradient before the optimizer, so the host defers them to the end of the backward.
#define OMLM_GROUP_MAX 48
struct omlm_gemm_wgrad_desc { const void* A; const void* B; float* C; const int* c_map; int M, N, K, lda, ldb, ldc; };   // include/omlm.h
struct GroupProb { const void* A; const void* B; float* C; const int* c_map; int M, N, K, lda, ldb, ldc, kt_per_split, start; };
struct GroupArgs { int n, total; GroupProb p[OMLM_GROUP_MAX]; };

template <bool FASTK, bool T8 = false>
__global__ __launch_bounds__(512) void gemm_wgrad_group_kernel(GroupArgs ga) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lg = xcd_logical_id(blockIdx.x, ga.total);
    int pi = 0;
    for (int i = 1; i < ga.n; ++i) if (lg >= ga.p[i].start) pi = i;      // uniform scalar scan (starts ascend)
    const GroupProb& q = ga.p[pi];
    GemmArgs g;
    g.A = q.A; g.B = q.B; g.C = q.C; g.Cin = q.C; g.a_map = nullptr; g.b_map = nullptr; g.c_map = q.c_map;
    g.a_rows = q.K; g.b_rows = q.K; g.M = q.M; g.N = q.N; g.K = q.K; g.lda = q.lda; g.ldb = q.ldb; g.ldc = q.ldc; g.ldcin = q.ldc;
    g.alpha = 1.f; g.kt_per_split = q.kt_per_split; g.bal_ck = 0; g.bal_chunks = 0; g.debug = 0; g.split3 = 0; g.A_lo = nullptr; g.B_lo = nullptr; g.C_lo = nullptr; g.c_lo8 = 0; g.c_split_stride = 0;
    g.epi_scale = nullptr; g.epi_norm = nullptr; g.epi_groups = 0; g.epi_ldnorm = 0; g.C2 = nullptr; g.c2_col0 = 0; g.ldc2 = 0;
    const int nk = (q.K + BK - 1) / BK;
    if constexpr (T8) {
        // the half-tile-ring schedule (round 5), same tile / split numbering as gemm_tile_body
        const int lq = lg - q.start;
        const int tiles_m = (q.M + 255) / 256, tiles_n = (q.N + 255) / 256, nwg = tiles_m * tiles_n;
        const int ksplit = lq / nwg, bid = lq - ksplit * nwg;
        const int kt0 = ksplit * q.kt_per_split, kt1 = min(nk, kt0 + q.kt_per_split);
        constexpr int GROUP = OMLM_SUPER_ROWS / 256;
        const int gsz = GROUP * tiles_n;
        const int grp = bid / gsz, first_m = grp * GROUP;
        const int rows_in = min(GROUP, tiles_m - first_m);
        const int tm = first_m + (bid - grp * gsz) % rows_in, tn = (bid - grp * gsz) / rows_in;
        if (kt0 < kt1) gemm_tile8_body<true, true, float>(g, tm * 256, tn * 256, kt0, kt1, q.kt_per_split < nk, smem);
    } else {
        gemm_tile_body<256, 256, 128, 64, true, true, float, false, false, FASTK>(g, lg - q.start, q.kt_per_split < nk, smem);
    }
}


#ifdef OMLM_ISA_ONLY       /* tools/isa_audit.py-style inspection builds: the persistent kernels alone (seconds instead of minutes) */
template __global__ void gemm_bf16_tile_persist_kernel<256, 256, 128, 64, false, false, h16_t, false>(GemmArgs);
template __global__ void gemm_bf16_tile_persist_kernel<256, 256, 128, 64, false, true, h16_t, false>(GemmArgs);
template __global__ void gemm_bf16_tile_persist_kernel<256, 256, 128, 64, false, false, float, true>(GemmArgs);
template __global__ void gemm_bf16_tile_persist_kernel<256, 256, 128, 64, false, true, float, true>(GemmArgs);
template __global__ void gemm_bf16_tile_persist_kernel<128, 128, 64, 64, false, false, h16_t, false>(GemmArgs);
template __global__ void gemm_bf16_tile_persist_kernel<128, 128, 64, 64, false, false, float, true>(GemmArgs);
template __global__ void gemm_bf16_tile_persist_kernel<128, 128, 64, 64, false, false, h16_t, false, 1>(GemmArgs);
template __global__ void gemm_tile8_kernel<false, false, h16_t>(GemmArgs);
template __global__ void gemm_tile8_kernel<false, true, h16_t>(GemmArgs);
template __global__ void gemm_tile8_kernel<false, false, float>(GemmArgs);
template __global__ void gemm_tile8_kernel<true, true, float>(GemmArgs);
template __global__ void gemm_tile8_kernel<false, false, h16pl_t, true>(GemmArgs);      // the plane route of fp16ff: 3 products, planes out / fp32 out
template __global__ void gemm_tile8_kernel<false, false, float, true>(GemmArgs);
}   // namespace
#else
using namespace omlm_plan;         // csrc/gemm_plan.h: every route decision below is taken there
static_assert(BK == KT && BM == 128 && BN == 128 && NTHREADS == 256, "gemm_plan.h plans for these tiles");

// The CU count, queried once per copy of the library; the planners receive the two numbers as arguments.
static int gemm_cu_query() {
    static int cus = -1;
    if (cus < 0) {
        int dev = 0, n = 0;
        cus = (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 0;
    }
    return cus;
}
__attribute__((visibility("hidden"))) int gemm_ncu() { const int n = gemm_cu_query(); return n > 0 ? n : 256; }
// workgroups of the persistent walk: one per CU, rounded down to a multiple of 8 (the walk's stride must keep a workgroup on its XCD);
// 0 = none (fewer than 8 CUs, or the query failed)
__attribute__((visibility("hidden"))) int gemm_persist_slots() { const int n = gemm_cu_query(); return n >= 8 ? n / 8 * 8 : 0; }

static GemmArgs gemm_args() {      // every field zero / NULL (the three retired ones included), alpha = 1
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.alpha = 1.f;
    return g;
}

// one planned launch of the 16-bit tile kernels: the k-loop form
template <int BM_, int BN_, int WM_, int WN_, bool AK, bool BKM, typename TOUT>
static void launch_form(const GemmArgs& g, const GemmLaunch& l, hipStream_t st) {
    const dim3 grid(l.grid_x, l.grid_y), block(l.threads);
    switch (l.form) {
    case FORM_RING:
        if constexpr (BM_ == 256 && BN_ == 256) {
            if constexpr (!OMLM_FP16)
                if (g.split3) return launch_with_lds<gemm_tile8_kernel<AK, BKM, TOUT, true>>(grid, block, l.lds, st, g);
            return launch_with_lds<gemm_tile8_kernel<AK, BKM, TOUT>>(grid, block, l.lds, st, g);
        }
        return;
    case FORM_PERSIST:
        if constexpr (!AK && BM_ == BN_) {
            if (g.Cin) return launch_with_lds<gemm_bf16_tile_persist_kernel<BM_, BN_, WM_, WN_, false, BKM, TOUT, true>>(grid, block, l.lds, st, g);
            return launch_with_lds<gemm_bf16_tile_persist_kernel<BM_, BN_, WM_, WN_, false, BKM, TOUT, false>>(grid, block, l.lds, st, g);
        }
        return;
    case FORM_ROT_SPLIT3:           // (instantiated in the bf16 copy only)
        if constexpr (!OMLM_FP16) launch_with_lds<gemm_bf16_tile_kernel<BM_, BN_, WM_, WN_, AK, BKM, TOUT, false, true>>(grid, block, l.lds, st, g);
        return;
    case FORM_ROT_KMAP:  return launch_with_lds<gemm_bf16_tile_kernel<BM_, BN_, WM_, WN_, AK, BKM, TOUT, (AK || BKM) && BM_ == 128>>(grid, block, l.lds, st, g);
    case FORM_ROT_FASTK: return launch_with_lds<gemm_bf16_tile_kernel<BM_, BN_, WM_, WN_, AK, BKM, TOUT, false, false, true>>(grid, block, l.lds, st, g);
    default:             return launch_with_lds<gemm_bf16_tile_kernel<BM_, BN_, WM_, WN_, AK, BKM, TOUT, false>>(grid, block, l.lds, st, g);
    }
}

// ... on one tile: the operand layouts and the output type.  The hi/lo-plane route of omlm_gemm_planes16 (row-major A [M, K] and B [N, K]) is
// built in both copies of the file (TOUT: float, or h16pl_t = the result leaves as planes too).
template <int BM_, int BN_, int WM_, int WN_>
static void launch_tile(const GemmArgs& g, const GemmShape& s, const GemmLaunch& l, hipStream_t st) {
    if (s.planes16) {
        const dim3 grid(l.grid_x, l.grid_y), block(l.threads);
        if constexpr (BM_ == 256 && BN_ == 256) {
            if (l.form == FORM_RING) {
                if (g.C_lo) return launch_with_lds<gemm_tile8_kernel<false, false, h16pl_t, true>>(grid, block, l.lds, st, g);
                return launch_with_lds<gemm_tile8_kernel<false, false, float, true>>(grid, block, l.lds, st, g);
            }
        }
        if (g.C_lo) return launch_with_lds<gemm_bf16_tile_kernel<BM_, BN_, WM_, WN_, false, false, h16pl_t, false, true>>(grid, block, l.lds, st, g);
        return launch_with_lds<gemm_bf16_tile_kernel<BM_, BN_, WM_, WN_, false, false, float, false, true>>(grid, block, l.lds, st, g);
    }
    const bool f32 = s.out_dtype == 0;
    switch (2 * s.a_kmajor + s.b_kmajor) {
    case 0:  return f32 ? launch_form<BM_, BN_, WM_, WN_, false, false, float>(g, l, st) : launch_form<BM_, BN_, WM_, WN_, false, false, h16_t>(g, l, st);
    case 1:  return f32 ? launch_form<BM_, BN_, WM_, WN_, false, true, float>(g, l, st) : launch_form<BM_, BN_, WM_, WN_, false, true, h16_t>(g, l, st);
    case 3:  return f32 ? launch_form<BM_, BN_, WM_, WN_, true, true, float>(g, l, st) : launch_form<BM_, BN_, WM_, WN_, true, true, h16_t>(g, l, st);
    default: return f32 ? launch_form<BM_, BN_, WM_, WN_, true, false, float>(g, l, st) : launch_form<BM_, BN_, WM_, WN_, true, false, h16_t>(g, l, st);
    }
}

// ... of rows l.M of `g` (s: the shape the launch was planned for): the tile
static int launch_planned(GemmArgs g, const GemmShape& s, const GemmLaunch& l, hipStream_t st) {
    if (l.kmap_unbuilt) { omlm_set_error("omlm_gemm: k-row maps are only built for the 128x128 tile"); return OMLM_ERR_UNSUPPORTED; }
    g.kt_per_split = l.kt_per_split;
    switch (l.bm + l.bn) {
    case 512: launch_tile<256, 256, 128, 64>(g, s, l, st); break;
    case 384: launch_tile<256, 128, 64, 64>(g, s, l, st); break;
    default:  launch_tile<128, 128, 64, 64>(g, s, l, st); break;
    }
    return omlm_post_launch(s.planes16 ? "omlm_gemm_planes16" : "omlm_gemm");
}

// ---- the peeled tail as a deterministic split-K (round 5) -------------------------------------------------------------------------
// The m-tile rows behind the last full round of 256 x 256 tiles run on 128 x 128 tiles (gemm_plan): 48 ... 190 workgroups whose
// k-loops (86 k-tiles for d(xn2), 129 loop tiles for the FF-out plane route) are one serial chain each on a fraction of the machine
// (80 / 121 us for ~35 / ~50 us of work at the chip's rate).  With a workspace (a per-call argument: GemmCall::ws) the tail's K range is cut
// into S slices that fill the 2-per-CU slots, every slice STORES its fp32 partial tile to its own plane of the workspace (no atomics, no
// pre-filled C), and gemm_tail_reduce_kernel adds the planes in a fixed order together with the residual and writes the output type
// (fp32, 16-bit, or 16-bit hi/lo planes): deterministic, two launches.  The workspace belongs to the
// caller and to ONE stream at a time (the library keeps no pointer: two streams pass two buffers); OMLM_GEMM_TAIL_SPLIT=0 or no workspace keeps the one-launch tail.

// what a call says beside its GemmArgs.  dtype codes shared with the Python host: 0 = fp32, 1 = bf16
struct GemmCall {
    int a_kmajor, b_kmajor, in_dtype, out_dtype;
    bool planes16, qknorm;         // the omlm_gemm_planes16 route / omlm_gemm_qknorm (its own checks stand in for the ones below)
    void* ws; long long ws_bytes;  // tail workspace
    void* stream;
};

static int gemm_impl(GemmArgs g, const GemmCall& c) {
    const int M = g.M, N = g.N, K = g.K;
    if (M <= 0 || N <= 0) return OMLM_OK;
    hipStream_t st = as_stream(c.stream);
    const GemmHooks hooks = gemm_hooks_from_env();
    if (c.qknorm) {
        const GemmLaunch l = qknorm_plan(M, N, K, gemm_persist_slots(), hooks);
        g.kt_per_split = l.kt_per_split;
        const dim3 grid(l.grid_x, l.grid_y), block(l.threads);
        if (l.form == FORM_PERSIST)         launch_with_lds<gemm_bf16_tile_persist_kernel<128, 128, 64, 64, false, false, h16_t, false, 1>>(grid, block, l.lds, st, g);
        else if (l.form == FORM_ROT_FASTK)  launch_with_lds<gemm_bf16_tile_kernel<128, 128, 64, 64, false, false, h16_t, false, false, true, 1>>(grid, block, l.lds, st, g);
        else                                launch_with_lds<gemm_bf16_tile_kernel<128, 128, 64, 64, false, false, h16_t, false, false, false, 1>>(grid, block, l.lds, st, g);
        return omlm_post_launch("omlm_gemm_qknorm");
    }
    const void *A = g.A, *B = g.B, *C = g.C;
    const int lda = g.lda, ldb = g.ldb, a_kmajor = c.a_kmajor, b_kmajor = c.b_kmajor, in_dtype = c.in_dtype, out_dtype = c.out_dtype;
    const long long a_rows = g.a_rows, b_rows = g.b_rows;
    OMLM_CHECK_ARG(A && B && C, "null operand");
    OMLM_CHECK_ARG(K > 0, "K must be positive");
    OMLM_CHECK_ARG((lda % 8) == 0 && (ldb % 8) == 0, "operand leading dimensions must be multiples of 8 elements");
    OMLM_CHECK_ARG(((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0, "operands must be 16-byte aligned");
    OMLM_CHECK_ARG(in_dtype == 0 || in_dtype == 1, "in_dtype: 0=fp32 (bf16x3) or 1=bf16");
    OMLM_CHECK_ARG(out_dtype == 0 || out_dtype == 1, "out_dtype: 0=fp32 or 1=bf16");
    const size_t esz = in_dtype == 0 ? 4 : 2;
    OMLM_CHECK_ARG((unsigned long long)a_rows * lda * esz < 0xFFFFFFF0ull, "A exceeds the 4 GiB buffer-descriptor window");
    OMLM_CHECK_ARG((unsigned long long)b_rows * ldb * esz < 0xFFFFFFF0ull, "B exceeds the 4 GiB buffer-descriptor window");
    // contiguous dims are consumed in chunks of 8: a ragged contiguous extent must be zero-padded to 8 by the caller
    if (a_kmajor) OMLM_CHECK_ARG(lda >= ((M + 7) / 8) * 8, "k-major A: row pitch shorter than M padded to 8");
    if (b_kmajor) OMLM_CHECK_ARG(ldb >= ((N + 7) / 8) * 8, "k-major B: row pitch shorter than N padded to 8");
    if (!a_kmajor || !b_kmajor) OMLM_CHECK_ARG(K % 8 == 0, "k-contiguous operands need K % 8 == 0 (zero-pad the contraction)");
    GemmShape s;
    s.M = M; s.N = N; s.K = K; s.a_kmajor = a_kmajor != 0; s.b_kmajor = b_kmajor != 0; s.a_map = g.a_map != nullptr; s.b_map = g.b_map != nullptr;
    s.c_map = g.c_map != nullptr; s.in_dtype = in_dtype; s.out_dtype = out_dtype; s.split3 = g.split3 != 0; s.planes16 = c.planes16;
    s.fp16_copy = OMLM_FP16 != 0; s.accumulates = g.Cin == (const float*)C; s.cin = g.Cin != nullptr; s.alpha_one = g.alpha == 1.0f;
    s.ws_bytes = c.ws ? c.ws_bytes : 0;
    const GemmPlan p = gemm_plan(s, gemm_ncu(), gemm_persist_slots(), hooks);
#if !OMLM_FP16      /* (the fp16 copy is entered with its 16-bit operands only: gemm_to_fp16_copy) */
    if (in_dtype == 0) {
        OMLM_CHECK_ARG(out_dtype == 0, "fp32 operands produce fp32 output");
        const GemmLaunch& l = p.main;
        const dim3 grid(l.grid_x, l.grid_y), block(l.threads);
        g.kt_per_split = l.kt_per_split;
        switch (2 * a_kmajor + b_kmajor) {
        case 0:  launch_with_lds<gemm_kernel<float, false, false, float>>(grid, block, l.lds, st, g); break;
        case 1:  launch_with_lds<gemm_kernel<float, false, true, float>>(grid, block, l.lds, st, g); break;
        case 3:  launch_with_lds<gemm_kernel<float, true, true, float>>(grid, block, l.lds, st, g); break;
        default: launch_with_lds<gemm_kernel<float, true, false, float>>(grid, block, l.lds, st, g); break;
        }
        return omlm_post_launch("omlm_gemm");
    }
#endif
    if (p.M1 == 0) return launch_planned(g, s, p.main, st);
    GemmArgs g1, g2;
    peel_rows(g, p.M1, out_dtype == 0 ? 4 : 2, out_dtype == 0 ? 4 : 2, g1, g2);
    if (g.A_lo) g2.A_lo = (const char*)g.A_lo + (size_t)p.M1 * lda * 2;       // (the peel is for row-major A only)
    const int rc = launch_planned(g1, s, p.main, st);
    if (rc != OMLM_OK) return rc;
    if (p.tail_slices == 0) return launch_planned(g2, s, p.tail, st);
    GemmShape w = s;
    w.out_dtype = 0;
    const GemmArgs gw = slice_args(g2, c.ws);
    const int rc2 = launch_planned(gw, w, p.tail, st);
    if (rc2 != OMLM_OK) return rc2;
    const dim3 blocks(p.reduce_blocks), th(256);
    const float* ws = (const float*)c.ws;
    if (p.reduce_kind == 0)      hipLaunchKernelGGL(gemm_tail_reduce_kernel<0>, blocks, th, 0, st, ws, p.tail_slices, gw.c_split_stride, g2.M, N, gw.ldc, g2.C, nullptr, g.ldc, g2.Cin, g.ldcin);
    else if (p.reduce_kind == 2) hipLaunchKernelGGL(gemm_tail_reduce_kernel<2>, blocks, th, 0, st, ws, p.tail_slices, gw.c_split_stride, g2.M, N, gw.ldc, g2.C, g2.C_lo, g.ldc, g2.Cin, g.ldcin);
    else                         hipLaunchKernelGGL(gemm_tail_reduce_kernel<1>, blocks, th, 0, st, ws, p.tail_slices, gw.c_split_stride, g2.M, N, gw.ldc, g2.C, nullptr, g.ldc, g2.Cin, g.ldcin);
    return omlm_post_launch("omlm_gemm (tail reduce)");
}
// the grouped weight gradients of omlm_gemm_wgrad_group, in the 16-bit type of this copy
static int wgrad_group_here(const omlm_gemm_wgrad_desc* d, int count, int splits, void* stream) {
    const GemmHooks hooks = gemm_hooks_from_env();
    for (int base = 0; base < count; base += OMLM_GROUP_MAX) {
        const int n = count - base < OMLM_GROUP_MAX ? count - base : OMLM_GROUP_MAX;
        WgradDims dims[OMLM_GROUP_MAX];
        for (int i = 0; i < n; ++i) {
            const omlm_gemm_wgrad_desc& q = d[base + i];
            OMLM_CHECK_ARG(q.A && q.B && q.C && q.M > 0 && q.N > 0 && q.K > 0, "wgrad group: bad problem");
            OMLM_CHECK_ARG((q.lda % 8) == 0 && (q.ldb % 8) == 0 && q.lda >= ((q.M + 7) / 8) * 8 && q.ldb >= ((q.N + 7) / 8) * 8,
                           "wgrad group: k-major operand pitches must be multiples of 8 covering the padded extent");
            OMLM_CHECK_ARG(((uintptr_t)q.A % 16) == 0 && ((uintptr_t)q.B % 16) == 0, "wgrad group: operands must be 16-byte aligned");
            OMLM_CHECK_ARG((unsigned long long)q.K * q.lda * 2 < 0xFFFFFFF0ull && (unsigned long long)q.K * q.ldb * 2 < 0xFFFFFFF0ull,
                           "wgrad group: operand exceeds the 4 GiB buffer-descriptor window");
            dims[i] = WgradDims{q.M, q.N, q.K};
        }
        int ktps[OMLM_GROUP_MAX], start[OMLM_GROUP_MAX];
        const WgradPlan p = wgrad_group_plan(dims, n, splits, gemm_ncu(), hooks, ktps, start);
        GroupArgs ga;
        memset(&ga, 0, sizeof(ga));
        ga.n = n; ga.total = p.total;
        for (int i = 0; i < n; ++i) {
            const omlm_gemm_wgrad_desc& q = d[base + i];
            GroupProb& gp = ga.p[i];
            gp.A = q.A; gp.B = q.B; gp.C = q.C; gp.c_map = q.c_map; gp.M = q.M; gp.N = q.N; gp.K = q.K; gp.lda = q.lda; gp.ldb = q.ldb; gp.ldc = q.ldc;
            gp.kt_per_split = ktps[i]; gp.start = start[i];
        }
        const dim3 grid(p.total), block(512);
        if (p.form == FORM_RING)           launch_with_lds<gemm_wgrad_group_kernel<true, true>>(grid, block, 131072, as_stream(stream), ga);
        else if (p.form == FORM_ROT_FASTK) launch_with_lds<gemm_wgrad_group_kernel<true>>(grid, block, 131072, as_stream(stream), ga);
        else                               launch_with_lds<gemm_wgrad_group_kernel<false>>(grid, block, 131072, as_stream(stream), ga);
    }
    return omlm_post_launch("omlm_gemm_wgrad_group");
}

static_assert(sizeof(GemmArgs) == 208 && sizeof(GemmCall) == 48, "GemmArgs / GemmCall: one layout in both copies");
#if OMLM_FP16
// the fp16 copy has two ways in: a call the bf16 copy handed over (gemm_to_fp16_copy), and the descriptor array of a grouped one
extern "C" __attribute__((visibility("hidden"))) int omlm_gemm_run_h(const GemmArgs* g, const GemmCall* c) { return gemm_impl(*g, *c); }
extern "C" __attribute__((visibility("hidden"))) int omlm_gemm_wgrad_group_run_h(const omlm_gemm_wgrad_desc* d, int count, int splits, void* stream) {
    return wgrad_group_here(d, count, splits, stream);
}
#else
extern "C" int omlm_gemm_run_h(const GemmArgs* g, const GemmCall* c);
extern "C" int omlm_gemm_wgrad_group_run_h(const omlm_gemm_wgrad_desc* d, int count, int splits, void* stream);
static int gemm_run(const GemmArgs& g, GemmCall c) { return gemm_to_fp16_copy(c.in_dtype, c.out_dtype) ? omlm_gemm_run_h(&g, &c) : gemm_impl(g, c); }

// ---- the C entries (include/omlm.h).  dtype codes: 0 = fp32, 1 = bf16, 2 = fp16 --------------------------------------------------------------------
// Workspace of the peeled tail's deterministic split-K: a caller-owned scratch buffer handed to every call that may peel a tail (omlm_gemm,
// omlm_gemm_planes16, omlm_gemm_planes) -- ONE per stream that launches such GEMMs concurrently; NULL / 0: the one-launch tail.  The library keeps no
// pointer.  omlm_gemm_tail_workspace_bytes: an upper bound of what an M x N output needs (8 fp32 slices of the at most one-machine-round tail).
// (its CU query stays its own, uncached and with 256 only where the device query fails: folding it into gemm_ncu() could change its value there)
extern "C" long long omlm_gemm_tail_workspace_bytes(int M, int N) {
    int dev = 0, ncu = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    return gemm_tail_workspace_bytes(M, N, ncu);
}

#define OMLM_CHECK_TAIL_WS() OMLM_CHECK_ARG((workspace == nullptr) == (workspace_bytes == 0) && workspace_bytes >= 0 && ((uintptr_t)workspace % 16) == 0, \
                                            "tail workspace: 16-byte aligned buffer and its size, or NULL / 0")

// fp16 operands (with fp32 or fp16 output) are served by the fp16 copy of this file; bf16 and fp32 operands here.
extern "C" int omlm_gemm(const void* A, const void* B, void* C, const float* Cin,
                         const int* a_map, const int* b_map, const int* c_map,
                         long long a_rows, long long b_rows,
                         int M, int N, int K, int lda, int ldb, int ldc, int ldcin,
                         int a_kmajor, int b_kmajor, int in_dtype, int out_dtype, float alpha, void* workspace, long long workspace_bytes, void* stream) {
    if (in_dtype == OMLM_DT_F16) OMLM_CHECK_ARG(out_dtype == OMLM_DT_F32 || out_dtype == OMLM_DT_F16, "fp16 operands produce fp32 or fp16 output");
    OMLM_CHECK_TAIL_WS();
    GemmArgs g = gemm_args();
    g.A = A; g.B = B; g.C = C; g.Cin = Cin; g.a_map = a_map; g.b_map = b_map; g.c_map = c_map; g.a_rows = a_rows; g.b_rows = b_rows;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldcin = ldcin; g.alpha = alpha;
    return gemm_run(g, GemmCall{a_kmajor, b_kmajor, in_dtype, out_dtype, false, false, workspace, workspace_bytes, stream});
}

// q / k projections with the attention's l2-norm + learned scale folded into the epilogue (transformer.py:254-271): C = 16-bit
// [M, N] (+ C2 for columns >= c2_col0, e.g. v of the fused k | v projection), epi_groups leading 64-column heads normalised, their norms
// to norm_out [M, ldnorm] fp32 (what the backward needs instead of the fp32 pre-norm projections).  A [M, K], B [N, K] row-major 16-bit.
extern "C" int omlm_gemm_qknorm(const void* A, const void* B, void* C, void* C2, int c2_col0, int ldc2, const float* scale,
                                float* norm_out, int ldnorm, int groups, long long a_rows, long long b_rows, int M, int N, int K,
                                int lda, int ldb, int ldc, int dtype, void* stream) {
    if (M <= 0 || N <= 0) return OMLM_OK;
    OMLM_CHECK_ARG_AS(dtype == 1 || dtype == 2, "gemm_qknorm: operand dtype 1 (bf16) or 2 (fp16) [dtype == 1]");
    OMLM_CHECK_ARG(A && B && C && scale && norm_out && K > 0 && (K % 8) == 0, "gemm_qknorm: null operand / K");
    OMLM_CHECK_ARG((N % 64) == 0 && groups >= 0 && groups * 64 <= N && ldnorm >= groups, "gemm_qknorm: N must be whole 64-wide heads");
    OMLM_CHECK_ARG((lda % 8) == 0 && (ldb % 8) == 0 && (ldc % 8) == 0 && ((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0 && ((uintptr_t)C % 16) == 0,
                   "gemm_qknorm: 16-byte aligned operands, pitches multiples of 8");
    OMLM_CHECK_ARG(!C2 || ((c2_col0 % 64) == 0 && (ldc2 % 8) == 0 && ((uintptr_t)C2 % 16) == 0), "gemm_qknorm: second output");
    OMLM_CHECK_ARG((unsigned long long)a_rows * lda * 2 < 0xFFFFFFF0ull && (unsigned long long)b_rows * ldb * 2 < 0xFFFFFFF0ull, "operand exceeds the 4 GiB window");
    GemmArgs g = gemm_args();
    g.A = A; g.B = B; g.C = C; g.a_rows = a_rows; g.b_rows = b_rows; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    g.epi_scale = scale; g.epi_norm = norm_out; g.epi_groups = groups; g.epi_ldnorm = ldnorm; g.C2 = C2; g.c2_col0 = c2_col0; g.ldc2 = ldc2;
    return gemm_run(g, GemmCall{0, 0, dtype, dtype, false, true, nullptr, 0, stream});
}

// C = A B^T (+ Cin) with BOTH operands as hi/lo planes of the 16-bit type `dtype` (1 = bf16, 2 = fp16): A [M, K] and B [N, K] row-major with
// their lo planes A_lo / B_lo in the same layout (separate allocations are fine), three products hi*hi + hi*lo + lo*hi accumulated in fp32
// in ONE launch (3 x the k-tiles).  The result is fp32 (C_lo NULL; Cin optional), or -- C_lo given -- leaves as planes of the same type:
// C = rne16(v), C_lo = rne16(v - C), so that the next consumer reads the un-rounded value and a 16-bit backward reads C alone.
// Precision "fp16ff" (round 5): the two ConvFeedForward GEMMs of the forward, which carry 86-88 % of the fp16 logits-error variance
// (profiles/r05_error_budget.md).
extern "C" int omlm_gemm_planes16(const void* A, const void* A_lo, const void* B, const void* B_lo, void* C, void* C_lo, const float* Cin,
                                  const int* a_map, const int* c_map, long long a_rows, long long b_rows, int M, int N, int K,
                                  int lda, int ldb, int ldc, int ldcin, int dtype, void* workspace, long long workspace_bytes, void* stream) {
    OMLM_CHECK_TAIL_WS();
    OMLM_CHECK_ARG_AS(dtype == 1 || dtype == 2, "gemm_planes16: operand dtype 1 (bf16) or 2 (fp16) [dtype == 1]");
    OMLM_CHECK_ARG(A_lo && B_lo, "gemm_planes16: null lo plane");
    OMLM_CHECK_ARG(((uintptr_t)A_lo % 16) == 0 && ((uintptr_t)B_lo % 16) == 0 && ((uintptr_t)C_lo % 16) == 0, "gemm_planes16: 16-byte aligned planes");
    OMLM_CHECK_ARG(!(C_lo && Cin), "gemm_planes16: plane output takes no residual");
    // a_map / c_map (optional): physical row of logical row m in A (both planes) / in C and Cin, as in omlm_gemm -- the logit heads
    GemmArgs g = gemm_args();
    g.A = A; g.B = B; g.C = C; g.Cin = Cin; g.a_map = a_map; g.c_map = c_map; g.a_rows = a_rows; g.b_rows = b_rows;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldcin = ldcin;
    g.split3 = 1; g.A_lo = A_lo; g.B_lo = B_lo; g.C_lo = C_lo;
    return gemm_run(g, GemmCall{0, 0, dtype, C_lo ? dtype : 0, true, false, workspace, workspace_bytes, stream});
}

// fp32-grade GEMM on bf16 hi/lo planes ("bf16x3" through the LDS-DMA tile kernels).  A and B are bf16 hi planes in the layout
// omlm_gemm takes for bf16 operands; the matching lo plane lies a_plane_bytes / b_plane_bytes behind each (omlm_split_planes
// writes such a pair).  One launch whose k-loop is three times as long: hi*hi + hi*lo + lo*hi, accumulated in fp32 -- the same
// three products per element as the register-staged fp32 path (gemm_kernel<float>), at the bf16 kernels' rate.
extern "C" int omlm_gemm_planes(const void* A, long long a_plane_bytes, const void* B, long long b_plane_bytes, void* C, const float* Cin,
                                const int* a_map, const int* b_map, const int* c_map, long long a_rows, long long b_rows,
                                int M, int N, int K, int lda, int ldb, int ldc, int ldcin,
                                int a_kmajor, int b_kmajor, int out_dtype, float alpha, void* workspace, long long workspace_bytes, void* stream) {
    OMLM_CHECK_TAIL_WS();
    OMLM_CHECK_ARG(a_plane_bytes > 0 && b_plane_bytes > 0 && (a_plane_bytes % 16) == 0 && (b_plane_bytes % 16) == 0, "plane strides");
    OMLM_CHECK_ARG(!(a_kmajor && a_map) && !(b_kmajor && b_map), "k-row maps are not supported on operand planes");
    // each plane has its own buffer descriptor (round 5): the lo planes are addressed by pointer, not by an offset inside A's / B's window
    GemmArgs g = gemm_args();
    g.A = A; g.B = B; g.C = C; g.Cin = Cin; g.a_map = a_map; g.b_map = b_map; g.c_map = c_map; g.a_rows = a_rows; g.b_rows = b_rows;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldcin = ldcin; g.alpha = alpha;
    g.split3 = 1; g.A_lo = (const char*)A + a_plane_bytes; g.B_lo = (const char*)B + b_plane_bytes;
    return gemm_impl(g, GemmCall{a_kmajor, b_kmajor, 1, out_dtype, false, false, workspace, workspace_bytes, stream});
}

// x [n] fp32 -> planes: hi[i] = x truncated to bf16 at planes[i], lo[i] = RNE(x - hi) at planes[plane_elems + i]  (x ~= hi + lo to 2^-17)
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ x, unsigned short* __restrict__ planes,
                                                           long long n, long long plane_elems) {
    const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;
    const long long stride = (long long)gridDim.x * 256 * 8;
    for (long long i = i0; i < n; i += stride) {
        if (i + 8 <= n) {
            const float4 a = *(const float4*)(x + i), b = *(const float4*)(x + i + 4);
            unsigned h0, h1, h2, h3, l0, l1, l2, l3;
            split_pair(a.x, a.y, h0, l0); split_pair(a.z, a.w, h1, l1);
            split_pair(b.x, b.y, h2, l2); split_pair(b.z, b.w, h3, l3);
            u32x4 hi, lo;
            hi[0] = h0; hi[1] = h1; hi[2] = h2; hi[3] = h3; lo[0] = l0; lo[1] = l1; lo[2] = l2; lo[3] = l3;
            *(u32x4*)(planes + i) = hi;
            *(u32x4*)(planes + plane_elems + i) = lo;
        } else {
            for (long long j = i; j < n; ++j) {
                const unsigned u = f2u(x[j]) & 0xFFFF0000u;
                planes[j] = (unsigned short)(u >> 16);
                planes[plane_elems + j] = (unsigned short)bf16_bits_rne(x[j] - u2f(u));
            }
        }
    }
}
extern "C" int omlm_split_planes(const float* x, void* planes, long long n, long long plane_elems, void* stream) {
    if (n <= 0) return OMLM_OK;
    OMLM_CHECK_ARG(x && planes && plane_elems >= n && (plane_elems % 8) == 0, "split_planes arguments");
    OMLM_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)planes % 16) == 0, "split_planes: 16-byte aligned buffers");
    long long blocks = (n / 8 + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, (unsigned short*)planes, n, plane_elems);
    return omlm_post_launch("omlm_split_planes");
}

// C_i[M_i, N_i] += A_i^T B_i for `count` problems with 16-bit k-major operands A_i [K_i, M_i], B_i [K_i, N_i] in ONE launch of 256x256
// full-K (or lightly split) tiles.  splits: K-splits per tile for every problem (0 = chosen here for whole machine rounds);
// dtype: operand type of ALL problems (1 = bf16, 2 = fp16).
extern "C" int omlm_gemm_wgrad_group(const omlm_gemm_wgrad_desc* d, int count, int splits, int dtype, void* stream) {
    if (count <= 0) return OMLM_OK;
    OMLM_CHECK_ARG(d, "null descriptor array");
    OMLM_CHECK_ARG_AS(dtype == 1 || dtype == 2, "wgrad group: operand dtype must be 1 (bf16) or 2 (fp16) [dtype == 1]");
    int out_dtype = 0;        // (fp32 accumulation into C_i)
    return gemm_to_fp16_copy(dtype, out_dtype) ? omlm_gemm_wgrad_group_run_h(d, count, splits, stream) : wgrad_group_here(d, count, splits, stream);
}
#endif

}   // namespace OMLM_NS
#endif   // OMLM_ISA_ONLY
