// Attention backward, dK / dV (transformer.py:303-331 autograd), third generation for 16-bit operands.
//
// What the counters said about the second-generation kernel (attention.hip: attn_bwd_dkv_kernel, profiles/r03a_attn_bwd_pmc.md:
// 323 us per layer at B = 32, N = 1116, H = 8 -- 55 % of the whole attention backward, 44 % of its wave-cycles parked in waits,
// 1.73 M vector-memory instructions): a workgroup owned ONE 32-key tile and each of its waves fetched the Q / dO tile of its own
// (query tile, head) item straight into MFMA fragments -- 32 rows x 32 bytes per load instruction (every instruction touches 32
// cache lines and uses a quarter of each), and every Q / dO tile of a sample travelled L2 -> CU once per 32-key tile: 1.3 GB per
// layer.  Here
//   * a workgroup owns 128 keys = 4 waves x 32 keys, and ALL its waves work on the SAME item: the item's Q and dO tiles
//     ([32 queries][64 dims]) are staged ONCE per workgroup by LDS-DMA (global_load_lds_dwordx4, 16 rows x 64 bytes per wave
//     instruction, straight into the blocked image the transpose reads want) into a 3-stage ring, two items ahead of the matrix
//     cores, one barrier per item -- a quarter of the L2 -> CU bytes, no VGPR staging, no per-item ds_write pass;
//   * lse / delta / the 63-value bias window of an item arrive the same way (two small DMA pieces per wave);
//   * a key range's items are cut into chunks of CH query tiles so that ~3 workgroups per CU exist and the longest one is short;
//     the chunks of a range add their dK / dV with fp32 atomics (64 KiB per workgroup, ~45 MB per layer) into zero-filled
//     outputs -- each wave owns its 32 keys, so there is no cross-wave reduction at all.
// Per element the arithmetic is the second generation's (same exponent form against the prepared table, same roundings).
#include "common.h"
#include "attn_plan.h"
#include <stdlib.h>

namespace OMLM_NS {

#define A3_T 256
#define A3_KR 128                      /* keys per workgroup */
#define A3_NST 3
#define A3_AUX 2048                    /* per-wave aux piece: [0,1024) window DMA (window 256 B | table tail 16 B | filler), [1024,1280) lse | delta */
#define A3_IMG (4096 + 256)            /* one [32][64] blocked image: the units of rows 16..31 sit 128 bytes further (see a3_blk_off) */
#define A3_STAGE (2 * A3_IMG + 4 * A3_AUX)
#define A3_NEG (-1.0e30f)
#define A3_LOG2E 1.4426950408889634f
#define A3_PAD 64                      /* zero entries in front of each row of the prepared bias table (attention2.hip: A2_PAD) */
static_assert(A3_PAD == omlm_plan::ATTN_PAD && A3_KR == omlm_plan::A3_KEYS && A3_NST * A3_STAGE == omlm_plan::A3_LDS,
              "attn_plan.h states the prepared table's layout, the keys per workgroup and the ring");

__device__ __forceinline__ int a3_crow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// blocked image of a [32 rows][64 cols] 16-bit tile (attention.hip: tile_off_blk): 1-KiB units (row / 16, col / 32), 128-byte blocks of
// [4 rows][16 cols] ordered for ds_read_b64_tr_b16
__device__ __forceinline__ int a3_blk_off(int row, int colbyte) {
    const int col = colbyte >> 1;
    const int rq = (row >> 2) & 3;
    const int p = ((rq >> 1) << 2) | ((rq & 1) << 1) | ((col >> 4) & 1);
    // + 128 bytes for rows 16..31: a 16-lane group of a row-fragment ds_read_b128 holds two row quads of each half, and with all units on
    // 1-KiB boundaries the four quads met on the same 32 banks (4-way conflict, SQ_LDS_BANK_CONFLICT 8 % of the kernel's wave-cycles);
    // shifted, the two halves use disjoint bank halves (2-way, the best this image allows: tools/lds_conflicts.py model)
    return (((row >> 4) << 1) + (col >> 5)) * 1024 + (row >> 4) * 128 + p * 128 + (row & 3) * 32 + (col & 15) * 2;
}
// A-operand row fragment (row = row0 + (lane & 31), dims 16 s + 8 (lane >> 5) .. +7) out of the blocked image
__device__ __forceinline__ h16x8 a3_frag_rows(const char* lds, int s, int lane) {
    return *(const h16x8*)(lds + a3_blk_off(lane & 31, (2 * s + (lane >> 5)) * 16));
}
// transposed operand: lane gets column col0 + (lane & 31) and the 8 rows MFMA k-index 8 (lane >> 5) + e maps to (accumulator row order)
__device__ __forceinline__ h16x8 a3_frag_cols_tr(const char* lds, int s, int col0, int lane) {
    const char* base = lds + ((s << 1) + (col0 >> 5)) * 1024 + s * 128 + lane * 8;
    s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, base));
    s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, base + 512));
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    s16x8 v = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(h16x8, v);
}
__device__ __forceinline__ h16x8 a3_pack(const f32x16& p, int s) {
    u32x4 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = pack_h16_rne(p[8 * s + 2 * e], p[8 * s + 2 * e + 1]);
    return __builtin_bit_cast(h16x8, h);
}

// LDS-DMA with per-lane 64-bit source addresses (any mix of buffers in one instruction); destination = M0 + lane * size.
// Inline asm: invisible to hipcc's vmcnt bookkeeping (attention2.hip explains why that is wanted); ordering is by the counted waits below.
// (M0 is written and read inside the one statement and declared clobbered: nothing else in this kernel uses it)
__device__ __forceinline__ void a3_dma16(const void* gsrc, unsigned lds_dst) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" :: "v"(gsrc), "s"(lds_dst) : "memory", "m0");
}
// the same with a wave-uniform base and a per-lane 32-bit byte offset (no 64-bit address arithmetic per item)
__device__ __forceinline__ void a3_dma16s(const void* sbase, unsigned voff, unsigned lds_dst) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voff), "s"(sbase), "s"(lds_dst) : "memory", "m0");
}
__device__ __forceinline__ void a3_dma4(const void* gsrc, unsigned lds_dst) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" :: "v"(gsrc), "s"(lds_dst) : "memory", "m0");
}

// grid: B x (workgroups per sample); a sample's workgroups walk its key ranges r = 0, 1, ... (128 keys each), range r being cut into
// ceil((nqt - 4 r) / CH) chunks of CH query tiles.
#ifndef A3_WAVES
#define A3_WAVES 2                     /* waves per SIMD the register allocation aims at */
#endif
// PFX: the non-causal prefix of Pn = min(P, N) rows.  A key range r with 128 r < Pn walks the query tiles from 0 instead of 4 r (its chunks
// are counted by a3_range_start in the launch's work split too); items above the diagonal keep (i, j) iff i, j < Pn; the prepared table
// holds off = Pn - 1 negative distances in front of the causal layout, so every window offset moves by off.
using omlm_plan::a3_range_start;
#define A3_KERNEL attn3_bwd_dkv_kernel
#define A3_PART false
#define A3_PART_ARG
#define A3_PART_PTR ((float*)nullptr)
#include "attention3_dkv.inc"
#undef A3_KERNEL
#undef A3_PART
#undef A3_PART_ARG
#undef A3_PART_PTR
#define A3_KERNEL attn3_bwd_dkv_part_kernel
#define A3_PART true
#define A3_PART_ARG , float* __restrict__ part
#define A3_PART_PTR part
#include "attention3_dkv.inc"
#undef A3_KERNEL
#undef A3_PART
#undef A3_PART_ARG
#undef A3_PART_PTR

// dK / dV from the slots of attn3_bwd_dkv_part_kernel: workgroup (r, b, which) owns the [128 keys][64] block of key range r and adds the
// range's ceil((nqt - 4 r) / CH) slots in chunk order (a sample's slots are laid out range by range, chunk by chunk: the kernel's own scan).
__global__ __launch_bounds__(256) void a3_part_reduce_kernel(const float* __restrict__ part, float* __restrict__ dk, float* __restrict__ dv,
                                                             int N, int CH, int wg_per_sample) {
    const int r = blockIdx.x, b = blockIdx.y, which = blockIdx.z;
    const int nqt = (N + 31) / 32;
    int first = 0;
    for (int rr = 0; rr < r; ++rr) first += (nqt - 4 * rr + CH - 1) / CH;
    const int nch = (nqt - 4 * r + CH - 1) / CH;
    const float* src = part + (((size_t)b * wg_per_sample + first) * 2 + which) * (A3_KR * 64);
    float* dst = (which == 0 ? dk : dv) + ((size_t)b * N + (size_t)r * A3_KR) * 64;
    for (int e4 = threadIdx.x; e4 < A3_KR * 64 / 4; e4 += 256) {
        if (r * A3_KR + (e4 >> 4) >= N) break;                // rows past N (e4 ascends with the row)
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int c = 0; c < nch; ++c) {
            const float4 x = *(const float4*)(src + (size_t)c * (2 * A3_KR * 64) + 4 * e4);
            a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
        }
        *(float4*)(dst + 4 * e4) = a;
    }
}

__global__ __launch_bounds__(256) void a3_zero_kernel(float4* __restrict__ p, size_t n4) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) p[i] = z;
}

// One launch of the plan's dK / dV part: the zero fill(s) and the kernel that adds into them with atomics, or (N > 4096 with a workspace,
// causal) the slot form and the sums of its slots in a fixed order.
// Zero fill by a KERNEL of this library, not hipMemsetAsync: as a memset node of a captured micro-step the fill detached everything
// behind it from the graph's completion -- the rest of the backward (this layer's dK / dV onwards) was still running when the launch
// had "finished" and the optimizer's kernels started (round 4: after one fp16 overflow the skipped step's gradient clear raced with
// those late writes and every later step stayed non-finite; no memset node, or a host sync after the replay, cured it).  A kernel node is ordered like every other launch.
void attn3_bwd_dkv_launch(const omlm_plan::AttnLaunch& l, int ldT, const void* q, const void* k, const void* v, const float* biasT,
                          const unsigned char* keymask, const void* dout, const float* lse, const float* delta, float* dk, float* dv,
                          int B, int N, int H, float scale, hipStream_t st, const AttnDrop& dr, int Pn, float* part) {
    const dim3 grid(l.gx, l.gy, l.gz), block(l.threads);
    auto go = [&](auto launch, auto... tail) {
        launch(grid, block, l.lds, st, (const h16_t*)q, (const h16_t*)k, (const h16_t*)v, keymask, (const h16_t*)dout, lse, delta, dk, dv, biasT,
               ldT, B, N, H, scale, l.CH, l.wps, dr, Pn, tail...);
    };
    if (l.family == omlm_plan::ATTN_A3_ZERO)                   // (l.floats: a multiple of 4; rows are 256-byte aligned)
        hipLaunchKernelGGL(a3_zero_kernel, grid, block, 0, st, (float4*)(l.which ? dv : dk), (size_t)(l.floats / 4));
    else if (l.family == omlm_plan::ATTN_A3_REDUCE)
        hipLaunchKernelGGL(a3_part_reduce_kernel, grid, block, 0, st, part, dk, dv, N, l.CH, l.wps);
    else if (l.form == omlm_plan::ATTN_FORM_PART) {
        if (l.drop) go([](auto... a) { launch_lds_cap<attn3_bwd_dkv_part_kernel<true>>(a...); }, part);
        else go([](auto... a) { launch_lds_cap<attn3_bwd_dkv_part_kernel<false>>(a...); }, part);
    } else
        with_flags(l.drop, l.pfx, [&](auto D, auto P) {
            go([](auto... a) { launch_lds_cap<attn3_bwd_dkv_kernel<decltype(D)::value, decltype(P)::value>>(a...); });
        });
}

}   // namespace OMLM_NS
