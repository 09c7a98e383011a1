// Causal multi-query attention of the reference trunk (transformer.py:254-331, non-xformers branch),
// flash-style: the [B, H, N, N] score / bias / mask tensors of the reference are never materialised.
//
//   sim[b,h,i,j] = 8 * <q[b,i,h,:], k[b,j,:]> + bias[h, i-j]        (one shared K/V head: MQA, :203-204)
//   masked (key mask, j > i)  -> excluded (reference fills -finfo.max; with >= 1 live key per row, which
//                                the wrapper guarantees since position 0 is never masked, that is identical)
//   out[b,i,h,:] = softmax_j(sim) @ v[b,j,:]
//
// MI355X mapping
//   * everything is computed transposed -- S^T = K Q^T, O^T = V^T P^T -- so that after the MFMA a lane
//     owns ONE query (column = lane & 31) and 16 keys: running max / sum / rescale are lane-local, and the
//     fp32 S^T accumulator registers are, after exp2 and bf16 packing, directly the B operand of the
//     second MFMA (no cross-lane shuffle, no LDS round trip for P).
//   * K/V tiles (64 keys x 64 dims) are staged once per workgroup in LDS and shared by the workgroup's
//     4 waves = 4 heads (the MQA reuse); V^T and K^T operands come from the same row-major tiles through
//     the hardware transpose read ds_read_b64_tr_b16.
//   * rel-pos bias is a 1-D table [H, N] (i - j >= 0) staged in LDS (pre-multiplied by log2 e), instead of
//     the reference's [H, N, N] gather; its gradient is reduced in LDS and flushed with one atomic per bin.
//   * T = float inputs select the bf16x3 split (hi*hi + hi*lo + lo*hi) for the forward; the backward
//     kernels always run single-pass bf16 MFMA with fp32 accumulation.
#include "common.h"
#include "attn_plan.h"
#include <stdlib.h>

namespace OMLM_NS {

#define AT_THREADS 256
#define TQ 32
#define TKV 64
#define NEG_BIG (-1.0e30f)
#define LOG2E 1.4426950408889634f

// [rows][64 dims] bf16 tile, 128 B per row; 16-B chunk index XOR ((row >> 1) & 7)
__device__ __forceinline__ int tile_off(int row, int colbyte) {
    return row * 128 + ((((colbyte >> 4) ^ ((row >> 1) & 7)) << 4) | (colbyte & 15));
}

// Blocked image of a [rows][64 dims] tile for the TRANSPOSE read: ds_read_b64_tr_b16 serves a [4 row][16 col] block
// (128 B) per 16-lane group; blocks are ordered so that a wave's four groups read 512 contiguous bytes
// (address = unit base + 8 * lane): unit = (row / 16, col / 32) -> 1 KiB; block p = r*4 + hi*2 + cc with
// (row / 4) & 3 = 2 r + hi (accumulator-row order: read r covers rows +8r, half-wave hi rows +4hi), cc = (col/16) & 1.
__device__ __forceinline__ int tile_off_blk(int row, int colbyte) {
    const int col = colbyte >> 1;
    const int rq = (row >> 2) & 3;
    const int p = ((rq >> 1) << 2) | ((rq & 1) << 1) | ((col >> 4) & 1);
    return (((row >> 4) << 1) + (col >> 5)) * 1024 + p * 128 + (row & 3) * 32 + (col & 15) * 2;
}

// key row held in accumulator register r of a 32x32 MFMA result for half-wave hi
__device__ __forceinline__ int crow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// ---- global -> register fragment: 8 consecutive elements of one row as bf16 (hi, optional lo) -------------
template <typename T, bool PRECISE>
__device__ __forceinline__ void load_row8(const T* p, bool ok, h16x8& hi, h16x8& lo);

template <>
__device__ __forceinline__ void load_row8<h16_t, false>(const h16_t* p, bool ok, h16x8& hi, h16x8& lo) {
    u32x4 z = {0u, 0u, 0u, 0u};
    u32x4 v = ok ? *(const u32x4*)p : z;
    hi = __builtin_bit_cast(h16x8, v);
}
template <>
__device__ __forceinline__ void load_row8<float, false>(const float* p, bool ok, h16x8& hi, h16x8& lo) {
    float4 a = make_float4(0, 0, 0, 0), b = a;
    if (ok) { a = ((const float4*)p)[0]; b = ((const float4*)p)[1]; }
    u32x4 v;
    v[0] = pack_h16_rne(a.x, a.y); v[1] = pack_h16_rne(a.z, a.w);
    v[2] = pack_h16_rne(b.x, b.y); v[3] = pack_h16_rne(b.z, b.w);
    hi = __builtin_bit_cast(h16x8, v);
}
template <>
__device__ __forceinline__ void load_row8<float, true>(const float* p, bool ok, h16x8& hi, h16x8& lo) {
    float4 a = make_float4(0, 0, 0, 0), b = a;
    if (ok) { a = ((const float4*)p)[0]; b = ((const float4*)p)[1]; }
    u32x4 h, l;
    unsigned h0, l0;
    split_pair(a.x, a.y, h0, l0); h[0] = h0; l[0] = l0;
    split_pair(a.z, a.w, h0, l0); h[1] = h0; l[1] = l0;
    split_pair(b.x, b.y, h0, l0); h[2] = h0; l[2] = l0;
    split_pair(b.z, b.w, h0, l0); h[3] = h0; l[3] = l0;
    hi = __builtin_bit_cast(h16x8, h);
    lo = __builtin_bit_cast(h16x8, l);
}

// K/V tile staging, split in two so the HBM latency of tile t+1 hides under the MFMA phase of tile t (guide T14):
// (1) global -> registers (issued before the compute phase), (2) registers -> swizzled LDS image after the barrier.
// A [TKV keys][64] tile is 512 chunks of 8 dims = 2 per thread; rows beyond N are zero.
template <typename T, bool PRECISE>
struct KVRegs {
    h16x8 hi[2], lo[2];
    __device__ __forceinline__ void load(const T* base /* row 0 of this sample, ld 64 */, int j0, int N) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = threadIdx.x + AT_THREADS * i;
            const int row = c >> 3, ch = c & 7;
            load_row8<T, PRECISE>(base + (size_t)(j0 + row) * 64 + ch * 8, (j0 + row) < N, hi[i], lo[i]);
        }
    }
    __device__ __forceinline__ void store(char* lds_hi, char* lds_lo) const {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = threadIdx.x + AT_THREADS * i;
            const int row = c >> 3, ch = c & 7;
            *(h16x8*)(lds_hi + tile_off(row, ch * 16)) = hi[i];
            if (PRECISE) *(h16x8*)(lds_lo + tile_off(row, ch * 16)) = lo[i];
        }
    }
    __device__ __forceinline__ void store_blk_hi(char* lds_hi) const {                 // blocked image of the hi plane only
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = threadIdx.x + AT_THREADS * i;
            *(h16x8*)(lds_hi + tile_off_blk(c >> 3, (c & 7) * 16)) = hi[i];
        }
    }
    __device__ __forceinline__ void store_blk(char* lds_hi, char* lds_lo) const {      // image for frag_cols_tr
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = threadIdx.x + AT_THREADS * i;
            const int row = c >> 3, ch = c & 7;
            *(h16x8*)(lds_hi + tile_off_blk(row, ch * 16)) = hi[i];
            if (PRECISE) *(h16x8*)(lds_lo + tile_off_blk(row, ch * 16)) = lo[i];
        }
    }
};

// normal operand fragment: row = row0 + (lane & 31), dims 16 s + 8 (lane >> 5) .. +7
__device__ __forceinline__ h16x8 frag_rows(const char* lds, int row0, int s, int lane) {
    return *(const h16x8*)(lds + tile_off(row0 + (lane & 31), (2 * s + (lane >> 5)) * 16));
}
// transposed operand fragment from a [rows][64] tile: lane gets column (col0 + (lane & 31)) and the 8 tile rows
// that MFMA k-index 8*(lane>>5)+e maps to under the accumulator row order:  row0 + 16 s + 8 (e>>2) + 4 (lane>>5) + (e&3)
__device__ __forceinline__ h16x8 frag_cols_tr(const char* lds, int row0, int s, int col0, int lane) {
    // blocked image (tile_off_blk): both reads are linear in the lane id
    const char* base = lds + ((((row0 >> 4) + s) << 1) + (col0 >> 5)) * 1024 + lane * 8;
    s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, base));
    s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, base + 512));
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    s16x8 v = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(h16x8, v);
}

#define MFMA(a, b, c) OMLM_MFMA_32x32x16(a, b, c)

// pack accumulator registers 8s..8s+7 into a bf16 B-operand (RNE), optional residual (lo) operand
template <bool PRECISE>
__device__ __forceinline__ void pack_acc(const f32x16& p, int s, h16x8& hi, h16x8& lo) {
    u32x4 h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float a = p[8 * s + 2 * e], b = p[8 * s + 2 * e + 1];
        if (PRECISE) { unsigned hh, ll; split_pair(a, b, hh, ll); h[e] = hh; l[e] = ll; }
        else h[e] = pack_h16_rne(a, b);
    }
    hi = __builtin_bit_cast(h16x8, h);
    if (PRECISE) lo = __builtin_bit_cast(h16x8, l);
}

// =============================================================================================================
// forward
// =============================================================================================================
// Lean inner loops (forward, the mask / bias part of the dQ kernel, the score loop of the dK/dV kernel; round 2: parity tests
// identical, forward 206 -> 145 us, backward 694 -> 643 us per layer).  The ISA of the straightforward forward showed ~400 VALU
// instructions per 8 MFMAs (one 32-key subtile), i.e. the kernel was VALU-bound 3:1.  The lean form removes, without changing
// a single result bit except where noted:
//   * 80 v_accvgpr_read/write per subtile: without an occupancy hint hipcc keeps the accumulators in AGPRs and copies them out
//     and back for the alpha rescale and the softmax -> amdgpu_waves_per_eu(2) (VGPR-form MFMA, as in the backward kernels);
//   * the rescale itself when no lane's running max moved (alpha == 1 for the whole wave: multiplying by 1.0 is exact);
//   * exp2f's denormal-range fix-up (v_ldexp + compare + select per score) -> raw v_exp_f32: differs only for results < 2^-126,
//     which only masked scores reach (they are 0 either way);
//   * on subtiles entirely below the diagonal (all but one per query tile): the causal compare, the clamp of the bias index and
//     the per-score address arithmetic (constant LDS offsets from one base), and the 64-bit mask-bit test (one 32-bit word).
#define AT_DQ_WPE 2        /* waves per SIMD the backward kernels are compiled for (2 = 256 registers) */
#define AT_DQP_WPE 2
#define AT_DKV_WPE 2
// PFX: the non-causal prefix (include/omlm.h): score (i, j) is live iff j <= i or (i < P and j < P), P = Pn = min(P, N) > 0.  bias points
// at the table's rel = 0 row; rows rel = -(Pn - 1) .. -1 precede it.  The wave's LDS bias table covers rel in [-(Pn - 1), nb) (index
// rel + off, off = Pn - 1), and a query tile with i0 < Pn walks its keys up to max(i0 + TQ, Pn).  PFX = false is the causal kernel as it was.
template <typename T, bool DROP = false, bool PFX = false>
__global__ __launch_bounds__(AT_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void attn_fwd_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                              const T* __restrict__ v, const float* __restrict__ bias,
                                                              const unsigned char* __restrict__ keymask, T* __restrict__ out,
                                                              float* __restrict__ lse, int B, int N, int H, float scale, int bias_ld,
                                                              const AttnDrop drop, int Pn) {
    constexpr bool PRECISE = elt_traits<T>::precise;
    constexpr int PLANE = TKV * 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Kh = smem;
    char* Vh = smem + PLANE;
    char* Kl = smem + 2 * PLANE;
    char* Vl = smem + 3 * PLANE;
    float* bias_l = (float*)(smem + (PRECISE ? 4 : 2) * PLANE);   // [4 waves][nb]

    const int nqt = (N + TQ - 1) / TQ;
    const int qt = nqt - 1 - (int)blockIdx.x;          // heavy (late) query tiles first
    const int b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hi = lane >> 5;
    const int h = blockIdx.y * 4 + wave;
    const bool active = h < H;
    const int i0 = qt * TQ;
    const int qi = i0 + (lane & 31);
    const int nb = i0 + TQ;                             // bias bins needed: rel in [0, i0 + 31]
    const size_t rowbase = (size_t)b * N;
    const int off = PFX ? Pn - 1 : 0;                   // PFX: negative-distance bins in front
    const int kend = PFX && i0 < Pn ? max(i0 + TQ, Pn) : i0 + TQ;      // keys [0, kend) can be live for this tile

    if (active) {
        float* bl = bias_l + (size_t)wave * (nb + off);
        if (PFX) {
            for (int r = lane; r < nb + off; r += 64) bl[r] = bias ? bias[(ptrdiff_t)min(r - off, N - 1) * bias_ld + h] * LOG2E : 0.f;
        } else {
            for (int r = lane; r < nb; r += 64) bl[r] = bias ? bias[(size_t)min(r, N - 1) * bias_ld + h] * LOG2E : 0.f;
        }
    }
    h16x8 qh[4], ql[4];
    if (active) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
            load_row8<T, PRECISE>(q + (rowbase + min(qi, N - 1)) * (size_t)(H * 64) + h * 64 + 16 * s + 8 * hi, qi < N, qh[s], ql[s]);
    }
    f32x16 acc[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; }
    float m = NEG_BIG, lsum = 0.f;
    const float c = scale * LOG2E;
    const float* bl = bias_l + (size_t)wave * (nb + off) + off;
    // DROP: row key of (b, h, qi) with this half-wave's key bit 4 hi / 2 (common.h); the pair (r, r + 1), r even, is keys j, j + 1
    const unsigned rk = DROP ? attn_drop_headkey(attn_drop_seed(drop), b, active ? h : 0) ^ ((unsigned)qi << 15) ^ (2u * (unsigned)hi) : 0u;

    const int nkt = (kend + TKV - 1) / TKV;
    KVRegs<T, PRECISE> kr, vr;
    kr.load(k + rowbase * 64, 0, N);
    vr.load(v + rowbase * 64, 0, N);
    for (int kt = 0; kt < nkt; ++kt) {
        const int j0 = kt * TKV;
        __syncthreads();
        kr.store(Kh, Kl);
        vr.store_blk(Vh, Vl);
        const int jk = j0 + lane;
        const bool live = jk < N && (keymask ? keymask[rowbase + jk] != 0 : true);
        const unsigned long long bits = __ballot(live);
        __syncthreads();
        if (kt + 1 < nkt) {                    // in flight during this tile's MFMA phase
            kr.load(k + rowbase * 64, j0 + TKV, N);
            vr.load(v + rowbase * 64, j0 + TKV, N);
        }
        if (!active) continue;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int jb = j0 + 32 * sub;
            if (jb > kend - 1) break;
            f32x16 st;
#pragma unroll
            for (int e = 0; e < 16; ++e) st[e] = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const h16x8 ka = frag_rows(Kh, 32 * sub, s, lane);
                if (PRECISE) {
                    const h16x8 kla = frag_rows(Kl, 32 * sub, s, lane);
                    st = MFMA(kla, qh[s], st);
                    st = MFMA(ka, ql[s], st);
                }
                st = MFMA(ka, qh[s], st);
            }
            float mloc = NEG_BIG;
            if (jb + 31 <= i0) {
                // every key of the subtile precedes every query of the wave: 0 <= rel = qi - key < nb without a test
                const unsigned w32 = (unsigned)(bits >> (32 * sub)) >> (4 * hi);
                const float* bp = bl + (qi - jb - 4 * hi);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int cr = (r & 3) + 8 * (r >> 2);                 // crow(r, hi) - 4 hi, a compile-time constant
                    const float val = st[r] * c + bp[-cr];
                    st[r] = ((w32 >> cr) & 1u) ? val : NEG_BIG;
                    mloc = fmaxf(mloc, st[r]);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kr = 32 * sub + crow(r, hi);
                    const int key = j0 + kr;
                    const int rel = qi - key;
                    const bool ok = (rel >= 0 || (PFX && qi < Pn && key < Pn)) && ((bits >> kr) & 1ull);
                    const float val = st[r] * c + bl[max(min(rel, nb - 1), -off)];
                    st[r] = ok ? val : NEG_BIG;
                    mloc = fmaxf(mloc, st[r]);
                }
            }
            mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
            const float mnew = fmaxf(m, mloc);
            const float alpha = __builtin_amdgcn_exp2f(m - mnew);
            m = mnew;
            float psum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { st[r] = __builtin_amdgcn_exp2f(st[r] - mnew); psum += st[r]; }
            lsum = lsum * alpha + psum;
            if (DROP) {                        // the denominator took every P; the numerator takes P Z (1 / (1 - p) at the store)
                const unsigned kb = rk ^ (unsigned)(jb >> 1);
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const unsigned w = omlm_hash32(kb ^ (unsigned)(((r & 3) + 8 * (r >> 2)) >> 1));
                    st[r] = (w << 16) >= drop.thr16 ? st[r] : 0.f;
                    st[r + 1] = w >= drop.thr16 ? st[r + 1] : 0.f;
                }
            }
            if (!__all(alpha == 1.0f)) {
#pragma unroll
                for (int e = 0; e < 16; ++e) { acc[0][e] *= alpha; acc[1][e] *= alpha; }
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                h16x8 ph, pl;
                pack_acc<PRECISE>(st, s, ph, pl);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const h16x8 va = frag_cols_tr(Vh, 32 * sub, s, 32 * dt, lane);
                    if (PRECISE) {
                        const h16x8 vla = frag_cols_tr(Vl, 32 * sub, s, 32 * dt, lane);
                        acc[dt] = MFMA(vla, ph, acc[dt]);
                        acc[dt] = MFMA(va, pl, acc[dt]);
                    }
                    acc[dt] = MFMA(va, ph, acc[dt]);
                }
            }
        }
    }
    if (!active || qi >= N) return;
    lsum += __shfl_xor(lsum, 32, 64);
    // a query without any live key (include/omlm.h): m never left NEG_BIG, every visited score counted as exp2(0) and acc holds a plain
    // average of the visited V rows -- emit zeros and the lse that zeroes its backward, as attention2.hip's forward does
    const bool seen = m > NEG_BIG;                  // (both half-waves hold the same m)
    const float inv = seen ? (DROP ? drop.rs : 1.0f) / lsum : 0.f;
    T* orow = out + (rowbase + qi) * (size_t)(H * 64) + h * 64;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d = 32 * dt + 8 * g4 + 4 * hi;
            store4_from_float(orow + d, acc[dt][4 * g4] * inv, acc[dt][4 * g4 + 1] * inv, acc[dt][4 * g4 + 2] * inv, acc[dt][4 * g4 + 3] * inv);
        }
    if (hi == 0 && lse) lse[((size_t)b * H + h) * N + qi] = seen ? m + log2f(lsum) : 1.0e30f;   // log2 domain (DROP: the same value)
}

// =============================================================================================================
// backward, kernel B: dQ, d(bias table), delta_i = sum_d dO[i,d] O[i,d]     (same geometry as the forward)
// =============================================================================================================
// PFX: the non-causal prefix, as in the forward; the d(bias) bins of negative distances (rel >= -(Pn - 1)) sit in front of the others and
// leave by atomics into dbias (which points at the rel = 0 row), the others as before.
template <typename T, bool DROP = false, bool PFX = false>
__global__ __launch_bounds__(AT_THREADS) __attribute__((amdgpu_waves_per_eu(AT_DQ_WPE))) void attn_bwd_dq_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                 const T* __restrict__ v, const float* __restrict__ bias,
                                                                 const unsigned char* __restrict__ keymask,
                                                                 const T* __restrict__ out, const T* __restrict__ dout,
                                                                 const float* __restrict__ lse, float* __restrict__ delta,
                                                                 float* __restrict__ dq, float* __restrict__ dbias,
                                                                 int B, int N, int H, float scale, int bias_ld, float* __restrict__ dpart,
                                                                 const AttnDrop drop, int Pn) {
    constexpr int PLANE = TKV * 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;                       // K rows  (S^T = K Q^T)
    char* Vs = smem + PLANE;               // V rows  (dP^T = V dO^T)
    char* Kt = smem + 2 * PLANE;           // K again, blocked for the transpose read (dQ^T += K^T dS^T)
    const int nqt = (N + TQ - 1) / TQ;
    const int qt = nqt - 1 - (int)blockIdx.x;
    const int b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hi = lane >> 5;
    const int h = blockIdx.y * 4 + wave;
    const bool active = h < H;
    const int i0 = qt * TQ;
    const int qi = i0 + (lane & 31);
    const int nb = i0 + TQ;
    const int off = PFX ? Pn - 1 : 0;                                              // PFX: negative-distance bins in front
    const int kend = PFX && i0 < Pn ? max(i0 + TQ, Pn) : i0 + TQ;
    float* bias_l = (float*)(smem + 3 * PLANE) + (size_t)wave * (nb + off);              // [4][nb + off]
    float* dbias_l = (float*)(smem + 3 * PLANE) + (size_t)(4 + wave) * (nb + off);       // [4][nb + off]
    // key-mask ballots of every 64-key tile, built once (a global load + ballot per k-tile stalled each iteration)
    unsigned long long* mbits = (unsigned long long*)(smem + 3 * PLANE + (size_t)8 * (nqt * TQ + off) * sizeof(float));
    const size_t rowbase = (size_t)b * N;
    const size_t qrow = (rowbase + min(qi, N - 1)) * (size_t)(H * 64) + (active ? h : 0) * 64;

    h16x8 qf[4], dof[4], dummy;
    float dl = 0.f, L = 0.f;
    if (active) {
        if (PFX) {
            for (int r = lane; r < nb + off; r += 64) {
                bias_l[r] = bias ? bias[(ptrdiff_t)min(r - off, N - 1) * bias_ld + h] * LOG2E : 0.f;
                dbias_l[r] = 0.f;
            }
        } else
        for (int r = lane; r < nb; r += 64) {
            bias_l[r] = bias ? bias[(size_t)min(r, N - 1) * bias_ld + h] * LOG2E : 0.f;
            dbias_l[r] = 0.f;
        }
        bias_l += off;                                 // index rel from here on
        dbias_l += off;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            h16x8 of;
            load_row8<T, false>(q + qrow + 16 * s + 8 * hi, qi < N, qf[s], dummy);
            load_row8<T, false>(dout + qrow + 16 * s + 8 * hi, qi < N, dof[s], dummy);
            // delta uses the unrounded tensors
            if (qi < N) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    dl += load_as_float(dout + qrow + 16 * s + 8 * hi + e) * load_as_float(out + qrow + 16 * s + 8 * hi + e);
            }
        }
        dl += __shfl_xor(dl, 32, 64);
        L = lse[((size_t)b * H + h) * N + min(qi, N - 1)];
        if (hi == 0 && qi < N) delta[((size_t)b * H + h) * N + qi] = dl;
    }
    f32x16 acc[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; }
    const float c = scale * LOG2E;
    // DROP: row key of (b, h, qi) with this half-wave's key bit (see the forward)
    const unsigned rk = DROP ? attn_drop_headkey(attn_drop_seed(drop), b, active ? h : 0) ^ ((unsigned)qi << 15) ^ (2u * (unsigned)hi) : 0u;

    const int nkt = (kend + TKV - 1) / TKV;
    KVRegs<T, false> kr, vr;
    kr.load(k + rowbase * 64, 0, N);
    vr.load(v + rowbase * 64, 0, N);
    for (int ch = wave; ch < nkt; ch += 4) {
        const int jk = ch * TKV + lane;
        const bool live = jk < N && (keymask ? keymask[rowbase + jk] != 0 : true);
        const unsigned long long bb = __ballot(live);
        if (lane == 0) mbits[ch] = bb;
    }
    for (int kt = 0; kt < nkt; ++kt) {
        const int j0 = kt * TKV;
        __syncthreads();
        kr.store(Ks, Ks);
        kr.store_blk(Kt, Kt);
        vr.store(Vs, Vs);
        __syncthreads();
        const unsigned long long bits = mbits[kt];
        if (kt + 1 < nkt) {
            kr.load(k + rowbase * 64, j0 + TKV, N);
            vr.load(v + rowbase * 64, j0 + TKV, N);
        }
        if (!active) continue;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int jb = j0 + 32 * sub;
            if (jb > kend - 1) break;
            f32x16 st, dp;
#pragma unroll
            for (int e = 0; e < 16; ++e) { st[e] = 0.f; dp[e] = 0.f; }
            {   // all eight fragment reads in flight before the first MFMA, retired in two groups: left to hipcc (at the register
                // ceiling here) every fragment went through the same four registers, one read -> wait -> MFMA at a time (ISA)
                h16x8 kfr[4], vfr[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) { kfr[s] = frag_rows(Ks, 32 * sub, s, lane); vfr[s] = frag_rows(Vs, 32 * sub, s, lane); }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    if ((s & 1) == 0) asm volatile("" : "+v"(kfr[s]), "+v"(vfr[s]), "+v"(kfr[s + 1]), "+v"(vfr[s + 1]));
                    st = MFMA(kfr[s], qf[s], st);                                // S^T  = K Q^T
                    dp = MFMA(vfr[s], dof[s], dp);                               // dP^T = V dO^T
                }
            }
            if (DROP) {                        // dP~ -> Z dP~ / (1 - p): then dS = P (Z dP~ / (1 - p) - delta) below
                const unsigned kb = rk ^ (unsigned)(jb >> 1);
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const unsigned w = omlm_hash32(kb ^ (unsigned)(((r & 3) + 8 * (r >> 2)) >> 1));
                    dp[r] = (w << 16) >= drop.thr16 ? dp[r] * drop.rs : 0.f;
                    dp[r + 1] = w >= drop.thr16 ? dp[r + 1] * drop.rs : 0.f;
                }
            }
            // three straight passes (gather bias, arithmetic, scatter d(bias)): a fused per-element loop compiled to 16
            // serialised LDS round trips (read -> wait -> exp -> atomic), ~3k cycles per 32x32 block
            float bv[16];
            auto element = [&](int r, bool ok) {
                const float p = __builtin_amdgcn_exp2f(ok ? st[r] * c + bv[r] - L : NEG_BIG);
                bv[r] = p * (dp[r] - dl);
                st[r] = bv[r] * scale;
            };
            if (jb + 31 <= i0) {
                // subtile entirely below the diagonal (see the forward): constant LDS offsets from one base, one 32-bit mask word
                const unsigned w32 = qi < N ? (unsigned)(bits >> (32 * sub)) >> (4 * hi) : 0u;
                const float* bp = bias_l + (qi - jb - 4 * hi);
#pragma unroll
                for (int r = 0; r < 16; ++r) bv[r] = bp[-((r & 3) + 8 * (r >> 2))];
#pragma unroll
                for (int r = 0; r < 16; ++r) element(r, (w32 >> ((r & 3) + 8 * (r >> 2))) & 1u);
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) bv[r] = bias_l[max(min(qi - (j0 + 32 * sub + crow(r, hi)), nb - 1), -off)];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kr = 32 * sub + crow(r, hi);
                    const int rel = qi - (j0 + kr);
                    element(r, (rel >= 0 || (PFX && qi < Pn && j0 + kr < Pn)) && ((bits >> kr) & 1ull) && (qi < N));
                }
            }
            if (dbias) {
                // d(bias)[rel] = sum of dS over the diagonal rel = i - j.  LDS float atomics (one per element) cost 930 us
                // per layer (measured: 1496 -> 565 us without them), so the 63 diagonals of the 32x32 block are summed in
                // registers instead: output lane L stands for t = q - kr = L - 31 and pulls row kr's element from query
                // column q = t + kr through the cross-lane permute (no LDS memory access); then ONE plain read-add-write
                // of the wave-private table, predicated so that every lane owns a distinct bin.
                const float dsum = diag_sum_32x32(bv, lane);
                const int rel = (i0 - j0 - 32 * sub) + (lane - 31);
                if (rel >= -off && rel < nb) dbias_l[rel] += dsum;
            }
            {   // the four K^T fragments requested together, the packing of dS under their latency, retired pair by pair
                h16x8 ktf[2][2], dsb[2];
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) ktf[s][dt] = frag_cols_tr(Kt, 32 * sub, s, 32 * dt, lane);
#pragma unroll
                for (int s = 0; s < 2; ++s) pack_acc<false>(st, s, dsb[s], dummy);
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    asm volatile("" : "+v"(ktf[s][0]), "+v"(ktf[s][1]));
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) acc[dt] = MFMA(ktf[s][dt], dsb[s], acc[dt]);   // dQ^T += K^T dS^T
                }
            }
        }
    }
    if (!active) return;
    if (qi < N) {
        float* drow = dq + (rowbase + qi) * (size_t)(H * 64) + h * 64;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int d = 32 * dt + 8 * g4 + 4 * hi;
                *(float4*)(drow + d) = make_float4(acc[dt][4 * g4], acc[dt][4 * g4 + 1], acc[dt][4 * g4 + 2], acc[dt][4 * g4 + 3]);
            }
    }
    if (dbias) {
        // LDS atomics of this wave are complete in program order for this wave's own later reads
        __builtin_amdgcn_s_waitcnt(0xc07f);
        if (dpart) {
            // this wave's table as ONE row of the partial buffer [(b, h, query tile)][nqt * TQ]: plain coalesced stores.  Device-scope
            // atomics into the shared [N, heads] table kept every wave alive until ~1800 contended read-modify-writes had drained
            // (measured at B = 8, N = 1817, H = 16: 290 us of a 790 us backward); omlm_attn_dbias_reduce adds the rows up.
            float* prow = dpart + (((size_t)b * H + h) * nqt + qt) * (size_t)(nqt * TQ);
            for (int r = lane; r < nb; r += 64) prow[r] = dbias_l[r];
        } else
        for (int r = lane; r < min(nb, N); r += 64) {
            const float vv = dbias_l[r];
            if (vv != 0.f) unsafeAtomicAdd(dbias + (size_t)r * bias_ld + h, vv);
        }
        if (PFX && i0 < Pn)                            // negative distances: only query tiles inside the prefix reach them
            for (int r = lane - off; r < 0; r += 64) {
                const float vv = dbias_l[r];
                if (vv != 0.f) unsafeAtomicAdd(dbias + (ptrdiff_t)r * bias_ld + h, vv);
            }
    }
}

// The same kernel for fp32 ("bf16x3") operands with hi/lo S and dP, kept as its own function so that the bf16 kernel's code and
// register allocation (already at the 256-register limit) stay exactly as measured.
template <typename T, bool DROP = false, bool PFX = false>
__global__ __launch_bounds__(AT_THREADS) __attribute__((amdgpu_waves_per_eu(AT_DQP_WPE))) void attn_bwd_dq_precise_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                 const T* __restrict__ v, const float* __restrict__ bias,
                                                                 const unsigned char* __restrict__ keymask,
                                                                 const T* __restrict__ out, const T* __restrict__ dout,
                                                                 const float* __restrict__ lse, float* __restrict__ delta,
                                                                 float* __restrict__ dq, float* __restrict__ dbias,
                                                                 int B, int N, int H, float scale, int bias_ld, float* __restrict__ dpart,
                                                                 const AttnDrop drop, int Pn) {
    // fp32 operands ("bf16x3"): S and dP -- the two products the probabilities and d(bias) are made of -- are formed from
    // hi/lo splits (3 MFMAs per product), so p, dS and the rel-pos bias gradient are fp32-grade; dQ = dS K itself stays a
    // single bf16 pass (dS rounded once), like every other gradient GEMM operand of this mode's backward.
    constexpr bool PRECISE = elt_traits<T>::precise;
    constexpr int PLANE = TKV * 128;
    constexpr int NPL = PRECISE ? 5 : 3;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;                       // K rows  (S^T = K Q^T)
    char* Vs = smem + PLANE;               // V rows  (dP^T = V dO^T)
    char* Kt = smem + 2 * PLANE;           // K again, blocked for the transpose read (dQ^T += K^T dS^T)
    char* Ksl = smem + 3 * PLANE;          // lo planes (PRECISE only)
    char* Vsl = smem + 4 * PLANE;
    const int nqt = (N + TQ - 1) / TQ;
    const int qt = nqt - 1 - (int)blockIdx.x;
    const int b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hi = lane >> 5;
    const int h = blockIdx.y * 4 + wave;
    const bool active = h < H;
    const int i0 = qt * TQ;
    const int qi = i0 + (lane & 31);
    const int nb = i0 + TQ;
    const int off = PFX ? Pn - 1 : 0;                                              // PFX: negative-distance bins in front
    const int kend = PFX && i0 < Pn ? max(i0 + TQ, Pn) : i0 + TQ;
    float* bias_l = (float*)(smem + NPL * PLANE) + (size_t)wave * (nb + off);              // [4][nb + off]
    float* dbias_l = (float*)(smem + NPL * PLANE) + (size_t)(4 + wave) * (nb + off);       // [4][nb + off]
    // key-mask ballots of every 64-key tile, built once (a global load + ballot per k-tile stalled each iteration)
    unsigned long long* mbits = (unsigned long long*)(smem + NPL * PLANE + (size_t)8 * (nqt * TQ + off) * sizeof(float));
    const size_t rowbase = (size_t)b * N;
    const size_t qrow = (rowbase + min(qi, N - 1)) * (size_t)(H * 64) + (active ? h : 0) * 64;

    h16x8 qf[4], dof[4], ql[4], dol[4], dummy;
    float dl = 0.f, L = 0.f;
    if (active) {
        if (PFX) {
            for (int r = lane; r < nb + off; r += 64) {
                bias_l[r] = bias ? bias[(ptrdiff_t)min(r - off, N - 1) * bias_ld + h] * LOG2E : 0.f;
                dbias_l[r] = 0.f;
            }
        } else
        for (int r = lane; r < nb; r += 64) {
            bias_l[r] = bias ? bias[(size_t)min(r, N - 1) * bias_ld + h] * LOG2E : 0.f;
            dbias_l[r] = 0.f;
        }
        bias_l += off;                                 // index rel from here on
        dbias_l += off;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            h16x8 of;
            load_row8<T, PRECISE>(q + qrow + 16 * s + 8 * hi, qi < N, qf[s], ql[s]);
            load_row8<T, PRECISE>(dout + qrow + 16 * s + 8 * hi, qi < N, dof[s], dol[s]);
            // delta uses the unrounded tensors
            if (qi < N) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    dl += load_as_float(dout + qrow + 16 * s + 8 * hi + e) * load_as_float(out + qrow + 16 * s + 8 * hi + e);
            }
        }
        dl += __shfl_xor(dl, 32, 64);
        L = lse[((size_t)b * H + h) * N + min(qi, N - 1)];
        if (hi == 0 && qi < N) delta[((size_t)b * H + h) * N + qi] = dl;
    }
    f32x16 acc[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; }
    const float c = scale * LOG2E;
    // DROP: row key of (b, h, qi) with this half-wave's key bit (see the forward)
    const unsigned rk = DROP ? attn_drop_headkey(attn_drop_seed(drop), b, active ? h : 0) ^ ((unsigned)qi << 15) ^ (2u * (unsigned)hi) : 0u;

    const int nkt = (kend + TKV - 1) / TKV;
    KVRegs<T, PRECISE> kr, vr;
    kr.load(k + rowbase * 64, 0, N);
    vr.load(v + rowbase * 64, 0, N);
    for (int ch = wave; ch < nkt; ch += 4) {
        const int jk = ch * TKV + lane;
        const bool live = jk < N && (keymask ? keymask[rowbase + jk] != 0 : true);
        const unsigned long long bb = __ballot(live);
        if (lane == 0) mbits[ch] = bb;
    }
    for (int kt = 0; kt < nkt; ++kt) {
        const int j0 = kt * TKV;
        __syncthreads();
        kr.store(Ks, Ksl);
        kr.store_blk_hi(Kt);
        vr.store(Vs, Vsl);
        __syncthreads();
        const unsigned long long bits = mbits[kt];
        if (kt + 1 < nkt) {
            kr.load(k + rowbase * 64, j0 + TKV, N);
            vr.load(v + rowbase * 64, j0 + TKV, N);
        }
        if (!active) continue;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int jb = j0 + 32 * sub;
            if (jb > kend - 1) break;
            f32x16 st, dp;
#pragma unroll
            for (int e = 0; e < 16; ++e) { st[e] = 0.f; dp[e] = 0.f; }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (PRECISE) {
                    const h16x8 ka = frag_rows(Ks, 32 * sub, s, lane), va = frag_rows(Vs, 32 * sub, s, lane);
                    st = MFMA(frag_rows(Ksl, 32 * sub, s, lane), qf[s], st);
                    st = MFMA(ka, ql[s], st);
                    st = MFMA(ka, qf[s], st);
                    dp = MFMA(frag_rows(Vsl, 32 * sub, s, lane), dof[s], dp);
                    dp = MFMA(va, dol[s], dp);
                    dp = MFMA(va, dof[s], dp);
                } else {
                    st = MFMA(frag_rows(Ks, 32 * sub, s, lane), qf[s], st);      // S^T  = K Q^T
                    dp = MFMA(frag_rows(Vs, 32 * sub, s, lane), dof[s], dp);     // dP^T = V dO^T
                }
            }
            if (DROP) {                        // dP~ -> Z dP~ / (1 - p): then dS = P (Z dP~ / (1 - p) - delta) below
                const unsigned kb = rk ^ (unsigned)(jb >> 1);
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const unsigned w = omlm_hash32(kb ^ (unsigned)(((r & 3) + 8 * (r >> 2)) >> 1));
                    dp[r] = (w << 16) >= drop.thr16 ? dp[r] * drop.rs : 0.f;
                    dp[r + 1] = w >= drop.thr16 ? dp[r + 1] * drop.rs : 0.f;
                }
            }
            // three straight passes (gather bias, arithmetic, scatter d(bias)): a fused per-element loop compiled to 16
            // serialised LDS round trips (read -> wait -> exp -> atomic), ~3k cycles per 32x32 block
            float bv[16];
            auto element = [&](int r, bool ok) {
                const float p = __builtin_amdgcn_exp2f(ok ? st[r] * c + bv[r] - L : NEG_BIG);
                bv[r] = p * (dp[r] - dl);
                st[r] = bv[r] * scale;
            };
            if (jb + 31 <= i0) {
                // subtile entirely below the diagonal (see the forward): constant LDS offsets from one base, one 32-bit mask word
                const unsigned w32 = qi < N ? (unsigned)(bits >> (32 * sub)) >> (4 * hi) : 0u;
                const float* bp = bias_l + (qi - jb - 4 * hi);
#pragma unroll
                for (int r = 0; r < 16; ++r) bv[r] = bp[-((r & 3) + 8 * (r >> 2))];
#pragma unroll
                for (int r = 0; r < 16; ++r) element(r, (w32 >> ((r & 3) + 8 * (r >> 2))) & 1u);
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) bv[r] = bias_l[max(min(qi - (j0 + 32 * sub + crow(r, hi)), nb - 1), -off)];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kr = 32 * sub + crow(r, hi);
                    const int rel = qi - (j0 + kr);
                    element(r, (rel >= 0 || (PFX && qi < Pn && j0 + kr < Pn)) && ((bits >> kr) & 1ull) && (qi < N));
                }
            }
            if (dbias) {
                // d(bias)[rel] = sum of dS over the diagonal rel = i - j.  LDS float atomics (one per element) cost 930 us
                // per layer (measured: 1496 -> 565 us without them), so the 63 diagonals of the 32x32 block are summed in
                // registers instead: output lane L stands for t = q - kr = L - 31 and pulls row kr's element from query
                // column q = t + kr through the cross-lane permute (no LDS memory access); then ONE plain read-add-write
                // of the wave-private table, predicated so that every lane owns a distinct bin.
                const float dsum = diag_sum_32x32(bv, lane);
                const int rel = (i0 - j0 - 32 * sub) + (lane - 31);
                if (rel >= -off && rel < nb) dbias_l[rel] += dsum;
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                h16x8 dsb;
                pack_acc<false>(st, s, dsb, dummy);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
                    acc[dt] = MFMA(frag_cols_tr(Kt, 32 * sub, s, 32 * dt, lane), dsb, acc[dt]);   // dQ^T += K^T dS^T
            }
        }
    }
    if (!active) return;
    if (qi < N) {
        float* drow = dq + (rowbase + qi) * (size_t)(H * 64) + h * 64;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int d = 32 * dt + 8 * g4 + 4 * hi;
                *(float4*)(drow + d) = make_float4(acc[dt][4 * g4], acc[dt][4 * g4 + 1], acc[dt][4 * g4 + 2], acc[dt][4 * g4 + 3]);
            }
    }
    if (dbias) {
        // LDS atomics of this wave are complete in program order for this wave's own later reads
        __builtin_amdgcn_s_waitcnt(0xc07f);
        if (dpart) {
            // this wave's table as ONE row of the partial buffer [(b, h, query tile)][nqt * TQ]: plain coalesced stores.  Device-scope
            // atomics into the shared [N, heads] table kept every wave alive until ~1800 contended read-modify-writes had drained
            // (measured at B = 8, N = 1817, H = 16: 290 us of a 790 us backward); omlm_attn_dbias_reduce adds the rows up.
            float* prow = dpart + (((size_t)b * H + h) * nqt + qt) * (size_t)(nqt * TQ);
            for (int r = lane; r < nb; r += 64) prow[r] = dbias_l[r];
        } else
        for (int r = lane; r < min(nb, N); r += 64) {
            const float vv = dbias_l[r];
            if (vv != 0.f) unsafeAtomicAdd(dbias + (size_t)r * bias_ld + h, vv);
        }
        if (PFX && i0 < Pn)                            // negative distances: only query tiles inside the prefix reach them
            for (int r = lane - off; r < 0; r += 64) {
                const float vv = dbias_l[r];
                if (vv != 0.f) unsafeAtomicAdd(dbias + (ptrdiff_t)r * bias_ld + h, vv);
            }
    }
}

// =============================================================================================================
// backward, kernel A: dK, dV.  One workgroup per (sample, 32-key tile); its 4 waves split the (query tile, head)
// work items and reduce their partial dK^T / dV^T through LDS at the end -- no atomics on dK / dV.
// =============================================================================================================
// PFX: the non-causal prefix (see the forward; biasT must be null).  A key tile with j0 < Pn walks every query tile from 0, not from its
// own, and the staged bias columns also cover the negative distances it can meet, rel >= -min(Pn - 1, j0 + 31) (index rel + off): at most
// 31 more entries per column than the causal kernel stages.
template <typename T, bool DROP = false, bool PFX = false>
__global__ __launch_bounds__(AT_THREADS) __attribute__((amdgpu_waves_per_eu(AT_DKV_WPE))) void attn_bwd_dkv_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                  const T* __restrict__ v, const float* __restrict__ bias,
                                                                  const unsigned char* __restrict__ keymask,
                                                                  const T* __restrict__ dout, const float* __restrict__ lse,
                                                                  const float* __restrict__ delta, float* __restrict__ dk,
                                                                  float* __restrict__ dv, int B, int N, int H, float scale, int bias_ld,
                                                                  const float* __restrict__ biasT, int ldT, const AttnDrop drop, int Pn) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hi = lane >> 5;
    char* Qs = smem + wave * 8192;            // per-wave private [32][64] bf16 tiles (Q, dO) for the transpose reads
    char* dOs = Qs + 4096;
    float* red = (float*)(smem);              // reused at the end: [4 waves][64 d][32 j] fp32 = 32 KiB
    float* bias_s = (float*)(smem + 32768);   // [H][nbk] rel-pos table (x log2 e) for rel in [0, N - j0)

    const int nqt = (N + TQ - 1) / TQ;
    const int jt = blockIdx.x;                // 32-key tile; low tiles carry the most (causal) work and launch first
    const int b = blockIdx.z;
    const int j0 = jt * 32;
    const int kj = j0 + (lane & 31);          // this lane's key (column of S)
    const size_t rowbase = (size_t)b * N;
    const float c = scale * LOG2E;
    const int off = PFX ? min(Pn - 1, j0 + 31) : 0;      // PFX: negative distances in front of each staged column
    const int it0 = PFX && j0 < Pn ? 0 : jt;  // first query tile with a live score for these keys
    const int nbk = nqt * TQ - j0 + off;      // rel = i - kj <= nqt*TQ - 1 - j0 (PFX: >= -off)
    h16x8 dummy;
    // WIN: the prepared table (omlm_attn_bias_prepare: [head][64 + rel], x log2 e, minus the head's reference point m_h) is there:
    // an item's 63 bias values are one coalesced load per lane, fetched with the item's Q / dO and parked in a 64-float LDS patch
    // per wave.  Without it the whole [H][N - j0] column set is staged below: 117 KiB for musiclm_large's fine stage
    // (H = 16, N = 1817), i.e. ONE 4-wave workgroup per CU.
    const bool WIN = !PFX && biasT != nullptr;

    // The rel-pos column of every head goes to LDS once.  (Per-element global gathers of bias / lse / delta -- 48
    // dependent L2 round trips per work item -- were >95 % of this kernel: 26k cycles per item for 16 MFMAs.)
    if (PFX) {
        for (int idx = threadIdx.x; idx < H * nbk; idx += AT_THREADS) {
            const int r = idx / H, hh = idx - r * H;
            bias_s[hh * nbk + r] = bias ? bias[(ptrdiff_t)min(r - off, N - 1) * bias_ld + hh] * LOG2E : 0.f;
        }
    } else
    if (!WIN) for (int idx = threadIdx.x; idx < H * nbk; idx += AT_THREADS) {
        const int r = idx / H, hh = idx - r * H;
        bias_s[hh * nbk + r] = bias ? bias[(size_t)min(r, N - 1) * bias_ld + hh] * LOG2E : 0.f;
    }

    // K^T, V^T B-operands: lane n = key kj, dims 16 s + 8 hi .. +7 -- resident for the whole kernel
    h16x8 kf[4], vf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        load_row8<T, false>(k + (rowbase + min(kj, N - 1)) * 64 + 16 * s + 8 * hi, kj < N, kf[s], dummy);
        load_row8<T, false>(v + (rowbase + min(kj, N - 1)) * 64 + 16 * s + 8 * hi, kj < N, vf[s], dummy);
    }
    const bool keylive = kj < N && (keymask ? keymask[rowbase + kj] != 0 : true);
    // DROP: the draw of (i, kj) is the (kj & 1) half of omlm_hash32(row key ^ (kj >> 1)), the upper half of (word << dsh) (common.h)
    const unsigned long long dseed = DROP ? attn_drop_seed(drop) : 0ull;
    const unsigned dsh = (kj & 1) ? 0u : 16u;

    f32x16 dkacc[2], dvacc[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) { dkacc[0][e] = 0.f; dkacc[1][e] = 0.f; dvacc[0][e] = 0.f; dvacc[1][e] = 0.f; }

    const int nitems = (nqt - it0) * H;       // (query tile it >= it0) x head
    // A-operand fragments (rows = queries i0 + (lane&31), dims 16 s + 8 hi) of Q and dO plus the tile's lse / delta
    // (one value per lane = per query); the NEXT item's are fetched while the current item is on the matrix cores.
    h16x8 qa[4], doa[4], qn[4], don[4];
    float La = 0.f, Da = 0.f, Ln = 0.f, Dn = 0.f, Ba = 0.f, Bn = 0.f, Ma = 0.f, Mn = 0.f;
    auto fetch = [&](int item, h16x8 (&fq)[4], h16x8 (&fd)[4], float& fl, float& fdl, float& fb, float& fm) {
        const int qi_ = (it0 + item / H) * TQ + (lane & 31);
        const int hh = item % H;
        const size_t qrow_ = (rowbase + min(qi_, N - 1)) * (size_t)(H * 64) + hh * 64;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            load_row8<T, false>(q + qrow_ + 16 * s + 8 * hi, qi_ < N, fq[s], dummy);
            load_row8<T, false>(dout + qrow_ + 16 * s + 8 * hi, qi_ < N, fd[s], dummy);
        }
        fl = lse[((size_t)b * H + hh) * N + min(qi_, N - 1)];
        fdl = delta[((size_t)b * H + hh) * N + min(qi_, N - 1)];
        if (WIN) {      // window of rel = i - j for the item: from (i0 - j0 - 31); table index 64 + rel; lse made relative to m_h
            const float* row = biasT + (size_t)hh * ldT;
            fb = row[64 + ((it0 + item / H) * TQ - j0 - 31) + min(lane, 62)];
            fm = row[ldT - 1];      // subtracted where the item is consumed: an arithmetic use here waits for every load issued above
        }
    };
    if (wave < nitems) fetch(wave, qa, doa, La, Da, Ba, Ma);
    // Consume the first item's loads HERE.  Left pending into the loop, hipcc's wait-count pass has to assume at the loop header
    // that qa / doa / La / Da may still be in flight from this block; its conservative counts (vmcnt(3) ... vmcnt(0) in front of
    // the first MFMA of EVERY item, seen in the ISA) then also drain the NEXT item's loads that the loop has just issued: the
    // prefetch ran with nothing in flight and every item paid a full memory round trip.
#pragma unroll
    for (int s = 0; s < 4; ++s) asm volatile("" : "+v"(qa[s]), "+v"(doa[s]));
    asm volatile("" : "+v"(La), "+v"(Da), "+v"(Ba), "+v"(Ma));
    __syncthreads();                           // bias_s staged
    for (int item = wave; item < nitems; item += 4) {
        const int it = it0 + item / H, h = item % H;
        const int i0 = it * TQ;
        if (item + 4 < nitems) fetch(item + 4, qn, don, Ln, Dn, Bn, Mn);
#pragma unroll
        for (int s = 0; s < 4; ++s) {        // park this item's tiles in LDS for the transpose reads
            *(h16x8*)(Qs + tile_off_blk(lane & 31, (2 * s + hi) * 16)) = qa[s];
            *(h16x8*)(dOs + tile_off_blk(lane & 31, (2 * s + hi) * 16)) = doa[s];
        }
        // lean form (see the forward): the tile's lse / delta go through a 64-float per-wave LDS patch instead of 4 v_readlane +
        // 2 selects per score row, and items whose queries all follow this workgroup's keys (all but the first query tile) skip the
        // causal compare, the i < N compare and the clamp of the bias index (constant LDS offsets from one base)
        const float* bh = bias_s + h * nbk + off;
        float* ld_l = WIN ? (float*)(smem + 32768) + wave * 128 : (float*)(smem + 32768 + (size_t)H * (PFX ? nqt * TQ + 31 : nqt * TQ) * sizeof(float)) + wave * 64;
        if (lane < 32) { ld_l[lane] = La - Ma; ld_l[32 + lane] = Da; }        // Ma: the head's reference point (WIN), else 0
        if (WIN) ld_l[64 + lane] = Ba;
        // window index of (query row crow(r, hi), this lane's key): cr + 4 hi - (lane & 31) + 31
        const float* bwp = ld_l + 64 + 31 + 4 * hi - (lane & 31);
        f32x16 st, dp, zz;
#pragma unroll
        for (int e = 0; e < 16; ++e) { st[e] = 0.f; dp[e] = 0.f; }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            st = MFMA(qa[s], kf[s], st);       // S  = Q K^T   (rows i, column = this lane's key)
            dp = MFMA(doa[s], vf[s], dp);      // dP = dO V^T
        }
        if (DROP) {                            // dP~ -> Z dP~ / (1 - p) (dS below), zz = Z / (1 - p) for dV's P Z / (1 - p)
            const unsigned lk = attn_drop_headkey(dseed, b, h) ^ ((unsigned)kj >> 1) ^ ((unsigned)(i0 + 4 * hi) << 15);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned w = omlm_hash32(lk ^ ((unsigned)((r & 3) + 8 * (r >> 2)) << 15));
                const float z = (w << dsh) >= drop.thr16 ? drop.rs : 0.f;
                dp[r] *= z;
                zz[r] = z;
            }
        }
        f32x16 pp;
        const float* lp = ld_l + 4 * hi;
        if (i0 >= j0 + 31 && i0 + 31 < N) {
            const float* bp = WIN ? bwp : bh + (i0 - kj + 4 * hi);
            // gather pass, values pinned, then the arithmetic: with the reads inside `keylive ? ... : NEG_BIG` hipcc wrapped each
            // element's two LDS reads in its own exec-masked block (read, read, wait, fma, wait, subtract: sixteen exposed LDS round
            // trips per item, seen in the ISA); all indices are in range for every lane here, so the reads need no predicate
            float bvv[16], lvv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cr = (r & 3) + 8 * (r >> 2);                     // crow(r, hi) - 4 hi
                bvv[r] = bp[cr];
                lvv[r] = lp[cr];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(bvv[r]), "+v"(lvv[r]));
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cr = (r & 3) + 8 * (r >> 2);
                const float x = st[r] * c + bvv[r] - lvv[r];
                const float p = __builtin_amdgcn_exp2f(keylive ? x : NEG_BIG);
                pp[r] = DROP ? p * zz[r] : p;
                st[r] = p * (dp[r] - lp[32 + cr]) * scale;
            }
        } else {
            // diagonal / tail items (16 of a workgroup's items: the first query tile, and the last one when N % 32 != 0).  Written as
            // one loop, `ok ? (expression with two LDS reads) : NEG_BIG` compiled to 16 branches, each around its own read -> wait ->
            // read -> wait (seen in the ISA).  Two passes, the gathered values pinned in registers in between: straight-line code with
            // counted waits like the branch above; same arithmetic per element.
            float bvv[16], lvv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cr = (r & 3) + 8 * (r >> 2);
                bvv[r] = WIN ? bwp[cr] : bh[max(min(i0 + crow(r, hi) - kj, nbk - off - 1), -off)];
                lvv[r] = lp[cr];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(bvv[r]), "+v"(lvv[r]));
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cr = (r & 3) + 8 * (r >> 2);
                const int i = i0 + crow(r, hi);
                const bool ok = (i >= kj || (PFX && i < Pn && kj < Pn)) && keylive && (i < N);
                const float x = st[r] * c + bvv[r] - lvv[r];
                const float p = __builtin_amdgcn_exp2f(ok ? x : NEG_BIG);
                pp[r] = DROP ? p * zz[r] : p;
                st[r] = p * (dp[r] - lp[32 + cr]) * scale;
            }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            h16x8 pb, dsb;
            pack_acc<false>(pp, s, pb, dummy);
            pack_acc<false>(st, s, dsb, dummy);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                dvacc[dt] = MFMA(frag_cols_tr(dOs, 0, s, 32 * dt, lane), pb, dvacc[dt]);    // dV^T += dO^T P
                dkacc[dt] = MFMA(frag_cols_tr(Qs, 0, s, 32 * dt, lane), dsb, dkacc[dt]);    // dK^T += Q^T dS
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) { qa[s] = qn[s]; doa[s] = don[s]; }
        La = Ln; Da = Dn; Ba = Bn; Ma = Mn;
    }
    // cross-wave reduction through LDS, one accumulator pair at a time
    for (int which = 0; which < 2; ++which) {
        __syncthreads();
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int d = 32 * dt + crow(r, hi);
                red[((size_t)wave * 64 + d) * 32 + (lane & 31)] = which == 0 ? dkacc[dt][r] : dvacc[dt][r];
            }
        __syncthreads();
        float* dst = which == 0 ? dk : dv;
        for (int e = threadIdx.x; e < 64 * 32; e += AT_THREADS) {
            const int j = e >> 6, d = e & 63;          // consecutive threads -> consecutive d (coalesced rows)
            const float s4 = red[(0 * 64 + d) * 32 + j] + red[(1 * 64 + d) * 32 + j] + red[(2 * 64 + d) * 32 + j] + red[(3 * 64 + d) * 32 + j];
            if (j0 + j < N) dst[(rowbase + j0 + j) * 64 + d] = s4;
        }
    }
}

// =============================================================================================================
// Host side.  csrc/attn_plan.h decides what a call runs -- kernels, grids, LDS bytes -- or why it is refused; the entry points below check
// their arguments, ask for the plan and launch its list.
using omlm_plan::AttnArgs; using omlm_plan::AttnCall; using omlm_plan::AttnLaunch; using omlm_plan::AttnPlan;
static_assert(omlm_plan::ATTN_UNSUPPORTED == OMLM_ERR_UNSUPPORTED && TQ == 32 && TKV == 64, "attn_plan.h states the return code and the first-generation tiles");

// attention2.hip / attention3.hip: one launch of the plan each
void attn2_fwd_launch(const AttnLaunch& l, int ldT, const void* q, const void* k, const void* v, const float* biasT, const unsigned char* keymask,
                      void* out, float* lse, int B, int N, int H, float scale, hipStream_t st, const AttnDrop& dr, int Pn);
void attn2_bwd_dq_launch(const AttnLaunch& l, int ldT, const void* q, const void* k, const void* v, const float* biasT, const unsigned char* keymask,
                         const void* out, const void* dout, const float* lse, float* delta, float* dq, float* dbias, int bias_ld,
                         float* dpart, int B, int N, int H, float scale, hipStream_t st, const AttnDrop& dr, int Pn);
extern "C" __attribute__((visibility("hidden"))) void omlm_attn_dbias_reduce_launch(const AttnLaunch* l, const float* dpart, float* dbias, int bias_ld, int B, int N, int H, void* stream);   // (bf16 copy)
void attn3_bwd_dkv_launch(const AttnLaunch& l, int ldT, const void* q, const void* k, const void* v, const float* biasT, const unsigned char* keymask,
                          const void* dout, const float* lse, const float* delta, float* dk, float* dv,
                          int B, int N, int H, float scale, hipStream_t st, const AttnDrop& dr, int Pn, float* part);

#define A1_LAUNCH(KERNEL, T, ...)                                                                                                        \
    with_flags(l.drop, l.pfx, [&](auto D, auto P) {                                                                                      \
        launch_lds_cap<KERNEL<T, decltype(D)::value, decltype(P)::value>>(dim3(l.gx, l.gy, l.gz), dim3(l.threads), l.lds, st, __VA_ARGS__); \
    })

// The launch loops.  The entry has checked the arguments, attn_run_here has the plan and the kernels' dropout argument.
static int attn_fwd_run_here(const AttnPlan& plan, const AttnCall& c, const AttnArgs& a, const AttnDrop& dr) {
    // Pn = min(P, N): 0 is causal, >= 1 the non-causal prefix of include/omlm.h.  The kernels take the rel = 0 row of the [N + Pn - 1, bias_ld] table.
    const int B = c.B, N = c.N, H = c.H, bias_ld = a.bias_ld, Pn = omlm_plan::attn_prefix_rows(N, c.P);
    const float scale = a.scale, *bias = a.bias && Pn > 0 ? a.bias + (size_t)(Pn - 1) * bias_ld : a.bias;
    hipStream_t st = as_stream(a.stream);
    for (int i = 0; i < plan.n; ++i) {
        const AttnLaunch& l = plan.l[i];
        if (l.family == omlm_plan::ATTN_A4_FWD) attn2_fwd_launch(l, plan.ldT, a.q, a.k, a.v, a.biasT, a.keymask, a.out, a.lse, B, N, H, scale, st, dr, Pn);
#if !OMLM_FP16
        else if (l.precise) A1_LAUNCH(attn_fwd_kernel, float, (const float*)a.q, (const float*)a.k, (const float*)a.v, bias, a.keymask, (float*)a.out, a.lse, B, N, H, scale, bias_ld, dr, Pn);
#endif
        else A1_LAUNCH(attn_fwd_kernel, h16_t, (const h16_t*)a.q, (const h16_t*)a.k, (const h16_t*)a.v, bias, a.keymask, (h16_t*)a.out, a.lse, B, N, H, scale, bias_ld, dr, Pn);
        if (int rc = omlm_post_launch("omlm_mqa_attn_fwd")) return rc;
    }
    return OMLM_OK;
}
// d(bias) of rel >= 0 goes through the workspace and its reduction, that of rel < 0 (Pn > 1) by atomics from the dQ kernel.
static int attn_bwd_run_here(const AttnPlan& plan, const AttnCall& c, const AttnArgs& a, const AttnDrop& dr) {
    const int B = c.B, N = c.N, H = c.H, bias_ld = a.bias_ld, Pn = omlm_plan::attn_prefix_rows(N, c.P);
    const size_t r0 = Pn > 0 ? (size_t)(Pn - 1) * bias_ld : 0;      // bias, dbias: the rel = 0 row of their tables
    const float scale = a.scale, *bias = a.bias ? a.bias + r0 : nullptr;
    float* dbias = a.dbias ? a.dbias + r0 : nullptr;
    float* dpart = dbias ? a.dbias_ws : nullptr;      // per-(sample, head, query tile) d(bias) rows, summed by the reduction
    float* dkv_part = plan.dkv_slots >= 0 ? a.dbias_ws + plan.dkv_slots : nullptr;
    hipStream_t st = as_stream(a.stream);
    for (int i = 0; i < plan.n; ++i) {
        const AttnLaunch& l = plan.l[i];
        switch (l.family) {
        case omlm_plan::ATTN_A2_DQ:
            attn2_bwd_dq_launch(l, plan.ldT, a.q, a.k, a.v, a.biasT, a.keymask, a.out, a.dout, a.lse, a.delta, a.dq, dbias, bias_ld, dpart, B, N, H, scale, st, dr, Pn);
            break;
        case omlm_plan::ATTN_A1_DQ:
#if !OMLM_FP16
            if (l.precise) A1_LAUNCH(attn_bwd_dq_precise_kernel, float, (const float*)a.q, (const float*)a.k, (const float*)a.v, bias, a.keymask, (const float*)a.out, (const float*)a.dout, a.lse, a.delta, a.dq, dbias, B, N, H, scale, bias_ld, dpart, dr, Pn);
            else
#endif
            A1_LAUNCH(attn_bwd_dq_kernel, h16_t, (const h16_t*)a.q, (const h16_t*)a.k, (const h16_t*)a.v, bias, a.keymask, (const h16_t*)a.out, (const h16_t*)a.dout, a.lse, a.delta, a.dq, dbias, B, N, H, scale, bias_ld, dpart, dr, Pn);
            break;
        case omlm_plan::ATTN_DBIAS_REDUCE:
            omlm_attn_dbias_reduce_launch(&l, dpart, dbias, bias_ld, B, N, H, st);
            break;
        case omlm_plan::ATTN_A1_DKV:
#if !OMLM_FP16
            if (l.precise) A1_LAUNCH(attn_bwd_dkv_kernel, float, (const float*)a.q, (const float*)a.k, (const float*)a.v, bias, a.keymask, (const float*)a.dout, a.lse, a.delta, a.dk, a.dv, B, N, H, scale, bias_ld, l.win ? a.biasT : nullptr, plan.ldT, dr, Pn);
            else
#endif
            A1_LAUNCH(attn_bwd_dkv_kernel, h16_t, (const h16_t*)a.q, (const h16_t*)a.k, (const h16_t*)a.v, bias, a.keymask, (const h16_t*)a.dout, a.lse, a.delta, a.dk, a.dv, B, N, H, scale, bias_ld, l.win ? a.biasT : nullptr, plan.ldT, dr, Pn);
            break;
        default:
            attn3_bwd_dkv_launch(l, plan.ldT, a.q, a.k, a.v, a.biasT, a.keymask, a.dout, a.lse, a.delta, a.dk, a.dv, B, N, H, scale, st, dr, Pn, dkv_part);
        }
        if (int rc = omlm_post_launch("omlm_mqa_attn_bwd")) return rc;
    }
    return OMLM_OK;
}
static int attn_run_here(AttnCall c, const AttnArgs& a) {
    c.fp16_copy = OMLM_FP16 != 0;
    const AttnPlan plan = omlm_plan::attn_plan(c);
    if (plan.rc) { omlm_set_error(plan.msg); return plan.rc; }
    AttnDrop dr = {0ull, nullptr, 0u, 1.0f};
    if (c.drop) (void)attn_drop_args(a.p, a.seed, a.seed_dev, dr);      // (p: checked by the entry)
    return c.backward ? attn_bwd_run_here(plan, c, a, dr) : attn_fwd_run_here(plan, c, a, dr);
}

static_assert(sizeof(AttnCall) == 36 && sizeof(AttnArgs) == 160, "AttnCall / AttnArgs: one layout in both copies");
#if OMLM_FP16
// the fp16 copy has one way in: a call the bf16 copy handed over (attn_to_fp16_copy)
extern "C" __attribute__((visibility("hidden"))) int omlm_attn_run_h(const AttnCall* c, const AttnArgs* a) { return attn_run_here(*c, *a); }
#else
extern "C" int omlm_attn_run_h(const AttnCall* c, const AttnArgs* a);
static int attn_run(AttnCall c, const AttnArgs& a) { return omlm_plan::attn_to_fp16_copy(c) ? omlm_attn_run_h(&c, &a) : attn_run_here(c, a); }

// ---- the C entries (include/omlm.h).  dtype: 0 = fp32 ("bf16x3"), 1 = bf16, 2 = fp16 ----------------------------------------------------------------
extern "C" int omlm_attn_max_positions(int dtype, int P) { return omlm_plan::attn_max_positions(dtype, P); }

extern "C" int omlm_mqa_attn_fwd(const void* q, const void* k, const void* v, const float* bias, const float* biasT, const unsigned char* keymask,
                                 void* out, float* lse, int B, int N, int H, float scale, int bias_ld, int dtype, int P, float p,
                                 unsigned long long seed, const unsigned long long* seed_dev, void* stream) {
    AttnDrop d;
    OMLM_CHECK_ARG(P >= 0, "prefix rows P >= 0");
    OMLM_CHECK_ARG(attn_drop_args(p, seed, seed_dev, d), "dropout p in [0, 1)");
    if (B <= 0 || N <= 0) return OMLM_OK;
    OMLM_CHECK_ARG(q && k && v && out && lse, "null pointer");
    OMLM_CHECK_ARG(H >= 1 && (!bias || bias_ld >= H), "heads / bias pitch");
    AttnArgs a = {};
    a.q = q; a.k = k; a.v = v; a.bias = bias; a.biasT = biasT; a.keymask = keymask; a.out = out; a.lse = lse; a.scale = scale; a.bias_ld = bias_ld;
    a.p = p; a.seed = seed; a.seed_dev = seed_dev; a.stream = stream;
    return attn_run({false, dtype, false, B, N, H, P, bias != nullptr, biasT != nullptr, false, false, p > 0.f, false}, a);
}

// dq [B*N, H*64] fp32, dk, dv [B*N, 64] fp32 (overwritten), dbias [N, bias_ld] fp32 (accumulated, +=), delta [B, H, N] scratch.
extern "C" int omlm_mqa_attn_bwd(const void* q, const void* k, const void* v, const float* bias, const float* biasT, const unsigned char* keymask,
                                 const void* out, const void* dout, const float* lse, float* delta, float* dq, float* dk, float* dv,
                                 float* dbias, float* dbias_ws, int B, int N, int H, float scale, int bias_ld, int dtype, int P,
                                 float p, unsigned long long seed, const unsigned long long* seed_dev, void* stream) {
    AttnDrop d;
    OMLM_CHECK_ARG(P >= 0, "prefix rows P >= 0");
    OMLM_CHECK_ARG(attn_drop_args(p, seed, seed_dev, d), "dropout p in [0, 1)");
    if (B <= 0 || N <= 0) return OMLM_OK;
    OMLM_CHECK_ARG(q && k && v && out && dout && lse && delta && dq && dk && dv, "null pointer");
    OMLM_CHECK_ARG(H >= 1 && ((!bias && !dbias) || bias_ld >= H), "heads / bias pitch");
    AttnArgs a = {};
    a.q = q; a.k = k; a.v = v; a.bias = bias; a.biasT = biasT; a.keymask = keymask; a.out = const_cast<void*>(out); a.lse = const_cast<float*>(lse);      // (read only here)
    a.dout = dout; a.delta = delta; a.dq = dq; a.dk = dk; a.dv = dv; a.dbias = dbias; a.dbias_ws = dbias_ws; a.scale = scale; a.bias_ld = bias_ld;
    a.p = p; a.seed = seed; a.seed_dev = seed_dev; a.stream = stream;
    return attn_run({true, dtype, false, B, N, H, P, bias != nullptr, biasT != nullptr, dbias != nullptr, dbias_ws != nullptr, p > 0.f,
                     dv == dk + (size_t)B * N * 64}, a);
}
#endif

}   // namespace OMLM_NS
