// Causal multi-query attention, second-generation kernels for bf16 operands (transformer.py:254-331 of the reference).
//
// What changed against attention.hip (whose kernels stay for fp32 / "bf16x3" operands), and why:
//   * one workgroup = 8 waves = 8 HEADS of the same 32*QB queries: the single shared K/V head (MQA) is staged once per tile
//     for all of them (the old geometry staged a tile for 4 heads through registers + ds_write behind two barriers per tile,
//     and paid a global round trip for the key mask inside the loop: ~3.9 k cycles per 32x32 block for 8 MFMAs);
//   * K / V tiles and the rel-pos bias window of the tile go HBM/L2 -> LDS by LDS-DMA (buffer_load ... lds) into a 3-stage
//     ring: no VGPR staging, no ds_write, ONE barrier per 64-key tile, two tiles in flight behind counted vmcnt waits;
//   * the key mask costs nothing per score: masked keys get ZERO V rows (the DMA reads them through an out-of-bounds
//     offset) and the softmax denominator is produced by the matrix cores from a 1/0 "live" vector (2 extra MFMAs per block),
//     so masked keys contribute to neither numerator nor denominator.  The running max may include masked keys' scores
//     (they are bounded like the others: l2-normalised q, k); that only moves the reference point of the exponentials;
//   * the causal compare exists only in the blocks that touch the diagonal;
//   * the rel-pos bias is read from a per-tile window (LDS, 128 floats per head) with compile-time offsets from one lane base.
// The arithmetic per score is: fma (scale * log2 e, bias), max, subtract, exp2, pack -- everything else is on the matrix cores.
#include "common.h"
#include "attn_plan.h"

namespace OMLM_NS {

#define A2_THREADS 512
#define A2_TKV 64
#define A2_PAD 64            /* zero entries in front of each row of the transposed bias table (rel >= -64) */
#define A2_BWIN 128          /* floats per head in a tile's bias window */
#define A2_NEG (-1.0e30f)
// the online forward's masked keys: A2_MASKED is added to q.k (the lowest finite half; bf16: -65536), and a running maximum under A2_DEAD c
// (c = scale log2 e) has seen no live score -- live ones have |q.k| far below 16384
#if OMLM_FP16
#define A2_MASKED_BITS 0xFBFFu
#define A2_ONE_BITS 0x3C00u
#else
#define A2_MASKED_BITS 0xC780u
#define A2_ONE_BITS 0x3F80u
#endif
#define A2_DEAD (-16384.0f)
#define A2_LOG2E 1.4426950408889634f
#define A2_STAGE (8192 + 8192 + 8 * A2_BWIN * 4)     /* K rows | V blocked | bias window = 20 KiB */
#define A2_NST 3
#define A2_NL OMLM_ATTN_NL    /* most positions per sample of the long forms (4096 < N <= A2_NL: attn4_fwd_long_kernel, attn2_bwd_dq_long_kernel) */
static_assert(A2_PAD == omlm_plan::ATTN_PAD && A2_BWIN == omlm_plan::ATTN_BWIN && A2_NST * A2_STAGE == omlm_plan::A4_RING,
              "attn_plan.h states the prepared table's layout and the forward's ring");

#define MFMA16(a, b, c) OMLM_MFMA_32x32x16(a, b, c)

// [rows][64 dims] bf16 tile, 128 B per row; 16-B chunk index XOR ((row >> 1) & 7)   (same image as attention.hip)
__device__ __forceinline__ int a2_tile_off(int row, int colbyte) {
    return row * 128 + ((((colbyte >> 4) ^ ((row >> 1) & 7)) << 4) | (colbyte & 15));
}
__device__ __forceinline__ int a2_crow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

__device__ __forceinline__ h16x8 a2_frag_rows(const char* lds, int row0, int s, int lane) {
    return *(const h16x8*)(lds + a2_tile_off(row0 + (lane & 31), (2 * s + (lane >> 5)) * 16));
}
// transposed operand from the BLOCKED image (see attention.hip tile_off_blk): both reads are linear in the lane id
__device__ __forceinline__ h16x8 a2_frag_cols_tr(const char* lds, int row0, int s, int col0, int lane) {
    const char* base = lds + ((((row0 >> 4) + s) << 1) + (col0 >> 5)) * 1024 + lane * 8;
    s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, base));
    s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, base + 512));
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    s16x8 v = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(h16x8, v);
}
__device__ __forceinline__ h16x8 a2_pack(const f32x16& p, int s) {
    u32x4 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = pack_h16_rne(p[8 * s + 2 * e], p[8 * s + 2 * e + 1]);
    return __builtin_bit_cast(h16x8, h);
}

// ---- bias table [N, ld] (row = i - j, column = head) -> transposed, padded, pre-multiplied by log2 e: [H8][ldT] ----------
// One workgroup per head.  With a bound on |q.k| (qk_max, from the learned scales or given) the fixed reference point
// m_h = c qk_max + max_r table_h[r] - p_max_log2 is subtracted from every entry (pads included) and written to the row's tail
// [ldT - 2] = 1.0 (flag), [ldT - 1] = m_h; without a bound, or if the exponent range could leave the operand type's normal range, the
// flag is 0.  The decision is the SAME for every head (it looks at the widest head's range): the forward picks its kernel by it.
//   p_max_log2: the largest probability numerator is 2^p_max_log2.  0 for bf16 / fp32 operands (numerators <= 1, fp32's exponent range
//   below); 15 for IEEE half, whose normal range is 2^-14 .. 2^15.99: numerators in (2^-13, 2^15] while 2 c qk_max + range < 28.
// (round 6) grid.y = layers: every layer's table in ONE launch -- the tables of a forward differ only through their layer's learned scales, and
// six launches of 8 workgroups were 6 x 14 us of latency per step (omlm_attn_bias_prepare_group; the single-layer entry passes one layer).
// PFX (non-causal prefix, off = min(P, N) - 1 > 0): bias points at the rel = 0 row of a table that also holds rel = -off .. -1 in front; the
// prepared row holds them at [A2_PAD, A2_PAD + off) (entry A2_PAD + off + rel), and they count for the maximum and the range.
#define A2_PREP_MAX 32
struct A2PrepGroup { float* out[A2_PREP_MAX]; const float* qs[A2_PREP_MAX]; const float* ks[A2_PREP_MAX]; };
template <bool PFX = false>
__global__ void attn2_bias_prep_kernel(const float* __restrict__ bias, A2PrepGroup grp, int N, int H, int ld, int ldT,
                                       float qk_bound, float c, int p_max_log2, int off) {
    __shared__ float red[4][2][8];
    __shared__ float redq[4];
    const int h = blockIdx.x, t = threadIdx.x;
    float* biasT = grp.out[blockIdx.y];
    const float* q_scale = grp.qs[blockIdx.y];
    const float* k_scale = grp.ks[blockIdx.y];
    float* row = biasT + (size_t)h * ldT;
    const bool has = bias && h < H;
    // every head's extremes (8 heads per pass): the widest range decides for all, this head's maximum sets its reference point
    float wide = 0.f, own_max = 0.f;
    if (bias) {
        for (int hb = 0; hb < H; hb += 8) {
            float mx[8], mn[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { mx[j] = -3.0e38f; mn[j] = 3.0e38f; }
            for (int r = PFX ? t - off : t; r < N; r += 256) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float x = hb + j < H ? bias[(PFX ? (ptrdiff_t)r : (size_t)r) * ld + hb + j] * A2_LOG2E : 0.f;
                    mx[j] = fmaxf(mx[j], x); mn[j] = fminf(mn[j], x);
                }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float a = wave_max(mx[j]), b = -wave_max(-mn[j]);
                if ((t & 63) == 0) { red[t >> 6][0][j] = a; red[t >> 6][1][j] = b; }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (hb + j < H) {
                    const float a = fmaxf(fmaxf(red[0][0][j], red[1][0][j]), fmaxf(red[2][0][j], red[3][0][j]));
                    const float b = fminf(fminf(red[0][1][j], red[1][1][j]), fminf(red[2][1][j], red[3][1][j]));
                    wide = fmaxf(wide, a - b);
                    if (hb + j == h) own_max = a;
                }
            }
        }
    }
    float qk = qk_bound;
    if (q_scale && k_scale) {
        qk = t < 64 ? fabsf(q_scale[t] * k_scale[t]) : 0.f;
        qk = wave_max(qk);
        if ((t & 63) == 0) redq[t >> 6] = qk;
        __syncthreads();
        qk = redq[0];
    }
    const float B = c * qk;
    // all exponents lie in [p_max_log2 - (2 B + range), p_max_log2]
    const bool fixed = qk > 0.f && (2.f * B + wide) < (p_max_log2 > 0 ? 13.f + (float)p_max_log2 : 80.f);
    const float m = fixed ? B + own_max - (float)p_max_log2 : 0.f;
    if (PFX) {
        for (int x = t; x < ldT - 2; x += 256) {
            const int r = x - A2_PAD - off;
            const float v = (has && r >= -off && r < N) ? bias[(ptrdiff_t)r * ld + h] * A2_LOG2E : 0.f;
            row[x] = v - m;
        }
    } else
    for (int x = t; x < ldT - 2; x += 256) {
        const int r = x - A2_PAD;
        const float v = (has && r >= 0 && r < N) ? bias[(size_t)r * ld + h] * A2_LOG2E : 0.f;
        row[x] = v - m;
    }
    if (t == 0) { row[ldT - 2] = fixed ? 1.0f : 0.f; row[ldT - 1] = m; }
}

// One LDS-DMA wave-instruction = 1 KiB (64 lanes x 16 B), destination lane-linear (M0 = wave-uniform LDS byte address).
// Issued as inline asm on purpose: with the builtin, hipcc tracks "a pending LDS write" and protects LDS reads it cannot
// prove disjoint with s_waitcnt vmcnt(N) -- one build of this kernel waited for the K tile it had JUST requested in front
// of every first MFMA of a tile (seen in the ISA), i.e. the 3-stage ring ran with zero tiles in flight.  The asm form is
// invisible to that bookkeeping; ordering is by the counted s_waitcnt vmcnt + s_barrier at the top of the tile loop.
typedef u32x4 a2_rsrc;
__device__ __forceinline__ a2_rsrc a2_make_rsrc(const void* p, unsigned bytes) {     // wave-uniform inputs only
    const unsigned long long a = (unsigned long long)p;
    a2_rsrc r;
    r[0] = (unsigned)a; r[1] = (unsigned)(a >> 32) & 0xFFFFu; r[2] = bytes; r[3] = 0x00020000u;
    return r;
}
__device__ __forceinline__ void a2_dma(a2_rsrc rs, unsigned lds_dst, unsigned off) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(off), "s"(lds_dst), "s"(rs) : "memory");
}

struct A2Stager {
    unsigned koff, voff, boff;       // per-lane source byte offsets relative to the tile (key j0) / window start
    int vrow;                        // this lane's key row (0..63) in the V unit it issues
    bool bias_wave;
    __device__ __forceinline__ void init(int wave, int lane, int ldT) {
        {   // K unit `wave`: rows 8 wave + (lane >> 3), slot lane & 7 holds chunk slot ^ ((row >> 1) & 7)
            const int row = 8 * wave + (lane >> 3), ch = (lane & 7) ^ ((row >> 1) & 7);
            koff = (unsigned)(row * 128 + ch * 16);
        }
        {   // V unit `wave` of the blocked image: unit = (row >> 4) * 2 + (col >> 5); lane = p * 8 + (row & 3) * 2 + ((col >> 3) & 1)
            const int p = lane >> 3, rq = ((p >> 2) << 1) | ((p >> 1) & 1);
            vrow = (wave >> 1) * 16 + rq * 4 + ((lane >> 1) & 3);
            const int col = (wave & 1) * 32 + (p & 1) * 16 + (lane & 1) * 8;
            voff = (unsigned)(vrow * 128 + col * 2);
        }
        {   // bias unit (wave & 3): heads 2 u, 2 u + 1; lane = (head & 1) * 32 + float4 index
            const int u = wave & 3, hh = 2 * u + (lane >> 5);
            boff = (unsigned)(((size_t)hh * ldT + 4 * (lane & 31)) * 4);
            bias_wave = wave < 4;
        }
    }
};

// Work item of workgroup `lin`: (sample b, query tile qt, head group hy).  XCD-aware: the workgroups of one sample (they share its K / V
// through the XCD's L2) are dealt to one XCD (workgroup lin runs on XCD lin % 8).  When an XCD's share is whole samples (B a multiple of
// 8), its items run heaviest (latest) query tile first ACROSS its samples -- dealt sample by sample, the last sample's longest items
// started two thirds into the launch and the SIMDs averaged 1.3 of 2 resident waves (forward 94 -> 86 us per layer at B = 32, N = 1116).
__device__ __forceinline__ void a2_item_order(int lin, int nqt, int ny, int B, int& b, int& qt, int& hy) {
    const int per = nqt * ny, total = per * B;
    const int qq = total >> 3, rr = total & 7, xcd = lin & 7, idx = lin >> 3;
    const int start = xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq, cnt = qq + (xcd < rr ? 1 : 0);
    if (start % per == 0 && cnt % per == 0) {
        const int ns = cnt / per, w = idx % (ns * ny);
        qt = nqt - 1 - idx / (ns * ny);
        b = start / per + w / ny;
        hy = w % ny;
    } else {                                                  // sample-major, heavy tiles first inside a sample
        const int lg = start + idx;
        b = lg / per;
        const int rem = lg - b * per;
        qt = nqt - 1 - rem / ny;
        hy = rem % ny;
    }
}

struct A4Acc {
    f32x16 acc[2][2];       // O^T: [head][d tile]
    f32x16 accl;            // denominators; row parity (i & 1) == hb holds those of head hb
    float m[2];             // running max (online form only)
};

// One 64-key tile against the wave's two heads x 32 queries.
//   FIXED: the exponentials are taken against a FIXED reference point instead of a running maximum.  q and k are l2-normalised
//          vectors times learned scales (transformer.py:269-271), so |q.k| <= max_d |q_scale_d k_scale_d| =: qk_max and every
//          score is <= m_h = scale log2(e) qk_max + max_rel bias_h.  omlm_attn_bias_prepare subtracts m_h from the table, so the
//          work per score is ONE fma (score * c + table) and ONE exp2: no row maximum, no cross-lane step, no rescaling of
//          the accumulators, no dependency between blocks other than the MFMA accumulation itself.  The result is the same
//          softmax (numerator and denominator share the factor 2^-m_h); it is only selected while 2 c qk_max + the table's
//          range stays inside the operand type's exponent range (flag in the table's tail), else the online form runs.
//   FULL:  every block of the tile lies strictly below the diagonal: straight-line code, no compares.
//   QSEL >= 0: only head QSEL is processed (the online form walks the heads one at a time: fewer live registers).
//   Addressing: every LDS read of the tile is (one lane-dependent base register) + (compile-time offset) -- the bias window from ONE
//   base below its lowest entry (the 64 window reads of a tile had an address add each), the live vectors from a per-head base that
//   points at the sample's liveness array for the lanes whose accumulator rows belong to that head and at a block of zeros for the
//   others (instead of 32 per-value selects): ~70 of ~260 VALU instructions per tile less in a loop that is VALU-issue bound.
//   DROP: the numerator MFMAs take P with the dropped keys' entries zeroed (attn_drop_pair_mask on the packed pairs; rk: the two heads' row
//   keys, see common.h), the denominator MFMA the undropped P -- the 1 / (1 - p) scale is applied with 1 / denominator at the store.
//   PFX: the non-causal prefix of Pn rows (include/omlm.h): keys up to kend = max(i0 + 32, Pn) for a query tile inside it, and the blocks
//   not wholly below the diagonal keep (i, j) iff j <= i or i, j < Pn.
//   lb (online form): the tile's liveness ballot (uniform); the scores of a tile's dead keys start from A2_MASKED, so that the running
//   maximum is taken over live keys only.
template <bool FIXED, bool FULL, int QSEL = -1, bool DROP = false, bool PFX = false>
__device__ __forceinline__ void a4_tile(A4Acc& A, const h16x8 (&qf)[2][4], const char* Ks, const h16_t* live0, const h16_t* live1,
                                        float c, int i0, int j0, int wave, int lane, const unsigned (&rk)[2], unsigned thr16, int kend = 0,
                                        int Pn = 0, unsigned long long lb = ~0ull) {
    const char* Vs = Ks + 8192;
    const int hi = lane >> 5, ql = lane & 31;
    // window index of (head hb, query ql, key 32 sub + 4 hi + cr): hb 128 + 64 + ql - 32 sub - 4 hi - cr, cr = crow(r, 0) <= 27
    // (the base as ONE opaque LDS address: hipcc otherwise folds the stage's 16 KB offset into each read's constant, past the offset field)
    unsigned bbo = (unsigned)(size_t)LDS_PTR(const float, (const float*)(Ks + 16384) + 2 * wave * A2_BWIN + ql - 4 * hi);
    asm volatile("" : "+v"(bbo));
    const __attribute__((address_space(3))) float* bb = (const __attribute__((address_space(3))) float*)(size_t)bbo;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
        const int jb = j0 + 32 * sub;
        if (!FULL && jb > (PFX ? kend - 1 : i0 + 31)) break;    // above the diagonal (PFX: past the prefix) for every query of the workgroup
        h16x8 kf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) kf[s] = a2_frag_rows(Ks, 32 * sub, s, lane);
        h16x8 pb[2][2];
        const bool diag = !FULL && !(jb + 31 <= i0);
        const int d0 = (i0 + ql) - (jb + 4 * hi);
        const bool qpre = PFX && i0 + ql < Pn;                  // PFX: this lane's query row lies in the prefix
        // lb: the tile's ballot word (uniform).  A masked key (or one past N) must not set the running maximum: neither sum takes its P,
        // but the live keys' exp2(s - m) would sit that far lower -- 14 octaves under a masked score they leave half's normal range, 24
        // under they are zero and the row comes out as one without a live key.  A tile with a dead key therefore starts its scores from
        // a rank-one product, (A2_MASKED per dead key) x (1 per query), in k-slot 0 of ONE extra MFMA per head: no work per score.
        const bool masked = !FIXED && lb != ~0ull;
        h16x8 mka, mkb;
        if (masked) {
            const unsigned w = (unsigned)(lb >> (32 * sub));
            u32x4 ua = {0u, 0u, 0u, 0u}, ub = {0u, 0u, 0u, 0u};
            ua[0] = (hi == 0 && !((w >> ql) & 1u)) ? A2_MASKED_BITS : 0u;      // A rows are keys 32 sub + ql
            ub[0] = hi == 0 ? A2_ONE_BITS : 0u;
            mka = __builtin_bit_cast(h16x8, ua);
            mkb = __builtin_bit_cast(h16x8, ub);
        }
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            if (QSEL >= 0 && hb != QSEL) continue;
            f32x16 st;
#pragma unroll
            for (int e = 0; e < 16; ++e) st[e] = 0.f;
            if (masked) st = MFMA16(mka, mkb, st);              // + A2_MASKED for the tile's dead keys, every query alike
#pragma unroll
            for (int s = 0; s < 4; ++s) st = MFMA16(kf[s], qf[hb][s], st);
            const __attribute__((address_space(3))) float* bp = bb + (hb * A2_BWIN + 64 - 32 * sub - 27);       // entries [27 - cr]: offsets >= 0
            if (FIXED) {
                if (!diag) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) st[r] = __builtin_amdgcn_exp2f(st[r] * c + bp[27 - ((r & 3) + 8 * (r >> 2))]);
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int cr = (r & 3) + 8 * (r >> 2);
                        const float e2 = __builtin_amdgcn_exp2f(st[r] * c + bp[27 - cr]);
                        st[r] = (d0 - cr >= 0 || (qpre && jb + 4 * hi + cr < Pn)) ? e2 : 0.f;
                    }
                }
            } else {
                float mloc = A2_NEG;
                if (!diag) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        st[r] = st[r] * c + bp[27 - ((r & 3) + 8 * (r >> 2))];
                        mloc = fmaxf(mloc, st[r]);
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int cr = (r & 3) + 8 * (r >> 2);
                        const float val = st[r] * c + bp[27 - cr];
                        st[r] = (d0 - cr >= 0 || (qpre && jb + 4 * hi + cr < Pn)) ? val : A2_NEG;
                        mloc = fmaxf(mloc, st[r]);
                    }
                }
                mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
                const float mnew = fmaxf(A.m[hb], mloc);
                const float alpha = __builtin_amdgcn_exp2f(A.m[hb] - mnew);
                A.m[hb] = mnew;
                // no live key yet (a masked score is about A2_MASKED c, one above the diagonal A2_NEG): the excluded scores must come out as
                // 0, not as exp2(0) = 1 -- the denominator's live vector covers the masked keys, but not the live ones above the diagonal
                const float msub = mnew > A2_DEAD * c ? mnew : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) st[r] = __builtin_amdgcn_exp2f(st[r] - msub);
                if (!__all(alpha == 1.0f)) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) { A.acc[hb][0][e] *= alpha; A.acc[hb][1][e] *= alpha; }
                    A.accl[hb] *= alpha;                        // rows 0/4 (head 0) and 1/5 (head 1) are the ones read
                }
            }
            pb[hb][0] = a2_pack(st, 0);
            pb[hb][1] = a2_pack(st, 1);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const h16x8 va0 = a2_frag_cols_tr(Vs, 32 * sub, s, 0, lane);
            const h16x8 va1 = a2_frag_cols_tr(Vs, 32 * sub, s, 32, lane);
#pragma unroll
            for (int hb = 0; hb < 2; ++hb) {
                if (QSEL >= 0 && hb != QSEL) continue;
                // live vector of the 16 keys of this k-step in MFMA k order: keys key0 + 4 hi + {0..3}, key0 + 8 + 4 hi + {0..3}; the
                // A rows of parity hb carry it for head hb, the others zeros: ONE denominator accumulator for both heads
                const h16_t* lp = (hb ? live1 : live0) + 32 * sub + 16 * s;
                const u32x2 l0 = *(const u32x2*)lp, l1 = *(const u32x2*)(lp + 8);
                u32x4 lv4;
                lv4[0] = l0[0]; lv4[1] = l0[1]; lv4[2] = l1[0]; lv4[3] = l1[1];
                h16x8 pn = pb[hb][s];
                if (DROP) {                                     // pair e holds keys jb + 4 hi + 16 s + 8 (e >> 1) + 2 (e & 1) + {0, 1}
                    u32x4 u = __builtin_bit_cast(u32x4, pn);
                    const unsigned kb = rk[hb] ^ (unsigned)(jb >> 1);
#pragma unroll
                    for (int e = 0; e < 4; ++e) u[e] &= attn_drop_pair_mask(omlm_hash32(kb ^ (unsigned)(8 * s + 4 * (e >> 1) + (e & 1))), thr16);
                    pn = __builtin_bit_cast(h16x8, u);
                }
                A.acc[hb][0] = MFMA16(va0, pn, A.acc[hb][0]);
                A.acc[hb][1] = MFMA16(va1, pn, A.acc[hb][1]);
                A.accl = MFMA16(__builtin_bit_cast(h16x8, lv4), pb[hb][s], A.accl);      // sum over live keys of P
            }
        }
    }
}

// Forward: one workgroup = 4 waves = 8 heads x 32 queries of one sample, each wave TWO heads; two workgroups per CU (63 KB of LDS,
// <= 256 registers).  Against the 8-wave form it replaces (one head per wave, one workgroup per CU: 122 us -> 95 us per layer at B = 32,
// N = 1116 with half operands):
//   * the K fragments and the V (transposed) fragments of a 32-key block are read from LDS once for two heads, and a wave has four
//     independent (head, key block) chains for the scheduler to interleave exponentials with MFMAs;
//   * the two waves of a SIMD belong to different workgroups, so they do not meet at the same barrier -- with 8 waves in one workgroup
//     both waves of a SIMD ran the same phase of the same tile at the same time (both want the VALU, then both want the matrix pipe), and
//     a workgroup's prologue / epilogue (~3 dependent round trips) had nothing to hide behind.
#define A4_THREADS 256
struct A4Stager {
    unsigned koff[2], voff[2], boff;     // per-lane source byte offsets of the wave's two K units, two V units, one bias unit
    int vrow[2];
    // Recomputed from the lane id at every use (a dozen integer ops per tile): kept across the tile loop these seven registers were
    // spilled (the tile body wants all 256), and hipcc puts s_waitcnt vmcnt(0) behind a scratch reload -- which drains the DMA ring.
    __device__ __forceinline__ void init(int wave, int lane, int ldT) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int unit = 2 * wave + u;
            {   // K unit: rows 8 unit + (lane >> 3), slot lane & 7 holds chunk slot ^ ((row >> 1) & 7)
                const int row = 8 * unit + (lane >> 3), ch = (lane & 7) ^ ((row >> 1) & 7);
                koff[u] = (unsigned)(row * 128 + ch * 16);
            }
            {   // V unit of the blocked image (see A2Stager)
                const int p = lane >> 3, rq = ((p >> 2) << 1) | ((p >> 1) & 1);
                vrow[u] = (unit >> 1) * 16 + rq * 4 + ((lane >> 1) & 3);
                const int col = (unit & 1) * 32 + (p & 1) * 16 + (lane & 1) * 8;
                voff[u] = (unsigned)(vrow[u] * 128 + col * 2);
            }
        }
        const int hh = 2 * wave + (lane >> 5);                   // bias unit `wave`: heads 2 wave, 2 wave + 1
        boff = (unsigned)(((size_t)hh * ldT + 4 * (lane & 31)) * 4);
    }
};

// FIXED is a template parameter of the KERNEL, and both instances are launched: which softmax form applies is known on the device only
// (the flag in the table's tail, omlm_attn_bias_prepare), and the instance the flag does not name returns at its first instruction
// (~3 us per layer).  One kernel holding both forms was tried: at 256 registers it either spilled ~20 loop-invariant registers -- hipcc
// waits vmcnt(0) behind every scratch reload, which drains the DMA ring -- or, with the online form walking its heads one at a time, kept
// the fixed form 10 % slower than this split (103 vs 92 us).
//   FIXED: both heads in one straight line.  Online (more live state: running maxima, rescale factors): the two heads one after the
//   other (QSEL), re-reading the K / V fragments per head.
// PFX: the non-causal prefix of Pn = min(P, N) rows; the table (omlm_attn_bias_prepare_group with P >= 1) holds Pn - 1 negative distances in
// front of the causal layout, so every window offset moves by off = Pn - 1.
#define A4_KERNEL attn4_fwd_kernel
#define A4_LONG false
#include "attention2_fwd.inc"
#undef A4_KERNEL
#undef A4_LONG
#define A4_KERNEL attn4_fwd_long_kernel
#define A4_LONG true
#include "attention2_fwd.inc"
#undef A4_KERNEL
#undef A4_LONG

// =========================================================================================================================
// backward, dQ / d(bias) / delta kernel on the same skeleton: 8 heads x 32 queries per workgroup, 64-key tiles through the
// 3-stage LDS-DMA ring -- per stage K as rows (S^T = K Q^T), K blocked (dQ^T += K^T dS^T), V as rows (dP^T = V dO^T) and the
// bias window.  The key mask is an additive 0 / -1e30 vector in LDS (one aligned 16-byte read per 4 scores); the probabilities
// come straight from the stored log-sum-exp (no maximum to track), so the blocks of a tile are independent.
#define A2B_STAGE (3 * 8192 + 8 * A2_BWIN * 4)       /* 28 KiB */
// PFX: the non-causal prefix (see attn4_fwd_kernel); the d(bias) bins of the negative distances sit in front of each wave's bins and leave
// by atomics into dbias (which points at the rel = 0 row).
#define A2_BINW 128          /* d(bias) bins per wave of the long form's ring */
#define A2Q_KERNEL attn2_bwd_dq_kernel
#define A2Q_LONG false
#include "attention2_dq.inc"
#undef A2Q_KERNEL
#undef A2Q_LONG
#define A2Q_KERNEL attn2_bwd_dq_long_kernel
#define A2Q_LONG true
#include "attention2_dq.inc"
#undef A2Q_KERNEL
#undef A2Q_LONG

static_assert(A2_NST * A2B_STAGE == omlm_plan::A2Q_RING && A2_BINW == omlm_plan::A2Q_BINW, "attn_plan.h states the dQ kernel's ring and bins");

// one ATTN_A2_DQ launch of the plan (Pn > 0: the non-causal prefix's PFX instances; the long form is causal)
void attn2_bwd_dq_launch(const omlm_plan::AttnLaunch& l, int ldT, const void* q, const void* k, const void* v, const float* biasT,
                         const unsigned char* keymask, const void* out, const void* dout, const float* lse, float* delta, float* dq,
                         float* dbias, int bias_ld, float* dpart, int B, int N, int H, float scale, hipStream_t st, const AttnDrop& dr, int Pn) {
    auto go = [&](auto launch) {
        launch(dim3(l.gx), dim3(l.threads), l.lds, st, (const h16_t*)q, (const h16_t*)k, (const h16_t*)v, biasT, ldT, keymask, (const h16_t*)out,
               (const h16_t*)dout, lse, delta, dq, dbias, bias_ld, dpart, B, N, H, scale, dr, Pn);
    };
    if (l.form == omlm_plan::ATTN_FORM_LONG) {
        if (l.drop) go([](auto... a) { launch_lds_cap<attn2_bwd_dq_long_kernel<true>>(a...); });
        else go([](auto... a) { launch_lds_cap<attn2_bwd_dq_long_kernel<false>>(a...); });
    } else
        with_flags(l.drop, l.pfx, [&](auto D, auto P) {
            go([](auto... a) { launch_lds_cap<attn2_bwd_dq_kernel<decltype(D)::value, decltype(P)::value>>(a...); });
        });
}

#if !OMLM_FP16      /* the bias table is fp32 in every precision: prepared by the bf16 copy of this file */
// -------------------------------------------------------------------------------------------------------------------------
// the prepared table of a prefix of P rows (0: causal): the min(P, N) - 1 negative distances in front of the causal layout
extern "C" long long omlm_attn_bias_table_floats(int N, int H, int P) {
    return omlm_plan::attn_bias_table_floats(N, H, P);
}

// biasT: omlm_attn_bias_table_floats(N, H, 0) floats.  bias may be null (no rel-pos bias).  q_scale / k_scale (64 floats each, optional):
// the learned per-dim scales applied after the l2 normalisation -- they give the bound max_d |q_scale_d k_scale_d| on |q.k| that
// selects the fixed-reference softmax; alternatively qk_bound > 0 states the bound directly (callers with unit q, k: 1.0);
// neither: online softmax.  scale: the attention scale (8).  p_max_log2: 0 for bf16 / fp32 attention operands, 15 for half operands (the
// fixed reference point is lowered by 15 so that the probability numerators use half's normal range; see attn2_bias_prep_kernel).
extern "C" int omlm_attn_bias_prepare(const float* bias, float* biasT, int N, int H, int bias_ld, const float* q_scale,
                                      const float* k_scale, float qk_bound, float scale, int p_max_log2, void* stream) {
    OMLM_CHECK_ARG(biasT && N > 0 && H > 0, "null table / sizes");
    OMLM_CHECK_ARG(p_max_log2 == 0 || p_max_log2 == 15, "p_max_log2: 0 (bf16 / fp32 operands) or 15 (half operands)");
    const int ldT = omlm_plan::attn_ldT(N, 0), H8 = (H + 7) / 8 * 8;
    A2PrepGroup grp;
    memset(&grp, 0, sizeof(grp));
    grp.out[0] = biasT; grp.qs[0] = q_scale; grp.ks[0] = k_scale;
    hipLaunchKernelGGL(attn2_bias_prep_kernel<false>, dim3(H8, 1), dim3(256), 0, as_stream(stream), bias, grp, N, H, bias_ld, ldT,
                       qk_bound, scale * A2_LOG2E, p_max_log2, 0);
    return omlm_post_launch("omlm_attn_bias_prepare");
}
// The tables of `layers` attention layers over ONE rel-pos table in one launch: biasT[l] (omlm_attn_bias_table_floats(N, H, P) floats each) from
// the layer's learned scales q_scale[l] / k_scale[l] (64 floats each; all given, or all NULL with qk_bound as in omlm_attn_bias_prepare).
// biasT / q_scale / k_scale: HOST arrays of device pointers.  P >= 1: the non-causal prefix's table (bias: [N + min(P, N) - 1, bias_ld] from
// its first row).
extern "C" int omlm_attn_bias_prepare_group(const float* bias, float* const* biasT, int layers, int N, int H, int bias_ld,
                                            const float* const* q_scale, const float* const* k_scale, float qk_bound, float scale,
                                            int p_max_log2, int P, void* stream) {
    OMLM_CHECK_ARG(P >= 0, "prefix rows P >= 0");
    if (layers <= 0) return OMLM_OK;
    OMLM_CHECK_ARG(biasT && N > 0 && H > 0, "null table / sizes");
    OMLM_CHECK_ARG(p_max_log2 == 0 || p_max_log2 == 15, "p_max_log2: 0 (bf16 / fp32 operands) or 15 (half operands)");
    OMLM_CHECK_ARG((q_scale == nullptr) == (k_scale == nullptr), "q_scale and k_scale: both or neither");
    const int off = omlm_plan::attn_prefix_off(N, P);
    if (bias && off > 0) bias += (size_t)off * bias_ld;      // the kernel reads rows -off .. N - 1 around the rel = 0 row
    const int ldT = omlm_plan::attn_ldT(N, P), H8 = (H + 7) / 8 * 8;
    for (int base = 0; base < layers; base += A2_PREP_MAX) {
        const int n = layers - base < A2_PREP_MAX ? layers - base : A2_PREP_MAX;
        A2PrepGroup grp;
        memset(&grp, 0, sizeof(grp));
        for (int l = 0; l < n; ++l) {
            OMLM_CHECK_ARG(biasT[base + l], "null table");
            grp.out[l] = biasT[base + l];
            grp.qs[l] = q_scale ? q_scale[base + l] : nullptr;
            grp.ks[l] = k_scale ? k_scale[base + l] : nullptr;
        }
        hipLaunchKernelGGL(P > 0 ? attn2_bias_prep_kernel<true> : attn2_bias_prep_kernel<false>, dim3(H8, n), dim3(256), 0, as_stream(stream),
                           bias, grp, N, H, bias_ld, ldT, qk_bound, scale * A2_LOG2E, p_max_log2, off);
    }
    return omlm_post_launch("omlm_attn_bias_prepare_group");
}

// d(bias) partial rows -> the [N, bias_ld] table.  The dQ kernels leave one fp32 row of nqt*32 bins per (sample, head, query tile) in
// the workspace (bins [0, 32 (qt + 1)) of row qt are written; the rest is never read); a thread here owns one (bin, head) and adds
// the rows of every S-th sample down its column -- coalesced along the bins -- then one atomic per thread folds the S sample groups.
#define A2_DBR_S 8
__global__ __launch_bounds__(256) void attn_dbias_reduce_kernel(const float* __restrict__ dpart, float* __restrict__ dbias, int bias_ld,
                                                                int B, int N, int H, int nqt) {
    const int r = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y, s = blockIdx.z;
    if (r >= N) return;
    const size_t NB = (size_t)nqt * 32;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int b = s; b < B; b += A2_DBR_S) {
        const float* col = dpart + ((size_t)b * H + h) * nqt * NB + r;
        int qt = r >> 5;
        for (; qt + 4 <= nqt; qt += 4) {
            a0 += col[(size_t)qt * NB];
            a1 += col[(size_t)(qt + 1) * NB];
            a2 += col[(size_t)(qt + 2) * NB];
            a3 += col[(size_t)(qt + 3) * NB];
        }
        for (; qt < nqt; ++qt) a0 += col[(size_t)qt * NB];
    }
    const float t = (a0 + a1) + (a2 + a3);
    if (t != 0.f) unsafeAtomicAdd(dbias + (size_t)r * bias_ld + h, t);
}

// include/omlm.h (csrc/attn_plan.h: the d(bias) rows, past N = 4096 followed by the dK / dV kernel's slots)
extern "C" long long omlm_mqa_attn_bwd_workspace_bytes(int B, int N, int H) { return omlm_plan::attn_bwd_workspace_bytes(B, N, H); }

extern "C" __attribute__((visibility("hidden"))) void omlm_attn_dbias_reduce_launch(const omlm_plan::AttnLaunch* l, const float* dpart, float* dbias, int bias_ld, int B, int N, int H, void* stream) {
    hipLaunchKernelGGL(attn_dbias_reduce_kernel, dim3(l->gx, l->gy, l->gz), dim3(l->threads), 0, as_stream(stream), dpart, dbias, bias_ld, B, N, H, (N + 31) / 32);
}

// ---- attention dropout: the keep-mask the attention kernels apply, written out (a test / integration hook), and the to_out dropout ------
__global__ __launch_bounds__(256) void attn_dropout_keep_kernel(unsigned char* __restrict__ keep, int B, int N, int H, const AttnDrop d) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x, n = (long long)B * H * N * N;
    if (e >= n) return;
    const int j = (int)(e % N), i = (int)((e / N) % N), h = (int)((e / ((long long)N * N)) % H), b = (int)(e / ((long long)N * N * H));
    const unsigned w = omlm_hash32(attn_drop_headkey(attn_drop_seed(d), b, h) ^ ((unsigned)i << 15) ^ ((unsigned)j >> 1));
    keep[e] = ((w << ((j & 1) ? 0 : 16)) >= d.thr16) ? 1 : 0;
}
extern "C" int omlm_attn_dropout_keep(unsigned char* keep, int B, int N, int H, float p, unsigned long long seed,
                                      const unsigned long long* seed_dev, void* stream) {
    if (B <= 0 || N <= 0 || H <= 0) return OMLM_OK;
    AttnDrop d;
    OMLM_CHECK_ARG(keep, "null pointer");
    OMLM_CHECK_ARG(attn_drop_args(p, seed, seed_dev, d), "dropout p in [0, 1)");
    const long long n = (long long)B * H * N * N;
    hipLaunchKernelGGL(attn_dropout_keep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), keep, B, N, H, d);
    return omlm_post_launch("omlm_attn_dropout_keep");
}

// to_out dropout, keyed by (seed'', row, column): the draws of columns c (even) and c + 1 are the low and high halves of
// omlm_hash32(omlm_hash32(omlm_hash32(lo32(seed'') ^ row) ^ hi32(seed'')) ^ (c >> 1)).  One thread per column pair.
__device__ __forceinline__ unsigned resid_drop_word(unsigned long long s, long long row, int c) {
    const unsigned rk = omlm_hash32(omlm_hash32((unsigned)s ^ (unsigned)row) ^ (unsigned)(s >> 32));
    return omlm_hash32(rk ^ ((unsigned)c >> 1));
}
__global__ __launch_bounds__(256) void dropout_residual_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ x1,
                                                                   long long M, int D, const AttnDrop d) {
    const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 2;
    if (e >= M * D) return;
    const long long row = e / D;
    const int c = (int)(e - row * D);
    const unsigned w = resid_drop_word(attn_drop_seed(d), row, c);
    const float2 xv = *(const float2*)(x + e), yv = *(const float2*)(y + e);
    const float z0 = (w << 16) >= d.thr16 ? d.rs : 0.f, z1 = w >= d.thr16 ? d.rs : 0.f;
    *(float2*)(x1 + e) = make_float2(xv.x + z0 * yv.x, xv.y + z1 * yv.y);
}
template <typename TO>
__global__ __launch_bounds__(256) void dropout_residual_bwd_kernel(const float* __restrict__ dx1, TO* __restrict__ dy, long long M, int D,
                                                                   const AttnDrop d) {
    const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 2;
    if (e >= M * D) return;
    const long long row = e / D;
    const int c = (int)(e - row * D);
    const unsigned w = resid_drop_word(attn_drop_seed(d), row, c);
    const float2 g = *(const float2*)(dx1 + e);
    store_from_float(dy + e, (w << 16) >= d.thr16 ? g.x * d.rs : 0.f);
    store_from_float(dy + e + 1, w >= d.thr16 ? g.y * d.rs : 0.f);
}
extern "C" int omlm_dropout_residual_fwd(const float* x, const float* y, float* x1, long long M, int D, float p, unsigned long long seed,
                                         const unsigned long long* seed_dev, void* stream) {
    if (M <= 0 || D <= 0) return OMLM_OK;
    AttnDrop d;
    OMLM_CHECK_ARG(x && y && x1, "null pointer");
    OMLM_CHECK_ARG(D % 2 == 0, "D even");
    OMLM_CHECK_ARG(attn_drop_args(p, seed, seed_dev, d), "dropout p in [0, 1)");
    const long long pairs = M * D / 2;
    hipLaunchKernelGGL(dropout_residual_fwd_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, as_stream(stream), x, y, x1, M, D, d);
    return omlm_post_launch("omlm_dropout_residual_fwd");
}
extern "C" int omlm_dropout_residual_bwd(const float* dx1, void* dy, long long M, int D, float p, unsigned long long seed,
                                         const unsigned long long* seed_dev, int out_dtype, void* stream) {
    if (M <= 0 || D <= 0) return OMLM_OK;
    AttnDrop d;
    OMLM_CHECK_ARG(dx1 && dy, "null pointer");
    OMLM_CHECK_ARG(D % 2 == 0, "D even");
    OMLM_CHECK_ARG(out_dtype >= 0 && out_dtype <= 2, "dtype");
    OMLM_CHECK_ARG(attn_drop_args(p, seed, seed_dev, d), "dropout p in [0, 1)");
    const long long pairs = M * D / 2;
    const dim3 grid((unsigned)((pairs + 255) / 256));
    if (out_dtype == OMLM_DT_F32) hipLaunchKernelGGL(dropout_residual_bwd_kernel<float>, grid, dim3(256), 0, as_stream(stream), dx1, (float*)dy, M, D, d);
    else if (out_dtype == OMLM_DT_BF16) hipLaunchKernelGGL(dropout_residual_bwd_kernel<h16_t>, grid, dim3(256), 0, as_stream(stream), dx1, (h16_t*)dy, M, D, d);
    else hipLaunchKernelGGL(dropout_residual_bwd_kernel<f16_t>, grid, dim3(256), 0, as_stream(stream), dx1, (f16_t*)dy, M, D, d);
    return omlm_post_launch("omlm_dropout_residual_bwd");
}

#endif

// one ATTN_A4_FWD launch of the plan: FIXED or online (both are launched where there is a table: the one its flag does not name returns at its
// first instruction), DROP, and for the short form PFX (the non-causal prefix; the long form is causal)
void attn2_fwd_launch(const omlm_plan::AttnLaunch& l, int ldT, const void* q, const void* k, const void* v, const float* biasT,
                      const unsigned char* keymask, void* out, float* lse, int B, int N, int H, float scale, hipStream_t st, const AttnDrop& dr, int Pn) {
    auto go = [&](auto launch) {
        launch(dim3(l.gx), dim3(l.threads), l.lds, st, (const h16_t*)q, (const h16_t*)k, (const h16_t*)v, biasT, ldT, keymask, (h16_t*)out, lse,
               B, N, H, scale, dr, Pn);
    };
    with_flags(l.fixed, l.drop, [&](auto F, auto D) {
        constexpr bool FIXED = decltype(F)::value, DROP = decltype(D)::value;
        if (l.form == omlm_plan::ATTN_FORM_LONG) go([](auto... a) { launch_lds_cap<attn4_fwd_long_kernel<FIXED, DROP>>(a...); });
        else if (l.pfx) go([](auto... a) { launch_lds_cap<attn4_fwd_kernel<FIXED, DROP, true>>(a...); });
        else go([](auto... a) { launch_lds_cap<attn4_fwd_kernel<FIXED, DROP>>(a...); });
    });
}

}   // namespace OMLM_NS
