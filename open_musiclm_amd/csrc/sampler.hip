// The fused sampler of the AR loop: the wave and workgroup kernels, one launcher, and the C entry points over them.
#include "common.h"
#include <string.h>
#include <math.h>

// ---------------------------------------------------------------------------------------------------------
// fused sampler of the AR loop (open_musiclm.py:309-316; utils.py:65-84): last-position logits [B, V] ->
//   eos logit -> -inf (unless allowed), keep the k = max(int((1-thres) V), 1) largest logits, argmax(l / T + Gumbel(u)).
// One workgroup per row; V <= 2048.  The k-th largest value is found by a bitwise radix descent on the
// order-preserving integer image of the floats (exact, no sort).  Tie rule (this library's own, deterministic): every entry strictly
// above the k-th largest value is kept and, of the entries equal to it, the LOWEST indices until exactly k are kept.  (torch.topk
// also keeps exactly k entries but promises no order among equals: on tied rows its kept set differs from this one.)  The id is the
// first maximum of l / T + Gumbel(u) over the kept entries; index 0 when every kept entry is -inf (as argmax of an all -inf row).
__device__ __forceinline__ unsigned f_ord(float f) { unsigned u = f2u(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }

// One WAVE per row: the row's logits sit in registers (V <= 2048 -> <= 32 per lane, element c = lane + 64 j), every count of the
// radix descent is a ballot + popcount on the scalar unit -- no LDS, no barrier.  (The first version used 256 threads, an LDS
// image and two barriers per bit: ~25 us of the ~200 us a sampled id costs at B = 1.)  Optionally gathers the embedding row of the
// sampled id (open_musiclm.py:123-134: id + quantizer offset) into x, so the decode step needs no separate gather launch.
// SAMPLE_NV (template): register slots per lane, 17 for V <= 1088 (the 1025-entry heads of every shipped model), 32 up to 2048.  A
// single wave is a serial instruction stream (~5-8 cycles per dependent instruction): the round-4 trace showed 43.9 us per call with the
// slot loops unrolled to 32 behind `j < nv` branches (32 bits x 32 slots of compare / branch / count), so the slot count is a compile-time
// constant and the descent stops at the first threshold that cuts exactly k keys.
//
// The uniforms come from one of two sources, chosen at compile time (RNG, as the attention kernels take DROP):
//   RNG = false: a buffer `uniform` [B, V] ([steps, B, V] with step_dev) -- how the golden id tests inject the reference's draws;
//   RNG = true:  the counter stream stated in include/omlm.h, u(t, b, c) a pure function of a 64-bit seed, the step t (*step_dev, or the
//                host's `step`), the global sample index b = row0 + row and the logit index c.  No pointer, no load: the per-row key
//                is hoisted (a handful of scalar hashes) and ONE hash per element is left in the slot loop, next to its two logs.
// Both are the same function of (logits, u): everything but the origin of u is the same code.
//
// The nucleus (NUC, a third compile-time choice; the function is stated in include/omlm.h): a SECOND selection over the keys already on
// chip, which tightens the top-k pair (t, number of tied entries kept) to (t_p, n_p); the scoring pass then runs on the new pair.  The
// masses are 64-bit integers q = floor(w 2^40), w = exp((l - m) / T) from ONE function (nucleus_q) of the key's inverse image: integer adds
// commute, so ballots, shuffles and LDS adds give the same sums in any order and in either kernel.  NUC = false takes the argument types
// of the parent (a pointer / SampleStream), NUC = true the same with top_p appended, so the existing instantiations keep their kernarg
// layout: they are compared with the parent's instruction for instruction (profiles/sampler_top_p.md section 1).
struct SampleStream { unsigned seed_lo, seed_hi; int step, row0; };
struct SampleBufferP { const float* u; float top_p; };
struct SampleStreamP { SampleStream s; float top_p; };
template <bool RNG, bool NUC = false> struct sample_src { typedef const float* __restrict__ type; };
template <> struct sample_src<true, false> { typedef SampleStream type; };
template <> struct sample_src<false, true> { typedef SampleBufferP type; };
template <> struct sample_src<true, true> { typedef SampleStreamP type; };
// per source: the row's uniforms (buffer) / the row's key (stream: t = *step_dev or the host's step, b = row0 + row).  Overloads, not
// `if constexpr` around an assignment: the buffer form must still read `const float* ur = uniform + row * V` as ONE initialisation --
// with `ur = nullptr; if constexpr (RNG) ...; else ur = ...` hipcc emitted the three wide RNG = false instantiations with two
// independent v_cndmask of the bin scan in the other order (profiles/sampler_stream.md section 1 compares them with the parent's).
__device__ __forceinline__ const float* sample_row_uniforms(const float* uniform, size_t offset) { return uniform + offset; }
__device__ __forceinline__ const float* sample_row_uniforms(const SampleStream&, size_t) { return nullptr; }
__device__ __forceinline__ unsigned sample_row_key(const float*, const int*, int) { return 0u; }
__device__ __forceinline__ unsigned sample_row_key(const SampleStream& s, const int* step_dev, int row) {
    const unsigned t = (unsigned)(step_dev ? step_dev[0] : s.step), b = (unsigned)(s.row0 + row);
    const unsigned s0 = omlm_hash32(omlm_hash32(s.seed_lo) ^ s.seed_hi);      // the seed is hashed BEFORE t is added: otherwise seeds s and
    return omlm_hash32(omlm_hash32(s0 + t * 0x9E3779B9u) ^ (b * 0x85EBCA6Bu));   // s ^ 1 are one stream with steps swapped pairwise
}
__device__ __forceinline__ float sample_stream_u(unsigned key, unsigned c) {      // 24-bit grid in [0, 1): exact in fp32
    return (float)(omlm_hash32(key ^ (c * 0x9E3779B9u)) >> 8) * 0x1p-24f;
}
// NUC = true: the same two per-source functions on the argument blocks that carry top_p, and top_p itself
__device__ __forceinline__ const float* sample_row_uniforms(const SampleBufferP& p, size_t offset) { return p.u + offset; }
__device__ __forceinline__ const float* sample_row_uniforms(const SampleStreamP&, size_t) { return nullptr; }
__device__ __forceinline__ unsigned sample_row_key(const SampleBufferP&, const int*, int) { return 0u; }
__device__ __forceinline__ unsigned sample_row_key(const SampleStreamP& p, const int* step_dev, int row) { return sample_row_key(p.s, step_dev, row); }
__device__ __forceinline__ float sample_top_p(const float*) { return 1.f; }
__device__ __forceinline__ float sample_top_p(const SampleStream&) { return 1.f; }
__device__ __forceinline__ float sample_top_p(const SampleBufferP& p) { return p.top_p; }
__device__ __forceinline__ float sample_top_p(const SampleStreamP& p) { return p.top_p; }
// The log-probabilities of the sampled id (LP, a fourth compile-time choice; the two quantities are stated in include/omlm.h): LP = true
// wraps the source's argument block and appends the two output pointers, so the LP = false instantiations keep the argument types and the
// kernarg layout they had.  The per-source functions above see through the wrapper.
template <typename S> struct SampleLP { S s; float* lp_model; float* lp_sampled; };
// The per-row parameters (ROWS, a fifth compile-time choice; omlm_sample_rows in include/omlm.h): [B] device arrays, each or null, that
// stand in for k, temperature, top_p, the stream's seed and the stream's sample index of a row.  ROWS = true extends the nucleus- and
// log-prob-capable block (a base class: every member, and every per-source function above, is reached as before) by the five pointers,
// so the ROWS = false instantiations keep their argument types and their kernarg layout.  Only that one form is built per kernel width
// and source: top_p_r == 1 skips the nucleus by a wave-uniform branch, null lp pointers skip the stores.
struct SampleRowParams { const int* k; const float* temperature; const float* top_p; const unsigned long long* seed; const int* sample; };
template <typename S> struct SampleRows : S { SampleRowParams r; };
template <bool RNG, bool NUC, bool LP, bool ROWS = false> struct sample_arg { typedef typename sample_src<RNG, NUC>::type type; };
template <bool RNG, bool NUC> struct sample_arg<RNG, NUC, true, false> { typedef SampleLP<typename sample_src<RNG, NUC>::type> type; };
template <bool RNG> struct sample_arg<RNG, true, true, true> { typedef SampleRows<SampleLP<typename sample_src<RNG, true>::type>> type; };
template <typename S> __device__ __forceinline__ const float* sample_row_uniforms(const SampleLP<S>& p, size_t offset) { return sample_row_uniforms(p.s, offset); }
template <typename S> __device__ __forceinline__ unsigned sample_row_key(const SampleLP<S>& p, const int* step_dev, int row) { return sample_row_key(p.s, step_dev, row); }
template <typename S> __device__ __forceinline__ float sample_top_p(const SampleLP<S>& p) { return sample_top_p(p.s); }
// ROWS: the row's values replace the call's, once, before anything reads them -- in the kernel's own copy of its arguments, so the stream
// key, the nucleus and the slot loops below are the code they are for a call-wide value.  The loads are wave-uniform (indexed by the row
// alone, also with step_dev): scalar loads.  k is clamped into [1, V]; the other values are the caller's (include/omlm.h: a temperature
// that is not > 0 or a top_p outside (0, 1] gives an unspecified id in [0, V), every index below is bounded whatever they are).  The
// stream's global sample index is row0 + row: row0 becomes sample_r - row.
__device__ __forceinline__ void sample_row_stream(SampleBufferP&, const SampleRowParams&, int) {}
__device__ __forceinline__ void sample_row_stream(SampleStreamP& p, const SampleRowParams& r, int row) {
    if (r.seed) { const unsigned long long s = r.seed[row]; p.s.seed_lo = (unsigned)s; p.s.seed_hi = (unsigned)(s >> 32); }
    if (r.sample) p.s.row0 = r.sample[row] - row;
}
template <typename S> __device__ __forceinline__ void sample_row_params(SampleRows<SampleLP<S>>& p, int row, int V, int& k, float& temperature) {
    if (p.r.k) { const int kr = p.r.k[row]; k = kr < 1 ? 1 : (kr > V ? V : kr); }
    if (p.r.temperature) temperature = p.r.temperature[row];
    if (p.r.top_p) p.s.top_p = p.r.top_p[row];
    sample_row_stream(p.s, p.r, row);
}
// The two values from the sums: l_s the sampled id's logit, m the largest kept logit, M = max(m, the forbidden last logit), sum_model the
// sum of exp(l_c - M) over all V entries, sum_sampled the sum of exp((l_c - m) / T) over the set the id was drawn from.  m = -inf (the
// "id 0" rule): both -inf.  A one-entry set gives sum_sampled = 1 and l_s = m: exactly 0.
__device__ __forceinline__ void sample_lp_store(float* lp_model, float* lp_sampled, int row, float ls, float m, float M, float sum_model,
                                                float sum_sampled, float temperature) {
    const bool live = m > -INFINITY;
    if (lp_model) lp_model[row] = live ? (ls - M) - logf(sum_model) : -INFINITY;
    if (lp_sampled) lp_sampled[row] = live ? (ls - m) / temperature - logf(sum_sampled) : -INFINITY;
}

// f_ord's inverse: the float whose key this is (a logit is the exact inverse image of its key)
__device__ __forceinline__ float f_ord_inv(unsigned key) { return u2f((key & 0x80000000u) ? key ^ 0x80000000u : ~key); }
// The fixed-point mass of a kept entry: floor(exp((l - m) / T) 2^40), l the logit of `key`, m the row's largest kept logit (so w <= 1 and
// q <= 2^40: 65536 entries sum below 2^57).  The ONE place a weight is formed, for both kernels; exp(-inf) = 0.
__device__ __forceinline__ unsigned long long nucleus_q(unsigned key, float m, float temperature) {
    return (unsigned long long)(expf((f_ord_inv(key) - m) / temperature) * 0x1p40f);
}
// The cut: an entry is in the nucleus iff the mass ranked strictly before it is < top_p W, i.e. < thr = ceil(top_p W) for integer masses
// (at least 1: the first-ranked entry is always kept).  Formed once per row, in fp64 (W < 2^57: relative error 2^-53).
__device__ __forceinline__ unsigned long long nucleus_thr(float top_p, unsigned long long W) {
    const unsigned long long thr = (unsigned long long)ceil((double)top_p * (double)W);
    return thr < 1ull ? 1ull : (thr > W ? W : thr);
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {      // every lane gets the sum of the 64 lanes
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}
__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long v) {      // a wave-uniform value, moved to scalar registers
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;              // the builtin returns int: unsigned BEFORE widening, or the low half sign-extends
}

template <int SAMPLE_NV, bool RNG, bool NUC, bool LP = false, bool ROWS = false>
__global__ __launch_bounds__(64) void sample_kernel(const float* __restrict__ logits, typename sample_arg<RNG, NUC, LP, ROWS>::type uniform,
                                                    long long* __restrict__ out, int V, int ld, int k, float temperature,
                                                    int forbid_last, const int* __restrict__ step_dev, long long* __restrict__ hist,
                                                    const float* __restrict__ emb_table, long long emb_row_offset, long long emb_rows,
                                                    float* __restrict__ x, int D) {
    if (step_dev) {          // graph-replayable form: this step's uniforms / history slot are selected by a DEVICE counter
        const long long sidx = step_dev[0];
        if constexpr (!LP && !RNG && !NUC) uniform += sidx * (long long)gridDim.x * V;
        if constexpr (!LP && !RNG && NUC) uniform.u += sidx * (long long)gridDim.x * V;
        if constexpr (LP && !RNG && !NUC) uniform.s += sidx * (long long)gridDim.x * V;
        if constexpr (LP && !RNG && NUC) uniform.s.u += sidx * (long long)gridDim.x * V;
        if constexpr (LP) {                                 // [steps, B] like hist
            if (uniform.lp_model) uniform.lp_model += sidx * gridDim.x;
            if (uniform.lp_sampled) uniform.lp_sampled += sidx * gridDim.x;
        }
        if (hist) hist += sidx * gridDim.x;
    }
    const int row = blockIdx.x, lane = threadIdx.x;
    if constexpr (ROWS) sample_row_params(uniform, row, V, k, temperature);
    const float* lr = logits + (size_t)row * ld;
    const float* ur = sample_row_uniforms(uniform, (size_t)row * V);
    const unsigned ukey = sample_row_key(uniform, step_dev, row);      // RNG: the stream's key of (step, global sample index), wave-uniform
    unsigned keys[SAMPLE_NV];
    float lv[SAMPLE_NV], uv[SAMPLE_NV];
    constexpr int nv = SAMPLE_NV;                      // every slot is live or clamped: no per-slot branches
    // every load of the row -- logits AND uniforms -- is requested before anything waits.  (Round 4 kernel trace: 43.9 us per call at
    // B = 1, a quarter of a decode step: the uniforms were loaded inside `if (keep)`, one dependent memory round trip per register
    // slot, 17 in a row behind the running arg-max.)
    // (hipcc sank each uniform's first log next to its predicated load, with a vmcnt(0) in between -- seen in the ISA: the loads are
    // therefore unconditional (clamped index, no branch) and all consumed by the empty asm below before any arithmetic.)
#pragma unroll
    for (int j = 0; j < SAMPLE_NV; ++j) {
        const int c = lane + 64 * j, cc = c < V ? c : V - 1;
        lv[j] = lr[cc];
        if constexpr (!RNG) uv[j] = ur[cc];
    }
#pragma unroll
    for (int j = 0; j < SAMPLE_NV; ++j) {
        if constexpr (RNG) asm volatile("" : "+v"(lv[j]));
        else asm volatile("" : "+v"(lv[j]), "+v"(uv[j]));
    }
#pragma unroll
    for (int j = 0; j < SAMPLE_NV; ++j) {
        const int c = lane + 64 * j;
        float v = c < V ? lv[j] : -INFINITY;
        if (forbid_last && c == V - 1) v = -INFINITY;
        lv[j] = v;
        keys[j] = c < V ? f_ord(v) : 0u;               // 0 sorts below every real key (f_ord(-inf) = 0x007fffff)
    }
    // largest threshold t such that count(keys >= t) >= k
    unsigned t = 0;
    bool exact = false;                                 // count(keys >= t) == k: the kept set is exactly {keys >= t}
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = t | (1u << bit);
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < SAMPLE_NV; ++j) cnt += __popcll(__ballot(keys[j] >= cand));
        if (cnt >= k) t = cand;
        if (cnt == k) { exact = true; break; }
    }
    // strictly-greater entries are all kept; of the entries equal to t keep the first (k - n_greater) by index
    int ng = 0;
    if (!exact) {
#pragma unroll
        for (int j = 0; j < SAMPLE_NV; ++j) ng += __popcll(__ballot(keys[j] > t));
    }
    int n_equal_keep = exact ? 0x7fffffff : k - ng;
    if constexpr (NUC) if (!ROWS || sample_top_p(uniform) < 1.f) {      // ROWS: a row of top_p 1 takes the NUC = false path (wave-uniform)
        // The nucleus: the largest x >= t whose mass M(x) = sum of q over the kept keys >= x reaches thr; then the entries above x are in,
        // and of the entries equal to x the first ceil((thr - mass above x) / q_x) by index (they share one q).  The kept entries tied at t
        // enter as ONE term n q_t, so no slot needs its rank here.  The descent starts below the bits t and the row maximum share (every kept
        // key lies between them): a mass is 17 / 32 selects and adds per lane plus a 64-bit wave sum, per bit.  Measured, this second
        // descent costs more than the first (+12.5 us per launch at V = 1025, profiles/sampler_top_p.md section 2): the wave sum is six
        // dependent steps of two ds_bpermute where a count is a ballot.  Next there: several bits per step, or DPP row sums.
        unsigned kmax = 0;
#pragma unroll
        for (int j = 0; j < SAMPLE_NV; ++j) kmax = keys[j] > kmax ? keys[j] : kmax;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const unsigned ok = __shfl_xor(kmax, o, 64); kmax = ok > kmax ? ok : kmax; }
        kmax = __builtin_amdgcn_readfirstlane(kmax);
        const float m = f_ord_inv(kmax);
        if (m > -INFINITY && m < INFINITY) {                // m = -inf: every kept entry is -inf, the id is 0 as without a nucleus
            int neq = n_equal_keep;                         // kept entries equal to t
            if (exact) {
                neq = 0;
#pragma unroll
                for (int j = 0; j < SAMPLE_NV; ++j) neq += __popcll(__ballot(keys[j] == t && lane + 64 * j < V));
            }
            unsigned long long q[SAMPLE_NV], part = 0;
#pragma unroll
            for (int j = 0; j < SAMPLE_NV; ++j) {           // a pad's key is 0: never above t
                q[j] = keys[j] > t ? nucleus_q(keys[j], m, temperature) : 0ull;
                part += q[j];
            }
            const unsigned long long qt = neq > 0 ? nucleus_q(t, m, temperature) : 0ull, Qt = (unsigned long long)neq * qt;
            const unsigned long long thr = nucleus_thr(sample_top_p(uniform), uniform_u64(wave_sum_u64(part)) + Qt);
            unsigned x = t;
            if (t != kmax) {
                const int hb = 31 - __clz(t ^ kmax);       // kmax has this bit, t does not
                x = t & ~((2u << hb) - 1u);
                for (int bit = hb; bit >= 0; --bit) {
                    const unsigned cand = x | (1u << bit);
                    unsigned long long ms = 0;
#pragma unroll
                    for (int j = 0; j < SAMPLE_NV; ++j) ms += keys[j] >= cand ? q[j] : 0ull;
                    ms = uniform_u64(wave_sum_u64(ms)) + (cand <= t ? Qt : 0ull);
                    if (ms >= thr) x = cand;
                }
            }
            unsigned long long g = 0;                       // the mass ranked before the entries equal to x
#pragma unroll
            for (int j = 0; j < SAMPLE_NV; ++j) g += keys[j] > x ? q[j] : 0ull;
            g = uniform_u64(wave_sum_u64(g));
            const unsigned long long qx = x == t ? qt : nucleus_q(x, m, temperature);
            int np = qx > 0 && thr > g ? (int)((thr - g + qx - 1ull) / qx) : 0x7fffffff;
            if (x == t && np > neq) np = neq;
            t = x;
            n_equal_keep = np;
        }
    }
    // LP: m = the largest kept logit (the top-k set and the nucleus both keep the row's largest masked logit), M = max(m, the forbidden
    // last logit, read again: lv[] holds -inf there); two running sums in slot order beside the scores; the winner's logit is one load of lr[besti]
    float lp_m = -INFINITY, lp_M = -INFINITY, lp_last = -INFINITY, lp_sum_model = 0.f, lp_sum_sampled = 0.f;
    if constexpr (LP) {
#pragma unroll
        for (int j = 0; j < SAMPLE_NV; ++j) lp_m = fmaxf(lp_m, lv[j]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lp_m = fmaxf(lp_m, __shfl_xor(lp_m, o, 64));
        if (forbid_last) lp_last = lr[V - 1];
        lp_M = fmaxf(lp_m, lp_last);
    }
    float best = -INFINITY;
    int besti = 0x7fffffff;
    int seen_eq = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < SAMPLE_NV; ++j) {
        const int c = lane + 64 * j;
        const bool in = c < V;
        const bool eq = in && keys[j] == t;
        const unsigned long long eqmask = __ballot(eq);
        const int rank = seen_eq + __popcll(eqmask & below);
        const bool keep = in && (keys[j] > t || (eq && rank < n_equal_keep));
        seen_eq += __popcll(eqmask);
        // branch-free: the Gumbel term of every slot is formed (2 logs per slot), dead slots lose the comparison
        if constexpr (RNG) uv[j] = sample_stream_u(ukey, (unsigned)c);
        const float gum = -logf(-logf(uv[j] + 1e-20f) + 1e-20f);
        const float v = keep ? lv[j] / temperature + gum : -INFINITY;
        if (v > best) { best = v; besti = c; }
        if constexpr (LP) {                             // the precise expf of nucleus_q; exp(-inf) = 0: pads and the forbidden entry add nothing
            lp_sum_model += expf(lv[j] - lp_M);
            lp_sum_sampled += keep ? expf((lv[j] - lp_m) / temperature) : 0.f;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(besti, o, 64);
        if (ov > best || (ov == best && oi < besti)) { best = ov; besti = oi; }
    }
    if (besti == 0x7fffffff) besti = 0;                 // every kept entry -inf (e.g. V = 1 with forbid_last): no slot won a comparison
    if (lane == 0) { out[row] = besti; if (hist) hist[row] = besti; }
    if constexpr (LP) {                                 // a fixed tree: one row gives the same bits in every launch
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lp_sum_model += __shfl_xor(lp_sum_model, o, 64);
            lp_sum_sampled += __shfl_xor(lp_sum_sampled, o, 64);
        }
        lp_sum_model += expf(lp_last - lp_M);           // the forbidden last entry belongs to the model's distribution (0 when it is not forbidden)
        if (lane == 0) sample_lp_store(uniform.lp_model, uniform.lp_sampled, row, lr[besti], lp_m, lp_M, lp_sum_model, lp_sum_sampled, temperature);
    }
    if (emb_table) {
        long long r = (long long)besti + emb_row_offset;
        r = r < 0 ? 0 : (r >= emb_rows ? emb_rows - 1 : r);
        const float4* src = (const float4*)(emb_table + r * D);
        float4* dst = (float4*)(x + (size_t)row * D);
        for (int i = lane; i < D / 4; i += 64) dst[i] = src[i];
    }
}

// The same function of (logits, uniforms, k, T, forbid_last) for 2048 < V <= 65536: one WORKGROUP per row (B <= 64 rows: a row is not
// spread over workgroups), up to 16 waves.  Wave w owns the CONTIGUOUS indices [w * 64 * NV, (w + 1) * 64 * NV), element
// c = base + lane + 64 j, so slot order then lane order is index order inside a wave and the wave kernel's seen_eq + popc(mask & below)
// ranks the tied entries of a segment; one scan over the waves' tie counts gives the segment's offset.
// Residency: a row of 65536 floats (256 KB) does not fit the LDS.  Only the KEYS stay on chip, in registers (NV <= 64 per lane, under
// the 128-VGPR ceiling of a 1024-thread workgroup); the logit of a kept entry is the exact inverse image of its key, so the logits are
// read once, and the uniforms are read once, after the kept set is known, for kept entries only (a dropped slot loads element 0 of
// the row: the load stays unconditional, one broadcast line).  Loads are dword loads: ld and V are arbitrary, rows are not 16-byte
// aligned.
// k-th largest key: radix descent by 8-bit digits, 4 rounds of a 256-bin LDS histogram (a per-bit descent as in the wave kernel would
// meet at 32 barriers).  The bins are integer counts -- the LDS adds commute, the counts and so the id do not depend on arrival order;
// no float is ever accumulated atomically.  Trained logits share their sign and high exponent bits, so the first round lands in a few
// bins: every bin has SW_COPIES copies (lane & 7) to spread the same-address adds, and wave 0 sums them when it scans the bins.
// The pads (key 0, at or below every live key) are counted too: k <= V, so the k-th largest key and kk are those of the live keys alone.
// The descent ends with t = the k-th largest key and kk = k - count(keys > t), the number of tied entries to keep.
constexpr int SW_COPIES = 8;
constexpr int SW_UC = 16;                                 // uniforms in flight per lane in the scoring pass
template <int NV, bool RNG, bool NUC, bool LP = false, bool ROWS = false>
__global__ __launch_bounds__(1024) void sample_wide_kernel(const float* __restrict__ logits, typename sample_arg<RNG, NUC, LP, ROWS>::type uniform,
                                                           long long* __restrict__ out, int V, int ld, int k, float temperature,
                                                           int forbid_last, const int* __restrict__ step_dev, long long* __restrict__ hist,
                                                           const float* __restrict__ emb_table, long long emb_row_offset,
                                                           long long emb_rows, float* __restrict__ x, int D) {
    __shared__ __attribute__((aligned(16))) int s_hist[256 * SW_COPIES];
    __shared__ int s_sel[2], s_weq[16], s_bi[16];
    __shared__ float s_bv[16];
    if (step_dev) {
        const long long sidx = step_dev[0];
        if constexpr (!LP && !RNG && !NUC) uniform += sidx * (long long)gridDim.x * V;
        if constexpr (!LP && !RNG && NUC) uniform.u += sidx * (long long)gridDim.x * V;
        if constexpr (LP && !RNG && !NUC) uniform.s += sidx * (long long)gridDim.x * V;
        if constexpr (LP && !RNG && NUC) uniform.s.u += sidx * (long long)gridDim.x * V;
        if constexpr (LP) {                                 // [steps, B] like hist
            if (uniform.lp_model) uniform.lp_model += sidx * gridDim.x;
            if (uniform.lp_sampled) uniform.lp_sampled += sidx * gridDim.x;
        }
        if (hist) hist += sidx * gridDim.x;
    }
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int base = wave * 64 * NV;
    // every pass forms its indices from a value of its own (the empty asm): hipcc otherwise keeps the 64 indices, and the 64 `c < V` masks,
    // of the first pass alive to the last one and spills them
    int c0 = base + lane;
    if constexpr (ROWS) sample_row_params(uniform, row, V, k, temperature);
    const float* lr = logits + (size_t)row * ld;
    const float* ur = sample_row_uniforms(uniform, (size_t)row * V);
    const unsigned ukey = sample_row_key(uniform, step_dev, row);      // RNG: the stream's key of (step, global sample index), one per workgroup
    unsigned keys[NV];
    {   // every logit load is requested before the first wait, unconditional on a clamped index (the wave kernel's two lessons)
        float lv[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = c0 + 64 * j;
            lv[j] = *(const float*)((const char*)lr + 4u * (unsigned)(c < V ? c : V - 1));       // uniform base + 32-bit lane offset
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) asm volatile("" : "+v"(lv[j]));
        asm volatile("" : "+v"(c0));
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = c0 + 64 * j;
            const float v = (forbid_last && c == V - 1) ? -INFINITY : lv[j];
            keys[j] = c < V ? f_ord(v) : 0u;
        }
    }
    for (int i = tid; i < 256 * SW_COPIES; i += blockDim.x) s_hist[i] = 0;
    __syncthreads();
    unsigned t = 0;
    int kk = k;                                            // entries still to keep among the keys that share the prefix t
    for (int r = 0; r < 4; ++r) {
        const int shift = 24 - 8 * r;
        const unsigned himask = r == 0 ? 0u : 0xffffffffu << (shift + 8);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            if ((keys[j] & himask) == t) atomicAdd(&s_hist[((keys[j] >> shift) & 255u) * SW_COPIES + (lane & (SW_COPIES - 1))], 1);
        }
        __syncthreads();
        if (wave == 0) {                                   // lane l owns bins 4 l .. 4 l + 3; higher bins hold larger keys
            int bin[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                int4* p = (int4*)&s_hist[(4 * lane + b) * SW_COPIES];
                const int4 a0 = p[0], a1 = p[1];
                bin[b] = a0.x + a0.y + a0.z + a0.w + a1.x + a1.y + a1.z + a1.w;
                p[0] = make_int4(0, 0, 0, 0);              // zero for the next round (the barrier below is in between)
                p[1] = make_int4(0, 0, 0, 0);
            }
            const int mine = bin[0] + bin[1] + bin[2] + bin[3];
            int suf = mine;                                // inclusive suffix sum over the lanes: entries in bins >= 4 l
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_down(suf, o, 64);
                if (lane + o < 64) suf += v;
            }
            int above = suf - mine;
            if (above < kk && kk <= suf) {                 // exactly one lane: the kk-th largest entry lies in one of its bins
                int d = 3;
                while (d > 0 && above + bin[d] < kk) { above += bin[d]; --d; }
                s_sel[0] = 4 * lane + d;
                s_sel[1] = kk - above;
            }
        }
        __syncthreads();
        t |= (unsigned)s_sel[0] << shift;
        kk = s_sel[1];
    }
    if constexpr (NUC) if (!ROWS || sample_top_p(uniform) < 1.f) {      // ROWS: a row of top_p 1 takes the NUC = false path (workgroup-uniform)
        // The nucleus on the same machinery: radix rounds over the 8-bit digits with a 64-bit MASS per bin (integer LDS adds: any arrival order
        // gives the same sums), scanned from the top bin down to the bin where the running mass reaches thr.  Only the keys above t add
        // their mass; the kk kept entries tied at t are one term kk q_t that wave 0 adds to t's bin, so no rank is needed.  The weights are
        // formed again from the keys in every round (nothing is stored: the registers hold the keys), and a round whose digit t and the row
        // maximum share -- every kept key lies between them -- is skipped.  The first round that runs sees the whole kept set: its total is W.
        __shared__ __attribute__((aligned(16))) unsigned long long s_mass[256 * SW_COPIES];
        __shared__ unsigned long long s_rem;
        __shared__ unsigned s_kmax[16];
        __shared__ int s_dig;
        unsigned kmax = 0;
#pragma unroll
        for (int j = 0; j < NV; ++j) kmax = keys[j] > kmax ? keys[j] : kmax;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const unsigned ok = __shfl_xor(kmax, o, 64); kmax = ok > kmax ? ok : kmax; }
        if (lane == 0) s_kmax[wave] = kmax;
        if (tid == 0) { s_dig = 0; s_rem = 1ull; }
        for (int i = tid; i < 256 * SW_COPIES; i += blockDim.x) s_mass[i] = 0ull;
        __syncthreads();
        kmax = s_kmax[0];
        for (int w = 1; w < nw; ++w) kmax = s_kmax[w] > kmax ? s_kmax[w] : kmax;
        const float m = f_ord_inv(kmax);
        if (m > -INFINITY && m < INFINITY) {                // m = -inf: every kept entry is -inf, the id is 0 as without a nucleus
            const float top_p = sample_top_p(uniform);
            unsigned x = 0;
            unsigned long long rem = 0;
            bool first = true;
            for (int r = 0; r < 4; ++r) {
                const int shift = 24 - 8 * r;
                const unsigned himask = r == 0 ? 0u : 0xffffffffu << (shift + 8);
                if (((t ^ kmax) >> shift) == 0u) { x |= t & (0xffu << shift); continue; }
                unsigned tok = 0;                              // one slot's weight at a time: each slot waits for the one before (the empty
#pragma unroll                                                 // asm), or hipcc forms many exponentials at once beside the keys and spills
                for (int j = 0; j < NV; ++j) {
                    unsigned kj = keys[j];
                    asm volatile("" : "+v"(kj), "+v"(tok));
                    if (kj > t && (kj & himask) == x) {
                        const unsigned long long q = nucleus_q(kj, m, temperature);
                        atomicAdd(&s_mass[((kj >> shift) & 255u) * SW_COPIES + (lane & (SW_COPIES - 1))], q);
                        tok = (unsigned)q;
                    }
                }
                __syncthreads();
                if (wave == 0) {                               // lane l owns bins 4 l .. 4 l + 3; higher bins hold larger keys
                    // the scan forms what it needs from values of its own (the empty asm): hipcc otherwise hoists the shuffle addresses, the
                    // tied term and top_p out of the round loop, a dozen registers held beside the 64 keys -- one too many at NV = 64
                    int ln = lane;
                    unsigned tt = t;
                    float tp = top_p;
                    asm volatile("" : "+v"(ln), "+v"(tt), "+v"(tp));
                    unsigned long long bin[4];
                    const bool t_here = (tt & himask) == x;
                    const int t_dig = (int)((tt >> shift) & 255u);
                    int l4 = 4 * ln;                           // one bin's 64 bytes in flight at a time
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        if (b > 0) asm volatile("" : "+v"(l4) : "v"((unsigned)bin[b - 1]));
                        ulonglong2* p = (ulonglong2*)&s_mass[(l4 + b) * SW_COPIES];
                        const ulonglong2 a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3];
                        bin[b] = a0.x + a0.y + a1.x + a1.y + a2.x + a2.y + a3.x + a3.y;
                        if (t_here && t_dig == l4 + b) bin[b] += (unsigned long long)kk * nucleus_q(tt, m, temperature);
                        p[0] = p[1] = p[2] = p[3] = make_ulonglong2(0ull, 0ull);      // zero for the next round (the barrier below is in between)
                    }
                    const unsigned long long mine = bin[0] + bin[1] + bin[2] + bin[3];
                    unsigned long long suf = mine;             // inclusive suffix sum over the lanes: mass in bins >= 4 l
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const unsigned lo = __builtin_amdgcn_ds_bpermute((ln + o) << 2, (int)(unsigned)suf);
                        const unsigned hi = __builtin_amdgcn_ds_bpermute((ln + o) << 2, (int)(unsigned)(suf >> 32));
                        if (ln + o < 64) suf += ((unsigned long long)hi << 32) | lo;
                    }
                    if (first) rem = nucleus_thr(tp, uniform_u64(suf));      // lane 0 holds the total
                    unsigned long long above = suf - mine;
                    if (above < rem && rem <= suf) {           // exactly one lane: the running mass reaches rem in one of its bins
                        int d = 3;
                        while (d > 0 && above + bin[d] < rem) { above += bin[d]; --d; }
                        s_dig = l4 + d;
                        s_rem = rem - above;
                    }
                }
                __syncthreads();
                x |= (unsigned)s_dig << shift;
                rem = s_rem;
                first = false;
            }
            // x: the lowest key of the nucleus; rem: what is left of thr after the mass above x.  The entries equal to x share one q.
            const unsigned long long qx = nucleus_q(x, m, temperature);
            if (first) rem = nucleus_thr(top_p, (unsigned long long)kk * qx);      // t is the row maximum: no round ran, x = t, S = the kk tied entries
            int np = qx > 0 && rem > 0 ? (int)((rem + qx - 1ull) / qx) : 0x7fffffff;
            if (x == t && np > kk) np = kk;
            t = x;
            kk = np;
        }
    }
    // of the entries equal to t keep the first kk by index: offset of this wave's segment among the tied entries
    int myeq = 0;                                          // per lane, then over the wave (64 ballots held for later would spill)
    int Vq = V;
    asm volatile("" : "+v"(Vq), "+v"(c0));
#pragma unroll
    for (int j = 0; j < NV; ++j) myeq += (keys[j] == t && c0 + 64 * j < Vq) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) myeq += __shfl_xor(myeq, o, 64);
    if (lane == 0) s_weq[wave] = myeq;
    __syncthreads();
    int seen_eq = 0;
    for (int w = 0; w < wave; ++w) seen_eq += s_weq[w];
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long keepbits = 0;
    asm volatile("" : "+v"(Vq), "+v"(c0));
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const bool eq = keys[j] == t && c0 + 64 * j < Vq;
        const unsigned long long eqmask = __ballot(eq);
        const int rank = seen_eq + __popcll(eqmask & below);
        if (keys[j] > t || (eq && rank < kk)) keepbits |= 1ull << j;            // a pad's key is 0: never above t
        seen_eq += __popcll(eqmask);
    }
    float best = -INFINITY;
    int besti = 0x7fffffff;
#pragma unroll
    for (int j0 = 0; j0 < NV; j0 += SW_UC) {
        constexpr int UC = NV < SW_UC ? NV : SW_UC;
        float uv[UC];
        unsigned long long kb = keepbits;
        asm volatile("" : "+v"(c0), "+v"(kb));
        if constexpr (!RNG) {
#pragma unroll
            for (int jj = 0; jj < UC; ++jj) uv[jj] = *(const float*)((const char*)ur + 4u * (unsigned)(((kb >> (j0 + jj)) & 1ull) ? c0 + 64 * (j0 + jj) : 0));
#pragma unroll
            for (int jj = 0; jj < UC; ++jj) asm volatile("" : "+v"(uv[jj]));
        }
#pragma unroll
        for (int jj = 0; jj < UC; ++jj) {
            const int j = j0 + jj;
            const bool keep = (kb >> j) & 1ull;
            const float l = u2f((keys[j] & 0x80000000u) ? keys[j] ^ 0x80000000u : ~keys[j]);      // f_ord's inverse: the logit's bits
            if constexpr (RNG) uv[jj] = sample_stream_u(ukey, (unsigned)(c0 + 64 * j));      // every slot, kept or not: one hash, no branch
            const float gum = -logf(-logf(uv[jj] + 1e-20f) + 1e-20f);
            const float v = keep ? l / temperature + gum : -INFINITY;
            if (v > best) { best = v; besti = c0 + 64 * j; }
            // NV = 64: one slot's hash and logs at a time (16 hashes in flight beside the 64 keys spilt 18 registers; the four waves of a
            // SIMD fill each other's latencies)
            if constexpr (RNG && NV > SW_UC) asm volatile("" : "+v"(best));
            // LP, NV = 64: keepbits outlives this pass, and the winner's index is settled slot by slot (hipcc otherwise keeps the 16
            // candidate indices of a round for one chain of selects at its end: spilt beside the 64 keys)
            if constexpr (LP && NV > SW_UC) asm volatile("" : "+v"(best), "+v"(besti));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(besti, o, 64);
        if (ov > best || (ov == best && oi < besti)) { best = ov; besti = oi; }
    }
    if (lane == 0) { s_bv[wave] = best; s_bi[wave] = besti; }
    __syncthreads();
    best = s_bv[0];
    besti = s_bi[0];
    for (int w = 1; w < nw; ++w) {
        const float ov = s_bv[w];
        const int oi = s_bi[w];
        if (ov > best || (ov == best && oi < besti)) { best = ov; besti = oi; }
    }
    if (besti == 0x7fffffff) besti = 0;                    // every kept entry -inf: no slot won a comparison
    if (tid == 0) { out[row] = besti; if (hist) hist[row] = besti; }
    if constexpr (LP) {
        // Only the keys are resident: a logit is the inverse image of its key (a pad's key is 0, no logit has it), keepbits says which
        // entries the id was drawn from.  One slot at a time (the empty asm), as in the mass round of the nucleus; per lane in slot order,
        // the wave's shuffle tree, then the waves' partials through LDS in wave order: no float atomics, one row gives the same bits.
        __shared__ unsigned s_lpk[16];
        __shared__ float s_lpm[16], s_lps[16];
        unsigned kmax = 0;
#pragma unroll
        for (int j = 0; j < NV; ++j) kmax = keys[j] > kmax ? keys[j] : kmax;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const unsigned ok = __shfl_xor(kmax, o, 64); kmax = ok > kmax ? ok : kmax; }
        if (lane == 0) s_lpk[wave] = kmax;
        __syncthreads();
        kmax = s_lpk[0];
        for (int w = 1; w < nw; ++w) kmax = s_lpk[w] > kmax ? s_lpk[w] : kmax;
        // workgroup-uniform values go to scalar registers: at NV = 64 the 64 keys leave the vector file no room for them
        const float m = f_ord_inv((unsigned)__builtin_amdgcn_readfirstlane((int)kmax));      // the largest kept logit: top-k and nucleus keep the row's largest masked logit
        float lastl = -INFINITY;                           // overwritten with -inf before the keys were formed: read again
        if (forbid_last) lastl = u2f((unsigned)__builtin_amdgcn_readfirstlane((int)f2u(lr[V - 1])));
        const float M = fmaxf(m, lastl);
        float sm = 0.f, ss = 0.f;
        if (m > -INFINITY) {
            unsigned long long kb = keepbits;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                unsigned kj = keys[j];
                asm volatile("" : "+v"(kj), "+v"(sm), "+v"(ss));
                const float l = f_ord_inv(kj);
                if (kj != 0u) sm += expf(l - M);
                asm volatile("" : "+v"(sm), "+v"(kb));         // one exponential at a time
                if ((kb >> j) & 1ull) ss += expf((l - m) / temperature);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sm += __shfl_xor(sm, o, 64);
            ss += __shfl_xor(ss, o, 64);
        }
        if (lane == 0) { s_lpm[wave] = sm; s_lps[wave] = ss; }
        __syncthreads();
        if (tid == 0) {
            sm = s_lpm[0];
            ss = s_lps[0];
            for (int w = 1; w < nw; ++w) { sm += s_lpm[w]; ss += s_lps[w]; }
            sm += expf(lastl - M);                         // the forbidden last entry belongs to the model's distribution
            sample_lp_store(uniform.lp_model, uniform.lp_sampled, row, lr[besti], m, M, sm, ss, temperature);
        }
    }
    if (emb_table) {
        long long r = (long long)besti + emb_row_offset;
        r = r < 0 ? 0 : (r >= emb_rows ? emb_rows - 1 : r);
        const float4* src = (const float4*)(emb_table + r * D);
        float4* dst = (float4*)(x + (size_t)row * D);
        for (int i = tid; i < D / 4; i += blockDim.x) dst[i] = src[i];
    }
}

struct omlm_sample_args {                                 // include/omlm.h
    const float* logits; int B, V, ld;
    const float* uniform; unsigned seed_lo, seed_hi; int step, row0; const int* step_dev;
    long long* out; long long* hist;
    int k; float temperature, top_p; int forbid_last;
    const float* emb_table; long long emb_row_offset, emb_rows; float* x; int D;
};

// The kernel for a row of V logits: V <= 1088 / 2048 the wave kernel with 17 / 32 slots; wider, the workgroup kernel with the fewest slots
// per lane that hold the row, and only the waves that own a live index.  `src` is the kernel's second argument (sample_arg).  The wide
// kernels are named first: instantiation order is function order in the module, and with the wave kernels first two independent
// instructions of the wide kernels' bin scan swap (profiles/sampler_stream.md section 1).
template <bool RNG, bool NUC, bool LP, bool ROWS = false>
static void sample_launch(const omlm_sample_args& a, typename sample_arg<RNG, NUC, LP, ROWS>::type src, void* stream) {
    const bool emb = a.emb_table != nullptr;
#define SAMPLE_GO(BLOCK_, ...) hipLaunchKernelGGL((__VA_ARGS__), dim3(a.B), BLOCK_, 0, as_stream(stream), a.logits, src, a.out, a.V, a.ld, a.k,   \
                                                  a.temperature, a.forbid_last, a.step_dev, a.hist, a.emb_table, emb ? a.emb_row_offset : 0ll, \
                                                  emb ? a.emb_rows : 0ll, emb ? a.x : nullptr, emb ? a.D : 0)
    if (a.V > 2048) {
        const int nv = a.V <= 4096 ? 4 : a.V <= 16384 ? 16 : 64;
        const dim3 block(64 * ((a.V + 64 * nv - 1) / (64 * nv)));
        if (nv == 4) SAMPLE_GO(block, sample_wide_kernel<4, RNG, NUC, LP, ROWS>);
        else if (nv == 16) SAMPLE_GO(block, sample_wide_kernel<16, RNG, NUC, LP, ROWS>);
        else SAMPLE_GO(block, sample_wide_kernel<64, RNG, NUC, LP, ROWS>);
    }
    else if (a.V <= 64 * 17) SAMPLE_GO(dim3(64), sample_kernel<17, RNG, NUC, LP, ROWS>);
    else SAMPLE_GO(dim3(64), sample_kernel<32, RNG, NUC, LP, ROWS>);
#undef SAMPLE_GO
}

// Every entry point ends here: the checks, then the one launch the block asks for -- uniforms from `uniform` or the counter stream, the
// nucleus when top_p < 1, the log-probabilities when either pointer is given.  `need`: what the calling entry requires beyond the block's
// own rules (its signature has no other form).
enum { NEED_UNIFORM = 1, NEED_STEP_DEV = 2, NEED_EMBED = 4 };
static int sample_checked(const char* name, const omlm_sample_args& a, int need, float* lp_model, float* lp_sampled, void* stream) {
    if (a.B <= 0) return OMLM_OK;
    OMLM_CHECK_ARG(a.logits && a.out && (a.uniform || !(need & NEED_UNIFORM)) && (a.step_dev || !(need & NEED_STEP_DEV)) && a.V > 0 &&
                   a.V <= 65536 && a.k >= 1 && a.k <= a.V && a.temperature > 0.f,
                   "sampler arguments (0 < V <= 65536, 1 <= k <= V, temperature > 0)");
    OMLM_CHECK_ARG(a.top_p > 0.f && a.top_p <= 1.f, "top_p (0 < top_p <= 1; 1 = no nucleus)");
    if (a.emb_table || (need & NEED_EMBED))
        OMLM_CHECK_ARG(a.emb_table && a.x && a.D > 0 && a.D % 4 == 0 && a.emb_rows > 0, "embedding arguments");
    const SampleStream st{a.seed_lo, a.seed_hi, a.step_dev ? 0 : a.step, a.row0};
    const SampleBufferP up{a.uniform, a.top_p};
    const SampleStreamP sp{st, a.top_p};
    const bool buf = a.uniform != nullptr, nuc = a.top_p < 1.f;
    // The order in which the eight forms are first named here is the order of the forty kernels in the module, and the compiled kernels
    // depend on it (the note above sample_launch): keep it -- profiles/sampler_split.md compares every kernel with its predecessor's.
#define SAMPLE_GO(RNG_, NUC_, LP_, ...) sample_launch<RNG_, NUC_, LP_>(a, __VA_ARGS__, stream)
    if (!lp_model && !lp_sampled) {
        if (!nuc && buf) SAMPLE_GO(false, false, false, a.uniform);
        else if (!nuc) SAMPLE_GO(true, false, false, st);
        else if (buf) SAMPLE_GO(false, true, false, up);
        else SAMPLE_GO(true, true, false, sp);
    }
    else if (nuc && buf) SAMPLE_GO(false, true, true, {up, lp_model, lp_sampled});
    else if (nuc) SAMPLE_GO(true, true, true, {sp, lp_model, lp_sampled});
    else if (buf) SAMPLE_GO(false, false, true, {a.uniform, lp_model, lp_sampled});
    else SAMPLE_GO(true, false, true, {st, lp_model, lp_sampled});
#undef SAMPLE_GO
    return omlm_post_launch(name);
}

// One entry point over every form (include/omlm.h): the argument block says where the uniforms come from (uniform / the counter stream),
// whether the step is a device counter (step_dev) and whether the embedding row is gathered (emb_table).
extern "C" int omlm_sample(const omlm_sample_args* a, void* stream) {
    OMLM_CHECK_ARG(a != nullptr, "args");
    return sample_checked("omlm_sample", *a, 0, nullptr, nullptr, stream);
}
// omlm_sample plus the log-probabilities of the id it returns (include/omlm.h); both pointers NULL: exactly omlm_sample.
extern "C" int omlm_sample_lp(const omlm_sample_args* a, float* lp_model, float* lp_sampled, void* stream) {
    OMLM_CHECK_ARG(a != nullptr, "args");
    return sample_checked("omlm_sample_lp", *a, 0, lp_model, lp_sampled, stream);
}

// The six entry points that predate the block: each fills one (top_p = 1) and requires what its signature has no other form for.
// Buffer forms: uniforms [B, V]; `_at`: uniforms [steps, B, V] and the id history [steps, B] indexed by *step_dev (a captured decode step);
// `embed`: plus the embedding gather of the sampled id, x[b, :] = emb_table[id_b + emb_row_offset] (rows clamped to [0, emb_rows)).
extern "C" int omlm_sample_topk_gumbel(const float* logits, const float* uniform, long long* out, int B, int V, int ld,
                                       int k, float temperature, int forbid_last, void* stream) {
    const omlm_sample_args a{logits, B, V, ld, uniform, 0u, 0u, 0, 0, nullptr, out, nullptr, k, temperature, 1.f, forbid_last};
    return sample_checked("omlm_sample_topk_gumbel", a, NEED_UNIFORM, nullptr, nullptr, stream);
}
extern "C" int omlm_sample_topk_gumbel_at(const float* logits, const float* uniform_base, const int* step_dev, long long* out,
                                          long long* hist, int B, int V, int ld, int k, float temperature, int forbid_last,
                                          void* stream) {
    const omlm_sample_args a{logits, B, V, ld, uniform_base, 0u, 0u, 0, 0, step_dev, out, hist, k, temperature, 1.f, forbid_last};
    return sample_checked("omlm_sample_topk_gumbel_at", a, NEED_UNIFORM | NEED_STEP_DEV, nullptr, nullptr, stream);
}
extern "C" int omlm_sample_embed_at(const float* logits, const float* uniform_base, const int* step_dev, long long* out,
                                    long long* hist, int B, int V, int ld, int k, float temperature, int forbid_last,
                                    const float* emb_table, long long emb_row_offset, long long emb_rows, float* x, int D,
                                    void* stream) {
    const omlm_sample_args a{logits, B, V, ld, uniform_base, 0u, 0u, 0, 0, step_dev, out, hist, k, temperature, 1.f, forbid_last,
                             emb_table, emb_row_offset, emb_rows, x, D};
    return sample_checked("omlm_sample_embed_at", a, NEED_UNIFORM | NEED_STEP_DEV | NEED_EMBED, nullptr, nullptr, stream);
}
// The same three on the counter stream (include/omlm.h): no uniform buffer; row b of the call draws u(t, row0 + b, c) with t = step (host)
// or *step_dev.  Seed halves and row0 are plain kernel arguments, so a captured cycle stays valid for a whole call.
extern "C" int omlm_sample_topk_gumbel_rng(const float* logits, unsigned seed_lo, unsigned seed_hi, int step, int row0, long long* out,
                                           int B, int V, int ld, int k, float temperature, int forbid_last, void* stream) {
    const omlm_sample_args a{logits, B, V, ld, nullptr, seed_lo, seed_hi, step, row0, nullptr, out, nullptr, k, temperature, 1.f, forbid_last};
    return sample_checked("omlm_sample_topk_gumbel_rng", a, 0, nullptr, nullptr, stream);
}
extern "C" int omlm_sample_topk_gumbel_at_rng(const float* logits, unsigned seed_lo, unsigned seed_hi, const int* step_dev, int row0,
                                              long long* out, long long* hist, int B, int V, int ld, int k, float temperature,
                                              int forbid_last, void* stream) {
    const omlm_sample_args a{logits, B, V, ld, nullptr, seed_lo, seed_hi, 0, row0, step_dev, out, hist, k, temperature, 1.f, forbid_last};
    return sample_checked("omlm_sample_topk_gumbel_at_rng", a, NEED_STEP_DEV, nullptr, nullptr, stream);
}
extern "C" int omlm_sample_embed_at_rng(const float* logits, unsigned seed_lo, unsigned seed_hi, const int* step_dev, int row0,
                                        long long* out, long long* hist, int B, int V, int ld, int k, float temperature, int forbid_last,
                                        const float* emb_table, long long emb_row_offset, long long emb_rows, float* x, int D,
                                        void* stream) {
    const omlm_sample_args a{logits, B, V, ld, nullptr, seed_lo, seed_hi, 0, row0, step_dev, out, hist, k, temperature, 1.f, forbid_last,
                             emb_table, emb_row_offset, emb_rows, x, D};
    return sample_checked("omlm_sample_embed_at_rng", a, NEED_STEP_DEV | NEED_EMBED, nullptr, nullptr, stream);
}

// The row-parameter form (include/omlm.h): per-row k / temperature / top_p / seed / sample index from [B] device arrays.  No array: the
// launch of omlm_sample_lp.  Otherwise one launch of the ROWS form of the kernel the block selects -- named here, after every other
// form (the note in sample_checked) -- with the scalars of the arrays that are given neither read nor checked.
struct omlm_sample_row_params {                          // include/omlm.h
    const int* k; const float* temperature; const float* top_p; const unsigned long long* seed; const int* sample;
};
extern "C" int omlm_sample_rows(const omlm_sample_args* args, const omlm_sample_row_params* rows, float* lp_model, float* lp_sampled,
                                void* stream) {
    OMLM_CHECK_ARG(args != nullptr, "args");
    if (!rows || (!rows->k && !rows->temperature && !rows->top_p && !rows->seed && !rows->sample))
        return sample_checked("omlm_sample_rows", *args, 0, lp_model, lp_sampled, stream);
    const omlm_sample_args& a = *args;
    if (a.B <= 0) return OMLM_OK;
    OMLM_CHECK_ARG(!(a.uniform && rows->seed), "omlm_sample_rows: rows->seed belongs to the counter stream; args->uniform selects the buffer");
    OMLM_CHECK_ARG(!(a.uniform && rows->sample), "omlm_sample_rows: rows->sample belongs to the counter stream; args->uniform selects the buffer");
    OMLM_CHECK_ARG(a.logits && a.out && a.V > 0 && a.V <= 65536 && (rows->k || (a.k >= 1 && a.k <= a.V)) &&
                   (rows->temperature || a.temperature > 0.f),
                   "sampler arguments (0 < V <= 65536, 1 <= k <= V, temperature > 0)");
    OMLM_CHECK_ARG(rows->top_p || (a.top_p > 0.f && a.top_p <= 1.f), "top_p (0 < top_p <= 1; 1 = no nucleus)");
    if (a.emb_table) OMLM_CHECK_ARG(a.x && a.D > 0 && a.D % 4 == 0 && a.emb_rows > 0, "embedding arguments");
    omlm_sample_args b = a;                               // the scalars a row array replaces: any valid value, the kernel overwrites it
    if (rows->k) b.k = 1;
    if (rows->temperature) b.temperature = 1.f;
    const float top_p = rows->top_p ? 1.f : a.top_p;
    const SampleRowParams rp{rows->k, rows->temperature, rows->top_p, rows->seed, rows->sample};
    if (a.uniform) sample_launch<false, true, true, true>(b, {{SampleBufferP{a.uniform, top_p}, lp_model, lp_sampled}, rp}, stream);
    else {
        const SampleStream st{a.seed_lo, a.seed_hi, a.step_dev ? 0 : a.step, a.row0};
        sample_launch<true, true, true, true>(b, {{SampleStreamP{st, top_p}, lp_model, lp_sampled}, rp}, stream);
    }
    return omlm_post_launch("omlm_sample_rows");
}

// ---------------------------------------------------------------------------------------------------------
// Classifier-free guidance around the sampler (include/omlm.h).  Two small kernels that sit in front of and behind the sampler launch
// of a guided decode cycle; the sampler kernels above are what they were.
//
// guide: out[r, c] = null[r, c] + scale * (cond[r, c] - null[r, c]) for c < V, three fp32 roundings (sub, mul, add) and no contraction,
// so a float32 restatement gives the same bits.  One thread forms four neighbouring columns: a 16-byte load of each row where VEC (ld a
// multiple of 4 and the three bases 16-byte aligned), four scalar loads otherwise; a group that reaches past V is finished by scalars, and
// columns V .. ld - 1 are never written.  out may be cond: a thread reads its columns before it writes them and no other thread reads them.
// The rule is __fadd_rn(n, __fmul_rn(s, __fsub_rn(l, n))).  It is written with plain operators under `fp contract(off)`: this compiler's
// __fmul_rn / __fadd_rn are the plain operators themselves, compiled with contraction allowed, and fuse into one v_fma after inlining.
__device__ __forceinline__ float guide_one(float l, float n, float s) {
#pragma clang fp contract(off)
    const float d = l - n;
    const float m = s * d;
    return n + m;
}

template <bool VEC>
__device__ __forceinline__ void guide_logits_row(const float* cond, const float* null, float* out, int V, int ld, float s) {
    const size_t base = (size_t)blockIdx.x * ld;                       // one row per blockIdx.x, 1024 columns per blockIdx.y
    const int c0 = 4 * (blockIdx.y * 256 + threadIdx.x);
    if (c0 >= V) return;
    if (VEC && c0 + 3 < V) {
        const float4 l = *(const float4*)(cond + base + c0);
        const float4 n = *(const float4*)(null + base + c0);
        float4 g;
        g.x = guide_one(l.x, n.x, s); g.y = guide_one(l.y, n.y, s); g.z = guide_one(l.z, n.z, s); g.w = guide_one(l.w, n.w, s);
        *(float4*)(out + base + c0) = g;
        return;
    }
    const int c1 = c0 + 4 < V ? c0 + 4 : V;
    for (int c = c0; c < c1; ++c) out[base + c] = guide_one(cond[base + c], null[base + c], s);
}
template <bool VEC>
__global__ __launch_bounds__(256) void guide_logits_kernel(const float* cond, const float* null, float* out, int V, int ld, float s) {
    guide_logits_row<VEC>(cond, null, out, V, ld, s);
}
// the same with a scale per row (omlm_guide_logits_rows): one workgroup-uniform load, then the code above
template <bool VEC>
__global__ __launch_bounds__(256) void guide_logits_rows_kernel(const float* cond, const float* null, float* out, int V, int ld,
                                                                const float* __restrict__ scale) {
    guide_logits_row<VEC>(cond, null, out, V, ld, scale[blockIdx.x]);
}

extern "C" int omlm_guide_logits(const float* cond, const float* null, float* out, int rows, int V, int ld, float scale, void* stream) {
    if (rows <= 0) return OMLM_OK;
    OMLM_CHECK_ARG(cond && null && out && V > 0 && ld >= V && V <= (1 << 24), "guide_logits arguments (0 < V <= ld, V <= 2^24)");
    OMLM_CHECK_ARG(scale >= 0.f && scale <= 3.4028234e38f, "guide_logits: scale must be a finite number >= 0");
    const bool vec = ld % 4 == 0 && (((size_t)cond | (size_t)null | (size_t)out) & 15) == 0;
    const dim3 grid(rows, (V + 1023) / 1024);
    if (vec) hipLaunchKernelGGL(guide_logits_kernel<true>, grid, dim3(256), 0, as_stream(stream), cond, null, out, V, ld, scale);
    else     hipLaunchKernelGGL(guide_logits_kernel<false>, grid, dim3(256), 0, as_stream(stream), cond, null, out, V, ld, scale);
    return omlm_post_launch("omlm_guide_logits");
}
// scale [rows] on the device: not checked (a non-finite value gives non-finite g in its own row, nothing out of range)
extern "C" int omlm_guide_logits_rows(const float* cond, const float* null, float* out, int rows, int V, int ld, const float* scale,
                                      void* stream) {
    if (rows <= 0) return OMLM_OK;
    OMLM_CHECK_ARG(cond && null && out && V > 0 && ld >= V && V <= (1 << 24), "guide_logits_rows arguments (0 < V <= ld, V <= 2^24)");
    OMLM_CHECK_ARG(scale != nullptr, "guide_logits_rows: scale (fp32 [rows], device)");
    const bool vec = ld % 4 == 0 && (((size_t)cond | (size_t)null | (size_t)out) & 15) == 0;
    const dim3 grid(rows, (V + 1023) / 1024);
    if (vec) hipLaunchKernelGGL(guide_logits_rows_kernel<true>, grid, dim3(256), 0, as_stream(stream), cond, null, out, V, ld, scale);
    else     hipLaunchKernelGGL(guide_logits_rows_kernel<false>, grid, dim3(256), 0, as_stream(stream), cond, null, out, V, ld, scale);
    return omlm_post_launch("omlm_guide_logits_rows");
}

// twin: what the sampler left for the conditional rows -- the sampled ids [rows] and their gathered embedding rows [rows, D] -- copied to
// the null twins' halves, in one launch.  Workgroup r copies id r (thread 0) and row r; either pair of pointers may be null.
template <bool VEC>
__global__ __launch_bounds__(256) void decode_twin_kernel(const long long* ids, long long* ids_twin, const float* x, float* x_twin, int D) {
    const int r = blockIdx.x;
    if (ids && threadIdx.x == 0) ids_twin[r] = ids[r];
    if (!x) return;
    const float* src = x + (size_t)r * D;
    float* dst = x_twin + (size_t)r * D;
    if (VEC) for (int i = threadIdx.x; i < D / 4; i += 256) ((float4*)dst)[i] = ((const float4*)src)[i];
    else     for (int i = threadIdx.x; i < D; i += 256) dst[i] = src[i];
}

extern "C" int omlm_decode_twin(const long long* ids, long long* ids_twin, const float* x, float* x_twin, int rows, int D, void* stream) {
    if (rows <= 0) return OMLM_OK;
    OMLM_CHECK_ARG((ids != nullptr) == (ids_twin != nullptr) && (x != nullptr) == (x_twin != nullptr), "decode_twin: a source without its twin");
    if (!ids && !x) return OMLM_OK;
    OMLM_CHECK_ARG(!x || D > 0, "decode_twin: D");
    const bool vec = x && D % 4 == 0 && (((size_t)x | (size_t)x_twin) & 15) == 0;
    if (vec) hipLaunchKernelGGL(decode_twin_kernel<true>, dim3(rows), dim3(256), 0, as_stream(stream), ids, ids_twin, x, x_twin, D);
    else     hipLaunchKernelGGL(decode_twin_kernel<false>, dim3(rows), dim3(256), 0, as_stream(stream), ids, ids_twin, x, x_twin, D);
    return omlm_post_launch("omlm_decode_twin");
}
