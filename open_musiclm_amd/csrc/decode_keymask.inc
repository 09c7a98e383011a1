// The cached decode's two attention kernels under a key mask (omlm_decode_step_masked, include/omlm.h); included by decode.hip behind
// dec_attn_kernel and dec_attn2_kernel.  Each is its unmasked kernel line for line -- same loads, same LDS layout, same order of every
// sum, the same ticket protocol -- plus one predicate:
//   key_live [B, Nmax] bytes, nonzero = attend.  The lane that owns key j0 + lane reads its byte (dec_attn2: with the other global loads at
//   the top, in front of the single barrier).  A masked key gets what an out-of-range lane gets: sv = -3.0e38f and p = 0.  p is SET, not
//   computed: in a range whose 64 keys are all masked m is -3.0e38f as well and __expf(sv - m) would give every masked key weight 1.
//   Such a range leaves the partial {m = -3.0e38f, l = 0, o = 0}.
// Every consumer of the partials -- stage_attention, dec2_stage_attention, dec_attn_combine_kernel, the last arriver below -- weighs a
// partial with __expf(m_part - m_all) and multiplies l and o by it.  The new key, row pos, is always live (the caller's duty: byte pos of
// every sample is 1), so m_all is finite, a fully masked partial gets __expf(-3.0e38f - m_all) = 0 and contributes 0 * 0; where a batch of
// eight partials in front of the first live one is all masked, the running (m, l, o) stays (-3.0e38f, 0, 0) through weights __expf(0) = 1
// on zeros, and is rescaled by 0 at the first live partial.  No NaN arises and l > 0 at the division, so the consumers are used as they are.
// Masked ranges are not skipped: their K / V are loaded and their workgroups take their tickets, so the per-sample count still reaches
// pos / 64 + 1.  The normalisation and write-back of the new key do not look at the mask.
// The unmasked kernels stay separate so that they compile to exactly what they compiled to before; a mask of all ones gives their bits
// (tests/test_gpu_decode_keymask.py), which is what keeps the two copies together.
template <typename TC>
__global__ __launch_bounds__(DEC_T) void dec_attn_masked_kernel(const float* __restrict__ q, TC* __restrict__ Kc,
                                                        const TC* __restrict__ Vc, const float* __restrict__ q_scale,
                                                        const float* __restrict__ k_scale, const float* __restrict__ bias, int bias_ld,
                                                        float* __restrict__ parts, int H, int Nmax, int nsplit,
                                                        const int* __restrict__ pos_dev, float scale, int round_bf16,
                                                        const float* __restrict__ k_new, const unsigned char* __restrict__ key_live) {
    constexpr bool KV16 = !std::is_same<TC, float>::value;
    extern __shared__ __attribute__((aligned(16))) float dsm[];
    const int pos = *pos_dev;
    const int s = blockIdx.x, b = blockIdx.y;
    const int j0 = s * DEC_KS;
    if (j0 > pos) return;
    const int nk = min(DEC_KS, pos + 1 - j0);
    float* Ks = dsm;                        // [64][65]
    float* Vs = Ks + 64 * 65;               // [64][64]
    float* qn = Vs + 64 * 64;               // [H][64]
    float* sc = qn + H * 64;                // [H][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int h = wave; h < H; h += 4) {                                   // q: l2norm * q_scale per head (utils.py:68-69)
        const float v = q[(size_t)b * H * 64 + h * 64 + lane];
        const float nrm = fmaxf(sqrtf(wave_sum(v * v)), 1e-12f);
        qn[h * 64 + lane] = round_if(v / nrm * q_scale[lane], round_bf16);
    }
    TC* Kb = Kc + ((size_t)b * Nmax + j0) * 64;
    const TC* Vb = Vc + ((size_t)b * Nmax + j0) * 64;
    if constexpr (!KV16) {
        for (int idx = threadIdx.x; idx < nk * 16; idx += DEC_T) {        // coalesced float4 rows
            const int j = idx >> 4, c = idx & 15;
            const float4 kk = ((const float4*)(Kb + (size_t)j * 64))[c];
            const float4 vv = ((const float4*)(Vb + (size_t)j * 64))[c];
            Ks[j * 65 + 4 * c] = kk.x; Ks[j * 65 + 4 * c + 1] = kk.y; Ks[j * 65 + 4 * c + 2] = kk.z; Ks[j * 65 + 4 * c + 3] = kk.w;
            *(float4*)(Vs + j * 64 + 4 * c) = vv;
        }
    } else {
        for (int idx = threadIdx.x; idx < nk * 8; idx += DEC_T) {         // coalesced 16-byte chunks: 8 per 128-byte row
            const int j = idx >> 3, c = idx & 7;
            float kf[8], vf[8];
            load_w8(Kb + (size_t)j * 64 + 8 * c, kf);                     // (row pos - j0 is stale here; replaced below)
            load_w8(Vb + (size_t)j * 64 + 8 * c, vf);
#pragma unroll
            for (int e = 0; e < 8; ++e) Ks[j * 65 + 8 * c + e] = kf[e];
            *(float4*)(Vs + j * 64 + 8 * c) = make_float4(vf[0], vf[1], vf[2], vf[3]);
            *(float4*)(Vs + j * 64 + 8 * c + 4) = make_float4(vf[4], vf[5], vf[6], vf[7]);
        }
    }
    __syncthreads();
    if (pos - j0 < DEC_KS && wave == 0) {                                 // the new key: normalise once, keep it in the cache
        const int j = pos - j0;
        float v;
        if constexpr (KV16) v = k_new[(size_t)b * 64 + lane];
        else v = Ks[j * 65 + lane];
        const float nrm = fmaxf(sqrtf(wave_sum(v * v)), 1e-12f);
        const float kn = round_if(v / nrm * k_scale[lane], round_bf16);
        Ks[j * 65 + lane] = kn;
        Kb[(size_t)j * 64 + lane] = (TC)kn;                               // (kn is a 16-bit number already: exact)
    }
    __syncthreads();
    const bool live = lane < nk && key_live[(size_t)b * Nmax + j0 + min(lane, nk - 1)] != 0;     // (rows j0 .. j0 + nk - 1 <= pos < Nmax only)
    for (int h = wave; h < H; h += 4) {                                   // one wave per head: lane = key
        float dot = 0.f;
        if (lane < nk) {
#pragma unroll 16
            for (int d = 0; d < 64; ++d) dot += qn[h * 64 + d] * Ks[lane * 65 + d];
        }
        const float sv = live ? dot * scale + (bias ? bias[(size_t)(pos - j0 - lane) * bias_ld + h] : 0.f) : -3.0e38f;
        const float m = wave_max(sv);
        const float p = live ? __expf(sv - m) : 0.f;                        // (set, not computed: all 64 masked -> sv == m)
        const float l = wave_sum(p);
        sc[h * 64 + lane] = p;
        if (lane == 0) {
            float* pp = parts + (((size_t)b * nsplit + s) * H + h) * DEC_PART;
            pp[0] = m; pp[1] = l;
        }
    }
    __syncthreads();
    for (int h = wave; h < H; h += 4) {                                   // lane = dim
        float acc = 0.f;
        for (int j = 0; j < nk; ++j) acc += sc[h * 64 + j] * Vs[j * 64 + lane];
        parts[(((size_t)b * nsplit + s) * H + h) * DEC_PART + 2 + lane] = acc;
    }
}

template <typename TC>
__global__ __launch_bounds__(DEC_AT2) void dec_attn2_masked_kernel(const float* q, TC* __restrict__ Kc,
                                                           const TC* __restrict__ Vc, const float* __restrict__ q_scale,
                                                           const float* __restrict__ k_scale, const float* __restrict__ bias, int bias_ld,
                                                           float* parts, int H, int Nmax, int nsplit,
                                                           const int* __restrict__ pos_dev, float scale, int round_bf16,
                                                           float* comb_out, int* comb_cnt, const float* __restrict__ k_new,
                                                           const unsigned char* __restrict__ key_live) {
    constexpr bool KV16 = !std::is_same<TC, float>::value;
    extern __shared__ __attribute__((aligned(16))) float dsm[];
    const int pos = *pos_dev;
    const int s = blockIdx.x, b = blockIdx.y;
    const int j0 = s * DEC_KS;
    if (j0 > pos) return;
    const int nk = min(DEC_KS, pos + 1 - j0);
    float* Ks = dsm;                        // [64][65]
    float* Vs = Ks + 64 * 65;               // [64][64]
    float* qn = Vs + 64 * 64;               // [H][64]
    float* sc = qn + H * 64;                // [8 waves][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    TC* Kb = Kc + ((size_t)b * Nmax + j0) * 64;
    const TC* Vb = Vc + ((size_t)b * Nmax + j0) * 64;
    // ---- all global loads first ----
    float4 kk[2], vv[2];                                        // fp32 cache: two rows of 16 float4s per 16 lanes
    u32x4 kh, vh;                                               // 16-bit cache: one chunk of 8 elements of row threadIdx.x >> 3
    const int c16 = threadIdx.x & 15, c8 = threadIdx.x & 7;
    const int jn = pos - j0;                                    // tile row of the new key (>= DEC_KS: another range holds it)
    if constexpr (!KV16) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int j = (threadIdx.x >> 4) + 32 * i;
            const int jj = min(j, nk - 1);
            kk[i] = ((const float4*)(Kb + (size_t)jj * 64))[c16];
            vv[i] = ((const float4*)(Vb + (size_t)jj * 64))[c16];
        }
    } else {
        const int jj = min((int)(threadIdx.x >> 3), nk - 1);     // (a clamped row is dropped below; rows <= pos < Nmax only)
        kh = *(const u32x4*)(Kb + (size_t)jj * 64 + 8 * c8);
        vh = *(const u32x4*)(Vb + (size_t)jj * 64 + 8 * c8);
        kk[0] = ((const float4*)(k_new + (size_t)b * 64))[c16];  // the raw key, fp32 (used where jn < DEC_KS)
    }
    const float4 ks4 = ((const float4*)k_scale)[c16];
    float qv[2] = {0.f, 0.f};
    const float qs = q_scale[lane];
    for (int h = wave, i = 0; h < H; h += 8, ++i) qv[i] = q[(size_t)b * H * 64 + h * 64 + lane];
    const unsigned char lv = key_live[(size_t)b * Nmax + j0 + min(lane, nk - 1)];     // the lane's key (a clamped lane is dropped below)
    // ---- q: l2norm * q_scale per head (utils.py:68-69), one wave per head ----
    for (int h = wave, i = 0; h < H; h += 8, ++i) {
        const float nrm = fmaxf(sqrtf(wave_sum(qv[i] * qv[i])), 1e-12f);
        qn[h * 64 + lane] = round_if(qv[i] / nrm * qs, round_bf16);
    }
    // ---- K / V tiles to LDS; the row written by dec_qkv this step is raw: normalise it here, keep it in the cache ----
    if constexpr (!KV16) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int j = (threadIdx.x >> 4) + 32 * i;
            float4 kx = kk[i];
            if (j == pos - j0) {                                    // uniform over the 16 lanes that hold this row
                float ss = kx.x * kx.x + kx.y * kx.y + kx.z * kx.z + kx.w * kx.w;
                ss += __shfl_xor(ss, 1, 64); ss += __shfl_xor(ss, 2, 64); ss += __shfl_xor(ss, 4, 64); ss += __shfl_xor(ss, 8, 64);
                const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
                kx.x = round_if(kx.x * inv * ks4.x, round_bf16); kx.y = round_if(kx.y * inv * ks4.y, round_bf16);
                kx.z = round_if(kx.z * inv * ks4.z, round_bf16); kx.w = round_if(kx.w * inv * ks4.w, round_bf16);
                ((float4*)(Kb + (size_t)j * 64))[c16] = kx;
            }
            if (j < nk) {
                Ks[j * 65 + 4 * c16] = kx.x; Ks[j * 65 + 4 * c16 + 1] = kx.y; Ks[j * 65 + 4 * c16 + 2] = kx.z; Ks[j * 65 + 4 * c16 + 3] = kx.w;
                *(float4*)(Vs + j * 64 + 4 * c16) = vv[i];
            }
        }
    } else {
        if ((int)(threadIdx.x >> 4) == (jn & 31) && jn < DEC_KS) {  // the 16 lanes that hold row jn above: same lanes, same order, same bits
            float4 kx = kk[0];
            float ss = kx.x * kx.x + kx.y * kx.y + kx.z * kx.z + kx.w * kx.w;
            ss += __shfl_xor(ss, 1, 64); ss += __shfl_xor(ss, 2, 64); ss += __shfl_xor(ss, 4, 64); ss += __shfl_xor(ss, 8, 64);
            const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
            kx.x = round_if(kx.x * inv * ks4.x, round_bf16); kx.y = round_if(kx.y * inv * ks4.y, round_bf16);
            kx.z = round_if(kx.z * inv * ks4.z, round_bf16); kx.w = round_if(kx.w * inv * ks4.w, round_bf16);
            store4_from_float(Kb + (size_t)jn * 64 + 4 * c16, kx.x, kx.y, kx.z, kx.w);      // (16-bit numbers already: exact)
            Ks[jn * 65 + 4 * c16] = kx.x; Ks[jn * 65 + 4 * c16 + 1] = kx.y; Ks[jn * 65 + 4 * c16 + 2] = kx.z; Ks[jn * 65 + 4 * c16 + 3] = kx.w;
        }
        const int j = threadIdx.x >> 3;
        if (j < nk) {
            if (j != jn) {                                          // (row jn of the cache is stale until the store above)
#pragma unroll
                for (int e = 0; e < 4; ++e) { Ks[j * 65 + 8 * c8 + 2 * e] = h16_lo_to_f(kh[e]); Ks[j * 65 + 8 * c8 + 2 * e + 1] = h16_hi_to_f(kh[e]); }
            }
            *(float4*)(Vs + j * 64 + 8 * c8) = make_float4(h16_lo_to_f(vh[0]), h16_hi_to_f(vh[0]), h16_lo_to_f(vh[1]), h16_hi_to_f(vh[1]));
            *(float4*)(Vs + j * 64 + 8 * c8 + 4) = make_float4(h16_lo_to_f(vh[2]), h16_hi_to_f(vh[2]), h16_lo_to_f(vh[3]), h16_hi_to_f(vh[3]));
        }
    }
    __syncthreads();
    const bool live = lane < nk && lv != 0;
    for (int h = wave; h < H; h += 8) {                                   // lane = key, then lane = dim
        float dot = 0.f;
        if (lane < nk) {
#pragma unroll 16
            for (int d = 0; d < 64; ++d) dot += qn[h * 64 + d] * Ks[lane * 65 + d];
        }
        const float sv = live ? dot * scale + (bias ? bias[(size_t)(pos - j0 - lane) * bias_ld + h] : 0.f) : -3.0e38f;
        const float m = wave_max(sv);
        const float p = live ? __expf(sv - m) : 0.f;                        // (set, not computed: all 64 masked -> sv == m)
        const float l = wave_sum(p);
        sc[wave * 64 + lane] = p;
        float* pp = parts + (((size_t)b * nsplit + s) * H + h) * DEC_PART;
        if (lane == 0) { pp[0] = m; pp[1] = l; }
        float acc = 0.f;
        for (int j = 0; j < nk; ++j) acc += sc[wave * 64 + j] * Vs[j * 64 + lane];
        pp[2 + lane] = acc;
    }
    if (!comb_cnt) return;
    // publish the partials, take a ticket (cdna_hip_programming.md: slab stores -> every wave vmcnt(0) -> barrier -> one lane: agent-scope
    // release, vmcnt(0), relaxed ticket; the last arriver: agent-scope acquire -> barrier -> plain loads)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        sc[0] = __int_as_float(__hip_atomic_fetch_add(comb_cnt + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    __syncthreads();
    const int ns = pos / DEC_KS + 1;
    if (__float_as_int(sc[0]) != ns - 1) return;
    if (threadIdx.x == 0) { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); comb_cnt[b] = 0; }
    __syncthreads();
    for (int h = wave; h < H; h += 8) {                                   // lane = dim (the arithmetic of dec_attn_combine_kernel)
        const float* pb = parts + ((size_t)b * nsplit * H + h) * DEC_PART;
        float m = -3.0e38f, l = 0.f, o = 0.f;
        for (int s0 = 0; s0 < ns; s0 += 8) {
            float pm[8], pl[8], po[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float* p = pb + (size_t)min(s0 + j, ns - 1) * H * DEC_PART;
                pm[j] = p[0]; pl[j] = p[1]; po[j] = p[2 + lane];
            }
            float mb = m;
#pragma unroll
            for (int j = 0; j < 8; ++j) if (s0 + j < ns) mb = fmaxf(mb, pm[j]);
            const float resc = __expf(m - mb);
            l *= resc; o *= resc; m = mb;
#pragma unroll
            for (int j = 0; j < 8; ++j) if (s0 + j < ns) { const float w = __expf(pm[j] - m); l += w * pl[j]; o += w * po[j]; }
        }
        comb_out[((size_t)b * H + h) * 64 + lane] = round_if(o / l, round_bf16);
    }
}
