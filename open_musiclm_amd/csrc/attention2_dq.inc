// The dQ / d(bias) / delta kernel of attention2.hip, included once per compiled form (the text is the kernel itself, so the short form
// compiles to exactly what it compiled to as a plain kernel):
//   A2Q_KERNEL attn2_bwd_dq_kernel,      A2Q_LONG false: its LDS holds the whole sequence's mask and bins (N up to about 2040)
//   A2Q_KERNEL attn2_bwd_dq_long_kernel, A2Q_LONG true:  4096 < N <= A2_NL, causal; LDS: the ring + 4 KiB scratch + 4 KiB of bin rings + N
//   bytes (108 KiB at A2_NL): one workgroup per CU, as the short form has at the bench shape.
// LONG: nothing in LDS grows with N but one BYTE per key.
//   * key mask: a byte per key, 0x00 live / 0xF1 dead; shifted into a float's top byte it is +0.0 / -2^99, so a live score is computed by
//     exactly the instructions of the short form (bias + 0.0 - lse) and a dead one still leaves through exp2(-huge) = 0;
//   * d(bias) bins: a ring of A2_BINW = 128 bins per wave, indexed rel & 127.  Key tile t touches the distances i0 - 64 t - 63 .. i0 - 64 t + 31
//     (95 < 128 of them), and the walk goes down in distance, so after tile t the 64 bins i0 - 64 t - 32 .. i0 - 64 t + 31 are final: lane L
//     stores bin i0 - 64 t - 32 + L to the wave's partial row (plain store; null workspace: atomic into the table) and zeroes its slot,
//     which tile t + 1 reuses for distance (that bin) - 128.  The last tile's flush reaches distance <= 0, so nothing is left at the end.
//     The stores count in vmcnt behind the tile's DMA requests: the counted waits of the ring only get stricter by them, never looser.
template <bool DROP = false, bool PFX = false>
__global__ __launch_bounds__(A2_THREADS) void A2Q_KERNEL(const h16_t* __restrict__ q, const h16_t* __restrict__ k,
                                                         const h16_t* __restrict__ v, const float* __restrict__ biasT, int ldT,
                                                         const unsigned char* __restrict__ keymask, const h16_t* __restrict__ out,
                                                         const h16_t* __restrict__ dout, const float* __restrict__ lse,
                                                         float* __restrict__ delta, float* __restrict__ dq, float* __restrict__ dbias,
                                                         int bias_ld, float* __restrict__ dpart, int B, int N, int H, float scale,
                                                         const AttnDrop drop, int Pn) {
    constexpr bool LONG = A2Q_LONG;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* ring = smem;
    char* scratch = smem + A2_NST * A2B_STAGE;
    const int npad = (N + 63) / 64 * 64;
    float* mb = (float*)(scratch + 4096);                     // [npad] 0 / -1e30 per key of this sample
    float* dbl = mb + npad;                                   // [8 waves][nbp]
    unsigned char* mby = (unsigned char*)(scratch + 4096 + 8 * A2_BINW * 4);      // LONG: [npad] bytes behind the 8 bin rings
    const int nqt = (N + 31) / 32, ny = (H + 7) / 8;
    int b, qt, hy;
    a2_item_order(blockIdx.x, nqt, ny, B, b, qt, hy);
    const int lane = threadIdx.x & 63, hi = lane >> 5, ql = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = hy * 8 + wave;
    const bool active = h < H;
    const int i0 = qt * 32, qi = i0 + ql;
    const int nb = i0 + 32;                                   // rel in [0, i0 + 31]
    const size_t rowbase = (size_t)b * N;
    const int off = PFX ? Pn - 1 : 0;                         // PFX: negative-distance bins in front
    const int kend = PFX && i0 < Pn ? max(i0 + 32, Pn) : i0 + 32;
    const int nkt = min((kend + A2_TKV - 1) / A2_TKV, (N + A2_TKV - 1) / A2_TKV);
    float* dbw = LONG ? (float*)(scratch + 4096) + wave * A2_BINW      // index rel & (A2_BINW - 1)
                      : dbl + (size_t)wave * (nb + off) + off;        // index rel

    if (LONG) {     // the mask bytes in passes of 4096 keys, a pass's eight loads in flight together; this wave's bin ring zeroed
        const int nkeys = nkt * A2_TKV;
        for (int base = 0; base < nkeys; base += 8 * A2_THREADS) {
            unsigned char mk[8];
#pragma unroll
            for (int it = 0; it < 8; ++it) mk[it] = 1;
            if (keymask) {                                      // unconditional loads at clamped indices: all eight leave before the first wait
#pragma unroll
                for (int it = 0; it < 8; ++it) mk[it] = keymask[rowbase + min(base + it * A2_THREADS + (int)threadIdx.x, N - 1)];
            }
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int j = base + it * A2_THREADS + (int)threadIdx.x;
                if (j < nkeys) mby[j] = (j < N && mk[it] != 0) ? (unsigned char)0x00 : (unsigned char)0xF1;
            }
        }
        dbw[lane] = 0.f; dbw[lane + 64] = 0.f;
    } else
    {   // additive key mask, all byte loads in flight at once; this wave's d(bias) bins zeroed
        unsigned char mk[8];
#pragma unroll
        for (int it = 0; it < 8; ++it) mk[it] = 1;
        if (keymask) {
#pragma unroll
            for (int it = 0; it < 8; ++it) mk[it] = keymask[rowbase + min(it * A2_THREADS + (int)threadIdx.x, N - 1)];
        }
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int j = it * A2_THREADS + threadIdx.x;
            if (j < nkt * A2_TKV) mb[j] = (j < N && mk[it] != 0) ? 0.f : A2_NEG;
        }
        if (dbias) for (int r = lane - off; r < nb; r += 64) dbw[r] = 0.f;
    }
    __syncthreads();
    // per-lane DMA source offsets: K rows and V rows use the row image, K blocked the blocked image (see A2Stager)
    A2Stager stg;
    stg.init(wave, lane, ldT);
    const a2_rsrc rsK = a2_make_rsrc(k + rowbase * 64, (unsigned)N * 128u);
    const a2_rsrc rsV = a2_make_rsrc(v + rowbase * 64, (unsigned)N * 128u);
    const a2_rsrc rsB = a2_make_rsrc(biasT ? (const void*)(biasT + (size_t)hy * 8 * ldT) : (const void*)k, biasT ? (unsigned)(8 * ldT * 4) : 0u);
    const unsigned ring_lds = (unsigned)(size_t)LDS_PTR(char, ring), scratch_lds = (unsigned)(size_t)LDS_PTR(char, scratch);
    auto issue = [&](int t) {                                  // 4 DMA wave-instructions per wave per tile
        const unsigned st = ring_lds + (unsigned)((t % A2_NST) * A2B_STAGE);
        const int j0 = t * A2_TKV;
        a2_dma(rsK, st + wave * 1024, (unsigned)(j0 * 128) + stg.koff);
        a2_dma(rsK, st + 8192 + wave * 1024, (unsigned)(j0 * 128) + stg.voff);
        a2_dma(rsV, st + 16384 + wave * 1024, (unsigned)(j0 * 128) + stg.koff);
        const unsigned w0 = (unsigned)((A2_PAD + off + i0 - j0 - 64) * 4);
        if (stg.bias_wave) a2_dma(rsB, st + 24576 + (wave & 3) * 1024, w0 + stg.boff);
        else               a2_dma(rsB, scratch_lds + (wave & 3) * 1024, OOB_OFF);
    };
    issue(0);
    if (nkt > 1) issue(1);

    // Q and dO fragments (B operands), delta_i = sum_d dO O, the row's log-sum-exp relative to the table's reference point
    h16x8 qf[4], dof[4];
    float dl = 0.f;
    const size_t qrow = (rowbase + min(qi, N - 1)) * (size_t)(H * 64) + (size_t)(active ? h : 0) * 64;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        u32x4 z = {0u, 0u, 0u, 0u};
        const bool ok = active && qi < N;
        const u32x4 qv = ok ? *(const u32x4*)(q + qrow + 16 * s + 8 * hi) : z;
        const u32x4 dv = ok ? *(const u32x4*)(dout + qrow + 16 * s + 8 * hi) : z;
        const u32x4 ov = ok ? *(const u32x4*)(out + qrow + 16 * s + 8 * hi) : z;
        qf[s] = __builtin_bit_cast(h16x8, qv);
        dof[s] = __builtin_bit_cast(h16x8, dv);
#pragma unroll
        for (int e = 0; e < 4; ++e) dl += h16_lo_to_f(dv[e]) * h16_lo_to_f(ov[e]) + h16_hi_to_f(dv[e]) * h16_hi_to_f(ov[e]);
    }
    dl += __shfl_xor(dl, 32, 64);
    float Lp = 0.f;
    if (active) {
        Lp = lse[((size_t)b * H + h) * N + min(qi, N - 1)];
        if (biasT) Lp -= biasT[(size_t)h * ldT + (ldT - 1)];     // the table is stored relative to its reference point m_h
        if (hi == 0 && qi < N) delta[((size_t)b * H + h) * N + qi] = dl;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) { asm volatile("" : "+v"(qf[s])); asm volatile("" : "+v"(dof[s])); }
    asm volatile("" : "+v"(Lp), "+v"(dl));                    // every prologue load is consumed before the tile loop
    unsigned rk = 0u;                                         // DROP: row key of (b, h, qi) with this half-wave's key bit (see the forward)
    if (DROP) rk = attn_drop_headkey(attn_drop_seed(drop), b, h) ^ ((unsigned)qi << 15) ^ (2u * (unsigned)hi);

    f32x16 acc[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; }
    const float c = scale * A2_LOG2E;

    for (int t = 0; t < nkt; ++t) {
        if (t + 1 < nkt) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else             asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (t + 2 < nkt) issue(t + 2);
        if (!active) continue;
        const char* Kr = ring + (t % A2_NST) * A2B_STAGE;
        const char* Kb = Kr + 8192;
        const char* Vr = Kr + 16384;
        const float* bw = (const float*)(Kr + 24576) + wave * A2_BWIN;
        const int j0 = t * A2_TKV;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int jb = j0 + 32 * sub;
            if (jb > kend - 1) break;
            f32x16 st, dp;
#pragma unroll
            for (int e = 0; e < 16; ++e) { st[e] = 0.f; dp[e] = 0.f; }
            {   // all eight fragment reads in flight before the first MFMA, retired in two groups (hipcc issued them one at a time
                // through the same four registers: read -> wait -> MFMA, seen in the ISA)
                h16x8 kfr[4], vfr[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) { kfr[s] = a2_frag_rows(Kr, 32 * sub, s, lane); vfr[s] = a2_frag_rows(Vr, 32 * sub, s, lane); }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    if ((s & 1) == 0) asm volatile("" : "+v"(kfr[s]), "+v"(vfr[s]), "+v"(kfr[s + 1]), "+v"(vfr[s + 1]));
                    st = MFMA16(kfr[s], qf[s], st);                               // S^T  = K Q^T
                    dp = MFMA16(vfr[s], dof[s], dp);                              // dP^T = V dO^T
                }
            }
            const float* bp = bw + (64 - 32 * sub) + ql - 4 * hi;
            const float* mp = mb + jb + 4 * hi;
            float bv[16];
            const bool diag = jb + 31 > i0;
            const int d0 = qi - (jb + 4 * hi);
            float4 m4s[4];
            if (LONG) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const unsigned w = *(const unsigned*)(mby + jb + 4 * hi + 8 * g);       // keys jb + 4 hi + 8 g + {0 .. 3}
                    m4s[g] = make_float4(__uint_as_float((w << 24) & 0xFF000000u), __uint_as_float((w << 16) & 0xFF000000u),
                                         __uint_as_float((w << 8) & 0xFF000000u), __uint_as_float(w & 0xFF000000u));
                }
            } else {
#pragma unroll
            for (int g = 0; g < 4; ++g) m4s[g] = *(const float4*)(mp + 8 * g);
            }
            float bpv[16];                     // bias window gathered in one pass (see m4s: nothing waits element by element)
#pragma unroll
            for (int r = 0; r < 16; ++r) bpv[r] = bp[-((r & 3) + 8 * (r >> 2))];
#pragma unroll
            for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(bpv[r]));
            if (diag) {                        // the block on the diagonal: keys above it leave through the bias term (a real branch: one block in nkt)
                int d0v = d0;
                asm volatile("" : "+v"(d0v));             // the selects depend on a value defined inside the branch: hipcc otherwise hoists all 16 of them in front of it
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int cr = (r & 3) + 8 * (r >> 2);
                    bpv[r] = (d0v - cr >= 0 || (PFX && qi < Pn && jb + 4 * hi + cr < Pn)) ? bpv[r] : A2_NEG;
                }
            }
            // element arithmetic on register pairs (v_pk_fma_f32 / v_pk_add_f32 / v_pk_mul_f32); the softmax scale is applied once to
            // dQ (dQ = scale dS K) instead of to every dS
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 m4 = m4s[g];
                const f32x2 mm2[2] = {{m4.x, m4.y}, {m4.z, m4.w}};
#pragma unroll
                for (int pq = 0; pq < 2; ++pq) {
                    const int r = 4 * g + 2 * pq, cr = 2 * pq + 8 * g;
                    const f32x2 t2 = (f32x2{bpv[r], bpv[r + 1]} + mm2[pq]) - f32x2{Lp, Lp};
                    const f32x2 x2 = __builtin_elementwise_fma(f32x2{st[r], st[r + 1]}, f32x2{c, c}, t2);
                    const f32x2 pr2 = {__builtin_amdgcn_exp2f(x2[0]), __builtin_amdgcn_exp2f(x2[1])};
                    f32x2 dp2 = {dp[r], dp[r + 1]};
                    if (DROP) {                // dropout: dS = P (Z dP~ / (1 - p) - delta); keys jb + 4 hi + cr + {0, 1} share one word
                        const unsigned w = omlm_hash32(rk ^ (unsigned)(jb >> 1) ^ (unsigned)(cr >> 1));
                        dp2 = dp2 * f32x2{drop.rs, drop.rs};
                        dp2 = f32x2{(w << 16) >= drop.thr16 ? dp2[0] : 0.f, w >= drop.thr16 ? dp2[1] : 0.f};
                    }
                    const f32x2 ds2 = pr2 * (dp2 - f32x2{dl, dl});   // dS = P (dP - delta), 0 where masked; scale: see the dQ store
                    bv[r] = ds2[0]; bv[r + 1] = ds2[1];
                    st[r] = ds2[0]; st[r + 1] = ds2[1];
                }
            }
            if (dbias) {
                // d(bias)[rel] = sum of dS over the diagonal rel = i - j: output lane L stands for t = q - kr = L - 31 and pulls row
                // kr's element from query column q = t + kr through the cross-lane permute; then one read-add-write of this
                // wave's private table (every lane owns a distinct bin)
                const float dsum = diag_sum_32x32(bv, lane);
                const int rel = (i0 - jb) + (lane - 31);
                if (LONG) { if (rel >= 0 && rel < nb) dbw[rel & (A2_BINW - 1)] += dsum; }
                else
                if (rel >= -off && rel < nb) dbw[rel] += dsum;      // (ds_add_f32 instead of this read-add-write: measured 20 us per layer SLOWER)
            }
            {
                h16x8 ktf[2][2], dsb[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) { ktf[s][0] = a2_frag_cols_tr(Kb, 32 * sub, s, 0, lane); ktf[s][1] = a2_frag_cols_tr(Kb, 32 * sub, s, 32, lane); }
#pragma unroll
                for (int s = 0; s < 2; ++s) dsb[s] = a2_pack(st, s);
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    asm volatile("" : "+v"(ktf[s][0]), "+v"(ktf[s][1]));
                    acc[0] = MFMA16(ktf[s][0], dsb[s], acc[0]);                                // dQ^T += K^T dS^T
                    acc[1] = MFMA16(ktf[s][1], dsb[s], acc[1]);
                }
            }
        }
        if (LONG && dbias) {                                  // the 64 bins this tile has made final leave; their slots start the next tile at zero
            const int rel = i0 - j0 - 32 + lane;
            if (rel >= 0) {
                const float vv = dbw[rel & (A2_BINW - 1)];
                dbw[rel & (A2_BINW - 1)] = 0.f;
                if (dpart) dpart[(((size_t)b * H + h) * nqt + qt) * (size_t)(nqt * 32) + rel] = vv;
                else if (vv != 0.f && rel < N) unsafeAtomicAdd(dbias + (size_t)rel * bias_ld + h, vv);
            }
        }
    }
    if (!active) return;
    if (qi < N) {
        float* drow = dq + (rowbase + qi) * (size_t)(H * 64) + (size_t)h * 64;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int d = 32 * dt + 8 * g4 + 4 * hi;
                *(float4*)(drow + d) = make_float4(scale * acc[dt][4 * g4], scale * acc[dt][4 * g4 + 1], scale * acc[dt][4 * g4 + 2], scale * acc[dt][4 * g4 + 3]);
            }
    }
    if (!LONG && dbias) {
        __builtin_amdgcn_s_waitcnt(0xc07f);                   // this wave's LDS updates are complete for its own reads
        if (dpart) {                                          // one row of the partial buffer (see attention.hip's dQ kernel): plain stores
            float* prow = dpart + (((size_t)b * H + h) * nqt + qt) * (size_t)(nqt * 32);
            for (int r = lane; r < nb; r += 64) prow[r] = dbw[r];
        } else
        for (int r = lane; r < min(nb, N); r += 64) {
            const float vv = dbw[r];
            if (vv != 0.f) unsafeAtomicAdd(dbias + (size_t)r * bias_ld + h, vv);
        }
        if (PFX && i0 < Pn)                                   // negative distances: only query tiles inside the prefix reach them
            for (int r = lane - off; r < 0; r += 64) {
                const float vv = dbw[r];
                if (vv != 0.f) unsafeAtomicAdd(dbias + (ptrdiff_t)r * bias_ld + h, vv);
            }
    }
}
