// The forward kernel of attention2.hip, included once per compiled form (the text is the kernel itself, so the short form compiles to exactly
// what it compiled to as a plain kernel):
//   A4_KERNEL attn4_fwd_kernel,      A4_LONG false: N <= 4096
//   A4_KERNEL attn4_fwd_long_kernel, A4_LONG true:  4096 < N <= A2_NL, causal -- the same walk and the same tile body; only the liveness
//   prologue differs: it covers the keys with a loop instead of 16 register slots, and livebits holds ceil(N / 64) ballot words, not 64.
//   LDS: the ring (60 KiB) + 136 ceil(N / 64) + 128 bytes -- two workgroups per CU (160 KiB) up to N = 9536, one above.
template <bool FIXED, bool DROP = false, bool PFX = false>
__global__ __launch_bounds__(A4_THREADS, 2) void A4_KERNEL(const h16_t* __restrict__ q, const h16_t* __restrict__ k,
                                                           const h16_t* __restrict__ v, const float* __restrict__ biasT, int ldT,
                                                           const unsigned char* __restrict__ keymask, h16_t* __restrict__ out,
                                                           float* __restrict__ lse, int B, int N, int H, float scale, const AttnDrop drop,
                                                           int Pn) {
    constexpr bool LONG = A4_LONG;
    // the flag of head 0: omlm_attn_bias_prepare decides once for all heads
    if ((biasT && __builtin_amdgcn_readfirstlane(__float_as_int(biasT[ldT - 2])) != 0) != FIXED) return;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* ring = smem;                                        // A2_NST stages
    h16_t* livef = (h16_t*)(smem + A2_NST * A2_STAGE);      // [nkt_all * 64] 1.0 / 0.0 per key of this sample
    const int nqt = (N + 31) / 32, ny = (H + 7) / 8;
    int b, qt, hy;
    a2_item_order(blockIdx.x, nqt, ny, B, b, qt, hy);
    const int lane = threadIdx.x & 63, hi = lane >> 5, ql = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h0 = hy * 8 + 2 * wave;                        // heads h0, h0 + 1
    const int i0 = qt * 32;
    const size_t rowbase = (size_t)b * N;
    const int off = PFX ? Pn - 1 : 0;
    const int kend = PFX && i0 < Pn ? max(i0 + 32, Pn) : i0 + 32;
    const int nkt = min((kend + A2_TKV - 1) / A2_TKV, (N + A2_TKV - 1) / A2_TKV);   // key tiles this query tile needs

    // ---- prologue: liveness of this sample's keys, as a 1/0 array of the operand type (denominator operand) and one ballot word per key
    // tile (V rows of masked keys are DMA'd as zeros).  All byte loads are issued before the first wait.
    unsigned long long* livebits = (unsigned long long*)(livef + (size_t)((N + 63) / 64) * 64);     // [64 tiles] (LONG: [ceil(N / 64)])
    unsigned* zeros = (unsigned*)(livebits + (LONG ? (N + 63) / 64 : 64));                        // 128 B of zeros (see a4_tile)
    if (LONG) {
        // passes of 2048 keys, a pass's eight byte loads in flight together; a wave's 64 keys are one tile, so its ballot is that tile's word
        const int nkeys = nkt * A2_TKV;
        for (int base = 0; base < nkeys; base += 8 * A4_THREADS) {
            unsigned char mk[8];
#pragma unroll
            for (int it = 0; it < 8; ++it) mk[it] = 1;
            if (keymask) {                                      // unconditional loads at clamped indices: all eight leave before the first wait
#pragma unroll
                for (int it = 0; it < 8; ++it) mk[it] = keymask[rowbase + min(base + it * A4_THREADS + (int)threadIdx.x, N - 1)];
            }
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int j = base + it * A4_THREADS + (int)threadIdx.x;
                if (base + it * A4_THREADS < nkeys) {           // uniform
                    const bool lv = j < N && mk[it] != 0;
                    const unsigned long long w = __ballot(lv);
                    if (j < nkeys) {                            // (uniform per wave: nkeys is a multiple of 64)
                        livef[j] = lv ? (h16_t)1.0f : (h16_t)0.0f;
                        if (lane == 0) livebits[j >> 6] = w;
                    }
                }
            }
        }
        if (threadIdx.x < 32) zeros[threadIdx.x] = 0u;
    } else {
        unsigned char mk[16];
#pragma unroll
        for (int it = 0; it < 16; ++it) mk[it] = 1;
        if (keymask) {
#pragma unroll
            for (int it = 0; it < 16; ++it)
                if (it * A4_THREADS < nkt * A2_TKV) mk[it] = keymask[rowbase + min(it * A4_THREADS + (int)threadIdx.x, N - 1)];   // uniform condition, clamped index
        }
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int j = it * A4_THREADS + threadIdx.x;
            if (it * A4_THREADS < nkt * A2_TKV) {               // uniform
                const bool lv = j < N && mk[it] != 0;
                const unsigned long long w = __ballot(lv);
                if (j < nkt * A2_TKV) livef[j] = lv ? (h16_t)1.0f : (h16_t)0.0f;
                if (lane == 0 && it * 4 + wave < nkt) livebits[it * 4 + wave] = w;
            }
        }
        if (threadIdx.x < 32) zeros[threadIdx.x] = 0u;
    }
    __syncthreads();                                          // livef / livebits visible; no LDS-DMA in flight yet
    const a2_rsrc rsK = a2_make_rsrc(k + rowbase * 64, (unsigned)N * 128u);
    const a2_rsrc rsV = a2_make_rsrc(v + rowbase * 64, (unsigned)N * 128u);
    const a2_rsrc rsB = a2_make_rsrc(biasT ? (const void*)(biasT + (size_t)hy * 8 * ldT) : (const void*)k, biasT ? (unsigned)(8 * ldT * 4) : 0u);
    const unsigned ring_lds = (unsigned)(size_t)LDS_PTR(char, ring);

    auto issue = [&](int t, int lane_) {                       // 5 DMA wave-instructions per wave per tile
        A4Stager stg;
        stg.init(wave, lane_, ldT);
        const unsigned st = ring_lds + (unsigned)((t % A2_NST) * A2_STAGE);
        const int j0 = t * A2_TKV;
        const unsigned long long lb = livebits[t];             // one broadcast LDS read per tile
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            a2_dma(rsK, st + (2 * wave + u) * 1024, (unsigned)(j0 * 128) + stg.koff[u]);           // rows >= N: beyond the descriptor -> zeros
            a2_dma(rsV, st + 8192 + (2 * wave + u) * 1024, ((lb >> stg.vrow[u]) & 1ull) ? (unsigned)(j0 * 128) + stg.voff[u] : OOB_OFF);
        }
        // bias window of this tile: table index PAD + rel, rel from i0 - j0 - 64 (no table: empty descriptor -> zeros)
        a2_dma(rsB, st + 16384 + wave * 1024, (unsigned)((A2_PAD + off + i0 - j0 - 64) * 4) + stg.boff);
    };

    issue(0, lane);
    if (nkt > 1) issue(1, lane);
    // Q fragments (B operand of S^T = K Q^T): query i0 + ql, dims 16 s + 8 hi .. +7, of the wave's two heads
    h16x8 qf[2][4];
    const int qi = i0 + ql;
#pragma unroll
    for (int hb = 0; hb < 2; ++hb) {
        const bool act = h0 + hb < H;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            u32x4 z = {0u, 0u, 0u, 0u};
            const h16_t* p = q + (rowbase + min(qi, N - 1)) * (size_t)(H * 64) + (size_t)(act ? h0 + hb : 0) * 64 + 16 * s + 8 * hi;
            u32x4 val = (act && qi < N) ? *(const u32x4*)p : z;
            qf[hb][s] = __builtin_bit_cast(h16x8, val);
        }
    }
    // Consume the Q loads HERE: hipcc then waits for them before the loop.  Left to their first use inside the loop, its
    // s_waitcnt vmcnt(0) sat in front of the first MFMA of every tile and drained the DMA ring each iteration (seen in the ISA).
#pragma unroll
    for (int hb = 0; hb < 2; ++hb)
#pragma unroll
        for (int s = 0; s < 4; ++s) asm volatile("" : "+v"(qf[hb][s]));

    A4Acc A;
#pragma unroll
    for (int hb = 0; hb < 2; ++hb) {
        A.m[hb] = A2_NEG;
#pragma unroll
        for (int e = 0; e < 16; ++e) { A.acc[hb][0][e] = 0.f; A.acc[hb][1][e] = 0.f; }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) A.accl[e] = 0.f;
    const float c = scale * A2_LOG2E;
    float mfix[2] = {0.f, 0.f};                              // fixed reference points of the two heads (table tails)
    if (FIXED) {
#pragma unroll
        for (int hb = 0; hb < 2; ++hb)
            mfix[hb] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(biasT[(size_t)(h0 + hb) * ldT + (ldT - 1)])));
    }
    asm volatile("" : "+s"(mfix[0]), "+s"(mfix[1]));          // loaded (and waited for) before the tile loop
    unsigned rk[2] = {0u, 0u};                               // DROP: row keys of (b, h0 + hb, qi), with this half-wave's key bit (4 hi) / 2
    if (DROP) {
        const unsigned long long sd = attn_drop_seed(drop);
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) rk[hb] = attn_drop_headkey(sd, b, h0 + hb) ^ ((unsigned)qi << 15) ^ (2u * (unsigned)hi);
    }

    for (int t = 0; t < nkt; ++t) {
        // own DMA of tile t retired (tile t+1's five may stay in flight), then everybody's; the barrier also says that all
        // waves are done with tile t-1, whose stage tile t+2 is about to overwrite
        if (t + 1 < nkt) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else             asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        int lane_ = lane;                                      // opaque per tile: every lane-derived address is rebuilt, none carried (see A4Stager)
        asm volatile("" : "+v"(lane_));
        if (t + 2 < nkt) issue(t + 2, lane_);
        const char* Ks = ring + (t % A2_NST) * A2_STAGE;
        const int j0 = t * A2_TKV;
        const bool full = j0 + A2_TKV - 1 <= i0;               // every block of the tile lies below the diagonal
        const h16_t* lv = livef + j0 + 4 * (lane_ >> 5);
        const h16_t* live0 = (lane_ & 1) == 0 ? lv : (const h16_t*)zeros;
        const h16_t* live1 = (lane_ & 1) == 1 ? lv : (const h16_t*)zeros;
        unsigned long long lbt = ~0ull;                         // online form: the running maximum is taken over live keys (a4_tile)
        if (!FIXED) {
            const unsigned long long lw = livebits[t];
            lbt = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(lw >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)lw);
        }
        if (FIXED) {
            if (full) a4_tile<true, true, -1, DROP, PFX>(A, qf, Ks, live0, live1, c, i0, j0, wave, lane_, rk, drop.thr16, kend, Pn);
            else      a4_tile<true, false, -1, DROP, PFX>(A, qf, Ks, live0, live1, c, i0, j0, wave, lane_, rk, drop.thr16, kend, Pn);
        } else if (full) {
            a4_tile<false, true, 0, DROP, PFX>(A, qf, Ks, live0, live1, c, i0, j0, wave, lane_, rk, drop.thr16, kend, Pn, lbt);
            __builtin_amdgcn_sched_barrier(0);
            a4_tile<false, true, 1, DROP, PFX>(A, qf, Ks, live0, live1, c, i0, j0, wave, lane_, rk, drop.thr16, kend, Pn, lbt);
        } else {
            a4_tile<false, false, 0, DROP, PFX>(A, qf, Ks, live0, live1, c, i0, j0, wave, lane_, rk, drop.thr16, kend, Pn, lbt);
            __builtin_amdgcn_sched_barrier(0);
            a4_tile<false, false, 1, DROP, PFX>(A, qf, Ks, live0, live1, c, i0, j0, wave, lane_, rk, drop.thr16, kend, Pn, lbt);
        }
    }
    if (qi >= N) return;
#pragma unroll
    for (int hb = 0; hb < 2; ++hb) {
        const int h = h0 + hb;
        if (h >= H) continue;
        const float lsum = A.accl[hb];                  // element e = hb: row crow(hb, hi) has parity hb
        const float mref = FIXED ? mfix[hb] : A.m[hb];
        // a query without any live causal key has no defined softmax: emit zeros and an lse that zeroes its backward
        const float inv = lsum > 0.f ? (DROP ? drop.rs : 1.0f) / lsum : 0.f;
        h16_t* orow = out + (rowbase + qi) * (size_t)(H * 64) + (size_t)h * 64;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int d = 32 * dt + 8 * g4 + 4 * hi;
                store4_from_float(orow + d, A.acc[hb][dt][4 * g4] * inv, A.acc[hb][dt][4 * g4 + 1] * inv,
                                  A.acc[hb][dt][4 * g4 + 2] * inv, A.acc[hb][dt][4 * g4 + 3] * inv);
            }
        if (hi == 0 && lse) lse[((size_t)b * H + h) * N + qi] = lsum > 0.f ? mref + log2f(lsum) : 1.0e30f;   // log2 domain
    }
}
