// The dK / dV kernel of attention3.hip, included once per compiled form (the text is the kernel itself, so the atomics form compiles to
// exactly what it compiled to as a plain kernel):
//   A3_KERNEL attn3_bwd_dkv_kernel,      A3_PART false, A3_PART_ARG empty,                        A3_PART_PTR a null pointer
//   A3_KERNEL attn3_bwd_dkv_part_kernel, A3_PART true,  A3_PART_ARG `, float* __restrict__ part`, A3_PART_PTR part
// PART (N > 4096 with a workspace): the workgroup leaves its [2][128 keys][64] fp32 sums in slot `lg` of `part`
// with plain stores instead of adding them to dK / dV; a3_part_reduce_kernel sums a key range's slots in ascending chunk order.  At long N a
// range has dozens of chunks, and fp32 atomics in order of arrival would make dK / dV differ from run to run.
template <bool DROP = false, bool PFX = false>
__global__ __launch_bounds__(A3_T) __attribute__((amdgpu_waves_per_eu(A3_WAVES)))
void A3_KERNEL(const h16_t* __restrict__ q, const h16_t* __restrict__ k, const h16_t* __restrict__ v,
               const unsigned char* __restrict__ keymask, const h16_t* __restrict__ dout,
               const float* __restrict__ lse, const float* __restrict__ delta, float* __restrict__ dk, float* __restrict__ dv,
               const float* __restrict__ biasT, int ldT, int B, int N, int H, float scale, int CH, int wg_per_sample,
               const AttnDrop drop, int Pn A3_PART_ARG) {
    constexpr bool PART = A3_PART;
    extern __shared__ __attribute__((aligned(16))) char smem3[];
    const int lane = threadIdx.x & 63, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nqt = (N + 31) / 32;
    // XCD-aware: the workgroups of one sample share its Q / dO tiles through an XCD's L2 (workgroup i runs on XCD i % 8); dealt in launch
    // order every XCD fetched every sample's Q and dO
    int lg = blockIdx.x;
    {
        const int total = B * wg_per_sample, lin = blockIdx.x;
        const int qq = total >> 3, rr = total & 7, xcd = lin & 7, idx = lin >> 3;
        lg = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + idx;
    }
    const int b = lg / wg_per_sample;
    int rem = lg - b * wg_per_sample, r = 0, chunk = 0;
    for (;; ++r) {                                            // uniform scalar scan: which key range this workgroup belongs to
        const int nch = (nqt - (PFX ? a3_range_start(r, Pn) : 4 * r) + CH - 1) / CH;
        if (rem < nch) { chunk = rem; break; }
        rem -= nch;
    }
    const int it0 = (PFX ? a3_range_start(r, Pn) : 4 * r) + chunk * CH, it1 = min(nqt, it0 + CH);
    const int off = PFX ? Pn - 1 : 0;
    const int nitems = (it1 - it0) * H;
    const int j0w = r * A3_KR + 32 * wave;                    // this wave's 32 keys
    const int jtw = 4 * r + wave;                             // ... as a 32-key tile index
    const int kj = j0w + (lane & 31);
    const size_t rowbase = (size_t)b * N;
    const float c = scale * A3_LOG2E;
    const bool has_bias = biasT != nullptr;
    // DROP: this lane holds key kj of 16 query rows; the draw of (i, kj) is the (kj & 1) half of omlm_hash32(row key ^ (kj >> 1)), taken
    // as the upper half of (word << dsh) (see AttnDrop); dseed: the salted seed, hashed into a head key once per item
    const unsigned long long dseed = DROP ? attn_drop_seed(drop) : 0ull;
    const unsigned dsh = (kj & 1) ? 0u : 16u;

    // K^T, V^T B-operands: lane n = key kj, dims 16 s + 8 hi .. +7 -- resident for the whole kernel
    h16x8 kf[4], vf[4];
    {
        const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const size_t off = (rowbase + min(kj, N - 1)) * 64 + 16 * s + 8 * hi;
            kf[s] = __builtin_bit_cast(h16x8, kj < N ? *(const u32x4*)(k + off) : z);
            vf[s] = __builtin_bit_cast(h16x8, kj < N ? *(const u32x4*)(v + off) : z);
        }
    }
    const bool keylive = kj < N && (keymask ? keymask[rowbase + min(kj, N - 1)] != 0 : true);
    // consumed here, so that hipcc's own waits for these loads sit in front of the loop and not inside it (they would drain the DMA ring)
#pragma unroll
    for (int s = 0; s < 4; ++s) asm volatile("" : "+v"(kf[s]), "+v"(vf[s]));

    // per-lane source coordinates of the unit this wave stages (unit = wave): row rowu, first column colu of the blocked image
    const int pp_ = lane >> 3, rq_ = ((pp_ >> 2) << 1) | ((pp_ >> 1) & 1);
    const int rowu = (wave >> 1) * 16 + rq_ * 4 + ((lane >> 1) & 3);
    const int colu = (wave & 1) * 32 + (pp_ & 1) * 16 + (lane & 1) * 8;
    const unsigned ring_lds = (unsigned)(size_t)LDS_PTR(char, smem3);

    // (it, h) of an item advance as counters, and so do the per-lane source offsets of its four DMA pieces: byte offsets from the tensor
    // bases (32 bits: the launch checks the extents), bumped by a constant per head and rebuilt once per query tile -- item / H, item % H
    // and the 64-bit address products were ~130 scalar + ~25 vector instructions per item (SQ_INSTS_SALU 2.1e7 in the counters).
    unsigned qoff = 0, boff = 0;                              // Q / dO piece; bias window piece (lanes 0-15) | table tail (the others)
    const float* ldp = lse;                                   // lse (lanes 0-31) | delta (lanes 32-63) element of the item
    const unsigned bstep = (unsigned)ldT * 4u;
    auto tile_offsets = [&](int it) {                         // head 0 of query tile `it`
        const int qi = min(32 * it + rowu, N - 1);            // rows past N: clamped (their scores are masked below)
        qoff = (unsigned)((((int)rowbase + qi) * H) * 64 + colu) * 2u;
        // lanes 0-15: the bias window for this wave's keys, table index A3_PAD + rel - 1 from rel = 32 (it - jtw) - 31 (one entry early:
        // 16-byte aligned); lane 16: the row's tail [.., flag, m_h]; the other lanes repeat lane 16's address
        const int w0 = max(A3_PAD + off + 32 * (it - jtw) - 32, 0);
        boff = has_bias ? (unsigned)(lane < 16 ? w0 + 4 * lane : ldT - 4) * 4u : 0u;
        ldp = (hi ? delta : lse) + ((size_t)b * H * N + min(32 * it + (lane & 31), N - 1));
    };
    auto issue = [&](int stage) {                             // 4 DMA wave-instructions per wave per item, then on to the next head
        const unsigned st = ring_lds + (unsigned)(stage * A3_STAGE);
        a3_dma16s(q, qoff, st + wave * 1024 + (wave >> 1) * 128);
        a3_dma16s(dout, qoff, st + A3_IMG + wave * 1024 + (wave >> 1) * 128);
        const unsigned ax = st + 2 * A3_IMG + wave * A3_AUX;
        a3_dma16s(has_bias ? (const void*)biasT : (const void*)lse, boff, ax);
        a3_dma4(ldp, ax + 1024);
        qoff += 128u; boff += has_bias ? bstep : 0u; ldp += N;
    };

    f32x16 dkacc[2], dvacc[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) { dkacc[0][e] = 0.f; dkacc[1][e] = 0.f; dvacc[0][e] = 0.f; dvacc[1][e] = 0.f; }

    int it_i = it0, h_i = 0, st_i = 0;                        // the next item to be issued
    tile_offsets(it0);
    auto issue_next = [&]() {
        issue(st_i);
        if (++h_i == H) { h_i = 0; ++it_i; tile_offsets(it_i); }
        if (++st_i == A3_NST) st_i = 0;
    };
    if (nitems > 0) issue_next();
    if (nitems > 1) issue_next();
    int it = it0, hcur = 0, stage = 0;                        // the item being multiplied
    for (int item = 0; item < nitems; ++item, (++hcur == H ? (hcur = 0, ++it) : 0), (++stage == A3_NST ? (stage = 0) : 0)) {
        // own pieces of `item` landed (the next item's four may stay in flight), then everybody's; the barrier also says that all
        // waves are done with item - 1, whose stage item + 2 is about to overwrite
        if (item + 1 < nitems) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else                   asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (item + 2 < nitems) issue_next();
        const int i0 = 32 * it;
        if (i0 + 31 < j0w && !(PFX && i0 < Pn && j0w < Pn)) continue;      // every query of the tile precedes every key of this wave (causal): nothing to do
        const char* Qs = smem3 + stage * A3_STAGE;
        const char* dOs = Qs + A3_IMG;
        const float* axa = (const float*)(Qs + 2 * A3_IMG + wave * A3_AUX);
        const float* axb = axa + 256;                         // lse[32] | delta[32]
        const float mh = has_bias ? axa[64 + 3] : 0.f;        // the head's reference point (table tail), 0 without a fixed one
        // window index of (query row crow(r, hi), this lane's key): rel - (32 (it - jtw) - 31) + 1 = cr + 4 hi - (lane & 31) + 32
        const float* bwp = axa + 32 + 4 * hi - (lane & 31);
        const float* lp = axb + 4 * hi;
        f32x16 st, dp;
#pragma unroll
        for (int e = 0; e < 16; ++e) { st[e] = 0.f; dp[e] = 0.f; }
        {
            h16x8 qa[4], doa[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) { qa[s] = a3_frag_rows(Qs, s, lane); doa[s] = a3_frag_rows(dOs, s, lane); }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                st = OMLM_MFMA_32x32x16(qa[s], kf[s], st);    // S  = Q K^T   (rows i, column = this lane's key)
                dp = OMLM_MFMA_32x32x16(doa[s], vf[s], dp);   // dP = dO V^T
            }
        }
        f32x16 pr;
        float bvv[16], lvv[16], dvv[16];
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int cr = (rr & 3) + 8 * (rr >> 2);          // crow(rr, hi) - 4 hi
            bvv[rr] = bwp[cr];                                // (no bias: overwritten below -- one branch, not one per element)
            lvv[rr] = lp[cr];
            dvv[rr] = lp[32 + cr];
        }
        if (!has_bias) {
            float z = 0.f;
            asm volatile("" : "+v"(z));                       // (defined inside the branch: otherwise 16 selects on every item)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) bvv[rr] = z;
        }
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) asm volatile("" : "+v"(bvv[rr]), "+v"(lvv[rr]), "+v"(dvv[rr]));
        // Element arithmetic on register pairs (v_pk_add_f32 / v_pk_fma_f32 / v_pk_mul_f32).  A dead key (this lane's column) leaves through
        // the reference point: mhk = m_h - 1e30 there, so x = c S + bias - (lse - mhk) = -1e30 and P = 0 without a select; dS carries no
        // softmax scale here -- dK = scale dS^T Q takes it once, at the final store.
        const float mhk = keylive ? mh : mh + A3_NEG;
        if (!(i0 >= j0w + 31 && i0 + 31 < N)) {               // the tile touches the diagonal or runs past N: those rows leave through the bias term
            int kjv = kj;
            asm volatile("" : "+v"(kjv));                     // (defined inside the branch: hipcc otherwise hoists the 16 selects in front of it)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int i = i0 + a3_crow(rr, hi);
                bvv[rr] = ((i >= kjv || (PFX && i < Pn && kjv < Pn)) && i < N) ? bvv[rr] : A3_NEG;
            }
        }
        // DROP: the lane's key part of the row keys, rows i0 + 4 hi + cr (cr = crow(rr, hi) - 4 hi: bits disjoint from i0 and 4 hi)
        const unsigned lk = DROP ? attn_drop_headkey(dseed, b, hcur) ^ ((unsigned)kj >> 1) ^ ((unsigned)(i0 + 4 * hi) << 15) : 0u;
#pragma unroll
        for (int rr = 0; rr < 16; rr += 2) {
            const f32x2 t2 = f32x2{bvv[rr], bvv[rr + 1]} - (f32x2{lvv[rr], lvv[rr + 1]} - f32x2{mhk, mhk});
            const f32x2 x2 = __builtin_elementwise_fma(f32x2{st[rr], st[rr + 1]}, f32x2{c, c}, t2);
            const f32x2 p2 = {__builtin_amdgcn_exp2f(x2[0]), __builtin_amdgcn_exp2f(x2[1])};
            f32x2 dp2 = {dp[rr], dp[rr + 1]}, z2 = {1.f, 1.f};
            if (DROP) {                                       // Z / (1 - p) of (rows cr, cr + 1; key kj): dV takes P Z / (1 - p), dS = P (Z dP~ / (1 - p) - delta)
                const int cr = (rr & 3) + 8 * (rr >> 2);
                const unsigned w0 = omlm_hash32(lk ^ ((unsigned)cr << 15)), w1 = omlm_hash32(lk ^ ((unsigned)(cr + 1) << 15));
                z2 = f32x2{(w0 << dsh) >= drop.thr16 ? drop.rs : 0.f, (w1 << dsh) >= drop.thr16 ? drop.rs : 0.f};
                dp2 = dp2 * z2;
            }
            const f32x2 ds2 = p2 * (dp2 - f32x2{dvv[rr], dvv[rr + 1]});
            const f32x2 pz2 = DROP ? p2 * z2 : p2;
            pr[rr] = pz2[0]; pr[rr + 1] = pz2[1];
            st[rr] = ds2[0]; st[rr + 1] = ds2[1];
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const h16x8 pb = a3_pack(pr, s), dsb = a3_pack(st, s);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                dvacc[dt] = OMLM_MFMA_32x32x16(a3_frag_cols_tr(dOs, s, 32 * dt, lane), pb, dvacc[dt]);    // dV^T += dO^T P
                dkacc[dt] = OMLM_MFMA_32x32x16(a3_frag_cols_tr(Qs, s, 32 * dt, lane), dsb, dkacc[dt]);    // dK^T += Q^T dS
            }
        }
    }
    // ---- this wave's 32 keys x 64 dims of dK and dV: transposed through LDS (pitch 33: conflict-free both ways) and added row by row ----
    __syncthreads();                                          // every wave is past its last reads of the ring
    float* red = (float*)smem3 + (size_t)wave * (64 * 33);
    for (int which = 0; which < 2; ++which) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int d = 32 * dt + a3_crow(rr, hi);
                red[d * 33 + (lane & 31)] = which == 0 ? scale * dkacc[dt][rr] : dvacc[dt][rr];
            }
        __builtin_amdgcn_s_waitcnt(0xc07f);                   // this wave's own LDS writes, then its own reads below
        float* dst = which == 0 ? dk : dv;
        if (PART) {
            float* slot = A3_PART_PTR + ((size_t)lg * 2 + which) * (A3_KR * 64) + (size_t)(32 * wave) * 64;
            for (int e = lane; e < 32 * 64; e += 64) slot[e] = red[(e & 63) * 33 + (e >> 6)];
        } else
        for (int e = lane; e < 32 * 64; e += 64) {
            const int j = e >> 6, d = e & 63;                 // consecutive lanes -> consecutive d (coalesced 256-byte rows)
            const float val = red[d * 33 + j];
            if (j0w + j < N && val != 0.f) unsafeAtomicAdd(dst + (rowbase + j0w + j) * 64 + d, val);
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
    }
}
