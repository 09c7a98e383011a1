// The squared-difference nearest-codeword arithmetic (FORM_SQ of optim_misc.hip), shared by omlm_nearest_centroid (rvq_kernel<FORM_SQ>)
// and the k-means fit (kmeans_fit.hip), so that both files compile the same code: fp32, every multiply and add rounded separately (no
// FMA contraction), d in index order; argmin with ties -> lowest index.
#pragma once
#include "common.h"

// Thread t of a 256-thread workgroup walks the codes c = t, t + 256, ... for R rows at once (r: [R][D] in LDS, cb: the codebook
// TRANSPOSED [D][C], consecutive threads read consecutive addresses).  Per (row, code) the operation sequence does not depend on R,
// so R = 1 and R = 4 return the same bits.  best / besti start at INFINITY / 0x7fffffff.
template <int R>
__device__ __forceinline__ void sq_nearest_thread_rows(const float* r, const float* __restrict__ cb, int D, int C, float (&best)[R],
                                                       int (&besti)[R]) {
    for (int c = threadIdx.x; c < C; c += 256) {
        float dist[R];
#pragma unroll
        for (int j = 0; j < R; ++j) dist[j] = 0.f;
        for (int d = 0; d < D; ++d) {
            const float e = cb[(size_t)d * C + c];
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const float diff = __fsub_rn(r[j * D + d], e);
                dist[j] = __fadd_rn(dist[j], __fmul_rn(diff, diff));
            }
        }
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (dist[j] < best[j]) { best[j] = dist[j]; besti[j] = c; }      // ascending c per thread: strict < keeps the lowest index
    }
}

// lexicographic (dist, index) min over the 64 lanes of a wave; every lane ends with the result
__device__ __forceinline__ void wave_lexmin(float& best, int& besti) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float od = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(besti, o, 64);
        if (od < best || (od == best && oi < besti)) { best = od; besti = oi; }
    }
}

// the same min over the four per-wave results of a 256-thread workgroup (one thread)
__device__ __forceinline__ void lexmin4(const float* bd, const int* bi, float& b, int& i0) {
    b = bd[0];
    i0 = bi[0];
    for (int w = 1; w < 4; ++w)
        if (bd[w] < b || (bd[w] == b && bi[w] < i0)) { b = bd[w]; i0 = bi[w]; }
}
