// Per-row diagnostics of the cross entropy (include/omlm.h: omlm_ce_metrics, omlm_ce_metrics_bins): a second, read-only pass over the fp32
// logits rows [R, ld] the loss has just walked.  Per live row: nll = lse - l[y], the exact integer rank of the label and the predictive
// entropy; a second launch bins them per quantizer in a fixed order.  Nothing here writes what the loss or its backward read, and
// csrc/embed_ce.hip is not touched: these kernels live in a translation unit of their own.
//
// lse is formed the way ce_fwd_wave_kernel / ce_fwd_kernel (csrc/embed_ce.hip) form it -- maximum, __expf, __logf, the same per-lane order
// and the same reductions -- so that it equals their row_lse bit for bit on the same row.  The entropy rides on the same pass:
// H = log s - (sum_c e_c d_c) / s with d_c = l[c] - max, e_c = exp(d_c), s = sum_c e_c; a column with e_c == 0 (a -inf logit, the slots past V)
// adds exactly 0, never 0 * inf.  The rank is integer counts only.
#include "common.h"
#include "ce_metrics_plan.h"

// One WAVE per row, V <= 64 * CE_METRICS_NV: the row sits in registers (element c = lane + 64 j).  Every load is unconditional on a clamped
// index and consumed together (predicated loads were serialised by hipcc, one wait each: csrc/embed_ce.hip); no LDS, no barrier.
__global__ __launch_bounds__(256) void ce_metrics_wave_kernel(const float* __restrict__ logits, const int* __restrict__ labels,
                                                              float* __restrict__ row_nll, int* __restrict__ row_rank,
                                                              float* __restrict__ row_entropy, int R, int V, int ld, int* __restrict__ err) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int row = blockIdx.x * 4 + wave; row < R; row += gridDim.x * 4) {
        const float* lr = logits + (size_t)row * ld;
        float v[CE_METRICS_NV];
#pragma unroll
        for (int j = 0; j < CE_METRICS_NV; ++j) { const int c = lane + 64 * j; v[j] = lr[c < V ? c : V - 1]; }
        const int lb = labels[row];
        const bool live = lb >= 0 && lb < V;
        const float own = lr[live ? lb : 0];
#pragma unroll
        for (int j = 0; j < CE_METRICS_NV; ++j) asm volatile("" : "+v"(v[j]));
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < CE_METRICS_NV; ++j) { if (lane + 64 * j >= V) v[j] = -INFINITY; mx = fmaxf(mx, v[j]); }
        mx = wave_max(mx);
        float s = 0.f, ed = 0.f;
        int cnt = 0;                                                     // wave-uniform: entries ahead of the label
#pragma unroll
        for (int j = 0; j < CE_METRICS_NV; ++j) {
            const float d = v[j] - mx, e = __expf(d);
            s += e;                                                      // (exp(-inf) = 0 for the slots past V)
            ed += e > 0.f ? e * d : 0.f;
            const int c = lane + 64 * j;
            cnt += __popcll(__ballot(c < V && (v[j] > own || (v[j] == own && c < lb))));
        }
        s = wave_sum(s);
        ed = wave_sum(ed);
        const float lse = mx + __logf(s);
        if (lane == 0) {
            if (lb >= V && err) atomicOr(err, 4);                        // a label past the vocabulary: row ignored, flag raised
            if (row_nll) row_nll[row] = live ? lse - own : 0.f;
            if (row_rank) row_rank[row] = live ? cnt : -1;
            if (row_entropy) row_entropy[row] = live ? __logf(s) - ed / s : 0.f;
        }
    }
}

__device__ __forceinline__ int block_sum_int256(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// One WORKGROUP per row, any V: the passes of ce_fwd_kernel (maximum, then the sums) with the entropy sum and the rank count on the second.
__global__ __launch_bounds__(256) void ce_metrics_block_kernel(const float* __restrict__ logits, const int* __restrict__ labels,
                                                               float* __restrict__ row_nll, int* __restrict__ row_rank,
                                                               float* __restrict__ row_entropy, int R, int V, int ld, int* __restrict__ err) {
    __shared__ float red[4];
    __shared__ int redi[4];
    for (int row = blockIdx.x; row < R; row += gridDim.x) {
        const float* lr = logits + (size_t)row * ld;
        float mx = -INFINITY;
        for (int c = threadIdx.x; c < V; c += 256) mx = fmaxf(mx, lr[c]);
        mx = wave_max(mx);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        const int lb = labels[row];
        const bool live = lb >= 0 && lb < V;
        const float own = lr[live ? lb : 0];
        float s = 0.f, ed = 0.f;
        int cnt = 0;
        for (int c = threadIdx.x; c < V; c += 256) {
            const float x = lr[c];
            const float d = x - mx;
            const float e = __expf(d);
            s += e;
            ed += e > 0.f ? e * d : 0.f;
            cnt += (x > own || (x == own && c < lb)) ? 1 : 0;
        }
        s = block_sum<256>(s, red);
        ed = block_sum<256>(ed, red);
        cnt = block_sum_int256(cnt, redi);
        const float lse = mx + __logf(s);
        if (threadIdx.x == 0) {
            if (lb >= V && err) atomicOr(err, 4);
            if (row_nll) row_nll[row] = live ? lse - own : 0.f;
            if (row_rank) row_rank[row] = live ? cnt : -1;
            if (row_entropy) row_entropy[row] = live ? __logf(s) - ed / s : 0.f;
        }
    }
}

// One WORKGROUP per bin, fp64, a fixed order: thread t adds its rows t, t + 1024, ... in ascending order, a wave folds its 64 lanes by the
// xor ladder, and thread i < 5 adds the 16 wave sums of quantity i in wave order onto bins[bin][i].  The same input gives the same bits on
// every launch, and the counts are exact (integers far below 2^53).  Rows are in [B, n] order, t = r mod n; the bin of a live row is Q where
// its label is the eos entry V - 1, t mod Q otherwise.
__global__ __launch_bounds__(CE_METRICS_BIN_THREADS) void ce_metrics_bins_kernel(const float* __restrict__ row_nll, const int* __restrict__ row_rank,
                                                                                 const float* __restrict__ row_entropy, const int* __restrict__ labels,
                                                                                 int R, int n, int Q, int V, int k_top, double* __restrict__ bins) {
    const int bin = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = threadIdx.x; r < R; r += CE_METRICS_BIN_THREADS) {
        const int y = labels[r];
        if (y < 0 || y >= V) continue;
        if ((y == V - 1 ? Q : (r % n) % Q) != bin) continue;
        const int rank = row_rank[r];
        a[0] += 1.0;
        a[1] += (double)row_nll[r];
        a[2] += (double)row_entropy[r];
        a[3] += rank == 0 ? 1.0 : 0.0;
        a[4] += rank < k_top ? 1.0 : 0.0;
    }
    __shared__ double red[CE_METRICS_BIN_THREADS / 64][5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a[i] += __shfl_xor(a[i], o, 64);
        if (lane == 0) red[wave][i] = a[i];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        double t = 0.0;
        for (int w = 0; w < CE_METRICS_BIN_THREADS / 64; ++w) t += red[w][threadIdx.x];
        bins[(size_t)bin * 5 + threadIdx.x] += t;
    }
}

// logits [R, ld] fp32 (columns [V, ld) never read), labels [R]; row_nll / row_rank / row_entropy [R], any of them null (not wanted).
extern "C" int omlm_ce_metrics(const float* logits, const int* labels, float* row_nll, int* row_rank, float* row_entropy,
                               int R, int V, int ld, int* err_flag, void* stream) {
    if (const char* why = ce_metrics_refusal(R, V, ld)) { omlm_set_error(why); return OMLM_ERR_ARG; }
    if (R == 0) return OMLM_OK;
    OMLM_CHECK_ARG(logits && labels, "ce_metrics: null pointer (logits, labels)");
    const dim3 grid((unsigned)ce_metrics_grid(R, V)), block(256);
    if (ce_metrics_route(V) == CE_METRICS_WAVE)
        hipLaunchKernelGGL(ce_metrics_wave_kernel, grid, block, 0, as_stream(stream), logits, labels, row_nll, row_rank, row_entropy, R, V, ld, err_flag);
    else
        hipLaunchKernelGGL(ce_metrics_block_kernel, grid, block, 0, as_stream(stream), logits, labels, row_nll, row_rank, row_entropy, R, V, ld, err_flag);
    return omlm_post_launch("omlm_ce_metrics");
}

// bins [Q + 1][5] doubles {count, nll, entropy, top1, topk}, ACCUMULATED onto.
extern "C" int omlm_ce_metrics_bins(const float* row_nll, const int* row_rank, const float* row_entropy, const int* labels,
                                    int R, int n, int Q, int V, int k_top, double* bins, void* stream) {
    if (const char* why = ce_metrics_bins_refusal(R, n, Q, V, k_top)) { omlm_set_error(why); return OMLM_ERR_ARG; }
    if (R == 0) return OMLM_OK;
    OMLM_CHECK_ARG(row_nll && row_rank && row_entropy && labels && bins, "ce_metrics_bins: null pointer");
    hipLaunchKernelGGL(ce_metrics_bins_kernel, dim3((unsigned)(Q + 1)), dim3(CE_METRICS_BIN_THREADS), 0, as_stream(stream),
                       row_nll, row_rank, row_entropy, labels, R, n, Q, V, k_top, bins);
    return omlm_post_launch("omlm_ce_metrics_bins");
}
