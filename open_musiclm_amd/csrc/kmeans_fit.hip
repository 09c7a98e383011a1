// Fitting the semantic k-means codebook on the device (reference: hf_hubert_kmeans.py:95-149, sklearn's MiniBatchKMeans on the host;
// here the published MiniBatchKMeans rules with the package's own random stream -- open_musiclm_amd/kmeans_fit.py drives these):
//
//   seeding      greedy k-means++ on a subset of m rows: per pick, `trials` candidates drawn proportionally to the current closest
//                squared distance, the candidate with the lowest resulting potential wins (omlm_kmeans_pp_pick / _seed)
//   mini-batch   gather-by-index assign (the arithmetic of omlm_nearest_centroid, vq_nearest.h) + counts / sums + batch inertia +
//                the running-mean update and sklearn's two stopping rules, state kept on the device (omlm_kmeans_minibatch_step)
//   inertia      sum over rows of the min squared distance, fp64 accumulator (omlm_kmeans_inertia)
//
// All fp32 data; every sum that decides something (cumulative weights, potentials, inertias) is formed in fp64 in a fixed order.
#include "common.h"
#include "vq_nearest.h"

#define KM_MAX_TRIALS 16
#define KM_PP_MAXG 1024          // workgroups of the distance pass = rows of the partial-potential table
#define KM_ROWS 4                // rows per workgroup pass of the assign kernel

// ---- k-means++ ------------------------------------------------------------------------------------------------------------------
// workspace: header | partial potentials [KM_MAX_TRIALS][KM_PP_MAXG] fp64 | dmin [TT][m] fp32 (min(closest_i, d(i, candidate t)))
struct KmPPHeader {
    int cand[KM_MAX_TRIALS];     // this pick's candidate rows
    int k;                       // the pick being made (copied from the device counter by the first kernel of the pick)
    int pad[15];
};
static inline int km_tt(int trials) { return trials <= 4 ? 4 : trials <= 8 ? 8 : 16; }
static inline size_t km_pp_dmin_offset() { return sizeof(KmPPHeader) + sizeof(double) * KM_MAX_TRIALS * KM_PP_MAXG; }
static inline int km_pp_rows_per_wave(int TT) { return TT <= 8 ? 4 : 2; }
static inline int km_pp_grid(int m, int TT) {
    const int per = 4 * km_pp_rows_per_wave(TT);
    const int g = (m + per - 1) / per;
    return g < KM_PP_MAXG ? g : KM_PP_MAXG;
}

// One workgroup of 1024 threads: the candidates of pick k.  k = 0: the first centre is row min(floor(u[0] * m), m - 1) and `closest`
// becomes +inf.  k > 0: inverse CDF over `closest`: cum_i = sum_{j <= i} closest_j in fp64 (thread-contiguous chunks, chunk sums
// combined by a fixed-order scan), r_t = (double)u_t * cum_{m-1}, candidate t = the FIRST row i with cum_i > r_t, i.e.
// #{i : cum_i <= r_t}, clipped to m - 1.  Rows of weight zero (equal cumulative values) are never drawn: the strict comparison skips
// them to the first row that adds weight.
__global__ __launch_bounds__(1024) void km_pp_select_kernel(float* __restrict__ closest, const float* __restrict__ uniforms,
                                                            const int* __restrict__ counter, KmPPHeader* __restrict__ hdr, int m, int K,
                                                            int trials, int TT) {
    __shared__ double sh[1024];
    __shared__ int cnts[KM_MAX_TRIALS];
    const int tid = threadIdx.x;
    const int k = counter[0];
    if (tid == 0) hdr->k = k;
    if (k < 0 || k >= K) return;
    if (k == 0) {
        int c = (int)((double)uniforms[0] * (double)m);
        c = c < 0 ? 0 : (c > m - 1 ? m - 1 : c);
        if (tid < KM_MAX_TRIALS) hdr->cand[tid] = c;
        for (int i = tid; i < m; i += 1024) closest[i] = INFINITY;
        return;
    }
    const int L = (m + 1023) / 1024;
    const int lo = min(tid * L, m), hi = min(lo + L, m);
    double s = 0.0;
    for (int i = lo; i < hi; ++i) s += (double)closest[i];
    sh[tid] = s;
    if (tid < KM_MAX_TRIALS) cnts[tid] = 0;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {       // inclusive scan of the chunk sums
        const double v = tid >= off ? sh[tid - off] : 0.0;
        __syncthreads();
        sh[tid] += v;
        __syncthreads();
    }
    const double total = sh[1023];
    double cum = tid > 0 ? sh[tid - 1] : 0.0;
    double r[KM_MAX_TRIALS];
    int cnt[KM_MAX_TRIALS];
#pragma unroll
    for (int t = 0; t < KM_MAX_TRIALS; ++t) {
        r[t] = t < trials ? (double)uniforms[(size_t)k * trials + t] * total : -1.0;
        cnt[t] = 0;
    }
    for (int i = lo; i < hi; ++i) {
        cum += (double)closest[i];
#pragma unroll
        for (int t = 0; t < KM_MAX_TRIALS; ++t) cnt[t] += cum <= r[t] ? 1 : 0;
    }
#pragma unroll
    for (int t = 0; t < KM_MAX_TRIALS; ++t)
        if (t < trials && cnt[t]) atomicAdd(&cnts[t], cnt[t]);           // integer LDS adds: order-free
    __syncthreads();
    if (tid < KM_MAX_TRIALS) {
        const int c = cnts[tid < trials ? tid : 0];                     // the unused slots of the TT-wide pass repeat candidate 0
        hdr->cand[tid] = c > m - 1 ? m - 1 : c;
    }
}

// Distance pass: every row against the TT candidates (candidates in LDS, one wave per R rows, the lanes split d), dmin[t][i] =
// min(closest_i, |x_i - x_cand_t|^2) and the per-workgroup partial potentials sum_i dmin[t][i] in fp64.  Rows go to waves by a fixed
// stride and the partials are combined in index order (km_pp_final_kernel), so a pick is bit-reproducible.
template <int TT, int R, int VEC>
__global__ __launch_bounds__(256) void km_pp_dist_kernel(const float* __restrict__ x, const float* __restrict__ closest,
                                                         const KmPPHeader* __restrict__ hdr, float* __restrict__ dmin,
                                                         double* __restrict__ partials, int m, int D, int K) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* cs = (float*)smem;                                            // [TT][D]
    double* wp = (double*)(smem + (((size_t)TT * D * sizeof(float) + 15) & ~(size_t)15));      // [4][TT]
    const int k = hdr->k;
    if (k < 0 || k >= K) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int t = 0; t < TT; ++t) {
        const int c = hdr->cand[t];
        for (int d = tid; d < D; d += 256) cs[t * D + d] = x[(size_t)c * D + d];
    }
    __syncthreads();
    double pot[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) pot[t] = 0.0;
    const int nw = gridDim.x * 4;
    for (int row0 = (blockIdx.x * 4 + w) * R; row0 < m; row0 += nw * R) {
        float acc[R][TT];
#pragma unroll
        for (int j = 0; j < R; ++j)
#pragma unroll
            for (int t = 0; t < TT; ++t) acc[j][t] = 0.f;
        const float* xr[R];
#pragma unroll
        for (int j = 0; j < R; ++j) xr[j] = x + (size_t)min(row0 + j, m - 1) * D;      // rows past the end re-read the last row, unused
        for (int d = lane * VEC; d < D; d += 64 * VEC) {
            float xv[R][VEC];
#pragma unroll
            for (int j = 0; j < R; ++j) {
                if (VEC == 4) {
                    const f32x4 v = *(const f32x4*)(xr[j] + d);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) xv[j][e] = v[e];
                } else {
                    xv[j][0] = xr[j][d];
                }
            }
#pragma unroll
            for (int t = 0; t < TT; ++t) {
                float cv[VEC];
                if (VEC == 4) {
                    const f32x4 v = *(const f32x4*)(cs + t * D + d);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) cv[e] = v[e];
                } else {
                    cv[0] = cs[t * D + d];
                }
#pragma unroll
                for (int j = 0; j < R; ++j)
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const float diff = xv[j][e] - cv[e];
                        acc[j][t] += diff * diff;
                    }
            }
        }
#pragma unroll
        for (int j = 0; j < R; ++j)
#pragma unroll
            for (int t = 0; t < TT; ++t)
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) acc[j][t] += __shfl_xor(acc[j][t], o, 64);     // every lane ends with the same sum
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int row = row0 + j;
            if (row < m) {
                const float cl = closest[row];
#pragma unroll
                for (int t = 0; t < TT; ++t) {
                    const float v = fminf(cl, acc[j][t]);
                    if (lane == t) dmin[(size_t)t * m + row] = v;
                    pot[t] += (double)v;
                }
            }
        }
    }
    if (lane == 0)
#pragma unroll
        for (int t = 0; t < TT; ++t) wp[w * TT + t] = pot[t];
    __syncthreads();
    if (tid < TT) partials[(size_t)tid * KM_PP_MAXG + blockIdx.x] = ((wp[tid] + wp[TT + tid]) + wp[2 * TT + tid]) + wp[3 * TT + tid];
}

// Winner = the candidate of lowest potential (ties: first), every workgroup forms the same fixed-order sums; closest <- dmin[winner];
// workgroup 0 writes centres[k], the transposed copy, the chosen row, the potential, and advances the device counter.
__global__ __launch_bounds__(256) void km_pp_final_kernel(const float* __restrict__ x, float* __restrict__ closest,
                                                          const KmPPHeader* __restrict__ hdr, const float* __restrict__ dmin,
                                                          const double* __restrict__ partials, int* __restrict__ counter,
                                                          float* __restrict__ centres, float* __restrict__ centres_T,
                                                          int* __restrict__ chosen, double* __restrict__ pots, int m, int D, int K, int trials,
                                                          int G) {
    __shared__ double pot[KM_MAX_TRIALS];
    __shared__ int win;
    const int k = hdr->k;
    if (k < 0 || k >= K) return;
    const int tid = threadIdx.x;
    if (tid < trials) {
        double s = 0.0;
        for (int g = 0; g < G; ++g) s += partials[(size_t)tid * KM_PP_MAXG + g];
        pot[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int wv = 0;
        for (int t = 1; t < trials; ++t)
            if (pot[t] < pot[wv]) wv = t;
        win = wv;
    }
    __syncthreads();
    const int wv = win;
    const int i = blockIdx.x * 256 + tid;
    if (i < m) closest[i] = dmin[(size_t)wv * m + i];
    if (blockIdx.x == 0) {
        const int c = hdr->cand[wv];
        for (int d = tid; d < D; d += 256) {
            const float v = x[(size_t)c * D + d];
            centres[(size_t)k * D + d] = v;
            centres_T[(size_t)d * K + k] = v;
        }
        if (tid == 0) {
            chosen[k] = c;
            pots[k] = pot[wv];
            counter[0] = k + 1;
        }
    }
}

extern "C" long long omlm_kmeans_pp_workspace_bytes(int m, int trials) {
    if (m <= 0 || trials <= 0 || trials > KM_MAX_TRIALS) return -1;
    return (long long)(km_pp_dmin_offset() + sizeof(float) * (size_t)km_tt(trials) * (size_t)m);
}

template <int TT, int R>
static void km_pp_dist_launch(hipStream_t st, const float* rows, const float* closest, const KmPPHeader* hdr, float* dmin,
                              double* partials, int m, int D, int K, int G) {
    const size_t lds = (((size_t)TT * D * sizeof(float) + 15) & ~(size_t)15) + sizeof(double) * 4 * TT;
    if (D % 4 == 0)
        hipLaunchKernelGGL((km_pp_dist_kernel<TT, R, 4>), dim3(G), dim3(256), lds, st, rows, closest, hdr, dmin, partials, m, D, K);
    else
        hipLaunchKernelGGL((km_pp_dist_kernel<TT, R, 1>), dim3(G), dim3(256), lds, st, rows, closest, hdr, dmin, partials, m, D, K);
}

static int km_pp_check(const float* rows, float* closest, const float* uniforms, int* pick_counter, float* centres, float* centres_T,
                       int* chosen, double* pots, void* workspace, long long workspace_bytes, int m, int D, int K, int trials) {
    OMLM_CHECK_ARG(rows && closest && uniforms && pick_counter && centres && centres_T && chosen && pots && workspace,
                   "kmeans_pp pointers");
    OMLM_CHECK_ARG(m > 0 && D > 0 && K > 0 && K <= m, "kmeans_pp sizes (need 0 < K <= m)");
    OMLM_CHECK_ARG(trials >= 1 && trials <= KM_MAX_TRIALS, "kmeans_pp trials (1..16)");
    OMLM_CHECK_ARG((size_t)km_tt(trials) * D * sizeof(float) <= 60 * 1024, "kmeans_pp: trials x D too large for LDS");
    OMLM_CHECK_ARG(workspace_bytes >= omlm_kmeans_pp_workspace_bytes(m, trials), "kmeans_pp workspace too small");
    OMLM_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)rows & 15) == 0, "kmeans_pp alignment (16 bytes)");
    return OMLM_OK;
}

static void km_pp_queue_pick(hipStream_t st, const float* rows, float* closest, const float* uniforms, int* pick_counter, float* centres,
                             float* centres_T, int* chosen, double* pots, void* workspace, int m, int D, int K, int trials) {
    KmPPHeader* hdr = (KmPPHeader*)workspace;
    double* partials = (double*)((char*)workspace + sizeof(KmPPHeader));
    float* dmin = (float*)((char*)workspace + km_pp_dmin_offset());
    const int TT = km_tt(trials), G = km_pp_grid(m, TT);
    hipLaunchKernelGGL(km_pp_select_kernel, dim3(1), dim3(1024), 0, st, closest, uniforms, (const int*)pick_counter, hdr, m, K, trials, TT);
    if (TT == 4) km_pp_dist_launch<4, 4>(st, rows, closest, hdr, dmin, partials, m, D, K, G);
    else if (TT == 8) km_pp_dist_launch<8, 4>(st, rows, closest, hdr, dmin, partials, m, D, K, G);
    else km_pp_dist_launch<16, 2>(st, rows, closest, hdr, dmin, partials, m, D, K, G);
    hipLaunchKernelGGL(km_pp_final_kernel, dim3((m + 255) / 256), dim3(256), 0, st, rows, closest, (const KmPPHeader*)hdr,
                       (const float*)dmin, (const double*)partials, pick_counter, centres, centres_T, chosen, pots, m, D, K, trials, G);
}

// one pick: number *pick_counter (device), which the call advances
extern "C" int omlm_kmeans_pp_pick(const float* rows, float* closest, const float* uniforms, int* pick_counter, float* centres,
                                   float* centres_T, int* chosen, double* pots, void* workspace, long long workspace_bytes, int m, int D,
                                   int K, int trials, void* stream) {
    const int rc = km_pp_check(rows, closest, uniforms, pick_counter, centres, centres_T, chosen, pots, workspace, workspace_bytes, m, D,
                               K, trials);
    if (rc != OMLM_OK) return rc;
    km_pp_queue_pick(as_stream(stream), rows, closest, uniforms, pick_counter, centres, centres_T, chosen, pots, workspace, m, D, K, trials);
    return omlm_post_launch("omlm_kmeans_pp_pick");
}

// a whole seeding: counter <- 0, then K picks queued back to back; nothing returns to the host
extern "C" int omlm_kmeans_pp_seed(const float* rows, float* closest, const float* uniforms, int* pick_counter, float* centres,
                                   float* centres_T, int* chosen, double* pots, void* workspace, long long workspace_bytes, int m, int D,
                                   int K, int trials, void* stream) {
    const int rc = km_pp_check(rows, closest, uniforms, pick_counter, centres, centres_T, chosen, pots, workspace, workspace_bytes, m, D,
                               K, trials);
    if (rc != OMLM_OK) return rc;
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(pick_counter, 0, sizeof(int), st) != hipSuccess) return omlm_post_launch("omlm_kmeans_pp_seed (memset)");
    for (int k = 0; k < K; ++k)
        km_pp_queue_pick(st, rows, closest, uniforms, pick_counter, centres, centres_T, chosen, pots, workspace, m, D, K, trials);
    return omlm_post_launch("omlm_kmeans_pp_seed");
}

// ---- assign: mini-batch step and inertia -------------------------------------------------------------------------------------
// state (fp64 x 8, device): [0] ewa inertia, [1] its minimum, [2] last batch inertia (mean), [3] last squared centre movement,
// [4] steps done, [5] steps without improvement, [6] stopped (0 no, 1 no improvement, 2 tol), [7] 0 = no ewa yet, 1 = ewa, 2 = minimum.
// KM_ROWS rows per workgroup pass (row i of the pass is x[idx[row]] or x[row]); each thread walks its codes once for all of them
// (vq_nearest.h: the bits of omlm_nearest_centroid).  Rows whose index is out of range take no part.
__global__ __launch_bounds__(256) void km_assign_kernel(const float* __restrict__ x, const int* __restrict__ idx, int n_src, int n_rows,
                                                        int D, int K, const float* __restrict__ cT, int* __restrict__ labels,
                                                        float* __restrict__ rowmin, float* __restrict__ bcounts, float* __restrict__ sums,
                                                        double* __restrict__ inertia, const double* __restrict__ state) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* r = (float*)smem;                              // [KM_ROWS][D]
    __shared__ float bd[KM_ROWS][4];
    __shared__ int bi[KM_ROWS][4];
    __shared__ int src[KM_ROWS];
    __shared__ int chosen[KM_ROWS];
    __shared__ float chosen_d[KM_ROWS];
    if (state && state[6] != 0.0) return;
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int row0 = blockIdx.x * KM_ROWS; row0 < n_rows; row0 += gridDim.x * KM_ROWS) {
        if (tid < KM_ROWS) {
            const int row = row0 + tid;
            int s = -1;
            if (row < n_rows) {
                s = idx ? idx[row] : row;
                if (s < 0 || s >= n_src) s = -1;
            }
            src[tid] = s;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KM_ROWS; ++j) {
            const int s = src[j];
            for (int d = tid; d < D; d += 256) r[j * D + d] = s >= 0 ? x[(size_t)s * D + d] : 0.f;
        }
        __syncthreads();
        float best[KM_ROWS];
        int besti[KM_ROWS];
#pragma unroll
        for (int j = 0; j < KM_ROWS; ++j) { best[j] = INFINITY; besti[j] = 0x7fffffff; }
        sq_nearest_thread_rows<KM_ROWS>(r, cT, D, K, best, besti);
#pragma unroll
        for (int j = 0; j < KM_ROWS; ++j) {
            wave_lexmin(best[j], besti[j]);
            if ((tid & 63) == 0) { bd[j][tid >> 6] = best[j]; bi[j][tid >> 6] = besti[j]; }
        }
        __syncthreads();
        if (tid < KM_ROWS) {
            float b; int i0;
            lexmin4(bd[tid], bi[tid], b, i0);
            chosen[tid] = i0;
            chosen_d[tid] = b;
            const int row = row0 + tid;
            if (row < n_rows) {
                const bool live = src[tid] >= 0;
                if (labels) labels[row] = live ? i0 : -1;
                if (rowmin) rowmin[row] = live ? b : 0.f;
            }
        }
        __syncthreads();
        if (sums) {
#pragma unroll
            for (int j = 0; j < KM_ROWS; ++j) {
                if (src[j] < 0) continue;
                const int kk = chosen[j];
                for (int d = tid; d < D; d += 256) unsafeAtomicAdd(sums + (size_t)kk * D + d, r[j * D + d]);
                if (tid == 0) unsafeAtomicAdd(bcounts + kk, 1.0f);
            }
        }
        if (inertia && tid == 0)
            for (int j = 0; j < KM_ROWS; ++j)
                if (src[j] >= 0) acc += (double)chosen_d[j];
        __syncthreads();
    }
    if (inertia && tid == 0) unsafeAtomicAdd(inertia, acc);            // one atomic per workgroup
}

// fixed-order block sum of doubles (256 threads)
__device__ __forceinline__ double km_block_sum256(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const double t = red[0];
    __syncthreads();
    return t;
}

// one workgroup per centre: counts_k += m_k; c_k += (sum_k - m_k c_k) / counts_k for centres that received rows; batch sums zeroed for
// the next step; the squared movement of the centre goes to move_partial[k]
__global__ __launch_bounds__(256) void km_update_kernel(float* __restrict__ centres, float* __restrict__ cT, float* __restrict__ counts,
                                                        float* __restrict__ bcounts, float* __restrict__ sums,
                                                        double* __restrict__ move_partial, const double* __restrict__ state, int K, int D) {
    __shared__ double red[256];
    if (state[6] != 0.0) return;
    const int k = blockIdx.x, tid = threadIdx.x;
    const float mk = bcounts[k];
    const float cnt = counts[k] + mk;
    double mv = 0.0;
    if (mk > 0.f) {
        for (int d = tid; d < D; d += 256) {
            const float c = centres[(size_t)k * D + d];
            const float cn = c + (sums[(size_t)k * D + d] - mk * c) / cnt;
            centres[(size_t)k * D + d] = cn;
            cT[(size_t)d * K + k] = cn;
            sums[(size_t)k * D + d] = 0.f;
            mv += (double)(cn - c) * (double)(cn - c);
        }
    }
    const double tot = km_block_sum256(mv, red);       // barrier: every thread has read counts[k] / bcounts[k]
    if (tid == 0) {
        move_partial[k] = tot;
        if (mk > 0.f) { counts[k] = cnt; bcounts[k] = 0.f; }
    }
}

// one workgroup: batch inertia (fixed-order fp64 sum of the per-row minima / B), squared movement, sklearn's stopping rules
// (_mini_batch_convergence: the first step is ignored; ewa <- ewa (1 - alpha) + batch alpha; tol on the movement; max_no_improvement
// steps without a new ewa minimum)
__global__ __launch_bounds__(256) void km_stats_kernel(const float* __restrict__ rowmin, const double* __restrict__ move_partial,
                                                       double* __restrict__ state, int B, int K, double alpha, double tol_abs, int use_tol,
                                                       int max_no_improvement) {
    __shared__ double red[256];
    if (state[6] != 0.0) return;
    const int tid = threadIdx.x;
    double s = 0.0, mv = 0.0;
    for (int i = tid; i < B; i += 256) s += (double)rowmin[i];
    for (int i = tid; i < K; i += 256) mv += move_partial[i];
    s = km_block_sum256(s, red);
    mv = km_block_sum256(mv, red);
    if (tid != 0) return;
    const double batch = s / (double)B;
    const int step = (int)state[4] + 1;
    state[4] = (double)step;
    state[2] = batch;
    state[3] = mv;
    if (step == 1) return;
    double ewa;
    if (state[7] == 0.0) { ewa = batch; state[7] = 1.0; }
    else ewa = state[0] * (1.0 - alpha) + batch * alpha;
    state[0] = ewa;
    if (use_tol && mv <= tol_abs) { state[6] = 2.0; return; }
    if (state[7] < 2.0 || ewa < state[1]) { state[1] = ewa; state[5] = 0.0; state[7] = 2.0; }
    else state[5] += 1.0;
    if (max_no_improvement > 0 && state[5] >= (double)max_no_improvement) state[6] = 1.0;
}

static inline int km_assign_grid(int n_rows) {
    const int g = (n_rows + KM_ROWS - 1) / KM_ROWS;
    return g < 4096 ? g : 4096;
}

// one mini-batch step: rows x[idx[0..B)] against the current centres.  bcounts [K] / sums [K, D] must be zero on entry of the first
// step (every step leaves them zero); rowmin [B], move_partial [K] (fp64) and state (fp64 x 8, zeroed before the first step) are device
// buffers of the caller.  Once state[6] != 0 a step changes nothing (steps queued behind a stop are no-ops).
extern "C" int omlm_kmeans_minibatch_step(const float* x, const int* idx, float* centres, float* centres_T, float* counts, float* bcounts,
                                          float* sums, float* rowmin, double* move_partial, double* state, int n, int B, int D, int K,
                                          double alpha, double tol_abs, int max_no_improvement, void* stream) {
    OMLM_CHECK_ARG(x && idx && centres && centres_T && counts && bcounts && sums && rowmin && move_partial && state,
                   "kmeans_minibatch_step pointers");
    OMLM_CHECK_ARG(n > 0 && B > 0 && D > 0 && K > 0, "kmeans_minibatch_step sizes");
    OMLM_CHECK_ARG((size_t)KM_ROWS * D * sizeof(float) <= 48 * 1024, "D too large");
    OMLM_CHECK_ARG(alpha >= 0.0 && alpha <= 1.0 && tol_abs >= 0.0 && max_no_improvement >= 0, "kmeans_minibatch_step stopping parameters");
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(km_assign_kernel, dim3(km_assign_grid(B)), dim3(256), (size_t)KM_ROWS * D * sizeof(float), st, x, idx, n, B, D, K,
                       (const float*)centres_T, (int*)nullptr, rowmin, bcounts, sums, (double*)nullptr, (const double*)state);
    hipLaunchKernelGGL(km_update_kernel, dim3(K), dim3(256), 0, st, centres, centres_T, counts, bcounts, sums, move_partial,
                       (const double*)state, K, D);
    hipLaunchKernelGGL(km_stats_kernel, dim3(1), dim3(256), 0, st, (const float*)rowmin, (const double*)move_partial, state, B, K, alpha,
                       tol_abs, tol_abs > 0.0 ? 1 : 0, max_no_improvement);
    return omlm_post_launch("omlm_kmeans_minibatch_step");
}

// out[0] += sum_i min_k |x_i - c_k|^2 (fp64; the caller zeroes it); labels (int32 [n]) optional
extern "C" int omlm_kmeans_inertia(const float* x, const float* centres_T, double* out, int* labels, int n, int D, int K, void* stream) {
    if (n <= 0) return OMLM_OK;
    OMLM_CHECK_ARG(x && centres_T && out && D > 0 && K > 0, "kmeans_inertia arguments");
    OMLM_CHECK_ARG((size_t)KM_ROWS * D * sizeof(float) <= 48 * 1024, "D too large");
    int g = (n + KM_ROWS - 1) / KM_ROWS;
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(km_assign_kernel, dim3(g), dim3(256), (size_t)KM_ROWS * D * sizeof(float), as_stream(stream), x, (const int*)nullptr, n,
                       n, D, K, centres_T, labels, (float*)nullptr, (float*)nullptr, (float*)nullptr, out, (const double*)nullptr);
    return omlm_post_launch("omlm_kmeans_inertia");
}
