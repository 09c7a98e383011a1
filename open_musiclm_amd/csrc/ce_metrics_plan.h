// Host-side plan of omlm_ce_metrics / omlm_ce_metrics_bins (csrc/ce_metrics.hip): which kernel serves a row width, with what grid, and every
// refusal -- pure functions of the scalar arguments, no HIP, so the host c++ builds this header on its own (OMLM_PLAN_TEST_ABI below).
#pragma once

#define CE_METRICS_NV 17                     /* register slots per lane of the wave-per-row kernel: CE_NV of csrc/embed_ce.hip */
#define CE_METRICS_BIN_THREADS 1024

enum { CE_METRICS_WAVE = 0, CE_METRICS_BLOCK = 1 };

// the route is a function of V alone: one wave per row while the row fits 64 lanes x CE_METRICS_NV registers, one workgroup per row above
static inline int ce_metrics_route(int V) { return V <= 64 * CE_METRICS_NV ? CE_METRICS_WAVE : CE_METRICS_BLOCK; }

// workgroups of 256 threads: four rows (waves) each on the wave route, one row each on the workgroup route; both walk further rows in trips
static inline int ce_metrics_grid(int R, int V) {
    if (ce_metrics_route(V) == CE_METRICS_WAVE) { const int blocks = (R + 3) / 4; return blocks < 1024 ? blocks : 1024; }
    return R < 4096 ? R : 4096;
}

// nullptr: the scalar arguments are fine; otherwise the refusal's message
static inline const char* ce_metrics_refusal(int R, int V, int ld) {
    if (R < 0) return "ce_metrics: R must be >= 0";
    if (V < 1) return "ce_metrics: V must be >= 1";
    if (ld < V) return "ce_metrics: ld must be >= V";
    return nullptr;
}
static inline const char* ce_metrics_bins_refusal(int R, int n, int Q, int V, int k_top) {
    if (R < 0) return "ce_metrics_bins: R must be >= 0";
    if (V < 1) return "ce_metrics_bins: V must be >= 1";
    if (n < 1) return "ce_metrics_bins: n must be >= 1";
    if (R % n != 0) return "ce_metrics_bins: R must be a multiple of n";
    if (Q < 1) return "ce_metrics_bins: Q must be >= 1";
    if (k_top < 1 || k_top > V) return "ce_metrics_bins: k_top must lie in [1, V]";
    return nullptr;
}

#ifdef OMLM_PLAN_TEST_ABI
extern "C" int omlm_plan_ce_metrics_route(int V) { return ce_metrics_route(V); }
extern "C" int omlm_plan_ce_metrics_grid(int R, int V) { return ce_metrics_grid(R, V); }
#endif
