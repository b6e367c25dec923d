// Training-summary statistics shared by the device kernels of wn_stats.hip, the host hooks wn_test_stats_hist_host / wn_test_stats_tensors_host and the
// stand-alone host program tests/host/stats_main.cpp: the histogram's bucket table and the search in it, the step that takes one element into a lane's
// accumulators, the cut of a row or a tensor into segments, the joins, and the validation of a configuration and of a call.  Everything here is written
// once and runs on either side, so the hooks give the device's bits.
//
// Order of every sum (what "fixed order" means here):
//   a run of n elements (one row of a histogram, one tensor of a flat buffer) is cut into k = stats_nseg(n) = min(64, ceil(n / 4096)) segments of
//   stats_seglen(n) = ceil(n / k) elements (the last may be shorter, or empty);
//   inside a segment   lane t of STATS_THREADS = 256 takes elements t, t + 256, ... ascending into double accumulators, and the 256 lanes join in a
//                      halving tree (t += t + 128, t += t + 64, ...);
//   a tensor           its up to 64 segment results sit in slots 0 ... 63 (identity beyond k) and join in a halving tree of 64;
//   a histogram        the slots j = row * 64 + segment of the whole call (identity beyond a row's k): lane t takes j = t, t + 256, ... ascending, and
//                      the 256 lanes join in the halving tree.
// Sums are doubles; the square of a float32 widened to double is exact, so sum_squares carries summation error only.  Minima, maxima and the integer
// counts (kept as doubles: all far below 2^53) are exact in any order.  Nothing depends on anything but the lengths.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/wavenet_mi355.h"

#define STATS_THREADS 256      // lanes of a workgroup
#define STATS_SEG_MIN 4096     // a run is cut only into segments of at least this many elements ...
#define STATS_MAX_SEG 64       // ... and into at most this many
#define STATS_POS 774          // positive limits below DBL_MAX: 1e-12 * 1.1^i < 1e20
#define STATS_MAX_DIM 65535    // rows / tensors of a handle (the second grid dimension)

// ---- the bucket table: TensorFlow's default summary limits.  ..., -1e-12 * 1.1, -1e-12, 0, 1e-12, 1e-12 * 1.1, ..., DBL_MAX by repeated multiplication
// in double (never pow: the products round differently); out [WN_HIST_BUCKETS], strictly ascending
static inline int wn_stats_build_limits(double* out) {
    int n = 0;
    for (double v = 1e-12; v < 1e20; v *= 1.1) {
        if (n < STATS_POS) out[STATS_POS + 2 + n] = v;
        ++n;
    }
    if (n != STATS_POS) return -1;
    out[2 * STATS_POS + 2] = DBL_MAX;
    out[STATS_POS + 1] = 0.0;
    for (int i = 0; i <= STATS_POS; ++i) out[STATS_POS - i] = -out[STATS_POS + 2 + i];
    return WN_HIST_BUCKETS;
}

// bucket of a FINITE x: the index of the first limit strictly greater than x (std::upper_bound); FLT_MAX < DBL_MAX, so there always is one
__host__ __device__ __forceinline__ int stats_bucket(const double* lim, float x) {
    const double v = (double)x;
    int lo = 0, hi = WN_HIST_BUCKETS - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lim[mid] > v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// 0 finite, 1 NaN, 2 +inf, 3 -inf, from the bits (no floating-point compare to be optimised away)
__host__ __device__ __forceinline__ int stats_class(float x) {
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    if ((u & 0x7f800000u) != 0x7f800000u) return 0;
    if (u & 0x007fffffu) return 1;
    return (u >> 31) ? 3 : 2;
}

// ---- the cut of a run of n elements
__host__ __device__ __forceinline__ int stats_nseg(int64_t n) {
    if (n <= 0) return 0;
    const int64_t k = (n + STATS_SEG_MIN - 1) / STATS_SEG_MIN;
    return k > STATS_MAX_SEG ? STATS_MAX_SEG : (int)k;
}
__host__ __device__ __forceinline__ int64_t stats_seglen(int64_t n) {
    const int k = stats_nseg(n);
    return k ? (n + k - 1) / k : 0;
}
// length of row r of a ragged batch: lengths[r] held inside [0, T]; NULL: T
__host__ __device__ __forceinline__ int stats_row_len(const int32_t* lengths, int r, int T) {
    if (!lengths) return T;
    const int n = lengths[r];
    return n < 0 ? 0 : n > T ? T : n;
}

// ---- accumulators.  Histogram: the eight of the summary, in its order; a join is + except for min (1) and max (2)
#define STATS_HQ 8
__host__ __device__ __forceinline__ double stats_hist_identity(int q) { return q == 1 ? (double)INFINITY : q == 2 ? -(double)INFINITY : 0.0; }
__host__ __device__ __forceinline__ double stats_hist_join(int q, double a, double b) {
#pragma clang fp contract(off)
    if (q == 1) return b < a ? b : a;
    if (q == 2) return b > a ? b : a;
    return a + b;
}
// one element into a lane's accumulators a[STATS_HQ]; returns its bucket, or -1 for a non-finite value (which enters its counter and nothing else)
__host__ __device__ __forceinline__ int stats_hist_add(double* a, const double* lim, float x) {
#pragma clang fp contract(off)
    const int c = stats_class(x);
    if (c) { a[4 + c] = a[4 + c] + 1.0; return -1; }
    const double v = (double)x;
    a[0] = a[0] + 1.0;
    if (v < a[1]) a[1] = v;
    if (v > a[2]) a[2] = v;
    a[3] = a[3] + v;
    a[4] = a[4] + v * v;
    return stats_bucket(lim, x);
}
// the joined accumulators -> summary[8]: an empty histogram has min = max = 0
__host__ __device__ __forceinline__ void stats_hist_finish(const double* a, double* summary) {
    for (int q = 0; q < STATS_HQ; ++q) summary[q] = a[q];
    if (a[0] == 0.0) summary[1] = summary[2] = 0.0;
}

// Tensor statistics: sum of squares (+), max |x| (max), non-finite count (+)
#define STATS_TQ 3
__host__ __device__ __forceinline__ double stats_tensor_join(int q, double a, double b) {
#pragma clang fp contract(off)
    if (q == 1) return b > a ? b : a;
    return a + b;
}
__host__ __device__ __forceinline__ void stats_tensor_add(double* a, float x) {
#pragma clang fp contract(off)
    if (stats_class(x)) { a[2] = a[2] + 1.0; return; }
    const double v = (double)x, m = v < 0.0 ? -v : v;
    a[0] = a[0] + v * v;
    if (m > a[1]) a[1] = m;
}

// ---- host: whole calls in the device's order (the hooks and stats_main.cpp)
// part [W][nq] -> part[0][.] by the halving tree of W lanes
template <class J> static inline void stats_host_tree(double* part, int W, int nq, J join) {
    for (int h = W / 2; h > 0; h >>= 1)
        for (int t = 0; t < h; ++t)
            for (int q = 0; q < nq; ++q) part[t * nq + q] = join(q, part[t * nq + q], part[(t + h) * nq + q]);
}

// bucket [WN_HIST_BUCKETS], summary [8]; lengths: HOST int32 [B] or NULL
static inline void wn_stats_host_hist(const double* lim, const float* x, int64_t pitch, const int32_t* lengths, int32_t B, int32_t T, int64_t* bucket, double* summary) {
    for (int b = 0; b < WN_HIST_BUCKETS; ++b) bucket[b] = 0;
    const size_t slots = (size_t)B * STATS_MAX_SEG;
    double* slot = (double*)malloc((slots ? slots : 1) * STATS_HQ * sizeof(double));
    double lane[STATS_THREADS * STATS_HQ];
    for (int r = 0; r < B; ++r) {
        const int n = stats_row_len(lengths, r, T), k = stats_nseg(n);
        const int64_t len = stats_seglen(n);
        for (int s = 0; s < STATS_MAX_SEG; ++s) {
            double* out = slot + ((size_t)r * STATS_MAX_SEG + s) * STATS_HQ;
            if (s >= k) { for (int q = 0; q < STATS_HQ; ++q) out[q] = stats_hist_identity(q); continue; }
            const int64_t i0 = s * len, i1 = i0 + len < n ? i0 + len : n;
            for (int t = 0; t < STATS_THREADS; ++t) {
                double* a = lane + t * STATS_HQ;
                for (int q = 0; q < STATS_HQ; ++q) a[q] = stats_hist_identity(q);
                for (int64_t i = i0 + t; i < i1; i += STATS_THREADS) {
                    const int bk = stats_hist_add(a, lim, x[(int64_t)r * pitch + i]);
                    if (bk >= 0) ++bucket[bk];
                }
            }
            stats_host_tree(lane, STATS_THREADS, STATS_HQ, stats_hist_join);
            for (int q = 0; q < STATS_HQ; ++q) out[q] = lane[q];
        }
    }
    for (int t = 0; t < STATS_THREADS; ++t) {
        double* a = lane + t * STATS_HQ;
        for (int q = 0; q < STATS_HQ; ++q) a[q] = stats_hist_identity(q);
        for (size_t j = t; j < slots; j += STATS_THREADS)
            for (int q = 0; q < STATS_HQ; ++q) a[q] = stats_hist_join(q, a[q], slot[j * STATS_HQ + q]);
    }
    stats_host_tree(lane, STATS_THREADS, STATS_HQ, stats_hist_join);
    stats_hist_finish(lane, summary);
    free(slot);
}

// out [nt, 4] = {sum of squares, max |x|, non-finite count, element count}
static inline void wn_stats_host_tensors(const float* flat, const int64_t* offsets, const int64_t* counts, int32_t nt, double* out) {
    double lane[STATS_THREADS * STATS_TQ], slot[STATS_MAX_SEG * STATS_TQ];
    for (int i = 0; i < nt; ++i) {
        const int64_t n = counts[i], len = stats_seglen(n);
        const int k = stats_nseg(n);
        const float* x = flat + offsets[i];
        for (int s = 0; s < STATS_MAX_SEG; ++s) {
            double* o = slot + s * STATS_TQ;
            o[0] = o[1] = o[2] = 0.0;
            if (s >= k) continue;
            const int64_t i0 = s * len, i1 = i0 + len < n ? i0 + len : n;
            for (int t = 0; t < STATS_THREADS; ++t) {
                double* a = lane + t * STATS_TQ;
                a[0] = a[1] = a[2] = 0.0;
                for (int64_t j = i0 + t; j < i1; j += STATS_THREADS) stats_tensor_add(a, x[j]);
            }
            stats_host_tree(lane, STATS_THREADS, STATS_TQ, stats_tensor_join);
            for (int q = 0; q < STATS_TQ; ++q) o[q] = lane[q];
        }
        stats_host_tree(slot, STATS_MAX_SEG, STATS_TQ, stats_tensor_join);
        out[i * 4 + 0] = slot[0]; out[i * 4 + 1] = slot[1]; out[i * 4 + 2] = slot[2]; out[i * 4 + 3] = (double)n;
    }
}

// ---- validation, before any device call: argument errors first, then shapes
#define WN_STATS_FAIL(code, ...) do { if (msg && cap > 0) snprintf(msg, (size_t)cap, __VA_ARGS__); return (code); } while (0)

static inline int wn_stats_check_config(const wn_stats_config* cfg, char* msg, int cap) {
    if (!cfg) WN_STATS_FAIL(WN_E_ARG, "null configuration");
    if (cfg->abi_version != WN_ABI_VERSION) WN_STATS_FAIL(WN_E_ARG, "abi_version %d != %d", cfg->abi_version, WN_ABI_VERSION);
    if (cfg->max_rows < 0 || cfg->max_rows > STATS_MAX_DIM) WN_STATS_FAIL(WN_E_ARG, "max_rows (%d) must be 0 ... %d", cfg->max_rows, STATS_MAX_DIM);
    if (cfg->max_time < 0 || (cfg->max_rows > 0 && cfg->max_time < 1)) WN_STATS_FAIL(WN_E_ARG, "max_time (%d) must be positive", cfg->max_time);
    if (cfg->max_tensors < 0 || cfg->max_tensors > STATS_MAX_DIM) WN_STATS_FAIL(WN_E_ARG, "max_tensors (%d) must be 0 ... %d", cfg->max_tensors, STATS_MAX_DIM);
    return WN_OK;
}
static inline int wn_stats_check_hist(const char* who, int32_t max_rows, int32_t max_time, const float* x, int64_t pitch, int32_t B, int32_t T, const int64_t* bucket,
                                      const double* summary, char* msg, int cap) {
    if (!x || !bucket || !summary) WN_STATS_FAIL(WN_E_ARG, "%s: null argument", who);
    if (B < 1) WN_STATS_FAIL(WN_E_ARG, "%s: B (%d) must be >= 1", who, B);
    if (T < 1) WN_STATS_FAIL(WN_E_ARG, "%s: T (%d) must be >= 1", who, T);
    if (B > max_rows) WN_STATS_FAIL(WN_E_SHAPE, "%s: B (%d) > max_rows = %d", who, B, max_rows);
    if (T > max_time) WN_STATS_FAIL(WN_E_SHAPE, "%s: T (%d) > max_time = %d", who, T, max_time);
    if (pitch < T) WN_STATS_FAIL(WN_E_SHAPE, "%s: pitch (%lld) < T = %d", who, (long long)pitch, T);
    return WN_OK;
}
// a tensor table: every count positive, no offset negative, no two tensors overlapping; order: scratch of nt int32
static inline int wn_stats_check_tensors(const char* who, int32_t max_tensors, const int64_t* offsets, const int64_t* counts, int32_t nt, int32_t* order, char* msg, int cap) {
    if (!offsets || !counts) WN_STATS_FAIL(WN_E_ARG, "%s: null argument", who);
    if (nt < 1) WN_STATS_FAIL(WN_E_ARG, "%s: nt (%d) must be >= 1", who, nt);
    for (int i = 0; i < nt; ++i) {
        if (counts[i] <= 0) WN_STATS_FAIL(WN_E_ARG, "%s: counts[%d] = %lld must be positive", who, i, (long long)counts[i]);
        if (offsets[i] < 0) WN_STATS_FAIL(WN_E_ARG, "%s: offsets[%d] = %lld is negative", who, i, (long long)offsets[i]);
    }
    if (nt > max_tensors) WN_STATS_FAIL(WN_E_SHAPE, "%s: nt (%d) > max_tensors = %d", who, nt, max_tensors);
    for (int i = 0; i < nt; ++i) order[i] = i;
    for (int i = 1; i < nt; ++i) {          // insertion sort by offset: tables arrive sorted
        const int v = order[i];
        int j = i;
        while (j > 0 && offsets[order[j - 1]] > offsets[v]) { order[j] = order[j - 1]; --j; }
        order[j] = v;
    }
    for (int i = 1; i < nt; ++i)
        if (offsets[order[i - 1]] + counts[order[i - 1]] > offsets[order[i]])
            WN_STATS_FAIL(WN_E_ARG, "%s: tensors %d and %d overlap", who, order[i - 1], order[i]);
    return WN_OK;
}
