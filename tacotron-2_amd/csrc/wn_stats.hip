// Training summaries: the histogram of a ragged batch and the per-tensor norms of a flat buffer (wn_stats_* of include/wavenet_mi355.h).  Replaces the
// tf.summary.histogram ops and the per-variable tf.norm of the reference's add_train_stats (wavenet_vocoder/train.py:41-56), which ran inside the
// session, by two reductions where the data is: the step's own y_hat, targets and gradient buffer.
//
// Memory-bound by construction and small: every input element is read once, coalesced (lane t of a workgroup takes elements t, t + 256, ... of its
// segment).  Each call is a store pass and a sum pass in two launches -- nothing waits across workgroups and no float is added atomically:
//   store   one workgroup per segment of a row (histogram) or of a tensor.  Histogram: the bucket table (1551 doubles, 12.4 KB) sits in LDS, every lane
//           finds its element's bucket there by binary search and counts it with an integer LDS atomic (integer adds commute); the lanes' double
//           accumulators join in a halving tree; the workgroup stores its 1551 counts and 8 doubles into its own slot.
//   sum     buckets: one lane per bucket adds the slots' counts (int64); summary / tensors: the slots join in the fixed order of wn_stats.h.
// The sum pass writes every output element, so the caller clears nothing.  All arithmetic is in wn_stats.h, shared with the host hooks.
#include "wn_stats.h"
#include "wn_common.h"

struct wn_stats {
    wn_stats_config cfg;
    std::string err;
    int nt = 0, seg_max = 0;                 // the tensor table: entries, and the most segments any tensor has
    DevBuf<double> limits;                   // [WN_HIST_BUCKETS]
    DevBuf<int32_t> hist_part;               // [max_rows * 64][WN_HIST_BUCKETS] the segments' counts
    DevBuf<double> hist_sum;                 // [max_rows * 64][8] the segments' accumulators
    DevBuf<int64_t> t_off, t_cnt;            // [max_tensors]
    DevBuf<double> t_part;                   // [max_tensors * 64][4]
};

struct StatsHistArgs {
    const float* x; const int32_t* lengths; const double* limits; int32_t* part; double* psum; int64_t* bucket; double* summary;
    int64_t pitch; int32_t B, T;
};
struct StatsTensorArgs { const float* flat; const int64_t* off; const int64_t* cnt; double* part; double* out; };

__global__ __launch_bounds__(STATS_THREADS) void wn_stats_hist_store_kernel(const StatsHistArgs g) {
    __shared__ double lim[WN_HIST_BUCKETS];
    __shared__ int32_t hist[WN_HIST_BUCKETS];
    __shared__ double red[STATS_HQ][STATS_THREADS];
    const int tid = threadIdx.x, s = blockIdx.x, r = blockIdx.y;
    const int n = stats_row_len(g.lengths, r, g.T);
    if (s >= stats_nseg(n)) return;          // block-uniform: no barrier has been reached; the sum pass skips the same slots
    for (int b = tid; b < WN_HIST_BUCKETS; b += STATS_THREADS) { lim[b] = g.limits[b]; hist[b] = 0; }
    __syncthreads();
    const int64_t len = stats_seglen(n), i0 = s * len, i1 = i0 + len < n ? i0 + len : n;
    const float* row = g.x + (int64_t)r * g.pitch;
    double a[STATS_HQ];
    for (int q = 0; q < STATS_HQ; ++q) a[q] = stats_hist_identity(q);
    for (int64_t i = i0 + tid; i < i1; i += STATS_THREADS) {
        const int bk = stats_hist_add(a, lim, row[i]);
        if (bk >= 0) atomicAdd(&hist[bk], 1);
    }
    for (int q = 0; q < STATS_HQ; ++q) red[q][tid] = a[q];
    __syncthreads();
    for (int h = STATS_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h)
            for (int q = 0; q < STATS_HQ; ++q) red[q][tid] = stats_hist_join(q, red[q][tid], red[q][tid + h]);
        __syncthreads();
    }
    const int64_t slot = (int64_t)r * STATS_MAX_SEG + s;
    if (tid < STATS_HQ) g.psum[slot * STATS_HQ + tid] = red[tid][0];
    for (int b = tid; b < WN_HIST_BUCKETS; b += STATS_THREADS) g.part[slot * WN_HIST_BUCKETS + b] = hist[b];
}

#define STATS_BUCKET_BLOCKS ((WN_HIST_BUCKETS + STATS_THREADS - 1) / STATS_THREADS)

// blocks 0 ... STATS_BUCKET_BLOCKS - 1: one lane per bucket; the last block: the summary
__global__ __launch_bounds__(STATS_THREADS) void wn_stats_hist_sum_kernel(const StatsHistArgs g) {
    __shared__ double red[STATS_HQ][STATS_THREADS];
    const int tid = threadIdx.x;
    if (blockIdx.x < STATS_BUCKET_BLOCKS) {
        const int b = blockIdx.x * STATS_THREADS + tid;
        if (b >= WN_HIST_BUCKETS) return;
        int64_t c = 0;
        for (int r = 0; r < g.B; ++r) {
            const int k = stats_nseg(stats_row_len(g.lengths, r, g.T));
            for (int s = 0; s < k; ++s) c += g.part[((int64_t)r * STATS_MAX_SEG + s) * WN_HIST_BUCKETS + b];
        }
        g.bucket[b] = c;
        return;
    }
    double a[STATS_HQ];
    for (int q = 0; q < STATS_HQ; ++q) a[q] = stats_hist_identity(q);
    const int64_t slots = (int64_t)g.B * STATS_MAX_SEG;
    for (int64_t j = tid; j < slots; j += STATS_THREADS) {
        const int r = (int)(j / STATS_MAX_SEG), s = (int)(j % STATS_MAX_SEG);
        const bool live = s < stats_nseg(stats_row_len(g.lengths, r, g.T));
        for (int q = 0; q < STATS_HQ; ++q) a[q] = stats_hist_join(q, a[q], live ? g.psum[j * STATS_HQ + q] : stats_hist_identity(q));
    }
    for (int q = 0; q < STATS_HQ; ++q) red[q][tid] = a[q];
    __syncthreads();
    for (int h = STATS_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h)
            for (int q = 0; q < STATS_HQ; ++q) red[q][tid] = stats_hist_join(q, red[q][tid], red[q][tid + h]);
        __syncthreads();
    }
    if (tid == 0) {
        double f[STATS_HQ], o[STATS_HQ];
        for (int q = 0; q < STATS_HQ; ++q) f[q] = red[q][0];
        stats_hist_finish(f, o);
        for (int q = 0; q < STATS_HQ; ++q) g.summary[q] = o[q];
    }
}

// grid (segments, tensors)
__global__ __launch_bounds__(STATS_THREADS) void wn_stats_tensor_store_kernel(const StatsTensorArgs g) {
    __shared__ double red[STATS_TQ][STATS_THREADS];
    const int tid = threadIdx.x, s = blockIdx.x, t = blockIdx.y;
    const int64_t n = g.cnt[t];
    if (s >= stats_nseg(n)) return;
    const int64_t len = stats_seglen(n), i0 = s * len, i1 = i0 + len < n ? i0 + len : n;
    const float* x = g.flat + g.off[t];
    double a[STATS_TQ] = {0.0, 0.0, 0.0};
    for (int64_t i = i0 + tid; i < i1; i += STATS_THREADS) stats_tensor_add(a, x[i]);
    for (int q = 0; q < STATS_TQ; ++q) red[q][tid] = a[q];
    __syncthreads();
    for (int h = STATS_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h)
            for (int q = 0; q < STATS_TQ; ++q) red[q][tid] = stats_tensor_join(q, red[q][tid], red[q][tid + h]);
        __syncthreads();
    }
    if (tid < STATS_TQ) g.part[((int64_t)t * STATS_MAX_SEG + s) * 4 + tid] = red[tid][0];
}

// one workgroup of 64 lanes per tensor: lane s holds segment s (identity beyond the tensor's segments)
__global__ __launch_bounds__(STATS_MAX_SEG) void wn_stats_tensor_sum_kernel(const StatsTensorArgs g) {
    __shared__ double red[STATS_TQ][STATS_MAX_SEG];
    const int s = threadIdx.x, t = blockIdx.x;
    const int64_t n = g.cnt[t];
    const bool live = s < stats_nseg(n);
    for (int q = 0; q < STATS_TQ; ++q) red[q][s] = live ? g.part[((int64_t)t * STATS_MAX_SEG + s) * 4 + q] : 0.0;
    __syncthreads();
    for (int h = STATS_MAX_SEG / 2; h > 0; h >>= 1) {
        if (s < h)
            for (int q = 0; q < STATS_TQ; ++q) red[q][s] = stats_tensor_join(q, red[q][s], red[q][s + h]);
        __syncthreads();
    }
    if (s < 4) g.out[(int64_t)t * 4 + s] = s < STATS_TQ ? red[s][0] : (double)n;
}

extern "C" int wn_stats_create(const wn_stats_config* cfg, wn_stats** out) {
    wn_stats* z = nullptr;
    if (!cfg || !out) WN_FAIL(z, WN_E_ARG, "wn_stats_create: null argument");
    *out = nullptr;
    char msg[256];
    if (int rc = wn_stats_check_config(cfg, msg, sizeof msg)) WN_FAIL(z, rc, "wn_stats_create: %s", msg);
    wn_stats* p = new wn_stats();
    p->cfg = *cfg;
    int rc = cfg->max_rows == 0 ? WN_OK : [&]() -> int {
        std::vector<double> lim(WN_HIST_BUCKETS);
        if (wn_stats_build_limits(lim.data()) != WN_HIST_BUCKETS) WN_FAIL(p, WN_E_STATE, "wn_stats_create: the bucket table does not have %d limits", WN_HIST_BUCKETS);
        WN_HIP(p, p->limits.reserve(WN_HIST_BUCKETS));
        WN_HIP(p, hipMemcpy(p->limits, lim.data(), lim.size() * sizeof(double), hipMemcpyHostToDevice));
        WN_HIP(p, p->hist_part.reserve((size_t)cfg->max_rows * STATS_MAX_SEG * WN_HIST_BUCKETS));
        WN_HIP(p, p->hist_sum.reserve((size_t)cfg->max_rows * STATS_MAX_SEG * STATS_HQ));
        if (cfg->max_tensors > 0) {
            WN_HIP(p, p->t_off.reserve(cfg->max_tensors));
            WN_HIP(p, p->t_cnt.reserve(cfg->max_tensors));
            WN_HIP(p, p->t_part.reserve((size_t)cfg->max_tensors * STATS_MAX_SEG * 4));
        }
        return WN_OK;
    }();
    if (rc != WN_OK) { g_create_err = p->err; delete p; return rc; }
    *out = p;
    return WN_OK;
}

extern "C" void wn_stats_destroy(wn_stats* p) { delete p; }

extern "C" const char* wn_stats_last_error(const wn_stats* p) { return p ? p->err.c_str() : g_create_err.c_str(); }

extern "C" int wn_stats_hist_limits(double* out, int32_t cap) {
    wn_stats* z = nullptr;
    if (cap < 0 || (!out && cap > 0)) WN_FAIL(z, WN_E_ARG, "wn_stats_hist_limits: null argument or negative cap");
    double lim[WN_HIST_BUCKETS];
    if (wn_stats_build_limits(lim) != WN_HIST_BUCKETS) WN_FAIL(z, WN_E_STATE, "wn_stats_hist_limits: the bucket table does not have %d limits", WN_HIST_BUCKETS);
    for (int i = 0; i < cap && i < WN_HIST_BUCKETS; ++i) out[i] = lim[i];
    return WN_HIST_BUCKETS;
}

extern "C" int wn_stats_histogram(wn_stats* p, const float* x, int64_t pitch, const int32_t* lengths, int32_t B, int32_t T, int64_t* bucket, double* summary, void* stream) {
    if (!p) return WN_E_ARG;
    char msg[256];
    if (int rc = wn_stats_check_hist("wn_stats_histogram", p->cfg.max_rows, p->cfg.max_time, x, pitch, B, T, bucket, summary, msg, sizeof msg)) WN_FAIL(p, rc, "%s", msg);
    hipStream_t st = (hipStream_t)stream;
    StatsHistArgs g;
    g.x = x; g.lengths = lengths; g.limits = p->limits; g.part = p->hist_part; g.psum = p->hist_sum; g.bucket = bucket; g.summary = summary;
    g.pitch = pitch; g.B = B; g.T = T;
    hipLaunchKernelGGL(wn_stats_hist_store_kernel, dim3(stats_nseg(T), B), dim3(STATS_THREADS), 0, st, g);
    WN_LAUNCH_CHECK(p);
    hipLaunchKernelGGL(wn_stats_hist_sum_kernel, dim3(STATS_BUCKET_BLOCKS + 1), dim3(STATS_THREADS), 0, st, g);
    WN_LAUNCH_CHECK(p);
    return WN_OK;
}

extern "C" int wn_stats_set_tensors(wn_stats* p, const int64_t* offsets, const int64_t* counts, int32_t nt) {
    if (!p) return WN_E_ARG;
    char msg[256];
    std::vector<int32_t> order(nt > 0 ? nt : 1);
    if (int rc = wn_stats_check_tensors("wn_stats_set_tensors", p->cfg.max_tensors, offsets, counts, nt, order.data(), msg, sizeof msg)) WN_FAIL(p, rc, "%s", msg);
    if (p->cfg.max_rows > 0) {
        WN_HIP(p, hipMemcpy(p->t_off, offsets, (size_t)nt * sizeof(int64_t), hipMemcpyHostToDevice));
        WN_HIP(p, hipMemcpy(p->t_cnt, counts, (size_t)nt * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    p->nt = nt; p->seg_max = 0;
    for (int i = 0; i < nt; ++i) if (stats_nseg(counts[i]) > p->seg_max) p->seg_max = stats_nseg(counts[i]);
    return WN_OK;
}

extern "C" int wn_stats_tensors(wn_stats* p, const float* flat, double* out, void* stream) {
    if (!p) return WN_E_ARG;
    if (!flat || !out) WN_FAIL(p, WN_E_ARG, "wn_stats_tensors: null argument");
    if (p->nt < 1) WN_FAIL(p, WN_E_STATE, "wn_stats_tensors: no tensor table (wn_stats_set_tensors)");
    if (p->cfg.max_rows == 0) WN_FAIL(p, WN_E_SHAPE, "wn_stats_tensors: a validation-only handle (max_rows = 0) runs nothing");
    hipStream_t st = (hipStream_t)stream;
    StatsTensorArgs g;
    g.flat = flat; g.off = p->t_off; g.cnt = p->t_cnt; g.part = p->t_part; g.out = out;
    hipLaunchKernelGGL(wn_stats_tensor_store_kernel, dim3(p->seg_max, p->nt), dim3(STATS_THREADS), 0, st, g);
    WN_LAUNCH_CHECK(p);
    hipLaunchKernelGGL(wn_stats_tensor_sum_kernel, dim3(p->nt), dim3(STATS_MAX_SEG), 0, st, g);
    WN_LAUNCH_CHECK(p);
    return WN_OK;
}

extern "C" int wn_test_stats_hist_host(const float* x, int64_t pitch, const int32_t* lengths, int32_t B, int32_t T, int64_t* bucket, double* summary) {
    wn_stats* z = nullptr;
    char msg[256];
    if (int rc = wn_stats_check_hist("wn_test_stats_hist_host", INT32_MAX, INT32_MAX, x, pitch, B, T, bucket, summary, msg, sizeof msg)) WN_FAIL(z, rc, "%s", msg);
    std::vector<double> lim(WN_HIST_BUCKETS);
    if (wn_stats_build_limits(lim.data()) != WN_HIST_BUCKETS) WN_FAIL(z, WN_E_STATE, "wn_test_stats_hist_host: the bucket table does not have %d limits", WN_HIST_BUCKETS);
    wn_stats_host_hist(lim.data(), x, pitch, lengths, B, T, bucket, summary);
    return WN_OK;
}

extern "C" int wn_test_stats_tensors_host(const float* flat, const int64_t* offsets, const int64_t* counts, int32_t nt, double* out) {
    wn_stats* z = nullptr;
    char msg[256];
    if (!flat || !out) WN_FAIL(z, WN_E_ARG, "wn_test_stats_tensors_host: null argument");
    std::vector<int32_t> order(nt > 0 ? nt : 1);
    if (int rc = wn_stats_check_tensors("wn_test_stats_tensors_host", INT32_MAX, offsets, counts, nt, order.data(), msg, sizeof msg)) WN_FAIL(z, rc, "%s", msg);
    wn_stats_host_tensors(flat, offsets, counts, nt, out);
    return WN_OK;
}
