// Pitch check: F0 and voicing of a ragged batch of signals by YIN on frames aligned with the mel frames, and the comparison of two such tracks
// (wn_pitch_* of include/wavenet_mi355.h).  What the reconstruction check cannot see -- pitch drift, octave jumps, flickering voicing -- measured where
// the generated samples and their target already are.
//
// One launch per group of 64 rows computes the difference function, its normalisation, the pick and the outputs.  A workgroup owns (row, tile of
// PITCH_TILE = 8 frames): all lanes stage the tile's signal span, 7 hop + window + tau_max floats, into LDS once, zero-filled outside [0, n) and never
// reading beyond lengths[b].  Then a lane owns a lag: it runs PITCH_CHAINS = 4 accumulators, frames 4 g ... 4 g + 3 of the tile at its lag tau, over
// j = 0 ... window - 1 ascending -- x_j is one address for every lane of the same frame group (a broadcast), x_{j+tau} is lane-consecutive (no bank
// conflict) -- and the (frame group, lag) items beyond one pass of the workgroup are taken in a stride loop.  The parallelism inside a lane comes from
// the independent chains, never from splitting one: the summation order is the contract (wn_pitch.h).  The d table of the tile lives in LDS; lane f of
// the first wavefront then runs the prefix, the normalisation and the pick of frame f, a few hundred operations, and all lanes copy d' out when it is
// asked for.  Bound by LDS reads: two 4-byte reads per (difference, fused multiply-add) pair.  A second kernel compares two tracks, one workgroup per
// row: all lanes form a chunk's per-frame terms (the log2 in double), one lane adds them in frame order.  No atomics, nothing shared between
// workgroups, no device memory of the handle's own, nothing allocated or synchronised by any call; all arithmetic is in wn_pitch.h, shared with the hooks.
#include "wn_pitch.h"
#include "wn_common.h"

struct wn_pitch {
    wn_pitch_config cfg;
    std::string err;
    size_t lds_bytes = 0;
};

struct PitchArgs {
    const float* wav; float* f0; float* ap; float* dprime;
    int64_t ld;
    int32_t b0, F_max, hop, window, tau_min, tau_max;
    float threshold, sample_rate;
    int32_t n[PITCH_GROUP];
};

__global__ __launch_bounds__(PITCH_THREADS) void wn_pitch_kernel(const PitchArgs g) {
    extern __shared__ float lds[];     // sig [span], d [PITCH_TILE][tau_max + 1]
    const int r = blockIdx.y, n = g.n[r], hop = g.hop, W = g.window, TM = g.tau_max, TP = TM + 1;
    const int F = 1 + n / hop, t0 = blockIdx.x * PITCH_TILE;
    if (t0 >= F) return;               // block-uniform: no barrier has been reached
    const int tid = threadIdx.x, L = W + TM;
    const int span = (PITCH_TILE - 1) * hop + L;
    const int64_t row = g.b0 + r;
    float* sig = lds;
    float* d = lds + pitch_span_floats(hop, W, TM);
    const float* x = g.wav + row * g.ld;
    const int64_t s0 = (int64_t)t0 * hop - L / 2;
    for (int i = tid; i < span; i += PITCH_THREADS) {
        const int64_t s = s0 + i;
        sig[i] = s >= 0 && s < n ? x[s] : 0.0f;
    }
    __syncthreads();
    const int items = (PITCH_TILE / PITCH_CHAINS) * TM;
    for (int it = tid; it < items; it += PITCH_THREADS) {
        const int grp = it / TM, tau = 1 + it % TM;
        const float* p = sig + grp * PITCH_CHAINS * hop;      // largest index read: 7 hop + (W - 1) + tau_max = span - 1
        float acc[PITCH_CHAINS];
#pragma unroll
        for (int c = 0; c < PITCH_CHAINS; ++c) acc[c] = 0.0f;
        for (int j = 0; j < W; ++j) {
#pragma unroll
            for (int c = 0; c < PITCH_CHAINS; ++c) acc[c] = pitch_term(acc[c], p[c * hop + j], p[c * hop + j + tau]);
        }
#pragma unroll
        for (int c = 0; c < PITCH_CHAINS; ++c) d[(grp * PITCH_CHAINS + c) * TP + tau] = acc[c];
    }
    __syncthreads();
    const int nf = F - t0 < PITCH_TILE ? F - t0 : PITCH_TILE;
    if (tid < nf) {
        float* dp = d + tid * TP;
        pitch_normalise(dp, TM);
        float v0, v1;
        pitch_pick(dp, g.tau_min, TM, g.threshold, g.sample_rate, &v0, &v1);
        const int64_t o = row * g.F_max + t0 + tid;
        g.f0[o] = v0;
        if (g.ap) g.ap[o] = v1;
    }
    if (!g.dprime) return;             // block-uniform
    __syncthreads();
    float* out = g.dprime + (row * g.F_max + t0) * TP;          // the tile's nf frames are one contiguous run of nf (tau_max + 1) floats
    for (int i = tid; i < nf * TP; i += PITCH_THREADS) out[i] = d[i];
}

struct PitchCmpArgs { const float* a; const float* b; float* table; int64_t pitch; int32_t b0; int32_t n[PITCH_GROUP]; };

__global__ __launch_bounds__(PITCH_THREADS) void wn_pitch_compare_kernel(const PitchCmpArgs g) {
    __shared__ double cents[PITCH_THREADS];
    __shared__ int32_t flags[PITCH_THREADS];
    const int tid = threadIdx.x, r = blockIdx.x, n = g.n[r];
    const int64_t row = g.b0 + r;
    const float* a = g.a + row * g.pitch;
    const float* b = g.b + row * g.pitch;
    PitchCmpSums s;                    // lane 0's
    for (int c0 = 0; c0 < n; c0 += PITCH_THREADS) {          // n is block-uniform: every lane reaches every barrier
        const int f = c0 + tid;
        if (f < n) pitch_cmp_frame(a[f], b[f], &flags[tid], &cents[tid]);
        __syncthreads();
        if (tid == 0) {
            const int m = n - c0 < PITCH_THREADS ? n - c0 : PITCH_THREADS;
            for (int k = 0; k < m; ++k) pitch_cmp_add(&s, flags[k], cents[k]);
        }
        __syncthreads();
    }
    if (tid == 0) pitch_cmp_finish(&s, n, g.table + row * PITCH_COLS);
}

extern "C" int wn_pitch_create(const wn_pitch_config* cfg, wn_pitch** out) {
    wn_pitch* z = nullptr;
    if (!cfg || !out) WN_FAIL(z, WN_E_ARG, "wn_pitch_create: null argument");
    *out = nullptr;
    char msg[256];
    if (int rc = wn_pitch_check_config(cfg, msg, sizeof msg)) WN_FAIL(z, rc, "wn_pitch_create: %s", msg);
    wn_pitch* p = new wn_pitch();
    p->cfg = *cfg;
    p->lds_bytes = (size_t)pitch_lds_floats(cfg->hop, cfg->window, cfg->tau_max) * sizeof(float);      // <= 64 KiB: no function attribute to raise
    *out = p;
    return WN_OK;
}

extern "C" void wn_pitch_destroy(wn_pitch* p) { delete p; }

extern "C" const char* wn_pitch_last_error(const wn_pitch* p) { return p ? p->err.c_str() : g_create_err.c_str(); }

extern "C" int64_t wn_pitch_num_frames(const wn_pitch* p, int64_t n_samples) {
    if (!p || n_samples < 0) return WN_E_ARG;
    return 1 + n_samples / p->cfg.hop;
}

extern "C" int wn_pitch_frame_tile(const wn_pitch* p) { return p ? PITCH_TILE : WN_E_ARG; }

extern "C" int wn_pitch_run(wn_pitch* p, const float* wav, int64_t ld, const int32_t* lengths, int32_t B, int32_t F_max, float* f0, float* ap, float* dprime, void* stream) {
    if (!p) return WN_E_ARG;
    char msg[256];
    if (int rc = wn_pitch_check_run("wn_pitch_run", &p->cfg, wav, ld, lengths, B, F_max, f0, msg, sizeof msg)) WN_FAIL(p, rc, "%s", msg);
    hipStream_t st = (hipStream_t)stream;
    PitchArgs g;
    g.wav = wav; g.f0 = f0; g.ap = ap; g.dprime = dprime; g.ld = ld; g.F_max = F_max;
    g.hop = p->cfg.hop; g.window = p->cfg.window; g.tau_min = p->cfg.tau_min; g.tau_max = p->cfg.tau_max;
    g.threshold = p->cfg.threshold; g.sample_rate = (float)p->cfg.sample_rate;
    for (int b0 = 0; b0 < B; b0 += PITCH_GROUP) {
        const int nb = B - b0 < PITCH_GROUP ? B - b0 : PITCH_GROUP;
        int32_t n_max = 0;
        g.b0 = b0;
        for (int r = 0; r < PITCH_GROUP; ++r) { g.n[r] = r < nb ? lengths[b0 + r] : 0; if (g.n[r] > n_max) n_max = g.n[r]; }
        hipLaunchKernelGGL(wn_pitch_kernel, dim3(cdiv(1 + n_max / p->cfg.hop, PITCH_TILE), nb), dim3(PITCH_THREADS), p->lds_bytes, st, g);
        WN_LAUNCH_CHECK(p);
    }
    return WN_OK;
}

extern "C" int wn_pitch_compare(wn_pitch* p, const float* f0_a, const float* f0_b, int64_t pitch, const int32_t* frames, int32_t B, float* table, void* stream) {
    if (!p) return WN_E_ARG;
    char msg[256];
    if (int rc = wn_pitch_check_compare("wn_pitch_compare", p->cfg.max_batch, 1 + p->cfg.max_samples / p->cfg.hop, f0_a, f0_b, pitch, frames, B, table, msg, sizeof msg))
        WN_FAIL(p, rc, "%s", msg);
    hipStream_t st = (hipStream_t)stream;
    PitchCmpArgs g;
    g.a = f0_a; g.b = f0_b; g.table = table; g.pitch = pitch;
    for (int b0 = 0; b0 < B; b0 += PITCH_GROUP) {
        const int nb = B - b0 < PITCH_GROUP ? B - b0 : PITCH_GROUP;
        g.b0 = b0;
        for (int r = 0; r < PITCH_GROUP; ++r) g.n[r] = r < nb ? frames[b0 + r] : 0;
        hipLaunchKernelGGL(wn_pitch_compare_kernel, dim3(nb), dim3(PITCH_THREADS), 0, st, g);
        WN_LAUNCH_CHECK(p);
    }
    return WN_OK;
}

extern "C" int wn_test_pitch_host(const wn_pitch_config* cfg, const float* wav, int64_t ld, const int32_t* lengths, int32_t B, int32_t F_max, float* f0, float* ap, float* dprime) {
    wn_pitch* z = nullptr;
    char msg[256];
    if (int rc = wn_pitch_check_config(cfg, msg, sizeof msg)) WN_FAIL(z, rc, "wn_test_pitch_host: %s", msg);
    if (int rc = wn_pitch_check_run("wn_test_pitch_host", cfg, wav, ld, lengths, B, F_max, f0, msg, sizeof msg)) WN_FAIL(z, rc, "%s", msg);
    std::vector<float> x((size_t)cfg->window + cfg->tau_max), dp((size_t)cfg->tau_max + 1);
    wn_pitch_host_rows(cfg, wav, ld, lengths, B, F_max, f0, ap, dprime, x.data(), dp.data());
    return WN_OK;
}

extern "C" int wn_test_pitch_compare_host(const float* f0_a, const float* f0_b, int64_t pitch, const int32_t* frames, int32_t B, float* table) {
    wn_pitch* z = nullptr;
    char msg[256];
    if (int rc = wn_pitch_check_compare("wn_test_pitch_compare_host", -1, -1, f0_a, f0_b, pitch, frames, B, table, msg, sizeof msg)) WN_FAIL(z, rc, "%s", msg);
    wn_pitch_compare_host_rows(f0_a, f0_b, pitch, frames, B, table);
    return WN_OK;
}
