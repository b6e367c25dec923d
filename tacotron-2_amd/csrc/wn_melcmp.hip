// Reconstruction check: per-frame and per-utterance distances between the mel-spectrogram of a generated signal and the conditioning it was generated
// from (wn_melcmp_* of include/wavenet_mi355.h).  Replaces the host side of the reference's only feedback on generated audio, the "Local Condition vs
// Reconst. Mel-Spectrogram" plot (a numpy melspectrogram of item 0 and a picture), by its numbers, for every row of a batch, where the samples already are.
//
// Memory-bound by construction: a and b are read twice (the compensated distances need the utterance's bias, which needs every frame), nothing else of
// size moves.  A workgroup of four wavefronts takes a tile of MELCMP_TF = 64 frames x num_mels: all lanes load a, then b, into one LDS tile -- along
// frames for a channels-first input, along channels for a channels-last one, so every global load is coalesced in either layout -- and form d in
// place.  From there the layout is forgotten: lane f of every wavefront owns frame f and walks its channels in LDS in ascending order (tile pitch odd:
// the 64 lanes fall on distinct banks; the DCT row is one address for the whole wavefront, a broadcast).  The four wavefronts share the work of a frame
// -- the cepstral coefficients k = 1 + q, 5 + q, ... go to wavefront q, bias / l1 / lsd to wavefronts 0 / 1 / 2 -- and the pieces join in a fixed order.
// Reductions over frames: one workgroup per row, lane t sums frames t, t + 256, ... and a halving tree joins the lanes.  No atomics, nothing shared
// between workgroups, nothing allocated or synchronised after wn_melcmp_create; all arithmetic is in wn_melcmp.h, shared with the host hook.
#include "wn_melcmp.h"
#include "wn_common.h"

struct wn_melcmp {
    wn_melcmp_config cfg;
    std::string err;
    size_t lds_bytes = 0;
    DevBuf<float> dct;                 // [n_cep, num_mels] rows 1 ... n_cep of D
    DevBuf<float> scratch;             // [max_batch, 6, max_frames] stands in for a NULL per_frame
};

struct MelcmpArgs {
    const float* a; const float* b; const float* dct; float* per_frame; float* summary; int32_t* marks;
    int64_t a_pitch, b_pitch, out_pitch;
    int32_t a_cf, b_cf, M, n_cep, b0, pass;      // pass (tile kernel) 0: bias, l1, lsd, mcd; 1: l1c, lsdc.  (reduce kernel) 0: the means of 0 ... 3; 1: of 4, 5, worst and marks
    float unit, alarm;
    int32_t n[MELCMP_GROUP];
};

// one input of a tile into LDS: x itself (FIRST) or d = unit * (tile - x) in place.  Each element is touched by exactly one lane per call.
template <bool FIRST>
__device__ __forceinline__ void melcmp_stage(float* tile, const float* x, int cf, int64_t pitch, int64_t row, int f0, int nf, int M, float unit) {
    const int tid = threadIdx.x, MP = melcmp_tile_pitch(M);
    if (cf) {                          // [B, M, pitch]: 64 consecutive frames of one channel per wavefront
        const int f = tid % MELCMP_TF;
        if (f < nf) {
            const float* src = x + row * M * pitch + f0 + f;
            for (int m = tid / MELCMP_TF; m < M; m += MELCMP_KQ) {
                const float v = src[(int64_t)m * pitch];
                float* t = tile + f * MP + m;
                *t = FIRST ? v : melcmp_diff(unit, *t, v);
            }
        }
    } else {                           // [B, pitch, M]: the tile's nf x M floats are one contiguous run
        const float* src = x + (row * pitch + f0) * M;
        const int cnt = nf * M;
        for (int i = tid; i < cnt; i += MELCMP_THREADS) {
            const float v = src[i];
            float* t = tile + (i / M) * MP + i % M;
            *t = FIRST ? v : melcmp_diff(unit, *t, v);
        }
    }
}

__global__ __launch_bounds__(MELCMP_THREADS) void wn_melcmp_tile_kernel(const MelcmpArgs g) {
    extern __shared__ float lds[];     // tile [TF][M | 1], parts [KQ][TF], dct [n_cep][M]
    const int r = blockIdx.y, n = g.n[r], f0 = blockIdx.x * MELCMP_TF;
    if (f0 >= n) return;               // block-uniform: no barrier has been reached
    const int tid = threadIdx.x, M = g.M, MP = melcmp_tile_pitch(M), nf = n - f0 < MELCMP_TF ? n - f0 : MELCMP_TF;
    const int64_t row = g.b0 + r;
    float* tile = lds;
    float* parts = tile + MELCMP_TF * MP;
    float* dct = parts + MELCMP_KQ * MELCMP_TF;
    if (g.pass == 0) for (int i = tid; i < g.n_cep * M; i += MELCMP_THREADS) dct[i] = g.dct[i];
    melcmp_stage<true>(tile, g.a, g.a_cf, g.a_pitch, row, f0, nf, M, g.unit);
    __syncthreads();
    melcmp_stage<false>(tile, g.b, g.b_cf, g.b_pitch, row, f0, nf, M, g.unit);
    __syncthreads();
    const int f = tid % MELCMP_TF, q = tid / MELCMP_TF;      // q is the wavefront: uniform
    const bool live = f < nf;
    const float* d = tile + f * MP;
    float* out = g.per_frame + row * 6 * g.out_pitch + f0 + f;
    if (g.pass == 0) {
        if (live) {
            parts[q * MELCMP_TF + f] = melcmp_frame_cep_part(d, dct, M, g.n_cep, q);
            if (q == 0) out[0] = melcmp_frame_bias(d, M);
            else if (q == 1) out[g.out_pitch] = melcmp_frame_l1(d, M, 0.0f);
            else if (q == 2) out[2 * g.out_pitch] = melcmp_frame_lsd(d, M, 0.0f);
        }
        __syncthreads();
        if (live && q == 3) out[3 * g.out_pitch] = melcmp_frame_mcd(parts[f], parts[MELCMP_TF + f], parts[2 * MELCMP_TF + f], parts[3 * MELCMP_TF + f]);
    } else if (live) {
        const float off = g.summary[row * 7];
        if (q == 0) out[4 * g.out_pitch] = melcmp_frame_l1(d, M, off);
        else if (q == 1) out[5 * g.out_pitch] = melcmp_frame_lsd(d, M, off);
    }
}

__global__ __launch_bounds__(MELCMP_THREADS) void wn_melcmp_reduce_kernel(const MelcmpArgs g) {
    __shared__ float red[MELCMP_THREADS];
    __shared__ int32_t red_at[MELCMP_THREADS], red_cnt[MELCMP_THREADS];
    const int tid = threadIdx.x, r = blockIdx.x, n = g.n[r];
    const int64_t row = g.b0 + r;
    const float* pf = g.per_frame + row * 6 * g.out_pitch;
    for (int j = g.pass ? 4 : 0; j < (g.pass ? 6 : 4); ++j) {
        red[tid] = melcmp_lane_sum(pf + j * g.out_pitch, n, tid);
        __syncthreads();
        for (int h = MELCMP_THREADS / 2; h > 0; h >>= 1) {
            if (tid < h) {
#pragma clang fp contract(off)
                red[tid] = red[tid] + red[tid + h];
            }
            __syncthreads();
        }
        if (tid == 0) g.summary[row * 7 + j] = melcmp_mean(red[0], n);
        __syncthreads();
    }
    if (!g.pass) return;
    float w; int32_t at, cnt;
    melcmp_lane_worst(pf + 4 * g.out_pitch, n, tid, g.alarm, &w, &at, &cnt);
    red[tid] = w; red_at[tid] = at; red_cnt[tid] = cnt;
    __syncthreads();
    for (int h = MELCMP_THREADS / 2; h > 0; h >>= 1) {           // a maximum with the earlier frame among equals, and an integer sum: exact in any order
        if (tid < h) {
            float w1 = red[tid]; int32_t i1 = red_at[tid];
            melcmp_join_worst(&w1, &i1, red[tid + h], red_at[tid + h]);
            red[tid] = w1; red_at[tid] = i1; red_cnt[tid] += red_cnt[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) { g.summary[row * 7 + 6] = red[0]; g.marks[row * 2] = red_at[0]; g.marks[row * 2 + 1] = red_cnt[0]; }
}

static size_t melcmp_lds_bytes(int M, int n_cep) { return ((size_t)MELCMP_TF * melcmp_tile_pitch(M) + MELCMP_KQ * MELCMP_TF + (size_t)n_cep * M) * sizeof(float); }

extern "C" int wn_melcmp_create(const wn_melcmp_config* cfg, wn_melcmp** out) {
    wn_melcmp* z = nullptr;
    if (!cfg || !out) WN_FAIL(z, WN_E_ARG, "wn_melcmp_create: null argument");
    *out = nullptr;
    char msg[256];
    if (int rc = wn_melcmp_check_config(cfg, msg, sizeof msg)) WN_FAIL(z, rc, "wn_melcmp_create: %s", msg);
    wn_melcmp* p = new wn_melcmp();
    p->cfg = *cfg;
    p->lds_bytes = melcmp_lds_bytes(cfg->num_mels, cfg->n_cep);      // at most 64 x 129 + 256 + 127 x 128 floats = 97 KiB of the 160
    int rc = cfg->max_batch == 0 ? WN_OK : [&]() -> int {
        std::vector<float> t((size_t)cfg->n_cep * cfg->num_mels);
        wn_melcmp_dct_table(cfg->num_mels, cfg->n_cep, t.data());
        WN_HIP(p, p->dct.reserve(t.size()));
        if (!t.empty()) WN_HIP(p, hipMemcpy(p->dct, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
        WN_HIP(p, p->scratch.reserve((size_t)cfg->max_batch * 6 * cfg->max_frames));
        // the attribute belongs to the function, not to the handle: always the module's largest tile (num_mels = 128, n_cep = 127), whatever this handle needs
        WN_HIP(p, hipFuncSetAttribute((const void*)wn_melcmp_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)melcmp_lds_bytes(MELCMP_MAX_MELS, MELCMP_MAX_MELS - 1)));
        return WN_OK;
    }();
    if (rc != WN_OK) { g_create_err = p->err; delete p; return rc; }
    *out = p;
    return WN_OK;
}

extern "C" void wn_melcmp_destroy(wn_melcmp* p) { delete p; }

extern "C" const char* wn_melcmp_last_error(const wn_melcmp* p) { return p ? p->err.c_str() : g_create_err.c_str(); }

extern "C" int wn_melcmp_run(wn_melcmp* p, const float* a, int32_t a_channels_first, int64_t a_pitch, const float* b, int32_t b_channels_first, int64_t b_pitch,
                             const int32_t* frames, int32_t B, float* per_frame, int64_t out_pitch, float* summary, int32_t* marks, void* stream) {
    if (!p) return WN_E_ARG;
    char msg[256];
    if (int rc = wn_melcmp_check_call("wn_melcmp_run", p->cfg.max_batch, p->cfg.max_frames, a, a_pitch, b, b_pitch, frames, B, per_frame, out_pitch, summary, marks, msg, sizeof msg))
        WN_FAIL(p, rc, "%s", msg);
    hipStream_t st = (hipStream_t)stream;
    MelcmpArgs g;
    g.a = a; g.b = b; g.dct = p->dct; g.summary = summary; g.marks = marks;
    g.per_frame = per_frame ? per_frame : p->scratch.get(); g.out_pitch = per_frame ? out_pitch : p->cfg.max_frames;
    g.a_pitch = a_pitch; g.b_pitch = b_pitch; g.a_cf = a_channels_first != 0; g.b_cf = b_channels_first != 0;
    g.M = p->cfg.num_mels; g.n_cep = p->cfg.n_cep; g.unit = p->cfg.unit_db; g.alarm = p->cfg.alarm_db;
    for (int pass = 0; pass < 2; ++pass)               // per-frame 0 ... 3 and their means (bias_b among them) for every group, then 4, 5 and the rest
        for (int b0 = 0; b0 < B; b0 += MELCMP_GROUP) {
            const int nb = B - b0 < MELCMP_GROUP ? B - b0 : MELCMP_GROUP;
            int32_t n_max = 0;
            g.b0 = b0; g.pass = pass;
            for (int r = 0; r < MELCMP_GROUP; ++r) { g.n[r] = r < nb ? frames[b0 + r] : 0; if (g.n[r] > n_max) n_max = g.n[r]; }
            if (n_max > 0) {
                hipLaunchKernelGGL(wn_melcmp_tile_kernel, dim3(cdiv(n_max, MELCMP_TF), nb), dim3(MELCMP_THREADS), p->lds_bytes, st, g);
                WN_LAUNCH_CHECK(p);
            }
            hipLaunchKernelGGL(wn_melcmp_reduce_kernel, dim3(nb), dim3(MELCMP_THREADS), 0, st, g);
            WN_LAUNCH_CHECK(p);
        }
    return WN_OK;
}

extern "C" int wn_test_melcmp_host(const wn_melcmp_config* cfg, const float* a, int32_t a_channels_first, int64_t a_pitch, const float* b, int32_t b_channels_first,
                                   int64_t b_pitch, const int32_t* frames, int32_t B, float* per_frame, int64_t out_pitch, float* summary, int32_t* marks) {
    wn_melcmp* z = nullptr;
    char msg[256];
    if (int rc = wn_melcmp_check_config(cfg, msg, sizeof msg)) WN_FAIL(z, rc, "wn_test_melcmp_host: %s", msg);
    if (int rc = wn_melcmp_check_call("wn_test_melcmp_host", cfg->max_batch ? cfg->max_batch : INT32_MAX, cfg->max_frames ? cfg->max_frames : INT32_MAX, a, a_pitch, b, b_pitch,
                                      frames, B, per_frame, out_pitch, summary, marks, msg, sizeof msg))
        WN_FAIL(z, rc, "%s", msg);
    int32_t n_max = 0;
    for (int r = 0; r < B; ++r) n_max = frames[r] > n_max ? frames[r] : n_max;
    std::vector<float> dct((size_t)cfg->n_cep * cfg->num_mels), col(cfg->num_mels), own(per_frame ? 0 : (size_t)B * 6 * n_max);
    wn_melcmp_dct_table(cfg->num_mels, cfg->n_cep, dct.data());
    wn_melcmp_host_rows(cfg, dct.data(), a, a_channels_first != 0, a_pitch, b, b_channels_first != 0, b_pitch, frames, B, per_frame ? per_frame : own.data(),
                        per_frame ? out_pitch : n_max, summary, marks, col.data());
    return WN_OK;
}
