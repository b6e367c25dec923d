// Mel analysis, the part wn_mel.hip (whole rows) and wn_mel_stream.hip (rows that arrive push by push) share: the geometry and the two tables of a
// configuration on the host, and on the device everything that follows the staging of a tile's signal span -- the windowed DFT of the tile's frames on the
// exact-fp32 matrix instruction, the power, the mel sums, level and normalisation.  A kernel stages sig[i] = y[first frame x hop - Hl + i] in LDS, zero
// outside the row, synchronises, and calls mel_core with a store functor; which tile a frame ran in, and at which row of the tile, leaves no trace in its
// bits: every (frame, bin) and (frame, mel) is its own row / column of the matrix instruction, taps ascending in bodies of 8, bins in chunks of 4 x 32, mel
// sums with bins ascending.
#pragma once
#include "wn_common.h"
#include <cmath>
#include <vector>

#define MEL_GROUP 64      // rows per launch: their lengths travel as kernel arguments (no device copy of the host array, nothing to allocate)
#define MEL_STAGE (32 * 129)      // power of 32 frames x the chunk's 128 bins, odd pitch

// What mel_core and mel_finish read from a kernel's argument struct A (wn_mel.hip's MelArgs, wn_mel_stream.hip's MelsArgs; filled by mel_core_args):
//   const float* basis, * melT;  int32_t channels_first, hop, win_pad, nchunks, ldb, num_mels, mt (= ldm / 32 mel tiles), ldm, sig_floats;
//   float kpre, pow_half;  int32_t pow_mode (0: power 2 as is, 1: power 1 sqrt, 2: powf);  float min_lin, ref_db, lo, maxabs;  int32_t norm, clip, symmetric

// ---- host: geometry and tables of a configuration
struct MelGeom {
    int NB = 0, G = 0, off = 0, win_pad = 0, MT = 0, ldb = 0, ldm = 0;
    float min_lin = 0.f;
};

static inline MelGeom mel_geom(const wn_mel_config& cfg) {
    MelGeom m;
    m.NB = 1 + cfg.n_fft / 2;
    m.G = ((m.NB + 31) / 32 + 3) / 4 * 4;
    m.off = (cfg.n_fft - cfg.win_size) / 2;
    m.win_pad = (cfg.win_size + 7) / 8 * 8;
    m.MT = (cfg.num_mels + 31) / 32;
    m.ldb = m.G * 64; m.ldm = m.MT * 32;
    m.min_lin = (float)std::pow(10.0, (double)cfg.min_level_db / 20.0);
    return m;
}

// the checks of wn_mel_create on the geometry and level fields (max_batch / max_samples are the caller's)
#define WN_MEL_FAIL(code, ...) do { if (msg && cap > 0) snprintf(msg, (size_t)cap, __VA_ARGS__); return (code); } while (0)
static inline int mel_check_geometry(const wn_mel_config* cfg, char* msg, int cap) {
    if (cfg->n_fft < 2 || cfg->n_fft % 2) WN_MEL_FAIL(WN_E_SHAPE, "n_fft (%d) must be even and >= 2", cfg->n_fft);
    if (cfg->win_size < 1 || cfg->win_size > cfg->n_fft) WN_MEL_FAIL(WN_E_SHAPE, "win_size (%d) must be in [1, n_fft = %d]", cfg->win_size, cfg->n_fft);
    if (cfg->hop_size < 1) WN_MEL_FAIL(WN_E_SHAPE, "hop_size (%d) must be >= 1", cfg->hop_size);
    if (cfg->num_mels < 1) WN_MEL_FAIL(WN_E_SHAPE, "num_mels (%d) must be >= 1", cfg->num_mels);
    if (cfg->num_mels > 128) WN_MEL_FAIL(WN_E_UNSUPPORTED, "num_mels (%d) > 128: the mel accumulator tiles are built for up to 128", cfg->num_mels);
    if (!(cfg->magnitude_power > 0.f)) WN_MEL_FAIL(WN_E_ARG, "magnitude_power (%g) must be > 0", (double)cfg->magnitude_power);
    if (cfg->signal_normalization && !(cfg->min_level_db < 0.f)) WN_MEL_FAIL(WN_E_ARG, "min_level_db (%g) must be < 0 for signal_normalization", (double)cfg->min_level_db);
    return WN_OK;
}

// LDS of a tile of FR x 32 frames: the signal span (or the mel buffer that overlays it) + the power patch
static inline size_t mel_lds(const wn_mel_config& cfg, const MelGeom& m, int FR, int* sig_floats) {
    const int64_t span = (int64_t)(FR * 32 - 1) * cfg.hop_size + m.win_pad, red = (int64_t)FR * 32 * m.ldm;
    const int64_t sf = span > red ? span : red;
    if (sf > (1 << 22)) return (size_t)1 << 30;
    if (sig_floats) *sig_floats = (int)sf;
    return (size_t)(sf + MEL_STAGE) * 4;
}

// [win_pad][G][re 32 | im 32] window x cos / -sin in double, argument reduced as integers; window = periodic Hann of win_size (scipy get_window('hann', win,
// fftbins=True)).  [32 G][32 MT] mel filters transposed, zero padded
static inline void mel_build_tables(const wn_mel_config& cfg, const MelGeom& m, const float* mel_basis, std::vector<float>* basis, std::vector<float>* melT) {
    const int n_fft = cfg.n_fft, win = cfg.win_size;
    std::vector<double> ct(n_fft), st(n_fft);
    const double two_pi = 6.283185307179586476925286766559;
    for (int i = 0; i < n_fft; ++i) { ct[i] = std::cos(two_pi * i / n_fft); st[i] = std::sin(two_pi * i / n_fft); }
    std::vector<float>& hb = *basis;
    hb.assign((size_t)m.win_pad * m.ldb, 0.0f);
    for (int k = 0; k < win; ++k) {
        const double w = 0.5 - 0.5 * std::cos(two_pi * k / win);
        for (int j = 0; j < m.NB; ++j) {
            const int idx = (int)(((int64_t)(k + m.off) * j) % n_fft);
            float* p = &hb[(size_t)k * m.ldb + (j / 32) * 64 + (j % 32)];
            p[0] = (float)(w * ct[idx]); p[32] = (float)(-w * st[idx]);
        }
    }
    std::vector<float>& hm = *melT;
    hm.assign((size_t)m.G * 32 * m.ldm, 0.0f);
    for (int q = 0; q < cfg.num_mels; ++q)
        for (int j = 0; j < m.NB; ++j) hm[(size_t)j * m.ldm + q] = mel_basis[(size_t)q * m.NB + j];
}

template <class A>
static inline void mel_core_args(const wn_mel_config& cfg, const MelGeom& m, const float* basis, const float* melT, int channels_first, int sig_floats, A* c) {
    c->basis = basis; c->melT = melT; c->channels_first = channels_first != 0;
    c->hop = cfg.hop_size; c->win_pad = m.win_pad; c->nchunks = m.G / 4; c->ldb = m.ldb;
    c->num_mels = cfg.num_mels; c->mt = m.MT; c->ldm = m.ldm; c->sig_floats = sig_floats;
    c->kpre = cfg.preemphasis; c->pow_half = 0.5f * cfg.magnitude_power;
    c->pow_mode = cfg.magnitude_power == 2.0f ? 0 : cfg.magnitude_power == 1.0f ? 1 : 2;
    c->min_lin = m.min_lin; c->ref_db = cfg.ref_level_db; c->lo = cfg.min_level_db; c->maxabs = cfg.max_abs_value;
    c->norm = cfg.signal_normalization != 0; c->clip = cfg.allow_clipping != 0; c->symmetric = cfg.symmetric_mels != 0;
}

// ---- device
// x[s] - k_pre * prev: two of the three separately rounded operations of y[s] = gain * (x[s] - k_pre * x[s - 1]) (what numpy does on float32 arrays)
static __device__ __forceinline__ float mel_preem_pair(float xs, float prev, float kpre) { return __fsub_rn(xs, __fmul_rn(kpre, prev)); }
static __device__ __forceinline__ float mel_preem(const float* __restrict__ x, int64_t s, float kpre) { return mel_preem_pair(x[s], s > 0 ? x[s - 1] : 0.0f, kpre); }

// audio.py:257-270: S = 20 log10(max(min_level, M)) - ref_level_db, then _normalize (without its assert)
template <class A>
static __device__ __forceinline__ float mel_finish(const A& a, float M) {
    const float S = 20.0f * log10f(fmaxf(a.min_lin, M)) - a.ref_db;
    if (!a.norm) return S;
    const float u = (S - a.lo) / (-a.lo);
    float v = a.symmetric ? (2.0f * a.maxabs) * u - a.maxabs : a.maxabs * u;
    if (a.clip) v = fminf(fmaxf(v, a.symmetric ? -a.maxabs : 0.0f), a.maxabs);
    return v;
}

// lds: the staged span sig[0 ... sig_floats) (complete and visible: the caller has synchronised), then MEL_STAGE floats.  nf: how many of the tile's TF = 32 FR
// frames exist; store(f, m, v) receives every (frame of the tile, mel): the finished value for f < nf, `pad` (an all-zero signal's value) for the rest.
template <int FR, class A, class Store>
static __device__ __forceinline__ void mel_core(const A& a, float* lds, int nf, float pad, Store&& store) {
    constexpr int TF = FR * 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    float* sig = lds;
    float* stage = lds + a.sig_floats;
    f32x16_t macc[FR];      // mel tile (frame subtile i, mels 32 wave ... 32 wave + 31): waves >= mt hold none
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) macc[i][r] = 0.0f;
    const float* sp = sig + l31 * a.hop + lh;      // A operand of frame subtile i, taps k / k + 1: lane l holds frame 32 i + l % 32, tap k + l / 32
    for (int c = 0; c < a.nchunks; ++c) {
        const int g = c * 4 + wave;                // this wave's bin group (the basis is padded to 4 nchunks groups: no divergence)
        f32x16_t re[FR], im[FR];
#pragma unroll
        for (int i = 0; i < FR; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) { re[i][r] = 0.0f; im[i][r] = 0.0f; }
        const float* bp = a.basis + (size_t)lh * a.ldb + g * 64 + l31;      // B operand: lane l holds basis[k + l / 32][column l % 32]
        // taps in bodies of 8 (win_pad is a multiple of 8, zero rows beyond win_size): the basis loads of the next body are in flight while this one is multiplied
        float nre[4], nim[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { nre[u] = bp[(size_t)(2 * u) * a.ldb]; nim[u] = bp[(size_t)(2 * u) * a.ldb + 32]; }
        for (int k0 = 0; k0 < a.win_pad; k0 += 8) {
            float bre[4], bim[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { bre[u] = nre[u]; bim[u] = nim[u]; }
            if (k0 + 8 < a.win_pad) {
#pragma unroll
                for (int u = 0; u < 4; ++u) { nre[u] = bp[(size_t)(k0 + 8 + 2 * u) * a.ldb]; nim[u] = bp[(size_t)(k0 + 8 + 2 * u) * a.ldb + 32]; }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int i = 0; i < FR; ++i) {
                    const float av = sp[i * 32 * a.hop + k0 + 2 * u];
                    re[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bre[u], re[i], 0, 0, 0);
                    im[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bim[u], im[i], 0, 0, 0);
                }
        }
#pragma unroll
        for (int i = 0; i < FR; ++i) {
            // accumulator register r of lane l is (frame 8 (r / 4) + 4 (l / 32) + r % 4, bin l % 32): through the wave's LDS patch into the A layout
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float p = re[i][r] * re[i][r] + im[i][r] * im[i][r];
                if (a.pow_mode == 1) p = sqrtf(p); else if (a.pow_mode == 2) p = powf(p, a.pow_half);
                stage[((r >> 2) * 8 + lh * 4 + (r & 3)) * 129 + wave * 32 + l31] = p;
            }
            __syncthreads();
            if (wave < a.mt) {      // [32 frames, 128 bins of this chunk] x [128, 32 mels]: bins ascending, chunks ascending -- a fixed order
                const float* mp = a.melT + (size_t)(c * 128 + lh) * a.ldm + wave * 32 + l31;
#pragma unroll 8
                for (int kk = 0; kk < 128; kk += 2)
                    macc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(stage[l31 * 129 + kk + lh], mp[(size_t)kk * a.ldm], macc[i], 0, 0, 0);
            }
            __syncthreads();
        }
    }
    // mel sums through LDS to the threads that finish and store them (red overlays the signal span, which is dead now)
    float* red = lds;
    if (wave < a.mt) {
#pragma unroll
        for (int i = 0; i < FR; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) red[(i * 32 + (r >> 2) * 8 + lh * 4 + (r & 3)) * a.ldm + wave * 32 + l31] = macc[i][r];
    }
    __syncthreads();
    for (int e = tid; e < TF * a.num_mels; e += 256) {
        int f, m;
        if (a.channels_first) { f = e % TF; m = e / TF; } else { f = e / a.num_mels; m = e % a.num_mels; }
        store(f, m, f < nf ? mel_finish(a, red[f * a.ldm + m]) : pad);
    }
}
