// Alignment check arithmetic shared by the device kernels of wn_align.hip, the host hooks wn_test_align_host / wn_test_align_dp_host and the stand-alone
// host program tests/host/align_main.cpp: a frame's cepstra, the cost of a frame pair, the band, one cell of the recurrence with its tie order, the
// back-trace, the summary, the validation of a configuration and of a call, and one whole call on the host.  Everything here is written once and
// runs on either side, so the hooks give the device's bits.
//
// The arithmetic (all float32, every step rounded on its own):
//   cepstra     u[m] = unit_db * x[m];  c[k] = sum_m D[k][m] u[m], k = 1 ... n_cep: one accumulator from 0, c = fma(D[k][m], u[m], c), m ascending.  D is
//               the orthonormal DCT-II table of the reconstruction check (wn_melcmp_dct_table: double on the host, rounded once); coefficient 0 is left
//               out, so a level offset between the two signals does not enter.
//   cell cost   cost(i, j) = sqrt(0.5 * sum_k (ca[i][k] - cb[j][k])^2): e = ca - cb, acc = fma(e, e, acc) from 0, k ascending, one product by 0.5, one
//               correctly rounded square root -- the MCD of the frame pair in dB.  The direct difference on purpose, never |a|^2 + |b|^2 - 2 a.b: all
//               terms are non-negative and every cell has a relative bound.
//   band        cell (i, j) is admissible iff band == 0 or |i Fb - j Fa| <= band * max(Fa, Fb), in int64.  Per row i that is the interval
//               j = ceil((i Fb - W) / Fa) ... floor((i Fb + W) / Fa), W = band max(Fa, Fb), cut to [0, Fb - 1] (align_span).  For band >= 1 the
//               staircase j = floor(i Fb / Fa) (Fa >= Fb; its transpose i = floor(j Fa / Fb) otherwise) lies inside the band: |i Fb - j Fa| < Fa <= W,
//               it starts at (0, 0), ends at (Fa - 1, Fb - 1) and moves by steps of the recurrence, so the two corners are always connected.
//               Inadmissible cells count as +inf.
//   recurrence  Dm(0, 0) = cost(0, 0);  Dm(i, j) = cost(i, j) + min(Dm(i-1, j-1), Dm(i-1, j), Dm(i, j-1)): one rounded add, the min is exact.  The
//               predecessor is the smallest candidate, ties to the first in the order diagonal, (i-1, j), (i, j-1); candidates outside the matrix or
//               the band are never chosen; an admissible cell without any candidate is +inf with no predecessor (align_cell).
//   path        back-trace from (Fa-1, Fb-1) to (0, 0) along the stored predecessors, at most Fa + Fb - 2 steps; at i == 0 the step is (i, j-1), at
//               j == 0 it is (i-1, j), a cell without predecessor steps diagonally: whatever the values (NaN included), the indices stay inside the
//               matrix and the loop ends at (0, 0).  Delivered in FORWARD order.
//   summary     Fa, Fb, n_path, total = Dm(Fa-1, Fb-1), mcd_dtw = (sum of the path's costs as doubles in path order) / n_path, the share of
//               non-diagonal steps (0 for a one-cell path), max_p |i_p Fb - j_p Fa| / max(Fa, Fb) (int64, divided in double); each rounded to float32 once.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../../include/wavenet_mi355.h"
#include "wn_melcmp.h"

#define ALIGN_T 64                    // block height and width: one lane per row of a block
#define ALIGN_WAVES 4                 // blocks of one block anti-diagonal in flight per workgroup
#define ALIGN_THREADS 256             // = ALIGN_T * ALIGN_WAVES
#define ALIGN_TP 66                   // pitch (floats) of a block's rows in LDS: lane l reads column s - l at 65 l + s, distinct banks for 32 consecutive lanes
#define ALIGN_GROUP 32                // rows per launch
#define ALIGN_MAX_FRAMES 4096         // per side: the block boundaries (3 x 4096 floats) and the back-trace's path (8191 x 12 bytes) live in LDS
#define ALIGN_MAX_CELLS (1ll << 27)   // max_batch x max_frames_a x max_frames_b: 512 MiB of cost matrix, 32 MiB of directions
#define ALIGN_MAX_BAND (1 << 20)
#define ALIGN_NONE 3                  // direction codes: 0 diagonal, 1 (i-1, j), 2 (i, j-1), 3 no predecessor

__host__ __device__ __forceinline__ float align_unit(float unit, float x) {
#pragma clang fp contract(off)
    return unit * x;
}
// one coefficient: row = D[k], u = the frame's scaled channels at a pitch of su floats
__host__ __device__ __forceinline__ float align_cep(const float* row, const float* u, int64_t su, int M) {
#pragma clang fp contract(off)
    float c = 0.0f;
    for (int m = 0; m < M; ++m) c = __builtin_fmaf(row[m], u[(int64_t)m * su], c);
    return c;
}
__host__ __device__ __forceinline__ float align_cost(const float* ca, const float* cb, int n_cep) {
#pragma clang fp contract(off)
    float acc = 0.0f;
    for (int k = 0; k < n_cep; ++k) { const float e = ca[k] - cb[k]; acc = __builtin_fmaf(e, e, acc); }
    return sqrtf(0.5f * acc);
}
// admissible columns of row i: [lo, hi], empty (lo > hi) for a row outside the matrix
__host__ __device__ __forceinline__ void align_span(int64_t i, int32_t Fa, int32_t Fb, int32_t band, int32_t* lo, int32_t* hi) {
    if (i < 0 || i >= Fa) { *lo = 1; *hi = 0; return; }
    if (band == 0) { *lo = 0; *hi = Fb - 1; return; }
    const int64_t W = (int64_t)band * (Fa > Fb ? Fa : Fb), c = i * (int64_t)Fb;
    const int64_t l = c - W <= 0 ? 0 : (c - W + Fa - 1) / Fa;
    int64_t h = (c + W) / Fa;
    if (h > Fb - 1) h = Fb - 1;
    *lo = (int32_t)l; *hi = (int32_t)h;
}
__host__ __device__ __forceinline__ bool align_in(int32_t j, int32_t lo, int32_t hi) { return j >= lo && j <= hi; }
// one cell: d, u, l the candidates Dm(i-1, j-1), Dm(i-1, j), Dm(i, j-1) and whether each is inside the matrix and the band
__host__ __device__ __forceinline__ float align_cell(float cost, float d, float u, float l, bool vd, bool vu, bool vl, bool origin, bool adm, int* dir) {
#pragma clang fp contract(off)
    float best = INFINITY; int w = ALIGN_NONE;
    if (vd) { best = d; w = 0; }
    if (vu && (w == ALIGN_NONE || u < best)) { best = u; w = 1; }
    if (vl && (w == ALIGN_NONE || l < best)) { best = l; w = 2; }
    *dir = adm ? w : ALIGN_NONE;
    if (!adm) return INFINITY;
    if (origin) return cost;
    return w == ALIGN_NONE ? INFINITY : cost + best;
}
// words of 16 directions, 2 bits each, per row of the matrix
__host__ __device__ __forceinline__ int64_t align_words(int64_t Fb) { return (Fb + 15) / 16; }

// the path in REVERSE order into pi / pj / pc (cell and its cost), each of Fa + Fb - 1 entries; returns its length
__host__ __device__ inline int align_backtrace(const uint32_t* dirs, int64_t wpr, const float* cost, int64_t cpitch, int Fa, int Fb, int32_t* pi, int32_t* pj, float* pc) {
    int i = Fa - 1, j = Fb - 1, n = 0;
    const int cap = Fa + Fb - 2;
    for (int step = 0; step < cap && (i > 0 || j > 0); ++step) {
        pi[n] = i; pj[n] = j; pc[n] = cost[(int64_t)i * cpitch + j]; ++n;
        int d = (int)((dirs[(int64_t)i * wpr + (j >> 4)] >> (2 * (j & 15))) & 3u);
        if (i == 0) d = 2; else if (j == 0) d = 1; else if (d == ALIGN_NONE) d = 0;
        if (d != 2) --i;
        if (d != 1) --j;
    }
    pi[n] = 0; pj[n] = 0; pc[n] = cost[0]; ++n;
    return n;
}
// sm[7] of a row from its reversed path
__host__ __device__ inline void align_summary(const int32_t* pi, const int32_t* pj, const float* pc, int n, int Fa, int Fb, float total, float* sm) {
    double s = 0.0;
    int64_t dev = 0; int nondiag = 0;
    for (int p = n - 1; p >= 0; --p) {
        s += (double)pc[p];
        int64_t e = (int64_t)pi[p] * Fb - (int64_t)pj[p] * Fa;
        if (e < 0) e = -e;
        if (e > dev) dev = e;
        if (p > 0 && (pi[p - 1] == pi[p] || pj[p - 1] == pj[p])) ++nondiag;
    }
    sm[0] = (float)Fa; sm[1] = (float)Fb; sm[2] = (float)n; sm[3] = total;
    sm[4] = (float)(s / (double)n);
    sm[5] = n > 1 ? (float)((double)nondiag / (double)(n - 1)) : 0.0f;
    sm[6] = (float)((double)dev / (double)(Fa > Fb ? Fa : Fb));
}
// the outputs of forward position p of a path of n cells held in reverse
__host__ __device__ __forceinline__ void align_emit(const int32_t* pi, const int32_t* pj, int n, int p, int32_t* path, int64_t path_pitch, int32_t* map_ab, int32_t* map_ba) {
    const int q = n - 1 - p, i = pi[q], j = pj[q];
    if (path) { path[p] = i; path[path_pitch + p] = j; }
    if (map_ab && (q == 0 || pi[q - 1] != i)) map_ab[i] = j;
    if (map_ba && (q == 0 || pj[q - 1] != j)) map_ba[j] = i;
}

// ---- host: one whole call in the device's order (the hooks and align_main.cpp), and the validation every entry point runs before any device call
static inline float align_host_at(const float* x, int cf, int64_t pitch, int M, int64_t row, int f, int m) {
    return cf ? x[(row * M + m) * pitch + f] : x[(row * pitch + f) * M + m];
}
// cepstra of one row's F frames: out [F][n_cep]; u: scratch of M floats
static inline void align_host_cepstra(float unit, const float* dct, const float* x, int cf, int64_t pitch, int M, int n_cep, int64_t row, int F, float* out, float* u) {
    for (int f = 0; f < F; ++f) {
        for (int m = 0; m < M; ++m) u[m] = align_unit(unit, align_host_at(x, cf, pitch, M, row, f, m));
        for (int k = 0; k < n_cep; ++k) out[(size_t)f * n_cep + k] = align_cep(dct + (size_t)k * M, u, 1, M);
    }
}
// recurrence over a cost matrix [Fa][cpitch]: dm [Fa][Fb], dirs [Fa][align_words(Fb)] (zeroed here)
static inline void align_host_dp(const float* cost, int64_t cpitch, int Fa, int Fb, int band, float* dm, uint32_t* dirs) {
    const int64_t wpr = align_words(Fb);
    for (int64_t w = 0; w < (int64_t)Fa * wpr; ++w) dirs[w] = 0;
    int32_t lo_u = 1, hi_u = 0;
    for (int i = 0; i < Fa; ++i) {
        int32_t lo, hi;
        align_span(i, Fa, Fb, band, &lo, &hi);
        for (int j = 0; j < Fb; ++j) {
            const bool vu = i > 0 && align_in(j, lo_u, hi_u), vd = i > 0 && j > 0 && align_in(j - 1, lo_u, hi_u), vl = j > 0 && align_in(j - 1, lo, hi);
            int dir;
            dm[(size_t)i * Fb + j] = align_cell(cost[(int64_t)i * cpitch + j], vd ? dm[(size_t)(i - 1) * Fb + j - 1] : 0.0f, vu ? dm[(size_t)(i - 1) * Fb + j] : 0.0f,
                                                vl ? dm[(size_t)i * Fb + j - 1] : 0.0f, vd, vu, vl, i == 0 && j == 0, align_in(j, lo, hi), &dir);
            dirs[(int64_t)i * wpr + (j >> 4)] |= (uint32_t)dir << (2 * (j & 15));
        }
        lo_u = lo; hi_u = hi;
    }
}
// back-trace, summary and the optional outputs of one row (pointers already at the row)
static inline void align_host_finish(const float* cost, int64_t cpitch, const float* dm, const uint32_t* dirs, int Fa, int Fb, int32_t* path, int64_t path_pitch,
                                     int32_t* map_ab, int32_t* map_ba, float* sm) {
    std::vector<int32_t> pi((size_t)Fa + Fb - 1), pj((size_t)Fa + Fb - 1);
    std::vector<float> pc((size_t)Fa + Fb - 1);
    const int n = align_backtrace(dirs, align_words(Fb), cost, cpitch, Fa, Fb, pi.data(), pj.data(), pc.data());
    align_summary(pi.data(), pj.data(), pc.data(), n, Fa, Fb, dm[(size_t)(Fa - 1) * Fb + Fb - 1], sm);
    for (int p = 0; p < n; ++p) align_emit(pi.data(), pj.data(), n, p, path, path_pitch, map_ab, map_ba);
}
// every row of a call on mels; cep_a [B, Fa_max, n_cep], cep_b [B, Fb_max, n_cep], cost and dm [B, Fa_max, Fb_max] are optional copies of the stages
static inline void wn_align_host_rows(const wn_align_config* cfg, const float* a, int a_cf, int64_t a_pitch, const float* b, int b_cf, int64_t b_pitch, const int32_t* fa,
                                      const int32_t* fb, int32_t B, int32_t* path, int64_t path_pitch, int32_t* map_ab, int64_t map_a_pitch, int32_t* map_ba, int64_t map_b_pitch,
                                      float* summary, float* cep_a, float* cep_b, float* cost_out, float* dm_out) {
    const int M = cfg->num_mels, K = cfg->n_cep;
    int32_t Fa_max = 0, Fb_max = 0;
    for (int r = 0; r < B; ++r) { if (fa[r] > Fa_max) Fa_max = fa[r]; if (fb[r] > Fb_max) Fb_max = fb[r]; }
    std::vector<float> dct((size_t)K * M), u(M);
    wn_melcmp_dct_table(M, K, dct.data());
    for (int64_t r = 0; r < B; ++r) {
        const int Fa = fa[r], Fb = fb[r];
        std::vector<float> ca((size_t)Fa * K), cb((size_t)Fb * K), cost((size_t)Fa * Fb), dm((size_t)Fa * Fb);
        std::vector<uint32_t> dirs((size_t)Fa * align_words(Fb));
        align_host_cepstra(cfg->unit_db, dct.data(), a, a_cf, a_pitch, M, K, r, Fa, ca.data(), u.data());
        align_host_cepstra(cfg->unit_db, dct.data(), b, b_cf, b_pitch, M, K, r, Fb, cb.data(), u.data());
        for (int i = 0; i < Fa; ++i)
            for (int j = 0; j < Fb; ++j) cost[(size_t)i * Fb + j] = align_cost(ca.data() + (size_t)i * K, cb.data() + (size_t)j * K, K);
        align_host_dp(cost.data(), Fb, Fa, Fb, cfg->band, dm.data(), dirs.data());
        align_host_finish(cost.data(), Fb, dm.data(), dirs.data(), Fa, Fb, path ? path + r * 2 * path_pitch : nullptr, path_pitch, map_ab ? map_ab + r * map_a_pitch : nullptr,
                          map_ba ? map_ba + r * map_b_pitch : nullptr, summary + r * 7);
        if (cep_a) for (size_t t = 0; t < ca.size(); ++t) cep_a[(size_t)r * Fa_max * K + t] = ca[t];
        if (cep_b) for (size_t t = 0; t < cb.size(); ++t) cep_b[(size_t)r * Fb_max * K + t] = cb[t];
        for (int i = 0; i < Fa; ++i)
            for (int j = 0; j < Fb; ++j) {
                if (cost_out) cost_out[((size_t)r * Fa_max + i) * Fb_max + j] = cost[(size_t)i * Fb + j];
                if (dm_out) dm_out[((size_t)r * Fa_max + i) * Fb_max + j] = dm[(size_t)i * Fb + j];
            }
    }
}
// every row of a call on a caller's cost matrix [B, Fa_max, Fb_max]
static inline void wn_align_host_dp_rows(int band, const float* cost, int32_t Fa_max, int32_t Fb_max, const int32_t* fa, const int32_t* fb, int32_t B, int32_t* path,
                                         int64_t path_pitch, int32_t* map_ab, int64_t map_a_pitch, int32_t* map_ba, int64_t map_b_pitch, float* summary, float* dm_out) {
    for (int64_t r = 0; r < B; ++r) {
        const int Fa = fa[r], Fb = fb[r];
        const float* c = cost + (size_t)r * Fa_max * Fb_max;
        std::vector<float> dm((size_t)Fa * Fb);
        std::vector<uint32_t> dirs((size_t)Fa * align_words(Fb));
        align_host_dp(c, Fb_max, Fa, Fb, band, dm.data(), dirs.data());
        align_host_finish(c, Fb_max, dm.data(), dirs.data(), Fa, Fb, path ? path + r * 2 * path_pitch : nullptr, path_pitch, map_ab ? map_ab + r * map_a_pitch : nullptr,
                          map_ba ? map_ba + r * map_b_pitch : nullptr, summary + r * 7);
        if (dm_out)
            for (int i = 0; i < Fa; ++i)
                for (int j = 0; j < Fb; ++j) dm_out[((size_t)r * Fa_max + i) * Fb_max + j] = dm[(size_t)i * Fb + j];
    }
}

#define WN_ALIGN_FAIL(code, ...) do { if (msg && cap > 0) snprintf(msg, (size_t)cap, __VA_ARGS__); return (code); } while (0)

static inline int wn_align_check_config(const wn_align_config* cfg, char* msg, int cap) {
    if (!cfg) WN_ALIGN_FAIL(WN_E_ARG, "null configuration");
    if (cfg->abi_version != WN_ABI_VERSION) WN_ALIGN_FAIL(WN_E_ARG, "abi_version %d != %d", cfg->abi_version, WN_ABI_VERSION);
    if (cfg->num_mels < 1 || cfg->num_mels > MELCMP_MAX_MELS) WN_ALIGN_FAIL(WN_E_ARG, "num_mels (%d) must be 1 ... %d", cfg->num_mels, MELCMP_MAX_MELS);
    if (cfg->n_cep < 1 || cfg->n_cep > cfg->num_mels - 1) WN_ALIGN_FAIL(WN_E_ARG, "n_cep (%d) must be 1 ... num_mels - 1 = %d", cfg->n_cep, cfg->num_mels - 1);
    if (!(cfg->unit_db > 0.0f) || isinf(cfg->unit_db)) WN_ALIGN_FAIL(WN_E_ARG, "unit_db (%g) must be finite and > 0", (double)cfg->unit_db);
    if (cfg->band < 0 || cfg->band > ALIGN_MAX_BAND) WN_ALIGN_FAIL(WN_E_ARG, "band (%d) must be 0 ... %d", cfg->band, ALIGN_MAX_BAND);
    if (cfg->max_batch < 0) WN_ALIGN_FAIL(WN_E_ARG, "max_batch (%d) must be >= 0", cfg->max_batch);
    if (cfg->max_frames_a < 0 || cfg->max_frames_b < 0) WN_ALIGN_FAIL(WN_E_ARG, "max_frames_a (%d) and max_frames_b (%d) must be >= 0", cfg->max_frames_a, cfg->max_frames_b);
    if (cfg->max_batch > 0 && (cfg->max_frames_a < 1 || cfg->max_frames_b < 1)) WN_ALIGN_FAIL(WN_E_ARG, "max_frames_a and max_frames_b must be >= 1 with max_batch > 0");
    return WN_OK;
}
// the reserve a handle may ask for
static inline int wn_align_check_reserve(const wn_align_config* cfg, char* msg, int cap) {
    if (cfg->max_frames_a > ALIGN_MAX_FRAMES || cfg->max_frames_b > ALIGN_MAX_FRAMES)
        WN_ALIGN_FAIL(WN_E_UNSUPPORTED, "max_frames_a (%d) and max_frames_b (%d) must not exceed %d", cfg->max_frames_a, cfg->max_frames_b, ALIGN_MAX_FRAMES);
    if ((int64_t)cfg->max_batch * cfg->max_frames_a * cfg->max_frames_b > ALIGN_MAX_CELLS)
        WN_ALIGN_FAIL(WN_E_UNSUPPORTED, "max_batch x max_frames_a x max_frames_b (%lld cells) exceeds the reserve limit of %lld", (long long)cfg->max_batch * cfg->max_frames_a * cfg->max_frames_b,
                      (long long)ALIGN_MAX_CELLS);
    return WN_OK;
}
// the rows and outputs of one call (wn_align_run and wn_test_align_dp alike); argument errors first, then shapes
static inline int wn_align_check_rows(const char* who, int32_t max_batch, int32_t max_a, int32_t max_b, const int32_t* fa, const int32_t* fb, int32_t B, const int32_t* path,
                                      int64_t path_pitch, const int32_t* map_ab, int64_t map_a_pitch, const int32_t* map_ba, int64_t map_b_pitch, const float* summary,
                                      int32_t* Fa_max, int32_t* Fb_max, char* msg, int cap) {
    if (!fa || !fb || !summary) WN_ALIGN_FAIL(WN_E_ARG, "%s: null argument", who);
    if (B < 1) WN_ALIGN_FAIL(WN_E_ARG, "%s: B (%d) must be >= 1", who, B);
    int32_t na = 0, nb = 0; int64_t np = 0;
    for (int r = 0; r < B; ++r) {
        if (fa[r] < 1) WN_ALIGN_FAIL(WN_E_ARG, "%s: frames_a[%d] = %d must be >= 1", who, r, fa[r]);
        if (fb[r] < 1) WN_ALIGN_FAIL(WN_E_ARG, "%s: frames_b[%d] = %d must be >= 1", who, r, fb[r]);
        if (fa[r] > na) na = fa[r];
        if (fb[r] > nb) nb = fb[r];
        if ((int64_t)fa[r] + fb[r] - 1 > np) np = (int64_t)fa[r] + fb[r] - 1;
    }
    if (B > max_batch) WN_ALIGN_FAIL(WN_E_SHAPE, "%s: B (%d) > max_batch = %d", who, B, max_batch);
    if (na > max_a) WN_ALIGN_FAIL(WN_E_SHAPE, "%s: the longest row of a (%d frames) > max_frames_a = %d", who, na, max_a);
    if (nb > max_b) WN_ALIGN_FAIL(WN_E_SHAPE, "%s: the longest row of b (%d frames) > max_frames_b = %d", who, nb, max_b);
    if (path && path_pitch < np) WN_ALIGN_FAIL(WN_E_SHAPE, "%s: path_pitch (%lld) < the longest possible path (%lld)", who, (long long)path_pitch, (long long)np);
    if (map_ab && map_a_pitch < na) WN_ALIGN_FAIL(WN_E_SHAPE, "%s: map_a_pitch (%lld) < the longest row of a (%d)", who, (long long)map_a_pitch, na);
    if (map_ba && map_b_pitch < nb) WN_ALIGN_FAIL(WN_E_SHAPE, "%s: map_b_pitch (%lld) < the longest row of b (%d)", who, (long long)map_b_pitch, nb);
    *Fa_max = na; *Fb_max = nb;
    return WN_OK;
}
static inline int wn_align_check_call(const char* who, int32_t max_batch, int32_t max_a, int32_t max_b, const float* a, int64_t a_pitch, const float* b, int64_t b_pitch,
                                      const int32_t* fa, const int32_t* fb, int32_t B, const int32_t* path, int64_t path_pitch, const int32_t* map_ab, int64_t map_a_pitch,
                                      const int32_t* map_ba, int64_t map_b_pitch, const float* summary, char* msg, int cap) {
    if (!a || !b) WN_ALIGN_FAIL(WN_E_ARG, "%s: null argument", who);
    int32_t na = 0, nb = 0;
    if (int rc = wn_align_check_rows(who, max_batch, max_a, max_b, fa, fb, B, path, path_pitch, map_ab, map_a_pitch, map_ba, map_b_pitch, summary, &na, &nb, msg, cap)) return rc;
    if (a_pitch < na) WN_ALIGN_FAIL(WN_E_SHAPE, "%s: a_pitch (%lld) < the longest row of a (%d)", who, (long long)a_pitch, na);
    if (b_pitch < nb) WN_ALIGN_FAIL(WN_E_SHAPE, "%s: b_pitch (%lld) < the longest row of b (%d)", who, (long long)b_pitch, nb);
    return WN_OK;
}
