// Alignment check: dynamic time warping of two mel-spectrograms over their cepstral distance, MCD along the path, the path and the frame maps
// (wn_align_* of include/wavenet_mi355.h).  The case the reconstruction and pitch checks cannot score: a generated utterance against a recording of
// another length and timing.  Four launches per group of 32 rows, all arithmetic in wn_align.h, shared with the host hooks:
//   cepstra     a workgroup stages 64 frames x num_mels of one input through LDS (coalesced in either layout, scaled by unit_db on the way), lane f of
//               every wavefront owns frame f and walks its channels; the coefficients k = 1 + q, 5 + q, ... go to wavefront q.  Both inputs in one grid.
//   cost        fully parallel: a workgroup stages the cepstra of 64 frames of a and 64 of b in LDS (pitch odd) and fills a 64 x 64 block of the cost
//               matrix, lane = column, so every store is coalesced.  This is where the arithmetic is; it uses the whole chip.
//   recurrence  ONE workgroup per row of the batch, so nothing ever waits across workgroups.  The matrix is cut into 64 x 64 blocks; the blocks of one
//               block anti-diagonal are independent and go to the four wavefronts in ascending block row, a round of four at a time.  A wavefront
//               loads its block of costs into LDS (coalesced), then walks it skewed: at step s lane l holds cell (i0 + l, j0 + s - l).  The left
//               neighbour is the lane's own previous value, the upper one the previous value of lane l - 1 (one lane shift), the diagonal one that
//               shifted value a step later.  Lane 0 takes the upper row from the bottom row of the block above, and a lane's first column takes its
//               left from the last column of the block to the left: both boundaries live in LDS (the bottom rows double-buffered by block-row parity,
//               so that the corner Dm(i0 - 1, j0 - 1) survives until it is read).  Every round reads its boundaries, passes a barrier, computes and
//               writes its boundaries, passes a barrier: no block reads what a block of the same round writes.  Directions leave at 2 bits per cell,
//               one 32-bit store per lane and 16 columns.
//   back-trace  one workgroup per row: one lane follows the directions from the corner (bounded loop, clamped indices) and keeps the reversed path and
//               its costs in LDS, sums the summary, then all lanes write the forward path and the two maps.
#include "wn_align.h"
#include "wn_common.h"

struct wn_align {
    wn_align_config cfg;
    std::string err;
    size_t lds_cep = 0, lds_cost = 0, lds_dp = 0, lds_trace = 0;
    int32_t cap_a = 0, cap_b = 0;      // max_frames_a / max_frames_b rounded up to whole blocks
    bool store_dm = false;
    DevBuf<float> dct;                 // [n_cep, num_mels] rows 1 ... n_cep of D
    DevBuf<float> cep_a, cep_b;        // [max_batch, max_frames_*, n_cep]
    DevBuf<float> cost;                // [max_batch, max_frames_a, max_frames_b]
    DevBuf<uint32_t> dirs;             // [max_batch, max_frames_a, align_words(max_frames_b)]
    DevBuf<float> total;               // [max_batch] Dm(Fa - 1, Fb - 1)
    DevBuf<float> dm;                  // [max_batch, max_frames_a, max_frames_b], only after wn_test_align_store_matrix
};

struct AlignArgs {
    const float* a; const float* b; const float* dct; float* cep_a; float* cep_b;
    const float* cost_in; float* cost; uint32_t* dirs; float* dm; float* total;
    int32_t* path; int32_t* map_ab; int32_t* map_ba; float* summary;
    int64_t a_pitch, b_pitch, path_pitch, map_a_pitch, map_b_pitch;
    int64_t cost_row, cost_pitch;      // element (r, i, j) of the cost matrix the recurrence reads: cost_in[r * cost_row + i * cost_pitch + j]
    int32_t a_cf, b_cf, M, n_cep, band, b0, max_a, max_b, cap_a, cap_b;
    float unit;
    int32_t fa[ALIGN_GROUP], fb[ALIGN_GROUP];
};

// blockIdx.z: 0 the frames of a, 1 of b
__global__ __launch_bounds__(ALIGN_THREADS) void wn_align_cep_kernel(const AlignArgs g) {
    extern __shared__ float lds[];     // tile [64][M | 1], dct [n_cep][M]
    const int side = blockIdx.z, r = blockIdx.y, n = side ? g.fb[r] : g.fa[r], f0 = blockIdx.x * ALIGN_T;
    if (f0 >= n) return;               // block-uniform: no barrier has been reached
    const int tid = threadIdx.x, M = g.M, MP = melcmp_tile_pitch(M), nf = n - f0 < ALIGN_T ? n - f0 : ALIGN_T;
    const int64_t row = g.b0 + r, pitch = side ? g.b_pitch : g.a_pitch;
    const float* x = side ? g.b : g.a;
    const int cf = side ? g.b_cf : g.a_cf;
    float* tile = lds;
    float* dct = tile + ALIGN_T * MP;
    for (int i = tid; i < g.n_cep * M; i += ALIGN_THREADS) dct[i] = g.dct[i];
    if (cf) {                          // [B, M, pitch]: 64 consecutive frames of one channel per wavefront
        const int f = tid % ALIGN_T;
        if (f < nf) {
            const float* src = x + row * M * pitch + f0 + f;
            for (int m = tid / ALIGN_T; m < M; m += ALIGN_WAVES) tile[f * MP + m] = align_unit(g.unit, src[(int64_t)m * pitch]);
        }
    } else {                           // [B, pitch, M]: the tile's nf x M floats are one contiguous run
        const float* src = x + (row * pitch + f0) * M;
        for (int i = tid; i < nf * M; i += ALIGN_THREADS) tile[(i / M) * MP + i % M] = align_unit(g.unit, src[i]);
    }
    __syncthreads();
    const int f = tid % ALIGN_T, q = tid / ALIGN_T;
    if (f >= nf) return;
    float* out = (side ? g.cep_b : g.cep_a) + (row * (side ? g.max_b : g.max_a) + f0 + f) * g.n_cep;
    for (int k = q; k < g.n_cep; k += ALIGN_WAVES) out[k] = align_cep(dct + k * M, tile + f * MP, 1, M);
}

__global__ __launch_bounds__(ALIGN_THREADS) void wn_align_cost_kernel(const AlignArgs g) {
    extern __shared__ float lds[];     // ca [64][n_cep | 1], cb [64][n_cep | 1]
    const int r = blockIdx.z, Fa = g.fa[r], Fb = g.fb[r], i0 = blockIdx.y * ALIGN_T, j0 = blockIdx.x * ALIGN_T;
    if (i0 >= Fa || j0 >= Fb) return;  // block-uniform
    const int tid = threadIdx.x, K = g.n_cep, KP = K | 1;
    const int ni = Fa - i0 < ALIGN_T ? Fa - i0 : ALIGN_T, nj = Fb - j0 < ALIGN_T ? Fb - j0 : ALIGN_T;
    const int64_t row = g.b0 + r;
    float* ca = lds;
    float* cb = ca + ALIGN_T * KP;
    const float* sa = g.cep_a + (row * g.max_a + i0) * K;      // ni x K and nj x K floats, each one contiguous run
    const float* sb = g.cep_b + (row * g.max_b + j0) * K;
    for (int t = tid; t < ni * K; t += ALIGN_THREADS) ca[(t / K) * KP + t % K] = sa[t];
    for (int t = tid; t < nj * K; t += ALIGN_THREADS) cb[(t / K) * KP + t % K] = sb[t];
    __syncthreads();
    const int j = tid % ALIGN_T;
    if (j >= nj) return;
    float* out = g.cost + (row * g.max_a + i0) * g.max_b + j0 + j;
    for (int i = tid / ALIGN_T; i < ni; i += ALIGN_WAVES) out[(int64_t)i * g.max_b] = align_cost(ca + i * KP, cb + j * KP, K);
}

__global__ __launch_bounds__(ALIGN_THREADS) void wn_align_dp_kernel(const AlignArgs g) {
    extern __shared__ float lds[];     // tiles [4][64][ALIGN_TP], rowb [2][cap_b], colb [cap_a]
    const int r = blockIdx.x, Fa = g.fa[r], Fb = g.fb[r];
    const int64_t row = g.b0 + r;
    const int tid = threadIdx.x, wave = tid / ALIGN_T, l = tid % ALIGN_T;
    const int nbi = (Fa + ALIGN_T - 1) / ALIGN_T, nbj = (Fb + ALIGN_T - 1) / ALIGN_T;
    float* tile = lds + wave * (ALIGN_T * ALIGN_TP);
    float* rowb = lds + ALIGN_WAVES * ALIGN_T * ALIGN_TP;
    float* colb = rowb + 2 * g.cap_b;
    const float* cost = g.cost_in + row * g.cost_row;
    const int64_t wpr = align_words(g.max_b);
    uint32_t* dirs = g.dirs + row * g.max_a * wpr;
    for (int d = 0; d < nbi + nbj - 1; ++d) {
        const int bi_lo = d - (nbj - 1) > 0 ? d - (nbj - 1) : 0, bi_hi = d < nbi - 1 ? d : nbi - 1;
        for (int q0 = bi_lo; q0 <= bi_hi; q0 += ALIGN_WAVES) {      // rounds in ascending block row: block (bi + 1, bj - 1), which overwrites this block's corner, never runs earlier
            const int bi = q0 + wave, bj = d - bi, i0 = bi * ALIGN_T, j0 = bj * ALIGN_T;
            const bool have = bi <= bi_hi;                           // wavefront-uniform
            const int nr = have ? (Fa - i0 < ALIGN_T ? Fa - i0 : ALIGN_T) : 0, nc = have ? (Fb - j0 < ALIGN_T ? Fb - j0 : ALIGN_T) : 0;
            float topv = 0.0f, leftb = 0.0f, corner = 0.0f;
            if (have) {
                if (bi > 0) {
                    const float* rp = rowb + ((bi - 1) & 1) * g.cap_b;
                    if (l < nc) topv = rp[j0 + l];
                    if (bj > 0) corner = rp[j0 - 1];
                }
                if (bj > 0 && l < nr) leftb = colb[i0 + l];
                if (l < nc)
                    for (int rr = 0; rr < nr; ++rr) tile[rr * ALIGN_TP + l] = cost[(int64_t)(i0 + rr) * g.cost_pitch + j0 + l];
            }
            __syncthreads();
            if (have) {
                const int i = i0 + l;
                const bool rowok = l < nr;
                int32_t lo_i, hi_i, lo_u, hi_u;
                align_span(i, Fa, Fb, g.band, &lo_i, &hi_i);
                align_span((int64_t)i - 1, Fa, Fb, g.band, &lo_u, &hi_u);
                float diag = __shfl_up(leftb, 1);
                if (l == 0) diag = corner;
                float prev = leftb, mine = 0.0f;
                uint32_t word = 0;
                float* rowb_w = rowb + (bi & 1) * g.cap_b;
                for (int s = 0; s < nc + nr - 1; ++s) {
                    const int c = s - l;
                    const bool act = rowok && c >= 0 && c < nc;
                    float up = __shfl_up(mine, 1);                   // lane l - 1's cell of the step before: (i - 1, j)
                    const float t = __shfl(topv, s & (ALIGN_T - 1));
                    if (l == 0) up = t;
                    if (act) {
                        const int j = j0 + c;
                        const bool vu = align_in(j, lo_u, hi_u), vd = j > 0 && align_in(j - 1, lo_u, hi_u), vl = j > 0 && align_in(j - 1, lo_i, hi_i);
                        int dir;
                        const float dm = align_cell(tile[l * ALIGN_TP + c], diag, up, prev, vd, vu, vl, i == 0 && j == 0, align_in(j, lo_i, hi_i), &dir);
                        tile[l * ALIGN_TP + c] = dm;
                        word |= (uint32_t)dir << (2 * (c & 15));
                        if ((c & 15) == 15 || c == nc - 1) { dirs[(int64_t)i * wpr + (j >> 4)] = word; word = 0; }
                        if (l == ALIGN_T - 1) rowb_w[j] = dm;        // the bottom row of a full block: the block below reads it
                        if (c == ALIGN_T - 1) colb[i] = dm;          // the last column of a full block: the block to the right reads it
                        if (i == Fa - 1 && j == Fb - 1) g.total[row] = dm;
                        diag = up; prev = dm; mine = dm;
                    }
                }
                if (g.dm && l < nc)
                    for (int rr = 0; rr < nr; ++rr) g.dm[(row * g.max_a + i0 + rr) * g.max_b + j0 + l] = tile[rr * ALIGN_TP + l];
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(ALIGN_THREADS) void wn_align_trace_kernel(const AlignArgs g) {
    extern __shared__ float lds[];     // pi, pj [cap_a + cap_b] int32, pc [cap_a + cap_b] float
    __shared__ int n_sh;
    const int r = blockIdx.x, Fa = g.fa[r], Fb = g.fb[r], tid = threadIdx.x, np = g.cap_a + g.cap_b;
    const int64_t row = g.b0 + r, wpr = align_words(g.max_b);
    int32_t* pi = (int32_t*)lds;
    int32_t* pj = pi + np;
    float* pc = (float*)(pj + np);
    if (tid == 0) {
        const int n = align_backtrace(g.dirs + row * g.max_a * wpr, wpr, g.cost_in + row * g.cost_row, g.cost_pitch, Fa, Fb, pi, pj, pc);
        align_summary(pi, pj, pc, n, Fa, Fb, g.total[row], g.summary + row * 7);
        n_sh = n;
    }
    __syncthreads();
    const int n = n_sh;
    for (int p = tid; p < n; p += ALIGN_THREADS)
        align_emit(pi, pj, n, p, g.path ? g.path + row * 2 * g.path_pitch : nullptr, g.path_pitch, g.map_ab ? g.map_ab + row * g.map_a_pitch : nullptr,
                   g.map_ba ? g.map_ba + row * g.map_b_pitch : nullptr);
}

static size_t align_lds_cep(int M, int n_cep) { return ((size_t)ALIGN_T * melcmp_tile_pitch(M) + (size_t)n_cep * M) * sizeof(float); }
static size_t align_lds_cost(int n_cep) { return (size_t)2 * ALIGN_T * (n_cep | 1) * sizeof(float); }
static size_t align_lds_dp(int cap_a, int cap_b) { return ((size_t)ALIGN_WAVES * ALIGN_T * ALIGN_TP + 2 * (size_t)cap_b + cap_a) * sizeof(float); }
static size_t align_lds_trace(int cap_a, int cap_b) { return (size_t)3 * (cap_a + cap_b) * sizeof(float); }
static int align_round(int n) { return (n + ALIGN_T - 1) / ALIGN_T * ALIGN_T; }

extern "C" int wn_align_create(const wn_align_config* cfg, wn_align** out) {
    wn_align* z = nullptr;
    if (!cfg || !out) WN_FAIL(z, WN_E_ARG, "wn_align_create: null argument");
    *out = nullptr;
    char msg[256];
    if (int rc = wn_align_check_config(cfg, msg, sizeof msg)) WN_FAIL(z, rc, "wn_align_create: %s", msg);
    if (int rc = wn_align_check_reserve(cfg, msg, sizeof msg)) WN_FAIL(z, rc, "wn_align_create: %s", msg);
    wn_align* p = new wn_align();
    p->cfg = *cfg;
    p->cap_a = align_round(cfg->max_frames_a); p->cap_b = align_round(cfg->max_frames_b);
    p->lds_cep = align_lds_cep(cfg->num_mels, cfg->n_cep);      // at most 64 x 129 + 127 x 128 floats = 96.5 KiB of the 160
    p->lds_cost = align_lds_cost(cfg->n_cep);                   // at most 2 x 64 x 127 floats = 63.5 KiB
    p->lds_dp = align_lds_dp(p->cap_a, p->cap_b);               // at most 4 x 64 x 66 + 3 x 4096 floats = 114 KiB
    p->lds_trace = align_lds_trace(p->cap_a, p->cap_b);         // at most 3 x 8192 words = 96 KiB
    int rc = cfg->max_batch == 0 ? WN_OK : [&]() -> int {
        const size_t nb = (size_t)cfg->max_batch, na = (size_t)cfg->max_frames_a, nbf = (size_t)cfg->max_frames_b;
        std::vector<float> t((size_t)cfg->n_cep * cfg->num_mels);
        wn_melcmp_dct_table(cfg->num_mels, cfg->n_cep, t.data());
        WN_HIP(p, p->dct.reserve(t.size()));
        WN_HIP(p, hipMemcpy(p->dct, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
        WN_HIP(p, p->cep_a.reserve(nb * na * cfg->n_cep));
        WN_HIP(p, p->cep_b.reserve(nb * nbf * cfg->n_cep));
        WN_HIP(p, p->cost.reserve(nb * na * nbf));
        WN_HIP(p, p->dirs.reserve(nb * na * (size_t)align_words(cfg->max_frames_b)));
        WN_HIP(p, p->total.reserve(nb));
        // the attributes belong to the functions, not to the handle: always the module's largest need, whatever this handle asks for
        WN_HIP(p, hipFuncSetAttribute((const void*)wn_align_cep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)align_lds_cep(MELCMP_MAX_MELS, MELCMP_MAX_MELS - 1)));
        WN_HIP(p, hipFuncSetAttribute((const void*)wn_align_cost_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)align_lds_cost(MELCMP_MAX_MELS - 1)));
        WN_HIP(p, hipFuncSetAttribute((const void*)wn_align_dp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)align_lds_dp(ALIGN_MAX_FRAMES, ALIGN_MAX_FRAMES)));
        WN_HIP(p, hipFuncSetAttribute((const void*)wn_align_trace_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)align_lds_trace(ALIGN_MAX_FRAMES, ALIGN_MAX_FRAMES)));
        return WN_OK;
    }();
    if (rc != WN_OK) { g_create_err = p->err; delete p; return rc; }
    *out = p;
    return WN_OK;
}

extern "C" void wn_align_destroy(wn_align* p) { delete p; }

extern "C" const char* wn_align_last_error(const wn_align* p) { return p ? p->err.c_str() : g_create_err.c_str(); }

extern "C" int wn_align_tile(const wn_align* p) { return p ? ALIGN_T : WN_E_ARG; }

// the launches of one validated call; cost_in == nullptr: from the mels a, b
static int align_launch(wn_align* p, AlignArgs& g, const int32_t* fa, const int32_t* fb, int32_t B, bool from_mels, hipStream_t st) {
    g.dct = p->dct; g.cep_a = p->cep_a; g.cep_b = p->cep_b; g.cost = p->cost; g.dirs = p->dirs; g.total = p->total; g.dm = p->store_dm ? p->dm.get() : nullptr;
    g.M = p->cfg.num_mels; g.n_cep = p->cfg.n_cep; g.band = p->cfg.band; g.unit = p->cfg.unit_db;
    g.max_a = p->cfg.max_frames_a; g.max_b = p->cfg.max_frames_b; g.cap_a = p->cap_a; g.cap_b = p->cap_b;
    if (from_mels) { g.cost_in = p->cost; g.cost_row = (int64_t)g.max_a * g.max_b; g.cost_pitch = g.max_b; }
    for (int b0 = 0; b0 < B; b0 += ALIGN_GROUP) {
        const int nb = B - b0 < ALIGN_GROUP ? B - b0 : ALIGN_GROUP;
        int32_t na = 0, nbf = 0;
        g.b0 = b0;
        for (int r = 0; r < ALIGN_GROUP; ++r) {
            g.fa[r] = r < nb ? fa[b0 + r] : 0; g.fb[r] = r < nb ? fb[b0 + r] : 0;
            if (g.fa[r] > na) na = g.fa[r];
            if (g.fb[r] > nbf) nbf = g.fb[r];
        }
        if (from_mels) {
            hipLaunchKernelGGL(wn_align_cep_kernel, dim3(cdiv(na > nbf ? na : nbf, ALIGN_T), nb, 2), dim3(ALIGN_THREADS), p->lds_cep, st, g);
            WN_LAUNCH_CHECK(p);
            hipLaunchKernelGGL(wn_align_cost_kernel, dim3(cdiv(nbf, ALIGN_T), cdiv(na, ALIGN_T), nb), dim3(ALIGN_THREADS), p->lds_cost, st, g);
            WN_LAUNCH_CHECK(p);
        }
        hipLaunchKernelGGL(wn_align_dp_kernel, dim3(nb), dim3(ALIGN_THREADS), p->lds_dp, st, g);
        WN_LAUNCH_CHECK(p);
        hipLaunchKernelGGL(wn_align_trace_kernel, dim3(nb), dim3(ALIGN_THREADS), p->lds_trace, st, g);
        WN_LAUNCH_CHECK(p);
    }
    return WN_OK;
}

extern "C" int wn_align_run(wn_align* p, const float* a, int32_t a_channels_first, int64_t a_pitch, const float* b, int32_t b_channels_first, int64_t b_pitch,
                            const int32_t* frames_a, const int32_t* frames_b, int32_t B, int32_t* path, int64_t path_pitch, int32_t* map_ab, int64_t map_a_pitch,
                            int32_t* map_ba, int64_t map_b_pitch, float* summary, void* stream) {
    if (!p) return WN_E_ARG;
    char msg[256];
    if (int rc = wn_align_check_call("wn_align_run", p->cfg.max_batch, p->cfg.max_frames_a, p->cfg.max_frames_b, a, a_pitch, b, b_pitch, frames_a, frames_b, B, path, path_pitch,
                                     map_ab, map_a_pitch, map_ba, map_b_pitch, summary, msg, sizeof msg))
        WN_FAIL(p, rc, "%s", msg);
    AlignArgs g = {};
    g.a = a; g.b = b; g.a_pitch = a_pitch; g.b_pitch = b_pitch; g.a_cf = a_channels_first != 0; g.b_cf = b_channels_first != 0;
    g.path = path; g.path_pitch = path_pitch; g.map_ab = map_ab; g.map_a_pitch = map_a_pitch; g.map_ba = map_ba; g.map_b_pitch = map_b_pitch; g.summary = summary;
    return align_launch(p, g, frames_a, frames_b, B, true, (hipStream_t)stream);
}

extern "C" int wn_test_align_dp(wn_align* p, const float* cost, int32_t Fa_max, int32_t Fb_max, const int32_t* frames_a, const int32_t* frames_b, int32_t B, int32_t* path,
                                int64_t path_pitch, int32_t* map_ab, int64_t map_a_pitch, int32_t* map_ba, int64_t map_b_pitch, float* summary, void* stream) {
    if (!p) return WN_E_ARG;
    char msg[256];
    if (!cost) WN_FAIL(p, WN_E_ARG, "wn_test_align_dp: null argument");
    int32_t na = 0, nb = 0;
    if (int rc = wn_align_check_rows("wn_test_align_dp", p->cfg.max_batch, p->cfg.max_frames_a, p->cfg.max_frames_b, frames_a, frames_b, B, path, path_pitch, map_ab, map_a_pitch,
                                     map_ba, map_b_pitch, summary, &na, &nb, msg, sizeof msg))
        WN_FAIL(p, rc, "%s", msg);
    if (Fa_max < na || Fb_max < nb) WN_FAIL(p, WN_E_SHAPE, "wn_test_align_dp: the cost matrix [%d, %d] is smaller than the longest rows (%d, %d)", Fa_max, Fb_max, na, nb);
    AlignArgs g = {};
    g.cost_in = cost; g.cost_row = (int64_t)Fa_max * Fb_max; g.cost_pitch = Fb_max;
    g.path = path; g.path_pitch = path_pitch; g.map_ab = map_ab; g.map_a_pitch = map_a_pitch; g.map_ba = map_ba; g.map_b_pitch = map_b_pitch; g.summary = summary;
    return align_launch(p, g, frames_a, frames_b, B, false, (hipStream_t)stream);
}

extern "C" int wn_test_align_store_matrix(wn_align* p, int32_t on) {
    if (!p) return WN_E_ARG;
    if (p->cfg.max_batch == 0) WN_FAIL(p, WN_E_SHAPE, "wn_test_align_store_matrix: a validation-only handle");
    if (on) WN_HIP(p, p->dm.reserve((size_t)p->cfg.max_batch * p->cfg.max_frames_a * p->cfg.max_frames_b));
    p->store_dm = on != 0;
    return WN_OK;
}

extern "C" int wn_test_align_copy(wn_align* p, int32_t what, float* dst, int64_t cap, void* stream) {
    if (!p) return WN_E_ARG;
    if (!dst || what < 0 || what > 3) WN_FAIL(p, WN_E_ARG, "wn_test_align_copy: null destination or what (%d) outside 0 ... 3", what);
    if (p->cfg.max_batch == 0) WN_FAIL(p, WN_E_SHAPE, "wn_test_align_copy: a validation-only handle");
    if (what == 3 && !p->dm.get()) WN_FAIL(p, WN_E_STATE, "wn_test_align_copy: no Dm was kept (wn_test_align_store_matrix)");
    const DevBuf<float>& src = what == 0 ? p->cep_a : what == 1 ? p->cep_b : what == 2 ? p->cost : p->dm;
    if (cap < (int64_t)src.cap()) WN_FAIL(p, WN_E_ARG, "wn_test_align_copy: cap (%lld) below %lld floats", (long long)cap, (long long)src.cap());
    WN_HIP(p, hipMemcpyAsync(dst, src.get(), src.bytes(), hipMemcpyDeviceToHost, (hipStream_t)stream));
    WN_HIP(p, hipStreamSynchronize((hipStream_t)stream));
    return WN_OK;
}

extern "C" int wn_test_align_host(const wn_align_config* cfg, const float* a, int32_t a_channels_first, int64_t a_pitch, const float* b, int32_t b_channels_first, int64_t b_pitch,
                                  const int32_t* frames_a, const int32_t* frames_b, int32_t B, int32_t* path, int64_t path_pitch, int32_t* map_ab, int64_t map_a_pitch,
                                  int32_t* map_ba, int64_t map_b_pitch, float* summary, float* cep_a, float* cep_b, float* cost, float* dm) {
    wn_align* z = nullptr;
    char msg[256];
    if (int rc = wn_align_check_config(cfg, msg, sizeof msg)) WN_FAIL(z, rc, "wn_test_align_host: %s", msg);
    if (int rc = wn_align_check_call("wn_test_align_host", INT32_MAX, INT32_MAX, INT32_MAX, a, a_pitch, b, b_pitch, frames_a, frames_b, B, path, path_pitch, map_ab, map_a_pitch,
                                     map_ba, map_b_pitch, summary, msg, sizeof msg))
        WN_FAIL(z, rc, "%s", msg);
    wn_align_host_rows(cfg, a, a_channels_first != 0, a_pitch, b, b_channels_first != 0, b_pitch, frames_a, frames_b, B, path, path_pitch, map_ab, map_a_pitch, map_ba, map_b_pitch,
                       summary, cep_a, cep_b, cost, dm);
    return WN_OK;
}

extern "C" int wn_test_align_dp_host(int32_t band, const float* cost, int32_t Fa_max, int32_t Fb_max, const int32_t* frames_a, const int32_t* frames_b, int32_t B, int32_t* path,
                                     int64_t path_pitch, int32_t* map_ab, int64_t map_a_pitch, int32_t* map_ba, int64_t map_b_pitch, float* summary, float* dm) {
    wn_align* z = nullptr;
    char msg[256];
    if (!cost || band < 0 || band > ALIGN_MAX_BAND) WN_FAIL(z, WN_E_ARG, "wn_test_align_dp_host: null cost matrix or band (%d) outside 0 ... %d", band, ALIGN_MAX_BAND);
    int32_t na = 0, nb = 0;
    if (int rc = wn_align_check_rows("wn_test_align_dp_host", INT32_MAX, INT32_MAX, INT32_MAX, frames_a, frames_b, B, path, path_pitch, map_ab, map_a_pitch, map_ba, map_b_pitch,
                                     summary, &na, &nb, msg, sizeof msg))
        WN_FAIL(z, rc, "%s", msg);
    if (Fa_max < na || Fb_max < nb) WN_FAIL(z, WN_E_SHAPE, "wn_test_align_dp_host: the cost matrix [%d, %d] is smaller than the longest rows (%d, %d)", Fa_max, Fb_max, na, nb);
    wn_align_host_dp_rows(band, cost, Fa_max, Fb_max, frames_a, frames_b, B, path, path_pitch, map_ab, map_a_pitch, map_ba, map_b_pitch, summary, dm);
    return WN_OK;
}
