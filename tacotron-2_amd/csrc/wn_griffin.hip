// Griffin-Lim: mel or magnitudes -> signal without a model (wn_griffin_* of include/wavenet_mi355.h; definition, packed spectrum and tables: wn_griffin.h).
// The reference's inv_mel_spectrogram / _griffin_lim (datasets/audio.py:97-112, 151-161), on the device.
//
// One magnitude launch per call fills S [B, Fpad, 1 + n_fft / 2]: one workgroup per (row, frame) turns the frame's normalised mels into amplitudes in LDS,
// then one lane per bin runs the product with the transposed pseudo-inverse, mels ascending in one chain.
// One iteration is two launches per group of 64 rows, shaped like the denoiser's (wn_denoise.hip).  The tile kernel: one workgroup owns GL_TILE = 32
// consecutive frames of one row.  It stages the contiguous span of y its frames read (31 hop + Wp floats, zero outside [0, n)); wave w takes the 32-bin
// groups w, w + 4, ...: the 32 frames x (re | im of 32 bins) product with the windowed DFT table over the win_size taps on v_mfma_f32_32x32x2_f32 (taps
// ascending in two interleaved chains joined once), the projection S (re, im) / hypot on the accumulators, and the projected bins into the row's packed
// spectrum in the workspace.  After a barrier the same workgroup reads its own spectrum rows back as the A operand of the inverse product against the
// [n_fft, ldi] inverse table (synthesis window, Hermitian weights and 1 / n_fft folded in; only the win_size samples the window leaves non-zero), packed
// columns ascending in four interleaved chains joined pairwise, and writes the windowed frames [B, Fpad, ldi].  The start from uniforms or zero phase is
// the same kernel with MODE = 1: no span and no forward product, the spectrum S e^{2 pi i u} written by all lanes.  The gather kernel: one lane per output
// sample adds the covering frames ascending, the window squares of the same frames in the same order, divides once, and alone writes y (and, in the call's
// last launch, the caller's buffer).
// No atomics, no sum split across workgroups, every order a function of the geometry and the sample's own row; nothing allocated or synchronised by a run.
#include "wn_griffin.h"
#include "wn_common.h"

#include <string.h>

struct wn_griffin {
    wn_griffin_config cfg;
    std::string err;
    GlGeom g;
    int64_t Fpad = 0, ypitch = 0;
    size_t lds_bytes = 0;
    bool have_pinv = false, hook = false, ran = false;
    int32_t B = 0;
    std::vector<int32_t> frames;           // of the last run: what wn_griffin_run with WN_GRIFFIN_CONTINUE carries on
    DevBuf<float> fb, ib, wsq, pinvT;      // the two tables, w^2 [ldi], pinv transposed [num_mels][NB]
    DevBuf<float> mag, spec, fr, y;        // [max_batch][Fpad][NB] | [max_batch][Fpad][N] | [max_batch][Fpad][ldi] | [max_batch][ypitch]
    DevBuf<float> pre;                     // test hook: the packed spectrum before the projection [max_batch][Fpad][N]
};

struct GlArgs {
    const float* y; const float* fb; const float* ib; const float* mag; const float* u; float* spec; float* fr; float* pre;
    int64_t y_pitch, mag_row, spec_row, fr_row, u_row;      // floats per row of each array
    int32_t b0, N, hop, Hl, Wp, G, ldb, ldi, sig_floats;
    int32_t F[GL_GROUP];
};

__device__ __forceinline__ int gl_acc_frame(int r, int lh) { return (r >> 2) * 8 + lh * 4 + (r & 3); }

// (copy of dn_forward_group with the tap count as a parameter) sp: the staged span at frame l31's first tap + lh; bp: fb + lh ldb + 64 g + l31
__device__ __forceinline__ void gl_forward_group(const float* sp, const float* bp, int ldb, int taps, f32x16_t* re, f32x16_t* im) {
    f32x16_t rc[2], ic[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { rc[0][r] = 0.0f; rc[1][r] = 0.0f; ic[0][r] = 0.0f; ic[1][r] = 0.0f; }
    float nre[4], nim[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { nre[u] = bp[(size_t)(2 * u) * ldb]; nim[u] = bp[(size_t)(2 * u) * ldb + 32]; }
    for (int k0 = 0; k0 < taps; k0 += 8) {      // Wp is a multiple of 8: whole bodies of 8 taps, the next body's table loads in flight
        float bre[4], bim[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { bre[u] = nre[u]; bim[u] = nim[u]; }
        if (k0 + 8 < taps) {
#pragma unroll
            for (int u = 0; u < 4; ++u) { nre[u] = bp[(size_t)(k0 + 8 + 2 * u) * ldb]; nim[u] = bp[(size_t)(k0 + 8 + 2 * u) * ldb + 32]; }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float av = sp[k0 + 2 * u];
            rc[u & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bre[u], rc[u & 1], 0, 0, 0);
            ic[u & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bim[u], ic[u & 1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) { (*re)[r] = __fadd_rn(rc[0][r], rc[1][r]); (*im)[r] = __fadd_rn(ic[0][r], ic[1][r]); }
}

// (copy of dn_inverse_group with the table's row pitch as a parameter) yp: Y + l31 N + 4 lh; bq: ib + lh ldi + 32 jg + l31
__device__ __forceinline__ void gl_inverse_group(const float* yp, const float* bq, int N, int ldi, f32x16_t* y) {
    f32x16_t acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[u][r] = 0.0f;
    for (int kb = 0; kb < N; kb += 8) {
        const f32x4_t a4 = *(const f32x4_t*)(yp + kb);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[u], bq[(size_t)(kb + 2 * u) * ldi], acc[u], 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) (*y)[r] = __fadd_rn(__fadd_rn(acc[0][r], acc[1][r]), __fadd_rn(acc[2][r], acc[3][r]));
}

// MODE 0: an iteration (reads y).  MODE 1: the start from a.u (NULL: zero phase).  STORE 1 (test hook, MODE 0 only): the spectrum before the projection
// also goes to a.pre; the product instantiation is the one without the store.
template <int MODE, int STORE>
__global__ __launch_bounds__(GL_THREADS) void wn_griffin_tile_kernel(const GlArgs a) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int b = blockIdx.y, Fb = a.F[b], N = a.N, H = N / 2, NB = H + 1, hop = a.hop;
    const int f0 = blockIdx.x * GL_TILE;
    if (f0 >= Fb) return;      // the whole tile lies past the row (block-uniform: no barrier has been reached)
    const int64_t row = a.b0 + b;
    const int64_t n = (int64_t)hop * (Fb - 1);
    float* Y = a.spec + row * a.spec_row + (int64_t)f0 * N;      // this tile's 32 packed spectrum rows (Fpad is a whole number of tiles)
    const float* S = a.mag + row * a.mag_row + (int64_t)f0 * NB;
    if (MODE == 0) {
        float* sig = lds;
        const float* y = a.y + row * a.y_pitch;
        const int64_t s0 = (int64_t)f0 * hop - a.Hl;
        for (int i = tid; i < a.sig_floats; i += GL_THREADS) {
            const int64_t s = s0 + i;
            sig[i] = (s >= 0 && s < n) ? y[s] : 0.0f;
        }
        __syncthreads();
        const float* sp = sig + l31 * hop + lh;      // largest index read: 31 hop + Wp - 1
        float* P = STORE ? a.pre + row * a.spec_row + (int64_t)f0 * N : nullptr;
        for (int g = wave; g < a.G; g += 4) {        // (wave-uniform; no workgroup barrier inside)
            f32x16_t re, im;
            gl_forward_group(sp, a.fb + (size_t)lh * a.ldb + g * 64 + l31, a.ldb, a.Wp, &re, &im);
            // accumulator register r of lane l is (frame gl_acc_frame(r, l / 32), bin 32 g + l % 32); bin 0's "im" is Re X[H]
            const int bin = g * 32 + l31;
            if (bin >= H) continue;
            const int slot = gl_spec_slot(bin, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int fr = gl_acc_frame(r, lh);
                const bool in = f0 + fr < Fb;      // frames past the row: zeros (their magnitudes are not defined)
                const float* Sf = S + (size_t)fr * NB;
                float yr = 0.0f, yi = 0.0f;
                if (in) {
                    if (bin == 0) { yr = gl_project_real(re[r], Sf[0]); yi = gl_project_real(im[r], Sf[H]); }
                    else gl_project(re[r], im[r], Sf[bin], &yr, &yi);
                }
                Y[(size_t)fr * N + slot] = yr; Y[(size_t)fr * N + slot + 4] = yi;
                if (STORE) { P[(size_t)fr * N + slot] = re[r]; P[(size_t)fr * N + slot + 4] = im[r]; }
            }
        }
    } else {
        const float* U = a.u ? a.u + row * a.u_row + (int64_t)f0 * NB : nullptr;
        for (int e = tid; e < GL_TILE * H; e += GL_THREADS) {
            const int fr = e / H, bin = e - fr * H;
            const bool in = f0 + fr < Fb;
            float yr = 0.0f, yi = 0.0f;
            if (in) {
                const float* Sf = S + (size_t)fr * NB;
                if (!U) { yr = Sf[bin]; yi = bin == 0 ? Sf[H] : 0.0f; }
                else {
                    const float* Uf = U + (size_t)fr * NB;
                    gl_start(Sf[bin], Uf[bin], &yr, &yi);
                    if (bin == 0) { float d; gl_start(Sf[H], Uf[H], &yi, &d); }      // bins 0 and H: the real parts alone reach the inverse
                }
            }
            const int slot = gl_spec_slot(bin, 0);
            Y[(size_t)fr * N + slot] = yr; Y[(size_t)fr * N + slot + 4] = yi;
        }
    }
    __syncthreads();      // the tile's spectrum rows are complete and visible to the workgroup that wrote them
    float* out = a.fr + row * a.fr_row + (int64_t)f0 * a.ldi;
    const float* yp = Y + (size_t)l31 * N + lh * 4;      // lane l: frame l % 32, (re | im) of four consecutive bins
    for (int jg = wave; jg < a.ldi / 32; jg += 4) {
        f32x16_t y;
        gl_inverse_group(yp, a.ib + (size_t)lh * a.ldi + jg * 32 + l31, N, a.ldi, &y);
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(size_t)gl_acc_frame(r, lh) * a.ldi + jg * 32 + l31] = y[r];
    }
}

struct GlGatherArgs {
    const float* fr; const float* wsq; float* y; float* out;      // out: NULL, or the caller's buffer (the call's last launch)
    int64_t y_pitch, out_pitch, fr_row;
    int32_t b0, hop, Hl, W, ldi;
    int32_t F[GL_GROUP];
};

__global__ __launch_bounds__(GL_THREADS) void wn_griffin_gather_kernel(const GlGatherArgs a) {
    const int b = blockIdx.y;
    const int64_t F = a.F[b], n = (int64_t)a.hop * (F - 1);
    const int64_t i = (int64_t)blockIdx.x * GL_THREADS + threadIdx.x;
    if (i >= n) return;
    const int64_t row = a.b0 + b, p = i + a.Hl;
    const int64_t f_lo = p >= a.W ? (p - a.W) / a.hop + 1 : 0, f_hi = p / a.hop < F - 1 ? p / a.hop : F - 1;
    const float* fr = a.fr + row * a.fr_row;
    float num = 0.0f, den = 0.0f;
    for (int64_t f = f_lo; f <= f_hi; ++f) {      // j = p - f hop lies in [0, W) for exactly these f
        const int64_t j = p - f * a.hop;
        num = __fadd_rn(num, fr[f * a.ldi + j]);
        den = __fadd_rn(den, a.wsq[j]);
    }
    const float v = __fdiv_rn(num, den);
    a.y[row * a.y_pitch + i] = v;
    if (a.out) a.out[row * a.out_pitch + i] = v;
}

// the start from a caller's signal: y0 -> y (and the caller's out when no iteration follows)
struct GlCopyArgs {
    const float* src; float* y; float* out;
    int64_t src_pitch, y_pitch, out_pitch;
    int32_t b0, hop;
    int32_t F[GL_GROUP];
};
__global__ __launch_bounds__(GL_THREADS) void wn_griffin_copy_kernel(const GlCopyArgs a) {
    const int b = blockIdx.y;
    const int64_t n = (int64_t)a.hop * (a.F[b] - 1), i = (int64_t)blockIdx.x * GL_THREADS + threadIdx.x;
    if (i >= n) return;
    const int64_t row = a.b0 + b;
    const float v = a.src[row * a.src_pitch + i];
    a.y[row * a.y_pitch + i] = v;
    if (a.out) a.out[row * a.out_pitch + i] = v;
}

struct GlMagArgs {
    const float* src; const float* pinvT; float* mag;
    int64_t mag_row;
    GlMelMap m;
    int32_t b0, src_kind, F_max, NB;
    int32_t F[GL_GROUP];
};
// grid (frames, rows): the frame's amplitudes in LDS, then one lane per bin
__global__ __launch_bounds__(GL_THREADS) void wn_griffin_mag_kernel(const GlMagArgs a) {
    __shared__ float amp[GL_MAX_MELS];
    const int b = blockIdx.y, f = blockIdx.x;
    if (f >= a.F[b]) return;      // (block-uniform)
    const int64_t row = a.b0 + b;
    float* dst = a.mag + row * a.mag_row + (int64_t)f * a.NB;
    if (a.src_kind == GL_SRC_MAG) {
        const float* s = a.src + ((size_t)row * a.F_max + f) * a.NB;
        for (int k = threadIdx.x; k < a.NB; k += GL_THREADS) dst[k] = s[k];
        return;
    }
    const int M = a.m.num_mels;
    for (int m = threadIdx.x; m < M; m += GL_THREADS)
        amp[m] = gl_mel_amp(a.m, a.src_kind == GL_SRC_MEL ? a.src[((size_t)row * a.F_max + f) * M + m] : a.src[((size_t)row * M + m) * a.F_max + f]);
    __syncthreads();
    for (int k = threadIdx.x; k < a.NB; k += GL_THREADS) dst[k] = gl_mel_bin(a.m, amp, a.pinvT, a.NB, k);
}

extern "C" int wn_griffin_create(const wn_griffin_config* cfg, const float* pinv, wn_griffin** out) {
    wn_griffin* z = nullptr;
    if (!cfg || !out) WN_FAIL(z, WN_E_ARG, "wn_griffin_create: null argument");
    *out = nullptr;
    char msg[256];
    if (int rc = wn_griffin_check_config(cfg, msg, sizeof msg)) WN_FAIL(z, rc, "wn_griffin_create: %s", msg);
    wn_griffin* d = new wn_griffin();
    d->cfg = *cfg;
    d->g = gl_geom(cfg->n_fft, cfg->win_size, cfg->hop);
    d->have_pinv = pinv != nullptr && cfg->num_mels > 0;
    d->Fpad = gl_frames_padded(cfg->max_frames);
    d->ypitch = cfg->max_frames > 0 ? (int64_t)cfg->hop * (cfg->max_frames - 1) : 0;
    d->lds_bytes = (size_t)gl_sig_floats(d->g) * sizeof(float);      // <= 31 x 1024 + 4096 floats = 140 KiB for every geometry wn_griffin_check_config admits
    *out = d;
    if (cfg->max_batch == 0) return WN_OK;      // geometry-only handle: reserves nothing and never touches a device; run refuses any B
    GlTables t;
    gl_build_tables(cfg->n_fft, cfg->win_size, cfg->hop, &t);
    std::vector<float> pT;
    if (d->have_pinv) {
        pT.resize((size_t)cfg->num_mels * d->g.NB);
        for (int k = 0; k < d->g.NB; ++k)
            for (int m = 0; m < cfg->num_mels; ++m) pT[(size_t)m * d->g.NB + k] = pinv[(size_t)k * cfg->num_mels + m];
    }
    const size_t rows = (size_t)cfg->max_batch * d->Fpad;
    int rc = [&]() -> int {
        WN_HIP(d, d->fb.reserve(t.fb.size()));
        WN_HIP(d, d->ib.reserve(t.ib.size()));
        WN_HIP(d, d->wsq.reserve(t.wsq.size()));
        if (d->have_pinv) WN_HIP(d, d->pinvT.reserve(pT.size()));
        WN_HIP(d, d->mag.reserve(rows * d->g.NB));
        WN_HIP(d, d->spec.reserve(rows * d->g.N));
        WN_HIP(d, d->fr.reserve(rows * d->g.ldi));
        WN_HIP(d, d->y.reserve((size_t)cfg->max_batch * d->ypitch));
        WN_HIP(d, hipMemcpy(d->fb, t.fb.data(), t.fb.size() * 4, hipMemcpyHostToDevice));
        WN_HIP(d, hipMemcpy(d->ib, t.ib.data(), t.ib.size() * 4, hipMemcpyHostToDevice));
        WN_HIP(d, hipMemcpy(d->wsq, t.wsq.data(), t.wsq.size() * 4, hipMemcpyHostToDevice));
        if (d->have_pinv) WN_HIP(d, hipMemcpy(d->pinvT, pT.data(), pT.size() * 4, hipMemcpyHostToDevice));
        // the attribute belongs to the function, not to this handle: always the 160 KiB cap
        WN_HIP(d, hipFuncSetAttribute((const void*)wn_griffin_tile_kernel<0, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        WN_HIP(d, hipFuncSetAttribute((const void*)wn_griffin_tile_kernel<0, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        return WN_OK;
    }();
    if (rc != WN_OK) { g_create_err = d->err; delete d; *out = nullptr; return rc; }
    return WN_OK;
}

extern "C" void wn_griffin_destroy(wn_griffin* d) { delete d; }

extern "C" const char* wn_griffin_last_error(const wn_griffin* d) { return d ? d->err.c_str() : g_create_err.c_str(); }

extern "C" int64_t wn_griffin_num_samples(const wn_griffin* d, int64_t frames) {
    if (!d || frames < 1) return (int64_t)WN_E_ARG;
    return (int64_t)d->cfg.hop * (frames - 1);
}

extern "C" int wn_griffin_run(wn_griffin* d, const float* src, int32_t src_kind, int32_t F_max, const int32_t* frames, int32_t B, const float* u, const float* y0,
                              int64_t y0_pitch, int32_t iters, int32_t flags, float* out, int64_t out_pitch, void* stream) {
    if (!d) return WN_E_ARG;
    char msg[256];
    const bool cont = (flags & WN_GRIFFIN_CONTINUE) != 0;
    if (flags & ~WN_GRIFFIN_CONTINUE) WN_FAIL(d, WN_E_ARG, "wn_griffin_run: unknown flags (%d)", flags);
    if (cont) {
        if (iters < 0) WN_FAIL(d, WN_E_ARG, "wn_griffin_run: iters (%d) is negative", iters);
        if (out_pitch < 0) WN_FAIL(d, WN_E_ARG, "wn_griffin_run: a pitch is negative");
        if (!d->ran) WN_FAIL(d, WN_E_STATE, "wn_griffin_run: nothing to continue: no run has been made on this handle");
        if (out)
            for (int b = 0; b < d->B; ++b)
                if ((int64_t)d->cfg.hop * (d->frames[b] - 1) > out_pitch) WN_FAIL(d, WN_E_SHAPE, "wn_griffin_run: row %d is longer than out_pitch = %lld", b, (long long)out_pitch);
    } else {
        if (int rc = wn_griffin_check_run("wn_griffin_run", &d->cfg, d->have_pinv, d->cfg.max_batch, src, src_kind, F_max, frames, B, y0, y0_pitch, iters, out, out_pitch, msg, sizeof msg))
            WN_FAIL(d, rc, "%s", msg);
        d->B = B; d->frames.assign(frames, frames + B); d->ran = true;
    }
    hipStream_t st = (hipStream_t)stream;
    const GlGeom& g = d->g;
    GlArgs a;
    a.y = d->y; a.fb = d->fb; a.ib = d->ib; a.mag = d->mag; a.u = u; a.spec = d->spec; a.fr = d->fr; a.pre = d->hook ? (float*)d->pre : nullptr;
    a.y_pitch = d->ypitch; a.mag_row = d->Fpad * g.NB; a.spec_row = d->Fpad * g.N; a.fr_row = d->Fpad * g.ldi; a.u_row = (int64_t)F_max * g.NB;
    a.N = g.N; a.hop = g.hop; a.Hl = g.Hl; a.Wp = g.Wp; a.G = g.G; a.ldb = g.ldb; a.ldi = g.ldi; a.sig_floats = (int32_t)gl_sig_floats(g);
    GlGatherArgs ga;
    ga.fr = d->fr; ga.wsq = d->wsq; ga.y = d->y; ga.y_pitch = d->ypitch; ga.out_pitch = out_pitch; ga.fr_row = a.fr_row;
    ga.hop = g.hop; ga.Hl = g.Hl; ga.W = g.W; ga.ldi = g.ldi;
    for (int b0 = 0; b0 < d->B; b0 += GL_GROUP) {
        const int nb = d->B - b0 < GL_GROUP ? d->B - b0 : GL_GROUP;
        int32_t f_max = 0;
        a.b0 = ga.b0 = b0;
        for (int r = 0; r < GL_GROUP; ++r) { a.F[r] = ga.F[r] = r < nb ? d->frames[b0 + r] : 0; if (a.F[r] > f_max) f_max = a.F[r]; }
        const dim3 tiles(cdiv(f_max, GL_TILE), nb), samples(cdiv((int64_t)g.hop * (f_max - 1), GL_THREADS), nb);
        if (!cont) {
            GlMagArgs m;
            m.src = src; m.pinvT = d->pinvT; m.mag = d->mag; m.mag_row = a.mag_row; m.m = gl_mel_map(d->cfg);
            m.b0 = b0; m.src_kind = src_kind; m.F_max = F_max; m.NB = g.NB;
            memcpy(m.F, a.F, sizeof m.F);
            hipLaunchKernelGGL(wn_griffin_mag_kernel, dim3(f_max, nb), dim3(GL_THREADS), 0, st, m);
            WN_LAUNCH_CHECK(d);
            if (y0) {
                GlCopyArgs c;
                c.src = y0; c.y = d->y; c.out = iters == 0 ? out : nullptr; c.src_pitch = y0_pitch; c.y_pitch = d->ypitch; c.out_pitch = out_pitch; c.b0 = b0; c.hop = g.hop;
                memcpy(c.F, a.F, sizeof c.F);
                hipLaunchKernelGGL(wn_griffin_copy_kernel, samples, dim3(GL_THREADS), 0, st, c);
                WN_LAUNCH_CHECK(d);
            } else {
                hipLaunchKernelGGL((wn_griffin_tile_kernel<1, 0>), tiles, dim3(GL_THREADS), 0, st, a);
                WN_LAUNCH_CHECK(d);
                ga.out = iters == 0 ? out : nullptr;
                hipLaunchKernelGGL(wn_griffin_gather_kernel, samples, dim3(GL_THREADS), 0, st, ga);
                WN_LAUNCH_CHECK(d);
            }
        }
        for (int it = 0; it < iters; ++it) {
            if (d->hook) hipLaunchKernelGGL((wn_griffin_tile_kernel<0, 1>), tiles, dim3(GL_THREADS), d->lds_bytes, st, a);
            else hipLaunchKernelGGL((wn_griffin_tile_kernel<0, 0>), tiles, dim3(GL_THREADS), d->lds_bytes, st, a);
            WN_LAUNCH_CHECK(d);
            ga.out = it == iters - 1 ? out : nullptr;
            hipLaunchKernelGGL(wn_griffin_gather_kernel, samples, dim3(GL_THREADS), 0, st, ga);
            WN_LAUNCH_CHECK(d);
        }
        if (cont && iters == 0 && out) {      // a continuation of no iterations hands out the handle's y
            GlCopyArgs c;
            c.src = d->y; c.y = d->y; c.out = out; c.src_pitch = d->ypitch; c.y_pitch = d->ypitch; c.out_pitch = out_pitch; c.b0 = b0; c.hop = g.hop;
            memcpy(c.F, a.F, sizeof c.F);
            hipLaunchKernelGGL(wn_griffin_copy_kernel, samples, dim3(GL_THREADS), 0, st, c);
            WN_LAUNCH_CHECK(d);
        }
    }
    return WN_OK;
}

// ---- test hooks
extern "C" int wn_test_griffin_store_spectrum(wn_griffin* d, int32_t on) {
    if (!d) return WN_E_ARG;
    if (d->cfg.max_batch == 0) WN_FAIL(d, WN_E_STATE, "wn_test_griffin_store_spectrum: a geometry-only handle runs nothing");
    if (on && !d->pre.cap()) {
        WN_HIP(d, d->pre.reserve((size_t)d->cfg.max_batch * d->Fpad * d->g.N));      // (the one reserve outside create: a test hook)
        WN_HIP(d, hipMemset(d->pre, 0, (size_t)d->cfg.max_batch * d->Fpad * d->g.N * 4));
    }
    d->hook = on != 0;
    return WN_OK;
}

// what = 0: the magnitudes -> dst [B][F_max][NB]; what = 1: the spectrum before the last projection -> dst [B][F_max][NB][2].  Frames beyond a row's are
// left as they are.  SYNCHRONISES the stream.
extern "C" int wn_test_griffin_copy(wn_griffin* d, int32_t what, float* dst, int32_t F_max, void* stream) {
    if (!d) return WN_E_ARG;
    if (!dst || what < 0 || what > 1) WN_FAIL(d, WN_E_ARG, "wn_test_griffin_copy: bad argument");
    if (!d->ran || (what == 1 && !d->pre.cap())) WN_FAIL(d, WN_E_STATE, "wn_test_griffin_copy: nothing to copy");
    const GlGeom& g = d->g;
    WN_HIP(d, hipStreamSynchronize((hipStream_t)stream));
    std::vector<float> tmp((size_t)(what ? g.N : g.NB));
    for (int64_t b = 0; b < d->B; ++b) {
        if (d->frames[b] > F_max) WN_FAIL(d, WN_E_SHAPE, "wn_test_griffin_copy: F_max (%d) is below the frames of row %lld", F_max, (long long)b);
        for (int64_t f = 0; f < d->frames[b]; ++f) {
            if (what == 0) {
                WN_HIP(d, hipMemcpy(dst + ((size_t)b * F_max + f) * g.NB, (const float*)d->mag + ((size_t)b * d->Fpad + f) * g.NB, (size_t)g.NB * 4, hipMemcpyDeviceToHost));
                continue;
            }
            WN_HIP(d, hipMemcpy(tmp.data(), (const float*)d->pre + ((size_t)b * d->Fpad + f) * g.N, (size_t)g.N * 4, hipMemcpyDeviceToHost));
            float* p = dst + ((size_t)b * F_max + f) * g.NB * 2;
            for (int k = 0; k < g.H; ++k) { p[2 * k] = tmp[gl_spec_slot(k, 0)]; p[2 * k + 1] = k == 0 ? 0.0f : tmp[gl_spec_slot(k, 1)]; }
            p[2 * g.H] = tmp[gl_spec_slot(0, 1)]; p[2 * g.H + 1] = 0.0f;
        }
    }
    return WN_OK;
}

extern "C" int wn_test_griffin_host(const wn_griffin_config* cfg, const float* pinv, const float* src, int32_t src_kind, int32_t F_max, const int32_t* frames, int32_t B,
                                    const float* u, const float* y0, int64_t y0_pitch, int32_t iters, float* out, int64_t out_pitch, float* mag_out, float* pre_out) {
    wn_griffin* z = nullptr;
    char msg[256];
    if (int rc = wn_griffin_check_config(cfg, msg, sizeof msg)) WN_FAIL(z, rc, "wn_test_griffin_host: %s", msg);
    if (!out) WN_FAIL(z, WN_E_ARG, "wn_test_griffin_host: null argument");
    if (int rc = wn_griffin_check_run("wn_test_griffin_host", cfg, pinv != nullptr, -1, src, src_kind, F_max, frames, B, y0, y0_pitch, iters, out, out_pitch, msg, sizeof msg))
        WN_FAIL(z, rc, "%s", msg);
    GlTables t;
    gl_build_tables(cfg->n_fft, cfg->win_size, cfg->hop, &t);
    const int NB = t.g.NB;
    std::vector<float> pT, mag((size_t)B * F_max * NB, 0.0f);
    if (src_kind != GL_SRC_MAG) {
        pT.resize((size_t)cfg->num_mels * NB);
        for (int k = 0; k < NB; ++k)
            for (int m = 0; m < cfg->num_mels; ++m) pT[(size_t)m * NB + k] = pinv[(size_t)k * cfg->num_mels + m];
    }
    gl_host_magnitudes(*cfg, pT.data(), src, src_kind, F_max, frames, B, mag.data());
    if (mag_out) memcpy(mag_out, mag.data(), mag.size() * 4);
    for (int64_t b = 0; b < B; ++b)
        gl_host_row(t, &mag[(size_t)b * F_max * NB], u ? u + (size_t)b * F_max * NB : nullptr, y0 ? y0 + b * y0_pitch : nullptr, frames[b], iters, out + b * out_pitch,
                    pre_out ? pre_out + (size_t)b * F_max * NB * 2 : nullptr);
    return WN_OK;
}
