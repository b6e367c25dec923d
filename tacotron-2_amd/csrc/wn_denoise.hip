// Spectral denoiser: subtract strength x a noise profile from the magnitude of every STFT bin of a ragged batch of signals, keep the phase, transform
// back and overlap-add (wn_denoise_* of include/wavenet_mi355.h; definition, packed spectrum and tables: wn_denoise.h).  The bias denoiser of the flow
// and autoregressive vocoders, on the device.
//
// Two launches per group of 64 rows.  The tile kernel: one workgroup owns DN_TILE = 32 consecutive frames of one row.  It stages the contiguous signal
// span of its frames in LDS once (31 hop + n_fft floats, zero outside [0, n), never reading beyond lengths[b]); wave w then takes the 32-bin groups
// w, w + 4, ...: the 32 frames x (re | im of 32 bins) product with the windowed DFT table on the exact-fp32 matrix instruction (v_mfma_f32_32x32x2_f32,
// taps ascending in two interleaved chains that are joined once), the shrink on the accumulators, and the shrunk bins into the row's packed spectrum in the handle's workspace (global memory: 32 frames x
// n_fft floats do not fit the LDS beside the span at n_fft = 2048).  After a barrier the same workgroup reads its own spectrum rows back as the A operand
// of the inverse product -- 16 bytes per lane hold (re, im) of four consecutive bins (dn_spec_slot) -- against the [n_fft, n_fft] inverse table with the
// synthesis window, the Hermitian weights and 1 / n_fft folded in, wave w taking the 32-sample column groups w, w + 4, ..., packed columns ascending in four interleaved chains joined pairwise, and
// writes the windowed frames [B, F, n_fft] to the second workspace.  The gather kernel: one lane per output sample sums the covering frames in ascending
// f, the window squares of the same frames in the same order, and divides; it alone writes `out`, so in == out is allowed.
// fit is the same tile kernel up to the accumulators: the magnitudes of the frames whose window lies inside the row meet in the wave's LDS patch, one
// lane per bin adds its 32 frames in ascending order (float32) and stores the (row, tile) partial; a second kernel adds the partials over (row, tile)
// ascending in double, divides by the frame count and rounds to float32 (the wn_stats pattern).
// No atomics, no sum split across workgroups, every order a function of (n_fft, hop) and the sample's own row; nothing allocated or synchronised by fit / run.
#include "wn_denoise_dev.h"

struct wn_denoise {
    wn_denoise_config cfg;
    std::string err;
    int NB = 0, G = 0, ldb = 0;
    int64_t Fpad = 0, NT = 0;              // frames of max_samples padded to whole tiles, and those tiles
    size_t lds_bytes = 0;
    bool have_profile = false, host_valid = false;
    std::vector<float> prof_host;          // what wn_denoise_set_profile was given (all a geometry-only handle keeps)
    DevBuf<float> fb, ib, wsq, prof;       // the two tables, w^2, the profile [NB]
    DevBuf<float> spec, frames, part;      // [max_batch][Fpad][n_fft] shrunk packed spectra / windowed frames; [max_batch][NT][NB] partial sums of fit
};

struct DnArgs {
    const float* in; const float* fb; const float* ib; const float* prof; float* spec; float* frames; float* part;
    int64_t in_pitch, ws_row;              // ws_row = Fpad n_fft floats per row of both workspaces
    int32_t b0, n_fft, hop, G, ldb, sig_floats, nt_part;
    float strength;
    int32_t n[DN_GROUP];
};

template <int FIT>
__global__ __launch_bounds__(DN_THREADS) void wn_denoise_tile_kernel(const DnArgs a) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int b = blockIdx.y, n = a.n[b], N = a.n_fft, H = N / 2, hop = a.hop;
    const int Fb = 1 + n / hop, f0 = blockIdx.x * DN_TILE;
    const int64_t row = a.b0 + b;
    float* prt = FIT ? a.part + ((size_t)row * a.nt_part + blockIdx.x) * (H + 1) : nullptr;
    if (f0 >= Fb) {      // the whole tile lies past the row (block-uniform: no barrier has been reached); fit's sum pass reads every tile of the launch
        if (FIT) for (int k = tid; k <= H; k += DN_THREADS) prt[k] = 0.0f;
        return;
    }
    float* sig = lds;
    {
        const float* x = a.in + row * a.in_pitch;
        const int64_t s0 = (int64_t)f0 * hop - H;
        for (int i = tid; i < a.sig_floats; i += DN_THREADS) {
            const int64_t s = s0 + i;
            sig[i] = (s >= 0 && s < n) ? x[s] : 0.0f;
        }
    }
    __syncthreads();
    float* Y = a.spec + row * a.ws_row + (int64_t)f0 * N;      // this tile's 32 packed spectrum rows
    float* patch = lds + a.sig_floats + wave * (DN_TILE * DN_PATCH);
    const float* sp = sig + l31 * hop + lh;      // A operand, taps k / k + 1: lane l holds frame l % 32, tap k + l / 32; largest index 31 hop + n_fft - 1
    for (int g = wave; g < a.G; g += 4) {        // (wave-uniform; no workgroup barrier inside)
        f32x16_t re, im;
        dn_forward_group(sp, a.fb + (size_t)lh * a.ldb + g * 64 + l31, a.ldb, N, &re, &im);      // wn_denoise_dev.h
        // accumulator register r of lane l is (frame 8 (r / 4) + 4 (l / 32) + r % 4, bin 32 g + l % 32); bin 0's "im" is Re X[H]
        const int bin = g * 32 + l31;
        const bool live = bin < H;
        if (!FIT) {
            dn_shrink_group(re, im, Y, a.prof, a.strength, g, N, l31, lh);
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int fr = (r >> 2) * 8 + lh * 4 + (r & 3);
                const int64_t c = (int64_t)(f0 + fr) * hop;
                const bool in = c >= H && c + H <= n;      // the frame's window lies inside [0, n)
                patch[fr * DN_PATCH + l31] = in ? (bin == 0 ? fabsf(re[r]) : dn_mag(re[r], im[r])) : 0.0f;
                if (bin == 0) patch[fr * DN_PATCH + 32] = in ? fabsf(im[r]) : 0.0f;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (lane < 32 ? live : (g == 0 && lane == 32)) {      // one lane per bin: its 32 frames ascending, one float32 accumulator
                float s = 0.0f;
                for (int fr = 0; fr < DN_TILE; ++fr) s = __fadd_rn(s, patch[fr * DN_PATCH + lane]);
                prt[lane < 32 ? bin : H] = s;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();      // the patch is rewritten by the wave's next group
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    if (FIT) return;
    __syncthreads();      // the tile's spectrum rows are complete and visible to the workgroup that wrote them
    float* out = a.frames + row * a.ws_row + (int64_t)f0 * N;
    const float* yp = Y + (size_t)l31 * N + lh * 4;      // lane l: frame l % 32, (re | im) of four consecutive bins
    for (int jg = wave; jg < N / 32; jg += 4) {
        f32x16_t y;
        dn_inverse_group(yp, a.ib + (size_t)lh * N + jg * 32 + l31, N, &y);
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(size_t)dn_acc_frame(r, lh) * N + jg * 32 + l31] = y[r];
    }
}

struct DnGatherArgs {
    const float* frames; const float* wsq; float* out;
    int64_t out_pitch, ws_row;
    int32_t b0, n_fft, hop;
    int32_t n[DN_GROUP];
};

__global__ __launch_bounds__(DN_THREADS) void wn_denoise_gather_kernel(const DnGatherArgs a) {
    const int b = blockIdx.y, n = a.n[b], N = a.n_fft, H = N / 2, hop = a.hop;
    const int64_t i = (int64_t)blockIdx.x * DN_THREADS + threadIdx.x;
    if (i >= n) return;
    const int64_t row = a.b0 + b;
    const int64_t F = 1 + n / hop;
    const int64_t f_lo = i >= H ? (i - H) / hop + 1 : 0, f_hi = (i + H) / hop < F - 1 ? (i + H) / hop : F - 1;
    const float* fr = a.frames + row * a.ws_row;
    float num = 0.0f, den = 0.0f;
    for (int64_t f = f_lo; f <= f_hi; ++f) {      // j = i - f hop + H lies in [0, n_fft) for exactly these f
        const int64_t j = i - f * hop + H;
        num = __fadd_rn(num, fr[f * N + j]);
        den = __fadd_rn(den, a.wsq[j]);
    }
    a.out[row * a.out_pitch + i] = __fdiv_rn(num, den);
}

// part [B][nt_part][nb] -> prof [nb]: (row, tile) ascending in double, / count, rounded once
__global__ __launch_bounds__(DN_THREADS) void wn_denoise_profile_kernel(const float* part, float* prof, int B, int tiles, int nt_part, int nb, double count) {
    const int k = blockIdx.x * DN_THREADS + threadIdx.x;
    if (k >= nb) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < tiles; ++t) s += (double)part[((size_t)b * nt_part + t) * nb + k];
    prof[k] = (float)(s / count);
}

#define DN_PROF_CHUNK 512
struct DnProfArgs { float* dst; int32_t off, cnt; float v[DN_PROF_CHUNK]; };

__global__ __launch_bounds__(DN_PROF_CHUNK) void wn_denoise_set_profile_kernel(const DnProfArgs a) {
    if ((int)threadIdx.x < a.cnt) a.dst[a.off + threadIdx.x] = a.v[threadIdx.x];
}

extern "C" int wn_denoise_create(const wn_denoise_config* cfg, wn_denoise** out) {
    wn_denoise* z = nullptr;
    if (!cfg || !out) WN_FAIL(z, WN_E_ARG, "wn_denoise_create: null argument");
    *out = nullptr;
    char msg[256];
    if (int rc = wn_denoise_check_config(cfg, msg, sizeof msg)) WN_FAIL(z, rc, "wn_denoise_create: %s", msg);
    wn_denoise* d = new wn_denoise();
    d->cfg = *cfg;
    d->NB = dn_bins(cfg->n_fft); d->G = dn_groups(cfg->n_fft); d->ldb = d->G * 64;
    d->Fpad = dn_frames_padded(cfg->max_samples, cfg->hop); d->NT = d->Fpad / DN_TILE;
    d->lds_bytes = (size_t)dn_lds_floats(cfg->n_fft, cfg->hop) * sizeof(float);      // <= 160 KiB for every geometry wn_denoise_check_config admits
    *out = d;
    if (cfg->max_batch == 0) return WN_OK;      // geometry-only handle: reserves nothing and never touches a device; fit / run refuse any B
    DnTables t;
    dn_build_tables(cfg->n_fft, &t);
    const size_t ws = (size_t)cfg->max_batch * d->Fpad * cfg->n_fft;
    int rc = [&]() -> int {
        WN_HIP(d, d->fb.reserve(t.fb.size()));
        WN_HIP(d, d->ib.reserve(t.ib.size()));
        WN_HIP(d, d->wsq.reserve(t.wsq.size()));
        WN_HIP(d, d->prof.reserve((size_t)d->NB));
        WN_HIP(d, d->spec.reserve(ws));
        WN_HIP(d, d->frames.reserve(ws));
        WN_HIP(d, d->part.reserve((size_t)cfg->max_batch * d->NT * d->NB));
        WN_HIP(d, hipMemcpy(d->fb, t.fb.data(), t.fb.size() * 4, hipMemcpyHostToDevice));
        WN_HIP(d, hipMemcpy(d->ib, t.ib.data(), t.ib.size() * 4, hipMemcpyHostToDevice));
        WN_HIP(d, hipMemcpy(d->wsq, t.wsq.data(), t.wsq.size() * 4, hipMemcpyHostToDevice));
        // the attribute belongs to the function, not to this handle: always the 160 KiB cap
        WN_HIP(d, hipFuncSetAttribute((const void*)wn_denoise_tile_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        WN_HIP(d, hipFuncSetAttribute((const void*)wn_denoise_tile_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        return WN_OK;
    }();
    if (rc != WN_OK) { g_create_err = d->err; delete d; *out = nullptr; return rc; }
    return WN_OK;
}

extern "C" void wn_denoise_destroy(wn_denoise* d) { delete d; }

extern "C" const char* wn_denoise_last_error(const wn_denoise* d) { return d ? d->err.c_str() : g_create_err.c_str(); }

extern "C" int64_t wn_denoise_num_frames(const wn_denoise* d, int64_t n) {
    if (!d || n < 0) return (int64_t)WN_E_ARG;
    return 1 + n / d->cfg.hop;
}

static void dn_fill(const wn_denoise* d, DnArgs* a) {
    a->fb = d->fb; a->ib = d->ib; a->prof = d->prof; a->spec = d->spec; a->frames = d->frames; a->part = d->part;
    a->ws_row = d->Fpad * d->cfg.n_fft;
    a->n_fft = d->cfg.n_fft; a->hop = d->cfg.hop; a->G = d->G; a->ldb = d->ldb; a->sig_floats = (int32_t)dn_sig_floats(d->cfg.n_fft, d->cfg.hop); a->nt_part = (int32_t)d->NT;
    a->strength = 0.0f;
}

extern "C" int wn_denoise_fit(wn_denoise* d, const float* wav, int64_t ld, const int32_t* lengths, int32_t B, void* stream) {
    if (!d) return WN_E_ARG;
    char msg[256];
    if (int rc = wn_denoise_check_args("wn_denoise_fit", wav, ld, lengths, B, msg, sizeof msg)) WN_FAIL(d, rc, "%s", msg);
    if (int rc = wn_denoise_check_shape("wn_denoise_fit", d->cfg.max_batch, d->cfg.max_samples, ld, lengths, B, msg, sizeof msg)) WN_FAIL(d, rc, "%s", msg);
    int64_t count = 0; int32_t n_max = 0;
    for (int b = 0; b < B; ++b) { count += wn_denoise_fit_frames(lengths[b], d->cfg.n_fft, d->cfg.hop); if (lengths[b] > n_max) n_max = lengths[b]; }
    if (count == 0) WN_FAIL(d, WN_E_SHAPE, "wn_denoise_fit: no row holds a whole window of n_fft = %d samples", d->cfg.n_fft);
    hipStream_t st = (hipStream_t)stream;
    DnArgs a;
    dn_fill(d, &a);
    a.in = wav; a.in_pitch = ld;
    const int tiles = cdiv(1 + n_max / d->cfg.hop, DN_TILE);
    for (int b0 = 0; b0 < B; b0 += DN_GROUP) {
        const int nb = B - b0 < DN_GROUP ? B - b0 : DN_GROUP;
        a.b0 = b0;
        for (int r = 0; r < DN_GROUP; ++r) a.n[r] = r < nb ? lengths[b0 + r] : 0;
        hipLaunchKernelGGL(wn_denoise_tile_kernel<1>, dim3(tiles, nb), dim3(DN_THREADS), d->lds_bytes, st, a);
        WN_LAUNCH_CHECK(d);
    }
    hipLaunchKernelGGL(wn_denoise_profile_kernel, dim3(cdiv(d->NB, DN_THREADS)), dim3(DN_THREADS), 0, st, (const float*)d->part, (float*)d->prof, B, tiles, (int)d->NT, d->NB, (double)count);
    WN_LAUNCH_CHECK(d);
    d->have_profile = true; d->host_valid = false;
    return WN_OK;
}

extern "C" int wn_denoise_set_profile(wn_denoise* d, const float* profile, void* stream) {
    if (!d) return WN_E_ARG;
    char msg[256];
    if (int rc = wn_denoise_check_profile("wn_denoise_set_profile", profile, d->NB, msg, sizeof msg)) WN_FAIL(d, rc, "%s", msg);
    d->prof_host.assign(profile, profile + d->NB);      // (all a geometry-only handle keeps)
    if (d->cfg.max_batch > 0) {
        // the values travel as kernel arguments, DN_PROF_CHUNK per launch: captured when the launch is enqueued, so no host array has to outlive the call,
        // two calls on one stream are ordered like any two launches, and nothing synchronises
        DnProfArgs a;
        a.dst = d->prof;
        for (int off = 0; off < d->NB; off += DN_PROF_CHUNK) {
            a.off = off; a.cnt = d->NB - off < DN_PROF_CHUNK ? d->NB - off : DN_PROF_CHUNK;
            memcpy(a.v, profile + off, (size_t)a.cnt * 4);
            hipLaunchKernelGGL(wn_denoise_set_profile_kernel, dim3(1), dim3(DN_PROF_CHUNK), 0, (hipStream_t)stream, a);
            WN_LAUNCH_CHECK(d);
        }
    }
    d->have_profile = true; d->host_valid = true;
    return WN_OK;
}

extern "C" int wn_denoise_get_profile(wn_denoise* d, float* profile, void* stream) {
    if (!d) return WN_E_ARG;
    if (!profile) WN_FAIL(d, WN_E_ARG, "wn_denoise_get_profile: null argument");
    if (!d->have_profile) WN_FAIL(d, WN_E_STATE, "wn_denoise_get_profile: no profile has been fitted or set");
    if (d->cfg.max_batch > 0) {
        WN_HIP(d, hipMemcpyAsync(profile, d->prof, (size_t)d->NB * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
        WN_HIP(d, hipStreamSynchronize((hipStream_t)stream));
    } else memcpy(profile, d->prof_host.data(), (size_t)d->NB * 4);
    return WN_OK;
}

extern "C" int wn_denoise_run(wn_denoise* d, const float* in, int64_t in_pitch, const int32_t* lengths, int32_t B, float strength, float* out, int64_t out_pitch, void* stream) {
    if (!d) return WN_E_ARG;
    char msg[256];
    if (!out) WN_FAIL(d, WN_E_ARG, "wn_denoise_run: null argument");
    if (int rc = wn_denoise_check_args("wn_denoise_run", in, in_pitch, lengths, B, msg, sizeof msg)) WN_FAIL(d, rc, "%s", msg);
    if (out_pitch < 0) WN_FAIL(d, WN_E_ARG, "wn_denoise_run: out_pitch (%lld) is negative", (long long)out_pitch);
    if (int rc = wn_denoise_check_strength("wn_denoise_run", strength, msg, sizeof msg)) WN_FAIL(d, rc, "%s", msg);
    if (!d->have_profile) WN_FAIL(d, WN_E_STATE, "wn_denoise_run: no profile has been fitted or set");
    if (int rc = wn_denoise_check_shape("wn_denoise_run", d->cfg.max_batch, d->cfg.max_samples, in_pitch < out_pitch ? in_pitch : out_pitch, lengths, B, msg, sizeof msg))
        WN_FAIL(d, rc, "%s", msg);
    hipStream_t st = (hipStream_t)stream;
    DnArgs a;
    dn_fill(d, &a);
    a.in = in; a.in_pitch = in_pitch; a.strength = strength;
    DnGatherArgs g;
    g.frames = d->frames; g.wsq = d->wsq; g.out = out; g.out_pitch = out_pitch; g.ws_row = a.ws_row; g.n_fft = d->cfg.n_fft; g.hop = d->cfg.hop;
    for (int b0 = 0; b0 < B; b0 += DN_GROUP) {
        const int nb = B - b0 < DN_GROUP ? B - b0 : DN_GROUP;
        int32_t n_max = 0;
        a.b0 = g.b0 = b0;
        for (int r = 0; r < DN_GROUP; ++r) { a.n[r] = g.n[r] = r < nb ? lengths[b0 + r] : 0; if (a.n[r] > n_max) n_max = a.n[r]; }
        if (n_max == 0) continue;      // rows of length 0 write nothing
        hipLaunchKernelGGL(wn_denoise_tile_kernel<0>, dim3(cdiv(1 + n_max / d->cfg.hop, DN_TILE), nb), dim3(DN_THREADS), d->lds_bytes, st, a);
        WN_LAUNCH_CHECK(d);
        hipLaunchKernelGGL(wn_denoise_gather_kernel, dim3(cdiv(n_max, DN_THREADS), nb), dim3(DN_THREADS), 0, st, g);
        WN_LAUNCH_CHECK(d);
    }
    return WN_OK;
}

// the fitted or set profile where it lives (wn_denoise.h): the streaming handle copies it device to device on its own stream, nothing synchronises
extern "C" int wn_denoise_profile_source(const wn_denoise* d, int32_t* n_fft, const float** device_profile, const float** host_profile) {
    if (!d || !n_fft || !device_profile || !host_profile) return WN_E_ARG;
    if (!d->have_profile) return WN_E_STATE;
    *n_fft = d->cfg.n_fft;
    *device_profile = d->cfg.max_batch > 0 ? (const float*)d->prof : nullptr;
    *host_profile = d->cfg.max_batch == 0 ? d->prof_host.data() : nullptr;
    return WN_OK;
}

extern "C" int wn_test_denoise_host(const wn_denoise_config* cfg, const float* fit_wav, int64_t fit_ld, const int32_t* fit_lengths, int32_t fit_B, float* profile,
                                    const float* in, int64_t in_pitch, const int32_t* lengths, int32_t B, float strength, float* out, int64_t out_pitch) {
    wn_denoise* z = nullptr;
    char msg[256];
    if (int rc = wn_denoise_check_config(cfg, msg, sizeof msg)) WN_FAIL(z, rc, "wn_test_denoise_host: %s", msg);
    if (!profile) WN_FAIL(z, WN_E_ARG, "wn_test_denoise_host: null argument");
    DnTables t;
    dn_build_tables(cfg->n_fft, &t);
    if (fit_wav) {
        if (int rc = wn_denoise_check_args("wn_test_denoise_host", fit_wav, fit_ld, fit_lengths, fit_B, msg, sizeof msg)) WN_FAIL(z, rc, "%s", msg);
        if (int rc = wn_denoise_check_shape("wn_test_denoise_host", -1, 0, fit_ld, fit_lengths, fit_B, msg, sizeof msg)) WN_FAIL(z, rc, "%s", msg);
        if (wn_denoise_host_fit(t, cfg->hop, fit_wav, fit_ld, fit_lengths, fit_B, profile) == 0)
            WN_FAIL(z, WN_E_SHAPE, "wn_test_denoise_host: no row holds a whole window of n_fft = %d samples", cfg->n_fft);
    }
    if (!in) return WN_OK;
    if (!out) WN_FAIL(z, WN_E_ARG, "wn_test_denoise_host: null argument");
    if (int rc = wn_denoise_check_args("wn_test_denoise_host", in, in_pitch, lengths, B, msg, sizeof msg)) WN_FAIL(z, rc, "%s", msg);
    if (out_pitch < 0) WN_FAIL(z, WN_E_ARG, "wn_test_denoise_host: out_pitch (%lld) is negative", (long long)out_pitch);
    if (int rc = wn_denoise_check_strength("wn_test_denoise_host", strength, msg, sizeof msg)) WN_FAIL(z, rc, "%s", msg);
    if (int rc = wn_denoise_check_profile("wn_test_denoise_host", profile, dn_bins(cfg->n_fft), msg, sizeof msg)) WN_FAIL(z, rc, "%s", msg);
    if (int rc = wn_denoise_check_shape("wn_test_denoise_host", -1, 0, in_pitch < out_pitch ? in_pitch : out_pitch, lengths, B, msg, sizeof msg)) WN_FAIL(z, rc, "%s", msg);
    wn_denoise_host_run(t, cfg->hop, profile, in, in_pitch, lengths, B, strength, out, out_pitch);
    return WN_OK;
}
