// Mel analysis: wav -> normalised mel-spectrogram on the device (wn_mel_* of include/wavenet_mi355.h).  Replaces the librosa / numpy front end of the
// reference's preprocessing (datasets/audio.py:70-77 melspectrogram, :178-182 _stft, :243-270 _linear_to_mel / _amp_to_db / _normalize) and,
// optionally fused into the signal staging, its pre-emphasis and rescale (audio.py:22-25, wavenet_preprocessor.py:71-76).
//
// win_size <= n_fft, so the windowed DFT of a frame is a product of its win_size samples with a fixed [win_size, 2 x (1 + n_fft / 2)] matrix
// (window folded in, built in double at create time with the argument reduced as integers).  One workgroup owns TF = 32 FR consecutive frames
// of one utterance for ALL bins: it stages the contiguous signal span of its frames in LDS once ((TF - 1) hop + win_size samples; frame rows
// are overlapping windows of it, nothing is materialised as an im2col buffer), then walks the bins in chunks of 4 x 32: wave w multiplies the
// TF frames with the re and im columns of bin group 4 chunk + w on the exact-fp32 matrix instruction (v_mfma_f32_32x32x2_f32, fp32
// accumulation, k ascending: a fixed order) and forms the power in registers; the powers of 32 frames x the chunk's 128 bins meet in an LDS patch,
// from which wave w < ldm / 32 adds their product with the mel filters of mels 32 w ... 32 w + 31 to its [TF, 32] mel accumulator (bins ascending).
// Then level, normalisation and the store in either layout.  No atomics, no split of the tap sum or the bin sum across workgroups, no scratch in HBM.
// Everything behind the staging is mel_core of wn_mel.h, which the streaming form (wn_mel_stream.hip) runs too: this file keeps the staging loop and the store.
#include "wn_mel.h"

struct wn_mel {
    wn_mel_config cfg;
    std::string err;
    MelGeom g;
    int FR = 0, n_cu = 256;                        // FR: the largest frame tile / 32 this context runs
    bool fixed_tile = false;                       // WN_MEL_TF: every call runs FR (the A/B of tools/mel_timing.py)
    DevBuf<float> basis, melT;                     // [win_pad][G][re 32 | im 32] window x cos / -sin;  [32 G][32 MT] mel filters transposed, zero padded
};

struct MelArgs {
    const float* wav; int64_t ld; const float* gain; float* out; const float* basis; const float* melT;
    int32_t b0, F_max, channels_first;
    int32_t hop, win_pad, off_lo, nchunks, ldb, num_mels, mt, ldm, sig_floats;      // mt = ldm / 32 mel tiles
    float kpre, pow_half; int32_t pow_mode;      // 0: power 2 (as is), 1: power 1 (sqrt), 2: powf
    float min_lin, ref_db, lo, maxabs; int32_t norm, clip, symmetric;
    int32_t n[MEL_GROUP];
};

template <int FR>
__global__ __launch_bounds__(256) void wn_mel_kernel(const MelArgs a) {
    extern __shared__ float lds[];
    constexpr int TF = FR * 32;
    const int tid = threadIdx.x;
    const int b = blockIdx.y, n = a.n[b], Fb = 1 + n / a.hop;
    const int f0 = blockIdx.x * TF;
    const int64_t ub = a.b0 + b;
    const float pad = mel_finish(a, 0.0f);          // what an all-zero signal gives: rows past the utterance's last frame
    auto store = [&](int f, int m, float v) {
        if (f0 + f >= a.F_max) return;
        if (a.channels_first) a.out[(ub * a.num_mels + m) * a.F_max + f0 + f] = v;
        else a.out[(ub * a.F_max + f0 + f) * a.num_mels + m] = v;
    };
    if (f0 >= Fb) {      // the whole tile lies past the utterance (block-uniform: no barrier has been reached)
        for (int e = tid; e < TF * a.num_mels; e += 256) {
            if (a.channels_first) store(e % TF, e / TF, pad); else store(e / a.num_mels, e % a.num_mels, pad);
        }
        return;
    }
    float* sig = lds;
    {   // the contiguous span of this tile's frames: sig[i] = y[f0 hop + off - n_fft / 2 + i], zero outside the utterance
        const float* x = a.wav + ub * a.ld;
        const float g = a.gain ? a.gain[ub] : 1.0f;
        const int64_t s0 = (int64_t)f0 * a.hop + a.off_lo;
        for (int i = tid; i < a.sig_floats; i += 256) {
            const int64_t s = s0 + i;
            sig[i] = (s >= 0 && s < n) ? __fmul_rn(g, mel_preem(x, s, a.kpre)) : 0.0f;
        }
    }
    __syncthreads();
    mel_core<FR>(a, lds, Fb - f0, pad, store);
}

struct PeakArgs { const float* wav; int64_t ld; float* peak; int32_t b0; float kpre; int32_t n[MEL_GROUP]; };

// max_s |x[s] - k_pre x[s - 1]|: a max is exact and order independent (one workgroup per utterance, tree in LDS)
__global__ __launch_bounds__(1024) void wn_mel_peak_kernel(const PeakArgs a) {
    __shared__ float part[1024];
    const int b = blockIdx.x, n = a.n[b];
    const float* x = a.wav + (int64_t)(a.b0 + b) * a.ld;
    float m = 0.0f;
    for (int s = threadIdx.x; s < n; s += 1024) m = fmaxf(m, fabsf(mel_preem(x, s, a.kpre)));
    part[threadIdx.x] = m;
    __syncthreads();
    for (int h = 512; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] = fmaxf(part[threadIdx.x], part[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x == 0) a.peak[a.b0 + b] = part[0];
}

typedef void (*mel_kernel_t)(const MelArgs);
static mel_kernel_t mel_kernel(int FR) { return FR == 1 ? wn_mel_kernel<1> : FR == 2 ? wn_mel_kernel<2> : wn_mel_kernel<4>; }

static size_t mel_lds(const wn_mel* m, int FR, int* sig_floats) { return mel_lds(m->cfg, m->g, FR, sig_floats); }

/* datasets/audio.py:70-77, 178-182, 243-270: the geometry and level hparams of melspectrogram; mel_basis = _build_mel_basis (librosa.filters.mel) */
extern "C" int wn_mel_create(const wn_mel_config* cfg, const float* mel_basis, wn_mel** out) {
    wn_mel* z = nullptr;
    if (!cfg || !out) WN_FAIL(z, WN_E_ARG, "wn_mel_create: null argument");
    *out = nullptr;
    if (cfg->abi_version != WN_ABI_VERSION) WN_FAIL(z, WN_E_ARG, "wn_mel_create: abi_version %d != %d", cfg->abi_version, WN_ABI_VERSION);
    if (!mel_basis) WN_FAIL(z, WN_E_ARG, "wn_mel_create: mel_basis is null");
    { char msg[256]; if (int rc = mel_check_geometry(cfg, msg, sizeof msg)) WN_FAIL(z, rc, "%s", msg); }
    if (cfg->max_batch < 0 || cfg->max_samples < 0 || cfg->max_samples > 0x7fffffffLL) WN_FAIL(z, WN_E_ARG, "max_batch / max_samples must be in [0, 2^31)");
    if (cfg->n_fft > (1 << 16)) WN_FAIL(z, WN_E_UNSUPPORTED, "n_fft (%d) > 65536", cfg->n_fft);

    wn_mel* m = new wn_mel();
    m->cfg = *cfg;
    m->g = mel_geom(*cfg);
    *out = m;
    if (cfg->max_batch == 0) return WN_OK;      // geometry-only context (wn_mel_num_frames): reserves nothing and never touches a device; wn_mel_run / wn_mel_peak refuse any B

    // frame tile: chosen per call among 32 / 64 / 128 (mel_pick_tile) up to the largest whose LDS fits; WN_MEL_TF pins one for the A/B
    m->FR = 4;
    if (const char* e = getenv("WN_MEL_TF")) {
        const int tf = atoi(e);
        if (tf != 32 && tf != 64 && tf != 128) { g_create_err = "WN_MEL_TF must be 32, 64 or 128"; delete m; *out = nullptr; return WN_E_ARG; }
        m->FR = tf / 32; m->fixed_tile = true;
    }
    while (m->FR > 1 && mel_lds(m, m->FR, nullptr) > 160 * 1024) m->FR /= 2;
    if (mel_lds(m, m->FR, nullptr) > 160 * 1024) {
        char bf[160]; snprintf(bf, sizeof bf, "hop_size %d / win_size %d: the signal span of a 32-frame tile does not fit the 160 KiB LDS", cfg->hop_size, cfg->win_size);
        g_create_err = bf; delete m; *out = nullptr; return WN_E_UNSUPPORTED;
    }
    std::vector<float> hb, hm;
    mel_build_tables(*cfg, m->g, mel_basis, &hb, &hm);
    int rc = [&]() -> int {
        WN_HIP(m, m->basis.reserve(hb.size()));
        WN_HIP(m, m->melT.reserve(hm.size()));
        WN_HIP(m, hipMemcpy(m->basis, hb.data(), hb.size() * 4, hipMemcpyHostToDevice));
        WN_HIP(m, hipMemcpy(m->melT, hm.data(), hm.size() * 4, hipMemcpyHostToDevice));
        // the attribute belongs to the function, not to this context: always the 160 KiB cap, so that contexts of different geometries do not lower it for one another
        for (int fr = 1; fr <= 4; fr *= 2)
            WN_HIP(m, hipFuncSetAttribute((const void*)mel_kernel(fr), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        int dev = 0; hipDeviceProp_t pr;
        WN_HIP(m, hipGetDevice(&dev));
        WN_HIP(m, hipGetDeviceProperties(&pr, dev));
        if (pr.multiProcessorCount > 0) m->n_cu = pr.multiProcessorCount;
        return WN_OK;
    }();
    if (rc != WN_OK) { g_create_err = m->err; wn_mel_destroy(m); *out = nullptr; return rc; }
    return WN_OK;
}

extern "C" void wn_mel_destroy(wn_mel* m) {
    delete m;
}

extern "C" const char* wn_mel_last_error(const wn_mel* m) { return m ? m->err.c_str() : g_create_err.c_str(); }

/* librosa.stft(center=True): 1 + n // hop frames (audio.py:178-182) */
extern "C" int64_t wn_mel_num_frames(const wn_mel* m, int64_t n_samples) {
    if (!m || n_samples < 0) return (int64_t)WN_E_ARG;
    return 1 + n_samples / m->cfg.hop_size;
}

/* largest frame tile of this context (32 / 64 / 128; 0 for a geometry-only context): the tile-boundary cases of the tests and tools/mel_timing.py read it */
extern "C" int wn_mel_frame_tile(const wn_mel* m) { return m ? m->FR * 32 : WN_E_ARG; }

// Frame tile of one call.  A workgroup of FR x 32 frames takes about 0.5 / 0.8 / 1.44 ms at FR = 1 / 2 / 4 (calibrated at the DEFAULT geometry on 256 CUs only and
// applied to every geometry; it also counts one workgroup per CU although two 32-frame tiles fit a CU's LDS -- speed only, never the result;
// profiles/mel_timing.json: the basis stream and the epilogue are paid once per workgroup, the products once per 32 frames), and the launch takes
// ceil(workgroups / CUs) such rounds: the tile with the smallest product wins, the larger one on a tie.  The result does not depend on the choice
// (every frame's sums run in the same order under all three).
static int mel_pick_tile(const wn_mel* m, const int32_t* lengths, int32_t B) {
    if (m->fixed_tile) return m->FR;
    static const double cost[3] = { 0.50, 0.80, 1.44 };
    int best = 1; double best_t = 1e300;
    for (int fr = 1, i = 0; fr <= m->FR; fr *= 2, ++i) {
        int64_t wg = 0;
        for (int b = 0; b < B; ++b) wg += (1 + lengths[b] / m->cfg.hop_size + fr * 32 - 1) / (fr * 32);
        const double t = (double)((wg + m->n_cu - 1) / m->n_cu) * cost[i];
        if (t <= best_t) { best_t = t; best = fr; }
    }
    return best;
}

static int mel_check_batch(wn_mel* m, const char* who, const float* wav, int64_t ld, const int32_t* lengths, int32_t B) {
    if (!wav || !lengths) WN_FAIL(m, WN_E_ARG, "%s: null argument", who);
    if (B < 1 || B > m->cfg.max_batch) WN_FAIL(m, WN_E_SHAPE, "%s: B (%d) must be in [1, max_batch = %d]", who, B, m->cfg.max_batch);
    if (ld < 0) WN_FAIL(m, WN_E_SHAPE, "%s: ld (%lld) < 0", who, (long long)ld);
    for (int b = 0; b < B; ++b) {
        if (lengths[b] < 0 || lengths[b] > ld) WN_FAIL(m, WN_E_SHAPE, "%s: lengths[%d] = %d must be in [0, ld = %lld]", who, b, lengths[b], (long long)ld);
        if (lengths[b] > m->cfg.max_samples) WN_FAIL(m, WN_E_SHAPE, "%s: lengths[%d] = %d exceeds max_samples = %lld", who, b, lengths[b], (long long)m->cfg.max_samples);
    }
    return WN_OK;
}

/* max |preemphasis(wav)| per utterance (audio.py:22-25; the denominator of wavenet_preprocessor.py:76) */
extern "C" int wn_mel_peak(wn_mel* m, const float* wav, int64_t ld, const int32_t* lengths, int32_t B, float* peak, void* stream) {
    if (!m) return WN_E_ARG;
    if (!peak) WN_FAIL(m, WN_E_ARG, "wn_mel_peak: null argument");
    if (int rc = mel_check_batch(m, "wn_mel_peak", wav, ld, lengths, B)) return rc;
    PeakArgs a;
    a.wav = wav; a.ld = ld; a.peak = peak; a.kpre = m->cfg.preemphasis;
    for (int b0 = 0; b0 < B; b0 += MEL_GROUP) {
        const int nb = B - b0 < MEL_GROUP ? B - b0 : MEL_GROUP;
        a.b0 = b0;
        for (int b = 0; b < MEL_GROUP; ++b) a.n[b] = b < nb ? lengths[b0 + b] : 0;
        hipLaunchKernelGGL(wn_mel_peak_kernel, dim3(nb), dim3(1024), 0, (hipStream_t)stream, a);
    }
    WN_LAUNCH_CHECK(m);
    return WN_OK;
}

/* audio.py:70-77 melspectrogram on a ragged batch; out = [B, F_max, num_mels] (the mels/mel-*.npy layout) or [B, num_mels, F_max] (wn_synthesize's c) */
extern "C" int wn_mel_run(wn_mel* m, const float* wav, int64_t ld, const int32_t* lengths, const float* gain, float* out, int32_t B, int32_t F_max,
                          int32_t channels_first, void* stream) {
    if (!m) return WN_E_ARG;
    if (!out) WN_FAIL(m, WN_E_ARG, "wn_mel_run: null argument");
    if (int rc = mel_check_batch(m, "wn_mel_run", wav, ld, lengths, B)) return rc;
    const int hop = m->cfg.hop_size;
    for (int b = 0; b < B; ++b)
        if (F_max < 1 + lengths[b] / hop) WN_FAIL(m, WN_E_SHAPE, "wn_mel_run: F_max (%d) < the %d frames of lengths[%d] = %d", F_max, 1 + lengths[b] / hop, b, lengths[b]);
    const int FR = mel_pick_tile(m, lengths, B);
    int sig_floats = 0;
    const size_t lds_bytes = mel_lds(m, FR, &sig_floats);
    MelArgs a;
    mel_core_args(m->cfg, m->g, m->basis, m->melT, channels_first, sig_floats, &a);
    a.wav = wav; a.ld = ld; a.gain = gain; a.out = out;
    a.F_max = F_max; a.off_lo = m->g.off - m->cfg.n_fft / 2;
    const int TF = FR * 32;
    mel_kernel_t kern = mel_kernel(FR);
    for (int b0 = 0; b0 < B; b0 += MEL_GROUP) {
        const int nb = B - b0 < MEL_GROUP ? B - b0 : MEL_GROUP;
        a.b0 = b0;
        for (int b = 0; b < MEL_GROUP; ++b) a.n[b] = b < nb ? lengths[b0 + b] : 0;
        hipLaunchKernelGGL(kern, dim3((F_max + TF - 1) / TF, nb), dim3(256), lds_bytes, (hipStream_t)stream, a);
    }
    WN_LAUNCH_CHECK(m);
    return WN_OK;
}
