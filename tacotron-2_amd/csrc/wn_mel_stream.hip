// Streaming mel analysis (wn_mel_stream_* of include/wavenet_mi355.h; the rule, the state of a row and the host side: wn_mel_stream.h): the analysis of
// wn_mel.hip on rows that arrive push by push, bit-identical to wn_mel_run of the whole row however it is cut.
//
// One launch per push and group of 64 rows.  One workgroup owns up to MELS_TILE = 32 NEW frames of one row (frames F0 + 32 x ... of the push; a tile's first
// frame is wherever the row stands, not a multiple of 32).  It stages the span of its frames in LDS -- below S0 from the row's carried tail, which is already
// in the analysed domain, from S0 on y = gain (x[s] - k x[s - 1]) of the push's samples with the three separately rounded operations of wn_mel_kernel, zero
// outside [0, S1) -- and runs mel_core of wn_mel.h exactly as wn_mel_kernel<1> does: every (frame, bin) and (frame, mel) is its own row / column of the matrix
// instruction, so which tile a frame ran in leaves no trace in its bits.  Frames below F1 are stored at out[f - F0]; the rest of the tile is computed and
// dropped.  Tile 0 of a row also writes the row's new tail y[T1, S1) and the raw sample x[S1 - 1] -- into the OTHER half of the row's tail buffer: the tiles
// of one row read the old half concurrently, so no order between workgroups is needed and none is assumed.
// The counters (S, F, the latched gain, ended, tail half) live on the host and travel as kernel arguments.  No atomics, no allocation, no synchronisation.
#include "wn_mel.h"
#include "wn_mel_stream.h"

struct wn_mel_stream {
    wn_mel_config cfg;
    std::string err;
    MelGeom g;
    MelsGeom sg;
    int32_t max_rows = 0, max_push = 0, tp = 0, sig_floats = 0;      // tp: floats of a tail half -- [0] the raw sample x[S - 1], [1 ...] y[T, S)
    size_t lds_bytes = 0;
    std::vector<MelsRow> rows;             // the counters, max_rows of them
    std::vector<MelsStep> steps;
    DevBuf<float> basis, melT, tail;       // the two tables of wn_mel; [max_rows][2][tp]
};

#define MELS_ACTIVE 1
#define MELS_FINAL 2
#define MELS_PAR 4

struct MelsArgs {
    const float* basis; const float* melT;
    int32_t channels_first, hop, win_pad, nchunks, ldb, num_mels, mt, ldm, sig_floats;
    float kpre, pow_half; int32_t pow_mode;
    float min_lin, ref_db, lo, maxabs; int32_t norm, clip, symmetric;
    const float* in; float* out; float* tail;
    int64_t in_pitch, out_pitch;
    MelsGeom g;
    int32_t b0, tp;
    int32_t S0[MEL_GROUP], n[MEL_GROUP], F0[MEL_GROUP];
    float gain[MEL_GROUP];
    uint8_t flags[MEL_GROUP];
};

__global__ __launch_bounds__(256) void wn_mel_stream_kernel(const MelsArgs a) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int b = blockIdx.y, flags = a.flags[b];
    if (!(flags & MELS_ACTIVE)) return;
    const int final = (flags & MELS_FINAL) ? 1 : 0;
    const int64_t row = a.b0 + b;
    const int64_t S0 = a.S0[b], S1 = S0 + a.n[b], F0 = a.F0[b], F1 = mels_ready(a.g, S1, final);
    const int64_t T0 = mels_tail_at(a.g, F0, S0);
    const float* told = a.tail + (row * 2 + ((flags & MELS_PAR) ? 1 : 0)) * a.tp;      // [0]: x[S0 - 1]; [1 ...]: y[T0, S0)
    const float* x = a.in + row * a.in_pitch;                                           // the samples [S0, S1)
    const float gain = a.gain[b], kpre = a.kpre;
    const float carry = S0 > 0 ? told[0] : 0.0f;                                        // x[-1] = 0 at a restart
    auto y = [&](int64_t s) -> float {      // T0 <= s < S1
        if (s < S0) return told[1 + (s - T0)];
        const int64_t i = s - S0;
        return __fmul_rn(gain, mel_preem_pair(x[i], i > 0 ? x[i - 1] : carry, kpre));
    };
    if (blockIdx.x == 0 && !final) {      // the new tail y[T1, S1) and x[S1 - 1] into the other half (fewer than win_size samples; a push that is not final has n > 0)
        float* tnew = a.tail + (row * 2 + ((flags & MELS_PAR) ? 0 : 1)) * a.tp;
        const int64_t T1 = mels_tail_at(a.g, F1, S1);      // T1 >= T0
        for (int64_t s = T1 + tid; s < S1; s += 256) tnew[1 + (s - T1)] = y(s);
        if (tid == 0) tnew[0] = x[a.n[b] - 1];
    }
    const int64_t f0 = F0 + (int64_t)blockIdx.x * MELS_TILE;
    if (f0 >= F1) return;      // no new frame in this tile (block-uniform: no barrier has been reached)
    {
        const int64_t s0 = f0 * a.g.hop - a.g.Hl;      // s0 >= T0 wherever s0 >= 0 and a carried sample is read: the tail reaches back far enough
        for (int i = tid; i < a.sig_floats; i += 256) {
            const int64_t s = s0 + i;
            lds[i] = (s >= 0 && s < S1) ? y(s) : 0.0f;
        }
    }
    __syncthreads();
    const int64_t nf = F1 - f0;
    auto store = [&](int f, int m, float v) {
        if (f >= nf) return;      // beyond the push's frames: the caller's bytes stay
        const int64_t fo = f0 + f - F0;
        if (a.channels_first) a.out[(row * a.num_mels + m) * a.out_pitch + fo] = v;
        else a.out[(row * a.out_pitch + fo) * a.num_mels + m] = v;
    };
    mel_core<1>(a, lds, nf < MELS_TILE ? (int)nf : MELS_TILE, 0.0f, store);
}

extern "C" int wn_mel_stream_create(const wn_mel_config* cfg, const float* mel_basis, int32_t max_rows, int32_t max_push, wn_mel_stream** out) {
    wn_mel_stream* z = nullptr;
    if (!cfg || !out) WN_FAIL(z, WN_E_ARG, "wn_mel_stream_create: null argument");
    *out = nullptr;
    if (cfg->abi_version != WN_ABI_VERSION) WN_FAIL(z, WN_E_ARG, "wn_mel_stream_create: abi_version %d != %d", cfg->abi_version, WN_ABI_VERSION);
    if (!mel_basis) WN_FAIL(z, WN_E_ARG, "wn_mel_stream_create: mel_basis is null");
    char msg[256];
    if (int rc = mel_check_geometry(cfg, msg, sizeof msg)) WN_FAIL(z, rc, "wn_mel_stream_create: %s", msg);
    if (cfg->n_fft > (1 << 16)) WN_FAIL(z, WN_E_UNSUPPORTED, "wn_mel_stream_create: n_fft (%d) > 65536", cfg->n_fft);
    if (int rc = mels_check_sizes(max_rows, max_push, msg, sizeof msg)) WN_FAIL(z, rc, "wn_mel_stream_create: %s", msg);
    const MelGeom g = mel_geom(*cfg);
    int sig_floats = 0;
    const size_t lds_bytes = mel_lds(*cfg, g, 1, &sig_floats);
    if (lds_bytes > 160 * 1024)
        WN_FAIL(z, WN_E_UNSUPPORTED, "wn_mel_stream_create: hop_size %d / win_size %d: the signal span of a 32-frame tile does not fit the 160 KiB LDS", cfg->hop_size, cfg->win_size);
    wn_mel_stream* h = new wn_mel_stream();
    h->cfg = *cfg; h->cfg.max_batch = 0; h->cfg.max_samples = 0;
    h->g = g; h->sg = mels_geom(cfg->n_fft, cfg->win_size, cfg->hop_size);
    h->max_rows = max_rows; h->max_push = max_push; h->tp = cfg->win_size + 1; h->sig_floats = sig_floats; h->lds_bytes = lds_bytes;
    h->rows.resize((size_t)max_rows);
    h->steps.resize((size_t)max_rows);
    *out = h;
    if (max_rows == 0) return WN_OK;      // geometry-only handle: reserves nothing and never touches a device; a push refuses any B
    std::vector<float> hb, hm;
    mel_build_tables(*cfg, g, mel_basis, &hb, &hm);
    int rc = [&]() -> int {
        WN_HIP(h, h->basis.reserve(hb.size()));
        WN_HIP(h, h->melT.reserve(hm.size()));
        WN_HIP(h, h->tail.reserve((size_t)max_rows * 2 * (size_t)h->tp));
        WN_HIP(h, hipMemcpy(h->basis, hb.data(), hb.size() * 4, hipMemcpyHostToDevice));
        WN_HIP(h, hipMemcpy(h->melT, hm.data(), hm.size() * 4, hipMemcpyHostToDevice));
        // the attribute belongs to the function, not to this handle: always the 160 KiB cap
        WN_HIP(h, hipFuncSetAttribute((const void*)wn_mel_stream_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        return WN_OK;
    }();
    if (rc != WN_OK) { g_create_err = h->err; delete h; *out = nullptr; return rc; }
    return WN_OK;
}

extern "C" void wn_mel_stream_destroy(wn_mel_stream* h) { delete h; }

extern "C" const char* wn_mel_stream_last_error(const wn_mel_stream* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

extern "C" int64_t wn_mel_stream_ready(const wn_mel_stream* h, int64_t S, int32_t final) {
    if (!h || S < 0 || S > 0x7fffffffLL) return (int64_t)WN_E_ARG;
    return mels_ready(h->sg, S, final ? 1 : 0);
}

extern "C" int wn_mel_stream_push(wn_mel_stream* h, const float* in, int64_t in_pitch, const int32_t* n, const int32_t* restart, const int32_t* final, const float* gain, int32_t B,
                                  float* out, int64_t out_pitch, int32_t channels_first, int32_t* n_out, void* stream) {
    if (!h) return WN_E_ARG;
    char msg[256];
    // (B is checked against max_rows before any row is indexed: a geometry-only handle refuses every push there)
    if (int rc = mels_plan_push("wn_mel_stream_push", h->sg, h->max_rows, h->max_push, h->rows.data(), in, in_pitch, n, restart, final, gain, B, out, out_pitch, n_out,
                                h->steps.data(), msg, sizeof msg))
        WN_FAIL(h, rc, "%s", msg);
    MelsArgs a;
    mel_core_args(h->cfg, h->g, h->basis, h->melT, channels_first, h->sig_floats, &a);
    a.in = in; a.out = out; a.tail = h->tail; a.in_pitch = in_pitch; a.out_pitch = out_pitch; a.g = h->sg; a.tp = h->tp;
    for (int b0 = 0; b0 < B; b0 += MEL_GROUP) {
        const int nb = B - b0 < MEL_GROUP ? B - b0 : MEL_GROUP;
        int64_t tiles = 0;
        bool any = false;
        a.b0 = b0;
        for (int r = 0; r < MEL_GROUP; ++r) {
            a.S0[r] = 0; a.n[r] = 0; a.F0[r] = 0; a.gain[r] = 1.0f; a.flags[r] = 0;
            if (r >= nb || !h->steps[b0 + r].active) continue;
            const MelsStep& s = h->steps[b0 + r];
            a.S0[r] = (int32_t)s.S0; a.n[r] = s.n; a.F0[r] = (int32_t)s.F0; a.gain[r] = s.gain;
            a.flags[r] = (uint8_t)(MELS_ACTIVE | (s.final ? MELS_FINAL : 0) | (s.par ? MELS_PAR : 0));
            const int64_t tl = (s.F1 - s.F0 + MELS_TILE - 1) / MELS_TILE;
            if (tl > tiles) tiles = tl;
            any = true;
        }
        if (!any) continue;      // rows that are left alone launch nothing
        hipLaunchKernelGGL(wn_mel_stream_kernel, dim3((unsigned)(tiles > 0 ? tiles : 1), nb), dim3(256), h->lds_bytes, (hipStream_t)stream, a);      // (tile 0 stores the tail even without a new frame)
        WN_LAUNCH_CHECK(h);
    }
    mels_commit_push(h->rows.data(), h->steps.data(), restart, B, n_out);
    return WN_OK;
}

extern "C" int wn_test_mel_stream_plan(const wn_mel_stream* h, const float* in, int64_t in_pitch, const int32_t* n, const int32_t* restart, const int32_t* final, int32_t P, int32_t B,
                                       int64_t out_pitch, int32_t* status, int32_t* n_out, int64_t* first_frame, int32_t* tail_len, int64_t* S, int64_t* F) {
    wn_mel_stream* z = nullptr;
    if (!h) return WN_E_ARG;
    if (h->max_rows != 0) WN_FAIL(z, WN_E_STATE, "wn_test_mel_stream_plan: the handle must be geometry-only (max_rows = 0)");
    if (P < 0 || B < 1) WN_FAIL(z, WN_E_ARG, "wn_test_mel_stream_plan: P (%d) must be >= 0 and B (%d) >= 1", P, B);
    if (P > 0 && (!status || !n_out || !first_frame || !tail_len || !S || !F)) WN_FAIL(z, WN_E_ARG, "wn_test_mel_stream_plan: null argument");
    std::vector<MelsRow> rows((size_t)B);
    std::vector<MelsStep> steps((size_t)B);
    const float dummy = 0.0f;      // (the plan only tests `out` against NULL)
    char msg[256];
    for (int64_t p = 0; p < P; ++p) {
        const int32_t* np = n ? n + p * B : nullptr; const int32_t* rp = restart ? restart + p * B : nullptr; const int32_t* fp = final ? final + p * B : nullptr;
        status[p] = mels_plan_push("wn_test_mel_stream_plan", h->sg, -1, h->max_push, rows.data(), in, in_pitch, np, rp, fp, nullptr, B, &dummy, out_pitch, n_out + p * B,
                                   steps.data(), msg, sizeof msg);
        if (status[p] == WN_OK) mels_commit_push(rows.data(), steps.data(), rp, B, n_out + p * B);      // a refused push changes no row
        for (int b = 0; b < B; ++b) {
            if (status[p] != WN_OK) n_out[p * B + b] = 0;
            first_frame[p * B + b] = status[p] == WN_OK ? steps[b].F0 : rows[b].F;
            S[p * B + b] = rows[b].S; F[p * B + b] = rows[b].F;
            tail_len[p * B + b] = rows[b].ended ? 0 : (int32_t)(rows[b].S - mels_tail_at(h->sg, rows[b].F, rows[b].S));
        }
    }
    return WN_OK;
}
