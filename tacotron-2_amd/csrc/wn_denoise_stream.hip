// Streaming spectral denoiser (wn_denoise_stream_* of include/wavenet_mi355.h; the rule, the state of a row and the host side: wn_denoise_stream.h): the
// denoiser of wn_denoise.hip on rows that arrive push by push, bit-identical to wn_denoise_run of the whole row however it is cut.
//
// Two launches per push and group of 64 rows.  The tile kernel: one workgroup owns up to DN_TILE = 32 NEW frames of one row (frames fd0 + 32 x ... of the
// push; a push of 8 mel frames adds about 9, so one mostly empty tile per row -- frames of several rows are not packed into one tile).  It stages the
// span of its frames in LDS -- below S0 from the row's carried tail, from S0 on the push's samples decoded by wn_post_decode, zero outside [0, S1) -- and
// runs the forward product, shrink and inverse product of wn_denoise_dev.h exactly as wn_denoise_tile_kernel does: every (frame, bin) and (frame, sample)
// is its own row of the matrix instruction, so which tile a frame ran in leaves no trace in its bits.  Frames below fd1 go to the row's ring (slot
// f % R), the rest of the tile is computed and dropped.  Tile 0 of a row also writes the row's new tail [E1, S1) -- into the OTHER half of the row's tail
// buffer: the tiles of one row read the old half concurrently, so no order between workgroups is needed and none is assumed.
// The gather kernel: one lane per emitted sample i in [E0, E1) sums the covering frames from the ring in ascending f, the window squares of the same
// frames in the same order, and divides -- wn_denoise_gather_kernel with the ring in place of the frame workspace.
// The counters (S per row, ended, tail half) live on the host; S0, n and the flags travel as kernel arguments, everything else follows from them on both
// sides by the same functions.  No atomics, no allocation, no synchronisation in a push.
#define WN_POST_HOST_TABLES
#include "wn_denoise_stream.h"
#include "wn_denoise_dev.h"

struct wn_denoise_stream {
    wn_denoise_stream_config cfg;
    std::string err;
    int NB = 0, G = 0, ldb = 0, R = 0, tiles = 0;
    size_t lds_bytes = 0;
    bool have_profile = false;
    std::vector<DnsRow> rows;              // the counters, max_rows of them (a geometry-only handle keeps DN_GROUP so that a push can be planned)
    std::vector<DnsStep> steps;
    DevBuf<float> fb, ib, wsq, prof;       // the two tables, w^2, the profile [NB]
    DevBuf<float> tail, ring, spec;        // [max_rows][2][n_fft], [max_rows][R][n_fft], [max_rows][tiles][32][n_fft]
};

#define DNS_ACTIVE 1
#define DNS_FINAL 2
#define DNS_PAR 4

struct DnsArgs {
    const void* in; const float* fb; const float* ib; const float* prof; float* spec; float* ring; float* tail;
    int64_t in_pitch;
    int32_t b0, n_fft, hop, G, ldb, sig_floats, R, tiles, in_type;
    float strength;
    int32_t S0[DN_GROUP], n[DN_GROUP];
    uint8_t flags[DN_GROUP];
};

__global__ __launch_bounds__(DN_THREADS) void wn_denoise_stream_tile_kernel(const DnsArgs a) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int b = blockIdx.y, N = a.n_fft, H = N / 2, hop = a.hop, flags = a.flags[b];
    if (!(flags & DNS_ACTIVE)) return;
    const int final = (flags & DNS_FINAL) ? 1 : 0;
    const int64_t row = a.b0 + b;
    const int64_t S0 = a.S0[b], S1 = S0 + a.n[b];
    const int64_t E0 = dns_ready(S0, N, hop, 0), fd0 = dns_frames_done(S0, N, hop, 0), fd1 = dns_frames_done(S1, N, hop, final);
    const float* told = a.tail + (row * 2 + ((flags & DNS_PAR) ? 1 : 0)) * N;      // the samples [E0, S0)
    const int32_t* x = (const int32_t*)a.in + row * a.in_pitch;                    // the samples [S0, S1), as their 32 bits
    if (blockIdx.x == 0 && !final) {      // the new tail [E1, S1) into the other half (E1 >= E0; fewer than n_fft samples)
        float* tnew = a.tail + (row * 2 + ((flags & DNS_PAR) ? 0 : 1)) * N;
        const int64_t E1 = dns_ready(S1, N, hop, 0);
        for (int64_t s = E1 + tid; s < S1; s += DN_THREADS) tnew[s - E1] = s < S0 ? told[s - E0] : wn_post_decode(a.in_type, x[s - S0]);
    }
    const int64_t f0 = fd0 + (int64_t)blockIdx.x * DN_TILE;
    if (f0 >= fd1) return;      // no new frame in this tile (block-uniform: no barrier has been reached)
    float* sig = lds;
    {
        const int64_t s0 = f0 * hop - H;      // s0 >= E0 wherever s0 >= 0: the tail reaches back far enough
        for (int i = tid; i < a.sig_floats; i += DN_THREADS) {
            const int64_t s = s0 + i;
            sig[i] = (s >= 0 && s < S1) ? (s < S0 ? told[s - E0] : wn_post_decode(a.in_type, x[s - S0])) : 0.0f;
        }
    }
    __syncthreads();
    float* Y = a.spec + ((row * a.tiles + blockIdx.x) * DN_TILE) * N;      // this tile's 32 packed spectrum rows
    const float* sp = sig + l31 * hop + lh;
    for (int g = wave; g < a.G; g += 4) {        // (wave-uniform; no workgroup barrier inside)
        f32x16_t re, im;
        dn_forward_group(sp, a.fb + (size_t)lh * a.ldb + g * 64 + l31, a.ldb, N, &re, &im);
        dn_shrink_group(re, im, Y, a.prof, a.strength, g, N, l31, lh);
    }
    __syncthreads();      // the tile's spectrum rows are complete and visible to the workgroup that wrote them
    float* ring = a.ring + row * a.R * N;
    const float* yp = Y + (size_t)l31 * N + lh * 4;
    for (int jg = wave; jg < N / 32; jg += 4) {
        f32x16_t y;
        dn_inverse_group(yp, a.ib + (size_t)lh * N + jg * 32 + l31, N, &y);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t f = f0 + dn_acc_frame(r, lh);
            if (f < fd1) ring[(f % a.R) * N + jg * 32 + l31] = y[r];
        }
    }
}

struct DnsGatherArgs {
    const float* ring; const float* wsq; float* out;
    int64_t out_pitch;
    int32_t b0, n_fft, hop, R;
    int32_t S0[DN_GROUP], n[DN_GROUP];
    uint8_t flags[DN_GROUP];
};

__global__ __launch_bounds__(DN_THREADS) void wn_denoise_stream_gather_kernel(const DnsGatherArgs a) {
    const int b = blockIdx.y, N = a.n_fft, H = N / 2, hop = a.hop, flags = a.flags[b];
    if (!(flags & DNS_ACTIVE)) return;
    const int final = (flags & DNS_FINAL) ? 1 : 0;
    const int64_t S0 = a.S0[b], S1 = S0 + a.n[b];
    const int64_t E0 = dns_ready(S0, N, hop, 0), E1 = dns_ready(S1, N, hop, final), fd1 = dns_frames_done(S1, N, hop, final);
    const int64_t i = E0 + (int64_t)blockIdx.x * DN_THREADS + threadIdx.x;
    if (i >= E1) return;
    const int64_t row = a.b0 + b;
    const int64_t f_lo = i >= H ? (i - H) / hop + 1 : 0, f_hi = (i + H) / hop < fd1 - 1 ? (i + H) / hop : fd1 - 1;
    const float* fr = a.ring + row * a.R * N;
    float num = 0.0f, den = 0.0f;
    for (int64_t f = f_lo; f <= f_hi; ++f) {      // j = i - f hop + H lies in [0, n_fft) for exactly these f
        const int64_t j = i - f * hop + H;
        num = __fadd_rn(num, fr[(f % a.R) * N + j]);
        den = __fadd_rn(den, a.wsq[j]);
    }
    a.out[row * a.out_pitch + (i - E0)] = __fdiv_rn(num, den);
}

#define DNS_PROF_CHUNK 512
struct DnsProfArgs { float* dst; int32_t off, cnt; float v[DNS_PROF_CHUNK]; };

__global__ __launch_bounds__(DNS_PROF_CHUNK) void wn_denoise_stream_set_profile_kernel(const DnsProfArgs a) {
    if ((int)threadIdx.x < a.cnt) a.dst[a.off + threadIdx.x] = a.v[threadIdx.x];
}

extern "C" int wn_denoise_stream_create(const wn_denoise_stream_config* cfg, wn_denoise_stream** out) {
    wn_denoise_stream* z = nullptr;
    if (!cfg || !out) WN_FAIL(z, WN_E_ARG, "wn_denoise_stream_create: null argument");
    *out = nullptr;
    char msg[256];
    if (int rc = dns_check_config(cfg, msg, sizeof msg)) WN_FAIL(z, rc, "wn_denoise_stream_create: %s", msg);
    wn_denoise_stream* d = new wn_denoise_stream();
    d->cfg = *cfg;
    d->NB = dn_bins(cfg->n_fft); d->G = dn_groups(cfg->n_fft); d->ldb = d->G * 64;
    d->R = (int)dns_ring_slots(cfg->n_fft, cfg->hop, cfg->max_push); d->tiles = (int)dns_tiles(cfg->n_fft, cfg->hop, cfg->max_push);
    d->lds_bytes = (size_t)dn_sig_floats(cfg->n_fft, cfg->hop) * sizeof(float);      // <= 160 KiB for every geometry dns_check_config admits
    d->rows.resize(cfg->max_rows > 0 ? cfg->max_rows : DN_GROUP);
    d->steps.resize(d->rows.size());
    *out = d;
    if (cfg->max_rows == 0) return WN_OK;      // geometry-only handle: reserves nothing and never touches a device; a push refuses any B
    DnTables t;
    dn_build_tables(cfg->n_fft, &t);
    const size_t N = (size_t)cfg->n_fft, rows = (size_t)cfg->max_rows;
    int rc = [&]() -> int {
        WN_HIP(d, d->fb.reserve(t.fb.size()));
        WN_HIP(d, d->ib.reserve(t.ib.size()));
        WN_HIP(d, d->wsq.reserve(t.wsq.size()));
        WN_HIP(d, d->prof.reserve((size_t)d->NB));
        WN_HIP(d, d->tail.reserve(rows * 2 * N));
        WN_HIP(d, d->ring.reserve(rows * d->R * N));
        WN_HIP(d, d->spec.reserve(rows * d->tiles * DN_TILE * N));
        WN_HIP(d, hipMemcpy(d->fb, t.fb.data(), t.fb.size() * 4, hipMemcpyHostToDevice));
        WN_HIP(d, hipMemcpy(d->ib, t.ib.data(), t.ib.size() * 4, hipMemcpyHostToDevice));
        WN_HIP(d, hipMemcpy(d->wsq, t.wsq.data(), t.wsq.size() * 4, hipMemcpyHostToDevice));
        // the attribute belongs to the function, not to this handle: always the 160 KiB cap
        WN_HIP(d, hipFuncSetAttribute((const void*)wn_denoise_stream_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        return WN_OK;
    }();
    if (rc != WN_OK) { g_create_err = d->err; delete d; *out = nullptr; return rc; }
    return WN_OK;
}

extern "C" void wn_denoise_stream_destroy(wn_denoise_stream* d) { delete d; }

extern "C" const char* wn_denoise_stream_last_error(const wn_denoise_stream* d) { return d ? d->err.c_str() : g_create_err.c_str(); }

extern "C" int64_t wn_denoise_stream_ready(const wn_denoise_stream* d, int64_t S, int32_t final) {
    if (!d || S < 0) return (int64_t)WN_E_ARG;
    return dns_ready(S, d->cfg.n_fft, d->cfg.hop, final ? 1 : 0);
}

extern "C" int wn_denoise_stream_set_profile(wn_denoise_stream* d, const float* profile, void* stream) {
    if (!d) return WN_E_ARG;
    char msg[256];
    if (int rc = wn_denoise_check_profile("wn_denoise_stream_set_profile", profile, d->NB, msg, sizeof msg)) WN_FAIL(d, rc, "%s", msg);
    if (d->cfg.max_rows > 0) {      // the values travel as kernel arguments, as wn_denoise_set_profile's
        DnsProfArgs a;
        a.dst = d->prof;
        for (int off = 0; off < d->NB; off += DNS_PROF_CHUNK) {
            a.off = off; a.cnt = d->NB - off < DNS_PROF_CHUNK ? d->NB - off : DNS_PROF_CHUNK;
            memcpy(a.v, profile + off, (size_t)a.cnt * 4);
            hipLaunchKernelGGL(wn_denoise_stream_set_profile_kernel, dim3(1), dim3(DNS_PROF_CHUNK), 0, (hipStream_t)stream, a);
            WN_LAUNCH_CHECK(d);
        }
    }
    d->have_profile = true;
    return WN_OK;
}

extern "C" int wn_denoise_stream_take_profile(wn_denoise_stream* d, const wn_denoise* src, void* stream) {
    if (!d) return WN_E_ARG;
    if (!src) WN_FAIL(d, WN_E_ARG, "wn_denoise_stream_take_profile: null argument");
    int32_t n_fft = 0;
    const float* dev = nullptr; const float* host = nullptr;
    if (wn_denoise_profile_source(src, &n_fft, &dev, &host) != WN_OK) WN_FAIL(d, WN_E_STATE, "wn_denoise_stream_take_profile: the source has no profile (fit or set it first)");
    if (n_fft != d->cfg.n_fft) WN_FAIL(d, WN_E_SHAPE, "wn_denoise_stream_take_profile: the source's n_fft (%d) != n_fft = %d", n_fft, d->cfg.n_fft);
    if (host) return wn_denoise_stream_set_profile(d, host, stream);      // a geometry-only source keeps its profile on the host
    if (d->cfg.max_rows > 0) WN_HIP(d, hipMemcpyAsync(d->prof, dev, (size_t)d->NB * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    d->have_profile = true;
    return WN_OK;
}

extern "C" int wn_denoise_stream_push(wn_denoise_stream* d, const void* in, int64_t in_pitch, const int32_t* n, const int32_t* restart, const int32_t* final, int32_t B,
                                      float strength, float* out, int64_t out_pitch, int32_t* n_out, void* stream) {
    if (!d) return WN_E_ARG;
    char msg[256];
    // (B is checked against max_rows before any row is indexed: a geometry-only handle refuses every push there)
    if (int rc = dns_plan_push("wn_denoise_stream_push", d->cfg, d->cfg.max_rows, d->have_profile, d->rows.data(), in, in_pitch, n, restart, final, B, strength, out, out_pitch,
                               n_out, d->steps.data(), msg, sizeof msg))
        WN_FAIL(d, rc, "%s", msg);
    hipStream_t st = (hipStream_t)stream;
    DnsArgs a;
    a.in = in; a.fb = d->fb; a.ib = d->ib; a.prof = d->prof; a.spec = d->spec; a.ring = d->ring; a.tail = d->tail;
    a.in_pitch = in_pitch; a.n_fft = d->cfg.n_fft; a.hop = d->cfg.hop; a.G = d->G; a.ldb = d->ldb; a.sig_floats = (int32_t)dn_sig_floats(d->cfg.n_fft, d->cfg.hop);
    a.R = d->R; a.tiles = d->tiles; a.in_type = d->cfg.in_type; a.strength = strength;
    DnsGatherArgs g;
    g.ring = d->ring; g.wsq = d->wsq; g.out = out; g.out_pitch = out_pitch; g.n_fft = d->cfg.n_fft; g.hop = d->cfg.hop; g.R = d->R;
    for (int b0 = 0; b0 < B; b0 += DN_GROUP) {
        const int nb = B - b0 < DN_GROUP ? B - b0 : DN_GROUP;
        int64_t tiles = 0, emit = 0;
        bool any = false;
        a.b0 = g.b0 = b0;
        for (int r = 0; r < DN_GROUP; ++r) {
            a.S0[r] = g.S0[r] = 0; a.n[r] = g.n[r] = 0; a.flags[r] = g.flags[r] = 0;
            if (r >= nb || !d->steps[b0 + r].active) continue;
            const DnsStep& s = d->steps[b0 + r];
            a.S0[r] = g.S0[r] = (int32_t)s.S0; a.n[r] = g.n[r] = s.n;
            a.flags[r] = g.flags[r] = (uint8_t)(DNS_ACTIVE | (s.final ? DNS_FINAL : 0) | (s.par ? DNS_PAR : 0));
            const int64_t tl = cdiv(s.fd1 - s.fd0, DN_TILE);
            if (tl > tiles) tiles = tl;
            if (s.E1 - s.E0 > emit) emit = s.E1 - s.E0;
            any = true;
        }
        if (!any) continue;      // rows that are left alone launch nothing
        hipLaunchKernelGGL(wn_denoise_stream_tile_kernel, dim3((unsigned)(tiles > 0 ? tiles : 1), nb), dim3(DN_THREADS), d->lds_bytes, st, a);      // (tile 0 stores the tail even without a new frame)
        WN_LAUNCH_CHECK(d);
        if (emit == 0) continue;
        hipLaunchKernelGGL(wn_denoise_stream_gather_kernel, dim3(cdiv(emit, DN_THREADS), nb), dim3(DN_THREADS), 0, st, g);
        WN_LAUNCH_CHECK(d);
    }
    dns_commit_push(d->rows.data(), d->steps.data(), restart, B, n_out);
    return WN_OK;
}

extern "C" int wn_test_denoise_stream_host(const wn_denoise_stream_config* cfg, const float* profile, float strength, const void* in, int64_t in_pitch, const int32_t* n,
                                           const int32_t* restart, const int32_t* final, int32_t P, int32_t B, float* out, int64_t out_pitch, int32_t* n_out) {
    wn_denoise_stream* z = nullptr;
    char msg[256];
    if (int rc = dns_check_config(cfg, msg, sizeof msg)) WN_FAIL(z, rc, "wn_test_denoise_stream_host: %s", msg);
    if (P < 0 || B < 1) WN_FAIL(z, WN_E_ARG, "wn_test_denoise_stream_host: P (%d) must be >= 0 and B (%d) >= 1", P, B);
    if (int rc = wn_denoise_check_profile("wn_test_denoise_stream_host", profile, dn_bins(cfg->n_fft), msg, sizeof msg)) WN_FAIL(z, rc, "%s", msg);
    if (P > 0 && (!n || !out || !n_out)) WN_FAIL(z, WN_E_ARG, "wn_test_denoise_stream_host: null argument");
    DnTables t;
    dn_build_tables(cfg->n_fft, &t);
    std::vector<DnsRow> rows((size_t)B);
    std::vector<DnsStep> steps((size_t)B);
    std::vector<DnsHostRow> st((size_t)B);
    for (int64_t p = 0; p < P; ++p) {
        const int32_t* np = n + p * B; const int32_t* rp = restart ? restart + p * B : nullptr; const int32_t* fp = final ? final + p * B : nullptr;
        const int32_t* ip = in ? (const int32_t*)in + p * B * in_pitch : nullptr;
        float* op = out + p * B * out_pitch;
        if (int rc = dns_plan_push("wn_test_denoise_stream_host", *cfg, -1, true, rows.data(), ip, in_pitch, np, rp, fp, B, strength, op, out_pitch, n_out + p * B, steps.data(), msg,
                                   sizeof msg))
            WN_FAIL(z, rc, "push %lld: %s", (long long)p, msg);
        for (int b = 0; b < B; ++b) dns_host_row(t, *cfg, profile, strength, steps[b], &st[b], ip ? ip + (int64_t)b * in_pitch : nullptr, op + (int64_t)b * out_pitch);
        dns_commit_push(rows.data(), steps.data(), rp, B, n_out + p * B);
    }
    return WN_OK;
}
