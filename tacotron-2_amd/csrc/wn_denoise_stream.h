// Streaming spectral denoiser: what the device code of wn_denoise_stream.hip, the host hook wn_test_denoise_stream_host and the stand-alone host program
// tests/host/denoise_stream_main.cpp share -- the emit rule, the sizes of a row's state, the validation and planning of a push (host counters only), and the
// whole state machine on host arrays in plain float32, built on dn_host_analyse_at / dn_host_synth_frame of wn_denoise.h.
//
// A row since its restart: S samples given, E emitted.  Not final: the frames f with f hop + H <= S are analysed, fd = floor((S - H) / hop) + 1 of them
// (0 for S < H), and E = max(0, fd hop - H): sample i is emitted once every frame up to floor((i + H) / hop) is.  Final: F = 1 + S / hop frames, zeros
// beyond S, E = S.  What a row carries between pushes:
//   tail   the decoded samples [E, S): exactly those the next frame fd reaches back to (fd hop - H = E when E > 0), fewer than n_fft
//   ring   the windowed frames, frame f in slot f % R; alive are the frames that cover a sample >= E, fewer than ceil(n_fft / hop), and a push adds at
//          most (max_push + H) / hop + 2 (the final push: the frames whose window hangs over the end)
// A push of n samples: frames [fd(S), fd(S + n)) are analysed from tail ++ new samples, out[E(S) ... E(S + n)) is gathered from the ring, frames ascending.
#pragma once
#include "wn_denoise.h"
#include "wn_post.h"

#define DNS_MAX_RESERVE_BYTES (4LL << 30)      // tables + tails + rings + spectrum rows of one handle

__host__ __device__ __forceinline__ int64_t dns_frames_done(int64_t S, int n_fft, int hop, int final) {
    const int64_t H = n_fft / 2;
    if (final) return S > 0 ? 1 + S / hop : 0;      // (a final row of no samples emits nothing and analyses nothing)
    return S >= H ? (S - H) / hop + 1 : 0;
}
__host__ __device__ __forceinline__ int64_t dns_ready(int64_t S, int n_fft, int hop, int final) {
    if (final) return S;
    const int64_t e = dns_frames_done(S, n_fft, hop, 0) * hop - n_fft / 2;
    return e > 0 ? e : 0;
}
static inline int64_t dns_max_new_frames(int64_t n_fft, int64_t hop, int64_t max_push) { return (max_push + n_fft / 2) / hop + 2; }
static inline int64_t dns_ring_slots(int64_t n_fft, int64_t hop, int64_t max_push) { return (n_fft + hop - 1) / hop + dns_max_new_frames(n_fft, hop, max_push); }
static inline int64_t dns_tiles(int64_t n_fft, int64_t hop, int64_t max_push) { return (dns_max_new_frames(n_fft, hop, max_push) + DN_TILE - 1) / DN_TILE; }
// floats per row: two tail halves, the ring, the spectrum rows of the row's tiles
static inline int64_t dns_row_floats(int64_t n_fft, int64_t hop, int64_t max_push) {
    return 2 * n_fft + dns_ring_slots(n_fft, hop, max_push) * n_fft + dns_tiles(n_fft, hop, max_push) * DN_TILE * n_fft;
}

static inline int dns_check_config(const wn_denoise_stream_config* cfg, char* msg, int cap) {
    if (!cfg) WN_DN_FAIL(WN_E_ARG, "null configuration");
    if (cfg->abi_version != WN_ABI_VERSION) WN_DN_FAIL(WN_E_ARG, "abi_version %d != %d", cfg->abi_version, WN_ABI_VERSION);
    if (cfg->max_rows < 0) WN_DN_FAIL(WN_E_ARG, "max_rows (%d) is negative", cfg->max_rows);
    if (cfg->max_push < 1) WN_DN_FAIL(WN_E_ARG, "max_push (%d) must be >= 1", cfg->max_push);
    if (cfg->in_type < 0 || cfg->in_type > 2) WN_DN_FAIL(WN_E_ARG, "in_type (%d) must be 0 (float waveform), 1 (float mu-law) or 2 (int32 class ids)", cfg->in_type);
    const wn_denoise_config g = {cfg->abi_version, cfg->n_fft, cfg->hop, 0, 0};
    if (int rc = wn_denoise_check_config(&g, msg, cap)) return rc;
    const double bytes = 4.0 * ((double)cfg->max_rows * (double)dns_row_floats(cfg->n_fft, cfg->hop, cfg->max_push) + (double)cfg->n_fft * (dn_groups(cfg->n_fft) * 64 + cfg->n_fft + 2));
    if (cfg->max_rows > 0 && bytes > (double)DNS_MAX_RESERVE_BYTES)
        WN_DN_FAIL(WN_E_UNSUPPORTED, "max_rows = %d rows of max_push = %d samples reserve %.0f MiB, above the limit of %lld MiB", cfg->max_rows, cfg->max_push, bytes / 1048576.0,
                   (long long)(DNS_MAX_RESERVE_BYTES >> 20));
    return WN_OK;
}

struct DnsRow { int64_t S = 0; bool ended = false; uint8_t par = 0; };      // par: the tail half the next push reads
// one row of one push, planned from the counters: S0 after the restart, what the device launches and the host hook both work from
struct DnsStep { int64_t S0, S1, E0, E1, fd0, fd1; int32_t n; uint8_t active, final, par; };

// validates a push and plans every row; changes nothing.  max_rows < 0: no limit on B (the host hook)
static inline int dns_plan_push(const char* who, const wn_denoise_stream_config& cfg, int32_t max_rows, bool have_profile, const DnsRow* rows, const void* in, int64_t in_pitch,
                                const int32_t* n, const int32_t* restart, const int32_t* final, int32_t B, float strength, const float* out, int64_t out_pitch, const int32_t* n_out,
                                DnsStep* steps, char* msg, int cap) {
    if (!n || !out || !n_out) WN_DN_FAIL(WN_E_ARG, "%s: null argument", who);
    if (B < 1) WN_DN_FAIL(WN_E_ARG, "%s: B (%d) must be >= 1", who, B);
    if (in_pitch < 0) WN_DN_FAIL(WN_E_ARG, "%s: in_pitch (%lld) is negative", who, (long long)in_pitch);
    if (out_pitch < 0) WN_DN_FAIL(WN_E_ARG, "%s: out_pitch (%lld) is negative", who, (long long)out_pitch);
    bool any = false;
    for (int b = 0; b < B; ++b) {
        if (n[b] < 0) WN_DN_FAIL(WN_E_ARG, "%s: n[%d] = %d is negative", who, b, n[b]);
        any = any || n[b] > 0;
    }
    if (any && !in) WN_DN_FAIL(WN_E_ARG, "%s: null argument (in)", who);
    if (int rc = wn_denoise_check_strength(who, strength, msg, cap)) return rc;
    if (!have_profile) WN_DN_FAIL(WN_E_STATE, "%s: no profile has been set or taken", who);
    if (max_rows >= 0 && B > max_rows) WN_DN_FAIL(WN_E_SHAPE, "%s: B (%d) > max_rows = %d", who, B, max_rows);
    for (int b = 0; b < B; ++b) {
        if (n[b] > cfg.max_push) WN_DN_FAIL(WN_E_SHAPE, "%s: n[%d] = %d > max_push = %d", who, b, n[b], cfg.max_push);
        if (n[b] > in_pitch) WN_DN_FAIL(WN_E_SHAPE, "%s: n[%d] = %d > in_pitch = %lld", who, b, n[b], (long long)in_pitch);
    }
    for (int b = 0; b < B; ++b) {
        DnsStep& s = steps[b];
        const bool rs = restart && restart[b], fin = final && final[b];
        s.n = n[b]; s.final = fin; s.active = n[b] > 0 || fin; s.par = rows[b].par;
        if (s.active && rows[b].ended && !rs) WN_DN_FAIL(WN_E_STATE, "%s: row %d has ended (final): restart[%d] must be set on its next push", who, b, b);
        s.S0 = rs ? 0 : rows[b].S;
        s.S1 = s.S0 + n[b];
        if (s.S1 > 0x7fffffffLL) WN_DN_FAIL(WN_E_SHAPE, "%s: row %d would hold %lld samples since its restart, above 2^31 - 1", who, b, (long long)s.S1);
        s.E0 = dns_ready(s.S0, cfg.n_fft, cfg.hop, 0); s.fd0 = dns_frames_done(s.S0, cfg.n_fft, cfg.hop, 0);
        s.E1 = s.active ? dns_ready(s.S1, cfg.n_fft, cfg.hop, fin) : s.E0; s.fd1 = s.active ? dns_frames_done(s.S1, cfg.n_fft, cfg.hop, fin) : s.fd0;
        if (s.E1 - s.E0 > out_pitch) WN_DN_FAIL(WN_E_SHAPE, "%s: out_pitch (%lld) < n_out[%d] = %lld", who, (long long)out_pitch, b, (long long)(s.E1 - s.E0));
    }
    return WN_OK;
}
// the counters after a planned push, and n_out
static inline void dns_commit_push(DnsRow* rows, const DnsStep* steps, const int32_t* restart, int32_t B, int32_t* n_out) {
    for (int b = 0; b < B; ++b) {
        const DnsStep& s = steps[b];
        n_out[b] = (int32_t)(s.E1 - s.E0);
        if (restart && restart[b]) { rows[b].S = 0; rows[b].ended = false; }
        if (!s.active) continue;
        rows[b].S = s.S1;
        if (s.final) rows[b].ended = true; else rows[b].par ^= 1;      // (a final push stores no tail)
    }
}

// ---- host: the state machine on host arrays
struct DnsHostRow { std::vector<float> tail, ring; };      // tail: the samples [E, S); ring: [R][n_fft]

// one planned row of one push: in = the row's n new elements of in_type, out receives E1 - E0 samples
static inline void dns_host_row(const DnTables& t, const wn_denoise_stream_config& cfg, const float* profile, float strength, const DnsStep& s, DnsHostRow* st, const void* in, float* out) {
#pragma clang fp contract(off)
    if (s.S0 == 0) st->tail.clear();      // restarted (or never started): nothing carried
    if (!s.active) return;
    const int N = cfg.n_fft, H = N / 2, hop = cfg.hop;
    const int64_t R = dns_ring_slots(N, hop, cfg.max_push);
    if (st->ring.empty()) st->ring.assign((size_t)R * N, 0.0f);
    std::vector<float> span(st->tail);    // the samples [E0, S1)
    for (int32_t i = 0; i < s.n; ++i) span.push_back(wn_post_decode(cfg.in_type, ((const int32_t*)in)[i]));
    std::vector<float> spec((size_t)2 * N), ch((size_t)4 * N);
    for (int64_t f = s.fd0; f < s.fd1; ++f) {
        dn_host_analyse_at(t, hop, span.data(), s.E0, s.S1, f, spec.data());
        dn_host_synth_frame(t, profile, strength, spec.data(), ch.data(), &st->ring[(size_t)(f % R) * N]);
    }
    for (int64_t i = s.E0; i < s.E1; ++i) {
        const int64_t f_lo = i >= H ? (i - H) / hop + 1 : 0, f_hi = (i + H) / hop < s.fd1 - 1 ? (i + H) / hop : s.fd1 - 1;
        float num = 0.0f, den = 0.0f;
        for (int64_t f = f_lo; f <= f_hi; ++f) { const int64_t j = i - f * hop + H; num = num + st->ring[(size_t)(f % R) * N + j]; den = den + t.wsq[j]; }
        out[i - s.E0] = num / den;
    }
    if (s.final) st->tail.clear();
    else st->tail.assign(span.begin() + (s.E1 - s.E0), span.end());      // [E1, S1)
}
