// Stand-alone host check of the streaming denoiser's host side (csrc/wn_denoise_stream.h: the emit rule, the validation and planning of a push, and the
// state machine with its input tail and frame ring on host arrays), built with -fsanitize=address,undefined and run as an ordinary program by
// tests/test_denoise_stream_cpu.py.  Every buffer is a heap block of exactly the needed size -- a push's n samples, a push's n_out outputs -- so a read
// past a push's samples, a write past what a push emits, or a ring / tail index out of range is the sanitizer's to report.  Rows are driven through ragged
// cuttings, restarts and finals and compared, bit for bit, with wn_denoise_host_run of the whole row.  Prints one "code <name> <value>" line per
// validation case (the test compares them) and "denoise stream ok".
#define WN_POST_HOST_TABLES
#include "wn_denoise_stream.h"
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static uint32_t g_rng = 2027u;
static uint32_t rnd_u() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
static float rnd() { return ((int32_t)(rnd_u() % 8001) - 4000) / 8000.0f; }
template <class T> static T* block(size_t n) { return (T*)malloc(n ? n * sizeof(T) : 1); }

// one row of n samples cut into pushes by `cut` (returns the next push's length given what is left), through plan / host_row / commit with exact-size blocks
template <class CUT> static void stream_row(const DnTables& t, const wn_denoise_stream_config& cfg, const float* prof, float strength, const float* x, int n, DnsRow* row,
                                            DnsHostRow* st, int restart_first, float* got, CUT cut) {
    char msg[128];
    int given = 0, emitted = 0, first = 1;
    for (;;) {
        int c = cut(n - given);
        if (c > n - given) c = n - given;
        const int32_t nn[1] = {c}, rs[1] = {first ? restart_first : 0}, fin[1] = {given + c == n};
        float* in = block<float>(c);
        memcpy(in, x + given, (size_t)c * 4);
        DnsStep s;
        int32_t n_out[1] = {-1};
        float dummy;
        CHECK(dns_plan_push("main", cfg, -1, true, row, in, c, nn, rs, fin, 1, strength, &dummy, 1 << 30, n_out, &s, msg, sizeof msg) == WN_OK);
        float* out = block<float>((size_t)(s.E1 - s.E0));
        dns_host_row(t, cfg, prof, strength, s, st, in, out);
        dns_commit_push(row, &s, rs, 1, n_out);
        CHECK(n_out[0] == s.E1 - s.E0 && emitted + n_out[0] <= n);
        CHECK(s.E1 == dns_ready(s.S1, cfg.n_fft, cfg.hop, fin[0]));
        if (!fin[0] && s.E1 > 0) CHECK(s.S1 - cfg.n_fft < s.E1 && s.E1 <= s.S1 - cfg.n_fft + cfg.hop);      // the lag bounds
        CHECK((int64_t)st->tail.size() == (fin[0] ? 0 : s.S1 - s.E1) && (int)st->tail.size() < cfg.n_fft);
        memcpy(got + emitted, out, (size_t)n_out[0] * 4);
        emitted += n_out[0]; given += c; first = 0;
        free(in); free(out);
        if (fin[0]) break;
    }
    CHECK(emitted == n && row->ended);
}

static void rows() {
    const int geos[][2] = {{64, 16}, {96, 20}, {32, 1}};
    for (const auto& geo : geos) {
        const int N = geo[0], hop = geo[1], H = N / 2;
        DnTables t;
        dn_build_tables(N, &t);
        float* prof = block<float>(H + 1);
        for (int k = 0; k <= H; ++k) prof[k] = 0.5f + 0.25f * rnd();
        const int ns[] = {0, 1, 15, 16, 17, H - 1, N, 32 * hop - 1, 32 * hop, 32 * hop + 1, 5 * N + 3};
        for (int n : ns) {
            float* x = block<float>(n); float* ref = block<float>(n); float* got = block<float>(n); float* other = block<float>(n);
            for (int s = 0; s < n; ++s) { x[s] = 0.4f * sinf(6.2831853f * s * 3.3f / N) + 0.05f * rnd(); other[s] = 0.3f * rnd(); }
            const int32_t len[1] = {n};
            wn_denoise_host_run(t, hop, prof, x, n, len, 1, 1.0f, ref, n);
            const int chunks[] = {1, hop - 1 > 0 ? hop - 1 : 1, hop, hop + 1, 32 * hop, 32 * hop + 1, n > 0 ? n : 1, -1};
            for (int c : chunks) {
                const int max_push = c > 0 ? c : 3 * hop + 7;
                const wn_denoise_stream_config cfg = {WN_ABI_VERSION, N, hop, 0, max_push, 0};
                DnsRow row;
                DnsHostRow st;
                // a first utterance that is cut off by the restart of the second: nothing of it may show
                {
                    char msg[64];
                    const int m = n < 2 * hop + 3 ? n : 2 * hop + 3, mm = m < max_push ? m : max_push;
                    const int32_t nn[1] = {mm}, rs[1] = {1}, fin[1] = {0};
                    DnsStep s; int32_t n_out[1]; float dummy;
                    float* in = block<float>(mm);
                    memcpy(in, other, (size_t)mm * 4);
                    CHECK(dns_plan_push("main", cfg, -1, true, &row, in, mm, nn, rs, fin, 1, 1.0f, &dummy, 1 << 30, n_out, &s, msg, sizeof msg) == WN_OK);
                    float* out = block<float>((size_t)(s.E1 - s.E0));
                    dns_host_row(t, cfg, prof, 1.0f, s, &st, in, out);
                    dns_commit_push(&row, &s, rs, 1, n_out);
                    free(in); free(out);
                }
                if (c > 0) stream_row(t, cfg, prof, 1.0f, x, n, &row, &st, 1, got, [&](int) { return c; });
                else stream_row(t, cfg, prof, 1.0f, x, n, &row, &st, 1, got, [&](int) { return (int)(rnd_u() % (uint32_t)(max_push + 1)); });      // ragged, zero-length pushes included
                CHECK(memcmp(got, ref, (size_t)n * 4) == 0);
                // the ended row refuses a push without restart, and takes one with it
                char msg[64];
                const int32_t one[1] = {1}, no[1] = {0}, yes[1] = {1};
                DnsStep s; int32_t n_out[1]; float dummy, v = 0.0f;
                CHECK(dns_plan_push("main", cfg, -1, true, &row, &v, 1, one, no, no, 1, 1.0f, &dummy, 8, n_out, &s, msg, sizeof msg) == WN_E_STATE);
                CHECK(dns_plan_push("main", cfg, -1, true, &row, &v, 1, one, yes, no, 1, 1.0f, &dummy, 8, n_out, &s, msg, sizeof msg) == WN_OK);
            }
            free(x); free(ref); free(got); free(other);
        }
        free(prof);
    }
}

static void decode() {      // in_type 1 and 2: the streamed row equals the one-shot run of the decoded row
    const int N = 64, hop = 16, n = 300;
    DnTables t;
    dn_build_tables(N, &t);
    float* prof = block<float>(N / 2 + 1);
    for (int k = 0; k <= N / 2; ++k) prof[k] = 0.05f;
    for (int type = 1; type <= 2; ++type) {
        int32_t* bits = block<int32_t>(n); float* x = block<float>(n); float* ref = block<float>(n); float* got = block<float>(n);
        for (int s = 0; s < n; ++s) {
            if (type == 2) bits[s] = (int32_t)(rnd_u() % 256); else { const float v = rnd(); memcpy(&bits[s], &v, 4); }
            x[s] = wn_post_decode(type, bits[s]);
        }
        const int32_t len[1] = {n};
        wn_denoise_host_run(t, hop, prof, x, n, len, 1, 1.0f, ref, n);
        const wn_denoise_stream_config cfg = {WN_ABI_VERSION, N, hop, 0, 37, type};
        DnsRow row; DnsHostRow st;
        stream_row(t, cfg, prof, 1.0f, (const float*)bits, n, &row, &st, 0, got, [&](int) { return 37; });
        CHECK(memcmp(got, ref, (size_t)n * 4) == 0);
        free(bits); free(x); free(ref); free(got);
    }
    free(prof);
}

static void rule() {
    const int geos[][2] = {{64, 16}, {96, 20}, {1024, 256}};
    for (const auto& geo : geos) {
        const int N = geo[0], hop = geo[1], H = N / 2;
        for (int64_t S = 0; S <= 4 * N; ++S) {
            int64_t e = 0;      // brute force: sample i goes out once the last frame that covers it, floor((i + H) / hop), has its whole window
            while (e < S && ((e + H) / hop) * hop + H <= S) ++e;
            CHECK(dns_ready(S, N, hop, 0) == e && dns_ready(S, N, hop, 1) == S);
            CHECK(dns_frames_done(S, N, hop, 1) == (S > 0 ? 1 + S / hop : 0));
        }
    }
}

static void codes() {
    char msg[48];      // (shorter than the longest message: the text is cut, never overrun)
    const wn_denoise_stream_config ok = {WN_ABI_VERSION, 1024, 256, 4, 2200, 0};
    auto cfg = [&](const char* name, wn_denoise_stream_config c) { printf("code %s %d\n", name, dns_check_config(&c, msg, sizeof msg)); };
    printf("code cfg_null %d\n", dns_check_config(nullptr, msg, sizeof msg));
    printf("code cfg_ok %d\n", dns_check_config(&ok, nullptr, 0));
    wn_denoise_stream_config c = ok;
    c.abi_version = WN_ABI_VERSION + 1; cfg("cfg_abi", c); c = ok;
    c.max_rows = -1; cfg("cfg_rows_neg", c); c.max_rows = 0; cfg("cfg_rows_zero", c); c = ok;
    c.max_push = 0; cfg("cfg_push_zero", c); c = ok;
    c.in_type = 3; cfg("cfg_in_type", c); c.in_type = 2; cfg("cfg_in_type_2", c); c = ok;
    c.n_fft = 1023; c.hop = 8; cfg("cfg_fft_odd", c); c = ok;
    c.hop = 257; cfg("cfg_hop_over", c); c = ok;
    c.n_fft = 100; c.hop = 25; cfg("cfg_fft_not_32", c); c = ok;
    c.max_rows = 4096; c.max_push = 1 << 20; cfg("cfg_reserve", c); c = ok;
    DnsRow rows[3];
    rows[2].ended = true;
    DnsStep steps[3];
    float x[4], y[4];
    int32_t n_out[3];
    const int32_t n[5] = {2200, 0, 0, 0, 0}, neg[3] = {2200, -1, 0}, big[3] = {2201, 0, 0}, zero[3] = {0, 0, 0}, ended[3] = {0, 0, 5}, fin2[3] = {0, 0, 1}, rs2[3] = {0, 0, 1};
    auto push = [&](const char* name, bool prof, const void* in, int64_t ip, const int32_t* nn, const int32_t* rs, const int32_t* fin, int32_t B, float st, const float* out, int64_t op,
                    const int32_t* no) {
        printf("code %s %d\n", name, dns_plan_push("main", ok, ok.max_rows, prof, rows, in, ip, nn, rs, fin, B, st, out, op, no, steps, msg, sizeof msg));
    };
    push("push_ok", true, x, 2200, n, nullptr, nullptr, 3, 1.0f, y, 2200, n_out);
    push("push_n_null", true, x, 2200, nullptr, nullptr, nullptr, 3, 1.0f, y, 2200, n_out);
    push("push_out_null", true, x, 2200, n, nullptr, nullptr, 3, 1.0f, nullptr, 2200, n_out);
    push("push_n_out_null", true, x, 2200, n, nullptr, nullptr, 3, 1.0f, y, 2200, nullptr);
    push("push_in_null", true, nullptr, 2200, n, nullptr, nullptr, 3, 1.0f, y, 2200, n_out);
    push("push_in_null_all_zero", true, nullptr, 0, zero, nullptr, nullptr, 3, 1.0f, y, 0, n_out);
    push("push_b_zero", true, x, 2200, n, nullptr, nullptr, 0, 1.0f, y, 2200, n_out);
    push("push_in_pitch_negative", true, x, -1, n, nullptr, nullptr, 3, 1.0f, y, 2200, n_out);
    push("push_out_pitch_negative", true, x, 2200, n, nullptr, nullptr, 3, 1.0f, y, -1, n_out);
    push("push_n_negative", true, x, 2200, neg, nullptr, nullptr, 3, 1.0f, y, 2200, n_out);
    push("push_strength_nan", true, x, 2200, n, nullptr, nullptr, 3, NAN, y, 2200, n_out);
    push("push_no_profile", false, x, 2200, n, nullptr, nullptr, 3, 1.0f, y, 2200, n_out);
    push("push_b_over", true, x, 2200, n, nullptr, nullptr, 5, 1.0f, y, 2200, n_out);
    push("push_n_over_max_push", true, x, 2201, big, nullptr, nullptr, 3, 1.0f, y, 2201, n_out);
    push("push_in_pitch_short", true, x, 2199, n, nullptr, nullptr, 3, 1.0f, y, 2200, n_out);
    push("push_out_pitch_short", true, x, 2200, n, nullptr, nullptr, 3, 1.0f, y, 1279, n_out);      // 2200 given, not final: 7 frames, 7 x 256 - 512 = 1280 go out
    push("push_out_pitch_exact", true, x, 2200, n, nullptr, nullptr, 3, 1.0f, y, 1280, n_out);
    push("push_ended_row", true, x, 2200, ended, nullptr, nullptr, 3, 1.0f, y, 2200, n_out);
    push("push_ended_row_final", true, x, 2200, zero, nullptr, fin2, 3, 1.0f, y, 2200, n_out);
    push("push_ended_row_restarted", true, x, 2200, ended, rs2, nullptr, 3, 1.0f, y, 2200, n_out);
    push("push_ended_row_left_alone", true, x, 2200, n, nullptr, nullptr, 3, 1.0f, y, 2200, n_out);
    rows[0].S = 0x7fffffffLL - 100;
    push("push_row_too_long", true, x, 2200, n, nullptr, nullptr, 3, 1.0f, y, 4000, n_out);
}

int main() {
    rule();
    rows();
    decode();
    codes();
    printf("denoise stream ok\n");
    return 0;
}
