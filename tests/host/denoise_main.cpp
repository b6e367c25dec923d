// Stand-alone host check of the spectral denoiser's host functions (csrc/wn_denoise.h: the tables, the analysis, the shrink, fit and run on host arrays, and
// the validation wn_denoise_create / fit / set_profile / run do before any device call), built with -fsanitize=address,undefined and run as an ordinary
// program by tests/test_denoise_cpu.py.  Every buffer is a heap block of exactly the needed size -- the row of n samples above all -- so a read one sample
// before or past a row, or a write past a row's length, is the sanitizer's to report.  Prints one "code <name> <value>" line per validation case (the test
// compares them) and "denoise ok".
#include "wn_denoise.h"
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static uint32_t g_rng = 2026u;
static float rnd() { g_rng = g_rng * 1664525u + 1013904223u; return ((int32_t)((g_rng >> 8) % 8001) - 4000) / 8000.0f; }
template <class T> static T* block(size_t n) { return (T*)malloc(n ? n * sizeof(T) : 1); }

static void rows() {
    const int geos[][2] = {{64, 16}, {96, 20}, {32, 1}};
    for (const auto& geo : geos) {
        const int N = geo[0], hop = geo[1], H = N / 2;
        DnTables t;
        dn_build_tables(N, &t);
        float* prof = block<float>(H + 1);
        {   // a profile from noise of 3 N + 1 samples; a row below N samples gives no frame
            const int n = 3 * N + 1;
            float* w = block<float>(n);
            for (int s = 0; s < n; ++s) w[s] = 0.1f * rnd();
            const int32_t len[1] = {n}, shrt[1] = {N - 1};
            CHECK(wn_denoise_host_fit(t, hop, w, n, shrt, 1, prof) == 0);
            CHECK(wn_denoise_host_fit(t, hop, w, n, len, 1, prof) == wn_denoise_fit_frames(n, N, hop));
            for (int k = 0; k <= H; ++k) CHECK(prof[k] >= 0.0f && prof[k] < 10.0f);
            free(w);
        }
        const int ns[] = {0, 1, 15, 16, 17, H - 1, N, 32 * hop - 1, 32 * hop, 32 * hop + 1};
        for (int n : ns)
            for (int kind = 0; kind < 3; ++kind) {      // a tone with noise, noise, silence
                float* in = block<float>(n); float* out = block<float>(n); float* id = block<float>(n);
                for (int s = 0; s < n; ++s) in[s] = kind == 0 ? 0.4f * sinf(6.2831853f * s * 3.3f / N) + 0.05f * rnd() : kind == 1 ? 0.1f * rnd() : 0.0f;
                const int32_t len[1] = {n};
                wn_denoise_host_run(t, hop, prof, in, n, len, 1, 1.0f, out, n);
                wn_denoise_host_run(t, hop, prof, in, n, len, 1, 0.0f, id, n);
                double e_in = 0.0, e_out = 0.0;
                for (int s = 0; s < n; ++s) {
                    CHECK(fabsf(id[s] - in[s]) <= 4e-6f);                       // strength 0 reproduces the input
                    if (kind == 2) CHECK(out[s] == 0.0f);
                    e_in += (double)in[s] * in[s]; e_out += (double)out[s] * out[s];
                }
                CHECK(e_out <= e_in * (1.0 + 1e-5) + 1e-12);
                memcpy(id, in, (size_t)n * 4);
                wn_denoise_host_run(t, hop, prof, id, n, len, 1, 1.0f, id, n);      // in place: the same bits
                CHECK(memcmp(id, out, (size_t)n * 4) == 0);
                wn_denoise_host_run(t, hop, prof, in, n, len, 1, 1e9f, out, n);       // beyond every |X|: exact zeros
                for (int s = 0; s < n; ++s) CHECK(out[s] == 0.0f);
                free(in); free(out); free(id);
            }
        free(prof);
    }
}

static void codes() {
    char msg[48];      // (shorter than the longest message: the text is cut, never overrun)
    const wn_denoise_config ok = {WN_ABI_VERSION, 1024, 256, 4, 6000};
    auto cfg = [&](const char* name, wn_denoise_config c) { printf("code %s %d\n", name, wn_denoise_check_config(&c, msg, sizeof msg)); };
    printf("code cfg_null %d\n", wn_denoise_check_config(nullptr, msg, sizeof msg));
    printf("code cfg_ok %d\n", wn_denoise_check_config(&ok, nullptr, 0));
    wn_denoise_config c = ok;
    c.abi_version = WN_ABI_VERSION + 1; cfg("cfg_abi", c); c = ok;
    c.max_batch = -1; cfg("cfg_batch_neg", c); c.max_batch = 0; cfg("cfg_batch_zero", c); c = ok;
    c.max_samples = -1; cfg("cfg_samples_neg", c); c = ok;
    c.n_fft = 1023; c.hop = 8; cfg("cfg_fft_odd", c); c.n_fft = 6; c.hop = 1; cfg("cfg_fft_small", c); c = ok;
    c.hop = 0; cfg("cfg_hop_zero", c); c.hop = 257; cfg("cfg_hop_over", c); c.hop = 256; cfg("cfg_hop_quarter", c); c = ok;
    c.n_fft = 100; c.hop = 25; cfg("cfg_fft_not_32", c); c.n_fft = 8192; c.hop = 2048; cfg("cfg_fft_large", c);
    c.n_fft = 2048; c.hop = 512; cfg("cfg_2048_512", c); c.n_fft = 4096; c.hop = 1024; cfg("cfg_4096_1024", c);
    float x[4];
    int32_t n[3] = {3000, 0, 6000}, neg[3] = {3000, -1, 6000}, lng[3] = {3000, 0, 6001}, five[5] = {1, 1, 1, 1, 1};
    auto args = [&](const char* name, const float* wav, int64_t pitch, const int32_t* len, int32_t B) {
        int rc = wn_denoise_check_args("denoise_main", wav, pitch, len, B, msg, sizeof msg);
        if (!rc) rc = wn_denoise_check_shape("denoise_main", ok.max_batch, ok.max_samples, pitch, len, B, msg, sizeof msg);
        printf("code %s %d\n", name, rc);
    };
    args("run_ok", x, 6000, n, 3);
    args("run_wav_null", nullptr, 6000, n, 3);
    args("run_lengths_null", x, 6000, nullptr, 3);
    args("run_b_zero", x, 6000, n, 0);
    args("run_pitch_negative", x, -1, n, 3);
    args("run_length_negative", x, 6000, neg, 3);
    args("run_b_over", x, 6000, five, 5);
    args("run_pitch_short", x, 5999, n, 3);
    args("run_length_over", x, 7000, lng, 3);
    auto str = [&](const char* name, float s) { printf("code %s %d\n", name, wn_denoise_check_strength("denoise_main", s, msg, sizeof msg)); };
    str("strength_zero", 0.0f); str("strength_neg", -0.5f); str("strength_nan", NAN); str("strength_inf", INFINITY);
    float p[3] = {0.0f, 1.0f, 2.0f};
    auto prof = [&](const char* name, const float* q) { printf("code %s %d\n", name, wn_denoise_check_profile("denoise_main", q, 3, msg, sizeof msg)); };
    prof("profile_ok", p); prof("profile_null", nullptr);
    p[1] = -1.0f; prof("profile_neg", p); p[1] = NAN; prof("profile_nan", p); p[1] = INFINITY; prof("profile_inf", p);
}

int main() {
    rows();
    codes();
    printf("denoise ok\n");
    return 0;
}
