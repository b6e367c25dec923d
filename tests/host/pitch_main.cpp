// Stand-alone host check of the pitch check's host functions (csrc/wn_pitch.h: the difference function, its normalisation, the pick, the comparison of two
// tracks, and the validation wn_pitch_create / wn_pitch_run / wn_pitch_compare do before any device call), built with -fsanitize=address,undefined and
// run as an ordinary program by tests/test_pitch_cpu.py.  Every buffer is a heap block of exactly the needed size -- the row of n samples above all -- so
// a read one sample before or past a row, or a write past a row's frames, is the sanitizer's to report.  Prints one "code <name> <value>" line per
// validation case (the test compares them) and "pitch ok".
#include "wn_pitch.h"
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static uint32_t g_rng = 2025u;
static float rnd() { g_rng = g_rng * 1664525u + 1013904223u; return ((int32_t)((g_rng >> 8) % 8001) - 4000) / 8000.0f; }
template <class T> static T* block(size_t n) { return (T*)malloc(n ? n * sizeof(T) : 1); }

static void rows() {
    const wn_pitch_config geos[] = {{WN_ABI_VERSION, 2000, 16, 64, 5, 40, 0.15f, 1, 1 << 20}, {WN_ABI_VERSION, 22050, 275, 1024, 44, 368, 0.15f, 1, 1 << 20},
                                    {WN_ABI_VERSION, 6400, 32, 128, 8, 128, 0.15f, 1, 1 << 20}};
    for (const wn_pitch_config& cfg : geos) {
        const int L = cfg.window + cfg.tau_max, TP = cfg.tau_max + 1;
        const int ns[] = {0, 1, cfg.hop - 1, cfg.hop, L - 1, L, 3 * L + 1};
        float* x = block<float>(L); float* dp = block<float>(TP);
        for (int n : ns)
            for (int kind = 0; kind < 3; ++kind) {      // a tone, noise, silence
                const int F = 1 + n / cfg.hop;
                float* wav = block<float>(n);
                for (int s = 0; s < n; ++s) wav[s] = kind == 0 ? 0.4f * sinf(6.2831853f * s * 2.5f / cfg.tau_max) : kind == 1 ? rnd() : 0.0f;
                float* f0 = block<float>(F); float* ap = block<float>(F); float* dpr = block<float>((size_t)F * TP);
                float* f0b = block<float>(F);
                const int32_t len[1] = {n};
                wn_pitch_host_rows(&cfg, wav, n, len, 1, F, f0, ap, dpr, x, dp);
                wn_pitch_host_rows(&cfg, wav, n, len, 1, F, f0b, nullptr, nullptr, x, dp);      // the optional outputs left out: the same track
                CHECK(memcmp(f0, f0b, (size_t)F * 4) == 0);
                for (int f = 0; f < F; ++f) {
                    CHECK(dpr[(size_t)f * TP] == 1.0f && ap[f] >= 0.0f);
                    if (kind == 2) CHECK(f0[f] == 0.0f && ap[f] == 1.0f);
                }
                float* table = block<float>(PITCH_COLS);
                const int32_t fr[1] = {F};
                wn_pitch_compare_host_rows(f0, f0b, F, fr, 1, table);
                CHECK(table[0] == (float)F && table[1] == table[2] && table[2] == table[3]);
                for (int j = 4; j < PITCH_COLS; ++j) CHECK(table[j] == 0.0f);
                free(wav); free(f0); free(ap); free(dpr); free(f0b); free(table);
            }
        free(x); free(dp);
    }
    // the comparison on tracks with every kind of frame, in blocks of exactly the row's size; an empty row gives zeros
    float a[6] = {100.0f, 0.0f, 200.0f, 0.0f, 100.0f, 150.0f}, b[6] = {100.0f, 120.0f, 0.0f, 0.0f, 200.0f, 150.0f};
    float* pa = block<float>(6); float* pb = block<float>(6); float* t = block<float>(2 * PITCH_COLS);
    memcpy(pa, a, sizeof a); memcpy(pb, b, sizeof b);
    const int32_t fr[2] = {3, 0};
    wn_pitch_compare_host_rows(pa, pb, 3, fr, 2, t);
    CHECK(t[0] == 3.0f && t[1] == 2.0f && t[2] == 2.0f && t[3] == 1.0f && fabsf(t[4] - 2.0f / 3.0f) < 1e-6f && t[5] == 0.0f && t[6] == 0.0f);
    for (int j = 0; j < PITCH_COLS; ++j) CHECK(t[PITCH_COLS + j] == 0.0f);
    const int32_t one[1] = {6};
    wn_pitch_compare_host_rows(pa, pb, 6, one, 1, t);
    CHECK(t[0] == 6.0f && t[3] == 3.0f && t[5] == 1.0f / 3.0f && fabsf(t[6] - 1200.0f / sqrtf(3.0f)) < 1e-3f && fabsf(t[7] - 400.0f) < 1e-3f && t[8] == 0.0f);
    free(pa); free(pb); free(t);
}

static void codes() {
    char msg[48];      // (shorter than the longest message: the text is cut, never overrun)
    const wn_pitch_config ok = {WN_ABI_VERSION, 22050, 275, 1024, 44, 368, 0.15f, 4, 4000};
    auto cfg = [&](const char* name, wn_pitch_config c) { printf("code %s %d\n", name, wn_pitch_check_config(&c, msg, sizeof msg)); };
    printf("code cfg_null %d\n", wn_pitch_check_config(nullptr, msg, sizeof msg));
    printf("code cfg_ok %d\n", wn_pitch_check_config(&ok, nullptr, 0));
    wn_pitch_config c = ok;
    c.abi_version = WN_ABI_VERSION + 1; cfg("cfg_abi", c); c = ok;
    c.sample_rate = 0; cfg("cfg_rate_zero", c); c = ok;
    c.hop = 0; cfg("cfg_hop_zero", c); c = ok;
    c.window = 0; cfg("cfg_window_zero", c); c = ok;
    c.tau_min = 1; cfg("cfg_tau_min_one", c); c.tau_min = 2; cfg("cfg_tau_min_two", c); c = ok;
    c.tau_max = 45; cfg("cfg_tau_max_tight", c); c.tau_max = 46; cfg("cfg_tau_max_least", c); c = ok;
    c.threshold = 0.0f; cfg("cfg_threshold_zero", c); c.threshold = 1.0f; cfg("cfg_threshold_one", c); c.threshold = 1.5f; cfg("cfg_threshold_over", c);
    c.threshold = NAN; cfg("cfg_threshold_nan", c); c = ok;
    c.max_batch = 0; cfg("cfg_batch_zero", c); c = ok;
    c.max_samples = -1; cfg("cfg_samples_neg", c); c.max_samples = 0; cfg("cfg_samples_zero", c); c = ok;
    c.window = 16384; cfg("cfg_lds_window", c); c = ok;
    c.hop = 2048; cfg("cfg_lds_hop", c); c = ok;
    c.tau_max = 1600; cfg("cfg_lds_tau", c);
    float x[4];
    int32_t n[3] = {3000, 0, 4000}, neg[3] = {3000, -1, 4000}, lng[3] = {3000, 0, 4001}, five[5] = {1, 1, 1, 1, 1};
    auto run = [&](const char* name, const float* wav, int64_t ld, const int32_t* len, int32_t B, int32_t F, const float* f0) {
        printf("code %s %d\n", name, wn_pitch_check_run("pitch_main", &ok, wav, ld, len, B, F, f0, msg, sizeof msg));
    };
    run("run_ok", x, 4000, n, 3, 15, x);
    run("run_wav_null", nullptr, 4000, n, 3, 15, x);
    run("run_lengths_null", x, 4000, nullptr, 3, 15, x);
    run("run_f0_null", x, 4000, n, 3, 15, nullptr);
    run("run_b_zero", x, 4000, n, 0, 15, x);
    run("run_f_negative", x, 4000, n, 3, -1, x);
    run("run_length_negative", x, 4000, neg, 3, 15, x);
    run("run_b_over", x, 4000, five, 5, 15, x);
    run("run_f_over", x, 4000, n, 3, 16, x);
    run("run_f_short", x, 4000, n, 3, 14, x);
    run("run_ld_short", x, 3999, n, 3, 15, x);
    run("run_length_over", x, 4100, lng, 3, 15, x);
    int32_t fr[3] = {15, 0, 7}, frneg[3] = {15, -1, 7}, frlng[3] = {16, 0, 7};
    auto cmp = [&](const char* name, const float* a, const float* b, int64_t pitch, const int32_t* f, int32_t B, const float* t) {
        printf("code %s %d\n", name, wn_pitch_check_compare("pitch_main", 4, 15, a, b, pitch, f, B, t, msg, sizeof msg));
    };
    cmp("cmp_ok", x, x, 15, fr, 3, x);
    cmp("cmp_a_null", nullptr, x, 15, fr, 3, x);
    cmp("cmp_b_null", x, nullptr, 15, fr, 3, x);
    cmp("cmp_frames_null", x, x, 15, nullptr, 3, x);
    cmp("cmp_table_null", x, x, 15, fr, 3, nullptr);
    cmp("cmp_b_zero", x, x, 15, fr, 0, x);
    cmp("cmp_frames_negative", x, x, 15, frneg, 3, x);
    cmp("cmp_b_over", x, x, 15, five, 5, x);
    cmp("cmp_pitch_short", x, x, 14, fr, 3, x);
    cmp("cmp_frames_over", x, x, 16, frlng, 3, x);
}

int main() {
    rows();
    codes();
    printf("pitch ok\n");
    return 0;
}
