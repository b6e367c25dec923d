// Stand-alone host check of the reconstruction check's host functions (csrc/wn_melcmp.h: the per-frame distances, the reductions over frames, the DCT
// table, and the validation wn_melcmp_create / wn_melcmp_run do before any device call), built with -fsanitize=address,undefined and run as an ordinary
// program by tests/test_melcmp_cpu.py.  Every buffer is a heap block of exactly the needed size, so a read or write one element past a row, a frame or
// the table is the sanitizer's to report.  Prints one "code <name> <value>" line per validation case (the test compares them) and "melcmp ok".
#include "wn_melcmp.h"
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static uint32_t g_rng = 2024u;
static float rnd() { g_rng = g_rng * 1664525u + 1013904223u; return ((int32_t)((g_rng >> 8) % 8001) - 4000) / 1000.0f; }
template <class T> static T* block(size_t n) { return (T*)malloc(n ? n * sizeof(T) : 1); }

static void rows() {
    const int Ms[] = {1, 13, 80, 128}, Fs[] = {0, 1, 63, 64, 65, 129};
    for (int M : Ms) {
        const int ceps[] = {0, 1, 13, M - 1};
        for (int n_cep : ceps) {
            if (n_cep > M - 1) continue;
            wn_melcmp_config cfg = {WN_ABI_VERSION, M, n_cep, 12.5f, 3.0f, 0, 0};
            float* dct = block<float>((size_t)n_cep * M);
            float* col = block<float>(M);
            wn_melcmp_dct_table(M, n_cep, dct);
            for (int k = 0; k < n_cep; ++k) {      // orthonormal rows
                double s = 0.0;
                for (int m = 0; m < M; ++m) s += (double)dct[k * M + m] * dct[k * M + m];
                CHECK(fabs(s - 1.0) < 1e-5);
            }
            for (int F : Fs)
                for (int layouts = 0; layouts < 4; ++layouts) {
                    // one row, pitch = its frames exactly, in either layout of either input; a second pair in the other layouts must give the same bits
                    const int a_cf = layouts & 1, b_cf = layouts >> 1;
                    const size_t n = (size_t)F * M;
                    float* a = block<float>(n); float* b = block<float>(n); float* a2 = block<float>(n); float* b2 = block<float>(n);
                    for (int f = 0; f < F; ++f)
                        for (int m = 0; m < M; ++m) {
                            const float va = rnd(), vb = rnd();
                            a[a_cf ? (size_t)m * F + f : (size_t)f * M + m] = va; a2[a_cf ? (size_t)f * M + m : (size_t)m * F + f] = va;
                            b[b_cf ? (size_t)m * F + f : (size_t)f * M + m] = vb; b2[b_cf ? (size_t)f * M + m : (size_t)m * F + f] = vb;
                        }
                    float* pf = block<float>(6 * (size_t)F); float* pf2 = block<float>(6 * (size_t)F);
                    float* sm = block<float>(7); float* sm2 = block<float>(7);
                    int32_t* mk = block<int32_t>(2); int32_t* mk2 = block<int32_t>(2);
                    const int32_t frames[1] = {F};
                    wn_melcmp_host_rows(&cfg, dct, a, a_cf, F, b, b_cf, F, frames, 1, pf, F, sm, mk, col);
                    wn_melcmp_host_rows(&cfg, dct, a2, !a_cf, F, b2, !b_cf, F, frames, 1, pf2, F, sm2, mk2, col);
                    CHECK(memcmp(pf, pf2, 6 * (size_t)F * 4) == 0 && memcmp(sm, sm2, 28) == 0 && memcmp(mk, mk2, 8) == 0);
                    if (F == 0) { for (int j = 0; j < 7; ++j) CHECK(sm[j] == 0.0f); CHECK(mk[0] == -1 && mk[1] == 0); }
                    else {
                        int32_t at = -1, count = 0; float w = 0.0f;
                        for (int f = 0; f < F; ++f) { const float x = pf[4 * F + f]; if (at < 0 || x > w) { w = x; at = f; } count += x > cfg.alarm_db; }
                        CHECK(mk[0] == at && mk[1] == count && sm[6] == w);
                        if (n_cep == 0) for (int f = 0; f < F; ++f) CHECK(pf[3 * F + f] == 0.0f);
                    }
                    // identical inputs: exactly zero
                    wn_melcmp_host_rows(&cfg, dct, a, a_cf, F, a, a_cf, F, frames, 1, pf, F, sm, mk, col);
                    for (size_t i = 0; i < 6 * (size_t)F; ++i) CHECK(pf[i] == 0.0f);
                    for (int j = 0; j < 7; ++j) CHECK(sm[j] == 0.0f);
                    CHECK(mk[0] == (F ? 0 : -1) && mk[1] == 0);
                    free(a); free(b); free(a2); free(b2); free(pf); free(pf2); free(sm); free(sm2); free(mk); free(mk2);
                }
            free(dct); free(col);
        }
    }
}

static void codes() {
    char msg[48];      // (shorter than the longest message: the text is cut, never overrun)
    const wn_melcmp_config ok = {WN_ABI_VERSION, 80, 13, 12.5f, 3.0f, 4, 8};
    auto cfg = [&](const char* name, wn_melcmp_config c) { printf("code %s %d\n", name, wn_melcmp_check_config(&c, msg, sizeof msg)); };
    printf("code cfg_null %d\n", wn_melcmp_check_config(nullptr, msg, sizeof msg));
    printf("code cfg_ok %d\n", wn_melcmp_check_config(&ok, nullptr, 0));
    wn_melcmp_config c = ok;
    c.abi_version = WN_ABI_VERSION + 1; cfg("cfg_abi", c); c = ok;
    c.num_mels = 0; cfg("cfg_mels_zero", c); c.num_mels = 129; cfg("cfg_mels_over", c); c.num_mels = 128; cfg("cfg_mels_top", c); c = ok;
    c.n_cep = -1; cfg("cfg_cep_neg", c); c.n_cep = 80; cfg("cfg_cep_over", c); c.n_cep = 79; cfg("cfg_cep_top", c); c.n_cep = 0; cfg("cfg_cep_zero", c); c = ok;
    c.unit_db = 0.0f; cfg("cfg_unit_zero", c); c.unit_db = -1.0f; cfg("cfg_unit_neg", c); c.unit_db = INFINITY; cfg("cfg_unit_inf", c); c.unit_db = NAN; cfg("cfg_unit_nan", c); c = ok;
    c.alarm_db = -0.5f; cfg("cfg_alarm_neg", c); c.alarm_db = INFINITY; cfg("cfg_alarm_inf", c); c.alarm_db = NAN; cfg("cfg_alarm_nan", c); c.alarm_db = 0.0f; cfg("cfg_alarm_zero", c); c = ok;
    c.max_batch = -1; cfg("cfg_batch_neg", c); c.max_batch = 0; cfg("cfg_batch_zero", c); c = ok;
    c.max_frames = -1; cfg("cfg_frames_neg", c); c.max_frames = 0; cfg("cfg_frames_zero", c);
    float x[4], s[4]; int32_t m[4];
    int32_t n[3] = {5, 0, 8}, neg[3] = {5, -1, 8}, lng[3] = {5, 0, 9}, five[5] = {5, 0, 8, 1, 1};
    auto call = [&](const char* name, const float* a, int64_t ap, const float* b, int64_t bp, const int32_t* fr, int32_t B, const float* pf, int64_t op, const float* sm, const int32_t* mk) {
        printf("code %s %d\n", name, wn_melcmp_check_call("melcmp_main", 4, 8, a, ap, b, bp, fr, B, pf, op, sm, mk, msg, sizeof msg));
    };
    call("run_ok", x, 8, x, 8, n, 3, x, 8, s, m);
    call("run_ok_no_per_frame", x, 8, x, 8, n, 3, nullptr, 0, s, m);
    call("run_a_null", nullptr, 8, x, 8, n, 3, x, 8, s, m);
    call("run_b_null", x, 8, nullptr, 8, n, 3, x, 8, s, m);
    call("run_frames_null", x, 8, x, 8, nullptr, 3, x, 8, s, m);
    call("run_summary_null", x, 8, x, 8, n, 3, x, 8, nullptr, m);
    call("run_marks_null", x, 8, x, 8, n, 3, x, 8, s, nullptr);
    call("run_b_zero", x, 8, x, 8, n, 0, x, 8, s, m);
    call("run_frames_negative", x, 8, x, 8, neg, 3, x, 8, s, m);
    call("run_b_over", x, 8, x, 8, five, 5, x, 8, s, m);
    call("run_frames_over", x, 9, x, 9, lng, 3, x, 9, s, m);
    call("run_a_pitch", x, 7, x, 8, n, 3, x, 8, s, m);
    call("run_b_pitch", x, 8, x, 7, n, 3, x, 8, s, m);
    call("run_out_pitch", x, 8, x, 8, n, 3, x, 7, s, m);
    call("run_out_pitch_unused", x, 8, x, 8, n, 3, nullptr, 7, s, m);
}

int main() {
    rows();
    codes();
    printf("melcmp ok\n");
    return 0;
}
