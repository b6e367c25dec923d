// Stand-alone host check of the Griffin-Lim host functions (csrc/wn_griffin.h: the tables, the analysis, the projection, the synthesis and the gather on
// host arrays, the mel -> magnitude map, and the validation wn_griffin_create / wn_griffin_run do before any device call), built with
// -fsanitize=address,undefined and run as an ordinary program by tests/test_griffin_cpu.py.  Every buffer is a heap block of exactly the needed size -- the
// row of hop (F - 1) samples above all -- so a read one sample before or past a row, or a write past a row's length, is the sanitizer's to report.  Prints
// one "code <name> <value>" line per validation case (the test compares them), "wss <n_fft> <win> <hop> <min>" per geometry and "griffin ok".
#include "wn_griffin.h"
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static uint32_t g_rng = 2026u;
static float rnd() { g_rng = g_rng * 1664525u + 1013904223u; return ((int32_t)((g_rng >> 8) % 8001) - 4000) / 8000.0f; }
template <class T> static T* block(size_t n) { return (T*)malloc(n ? n * sizeof(T) : 1); }

static void rows() {
    const int geos[][3] = {{64, 48, 12}, {96, 80, 20}, {64, 64, 16}, {32, 4, 1}, {32, 30, 7}};
    for (const auto& geo : geos) {
        GlTables t;
        gl_build_tables(geo[0], geo[1], geo[2], &t);
        const GlGeom& g = t.g;
        float wmin = 1e30f;
        const int Fs[] = {2, 3, 31, 32, 33, 65};
        for (int F : Fs) {
            const int64_t n = (int64_t)g.hop * (F - 1);
            for (int kind = 0; kind < 3; ++kind) {      // a tone with noise, noise, silence
                float* x = block<float>(n); float* y = block<float>(n); float* z = block<float>(n);
                float* S = block<float>((size_t)F * g.NB); float* u = block<float>((size_t)F * g.NB); float* pre = block<float>((size_t)F * g.NB * 2);
                float* spec = block<float>((size_t)2 * g.N);
                for (int64_t s = 0; s < n; ++s) x[s] = kind == 0 ? 0.4f * sinf(6.2831853f * s * 3.3f / g.N) + 0.05f * rnd() : kind == 1 ? 0.1f * rnd() : 0.0f;
                for (int f = 0; f < F; ++f) {      // S = |STFT(x)|: x is a fixed point of the iteration
                    gl_host_analyse(t, x, n, f, spec);
                    S[(size_t)f * g.NB] = fabsf(spec[0]); S[(size_t)f * g.NB + g.H] = fabsf(spec[1]);
                    for (int k = 1; k < g.H; ++k) S[(size_t)f * g.NB + k] = sqrtf(spec[2 * k] * spec[2 * k] + spec[2 * k + 1] * spec[2 * k + 1]);
                    for (int k = 0; k < g.NB; ++k) u[(size_t)f * g.NB + k] = 0.5f + 0.5f * rnd();
                }
                gl_host_row(t, S, nullptr, x, F, 1, y, pre);      // from x itself: the consistent spectrum comes back
                float mx = 0.0f;
                for (int64_t s = 0; s < n; ++s) mx = fmaxf(mx, fabsf(x[s]));
                for (int64_t s = 0; s < n; ++s) CHECK(fabsf(y[s] - x[s]) <= 2e-5f * fmaxf(mx, 1.0f));
                gl_host_row(t, S, u, nullptr, F, 2, y, nullptr);      // from uniforms
                gl_host_row(t, S, nullptr, nullptr, F, 2, z, nullptr);      // from zero phase
                for (int64_t s = 0; s < n; ++s) { CHECK(isfinite(y[s]) && isfinite(z[s])); if (kind == 2) CHECK(y[s] == 0.0f && z[s] == 0.0f); }
                free(x); free(y); free(z); free(S); free(u); free(pre); free(spec);
            }
            for (int64_t i = 0; i < n; ++i) {      // the window-square sum of every sample of the row
                const int64_t p = i + g.Hl;
                const int64_t f_lo = p >= g.W ? (p - g.W) / g.hop + 1 : 0, f_hi = p / g.hop < F - 1 ? p / g.hop : F - 1;
                float den = 0.0f;
                for (int64_t f = f_lo; f <= f_hi; ++f) den += t.wsq[p - f * g.hop];
                wmin = fminf(wmin, den);
            }
        }
        CHECK(wmin > 0.0f);
        printf("wss %d %d %d %.6f\n", geo[0], geo[1], geo[2], (double)wmin);
    }
}

static void mels() {
    const int N = 64, NB = 33, M = 7, F_max = 5;
    wn_griffin_config c = {WN_ABI_VERSION, N, 48, 12, M, 2.0f, 1.5f, -100.0f, 20.0f, 4.0f, 1, 1, 1, 0, 0};
    float* pT = block<float>((size_t)M * NB);
    for (int i = 0; i < M * NB; ++i) pT[i] = 0.1f * rnd();
    const int32_t frames[2] = {5, 2};
    for (int variant = 0; variant < 5; ++variant) {
        c.signal_normalization = variant < 4; c.allow_clipping = variant & 1; c.symmetric_mels = (variant >> 1) & 1;
        for (int kind = 0; kind < 2; ++kind) {
            float* mel = block<float>((size_t)2 * F_max * M); float* mag = block<float>((size_t)2 * F_max * NB);
            for (int i = 0; i < 2 * F_max * M; ++i) mel[i] = 5.0f * rnd();
            for (int i = 0; i < 2 * F_max * NB; ++i) mag[i] = -1.0f;
            gl_host_magnitudes(c, pT, mel, kind, F_max, frames, 2, mag);
            for (int b = 0; b < 2; ++b)
                for (int f = 0; f < F_max; ++f)
                    for (int k = 0; k < NB; ++k) {
                        const float v = mag[((size_t)b * F_max + f) * NB + k];
                        if (f < frames[b]) CHECK(v > 0.0f && isfinite(v)); else CHECK(v == -1.0f);
                    }
            free(mel); free(mag);
        }
    }
    free(pT);
}

static void codes() {
    char msg[48];      // (shorter than the longest message: the text is cut, never overrun)
    const wn_griffin_config ok = {WN_ABI_VERSION, 2048, 1100, 275, 80, 2.0f, 1.5f, -100.0f, 20.0f, 4.0f, 1, 1, 1, 4, 40};
    auto cfg = [&](const char* name, wn_griffin_config c) { printf("code %s %d\n", name, wn_griffin_check_config(&c, msg, sizeof msg)); };
    printf("code cfg_null %d\n", wn_griffin_check_config(nullptr, msg, sizeof msg));
    printf("code cfg_ok %d\n", wn_griffin_check_config(&ok, nullptr, 0));
    wn_griffin_config c = ok;
    c.abi_version = WN_ABI_VERSION + 1; cfg("cfg_abi", c); c = ok;
    c.max_batch = -1; cfg("cfg_batch_neg", c); c.max_batch = 0; c.max_frames = 0; cfg("cfg_geometry_only", c); c = ok;
    c.max_frames = -1; cfg("cfg_frames_neg", c); c.max_frames = 1; cfg("cfg_frames_one", c); c = ok;
    c.num_mels = -1; cfg("cfg_mels_neg", c); c.num_mels = 513; cfg("cfg_mels_over", c); c.num_mels = 0; cfg("cfg_mels_zero", c); c = ok;
    c.magnitude_power = 0.0f; cfg("cfg_mp_zero", c); c.magnitude_power = NAN; cfg("cfg_mp_nan", c); c = ok;
    c.power = -1.0f; cfg("cfg_power_neg", c); c.power = INFINITY; cfg("cfg_power_inf", c); c = ok;
    c.min_level_db = 0.0f; cfg("cfg_level_zero", c); c.signal_normalization = 0; cfg("cfg_level_zero_unnormalised", c); c = ok;
    c.n_fft = 2047; cfg("cfg_fft_odd", c); c.n_fft = 6; c.win_size = 4; c.hop = 1; cfg("cfg_fft_small", c); c = ok;
    c.win_size = 2049; cfg("cfg_win_over", c); c.win_size = 3; c.hop = 1; cfg("cfg_win_small", c); c = ok;
    c.hop = 0; cfg("cfg_hop_zero", c); c.hop = 276; cfg("cfg_hop_over", c); c.hop = 275; cfg("cfg_hop_quarter", c); c = ok;
    c.n_fft = 100; c.win_size = 100; c.hop = 25; cfg("cfg_fft_not_32", c); c.n_fft = 8192; c.win_size = 8192; c.hop = 2048; cfg("cfg_fft_large", c);
    c.n_fft = 4096; c.win_size = 4096; c.hop = 1024; cfg("cfg_4096_1024", c); c = ok;
    c.hop = 256; c.win_size = 1024; cfg("cfg_hop_256", c);
    float x[4];
    int32_t fr[3] = {40, 2, 33}, one[3] = {40, 1, 33}, lng[3] = {40, 2, 41}, five[5] = {2, 2, 2, 2, 2};
    const int64_t pitch = 275 * 39;
    auto run = [&](const char* name, int have_pinv, const float* src, int32_t kind, int32_t F_max, const int32_t* frames, int32_t B, const float* y0, int64_t y0_pitch,
                   int32_t iters, const float* out, int64_t out_pitch) {
        printf("code %s %d\n", name, wn_griffin_check_run("griffin_main", &ok, have_pinv, ok.max_batch, src, kind, F_max, frames, B, y0, y0_pitch, iters, out, out_pitch, msg, sizeof msg));
    };
    run("run_ok", 1, x, 0, 40, fr, 3, nullptr, 0, 60, x, pitch);
    run("run_src_null", 1, nullptr, 0, 40, fr, 3, nullptr, 0, 60, x, pitch);
    run("run_frames_null", 1, x, 0, 40, nullptr, 3, nullptr, 0, 60, x, pitch);
    run("run_kind_bad", 1, x, 3, 40, fr, 3, nullptr, 0, 60, x, pitch);
    run("run_mel_without_pinv", 0, x, 1, 40, fr, 3, nullptr, 0, 60, x, pitch);
    run("run_magnitude_without_pinv", 0, x, 2, 40, fr, 3, nullptr, 0, 60, x, pitch);
    run("run_b_zero", 1, x, 0, 40, fr, 0, nullptr, 0, 60, x, pitch);
    run("run_iters_negative", 1, x, 0, 40, fr, 3, nullptr, 0, -1, x, pitch);
    run("run_iters_zero", 1, x, 0, 40, fr, 3, nullptr, 0, 0, x, pitch);
    run("run_pitch_negative", 1, x, 0, 40, fr, 3, nullptr, 0, 60, x, -1);
    run("run_b_over", 1, x, 0, 40, five, 5, nullptr, 0, 60, x, pitch);
    run("run_one_frame", 1, x, 0, 40, one, 3, nullptr, 0, 60, x, pitch);
    run("run_frames_over_fmax", 1, x, 0, 39, fr, 3, nullptr, 0, 60, x, pitch);
    run("run_frames_over_max", 1, x, 0, 41, lng, 3, nullptr, 0, 60, x, 275 * 40);
    run("run_out_pitch_short", 1, x, 0, 40, fr, 3, nullptr, 0, 60, x, pitch - 1);
    run("run_y0_pitch_short", 1, x, 0, 40, fr, 3, x, pitch - 1, 60, x, pitch);
    run("run_out_null", 1, x, 0, 40, fr, 3, nullptr, 0, 60, nullptr, 0);
}

int main() {
    rows();
    mels();
    codes();
    printf("griffin ok\n");
    return 0;
}
