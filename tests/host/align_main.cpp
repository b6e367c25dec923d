// Stand-alone host check of the alignment check's host functions (csrc/wn_align.h: the cepstra, the cost of a frame pair, the band, the recurrence with
// its tie order, the back-trace, the summary and the maps, and the validation wn_align_create / wn_align_run do before any device call), built with
// -fsanitize=address,undefined and run as an ordinary program by tests/test_align_cpu.py.  Every buffer is a heap block of exactly the needed size -- a
// row's frames above all, in either layout -- so a read past a row's frames, a write past a path's cells or past a map's row is the sanitizer's to report.
// Prints one "code <name> <value>" line per validation case (the test compares them) and "align ok".
#include "wn_align.h"
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static uint32_t g_rng = 2026u;
static float rnd() { g_rng = g_rng * 1664525u + 1013904223u; return ((int32_t)((g_rng >> 8) % 8001) - 4000) / 1000.0f; }
template <class T> static T* block(size_t n) { return (T*)malloc(n ? n * sizeof(T) : 1); }

static void check_path(const int32_t* path, int64_t pitch, int n, int Fa, int Fb, int band, const int32_t* map_ab, const int32_t* map_ba) {
    CHECK(n >= 1 && n <= Fa + Fb - 1 && path[0] == 0 && path[pitch] == 0 && path[n - 1] == Fa - 1 && path[pitch + n - 1] == Fb - 1);
    for (int p = 0; p < n; ++p) {
        const int i = path[p], j = path[pitch + p];
        int32_t lo, hi;
        align_span(i, Fa, Fb, band, &lo, &hi);
        CHECK(align_in(j, lo, hi));
        if (p > 0) {
            const int di = i - path[p - 1], dj = j - path[pitch + p - 1];
            CHECK(di >= 0 && di <= 1 && dj >= 0 && dj <= 1 && di + dj >= 1);
        }
        CHECK(map_ab[i] >= j && map_ba[j] >= i);
    }
}

static void rows() {
    const int shapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {15, 16}, {16, 17}, {33, 5}, {5, 33}, {40, 40}};
    for (int M : {2, 16})
        for (int band : {0, 1, 3})
            for (int cf = 0; cf < 2; ++cf)
                for (const auto& s : shapes) {
                    const int Fa = s[0], Fb = s[1], K = M - 1 < 13 ? M - 1 : 13, np = Fa + Fb - 1;
                    const wn_align_config cfg = {WN_ABI_VERSION, M, K, 1.5f, band, 0, 0, 0};
                    float* a = block<float>((size_t)Fa * M); float* b = block<float>((size_t)Fb * M);      // pitches of exactly the rows' frames
                    for (int t = 0; t < Fa * M; ++t) a[t] = rnd();
                    for (int t = 0; t < Fb * M; ++t) b[t] = rnd();
                    int32_t* path = block<int32_t>((size_t)2 * np); int32_t* mab = block<int32_t>(Fa); int32_t* mba = block<int32_t>(Fb);
                    float* sm = block<float>(7); float* sm2 = block<float>(7);
                    float* dm = block<float>((size_t)Fa * Fb); float* cost = block<float>((size_t)Fa * Fb);
                    const int32_t fa[1] = {Fa}, fb[1] = {Fb};
                    wn_align_host_rows(&cfg, a, cf, Fa, b, !cf, Fb, fa, fb, 1, path, np, mab, Fa, mba, Fb, sm, nullptr, nullptr, cost, dm);
                    wn_align_host_rows(&cfg, a, cf, Fa, b, !cf, Fb, fa, fb, 1, nullptr, 0, nullptr, 0, nullptr, 0, sm2, nullptr, nullptr, nullptr, nullptr);      // the optional outputs left out
                    CHECK(memcmp(sm, sm2, 7 * sizeof(float)) == 0);
                    const int n = (int)sm[2];
                    CHECK(sm[0] == (float)Fa && sm[1] == (float)Fb && sm[3] == dm[(size_t)Fa * Fb - 1] && isfinite(sm[3]) && sm[4] >= 0.0f);
                    check_path(path, np, n, Fa, Fb, band, mab, mba);
                    // the recurrence alone on that cost matrix gives the same bits
                    float* dm2 = block<float>((size_t)Fa * Fb);
                    wn_align_host_dp_rows(band, cost, Fa, Fb, fa, fb, 1, path, np, mab, Fa, mba, Fb, sm2, dm2);
                    CHECK(memcmp(sm, sm2, 7 * sizeof(float)) == 0 && memcmp(dm, dm2, (size_t)Fa * Fb * sizeof(float)) == 0);
                    // non-finite frames: a valid path all the same
                    if (Fa > 2) for (int m = 0; m < M; ++m) a[cf ? (size_t)m * Fa + 1 : (size_t)M + m] = NAN;
                    if (Fb > 3) b[!cf ? (size_t)2 : (size_t)2 * M] = INFINITY;
                    wn_align_host_rows(&cfg, a, cf, Fa, b, !cf, Fb, fa, fb, 1, path, np, mab, Fa, mba, Fb, sm, nullptr, nullptr, nullptr, nullptr);
                    check_path(path, np, (int)sm[2], Fa, Fb, 0, mab, mba);      // (the band is not promised for such inputs: checked against the whole matrix)
                    free(a); free(b); free(path); free(mab); free(mba); free(sm); free(sm2); free(dm); free(cost); free(dm2);
                }
}

static void codes() {
    char msg[48];      // (shorter than the longest message: the text is cut, never overrun)
    const wn_align_config ok = {WN_ABI_VERSION, 80, 13, 1.0f, 0, 4, 500, 600};
    auto cfg = [&](const char* name, wn_align_config c) {
        int rc = wn_align_check_config(&c, msg, sizeof msg);
        if (rc == WN_OK) rc = wn_align_check_reserve(&c, msg, sizeof msg);
        printf("code %s %d\n", name, rc);
    };
    printf("code cfg_null %d\n", wn_align_check_config(nullptr, msg, sizeof msg));
    printf("code cfg_ok %d\n", wn_align_check_config(&ok, nullptr, 0));
    wn_align_config c = ok;
    c.abi_version = WN_ABI_VERSION + 1; cfg("cfg_abi", c); c = ok;
    c.num_mels = 0; cfg("cfg_mels_zero", c); c.num_mels = 129; cfg("cfg_mels_over", c); c = ok;
    c.n_cep = 0; cfg("cfg_cep_zero", c); c.n_cep = 80; cfg("cfg_cep_over", c); c.n_cep = 79; cfg("cfg_cep_most", c); c = ok;
    c.unit_db = 0.0f; cfg("cfg_unit_zero", c); c.unit_db = NAN; cfg("cfg_unit_nan", c); c.unit_db = INFINITY; cfg("cfg_unit_inf", c); c = ok;
    c.band = -1; cfg("cfg_band_neg", c); c.band = 7; cfg("cfg_band_seven", c); c = ok;
    c.max_batch = -1; cfg("cfg_batch_neg", c); c.max_batch = 0; c.max_frames_a = 0; c.max_frames_b = 0; cfg("cfg_validation_only", c); c = ok;
    c.max_frames_a = 0; cfg("cfg_frames_zero", c); c.max_frames_a = -1; cfg("cfg_frames_neg", c); c = ok;
    c.max_frames_a = 4096; c.max_frames_b = 4096; cfg("cfg_frames_most", c); c.max_frames_b = 4097; cfg("cfg_frames_over", c); c = ok;
    c.max_batch = 600; c.max_frames_a = 500; c.max_frames_b = 500; cfg("cfg_cells_over", c);
    float x[4]; int32_t o[4];
    int32_t fa[3] = {400, 1, 500}, fb[3] = {600, 1, 2}, zero[3] = {400, 0, 500}, lng[3] = {400, 1, 501}, lngb[3] = {601, 1, 2}, five[5] = {1, 1, 1, 1, 1};
    auto run = [&](const char* name, const float* a, int64_t ap, const float* b, int64_t bp, const int32_t* f, const int32_t* g, int32_t B, const int32_t* path, int64_t pp,
                   const int32_t* ma, int64_t pa, const int32_t* mb, int64_t pb, const float* sm) {
        printf("code %s %d\n", name, wn_align_check_call("align_main", 4, 500, 600, a, ap, b, bp, f, g, B, path, pp, ma, pa, mb, pb, sm, msg, sizeof msg));
    };
    run("run_ok", x, 500, x, 600, fa, fb, 3, o, 999, o, 500, o, 600, x);
    run("run_ok_no_outputs", x, 500, x, 600, fa, fb, 3, nullptr, 0, nullptr, 0, nullptr, 0, x);
    run("run_a_null", nullptr, 500, x, 600, fa, fb, 3, o, 999, o, 500, o, 600, x);
    run("run_b_null", x, 500, nullptr, 600, fa, fb, 3, o, 999, o, 500, o, 600, x);
    run("run_frames_a_null", x, 500, x, 600, nullptr, fb, 3, o, 999, o, 500, o, 600, x);
    run("run_frames_b_null", x, 500, x, 600, fa, nullptr, 3, o, 999, o, 500, o, 600, x);
    run("run_summary_null", x, 500, x, 600, fa, fb, 3, o, 999, o, 500, o, 600, nullptr);
    run("run_b_zero", x, 500, x, 600, fa, fb, 0, o, 999, o, 500, o, 600, x);
    run("run_frames_a_zero", x, 500, x, 600, zero, fb, 3, o, 999, o, 500, o, 600, x);
    run("run_frames_b_zero", x, 500, x, 600, fa, zero, 3, o, 999, o, 500, o, 600, x);
    run("run_b_over", x, 500, x, 600, five, five, 5, o, 999, o, 500, o, 600, x);
    run("run_frames_a_over", x, 501, x, 600, lng, fb, 3, o, 999, o, 501, o, 600, x);
    run("run_frames_b_over", x, 500, x, 601, fa, lngb, 3, o, 1000, o, 500, o, 601, x);
    run("run_path_short", x, 500, x, 600, fa, fb, 3, o, 998, o, 500, o, 600, x);
    run("run_map_a_short", x, 500, x, 600, fa, fb, 3, o, 999, o, 499, o, 600, x);
    run("run_map_b_short", x, 500, x, 600, fa, fb, 3, o, 999, o, 500, o, 599, x);
    run("run_a_pitch_short", x, 499, x, 600, fa, fb, 3, o, 999, o, 500, o, 600, x);
    run("run_b_pitch_short", x, 500, x, 599, fa, fb, 3, o, 999, o, 500, o, 600, x);
}

int main() {
    rows();
    codes();
    printf("align ok\n");
    return 0;
}
