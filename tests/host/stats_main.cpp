// Stand-alone host check of the training-summary statistics' host functions (csrc/wn_stats.h: the bucket table and the search in it, the element steps,
// the cut into segments, the joins, and the validation wn_stats_create / wn_stats_histogram / wn_stats_set_tensors do before any device call), built with
// -fsanitize=address,undefined and run as an ordinary program by tests/test_train_stats_cpu.py.  Every buffer is a heap block of exactly the needed size,
// so a read one element past a row's length, into the pitch gap's end or past a tensor is the sanitizer's to report.  Prints one "code <name> <value>"
// line per validation case (the test compares them) and "stats ok".
#include "wn_stats.h"
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static uint32_t g_rng = 2025u;
static float rnd() { g_rng = g_rng * 1664525u + 1013904223u; return ((int32_t)((g_rng >> 8) % 8001) - 4000) / 1000.0f; }
template <class T> static T* block(size_t n) { return (T*)malloc(n ? n * sizeof(T) : 1); }

static void table(double* lim) {
    CHECK(wn_stats_build_limits(lim) == WN_HIST_BUCKETS);
    for (int i = 1; i < WN_HIST_BUCKETS; ++i) CHECK(lim[i - 1] < lim[i]);
    CHECK(lim[0] == -DBL_MAX && lim[WN_HIST_BUCKETS - 1] == DBL_MAX && lim[STATS_POS + 1] == 0.0 && lim[STATS_POS + 2] == 1e-12);
    CHECK(stats_bucket(lim, 0.0f) == 776 && stats_bucket(lim, -0.0f) == 776 && stats_bucket(lim, 1e-12f) == 776 && stats_bucket(lim, -FLT_MAX) == 1);
    CHECK(stats_bucket(lim, FLT_MAX) == WN_HIST_BUCKETS - 1 && stats_bucket(lim, -1.4e-45f) == 775 && stats_bucket(lim, 1.4e-45f) == 776);
    for (int i = 0; i < WN_HIST_BUCKETS; ++i) {          // the float32 values around every limit inside the float range against a linear search
        if (fabs(lim[i]) > 1e20) continue;
        const float f = (float)lim[i], around[3] = {nextafterf(f, -INFINITY), f, nextafterf(f, INFINITY)};
        for (float v : around) {
            int want = 0;
            while (!(lim[want] > (double)v)) ++want;
            CHECK(stats_bucket(lim, v) == want);
        }
    }
}

static void histograms(const double* lim) {
    const int shapes[][3] = {{1, 1, 1}, {1, 63, 63}, {1, 64, 80}, {2, 65, 65}, {3, 257, 300}, {2, 4099, 4099}, {8, 1031, 1040}, {1, 4096, 4096}, {1, 4097, 4097}, {1, 270000, 270000}};
    for (const auto& sh : shapes) {
        const int B = sh[0], T = sh[1], pitch = sh[2];
        int32_t* len = block<int32_t>(B);
        int64_t total = 0;
        for (int b = 0; b < B; ++b) { len[b] = b == 0 ? T : (b == B / 2 ? 0 : T - 1 - 37 * b); if (len[b] < 0) len[b] = 0; total += len[b]; }
        // the ragged rows in ONE block that ends with the last row's last element: row b at b * pitch, nothing behind the last length
        const size_t n = (size_t)(B - 1) * pitch + len[B - 1];
        float* x = block<float>(n);
        float* dense = block<float>((size_t)B * T);
        for (size_t i = 0; i < n; ++i) x[i] = NAN;
        for (size_t i = 0; i < (size_t)B * T; ++i) dense[i] = INFINITY;
        int64_t nan = 0;
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < len[b]; ++t) {
                float v = rnd();
                if ((b * 131 + t) % 997 == 5) { v = NAN; ++nan; }
                x[(size_t)b * pitch + t] = v; dense[(size_t)b * T + t] = v;
            }
        int64_t* bk = block<int64_t>(WN_HIST_BUCKETS); int64_t* bk2 = block<int64_t>(WN_HIST_BUCKETS);
        double sm[8], sm2[8];
        wn_stats_host_hist(lim, x, pitch, len, B, T, bk, sm);
        wn_stats_host_hist(lim, dense, T, len, B, T, bk2, sm2);          // another pitch, other poison: the same bits
        CHECK(memcmp(bk, bk2, WN_HIST_BUCKETS * sizeof(int64_t)) == 0 && memcmp(sm, sm2, sizeof sm) == 0);
        int64_t sum = 0;
        for (int i = 0; i < WN_HIST_BUCKETS; ++i) sum += bk[i];
        CHECK(sum == total - nan && sm[0] == (double)sum && sm[5] == (double)nan && sm[6] == 0.0 && sm[7] == 0.0);
        if (sum) CHECK(sm[1] >= -4.0 && sm[2] <= 4.0 && sm[1] <= sm[2] && sm[4] >= 0.0); else CHECK(sm[1] == 0.0 && sm[2] == 0.0 && sm[3] == 0.0);
        free(len); free(x); free(dense); free(bk); free(bk2);
    }
    // lengths NULL: every row T long; lengths outside [0, T] are held inside it
    float* x = block<float>(2 * 5);
    for (int i = 0; i < 10; ++i) x[i] = (float)i;
    int64_t* bk = block<int64_t>(WN_HIST_BUCKETS);
    double sm[8];
    wn_stats_host_hist(lim, x, 5, nullptr, 2, 5, bk, sm);
    CHECK(sm[0] == 10.0 && sm[1] == 0.0 && sm[2] == 9.0 && sm[3] == 45.0 && sm[4] == 285.0);
    const int32_t wild[2] = {-3, 9};
    wn_stats_host_hist(lim, x, 5, wild, 2, 5, bk, sm);
    CHECK(sm[0] == 5.0 && sm[1] == 5.0 && sm[2] == 9.0);
    const float bad[4] = {NAN, INFINITY, -INFINITY, -INFINITY};
    wn_stats_host_hist(lim, bad, 4, nullptr, 1, 4, bk, sm);
    CHECK(sm[0] == 0.0 && sm[1] == 0.0 && sm[2] == 0.0 && sm[3] == 0.0 && sm[4] == 0.0 && sm[5] == 1.0 && sm[6] == 1.0 && sm[7] == 2.0);
    for (int i = 0; i < WN_HIST_BUCKETS; ++i) CHECK(bk[i] == 0);
    free(x); free(bk);
}

static void tensors() {
    const int64_t counts[] = {1, 7, 8, 64, 4095, 4096, 4097, 8200, 24576, 270000};
    for (int64_t n : counts) {
        float* x = block<float>((size_t)n);          // exactly the tensor: offset 0
        double want = 0.0, mx = 0.0;
        for (int64_t i = 0; i < n; ++i) { x[i] = rnd(); want += (double)x[i] * x[i]; if (fabs((double)x[i]) > mx) mx = fabs((double)x[i]); }
        const int64_t off[1] = {0}, cnt[1] = {n};
        double out[4];
        wn_stats_host_tensors(x, off, cnt, 1, out);
        CHECK(fabs(out[0] - want) <= 1e-12 * want && out[1] == mx && out[2] == 0.0 && out[3] == (double)n);
        if (n >= 7) {
            x[n / 2] = NAN; x[0] = -INFINITY;
            wn_stats_host_tensors(x, off, cnt, 1, out);
            CHECK(out[2] == 2.0 && out[0] <= want && out[1] <= mx);
        }
        free(x);
    }
    CHECK(stats_nseg(0) == 0 && stats_nseg(1) == 1 && stats_nseg(4096) == 1 && stats_nseg(4097) == 2 && stats_nseg(1 << 30) == STATS_MAX_SEG);
    for (int64_t n : counts) CHECK(stats_seglen(n) * stats_nseg(n) >= n && stats_seglen(n) * (stats_nseg(n) - 1) < n);
}

static void codes() {
    char msg[40];      // (shorter than the longest message: the text is cut, never overrun)
    const wn_stats_config ok = {WN_ABI_VERSION, 4, 8, 3};
    auto cfg = [&](const char* name, wn_stats_config c) { printf("code %s %d\n", name, wn_stats_check_config(&c, msg, sizeof msg)); };
    printf("code cfg_null %d\n", wn_stats_check_config(nullptr, msg, sizeof msg));
    printf("code cfg_ok %d\n", wn_stats_check_config(&ok, nullptr, 0));
    wn_stats_config c = ok;
    c.abi_version = WN_ABI_VERSION + 1; cfg("cfg_abi", c); c = ok;
    c.max_rows = -1; cfg("cfg_rows_neg", c); c.max_rows = 65536; cfg("cfg_rows_over", c); c.max_rows = 0; cfg("cfg_rows_zero", c); c = ok;
    c.max_time = -1; cfg("cfg_time_neg", c); c.max_time = 0; cfg("cfg_time_zero", c); c.max_rows = 0; cfg("cfg_time_zero_validation_only", c); c = ok;
    c.max_tensors = -1; cfg("cfg_tensors_neg", c); c.max_tensors = 65536; cfg("cfg_tensors_over", c); c.max_tensors = 0; cfg("cfg_tensors_zero", c);
    float x[4]; int64_t bk[1]; double sm[1];
    auto hist = [&](const char* name, const float* xx, int64_t pitch, int32_t B, int32_t T, const int64_t* b, const double* s) {
        printf("code %s %d\n", name, wn_stats_check_hist("stats_main", 4, 8, xx, pitch, B, T, b, s, msg, sizeof msg));
    };
    hist("hist_ok", x, 8, 4, 8, bk, sm);
    hist("hist_x_null", nullptr, 8, 4, 8, bk, sm);
    hist("hist_bucket_null", x, 8, 4, 8, nullptr, sm);
    hist("hist_summary_null", x, 8, 4, 8, bk, nullptr);
    hist("hist_b_zero", x, 8, 0, 8, bk, sm);
    hist("hist_t_zero", x, 8, 4, 0, bk, sm);
    hist("hist_b_over", x, 8, 5, 8, bk, sm);
    hist("hist_t_over", x, 9, 4, 9, bk, sm);
    hist("hist_pitch", x, 7, 4, 8, bk, sm);
    int32_t order[4];
    const int64_t off[3] = {10, 0, 4}, cnt[3] = {5, 4, 6}, cnt0[3] = {5, 0, 6}, offn[3] = {10, -1, 4}, lap[3] = {5, 5, 6}, off4[4] = {0, 4, 10, 15}, cnt4[4] = {4, 6, 5, 1};
    auto tab = [&](const char* name, const int64_t* o, const int64_t* n, int32_t nt) {
        printf("code %s %d\n", name, wn_stats_check_tensors("stats_main", 3, o, n, nt, order, msg, sizeof msg));
    };
    tab("tensors_ok_unsorted", off, cnt, 3);
    tab("tensors_off_null", nullptr, cnt, 3);
    tab("tensors_cnt_null", off, nullptr, 3);
    tab("tensors_nt_zero", off, cnt, 0);
    tab("tensors_count_zero", off, cnt0, 3);
    tab("tensors_offset_neg", offn, cnt, 3);
    tab("tensors_overlap", off, lap, 3);
    tab("tensors_nt_over", off4, cnt4, 4);
}

int main() {
    double* lim = block<double>(WN_HIST_BUCKETS);
    table(lim);
    histograms(lim);
    tensors();
    codes();
    free(lim);
    printf("stats ok\n");
    return 0;
}
