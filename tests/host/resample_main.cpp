// Stand-alone host check of the resampler's host functions (csrc/wn_resample.h: the plan, the emit rule, the coefficient table, the one-output loop, the
// state machine of a push and the validation every entry point runs before any device call), built with -fsanitize=address,undefined and run as an ordinary
// program by tests/test_resample_cpu.py.  Every buffer is a heap block of exactly the row's size, so a read or write one element past a row is the
// sanitizer's to report.  Prints one "code <name> <value>" line per validation case (the test compares them) and "resample ok".
#include "wn_resample.h"
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

static wn_resample_config config(int sr_in, int sr_out, int zeros) { return wn_resample_config{WN_ABI_VERSION, 0, 0, sr_in, sr_out, zeros, 14.769656459379492, 0.9475937167399596}; }

// a row of n samples whole, then cut into pushes of every listed size through the carried tail: the same bits
static void rows() {
    const int pairs[][3] = {{3, 2, 4}, {2, 3, 4}, {2, 1, 4}, {1, 2, 4}, {7, 5, 3}, {320, 147, 4}, {147, 320, 4}, {5, 5, 4}, {48000, 22050, 64}};
    for (const auto& pr : pairs) {
        wn_resample_config cfg = config(pr[0], pr[1], pr[2]);
        RsPlan p;
        char msg[128];
        CHECK(rs_check_config(&cfg, &p, msg, sizeof msg) == WN_OK);
        std::vector<float> C;
        rs_build_table(cfg, p, &C);
        CHECK((int64_t)C.size() == p.L * p.T);
        const int64_t W = p.W, sizes[] = {0, 1, W, 2 * W + 1, 3 * W + 7};
        for (int64_t n : sizes) {
            const int64_t n_out = rs_num_out(n, p.L, p.M);
            CHECK(n_out == rs_ready(n, p.L, p.M, p.W, 1));
            float* x = (float*)malloc(n ? n * 4 : 1);
            float* y = (float*)malloc(n_out ? n_out * 4 : 1);
            for (int64_t t = 0; t < n; ++t) x[t] = ((int32_t)(rnd() % 20001) - 10000) / 10101.0f;
            rs_host_row(p, C.data(), x, n, y);
            for (int64_t cut : {(int64_t)1, W - 1, W, W + 1, (int64_t)0, 2 * W + 3}) {
                RsRow row; RsStep st; std::vector<float> tail;
                float* y2 = (float*)malloc(n_out ? n_out * 4 : 1);
                int64_t pos = 0, got = 0;
                bool first = true, done = false;
                while (!done) {
                    int32_t c = (int32_t)(cut > 0 ? (cut < n - pos ? cut : n - pos) : (first ? 0 : n - pos));
                    int32_t fin = (pos + c == n && !(cut == 0 && first)) ? 1 : 0, rs1 = first ? 1 : 0, n_o = -1;
                    float* in = (float*)malloc(c ? c * 4 : 1);
                    memcpy(in, x + pos, (size_t)c * 4);
                    const int64_t e = rs_ready(row.S * (first ? 0 : 1) + c, p.L, p.M, p.W, fin) - rs_ready(first ? 0 : row.S, p.L, p.M, p.W, 0);
                    float* o = (float*)malloc(e ? e * 4 : 1);
                    CHECK(rs_plan_push("main", cfg, p, -1, &row, in, c, &c, &rs1, &fin, 1, o, e, &n_o, &st, msg, sizeof msg) == WN_OK);
                    rs_host_push_row(p, C.data(), st, &tail, in, o);
                    rs_commit_push(&row, &st, &rs1, 1, &n_o);
                    CHECK(n_o == e && (int64_t)tail.size() <= (p.W ? 2 * p.W - 1 : 0));      // at most 2 W - 1 carried
                    memcpy(y2 + got, o, (size_t)e * 4);
                    got += e; pos += c; first = false; done = fin != 0;
                    free(in); free(o);
                }
                CHECK(got == n_out && memcmp(y, y2, (size_t)n_out * 4) == 0 && row.ended);
                free(y2);
            }
            free(x); free(y);
        }
    }
    // the emit rule against a brute-force statement: output m is ready once its last tap k0 + W is below S
    for (const auto& pr : pairs) {
        wn_resample_config cfg = config(pr[0], pr[1], pr[2]);
        RsPlan p;
        CHECK(rs_check_config(&cfg, &p, nullptr, 0) == WN_OK);
        if (p.T == 0) continue;
        for (int64_t S = 0; S <= 3 * p.W + 5; ++S) {
            int64_t e = 0;
            while (e * p.M / p.L + p.W <= S - 1) ++e;
            CHECK(rs_ready(S, p.L, p.M, p.W, 0) == e);
        }
    }
}

static void codes() {
    char msg[48];      // (shorter than the longest message: the text is cut, never overrun)
    wn_resample_config ok = config(48000, 22050, 64);
    RsPlan p;
    auto cfg = [&](const char* name, wn_resample_config c) { printf("code %s %d\n", name, rs_check_config(&c, &p, msg, sizeof msg)); };
    printf("code cfg_null %d\n", rs_check_config(nullptr, &p, msg, sizeof msg));
    printf("code cfg_ok %d\n", rs_check_config(&ok, nullptr, nullptr, 0));
    wn_resample_config c = ok;
    c.abi_version = WN_ABI_VERSION + 1; cfg("cfg_abi", c); c = ok;
    c.max_rows = -1; cfg("cfg_rows", c); c = ok;
    c.max_in = -1; cfg("cfg_max_in_neg", c); c.max_rows = 2; c.max_in = 0; cfg("cfg_max_in_zero", c); c = ok;
    c.sr_in = 0; cfg("cfg_sr_in", c); c = ok;
    c.sr_out = 0; cfg("cfg_sr_out", c); c = ok;
    c.zeros = 0; cfg("cfg_zeros", c); c = ok;
    c.rolloff = 0.0; cfg("cfg_rolloff_zero", c); c.rolloff = 1.5; cfg("cfg_rolloff_hi", c); c.rolloff = NAN; cfg("cfg_rolloff_nan", c); c.rolloff = 1.0; cfg("cfg_rolloff_one", c); c = ok;
    c.beta = -1.0; cfg("cfg_beta_neg", c); c.beta = INFINITY; cfg("cfg_beta_inf", c); c.beta = NAN; cfg("cfg_beta_nan", c); c.beta = 0.0; cfg("cfg_beta_zero", c);
    c.beta = 300.0; cfg("cfg_beta_big", c); c = ok;
    c.sr_in = 44101; c.sr_out = 44100; cfg("cfg_table", c); c = ok;
    c.sr_in = 1000000; c.sr_out = 1; c.zeros = 1; cfg("cfg_span", c); c = ok;
    c.sr_in = c.sr_out = 16000; cfg("cfg_identity", c); c = ok;
    CHECK(rs_check_config(&ok, &p, msg, sizeof msg) == WN_OK && p.L == 147 && p.M == 320 && p.W == 140 && p.T == 280);
    ok.max_in = 8;
    float in[8] = {0}, out[8];
    int32_t n[3] = {5, 0, 8}, neg[3] = {5, -1, 8}, big[3] = {5, 9, 8};
    auto run = [&](const char* name, const float* i, int64_t ip, const int32_t* nn, int32_t B, const float* o, int64_t op) {
        printf("code %s %d\n", name, rs_check_run("main", ok, p, 4, i, ip, nn, B, o, op, msg, sizeof msg));
    };
    run("run_ok", in, 8, n, 3, out, 4);
    run("run_in_null", nullptr, 8, n, 3, out, 4);
    run("run_n_null", in, 8, nullptr, 3, out, 4);
    run("run_out_null", in, 8, n, 3, nullptr, 4);
    run("run_b_zero", in, 8, n, 0, out, 4);
    run("run_n_negative", in, 8, neg, 3, out, 4);
    run("run_pitch_negative", in, -1, n, 3, out, 4);
    run("run_b_over", in, 8, n, 5, out, 4);
    run("run_max_in", in, 9, big, 3, out, 5);
    run("run_in_pitch", in, 7, n, 3, out, 4);
    run("run_out_pitch", in, 8, n, 3, out, 3);
    RsRow rows[3]; RsStep steps[3];
    int32_t n_out[3] = {-9, -9, -9}, fin[3] = {0, 0, 1}, none[3] = {0, 0, 0}, rst[3] = {0, 0, 1};
    auto push = [&](const char* name, const float* i, int64_t ip, const int32_t* nn, const int32_t* rs, const int32_t* f, int32_t B, const float* o, int64_t op, const int32_t* no) {
        printf("code %s %d\n", name, rs_plan_push("main", ok, p, 4, rows, i, ip, nn, rs, f, B, o, op, no, steps, msg, sizeof msg));
    };
    push("push_ok", in, 8, n, nullptr, fin, 3, out, 4, n_out);
    push("push_in_null", nullptr, 8, n, nullptr, fin, 3, out, 4, n_out);
    push("push_n_null", in, 8, nullptr, nullptr, fin, 3, out, 4, n_out);
    push("push_out_null", in, 8, n, nullptr, fin, 3, nullptr, 4, n_out);
    push("push_n_out_null", in, 8, n, nullptr, fin, 3, out, 4, nullptr);
    push("push_b_zero", in, 8, n, nullptr, fin, 0, out, 4, n_out);
    push("push_n_negative", in, 8, neg, nullptr, fin, 3, out, 4, n_out);
    push("push_b_over", in, 8, n, nullptr, fin, 5, out, 4, n_out);
    push("push_max_in", in, 9, big, nullptr, fin, 3, out, 5, n_out);
    push("push_in_pitch", in, 7, n, nullptr, fin, 3, out, 4, n_out);
    push("push_out_pitch", in, 8, n, nullptr, fin, 3, out, 3, n_out);      // row 2 is final: ceil(8 x 147 / 320) = 4 outputs
    CHECK(n_out[0] == -9);                                                    // planning writes no n_out
    CHECK(rs_plan_push("main", ok, p, 4, rows, in, 8, n, nullptr, fin, 3, out, 4, n_out, steps, msg, sizeof msg) == WN_OK);
    rs_commit_push(rows, steps, nullptr, 3, n_out);
    CHECK(n_out[0] == 0 && n_out[1] == 0 && n_out[2] == 4 && rows[2].ended && rows[0].S == 5 && rows[1].S == 0);
    push("push_ended", in, 8, n, nullptr, none, 3, out, 4, n_out);
    push("push_ended_restarted", in, 8, n, rst, none, 3, out, 4, n_out);
    rows[0].S = 0x7ffffffdLL;
    push("push_row_too_long", in, 8, n, rst, none, 3, out, 4, n_out);
}

int main() {
    rows();
    codes();
    printf("resample ok\n");
    return 0;
}
