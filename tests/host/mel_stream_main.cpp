// Stand-alone host check of the streaming mel analysis' host functions (csrc/wn_mel_stream.h: the geometry, the rule of readiness, and the validation and
// planning every push runs before any device call), built with -fsanitize=address,undefined and run as an ordinary program by tests/test_mel_stream_cpu.py.
// Every array is a heap block of exactly B entries, so a read or write one entry past a row is the sanitizer's to report.  Prints one "code <name> <value>"
// line per validation case (the test compares them) and "mel stream ok".
#include "wn_mel_stream.h"
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static uint32_t g_rng = 2468u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

static const int GEOMS[][3] = {{2048, 1100, 275}, {1024, 1024, 256}, {800, 800, 200}, {256, 256, 16}, {64, 7, 3}, {2, 1, 1}, {16, 4, 9}};      // n_fft, win_size, hop

// the rule against a brute-force statement, and its two orders
static void rule() {
    for (const auto& gm : GEOMS) {
        const MelsGeom g = mels_geom(gm[0], gm[1], gm[2]);
        CHECK(g.Hl + g.Hr == g.win && g.Hl >= 0 && g.Hr >= 0);
        for (int64_t S = 0; S <= 3 * (int64_t)g.win + 5 * g.hop; ++S) {
            int64_t f = 0;
            while (f * g.hop + g.Hr <= S) ++f;
            CHECK(mels_ready(g, S, 0) == f);
            CHECK(mels_ready(g, S, 1) == 1 + S / g.hop && mels_ready(g, S, 0) <= mels_ready(g, S, 1));
        }
    }
}

// rows cut into pushes: summed n_out = 1 + S / hop, frames contiguous, the tail below win_size and exactly what the next frame reaches back to
static void rows() {
    for (const auto& gm : GEOMS) {
        const MelsGeom g = mels_geom(gm[0], gm[1], gm[2]);
        const int32_t max_push = 3 * g.win + 2 * g.hop;
        const int64_t cuts[] = {1, g.hop - 1, g.hop, g.hop + 1, g.Hr - 1, g.Hr, g.win, max_push, 0};
        for (int trial = 0; trial < 40; ++trial) {
            const int B = 1 + (int)(rnd() % 5);
            MelsRow* rows = new MelsRow[B];
            MelsStep* steps = new MelsStep[B];
            int32_t* n = (int32_t*)malloc(B * 4); int32_t* rs = (int32_t*)malloc(B * 4); int32_t* fin = (int32_t*)malloc(B * 4); int32_t* n_out = (int32_t*)malloc(B * 4);
            float* gain = (float*)malloc(B * 4);
            int64_t* left = (int64_t*)malloc(B * 8); int64_t* total = (int64_t*)malloc(B * 8); int64_t* frames = (int64_t*)malloc(B * 8);
            bool* started = (bool*)malloc(B); bool* done = (bool*)malloc(B);
            for (int b = 0; b < B; ++b) { left[b] = total[b] = rnd() % (6 * (uint32_t)g.win + 3); frames[b] = 0; started[b] = done[b] = false; }
            const float in = 0.0f, out = 0.0f;
            char msg[200];
            for (int guard = 0; guard < 10000; ++guard) {
                bool all = true;
                for (int b = 0; b < B; ++b) all = all && done[b];
                if (all) break;
                for (int b = 0; b < B; ++b) {
                    n[b] = rs[b] = fin[b] = 0; gain[b] = 0.5f + b;
                    if (done[b]) continue;
                    int64_t c = cuts[rnd() % 9];
                    if (c < 0) c = 0;
                    if (c > left[b]) c = left[b];
                    n[b] = (int32_t)c; rs[b] = !started[b]; started[b] = true; left[b] -= c;
                    if (left[b] == 0 && rnd() % 3 != 0) { fin[b] = 1; done[b] = true; }      // (else: a later push of n = 0 is the final one)
                }
                CHECK(mels_plan_push("main", g, B, max_push, rows, &in, max_push, n, rs, fin, gain, B, &out, max_push / g.hop + 4, n_out, steps, msg, sizeof msg) == WN_OK);
                for (int b = 0; b < B; ++b) {
                    CHECK(steps[b].F0 == frames[b] || rs[b]);
                    CHECK(steps[b].T0 <= steps[b].S0 && steps[b].T1 <= steps[b].S1 && steps[b].T0 <= steps[b].T1);
                    // every sample a new frame reads lies in the tail or in the new samples
                    if (steps[b].F1 > steps[b].F0) CHECK(mels_tail_lo(g, steps[b].F0) >= steps[b].T0 || steps[b].T0 == steps[b].S0);
                }
                mels_commit_push(rows, steps, rs, B, n_out);
                for (int b = 0; b < B; ++b) {
                    frames[b] += n_out[b];
                    CHECK(rows[b].F == frames[b] && rows[b].S == total[b] - left[b]);
                    CHECK(rows[b].S - mels_tail_at(g, rows[b].F, rows[b].S) < g.win);
                    if (rs[b]) CHECK(rows[b].gain == 0.5f + b);
                    if (!rows[b].ended) CHECK(rows[b].F == mels_ready(g, rows[b].S, 0) || rows[b].S == 0);
                }
            }
            for (int b = 0; b < B; ++b) CHECK(done[b] && rows[b].ended && frames[b] == 1 + total[b] / g.hop);
            delete[] rows; delete[] steps;
            free(n); free(rs); free(fin); free(n_out); free(gain); free(left); free(total); free(frames); free(started); free(done);
        }
    }
}

static void codes() {
    char msg[48];      // (shorter than the longest message: the text is cut, never overrun)
    printf("code sizes_ok %d\n", mels_check_sizes(0, 1, msg, sizeof msg));
    printf("code sizes_rows %d\n", mels_check_sizes(-1, 1, msg, sizeof msg));
    printf("code sizes_push %d\n", mels_check_sizes(2, 0, msg, sizeof msg));
    const MelsGeom g = mels_geom(2048, 1100, 275);
    float in[8] = {0}, out[8];
    int32_t n[3] = {5, 0, 8}, neg[3] = {5, -1, 8}, big[3] = {5, 9, 8};
    MelsRow rows[3]; MelsStep steps[3];
    int32_t n_out[3] = {-9, -9, -9}, fin[3] = {0, 0, 1}, none[3] = {0, 0, 0}, rst[3] = {0, 0, 1};
    float gains[3] = {1.0f, 2.0f, 3.0f}, bad_gain[3] = {1.0f, 2.0f, INFINITY};
    auto push = [&](const char* name, const float* i, int64_t ip, const int32_t* nn, const int32_t* rs, const int32_t* f, const float* gn, int32_t B, const float* o, int64_t op,
                    const int32_t* no) {
        printf("code %s %d\n", name, mels_plan_push("main", g, 4, 8, rows, i, ip, nn, rs, f, gn, B, o, op, no, steps, msg, sizeof msg));
    };
    push("push_ok", in, 8, n, nullptr, fin, nullptr, 3, out, 1, n_out);
    push("push_in_null", nullptr, 8, n, nullptr, fin, nullptr, 3, out, 1, n_out);
    push("push_n_null", in, 8, nullptr, nullptr, fin, nullptr, 3, out, 1, n_out);
    push("push_out_null", in, 8, n, nullptr, fin, nullptr, 3, nullptr, 1, n_out);
    push("push_n_out_null", in, 8, n, nullptr, fin, nullptr, 3, out, 1, nullptr);
    push("push_b_zero", in, 8, n, nullptr, fin, nullptr, 0, out, 1, n_out);
    push("push_n_negative", in, 8, neg, nullptr, fin, nullptr, 3, out, 1, n_out);
    push("push_pitch_negative", in, -1, n, nullptr, fin, nullptr, 3, out, 1, n_out);
    push("push_b_over", in, 8, n, nullptr, fin, nullptr, 5, out, 1, n_out);
    push("push_max_push", in, 9, big, nullptr, fin, nullptr, 3, out, 1, n_out);
    push("push_in_pitch", in, 7, n, nullptr, fin, nullptr, 3, out, 1, n_out);
    push("push_out_pitch", in, 8, n, nullptr, fin, nullptr, 3, out, 0, n_out);      // row 2 is final: 1 + 8 / 275 = 1 frame
    push("push_gain_not_finite", in, 8, n, rst, fin, bad_gain, 3, out, 1, n_out);
    CHECK(n_out[0] == -9);                                                          // planning writes no n_out
    CHECK(mels_plan_push("main", g, 4, 8, rows, in, 8, n, rst, fin, gains, 3, out, 1, n_out, steps, msg, sizeof msg) == WN_OK);
    mels_commit_push(rows, steps, rst, 3, n_out);
    CHECK(n_out[0] == 0 && n_out[1] == 0 && n_out[2] == 1 && rows[2].ended && rows[0].S == 5 && rows[1].S == 0 && rows[2].gain == 3.0f && rows[0].gain == 1.0f);
    push("push_ended", in, 8, n, nullptr, none, nullptr, 3, out, 1, n_out);
    push("push_ended_restarted", in, 8, n, rst, none, nullptr, 3, out, 1, n_out);
    rows[0].S = 0x7ffffffdLL;
    push("push_row_too_long", in, 8, n, rst, none, nullptr, 3, out, 1, n_out);
    CHECK(rows[0].S == 0x7ffffffdLL && rows[2].ended);                              // a refused push changes no row
}

int main() {
    rule();
    rows();
    codes();
    printf("mel stream ok\n");
    return 0;
}
