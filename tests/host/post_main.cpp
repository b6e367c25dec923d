// Stand-alone host check of the output stage's host functions (csrc/wn_post.h: decode, chain step, PCM conversion, the row loop of the hook, and the
// validation wn_post_create / wn_post_push / wn_post_finish run before any device call), built with -fsanitize=address,undefined and run as an ordinary
// program by tests/test_post_cpu.py.  Every buffer is a heap block of exactly the row's size, so a read or write one element past a row is the
// sanitizer's to report.  Prints one "code <name> <value>" line per validation case (the test compares them) and "post ok".
#define WN_POST_HOST_TABLES
#include "wn_post.h"
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

static void fill(int type, int32_t* in, int64_t n) {
    for (int64_t t = 0; t < n; ++t) {
        if (type == 2) in[t] = (int32_t)(rnd() % 300) - 20;      // ids outside 0 ... 255 too: the decode clamps them
        else { const float v = ((int32_t)(rnd() % 20001) - 10000) / 10101.0f; memcpy(&in[t], &v, 4); }
    }
}

static void rows() {
    const int64_t sizes[] = {0, 1, 63, 64, 65, 1025, 4099};
    const float ks[] = {0.0f, 0.85f, 0.97f};
    for (int type = 0; type < 3; ++type)
        for (float k : ks)
            for (int64_t n : sizes) {
                int32_t* in = (int32_t*)malloc(n ? n * 4 : 1);
                float* y = (float*)malloc(n ? n * 4 : 1);
                int16_t* q = (int16_t*)malloc(n ? n * 2 : 1);
                fill(type, in, n);
                float carry = -1.0f, peak = -1.0f; int32_t clipped = -1;
                wn_post_host_row(type, k, in, n, 0.25f, 4.0f * 32767.0f, y, q, &carry, &peak, &clipped);
                CHECK(n > 0 ? carry == y[n - 1] : carry == 0.25f);
                int32_t over = 0; float pk = 0.0f;
                for (int64_t t = 0; t < n; ++t) {
                    CHECK(q[t] >= -32767 && q[t] <= 32767);
                    over += fabsf(y[t] * (4.0f * 32767.0f)) > 32767.0f;
                    pk = fabsf(y[t]) > pk ? fabsf(y[t]) : pk;
                }
                CHECK(over == clipped && pk == peak);
                // the same row in two calls through the carry: the same bits, whatever the cut
                for (int64_t cut : {(int64_t)0, n / 3, n}) {
                    float* y2 = (float*)malloc(n ? n * 4 : 1);
                    float c1 = 0.0f, c2 = 0.0f;
                    wn_post_host_row(type, k, in, cut, 0.25f, 1.0f, y2, nullptr, &c1, nullptr, nullptr);
                    wn_post_host_row(type, k, in + cut, n - cut, c1, 1.0f, y2 + cut, nullptr, &c2, nullptr, nullptr);
                    CHECK(memcmp(y, y2, n * 4) == 0 && memcmp(&c2, &carry, 4) == 0);
                    free(y2);
                }
                // outputs are optional one by one
                wn_post_host_row(type, k, in, n, 0.25f, 1.0f, nullptr, nullptr, nullptr, nullptr, nullptr);
                free(in); free(y); free(q);
            }
    // truncation toward zero, the clamp and the count
    int32_t c = 0;
    CHECK(wn_post_pcm(0.99999f, 1.0f, &c) == 0 && wn_post_pcm(-0.99999f, 1.0f, &c) == 0 && wn_post_pcm(1.5f, 1.0f, &c) == 1 && wn_post_pcm(-1.5f, 1.0f, &c) == -1 && c == 0);
    CHECK(wn_post_pcm(1.0f, 32767.0f, &c) == 32767 && c == 0 && wn_post_pcm(1.0f, 32768.0f, &c) == 32767 && c == 1 && wn_post_pcm(-2.0f, 32767.0f, &c) == -32767 && c == 2);
    CHECK(wn_post_peak_scale(0.0f) == (float)(32767.0 / 0.01) && wn_post_peak_scale(0.5f) == 65534.0f && wn_post_gain_scale(1.0f) == 32767.0f);
}

static void codes() {
    char msg[64];      // (shorter than the longest message: the text is cut, never overrun)
    wn_post_config ok = {WN_ABI_VERSION, 4, 2, 0.97f, 1.0f};
    auto cfg = [&](const char* name, wn_post_config c) { printf("code %s %d\n", name, wn_post_check_config(&c, msg, sizeof msg)); };
    printf("code cfg_null %d\n", wn_post_check_config(nullptr, msg, sizeof msg));
    printf("code cfg_ok %d\n", wn_post_check_config(&ok, nullptr, 0));
    wn_post_config c = ok;
    c.abi_version = WN_ABI_VERSION + 1; cfg("cfg_abi", c); c = ok;
    c.max_rows = 0; cfg("cfg_rows", c); c = ok;
    c.in_type = 3; cfg("cfg_type_hi", c); c.in_type = -1; cfg("cfg_type_lo", c); c = ok;
    c.deemphasis = 1.0f; cfg("cfg_k_one", c); c.deemphasis = -0.1f; cfg("cfg_k_neg", c); c.deemphasis = NAN; cfg("cfg_k_nan", c); c.deemphasis = 0.0f; cfg("cfg_k_zero", c); c = ok;
    c.gain = 0.0f; cfg("cfg_gain_zero", c); c.gain = -1.0f; cfg("cfg_gain_neg", c); c.gain = INFINITY; cfg("cfg_gain_inf", c); c.gain = NAN; cfg("cfg_gain_nan", c);
    int32_t in[8] = {0}; float f[8]; int16_t q[8];
    int32_t n[3] = {5, 0, 8}, neg[3] = {5, -1, 8};
    auto call = [&](const char* name, int finish, const void* i, int64_t ip, const int32_t* nn, int32_t B, const float* of, const int16_t* oq, int64_t op) {
        printf("code %s %d\n", name, wn_post_check_call("post_main", finish, 4, i, ip, nn, B, of, oq, op, msg, sizeof msg));
    };
    call("push_ok", 0, in, 8, n, 3, f, q, 8);
    call("push_ok_pcm_only", 0, in, 8, n, 3, nullptr, q, 8);
    call("push_ok_float_only", 0, in, 8, n, 3, f, nullptr, 8);
    call("push_in_null", 0, nullptr, 8, n, 3, f, q, 8);
    call("push_n_null", 0, in, 8, nullptr, 3, f, q, 8);
    call("push_no_output", 0, in, 8, n, 3, nullptr, nullptr, 8);
    call("push_b_zero", 0, in, 8, n, 0, f, q, 8);
    call("push_n_negative", 0, in, 8, neg, 3, f, q, 8);
    call("push_b_over", 0, in, 8, n, 5, f, q, 8);
    call("push_in_pitch", 0, in, 7, n, 3, f, q, 8);
    call("push_out_pitch", 0, in, 8, n, 3, f, q, 7);
    call("finish_ok", 1, in, 8, n, 3, f, nullptr, 8);
    call("finish_no_float", 1, in, 8, n, 3, nullptr, q, 8);
    call("finish_b_over", 1, in, 8, n, 5, f, q, 8);
    call("finish_out_pitch", 1, in, 8, n, 3, f, q, 7);
}

int main() {
    rows();
    codes();
    printf("post ok\n");
    return 0;
}
