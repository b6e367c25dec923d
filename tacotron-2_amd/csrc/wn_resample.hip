// Sample-rate conversion on the device (wn_resample_* of include/wavenet_mi355.h; the definition, the plan, the table and the host side: wn_resample.h).
//
// One kernel serves wn_resample_run and wn_resample_push: a run is a push of a row that starts at S = 0, is final and carries nothing.  A workgroup owns a
// block of up to 1024 consecutive outputs of one row (plan.block; smaller where M / L is large, so that the staged inputs fit 48 KiB).  It stages the inputs
// its outputs read -- [k0(first) - W + 1, k0(last) + W], below S0 from the row's carried tail, from S0 on from the push, 0.0f outside [0, S1) -- in LDS, then
// every lane runs RS_PER_THREAD outputs side by side (lane t: outputs t, t + 256, ...), each with its own accumulator over its own row p = (m M) mod L of the
// table in global memory: T fmaf in ascending j.  No sum is ever split, so the bits equal rs_host_output's.  Workgroup 0 of a row that is not final also
// writes the row's new tail into the OTHER half of its tail buffer: the workgroups of one row read the old half concurrently and need no order among them.
// The counters (S per row, ended, tail half) live on the host and travel as kernel arguments.  No atomics, no allocation, no synchronisation in a call.
#include "wn_resample.h"
#include "wn_common.h"

#define RS_GROUP 64      // rows per launch
#define RS_ACTIVE 1
#define RS_FINAL 2
#define RS_PAR 4

struct wn_resample {
    wn_resample_config cfg;
    RsPlan plan;
    std::string err;
    std::vector<RsRow> rows;      // the counters, max_rows of them (a geometry-only handle keeps RS_GROUP so that a push can be planned)
    std::vector<RsStep> steps;
    DevBuf<float> table, tail;    // [L][T]; [max_rows][2][tail_cap]
};

struct RsArgs {
    const float* in; const float* C; float* out; float* tail;
    int64_t in_pitch, out_pitch;
    int32_t b0, L, M, W, T, block, span, tail_cap;
    int32_t S0[RS_GROUP], n[RS_GROUP];
    uint8_t flags[RS_GROUP];
};

__global__ __launch_bounds__(RS_THREADS) void wn_resample_kernel(const RsArgs a) {
    extern __shared__ float span[];
    const int tid = threadIdx.x, b = blockIdx.y, flags = a.flags[b];
    if (!(flags & RS_ACTIVE)) return;
    const int final = (flags & RS_FINAL) ? 1 : 0;
    const int64_t L = a.L, M = a.M, W = a.W, T = a.T, row = a.b0 + b;
    const int64_t S0 = a.S0[b], S1 = S0 + a.n[b];
    const int64_t E0 = rs_ready(S0, L, M, W, 0), E1 = rs_ready(S1, L, M, W, final), lo0 = rs_tail_lo(E0, L, M, W);
    const float* told = a.tail ? a.tail + (row * 2 + ((flags & RS_PAR) ? 1 : 0)) * a.tail_cap : nullptr;      // the inputs [lo0, S0)
    const float* x = a.in + row * a.in_pitch;                                                                // the inputs [S0, S1)
    if (blockIdx.x == 0 && !final && a.tail) {      // the new tail [lo1, S1) into the other half: at most 2 W - 1 inputs
        float* tnew = a.tail + (row * 2 + ((flags & RS_PAR) ? 0 : 1)) * a.tail_cap;
        const int64_t lo1 = rs_tail_lo(E1, L, M, W);
        for (int64_t k = lo1 + tid; k < S1; k += RS_THREADS) tnew[k - lo1] = k < S0 ? told[k - lo0] : x[k - S0];
    }
    const int64_t m0 = E0 + (int64_t)blockIdx.x * a.block;
    if (m0 >= E1) return;      // no output in this block (block-uniform: no barrier has been reached)
    float* y = a.out + row * a.out_pitch + (m0 - E0);      // the block's first output
    if (T == 0) {              // L = M = 1: the bits are copied (E0 = S0)
        for (int o = tid; o < a.block && m0 + o < E1; o += RS_THREADS) y[o] = x[m0 + o - S0];
        return;
    }
    const int64_t k00 = m0 * M / L, klo = k00 - W + 1;
    for (int i = tid; i < a.span; i += RS_THREADS) {
        const int64_t k = klo + i;
        span[i] = (k >= 0 && k < S1) ? (k < S0 ? told[k - lo0] : x[k - S0]) : 0.0f;
    }
    __syncthreads();
    // an output past the block or the row computes output m0 again and stores nothing
    const float* c[RS_PER_THREAD];
    const float* xs[RS_PER_THREAD];
    float acc[RS_PER_THREAD];
    bool live[RS_PER_THREAD];
#pragma unroll
    for (int r = 0; r < RS_PER_THREAD; ++r) {
        const int o = tid + r * RS_THREADS;
        live[r] = o < a.block && m0 + o < E1;
        const int64_t m = live[r] ? m0 + o : m0, mm = m * M;
        c[r] = a.C + (mm % L) * T;
        xs[r] = span + (mm / L - k00);      // tap j reads input k0 - W + 1 + j = klo + (k0 - k00) + j; the last index stays below a.span
        acc[r] = 0.0f;
    }
    for (int j = 0; j < (int)T; ++j) {
#pragma unroll
        for (int r = 0; r < RS_PER_THREAD; ++r) acc[r] = __fmaf_rn(c[r][j], xs[r][j], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < RS_PER_THREAD; ++r)
        if (live[r]) y[tid + r * RS_THREADS] = acc[r];
}

// the launches of planned rows: steps[b] for b < B
static int rs_launch(wn_resample* h, const float* in, int64_t in_pitch, int32_t B, float* out, int64_t out_pitch, bool state, hipStream_t st) {
    const RsPlan& p = h->plan;
    RsArgs a;
    a.in = in; a.C = h->table; a.out = out; a.tail = state ? h->tail.get() : nullptr;
    a.in_pitch = in_pitch; a.out_pitch = out_pitch;
    a.L = (int32_t)p.L; a.M = (int32_t)p.M; a.W = (int32_t)p.W; a.T = (int32_t)p.T; a.block = p.block; a.span = p.span; a.tail_cap = (int32_t)rs_tail_cap(p.W);
    for (int b0 = 0; b0 < B; b0 += RS_GROUP) {
        const int nb = B - b0 < RS_GROUP ? B - b0 : RS_GROUP;
        int64_t emit = 0;
        bool any = false;
        a.b0 = b0;
        for (int r = 0; r < RS_GROUP; ++r) {
            a.S0[r] = 0; a.n[r] = 0; a.flags[r] = 0;
            if (r >= nb || !h->steps[b0 + r].active) continue;
            const RsStep& s = h->steps[b0 + r];
            a.S0[r] = (int32_t)s.S0; a.n[r] = s.n;
            a.flags[r] = (uint8_t)(RS_ACTIVE | (s.final ? RS_FINAL : 0) | (s.par ? RS_PAR : 0));
            if (s.E1 - s.E0 > emit) emit = s.E1 - s.E0;
            any = any || s.E1 > s.E0 || (state && !s.final);      // (workgroup 0 stores the tail even without an output)
        }
        if (!any) continue;      // rows that are left alone launch nothing
        const int64_t blocks = emit > 0 ? rs_cdiv(emit, p.block) : 1;
        hipLaunchKernelGGL(wn_resample_kernel, dim3((unsigned)blocks, nb), dim3(RS_THREADS), (size_t)p.span * sizeof(float), st, a);
        WN_LAUNCH_CHECK(h);
    }
    return WN_OK;
}

extern "C" int wn_resample_create(const wn_resample_config* cfg, wn_resample** out) {
    wn_resample* z = nullptr;
    if (!cfg || !out) WN_FAIL(z, WN_E_ARG, "wn_resample_create: null argument");
    *out = nullptr;
    char msg[320];
    RsPlan plan;
    if (int rc = rs_check_config(cfg, &plan, msg, sizeof msg)) WN_FAIL(z, rc, "wn_resample_create: %s", msg);
    wn_resample* h = new wn_resample();
    h->cfg = *cfg; h->plan = plan;
    h->rows.resize(cfg->max_rows > 0 ? cfg->max_rows : RS_GROUP);
    h->steps.resize(h->rows.size());
    *out = h;
    if (cfg->max_rows == 0) return WN_OK;      // geometry-only handle: reserves nothing and never touches a device; run and push refuse any B
    std::vector<float> C;
    rs_build_table(*cfg, plan, &C);
    int rc = [&]() -> int {
        WN_HIP(h, h->table.reserve(C.size() > 0 ? C.size() : 1));
        WN_HIP(h, h->tail.reserve((size_t)cfg->max_rows * 2 * (size_t)rs_tail_cap(plan.W)));
        if (!C.empty()) WN_HIP(h, hipMemcpy(h->table, C.data(), C.size() * 4, hipMemcpyHostToDevice));
        return WN_OK;
    }();
    if (rc != WN_OK) { g_create_err = h->err; delete h; *out = nullptr; return rc; }
    return WN_OK;
}

extern "C" void wn_resample_destroy(wn_resample* h) { delete h; }

extern "C" const char* wn_resample_last_error(const wn_resample* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

extern "C" int64_t wn_resample_num_out(const wn_resample* h, int64_t n) {
    if (!h || n < 0 || n > 0x7fffffffLL) return (int64_t)WN_E_ARG;
    return rs_num_out(n, h->plan.L, h->plan.M);
}

extern "C" int64_t wn_resample_ready(const wn_resample* h, int64_t S, int32_t final) {
    if (!h || S < 0 || S > 0x7fffffffLL) return (int64_t)WN_E_ARG;
    return rs_ready(S, h->plan.L, h->plan.M, h->plan.W, final ? 1 : 0);
}

extern "C" int wn_resample_taps(const wn_resample* h, int32_t* L, int32_t* M, int32_t* W) {
    if (!h) return WN_E_ARG;
    if (L) *L = (int32_t)h->plan.L;
    if (M) *M = (int32_t)h->plan.M;
    if (W) *W = (int32_t)h->plan.W;
    return WN_OK;
}

extern "C" int wn_resample_run(wn_resample* h, const float* in, int64_t in_pitch, const int32_t* lengths, int32_t B, float* out, int64_t out_pitch, void* stream) {
    if (!h) return WN_E_ARG;
    char msg[256];
    // (B is checked against max_rows before any row is indexed: a geometry-only handle refuses every run there)
    if (int rc = rs_check_run("wn_resample_run", h->cfg, h->plan, h->cfg.max_rows, in, in_pitch, lengths, B, out, out_pitch, msg, sizeof msg)) WN_FAIL(h, rc, "%s", msg);
    for (int b = 0; b < B; ++b) {      // a whole row: from S = 0, final, nothing carried
        RsStep& s = h->steps[b];
        s.S0 = 0; s.S1 = lengths[b]; s.E0 = 0; s.E1 = rs_num_out(lengths[b], h->plan.L, h->plan.M); s.n = lengths[b]; s.active = lengths[b] > 0; s.final = 1; s.par = 0;
    }
    return rs_launch(h, in, in_pitch, B, out, out_pitch, false, (hipStream_t)stream);
}

extern "C" int wn_resample_push(wn_resample* h, const float* in, int64_t in_pitch, const int32_t* n, const int32_t* restart, const int32_t* final, int32_t B, float* out,
                                int64_t out_pitch, int32_t* n_out, void* stream) {
    if (!h) return WN_E_ARG;
    char msg[256];
    if (int rc = rs_plan_push("wn_resample_push", h->cfg, h->plan, h->cfg.max_rows, h->rows.data(), in, in_pitch, n, restart, final, B, out, out_pitch, n_out, h->steps.data(),
                              msg, sizeof msg))
        WN_FAIL(h, rc, "%s", msg);
    if (int rc = rs_launch(h, in, in_pitch, B, out, out_pitch, true, (hipStream_t)stream)) return rc;
    rs_commit_push(h->rows.data(), h->steps.data(), restart, B, n_out);
    return WN_OK;
}

extern "C" int wn_test_resample_table(const wn_resample_config* cfg, float* table, int64_t cap) {
    wn_resample* z = nullptr;
    char msg[320];
    RsPlan plan;
    if (int rc = rs_check_config(cfg, &plan, msg, sizeof msg)) WN_FAIL(z, rc, "wn_test_resample_table: %s", msg);
    if (!table || cap < plan.L * plan.T) WN_FAIL(z, WN_E_ARG, "wn_test_resample_table: the table holds %lld floats (cap = %lld)", (long long)(plan.L * plan.T), (long long)cap);
    std::vector<float> C;
    rs_build_table(*cfg, plan, &C);
    for (size_t i = 0; i < C.size(); ++i) table[i] = C[i];
    return WN_OK;
}

extern "C" int wn_test_resample_host(const wn_resample_config* cfg, const float* in, int64_t in_pitch, const int32_t* n, const int32_t* restart, const int32_t* final, int32_t P,
                                     int32_t B, float* out, int64_t out_pitch, int32_t* n_out) {
    wn_resample* z = nullptr;
    char msg[320];
    RsPlan plan;
    if (int rc = rs_check_config(cfg, &plan, msg, sizeof msg)) WN_FAIL(z, rc, "wn_test_resample_host: %s", msg);
    if (P < 0 || B < 1) WN_FAIL(z, WN_E_ARG, "wn_test_resample_host: P (%d) must be >= 0 and B (%d) >= 1", P, B);
    if (P > 0 && (!n || !out || !n_out)) WN_FAIL(z, WN_E_ARG, "wn_test_resample_host: null argument");
    std::vector<float> C;
    rs_build_table(*cfg, plan, &C);
    std::vector<RsRow> rows((size_t)B);
    std::vector<RsStep> steps((size_t)B);
    std::vector<std::vector<float>> tails((size_t)B);
    for (int64_t p = 0; p < P; ++p) {
        const int32_t* np = n + p * B; const int32_t* rp = restart ? restart + p * B : nullptr; const int32_t* fp = final ? final + p * B : nullptr;
        const float* ip = in ? in + p * B * in_pitch : nullptr;
        float* op = out + p * B * out_pitch;
        if (int rc = rs_plan_push("wn_test_resample_host", *cfg, plan, -1, rows.data(), ip, in_pitch, np, rp, fp, B, op, out_pitch, n_out + p * B, steps.data(), msg, sizeof msg))
            WN_FAIL(z, rc, "push %lld: %s", (long long)p, msg);
        for (int b = 0; b < B; ++b) rs_host_push_row(plan, C.data(), steps[b], &tails[b], ip ? ip + (int64_t)b * in_pitch : nullptr, op + (int64_t)b * out_pitch);
        rs_commit_push(rows.data(), steps.data(), rp, B, n_out + p * B);
    }
    return WN_OK;
}
