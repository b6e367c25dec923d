// Output stage: model-domain samples -> decoded, de-emphasised float32 and / or 16-bit PCM on the device (wn_post_* of include/wavenet_mi355.h).  Replaces,
// behind the synthesis routes, the host round trip of the reference's output path: the mu-law decode (util.py:94-129), inv_preemphasis (audio.py:27-30, a
// whole-utterance scipy lfilter) and save_wavenet_wav's peak normalisation and int16 cast (audio.py:17-20).
//
// y[t] = k y[t - 1] + x[t] is serial per row by definition, and it is evaluated that way -- one multiply and one add per sample, each rounded, in sample
// order -- because that is what makes a row bit-identical however it is cut into pushes and exactly reproducible in numpy float32 (a parallel scan
// reassociates and is neither).  Everything around the chain is parallel: one workgroup per row walks it in blocks of POST_BLK samples; all lanes load
// (16 bytes a lane where the row's address allows it) and decode into LDS, lane 0 runs the chain over the block in LDS, all lanes scale, clamp, convert,
// reduce peak / clipped and store.  Rows of a call run side by side; their lengths and restart flags travel by value, 32 rows a launch.  No atomics, nothing
// shared between workgroups, nothing allocated or synchronised after wn_post_create.
#define WN_POST_HOST_TABLES      // the hook decodes on the host
#include "wn_post.h"
#include "wn_common.h"

#define POST_GROUP 32          // rows per launch
#define POST_BLK 4096          // samples per LDS block (a multiple of 4: a block starts 16-byte aligned whenever its row does)
#define POST_THREADS 256

struct wn_post {
    wn_post_config cfg;
    std::string err;
    float pcm_scale = 0.f;             // wn_post_push: (float)(gain * 32767.0)
    DevBuf<float> state;               // [max_rows] carried y[-1] per row, then [max_rows] peaks of a wn_post_finish whose caller passes none
};

struct PostArgs {
    const int32_t* in; int64_t in_pitch; float* out_f32; int16_t* out_pcm; int64_t out_pitch;
    float* state; float* peak; int32_t* clipped;
    int32_t b0, finish; float k, s; uint32_t restart;      // restart: bit b = row b0 + b starts from y[-1] = 0
    int32_t n[POST_GROUP];
};

template <int TYPE>
__global__ __launch_bounds__(POST_THREADS) void wn_post_chain_kernel(const PostArgs a) {
    __shared__ __attribute__((aligned(16))) float blk[POST_BLK];
    __shared__ float red_peak[POST_THREADS];
    __shared__ int32_t red_clip[POST_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x, n = a.n[b];
    const int64_t row = a.b0 + b;
    const bool restart = a.finish || ((a.restart >> b) & 1u);
    if (n == 0) {      // block-uniform: no barrier has been reached.  An empty row keeps its state unless it is restarted
        if (tid == 0) {
            if (!a.finish && restart) a.state[row] = 0.0f;
            if (a.peak) a.peak[row] = 0.0f;
            if (a.clipped) a.clipped[row] = 0;
        }
        return;
    }
    const int32_t* in = a.in + row * a.in_pitch;
    float* of = a.out_f32 ? a.out_f32 + row * a.out_pitch : nullptr;
    int16_t* op = (a.out_pcm && !a.finish) ? a.out_pcm + row * a.out_pitch : nullptr;      // wn_post_finish converts in a launch of its own, once the peak is known
    const bool vin = ((uintptr_t)in & 15) == 0, vof = ((uintptr_t)of & 15) == 0, vop = ((uintptr_t)op & 7) == 0;
    float carry = 0.0f;
    if (tid == 0 && !restart) carry = a.state[row];
    float pk = 0.0f;
    int32_t nclip = 0;
    for (int64_t t0 = 0; t0 < n; t0 += POST_BLK) {
        const int m = (int)(n - t0 < POST_BLK ? n - t0 : POST_BLK);
        for (int i = tid * 4; i < m; i += POST_THREADS * 4) {      // all lanes: load, decode
            if (vin && i + 3 < m) {
                const int4 q = *reinterpret_cast<const int4*>(in + t0 + i);
                *reinterpret_cast<float4*>(blk + i) = make_float4(wn_decode_sample<TYPE>(q.x), wn_decode_sample<TYPE>(q.y), wn_decode_sample<TYPE>(q.z), wn_decode_sample<TYPE>(q.w));
            } else {
                for (int j = 0; j < 4 && i + j < m; ++j) blk[i + j] = wn_decode_sample<TYPE>(in[t0 + i + j]);
            }
        }
        __syncthreads();
        if (tid == 0) {                                            // one lane: the chain over the block, in place
            if (a.k != 0.0f) {
                const float k = a.k;
                float y = carry;
                int i = 0;
                for (; i + 3 < m; i += 4) {
                    float4 x = *reinterpret_cast<const float4*>(blk + i);
                    x.x = wn_post_step(k, y, x.x); x.y = wn_post_step(k, x.x, x.y); x.z = wn_post_step(k, x.y, x.z); x.w = wn_post_step(k, x.z, x.w);
                    y = x.w;
                    *reinterpret_cast<float4*>(blk + i) = x;
                }
                for (; i < m; ++i) { y = wn_post_step(k, y, blk[i]); blk[i] = y; }
                carry = y;
            } else carry = blk[m - 1];                             // k = 0: no arithmetic, y has the bits of x
        }
        __syncthreads();
        for (int i = tid * 4; i < m; i += POST_THREADS * 4) {      // all lanes: peak, scale, clamp, convert, store
            const int cnt = i + 3 < m ? 4 : m - i;
            float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            int16_t q[4] = {0, 0, 0, 0};
            for (int j = 0; j < cnt; ++j) {
                y[j] = blk[i + j];
                const float ab = fabsf(y[j]);
                if (ab > pk) pk = ab;
                if (op) q[j] = wn_post_pcm(y[j], a.s, &nclip);
            }
            if (of) {
                if (vof && cnt == 4) *reinterpret_cast<float4*>(of + t0 + i) = make_float4(y[0], y[1], y[2], y[3]);
                else for (int j = 0; j < cnt; ++j) of[t0 + i + j] = y[j];
            }
            if (op) {
                if (vop && cnt == 4) *reinterpret_cast<short4*>(op + t0 + i) = make_short4(q[0], q[1], q[2], q[3]);
                else for (int j = 0; j < cnt; ++j) op[t0 + i + j] = q[j];
            }
        }
        __syncthreads();                                           // the block is read: the next one may overwrite it
    }
    red_peak[tid] = pk; red_clip[tid] = nclip;
    __syncthreads();
    for (int h = POST_THREADS / 2; h > 0; h >>= 1) {               // a max and an integer sum: exact in any order
        if (tid < h) { red_peak[tid] = fmaxf(red_peak[tid], red_peak[tid + h]); red_clip[tid] += red_clip[tid + h]; }
        __syncthreads();
    }
    if (tid == 0) {
        if (!a.finish) a.state[row] = carry;
        if (a.peak) a.peak[row] = red_peak[0];
        if (a.clipped) a.clipped[row] = red_clip[0];
    }
}

// wn_post_finish, second launch: PCM of the de-emphasised rows at s = 32767 / max(0.01, peak) (double, on the device); four samples a lane
__global__ __launch_bounds__(POST_THREADS) void wn_post_convert_kernel(const PostArgs a) {
    const int b = blockIdx.y, n = a.n[b];
    const int64_t row = a.b0 + b;
    const int64_t i = ((int64_t)blockIdx.x * POST_THREADS + threadIdx.x) * 4;
    if (i >= n) return;
    const float s = wn_post_peak_scale(a.peak[row]);
    const float* y = a.out_f32 + row * a.out_pitch + i;
    int16_t* op = a.out_pcm + row * a.out_pitch + i;
    int32_t nclip = 0;
    if (i + 3 < n && ((uintptr_t)y & 15) == 0 && ((uintptr_t)op & 7) == 0) {
        const float4 v = *reinterpret_cast<const float4*>(y);
        *reinterpret_cast<short4*>(op) = make_short4(wn_post_pcm(v.x, s, &nclip), wn_post_pcm(v.y, s, &nclip), wn_post_pcm(v.z, s, &nclip), wn_post_pcm(v.w, s, &nclip));
    } else {
        for (int j = 0; j < 4 && i + j < n; ++j) op[j] = wn_post_pcm(y[j], s, &nclip);
    }
}

typedef void (*post_kernel_t)(const PostArgs);
static post_kernel_t post_kernel(int type) {
    return type == WN_INPUT_MULAW_QUANTIZE ? wn_post_chain_kernel<WN_INPUT_MULAW_QUANTIZE> : type == WN_INPUT_MULAW ? wn_post_chain_kernel<WN_INPUT_MULAW> : wn_post_chain_kernel<WN_INPUT_RAW>;
}

extern "C" int wn_post_create(const wn_post_config* cfg, wn_post** out) {
    wn_post* z = nullptr;
    if (!cfg || !out) WN_FAIL(z, WN_E_ARG, "wn_post_create: null argument");
    *out = nullptr;
    char msg[256];
    if (int rc = wn_post_check_config(cfg, msg, sizeof msg)) WN_FAIL(z, rc, "wn_post_create: %s", msg);
    wn_post* p = new wn_post();
    p->cfg = *cfg;
    p->pcm_scale = wn_post_gain_scale(cfg->gain);
    int rc = [&]() -> int {
        WN_HIP(p, p->state.reserve((size_t)cfg->max_rows * 2));
        WN_HIP(p, hipMemset(p->state, 0, p->state.bytes()));
        return WN_OK;
    }();
    if (rc != WN_OK) { g_create_err = p->err; delete p; return rc; }
    *out = p;
    return WN_OK;
}

extern "C" void wn_post_destroy(wn_post* p) { delete p; }

extern "C" const char* wn_post_last_error(const wn_post* p) { return p ? p->err.c_str() : g_create_err.c_str(); }

// the chain launches of one call, 32 rows each
static void post_launch(const wn_post* p, PostArgs& a, const int32_t* n, const int32_t* restart, int32_t B, hipStream_t st) {
    post_kernel_t kern = post_kernel(p->cfg.in_type);
    for (int b0 = 0; b0 < B; b0 += POST_GROUP) {
        const int nb = B - b0 < POST_GROUP ? B - b0 : POST_GROUP;
        a.b0 = b0; a.restart = 0;
        for (int b = 0; b < POST_GROUP; ++b) {
            a.n[b] = b < nb ? n[b0 + b] : 0;
            if (b < nb && restart && restart[b0 + b]) a.restart |= 1u << b;
        }
        hipLaunchKernelGGL(kern, dim3(nb), dim3(POST_THREADS), 0, st, a);
    }
}

extern "C" int wn_post_push(wn_post* p, const void* in, int64_t in_pitch, const int32_t* n, const int32_t* restart, int32_t B,
                            float* out_f32, int16_t* out_pcm, int64_t out_pitch, int32_t* clipped, void* stream) {
    if (!p) return WN_E_ARG;
    char msg[256];
    if (int rc = wn_post_check_call("wn_post_push", 0, p->cfg.max_rows, in, in_pitch, n, B, out_f32, out_pcm, out_pitch, msg, sizeof msg)) WN_FAIL(p, rc, "%s", msg);
    PostArgs a;
    a.in = (const int32_t*)in; a.in_pitch = in_pitch; a.out_f32 = out_f32; a.out_pcm = out_pcm; a.out_pitch = out_pitch;
    a.state = p->state; a.peak = nullptr; a.clipped = clipped; a.finish = 0; a.k = p->cfg.deemphasis; a.s = p->pcm_scale;
    post_launch(p, a, n, restart, B, (hipStream_t)stream);
    WN_LAUNCH_CHECK(p);
    return WN_OK;
}

extern "C" int wn_post_finish(wn_post* p, const void* in, int64_t in_pitch, const int32_t* n, int32_t B,
                              float* out_f32, int16_t* out_pcm, int64_t out_pitch, float* peak, void* stream) {
    if (!p) return WN_E_ARG;
    char msg[256];
    if (int rc = wn_post_check_call("wn_post_finish", 1, p->cfg.max_rows, in, in_pitch, n, B, out_f32, out_pcm, out_pitch, msg, sizeof msg)) WN_FAIL(p, rc, "%s", msg);
    PostArgs a;
    a.in = (const int32_t*)in; a.in_pitch = in_pitch; a.out_f32 = out_f32; a.out_pcm = out_pcm; a.out_pitch = out_pitch;
    a.state = p->state; a.peak = peak ? peak : p->state.get() + p->cfg.max_rows; a.clipped = nullptr; a.finish = 1; a.k = p->cfg.deemphasis; a.s = 0.0f;
    post_launch(p, a, n, nullptr, B, (hipStream_t)stream);
    if (out_pcm) {
        for (int b0 = 0; b0 < B; b0 += POST_GROUP) {
            const int nb = B - b0 < POST_GROUP ? B - b0 : POST_GROUP;
            int32_t n_max = 0;
            a.b0 = b0;
            for (int b = 0; b < POST_GROUP; ++b) { a.n[b] = b < nb ? n[b0 + b] : 0; if (a.n[b] > n_max) n_max = a.n[b]; }
            if (n_max > 0) hipLaunchKernelGGL(wn_post_convert_kernel, dim3(cdiv(n_max, POST_THREADS * 4), nb), dim3(POST_THREADS), 0, (hipStream_t)stream, a);
        }
    }
    WN_LAUNCH_CHECK(p);
    return WN_OK;
}

extern "C" int wn_test_post_host(const wn_post_config* cfg, const void* in, int64_t n, float carry_in, float pcm_scale, float* out_f32, int16_t* out_pcm, float* carry_out) {
    wn_post* z = nullptr;
    char msg[256];
    if (int rc = wn_post_check_config(cfg, msg, sizeof msg)) WN_FAIL(z, rc, "wn_test_post_host: %s", msg);
    if (n < 0 || (n > 0 && !in)) WN_FAIL(z, WN_E_ARG, "wn_test_post_host: n (%lld) < 0 or no input", (long long)n);
    wn_post_host_row(cfg->in_type, cfg->deemphasis, in, n, carry_in, pcm_scale, out_f32, out_pcm, carry_out, nullptr, nullptr);
    return WN_OK;
}
