// Folded synthesis: one utterance generated as overlapping segments that run side by side as the rows of ONE slot-form span, and are cross-faded back
// into one waveform (include/wavenet_mi355.h: wn_fold_plan / wn_fold_check / wn_synthesize_folded).  Host: the planner, the validation of a plan, the
// fade tables, the driver.  Device: two plain streaming kernels -- the fold (rows of the whole utterances' upsampled conditioning into the session
// table; several rows read the same source, which wn_slots_scatter_kernel cannot express) and the unfold (decode + cross-fade).  The synthesis paths
// are entered through their span entries as they are.
#include "wn_common.h"
#include "wn_post.h"
#include <math.h>
#include <algorithm>
#include <vector>

// ---- planner (host only) ------------------------------------------------------------------------------------------------------------------------
extern "C" int wn_fold_plan(const int32_t* utt_frames, int32_t U, int32_t rows_max, int32_t warm, int32_t fade, int32_t min_keep, wn_fold_row* rows, int32_t cap) {
    if (!utt_frames || !rows || U < 1 || warm < 0 || fade < 0 || min_keep < 1) return WN_E_ARG;
    for (int u = 0; u < U; ++u) if (utt_frames[u] < 1) return WN_E_ARG;
    if (rows_max < U || rows_max > 32) return WN_E_SHAPE;
    int k[32]; bool open[32];
    for (int u = 0; u < U; ++u) { k[u] = 1; open[u] = true; }
    for (int left = rows_max - U; left > 0; --left) {
        // the utterance whose rows are currently longest (F_u / k_u as a fraction; ties: the lowest index) among those another row would not cut below min_keep
        int best = -1;
        for (int u = 0; u < U; ++u) {
            if (open[u] && utt_frames[u] / (k[u] + 1) < min_keep) open[u] = false;
            if (!open[u]) continue;
            if (best < 0 || (int64_t)utt_frames[u] * k[best] > (int64_t)utt_frames[best] * k[u]) best = u;
        }
        if (best < 0) break;
        ++k[best];
    }
    int n = 0;
    for (int u = 0; u < U; ++u) n += k[u];
    if (n > cap) return WN_E_SHAPE;
    n = 0;
    for (int u = 0; u < U; ++u) {
        const int64_t F = utt_frames[u];
        for (int j = 0; j < k[u]; ++j) {
            const int32_t a0 = (int32_t)(j * F / k[u]), a1 = (int32_t)((j + 1) * F / k[u]);
            const int32_t a2 = j + 2 <= k[u] ? (int32_t)((j + 2) * F / k[u]) : (int32_t)F;
            wn_fold_row& r = rows[n++];
            r.utt = u; r.keep = a0; r.first = std::max(0, a0 - warm);
            r.fade = j == 0 ? 0 : std::min(fade, a1 - a0);
            const int32_t end = j + 1 == k[u] ? (int32_t)F : a1 + std::min(fade, a2 - a1);      // the next row's keep + fade
            r.frames = end - r.first;
        }
    }
    return n;
}

extern "C" int wn_fold_check(const int32_t* utt_frames, int32_t U, const wn_fold_row* rows, int32_t n_rows, char* msg, int32_t cap) {
#define WN_FOLD_BAD(...) do { if (msg && cap > 0) snprintf(msg, (size_t)cap, __VA_ARGS__); return WN_E_ARG; } while (0)
    if (!utt_frames || !rows) WN_FOLD_BAD("folded synthesis: null utt_frames or rows");
    if (U < 1 || n_rows < U) WN_FOLD_BAD("folded synthesis: %d utterances need at least as many rows (got %d)", U, n_rows);
    for (int u = 0; u < U; ++u) if (utt_frames[u] < 1) WN_FOLD_BAD("folded synthesis: utterance %d has %d frames", u, utt_frames[u]);
    for (int r = 0; r < n_rows; ++r) {
        const wn_fold_row& w = rows[r];
        const int prev = r ? rows[r - 1].utt : -1;
        if (w.utt < 0 || w.utt >= U || (w.utt != prev && w.utt != prev + 1))
            WN_FOLD_BAD("folded synthesis: row %d names utterance %d: rows must be sorted by utterance and every utterance 0 ... %d needs one", r, w.utt, U - 1);
        const int F = utt_frames[w.utt];
        if (w.frames < 1 || w.first < 0 || w.fade < 0 || w.keep < w.first || (int64_t)w.keep + w.fade > (int64_t)w.first + w.frames || (int64_t)w.first + w.frames > F)
            WN_FOLD_BAD("folded synthesis: row %d (first %d, frames %d, keep %d, fade %d) violates 0 <= first <= keep, keep + fade <= first + frames <= %d frames of utterance %d",
                        r, w.first, w.frames, w.keep, w.fade, F, w.utt);
        if (w.utt != prev) {
            if (w.first != 0 || w.keep != 0 || w.fade != 0)
                WN_FOLD_BAD("folded synthesis: row %d is the first of utterance %d and must have first = keep = fade = 0 (got %d, %d, %d)", r, w.utt, w.first, w.keep, w.fade);
        } else {
            const wn_fold_row& p = rows[r - 1];
            if (w.keep + w.fade != p.first + p.frames)
                WN_FOLD_BAD("folded synthesis: row %d: keep + fade = %d must be where row %d ends (frame %d)", r, w.keep + w.fade, r - 1, p.first + p.frames);
            if (w.keep < p.keep + p.fade)
                WN_FOLD_BAD("folded synthesis: row %d: keep = %d lies inside the fade of row %d (which ends at frame %d)", r, w.keep, r - 1, p.keep + p.fade);
        }
        if ((r + 1 == n_rows || rows[r + 1].utt != w.utt) && w.first + w.frames != F)
            WN_FOLD_BAD("folded synthesis: row %d is the last of utterance %d and must end at its last frame (%d, got %d)", r, w.utt, F, w.first + w.frames);
    }
    if (rows[n_rows - 1].utt != U - 1) WN_FOLD_BAD("folded synthesis: utterance %d has no row", rows[n_rows - 1].utt + 1);
#undef WN_FOLD_BAD
    return WN_OK;
}

// float32 tables from double arithmetic on the host: the kernel only multiplies and adds
extern "C" int wn_fold_weights(int32_t fade_kind, int32_t n, float* w_in, float* w_out) {
    if (n < 1 || !w_in || !w_out || (fade_kind != 0 && fade_kind != 1)) return WN_E_ARG;
    for (int i = 0; i < n; ++i) {
        const double x = ((double)i + 0.5) / (double)n;
        w_in[i] = (float)(fade_kind == 0 ? sin(M_PI / 2 * x) : x);
        w_out[i] = (float)(fade_kind == 0 ? cos(M_PI / 2 * x) : 1.0 - x);
    }
    return WN_OK;
}

// ---- device -------------------------------------------------------------------------------------------------------------------------------------
// the table travels in kernel arguments: the host array is free when the launch returns, nothing is pinned and nothing waits
#define WN_FOLD_WCHUNK 512
struct WnFoldW { float v[WN_FOLD_WCHUNK]; };
__global__ void wn_fold_weights_kernel(float* __restrict__ dst, int n, WnFoldW w) {
    const int i = threadIdx.x + blockIdx.x * blockDim.x;
    if (i < n) dst[i] = w.v[i];
}

// (b) rows of a group of equally long utterances: row r copies n[r] samples from sample off[r] of group member gi[r] out of the group's upsampled
// conditioning cbt [g][Tw][C] (bf16) / cup [g][C][Tw] (fp32) into scbt [row][n_max][C] / feat [row][C][n_max], and its teacher-forcing inputs
// ti [U][wav_pitch] -> fti [row][row_pitch].  A row's cbt block is contiguous on both sides and C % 16 == 0: 16-byte copies always; the fp32 rows take
// 16-byte accesses when every pitch and offset is a multiple of 4 elements (vec_f / vec_t, decided by the host), else element by element.
struct WnFoldGrp { int32_t nr, row[32], gi[32], utt[32], off[32], n[32]; };
__global__ void wn_fold_kernel(const bf16_t* __restrict__ cbt, const float* __restrict__ cup, int64_t Tw, int C, bf16_t* __restrict__ scbt, float* __restrict__ feat, int64_t n_max,
                               const int32_t* __restrict__ ti, int64_t wav_pitch, int32_t* __restrict__ fti, int64_t row_pitch, int vec_f, int vec_t, WnFoldGrp p) {
    const int k = blockIdx.y;
    const int64_t n = p.n[k], r = p.row[k], g = p.gi[k], off = p.off[k];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n * C / 8)
        reinterpret_cast<uint4*>(scbt + r * n_max * C)[i] = reinterpret_cast<const uint4*>(cbt + (g * Tw + off) * C)[i];
    const int64_t nq = (n + 3) / 4;
    if (i < nq * C) {
        const int64_t ch = i / nq, t = (i - ch * nq) * 4;
        const float* s = cup + (g * C + ch) * Tw + off + t;
        float* d = feat + (r * C + ch) * n_max + t;
        if (vec_f && t + 3 < n) *reinterpret_cast<float4*>(d) = *reinterpret_cast<const float4*>(s);
        else for (int j = 0; j < 4 && t + j < n; ++j) d[j] = s[j];
    }
    if (ti && i < nq) {
        const int64_t t = i * 4;
        const int32_t* s = ti + (int64_t)p.utt[k] * wav_pitch + off + t;
        int32_t* d = fti + r * row_pitch + t;
        if (vec_t && t + 3 < n) *reinterpret_cast<int4*>(d) = *reinterpret_cast<const int4*>(s);
        else for (int j = 0; j < 4 && t + j < n; ++j) d[j] = s[j];
    }
}

// (f) decode of a model-domain sample: the arithmetic of wn_inv_mulaw_kernel / wn_inv_mulaw_quantize_kernel (wn_loss.hip), identity for 'raw'
// (wn_post.h: shared with the output stage)
template <int TYPE> __device__ __forceinline__ float fold_decode(int32_t bits) { return wn_decode_sample<TYPE>(bits); }
__device__ __forceinline__ float fold_xfade(float a, float w_out, float b, float w_in) {
#pragma clang fp contract(off)
    const float x = a * w_out;
    const float y = b * w_in;
    return x + y;
}
// rows of every utterance in SAMPLES: row r of utterance u = row0[u] ... row0[u + 1] - 1 covers [first, end), is the output from keep + fade on and fades in
// over [keep, keep + fade) with the weights at woff (w_in[fade], then w_out[fade])
struct WnUnfold { int32_t row0[33], len[32], first[32], keep[32], fade[32], woff[32]; };
template <int TYPE>
__global__ void wn_unfold_kernel(const int32_t* __restrict__ rows, int64_t row_pitch, const float* __restrict__ w, float* __restrict__ wav, int64_t wav_pitch, int vec, WnUnfold p) {
    const int u = blockIdx.y;
    const int64_t len = p.len[u];
    const int64_t s0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (s0 >= len) return;
    const int r0 = p.row0[u], r1 = p.row0[u + 1];
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int cnt = s0 + 3 < len ? 4 : (int)(len - s0);
    int r = r0;
    while (r + 1 < r1 && p.keep[r + 1] <= s0) ++r;            // the row that is (or fades) in at s0
    // four samples of one row's plain region at a 16-byte aligned place: one load
    if (vec && cnt == 4 && s0 >= (int64_t)p.keep[r] + p.fade[r] && (r + 1 == r1 || s0 + 3 < p.keep[r + 1]) && ((s0 - p.first[r]) & 3) == 0) {
        const int4 q = *reinterpret_cast<const int4*>(rows + r * row_pitch + (s0 - p.first[r]));
        v[0] = fold_decode<TYPE>(q.x); v[1] = fold_decode<TYPE>(q.y); v[2] = fold_decode<TYPE>(q.z); v[3] = fold_decode<TYPE>(q.w);
    } else {
        for (int j = 0; j < cnt; ++j) {
            const int64_t s = s0 + j;
            while (r + 1 < r1 && p.keep[r + 1] <= s) ++r;
            const float b = fold_decode<TYPE>(rows[r * row_pitch + (s - p.first[r])]);
            const int64_t i = s - p.keep[r];
            if (i < p.fade[r]) {                              // (the first row of an utterance has fade 0)
                const float a = fold_decode<TYPE>(rows[(r - 1) * row_pitch + (s - p.first[r - 1])]);
                v[j] = fold_xfade(a, w[p.woff[r] + p.fade[r] + i], b, w[p.woff[r] + i]);
            } else v[j] = b;
        }
    }
    float* d = wav + u * wav_pitch + s0;
    if (vec && cnt == 4) *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
    else for (int j = 0; j < cnt; ++j) d[j] = v[j];
}

// every whole utterance of a group side by side [g][C][F] (the upsample net takes a batch of equal width): member k = utterance utt[k] of c [U][C][F_max]
struct WnFoldUtts { int32_t utt[32]; };
__global__ void wn_fold_gather_kernel(const float* __restrict__ c, int64_t F_max, int64_t F, int C, float* __restrict__ win, WnFoldUtts p) {
    const int k = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C * F) return;
    const int64_t ch = i / F, f = i - ch * F;
    win[(int64_t)k * C * F + i] = c[((int64_t)p.utt[k] * C + ch) * F_max + f];
}

static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- driver -------------------------------------------------------------------------------------------------------------------------------------
extern "C" int wn_synthesize_folded(wn_ctx* c, const float* cc, const int32_t* utt_frames, int32_t U, const wn_fold_row* rows, int32_t n_rows, int32_t fade_kind,
                                    const void* g, const float* noise, uint64_t seed, const void* test_inputs, float* out_wav, int32_t wav_pitch,
                                    void* out_rows, float* out_raw, int32_t row_pitch, int32_t steps_per_graph, void* stream) {
    if (!c) return WN_E_ARG;
    if (c->cfg.compute_dtype == WN_COMPUTE_F32) WN_FAIL(c, WN_E_UNSUPPORTED, "wn_synthesize_folded: folded synthesis is not built for the fp32 validation mode (compute_dtype = WN_COMPUTE_F32)");
    if (!c->packed) WN_FAIL(c, WN_E_STATE, "wn_pack_weights must be called before wn_synthesize_folded");
    if (!cc || !out_wav) WN_FAIL(c, WN_E_ARG, "wn_synthesize_folded: null c or out_wav");
    if (fade_kind != 0 && fade_kind != 1) WN_FAIL(c, WN_E_ARG, "wn_synthesize_folded: fade_kind %d (0 equal power, 1 linear)", fade_kind);
    if ((c->gin > 0) != (g != nullptr)) WN_FAIL(c, WN_E_ARG, "wn_synthesize_folded: g must be given iff the model has global conditioning (gin_channels = %d)", c->gin);
    {
        char msg[400];
        if (wn_fold_check(utt_frames, U, rows, n_rows, msg, (int32_t)sizeof msg) != WN_OK) WN_FAIL(c, WN_E_ARG, "%s", msg);
    }
    if (n_rows > 32 || n_rows > c->maxB) WN_FAIL(c, WN_E_SHAPE, "wn_synthesize_folded: %d rows outside (0, min(32, max_batch = %d)]", n_rows, c->maxB);
    const int hop = c->hop, C = c->C;
    int64_t F_max = 0, n_max = 0;
    for (int u = 0; u < U; ++u) F_max = std::max<int64_t>(F_max, utt_frames[u]);
    for (int r = 0; r < n_rows; ++r) n_max = std::max<int64_t>(n_max, (int64_t)rows[r].frames * hop);
    if (n_max > c->maxT) WN_FAIL(c, WN_E_SHAPE, "wn_synthesize_folded: the longest row has %lld samples, max_time is %d", (long long)n_max, c->maxT);
    if ((int64_t)n_rows * n_max > c->NT) WN_FAIL(c, WN_E_SHAPE, "wn_synthesize_folded: %d rows x %lld samples exceed the workspace (max_batch * max_time = %lld)", n_rows, (long long)n_max, (long long)c->NT);
    if (F_max * hop > INT32_MAX || wav_pitch < F_max * hop) WN_FAIL(c, WN_E_ARG, "wn_synthesize_folded: wav_pitch %d < %lld samples of the longest utterance", wav_pitch, (long long)(F_max * hop));
    if ((out_rows || out_raw) && row_pitch < n_max) WN_FAIL(c, WN_E_ARG, "wn_synthesize_folded: row_pitch %d < %lld samples of the longest row", row_pitch, (long long)n_max);
    const int64_t pitch = (out_rows || out_raw) ? row_pitch : n_max;
    if ((!out_rows || test_inputs) && (int64_t)n_rows * pitch > c->NT)
        WN_FAIL(c, WN_E_SHAPE, "wn_synthesize_folded: %d rows at a pitch of %lld exceed the row scratch (max_batch * max_time = %lld)", n_rows, (long long)pitch, (long long)c->NT);
    // utterances of equal length are upsampled as one batch; a group's whole utterances must fit the workspace
    int grp_of[32], n_grp = 0, grp_F[32], grp_n[32];
    for (int u = 0; u < U; ++u) {
        int k = 0;
        while (k < n_grp && grp_F[k] != utt_frames[u]) ++k;
        if (k == n_grp) { grp_F[k] = utt_frames[u]; grp_n[k] = 0; ++n_grp; }
        grp_of[u] = k; ++grp_n[k];
    }
    for (int k = 0; k < n_grp; ++k)
        if ((int64_t)grp_n[k] * grp_F[k] * hop > c->NT)
            WN_FAIL(c, WN_E_SHAPE, "wn_synthesize_folded: %d utterances of %d frames (%lld samples) exceed the workspace (max_batch * max_time = %lld)", grp_n[k], grp_F[k],
                    (long long)grp_n[k] * grp_F[k] * hop, (long long)c->NT);
    c->strm.open = false; c->slots.open = false;            // (ends an open stream / slot session: its queues and tables are overwritten)
    int rc = wn_pipe_check(c, false);                       // a hand-off timeout of the previous pipeline run surfaces here at the latest
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    auto& S = c->slots;
    const int path = wn_synth_takes_pipe(c, n_rows, steps_per_graph) ? 2 : 1;
    if ((rc = wn_noise_reserve(c, n_rows, (int)n_max))) return rc;
    if ((rc = path == 2 ? wn_pipe_reserve(c, n_rows, c->maxT) : wn_synth_reserve(c))) return rc;
    if ((rc = wn_slots_alloc(c, std::min(32, c->maxB)))) return rc;
    // ---- fade tables: one per distinct fade length (sum of the fades <= n_rows x n_max <= what fw holds)
    WnUnfold uf; memset(&uf, 0, sizeof uf);
    {
        std::vector<float> tab; int done_fade[32], done_off[32], nd = 0;
        for (int r = 0; r < n_rows; ++r) {
            const int n = rows[r].fade * hop;
            if (n == 0) continue;
            int k = 0;
            while (k < nd && done_fade[k] != n) ++k;
            if (k == nd) {
                done_fade[k] = n; done_off[k] = (int)tab.size(); ++nd;
                tab.resize(tab.size() + 2 * (size_t)n);
                wn_fold_weights(fade_kind, n, tab.data() + done_off[k], tab.data() + done_off[k] + n);
            }
            uf.woff[r] = done_off[k];
        }
        for (size_t o = 0; o < tab.size(); o += WN_FOLD_WCHUNK) {
            WnFoldW w; const int n = (int)std::min<size_t>(WN_FOLD_WCHUNK, tab.size() - o);
            memcpy(w.v, tab.data() + o, (size_t)n * 4);
            hipLaunchKernelGGL(wn_fold_weights_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, S.fw + o, n, w);
            WN_LAUNCH_CHECK(c);
        }
    }
    // ---- (a) + (b): group by group, the whole utterances through the upsample net, then every row of the group out of the result
    int32_t* ti_rows = test_inputs ? S.fti.get() : nullptr;
    int32_t* row_buf = out_rows ? (int32_t*)out_rows : S.frow.get();
    for (int k = 0; k < n_grp; ++k) {
        const int64_t F = grp_F[k], Tw = F * hop;
        WnFoldUtts gu; memset(&gu, 0, sizeof gu); int member[32], ng = 0;
        for (int u = 0; u < U; ++u) if (grp_of[u] == k) { member[u] = ng; gu.utt[ng++] = u; }
        if (S.ftime) WN_HIP(c, hipEventRecord(S.fev[0], st));
        hipLaunchKernelGGL(wn_fold_gather_kernel, dim3(cdiv((int64_t)C * F, 256), ng), dim3(256), 0, st, cc, F_max, F, C, S.fwin, gu);
        WN_LAUNCH_CHECK(c);
        if ((rc = wn_upsample_fwd(c, nullptr, S.fwin, ng, (int)F, st))) return rc;
        if (S.ftime) WN_HIP(c, hipEventRecord(S.fev[1], st));
        WnFoldGrp p; memset(&p, 0, sizeof p); int64_t nmaxg = 0; bool a4 = true;
        for (int r = 0; r < n_rows; ++r) {
            if (grp_of[rows[r].utt] != k) continue;
            const int q = p.nr++;
            p.row[q] = r; p.gi[q] = member[rows[r].utt]; p.utt[q] = rows[r].utt; p.off[q] = rows[r].first * hop; p.n[q] = rows[r].frames * hop;
            nmaxg = std::max<int64_t>(nmaxg, p.n[q]); a4 = a4 && (p.off[q] & 3) == 0;
        }
        const int vec_f = a4 && (Tw & 3) == 0 && (n_max & 3) == 0 && al16(c->CUP[c->cup_final_idx]) && al16(S.feat.get());
        const int vec_t = a4 && (wav_pitch & 3) == 0 && (pitch & 3) == 0 && al16(test_inputs) && al16(ti_rows);
        hipLaunchKernelGGL(wn_fold_kernel, dim3(cdiv(nmaxg * C, 256), p.nr), dim3(256), 0, st, c->cbt, c->CUP[c->cup_final_idx], Tw, C, S.cbt, S.feat, n_max,
                           (const int32_t*)test_inputs, (int64_t)wav_pitch, ti_rows, pitch, vec_f, vec_t, p);
        WN_LAUNCH_CHECK(c);
        if (S.ftime) WN_HIP(c, hipEventRecord(S.fev[2], st));
    }
    // ---- (c) the gate-bias row of each row's utterance
    if (c->gin > 0) {
        const size_t gstride = c->cfg.use_speaker_embedding ? 4 : (size_t)c->gin * 4;
        for (int r = 0; r < n_rows; ++r)
            if ((rc = wn_gbias_row(c, (const char*)g + gstride * rows[r].utt, S.gbias, n_rows, r, st))) return rc;
    }
    // ---- (d) noise: column r = the one-stream noise of seed + r, tempered by the context's pair; caller noise is tempered into the context's buffer
    if (!noise) {
        uint64_t sd[32]; int64_t first[32], cnt[32]; float ts[32], tsel[32]; const int nps = wn_noise_per_step(c);
        for (int r = 0; r < n_rows; ++r) { sd[r] = seed + (uint64_t)r; first[r] = 0; cnt[r] = (int64_t)rows[r].frames * hop * nps; ts[r] = c->tau_scale; tsel[r] = c->tau_select; }
        if ((rc = wn_fill_noise_slots(c, c->noise_buf, n_rows, sd, first, cnt, ts, tsel, st))) return rc;
        noise = c->noise_buf;
    } else if (c->tau_scale != 1.0f || c->tau_select != 1.0f) {
        if ((rc = wn_temper_noise_impl(c, noise, c->noise_buf, n_rows, (int)n_max, c->tau_scale, c->tau_select, st))) return rc;
        noise = c->noise_buf;
    }
    // ---- (e) ONE span in the slot form: every row fresh at its own t = 0; `whole`: not a push, a failed run poisons nothing opened afterwards
    {
        int32_t st0[32], snl[32];
        for (int r = 0; r < 32; ++r) { st0[r] = 0; snl[r] = r < n_rows ? rows[r].frames * hop : 0; }
        WnSpan sp;
        sp.t0 = 0; sp.Tcb = (int)n_max; sp.cbt_off = 0; sp.carry = S.carry; sp.gbias = S.gbias; sp.whole = true;
        sp.st0 = st0; sp.snl = snl; sp.out_pitch = (int)pitch; sp.cbt = S.cbt; sp.reslice = true; sp.tdev = S.tdev;
        const uint32_t fresh = n_rows == 32 ? 0xffffffffu : ((1u << n_rows) - 1u);
        sp.fresh = &fresh;
        rc = path == 2 ? wn_pipe_span(c, n_rows, (int)n_max, sp, noise, ti_rows, row_buf, out_raw, st)
                       : wn_synth_span(c, n_rows, (int)n_max, sp, noise, ti_rows, row_buf, out_raw, steps_per_graph, st);
        if (rc) return rc;
        c->fB = n_rows; c->fT = (int)n_max; c->fTc = 0; c->fup_pitch = -1; S.feat_pitch = n_max; S.feat_B = n_rows;
    }
    // ---- (f) decode + cross-fade into one waveform per utterance
    {
        for (int r = 0; r < n_rows; ++r) {
            const int u = rows[r].utt;
            if (r == 0 || rows[r - 1].utt != u) uf.row0[u] = r;
            uf.first[r] = rows[r].first * hop; uf.keep[r] = rows[r].keep * hop; uf.fade[r] = rows[r].fade * hop;
        }
        for (int u = 0; u < U; ++u) uf.len[u] = utt_frames[u] * hop;
        uf.row0[U] = n_rows;
        const int vec = (wav_pitch & 3) == 0 && (pitch & 3) == 0 && al16(out_wav) && al16(row_buf);
        const dim3 grid(cdiv(cdiv(F_max * hop, 4), 256), U);
        const int type = c->cfg.input_type;
        if (S.ftime) WN_HIP(c, hipEventRecord(S.fev[3], st));
        if (type == WN_INPUT_RAW) hipLaunchKernelGGL(wn_unfold_kernel<WN_INPUT_RAW>, grid, dim3(256), 0, st, row_buf, pitch, S.fw, out_wav, (int64_t)wav_pitch, vec, uf);
        else if (type == WN_INPUT_MULAW) hipLaunchKernelGGL(wn_unfold_kernel<WN_INPUT_MULAW>, grid, dim3(256), 0, st, row_buf, pitch, S.fw, out_wav, (int64_t)wav_pitch, vec, uf);
        else hipLaunchKernelGGL(wn_unfold_kernel<WN_INPUT_MULAW_QUANTIZE>, grid, dim3(256), 0, st, row_buf, pitch, S.fw, out_wav, (int64_t)wav_pitch, vec, uf);
        WN_LAUNCH_CHECK(c);
        if (S.ftime) { WN_HIP(c, hipEventRecord(S.fev[4], st)); S.ftimed = true; }
    }
    return WN_OK;
}

// test hooks (tools/fold_timing.py): device time of the three steps a folded run adds around the span, by events on the caller's stream
extern "C" int wn_test_fold_timing(wn_ctx* c, int32_t enable) {
    if (!c) return WN_E_ARG;
    auto& S = c->slots;
    S.ftime = false; S.ftimed = false;
    if (enable) { for (auto& e : S.fev) WN_HIP(c, e.create()); S.ftime = true; }
    return WN_OK;
}
extern "C" int wn_test_fold_times(wn_ctx* c, double out_ms[3]) {
    if (!c || !out_ms) return WN_E_ARG;
    auto& S = c->slots;
    if (!S.ftime || !S.ftimed) WN_FAIL(c, WN_E_STATE, "wn_test_fold_times: no folded run since wn_test_fold_timing(ctx, 1)");
    WN_HIP(c, hipEventSynchronize(S.fev[4]));
    const int pair[3][2] = {{0, 1}, {1, 2}, {3, 4}};
    for (int i = 0; i < 3; ++i) { float ms = 0.0f; WN_HIP(c, hipEventElapsedTime(&ms, S.fev[pair[i][0]], S.fev[pair[i][1]])); out_ms[i] = ms; }
    return WN_OK;
}
