// Host driver shared by the two launch-per-layer synthesis paths (wn_synth.hip: bf16 MFMA steps, wn_synth_f32.hip: fp32 steps).
//
// WnStepRunner owns what "run n steps of a span" needs besides the step itself: the ctx-owned stream the steps are captured and replayed on (the
// caller's may be the legacy NULL stream, which cannot be captured), the two events that order it behind and in front of the caller's stream, and the
// hipGraphExec_t of `steps` steps with the key it was captured for.  Every step kernel reads its time index from device memory, so a graph is replayed
// unchanged for as long as the key -- every pointer and size the captured launches carry -- matches; anything else is captured again.
//     enter(caller) -> run(n, key, step) -> leave(caller);   everything is released with the runner (the stream is drained first: wn_dev.h).
#pragma once
#include "wn_common.h"

struct WnStepKey {      // compared bytewise: pointers first, no padding
    const void* p[7];   // noise, test_inputs, out_samples, out_raw, conditioning rows, gate-bias table, slot table (bf16 path; else null)
    int steps, B, T, Tcb;   // steps per graph, streams, row pitch of the outputs, conditioning rows per stream
};
static_assert(sizeof(WnStepKey) == 7 * sizeof(void*) + 4 * sizeof(int), "WnStepKey is compared with memcmp");

struct WnStepRunner {
    DevGraphExec gexec; WnStepKey key = {};
    DevEvent ev0, ev1;
    DevStream st;           // (declared last: destroyed, i.e. drained, first)

    int create(wn_ctx* c) {      // (once; inference-only contexts: at wn_create, through the path's reserve)
        WN_HIP(c, st.create(hipStreamNonBlocking));
        WN_HIP(c, ev0.create(hipEventDisableTiming));
        WN_HIP(c, ev1.create(hipEventDisableTiming));
        return WN_OK;
    }
    void drop_graph() { gexec.reset(); }
    // everything between enter and leave runs on `st`, after what the caller's stream holds now and before its next operation
    int enter(wn_ctx* c, hipStream_t caller) {
        WN_HIP(c, hipEventRecord(ev0, caller));
        WN_HIP(c, hipStreamWaitEvent(st, ev0, 0));
        return WN_OK;
    }
    int leave(wn_ctx* c, hipStream_t caller) {
        WN_HIP(c, hipEventRecord(ev1, st));
        WN_HIP(c, hipStreamWaitEvent(caller, ev1, 0));
        return WN_OK;
    }
    // n steps: replays of the graph of k.steps steps (k.steps > 1), then single steps.  step(stream) enqueues one step and returns a WN_ code;
    // a failed enqueue ends the capture before returning.
    template <class Step> int run(wn_ctx* c, int n, const WnStepKey& k, Step step) {
        int rc, done = 0;
        if (k.steps > 1 && n >= k.steps) {
            if (!gexec || memcmp(&k, &key, sizeof k) != 0) {
                drop_graph();
                DevGraphGuard graph;      // (destroyed on every way out, a failed instantiation included)
                WN_HIP(c, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
                for (int i = 0; i < k.steps; ++i)
                    if ((rc = step(st))) { hipStreamEndCapture(st, &graph.g); return rc; }
                WN_HIP(c, hipStreamEndCapture(st, &graph.g));
                WN_HIP(c, gexec.instantiate(graph.g));
                key = k;
            }
            for (; done + k.steps <= n; done += k.steps) WN_HIP(c, hipGraphLaunch(gexec, st));
        }
        for (; done < n; ++done) if ((rc = step(st))) return rc;
        return WN_OK;
    }
};

// ---- the first input of a span, for queues of bf16 (wn_synth.hip) or fp32 (wn_synth_f32.hip) elements
__device__ __forceinline__ void wn_queue_store(bf16_t* q, float v) { *q = f2bf(v); }
__device__ __forceinline__ void wn_queue_store(float* q, float v) { *q = v; }

// initial input (silence, wavenet.py:433-445) -> queue 0 slot 0; t = 0.  One block per tile of 32 streams (blockIdx.y): stream b = 32 * tile + n; the
// sampler of tile k > 0 keeps its own copy of the time index in t_dev[1 + k] (wn_synth_sample), tile 0 the one every other kernel reads
template <class Q>
__global__ void wn_synth_init(const float* __restrict__ Wf, const float* __restrict__ bf_, int R, int mode, int start_id, Q* __restrict__ ring0, int B, int32_t* t_dev) {
    const int tile = blockIdx.y, nb = min(32, B - 32 * tile);
    for (int o = threadIdx.x; o < nb * R; o += blockDim.x) {
        const int n = o / R, r = o - n * R;
        wn_queue_store(ring0 + ((size_t)32 * tile + n) * R + r, (mode == 2) ? Wf[(size_t)start_id * R + r] + bf_[r] : bf_[r]);      // x = 0 for raw / mulaw
    }
    if (threadIdx.x == 0) { if (tile == 0) { t_dev[0] = 0; t_dev[1] = 0; } else t_dev[1 + tile] = 0; }
}

// A span that begins an utterance (t0 == 0) zeroes the queues (wavenet.py:815-816: `SB` streams per queue row) and starts from silence; any other one
// continues from the queues, the time index and queue 0's next input its predecessor left, and only learns its first sample (t_dev[1]).
template <class Q>
static int wn_span_start(wn_ctx* c, const std::vector<DevBuf<Q>>& ring, const std::vector<int>& mask, int SB, int B, int32_t* t_dev, int t0, hipStream_t st) {
    if (t0 != 0) { WN_HIP(c, hipMemsetD32Async((hipDeviceptr_t)(t_dev + 1), t0, 1, st)); return WN_OK; }
    for (int l = 0; l < c->L; ++l) WN_HIP(c, hipMemsetAsync(ring[l], 0, (size_t)(mask[l] + 1) * SB * c->R * sizeof(Q), st));
    hipLaunchKernelGGL(wn_synth_init<Q>, dim3(1, (B + 31) / 32), dim3(256), 0, st, c->params_dev + c->first.dil_k, c->params_dev + c->first.dil_b, c->R, wn_sample_mode(c), 127, ring[0], B, t_dev);
    WN_LAUNCH_CHECK(c);
    return WN_OK;
}
