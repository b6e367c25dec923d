// Fast-WaveNet autoregressive synthesis (replaces WaveNet.incremental, wavenet.py:724-911).
//
// What differs from the reference's formulation:
//   * queues are RING BUFFERS of 4*d slots per layer, indexed t & (4d-1): O(1) per step instead of the
//     slice+concat rebuild of the whole [B,2d+1,R] queue (modules.py:285-288); unwritten slots are zero,
//     which is exactly the reference's zero-initialised queue (wavenet.py:815-816);
//   * per step and layer two tiny MFMA contractions replace ~20 TF ops: streams are the N dimension
//     of v_mfma_f32_32x32x16_bf16 (32 per tile; blockIdx.y is the tile: stream b = 32 * tile + (lane & 31), queue rows [slot][SB][R] with
//     SB = 32 * tiles -- one tile for wn_synthesize, streams and the slot sessions of up to 32 slots, ceil(B / 32) for wn_synthesize_wide and wide slot sessions), weights are the same fragment-ordered bf16 packs the
//     training kernels use (one coalesced 1-KiB load per wave and k-step, L2-resident), the 4 waves of
//     a workgroup split K and reduce through LDS;
//   * the whole step (2L+3 kernels) is captured once into a hipGraph of `steps_per_graph` steps; all
//     kernels read the time index from device memory so the graph is replayed unchanged (WnStepRunner, wn_steps.h).
// Host side: wn_synth_impl does the whole-utterance work of wn_synthesize once for all three paths and hands each of them a WnSpan;
// wn_synth_span is the only way into this path (a whole utterance, a stream push, a push of a slot session).
#include "wn_steps.h"
#include <stdlib.h>

// One owner of this kind serves the runs of up to 32 streams (wn_ctx::synth: SB = 32, one tile), a second one the wide runs and wide slot sessions (wn_ctx::wide: SB = 32 * tiles),
// each with its own runner, so that neither evicts the other's captured graph.
struct Synth {
    int B = 0, T = 0;
    int SB = 32;                   // streams per queue row of the RUNNING span, a multiple of 32; capSB: what the buffers hold
    int capSB = 0;
    std::vector<DevBuf<bf16_t>> ring; std::vector<int> mask;      // ring[l]: [4 d slots][SB][R]
    DevBuf<bf16_t> ucur;           // [SB][GH]
    DevBuf<float> skip_acc;        // [SB][S]
    DevBuf<bf16_t> h2;             // [SB][S]
    DevBuf<float> yraw;            // [SB][OP]
    DevBuf<int32_t> t_dev;         // [0] absolute time index of the next step, [1] first sample of the running span (0 for wn_synthesize; a stream push: its t0),
                                   // [1 + k] the sampler's own copy of [0] for tile k > 0
    WnStepRunner run;              // the ctx-owned stream the steps run on, the step graph and its key
    // slot sessions: sl != nullptr while a push of a session is enqueued -- one block of WN_SL_STRIDE entries per tile of 32 streams (tile k: sl + k * WN_SL_STRIDE),
    // in it [0..31] absolute index of every stream's next sample, [32..63] samples it generates in this push, [64] push-local step.  A stream whose count is
    // used up (or an idle slot) is a dummy for the rest of the push: its operand columns are zero, nothing of it is stored; a tile without a live slot runs
    // as dummies only.  Values live in device memory, so captured graphs stay valid across pushes.
    const int32_t* sl = nullptr;
};
#define WN_SL_N 32
#define WN_SL_STEP 64
// The block of this workgroup's tile.  Every tile keeps and advances its OWN push-local step (the hazard wn_synth_sample documents for t_dev: a block of
// tile k may start after tile 0's sampler stored the incremented step), so no kernel reads another tile's block.  ONE: tile 0, a compile-time fact.
template <bool ONE> __device__ __forceinline__ const int32_t* wn_sl_tile(const int32_t* sl) { return (ONE || !sl) ? sl : sl + (size_t)blockIdx.y * WN_SL_STRIDE; }

__device__ __forceinline__ f32x16_t zero16() { f32x16_t z; for (int i = 0; i < 16; ++i) z[i] = 0.0f; return z; }

// map (channel-in-tile ch, stream n) -> (lane, reg) of the 32x32 accumulator layout
__device__ __forceinline__ float acc_at(const float* red, int wave_stride, int nw, int tile, int ch, int n) {
    const int reg = ((ch >> 3) << 2) | (ch & 3), lane = n + 32 * ((ch >> 2) & 1);
    float s = 0.0f;
    for (int w = 0; w < nw; ++w) s += red[(size_t)w * wave_stride + (tile * 64 + lane) * 16 + reg];
    return s;
}

// Launch-per-layer kernels are LATENCY-bound (a few blocks per launch, one dependent chain of L2 reads per wave): round 5 splits K over NW waves
// (4 or 8 by the K of the launch) and issues EVERY fragment load of a wave up front (<= WN_SYN_MAXK k-steps per pass, unrolled and predicated:
// one L2 round trip per pass instead of one per k-step).  C5 width (G = 1024, K = 1616): 834 -> see profiles/ (DESIGN 3.4).
#define WN_SYN_MAXK 8
// ---- stage A: z = [W_dil | W_cin] [x(t-2d); x(t-d); x(t); c_t] + b  -> tanh * sigmoid -> u    (modules.py:273-303, 494-510)
// ONE: the launch has one tile of queue rows of 32 streams (every run of <= 32 streams, every slot session of <= 32 slots): tile index, row stride and the
// tile's block of the session table are compile-time
// constants of the same kernel, which then is the kernel of before the tile index (measured: profiles/wide_timing.json -> existing_path)
template <int NW, bool ONE>
__global__ __launch_bounds__(NW * 64) void wn_synth_gate(const bf16_t* __restrict__ Apk, int ksteps, const bf16_t* __restrict__ ring, int mask,
                                                     int d, int R, const bf16_t* __restrict__ cbt, int C, int Tcb, int B,
                                                     const float* __restrict__ bias, int bias_bstride, int GH, bf16_t* __restrict__ ucur,
                                                     const int32_t* __restrict__ t_dev, int kil, const int32_t* __restrict__ sla, int SBa) {
    __shared__ float red[NW * 2 * 64 * 16];
    const int32_t* const sl = wn_sl_tile<ONE>(sla);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5;
    const int SB = ONE ? 32 : SBa, b0 = ONE ? 0 : 32 * (int)blockIdx.y, b = b0 + n;      // streams per queue row; the tile's first stream, this lane's stream
    // absolute (queues) / span-local (conditioning rows cbt[n][tl], Tcb per stream); a slot session: both per stream, a dummy step multiplies zeros
    const int t = sl ? sl[n] : t_dev[0], tl = sl ? sl[WN_SL_STEP] : t - t_dev[1];
    const bool live = !sl || tl < sl[WN_SL_N + n];
    const int blk = blockIdx.x;
    f32x16_t acc0 = zero16(), acc1 = zero16();
    const bf16_t* A0 = Apk + ((size_t)(2 * blk) * ksteps * 64 + lane) * 8;
    const bf16_t* A1 = Apk + ((size_t)(2 * blk + 1) * ksteps * 64 + lane) * 8;
    for (int ks0 = wave; ks0 < ksteps; ks0 += NW * WN_SYN_MAXK) {
        uint4 bv[WN_SYN_MAXK], a0[WN_SYN_MAXK], a1[WN_SYN_MAXK];
#pragma unroll
        for (int i = 0; i < WN_SYN_MAXK; ++i) {
            const int ks = ks0 + i * NW;
            bv[i] = make_uint4(0, 0, 0, 0); a0[i] = make_uint4(0, 0, 0, 0); a1[i] = make_uint4(0, 0, 0, 0);
            if (ks < ksteps) {
                const int k0 = ks * 16 + h * 8;
                if (b < B && live) {
                    if (k0 < 3 * R) {
                        // K order of the pack: [tap0 | tap1 | tap2] or, interleaved in blocks of `kil` channels, [tap0 b0 | tap1 b0 | tap2 b0 | tap0 b1 | ...]
                        int j, r;
                        if (kil > 0) { const int kb = k0 / kil; j = kb % 3; r = (kb / 3) * kil + (k0 - kb * kil); }
                        else { j = k0 / R; r = k0 - j * R; }
                        const int tau = t - (2 - j) * d;
                        if (tau >= 0) bv[i] = *reinterpret_cast<const uint4*>(ring + ((size_t)(tau & mask) * SB + b) * R + r);
                    } else {
                        bv[i] = *reinterpret_cast<const uint4*>(cbt + ((size_t)b * Tcb + tl) * C + (k0 - 3 * R));
                    }
                }
                a0[i] = *reinterpret_cast<const uint4*>(A0 + (size_t)ks * 512);
                a1[i] = *reinterpret_cast<const uint4*>(A1 + (size_t)ks * 512);
            }
        }
#pragma unroll
        for (int i = 0; i < WN_SYN_MAXK; ++i) {      // (k-steps past the end multiply zeros)
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a0[i]), __builtin_bit_cast(bf16x8_t, bv[i]), acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a1[i]), __builtin_bit_cast(bf16x8_t, bv[i]), acc1, 0, 0, 0);
        }
    }
    float* my = red + (size_t)wave * (2 * 64 * 16);
#pragma unroll
    for (int r = 0; r < 16; ++r) { my[(0 * 64 + lane) * 16 + r] = acc0[r]; my[(1 * 64 + lane) * 16 + r] = acc1[r]; }
    __syncthreads();
    for (int o = tid; o < 32 * 32; o += NW * 64) {
        const int nn = o & 31, ch = o >> 5;
        if (b0 + nn >= B) continue;
        const int g = blk * 32 + ch;
        const float* const gb = bias + (size_t)(b0 + nn) * bias_bstride;          // per-stream bias under global conditioning (wavenet.py:766-777)
        const float za = acc_at(red, 2 * 64 * 16, NW, 0, ch, nn) + gb[g];
        const float zb = acc_at(red, 2 * 64 * 16, NW, 1, ch, nn) + gb[GH + g];
        const float e = __expf(2.0f * za);
        const float u = (1.0f - 2.0f / (e + 1.0f)) * (1.0f / (1.0f + __expf(-zb)));
        ucur[(size_t)(b0 + nn) * GH + g] = f2bf(u);
    }
}

// ---- stage B: x_next = (W_out u + b + x) * rho -> next layer's ring;  skip_acc += c_l W_skip u   (modules.py:512-521, wavenet.py:833-836)
template <int NW, bool ONE>
__global__ __launch_bounds__(NW * 64) void wn_synth_out(const bf16_t* __restrict__ Wo, const bf16_t* __restrict__ Ws, int ksteps,
                                                    int R, int S, const bf16_t* __restrict__ ucur, int GH,
                                                    const float* __restrict__ out_bias, float rho,
                                                    const bf16_t* __restrict__ ring_cur, int mask_cur,
                                                    bf16_t* __restrict__ ring_next, int mask_next,
                                                    float* __restrict__ skip_acc, int first_layer, int B,
                                                    const int32_t* __restrict__ t_dev, const int32_t* __restrict__ sla, int SBa) {
    __shared__ float red[NW * 64 * 16];
    const int32_t* const sl = wn_sl_tile<ONE>(sla);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t0_ = sl ? 0 : *t_dev;
    const int n = lane & 31, h = lane >> 5;
    const int SB = ONE ? 32 : SBa, b0 = ONE ? 0 : 32 * (int)blockIdx.y, b = b0 + n;
    const int mt = blockIdx.x;
    const int nR = R >> 5;
    const bool is_skip = mt >= nR;
    if (!is_skip && ring_next == nullptr) return;        // top layer: residual output unused
    const bf16_t* A = (is_skip ? Ws + ((size_t)(mt - nR) * ksteps * 64 + lane) * 8 : Wo + ((size_t)mt * ksteps * 64 + lane) * 8);
    f32x16_t acc = zero16();
    for (int ks0 = wave; ks0 < ksteps; ks0 += NW * WN_SYN_MAXK) {
        uint4 bv[WN_SYN_MAXK], av[WN_SYN_MAXK];
#pragma unroll
        for (int i = 0; i < WN_SYN_MAXK; ++i) {
            const int ks = ks0 + i * NW;
            bv[i] = make_uint4(0, 0, 0, 0); av[i] = make_uint4(0, 0, 0, 0);
            if (ks < ksteps) {
                if (b < B) bv[i] = *reinterpret_cast<const uint4*>(ucur + (size_t)b * GH + ks * 16 + h * 8);
                av[i] = *reinterpret_cast<const uint4*>(A + (size_t)ks * 512);
            }
        }
#pragma unroll
        for (int i = 0; i < WN_SYN_MAXK; ++i)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, av[i]), __builtin_bit_cast(bf16x8_t, bv[i]), acc, 0, 0, 0);
    }
    float* my = red + (size_t)wave * (64 * 16);
#pragma unroll
    for (int r = 0; r < 16; ++r) my[lane * 16 + r] = acc[r];
    __syncthreads();
    for (int o = tid; o < 32 * 32; o += NW * 64) {
        const int nn = o & 31, ch = o >> 5;
        if (b0 + nn >= B) continue;
        const float v = acc_at(red, 64 * 16, NW, 0, ch, nn);
        if (is_skip) {
            const int s = (mt - nR) * 32 + ch;
            float* p = skip_acc + (size_t)(b0 + nn) * S + s;
            *p = first_layer ? v : (*p + v);
        } else {
            const int r = mt * 32 + ch;
            const int t = sl ? sl[nn] : t0_;
            if (sl && sl[WN_SL_STEP] >= sl[WN_SL_N + nn]) continue;      // a dummy step writes no queue row
            const float x = bf2f(ring_cur[((size_t)(t & mask_cur) * SB + b0 + nn) * R + r]);
            ring_next[((size_t)(t & mask_next) * SB + b0 + nn) * R + r] = f2bf((v + out_bias[r] + x) * rho);
        }
    }
}

// ---- head 1: h2 = relu(W1 relu(skips + b_skip) + b1)     (wavenet.py:840-844)
template <bool ONE>
__global__ __launch_bounds__(256) void wn_synth_head1(const bf16_t* __restrict__ Apk, int ksteps, int S, const float* __restrict__ skip_acc,
                                                      const float* __restrict__ skip_bias, const float* __restrict__ b1,
                                                      bf16_t* __restrict__ h2, int B) {
    __shared__ float red[4 * 64 * 16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5, mt = blockIdx.x;
    const int b0 = ONE ? 0 : 32 * (int)blockIdx.y, b = b0 + n;
    const bf16_t* A = Apk + ((size_t)mt * ksteps * 64 + lane) * 8;
    f32x16_t acc = zero16();
    for (int ks = wave; ks < ksteps; ks += 4) {
        uint32_t w[4] = {0, 0, 0, 0};
        if (b < B) {
            const float* p = skip_acc + (size_t)b * S + ks * 16 + h * 8;
            const float* bb = skip_bias + ks * 16 + h * 8;
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = pack_bf2(fmaxf(p[2 * i] + bb[2 * i], 0.0f), fmaxf(p[2 * i + 1] + bb[2 * i + 1], 0.0f));
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(A + (size_t)ks * 512)),
                                                      __builtin_bit_cast(bf16x8_t, make_uint4(w[0], w[1], w[2], w[3])), acc, 0, 0, 0);
    }
    float* my = red + (size_t)wave * (64 * 16);
#pragma unroll
    for (int r = 0; r < 16; ++r) my[lane * 16 + r] = acc[r];
    __syncthreads();
    for (int o = tid; o < 32 * 32; o += 256) {
        const int nn = o & 31, ch = o >> 5;
        if (b0 + nn >= B) continue;
        const int s = mt * 32 + ch;
        h2[(size_t)(b0 + nn) * S + s] = f2bf(fmaxf(acc_at(red, 64 * 16, 4, 0, ch, nn) + b1[s], 0.0f));
    }
}

// ---- head 2: y = W2 h2 + b2  -> yraw[n][o]
template <bool ONE>
__global__ __launch_bounds__(256) void wn_synth_head2(const bf16_t* __restrict__ Apk, int ksteps, int S, const bf16_t* __restrict__ h2,
                                                      const float* __restrict__ b2, float* __restrict__ yraw, int O, int OP, int B) {
    __shared__ float red[4 * 64 * 16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5, mt = blockIdx.x;
    const int b0 = ONE ? 0 : 32 * (int)blockIdx.y, b = b0 + n;
    const bf16_t* A = Apk + ((size_t)mt * ksteps * 64 + lane) * 8;
    f32x16_t acc = zero16();
    for (int ks = wave; ks < ksteps; ks += 4) {
        uint4 bv = make_uint4(0, 0, 0, 0);
        if (b < B) bv = *reinterpret_cast<const uint4*>(h2 + (size_t)b * S + ks * 16 + h * 8);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(A + (size_t)ks * 512)),
                                                      __builtin_bit_cast(bf16x8_t, bv), acc, 0, 0, 0);
    }
    float* my = red + (size_t)wave * (64 * 16);
#pragma unroll
    for (int r = 0; r < 16; ++r) my[lane * 16 + r] = acc[r];
    __syncthreads();
    for (int o = tid; o < 32 * 32; o += 256) {
        const int nn = o & 31, ch = o >> 5;
        const int oc = mt * 32 + ch;
        if (b0 + nn >= B || oc >= O) continue;
        yraw[(size_t)(b0 + nn) * OP + oc] = acc_at(red, 64 * 16, 4, 0, ch, nn) + b2[oc];
    }
}

// ---- sampler + bookkeeping + input convolution of the NEXT step      (wavenet.py:847-878, 826)
// mode 0 MoL, 1 Gaussian, 2 categorical.  noise [T][B][nps].  One block per tile of 32 streams (blockIdx.y).  Tile 0 advances t_dev[0], the index every
// other kernel reads; a block of another tile may start after that store, so tile k > 0 keeps and advances its own copy t_dev[1 + k] (wn_synth_init).
template <bool ONE>
__global__ __launch_bounds__(256) void wn_synth_sample(const float* __restrict__ yraw, int O, int OP, int mode, int nps, float lsmin,
                                                       const float* __restrict__ noise, const void* __restrict__ test_inputs,
                                                       void* __restrict__ out_samples, float* __restrict__ out_raw,
                                                       const float* __restrict__ Wf, const float* __restrict__ bf_, int R,
                                                       bf16_t* __restrict__ ring0, int mask0, int B, int T, int32_t* __restrict__ t_dev, int32_t* __restrict__ sla, int SBa) {
    int32_t* const sl = const_cast<int32_t*>(wn_sl_tile<ONE>(sla));
    __shared__ float nxt_f[32];
    __shared__ int nxt_i[32];
    __shared__ int t_n[32];
    __shared__ int live_n[32];
    const int tid = threadIdx.x;
    const int SB = ONE ? 32 : SBa, b0 = ONE ? 0 : 32 * (int)blockIdx.y, nb = ONE ? B : min(32, B - b0);      // streams per queue row; the tile's first stream and its streams
    int32_t* const t_own = (ONE || blockIdx.y == 0) ? t_dev : t_dev + 1 + blockIdx.y;
    const int t = sl ? 0 : *t_own, tl = sl ? sl[WN_SL_STEP] : t - t_dev[1];      // ring slots by the absolute index; noise, teacher forcing and outputs [.., T] by the span's
    if (tid < 32) { t_n[tid] = sl ? sl[tid] : t; live_n[tid] = !sl || tl < sl[WN_SL_N + tid]; }      // (a slot session: per stream; T is then the row pitch of the outputs)
    __syncthreads();
    if (tid < nb && live_n[tid]) {
        const int n = tid;
        const size_t b = (size_t)b0 + n;
        const float* p = yraw + b * OP;
        const float* nz = noise + ((size_t)tl * B + b) * nps;
        if (mode == 2) {
            const int bi = sample_cat(p, 1, O, nz);
            ((int32_t*)out_samples)[b * T + tl] = bi;
            nxt_i[n] = test_inputs ? ((const int32_t*)test_inputs)[b * T + tl] : bi;
        } else {
            const float x = mode == 0 ? sample_mol(p, 1, O / 3, nz, lsmin) : sample_gauss(p, 1, nz, lsmin);
            ((float*)out_samples)[b * T + tl] = x;
            nxt_f[n] = test_inputs ? ((const float*)test_inputs)[b * T + tl] : x;
        }
    }
    if (out_raw) for (int o = tid; o < nb * O; o += 256) { const int n = o / O, oc = o - n * O; const size_t b = (size_t)b0 + n; if (live_n[n]) out_raw[(b * O + oc) * T + tl] = yraw[b * OP + oc]; }
    __syncthreads();
    // input convolution for step t+1 into ring 0
    for (int o = tid; o < nb * R; o += 256) {
        const int n = o / R, r = o - n * R;
        if (!live_n[n]) continue;
        const float v = (mode == 2) ? Wf[(size_t)nxt_i[n] * R + r] + bf_[r] : Wf[r] * nxt_f[n] + bf_[r];
        ring0[((size_t)((t_n[n] + 1) & mask0) * SB + b0 + n) * R + r] = f2bf(v);
    }
    __syncthreads();
    if (sl) { if (tid < nb && live_n[tid]) sl[tid] = t_n[tid] + 1; if (tid == 0) sl[WN_SL_STEP] = tl + 1; }
    else if (tid == 0) *t_own = t + 1;
}

// a push of a slot session: the samples every stream generates, the push-local step, and for the slots opened with this push (bit n of `fresh`) the
// input of their first step (silence) in ring 0 at THEIR index 0.  Nothing is cleared: a tap is valid iff t_n - k d >= 0, rows of an earlier occupant are unreachable.
// One launch serves ONE tile: its B <= 32 slots are the streams b0 .. b0 + B - 1 of the queue rows, `sl` is the tile's block, `fresh` and `cnt` are the tile's.
struct WnSlCounts { int32_t n[32]; };
__global__ void wn_synth_slots_setup(const float* __restrict__ Wf, const float* __restrict__ bf_, int R, int mode, int start_id, bf16_t* __restrict__ ring0, int B,
                                     int32_t* __restrict__ sl, WnSlCounts cnt, uint32_t fresh, int b0) {
    for (int o = threadIdx.x; o < B * R; o += blockDim.x) {
        const int n = o / R, r = o - n * R;
        if (!((fresh >> n) & 1u)) continue;
        const float v = (mode == 2) ? Wf[(size_t)start_id * R + r] + bf_[r] : bf_[r];
        ring0[((size_t)b0 + n) * R + r] = f2bf(v);
    }
    if (threadIdx.x < 32) { sl[WN_SL_N + threadIdx.x] = threadIdx.x < B ? cnt.n[threadIdx.x] : 0; if ((fresh >> threadIdx.x) & 1u) sl[threadIdx.x] = 0; }
    if (threadIdx.x == 0) sl[WN_SL_STEP] = 0;
}

void WnStateDelete::operator()(Synth* s) const { delete s; }

static int enqueue_step(wn_ctx* c, Synth* s, const bf16_t* cbt, int Tcb, const float* gbias, const float* noise, const void* test_inputs, void* out_samples,
                        float* out_raw, hipStream_t st) {
    const int L = c->L, R = c->R, GH = c->GH, S = c->S, C = c->C, B = s->B, T = s->T, SB = s->SB;
    const unsigned tiles = (unsigned)((B + 31) / 32);      // grid.y: 32 streams each (a run or a slot session of <= 32 streams: one)
    const bool one = tiles == 1 && SB == 32;
    for (int l = 0; l < L; ++l) {
        // waves per block by the K of the launch: every wave should get its k-steps in ONE pass of <= WN_SYN_MAXK loads
        const int ksg = c->packs[l].w1.K >> 4, kso = GH >> 4;
        const float* gbias_l = c->gin > 0 ? gbias + (size_t)l * B * c->G : c->b1sum + (size_t)l * c->G;
#define WN_LAUNCH_GATE(NW_, ONE_) hipLaunchKernelGGL((wn_synth_gate<NW_, ONE_>), dim3(GH / 32, tiles), dim3(NW_ * 64), 0, st, c->packs[l].w1.dev, ksg, s->ring[l], s->mask[l], \
                           c->dil[l], R, cbt, C, Tcb, B, gbias_l, c->gin > 0 ? c->G : 0, GH, s->ucur, s->t_dev, c->packs[l].w1.kil, s->sl, SB)
        if (one) { if (ksg > 4 * WN_SYN_MAXK) WN_LAUNCH_GATE(8, true); else WN_LAUNCH_GATE(4, true); }
        else { if (ksg > 4 * WN_SYN_MAXK) WN_LAUNCH_GATE(8, false); else WN_LAUNCH_GATE(4, false); }      // (16 waves = 1024 threads cap the kernel at 128 VGPRs: the up-front loads spill)
#undef WN_LAUNCH_GATE
        const bool top = (l == L - 1);
#define WN_LAUNCH_OUT(NW_, ONE_) hipLaunchKernelGGL((wn_synth_out<NW_, ONE_>), dim3(R / 32 + S / 32, tiles), dim3(NW_ * 64), 0, st, c->packs[l].wo.dev, c->packs[l].ws.dev, kso, R, S, s->ucur, GH, \
                           c->params_dev + c->lay[l].out_b, c->res_scale, s->ring[l], s->mask[l], top ? nullptr : s->ring[l + 1], top ? 0 : s->mask[l + 1], \
                           s->skip_acc, l == 0 ? 1 : 0, B, s->t_dev, s->sl, SB)
        if (one) { if (kso > 4 * WN_SYN_MAXK) WN_LAUNCH_OUT(8, true); else WN_LAUNCH_OUT(4, true); }
        else { if (kso > 4 * WN_SYN_MAXK) WN_LAUNCH_OUT(8, false); else WN_LAUNCH_OUT(4, false); }
#undef WN_LAUNCH_OUT
    }
#define WN_LAUNCH_HEAD(ONE_) do { \
    hipLaunchKernelGGL(wn_synth_head1<ONE_>, dim3(S / 32, tiles), dim3(256), 0, st, c->wh1.dev, S >> 4, S, s->skip_acc, c->skip_bias_total, c->params_dev + c->fin1_b, s->h2, B); \
    hipLaunchKernelGGL(wn_synth_head2<ONE_>, dim3(c->OP / 32, tiles), dim3(256), 0, st, c->wh2.dev, S >> 4, S, s->h2, c->params_dev + c->fin2_b, s->yraw, c->O, c->OP, B); \
    hipLaunchKernelGGL(wn_synth_sample<ONE_>, dim3(1, tiles), dim3(256), 0, st, s->yraw, c->O, c->OP, wn_sample_mode(c), wn_noise_per_step(c), wn_sample_lsmin(c), noise, test_inputs, out_samples, out_raw, \
                       c->params_dev + c->first.dil_k, c->params_dev + c->first.dil_b, R, s->ring[0], s->mask[0], B, T, s->t_dev, const_cast<int32_t*>(s->sl), SB); \
    } while (0)
    if (one) WN_LAUNCH_HEAD(true); else WN_LAUNCH_HEAD(false);
#undef WN_LAUNCH_HEAD
    WN_LAUNCH_CHECK(c);
    return WN_OK;
}

// state of the launch-per-layer path: ring queues for SB streams (a multiple of 32), per-step scratch, the capture stream (sizes do not depend
// on the utterance length)
static int synth_alloc(wn_ctx* c, Synth* s, int SB) {
    const int L = c->L, R = c->R;
    s->ring.resize(L); s->mask.assign(L, 0);
    for (int l = 0; l < L; ++l) {
        int slots = 4; while (slots < 4 * c->dil[l]) slots <<= 1;
        s->mask[l] = slots - 1;
        WN_HIP(c, s->ring[l].grow((size_t)slots * SB * R));
    }
    WN_HIP(c, s->ucur.grow((size_t)SB * c->GH));
    WN_HIP(c, s->skip_acc.grow((size_t)SB * c->S));
    WN_HIP(c, s->h2.grow((size_t)SB * c->S));
    WN_HIP(c, s->yraw.grow((size_t)SB * c->OP));
    WN_HIP(c, s->t_dev.grow(2 + SB / 32));
    s->capSB = SB;
    return WN_OK;
}
// the owner of the runs of <= 32 streams.  wn_create calls this on inference-only contexts; training contexts get here on first use.
int wn_synth_reserve(wn_ctx* c) {
    if (c->synth) return WN_OK;
    c->synth.reset(new Synth());
    Synth* s = c->synth.get();
    int rc = synth_alloc(c, s, 32);
    if (rc) return rc;
    return s->run.create(c);
}
// the owner of the wide runs, for B streams: it grows to the largest B seen on a training context; an inference-only context sizes it once, at wn_create
int wn_synth_wide_reserve(wn_ctx* c, int B) {
    const int SB = 32 * ((B + 31) / 32);
    int rc;
    if (!c->wide) { c->wide.reset(new Synth()); if ((rc = c->wide->run.create(c))) return rc; }
    Synth* s = c->wide.get();
    if (SB <= s->capSB) return WN_OK;
    if (c->inference && s->capSB > 0) WN_FAIL(c, WN_E_SHAPE, "wide synthesis: %d streams exceed the %d this inference-only context was sized for", B, s->capSB);
    if (s->capSB > 0) WN_HIP(c, hipStreamSynchronize(s->run.st));      // (growing: nothing may still read the old queues)
    s->run.drop_graph();
    s->capSB = 0;
    return synth_alloc(c, s, SB);
}

// The bf16 path of wn_synthesize(steps_per_graph) for B streams (a stream keeps the answer of its begin: the same path gives the same bits).
// steps_per_graph <= 0 selects the persistent dataflow pipeline (wn_synth_pipe.hip) when the model fits it; WN_SYNTH_MODE=graph|pipe overrides.
// (an inference-only context never grows its pre-sized pipeline: a batch beyond pipe_cap takes the launch-per-layer path, as
// wn_synth_pipe_eligible tells the caller -- ADVICE round 5: this dispatch used to ignore pipe_cap and fail in wn_pipe_reserve)
bool wn_synth_takes_pipe(const wn_ctx* c, int B, int steps_per_graph) {
    const char* m = getenv("WN_SYNTH_MODE");
    const bool want_pipe = m ? (strcmp(m, "pipe") == 0) : (steps_per_graph <= 0);
    const bool over_cap = c->inference && c->pipe_cap > 0 && B > c->pipe_cap;
    return want_pipe && !over_cap && wn_pipe_eligible(c, B);
}

// wn_synthesize: the whole-utterance work, once for all three paths, then the utterance as ONE span from silence on the path of steps_per_graph.
// The conditioning is upsampled on the caller's stream: every path orders its own stream behind it when it is entered.
int wn_synth_impl(wn_ctx* c, const float* cin, int B, int Tc, const float* noise, uint64_t, const void* test_inputs,
                  void* out_samples, float* out_raw, int steps_per_graph, hipStream_t st, bool wide) {
    const int T = Tc * c->hop;
    if ((int64_t)B * T > c->NT) WN_FAIL(c, WN_E_SHAPE, "synthesis B*T = %d*%d exceeds the workspace (max_batch*max_time = %lld)", B, T, (long long)c->NT);
    if (c->gin > 0 && (!c->have_g || c->gB != B))
        WN_FAIL(c, WN_E_STATE, "global conditioning is enabled: call wn_set_global_condition with this batch (B=%d) first [wavenet.py:766-777]", B);
    c->fB = B; c->fT = T; c->fTc = Tc; c->fup_pitch = 0;
    int rc = wn_upsample_fwd(c, nullptr, cin, B, Tc, st);      // cbt [B*T][C] bf16, CUP [B][C][T] fp32 (wavenet.py:781-803)
    if (rc) return rc;
    if ((rc = wn_gbias_fwd(c, B, st))) return rc;              // global conditioning of this batch (wavenet.py:766-777)
    WnSpan sp;
    sp.t0 = 0; sp.Tcb = T; sp.cbt_off = 0; sp.carry = nullptr; sp.gbias = c->gbias; sp.whole = true;
    if (wide) return wn_synth_wide_span(c, B, T, sp, noise, test_inputs, out_samples, out_raw, steps_per_graph, st);      // wn_synthesize_wide: always this path (bf16 modes only)
    // fp32: the reference's own arithmetic (fp32 weights, queues, accumulation), its own launch-per-layer path, never the bf16 pipeline
    if (c->cfg.compute_dtype == WN_COMPUTE_F32) return wn_synth_f32_span(c, B, T, sp, noise, test_inputs, out_samples, out_raw, steps_per_graph, st);
    if (wn_synth_takes_pipe(c, B, steps_per_graph)) return wn_pipe_span(c, B, T, sp, noise, test_inputs, out_samples, out_raw, st);
    return wn_synth_span(c, B, T, sp, noise, test_inputs, out_samples, out_raw, steps_per_graph, st);
}

// T steps of a span on this path.  A span with t0 > 0 continues from the queues, the time index and ring 0's next input its predecessor left (its last
// step wrote ring0[(t + 1) & mask0]); its first sample goes to t_dev[1] in device memory, so captured graphs stay valid whatever t0 is.  The conditioning
// rows are cbt[b][sp.cbt_off + t] of a window of sp.Tcb.  A push of a slot session (sp.st0): T steps, every stream with its own index and count in the
// session's device table, outputs at a pitch of sp.out_pitch, conditioning rows from the session's own table.
static int synth_span_on(wn_ctx* c, Synth* s, int SB, int B, int T, const WnSpan& sp, const float* noise, const void* test_inputs, void* out_samples, float* out_raw,
                         int steps_per_graph, hipStream_t caller_st) {
    int rc;
    c->synth_path = 1;
    s->SB = SB;
    if (steps_per_graph <= 0) steps_per_graph = 32;
    if ((rc = s->run.enter(c, caller_st))) return rc;
    hipStream_t st = s->run.st;
    s->B = B; s->T = sp.st0 ? sp.out_pitch : T; s->sl = nullptr;      // (T of the kernels: the row pitch of the outputs)
    if (sp.st0) {
        for (int k = 0; 32 * k < B; ++k) {      // one small launch per tile and push (the counts travel by value: 1 024 of them would not fit the kernel arguments)
            const int b0 = 32 * k, nbt = std::min(32, B - b0);
            WnSlCounts cnt; for (int i = 0; i < 32; ++i) cnt.n[i] = i < nbt ? sp.snl[b0 + i] : 0;
            hipLaunchKernelGGL(wn_synth_slots_setup, dim3(1), dim3(256), 0, st, c->params_dev + c->first.dil_k, c->params_dev + c->first.dil_b, c->R, wn_sample_mode(c), 127,
                               s->ring[0], nbt, sp.tdev + (size_t)k * WN_SL_STRIDE, cnt, sp.fresh[k], b0);
            WN_LAUNCH_CHECK(c);
        }
        s->sl = sp.tdev;
    } else if ((rc = wn_span_start(c, s->ring, s->mask, SB, B, s->t_dev, sp.t0, st))) return rc;
    const bf16_t* cbt = (sp.cbt ? sp.cbt : c->cbt) + (size_t)sp.cbt_off * c->C;
    const WnStepKey key = {{noise, test_inputs, out_samples, out_raw, cbt, sp.gbias, s->sl}, steps_per_graph, B, s->T, sp.Tcb};
    rc = s->run.run(c, T, key, [&](hipStream_t q) { return enqueue_step(c, s, cbt, sp.Tcb, sp.gbias, noise, test_inputs, out_samples, out_raw, q); });
    s->sl = nullptr;
    if (rc) return rc;
    return s->run.leave(c, caller_st);
}
int wn_synth_span(wn_ctx* c, int B, int T, const WnSpan& sp, const float* noise, const void* test_inputs, void* out_samples, float* out_raw,
                  int steps_per_graph, hipStream_t caller_st) {
    int rc = wn_synth_reserve(c);
    if (rc) return rc;
    return synth_span_on(c, c->synth.get(), 32, B, T, sp, noise, test_inputs, out_samples, out_raw, steps_per_graph, caller_st);
}
// A whole utterance, or a push of a wide slot session (sp.st0), of any B on the wide owner: the same steps with ceil(B / 32) tiles and queue rows of
// 32 * tiles streams.  (The key of the captured graph carries B, which fixes both.)
int wn_synth_wide_span(wn_ctx* c, int B, int T, const WnSpan& sp, const float* noise, const void* test_inputs, void* out_samples, float* out_raw,
                       int steps_per_graph, hipStream_t caller_st) {
    int rc = wn_synth_wide_reserve(c, B);
    if (rc) return rc;
    return synth_span_on(c, c->wide.get(), 32 * ((B + 31) / 32), B, T, sp, noise, test_inputs, out_samples, out_raw, steps_per_graph, caller_st);
}
