// The product loops of the spectral denoiser, written once for the whole-utterance kernel (wn_denoise.hip) and the streaming kernel
// (wn_denoise_stream.hip): the forward product of 32 frames with one 32-bin group of the windowed DFT table, the shrink of that group into the tile's
// packed spectrum rows, and the inverse product of the tile's spectrum rows with one 32-sample column group of the inverse table.  Every (frame, bin)
// and (frame, sample) element is one row of the exact-fp32 matrix instruction: its bits depend on that frame's samples alone, never on which tile or
// which kernel the frame ran in.  Lane l of a wave: l31 = l % 32 (frame of the A operand / column of the B operand), lh = l / 32 (tap or packed column
// parity).  Accumulator register r of lane l is (frame 8 (r / 4) + 4 lh + r % 4, column l31).
#pragma once
#include "wn_denoise.h"
#include "wn_common.h"

__device__ __forceinline__ int dn_acc_frame(int r, int lh) { return (r >> 2) * 8 + lh * 4 + (r & 3); }

// sp: the staged span at frame l31's first tap + lh (largest index read: n_fft - 2 + lh); bp: fb + lh ldb + 64 g + l31.  Taps ascending in two
// interleaved chains that are joined once: re / im of (frame, bin 32 g + l31); bin 0's "im" is Re X[H].
__device__ __forceinline__ void dn_forward_group(const float* sp, const float* bp, int ldb, int N, f32x16_t* re, f32x16_t* im) {
    f32x16_t rc[2], ic[2];      // two chains per sum (MFMA steps alternate between them), joined once: half the length of every rounding chain
#pragma unroll
    for (int r = 0; r < 16; ++r) { rc[0][r] = 0.0f; rc[1][r] = 0.0f; ic[0][r] = 0.0f; ic[1][r] = 0.0f; }
    float nre[4], nim[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { nre[u] = bp[(size_t)(2 * u) * ldb]; nim[u] = bp[(size_t)(2 * u) * ldb + 32]; }
    for (int k0 = 0; k0 < N; k0 += 8) {      // n_fft is a multiple of 32: whole bodies of 8 taps, the next body's table loads in flight
        float bre[4], bim[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { bre[u] = nre[u]; bim[u] = nim[u]; }
        if (k0 + 8 < N) {
#pragma unroll
            for (int u = 0; u < 4; ++u) { nre[u] = bp[(size_t)(k0 + 8 + 2 * u) * ldb]; nim[u] = bp[(size_t)(k0 + 8 + 2 * u) * ldb + 32]; }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float av = sp[k0 + 2 * u];
            rc[u & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bre[u], rc[u & 1], 0, 0, 0);
            ic[u & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bim[u], ic[u & 1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) { (*re)[r] = __fadd_rn(rc[0][r], rc[1][r]); (*im)[r] = __fadd_rn(ic[0][r], ic[1][r]); }
}

// the shrink of group g on the accumulators, into the tile's 32 packed spectrum rows Y [32][n_fft]
__device__ __forceinline__ void dn_shrink_group(const f32x16_t& re, const f32x16_t& im, float* Y, const float* prof, float strength, int g, int N, int l31, int lh) {
    const int H = N / 2, bin = g * 32 + l31;
    const bool live = bin < H;
    const float t = live ? __fmul_rn(strength, prof[bin]) : 0.0f, tH = __fmul_rn(strength, prof[H]);
    float* y = Y + dn_spec_slot(live ? bin : 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int fr = dn_acc_frame(r, lh);
        float yr, yi, d;
        if (bin == 0) { dn_shrink(re[r], 0.0f, t, &yr, &d); dn_shrink(im[r], 0.0f, tH, &yi, &d); }
        else dn_shrink(re[r], im[r], t, &yr, &yi);
        if (live) { y[(size_t)fr * N] = yr; y[(size_t)fr * N + 4] = yi; }
    }
}

// yp: Y + l31 n_fft + 4 lh (lane l: frame l31, (re | im) of four consecutive bins); bq: ib + lh n_fft + 32 jg + l31.  Packed columns ascending in four
// interleaved chains joined pairwise: the windowed frame's samples 32 jg + l31 of the accumulator's frames.
__device__ __forceinline__ void dn_inverse_group(const float* yp, const float* bq, int N, f32x16_t* y) {
    f32x16_t acc[4];      // four chains (one per bin of a body of four), joined pairwise once
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[u][r] = 0.0f;
    for (int kb = 0; kb < N; kb += 8) {
        const f32x4_t a4 = *(const f32x4_t*)(yp + kb);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[u], bq[(size_t)(kb + 2 * u) * N], acc[u], 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) (*y)[r] = __fadd_rn(__fadd_rn(acc[0][r], acc[1][r]), __fadd_rn(acc[2][r], acc[3][r]));
}
