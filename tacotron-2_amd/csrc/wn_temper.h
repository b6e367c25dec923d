// Sampling temperature in the NOISE domain.  All three samplers (wn_common.h: sample_mol / sample_gauss / sample_cat, the pipeline's head,
// wn_synth_sample, the fp32 path) consume noise in a form where temperature is a change of the noise entry and not of the sampler:
//   select   (Gumbel-max choice of a mixture component / class)   argmax(logit_i - log(-log u_i))      the Gumbel term times tau
//   logistic (the draw of the chosen logistic)                    mu + exp(ls) (log u - log(1 - u))    the logit of u times tau
//   normal   (the Gaussian head's draw)                           mu + exp(ls) eps                     eps times tau
// so a tempered noise buffer run through the unchanged sampler IS the tempered sampler.  One function, used by the fused noise kernels, the
// stand-alone kernel (wn_temper_noise) and the host test hook (wn_test_temper_noise): fused and stand-alone callers give the same bits.
//   tau == 1   the entry comes back untouched (no arithmetic: bit-identical to the untempered stream)
//   tau == 0   constants: select -> exp(-1) (every Gumbel term equal: the arg-max logit wins), logistic -> 0.5 (its logit is exactly 0: the sample
//              is clip(mu)), normal -> 0
//   0 < tau <= 1   the clamp to [1e-5, 1 - 1e-5] never acts (checked in float32 over the whole clamped 24-bit grid)
//   1 < tau <= 2   the clamp TRUNCATES the tails: an entry whose tempered value leaves [1e-5, 1 - 1e-5] is pulled back to the range the samplers
//              were written for, so the tails are lighter than tau asks for
// Valid tau: finite, 0 <= tau <= 2 (wn_tau_valid); the entry points reject anything else with WN_E_ARG.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define WN_NOISE_LO 1e-5f
#define WN_NOISE_HI (1.0f - 1e-5f)

enum { WN_NZ_SELECT = 0, WN_NZ_LOGISTIC = 1, WN_NZ_NORMAL = 2 };

__host__ __device__ __forceinline__ bool wn_tau_valid(float tau) { return tau >= 0.0f && tau <= 2.0f; }      // (NaN fails both comparisons)

// kind of entry q of a sample's nps noise values.  mode 0 MoL: M = nps - 1 select entries, then the logistic draw; 1 Gaussian; 2 softmax
__host__ __device__ __forceinline__ int wn_noise_kind(int mode, int nps, int q) {
    return mode == 1 ? WN_NZ_NORMAL : (mode == 0 && q == nps - 1) ? WN_NZ_LOGISTIC : WN_NZ_SELECT;
}

__host__ __device__ __forceinline__ float wn_temper(float v, int kind, float tau) {
#pragma clang fp contract(off)
    if (tau == 1.0f) return v;
    if (kind == WN_NZ_NORMAL) return tau == 0.0f ? 0.0f : tau * v;
    float r;
    if (kind == WN_NZ_SELECT) {
        if (tau == 0.0f) return 0.36787945f;
        const float x = -logf(v);                 // -ln u > 0
        r = expf(-powf(x, tau));                  // -ln u' = (-ln u)^tau  <=>  Gumbel(u') = tau Gumbel(u)
    } else {
        if (tau == 0.0f) return 0.5f;
        const float l = logf(v) - logf(1.0f - v);
        const float z = tau * l;
        r = 1.0f / (1.0f + expf(-z));             // logit(u') = tau logit(u)
    }
    return fminf(fmaxf(r, WN_NOISE_LO), WN_NOISE_HI);
}

// entry q of a sample under the pair (tau_scale: logistic / normal draws, tau_select: Gumbel choices)
__host__ __device__ __forceinline__ float wn_temper_entry(float v, int mode, int nps, int q, float tau_scale, float tau_select) {
    const int kind = wn_noise_kind(mode, nps, q);
    return wn_temper(v, kind, kind == WN_NZ_SELECT ? tau_select : tau_scale);
}
