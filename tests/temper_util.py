"""Sampling temperature in the noise domain (csrc/wn_temper.h), restated in numpy: the three formulas with their clamp on a [rows, nps] array of a
head's noise, in float64 (the reference) or in plain numpy float32 (the yardstick: what the same formulas give when every operation rounds to
float32), and the error measure of the accuracy tests -- taken where the sampler reads the noise, normalised by what storing u' in float32 makes
unavoidable."""
import numpy as np

LO = np.float32(1e-5)
HI = np.float32(1.0) - np.float32(1e-5)
SELECT, LOGISTIC, NORMAL = 0, 1, 2
MOL, GAUSS, SOFTMAX = 0, 1, 2
TAUS = (0.1, 0.5, 0.8, 0.95, 1.5, 2.0)
SELECT_AT_ZERO, LOGISTIC_AT_ZERO, NORMAL_AT_ZERO = np.float32(0.36787945), np.float32(0.5), np.float32(0.0)


def kinds(mode, nps):
    """kind of each of a sample's nps entries: MoL = nps - 1 select entries then the logistic draw, Gaussian = normal, softmax = select"""
    k = np.full(nps, NORMAL if mode == GAUSS else SELECT, dtype=np.int64)
    if mode == MOL:
        k[nps - 1] = LOGISTIC
    return k


def temper_kind(v, kind, tau, dtype=np.float64):
    """one kind of entry at temperature tau, every operation in `dtype`"""
    v = np.asarray(v).astype(dtype)
    t = dtype(np.float32(tau))
    one = dtype(1.0)
    if kind == NORMAL:
        return t * v
    if kind == SELECT:
        r = np.exp(-np.power(-np.log(v), t))
    else:
        r = one / (one + np.exp(-(t * (np.log(v) - np.log(one - v)))))
    return np.minimum(np.maximum(r, dtype(LO)), dtype(HI))


def temper(noise, mode, tau_scale, tau_select, dtype=np.float64):
    """[rows, nps] noise of a head -> tempered, in `dtype` (float64: the reference; float32: the yardstick)"""
    noise = np.asarray(noise)
    out = np.empty(noise.shape, dtype=dtype)
    for q, kind in enumerate(kinds(mode, noise.shape[1])):
        out[:, q] = temper_kind(noise[:, q], kind, tau_select if kind == SELECT else tau_scale, dtype)
    return out


def gumbel(u):
    u = np.asarray(u, dtype=np.float64)
    return -np.log(-np.log(u))


def logit(u):
    u = np.asarray(u, dtype=np.float64)
    return np.log(u) - np.log(1.0 - u)


def floor_select(u_ref, ref):
    """s_g: what one float32 rounding of u' moves the Gumbel term by, plus two float32 roundings of the term itself"""
    return 2.0 ** -24 / (u_ref * -np.log(u_ref)) + 2.0 ** -23 * np.maximum(1.0, np.abs(ref))


def floor_logistic(u_ref, ref):
    return 2.0 ** -24 / (u_ref * (1.0 - u_ref)) + 2.0 ** -23 * np.maximum(1.0, np.abs(ref))


def worst_error(u, got, kind, tau):
    """worst normalised error of tempered entries `got` (float32) for inputs u (float32) of one kind at tau: |f(got) - clip(tau f(u))| / s with
    f the Gumbel term / the logit, the clip at f(LO), f(HI), and s the float32 floor at the float64 reference u'"""
    f, floor = (gumbel, floor_select) if kind == SELECT else (logit, floor_logistic)
    t = float(np.float32(tau))
    ref = np.clip(t * f(u), f(LO), f(HI))
    u_ref = temper_kind(u, kind, tau, np.float64)
    err = np.abs(f(np.asarray(got, dtype=np.float32)) - ref) / floor(u_ref, ref)
    return float(err.max())


def hardest_inputs(n=1 << 20, seed=20260101):
    """the clamped 24-bit uniforms of the device stream plus both ends of the clamp"""
    from hip_util import device_uniform_noise
    return np.concatenate([device_uniform_noise(n, seed), np.array([LO, HI], dtype=np.float32)])
