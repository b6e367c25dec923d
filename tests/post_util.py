"""The output stage (csrc/wn_post.hip) restated on numpy, operation for operation, and its float64 reference.

Mirror (float32, what the device and the host hook must equal bit for bit):
  decode   in_type 0: the float itself; 1: sign(v) (1 / 255) (256^|v| - 1) in float64, rounded to float32 once (oracle/mulaw.py on float64 input: the
           arithmetic of wn_inv_mulaw); 2: the 256-entry float32 table of the reference's numpy path (tests/golden/mulaw_golden.npz inv_q_all, what
           wn_inv_mulaw_quantize looks up), ids clamped to 0 ... 255
  chain    y[t] = fl32(fl32(k y[t-1]) + x[t]) in sample order from y[-1] = carry; k = 0 does no arithmetic
  PCM      v = fl32(y s), clamped to [-32767, 32767], truncated toward zero; clipped = #(|v| > 32767); s = fl32(gain 32767) for a push,
           fl32(32767 / max(0.01, peak)) for a finish -- save_wavenet_wav's own expression
Reference (float64): scipy.signal.lfilter([1], [1, -float(np.float32(k))], x64)."""
import os

import numpy as np
from scipy import signal

from oracle import mulaw as M

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mulaw_golden.npz')
DECODE_TABLE = np.load(_GOLDEN)['inv_q_all'].astype(np.float32)
TINY = np.float32(2.0 ** -126)
IN_DTYPE = {0: np.float32, 1: np.float32, 2: np.int32}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def decode(in_type, a):
    if in_type == 2:
        return DECODE_TABLE[np.clip(np.asarray(a, dtype=np.int64), 0, 255)]
    a = np.asarray(a, dtype=np.float32)
    if in_type == 0:
        return a.copy()
    return M.inv_mulaw(a.astype(np.float64)).astype(np.float32)


def chain(x, k, carry=0.0):
    """-> (y float32 [n], carry_out float32)"""
    x = np.asarray(x, dtype=np.float32)
    k, y = np.float32(k), np.float32(carry)
    if x.size == 0:
        return x.copy(), y
    if k == 0:
        return x.copy(), x[-1]
    out = np.empty_like(x)
    for t in range(x.size):
        y = np.float32(np.float32(k * y) + x[t])
        out[t] = y
    return out, y


def push_scale(gain):
    return np.float32(float(np.float32(gain)) * 32767.0)


def peak_scale(peak):
    return np.float32(32767.0 / max(0.01, float(peak)))


def pcm(y, s):
    """-> (int16 [n], clipped)"""
    v = np.asarray(y, dtype=np.float32) * np.float32(s)
    assert v.dtype == np.float32
    return np.clip(v, np.float32(-32767), np.float32(32767)).astype(np.int16), int(np.sum(np.abs(v) > np.float32(32767)))


def save_wavenet_wav_pcm(wav):
    """datasets.audio.save_wavenet_wav's arithmetic (audio.py:17-20 of the reference), without the file"""
    wav = np.asarray(wav, dtype=np.float32)
    out = wav * (32767 / max(0.01, float(np.max(np.abs(wav))) if wav.size else 0.01))
    return out.astype(np.int16)


def mirror_push(in_type, a, k, carry=0.0, gain=1.0):
    """one row of one push -> (y, int16, clipped, carry_out)"""
    y, c = chain(decode(in_type, a), k, carry)
    q, nclip = pcm(y, push_scale(gain))
    return y, q, nclip, c


def mirror_finish(in_type, a, k):
    """one whole row -> (y, int16, peak)"""
    y, _ = chain(decode(in_type, a), k, 0.0)
    peak = np.float32(np.max(np.abs(y))) if y.size else np.float32(0)
    return y, pcm(y, peak_scale(peak))[0], peak


def lfilter64(x, k):
    return signal.lfilter([1.0], [1.0, -float(np.float32(k))], np.asarray(x, dtype=np.float64))


def samples(in_type, n, seed):
    """model-domain test input of one row: floats in (-1, 1) / class ids with a few outside 0 ... 255 (the decode clamps them)"""
    rng = np.random.RandomState(seed)
    if in_type == 2:
        q = rng.randint(0, 256, size=n).astype(np.int32)
        if n > 8:
            q[3], q[n - 2] = -5, 300
        return q
    return rng.uniform(-0.99, 0.99, size=n).astype(np.float32)


def speech_like(n, seed, k=0.97, peak=0.9):
    """pre-emphasised integrated noise scaled to `peak`: what the model is trained to generate (a low-pass signal through lfilter([1, -k], [1]))"""
    rng = np.random.RandomState(seed)
    low = signal.lfilter([1.0], [1.0, -0.995], rng.randn(n))
    pre = signal.lfilter([1.0, -k], [1.0], low)
    return (pre * (peak / np.max(np.abs(pre)))).astype(np.float32)
