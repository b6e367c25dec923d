"""What the streaming-denoiser tests share (tests/test_denoise_stream_cpu.py, tests/test_hip_denoise_stream.py): the emit rule stated by brute force, the
cuttings of a ragged batch into pushes, and a numpy statement of the state machine (counters, input tail, frame store, emit rule) in float64 that takes a
`fault` to seed one of five mistakes.  The signals, the profile and the float64 parity rule are those of tests/denoise_ref.py."""
import numpy as np

import denoise_ref as R

CUTTINGS = ('one', 'hop-1', 'hop', 'hop+1', '32hop', '32hop+1', 'zero_mid', 'all_final', 'ragged', 'final_empty')
FAULTS = ('tail_one_sample_short', 'frame_emitted_before_complete', 'edge_frames_left_out_of_window_sum_at_final', 'restart_keeps_the_ring', 'final_does_not_zero_pad')


def ready_brute(n_fft, hop, S, final):
    """samples emitted of a row given S: sample i goes out iff every frame <= min((i + H) // hop, F - 1) is complete -- its window lies within the S samples
    (f hop + H <= S), or the row is final (F = 1 + S // hop frames, zero-padded)."""
    H = n_fft // 2
    if final:
        return S
    e = 0
    while e < S and all(f * hop + H <= S for f in range((e + H) // hop + 1)):
        e += 1
    return e


def schedule(lens, kind, n_fft, hop, seed=5):
    """A ragged batch cut into pushes: a list of (n [B], final [B]); row b's pushes sum to lens[b] and its last one carries final (rows end at different
    pushes; a row of length 0 ends with an empty final push at once)."""
    B = len(lens)
    rs = np.random.RandomState(seed)
    left = [int(v) for v in lens]
    ended = [False] * B
    chunk = {'one': 1, 'hop-1': max(hop - 1, 1), 'hop': hop, 'hop+1': hop + 1, '32hop': 32 * hop, '32hop+1': 32 * hop + 1, 'zero_mid': hop + 1, 'final_empty': hop}
    out, k = [], 0
    while not all(ended):
        n, fin = [0] * B, [0] * B
        if kind == 'zero_mid' and k == 2:
            out.append((n, fin))      # a push that gives nobody anything
            k += 1
            continue
        for b in range(B):
            if ended[b]:
                continue
            if kind == 'all_final':
                c = left[b]
            elif kind == 'ragged':
                c = int(rs.randint(0, 3 * hop + 2))
            else:
                c = kind if isinstance(kind, int) else chunk[kind]      # (an int: pushes of that many samples)
            c = min(c, left[b])
            if kind == 'final_empty' and left[b] == 0:
                fin[b] = 1      # the end arrives as a push of its own, with no samples
            elif kind != 'final_empty' and c == left[b]:
                fin[b] = 1
            n[b] = c
            left[b] -= c
            ended[b] = bool(fin[b])
        out.append((n, fin))
        k += 1
    return out


def blocks(wav, sched):
    """the pushes of `sched` as (block [B, pitch], n, restart, final): row b's next n[b] samples at the row's start, NaN (float) or -7 (int) beyond; the first
    push restarts every row"""
    B = wav.shape[0]
    pos = [0] * B
    res = []
    for k, (n, fin) in enumerate(sched):
        blk = np.full((B, max(max(n), 1) + 2), np.nan if wav.dtype == np.float32 else -7, wav.dtype)
        for b in range(B):
            blk[b, :n[b]] = wav[b, pos[b]:pos[b] + n[b]]
            pos[b] += n[b]
        res.append((blk, list(n), [int(k == 0)] * B, list(fin)))
    return res


def gather(results, B):
    """the per-push (out, n_out) of a run -> one array per row; asserts nothing"""
    return [np.concatenate([o[b, :m[b]] for o, m in results] or [np.zeros(0, np.float32)]) for b in range(B)]


class NumpyStream:
    """One row of the state machine in float64 numpy: S, E, the tail [E, S), the windowed frames kept by index.  fault: one of FAULTS."""

    def __init__(self, n_fft, hop, profile, strength, fault=None):
        assert fault is None or fault in FAULTS
        self.N, self.hop, self.H = n_fft, hop, n_fft // 2
        self.t = float(strength) * np.asarray(profile, np.float64)
        self.w = R.window(n_fft)
        self.fault = fault
        self.frames = {}
        self.restart()

    def restart(self):
        self.S = self.E = self.fd = 0
        self.tail = np.zeros(0)
        if self.fault != 'restart_keeps_the_ring':
            self.frames = {}

    def _frame(self, span, base, f, S):
        x = np.zeros(self.N)
        lo = f * self.hop - self.H
        for j in range(self.N):
            s = lo + j
            if 0 <= s < S and 0 <= s - base < len(span):
                x[j] = span[s - base]
        Y = R.shrink(np.fft.rfft(x * self.w)[None, :], self.t[None, :])[0]
        return np.fft.irfft(Y, self.N) * self.w

    def push(self, x, final=False):
        N, hop, H = self.N, self.hop, self.H
        span = np.concatenate([self.tail, np.asarray(x, np.float64)])
        base, S1 = self.E, self.S + len(x)
        early = hop if self.fault == 'frame_emitted_before_complete' else 0
        fd1 = (S1 + early - H) // hop + 1 if S1 + early >= H else 0
        E1 = min(S1, max(0, fd1 * hop - H))
        if final:
            E1 = S1
            if self.fault != 'final_does_not_zero_pad':
                fd1 = 1 + S1 // hop if S1 > 0 else 0
        fd1 = max(fd1, self.fd)
        for f in range(self.fd, fd1):
            if f not in self.frames:      # (a frame store that was not cleared at restart still holds the previous utterance's)
                self.frames[f] = self._frame(span, base, f, S1)
        out = np.zeros(E1 - self.E)
        F = fd1
        for i in range(self.E, E1):
            num = den = 0.0
            for f in range((i - H) // hop + 1 if i >= H else 0, min((i + H) // hop, F - 1) + 1):
                j = i - f * hop + H
                num += self.frames[f][j]
                if not (final and self.fault == 'edge_frames_left_out_of_window_sum_at_final' and f in (0, F - 1)):
                    den += self.w[j] ** 2
            with np.errstate(divide='ignore', invalid='ignore'):
                out[i - self.E] = np.float64(num) / np.float64(den)
        keep = E1 - self.E + (1 if self.fault == 'tail_one_sample_short' else 0)
        self.tail = span[keep:]
        if self.fault == 'tail_one_sample_short' and E1 < S1:
            self.tail = np.concatenate([[0.0], self.tail])[:S1 - E1]      # the oldest carried sample is lost (nothing is indexed out of range)
        if self.fault != 'restart_keeps_the_ring':
            for f in [f for f in self.frames if f * hop + H <= E1]:      # every sample the frame covers is out
                del self.frames[f]
        self.S, self.E, self.fd = S1, E1, fd1
        return out
