"""numpy mirror of folded synthesis (wn_fold_plan's rules, the fade tables, the unfold), shared by tests/test_fold_cpu.py and tests/test_hip_fold.py.
Rows are (utt, first, frames, keep, fade) tuples in mel frames, as _ext.fold_plan returns them."""
import numpy as np


def weights(kind, n):
    """float32 (w_in, w_out) of a fade of n samples, from float64: the header's formulas."""
    x = (np.arange(n, dtype=np.float64) + 0.5) / n
    if kind == 'equal_power':
        return np.sin(np.pi / 2 * x).astype(np.float32), np.cos(np.pi / 2 * x).astype(np.float32)
    return x.astype(np.float32), (1.0 - x).astype(np.float32)


def check_rules(frames, plan):
    """every rule of the planner section; raises AssertionError naming the row"""
    U = len(frames)
    assert [r[0] for r in plan] == sorted(r[0] for r in plan) and sorted({r[0] for r in plan}) == list(range(U)), plan
    for u in range(U):
        rows = [r for r in plan if r[0] == u]
        assert rows[0][1] == rows[0][3] == rows[0][4] == 0, (u, rows[0])
        assert rows[-1][1] + rows[-1][2] == frames[u], (u, rows[-1])
        for _, first, n, keep, fade in rows:
            assert n >= 1 and 0 <= first <= keep and fade >= 0 and keep + fade <= first + n <= frames[u], (u, first, n, keep, fade)
        for a, b in zip(rows, rows[1:]):
            assert b[3] + b[4] == a[1] + a[2], (u, a, b)
            assert b[3] >= a[3] + a[4], (u, a, b)


def coverage(frames, plan):
    """per utterance: how many rows contribute to every frame -- row j contributes from its keep to the end of the next row's fade (its own end)"""
    out = []
    for u, F in enumerate(frames):
        cnt = np.zeros(F, np.int64)
        for _, first, n, keep, fade in (r for r in plan if r[0] == u):
            assert first <= keep
            cnt[keep:first + n] += 1
        out.append(cnt)
    return out


def expected_coverage(frames, plan):
    out = []
    for u, F in enumerate(frames):
        cnt = np.ones(F, np.int64)
        for _, first, n, keep, fade in (r for r in plan if r[0] == u):
            cnt[keep:keep + fade] = 2
        out.append(cnt)
    return out


def unfold(frames, plan, hop, decoded, kind):
    """decoded: float32 [n_rows, >= n_max] decoded samples of every row -> list of float32 waveforms; a fade is fl(fl(a * w_out) + fl(b * w_in)) in float32"""
    out = []
    for u, F in enumerate(frames):
        idx = [i for i, r in enumerate(plan) if r[0] == u]
        wav = np.zeros(F * hop, np.float32)
        for k, i in enumerate(idx):
            _, first, n, keep, fade = plan[i]
            end = plan[idx[k + 1]][3] if k + 1 < len(idx) else first + n
            s0, s1, s2 = keep * hop, (keep + fade) * hop, end * hop
            wav[s1:s2] = decoded[i, s1 - first * hop:s2 - first * hop]
            if fade:
                p = idx[k - 1]
                a = decoded[p, s0 - plan[p][1] * hop:s1 - plan[p][1] * hop].astype(np.float32)
                b = decoded[i, s0 - first * hop:s1 - first * hop].astype(np.float32)
                w_in, w_out = weights(kind, fade * hop)
                wav[s0:s1] = (a * w_out).astype(np.float32) + (b * w_in).astype(np.float32)
        out.append(wav)
    return out
