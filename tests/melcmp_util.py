"""Reconstruction check: the numpy side of the tests.

reference(..., dtype=np.float64) evaluates the formulas of include/wavenet_mi355.h (the wn_melcmp section) in float64, in numpy's own order: no attempt to
copy the device's.  The same function at dtype=np.float32 is the YARDSTICK: what plain numpy float32 makes of the same formulas.  bounds() derives, from the
float64 values alone, how far a float32 evaluation in ANY order may be from them.

Derivation (u = 2^-24, the float32 unit roundoff; a sum of n float32 terms in any order is within (n - 1) u sum |x_i| of the exact sum of the same terms):
  d        = fl(unit fl(a - b)): two roundings, |d32 - d| <= 2 u |d|.
  bias     M terms with 2 u each, M - 1 additions, one division:                         (M + 2) u mean_m |d|
  l1       the same on |d|:                                                              (M + 2) u mean_m |d|
  lsd^2    d^2 carries 2 x 2 u + the product's u, M - 1 additions, the division, and the square root's u twice on the square:
                                                                                         (M + 7) u mean_m d^2
  mcd^2    c_k = sum_m D[k][m] d[m]: M roundings of the accumulation, 2 u of d, u of the float32 table: |c32 - c| <= (M + 3) u A_k with
           A_k = sum_m |D[k][m]| |d[m]| >= |c_k|; c^2 moves by at most 2 A_k that much plus the square's u; at most n_cep - 1 additions (+ 3 for
           the four partial sums), the exact 0.5, the square root's 2 u:                  (2 M + n_cep + 11) u 0.5 sum_k A_k^2
  bias_b   the mean of F per-frame values adds the reduction's own term: a lane's serial sum of ceil(F / 256) terms, 8 tree levels, one division:
           E_b = mean_f bound(bias_f) + (ceil(F / 256) + 9) u mean_f |bias_f|
  l1c      e = d - bias_b: |e32 - e| <= de = 2 u |d| + E_b + u |e|; M - 1 additions and the division:
                                                                                         mean_m de + (M + 1) u mean_m |e|
  lsdc^2   e^2 moves by 2 |e| de + de^2 + u e^2; additions, division, square root:       mean_m (2 |e| de + de^2) + (M + 3) u mean_m e^2
  means    over F frames of a per-frame value v: mean_f bound(v_f) + (ceil(F / 256) + 9) u mean_f |v_f|.  For lsd, mcd and lsdc the per-frame bound is
           on the square (the square root of a cancelling sum has no useful relative bound); for x, y >= 0, |x - y| <= min(sqrt |x^2 - y^2|,
           |x^2 - y^2| / y), which turns it into one on the value for the mean.
  worst    a maximum moves by at most the largest bound of its candidates.
Every bound is multiplied by SLACK = 1.01 for the second-order terms left out above.

Against the yardstick: per result kind, over all rows of a case, the worst error of the evaluation under test is at most FACTOR = 8 x the worst error
of the numpy float32 evaluation (the factor tests/mel_util.py allows a float32 sum taken in another order), the yardstick floored at one unit
roundoff of the largest reference value of that kind: a yardstick that happens to be exact -- one channel, one frame -- says nothing."""
import numpy as np

U = 2.0 ** -24
SLACK = 1.01
FACTOR = 8.0
KINDS = ('bias', 'l1', 'lsd', 'mcd', 'l1c', 'lsdc')
SQUARED = (2, 3, 5)                 # per-frame kinds whose bound is stated on the square


def dct_table(M, n_cep, dtype=np.float64):
    """rows k = 1 ... n_cep of the orthonormal DCT-II"""
    k = np.arange(1, n_cep + 1, dtype=np.float64)[:, None]
    m = np.arange(M, dtype=np.float64)[None, :]
    return (np.sqrt(2.0 / M) * np.cos(np.pi * k * (m + 0.5) / M)).astype(dtype)


def reference(a, b, frames, n_cep, unit_db, alarm_db, dtype=np.float64):
    """a, b [B, M, pitch] (channels first).  Returns a list over rows of dicts: per_frame [6, F], summary [7], marks (worst frame, alarmed frames)."""
    out = []
    M = a.shape[1]
    D = dct_table(M, n_cep, dtype)
    unit = dtype(np.float32(unit_db))
    for r, F in enumerate(frames):
        F = int(F)
        d = unit * (a[r, :, :F].astype(dtype) - b[r, :, :F].astype(dtype))      # [M, F]
        pf = np.zeros((6, F), dtype)
        if F:
            pf[0] = d.mean(axis=0, dtype=dtype)
            pf[1] = np.abs(d).mean(axis=0, dtype=dtype)
            pf[2] = np.sqrt((d * d).mean(axis=0, dtype=dtype))
            if n_cep:
                c = D @ d
                pf[3] = np.sqrt(dtype(0.5) * (c * c).sum(axis=0, dtype=dtype))
            e = d - pf[0].mean(dtype=dtype)
            pf[4] = np.abs(e).mean(axis=0, dtype=dtype)
            pf[5] = np.sqrt((e * e).mean(axis=0, dtype=dtype))
        sm = np.zeros(7, dtype)
        if F:
            sm[:6] = pf.mean(axis=1, dtype=dtype)
            sm[6] = pf[4].max()
        marks = (int(np.argmax(pf[4])) if F else -1, int(np.sum(pf[4] > dtype(np.float32(alarm_db)))))
        out.append(dict(per_frame=pf, summary=sm, marks=marks))
    return out


def _value_bound(bsq, v):
    """a bound on |x - v| from one on |x^2 - v^2|, x, v >= 0"""
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.minimum(np.sqrt(bsq), np.where(v > 0, bsq / v, np.inf))


def bounds(a, b, frames, n_cep, unit_db):
    """per row: per_frame [6, F] (kinds 2, 3, 5 on the SQUARE of the value) and summary [7], from the float64 values alone"""
    out = []
    M = a.shape[1]
    D = np.abs(dct_table(M, n_cep))
    unit = np.float64(np.float32(unit_db))
    ref = reference(a, b, frames, n_cep, unit_db, 0.0)
    for r, F in enumerate(frames):
        F = int(F)
        d = unit * (a[r, :, :F].astype(np.float64) - b[r, :, :F].astype(np.float64))
        ad = np.abs(d)
        pf, sm = np.zeros((6, F)), np.zeros(7)
        if F:
            v = ref[r]['per_frame']
            red = (np.ceil(F / 256.0) + 9) * U
            pf[0] = (M + 2) * U * ad.mean(axis=0)
            pf[1] = (M + 2) * U * ad.mean(axis=0)
            pf[2] = (M + 7) * U * (d * d).mean(axis=0)
            if n_cep:
                A = D @ ad
                pf[3] = (2 * M + n_cep + 11) * U * 0.5 * (A * A).sum(axis=0)
            E_b = pf[0].mean() + red * np.abs(v[0]).mean()
            e = np.abs(d - v[0].mean())
            de = 2 * U * ad + E_b + U * e
            pf[4] = de.mean(axis=0) + (M + 1) * U * e.mean(axis=0)
            pf[5] = (2 * e * de + de * de).mean(axis=0) + (M + 3) * U * (e * e).mean(axis=0)
            pf *= SLACK
            for j in range(6):
                bv = _value_bound(pf[j], v[j]) if j in SQUARED else pf[j]
                sm[j] = bv.mean() + SLACK * red * np.abs(v[j]).mean()
            sm[6] = pf[4].max()
        out.append(dict(per_frame=pf, summary=sm))
    return out


def errors(got_pf, got_sm, ref, bnd):
    """one row: (err, bound) arrays per result kind, the per-frame kinds 2, 3, 5 compared on their squares.  got_pf [6, >= F], got_sm [7]."""
    F = ref['per_frame'].shape[1]
    g = np.asarray(got_pf, np.float64)[:, :F]
    res = {}
    for j, k in enumerate(KINDS):
        if j in SQUARED:
            res[k] = (np.abs(g[j] ** 2 - ref['per_frame'][j] ** 2), bnd['per_frame'][j])
        else:
            res[k] = (np.abs(g[j] - ref['per_frame'][j]), bnd['per_frame'][j])
    for j, k in enumerate(KINDS + ('worst',)):
        res['mean_' + k if j < 6 else k] = (np.abs(np.float64(got_sm[j]) - ref['summary'][j])[None], bnd['summary'][j][None])
    return res


def check_row(got_pf, got_sm, got_marks, ref, bnd, alarm_db, where=''):
    """every element of one row inside its bound; the worst frame and the alarm count up to what the bound leaves open.  Returns {kind: worst err / bound}."""
    ratios = {}
    for k, (err, bd) in errors(got_pf, got_sm, ref, bnd).items():
        assert np.all(np.isfinite(err)), (where, k)
        assert np.all(err <= bd), (where, k, float(err.max()), float(bd[np.argmax(err - bd)]))
        with np.errstate(divide='ignore', invalid='ignore'):
            q = np.where(bd > 0, err / bd, 0.0)
        ratios[k] = float(q.max()) if q.size else 0.0
    l1c, bl = ref['per_frame'][4], bnd['per_frame'][4]
    F = l1c.size
    at, count = int(got_marks[0]), int(got_marks[1])
    if F == 0:
        assert (at, count) == (-1, 0), where
    else:
        assert 0 <= at < F and l1c[at] >= l1c.max() - 2 * bl.max(), (where, at)
        alarm = np.float64(np.float32(alarm_db))
        assert int(np.sum(l1c > alarm + bl)) <= count <= int(np.sum(l1c >= alarm - bl)), (where, count)
    return ratios


def mels(B, M, pitch, seed, lo=-4.0, hi=4.0, saturate=True):
    """seeded mels in the normalised range [lo, hi], channels first, with some channels saturated at both ends"""
    rng = np.random.RandomState(seed)
    x = rng.uniform(lo, hi, size=(B, M, pitch)).astype(np.float32)
    if saturate and M >= 3:
        x[:, 0] = lo
        x[:, M - 1] = hi
        x[:, M // 2, ::3] = lo
    return x


def layout(x, channels_first, pitch=None, fill=np.nan):
    """[B, M, P] -> the requested layout at a pitch >= P, the padding filled (NaN: poison)"""
    B, M, P = x.shape
    pitch = P if pitch is None else pitch
    y = np.full((B, M, pitch), fill, np.float32)
    y[:, :, :P] = x
    return np.ascontiguousarray(y if channels_first else y.transpose(0, 2, 1))


def poison(x, frames):
    """NaN beyond every row's frames ([B, M, P] channels first)"""
    y = x.copy()
    for r, F in enumerate(frames):
        y[r, :, int(F):] = np.nan
    return y


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def check_against_yardstick(got, yard, ref, bnd, where=''):
    """got / yard: per row (per_frame [6, >= F], summary [7]) of the evaluation under test and of the numpy float32 one; ref, bnd: reference() and bounds().
    Asserts, per result kind over all rows, worst error <= FACTOR x max(worst yardstick error, U x the largest reference value).  Returns
    {kind: (worst error, worst yardstick error, floor)}."""
    acc = {}
    for r in range(len(ref)):
        eg, ey = errors(got[r][0], got[r][1], ref[r], bnd[r]), errors(yard[r][0], yard[r][1], ref[r], bnd[r])
        F = ref[r]['per_frame'].shape[1]
        for j, k in enumerate(KINDS + ('worst',)):
            vals = {k: np.abs(ref[r]['per_frame'][j]) ** (2 if j in SQUARED else 1)} if j < 6 else {}
            vals['mean_' + k if j < 6 else k] = np.abs(ref[r]['summary'][j])[None]
            for name, v in vals.items():
                g, y, sc = acc.get(name, (0.0, 0.0, 0.0))
                if F:
                    acc[name] = (max(g, float(eg[name][0].max())), max(y, float(ey[name][0].max())), max(sc, float(v.max())))
                else:
                    acc[name] = (g, y, sc)
    out = {}
    for name, (g, y, sc) in acc.items():
        floor = U * sc
        assert g <= FACTOR * max(y, floor), (where, name, g, y, floor)
        out[name] = (g, y, floor)
    return out
