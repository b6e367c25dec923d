"""float64 reference of the alignment check (csrc/wn_align.h) and the bounds its tests hold the float32 code to.

Stages, each applied to the PREVIOUS stage as the code under test produced it (so that every bound is launch-local):

  cepstra     c[k] = sum_m D[k][m] (unit x[m]) in float64 from the float32 table D and the float32 inputs.
              Bound.  u_dev = unit x (1 + d), |d| <= e = 2^-24.  A fused dot product of M terms rounds once per term; the standard running-error bound is
              |c_dev - sum D u_dev| <= g(M) sum |D||u_dev|, g(n) = n e / (1 - n e).  With (1 + g(M)) (1 + e) <= 1 + g(M + 1):
                  |c_dev - c_64| <= g(M + 1) sum_m |D[k][m]| |unit x[m]|      (+ the reference's own M 2^-52 of the same sum).
  cost        cost_64 = sqrt(0.5 sum_k (ca[k] - cb[k])^2) in float64 from the device's OWN float32 cepstra.
              Bound.  e_k = fl(ca - cb) = (ca - cb)(1 + d1); e_k^2 is exact inside the fma; n_cep fused adds of non-negative terms give
              s_dev = s (1 + t), |t| <= g(n_cep + 2); the halving is exact; the square root is correctly rounded:
                  |cost_dev - cost_64| <= (sqrt(1 + g(n_cep + 2)) (1 + e) - 1) cost_64 <= (g(n_cep + 2) / 2 + e (1 + g(n_cep + 2) / 2)) cost_64.
  recurrence  Dm_64 over the device's OWN float32 cost matrix, same band, same tie order.
              Bound.  All terms are non-negative, each cell adds one rounding and min preserves a common relative factor: if every candidate is within
              (1 + e)^n of its float64 value (n = i + j of the candidate + 1 <= i + j), so is their minimum against the float64 minimum, and one add gives
                  |Dm_dev(i, j) - Dm_64(i, j)| <= ((1 + e)^(i + j + 1) - 1) Dm_64(i, j)      for every admissible cell.
  path        NOT compared with float64's path on real inputs (near-ties are common; an undecidability excuse would hide faults).  It must equal, cell for
              cell, backtrace() applied to the device's OWN float32 Dm, and its cost T summed in float64 must satisfy
                  T <= ((1 + e) / (1 - e))^n_path Dm_64(Fa - 1, Fb - 1):
              along the device's path Dm_dev(p) = fl(cost(p) + Dm_dev(p - 1)) >= (cost(p) + Dm_dev(p - 1)) (1 - e), so T <= Dm_dev(end) / (1 - e)^n_path; and
              Dm_dev(end) is not above the rounded sum along any one path (min and rounding are monotone), in particular along a float64-optimal one, whose
              rounded sum is within (1 + e)^(its length) of Dm_64(end).  (Where that path is longer than the device's, the numerator's exponent of this
              derivation is that length, at most Fa + Fb - 1; the test keeps the tighter n_path.)
Underflow is excluded throughout (the tests' inputs are of ordinary size)."""
import numpy as np

EPS = 2.0 ** -24
NONE = 3


def gamma(n):
    return n * EPS / (1.0 - n * EPS)


def dct_table(M, n_cep):
    """rows k = 1 ... n_cep of the orthonormal DCT-II, in double, rounded to float32: [n_cep, M]"""
    k = np.arange(1, n_cep + 1, dtype=np.float64)[:, None]
    m = np.arange(M, dtype=np.float64)[None, :]
    return (np.sqrt(2.0 / M) * np.cos(np.pi * k * (m + 0.5) / M)).astype(np.float32)


def cepstra(x, unit_db, n_cep):
    """x float32 [F, M] -> (c float64 [F, n_cep], bound float64 [F, n_cep])"""
    x = np.asarray(x, np.float32)
    M = x.shape[1]
    D = dct_table(M, n_cep).astype(np.float64)
    u = np.float64(np.float32(unit_db)) * x.astype(np.float64)
    c = u @ D.T
    mag = np.abs(u) @ np.abs(D).T
    return c, (gamma(M + 1) + M * 2.0 ** -52) * mag


def cost_matrix(ca, cb):
    """ca [Fa, K], cb [Fb, K] (float32 as the code under test produced them) -> (cost float64 [Fa, Fb], relative bound)"""
    ca, cb = np.asarray(ca, np.float64), np.asarray(cb, np.float64)
    K = ca.shape[1]
    e = ca[:, None, :] - cb[None, :, :]
    g = gamma(K + 2)
    return np.sqrt(0.5 * np.sum(e * e, axis=2)), 0.5 * g + EPS * (1.0 + 0.5 * g) + 4 * 2.0 ** -52


def admissible(i, j, Fa, Fb, band):
    return band == 0 or abs(i * Fb - j * Fa) <= band * max(Fa, Fb)


def _choose(i, j, Fa, Fb, band, get):
    """predecessor of (i, j) by the rule: smallest candidate, ties to the first of diagonal, up, left; candidates outside the matrix or band never.
    Returns (direction, value)."""
    best, w = np.inf, NONE
    if i > 0 and j > 0 and admissible(i - 1, j - 1, Fa, Fb, band):
        best, w = get(i - 1, j - 1), 0
    if i > 0 and admissible(i - 1, j, Fa, Fb, band):
        v = get(i - 1, j)
        if w == NONE or v < best:
            best, w = v, 1
    if j > 0 and admissible(i, j - 1, Fa, Fb, band):
        v = get(i, j - 1)
        if w == NONE or v < best:
            best, w = v, 2
    return w, best


def recurrence(cost, band=0, dtype=np.float64):
    """cost [Fa, Fb] -> Dm [Fa, Fb] of `dtype` (every add rounded to it); inadmissible or unreachable cells +inf"""
    cost = np.asarray(cost)
    Fa, Fb = cost.shape
    dm = np.full((Fa, Fb), np.inf, dtype)
    c = cost.astype(dtype)
    for i in range(Fa):
        for j in range(Fb):
            if not admissible(i, j, Fa, Fb, band):
                continue
            if i == 0 and j == 0:
                dm[0, 0] = c[0, 0]
                continue
            w, best = _choose(i, j, Fa, Fb, band, lambda p, q: dm[p, q])
            if w != NONE:
                dm[i, j] = dtype(c[i, j] + best)
    return dm


def recurrence_bound(dm64):
    """((1 + e)^(i + j + 1) - 1) Dm_64(i, j); inf where Dm_64 is"""
    Fa, Fb = dm64.shape
    n = np.arange(Fa)[:, None] + np.arange(Fb)[None, :] + 1
    with np.errstate(invalid='ignore'):
        return np.expm1(n * np.log1p(EPS)) * dm64


def backtrace(dm, band=0):
    """the path the rule gives on a matrix Dm (any dtype), FORWARD order: int array [n, 2].  Bounded and clamped like the code under test."""
    Fa, Fb = dm.shape
    i, j = Fa - 1, Fb - 1
    rev = []
    for _ in range(Fa + Fb - 2):
        if i == 0 and j == 0:
            break
        rev.append((i, j))
        w, _ = _choose(i, j, Fa, Fb, band, lambda p, q: dm[p, q])
        if i == 0:
            w = 2
        elif j == 0:
            w = 1
        elif w == NONE:
            w = 0
        if w != 2:
            i -= 1
        if w != 1:
            j -= 1
    rev.append((0, 0))
    return np.array(rev[::-1], np.int64)


def maps(path, Fa, Fb):
    mab, mba = np.full(Fa, -1, np.int64), np.full(Fb, -1, np.int64)
    for i, j in path:
        mab[i] = max(mab[i], j)
        mba[j] = max(mba[j], i)
    return mab, mba


def summary(path, cost, total):
    """the 7 columns in float64 (the code under test rounds each to float32 once)"""
    Fa, Fb = cost.shape
    n = len(path)
    s = 0.0
    for i, j in path:
        s += float(cost[i, j])
    steps = np.diff(path, axis=0)
    nondiag = int(np.sum((steps[:, 0] == 0) | (steps[:, 1] == 0))) if n > 1 else 0
    dev = int(np.max(np.abs(path[:, 0] * Fb - path[:, 1] * Fa)))
    return np.array([Fa, Fb, n, total, s / n, nondiag / (n - 1) if n > 1 else 0.0, dev / max(Fa, Fb)], np.float64)


def path_cost(path, cost):
    return float(np.sum(np.asarray(cost, np.float64)[path[:, 0], path[:, 1]]))


def near_optimal(path, cost, dm64_end):
    """(T, limit) of T <= ((1 + e) / (1 - e))^n_path Dm_64(Fa-1, Fb-1): near-optimality of the path the code under test delivered (module docstring)"""
    n = len(path)
    return path_cost(path, cost), ((1.0 + EPS) / (1.0 - EPS)) ** n * float(dm64_end)


def brute_force(cost, band=0):
    """min over all monotone paths of their float64 cost, by plain recursion (tiny sizes only)"""
    cost = np.asarray(cost, np.float64)
    Fa, Fb = cost.shape

    def go(i, j):
        if not admissible(i, j, Fa, Fb, band):
            return np.inf
        if i == 0 and j == 0:
            return cost[0, 0]
        best = np.inf
        if i > 0 and j > 0:
            best = min(best, go(i - 1, j - 1))
        if i > 0:
            best = min(best, go(i - 1, j))
        if j > 0:
            best = min(best, go(i, j - 1))
        return cost[i, j] + best
    return go(Fa - 1, Fb - 1)


def is_valid_path(path, Fa, Fb):
    path = np.asarray(path)
    if len(path) < 1 or tuple(path[0]) != (0, 0) or tuple(path[-1]) != (Fa - 1, Fb - 1):
        return False
    st = np.diff(path, axis=0)
    return bool(np.all((st >= 0) & (st <= 1)) and np.all(st.sum(axis=1) >= 1))
