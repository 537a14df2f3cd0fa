"""NumPy restatement of csg_farthest_points, written from the text of
include/csg_api.h (not from the kernel), and the synthetic point sets the tests
share.  Every float operation is float32 and rounds once: NumPy's float32
arrays do exactly that.
"""
from __future__ import annotations

import numpy as np

EMPTY = 0xFFFFFFFF
NAN_BITS = 0x7FC00000
F32 = np.float32


def fmix32(x: int) -> int:
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def set_rows(count, rows: int) -> int:
    """m_s."""
    if count is None:
        return rows
    count = int(count)
    return 0 if count == EMPTY else min(count, rows)


def candidate_rows(m: int, pool: int) -> np.ndarray:
    c = min(m, pool)
    return np.array([(j * m) // c for j in range(c)], np.int64)   # Python integers: no width to overflow


def start_candidate(valid: np.ndarray, seed: int, key: int) -> int:
    c = valid.shape[0]
    h = fmix32(fmix32((seed ^ key) & 0xFFFFFFFF) ^ 0x9E3779B9)
    j0 = (h * c) >> 32
    vj = np.flatnonzero(valid).astype(np.int64)
    cyc = (vj + c - j0) % c               # distinct values: one minimum
    return int(vj[np.argmin(cyc)])


def dist2(p: np.ndarray, a: np.ndarray) -> np.ndarray:
    """d2 of every row of p (n, 3) float32 to the point a (3,) float32."""
    with np.errstate(over="ignore", invalid="ignore"):
        d = p - a[None, :]                      # fl32(ax - bx)
        q = d * d                               # fl32(dx * dx)
        return (q[:, 0] + q[:, 1]) + q[:, 2]    # fl32(fl32(.. + ..) + ..)


def run_set(pts: np.ndarray, m: int, pool: int, samples: int, seed: int, key: int):
    """One set: (index (K,) uint32, t0, v, dist2 (K,) float32).  pts is (C, 3) float32."""
    K = samples
    index = np.full(K, EMPTY, np.uint32)
    d2 = np.zeros(K, F32)
    rows = candidate_rows(m, pool)
    cand = pts[rows] if rows.size else np.zeros((0, 3), F32)
    valid = np.isfinite(cand).all(axis=1)
    v = int(valid.sum())
    if v == 0:
        return index, 0, 0, d2
    vj = np.flatnonzero(valid)            # ascending: the first maximum below is the lowest j
    p = np.ascontiguousarray(cand[vj])
    mind = np.full(v, np.inf, F32)
    a = int(np.searchsorted(vj, start_candidate(valid, seed, key)))
    chosen = [a]
    d2[0] = np.inf
    t0 = K
    for t in range(1, K + 1):
        mind = np.minimum(mind, dist2(p, p[a]))
        if t == K:
            break
        g = mind.max()
        if g == 0:
            t0 = t
            break
        a = int(np.argmax(mind == g))
        chosen.append(a)
        d2[t] = g
    chosen = rows[vj[np.array(chosen)]]
    for t in range(K):
        index[t] = chosen[t % t0]
    return index, t0, v, d2


def farthest_points_ref(xyz, counts=None, *, samples, pool=16384, seed=0, set_keys=None, payloads=(), fills=None):
    """The whole pass on host arrays: xyz (S, C, 3) float32; payloads arrays
    (S, C, ...).  Returns a dict like Renderer.farthest_points_host."""
    xyz = np.ascontiguousarray(xyz, F32)
    S, C = xyz.shape[:2]
    K = int(samples)
    out = {"index": np.empty((S, K), np.uint32), "xyz": np.empty((S, K, 3), F32), "dist2": np.empty((S, K), F32),
           "count": np.empty((S, 2), np.uint32), "payloads": []}
    for s in range(S):
        m = set_rows(None if counts is None else counts[s], C)
        key = s if set_keys is None else int(set_keys[s])
        idx, t0, v, d2 = run_set(xyz[s], m, int(pool), K, int(seed), key)
        out["index"][s], out["dist2"][s], out["count"][s] = idx, d2, (t0, v)
        if v:
            out["xyz"][s].view(np.uint32)[...] = xyz[s][idx].view(np.uint32)
        else:
            out["xyz"][s].view(np.uint32)[...] = NAN_BITS
    for i, pl in enumerate(payloads):
        pl = np.ascontiguousarray(pl)
        g = np.empty((S, K) + pl.shape[2:], pl.dtype)
        for s in range(S):
            if out["count"][s, 1]:
                g[s] = pl[s][out["index"][s]]
            else:
                g[s].reshape(-1).view(np.uint8)[...] = 0 if fills is None else fills[i]
        out["payloads"].append(g)
    return out


# ---- the shared synthetic sets ------------------------------------------------------------------------

def lattice(n: int = 8) -> np.ndarray:
    """The n x n unit lattice in the plane z = 0, row-major: exact ties everywhere."""
    y, x = np.mgrid[0:n, 0:n]
    return np.stack([x, y, np.zeros_like(x)], -1).reshape(-1, 3).astype(F32)


def cloud(rng: np.random.Generator, n: int, scale: float = 1.0) -> np.ndarray:
    """n points of a lumpy cloud: a box plus a dense cluster, as an object seen from near."""
    p = rng.uniform(-1.0, 1.0, (n, 3)).astype(F32)
    k = n // 3
    p[:k] = (p[:k] * F32(0.05) + F32(0.7)).astype(F32)
    return (p * F32(scale)).astype(F32)


def spoil(rng: np.random.Generator, p: np.ndarray, share: float = 0.1) -> np.ndarray:
    """Rows with NaN, +inf and -inf, each in each coordinate."""
    p = p.copy()
    bad = np.flatnonzero(rng.random(p.shape[0]) < share)
    vals = np.array([np.nan, np.inf, -np.inf], F32)
    for i, r in enumerate(bad):
        p[r, i % 3] = vals[(i // 3) % 3]
    return p


def brute_cover(cand: np.ndarray, chosen: np.ndarray) -> float:
    """max over the valid candidates of the min over the samples of d2, float32, by a plain double loop
    over the samples (independent of run_set's bookkeeping)."""
    valid = np.isfinite(cand).all(axis=1)
    p = cand[valid]
    best = np.full(p.shape[0], np.inf, F32)
    for a in chosen:
        best = np.minimum(best, dist2(p, a))
    return float(best.max()) if p.shape[0] else 0.0
