"""Farthest-point sampling of point sets (csg_farthest_points):
the host-side arithmetic around :meth:`renderer.Renderer.farthest_points` --
which rows of a set are candidates, what a run covers, and how a loader takes
a shorter run out of a stored one.  The definition is the text of
``include/csg_api.h``; nothing here touches the GPU.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

MAX_POOL = 16384      # candidates of a set at most (one workgroup holds them in registers)
MAX_SAMPLES = 16384   # samples of a set at most
MAX_PAYLOADS = 4
MAX_ROW_BYTES = 64
EMPTY_INDEX = 0xFFFFFFFF   # fp_index of an empty set


def candidate_rows(m: int, pool: int = MAX_POOL) -> np.ndarray:
    """The rows of a set of ``m`` rows that are its candidates under ``pool``:
    ``r_j = (j * m) // c`` for ``j < c = min(m, pool)`` -- every row when
    ``m <= pool``, an even stride otherwise.  Strictly increasing, below ``m``."""
    m, pool = int(m), int(pool)
    if m < 0 or pool < 1:
        raise ValueError(f"candidate_rows: m {m} must be >= 0 and pool {pool} >= 1")
    c = min(m, pool)
    if c == 0:
        return np.zeros(0, np.int64)
    return (np.arange(c, dtype=np.int64) * m) // c


def coverage_radius(dist2, count) -> np.ndarray:
    """The covering radius of each run, in the units of the points: the square
    root of the last chosen ``fp_dist2``.  Every valid candidate of set ``s``
    lies within it of one of the set's samples (a sample chosen later would
    have been at least as far).  ``dist2`` is (S, K), ``count`` (S, 2) as
    ``fp_count`` or (S,) as ``t0``.  inf for a run of one sample (nothing bounds
    the others), nan for an empty set."""
    dist2 = np.asarray(dist2, np.float32)
    t0 = np.asarray(count)
    if t0.ndim == dist2.ndim:
        t0 = t0[..., 0]
    t0 = t0.astype(np.int64)
    last = np.take_along_axis(dist2, np.maximum(t0 - 1, 0)[..., None], axis=-1)[..., 0]
    with np.errstate(invalid="ignore"):
        return np.where(t0 > 0, np.sqrt(last.astype(np.float64)), np.nan)


def take_prefix(run: Dict[str, np.ndarray], k: int) -> Dict[str, np.ndarray]:
    """The run of ``k`` samples out of a stored run of K >= ``k``: its first
    ``k`` entries, exactly what the pass returns for ``samples=k`` on the same
    sets, keys and seed (every prefix of a farthest-point run is one; entries
    past ``t0`` repeat the run and do so in a prefix too).  ``run`` maps names
    to arrays whose axis 1 is the samples (``index``, ``xyz``, ``dist2``, any
    payload; a list of such arrays, as ``payloads`` of
    ``Renderer.farthest_points_host``) and ``count`` to (S, 2) ``fp_count``,
    whose ``t0`` becomes ``min(t0, k)``."""
    k = int(k)
    out = {}
    for name, v in run.items():
        if isinstance(v, (list, tuple)):   # "payloads" of farthest_points_host: one array each
            out[name] = [take_prefix({name: p}, k)[name] for p in v]
            continue
        v = np.asarray(v)
        if name == "count":
            c = v.copy()
            c[..., 0] = np.minimum(c[..., 0], k)
            out[name] = c
            continue
        if v.ndim < 2 or k < 1 or k > v.shape[1]:
            raise ValueError(f"take_prefix: {name!r} of shape {v.shape} has no prefix of {k} samples")
        out[name] = v[:, :k].copy()
    return out
