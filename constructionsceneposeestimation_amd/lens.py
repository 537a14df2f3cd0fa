"""Lens distortion (Brown-Conrady, OpenCV's rational model) of rendered frames:
the model, its presets, the per-lens map (``csg_lens_map``: host arithmetic in
float64, no GPU), the fits of the second camera, and the keypoints' forward model.
The frames themselves are resampled on the GPU (:meth:`renderer.Renderer.lens_remap`,
:meth:`renderer.Renderer.lens_remap_host`, ``--outputs lens``); include/csg_api.h
holds the definition, DESIGN.md §13.13 the reasoning.

Two cameras: the *source* camera is the pinhole camera the frames were rendered
with (a wider field of view, any size); the *output* camera is the one with the
lens.  Pixel ``i`` covers ``[i, i + 1)`` and its centre is ``i + 0.5`` in both
(``cx = W / 2`` for a centred lens); :meth:`LensModel.opencv` gives OpenCV's
numbers, which are these minus 1/2."""
from __future__ import annotations

import ctypes as C
import dataclasses
import hashlib
import math
from typing import Dict, Optional, Tuple

import numpy as np

COEFFS = ("k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6")   # OpenCV's order
cause_names = ("valid", "no_preimage", "outside")             # lens_valid / lens_count
FOCAL_STEP = 1.0 / 64.0                                       # the grid of fit_source and fit_output, pixels
F32 = np.float32

# Illustrative coefficient sets, NOT calibrated against any device: the orders of magnitude wide-angle site
# cameras report (k1 .. k6 in OpenCV's order).
PRESETS: Dict[str, Tuple[float, ...]] = {
    "mild": (-0.08, 0.01, 2e-4, -1e-4, 0.0, 0.0, 0.0, 0.0),
    "wide": (-0.2, 0.03, 8e-4, -5e-4, 0.0, 0.0, 0.0, 0.0),
    "site": (-0.25, 0.05, 1e-3, -5e-4, -0.005, 0.0, 0.0, 0.0),
    "rational": (0.9, 0.3, 2e-4, 1e-4, 0.01, 1.3, 0.6, 0.05),
}


@dataclasses.dataclass(frozen=True)
class LensModel:
    """csg_lens_model: the output camera, the coefficients, the source camera."""
    width: int
    height: int
    fx: float
    fy: float
    cx: float
    cy: float
    k1: float = 0.0
    k2: float = 0.0
    p1: float = 0.0
    p2: float = 0.0
    k3: float = 0.0
    k4: float = 0.0
    k5: float = 0.0
    k6: float = 0.0
    src_width: int = 0
    src_height: int = 0
    sfx: float = 0.0
    sfy: float = 0.0
    scx: float = 0.0
    scy: float = 0.0

    @property
    def coeffs(self) -> Tuple[float, ...]:
        return tuple(float(getattr(self, k)) for k in COEFFS)

    def as_dict(self) -> dict:
        return dataclasses.asdict(self)

    @classmethod
    def from_dict(cls, d: dict) -> "LensModel":
        ints = ("width", "height", "src_width", "src_height")
        return cls(**{f.name: (int if f.name in ints else float)(d[f.name]) for f in dataclasses.fields(cls)})

    def with_source(self, src_width: int, src_height: int, sfx: float, sfy: float, scx: float, scy: float) -> "LensModel":
        return dataclasses.replace(self, src_width=int(src_width), src_height=int(src_height), sfx=float(sfx),
                                   sfy=float(sfy), scx=float(scx), scy=float(scy))

    def opencv(self) -> dict:
        """Both cameras in OpenCV's pixel convention (centre of pixel i at i): K matrices and the coefficients."""
        return {"K": [[self.fx, 0.0, self.cx - 0.5], [0.0, self.fy, self.cy - 0.5], [0.0, 0.0, 1.0]],
                "dist_coeffs": list(self.coeffs),
                "source_K": [[self.sfx, 0.0, self.scx - 0.5], [0.0, self.sfy, self.scy - 0.5], [0.0, 0.0, 1.0]]}

    def to_c(self):
        from . import _lib
        return _lib.LensModel(int(self.width), int(self.height), int(self.src_width), int(self.src_height),
                              float(self.fx), float(self.fy), float(self.cx), float(self.cy),
                              *[float(v) for v in self.coeffs], float(self.sfx), float(self.sfy), float(self.scx),
                              float(self.scy))


def output_camera(coeffs, width: int, height: int, f: float) -> LensModel:
    """A centred output camera of focal length ``f`` with ``coeffs`` (k1 k2 p1 p2 k3 [k4 k5 k6]); no source yet."""
    c = tuple(float(v) for v in coeffs) + (0.0,) * (8 - len(coeffs))
    if len(c) != 8:
        raise ValueError(f"lens: {len(coeffs)} coefficients, want 5 or 8 (k1 k2 p1 p2 k3 [k4 k5 k6])")
    return LensModel(int(width), int(height), float(f), float(f), width / 2.0, height / 2.0, *c)


def build_map(model: LensModel):
    """``csg_lens_map`` -> (map (H, W, 2) int32, counts (3,) uint32 = valid, no preimage, outside).  A valid
    entry is the source position in 1/256 px, any other ``(INT32_MIN, cause)``.  Needs no GPU."""
    from . import _lib
    lib = _lib.load()
    W, H = int(model.width), int(model.height)
    if not (1 <= W <= 8192 and 1 <= H <= 8192):
        raise _lib.CsgError(f"lens map: output size {W} x {H} outside 1..8192")
    out = np.empty((H, W, 2), np.int32)
    counts = np.zeros(3, np.uint32)
    m = model.to_c()
    rc = lib.csg_lens_map(C.byref(m), out.ctypes.data, counts.ctypes.data)
    if rc != 0:
        raise _lib.CsgError(f"lens map: the model is refused (a size outside 1..8192, a number that is not finite, "
                            f"a focal length that is not > 0): {model}")
    return out, counts


def map_digest(lens_map: np.ndarray) -> str:
    """SHA-256 of the map's little-endian int32 bytes in (H, W, 2) order."""
    return hashlib.sha256(np.ascontiguousarray(lens_map, "<i4").tobytes()).hexdigest()


def forward(model: LensModel, x, y):
    """The forward model in float64: normalised pinhole (x, y) -> normalised distorted (xd, yd)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    k1, k2, p1, p2, k3, k4, k5, k6 = model.coeffs
    r2 = x * x + y * y
    R = (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1.0 + r2 * (k4 + r2 * (k5 + r2 * k6)))
    return (x * R + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x), y * R + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)


def _outside(model: LensModel) -> int:
    return int(build_map(model)[1][2])


def _border_outside(model: LensModel) -> int:
    """The outside count of the four border rows and columns alone, as one-pixel-wide cameras: an estimate
    that places the start of a search (the extreme source positions of a lens without a fold lie on the
    border); the searches themselves count whole maps."""
    W, H = model.width, model.height
    strips = (dataclasses.replace(model, height=1), dataclasses.replace(model, height=1, cy=model.cy - (H - 1)),
              dataclasses.replace(model, width=1), dataclasses.replace(model, width=1, cx=model.cx - (W - 1)))
    return sum(_outside(s) for s in strips)


def _search(outside_at, n: int, grow: int) -> int:
    """The grid focal length n (in FOCAL_STEPs) nearest the start for which ``outside_at(n) == 0`` and
    ``outside_at(n + grow) > 0`` (grow = +1 or -1); ``outside_at`` is monotone along ``grow``."""
    n = max(int(n), 1)
    step = 1
    while outside_at(n) > 0:            # back off, doubling, until a fit
        n -= grow * step
        step *= 2
        if n < 1 or n > 1 << 26:
            raise ValueError("lens: no focal length on the grid fits")
    lo, hi = n, None                    # lo fits; find a hi that does not, then bisect
    step = 1
    while hi is None:
        cand = lo + grow * step
        if cand < 1 or cand > 1 << 26:
            raise ValueError("lens: every focal length on the grid fits")
        if outside_at(cand) > 0:
            hi = cand
        else:
            lo, step = cand, step * 2
    while abs(hi - lo) > 1:
        mid = (lo + hi) // 2
        if outside_at(mid) > 0:
            hi = mid
        else:
            lo = mid
    return lo


def fit_source(model: LensModel, W: Optional[int] = None, H: Optional[int] = None, src_size=None) -> LensModel:
    """The source camera for ``model``'s output camera (``W``, ``H`` default to the model's): centred in
    ``src_size`` = (SW, SH) (default the output's size), square pixels, and the largest focal length on the grid
    of FOCAL_STEP = 1/64 px whose map has no pixel outside the source -- the finest sampling the source size
    allows.  Deterministic: the outside count is monotone in the focal length, the search bisects it with
    ``csg_lens_map`` itself (from a start that the border pixels alone place), so one step more gives an
    outside pixel."""
    W = model.width if W is None else int(W)
    H = model.height if H is None else int(H)
    SW, SH = (W, H) if src_size is None else (int(src_size[0]), int(src_size[1]))
    base = dataclasses.replace(model, width=W, height=H)

    def at(n):
        return _outside(base.with_source(SW, SH, n * FOCAL_STEP, n * FOCAL_STEP, SW / 2.0, SH / 2.0))

    def cam(n):
        return base.with_source(SW, SH, n * FOCAL_STEP, n * FOCAL_STEP, SW / 2.0, SH / 2.0)

    start = _search(lambda k: _border_outside(cam(k)), int(min(model.fx, model.fy) / FOCAL_STEP), +1)
    n = _search(at, start, +1)
    return base.with_source(SW, SH, n * FOCAL_STEP, n * FOCAL_STEP, SW / 2.0, SH / 2.0)


def fit_output(model: LensModel, source=None) -> LensModel:
    """The output camera for a given source camera (``source`` = (SW, SH, sfx, sfy, scx, scy), default the
    model's own): centred, square pixels, and the widest view -- the smallest focal length on the grid of
    FOCAL_STEP -- whose map has no pixel outside the source.  (A longer focal length only narrows the view and
    never adds an outside pixel, so it is one step *less* that gives one.)"""
    if source is not None:
        model = model.with_source(*source)

    def cam(n):
        return dataclasses.replace(model, fx=n * FOCAL_STEP, fy=n * FOCAL_STEP, cx=model.width / 2.0, cy=model.height / 2.0)

    start = _search(lambda k: _border_outside(cam(k)), int(math.ceil(max(model.sfx, model.sfy) / FOCAL_STEP)), -1)
    n = _search(lambda k: _outside(cam(k)), start, -1)
    return cam(n)


def distort_points(model: LensModel, uv, vis):
    """``csg_lens_points`` in NumPy float32, operation for operation: keypoints ``uv`` (..., 2) float32 in source
    pixels and their ``vis`` (...) int32 -> (uv, vis) in the output camera.  ``vis`` becomes 0 where the point
    leaves the output frame or lies beyond the fold (the Jacobian is not positive definite); where a value is
    not finite the point is (0, 0) and ``vis`` 0."""
    uv = np.asarray(uv, F32)
    vis = np.asarray(vis, np.int32)
    f = {k: F32(getattr(model, k)) for k in COEFFS + ("fx", "fy", "cx", "cy", "sfx", "sfy", "scx", "scy")}
    one, two, three, six = F32(1.0), F32(2.0), F32(3.0), F32(6.0)
    with np.errstate(all="ignore"):
        x = (uv[..., 0] - f["scx"]) / f["sfx"]
        y = (uv[..., 1] - f["scy"]) / f["sfy"]
        xx, yy, xy = x * x, y * y, x * y
        r2 = xx + yy
        r4 = r2 * r2
        r6 = r4 * r2
        N = one + ((f["k1"] * r2 + f["k2"] * r4) + f["k3"] * r6)
        D = one + ((f["k4"] * r2 + f["k5"] * r4) + f["k6"] * r6)
        Np = (f["k1"] + (two * f["k2"]) * r2) + (three * f["k3"]) * r4
        Dp = (f["k4"] + (two * f["k5"]) * r2) + (three * f["k6"]) * r4
        R = N / D
        Rp = (Np * D - N * Dp) / (D * D)
        xd = (x * R + (two * f["p1"]) * xy) + f["p2"] * (r2 + two * xx)
        yd = (y * R + f["p1"] * (r2 + two * yy)) + (two * f["p2"]) * xy
        a = ((R + (two * xx) * Rp) + (two * f["p1"]) * y) + (six * f["p2"]) * x
        b = ((two * xy) * Rp + (two * f["p1"]) * x) + (two * f["p2"]) * y
        d = ((R + (two * yy) * Rp) + (six * f["p1"]) * y) + (two * f["p2"]) * x
        uo = f["fx"] * xd + f["cx"]
        vo = f["fy"] * yd + f["cy"]
        finite = np.isfinite(uo) & np.isfinite(vo) & np.isfinite(a) & np.isfinite(b) & np.isfinite(d)
        inside = (uo >= F32(0.0)) & (uo < F32(model.width)) & (vo >= F32(0.0)) & (vo < F32(model.height))
        unfolded = (a * d - b * b > F32(0.0)) & (a + d > F32(0.0))
    assert uo.dtype == F32 and a.dtype == F32
    out = np.stack([np.where(finite, uo, F32(0.0)), np.where(finite, vo, F32(0.0))], axis=-1).astype(F32)
    return out, np.where(finite & inside & unfolded, vis, 0).astype(np.int32)
