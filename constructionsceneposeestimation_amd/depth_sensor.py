"""Simulated stereo-camera depth, host side: the model that goes with
``csg_sensor_depth`` (include/csg_api.h), whose images are made on the GPU
(:meth:`renderer.Renderer.sensor_depth`, :meth:`renderer.Renderer.sensor_depth_host`,
``--outputs depth_sensor16_png``).

A :class:`StereoModel` describes a stereo depth camera registered to the colour
camera in the terms its data sheet uses -- baseline, range, matching window,
sub-pixel step, disparity noise -- and :meth:`StereoModel.to_job_fields` turns
them into the integers of ``csg_sensor_job``.  The pass returns the depth such a
camera would report (0.0 where it reports none) and, per pixel, why a value is
missing (:data:`cause_names`).
"""
from __future__ import annotations

import math
from dataclasses import asdict, dataclass

# sensor_cause: why a pixel has no depth (0: it has)
cause_names = ("return", "none", "range", "half_occluded", "band", "support", "noise")
CLIP_BAND = 1   # CSG_SENSOR_CLIP_BAND


@dataclass(frozen=True)
class StereoModel:
    """A stereo depth camera registered to the colour camera.

    ``baseline`` metres, the second camera's x in the OpenCV camera frame (its
    sign decides on which side of a foreground edge the half-occlusion band
    lies); ``z_min`` / ``z_max`` metres, the range it reports; ``window`` the
    side of the matching window in pixels (odd, 1..9); ``min_support_fraction``
    the share of the window that must lie on the centre's surface (within
    ``tol_px`` of its disparity) for a match; ``subpixel`` the disparity steps
    per pixel (a power of two, 1..256); ``noise_sigma_px`` the standard deviation
    of the disparity noise in pixels; ``clip_band``: no depth where the second
    camera's image ends."""
    baseline: float = 0.12
    z_min: float = 0.5
    z_max: float = 30.0
    window: int = 5
    min_support_fraction: float = 0.5
    tol_px: float = 1.0
    subpixel: int = 8
    noise_sigma_px: float = 0.08
    clip_band: bool = True

    def __post_init__(self):
        if not (math.isfinite(self.baseline) and self.baseline != 0):
            raise ValueError(f"StereoModel: baseline {self.baseline!r} is not a finite value other than 0")
        if not (math.isfinite(self.z_min) and math.isfinite(self.z_max) and 0 < self.z_min <= self.z_max):
            raise ValueError(f"StereoModel: z_min {self.z_min!r}, z_max {self.z_max!r}: 0 < z_min <= z_max")
        if self.window not in (1, 3, 5, 7, 9):
            raise ValueError(f"StereoModel: window {self.window!r} is not odd in 1..9")
        if not 0 <= self.min_support_fraction <= 1:
            raise ValueError(f"StereoModel: min_support_fraction {self.min_support_fraction!r} outside 0..1")
        if not (math.isfinite(self.tol_px) and 0 <= self.tol_px * 256 < 2 ** 32):
            raise ValueError(f"StereoModel: tol_px {self.tol_px!r}")
        if self.subpixel not in (1, 2, 4, 8, 16, 32, 64, 128, 256):
            raise ValueError(f"StereoModel: subpixel {self.subpixel!r} is not a power of two in 1..256")
        if not (math.isfinite(self.noise_sigma_px) and 0 <= round(self.noise_sigma_px * 256 * math.sqrt(3)) <= 2 ** 20):
            raise ValueError(f"StereoModel: noise_sigma_px {self.noise_sigma_px!r}")

    def to_job_fields(self) -> dict:
        """The model fields of ``csg_sensor_job``: ``radius``, ``min_support``,
        ``tol``, ``subpixel_bits``, ``noise_k``, ``flags``, ``baseline``, ``z_min``,
        ``z_max``."""
        return {"radius": self.window // 2,
                "min_support": max(1, math.ceil(self.min_support_fraction * self.window ** 2)),
                "tol": int(round(self.tol_px * 256)),
                "subpixel_bits": self.subpixel.bit_length() - 1,
                "noise_k": int(round(self.noise_sigma_px * 256 * math.sqrt(3))),
                "flags": CLIP_BAND if self.clip_band else 0,
                "baseline": float(self.baseline), "z_min": float(self.z_min), "z_max": float(self.z_max)}

    def expected_sigma_z(self, z, fx):
        """The textbook depth noise of a stereo pair at depth ``z`` metres:
        ``z^2 * sigma_d / (fx * |baseline|)``, metres."""
        return z * z * self.noise_sigma_px / (fx * abs(self.baseline))

    def as_dict(self) -> dict:
        return asdict(self)


# Illustrative models, not calibrated against any device: a short-baseline indoor
# camera and a wide-baseline one for the 2-30 m of a construction site.
PRESETS = {
    "near": StereoModel(baseline=0.05, z_min=0.3, z_max=10.0, window=7, min_support_fraction=0.5, tol_px=1.0,
                        subpixel=8, noise_sigma_px=0.08, clip_band=True),
    "site": StereoModel(baseline=0.12, z_min=0.5, z_max=30.0, window=5, min_support_fraction=0.5, tol_px=1.0,
                        subpixel=16, noise_sigma_px=0.1, clip_band=True),
}
