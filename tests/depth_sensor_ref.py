"""The definition of csg_sensor_depth (include/csg_api.h) restated in NumPy, and
the synthetic depth images its tests share.  Every float operation is a float32
array operation, which rounds once; everything else is int64."""
import numpy as np

F32 = np.float32
CLIP_BAND = 1
BIG = 1 << 40


def job_fields(**kw):
    """The model fields of a csg_sensor_job with the tests' defaults."""
    j = dict(radius=2, min_support=13, tol=256, subpixel_bits=3, noise_k=40, seed=1, flags=CLIP_BAND, baseline=0.12,
             z_min=0.5, z_max=20.0)
    j.update(kw)
    return j


def fmix32(x):
    x = np.asarray(x, np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def noise_e(seed, key, p, noise_k):
    """e of the pixels ``p`` (row-major indices) of the frame with ``key``, int64."""
    base = fmix32(np.uint64((int(seed) ^ int(key)) & 0xFFFFFFFF))
    h1 = fmix32(base ^ np.asarray(p, np.uint64))
    h2 = fmix32(h1 ^ np.uint64(0x9E3779B9))
    g = ((h1 & 0xFFFF) + (h1 >> 16) + (h2 & 0xFFFF) + (h2 >> 16)).astype(np.int64) - 131070
    return (g * int(noise_k) + 32768) >> 16


def disparity(depth, fx, baseline):
    """-> (fb, surface, dq int64) of a frame."""
    with np.errstate(all="ignore"):
        d = np.asarray(depth, F32)
        fb = F32(fx) * F32(abs(F32(baseline)))
        D = fb / d
        surface = np.isfinite(d) & (d > 0) & (D > 0)
        big = np.isinf(D) | (D >= F32(4194304.0))
        t = D * F32(256.0) + F32(0.5)
        dq = np.where(surface & ~big, np.where(surface & ~big, t, F32(0)).astype(np.int64), 1 << 30)
    return fb, surface, dq


def restate_frame(depth, fx, key, job):
    """One frame (H, W) -> dict(sensor_depth (H, W) float32, sensor_cause (H, W) uint8,
    sensor_count (7,) uint32, lit, dq)."""
    d = np.asarray(depth, F32)
    H, W = d.shape
    b = float(F32(job["baseline"]))
    fb, surface, dq = disparity(d, fx, b)
    x = np.arange(W, dtype=np.int64)[None, :]
    u = 256 * x + 128 - dq if b > 0 else 256 * x + 128 + dq
    if b > 0:   # exclusive suffix minimum of u over the surface pixels
        v = np.where(surface, u, BIG)
        run = np.minimum.accumulate(v[:, ::-1], axis=1)[:, ::-1]
        before = np.concatenate([run[:, 1:], np.full((H, 1), BIG)], axis=1)
        hidden = before <= u
        band = u < 0
    else:       # exclusive prefix maximum
        v = np.where(surface, u, -BIG)
        run = np.maximum.accumulate(v, axis=1)
        before = np.concatenate([np.full((H, 1), -BIG), run[:, :-1]], axis=1)
        hidden = before >= u
        band = u >= 256 * W
    with np.errstate(all="ignore"):
        in_range = (F32(job["z_min"]) <= d) & (d <= F32(job["z_max"]))
    cause = np.zeros((H, W), np.uint8)
    cause[band & bool(job["flags"] & CLIP_BAND)] = 4
    cause[hidden] = 3
    cause[~in_range] = 2
    cause[~surface] = 1
    lit = cause == 0
    r, tol = int(job["radius"]), int(job["tol"])
    litp = np.pad(lit, r, constant_values=False)
    dqp = np.pad(dq, r, constant_values=0)
    n = np.zeros((H, W), np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            n += litp[dy:dy + H, dx:dx + W] & (np.abs(dqp[dy:dy + H, dx:dx + W] - dq) <= tol)
    cause[lit & (n < int(job["min_support"]))] = 5
    p = (np.arange(H, dtype=np.int64)[:, None] * W + x).astype(np.uint64)
    e = noise_e(job["seed"], key, p, job["noise_k"])
    sh = 8 - int(job["subpixel_bits"])
    m = (dq + e + ((1 << sh) >> 1)) >> sh
    cause[(cause == 0) & (m <= 0)] = 6
    ret = cause == 0
    dn = np.where(ret, m << sh, 1)
    assert dn.max() < 2 ** 31
    with np.errstate(all="ignore"):
        val = (fb * F32(256.0)) / dn.astype(F32)
    out = np.where(ret, val, F32(0)).astype(F32)
    return dict(sensor_depth=out, sensor_cause=cause, sensor_count=np.bincount(cause.ravel(), minlength=7).astype(np.uint32),
                lit=lit, dq=dq)


def restate(depth, intrinsics, job, frame_keys=None):
    """Frames (n, H, W) -> dict of the three outputs, stacked."""
    fr = [restate_frame(depth[f], intrinsics[f][0], f if frame_keys is None else int(frame_keys[f]), job)
          for f in range(len(depth))]
    return {k: np.stack([x[k] for x in fr]) for k in ("sensor_depth", "sensor_cause", "sensor_count")}


def intr(n, fx=600.0):
    a = np.zeros((n, 4), F32)
    a[:, 0] = fx
    a[:, 1] = fx
    return a


def composite(H=67, W=131):
    """A background plane at 8 m; 6 rows of +inf; a 20-column box at 2 m; a 2-px bar at 3 m; a strip at
    25 m and one at 0.3 m (6 rows each); a ramp whose disparity gradient exceeds 1 px/px (fx 600, |b| 0.12)."""
    d = np.full((H, W), 8.0, F32)
    d[0:6] = np.inf
    d[6:12] = 25.0
    d[12:18] = 0.3
    d[18:, 40:60] = 2.0
    d[18:, 80:82] = 3.0
    # disparity 9 px at the plane; the ramp climbs 2 px of disparity per column over 12 columns
    cols = np.arange(100, 112)
    d[40:60, 100:112] = (F32(72.0) / (F32(9.0) + F32(2.0) * (cols - 99).astype(F32)))[None, :]
    return d


def scale_composite(d, H, W):
    """The composite resampled (nearest) to another size, so small frames keep a bit of everything."""
    ys = (np.arange(H) * d.shape[0]) // H
    xs = (np.arange(W) * d.shape[1]) // W
    return np.ascontiguousarray(d[ys][:, xs])


def random_depth(n, H, W, rng):
    """Mostly plausible depths in patches, salted with NaN, +-inf, 0, negatives, denormals, 1e-30 and 1e30."""
    d = rng.uniform(0.4, 22.0, (n, H, W)).astype(F32)
    smooth = rng.uniform(1.0, 12.0, (n, (H + 7) // 8, (W + 7) // 8)).astype(F32)
    block = np.repeat(np.repeat(smooth, 8, axis=1), 8, axis=2)[:, :H, :W]
    d = np.where(rng.random((n, H, W)) < 0.7, block, d).astype(F32)
    odd = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -3.0, 1e-40, 1.4e-45, 1e-30, 1e30, 1e-38], F32)
    pick = rng.random((n, H, W)) < 0.08
    d[pick] = odd[rng.integers(0, len(odd), int(pick.sum()))]
    return d
