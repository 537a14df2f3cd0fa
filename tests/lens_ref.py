"""The definitions of csg_lens_map and csg_lens_remap (include/csg_api.h, the
header comment of csrc/csg_lens_map.h) restated in NumPy, from the text and not
from the code, and the lenses, models and adversarial sources the tests share.

A model is a plain dict with the fields of csg_lens_model.  Every float64
operation of NumPy rounds once, as the C code built with -ffp-contract=off
does, so the map is compared bit for bit."""
import numpy as np

NEWTON = 16
INT32_MIN = -2 ** 31
COEFFS = ("k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6")

# name -> k1 k2 p1 p2 k3 k4 k5 k6 (OpenCV's order)
LENSES = {
    "tame": (-0.2, 0.03, 8e-4, -5e-4, 0.0, 0.0, 0.0, 0.0),
    "pin": (0.1, 0.02, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
    "rational": (0.9, 0.3, 2e-4, 1e-4, 0.01, 1.3, 0.6, 0.05),
    "barrel": (-0.25, 0.05, 1e-3, -5e-4, -0.005, 0.0, 0.0, 0.0),
    "fold": (-0.6, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
}
SIZES = [(1, 1), (3, 5), (1, 130), (67, 131), (240, 320)]   # H, W


def model(coeffs, W=320, H=240, fx=200.0, fy=None, cx=None, cy=None, src=None, sf=None, sc=None):
    """A model dict: output camera W x H with fx, fy (fy = fx) and centre (W / 2, H / 2) unless given; source
    camera of size ``src`` = (SW, SH) (default the output's) with focal lengths ``sf`` (default the output's)
    and centre ``sc`` (default its middle)."""
    fy = fx if fy is None else fy
    SW, SH = (W, H) if src is None else src
    sfx, sfy = (fx, fy) if sf is None else sf
    scx, scy = (SW / 2.0, SH / 2.0) if sc is None else sc
    m = dict(width=int(W), height=int(H), src_width=int(SW), src_height=int(SH), fx=float(fx), fy=float(fy),
             cx=float(W / 2.0 if cx is None else cx), cy=float(H / 2.0 if cy is None else cy),
             sfx=float(sfx), sfy=float(sfy), scx=float(scx), scy=float(scy))
    m.update({k: float(v) for k, v in zip(COEFFS, coeffs)})
    return m


def forward(m, x, y):
    """The forward model and its (symmetric) Jacobian in float64, in the header's order -> xd, yd, a, b, d."""
    k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(m[k]) for k in COEFFS)
    with np.errstate(all="ignore"):
        xx, yy, xy = x * x, y * y, x * y
        r2 = xx + yy
        r4 = r2 * r2
        r6 = r4 * r2
        N = 1.0 + ((k1 * r2 + k2 * r4) + k3 * r6)
        D = 1.0 + ((k4 * r2 + k5 * r4) + k6 * r6)
        Np = (k1 + (2.0 * k2) * r2) + (3.0 * k3) * r4
        Dp = (k4 + (2.0 * k5) * r2) + (3.0 * k6) * r4
        R = N / D
        Rp = (Np * D - N * Dp) / (D * D)
        xd = (x * R + (2.0 * p1) * xy) + p2 * (r2 + 2.0 * xx)
        yd = (y * R + p1 * (r2 + 2.0 * yy)) + (2.0 * p2) * xy
        a = ((R + (2.0 * xx) * Rp) + (2.0 * p1) * y) + (6.0 * p2) * x
        b = ((2.0 * xy) * Rp + (2.0 * p1) * x) + (2.0 * p2) * y
        d = ((R + (2.0 * yy) * Rp) + (6.0 * p1) * y) + (2.0 * p2) * x
    return xd, yd, a, b, d


def invert(m):
    """Newton's inverse of every output pixel -> x, y (H, W) float64 and the last forward evaluation."""
    W, H = m["width"], m["height"]
    i = np.arange(W, dtype=np.float64)[None, :] + np.zeros((H, 1))
    j = np.arange(H, dtype=np.float64)[:, None] + np.zeros((1, W))
    with np.errstate(all="ignore"):
        xd0 = ((i + 0.5) - np.float64(m["cx"])) / np.float64(m["fx"])
        yd0 = ((j + 0.5) - np.float64(m["cy"])) / np.float64(m["fy"])
        x, y = xd0.copy(), yd0.copy()
        for _ in range(NEWTON):
            xd, yd, a, b, d = forward(m, x, y)
            ex, ey = xd - xd0, yd - yd0
            det = a * d - b * b
            x = x - (d * ex - b * ey) / det
            y = y - (a * ey - b * ex) / det
    return x, y, xd0, yd0, forward(m, x, y)


def lens_map(m):
    """csg_lens_map restated -> (map (H, W, 2) int32, counts (3,) uint32)."""
    x, y, xd0, yd0, (xd, yd, a, b, d) = invert(m)
    with np.errstate(all="ignore"):
        mx, my = (xd - xd0) * np.float64(m["fx"]), (yd - yd0) * np.float64(m["fy"])
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(xd) & np.isfinite(yd) & np.isfinite(a) & np.isfinite(b) & np.isfinite(d)
        miss = mx * mx + my * my > 2.0 ** -20
        unfolded = (a * d - b * b > 0.0) & (a + d > 0.0)
        pre = finite & ~miss & unfolded
        sx, sy = np.float64(m["sfx"]) * x + np.float64(m["scx"]), np.float64(m["sfy"]) * y + np.float64(m["scy"])
        tx, ty = np.floor(sx * 256.0 + 0.5), np.floor(sy * 256.0 + 0.5)
        lim = 2147483647.0
        fits = (tx >= -lim) & (tx <= lim) & (ty >= -lim) & (ty <= lim)
    qx = np.where(pre & fits, tx, 0.0).astype(np.int64)
    qy = np.where(pre & fits, ty, 0.0).astype(np.int64)
    inside = pre & fits & ((qx >> 8) >= 0) & ((qx >> 8) < m["src_width"]) & ((qy >> 8) >= 0) & ((qy >> 8) < m["src_height"])
    cause = np.where(~pre, 1, np.where(~inside, 2, 0))
    out = np.empty((m["height"], m["width"], 2), np.int32)
    out[..., 0] = np.where(cause == 0, qx, INT32_MIN)
    out[..., 1] = np.where(cause == 0, qy, cause)
    return out, np.bincount(cause.reshape(-1), minlength=3).astype(np.uint32)


def identity_model(W, H, f=100.0):
    return model((0.0,) * 8, W=W, H=H, fx=f)


def map_cause(mp, SW, SH):
    """The cause csg_lens_remap gives every entry of a map (H, W, 2) int32, and the source pixel of the valid ones."""
    qx, qy = mp[..., 0].astype(np.int64), mp[..., 1].astype(np.int64)
    tagged = qx == INT32_MIN
    px, py = qx >> 8, qy >> 8
    outside = (px < 0) | (px >= SW) | (py < 0) | (py >= SH)
    cause = np.where(tagged, np.where(qy == 1, 1, 2), np.where(outside, 2, 0)).astype(np.uint8)
    return cause, np.where(cause == 0, px, 0), np.where(cause == 0, py, 0)


def remap(mp, SW, SH, n, rgb=None, instance=None, depth=None, obj_coords=None, n_labels=0, nearest=False):
    """csg_lens_remap restated: every output the given sources allow, for ``n`` frames."""
    H, W = mp.shape[:2]
    cause, px, py = map_cause(mp, SW, SH)
    ok = cause == 0
    out = {"lens_valid": np.broadcast_to(cause, (n, H, W)).copy()}
    out["lens_count"] = np.tile(np.bincount(cause.reshape(-1), minlength=3).astype(np.uint32), (n, 1))
    if instance is not None:
        ids = np.where(ok, instance[:, py, px], -1).astype(np.int32)
        out["lens_instance"] = ids
        if n_labels:
            st = np.zeros((n, n_labels, 5), np.uint32)
            st[:, :, 1:3] = 0xFFFFFFFF
            for f in range(n):
                for l in np.unique(ids[f]):
                    if 0 <= l < n_labels:
                        ys, xs = np.nonzero(ids[f] == l)
                        st[f, l] = (len(xs), xs.min(), ys.min(), xs.max(), ys.max())
            out["lens_stats"] = st
    if depth is not None:
        bits = depth.view(np.uint32)[:, py, px]
        out["lens_depth"] = np.where(ok, bits, np.uint32(0x7F800000)).astype(np.uint32).view(np.float32)
    if obj_coords is not None:
        out["lens_coords"] = np.where(ok[..., None], obj_coords[:, py, px], 0).astype(np.uint16)
    if rgb is not None:
        if nearest:
            out["lens_rgb"] = np.where(ok[..., None], rgb[:, py, px], 0).astype(np.uint8)
        else:
            qx = np.where(ok, mp[..., 0], 128).astype(np.int64)
            qy = np.where(ok, mp[..., 1], 128).astype(np.int64)
            tx, ty = qx - 128, qy - 128
            x0, y0, fx, fy = tx >> 8, ty >> 8, tx & 255, ty & 255
            xl, xr = np.clip(x0, 0, SW - 1), np.clip(x0 + 1, 0, SW - 1)
            yt, yb = np.clip(y0, 0, SH - 1), np.clip(y0 + 1, 0, SH - 1)
            c = rgb.astype(np.int64)
            acc = (((256 - fx) * (256 - fy))[..., None] * c[:, yt, xl] + (fx * (256 - fy))[..., None] * c[:, yt, xr] +
                   ((256 - fx) * fy)[..., None] * c[:, yb, xl] + (fx * fy)[..., None] * c[:, yb, xr] + 32768) >> 16
            out["lens_rgb"] = np.where(ok[..., None], acc, 0).astype(np.uint8)
    return out


def sources(n, SH, SW, n_labels, seed):
    """Adversarial source frames: random RGB, ids with -1 and ids at or above n_labels, depths with +-inf, NaN
    (two payloads) and denormals, random object coordinates."""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (n, SH, SW, 3), dtype=np.uint8)
    blocks = rng.integers(-1, n_labels + 3, (n, (SH + 6) // 7, (SW + 8) // 9))   # patches of one id: uniform waves too
    inst = np.repeat(np.repeat(blocks, 7, axis=1), 9, axis=2)[:, :SH, :SW].astype(np.int32)
    noise = rng.random((n, SH, SW)) < 0.1
    inst = np.where(noise, rng.integers(-1, n_labels + 3, (n, SH, SW)), inst).astype(np.int32)
    inst.reshape(-1)[:3] = [-1, n_labels, 2 ** 31 - 1][:inst.size]
    depth = rng.uniform(0.5, 250.0, (n, SH, SW)).astype(np.float32)
    odd = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC12345, 0x00000001, 0x807FFFFF, 0x00000000, 0x80000000],
                   np.uint32).view(np.float32)
    pick = rng.random((n, SH, SW)) < 0.15
    depth = np.where(pick, odd[rng.integers(0, len(odd), (n, SH, SW))], depth).astype(np.float32)
    coords = rng.integers(0, 65536, (n, SH, SW, 3), dtype=np.uint16)
    return rgb, inst, depth, coords


def hand_map(H, W, SH, SW, seed):
    """A hand-made map: random valid entries; entries on the source's first and last row and column; fractions 0
    and 255; tagged entries of every cause and of unknown causes; untagged entries far outside the source and
    negative ones."""
    rng = np.random.default_rng(seed)
    mp = np.empty((H, W, 2), np.int32)
    mp[..., 0] = rng.integers(0, SW * 256, (H, W))
    mp[..., 1] = rng.integers(0, SH * 256, (H, W))
    flat = mp.reshape(-1, 2)
    special = [(0, 0), (255, 255), (SW * 256 - 1, SH * 256 - 1), (SW * 256 - 256, 0), (0, SH * 256 - 256),
               (127, 128), (128, 127), (SW * 256 - 129, SH * 256 - 128), (256 * (SW // 2), 256 * (SH // 2) + 255),
               (INT32_MIN, 1), (INT32_MIN, 2), (INT32_MIN, 0), (INT32_MIN, 3), (INT32_MIN, -1), (INT32_MIN, INT32_MIN),
               (INT32_MIN, 2 ** 31 - 1), (SW * 256, 0), (0, SH * 256), (2 ** 31 - 1, 2 ** 31 - 1), (-1, 0), (0, -1),
               (-256, -256), (INT32_MIN + 1, 5), (5, INT32_MIN), (2 ** 30, 7), (-2 ** 30, -2 ** 30)]
    where = rng.permutation(flat.shape[0])
    for k, e in enumerate(special * 3):
        if k < len(where):
            flat[where[k]] = e
    return mp
