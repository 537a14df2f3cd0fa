"""The GPU file encoders (csg_encode.hip) on adversarial synthetic buffers.

Every other GPU file test feeds the encoders what the renderer produced:
natural images, depths of 0.5..250 m or inf, points all-NaN or all-finite.
Here csg_encode_files (Renderer.encode_files) runs the same passes on device
tensors made for the purpose, at the shapes and values where the kernels take
another path, and every file is compared with a reference made in this module
by NumPy, zlib or np.savetxt -- never by the package's writers:

* PNG: decoded by zlib (tests/pngutil.py: every CRC, the Adler-32, the exact
  end of the stream, nothing after IEND), every IDAT chunk but the last 2048
  bytes, and byte for byte the file of the sequential restatement
  (tests/deflate_host.cpp, the GPU's unit split);
* CSV and point-cloud TXT: byte-identical to np.savetxt;
* PLY: byte-identical to ``restate_ply``;
* depth16: the quantiser of include/csg_api.h restated in float32 NumPy;
* depth_stats: counts and min / max exact, the sum against math.fsum.

Several frames of different content share a call wherever a case allows, and
one module-scoped context serves every shape, so per-frame histograms, offsets
and staging areas -- and scratch left over from a larger, earlier call -- are
checked too.  Preconditions a case relies on (Huffman depth above 15, zlib
length mod 2048, 47-character values, every run length present) are asserted
in the case itself.
"""
import heapq
import io
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from pngutil import decode_png
from tests.test_compact_files import decode_png16, restate_ply

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEG = 512                      # kSegBytes (csg_deflate.h): raw row bytes per PNG work unit
FLT_MAX = np.float32(3.4028235e38)
ALL_KINDS = ("rgb_png", "depth_csv", "depth_png", "pointcloud_txt", "pointcloud_ply", "depth16_png")


# ---------------------------------------------------------------------------
# fixtures and plumbing
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def enc(cone):
    """One context for every shape of the module (its own size is irrelevant)."""
    from constructionsceneposeestimation_amd.renderer import Renderer
    with Renderer(cone, 64, 64, max_frames=1) as r:
        yield r


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("enc")
    exe = str(d / "deflate_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(HERE, "deflate_host.cpp"), "-o", exe],
                   check=True)
    return exe, d


def _dev(a, offset=0):
    """``a`` as a device tensor, ``offset`` bytes into its allocation: (keep-alive, pointer)."""
    import torch
    a = np.ascontiguousarray(a)
    raw = torch.from_numpy(a.view(np.uint8).reshape(-1))
    buf = torch.zeros(raw.numel() + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[offset:offset + raw.numel()].copy_(raw)
    return buf, buf.data_ptr() + offset


def _encode(r, kinds, n, W, H, rgb=None, depth_vis=None, depth=None, points=None, scale=0.0, stats=False,
            offset=0, cap=None):
    """Run the encoders on NumPy arrays uploaded as torch tensors (the uint8
    images ``offset`` bytes off alignment); returns the files (and the stats)."""
    import torch
    keep, ptr = [], {}
    for name, a, off in (("rgb", rgb, offset), ("depth_vis", depth_vis, offset), ("depth", depth, 0),
                         ("points", points, 0)):
        if a is not None:
            t, p = _dev(a, off)
            keep.append(t)
            ptr[name] = p
    torch.cuda.synchronize()
    files = np.zeros(cap if cap is not None else (1 << 20) + n * H * W * 200, np.uint8)
    res = r.encode_files(n, W, H, kinds, files, depth16_counts_per_metre=scale, depth_stats=stats, **ptr)
    offsets, need = res[0], res[1]
    if cap is not None:
        assert offsets is None and need > cap
        files = np.zeros(need, np.uint8)
        offsets = r.copy_files(files, n * len(kinds))
    assert offsets is not None and int(offsets[-1]) == need
    assert (np.diff(offsets.astype(np.int64)) > 0).all()
    blobs = [bytes(files[int(offsets[j]):int(offsets[j + 1])]) for j in range(len(offsets) - 1)]
    del keep
    return (blobs, res[2]) if stats else blobs


# ---------------------------------------------------------------------------
# PNG: restatements
# ---------------------------------------------------------------------------
def _residuals_to_image(res, bpp=3):
    """Integrate Sub residuals (H, row bytes) along each row mod 256: the raw
    rows whose filtered stream is ``res``."""
    H, rb = res.shape
    lanes = res.reshape(H, rb // bpp, bpp).astype(np.uint64)
    return (np.cumsum(lanes, axis=1) & 255).astype(np.uint8).reshape(H, rb)


def _unit_runs(raw, bpp):
    """The run-length view of the GPU's token stream of raw rows (H, row
    bytes): per work unit (the filter byte leads unit 0 of a row) the list of
    (byte, run length).  A restatement of png_unit_bytes + RunTokenizer."""
    H, rb = raw.shape
    left = np.zeros_like(raw)
    left[:, bpp:] = raw[:, :-bpp]
    filt = np.concatenate([np.ones((H, 1), np.uint8), raw - left], axis=1)   # uint8 arithmetic wraps mod 256
    units = []
    for row in filt:
        for k in range((rb + SEG - 1) // SEG):
            s = row[(0 if k == 0 else 1 + k * SEG):1 + min((k + 1) * SEG, rb)]
            cut = np.flatnonzero(np.diff(s.astype(np.int16))) + 1
            starts = np.concatenate([[0], cut])
            lens = np.diff(np.concatenate([starts, [s.size]]))
            units.append((s[starts], lens))
    return units


def _token_histogram(raw, bpp):
    """Literal / length symbol counts (286) and the set of match lengths of the
    image's token stream (run_tokens of csg_deflate.h restated): a run is one
    literal, matches of at most 258 while 3 or more bytes remain, then literals."""
    hist = np.zeros(286, np.int64)
    match_lens, run_lens = set(), set()
    base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]                                                       # RFC 1951 3.2.5
    for vals, lens in _unit_runs(raw, bpp):
        short = lens <= 3
        np.add.at(hist, vals[short], lens[short])
        run_lens.update(np.unique(lens).tolist())
        for b, n in zip(vals[~short].tolist(), lens[~short].tolist()):
            hist[b] += 1
            rem = n - 1
            while rem >= 3:
                m = min(rem, 258)
                match_lens.add(m)
                hist[257 + max(i for i in range(29) if base[i] <= m)] += 1
                rem -= m
            hist[b] += rem
    hist[256] = 1
    return hist, match_lens, run_lens


def _min_max_depth(freq):
    """The smallest maximum code length over all optimal (unlimited) Huffman
    codes of ``freq``: ties go to the shallower subtree."""
    h = [(int(f), 0) for f in freq if f]
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


def _idat_sizes(png):
    pos, sizes = 8, []
    while pos < len(png):
        n, typ = struct.unpack(">I4s", png[pos:pos + 8])
        if typ == b"IDAT":
            sizes.append(n)
        pos += 12 + n
    assert pos == len(png)
    return sizes


def _harness_png(harness, raw, W, H, bpp):
    exe, d = harness
    src, dst = str(d / "in.raw"), str(d / "out.png")
    np.ascontiguousarray(raw).tofile(src)
    subprocess.run([exe, "png", str(W), str(H), src, dst] + (["2"] if bpp == 2 else []), check=True)
    return open(dst, "rb").read()


def _harness_zlen(harness, raw, W, H, bpp=3):
    exe, d = harness
    src = str(d / "z.raw")
    np.ascontiguousarray(raw).tofile(src)
    return int(subprocess.run([exe, "zlen", str(W), str(H), src, str(bpp)], check=True, capture_output=True,
                              text=True).stdout)


def _check_png(blob, img, harness, what):
    """``img``: (H, W, 3) uint8 or (H, W) uint16."""
    bpp = 3 if img.ndim == 3 else 2
    H, W = img.shape[:2]
    got = decode_png(blob) if bpp == 3 else decode_png16(blob)   # CRCs, Adler-32, exact stream end, nothing after IEND
    assert np.array_equal(got, img), what
    assert blob.endswith(b"\0\0\0\0IEND\xaeB`\x82"), what
    sizes = _idat_sizes(blob)
    assert sizes and all(n == 2048 for n in sizes[:-1]) and 0 < sizes[-1] <= 2048, (what, sizes)
    raw = img if bpp == 3 else img.astype(">u2")
    ref = _harness_png(harness, raw, W, H, bpp)
    assert len(blob) == len(ref) and blob == ref, f"{what}: differs from the sequential restatement"
    return sum(sizes)


# ---------------------------------------------------------------------------
# PNG: contents
# ---------------------------------------------------------------------------
def _noise(rng, H, W):
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def _ruler_residuals(rb, lo=1, hi=300):
    """Residual rows of ``rb`` bytes holding one run of every length lo..hi,
    each inside one work unit (never cut) and next to other values; the space
    left in a unit holds an alternating filler (runs of 1)."""
    assert hi <= min(SEG, rb)
    spans = [(a, min(a + SEG, rb)) for a in range(0, rb, SEG)]
    rows, row, u, pos, val = [], np.zeros(rb, np.uint8), 0, 0, 0

    def fill_to(end):
        row[pos:end] = 100 + 3 * (np.arange(end - pos) % 2)          # 100, 103, 100, ...

    for n in range(lo, hi + 1):
        while pos + n > spans[u][1]:
            fill_to(spans[u][1])
            u += 1
            if u == len(spans):
                rows.append(row)
                row, u = np.zeros(rb, np.uint8), 0
            pos = spans[u][0]
        val = 2 + (val + 1) % 90                                      # 2..91: never the filler, nor the last run's
        row[pos:pos + n] = val
        pos += n
    fill_to(rb)
    rows.append(row)
    return np.stack(rows)


def _ruler(W, H=None, bpp=3, hi=300):
    """An image whose filtered rows are the ruler's (repeated or cut to H rows)."""
    res = _ruler_residuals(bpp * W, 1, hi)
    if H is not None:
        res = np.resize(res, (H, bpp * W)) if res.shape[0] < H else res[:H]
    img = _residuals_to_image(np.ascontiguousarray(res), bpp)
    return img.reshape(img.shape[0], W, bpp)


def _fibonacci_image(W=171, H=236, n=24, seed=5):
    """Residual bytes whose counts are the Fibonacci numbers (the last count
    takes what is left of the image), shuffled: the optimal code is a comb."""
    fib = [1, 1]
    while len(fib) < n - 1:
        fib.append(fib[-1] + fib[-2])
    total = 3 * W * H
    assert sum(fib) < total
    counts = fib + [total - sum(fib)]
    res = np.repeat(np.arange(10, 10 + n, dtype=np.uint8), counts)
    np.random.default_rng(seed).shuffle(res)
    return _residuals_to_image(res.reshape(H, 3 * W)).reshape(H, W, 3)


PNG_SHAPES = [(1, 1), (1, 300), (170, 17), (171, 17), (341, 17), (342, 17), (176, 5), (16, 3)]   # W, H


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("W,H", PNG_SHAPES)
def test_png_shapes(enc, harness, W, H, offset):
    """Row bytes 3 (one unit of 4 stream bytes), 510, 513, 1023, 1026, 528 (every
    row 16-byte aligned: the 16-byte loads) and 48; 1x300 is 300 units (more
    than the 256 threads of the layout scan, more than 64 rows).  One batch
    mixes noise, flat and ruler frames; with ``offset`` 1 no row is aligned."""
    rng = np.random.default_rng(1000 * W + H)
    ruler = _ruler(W, H, hi=300) if 3 * W >= 300 else _residuals_to_image(
        np.repeat(rng.integers(0, 256, (H, W), dtype=np.uint8), 3, axis=1)).reshape(H, W, 3)
    ones = np.ones((H, W, 3), np.uint8)                            # a row's first run takes in the filter byte
    frames = np.stack([_noise(rng, H, W), np.full((H, W, 3), 200, np.uint8), ruler, ones, _noise(rng, H, W)])
    blobs = _encode(enc, ("rgb_png",), 5, W, H, rgb=frames, offset=offset)
    for f in range(5):
        _check_png(blobs[f], frames[f], harness, f"{W}x{H} frame {f} offset {offset}")


def test_png_ruler_every_run_and_match_length(enc, harness):
    """Filtered rows with a run of every length 1..300, none cut by a unit: so
    every match length 3..258 and every residual literal count occurs (asserted
    on the NumPy restatement of the tokens); a flat frame beside it has its
    runs cut at every 512-byte unit boundary."""
    W = 342
    ruler = _ruler(W)
    H = ruler.shape[0]
    hist, match_lens, run_lens = _token_histogram(ruler.reshape(H, 3 * W), 3)
    assert match_lens == set(range(3, 259)), sorted(set(range(3, 259)) - match_lens)
    assert set(range(1, 301)) <= run_lens
    assert (hist[257:286] > 0).all()                               # every length symbol
    flat = np.full((H, W, 3), 9, np.uint8)
    _, _, flat_runs = _token_histogram(flat.reshape(H, 3 * W), 3)
    assert {SEG - 3, SEG, 3 * W - 2 * SEG} <= flat_runs            # unit 0 after the first pixel, unit 1, unit 2
    frames = np.stack([ruler, flat, ruler[::-1].copy()])
    blobs = _encode(enc, ("rgb_png",), 3, W, H, rgb=frames)
    for f in range(3):
        _check_png(blobs[f], frames[f], harness, f"ruler frame {f}")


def test_png_code_length_limit_binds(enc, harness):
    """Fibonacci symbol counts: every optimal code is deeper than the 15 bits
    deflate allows, so the length limiter of huff_lengths decides the code."""
    W, H = 171, 236
    fib = _fibonacci_image(W, H)
    hist, _, _ = _token_histogram(fib.reshape(H, 3 * W), 3)
    assert _min_max_depth(hist) > 15, _min_max_depth(hist)
    rng = np.random.default_rng(2)
    frames = np.stack([fib, _noise(rng, H, W)])
    blobs = _encode(enc, ("rgb_png",), 2, W, H, rgb=frames)
    for f in range(2):
        _check_png(blobs[f], frames[f], harness, f"fibonacci frame {f}")


def test_png_all_286_symbols(enc, harness):
    """Every literal, every length symbol and the end-of-block code in one
    frame's code: the ruler's rows above rows of all 256 residual bytes."""
    W = 342
    res = _ruler_residuals(3 * W)
    allb = np.resize(np.arange(256, dtype=np.uint8), (2, 3 * W))
    img = _residuals_to_image(np.concatenate([res, allb])).reshape(-1, W, 3)
    H = img.shape[0]
    hist, _, _ = _token_histogram(img.reshape(H, 3 * W), 3)
    assert (hist > 0).all()
    blobs = _encode(enc, ("rgb_png",), 1, W, H, rgb=img[None])
    _check_png(blobs[0], img, harness, "286 symbols")


# Noise images (np.random.default_rng(seed).integers(0, 256, (H, W, 3))) whose zlib
# stream is 0, 1..3 and 4 bytes past a multiple of 2048: found once with the harness.
IDAT_EDGE = [(337, 4, 7, 0), (337, 4, 3, 1), (337, 4, 8, 3), (337, 4, 15, 4)]   # W, H, seed, zlib length mod 2048


@pytest.mark.parametrize("W,H,seed,mod", IDAT_EDGE)
def test_png_adler_at_the_idat_edge(enc, harness, W, H, seed, mod):
    """The Adler-32 ends an IDAT chunk exactly (0), straddles two chunks
    (1..3) or is a last chunk of its own (4)."""
    img = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    zlen = _harness_zlen(harness, img, W, H)
    assert zlen % 2048 == mod and zlen > 2048, zlen
    other = _noise(np.random.default_rng(seed + 1), H, W)
    blobs = _encode(enc, ("rgb_png",), 2, W, H, rgb=np.stack([img, other]))
    assert _check_png(blobs[0], img, harness, f"idat edge {mod}") == zlen
    assert _idat_sizes(blobs[0])[-1] == (mod or 2048)
    _check_png(blobs[1], other, harness, "idat edge neighbour")


def _u16(depth, s):
    """The quantiser of include/csg_api.h (CSG_FILE_DEPTH16_PNG), restated:
    float32 multiply, float32 add, each rounded once."""
    d = np.asarray(depth, np.float32)
    ok = np.isfinite(d) & (d > 0)
    with np.errstate(over="ignore", invalid="ignore"):
        t = (np.where(ok, d, np.float32(0)).astype(np.float32) * np.float32(s)).astype(np.float32)
        sat = t >= 65535
        v = (np.where(sat, np.float32(0), t).astype(np.float32) + np.float32(0.5)).astype(np.float32).astype(np.uint32)
    return np.where(ok, np.where(sat, 65535, v), 0).astype(np.uint16)


@pytest.mark.parametrize("W", [256, 257, 512])
def test_png_16bit_rows(enc, harness, W):
    """bpp 2 through depth16_png: rows of 512, 514 and 1024 bytes.  Depths k / s
    for chosen samples k: noise, flat, runs of growing length, and 0 / 65535."""
    H, s = 7, 256.0                                                # (k / 256) * 256 is exact in float32
    rng = np.random.default_rng(W)
    ruler = _ruler(W, H, bpp=2).reshape(H, 2 * W).view(">u2").astype(np.uint16)
    want = np.stack([rng.integers(0, 65536, (H, W)).astype(np.uint16), np.full((H, W), 0x0101, np.uint16), ruler,
                     rng.integers(0, 2, (H, W)).astype(np.uint16) * 65535])
    depth = (want.astype(np.float32) / np.float32(s)).astype(np.float32)
    assert np.array_equal(_u16(depth, s), want)
    blobs = _encode(enc, ("depth16_png",), 4, W, H, depth=depth, scale=s)
    for f in range(4):
        _check_png(blobs[f], want[f], harness, f"16-bit {W} frame {f}")


# ---------------------------------------------------------------------------
# depth CSV
# ---------------------------------------------------------------------------
def _csv_pool():
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-7, 5e-7, 4.9999997e-7, 2.0 ** -21, 0.5, 1.0,
                         2.0 ** 40, 2.0 ** 41, 3.4028235e38, -3.4028235e38, 1e20, 1.4e-45, 123.456789,
                         0.0000005, 0.0000015, 0.0000025, 249.99998, 0.5000001, 7.0e15, 16777217.0],
                        np.float32)                                # the list of test_csv_matches_savetxt
    ties = (np.arange(1, 512, 2) / 128.0).astype(np.float32)      # n / 128, n odd: exactly half a unit of the 6th place
    edges = []
    for c in (4294.967296, 2.0 ** 40, 2.0 ** 41, 2.0 ** 64, 2.0 ** 96, 1e-6, 0.5e-6, 1.0, 10.0, 1e9):
        x = np.float32(c)                                          # both sides of the formatter's branch points
        lo = np.nextafter(np.nextafter(x, np.float32(0)), np.float32(0))
        for _ in range(5):
            edges += [lo, -lo]
            lo = np.nextafter(lo, np.float32(np.inf))
    den = np.array([1, 2, 0x7FFFFF, 0x800000, 0x80000001, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7FC00000, 0xFFC00000,
                    0x7F800001, 0xFF800000], np.uint32).view(np.float32)
    rnd = np.random.default_rng(17).integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return np.concatenate([specials, ties, -ties[:16], np.array(edges, np.float32), den, rnd])


def _savetxt(img):
    ref = io.BytesIO()
    np.savetxt(ref, img, fmt="%.6f", delimiter=" ")
    return ref.getvalue()


@pytest.mark.parametrize("W,H", [(1, 300), (63, 5), (64, 5), (65, 130), (129, 67)])
def test_csv_values(enc, W, H):
    """Units of 1, 63, 64, 64 + 1 and 64 + 64 + 1 values; 65x130 is 260 units
    (more than the layout scan's 256 threads).  Frame 0: the value pool (ties,
    branch points, specials, random bit patterns); frame 1: whole rows of
    -FLT_MAX (every unit 64 values of 47 characters, what the wave's text
    buffer is sized for) and of +FLT_MAX in turn; frame 2: the pool reversed;
    frame 3: random bit patterns of this shape."""
    assert "%.6f" % 0.0078125 == "0.007812" and "%.6f" % 0.0234375 == "0.023438"   # half to even
    assert len("%.6f" % float(-FLT_MAX)) == 47
    pool = _csv_pool()
    n = W * H
    rnd = np.random.default_rng(W).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    fmax = np.where(np.arange(H)[:, None] % 2 == 0, -FLT_MAX, FLT_MAX) * np.ones((1, W), np.float32)
    frames = np.stack([np.resize(pool, n), fmax.astype(np.float32).reshape(-1), np.resize(pool[::-1], n), rnd])
    frames = frames.reshape(4, H, W)
    if n >= pool.size:
        assert np.isin(pool.view(np.uint32), frames[0].view(np.uint32)).all()
    blobs = _encode(enc, ("depth_csv",), 4, W, H, depth=frames)
    for f in range(4):
        ref = _savetxt(frames[f])
        assert len(blobs[f]) == len(ref), f"frame {f}"
        if blobs[f] != ref:
            got, exp = blobs[f].split(), ref.split()
            bad = [(i, frames[f].reshape(-1)[i].view(np.uint32), g, e) for i, (g, e) in enumerate(zip(got, exp))
                   if g != e][:5]
            raise AssertionError(f"{W}x{H} frame {f}: (index, bits, got, expected) {bad}")


def test_csv_whole_pool_once(enc):
    """Every value of the pool in one frame (64 wide), whatever the other cases' sizes hold."""
    pool = _csv_pool()
    H = (pool.size + 63) // 64
    img = np.resize(pool, (H, 64))
    blobs = _encode(enc, ("depth_csv",), 1, 64, H, depth=img[None])
    assert blobs[0] == _savetxt(img)


# ---------------------------------------------------------------------------
# point clouds: TXT and PLY
# ---------------------------------------------------------------------------
def _pcd_savetxt(points, rgb):
    p, c = points.reshape(-1, 3), rgb.reshape(-1, 3)
    ok = ~np.isnan(p).any(axis=1)
    ref = io.BytesIO()
    np.savetxt(ref, np.hstack([p[ok], c[ok]]), fmt="%.6f", delimiter=" ", header="x y z r g b", comments="")
    return ref.getvalue()


def _check_clouds(enc, points, rgb, offset=0):
    n, H, W = points.shape[:3]
    blobs = _encode(enc, ("pointcloud_txt", "pointcloud_ply"), n, W, H, rgb=rgb, points=points, offset=offset)
    for f in range(n):
        ref = _pcd_savetxt(points[f], rgb[f])
        assert len(blobs[2 * f]) == len(ref) and blobs[2 * f] == ref, f"frame {f}: txt"
        ref = restate_ply(points[f], rgb[f])
        assert len(blobs[2 * f + 1]) == len(ref) and blobs[2 * f + 1] == ref, f"frame {f}: ply"
    return blobs


@pytest.mark.parametrize("offset", [0, 1])
def test_clouds_validity_and_halves(enc, offset):
    """128 wide (two units per row).  Frame 0: NaN in x only, y only, z only (not
    points), +-inf and -0.0 components (points; PLY copies the bits), units with
    only lanes 0-31 or only lanes 32-63 valid, a unit of 64 lines of -FLT_MAX
    with rgb 255 (each half-wave the 32 longest lines the buffer is sized for),
    rgb of every digit count.  Frame 1: its first 64 pixels hold no point, so
    unit 0 carries the header alone.  Frame 2: no point at all."""
    W, H = 128, 8
    rng = np.random.default_rng(8)
    p = rng.normal(0, 50, (3, H, W, 3)).astype(np.float32)
    c = rng.choice(np.array([0, 9, 10, 99, 100, 255], np.uint8), (3, H, W, 3))
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for k in range(3):                       # row 0: one NaN component, cycling, every other pixel
        p[0, 0, k * 2::6, k] = nan
    p[0, 1, 32:64] = nan                     # unit (1, 0): lanes 0-31 only
    p[0, 1, 64:96] = nan                     # unit (1, 1): lanes 32-63 only
    p[0, 2, 0:64:3, 0] = inf
    p[0, 2, 1:64:3, 1] = -inf
    p[0, 2, 2:64:3, 2] = np.float32(-0.0)
    p[0, 2, 64:, :] = np.float32(-0.0)
    p[0, 3, :64] = -FLT_MAX
    c[0, 3, :64] = 255
    p[0, 3, 64:] = nan                       # ... next to an empty unit
    p[0, 4, :32] = -FLT_MAX                  # the longest lines in lanes 0-31, short ones in 32-63
    c[0, 4, :32] = 255
    p[0, 5, 96:] = FLT_MAX
    p[0, 6] = rng.integers(0, 2 ** 32, (W, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    p[1, 0, :64] = nan
    p[1, 0, 3, 0] = np.float32(1.0)          # ... two numbers do not make a point
    p[1, 0, 3, 2] = np.float32(2.0)
    p[2] = nan
    line = "%.6f %.6f %.6f 255.000000 255.000000 255.000000\n" % ((float(-FLT_MAX),) * 3)
    assert len(line) == 177 and 32 * len(line) + 12 <= 5772            # kPcdBuf
    blobs = _check_clouds(enc, p, c, offset)
    assert blobs[0].count(line.encode()) == 96
    assert blobs[4] == b"x y z r g b\n" and b"element vertex 0\n" in blobs[5]
    ok = ~np.isnan(p[0]).any(axis=-1)
    assert not ok[0, 0] and ok[0, 1] and ok[2, :64].all()       # a NaN component: no point; inf and -0.0: points


def test_clouds_point_counts_across_digit_boundaries(enc):
    """One batch whose frames hold 0, 9, 10, 99, 100 and 1000 points: the PLY
    header's length changes inside the batch."""
    W, H = 40, 26
    counts = [0, 9, 10, 99, 100, 1000]
    rng = np.random.default_rng(4)
    p = np.full((len(counts), H * W, 3), np.nan, np.float32)
    for f, n in enumerate(counts):
        at = rng.choice(H * W, n, replace=False)
        p[f, at] = rng.normal(0, 5, (n, 3)).astype(np.float32)
    c = rng.integers(0, 256, (len(counts), H, W, 3), dtype=np.uint8)
    blobs = _check_clouds(enc, p.reshape(len(counts), H, W, 3), c)
    for f, n in enumerate(counts):
        assert b"element vertex %d\n" % n in blobs[2 * f + 1]
        assert blobs[2 * f].count(b"\n") == n + 1


def test_clouds_odd_width_many_units(enc):
    """65 x 130: 260 units of 64 and 1 pixels, sparse points."""
    W, H = 65, 130
    rng = np.random.default_rng(6)
    p = rng.normal(0, 3000, (2, H, W, 3)).astype(np.float32)
    p[0][rng.random((H, W)) < 0.7] = np.nan
    p[1, :, :64] = np.nan                                          # only the 1-pixel units hold points
    c = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    _check_clouds(enc, p, c, offset=1)


# ---------------------------------------------------------------------------
# depth16 quantiser
# ---------------------------------------------------------------------------
def _depth16_values(s):
    s32 = np.float32(s)
    vals = [np.float32(0.0), np.float32(-0.0), np.float32(-1.0), np.float32(-1e-30), np.float32(1e-45),
            np.float32(1e-39), np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan)]
    centres = [(k + 0.5) / s for k in (0, 1, 2, 3, 127, 128, 255, 256, 1000, 32767, 32768, 65533, 65534)]
    centres += [65534.5 / s, 65535.0 / s, 65536.0 / s]
    with np.errstate(over="ignore"):
        for c in centres:
            x = np.float32(c)
            lo = np.nextafter(np.nextafter(x, np.float32(0)), np.float32(0))
            for _ in range(5):                                     # c's two float32 neighbours on either side
                vals.append(lo)
                lo = np.nextafter(lo, np.float32(np.inf))
        vals += [FLT_MAX, np.float32(FLT_MAX / s32) if s > 1 else FLT_MAX, np.float32(1e10), np.float32(3e38)]
    return np.array(vals, np.float32)


@pytest.mark.parametrize("s", [250.0, 1000.0, 0.001, 1e30])
def test_depth16_quantiser(enc, s):
    """Half-count inputs and their neighbours, the saturation edge, d * s
    overflowing to inf, zeros, negatives, denormals, inf and nan; as a 3x3
    frame (odd pixel count: the tail store), a 3x3x3 batch and a batch of
    3x3 frames that holds every value."""
    vals = _depth16_values(s)
    exp = _u16(vals, s)
    assert exp[:9].tolist() == [0] * 9                             # zeros, negatives, denormals, inf, nan: "no hit"
    if s == 1e30:
        with np.errstate(over="ignore"):
            assert np.isinf(vals[np.isfinite(vals)] * np.float32(s)).any()
    assert {0, 1, 2, 65534, 65535} <= set(exp.tolist())
    F = (vals.size + 8) // 9
    F += 1 - F % 2                                                 # odd: 9 F pixels is odd too
    full = np.resize(vals, (F, 3, 3))
    for d in (full[:1], full[1:4], full):
        n = d.shape[0]
        blobs = _encode(enc, ("depth16_png",), n, 3, 3, depth=d, scale=s)
        for f in range(n):
            got, want = decode_png16(blobs[f]), _u16(d[f], s)
            assert np.array_equal(got, want), (s, f, d[f].view(np.uint32), got, want)


# ---------------------------------------------------------------------------
# depth statistics
# ---------------------------------------------------------------------------
def _ref_stats(d):
    d = d.reshape(-1)
    ok = np.isfinite(d) & (d > 0)
    v = d[ok]
    return (int(ok.sum()), int((d == 0).sum()), int(np.isinf(d).sum()), math.fsum(float(x) for x in v),
            float(v.min()) if v.size else 0.0, float(v.max()) if v.size else 0.0)


@pytest.mark.parametrize("W,H", [(1, 1), (10, 10), (64, 64)])
def test_depth_stats(enc, W, H):
    """Frames of 1, 100 and 4096 pixels, all smaller than the 64 x 256 grid of
    k_depth_stats (blocks without an element): +0, -0, negative, NaN, +-inf and
    denormal pixels; one frame without a valid pixel."""
    n = W * H
    rng = np.random.default_rng(n)
    junk = np.array([0.0, -0.0, -1.0, -1e-40, np.nan, np.inf, -np.inf, 1e-40, 1.4e-45, -3e38], np.float32)
    frames = [np.where(rng.random(n) < 0.5, rng.choice(junk, n), rng.uniform(0.5, 250.0, n).astype(np.float32)),
              rng.choice(junk[:7], n),                             # no valid pixel
              rng.choice(junk, n),
              np.full(n, 1e-40, np.float32),                       # denormals only: valid
              rng.uniform(1e-3, 3e38, n).astype(np.float32)]
    if n == 1:                                                     # one pixel of every class
        frames += [np.array([x], np.float32) for x in (0.0, -0.0, -2.0, np.nan, np.inf, -np.inf, 1e-42, 7.5)]
    d = np.stack(frames).astype(np.float32).reshape(-1, H, W)
    _, stats = _encode(enc, 0, d.shape[0], W, H, depth=d, stats=True)
    assert stats.shape == (d.shape[0], 6)
    for f in range(d.shape[0]):
        valid, zero, inf, total, mn, mx = _ref_stats(d[f])
        got = stats[f]
        assert (got[0], got[1], got[2], got[4], got[5]) == (valid, zero, inf, mn, mx), (f, got, _ref_stats(d[f]))
        assert abs(got[3] - total) <= valid * 2.0 ** -53 * total, (f, got[3], total)
    assert _ref_stats(d[1])[0] == 0 and stats[1][3] == 0.0


def test_depth_stats_with_files(enc):
    """depth_stats beside a file kind, and still written when the files do not fit."""
    rng = np.random.default_rng(3)
    d = rng.uniform(-5, 250, (3, 9, 33)).astype(np.float32)
    blobs, stats = _encode(enc, ("depth_csv",), 3, 33, 9, depth=d, stats=True)
    blobs2, stats2 = _encode(enc, ("depth_csv",), 3, 33, 9, depth=d, stats=True, cap=100)
    assert blobs == blobs2 == [_savetxt(d[f]) for f in range(3)]
    assert np.array_equal(stats, stats2) and [int(x) for x in stats[:, 0]] == [_ref_stats(d[f])[0] for f in range(3)]


# ---------------------------------------------------------------------------
# all kinds in one call; errors
# ---------------------------------------------------------------------------
def test_all_kinds_in_one_call(enc, harness):
    """Six kinds, three frames, 65 x 9, every uint8 image off alignment: slot
    order, three PNG kinds staged together, and each file equal to the file of
    a call for its kind alone."""
    W, H, n = 65, 9, 3
    rng = np.random.default_rng(12)
    rgb, dvis = _noise(rng, n * H, W).reshape(n, H, W, 3), np.repeat(_noise(rng, n * H, W // 5 + 1), 5, axis=1)
    dvis = np.ascontiguousarray(dvis[:, :W]).reshape(n, H, W, 3)
    depth = rng.uniform(0.0, 300.0, (n, H, W)).astype(np.float32)
    depth[rng.random((n, H, W)) < 0.2] = np.inf
    pts = rng.normal(0, 20, (n, H, W, 3)).astype(np.float32)
    pts[np.isinf(depth)] = np.nan
    src = dict(rgb=rgb, depth_vis=dvis, depth=depth, points=pts)
    blobs = _encode(enc, ALL_KINDS, n, W, H, offset=1, **src)
    assert len(blobs) == 6 * n
    for f in range(n):
        _check_png(blobs[6 * f], rgb[f], harness, f"rgb {f}")
        assert blobs[6 * f + 1] == _savetxt(depth[f])
        _check_png(blobs[6 * f + 2], dvis[f], harness, f"depth_vis {f}")
        assert blobs[6 * f + 3] == _pcd_savetxt(pts[f], rgb[f])
        assert blobs[6 * f + 4] == restate_ply(pts[f], rgb[f])
        _check_png(blobs[6 * f + 5], _u16(depth[f], 250.0), harness, f"depth16 {f}")
    for k, kind in enumerate(ALL_KINDS):
        assert _encode(enc, (kind,), n, W, H, **src) == blobs[k::6], kind


def test_errors(enc):
    from constructionsceneposeestimation_amd._lib import CsgError
    rng = np.random.default_rng(0)
    rgb = _noise(rng, 4, 5)[None]
    depth = rng.uniform(1, 2, (1, 4, 5)).astype(np.float32)
    with pytest.raises(CsgError, match="need rgb"):
        _encode(enc, ("rgb_png",), 1, 5, 4)                        # a missing pointer
    with pytest.raises(CsgError, match="need points"):
        _encode(enc, ("pointcloud_ply",), 1, 5, 4, rgb=rgb)
    with pytest.raises(CsgError, match="depth_vis"):
        _encode(enc, ("depth_png",), 1, 5, 4, rgb=rgb)
    with pytest.raises(CsgError, match="need depth"):
        _encode(enc, 0, 1, 5, 4, rgb=rgb, stats=True)
    with pytest.raises(CsgError, match="frame size"):
        _encode(enc, ("rgb_png",), 1, 0, 4, rgb=rgb)               # W = 0
    with pytest.raises(CsgError, match="frame size"):
        _encode(enc, ("rgb_png",), 1, 5, 0, rgb=rgb)
    with pytest.raises(CsgError, match="unknown file kinds"):
        _encode(enc, 64, 1, 5, 4, rgb=rgb)                         # an unknown kind
    with pytest.raises(CsgError, match="no frames"):
        _encode(enc, ("rgb_png",), 0, 5, 4, rgb=rgb)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(CsgError, match="depth16_counts_per_metre"):
            _encode(enc, ("depth16_png",), 1, 5, 4, depth=depth, scale=bad)
    # the context still works, and a too-small buffer is CSG_ERR_CAPACITY, then csg_copy_files
    small = _encode(enc, ("rgb_png", "depth_csv"), 1, 5, 4, rgb=rgb, depth=depth, cap=10)
    assert small == _encode(enc, ("rgb_png", "depth_csv"), 1, 5, 4, rgb=rgb, depth=depth)
    assert np.array_equal(decode_png(small[0]), rgb[0]) and small[1] == _savetxt(depth[0])
