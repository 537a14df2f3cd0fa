"""What the JPEG tests share (tests/test_jpeg.py, tests/test_gpu_jpeg.py): the
image set, the list of cases, the reference files of ``writers.jpeg_bytes``
(each made once), and a small baseline decoder that takes a file back to its
quantised coefficients and checks the framing on the way."""
import functools

import numpy as np

from constructionsceneposeestimation_amd import writers

# (W, H): edge extension in both axes, one MCU, odd chroma sizes, MCU rows of one MCU; 16 x 80 has ten
# restart intervals in 4:4:4, so RSTm wraps
SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 9), (33, 31), (67, 35), (96, 64), (16, 80)]
KINDS = ["black", "white", "red", "green", "blue", "checker", "noise", "hramp", "vramp", "rendered"]
QUALITIES = [1, 50, 75, 95, 100]
SUBSAMPLINGS = ["444", "420"]


@functools.lru_cache(maxsize=None)
def make_image(kind: str, W: int, H: int) -> np.ndarray:
    y, x = np.mgrid[0:H, 0:W]
    img = np.zeros((H, W, 3), np.uint8)
    if kind == "black":
        pass
    elif kind == "white":
        img[:] = 255
    elif kind in ("red", "green", "blue"):
        img[..., ("red", "green", "blue").index(kind)] = 255
    elif kind == "checker":   # 0 / 255 at one-pixel pitch: the largest DCT amplitudes
        img[:] = (((x + y) & 1) * 255)[..., None]
    elif kind == "noise":
        img = np.random.default_rng(W * 10007 + H).integers(0, 256, (H, W, 3), dtype=np.uint8)
    elif kind == "hramp":
        img[:] = (x * 255 // max(W - 1, 1))[..., None]
    elif kind == "vramp":
        img[:] = (y * 255 // max(H - 1, 1))[..., None]
    elif kind == "rendered":   # smooth shading with hard edges: a lit sphere and a box over a graded ground
        u, v = (x + 0.5) / W - 0.5, (y + 0.5) / H - 0.5
        img[..., 0] = 40 + 60 * (v + 0.5)
        img[..., 1] = 70 + 90 * (v + 0.5)
        img[..., 2] = 120 + 100 * (0.5 - v)
        r2 = (u + 0.1) ** 2 + (v * H / W) ** 2
        inside = r2 < 0.09
        shade = np.clip(1.0 - r2 / 0.09, 0, 1) ** 0.5 * np.clip(0.6 - 1.5 * u - 1.0 * v, 0.15, 1.0)
        for c, base in enumerate((230, 120, 40)):
            img[..., c] = np.where(inside, np.clip(base * shade + 12, 0, 255), img[..., c])
        box = (u > 0.2) & (u < 0.42) & (v > -0.3) & (v < 0.35)
        for c, base in enumerate((60, 180, 90)):
            img[..., c] = np.where(box, np.clip(base * (0.55 + 0.9 * (u - 0.2)), 0, 255), img[..., c])
    else:
        raise KeyError(kind)
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def reference(kind: str, W: int, H: int, quality: int, subsampling: str) -> bytes:
    """``writers.jpeg_bytes`` of one case, made once per process."""
    return writers.jpeg_bytes(make_image(kind, W, H), quality, subsampling)


def _huffman_table(bits, vals):
    """A DHT segment's table as a lookup by the next 16 bits of the stream: (symbol, code length) arrays; length
    0 marks 16 bits that begin no code."""
    sym, length = np.zeros(65536, np.int32), np.zeros(65536, np.int32)
    code, k = 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            sym[code << (16 - n):(code + 1) << (16 - n)] = vals[k]
            length[code << (16 - n):(code + 1) << (16 - n)] = n
            code += 1
            k += 1
        code <<= 1
    return sym.tolist(), length.tolist()


def parse_header(jpg: bytes) -> dict:
    """The marker segments from SOI through the SOS header: their order, the
    tables, the frame's numbers, and ``data``, the offset of the entropy data."""
    assert jpg[:2] == b"\xff\xd8"
    p, out = 2, {"markers": [0xD8], "q": {}, "huff": {}, "dri": 0}
    while True:
        assert jpg[p] == 0xFF, p
        m, n = jpg[p + 1], jpg[p + 2] * 256 + jpg[p + 3]
        seg = jpg[p + 4:p + 2 + n]
        out["markers"].append(m)
        if m == 0xDB:
            out["q"][seg[0]] = list(seg[1:65])
        elif m == 0xC0:
            out["H"], out["W"] = seg[1] * 256 + seg[2], seg[3] * 256 + seg[4]
            out["sampling"] = [seg[7 + 3 * c] for c in range(seg[5])]
        elif m == 0xC4:
            out["huff"][seg[0]] = _huffman_table(seg[1:17], seg[17:])
        elif m == 0xDD:
            out["dri"] = seg[0] * 256 + seg[1]
        p += 2 + n
        if m == 0xDA:
            out["data"] = p
            return out


def decode_coefficients(jpg: bytes):
    """Back to the quantised coefficients of a baseline file with one restart
    interval per MCU row: ``(header, rows, stuffed)`` with ``rows[r]`` a list
    of ``(component, zz[64])`` in scan order (DC absolute) and ``stuffed`` the
    number of FF 00 pairs.  Asserts the framing: RSTm in order behind every
    interval but the last, 1-bit padding of less than a byte, nothing between
    the last interval and EOI."""
    h = parse_header(jpg)
    sub = h["sampling"][0] == 0x22
    order = [0, 0, 0, 0, 1, 2] if sub else [0, 1, 2]
    m = 16 if sub else 8
    mx, my = -(-h["W"] // m), -(-h["H"] // m)
    assert h["dri"] == mx and jpg[-2:] == b"\xff\xd9"
    data = jpg[h["data"]:-2]
    rows, pos, stuffed = [], 0, 0
    for r in range(my):
        e = pos
        while e < len(data) and not (data[e] == 0xFF and data[e + 1] != 0):
            e += 2 if data[e] == 0xFF else 1
        stuffed += data[pos:e].count(b"\xff\x00")
        chunk = data[pos:e].replace(b"\xff\x00", b"\xff")
        if r + 1 < my:
            assert data[e:e + 2] == bytes([0xFF, 0xD0 + (r & 7)]), (r, data[e:e + 2])
            pos = e + 2
        else:
            assert e == len(data), "bytes behind the last interval"
        nb, at = len(chunk) * 8, 0
        word = int.from_bytes(chunk, "big") << 16       # (16 bits of room for the last symbol's lookup)

        def take(n):
            nonlocal at
            assert at + n <= nb, "interval ends inside a symbol"
            at += n
            return (word >> (nb + 16 - at)) & ((1 << n) - 1)

        def symbol(t):
            nonlocal at
            peek = (word >> (nb - at)) & 0xFFFF
            n = t[1][peek]
            assert n and at + n <= nb, "no such code"
            at += n
            return t[0][peek]

        def extend(s):
            if s == 0:
                return 0
            v = take(s)
            return v if v >> (s - 1) else v - (1 << s) + 1

        pred, blocks = [0, 0, 0], []
        for _ in range(mx):
            for c in order:
                zz = [0] * 64
                pred[c] += extend(symbol(h["huff"][min(c, 1)]))
                zz[0] = pred[c]
                i = 1
                while i < 64:
                    rs = symbol(h["huff"][0x10 | min(c, 1)])
                    if rs == 0:
                        break
                    if rs == 0xF0:
                        i += 16
                        continue
                    i += rs >> 4
                    assert i < 64
                    zz[i] = extend(rs & 15)
                    i += 1
                blocks.append((c, zz))
        rest = nb - at
        assert 0 <= rest < 8 and take(rest) == (1 << rest) - 1, "padding"
        rows.append(blocks)
    return h, rows, stuffed
