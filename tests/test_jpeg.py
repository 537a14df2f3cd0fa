"""CPU tests of the JPEG format of csg_encode_jpeg:
``writers.jpeg_bytes``, the NumPy statement of the format, and
tests/jpeg_host.cpp, a one-thread encoder built from the kernels' own format
header (csrc/csg_jpeg.h; also built with AddressSanitizer and UBSan and run as
a program), must write the same bytes; the header segments must equal
Pillow's; the integer DCT must lie within 0.5 of the exact one; the coded
coefficients must be the float64 chain's, rounding ties apart; Pillow must
decode every file; and the files must be as good and as small as Pillow's
within measured margins.

The image set, the cases and the decoder are in tests/jpeg_cases.py."""
import io
import os
import subprocess
import warnings

import numpy as np
import pytest

from constructionsceneposeestimation_amd import writers
from tests import jpeg_cases as jc

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(k, W, H, q, ss) for (W, H) in jc.SIZES for k in jc.KINDS for q in jc.QUALITIES for ss in jc.SUBSAMPLINGS]

# Fidelity against Pillow's own file of the same image, quality and sampling (test_fidelity): the worst
# gaps measured with writers.jpeg_bytes over the image set, rounded up to the next 0.05 dB and 0.5 %.
PSNR_MARGIN_DB = 0.50      # worst measured 0.476 dB (8 x 8 noise, quality 1, 4:2:0)
SIZE_MARGIN = 0.020        # worst measured 1.80 % (8 x 8 noise, quality 50, 4:2:0: 679 against 667 bytes)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """jpeg_host, plain and sanitised, each run once over every case (--list): {program: {case: file bytes}}."""
    d = tmp_path_factory.mktemp("jpeg")
    src = os.path.join(HERE, "jpeg_host.cpp")
    exe, san = str(d / "jpeg_host"), str(d / "jpeg_host_san")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", exe], check=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", src, "-o", san], check=True)
    for (W, H) in jc.SIZES:
        for k in jc.KINDS:
            jc.make_image(k, W, H).tofile(str(d / f"{k}_{W}x{H}.raw"))
    out = {}
    for prog in (exe, san):
        name = os.path.basename(prog)
        with open(d / f"{name}.txt", "w") as fh:
            for k, W, H, q, ss in CASES:
                fh.write(f"{W} {H} {q} {writers.JPEG_SUBSAMPLING[ss]} {d / f'{k}_{W}x{H}.raw'} "
                         f"{d / f'{name}_{k}_{W}x{H}_{q}_{ss}.jpg'}\n")
        subprocess.run([prog, "--list", str(d / f"{name}.txt")], check=True)
        out[name] = {}
        for c in CASES:
            k, W, H, q, ss = c
            with open(d / f"{name}_{k}_{W}x{H}_{q}_{ss}.jpg", "rb") as fh:
                out[name][c] = fh.read()
    return exe, san, d, out


@pytest.mark.parametrize("W,H", jc.SIZES)
def test_host_encoder_equals_python(harness, W, H):
    _, _, _, files = harness
    for c in CASES:
        if c[1:3] == (W, H):
            want = jc.reference(*c)
            assert files["jpeg_host"][c] == want, c
            assert files["jpeg_host_san"][c] == want, c


def test_host_encoder_as_a_single_call(harness):
    exe, san, d, _ = harness
    for prog in (exe, san):
        dst = str(d / "single.jpg")
        subprocess.run([prog, "67", "35", "95", "1", str(d / "rendered_67x35.raw"), dst], check=True)
        with open(dst, "rb") as fh:
            assert fh.read() == jc.reference("rendered", 67, 35, 95, "420")
        assert subprocess.run([prog, "67", "35", "101", "1", str(d / "rendered_67x35.raw"), dst]).returncode == 2


def test_quantiser_without_division(harness):
    """csg_jpeg.h's quantise multiplies by a reciprocal: it equals the division it stands for, for every
    quantiser and every quotient at the ends of its range (jpeg_host --quantiser, also sanitised)."""
    exe, san, _, _ = harness
    for prog in (exe, san):
        subprocess.run([prog, "--quantiser"], check=True)
    a, q = np.arange(2048)[:, None], np.arange(1, 256)[None, :]
    assert np.array_equal((a * ((2 ** 20 + q - 1) // q)) >> 20, a // q)


def pillow_bytes(img, q, ss):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=q, subsampling=0 if ss == "444" else 2, restart_marker_rows=1)
    return b.getvalue()


@pytest.mark.parametrize("W,H", jc.SIZES)
def test_headers_equal_pillows(W, H):
    """Every byte through the SOS header: the markers SOI, APP0, DQT x 2, SOF0, DHT x 4, DRI, SOS with Pillow's
    tables and lengths, for every quality and both samplings."""
    pytest.importorskip("PIL")
    img = jc.make_image("rendered", W, H)
    for q in jc.QUALITIES:
        for ss in jc.SUBSAMPLINGS:
            ours, theirs = jc.reference("rendered", W, H, q, ss), pillow_bytes(img, q, ss)
            h = jc.parse_header(theirs)
            assert h["markers"] == [0xD8, 0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
            assert h["data"] == writers.JPEG_HEAD_BYTES
            assert ours[:h["data"]] == theirs[:h["data"]], (q, ss)
            assert writers.jpeg_header(W, H, q, ss) == ours[:writers.JPEG_HEAD_BYTES]
            assert h["q"][0] == writers.jpeg_quant_tables(q)[0].tolist()
            assert h["q"][1] == writers.jpeg_quant_tables(q)[1].tolist()


def dct_blocks():
    """10,000 random blocks and the extreme ones: every sample at -128 or 127, both checkerboards and the
    stripes at one-sample pitch, random signs at full amplitude, and an impulse of either sign at each of the
    64 positions over either flat level."""
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:8, 0:8]
    blocks = [rng.integers(-128, 128, (10000, 8, 8))]
    flat = [np.full((8, 8), -128), np.full((8, 8), 127), np.zeros((8, 8), int)]
    pat = [np.where((x + y) & 1, 127, -128), np.where((x + y) & 1, -128, 127), np.where(x & 1, 127, -128),
           np.where(y & 1, 127, -128), np.where(x & 1, -128, 127), np.where(y & 1, -128, 127)]
    signs = np.where(rng.integers(0, 2, (500, 8, 8)) == 1, 127, -128)
    imp = []
    for p in range(64):
        for base, peak in ((-128, 127), (127, -128), (0, 127), (0, -128)):
            b = np.full(64, base)
            b[p] = peak
            imp.append(b.reshape(8, 8))
    return np.concatenate([blocks[0], np.stack(flat + pat + imp), signs]).astype(np.int64)


def test_dct_within_half_of_the_exact_transform(harness):
    """|F' / 2^20 - dctn(f, norm='ortho')| <= 0.5 on every coefficient of every block (the header derives
    0.2), through the Python statement and through jpeg_host --dct; the two agree exactly."""
    from scipy.fft import dctn
    exe, san, d, _ = harness
    f = dct_blocks()
    exact = dctn(f.astype(np.float64), axes=(1, 2), norm="ortho")
    py = writers.jpeg_fdct(f)
    f.astype("<i4").tofile(str(d / "dct_in.i32"))
    for prog in (exe, san):
        subprocess.run([prog, "--dct", str(d / "dct_in.i32"), str(d / "dct_out.i32")], check=True)
        assert np.array_equal(np.fromfile(str(d / "dct_out.i32"), "<i4").reshape(-1, 8, 8), py), prog
    err = np.abs(py / float(1 << writers.JPEG_DCT_SHIFT) - exact)
    print(f"integer DCT: worst error {err.max():.4f} over {err.size} coefficients")
    assert err.max() <= 0.5
    assert err.max() <= 0.2            # the bound csrc/csg_jpeg.h derives for these fixed-point widths
    assert np.abs(py).max() < 2 ** 31  # int32 holds every result


def luma_source(W, H, m, r, k):
    """jpg::luma_source: the block of a 4:2:0 MCU whose DC an empty luminance block k repeats (k itself: not empty)."""
    col, row = m * 16 + 8 < W, r * 16 + 8 < H
    s1 = 1 if col else 0
    if k == 1:
        return s1
    if k >= 2 and not row:
        return s1
    return 2 if k == 3 and not col else k


@pytest.mark.parametrize("W,H", jc.SIZES)
def test_coefficients_are_the_float64_chains(W, H):
    """The entropy data of writers.jpeg_bytes decoded back: each coefficient equals round_half_away(coef / q)
    of the float64 DCT of the same integer samples, or differs by 1 where the exact quotient lies within
    0.5 / q of a tie.  Nothing else may differ.  An empty 4:2:0 luminance block repeats its source's DC."""
    from scipy.fft import dctn
    for k in jc.KINDS:
        img = jc.make_image(k, W, H)
        for ss in jc.SUBSAMPLINGS:
            samples, comp = writers.jpeg_samples(img, ss)
            exact = dctn(samples.astype(np.float64), axes=(2, 3), norm="ortho").reshape(*samples.shape[:2], 64)
            exact = exact[..., writers.JPEG_ZIGZAG]
            for q in jc.QUALITIES:
                qt = writers.jpeg_quant_tables(q)[np.minimum(comp, 1)].astype(np.float64)
                quot = exact / qt
                want = np.sign(quot) * np.floor(np.abs(quot) + 0.5)
                near_tie = np.abs(np.abs(quot) - np.floor(np.abs(quot)) - 0.5) <= 0.5 / qt
                h, rows, _ = jc.decode_coefficients(jc.reference(k, W, H, q, ss))
                assert (h["W"], h["H"]) == (W, H)
                got = np.array([[zz for _, zz in row] for row in rows])
                assert [c for c, _ in rows[0]] == comp.tolist()
                for r in range(got.shape[0]):
                    for j in range(got.shape[1]):
                        m, kk = divmod(j, 6)
                        src = luma_source(W, H, m, r, kk) if ss == "420" and kk < 4 else kk
                        if src != kk:
                            assert got[r, j, 0] == got[r, m * 6 + src, 0] and not got[r, j, 1:].any(), (k, q, ss, r, j)
                            continue
                        diff = np.abs(got[r, j] - want[r, j])
                        assert ((diff == 0) | ((diff == 1) & near_tie[r, j])).all(), (k, q, ss, r, j)


def test_restart_markers_wrap_and_stuffing_is_exercised():
    h, rows, _ = jc.decode_coefficients(jc.reference("noise", 16, 80, 95, "444"))     # the decoder checks RSTm's order
    assert len(rows) == 10
    data = jc.reference("noise", 16, 80, 95, "444")[h["data"]:]
    assert [data[i + 1] for i in range(len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7] == [
        0xD0 + (r & 7) for r in range(9)]
    jpg = jc.reference("noise", 96, 64, 100, "444")
    h, rows, stuffed = jc.decode_coefficients(jpg)
    assert stuffed > 0 and jpg[h["data"]:].count(b"\xff\x00") == stuffed


def psnr(a, b):
    mse = ((a.astype(np.float64) - b) ** 2).mean()
    return np.inf if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


@pytest.mark.parametrize("W,H", jc.SIZES)
def test_pillow_decodes_and_fidelity(W, H):
    """Pillow opens every file with the right size and mode and without a truncation warning, and against
    Pillow's own file of the same image, quality and sampling (restart_marker_rows=1, no optimise):

      size:  ours <= Pillow's * (1 + s) for every case, s = 2.0 % (worst measured 1.80 %);
      PSNR:  ours >= Pillow's - m for every non-degenerate case, m = 0.50 dB (worst measured 0.476 dB).

    Degenerate for the PSNR are the cases where it says nothing about the arithmetic: a decode that is exact
    on either side (infinite PSNR: the flat images, ramps and checkerboards at high quality), and images of
    fewer than 64 pixels (1 x 1, 7 x 5: less than one block of samples, most of every block is edge
    extension that the error is not measured on, and the two encoders differ only in which way coefficients
    near a tie round -- measured there: 1.31 dB behind at 7 x 5 'rendered' quality 100 4:4:4 with byte-equal
    size, 1.19 dB at 7 x 5 'checker' quality 95, and 1.22 dB ahead at 7 x 5 'noise' quality 100).  Tables, layout and
    Huffman codes are Pillow's, so only the rounding of colour, chroma mean and DCT can differ; a gap above
    0.5 dB or 3 % would mean wrong arithmetic."""
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageFile
    assert ImageFile.LOAD_TRUNCATED_IMAGES is False
    worst_m, worst_s = -np.inf, -np.inf
    for c in CASES:
        if c[1:3] != (W, H):
            continue
        k, _, _, q, ss = c
        img, ours = jc.make_image(k, W, H), jc.reference(*c)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            im = Image.open(io.BytesIO(ours))
            assert im.size == (W, H) and im.mode == "RGB" and im.format == "JPEG", c
            dec = np.asarray(im.convert("RGB"))
        theirs = pillow_bytes(img, q, ss)
        ref = np.asarray(Image.open(io.BytesIO(theirs)).convert("RGB"))
        gap_s = len(ours) / len(theirs) - 1.0
        worst_s = max(worst_s, gap_s)
        assert len(ours) <= len(theirs) * (1.0 + SIZE_MARGIN), (c, len(ours), len(theirs))
        p_ours, p_theirs = psnr(dec, img), psnr(ref, img)
        if np.isinf(p_ours) or np.isinf(p_theirs) or W * H < 64:
            continue
        worst_m = max(worst_m, p_theirs - p_ours)
        assert p_ours >= p_theirs - PSNR_MARGIN_DB, (c, p_ours, p_theirs)
    print(f"{W} x {H}: worst PSNR gap {worst_m:.3f} dB, worst size gap {100 * worst_s:.2f} %")


def test_argument_errors():
    img = np.zeros((5, 7, 3), np.uint8)
    for q in (0, 101):
        with pytest.raises(ValueError):
            writers.jpeg_bytes(img, q)
    with pytest.raises(TypeError):
        writers.jpeg_bytes(img.astype(np.int32))
    for bad in (np.zeros((5, 7), np.uint8), np.zeros((5, 7, 4), np.uint8), np.zeros((0, 7, 3), np.uint8)):
        with pytest.raises(ValueError):
            writers.jpeg_bytes(bad)
    with pytest.raises(ValueError):
        writers.jpeg_bytes(img, 95, "422")
    assert writers.jpeg_bytes(img, 95, "420") == writers.jpeg_bytes(img)     # the defaults


def test_generator_knows_the_output():
    from constructionsceneposeestimation_amd import _lib
    from constructionsceneposeestimation_amd.generate import OUTPUTS, REFERENCE_OUTPUTS, file_path, parse_outputs
    assert parse_outputs("rgb_jpg") == ("rgb_jpg",)
    assert parse_outputs("rgb,rgb_jpg,mask_rle") == ("rgb", "rgb_jpg", "mask_rle")
    assert "rgb_jpg" in OUTPUTS and "rgb_jpg" not in REFERENCE_OUTPUTS and parse_outputs("all") == OUTPUTS
    with pytest.raises(ValueError):
        parse_outputs("rgb,jpeg")
    assert file_path("/run", "rgb_jpg", 7) == "/run/rgb/rgb_000007.jpg"
    assert _lib.ABI_VERSION == 14 and "csg_encode_jpeg" in _lib.EXPORTED
    assert _lib.JPEG_SUBSAMPLING == writers.JPEG_SUBSAMPLING
