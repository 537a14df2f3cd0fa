"""The kernels against the exact integer coverage reference of
tests/raster_exact.py: ids, label stats and label coverage of every family's
frames equal what Python integers say (no oracle involved), every output is
bit-exact against the oracle besides, and csg_amodal_spans' per-label masks and
stats equal each layer's exact mask.  All frames of a size are one batch; the
CPU side of the same frames is tests/test_raster_exact.py."""
import numpy as np
import pytest

from tests import raster_exact as rx
from tests.test_gpu_amodal_rle import _decode, _run
from tests.test_gpu_parity import _assert_extra, _assert_same

pytestmark = pytest.mark.gpu
SIZES = [pytest.param(s, id=f"{s[0]}x{s[1]}") for s in rx.SIZES]
WANT = ("rgb", "instance", "depth", "normals", "points", "stats", "covered")


@pytest.fixture(scope="module", params=SIZES)
def run(request):
    """One context per size: the batch rendered once, and the amodal pass on the same frames."""
    from constructionsceneposeestimation_amd.renderer import Renderer, make_frames
    W, H = request.param
    b = rx.batch(W, H)
    n = len(b["frames"])
    fr = make_frames(b["V"], b["P"], list(range(n)), list(range(n)))
    # vertical runs of every layer's exact mask: the span records the amodal pass needs at most
    runs = max(int((np.diff(np.pad(f["masks"], ((0, 0), (1, 0), (0, 0))).astype(np.int8), axis=1) == 1).sum())
               for f in b["frames"])
    cap = runs + 64
    with Renderer(b["scene"], W, H, max_frames=n) as r:
        assert r.n_labels == r._n_inst_labels == rx.N_LABELS
        for f in range(n):
            r.set_instance_transforms(f, b["models"][f])
        gpu = r.render(fr, want=WANT)
        amodal = _run(r, fr, cap)
    return dict(W=W, H=H, b=b, gpu=gpu, amodal=amodal, cap=cap)


def test_ids_stats_and_coverage_equal_the_integer_reference(run):
    gpu = run["gpu"]
    for f, fr in enumerate(run["b"]["frames"]):
        what = f'{run["W"]}x{run["H"]} {fr["family"]}/{fr["order"]}'
        bad = np.argwhere(gpu["instance"][f] != fr["ids"])
        assert len(bad) == 0, f"{what}: {len(bad)} ids differ from the exact ones, first at (y, x) {bad[:5].tolist()}"
        assert np.array_equal(gpu["inst_stats"][f], fr["inst_stats"]), what
        assert np.array_equal(gpu["label_covered"][f], fr["covered"]), what
        assert np.isinf(gpu["depth"][f][fr["ids"] < 0]).all(), what


def test_every_output_is_bit_exact_against_the_oracle(run):
    gpu, ora = run["gpu"], rx.oracle_frames(run["W"], run["H"])
    for f, fr in enumerate(run["b"]["frames"]):
        _assert_same(gpu, ora[f], f)
        _assert_extra(gpu, ora[f], f)
        what = f'{fr["family"]}/{fr["order"]}'
        assert np.array_equal(gpu["inst_stats"][f], ora[f]["inst_stats"]), what
        assert np.array_equal(gpu["label_covered"][f], ora[f]["label_covered"]), what


def test_amodal_spans_equal_each_layers_exact_mask(run):
    W, H = run["W"], run["H"]
    off, sp, st = run["amodal"]
    for f, fr in enumerate(run["b"]["frames"]):
        what = f'{W}x{H} {fr["family"]}/{fr["order"]}'
        assert int(off[f, -1]) <= run["cap"], what
        assert np.array_equal(st[f], fr["amodal_stats"]), what
        for l in range(rx.N_LABELS):
            got = _decode(off[f], sp[f], l, H, W)
            bad = np.argwhere(got != fr["masks"][l])
            assert len(bad) == 0, f"{what} layer {l}: {len(bad)} pixels differ, first at (y, x) {bad[:5].tolist()}"
