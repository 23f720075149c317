"""ops.cell_stats (csrc/cellprops.hip), Evaluator.measure_cells and Evaluator.evaluate_measurements against the
plain-loop restatement of tests/_cellprops_ref.py.  Every table is an integer table: every comparison is
np.array_equal."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _cellprops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# test_gpu_pairs.py's shapes, then the edges of a wave's 256-pixel chunk of a row: exact, one short, two chunks and one
SHAPES = [(1, 1), (1, 300), (2, 65), (37, 131), (129, 257), (3, 256), (3, 255), (2, 513)]
PATTERNS = ["background", "one id", "rectangles", "noise", "out of range"]


def _plane(pattern, h, w):
    """(ids int64 [h, w], n)"""
    if pattern == "background":
        return np.zeros((h, w), np.int64), 3
    if pattern == "one id":  # whole-wave runs; every row is a run of its own
        return np.full((h, w), 2, np.int64), 2
    if pattern == "rectangles":
        return R.rectangles(h, w), 3
    if pattern == "noise":
        return R.noise(h, w, 50, h * 1000 + w), 50
    ids = R.noise(h, w, 9, h * 1000 + w + 1)  # ids 6..9 lie above n = 5; every seventh pixel is negative
    ids.reshape(-1)[::7] = -1 - (np.arange(ids.size)[::7] % 3)
    return ids, 5


def _dev(a, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _check(ids, n, image=None, dtype=torch.int64, img_dev=None):
    """ops.cell_stats on the device against the restatement; returns the device result."""
    from eunet import ops
    ids = np.asarray(ids)
    got = ops.cell_stats(_dev(ids, dtype), n, img_dev if img_dev is not None else
                         (None if image is None else torch.from_numpy(np.ascontiguousarray(image)).to(DEV)))
    geom, inten, skipped = R.cell_stats(ids, n, image)
    assert got["geom"].dtype == np.int64 and got["geom"].shape == geom.shape
    assert np.array_equal(got["geom"], geom)
    assert np.array_equal(got["skipped"], skipped) and got["shape"] == ids.shape[-2:]
    if image is None:
        assert got["intensity"] is None
    else:
        assert got["intensity"].shape == inten.shape and np.array_equal(got["intensity"], inten)
    return got


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_tables_equal_the_restatement(shape, pattern):
    h, w = shape
    ids, n = _plane(pattern, h, w)
    got = _check(ids, n, R.image(h, w, 3, h + w), dtype=torch.int32)
    if pattern == "out of range":
        assert got["skipped"][0] == ((ids < 0) | (ids > n)).sum() > 0 or h * w == 1
    else:
        assert got["skipped"][0] == 0
    _check(ids, n, dtype=torch.int64)


def test_a_run_that_starts_in_the_last_lane_of_a_chunk_and_goes_on_in_the_next():
    ids = np.zeros((3, 600), np.int64)
    ids[0, 255:300] = 1   # the chunk's last pixel, then 44 of the next chunk
    ids[1, 252:258] = 2   # the last lane's four pixels and two more
    ids[2, 253:513] = 3   # across two chunk edges
    ids[2, 0:3], ids[2, 599] = 4, 4
    _check(ids, 4, R.image(3, 600, 2, 1), dtype=torch.int32)


def test_a_label_on_all_four_borders_and_a_label_that_is_absent():
    from eunet import metrics as M
    ids = np.zeros((37, 131), np.int64)
    ids[0, :], ids[-1, :], ids[:, 0], ids[:, -1] = 1, 1, 1, 1
    ids[10:20, 10:30] = 3
    got = _check(ids, 4, R.image(37, 131, 1, 2))
    assert got["geom"][0, 1, 6:10].tolist() == [0, 0, 130, 36]
    for label in (2, 4):  # absent: the box of no pixel, the range of no value
        assert got["geom"][0, label].tolist() == [0] * 6 + [131, 37, -1, -1] + [0] * 4
        assert got["intensity"][0, label, 0].tolist() == [0, 0, 255, 0]
    m = M.cell_measurements(got)
    assert m["touches_border"].tolist()[:1] == [1.0] and m["touches_border"][2] == 0.0 and m["holes"][0] == 1.0
    assert np.isnan(m["centroid_x"][1]) and m["area"].tolist() == [2 * 131 + 2 * 35, 0, 200, 0]


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("p", [1, 2, 3])
def test_planes_and_dtypes(p, dtype):
    h, w = 37, 131
    ids = np.stack([R.blobs(h, w, 6, 10 + q) for q in range(p)])
    ids[ids == 6] = 0
    ids[p - 1, 30:33, 100:120] = 6  # id 6 in the last plane only
    got = _check(ids, 6, R.image(h, w, 3, 4), dtype=dtype)
    assert [int(got["geom"][q, 6, 0]) for q in range(p)] == [0] * (p - 1) + [60]
    got2 = _check(ids[0], 6, dtype=dtype)  # [h, w]: one plane
    assert got2["geom"].shape == (1, 7, 14)


@pytest.mark.parametrize("c", [0, 1, 2, 3])
def test_image_channels_and_extremes(c):
    h, w = 37, 131
    ids = R.blobs(h, w, 8, 21)
    img = R.image(h, w, max(c, 1), 5)
    _check(ids, 8, img[:, :, 0] if c == 0 else img)  # c = 0: an [h, w] image
    for value in (0, 255):
        got = _check(ids, 8, np.full((h, w, max(c, 1)), value, np.uint8))
        present = got["geom"][0, 1:, 0] > 0
        assert present.any() and (got["intensity"][0, 1:, :, 2:][present] == value).all()


@pytest.mark.parametrize("offset", [1, 2, 3, 5])
def test_an_image_off_the_16_byte_boundary_is_handled(offset):
    """include/eunet.h: the image may have any byte alignment."""
    h, w, c = 37, 131, 3
    ids, img = R.noise(h, w, 20, 8), R.image(h, w, c, 9)
    flat = torch.zeros(h * w * c + offset, dtype=torch.uint8, device=DEV)
    flat[offset:] = torch.from_numpy(img).to(DEV).reshape(-1)
    view = flat[offset:].view(h, w, c)
    assert view.data_ptr() % 16 == offset % 16 and view.is_contiguous()
    _check(ids, 20, img, img_dev=view)
    # ids 4 bytes off a 16-byte line, as test_gpu_pairs.py does
    from eunet import ops
    t = torch.zeros(h * w + 1, dtype=torch.int32, device=DEV)
    t[1:] = _dev(ids, torch.int32).reshape(-1)
    got = ops.cell_stats(t[1:].view(h, w), 20, view)
    assert np.array_equal(got["geom"], R.cell_stats(ids, 20)[0])


def test_n_of_zero_one_and_a_million():
    """n = PAIRS_MAX_ID would need a geom table of (2^24) 14 8 bytes = 1.9 GB on the device and on the host; the
    tested n is capped at 2^20 (117 MB) and the limit itself is checked on the host side
    (tests/test_cellprops_host.py)."""
    from eunet import ops
    ids = np.array([[0, 1, 1], [2 ** 20, 0, 2 ** 20 - 1]], np.int64)
    got = _check(ids, 0)
    assert got["geom"].shape == (1, 1, 14) and not got["geom"].any() and got["skipped"][0] == 4
    _check(ids, 0, R.image(2, 3, 2, 1))
    assert _check(ids, 1)["skipped"][0] == 2
    big = _check(ids, 2 ** 20, R.image(2, 3, 1, 1))
    assert big["geom"][0, 2 ** 20, :3].tolist() == [1, 0, 1] and big["skipped"][0] == 0
    with pytest.raises(ValueError):
        ops.cell_stats(_dev(ids), ops.PAIRS_MAX_ID + 1)


def test_two_calls_give_identical_tables_and_the_entry_clears_a_dirty_buffer():
    """The order-independence claim: integer atomics only.  And the C-ABI writes every table entry itself."""
    from eunet import _lib, ops
    h, w, n, c = 129, 257, 50, 3
    ids, img = R.noise(h, w, n, 77), R.image(h, w, c, 78)
    ids[40:90, 30:200] = 7
    d_ids, d_img = _dev(ids, torch.int32), torch.from_numpy(img).to(DEV)
    a, b = ops.cell_stats(d_ids, n, d_img), ops.cell_stats(d_ids, n, d_img)
    for k in ("geom", "intensity", "skipped"):
        assert np.array_equal(a[k], b[k]), k
    geom = torch.full((1, n + 1, 14), -12345, dtype=torch.int64, device=DEV)
    inten = torch.full((1, n + 1, c, 4), 999, dtype=torch.int64, device=DEV)
    skipped = torch.full((1,), 55, dtype=torch.int64, device=DEV)
    for _ in range(2):  # into the dirty buffers, then into its own result
        _lib.call("eunet_cell_stats", ops._ptr(d_ids), 4, 1, h, w, n, ops._ptr(d_img), c, ops._ptr(geom),
                  ops._ptr(inten), ops._ptr(skipped), ops._stream())
        assert np.array_equal(geom.cpu().numpy(), a["geom"]) and np.array_equal(inten.cpu().numpy(), a["intensity"])
        assert skipped.item() == 0
    g_ref, i_ref, _ = R.cell_stats(ids, n, img)
    assert np.array_equal(a["geom"], g_ref) and np.array_equal(a["intensity"], i_ref)


# ---- the evaluator ------------------------------------------------------------------------------------------
_STATE = {}


def _model():
    if "model" not in _STATE:
        from eunet.models import EnhancedUNet
        torch.manual_seed(3)
        _STATE["model"] = EnhancedUNet(num_classes=3, in_channels=3, base_ch=16).to(DEV).eval()
    return _STATE["model"]


def _evaluator(model=None, **kw):
    from eunet.evaluator import Evaluator
    return Evaluator(model, DEV, "enhanced_unet", preprocess=None, **kw)


def _mask_evaluator(masks, **kw):
    """An Evaluator whose predicted masks are given, one per call: a randomly initialised small model predicts no
    usable cells, and what is under test here is everything after the mask."""
    ev = _evaluator(_model(), **kw)
    queue = [torch.from_numpy(np.ascontiguousarray(m).astype(np.int64)).to(DEV) for m in masks]
    ev._predict_mask_device = lambda image: queue.pop(0)
    return ev


def _item(h, w, seed):
    """A synthetic tile as a dataset item (tests/test_gpu_panoptic.py's)."""
    from eunet import synth
    x, m, inst = synth.tile(h, w, seed, num_classes=3, in_channels=3, instances=True)
    m = np.ascontiguousarray(m).astype(np.int64)
    masks, labels = [], []
    for j in np.unique(inst[inst > 0]).tolist():
        sel = inst == j
        masks.append(torch.from_numpy(sel.astype(np.uint8)))
        labels.append(int(m[sel][0]) - 1)
    m[:6, :9] = 255
    return x, {"semantic_mask": m, "instance_masks": masks, "instance_labels": labels}


def _shifted(m):
    """The ground-truth mask moved by two pixels: a prediction that matches most cells without being equal."""
    out = np.zeros_like(m)
    out[2:, 1:] = np.where(m == 255, 0, m)[:-2, :-1]
    return out


@pytest.mark.parametrize("split", ["erosion", "watershed"])
def test_measure_cells_is_the_restatement_on_the_instance_maps(split):
    from eunet import metrics as M
    x, item = _item(96, 128, 40)
    sem = _shifted(item["semantic_mask"])
    gray = (np.clip(np.asarray(x).transpose(1, 2, 0), 0, 1) * 255).astype(np.uint8) if np.asarray(x).ndim == 3 else None
    assert gray is not None and gray.shape == (96, 128, 3)
    ev = _mask_evaluator([sem, sem], split=split)
    ids, counts, scores = ev.semantic_to_instance_maps(torch.from_numpy(sem).to(DEV))
    assert min(counts) >= 1
    for intensity in (None, gray):
        got = ev.measure_cells(torch.from_numpy(np.asarray(x)), intensity=intensity, pixel_size=0.5)
        geom, inten, _ = R.cell_stats(ids.cpu().numpy(), max(counts), intensity)
        ref_stats = {"geom": geom, "intensity": inten, "shape": (96, 128)}
        assert (got["n_live"], got["n_dead"]) == tuple(counts)
        assert got["viability"] == counts[0] / (counts[0] + counts[1])
        for plane, name in enumerate(M.INSTANCE_CLASSES):
            ref = M.cell_measurements(ref_stats, plane, 0.5)
            assert set(got[name]) == set(ref) | {"score"}
            assert ("mean_2" in got[name]) == (intensity is not None)
            for k, v in ref.items():
                assert np.array_equal(got[name][k], v[:counts[plane]]), (name, k)
            assert (got[name]["area"] > 0).all() and got[name]["score"].tolist() == scores[plane]
    empty = _mask_evaluator([np.zeros((96, 128), np.int64)]).measure_cells(torch.from_numpy(np.asarray(x)))
    assert (empty["n_live"], empty["n_dead"], empty["viability"]) == (0, 0, 0.0) and len(empty["live"]["area"]) == 0


def test_measure_cells_runs_the_model_and_refuses_a_sigmoid_model():
    from eunet import synth
    x, _ = synth.tile(96, 128, 40, num_classes=3, in_channels=3)
    ev = _evaluator(_model())
    got = ev.measure_cells(torch.from_numpy(np.asarray(x)))
    ids, counts, _ = ev.semantic_to_instance_maps(ev._predict_mask_device(torch.from_numpy(np.asarray(x))))
    assert (got["n_live"], got["n_dead"]) == tuple(counts)
    geom, _, _ = R.cell_stats(ids.cpu().numpy(), max(counts))
    for plane, name in enumerate(("live", "dead")):
        assert np.array_equal(got[name]["area"], geom[plane, 1:counts[plane] + 1, 0].astype(np.float64))
    sig = _evaluator(_model(), activation="sigmoid")
    with pytest.raises(ValueError):
        sig.measure_cells(torch.from_numpy(np.asarray(x)))
    with pytest.raises(ValueError):
        sig.evaluate_measurements([])


def test_evaluate_measurements_is_measurement_agreement_on_the_restatements_tables():
    from eunet import metrics as M
    from eunet import ops
    items = [_item(96, 128, 40), _item(128, 96, 43)]
    loader = [{"images": [torch.from_numpy(np.asarray(x))], "batch_items": [it]} for x, it in items]
    preds = [_shifted(it["semantic_mask"]) for _, it in items]
    ev = _mask_evaluator(preds, split="watershed")
    result = ev.evaluate_measurements(loader)
    assert set(result) == {f"{k}_{c}" for k in M.AGREEMENT_KEYS for c in ("live", "dead")}
    parts = [[], []]
    for (x, it), sem in zip(items, preds):
        pred_ids, counts, _ = ev.semantic_to_instance_maps(torch.from_numpy(sem).to(DEV))
        gt_ids, _ = ev._gt_instance_maps(it, pred_ids.shape[1:], pred_ids.device)
        pairs = ops.label_pairs(pred_ids, gt_ids)
        gp, _, _ = R.cell_stats(pred_ids.cpu().numpy(), max(counts))
        gg, _, skipped = R.cell_stats(gt_ids.cpu().numpy(), len(it["instance_labels"]))
        assert skipped.sum() > 0  # the ignored corner is measured nowhere
        for plane in (0, 1):
            parts[plane].append(M.measurement_agreement(pairs, gp, gg, plane))
    for plane, name in enumerate(("live", "dead")):
        ref = M.agreement_summary(parts[plane])
        assert ref["n_matched"] >= 1 and ref["area_rel_err_mean"] < 1.0
        for k, v in ref.items():
            assert result[f"{k}_{name}"] == v or (v != v and result[f"{k}_{name}"] != result[f"{k}_{name}"]), k
    with pytest.raises(ValueError):
        ev.evaluate_measurements([])


DEBUG_CHILD = r'''
import sys, numpy as np, torch
sys.path[:0] = [ROOT, ROOT + "/enhanced-unet_amd", ROOT + "/tests"]
from eunet import _lib, ops
import _cellprops_ref as R
assert _lib.load().eunet_debug_enabled() == 1, "not the debug build"
assert _lib.debug_status(reset=True) == (0, 0)
h, w = 37, 131
img = torch.from_numpy(R.image(h, w, 3, 1)).to("cuda")
for name, ids, n in (("noise", R.noise(h, w, 50, 2), 50), ("rectangles", R.rectangles(h, w), 3)):
    for dtype in (torch.int32, torch.int64):
        got = ops.cell_stats(torch.from_numpy(ids).to("cuda").to(dtype), n, img)
        assert np.array_equal(got["geom"], R.cell_stats(ids, n)[0])
        st = _lib.debug_status()
        print(name, dtype, "debug status", st)
        assert st == (0, 0), (name, st)
print("DEBUG_OK")
'''


def test_debug_build_bounds_checks_pass():
    """The kernels' EUNET_DASSERT checks of every table index and pixel address stay silent."""
    lib = os.path.join(ROOT, "enhanced-unet_amd", "eunet", "libeunet_hip_debug.so")
    assert os.path.exists(lib), "build it: make -C enhanced-unet_amd debug"
    child = DEBUG_CHILD.replace("ROOT", repr(ROOT))
    r = subprocess.run([sys.executable, "-c", child], env=dict(os.environ, EUNET_LIB=lib), capture_output=True,
                       text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "DEBUG_OK" in r.stdout
