"""Generate tests/golden/instances.npz by running the REFERENCE implementation (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_instances.py

Three groups of fixtures, all produced by the reference's own functions (imported read-only through
gen_golden's stub modules, never copied):

  metrics   metrics.calculate_instance_metrics / calculate_viability_metrics (pure numpy) on hand-built
            mask lists: matches above and below the threshold, a class with predictions but no ground
            truth and the reverse, no predictions at all, equal scores (stable order), two ground truths
            of equal IoU (the first wins), overlapping ground truth, an all-zero prediction against an
            all-zero ground truth (IoU 1.0), `live_avg_iou_below_threshold`, the four viability branches.
  split     Evaluator.semantic_to_instances.  cv2 and skimage are not installed, so the reference's
            CONTROL FLOW is pinned and the primitives are supplied: the stub cv2 / skimage.measure
            modules get scipy-backed shims (minimum_filter / maximum_filter with mode='constant', cval 1 /
            0 and the element as footprint = OpenCV's un-reflected element and (k/2, k/2) anchor;
            ndimage.label with a 3x3 structure of ones = skimage's connectivity=2 numbering; the three
            MORPH_ELLIPSE elements as tables; a Suzuki-Abe outer-border follower and an arcLength that
            counts axis steps + diagonal steps * sqrt(2)).  A line tracer asserts that every branch arm of
            train_eval.py:654-850 ran in at least one case, except the arms listed in UNREACHED.
  evaluate  Evaluator.evaluate over two fake batches with predict_semantic_mask replaced by a lookup of
            prepared masks and the RLE / bounding-rect / COCO calls stubbed; the two mAP keys are dropped.

What the shims cannot pin (no cv2 here): which contour cv2.findContours lists first for an instance of
several components (taken as the one discovered last: OpenCV prepends) and cv2.arcLength's float32
segment rounding.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_golden import REF, _install_stubs  # noqa: E402

# cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (k, k)) for the three sizes the reference asks for
ELEMS = {
    (2, 2): np.array([[0, 1], [1, 1]], np.uint8),
    (3, 3): np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8),
    (5, 5): np.array([[0, 0, 1, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0]], np.uint8),
}
ONES3 = np.ones((3, 3), np.int32)
# direction codes of the border follower: 0 E, 1 NE, 2 N, 3 NW, 4 W, 5 SW, 6 S, 7 SE (y grows downwards)
DX = (1, 1, 0, -1, -1, -1, 0, 1)
DY = (0, -1, -1, -1, 0, 1, 1, 1)

# Arms of train_eval.py:654-850 (one line inside each) that must run in at least one split case ...
ARM_LINES = {
    669: "class absent: continue",
    694: "region under 200 px kept as one instance",
    734: "first-level piece over 200 px that the second erosion does not split",
    739: "first-level piece of at most 200 px",
    760: "piece of the single-erosion loop",
    763: "single-erosion loop succeeded: break",
    779: "piece of the 5x5 stage",
    784: "region that nothing splits, kept whole",
    810: "instance under the minimum area",
    813: "instance over the maximum area",
    823: "compactness from the perimeter",
    846: "cut to the 500 highest scores",
}
# ... and the arms no input reaches (the `except` arm is exempt by the task's definition):
UNREACHED = {
    729: "second-level split (sub_num2 > 1): the piece is dilate_it(E) for one connected component E of the "
         "it-times eroded region (it >= 2; the AND with the region removes nothing because dilate_it(E) lies "
         "inside the region's opening), and eroding it twice leaves closing_2(dilate_(it-2)(E)), which "
         "contains the connected set dilate_(it-2)(E); a randomised search over blob unions (search_second_"
         "level below, 4000 shapes) found no input with sub_num2 > 1 either",
    825: "perimeter == 0 needs contours[0] to be a single pixel; an instance arrives here with area >= 3, so "
         "only an instance of several components whose last-discovered component is one pixel could reach "
         "it -- none constructed",
    827: "len(contours) == 0 with area >= 3: a non-empty mask always has an external contour",
}


class Contour:
    """What the shimmed cv2.findContours returns per component: the chain-step counts of its outer border."""

    def __init__(self, n_axis, n_diag):
        self.n_axis, self.n_diag = n_axis, n_diag


def follow_outer_border(mask, y0, x0):
    """Suzuki-Abe outer-border following (8-connectivity) from the component's raster-first pixel (y0, x0):
    search clockwise from W for the first set neighbour; then walk counter-clockwise until the start is
    reached again from that neighbour.  Returns (axis steps, diagonal steps); an isolated pixel gives (0, 0)."""
    h, w = mask.shape

    def at(y, x):
        return 0 <= y < h and 0 <= x < w and mask[y, x] != 0

    s = 4
    while True:
        s = (s - 1) & 7
        if at(y0 + DY[s], x0 + DX[s]) or s == 4:
            break
    if s == 4:
        return 0, 0
    y1, x1 = y0 + DY[s], x0 + DX[s]
    y3, x3 = y0, x0
    n_axis = n_diag = 0
    for _ in range(4 * h * w + 4):
        for t in range(1, 9):
            ss = (s + t) & 7
            if at(y3 + DY[ss], x3 + DX[ss]):
                s = ss
                break
        y4, x4 = y3 + DY[s], x3 + DX[s]
        if s & 1:
            n_diag += 1
        else:
            n_axis += 1
        if (y4, x4) == (y0, x0) and (y3, x3) == (y1, x1):
            return n_axis, n_diag
        y3, x3, s = y4, x4, (s + 4) & 7
    raise AssertionError("border following did not close")


def install_shims():
    """Give the stub cv2 / skimage.measure modules the primitives semantic_to_instances calls."""
    cv2, measure = sys.modules["cv2"], sys.modules["skimage.measure"]
    cv2.MORPH_ELLIPSE, cv2.MORPH_OPEN, cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_SIMPLE = 2, 2, 0, 2

    def get_structuring_element(shape, ksize):
        assert shape == cv2.MORPH_ELLIPSE
        return ELEMS[tuple(ksize)]

    def erode(img, kernel, iterations=1):
        out = np.asarray(img, np.uint8)
        for _ in range(iterations):
            out = ndimage.minimum_filter(out, footprint=kernel, mode="constant", cval=1)
        return out

    def dilate(img, kernel, iterations=1):
        out = np.asarray(img, np.uint8)
        for _ in range(iterations):
            out = ndimage.maximum_filter(out, footprint=kernel, mode="constant", cval=0)
        return out

    def morphology_ex(img, op, kernel):
        assert op == cv2.MORPH_OPEN
        return dilate(erode(img, kernel), kernel)

    def find_contours(img, mode, method):
        lab, n = ndimage.label(img, structure=ONES3)
        firsts = ndimage.minimum_position(np.arange(img.size).reshape(img.shape), lab, range(1, n + 1)) if n else []
        contours = [Contour(*follow_outer_border(lab == k + 1, *firsts[k])) for k in range(n)]
        return contours[::-1], None  # OpenCV lists the contours in reverse order of discovery

    def label(img, connectivity=2, return_num=True):
        assert connectivity == 2 and return_num
        lab, n = ndimage.label(img, structure=ONES3)
        return lab, n

    cv2.getStructuringElement, cv2.erode, cv2.dilate = get_structuring_element, erode, dilate
    cv2.morphologyEx, cv2.bitwise_and = morphology_ex, np.bitwise_and
    cv2.findContours = find_contours
    cv2.arcLength = lambda c, closed: c.n_axis + c.n_diag * math.sqrt(2.0)
    cv2.boundingRect = lambda m: (0, 0, 1, 1)
    measure.label = label
    sys.modules["pycocotools.mask"].encode = lambda m: {"counts": ""}


def import_reference():
    _install_stubs()
    install_shims()
    sys.path.insert(0, REF)
    import metrics as ref_metrics  # noqa
    import train_eval as ref_te  # noqa
    return ref_metrics, ref_te


# ---- metrics ---------------------------------------------------------------------------------------
def rect(h, w, y0, y1, x0, x1):
    m = np.zeros((h, w), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def metric_cases():
    """(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels, iou_threshold) per case, 12 x 16 masks."""
    def r(*a):
        return rect(12, 16, *a)
    z = np.zeros((12, 16), np.uint8)
    return [
        # matches above and below 0.05, overlapping ground truth, both classes
        ([r(0, 4, 0, 4), r(0, 4, 6, 10), r(8, 12, 0, 8), r(8, 10, 10, 14)], [0, 0, 0, 1], [0.9, 0.8, 0.5, 0.8],
         [r(0, 4, 1, 6), r(0, 4, 5, 9), r(11, 12, 7, 16), r(8, 11, 10, 14)], [0, 0, 0, 1], 0.05),
        # live predictions without live ground truth; dead ground truth without dead predictions
        ([r(0, 4, 0, 4), r(5, 9, 0, 4)], [0, 0], [0.7, 0.6], [r(0, 4, 8, 12)], [1], 0.05),
        # no predictions at all
        ([], [], [], [r(0, 4, 0, 4), r(6, 9, 6, 9)], [0, 1], 0.05),
        # equal scores: the stable order gives the ground truth to the first prediction (IoU 0.8, not 0.6)
        ([r(0, 4, 1, 5), r(0, 4, 2, 5), r(6, 8, 0, 2)], [0, 0, 0], [0.5, 0.5, 0.5], [r(0, 4, 0, 5)], [0], 0.05),
        ([r(0, 4, 2, 5), r(0, 4, 1, 5)], [0, 0], [0.5, 0.5], [r(0, 4, 0, 5)], [0], 0.05),
        # two ground truths of equal IoU: the first wins, the second is left for the next prediction
        ([r(0, 4, 2, 6), r(0, 4, 5, 8)], [0, 0], [0.9, 0.3], [r(0, 4, 0, 4), r(0, 4, 4, 8)], [0, 0], 0.05),
        # all-zero prediction against all-zero ground truth: IoU 1.0
        ([z, r(4, 8, 4, 8)], [0, 1], [0.4, 0.6], [z, r(4, 8, 5, 9)], [0, 1], 0.05),
        # every prediction below a raised threshold, mean IoU >= 0.1: live_avg_iou_below_threshold appears
        ([r(0, 4, 0, 6), r(6, 10, 0, 4)], [0, 0], [0.9, 0.2], [r(0, 4, 3, 9), r(6, 10, 2, 8)], [0, 0], 0.5),
        # ... and below 0.1: it does not (the dead class here)
        ([r(0, 8, 0, 4)], [1], [0.9], [r(7, 9, 3, 16)], [1], 0.05),
        # scores in ascending order, masks as bool and int64 arrays
        ([r(0, 3, 0, 3).astype(bool), r(0, 3, 4, 7).astype(np.int64) * 7, r(5, 9, 5, 9)], [0, 0, 1], [0.1, 0.2, 0.3],
         [r(0, 3, 4, 8), r(0, 3, 0, 2), r(5, 9, 4, 9)], [0, 0, 1], 0.05),
    ]


def gen_metrics(ref_metrics, out):
    cases = metric_cases()
    seen = set()
    for i, (pm, pl, ps, gm, gl, thr) in enumerate(cases):
        m = ref_metrics.calculate_instance_metrics(pm, pl, ps, gm, gl, iou_threshold=thr)
        out[f"m{i}_pred"] = np.stack([np.asarray(x != 0, np.uint8) for x in pm]) if pm else np.zeros((0, 12, 16), np.uint8)
        out[f"m{i}_pred_labels"], out[f"m{i}_scores"] = np.array(pl, np.int64), np.array(ps, np.float64)
        out[f"m{i}_gt"] = np.stack([np.asarray(x != 0, np.uint8) for x in gm])
        out[f"m{i}_gt_labels"], out[f"m{i}_thr"] = np.array(gl, np.int64), np.float64(thr)
        out[f"m{i}_keys"] = np.array(sorted(m))
        out[f"m{i}_vals"] = np.array([float(m[k]) for k in sorted(m)], np.float64)
        seen |= set(m)
    assert "live_avg_iou_below_threshold" in seen
    out["m_n"] = len(cases)
    via = [(3, 1, 2, 2), (0, 0, 2, 1), (2, 1, 0, 0), (0, 0, 0, 0), (5, 0, 1, 4)]
    out["v_in"] = np.array(via, np.int64)
    keys = None
    vals = []
    for a in via:
        m = ref_metrics.calculate_viability_metrics(*a)
        keys = sorted(m)
        vals.append([float(m[k]) for k in keys])
    out["v_keys"], out["v_vals"] = np.array(keys), np.array(vals, np.float64)


# ---- instance split --------------------------------------------------------------------------------
def disc(m, cy, cx, r, v):
    yy, xx = np.ogrid[:m.shape[0], :m.shape[1]]
    m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = v


def split_cases():
    """name -> semantic mask (int64, at most 96 x 128; 1 live, 2 dead)."""
    c = {}
    m = np.zeros((40, 48), np.int64)
    m[4:9, 5:11] = 1                 # a small blob
    m[20, 20] = 1                    # an isolated pixel: the opening removes it
    m[0:6, 40:48] = 1                # a blob on the image border (corner)
    m[34:40, 0:5] = 2                # a dead blob on the border
    m[15:17, 30:32] = 2              # dead 2x2 block: 3 px after the opening, under the dead minimum of 5
    m[25:27, 30:33] = 2              # dead 2x3 block: under 5 px after the opening as well
    m[28:33, 10:16] = 2              # a dead blob that stays
    c["small"] = m
    m = np.zeros((30, 60), np.int64)
    disc(m, 14, 14, 9, 1)
    disc(m, 14, 40, 9, 1)
    m[13:16, 14:40] = 1              # two discs of radius 9 joined by a 3-px neck: the first erosion splits
    c["neck3"] = m
    m = np.zeros((64, 96), np.int64)
    m[3:18, 3:18] = 1                # 15 x 15 square: 224 px after the opening, nothing splits it, kept whole
    m[22:62, 30:70] = 1              # 40 x 40 square: over 1500 px, dropped
    c["squares"] = m
    m = np.zeros((32, 64), np.int64)
    m[4:24, 4:24] = 1
    m[4:24, 36:56] = 1
    m[10:18, 24:36] = 1              # two 20 x 20 squares joined by an 8-px-wide neck: splits at the 5x5 stage
    c["neck8"] = m
    m = np.zeros((24, 48), np.int64)
    m[4:18, 3:17] = 2
    m[4:18, 27:41] = 2
    m[8:13, 17:27] = 2               # two 14 x 14 squares, 5-px neck: connected after two erosions, split by the third
    c["neck5"] = m
    m = np.zeros((40, 96), np.int64)
    m[4:36, 4:36] = 1
    m[4:36, 50:90] = 1
    m[18:21, 36:50] = 1              # two pieces still over 200 px after the first split; the second erosion
    c["big_pair"] = m                # splits neither (they are kept, then dropped or kept by area)
    m = np.zeros((30, 70), np.int64)
    m[5:21, 4:20] = 1
    m[5:15, 26:36] = 1
    m[11:14, 20:26] = 1              # a piece over 200 px and a piece under 200 px from one first-level split
    c["mixed_pair"] = m
    m = np.zeros((72, 72), np.int64)
    for y in range(0, 72, 3):
        for x in range(0, 72, 3):
            m[y:y + 2, x:x + 2] = 1  # 576 blocks of 2 x 2 at pitch 3: more than 500 candidates
    c["field"] = m
    m = np.zeros((78, 72), np.int64)
    m[:72] = c["field"]
    m[73:78, 2:30] = 2               # the cut runs again after the dead class, on the combined list
    m[73:78, 40:46] = 2
    c["field_dead"] = m
    c["empty"] = np.zeros((16, 16), np.int64)
    return c


class LineTracer:
    """Records the lines of Evaluator.semantic_to_instances that execute."""

    def __init__(self, code):
        self.code, self.lines = code, set()

    def __call__(self, frame, event, arg):
        if frame.f_code is not self.code:
            return None
        if event == "line":
            self.lines.add(frame.f_lineno)
        return self

    def __enter__(self):
        sys.settrace(self)
        return self

    def __exit__(self, *exc):
        sys.settrace(None)


def index_map(masks, shape):
    """Instance masks (disjoint: they come from one marker image per class) -> int32 map of 1 + output index."""
    idx = np.zeros(shape, np.int32)
    for i, mk in enumerate(masks):
        assert not idx[mk > 0].any()
        idx[mk > 0] = i + 1
    return idx


def gen_split(ref_te, out):
    ev = ref_te.Evaluator(torch.nn.Identity(), "cpu", "enhanced_unet")
    code = ref_te.Evaluator.semantic_to_instances.__code__
    first = code.co_firstlineno
    assert first == 654, f"train_eval.py moved: semantic_to_instances starts at {first}"
    names, lines = [], set()
    for name, sem in split_cases().items():
        assert sem.shape[0] <= 96 and sem.shape[1] <= 128
        with LineTracer(code) as tr:
            masks, labels, scores = ev.semantic_to_instances(sem)
        lines |= tr.lines
        names.append(name)
        out[f"s_{name}_sem"] = sem
        out[f"s_{name}_index"] = index_map(masks, sem.shape)
        out[f"s_{name}_areas"] = np.array([int(mk.sum()) for mk in masks], np.int64)
        out[f"s_{name}_labels"] = np.array(labels, np.int64)
        out[f"s_{name}_scores"] = np.array([float(s) for s in scores], np.float64)
        print(f"  split {name}: {len(masks)} instances, labels {sorted(set(labels))}")
    out["s_names"] = np.array(names)
    missing = [f"{ln}: {why}" for ln, why in ARM_LINES.items() if ln not in lines]
    assert not missing, "branch arms that no split case reached:\n  " + "\n  ".join(missing)
    reached = [ln for ln in UNREACHED if ln in lines]
    assert not reached, f"arms listed as unreached did run: {reached}"
    assert len(out["s_field_labels"]) == 500 and len(out["s_field_dead_labels"]) == 500


def search_second_level(ref_te, tries=4000, seed=7):
    """Randomised search for an input whose second-level erosion splits a first-level piece
    (train_eval.py:722-730); not part of the fixture.  Run with `--search`."""
    ev = ref_te.Evaluator(torch.nn.Identity(), "cpu", "enhanced_unet")
    code = ref_te.Evaluator.semantic_to_instances.__code__
    g = np.random.default_rng(seed)
    for t in range(tries):
        m = np.zeros((96, 128), np.int64)
        for _ in range(int(g.integers(2, 9))):
            if g.random() < 0.5:
                disc(m, int(g.integers(8, 88)), int(g.integers(8, 120)), int(g.integers(3, 24)), 1)
            else:
                y, x = int(g.integers(0, 80)), int(g.integers(0, 110))
                m[y:y + int(g.integers(2, 40)), x:x + int(g.integers(2, 60))] = 1
        if g.random() < 0.5:
            m[g.random(m.shape) < 0.03] = 0
        with LineTracer(code) as tr:
            ev.semantic_to_instances(m)
        if 729 in tr.lines:
            return t, m
    return None


# ---- evaluate --------------------------------------------------------------------------------------
def evaluate_batches():
    """Two fake batches (2 + 1 images): prepared semantic predictions, ground-truth instances and masks."""
    cases = split_cases()
    items = []
    for name, shift in (("small", 1), ("neck3", 2), ("mixed_pair", 0)):
        pred = cases[name]
        gt_sem = np.roll(pred, shift, axis=1)
        gt_masks, gt_labels = [], []
        for cid in (1, 2):
            lab, n = ndimage.label(gt_sem == cid, structure=ONES3)
            for k in range(1, n + 1):
                gt_masks.append((lab == k).astype(np.uint8))
                gt_labels.append(cid - 1)
        items.append((pred, gt_sem, gt_masks, gt_labels))
    return items


def gen_evaluate(ref_te, out):
    items = evaluate_batches()
    ev = ref_te.Evaluator(torch.nn.Identity(), "cpu", "enhanced_unet")
    ev.predict_semantic_mask = lambda image: items[int(image)][0]
    ref_te.calculate_coco_metrics = lambda p, g: {"bbox_mAP": 0.0, "segm_mAP": 0.0}
    ref_te.tqdm = lambda it, **k: it

    def batch(idx):
        return {"images": [torch.tensor(i) for i in idx],
                "batch_items": [{"instance_masks": items[i][2], "instance_labels": items[i][3],
                                 "semantic_mask": torch.from_numpy(items[i][1]), "image_id": f"img{i}"} for i in idx]}

    res = ev.evaluate([batch([0, 1]), batch([2])])
    for k in ("bbox_mAP", "segm_mAP"):
        res.pop(k)
    for i, (pred, gt_sem, gt_masks, gt_labels) in enumerate(items):
        out[f"e{i}_pred"], out[f"e{i}_gt_sem"] = pred, gt_sem
        out[f"e{i}_gt_masks"], out[f"e{i}_gt_labels"] = np.stack(gt_masks), np.array(gt_labels, np.int64)
    out["e_n"] = len(items)
    out["e_keys"] = np.array(sorted(res))
    out["e_vals"] = np.array([float(res[k]) for k in sorted(res)], np.float64)


def save_npz(path, arrays):
    """np.savez_compressed with fixed zip timestamps, so that the file regenerates bit-identically."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[name]), allow_pickle=False)


def main():
    ref_metrics, ref_te = import_reference()
    if "--search" in sys.argv:
        print("second-level split:", search_second_level(ref_te))
        return
    out = {}
    gen_metrics(ref_metrics, out)
    gen_split(ref_te, out)
    gen_evaluate(ref_te, out)
    save_npz(os.path.join(HERE, "instances.npz"), out)
    print("wrote instances.npz:", os.path.getsize(os.path.join(HERE, "instances.npz")), "bytes")


if __name__ == "__main__":
    main()
