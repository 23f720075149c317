"""ops.score_hist (csrc/curves.hip) against the restatement of tests/_curves_ref.py, and the evaluator's curve
statistics on top of it.  Every histogram is integer: compared with torch.equal, no tolerance."""
import numpy as np
import pytest
import torch

import _curves_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEXT1 = np.nextafter(np.float32(1), np.float32(2))
DENORM = np.float32(1.401298464324817e-45)  # the smallest denormal


def _edges(bins):
    from eunet.metrics import ceil32, curve_edges
    if bins == 1208:
        e = curve_edges()
    else:
        e = ceil32(np.linspace(0, 1, bins + 1))
    assert len(e) == bins + 1 and np.all(np.diff(e) > 0)
    return e


def _probs(rng, shape):
    """Uniform scores with a saturated half (exact 0 and 1), a few above 1 and a few invalid ones."""
    p = rng.random(shape, dtype=np.float32)
    u = rng.random(shape)
    p[u < 0.25] = 0.0
    p[(u >= 0.25) & (u < 0.5)] = 1.0
    p[(u >= 0.5) & (u < 0.52)] = NEXT1
    p[(u >= 0.52) & (u < 0.53)] = np.nan
    p[(u >= 0.53) & (u < 0.54)] = -0.25
    p[(u >= 0.54) & (u < 0.55)] = np.inf
    p[(u >= 0.55) & (u < 0.57)] = -0.0
    return p


def _mask(rng, shape):
    return rng.choice(np.array([0, 1, 2, 255, 7, -1], np.int64), size=shape, p=[0.4, 0.2, 0.2, 0.1, 0.05, 0.05])


def _run(p, m, e, **kw):
    from eunet import ops
    hist, inv = ops.score_hist(torch.from_numpy(p).to(DEV), torch.from_numpy(m).to(DEV), e, **kw)
    assert hist.dtype == torch.int64 and inv.dtype == torch.int64 and tuple(inv.shape) == (1,)
    return hist.cpu(), int(inv.item())


def _check(p, m, e, **kw):
    hist, inv = _run(p, m, e, **kw)
    ref, rinv = R.score_hist_ref(p, m, e, **kw)
    assert tuple(hist.shape) == ref.shape
    assert torch.equal(hist, torch.from_numpy(ref))
    assert inv == rinv
    return hist, inv


@pytest.mark.parametrize("hw", [1, 3, 4, 5, 63, 257, 4099, 33153])
def test_shapes_classes_and_batches(hw):
    """Every head / tail length, class planes that start off a 16-byte boundary (hw % 4 != 0, K >= 2), one block
    and several (33153 pixels: five blocks a class), [K,h,w] and [N,K,h,w]."""
    rng = np.random.default_rng(hw)
    e = _edges(1208)
    h, w = (1, hw) if hw < 33153 else (129, 257)
    for k in (1, 2, 3):
        for n in (1, 2):
            p, m = _probs(rng, (n, k, h, w)), _mask(rng, (n, h, w))
            _check(p, m, e)
            if n == 1:
                _check(p[0], m[0], e)


@pytest.mark.parametrize("off", [1, 2, 3])
def test_a_probability_tensor_off_the_16_byte_boundary(off):
    """A contiguous view that starts `off` floats into its storage: class 0 needs the scalar head as well."""
    from eunet import ops
    rng = np.random.default_rng(off)
    e = _edges(1208)
    p, m = _probs(rng, (3, 7, 37)), _mask(rng, (7, 37))
    store = torch.zeros(p.size + off, dtype=torch.float32, device=DEV)
    view = store[off:].view(3, 7, 37)
    view.copy_(torch.from_numpy(p))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * off
    hist, inv = ops.score_hist(view, torch.from_numpy(m).to(DEV), e)
    ref, rinv = R.score_hist_ref(p, m, e)
    assert torch.equal(hist.cpu(), torch.from_numpy(ref)) and int(inv.item()) == rinv


@pytest.mark.parametrize("bins", [1, 2, 50, 1208, 3072])
def test_bin_counts(bins):
    rng = np.random.default_rng(bins)
    e = _edges(bins)
    _check(_probs(rng, (3, 31, 67)), _mask(rng, (31, 67)), e)


@pytest.mark.parametrize("bins", [50, 1208])
def test_every_edge_with_its_neighbours(bins):
    """Every edge, its fp32 predecessor and its successor, as positives of one class and negatives of another."""
    e = _edges(bins)
    vals = np.concatenate([e, np.nextafter(e, np.float32(-1)), np.nextafter(e, np.float32(2))]).astype(np.float32)
    p = np.stack([vals, vals[::-1]]).reshape(2, 1, -1)
    m = (np.arange(vals.size, dtype=np.int64) % 2).reshape(1, -1)
    hist, inv = _check(p, m, e)
    assert inv == 2  # the predecessor of 0, once per class
    # an edge belongs to the bin it opens; 1, and what lies above it, to the last bin
    one = _run(np.array([e[3], np.nextafter(e[3], np.float32(0)), 1.0, NEXT1], np.float32).reshape(1, 1, 4),
               np.zeros((1, 4), np.int64), e)[0]
    assert one[0, 3, 0] == 1 and one[0, 2, 0] == 1 and one[0, bins - 1, 0] == 2


def test_special_values():
    e = _edges(1208)
    vals = np.array([0.0, -0.0, 1.0, NEXT1, 1.5, DENORM, np.nan, np.inf, -np.inf, -1e-30], np.float32)
    p = vals.reshape(1, 1, -1)
    m = np.array([[0, 1, 1, 0, 1, 0, 1, 0, 1, 0]], np.int64)
    hist, inv = _check(p, m, e)
    assert inv == 4
    assert hist[0, 0].tolist() == [2, 1, 0]  # 0, -0.0 and the denormal: bin 0, confidence 0
    assert hist[0, 1207].tolist() == [1, 2, 3 * 2 ** 24]  # 1, nextafter(1) and 1.5, each clamped to 1
    assert int(hist[0, :, :2].sum()) == 6


@pytest.mark.parametrize("shape", [(64, 96), (129, 257), (10, 10)])
def test_one_bin_images(shape):
    """Every pixel on one (bin, truth) address -- the uniform-wave path --, then the same image with exactly one
    lane of one wave different (another bin, another truth, an invalid score, an ignored pixel); (10, 10) is
    fewer pixels than one block."""
    e = _edges(1208)
    h, w = shape
    p = np.zeros((3, h, w), np.float32)
    p[0] = 1.0
    p[1] = np.float32(0.3337)
    m = np.zeros((h, w), np.int64)
    hist, inv = _check(p, m, e)
    assert inv == 0 and hist[0, 1207].tolist() == [0, h * w, h * w * 2 ** 24] and hist[2, 0].tolist() == [h * w, 0, 0]
    y, x = h // 2, min(w - 1, 37)
    for change in ("bin", "truth", "invalid", "ignored"):
        q, t = p.copy(), m.copy()
        if change == "bin":
            q[:, y, x] = (0.5, 0.25, 0.125)
        elif change == "truth":
            t[y, x] = 1
        elif change == "invalid":
            q[1, y, x] = np.nan
        else:
            t[y, x] = 255
        got, ginv = _check(q, t, e)
        assert ginv == (1 if change == "invalid" else 0)
        assert not torch.equal(got, hist)


def test_an_all_ignored_mask_leaves_everything_zero():
    rng = np.random.default_rng(9)
    p = _probs(rng, (2, 3, 33, 65))
    for ignore in (255, -1, 3):
        m = np.full((2, 33, 65), ignore, np.int64)
        hist, inv = _check(p, m, _edges(50), ignore_index=ignore)
        assert inv == 0 and int(hist.abs().sum()) == 0


def test_labels_outside_the_classes_and_the_one_logit_rule():
    e = _edges(50)
    rng = np.random.default_rng(10)
    p = rng.random((3, 1, 600), dtype=np.float32)
    m = np.resize(np.array([7, -1, 0, 1, 2], np.int64), (1, 600))
    hist, _ = _check(p, m, e)
    assert [int(hist[c, :, 1].sum()) for c in range(3)] == [120, 120, 120]  # 7 and -1: negatives of every class
    assert [int(hist[c, :, 0].sum()) for c in range(3)] == [480, 480, 480]
    m1 = np.resize(np.array([0, 1, 2], np.int64), (1, 600))
    h1, _ = _check(p[:1], m1, e)
    assert int(h1[0, :, 1].sum()) == 400 and int(h1[0, :, 0].sum()) == 200  # K = 1: positive where the mask is >= 1
    _check(p[:1], m, e)  # -1 is a negative, 7 a positive of the one logit


def test_accumulation_and_fresh_outputs():
    """Two calls through out= equal one call on the concatenation; out=None starts from zero whatever the
    allocator hands back."""
    from eunet import ops
    rng = np.random.default_rng(11)
    e = _edges(1208)
    p, m = _probs(rng, (2, 3, 40, 50)), _mask(rng, (2, 40, 50))
    both, binv = _check(p, m, e)
    dp, dm = torch.from_numpy(p).to(DEV), torch.from_numpy(m).to(DEV)
    acc = ops.score_hist(dp[0], dm[0], e)
    back = ops.score_hist(dp[1], dm[1], e, out=acc)
    assert back[0] is acc[0] and back[1] is acc[1]
    assert torch.equal(acc[0].cpu(), both) and int(acc[1].item()) == binv
    first = [t.clone() for t in ops.score_hist(dp[0], dm[0], e)]
    del acc, back
    for _ in range(3):  # leave non-zero int64 blocks of the outputs' sizes in the allocator's cache
        junk = [torch.full((3, 1208, 3), -7, dtype=torch.int64, device=DEV),
                torch.full((1,), -7, dtype=torch.int64, device=DEV)]
        del junk
        again = ops.score_hist(dp[0], dm[0], e)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
        del again
    # the edge table may be a device tensor as well
    ed = torch.from_numpy(e).to(DEV)
    assert torch.equal(ops.score_hist(dp[0], dm[0], ed)[0], first[0])


def test_the_wrapper_refuses():
    from eunet import ops
    e = _edges(50)
    p = torch.rand(3, 8, 8, device=DEV)
    m = torch.zeros(8, 8, dtype=torch.int64, device=DEV)
    ops.score_hist(p, m, e)
    bad = [
        lambda: ops.score_hist(p.double(), m, e),
        lambda: ops.score_hist(p, m.int(), e),
        lambda: ops.score_hist(p.cpu(), m, e),
        lambda: ops.score_hist(p, m.cpu(), e),
        lambda: ops.score_hist(p, m[:7], e),
        lambda: ops.score_hist(p[None], m, e),
        lambda: ops.score_hist(p, m[None], e),
        lambda: ops.score_hist(torch.rand(4, 8, 8, device=DEV), m, e),
        lambda: ops.score_hist(p.transpose(1, 2), m, e),
        lambda: ops.score_hist(p[:, :, ::2], m[:, ::2], e),
        lambda: ops.score_hist(p, m, e[:-1]),  # does not end at 1
        lambda: ops.score_hist(p, m, e[1:]),  # does not start at 0
        lambda: ops.score_hist(p, m, np.array([0, 0.5, 0.5, 1], np.float32)),
        lambda: ops.score_hist(p, m, np.array([0, 0.6, 0.5, 1], np.float32)),
        lambda: ops.score_hist(p, m, np.array([0, np.nan, 1], np.float32)),
        lambda: ops.score_hist(p, m, np.array([1.0], np.float32)),
        lambda: ops.score_hist(p, m, np.linspace(0, 1, 3074).astype(np.float32)),
        lambda: ops.score_hist(p, m, torch.from_numpy(e).to(DEV).double()),
        lambda: ops.score_hist(p, m, torch.tensor([0.0, 0.7, 0.2, 1.0], device=DEV)),
        lambda: ops.score_hist(p, m, e, ignore_index=2 ** 31),
        lambda: ops.score_hist(p, m, e, out=(torch.zeros(3, 49, 3, dtype=torch.int64, device=DEV),
                                             torch.zeros(1, dtype=torch.int64, device=DEV))),
        lambda: ops.score_hist(p, m, e, out=(torch.zeros(3, 50, 3, dtype=torch.int32, device=DEV),
                                             torch.zeros(1, dtype=torch.int64, device=DEV))),
        lambda: ops.score_hist(p, m, e, out=(torch.zeros(3, 50, 3, dtype=torch.int64, device=DEV),
                                             torch.zeros(1, dtype=torch.int64))),
    ]
    for i, f in enumerate(bad):
        try:
            f()
        except ValueError:
            continue
        pytest.fail(f"case {i} was accepted")


# ---- the evaluator ----------------------------------------------------------------------------------------
_MODELS = {}


def _model(K):
    """A base-16 enhanced_unet in eval mode with random weights and non-trivial BatchNorm statistics; built once."""
    if K not in _MODELS:
        from eunet.models import get_model
        torch.manual_seed(3)
        m = get_model("enhanced_unet", num_classes=K, base_ch=16)
        g = torch.Generator().manual_seed(4)
        for k, v in m.state_dict().items():
            if k.endswith("running_mean"):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            elif k.endswith("running_var"):
                v.copy_(0.5 + torch.rand(v.shape, generator=g))
        _MODELS[K] = m.to(DEV).eval()
    return _MODELS[K]


def _loader(sizes=((64, 96), (70, 90)), seed=21):
    """One batch of two images (64 x 96 and a size that is no multiple of 32) with masks of 0, 1, 2 and 255."""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    images, items = [], []
    for h, w in sizes:
        images.append(torch.rand(3, h, w, generator=g))
        sem = rng.choice(np.array([0, 1, 2, 255], np.int64), size=(h, w), p=[0.5, 0.25, 0.2, 0.05])
        items.append({"semantic_mask": sem, "instance_masks": [], "instance_labels": [], "image_id": f"{h}x{w}"})
    return [{"images": images[:1], "batch_items": items[:1]}, {"images": images[1:], "batch_items": items[1:]}]


def _expected(ev, loader, probs_of):
    from eunet import ops
    from eunet.metrics import curve_edges
    acc = None
    for batch in loader:
        for img, item in zip(batch["images"], batch["batch_items"]):
            with torch.no_grad():
                probs = probs_of(img)
            acc = ops.score_hist(probs, torch.from_numpy(item["semantic_mask"]).to(DEV), curve_edges(), out=acc)
    return acc[0].cpu().numpy(), int(acc[1].item())


@pytest.mark.parametrize("tta", [False, True])
def test_evaluate_curves_bins_the_evaluators_own_probabilities(tta):
    from eunet.evaluator import Evaluator
    ev = Evaluator(_model(3), DEV, "enhanced_unet", preprocess=None)
    loader = _loader()
    res = ev.evaluate_curves(loader, tta=tta)
    if tta:
        hist, inv = _expected(ev, loader, ev.predict_probs)
    else:
        hist, inv = _expected(ev, loader, lambda img: ev._run_model_single(img.to(DEV)))
    assert res["hist"].dtype == np.int64 and np.array_equal(res["hist"], hist) and res["invalid"] == inv == 0
    assert int(hist[:, :, :2].sum()) == 3 * sum(int((b["batch_items"][0]["semantic_mask"] != 255).sum()) for b in loader)
    for name in ("background", "live", "dead"):
        r = res[name]
        assert 0.0 <= r["auc"] <= 1.0 and 0.0 <= r["ap"] <= 1.0 and 0.0 <= r["ece"] <= 1.0
        assert r["cal_count"].sum() == r["n_pos"] + r["n_neg"] == r["conf_hist"].sum()
    other = ev.evaluate_curves(loader, tta=not tta)
    assert not np.array_equal(other["hist"], res["hist"])  # the two definitions do differ


def test_evaluate_curves_tiled_equals_untiled():
    """tile=160 is the smallest tile the default exact blend (margin 64) accepts; 200 x 170 pads to 224 x 192 and
    is cut in both axes."""
    from eunet.evaluator import Evaluator
    loader = _loader(sizes=((200, 170), (70, 90)), seed=22)
    whole = Evaluator(_model(3), DEV, "enhanced_unet", preprocess=None)
    tiled = Evaluator(_model(3), DEV, "enhanced_unet", preprocess=None, tile=160)
    assert tiled._tile_plan(200, 170).n > 1
    for tta in (False, True):
        a, b = whole.evaluate_curves(loader, tta=tta), tiled.evaluate_curves(loader, tta=tta)
        assert np.array_equal(a["hist"], b["hist"]) and a["invalid"] == b["invalid"]
        assert a["live"]["auc"] == b["live"]["auc"]


def test_evaluate_with_curves_adds_the_curve_rows():
    """evaluate_with_curves: evaluate()'s 23 rows with evaluate()'s values, plus CURVE_KEYS with evaluate_curves'
    values (evaluate's own signature is pinned by tests/test_coco_host.py, so the flag is a method)."""
    import inspect
    from eunet.evaluator import CURVE_KEYS, EVALUATE_KEYS, Evaluator
    ev = Evaluator(_model(3), DEV, "enhanced_unet", preprocess=None)
    loader = _loader()
    plain = ev.evaluate(loader)
    with_curves = ev.evaluate_with_curves(loader)
    assert list(inspect.signature(Evaluator.evaluate).parameters) == ["self", "dataloader", "coco_map"]
    assert len(EVALUATE_KEYS) == 23 and sorted(plain) == sorted(EVALUATE_KEYS)
    assert sorted(with_curves) == sorted(EVALUATE_KEYS + CURVE_KEYS)
    assert CURVE_KEYS == tuple(f"{s}_{c}" for c in ("background", "live", "dead") for s in ("auc", "ap", "ece"))
    for k in EVALUATE_KEYS:
        assert with_curves[k] == plain[k], k
    curves = ev.evaluate_curves(loader, tta=True)
    for c in ("background", "live", "dead"):
        for s in ("auc", "ap", "ece"):
            assert with_curves[f"{s}_{c}"] == curves[c][s]


def test_a_one_logit_sigmoid_model_runs():
    from eunet.evaluator import Evaluator
    ev = Evaluator(_model(1), DEV, "enhanced_unet", preprocess=None, activation="sigmoid")
    loader = _loader()
    res = ev.evaluate_curves(loader)
    hist, inv = _expected(ev, loader, ev.predict_probs)
    assert res["hist"].shape == (1, 1208, 3) and np.array_equal(res["hist"], hist) and res["invalid"] == inv
    r = res["foreground"]
    n_fg = sum(int(((b["batch_items"][0]["semantic_mask"] >= 1) & (b["batch_items"][0]["semantic_mask"] != 255)).sum())
               for b in loader)
    assert r["n_pos"] == n_fg and 0.0 <= r["auc"] <= 1.0
