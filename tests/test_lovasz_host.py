"""The Lovasz losses on the host: the restatement tests/_lovasz_ref.py against the definition of the Lovasz extension
by brute force, its closed-form gradient against exact fractions, the degenerate segments, every ValueError of the
Python layer, and the header / _lib parity of the new entry points.  No GPU."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import _lovasz_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _jaccard_loss(gt, m):
    """Delta(M) = 1 - |G \\ M| / |G u M| for the set of mispredicted elements M (Berman et al., eq. 5 with the
    mispredictions as the argument); 0 for G and M both empty."""
    union = int((gt | m).sum())
    return 0.0 if union == 0 else 1.0 - int((gt & ~m).sum()) / union


@pytest.mark.parametrize("seed", range(40))
def test_restatement_is_the_lovasz_extension_of_the_jaccard_loss(seed):
    """l = sum_r e_(r) (Delta_r - Delta_{r-1}) with Delta_r the set loss of the first r elements in sorted order, to
    1e-12; and g sums to Delta(all)."""
    rng = np.random.default_rng(seed)
    L = int(rng.integers(1, 9))
    e = rng.random(L)
    if seed % 3 == 0:
        e[rng.integers(0, L, size=2)] = 0.5  # ties
    gt = rng.random(L) < 0.5
    flags = gt.astype(np.uint8)
    order, v = R.order_of(e, flags)
    assert v == L
    g = R.lovasz_grad(gt[order]).astype(np.float64)
    m = np.zeros(L, dtype=bool)
    prev, brute = _jaccard_loss(gt, m), 0.0
    for i in order:
        m[i] = True
        cur = _jaccard_loss(gt, m)
        brute += e[i] * (cur - prev)
        prev = cur
    if not gt.any():  # G = 0: the definition's special case, the largest error is penalised
        brute = e[order[0]]
        assert g[0] == 1.0 and not g[1:].any()
    else:
        assert abs(g.sum() - _jaccard_loss(gt, np.ones(L, dtype=bool))) <= 1e-6  # g is rounded to fp32
    assert abs(float((e[order] * g).sum()) - brute) <= 1e-6
    # the same in exact arithmetic on the unrounded closed form
    G = int(gt.sum())
    if G:
        F = np.cumsum(gt[order])
        exact = [1.0 / (G + r - F[r - 1]) if gt[order[r - 1]] else
                 (G - F[r - 1]) / ((G + r - F[r - 1] - 1.0) * (G + r - F[r - 1])) for r in range(1, L + 1)]
        assert abs(float((e[order] * np.array(exact)).sum()) - brute) <= 1e-12
        assert abs(sum(exact) - _jaccard_loss(gt, np.ones(L, dtype=bool))) <= 1e-12


@pytest.mark.parametrize("seed", range(10))
def test_closed_form_equals_the_jaccard_differences_in_fractions(seed):
    rng = np.random.default_rng(100 + seed)
    L = int(rng.integers(1, 40))
    fg = rng.random(L) < rng.random()
    if not fg.any():
        fg[rng.integers(0, L)] = True
    G = int(fg.sum())
    g = R.lovasz_grad(fg)
    F, prev = 0, Fraction(0)
    for r in range(1, L + 1):
        F += int(fg[r - 1])
        J = 1 - Fraction(G - F, G + r - F)
        assert g[r - 1] == np.float32(float(J - prev)), (r, g[r - 1], J - prev)
        prev = J


def test_degenerate_segments():
    g = R.lovasz_grad(np.zeros(5, dtype=bool))  # G = 0
    assert g.tolist() == [1, 0, 0, 0, 0]
    g = R.lovasz_grad(np.ones(4, dtype=bool))  # all foreground: 1 / G each
    assert g.tolist() == [0.25] * 4
    order, grad, counts = R.sort_ref(np.array([[0.3, 0.9, 0.1]]), np.full((1, 3), 2, dtype=np.uint8))  # V = 0
    assert order.tolist() == [[0, 1, 2]] and not grad.any() and counts.tolist() == [[0, 0]]
    x = torch.zeros(1, 2, 1, 3)
    t = torch.full((1, 1, 3), 255)
    out = R.loss(x, t, "softmax", ignore_index=255)
    assert out["loss"] == 0.0 and np.isnan(out["parts"]).all() and not out["weights"].any()


def test_order_rules():
    e = np.array([0.0, np.inf, -0.0, np.nan, 1.0, 5.0, 1.0, -2.0])
    flags = np.array([0, 0, 1, 0, 1, 2, 0, 0], dtype=np.uint8)
    order, v = R.order_of(e, flags)
    assert v == 7 and order.tolist() == [3, 1, 4, 6, 0, 2, 7, 5]


def _cpu_pair(k=2, h=3, w=4, n=2):
    return torch.zeros(n, k, h, w), torch.zeros(n, h, w, dtype=torch.int64)


@pytest.mark.parametrize("what,make", [
    ("activation", lambda x, t: dict(logits=x, target=t, activation="sigmoid")),
    ("K = 1", lambda x, t: dict(logits=x[:, :1].contiguous(), target=t)),
    ("float32", lambda x, t: dict(logits=x.double(), target=t)),
    ("int64", lambda x, t: dict(logits=x, target=t.int())),
    ("does not match", lambda x, t: dict(logits=x, target=t[:, :2])),
    ("N, K, H, W", lambda x, t: dict(logits=x[0], target=t[0])),
    ("shape rule", lambda x, t: dict(logits=torch.zeros(2, 4, 3, 4), target=t)),
    ("shape rule", lambda x, t: dict(logits=torch.zeros(65, 2, 1, 1), target=torch.zeros(65, 1, 1, dtype=torch.int64))),
    ("one GPU", lambda x, t: dict(logits=x, target=t)),
    ("int32", lambda x, t: dict(logits=x, target=t, ignore_index=2 ** 40)),
    ("classes", lambda x, t: dict(logits=x, target=t, classes="some")),
    ("classes", lambda x, t: dict(logits=x, target=t, classes=[2])),
    ("classes", lambda x, t: dict(logits=x, target=t, classes=[])),
])
def test_python_layer_refusals(what, make):
    """Every refusal is a ValueError raised before any launch (there is no device here to launch on)."""
    from eunet.losses import lovasz_loss
    x, t = _cpu_pair()
    with pytest.raises(ValueError, match=re.escape(what)):
        lovasz_loss(**make(x, t))


def test_ops_refusals():
    from eunet import ops
    x, t = _cpu_pair()
    with pytest.raises(ValueError, match="one GPU"):
        ops.lovasz_errors(x, t, "softmax")
    with pytest.raises(ValueError, match="contiguous"):
        ops.lovasz_errors(x.permute(0, 1, 3, 2), t.permute(0, 2, 1), "softmax")
    with pytest.raises(ValueError, match="K = 1"):
        ops.lovasz_errors(x[:, :1].contiguous(), t, "softmax")
    e, f = torch.zeros(2, 5), torch.zeros(2, 5, dtype=torch.uint8)
    for bad_e, bad_f, msg in ((e.double(), f, "float32"), (e, f.int(), "uint8"), (e[0], f[0], r"\[S, L\]"),
                              (e, f[:, :4].contiguous(), "differ in shape"), (e.t(), f.t(), "contiguous"),
                              (e, f, "one GPU")):
        with pytest.raises(ValueError, match=msg):
            ops.lovasz_sort(bad_e, bad_f)


def test_module_reads_its_attributes_at_call_time():
    from eunet.losses import LovaszLoss
    m = LovaszLoss()
    assert (m.activation, m.classes, m.per_image, m.ignore_index, m.weight) == ("softmax", None, False, None, 1.0)
    m.activation = "sigmoid"
    with pytest.raises(ValueError, match="activation"):
        m(*_cpu_pair())


def test_header_and_lib_declare_the_lovasz_entry_points():
    from eunet import _lib
    src = open(os.path.join(ROOT, "include", "eunet.h")).read()
    declared = set(re.findall(r"^\s*int\s+(eunet_lovasz_\w+)\s*\(", src, flags=re.M))
    expect = {"eunet_lovasz_workspace_bytes", "eunet_lovasz_errors", "eunet_lovasz_sort", "eunet_lovasz_fwd",
              "eunet_lovasz_bwd"}
    assert declared == expect
    assert {s for s in _lib.exported_symbols() if s.startswith("eunet_lovasz_")} == expect
    lib = _lib.load()
    for name in expect:
        assert hasattr(lib, name), name
    b = _lib.c_size_t()
    _lib.call("eunet_lovasz_workspace_bytes", 3, 4 * 1024 * 1024, __import__("ctypes").byref(b))
    assert 16 * 3 * 4 * 1024 * 1024 <= b.value < 17 * 3 * 4 * 1024 * 1024  # 16 bytes per element and small tables
