"""Host side of the signed distance map and the boundary loss: the fp64 restatement the GPU tests compare with
(tests/_sdf_ref.py) against hand-derived answers, scipy's Euclidean transform (where scipy imports) and a finite
difference, and the argument checks of the public functions that run before any device call.  None needs a GPU."""
import numpy as np
import pytest
import torch

import _sdf_ref as S

IGN = 255


def _phi(rows, K, **kw):
    return S.signed_distance(np.asarray(rows, dtype=np.int64)[None], K, **kw)[0][0]


def test_row_of_five():
    """[0,1,1,1,0]: class 1 is 0 on its two contour pixels, -1 at its centre, +1 on the first pixels outside; class 0
    mirrors it with the +1 / 0 roles swapped."""
    phi = _phi([[0, 1, 1, 1, 0]], 2)
    assert phi.dtype == np.float32 and phi.shape == (2, 1, 5)
    assert phi[1, 0].tolist() == [1.0, 0.0, -1.0, 0.0, 1.0]
    assert phi[0, 0].tolist() == [0.0, 1.0, 2.0, 1.0, 0.0]
    assert _phi([[0, 2, 1, 2, 0]], 1)[0, 0].tolist() == [1.0, 0.0, -1.0, 0.0, 1.0]  # K = 1: target >= 1


def test_single_pixel():
    t = np.zeros((5, 5), dtype=np.int64)
    t[2, 2] = 1
    phi = _phi(t, 2)[1]
    assert phi[2, 2] == 0.0  # its own contour
    assert phi[2, 3] == 1.0 and phi[1, 2] == 1.0
    assert phi[1, 1] == np.float32(np.sqrt(2.0)) and phi[0, 0] == np.float32(np.sqrt(8.0))
    assert phi[0, 2] == 2.0


def test_empty_and_full_class_are_zero():
    t = np.zeros((1, 4, 6), dtype=np.int64)
    phi, _, _ = S.signed_distance(t, 3)
    assert not phi.any()  # class 0 is full, 1 and 2 are empty
    phi1, _, _ = S.signed_distance(t + 2, 1)
    assert not phi1.any()  # K = 1: everything is foreground


def test_ignored_pixel():
    """[1,1,IGN,0,0]: the ignored pixel is 0 in every plane, lies outside both classes and is a site of both
    complements, so the class-1 pixel next to it is a contour pixel (0) and the one behind it is at -1."""
    phi = _phi([[1, 1, IGN, 0, 0]], 2, ignore_index=IGN)
    assert phi[1, 0].tolist() == [-1.0, 0.0, 0.0, 2.0, 3.0]
    assert phi[0, 0].tolist() == [3.0, 2.0, 0.0, 0.0, -1.0]
    assert _phi([[1, 1, IGN, 0, 0]], 1, ignore_index=IGN)[0, 0].tolist() == [-1.0, 0.0, 0.0, 2.0, 3.0]
    # a sample whose only other pixels are ignored: the complement is not empty, the contour exists
    assert _phi([[IGN, 1, 1, 1, IGN]], 2, ignore_index=IGN)[1, 0].tolist() == [0.0, 0.0, -1.0, 0.0, 0.0]


def test_clip_and_scale():
    row = [[0] * 6 + [1] * 9 + [0]]
    phi, raw, clamped = S.signed_distance(np.asarray(row, dtype=np.int64)[None], 2, clip=3.0, scale=0.25)
    assert raw[0, 1, 0].tolist() == [6, 5, 4, 3, 2, 1, 0, -1, -2, -3, -4, -3, -2, -1, 0, 1]
    assert phi[0, 1, 0].tolist() == [0.75, 0.75, 0.75, 0.75, 0.5, 0.25, 0, -0.25, -0.5, -0.75, -0.75, -0.75, -0.5,
                                     -0.25, 0, 0.25]
    assert clamped[0, 1, 0].tolist() == [True] * 3 + [False] * 7 + [True] + [False] * 5


def test_restatement_equals_scipy_on_non_degenerate_planes():
    ndi = pytest.importorskip("scipy.ndimage")
    t = S.blobs(2, 23, 29, (0, 1, 2), seed=3)
    phi, raw, _ = S.signed_distance(t, 3)
    for n in range(2):
        for c in range(3):
            m = t[n] == c
            assert m.any() and not m.all()
            ref = ndi.distance_transform_edt(~m) * ~m - (ndi.distance_transform_edt(m) - 1) * m
            assert float(np.abs(raw[n, c] - ref).max()) <= 1e-12
    fg = t >= 1
    raw1 = S.signed_distance(t, 1)[1]
    for n in range(2):
        ref = ndi.distance_transform_edt(~fg[n]) * ~fg[n] - (ndi.distance_transform_edt(fg[n]) - 1) * fg[n]
        assert float(np.abs(raw1[n, 0] - ref).max()) <= 1e-12


@pytest.mark.parametrize("activation,K", [("softmax", 2), ("softmax", 3), ("sigmoid", 1), ("sigmoid", 3)])
def test_loss_gradient_against_a_finite_difference(activation, K):
    g = torch.Generator().manual_seed(11 + K)
    x = torch.randn(2, K, 3, 4, generator=g)
    d = torch.randn(2, K, 3, 4, generator=g) * 3
    cw = (0.0, 1.0, 2.0)[3 - K:]
    v, parts, grad, a, parts_a = S.boundary_loss(x, d, activation, cw, g=3.7)
    assert abs(float(parts.mean()) - v) <= 1e-15 and a >= abs(v) and bool((parts_a >= parts.abs()).all())
    xd, eps, worst = x.double(), 1e-6, 0.0
    for i in range(x.numel()):
        e = torch.zeros(x.numel(), dtype=torch.float64)
        e[i] = eps
        e = e.view_as(xd)
        hi = S.boundary_loss(xd + e, d, activation, cw)[0]
        lo = S.boundary_loss(xd - e, d, activation, cw)[0]
        worst = max(worst, abs(3.7 * (hi - lo) / (2 * eps) - float(grad.view(-1)[i])))
    assert worst <= 1e-8, worst


def test_restatement_probabilities_and_their_saturated_gradient():
    """The restatement's p equals torch's softmax and sigmoid; its autograd gradient stays exact where torch's own
    backward cancels: two logits 100 apart give p_0 p_1 (a_0 - a_1) with p_1 = exp(-100), antisymmetric, and a
    sigmoid at +60 gives dist exp(-60), not 0."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, 4, 5, generator=g, dtype=torch.float64) * 3
    assert float((S.probabilities(x, "softmax") - torch.softmax(x, 1)).abs().max()) <= 1e-15
    assert float((S.probabilities(x, "sigmoid") - torch.sigmoid(x)).abs().max()) <= 1e-15
    x2 = torch.tensor([50.0, -50.0]).view(1, 2, 1, 1)
    d2 = torch.tensor([3.0, -2.0]).view(1, 2, 1, 1)
    grad = S.boundary_loss(x2, d2, "softmax")[2].view(-1)
    want = np.exp(-100.0) * 5.0 / 2  # Kw = 2
    assert abs(float(grad[0]) - want) <= 1e-12 * want and abs(float(grad[1]) + want) <= 1e-12 * want
    gs = S.boundary_loss(torch.tensor([60.0]).view(1, 1, 1, 1), torch.tensor([3.0]).view(1, 1, 1, 1), "sigmoid")[2]
    assert abs(float(gs) - 3.0 * np.exp(-60.0)) <= 1e-12 * 3.0 * np.exp(-60.0)
    far = S.boundary_loss(torch.tensor([900.0, -900.0]).view(1, 2, 1, 1), d2, "softmax")
    assert far[0] == 1.5 and bool(torch.isfinite(far[2]).all())


def test_kervadec_idc_weights_count_one_class():
    """class_weight (0, 1, 0): Kw = 1 and only class 1 is integrated."""
    g = torch.Generator().manual_seed(5)
    x, d = torch.randn(1, 3, 4, 5, generator=g), torch.randn(1, 3, 4, 5, generator=g)
    v = S.boundary_loss(x, d, "softmax", (0, 1, 0))[0]
    ref = float((torch.softmax(x.double(), 1)[:, 1] * d.double()[:, 1]).mean())
    assert abs(v - ref) <= 1e-15


# ---- argument checks that run before any device call (CPU tensors: nothing here reaches the library) ----
def test_signed_distance_map_refuses_bad_arguments():
    from eunet import ops
    t = torch.zeros(2, 4, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="int64"):
        ops.signed_distance_map(t.int(), 3)
    with pytest.raises(ValueError, match=r"\[H, W\] or \[N, H, W\]"):
        ops.signed_distance_map(t[None], 3)
    with pytest.raises(ValueError, match="num_classes"):
        ops.signed_distance_map(t, 4)
    with pytest.raises(ValueError, match="num_classes"):
        ops.signed_distance_map(t, 0)
    for clip in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="clip"):
            ops.signed_distance_map(t, 3, clip=clip)
    with pytest.raises(ValueError, match="scale"):
        ops.signed_distance_map(t, 3, scale=float("inf"))
    with pytest.raises(ValueError, match="one of the 3 classes"):
        ops.signed_distance_map(t, 3, ignore_index=2)


def test_boundary_loss_refuses_bad_arguments():
    from eunet.losses import BoundaryLoss, boundary_loss
    x = torch.zeros(2, 3, 4, 4)
    d = torch.zeros(2, 3, 4, 4)
    with pytest.raises(ValueError, match="float32"):
        boundary_loss(x, d.double())
    with pytest.raises(ValueError, match="floating point"):
        boundary_loss(x.long(), d)
    with pytest.raises(ValueError, match=r"\[N, K, H, W\]"):
        boundary_loss(x[0], d[0])
    with pytest.raises(ValueError, match="K must be 1..3"):
        boundary_loss(torch.zeros(2, 4, 4, 4), torch.zeros(2, 4, 4, 4))
    with pytest.raises(ValueError, match="softmax over K = 1"):
        boundary_loss(x[:, :1], d[:, :1].contiguous())
    with pytest.raises(ValueError, match="softmax over K = 1"):
        BoundaryLoss()(x[:, :1], d[:, :1].contiguous())
    with pytest.raises(ValueError, match="no gradient"):
        boundary_loss(x, d.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="does not match"):
        boundary_loss(x, d[:, :2].contiguous())
    with pytest.raises(ValueError, match="activation"):
        boundary_loss(x, d, activation="tanh")
    with pytest.raises(ValueError, match="class_weight"):
        boundary_loss(x, d, class_weight=(0.0, 1.0))


def test_boundary_loss_has_no_cpu_fallback():
    from eunet._lib import EunetError
    from eunet.losses import boundary_loss
    with pytest.raises(EunetError):
        boundary_loss(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4))
