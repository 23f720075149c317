"""The warp restatement (tests/_warp_ref.py) held to plain torch, and the host side of the feature: the affine
matrix, the option's validation, the binding table.  No GPU.

grid_sample takes normalised coordinates; with align_corners=True pixel s of an axis of n is 2 s / (n - 1) - 1,
its reflection padding mirrors about the centres of the first and last pixel (reflect-101), and all of it is
run in fp64 here, so what it adds to the comparison is of the order of 1e-12."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _warp_ref as R


def _normalised(grid, hi, wi):
    g = torch.from_numpy(np.asarray(grid, dtype=np.float64)).clone()
    g[..., 0] = 2.0 * g[..., 0] / (wi - 1) - 1.0
    g[..., 1] = 2.0 * g[..., 1] / (hi - 1) - 1.0
    return g[None]


def _sample(img_hwc, grid, mode, padding):
    x = torch.from_numpy(np.asarray(img_hwc, dtype=np.float64)).permute(2, 0, 1)[None]
    out = F.grid_sample(x, _normalised(grid, *img_hwc.shape[:2]), mode=mode, padding_mode=padding, align_corners=True)
    return out[0].permute(1, 2, 0).numpy()


def _map32(rng, ho, wo, lo, hi_, step=32):
    """A float32 map of multiples of 1 / step in [lo, hi_)."""
    q = rng.integers(int(lo * step), int(hi_ * step), (ho, wo, 2))
    return (q / float(step)).astype(np.float32)


@pytest.mark.parametrize("h,w,gh,gw", [(1, 1, 2, 2), (7, 5, 3, 3), (33, 65, 4, 7), (40, 24, 16, 16), (9, 1, 2, 5)])
def test_displacement_is_torch_bicubic_align_corners(h, w, gh, gw):
    rng = np.random.default_rng(h * 100 + w)
    ctrl = rng.normal(0, 10.0, (2, gh, gw))
    want = F.interpolate(torch.from_numpy(ctrl)[None], size=(h, w), mode="bicubic", align_corners=True)[0].numpy()
    got = R.displacement_ref(h, w, ctrl)
    assert np.abs(got - want).max() <= 1e-12
    m = np.array([[0.5, -0.25, 3.0], [0.125, 2.0, -7.0]])
    g = R.grid_ref(h, w, ctrl, m)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    assert np.abs(g[..., 0] - (0.5 * x - 0.25 * y + 3.0 + want[0])).max() <= 1e-12
    assert np.abs(g[..., 1] - (0.125 * x + 2.0 * y - 7.0 + want[1])).max() <= 1e-12
    assert np.array_equal(R.grid_ref(h, w, np.zeros((2, gh, gw)))[..., 0], x.astype(np.float64))


@pytest.mark.parametrize("hi,wi,c", [(7, 5, 1), (12, 9, 3), (2, 2, 4), (33, 17, 3)])
def test_bilinear_restatement_is_within_half_a_grey_level_of_grid_sample(hi, wi, c):
    rng = np.random.default_rng(hi + wi + c)
    img = rng.integers(0, 256, (hi, wi, c), dtype=np.uint8)
    # reflection: coordinates up to three sizes outside, so several reflections occur
    g = _map32(rng, 19, 23, -3 * max(hi, wi), 4 * max(hi, wi))
    got = R.warp_u8_ref(img, g, "reflect").astype(np.float64)
    assert np.abs(got - _sample(img, g, "bilinear", "reflection")).max() <= 0.5 + 1e-9
    # constant, fill 0: grid_sample's zero padding as it is
    got = R.warp_u8_ref(img, g, "constant", 0).astype(np.float64)
    assert np.abs(got - _sample(img, g, "bilinear", "zeros")).max() <= 0.5 + 1e-9
    # constant, fill 7 and 255: through an image padded with `fill`, on coordinates whose taps stay inside the padding
    for fill in (7, 255):
        k = 2
        g = _map32(rng, 19, 23, -k, min(hi, wi) - 1 + k)
        padded = np.full((hi + 2 * k, wi + 2 * k, c), fill, dtype=np.uint8)
        padded[k:-k, k:-k] = img
        got = R.warp_u8_ref(img, g, "constant", fill).astype(np.float64)
        assert np.abs(got - _sample(padded, g + np.float32(k), "bilinear", "zeros")).max() <= 0.5 + 1e-9


def test_bilinear_restatement_known_answers():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (6, 9, 3), dtype=np.uint8)
    y, x = np.meshgrid(np.arange(6), np.arange(9), indexing="ij")
    ident = np.stack([x, y], -1).astype(np.float32)
    for border in ("reflect", "constant"):
        assert np.array_equal(R.warp_u8_ref(img, ident, border, 9), img)
    # halfway between two pixels: (a + b + 1) >> 1 by the + 512 rounding
    half = ident[:, :8] + np.array([0.5, 0.0], dtype=np.float32)
    want = (img[:, :8].astype(np.int64) + img[:, 1:] + 1) >> 1
    assert np.array_equal(R.warp_u8_ref(img, half, "reflect"), want.astype(np.uint8))
    # non-finite coordinates are `fill` under both rules
    bad = ident.copy()
    bad[0, 0, 0], bad[1, 1, 1], bad[2, 2, 0] = np.nan, np.inf, -np.inf
    for border in ("reflect", "constant"):
        out = R.warp_u8_ref(img, bad, border, 7)
        assert (out[0, 0] == 7).all() and (out[1, 1] == 7).all() and (out[2, 2] == 7).all()
        assert np.array_equal(out[3:], img[3:])
        lab = R.warp_labels_ref(img[..., 0].astype(np.int64), bad, border, -5)
        assert lab[0, 0] == -5 and lab[1, 1] == -5 and lab[2, 2] == -5 and np.array_equal(lab[3:], img[3:, :, 0])


@pytest.mark.parametrize("hi,wi", [(7, 5), (12, 9), (2, 2)])
def test_nearest_restatement_is_grid_sample_nearest_away_from_half_integers(hi, wi):
    """Away from half-integers: quantising to 1/32 moves a coordinate by at most 1/64, so it cannot carry it across
    a rounding boundary that is further away than that (a coordinate exactly 1/64 below one can reach the tie;
    the random float32 coordinates used here never sit there)."""
    rng = np.random.default_rng(hi * wi)
    lab = rng.integers(0, 200, (hi, wi)).astype(np.int64)
    g = rng.uniform(-3.0 * max(hi, wi), 4.0 * max(hi, wi), (31, 29, 2)).astype(np.float32)
    far = (np.abs(g - np.floor(g) - 0.5) >= 1.0 / 64).all(-1)
    assert far.mean() > 0.8
    for border, padding in (("reflect", "reflection"), ("constant", "zeros")):
        want = _sample(lab[..., None].astype(np.float64), g, "nearest", padding)[..., 0]
        got = R.warp_labels_ref(lab, g, border, 0)
        assert np.array_equal(got[far], want[far].astype(np.int64))
    stack = rng.integers(0, 2, (3, hi, wi), dtype=np.uint8)
    got = R.warp_labels_ref(stack, g, "reflect", 0, flip_h=True, flip_v=True)
    for i in range(3):
        assert np.array_equal(got[i], R.warp_labels_ref(stack[i].astype(np.int64), g, "reflect")[::-1, ::-1])


def test_reflect_101_at_small_sizes_and_several_periods_out():
    for n in (2, 3, 5, 8):
        k = 5 * n  # np.pad(mode="reflect") mirrors about the edge pixels' centres, as often as it takes
        padded = np.pad(np.arange(n), (k, k), mode="reflect")
        i = np.arange(-k, n + k)
        r, inside = R.border_index(i, n, "reflect")
        assert inside.all() and np.array_equal(r, padded)
    r, _ = R.border_index(np.array([-3, -2, -1, 0, 1, 2, 3, 4]), 2, "reflect")
    assert r.tolist() == [1, 0, 1, 0, 1, 0, 1, 0]
    r, inside = R.border_index(np.array([-100, -1, 0, 1, 77]), 1, "reflect")
    assert r.tolist() == [0] * 5 and inside.all()
    r, inside = R.border_index(np.array([-1, 0, 4, 5]), 5, "constant")
    assert inside.tolist() == [False, True, True, False]
    # a 1 x 1 image under reflection is its one pixel everywhere; a 1 x n row repeats with period 2 (n - 1)
    one = np.array([[[42, 7]]], dtype=np.uint8)
    g = np.array([[[-50.25, 3.5], [1000.0, -7.0]]], dtype=np.float32)
    assert (R.warp_u8_ref(one, g, "reflect") == one).all()
    row = np.arange(4, dtype=np.int64)[None]
    g = np.stack([np.arange(-12, 13, dtype=np.float32), np.full(25, 9.0, dtype=np.float32)], -1)[None]
    assert R.warp_labels_ref(row, g, "reflect")[0].tolist() == [abs((i + 3) % 6 - 3) for i in range(-12, 13)]


def test_warp_matrix():
    from eunet.data import warp_matrix
    m = warp_matrix(96, 128, 0.0, 1.0)
    assert m.dtype == np.float64 and np.array_equal(m, np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]))
    # the centre is a fixed point; a quarter turn at scale 2 maps dst - c = (2, 0) to src - c = (0, 1)
    m = warp_matrix(9, 5, 90.0, 2.0)
    c = np.array([2.0, 4.0])
    assert np.abs(m @ np.array([2.0, 4.0, 1.0]) - c).max() <= 1e-12
    assert np.abs(m @ np.array([4.0, 4.0, 1.0]) - (c + [0.0, 1.0])).max() <= 1e-12
    m = warp_matrix(7, 7, 30.0, 0.5)
    r = np.deg2rad(30.0)
    assert np.abs(m[:, :2] - 2.0 * np.array([[np.cos(r), -np.sin(r)], [np.sin(r), np.cos(r)]])).max() <= 1e-15


@pytest.mark.parametrize("bad", [dict(sigmas=1.0), dict(sigma=-1.0), dict(p=1.5), dict(p=-0.1), dict(scale=(0.0, 1.0)),
                                 dict(scale=(1.2, 0.8)), dict(scale=(-1.0, 1.0)), dict(rotate=-5.0), dict(grid=1),
                                 dict(grid=17), dict(grid=(3, 40)), dict(border="wrap"), "reflect"])
def test_elastic_option_is_validated_on_the_host(tmp_path, bad):
    from eunet.data import CellDataset
    with pytest.raises(ValueError):
        CellDataset(str(tmp_path), split="train", device="cpu", elastic=bad)


def test_elastic_option_defaults_and_forms(tmp_path):
    from eunet.data import CellDataset
    assert CellDataset(str(tmp_path), device="cpu").elastic is None
    c = CellDataset(str(tmp_path), device="cpu", elastic={}).elastic
    assert c == dict(sigma=10.0, grid=(3, 3), rotate=0.0, scale=(1.0, 1.0), p=1.0, border="reflect", seed=None)
    c = CellDataset(str(tmp_path), device="cpu", elastic=dict(grid=(4, 7), sigma=0, p=0, border="constant", seed=3)).elastic
    assert c["grid"] == (4, 7) and c["sigma"] == 0.0 and c["p"] == 0.0 and c["border"] == "constant"


def test_ops_validate_on_the_host():
    from eunet import ops
    z = np.zeros((2, 3, 3), dtype=np.float32)
    for ctrl in (np.zeros((2, 1, 3)), np.zeros((2, 3, 17)), np.zeros((3, 3, 3)), np.full((2, 3, 3), np.nan),
                 np.full((2, 3, 3), np.inf)):
        with pytest.raises(ValueError):
            ops.elastic_grid(8, 8, ctrl, device="cpu")
    with pytest.raises(ValueError):
        ops.elastic_grid(8, 8, z, matrix=np.full((2, 3), np.nan), device="cpu")
    g = torch.zeros(4, 4, 2)
    with pytest.raises(ValueError):
        ops.warp_u8(torch.zeros(4, 4, 3, dtype=torch.uint8), g, border="wrap")
    with pytest.raises(ValueError):
        ops.warp_labels(torch.zeros(4, 4, dtype=torch.int64), g, border="edge")


def test_entry_points_are_bound():
    from eunet import _lib
    for name in ("eunet_warp_grid", "eunet_warp_u8", "eunet_warp_labels"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
