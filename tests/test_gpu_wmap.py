"""weightmap.hip: the U-Net border weight map and the separation of touching instances on the GPU against
the fp64 restatement of tests/_wmap_ref.py (include/eunet.h is the definition).

border_weight_kernel works on T x T output tiles (T read from the source below) with an R-wide halo staged
in LDS, so the shapes sit on either side of a tile in each axis, degenerate to one row / column / pixel and
drop below R; the window edge is probed at exactly R and R + 1 along x, y and the diagonal.

Gates.  separate_instances: exact.  The map: |err| <= 16 2^-23 (1 + a) ref + 2^-23 max(1, w0) with
a = (d1 + d2)^2 / (2 sigma^2) -- the handful of fp32 roundings in forming the exponent, amplified by a, plus
expf; where the restatement's border term is exactly 0 the output is exactly base, and base is exact
everywhere.  Every check prints its worst ratio to that bound.
"""
import os
import re

import numpy as np
import pytest
import torch

import _wmap_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -23

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "enhanced-unet_amd", "csrc",
                   "weightmap.hip")
T = int(re.search(r"constexpr int WT = (\d+);", open(SRC).read()).group(1))
IDS = (3, 70000, 7, 65539, 12, 2 ** 31 + 5)  # 65539 = 3 + 2^16: a 16-bit staging would merge it with 3


def disc(lab, cy, cx, r, i):
    yy, xx = np.mgrid[0:lab.shape[-2], 0:lab.shape[-1]]
    lab[..., (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = i
    return lab


def scene(H, W, n, seed, rmax=4):
    rng = np.random.RandomState(seed)
    lab = np.zeros((H, W), np.int64)
    for j in range(n):
        disc(lab, rng.randint(0, H), rng.randint(0, W), rng.randint(0, rmax + 1), IDS[j % len(IDS)] + (j // len(IDS)) * 100)
    return lab


def check(name, lab, sem=None, **kw):
    """The kernel's map of lab (numpy int64 [H,W] or [N,H,W]) against the restatement; returns the GPU map."""
    from eunet import ops
    cw = kw.get("class_weight", (1.0, 1.0, 1.0))
    w0, sigma = kw.get("w0", 10.0), kw.get("sigma", 5.0)
    radius = kw.get("radius")
    ref, a = M.border_weight_map(lab, sem, cw, w0, sigma, "default" if radius is None else radius)
    base, _ = M.border_weight_map(lab, sem, cw, 0.0, sigma, 1)
    got = ops.border_weight_map(torch.from_numpy(lab).to(DEV), None if sem is None else torch.from_numpy(sem).to(DEV),
                                **kw)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == lab.shape
    out = got.double().cpu().numpy()
    assert np.isfinite(out).all(), name
    zero = ref == base  # the restatement's border term is exactly 0: cell pixels, < 2 ids in reach, underflow
    assert (out[zero] == base[zero]).all(), (name, "base must be exact where the border term is 0")
    bound = 16 * EPS * (1 + a) * ref + EPS * max(1.0, w0)
    ratio = float((np.abs(out - ref) / bound).max())
    print(f"{name}: {int((~zero).sum())} border px of {lab.size}, max m {ref.max():.6g}, worst |err| / bound {ratio:.3g}")
    assert ratio <= 1.0, (name, ratio)
    return out


@pytest.mark.parametrize("H,W", [(T - 1, T - 1), (T, T), (T + 1, T + 1), (T - 1, T + 1), (T + 1, T - 1), (T, 2 * T + 1),
                                 (1, 1), (1, 40), (40, 1), (9, 7)])
def test_shapes_around_the_tile(H, W):
    """sigma = 2 (R = 11): T - 1, T, T + 1 in each axis, one pixel, one row, one column, smaller than R."""
    lab = scene(H, W, 8, seed=H * 100 + W, rmax=2)
    if H == 1 or W == 1:
        lab[:] = 0
        flat = lab.reshape(-1)
        flat[3:6], flat[9:11], flat[-4:-1] = 3, 70000, 7
    out = check(f"{H}x{W}", lab, sigma=2.0)
    if H * W > 1:
        assert out.max() > 1.0  # the scene does have a border term
    check(f"{H}x{W} empty", np.zeros((H, W), np.int64), sigma=2.0)


@pytest.mark.parametrize("axis", ["x", "y", "diagonal"])
def test_window_edge_is_inclusive(axis):
    """Instance A next to the probe pixel, instance B at exactly R along the axis: a non-zero term.  B one pixel
    further: outside the window, fewer than two ids, exactly base.  R = 5, sigma = 3."""
    Rr, sigma, w0 = 5, 3.0, 10.0
    H = W = 2 * Rr + 5
    cy = cx = Rr + 2
    dy, dx = {"x": (0, 1), "y": (1, 0), "diagonal": (1, 1)}[axis]
    for off in (Rr, Rr + 1):
        lab = np.zeros((H, W), np.int64)
        lab[cy - dy, cx - dx] = 3
        lab[cy + dy * off, cx + dx * off] = 70000
        out = check(f"edge {axis} at {off}", lab, radius=Rr, sigma=sigma, w0=w0)
        d = np.hypot(dy, dx)
        if off == Rr:
            want = 1.0 + w0 * np.exp(-(d + d * Rr) ** 2 / (2 * sigma * sigma))
            assert out[cy, cx] > 1.0 and abs(out[cy, cx] - want) <= 1e-5 * want
        else:
            assert out[cy, cx] == 1.0


def test_same_id_twice_then_a_third_instance():
    """The two nearest cell pixels carry id 5; id 9 lies farther away: d1 = 1 (id 5), d2 = 4 (id 9)."""
    lab = np.zeros((15, 15), np.int64)
    lab[7, 6], lab[5, 7], lab[7, 11] = 5, 5, 9
    out = check("same id twice", lab, sigma=2.0, w0=10.0)
    want = 1.0 + 10.0 * np.exp(-(1 + 4) ** 2 / 8.0)
    assert abs(out[7, 7] - want) <= 1e-5 * want


def test_image_border_and_three_instances():
    lab = np.zeros((20, 26), np.int64)
    lab[0:3, 0:3], lab[0:2, 23:26], lab[18:20, 5:9], lab[8:11, 12:14] = 1, 2, 3, 70000
    check("image border", lab, sigma=3.0)


def test_id_70000_next_to_id_3_and_ids_apart_by_2_pow_16():
    lab = np.zeros((12, 20), np.int64)
    lab[4:8, 3:7], lab[4:8, 9:13], lab[4:8, 15:19] = 3, 70000, 65539
    out = check("large ids", lab, sigma=2.0)
    assert out[5, 8] > 2.0 and out[5, 14] > 2.0  # both gaps are borders between distinct instances


def test_batch_isolation_and_fewer_than_two_ids():
    lab = np.zeros((2, 40, 37), np.int64)
    lab[0] = scene(40, 37, 6, seed=5)
    out = check("N=2", lab, sigma=2.0)
    assert out[0].max() > 1.0 and (out[1] == 1.0).all()
    one = disc(np.zeros((1, 40, 37), np.int64), 20, 18, 6, 70000)
    assert (check("one instance", one, sigma=2.0) == 1.0).all()
    assert (check("no instance", np.zeros((1, 40, 37), np.int64)) == 1.0).all()
    # [H, W] is N = 1, and out= is written in place
    from eunet import ops
    buf = torch.full((40, 37), -1.0, device=DEV)
    res = ops.border_weight_map(torch.from_numpy(lab[0]).to(DEV), sigma=2.0, out=buf)
    assert res is buf and np.array_equal(buf.double().cpu().numpy(), out[0])


def test_semantic_class_weights():
    lab = scene(33, 35, 6, seed=9)
    sem = np.where(lab == 0, 0, np.where(lab % 2 == 1, 1, 2)).astype(np.int64)
    sem[0, 0] = 255  # neither 0, 1 nor 2: base 1
    sem[20, 20] = -1
    out = check("semantic", lab, sem, class_weight=(1.0, 3.0, 2.0), sigma=2.0)
    assert out[0, 0] >= 1.0 and set(np.unique(out[lab != 0])) <= {1.0, 2.0, 3.0}
    check("semantic bg weight", lab, sem, class_weight=(0.5, 3.0, 2.0), sigma=2.0, w0=4.0)


@pytest.mark.parametrize("radius,sigma", [(1, 5.0), (48, 5.0), (None, 0.5), (None, 8.0), (48, 20.0), (3, 0.5)])
def test_explicit_radius_and_sigma(radius, sigma):
    """radius 1 and 48 (64 KiB of staged labels), sigma 0.5 (R = 3, the exponent reaches a = 72) and 8 (R = 44)."""
    lab = scene(70, 130, 14, seed=17, rmax=5)
    lab[30, 60:65] = 0
    lab[30, 60:62], lab[30, 63:65] = 3, 7  # one background pixel between two instances: in reach of radius 1
    kw = dict(sigma=sigma) if radius is None else dict(sigma=sigma, radius=radius)
    out = check(f"radius {radius} sigma {sigma}", lab, **kw)
    assert out[30, 62] > 1.0


def test_large_multi_block_case():
    """257 x 300 (9 x 10 tiles) with 40 random discs, default radius at sigma = 5 (R = 28), N = 2."""
    lab = np.stack([scene(257, 300, 40, seed=23, rmax=10), scene(257, 300, 40, seed=24, rmax=10)])
    sem = np.where(lab == 0, 0, 1 + (lab % 2)).astype(np.int64)
    out = check("257x300", lab, sem, class_weight=(1.0, 3.0, 2.0))
    assert out.max() > 1.5


def test_refusals():
    from eunet import ops
    from eunet._lib import EunetError, WMAP_RADIUS_AUTO
    lab = torch.zeros(1, 8, 8, dtype=torch.int64, device=DEV)
    for kw in (dict(radius=0), dict(radius=49), dict(sigma=0.0), dict(sigma=-1.0), dict(w0=-1.0), dict(sigma=9.0)):
        with pytest.raises((ValueError, EunetError)):
            ops.border_weight_map(lab, **kw)
    # the library's own checks, past the Python layer
    out = torch.empty(1, 8, 8, device=DEV)
    for (w0, sigma, r) in ((10.0, 5.0, 0), (10.0, 5.0, 49), (10.0, 0.0, 5), (10.0, -1.0, WMAP_RADIUS_AUTO),
                           (-1.0, 5.0, 5), (10.0, 9.0, WMAP_RADIUS_AUTO), (10.0, float("nan"), 5)):
        with pytest.raises(EunetError):
            ops._border_weight_map_op(lab, None, 1.0, 1.0, 1.0, w0, sigma, r, out)
    with pytest.raises(EunetError):
        ops._separate_instances_op(lab, lab.clone(), torch.empty_like(lab), None)


# ---- separate_instances ----------------------------------------------------------------------------
def check_separate(name, lab, sem=None):
    from eunet import ops
    lo_ref, so_ref = M.separate(lab, sem)
    lt = torch.from_numpy(lab).to(DEV)
    st = None if sem is None else torch.from_numpy(sem).to(DEV)
    keep_l, keep_s = lt.clone(), None if st is None else st.clone()
    lo, so = ops.separate_instances(lt, st)
    torch.cuda.synchronize()
    assert torch.equal(lt, keep_l) and (st is None or torch.equal(st, keep_s)), name  # not in place
    assert lo.dtype == torch.int64 and np.array_equal(lo.cpu().numpy(), lo_ref), name
    if sem is None:
        assert so is None
    else:
        assert so.dtype == torch.int64 and np.array_equal(so.cpu().numpy(), so_ref), name
    return lo.cpu().numpy(), None if so is None else so.cpu().numpy()


def test_separate_abutting_rectangles():
    lab = np.zeros((9, 12), np.int64)
    lab[2:7, 1:6], lab[2:7, 6:11] = 3, 70000
    sem = np.where(lab == 3, 1, np.where(lab == 70000, 2, 0)).astype(np.int64)
    lo, so = check_separate("abutting", lab, sem)
    assert (lo[:, 5] == 0).all() and (lo[:, 6] == 0).all() and (so[:, 5:7] == 0).all()
    assert (lo[2:7, 1:5] == 3).all() and (lo[2:7, 7:11] == 70000).all() and (so[2:7, 1:5] == 1).all()


def test_separate_diagonal_contact_lone_cell_and_image_edge():
    lab = np.zeros((T + 3, T + 5), np.int64)
    lab[2:5, 2:5], lab[5:8, 5:8] = 4, 9          # touch at one corner only
    lab[12:16, 20:24] = 11                        # touches only the background
    lab[0:3, T:T + 2], lab[0:3, T + 2:T + 5] = 5, 6  # contact at the image edge (top row, right column)
    lab[T + 2, 0:4], lab[T + 2, 4:8] = 7, 2 ** 40 + 7  # bottom row; ids equal in their low 32 bits stay distinct
    sem = (lab > 0).astype(np.int64) * 2
    lo, so = check_separate("contacts", lab, sem)
    assert lo[4, 4] == 0 and lo[5, 5] == 0 and lo[3, 3] == 4 and lo[6, 6] == 9
    assert (lo[12:16, 20:24] == 11).all()
    assert (lo[0:3, T + 1] == 0).all() and (lo[0:3, T + 2] == 0).all() and lo[0, T] == 5 and lo[0, T + 4] == 6
    assert lo[T + 2, 3] == 0 and lo[T + 2, 4] == 0 and lo[T + 2, 2] == 7
    check_separate("no semantic", lab)
    check_separate("batch", np.stack([lab, np.zeros_like(lab), lab[::-1].copy()]), np.stack([sem, sem, sem[::-1].copy()]))
    check_separate("one pixel", np.array([[5]], np.int64), np.array([[1]], np.int64))
