"""ops.elastic_grid / warp_u8 / warp_labels (csrc/warp.hip) against the restatement of tests/_warp_ref.py.

The map is held to the fp64 restatement, given the same float32-rounded control points and matrix, within
8 * 2^-23 * max(h, w, max |grid_ref|): an a-priori bound over the handful of fp32 operations at coordinate
magnitude (an fp32 emulation of the kernel's arithmetic on the CPU stays below 1 of those units with sigma = 10
displacements and below 4 with displacements of three image sizes; on the device 1.1 and 2.7 were measured,
profiles/warp_bench.txt).  The gathers are pure
functions of the fp32 map: they are evaluated on the device's own map, downloaded, and must equal the integer
restatement bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _warp_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (7, 5), (33, 65), (96, 128), (256, 256)]
CTRLS = [(2, 2), (3, 3), (4, 7), (16, 16)]
UNIT = 2.0 ** -23


def _matrix(h, w, angle, scale):
    from eunet.data import warp_matrix
    return warp_matrix(h, w, angle, scale)


def _ctrl(seed, gh, gw, sigma):
    return np.random.default_rng(seed).normal(0.0, sigma, (2, gh, gw)).astype(np.float32)


def _map_error(h, w, ctrl, m):
    """(device map, error in units of the bound's 2^-23 max(h, w, max |ref|))."""
    from eunet import ops
    got = ops.elastic_grid(h, w, ctrl, m, device=DEV)
    assert got.dtype == torch.float32 and got.shape == (h, w, 2) and got.device.type == DEV
    m32 = None if m is None else np.asarray(m, dtype=np.float32).astype(np.float64)
    ref = R.grid_ref(h, w, ctrl.astype(np.float64), m32)
    scale = UNIT * max(h, w, float(np.abs(ref).max()))
    return got, float(np.abs(got.double().cpu().numpy() - ref).max()) / scale


# every small shape with every control grid, and the one 256 x 256 case
MAP_CASES = [s + g for s in SHAPES[:-1] for g in CTRLS] + [(256, 256, 3, 3)]


@pytest.mark.parametrize("h,w,gh,gw", MAP_CASES, ids=lambda v: str(v))
def test_map_is_within_the_rounding_bound_of_the_fp64_restatement(h, w, gh, gw):
    worst = 0.0
    # the identity, rotations at scale 0.5 / 2 / 0.7, and displacements of three image sizes (the bound grows with them)
    for k, (angle, scale, sigma) in enumerate([(0.0, 1.0, 10.0), (33.0, 0.5, 4.0), (-10.0, 2.0, 2.0), (45.0, 0.7, 10.0),
                                               (45.0, 0.7, 3.0 * max(h, w))]):
        ctrl = _ctrl(h * 1000 + w * 10 + gh + k, gh, gw, sigma)
        _, err = _map_error(h, w, ctrl, None if k == 0 else _matrix(h, w, angle, scale))
        worst = max(worst, err)
    print(f"map {h}x{w} ctrl {gh}x{gw}: max error {worst:.3f} units of 2^-23 max(h, w, |grid|) (bound 8)")
    assert worst <= 8.0


@pytest.mark.parametrize("h,w,gh,gw", [(1, 1, 2, 2), (7, 5, 3, 3), (33, 65, 3, 5), (96, 128, 16, 16), (97, 129, 4, 7),
                                       (256, 256, 3, 3)])
def test_map_known_answers(h, w, gh, gw):
    from eunet import ops
    # zero displacements with the identity matrix (given or defaulted): exactly (x, y)
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    ident = torch.stack([x, y], -1).float()
    z = np.zeros((2, gh, gw), dtype=np.float32)
    assert torch.equal(ops.elastic_grid(h, w, z, device=DEV).cpu(), ident)
    assert torch.equal(ops.elastic_grid(h, w, torch.from_numpy(z).to(DEV), _matrix(h, w, 0.0, 1.0), device=DEV).cpu(), ident)
    # at the pixels that sit on control points the displacement is the control value
    ctrl = _ctrl(h + w, gh, gw, 10.0)
    got = (ops.elastic_grid(h, w, ctrl, device=DEV).cpu().double() - ident.double()).numpy()

    def points(n, g):  # (pixel, control index): 0, n - 1, and every control point when (n - 1) % (g - 1) == 0
        p = {(0, 0), (n - 1, g - 1 if n > 1 else 0)}
        if n > 1 and (n - 1) % (g - 1) == 0:
            p |= {(j * (n - 1) // (g - 1), j) for j in range(g)}
        return sorted(p)
    bound = 8 * UNIT * max(h, w, float(np.abs(R.grid_ref(h, w, ctrl.astype(np.float64))).max()))
    for py, cy in points(h, gh):
        for px, cx in points(w, gw):
            assert abs(got[py, px, 0] - ctrl[0, cy, cx]) <= bound and abs(got[py, px, 1] - ctrl[1, cy, cx]) <= bound


def _maps(ho, wo, hi, wi, seed):
    """Named device maps [ho, wo, 2] into a source of (hi, wi): rotation at scale 0.5 and 2, displacements of up to
    three sizes (several reflections), exact ties of the 1/32 rounding, and NaN / +-inf entries."""
    from eunet import ops
    rng = np.random.default_rng(seed)
    fit = np.array([[wi / wo, 0.0, 0.0], [0.0, hi / ho, 0.0]])  # the map's frame stretched over the source

    def affine(angle, scale):
        m = np.vstack([_matrix(ho, wo, angle, scale), [0.0, 0.0, 1.0]])
        return fit @ m
    span = 3.0 * max(hi, wi)
    maps = {"rot_half": ops.elastic_grid(ho, wo, _ctrl(seed, 3, 3, 4.0), affine(33.0, 0.5), device=DEV),
            "rot_two": ops.elastic_grid(ho, wo, _ctrl(seed + 1, 4, 7, 2.0), affine(-10.0, 2.0), device=DEV),
            "far": ops.elastic_grid(ho, wo, rng.uniform(-span, span, (2, 16, 16)).astype(np.float32), fit, device=DEV)}
    ties = (rng.integers(-64 * wi, 128 * wi, (ho, wo, 2)) / 64.0).astype(np.float32)
    maps["ties"] = torch.from_numpy(ties).to(DEV)
    bad = maps["far"].cpu().numpy().copy()
    flat = bad.reshape(-1)
    for j, v in enumerate((np.nan, np.inf, -np.inf, 3e38, -3e38, 1048576.0, -1048577.0)):
        flat[(j * 5) % flat.size] = v
    maps["bad"] = torch.from_numpy(bad).to(DEV)
    return maps


GATHER_CASES = [(1, 1, 1, 1), (7, 5, 7, 5), (33, 65, 33, 65), (96, 128, 96, 128), (256, 256, 256, 256),
                (7, 5, 33, 65), (33, 65, 7, 5)]  # (ho, wo, hi, wi): the last two have a source larger / smaller than the map


U8_CASES = [g + (c,) for g in GATHER_CASES for c in (1, 3, 4) if g[0] != 256 or c == 3]


@pytest.mark.parametrize("ho,wo,hi,wi,c", U8_CASES, ids=lambda v: str(v))
def test_warp_u8_equals_the_integer_restatement(ho, wo, hi, wi, c):
    from eunet import ops
    rng = np.random.default_rng(ho * wo + c)
    img = rng.integers(0, 256, (hi, wi, c), dtype=np.uint8)
    dimg = torch.from_numpy(img).to(DEV)
    for name, g in _maps(ho, wo, hi, wi, seed=hi + wo + c).items():
        gh = g.cpu().numpy()
        for border in ("reflect", "constant"):
            for fill in (0, 7, 255):
                if border == "reflect" and fill == 7 and name != "bad":
                    continue  # fill shows under reflection only at non-finite coordinates
                got = ops.warp_u8(dimg, g, border=border, fill=fill)
                assert got.dtype == torch.uint8 and got.shape == (ho, wo, c)
                want = torch.from_numpy(R.warp_u8_ref(img, gh, border, fill))
                assert torch.equal(got.cpu(), want), (name, border, fill, int((got.cpu() != want).sum()))


@pytest.mark.parametrize("ho,wo,hi,wi", GATHER_CASES, ids=lambda v: str(v))
def test_warp_labels_equals_the_integer_restatement(ho, wo, hi, wi):
    from eunet import ops
    rng = np.random.default_rng(ho + wo * hi)
    ids = rng.integers(-3, 40, (hi, wi)).astype(np.int64)
    ids[0, 0] = (1 << 40) + 5  # all 64 bits travel
    stacks = {n: rng.integers(0, 256, (n, hi, wi), dtype=np.uint8) for n in (0, 1, 5)}
    for name, g in _maps(ho, wo, hi, wi, seed=ho + wi).items():
        gh = g.cpu().numpy()
        for border in ("reflect", "constant"):
            for fill in (0, 7, 255):
                got = ops.warp_labels(torch.from_numpy(ids).to(DEV), g, border=border, fill=fill)
                want = R.warp_labels_ref(ids, gh, border, fill)
                assert got.dtype == torch.int64 and torch.equal(got.cpu(), torch.from_numpy(want)), (name, border, fill)
                # every output label occurs in the source, or is fill
                assert set(np.unique(got.cpu().numpy()).tolist()) <= set(np.unique(ids).tolist()) | {fill}
                for n, st in stacks.items():
                    got = ops.warp_labels(torch.from_numpy(st).to(DEV), g, border=border, fill=fill)
                    assert got.dtype == torch.uint8 and got.shape == (n, ho, wo)
                    assert torch.equal(got.cpu(), torch.from_numpy(R.warp_labels_ref(st, gh, border, fill))), (name, border, fill, n)
        for fh, fv in ((True, False), (False, True), (True, True)):
            dims = [d for d, f in ((-1, fh), (-2, fv)) if f]
            for x in (torch.from_numpy(ids).to(DEV), torch.from_numpy(stacks[5]).to(DEV)):
                plain = ops.warp_labels(x, g, border="reflect")
                assert torch.equal(ops.warp_labels(x, g, border="reflect", flip_h=fh, flip_v=fv), plain.flip(dims)), (name, fh, fv)


@pytest.mark.parametrize("h,w,c", [(7, 5, 3), (33, 65, 1), (96, 128, 4), (64, 64, 3)])
def test_exact_known_answers(h, w, c):
    from eunet import ops
    rng = np.random.default_rng(h + w + c)
    img = torch.from_numpy(rng.integers(0, 256, (h, w, c), dtype=np.uint8)).to(DEV)
    ids = torch.from_numpy(rng.integers(0, 1 << 33, (h, w))).to(DEV)
    stack = torch.from_numpy(rng.integers(0, 256, (3, h, w), dtype=np.uint8)).to(DEV)
    z = np.zeros((2, 2, 2), dtype=np.float32)
    ident = ops.elastic_grid(h, w, z, device=DEV)
    for border in ("reflect", "constant"):
        assert torch.equal(ops.warp_u8(img, ident, border=border, fill=9), img)
        assert torch.equal(ops.warp_labels(ids, ident, border=border, fill=9), ids)
        assert torch.equal(ops.warp_labels(stack, ident, border=border, fill=9), stack)
    # an integer translation under the constant border: the shifted image with fill outside
    tx, ty = 3, -2
    shift = ops.elastic_grid(h, w, z, np.array([[1.0, 0.0, tx], [0.0, 1.0, ty]]), device=DEV)
    want_img = torch.full_like(img, 7)
    want_ids = torch.full_like(ids, 7)
    y0, y1, x0, x1 = max(0, -ty), min(h, h - ty), max(0, -tx), min(w, w - tx)
    if y1 > y0 and x1 > x0:
        want_img[y0:y1, x0:x1] = img[y0 + ty:y1 + ty, x0 + tx:x1 + tx]
        want_ids[y0:y1, x0:x1] = ids[y0 + ty:y1 + ty, x0 + tx:x1 + tx]
    assert torch.equal(ops.warp_u8(img, shift, border="constant", fill=7), want_img)
    assert torch.equal(ops.warp_labels(ids, shift, border="constant", fill=7), want_ids)
    if h == w:  # an exact quarter turn: out[y, x] = src[x, n - 1 - y]
        turn = ops.elastic_grid(h, w, z, np.array([[0.0, -1.0, h - 1.0], [1.0, 0.0, 0.0]]), device=DEV)
        assert torch.equal(ops.warp_u8(img, turn, border="constant"), torch.rot90(img, 1, (0, 1)))
        assert torch.equal(ops.warp_labels(ids, turn), torch.rot90(ids, 1, (0, 1)))
        assert torch.equal(ops.warp_labels(stack, turn), torch.rot90(stack, 1, (1, 2)))


def test_bad_arguments_raise():
    from eunet import EunetError, ops
    g = torch.zeros(4, 4, 2, device=DEV)
    img = torch.zeros(4, 4, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        ops.warp_u8(img, g, border="wrap")
    with pytest.raises(ValueError):
        ops.warp_u8(img, g, fill=256)
    with pytest.raises(ValueError):
        ops.warp_u8(torch.zeros(4, 4, 5, dtype=torch.uint8, device=DEV), g)
    with pytest.raises(ValueError):
        ops.warp_labels(torch.zeros(4, 4, dtype=torch.int32, device=DEV), g)
    with pytest.raises(ValueError):
        ops.warp_labels(torch.zeros(1, 4, 4, dtype=torch.uint8, device=DEV), g, fill=300)
    with pytest.raises(ValueError):
        ops.elastic_grid(4, 4, torch.zeros(2, 17, 3, device=DEV))
    with pytest.raises((EunetError, ValueError)):
        ops.warp_u8(img.cpu(), g.cpu())


CHILD = r'''
import sys
import numpy as np
import torch
sys.path[:0] = [ROOT, ROOT + "/enhanced-unet_amd", ROOT + "/tests"]
import _warp_ref as R
from eunet import _lib, ops
assert _lib.load().eunet_debug_enabled() == 1, "not the debug build"
assert _lib.debug_status(reset=True) == (0, 0)
rng = np.random.default_rng(5)
for (ho, wo, hi, wi, c) in ((7, 5, 7, 5, 3), (33, 65, 7, 5, 1), (7, 5, 33, 65, 4), (96, 128, 96, 128, 3), (3, 4, 1, 1, 3)):
    span = 3.0 * max(hi, wi)
    g = ops.elastic_grid(ho, wo, rng.uniform(-span, span, (2, 16, 16)).astype(np.float32),
                         np.array([[0.4, -0.9, 2.0], [0.9, 0.4, -3.0]]), device="cuda")
    gh = g.cpu().numpy().copy()
    for j, v in enumerate((np.nan, np.inf, -np.inf, 3e38, -3e38, 1048576.0, -1048577.0)):
        gh.reshape(-1)[(j * 5) % gh.size] = v
    g = torch.from_numpy(gh).cuda()
    img = rng.integers(0, 256, (hi, wi, c), dtype=np.uint8)
    ids = rng.integers(0, 9, (hi, wi)).astype(np.int64)
    st = rng.integers(0, 2, (5, hi, wi), dtype=np.uint8)
    for border in ("reflect", "constant"):
        assert np.array_equal(ops.warp_u8(torch.from_numpy(img).cuda(), g, border=border, fill=7).cpu().numpy(),
                              R.warp_u8_ref(img, gh, border, 7))
        assert np.array_equal(ops.warp_labels(torch.from_numpy(ids).cuda(), g, border=border, fill=7, flip_h=True).cpu().numpy(),
                              R.warp_labels_ref(ids, gh, border, 7, flip_h=True))
        assert np.array_equal(ops.warp_labels(torch.from_numpy(st).cuda(), g, border=border, fill=7, flip_v=True).cpu().numpy(),
                              R.warp_labels_ref(st, gh, border, 7, flip_v=True))
    st = _lib.debug_status()
    print((ho, wo, hi, wi, c), "debug status", st)
    assert st == (0, 0), st
print("DEBUG_OK")
'''


def test_debug_build_reports_no_failed_index_check_on_out_of_range_coordinates():
    """The bounds-checked library (EUNET_DASSERT on every gathered index) on maps that leave the source by several
    sizes and hold NaN / +-inf: same results, no failed check.  Selected as tests/test_gpu_debug.py does."""
    lib = os.path.join(ROOT, "enhanced-unet_amd", "eunet", "libeunet_hip_debug.so")
    assert os.path.exists(lib), "build it: make -C enhanced-unet_amd debug"
    r = subprocess.run([sys.executable, "-c", CHILD.replace("ROOT", repr(ROOT))], env=dict(os.environ, EUNET_LIB=lib),
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "DEBUG_OK" in r.stdout
