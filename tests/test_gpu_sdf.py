"""sdf.hip, the signed distance map: ops.signed_distance_map against the brute-force restatement of tests/_sdf_ref.py.

The map is two exact integer transforms (boundary.hip's, tested in tests/test_gpu_boundary.py) and one elementwise
kernel: a thread takes 4 pixels and 16-byte accesses when H*W is a multiple of 4 and one pixel otherwise, reads the
per-(sample, class) emptiness from element 0 of both planes, and takes the square root in fp64.  The shapes: 1x1; a
single row and a single column (the transform's passes degenerate); 5x7 (scalar path); 1023, 1024 and 1025 pixels (the
scalar path twice, the vector path at 1024, and 5 blocks of 256 threads at 1025); 64x64 discs with an ignored stripe; a
batch whose samples have an empty and a full class next to a normal one.

Bound: the fp64 square root of an exact integer is correctly rounded and is rounded to fp32 once on both sides, so
equality is expected and at most 1 fp32 ulp is allowed; exactly 0 where the definition says 0 and exactly
+-float32(scale * clip) where clamped.  Every case prints its worst deviation in ulps."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _sdf_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
IGN = 255
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 37), (37, 1), (5, 7), (31, 33), (32, 32), (25, 41)]
PREP = [(None, 1.0), (3.0, 0.25)]  # (clip, scale)


def _check(name, target, K, ignore_index=None, clip=None, scale=1.0):
    """target int64 numpy [N, H, W]; returns the device result."""
    from eunet import ops
    ref, raw, clamped = S.signed_distance(target, K, ignore_index, clip, scale)
    got_d = ops.signed_distance_map(torch.from_numpy(target).to(DEV), K, ignore_index=ignore_index, clip=clip,
                                    scale=scale)
    got = got_d.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert np.isfinite(got).all(), name
    ulps = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.maximum(np.abs(ref), np.float32(1e-30)))
    worst = float(ulps.max())
    print(f"{name}: worst deviation {worst:.3g} ulp, {int(clamped.sum())} clamped, {int((raw == 0).sum())} zeros")
    assert worst <= 1.0, (name, worst)
    assert not got[raw == 0.0].any(), name  # exactly 0 where the definition says 0
    if clip is not None:
        edge = np.float32(np.float64(np.float32(scale)) * np.float64(np.float32(clip)))
        assert (got[clamped] == np.where(raw[clamped] > 0, edge, -edge)).all(), name
    return got_d


@pytest.mark.parametrize("clip,scale", PREP)
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_classes_and_preparation(H, W, K, clip, scale):
    """N = 3 maps of 5x5 blocks.  K = 1 draws from {0, 1, 2}: 2 is foreground too."""
    t = S.blobs(3, H, W, (0, 1, 2) if K == 1 else tuple(range(K)), seed=100 * H + W + K)
    if K == 1 and H * W > 25:
        assert (t == 2).any()
    _check(f"{H}x{W} K{K} clip {clip} scale {scale}", t, K, clip=clip, scale=scale)


@pytest.mark.parametrize("K", [1, 3])
def test_discs_with_an_ignored_stripe(K):
    """One 64x64 map of a few discs (two of them touching, one cut by the border) and a 3-pixel ignored stripe
    through them: the stripe is 0 in every plane and a site of every complement."""
    t = S.discs(64, 64, [(14, 14, 9), (14, 30, 8), (44, 40, 13), (60, 8, 7)])
    t[S.discs(64, 64, [(44, 40, 5)]) == 1] = 2
    t[:, 20:23] = IGN
    got = _check(f"discs K{K}", t[None], K, ignore_index=IGN).cpu()
    assert float(got[0, :, :, 20:23].abs().max()) == 0.0
    _check(f"discs K{K} clipped", t[None], K, ignore_index=IGN, clip=3.0, scale=0.25)


@pytest.mark.parametrize("K", [1, 2, 3])
def test_empty_and_full_class_next_to_a_normal_sample(K):
    """25x41, N = 3: sample 0 is normal, the last class never occurs in sample 1, sample 2 is one class throughout
    (that class is full, every other empty).  The per-(sample, class) flag zeroes exactly those planes."""
    t = S.blobs(3, 25, 41, (0, 1, 2) if K == 1 else tuple(range(K)), seed=7 + K)
    t[1][t[1] == (K - 1 if K > 1 else 2)] = 0
    if K == 1:
        t[1] = 0  # no foreground at all
    t[2] = 1 if K > 1 else 2
    got = _check(f"empty/full K{K}", t, K).cpu()
    assert float(got[0].abs().max()) > 0.0
    assert float(got[2].abs().max()) == 0.0
    assert float(got[1, K - 1].abs().max()) == 0.0
    if K == 3:
        assert float(got[1, 0].abs().max()) > 0.0  # the other planes of that sample are live


def test_fully_ignored_sample_is_zero():
    t = S.blobs(2, 9, 12, (0, 1), seed=3)
    t[1] = IGN
    got = _check("ignored sample", t, 2, ignore_index=IGN).cpu()
    assert float(got[1].abs().max()) == 0.0 and float(got[0].abs().max()) > 0.0


def test_out_buffer_single_map_and_bit_identical_runs():
    from eunet import ops
    t = torch.from_numpy(S.blobs(3, 32, 32, (0, 1, 2), seed=5)).to(DEV)
    a = ops.signed_distance_map(t, 3, clip=3.0, scale=0.25)
    b = ops.signed_distance_map(t, 3, clip=3.0, scale=0.25)
    out = torch.full((3, 3, 32, 32), float("nan"), device=DEV)
    c = ops.signed_distance_map(t, 3, clip=3.0, scale=0.25, out=out)
    assert c is out
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), out.view(torch.int32))
    single = ops.signed_distance_map(t[1], 3, clip=3.0, scale=0.25)
    assert single.shape == (3, 32, 32) and torch.equal(single, a[1])
    with pytest.raises(ValueError):
        ops.signed_distance_map(t, 3, out=torch.empty(3, 2, 32, 32, device=DEV))
    with pytest.raises(ValueError):
        ops.signed_distance_map(t.cpu(), 3)


def test_library_refuses_bad_arguments():
    from eunet import ops
    from eunet._lib import EunetError
    t = torch.zeros(1, 4, 4, dtype=torch.int64, device=DEV)
    ws = torch.empty(ops.signed_distance_workspace_bytes(1, 3, 4, 4) // 4, dtype=torch.int32, device=DEV)
    assert ws.numel() == 2 * 3 * 16
    assert ops.signed_distance_workspace_bytes(1, 1, 4, 4) == 2 * 16 * 4 + 16 * 8
    out = torch.empty(1, 3, 4, 4, device=DEV)
    for k, ign, clip, scale in ((4, -1, 0.0, 1.0), (3, 1, 0.0, 1.0), (3, -1, -1.0, 1.0), (3, -1, float("inf"), 1.0),
                                (3, -1, 0.0, float("nan"))):
        with pytest.raises(EunetError):
            ops.signed_distance(t, k, ign, clip, scale, ws, out)


DEBUG_CHILD = r'''
import sys, numpy as np, torch
sys.path[:0] = [ROOT, ROOT + "/enhanced-unet_amd", ROOT + "/tests"]
from eunet import _lib, ops
from eunet.losses import boundary_loss
import _sdf_ref as S
assert _lib.load().eunet_debug_enabled() == 1, "not the debug build"
assert _lib.debug_status(reset=True) == (0, 0)
for h, w in SHAPES:
    for K in (1, 2, 3):
        t = torch.from_numpy(S.blobs(3, h, w, (0, 1, 2) if K == 1 else tuple(range(K)), seed=h * 31 + w))
        t.view(-1)[::11] = 255
        phi = ops.signed_distance_map(t.to("cuda"), K, ignore_index=255, clip=3.0, scale=0.25)
        for act in ("sigmoid",) + (("softmax",) if K > 1 else ()):
            x = torch.randn(3, K, h, w, device="cuda", requires_grad=True)
            boundary_loss(x, phi, activation=act).backward()
    st = _lib.debug_status()
    print((h, w), "debug status", st)
    assert st == (0, 0), (h, w, st)
print("DEBUG_OK")
'''


def test_debug_build_bounds_checks_pass():
    """The kernels' EUNET_DASSERT index checks (the bounds-checked debug build) stay silent on every shape above, for
    the map and for both directions of the loss."""
    lib = os.path.join(ROOT, "enhanced-unet_amd", "eunet", "libeunet_hip_debug.so")
    assert os.path.exists(lib), "build it: make -C enhanced-unet_amd debug"
    child = DEBUG_CHILD.replace("ROOT", repr(ROOT)).replace("SHAPES", repr(SHAPES + [(64, 64), (513, 512)]))
    r = subprocess.run([sys.executable, "-c", child], env=dict(os.environ, EUNET_LIB=lib), capture_output=True,
                       text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "DEBUG_OK" in r.stdout
