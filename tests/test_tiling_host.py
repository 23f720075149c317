"""Overlap-tile inference, the part that needs no GPU: the plan's geometry (eunet.tiling) against the
plain-loop restatement (tests/_tiling_ref.py), every refusal, the C-ABI surface, and the receptive margin
measured on the fp64 oracle."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _tiling_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _total_weight(p):
    tot = np.zeros((p.hp, p.wp), np.float64)
    for iy, oy in enumerate(p.origins(0)):
        for ix, ox in enumerate(p.origins(1)):
            tot[oy:oy + p.th, ox:ox + p.tw] += np.outer(p.weights(0, iy).astype(np.float64),
                                                        p.weights(1, ix).astype(np.float64))
    return tot


# (h, w, tile, kwargs) -> (hp, wp, th, tw, stride, origins_y, origins_x)
GEOMETRIES = [
    # an image no larger than the tile: one tile of the padded size
    ((100, 120, 256, {}), (128, 128, 128, 128, 128, (0,), (0,))),
    ((256, 256, 256, {}), (256, 256, 256, 256, 128, (0,), (0,))),
    # one tile along one axis only (rows fit, columns do not); tiles are not square
    ((150, 500, 256, {}), (160, 512, 160, 256, 128, (0,), (0, 128, 256))),
    # the end-to-end GPU test's geometry: 2 x 3 tiles, flush edges and an interior column
    ((250, 300, 192, {}), (256, 320, 192, 192, 64, (0, 64), (0, 64, 128))),
    # L - tile no multiple of S: the last tile is pulled back flush with the edge; h, w no multiples of 32
    ((70, 101, 64, dict(margin=0)), (96, 128, 64, 64, 64, (0, 32), (0, 64))),
    ((70, 101, 64, dict(margin=16)), (96, 128, 64, 64, 32, (0, 32), (0, 32, 64))),
    ((300, 420, 256, dict(margin=48)), (320, 448, 256, 256, 160, (0, 64), (0, 160, 192))),
    # the blended modes: S = max(32, 32 floor(tile (1 - overlap) / 32))
    ((70, 101, 64, dict(blend="constant")), (96, 128, 64, 64, 32, (0, 32), (0, 32, 64))),
    ((70, 101, 64, dict(blend="gaussian", overlap=0.0)), (96, 128, 64, 64, 64, (0, 32), (0, 64))),
    ((333, 777, 160, dict(blend="gaussian", overlap=0.5)), (352, 800, 160, 160, 64, (0, 64, 128, 192),
                                                            (0, 64, 128, 192, 256, 320, 384, 448, 512, 576, 640))),
    ((200, 200, 96, dict(blend="constant", overlap=0.9)), (224, 224, 96, 96, 32, (0, 32, 64, 96, 128),
                                                           (0, 32, 64, 96, 128))),
]


@pytest.mark.parametrize("args,want", GEOMETRIES)
def test_plan_geometry(args, want):
    from eunet import tiling
    h, w, tile, kw = args
    p = tiling.plan(h, w, tile, **kw)
    hp, wp, th, tw, stride, oys, oxs = want
    assert (p.h, p.w, p.hp, p.wp, p.th, p.tw, p.stride) == (h, w, hp, wp, th, tw, stride)
    assert p.origins(0) == oys and p.origins(1) == oxs
    assert (p.ny, p.nx, p.n) == (len(oys), len(oxs), len(oys) * len(oxs))
    # the restatement's loops give the same origins
    assert tuple(T.origins(hp, th, stride)) == oys and tuple(T.origins(wp, tw, stride)) == oxs
    for L, e, os_ in ((hp, th, oys), (wp, tw, oxs)):
        assert all(o % 32 == 0 and 0 <= o and o + e <= L for o in os_)
        assert os_[0] == 0 and os_[-1] == L - e
        assert all(0 < b - a <= stride for a, b in zip(os_, os_[1:]))
    assert [p.origin(n) for n in range(p.n)] == [(oy, ox) for oy in oys for ox in oxs]
    with pytest.raises(IndexError):
        p.origin(p.n)
    tot = _total_weight(p)
    assert tot.min() > 0.0  # full positive coverage
    if p.blend == "crop":
        assert set(np.unique(tot)) <= {1.0, 2.0, 4.0}
        for axis, n in ((0, p.ny), (1, p.nx)):  # at most two cores overlap per axis
            L, e = ((p.hp, p.th), (p.wp, p.tw))[axis]
            cover = np.zeros(L)
            for i, o in enumerate(p.origins(axis)):
                cover[o:o + e] += p.weights(axis, i)
            assert set(np.unique(cover)) <= {1.0, 2.0}
    # the plan's weights are the restatement's
    for axis, n in ((0, p.ny), (1, p.nx)):
        L, e = ((p.hp, p.th), (p.wp, p.tw))[axis]
        for i, o in enumerate(p.origins(axis)):
            ref = T.axis_weights(p.blend, L, e, o, p.margin, p.table(axis)).numpy()
            assert np.array_equal(p.weights(axis, i).astype(np.float64), ref)
    assert p.inflation == pytest.approx(p.n * th * tw / (hp * wp))


def test_crop_weight_sums_take_all_three_values():
    from eunet import tiling
    tot = _total_weight(tiling.plan(70, 101, 64, margin=0))  # the clamped last tile overlaps its neighbour
    assert set(np.unique(tot)) == {1.0, 2.0}
    tot = _total_weight(tiling.plan(320, 320, 192, margin=16))  # origins 0, 128: cores [0,176) and [144,320)
    assert set(np.unique(tot)) == {1.0, 2.0, 4.0}


def test_default_margin_and_inflation():
    from eunet import tiling
    assert tiling.RECEPTIVE_MARGIN == 64
    p = tiling.plan(2048, 2048, 512)
    assert (p.margin, p.stride, p.ny, p.nx) == (64, 384, 5, 5)
    assert round(p.inflation, 2) == 1.56
    p = tiling.plan(2048, 2048, 1024)
    assert (p.stride, p.ny, p.nx) == (896, 3, 3) and round(p.inflation, 2) == 2.25


def test_gaussian_table_is_the_closed_form_in_fp32():
    from eunet import tiling
    p = tiling.plan(333, 777, 160, blend="gaussian", overlap=0.5, sigma_scale=0.125)
    for axis in (0, 1):
        tab = p.table(axis)
        assert tab.dtype == np.float32 and tab.shape == (160,)
        ref = np.array(T.gauss_closed_form(160, 0.125))
        # z = (t - c) / s carries 4 fp32 roundings (c, s, the difference, the quotient), z z twice that plus
        # one; the exponent reaches 8 at the tile edge, so its absolute error is <= 8 * 9 * 2^-24, which is the
        # relative error of exp; 2 more for expf and the store
        assert np.all(np.abs(tab - ref) <= 74 * 2.0 ** -24 * ref)
        assert tab.min() > 0.0 and tab.max() <= 1.0
    assert tiling.plan(64, 64, 64, margin=0).table(0) is None


@pytest.mark.parametrize("kw,match", [
    (dict(h=100, w=100, tile=100), "multiple of 32"),
    (dict(h=100, w=100, tile=0), "multiple of 32"),
    (dict(h=100, w=100, tile=256, margin=24), "multiple of 16"),
    (dict(h=100, w=100, tile=256, margin=-16), "multiple of 16"),
    (dict(h=100, w=100, tile=128, margin=64), "too small for margin"),
    (dict(h=100, w=100, tile=64), "too small for margin"),  # the default margin
    (dict(h=100, w=100, tile=128, blend="linear"), "blend must be one of"),
    (dict(h=100, w=100, tile=128, blend="constant", overlap=1.0), "overlap"),
    (dict(h=100, w=100, tile=128, blend="gaussian", sigma_scale=0.0), "sigma_scale"),
    (dict(h=16, w=100, tile=128, margin=0), "reflect-padded"),  # F.pad refuses 16 rows of padding on 16 rows
    (dict(h=100, w=5, tile=128, margin=0), "reflect-padded"),
    (dict(h=0, w=5, tile=128), "at least 1 x 1"),
])
def test_plan_refusals(kw, match):
    from eunet import tiling
    kw = dict(kw)
    h, w, tile = kw.pop("h"), kw.pop("w"), kw.pop("tile")
    with pytest.raises(ValueError, match=match):
        tiling.plan(h, w, tile, **kw)


def test_reflect_refusal_is_torchs():
    """plan refuses exactly where F.pad(mode="reflect") does: padding >= the dimension."""
    from eunet import tiling
    for h in (15, 16, 17, 31, 33):
        pad = (32 - h % 32) % 32
        try:
            F.pad(torch.zeros(1, 1, h, 64), (0, 0, 0, pad), mode="reflect")
            torch_ok = True
        except RuntimeError:
            torch_ok = False
        try:
            tiling.plan(h, 64, 64, margin=0)
            plan_ok = True
        except ValueError:
            plan_ok = False
        assert plan_ok == torch_ok, h


def test_evaluator_refusals_and_surface():
    from eunet.evaluator import Evaluator
    from eunet.models import EnhancedUNet, UNet
    sig = inspect.signature(Evaluator.__init__)
    for name, default in (("tile", None), ("tile_blend", "crop"), ("tile_margin", None), ("tile_overlap", 0.25),
                          ("tile_batch", 4)):
        assert sig.parameters[name].default == default and sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(Evaluator.predict_probs).parameters) == ["self", "image"]
    m = UNet(num_classes=3, base_ch=16)
    assert Evaluator(m, "cpu", "unet").tile is None
    assert Evaluator(m, "cpu", "unet", tile=192).tile == 192
    for kw, match in ((dict(tile=100), "multiple of 32"), (dict(tile=192, tile_margin=24), "multiple of 16"),
                      (dict(tile=128), "too small for margin"), (dict(tile=192, tile_blend="feather"), "blend must be"),
                      (dict(tile=192, tile_batch=0), "tile_batch")):
        with pytest.raises(ValueError, match=match):
            Evaluator(m, "cpu", "unet", **kw)
    dual = EnhancedUNet(num_classes=3, base_ch=16, dual_branch=True)
    with pytest.raises(ValueError, match="dual-branch"):
        Evaluator(dual, "cpu", "enhanced_unet", tile=192)
    assert Evaluator(dual, "cpu", "enhanced_unet").tile is None  # untiled stays allowed


def test_ops_refusals_need_no_gpu():
    from eunet import ops, tiling
    p = tiling.plan(70, 101, 64, margin=16)
    with pytest.raises(ValueError, match="plan is for"):
        ops.tile_gather(torch.zeros(3, 70, 100), p)
    with pytest.raises(ValueError, match="not inside the plan"):
        ops.tile_gather(torch.zeros(3, 70, 101), p, first=4, count=3)
    with pytest.raises(ValueError, match="activation"):
        ops.tile_blend(torch.zeros(p.n, 3, 64, 64), p, "tanh")
    with pytest.raises(ValueError, match="logits must be"):
        ops.tile_blend(torch.zeros(p.n - 1, 3, 64, 64), p, "softmax")


def test_c_abi_surface():
    from eunet import _lib, ops
    src = open(os.path.join(ROOT, "include", "eunet.h")).read()
    lib = _lib.load()
    for name in ("eunet_tile_gather", "eunet_tile_blend"):
        assert re.search(r"^int\s+" + name + r"\s*\(", src, flags=re.M), name
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name in _lib.exported_symbols()
        assert name[len("eunet_"):] in ops.DISPATCHED
    at = src.index("int eunet_tile_gather")
    comment = src[src.rindex("/*", 0, at):at]
    assert "no reference line" in comment and "increasing tile number" in comment and "2 (n - 1) - r" in comment
    assert "10 tiling" in src  # the debug build's unit list
    for c_name, value in (("EUNET_TILE_CROP", 0), ("EUNET_TILE_CONSTANT", 1), ("EUNET_TILE_GAUSSIAN", 2),
                          ("EUNET_TILE_ACT_NONE", 0), ("EUNET_TILE_ACT_SOFTMAX", 1), ("EUNET_TILE_ACT_SIGMOID", 2)):
        assert re.search(rf"#define {c_name} {value}\b", src), c_name
    from eunet import tiling
    assert tiling.BLENDS == ("crop", "constant", "gaussian")
    assert ops.TILE_ACTIVATIONS == {"none": 0, "softmax": 1, "sigmoid": 2}
    sch = str(torch.ops.eunet.tile_gather.default._schema)
    assert sch.startswith("eunet::tile_gather(Tensor image, int hp, int wp, int th, int tw, int sy, int sx, int first, "
                          "int count, Tensor(a!) out)"), sch


def test_c_abi_argument_checks():
    """The launchers refuse bad geometry before any launch (name: message through eunet_last_error); the
    pointers are never dereferenced on the host, so this runs without a GPU."""
    import ctypes
    from eunet import _lib
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.c_void_p(ctypes.addressof(buf) // 16 * 16 + 16)

    def gather(c=3, h=70, w=101, hp=96, wp=128, th=64, tw=64, sy=32, sx=32, first=0, count=1):
        _lib.call("eunet_tile_gather", ptr, c, h, w, hp, wp, th, tw, sy, sx, first, count, ptr, None)

    def blend(k=3, h=70, w=101, hp=96, wp=128, th=64, tw=64, sy=32, sx=32, mode=0, margin=16, wy=None, wx=None,
              act=1):
        _lib.call("eunet_tile_blend", ptr, k, h, w, hp, wp, th, tw, sy, sx, mode, margin, wy, wx, act, 0, 0, ptr, None)

    for fn, kw, match in (
            (gather, dict(c=5), "tile_gather: C must be 1..4"),
            (gather, dict(hp=128), "tile_gather: hp x wp must be"),
            (gather, dict(th=48), "tile_gather: tile extents"),
            (gather, dict(th=128), "tile_gather: tile extents"),
            (gather, dict(sx=16), "tile_gather: strides"),
            (gather, dict(first=5, count=2), "tile_gather: tiles 5 .. 6 are not inside"),
            (gather, dict(h=16, hp=32), "tile_gather: the reflect padding"),
            (blend, dict(k=4), "tile_blend: K must be 1..3"),
            (blend, dict(mode=3), "tile_blend: unknown blend mode"),
            (blend, dict(act=3), "tile_blend: unknown activation"),
            (blend, dict(margin=8), "tile_blend: margin"),
            (blend, dict(margin=32), "tile_blend: stride \\+ 2 margin exceeds"),
            (blend, dict(mode=1, sy=96, sx=96), "tile_blend: a stride exceeds"),
            (blend, dict(mode=2), "tile_blend: the gaussian mode needs"),
            (blend, dict(wp=96), "tile_blend: hp x wp must be")):
        with pytest.raises(_lib.EunetError, match=match):
            fn(**kw)


def _perturbed_weights():
    """Formula weights with the BatchNorm running statistics moved off (0, 1), so eval mode is a real affine."""
    from oracle import eunet_ref as R
    g = torch.Generator().manual_seed(11)
    S = R.formula_weights(16, 3, 3, dtype=torch.float64)
    for k in S:
        if k.endswith("running_mean"):
            S[k] = 0.1 * torch.randn(S[k].shape, generator=g, dtype=torch.float64)
        elif k.endswith("running_var"):
            S[k] = 0.5 + torch.rand(S[k].shape, generator=g, dtype=torch.float64)
    return S, g


def test_receptive_margin_on_the_oracle():
    """oracle.eunet_ref.forward, fp64, eval mode, base 16: the logits at H of a 256 x 256 tile at origin
    (64, 64) of a 384 x 384 image against the whole-image logits.  They agree to 1e-10 max|ref| everywhere at
    depth >= RECEPTIVE_MARGIN from the tile edge, and do not agree somewhere at depth >= RECEPTIVE_MARGIN - 16.
    Measured: the largest difference over max|ref| is 2.0e-8 at depth 48, 6.9e-11 at depth 53 and 5e-16 from
    depth 54 inwards (max|ref| = 0.169)."""
    from eunet import tiling
    from oracle import eunet_ref as R
    S, g = _perturbed_weights()
    x = torch.rand(1, 3, 384, 384, generator=g, dtype=torch.float64)
    with torch.no_grad():
        full = F.avg_pool2d(R.forward(S, x, training=False), 2)[0]
        tile = F.avg_pool2d(R.forward(S, x[:, :, 64:320, 64:320], training=False), 2)[0]
    scale = float(full.abs().max())
    diff = (tile - full[:, 64:320, 64:320]).abs().amax(0)
    i = torch.arange(256)
    d1 = torch.minimum(i, 255 - i)
    depth = torch.minimum(d1[:, None], d1[None, :])
    m = tiling.RECEPTIVE_MARGIN
    inner = float(diff[depth >= m].max()) / scale
    outer = float(diff[depth >= m - 16].max()) / scale
    print(f"max|ref| {scale:.3e}; depth >= {m}: {inner:.3e}; depth >= {m - 16}: {outer:.3e}")
    assert inner <= 1e-10
    assert outer > 1e-10
