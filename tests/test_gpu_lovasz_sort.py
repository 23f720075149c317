"""lovasz.hip, the sort and the Lovasz gradient: ops.lovasz_sort against tests/_lovasz_ref.py.

order and counts must be equal exactly.  grad is a closed form of integers evaluated in correctly rounded fp64
operations and rounded once, so equality is expected too; 1 fp32 ulp is allowed (as tests/test_gpu_sdf.py allows for
its correctly rounded square root) and the worst deviation is printed.

T is the sort's (and the scan's) pairs per block, B the block size of the scan of the block totals; both are read
from the code.  Lengths sit on either side of a wave round (64), of a block (T) and of the second level of the
block-total scan (B T); the key patterns make each of the four 8-bit passes the one that decides."""
import os
import re

import numpy as np
import pytest
import torch

import _lovasz_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _const(path, name):
    src = open(os.path.join(ROOT, "enhanced-unet_amd", "csrc", path)).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))


B = _const("labelmap.h", "LM_NT")
T = B * _const("lovasz.hip", "LZ_ITEMS")


def _run(errors, flags):
    from eunet import ops
    order, grad, counts = ops.lovasz_sort(torch.from_numpy(errors).to(DEV), torch.from_numpy(flags).to(DEV))
    torch.cuda.synchronize()
    return order.cpu().numpy(), grad.cpu().numpy(), counts.cpu().numpy()


def _ulps(a, b):
    """The distance of two float32 arrays in units of the last place (both finite and of one sign, or equal)."""
    ai, bi = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return int(np.abs(ai - bi).max()) if a.size else 0


def _check(name, errors, flags):
    errors = np.ascontiguousarray(errors, dtype=np.float32)
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    order, grad, counts = _run(errors, flags)
    o_ref, g_ref, c_ref = R.sort_ref(errors, flags)
    worst = _ulps(grad, g_ref)
    print(f"{name}: S {errors.shape[0]} L {errors.shape[1]}, grad worst deviation {worst} ulp")
    assert np.array_equal(counts, c_ref), (name, counts, c_ref)
    assert np.array_equal(order, o_ref), (name, np.argwhere(order != o_ref)[:5])
    assert (grad >= 0).all() and worst <= 1, (name, worst)
    return order, grad, counts


def _flags(rng, shape):
    return rng.choice(np.array([0, 1, 2], dtype=np.uint8), size=shape, p=[0.5, 0.4, 0.1])


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3])
def test_lengths_around_a_round_and_a_block(L):
    rng = np.random.default_rng(L)
    for kind in ("random", "coarse"):
        e = rng.random((2, L), dtype=np.float32)
        if kind == "coarse":
            e = np.round(e * 8) / 8  # many equal keys: stability across rounds, waves and blocks
        _check(f"L{L} {kind}", e, _flags(rng, (2, L)))


def test_second_level_of_the_block_total_scan_and_bit_identical_runs():
    """L just above B T: more than B blocks per segment, so scan_block_counts_kernel takes a second chunk, in the
    sort's digit rows and in the foreground scan.  The largest case: two runs give identical bits."""
    L = B * T + 5
    rng = np.random.default_rng(7)
    e = (np.round(rng.random((1, L), dtype=np.float32) * 4096) / 4096).astype(np.float32)
    e[0, rng.random(L) < 0.5] = 0.0
    f = _flags(rng, (1, L))
    a = _check(f"L{L}", e, f)
    b = _run(e, f)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


@pytest.mark.parametrize("S", [1, 3, 6])
def test_segment_counts(S):
    rng = np.random.default_rng(S)
    e = rng.standard_normal((S, 35)).astype(np.float32)
    _check(f"S{S}", e, _flags(rng, (S, 35)))


def _bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def _patterns(L, rng):
    r = rng.random(L, dtype=np.float32)
    sat = r.copy()
    sat[: L // 2] = 0.0
    sat[L // 2: L // 2 + L // 4] = 1.0
    special = r.copy()
    special[::7] = 0.0
    special[1::7] = -0.0
    special[2::7] = _bits(rng.integers(1, 100, size=special[2::7].shape))  # denormals
    special[3::11] = np.inf
    special[L // 3] = np.nan
    return {
        "all equal": np.full(L, 0.25, dtype=np.float32),
        "two values": np.where(rng.random(L) < 0.5, 0.75, 0.125).astype(np.float32),
        "descending": np.linspace(1.0, 0.0, L, dtype=np.float32),
        "ascending": np.linspace(0.0, 1.0, L, dtype=np.float32),
        # bit 22 set and bit 23 clear: no exponent of all ones, so neither inf nor NaN; both signs
        "top byte only": _bits((rng.integers(0, 256, size=L).astype(np.uint32) << 24) | 0x00400000),
        "bottom byte only": _bits(0x3F000000 | rng.integers(0, 256, size=L).astype(np.uint32)),
        "second byte only": _bits(0x3F000000 | (rng.integers(0, 256, size=L).astype(np.uint32) << 8)),
        "third byte only": _bits(0x3F000000 | (rng.integers(0, 128, size=L).astype(np.uint32) << 16)),
        "saturated": rng.permutation(sat),
        "zeros denormals inf nan": special,
        "negative (hinge)": (rng.standard_normal(L) * 3).astype(np.float32),
    }


@pytest.mark.parametrize("name", list(_patterns(8, np.random.default_rng(0))))
def test_key_patterns(name):
    for L in (300, T + 77):
        rng = np.random.default_rng(L)
        e = np.stack([_patterns(L, rng)[name], _patterns(L, rng)[name]])
        f = _flags(rng, (2, L))
        f[1] = rng.integers(0, 2, size=L)  # the second segment has no ignored element
        order, grad, counts = _check(f"{name} L{L}", e, f)
        if name == "all equal":
            assert np.array_equal(order[1], np.arange(L))


def test_flag_patterns():
    L = T + 77
    rng = np.random.default_rng(3)
    e = rng.random((4, L), dtype=np.float32)
    f = np.zeros((4, L), dtype=np.uint8)
    f[0] = 2  # all ignored
    f[1] = 1  # all foreground
    f[2] = 0  # no foreground
    f[3] = rng.integers(0, 2, size=L)
    order, grad, counts = _check("flags", e, f)
    assert np.array_equal(order[0], np.arange(L)) and not grad[0].any() and counts[0].tolist() == [0, 0]
    assert (grad[1] == np.float32(1.0 / L)).all()
    assert grad[2].sum() == 1.0 and grad[2, np.argmax(e[2])] == 1.0


def test_ignored_elements_between_valid_zero_errors():
    """Ignored elements interleaved with valid elements of error 0 land last, and no valid g changes when they are
    taken away."""
    L = T + 77
    rng = np.random.default_rng(4)
    e = rng.random((1, L), dtype=np.float32)
    e[0, ::2] = 0.0
    f = rng.integers(0, 2, size=(1, L)).astype(np.uint8)
    ign = np.zeros(L, dtype=bool)
    ign[1::4] = True
    ign[0::6] = True  # some of the zero-error elements too
    f[0, ign] = 2
    order, grad, counts = _check("interleaved", e, f)
    v = int(counts[0, 1])
    assert v == int((~ign).sum()) and np.array_equal(np.sort(order[0, v:]), np.flatnonzero(ign))
    assert np.array_equal(order[0, v:], np.flatnonzero(ign))
    order2, grad2, counts2 = _check("compacted", e[:, ~ign], f[:, ~ign])
    assert np.array_equal(grad[0, ~ign].view(np.uint32), grad2[0].view(np.uint32))
