"""fusion.hip kernel by kernel against fp64 references, at the edges of its tiles (GPU only).

The forward and backward glue of the dual-branch fusion works on tiles of TP = 2048 flattened pixels
(gate_bwd3: 16x32 spatial tiles).  tests/test_gpu_dual.py sees these kernels only through whole-model
parameter gradients at /32 image sizes, where every tile but the last is full and the spatial tiles
divide the image.  Here each kernel gets inputs of its own (seeded Gaussians; branch outputs with a mean
of 0.5; BN mean / invstd / gamma / beta away from their defaults), is compared element by element and
partial by partial with the contract of its header comment written in fp64, and runs at

    (1,1,1)              a single pixel: every tap is padding, a tile count of 1
    (2,1,40), (2,40,1)   one row / one column; W = 40 crosses the 32-wide gate tile
    (1,32,64)            P = 2048: exactly one full tile and an exact 2x2 set of gate tiles
    (3,19,37)            P = 2109: one full tile + 61 pixels, samples straddling the tile boundary,
                         19 > 16 and 37 > 32 ragged in both directions
    (2,33,65)            P = 4290: three tiles; 3x3 gate tiles whose last row / column is one pixel wide

for K = 1, 2 and 3.  One composed test then runs the whole gate forward and backward as
DualEngine chains it against fp64 autograd of the reference module's expression, so that a per-kernel
reference restating a wrong formula cannot pass unnoticed.

Gates
  element-wise fp32 outputs   max|got - ref| <= 1e-4 max|ref|           (tests/test_gpu_ops.py, fp32)
  bf16 output (gate_out_fwd)  |got - ref| <= 2^-8 |ref| + 1e-5 max|ref|  per element (one rounding)
  per-tile sums               |got - ref| <= 1e-5 sum|terms| over that tile, sum|terms| from the fp64
                              reference.  The TP-tile kernels add 8 values per thread and then 8
                              butterfly / tree levels: at most 16 roundings of 2^-24, about 1e-6 of
                              sum|terms|; 1e-5 leaves a tenfold margin for the few-ulp erff / expf in the
                              terms.  (gate_bwd3 adds its 512 pixels serially, 512 * 2^-24 = 3e-5 in the
                              worst case and about sqrt(512) * 2^-24 = 1.4e-6 for rounding errors of
                              random sign; it is held to the same 1e-5.)
  composed test               per tensor max(1e-4, 3 x the error of the same autograd chain in fp32 on
                              the CPU), both relative to the largest fp64 value
Every output, partial and statistics buffer carries a 64-element tail of a sentinel that must survive,
and every kernel runs twice with bit-equal results (fixed-order reductions).
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
TP = 2048             # flattened pixels per tile (fusion.hip NT * PPT)
GTH, GTW = 16, 32     # gate_bwd3's spatial tile
TAIL, SENT = 64, -12345.5
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
SHAPES = [(1, 1, 1), (2, 1, 40), (2, 40, 1), (1, 32, 64), (3, 19, 37), (2, 33, 65)]
KS = [1, 2, 3]
DTYPES = [torch.float32, torch.bfloat16]
shapes_and_k = pytest.mark.parametrize("shape,K", [(s, k) for s in SHAPES for k in KS],
                                       ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"K{v}")


def _ops():
    from eunet import ops
    return ops


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


# ---- inputs ---------------------------------------------------------------------------------------------
class Case:
    """Seeded inputs of one (shape, K): c.<name> fp32 on the host, c.d.<name> on the device, c.r.<name> fp64."""

    def __init__(self, host):
        self.__dict__.update(host)
        self.d = type("Dev", (), {k: v.to(DEV) for k, v in host.items()})
        self.r = type("Ref", (), {k: v.double() for k, v in host.items()})


@functools.lru_cache(maxsize=None)
def _case(shape, K):
    N, H, W = shape
    P, C2 = N * H * W, 2 * K
    g = torch.Generator().manual_seed(7919 * K + 31 * P + H)

    def rn(*s):
        return torch.randn(*s, generator=g)

    def ru(*s):
        return torch.rand(*s, generator=g)

    def sign(*s):
        return torch.where(ru(*s) < 0.5, -1.0, 1.0)

    h = {}

    def bn(tag, C):
        mean, istd = sign(C) * (0.2 + 0.6 * ru(C)), 0.5 + 1.5 * ru(C)
        gam, bet = sign(C) * (0.5 + ru(C)), 0.3 * rn(C)
        sc = (gam.double() * istd.double()).float()
        h.update({f"mean{tag}": mean, f"istd{tag}": istd, f"gam{tag}": gam, f"bet{tag}": bet, f"sc{tag}": sc,
                  f"sh{tag}": (bet.double() - mean.double() * sc.double()).float()})

    h.update(za=0.5 + rn(N, H, W, K), zb=0.5 + rn(N, H, W, K), w1=0.3 * rn(K, C2, 3, 3), w2=0.5 * rn(C2, K),
             wr=0.5 * rn(K, C2), br=rn(K), w11=0.2 * rn(K, 64), b11=rn(K),
             a=0.3 + rn(N, H, W, K), b=0.2 + rn(N, H, W, C2), y3=rn(N, H, W, 64),
             gout=rn(N, K, H, W), gf2c=rn(N, H, W, 8), gf2res=rn(N, H, W, C2), gbhat=0.1 + rn(N, H, W, C2),
             gabn=0.1 + rn(N, H, W, K), gffd=rn(N, H, W, C2), gaux_a=rn(N, K, H, W), gaux_b=rn(N, K, H, W),
             # BN-backward reductions as the real chain produces them: sums over P pixels
             dbet2=P * (0.3 + 0.2 * rn(C2)), dgam2=P * (0.3 + 0.2 * rn(C2)),
             dbet1=P * (0.3 + 0.2 * rn(K)), dgam1=P * (0.3 + 0.2 * rn(K)))
    bn("1", K)
    bn("2", C2)
    bn("3", 64)
    return Case(h)


class Outs:
    """Output buffers with a sentinel tail; check() synchronises and asserts that every tail survived."""

    def __init__(self):
        self.items = []

    def new(self, shape, dtype=torch.float32, fill=None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = math.prod(shape)
        flat = torch.full((n + TAIL,), SENT, dtype=dtype, device=DEV)
        v = flat[:n].view(shape)
        if fill is not None:
            v.fill_(fill)
        self.items.append((flat, n))
        return v

    def check(self):
        torch.cuda.synchronize()
        for flat, n in self.items:
            assert torch.equal(flat[n:], torch.full((TAIL,), SENT, dtype=flat.dtype, device=DEV)), "tail overwritten"


def _twice(run):
    """run() launches into fresh buffers and returns its outputs; both runs must agree bit for bit."""
    first, second = run(), run()
    for i, (x, y) in enumerate(zip(first, second)):
        assert torch.equal(x, y), f"output {i} differs between two runs"
    return [t.detach().cpu() for t in first]


# ---- gates ----------------------------------------------------------------------------------------------
def _gate(name, got, ref, dt=torch.float32):
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), name
    mx = float(ref.abs().max())
    err = (got - ref).abs()
    if dt == torch.float32:
        assert float(err.max()) <= 1e-4 * mx, (name, float(err.max()), mx)
    else:
        worst = float((err / (2.0 ** -8 * ref.abs() + 1e-5 * mx).clamp_min(1e-300)).max())
        assert worst <= 1.0, (name, worst)


def _sum_gate(name, got, ref, mag):
    got = got.detach().double().cpu().reshape(ref.shape)
    bad = (got - ref).abs() > 1e-5 * mag
    assert not bool(bad.any()), (name, int(bad.sum()), float(((got - ref).abs() / mag.clamp_min(1e-300)).max()))


def _tile_sums(terms):
    """terms [P, C] fp64 -> per-TP-chunk (sums [tiles, C], sums of |terms| [tiles, C])."""
    P, C = terms.shape
    tiles = (P + TP - 1) // TP
    pad = torch.zeros(tiles * TP, C, dtype=torch.float64)
    pad[:P] = terms
    v = pad.view(tiles, TP, C)
    return v.sum(1), v.abs().sum(1)


def _check_partials(name, part, terms):
    """part [tiles][C] against the chunk sums of terms [P, C], and its colsum against the full sums."""
    ops = _ops()
    ref, mag = _tile_sums(terms)
    tiles, C = ref.shape
    _sum_gate(name, part, ref, mag)
    o = Outs()
    red = o.new(C)
    ops.colsum(part.to(DEV), tiles, C, red)
    o.check()
    _sum_gate(name + " colsum", red, terms.sum(0), terms.abs().sum(0))


def _check_stats(name, st, vals, C):
    """st decoded directly: st[tile][0][c] = sum, st[tile][1][c] = M2 about the tile mean, counts at
    st[2*C*tiles + tile]; vals [P, C] is the fp64 reference of the tensor the statistics are of."""
    P = vals.shape[0]
    tiles = (P + TP - 1) // TP
    st = st.double().cpu()
    assert st.numel() == tiles * (2 * C + 1)
    body, cnt = st[:2 * C * tiles].view(tiles, 2, C), st[2 * C * tiles:]
    for t in range(tiles):
        n = min(TP, P - TP * t)
        assert cnt[t].item() == n, (name, t, cnt[t].item(), n)
        chunk = vals[t * TP:t * TP + n]
        m2 = ((chunk - chunk.mean(0)) ** 2).sum(0)
        _sum_gate(f"{name} sum tile {t}", body[t, 0], chunk.sum(0), chunk.abs().sum(0))
        _sum_gate(f"{name} M2 tile {t}", body[t, 1], m2, m2)


# ---- fp64 pieces of the contract --------------------------------------------------------------------------
SQRT1_2, INV_SQRT_2PI = 0.70710678118654752, 0.39894228040143268


def _gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x * SQRT1_2)) + x * INV_SQRT_2PI * torch.exp(-0.5 * x * x)


def _ff(r):
    return torch.cat([r.za, r.zb], -1)


def _f2(r):
    return _ff(r) * torch.sigmoid(r.b * r.sc2 + r.sh2)


def _bn_bwd(g, x, mean, istd, gam, dbet, dgam, P):
    xh = (x - mean) * istd
    return gam * istd * (g - dbet / P - xh * dgam / P)


# ---- forward kernels --------------------------------------------------------------------------------------
@shapes_and_k
def test_gate_fwd(shape, K):
    ops, c = _ops(), _case(shape, K)
    N, H, W = shape
    P = N * H * W
    tiles, gtiles = ops.fusion_tiles(N, H, W)
    assert tiles == (P + TP - 1) // TP and gtiles == N * ((H + GTH - 1) // GTH) * ((W + GTW - 1) // GTW)

    def run():
        o = Outs()
        a, st = o.new((N, H, W, K)), o.new(tiles * (2 * K + 1))
        aux_a, aux_b = o.new((N, K, H, W)), o.new((N, K, H, W))
        ops.gate_fwd(c.d.za, c.d.zb, K, c.d.w1, a, st, aux_a, aux_b)
        o.check()
        return a, st, aux_a, aux_b

    a, st, aux_a, aux_b = _twice(run)
    ref = nhwc(F.conv2d(nchw(_ff(c.r)), c.r.w1, padding=1))
    _gate("a", a, ref)
    assert torch.equal(aux_a, nchw(c.za)) and torch.equal(aux_b, nchw(c.zb))
    _check_stats("st1", st, ref.view(P, K), K)


@shapes_and_k
def test_gate_mid_fwd(shape, K):
    ops, c = _ops(), _case(shape, K)
    N, H, W = shape
    P, C2 = N * H * W, 2 * K
    tiles, _ = ops.fusion_tiles(N, H, W)

    def run():
        o = Outs()
        b, st = o.new((N, H, W, C2)), o.new(tiles * (2 * C2 + 1))
        ops.gate_mid_fwd(c.d.za, c.d.zb, K, c.d.a, c.d.sc1, c.d.sh1, c.d.w2, b, st)
        o.check()
        return b, st

    b, st = _twice(run)
    ref = F.gelu(c.r.a * c.r.sc1 + c.r.sh1) @ c.r.w2.t()
    _gate("b", b, ref)
    _check_stats("st2", st, ref.view(P, C2), C2)


@shapes_and_k
def test_gate_out_fwd(shape, K):
    """Channels [0, 2K) hold ff * sigmoid(bn2(b)); the kernel also owns the pad [2K, 8): exactly 0 over NaN."""
    ops, c = _ops(), _case(shape, K)
    N, H, W = shape
    C2 = 2 * K
    ref = _f2(c.r)
    for dt in DTYPES:
        def run():
            o = Outs()
            f2 = o.new((N, H, W, 8), dt, fill=float("nan"))
            ops.gate_out_fwd(c.d.za, c.d.zb, K, c.d.b, c.d.sc2, c.d.sh2, ops.act(f2, 0, C2))
            o.check()
            assert not bool(torch.isnan(f2).any())
            return (f2,)

        (f2,) = _twice(run)
        _gate(f"f2 {dt}", f2[..., :C2], ref, dt)
        assert float(f2[..., C2:].abs().max()) == 0.0, f"pad channels {dt}"


def test_gate_out_fwd_rejects_a_larger_f2():
    """f2 must have the branch outputs' n, h and w: one more sample (the larger allocation: the kernel takes its
    pixel count from za) is EUNET_ERR_INVALID, for both dtypes."""
    from eunet._lib import EunetError
    ops, K = _ops(), 1
    za = torch.zeros(1, 2, 2, K, device=DEV)
    b, v = torch.zeros(1, 2, 2, 2 * K, device=DEV), torch.zeros(2 * K, device=DEV)
    for dt in DTYPES:
        f2 = torch.zeros(2, 2, 2, 8, dtype=dt, device=DEV)
        with pytest.raises(EunetError):
            ops.gate_out_fwd(za, za, K, b, v, v, ops.act(f2, 0, 2 * K))
    torch.cuda.synchronize()


@shapes_and_k
def test_fusion_out_fwd(shape, K):
    ops, c = _ops(), _case(shape, K)
    N, H, W = shape
    for dt in DTYPES:
        y3 = c.y3.to(dt)
        y3d = y3.to(DEV)

        def run():
            o = Outs()
            out = o.new((N, K, H, W))
            ops.fusion_out_fwd(c.d.za, c.d.zb, K, ops.act(y3d), c.d.sc3, c.d.sh3, c.d.w11, c.d.b11, c.d.b, c.d.sc2,
                               c.d.sh2, c.d.wr, c.d.br, out)
            o.check()
            return (out,)

        (out,) = _twice(run)
        h = (y3.double() * c.r.sc3 + c.r.sh3).clamp_min(0.0)  # the reference on y3 as stored
        ref = h @ c.r.w11.t() + c.r.b11 + _f2(c.r) @ c.r.wr.t() + c.r.br
        _gate(f"out {dt}", out, nchw(ref))


# ---- backward kernels -------------------------------------------------------------------------------------
@shapes_and_k
def test_fusion_out_bwd(shape, K):
    ops, c = _ops(), _case(shape, K)
    N, H, W = shape
    P, C2 = N * H * W, 2 * K
    nv = K * C2 + K
    tiles, _ = ops.fusion_tiles(N, H, W)

    def run():
        o = Outs()
        gz, gf2res, part = o.new((N, H, W, K)), o.new((N, H, W, C2)), o.new(tiles * nv)
        ops.fusion_out_bwd(c.d.za, c.d.zb, K, c.d.gout, c.d.b, c.d.sc2, c.d.sh2, c.d.wr, gz, gf2res, part)
        o.check()
        return gz, gf2res, part

    gz, gf2res, part = _twice(run)
    go = nhwc(c.r.gout)
    _gate("gz", gz, go)
    _gate("gf2res", gf2res, go @ c.r.wr)
    go, f2 = go.view(P, K), _f2(c.r).view(P, C2)
    terms = torch.cat([(go[:, :, None] * f2[:, None, :]).reshape(P, K * C2), go], 1)  # dWr k-major, then dbr
    _check_partials("dWr / dbr", part.view(tiles, nv), terms)


@shapes_and_k
def test_gate_bwd1(shape, K):
    ops, c = _ops(), _case(shape, K)
    N, H, W = shape
    P, C2 = N * H * W, 2 * K
    tiles, _ = ops.fusion_tiles(N, H, W)
    for dt in DTYPES:
        gc = c.gf2c.to(dt)  # all 8 channels random: the pad must be ignored
        gcd = gc.to(DEV)

        def run():
            o = Outs()
            gffd, gbhat, part = o.new((N, H, W, C2)), o.new((N, H, W, C2)), o.new(tiles * 2 * C2)
            ops.gate_bwd1(c.d.za, c.d.zb, K, ops.act(gcd), c.d.gf2res, c.d.b, c.d.mean2, c.d.istd2, c.d.gam2,
                          c.d.bet2, gffd, gbhat, part)
            o.check()
            return gffd, gbhat, part

        gffd, gbhat, part = _twice(run)
        r = c.r
        gf = gc.double()[..., :C2] + r.gf2res  # the reference on g_f2conv as stored
        xh = (r.b - r.mean2) * r.istd2
        at = torch.sigmoid(r.gam2 * xh + r.bet2)
        gb = gf * _ff(r) * at * (1.0 - at)
        _gate(f"gffd {dt}", gffd, gf * at)
        _gate(f"gbhat {dt}", gbhat, gb)
        terms = torch.cat([gb.view(P, C2), (gb * xh).view(P, C2)], 1)  # [tile][2][2K]
        _check_partials(f"BN2 reductions {dt}", part.view(tiles, 2 * C2), terms)


@shapes_and_k
def test_gate_bwd2(shape, K):
    ops, c = _ops(), _case(shape, K)
    N, H, W = shape
    P, C2 = N * H * W, 2 * K
    nv = C2 * K + 2 * K
    tiles, _ = ops.fusion_tiles(N, H, W)

    def run():
        o = Outs()
        gabn, part = o.new((N, H, W, K)), o.new(tiles * nv)
        ops.gate_bwd2(N, H, W, K, c.d.gbhat, c.d.b, c.d.mean2, c.d.istd2, c.d.gam2, c.d.dbet2, c.d.dgam2, c.d.a,
                      c.d.mean1, c.d.istd1, c.d.gam1, c.d.bet1, c.d.w2, gabn, part)
        o.check()
        return gabn, part

    gabn, part = _twice(run)
    r = c.r
    gb = _bn_bwd(r.gbhat, r.b, r.mean2, r.istd2, r.gam2, r.dbet2, r.dgam2, P)
    xh1 = (r.a - r.mean1) * r.istd1
    abn = r.gam1 * xh1 + r.bet1
    v = F.gelu(abn)
    ga = (gb @ r.w2) * _gelu_grad(abn)  # g_v[k] = sum_j Wg2[j][k] g_b[j]
    _gate("gabn", gabn, ga)
    gb, v, ga, xh1 = gb.view(P, C2), v.view(P, K), ga.view(P, K), xh1.view(P, K)
    terms = torch.cat([(gb[:, :, None] * v[:, None, :]).reshape(P, C2 * K), ga, ga * xh1], 1)  # dWg2 j-major
    _check_partials("dWg2 / BN1 reductions", part.view(tiles, nv), terms)


def _gate_tile_sums(terms, H, W):
    """terms [N, C, H, W] -> sums over gate_bwd3's 16x32 tiles, [N * ty * tx, C] in the kernel's tile order."""
    N, C = terms.shape[:2]
    ty, tx = (H + GTH - 1) // GTH, (W + GTW - 1) // GTW
    pad = torch.zeros(N, C, ty * GTH, tx * GTW, dtype=torch.float64)
    pad[:, :, :H, :W] = terms
    s = pad.view(N, C, ty, GTH, tx, GTW).sum((3, 5))  # [N, C, ty, tx]
    return s.permute(0, 2, 3, 1).reshape(N * ty * tx, C)


@pytest.mark.parametrize("aux", [True, False], ids=["aux", "noaux"])
@shapes_and_k
def test_gate_bwd3(shape, K, aux):
    ops, c = _ops(), _case(shape, K)
    N, H, W = shape
    P, C2 = N * H * W, 2 * K
    nw = K * C2 * 9
    _, gtiles = ops.fusion_tiles(N, H, W)

    def run():
        o = Outs()
        gz_a, gz_b, part = o.new((N, H, W, K)), o.new((N, H, W, K)), o.new(gtiles * nw)
        ops.gate_bwd3(c.d.za, c.d.zb, K, c.d.gabn, c.d.a, c.d.mean1, c.d.istd1, c.d.gam1, c.d.dbet1, c.d.dgam1,
                      c.d.w1, c.d.gffd, c.d.gaux_a if aux else None, c.d.gaux_b if aux else None, gz_a, gz_b, part)
        o.check()
        return gz_a, gz_b, part

    gz_a, gz_b, part = _twice(run)
    r = c.r
    ga = nchw(_bn_bwd(r.gabn, r.a, r.mean1, r.istd1, r.gam1, r.dbet1, r.dgam1, P))  # [N, K, H, W]
    # g_ff[p][j] = g_ffd[p][j] + sum_{t,k} Wg1[k][j][t] g_a[p - d_t][k]: the adjoint of the 3x3 conv
    gff = r.gffd + nhwc(F.conv_transpose2d(ga, r.w1, padding=1))
    ref_a, ref_b = gff[..., :K], gff[..., K:]
    if aux:
        ref_a, ref_b = ref_a + nhwc(r.gaux_a), ref_b + nhwc(r.gaux_b)
    _gate("gz_a", gz_a, ref_a)
    _gate("gz_b", gz_b, ref_b)
    # dWg1[k][j][t] = sum_q g_a[q][k] ff[q + d_t][j] over each 16x32 tile, g_a and ff of the whole image
    ffp = F.pad(nchw(_ff(r)), (1, 1, 1, 1))
    shifted = torch.stack([ffp[:, :, t // 3:t // 3 + H, t % 3:t % 3 + W] for t in range(9)], 2)  # [N, 2K, 9, H, W]
    terms = (ga[:, :, None, None] * shifted[:, None]).reshape(N, nw, H, W)  # (k, j, t) major to minor
    ref, mag = _gate_tile_sums(terms, H, W), _gate_tile_sums(terms.abs(), H, W)
    assert ref.shape == (gtiles, nw)
    _sum_gate("dWg1 partials", part, ref, mag)
    o = Outs()
    red = o.new(nw)
    ops.colsum(part.to(DEV), gtiles, nw, red)
    o.check()
    _sum_gate("dWg1 colsum", red, terms.sum((0, 2, 3)), terms.abs().sum((0, 2, 3)))


@pytest.mark.parametrize("with_g", [True, False], ids=["gscale", "nogscale"])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_dropout_affine(p, with_g):
    """n*c = 3*100 (one ragged block).  Exact in fp32: the same fp32 expression on the CPU, bit for bit."""
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    n, C = 3, 100
    sc, sh = torch.randn(C, generator=g), torch.randn(C, generator=g)
    keep = (torch.rand(n, C, generator=g) >= 0.3).float()
    assert 0 < int(keep.sum()) < n * C

    def run():
        o = Outs()
        osc, osh, og = o.new((n, C)), o.new((n, C)), o.new((n, C))
        ops.dropout_affine(sc.to(DEV), sh.to(DEV), keep.to(DEV), p, osc, osh, og if with_g else None)
        o.check()
        return osc, osh, og

    osc, osh, og = _twice(run)
    one = torch.tensor(1.0, dtype=torch.float32)
    m = keep * (one / (one - torch.tensor(p, dtype=torch.float32)))
    assert torch.equal(osc, sc[None, :] * m) and torch.equal(osh, sh[None, :] * m)
    assert torch.equal(og, m if with_g else torch.full((n, C), SENT))


# ---- the composed gate: forward and backward as DualEngine chains them, against fp64 autograd -------------
def _gate_autograd(c, K, dtype, G):
    """The reference module's own expression and its gradients in `dtype` on the CPU."""
    t = {k: getattr(c, k).to(dtype).clone().requires_grad_(True)
         for k in ("za", "zb", "w1", "gam1", "bet1", "w2", "gam2", "bet2", "wr", "br")}
    C2 = 2 * K
    run = {k: G[k].to(dtype).clone() for k in ("rm1", "rv1", "rm2", "rv2")}
    ff = torch.cat([nchw(t["za"]), nchw(t["zb"])], 1)
    h = F.conv2d(ff, t["w1"], padding=1)
    h = F.batch_norm(h, run["rm1"], run["rv1"], t["gam1"], t["bet1"], True, BN_MOMENTUM, BN_EPS)
    h = F.conv2d(F.gelu(h), t["w2"].view(C2, K, 1, 1))
    att = torch.sigmoid(F.batch_norm(h, run["rm2"], run["rv2"], t["gam2"], t["bet2"], True, BN_MOMENTUM, BN_EPS))
    f2 = ff * att
    res = F.conv2d(f2, t["wr"].view(K, C2, 1, 1), t["br"])
    s = (res * G["gout"].to(dtype)).sum() + (f2 * nchw(G["gc"]).to(dtype)).sum() \
        + (nchw(t["za"]) * G["gaux_a"].to(dtype)).sum() + (nchw(t["zb"]) * G["gaux_b"].to(dtype)).sum()
    s.backward()
    out = {"d " + k: v.grad for k, v in t.items()}
    out.update(run)
    out["f2"] = nhwc(f2.detach())
    return out


@pytest.mark.parametrize("K", KS)
def test_gate_composed_matches_autograd(K):
    """(3,19,37): gate_fwd, bn_finalize, gate_mid_fwd, bn_finalize, gate_out_fwd, then fusion_out_bwd,
    gate_bwd1, colsum, gate_bwd2, colsum, gate_bwd3, colsum with the calls of DualEngine.forward / backward;
    fixed random tensors stand in for the head (Gout = d out, Gc = the head's g_f2, Gaux_a / Gaux_b)."""
    ops = _ops()
    shape = (3, 19, 37)
    N, H, W = shape
    c = _case(shape, K)
    C2 = 2 * K
    gen = torch.Generator().manual_seed(77 + K)
    G = dict(gout=c.gout, gc=c.gf2c[..., :C2].contiguous(), gaux_a=c.gaux_a, gaux_b=c.gaux_b,
             rm1=torch.randn(K, generator=gen), rv1=0.5 + torch.rand(K, generator=gen),
             rm2=torch.randn(C2, generator=gen), rv2=0.5 + torch.rand(C2, generator=gen))
    ref = _gate_autograd(c, K, torch.float64, G)
    ref32 = _gate_autograd(c, K, torch.float32, G)

    d = c.d
    tiles, gtiles = ops.fusion_tiles(N, H, W)
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=DEV)  # noqa: E731

    def bn(st, C, gam, bet, rm, rv):
        mean, invstd, scale, shift = e(C), e(C), e(C), e(C)
        nbt = torch.zeros((), dtype=torch.int64, device=DEV)
        ops.bn_finalize(st, tiles, C, gam, bet, BN_EPS, BN_MOMENTUM, rm, rv, mean, invstd, scale, shift, nbt)
        return dict(mean=mean, invstd=invstd, scale=scale, shift=shift)

    # ---- forward (DualEngine.forward)
    run = {k: G[k].to(DEV) for k in ("rm1", "rv1", "rm2", "rv2")}
    a, st1 = e(N, H, W, K), e(tiles * (2 * K + 1))
    aux_a, aux_b = e(N, K, H, W), e(N, K, H, W)
    ops.gate_fwd(d.za, d.zb, K, d.w1, a, st1, aux_a, aux_b)
    g1 = bn(st1, K, d.gam1, d.bet1, run["rm1"], run["rv1"])
    b, st2 = e(N, H, W, C2), e(tiles * (4 * K + 1))
    ops.gate_mid_fwd(d.za, d.zb, K, a, g1["scale"], g1["shift"], d.w2, b, st2)
    g2 = bn(st2, C2, d.gam2, d.bet2, run["rm2"], run["rv2"])
    f2 = torch.zeros((N, H, W, 8), dtype=torch.float32, device=DEV)
    ops.gate_out_fwd(d.za, d.zb, K, b, g2["scale"], g2["shift"], ops.act(f2, 0, C2))
    # ---- backward (DualEngine.backward: output 1x1 + residual, then the attention gate)
    gz, gf2res = e(N, H, W, K), e(N, H, W, C2)
    nv = K * C2 + K
    part = e(tiles * nv)
    ops.fusion_out_bwd(d.za, d.zb, K, d.gout, b, g2["scale"], g2["shift"], d.wr, gz, gf2res, part)
    red = e(nv)
    ops.colsum(part, tiles, nv, red)
    gf2c = torch.zeros((N, H, W, 8), dtype=torch.float32, device=DEV)
    gf2c[..., :C2] = G["gc"].to(DEV)
    gffd, gbhat = e(N, H, W, C2), e(N, H, W, C2)
    part = e(tiles * 4 * K)
    ops.gate_bwd1(d.za, d.zb, K, ops.act(gf2c), gf2res, b, g2["mean"], g2["invstd"], d.gam2, d.bet2, gffd, gbhat, part)
    red2 = e(4 * K)
    ops.colsum(part, tiles, 4 * K, red2)
    nv1 = C2 * K + 2 * K
    gabn, part = e(N, H, W, K), e(tiles * nv1)
    ops.gate_bwd2(N, H, W, K, gbhat, b, g2["mean"], g2["invstd"], d.gam2, red2[:C2], red2[C2:], a, g1["mean"],
                  g1["invstd"], d.gam1, d.bet1, d.w2, gabn, part)
    red1 = e(nv1)
    ops.colsum(part, tiles, nv1, red1)
    db1, dg1 = red1[C2 * K:C2 * K + K], red1[C2 * K + K:]
    gz_a, gz_b = e(N, H, W, K), e(N, H, W, K)
    nw = K * C2 * 9
    part = e(gtiles * nw)
    ops.gate_bwd3(d.za, d.zb, K, gabn, a, g1["mean"], g1["invstd"], d.gam1, db1, dg1, d.w1, gffd, d.gaux_a, d.gaux_b,
                  gz_a, gz_b, part)
    dw1 = e(nw)
    ops.colsum(part, gtiles, nw, dw1)
    torch.cuda.synchronize()

    got = {"d za": gz_a, "d zb": gz_b, "d w1": dw1.view(K, C2, 3, 3), "d gam1": dg1, "d bet1": db1,
           "d w2": red1[:C2 * K].view(C2, K), "d gam2": red2[C2:], "d bet2": red2[:C2],
           "d wr": red[:K * C2].view(K, C2), "d br": red[K * C2:], "f2": f2[..., :C2], **run}
    assert float(f2[..., C2:].abs().max()) == 0.0
    assert torch.equal(gz.cpu(), nhwc(c.gout))
    failed = []
    for name, r in ref.items():
        mx = float(r.abs().max())
        err32 = float((ref32[name].double() - r).abs().max()) / mx
        err = float((got[name].detach().double().cpu() - r).abs().max()) / mx
        tol = max(1e-4, 3.0 * err32)
        print(f"gate composed K={K} {name}: fp32 autograd err {err32:.3e} -> gate {tol:.3e}, kernels {err:.3e}")
        if not err <= tol:
            failed.append((name, err, tol))
    assert not failed, failed


# ---- consistency pair -------------------------------------------------------------------------------------
def _consistency_ref(f, a, b, c0, c1, gl):
    ts = [t.double().clone().requires_grad_(True) for t in (f, a, b)]
    pf = F.softmax(ts[0], 1)
    ref = c0 * F.mse_loss(F.softmax(ts[1], 1), pf) + c1 * F.mse_loss(F.softmax(ts[2], 1), pf)
    (ref * gl).backward()
    return ref.item(), [t.grad for t in ts]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", [(3, 45, 47), (1, 1, 1)], ids=["3x45x47", "1x1x1"])
def test_consistency_pair(shape, K):
    """(3,45,47): 2115 px per sample, one full tile + 67.  Upstream gradient 3.7; K = 1 gives loss 0 and
    all-zero gradients.  The backward ACCUMULATES: called on buffers holding random values it must leave
    prefill + gradient (the prefill is scaled to the gradient so that the sum keeps its digits)."""
    from eunet.losses import consistency_loss
    ops = _ops()
    N, H, W = shape
    c0, c1, gl = 0.24, 0.2, 3.7
    gen = torch.Generator().manual_seed(3 + K + H)
    f, a, b = ((torch.randn(N, K, H, W, generator=gen, dtype=torch.float64) * 2).float() for _ in range(3))
    ref, grads = _consistency_ref(f, a, b, c0, c1, gl)
    gs = [t.to(DEV).requires_grad_(True) for t in (f, a, b)]
    out = consistency_loss(gs[0], gs[1], gs[2], c0, c1)
    (out * gl).backward()
    torch.cuda.synchronize()
    assert abs(out.item() - ref) <= 1e-5 * abs(ref), (out.item(), ref)
    scale = max(float(g.abs().max()) for g in grads)
    if K == 1:
        assert ref == 0.0 and scale == 0.0
    for t, r in zip(gs, grads):
        assert float((t.grad.double().cpu() - r).abs().max()) <= 1e-4 * float(r.abs().max())
    # the accumulate contract, through ops.consistency_bwd itself
    pre = [torch.randn(N, K, H, W, generator=gen) * (scale if scale > 0.0 else 1.0) for _ in range(3)]
    bufs = [p.to(DEV) for p in pre]
    gloss = torch.tensor([gl], dtype=torch.float32, device=DEV)
    ops.consistency_bwd(gs[0].detach(), gs[1].detach(), gs[2].detach(), c0, c1, gloss, bufs[0], bufs[1], bufs[2])
    torch.cuda.synchronize()
    for p, got, r in zip(pre, bufs, grads):
        if K == 1:
            assert torch.equal(got.cpu(), p)  # adds exactly 0
        else:
            # 1e-4 of the gradient as above, plus the rounding of the fp32 sum prefill + gradient
            tol = 1e-4 * float(r.abs().max()) + 2.0 ** -23 * float((p.double() + r).abs().max())
            assert float((got.double().cpu() - (p.double() + r)).abs().max()) <= tol
