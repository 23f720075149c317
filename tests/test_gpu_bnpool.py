"""bn_pool_up.hip kernel by kernel against fp64 references, at its block, unit and slot edges (GPU only).

tests/test_gpu_ops.py compares most of these kernels with each other (fused against unfused) and holds
their bf16 outputs to 2e-2 of the output scale; several (bn_bwd_apply_pool, bn_bwd_apply_1x1,
bn_eval_affine, colsum(split), the gout=None / gact=None / gskip=None modes) are reached only through
whole-model steps.  Here every kernel of the file is compared with the fp64 contract of its header
comment, element by element and partial row by partial row.

Inputs   seeded per case.  BN constants away from their defaults: signed gamma, |mean| in [0.2, 0.8],
         invstd in [0.5, 2].  Channel 0 of every BN'd tensor sits on the ReLU boundary: scale = 0.5,
         shift = -0.5 * 1.25 and y cycling through 1.25 and its two neighbours in the tensor's dtype, so
         y * scale + shift is exactly 0, +ulp/2 and -ulp/2.  Max-pool inputs hold windows whose four
         pre-activations are all negative, windows of equal values and windows of neighbouring values
         (ties made by the rounding of the stored activation); the plain adjoint also sees a NaN window.
Slots    every Act is a channel slice of a wider buffer with its own (ctot, coff), different for each
         tensor of a call; the other channels hold a sentinel that must survive.  Every flat output
         (partials, stats, z, reductions) carries a 64-element sentinel tail that must survive.
Runs     every kernel runs twice into fresh buffers, bit-equal.
Contract the ReLU mask is fmaf(y, scale, shift) > 0 on the fp32 constants: the reference forms
         y * scale + shift in fp64 (exact for these operands) and rounds once to fp32 (fma32()).  The
         max-pool argmax is an explicit loop over the stored (rounded) activation in window order
         (0,0), (0,1), (1,0), (1,1): a later tap wins only if greater or NaN.  The fused reductions and
         the recomputing applies use the gradient as stored (rounded to T); the reference rounds at the
         same point, so fused and unfused contracts are identical.

Shapes (the smallest that cross each edge; constants are those of bn_pool_up.hip)
  bn_finalize     tiles 1, 2, 1023, 1024, 1025 (tree width FNT = 1024), 8192, 8193 (sweep FNT * FB)
  conv_small      (1,1,1) (2,1,33) (2,17,1) (1,16,32) (3,19,37) (2,33,65): forward tile 16x32, weight
                  gradient tile 8x32, 64 output channels per blockIdx.y; cin 1 (C1 instance), 2, 4 | 5
                  (CI instance boundary), 8; cout 8, 64, 72, 96, and 60 / an odd slot (element stores)
  producers       (1,1,1) / (1,2,2), (2,2,66), (3,14,26), U = 1, 3, 12, 16 channel units; 1x1: P = 1, 127,
                  128, 129 around the 4 x 32-pixel block step and P = 8192 * 128 + 1 (grid wrap)
  upsample        (1,1,1) (2,1,5) (2,5,1) (1,4,2) (1,9,7) (3,13,21); (4,509,511,128) bf16 is the file's one
                  large case (the 8-rows-per-thread path needs >= 4096 * 256 threads)
  bn_bwd_*        P = 1, 63, 64, 65, 129 around the 64-pixel tile; (1,261,511): tpix = 128, ragged last tile;
                  U = 1, 3 (255-thread apply block, idle reduce thread), 12, 256 (limit); P = 4160 at
                  U = 256 wraps the apply's 4096-block grid; U = 257 raises
  conv1x1_bwd     P = 1, 31, 32, 33, 64, 65, 1023, 1024, 1025, 2049: the 32-pixel slot step, the two pixels
                  per iteration of J = 1, the 1024-pixel block; C = 8, 64, 72, 128 (J = 1 | 2)
  pool adjoints   (1,2,2) (2,2,6) (2,10,14); U = 1, 3, 12, 16, 96 (blocks of 256 and 192 threads); U = 5 is
                  not fusable; one grid wrap per cap (2048 reduce blocks, 8192 apply blocks)
  colsum          rows 1 .. 20000 (rb saturates at 256 from 16384 rows, chunk > 64 from 16385), cols 1 .. 130

Gates (derived from the arithmetic, not from what the kernels return)
  fp32 elements        max|got - ref| <= 1e-4 max|ref|                               (the project's gate)
  bf16 elements        |got - ref| <= 2^-8 |ref| + 1e-5 S per element: one rounding of an fp32 result
                       (2^-8 = twice the round-to-nearest bound), S = the sum of the absolute values of
                       the terms added to form the element (bn_bwd_apply: |k1 g'| + |k2 y| + |k3|); the
                       operand-exact conv gate keeps S = max|ref| as tests/test_gpu_ops.py has it
  partial rows         |got - ref| <= n_add * 2^-24 * sum|terms| over exactly the pixels of that block,
                       n_add = the serial fp32 additions on the kernel's longest path (a formula beside
                       each test); the block of a pixel follows from the kernel's grid-stride indexing
  colsum               |got - ref| <= 2^-23 |ref| + 2^-50 sum|terms| (fp64 accumulation, one rounding)
  conv_small stats     against the kernel's fp32 accumulators, emulated fma by fma in its order: counts exact; a
                       tile's sum is count x a Welford mean (16 updates per thread + 3 Chan merges of three
                       roundings each, one more for the product: n_add = 58 on count x max|v|); its M2, and the
                       batch variance, to 2e-4 of themselves (as the MFMA conv's statistics are held)
  bn_finalize          1e-6 relative against the fp64 closed form of the same stats buffer
  upsample forward     fp32: 1e-6 ref per element (four roundings of non-negative terms, 4 * 2^-24 = 2.4e-7;
                       the weights are exact binary fractions); bf16: one more rounding
  composed             fp32: 1e-4 max|ref|; bf16: the gradient the apply recomputes was rounded to bf16
                       before it was reduced and applied, so 2^-8 |ref| + (2^-9 + 1e-5) S', S' the apply's
                       terms with the reduced sums taken over absolute values
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
TAIL, SENT = 64, -12288.0          # (bf16-exact)
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
EOF = {F32: 4, BF16: 8}            # elements of a 16-byte channel unit
EPS24 = 2.0 ** -24
NT = 256                           # block size of most kernels of the file
Y0 = 1.25                          # the ReLU-boundary value of channel 0
BN_EPS, BN_MOM = 1e-5, 0.1
EPS32, MOM32 = float(torch.tensor(BN_EPS).float()), float(torch.tensor(BN_MOM).float())  # as the C ABI receives them
dts = pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])


def _ops():
    from eunet import ops
    return ops


def _err():
    from eunet import _lib
    return _lib.EunetError


def cdiv(a, b):
    return -(-a // b)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def rt(x, dt):
    """An fp32 result (held in fp64) rounded to the stored dtype."""
    return x.float().to(dt).double()


def fma32(a, b, c):
    """fmaf(a, b, c) of fp32 operands: the fp64 product and sum are exact here, rounded once to fp32."""
    return (a * b + c).float().double()


def ulp_of_y0(dt):
    return 2.0 ** -7 if dt == BF16 else 2.0 ** -23


# ---- buffers ------------------------------------------------------------------------------------------------
class Slots:
    """Acts as channel slices of wider buffers: a different (ctot, coff) for each tensor, sentinel elsewhere."""

    def __init__(self, dt):
        self.dt, self.E, self.k, self.outs = dt, EOF[dt], 0, []

    def _geom(self, C, geom):
        if geom is not None:
            return geom
        self.k += 1
        coff = self.E * (1 + self.k % 3)
        return coff, coff + C + self.E * (1 + (self.k // 3) % 2)

    def put(self, v, geom=None):
        """v [N,H,W,C] (values exact in dt) -> Act on the device."""
        N, H, W, C = v.shape
        coff, ctot = self._geom(C, geom)
        buf = torch.full((N, H, W, ctot), SENT, dtype=self.dt, device=DEV)
        buf[..., coff:coff + C] = v.to(DEV).to(self.dt)
        return _ops().act(buf, coff, C)

    def out(self, N, H, W, C, geom=None):
        coff, ctot = self._geom(C, geom)
        n = N * H * W * ctot
        flat = torch.full((n + TAIL,), SENT, dtype=self.dt, device=DEV)
        a = _ops().act(flat[:n].view(N, H, W, ctot), coff, C)
        self.outs.append((flat, n, a))
        return a

    def check(self):
        torch.cuda.synchronize()
        for flat, n, a in self.outs:
            s = torch.tensor(SENT, dtype=self.dt, device=DEV)
            assert bool((flat[n:] == s).all()), "tail overwritten"
            assert bool((a._keep[..., :a.coff] == s).all()) and bool((a._keep[..., a.coff + a.c:] == s).all()), \
                "channels outside the slot overwritten"


def val(a):
    """The slot's own channels."""
    return a._keep[..., a.coff:a.coff + a.c]


class Outs:
    """Flat output buffers with a sentinel tail; check() synchronises and asserts that every tail survived."""

    def __init__(self):
        self.items = []

    def new(self, shape, dtype=F32, fill=None):
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
            assert bool((flat[n:] == torch.tensor(SENT, device=DEV).to(flat.dtype)).all()), "tail overwritten"


def _same(x, y):
    if not x.is_floating_point():
        return torch.equal(x, y)
    return torch.equal(x.nan_to_num(nan=777.0), y.nan_to_num(nan=777.0))


def _twice(run, keep=False):
    """run() launches into fresh buffers and returns its outputs; both runs must agree bit for bit."""
    first, second = run(), run()
    for i, (x, y) in enumerate(zip(first, second)):
        assert _same(x, y), f"output {i} differs between two runs"
    return [t.detach() if keep else t.detach().cpu() for t in first]


# ---- gates --------------------------------------------------------------------------------------------------
def gate_el(name, got, ref, dt, S=None):
    """fp32: max|got - ref| <= 1e-4 max|ref|.  bf16: |got - ref| <= 2^-8 |ref| + 1e-5 S per element
    (S None: max|ref|, the operand-exact gate of tests/test_gpu_ops.py)."""
    got, ref = got.detach().double().to(ref.device).reshape(ref.shape), ref.double()
    assert bool(torch.isfinite(got).all()), name
    mx = float(ref.abs().max())
    err = (got - ref).abs()
    print(f"{name}: max err {float(err.max()):.3e} max|ref| {mx:.3e}")
    if dt == F32:
        assert float(err.max()) <= 1e-4 * mx, (name, float(err.max()), mx)
    else:
        bound = 2.0 ** -8 * ref.abs() + 1e-5 * (mx if S is None else S.reshape(ref.shape))
        bad = err > bound
        assert not bool(bad.any()), (name, int(bad.sum()), float((err / bound.clamp_min(1e-300)).max()))


def gate_sum(name, got, ref, mag, n_add):
    """Partial sums: |got - ref| <= n_add 2^-24 sum|terms|."""
    got = got.detach().double().to(ref.device).reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), name
    err, bound = (got - ref).abs(), n_add * EPS24 * mag
    print(f"{name}: worst err/bound {float((err / bound.clamp_min(1e-300)).max()):.3e} (n_add {n_add})")
    bad = err > bound
    assert not bool(bad.any()), (name, int(bad.sum()), float((err / bound.clamp_min(1e-300)).max()))


def gate_colsum(name, got, ref, mag, extra=None):
    """colsum: fp64 accumulation and one rounding; extra: what its fp32 inputs already carry."""
    got = got.detach().double().to(ref.device).reshape(ref.shape)
    bound = 2.0 ** -23 * ref.abs() + 2.0 ** -50 * mag + (0.0 if extra is None else extra)
    bad = (got - ref).abs() > bound
    assert not bool(bad.any()), (name, int(bad.sum()), float(((got - ref).abs() / bound.clamp_min(1e-300)).max()))


# ---- inputs -------------------------------------------------------------------------------------------------
class Bn:
    """fp32 BN constants on the host (.mean .istd .gam .bet .sc .sh), .d.* on the device, .r.* in fp64."""

    def __init__(self, C, g, boundary=True):
        def ru(n):
            return torch.rand(n, generator=g)

        def sign(n):
            return torch.where(ru(n) < 0.5, -1.0, 1.0)

        self.mean, self.istd = sign(C) * (0.2 + 0.6 * ru(C)), 0.5 + 1.5 * ru(C)
        self.gam, self.bet = sign(C) * (0.5 + ru(C)), 0.3 * torch.randn(C, generator=g)
        self.sc = (self.gam.double() * self.istd.double()).float()
        self.sh = (self.bet.double() - self.mean.double() * self.sc.double()).float()
        if boundary:  # channel 0: y * 0.5 - 0.5 Y0, exactly 0 at y = Y0
            self.sc[0], self.sh[0] = 0.5, -0.5 * Y0
        self._mk()

    def _mk(self):
        names = ("mean", "istd", "gam", "bet", "sc", "sh")
        self.d = type("Dev", (), {k: getattr(self, k).to(DEV) for k in names})
        self.r = type("Ref", (), {k: getattr(self, k).double() for k in names})

    def on(self, dev):
        return type("Ref", (), {k: getattr(self, k).double().to(dev) for k in ("mean", "istd", "gam", "bet", "sc", "sh")})


def rand_y(shape, dt, g):
    """[N,H,W,C] fp64 values exact in dt; channel 0 cycles through Y0 and its two neighbours in dt."""
    y = rt(0.3 + torch.randn(*shape, generator=g, dtype=torch.float64), dt)
    P = shape[0] * shape[1] * shape[2]
    u = ulp_of_y0(dt)
    y.view(P, -1)[:, 0] = Y0 + u * ((torch.arange(P) % 3).double() - 1.0)  # Y0 - ulp, Y0, Y0 + ulp
    assert torch.equal(rt(y, dt), y)
    return y


def rand_t(shape, dt, g, scale=1.0):
    return rt(scale * torch.randn(*shape, generator=g, dtype=torch.float64), dt)


# ---- fp64 pieces of the contract ----------------------------------------------------------------------------
def ref_mask(y, r):
    return fma32(y, r.sc, r.sh) > 0


def ref_act32(y, r):
    return fma32(y, r.sc, r.sh).clamp_min(0.0)


def ref_terms(g, y, r):
    """(g', g' xhat) of the BN-backward reduction, g the gradient as stored."""
    gp = torch.where(ref_mask(y, r), g, torch.zeros_like(g))
    return gp, gp * ((y - r.mean) * r.istd)


def ref_apply(g, y, r, dbeta, dgamma, n):
    """gy = gamma istd (g' - dbeta / n - xhat dgamma / n) as k1 g' + k2 y + k3, and S = |k1 g'| + |k2 y| + |k3|."""
    gp = torch.where(ref_mask(y, r), g, torch.zeros_like(g))
    k1 = r.sc
    k2 = -r.sc * r.istd * dgamma / n
    k3 = -r.sc * (-r.mean * r.istd * dgamma / n + dbeta / n)
    return k1 * gp + k2 * y + k3, (k1 * gp).abs() + (k2 * y).abs() + k3.abs().expand_as(y)


def win(t):
    """[N,H,W,C] -> [N,H/2,W/2,4,C], taps in window order (0,0), (0,1), (1,0), (1,1)."""
    return torch.stack([t[:, 0::2, 0::2], t[:, 0::2, 1::2], t[:, 1::2, 0::2], t[:, 1::2, 1::2]], 3)


def unwin(w4):
    N, Ho, Wo, _, C = w4.shape
    t = torch.empty(N, 2 * Ho, 2 * Wo, C, dtype=w4.dtype, device=w4.device)
    t[:, 0::2, 0::2], t[:, 0::2, 1::2], t[:, 1::2, 0::2], t[:, 1::2, 1::2] = w4.unbind(3)
    return t


def ref_argmax(a4):
    """First maximum in window order over the stored activation; a NaN wins."""
    best, arg = a4[..., 0, :].clone(), torch.zeros_like(a4[..., 0, :], dtype=torch.long)
    for k in range(1, 4):
        v = a4[..., k, :]
        upd = (v > best) | torch.isnan(v)
        best, arg = torch.where(upd, v, best), torch.where(upd, torch.full_like(arg, k), arg)
    return best, arg


def ref_pool_bwd(act_st, gp, gs, dt):
    """gout = gskip + scatter(gpool) at the argmax, formed in fp32 and rounded to T; and S = |gs| + |scattered gp|."""
    _, arg = ref_argmax(win(act_st))
    sc4 = torch.stack([torch.where(arg == k, gp, torch.zeros_like(gp)) for k in range(4)], 3)
    sc = unwin(sc4)
    tot = sc if gs is None else sc + gs
    return rt(tot, dt), sc.abs() + (0.0 if gs is None else gs.abs())


def ref_up_adj(g):
    """fp64 adjoint of F.interpolate(scale_factor=2, bilinear, align_corners=False): g [N,2h,2w,C] -> [N,h,w,C]."""
    N, H2, W2, C = g.shape
    x = torch.zeros(N, C, H2 // 2, W2 // 2, dtype=torch.float64, device=g.device, requires_grad=True)
    F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False).backward(nchw(g))
    return nhwc(x.grad)


def rows_ref(block, t, rows):
    """block [P,C] (the partial row of each pixel and channel), t [P,C] -> (row sums, sums of |t|) [rows,C]."""
    out = torch.zeros(rows, t.shape[1], dtype=torch.float64, device=t.device)
    mag = torch.zeros_like(out)
    out.scatter_add_(0, block, t)
    mag.scatter_add_(0, block, t.abs())
    return out, mag


def check_bn_part(name, part, rows, block, t1, t2, n_add):
    """part [rows][2][C] row by row against the fp64 sums over each block's own pixels, then its colsum (split into
    dbeta | dgamma) against the totals.  Returns (dbeta, dgamma) fp32 on the device."""
    ops = _ops()
    C = t1.shape[1]
    pv = part.to(t1.device).view(rows, 2, C)
    bounds = []
    for i, t in enumerate((t1, t2)):
        ref, mag = rows_ref(block, t, rows)
        gate_sum(f"{name} part[{i}]", pv[:, i], ref, mag, n_add)
        bounds.append((n_add * EPS24 * mag).sum(0))
    o = Outs()
    db, dg = o.new(C), o.new(C)
    ops.colsum(part.to(DEV), rows, 2 * C, db, split=C, out_hi=dg)
    o.check()
    gate_colsum(name + " dbeta", db, t1.sum(0), t1.abs().sum(0), bounds[0])
    gate_colsum(name + " dgamma", dg, t2.sum(0), t2.abs().sum(0), bounds[1])
    return db, dg


def bwd_pix(P):
    pix = ((P // 2048 + 63) // 64) * 64
    return min(max(pix, 64), 1024)


def bnr_block(U):
    return NT if NT % U == 0 else (192 if 192 % U == 0 else 0)


# ---- A. BN statistics ---------------------------------------------------------------------------------------
def _stats_buf(tiles, C, g, offset=0.0, counts=None):
    """[tiles][2][C] (sum, M2) + [tiles] counts, ragged counts 1 .. 512 with empty tiles in the middle and at the end
    (their sums hold garbage that must be ignored)."""
    if counts is None:
        counts = torch.randint(1, 513, (tiles,), generator=g).double()
        if tiles > 4:
            counts[[tiles // 3, tiles // 2, tiles // 2 + 1, tiles - 1]] = 0.0
    tm = offset + torch.randn(tiles, C, generator=g, dtype=torch.float64)
    m2 = counts[:, None] * (0.5 + torch.rand(tiles, C, generator=g, dtype=torch.float64))
    m2[counts <= 1] = 0.0
    body = torch.stack([tm * counts[:, None], m2], 1)
    body[counts == 0] = 1e30
    return torch.cat([body.reshape(-1), counts]).float()


def _finalize_ref(st, tiles, C, gam, bet, rm, rv):
    st = st.double()
    body, n_t = st[:2 * C * tiles].view(tiles, 2, C), st[2 * C * tiles:]
    on = n_t > 0
    S, M2, n_t = body[on, 0], body[on, 1], n_t[on]
    n = n_t.sum()
    mean = S.sum(0) / n
    m2 = (M2 + n_t[:, None] * (S / n_t[:, None] - mean) ** 2).sum(0)
    var_b = m2 / n
    var_u = m2 / (n - 1) if n > 1 else var_b
    istd = 1.0 / torch.sqrt(var_b + EPS32)
    sc = gam.double() * istd
    return dict(mean=mean, istd=istd, sc=sc, sh=bet.double() - mean * sc,
                rm=(1 - MOM32) * rm.double() + MOM32 * mean, rv=(1 - MOM32) * rv.double() + MOM32 * var_u)


def _rel6(name, got, ref, floor):
    """1e-6 relative per element; floor: the magnitude of the quantities the element was formed from (an
    fp64 cancellation leaves about 1e-16 of those, far below 1e-12)."""
    err = (got.double().cpu() - ref).abs()
    assert bool((err <= 1e-6 * ref.abs() + 1e-12 * floor).all()), (name, float(err.max()), float(ref.abs().max()))


def _run_finalize(st, tiles, C, g, outs="all", nbt0=5):
    ops = _ops()
    gam = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0) * (0.5 + torch.rand(C, generator=g))
    bet = 0.3 * torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    std = st.to(DEV)

    def run():
        o = Outs()
        rm, rv = o.new(C), o.new(C)
        rm.copy_(rm0)
        rv.copy_(rv0)
        res = {k: o.new(C) for k in ("mean", "istd", "sc", "sh")}
        nbt = o.new(1, dtype=torch.int64, fill=nbt0)
        use = {k: (v if outs == "all" or k in outs else None) for k, v in res.items()}
        run_stats = outs == "all" or "run" in outs
        ops.bn_finalize(std, tiles, C, gam.to(DEV), bet.to(DEV), BN_EPS, BN_MOM, rm if run_stats else None,
                        rv if run_stats else None, use["mean"], use["istd"], use["sc"], use["sh"],
                        nbt if run_stats else None)
        o.check()
        return [rm, rv, nbt] + [res[k] for k in ("mean", "istd", "sc", "sh")]

    rm, rv, nbt, mean, istd, sc, sh = _twice(run)
    ref = _finalize_ref(st, tiles, C, gam, bet, rm0, rv0)
    floor = float(st[:2 * C * tiles][st[:2 * C * tiles] < 1e29].abs().max()) + 1.0
    for k, got in (("mean", mean), ("istd", istd), ("sc", sc), ("sh", sh)):
        if outs == "all" or k in outs:
            _rel6(k, got, ref[k], floor)
        else:
            assert bool((got == SENT).all()), k
    if outs == "all" or "run" in outs:
        _rel6("run_mean", rm, ref["rm"], floor)
        _rel6("run_var", rv, ref["rv"], floor)
        assert int(nbt) == nbt0 + 1  # one per call, not one per channel block
    else:
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0) and int(nbt) == nbt0
    return ref


@pytest.mark.parametrize("tiles", [1, 2, 1023, 1024, 1025, 8192, 8193])
def test_bn_finalize_tiles(tiles):
    for C in (1, 3, 64):
        g = torch.Generator().manual_seed(1000 * tiles + C)
        _run_finalize(_stats_buf(tiles, C, g), tiles, C, g)


def test_bn_finalize_offset_mean():
    """Channel means of about 300 with unit spread: the variance stays accurate relative to the variance."""
    g = torch.Generator().manual_seed(11)
    ref = _run_finalize(_stats_buf(1025, 3, g, offset=300.0), 1025, 3, g)
    assert float(ref["mean"].min()) > 290 and float(1 / ref["istd"].max() ** 2) < 5


def test_bn_finalize_single_sample():
    """n = 1 in total: var_u = var_b = 0, invstd = 1 / sqrt(eps), no division by zero."""
    g = torch.Generator().manual_seed(12)
    for tiles, counts in ((1, [1.0]), (3, [0.0, 1.0, 0.0])):
        ref = _run_finalize(_stats_buf(tiles, 3, g, counts=torch.tensor(counts, dtype=torch.float64)), tiles, 3, g)
        assert bool((ref["istd"] == 1.0 / math.sqrt(EPS32)).all())


@pytest.mark.parametrize("outs", [("mean", "istd"), ("sc", "sh", "run"), ("mean", "istd", "sc", "sh"), ("sc", "sh")],
                         ids=lambda o: "+".join(o))
def test_bn_finalize_optional_outputs(outs):
    """The None combinations of the engine (statistics only; affine with / without the running update)."""
    g = torch.Generator().manual_seed(13)
    _run_finalize(_stats_buf(5, 3, g), 5, 3, g, outs=outs)


def test_bn_finalize_update_guard():
    """While the update guard is raised run_mean / run_var / num_batches_tracked stay bit-unchanged and mean, invstd,
    scale and shift are still written."""
    ops = _ops()
    g = torch.Generator().manual_seed(14)
    tiles, C = 7, 3
    st = _stats_buf(tiles, C, g)
    gam, bet = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    guard = torch.ones(1, dtype=torch.float64, device=DEV)
    prev = ops.update_guard(DEV)
    o = Outs()
    rm, rv = o.new(C), o.new(C)
    rm.copy_(rm0)
    rv.copy_(rv0)
    mean, istd, sc, sh = (o.new(C) for _ in range(4))
    nbt = o.new(1, dtype=torch.int64, fill=9)
    ref = _finalize_ref(st, tiles, C, gam, bet, rm0, rv0)
    floor = float(st[st < 1e29].abs().max()) + 1.0
    try:
        ops.set_update_guard(DEV, guard)
        ops.bn_finalize(st.to(DEV), tiles, C, gam.to(DEV), bet.to(DEV), BN_EPS, BN_MOM, rm, rv, mean, istd, sc, sh, nbt)
        o.check()
        assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0) and int(nbt) == 9
        for k, got in (("mean", mean), ("istd", istd), ("sc", sc), ("sh", sh)):  # written under the guard
            _rel6(k + " (guarded)", got, ref[k], floor)
            got.fill_(SENT)
        guard.zero_()  # lowered: the same call updates
        ops.bn_finalize(st.to(DEV), tiles, C, gam.to(DEV), bet.to(DEV), BN_EPS, BN_MOM, rm, rv, mean, istd, sc, sh, nbt)
        o.check()
    finally:
        ops.set_update_guard(DEV, prev)
    for k, got in (("mean", mean), ("istd", istd), ("sc", sc), ("sh", sh), ("rm", rm), ("rv", rv)):
        _rel6(k, got, ref[k], floor)
    assert int(nbt) == 10


@pytest.mark.parametrize("C", [1, 255, 256, 257])
def test_bn_eval_affine(C):
    """scale = gamma / sqrt(run_var + eps), shift = beta - run_mean scale: 1e-6 of the terms (fp32 arithmetic,
    three roundings of 2^-24 in scale, two more in shift)."""
    ops = _ops()
    g = torch.Generator().manual_seed(20 + C)
    gam = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0) * (0.5 + torch.rand(C, generator=g))
    bet, rm, rv = torch.randn(C, generator=g), torch.randn(C, generator=g), 0.05 + torch.rand(C, generator=g)

    def run():
        o = Outs()
        sc, sh = o.new(C), o.new(C)
        ops.bn_eval_affine(gam.to(DEV), bet.to(DEV), rm.to(DEV), rv.to(DEV), BN_EPS, sc, sh)
        o.check()
        return sc, sh

    sc, sh = _twice(run)
    rs = gam.double() / torch.sqrt(rv.double() + BN_EPS)
    assert bool(((sc.double() - rs).abs() <= 1e-6 * rs.abs()).all())
    assert bool(((sh.double() - (bet.double() - rm.double() * rs)).abs() <= 1e-6 * (bet.double().abs() + (rm.double() * rs).abs())).all())


# ---- B. the direct conv -------------------------------------------------------------------------------------
# every shape, cin and cout with every dtype; (cout 60 | an odd slot: the element-store path of the forward)
CONV_CASES = [((1, 1, 1), 1, 8, None), ((2, 1, 33), 2, 64, None), ((2, 17, 1), 4, 72, None), ((1, 16, 32), 5, 96, None),
              ((3, 19, 37), 8, 72, None), ((2, 33, 65), 1, 96, None), ((3, 19, 37), 4, 60, None),
              ((2, 17, 1), 5, 64, (3, 75))]
conv_cases = pytest.mark.parametrize("shape,cin,cout,ygeom", CONV_CASES,
                                     ids=[f"{'x'.join(map(str, s))}-ci{ci}-co{co}{'-odd' if yg else ''}"
                                          for s, ci, co, yg in CONV_CASES])
SFH, STH, STW = 16, 8, 32


@functools.lru_cache(maxsize=None)
def _conv_case(shape, cin, cout, dt, bias):
    N, H, W = shape
    g = torch.Generator().manual_seed(97 * N * H * W + 13 * cin + cout)
    x = rand_t((N, H, W, cin), dt, g)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / 3).float()
    b = (bias + torch.randn(cout, generator=g)).float()
    ref = nhwc(F.conv2d(nchw(x), w.double(), b.double(), padding=1))
    # the kernel's fp32 accumulators, fma by fma in its order (bias, then input channel by input channel, tap by
    # tap): the statistics are taken from these, before any rounding of the output
    xp = F.pad(nchw(x), (1, 1, 1, 1))
    acc = b.double()[None, :, None, None].expand(N, cout, H, W)
    for ci in range(cin):
        for t in range(9):
            ky, kx = divmod(t, 3)
            acc = fma32(w.double()[None, :, ci, ky, kx, None, None], xp[:, ci:ci + 1, ky:ky + H, kx:kx + W], acc)
    gy = rand_t((N, H, W, cout), dt, g)
    return x, w, b, ref, gy, nhwc(acc)


def _check_conv_stats(st, ref, shape, cout):
    """st[tile][0][c] = sum, st[tile][1][c] = M2 about the tile's mean, counts at st[2 cout tiles + tile], decoded
    tile by tile (16 x 32 tiles in sample-major order); ref: the fp32 accumulators (emulated, held in fp64)."""
    N, H, W = shape
    ty, tx = cdiv(H, SFH), cdiv(W, STW)
    tiles = N * ty * tx
    st = st.double().cpu()
    assert st.numel() == tiles * (2 * cout + 1)
    body, cnt = st[:2 * cout * tiles].view(tiles, 2, cout), st[2 * cout * tiles:]
    for n in range(N):
        for iy in range(ty):
            for ix in range(tx):
                t = (n * ty + iy) * tx + ix
                v = ref[n, iy * SFH:(iy + 1) * SFH, ix * STW:(ix + 1) * STW].reshape(-1, cout)
                k = v.shape[0]
                assert cnt[t].item() == k, (t, cnt[t].item(), k)
                # the sum is count x a Welford mean: a thread updates over its SFH = 16 pixels (one per pass), then
                # 3 Chan merges across lanes, three roundings each on values up to max|v|, one rounding of the
                # product: n_add = 3 (16 + 3) + 1 on count x max|v|
                gate_sum(f"sum tile {t}", body[t, 0], v.sum(0), k * v.abs().max(0).values, 3 * (SFH + 3) + 1)
                # M2 relative to the M2 of the same accumulators: 2e-4, as the MFMA conv's statistics are held
                m2 = ((v - v.mean(0)) ** 2).sum(0)
                err = (body[t, 1] - m2).abs()
                assert bool((err <= 2e-4 * m2).all()), (t, float((err / m2.clamp_min(1e-300)).max()))
    # and the batch variance from these partials, relative to the variance
    S, M2, nt = body[:, 0], body[:, 1], cnt[:, None]
    mean = S.sum(0) / nt.sum()
    var = (M2 + nt * (S / nt - mean) ** 2).sum(0) / nt.sum()
    vref = ref.reshape(-1, cout).var(0, unbiased=False)
    if N * H * W > 1:
        assert float(((var - vref).abs() / vref).max()) < 2e-4


@dts
@conv_cases
def test_conv_small_fwd(shape, cin, cout, ygeom, dt):
    ops = _ops()
    N, H, W = shape
    for bias in (0.0, 300.0):
        x, w, b, ref, _, acc = _conv_case(shape, cin, cout, dt, bias)
        tiles = N * cdiv(H, SFH) * cdiv(W, STW)

        def run(stats=True):
            s, o = Slots(dt), Outs()
            xa = s.put(x, (3, cin + 5))
            ya = s.out(N, H, W, cout, ygeom)
            st = o.new(tiles * (2 * cout + 1)) if stats else None
            ops.conv_small_fwd(xa, w.to(DEV), b.to(DEV), ya, st)
            s.check()
            o.check()
            return [val(ya)] + ([st] if stats else [])

        y, st = _twice(run)
        gate_el(f"conv_small_fwd bias {bias}", y, ref, dt)
        _check_conv_stats(st, acc, shape, cout)
        (y2,) = _twice(lambda: run(False))
        assert torch.equal(y2, y)


@dts
def test_conv_small_rejects(dt):
    ops, E = _ops(), EOF[dt]
    x9 = torch.zeros(1, 4, 4, 9, dtype=dt, device=DEV)
    y = torch.zeros(1, 4, 4, 64, dtype=dt, device=DEV)
    st = torch.zeros(2 * 64 + 1, device=DEV)
    with pytest.raises(_err()):
        ops.conv_small_fwd(ops.act(x9), torch.zeros(64, 9, 3, 3, device=DEV), None, ops.act(y), st)
    x = torch.zeros(1, 4, 4, 4, dtype=dt, device=DEV)
    dwp, dbp = torch.zeros(4 * 64 * 36, device=DEV), torch.zeros(4 * 64, device=DEV)
    with pytest.raises(_err()):
        ops.conv_small_wgrad(ops.act(x9), ops.act(y), torch.zeros(64 * 81, device=DEV), dbp, 1)
    # dY is read in whole 16-byte units: a channel count, slot or row stride that is no multiple of one is refused
    wide = torch.zeros(1, 4, 4, 64 + E, dtype=dt, device=DEV)
    odd = torch.zeros(1, 4, 4, 64 + E + 1, dtype=dt, device=DEV)
    for dy in (ops.act(wide, 0, 64 - E // 2), ops.act(wide, E // 2, 56), ops.act(odd, 0, 64),
               ops.act(torch.zeros(1, 4, 4, 60 if dt == BF16 else 62, dtype=dt, device=DEV))):
        with pytest.raises(_err()):
            ops.conv_small_wgrad(ops.act(x), dy, dwp, dbp, 1)
    with pytest.raises(_err()):  # 1 tile: 2 splits do not exist
        ops.conv_small_wgrad(ops.act(x), ops.act(y), dwp, dbp, 2)
    for other in ((1, 5, 4), (1, 4, 5), (2, 4, 4)):  # x and dy must agree in n, h and w
        with pytest.raises(_err()):
            ops.conv_small_wgrad(ops.act(x), ops.act(torch.zeros(*other, 64, dtype=dt, device=DEV)), dwp, dbp, 1)
    torch.cuda.synchronize()


@dts
@pytest.mark.parametrize("shape,cin,cout", [c[:3] for c in CONV_CASES[:6]],
                         ids=[f"{'x'.join(map(str, s))}-ci{ci}-co{co}" for s, ci, co, _ in CONV_CASES[:6]])
def test_conv_small_wgrad(shape, cin, cout, dt):
    """dw against the fp64 weight gradient of the rounded operands, db against the column sum, both 1e-5 of the
    largest value (as the conv3x3 weight gradient is held), with the library's split and a hand-picked one whose
    8 x 32 tile ranges cross samples."""
    ops = _ops()
    N, H, W = shape
    x, _, _, _, gy, _ = _conv_case(shape, cin, cout, dt, 0.0)
    wt = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(nchw(x), wt, None, padding=1).backward(nchw(gy))
    ntiles = N * cdiv(H, STH) * cdiv(W, STW)
    tpi = ntiles // N
    crossing = [s for s in range(2, ntiles) if cdiv(ntiles, cdiv(ntiles, s)) == s and cdiv(ntiles, s) % tpi]
    assert crossing or ntiles <= 2 * N
    s0 = Slots(dt)
    splits = [ops.conv_small_wgrad_splits(s0.put(gy))] + crossing[:1]
    for ns in splits:
        def run():
            s, o = Slots(dt), Outs()
            xa, da = s.put(x, (3, cin + 5)), s.put(gy)
            dwp, dbp = o.new(ns * cout * 9 * cin), o.new(ns * cout)
            dw, db = o.new((cout, cin, 3, 3)), o.new(cout)
            ops.conv_small_wgrad(xa, da, dwp, dbp, ns)
            ops.wgrad_reduce(dwp, dbp, ns, cout, cin, 9, dw, db)
            o.check()
            return dw, db

        dw, db = _twice(run)
        rdw, rdb = wt.grad, gy.sum(dim=(0, 1, 2))
        e_dw = float((dw.double() - rdw).abs().max() / rdw.abs().max().clamp_min(1e-30))
        e_db = float((db.double() - rdb).abs().max() / rdb.abs().max().clamp_min(1e-30))
        print(f"wgrad ns {ns}: dw {e_dw:.2e} db {e_db:.2e}")
        assert e_dw < 1e-5 and e_db < 1e-5, (ns, e_dw, e_db)
    with pytest.raises(_err()):  # a split count the tile count does not produce
        s = Slots(dt)
        ops.conv_small_wgrad(s.put(x, (3, cin + 5)), s.put(gy), torch.zeros((ntiles + 1) * cout * 9 * cin, device=DEV),
                             None, ntiles + 1)
    torch.cuda.synchronize()


# ---- C. forward producers -----------------------------------------------------------------------------------
FWD_SHAPES = [(1, 2, 2), (2, 2, 66), (3, 14, 26)]
FWD_U = [1, 3, 12, 16]
fwd_cases = pytest.mark.parametrize("shape,U", [(s, u) for s in FWD_SHAPES for u in FWD_U],
                                    ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"U{v}")


@dts
@fwd_cases
def test_bnrelu_and_pool(shape, U, dt):
    """bnrelu: one rounding of relu(fmaf(y, scale, shift)); bnrelu_pool stores the same activation and its 2x2
    maximum, which equals the maximum over the stored activation exactly (rounding is monotone)."""
    ops = _ops()
    N, H, W = shape
    C = U * EOF[dt]
    g = torch.Generator().manual_seed(300 + 7 * N * H * W + U)
    bn = Bn(C, g)

    def check_bnrelu(yv):
        def run():
            s = Slots(dt)
            ya, oa = s.put(yv), s.out(*yv.shape[:3], C)
            ops.bnrelu(ya, bn.d.sc, bn.d.sh, oa)
            s.check()
            return [val(oa)]

        (z,) = _twice(run)
        ref = ref_act32(yv, bn.r)
        gate_el("bnrelu", z, ref, dt, S=ref)
        assert torch.equal(z.double(), rt(ref, dt))  # one correctly rounded fma: nothing left to tolerate
        return ref

    if shape == (1, 2, 2):  # bnrelu also at a single pixel
        check_bnrelu(rand_y((1, 1, 1, C), dt, g))
    y = rand_y(shape + (C,), dt, g)
    a32 = check_bnrelu(y)
    for with_act in (True, False):
        def run():
            s = Slots(dt)
            ya, pa = s.put(y), s.out(N, H // 2, W // 2, C)
            aa = s.out(N, H, W, C) if with_act else None
            ops.bnrelu_pool(ya, bn.d.sc, bn.d.sh, aa, pa)
            s.check()
            return [val(pa)] + ([val(aa)] if with_act else [])

        got = _twice(run)
        stored = rt(a32, dt)
        if with_act:
            assert torch.equal(got[1].double(), stored)
            assert torch.equal(got[0], win(got[1]).max(3).values)
        assert torch.equal(got[0].double(), win(stored).max(3).values)


C1X_CASES = [(C, K) for C in (8, 64, 72, 128) for K in (1, 2, 3)]


def _c1x_inputs(P, C, K, dt, seed):
    g = torch.Generator().manual_seed(seed)
    bn = Bn(C, g)
    y = rand_y((1, 1, P, C), dt, g)
    w = (0.3 * torch.randn(K, C, generator=g)).float()
    b = torch.randn(K, generator=g).float()
    return bn, y, w, b


@dts
@pytest.mark.parametrize("C,K", C1X_CASES)
def test_bnrelu_conv1x1(C, K, dt):
    """z[p][k] = b[k] + sum_c W[k][c] relu(bn(y))[p][c] in fp32: per element n_add 2^-24 S with S = |b| + sum |W a| and
    n_add = 16 fmas per lane + 3 octet butterflies + the bias = 20; around the 128-pixel block step."""
    ops = _ops()
    for P in (1, 127, 128, 129):
        bn, y, w, b = _c1x_inputs(P, C, K, dt, 400 + P + C + K)

        def run():
            s, o = Slots(dt), Outs()
            z = o.new((P, K))
            ops.bnrelu_conv1x1(s.put(y), bn.d.sc, bn.d.sh, w.to(DEV), b.to(DEV), K, z)
            o.check()
            return [z]

        (z,) = _twice(run)
        a = ref_act32(y.view(P, C), bn.r)
        ref = a @ w.double().t() + b.double()
        S = a @ w.double().abs().t() + b.double().abs()
        gate_el("z", z, ref, F32)
        gate_sum("z per element", z, ref, S, 20)


@dts
def test_bnrelu_conv1x1_grid_wrap(dt):
    """P = 8192 * 128 + 1: the 8192-block grid wraps; the last pixel is the only one of its second step."""
    ops = _ops()
    P, C, K = 8192 * 128 + 1, 8, 2
    bn, y, w, b = _c1x_inputs(P, C, K, dt, 499)

    def run():
        s, o = Slots(dt), Outs()
        z = o.new((P, K))
        ops.bnrelu_conv1x1(s.put(y), bn.d.sc, bn.d.sh, w.to(DEV), b.to(DEV), K, z)
        o.check()
        return [z]

    (z,) = _twice(run)
    a = ref_act32(y.view(P, C), bn.r)
    gate_sum("z", z, a @ w.double().t() + b.double(), a @ w.double().abs().t() + b.double().abs(), 20)


UP_SHAPES = [(1, 1, 1), (2, 1, 5), (2, 5, 1), (1, 4, 2), (1, 9, 7), (3, 13, 21)]


def _gate_up(got, ref, dt):
    """ref >= 0 is its own sum of terms: fp32 1e-6 ref; bf16 one rounding more, (2^-8 + 1e-5) ref."""
    err = (got.double() - ref).abs()
    bound = (1e-6 if dt == F32 else 2.0 ** -8 + 1e-5) * ref
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())


@dts
@pytest.mark.parametrize("U", [1, 3])
@pytest.mark.parametrize("shape", UP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bnrelu_upsample(shape, U, dt):
    ops = _ops()
    N, h, w = shape
    C = U * EOF[dt]
    g = torch.Generator().manual_seed(500 + 7 * N * h * w + U)
    bn = Bn(C, g)
    y = rand_y(shape + (C,), dt, g)

    def run():
        s = Slots(dt)
        oa = s.out(N, 2 * h, 2 * w, C)
        ops.bnrelu_upsample(s.put(y), bn.d.sc, bn.d.sh, oa)
        s.check()
        return [val(oa)]

    (up,) = _twice(run)
    ref = nhwc(F.interpolate(nchw(ref_act32(y, bn.r)), scale_factor=2, mode="bilinear", align_corners=False))
    _gate_up(up, ref, dt)


def test_bnrelu_upsample_eight_rows_per_thread():
    """(4,509,511,128) bf16: 4 * 64 * 256 * 16 threads = 4096 blocks, the smallest grid that takes 8 rows per thread;
    the last row block has 5 rows and the last column pair is single.  Reference in fp64 on the device."""
    ops = _ops()
    N, h, w, C, dt = 4, 509, 511, 128, BF16
    g = torch.Generator(device=DEV).manual_seed(77)
    bn = Bn(C, torch.Generator().manual_seed(77))
    ybuf = torch.full((N, h, w, C + 16), SENT, dtype=dt, device=DEV)
    ybuf[..., 8:8 + C] = (0.3 + torch.randn(N, h, w, C, generator=g, device=DEV)).to(dt)
    ya = ops.act(ybuf, 8, C)
    r = bn.on(DEV)

    def run():
        s = Slots(dt)
        oa = s.out(N, 2 * h, 2 * w, C)
        ops.bnrelu_upsample(ya, bn.d.sc, bn.d.sh, oa)
        s.check()
        return [val(oa)]

    (up,) = _twice(run, keep=True)
    ref = F.interpolate(ref_act32(val(ya).double(), r).permute(0, 3, 1, 2), scale_factor=2, mode="bilinear",
                        align_corners=False).permute(0, 2, 3, 1)
    _gate_up(up, ref, dt)


# ---- D1. bn_bwd_reduce + colsum, bn_bwd_apply ---------------------------------------------------------------
BWD_SHAPES = [(1, 1, 1), (1, 7, 9), (1, 8, 8), (1, 5, 13), (3, 1, 43)]
BWD_CASES = [(s, u) for s in BWD_SHAPES for u in (1, 3, 12, 256)] + [((1, 261, 511), 1), ((1, 64, 65), 256)]


def _check_apply(name, gy, g, y, r, db, dg, P, dt):
    ref, S = ref_apply(g, y, r, db.double().to(g.device), dg.double().to(g.device), float(P))
    gate_el(name, gy, ref, dt, S=S)


@dts
@pytest.mark.parametrize("shape,U", BWD_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"U{v}")
def test_bn_bwd_reduce_apply(shape, U, dt):
    """bn_bwd_reduce: block b sums the pixels [b tpix, min(P, (b + 1) tpix)); a thread adds ceil(tpix / slots) pixels of
    its slot, thread 0 of a unit then adds the slots serially: n_add = ceil(tpix / slots) + slots, slots = 256 // U.
    bn_bwd_apply with the reduced sums against the header's formula, and with dbeta = dgamma = 0, where
    gy = scale g' shows the mask itself."""
    ops = _ops()
    N, H, W = shape
    if (1, 261, 511) == shape and dt == F32:
        U = 2  # C = 8
    P, C = N * H * W, U * EOF[dt]
    g = torch.Generator().manual_seed(600 + 7 * P + U)
    bn = Bn(C, g)
    y = rand_y(shape + (C,), dt, g)
    gr = rand_t(shape + (C,), dt, g)
    gr[gr == 0] = 1.0
    tpix = bwd_pix(P)
    tiles = cdiv(P, tpix)

    def run():
        s, o = Slots(dt), Outs()
        ga, ya = s.put(gr), s.put(y)
        assert ops.bn_bwd_tiles(ya) == tiles
        part = o.new(tiles * 2 * C)
        ops.bn_bwd_reduce(ga, ya, bn.d.mean, bn.d.istd, bn.d.sc, bn.d.sh, part)
        o.check()
        return [part]

    (part,) = _twice(run, keep=True)
    t1, t2 = ref_terms(gr.view(P, C), y.view(P, C), bn.r)
    block = (torch.arange(P) // tpix)[:, None].expand(P, C).contiguous()
    slots = NT // U
    db, dg = check_bn_part("bn_bwd_reduce", part.cpu(), tiles, block, t1, t2, cdiv(tpix, slots) + slots)
    zero = torch.zeros(C, device=DEV)
    for dbeta, dgamma in ((db, dg), (zero, zero)):
        def run():
            s = Slots(dt)
            oa = s.out(N, H, W, C)
            ops.bn_bwd_apply(s.put(gr), s.put(y), bn.d.mean, bn.d.istd, bn.d.sc, bn.d.sh, dbeta, dgamma, oa)
            s.check()
            return [val(oa)]

        (gy,) = _twice(run)
        _check_apply("bn_bwd_apply", gy, gr, y, bn.r, dbeta.cpu(), dgamma.cpu(), P, dt)
    # dbeta = dgamma = 0: gy = scale g' (one product), nonzero exactly where the mask holds -- no tolerance
    assert torch.equal(gy != 0, ref_mask(y, bn.r))
    pre = fma32(y, bn.r.sc, bn.r.sh)[..., 0].reshape(-1)  # channel 0: exactly 0 and one ulp to either side
    assert int((pre == 0).sum()) == (P + 1) // 3 and int((pre > 0).sum()) == P // 3


@dts
def test_bn_bwd_too_many_units(dt):
    ops = _ops()
    C = 257 * EOF[dt]
    t = torch.zeros(1, 1, 2, C, dtype=dt, device=DEV)
    v = torch.zeros(C, device=DEV)
    with pytest.raises(_err()):
        ops.bn_bwd_reduce(ops.act(t), ops.act(t), v, v, v, v, torch.zeros(2 * C, device=DEV))
    with pytest.raises(_err()):
        ops.bn_bwd_apply(ops.act(t), ops.act(t), v, v, v, v, v, v, ops.act(torch.zeros_like(t)))
    torch.cuda.synchronize()


# ---- D2. dec1's 1x1 backward --------------------------------------------------------------------------------
C1X_PIX = 1024
C1X_P = [1, 31, 32, 33, 64, 65, 1023, 1024, 1025, 2049]
C1X_NADD = C1X_PIX // 32 + 3 + 3  # pixels of a slot in a block + the 3 slot butterflies + the 4 waves


@dts
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("C", [8, 64, 72, 128])
def test_conv1x1_bwd(C, K, dt):
    """gact = W^T gz (rounded to T), per-block partials of gW [K][C] and gb [K] over the block's 1024 pixels
    (n_add = 1024 / 32 pixels of a lane's slot + 3 butterflies over the 8 slots of a wave + 3 adds over the waves;
    + 2 in the BN sums for the two roundings of xhat), the fused BN-backward partials over the stored gact, with and
    without storing it, and the recomputing apply."""
    ops = _ops()
    for P in C1X_P:
        bn, y, w, _ = _c1x_inputs(P, C, K, dt, 700 + P + C + K)
        gz = torch.randn(P, K, generator=torch.Generator().manual_seed(P + K)).float()
        tiles, stride = cdiv(P, C1X_PIX), K * C + K

        def run(mode):
            s, o = Slots(dt), Outs()
            ya = s.put(y)
            assert ops.conv1x1_bwd_tiles(ya) == tiles
            ga = s.out(1, 1, P, C) if mode != "none" else None
            part = o.new(tiles * stride)
            outs = [part]
            if mode == "plain":
                ops.conv1x1_bwd(ya, bn.d.sc, bn.d.sh, w.to(DEV), K, gz.to(DEV), ga, part)
            else:
                bpart = o.new(tiles * 2 * C)
                ops.conv1x1_bwd_bnr(ya, bn.d.sc, bn.d.sh, w.to(DEV), K, gz.to(DEV), ga, part, bn.d.mean, bn.d.istd,
                                    bpart)
                outs.append(bpart)
            s.check()
            o.check()
            return outs + ([val(ga)] if ga is not None else [])

        part0, gact0 = _twice(lambda: run("plain"))
        part1, bpart1, gact1 = _twice(lambda: run("bnr"))
        part2, bpart2 = _twice(lambda: run("none"))
        assert torch.equal(gact0, gact1) and torch.equal(part0, part1) and torch.equal(part0, part2)
        assert torch.equal(bpart1, bpart2)
        y2, wd, gzd = y.view(P, C), w.double(), gz.double()
        gate_el("gact", gact0, gzd @ wd, dt, S=gzd.abs() @ wd.abs())
        a = ref_act32(y2, bn.r)
        terms = torch.cat([(gzd[:, k:k + 1] * a) for k in range(K)] + [gzd], 1)  # [P][K C + K]
        block = (torch.arange(P) // C1X_PIX)[:, None]
        ref, mag = rows_ref(block.expand(P, stride).contiguous(), terms, tiles)
        gate_sum("gW | gb partials", part0.view(tiles, stride), ref, mag, C1X_NADD)
        gst = gact0.double().view(P, C)  # the gradient as stored
        t1, t2 = ref_terms(gst, y2, bn.r)
        db, dg = check_bn_part("conv1x1_bwd_bnr", bpart1.to(DEV), tiles, block.expand(P, C).contiguous().to(DEV),
                               t1.to(DEV), t2.to(DEV), C1X_NADD + 2)

        def run_apply(recompute):
            s = Slots(dt)
            ya, oa = s.put(y), s.out(1, 1, P, C)
            if recompute:
                ops.bn_bwd_apply_1x1(ya, w.to(DEV), K, gz.to(DEV), bn.d.mean, bn.d.istd, bn.d.sc, bn.d.sh, db, dg, oa)
            else:
                ops.bn_bwd_apply(s.put(gact0.view(1, 1, P, C)), ya, bn.d.mean, bn.d.istd, bn.d.sc, bn.d.sh, db, dg, oa)
            s.check()
            return [val(oa)]

        (gy,) = _twice(lambda: run_apply(True))
        (gy_plain,) = _twice(lambda: run_apply(False))
        assert torch.equal(gy, gy_plain)
        _check_apply("bn_bwd_apply_1x1", gy, gst.view(1, 1, P, C), y, bn.r, db.cpu(), dg.cpu(), P, dt)


# ---- D3. max-pool adjoints ----------------------------------------------------------------------------------
POOL_CASES = [(s, u) for s in [(1, 2, 2), (2, 2, 6), (2, 10, 14)] for u in (1, 3, 12, 16)] + [((1, 2, 2), 96)]


def _pool_y(shape, C, dt, g, dev="cpu"):
    """y with all-negative windows (every 5th), windows of four equal values (every 7th) and windows of neighbouring
    values in dt (every 11th), so the stored activations tie."""
    y = rand_y(shape + (C,), dt, g).to(dev)
    y4 = win(y)
    nw = y4.shape[0] * y4.shape[1] * y4.shape[2]
    f = y4.reshape(nw, 4, C)
    idx = torch.arange(nw, device=dev)
    f[idx % 7 == 3] = f[idx % 7 == 3][:, 3:4, :].expand(-1, 4, -1).clone()
    nb = f[idx % 11 == 5][:, 0:1, :]
    step = torch.tensor([0.0, 1.0, 0.0, 1.0], dtype=torch.float64, device=dev)[None, :, None]
    f[idx % 11 == 5] = rt(nb * (1.0 + step * (2.0 ** -7 if dt == BF16 else 2.0 ** -23)), dt)
    return unwin(f.reshape(y4.shape)), idx


def _pool_inputs(shape, U, dt, seed, dev="cpu"):
    N, H, W = shape
    C = U * EOF[dt]
    g = torch.Generator().manual_seed(seed)
    bn = Bn(C, g)
    y, idx = _pool_y(shape, C, dt, g, dev)
    r = bn.on(dev)
    # every 5th window: all four pre-activations negative (y moved against the sign of scale)
    y4 = win(y).reshape(-1, 4, C)
    neg = -(r.sh.abs() + 1.0 + y4[idx % 5 == 1].abs()) / r.sc
    y4[idx % 5 == 1] = rt(neg, dt)
    y = unwin(y4.reshape(N, H // 2, W // 2, 4, C))
    gp = rand_t((N, H // 2, W // 2, C), dt, g).to(dev)
    gs = rand_t((N, H, W, C), dt, g).to(dev)
    return bn, r, y, gp, gs


def _pool_block(shape, U, E, grid, bs, dev="cpu"):
    """The partial row of every (pixel, channel): thread id = window * U + unit, block = (id mod (grid bs)) // bs."""
    N, H, W = shape
    n, yy, xx = torch.meshgrid(torch.arange(N, device=dev), torch.arange(H, device=dev), torch.arange(W, device=dev),
                               indexing="ij")
    wnd = ((n * (H // 2) + yy // 2) * (W // 2) + xx // 2).reshape(-1, 1)
    tid = wnd * U + torch.arange(U, device=dev)[None, :]
    return ((tid % (grid * bs)) // bs).repeat_interleave(E, dim=1)


def _run_pool_case(shape, U, dt, seed, dev="cpu", nan=False, modes=(True, False)):
    ops = _ops()
    N, H, W = shape
    E = EOF[dt]
    C, P = U * E, N * H * W
    bn, r, y, gp, gs_full = _pool_inputs(shape, U, dt, seed, dev)
    stored = rt(ref_act32(y, r), dt)
    assert int((win(stored).amax(3) == 0).sum()) > 0 or P < 8  # all-zero windows are there
    bs = bnr_block(U)
    threads = P // 4 * U
    rows = min(cdiv(threads, bs), 2048)
    iters = cdiv(threads, rows * bs)
    n_add = 4 * iters + bs // U + 2  # 4 pixels per window and step; the block sums bs / U threads serially; xhat
    block = _pool_block(shape, U, E, rows, bs, dev)
    for with_skip in modes:
        gs = gs_full if with_skip else None
        act_in = stored.clone()
        if nan:  # plain adjoint only: a NaN in tap 2 of window 0 (the reductions would carry the NaN by contract)
            act_in[0, 1, 0, :] = float("nan")

        def run(mode):
            s, o = Slots(dt), Outs()
            aa, gpa, ya = s.put(act_in if mode == "plain" else stored), s.put(gp), s.put(y)
            gsa = s.put(gs) if gs is not None else None
            if mode == "plain":
                oa = s.out(N, H, W, C)
                ops.pool_bwd_add(aa, gpa, gsa, oa)
                res = [val(oa)]
            elif mode in ("bnr", "bnr_none"):
                oa = s.out(N, H, W, C) if mode == "bnr" else None
                assert ops.pool_bwd_add_bnr_rows(oa if oa is not None else ya) == rows
                part = o.new(rows * 2 * C)
                ops.pool_bwd_add_bnr(aa, gpa, gsa, oa, ya, bn.d.mean, bn.d.istd, bn.d.sc, bn.d.sh, part)
                res = [part] + ([val(oa)] if oa is not None else [])
            s.check()
            o.check()
            return res

        (gout_plain,) = _twice(lambda: run("plain"), keep=True)
        ref_g, S = ref_pool_bwd(act_in, gp, gs, dt)
        fin = torch.isfinite(ref_g)
        assert torch.equal(torch.isfinite(gout_plain.to(dev)), fin)
        assert _same(gout_plain.to(dev).double(), ref_g)  # sums of two stored values, rounded once: exact
        if nan:
            _, arg = ref_argmax(win(act_in))
            assert bool((arg[0, 0, 0] == 2).all())
            continue
        part, gout = _twice(lambda: run("bnr"), keep=True)
        (part_none,) = _twice(lambda: run("bnr_none"), keep=True)
        assert torch.equal(gout, gout_plain) and torch.equal(part, part_none)
        gate_el("gout", gout, ref_g, dt, S=S)
        t1, t2 = ref_terms(ref_g.view(P, C), y.view(P, C), r)
        db, dg = check_bn_part("pool_bwd_add_bnr", part.to(dev), rows, block, t1, t2, n_add)
        db, dg = db.to(DEV), dg.to(DEV)

        def run_apply(recompute):
            s = Slots(dt)
            ya, oa = s.put(y), s.out(N, H, W, C)
            gsa = s.put(gs) if gs is not None else None
            if recompute:
                ops.bn_bwd_apply_pool(s.put(gp), gsa, ya, bn.d.mean, bn.d.istd, bn.d.sc, bn.d.sh, db, dg, oa)
            else:
                ops.bn_bwd_apply(s.put(gout), ya, bn.d.mean, bn.d.istd, bn.d.sc, bn.d.sh, db, dg, oa)
            s.check()
            return [val(oa)]

        (gy,) = _twice(lambda: run_apply(True), keep=True)
        (gy_plain,) = _twice(lambda: run_apply(False), keep=True)
        assert torch.equal(gy, gy_plain)
        ref, S = ref_apply(ref_g, y, r, db.double().to(dev), dg.double().to(dev), float(P))
        gate_el("bn_bwd_apply_pool", gy.to(dev), ref, dt, S=S)


@dts
@pytest.mark.parametrize("shape,U", POOL_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"U{v}")
def test_pool_bwd(shape, U, dt):
    """pool_bwd_add, pool_bwd_add_bnr (storing gout and not) and bn_bwd_apply_pool, with and without gskip.  A thread
    of the fused reduction adds the 4 pixels of each of its windows, the block then sums its bs / U threads of equal
    unit serially: n_add = 4 ceil(windows U / (rows bs)) + bs / U (+ 2: the roundings of xhat)."""
    _run_pool_case(shape, U, dt, 800 + U + shape[1] * shape[2])


@dts
def test_pool_bwd_nan_window(dt):
    """A NaN in the saved activation wins its window (as max_pool2d's argmax) and only there."""
    _run_pool_case((2, 2, 6), 3, dt, 801, nan=True)


@pytest.mark.parametrize("shape", [(1, 128, 130), (1, 256, 258)], ids=["reduce-cap-2048", "apply-cap-8192"])
def test_pool_bwd_grid_wrap(shape):
    """U = 96 (C = 768 bf16, 192-thread blocks): 64 x 65 = 4160 windows x 96 units exceed the reduction's 2048 blocks,
    128 x 129 = 16512 windows the apply's 8192.  Reference in fp64 on the device."""
    _run_pool_case(shape, 96, BF16, 802, dev=DEV, modes=(True,))


@dts
def test_pool_up_bwd_unfusable_units(dt):
    """U = 5: neither 256 nor 192 threads cover whole units -- the row counts are 0 and the fused kernels refuse."""
    ops = _ops()
    C = 5 * EOF[dt]
    y = torch.zeros(1, 2, 2, C, dtype=dt, device=DEV)
    lo = torch.zeros(1, 1, 1, C, dtype=dt, device=DEV)
    v = torch.zeros(C, device=DEV)
    part = torch.zeros(64 * C, device=DEV)
    assert ops.pool_bwd_add_bnr_rows(ops.act(y)) == 0 and ops.upsample_bwd_bnr_rows(ops.act(lo)) == 0
    with pytest.raises(_err()):
        ops.pool_bwd_add_bnr(ops.act(y), ops.act(lo), None, ops.act(torch.zeros_like(y)), ops.act(y), v, v, v, v, part)
    with pytest.raises(_err()):
        ops.bn_bwd_apply_pool(ops.act(lo), None, ops.act(y), v, v, v, v, v, v, ops.act(torch.zeros_like(y)))
    with pytest.raises(_err()):
        ops.upsample_bwd_bnr(ops.act(y), ops.act(torch.zeros_like(lo)), ops.act(lo), v, v, v, v, part)
    torch.cuda.synchronize()


def _view_refusals(ops, dt, odd):
    """The calls of the older launchers with one view that disagrees with the reference view y of shape (1, 2, 2, C),
    C = two channel units: odd(kind, base shape) builds the disagreeing view ('n': one more sample, 'h' / 'w': one more
    row / column, 'f32': fp32 storage).  The odd view is always the larger allocation and the launchers take n, h, w
    and the element type from the reference view, so a call that were accepted would stay inside every buffer."""
    C = 2 * EOF[dt]
    z = lambda *s: ops.act(torch.zeros(*s, C, dtype=dt, device=DEV))
    y, half = z(1, 2, 2), z(1, 1, 1)
    full, lo = (1, 2, 2), (1, 1, 1)
    v, part = torch.zeros(C, device=DEV), torch.zeros(64 * C, device=DEV)
    w, gz = torch.zeros(1, C, device=DEV), torch.zeros(4, 1, device=DEV)
    calls = {}

    def add(name, kinds, base, fn):
        for k in kinds:
            if odd(k, base) is not None:
                calls[f"{name}-{k}"] = functools.partial(fn, odd(k, base))

    add("bnrelu_pool.pooled", ["f32"], lo, lambda o: ops.bnrelu_pool(y, v, v, None, o))
    add("bnrelu_pool.act", ["n", "f32"], full, lambda o: ops.bnrelu_pool(y, v, v, o, half))
    add("bn_bwd_apply.g", ["n"], full, lambda o: ops.bn_bwd_apply(o, y, v, v, v, v, v, v, z(*full)))
    add("bn_bwd_apply.gy", ["h", "w"], full, lambda o: ops.bn_bwd_apply(z(*full), y, v, v, v, v, v, v, o))
    for name, run in [("pool_bwd_add", lambda gp, gs, go: ops.pool_bwd_add(y, gp, gs, go)),
                      ("pool_bwd_add_bnr", lambda gp, gs, go: ops.pool_bwd_add_bnr(y, gp, gs, go, y, v, v, v, v, part))]:
        add(name + ".gpool", ["n", "f32"], lo, lambda o, run=run: run(o, z(*full), z(*full)))
        add(name + ".gskip", ["n", "h", "f32"], full, lambda o, run=run: run(half, o, z(*full)))
        add(name + ".gout", ["n"], full, lambda o, run=run: run(half, z(*full), o))
    reduce_only = lambda gp, gs: ops.pool_bwd_add_bnr(y, gp, gs, None, y, v, v, v, v, part)
    add("pool_bwd_add_bnr.reduce.gpool", ["n", "f32"], lo, lambda o: reduce_only(o, z(*full)))
    add("pool_bwd_add_bnr.reduce.gskip", ["n", "h", "f32"], full, lambda o: reduce_only(half, o))
    add("conv1x1_bwd.gact", ["n", "h"], full, lambda o: ops.conv1x1_bwd(y, v, v, w, 1, gz, o, part))
    add("conv1x1_bwd_bnr.gact", ["n", "h"], full, lambda o: ops.conv1x1_bwd_bnr(y, v, v, w, 1, gz, o, part, v, v, part))
    return calls


@dts
def test_views_must_agree_in_shape(dt):
    """Every view of a call agrees with the reference view in n, h and w (up to the op's factor 2): one more sample,
    row or column in any other view is EUNET_ERR_INVALID before anything is launched."""
    ops = _ops()
    C = 2 * EOF[dt]
    grow = {"n": (1, 0, 0), "h": (0, 1, 0), "w": (0, 0, 1)}

    def odd(kind, base):
        if kind not in grow:
            return None
        return ops.act(torch.zeros(*[b + d for b, d in zip(base, grow[kind])], C, dtype=dt, device=DEV))

    calls = _view_refusals(ops, dt, odd)
    assert len(calls) == 19
    for name, call in calls.items():
        with pytest.raises(_err()):
            call()
            pytest.fail(f"{name}: accepted")
    torch.cuda.synchronize()


def test_views_must_agree_in_dtype():
    """The same for the element type: an fp32 view among bf16 ones (the element type is the reference view's, so the
    fp32 tensor is the larger allocation)."""
    ops = _ops()
    C = 2 * EOF[BF16]

    def odd(kind, base):
        return ops.act(torch.zeros(*base, C, dtype=F32, device=DEV)) if kind == "f32" else None

    calls = _view_refusals(ops, BF16, odd)
    assert len(calls) == 8
    for name, call in calls.items():
        with pytest.raises(_err()):
            call()
            pytest.fail(f"{name}: accepted")
    torch.cuda.synchronize()


# ---- D4. upsample adjoints ----------------------------------------------------------------------------------
UPB_SHAPES =[(1, 1, 1), (2, 1, 5), (2, 5, 1), (1, 8, 2), (1, 9, 7), (2, 17, 3)]
UP_R = 8


@dts
@pytest.mark.parametrize("U", [1, 3, 12])
@pytest.mark.parametrize("shape", UPB_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upsample_bwd(shape, U, dt):
    """upsample_bwd and upsample_bwd_bnr against the fp64 adjoint of F.interpolate.  The fused reduction's thread adds
    the 2 columns x 8 rows of its cell, the block then bs / U threads: n_add = 16 ceil(cells U / (rows bs)) + bs / U
    (+ 2: xhat)."""
    ops = _ops()
    N, h, w = shape
    E = EOF[dt]
    C, P = U * E, N * h * w
    g = torch.Generator().manual_seed(900 + 7 * P + U)
    bn = Bn(C, g)
    y = rand_y(shape + (C,), dt, g)
    gh = rand_t((N, 2 * h, 2 * w, C), dt, g)
    hr, wb = cdiv(h, UP_R), cdiv(w, 2)
    bs = bnr_block(U)
    threads = N * hr * wb * U
    rows = min(cdiv(threads, bs), 8192)
    n_add = 2 * UP_R * cdiv(threads, rows * bs) + bs // U + 2

    def run(fused):
        s, o = Slots(dt), Outs()
        ga, oa = s.put(gh), s.out(N, h, w, C)
        res = [val(oa)]
        if fused:
            assert ops.upsample_bwd_bnr_rows(oa) == rows
            part = o.new(rows * 2 * C)
            ops.upsample_bwd_bnr(ga, oa, s.put(y), bn.d.mean, bn.d.istd, bn.d.sc, bn.d.sh, part)
            res.append(part)
        else:
            ops.upsample_bwd(ga, oa)
        s.check()
        o.check()
        return res

    (glo,) = _twice(lambda: run(False))
    glo_f, part = _twice(lambda: run(True))
    assert torch.equal(glo, glo_f)
    gate_el("glo", glo, ref_up_adj(gh), dt, S=ref_up_adj(gh.abs()))
    t1, t2 = ref_terms(glo.double().view(P, C), y.view(P, C), bn.r)  # over the gradient as stored
    n, yy, xx = torch.meshgrid(torch.arange(N), torch.arange(h), torch.arange(w), indexing="ij")
    cell = ((n * hr + yy // UP_R) * wb + xx // 2).reshape(-1, 1)
    tid = cell * U + torch.arange(U)[None, :]
    block = ((tid % (rows * bs)) // bs).repeat_interleave(E, dim=1)
    check_bn_part("upsample_bwd_bnr", part.to(DEV), rows, block.to(DEV), t1.to(DEV), t2.to(DEV), n_add)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", UPB_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upsample_bwd_small_k(shape, K):
    """The head's fp32 K-channel kernels (K = 2 has its own): at most 16 fmas per output, n_add = 16."""
    ops = _ops()
    N, h, w = shape
    gh = torch.randn(N, 2 * h, 2 * w, K, generator=torch.Generator().manual_seed(950 + K + h * w), dtype=torch.float64)
    gh = gh.float().double()

    def run():
        o = Outs()
        out = o.new((N, h, w, K))
        ops.upsample_bwd(ops.act(gh.float().to(DEV)), ops.act(out))
        o.check()
        return [out]

    (glo,) = _twice(run)
    ref = ref_up_adj(gh)
    gate_el("glo", glo, ref, F32)
    gate_sum("glo per element", glo, ref, ref_up_adj(gh.abs()), 16 + 1)


# ---- E. colsum ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 64, 65, 4097, 16384, 16385, 20000])
def test_colsum(rows):
    """Rows alternate +-1e6 plus O(1) values: an fp32 accumulation loses 0.06 per addition (errors of about
    0.06 sqrt(rows) against a gate of 2^-23 |sum| + 2^-50 sum|terms|, which is 1e-7 for an even row count)."""
    ops = _ops()
    for cols in (1, 63, 64, 65, 130):
        g = torch.Generator().manual_seed(rows * 131 + cols)
        part = (1e6 * (1.0 - 2.0 * (torch.arange(rows) % 2).double())[:, None] +
                torch.randn(rows, cols, generator=g, dtype=torch.float64)).float()
        pd = part.to(DEV)
        ref, mag = part.double().sum(0), part.double().abs().sum(0)

        def run(split):
            o = Outs()
            if split is None:
                out = o.new(cols)
                ops.colsum(pd, rows, cols, out)
                res = [out]
            else:
                lo, hi = o.new(split), o.new(cols - split)
                ops.colsum(pd, rows, cols, lo, split=split, out_hi=hi)
                res = [lo, hi]
            o.check()
            return res

        (out,) = _twice(lambda: run(None))
        gate_colsum(f"colsum {rows}x{cols}", out, ref, mag)
        for split in sorted({s for s in (1, 64, 65, cols - 1) if 0 < s < cols}):
            lo, hi = _twice(lambda: run(split))
            assert torch.equal(torch.cat([lo, hi]), out), split
        for split in (0, cols):
            with pytest.raises(_err()):
                ops.colsum(pd, rows, cols, torch.zeros(cols, device=DEV), split=split, out_hi=torch.zeros(cols, device=DEV))
    torch.cuda.synchronize()


# ---- F. composed --------------------------------------------------------------------------------------------
def _composed_inputs(dt):
    """y whose every 2x2 window has one clear winner per channel (a margin no rounding closes), batch statistics
    taken from that y."""
    N, H, W, C = 2, 10, 14, 24
    g = torch.Generator().manual_seed(1234)
    gam = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0) * (0.5 + torch.rand(C, generator=g))
    bet = 0.1 * torch.randn(C, generator=g)
    y4 = (0.3 * torch.randn(N, H // 2, W // 2, 4, C, generator=g, dtype=torch.float64)).clamp(-1, 1)
    tap = torch.randint(0, 4, (N, H // 2, W // 2, 1, C), generator=g)
    boost = torch.sign(gam.double()) * (3.0 + torch.rand(N, H // 2, W // 2, 1, C, generator=g, dtype=torch.float64))
    y4.scatter_(3, tap, boost)
    y = rt(unwin(y4), dt)
    P = N * H * W
    mean = y.view(P, C).mean(0).float()
    istd = (1.0 / torch.sqrt(y.view(P, C).var(0, unbiased=False) + BN_EPS)).float()
    bn = Bn(C, g, boundary=False)
    bn.mean, bn.istd, bn.gam, bn.bet = mean, istd, gam.float(), bet.float()
    bn.sc = (bn.gam.double() * istd.double()).float()
    bn.sh = (bn.bet.double() - mean.double() * bn.sc.double()).float()
    bn._mk()
    return N, H, W, C, g, bn, y


def _gate_composed(name, gy, ref, S, dt):
    err = (gy.double() - ref).abs()
    print(f"{name}: max err {float(err.max()):.3e}, max|ref| {float(ref.abs().max()):.3e}")
    if dt == F32:
        assert float(err.max()) <= 1e-4 * float(ref.abs().max()), name
    else:
        bound = 2.0 ** -8 * ref.abs() + (2.0 ** -9 + 1e-5) * S
        assert bool((err <= bound).all()), (name, float((err / bound).max()))


def _apply_mag(g, y, bn, P):
    """S' of the composed gate: the apply's terms with the reduced sums taken over absolute values."""
    r = bn.r
    gp = torch.where(ref_mask(y, r), g, torch.zeros_like(g)).abs()
    xh = ((y - r.mean) * r.istd).abs()
    sums = gp.view(P, -1).sum(0) / P, (gp * xh).view(P, -1).sum(0) / P
    return r.sc.abs() * (gp + sums[0] + xh * sums[1])


@dts
def test_composed_double_conv_backward(dt):
    """The two BN-backward chains of UNetEngine that keep no gradient in memory, against fp64 autograd of
    relu(batch_norm(y)) -> max_pool2d + skip, respectively -> 1x1 conv, evaluated on the same rounded y:
      pool_bwd_add_bnr(gout=None) -> colsum(split) -> bn_bwd_apply_pool
      conv1x1_bwd_bnr(gact=None)  -> colsum(split) -> bn_bwd_apply_1x1   (and gW, gb from its partials)."""
    ops = _ops()
    N, H, W, C, g, bn, y = _composed_inputs(dt)
    P, K = N * H * W, 3
    stored = rt(ref_act32(y, bn.r), dt)
    top2 = win(stored).topk(2, dim=3).values
    tied = float((top2[..., 0, :] == top2[..., 1, :]).double().mean())
    assert tied == 0.0, tied  # checked on the host, before anything runs
    gp, gs = rand_t((N, H // 2, W // 2, C), dt, g), rand_t((N, H, W, C), dt, g)
    w = (0.3 * torch.randn(K, C, generator=g)).float()
    gz = torch.randn(P, K, generator=g).float()

    def autograd(head):
        yl = nchw(y).clone().requires_grad_(True)
        wl = w.double().clone().requires_grad_(True)
        bl = torch.zeros(K, dtype=torch.float64, requires_grad=True)
        a = F.relu(F.batch_norm(yl, None, None, bn.r.gam, bn.r.bet, True, 0.0, BN_EPS))
        if head == "pool":
            (F.max_pool2d(a, 2) * nchw(gp)).sum().add((a * nchw(gs)).sum()).backward()
        else:
            (F.conv2d(a, wl[:, :, None, None], bl) * nchw(gz.double().view(N, H, W, K))).sum().backward()
        return nhwc(yl.grad), wl.grad, bl.grad

    def chain(head):
        s, o = Slots(dt), Outs()
        ya, oa = s.put(y), s.out(N, H, W, C)
        db, dg = o.new(C), o.new(C)
        res = [val(oa)]
        if head == "pool":
            rows = ops.pool_bwd_add_bnr_rows(ya)
            part = o.new(rows * 2 * C)
            gpa, gsa = s.put(gp), s.put(gs)
            ops.pool_bwd_add_bnr(s.put(stored), gpa, gsa, None, ya, bn.d.mean, bn.d.istd, bn.d.sc, bn.d.sh, part)
            ops.colsum(part, rows, 2 * C, db, split=C, out_hi=dg)
            ops.bn_bwd_apply_pool(gpa, gsa, ya, bn.d.mean, bn.d.istd, bn.d.sc, bn.d.sh, db, dg, oa)
        else:
            tiles = ops.conv1x1_bwd_tiles(ya)
            part, bpart = o.new(tiles * (K * C + K)), o.new(tiles * 2 * C)
            gw, gb = o.new(K * C), o.new(K)
            ops.conv1x1_bwd_bnr(ya, bn.d.sc, bn.d.sh, w.to(DEV), K, gz.to(DEV), None, part, bn.d.mean, bn.d.istd, bpart)
            ops.colsum(bpart, tiles, 2 * C, db, split=C, out_hi=dg)
            ops.colsum(part, tiles, K * C + K, gw, split=K * C, out_hi=gb)
            ops.bn_bwd_apply_1x1(ya, w.to(DEV), K, gz.to(DEV), bn.d.mean, bn.d.istd, bn.d.sc, bn.d.sh, db, dg, oa)
            res += [gw, gb]
        s.check()
        o.check()
        return res

    (gy,) = _twice(lambda: chain("pool"))
    ref, _, _ = autograd("pool")
    gout, _ = ref_pool_bwd(stored, gp, gs, F32)  # unrounded: what autograd sees
    _gate_composed("pool chain gy", gy, ref, _apply_mag(gout, y, bn, P), dt)
    gy, gw, gb = _twice(lambda: chain("1x1"))
    ref, rw, rb = autograd("1x1")
    _gate_composed("1x1 chain gy", gy, ref, _apply_mag(gz.double().view(N, H, W, K) @ w.double(), y, bn, P), dt)
    a = ref_act32(y.view(P, C), bn.r)
    gate_sum("gW", gw, rw.reshape(-1), (gz.double().abs().t() @ a).reshape(-1), C1X_NADD)
    gate_sum("gb", gb, rb, gz.double().abs().sum(0), C1X_NADD)
