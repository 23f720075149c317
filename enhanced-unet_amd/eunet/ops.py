"""Thin torch-tensor wrappers over the C-ABI (one function per entry point).

Tensors are device memory only (torch is the allocator); every call is
enqueued on torch's current HIP stream.  Activations are NHWC tensors
[N, H, W, Ctot]; a channel slice is expressed by (coff, c).
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib, kprof
from ._lib import Act, call, c_int, c_size_t

DTYPES = {torch.float32: _lib.EUNET_F32, torch.bfloat16: _lib.EUNET_BF16}

# ---- torch.ops.eunet.* ---------------------------------------------------------------------------
# The network's device ops are registered with PyTorch's dispatcher (library "eunet", CUDA key), so they
# appear as eunet::<op> in torch.profiler traces and go through dispatcher hooks.  A
# decorated function keeps its Python signature: its arguments are flattened into the op schema
# (an Act becomes (tensor, coff, c)), the dispatcher calls the CUDA impl, which rebuilds the Acts and
# runs the original body (one C-ABI call).  Cost ~2 us of dispatcher per call (USE_DISPATCHER = False
# calls the bodies directly; tools/ab_attr.py ops.USE_DISPATCHER=0).
USE_DISPATCHER = True
_LIB = torch.library.Library("eunet", "DEF")
DISPATCHED: dict = {}


def _dispatched(kinds: str, returns_tensor: bool = False, names=None):
    """kinds: one token per parameter -- A (Act), T (tensor), i (int), I (list of int), f (float), b (bool),
    d (torch dtype), s (str); A! / T! mark the arguments the op writes, a trailing ? an optional (None-able) argument.
    names: the parameter names of a function that takes *args (no defaults); otherwise read from its signature."""
    import inspect
    import string

    ks = kinds.split()

    def deco(fn):
        params = [] if names else list(inspect.signature(fn).parameters.values())
        argnames = list(names or (p.name for p in params))
        if len(argnames) != len(ks):
            raise _lib.EunetError(f"_dispatched({fn.__name__}): {len(argnames)} parameters, {len(ks)} kinds")
        letters = iter(string.ascii_lowercase)
        parts = []
        for nm, k in zip(argnames, ks):
            q = "?" if k.endswith("?") else ""
            base = k.rstrip("?")
            w = base.endswith("!")
            base = base.rstrip("!")
            if base in ("A", "T"):
                ty = f"Tensor({next(letters)}!){q}" if w else f"Tensor{q}"
                parts += [f"{ty} {nm}"] + ([f"int {nm}_coff", f"int {nm}_c"] if base == "A" else [])
            else:
                ty = {"i": "int", "I": "int[]", "f": "float", "b": "bool", "d": "ScalarType", "s": "str"}[base]
                parts.append(f"{ty}{q} {nm}")
        _LIB.define(f"{fn.__name__}({', '.join(parts)}) -> {'Tensor' if returns_tensor else '()'}")

        def impl(*flat):
            args, j = [], 0
            for k in ks:
                if k.startswith("A"):
                    t, coff, c = flat[j:j + 3]
                    j += 3
                    args.append(None if t is None else act(t, coff, c))
                else:
                    args.append(flat[j])
                    j += 1
            return fn(*args)

        _LIB.impl(fn.__name__, impl, "CUDA")
        _LIB.impl(fn.__name__, impl, "CPU")  # raises EunetError in _ptr / act: no CPU fallback
        op = getattr(torch.ops.eunet, fn.__name__)

        defaults = [p.default for p in params]
        index = {nm: i for i, nm in enumerate(argnames)}
        isact = [k.startswith("A") for k in ks]

        def wrapper(*args, **kwargs):
            if not USE_DISPATCHER:
                return fn(*args, **kwargs)
            vals = list(args) + defaults[len(args):]
            for nm, v in kwargs.items():
                vals[index[nm]] = v
            flat = []
            for a, v in zip(isact, vals):
                if not a:
                    flat.append(v)
                elif v is None:
                    flat += (None, 0, 0)
                else:
                    flat += (v._keep, v.coff, v.c)
            return op(*flat)

        wrapper.__name__, wrapper.__doc__, wrapper.__wrapped__ = fn.__name__, fn.__doc__, fn
        DISPATCHED[fn.__name__] = op
        return wrapper

    return deco


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def stream_wait(frm: torch.cuda.Stream, to: torch.cuda.Stream):
    """`to` waits for the work enqueued on `frm` so far: eunet_stream_wait (a device-scope event release,
    where torch's Stream.wait_stream records a system-scope one)."""
    call("eunet_stream_wait", ctypes.c_void_p(frm.cuda_stream), ctypes.c_void_p(to.cuda_stream))


_guards = {}  # device index -> the fp64 [1] tensor eunet_set_update_guard points at (kept alive here)


def set_update_guard(device, guard):
    """eunet_set_update_guard: while guard (a device fp64 [1] tensor, or None) is nonzero, BN running
    statistics and the native clip + AdamW leave the persistent state untouched."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if guard is not None and (guard.dtype != torch.float64 or guard.device.type != "cuda" or guard.device.index != idx):
        raise ValueError("update guard: an fp64 tensor on the guarded device")
    if _guards.get(idx) is guard:
        return
    call("eunet_set_update_guard", idx, None if guard is None else ctypes.c_void_p(guard.data_ptr()))
    if guard is None:
        _guards.pop(idx, None)
    else:
        _guards[idx] = guard


def update_guard(device):
    """The tensor eunet_set_update_guard currently points at for device (None: no guard)."""
    dev = torch.device(device)
    return _guards.get(dev.index if dev.index is not None else torch.cuda.current_device())


def _ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.EunetError("eunet ops need device tensors (no CPU fallback)")
    return ctypes.c_void_p(t.data_ptr())


def act(t: torch.Tensor, coff: int = 0, c: int | None = None) -> Act:
    """NHWC view of a contiguous [N,H,W,Ctot] tensor, channels [coff, coff+c)."""
    if t.dim() != 4 or not t.is_contiguous():
        raise _lib.EunetError(f"act(): need a contiguous NHWC tensor, got {tuple(t.shape)}")
    if not t.is_cuda:
        raise _lib.EunetError("act(): tensor must live on the GPU")
    n, h, w, ct = t.shape
    a = Act(t.data_ptr(), n, h, w, ct - coff if c is None else c, ct, coff, DTYPES[t.dtype])
    a._keep = t  # the view keeps its tensor (and device memory) alive
    return a


def _ref(a):
    return None if a is None else ctypes.byref(a)


@_dispatched("T T!")
def nchw_to_nhwc(x: torch.Tensor, out: torch.Tensor):
    call("eunet_nchw_to_nhwc", _ptr(x), ctypes.byref(act(out)), _stream())


def conv3x3_packed_bytes(cout, cin, dtype):
    b = c_size_t()
    call("eunet_conv3x3_packed_bytes", cout, cin, DTYPES[dtype], ctypes.byref(b))
    return b.value


@_dispatched("T d b", returns_tensor=True)
def conv3x3_pack(w: torch.Tensor, dtype, flip: bool) -> torch.Tensor:
    cout, cin = w.shape[0], w.shape[1]
    nbytes = conv3x3_packed_bytes(cin if flip else cout, cout if flip else cin, dtype)
    wp = torch.empty(nbytes // (2 if dtype == torch.bfloat16 else 4), dtype=dtype, device=w.device)
    call("eunet_conv3x3_pack", _ptr(w.contiguous()), cout, cin, int(flip), _ptr(wp), DTYPES[dtype], _stream())
    return wp


def conv3x3_pack_many(items, dtype):
    """[(w, flip), ...] -> packed tensors, one launch per PACK_MAX tensors (eunet_conv3x3_pack_many)."""
    out = []
    for lo in range(0, len(items), _lib.PACK_MAX):
        chunk = items[lo:lo + _lib.PACK_MAX]
        descs = (_lib.PackDesc * len(chunk))()
        keep = []
        for d, (w, flip) in zip(descs, chunk):
            cout, cin = w.shape[0], w.shape[1]
            nbytes = conv3x3_packed_bytes(cin if flip else cout, cout if flip else cin, dtype)
            wp = torch.empty(nbytes // (2 if dtype == torch.bfloat16 else 4), dtype=dtype, device=w.device)
            wc = w.contiguous()
            keep.append(wc)
            d.w, d.cout, d.cin, d.flip, d.wp = wc.data_ptr(), cout, cin, int(flip), wp.data_ptr()
            out.append(wp)
        call("eunet_conv3x3_pack_many", ctypes.cast(descs, ctypes.c_void_p), len(chunk), DTYPES[dtype], _stream())
    return out


def conv3x3_tiles(y_act: Act) -> int:
    t = c_int()
    call("eunet_conv3x3_tiles", ctypes.byref(y_act), ctypes.byref(t))
    return t.value


@_dispatched("A T A! T? T? T? T!? i s?")
def conv3x3_fwd(x: Act, wp, y: Act, bias=None, scale=None, shift=None, stats=None, nstride=0, sub=None):
    """nstride > 0: scale/shift are per-sample [N][nstride] (BN+ReLU+Dropout2d folded).
    sub: optional kprof sub-family the launch is also credited to (e.g. the encoder forward convs)."""
    flops = 2.0 * 9 * x.c * y.c * x.n * x.h * x.w
    esz = 2 if x.dtype == _lib.EUNET_BF16 else 4
    # algorithmic HBM bytes: read x once, write y once, read the packed weights once
    nbytes = float(esz * x.n * x.h * x.w * (x.c + y.c) + wp.numel() * wp.element_size())
    with kprof.timed("conv3x3_fwd", flops, nbytes, sub=sub):
        call("eunet_conv3x3_fwd", ctypes.byref(x), _ptr(scale), _ptr(shift), int(nstride), _ptr(wp), _ptr(bias),
             ctypes.byref(y), _ptr(stats), _stream())


@_dispatched("A T A! T?")
def conv3x3_dgrad(dy: Act, wp_t, gx: Act, gscale=None):
    """plain dgrad (the block-input gradient): gx = conv(dy, W'), wp_t packed with flip=True."""
    flops = 2.0 * 9 * dy.c * gx.c * dy.n * dy.h * dy.w
    esz = 2 if dy.dtype == _lib.EUNET_BF16 else 4
    nbytes = float(esz * dy.n * dy.h * dy.w * (dy.c + gx.c) + wp_t.numel() * wp_t.element_size())
    with kprof.timed("conv3x3_dgrad", flops, nbytes):
        call("eunet_conv3x3_dgrad", ctypes.byref(dy), _ptr(wp_t), ctypes.byref(gx), _ptr(gscale), _stream())


@_dispatched("A T A! A T T T T T! T?")
def conv3x3_dgrad_bnbwd(dy: Act, wp_t, gx: Act, y: Act, mean, invstd, scale, shift, part, gscale=None):
    """dgrad + the BN-backward partial sums of the layer it feeds (see eunet.h)."""
    flops = 2.0 * 9 * dy.c * gx.c * dy.n * dy.h * dy.w
    esz = 2 if dy.dtype == _lib.EUNET_BF16 else 4
    nbytes = float(esz * dy.n * dy.h * dy.w * (dy.c + 2 * gx.c) + wp_t.numel() * wp_t.element_size())
    with kprof.timed("conv3x3_dgrad", flops, nbytes):
        call("eunet_conv3x3_dgrad_bnbwd", ctypes.byref(dy), _ptr(wp_t), ctypes.byref(gx), ctypes.byref(y), _ptr(mean),
             _ptr(invstd), _ptr(scale), _ptr(shift), _ptr(gscale), _ptr(part), _stream())


def conv3x3_wgrad_splits(dy: Act, cin: int, dtype) -> int:
    s = c_int()
    call("eunet_conv3x3_wgrad_splits", ctypes.byref(dy), cin, DTYPES[dtype], ctypes.byref(s))
    return s.value


@_dispatched("A A T! T!? i T? T? i")
def conv3x3_wgrad(x: Act, dy: Act, dw_part, db_part, nsplit, scale=None, shift=None, nstride=0):
    flops = 2.0 * 9 * x.c * dy.c * x.n * x.h * x.w
    esz = 2 if x.dtype == _lib.EUNET_BF16 else 4
    # algorithmic HBM bytes: read x and dy once, write the fp32 split partials of dW (and db) once
    nbytes = float(esz * x.n * x.h * x.w * (x.c + dy.c) + 4 * nsplit * dy.c * (9 * x.c + 1))
    with kprof.timed("conv3x3_wgrad", flops, nbytes):
        call("eunet_conv3x3_wgrad", ctypes.byref(x), _ptr(scale), _ptr(shift), int(nstride), ctypes.byref(dy),
             _ptr(dw_part),
             _ptr(db_part), nsplit, _stream())


@_dispatched("T T? i i i i T! T!?")
def wgrad_reduce(dw_part, db_part, nsplit, cout, cin, taps, dw, db):
    call("eunet_wgrad_reduce", _ptr(dw_part), _ptr(db_part), nsplit, cout, cin, taps, _ptr(dw), _ptr(db),
         _stream())


@_dispatched("A T T? A! T!?")
def conv_small_fwd(x: Act, w, bias, y: Act, stats=None):
    call("eunet_conv_small_fwd", ctypes.byref(x), _ptr(w), _ptr(bias), ctypes.byref(y), _ptr(stats), _stream())


def conv3x3_fwd_narrow(x: Act, cin: int, wp, y: Act, bias=None, stats=None):
    """A few-channel conv (cin < 8) on the MFMA forward: x is a view of 8 channels whose channels >= cin
    are zero and wp packs the [cout][cin] weights (its padding is zero too).  Timed as the HBM-bound
    "conv_small" family with its true FLOPs, outside the conv3x3 MFMA roofline family."""
    flops = 2.0 * 9 * cin * y.c * x.n * x.h * x.w
    esz = 2 if x.dtype == _lib.EUNET_BF16 else 4
    nbytes = float(esz * x.n * x.h * x.w * (x.c + y.c))
    with kprof.timed("conv_small", flops, nbytes):
        call("eunet_conv3x3_fwd", ctypes.byref(x), None, None, 0, _ptr(wp), _ptr(bias), ctypes.byref(y),
             _ptr(stats), _stream())


def conv_small_wgrad_splits(dy: Act) -> int:
    s = c_int()
    call("eunet_conv_small_wgrad_splits", ctypes.byref(dy), ctypes.byref(s))
    return s.value


@_dispatched("A A T! T!? i")
def conv_small_wgrad(x: Act, dy: Act, dw_part, db_part, nsplit):
    call("eunet_conv_small_wgrad", ctypes.byref(x), ctypes.byref(dy), _ptr(dw_part), _ptr(db_part), nsplit,
         _stream())


@_dispatched("T i i T T f f T!? T!? T!? T!? T!? T!? T!?")
def bn_finalize(stats, tiles, c, gamma, beta, eps, momentum, run_mean, run_var, mean, invstd, scale, shift,
                num_batches_tracked=None):
    call("eunet_bn_finalize", _ptr(stats), tiles, c, _ptr(gamma), _ptr(beta), float(eps), float(momentum),
         _ptr(run_mean), _ptr(run_var), _ptr(mean), _ptr(invstd), _ptr(scale), _ptr(shift),
         _ptr(num_batches_tracked), _stream())


@_dispatched("T T T T f T! T!")
def bn_eval_affine(gamma, beta, run_mean, run_var, eps, scale, shift):
    call("eunet_bn_eval_affine", gamma.numel(), _ptr(gamma), _ptr(beta), _ptr(run_mean), _ptr(run_var),
         float(eps), _ptr(scale), _ptr(shift), _stream())


@_dispatched("A T T A!")
def bnrelu(y: Act, scale, shift, out: Act):
    call("eunet_bnrelu", ctypes.byref(y), _ptr(scale), _ptr(shift), ctypes.byref(out), _stream())


@_dispatched("A T T A!? A!")
def bnrelu_pool(y: Act, scale, shift, act_out: Act | None, pooled: Act):
    call("eunet_bnrelu_pool", ctypes.byref(y), _ptr(scale), _ptr(shift), _ref(act_out), ctypes.byref(pooled),
         _stream())


@_dispatched("A T T A!")
def bnrelu_upsample(y: Act, scale, shift, out: Act):
    call("eunet_bnrelu_upsample", ctypes.byref(y), _ptr(scale), _ptr(shift), ctypes.byref(out), _stream())


@_dispatched("A T T T T i T!")
def bnrelu_conv1x1(y: Act, scale, shift, w, b, k, z):
    call("eunet_bnrelu_conv1x1", ctypes.byref(y), _ptr(scale), _ptr(shift), _ptr(w), _ptr(b), k, _ptr(z),
         _stream())


KTAIL_UP2, KTAIL_SMOOTH = 0, 1  # EUNET_KTAIL_*


def _ktail_check(name, t, shape):
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise _lib.EunetError(f"{name}: need a contiguous fp32 tensor of shape {tuple(shape)}, got "
                              f"{t.dtype} {tuple(t.shape)}")


@_dispatched("i T T!")
def ktail_fwd(mode, z_lo, out):
    """z_lo [N,h,w,K] NHWC fp32 -> out NCHW fp32: [N,K,2h,2w] = up2(z_lo) (KTAIL_UP2) or
    [N,K,h,w] = mean2x2(up2(z_lo)) (KTAIL_SMOOTH)."""
    n, h, w, k = z_lo.shape
    s = 2 if mode == KTAIL_UP2 else 1
    _ktail_check("ktail_fwd z_lo", z_lo, (n, h, w, k))
    _ktail_check("ktail_fwd out", out, (n, k, s * h, s * w))
    call("eunet_ktail_fwd", int(mode), _ptr(z_lo), n, h, w, k, _ptr(out), _stream())


@_dispatched("i T T!")
def ktail_bwd(mode, g, gz_lo):
    """The adjoints of ktail_fwd: g NCHW -> gz_lo [N,h,w,K]."""
    n, h, w, k = gz_lo.shape
    s = 2 if mode == KTAIL_UP2 else 1
    _ktail_check("ktail_bwd g", g, (n, k, s * h, s * w))
    _ktail_check("ktail_bwd gz_lo", gz_lo, (n, h, w, k))
    call("eunet_ktail_bwd", int(mode), _ptr(g), n, h, w, k, _ptr(gz_lo), _stream())


def head_workspace_bytes(n, h, w, k, dtype=torch.float32):
    b = c_size_t()
    call("eunet_head_workspace_bytes", n, h, w, k, DTYPES[dtype], ctypes.byref(b))
    return b.value


@_dispatched("T i i i i T T T T T T b f f T!? T!? T!? T!? T!? T!? T! d")
def head_fwd(z, n, h, w, k, w1, b1, gamma, beta, w2, b2, training, eps, momentum, run_mean, run_var, mean,
             invstd, out2h, logits, ws, dtype=torch.float32):
    call("eunet_head_fwd", _ptr(z), n, h, w, k, _ptr(w1), _ptr(b1), _ptr(gamma), _ptr(beta), _ptr(w2), _ptr(b2),
         int(training), float(eps), float(momentum), _ptr(run_mean), _ptr(run_var), _ptr(mean), _ptr(invstd),
         _ptr(out2h), _ptr(logits), DTYPES[dtype], _ptr(ws), _stream())


@_dispatched("T i i i i T T T T T T T T? T? T! T! T! T! T! T! T! T! d")
def head_bwd(z, n, h, w, k, w1, b1, gamma, beta, w2, mean, invstd, g_logits, g_out2h, gz, gw1, gb1, ggamma,
             gbeta, gw2, gb2, ws, dtype=torch.float32):
    call("eunet_head_bwd", _ptr(z), n, h, w, k, _ptr(w1), _ptr(b1), _ptr(gamma), _ptr(beta), _ptr(w2),
         _ptr(mean), _ptr(invstd), _ptr(g_logits), _ptr(g_out2h), _ptr(gz), _ptr(gw1), _ptr(gb1), _ptr(ggamma),
         _ptr(gbeta), _ptr(gw2), _ptr(gb2), DTYPES[dtype], _ptr(ws), _stream())


def loss_reference_params() -> _lib.LossParams:
    p = _lib.LossParams()
    call("eunet_loss_reference_params", ctypes.byref(p))
    return p


def loss_sums_len(n, k):
    v = c_int()
    call("eunet_loss_sums_len", n, k, ctypes.byref(v))
    return v.value


def loss_workspace_bytes(n, k, h, w):
    b = c_size_t()
    call("eunet_loss_workspace_bytes", n, k, h, w, ctypes.byref(b))
    return b.value


def loss_fwd(logits, target, params, sums, loss, parts, ws):
    """params: _lib.LossParams or None (the reference Trainer's configuration)."""
    n, k, h, w = logits.shape
    call("eunet_loss_fwd", _ptr(logits), _ptr(target), n, k, h, w, _ref(params), _ptr(sums), _ptr(loss),
         _ptr(parts), _ptr(ws), _stream())


def loss_bwd(logits, target, params, sums, gloss, glogits):
    n, k, h, w = logits.shape
    call("eunet_loss_bwd", _ptr(logits), _ptr(target), n, k, h, w, _ref(params), _ptr(sums), _ptr(gloss),
         _ptr(glogits), _stream())


def loss_fwd_w(logits, target, pixel_weight, params, sums, loss, parts, ws):
    """eunet_loss_fwd_w: loss_fwd with the focal summand multiplied by pixel_weight [N,H,W] fp32."""
    n, k, h, w = logits.shape
    call("eunet_loss_fwd_w", _ptr(logits), _ptr(target), _ptr(pixel_weight), n, k, h, w, _ref(params), _ptr(sums),
         _ptr(loss), _ptr(parts), _ptr(ws), _stream())


def loss_bwd_w(logits, target, pixel_weight, params, sums, gloss, glogits):
    n, k, h, w = logits.shape
    call("eunet_loss_bwd_w", _ptr(logits), _ptr(target), _ptr(pixel_weight), n, k, h, w, _ref(params), _ptr(sums),
         _ptr(gloss), _ptr(glogits), _stream())


# ---- sigmoid BCE + Dice loss (bce_dice.hip) ------------------------------------------------
def bce_dice_default_params() -> _lib.BCEDiceParams:
    p = _lib.BCEDiceParams()
    call("eunet_bce_dice_default_params", ctypes.byref(p))
    return p


def bce_dice_sums_len(n, k):
    v = c_int()
    call("eunet_bce_dice_sums_len", n, k, ctypes.byref(v))
    return v.value


def bce_dice_workspace_bytes(n, k, h, w):
    b = c_size_t()
    call("eunet_bce_dice_workspace_bytes", n, k, h, w, ctypes.byref(b))
    return b.value


# eunet_bce_dice_params as the dispatcher schema spells it: (struct field, kind, schema names); a table of three
# floats is three scalars.  The four op schemas, _bce_flat and _bce_struct are derived from this list.
_BCE_FIELDS = (("pos_weight", "f", ("pw0", "pw1", "pw2")), ("class_weight", "f", ("cw0", "cw1", "cw2")),
               ("dice_weight", "f", ("dw0", "dw1", "dw2")), ("w_bce", "f", ("w_bce",)), ("w_dice", "f", ("w_dice",)),
               ("smooth", "f", ("smooth",)), ("ignore_index", "i", ("ignore_index",)),
               ("target_mode", "i", ("target_mode",)))
_BCE_NAMES = [nm for _, _, names in _BCE_FIELDS for nm in names]
_BCE_KINDS = [kind for _, kind, names in _BCE_FIELDS for _ in names]

_bce_defaults = None  # the library's default parameters as _bce_flat gives them, read once


def _bce_flat(p):
    """eunet_bce_dice_params as the scalars of the dispatcher schema (None: the library's defaults)."""
    global _bce_defaults
    if p is None:
        if _bce_defaults is None:
            _bce_defaults = _bce_flat(bce_dice_default_params())
        return _bce_defaults
    flat = []
    for field, _, names in _BCE_FIELDS:
        v = getattr(p, field)
        flat += list(v) if len(names) > 1 else [v]
    return tuple(flat)


def _bce_struct(v):
    p, j = _lib.BCEDiceParams(), 0
    for field, _, names in _BCE_FIELDS:
        if len(names) > 1:
            getattr(p, field)[:] = v[j:j + len(names)]
        else:
            setattr(p, field, v[j])
        j += len(names)
    return p


def _bce_op(entry, lead, tail):
    """Registers torch.ops.eunet.<entry>(*lead, <the parameter scalars>, *tail) over eunet_<entry>(*lead, n, k, h, w,
    &params, *tail, stream); lead / tail: the tensor arguments as "name:kind" words.  The dispatcher op takes the
    struct spread over scalars (a float of the struct survives the round trip through the schema's double)."""
    lead, tail = ([a.split(":") for a in side.split()] for side in (lead, tail))

    def body(*args):
        tensors, scalars, outs = args[:len(lead)], args[len(lead):-len(tail)], args[-len(tail):]
        n, k, h, w = tensors[0].shape
        call("eunet_" + entry, *map(_ptr, tensors), n, k, h, w, ctypes.byref(_bce_struct(scalars)), *map(_ptr, outs),
             _stream())

    body.__name__ = entry
    return _dispatched(" ".join([k for _, k in lead] + _BCE_KINDS + [k for _, k in tail]),
                       names=[nm for nm, _ in lead] + _BCE_NAMES + [nm for nm, _ in tail])(body)


_FWD, _BWD = "sums:T! loss:T! parts:T! ws:T!", "sums:T gloss:T glogits:T!"
_bce_dice_fwd_op = _bce_op("bce_dice_fwd", "logits:T target:T", _FWD)
_bce_dice_bwd_op = _bce_op("bce_dice_bwd", "logits:T target:T", _BWD)
_bce_dice_fwd_w_op = _bce_op("bce_dice_fwd_w", "logits:T target:T pixel_weight:T", _FWD)
_bce_dice_bwd_w_op = _bce_op("bce_dice_bwd_w", "logits:T target:T pixel_weight:T", _BWD)


# the module's functions of the ops' names take the struct
def bce_dice_fwd(logits, target, params, sums, loss, parts, ws):
    """torch.ops.eunet.bce_dice_fwd; params: _lib.BCEDiceParams or None (the library's defaults)."""
    _bce_dice_fwd_op(logits, target, *_bce_flat(params), sums, loss, parts, ws)


def bce_dice_bwd(logits, target, params, sums, gloss, glogits):
    """torch.ops.eunet.bce_dice_bwd: glogits = gloss * d loss / d logits from the forward's sums."""
    _bce_dice_bwd_op(logits, target, *_bce_flat(params), sums, gloss, glogits)


def bce_dice_fwd_w(logits, target, pixel_weight, params, sums, loss, parts, ws):
    """torch.ops.eunet.bce_dice_fwd_w: bce_dice_fwd with bce(x,t)_c multiplied by pixel_weight [N,H,W] fp32."""
    _bce_dice_fwd_w_op(logits, target, pixel_weight, *_bce_flat(params), sums, loss, parts, ws)


def bce_dice_bwd_w(logits, target, pixel_weight, params, sums, gloss, glogits):
    _bce_dice_bwd_w_op(logits, target, pixel_weight, *_bce_flat(params), sums, gloss, glogits)


# ---- U-Net border weight map and instance separation (weightmap.hip) -------------------------
@_dispatched("T T? f f f f f i T!")
def border_weight_map(labels, semantic, cw0, cw1, cw2, w0, sigma, radius, out):
    n, h, w = labels.shape
    cw = (_lib.c_float * 3)(cw0, cw1, cw2)
    call("eunet_border_weight_map", _ptr(labels), _ptr(semantic), n, h, w, ctypes.byref(cw), w0, sigma, radius,
         _ptr(out), _stream())


_border_weight_map_op = border_weight_map  # torch.ops.eunet.border_weight_map writes into out; the function below allocates it


def _label_maps(what, labels, semantic):
    """labels / semantic as contiguous int64 [N,H,W] device tensors ([H,W] is N = 1) and whether a batch axis was added."""
    if labels.dim() not in (2, 3):
        raise ValueError(f"{what}: labels must be [H, W] or [N, H, W], got {tuple(labels.shape)}")
    if labels.dtype != torch.int64:
        raise ValueError(f"{what}: labels must be int64, got {labels.dtype}")
    if semantic is not None and (semantic.dtype != torch.int64 or semantic.shape != labels.shape or
                                 semantic.device != labels.device):
        raise ValueError(f"{what}: semantic must be int64 of labels' shape {tuple(labels.shape)} on its device")
    squeeze = labels.dim() == 2
    lb = labels.contiguous()
    sm = None if semantic is None else semantic.contiguous()
    if squeeze:
        lb, sm = lb.unsqueeze(0), None if sm is None else sm.unsqueeze(0)
    return lb, sm, squeeze


def border_weight_map(labels, semantic=None, *, class_weight=(1.0, 1.0, 1.0), w0: float = 10.0, sigma: float = 5.0,
                      radius=None, out=None):
    """The U-Net border weight map (include/eunet.h, eunet_border_weight_map): labels int64 [N,H,W] or [H,W]
    (0 background, anything else an instance id), semantic (optional, same shape) -> float32 of labels' shape,
    class_weight[semantic] + w0 exp(-(d1 + d2)^2 / (2 sigma^2)) on background pixels with two distinct ids inside
    the square window of radius R (None: ceil(5.5 sigma); 1 <= R <= 48)."""
    lb, sm, squeeze = _label_maps("border_weight_map", labels, semantic)
    cw = [float(c) for c in class_weight]
    if len(cw) != 3:
        raise ValueError(f"border_weight_map: class_weight needs 3 values, got {len(cw)}")
    if not float(sigma) > 0.0 or not float(w0) >= 0.0:
        raise ValueError(f"border_weight_map: needs sigma > 0 and w0 >= 0, got sigma {sigma}, w0 {w0}")
    r = _lib.WMAP_RADIUS_AUTO if radius is None else int(radius)
    if radius is not None and not 1 <= r <= _lib.WMAP_MAX_RADIUS:
        raise ValueError(f"border_weight_map: radius {radius} outside 1..{_lib.WMAP_MAX_RADIUS}")
    if out is None:
        out = torch.empty(labels.shape, dtype=torch.float32, device=labels.device)
    elif out.dtype != torch.float32 or out.shape != labels.shape or not out.is_contiguous() or out.device != labels.device:
        raise ValueError("border_weight_map: out must be a contiguous float32 tensor of labels' shape on its device")
    _border_weight_map_op(lb, sm, cw[0], cw[1], cw[2], float(w0), float(sigma), r, out.unsqueeze(0) if squeeze else out)
    return out


@_dispatched("T T? T! T!?")
def separate_instances(labels, semantic, labels_out, semantic_out):
    n, h, w = labels.shape
    call("eunet_separate_instances", _ptr(labels), _ptr(semantic), n, h, w, _ptr(labels_out), _ptr(semantic_out),
         _stream())


_separate_instances_op = separate_instances


def separate_instances(labels, semantic=None):
    """eunet_separate_instances: a pixel whose 3x3 neighbourhood holds another instance's label becomes background
    in labels and in semantic, so both sides of a contact lose one pixel -> (labels', semantic' or None)."""
    lb, sm, squeeze = _label_maps("separate_instances", labels, semantic)
    lo = torch.empty_like(lb)
    so = None if sm is None else torch.empty_like(sm)
    _separate_instances_op(lb, sm, lo, so)
    if squeeze:
        lo, so = lo[0], None if so is None else so[0]
    return lo, so


def bn_bwd_tiles(y: Act) -> int:
    t = c_int()
    call("eunet_bn_bwd_tiles", ctypes.byref(y), ctypes.byref(t))
    return t.value


@_dispatched("A A T T T T T!")
def bn_bwd_reduce(g: Act, y: Act, mean, invstd, scale, shift, part):
    call("eunet_bn_bwd_reduce", ctypes.byref(g), ctypes.byref(y), _ptr(mean), _ptr(invstd), _ptr(scale),
         _ptr(shift), _ptr(part), _stream())


@_dispatched("T i i T! i? T!?")
def colsum(part, rows, cols, out, split=None, out_hi=None):
    """Column sums of part [rows][cols] -> out (or out[:split] / out_hi[:cols - split])."""
    b = c_size_t()
    call("eunet_colsum_ws_bytes", rows, cols, ctypes.byref(b))
    ws = torch.empty(b.value, dtype=torch.uint8, device=part.device)
    if out_hi is None:
        call("eunet_colsum", _ptr(part), rows, cols, _ptr(out), _ptr(ws), _stream())
    else:
        call("eunet_colsum_split", _ptr(part), rows, cols, int(split), _ptr(out), _ptr(out_hi), _ptr(ws), _stream())


@_dispatched("A A T T T T T T A!")
def bn_bwd_apply(g: Act, y: Act, mean, invstd, scale, shift, dbeta, dgamma, gy: Act):
    """scale / shift: the BN's forward affine (they define the ReLU mask, see eunet.h)."""
    call("eunet_bn_bwd_apply", ctypes.byref(g), ctypes.byref(y), _ptr(mean), _ptr(invstd), _ptr(scale),
         _ptr(shift), _ptr(dbeta), _ptr(dgamma), ctypes.byref(gy), _stream())


@_dispatched("A A A? A!")
def pool_bwd_add(act_saved: Act, gpool: Act, gskip: Act | None, gout: Act):
    call("eunet_pool_bwd_add", ctypes.byref(act_saved), ctypes.byref(gpool), _ref(gskip), ctypes.byref(gout),
         _stream())


@_dispatched("A A!")
def upsample_bwd(ghi: Act, glo: Act):
    call("eunet_upsample_bwd", ctypes.byref(ghi), ctypes.byref(glo), _stream())


def pool_bwd_add_bnr_rows(gout: Act) -> int:
    r = c_int()
    call("eunet_pool_bwd_add_bnr_rows", ctypes.byref(gout), ctypes.byref(r))
    return r.value


@_dispatched("A A A? A!? A T T T T T!")
def pool_bwd_add_bnr(act_saved: Act, gpool: Act, gskip: Act | None, gout: Act | None, y: Act, mean, invstd, scale,
                     shift, part):
    """pool_bwd_add + the BN-backward partial sums of the block whose output gradient gout is (gout None: reduced
    only, bn_bwd_apply_pool recomputes it)."""
    call("eunet_pool_bwd_add_bnr", ctypes.byref(act_saved), ctypes.byref(gpool), _ref(gskip), _ref(gout),
         ctypes.byref(y), _ptr(mean), _ptr(invstd), _ptr(scale), _ptr(shift), _ptr(part), _stream())


@_dispatched("A A? A T T T T T T A!")
def bn_bwd_apply_pool(gpool: Act, gskip: Act | None, y: Act, mean, invstd, scale, shift, dbeta, dgamma, gy: Act):
    """bn_bwd_apply of gout = gskip + scatter(gpool) that pool_bwd_add_bnr reduced without storing (recomputed per
    2x2 window with its arithmetic and rounding: the same gy bit for bit)."""
    call("eunet_bn_bwd_apply_pool", ctypes.byref(gpool), _ref(gskip), ctypes.byref(y), _ptr(mean), _ptr(invstd),
         _ptr(scale), _ptr(shift), _ptr(dbeta), _ptr(dgamma), ctypes.byref(gy), _stream())


def upsample_bwd_bnr_rows(glo: Act) -> int:
    r = c_int()
    call("eunet_upsample_bwd_bnr_rows", ctypes.byref(glo), ctypes.byref(r))
    return r.value


@_dispatched("A A! A T T T T T!")
def upsample_bwd_bnr(ghi: Act, glo: Act, y: Act, mean, invstd, scale, shift, part):
    """upsample_bwd + the BN-backward partial sums of the block whose output gradient glo is."""
    call("eunet_upsample_bwd_bnr", ctypes.byref(ghi), ctypes.byref(glo), ctypes.byref(y), _ptr(mean), _ptr(invstd),
         _ptr(scale), _ptr(shift), _ptr(part), _stream())


# ---- learned 2x upsample: ConvTranspose2d(C, C, 2, stride=2) behind a BN+ReLU (upconv.hip) ----------
# kprof family "upconv2x2", credited with the algorithmic counts of one pass: 8 M C^2 FLOP and, in bytes,
# the M x C low-res tensor + the 4M x C high-res one + the weights (10 M C at bf16).
def _upconv_counts(lo: Act, extra_bytes: float = 0.0):
    m = lo.n * lo.h * lo.w
    esz = 2 if lo.dtype == _lib.EUNET_BF16 else 4
    return 8.0 * m * lo.c * lo.c, float(esz * (5 * m * lo.c + 4 * lo.c * lo.c)) + extra_bytes


def upconv2x2_packed_bytes(c, dtype):
    b = c_size_t()
    call("eunet_upconv2x2_packed_bytes", c, DTYPES[dtype], ctypes.byref(b))
    return b.value


def _upconv_weight(name, w):
    if w.dim() != 4 or w.shape[0] != w.shape[1] or tuple(w.shape[2:]) != (2, 2) or w.dtype != torch.float32:
        raise _lib.EunetError(f"{name}: need an fp32 ConvTranspose2d weight [C, C, 2, 2], got {w.dtype} {tuple(w.shape)}")
    return w.shape[0]


@_dispatched("T d", returns_tensor=True)
def upconv2x2_pack(w: torch.Tensor, dtype) -> torch.Tensor:
    """torch weight [C, C, 2, 2] fp32 -> the packed forward + data-gradient operands (once per step)."""
    c = _upconv_weight("upconv2x2_pack", w)
    if dtype not in DTYPES:
        raise _lib.EunetError(f"upconv2x2_pack: dtype {dtype} is not fp32 / bf16")
    wp = torch.empty(8 * c * c, dtype=dtype, device=w.device)
    with kprof.timed("upconv2x2", 0.0, float(16 * c * c + wp.numel() * wp.element_size())):
        call("eunet_upconv2x2_pack", _ptr(w.contiguous()), c, _ptr(wp), DTYPES[dtype], _stream())
    return wp


def _upconv_packed(name, wp, a: Act):
    if wp.dim() != 1 or DTYPES.get(wp.dtype) != a.dtype or wp.numel() != 8 * a.c * a.c:
        raise _lib.EunetError(f"{name}: packed weights {wp.dtype} [{wp.numel()}] do not fit C = {a.c} of the "
                              "activations (upconv2x2_pack of the same dtype)")


@_dispatched("A T T T T A!")
def bnrelu_upconv2x2(y: Act, scale, shift, wp, bias, out: Act):
    """out[n, 2i+a, 2j+b, :] = bias + relu(bn(y))[n, i, j, :] @ W[:, :, a, b] (eunet_bnrelu_upconv2x2_fwd)."""
    _upconv_packed("bnrelu_upconv2x2", wp, y)
    for nm, t in (("scale", scale), ("shift", shift), ("bias", bias)):
        if t.dtype != torch.float32 or t.numel() != y.c:
            raise _lib.EunetError(f"bnrelu_upconv2x2: {nm} must be fp32 [{y.c}], got {t.dtype} {tuple(t.shape)}")
    flops, nbytes = _upconv_counts(y)
    with kprof.timed("upconv2x2", flops, nbytes):
        call("eunet_bnrelu_upconv2x2_fwd", ctypes.byref(y), _ptr(scale), _ptr(shift), _ptr(wp), _ptr(bias),
             ctypes.byref(out), _stream())


@_dispatched("A T A!")
def upconv2x2_dgrad(g: Act, wp, gd: Act):
    """gd[n, i, j, ci] = sum_{a, b, co} g[n, 2i+a, 2j+b, co] W[ci, co, a, b]: the gradient w.r.t. relu(bn(y))."""
    _upconv_packed("upconv2x2_dgrad", wp, gd)
    flops, nbytes = _upconv_counts(gd)
    with kprof.timed("upconv2x2", flops, nbytes):
        call("eunet_upconv2x2_dgrad", ctypes.byref(g), _ptr(wp), ctypes.byref(gd), _stream())


def upconv2x2_wgrad_splits(y: Act, dtype) -> int:
    s = c_int()
    call("eunet_upconv2x2_wgrad_splits", ctypes.byref(y), DTYPES[dtype], ctypes.byref(s))
    return s.value


@_dispatched("A T T A T! T!? i")
def upconv2x2_wgrad(y: Act, scale, shift, g: Act, dw_part, db_part, nsplit):
    """Split partials of dW and db: dw_part [nsplit, C, 4, C] (wgrad_reduce(cout = cin = C, taps = 4) -> torch's
    [C, C, 2, 2]), db_part [nsplit, 4, C] (colsum over nsplit * 4 rows -> db)."""
    c = y.c
    if dw_part.dtype != torch.float32 or dw_part.numel() < nsplit * 4 * c * c:
        raise _lib.EunetError(f"upconv2x2_wgrad: dw_part must be fp32 with >= {nsplit * 4 * c * c} elements")
    if db_part is not None and (db_part.dtype != torch.float32 or db_part.numel() < nsplit * 4 * c):
        raise _lib.EunetError(f"upconv2x2_wgrad: db_part must be fp32 with >= {nsplit * 4 * c} elements")
    for nm, t in (("scale", scale), ("shift", shift)):
        if t.dtype != torch.float32 or t.numel() != c:
            raise _lib.EunetError(f"upconv2x2_wgrad: {nm} must be fp32 [{c}], got {t.dtype} {tuple(t.shape)}")
    flops, nbytes = _upconv_counts(y, 4.0 * nsplit * 4 * c * (c + 1))
    with kprof.timed("upconv2x2", flops, nbytes):
        call("eunet_upconv2x2_wgrad", ctypes.byref(y), _ptr(scale), _ptr(shift), ctypes.byref(g), _ptr(dw_part),
             _ptr(db_part), int(nsplit), _stream())


def conv1x1_bwd_tiles(y: Act) -> int:
    t = c_int()
    call("eunet_conv1x1_bwd_tiles", ctypes.byref(y), ctypes.byref(t))
    return t.value


@_dispatched("A T T T i T A! T!?")
def conv1x1_bwd(y: Act, scale, shift, w, k, gz, gact: Act, part):
    call("eunet_conv1x1_bwd", ctypes.byref(y), _ptr(scale), _ptr(shift), _ptr(w), k, _ptr(gz),
         ctypes.byref(gact), _ptr(part), _stream())


@_dispatched("A T T T i T A!? T!? T T T!")
def conv1x1_bwd_bnr(y: Act, scale, shift, w, k, gz, gact: Act | None, part, mean, invstd, bn_part):
    """conv1x1_bwd + the BN-backward partial sums [tiles][2][C] of y's BatchNorm over gact (gact None: the
    gradient is reduced, not stored -- bn_bwd_apply_1x1 recomputes it)."""
    call("eunet_conv1x1_bwd_bnr", ctypes.byref(y), _ptr(scale), _ptr(shift), _ptr(w), k, _ptr(gz),
         _ref(gact), _ptr(part), _ptr(mean), _ptr(invstd), _ptr(bn_part), _stream())


@_dispatched("A T i T T T T T T T A!")
def bn_bwd_apply_1x1(y: Act, w, k, gz, mean, invstd, scale, shift, dbeta, dgamma, gy: Act):
    """bn_bwd_apply of the gradient W^T gz that conv1x1_bwd_bnr reduced without storing (recomputed per pixel
    with its arithmetic and rounding: the same gy bit for bit)."""
    call("eunet_bn_bwd_apply_1x1", ctypes.byref(y), _ptr(w), k, _ptr(gz), _ptr(mean), _ptr(invstd), _ptr(scale),
         _ptr(shift), _ptr(dbeta), _ptr(dgamma), ctypes.byref(gy), _stream())


# ---- evaluation path (evalpath.hip) ------------------------------------------------
def semantic_counts(pred, gt):
    """pred, gt int64 [n, ...] -> counts int64 [n, 3, 3] = (#pred==c, #gt==c, #both==c)."""
    n = pred.shape[0]
    hw = pred[0].numel()
    counts = torch.empty(n, 3, 3, dtype=torch.int64, device=pred.device)
    call("eunet_semantic_counts", _ptr(pred.contiguous()), _ptr(gt.contiguous()), n, hw, _ptr(counts), _stream())
    return counts


def binary_overlap(a, b):
    """int64 masks -> (inter, union, sum a, sum b) as python ints (nonzero = foreground)."""
    out = torch.empty(4, dtype=torch.int64, device=a.device)
    call("eunet_binary_overlap", _ptr(a.contiguous()), _ptr(b.contiguous()), a.numel(), _ptr(out), _stream())
    return tuple(int(v) for v in out.tolist())


def resize_bilinear(x, hout, wout, scale_h=None, scale_w=None, flip_h=False, flip_w=False, out=None):
    """x [..., H, W] fp32 -> [..., hout, wout]; scale_* = 1/scale_factor (F.interpolate with
    scale_factor) or None for in/out (F.interpolate with size)."""
    x = x.contiguous()
    hin, win = x.shape[-2:]
    planes = x.numel() // (hin * win)
    sh = float(scale_h) if scale_h is not None else hin / hout
    sw = float(scale_w) if scale_w is not None else win / wout
    y = out if out is not None else torch.empty(*x.shape[:-2], hout, wout, dtype=torch.float32, device=x.device)
    call("eunet_resize_bilinear", _ptr(x), planes, hin, win, _ptr(y), hout, wout, sh, sw, int(flip_h), int(flip_w),
         _stream())
    return y


def softmax_crop(logits, h, w, flip_h=False, flip_w=False, out=None):
    """logits [K, hp, wp] fp32 -> probs [K, h, w] (crop to the top-left h x w, optional flips)."""
    logits = logits.contiguous().float()
    k, hp, wp = logits.shape
    y = out if out is not None else torch.empty(k, h, w, dtype=torch.float32, device=logits.device)
    call("eunet_softmax_crop", _ptr(logits), k, hp, wp, h, w, int(flip_h), int(flip_w), _ptr(y), _stream())
    return y


def accumulate(acc, p, mode: int, count: float = 1.0):
    call("eunet_accumulate", _ptr(acc), _ptr(p.contiguous()), acc.numel(), int(mode), float(count), _stream())


def probs_to_mask(probs):
    """probs [K, h, w] fp32 -> int64 mask [h, w] (the reference's thresholded conversion)."""
    probs = probs.contiguous().float()
    k, h, w = probs.shape
    mask = torch.empty(h, w, dtype=torch.int64, device=probs.device)
    ws = torch.empty(2, dtype=torch.int64, device=probs.device)
    call("eunet_probs_to_mask", _ptr(probs), k, h, w, _ptr(mask), _ptr(ws), _stream())
    return mask


@_dispatched("T i i b b T!")
def sigmoid_crop(logits, h, w, flip_h, flip_w, out):
    k, hp, wp = logits.shape
    call("eunet_sigmoid_crop", _ptr(logits), k, hp, wp, h, w, int(flip_h), int(flip_w), _ptr(out), _stream())


_sigmoid_crop_op = sigmoid_crop  # torch.ops.eunet.sigmoid_crop writes into out; the function below allocates it


def sigmoid_crop(logits, h, w, flip_h=False, flip_w=False, out=None):
    """logits [K, hp, wp] fp32 (K = 1..3) -> sigmoid probs [K, h, w]: softmax_crop's crop and flips."""
    logits = logits.contiguous().float()
    y = out if out is not None else torch.empty(logits.shape[0], h, w, dtype=torch.float32, device=logits.device)
    _sigmoid_crop_op(logits, h, w, bool(flip_h), bool(flip_w), y)
    return y


@_dispatched("T f T!")
def probs_threshold(probs, threshold, mask):
    k, h, w = probs.shape
    call("eunet_probs_threshold", _ptr(probs), k, h, w, float(threshold), _ptr(mask), _stream())


_probs_threshold_op = probs_threshold


def probs_threshold(probs, threshold: float = 0.5):
    """probs [K, h, w] fp32 -> int64 mask [h, w]: K = 1 [p >= threshold]; K >= 2 the argmax (first maximum)."""
    probs = probs.contiguous().float()
    mask = torch.empty(probs.shape[1:], dtype=torch.int64, device=probs.device)
    _probs_threshold_op(probs, float(threshold), mask)
    return mask


# ---- pixel-level score histograms (curves.hip) ---------------------------------------------
SCORE_HIST_MAX_BINS = 3072
_edge_tables: dict = {}  # (device, table bytes) -> the validated table on that device
_edge_checked: dict = {}  # (device, data_ptr, numel, version) of the device tables already validated


@_dispatched("T T T i T! T!")
def score_hist(probs, mask, edges, ignore_index, hist, invalid):
    n, k = probs.shape[:2]
    hw = probs[0, 0].numel()
    # one read of the probabilities and, per class, of the mask
    with kprof.timed("score_hist", 0.0, 4.0 * probs.numel() + 8.0 * k * mask.numel()):
        call("eunet_score_hist", _ptr(probs), _ptr(mask), n, k, hw, _ptr(edges), edges.numel() - 1, ignore_index,
             _ptr(hist), _ptr(invalid), _stream())


_score_hist_op = score_hist  # torch.ops.eunet.score_hist adds into hist and invalid; the function below allocates them


def _check_edges(e):
    """e: a host float32 array.  The table eunet_score_hist requires, or ValueError."""
    import numpy as np
    if e.ndim != 1 or e.size < 2 or e.size - 1 > SCORE_HIST_MAX_BINS:
        raise ValueError(f"score_hist: edges must be bins + 1 values, bins = 1..{SCORE_HIST_MAX_BINS}, "
                         f"got shape {tuple(e.shape)}")
    if e[0] != 0.0 or e[-1] != 1.0 or not bool(np.all(np.diff(e) > 0)):
        raise ValueError("score_hist: edges must be strictly increasing from edges[0] = 0 to edges[bins] = 1")


def score_edges(edges, device):
    """The validated fp32 edge table on `device`: a host array (or sequence) is checked, uploaded once and kept;
    a device tensor is checked once (one copy to the host) and passed through."""
    import numpy as np
    device = torch.device(device)
    if isinstance(edges, torch.Tensor):
        if edges.dtype != torch.float32 or edges.dim() != 1 or not edges.is_contiguous():
            raise ValueError(f"score_hist: edges must be a contiguous 1-D fp32 table, got {tuple(edges.shape)} "
                             f"{edges.dtype}")
        if not edges.is_cuda:
            return score_edges(edges.numpy(), device)
        if edges.device != device:
            raise ValueError(f"score_hist: edges live on {edges.device}, probs on {device}")
        key = (str(device), edges.data_ptr(), edges.numel(), edges._version)
        if key not in _edge_checked:
            _check_edges(edges.cpu().numpy())
            if len(_edge_checked) >= 16:
                _edge_checked.clear()
            _edge_checked[key] = True
        return edges
    e = np.ascontiguousarray(np.asarray(edges), dtype=np.float32)
    _check_edges(e)
    key = (str(device), e.tobytes())
    if key not in _edge_tables:
        if len(_edge_tables) >= 16:
            _edge_tables.clear()
        _edge_tables[key] = torch.from_numpy(e.copy()).to(device)
    return _edge_tables[key]


def score_hist(probs, mask, edges, ignore_index: int = 255, out=None):
    """probs [K, h, w] or [N, K, h, w] fp32 (K = 1..3), mask int64 [h, w] or [N, h, w], edges bins + 1 floats
    (metrics.curve_edges; a host array or a device tensor) -> (hist int64 [K, bins, 3], invalid int64 [1]).

    hist[c, b] = (#negatives, #positives, sum of llrint(min(p, 1) 2^24)) of class c in score bin b
    (edges[b] <= p < edges[b+1] in fp32, the last bin closed); a pixel of mask == ignore_index counts nowhere,
    a p that is NaN, +-inf or < 0 only in invalid (include/eunet.h, eunet_score_hist).  out = (hist, invalid)
    is added to -- how a validation set streams through; None allocates zeroed ones."""
    if not isinstance(probs, torch.Tensor) or not isinstance(mask, torch.Tensor):
        raise ValueError("score_hist: probs and mask must be tensors")
    if not probs.is_cuda or not mask.is_cuda or probs.device != mask.device:
        raise ValueError(f"score_hist: probs and mask must live on one GPU, got {probs.device} and {mask.device}")
    if probs.dtype != torch.float32 or mask.dtype != torch.int64:
        raise ValueError(f"score_hist: probs must be fp32 and mask int64, got {probs.dtype} and {mask.dtype}")
    if probs.dim() == 3 and mask.dim() == 2:
        probs, mask = probs.unsqueeze(0), mask.unsqueeze(0)
    elif probs.dim() != 4 or mask.dim() != 3:
        raise ValueError(f"score_hist: probs [K, h, w] with mask [h, w], or [N, K, h, w] with [N, h, w]; got "
                         f"{tuple(probs.shape)} and {tuple(mask.shape)}")
    n, k, h, w = probs.shape
    if tuple(mask.shape) != (n, h, w) or not 1 <= k <= 3 or n < 1 or h * w < 1:
        raise ValueError(f"score_hist: probs {tuple(probs.shape)} (K = 1..3, no empty axis) and mask "
                         f"{tuple(mask.shape)} do not agree")
    if not probs.is_contiguous() or not mask.is_contiguous():
        raise ValueError("score_hist: probs and mask must be contiguous")
    if not -2 ** 31 <= int(ignore_index) < 2 ** 31:
        raise ValueError(f"score_hist: ignore_index {ignore_index} is not an int32")
    e = score_edges(edges, probs.device)
    bins = e.numel() - 1
    if out is None:
        hist = torch.zeros(k, bins, 3, dtype=torch.int64, device=probs.device)
        invalid = torch.zeros(1, dtype=torch.int64, device=probs.device)
    else:
        hist, invalid = out
        for name, t, shape in (("hist", hist, (k, bins, 3)), ("invalid", invalid, (1,))):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.int64 or \
                    not t.is_contiguous() or t.device != probs.device:
                raise ValueError(f"score_hist: out {name} must be a contiguous int64 {shape} on {probs.device}")
    _score_hist_op(probs, mask, e, int(ignore_index), hist, invalid)
    return hist, invalid


# ---- exact distance transform and boundary statistics (boundary.hip) ------------------------
EDT_MODES = {"eq": _lib.EDT_EQ, "ne": _lib.EDT_NE, "edge": _lib.EDT_EDGE}  # EUNET_EDT_*
EDT_NONE = _lib.EDT_NONE


@_dispatched("T I i T!")
def distance_transform_sq(labels, values, mode, out):
    n, h, w = labels.shape
    vals = (_lib.c_int64 * len(values))(*values)
    # the column pass reads the map (with its neighbours from cache) and writes and re-reads the plane; the row
    # pass reads and writes it once more
    with kprof.timed("edt_sq", 0.0, len(values) * labels.numel() * (8.0 + 4 * 4.0)):
        call("eunet_edt_sq", _ptr(labels), n, h, w, vals, len(values), mode, _ptr(out), _stream())


_distance_transform_sq_op = distance_transform_sq  # torch.ops.eunet.distance_transform_sq writes into out


def _plane_shape(name, what, shape, bound_pixels, planes="p", verb="are"):
    """An [h, w] or [p, h, w] shape as (p, h, w), within the plane-stack rule of the label-map kernels (csrc/labelmap.h,
    plane_stack_ok): p 1..65535, h and w 1..EDT_MAX_SIDE, and with bound_pixels p h w < 2^31."""
    p, h, w = (1,) + tuple(shape) if len(shape) == 2 else tuple(shape)
    side = _lib.EDT_MAX_SIDE
    if not (1 <= p <= 65535 and 1 <= h <= side and 1 <= w <= side and (not bound_pixels or p * h * w < 2 ** 31)):
        raise ValueError(f"{name}: {what} {tuple(shape)} {verb} outside {planes} 1..65535, h and w 1..{side}"
                         + (", p h w < 2^31" if bound_pixels else ""))
    return p, h, w


def _table_cap(name, capacity):
    """The _table_capacity argument of an op with a growing hash table: None, or a power of two in 2..2^30."""
    if capacity is None:
        return None
    cap = int(capacity)
    if cap < 2 or cap > 2 ** 30 or cap & (cap - 1):
        raise ValueError(f"{name}: _table_capacity must be a power of two in 2..2^30, got {capacity!r}")
    return cap


def _fill_table(name, what, cap, launch):
    """Runs launch(cap) -> (inserts that found no slot, what the caller reads back) with a table of cap slots, twice as
    large each time, until every insert found one -> (cap, what the last launch read back)."""
    while True:
        overflow, back = launch(cap)
        if overflow == 0:
            return cap, back
        if cap >= 2 ** 30:
            raise _lib.EunetError(f"{name}: the {what} table overflows at 2^30 slots")
        cap *= 2  # nothing was dropped silently: the pass is run again with room for every pair


def _int64_maps(name, what, t, device=None):
    """t as a contiguous int64 [n, h, w] device map within the transform's limits (and whether it came as [h, w])."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: {what} must be a tensor")
    if not t.is_cuda or (device is not None and t.device != device):
        raise ValueError(f"{name}: {what} must live on {'one GPU' if device is None else device}, got {t.device}")
    if t.dtype != torch.int64:
        raise ValueError(f"{name}: {what} must be int64, got {t.dtype}")
    if t.dim() not in (2, 3):
        raise ValueError(f"{name}: {what} must be [h, w] or [n, h, w], got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: {what} must be contiguous")
    single = t.dim() == 2
    if single:
        t = t.unsqueeze(0)
    _plane_shape(name, what, t.shape, False, planes="n", verb="is")
    return t, single


def _int_list(name, what, xs, lo, hi, nmin, nmax):
    import operator
    try:
        out = [operator.index(x) for x in xs]
    except TypeError:
        raise ValueError(f"{name}: {what} must be a sequence of integers, got {xs!r}") from None
    if not nmin <= len(out) <= nmax or any(not lo <= x <= hi for x in out):
        raise ValueError(f"{name}: {what} must be {nmin}..{nmax} integers in [{lo}, {hi}], got {xs!r}")
    return out


def _out_buffer(name, what, t, shape, dtype, device):
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or \
            not t.is_contiguous() or t.device != device:
        raise ValueError(f"{name}: out {what} must be a contiguous {dtype} {tuple(shape)} on {device}")
    return t


def distance_transform_sq(labels, values, mode: str = "eq", out=None):
    """labels int64 [n, h, w] or [h, w], values 1..8 integers -> int32 [n, nv, h, w] (or [nv, h, w]): the exact
    squared Euclidean distance of every pixel to the nearest site of its own sample, the sites of plane j being
    the pixels equal to values[j] (mode "eq"), different from it ("ne") or on its edge ("edge": equal, with a
    4-neighbour that is not, or that lies outside the image).  A sample without a site is EDT_NONE (INT32_MAX)
    everywhere.  h, w <= 8192.  out: the buffer to write (include/eunet.h, eunet_edt_sq)."""
    name = "distance_transform_sq"
    if mode not in EDT_MODES:
        raise ValueError(f"{name}: mode must be one of {sorted(EDT_MODES)}, not {mode!r}")
    t, single = _int64_maps(name, "labels", labels)
    vals = _int_list(name, "values", values, -2 ** 63, 2 ** 63 - 1, 1, _lib.EDT_MAX_VALUES)
    n, h, w = t.shape
    shape = (len(vals), h, w) if single else (n, len(vals), h, w)
    if out is None:
        out = torch.empty(shape, dtype=torch.int32, device=t.device)
    else:
        _out_buffer(name, "", out, shape, torch.int32, t.device)
    _distance_transform_sq_op(t, vals, EDT_MODES[mode], out)
    return out


@_dispatched("T T i i i I T! T! T!? T!")
def boundary_stats(pred, gt, k, ignore_index, cap, radii, ws, surf, band, refrows):
    n, h, w = pred.shape
    rr = (c_int * max(len(radii), 1))(*radii)
    # two transforms, the 13-pixel pass over both maps and the statistics pass over maps and transforms
    with kprof.timed("boundary_stats", 0.0, pred.numel() * (2 * k * (8.0 + 4 * 4.0) + 16.0 + k * 24.0)):
        call("eunet_boundary_stats", _ptr(pred), _ptr(gt), n, h, w, k, ignore_index, cap, rr, len(radii), _ptr(ws),
             _ptr(surf), _ptr(band), _ptr(refrows), _stream())


_boundary_stats_op = boundary_stats  # torch.ops.eunet.boundary_stats adds into surf, band and refrows


def boundary_workspace_bytes(n, k, h, w):
    b = c_size_t()
    call("eunet_boundary_workspace_bytes", n, k, h, w, ctypes.byref(b))
    return b.value


def boundary_stats(pred, gt, num_classes: int = 3, ignore_index: int = 255, cap: int = 64, band_radii=(2,), out=None):
    """pred, gt int64 [h, w] or [n, h, w] -> (surf int64 [k, 2, cap^2 + 5], band int64 [k, nr, 3], refrows int64
    [n, k, 2, 3]): the edge-to-edge squared-distance histograms of both directions with their overflow and
    no-edge counts, maximum and fixed-point distance sum; the Boundary-IoU band counts for each radius; the
    reference's boundary and interior set counts per image (include/eunet.h, eunet_boundary_stats).  A pixel whose
    gt is ignore_index is ignored in pred too, except in refrows.  out = (surf, band, refrows) is added to (the
    maximum is combined by max); None allocates zeroed ones."""
    name = "boundary_stats"
    p, _ = _int64_maps(name, "pred", pred)
    g, _ = _int64_maps(name, "gt", gt, p.device)
    if p.shape != g.shape:
        raise ValueError(f"{name}: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape")
    k, cap = int(num_classes), int(cap)
    if not 1 <= k <= 3:
        raise ValueError(f"{name}: num_classes must be 1..3, not {num_classes}")
    if not 1 <= cap <= _lib.BOUNDARY_MAX_CAP:
        raise ValueError(f"{name}: cap must be 1..{_lib.BOUNDARY_MAX_CAP}, not {cap}")
    if not -2 ** 31 <= int(ignore_index) < 2 ** 31:
        raise ValueError(f"{name}: ignore_index {ignore_index} is not an int32")
    radii = _int_list(name, "band_radii", band_radii, 0, 2 ** 31 - 1, 0, _lib.BOUNDARY_MAX_RADII)
    n, h, w = p.shape
    shapes = ((k, 2, cap * cap + 5), (k, len(radii), 3), (n, k, 2, 3))
    if out is None:
        surf, band, refrows = (torch.zeros(s, dtype=torch.int64, device=p.device) for s in shapes)
    else:
        if not isinstance(out, (tuple, list)) or len(out) != 3:
            raise ValueError(f"{name}: out must be (surf, band, refrows)")
        surf, band, refrows = (_out_buffer(name, what, t, s, torch.int64, p.device)
                               for what, t, s in zip(("surf", "band", "refrows"), out, shapes))
    ws = torch.empty(boundary_workspace_bytes(n, k, h, w) // 4, dtype=torch.int32, device=p.device)
    _boundary_stats_op(p, g, k, int(ignore_index), cap, radii, ws, surf, band if radii else None, refrows)
    return surf, band, refrows


# ---- signed distance maps and the boundary loss (sdf.hip) ----------------------------------
BOUNDARY_ACTIVATIONS = {"softmax": _lib.BOUNDARY_SOFTMAX, "sigmoid": _lib.BOUNDARY_SIGMOID}  # EUNET_BOUNDARY_*


def signed_distance_workspace_bytes(n, k, h, w):
    b = c_size_t()
    call("eunet_signed_distance_workspace_bytes", n, k, h, w, ctypes.byref(b))
    return b.value


@_dispatched("T i i f f T! T!")
def signed_distance(target, k, ignore_index, clip, scale, ws, out):
    n, h, w = target.shape
    # two transforms of k planes (distance_transform_sq's count), the combine pass (the target and two int32 planes in,
    # one fp32 plane out) and, for k = 1, the foreground plane written and read by both transforms' column passes
    nbytes = target.numel() * (2 * k * (8.0 + 4 * 4.0) + 8.0 + k * 12.0 + (8.0 if k == 1 else 0.0))
    with kprof.timed("signed_distance", 0.0, nbytes):
        call("eunet_signed_distance", _ptr(target), n, k, h, w, ignore_index, clip, scale, _ptr(ws), _ptr(out),
             _stream())


_signed_distance_op = signed_distance  # torch.ops.eunet.signed_distance writes into ws and out


def signed_distance_map(target, num_classes: int, ignore_index=None, clip=None, scale: float = 1.0, out=None):
    """target int64 [N,H,W] or [H,W] on the device -> float32 [N,K,H,W] (or [K,H,W]), K = num_classes in 1..3: per
    class the signed Euclidean distance to the class contour, +sqrt(Dout) outside the class and -(sqrt(Din) - 1)
    inside, 0 on a sample where the class or its complement is empty and on pixels equal to ignore_index (which
    belong to no class), then scale * clamp(phi, -clip, clip) (include/eunet.h, eunet_signed_distance).  K = 1: the
    class is target >= 1.  h, w <= 8192.  out: the buffer to write."""
    name = "signed_distance_map"
    if not isinstance(target, torch.Tensor):
        raise ValueError(f"{name}: target must be a tensor")
    if target.dtype != torch.int64:
        raise ValueError(f"{name}: target must be int64, got {target.dtype}")
    if target.dim() not in (2, 3):
        raise ValueError(f"{name}: target must be [H, W] or [N, H, W], got {tuple(target.shape)}")
    k = int(num_classes)
    if not 1 <= k <= 3:
        raise ValueError(f"{name}: num_classes must be 1..3, not {num_classes}")
    if clip is not None and not (math.isfinite(float(clip)) and float(clip) > 0.0):
        raise ValueError(f"{name}: clip must be None or a finite value > 0, got {clip}")
    if not math.isfinite(float(scale)):
        raise ValueError(f"{name}: scale must be finite, got {scale}")
    ign = -(2 ** 31) if ignore_index is None else int(ignore_index)  # EUNET_NO_IGNORE
    if not -2 ** 31 <= ign < 2 ** 31:
        raise ValueError(f"{name}: ignore_index {ignore_index} is not an int32")
    if k >= 2 and 0 <= ign < k:
        raise ValueError(f"{name}: ignore_index {ign} is one of the {k} classes")
    t, single = _int64_maps(name, "target", target)
    n, h, w = t.shape
    shape = (k, h, w) if single else (n, k, h, w)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=t.device)
    else:
        _out_buffer(name, "", out, shape, torch.float32, t.device)
    ws = torch.empty(signed_distance_workspace_bytes(n, k, h, w) // 4, dtype=torch.int32, device=t.device)
    _signed_distance_op(t, k, ign, 0.0 if clip is None else float(clip), float(scale), ws, out)
    return out


def boundary_loss_workspace_bytes(n, h, w):
    b = c_size_t()
    call("eunet_boundary_loss_workspace_bytes", n, h, w, ctypes.byref(b))
    return b.value


@_dispatched("T T i f f f T! T!? T!")
def boundary_loss_fwd(logits, dist, activation, cw0, cw1, cw2, loss, parts, ws):
    """torch.ops.eunet.boundary_loss_fwd: loss = sum w_c p_c dist_c / (N H W Kw), parts [N] per sample."""
    n, k, h, w = logits.shape
    cw = (_lib.c_float * 3)(cw0, cw1, cw2)
    with kprof.timed("boundary_loss_fwd", 0.0, 8.0 * logits.numel()):
        call("eunet_boundary_loss_fwd", _ptr(logits), _ptr(dist), n, k, h, w, activation, ctypes.byref(cw), _ptr(loss),
             _ptr(parts), _ptr(ws), _stream())


@_dispatched("T T i f f f T T!")
def boundary_loss_bwd(logits, dist, activation, cw0, cw1, cw2, gloss, glogits):
    """torch.ops.eunet.boundary_loss_bwd: glogits = gloss * d loss / d logits, one pass over logits and dist."""
    n, k, h, w = logits.shape
    cw = (_lib.c_float * 3)(cw0, cw1, cw2)
    with kprof.timed("boundary_loss_bwd", 0.0, 12.0 * logits.numel()):
        call("eunet_boundary_loss_bwd", _ptr(logits), _ptr(dist), n, k, h, w, activation, ctypes.byref(cw), _ptr(gloss),
             _ptr(glogits), _stream())


# ---- Lovasz losses (lovasz.hip; include/eunet.h, "Lovasz losses") -----------------------------
LOVASZ_ACTIVATIONS = {"softmax": _lib.LOVASZ_SOFTMAX, "hinge": _lib.LOVASZ_HINGE}  # EUNET_LOVASZ_*
_NO_IGNORE = -(2 ** 31)  # EUNET_NO_IGNORE


def lovasz_workspace_bytes(s, l):
    """The workspace of a call over s segments of l elements (a function of the shape alone)."""
    b = c_size_t()
    call("eunet_lovasz_workspace_bytes", s, l, ctypes.byref(b))
    return b.value


def lovasz_segments(n, k, h, w, per_image):
    """(S, L): K segments of N H W elements, or per image N K segments of H W."""
    return (n * k, h * w) if per_image else (k, n * h * w)


def _check_lovasz_args(logits, target, activation, ignore_index, what: str, more=None):
    """The rules of the Lovasz ops that need no launch, raised as ValueError; returns ignore_index as the int32 of the
    C ABI.  more(): the caller's own value rules, checked after the shapes and before the device."""
    if activation not in LOVASZ_ACTIVATIONS:
        raise ValueError(f"{what}: activation must be 'softmax' or 'hinge', not {activation!r}")
    if not isinstance(logits, torch.Tensor) or logits.dim() != 4:
        raise ValueError(f"{what}: expected [N, K, H, W] logits, got "
                         f"{tuple(logits.shape) if isinstance(logits, torch.Tensor) else type(logits).__name__}")
    if not isinstance(target, torch.Tensor):
        raise ValueError(f"{what}: target must be a tensor, got {type(target).__name__}")
    if logits.dtype != torch.float32:
        raise ValueError(f"{what}: logits must be float32, got {logits.dtype}")
    if target.dtype != torch.int64:
        raise ValueError(f"{what}: target must be int64, got {target.dtype}")
    n, k, h, w = logits.shape
    if tuple(target.shape) != (n, h, w):
        raise ValueError(f"{what}: target {tuple(target.shape)} does not match logits {tuple(logits.shape)}")
    if not (1 <= n <= 64 and 1 <= k <= 3 and h > 0 and w > 0 and h * w < 2 ** 31 - 1024 and n * h * w < 2 ** 31):
        raise ValueError(f"{what}: logits {tuple(logits.shape)} are outside the shape rule (N 1..64, K 1..3, H > 0, "
                         f"W > 0, H*W < 2^31 - 1024, N*H*W < 2^31)")
    if activation == "softmax" and k == 1:
        raise ValueError(f"{what}: a softmax over K = 1 is constant; use activation='hinge'")
    ign = _NO_IGNORE if ignore_index is None else int(ignore_index)
    if not -2 ** 31 <= ign < 2 ** 31:
        raise ValueError(f"{what}: ignore_index {ignore_index} is not an int32")
    if more is not None:
        more()
    if not logits.is_contiguous() or not target.is_contiguous():
        raise ValueError(f"{what}: logits and target must be contiguous")
    if not logits.is_cuda or target.device != logits.device:
        raise ValueError(f"{what}: logits and target must live on one GPU, got {logits.device} and {target.device}")
    return ign


@_dispatched("T T i i T! T!")
def lovasz_errors_op(logits, target, activation, ignore_index, errors, flags):
    """torch.ops.eunet.lovasz_errors_op: the errors and flags of every (pixel, class) into errors and flags."""
    n, k, h, w = logits.shape
    with kprof.timed("lovasz_errors", 0.0, 9.0 * logits.numel() + 8.0 * target.numel()):
        call("eunet_lovasz_errors", _ptr(logits), _ptr(target), n, k, h, w, activation, ignore_index, _ptr(errors),
             _ptr(flags), _stream())


def lovasz_errors(logits, target, activation, ignore_index=None):
    """logits float32 [N,K,H,W], target int64 [N,H,W] -> (errors float32 [N,K,H,W], flags uint8 [N,K,H,W]): per
    element the error of the Lovasz loss (softmax: |fg - p_c|; hinge: 1 - z_c (2 fg - 1)) and its flag, 0 background,
    1 foreground, 2 ignored or out of range (error 0)."""
    ign = _check_lovasz_args(logits, target, activation, ignore_index, "lovasz_errors")
    errors = torch.empty_like(logits)
    flags = torch.empty(logits.shape, dtype=torch.uint8, device=logits.device)
    lovasz_errors_op(logits, target, LOVASZ_ACTIVATIONS[activation], ign, errors, flags)
    return errors, flags


@_dispatched("T T T! T! T! T!")
def lovasz_sort_op(errors, flags, order, grad, counts, ws):
    s, l = errors.shape
    with kprof.timed("lovasz_sort", 0.0, 160.0 * errors.numel()):
        call("eunet_lovasz_sort", _ptr(errors), _ptr(flags), s, l, _ptr(order), _ptr(grad), _ptr(counts), _ptr(ws),
             _stream())


def lovasz_sort(errors, flags):
    """errors float32 [S,L], flags uint8 [S,L] (0 background, 1 foreground, >= 2 ignored) -> (order int32 [S,L], grad
    float32 [S,L], counts int64 [S,2]): per segment the stable descending order of the valid errors (ignored
    elements last, in index order), the Lovasz gradient g at every element's own index (0 where ignored), and
    (G, V), the foreground and valid counts."""
    name = "lovasz_sort"
    for what, t, dt in (("errors", errors, torch.float32), ("flags", flags, torch.uint8)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError(f"{name}: {what} must be a [S, L] tensor")
        if t.dtype != dt:
            raise ValueError(f"{name}: {what} must be {dt}, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: {what} must be contiguous")
    if errors.shape != flags.shape:
        raise ValueError(f"{name}: errors {tuple(errors.shape)} and flags {tuple(flags.shape)} differ in shape")
    s, l = errors.shape
    if not (1 <= s <= 65535 and 1 <= l < 2 ** 31):
        raise ValueError(f"{name}: S must be 1..65535 and L 1..2^31-1, got {s} x {l}")
    if not errors.is_cuda or flags.device != errors.device:
        raise ValueError(f"{name}: errors and flags must live on one GPU, got {errors.device} and {flags.device}")
    dev = errors.device
    order = torch.empty((s, l), dtype=torch.int32, device=dev)
    grad = torch.empty((s, l), dtype=torch.float32, device=dev)
    counts = torch.empty((s, 2), dtype=torch.int64, device=dev)
    ws = torch.empty(lovasz_workspace_bytes(s, l), dtype=torch.uint8, device=dev)
    lovasz_sort_op(errors, flags, order, grad, counts, ws)
    return order, grad, counts


@_dispatched("T T i b i i i T! T! T! T!? T!? T!? T!")
def lovasz_fwd(logits, target, activation, per_image, classes_mode, class_mask, ignore_index, weights, factor, loss,
               parts, counts, bad, ws):
    """torch.ops.eunet.lovasz_fwd: weights [N,K,H,W] = g at every element, factor [S] = the segments' shares of the
    mean, loss, parts [S], counts [S,2] = (G, V), bad [1] = the out-of-range targets."""
    n, k, h, w = logits.shape
    with kprof.timed("lovasz_fwd", 0.0, 170.0 * logits.numel()):
        call("eunet_lovasz_fwd", _ptr(logits), _ptr(target), n, k, h, w, activation, int(per_image), classes_mode,
             class_mask, ignore_index, _ptr(weights), _ptr(factor), _ptr(loss), _ptr(parts), _ptr(counts), _ptr(bad),
             _ptr(ws), _stream())


@_dispatched("T T i b T T T T!")
def lovasz_bwd(logits, target, activation, per_image, weights, factor, gloss, glogits):
    """torch.ops.eunet.lovasz_bwd: glogits = gloss * d loss / d logits from the forward's weights and factor."""
    n, k, h, w = logits.shape
    with kprof.timed("lovasz_bwd", 0.0, 12.0 * logits.numel() + 8.0 * target.numel()):
        call("eunet_lovasz_bwd", _ptr(logits), _ptr(target), n, k, h, w, activation, int(per_image), _ptr(weights),
             _ptr(factor), _ptr(gloss), _ptr(glogits), _stream())


# ---- overlap-tile inference (tiling.hip; the geometry is eunet.tiling.TilePlan) ----------
TILE_ACTIVATIONS = {"none": 0, "softmax": 1, "sigmoid": 2}  # EUNET_TILE_ACT_*


@_dispatched("T i i i i i i i i T!")
def tile_gather(image, hp, wp, th, tw, sy, sx, first, count, out):
    c, h, w = image.shape
    with kprof.timed("tile_gather", 0.0, 8.0 * out.numel()):
        call("eunet_tile_gather", _ptr(image), c, h, w, hp, wp, th, tw, sy, sx, first, count, _ptr(out), _stream())


_tile_gather_op = tile_gather  # torch.ops.eunet.tile_gather takes the geometry as integers and writes into out


def _plan_of(name, plan, h, w):
    if (plan.h, plan.w) != (h, w):
        raise ValueError(f"{name}: the plan is for a {plan.h} x {plan.w} image, not {h} x {w}")


def tile_gather(image, plan, first: int = 0, count: int | None = None, out=None):
    """image [C, h, w] fp32 (C = 1..4) -> tiles [count, C, th, tw]: tile numbers first .. first + count - 1 of
    plan (eunet.tiling.plan) cut from the image as reflect-padded to plan.hp x plan.wp; no padded copy is made."""
    if image.dim() != 3:
        raise ValueError(f"tile_gather: image must be [C, h, w], got {tuple(image.shape)}")
    image = image.contiguous().float()
    c, h, w = image.shape
    _plan_of("tile_gather", plan, h, w)
    count = plan.n - first if count is None else int(count)
    if first < 0 or count < 1 or first + count > plan.n:
        raise ValueError(f"tile_gather: tiles {first} .. {first + count - 1} are not inside the plan's {plan.n}")
    shape = (count, c, plan.th, plan.tw)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=image.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"tile_gather: out must be a contiguous fp32 {shape}, got {tuple(out.shape)} {out.dtype}")
    _tile_gather_op(image, plan.hp, plan.wp, plan.th, plan.tw, plan.stride, plan.stride, int(first), count, out)
    return out


@_dispatched("T i i i i i i i i i i T? T? i b b T!")
def tile_blend(logits, h, w, hp, wp, th, tw, sy, sx, mode, margin, wy, wx, activation, flip_h, flip_w, out):
    k = logits.shape[1]
    # per output pixel: K floats written, and K floats read per covering tile (logits.numel() in all)
    with kprof.timed("tile_blend", 0.0, 4.0 * (logits.numel() + out.numel())):
        call("eunet_tile_blend", _ptr(logits), k, h, w, hp, wp, th, tw, sy, sx, mode, margin, _ptr(wy), _ptr(wx),
             activation, int(flip_h), int(flip_w), _ptr(out), _stream())


_tile_blend_op = tile_blend
_tile_tables: dict = {}  # (device, th, tw, sigma_scale) -> the gaussian tables (wy, wx) on that device


def _gauss_tables(plan, device):
    key = (str(device), plan.th, plan.tw, plan.sigma_scale)
    if key not in _tile_tables:
        if len(_tile_tables) >= 16:
            _tile_tables.clear()
        _tile_tables[key] = tuple(torch.from_numpy(plan.table(a)).to(device) for a in (0, 1))
    return _tile_tables[key]


def tile_blend(logits, plan, activation: str = "softmax", flip_h=False, flip_w=False, out=None):
    """tile logits [plan.n, K, th, tw] fp32 (K = 1..3) -> probs [K, h, w]: per pixel the weighted mean, over
    the tiles that cover it in increasing tile number, of activation ('softmax' over K, 'sigmoid' or 'none')
    of the tile's logits, with plan.blend's weights; cropped to h x w, softmax_crop's flips on the destination."""
    if activation not in TILE_ACTIVATIONS:
        raise ValueError(f"tile_blend: activation must be one of {tuple(TILE_ACTIVATIONS)}, not {activation!r}")
    if logits.dim() != 4 or tuple(logits.shape[2:]) != (plan.th, plan.tw) or logits.shape[0] != plan.n:
        raise ValueError(f"tile_blend: logits must be [{plan.n}, K, {plan.th}, {plan.tw}], got {tuple(logits.shape)}")
    logits = logits.contiguous().float()
    k = logits.shape[1]
    shape = (k, plan.h, plan.w)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=logits.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"tile_blend: out must be a contiguous fp32 {shape}, got {tuple(out.shape)} {out.dtype}")
    wy, wx = _gauss_tables(plan, logits.device) if plan.blend == "gaussian" else (None, None)
    _tile_blend_op(logits, plan.h, plan.w, plan.hp, plan.wp, plan.th, plan.tw, plan.stride, plan.stride, plan.mode,
                   plan.margin, wy, wx, TILE_ACTIVATIONS[activation], bool(flip_h), bool(flip_w), out)
    return out


# ---- instance-level evaluation (instances.hip) -----------------------------------------
MORPH_ELEMS = {2: 0, 3: 1, 5: 2}  # side of cv2.getStructuringElement(MORPH_ELLIPSE, (k, k)) -> eunet_morph_u8 elem


def _u8(t):
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.dtype != torch.uint8:
        raise _lib.EunetError(f"instance ops take uint8 masks, got {t.dtype}")
    return t.contiguous()


def pack_masks(masks):
    """masks uint8 [n, h, w] (non-zero = set) -> (packed int64 [n, ceil(hw/64)] holding the 64-bit words,
    areas int64 [n])."""
    masks = _u8(masks)
    n, h, w = masks.shape
    words = (h * w + 63) // 64
    packed = torch.empty(n, words, dtype=torch.int64, device=masks.device)
    areas = torch.empty(n, dtype=torch.int64, device=masks.device)
    call("eunet_pack_masks", _ptr(masks), n, h, w, _ptr(packed), _ptr(areas), _stream())
    return packed, areas


def pack_masks_bbox(masks):
    """pack_masks plus, from the same pass, bbox int32 [n, 4] = (xmin, ymin, xmax, ymax), inclusive, of the
    set pixels; an empty mask gives (w, h, -1, -1)."""
    masks = _u8(masks)
    n, h, w = masks.shape
    words = (h * w + 63) // 64
    packed = torch.empty(n, words, dtype=torch.int64, device=masks.device)
    areas = torch.empty(n, dtype=torch.int64, device=masks.device)
    bbox = torch.empty(n, 4, dtype=torch.int32, device=masks.device)
    call("eunet_pack_masks_bbox", _ptr(masks), n, h, w, _ptr(packed), _ptr(areas), _ptr(bbox), _stream())
    return packed, areas, bbox


def coco_match(inter, area_d, area_g, box_d, box_g, cls_d, cls_g, thrs):
    """COCOeval.evaluateImg's greedy matching of one image on the device (eunet_coco_match): inter int64
    [D, G], areas int64, boxes int32 [., 4] as (x, y, w, h), classes int32 in {0, 1}, detections in visiting
    order; thrs a host sequence of floats.  -> match int32 [2, T, D] (0 bbox, 1 segm): the index of the ground
    truth each detection takes, or -1.  D, G >= 1 (the caller handles the empty sides without a launch)."""
    d, g = inter.shape
    t = len(thrs)

    def dev(x, dtype, shape):
        if x.dtype != dtype or tuple(x.shape) != shape:
            raise _lib.EunetError(f"coco_match: expected {dtype} {shape}, got {x.dtype} {tuple(x.shape)}")
        return x.contiguous()

    inter = dev(inter, torch.int64, (d, g))
    area_d, area_g = dev(area_d, torch.int64, (d,)), dev(area_g, torch.int64, (g,))
    box_d, box_g = dev(box_d, torch.int32, (d, 4)), dev(box_g, torch.int32, (g, 4))
    cls_d, cls_g = dev(cls_d, torch.int32, (d,)), dev(cls_g, torch.int32, (g,))
    th = (ctypes.c_double * max(t, 1))(*[float(v) for v in thrs])
    match = torch.empty(2, t, d, dtype=torch.int32, device=inter.device)
    call("eunet_coco_match", _ptr(inter), _ptr(area_d), _ptr(area_g), _ptr(box_d), _ptr(box_g), _ptr(cls_d),
         _ptr(cls_g), d, g, th, t, _ptr(match), _stream())
    return match


def pairwise_overlap(pa, pb):
    """packed [P, words] x packed [G, words] -> inter int64 [P, G] = |a & b| per pair."""
    if pa.shape[1] != pb.shape[1]:
        raise ValueError(f"packed widths differ: {pa.shape[1]} vs {pb.shape[1]}")
    inter = torch.empty(pa.shape[0], pb.shape[0], dtype=torch.int64, device=pa.device)
    call("eunet_pairwise_overlap", _ptr(pa.contiguous()), pa.shape[0], _ptr(pb.contiguous()), pb.shape[0],
         pa.shape[1], _ptr(inter), _stream())
    return inter


def morph_u8(img, ksize: int, dilate: bool, iterations: int = 1):
    """cv2.erode / cv2.dilate of a uint8 [h, w] image by the MORPH_ELLIPSE element of side ksize (2, 3, 5)."""
    img = _u8(img)
    h, w = img.shape
    out = torch.empty_like(img)
    tmp = torch.empty_like(img) if iterations > 1 else None
    call("eunet_morph_u8", _ptr(img), _ptr(out), _ptr(tmp), h, w, MORPH_ELEMS[ksize], int(dilate), int(iterations),
         _stream())
    return out


def label_components(img, connectivity: int = 8):
    """Connected components of a uint8 [h, w] image -> (labels int32 [h, w], n, areas int32 [n] on the device);
    numbered 1..n in raster order of each component's first pixel.  connectivity 8 (skimage.measure.label's
    connectivity=2) or 4 (scipy.ndimage.label's default).  Synchronises to read n."""
    if connectivity not in (4, 8):
        raise ValueError(f"label_components: connectivity must be 4 or 8, got {connectivity!r}")
    img = _u8(img)
    h, w = img.shape
    nbytes = c_size_t()
    call("eunet_label_workspace_bytes", h, w, ctypes.byref(nbytes))
    cap = ((h + 1) // 2) * ((w + 1) // 2) if connectivity == 8 else (h * w + 1) // 2
    labels = torch.empty(h, w, dtype=torch.int32, device=img.device)
    ws = torch.empty(nbytes.value // 4, dtype=torch.int32, device=img.device)
    areas = torch.empty(cap + 1, dtype=torch.int32, device=img.device)  # [cap] holds n
    if connectivity == 8:
        call("eunet_label_components", _ptr(img), h, w, _ptr(labels), _ptr(areas[cap:]), _ptr(areas), cap, _ptr(ws),
             _stream())
    else:
        call("eunet_label_components_conn", _ptr(img), h, w, _ptr(labels), _ptr(areas[cap:]), _ptr(areas), cap,
             _ptr(ws), 4, _stream())
    n = int(areas[cap].item())
    return labels, n, areas[:n]


def outer_perimeter(labels, n: int):
    """Per label 1..n of an int32 [h, w] label map: stats int32 [n, 8] = (axis steps, diagonal steps, area,
    start pixel, x0, y0, x1, y1) of the outer border of the label's chosen component."""
    if labels.dtype != torch.int32:
        raise _lib.EunetError("outer_perimeter: int32 label map")
    labels = labels.contiguous()
    h, w = labels.shape
    stats = torch.empty(n, 8, dtype=torch.int32, device=labels.device)
    ws = torch.empty(h * w, dtype=torch.int32, device=labels.device)
    call("eunet_outer_perimeter", _ptr(labels), h, w, n, _ptr(stats), _ptr(ws), _stream())
    return stats


def mask_eq(src, value: int):
    """(src == value) as uint8 0/1 of an int32 / int64 tensor, and the device int64 [1] count of ones."""
    if src.dtype not in (torch.int32, torch.int64):
        raise _lib.EunetError(f"mask_eq: int32 or int64 source, got {src.dtype}")
    src = src.contiguous()
    dst = torch.empty(src.shape, dtype=torch.uint8, device=src.device)
    count = torch.empty(1, dtype=torch.int64, device=src.device)
    call("eunet_mask_eq", _ptr(src), src.element_size(), src.numel(), int(value), _ptr(dst), _ptr(count), _stream())
    return dst, count


def mask_and(a, b):
    """(a != 0) & (b != 0) as uint8 0/1, and the device int64 [1] count of ones."""
    a, b = _u8(a), _u8(b)
    dst = torch.empty_like(a)
    count = torch.empty(1, dtype=torch.int64, device=a.device)
    call("eunet_mask_and", _ptr(a), _ptr(b), a.numel(), _ptr(dst), _ptr(count), _stream())
    return dst, count


def write_label(mask, label: int, markers):
    """markers[mask != 0] = label, in place (int32 markers)."""
    call("eunet_write_label", _ptr(_u8(mask)), markers.numel(), int(label), _ptr(markers), _stream())


def relabel_table(labels, table, markers):
    """markers[i] = table[labels[i] - 1] where that entry is > 0, in place (int32 everywhere)."""
    call("eunet_relabel_table", _ptr(labels), labels.numel(), _ptr(table), table.numel(), _ptr(markers), _stream())


def expand_labels(labels, table, m: int):
    """uint8 [m, h, w]: plane table[l - 1] is the mask of label l (entries < 0 are dropped)."""
    out = torch.empty(m, *labels.shape, dtype=torch.uint8, device=labels.device)
    call("eunet_expand_labels", _ptr(labels), labels.numel(), _ptr(table), table.numel(), m, _ptr(out), _stream())
    return out


# ---- distance-transform watershed (watershed.hip) ---------------------------------------------
def merge_basins(peak, root, offs, a, b, saddle, depth: float):
    """The host half of the watershed (include/eunet.h, "distance-transform watershed"), over the basin graph of all
    planes at once: peak / root int arrays [nb] (D at, and plane index of, each basin's root; the basins of plane q
    are the slots offs[q] .. offs[q + 1] - 1, in raster order of their first pixel), edges (a[e], b[e]) with
    saddle[e].  The edges are visited by (-saddle, smaller root, larger root); the set whose representative (its
    member root of largest key (D, -index)) has the smaller key joins the other when sqrt(its peak) -
    sqrt(saddle) < depth.  Returns (table int32 [nb]: the final id of every basin, 1..m per plane in raster order
    of each set's first pixel; m int64 [p])."""
    import math

    import numpy as np
    peak, root = np.asarray(peak, np.int64), np.asarray(root, np.int64)
    a, b, saddle = np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(saddle, np.int64)
    nb = len(peak)
    par = list(range(nb))

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x

    if len(a):
        ra, rb = root[a], root[b]
        # edges of different planes never share a set, so their mutual order is free; within a plane this is the
        # order of the definition (the slot breaks the ties between planes, to keep the order total)
        order = np.lexsort((a, np.maximum(ra, rb), np.minimum(ra, rb), -saddle))
        pk, rt = peak.tolist(), root.tolist()
        ea, eb, es = a.tolist(), b.tolist(), saddle.tolist()
        for e in order.tolist():
            x, y = find(ea[e]), find(eb[e])
            if x == y:
                continue
            lo, hi = (x, y) if (pk[x], -rt[x]) < (pk[y], -rt[y]) else (y, x)
            if math.sqrt(pk[lo]) - math.sqrt(es[e]) < depth:
                par[lo] = hi
    table = np.zeros(nb, np.int32)
    m = np.zeros(len(offs) - 1, np.int64)
    for q in range(len(offs) - 1):
        seen, nxt = {}, 0
        for g in range(int(offs[q]), int(offs[q + 1])):  # ascending first pixel: a set is met at its first pixel
            r = find(g)
            t = seen.get(r)
            if t is None:
                nxt += 1
                seen[r] = t = nxt
            table[g] = t
        m[q] = nxt
    return table, m


def _watershed_depth(name, depth):
    try:
        d = float(depth)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: depth must be a number of pixels, got {depth!r}") from None
    if d != d or d < 0.0:
        raise ValueError(f"{name}: depth must be >= 0 (inf allowed), got {depth!r}")
    return d


def watershed_from_distance(dist_sq, depth: float = 1.0, out=None, _table_capacity=None):
    """dist_sq int32 [h, w] or [p, h, w] of squared distances (foreground: > 0; what distance_transform_sq gives in
    mode "ne") -> (ids int32 of the same shape, counts int64 [p] on the device, areas int32 [p, max(counts)] on the
    device, zero past a plane's count; [max] for an [h, w] input): the basins of each plane, those merged whose
    peak stands less than `depth` pixels above the saddle to a higher neighbour, numbered 1..counts[plane] in raster
    order of each region's first pixel, background 0 (include/eunet.h, "distance-transform watershed"; depth 0: every
    basin, inf: the 8-connected components).  The basin graph is merged on the host (merge_basins): the call
    synchronises.  out: the ids buffer to write.  _table_capacity: the first size of the saddle hash table (a power
    of two; it is doubled until every pair fits), for tests."""
    import numpy as np
    name = "watershed_from_distance"
    _id_maps(name, "dist_sq", dist_sq, (torch.int32,))
    single = dist_sq.dim() == 2
    d = dist_sq.unsqueeze(0) if single else dist_sq
    p, h, w = _plane_shape(name, "dist_sq", dist_sq.shape, True, verb="is")
    depth = _watershed_depth(name, depth)
    cap = _table_cap(name, _table_capacity)
    dev = d.device
    if out is None:
        ids = torch.empty(tuple(dist_sq.shape), dtype=torch.int32, device=dev)
    else:
        ids = _out_buffer(name, "", out, tuple(dist_sq.shape), torch.int32, dev)
        if ids.data_ptr() == dist_sq.data_ptr():
            raise ValueError(f"{name}: out must not be dist_sq")
    hw = h * w
    nbytes = c_size_t()
    call("eunet_watershed_workspace_bytes", p, h, w, ctypes.byref(nbytes))
    ws = torch.empty(nbytes.value // 4, dtype=torch.int32, device=dev)
    counts32 = torch.empty(p, dtype=torch.int32, device=dev)
    # up reads the plane and writes the parents; a jump round reads and writes them; first / count / rank / fill
    # read roots and firsts and write the basins
    with kprof.timed("watershed_basins", 0.0, p * hw * 4.0 * 12):
        call("eunet_watershed_basins", _ptr(d), p, h, w, _ptr(ids), _ptr(counts32), _ptr(ws), _stream())
    nb = counts32.cpu().numpy().astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(nb)])
    nb_total = int(offs[-1])
    if nb_total == 0:  # no foreground anywhere: the basin map is all background already
        areas = torch.zeros((0,) if single else (p, 0), dtype=torch.int32, device=dev)
        return ids, torch.zeros(p, dtype=torch.int64, device=dev), areas
    offs_d = upload(offs[:-1].astype(np.int32), dev)
    rootpeak = torch.empty(2, nb_total, dtype=torch.int32, device=dev)
    with kprof.timed("watershed_peaks", 0.0, p * hw * 4.0):
        call("eunet_watershed_peaks", _ptr(d), _ptr(ids), _ptr(ws), p, h, w, _ptr(offs_d), nb_total, _ptr(rootpeak[0]),
             _ptr(rootpeak[1]), _stream())
    if cap is None:  # about 2.5 pairs per basin at most on noise; 8 slots per basin keep the probes short
        cap = 64
        while cap < 8 * nb_total:
            cap *= 2

    def saddles(cap):
        keys = torch.empty(cap, dtype=torch.int64, device=dev)
        vals = torch.empty(cap + 1, dtype=torch.int32, device=dev)  # [cap]: the overflow count
        with kprof.timed("watershed_saddles", 0.0, p * hw * 4.0 * 10):
            call("eunet_watershed_saddles", _ptr(d), _ptr(ids), p, h, w, _ptr(offs_d), _ptr(keys), _ptr(vals), cap,
                 _ptr(vals[cap:]), _stream())
        v = vals.cpu().numpy()
        return v[cap], (keys, v)

    cap, (keys, v) = _fill_table(name, "saddle", cap, saddles)
    k = keys.cpu().numpy()
    used = k != -1
    rp = rootpeak.cpu().numpy()
    table, m = merge_basins(rp[1], rp[0], offs, k[used] >> 32, k[used] & 0xffffffff, v[:cap][used], depth)
    amax = int(m.max())
    areas = torch.empty(p, amax, dtype=torch.int32, device=dev)
    with kprof.timed("watershed_relabel", 0.0, p * hw * 4.0 * 2):
        call("eunet_watershed_relabel", _ptr(ids), p, h, w, _ptr(offs_d), _ptr(upload(table, dev)), nb_total, _ptr(ids),
             _ptr(areas), amax, _stream())
    return ids, upload(m, dev), areas[0] if single else areas


def watershed_split(labels, values, depth: float = 1.0, out=None):
    """labels int64 [n, h, w] or [h, w], values 1..8 integers -> (ids int32 [n, nv, h, w] (or [nv, h, w]), counts int64
    [n, nv] (or [nv]), areas int32 [n, nv, max count] (or [nv, max count])): plane j splits the region labels ==
    values[j] of each sample along the ridges of its distance to the rest, distance_transform_sq(labels, values,
    "ne") followed by watershed_from_distance.  out: the ids buffer to write."""
    name = "watershed_split"
    depth = _watershed_depth(name, depth)
    t, single = _int64_maps(name, "labels", labels)
    vals = _int_list(name, "values", values, -2 ** 63, 2 ** 63 - 1, 1, _lib.EDT_MAX_VALUES)
    n, h, w = t.shape
    nv = len(vals)
    if n * nv > 65535 or n * nv * h * w >= 2 ** 31:
        raise ValueError(f"{name}: {n} x {nv} planes of {h} x {w} exceed 65535 planes or 2^31 pixels")
    shape = (nv, h, w) if single else (n, nv, h, w)
    if out is not None:
        _out_buffer(name, "", out, shape, torch.int32, t.device)
    dist = distance_transform_sq(t, vals, "ne")
    ids, counts, areas = watershed_from_distance(dist.view(n * nv, h, w), depth,
                                                 out=None if out is None else out.view(n * nv, h, w))
    ids = ids.view(shape) if out is None else out
    if single:
        return ids, counts, areas
    return ids, counts.view(n, nv), areas.view(n, nv, areas.shape[-1])


# ---- label-map instance metrics (pairs.hip) -----------------------------------------------------
PAIRS_FIRST_CAPACITY = 4096
PAIRS_MAX_ID = _lib.PAIRS_MAX_ID  # the largest id of a map


def _id_maps(name, what, t, dtypes=(torch.int32, torch.int64)):
    """t as a contiguous [h, w] or [p, h, w] device map of one of the dtypes."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: {what} must be a tensor")
    if not t.is_cuda:
        raise ValueError(f"{name}: {what} must live on a GPU, got {t.device}")
    if t.dtype not in dtypes:
        raise ValueError(f"{name}: {what} must be {' or '.join(str(d)[6:] for d in dtypes)}, got {t.dtype}")
    if t.dim() not in (2, 3):
        raise ValueError(f"{name}: {what} must be [h, w] or [p, h, w], got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: {what} must be contiguous")
    return t


def label_pairs(a, b, _table_capacity=None):
    """The sparse contingency table of two label maps (include/eunet.h, "label-map instance metrics"): a and b are
    [h, w] or [p, h, w] device tensors of equal shape, int32 or int64 each, contiguous -> numpy int64 [m, 4] of rows
    (plane, a, b, n) sorted lexicographically: n pixels of the plane carry id a in the first map and id b in the
    second.  Pixels that are background (0) in both maps are left out, pixels with a negative id in either are
    ignored.  Ids reach 2^24 - 1; a larger one raises ValueError.  The table is read back: the call synchronises.
    _table_capacity: the first size of the hash table (a power of two; it is doubled until every pair fits), for
    tests."""
    import numpy as np
    name = "label_pairs"
    a, b = _id_maps(name, "a", a), _id_maps(name, "b", b)
    if a.shape != b.shape:
        raise ValueError(f"{name}: the maps differ in shape: {tuple(a.shape)} vs {tuple(b.shape)}")
    if a.device != b.device:
        raise ValueError(f"{name}: the maps live on different devices: {a.device} vs {b.device}")
    p, h, w = _plane_shape(name, "maps", a.shape, True)
    cap = _table_cap(name, _table_capacity) or PAIRS_FIRST_CAPACITY
    dev = a.device
    nbytes = float(p * h * w * (a.element_size() + b.element_size()))

    def pairs(cap):
        # one int64 buffer: the keys, then [cap] the invalid count, then the int32 counts and [cap] the overflow
        buf = torch.empty(cap + 1 + (cap + 2) // 2, dtype=torch.int64, device=dev)
        vals = buf[cap + 1:].view(torch.int32)
        with kprof.timed("label_pairs", 0.0, nbytes):
            call("eunet_label_pairs", _ptr(a), a.element_size(), _ptr(b), b.element_size(), p, h, w, _ptr(buf), _ptr(vals),
                 cap, _ptr(vals[cap:]), _ptr(buf[cap:]), _stream())
        host = buf.cpu().numpy()  # the one copy to the host
        k, invalid = host[:cap], int(host[cap])
        v = host[cap + 1:].view(np.int32)
        if invalid:
            raise ValueError(f"{name}: {invalid} pixel(s) hold an id above 2^24 - 1")
        return v[cap], (k, v)

    cap, (k, v) = _fill_table(name, "pair", cap, pairs)
    used = k != -1
    k, n = k[used].view(np.uint64), v[:cap][used].astype(np.int64)  # unsigned: a plane above 32767 sets the top bit
    order = np.argsort(k, kind="stable")  # plane, a, b are the key's fields from the top: key order is row order
    k, n = k[order], n[order]
    mask = np.uint64(_lib.PAIRS_MAX_ID)
    fields = [k >> np.uint64(48), (k >> np.uint64(24)) & mask, k & mask]
    return np.stack([f.astype(np.int64) for f in fields] + [n], axis=1).reshape(-1, 4)


def labels_from_stack(masks, ids, ignore=None):
    """masks uint8 (or bool) [n, h, w] on the device (non-zero = set), ids n integers (a sequence or an int32 device
    tensor), ignore None or a uint8 / bool [h, w] device mask -> (labels int32 [h, w] on the device, overlap int):
    labels[i] = ids[j] for the largest j with masks[j][i] set and ids[j] > 0, 0 where there is none, -1 where ignore
    is set; overlap = the pixels that more than one selected plane claims.  n may be 0.  Synchronises to read
    overlap."""
    import numpy as np
    name = "labels_from_stack"
    if not isinstance(masks, torch.Tensor) or not masks.is_cuda or masks.dim() != 3 or \
            masks.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"{name}: masks must be a uint8 or bool [n, h, w] device tensor")
    masks = _u8(masks)
    n, h, w = masks.shape
    if not (0 <= n <= 65535 and h >= 1 and w >= 1 and h * w < 2 ** 31):
        raise ValueError(f"{name}: masks {tuple(masks.shape)} are outside n 0..65535, h w < 2^31")
    dev = masks.device
    if isinstance(ids, torch.Tensor):
        if ids.dtype != torch.int32 or ids.device != dev or tuple(ids.shape) != (n,):
            raise ValueError(f"{name}: ids must be an int32 [{n}] tensor on {dev}")
        ids_d = ids.contiguous()
    else:
        ids_h = _int_list(name, "ids", ids, -2 ** 31, 2 ** 31 - 1, n, n)
        ids_d = upload(np.asarray(ids_h, np.int32), dev) if n else None
    if ignore is not None:
        if not isinstance(ignore, torch.Tensor) or ignore.device != dev or tuple(ignore.shape) != (h, w) or \
                ignore.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"{name}: ignore must be a uint8 or bool [{h}, {w}] tensor on {dev}")
        ignore = _u8(ignore)
    out = torch.empty(h, w, dtype=torch.int32, device=dev)
    overlap = torch.empty(1, dtype=torch.int64, device=dev)
    with kprof.timed("labels_from_stack", 0.0, float(h * w * (n + 4 + (ignore is not None)))):
        call("eunet_labels_from_stack", _ptr(masks) if n else None, n, h, w, _ptr(ids_d) if n else None,
             None if ignore is None else _ptr(ignore), _ptr(out), _ptr(overlap), _stream())
    return out, int(overlap.item())


# ---- per-cell measurements (cellprops.hip) -------------------------------------------------------
CELL_GEOM_COLS = _lib.CELL_GEOM_COLS


def cell_stats(ids, n: int, image=None):
    """The integer sums of every label 1..n of a label map (include/eunet.h, "per-cell measurements"): ids [h, w] or
    [p, h, w], int32 or int64, contiguous, on the device; image None or a contiguous uint8 [h, w] / [h, w, c] (c <= 3)
    device tensor of the same device, shared by the planes -> {"geom": numpy int64 [p, n + 1, 14] (area, sum x, sum y,
    sum x^2, sum y^2, sum x y, x0, y0, x1, y1, q1, q2, q3, qd; row 0 zero; a label with no pixel has the box w, h, -1,
    -1), "intensity": numpy int64 [p, n + 1, c, 4] (sum, sum of squares, min, max per channel; 255 / 0 for a label
    with no pixel) or None without an image, "skipped": numpy int64 [p], the pixels whose id is negative or above n
    (measured nowhere), "shape": (h, w)}.  n may be 0.  The tables come back in one copy: the call synchronises.
    metrics.cell_measurements forms the descriptors."""
    import operator
    name = "cell_stats"
    ids = _id_maps(name, "ids", ids)
    p, h, w = _plane_shape(name, "ids", ids.shape, False)
    try:
        n = operator.index(n)
    except TypeError:
        raise ValueError(f"{name}: n must be an integer, got {n!r}") from None
    if not 0 <= n <= _lib.PAIRS_MAX_ID:
        raise ValueError(f"{name}: n must lie in 0..{_lib.PAIRS_MAX_ID}, got {n}")
    c = 0
    if image is not None:
        if not isinstance(image, torch.Tensor):
            raise ValueError(f"{name}: image must be a tensor")
        if image.dtype != torch.uint8:
            raise ValueError(f"{name}: image must be uint8, got {image.dtype}")
        if image.device != ids.device:
            raise ValueError(f"{name}: image lives on {image.device}, the ids on {ids.device}")
        if image.dim() not in (2, 3) or tuple(image.shape[:2]) != (h, w) or (image.dim() == 3 and
                                                                              not 1 <= image.shape[2] <= 3):
            raise ValueError(f"{name}: image must be [{h}, {w}] or [{h}, {w}, c] with c in 1..3, got "
                             f"{tuple(image.shape)}")
        if not image.is_contiguous():
            raise ValueError(f"{name}: image must be contiguous")
        c = 1 if image.dim() == 2 else int(image.shape[2])
    rows = p * (n + 1)
    cuts = (rows * CELL_GEOM_COLS, rows * (CELL_GEOM_COLS + 4 * c))
    buf = torch.empty(cuts[1] + p, dtype=torch.int64, device=ids.device)  # geom, intensity, skipped: one copy back
    with kprof.timed("cell_stats", 0.0, float(2 * p * h * w * ids.element_size() + p * h * w * c + 16 * buf.numel())):
        call("eunet_cell_stats", _ptr(ids), ids.element_size(), p, h, w, n, None if image is None else _ptr(image), c,
             _ptr(buf), _ptr(buf[cuts[0]:]) if c else None, _ptr(buf[cuts[1]:]), _stream())
    host = buf.cpu().numpy()
    return {"geom": host[:cuts[0]].reshape(p, n + 1, CELL_GEOM_COLS),
            "intensity": host[cuts[0]:cuts[1]].reshape(p, n + 1, c, 4) if c else None,
            "skipped": host[cuts[1]:], "shape": (h, w)}


# ---- per-cell convex hulls (hull.hip) --------------------------------------------------------------
CELL_HULL_COLS = _lib.CELL_HULL_COLS


def cell_hulls(ids, stats):
    """The convex hull of every label 1..n of a label map (include/eunet.h, "per-cell convex hulls"): ids as for
    cell_stats, stats the dict cell_stats(ids, n, ...) returned for the same ids (n = geom.shape[1] - 1; its bounding
    boxes give the row layout) -> {"hull": numpy int64 [p, n + 1, 11] (vertex count, twice the hull's area, the
    perimeter in 2^-16 pixels, the largest squared vertex distance and its pair xa, ya, xb, yb, the minimum width's
    numerator c and its edge dx, dy; all zero for a label with no pixel), "verts": per plane a list of n int32
    [nv_i, 2] arrays of (x, y), label i at index i - 1, in the header's order, "ext": numpy int32 [R, 2], per label and
    row of its box the smallest and largest x, (w, -1) for a row without a pixel, "row_off": numpy int64
    [p (n + 1) + 1], the first row of every label in ext, "shape": (h, w)}.  Stats that do not belong to these ids
    raise ValueError: nothing is stored outside the tables.  The tables come back in one copy: the call synchronises.
    metrics.hull_measurements forms the descriptors."""
    import numpy as np
    name = "cell_hulls"
    ids = _id_maps(name, "ids", ids)
    p, h, w = _plane_shape(name, "ids", ids.shape, False)
    if not isinstance(stats, dict) or "geom" not in stats or "shape" not in stats:
        raise ValueError(f"{name}: stats must be cell_stats' dict (\"geom\", \"shape\")")
    if tuple(int(v) for v in stats["shape"]) != (h, w):
        raise ValueError(f"{name}: the stats are of a {tuple(stats['shape'])} map, the ids are {(h, w)}")
    geom = np.asarray(stats["geom"])
    if geom.dtype != np.int64 or geom.ndim != 3 or geom.shape[0] != p or geom.shape[1] < 1 or \
            geom.shape[2] != CELL_GEOM_COLS:
        raise ValueError(f"{name}: geom must be int64 [{p}, n + 1, {CELL_GEOM_COLS}], got {geom.dtype} {geom.shape}")
    n = geom.shape[1] - 1
    if n > _lib.PAIRS_MAX_ID:
        raise ValueError(f"{name}: n must lie in 0..{_lib.PAIRS_MAX_ID}, got {n}")
    L = p * (n + 1)
    y0, y1 = geom[:, :, 7].reshape(L), geom[:, :, 9].reshape(L)
    rows = np.where(np.arange(L) % (n + 1) == 0, 0, np.maximum(y1 - y0 + 1, 0))  # id 0 has no rows
    present = rows > 0
    if (present & ((y0 < 0) | (y1 >= h))).any():
        raise ValueError(f"{name}: a bounding box of the stats leaves the {h} rows of the map")
    row_off = np.zeros(L + 1, np.int64)
    np.cumsum(rows, out=row_off[1:])
    R = int(row_off[L])
    if R > _lib.CELL_HULL_MAX_ROWS:
        raise ValueError(f"{name}: the labels' boxes have {R} rows together, above 2^28")
    layout = np.zeros(L + 1 + (L + 1) // 2, np.int64)  # row_off, then row_y0 as int32: one upload
    layout[:L + 1] = row_off
    layout[L + 1:].view(np.int32)[:L] = np.where(present, y0, 0)
    layout_d = upload(layout, ids.device)
    cuts = np.cumsum([L * CELL_HULL_COLS, p, 2 * (R + L), R]).tolist()  # hull, outside, verts, ext in int64 words
    buf = torch.empty(cuts[3], dtype=torch.int64, device=ids.device)
    with kprof.timed(name, 0.0, float(p * h * w * ids.element_size() + 8 * buf.numel() + 8 * layout.size)):
        call("eunet_cell_hulls", _ptr(ids), ids.element_size(), p, h, w, n, _ptr(layout_d), _ptr(layout_d[L + 1:]),
             _ptr(buf[cuts[2]:]) if R else _ptr(buf), _ptr(buf[cuts[1]:]), _ptr(buf), _ptr(buf[cuts[0]:]), _stream())
    host = buf.cpu().numpy()  # the one copy to the host
    outside = host[cuts[0]:cuts[1]]
    if outside.any():
        raise ValueError(f"{name}: {int(outside.sum())} pixel(s) lie outside their label's rows: the stats are not "
                         "of these ids")
    hull = host[:cuts[0]].reshape(p, n + 1, CELL_HULL_COLS)
    slots = host[cuts[1]:cuts[2]].view(np.int32).reshape(-1, 2)
    start = 2 * (row_off[:L] + np.arange(L))
    nv = hull[:, :, 0].reshape(L)
    verts = [[slots[start[q * (n + 1) + i]:start[q * (n + 1) + i] + nv[q * (n + 1) + i]] for i in range(1, n + 1)]
             for q in range(p)]
    return {"hull": hull, "verts": verts, "ext": host[cuts[2]:].view(np.int32).reshape(R, 2), "row_off": row_off,
            "shape": (h, w)}


# ---- nearest-cell transform, label expansion and cell contacts (neighbors.hip) ----------------------
CONTACTS_FIRST_CAPACITY = 4096


def nearest_site(ids):
    """The feature transform of a label map (include/eunet.h, "nearest-cell transform, label expansion and cell
    contacts"): ids [h, w] or [p, h, w], int32 or int64, contiguous, on the device -> (dist, site), int32 tensors shaped
    as ids.  The sites of a plane are its pixels with id >= 1; dist is the exact squared Euclidean distance to the
    nearest site of the own plane and site that site's linear index y w + x, the smallest index among the sites at the
    minimum distance.  A plane without a site holds EDT_NONE and -1.  h, w <= 8192.  No synchronisation."""
    name = "nearest_site"
    ids = _id_maps(name, "ids", ids)
    p, h, w = _plane_shape(name, "ids", ids.shape, False)
    dist = torch.empty(ids.shape, dtype=torch.int32, device=ids.device)
    site = torch.empty(ids.shape, dtype=torch.int32, device=ids.device)
    # the column pass reads the ids and writes and re-reads the plane of rows; the row pass reads it and writes two
    with kprof.timed(name, 0.0, float(p * h * w * (ids.element_size() + 6 * 4))):
        call("eunet_nearest_site", _ptr(ids), ids.element_size(), p, h, w, _ptr(dist), _ptr(site), _stream())
    return dist, site


def expand_label_map(ids, distance=None, out=None):
    """skimage.segmentation.expand_labels with a stated tie rule (include/eunet.h, eunet_expand_label_map): ids as for
    nearest_site -> a tensor of ids' dtype and shape.  A pixel with an id other than 0 keeps it (negative "ignore"
    ids too, which are no sites and are never overwritten); a pixel with id 0 takes the id of nearest_site's site when
    its squared distance is <= floor(distance^2), and stays 0 otherwise.  distance None: no limit, the discrete
    Voronoi partition of every plane that has a label.  out: the buffer to write, not ids itself.  (ops.expand_labels
    is the instance unit's label map -> mask stack.)  No synchronisation."""
    import math
    name = "expand_label_map"
    ids = _id_maps(name, "ids", ids)
    p, h, w = _plane_shape(name, "ids", ids.shape, False)
    if distance is None:
        limit2 = -1
    else:
        try:
            d = float(distance)
        except (TypeError, ValueError):
            raise ValueError(f"{name}: distance must be None or a number, got {distance!r}") from None
        if math.isnan(d) or d < 0.0:
            raise ValueError(f"{name}: distance must be None or >= 0, got {distance!r}")
        # beyond the longest distance of an 8192 x 8192 map every limit is "no smaller than any distance"
        limit2 = int(math.floor(d * d)) if d < 2.0 ** 15 else 2 ** 31 - 2
    if out is None:
        out = torch.empty_like(ids)
    else:
        _out_buffer(name, "", out, ids.shape, ids.dtype, ids.device)
        if out.data_ptr() == ids.data_ptr():
            raise ValueError(f"{name}: out must not be ids itself")
    ws = torch.empty(ids.shape, dtype=torch.int32, device=ids.device)
    with kprof.timed(name, 0.0, float(p * h * w * (3 * ids.element_size() + 3 * 4))):
        call("eunet_expand_label_map", _ptr(ids), ids.element_size(), p, h, w, limit2, _ptr(ws), _ptr(out), _stream())
    return out


def label_contacts(ids, connectivity: int = 4, _table_capacity=None):
    """The sparse adjacency table of one label map (include/eunet.h, eunet_label_contacts): ids [h, w] or [p, h, w],
    int32 or int64, contiguous, on the device -> numpy int64 [m, 4] of rows (plane, a, b, n), a < b, sorted
    lexicographically: n adjacent pixel pairs of the plane carry the ids a and b.  connectivity 4 pairs a pixel with
    its right and lower neighbour (n = the unit pixel sides the two labels share), 8 also with the two lower diagonal
    ones.  Ids 0 and below take no part.  Ids reach 2^24 - 1; a larger one raises ValueError.  The table is read
    back: the call synchronises.  _table_capacity: the first size of the hash table (a power of two; it is doubled
    until every row fits), for tests."""
    import numpy as np
    name = "label_contacts"
    ids = _id_maps(name, "ids", ids)
    p, h, w = _plane_shape(name, "ids", ids.shape, False)
    if connectivity not in (4, 8):
        raise ValueError(f"{name}: connectivity must be 4 or 8, got {connectivity!r}")
    cap = _table_cap(name, _table_capacity) or CONTACTS_FIRST_CAPACITY
    dev = ids.device
    nbytes = float(p * h * w * ids.element_size())

    def contacts(cap):
        # one int64 buffer: the keys, then [cap] the invalid count, then the int32 counts and [cap] the overflow
        buf = torch.empty(cap + 1 + (cap + 2) // 2, dtype=torch.int64, device=dev)
        vals = buf[cap + 1:].view(torch.int32)
        with kprof.timed(name, 0.0, nbytes):
            call("eunet_label_contacts", _ptr(ids), ids.element_size(), p, h, w, int(connectivity), _ptr(buf),
                 _ptr(vals), cap, _ptr(vals[cap:]), _ptr(buf[cap:]), _stream())
        host = buf.cpu().numpy()  # the one copy to the host
        k, invalid = host[:cap], int(host[cap])
        v = host[cap + 1:].view(np.int32)
        if invalid:
            raise ValueError(f"{name}: {invalid} pixel(s) hold an id above 2^24 - 1")
        return v[cap], (k, v)

    cap, (k, v) = _fill_table(name, "contact", cap, contacts)
    used = k != -1
    k, n = k[used].view(np.uint64), v[:cap][used].astype(np.int64)  # unsigned: a plane above 32767 sets the top bit
    order = np.argsort(k, kind="stable")  # plane, a, b are the key's fields from the top: key order is row order
    k, n = k[order], n[order]
    mask = np.uint64(_lib.PAIRS_MAX_ID)
    fields = [k >> np.uint64(48), (k >> np.uint64(24)) & mask, k & mask]
    return np.stack([f.astype(np.int64) for f in fields] + [n], axis=1).reshape(-1, 4)


# ---- dual-branch fusion (fusion.hip) -------------------------------------------------
def fusion_tiles(n, h, w):
    t, gt = c_int(), c_int()
    call("eunet_fusion_tiles", n, h, w, ctypes.byref(t), ctypes.byref(gt))
    return t.value, gt.value


def gate_fwd(za, zb, k, w1, a, st1, aux_a, aux_b):
    n, h, w, _ = za.shape
    call("eunet_gate_fwd", _ptr(za), _ptr(zb), n, h, w, k, _ptr(w1), _ptr(a), _ptr(st1), _ptr(aux_a), _ptr(aux_b),
         _stream())


def gate_mid_fwd(za, zb, k, a, sc1, sh1, w2, b, st2):
    n, h, w, _ = za.shape
    call("eunet_gate_mid_fwd", _ptr(za), _ptr(zb), n, h, w, k, _ptr(a), _ptr(sc1), _ptr(sh1), _ptr(w2), _ptr(b),
         _ptr(st2), _stream())


def gate_out_fwd(za, zb, k, b, sc2, sh2, f2: Act):
    n, h, w, _ = za.shape
    call("eunet_gate_out_fwd", _ptr(za), _ptr(zb), n, h, w, k, _ptr(b), _ptr(sc2), _ptr(sh2), ctypes.byref(f2),
         _stream())


def fusion_out_fwd(za, zb, k, y3: Act, sc3, sh3, w11, b11, b, sc2, sh2, wr, br, out):
    call("eunet_fusion_out_fwd", _ptr(za), _ptr(zb), k, ctypes.byref(y3), _ptr(sc3), _ptr(sh3), _ptr(w11), _ptr(b11),
         _ptr(b), _ptr(sc2), _ptr(sh2), _ptr(wr), _ptr(br), _ptr(out), _stream())


def fusion_out_bwd(za, zb, k, gout, b, sc2, sh2, wr, gz, gf2res, part):
    n, h, w, _ = za.shape
    call("eunet_fusion_out_bwd", _ptr(za), _ptr(zb), n, h, w, k, _ptr(gout), _ptr(b), _ptr(sc2), _ptr(sh2),
         _ptr(wr), _ptr(gz), _ptr(gf2res), _ptr(part), _stream())


def gate_bwd1(za, zb, k, gf2conv: Act, gf2res, b, mean2, istd2, gam2, bet2, gffd, gbhat, part):
    call("eunet_gate_bwd1", _ptr(za), _ptr(zb), k, ctypes.byref(gf2conv), _ptr(gf2res), _ptr(b), _ptr(mean2),
         _ptr(istd2), _ptr(gam2), _ptr(bet2), _ptr(gffd), _ptr(gbhat), _ptr(part), _stream())


def gate_bwd2(n, h, w, k, gbhat, b, mean2, istd2, gam2, dbet2, dgam2, a, mean1, istd1, gam1, bet1, w2, gabn, part):
    call("eunet_gate_bwd2", n, h, w, k, _ptr(gbhat), _ptr(b), _ptr(mean2), _ptr(istd2), _ptr(gam2), _ptr(dbet2),
         _ptr(dgam2), _ptr(a), _ptr(mean1), _ptr(istd1), _ptr(gam1), _ptr(bet1), _ptr(w2), _ptr(gabn), _ptr(part),
         _stream())


def gate_bwd3(za, zb, k, gabn, a, mean1, istd1, gam1, dbet1, dgam1, w1, gffd, gaux_a, gaux_b, gz_a, gz_b, part):
    n, h, w, _ = za.shape
    call("eunet_gate_bwd3", _ptr(za), _ptr(zb), n, h, w, k, _ptr(gabn), _ptr(a), _ptr(mean1), _ptr(istd1),
         _ptr(gam1), _ptr(dbet1), _ptr(dgam1), _ptr(w1), _ptr(gffd), _ptr(gaux_a), _ptr(gaux_b), _ptr(gz_a),
         _ptr(gz_b), _ptr(part), _stream())


def dropout_affine(scale, shift, keep, p, nscale, nshift, gscale=None):
    n, c = keep.shape
    call("eunet_dropout_affine", _ptr(scale), _ptr(shift), _ptr(keep), n, c, float(p), _ptr(nscale), _ptr(nshift),
         _ptr(gscale), _stream())


def consistency_tiles(h, w):
    t = c_int()
    call("eunet_consistency_tiles", h, w, ctypes.byref(t))
    return t.value


def consistency_fwd(fused, b0, b1, c0, c1, part, loss):
    n, k, h, w = fused.shape
    call("eunet_consistency_fwd", _ptr(fused), _ptr(b0), _ptr(b1), n, k, h, w, float(c0), float(c1), _ptr(part),
         _ptr(loss), _stream())


def consistency_bwd(fused, b0, b1, c0, c1, gloss, gfused, g0, g1):
    n, k, h, w = fused.shape
    call("eunet_consistency_bwd", _ptr(fused), _ptr(b0), _ptr(b1), n, k, h, w, float(c0), float(c1), _ptr(gloss),
         _ptr(gfused), _ptr(g0), _ptr(g1), _stream())


# ---- device-side data path (datapath.hip) ---------------------------------------------
def upload(a, device):
    """Host numpy array -> device tensor without a host synchronisation: staged through the
    caching pinned-memory allocator and copied asynchronously on the current stream (a pageable
    copy would wait for the stream to drain first)."""
    import numpy as np
    t = torch.from_numpy(np.ascontiguousarray(a))
    if torch.device(device).type != "cuda":
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


def _poly_arrays(polys):
    import numpy as np
    pts = np.concatenate([np.asarray(p, np.int32).reshape(-1, 2) for p in polys])
    off = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.int32)
    return pts, off


def rasterize_polygons(polys, labels, h, w, device):
    """polys: list of int32 [n_i, 2] (x, y) arrays; labels: ints (1 live, 2 dead) -> int64 [h, w]."""
    mask = torch.empty(h, w, dtype=torch.int64, device=device)
    if not polys:
        call("eunet_rasterize_polygons", None, None, None, 0, h, w, _ptr(mask), _stream())
        return mask
    import numpy as np
    pts_h, off_h = _poly_arrays(polys)
    pts, off, lab = upload(pts_h, device), upload(off_h, device), upload(np.asarray(labels, np.int32), device)
    call("eunet_rasterize_polygons", _ptr(pts), _ptr(off), _ptr(lab), len(polys), h, w, _ptr(mask), _stream())
    return mask


def rasterize_instances(polys, h, w, device, flip_h: bool = False, flip_v: bool = False):
    """One uint8 [h, w] mask per polygon (stacked [n, h, w]), mirrored by the training flips."""
    if not polys:
        return torch.zeros(0, h, w, dtype=torch.uint8, device=device)
    pts_h, off_h = _poly_arrays(polys)
    pts, off = upload(pts_h, device), upload(off_h, device)
    masks = torch.empty(len(polys), h, w, dtype=torch.uint8, device=device)
    call("eunet_rasterize_instances", _ptr(pts), _ptr(off), len(polys), h, w, int(flip_h), int(flip_v), _ptr(masks),
         _stream())
    return masks


def flip_u8(img, mode: int):
    out = torch.empty_like(img)
    h, w, c = img.shape
    call("eunet_flip_u8", _ptr(img.contiguous()), _ptr(out), h, w, c, int(mode), _stream())
    return out


def flip_mask(mask, mode: int):
    out = torch.empty_like(mask)
    h, w = mask.shape
    call("eunet_flip_mask", _ptr(mask.contiguous()), _ptr(out), h, w, int(mode), _stream())
    return out


# ---- elastic deformation and affine warp (warp.hip; U-Net paper §3.1, no reference counterpart) ----
WARP_BORDERS = {"constant": 0, "reflect": 1}  # EUNET_WARP_CONSTANT, EUNET_WARP_REFLECT101
WARP_GRID_MAX = 16


def _warp_border(what, border):
    if border not in WARP_BORDERS:
        raise ValueError(f"{what}: unknown border {border!r}; known: {sorted(WARP_BORDERS)}")
    return WARP_BORDERS[border]


def _warp_map(what, grid):
    if grid.dim() != 3 or grid.shape[2] != 2 or grid.dtype != torch.float32 or min(grid.shape[:2]) < 1:
        raise ValueError(f"{what}: grid must be float32 [h, w, 2], got {grid.dtype} {tuple(grid.shape)}")
    return grid.contiguous()


def elastic_grid(h, w, ctrl, matrix=None, device="cuda"):
    """eunet_warp_grid: the dense sampling map float32 [h, w, 2], (sx, sy) in absolute source pixels, of the 2x3
    inverse (destination -> source) affine map `matrix` (host array; None: the identity) plus the bicubic
    interpolation (F.interpolate, align_corners=True) of the control displacements ctrl [2, gh, gw] (host array
    or device tensor; plane 0 dx, plane 1 dy, in pixels; 2 <= gh, gw <= 16)."""
    import numpy as np
    if isinstance(ctrl, torch.Tensor):
        c = ctrl
    else:
        a = np.asarray(ctrl, dtype=np.float32)
        if not np.isfinite(a).all():
            raise ValueError("elastic_grid: ctrl holds non-finite values")
        c = a
    if len(c.shape) != 3 or c.shape[0] != 2:
        raise ValueError(f"elastic_grid: ctrl must be [2, gh, gw], got {tuple(c.shape)}")
    gh, gw = int(c.shape[1]), int(c.shape[2])
    if not (2 <= gh <= WARP_GRID_MAX and 2 <= gw <= WARP_GRID_MAX):
        raise ValueError(f"elastic_grid: control grid {gh} x {gw} outside 2..{WARP_GRID_MAX}")
    if int(h) < 1 or int(w) < 1:
        raise ValueError(f"elastic_grid: size {h} x {w} must be at least 1 x 1")
    m = None
    if matrix is not None:
        mh = np.asarray(matrix, dtype=np.float64)
        if mh.shape != (2, 3) or not np.isfinite(mh).all():
            raise ValueError("elastic_grid: matrix must be a finite host 2x3 array")
        m = ctypes.byref((ctypes.c_double * 6)(*mh.reshape(-1).tolist()))
    if isinstance(c, torch.Tensor):
        c = c.to(device=device, dtype=torch.float32).contiguous()
    else:
        c = upload(c, device)
    out = torch.empty(int(h), int(w), 2, dtype=torch.float32, device=c.device)
    call("eunet_warp_grid", _ptr(c), gh, gw, m, int(h), int(w), _ptr(out), _stream())
    return out


def warp_u8(img, grid, border="reflect", fill=0):
    """eunet_warp_u8: HWC uint8 image (1..4 channels) gathered bilinearly through a map [ho, wo, 2] (elastic_grid's,
    or any float32 map of absolute source coordinates) -> uint8 [ho, wo, c]; integer arithmetic in 1/32 pixel."""
    b = _warp_border("warp_u8", border)
    g = _warp_map("warp_u8", grid)
    if img.dim() != 3 or img.dtype != torch.uint8 or not 1 <= img.shape[2] <= 4 or img.device != g.device:
        raise ValueError(f"warp_u8: img must be uint8 [h, w, 1..4] on the map's device, got {img.dtype} {tuple(img.shape)}")
    if not 0 <= int(fill) <= 255:
        raise ValueError(f"warp_u8: fill {fill} outside 0..255")
    hi, wi, c = img.shape
    ho, wo = g.shape[:2]
    out = torch.empty(ho, wo, c, dtype=torch.uint8, device=img.device)
    call("eunet_warp_u8", _ptr(img.contiguous()), hi, wi, c, _ptr(g), ho, wo, b, int(fill), _ptr(out), _stream())
    return out


def warp_labels(x, grid, border="reflect", fill=0, flip_h: bool = False, flip_v: bool = False):
    """eunet_warp_labels: an int64 [h, w] label map or a uint8 [n, h, w] stack gathered nearest-neighbour through
    the map -> [ho, wo] / [n, ho, wo]; every output value is a source value or `fill`.  flip_h / flip_v mirror
    the result (the training flips, as rasterize_instances takes them)."""
    b = _warp_border("warp_labels", border)
    g = _warp_map("warp_labels", grid)
    ho, wo = g.shape[:2]
    if x.dtype == torch.int64 and x.dim() == 2:
        planes, (hi, wi), eb, shape = 1, x.shape, 8, (ho, wo)
    elif x.dtype == torch.uint8 and x.dim() == 3:
        planes, (hi, wi), eb, shape = x.shape[0], x.shape[1:], 1, (x.shape[0], ho, wo)
        if not 0 <= int(fill) <= 255:
            raise ValueError(f"warp_labels: fill {fill} outside 0..255 for a uint8 stack")
    else:
        raise ValueError(f"warp_labels: needs an int64 [h, w] map or a uint8 [n, h, w] stack, got {x.dtype} {tuple(x.shape)}")
    if x.device != g.device:
        raise ValueError("warp_labels: labels and map must be on one device")
    out = torch.empty(shape, dtype=x.dtype, device=x.device)
    call("eunet_warp_labels", _ptr(x.contiguous()) if planes else None, eb, planes, hi, wi, _ptr(g), ho, wo, b, int(fill),
         int(bool(flip_h)), int(bool(flip_v)), _ptr(out) if planes else None, _stream())
    return out


def augment_u8(img, alpha=None, beta=None, noise=None, lut=None):
    """In-place on a contiguous uint8 device tensor (reference order: alpha, beta, noise, LUT)."""
    flags = (1 if alpha is not None else 0) | (2 if beta is not None else 0) | \
        (4 if noise is not None else 0) | (8 if lut is not None else 0)
    call("eunet_augment_u8", _ptr(img), img.numel(), flags, float(alpha or 0.0), float(beta or 0.0),
         _ptr(noise), _ptr(lut), _stream())
    return img


def augment_ratio_u8(img, counts, u_alpha=None, u_beta=None):
    """In place: the reference's live-ratio-dependent brightness / contrast (dataset.py:225-257) with
    the ratio read from device counts (semantic_counts) and u_* the host's random.random() draws."""
    flags = (1 if u_alpha is not None else 0) | (2 if u_beta is not None else 0)
    if flags:
        call("eunet_augment_ratio_u8", _ptr(img), img.numel(), _ptr(counts), flags,
             0.0 if u_alpha is None else float(u_alpha), 0.0 if u_beta is None else float(u_beta), _stream())
    return img


def to_tensor(img):
    h, w, c = img.shape
    out = torch.empty(c, h, w, dtype=torch.float32, device=img.device)
    call("eunet_to_tensor", _ptr(img.contiguous()), h, w, c, _ptr(out), _stream())
    return out


def resize_u8(img, ho, wo):
    hi, wi, c = img.shape
    out = torch.empty(ho, wo, c, dtype=torch.uint8, device=img.device)
    call("eunet_resize_u8", _ptr(img.contiguous()), hi, wi, c, _ptr(out), ho, wo, _stream())
    return out


# ---- cv2 image operations (imgproc.hip) -------------------------------------------------
SHARPEN_3X3 = (-1.0, -1.0, -1.0, -1.0, 9.0, -1.0, -1.0, -1.0, -1.0)  # dataset.py:288-290, train_eval.py:388-390


def _size_out(fn, *args):
    n = ctypes.c_size_t(0)
    call(fn, *args, ctypes.byref(n))
    return int(n.value)


def rgb2lab_u8(img):
    out = torch.empty_like(img)
    call("eunet_rgb2lab_u8", _ptr(img.contiguous()), _ptr(out), img.shape[0] * img.shape[1], _stream())
    return out


def lab2rgb_u8(lab):
    out = torch.empty_like(lab)
    call("eunet_lab2rgb_u8", _ptr(lab.contiguous()), _ptr(out), lab.shape[0] * lab.shape[1], _stream())
    return out


def rgb2gray_u8(img):
    h, w, _ = img.shape
    out = torch.empty(h, w, dtype=torch.uint8, device=img.device)
    call("eunet_rgb2gray_u8", _ptr(img.contiguous()), _ptr(out), h * w, _stream())
    return out


def hsv_adjust_u8(img, sat=None, hue=None, val=None):
    """In place: S *= sat (dataset.py:259-264) or H += hue mod 180, V *= val (:295-300)."""
    mode = (1 if sat is not None else 0) | (2 if hue is not None else 0)
    if mode & 2 and val is None:
        raise ValueError("hsv_adjust_u8: hue and val go together")
    # explicit None tests: sat = 0.0 / val = 0.0 are real requests (desaturate / black), not "unset"
    call("eunet_hsv_adjust_u8", _ptr(img), img.shape[0] * img.shape[1], 1.0 if sat is None else float(sat),
         0.0 if hue is None else float(hue), 1.0 if val is None else float(val), mode, _stream())
    return img


def clahe_u8(src, clip_limit, grid=(8, 8), lab_to_rgb=False):
    """cv2.createCLAHE(clip_limit, grid).apply.  lab_to_rgb: src is a Lab image, its L channel is
    equalised and the RGB image is returned (the merge + LAB2RGB of dataset.py:70-71)."""
    h, w = src.shape[:2]
    luts = torch.empty(grid[0] * grid[1] * 256, dtype=torch.uint8, device=src.device)
    out = torch.empty(h, w, 3, dtype=torch.uint8, device=src.device) if lab_to_rgb else torch.empty_like(src)
    call("eunet_clahe_u8", _ptr(src.contiguous()), int(lab_to_rgb), h, w, float(clip_limit), grid[0], grid[1],
         _ptr(luts), _ptr(out), _stream())
    return out


def clahe_rgb_u8(img, clip_limit, grid=(8, 8)):
    """RGB -> Lab, CLAHE on L, -> RGB (dataset.py:63-71, 268-272; train_eval.py:380-385)."""
    return clahe_u8(rgb2lab_u8(img), clip_limit, grid, lab_to_rgb=True)


def filter3x3_u8(img, k9):
    h, w = img.shape[:2]
    c = img.shape[2] if img.dim() == 3 else 1
    kk = (ctypes.c_float * 9)(*[float(v) for v in k9])
    out = torch.empty_like(img)
    call("eunet_filter3x3_u8", _ptr(img.contiguous()), _ptr(out), h, w, c, ctypes.addressof(kk), _stream())
    return out


def sharpen_u8(img, strength):
    """cv2.filter2D(img, -1, [[-1,-1,-1],[-1,9,-1],[-1,-1,-1]] * strength)."""
    return filter3x3_u8(img, [v * strength for v in SHARPEN_3X3])


def unsharp_u8(img):
    h, w = img.shape[:2]
    c = img.shape[2] if img.dim() == 3 else 1
    out = torch.empty_like(img)
    call("eunet_unsharp_u8", _ptr(img.contiguous()), _ptr(out), h, w, c, _stream())
    return out


def edge_features_u8(gray):
    h, w = gray.shape
    ws = torch.empty(_size_out("eunet_edge_features_workspace_bytes", h, w), dtype=torch.uint8, device=gray.device)
    out = torch.empty_like(gray)
    call("eunet_edge_features_u8", _ptr(gray.contiguous()), h, w, _ptr(ws), _ptr(out), _stream())
    return out


def cell_preprocess_u8(img, live_mask, dead_mask=None):
    """dataset.py:58-131 (_apply_cell_specific_preprocessing) on an HWC uint8 device image.
    live_mask / dead_mask: int64 [h, w], nonzero where any live / dead instance covers the
    pixel (the np.maximum unions of :96-100); dead_mask None = no dead instance."""
    h, w, _ = img.shape
    img = img.contiguous()
    clahe = clahe_rgb_u8(img, 2.5)
    edges = edge_features_u8(rgb2gray_u8(img))
    if live_mask is not None:
        call("eunet_live_boost_u8", _ptr(clahe), _ptr(live_mask.contiguous()), h * w, _stream())
    dead_gray = clahe_u8(rgb2gray_u8(clahe), 3.0) if dead_mask is not None else None
    mixed = torch.empty_like(img)
    call("eunet_cell_mix_u8", _ptr(img), _ptr(clahe), _ptr(edges),
         _ptr(dead_mask.contiguous() if dead_mask is not None else None), _ptr(dead_gray), h * w, _ptr(mixed),
         _stream())
    return unsharp_u8(mixed)


def chw_to_u8(x):
    """train_eval.py:367-377: CHW float -> HWC uint8 (x * 255 if max(x) <= 1), on the device."""
    c, h, w = x.shape
    x = x.contiguous().float()
    ws = torch.empty(_size_out("eunet_chw_to_u8_workspace_bytes", c, h, w), dtype=torch.uint8, device=x.device)
    out = torch.empty(h, w, c, dtype=torch.uint8, device=x.device)
    call("eunet_chw_to_u8", _ptr(x), c, h, w, _ptr(ws), _ptr(out), _stream())
    return out
