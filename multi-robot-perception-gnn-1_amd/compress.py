"""The 1x1 compress convolution after the concatenation (``dgl/model/models.py:163-165,181-184,186-189``:
``h = conv(torch.cat((h, g_h), 1))`` with ``conv = nn.Conv2d(2C, C, kernel_size=1)``) and both of its
gradients on hand-written matrix-core kernels (``include/mrp_gnn.h``).

Per node n a 1x1 convolution over NCHW is ``y[n] = W [x[n]; a[n]] + b`` with W (C, 2C) shared, so:

* forward:      one GEMM whose K rows come from two tensors (x and the aggregate) — the (N, 2C, H, W)
  concatenation is never written;
* data grad:    ``[dx[n]; da[n]] = W^T dy[n]``, written straight into x's gradient half and the
  aggregate's gradient (which the aggregation backward then consumes) — no (N, 2C, H, W) buffer;
* weight grad:  ``dW = sum_n dy[n] [x[n]; a[n]]^T`` and ``db = sum dy`` in one split-K kernel with a
  fixed-order sum of its partial tiles (deterministic), no (N, C, 2C) temporary, no layout copies.

Arithmetic (:func:`set_compress_path`): ``"split"`` (default) runs all three products on the bf16
matrix cores with every fp32 operand split exactly into three bf16 parts and six partial products per
product (``mrp_compress_fwd_split`` / ``_bwd_data_split`` / ``_bwd_weight_split``, as accurate as an
fp32 GEMM: the omitted terms are below 2^-25 of each product; the weight gradient where C % 64 == 0);
``"hip"`` runs all three on the fp32 MFMA (``mrp_compress_fwd`` / ``_bwd_data`` / ``_bwd_weight``, exact
fp32 products).  Both are checked against float64 (``tests/stack_ref``).  The split weight images are
built once per weight version (:func:`packed_weight`).

The module keeps the reference's ``nn.Conv2d`` parameters (``conv1.weight`` (C, 2C, 1, 1),
``conv1.bias``), so ``state_dict`` keys are unchanged.

Shapes the kernels do not tile (C % 32 != 0, H W % 4 != 0 — and, for the weight gradient only,
H W % 32 != 0 — none of them a reference configuration: the reference's planes are
``image_size/32`` squares, 8 x 8 at its default) run the same kernels on zero-padded operands
(:func:`_fwd`, :func:`_bwd_data`, :func:`_bwd_weight`); ``set_compress_path("library")`` runs
torch's own GEMMs everywhere, for A/B measurements only.

bf16 / fp16 feature maps (a backbone under ``torch.autocast``; the parameters stay fp32) run the same
three products natively (``csrc/compress_half.hip``: ``mrp_compress_fwd_t`` / ``_bwd_data_t`` /
``_bwd_weight_t``): the weight is rounded once to the feature type T when it is packed, every product
of two T values is exact in the fp32 accumulator, the fp32 bias is added to the fp32 sum, outputs and
data gradients are rounded once at the store, and ``dW`` / ``db`` are accumulated and stored in fp32.
Their tiles need C % 32 == 0 and H W % 8 == 0 (32 for the weight gradient); other shapes are
zero-padded as above.  :func:`set_half_compress` ``("torch")`` restores the earlier route (the 16-bit
cat kernel + torch's convolution) for A/B runs; :data:`PATH_COUNTS` counts the launches per route.

Precision of the ``"split"`` path on fp32 features (:func:`set_compress_precision`): ``"highest"``
(default) keeps all three bf16 parts of every operand and the six partial products; ``"high"`` keeps two
parts and the three products ``a0 b0 + a0 b1 + a1 b0`` (per-term error at most 3.1 x 2^-18, about 100 x
finer than TF32); ``"medium"`` keeps one part and one product (bf16 operands, fp32 accumulation and
output; per-term error at most 2.01 x 2^-9).  The reduced forms skip the dropped parts' conversions, LDS
traffic and MFMAs (``mrp_compress_fwd_split_p`` / ``_bwd_data_split_p`` / ``_bwd_weight_split_p``); the
packed weight images and ``db`` (the fp32 sum of the full ``dy``) are the same in every mode.

Pixel-major (``torch.channels_last``) bf16 / fp16 feature maps with C % 32 == 0 run the three products
on kernels of their own (``csrc/compress_half_cl.hip``: ``mrp_compress_fwd_cl`` / ``_bwd_data_cl`` /
``_bwd_weight_cl``), which read the features in place — dense maps or the halves of a channels_last
concatenation buffer — tile any H W without padding, reuse the same packed weight images and return
dense channels_last.  :func:`set_channels_last_compress` ``("convert")`` restores the earlier route (a
copy to NCHW, the kernels above, NCHW results); C % 32 != 0 always takes it
(``PATH_COUNTS["convert_cl"]`` counts the 16-bit calls that did), and so do fp32 channels_last features by
default.

Pixel-major fp32 feature maps have kernels of their own too (``csrc/compress_split_cl.hip``:
``mrp_compress_fwd_split_cl`` / ``_bwd_data_split_cl`` / ``_bwd_weight_split_cl``, the split-bf16 arithmetic
in the three precision modes, any H W, dense or strided halves, channels_last results), behind an opt-in
switch: :func:`set_channels_last_compress_fp32` ``("native")``; its default ``"convert"`` is the route above,
unchanged.  They count under ``fwd_cl_f32`` / ``dgrad_cl_f32`` / ``wgrad_cl_f32`` (``_high`` / ``_medium``
for the reduced modes).
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import weakref

import torch

from . import _lib

_PATH = ["split"]
# products the "split" path runs on the split-bf16 kernels (the rest on the fp32 MFMA): "fwd", "dgrad",
# "wgrad" (set_compress_path(..., split_ops=...); for A/B and accuracy studies)
_SPLIT_OPS = {"fwd", "dgrad", "wgrad"}


#: 16-bit feature dtypes of the native compress -> enum mrp_dtype, and the counter keys of every dtype
HALF_DTYPES = {torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}
_KEYS = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}

#: Which route ran: ``fwd_*`` / ``dgrad_*`` / ``wgrad_*`` for each of ``f32`` / ``bf16`` / ``f16`` count
#: the kernel launches of this module per feature dtype; ``torch_16`` counts 16-bit layers handed to
#: torch's convolution (:func:`compress_1x1` with ``set_half_compress("torch")``, or a conv stored in T).
#: fp32 calls that ran a reduced split form count under ``fwd_f32_high`` / ``dgrad_f32_high`` /
#: ``wgrad_f32_high`` (and ``_medium``) instead of the plain ``_f32`` keys.
PATH_COUNTS = collections.Counter()

#: precision mode -> bf16 parts kept per operand (the products kept are those with i + j < parts)
PRECISION_PARTS = {"highest": 3, "high": 2, "medium": 1}
_PRECISION = ["highest"]


def set_compress_precision(mode: str) -> str:
    """Precision of the fp32 products on the ``"split"`` compress path: ``"highest"`` (default) six partial
    products per product, fp32 accuracy; ``"high"`` two bf16 parts per operand and three products (bf16x3,
    per-term error <= 3.1 x 2^-18); ``"medium"`` one part and one product (bf16 operands, fp32 accumulation,
    per-term error <= 2.01 x 2^-9).  Applies to fp32 features only — zero-padded odd shapes, per-node-range
    calls and the convert route of fp32 channels_last features included, which all end in the same kernels,
    and the pixel-major fp32 kernels of :func:`set_channels_last_compress_fp32` ``("native")``.
    ``set_compress_path("hip" | "library")`` and bf16 / fp16 features ignore the mode.  An autograd node
    keeps the mode its forward ran in for both of its gradients.  Returns the previous mode."""
    if mode not in PRECISION_PARTS:
        raise ValueError("compress precision must be 'highest', 'high' or 'medium'")
    prev, _PRECISION[0] = _PRECISION[0], mode
    return prev


def compress_precision() -> str:
    """The current mode of :func:`set_compress_precision`."""
    return _PRECISION[0]


@contextlib.contextmanager
def compress_precision_scope(mode: str):
    """``with compress_precision_scope("high"): ...`` — the mode inside, the previous one restored on the way
    out (also when the body raises).  Split-path fp32 products only; see :func:`set_compress_precision`."""
    prev = set_compress_precision(mode)
    try:
        yield
    finally:
        _PRECISION[0] = prev


def _mode(precision) -> str:
    if precision is None:
        return _PRECISION[0]
    if precision not in PRECISION_PARTS:
        raise ValueError("compress precision must be 'highest', 'high' or 'medium'")
    return precision


def _mode_key(key: str, mode: str) -> str:
    return key if mode == "highest" else key + "_" + mode

_HALF = ["native"]


def set_half_compress(route: str) -> str:
    """Route of a bf16 / fp16 ``cat_compress`` layer with fp32 parameters: ``"native"`` (default) the
    kernels of ``compress_half.hip``; ``"torch"`` the 16-bit cat kernel followed by ``conv(h)``, torch's
    own convolution (needs ``torch.autocast``), for A/B runs.  Returns the previous value."""
    if route not in ("native", "torch"):
        raise ValueError("half compress route must be 'native' or 'torch'")
    prev, _HALF[0] = _HALF[0], route
    return prev


def half_compress() -> str:
    return _HALF[0]


_CL = ["native"]


def set_channels_last_compress(route: str) -> str:
    """Route of a pixel-major (``torch.channels_last``) bf16 / fp16 operand set: ``"native"`` (default) the
    pixel-major kernels of ``compress_half_cl.hip`` (``mrp_compress_fwd_cl`` / ``_bwd_data_cl`` /
    ``_bwd_weight_cl``), which read the features in place and return channels_last; ``"convert"`` copies
    them to NCHW and runs the node-major kernels (the route before the pixel-major kernels existed; for
    A/B runs).  ``aggregate.set_channels_last("convert")`` implies ``"convert"`` here.  C % 32 != 0 takes
    the convert route either way; fp32 features have a switch of their own
    (:func:`set_channels_last_compress_fp32`, default ``"convert"``).  This switch is the A/B lever from Python; the library's
    tuning knob ``compress_half_cl`` = 0 makes the C entry points decline and is meant for C callers: this
    module does not consult it, and a declined pixel-major call raises.  Returns the previous value."""
    if route not in ("native", "convert"):
        raise ValueError("channels_last compress route must be 'native' or 'convert'")
    prev, _CL[0] = _CL[0], route
    return prev


def channels_last_compress() -> str:
    return _CL[0]


_CL_F32 = ["convert"]


def set_channels_last_compress_fp32(route: str) -> str:
    """Route of a pixel-major (``torch.channels_last``) fp32 operand set: ``"convert"`` (default) copies it
    to NCHW, runs the node-major kernels and returns NCHW; ``"native"`` runs the pixel-major split-bf16
    kernels of ``compress_split_cl.hip`` (``mrp_compress_fwd_split_cl`` / ``_bwd_data_split_cl`` /
    ``_bwd_weight_split_cl``), which read the features in place, tile any H W and return dense channels_last,
    in the mode of :func:`set_compress_precision`.  ``"native"`` applies where ``aggregate.set_channels_last``
    is ``"native"``, the path is ``"split"`` with all three products on the split kernels and C % 32 == 0;
    elsewhere the convert route runs as before.  Results agree with the NCHW kernels' to fp32 rounding (the
    k order inside a product differs), not bit for bit.  Measured against the convert route in the same
    process (``tools/bench_channels_last_compress_fp32.py``) at configs[1], [2], [4] in all
    three modes: every product is faster than ``"convert"`` (forward 0.31-0.75 x, data gradient 0.55-0.84 x,
    weight gradient 0.43-0.78 x its time; a layer's training step 0.48-0.81 x); against NCHW tensors on the
    NCHW kernels the forward and data gradient take 1.02-1.17 x and the weight gradient 1.16-1.25 x
    (``"highest"``) to 2.06 x (``"medium"``, C = 1280).  Returns the previous value."""
    if route not in ("native", "convert"):
        raise ValueError("fp32 channels_last compress route must be 'native' or 'convert'")
    prev, _CL_F32[0] = _CL_F32[0], route
    return prev


def channels_last_compress_fp32() -> str:
    """The current route of :func:`set_channels_last_compress_fp32`."""
    return _CL_F32[0]


def _cl_features(t: torch.Tensor) -> bool:
    """A bf16 / fp16 pixel-major feature map (``aggregate.pixel_strides``)."""
    from .aggregate import pixel_strides
    return t.dtype in HALF_DTYPES and t.is_cuda and pixel_strides(t) is not None


def _cl_route(t: torch.Tensor) -> bool:
    """Whether this feature map's products run on the pixel-major kernels."""
    from . import aggregate
    if t.dtype == torch.float32:  # opt-in, the split path's three products only
        return (_CL_F32[0] == "native" and aggregate._CHANNELS_LAST == "native" and _PATH[0] == "split"
                and _SPLIT_OPS >= {"fwd", "dgrad", "wgrad"} and t.shape[1] % 32 == 0 and t.is_cuda
                and aggregate.pixel_strides(t) is not None)
    return (_CL[0] == "native" and aggregate._CHANNELS_LAST == "native" and _PATH[0] != "library"
            and t.shape[1] % 32 == 0 and _cl_features(t))


def _count_convert(t: torch.Tensor) -> None:
    if _cl_features(t):
        PATH_COUNTS["convert_cl"] += 1


def _pstrides(t: torch.Tensor):
    """(node stride, pixel stride) of a pixel-major tensor laid out as the kernels need (16-byte aligned,
    strides whole 16-byte pieces), else None."""
    from .aggregate import pixel_strides
    s = pixel_strides(t)
    m = 16 // t.element_size()  # elements per 16-byte piece: 8 for bf16 / fp16, 4 for fp32
    if s is None or s[0] % m != 0 or s[1] % m != 0 or t.data_ptr() % 16 != 0:
        return None
    return s


def _pixel_major(t: torch.Tensor):
    """(tensor, node stride, pixel stride), converting (one copy) an operand that is not pixel-major."""
    s = _pstrides(t)
    if s is None:
        n, c, h, w = t.shape
        t = _empty_cl(t.shape, t.device, t.dtype).copy_(t)
        s = (c * h * w, c)
    return t, s[0], s[1]


def _empty_cl(shape, device, dtype) -> torch.Tensor:
    return torch.empty(tuple(shape), device=device, dtype=dtype, memory_format=torch.channels_last)


def _split(op: str) -> bool:
    return _PATH[0] == "split" and op in _SPLIT_OPS


def set_compress_path(path: str, split_ops=None) -> None:
    """``"split"`` (default): forward, data gradient and weight gradient on the split-bf16 matrix
    cores (``compress_split.hip``, fp32-accurate; the weight gradient falls back to the fp32 MFMA
    where C % 64 or H W % 32 is not 0); ``split_ops`` narrows which of "fwd" / "dgrad" / "wgrad" take
    the split kernels; ``"hip"``: all three on
    the fp32 MFMA (``compress_gemm.hip``); ``"library"``: the cat kernel + torch's library GEMMs (the
    round-2 path), for A/B measurement."""
    if path not in ("split", "hip", "library"):
        raise ValueError("compress path must be 'split', 'hip' or 'library'")
    _PATH[0] = path
    if split_ops is not None:
        ops = set(split_ops)
        if not ops <= {"fwd", "dgrad", "wgrad"}:
            raise ValueError("split_ops: a subset of {'fwd', 'dgrad', 'wgrad'}")
        _SPLIT_OPS.clear()
        _SPLIT_OPS.update(ops)


# packed split-bf16 images of a compress weight, per weight tensor: id -> (weakref, {"fwd" | "bwd":
# (key, image)}), dropped when the tensor dies (tensors compare elementwise, so no WeakKeyDictionary).
# The key holds the data pointer and autograd version, so an optimizer step (an in-place update under
# no_grad) triggers a repack; writes through ``.data`` bypass the version counter: call
# :func:`clear_packed_weights` after those.  Kept outside the modules (not pickled, not deep-copied).
_packed = {}


def clear_packed_weights() -> None:
    _packed.clear()
    _padded_w.clear()


def packed_weight(weight: torch.Tensor, kind: str, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``mrp_compress_split_pack`` image of the (C, 2C[, 1, 1]) weight: ``"fwd"`` packs W (M = C,
    K = 2C) for the forward, ``"bwd"`` packs W^T (M = 2C, K = C) for the data gradient.  ``dtype``
    bf16 / fp16: the ``mrp_compress_pack_t`` image, the weight rounded once to that type (cached per
    weight version, kind and dtype)."""
    from .aggregate import _ptr, _stream
    key = (weight.data_ptr(), weight._version, weight.device.index)
    entry = _packed.get(id(weight))
    slot = entry[1] if entry is not None and entry[0]() is weight else None
    kind, op = (kind if dtype == torch.float32 else (kind, dtype)), kind
    if slot is not None and kind in slot and slot[kind][0] == key:
        return slot[kind][1]
    C = weight.shape[0]
    w = _weight2d(weight)
    M, K, trans = (C, 2 * C, 0) if op == "fwd" else (2 * C, C, 1)
    lib = _lib.load_library()
    if dtype == torch.float32:
        img = torch.empty((int(lib.mrp_compress_split_pack_bytes(M, K)) + 3) // 4, device=w.device,
                          dtype=torch.float32)
        with torch.cuda.device(w.device):
            _lib.check(lib.mrp_compress_split_pack(_ptr(w), 2 * C, trans, M, K, _ptr(img), _stream(w.device)),
                       "mrp_compress_split_pack")
    else:
        img = torch.empty((int(lib.mrp_compress_pack_t_bytes(M, K)) + 3) // 4, device=w.device, dtype=torch.float32)
        with torch.cuda.device(w.device):
            _lib.check(lib.mrp_compress_pack_t(HALF_DTYPES[dtype], _ptr(w), 2 * C, trans, M, K, _ptr(img),
                                               _stream(w.device)), "mrp_compress_pack_t")
    if slot is None:
        slot = {}
        wid = id(weight)
        _packed[wid] = (weakref.ref(weight, lambda _r, wid=wid: _packed.pop(wid, None)), slot)
    slot[kind] = (key, img)
    return img


def compress_path() -> str:
    return _PATH[0]


def _nstride(t: torch.Tensor):
    """Node stride of an (N, C, H, W) fp32 / bf16 / fp16 tensor laid out as the kernels need (each
    node's C H W block contiguous, 16-byte aligned, stride a multiple of 16 bytes), else None."""
    from .aggregate import node_stride
    s = node_stride(t)
    if s is None or s % (16 // t.element_size()) != 0 or t.data_ptr() % 16 != 0:
        return None
    return s


def _node_major(t: torch.Tensor):
    s = _nstride(t)
    if s is None:
        t = t.contiguous()
        s = t.shape[1] * t.shape[2] * t.shape[3]
    return t, s


def _span_nodes(n: int, C: int, P: int, *out_strides: int) -> int:
    """Nodes per call of ``mrp_compress_fwd_t`` / ``_bwd_data_t``: their stores go through 32-bit buffer
    offsets, so the entry points decline an output whose node range — (nodes - 1) node strides + C P
    elements of 2 bytes — reaches 2^31 bytes (``include/mrp_gnn.h``).  Nodes are independent in both products,
    so a wider output (a sparse view, a batch slice of a far larger buffer) is written by consecutive node
    ranges that each fit, with the same values."""
    room = (1 << 30) - 1 - C * P  # elements left for the (nodes - 1) strides
    return max(1, min(n, 1 + max(room, 0) // max(1, *out_strides)))


def _at(t: torch.Tensor, elements: int):
    """Pointer ``elements`` elements behind t's first."""
    return ctypes.c_void_p(t.data_ptr() + elements * t.element_size())


def _weight2d(weight: torch.Tensor) -> torch.Tensor:
    C = weight.shape[0]
    w = weight.detach().reshape(C, weight.shape[1])
    if not w.is_contiguous() or w.dtype != torch.float32:
        w = w.float().contiguous()
    return w


def conv_is_plain_1x1(conv: torch.nn.Conv2d, C: int) -> bool:
    return (conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.groups == 1 and conv.dilation == (1, 1)
            and conv.padding in ((0, 0), "valid") and tuple(conv.weight.shape[:2]) == (C, 2 * C)
            and conv.weight.dtype == torch.float32)


def _pixel_multiple(dtype: torch.dtype) -> int:
    return 8 if dtype in HALF_DTYPES else 4  # 16-byte row pieces


def kernels_supported(C: int, P: int, dtype: torch.dtype = torch.float32) -> bool:
    """The forward and data-gradient kernels: C % 32 == 0, P % 4 == 0 — P % 8 == 0 for bf16 / fp16
    features (``include/mrp_gnn.h``)."""
    return C > 0 and P > 0 and C % 32 == 0 and P % _pixel_multiple(dtype) == 0


def compress_forward(weight: torch.Tensor, bias, x: torch.Tensor, a: torch.Tensor,
                     pixel_major: bool = None, precision: str = None) -> torch.Tensor:
    """``conv(torch.cat((x, a), 1))`` for a (C, 2C, 1, 1) weight without the concatenation
    (``mrp_compress_fwd``); x and a are (N, C, H, W), e.g. views of a cat buffer's halves.  ``precision``:
    the mode of the fp32 split product (default: :func:`compress_precision`); ignored by bf16 / fp16
    features and by the ``"hip"`` path."""
    from .aggregate import _ptr, _stream
    n, C, H, W = x.shape
    dtype = x.dtype  # the feature dtype: a is cast to it, y is allocated in it
    if a.dtype != dtype:
        a = a.to(dtype)
    # pixel-major features on a native route (or the caller's decision): read in place, y dense channels_last
    if _cl_route(x) if pixel_major is None else pixel_major:
        x, xn, xp = _pixel_major(x)
        a, an, ap = _pixel_major(a)
        b = bias.detach() if bias is not None else None
        if b is not None and (b.dtype != torch.float32 or not b.is_contiguous()):
            b = b.float().contiguous()
        y = _empty_cl((n, C, H, W), x.device, dtype)
        mode = _mode(precision) if dtype == torch.float32 else "highest"
        PATH_COUNTS[_mode_key("fwd_cl_" + _KEYS[dtype], mode)] += 1
        with torch.cuda.device(x.device):
            img = packed_weight(weight, "fwd", dtype)
            if dtype == torch.float32:  # the same three-part image in every mode
                _lib.check(_lib.load_library().mrp_compress_fwd_split_cl(
                    _ptr(x), xn, xp, _ptr(a), an, ap, n, C, H * W, _ptr(img), _ptr(b), _ptr(y), C * H * W, C,
                    PRECISION_PARTS[mode], _stream(x.device)), "mrp_compress_fwd_split_cl")
                return y
            _lib.check(_lib.load_library().mrp_compress_fwd_cl(
                HALF_DTYPES[dtype], _ptr(x), xn, xp, _ptr(a), an, ap, n, C, H * W, _ptr(img), _ptr(b), _ptr(y),
                C * H * W, C, _stream(x.device)), "mrp_compress_fwd_cl")
        return y
    x, xs = _node_major(x)
    a, as_ = _node_major(a)
    w = _weight2d(weight)
    b = bias.detach() if bias is not None else None
    if b is not None and (b.dtype != torch.float32 or not b.is_contiguous()):
        b = b.float().contiguous()
    y = torch.empty((n, C, H, W), device=x.device, dtype=dtype)
    lib = _lib.load_library()
    mode = _mode(precision) if dtype == torch.float32 and _split("fwd") else "highest"
    PATH_COUNTS[_mode_key("fwd_" + _KEYS[dtype], mode)] += 1
    with torch.cuda.device(x.device):
        if dtype in HALF_DTYPES:
            img = packed_weight(weight, "fwd", dtype)
            k = _span_nodes(n, C, H * W, C * H * W)
            for i in range(0, n, k):  # one call unless y's node range passes the kernel's 31-bit store offsets
                _lib.check(lib.mrp_compress_fwd_t(HALF_DTYPES[dtype], _at(x, i * xs), xs, _at(a, i * as_), as_,
                                                  min(k, n - i), C, H * W, _ptr(img), _ptr(b), _at(y, i * C * H * W),
                                                  C * H * W, _stream(x.device)), "mrp_compress_fwd_t")
        elif _split("fwd") and mode != "highest":
            img = packed_weight(weight, "fwd")  # the same three-part image: a reduced form fetches fewer parts
            _lib.check(lib.mrp_compress_fwd_split_p(_ptr(x), xs, _ptr(a), as_, n, C, H * W, _ptr(img), _ptr(b), _ptr(y),
                                                    C * H * W, PRECISION_PARTS[mode], _stream(x.device)),
                       "mrp_compress_fwd_split_p")
        elif _split("fwd"):
            img = packed_weight(weight, "fwd")
            _lib.check(lib.mrp_compress_fwd_split(_ptr(x), xs, _ptr(a), as_, n, C, H * W, _ptr(img), _ptr(b), _ptr(y),
                                                  C * H * W, _stream(x.device)), "mrp_compress_fwd_split")
        else:
            _lib.check(lib.mrp_compress_fwd(_ptr(x), xs, _ptr(a), as_, n, C, H * W, _ptr(w), _ptr(b), _ptr(y),
                                            C * H * W, _stream(x.device)), "mrp_compress_fwd")
    return y


def compress_backward_data(weight: torch.Tensor, gy: torch.Tensor, gx: torch.Tensor = None, ga: torch.Tensor = None,
                           dtype: torch.dtype = None, pixel_major: bool = None, precision: str = None):
    """(gx, ga) = (W[:, :C]^T gy, W[:, C:]^T gy) per node (``mrp_compress_bwd_data``), written into
    the given (N, C, H, W) outputs (e.g. the halves of a cat buffer's gradient) or new tensors.  The
    feature dtype is the given outputs', else ``dtype``, else gy's; gy is cast to it.  16-bit pixel-major
    outputs (or, with none given, a pixel-major gy — or ``pixel_major=True``, the layout of the forward's
    features) take the pixel-major kernel (``mrp_compress_bwd_data_cl``; fp32 ones
    ``mrp_compress_bwd_data_split_cl`` where :func:`set_channels_last_compress_fp32` is ``"native"``): new
    outputs are dense channels_last, a gy in the other layout is converted once.  ``precision``: as :func:`compress_forward`."""
    from .aggregate import _ptr, _stream
    n, C, H, W = gy.shape
    lib = _lib.load_library()
    dtype = gx.dtype if gx is not None else ga.dtype if ga is not None else dtype if dtype is not None else gy.dtype
    if gy.dtype != dtype:
        gy = gy.to(dtype)
    if pixel_major is None:
        pixel_major = _cl_route(gx if gx is not None else ga if ga is not None else gy)
    if pixel_major:
        gy, gn, gp = _pixel_major(gy)
        gx = _empty_cl((n, C, H, W), gy.device, dtype) if gx is None else gx
        ga = _empty_cl((n, C, H, W), gy.device, dtype) if ga is None else ga
        sx, sa = _pstrides(gx), _pstrides(ga)
        if sx is None or sa is None or gx.dtype != dtype or ga.dtype != dtype:
            raise ValueError("compress_backward_data: outputs must be pixel-major in one feature dtype, "
                             "16-byte aligned")
        mode = _mode(precision) if dtype == torch.float32 else "highest"
        PATH_COUNTS[_mode_key("dgrad_cl_" + _KEYS[dtype], mode)] += 1
        with torch.cuda.device(gy.device):
            img = packed_weight(weight, "bwd", dtype)
            if dtype == torch.float32:
                _lib.check(lib.mrp_compress_bwd_data_split_cl(_ptr(gy), gn, gp, n, C, H * W, _ptr(img), _ptr(gx),
                                                              sx[0], sx[1], _ptr(ga), sa[0], sa[1],
                                                              PRECISION_PARTS[mode], _stream(gy.device)),
                           "mrp_compress_bwd_data_split_cl")
                return gx, ga
            _lib.check(lib.mrp_compress_bwd_data_cl(HALF_DTYPES[dtype], _ptr(gy), gn, gp, n, C, H * W, _ptr(img),
                                                    _ptr(gx), sx[0], sx[1], _ptr(ga), sa[0], sa[1],
                                                    _stream(gy.device)), "mrp_compress_bwd_data_cl")
        return gx, ga
    gy, gs = _node_major(gy)
    gx = torch.empty((n, C, H, W), device=gy.device, dtype=dtype) if gx is None else gx
    ga = torch.empty((n, C, H, W), device=gy.device, dtype=dtype) if ga is None else ga
    gxs, gas = _nstride(gx), _nstride(ga)
    if gxs is None or gas is None or gx.dtype != dtype or ga.dtype != dtype:
        raise ValueError("compress_backward_data: outputs must be node-major in one feature dtype, 16-byte aligned")
    st = _stream(gy.device)
    mode = _mode(precision) if dtype == torch.float32 and _split("dgrad") else "highest"
    PATH_COUNTS[_mode_key("dgrad_" + _KEYS[dtype], mode)] += 1
    with torch.cuda.device(gy.device):
        if dtype in HALF_DTYPES:
            img = packed_weight(weight, "bwd", dtype)
            k = _span_nodes(n, C, H * W, gxs, gas)
            for i in range(0, n, k):  # one call unless an output's node range passes the 31-bit store offsets
                _lib.check(lib.mrp_compress_bwd_data_t(HALF_DTYPES[dtype], _at(gy, i * gs), gs, min(k, n - i), C, H * W,
                                                       _ptr(img), _at(gx, i * gxs), gxs, _at(ga, i * gas), gas, st),
                           "mrp_compress_bwd_data_t")
            return gx, ga
        if _split("dgrad") and mode != "highest":
            img = packed_weight(weight, "bwd")
            _lib.check(lib.mrp_compress_bwd_data_split_p(_ptr(gy), gs, n, C, H * W, _ptr(img), _ptr(gx), gxs, _ptr(ga),
                                                         gas, PRECISION_PARTS[mode], st),
                       "mrp_compress_bwd_data_split_p")
            return gx, ga
        if _split("dgrad"):
            img = packed_weight(weight, "bwd")
            _lib.check(lib.mrp_compress_bwd_data_split(_ptr(gy), gs, n, C, H * W, _ptr(img), _ptr(gx), gxs, _ptr(ga),
                                                       gas, st), "mrp_compress_bwd_data_split")
            return gx, ga
        w = _weight2d(weight)
        wt = torch.empty((2 * C, C), device=gy.device, dtype=torch.float32)
        _lib.check(lib.mrp_compress_weight_transpose(_ptr(w), _ptr(wt), C, st), "mrp_compress_weight_transpose")
        _lib.check(lib.mrp_compress_bwd_data(_ptr(gy), gs, n, C, H * W, _ptr(wt), _ptr(gx), gxs, _ptr(ga), gas, st),
                   "mrp_compress_bwd_data")
    return gx, ga


def compress_backward_weight(gy: torch.Tensor, x: torch.Tensor, a: torch.Tensor, want_bias: bool = True,
                             weight: torch.Tensor = None, bias: torch.Tensor = None, want_weight: bool = True,
                             pixel_major: bool = None, precision: str = None):
    """(dW (C, 2C, 1, 1), db (C) or None) = (sum_n gy[n] [x[n]; a[n]]^T, sum gy)
    (``mrp_compress_bwd_weight``); None when the kernel declines the shape (H W % 32 != 0).  Given
    the parameters, the results are written straight into a gradient all-reducer's buckets when
    one holds them (``dist.grad_out_like``) — only for a gradient that is wanted, and the slots are
    given back (``dist.release_grad_out``) when the kernel declines the shape.  ``precision``: as
    :func:`compress_forward` (the split kernels only: where the weight gradient falls back to the fp32 MFMA
    it is exact fp32 and counts under the plain key); db is the fp32 sum of the full gy in every mode."""
    from .aggregate import _ptr, _stream
    from .dist import grad_out_like, release_grad_out
    n, C, H, W = gy.shape
    lib = _lib.load_library()
    dtype = x.dtype  # the feature dtype: gy and a are cast to it; dW and db are fp32 either way
    if gy.dtype != dtype:
        gy = gy.to(dtype)
    if a.dtype != dtype:
        a = a.to(dtype)
    if pixel_major is None:
        pixel_major = _cl_route(x)
    if pixel_major:  # pixel-major x: mrp_compress_bwd_weight_cl / _split_cl, gy / a converted once if they differ
        (gy, gs, gp), (x, xs, xp), (a, as_, ap) = _pixel_major(gy), _pixel_major(x), _pixel_major(a)
        head = (_ptr(gy), gs, gp, _ptr(x), xs, xp, _ptr(a), as_, ap)
    else:
        gy, gs = _node_major(gy)
        x, xs = _node_major(x)
        a, as_ = _node_major(a)
        head = (_ptr(gy), gs, _ptr(x), xs, _ptr(a), as_)
    claimed = []
    dw = grad_out_like(weight) if want_weight and weight is not None and weight.dim() == 4 else None
    if dw is not None:
        claimed.append((weight, dw))
    else:
        dw = torch.empty((C, 2 * C, 1, 1), device=gy.device, dtype=torch.float32)
    db = None
    if want_bias:
        db = grad_out_like(bias) if bias is not None else None
        if db is not None:
            claimed.append((bias, db))
        else:
            db = torch.empty((C,), device=gy.device, dtype=torch.float32)
    P = H * W
    split = _split("wgrad") and C % 64 == 0 and P % 32 == 0
    key = "wgrad_" + _KEYS[dtype]
    if pixel_major and dtype == torch.float32:
        mode = _mode(precision)
        nbytes = int(lib.mrp_compress_bwd_weight_split_cl_workspace(n, C, P))  # the bound for every part count
        split_cl = lib.mrp_compress_bwd_weight_split_cl
        fn = lambda *args: split_cl(*args[:-1], PRECISION_PARTS[mode], args[-1])  # noqa: E731
        name, key = "mrp_compress_bwd_weight_split_cl", _mode_key("wgrad_cl_f32", mode)
    elif pixel_major:
        nbytes = int(lib.mrp_compress_bwd_weight_cl_workspace(n, C, P))
        typed_cl = lib.mrp_compress_bwd_weight_cl
        fn, name = (lambda *args: typed_cl(HALF_DTYPES[dtype], *args)), "mrp_compress_bwd_weight_cl"
        key = "wgrad_cl_" + _KEYS[dtype]
    elif dtype in HALF_DTYPES:
        nbytes = int(lib.mrp_compress_bwd_weight_t_workspace(n, C, P))
        typed = lib.mrp_compress_bwd_weight_t
        fn, name = (lambda *args: typed(HALF_DTYPES[dtype], *args)), "mrp_compress_bwd_weight_t"
    elif split and _mode(precision) != "highest":
        mode = _mode(precision)
        nbytes = int(lib.mrp_compress_bwd_weight_split_workspace(n, C, P))  # the bound for every part count
        split_p = lib.mrp_compress_bwd_weight_split_p
        fn = lambda *args: split_p(*args[:-1], PRECISION_PARTS[mode], args[-1])  # noqa: E731
        name, key = "mrp_compress_bwd_weight_split_p", _mode_key(key, mode)
    elif split:
        nbytes = int(lib.mrp_compress_bwd_weight_split_workspace(n, C, P))
        fn, name = lib.mrp_compress_bwd_weight_split, "mrp_compress_bwd_weight_split"
    else:
        nbytes = int(lib.mrp_compress_bwd_weight_workspace(n, C, P, max(gs, xs, as_)))
        fn, name = lib.mrp_compress_bwd_weight, "mrp_compress_bwd_weight"
    done = False
    try:  # claimed bucket slots go back unless the kernel wrote them (declined shape, error, exception)
        ws = torch.empty((nbytes + 3) // 4, device=gy.device, dtype=torch.float32) if nbytes > 0 else None
        with torch.cuda.device(gy.device):
            code = fn(*head, n, C, P, _ptr(dw), _ptr(db), _ptr(ws), nbytes, _stream(gy.device))
        if code == _lib.HIP_ERROR_NOT_SUPPORTED and not pixel_major:
            return None
        _lib.check(code, name)
        PATH_COUNTS[key] += 1
        done = True
        return dw, db
    finally:
        if not done:
            for p, v in claimed:
                release_grad_out(p, v)


# ---- torch library GEMMs: the A/B comparison path and the shapes the kernels decline -------------

def _lib_forward(weight, bias, x, a):
    n, C, H, W = x.shape
    cat = torch.cat((x, a), 1).reshape(n, 2 * C, H * W)
    w2 = weight.reshape(C, 2 * C)
    y = torch.baddbmm(bias.view(1, C, 1), w2.expand(n, C, 2 * C), cat) if bias is not None else \
        torch.bmm(w2.expand(n, C, 2 * C), cat)
    return y.view(n, C, H, W)


def _lib_backward_data(weight, gy):
    n, C, H, W = gy.shape
    d = torch.bmm(weight.reshape(C, 2 * C).t().expand(n, 2 * C, C), gy.reshape(n, C, H * W)).view(n, 2 * C, H, W)
    return d[:, :C], d[:, C:]


def _lib_backward_weight(gy, x, a, want_bias):
    n, C, H, W = gy.shape
    cat = torch.cat((x, a), 1)
    g2 = gy.reshape(n, C, H * W).permute(1, 0, 2).reshape(C, -1)
    h2 = cat.reshape(n, 2 * C, H * W).permute(1, 0, 2).reshape(2 * C, -1)
    return torch.mm(g2, h2.t()).view(C, 2 * C, 1, 1), (gy.sum((0, 2, 3)) if want_bias else None)


# ---- shapes the kernels do not tile: the same kernels on zero-padded operands ---------------------
# C rounded up to 32 and H W to 4 — 8 for bf16 / fp16 features — (forward, data gradient) or 32 (weight
# gradient): padded channels
# carry zero features and zero weight rows / columns, padded pixels zero features and zero gradients,
# so every padded term of every sum is a product with an exact zero and the results are the leading
# blocks of the padded ones.

def _round(n: int, m: int) -> int:
    return (n + m - 1) // m * m


# padded (weight, bias) per weight tensor, keyed like the packed images: id -> (weakref, key, wp, bp)
_padded_w = {}


def _padded_params(weight: torch.Tensor, bias):
    key = (weight.data_ptr(), weight._version, weight.device.index) + \
        ((bias.data_ptr(), bias._version) if bias is not None else ())
    hit = _padded_w.get(id(weight))
    if hit is not None and hit[0]() is weight and hit[1] == key:
        return hit[2], hit[3]
    C = weight.shape[0]
    Cp = _round(C, 32)
    w = _weight2d(weight)
    with torch.no_grad():
        wp = torch.zeros((Cp, 2 * Cp, 1, 1), device=w.device, dtype=torch.float32)
        wp[:C, :C, 0, 0] = w[:, :C]
        wp[:C, Cp:Cp + C, 0, 0] = w[:, C:]
        bp = None
        if bias is not None:
            bp = torch.zeros((Cp,), device=w.device, dtype=torch.float32)
            bp[:C] = bias.detach()
    wid = id(weight)
    _padded_w[wid] = (weakref.ref(weight, lambda _r, wid=wid: _padded_w.pop(wid, None)), key, wp, bp)
    return wp, bp


def _pad_planes(t: torch.Tensor, Cp: int, Pp: int) -> torch.Tensor:
    """(N, C, H, W) -> (N, Cp, Pp, 1) with t in the leading (C, H W) block, zeros elsewhere."""
    n, C, H, W = t.shape
    out = torch.zeros((n, Cp, Pp, 1), device=t.device, dtype=t.dtype)
    out.view(n, Cp, Pp)[:, :C, : H * W] = t.reshape(n, C, H * W)
    return out


def _unpad_planes(t: torch.Tensor, C: int, H: int, W: int) -> torch.Tensor:
    n, Cp, Pp, _ = t.shape
    return t.view(n, Cp, Pp)[:, :C, : H * W].contiguous().view(n, C, H, W)


def _fwd(weight, bias, x, a, cl=None, precision=None):
    """``cl``: the route an autograd function decided once (``_cl_route(x)``), else decided here;
    ``precision``: likewise the mode it read once (``ctx.precision``)."""
    n, C, H, W = x.shape
    if _cl_route(x) if cl is None else cl:
        return compress_forward(weight, bias, x, a, pixel_major=True, precision=precision)
    _count_convert(x)
    if kernels_supported(C, H * W, x.dtype):
        return compress_forward(weight, bias, x, a, pixel_major=False, precision=precision)
    Cp, Pp = _round(C, 32), _round(H * W, _pixel_multiple(x.dtype))
    wp, bp = _padded_params(weight, bias)
    y = compress_forward(wp, bp, _pad_planes(x, Cp, Pp), _pad_planes(a.to(x.dtype), Cp, Pp), pixel_major=False,
                         precision=precision)
    return _unpad_planes(y, C, H, W)


def _bwd_data(weight, gy, dtype=None, like=None, cl=None, precision=None):
    """``like``: the forward's first feature operand — its layout decided the forward's route; ``cl``:
    that decision as the forward remembered it (an autograd function's ``ctx.cl``); ``precision``: the
    forward's mode (``ctx.precision``)."""
    n, C, H, W = gy.shape
    dtype = gy.dtype if dtype is None else dtype
    if (like is not None and _cl_route(like)) if cl is None else cl:
        return compress_backward_data(weight, gy, dtype=dtype, pixel_major=True, precision=precision)
    if like is not None:
        _count_convert(like)
    if kernels_supported(C, H * W, dtype):
        return compress_backward_data(weight, gy, dtype=dtype, pixel_major=False, precision=precision)
    Cp, Pp = _round(C, 32), _round(H * W, _pixel_multiple(dtype))
    wp, _ = _padded_params(weight, None)
    gx, ga = compress_backward_data(wp, _pad_planes(gy.to(dtype), Cp, Pp), pixel_major=False, precision=precision)
    return _unpad_planes(gx, C, H, W), _unpad_planes(ga, C, H, W)


def _bwd_weight(gy, x, a, want_bias, weight, bias, want_weight=True, cl=None, precision=None):
    n, C, H, W = gy.shape
    if _cl_route(x) if cl is None else cl:
        return compress_backward_weight(gy, x, a, want_bias, weight, bias, want_weight=want_weight, pixel_major=True,
                                        precision=precision)
    _count_convert(x)
    if kernels_supported(C, H * W, x.dtype):
        r = compress_backward_weight(gy, x, a, want_bias, weight, bias, want_weight=want_weight, pixel_major=False,
                                     precision=precision)
        if r is not None:
            return r
    Cp, Pp = _round(C, 32), _round(H * W, 32)
    r = compress_backward_weight(*(_pad_planes(t.to(x.dtype), Cp, Pp) for t in (gy, x, a)), want_bias,
                                 pixel_major=False, precision=precision)
    if r is None:
        raise RuntimeError(f"mrp_gnn: the compress weight-gradient kernels declined the padded shape C={Cp}, HW={Pp}")
    dwp, dbp = r
    dw = torch.cat((dwp[:C, :C], dwp[:C, Cp:Cp + C]), 1)
    return dw, (dbp[:C].contiguous() if dbp is not None else None)


class CompressFunction(torch.autograd.Function):
    """``conv(torch.cat((x, a), 1))`` with autograd, x and a separate (N, C, H, W) tensors."""

    @staticmethod
    def forward(ctx, x, a, weight, bias):
        hip = _PATH[0] != "library"
        cl = hip and _cl_route(x)  # decided once: the backward follows the forward's route
        mode = _PRECISION[0]  # read once: both gradients of this node run in the forward's mode
        y = _fwd(weight, bias, x, a, cl=cl, precision=mode) if hip else _lib_forward(weight, bias, x, a)
        ctx.save_for_backward(x, a, weight)
        ctx.hip, ctx.has_bias, ctx.cl, ctx.precision = hip, bias is not None, cl, mode
        return y

    @staticmethod
    def backward(ctx, gy):
        x, a, weight = ctx.saved_tensors
        gx = ga = dw = db = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gx, ga = _bwd_data(weight, gy, x.dtype, like=x, cl=ctx.cl, precision=ctx.precision) if ctx.hip else \
                _lib_backward_data(weight, gy)
        if ctx.needs_input_grad[2] or (ctx.has_bias and ctx.needs_input_grad[3]):
            dw, db = _bwd_weight(gy, x, a, ctx.has_bias, None, None, cl=ctx.cl, precision=ctx.precision) if ctx.hip \
                else _lib_backward_weight(gy, x, a, ctx.has_bias)
        return gx, ga, dw, db


class LibraryCompressFunction(torch.autograd.Function):
    """``conv(h)`` over a (N, 2C, H, W) concatenation buffer on torch's library GEMMs (the round-2
    path: batched GEMM forward and data gradient, one GEMM with K = N H W for the weight gradient)."""

    @staticmethod
    def forward(ctx, h, weight, bias):
        n, k, H, W = h.shape
        C = weight.shape[0]
        h = h.contiguous()
        w2 = weight.reshape(C, k)
        y = torch.baddbmm(bias.view(1, C, 1), w2.expand(n, C, k), h.view(n, k, H * W)) if bias is not None else \
            torch.bmm(w2.expand(n, C, k), h.view(n, k, H * W))
        ctx.save_for_backward(h, weight)
        ctx.has_bias = bias is not None
        return y.view(n, C, H, W)

    @staticmethod
    def backward(ctx, gy):
        h, weight = ctx.saved_tensors
        n, k, H, W = h.shape
        C = weight.shape[0]
        gy = gy.contiguous()
        dh = dw = db = None
        if ctx.needs_input_grad[0]:
            dh = torch.bmm(weight.reshape(C, k).t().expand(n, k, C), gy.view(n, C, H * W)).view(n, k, H, W)
        if ctx.needs_input_grad[1]:
            g2 = gy.reshape(n, C, H * W).permute(1, 0, 2).reshape(C, -1)
            h2 = h.reshape(n, k, H * W).permute(1, 0, 2).reshape(k, -1)
            dw = torch.mm(g2, h2.t()).view(weight.shape)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = gy.sum((0, 2, 3))
        return dh, dw, db


def compress_1x1(conv: torch.nn.Conv2d, h: torch.Tensor) -> torch.Tensor:
    """``conv(h)`` for the reference's 1x1 compress conv over a (N, 2C, H, W) concatenation h: the
    matrix-core kernels read its two halves in place (``set_compress_path('library')``: torch's
    library GEMMs)."""
    C = h.shape[1] // 2
    half = h.dtype in HALF_DTYPES
    native = h.dtype == torch.float32 or (half and _HALF[0] == "native" and _PATH[0] != "library")
    if not h.is_cuda or not native or h.shape[1] != 2 * C or not conv_is_plain_1x1(conv, C):
        if half and h.is_cuda:
            PATH_COUNTS["torch_16"] += 1
        return conv(h)
    if _PATH[0] == "library":
        return LibraryCompressFunction.apply(h, conv.weight, conv.bias)
    return CompressFunction.apply(h[:, :C], h[:, C:], conv.weight, conv.bias)


class FilmCompressFunction(torch.autograd.Function):
    """``conv(torch.cat((x, film_mean(x, gb)), 1))`` (``models.py:181-184``) with autograd and without
    the concatenation: forward = the aggregation kernel into its own (N, C, H, W) output, then the
    two-source compress.  Backward: ``[gx; ga] = W^T dy`` by the data-gradient kernel, ONE
    aggregation-backward pass with ga as its grad_out and gx as the base of x's gradient (x's two
    gradient terms are never added by a separate kernel), and the weight gradient from x and the
    saved aggregate.  Saves x, gb and the aggregate — not a 2C-channel buffer."""

    @staticmethod
    def forward(ctx, x, gb, weight, bias, csr, mode: int, reducer: str = "mean", scale=None, heads: int = 1):
        from .aggregate import film_attn_forward_into, film_max_forward_into, film_mean_forward_into
        n, C, H, W = x.shape
        hip = _PATH[0] != "library"
        if reducer in ("max", "attn"):
            # the max and attention reducers (mode: their flags, 0 or GB_LOGITS) have NCHW kernels only: a
            # channels_last x is copied first and the layer continues on the NCHW route
            x = x.contiguous()
        # a pixel-major 16-bit x: the pixel-major aggregation into a channels_last aggregate, read in place
        # by the pixel-major compress (no layout copy of x, the aggregate or y)
        cl = hip and _cl_route(x)  # decided once: the backward follows the forward's route
        agg = _empty_cl(x.shape, x.device, x.dtype) if cl else torch.empty(x.shape, device=x.device, dtype=x.dtype)
        attn = None
        if reducer == "max":
            film_max_forward_into(x, gb, csr, mode, agg)
        elif reducer == "attn":
            # the weights: saved for the backward
            attn = film_attn_forward_into(x, gb, csr, mode, agg, scale, heads=heads)
        else:
            film_mean_forward_into(x, gb, csr, mode, agg)
        prec = _PRECISION[0]  # read once: both gradients of this node run in the forward's mode
        y = _fwd(weight, bias, x, agg, cl=cl, precision=prec) if hip else _lib_forward(weight, bias, x, agg)
        ctx.save_for_backward(x, gb, agg, weight, bias, attn)
        ctx.csr, ctx.mode, ctx.has_bias, ctx.hip, ctx.cl, ctx.precision = csr, mode, bias is not None, hip, cl, prec
        # the aggregation step and its backward dispatch on the reducer
        ctx.reducer, ctx.scale, ctx.heads = reducer, scale, heads
        return y

    @staticmethod
    def backward(ctx, gy):
        from .aggregate import film_attn_backward, film_max_backward, film_mean_backward
        x, gb, agg, weight, bias, attn = ctx.saved_tensors
        need_x, need_gb = ctx.needs_input_grad[0], gb is not None and ctx.needs_input_grad[1]
        dx = dgb = dw = db = None
        if need_x or need_gb:
            # ctx.cl: channels_last gx / ga straight into the pixel-major aggregation backward
            gx, ga = _bwd_data(weight, gy, x.dtype, like=x, cl=ctx.cl, precision=ctx.precision) if ctx.hip else \
                _lib_backward_data(weight, gy)
            if ctx.reducer == "max":
                dx, dgb = film_max_backward(ga, x, gb, ctx.csr, ctx.mode, need_x, need_gb,
                                            grad_x_base=gx if need_x else None)
            elif ctx.reducer == "attn":
                dx, dgb = film_attn_backward(ga, x, gb, attn, ctx.csr, ctx.mode, need_x, need_gb,
                                             grad_x_base=gx if need_x else None, scale=ctx.scale, heads=ctx.heads)
            else:
                dx, dgb = film_mean_backward(ga, x, gb, ctx.csr, ctx.mode, need_x, need_gb,
                                             grad_x_base=gx if need_x else None,
                                             pixel_major=ctx.cl)  # else the forward above ran the NCHW kernels
            if dgb is not None:
                dgb = dgb.view(gb.shape).to(gb.dtype)
        if ctx.needs_input_grad[2] or (ctx.has_bias and ctx.needs_input_grad[3]):
            dw, db = _bwd_weight(gy, x, agg, ctx.has_bias and ctx.needs_input_grad[3], weight, bias,
                                 want_weight=ctx.needs_input_grad[2], cl=ctx.cl, precision=ctx.precision) if ctx.hip else \
                _lib_backward_weight(gy, x, agg, ctx.has_bias)
            if not ctx.needs_input_grad[2]:
                dw = None
        return dx, dgb, dw, db, None, None, None, None, None


class FilmWMeanCompressFunction(torch.autograd.Function):
    """``conv(torch.cat((x, film_wmean(x, gb, w)), 1))`` with autograd and without the concatenation, as
    :class:`FilmCompressFunction`: the weighted aggregation into its own buffer, the two-source compress, and
    in backward ONE aggregation-backward pass that also returns the gradient of the sender maps.  NCHW
    kernels only: a channels_last x is copied first."""

    @staticmethod
    def forward(ctx, x, gb, w, weight, bias, csr, flags: int, wagg: int):
        from .aggregate import film_wmean_forward_into
        x = x.contiguous()
        hip = _PATH[0] != "library"
        agg = torch.empty(x.shape, device=x.device, dtype=x.dtype)
        film_wmean_forward_into(x, gb, w, csr, flags, agg, wagg)
        prec = _PRECISION[0]  # read once: both gradients of this node run in the forward's mode
        y = _fwd(weight, bias, x, agg, cl=False, precision=prec) if hip else _lib_forward(weight, bias, x, agg)
        ctx.save_for_backward(x, gb, w, agg, weight, bias)
        ctx.csr, ctx.flags, ctx.wagg, ctx.has_bias, ctx.hip, ctx.precision = csr, flags, wagg, bias is not None, hip, prec
        return y

    @staticmethod
    def backward(ctx, gy):
        from .aggregate import film_wmean_backward
        x, gb, w, agg, weight, bias = ctx.saved_tensors
        need_x, need_gb, need_w = ctx.needs_input_grad[:3]
        dx = dgb = dwt = dw = db = None
        if need_x or need_gb or need_w:
            gx, ga = _bwd_data(weight, gy, x.dtype, like=x, cl=False, precision=ctx.precision) if ctx.hip else \
                _lib_backward_data(weight, gy)
            dx, dgb, dwt = film_wmean_backward(ga, x, gb, w, ctx.csr, ctx.flags, need_x, need_gb, need_w,
                                               grad_x_base=gx if need_x else None, mode=ctx.wagg)
            if dgb is not None:
                dgb = dgb.view(gb.shape).to(gb.dtype)
            if dwt is not None:
                dwt = dwt.view(w.shape)
        if ctx.needs_input_grad[3] or (ctx.has_bias and ctx.needs_input_grad[4]):
            dw, db = _bwd_weight(gy, x, agg, ctx.has_bias and ctx.needs_input_grad[4], weight, bias,
                                 want_weight=ctx.needs_input_grad[3], cl=False, precision=ctx.precision) if ctx.hip else \
                _lib_backward_weight(gy, x, agg, ctx.has_bias)
            if not ctx.needs_input_grad[3]:
                dw = None
        return dx, dgb, dwt, dw, db, None, None, None


def film_compress_supported(conv: torch.nn.Conv2d, x: torch.Tensor) -> bool:
    """Whether :func:`film_compress` takes this layer: fp32, bf16 or fp16 CUDA (N, C, H, W) features and
    a plain 1x1 ``Conv2d(2C, C)`` with fp32 parameters (the matrix-core kernels, on zero-padded operands
    for shapes they do not tile), inside or outside ``torch.autocast``.  Declined, i.e. left to the cat
    kernel followed by ``conv(h)``: a conv whose weight is stored in 16 bits (a module cast with
    ``.to(torch.bfloat16)``), and 16-bit features after ``set_half_compress("torch")``."""
    ok = x.dtype == torch.float32 or (x.dtype in HALF_DTYPES and _HALF[0] == "native")
    return x.dim() == 4 and x.is_cuda and ok and conv_is_plain_1x1(conv, x.shape[1])


def film_compress(conv: torch.nn.Conv2d, x: torch.Tensor, gb, csr, mode: int, reducer: str = "mean",
                  scale=None, weights=None, heads: int = 1) -> torch.Tensor:
    """Autograd form of ``conv(torch.cat((x, film_mean(x, gb)), 1))`` without the concatenation
    (:class:`FilmCompressFunction`); the caller checks :func:`film_compress_supported`.  ``reducer="max"``:
    the aggregate is ``film_max(x, gb)`` and ``mode`` carries its flags (0 or ``GB_LOGITS``);
    ``reducer="attn"``: likewise ``film_attn(x, gb, scale=scale, heads=heads)``; ``reducer="wmean"``: the aggregate is
    ``film_wmean(x, gb, weights)`` with ``mode`` = ``MODE_FILM_MEAN`` or ``MODE_FILM_SUM`` (the normalised or
    the plain weighted sum), optionally with ``GB_LOGITS`` (:class:`FilmWMeanCompressFunction`)."""
    if reducer not in ("mean", "max", "attn", "wmean"):
        raise ValueError(f'reducer must be "mean", "max", "attn" or "wmean", got {reducer!r}')
    if isinstance(heads, bool) or not isinstance(heads, int) or heads < 1:
        raise ValueError(f"heads must be a positive int, got {heads!r}")
    if heads != 1 and reducer != "attn":
        raise ValueError('heads belong to reducer="attn"')
    if x.dim() == 4 and x.shape[1] % heads:
        raise ValueError(f"heads must divide the channels: C = {x.shape[1]}, heads = {heads}")
    if (weights is not None) != (reducer == "wmean"):
        raise ValueError('weights belong to reducer="wmean", which needs them')
    if reducer == "wmean":
        if scale is not None:
            raise ValueError('scale belongs to reducer="attn"')
        base = int(mode) & ~_lib.GB_LOGITS
        if base not in (_lib.MODE_FILM_MEAN, _lib.MODE_FILM_SUM):
            raise ValueError(f'reducer="wmean" takes MODE_FILM_MEAN or MODE_FILM_SUM (with or without GB_LOGITS) '
                             f'as mode, got {int(mode):#x}')
        if gb is None:
            raise ValueError("gamma/beta tensor required for film_wmean")
        gb = gb.reshape(csr.num_edges, x.shape[1], 2)
        wagg = _lib.WAGG_MEAN if base == _lib.MODE_FILM_MEAN else _lib.WAGG_SUM
        return FilmWMeanCompressFunction.apply(x, gb, weights, conv.weight, conv.bias, csr,
                                               int(mode) & _lib.GB_LOGITS, wagg)
    if reducer in ("max", "attn"):
        # `mode` then carries the operator's flags, not a MODE_* value of the mean: say so here, not deep in the launch
        if int(mode) not in (0, _lib.GB_LOGITS):
            raise ValueError(f'reducer="{reducer}" takes flags 0 or GB_LOGITS ({_lib.GB_LOGITS:#x}) as mode, '
                             f'got {int(mode):#x}')
        if gb is None:
            raise ValueError(f"gamma/beta tensor required for film_{reducer}")
    if scale is not None and reducer != "attn":
        raise ValueError('scale belongs to reducer="attn"')
    if gb is not None:
        gb = gb.reshape(csr.num_edges, x.shape[1], 2)
    return FilmCompressFunction.apply(x, gb, conv.weight, conv.bias, csr, mode, reducer, scale, heads)
