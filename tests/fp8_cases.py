"""Test infrastructure shared by the FP8-message tests (test_capi_fp8.py, test_fp8_quant_cpu.py,
test_gpu_fp8_messages.py): the two OCP formats, their decode tables, the cases of ``half_cases`` quantised on
the CPU with torch's own cast (so no test rests on a GPU cast), the FP8 placements, and cached float64
references on the dequantised values (computed once per case, never modified).

Bars, all from the number formats:

* quantiser: ``|x^ - x| <= u |x| + s m / 2 + 2^-22 |x|`` per element, with u half an ulp of the format
  (E4M3: 2^-4, E5M2: 2^-3), m its smallest subnormal (2^-9, 2^-16) — ``s m / 2`` is the rounding error in the
  subnormal range — and 2^-22 |x| the two fp32 roundings (the division by s, the product with s);
* aggregate of the quantised features against float64 on x^: ``half_cases``' bars, ``u_T |ref| + 1e-5
  max|ref|`` with ``u_fp32 = 0``;
* the contract itself is bit equality and has no bar.
"""
import functools

import numpy as np
import torch

import mrp_gnn_amd as m
import half_cases as hc
import oracle

#: fmt -> (torch dtype, enum mrp_qdtype, largest finite value, u = half an ulp, m = smallest subnormal)
FORMATS = {
    "e4m3": (torch.float8_e4m3fn, 0, 448.0, 2.0 ** -4, 2.0 ** -9),
    "e5m2": (torch.float8_e5m2, 1, 57344.0, 2.0 ** -3, 2.0 ** -16),
}
OUT_DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
UNIT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
MODES = ("film_mean", "film_sum", "copy_mean")

#: half_cases.CASES plus FP8 views 8, 4 and 1 bytes into a flat buffer (the geometry of case b)
CASES = dict(hc.CASES)
for _off in (8, 4, 1):
    CASES[f"v{_off}"] = (hc.CASES["b"][0], 16, 8, 8, f"FP8 codes {_off} byte(s) into a flat buffer")
_BYTE_OFFSET = {"v8": 8, "v4": 4, "v1": 1, "i4": 4, "i1": 1}  # i4 / i1: half_cases' element offsets, in bytes here


def all_codes():
    """The 256 codes, in order, as uint8."""
    return torch.arange(256, dtype=torch.int16).to(torch.uint8)


def decode_ocp(fmt):
    """torch's own decode of the 256 codes of an OCP format (fp32)."""
    return all_codes().view(FORMATS[fmt][0]).float()


def decode_fnuz(fmt):
    """The 256 codes under the FNUZ reading of the same bit layout (the encoding these kernels must NOT use):
    exponent bias one larger than OCP's (E4M3: 8, E5M2: 16), no infinities, no negative zero, the single NaN
    at 0x80, every other exponent-all-ones code an ordinary number."""
    ebits, mbits, bias = (4, 3, 8) if fmt == "e4m3" else (5, 2, 16)
    out = np.zeros(256, np.float64)
    for c in range(256):
        if c == 0x80:
            out[c] = np.nan
            continue
        sign = -1.0 if c & 0x80 else 1.0
        e = (c >> mbits) & ((1 << ebits) - 1)
        f = c & ((1 << mbits) - 1)
        if e == 0:
            out[c] = sign * f * 2.0 ** (1 - bias - mbits)
        else:
            out[c] = sign * (1.0 + f * 2.0 ** -mbits) * 2.0 ** (e - bias)
    return torch.from_numpy(out).float()


@functools.lru_cache(maxsize=None)
def graph(name):
    return CASES[name][0]()


def shape(name):
    _, C, H, W, _ = CASES[name]
    return graph(name).num_nodes(), C, H, W


@functools.lru_cache(maxsize=None)
def host_inputs(name, fmt, per="channel"):
    """(xq, s, xhat, gb, z) on the CPU: features drawn in fp32, quantised by ``quantize_features`` on the
    CPU (torch's cast); xhat = ``dequantize_features`` (fp32); gb uniform (0, 1) with gb == sigmoid(z)."""
    n, C, H, W = shape(name)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 131 + (7 if fmt == "e4m3" else 11))
    x = torch.randn(n, C, H, W, generator=gen) * 3.0
    z = torch.randn(graph(name).num_edges(), C, 2, generator=gen)
    xq, s = m.quantize_features(x, fmt, per)
    return xq, s, m.dequantize_features(xq, s), torch.sigmoid(z), z


@functools.lru_cache(maxsize=None)
def ref64(name, fmt, mode="film_mean"):
    """The float64 oracle on the dequantised features."""
    _, _, xhat, gb, _ = host_inputs(name, fmt)
    src, dst = (t.numpy() for t in graph(name).edges())
    return oracle.film_aggregate(xhat.double(), gb.double(), src, dst, mode)


def embed(name, xq, dev):
    """The FP8 tensor a case hands the kernel, holding xq's codes, on ``dev``: case h a channel slice of a
    wider tensor (node stride != C P), i4 / i1 / v8 / v4 / v1 a view that many bytes into a flat buffer."""
    raw = xq.view(torch.uint8).to(dev)
    n, C, H, W = raw.shape
    if name == "h":
        leaf = torch.zeros(n, C + 2, H, W, dtype=torch.uint8, device=dev)
        leaf[:, 1:C + 1] = raw
        return leaf[:, 1:C + 1].view(xq.dtype)
    if name in _BYTE_OFFSET:
        off = _BYTE_OFFSET[name]
        leaf = torch.zeros(raw.numel() + 16, dtype=torch.uint8, device=dev)
        assert leaf.data_ptr() % 16 == 0
        leaf[off:off + raw.numel()] = raw.reshape(-1)
        return leaf[off:off + raw.numel()].view(n, C, H, W).view(xq.dtype)
    return raw.clone().view(xq.dtype)


def bits(t):
    """Raw bits on the CPU (NaN-safe, sign-of-zero-exact comparison)."""
    t = t.detach().contiguous().cpu()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def assert_bars(got, ref, T, what=""):
    """|got - ref| <= u_T |ref| + 1e-5 max|ref| for every element (u_fp32 = 0)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape
    bound = UNIT[T] * ref.abs() + 1e-5 * ref.abs().max()
    excess = float(((got - ref).abs() - bound).max())
    assert excess <= 0.0, (what, excess, float((got - ref).abs().max()))
