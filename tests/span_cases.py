"""Test infrastructure for operands that span more than 2 and 4 GiB (``test_gpu_large_span.py``,
``test_capi_large_span.py``): the entry points of ``include/mrp_gnn.h`` see only pointers and strides, so
a multi-GiB span costs no compute — a few tiny node blocks placed far apart by a large node stride.

**Arena** (:class:`Arena`): one ``torch.uint8`` allocation laid out as

    [2 GiB guard][working span: 64 encoder row strides + 64 MiB][256 MiB tail]     about 10.8 GiB

with every byte the sentinel ``0xCB`` (a finite negative value in fp32, bf16 and fp16).  Views start after
the guard, so an offset that is wrong with either sign, or truncated to 32 bits, lands inside the arena
and shows as a wrong value or a touched sentinel, not as a fault.

**Placer** (:meth:`Arena.place` / :meth:`Arena.reserve`): node ``i`` of a logical (n, C, H, W) tensor —
NCHW blocks or pixel-major rows — lies at ``view base + tensor offset + i * S`` with
``S = 2^28 bytes + 64 KiB``: a multiple of 16 bytes and of 8 elements in every dtype.  Node 8 onward is
beyond 2^31 bytes, node 16 onward beyond 2^32 bytes (and, for the 16-bit types, beyond 2^31 elements).
Tensor offsets are whole MiB slots (at most 63), so blocks of different tensors never overlap: two
blocks could only meet if a slot difference (< 64 MiB) equalled a multiple of S.  The encoder's row-strided
matrices (h^T, dh^T: C rows; dz^T: 2C rows of E floats) are placed the same way, a row per "node", with the
row stride ``2^27 bytes + 8 MiB``: row 16 is past 2 GiB, row 31 past 4 GiB, and dz^T's 64 rows end at
8.4 GiB — which sets the working span.  One aggregation case (``complete_1x16_s512``) has a stride of its own,
``2^29 bytes + 64 KiB``: a single 16-node graph whose node 4 onward lies beyond 2^31 and node 8 onward beyond
2^32 bytes *from the graph's own first node* (with S no graph reaches past 11 S = 2.75 GiB from its first node, so
a 64-bit per-graph base with a 32-bit per-node offset would pass every other case); its 15 strides and the
slots end inside the working span (asserted below).  The fp32 sender maps ``w`` / ``grad_w`` of the weighted
families are placed like any feature tensor, as (n, 1, H, W).

**Checker** (:meth:`Arena.check`): reads the outputs back, restores the sentinel over every region the
call was allowed to write, compares the input blocks with their original bits and scans the whole arena:
the number of non-sentinel bytes must be exactly the inputs' own.

**Decline table** (:data:`EXPECTED`): the return code of every (entry point, dtype, case), written out
from the limits ``include/mrp_gnn.h`` states — not from what the library answers.
"""
import ctypes

import pytest
import torch

GUARD = 2 << 30
NODE_STRIDE = (1 << 28) + (64 << 10)  # S, bytes
MAX_NODES = 24
ROW_STRIDE = (1 << 27) + (8 << 20)  # the encoder's row stride, bytes
MAX_ROWS = 64
SLOT = 1 << 20  # tensor offsets: whole MiB
MAX_SLOTS = 64
WORK = max(MAX_NODES * NODE_STRIDE, MAX_ROWS * ROW_STRIDE) + MAX_SLOTS * SLOT
TAIL = 256 << 20
TOTAL = GUARD + WORK + TAIL
SENTINEL = 0xCB
_SENT64 = int.from_bytes(bytes([SENTINEL]) * 8, "little", signed=True)
_CHUNK = 512 << 20  # bytes per scan step
assert NODE_STRIDE % 16 == 0 and TOTAL % 8 == 0

NS = 801  # hipErrorNotSupported
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
ENUM = {"f32": 0, "bf16": 1, "f16": 2}  # enum mrp_dtype


def bits(t):
    """Raw bits of a tensor on the CPU (NaN-safe, sign-of-zero-exact comparison)."""
    t = t.detach().contiguous().cpu()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


class Placed:
    """A logical (n, C, H, W) tensor of the arena: node i at ``off + i * stride_bytes`` after the guard.
    ``layout`` "nchw": a contiguous C H W block per node; "cl": H W pixel rows of C contiguous channels,
    ``ps`` elements apart (2C: one half of a channels_last concatenation buffer)."""

    def __init__(self, arena, shape, dtype, off, layout, ps, stride_bytes, data):
        self.arena, self.shape, self.dtype, self.off, self.layout = arena, tuple(shape), dtype, off, layout
        self.stride_bytes, self.data = stride_bytes, data
        self.es = torch.empty((), dtype=dtype).element_size()
        n, C, H, W = self.shape
        self.ps = (C if ps is None else ps) if layout == "cl" else None
        assert off % 16 == 0 and stride_bytes % self.es == 0
        assert GUARD + off + (n - 1) * stride_bytes + self._block_bytes() <= GUARD + WORK

    def _block_bytes(self):
        n, C, H, W = self.shape
        return (C * H * W if self.layout == "nchw" else (H * W - 1) * self.ps + C) * self.es

    @property
    def address(self):
        return self.arena.buf.data_ptr() + GUARD + self.off

    @property
    def ptr(self):
        return ctypes.c_void_p(self.address)

    @property
    def ns(self):  # node stride in elements
        return self.stride_bytes // self.es

    def node(self, i):
        """Node i's (C, H, W) block as a device view."""
        n, C, H, W = self.shape
        start = GUARD + self.off + i * self.stride_bytes
        flat = self.arena.buf[start:start + self._block_bytes()].view(self.dtype)
        if self.layout == "nchw":
            return flat.view(C, H, W)
        return flat.as_strided((C, H, W), (1, W * self.ps, self.ps))

    def view(self):
        """The whole tensor as one strided (n, C, H, W) torch view (for the Python routes)."""
        n, C, H, W = self.shape
        flat = self.arena.buf[GUARD + self.off:GUARD + WORK].view(self.dtype)
        inner = (H * W, W, 1) if self.layout == "nchw" else (1, W * self.ps, self.ps)
        return flat.as_strided(self.shape, (self.ns,) + inner)

    def write(self, t):
        for i in range(self.shape[0]):
            self.node(i).copy_(t[i])

    def read(self):
        return torch.stack([self.node(i).cpu() for i in range(self.shape[0])])

    def restore(self):
        """The sentinel over exactly this tensor's elements."""
        n, C, H, W = self.shape
        for i in range(n):
            start = GUARD + self.off + i * self.stride_bytes
            raw = self.arena.buf[start:start + self._block_bytes()]
            if self.layout == "nchw":
                raw.fill_(SENTINEL)
            else:
                raw.as_strided((H * W, C * self.es), (self.ps * self.es, 1)).fill_(SENTINEL)


class Arena:
    def __init__(self, dev):
        free, _total = torch.cuda.mem_get_info(dev)
        if free < TOTAL + (2 << 30):
            pytest.skip(f"the span arena needs {TOTAL >> 20} MiB + 2 GiB of free device memory, {free >> 20} MiB free")
        self.dev = dev
        self.buf = torch.full((TOTAL,), SENTINEL, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.placed, self._slot = [], 0

    def _new(self, shape, dtype, layout, ps, stride_bytes, data, beside):
        if beside is None:  # a slot of its own
            assert self._slot < MAX_SLOTS
            off = self._slot * SLOT
            self._slot += 1
        else:  # the second half of `beside`'s pixel rows: a channels_last concatenation buffer
            assert layout == "cl" and beside.layout == "cl" and ps == beside.ps == 2 * beside.shape[1]
            assert beside.stride_bytes == stride_bytes
            off = beside.off + beside.shape[1] * beside.es
        p = Placed(self, shape, dtype, off, layout, ps, stride_bytes, data)
        self.placed.append(p)
        return p

    def place(self, t, layout="nchw", ps=None, stride_bytes=NODE_STRIDE, beside=None):
        """Write the CPU tensor t (n, C, H, W) sparsely into the arena (an input)."""
        p = self._new(t.shape, t.dtype, layout, ps, stride_bytes, t.clone(), beside)
        p.write(t)
        return p

    def reserve(self, shape, dtype, layout="nchw", ps=None, stride_bytes=NODE_STRIDE, beside=None):
        """An output: its blocks keep the sentinel until a kernel writes them."""
        return self._new(shape, dtype, layout, ps, stride_bytes, None, beside)

    def dirty_bytes(self):
        """Non-sentinel bytes of the whole arena (guard and tail included)."""
        torch.cuda.synchronize(self.dev)
        words = self.buf.view(torch.int64)
        step = _CHUNK // 8
        dirty = []  # the 8-byte words that differ, then their bytes
        for s in range(0, words.numel(), step):
            w = words[s:s + step]
            dirty.append(w[w != _SENT64])
        return int((torch.cat(dirty).view(torch.uint8) != SENTINEL).sum())

    def check(self, inputs, outputs, untouched=False):
        """After a call: the outputs' values (CPU tensors, in order).  Asserts that the inputs hold their
        original bits and that, with the outputs' elements restored to the sentinel, no other byte of the
        arena differs from it.  ``untouched``: the call declined, so the outputs too must be sentinel."""
        torch.cuda.synchronize(self.dev)
        outs = [o.read() for o in outputs]
        if untouched:
            for o, got in zip(outputs, outs):
                assert bool((bits(got).view(torch.uint8) == SENTINEL).all()), "a declined call wrote an output"
        for o in outputs:
            o.restore()
        own = 0
        for p in inputs:
            assert torch.equal(bits(p.read()), bits(p.data)), "an input block changed"
            own += int((bits(p.data).view(torch.uint8) != SENTINEL).sum())
        dirty = self.dirty_bytes()
        assert dirty == own, f"{dirty - own} bytes touched outside the permitted blocks"
        return outs

    def clear(self):
        """Restore every placement of the test and start the slots over."""
        for p in self.placed:
            p.restore()
        self.placed, self._slot = [], 0
        if self.dirty_bytes():  # a failed test left stray bytes: the next one starts clean all the same
            self.buf.fill_(SENTINEL)


# ---- cases ------------------------------------------------------------------------------------------------
#: compress cases: name -> (nodes, C, H, W)
COMPRESS = {
    "n18_c32_p32": (18, 32, 4, 8),     # fp32 MFMA and 16-bit: 18 nodes, 4.25 GiB
    "n7_c32_p32": (7, 32, 4, 8),       # 16-bit: 1.75 GiB, inside launch_nn's output guard
    "n8_c32_p32": (8, 32, 4, 8),       # 16-bit: 7 S + a block < 2^31 bytes, the most nodes the guard accepts
    "n18_c64_p32": (18, 64, 4, 8),     # split-bf16 (the weight gradient needs C % 64 == 0)
    "n18_c256_p32": (18, 256, 4, 8),   # split-bf16 forward, M % 256 == 0: mf16_ok's span test decides the form
    "n18_c32_p49": (18, 32, 7, 7),     # 16-bit pixel-major: stages cross node boundaries
}

#: aggregation cases: name -> (graph sizes, k of k-NN or None, C, H, W, node stride in elements beyond the
#: case's base stride)
AGG = {
    "complete_3x8": ((8, 8, 8), None, 8, 8, 8, 0),
    "complete_2x12": ((12, 12), None, 8, 8, 8, 0),
    "knn4_2x12": ((12, 12), 4, 8, 8, 8, 0),
    "ragged_8_5_1_8": ((8, 5, 1, 8), None, 8, 8, 8, 0),
    "scalar_3x8_p15": ((8, 8, 8), None, 8, 3, 5, 1),  # P = 15 and an odd node stride (S + one element)
    # P = 80: two 64-pixel attention tiles, the second ragged; C = 17: two channel blocks of 16, the second ragged
    "wide_3x8_c17_p80": ((8, 8, 8), None, 17, 8, 10, 0),
    # one graph that by itself spans 2^32 bytes: node 4 onward is more than 2^31 bytes, node 8 onward more than
    # 2^32 bytes from the graph's first node (AGG_STRIDE)
    "complete_1x16_s512": ((16,), None, 8, 8, 8, 0),
}
#: the first five: S is the stride, a graph's farthest node at most 11 S = 2.75 GiB from its first
AGG_S = tuple(AGG)[:5]
#: cases whose base node stride is not S: name -> bytes
AGG_STRIDE = {"complete_1x16_s512": (1 << 29) + (64 << 10)}
AGG_CL = ("complete_3x8", "knn4_2x12")
#: the pixel-major span runs: those and the self-spanning graph
AGG_CL_SPAN = AGG_CL + ("complete_1x16_s512",)
#: the graph sets of the max / attention / weighted families' span tests: all seven
AGG_FAMILIES = tuple(AGG)


def agg_stride(case, es):
    """Node stride in bytes of an aggregation case's tensor of ``es``-byte elements."""
    return AGG_STRIDE.get(case, NODE_STRIDE) + AGG[case][5] * es


def agg_node_offsets(case, es):
    """[(byte offset of node i from its tensor's first node, from its own graph's first node)] of a case."""
    s, out, first = agg_stride(case, es), [], 0
    for k in AGG[case][0]:
        out += [((first + i) * s, i * s) for i in range(k)]
        first += k
    return out


# the self-spanning graph ends inside the working span: 15 strides, the last slot, one (C, H, W) fp32 block
assert 15 * AGG_STRIDE["complete_1x16_s512"] + (MAX_SLOTS - 1) * SLOT + 8 * 8 * 8 * 4 <= WORK
assert all(s % 16 == 0 for s in AGG_STRIDE.values())

#: encoder cases: name -> (C, E); h^T / dh^T (C, E) and dz^T (2C, E) with rows ROW_STRIDE bytes apart
ENCODER = {"enc_c32_e64": (32, 64)}

#: (entry point, dtype, case) -> expected return code.  Limits the header states and these cases exceed:
#: mrp_compress_fwd_t / _bwd_data_t decline "an output node range beyond 31-bit byte offsets" — 18 nodes put
#: the last output block 17 S = 4.25 GiB from the first, 7 nodes 6 S = 1.5 GiB, 8 nodes 7 S = 1.75 GiB (9 nodes
#: would be the first to decline: test_capi_large_span.py).  Nothing else here is declined:
#: the fp32 MFMA kernels address one column tile's (or one split's) node range with 31-bit offsets, not the
#: tensor's; the split-bf16, the pixel-major and the 16-bit weight-gradient kernels, the aggregation kernels of
#: every family (mean, max, attention, confidence-weighted, confidence-gated: rows added below the table) and
#: the encoder's row-strided kernels form 64-bit node / row addresses.  The mean's matrix-core backward alone
#: keeps 32-bit offsets across a graph's nodes, and where they do not fit (``complete_1x16_s512``) its launcher
#: runs the VALU kernels instead: success, not a decline.
EXPECTED = {
    ("mrp_compress_fwd", "f32", "n18_c32_p32"): 0,
    ("mrp_compress_bwd_data", "f32", "n18_c32_p32"): 0,
    ("mrp_compress_bwd_weight", "f32", "n18_c32_p32"): 0,
    ("mrp_compress_fwd_split", "f32", "n18_c64_p32"): 0,
    ("mrp_compress_bwd_data_split", "f32", "n18_c64_p32"): 0,
    ("mrp_compress_bwd_weight_split", "f32", "n18_c64_p32"): 0,
    ("mrp_compress_fwd_split", "f32", "n18_c256_p32"): 0,
    ("mrp_compress_fwd_t", "bf16", "n18_c32_p32"): NS,
    ("mrp_compress_fwd_t", "f16", "n18_c32_p32"): NS,
    ("mrp_compress_bwd_data_t", "bf16", "n18_c32_p32"): NS,
    ("mrp_compress_bwd_data_t", "f16", "n18_c32_p32"): NS,
    ("mrp_compress_bwd_weight_t", "bf16", "n18_c32_p32"): 0,
    ("mrp_compress_bwd_weight_t", "f16", "n18_c32_p32"): 0,
    ("mrp_compress_fwd_t", "bf16", "n7_c32_p32"): 0,
    ("mrp_compress_fwd_t", "f16", "n7_c32_p32"): 0,
    ("mrp_compress_bwd_data_t", "bf16", "n7_c32_p32"): 0,
    ("mrp_compress_bwd_data_t", "f16", "n7_c32_p32"): 0,
    ("mrp_compress_bwd_weight_t", "bf16", "n7_c32_p32"): 0,
    ("mrp_compress_bwd_weight_t", "f16", "n7_c32_p32"): 0,
    ("mrp_compress_fwd_t", "bf16", "n8_c32_p32"): 0,
    ("mrp_compress_fwd_t", "f16", "n8_c32_p32"): 0,
    ("mrp_compress_bwd_data_t", "bf16", "n8_c32_p32"): 0,
    ("mrp_compress_bwd_data_t", "f16", "n8_c32_p32"): 0,
    ("mrp_compress_bwd_weight_t", "bf16", "n8_c32_p32"): 0,
    ("mrp_compress_bwd_weight_t", "f16", "n8_c32_p32"): 0,
    ("mrp_compress_fwd_cl", "bf16", "n18_c32_p49"): 0,
    ("mrp_compress_fwd_cl", "f16", "n18_c32_p49"): 0,
    ("mrp_compress_bwd_data_cl", "bf16", "n18_c32_p49"): 0,
    ("mrp_compress_bwd_data_cl", "f16", "n18_c32_p49"): 0,
    ("mrp_compress_bwd_weight_cl", "bf16", "n18_c32_p49"): 0,
    ("mrp_compress_bwd_weight_cl", "f16", "n18_c32_p49"): 0,
    ("mrp_film_mean_fwd_t", "f32", "complete_3x8"): 0,
    ("mrp_film_mean_fwd_t", "bf16", "complete_3x8"): 0,
    ("mrp_film_mean_fwd_t", "f16", "complete_3x8"): 0,
    ("mrp_film_mean_bwd_t", "f32", "complete_3x8"): 0,
    ("mrp_film_mean_bwd_t", "bf16", "complete_3x8"): 0,
    ("mrp_film_mean_bwd_t", "f16", "complete_3x8"): 0,
    ("mrp_film_mean_fwd_t", "f32", "complete_2x12"): 0,
    ("mrp_film_mean_fwd_t", "bf16", "complete_2x12"): 0,
    ("mrp_film_mean_fwd_t", "f16", "complete_2x12"): 0,
    ("mrp_film_mean_bwd_t", "f32", "complete_2x12"): 0,
    ("mrp_film_mean_bwd_t", "bf16", "complete_2x12"): 0,
    ("mrp_film_mean_bwd_t", "f16", "complete_2x12"): 0,
    ("mrp_film_mean_fwd_t", "f32", "knn4_2x12"): 0,
    ("mrp_film_mean_fwd_t", "bf16", "knn4_2x12"): 0,
    ("mrp_film_mean_fwd_t", "f16", "knn4_2x12"): 0,
    ("mrp_film_mean_bwd_t", "f32", "knn4_2x12"): 0,
    ("mrp_film_mean_bwd_t", "bf16", "knn4_2x12"): 0,
    ("mrp_film_mean_bwd_t", "f16", "knn4_2x12"): 0,
    ("mrp_film_mean_fwd_t", "f32", "ragged_8_5_1_8"): 0,
    ("mrp_film_mean_fwd_t", "bf16", "ragged_8_5_1_8"): 0,
    ("mrp_film_mean_fwd_t", "f16", "ragged_8_5_1_8"): 0,
    ("mrp_film_mean_bwd_t", "f32", "ragged_8_5_1_8"): 0,
    ("mrp_film_mean_bwd_t", "bf16", "ragged_8_5_1_8"): 0,
    ("mrp_film_mean_bwd_t", "f16", "ragged_8_5_1_8"): 0,
    ("mrp_film_mean_fwd_t", "f32", "scalar_3x8_p15"): 0,
    ("mrp_film_mean_fwd_t", "bf16", "scalar_3x8_p15"): 0,
    ("mrp_film_mean_fwd_t", "f16", "scalar_3x8_p15"): 0,
    ("mrp_film_mean_bwd_t", "f32", "scalar_3x8_p15"): 0,
    ("mrp_film_mean_bwd_t", "bf16", "scalar_3x8_p15"): 0,
    ("mrp_film_mean_bwd_t", "f16", "scalar_3x8_p15"): 0,
    ("mrp_film_mean_fwd_cl", "f32", "complete_3x8"): 0,
    ("mrp_film_mean_fwd_cl", "bf16", "complete_3x8"): 0,
    ("mrp_film_mean_fwd_cl", "f16", "complete_3x8"): 0,
    ("mrp_film_mean_bwd_cl", "f32", "complete_3x8"): 0,
    ("mrp_film_mean_bwd_cl", "bf16", "complete_3x8"): 0,
    ("mrp_film_mean_bwd_cl", "f16", "complete_3x8"): 0,
    ("mrp_film_mean_fwd_cl", "f32", "knn4_2x12"): 0,
    ("mrp_film_mean_fwd_cl", "bf16", "knn4_2x12"): 0,
    ("mrp_film_mean_fwd_cl", "f16", "knn4_2x12"): 0,
    ("mrp_film_mean_bwd_cl", "f32", "knn4_2x12"): 0,
    ("mrp_film_mean_bwd_cl", "bf16", "knn4_2x12"): 0,
    ("mrp_film_mean_bwd_cl", "f16", "knn4_2x12"): 0,
    ("mrp_edge_encoder_fwd_split_train", "f32", "enc_c32_e64"): 0,
    ("mrp_edge_encoder_bwd_prep", "f32", "enc_c32_e64"): 0,
    ("mrp_edge_encoder_bwd_t", "f32", "enc_c32_e64"): 0,
    ("mrp_edge_encoder_bwd_pose", "f32", "enc_c32_e64"): 0,
}
# The graph that spans 2^32 bytes by itself, mrp_film_mean_*: the header states no span limit for the typed and
# the pixel-major mean entry points (the matrix-core backward's 32-bit lane offsets are the launcher's own affair:
# where 15 node strides do not fit it must run the VALU kernels, not decline).
EXPECTED.update({(e, k, "complete_1x16_s512"): 0 for k in DTYPES for e in (
    "mrp_film_mean_fwd_t", "mrp_film_mean_bwd_t", "mrp_film_mean_fwd_cl", "mrp_film_mean_bwd_cl")})
#: the max-pooled, attention-pooled, confidence-weighted and confidence-gated aggregations
FAMILY_ENTRIES = {fam: (f"mrp_film_{fam}_fwd", f"mrp_film_{fam}_bwd") for fam in ("max", "attn", "wmean", "wattn")}
# The header declares no span limit for any of the eight ("64-bit node offsets"; node strides are int64_t elements
# and nothing is said to be declined for their size): every dtype, every graph set, 0.
EXPECTED.update({(e, k, case): 0 for es in FAMILY_ENTRIES.values() for e in es for k in DTYPES
                 for case in AGG_FAMILIES})


def expected(entry, key, case):
    return EXPECTED[(entry, key, case)]


def declining():
    """The rows of the table that decline."""
    return sorted(k for k, v in EXPECTED.items() if v != 0)
