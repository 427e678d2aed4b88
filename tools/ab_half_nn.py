#!/usr/bin/env python3
"""Kernel lab (not product code): the 16-bit compress forward and both gradients of the product library
(A) against a variant library (B, tools/build_variant_lib.py) in one process, the two taking turns call
by call (tools/bench_half_io.py's method: hipEvents, 5 warm-ups, median of ``iters``, operand sets rotated
over > 512 MB), at the configs[1] / [2] / [4] layer shapes; outputs compared bit for bit.  With ``cl`` the
operands are channels_last, so the two libraries' pixel-major kernels (compress_half_cl.hip) are timed.
AB_LIB_A=<library> in the environment takes that library as A instead (a control: a library against a copy of
itself shows the spread of the B/A ratios on the machine at hand).
usage: python tools/ab_half_nn.py tools/bin/<variant>.so [iters] [cl]"""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mrp_gnn_amd import _lib, aggregate, compress  # noqa: E402
from tools.bench_half_io import MIN_FOOTPRINT, timed_interleaved  # noqa: E402

lib_a = _lib.load_library(os.path.abspath(os.environ["AB_LIB_A"])) if "AB_LIB_A" in os.environ else _lib.load_library()
lib_b = ctypes.CDLL(os.path.abspath(sys.argv[1]))
_lib._declare(lib_b)
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 50
layout = torch.channels_last if len(sys.argv) > 3 and sys.argv[3] == "cl" else torch.contiguous_format
dev = torch.device("cuda:0")
stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
block_a = torch.empty(256 << 20, device=dev, dtype=torch.uint8)
block_b = torch.empty_like(block_a)


def blocker():
    for _ in range(40):
        _lib.check(lib_a.mrp_stream_copy(aggregate._ptr(block_a), aggregate._ptr(block_b), block_a.numel(), stream),
                   "mrp_stream_copy")


def use(lib):
    def setup():
        _lib._lib = lib
    return setup


gen = torch.Generator(device=dev).manual_seed(0)
with torch.no_grad():
    for name, Nt, C, H in (("configs1", 128, 512, 32), ("configs2", 256, 1280, 8), ("configs4", 128, 1024, 16)):
        w = torch.randn(C, 2 * C, 1, 1, device=dev, generator=gen) / (2 * C) ** 0.5
        b = torch.randn(C, device=dev, generator=gen)
        for label, T in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
            k = max(2, -(-MIN_FOOTPRINT // (3 * Nt * C * H * H * 2)) + 1)
            sets = [tuple(torch.randn(Nt, C, H, H, device=dev, generator=gen).to(T).contiguous(memory_format=layout)
                          for _ in range(3)) for _ in range(k)]
            fwd = [(lambda x=x, a=a: compress.compress_forward(w, b, x, a)) for x, a, _ in sets]
            dgr = [(lambda gy=gy: compress.compress_backward_data(w, gy)) for _, _, gy in sets]
            wgr = [(lambda x=x, a=a, gy=gy: compress.compress_backward_weight(gy, x, a)) for x, a, gy in sets]
            res = {}
            for op, calls in (("fwd", fwd), ("dgrad", dgr), ("wgrad", wgr)):
                res[op] = timed_interleaved({"A": (use(lib_a), calls), "B": (use(lib_b), calls)}, iters, blocker)
            outs = {}
            for lab, lib in (("A", lib_a), ("B", lib_b)):
                _lib._lib = lib
                outs[lab] = (compress.compress_forward(w, b, *sets[0][:2]),) + compress.compress_backward_data(w, sets[0][2]) \
                    + compress.compress_backward_weight(sets[0][2], *sets[0][:2])
            _lib._lib = lib_a
            same = all(torch.equal(p.view(torch.int16), q.view(torch.int16)) for p, q in zip(outs["A"], outs["B"]))
            print(f"{name} {label}  " + "  ".join(f"{op} A {t['A']:7.1f} B {t['B']:7.1f} us (B/A {t['B'] / t['A']:.3f})"
                                                   for op, t in res.items()) + f"  outputs bit-identical {same}", flush=True)
            del sets, fwd, dgr, wgr, outs
            torch.cuda.empty_cache()
