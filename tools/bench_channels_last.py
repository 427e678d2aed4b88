"""The FiLM-mean aggregation on channels_last feature maps: native pixel-major kernels against the
convert-first route, the NCHW kernels and a streaming copy, timed in one run on one GPU.

For each shape of ``tools/bench_half_io.py`` and each feature dtype, forward and backward (grad_x and
grad_gb), these legs take turns call by call in one timed loop (drift of the box hits all alike):

* ``native``        the pixel-major kernels (``mrp_film_mean_fwd_cl`` / ``_bwd_cl``) on channels_last tensors;
* ``convert``       what ``set_channels_last("convert")`` does with the same tensors, i.e. the route before
                    the pixel-major kernels existed: ``.contiguous()`` copies, then the NCHW kernels;
* ``convert_back``  ``convert`` plus turning the result (out / grad_x) into channels_last again: what a
                    channels_last consumer paid;
* ``nchw``          the NCHW kernels on NCHW tensors of the same values (the yardstick);
* ``copy``          ``mrp_stream_copy`` over the algorithmic bytes (forward: x read + out written; backward:
                    grad_out and x read + grad_x written).

Protocol: hipEvents around every call, the host running ahead of the device behind a queue of copies; 5
warm-ups per leg; the median of ``--iters`` (>= 50) timed calls; operand sets rotated over more than 512 MB.

Prints one JSON line and writes ``profiles/channels_last_bench.json``.

    python tools/bench_channels_last.py [--iters 50] [--shapes headline,small_planes,...] [--out PATH]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from mrp_gnn_amd import _lib, aggregate  # noqa: E402
from bench_half_io import DTYPES, MIN_FOOTPRINT, SHAPES, WARMUP, frames, timed_interleaved  # noqa: E402

CL = torch.channels_last


def bench_shape(name, dev, iters):
    B, n, knn, C, H, W = SHAPES[name]
    g = frames(B, n, knn)
    csr = g.csr(dev)
    Nt, E = g.num_nodes(), g.num_edges()
    lib = _lib.load_library()
    gen = torch.Generator(device=dev).manual_seed(0)
    z = torch.randn(E, C, 2, device=dev, generator=gen)  # logits, as the model hands them over
    mode = _lib.MODE_FILM_MEAN | _lib.GB_LOGITS
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = aggregate._ptr
    block_a = torch.empty(256 << 20, device=dev, dtype=torch.uint8)
    block_b = torch.empty_like(block_a)

    def blocker():  # the legs go through the Python ops: a longer queue than bench_half_io's keeps the host ahead
        for _ in range(200):
            _lib.check(lib.mrp_stream_copy(ptr(block_a), ptr(block_b), block_a.numel(), stream), "mrp_stream_copy")

    def native():
        aggregate.set_channels_last("native")

    def convert():
        aggregate.set_channels_last("convert")

    rows = {}
    for label, T in DTYPES:
        tensor_bytes = Nt * C * H * W * torch.empty((), dtype=T).element_size()
        sets = []
        for _ in range(max(2, -(-MIN_FOOTPRINT // (2 * tensor_bytes)) + 1)):
            x = torch.randn(Nt, C, H, W, device=dev, generator=gen).to(T)
            G = torch.randn(Nt, C, H, W, device=dev, generator=gen).to(T)
            sets.append(dict(x=x, G=G, xcl=x.contiguous(memory_format=CL), Gcl=G.contiguous(memory_format=CL),
                             out=torch.empty_like(x), outcl=torch.empty_like(x, memory_format=CL)))

        def copy_calls(nbytes):
            half = (nbytes // 2 + 15) // 16 * 16  # read `half`, write `half`
            bufs = [(torch.empty(half, device=dev, dtype=torch.uint8), torch.empty(half, device=dev, dtype=torch.uint8))
                    for _ in range(max(2, -(-MIN_FOOTPRINT // (2 * half)) + 1))]
            return [(lambda a=a, b=b: _lib.check(lib.mrp_stream_copy(ptr(a), ptr(b), half, stream), "mrp_stream_copy"))
                    for a, b in bufs]

        def fwd(xk, ok, back=False):
            def one(s):
                def call():
                    out = aggregate.film_mean_forward_into(s[xk], z, csr, mode, s[ok])
                    if back:
                        out.contiguous(memory_format=CL)
                return call
            return [one(s) for s in sets]

        def bwd(xk, gk, back=False):
            def one(s):
                def call():
                    dx, _ = aggregate.film_mean_backward(s[gk], s[xk], z, csr, mode, True, True)
                    if back:
                        dx.contiguous(memory_format=CL)
                return call
            return [one(s) for s in sets]

        before = dict(aggregate.PATH_COUNTS)
        try:
            with torch.no_grad():
                t_f = timed_interleaved({
                    "native": (native, fwd("xcl", "outcl")),
                    # an NCHW out selects the NCHW kernels; the channels_last x is copied first
                    "convert": (convert, fwd("xcl", "out")),
                    "convert_back": (convert, fwd("xcl", "out", back=True)),
                    "nchw": (native, fwd("x", "out")),
                    "copy": (None, copy_calls(2 * tensor_bytes)),
                }, iters, blocker)
                t_b = timed_interleaved({
                    "native": (native, bwd("xcl", "Gcl")),
                    "convert": (convert, bwd("xcl", "Gcl")),
                    "convert_back": (convert, bwd("xcl", "Gcl", back=True)),
                    "nchw": (native, bwd("x", "G")),
                    "copy": (None, copy_calls(3 * tensor_bytes)),
                }, iters, blocker)
        finally:
            aggregate.set_channels_last("native")
        key = aggregate._DTYPE_KEYS[T]
        ran = {k: aggregate.PATH_COUNTS[k] - before.get(k, 0) for k in ("fwd_cl_" + key, "bwd_cl_" + key)}
        calls = iters + WARMUP
        assert ran == {"fwd_cl_" + key: calls, "bwd_cl_" + key: calls}, ran  # only the native legs ran them
        nsets = len(sets)
        del sets
        torch.cuda.empty_cache()

        def leg(t):
            r = {k + "_us": round(v, 2) for k, v in t.items()}
            r["native_vs_convert"] = round(t["native"] / t["convert"], 3)
            r["native_vs_convert_back"] = round(t["native"] / t["convert_back"], 3)
            r["native_vs_nchw"] = round(t["native"] / t["nchw"], 3)
            r["native_vs_copy"] = round(t["native"] / t["copy"], 3)
            r["native_lt_convert"] = bool(t["native"] < t["convert"])
            return r
        rows[label] = {"fwd": leg(t_f), "bwd": leg(t_b), "fwd_bytes": 2 * tensor_bytes, "bwd_bytes": 3 * tensor_bytes,
                       "rotated_sets": nsets}
    return {"graphs": B, "nodes": n, "knn": knn, "C": C, "H": H, "W": W, "dtypes": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channels_last_bench.json"))
    a = ap.parse_args()
    if a.iters < 50:
        ap.error("--iters must be >= 50 (median of at least 50 timed calls)")
    dev = torch.device("cuda:0")
    result = {"tool": "bench_channels_last", "device": torch.cuda.get_device_name(dev), "iters": a.iters,
              "warmup": WARMUP, "abi": _lib.ABI_VERSION, "shapes": {}}
    for name in a.shapes.split(","):
        result["shapes"][name] = bench_shape(name, dev, a.iters)
    result["native_lt_convert_everywhere"] = all(
        r[d]["native_lt_convert"] for s in result["shapes"].values() for r in s["dtypes"].values() for d in ("fwd", "bwd"))
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
