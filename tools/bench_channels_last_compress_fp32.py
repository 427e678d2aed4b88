"""The pixel-major (``torch.channels_last``) fp32 split-bf16 1x1 compress (``compress_split_cl.hip``, behind
``compress.set_channels_last_compress_fp32("native")``) against the convert route it replaces (today's
default) and against the NCHW kernels, timed in one run on one GPU.

Rows: the ``cat_compress`` layer shapes of BASELINE configs[1] (Nt = 128, C = 512, 32 x 32), configs[2]
(256, 1280, 8 x 8) and configs[4] (128, 1024, 16 x 16, k-NN(4) graphs of 16), for each precision mode of
``compress.set_compress_precision`` (``highest`` / ``high`` / ``medium``): the forward, the data gradient and
the weight gradient alone, and the whole layer's training step (``GCNStack`` of one ``cat_compress`` layer,
forward + backward).  Legs:

* ``native``        channels_last operands through the pixel-major kernels (``mrp_compress_fwd_split_cl`` /
                    ``_bwd_data_split_cl`` / ``_bwd_weight_split_cl``; the step also runs the pixel-major
                    aggregation);
* ``convert``       the same operands on the default route: copies to NCHW, the NCHW split kernels, NCHW
                    results;
* ``convert_back``  convert, plus the copy of the results back to channels_last (what a channels_last
                    consumer of the convert route pays; the weight gradient's results are parameter
                    gradients, so it has no such copy and the leg equals ``convert``);
* ``nchw``          NCHW operands through the NCHW split kernels;
* ``copy``          ``mrp_stream_copy`` over the product's algorithmic bytes (three feature tensors).

Protocol (``tools/bench_channels_last_compress.py``'s): hipEvents around every call behind a few milliseconds
of queued copies, 5 warm-ups, the median of ``--iters`` (>= 50) calls, operand sets rotated over more than
512 MB, the legs of one measurement taking turns call by call in one loop.  Prints one JSON line and writes
``profiles/channels_last_compress_fp32_bench.json``.

    python tools/bench_channels_last_compress_fp32.py [--iters 50] [--shapes configs1,configs2,configs4]
                                                      [--modes highest,high,medium] [--out PATH]
"""
import argparse
import ctypes
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import mrp_gnn_amd as m  # noqa: E402
from mrp_gnn_amd import _lib, aggregate, compress  # noqa: E402
from tools.bench_half_compress import SHAPES, nsets  # noqa: E402
from tools.bench_half_io import MIN_FOOTPRINT, WARMUP, frames, timed_interleaved  # noqa: E402

CL = torch.channels_last
MODES = ("highest", "high", "medium")


def bench_shape(name, dev, iters, modes):
    B, n, knn, C, H, W = SHAPES[name]
    g = frames(B, n, knn).to(dev)
    Nt, P = g.num_nodes(), H * W
    lib = _lib.load_library()
    gen = torch.Generator(device=dev).manual_seed(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = aggregate._ptr
    block_a = torch.empty(256 << 20, device=dev, dtype=torch.uint8)
    block_b = torch.empty_like(block_a)

    def blocker():
        for _ in range(40):
            _lib.check(lib.mrp_stream_copy(ptr(block_a), ptr(block_b), block_a.numel(), stream), "mrp_stream_copy")

    torch.manual_seed(0)
    stack = m.GCNStack(types.SimpleNamespace(feature_dim=C, gcn_layers=1, gcn_combine="cat_compress")).to(dev)
    w, b = stack.conv1.weight.detach(), stack.conv1.bias.detach()
    flops = 2.0 * Nt * P * C * 2 * C
    elems = Nt * C * P

    def route(r):
        return lambda: compress.set_channels_last_compress_fp32(r)

    def back(t):
        return t.contiguous(memory_format=CL)

    def products(sets, copy_back):
        """name -> list of calls (one per operand set) through the layer-level entry points, which follow
        the operands' layout, the route and the precision mode in force."""
        def fwd(x, a):
            y = compress._fwd(w, b, x, a)
            return back(y) if copy_back else y

        def dgrad(x, gy):
            gx, ga = compress._bwd_data(w, gy, x.dtype, like=x)
            return (back(gx), back(ga)) if copy_back else (gx, ga)

        return {"fwd": [(lambda x=x, a=a: fwd(x, a)) for x, a, _ in sets],
                "dgrad": [(lambda x=x, gy=gy: dgrad(x, gy)) for x, _, gy in sets],
                "wgrad": [(lambda x=x, a=a, gy=gy: compress._bwd_weight(gy, x, a, True, None, None)) for x, a, gy in sets]}

    def step_calls(sets, copy_back):
        def one(x, G):
            def call():
                for p in stack.parameters():
                    p.grad = None
                x.grad = None
                out = stack(g, x)
                if copy_back:
                    out = back(out)
                out.backward(G)
            return call
        return [one(x.requires_grad_(True), G) for x, _, G in sets]

    k = nsets(elems * 4, 3)
    nm = [tuple(torch.randn(Nt, C, H, W, device=dev, generator=gen) for _ in range(3)) for _ in range(k)]
    cl = [tuple(t.contiguous(memory_format=CL) for t in s) for s in nm]
    half = (3 * elems * 4 // 2 + 15) // 16 * 16  # the copy reads `half` bytes and writes `half`
    bufs = [(torch.empty(half, device=dev, dtype=torch.uint8), torch.empty(half, device=dev, dtype=torch.uint8))
            for _ in range(max(2, -(-MIN_FOOTPRINT // (2 * half)) + 1))]
    copies = [(lambda s=s, d=d: _lib.check(lib.mrp_stream_copy(ptr(s), ptr(d), half, stream), "mrp_stream_copy"))
              for s, d in bufs]
    rows = {}
    for mode in modes:
        row = {"rotated_sets": k, "product_bytes": 3 * elems * 4}
        prev = compress.set_compress_precision(mode)
        try:
            with torch.no_grad():
                pcl, pback, pnm = products(cl, False), products(cl, True), products(nm, False)
                for op in ("fwd", "dgrad", "wgrad"):
                    legs = {"native": (route("native"), pcl[op]), "convert": (route("convert"), pcl[op]),
                            "convert_back": (route("convert"), pback[op]), "nchw": (route("convert"), pnm[op]),
                            "copy": (None, copies)}
                    t = timed_interleaved(legs, iters, blocker)
                    row[op] = {leg + "_us": round(v, 2) for leg, v in t.items()}
                    row[op].update(vs_convert=round(t["native"] / t["convert"], 3),
                                   vs_convert_back=round(t["native"] / t["convert_back"], 3),
                                   vs_nchw=round(t["native"] / t["nchw"], 3),
                                   native_tflops=round(flops / t["native"] * 1e-6, 1),
                                   nchw_tflops=round(flops / t["nchw"] * 1e-6, 1),
                                   ceiling_frac=round(t["copy"] / t["native"], 3))
                del pcl, pback, pnm
            t = timed_interleaved({"native": (route("native"), step_calls(cl, False)),
                                   "convert": (route("convert"), step_calls(cl, False)),
                                   "convert_back": (route("convert"), step_calls(cl, True)),
                                   "nchw": (route("convert"), step_calls(nm, False))}, iters, blocker)
        finally:
            compress.set_channels_last_compress_fp32("convert")
            compress.set_compress_precision(prev)
        row["layer_step"] = {leg + "_us": round(v, 2) for leg, v in t.items()}
        row["layer_step"].update(vs_convert=round(t["native"] / t["convert"], 3),
                                 vs_convert_back=round(t["native"] / t["convert_back"], 3),
                                 vs_nchw=round(t["native"] / t["nchw"], 3))
        rows[mode] = row
        for x, _, _ in nm + cl:
            x.requires_grad_(False)
            x.grad = None
    del nm, cl, bufs, copies
    torch.cuda.empty_cache()
    return {"graphs": B, "nodes": n, "knn": knn, "Nt": Nt, "C": C, "H": H, "W": W, "product_flops": flops,
            "modes": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channels_last_compress_fp32_bench.json"))
    a = ap.parse_args()
    if a.iters < 50:
        ap.error("--iters must be >= 50 (median of at least 50 timed calls)")
    modes = a.modes.split(",")
    for mode in modes:
        if mode not in MODES:
            ap.error(f"unknown precision mode {mode!r}")
    dev = torch.device("cuda:0")
    result = {"tool": "bench_channels_last_compress_fp32", "device": torch.cuda.get_device_name(dev), "iters": a.iters,
              "warmup": WARMUP, "abi": _lib.ABI_VERSION, "shapes": {}}
    for name in a.shapes.split(","):
        result["shapes"][name] = bench_shape(name, dev, a.iters, modes)
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
