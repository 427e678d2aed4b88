"""The native bf16 / fp16 1x1 compress (``compress_half.hip``) against the route it replaces and against
the fp32 split kernels, timed in one run on one GPU.

Rows: the ``cat_compress`` layer shapes of BASELINE configs[1] (Nt = 128, C = 512, 32 x 32), configs[2]
(256, 1280, 8 x 8) and configs[4] (128, 1024, 16 x 16, k-NN(4) graphs of 16).  For each of bf16 and
fp16:

* the forward, the data gradient and the weight gradient alone — ``native`` (``mrp_compress_fwd_t`` /
  ``_bwd_data_t`` / ``_bwd_weight_t`` through ``compress.py``), ``torch`` (the earlier route's products:
  torch's convolution and its two gradients over the (Nt, 2C, H, W) concatenation in T, the weight cast
  to T as autocast does; the cast and the concatenation are not in the interval) and ``fp32`` (the
  split-bf16 kernels on fp32 operands), plus ``mrp_stream_copy`` over the 16-bit product's algorithmic
  bytes (three feature tensors: forward x and a read, y written; data gradient gy read, gx and ga
  written; weight gradient gy, x and a read) as the same-box ceiling;
* the whole layer's training step (``GCNStack`` of one ``cat_compress`` layer, forward + backward, under
  ``torch.autocast``): ``native``, ``torch`` (``compress.set_half_compress("torch")``, the parent's
  behaviour) and ``fp32`` (fp32 features, no autocast).

Protocol (``tools/bench_half_io.py``'s): hipEvents around every call behind a few milliseconds of queued
copies, 5 warm-ups, the median of ``--iters`` (>= 50) calls, operand sets rotated over more than 512 MB,
the variants of one measurement taking turns call by call in one loop.  Reports us, t / t_fp32,
t / t_torch-route, TF/s and the copy ceiling's fraction.  Prints one JSON line and writes
``profiles/half_compress_bench.json``.

    python tools/bench_half_compress.py [--iters 50] [--shapes configs1,configs2,configs4] [--out PATH]
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
from tools.bench_half_io import MIN_FOOTPRINT, WARMUP, frames, timed_interleaved  # noqa: E402

SHAPES = {
    # name: (graphs, nodes per graph, k-NN degree or None, C, H, W)
    "configs1": (16, 8, None, 512, 32, 32),
    "configs2": (32, 8, None, 1280, 8, 8),
    "configs4": (8, 16, 4, 1024, 16, 16),
}
HALF = [("bf16", torch.bfloat16), ("fp16", torch.float16)]


def nsets(tensor_bytes, tensors):
    return max(2, -(-MIN_FOOTPRINT // (tensors * tensor_bytes)) + 1)


def bench_shape(name, dev, iters):
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

    def rand(T):
        return torch.randn(Nt, C, H, W, device=dev, generator=gen).to(T)

    torch.manual_seed(0)
    stack = m.GCNStack(types.SimpleNamespace(feature_dim=C, gcn_layers=1, gcn_combine="cat_compress")).to(dev)
    w, b = stack.conv1.weight.detach(), stack.conv1.bias.detach()
    flops = 2.0 * Nt * P * C * 2 * C
    elems = Nt * C * P

    # fp32 operand sets, shared by every fp32 variant: (x, a, gy) and the step's (x, G)
    k32 = nsets(elems * 4, 3)
    sets32 = [(rand(torch.float32), rand(torch.float32), rand(torch.float32)) for _ in range(k32)]

    def products(T, sets, route):
        """name -> list of calls (one per operand set) of the three products on one route."""
        if route == "torch":
            wT, bT = w.to(T), b.to(T)
            cats = [torch.cat((x, a), 1) for x, a, _ in sets]
            conv_bwd = torch.ops.aten.convolution_backward

            def bwd(gy, h, mask):
                return lambda: conv_bwd(gy, h, wT, [C], [1, 1], [0, 0], [1, 1], False, [0, 0], 1, mask)
            return {"fwd": [(lambda h=h: torch.nn.functional.conv2d(h, wT, bT)) for h in cats],
                    "dgrad": [bwd(s[2], h, [True, False, False]) for s, h in zip(sets, cats)],
                    "wgrad": [bwd(s[2], h, [False, True, True]) for s, h in zip(sets, cats)]}
        return {"fwd": [(lambda x=x, a=a: compress.compress_forward(w, b, x, a)) for x, a, _ in sets],
                "dgrad": [(lambda gy=gy: compress.compress_backward_data(w, gy)) for _, _, gy in sets],
                "wgrad": [(lambda x=x, a=a, gy=gy: compress.compress_backward_weight(gy, x, a)) for x, a, gy in sets]}

    def step_calls(T, sets, autocast):
        def one(x, G):
            def call():
                for p in stack.parameters():
                    p.grad = None
                x.grad = None
                if autocast:
                    with torch.autocast("cuda", dtype=T):
                        out = stack(g, x)
                else:
                    out = stack(g, x)
                out.backward(G)
            return call
        return [one(x.requires_grad_(True), G) for x, _, G in sets]

    def route(r):
        return lambda: compress.set_half_compress(r)

    rows = {}
    with torch.no_grad():
        p32 = products(torch.float32, sets32, "native")
    for label, T in HALF:
        k = nsets(elems * 2, 3)
        sets = [(rand(T), rand(T), rand(T)) for _ in range(k)]
        half = (3 * elems * 2 // 2 + 15) // 16 * 16  # the copy reads `half` bytes and writes `half`
        bufs = [(torch.empty(half, device=dev, dtype=torch.uint8), torch.empty(half, device=dev, dtype=torch.uint8))
                for _ in range(max(2, -(-MIN_FOOTPRINT // (2 * half)) + 1))]
        copies = [(lambda s=s, d=d: _lib.check(lib.mrp_stream_copy(ptr(s), ptr(d), half, stream), "mrp_stream_copy"))
                  for s, d in bufs]
        row = {"rotated_sets": k, "product_bytes": 3 * elems * 2}
        with torch.no_grad():
            pn, pt = products(T, sets, "native"), products(T, sets, "torch")
            for op in ("fwd", "dgrad", "wgrad"):
                t = timed_interleaved({"native": (None, pn[op]), "torch": (None, pt[op]), "fp32": (None, p32[op]),
                                       "copy": (None, copies)}, iters, blocker)
                row[op] = {"native_us": round(t["native"], 2), "torch_us": round(t["torch"], 2),
                           "fp32_us": round(t["fp32"], 2), "copy_us": round(t["copy"], 2),
                           "vs_fp32": round(t["native"] / t["fp32"], 3), "vs_torch": round(t["native"] / t["torch"], 3),
                           "native_tflops": round(flops / t["native"] * 1e-6, 1),
                           "torch_tflops": round(flops / t["torch"] * 1e-6, 1),
                           "fp32_tflops": round(flops / t["fp32"] * 1e-6, 1),
                           "ceiling_frac": round(t["copy"] / t["native"], 3)}
            del pt, pn
        try:
            t = timed_interleaved({"native": (route("native"), step_calls(T, sets, True)),
                                   "torch": (route("torch"), step_calls(T, sets, True)),
                                   "fp32": (route("native"), step_calls(torch.float32, sets32, False))}, iters, blocker)
        finally:
            compress.set_half_compress("native")
        row["layer_step"] = {"native_us": round(t["native"], 2), "torch_us": round(t["torch"], 2),
                             "fp32_us": round(t["fp32"], 2), "vs_fp32": round(t["native"] / t["fp32"], 3),
                             "vs_torch": round(t["native"] / t["torch"], 3)}
        rows[label] = row
        for x, _, _ in sets + sets32:
            x.requires_grad_(False)
            x.grad = None
        del sets, bufs, copies
        torch.cuda.empty_cache()
    return {"graphs": B, "nodes": n, "knn": knn, "Nt": Nt, "C": C, "H": H, "W": W, "product_flops": flops,
            "dtypes": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_compress_bench.json"))
    a = ap.parse_args()
    if a.iters < 50:
        ap.error("--iters must be >= 50 (median of at least 50 timed calls)")
    dev = torch.device("cuda:0")
    result = {"tool": "bench_half_compress", "device": torch.cuda.get_device_name(dev), "iters": a.iters,
              "warmup": WARMUP, "abi": _lib.ABI_VERSION, "shapes": {}}
    for name in a.shapes.split(","):
        result["shapes"][name] = bench_shape(name, dev, a.iters)
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
