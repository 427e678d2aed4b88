"""fp32 / bf16 / fp16 feature I/O of the FiLM-mean aggregation, timed in one run on one GPU.

For each shape and feature dtype: the aggregation forward (``mrp_film_mean_fwd_t``), the backward with
grad_x and grad_gb (``mrp_film_mean_bwd_t``), and ``mrp_stream_copy`` over the same algorithmic byte
count as the same-box ceiling (forward: x read + out written; backward: grad_out and x read + grad_x
written; gamma/beta and index traffic, a few per cent at most, is not counted).

Protocol: hipEvents around every call, the host running ahead of the device so an interval
holds device time only (a few milliseconds of copies are queued first); 5 warm-ups; the median of ``--iters`` (>= 50) timed calls; input/output sets
rotated over a total footprint above 512 MB so no call finds its operands in the 256 MB last-level cache.

``--knob NAME=V0,V1[,...]`` (e.g. ``bwd_half_mfma=0,1``) adds an A/B of the 16-bit backward on the rows
of 9..16-node graphs: one timed loop in which the knob values and the fp32 backward take turns call by call
(settings interleaved, so drift of the box hits every variant alike), the median per variant
(``bwd_ab_us``), each variant's fraction of the copy ceiling and ``t / t_fp32``.

Prints one JSON line and writes ``profiles/half_io_bench.json`` (with ``--knob``:
``profiles/half_io_bench_mfma.json``).

    python tools/bench_half_io.py [--iters 50] [--shapes headline,small_planes,knn] [--knob bwd_half_mfma=0,1]
                                  [--out PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import mrp_gnn_amd as m  # noqa: E402
from mrp_gnn_amd import _lib, aggregate  # noqa: E402

SHAPES = {
    # name: (graphs, nodes per graph, k-NN degree or None, C, H, W)
    "headline": (32, 8, None, 512, 32, 32),
    "small_planes": (32, 8, None, 1280, 8, 8),
    "knn": (8, 16, 4, 1024, 16, 16),
    "complete16": (8, 16, None, 1024, 16, 16),
    "complete12_small_planes": (32, 12, None, 1280, 8, 8),  # one 64-pixel group per plane
}
DTYPES = [("fp32", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16)]
WARMUP = 5
MIN_FOOTPRINT = 512 << 20


def frames(B, n, knn, seed=0):
    rng = np.random.RandomState(seed)
    graphs = []
    for _ in range(B):
        poses = np.concatenate([rng.uniform(-10, 10, (n, 3)), rng.standard_normal((n, 4))], 1).astype(np.float32)
        graphs.append(m.frame_graph(poses, knn=knn))
    return m.batch(graphs)


def timed(calls, iters, blocker):
    """Median device time (us) of calls[i % len(calls)](), events around each, no sync inside the loop.
    ``blocker`` enqueues a few milliseconds of other work first, so the host has every timed call queued
    before the device reaches it and no interval contains host latency."""
    for i in range(WARMUP):
        calls[i % len(calls)]()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    blocker()
    for i, (a, b) in enumerate(ev):
        a.record()
        calls[i % len(calls)]()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3


def timed_interleaved(variants, iters, blocker):
    """Medians (us) of several variants timed in one loop, taking turns call by call.  variants: name ->
    (setup or None, calls); setup() runs on the host before each of the variant's calls (a tuning knob: it
    decides the launch, so it holds for the call enqueued right after it)."""
    turn = 0  # counts every call: variants that share operand sets never follow each other on one set
    for name, (setup, calls) in variants.items():
        for i in range(WARMUP):
            if setup:
                setup()
            calls[turn % len(calls)]()
            turn += 1
    torch.cuda.synchronize()
    ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
          for name in variants}
    blocker()
    for i in range(iters):
        for name, (setup, calls) in variants.items():
            if setup:
                setup()
            a, b = ev[name][i]
            a.record()
            calls[turn % len(calls)]()
            b.record()
            turn += 1
    torch.cuda.synchronize()
    return {name: statistics.median(a.elapsed_time(b) for a, b in ev[name]) * 1e3 for name in variants}


def bench_shape(name, dev, iters, knob=None):
    B, n, knn, C, H, W = SHAPES[name]
    g = frames(B, n, knn)
    csr = g.csr(dev)
    Nt, E, P = g.num_nodes(), g.num_edges(), H * W
    lib = _lib.load_library()
    gen = torch.Generator(device=dev).manual_seed(0)
    z = torch.randn(E, C, 2, device=dev, generator=gen)  # logits, as the model hands them over
    mode = _lib.MODE_FILM_MEAN | _lib.GB_LOGITS
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = aggregate._ptr
    graph = (ptr(z), ptr(csr.indptr), ptr(csr.src), ptr(csr.eid), ptr(csr.graph_off), csr.num_graphs, csr.max_nodes,
             csr.graph_kind, csr.num_nodes, csr.num_edges, C, P, mode)
    stride = C * P
    block_a = torch.empty(256 << 20, device=dev, dtype=torch.uint8)
    block_b = torch.empty_like(block_a)

    def blocker():  # ~40 x (256 MB read + 256 MB written): a few milliseconds
        for _ in range(40):
            _lib.check(lib.mrp_stream_copy(ptr(block_a), ptr(block_b), block_a.numel(), stream), "mrp_stream_copy")

    def make_sets(T):
        """Sets of (x, out, grad_out, grad_x, grad_gb): enough of them, rotated, to exceed the footprint."""
        tensor_bytes = Nt * C * P * torch.empty((), dtype=T).element_size()
        sets = []
        for _ in range(max(2, -(-MIN_FOOTPRINT // (2 * tensor_bytes)) + 1)):
            x = torch.randn(Nt, C, H, W, device=dev, generator=gen).to(T)
            G = torch.randn(Nt, C, H, W, device=dev, generator=gen).to(T)
            sets.append((x, torch.empty_like(x), G, torch.empty_like(x),
                         torch.empty(E, C, 2, device=dev, dtype=torch.float32)))
        return sets

    def bwd_calls(T, sets):
        dt = aggregate.FEATURE_DTYPES[T]

        def bwd(s):
            x, _, G, dx, dgb = s
            args = (dt, ptr(G), stride, ptr(x), stride) + graph + (ptr(dx), stride, None, 0, ptr(dgb), None, stream)
            return lambda: _lib.check(lib.mrp_film_mean_bwd_t(*args), "mrp_film_mean_bwd_t")
        return [bwd(s) for s in sets]

    rows = {}
    for label, T in DTYPES:
        elem = torch.empty((), dtype=T).element_size()
        tensor_bytes = Nt * C * P * elem
        sets = make_sets(T)
        nsets = len(sets)

        dt = aggregate.FEATURE_DTYPES[T]  # fp32: the typed entry points forward to the fp32 implementation

        def fwd(s):
            args = (dt, ptr(s[0]), stride) + graph + (ptr(s[1]), stride, None, stream)
            return lambda: _lib.check(lib.mrp_film_mean_fwd_t(*args), "mrp_film_mean_fwd_t")

        def copy(nbytes):
            half = (nbytes // 2 + 15) // 16 * 16  # read `half`, write `half`
            bufs = [(torch.empty(half, device=dev, dtype=torch.uint8), torch.empty(half, device=dev, dtype=torch.uint8))
                    for _ in range(max(2, -(-MIN_FOOTPRINT // (2 * half)) + 1))]

            def one(src, dst):
                return lambda: _lib.check(lib.mrp_stream_copy(ptr(src), ptr(dst), half, stream), "mrp_stream_copy")
            return [one(a, b) for a, b in bufs]

        fwd_bytes, bwd_bytes = 2 * tensor_bytes, 3 * tensor_bytes
        t_fwd = timed([fwd(s) for s in sets], iters, blocker)
        t_bwd = timed(bwd_calls(T, sets), iters, blocker)
        t_cf = timed(copy(fwd_bytes), iters, blocker)
        t_cb = timed(copy(bwd_bytes), iters, blocker)
        ab = None
        if knob is not None and T != torch.float32 and n > 8:
            kname, values = knob

            def setter(v):
                return lambda: _lib.check(lib.mrp_tuning_set(kname.encode(), v), "mrp_tuning_set")
            sets32 = make_sets(torch.float32)
            variants = {f"{kname}={v}": (setter(v), bwd_calls(T, sets)) for v in values}
            variants["fp32"] = (None, bwd_calls(torch.float32, sets32))
            try:
                ab = timed_interleaved(variants, iters, blocker)
            finally:
                _lib.check(lib.mrp_tuning_set(b"reset", 0), "mrp_tuning_set")
            del sets32
        del sets
        torch.cuda.empty_cache()
        rows[label] = {
            "fwd_us": round(t_fwd, 2), "bwd_us": round(t_bwd, 2),
            "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes,
            "copy_fwd_us": round(t_cf, 2), "copy_bwd_us": round(t_cb, 2),
            "fwd_tbps": round(fwd_bytes / t_fwd * 1e-6, 3), "bwd_tbps": round(bwd_bytes / t_bwd * 1e-6, 3),
            "fwd_ceiling_frac": round(t_cf / t_fwd, 3), "bwd_ceiling_frac": round(t_cb / t_bwd, 3),
            "rotated_sets": nsets,
        }
        if ab is not None:
            rows[label]["bwd_ab_us"] = {k: round(v, 2) for k, v in ab.items()}
            rows[label]["bwd_ab_vs_fp32"] = {k: round(v / ab["fp32"], 3) for k, v in ab.items() if k != "fp32"}
            rows[label]["bwd_ab_ceiling_frac"] = {k: round(t_cb / v, 3) for k, v in ab.items() if k != "fp32"}
    for label in ("bf16", "fp16"):
        rows[label]["fwd_vs_fp32"] = round(rows[label]["fwd_us"] / rows["fp32"]["fwd_us"], 3)
        rows[label]["bwd_vs_fp32"] = round(rows[label]["bwd_us"] / rows["fp32"]["bwd_us"], 3)
    return {"graphs": B, "nodes": n, "knn": knn, "C": C, "H": H, "W": W, "dtypes": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--knob", default=None, help="NAME=V0,V1[,...]: A/B of the 16-bit backward over a tuning knob")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.iters < 50:
        ap.error("--iters must be >= 50 (median of at least 50 timed calls)")
    knob = None
    if a.knob is not None:
        kname, _, vals = a.knob.partition("=")
        if not kname or not vals:
            ap.error("--knob takes NAME=V0,V1[,...]")
        knob = (kname, [int(v) for v in vals.split(",")])
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "half_io_bench_mfma.json" if knob else "half_io_bench.json")
    dev = torch.device("cuda:0")
    result = {"tool": "bench_half_io", "device": torch.cuda.get_device_name(dev), "iters": a.iters,
              "warmup": WARMUP, "abi": _lib.ABI_VERSION, "knob": a.knob, "shapes": {}}
    for name in a.shapes.split(","):
        result["shapes"][name] = bench_shape(name, dev, a.iters, knob)
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
