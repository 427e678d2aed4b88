"""FP8 messages against bf16 feature maps in the FiLM-mean aggregation forward, timed in one run on one GPU.

For each shape: ``mrp_film_mean_fwd_q`` (e4m3 -> bf16 and e5m2 -> bf16, per-channel scales), the bf16
``mrp_film_mean_fwd_t`` forward on the same values, ``mrp_stream_copy`` over each variant's own algorithmic
bytes (FP8: 1 byte read + 2 written per element; bf16: 2 + 2; scales, gamma/beta and index traffic, a few per
cent at most, are not counted) and, as a separate figure, the time of ``quantize_features`` (torch ops: what a
single-GPU simulation pays to make the codes, and a receiver of FP8 buffers does not).

Protocol: that of ``tools/bench_half_io.py`` (its helpers are imported): hipEvents around every call with the
host running ahead of the device, 5 warm-ups, the median of ``--iters`` (>= 50) timed calls, operand sets
rotated over more than 512 MB.  The five kernel variants take turns call by call within one timed loop, so
drift of the box hits them alike.  No target is fixed: ``t_q / t_bf16`` and each variant's fraction of its copy
ceiling are recorded as measured.

Prints one JSON line and writes ``profiles/fp8_messages_bench.json``.

    python tools/bench_fp8_messages.py [--iters 50] [--shapes headline,small_planes,knn,complete16] [--out PATH]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

TOOLS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TOOLS)
for p in (ROOT, TOOLS):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench_half_io as hio  # noqa: E402  (frames, timed, timed_interleaved, SHAPES: the shared protocol)
import mrp_gnn_amd as m  # noqa: E402
from mrp_gnn_amd import _lib, aggregate  # noqa: E402

SHAPES = ("headline", "small_planes", "knn", "complete16")
FORMATS = (("e4m3", _lib.QDTYPE_E4M3), ("e5m2", _lib.QDTYPE_E5M2))


def bench_shape(name, dev, iters):
    B, n, knn, C, H, W = hio.SHAPES[name]
    g = hio.frames(B, n, knn)
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
    elems = Nt * C * P
    block_a = torch.empty(256 << 20, device=dev, dtype=torch.uint8)
    block_b = torch.empty_like(block_a)

    def blocker():  # ~40 x (256 MB read + 256 MB written): a few milliseconds
        for _ in range(40):
            _lib.check(lib.mrp_stream_copy(ptr(block_a), ptr(block_b), block_a.numel(), stream), "mrp_stream_copy")

    def coprime(k):  # five variants take turns: a set count that shares no factor with 5 visits every set
        return k + 1 if k % 5 == 0 else k

    nsets = coprime(max(2, -(-hio.MIN_FOOTPRINT // (3 * elems)) + 1))  # sized by the smallest set (1 + 2 bytes / element)
    sets = []  # (x fp32 for the quantiser's own timing is drawn once, below)
    for _ in range(nsets):
        x = torch.randn(Nt, C, H, W, device=dev, generator=gen)
        q = {fmt: m.quantize_features(x, fmt) for fmt, _ in FORMATS}
        xb = m.dequantize_features(*q["e4m3"]).to(torch.bfloat16)  # the same values, as bf16 features
        sets.append((q, xb, torch.empty(Nt, C, H, W, device=dev, dtype=torch.bfloat16)))
        del x

    def fwd_q(fmt, code, s):
        xq, sc = s[0][fmt]
        args = (code, ptr(xq), stride, ptr(sc), _lib.DTYPE_BF16) + graph + (ptr(s[2]), stride, None, stream)
        return lambda: _lib.check(lib.mrp_film_mean_fwd_q(*args), "mrp_film_mean_fwd_q")

    def fwd_bf16(s):
        args = (_lib.DTYPE_BF16, ptr(s[1]), stride) + graph + (ptr(s[2]), stride, None, stream)
        return lambda: _lib.check(lib.mrp_film_mean_fwd_t(*args), "mrp_film_mean_fwd_t")

    def copy(nbytes):
        half = (nbytes // 2 + 15) // 16 * 16  # read `half`, write `half`
        bufs = [(torch.empty(half, device=dev, dtype=torch.uint8), torch.empty(half, device=dev, dtype=torch.uint8))
                for _ in range(coprime(max(2, -(-hio.MIN_FOOTPRINT // (2 * half)) + 1)))]

        def one(src, dst):
            return lambda: _lib.check(lib.mrp_stream_copy(ptr(src), ptr(dst), half, stream), "mrp_stream_copy")
        return [one(a, b) for a, b in bufs]

    q_bytes, bf16_bytes = 3 * elems, 4 * elems
    variants = {f"q_{fmt}": (None, [fwd_q(fmt, code, s) for s in sets]) for fmt, code in FORMATS}
    variants["bf16"] = (None, [fwd_bf16(s) for s in sets])
    variants["copy_q"] = (None, copy(q_bytes))
    variants["copy_bf16"] = (None, copy(bf16_bytes))
    t = hio.timed_interleaved(variants, iters, blocker)
    del variants

    xs = [torch.randn(Nt, C, H, W, device=dev, generator=gen).to(torch.bfloat16) for _ in range(2)]
    t_quant = {fmt: hio.timed([(lambda x=x, fmt=fmt: m.quantize_features(x, fmt)) for x in xs], iters, blocker)
               for fmt, _ in FORMATS}
    del sets, xs
    torch.cuda.empty_cache()

    plan = _lib.AggPlan()
    p16 = ctypes.c_void_p(1 << 20)
    _lib.check(lib.mrp_film_mean_fwd_q_plan(_lib.QDTYPE_E4M3, p16, stride, p16, _lib.DTYPE_BF16, *graph, p16, stride,
                                            None, ctypes.byref(plan)), "mrp_film_mean_fwd_q_plan")
    row = {"graphs": B, "nodes": n, "knn": knn, "C": C, "H": H, "W": W, "rotated_sets": nsets,
           "plan_q": {"kernel": plan.kernel_name, "vec": plan.vec, "lpc": plan.lpc, "cpb": plan.cpb,
                      "psplit": plan.psplit},
           "q_bytes": q_bytes, "bf16_bytes": bf16_bytes, "bytes_ratio": 0.75,
           "us": {k: round(v, 2) for k, v in t.items()},
           "quantize_features_us": {k: round(v, 2) for k, v in t_quant.items()}}
    for fmt, _ in FORMATS:
        row[f"t_q_{fmt}_over_t_bf16"] = round(t[f"q_{fmt}"] / t["bf16"], 3)
        row[f"q_{fmt}_ceiling_frac"] = round(t["copy_q"] / t[f"q_{fmt}"], 3)
        row[f"q_{fmt}_tbps"] = round(q_bytes / t[f"q_{fmt}"] * 1e-6, 3)
    row["bf16_ceiling_frac"] = round(t["copy_bf16"] / t["bf16"], 3)
    row["bf16_tbps"] = round(bf16_bytes / t["bf16"] * 1e-6, 3)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_messages_bench.json"))
    a = ap.parse_args()
    if a.iters < 50:
        ap.error("--iters must be >= 50 (median of at least 50 timed calls)")
    dev = torch.device("cuda:0")
    result = {"tool": "bench_fp8_messages", "device": torch.cuda.get_device_name(dev), "iters": a.iters,
              "warmup": hio.WARMUP, "abi": _lib.ABI_VERSION, "shapes": {}}
    for name in a.shapes.split(","):
        result["shapes"][name] = bench_shape(name, dev, a.iters)
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
