"""The confidence-weighted FiLM aggregation against the mean on identical tensors, timed in one run on one GPU.

Legs: forward and backward (with grad_w: grad_x, grad_gb and grad_w; without: grad_x and grad_gb), fp32 and
bf16, at
  * the headline shape: B = 32 complete 8-node graphs, C = 512, 32x32;
  * BASELINE configs[2]: B = 32 complete 8-node graphs, C = 1280, 8x8;
  * BASELINE configs[4]: B = 8 k-NN(4) 16-node graphs, C = 1024, 16x16.

The mean kernels are code the weighted operator does not touch, so they are the yardstick: ``film_wmean``,
``film_mean`` (mode film_mean, plain gamma/beta) and a plain copy of the mean's byte count (the same-box
ceiling) take turns call by call in one process, for ``--rounds`` (>= 5) rounds of ``--iters`` calls each; per
round the median per operator, over the rounds the median ratio wmean / mean and the spread ((max - min) /
median of an operator's round medians, the larger of the two).  Achieved bytes/s are over each operator's own
algorithmic bytes: forward x read and out written (Nt C P elements each); backward grad_out and x read, grad_x
written; gamma/beta (and their gradient) 2 C fp32 per edge; the weighted operator adds the maps (Nt P fp32,
and as many again for grad_w).  ``byte_ratio`` is the ratio the bytes alone would give.

Protocol as tools/bench_range_graphs.py: events around every call with the host running ahead of the
device, 5 warm-ups, operand sets rotated over more than 512 MB (larger than the Infinity Cache).  Prints one
JSON line and writes ``profiles/film_wmean_bench.json``.

    python tools/bench_film_wmean.py [--rounds 5] [--iters 20] [--out PATH]
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

DTYPES = [("fp32", torch.float32), ("bf16", torch.bfloat16)]
WARMUP = 5
MIN_FOOTPRINT = 512 << 20
SHAPES = [("headline", 32, 8, None, 512, 32, 32), ("configs2", 32, 8, None, 1280, 8, 8),
          ("configs4", 8, 16, 4, 1024, 16, 16)]


def interleaved(variants, iters, blocker, turn0=0):
    """Per-variant median (us) of ``iters`` calls, the variants taking turns call by call."""
    turn = turn0
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
          for k in variants}
    blocker()
    for i in range(iters):
        for k, calls in variants.items():
            a, b = ev[k][i]
            a.record()
            calls[turn % len(calls)]()
            b.record()
            turn += 1
    torch.cuda.synchronize()
    return {k: statistics.median(a.elapsed_time(b) for a, b in ev[k]) * 1e3 for k in variants}, turn


def rounds_of(variants, rounds, iters, blocker):
    turn = 0
    for calls in variants.values():
        for i in range(WARMUP):
            calls[i % len(calls)]()
    torch.cuda.synchronize()
    per_round = []
    for _ in range(rounds):
        med, turn = interleaved(variants, iters, blocker, turn)
        per_round.append(med)
    return per_round


def summarise(per_round, a, b, bytes_a, bytes_b):
    ratios = [r[a] / r[b] for r in per_round]
    spread = max((max(r[k] for r in per_round) - min(r[k] for r in per_round)) / statistics.median(r[k] for r in per_round)
                 for k in (a, b))
    out = {a + "_us": [round(r[a], 2) for r in per_round], b + "_us": [round(r[b], 2) for r in per_round],
           "copy_us": [round(r["copy"], 2) for r in per_round],
           "ratio_per_round": [round(x, 4) for x in ratios], "ratio": round(statistics.median(ratios), 4),
           "byte_ratio": round(bytes_a / bytes_b, 4), "spread": round(spread, 4),
           a + "_bytes": bytes_a, b + "_bytes": bytes_b}
    for k, nb in ((a, bytes_a), (b, bytes_b), ("copy", bytes_b)):
        out[k + "_TBps"] = round(nb / (statistics.median(r[k] for r in per_round) * 1e-6) / 1e12, 3)
    out[b + "_ceiling_frac"] = round(statistics.median(r["copy"] / r[b] for r in per_round), 3)
    return out


def bench_shape(dev, name, B, n, knn, C, H, W, label, T, rounds, iters, blocker, copy):
    rng = np.random.RandomState(7)
    if knn is None:
        g = m.batch([m.complete_graph(n) for _ in range(B)])
    else:
        g = m.batch([m.RobotGraph(*m.knn_edges(rng.standard_normal((n, 3)), knn), num_nodes=n) for _ in range(B)])
    csr = g.csr(dev)
    Nt, E, P = g.num_nodes(), g.num_edges(), H * W
    elem = torch.empty(0, dtype=T).element_size()
    per_set = 4 * Nt * C * P * elem
    nsets = max(2, -(-MIN_FOOTPRINT // per_set))
    gen = torch.Generator(device=dev).manual_seed(11)
    sets = []
    for _ in range(nsets):
        w = 1.0 / 16 + (15.0 / 16) * torch.rand(Nt, H, W, device=dev, generator=gen)
        w[torch.rand(Nt, H, W, device=dev, generator=gen) < 0.25] = 0.0  # a quarter of the map is not transmitted
        sets.append(dict(x=torch.randn(Nt, C, H, W, device=dev, generator=gen).to(T),
                         G=torch.randn(Nt, C, H, W, device=dev, generator=gen).to(T),
                         gb=torch.rand(E, C, 2, device=dev, generator=gen), w=w,
                         out=torch.empty(Nt, C, H, W, device=dev, dtype=T)))
    fbytes = 2 * Nt * C * P * elem + E * C * 8
    bbytes = 3 * Nt * C * P * elem + 2 * E * C * 8
    wbytes = Nt * P * 4

    def copies(nbytes):  # read half, write half: the same-box ceiling at the mean's byte count
        half = (nbytes // 2 + 15) // 16 * 16
        bufs = [(torch.empty(half, device=dev, dtype=torch.uint8), torch.empty(half, device=dev, dtype=torch.uint8))
                for _ in range(max(2, -(-MIN_FOOTPRINT // (2 * half))))]
        return [lambda a=a, b=b: copy(a, b, half) for a, b in bufs]

    fwd = {"wmean": [lambda s=s: m.film_wmean_forward_into(s["x"], s["gb"], s["w"], csr, 0, s["out"]) for s in sets],
           "mean": [lambda s=s: aggregate.film_mean_forward_into(s["x"], s["gb"], csr, _lib.MODE_FILM_MEAN, s["out"])
                    for s in sets],
           "copy": copies(fbytes)}
    mean_bwd = [lambda s=s: aggregate.film_mean_backward(s["G"], s["x"], s["gb"], csr, _lib.MODE_FILM_MEAN, True, True)
                for s in sets]
    bwd = {"wmean": [lambda s=s: m.film_wmean_backward(s["G"], s["x"], s["gb"], s["w"], csr, 0, True, True, True)
                     for s in sets],
           "mean": mean_bwd, "copy": copies(bbytes)}
    bwd_nodw = {"wmean": [lambda s=s: m.film_wmean_backward(s["G"], s["x"], s["gb"], s["w"], csr, 0, True, True, False)
                          for s in sets],
                "mean": mean_bwd, "copy": bwd["copy"]}
    return {"shape": name, "B": B, "n": n, "knn": knn, "C": C, "H": H, "W": W, "dtype": label, "sets": nsets,
            "graph_kind": csr.graph_kind,
            "forward": summarise(rounds_of(fwd, rounds, iters, blocker), "wmean", "mean", fbytes + wbytes, fbytes),
            "backward": summarise(rounds_of(bwd, rounds, iters, blocker), "wmean", "mean", bbytes + 2 * wbytes, bbytes),
            "backward_no_grad_w": summarise(rounds_of(bwd_nodw, rounds, iters, blocker), "wmean", "mean",
                                            bbytes + wbytes, bbytes)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "film_wmean_bench.json"))
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be >= 5")
    dev = torch.device("cuda:0")
    lib = _lib.load_library()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    block_a = torch.empty(256 << 20, device=dev, dtype=torch.uint8)
    block_b = torch.empty_like(block_a)

    def copy(a, b, nbytes):
        _lib.check(lib.mrp_stream_copy(aggregate._ptr(a), aggregate._ptr(b), nbytes, stream), "mrp_stream_copy")

    def blocker():  # a few milliseconds of copies: the host queues every timed call before the device gets there
        for _ in range(40):
            _lib.check(lib.mrp_stream_copy(aggregate._ptr(block_a), aggregate._ptr(block_b), block_a.numel(), stream),
                       "mrp_stream_copy")

    result = {"tool": "bench_film_wmean", "device": torch.cuda.get_device_name(dev), "rounds": a.rounds,
              "iters": a.iters, "warmup": WARMUP, "abi": _lib.ABI_VERSION, "legs": []}
    for shape in [s for s in SHAPES if s[0] in a.shapes.split(",")]:
        for label, T in DTYPES:
            torch.cuda.empty_cache()
            result["legs"].append(bench_shape(dev, *shape, label, T, a.rounds, a.iters, blocker, copy))
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
