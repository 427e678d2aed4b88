"""The confidence-gated attention fusion against film_attn on identical tensors, timed in one run on one GPU.

Legs: forward (inference: no rate; training: rate written) and backward (grad_x and grad_gb, with and without
grad_w), fp32 and bf16, at tools/bench_film_attn.py's shapes (headline, 8x8 planes, k-NN(4) N = 16), each with
two sender maps:
  * ``ones``: w == 1, the case in which the operator is film_attn bit for bit;
  * ``half``: about half of the (node, pixel) entries silent, the rest uniform in [0.25, 1].

``film_wattn`` and ``film_attn`` take turns call by call in one process on the same x, gb and grad_out, with
that tool's protocol (its ``interleaved`` / ``rounds_of``: events around every call with the host running ahead
of the device, 5 warm-ups, operand sets rotated over more than 512 MB); per round the median per variant, over
the rounds the median ratio to film_attn and the spread ((max - min) / median of a variant's round medians, the
largest over the variants).  Algorithmic bytes on top of film_attn's: the forward reads w (Nt P fp32) and, for
training, writes rate (E P fp32); the backward reads w and, with grad_w, reads rate and writes grad_w (Nt P).
Prints one JSON line and writes ``profiles/film_wattn_bench.json``.

    python tools/bench_film_wattn.py [--rounds 5] [--iters 20] [--out PATH]
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
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mrp_gnn_amd as m  # noqa: E402
from mrp_gnn_amd import _lib, aggregate  # noqa: E402
from bench_film_attn import DTYPES, MIN_FOOTPRINT, SHAPES, WARMUP, rounds_of  # noqa: E402

MAPS = ("ones", "half")


def summarise(per_round, base, nbytes):
    """Every variant against ``base``; ``nbytes``: {variant: its algorithmic bytes}."""
    med = {k: statistics.median(r[k] for r in per_round) for k in per_round[0]}
    out = {"us": {k: [round(r[k], 2) for r in per_round] for k in med},
           "spread": round(max((max(r[k] for r in per_round) - min(r[k] for r in per_round)) / med[k] for k in med), 4),
           "bytes": nbytes, "TBps": {k: round(nbytes[k] / (med[k] * 1e-6) / 1e12, 3) for k in med}, "ratio": {}}
    for k in med:
        if k != base:
            out["ratio"][k] = round(statistics.median(r[k] / r[base] for r in per_round), 4)
    return out


def bench_shape(dev, name, B, n, knn, C, H, W, label, T, wmap, rounds, iters, blocker):
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
    gen = torch.Generator(device="cpu").manual_seed(11)
    sets = []
    for _ in range(nsets):
        s = dict(x=torch.randn(Nt, C, H, W, generator=gen).to(dev).to(T),
                 G=torch.randn(Nt, C, H, W, generator=gen).to(dev).to(T),
                 gb=torch.rand(E, C, 2, generator=gen).to(dev),
                 out=torch.empty(Nt, C, H, W, device=dev, dtype=T))
        if wmap == "ones":
            s["w"] = torch.ones(Nt, H, W, device=dev)
        else:
            w = 0.25 + 0.75 * torch.rand(Nt, H, W, generator=gen)
            w[torch.rand(Nt, H, W, generator=gen) < 0.5] = 0.0
            s["w"] = w.to(dev)
        for k in ("attn", "wattn", "rate"):
            s[k] = torch.empty(E, P, device=dev, dtype=torch.float32)
        sets.append(s)
    for s in sets:  # each backward reads the weights of its own set and operator
        m.film_attn_forward_into(s["x"], s["gb"], csr, 0, s["out"], attn=s["attn"])
        m.film_wattn_forward_into(s["x"], s["gb"], s["w"], csr, 0, s["out"], attn=s["wattn"], rate=s["rate"])
    silent = float(sum(float((s["w"] == 0).float().mean()) for s in sets) / nsets)
    fwd = {"attn": [lambda s=s: m.film_attn_forward_into(s["x"], s["gb"], csr, 0, s["out"], attn=s["attn"])
                    for s in sets],
           "wattn": [lambda s=s: m.film_wattn_forward_into(s["x"], s["gb"], s["w"], csr, 0, s["out"], attn=s["wattn"])
                     for s in sets],
           "wattn_rate": [lambda s=s: m.film_wattn_forward_into(s["x"], s["gb"], s["w"], csr, 0, s["out"],
                                                                attn=s["wattn"], rate=s["rate"]) for s in sets]}
    bwd = {"attn": [lambda s=s: m.film_attn_backward(s["G"], s["x"], s["gb"], s["attn"], csr, 0, True, True)
                    for s in sets],
           "wattn": [lambda s=s: m.film_wattn_backward(s["G"], s["x"], s["gb"], s["w"], s["wattn"], None, csr, 0,
                                                       True, True, False) for s in sets],
           "wattn_dw": [lambda s=s: m.film_wattn_backward(s["G"], s["x"], s["gb"], s["w"], s["wattn"], s["rate"], csr,
                                                          0, True, True, True) for s in sets]}
    fa = 3 * Nt * C * P * elem + 2 * E * C * 8 + E * P * 4
    ba = 5 * Nt * C * P * elem + 3 * E * C * 8 + E * P * 4
    fbytes = {"attn": fa, "wattn": fa + Nt * P * 4, "wattn_rate": fa + Nt * P * 4 + E * P * 4}
    bbytes = {"attn": ba, "wattn": ba + Nt * P * 4, "wattn_dw": ba + 2 * Nt * P * 4 + E * P * 4}
    return {"shape": name, "B": B, "n": n, "knn": knn, "C": C, "H": H, "W": W, "dtype": label, "map": wmap,
            "silent_fraction": round(silent, 4), "sets": nsets, "graph_kind": csr.graph_kind,
            "forward": summarise(rounds_of(fwd, rounds, iters, blocker), "attn", fbytes),
            "backward": summarise(rounds_of(bwd, rounds, iters, blocker), "attn", bbytes)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "film_wattn_bench.json"))
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be >= 5")
    dev = torch.device("cuda:0")
    lib = _lib.load_library()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    block_a = torch.empty(256 << 20, device=dev, dtype=torch.uint8)
    block_b = torch.empty_like(block_a)

    def blocker():  # a few milliseconds of copies: the host queues every timed call before the device gets there
        for _ in range(40):
            _lib.check(lib.mrp_stream_copy(aggregate._ptr(block_a), aggregate._ptr(block_b), block_a.numel(), stream),
                       "mrp_stream_copy")

    result = {"tool": "bench_film_wattn", "device": torch.cuda.get_device_name(dev), "rounds": a.rounds,
              "iters": a.iters, "warmup": WARMUP, "abi": _lib.ABI_VERSION, "legs": []}
    for shape in SHAPES:
        for label, T in DTYPES:
            for wmap in MAPS:
                result["legs"].append(bench_shape(dev, *shape, label, T, wmap, a.rounds, a.iters, blocker))
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
