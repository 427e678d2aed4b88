"""FP8 messages for the max and attention reducers, receiver side, against the operators they stand beside, timed
in one run on one GPU on the same values.

Shapes (tools/bench_film_attn.py's): the headline (B = 32 complete 8-node graphs, C = 512, 32x32), 8x8 planes
(BASELINE configs[2]: B = 32 complete 8-node graphs, C = 1280) and k-NN(4) N = 16 (configs[4]: B = 8, C = 1024,
16x16).  Per shape, for e4m3 and e5m2:

  * ``film_attn_q`` and ``film_wattn_q`` (bf16 query and output) at ``heads`` 1 and 4, call by call in turn with
      - ``film_attn`` / ``film_wattn`` on bf16 features (the unquantised operator), and
      - the route they replace: ``dequantize_features`` (a pass that writes fp32) followed by the fp32 operator;
  * ``film_max_q`` (bf16 output) in turn with ``film_max`` on bf16 features and with dequantise-then-``film_max``.

The messages of every leg are one draw: the bf16 operator reads x, the FP8 ones read quantize_features(x) and the
query x.  Each operator's own algorithmic bytes are printed, so the ratio the bytes alone would give stands beside
the measured one: features and codes per element read or written (the attention forwards read their messages
twice), the weights (heads E P fp32) written, gamma/beta (E C 2 fp32, twice in the attention), the scales; the
dequantise route adds its pass (codes read, fp32 written) and reads fp32.  No ratio is fixed in advance.

Protocol as tools/bench_film_attn.py: events around every call with the host running ahead of the device, 5
warm-ups, operand sets rotated over more than 512 MB, ``--rounds`` (>= 5) rounds of ``--iters`` calls, per round
the median per operator, over the rounds the median ratio.  Prints one JSON line and writes
``profiles/fp8_attn_bench.json``.

    python tools/bench_fp8_attn.py [--rounds 5] [--iters 20] [--out PATH]
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

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_film_attn import MIN_FOOTPRINT, SHAPES, WARMUP, rounds_of  # noqa: E402

FORMATS = ("e4m3", "e5m2")
HEADS = (1, 4)
T = torch.bfloat16


def summarise(per_round, native, others, nbytes):
    """Round medians per operator, and native / other per ``others`` with the ratio of their bytes beside it."""
    keys = [native] + list(others)
    med = {k: statistics.median(r[k] for r in per_round) for k in keys}
    out = {k + "_us": [round(r[k], 2) for r in per_round] for k in keys}
    out["bytes"] = nbytes
    out["spread"] = round(max((max(r[k] for r in per_round) - min(r[k] for r in per_round)) / med[k] for k in keys), 4)
    for k in keys:
        out[k + "_TBps"] = round(nbytes[k] / (med[k] * 1e-6) / 1e12, 3)
    for o in others:
        out[f"{native}_over_{o}"] = round(statistics.median(r[native] / r[o] for r in per_round), 4)
        out[f"{native}_over_{o}_bytes"] = round(nbytes[native] / nbytes[o], 4)
    return out


def bench_shape(dev, name, B, n, knn, C, H, W, rounds, iters, blocker):
    rng = np.random.RandomState(7)
    if knn is None:
        g = m.batch([m.complete_graph(n) for _ in range(B)])
    else:
        g = m.batch([m.RobotGraph(*m.knn_edges(rng.standard_normal((n, 3)), knn), num_nodes=n) for _ in range(B)])
    csr = g.csr(dev)
    Nt, E, P = g.num_nodes(), g.num_edges(), H * W
    NCP = Nt * C * P
    per_set = NCP * (2 + 2 + 1 + 4 + 4)  # x, out, codes, the dequantised copy, the fp32 output
    nsets = max(2, -(-MIN_FOOTPRINT // per_set))
    gen = torch.Generator(device="cpu").manual_seed(11)
    legs = []
    for fmt in FORMATS:
        sets = []
        for _ in range(nsets):
            x = torch.randn(Nt, C, H, W, generator=gen).to(dev).to(T)
            xq, sc = m.quantize_features(x, fmt)
            w = torch.rand(Nt, H, W, generator=gen).to(dev)
            sets.append(dict(x=x, xq=xq, sc=sc, w=torch.where(w < 0.3, torch.zeros_like(w), w),
                             gb=torch.rand(E, C, 2, generator=gen).to(dev),
                             out=torch.empty(Nt, C, H, W, device=dev, dtype=T),
                             out32=torch.empty(Nt, C, H, W, device=dev, dtype=torch.float32)))
        gbb, scb = E * C * 8, Nt * C * 4
        with torch.no_grad():
            # the max
            v = {"max_q": [lambda s=s: aggregate.film_max_q_forward_into(s["xq"], s["sc"], s["gb"], csr, s["out"])
                           for s in sets],
                 "max_bf16": [lambda s=s: m.film_max_forward_into(s["x"], s["gb"], csr, 0, s["out"]) for s in sets],
                 "deq_max": [lambda s=s: m.film_max_forward_into(m.dequantize_features(s["xq"], s["sc"]), s["gb"], csr,
                                                                 0, s["out32"]) for s in sets]}
            nb = {"max_q": NCP * (1 + 2) + gbb + scb, "max_bf16": NCP * (2 + 2) + gbb,
                  "deq_max": NCP * (1 + 4) + scb + NCP * (4 + 4) + gbb}
            legs.append({"op": "film_max", "fmt": fmt,
                         **summarise(rounds_of(v, rounds, iters, blocker), "max_q", ("max_bf16", "deq_max"), nb)})
            for heads in HEADS:
                attn = torch.empty(aggregate._weights_shape(csr, P, heads), device=dev, dtype=torch.float32)
                ab = heads * E * P * 4
                nb = {"q": NCP * (2 * 1 + 2 + 2) + 2 * gbb + 2 * scb + ab, "bf16": NCP * (2 * 2 + 2) + 2 * gbb + ab,
                      "deq": NCP * (1 + 4) + scb + NCP * (2 * 4 + 4) + 2 * gbb + ab}
                v = {"q": [lambda s=s: aggregate.film_attn_q_forward_into(s["x"], s["xq"], s["sc"], s["gb"], csr,
                                                                          s["out"], heads=heads, attn=attn)
                           for s in sets],
                     "bf16": [lambda s=s: m.film_attn_forward_into(s["x"], s["gb"], csr, 0, s["out"], attn=attn,
                                                                   heads=heads) for s in sets],
                     "deq": [lambda s=s: m.film_attn_forward_into(m.dequantize_features(s["xq"], s["sc"]), s["gb"], csr,
                                                                  0, s["out32"], attn=attn, heads=heads)
                             for s in sets]}
                legs.append({"op": "film_attn", "fmt": fmt, "heads": heads,
                             **summarise(rounds_of(v, rounds, iters, blocker), "q", ("bf16", "deq"), nb)})
                wb = Nt * P * 4
                nb = {k: b + wb for k, b in nb.items()}
                v = {"q": [lambda s=s: aggregate.film_wattn_q_forward_into(s["x"], s["xq"], s["sc"], s["gb"], s["w"],
                                                                           csr, s["out"], heads=heads, attn=attn)
                           for s in sets],
                     "bf16": [lambda s=s: m.film_wattn_forward_into(s["x"], s["gb"], s["w"], csr, 0, s["out"],
                                                                    attn=attn, heads=heads) for s in sets],
                     "deq": [lambda s=s: m.film_wattn_forward_into(m.dequantize_features(s["xq"], s["sc"]), s["gb"],
                                                                   s["w"], csr, 0, s["out32"], attn=attn, heads=heads)
                             for s in sets]}
                legs.append({"op": "film_wattn", "fmt": fmt, "heads": heads,
                             **summarise(rounds_of(v, rounds, iters, blocker), "q", ("bf16", "deq"), nb)})
        del sets
        torch.cuda.empty_cache()
    return {"shape": name, "B": B, "n": n, "knn": knn, "C": C, "H": H, "W": W, "dtype": "bf16", "sets": nsets,
            "graph_kind": csr.graph_kind, "legs": legs}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_attn_bench.json"))
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

    result = {"tool": "bench_fp8_attn", "device": torch.cuda.get_device_name(dev), "rounds": a.rounds,
              "iters": a.iters, "warmup": WARMUP, "abi": _lib.ABI_VERSION, "shapes": []}
    for shape in SHAPES:
        result["shapes"].append(bench_shape(dev, *shape, a.rounds, a.iters, blocker))
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
