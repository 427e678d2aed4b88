"""Multi-head attention fusion (``film_attn(..., heads=H)``) against the two routes a user had before it, on
identical tensors, timed in one run on one GPU.

Legs: forward and backward (grad_x and grad_gb), fp32 and bf16, H in {1, 4, 8}, at tools/bench_film_attn.py's
three shapes (the headline shape, BASELINE configs[2] and configs[4]).  Three variants take turns call by call:

  * ``mh``      (a) the one-launch H-head call (``mrp_film_attn_fwd_mh`` / ``_bwd_mh``; H = 1 takes the single-head
                entry points, as the ops do);
  * ``slices``  (b) what a user had: H single-head calls on the heads' channel slices through the existing op
                (strided views of x and grad_out, gb[:, slice] copied by the op as it always is) and the
                concatenation of the H results (``torch.cat`` of out; of grad_x and of grad_gb);
  * ``single``  (c) single-head attention over all C channels: another function, the cost the heads are measured
                against.

Per leg: the round medians of each variant, the ratios a / b and a / c per round and their medians, and the spread
((max - min) / median of a variant's round medians, the largest of the three).  tools/bench_film_attn.py's
protocol: events around every call with the host running ahead of the device, 5 warm-ups, operand sets rotated
over more than 512 MB, ``--rounds`` (>= 5) rounds of ``--iters`` calls.  Prints one JSON line and writes
``profiles/film_attn_heads_bench.json``.

    python tools/bench_film_attn_heads.py [--rounds 5] [--iters 20] [--out PATH]
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

HEADS = (1, 4, 8)
VARIANTS = ("mh", "slices", "single")


def summarise(per_round):
    med = {k: statistics.median(r[k] for r in per_round) for k in VARIANTS}
    spread = max((max(r[k] for r in per_round) - min(r[k] for r in per_round)) / med[k] for k in VARIANTS)
    out = {k + "_us": [round(r[k], 2) for r in per_round] for k in VARIANTS}
    for name, den in (("mh_over_slices", "slices"), ("mh_over_single", "single")):
        ratios = [r["mh"] / r[den] for r in per_round]
        out[name + "_per_round"] = [round(x, 4) for x in ratios]
        out[name] = round(statistics.median(ratios), 4)
    out["spread"] = round(spread, 4)
    return out


def variants_of(sets, csr, H, C):
    """{variant: [one callable per operand set]} for the forward and for the backward."""
    Ch = C // H
    sls = [slice(k * Ch, (k + 1) * Ch) for k in range(H)]

    def fwd_slices(s):
        outs = []
        for k, sl in enumerate(sls):
            o = torch.empty_like(s["out"][:, sl], memory_format=torch.contiguous_format)
            m.film_attn_forward_into(s["x"][:, sl], s["gb"][:, sl], csr, 0, o, attn=s["attn_h"][k])
            outs.append(o)
        return torch.cat(outs, 1)

    def bwd_slices(s):
        res = [m.film_attn_backward(s["G"][:, sl], s["x"][:, sl], s["gb"][:, sl], s["attn_h"][k], csr, 0, True, True)
               for k, sl in enumerate(sls)]
        return torch.cat([r[0] for r in res], 1), torch.cat([r[1] for r in res], 1)

    fwd = {"mh": [lambda s=s: m.film_attn_forward_into(s["x"], s["gb"], csr, 0, s["out"],
                                                       attn=s["attn_h"] if H > 1 else s["attn_h"][0], heads=H)
                  for s in sets],
           "slices": [lambda s=s: fwd_slices(s) for s in sets],
           "single": [lambda s=s: m.film_attn_forward_into(s["x"], s["gb"], csr, 0, s["out"], attn=s["attn_1"])
                      for s in sets]}
    bwd = {"mh": [lambda s=s: m.film_attn_backward(s["G"], s["x"], s["gb"], s["attn_h"] if H > 1 else s["attn_h"][0],
                                                   csr, 0, True, True, heads=H) for s in sets],
           "slices": [lambda s=s: bwd_slices(s) for s in sets],
           "single": [lambda s=s: m.film_attn_backward(s["G"], s["x"], s["gb"], s["attn_1"], csr, 0, True, True)
                      for s in sets]}
    return fwd, bwd


def bench_shape(dev, name, B, n, knn, C, H, W, label, T, rounds, iters, blocker):
    rng = np.random.RandomState(7)
    if knn is None:
        g = m.batch([m.complete_graph(n) for _ in range(B)])
    else:
        g = m.batch([m.RobotGraph(*m.knn_edges(rng.standard_normal((n, 3)), knn), num_nodes=n) for _ in range(B)])
    csr = g.csr(dev)
    Nt, E, P = g.num_nodes(), g.num_edges(), H * W
    elem = torch.empty(0, dtype=T).element_size()
    nsets = max(2, -(-MIN_FOOTPRINT // (4 * Nt * C * P * elem)))
    gen = torch.Generator(device="cpu").manual_seed(11)
    sets = []
    for _ in range(nsets):
        sets.append(dict(x=torch.randn(Nt, C, H, W, generator=gen).to(dev).to(T),
                         G=torch.randn(Nt, C, H, W, generator=gen).to(dev).to(T),
                         gb=torch.rand(E, C, 2, generator=gen).to(dev),
                         out=torch.empty(Nt, C, H, W, device=dev, dtype=T),
                         attn_1=torch.empty(E, P, device=dev, dtype=torch.float32)))
    legs = []
    for heads in HEADS:
        for s in sets:  # the backwards read the weights of their own set
            s["attn_h"] = torch.empty(heads, E, P, device=dev, dtype=torch.float32)
            m.film_attn_forward_into(s["x"], s["gb"], csr, 0, s["out"], attn=s["attn_1"])
            m.film_attn_forward_into(s["x"], s["gb"], csr, 0, s["out"],
                                     attn=s["attn_h"] if heads > 1 else s["attn_h"][0], heads=heads)
        fwd, bwd = variants_of(sets, csr, heads, C)
        legs.append({"shape": name, "B": B, "n": n, "knn": knn, "C": C, "H": H, "W": W, "dtype": label,
                     "heads": heads, "sets": nsets, "graph_kind": csr.graph_kind,
                     "workgroups": {"mh": csr.num_graphs * (-(-P // 64)) * heads,
                                    "single": csr.num_graphs * (-(-P // 64))},
                     "forward": summarise(rounds_of(fwd, rounds, iters, blocker)),
                     "backward": summarise(rounds_of(bwd, rounds, iters, blocker))})
    return legs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "film_attn_heads_bench.json"))
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

    result = {"tool": "bench_film_attn_heads", "device": torch.cuda.get_device_name(dev), "rounds": a.rounds,
              "iters": a.iters, "warmup": WARMUP, "abi": _lib.ABI_VERSION, "heads": list(HEADS), "legs": []}
    for shape in SHAPES:
        for label, T in DTYPES:
            result["legs"] += bench_shape(dev, *shape, label, T, a.rounds, a.iters, blocker)
            torch.cuda.empty_cache()
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
