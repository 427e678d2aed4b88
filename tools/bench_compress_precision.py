"""The fp32 split-bf16 compress in its three precision modes (``compress.set_compress_precision``:
``highest`` six partial products, ``high`` three, ``medium`` one) against the PARENT COMMIT's library,
timed in one process on one GPU.

Rows: the ``cat_compress`` layer shapes of BASELINE configs[1] (Nt = 128, C = 512, 32 x 32), configs[2]
(256, 1280, 8 x 8), configs[3] (64, 2048, 8 x 8) and configs[4] (128, 1024, 16 x 16, k-NN(4) graphs of 16).

* the forward, the data gradient and the weight gradient alone, HIP-graph timed (``bench.time_launches``:
  ``--iters`` launches captured once, the median of 5 replays), operand sets rotated over more than twice the
  Infinity Cache, random operands; the variants — ``parent`` (the parent library), ``parent_again`` (the same
  library a second time in every round), ``highest``, ``high``, ``medium`` (this build) — take turns within
  each of ``--rounds`` rounds, the order rotated by one from round to round (on a power-limited chip a variant
  that always follows a light one would start at a higher clock);
* the layer's training step (``GCNStack`` of one ``cat_compress`` layer, forward + backward), events around
  every call behind queued copies, the same variants taking turns call by call
  (``tools/bench_half_io.timed_interleaved``).

The baseline of every ratio is the parent library's median, not this build's ``highest``.  The margin is the
parent's own run-to-run spread: the largest relative difference between ``parent`` and ``parent_again``
medians and between either's rounds.  ``highest`` must sit within it (``within_margin``); a reduced mode
counts as faster only when it beats the parent by more than it (``faster``).  Also records the accuracy
figures of ``tests/test_gpu_compress_precision.py`` (error against float64, and as a fraction of the derived
truncation term).  Prints one JSON line and writes ``profiles/compress_precision_bench.json``.

The parent library: build the parent commit's sources into ``tools/bin/<name>.so`` (a checkout of the
parent in another directory and ``tools/build_variant_lib.py`` there with an empty PATCH, or its
``lib/libmrp_gnn.so`` copied), then

    python tools/bench_compress_precision.py --parent tools/bin/parent.so [--iters 20] [--rounds 5]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
import mrp_gnn_amd as m  # noqa: E402
from mrp_gnn_amd import _lib, aggregate, compress  # noqa: E402
from tools.bench_half_io import frames, timed_interleaved  # noqa: E402

SHAPES = {
    # name: (graphs, nodes per graph, k-NN degree or None, C, H, W)
    "configs1": (16, 8, None, 512, 32, 32),
    "configs2": (32, 8, None, 1280, 8, 8),
    "configs3": (8, 8, None, 2048, 8, 8),
    "configs4": (8, 16, 4, 1024, 16, 16),
}
MODES = ("highest", "high", "medium")
VARIANTS = ("parent", "parent_again") + MODES
OPS = ("fwd", "dgrad", "wgrad")
NEW_SYMBOLS = ("mrp_compress_fwd_split_p", "mrp_compress_bwd_data_split_p", "mrp_compress_bwd_weight_split_p")


def load_parent(path):
    """The parent library with this build's declarations; the entry points it does not have yet are never
    called on it (the parent variants run in ``highest``, i.e. through the entry points it has)."""
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in NEW_SYMBOLS:
        if not hasattr(lib, name):
            setattr(lib, name, types.SimpleNamespace())
    _lib._declare(lib)
    return lib


def rotated(r):
    """The variants in round r's order."""
    r %= len(VARIANTS)
    return VARIANTS[r:] + VARIANTS[:r]


def use(lib, mode):
    def setup():
        _lib._lib = lib
        compress.set_compress_precision(mode)
    return setup


def summarise(times):
    """times: variant -> list of seconds (or us) per round.  Medians, the parent's spread, ratios."""
    med = {k: statistics.median(v) for k, v in times.items()}
    base = statistics.median(times["parent"] + times["parent_again"])
    pooled = times["parent"] + times["parent_again"]
    margin = max(abs(med["parent"] - med["parent_again"]) / base, (max(pooled) - min(pooled)) / base)
    row = {"parent_us": round(base * 1e6, 2), "parent_medians_us": [round(med["parent"] * 1e6, 2),
                                                                    round(med["parent_again"] * 1e6, 2)],
           "margin": round(margin, 4)}
    for k in MODES:
        r = med[k] / base
        row[k] = {"us": round(med[k] * 1e6, 2), "min_us": round(min(times[k]) * 1e6, 2), "vs_parent": round(r, 4)}
    row["highest"]["within_margin"] = abs(row["highest"]["vs_parent"] - 1.0) <= margin
    for k in ("high", "medium"):
        row[k]["faster"] = row[k]["vs_parent"] < 1.0 - margin
    return row


def bench_shape(name, dev, iters, rounds, libs):
    B, n, knn, C, H, W = SHAPES[name]
    g = frames(B, n, knn).to(dev)
    Nt, P = g.num_nodes(), H * W
    gen = torch.Generator(device=dev).manual_seed(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = aggregate._ptr

    def rand():
        return torch.randn(Nt, C, H, W, device=dev, generator=gen)

    torch.manual_seed(0)
    stack = m.GCNStack(types.SimpleNamespace(feature_dim=C, gcn_layers=1, gcn_combine="cat_compress")).to(dev)
    w, b = stack.conv1.weight.detach(), stack.conv1.bias.detach()
    flops = 2.0 * Nt * P * C * 2 * C
    k = max(2, bench.rotating_sets(3 * Nt * C * P * 4))
    sets = [(rand(), rand(), rand()) for _ in range(k)]
    calls = {"fwd": [(lambda x=x, a=a: compress.compress_forward(w, b, x, a)) for x, a, _ in sets],
             "dgrad": [(lambda gy=gy: compress.compress_backward_data(w, gy)) for _, _, gy in sets],
             "wgrad": [(lambda x=x, a=a, gy=gy: compress.compress_backward_weight(gy, x, a)) for x, a, gy in sets]}
    setups = {"parent": use(libs["parent"], "highest"), "parent_again": use(libs["parent"], "highest"),
              "highest": use(libs["this"], "highest"), "high": use(libs["this"], "high"),
              "medium": use(libs["this"], "medium")}
    row = {"graphs": B, "nodes": n, "knn": knn, "Nt": Nt, "C": C, "H": H, "W": W, "rotated_sets": k,
           "product_flops": flops}
    try:
        with torch.no_grad():
            for op in OPS:
                times = {v: [] for v in VARIANTS}
                for r in range(rounds):
                    for v in rotated(r):
                        setups[v]()
                        times[v].append(bench.time_launches(calls[op], iters, dev))
                row[op] = summarise(times)
                for v in MODES:
                    row[op][v]["tflops"] = round(flops / (row[op][v]["us"] * 1e-6) * 1e-12, 1)

        block_a = torch.empty(256 << 20, device=dev, dtype=torch.uint8)
        block_b = torch.empty_like(block_a)
        lib = libs["this"]

        def blocker():
            for _ in range(40):
                _lib.check(lib.mrp_stream_copy(ptr(block_a), ptr(block_b), block_a.numel(), stream), "mrp_stream_copy")

        def one(x, G):
            def call():
                for p in stack.parameters():
                    p.grad = None
                x.grad = None
                stack(g, x).backward(G)
            return call
        steps = [one(x.requires_grad_(True), G) for x, _, G in sets]
        times = {v: [] for v in VARIANTS}
        for r in range(rounds):
            t = timed_interleaved({v: (setups[v], steps) for v in rotated(r)}, max(iters, 20), blocker)
            for v in VARIANTS:
                times[v].append(t[v] * 1e-6)
        row["layer_step"] = summarise(times)
    finally:
        _lib._lib = libs["this"]
        compress.set_compress_precision("highest")
    for x, _, _ in sets:
        x.requires_grad_(False)
        x.grad = None
    del sets, calls, steps
    torch.cuda.empty_cache()
    return row


def accuracy(dev):
    """The random-operand figures of tests/test_gpu_compress_precision.py: per mode and product the error
    against float64 (max |d| / max |ref|) and the largest |d| as a fraction of the derived truncation term
    c sum_k |a_k b_k| (c = 3.1 x 2^-18 / 2.01 x 2^-9)."""
    bound = {"high": 3.1 * 2.0 ** -18, "medium": 2.01 * 2.0 ** -9}
    torch.manual_seed(11)
    n, C, P = 2, 512, 32
    w = torch.randn(C, 2 * C, device=dev) * (2 * C) ** -0.5
    b = torch.randn(C, device=dev)
    cat = torch.randn(n, 2 * C, P, device=dev)
    gy = torch.randn(n, C, P, device=dev)
    torch.manual_seed(12)
    n2, C2, P2 = 32, 64, 32
    gy2 = torch.randn(n2, C2, P2, device=dev) * (n2 * P2) ** -0.5
    cat2 = torch.randn(n2, 2 * C2, P2, device=dev)
    rows = lambda t: t.double().permute(1, 0, 2).reshape(t.shape[1], -1)  # noqa: E731
    ref = {"fwd": (torch.matmul(w.double(), cat.double()) + b.double()[None, :, None],
                   torch.matmul(w.double().abs(), cat.double().abs())),
           "dgrad": (torch.matmul(w.double().t(), gy.double()), torch.matmul(w.double().abs().t(), gy.double().abs())),
           "wgrad": (rows(gy2) @ rows(cat2).t(), rows(gy2).abs() @ rows(cat2).abs().t())}
    x, a = (cat[:, i * C:(i + 1) * C].reshape(n, C, 4, P // 4) for i in (0, 1))
    x2, a2 = (cat2[:, i * C2:(i + 1) * C2].reshape(n2, C2, 4, P2 // 4) for i in (0, 1))
    out = {}
    for mode in MODES:
        with compress.compress_precision_scope(mode):
            y = compress.compress_forward(w.view(C, 2 * C, 1, 1), b, x, a)
            gx, ga = compress.compress_backward_data(w.view(C, 2 * C, 1, 1), gy.view(n, C, 4, P // 4))
            gw, _ = compress.compress_backward_weight(gy2.view(n2, C2, 4, P2 // 4), x2, a2)
        got = {"fwd": y.view(n, C, P), "dgrad": torch.cat((gx, ga), 1).view(n, 2 * C, P), "wgrad": gw.view(C2, 2 * C2)}
        out[mode] = {}
        for op, (f64, mag) in ref.items():
            d = (got[op].double() - f64).abs()
            rec = {"err": float(d.max() / f64.abs().max())}
            if mode in bound:
                rec["of_truncation_term"] = round(float((d / (bound[mode] * mag)).max()), 4)
            out[mode][op] = rec
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", required=True, help="the parent commit's library (tools/bin/<name>.so)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compress_precision_bench.json"))
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be >= 3 (the parent's spread is taken over the rounds)")
    dev = torch.device("cuda:0")
    libs = {"this": _lib.load_library(), "parent": load_parent(a.parent)}
    compress.set_compress_path("split")
    result = {"tool": "bench_compress_precision", "device": torch.cuda.get_device_name(dev), "iters": a.iters,
              "rounds": a.rounds, "abi": _lib.ABI_VERSION, "accuracy": accuracy(dev), "shapes": {}}
    for name in a.shapes.split(","):
        result["shapes"][name] = bench_shape(name, dev, a.iters, a.rounds, libs)
        print(name, json.dumps(result["shapes"][name]), file=sys.stderr, flush=True)
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
