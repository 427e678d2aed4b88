"""Range-limited robot graphs (kind ``GRAPH_SIMPLE``), timed in one run on one GPU.

Shape: BASELINE configs[4]'s — B = 8 frames, C = 1024, 16x16 planes, fp32 and bf16 — at N = 16 and N = 12
robots, on range graphs of mean in-degree about 4 and about 8 drawn from a seed (the range is the quantile of
the batch's pairwise distances that gives the degree).

* backward A/B: the same CSR arrays through kind ``GRAPH_SIMPLE`` (``film_bwd_mfma``, CSR-row form, its
  clearing of the unnamed grad_gb rows included) against kind ``GRAPH_CSR`` (``film_bwd_dx`` + the Gram pass:
  the route such a graph had before the kind existed; its plan is asserted).  The two take turns call by call in
  one process, for ``--rounds`` (>= 5) rounds of ``--iters`` calls each; per round the median per route, over
  the rounds the median ratio and the spread ((max - min) / median of a route's round medians, the larger of
  the two).  Outputs of the two routes are compared at the timed size.
* forward of both kinds (the same kernel: expected equal).
* achieved bytes/s over the backward's algorithmic bytes: grad_out, x read and grad_x written (Nt C P
  elements each), gamma/beta read and their gradient written for the existing edges (2 C fp32 each).
* the builder: ``frame_batch(poses, max_range=...)`` against ``frame_graph`` per frame + ``batch`` + the copy
  of the CSR and the edge poses to the device, wall clock with a device synchronisation, at B = 32, n = 8
  and B = 8, n = 16.

Protocol as tools/bench_half_io.py: events around every call with the host running ahead of the device, 5
warm-ups, operand sets rotated over more than 512 MB.  Prints one JSON line and writes
``profiles/range_graphs_bench.json``.

    python tools/bench_range_graphs.py [--rounds 5] [--iters 20] [--out PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import mrp_gnn_amd as m  # noqa: E402
from mrp_gnn_amd import _lib, aggregate  # noqa: E402

B, C, H, W = 8, 1024, 16, 16
DTYPES = [("fp32", torch.float32), ("bf16", torch.bfloat16)]
WARMUP = 5
MIN_FOOTPRINT = 512 << 20
TOL = 1e-5  # the suite's fp32 bar (max |d| / max |ref|)


def poses_for(Bn, n, seed):
    rng = np.random.RandomState(seed)
    return np.concatenate([rng.uniform(-10, 10, (Bn, n, 3)), rng.standard_normal((Bn, n, 4))], -1).astype(np.float32)


def range_for_degree(poses, degree):
    """The range at which the batch's mean in-degree is about ``degree``: that quantile of the pair distances."""
    t = poses[..., :3].astype(np.float64)
    d = np.linalg.norm(t[:, :, None] - t[:, None, :], axis=-1)
    n = poses.shape[1]
    pairs = d[:, ~np.eye(n, dtype=bool)]
    return float(np.quantile(pairs, degree / (n - 1)))


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


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


def summarise(per_round, a, b):
    """Ratio a / b over the rounds and the routes' spread."""
    ratios = [r[a] / r[b] for r in per_round]
    spread = max((max(r[k] for r in per_round) - min(r[k] for r in per_round)) / statistics.median(r[k] for r in per_round)
                 for k in (a, b))
    return {a + "_us": [round(r[a], 2) for r in per_round], b + "_us": [round(r[b], 2) for r in per_round],
            "ratio_per_round": [round(x, 4) for x in ratios], "ratio": round(statistics.median(ratios), 4),
            "spread": round(spread, 4)}


def bench_aggregation(dev, n, degree, label, T, rounds, iters, blocker):
    poses = poses_for(B, n, seed=1000 + n)
    rng_ = range_for_degree(poses, degree)
    g = m.batch([m.frame_graph(p, max_range=rng_) for p in poses])
    kinds = {"simple": g.csr(dev), "csr": g.csr(dev, simple=False)}
    Nt, E, P = g.num_nodes(), g.num_edges(), H * W
    e_act = int(g.edge_active.sum())
    plans = {k: aggregate.launch_plan("bwd", c, C, P, dtype=T, logits=True).kernel_name for k, c in kinds.items()}
    assert plans["csr"] == "film_bwd_dx_gram", plans  # the route before the kind existed
    fplans = {k: aggregate.launch_plan("fwd", c, C, P, dtype=T, logits=True).kernel_name for k, c in kinds.items()}
    assert fplans["simple"] == fplans["csr"], fplans
    lib = _lib.load_library()
    gen = torch.Generator(device=dev).manual_seed(n * 10 + degree)
    z = torch.randn(E, C, 2, device=dev, generator=gen)
    mode = _lib.MODE_FILM_MEAN | _lib.GB_LOGITS
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = aggregate._ptr
    dt = aggregate.FEATURE_DTYPES[T]
    stride = C * P
    elem = torch.empty((), dtype=T).element_size()
    tensor_bytes = Nt * C * P * elem
    sets = []
    for _ in range(max(2, -(-MIN_FOOTPRINT // (3 * tensor_bytes)) + 1)):
        x = torch.randn(Nt, C, H, W, device=dev, generator=gen).to(T)
        G = torch.randn(Nt, C, H, W, device=dev, generator=gen).to(T)
        sets.append((x, torch.empty_like(x), G, torch.empty_like(x), torch.zeros(E, C, 2, device=dev)))

    def graph_args(c):
        return (ptr(z), ptr(c.indptr), ptr(c.src), ptr(c.eid), ptr(c.graph_off), c.num_graphs, c.max_nodes,
                c.graph_kind, c.num_nodes, c.num_edges, C, P, mode)

    def bwd(c, s):
        x, _, G, dx, dgb = s
        args = (dt, ptr(G), stride, ptr(x), stride) + graph_args(c) + (ptr(dx), stride, None, 0, ptr(dgb), None, stream)
        return lambda: _lib.check(lib.mrp_film_mean_bwd_t(*args), "mrp_film_mean_bwd_t")

    def fwd(c, s):
        args = (dt, ptr(s[0]), stride) + graph_args(c) + (ptr(s[1]), stride, None, stream)
        return lambda: _lib.check(lib.mrp_film_mean_fwd_t(*args), "mrp_film_mean_fwd_t")

    # the two routes' outputs at the timed size (grad_gb starts as zeros: the CSR route leaves unnamed rows alone)
    outs = {}
    for k, c in kinds.items():
        x, out, G, dx, dgb = sets[0]
        fwd(c, sets[0])()
        bwd(c, sets[0])()
        torch.cuda.synchronize()
        outs[k] = (out.clone(), dx.clone(), dgb.clone())
    agree = {"out_bit_equal": bool(torch.equal(outs["simple"][0], outs["csr"][0])),
             "dx_rel": rel(outs["simple"][1], outs["csr"][1]), "dgb_rel": rel(outs["simple"][2], outs["csr"][2])}
    # 16-bit grad_x: each route rounds its fp32 value once, so they may differ by the rounding (2^-8 for bf16)
    dx_bar = TOL if T == torch.float32 else 2.0 ** -7
    assert agree["out_bit_equal"] and agree["dx_rel"] <= dx_bar and agree["dgb_rel"] <= TOL, agree
    del outs

    bw = summarise(rounds_of({k: [bwd(c, s) for s in sets] for k, c in kinds.items()}, rounds, iters, blocker),
                   "simple", "csr")
    fw = summarise(rounds_of({k: [fwd(c, s) for s in sets] for k, c in kinds.items()}, rounds, iters, blocker),
                   "simple", "csr")
    bytes_bwd = 3 * tensor_bytes + 2 * e_act * 2 * C * 4
    t_s, t_c = statistics.median(bw["simple_us"]), statistics.median(bw["csr_us"])
    row = {"N": n, "dtype": label, "target_degree": degree, "max_range": round(rng_, 4),
           "mean_in_degree": round(e_act / Nt, 3), "edge_slots": E, "edges": e_act, "rotated_sets": len(sets),
           "bwd_plan": plans, "fwd_plan": fplans["simple"], "agreement": agree, "bwd": bw, "fwd": fw,
           "bwd_bytes": bytes_bwd, "bwd_simple_tbps": round(bytes_bwd / t_s * 1e-6, 3),
           "bwd_csr_tbps": round(bytes_bwd / t_c * 1e-6, 3),
           "simple_faster_beyond_spread": bool(bw["ratio"] < 1.0 - bw["spread"]),
           "simple_is_mfma": plans["simple"] == "film_bwd_mfma"}
    del sets
    torch.cuda.empty_cache()
    return row


def bench_builder(dev, Bn, n, reps=20):
    poses = poses_for(Bn, n, seed=7 * Bn + n)
    rng_ = range_for_degree(poses, min(4, n - 1))
    pd = torch.from_numpy(poses).to(dev)

    def device_build():
        g = m.frame_batch(pd, max_range=rng_)
        return g.csr(dev), g.edata["pose"]

    def host_build():
        g = m.batch([m.frame_graph(p, max_range=rng_) for p in poses])
        return g.csr(dev), g.edata["pose"].to(dev)

    res = {}
    for name, fn in (("device", device_build), ("host", host_build)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        res[name + "_us"] = round(statistics.median(ts), 1)
    # the device build's own time on the device: events around the call, the host running ahead
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        device_build()
        b.record()
    torch.cuda.synchronize()
    res["device_event_us"] = round(statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3, 1)
    res.update(B=Bn, n=n, host_over_device=round(res["host_us"] / res["device_us"], 1))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_graphs_bench.json"))
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

    result = {"tool": "bench_range_graphs", "device": torch.cuda.get_device_name(dev), "rounds": a.rounds,
              "iters": a.iters, "warmup": WARMUP, "abi": _lib.ABI_VERSION, "B": B, "C": C, "H": H, "W": W,
              "aggregation": [], "builder": []}
    for n in (16, 12):
        for degree in (4, 8):
            for label, T in DTYPES:
                result["aggregation"].append(bench_aggregation(dev, n, degree, label, T, a.rounds, a.iters, blocker))
    for Bn, n in ((32, 8), (8, 16)):
        result["builder"].append(bench_builder(dev, Bn, n))
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
