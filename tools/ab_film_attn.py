#!/usr/bin/env python3
"""Kernel lab (not product code): film_attn of the product library against another build of the library (for
instance the parent commit's, or a tools/build_variant_lib.py variant) in one process, as tools/ab_libs.py does
for the mean kernels, at tools/bench_film_attn.py's shapes and with its protocol.

Three variants take turns call by call on the same operands: the product library ("this"), the other build
("other") and a second load of the other build ("other2": the same code under another handle).  Per leg: the
median over the rounds of this / other, and the range of other2 / other over the rounds: the spread the other
build shows against itself in the same run.  The outputs of the two builds are compared bit for bit.  Prints one
JSON line; ``--out PATH`` also writes it.

usage: python tools/ab_film_attn.py <other.so> [--rounds 5] [--iters 20] [--out PATH]"""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mrp_gnn_amd as m  # noqa: E402
from mrp_gnn_amd import _lib, aggregate  # noqa: E402
from bench_film_attn import DTYPES, MIN_FOOTPRINT, SHAPES, rounds_of  # noqa: E402

USED = ("mrp_film_attn_fwd", "mrp_film_attn_bwd", "mrp_film_attn_workspace", "mrp_error_string", "mrp_stream_copy")


def load_other(path, product):
    """The other build under a handle of its own, with the product's declarations of the functions used here (it
    may lack entry points the product has)."""
    lib = ctypes.CDLL(path)
    for name in USED:
        getattr(lib, name).argtypes = getattr(product, name).argtypes
        getattr(lib, name).restype = getattr(product, name).restype
    return lib


def with_lib(lib, f):
    def call():
        _lib._lib = lib
        return f()
    return call


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("other")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    this = _lib.load_library()
    tmp = tempfile.mkdtemp()
    second = shutil.copy(a.other, os.path.join(tmp, "other2.so"))
    libs = {"this": this, "other": load_other(os.path.abspath(a.other), this), "other2": load_other(second, this)}
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    block_a = torch.empty(256 << 20, device=dev, dtype=torch.uint8)
    block_b = torch.empty_like(block_a)

    def blocker():
        for _ in range(40):
            this.mrp_stream_copy(aggregate._ptr(block_a), aggregate._ptr(block_b), block_a.numel(), stream)

    result = {"tool": "ab_film_attn", "device": torch.cuda.get_device_name(dev), "rounds": a.rounds,
              "iters": a.iters, "legs": []}
    for name, B, n, knn, C, H, W in SHAPES:
        for label, T in DTYPES:
            rng = np.random.RandomState(7)
            if knn is None:
                g = m.batch([m.complete_graph(n) for _ in range(B)])
            else:
                g = m.batch([m.RobotGraph(*m.knn_edges(rng.standard_normal((n, 3)), knn), num_nodes=n)
                             for _ in range(B)])
            csr = g.csr(dev)
            Nt, E, P = g.num_nodes(), g.num_edges(), H * W
            per_set = 4 * Nt * C * P * torch.empty(0, dtype=T).element_size()
            gen = torch.Generator(device="cpu").manual_seed(11)
            sets = []
            for _ in range(max(2, -(-MIN_FOOTPRINT // per_set))):
                sets.append(dict(x=torch.randn(Nt, C, H, W, generator=gen).to(dev).to(T),
                                 G=torch.randn(Nt, C, H, W, generator=gen).to(dev).to(T),
                                 gb=torch.rand(E, C, 2, generator=gen).to(dev),
                                 out=torch.empty(Nt, C, H, W, device=dev, dtype=T),
                                 attn=torch.empty(E, P, device=dev, dtype=torch.float32)))
            same = True
            outs = {}
            for k in ("this", "other"):
                _lib._lib = libs[k]
                s = sets[0]
                o = torch.empty_like(s["out"])
                at = m.film_attn_forward_into(s["x"], s["gb"], csr, 0, o)
                outs[k] = (o, at) + m.film_attn_backward(s["G"], s["x"], s["gb"], at, csr, 0, True, True)
            same = all(torch.equal(p.view(torch.uint8), q.view(torch.uint8)) for p, q in zip(outs["this"], outs["other"]))
            _lib._lib = this
            for s in sets:
                m.film_attn_forward_into(s["x"], s["gb"], csr, 0, s["out"], attn=s["attn"])
            fwd = {k: [with_lib(lib, lambda s=s: m.film_attn_forward_into(s["x"], s["gb"], csr, 0, s["out"],
                                                                           attn=s["attn"])) for s in sets]
                   for k, lib in libs.items()}
            bwd = {k: [with_lib(lib, lambda s=s: m.film_attn_backward(s["G"], s["x"], s["gb"], s["attn"], csr, 0, True,
                                                                      True)) for s in sets]
                   for k, lib in libs.items()}
            leg = {"shape": name, "dtype": label, "bit_identical": same}
            for d, variants in (("forward", fwd), ("backward", bwd)):
                per_round = rounds_of(variants, a.rounds, a.iters, blocker)
                own = [r["other2"] / r["other"] for r in per_round]
                leg[d] = {"us": {k: [round(r[k], 2) for r in per_round] for k in libs},
                          "this_over_other": round(statistics.median(r["this"] / r["other"] for r in per_round), 4),
                          "other_over_itself": [round(min(own), 4), round(max(own), 4)]}
            _lib._lib = this
            result["legs"].append(leg)
            del sets, outs
            torch.cuda.empty_cache()
    shutil.rmtree(tmp)
    line = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
