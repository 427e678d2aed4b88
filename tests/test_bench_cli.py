"""``bench.py``'s command line: a plain run measures the headline figure only, ``--full`` adds the
other measurements, and ``--dump-outputs DIR`` writes what the last timed step returned — the same
arrays from run to run, equal to the layer's output on the benchmark's seeded inputs."""
import importlib.util
import json
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_KEYS = {"roofline", "copy_ceiling", "train_step", "configs", "graph_build", "cpu_baseline"}
TINY = ["--gpus", "1", "--graphs", "3", "--nodes", "5", "--channels", "32", "--hw", "8", "--spinup-s", "0"]


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_cli_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(bench, capsys, argv):
    bench.main(argv)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1  # one JSON result line
    return json.loads(lines[0])


def test_options_default_off(bench):
    args = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (7, 2, False, None)
    args = bench.parse_args(["--full", "--dump-outputs", "somewhere"])
    assert args.full and args.dump_outputs == "somewhere"


def test_dump_outputs_whole_and_sampled(bench, tmp_path, monkeypatch):
    assert bench.DUMP_MAX_BYTES <= 64 << 20  # one array per rank, 64 MB at the most
    x = torch.arange(6000, dtype=torch.float64).reshape(3, 20, 100)
    rec = bench.dump_outputs(str(tmp_path / "new" / "dir"), "whole", x)
    a = np.load(tmp_path / "new" / "dir" / "whole.npy")
    assert a.dtype == np.float32 and np.array_equal(a, np.arange(6000, dtype=np.float32))
    assert rec["elements"] == rec["of"] == 6000 and rec["shape"] == [3, 20, 100] and rec["sample_seed"] is None
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 400)  # 100 elements
    recs = [bench.dump_outputs(str(tmp_path), name, x) for name in ("s1", "s2")]
    s1, s2 = np.load(tmp_path / "s1.npy"), np.load(tmp_path / "s2.npy")
    assert s1.dtype == np.float32 and s1.shape == (100,) and np.array_equal(s1, s2)
    assert recs[0]["elements"] == 100 and recs[0]["of"] == 6000 and recs[0]["sample_seed"] == bench.DUMP_SEED
    # the values are their own flat indices: in range, and spread over the tensor
    assert s1.min() >= 0 and s1.max() < 6000 and len(np.unique(s1 // 1000)) == 6


@pytest.mark.gpu
def test_plain_run_is_headline_only_and_dump_is_reproducible(bench, capsys, tmp_path, cuda_device):
    calls = []
    step_fn = bench.mrp.GCN.forward

    def counting(self, *a, **kw):
        calls.append(1)
        return step_fn(self, *a, **kw)

    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    bench.mrp.GCN.forward = counting
    try:
        r1 = run(bench, capsys, TINY + ["--steps", "3", "--warmup", "2", "--dump-outputs", d1])
    finally:
        bench.mrp.GCN.forward = step_fn
    assert len(calls) == 3 + 2  # --steps timed steps, --warmup warmup steps, nothing else runs the layer
    r2 = run(bench, capsys, TINY + ["--steps", "4", "--warmup", "1", "--dump-outputs", d2])
    for r, steps in ((r1, 3), (r2, 4)):
        assert HEADLINE_KEYS <= set(r) and not FULL_KEYS & set(r)
        assert r["steps"] == steps and r["unit"] == "elems/s" and r["dtype"] == "f32" and r["higher_is_better"] is True
        assert r["ms_per_step"] > 0
        # value is the elements of one step over the step time
        assert r["value"] == pytest.approx(15 * 32 * 64 / (r["ms_per_step"] * 1e-3), rel=1e-9)
    assert os.listdir(d1) == ["gcn_out.npy"]
    a, b = np.load(os.path.join(d1, "gcn_out.npy")), np.load(os.path.join(d2, "gcn_out.npy"))
    assert a.dtype == np.float32 and a.shape == (15 * 32 * 64,) and r1["dumped_outputs"]["sample_seed"] is None
    assert np.array_equal(a, b)
    # the same seeded workload and layer, computed here
    g = bench.make_workload(3, 5, 32, 8, 8, seed=0, device=cuda_device)
    torch.manual_seed(0)
    gcn = bench.mrp.GCN(types.SimpleNamespace(feature_dim=32)).to(cuda_device)
    with torch.no_grad():
        want = gcn(g, g.ndata["image"]).reshape(-1).cpu().numpy()
    assert np.array_equal(a, want)
    assert np.isfinite(a).all() and np.abs(a).max() > 0


@pytest.mark.gpu
def test_dump_of_a_large_output_is_a_fixed_sample(bench, capsys, tmp_path, cuda_device, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)  # 1024 elements of the 30720
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    r = run(bench, capsys, TINY + ["--steps", "2", "--warmup", "1", "--dump-outputs", d1])
    run(bench, capsys, TINY + ["--steps", "2", "--warmup", "1", "--dump-outputs", d2])
    a, b = np.load(os.path.join(d1, "gcn_out.npy")), np.load(os.path.join(d2, "gcn_out.npy"))
    assert a.dtype == np.float32 and a.shape == (1024,) and np.array_equal(a, b)
    assert r["dumped_outputs"]["of"] == 15 * 32 * 64 and r["dumped_outputs"]["sample_seed"] == bench.DUMP_SEED
    g = bench.make_workload(3, 5, 32, 8, 8, seed=0, device=cuda_device)
    torch.manual_seed(0)
    gcn = bench.mrp.GCN(types.SimpleNamespace(feature_dim=32)).to(cuda_device)
    with torch.no_grad():
        want = gcn(g, g.ndata["image"]).reshape(-1).cpu()
    idx = torch.randint(0, want.numel(), (1024,), generator=torch.Generator().manual_seed(bench.DUMP_SEED))
    assert np.array_equal(a, want[idx].numpy())
    assert len(set(idx.tolist())) > 900  # spread over the tensor, not one corner of it


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements(bench, capsys, cuda_device):
    r = run(bench, capsys, TINY + ["--steps", "2", "--warmup", "1", "--full", "--kernel-iters", "2", "--train-steps", "2",
                                   "--configs", "0", "--config-steps", "2", "--cpu-seconds", "0.05"])
    assert HEADLINE_KEYS | FULL_KEYS <= set(r)
    assert set(r["configs"]) == {"configs[0]"} and r["roofline"]["kernel"] == "film_fwd"
    assert r["train_step"]["ms_per_step"] > 0 and r["cpu_baseline"]["value"] > 0
