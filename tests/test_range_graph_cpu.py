"""CPU: range-limited / drop-out robot graphs — graph kind ``GRAPH_SIMPLE`` in the launch planner and the C
ABI's validation, the host builder ``frame_graph(poses, knn, max_range, active)`` against a brute-force
restatement of the edge rule, and what a ``RobotGraph`` with an ``edge_active`` mask shows.  No GPU call is
made: the plan queries and the argument checks are decided on the host.

Before the kind existed the library rejected ``graph_kind = 3`` and the builders had no such arguments.
"""
import ctypes
import itertools
import math
import types

import numpy as np
import pytest
import torch

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib, aggregate
import geometry_cases as gc

HIP_INVALID_VALUE = 1
KEYS = ("f32", "bf16", "f16")


def simple_ns(ns, kind=None, extra_rows=0):
    """Graph arguments of a batch with ``ns`` nodes per graph: gamma/beta rows for every ordered pair (plus
    ``extra_rows``), as a range-limited frame has them whatever edges exist."""
    E = sum(n * (n - 1) for n in ns) + extra_rows
    return types.SimpleNamespace(num_graphs=len(ns), max_nodes=max(ns), graph_kind=_lib.GRAPH_SIMPLE if kind is None
                                 else kind, num_nodes=sum(ns), num_edges=E)


# ------------------------------------------------------------------------------------------------ plans
@pytest.mark.parametrize("base", [False, True])
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("C", [1, 7, 9, 17])
@pytest.mark.parametrize("P", [64, 256])
@pytest.mark.parametrize("n", [9, 12, 16])
def test_simple_graphs_of_9_to_16_nodes_plan_the_matrix_core_backward(n, P, C, key, base):
    g = simple_ns((n, n, n - 2))
    p = aggregate.launch_plan("bwd", g, C, P, dtype=gc.DTYPES[key], grad_x_base=base)
    assert p.kernel_name == "film_bwd_mfma"
    assert gc.violations(p, key, g, C, P, 16) == []


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("n", [9, 12, 16])
def test_shapes_the_matrix_core_kernel_does_not_take_keep_the_two_pass_route(n, key):
    g = simple_ns((n, n - 1))
    for P in (16, 144):
        p = aggregate.launch_plan("bwd", g, 7, P, dtype=gc.DTYPES[key])
        assert p.kernel_name == "film_bwd_dx_gram", P
        assert gc.violations(p, key, g, 7, P, 16) == []
    p = aggregate.launch_plan("bwd", g, 7, 64, dtype=gc.DTYPES[key], align=4)
    assert p.kernel_name == "film_bwd_dx_gram"
    assert gc.violations(p, key, g, 7, 64, 4) == []


@pytest.mark.parametrize("n", [1, 5, 8])
def test_small_simple_graphs_plan_the_fused_backward(n):
    g = simple_ns((n, n))
    assert aggregate.launch_plan("bwd", g, 7, 64).kernel_name == "film_bwd_fused"


def test_the_regular_mfma_knob_gates_the_csr_row_form():
    g = simple_ns((12, 12))
    with gc.knobs(bwd_regular_mfma=0):
        assert aggregate.launch_plan("bwd", g, 7, 64).kernel_name == "film_bwd_dx_gram"
    assert aggregate.launch_plan("bwd", g, 7, 64).kernel_name == "film_bwd_mfma"
    with gc.knobs(bwd_half_mfma=0):
        assert aggregate.launch_plan("bwd", g, 7, 64, dtype=torch.bfloat16).kernel_name == "film_bwd_dx_gram"
        assert aggregate.launch_plan("bwd", g, 7, 64).kernel_name == "film_bwd_mfma"


def test_the_cpw_knob_sets_the_channels_per_workgroup():
    g = simple_ns((16, 16))
    for cpw, cpb in ((1, 4), (2, 8)):
        with gc.knobs(bwd_mfma_cpw=cpw):
            p = aggregate.launch_plan("bwd", g, 17, 128)
            assert (p.kernel_name, p.cpb) == ("film_bwd_mfma", cpb)
            assert gc.violations(p, "f32", g, 17, 128, 16) == []


@pytest.mark.parametrize("key", KEYS)
def test_plain_csr_graphs_plan_what_they_planned(key):
    """The same arguments as GRAPH_CSR keep their route: the pinned case, and every backward plan here is the
    one SIMPLE gives wherever the matrix-core kernel does not take over."""
    g = simple_ns((12, 12), kind=_lib.GRAPH_CSR)
    assert aggregate.launch_plan("bwd", g, 7, 64, dtype=gc.DTYPES[key]).kernel_name == "film_bwd_dx_gram"
    for n, P, C in itertools.product((5, 8, 12, 16), (16, 64, 144), (1, 9)):
        c = aggregate.launch_plan("bwd", simple_ns((n, n), kind=_lib.GRAPH_CSR), C, P, dtype=gc.DTYPES[key])
        s = aggregate.launch_plan("bwd", simple_ns((n, n)), C, P, dtype=gc.DTYPES[key])
        assert c.kernel_name in ("film_bwd_fused", "film_bwd_dx_gram")
        if s.kernel_name != "film_bwd_mfma":
            assert gc.plan_tuple(s) == gc.plan_tuple(c), (n, P, C)


@pytest.mark.parametrize("key", KEYS)
def test_the_forward_plan_of_simple_is_the_csr_plan(key):
    for n, P, C, mode in itertools.product((5, 8, 12, 16), (16, 64, 100), (1, 9, 17), ("film_mean", "copy_mean")):
        c = aggregate.launch_plan("fwd", simple_ns((n, n - 1), kind=_lib.GRAPH_CSR), C, P, dtype=gc.DTYPES[key], mode=mode)
        s = aggregate.launch_plan("fwd", simple_ns((n, n - 1)), C, P, dtype=gc.DTYPES[key], mode=mode)
        assert gc.plan_tuple(s) == gc.plan_tuple(c), (n, P, C, mode)


# ------------------------------------------------------------------------------------------------ C ABI
def _plan_code(direction, g, indptr=1 << 20):
    """Return code of a plan query with made-up, aligned pointers (looked at for NULL and alignment only)."""
    lib = m.load_library()
    p = ctypes.c_void_p(1 << 20)
    plan = _lib.AggPlan()
    graph = (p, ctypes.c_void_p(indptr), p, p, p, g.num_graphs, g.max_nodes, g.graph_kind, g.num_nodes, g.num_edges,
             7, 64, 0)
    if direction == "fwd":
        return lib.mrp_film_mean_fwd_plan(0, p, 7 * 64, *graph, p, 7 * 64, None, ctypes.byref(plan))
    return lib.mrp_film_mean_bwd_plan(0, p, 7 * 64, p, 7 * 64, *graph, p, 7 * 64, None, 7 * 64, p, None,
                                      ctypes.byref(plan))


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_kind_3_is_accepted_and_checked_like_csr(direction):
    assert _lib.GRAPH_SIMPLE == 3
    assert _plan_code(direction, simple_ns((12, 10))) == 0
    assert _plan_code(direction, simple_ns((12, 10), extra_rows=5)) == 0  # more gamma/beta rows than edges
    g17 = simple_ns((12, 10))
    g17.max_nodes = 17
    assert _plan_code(direction, g17) == HIP_INVALID_VALUE
    assert _plan_code(direction, simple_ns((12, 10)), indptr=0) == HIP_INVALID_VALUE
    small = simple_ns((12, 12))
    small.max_nodes = 11  # num_graphs * max_nodes < num_nodes
    assert _plan_code(direction, small) == HIP_INVALID_VALUE
    assert _plan_code(direction, simple_ns((12, 10), kind=4)) == HIP_INVALID_VALUE  # still no such kind


def _build_range(B, n, k, max_range, ws=None, nbytes=0):
    lib = m.load_library()
    p = ctypes.c_void_p(1 << 20)
    null = ctypes.c_void_p(0)
    return lib.mrp_frame_graph_build_range(p if B * n else null, null, B, n, k, max_range, null, null, null, null, null,
                                           ws if ws is not None else null, nbytes, null)


def test_range_builder_rejects_bad_arguments_before_any_launch():
    big = ctypes.c_void_p(1 << 20), 1 << 30
    assert _build_range(2, 17, 0, 1.0, *big) == HIP_INVALID_VALUE
    assert _build_range(2, 5, 5, 1.0, *big) == HIP_INVALID_VALUE
    assert _build_range(2, 5, 6, 1.0, *big) == HIP_INVALID_VALUE
    assert _build_range(2, 5, -1, 1.0, *big) == HIP_INVALID_VALUE
    assert _build_range(2, 5, 0, -1.0, *big) == HIP_INVALID_VALUE
    assert _build_range(2, 5, 0, -0.5, *big) == HIP_INVALID_VALUE
    assert _build_range(2, 5, 0, math.nan, *big) == HIP_INVALID_VALUE
    assert _build_range(-1, 5, 0, 1.0, *big) == HIP_INVALID_VALUE
    # a missing or short workspace is an argument error too
    need = m.load_library().mrp_frame_graph_build_range_workspace(2, 5)
    assert _build_range(2, 5, 0, 1.0) == HIP_INVALID_VALUE
    assert _build_range(2, 5, 0, 1.0, ctypes.c_void_p(1 << 20), need - 1) == HIP_INVALID_VALUE


def test_range_builder_succeeds_on_no_graphs():
    assert _build_range(0, 5, 0, 1.0) == 0
    assert _build_range(0, 5, 2, math.inf) == 0
    assert _build_range(3, 0, 0, 0.0) == 0


def test_range_workspace_query_is_positive_and_monotone():
    ws = m.load_library().mrp_frame_graph_build_range_workspace
    assert ws(0, 5) == 0 and ws(5, 0) == 0
    last = 0
    for B, n in ((1, 1), (1, 2), (1, 16), (3, 16), (300, 5), (300, 16), (4096, 16)):
        got = ws(B, n)
        assert got > 0 and got >= last, (B, n)
        assert got >= 2 * 4 * B * n  # a mask and a prefix per robot at least
        last = got


# ------------------------------------------------------------------------------------------------ host builder
def lattice_poses(n, seed=0, coincident=True, nan_robot=None):
    """Robots on the integer lattice around 3-4-5 offsets: robot 1 is exactly 5.0 from robot 0 ((3, 4, 0)),
    robot 2 exactly 5.0 from robot 1 ((3, 4, 0) + (0, 3, 4)); the last robot sits on robot 0 (distance 0)."""
    rng = np.random.RandomState(100 + n + seed)
    t = rng.randint(-6, 7, size=(n, 3)).astype(np.float32)
    t[0] = 0
    if n > 1:
        t[1] = (3, 4, 0)
    if n > 2:
        t[2] = (3, 7, 4)
    if coincident and n > 3:
        t[n - 1] = t[0]
    q = rng.standard_normal((n, 4)).astype(np.float32)
    poses = np.concatenate([t, q], 1)
    if nan_robot is not None and nan_robot < n:
        poses[nan_robot, 1] = np.nan
    return poses


def brute_force_edges(poses, max_range, active, knn):
    """The issue's rule restated with Python loops: the set of (u, v)."""
    n = poses.shape[0]
    rng = math.inf if max_range is None else max_range
    act = [True] * n if active is None else [bool(a) for a in active]
    t = poses[:, :3].astype(np.float64)
    edges = set()
    for v in range(n):
        cand = []
        for u in range(n):
            if u == v or not act[u] or not act[v]:
                continue
            dx, dy, dz = (t[u] - t[v])
            d = math.sqrt((dx * dx + dy * dy) + dz * dz) if not any(map(math.isnan, (dx, dy, dz))) else math.nan
            if d <= rng:  # False for NaN
                cand.append((d, u))
        if knn is not None and len(cand) > knn:
            cand = sorted(cand)[:knn]
        edges.update((u, v) for _, u in cand)
    return edges


def actives(n):
    some = np.ones(n, bool)
    some[::3] = False
    return {"all": None, "some": some, "none": np.zeros(n, bool)}


def masked_edge_set(g):
    s, d = (t.numpy() for t in g.edges())
    mask = g.edge_active.numpy()
    return {(int(u), int(v)) for u, v, a in zip(s, d, mask) if a}


@pytest.mark.parametrize("act", ["all", "some", "none"])
@pytest.mark.parametrize("max_range", [0.0, 5.0, math.inf])
@pytest.mark.parametrize("n", [1, 2, 5, 9, 16])
def test_host_builder_follows_the_rule(n, max_range, act):
    poses = lattice_poses(n)
    active = actives(n)[act]
    for knn in (None, 1, 4):
        if knn is not None and knn >= n:
            with pytest.raises(ValueError):
                m.frame_graph(poses, knn=knn, max_range=max_range, active=active)
            continue
        g = m.frame_graph(poses, knn=knn, max_range=max_range, active=active)
        assert g.num_nodes() == n and g.num_edges() == n * (n - 1)
        want = brute_force_edges(poses, max_range, active, knn)
        assert masked_edge_set(g) == want, (n, max_range, act, knn)
        assert torch.equal(g.in_degrees(), torch.bincount(torch.tensor([v for _, v in want], dtype=torch.int64),
                                                          minlength=n))


def test_pairs_at_exactly_the_range_are_edges_and_coincident_robots_are_neighbours():
    g = m.frame_graph(lattice_poses(5), max_range=5.0)
    edges = masked_edge_set(g)
    assert {(0, 1), (1, 0), (1, 2), (2, 1)} <= edges  # sqrt(25.0) == 5.0 exactly: inclusive
    assert {(0, 4), (4, 0)} <= edges                  # distance 0
    assert masked_edge_set(m.frame_graph(lattice_poses(5), max_range=0.0)) == {(0, 4), (4, 0)}
    below = np.nextafter(5.0, 0.0)
    assert not {(0, 1), (1, 2)} & masked_edge_set(m.frame_graph(lattice_poses(5), max_range=below))


@pytest.mark.parametrize("max_range", [5.0, math.inf])
def test_a_robot_with_a_nan_translation_has_no_edges(max_range):
    poses = lattice_poses(9, nan_robot=3)
    g = m.frame_graph(poses, max_range=max_range)
    edges = masked_edge_set(g)
    assert edges == brute_force_edges(poses, max_range, None, None)
    assert all(3 not in e for e in edges) and len(edges) > 0


def test_bad_range_arguments_raise():
    poses = lattice_poses(5)
    for bad in (-1.0, math.nan):
        with pytest.raises(ValueError):
            m.frame_graph(poses, max_range=bad)
    with pytest.raises(ValueError):
        m.frame_graph(poses, max_range=1.0, active=np.ones(4, bool))


def test_without_the_new_arguments_frame_graph_is_unchanged():
    poses = lattice_poses(6, coincident=False)
    for knn in (None, 3):
        g = m.frame_graph(poses, knn=knn)
        assert g.edge_active is None
        want = _lib.GRAPH_COMPLETE if knn is None else _lib.graph_regular(3)
        assert g.csr("cpu").graph_kind == want
    mixed = m.RobotGraph([0, 0, 2], [1, 1, 0], num_nodes=3)
    assert mixed.csr("cpu").graph_kind == _lib.GRAPH_CSR and mixed.edge_active is None


# ------------------------------------------------------------------------------------------------ RobotGraph
def test_masked_graph_semantics():
    n = 9
    poses = lattice_poses(n)
    active = actives(n)["some"]
    g = m.frame_graph(poses, max_range=7.0, active=active)
    full = m.frame_graph(poses)
    E = n * (n - 1)
    assert g.num_edges() == E and int(g.batch_num_edges()[0]) == E
    assert torch.equal(g.edata["pose"].view(torch.int32), full.edata["pose"].view(torch.int32))
    assert all(torch.equal(a, b) for a, b in zip(g.edges(), full.edges()))
    assert not g.is_complete()
    mask = g.edge_active
    assert mask.dtype == torch.bool and mask.numel() == E and 0 < int(mask.sum()) < E
    assert torch.equal(g.in_degrees(), torch.bincount(g.edges()[1][mask], minlength=n))
    indptr, src, eid, goff, mx = g.host_csr()
    assert mx == n and indptr[-1] == int(mask.sum()) == len(src) == len(eid)
    s, d = (t.numpy() for t in g.edges())
    for v in range(n):
        row = eid[indptr[v]:indptr[v + 1]]
        assert np.all(d[row] == v) and np.all(mask.numpy()[row]) and np.all(np.diff(row) > 0)
        assert np.array_equal(s[row], src[indptr[v]:indptr[v + 1]])
    csr = g.csr("cpu")
    assert csr.graph_kind == _lib.GRAPH_SIMPLE and csr.num_edges == E and csr.num_nodes == n
    assert csr.src.numel() == E and csr.eid.numel() == E  # capacity: every slot
    assert np.array_equal(csr.eid.numpy()[:indptr[-1]], eid)
    as_csr = g.csr("cpu", simple=False)
    assert as_csr.graph_kind == _lib.GRAPH_CSR and as_csr.num_edges == E and as_csr.sparse_eid
    assert as_csr.eid is csr.eid


def test_to_local_scope_and_batch_keep_the_mask():
    a = m.frame_graph(lattice_poses(5), max_range=5.0)
    b = m.frame_graph(lattice_poses(4, seed=1))  # unmasked
    moved = a.to("cpu")
    assert torch.equal(moved.edge_active, a.edge_active) and moved.csr("cpu").graph_kind == _lib.GRAPH_SIMPLE
    with a.local_scope():
        a.edata["tmp"] = torch.zeros(a.num_edges(), 1)
        assert a.csr("cpu").graph_kind == _lib.GRAPH_SIMPLE
    assert "tmp" not in a.edata and a.edge_active is not None
    u = m.batch([a, b, a])
    assert u.num_edges() == 20 + 12 + 20 and u.batch_size == 3
    assert torch.equal(u.edge_active, torch.cat([a.edge_active, torch.ones(12, dtype=torch.bool), a.edge_active]))
    assert u.edata["pose"].shape == (52, 9)
    csr = u.csr("cpu")
    assert csr.graph_kind == _lib.GRAPH_SIMPLE and csr.num_edges == 52 and csr.max_nodes == 5
    assert int(csr.indptr[-1]) == 2 * int(a.edge_active.sum()) + 12
    # an unmasked batch keeps its kind
    assert m.batch([b, b]).edge_active is None and m.batch([b, b]).csr("cpu").graph_kind == _lib.GRAPH_COMPLETE
    # unbatch carries the mask; the disk cache and the sharder name the limitation instead of dropping it
    parts = m.unbatch(u)
    assert torch.equal(parts[0].edge_active, a.edge_active) and bool(parts[1].edge_active.all())
    with pytest.raises(ValueError, match="edge_active"):
        m.save_graphs("/nonexistent/never_written.npz", [a])
    from mrp_gnn_amd import dist
    with pytest.raises(ValueError, match="edge_active"):
        dist.shard_graph(u, 0, 2)
