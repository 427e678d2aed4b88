"""CPU: the index arithmetic the pixel-major compress (``csrc/compress_half_cl.hip``) is designed on, restated
in Python and checked against brute-force enumeration.  Only
``test_workspace_query_agrees_with_the_restated_plan`` calls the built library (the host planner, through the
workspace query); the other cases check the restatement itself — that the scheme the kernels implement is
sound — and do not execute the kernels' code, which ``tests/test_gpu_compress_cl.py`` tests on the GPU:

* the forced split plan of the weight gradient (``plan_splits`` with ``half_cl_splits`` > 0): splits of whole
  32-row stages, the last stage ragged, every pixel row in exactly one split, no split empty — and the
  library's workspace query agrees with the restated split count;
* the planner's own choice (``half_cl_splits`` = 0) through the workspace query: a whole number of
  [C][2C] + [C] fp32 partials, at most one split per stage;
* a weight-gradient thread's row walk: (node, pixel) advanced by (32 // P, 32 % P) with one carry per stage
  equals (r // P, r % P), and the row's element offset ``node * node_stride + pixel * pixel_stride`` stays
  inside its node's P pixel strides;
* the forward / data-gradient tile's pixel rows: clamped loads and masked stores at the last tile."""
import pytest

import mrp_gnn_amd as m

BK, TN = 32, 128


def forced_plan(ktot, forced):
    """compress_half_common.hpp plan_splits, forced > 0: (number of splits, rows per split)."""
    stages = (ktot + BK - 1) // BK
    per = (stages + forced - 1) // forced
    return (stages + per - 1) // per, per * BK


def kernel_split_rows(ktot, nsplit, kchunk):
    """gemm_wg_cl_half: the rows each split's workgroups sum, zero-filled rows of the ragged stage left out."""
    rows = []
    for split in range(nsplit):
        kbeg = split * kchunk
        kend = min(kbeg + kchunk, ktot)
        nst = (kend - kbeg + BK - 1) // BK if kend > kbeg else 0
        mine = []
        for s in range(nst):
            for kr in range(BK):
                r = kbeg + BK * s + kr
                if r < kend:
                    mine.append(r)
        rows.append(mine)
    return rows


@pytest.mark.parametrize("ktot", [1, 3, 31, 32, 33, 49, 245, 4096, 4097, 5 * 49 * 7])
@pytest.mark.parametrize("forced", [1, 2, 3, 5, 64, 256])
def test_forced_split_plan_covers_every_row_once(ktot, forced):
    ns, kchunk = forced_plan(ktot, forced)
    assert 1 <= ns <= forced and kchunk % BK == 0
    rows = kernel_split_rows(ktot, ns, kchunk)
    assert all(rows), "an empty split"
    flat = [r for mine in rows for r in mine]
    assert flat == list(range(ktot))  # each row once, in order


@pytest.mark.parametrize("n,C,P", [(64, 64, 64), (5, 64, 49), (1, 64, 3), (2, 256, 64), (3, 32, 64), (128, 512, 49)])
def test_workspace_query_agrees_with_the_restated_plan(n, C, P):
    lib = m.load_library()
    ws = lib.mrp_compress_bwd_weight_cl_workspace
    part = (C * 2 * C + C) * 4
    try:
        for forced in (1, 2, 3, 7, 256):
            assert lib.mrp_tuning_set(b"half_cl_splits", forced) == 0
            ns, _ = forced_plan(n * P, forced)
            assert ws(n, C, P) == (0 if ns == 1 else ns * part), (forced, ns)
    finally:
        assert lib.mrp_tuning_set(b"half_cl_splits", 0) == 0
    got = ws(n, C, P)  # the planner's choice
    stages = (n * P + BK - 1) // BK
    assert got % part == 0 and got // part <= max(stages, 1) and got // part != 1


@pytest.mark.parametrize("P", [1, 3, 7, 31, 32, 33, 36, 49, 64, 100])
def test_row_walk_matches_division(P):
    """The thread of stage row kr starts at r = kbeg + kr and adds 32 per stage."""
    qs, rs = BK // P, BK % P
    for ps, extra in ((64, 0), (128, 24)):  # dense, and a 2C buffer's half inside a padded batch slice
        ns = P * ps + extra
        for kbeg in (0, 32, 32 * 5):
            for kr in (0, 1, 15, 31):
                r = kbeg + kr
                node, px = divmod(r, P)
                for _stage in range(12):
                    assert (node, px) == divmod(r, P)
                    off = node * ns + px * ps
                    assert node * ns <= off and off + 64 <= node * ns + P * ps  # inside the node's pixel rows
                    r += BK
                    node += qs
                    px += rs
                    if px >= P:
                        px -= P
                        node += 1
                    assert 0 <= px < P


@pytest.mark.parametrize("nodes,P", [(3, 64), (5, 49), (1, 3), (2, 128), (7, 36)])
def test_tile_rows_are_clamped_for_loads_and_masked_for_stores(nodes, P):
    """gemm_cl_half: tile nt's load thread reads row min(128 nt + t // 4, rows - 1); the store lane writes row
    n only if n < rows: over all tiles, every row is stored exactly once, no load leaves the tensor, and the
    row -> (node, pixel) split never crosses a node."""
    rows = nodes * P
    ntiles = (rows + TN - 1) // TN
    stored = []
    for nt in range(ntiles):
        for t in range(512):
            row = min(TN * nt + t // 4, rows - 1)
            node, pix = divmod(row, P)
            assert 0 <= node < nodes and 0 <= pix < P
        for wn in range(2):
            for ni in range(4):
                for r16 in range(16):
                    n = TN * nt + 64 * wn + 16 * ni + r16
                    if n < rows:
                        stored.append(n)
    assert sorted(stored) == list(range(rows))
