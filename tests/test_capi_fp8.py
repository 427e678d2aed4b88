"""CPU: the FP8-message entry points (``mrp_film_mean_fwd_q`` / ``mrp_film_mean_fwd_q_plan``, added to ABI 22
without a new number): exports, every rejection the header lists — all decided on the host before any launch,
so no GPU is needed (a launch attempted here would come back with a no-device error, not with
hipErrorInvalidValue) — the zero-size no-op paths, and the launch plan walked over graph kinds, graph sizes,
channel counts, plane sizes, alignments and output types under the invariants of test_geometry_cpu.py plus the
two that are this path's own: the slice width divides P, and the slice is aligned for both the 1-byte input and
the output type."""
import ctypes
import itertools

import pytest

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib

HIP_INVALID_VALUE = 1
DUMMY = ctypes.c_void_p(1 << 20)  # never dereferenced on the host
QDTYPES = [_lib.QDTYPE_E4M3, _lib.QDTYPE_E5M2]
OUT = {_lib.DTYPE_F32: 4, _lib.DTYPE_BF16: 2, _lib.DTYPE_F16: 2}  # out_dtype -> bytes per element
FULL = dict(kind=1, B=2, maxn=4, Nt=8, E=24, C=2, P=16, gb=DUMMY, xq=DUMMY, xs=32, out=DUMMY, os=32)


def _call(fn, qdtype, out_dtype, tail, **kw):
    a = dict(xq=None, xs=0, scale=None, gb=None, indptr=None, src=None, eid=None, goff=None, B=0, maxn=0, kind=0,
             Nt=0, E=0, C=0, P=0, mode=0, out=None, os=0, ep=None)
    a.update(kw)
    return fn(qdtype, a["xq"], a["xs"], a["scale"], out_dtype, a["gb"], a["indptr"], a["src"], a["eid"], a["goff"],
              a["B"], a["maxn"], a["kind"], a["Nt"], a["E"], a["C"], a["P"], a["mode"], a["out"], a["os"], a["ep"],
              tail)


def _fwd(lib, qdtype, out_dtype, **kw):
    return _call(lib.mrp_film_mean_fwd_q, qdtype, out_dtype, None, **kw)


def _plan(lib, qdtype, out_dtype, **kw):
    plan = _lib.AggPlan()
    return _call(lib.mrp_film_mean_fwd_q_plan, qdtype, out_dtype, ctypes.byref(plan), **kw), plan


def test_symbols_exported_and_abi_unchanged():
    lib = m.load_library()
    for s in ("mrp_film_mean_fwd_q", "mrp_film_mean_fwd_q_plan"):
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert lib.mrp_abi_version() == _lib.ABI_VERSION == 22
    assert (_lib.QDTYPE_E4M3, _lib.QDTYPE_E5M2) == (0, 1)


@pytest.mark.parametrize("out_dtype", list(OUT))
@pytest.mark.parametrize("qdtype", QDTYPES)
def test_rejections_come_before_any_launch(qdtype, out_dtype):
    lib = m.load_library()
    ok = dict(FULL)
    both = lambda **kw: (_fwd(lib, qdtype, out_dtype, **kw), _plan(lib, qdtype, out_dtype, **kw)[0])  # noqa: E731
    for bad_q in (-1, 2):
        assert _fwd(lib, bad_q, out_dtype) == HIP_INVALID_VALUE  # even for an empty batch
        assert _fwd(lib, bad_q, out_dtype, **ok) == HIP_INVALID_VALUE
        assert _plan(lib, bad_q, out_dtype, **ok)[0] == HIP_INVALID_VALUE
    for bad_t in (3, 7, -1):  # the codes every entry point rejects
        assert _fwd(lib, qdtype, bad_t) == HIP_INVALID_VALUE
        assert _fwd(lib, qdtype, bad_t, **ok) == HIP_INVALID_VALUE
        assert _plan(lib, qdtype, bad_t, **ok)[0] == HIP_INVALID_VALUE
    assert both(**dict(ok, xq=None)) == (1, 1)  # a NULL pointer with work to do
    assert both(**dict(ok, out=None)) == (1, 1)
    assert both(**dict(ok, gb=None)) == (1, 1)  # FiLM mode without gamma/beta
    assert both(**dict(ok, xs=31)) == (1, 1)  # node stride < C * P
    assert both(**dict(ok, os=31)) == (1, 1)
    assert both(**dict(ok, maxn=17, Nt=34, E=2 * 17 * 16)) == (1, 1)  # max_nodes > MRP_MAX_NODES
    assert both(**dict(ok, kind=4)) == (1, 1)  # an unknown graph kind
    assert both(**dict(ok, mode=3)) == (1, 1)  # an unknown mode
    assert both(**dict(ok, mode=0x200)) == (1, 1)  # an unknown flag
    assert both(**dict(ok, E=23)) == (1, 1)  # a complete graph with the wrong edge count
    # the own-feature terms cannot come from the codes
    self_ep = _lib.Epilogue(1.0, 1.0, None, 0, 0.0, None, 0)
    assert both(**dict(ok, ep=ctypes.byref(self_ep))) == (1, 1)
    xcopy_ep = _lib.Epilogue(1.0, 0.0, None, 0, 0.0, DUMMY.value, 32)
    assert both(**dict(ok, ep=ctypes.byref(xcopy_ep))) == (1, 1)
    x0_short = _lib.Epilogue(1.0, 0.0, DUMMY.value, 31, 1.0, None, 0)  # x0's node stride < C * P
    assert both(**dict(ok, ep=ctypes.byref(x0_short))) == (1, 1)
    assert _call(lib.mrp_film_mean_fwd_q_plan, qdtype, out_dtype, None, **ok) == HIP_INVALID_VALUE  # NULL plan
    # the valid call plans (the launch itself needs a GPU: test_gpu_fp8_messages.py)
    code, plan = _plan(lib, qdtype, out_dtype, **ok)
    assert code == 0 and plan.kernel_name == "film_fwd"
    x0_ep = _lib.Epilogue(0.75, 0.0, DUMMY.value, 32, 0.25, None, 0)
    assert _plan(lib, qdtype, out_dtype, **dict(ok, ep=ctypes.byref(x0_ep)))[0] == 0
    assert _plan(lib, qdtype, out_dtype, **dict(ok, scale=DUMMY))[0] == 0
    assert _plan(lib, qdtype, out_dtype, **dict(ok, mode=2, gb=None))[0] == 0  # copy_mean needs no gamma/beta


@pytest.mark.parametrize("out_dtype", list(OUT))
@pytest.mark.parametrize("qdtype", QDTYPES)
def test_zero_sizes_are_noops(qdtype, out_dtype):
    lib = m.load_library()
    assert _fwd(lib, qdtype, out_dtype) == 0  # empty batch
    for kw in (dict(kind=1, B=2, maxn=4, Nt=8, E=24, C=0, P=16), dict(kind=1, B=2, maxn=4, Nt=8, E=24, C=2, P=0),
               dict(kind=1, B=0, maxn=4, Nt=0, E=0, C=2, P=16)):
        assert _fwd(lib, qdtype, out_dtype, **kw) == 0
        code, plan = _plan(lib, qdtype, out_dtype, **kw)
        assert code == 0 and plan.kernel_name == "none"


def test_other_entry_points_still_reject_the_new_codes():
    """Nothing existing changed: dtype codes 3 and 7 and max_nodes = 17 are rejected as before."""
    lib = m.load_library()
    plan = _lib.AggPlan()
    graph = (DUMMY, None, None, None, None, 2, 4, 1, 8, 24, 2, 16, 0)
    for bad in (3, 7):
        assert lib.mrp_film_mean_fwd_t(bad, DUMMY, 32, *graph, DUMMY, 32, None, None) == HIP_INVALID_VALUE
        assert lib.mrp_film_mean_fwd_plan(bad, DUMMY, 32, *graph, DUMMY, 32, None, ctypes.byref(plan)) == \
            HIP_INVALID_VALUE
    g17 = (DUMMY, None, None, None, None, 2, 17, 1, 34, 2 * 17 * 16, 2, 16, 0)
    for dt in (0, 1, 2):
        assert lib.mrp_film_mean_fwd_t(dt, DUMMY, 32, *g17, DUMMY, 32, None, None) == HIP_INVALID_VALUE


# ---- the plan walk --------------------------------------------------------------------------------------------
KINDS = ("complete", "csr", "simple", "knn4")
NODES = (1, 2, 8, 9, 12, 16)
CHANNELS = (1, 3, 17, 64)
PLANES = (1, 9, 36, 64, 1024)
ALIGNS = (16, 8, 4, 1)  # bytes, of the codes; out is aligned to the same number of its own elements


def _graph_kw(kind, n):
    B = 2
    if kind == "complete":
        return dict(kind=_lib.GRAPH_COMPLETE, B=B, maxn=n, Nt=B * n, E=B * n * (n - 1))
    if kind == "knn4":
        return dict(kind=_lib.graph_regular(4), B=B, maxn=n, Nt=B * n, E=4 * B * n, indptr=DUMMY, src=DUMMY,
                    eid=DUMMY, goff=DUMMY)
    return dict(kind=_lib.GRAPH_CSR if kind == "csr" else _lib.GRAPH_SIMPLE, B=B, maxn=n, Nt=B * n, E=3 * B * n,
                indptr=DUMMY, src=DUMMY, eid=DUMMY, goff=DUMMY)


def _expected_vec(n, P, align, elem):
    """The header's rule: the widest of 8 (<= 8 nodes, 16-bit outputs) / 4 / 1 elements for which the codes
    (1-byte elements) and out (elem bytes) are both aligned and P is a multiple of it."""
    for v in (8, 4):
        if v == 8 and (n > 8 or elem != 2):
            continue
        if P % v == 0 and align % v == 0 and (align * elem) % (v * elem) == 0:
            return v
    return 1


@pytest.mark.parametrize("out_dtype", list(OUT))
@pytest.mark.parametrize("kind", KINDS)
def test_plan_invariants(kind, out_dtype):
    lib = m.load_library()
    elem = OUT[out_dtype]
    base = DUMMY.value
    seen = set()
    for n, C, P, align, qdtype in itertools.product(NODES, CHANNELS, PLANES, ALIGNS, QDTYPES):
        xp = base + (align if align % 16 else 0)
        op = base + (align * elem if align % 16 else 0)
        kw = dict(_graph_kw(kind, n), C=C, P=P, gb=DUMMY, xq=ctypes.c_void_p(xp), xs=C * P,
                  out=ctypes.c_void_p(op), os=C * P, scale=DUMMY)
        code, plan = _plan(lib, qdtype, out_dtype, **kw)
        what = (kind, n, C, P, align, out_dtype, qdtype)
        assert code == 0, what
        assert plan.kernel_name == ("film_fwd_regular" if kind == "knn4" else "film_fwd"), what
        v = plan.vec
        assert v == _expected_vec(n, P, align, elem), what
        assert P % v == 0, what  # the slice width divides P ...
        assert xp % v == 0 and op % (v * elem) == 0 and (C * P) % v == 0, what  # ... aligned for input and output
        assert plan.lpc >= 1 and plan.lpc & (plan.lpc - 1) == 0 and plan.lpc <= max(P // v, 1), what
        assert plan.threads == plan.cpb * plan.lpc <= 256, what
        assert plan.cpb >= 1 and plan.ncb * plan.cpb >= C > (plan.ncb - 1) * plan.cpb, what  # every channel, once
        assert 0 < plan.lds_bytes <= 64 * 1024, what
        assert plan.psplit >= 1 and plan.grid == 2 * plan.ncb * plan.psplit, what
        assert plan.psplit * plan.lpc * v >= P or plan.psplit == 1, what  # a split plane: one slice per lane
        seen.add(v)
    assert seen == ({8, 4, 1} if elem == 2 else {4, 1})


def test_plan_checks_the_epilogue_tensor_too():
    """x0 (in the output type) takes part in the alignment rule: a misaligned x0 narrows the slice."""
    lib = m.load_library()
    kw = dict(_graph_kw("complete", 4), C=4, P=64, gb=DUMMY, xq=DUMMY, xs=256, out=DUMMY, os=256)
    assert _plan(lib, 0, _lib.DTYPE_BF16, **kw)[1].vec == 8
    for off, vec in ((8, 4), (2, 1)):
        ep = _lib.Epilogue(1.0, 0.0, DUMMY.value + off, 256, 1.0, None, 0)
        assert _plan(lib, 0, _lib.DTYPE_BF16, **dict(kw, ep=ctypes.byref(ep)))[1].vec == vec
    ep = _lib.Epilogue(1.0, 0.0, DUMMY.value, 260, 1.0, None, 0)  # x0's node stride: a multiple of 4, not of 8
    assert _plan(lib, 0, _lib.DTYPE_BF16, **dict(kw, ep=ctypes.byref(ep)))[1].vec == 4
