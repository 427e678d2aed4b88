"""The multi-head attention entry points' C ABI without a GPU launch: exports and signatures, validation before any
launch (the single-head entry points' rejections, plus the head count's), empty work, the workspace queries."""
import ctypes
import itertools
import os
import re

import pytest

import mrp_gnn_amd as m
from mrp_gnn_amd import _lib
from conftest import ROOT

HIP_INVALID_VALUE = 1
DUMMY = ctypes.c_void_p(16)
NAMES = ("mrp_film_attn_fwd_mh", "mrp_film_attn_bwd_mh", "mrp_film_attn_workspace_mh", "mrp_film_wattn_fwd_mh",
         "mrp_film_wattn_bwd_mh", "mrp_film_wattn_workspace_mh")
I32, I64, PTR, F32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float
C_TYPES = {"int32_t": I32, "int64_t": I64, "float": F32}


def _call(lib, gated, bwd, **kw):
    """One of the four _mh entry points by keyword, everything absent 0 / NULL, heads 1, scale 1."""
    a = dict(dtype=0, g=None, gs=0, x=None, xs=0, gb=None, w=None, ws=0, indptr=None, src=None, eid=None, goff=None,
             B=0, maxn=0, kind=0, Nt=0, E=0, C=0, P=0, flags=0, heads=1, out=None, os=0, dx=None, dxs=0, base=None,
             bs=0, dgb=None, scale=1.0, attn=None, rate=None, dw=None, dws=0, work=None, wbytes=0, stream=None)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    args = [a["dtype"]] + ([a["g"], a["gs"]] if bwd else []) + [a["x"], a["xs"], a["gb"]]
    args += [a["w"], a["ws"]] if gated else []
    args += [a[k] for k in ("indptr", "src", "eid", "goff", "B", "maxn", "kind", "Nt", "E", "C", "P", "flags", "heads")]
    args += [a["dx"], a["dxs"], a["base"], a["bs"], a["dgb"]] if bwd else [a["out"], a["os"]]
    args += [a["scale"], a["attn"]]
    if gated:
        args += [a["rate"], a["dw"], a["dws"]] if bwd else [a["rate"]]
    args += [a["work"], a["wbytes"], a["stream"]]
    fn = getattr(lib, "mrp_film_%s_%s_mh" % ("wattn" if gated else "attn", "bwd" if bwd else "fwd"))
    assert len(args) == len(fn.argtypes)
    return fn(*args)


def _header_params(text, name):
    body = re.search(r"^(?:int|int64_t)\s+%s\s*\(([^;]*?)\)\s*;" % name, text, re.S | re.M).group(1)
    out = []
    for p in body.split(","):
        p = " ".join(p.split())
        typ, ident = p.rsplit(" ", 1) if "*" not in p else (p[: p.rindex("*") + 1], p[p.rindex("*") + 1:].strip())
        out.append((typ.strip(), ident))
    return out


def test_the_six_symbols_exist_with_the_headers_signatures_and_the_abi_is_22():
    text = open(os.path.join(ROOT, "include", "mrp_gnn.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t|const char\*|void)\s+(mrp_\w+)\s*\(", text, re.M))
    assert set(NAMES) <= declared
    assert declared == set(_lib.EXPORTED_SYMBOLS)  # header and exports stay equal
    lib = m.load_library()
    assert lib.mrp_abi_version() == 22 == _lib.ABI_VERSION
    for name in NAMES:
        fn = getattr(lib, name)
        single = _header_params(text, name[:-3])
        multi = _header_params(text, name)
        # the single-head signature with `int32_t heads` after `C, P, flags` (`C, P` in the workspace queries)
        after = "P" if name.endswith("workspace_mh") else "flags"
        at = [ident for _, ident in single].index(after) + 1
        assert multi == single[:at] + [("int32_t", "heads")] + single[at:], name
        # and the bindings declare what the header declares
        want = [PTR if "*" in typ else C_TYPES[typ] for typ, _ in multi]
        assert list(fn.argtypes) == want, name
        assert fn.restype == (ctypes.c_int64 if name.endswith("workspace_mh") else ctypes.c_int)
        assert list(getattr(lib, name[:-3]).argtypes) == want[:at] + want[at + 1:]


@pytest.mark.parametrize("gated", [False, True], ids=["attn", "wattn"])
@pytest.mark.parametrize("heads", [1, 2])
def test_forward_declines_what_the_single_head_forward_declines(gated, heads):
    lib = m.load_library()

    def fwd(**kw):
        return _call(lib, gated, False, heads=heads, **kw)
    ok = dict(B=1, maxn=2, Nt=2, goff=DUMMY, indptr=DUMMY, C=2, P=4, x=DUMMY, out=DUMMY, xs=8, os=8, w=DUMMY, ws=4)
    assert fwd() == 0  # empty batch: no-op
    assert fwd(kind=1, B=2, maxn=4, Nt=8, E=24, C=0, P=16) == 0  # consistent, empty features: no-op
    assert fwd(**dict(ok, P=0, xs=0, os=0, ws=0)) == 0
    assert fwd(maxn=17, B=1, Nt=1, goff=DUMMY, indptr=DUMMY) == HIP_INVALID_VALUE  # > MRP_MAX_NODES
    for bad in (dict(dtype=3), dict(dtype=-1), dict(kind=2), dict(kind=7), dict(flags=1), dict(flags=3),
                dict(flags=0x101), dict(C=-1), dict(P=-1), dict(B=-1), dict(Nt=-1), dict(E=-1), dict(maxn=-1),
                dict(scale=float("nan")), dict(scale=float("inf")), dict(scale=float("-inf")), dict(wbytes=-1)):
        assert fwd(**bad) == HIP_INVALID_VALUE, bad
    assert fwd(**dict(ok, xs=7)) == HIP_INVALID_VALUE  # node stride < C * P
    assert fwd(**dict(ok, os=7)) == HIP_INVALID_VALUE
    for null in ("x", "out", "goff", "indptr"):
        assert fwd(**dict(ok, **{null: None})) == HIP_INVALID_VALUE, null  # NULL pointers with work to do
    if gated:
        assert fwd(**dict(ok, w=None)) == HIP_INVALID_VALUE
        assert fwd(**dict(ok, ws=3)) == HIP_INVALID_VALUE  # w_node_stride < P
    edges = dict(ok, E=2, src=DUMMY, eid=DUMMY, gb=DUMMY, attn=DUMMY)
    for null in ("gb", "attn", "src"):
        assert fwd(**dict(edges, **{null: None})) == HIP_INVALID_VALUE, null
    assert fwd(**dict(ok, Nt=3)) == HIP_INVALID_VALUE  # more nodes than num_graphs * max_nodes
    assert fwd(kind=1, B=2, maxn=4, Nt=8, E=23) == HIP_INVALID_VALUE  # COMPLETE with inconsistent counts
    assert fwd(kind=1, B=2, maxn=4, Nt=7, E=24) == HIP_INVALID_VALUE
    assert fwd(kind=_lib.graph_regular(2), B=1, maxn=4, Nt=4, E=7, goff=DUMMY, indptr=DUMMY) == HIP_INVALID_VALUE
    assert fwd(kind=_lib.graph_regular(17), B=1, maxn=16, Nt=16, E=17 * 16, goff=DUMMY, indptr=DUMMY, src=DUMMY,
               eid=DUMMY) == HIP_INVALID_VALUE


@pytest.mark.parametrize("gated", [False, True], ids=["attn", "wattn"])
@pytest.mark.parametrize("heads", [1, 2])
def test_backward_declines_what_the_single_head_backward_declines(gated, heads):
    lib = m.load_library()

    def bwd(**kw):
        return _call(lib, gated, True, heads=heads, **kw)
    ok = dict(B=1, maxn=2, Nt=2, goff=DUMMY, indptr=DUMMY, C=2, P=4, g=DUMMY, gs=8, x=DUMMY, xs=8, dx=DUMMY, dxs=8,
              w=DUMMY, ws=4)
    assert bwd() == 0  # nothing requested
    assert bwd(**dict(ok, dx=None)) == 0  # work, but no output wanted
    assert bwd(dx=DUMMY, dgb=DUMMY) == 0  # empty work
    assert bwd(kind=1, B=2, maxn=4, Nt=8, E=24, C=0, P=16, dx=DUMMY) == 0
    assert bwd(maxn=17, B=1, Nt=1, goff=DUMMY, indptr=DUMMY, dx=DUMMY) == HIP_INVALID_VALUE
    for bad in (dict(dtype=3), dict(kind=2), dict(flags=2), dict(flags=0x102), dict(C=-1), dict(P=-1), dict(B=-1),
                dict(Nt=-1), dict(E=-1), dict(scale=float("nan")), dict(scale=float("inf")), dict(wbytes=-1)):
        assert bwd(dx=DUMMY, **bad) == HIP_INVALID_VALUE, bad
    for key in ("gs", "xs", "dxs"):
        assert bwd(**dict(ok, **{key: 7})) == HIP_INVALID_VALUE, key  # node stride < C * P
    assert bwd(**dict(ok, base=DUMMY, bs=7)) == HIP_INVALID_VALUE
    assert bwd(**dict(ok, g=None)) == HIP_INVALID_VALUE  # NULL pointers with work to do
    assert bwd(**dict(ok, x=None)) == HIP_INVALID_VALUE
    edges = dict(ok, E=2, src=DUMMY, eid=DUMMY, gb=DUMMY, attn=DUMMY)
    assert bwd(**dict(edges, gb=None)) == HIP_INVALID_VALUE
    assert bwd(**dict(edges, attn=None)) == HIP_INVALID_VALUE
    if gated:
        assert bwd(**dict(ok, w=None)) == HIP_INVALID_VALUE
        assert bwd(**dict(ok, ws=3)) == HIP_INVALID_VALUE
        assert bwd(**dict(ok, dw=DUMMY, dws=3)) == HIP_INVALID_VALUE  # gw_node_stride < P
        assert bwd(**dict(edges, dw=DUMMY, dws=4, rate=None, work=DUMMY, wbytes=1 << 20)) == HIP_INVALID_VALUE
    assert bwd(kind=1, B=2, maxn=4, Nt=8, E=23, dx=DUMMY) == HIP_INVALID_VALUE
    assert bwd(kind=1, B=2, maxn=4, Nt=7, E=24, dx=DUMMY) == HIP_INVALID_VALUE
    assert bwd(kind=_lib.graph_regular(17), B=1, maxn=16, Nt=16, E=17 * 16, goff=DUMMY, indptr=DUMMY, src=DUMMY,
               eid=DUMMY, dx=DUMMY) == HIP_INVALID_VALUE
    # grad_gb of a plane that spans several tiles needs the queried workspace
    big = dict(kind=1, B=1, maxn=2, Nt=2, E=2, C=2, P=256, g=DUMMY, gs=512, x=DUMMY, xs=512, gb=DUMMY, attn=DUMMY,
               dgb=DUMMY, w=DUMMY, ws=256)
    q = lib.mrp_film_wattn_workspace_mh if gated else lib.mrp_film_attn_workspace_mh
    need = q(1, 1, 2, 1, 2, 2, 2, 256, 1)
    assert need > 0
    assert bwd(**big) == HIP_INVALID_VALUE  # no workspace
    assert bwd(**dict(big, work=DUMMY, wbytes=need - 1)) == HIP_INVALID_VALUE  # smaller than the query
    assert bwd(**dict(big, work=None, wbytes=need)) == HIP_INVALID_VALUE
    if gated and heads > 1:
        # grad_w of several heads needs its partials too, and only where grad_w is wanted
        one = dict(big, P=64, gs=128, xs=128, ws=64, dgb=None, rate=DUMMY, dw=DUMMY, dws=64)
        part = heads * 2 * 64 * 4
        assert q(1, 1, 2, 1, 2, 2, 2, 64, heads) == part
        assert bwd(**one) == HIP_INVALID_VALUE
        assert bwd(**dict(one, work=DUMMY, wbytes=part - 1)) == HIP_INVALID_VALUE
        assert bwd(**dict(one, work=None, wbytes=part)) == HIP_INVALID_VALUE


@pytest.mark.parametrize("gated", [False, True], ids=["attn", "wattn"])
@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
def test_the_head_count_is_validated_before_any_launch(gated, bwd):
    lib = m.load_library()
    ok = dict(B=1, maxn=2, Nt=2, goff=DUMMY, indptr=DUMMY, C=6, P=4, x=DUMMY, xs=24, w=DUMMY, ws=4, kind=0)
    ok.update(dict(g=DUMMY, gs=24, dx=DUMMY, dxs=24) if bwd else dict(out=DUMMY, os=24))
    for heads in (0, -1, -(2 ** 31)):
        assert _call(lib, gated, bwd, heads=heads, **ok) == HIP_INVALID_VALUE, heads
        assert _call(lib, gated, bwd, heads=heads, dx=DUMMY if bwd else None) == HIP_INVALID_VALUE  # empty work too
    for heads in (4, 5, 7, 12):
        assert _call(lib, gated, bwd, heads=heads, **ok) == HIP_INVALID_VALUE, heads  # C % heads != 0
    # C == 0 divides by anything: empty work, success
    for heads in (1, 2, 7):
        assert _call(lib, gated, bwd, heads=heads, kind=1, B=2, maxn=4, Nt=8, E=24, C=0, P=16,
                     dx=DUMMY if bwd else None) == 0


def test_empty_work_returns_success():
    lib = m.load_library()
    for gated, bwd, heads in itertools.product((False, True), (False, True), (1, 2, 3)):
        out = dict(dx=DUMMY, dgb=DUMMY) if bwd else {}
        assert _call(lib, gated, bwd, heads=heads, **out) == 0
        assert _call(lib, gated, bwd, heads=heads, kind=1, B=2, maxn=4, Nt=8, E=24, C=0, P=0, **out) == 0
        assert _call(lib, gated, bwd, heads=heads, C=6, P=4, **out) == 0  # no graphs


SIZES = [(kind, nodes, C, P) for kind in (_lib.GRAPH_CSR, _lib.GRAPH_COMPLETE, _lib.GRAPH_SIMPLE, _lib.graph_regular(4))
         for nodes in (0, 8, 16) for C in (0, 1, 12, 64) for P in (0, 16, 64, 65, 80, 1024)]


def test_workspace_queries():
    lib = m.load_library()
    for kind, nodes, C, P in SIZES:
        B = 2
        per = nodes // B
        E = B * per * (per - 1) if kind == _lib.GRAPH_COMPLETE else (4 * nodes if kind == _lib.graph_regular(4) else
                                                                     3 * nodes)
        E = max(E, 0)
        for direction in (0, 1):
            sizes = (direction, B, per, kind, nodes, E, C, P)
            old_a, old_w = lib.mrp_film_attn_workspace(*sizes), lib.mrp_film_wattn_workspace(*sizes)
            # heads = 1: the old queries' values
            assert lib.mrp_film_attn_workspace_mh(*sizes, 1) == old_a, sizes
            assert lib.mrp_film_wattn_workspace_mh(*sizes, 1) == old_w, sizes
            for heads in (2, 3, 4, 12):
                # film_attn: the tile partials hold every head's columns
                assert lib.mrp_film_attn_workspace_mh(*sizes, heads) == old_a, (sizes, heads)
                # film_wattn backward: exactly the heads' grad_w partials more; the forward needs none
                grow = heads * nodes * P * 4 if direction else 0
                assert lib.mrp_film_wattn_workspace_mh(*sizes, heads) == old_w + grow, (sizes, heads)
    assert lib.mrp_film_wattn_workspace_mh(1, 2, 8, 1, 16, 112, 64, 1024, 4) == \
        16 * 112 * 64 * 2 * 4 + 4 * 16 * 1024 * 4
