"""Test infrastructure for special values (``test_gpu_special_values.py``, ``test_special_values_cpu.py``):
zeros, subnormals, infinities, NaNs and overflow — the inputs that ``randn`` never draws — and the reference
evaluation of what the kernels must make of them.  No GPU code here.

* **the mean's division** (:func:`division_case`): complete batches ``[n, n]`` with gamma = 1, beta = 0, so
  a destination's sum is the fp32 sum of its sources, and chosen (channel, pixel) slots whose sums are +0,
  a subnormal, a value below 2^-124 on which ``div_fast<D>`` differs from ``x / D`` (:func:`tiny_mismatches`),
  +-inf and NaN (from +inf and -inf as two sources) — each in a destination of the first group of four,
  the middle and the last (short, when n % 4 != 0) group, each at its own pixel of a 16-byte slice;
* **the sigmoid at saturation** (:data:`LOGITS`, :func:`sigmoid_bound`);
* **the store to bf16 / fp16** (:func:`store_table`): fp32 targets at overflow, ties, T's subnormal range,
  NaN, +-inf and -0, each the exact fp32 value of ``gamma (a + b)`` with a, b values of T and gamma a power
  of two;
* **poison** (:data:`POISON`, :func:`assert_confined`): one non-finite element; everything the reference
  keeps finite must have the clean run's bits, everything it makes non-finite must be non-finite;
* **scale equivariance of the split-bf16 products** (:func:`scale_case`, :data:`SCALE_PAIRS`).

Comparisons use bits where the reference is finite (the sign of zero included) and "is NaN" where it is NaN.
"""
import functools

import numpy as np
import torch

import half_cases as hc
import oracle
import span_cases as sp
import split_cases as sc

DTYPES = sp.DTYPES  # "f32" / "bf16" / "f16"
bits = sp.bits


def from_bits(pattern):
    """The fp32 scalar tensor with this bit pattern."""
    signed = pattern - (1 << 32) if pattern >= 1 << 31 else pattern
    return torch.tensor([signed], dtype=torch.int32).view(torch.float32)[0]


NEG_NAN = from_bits(0xFFC00000)  # a quiet NaN with its sign bit set
FULL_NAN = from_bits(0x7FFFFFFF)  # a NaN whose payload is all ones (a guard-less bf16 rounding carries out of it)
#: the poisons of the confinement tests
POISON = {"inf": torch.tensor(float("inf")), "nan": torch.tensor(float("nan")), "neg_nan": NEG_NAN}


def assert_same(got, want, what):
    """Bits where ``want`` is not NaN (sign of zero and infinities included), is-NaN where it is."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), \
        f"{what}: NaN at {int((torch.isnan(got) != nan).sum())} wrong places, first {_first(torch.isnan(got) != nan)}"
    bad = (bits(got) != bits(want)) & ~nan
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at " \
        f"{_first(bad)}: got {got[_first(bad)].item()!r}, want {want[_first(bad)].item()!r}"


def _first(mask):
    return tuple(int(i) for i in mask.nonzero()[0]) if bool(mask.any()) else None


def assert_confined(got, clean, ref_poisoned, what, allowed=None):
    """``got``: a kernel's output on poisoned input, ``clean``: the same kernel's on the clean input,
    ``ref_poisoned``: the reference's on the poisoned input.  Everything the reference makes non-finite is
    non-finite in ``got``; every element outside ``allowed`` (a bool mask; default: the reference's non-finite
    set, i.e. the strict form) has the clean run's bits and is finite."""
    got, clean, ref = got.detach().cpu(), clean.detach().cpu(), ref_poisoned.detach().cpu()
    must = ~torch.isfinite(ref.float())
    allowed = must if allowed is None else allowed.cpu()
    assert bool(must.any()), f"{what}: the reference stays finite — the poison tests nothing"
    assert not bool((must & ~allowed).any()), f"{what}: the allowed set does not cover the reference's"
    bad = ~torch.isfinite(got.float())
    assert not bool((must & ~bad).any()), \
        f"{what}: {int((must & ~bad).sum())} elements the reference makes non-finite are finite, first {_first(must & ~bad)}"
    leak = ~allowed & (bits(got) != bits(clean))
    assert not bool(leak.any()), \
        f"{what}: {int(leak.sum())} elements outside the allowed set changed, first {_first(leak)}: " \
        f"{got[_first(leak)].item()!r} for {clean[_first(leak)].item()!r}"
    assert bool(torch.isfinite(clean.float()).all()), f"{what}: the clean run is not finite"


# ---- 1. the mean's division ---------------------------------------------------------------------------------

def div_fast(x, D):
    """``fast_math.hpp``'s ``div_fast<D>`` on a float32 numpy array, without its gate: q0 = fl(x RN(1/D)),
    r = fl(fma(-q0, D, x)), q = fl(fma(r, RN(1/D), q0)).  Both fmas are evaluated in float64, which is exact
    for the magnitudes used here (every term a multiple of 2^-176 below 2^-100, or |x| < 2^20)."""
    x = np.asarray(x, np.float32)
    y = float(np.float32(1) / np.float32(D))
    with np.errstate(all="ignore"):
        x64 = x.astype(np.float64)
        q0 = (x64 * y).astype(np.float32).astype(np.float64)
        r = (x64 - q0 * D).astype(np.float32).astype(np.float64)
        return (r * y + q0).astype(np.float32)


#: the divisors 2..15 for which div_fast<D> has wrong quotients in (0, 2^-124); for the others it is wrong only
#: at +-0 (the sign) and +-inf (an exhaustive run over the 3 x 2^23 patterns below 2^-124 found none)
TINY_DIVISORS = (6, 10, 12, 14)


@functools.lru_cache(maxsize=None)
def tiny_mismatches(D, count=3):
    """Up to ``count`` fp32 values in (0, 2^-124) with div_fast<D>(x) != x / D: a search over the bit patterns
    1 .. 2^14 and 2^16 patterns spread up to 2^-124."""
    pat = np.concatenate([np.arange(1, 1 << 14), np.linspace(1 << 14, (3 << 23) - 1, 1 << 16).astype(np.int64)])
    x = pat.astype(np.uint32).view(np.float32)
    bad = x[div_fast(x, D) != x / np.float32(D)]
    return tuple(float(v) for v in (bad[0], bad[len(bad) // 2], bad[-1])[:count]) if len(bad) else ()


DIV_KINDS = ("zero", "subnormal", "tiny", "pinf", "ninf", "nan")
DIV_C, DIV_H, DIV_W = 8, 4, 4


def div_placements(n):
    """Destinations (local) that get a special sum: in the first group of four, in the middle, and the last
    node — the short last group when n % 4 != 0."""
    return sorted({min(1, n - 1), n // 2, n - 1})


@functools.lru_cache(maxsize=None)
def division_case(n, key):
    """A complete batch [n, n] at C = 8, 4 x 4: dict of the graph, x (2n, C, 4, 4) in T, gb (E, C, 2) with
    gamma = 1 and beta = 0, and ``slots``: (kind, global destination, channel, pixel) of every special sum."""
    T = DTYPES[key]
    g = hc._frames([n, n], 100 + n)
    C, H, W = DIV_C, DIV_H, DIV_W
    P = H * W
    gen = torch.Generator().manual_seed(n * 31 + list(DTYPES).index(key))
    x = torch.randn(2 * n, C, P, generator=gen).to(T)
    tiny = tiny_mismatches(n - 1) if n - 1 in TINY_DIVISORS and key == "f32" else ()
    value = {"zero": 0.0, "subnormal": 2.0 ** -133 if key != "f16" else None,  # 2^-133: bf16's smallest
             "tiny": tiny[len(tiny) // 2] if tiny else None}
    slots, s = [], 0
    for gi in range(2):
        base = gi * n
        for v in div_placements(n):
            for kind in DIV_KINDS:
                if kind in value and value[kind] is None:
                    continue
                flat = (s * 37) % (C * P)  # 37 is coprime with 128: every slot its own (channel, pixel)
                c, p = flat // P, flat % P
                s += 1
                u0 = (v + 1) % n
                if kind in value:  # every source of v zero but one
                    for u in range(n):
                        if u != v:
                            x[base + u, c, p] = 0.0
                    x[base + u0, c, p] = value[kind]
                    slots.append((kind, base + v, c, p))
                elif kind in ("pinf", "ninf"):  # source v: every destination but v itself sees it
                    x[base + v, c, p] = float("inf") if kind == "pinf" else float("-inf")
                    slots.append((kind, base + u0, c, p))
                elif n > 2:  # +inf and -inf as two sources: NaN in every other destination
                    x[base + v, c, p] = float("inf")
                    x[base + u0, c, p] = float("-inf")
                    slots.append((kind, base + (v + 2) % n, c, p))
    assert s <= C * P
    gb = torch.zeros(g.num_edges(), C, 2)
    gb[:, :, 0] = 1.0
    x = x.view(2 * n, C, H, W)
    assert torch.equal(x.float().to(T), x) or bool(torch.isnan(x.float()).any())
    return dict(graph=g, x=x, gb=gb, slots=slots, n=n)


@functools.lru_cache(maxsize=None)
def special_sums_case(name, key):
    """A ``half_cases`` case (e: REGULAR(4), g: CSR with mixed in-degrees) with gamma = 1, beta = 0 and, for a few
    destinations with in-edges, sums that are +0, subnormal, +inf, -inf and NaN, each at its own (channel, pixel)."""
    T = DTYPES[key]
    g = hc.graph(name)
    n, C, H, W = hc.shape(name)
    P = H * W
    src, dst = (t.numpy() for t in g.edges())
    x = hc.host_inputs(name, key if key != "f32" else "bf16")[0].to(T).reshape(n, C, P).clone()
    kinds = [("zero", 0.0), ("pinf", float("inf")), ("ninf", float("-inf")), ("nan", None)] + ([("subnormal", 2.0 ** -133)] if key != "f16" else [])
    fed = sorted(set(dst.tolist()))
    s = 0
    for v in (fed[0], fed[len(fed) // 2], fed[-1]):
        sources = sorted(set(src[dst == v].tolist()))
        for kind, value in kinds:
            flat = (s * 37) % (C * P)
            c, p = flat // P, flat % P
            s += 1
            for u in sources:
                x[u, c, p] = 0.0
            if kind == "nan" and len(sources) > 1:
                x[sources[0], c, p], x[sources[1], c, p] = float("inf"), float("-inf")
            elif kind != "nan":
                x[sources[0], c, p] = value
    gb = torch.zeros(len(src), C, 2)
    gb[:, :, 0] = 1.0
    return dict(graph=g, x=x.view(n, C, H, W), gb=gb)


def aggregate_ref(g, x, gb, mode="film_mean", self_scale=0.0):
    """The fp32 oracle on the widened x (+ ``self_scale`` x, the residual epilogue), in fp32."""
    src, dst = (t.numpy() for t in g.edges())
    with np.errstate(all="ignore"):
        out = oracle.film_aggregate(x.float(), gb.float(), src, dst, mode)
    return out + self_scale * x.float() if self_scale != 0.0 else out


def division_sums(c):
    """The fp32 sums the kernel divides: the oracle in ``film_sum``."""
    return aggregate_ref(c["graph"], c["x"], c["gb"], "film_sum")


# ---- 2. the sigmoid at saturation -----------------------------------------------------------------------------

LOGITS = tuple(s * v for v in (0.0, 1e-30, 20.0, 80.0, 87.5, 89.0, 104.0, 1e4, 3e38, float("inf")) for s in (1.0, -1.0))
#: from here on sigma is exactly 1 in fp32: e^-z <= 2^-24 e^-20 = 1.2e-16, far below half an ulp of 1 (2^-25)
ONE_FROM = 20.0 + 24.0 * np.log(2.0)


def sigmoid64(z):
    with np.errstate(all="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


def sigmoid_bound(z):
    """|sigma - sigma64| <= (2.5 2^-23 + 2^-24 |z|) sigma64 + 2^-126: the exp2 and rcp one-ulp errors, the add's
    half ulp, the rounding of z log2 e and of the constant; plus one flushed subnormal."""
    z = np.asarray(z, np.float64)
    with np.errstate(all="ignore"):
        rel = np.where(np.isfinite(z), 2.5 * 2.0 ** -23 + 2.0 ** -24 * np.abs(z), 0.0)
    return rel * sigmoid64(z) + 2.0 ** -126


def dsigmoid64(z):
    s = sigmoid64(z)
    return s * (1.0 - s)


# ---- 3. the store to bf16 / fp16 --------------------------------------------------------------------------------

#: per type: (a, b, log2 gamma) — the fp32 target is gamma (a + b), exact; a and b are values of T
_STORE = {
    "f16": [
        (65504.0, 15.984375, 0),        # 65519.984375 -> 65504
        (65504.0, 16.0, 0),             # 65520, the overflow tie -> inf
        (65504.0, 65504.0, 0),          # far past it -> inf
        (-65504.0, -16.0, 0),           # -> -inf
        (2.0 ** -24, 0.0, 0),           # the smallest subnormal, kept
        (2.0 ** -24, 2.0 ** -24, -2),   # 2^-25, the tie -> 0
        (-2.0 ** -24, -2.0 ** -24, -2),  # -2^-25 -> -0
        (2.0 ** -23, 2.0 ** -24, -2),   # 1.5 2^-25 -> 2^-24
        (2.0 ** -15, 2.0 ** -24, 0),    # a subnormal result with two bits set, exact
        (1.0, 2.0 ** -11, 0),           # a tie to even -> 1
        (1.0 + 2.0 ** -10, 2.0 ** -11, 0),  # a tie to odd -> 1 + 2^-9
        (1.0, 2.0 ** -12, 0),           # below the tie -> 1
        (1.0, 3 * 2.0 ** -12, 0),       # above the tie -> 1 + 2^-10
    ],
    "bf16": [
        (2.0 ** 128 - 2.0 ** 120, 2.0 ** 119 - 2.0 ** 111, 0),  # just under the overflow tie -> the largest bf16
        (2.0 ** 128 - 2.0 ** 120, 2.0 ** 119, 0),               # 0x7f7f8000, the tie -> inf
        (-(2.0 ** 128 - 2.0 ** 120), -2.0 ** 119, 0),           # -> -inf
        (2.0 ** -133, 0.0, 0),          # the smallest subnormal, kept
        (2.0 ** -133, 2.0 ** -133, -2),  # 2^-134, the tie -> 0
        (-2.0 ** -133, -2.0 ** -133, -2),  # -> -0
        (2.0 ** -132, 2.0 ** -133, -2),  # 1.5 2^-134 -> 2^-133
        (2.0 ** -127, 2.0 ** -133, 0),  # a subnormal result with two bits set, exact
        (1.0, 2.0 ** -8, 0),            # a tie to even -> 1
        (1.0 + 2.0 ** -7, 2.0 ** -8, 0),  # a tie to odd -> 1 + 2^-6
        (1.0, 2.0 ** -9, 0),            # below the tie -> 1
        (1.0, 3 * 2.0 ** -9, 0),        # above the tie -> 1 + 2^-7
    ],
}
_STORE_BOTH = [(float("nan"), 0.0, 0), (float("inf"), 0.0, 0), (float("-inf"), 0.0, 0), (float("inf"), float("-inf"), 0),
               (-0.0, 0.0, 0), (0.0, 0.0, 0), (1.0, -1.0, 0)]
STORE_P = 24  # pixels of the store cases (3 x 8): one per table row, the rest ordinary


@functools.lru_cache(maxsize=None)
def store_table(key):
    """(a, b in T; gamma, target in fp32), one entry per row of the table: the target is the fp32 value
    gamma (a + b), asserted exact in float64."""
    T = DTYPES[key]
    rows = _STORE[key] + _STORE_BOTH
    a = torch.tensor([r[0] for r in rows], dtype=torch.float64)
    b = torch.tensor([r[1] for r in rows], dtype=torch.float64)
    gam = torch.tensor([2.0 ** r[2] for r in rows], dtype=torch.float64)
    for t in (a, b):
        ok = (t.to(T).double() == t) | torch.isnan(t)
        assert bool(ok.all()), f"{key}: a table operand is no value of T"
    t64 = gam * a + gam * b
    t32 = (gam.float() * a.float()) + (gam.float() * b.float())
    exact = (t32.double() == t64) | torch.isnan(t64)
    assert bool(exact.all()), f"{key}: a target is not the exact fp32 sum"
    assert len(rows) <= STORE_P
    return a.to(T), b.to(T), gam.float(), t32


def store_case(key, layout_seed=0):
    """Two complete 3-node graphs, C = 3, ``film_sum``: in graph 0 ``out[0] = gamma (x[1] + x[2])`` holds the
    table (channel 0 rows with gamma = 1, channel 1 rows with gamma = 1/4, beta = 0 everywhere); channel 2 of
    node 0 has gamma = a NaN with an all-ones payload on one in-edge; graph 1 is ordinary.  Returns the graph,
    x (6, 3, 3, 8) in T, gb (12, 3, 2) and the expected output in T: torch's CPU cast of the fp32 oracle."""
    T = DTYPES[key]
    a, b, gam, _ = store_table(key)
    g = hc._frames([3, 3], 300)
    src, dst = (t.numpy() for t in g.edges())
    gen = torch.Generator().manual_seed(7 + layout_seed)
    x = torch.randn(6, 3, STORE_P, generator=gen).to(T)
    gb = torch.zeros(len(src), 3, 2)
    gb[:, :, 0] = 1.0
    gb[:, 1, 0] = 0.25
    for i in range(len(a)):
        c = 0 if float(gam[i]) == 1.0 else 1
        x[0, c, i], x[1, c, i], x[2, c, i] = 0.0, a[i], b[i]
    e = int(np.nonzero((dst == 0) & (src == 1))[0][0])
    gb[e, 2, 0] = FULL_NAN
    want = aggregate_ref(g, x.view(6, 3, 3, 8), gb, "film_sum")
    return dict(graph=g, x=x.view(6, 3, 3, 8), gb=gb, want=want.to(T), want32=want, rows=len(a))


COMPRESS_STORE_SHAPE = (3, 32, 4, 8)


@functools.lru_cache(maxsize=None)
def compress_store_case(key):
    """The table through the 16-bit compress products, C = 32, 4 x 8, 3 nodes, with selection weights (s = 1/4 on
    channel 1, 1 elsewhere; every product with a power of two exact, every output one fp32 addition):

    * forward: ``W[o, o] = W[o, C + o] = s[o]``, bias 0: y = s x + s agg; node 0 holds a in x and b in agg;
    * data gradient: ``W[c, c] = W[c + 16, c] = s[c]`` (both halves): gx = gagg = s (gy[c] + gy[c + 16 mod 32]);
      node 0 holds a in gy's channels 0 / 1 and b in channels 16 / 17;
    * weight gradient: gy = T's smallest subnormal on channel 5 and zero elsewhere, x = 1 on channel 3:
      gw[5, 3] = gbias[5] = 96 subnormals exactly, every other row of gw zero.

    The expected outputs are torch's CPU casts of the fp32 sums (the float64 product, which is exact, rounded)."""
    T = DTYPES[key]
    n, C, H, W = COMPRESS_STORE_SHAPE
    P = H * W
    a, b, gam, _ = store_table(key)
    gen = torch.Generator().manual_seed(23 + list(DTYPES).index(key))
    x, agg, gy = (torch.randn(n, C, P, generator=gen).to(T) for _ in range(3))
    s = torch.ones(C)
    s[1] = 0.25
    for i in range(len(a)):
        c = 0 if float(gam[i]) == 1.0 else 1
        x[0, c, i], agg[0, c, i] = a[i], b[i]
        gy[0, c, i], gy[0, c + 16, i] = a[i], b[i]
    wf = torch.zeros(C, 2 * C)
    wd = torch.zeros(C, 2 * C)
    idx = torch.arange(C)
    wf[idx, idx], wf[idx, C + idx] = s, s
    for half in (0, C):
        wd[idx, half + idx], wd[(idx + 16) % C, half + idx] = s, s
    # the products are dense: a zero weight times a NaN or an infinity is NaN, so a non-finite table row makes
    # its whole (node, pixel) column NaN; every finite output is one exact float64 sum, rounded to fp32 once
    with np.errstate(all="ignore"):
        y = torch.einsum("oc,ncp->nop", wf.double(), torch.cat((x, agg), 1).double()).float().to(T)
        gx = torch.einsum("oc,nop->ncp", wd.double(), gy.double())[:, :C].float().to(T)
    tiny = 2.0 ** -24 if key == "f16" else 2.0 ** -133
    gyw = torch.zeros(n, C, P, dtype=T)
    gyw[:, 5] = tiny
    xw = torch.randn(n, C, P, generator=gen).to(T)
    xw[:, 3] = 1.0
    shape = (n, C, H, W)
    v = lambda t: t.view(shape)  # noqa: E731
    return dict(x=v(x), a=v(agg), gy=v(gy), wf=wf.view(C, 2 * C, 1, 1), wd=wd.view(C, 2 * C, 1, 1), y=v(y), gx=v(gx),
                gyw=v(gyw), xw=v(xw), gw53=float(n * P * tiny), rows=len(a), tiny=tiny)


def cast_saturating(x, T):
    """A defective store: clamps to T's largest finite value before rounding."""
    big = torch.finfo(T).max
    return torch.where(torch.isnan(x), x, x.clamp(-big, big)).to(T)


def cast_truncating(x, T):
    """A defective store: rounds toward zero."""
    r = x.to(T)
    over = (r.float().abs() > x.abs()) & torch.isfinite(x)
    step = torch.nextafter(r, torch.zeros_like(r))
    big = torch.tensor(torch.finfo(T).max, dtype=T)
    step = torch.where(torch.isinf(r), torch.copysign(big, r), step)
    return torch.where(over, step, r)


def cast_bf16_no_nan_guard(x):
    """A defective bf16 store: (bits + 0x7fff + lsb) >> 16 on every pattern, NaN included."""
    b = bits(x.float().contiguous()).to(torch.int64) & 0xFFFFFFFF
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    return torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16).view(torch.bfloat16)


# ---- 4. poison ----------------------------------------------------------------------------------------------------

def poison_places(name):
    """(node, channel, pixel) of the poisoned elements of a ``half_cases`` case, each at its own (channel, pixel):
    node 0 (a non-neighbour of some destination in k-NN), the last node of the first graph and the first node
    of the next (the clamped loads of a ragged batch), the last node of the batch, and in the ragged case g the
    edgeless node 4 of its 5-node graph (global 6) and that graph's neighbours in memory; the last channel
    (C no multiple of the channel block in case c) and the last pixel among them."""
    g = hc.graph(name)
    n, C, H, W = hc.shape(name)
    P = H * W
    first = int(g.batch_num_nodes()[0])
    nodes = [0, first - 1, n - 1] + ([first] if first < n else [])
    if name == "g":
        nodes += [6, 7]
    nodes = sorted(set(nodes))
    out = []
    for i, node in enumerate(nodes):
        c = C - 1 if i == 0 else (i * 3) % C
        p = P - 1 if i == 1 else (i * 5 + 1) % P
        out.append((node, c, p))
    assert len({(c, p) for _, c, p in out}) == len(out)
    return out


def graph_nodes(g, node):
    """The node range (start, stop) of the graph of the batch that holds ``node``."""
    start = 0
    for s in (int(s) for s in g.batch_num_nodes()):
        if node < start + s:
            return start, start + s
        start += s
    raise ValueError(node)


def poisoned(x, places, value):
    """A copy of x (n, C, H, W) with ``value`` (fp32 scalar tensor; its bits are kept where T can hold them) at
    the places."""
    x = x.clone()
    flat = x.view(x.shape[0], x.shape[1], -1)
    for node, c, p in places:
        flat[node, c, p] = value.to(x.dtype)
    return x


def dense_forward(g, x, gb, mode="film_mean"):
    """A defective forward: the dense form, adjacency weights times messages — 0 * inf for non-neighbours."""
    src, dst = (t.numpy() for t in g.edges())
    n, C = x.shape[:2]
    x = x.float()
    gamma = torch.zeros(n, n, C)
    beta = torch.zeros(n, n, C)
    adj = torch.zeros(n, n)
    for e, (u, v) in enumerate(zip(src, dst)):
        gamma[v, u] += gb[e, :, 0]
        beta[v, u] += gb[e, :, 1]
        adj[v, u] += 1.0
    with np.errstate(all="ignore"):
        out = torch.einsum("vuc,uchw->vchw", gamma, x) + (beta.sum(1))[:, :, None, None]
    deg = adj.sum(1).clamp(min=1.0)
    return out / deg[:, None, None, None] if mode == "film_mean" else out


def relu_drops_nan(x):
    """A defective ReLU: x > 0 ? x : 0."""
    return torch.where(x > 0, x, torch.zeros_like(x))


def relu_integer_max(x):
    """A defective ReLU: the integer max of the bit pattern and 0."""
    return bits(x.float().contiguous()).clamp(min=0).view(torch.float32)


def relu_keeps_nan(x):
    """x < 0 ? 0 : x."""
    return torch.where(x < 0, torch.zeros_like(x), x)


#: encoder shapes (E, C): a ragged edge block, three hidden blocks, and C = 48 through the zero-padded route
ENCODER_SHAPES = ((33, 32), (96, 96))
ENCODER_PADDED = (33, 48)


def encoder_case(E, C):
    """fp32 encoder parameters (the reference's layer shapes) and poses of robot-scale magnitude."""
    gen = torch.Generator().manual_seed(E * 13 + C)
    w1 = (torch.rand(C, 9, generator=gen) * 2 - 1) / 3.0
    b1 = (torch.rand(C, generator=gen) * 2 - 1) / 3.0
    w2 = (torch.rand(2 * C, C, generator=gen) * 2 - 1) / C ** 0.5
    b2 = (torch.rand(2 * C, generator=gen) * 2 - 1) / C ** 0.5
    pose = torch.randn(E, 9, generator=gen) * 4
    return dict(E=E, C=C, w1=w1, b1=b1, w2=w2, b2=b2, pose=pose, rows=(E // 2, E - 1), col=(4, 8))


def encoder_ref(c, pose, relu=torch.relu):
    """(h (E, C), z (E, 2C)) of the reference layers in fp32 with the given ReLU."""
    h = relu(torch.nn.functional.linear(pose, c["w1"], c["b1"]))
    return h, torch.nn.functional.linear(h, c["w2"], c["b2"])


# ---- 5. scale equivariance of the split-bf16 products ---------------------------------------------------------------

#: per-operand exponents (sa, sb) under which ``split_cases.emulate`` is bit-equivariant on the operands used
#: (asserted in test_special_values_cpu.py, with every non-zero part a normal bf16)
SCALE_PAIRS = ((40, 40), (-40, -40), (100, 0), (0, -100), (60, 60))


def scale_pairs(C):
    """The pairs used at C channels: (-55, -55) passes that CPU check at C = 64 only (at C = 128 and 256 some
    third parts of the scaled operands fall below 2^-126), and a pair that fails it is not used."""
    return SCALE_PAIRS + (((-55, -55),) if C == 64 else ())
#: pairs at which the emulation is not equivariant: parts fall below bf16's normal range or overflow
SCALE_BROKEN = ((63, 63), (124, 0), (-60, -60), (-105, 0), (0, -110))
#: the encoder chains two products (h = relu(pose W1^T + b1) is split again): the pairs whose h and partial
#: parts stay normal too — (0, -100) is not among them: parts of the smallest hidden units fall below 2^-126
ENC_SCALE_PAIRS = ((40, 40), (-40, -40), (100, 0), (0, -80))
TOP = 0x7F7F8000  # the smallest finite fp32 that rounds to a bf16 infinity: 2^128 - 2^119


def away(t):
    """sign (0.25 + |t|): t bounded away from zero."""
    return torch.where(t < 0, -1.0, 1.0) * (0.25 + t.abs())


def away_from_zero(shape, seed):
    """``away`` of randn: random operands bounded away from zero."""
    return away(torch.randn(shape, generator=torch.Generator().manual_seed(seed)))


def scale_case(n, C, P, seed=0):
    """Operands of the three compress products: w (C, 2C), b (C), x, a, gy (n, C, P)."""
    return dict(n=n, C=C, P=P, w=away_from_zero((C, 2 * C), seed + 1) / (2 * C) ** 0.5, b=away_from_zero((C,), seed + 2),
                x=away_from_zero((n, C, P), seed + 3), a=away_from_zero((n, C, P), seed + 4),
                gy=away_from_zero((n, C, P), seed + 5))


def scale_products(c):
    """name -> (A, B, bias, which side the weight is on) as 2-D products (``split_cases.compress_products``'s
    layout): the weight-side operand is scaled by 2^sa, the feature side by 2^sb."""
    r = sc._rows
    return {"fwd": (c["w"], torch.cat((r(c["x"]), r(c["a"])), 0), c["b"]),
            "dgrad": (c["w"].t().contiguous(), r(c["gy"]), None),
            "wgrad": (r(c["gy"]), torch.cat((r(c["x"]), r(c["a"])), 0).t().contiguous(), None)}


def parts_normal(t):
    """Every non-zero bf16 part of t is a normal bf16 (and finite)."""
    for p in sc.split3(t):
        nz = p[p != 0]
        if not bool(torch.isfinite(nz).all()) or (nz.numel() and float(nz.abs().min()) < 2.0 ** -126):
            return False
    return True


def encoder_scale_case(E, C):
    """``encoder_case`` with W1, b1 and the poses bounded away from zero."""
    c = encoder_case(E, C)
    return dict(c, w1=away(c["w1"]), b1=away(c["b1"]), pose=away(c["pose"]))


def encoder_scaled(c, sa, sb):
    """W1 scaled by 2^sa, the poses by 2^sb, b1 and b2 by 2^(sa + sb): z scales by 2^(sa + sb)."""
    k = 2.0 ** (sa + sb)
    return dict(c, w1=c["w1"] * 2.0 ** sa, pose=c["pose"] * 2.0 ** sb, b1=c["b1"] * k, b2=c["b2"] * k)


def encoder_emulate(c):
    """(h^T (C, E), z^T (2C, E)) as the split kernel forms them (``split_cases.emulate``; b1 a tenth input of value
    1.0) and the operand pairs (A, B) of its two products."""
    A1 = torch.cat((c["w1"], c["b1"][:, None]), 1)
    B1 = torch.cat((c["pose"].t(), torch.ones(1, c["E"])), 0).contiguous()
    hT = relu_keeps_nan(sc.emulate(A1, B1))
    return hT, sc.emulate(c["w2"], hT, "six", c["b2"]), ((A1, B1), (c["w2"], hT))
