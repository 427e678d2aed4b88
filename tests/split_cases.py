"""Test infrastructure for the split-bf16 kernels' fp32-accuracy claim (``csrc/compress_split.hip``,
``csrc/encoder_split.hip``, ``csrc/encoder_split.hpp``): every fp32 operand split exactly into three
bf16 parts, a product = the six partial products ``a_i b_j`` with ``i + j <= 2``, ``a0 b0`` in its own
accumulator.

**Lattice operands** — values whose three parts are known by construction:

* ``bf16``:  ``s``                                 parts ``(s, 0, 0)``
* ``two``:   ``s (1 + j 2^-10)``                    parts ``(s, s j 2^-10, 0)``
* ``three``: ``s (1 + j 2^-10 + t 2^-19)``          parts ``(s, s j 2^-10, s t 2^-19)``

with ``s, t`` in ``{-1, +1}`` and ``j`` in ``{-1, 1, 2, 3}``.  (``j`` in ``{-2, -3}`` is left out: below
1 a bf16 step is 2^-8, so ``1 - 3 2^-10`` rounds to ``1 - 2^-8`` and ``1 - 2 2^-10 - 2^-19`` likewise —
the round-to-nearest-even split of those is not the one written above; :func:`lattice` asserts the
parts of everything it returns.)

Operands are made sparse (:func:`sparse_mask`: at most 12 non-zero products per output) so that, with q
the common quantum of the terms, ``sum_k |a_k b_k| < 2^24 q`` for every output: every partial sum, in
any order, in either accumulator, is a multiple of q below 2^24 q, i.e. an fp32 value — so a correct
six-product kernel, an fp32-MFMA kernel and torch must all reproduce the float64 product bit for bit
(:func:`exact_product` asserts the condition itself, in float64).

**Pairings** (kind of the A operand x kind of the B operand) and what each one needs:

* ``three x bf16``: ``a1 b0`` and ``a2 b0`` — fails with ``a2 b0`` dropped, a two-way split, first-order only;
* ``bf16 x three``: ``a0 b1`` and ``a0 b2`` — fails with a two-way split, first-order only;
* ``two x two``:    ``a1 b1``                — fails with ``a1 b1`` dropped.

:func:`emulate` is the torch emulation of the scheme and of its defective forms (:data:`FORMS`) that
``test_split_lattice_cpu.py`` uses to pin those statements without a GPU.

**Random operands**: :func:`within_fp32` — error against float64 at most ``factor`` x the error of an
fp32 evaluation of the same product, no absolute floor.
"""
import contextlib
import ctypes

import torch

import stack_ref

PAIRINGS = (("three", "bf16"), ("bf16", "three"), ("two", "two"))
#: quantum of a lattice value of each kind ("prod": a two x two product, the hidden layer of variant C)
QUANTUM = {"bf16": 1.0, "two": 2.0 ** -10, "three": 2.0 ** -19, "prod": 2.0 ** -20}
MAX_NNZ = 12


def pairing_id(p):
    return f"{p[0]}x{p[1]}"


def split3(x):
    """The three bf16 parts of fp32 x by round-to-nearest-even casts of the successive residuals (the
    kernels' ``split8``), as fp32 tensors."""
    x = x.float()
    a0 = x.bfloat16().float()
    r1 = x - a0
    a1 = r1.bfloat16().float()
    r2 = r1 - a1
    a2 = r2.bfloat16().float()
    return a0, a1, a2


def lattice(kind, shape, seed):
    """A dense fp32 CPU tensor of lattice values of ``kind``; asserts their three parts."""
    g = torch.Generator().manual_seed(seed)
    s = (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()
    jv = torch.tensor([-1.0, 1.0, 2.0, 3.0], dtype=torch.float64)
    j = jv[torch.randint(0, 4, shape, generator=g)]
    t = (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()
    p0, p1, p2 = s, s * j * 2.0 ** -10, s * t * 2.0 ** -19
    if kind == "bf16":
        p1, p2 = torch.zeros_like(s), torch.zeros_like(s)
    elif kind == "two":
        p2 = torch.zeros_like(s)
    elif kind != "three":
        raise ValueError(kind)
    x64 = p0 + p1 + p2
    x = x64.float()
    assert torch.equal(x.double(), x64), f"{kind}: lattice values are not fp32 values"
    a0, a1, a2 = split3(x)
    assert torch.equal(a0.double(), p0) and torch.equal(a1.double(), p1) and torch.equal(a2.double(), p2), \
        f"{kind}: the bf16 split of the lattice values is not the constructed one"
    assert torch.equal((a0.double() + a1.double() + a2.double()), x64)
    return x


def sparse_mask(M, K, nnz=MAX_NNZ, cover=True):
    """(M, K) 0/1 mask with ones at k = (5 m + 21 t) mod K, t < nnz, in row m: at most nnz per row.  With
    ``cover`` asserts that over the rows every k is hit — k = 0, k = K - 1 and both sides of every 16-
    and 32-wide k-step boundary among them."""
    m = torch.arange(M)[:, None]
    t = torch.arange(nnz)[None, :]
    mask = torch.zeros(M, K)
    mask[m.expand(M, nnz), (5 * m + 21 * t) % K] = 1.0
    assert int(mask.sum(1).max()) <= nnz
    if cover:
        assert bool((mask.sum(0) > 0).all()), f"sparse_mask({M}, {K}): not every k index is hit"
    return mask


def exact_product(A, B, qa, qb, bias=None, what="", most=True):
    """The float64 product A B (+ bias down the rows) of fp32 CPU operands whose entries are multiples
    of qa / qb, after asserting the exactness conditions: sum_k |a_k b_k| (+ |bias|) < 2^24 qa qb for
    every output, at most 12 non-zero products per output, and the result an fp32 value."""
    A64, B64 = A.double(), B.double()
    for o, q in ((A64, qa), (B64, qb)):
        assert torch.equal((o / q).round() * q, o), f"{what}: operand entries are not multiples of {q}"
    q = qa * qb
    mag = A64.abs() @ B64.abs()
    nnz = (A64 != 0).double() @ (B64 != 0).double()
    ref = A64 @ B64
    if bias is not None:
        b64 = bias.double()
        assert bool(((b64 == 0) | (b64.abs() == 1)).all()), f"{what}: the bias is not 0 or +-1"
        mag = mag + b64.abs()[:, None]
        ref = ref + b64[:, None]
    assert float(mag.max()) < 2.0 ** 24 * q, f"{what}: sum |a b| = {float(mag.max())} reaches 2^24 x {q}"
    assert int(nnz.max()) <= MAX_NNZ, f"{what}: {int(nnz.max())} non-zero products in one output"
    if most:  # the product is there to catch defects: most of its outputs must hold a non-zero product
        assert int((nnz > 0).sum()) * 2 >= nnz.numel(), f"{what}: most outputs are empty sums"
    assert torch.equal(ref.float().double(), ref), f"{what}: the float64 result is not an fp32 value"
    return ref


def assert_bit_equal(got, ref64, what):
    """``torch.equal(got, ref64.float())`` with the count of wrong elements and the first wrong index."""
    got = got.detach().cpu()
    want = ref64.float().reshape(got.shape)
    if torch.equal(got, want):
        return
    bad = (got != want) | torch.isnan(got)
    idx = tuple(int(i) for i in bad.nonzero()[0])
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the float64 product; "
                         f"first at {idx}: got {got[idx].item()!r}, want {want[idx].item()!r}")


# ---- the emulation ----------------------------------------------------------------------------------

_SIX = ((1, 1), (0, 2), (2, 0), (0, 1), (1, 0), (0, 0))
#: form -> (bf16 parts kept per operand, the partial products (i, j) summed)
FORMS = {"six": (3, _SIX)}
for _i, _j in _SIX:
    FORMS[f"drop_a{_i}b{_j}"] = (3, tuple(p for p in _SIX if p != (_i, _j)))
FORMS["two_way"] = (2, tuple(p for p in _SIX if max(p) < 2))
FORMS["first_order"] = (3, ((0, 1), (1, 0), (0, 0)))
DEFECTS = tuple(f for f in FORMS if f != "six")


def emulate(A, B, form="six", bias=None, block=32):
    """A B (+ bias down the rows) as the kernels form it: bf16 casts for the split, float64 products of
    ``block``-wide k steps, the ``a0 b0`` steps added into one fp32 accumulator (hi) and the others into
    a second (lo), hi + lo (+ bias) in fp32 at the end."""
    nparts, pairs = FORMS[form]
    pa = [p.double() for p in split3(A)[:nparts]]
    pb = [p.double() for p in split3(B)[:nparts]]
    M, K = A.shape
    hi = torch.zeros(M, B.shape[1])
    lo = torch.zeros(M, B.shape[1])
    for k0 in range(0, K, block):
        for i, j in pairs:
            blk = pa[i][:, k0:k0 + block] @ pb[j][k0:k0 + block]
            if (i, j) == (0, 0):
                hi = (hi.double() + blk).float()
            else:
                lo = (lo.double() + blk).float()
    out = hi + lo
    return out + bias.float()[:, None] if bias is not None else out


def within_fp32(ours, f32, f64, factor):
    """ours is within ``factor`` x the fp32 evaluation's error of the float64 result (``stack_ref.err``:
    max |d| / max |ref|); no absolute floor.  Returns (ok, (err of ours, err of f32))."""
    e_ours, e_ref = stack_ref.err(ours, f64), stack_ref.err(f32, f64)
    return e_ours <= factor * e_ref, (e_ours, e_ref)


# ---- compress cases ---------------------------------------------------------------------------------

def _bias(n, seed):
    return (torch.randint(-1, 2, (n,), generator=torch.Generator().manual_seed(seed))).float()


def compress_case(n, C, P, pairing, seed=0, cover=True):
    """Operands of the three compress products with the A-side kind of ``pairing`` in the weight (forward,
    data gradient) and in gy (weight gradient), the B-side kind in the activations:

    * ``w`` (C, 2C): at most 12 non-zeros per row and per column; ``b`` (C) in {0, +-1};
    * ``x``, ``a`` (n, C, P) dense — the forward's B operand; ``gy`` (n, C, P) dense — the data gradient's;
    * ``gy_s`` (n, C, P): at most 12 non-zero (node, pixel) positions per channel, and ``xs``, ``as_``
      dense — the weight gradient's A and B operands (``gb`` = the row sums of gy_s).
    """
    ka, kb = pairing
    s = seed * 100
    w = lattice(ka, (C, 2 * C), s + 1) * sparse_mask(C, 2 * C, cover=cover)
    assert int((w != 0).sum(0).max()) <= MAX_NNZ
    gmask = sparse_mask(C, n * P, cover=cover).view(C, n, P).permute(1, 0, 2)
    return {
        "n": n, "C": C, "P": P, "pairing": pairing, "w": w, "b": _bias(C, s + 2),
        "x": lattice(kb, (n, C, P), s + 3), "a": lattice(kb, (n, C, P), s + 4),
        "gy": lattice(kb, (n, C, P), s + 5),
        "gy_s": lattice(ka, (n, C, P), s + 6) * gmask,
        "xs": lattice(kb, (n, C, P), s + 7), "as_": lattice(kb, (n, C, P), s + 8),
    }


def _rows(t):
    """(n, C, P) -> (C, n P): channel rows over k = (node, pixel)."""
    return t.permute(1, 0, 2).reshape(t.shape[1], -1)


def compress_products(c, bias=True):
    """name -> (A, B, bias or None) of the 2-D products of a compress case (CPU, fp32): ``fwd`` (y as
    (C, n P)), ``dgrad`` ([gx; ga] as (2C, n P)), ``wgrad`` (gw (C, 2C))."""
    return {
        "fwd": (c["w"], torch.cat((_rows(c["x"]), _rows(c["a"])), 0), c["b"] if bias else None),
        "dgrad": (c["w"].t().contiguous(), _rows(c["gy"]), None),
        "wgrad": (_rows(c["gy_s"]), torch.cat((_rows(c["xs"]), _rows(c["as_"])), 0).t().contiguous(), None),
    }


def compress_refs(c, bias=True):
    """Float64 results of a compress case in the kernels' layouts, the exactness conditions asserted:
    y, gx, ga (n, C, P), gw (C, 2C), gb (C)."""
    n, C, P = c["n"], c["C"], c["P"]
    qa, qb = QUANTUM[c["pairing"][0]], QUANTUM[c["pairing"][1]]
    r = {k: exact_product(A, B, qa, qb, bb, f"compress {k} {pairing_id(c['pairing'])}")
         for k, (A, B, bb) in compress_products(c, bias).items()}
    g = r["dgrad"].view(2 * C, n, P).permute(1, 0, 2)
    gb = _rows(c["gy_s"]).double().sum(1)
    assert torch.equal(gb.float().double(), gb)
    return {"y": r["fwd"].view(C, n, P).permute(1, 0, 2).contiguous(), "gx": g[:, :C].contiguous(),
            "ga": g[:, C:].contiguous(), "gw": r["wgrad"], "gb": gb}


# ---- encoder cases ----------------------------------------------------------------------------------

#: variant -> (pose kind, W1 kind, hidden kind, W2 kind): the pairing of the hidden product (pose, W1) and
#: of the logits product (h, W2); "-" marks a product that needs no small part
ENCODER_VARIANTS = {
    "three.bf16/three.bf16": ("three", "bf16", "three", "bf16"),
    "bf16.three/three.bf16": ("bf16", "three", "three", "bf16"),
    "two.two/prod.bf16": ("two", "two", "prod", "bf16"),
    "-/bf16.three": ("bf16", "bf16", "bf16", "three"),
    "-/two.two": ("two", "bf16", "two", "two"),
}


def encoder_case(E, C, variant, seed=0):
    """A two-stage chain that stays exact: W1 rows one-hot (unit u reads pose column u mod 9) and b1 = 0,
    so h = relu(pose_i w) is a lattice value (or a two x two product) or 0; W2 (2C, C) with at most 6
    non-zeros per row and 12 per column; b2 in {0, +-1}.  Returns the operands and the float64 h, z."""
    kp, k1, kh, k2 = ENCODER_VARIANTS[variant]
    s = seed * 100 + 50
    pose = lattice(kp, (E, 9), s + 1)
    w1 = torch.zeros(C, 9)
    w1[torch.arange(C), torch.arange(C) % 9] = lattice(k1, (C,), s + 2)
    b1 = torch.zeros(C)
    h64 = torch.relu(pose.double() @ w1.double().t())
    assert torch.equal(h64.float().double(), h64)
    w2 = lattice(k2, (2 * C, C), s + 3) * sparse_mask(2 * C, C, nnz=6)
    assert int((w2 != 0).sum(0).max()) <= MAX_NNZ
    b2 = _bias(2 * C, s + 4)
    z64 = exact_product(w2, h64.float().t().contiguous(), QUANTUM[k2], QUANTUM[kh], b2, f"encoder z {variant}").t()
    return {"E": E, "C": C, "pose": pose, "w1": w1, "b1": b1, "w2": w2, "b2": b2, "h64": h64, "z64": z64.contiguous()}


def encoder_products(c):
    """name -> (A, B, bias) of the 2-D products of an encoder case: the hidden layer's (before its ReLU)
    and the logits' (as z^T)."""
    return {"hidden": (c["w1"], c["pose"].t().contiguous(), None),
            "logits": (c["w2"], c["h64"].float().t().contiguous(), c["b2"])}


def encoder_bwd_case(E, C, pairing, seed=0):
    """Operands of the encoder's backward GEMMs, the A-side kind of ``pairing`` in dz, the B-side kind in
    W2 and h: ``dz`` (E, 2C) with at most 12 non-zero edges per column, ``dz_d`` dense, ``w2`` (2C, C) with
    at most 6 non-zeros per row and 12 per column, ``hT`` (C, E) = relu of lattice values, ``pose`` +-1.
    Float64 results: ``dhT`` / ``dhT_d`` (C, E) = W2^T dz^T for dz / dz_d, ``dw2`` (2C, C) = dz^T h and
    ``db2`` (2C) = the column sums of dz."""
    ka, kb = pairing
    s = seed * 100 + 70
    dz = lattice(ka, (E, 2 * C), s + 1) * sparse_mask(2 * C, E).t()
    dz_d = lattice(ka, (E, 2 * C), s + 2)
    w2 = lattice(kb, (2 * C, C), s + 3) * sparse_mask(2 * C, C, nnz=6)
    hT = torch.relu(lattice(kb, (C, E), s + 4))
    pose = lattice("bf16", (E, 9), s + 5)
    qa, qb = QUANTUM[ka], QUANTUM[kb]
    w2t = w2.t().contiguous()
    tag = pairing_id(pairing)
    db2 = dz.double().sum(0)
    assert torch.equal(db2.float().double(), db2)
    return {"E": E, "C": C, "pairing": pairing, "dz": dz, "dz_d": dz_d, "w2": w2, "hT": hT, "pose": pose,
            "dhT": exact_product(w2t, dz.t().contiguous(), qb, qa, None, f"encoder dhT {tag}", most=False),
            "dhT_d": exact_product(w2t, dz_d.t().contiguous(), qb, qa, None, f"encoder dhT (dense dz) {tag}"),
            "dw2": exact_product(dz.t().contiguous(), hT.t().contiguous(), qa, qb, None, f"encoder dW2 {tag}"),
            "db2": db2}


def encoder_bwd_products(c):
    return {"dhT": (c["w2"].t().contiguous(), c["dz_d"].t().contiguous(), None),
            "dw2": (c["dz"].t().contiguous(), c["hT"].t().contiguous(), None)}


def encoder_dw1_refs(c):
    """Float64 dW1 (C, 9) and db1 (C) of a backward case through the whole chain — dpre = dh^T (.) [h^T > 0],
    dW1 = dpre pose, db1 = its row sums — with the condition that keeps the second summation exact
    asserted: sum_e |dpre| < 2^24 x the quantum of dh^T (pose is +-1).  Holds for the coarse pairing
    (bf16 dz, two W2: quantum 2^-10), not for the three :data:`PAIRINGS`."""
    q = QUANTUM[c["pairing"][0]] * QUANTUM[c["pairing"][1]]
    dpre = c["dhT"] * (c["hT"] > 0)
    assert float(dpre.abs().sum(1).max()) < 2.0 ** 24 * q
    dw1, db1 = dpre @ c["pose"].double(), dpre.sum(1)
    assert torch.equal(dw1.float().double(), dw1) and torch.equal(db1.float().double(), db1)
    return dw1, db1


def encoder_reduce_case(E, C, pairing, seed=0):
    """Lattice operands fed directly to ``mrp_edge_encoder_bwd_t`` and ``_bwd_pose``: ``hT`` (C, E) relu of
    lattice values; for dW1 = dpre pose / db1: ``dhT`` (C, E) with at most 12 non-zeros per row (A-side
    kind) and ``pose`` (E, 9) dense (B-side kind); for dpose = dpre^T W1: ``dhT_p`` with at most 12
    non-zeros per column and ``w1`` (C, 9) dense.  Float64 ``dw1``, ``db1``, ``dpose``."""
    ka, kb = pairing
    s = seed * 100 + 90
    hT = torch.relu(lattice("two", (C, E), s + 1))
    dhT = lattice(ka, (C, E), s + 2) * sparse_mask(C, E)
    dhT_p = lattice(ka, (C, E), s + 3) * sparse_mask(E, C).t()
    pose = lattice(kb, (E, 9), s + 4)
    w1 = lattice(kb, (C, 9), s + 5)
    qa, qb = QUANTUM[ka], QUANTUM[kb]
    gate = (hT > 0).float()
    tag = pairing_id(pairing)
    db1 = (dhT * gate).double().sum(1)
    assert torch.equal(db1.float().double(), db1)
    return {"E": E, "C": C, "hT": hT, "dhT": dhT, "dhT_p": dhT_p, "pose": pose, "w1": w1,
            "dw1": exact_product(dhT * gate, pose, qa, qb, None, f"encoder dW1 {tag}"), "db1": db1,
            "dpose": exact_product((dhT_p * gate).t().contiguous(), w1, qa, qb, None, f"encoder dpose {tag}")}


# ---- shapes shared by the GPU tests and the CPU test of their teeth ------------------------------------

#: (n, C, P) of the compress lattice cases: C = 64 (gemm_split 2: 128-row workgroups; M = C is one ragged
#: tile forward, 2C = 128 a whole one in the data gradient) and C = 256 (form 7's 256-row workgroups), n = 3
#: nodes of 32 pixels (96 columns: a ragged 128-column tile)
COMPRESS_SHAPES = ((3, 64, 32), (3, 256, 32))
#: (E, C) of the encoder forward lattice cases
ENCODER_SHAPES = tuple((E, C) for E in (1, 33, 96) for C in (32, 96))
#: (E, C) of the encoder backward lattice cases: one ragged tile, and two row tiles of dW2 (2C = 384 > 256)
ENCODER_BWD_SHAPES = ((32, 32), (96, 192))

# ---- GPU-side helpers shared by test_gpu_split_lattice.py and test_gpu_split_fp32.py ------------------------


def stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


@contextlib.contextmanager
def knobs(path="split", **knobs):
    """The compress path and tuning knobs of one form; everything restored on the way out."""
    import mrp_gnn_amd as m
    lib = m.load_library()
    prev = m.compress.compress_path()
    m.compress.set_compress_path(path)
    try:
        for k, v in knobs.items():
            assert lib.mrp_tuning_set(k.encode(), v) == 0, k
        yield lib
    finally:
        lib.mrp_tuning_set(b"reset", 0)
        m.compress.set_compress_path(prev)


#: form -> (compress path, knobs): "split" the per-shape choice, 2 = 128-row workgroups on 32x32x16 MFMAs,
#: 7 = 256-row workgroups on 16x16x32 (where M % 256 == 0, else 2's kernel), "hip" the fp32 MFMA
GEMM_FORMS = {"split": ("split", {}), "split2": ("split", {"gemm_split": 2}), "split7": ("split", {"gemm_split": 7}),
              "hip": ("hip", {})}
NT_FORMS = {"split_nt3": ("split", {"split_nt": 3}), "split_nt4": ("split", {"split_nt": 4}), "hip": ("hip", {})}


def bwd_split(lib, dev, E, C, dz, dzT, w2t, hT, dhT, dw2, db2):
    import mrp_gnn_amd as m
    from mrp_gnn_amd.aggregate import _ptr
    nbytes = int(lib.mrp_edge_encoder_bwd_split_workspace(E, C))
    ws = torch.empty((nbytes + 3) // 4, device=dev) if nbytes > 0 else None
    p = lambda t: _ptr(t) if t is not None else None  # noqa: E731
    m._lib.check(lib.mrp_edge_encoder_bwd_split(p(dz), p(dzT), p(w2t), p(hT), E, C, p(dhT), p(dw2), p(db2), p(ws),
                                                nbytes, stream(dev)), "mrp_edge_encoder_bwd_split")
    torch.cuda.synchronize()


def bwd_fused(lib, dev, c, t):
    import mrp_gnn_amd as m
    from mrp_gnn_amd.aggregate import _ptr
    E, C = c["E"], c["C"]
    img = m.encoder._pack_w2t(t["w2"])
    nbytes = int(lib.mrp_edge_encoder_bwd_fused_workspace(E, C))
    ws = torch.empty((nbytes + 3) // 4, device=dev)
    new = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731
    dw1, db1, dw2, db2 = new(C, 9), new(C), new(2 * C, C), new(2 * C)
    m._lib.check(lib.mrp_edge_encoder_bwd_fused(_ptr(t["dz"]), _ptr(t["w2t"]), _ptr(img), _ptr(t["hT"]), _ptr(t["pose"]),
                                                E, C, _ptr(dw1), _ptr(db1), _ptr(dw2), _ptr(db2), _ptr(ws), nbytes,
                                                stream(dev)), "mrp_edge_encoder_bwd_fused")
    torch.cuda.synchronize()
    return dw1, db1, dw2, db2


#: knobs of the fused backward's forms: its A operands pre-split or not, and the split counts of its two
#: products forced to 1 and to 2 (the reduction of the partial tiles)
FUSED_FORMS = [{"enc_bwd_psa": 2}, {"enc_bwd_psa": 1}, {"enc_bwd_psa": 0}, {"enc_s1": 1, "enc_s2": 1},
               {"enc_s1": 2, "enc_s2": 2}, {"enc_bwd_psa": 0, "enc_s1": 2, "enc_s2": 3}]
