"""The no-grad edge encoder on its own stream (``encoder.encoder_forward_split`` -> ``_enc_begin`` /
``_enc_end``): the only place where a product kernel reads memory that another stream may still be
writing.  The encoder stream is ordered only after per-tensor readiness events (``_ready_event``,
``_image_ready``) and the caller's stream joins it (``mrp_stream_join`` or ``wait_stream``).

Every scenario runs the same forward twice — on the encoder stream and, with
``set_encoder_stream(False)``, on the caller's stream, which is ordered after everything by
construction — and asserts

(a) the two outputs are ``torch.equal``;
(b) ``encoder.PATH_COUNTS["enc_stream"]`` rose by the number of encoder calls of the first run and
    ``"enc_inline"`` by that of the second (so the first run really left the caller's stream);
(c) where a write sits behind a stall, that the write was still pending when the stream-on forward
    returned (an event recorded right after the write has not completed): otherwise the encoder could
    not have run ahead of the write and the scenario would prove nothing.  It then fails, saying that
    the stall is too short.

The stall is ``busy.mul_(1.0)`` on a 256 MB buffer, repeated; the repeat count comes from two
measurements made by the module fixture on the device the tests run on: the GPU time of one repeat
(a pair of timing events) and the host time of one no-grad ``GCN.forward`` enqueue (``perf_counter``),
so that one stall lasts at least 10 enqueues; scenarios with k forwards (or k encoders, or a
rebuild of the weight images) in flight queue k stalls.  Measured on an MI355X (five runs): one
``busy.mul_(1.0)`` 0.0736-0.0739 ms of GPU time (512 MB of traffic), one forward enqueue 75-84 us of
host time, hence 11 or 12 repeats per stall (0.81-0.89 ms).  S12 sizes its stall from the host time of
its own sequence, because the first use of a fresh stream costs the host milliseconds: 6.3 to 13 ms
measured for the two forwards around the switch, i.e. 72 to 159 stalls (64-129 ms).

The small shape (2 complete 4-robot graphs, E = 24, C = 32, 4 x 4 planes) reaches the encoder stream
through ``set_encoder_stream_min_work(0)``; S4, S14 and S16 reach it at the default threshold.

Under a mutation of ``_enc_begin`` whose inner ``wait(ev)`` does nothing (stale reads of valid
memory; ``record_stream`` and the join left alone) S1-S6 (every case), S8, S9, S10, S11 and S12
failed on (a) on an MI355X; S7 (``wait_stream`` branch), S13-S16 (no stalled write) passed, and so did
``test_gpu_eval_path.py::test_encoder_stream_ordered_after_input_writes``, which never leaves the
caller's stream.  On the parent's ``encoder.py`` S12 failed on (a) for its second forward (the stream
created by the priority switch inherited the old stream's ``_waited``) and everything else passed.

S16 cannot assert that an encoder and ``film_fwd`` really shared the CUs (no profiler in a test): it
is the bit-for-bit evidence for back-to-back forwards at a size where the next encoder has an
aggregation to run beside, not a statement about co-residency.
"""
import math
import time
import types

import numpy as np
import pytest
import torch

import mrp_gnn_amd as m
import stack_ref

pytestmark = pytest.mark.gpu

enc = m.encoder
DEFAULT_MIN_WORK = 1 << 18
SMALL = dict(B=2, N=4, C=32, H=4)
NATURAL = dict(B=32, N=8, C=512, H=4)  # E C = 1792 x 512 = 917 504 >= 2^18


@pytest.fixture(autouse=True)
def _restore_encoder_state():
    yield
    enc.set_encoder_stream(True)
    enc.set_encoder_stream_min_work(DEFAULT_MIN_WORK)
    enc.set_encoder_stream_priority(-1)
    enc.set_fast_join(True)


def _robot_poses(B, N, seed):
    rng = np.random.RandomState(seed)
    t = rng.uniform(-10, 10, size=(B, N, 3))
    q = rng.standard_normal((B, N, 4))
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    return np.concatenate([t, q], 2).astype(np.float32)


def _graph(device, B, N, seed=11):
    """B complete N-robot graphs with their edge poses on the device, no node features."""
    return m.batch([m.frame_graph(p) for p in _robot_poses(B, N, seed)]).to(device)


def _feats(device, B, N, C, H, seed=11):
    gen = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(B * N, C, H, H, device=device, generator=gen)


def _gcn(device, C, seed=2, **opt):
    torch.manual_seed(seed)
    return m.GCN(types.SimpleNamespace(feature_dim=C, **opt)).to(device)


def _setup(device, B, N, C, H, seed=11):
    return _gcn(device, C), _graph(device, B, N, seed), _feats(device, B, N, C, H, seed)


def _counts():
    return enc.PATH_COUNTS["enc_stream"], enc.PATH_COUNTS["enc_inline"]


class _Stall:
    def __init__(self, busy, reps, rep_ms, host_us):
        self.busy, self.reps, self.rep_ms, self.host_us = busy, reps, rep_ms, host_us

    def __call__(self, scale=1):
        for _ in range(self.reps * scale):
            self.busy.mul_(1.0)

    def write(self, fn, scale=1):
        """Queue ``scale`` stalls and then the write ``fn`` on the current stream; the event recorded
        right after the write."""
        with torch.no_grad():
            self(scale)
            fn()
        ev = torch.cuda.Event()
        ev.record()
        return ev

    def too_short(self, scale=1):
        return (f"the stall is too short: the work queued behind it had completed when the stream-on forward "
                f"returned ({self.reps * scale} repeats of {self.rep_ms:.3f} ms; host enqueue measured "
                f"{self.host_us:.0f} us) - the scenario proved nothing")


@pytest.fixture(scope="module")
def stall(cuda_device):
    busy = torch.randn(64 << 20, device=cuda_device)  # 256 MB, once per module
    scratch = torch.zeros(8, device=cuda_device)
    for _ in range(3):
        busy.mul_(1.0)
        scratch.add_(0.5)  # the kernels the stalled writes use are loaded before any stall
        scratch.mul_(1.25)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(8):
        busy.mul_(1.0)
    t1.record()
    torch.cuda.synchronize()
    rep_ms = t0.elapsed_time(t1) / 8
    gcn, g, x = _setup(cuda_device, **SMALL)
    prev = enc.set_encoder_stream_min_work(0)
    try:
        with torch.no_grad():
            for _ in range(5):
                gcn(g, x)
            torch.cuda.synchronize()
            h0 = time.perf_counter()
            for _ in range(20):
                gcn(g, x)
            host_us = (time.perf_counter() - h0) / 20 * 1e6
        torch.cuda.synchronize()
    finally:
        enc.set_encoder_stream_min_work(prev)
    reps = max(4, math.ceil(10 * host_us * 1e-3 / rep_ms))
    print(f"\n[encoder-stream stall] one busy.mul_ {rep_ms:.4f} ms GPU; one no-grad GCN.forward enqueue "
          f"{host_us:.1f} us host; repeats per stall {reps} ({reps * rep_ms:.2f} ms)")
    return _Stall(busy, reps, rep_ms, host_us)


def _pair(fwd, calls, stall=None, ev=None, scale=1):
    """``fwd()`` (a tensor or a list of tensors) on the encoder stream and then on the caller's
    stream: (b) the path counters, (c) ``ev`` still pending right after the first, (a) equal outputs.
    Returns the first run's outputs."""
    s0, i0 = _counts()
    with torch.no_grad():
        on = fwd()
    pending = ev is None or not ev.query()  # before anything synchronises
    s1, i1 = _counts()
    enc.set_encoder_stream(False)
    try:
        with torch.no_grad():
            off = fwd()
    finally:
        enc.set_encoder_stream(True)
    s2, i2 = _counts()
    assert pending, stall.too_short(scale)
    assert (s1 - s0, i1 - i0) == (calls, 0), "the stream-on run did not take the encoder stream"
    assert (s2 - s1, i2 - i1) == (0, calls)
    torch.cuda.synchronize()
    if torch.is_tensor(on):
        assert torch.equal(on, off), "encoder-stream result differs from the caller's-stream result"
    else:
        bad = [k for k, (a, b) in enumerate(zip(on, off)) if not torch.equal(a, b)]
        assert len(on) == len(off) and not bad, f"outputs {bad} differ from the caller's-stream results"
    return on


def _warm(gcn, g, x):
    """One stream-on forward outside the measurement: the device CSR and the weight image exist, the
    readiness events are cached, nothing of the next forward touches the host allocator or syncs."""
    with torch.no_grad():
        out = gcn(g, x)
    torch.cuda.synchronize()
    return out


JOINS = pytest.mark.parametrize("fast_join", [True, False], ids=["mrp_stream_join", "wait_stream"])


@JOINS
def test_s1_pose_written_behind_stall(cuda_device, stall, fast_join):
    enc.set_fast_join(fast_join)
    enc.set_encoder_stream_min_work(0)
    gcn, g, x = _setup(cuda_device, **SMALL)
    a = _warm(gcn, g, x)
    ev = stall.write(lambda: g.edata["pose"].mul_(1.25))
    c = _pair(lambda: gcn(g, x), 1, stall, ev)
    assert not torch.equal(c, a)


@JOINS
def test_s2_optimizer_step_behind_stall(cuda_device, stall, fast_join):
    """Every parameter updated in place: the packed image is rebuilt by the forward (its pack kernel
    behind the stall too) and its ``_track_image`` event orders it."""
    enc.set_fast_join(fast_join)
    enc.set_encoder_stream_min_work(0)
    gcn, g, x = _setup(cuda_device, **SMALL)
    a = _warm(gcn, g, x)
    img = enc.packed_weights(gcn.edge_encoder.layers[0], gcn.edge_encoder.layers[2])

    def step():
        for p in gcn.parameters():
            p.mul_(0.75)

    ev = stall.write(step, scale=2)
    c = _pair(lambda: gcn(g, x), 1, stall, ev, scale=2)
    assert not torch.equal(c, a)
    assert enc.packed_weights(gcn.edge_encoder.layers[0], gcn.edge_encoder.layers[2]) is not img


@JOINS
def test_s3_b2_only_behind_stall(cuda_device, stall, fast_join):
    """Only ``layers[2].bias`` changed: not in the image key, ordered by its own readiness event."""
    enc.set_fast_join(fast_join)
    enc.set_encoder_stream_min_work(0)
    gcn, g, x = _setup(cuda_device, **SMALL)
    a = _warm(gcn, g, x)
    img = enc.packed_weights(gcn.edge_encoder.layers[0], gcn.edge_encoder.layers[2])
    ev = stall.write(lambda: gcn.edge_encoder.layers[2].bias.add_(0.5))
    c = _pair(lambda: gcn(g, x), 1, stall, ev)
    assert not torch.equal(c, a)
    assert enc.packed_weights(gcn.edge_encoder.layers[0], gcn.edge_encoder.layers[2]) is img


@JOINS
def test_s4_pose_written_at_natural_threshold(cuda_device, stall, fast_join):
    """S1 without the hook: E C = 917 504 is past the default threshold."""
    enc.set_fast_join(fast_join)
    assert enc.set_encoder_stream_min_work(DEFAULT_MIN_WORK) == DEFAULT_MIN_WORK
    gcn, g, x = _setup(cuda_device, **NATURAL)
    assert g.num_edges() * NATURAL["C"] >= DEFAULT_MIN_WORK
    a = _warm(gcn, g, x)
    ev = stall.write(lambda: g.edata["pose"].mul_(1.25))
    c = _pair(lambda: gcn(g, x), 1, stall, ev)
    assert not torch.equal(c, a)


@pytest.mark.parametrize("kind", ["float64", "noncontiguous"])
def test_s5_converted_pose_copy(cuda_device, stall, kind):
    """The converted-copy branch of ``_enc_begin`` (``same`` false, a fresh event per call): the
    conversion kernel itself sits behind the stall."""
    enc.set_encoder_stream_min_work(0)
    gcn, g, x = _setup(cuda_device, **SMALL)
    pose = g.edata["pose"]
    if kind == "float64":
        p = pose.double()
    else:
        p = pose.t().contiguous().t()
        assert not p.is_contiguous() and p.shape == pose.shape
    g.edata["pose"] = p
    a = _warm(gcn, g, x)
    ev = stall.write(lambda: p.mul_(1.25))
    c = _pair(lambda: gcn(g, x), 1, stall, ev)
    assert not torch.equal(c, a)


@pytest.mark.parametrize("write", ["pose", "bias"])
def test_s6_padded_weights_route(cuda_device, stall, write):
    """C = 48: ``padded_weights`` and its ``rec.b2``, with S1's pose write or S3's bias write (which
    rebuilds the padded record: a dozen small kernels behind the stall)."""
    enc.set_encoder_stream_min_work(0)
    C = 48
    gcn, g, x = _setup(cuda_device, SMALL["B"], SMALL["N"], C, SMALL["H"])
    a = _warm(gcn, g, x)
    rec = enc._padded.get(gcn.edge_encoder.layers[2])
    assert rec is not None and rec.Cp == 64
    split0 = enc.PATH_COUNTS["split"]
    if write == "pose":
        ev = stall.write(lambda: g.edata["pose"].mul_(1.25))
        c = _pair(lambda: gcn(g, x), 1, stall, ev)
    else:
        ev = stall.write(lambda: gcn.edge_encoder.layers[2].bias.add_(0.5), scale=3)
        c = _pair(lambda: gcn(g, x), 1, stall, ev, scale=3)
    assert not torch.equal(c, a)
    assert enc.PATH_COUNTS["split"] == split0 + 2
    assert (enc._padded.get(gcn.edge_encoder.layers[2]) is rec) == (write == "pose")


def test_s7_untracked_image(cuda_device, stall):
    """An image this module holds no event for: the ``side.wait_stream`` branch."""
    enc.set_encoder_stream_min_work(0)
    gcn, g, x = _setup(cuda_device, **SMALL)
    a = _warm(gcn, g, x)
    enc._image_ready.clear()
    ev = stall.write(lambda: g.edata["pose"].mul_(1.25))
    c = _pair(lambda: gcn(g, x), 1, stall, ev)
    assert not torch.equal(c, a)
    assert not enc._image_ready


def test_s8_fresh_device_graph_per_step(cuda_device, stall):
    """The reference's eval loop: a new graph per step from ``frame_batch`` on robot poses written in
    place behind the stall, so ``mrp_frame_graph_build`` and its ``edata['pose']`` are queued behind it."""
    enc.set_encoder_stream_min_work(0)
    B, N, C, H = (SMALL[k] for k in "BNCH")
    gcn = _gcn(cuda_device, C)
    x = _feats(cuda_device, B, N, C, H)
    robots = torch.from_numpy(_robot_poses(B, N, 5)).to(cuda_device)
    _warm(gcn, m.frame_batch(robots), x)
    prev = None
    for _ in range(3):
        ev = stall.write(lambda: robots[..., :3].mul_(1.25), scale=2)
        out = _pair(lambda: gcn(m.frame_batch(robots), x), 1, stall, ev, scale=2)
        assert prev is None or not torch.equal(out, prev)
        prev = out


def test_s9_two_layer_stack_one_pose_tensor(cuda_device, stall):
    """Two encoders read one pose tensor; the second finds the first's cached event."""
    enc.set_encoder_stream_min_work(0)
    B, N, C, H = (SMALL[k] for k in "BNCH")
    torch.manual_seed(4)
    net = m.GCNStack(types.SimpleNamespace(feature_dim=C, gcn_layers=2, gcn_combine="residual")).to(cuda_device)
    g, x = _graph(cuda_device, B, N), _feats(cuda_device, B, N, C, H)
    a = _warm(net, g, x)
    ev = stall.write(lambda: g.edata["pose"].mul_(1.25), scale=2)
    c = _pair(lambda: net(g, x), 2, stall, ev, scale=2)
    assert not torch.equal(c, a)


def test_s10_more_than_64_readiness_events(cuda_device, stall):
    """70 distinct pose tensors in turn, then all again with pose 0 written behind a stall: the
    wholesale clear of ``_waited`` past 64 entries."""
    enc.set_encoder_stream_min_work(0)
    gcn, g, x = _setup(cuda_device, **SMALL)
    base = g.edata["pose"]
    poses = [base * (1.0 + 0.01 * i) for i in range(70)]
    _warm(gcn, g, x)

    def sweep():
        outs = []
        for p in poses:
            g.edata["pose"] = p
            outs.append(gcn(g, x))
        return outs

    first = _pair(sweep, 70)
    ev = stall.write(lambda: poses[0].mul_(1.25))
    state = {}

    def sweep_checked():
        outs = []
        for k, p in enumerate(poses):
            g.edata["pose"] = p
            outs.append(gcn(g, x))
            if k == 0:
                state.setdefault("pending", not ev.query())
        return outs

    second = _pair(sweep_checked, 70)
    assert state["pending"], stall.too_short()
    assert not torch.equal(second[0], first[0])
    assert all(torch.equal(a, b) for a, b in zip(first[1:], second[1:]))


def test_s11_caller_on_non_default_stream(cuda_device, stall):
    enc.set_encoder_stream_min_work(0)
    gcn, g, x = _setup(cuda_device, **SMALL)
    a = _warm(gcn, g, x)
    s = torch.cuda.Stream(device=cuda_device)
    s.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(s):
        ev = stall.write(lambda: g.edata["pose"].mul_(1.25))
        c = _pair(lambda: gcn(g, x), 1, stall, ev)
    torch.cuda.current_stream(cuda_device).wait_stream(s)
    torch.cuda.synchronize()
    assert not torch.equal(c, a)


def test_s12_priority_switch_keeps_the_waits(cuda_device, stall):
    """``set_encoder_stream_priority`` replaces the encoder stream: the new stream has passed none of
    the old stream's waits.  Stall, pose write, a forward (the new event recorded, stream A waits on
    it), the switch, a forward on the same pose version on stream B - all before the stall drains."""
    enc.set_encoder_stream_min_work(0)
    gcn, g, x = _setup(cuda_device, **SMALL)

    def two():
        enc.set_encoder_stream_priority(-1)
        first = gcn(g, x)
        enc.set_encoder_stream_priority(0)
        return [first, gcn(g, x)]

    # every switch hands the encoder a stream it has not used yet, whose first use costs the host far
    # more than a forward does: the stall is sized from the host time of this very sequence
    with torch.no_grad():
        two()
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        a = two()[1]
        host_ms = (time.perf_counter() - h0) * 1e3
    torch.cuda.synchronize()
    scale = max(4, math.ceil(10 * host_ms / (stall.reps * stall.rep_ms)))
    print(f"\n[S12] two forwards around a priority switch: {host_ms * 1e3:.0f} us host; {scale} stalls")
    ev = stall.write(lambda: g.edata["pose"].mul_(1.25), scale=scale)
    first, second = _pair(two, 2, stall, ev, scale=scale)
    assert torch.equal(first, second) and not torch.equal(first, a)


def test_s13_outputs_outlive_their_logits(cuda_device, stall):
    """8 back-to-back forwards behind a stall, each with its own features and poses (events cached, so
    the encoders run ahead during the stall); every z is dropped as its forward returns and must
    survive until its aggregation has read it (``record_stream``, the join)."""
    enc.set_encoder_stream_min_work(0)
    gcn, g, x = _setup(cuda_device, **SMALL)
    base = g.edata["pose"]
    poses = [base * (1.0 + 0.05 * i) for i in range(8)]
    xs = [x * (1.0 + 0.1 * i) for i in range(8)]

    def burst():
        outs = []
        for p, xi in zip(poses, xs):
            g.edata["pose"] = p
            outs.append(gcn(g, xi))
        return outs

    with torch.no_grad():
        burst()
    torch.cuda.synchronize()
    ev = stall.write(lambda: None, scale=8)
    outs = _pair(burst, 8, stall, ev, scale=8)
    assert len({o.data_ptr() for o in outs}) == 8
    assert not any(torch.equal(outs[0], o) for o in outs[1:])


@pytest.mark.parametrize("E,path", [(4096, "enc_stream"), (4095, "enc_inline")])
def test_s14_threshold_edge(cuda_device, E, path):
    """E C = 2^18 exactly takes the encoder stream at the default threshold, one edge fewer does not."""
    C = 64
    assert enc.set_encoder_stream_min_work(DEFAULT_MIN_WORK) == DEFAULT_MIN_WORK
    assert 4096 * C == DEFAULT_MIN_WORK
    torch.manual_seed(E)
    net = m.edge_encoder([C, C]).to(cuda_device)
    pose = torch.randn(E, 9, device=cuda_device) * 8
    before = dict(enc.PATH_COUNTS)
    with torch.no_grad():
        z_on = enc.edge_logits(net.layers, pose)
        mid = dict(enc.PATH_COUNTS)
        enc.set_encoder_stream(False)
        z_off = enc.edge_logits(net.layers, pose)
    other = "enc_inline" if path == "enc_stream" else "enc_stream"
    assert mid.get(path, 0) == before.get(path, 0) + 1 and mid.get(other, 0) == before.get(other, 0)
    assert enc.PATH_COUNTS["enc_inline"] == mid.get("enc_inline", 0) + 1
    assert enc.PATH_COUNTS["enc_stream"] == mid.get("enc_stream", 0)
    assert enc.PATH_COUNTS["split"] == before.get("split", 0) + 2
    torch.cuda.synchronize()
    assert torch.equal(z_on, z_off)


def test_s15_stream_capture_stays_inline(cuda_device):
    """Under ``torch.cuda.graph`` capture the layer records on one stream; the replay is bit-equal."""
    enc.set_encoder_stream_min_work(0)
    gcn, g, x = _setup(cuda_device, **SMALL)
    s0, i0 = _counts()
    eager = _warm(gcn, g, x)
    assert _counts() == (s0 + 1, i0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.stream(side):
        gcn(g, x)  # warm the allocator outside the capture
        torch.cuda.current_stream().synchronize()
        s1, i1 = _counts()
        with torch.cuda.graph(graph, stream=side):
            out = gcn(g, x)
        assert _counts() == (s1, i1 + 1), "the captured layer left the capturing stream"
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_s16_overlap_at_size(cuda_device):
    """B = 32, N = 8, C = 512, 16 x 16: ~270 MB of aggregation traffic per forward, long enough for
    the next forward's encoder to run beside it.  Two graphs and two feature tensors alternating, 8
    forwards back to back with nothing synchronising in between."""
    B, N, C, H = 32, 8, 512, 16
    gcn = _gcn(cuda_device, C, seed=0)
    gs = [_graph(cuda_device, B, N, seed) for seed in (11, 12)]
    xs = [_feats(cuda_device, B, N, C, H, seed) for seed in (11, 12)]
    assert not torch.equal(gs[0].edata["pose"], gs[1].edata["pose"])
    for g, x in zip(gs, xs):
        _warm(gcn, g, x)
    outs = _pair(lambda: [gcn(gs[k % 2], xs[k % 2]) for k in range(8)], 8)
    g, x = gs[0], xs[0]
    params = {"enc." + k: v.detach() for k, v in gcn.edge_encoder.named_parameters()}
    src, dst = (t.to(cuda_device).long() for t in g.edges())
    pose = g.edata["pose"]
    first = outs[0]
    del outs
    with torch.no_grad():
        f32 = stack_ref.aggregate(x, stack_ref.edge_gb(params, "enc.", pose), src, dst)
        p64 = {k: v.double() for k, v in params.items()}
        f64 = stack_ref.aggregate(x.double(), stack_ref.edge_gb(p64, "enc.", pose.double()), src, dst)
    ok, errs = stack_ref.within(first, f32, f64)
    assert ok, errs
    del f32, f64
    torch.cuda.empty_cache()
