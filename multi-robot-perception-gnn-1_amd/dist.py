"""Multi-GPU data parallelism for the GCN path: one process per GPU, RCCL over xGMI.

Replaces ``torch.nn.DataParallel(model, device_ids=[0, 1])`` (``dgl/training.py:324-325``), the
reference's only parallelism (single process, and it cannot scatter a DGLGraph).

* The graphs of a batch are independent (``dgl.batch`` of per-frame graphs), so the forward and
  the aggregation need no communication: :func:`shard_range` gives each rank a contiguous range
  of graphs (weak scaling when every rank keeps its own batch).
* Parameters are replicated; the only collective is the gradient all-reduce.
  :class:`GradAllReducer` packs gradients into flat buckets in reverse registration order (the
  order backward produces them), launches each bucket's ``all_reduce`` asynchronously from a
  post-accumulate-grad hook as soon as its last gradient lands (overlapping the rest of
  backward), and averages on :meth:`GradAllReducer.synchronize`.  Buckets default to 32 MiB:
  large enough that each ring step over one ~153 GB/s xGMI link is bandwidth- rather than
  latency-bound, few enough that the per-layer edge-encoder (2C^2+12C) and 1x1 compress
  (2C^2+C) gradients of a GCN layer land in one or two buckets.

Averaging: each rank's loss is normally a mean over its own graphs, so with uneven shards
(``shard_range`` of B graphs over P ranks when P does not divide B) the full-batch gradient is
``sum_r (n_r / N) g_r``, not ``(1/P) sum_r g_r``.  :meth:`GradAllReducer.set_local_count` gives the
reducer ``n_r`` (one tiny all-reduce finds ``N``); every bucket is then reduced as ``sum_r s_r g_r``
with ``s_r = n_r / N``.  Without it the reducer assumes equal shards and uses ``s_r = 1/P``.  On RCCL
the scale rides inside the collective (a pre-multiplied sum, ``ncclRedOpCreatePreMulSum``): no pass
over the bucket before it; backends without one (gloo) scale the bucket in place first.
One backward per :meth:`GradAllReducer.synchronize`: a gradient that lands again after its
bucket's all-reduce was launched (gradient accumulation over several backwards) raises instead
of silently reducing a partial sum.
"""
from __future__ import annotations

import os
import weakref
from typing import Iterable, List, Optional, Tuple

import torch
import torch.distributed as dist


def env_rank_world() -> Tuple[int, int, int]:
    """(rank, world_size, local_rank) from the torchrun environment (defaults 0, 1, 0)."""
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", str(rank)))
    return rank, world, local


def shard_range(num_items: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous [lo, hi) share of ``num_items`` for ``rank`` (sizes differ by at most one)."""
    if world <= 0 or not 0 <= rank < world:
        raise ValueError(f"bad rank {rank} / world {world}")
    base, extra = divmod(num_items, world)
    lo = rank * base + min(rank, extra)
    hi = lo + base + (1 if rank < extra else 0)
    return lo, hi


def shard(items, rank: int, world: int):
    lo, hi = shard_range(len(items), rank, world)
    return items[lo:hi]


def shard_graph(g, rank: int, world: int):
    """This rank's share of a batched graph (``dgl.batch`` of frames): the contiguous range of
    graphs ``shard_range(g.batch_size, rank, world)`` as a batched graph of its own (node and edge
    ids renumbered from 0, every node/edge feature sliced without a copy).  Returns
    ``(sub_graph, (lo, hi))``.  Replaces what ``DataParallel`` (``dgl/training.py:324-325``) could
    not do: scatter a graph batch."""
    import numpy as np

    from .graph import RobotGraph
    lo, hi = shard_range(g.batch_size, rank, world)
    if g._masked():
        raise ValueError("shard_graph: a graph with an edge_active mask (range-limited / drop-out frames) "
                         "cannot be sharded yet; shard the poses and build each rank's frames")
    bnn = [int(v) for v in g.batch_num_nodes().tolist()]
    bne = [int(v) for v in g.batch_num_edges().tolist()]
    noff = np.concatenate([[0], np.cumsum(bnn)]).astype(np.int64)
    eoff = np.concatenate([[0], np.cumsum(bne)]).astype(np.int64)
    n0, n1, e0, e1 = (int(v) for v in (noff[lo], noff[hi], eoff[lo], eoff[hi]))
    src, dst = g.edges()
    sub = RobotGraph(src[e0:e1] - n0, dst[e0:e1] - n0, num_nodes=n1 - n0, batch_num_nodes=bnn[lo:hi],
                     batch_num_edges=bne[lo:hi])
    for k, v in g.ndata.items():
        sub.ndata[k] = v[n0:n1]
    for k, v in g.edata.items():
        sub.edata[k] = v[e0:e1]
    return sub, (lo, hi)


#: live reducers, consulted by the backward kernels' output allocation (:func:`grad_out_like`)
_ACTIVE = weakref.WeakSet()


def grad_out_like(param: torch.Tensor) -> Optional[torch.Tensor]:
    """Where a backward kernel should write ``param``'s gradient: a fresh view of the slot a live,
    ARMED :class:`GradAllReducer` keeps for it in its flat bucket, or None (allocate normally).
    Autograd's AccumulateGrad then adopts the returned tensor as ``param.grad`` without a copy (a
    freshly made, unshared tensor with the parameter's layout), so the gradient is already in the
    all-reduce buffer.  Handed out once per step, only while ``param.grad`` is None (a gradient that
    accumulates onto an existing one is written elsewhere and added by autograd as usual), only for
    fp32 parameters (the HIP kernels write fp32), and only between :meth:`GradAllReducer.arm` (or
    ``set_local_count``) and ``synchronize()`` — a backward the reducer is not meant to see (e.g.
    ``torch.autograd.grad``) gets ordinary tensors.  A caller whose kernel then declines the shape
    gives the slot back with :func:`release_grad_out`."""
    for red in list(_ACTIVE):
        v = red.claim(param)
        if v is not None:
            return v
    return None


def release_grad_out(param: Optional[torch.Tensor], view: Optional[torch.Tensor]) -> None:
    """Undo :func:`grad_out_like` for a slot that was not written (the kernel declined the shape):
    the gradient computed elsewhere then takes the hook's copy path as usual."""
    if param is None or view is None:
        return
    for red in list(_ACTIVE):
        red.release(param, view)


class GradAllReducer:
    """Bucketed, backward-overlapped gradient averaging over a process group.

    Every bucket is one preallocated flat buffer and every parameter's ``.grad`` is a view into it
    (the gradient-as-bucket-view layout): the all-reduce runs in place on the gradients themselves,
    with no per-step concatenation and no copy back.  A gradient that autograd allocated on its
    own (``zero_grad(set_to_none=True)`` and an op that did not write through :func:`grad_out_like`)
    is copied into its slot once, in the hook; with ``set_to_none=False`` autograd accumulates
    straight into the views.  ``copies`` counts those hook copies (tests).

    Slots start at multiples of :attr:`SLOT_ALIGN` bytes (the HIP kernels that write gradients in
    place take 16-byte aligned pointers; parameters of any size may precede them in a bucket).
    Kernels are handed slots only while the reducer is armed (:meth:`arm`, or ``set_local_count``),
    until ``synchronize()``; arming re-keys the slot lookup on the parameters' current storage, so
    a model moved in place after the reducer was built keeps the zero-copy path, and a parameter
    that changed device or dtype raises (its bucket lives on the old device / dtype)."""

    SLOT_ALIGN = 256

    def __init__(self, params: Iterable[torch.nn.Parameter], bucket_bytes: int = 32 << 20,
                 group: Optional[dist.ProcessGroup] = None, auto_arm: bool = False):
        self.group = group
        #: re-arm in every ``synchronize()`` (for callers that never call :meth:`arm` themselves): the
        #: kernels then keep writing gradients into the buckets step after step
        self.auto_arm = bool(auto_arm)
        self._was_armed = False
        self._warned_unarmed = False
        self.world = dist.get_world_size(group)
        params = [p for p in params if p.requires_grad]
        self.buckets: List[List[torch.nn.Parameter]] = []
        cur, size = [], 0
        for p in reversed(params):  # backward produces gradients roughly in reverse order
            nbytes = p.numel() * p.element_size()
            if cur and (size + nbytes > bucket_bytes or p.dtype != cur[0].dtype or p.device != cur[0].device):
                self.buckets.append(cur)
                cur, size = [], 0
            cur.append(p)
            size += nbytes
        if cur:
            self.buckets.append(cur)
        self._slot = {}    # id(p) -> (bucket, offset, numel)
        self._by_ptr = {}  # parameter storage address -> parameter (grad_out_like lookups)
        self._flat: List[torch.Tensor] = []
        for bi, b in enumerate(self.buckets):
            off = 0
            align = max(1, self.SLOT_ALIGN // b[0].element_size())
            for p in b:
                off = -(-off // align) * align  # every slot starts SLOT_ALIGN-byte aligned
                self._slot[id(p)] = (bi, off, p.numel())
                off += p.numel()
            self._flat.append(torch.zeros(max(off, 1), dtype=b[0].dtype, device=b[0].device))
        self._params = [p for b in self.buckets for p in b]
        self._bucket_of = {k: v[0] for k, v in self._slot.items()}
        self._armed = False
        self._rekey()
        self._scale = 1.0 / self.world
        self._empty = False  # this rank holds no graphs this step (set_local_count(0))
        self.copies = 0
        self.scaled_passes_skipped = 0  # buckets whose scale rode inside the collective (tests)
        self._ops = {}  # scale -> RCCL pre-multiplied-sum op
        #: (event, bucket) in the order they happen during a backward: ("grad", b) when a parameter's
        #: gradient lands, ("launch", b) when a bucket's all-reduce is started; ``last_events`` is the
        #: record of the last synchronized step — the evidence that the all-reduces overlap backward
        #: (tests/test_dist_gloo.py)
        self.events: List[Tuple[str, int]] = []
        self.last_events: List[Tuple[str, int]] = []
        self._hooks = [p.register_post_accumulate_grad_hook(self._on_grad) for p in params]
        self.reset()
        _ACTIVE.add(self)

    def set_local_count(self, n_local: int) -> float:
        """This rank holds ``n_local`` of the step's graphs (its loss a mean over them): scale its
        gradients by ``n_local / N`` (N = the sum over ranks) so the reduced gradient is the
        full-batch mean even for uneven shards.  Call before backward; returns the scale."""
        t = torch.tensor([float(n_local)], dtype=torch.float64,
                         device=self._device() if dist.get_backend(self.group) == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        total = float(t.item())
        self._scale = float(n_local) / total if total > 0 else 0.0
        # an empty shard (more ranks than graphs, e.g. a DataLoader's short last batch) has a mean loss
        # of 0/0 = NaN: its contribution must be exact zeros, since 0 * NaN would poison every rank
        self._empty = n_local == 0
        self.arm()
        return self._scale

    def arm(self) -> "GradAllReducer":
        """Hand bucket slots to the backward kernels (:func:`grad_out_like`) until ``synchronize()``.
        Re-keys the lookup on the parameters' current storage; raises if a parameter moved to another
        device or dtype after the reducer was built.  Returns self (``reducer.arm(); loss.backward()``)."""
        self._rekey()
        self._armed = True
        self._was_armed = True
        return self

    def _rekey(self) -> None:
        by_ptr = {}
        for p in self._params:
            flat = self._flat[self._bucket_of[id(p)]]
            if p.device != flat.device or p.dtype != flat.dtype:
                raise RuntimeError(f"GradAllReducer: a parameter is now {p.dtype} on {p.device} but its bucket is "
                                   f"{flat.dtype} on {flat.device} (moved or re-cast after the reducer was built); "
                                   "build a new GradAllReducer")
            by_ptr[(p.data_ptr(), p.device)] = p
        self._by_ptr = by_ptr

    def _device(self):
        for b in self.buckets:
            return b[0].device
        return torch.device("cpu")

    def view(self, p: torch.Tensor) -> torch.Tensor:
        """``p``'s slot in its bucket's flat buffer, shaped like ``p`` (a new view object)."""
        bi, off, n = self._slot[id(p)]
        return self._flat[bi][off:off + n].view_as(p)

    def claim(self, t: torch.Tensor) -> Optional[torch.Tensor]:
        """:func:`grad_out_like` for this reducer's parameters (see there)."""
        if not self._armed:
            return None
        p = self._by_ptr.get((t.data_ptr(), t.device))
        if p is None or p.shape != t.shape or p.dtype != torch.float32 or t.dtype != torch.float32 \
                or not p.is_contiguous() or p.grad is not None or id(p) in self._handed \
                or self._work[self._bucket_of[id(p)]] is not None:
            return None
        self._handed.add(id(p))
        return self.view(p)

    def release(self, t: torch.Tensor, view: torch.Tensor) -> None:
        """:func:`release_grad_out`: give back a slot handed out for ``t`` (matched by the view)."""
        p = self._by_ptr.get((t.data_ptr(), t.device))
        if p is not None and id(p) in self._handed and view.data_ptr() == self.view(p).data_ptr():
            self._handed.discard(id(p))

    def reset(self) -> None:
        self.events = []
        self._pending = [len(b) for b in self.buckets]
        self._work = [None] * len(self.buckets)
        self._landed = set()
        self._handed = set()

    def _adopt(self, p: torch.Tensor) -> None:
        """Make ``p.grad`` its bucket slot (copying a gradient that lives elsewhere; zeros if none)."""
        v = self.view(p)
        g = p.grad
        if g is None:
            v.zero_()
        elif g.data_ptr() != v.data_ptr():
            if not self._armed and self._was_armed and not self._warned_unarmed:
                # armed once, not since the last synchronize(): the HIP kernels' gradients now take this
                # copy instead of being written in place — correct, but a hidden pass per gradient
                import warnings
                warnings.warn("GradAllReducer: a gradient landed while the reducer was not armed (call arm() or "
                              "set_local_count() before every backward, or build it with auto_arm=True); it is "
                              "copied into its bucket instead of being written there by the kernel", stacklevel=2)
                self._warned_unarmed = True
            v.copy_(g)
            self.copies += 1
        else:
            return
        p.grad = v

    def _on_grad(self, p: torch.Tensor) -> None:
        bi = self._bucket_of[id(p)]
        if self._work[bi] is not None:
            raise RuntimeError("GradAllReducer: a gradient landed after its bucket's all-reduce was launched "
                               "(more than one backward before synchronize()); call synchronize() after "
                               "every backward")
        self.events.append(("grad", bi))
        self._adopt(p)
        self._landed.add(id(p))
        self._pending[bi] -= 1
        if self._pending[bi] == 0:
            self._launch(bi)

    def _premul(self) -> bool:
        """The collective applies the scale itself (RCCL's pre-multiplied sum)."""
        return dist.get_backend(self.group) == "nccl" and hasattr(dist, "_make_nccl_premul_sum")

    def _reduce_op(self, flat: torch.Tensor):
        """The reduction of one bucket: ``sum_r s_r g_r`` with this rank's scale ``s_r`` (n_r / N, or 1/P).
        RCCL: a pre-multiplied sum (the scale applied inside the collective's own pass; no read and
        write of the bucket before it).  Other backends: the bucket scaled in place, then a SUM."""
        if self._premul():
            op = self._ops.get(self._scale)
            if op is None:
                op = self._ops[self._scale] = dist._make_nccl_premul_sum(self._scale)
            self.scaled_passes_skipped += 1
            return op
        flat.mul_(self._scale)
        return dist.ReduceOp.SUM

    def _launch(self, bi: int) -> None:
        for p in self.buckets[bi]:
            if id(p) not in self._landed:  # no gradient this step (an unused parameter)
                self._adopt(p)
        flat = self._flat[bi]
        if self._empty:
            # an empty shard contributes exact zeros (its 0/0 mean loss is NaN: 0 * NaN would poison the sum)
            flat.zero_()
            op = dist.ReduceOp.SUM
        else:
            op = self._reduce_op(flat)
        self.events.append(("launch", bi))
        self._work[bi] = dist.all_reduce(flat, op=op, group=self.group, async_op=True)

    def synchronize(self) -> None:
        """Wait for every bucket (launching any whose hooks did not all fire, e.g. unused
        parameters); the averaged gradients are then in every ``p.grad`` (views of the buckets)."""
        for bi in range(len(self.buckets)):
            if self._work[bi] is None:
                self._launch(bi)
        for bi in range(len(self.buckets)):
            self._work[bi].wait()
        self.last_events = self.events
        self.reset()
        self._armed = False
        if self.auto_arm:
            self.arm()

    def remove(self) -> None:
        for h in self._hooks:
            h.remove()
        self._hooks = []
        _ACTIVE.discard(self)
