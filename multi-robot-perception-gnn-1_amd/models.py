"""Drop-in model classes for the GCN hot path, with the reference's API and ``state_dict`` keys.

Mirrors ``dgl/model/models.py``:

* :class:`edge_encoder`  — ``models.py:142-155``: ``Linear(9,C) -> ReLU -> Linear(C,2C) -> Sigmoid``;
  keys ``layers.0.weight``, ``layers.0.bias``, ``layers.2.weight``, ``layers.2.bias``.
* :class:`GCN`           — ``models.py:213-226``: ``forward(g)`` (the reference call, ``models.py:181``)
  and ``forward(g, feats)`` (the north-star signature).  Aggregation runs in the HIP kernel.
* :class:`GCNBlock`      — the GCN stacking of ``multi_view_dgl_model.forward`` (``models.py:180-189``):
  ``gcn1 -> cat -> [conv1] -> [gcn2 -> cat -> conv2]``, keys ``gcn1.*``, ``conv1.*``, ``gcn2.*``, ``conv2.*``;
  the 1x1 convs run on the matrix-core compress kernels without the concatenation (``compress.py``).
* :class:`GCNStack`      — the same for k layers (``opt.gcn_layers``; BASELINE configs[4] runs 3) and
  the residual (``dgl_models.py:36-37``) / initial-feature-mix combinations, each fused into the
  aggregation kernel's epilogue.
* :class:`multi_view_dgl_model` — ``models.py:157-205`` with the CNN encoder/decoder supplied by the
  caller (they are torchvision/dense-conv code outside the hot path), so a reference
  ``encoder``/``decoder`` instance can be plugged in unchanged.

Semantics switch ``opt.gcn_return``:

* ``'aggregate'`` (default): return the FiLM-mean aggregate — what ``update_all`` computes and
  what the scratch variants return (``dgl/model/dgl_models.py:61,127,189``).
* ``'input'``: bit-faithful to ``models.py:226``, which returns ``g.ndata['image']`` (the input)
  because ``node_udf`` writes ``'images'``; the aggregate is then dead work and is skipped.

``opt.gcn_mode``: ``'film_mean'`` (default, ``models.py:223``), ``'copy_mean'`` (the commented-out
``fn.copy_u`` variant, ``models.py:225``), ``'film_sum'``, ``'film_max'`` (``node_udf`` =
``torch.max(mailbox, 1)``: :func:`aggregate.film_max`, every in-degree <= 16), ``'film_attn'`` (per-location
attention over the messages: :func:`aggregate.film_attn`, every in-degree <= 16; ``opt.gcn_attn_scale``
sets the score scale, default ``None``: 1/sqrt(C)), ``'film_wattn'`` (the same attention over what each sender's
confidence map delivered: :func:`aggregate.film_wattn`, with the maps of ``opt.gcn_confidence`` or ``weights=``;
with neither it is ``'film_attn'`` itself, same kernels, same bits).  ``opt.gcn_attn_heads = H`` (absent or 1:
nothing changes) makes both attention modes multi-head: H independent channel groups of C/H channels, each with
its own scores and softmax, in one launch (``heads=`` of :func:`aggregate.film_attn`; the default scale becomes
1/sqrt(C/H)).  It adds no parameter; a value that is not a positive int dividing ``feature_dim``, or any value
but 1 under another ``gcn_mode``, is a ``ValueError`` when the module is built.

``opt.gcn_message_dtype``: ``None`` (default: nothing changes), ``'fp8_e4m3'`` or ``'fp8_e5m2'`` — the
feature maps every GCN layer aggregates are quantised per node to OCP FP8, as each robot would transmit them
over an 8-bit link, with one scale per (node, channel) (``opt.gcn_message_scale='channel'``, the default) or
per node (``'node'``); the layer's own-feature terms (cat half, residual, compress input) use the
unquantised features.  In a single-GPU simulation the quantise pass costs more than the aggregation saves:
the option exists to evaluate and train models for 8-bit links.  The saving belongs to a receiver that is
handed FP8 buffers (:func:`aggregate.film_mean_q`).  See :meth:`GCN._aggregate_q`.  That receiver's layer is
:meth:`GCN.forward_received` / :meth:`GCN.forward_cat_received`: own features at full precision, received codes,
scales and (``film_wattn``) confidence maps in, for every ``gcn_mode`` — the max and attention reducers included,
which ``gcn_message_dtype`` itself still refuses.

``opt.gcn_confidence`` (default off: nothing changes, no new parameters): every GCN layer owns a 1x1 head
``confidence = nn.Conv2d(C, 1, 1)``; each sender attaches ``w = sigmoid(confidence(x))`` to its feature map and
the receiver averages, pixel by pixel, over what was delivered (:func:`aggregate.film_wmean`; Where2comm-style
sparse messaging).  ``opt.gcn_confidence_threshold = tau`` hard-gates the map (``w < tau`` is not transmitted:
0; the gradient flows through the kept values).  Every ``GCN`` method also takes ``weights=`` to supply a map
(N, H, W) directly.  Modes ``film_mean``, ``film_sum`` and ``copy_mean`` average (:func:`aggregate.film_wmean`);
``film_wattn`` attends over what was delivered (:func:`aggregate.film_wattn`); combined with ``film_max``,
``film_attn`` or ``gcn_message_dtype`` a ``ValueError`` is raised when the module is built.
"""
from __future__ import annotations

import warnings

import torch
import torch.nn as nn

from .aggregate import (film_mean_fq, film_mean_q, film_mean_q_forward_into, quantize_features)
from .aggregate import film_attn_q_forward_into, film_max_q_forward_into, film_wattn_q_forward_into
from .aggregate import film_wmean, film_wmean_cat, film_wmean_mix, film_wmean_residual
from .aggregate import film_wattn, film_wattn_cat, film_wattn_mix, film_wattn_residual
from .aggregate import (film_attn, film_attn_cat, film_attn_mix, film_attn_residual, film_max, film_max_cat,
                        film_max_mix, film_max_residual, film_mean, film_mean_cat, film_mean_mix, film_mean_residual)
from .compress import CompressFunction, compress_1x1, compress_path, film_compress, film_compress_supported
from .encoder import edge_logits


def clear_packed_weights() -> None:
    """Drop every cached split-bf16 weight image (edge encoder and 1x1 compress).  The images are
    keyed by a weight's data pointer and autograd version, which in-place optimizer steps bump;
    writes that bypass the version counter (``param.data = t``, ``.data`` copies, collectives
    writing into parameters) need this call.  The modules below call it themselves when they are
    moved or cast (``.to()``, ``.cuda()``, ``.float()``: ``nn.Module._apply``) and after
    ``load_state_dict``."""
    from . import compress, encoder
    compress.clear_packed_weights()
    encoder.clear_packed_weights()


class _PackedImages:
    """Mixin: invalidate the packed weight images when parameters are replaced wholesale."""

    def _apply(self, fn, *args, **kwargs):
        clear_packed_weights()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        clear_packed_weights()
        return out


class edge_encoder(_PackedImages, nn.Module):  # noqa: N801  (reference class name)
    """FiLM parameter generator, ``dgl/model/models.py:142-155``."""

    def __init__(self, layers_dim):
        super().__init__()
        self.layers_dim = layers_dim
        self.layers = nn.Sequential(
            nn.Linear(9, layers_dim[0]),
            nn.ReLU(),
            nn.Linear(layers_dim[0], layers_dim[1] * 2),
            nn.Sigmoid(),
        )

    def logits(self, edge: torch.Tensor) -> torch.Tensor:
        """Pre-sigmoid FiLM parameters z, (E, C, 2) interleaved.  On the GPU (``encoder.edge_logits``):
        one split-bf16 matrix-core kernel for both Linears (``mrp_edge_encoder_fwd_split``); with a
        gradient wanted the same kernel also keeps h^T for a backward on the split-bf16 GEMM kernels.
        The sigmoid is left to the aggregation kernel (``MRP_AGG_GB_LOGITS``)."""
        if edge.is_cuda:
            z = edge_logits(self.layers, edge)
        else:
            z = self.layers[2](self.layers[1](self.layers[0](edge.float())))
        return z.view(-1, self.layers_dim[1], 2)

    def film_params(self, edge: torch.Tensor) -> torch.Tensor:
        """Interleaved gamma/beta = sigmoid(z), (E, C, 2) (``models.py:153-154``)."""
        return torch.sigmoid(self.logits(edge))

    def forward(self, edge: torch.Tensor):
        """Reference return value: gamma, beta as (E, C, 1, 1) views (``models.py:152-155``)."""
        gb = self.film_params(edge)
        return gb[:, :, 0].unsqueeze(-1).unsqueeze(-1), gb[:, :, 1].unsqueeze(-1).unsqueeze(-1)


def _opt(opt, name, default):
    return getattr(opt, name, default) if opt is not None else default


#: ``opt.gcn_message_dtype`` -> the FP8 format of the aggregated messages (``aggregate.QUANT_FORMATS``)
MESSAGE_DTYPES = {None: None, "fp8_e4m3": "e4m3", "fp8_e5m2": "e5m2"}
MESSAGE_SCALES = ("channel", "node")


def message_format(opt):
    """(FP8 format or None, scale granularity) from ``opt.gcn_message_dtype`` / ``opt.gcn_message_scale``;
    an unknown value is a ``ValueError`` (raised when a module is built)."""
    dtype = _opt(opt, "gcn_message_dtype", None)
    per = _opt(opt, "gcn_message_scale", "channel")
    if dtype not in MESSAGE_DTYPES:
        raise ValueError(f"gcn_message_dtype must be one of {tuple(MESSAGE_DTYPES)}, got {dtype!r}")
    if per not in MESSAGE_SCALES:
        raise ValueError(f"gcn_message_scale must be one of {MESSAGE_SCALES}, got {per!r}")
    return MESSAGE_DTYPES[dtype], per


def confidence_options(opt):
    """(head?, threshold or None) from ``opt.gcn_confidence`` / ``opt.gcn_confidence_threshold``; a combination
    the weighted aggregation does not provide is a ``ValueError`` (raised when a module is built)."""
    on = bool(_opt(opt, "gcn_confidence", False))
    tau = _opt(opt, "gcn_confidence_threshold", None)
    if on:
        _check_weighted(opt)
    if tau is not None and not 0.0 <= float(tau) <= 1.0:
        raise ValueError(f"gcn_confidence_threshold must be in [0, 1], got {tau!r}")
    return on, (None if tau is None else float(tau))


def _check_weighted(opt) -> None:
    mode = _opt(opt, "gcn_mode", "film_mean")
    if mode in ("film_max", "film_attn"):
        raise ValueError(f"confidence-weighted aggregation is not provided for gcn_mode={mode!r} "
                         "(film_mean, film_sum, copy_mean, film_wattn)")
    if _opt(opt, "gcn_message_dtype", None) is not None:
        raise ValueError("confidence-weighted aggregation is not provided together with gcn_message_dtype")


def attn_heads(opt) -> int:
    """``opt.gcn_attn_heads`` (absent: 1), checked: a positive int that divides ``opt.feature_dim``, and 1 unless
    ``opt.gcn_mode`` is ``'film_attn'`` or ``'film_wattn'`` (``ValueError``, raised when a module is built)."""
    heads = _opt(opt, "gcn_attn_heads", 1)
    if isinstance(heads, bool) or not isinstance(heads, int) or heads < 1:
        raise ValueError(f"gcn_attn_heads must be a positive int, got {heads!r}")
    if heads == 1:
        return 1
    mode = _opt(opt, "gcn_mode", "film_mean")
    if mode not in ("film_attn", "film_wattn"):
        raise ValueError(f"gcn_attn_heads={heads} is not provided for gcn_mode={mode!r} (film_attn, film_wattn)")
    if opt.feature_dim % heads:
        raise ValueError(f"gcn_attn_heads must divide feature_dim: {opt.feature_dim} % {heads} != 0")
    return heads


#: ``gcn_return`` given to a GCN unpickled from a reference checkpoint whose ``opt`` has none (see
#: :meth:`GCN.__setstate__`); ``compat.reference_class_path(gcn_return=...)`` sets it.
UNPICKLED_GCN_RETURN = "input"


class GCN(_PackedImages, nn.Module):
    """FiLM-mean graph convolution over per-frame robot graphs, ``dgl/model/models.py:213-226``."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        fmt = message_format(opt)[0]  # an unknown gcn_message_dtype / gcn_message_scale: ValueError here
        if fmt is not None and _opt(opt, "gcn_mode", "film_mean") == "film_wattn":
            raise ValueError("gcn_message_dtype is not provided for gcn_mode='film_wattn' "
                             "(film_mean, film_sum, copy_mean)")
        attn_heads(opt)  # a gcn_attn_heads the attention modes cannot take: ValueError here
        self.edge_encoder = edge_encoder(layers_dim=[opt.feature_dim, opt.feature_dim])
        if confidence_options(opt)[0]:  # a forbidden combination: ValueError here
            self.confidence = nn.Conv2d(opt.feature_dim, 1, kernel_size=1)
        # marks a GCN this framework built: its pickles (deepcopy, torch.save of the whole model as the
        # reference's training.py:345-355 does) keep computing the aggregate
        self.gcn_return_default = "aggregate"

    def __setstate__(self, state):
        """Unpickling a checkpoint the reference wrote (``torch.save({'model': model})``,
        ``dgl/training.py:345-355``): its ``opt`` has no ``gcn_return``, and the reference forward
        it was trained and evaluated with returns its input (``models.py:226``).  Keep that
        behaviour so ``eval.py`` reproduces the reference's outputs, and say so once.  A GCN built
        here carries ``gcn_return_default`` in its state and keeps it."""
        super().__setstate__(state)
        if self.__dict__.get("opt") is not None and not hasattr(self.opt, "gcn_return") \
                and "gcn_return_default" not in self.__dict__:
            self.gcn_return_default = UNPICKLED_GCN_RETURN
            if UNPICKLED_GCN_RETURN == "input":
                warnings.warn("mrp_gnn: GCN unpickled from a checkpoint without opt.gcn_return: returning the "
                              "input as the reference's GCN.forward does (models.py:226); set "
                              "opt.gcn_return='aggregate' for the message-passing result", stacklevel=2)

    def _return_mode(self) -> str:
        return _opt(self.opt, "gcn_return", self.__dict__.get("gcn_return_default", "aggregate"))

    def _attn_scale(self):
        """``opt.gcn_attn_scale``: the score scale of ``gcn_mode='film_attn'`` (None: 1/sqrt(C))."""
        return _opt(self.opt, "gcn_attn_scale", None)

    def _attn_heads(self) -> int:
        """``opt.gcn_attn_heads``: the heads of ``gcn_mode='film_attn'`` / ``'film_wattn'`` (absent: 1)."""
        return attn_heads(self.opt)

    def confidence_map(self, x: torch.Tensor) -> torch.Tensor:
        """The sender maps w (N, 1, H, W) fp32 of feature maps x: ``sigmoid(confidence(x))``, hard-gated by
        ``opt.gcn_confidence_threshold`` (values below it become 0; the kept ones carry the gradient)."""
        if "confidence" not in self._modules:
            raise ValueError("GCN.confidence_map needs opt.gcn_confidence (the module has no confidence head)")
        w = torch.sigmoid(self.confidence(x.to(self.confidence.weight.dtype))).float()
        tau = confidence_options(self.opt)[1]
        if tau is not None:
            w = torch.where(w >= tau, w, torch.zeros_like(w))
        return w.contiguous()

    def _weights(self, x, weights):
        """The sender maps of this call: ``weights=`` if given, else the head's, else None (unweighted)."""
        if weights is not None:
            _check_weighted(self.opt)
            return weights
        return self.confidence_map(x) if "confidence" in self._modules else None

    def _wattn(self) -> bool:
        """``opt.gcn_mode == 'film_wattn'``: sender maps gate the attention (:func:`aggregate.film_wattn`);
        without maps every branch below takes ``film_attn``'s route."""
        return _opt(self.opt, "gcn_mode", "film_mean") == "film_wattn"

    def _wattn_args(self, g, x, w):
        """The leading arguments of ``film_wattn*``: features, logits, maps, graph."""
        return x, self.edge_encoder.logits(g.edata["pose"]), w, g.csr(x.device)

    def _wmean_args(self, g, x):
        """(gb or logits, csr, mode, logits?) of the weighted aggregation for ``opt.gcn_mode``; ``copy_mean`` is
        gamma = 1, beta = 0, materialised."""
        mode = _opt(self.opt, "gcn_mode", "film_mean")
        csr = g.csr(x.device)
        if mode == "copy_mean":
            gb = torch.zeros((csr.num_edges, x.shape[1], 2), device=x.device, dtype=torch.float32)
            gb[:, :, 0] = 1.0
            return gb, csr, "mean", False
        return self.edge_encoder.logits(g.edata["pose"]), csr, ("sum" if mode == "film_sum" else "mean"), True

    def _aggregate_q(self, g, x, fmt, per, x0=None, agg_scale=1.0, x0_scale=0.0, out=None):
        """``agg_scale * aggregate(quantised x) + x0_scale * x0`` for ``opt.gcn_message_dtype``, in x's
        dtype.  Grad mode off and CUDA features: ``quantize_features`` + the native FP8 kernel
        (``film_mean_q``; into ``out`` if given).  Grad mode on: the fake-quant route ``film_mean_fq`` on the
        fp32 kernels, straight-through to x.  Both return the same bits.  In a single-GPU simulation the
        quantise pass costs more than the aggregation saves; the option is for evaluating and training
        models for 8-bit links, and the saving belongs to a receiver that is handed FP8 buffers."""
        mode = _opt(self.opt, "gcn_mode", "film_mean")
        if mode in ("film_max", "film_attn", "film_wattn"):
            raise ValueError(f"gcn_message_dtype is not provided for gcn_mode={mode!r} (film_mean, film_sum, copy_mean)")
        if self._return_mode() == "input":
            raise ValueError("gcn_message_dtype with gcn_return='input': no message is aggregated")
        csr = g.csr(x.device)
        z = None if mode == "copy_mean" else self.edge_encoder.logits(g.edata["pose"])
        if x.is_cuda and not torch.is_grad_enabled():
            xq, s = quantize_features(x, fmt, per)
            if out is None:
                return film_mean_q(xq, s, z, csr, mode, logits=True, out_dtype=x.dtype, x0=x0, agg_scale=agg_scale,
                                   x0_scale=x0_scale)
            return film_mean_q_forward_into(xq, s, z, csr, out, mode, logits=True, x0=x0, agg_scale=agg_scale,
                                            x0_scale=x0_scale)
        a = film_mean_fq(x, z, csr, fmt, per, mode, logits=True, x0=x0, agg_scale=agg_scale, x0_scale=x0_scale)
        return a if out is None else out.copy_(a)

    def forward(self, g, feats: torch.Tensor = None, weights: torch.Tensor = None) -> torch.Tensor:
        """The aggregate of ``feats`` (fp32, bf16 or fp16; returned in that dtype — the encoder's logits
        stay fp32 and the aggregation's arithmetic is fp32 either way).  ``weights`` (N, H, W) fp32, or the
        module's confidence head: the confidence-weighted aggregate (module docstring)."""
        x = g.ndata["image"] if feats is None else feats
        w = self._weights(x, weights)
        fmt, per = message_format(self.opt)
        if fmt is not None:
            return self._aggregate_q(g, x, fmt, per)
        if self._return_mode() == "input":
            return x  # models.py:226 returns the input; update_all's result is never read
        if w is not None:
            if self._wattn():
                return film_wattn(*self._wattn_args(g, x, w), logits=True, scale=self._attn_scale(), heads=self._attn_heads())
            gb, csr, wmode, logits = self._wmean_args(g, x)
            return film_wmean(x, gb, w, csr, wmode, logits=logits)
        mode = _opt(self.opt, "gcn_mode", "film_mean")
        if mode == "copy_mean":
            return film_mean(x, None, g.csr(x.device), mode)
        # logits in, sigmoid applied inside the aggregation kernel
        z = self.edge_encoder.logits(g.edata["pose"])
        if mode == "film_max":  # the max reducer: an operator of its own (aggregate.film_max)
            return film_max(x, z, g.csr(x.device), logits=True)
        if mode in ("film_attn", "film_wattn"):  # per-location attention over the messages (aggregate.film_attn)
            return film_attn(x, z, g.csr(x.device), logits=True, scale=self._attn_scale(), heads=self._attn_heads())
        return film_mean(x, z, g.csr(x.device), mode, logits=True)

    def forward_cat(self, g, feats: torch.Tensor = None, weights: torch.Tensor = None) -> torch.Tensor:
        """``torch.cat((feats, self(g, feats)), 1)`` (``models.py:181-182``) with the aggregate written
        straight into the concatenation buffer (and the backward fused likewise)."""
        x = g.ndata["image"] if feats is None else feats
        w = self._weights(x, weights)  # explicit maps with an unsupported option: ValueError here
        fmt, per = message_format(self.opt)
        if fmt is not None:
            if torch.is_grad_enabled() or not x.is_cuda:
                return torch.cat((x, self._aggregate_q(g, x, fmt, per)), dim=1)
            n, C, H, W = x.shape  # the aggregate straight into the buffer's second half, one copy of x
            cat = torch.empty((n, 2 * C, H, W), device=x.device, dtype=x.dtype)
            self._aggregate_q(g, x, fmt, per, out=cat[:, C:])
            cat[:, :C].copy_(x)
            return cat
        if w is not None and self._return_mode() != "input":
            if self._wattn():
                return film_wattn_cat(*self._wattn_args(g, x, w), logits=True, scale=self._attn_scale(), heads=self._attn_heads())
            gb, csr, wmode, logits = self._wmean_args(g, x)
            return film_wmean_cat(x, gb, w, csr, wmode, logits=logits)
        if self._return_mode() == "input" or not x.is_cuda:
            return torch.cat((x, self(g, x)), dim=1)
        mode = _opt(self.opt, "gcn_mode", "film_mean")
        if mode == "copy_mean":
            return film_mean_cat(x, None, g.csr(x.device), mode)
        z = self.edge_encoder.logits(g.edata["pose"])
        if mode == "film_max":
            return film_max_cat(x, z, g.csr(x.device), logits=True)
        if mode in ("film_attn", "film_wattn"):
            return film_attn_cat(x, z, g.csr(x.device), logits=True, scale=self._attn_scale(), heads=self._attn_heads())
        return film_mean_cat(x, z, g.csr(x.device), mode, logits=True)

    def _received(self, g, x, xq, xscale, weights, out):
        """The aggregate of received FP8 messages into ``out`` (N, C, H, W) of x's dtype, for ``opt.gcn_mode``."""
        if torch.is_grad_enabled():
            raise RuntimeError("mrp_gnn: GCN.forward_received is inference-only (the FP8 receiver kernels have no "
                               "backward); run it under torch.no_grad()")
        if self._return_mode() == "input":
            raise ValueError("forward_received with gcn_return='input': no message is aggregated")
        mode = _opt(self.opt, "gcn_mode", "film_mean")
        if weights is not None and mode != "film_wattn":
            raise ValueError(f"forward_received takes weights= for gcn_mode='film_wattn' only, not {mode!r}")
        if x.dim() != 4 or tuple(xq.shape) != tuple(x.shape):
            raise ValueError(f"x {tuple(x.shape)} and xq {tuple(xq.shape)} must be the same (N, C, H, W)")
        csr = g.csr(x.device)
        z = None if mode == "copy_mean" else self.edge_encoder.logits(g.edata["pose"])
        if mode == "film_max":
            return film_max_q_forward_into(xq, xscale, z, csr, out, logits=True)
        if mode in ("film_attn", "film_wattn"):
            kw = dict(logits=True, scale=self._attn_scale(), heads=self._attn_heads())
            if weights is not None:
                film_wattn_q_forward_into(x, xq, xscale, z, weights, csr, out, **kw)
            else:
                film_attn_q_forward_into(x, xq, xscale, z, csr, out, **kw)
            return out
        return film_mean_q_forward_into(xq, xscale, z, csr, out, mode, logits=True)

    def forward_received(self, g, x: torch.Tensor, xq: torch.Tensor, xscale: torch.Tensor = None,
                         weights: torch.Tensor = None) -> torch.Tensor:
        """The layer of a robot that was handed FP8 buffers: the aggregate of the received messages ``xq``
        (N, C, H, W) ``torch.float8_e4m3fn`` / ``torch.float8_e5m2`` with scales ``xscale`` ((N,), (N, 1), (N, C) or
        None), in the dtype of the receiver-side own features ``x`` (N, C, H, W).  Every ``opt.gcn_mode``: the mean
        modes through :func:`aggregate.film_mean_q`, ``film_max`` through :func:`aggregate.film_max_q` (neither
        reads x beyond its dtype), ``film_attn`` / ``film_wattn`` through :func:`aggregate.film_attn_q` with x as
        the query (``opt.gcn_attn_scale``, ``opt.gcn_attn_heads``), and ``film_wattn`` with ``weights=`` (the
        received maps, (N, H, W) fp32) through :func:`aggregate.film_wattn_q`.  Inference-only; nothing is read
        from ``opt.gcn_message_dtype`` (that option simulates the link on one GPU)."""
        out = torch.empty(tuple(x.shape), device=x.device, dtype=x.dtype)
        return self._received(g, x, xq, xscale, weights, out)

    def forward_cat_received(self, g, x: torch.Tensor, xq: torch.Tensor, xscale: torch.Tensor = None,
                             weights: torch.Tensor = None) -> torch.Tensor:
        """``torch.cat((x, self.forward_received(g, x, xq, xscale, weights)), 1)`` with the aggregate written
        straight into the buffer's second half."""
        if x.dim() != 4:
            raise ValueError(f"x must be (N, C, H, W), got {tuple(x.shape)}")
        n, C, H, W = x.shape
        cat = torch.empty((n, 2 * C, H, W), device=x.device, dtype=x.dtype)
        self._received(g, x, xq, xscale, weights, cat[:, C:])
        cat[:, :C].copy_(x)
        return cat

    def forward_cat_compress(self, g, feats: torch.Tensor, conv: nn.Conv2d,
                             weights: torch.Tensor = None) -> torch.Tensor:
        """``conv(torch.cat((feats, self(g, feats)), 1))`` (``models.py:181-184``) without the
        concatenation: the aggregation kernel into its own buffer, then the matrix-core compress
        reading x and the aggregate in place, and in backward the data-gradient kernel writing x's
        gradient half and the aggregate's gradient straight into the aggregation backward, plus the
        split-K weight-gradient kernel (``compress.FilmCompressFunction``).  With
        ``compress.set_compress_path('library')``: the cat kernel + torch's library GEMMs.  bf16 / fp16
        features with fp32 conv parameters (a backbone under ``torch.autocast``, or outside it) take the
        same route on the 16-bit kernels (``compress_half.hip``) and return their dtype: the weight
        rounded once to it, fp32 accumulation and bias, one rounding at the store, fp32 ``dW`` / ``db``.
        A conv stored in 16 bits, or ``compress.set_half_compress('torch')``: the 16-bit cat kernel,
        then ``conv(h)`` by torch.  ``torch.channels_last`` bf16 / fp16 features (C % 32 == 0) stay
        channels_last through the layer and its backward: the pixel-major aggregation and compress
        kernels read and write them in place (``compress_half_cl.hip``;
        ``compress.set_channels_last_compress('convert')`` restores the copy to NCHW); fp32 channels_last
        features do the same after ``compress.set_channels_last_compress_fp32('native')``
        (``compress_split_cl.hip``; by default they are copied to NCHW and the layer returns NCHW)."""
        x = feats
        w = self._weights(x, weights)  # explicit maps with an unsupported option: ValueError here
        fmt, per = message_format(self.opt)
        if fmt is not None:
            # the aggregate of the quantised messages into its own buffer, then the compress kernels on
            # (x, aggregate) with no concatenation; x itself stays unquantised
            a = self._aggregate_q(g, x, fmt, per)
            if x.is_cuda and film_compress_supported(conv, x):
                return CompressFunction.apply(x, a, conv.weight, conv.bias)
            return compress_1x1(conv, torch.cat((x, a), dim=1))
        if w is not None and self._return_mode() != "input":
            if self._wattn():  # the cat kernel, then the compress reading the buffer's two halves in place
                return compress_1x1(conv, self.forward_cat(g, x, weights=w))
            if x.is_cuda and compress_path() != "library" and film_compress_supported(conv, x):
                gb, csr, wmode, logits = self._wmean_args(g, x)
                flags = _lib_modes()["film_sum" if wmode == "sum" else "film_mean"] | (_lib_logits() if logits else 0)
                return film_compress(conv, x, gb, csr, flags, reducer="wmean", weights=w)
            return compress_1x1(conv, self.forward_cat(g, x, weights=w))
        if (x.is_cuda and self._return_mode() != "input" and compress_path() != "library"
                and film_compress_supported(conv, x)):
            mode = _opt(self.opt, "gcn_mode", "film_mean")
            if mode == "copy_mean":
                return film_compress(conv, x, None, g.csr(x.device), _lib_modes()[mode])
            z = self.edge_encoder.logits(g.edata["pose"])
            if mode == "film_max":
                return film_compress(conv, x, z, g.csr(x.device), _lib_logits(), reducer="max")
            if mode in ("film_attn", "film_wattn"):
                return film_compress(conv, x, z, g.csr(x.device), _lib_logits(), reducer="attn",
                                     scale=self._attn_scale(), heads=self._attn_heads())
            return film_compress(conv, x, z, g.csr(x.device), _lib_modes()[mode] | _lib_logits())
        return compress_1x1(conv, self.forward_cat(g, x))

    def forward_residual(self, g, feats: torch.Tensor = None, weights: torch.Tensor = None) -> torch.Tensor:
        """``feats + self(g, feats)`` in one kernel pass: the residual combination ``h = g_h + h``
        of ``dgl/model/dgl_models.py:36-37`` (the FiLM-mean 'add' variant)."""
        x = g.ndata["image"] if feats is None else feats
        w = self._weights(x, weights)  # explicit maps with an unsupported option: ValueError here
        fmt, per = message_format(self.opt)
        if fmt is not None:  # the layer's own h through the epilogue's x0, unquantised
            return self._aggregate_q(g, x, fmt, per, x0=x, x0_scale=1.0)
        if w is not None and self._return_mode() != "input":
            if self._wattn():
                return film_wattn_residual(*self._wattn_args(g, x, w), logits=True, scale=self._attn_scale(), heads=self._attn_heads())
            gb, csr, wmode, logits = self._wmean_args(g, x)
            return film_wmean_residual(x, gb, w, csr, wmode, logits=logits)
        if self._return_mode() == "input" or not x.is_cuda:
            return x + self(g, x)
        mode = _opt(self.opt, "gcn_mode", "film_mean")
        if mode == "copy_mean":
            return film_mean_residual(x, None, g.csr(x.device), mode)
        z = self.edge_encoder.logits(g.edata["pose"])
        if mode == "film_max":
            return film_max_residual(x, z, g.csr(x.device), logits=True)
        if mode in ("film_attn", "film_wattn"):
            return film_attn_residual(x, z, g.csr(x.device), logits=True, scale=self._attn_scale(), heads=self._attn_heads())
        return film_mean_residual(x, z, g.csr(x.device), mode, logits=True)

    def forward_mix(self, g, feats: torch.Tensor, x0: torch.Tensor, alpha: float,
                    weights: torch.Tensor = None) -> torch.Tensor:
        """``(1 - alpha) * self(g, feats) + alpha * x0`` in one kernel pass: a GCN2-style
        initial-feature mix (BASELINE configs[3]'s "GCN2Conv"; not in the reference)."""
        x = feats
        w = self._weights(x, weights)  # explicit maps with an unsupported option: ValueError here
        fmt, per = message_format(self.opt)
        if fmt is not None:
            return self._aggregate_q(g, x, fmt, per, x0=x0, agg_scale=1.0 - float(alpha), x0_scale=float(alpha))
        if w is not None and self._return_mode() != "input":
            if self._wattn():
                return film_wattn_mix(*self._wattn_args(g, x, w), x0, alpha, logits=True, scale=self._attn_scale(), heads=self._attn_heads())
            gb, csr, wmode, logits = self._wmean_args(g, x)
            return film_wmean_mix(x, gb, w, csr, x0, alpha, wmode, logits=logits)
        if self._return_mode() == "input" or not x.is_cuda:
            return (1.0 - alpha) * self(g, x) + alpha * x0
        mode = _opt(self.opt, "gcn_mode", "film_mean")
        if mode == "copy_mean":
            return film_mean_mix(x, None, g.csr(x.device), x0, alpha, mode)
        z = self.edge_encoder.logits(g.edata["pose"])
        if mode == "film_max":
            return film_max_mix(x, z, g.csr(x.device), x0, alpha, logits=True)
        if mode in ("film_attn", "film_wattn"):
            return film_attn_mix(x, z, g.csr(x.device), x0, alpha, logits=True, scale=self._attn_scale(), heads=self._attn_heads())
        return film_mean_mix(x, z, g.csr(x.device), x0, alpha, mode, logits=True)


def _lib_modes():
    from . import _lib
    return _lib.MODES


def _lib_logits():
    from . import _lib
    return _lib.GB_LOGITS


#: layer compositions of a GCN stack (``GCNStack``, ``multi_view_dgl_model``)
COMBINES = ("cat_compress", "cat", "residual", "initial_mix")


def stack_layout(opt):
    """(number of GCN layers, combine, 1x1 compress convs?) from the reference flags
    (``compress_gcn``, ``multi_gcn``, ``models.py:162-171``) or their generalisation
    ``opt.gcn_layers`` / ``opt.gcn_combine``:

    * ``'cat_compress'`` — ``h = conv_i(cat(h, gcn_i(h)))`` per layer (``models.py:180-189``;
      ``multi_gcn`` is two such layers; k layers extend the ``gcn<i>``/``conv<i>`` naming);
    * ``'cat'`` — one layer, ``h = cat(h, gcn1(h))`` (2C channels; ``compress_gcn`` off);
    * ``'residual'`` — ``h = h + gcn_i(h)`` (``dgl_models.py:36-37``), no convs;
    * ``'initial_mix'`` — ``h = (1 - alpha) gcn_i(h) + alpha h0`` (``opt.gcn2_alpha``, default 0.1;
      GCN2-style extension, not in the reference), no convs."""
    layers = int(_opt(opt, "gcn_layers", 0) or (2 if _opt(opt, "multi_gcn", False) else 1))
    combine = _opt(opt, "gcn_combine", None)
    if combine is None:
        combine = "cat_compress" if _opt(opt, "compress_gcn", False) else "cat"
    if combine not in COMBINES:
        raise ValueError(f"gcn_combine must be one of {COMBINES}, got {combine!r}")
    if layers < 1:
        raise ValueError("gcn_layers must be >= 1")
    if combine == "cat" and layers > 1:
        raise AssertionError("stacked GCN layers need compress_gcn (models.py:169)")
    return layers, combine, combine == "cat_compress"


def _build_stack(module: nn.Module, opt) -> None:
    layers, combine, convs = stack_layout(opt)
    module.gcn_layers, module.gcn_combine = layers, combine
    for i in range(1, layers + 1):
        setattr(module, f"gcn{i}", GCN(opt))
        if convs:
            setattr(module, f"conv{i}", nn.Conv2d(opt.feature_dim * 2, opt.feature_dim, kernel_size=1))


def _run_stack(module: nn.Module, g, h: torch.Tensor) -> torch.Tensor:
    """The layer loop of ``multi_view_dgl_model.forward`` (``models.py:180-189``), k layers."""
    h0 = h
    alpha = float(_opt(module.opt, "gcn2_alpha", 0.1))
    for i in range(1, module.gcn_layers + 1):
        gcn = getattr(module, f"gcn{i}")
        if module.gcn_combine == "cat_compress":
            h = gcn.forward_cat_compress(g, h, getattr(module, f"conv{i}"))  # conv_i(cat((h, gcn_i(h)), 1))
        elif module.gcn_combine == "cat":
            h = gcn.forward_cat(g, h)  # cat((h, gcn_i(h)), 1), one kernel pass
        elif module.gcn_combine == "residual":
            h = gcn.forward_residual(g, h)
        else:
            h = gcn.forward_mix(g, h, h0, alpha)
    return h


class GCNStack(_PackedImages, nn.Module):
    """k stacked GCN layers (``dgl/model/models.py:162-171,180-189`` generalised; see
    :func:`stack_layout`).  ``state_dict`` keys ``gcn1.*``, ``conv1.*``, ..., ``gcn<k>.*``,
    ``conv<k>.*`` — the reference's naming for k = 1, 2."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        _build_stack(self, opt)

    def forward(self, g, h: torch.Tensor) -> torch.Tensor:
        return _run_stack(self, g, h)


class GCNBlock(GCNStack):
    """GCN stacking of ``multi_view_dgl_model`` (``dgl/model/models.py:162-171,180-189``): gcn1 ->
    cat -> [conv1] -> [gcn2 -> cat -> conv2] from the reference's ``compress_gcn``/``multi_gcn``
    flags (a :class:`GCNStack` of one or two layers)."""

    def __init__(self, opt):
        if opt.multi_gcn:
            assert opt.compress_gcn  # models.py:169
        super().__init__(opt)


class multi_view_dgl_model(_PackedImages, nn.Module):  # noqa: N801  (reference class name)
    """``dgl/model/models.py:157-205`` with caller-supplied CNN ``encoder``/``decoder``.

    ``encoder(images (B, N, 3, S, S)) -> list of feature maps`` (last one used) and
    ``decoder(h) -> prediction`` follow the reference modules' call signatures; with
    ``encoder=None`` the node features in ``g.ndata['image']`` are taken to be feature maps
    already (the synthetic benchmark setting).
    """

    def __init__(self, opt, encoder: nn.Module = None, decoder: nn.Module = None):
        super().__init__()
        self.opt = opt
        if encoder is not None:
            self.encoder = encoder
        if _opt(opt, "multi_gcn", False):
            assert opt.compress_gcn  # models.py:169
        _build_stack(self, opt)  # gcn1 [conv1] [gcn2 conv2] ... (models.py:162-171)
        if decoder is not None:
            self.decoder = decoder

    def __setstate__(self, state):
        super().__setstate__(state)
        if "gcn_layers" not in self.__dict__:  # pickled by the reference: its flags give the layout
            self.gcn_layers, self.gcn_combine, _ = stack_layout(self.opt)

    def features(self, g):
        """Encoder output per node, (B*N, C, h, w), and the encoder's feature list
        (``models.py:175-179``)."""
        image = g.ndata["image"]
        if not hasattr(self, "encoder"):
            return image, [image]
        image = image.view(-1, self.opt.camera_num, 3, self.opt.image_size, self.opt.image_size)
        h_list = self.encoder(image)
        h = h_list[-1]
        return h.view(-1, h.size()[-3], h.size()[-2], h.size()[-1]), h_list

    def decode(self, h, h_list):
        """The decoder heads of ``models.py:190-205``: ``skip_level`` also passes the encoder's
        feature list; ``task='depthseg'`` calls ``depth_decoder`` and ``seg_decoder``."""
        if _opt(self.opt, "task", "depth") == "depthseg" and hasattr(self, "depth_decoder"):
            heads = (self.depth_decoder, self.seg_decoder)
        elif hasattr(self, "decoder"):
            heads = (self.decoder,)
        else:
            return h  # no decoder supplied: the GCN block's output (the benchmark setting)
        args = (h, h_list) if _opt(self.opt, "skip_level", False) else (h,)
        outs = tuple(head(*args) for head in heads)
        return outs if len(outs) > 1 else outs[0]

    def forward(self, g):
        with g.local_scope():
            h, h_list = self.features(g)
            g.ndata["image"] = h
            h = _run_stack(self, g, h)  # gcn1 -> cat -> conv1 [-> gcn2 -> cat -> conv2], models.py:180-189
            return self.decode(h, h_list)
