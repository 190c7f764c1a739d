"""Host-side mirror of the reference's operator API around the mixer.

  Block          reference models/block.py:17-76   (Add -> LayerNorm -> mixer, DropPath)
  create_block   reference models/point_mamba.py:147-175
  _init_weights  reference models/point_mamba.py:115-144
  MixerModel     reference models/point_mamba.py:178-272
  MixerModel_add reference models/point_mamba.py:281-428   (add_after_layer: cross-merge after every block)

Same constructor arguments, forward signatures, return values and parameter names, so a
state_dict of the reference's ``blocks.*`` loads unchanged.  The Triton fused add+norm path
(``fused_add_norm=True``) is never enabled by any reference config and is refused here
(no Triton in this framework).
"""
from __future__ import annotations

import math
from functools import partial
from typing import NamedTuple, Optional

import torch
import torch.nn as nn
from torch import Tensor

from . import _lib
from .add_norm import add_layer_norm_fn
from .cross_merge import cross_merge, cross_merge_composed, cross_merge_maps
from .mamba_simple import Mamba
from .out_norm import out_proj_add_ln_fn, out_proj_add_ln_ok
from .rms_norm import RMSNorm
from .spectral import argsort_rows, take

_KERNEL_NORMS = (nn.LayerNorm, RMSNorm)      # the norms the add + norm kernels compute


def _fused_norm(hidden, residual, norm, rowscale=None, out_dtype=None, **compact):
    """Add (+ DropPath) + ``norm`` (an nn.LayerNorm or an RMSNorm) through the add_norm kernel: -> (normed, residual).
    RMSNorm routes are counted (``add_rms_norm``).  ``compact``: add_layer_norm_fn's slot-map arguments."""
    rms = type(norm) is RMSNorm
    if rms:
        _lib.count("add_rms_norm")
    return add_layer_norm_fn(hidden, residual, norm.weight, norm.bias, norm.eps, rowscale=rowscale,
                             out_dtype=out_dtype, rms=rms, **compact)


class DropPath(nn.Module):
    """Per-sample stochastic depth (the timm layer the reference imports at models/block.py:13)."""

    def __init__(self, drop_prob: float = 0.0, scale_by_keep: bool = True):
        super().__init__()
        self.drop_prob = drop_prob
        self.scale_by_keep = scale_by_keep

    def rowscale(self, x):
        """Per-sample factor (B,) this layer would multiply x by, or None when it is the identity."""
        return self.rowscale_for(x.shape[0], x.device)

    def rowscale_for(self, batch, device):
        """rowscale() from the batch size and the device alone: the same draw, for callers that make it before the
        tensor exists (MixerModel.draw_drop_plan)."""
        if self.drop_prob == 0.0 or not self.training:
            return None
        keep = 1.0 - self.drop_prob
        mask = torch.empty(batch, device=device, dtype=torch.float32).bernoulli_(keep)
        if keep > 0.0 and self.scale_by_keep:
            mask.div_(keep)
        return mask

    def forward(self, x):
        mask = self.rowscale(x)
        return x if mask is None else x * mask.to(x.dtype).view((-1,) + (1,) * (x.dim() - 1))


class Block(nn.Module):
    def __init__(self, dim, mixer_cls, norm_cls=nn.LayerNorm, fused_add_norm=False,
                 residual_in_fp32=False, drop_path=0.):
        super().__init__()
        if fused_add_norm:
            raise NotImplementedError("fused_add_norm (Triton) is not part of this framework; "
                                      "no reference config enables it")
        self.residual_in_fp32 = residual_in_fp32
        self.fused_add_norm = False
        self.mixer = mixer_cls(dim)
        self.norm = norm_cls(dim)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()

    def forward(self, hidden_states: Tensor, residual: Optional[Tensor] = None, inference_params=None, A=None, *,
                rowscale=None, draw=True, compact=None):
        """hidden_states = Mixer(LN(residual)); returns (hidden_states, residual).  ``A`` (optional, specific to this
        implementation): the mixer's -exp(A_log) when the caller has already formed it (MixerModel does, for all
        layers in one launch); handed on as an argument, never parked on the module.

        Add (+ DropPath) + LayerNorm (or RMSNorm) run as one HIP pass each way (add_norm.py) for such blocks on the
        GPU; the composed torch form below is the reference's own and serves any other norm / device.

        ``rowscale`` (B,), ``draw``, ``compact`` (specific to this implementation, MixerModel's): the DropPath factors
        when the caller has already drawn them; ``draw=False`` when it drew the whole forward's ahead (a DropPlan): the
        block then draws none even where ``rowscale`` is None (block 0), and ``compact`` may hold add_layer_norm_fn's
        slot-map arguments for a ``hidden_states`` of only some samples and / or a mixer that is to run only on some;
        the hidden_states returned are then compact too, None when the mixer has no sample to run on."""
        if not draw:
            hidden_states, residual = _fused_norm(hidden_states, residual, self.norm, rowscale=rowscale,
                                                  **(compact or {}))
            if hidden_states.shape[0] == 0:
                return None, residual
        elif hidden_states.is_cuda and type(self.norm) in _KERNEL_NORMS and hidden_states.dim() == 3:
            scale = rowscale
            if scale is None and isinstance(self.drop_path, DropPath):
                scale = self.drop_path.rowscale(hidden_states)
            hidden_states, residual = _fused_norm(hidden_states, residual, self.norm, rowscale=scale)
        elif rowscale is not None:
            raise NotImplementedError("Block.forward(rowscale=...): drawn DropPath factors are taken by the add + norm "
                                      "kernel route only")
        else:
            residual = (self.drop_path(hidden_states) + residual) if residual is not None else hidden_states
            hidden_states = self.norm(residual.to(dtype=self.norm.weight.dtype))
            if self.residual_in_fp32:
                residual = residual.to(torch.float32)
        if A is not None:
            hidden_states = self.mixer(hidden_states, inference_params=inference_params, A=A)
        else:
            hidden_states = self.mixer(hidden_states, inference_params=inference_params)
        return hidden_states, residual

    def allocate_inference_cache(self, batch_size, max_seqlen, dtype=None, **kwargs):
        return self.mixer.allocate_inference_cache(batch_size, max_seqlen, dtype=dtype, **kwargs)


def _init_weights(module, n_layer, initializer_range=0.02, rescale_prenorm_residual=True,
                  n_residuals_per_layer=1):
    if isinstance(module, nn.Linear):
        if module.bias is not None and not getattr(module.bias, "_no_reinit", False):
            nn.init.zeros_(module.bias)
    elif isinstance(module, nn.Embedding):
        nn.init.normal_(module.weight, std=initializer_range)
    if rescale_prenorm_residual:
        # GPT-2 style: residual-branch output projections scaled by 1/sqrt(#residual layers)
        for name, p in module.named_parameters():
            if name in ("out_proj.weight", "fc2.weight"):
                nn.init.kaiming_uniform_(p, a=math.sqrt(5))
                with torch.no_grad():
                    p /= math.sqrt(n_residuals_per_layer * n_layer)


def create_block(d_model, ssm_cfg=None, norm_epsilon=1e-5, rms_norm=False, residual_in_fp32=False,
                 fused_add_norm=False, layer_idx=None, drop_path=0., device=None, dtype=None):
    ssm_cfg = {} if ssm_cfg is None else ssm_cfg
    factory_kwargs = {"device": device, "dtype": dtype}
    mixer_cls = partial(Mamba, layer_idx=layer_idx, **ssm_cfg, **factory_kwargs)
    norm_cls = partial(nn.LayerNorm if not rms_norm else RMSNorm, eps=norm_epsilon, **factory_kwargs)
    block = Block(d_model, mixer_cls, norm_cls=norm_cls, fused_add_norm=fused_add_norm,
                  residual_in_fp32=residual_in_fp32, drop_path=drop_path)
    block.layer_idx = layer_idx
    return block


class _SkippedMixerFn(torch.autograd.Function):
    """x, unchanged, with exact-zero gradients for ``params``: stands in for a mixer that ran on no sample, so that its
    parameters receive what the full route gives them (zeros, not None -- optimisers and gradient reducers tell the
    two apart)."""

    @staticmethod
    def forward(ctx, x, *params):
        ctx.save_for_backward(*params)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, dx):
        return (dx,) + tuple(torch.zeros_like(p) for p in ctx.saved_tensors)


# One side stream per device, and per (device, blocks, batch) a pool of free pinned staging pairs (not module
# attributes: modules get deep-copied and pickled).  A plan owns its pair from the draw until its maps are on their
# way up, so plans in flight at the same time -- two stacks of one shape, or a plan drawn and never used -- never share
# one; a plan that is dropped simply keeps its pair out of the pool.
_drop_streams = {}
_drop_hosts = {}


class DropPlan:
    """The DropPath factors of one forward of a MixerModel, drawn ahead of the blocks (MixerModel.draw_drop_plan), and
    what follows from them once they are on the host (MixerModel._finish_plan).

    ``masks[j - 1]`` (B,) fp32 on the device is block j's rowscale, j = 1 .. n - 1.  ``lead``: a draw for block 0
    came first (the route on which block 0 runs through Block.forward draws one and never applies it).  After
    _finish_plan, for every boundary j: ``sizes[j - 1]`` = the compact batch mixer j - 1 runs at (B: all of it, 0: not
    at all) and ``maps[j - 1]`` = the (B,) int32 device map sample -> slot, None at B; ``sel`` (sizes[0],) int32 =
    the samples of boundary 1 by slot, for the route that compacts block 0's tokens with index_select."""
    __slots__ = ("masks", "lead", "batch", "event", "host", "sizes", "maps", "sel")


class StackRoute(NamedTuple):
    """Which way one forward of a MixerModel goes (MixerModel.route)."""
    first_on_tokens: bool       # block 0 runs on the G distinct tokens (_first_block_on_distinct_tokens)
    stack: str                  # "chain" (fused bf16, _chain), "compact" (a DropPlan, _compact_stack) or "layers"

    @property
    def lead(self):
        """Does a DropPlan of this route open with block 0's draw?  Where block 0 goes through Block.forward it draws
        a rowscale it never applies; on the distinct tokens it draws none."""
        return not self.first_on_tokens


class MixerModel(nn.Module):
    def __init__(self, d_model: int, n_layer: int, ssm_cfg=None, norm_epsilon: float = 1e-5,
                 rms_norm: bool = False, initializer_cfg=None, fused_add_norm=False,
                 residual_in_fp32=False, drop_out_in_block: float = 0., drop_path: float = 0.1,
                 device=None, dtype=None) -> None:
        factory_kwargs = {"device": device, "dtype": dtype}
        super().__init__()
        self.residual_in_fp32 = residual_in_fp32
        self.fused_add_norm = fused_add_norm
        self.layers = nn.ModuleList([
            create_block(d_model, ssm_cfg=ssm_cfg, norm_epsilon=norm_epsilon, rms_norm=rms_norm,
                         residual_in_fp32=residual_in_fp32, fused_add_norm=fused_add_norm, layer_idx=i,
                         drop_path=drop_path, **factory_kwargs)
            for i in range(n_layer)])
        self.norm_f = (nn.LayerNorm if not rms_norm else RMSNorm)(d_model, eps=norm_epsilon, **factory_kwargs)
        self.apply(partial(_init_weights, n_layer=n_layer,
                           **(initializer_cfg if initializer_cfg is not None else {})))
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.drop_out_in_block = nn.Dropout(drop_out_in_block) if drop_out_in_block > 0. else nn.Identity()
        # run each mixer only on the samples the next block's DropPath keeps (draw_drop_plan); stacks that have not
        # been measured on the route switch it off (mae.py)
        self.drop_path_compact = True

    def allocate_inference_cache(self, batch_size, max_seqlen, dtype=None, **kwargs):
        return {i: layer.allocate_inference_cache(batch_size, max_seqlen, dtype=dtype, **kwargs)
                for i, layer in enumerate(self.layers)}

    # ---- DropPath: mixers on the kept samples only -------------------------------------------------------------------
    # Block j (j >= 1) forms residual = rowscale_j * hidden_{j-1} + residual, and rowscale_j[b] is 0 for the samples its
    # DropPath drops: mixer j - 1 is computed for them and multiplied by zero, and backward their dhidden is zero, so
    # the whole mixer backward runs on zeros.  With the factors known BEFORE the stack starts, mixer j - 1 runs on the
    # kept samples only: block j - 1's add + norm writes `normed` compacted, block j's reads `hidden` compacted
    # (add_norm.py's slot maps); the residual stream keeps the whole batch.

    def route(self, like, seqlen=None, inference_params=None):
        """The StackRoute of a forward, from shapes, dtypes (autocast's), modes and the configuration alone, so that it
        can be asked before the tokens exist; the one place the three predicates below are asked, each once.
        ``like``: what the stack is handed, or a stand-in of its shape and device; ``seqlen``: the length of the
        balanced ``token_index`` that comes with (B, G, C) distinct tokens, None when ``like`` is the sequence."""
        plain = inference_params is None and len(self.layers) > 0
        first = plain and seqlen is not None and self._first_block_applies(like, seqlen)
        if plain and self._chain_ok(like):
            return StackRoute(first, "chain")
        return StackRoute(first, "compact" if self._compact_ok(like, inference_params) else "layers")

    def _compact_ok(self, x, inference_params=None):
        """Does a forward on ``x`` take the compact route, the fused chain apart (route() asks _chain_ok first)?
        Training with DropPath in every block, plain blocks on the add + norm kernels, nothing between the blocks, no
        stream capture (the plan needs the factors on the host), and not switched off (_lib.drop_path_compact,
        self.drop_path_compact)."""
        if not (self.drop_path_compact and _lib.drop_path_compact_enabled() and self.training
                and type(self) is MixerModel and inference_params is None and len(self.layers) > 1
                and x.is_cuda and x.dim() == 3 and isinstance(self.drop_out_in_block, nn.Identity)
                and type(self.norm_f) in _KERNEL_NORMS):
            return False
        for layer in self.layers:
            dp = layer.drop_path
            if not (type(layer) is Block and type(layer.norm) in _KERNEL_NORMS and type(layer.mixer) is Mamba
                    and isinstance(dp, DropPath) and dp.training and 0.0 < dp.drop_prob < 1.0):
                return False
        return not torch.cuda.is_current_stream_capturing()

    def _first_block_applies(self, tokens, seqlen):
        """Will _first_block_on_distinct_tokens take (B, G, C) ``tokens`` expanded to ``seqlen`` positions?  Shapes and
        types only, so that it can be answered before the index map exists (its other condition, L % G, is among
        expansion_ok's)."""
        from . import seq_expand
        layer = self.layers[0]
        return (tokens.is_cuda and type(layer.norm) in _KERNEL_NORMS and isinstance(layer.mixer, Mamba)
                and layer.mixer.use_fast_path and seq_expand.expansion_len_ok(tokens, seqlen))

    def draw_drop_plan(self, like, lead=False, drop_masks=None, route=None):
        """Draw the DropPath factors of blocks 1 .. n - 1 for a batch like ``like``'s NOW -- the same bernoulli_ calls
        in the same order as the blocks would make (``lead``: block 0's unused draw first, see DropPlan) -- and start
        their copy to the host.  -> a DropPlan for forward(drop_plan=...), or None when a forward on ``like`` would not
        take the compact route (then nothing is drawn).  ``drop_masks``: these factors instead of drawn ones.
        ``route``: route()'s answer for this forward when the caller holds it (``lead`` is then ``route.lead``)."""
        if route is None:
            route = self.route(like)
        if route.stack != "compact":
            return None
        n, B, dev = len(self.layers), like.shape[0], like.device
        plan = DropPlan()
        if drop_masks is None:
            with torch.cuda.stream(self._drop_stream(dev)):
                if lead:
                    self.layers[0].drop_path.rowscale_for(B, dev)
                plan.masks = [self.layers[j].drop_path.rowscale_for(B, dev) for j in range(1, n)]
        else:
            if len(drop_masks) != n - 1:
                raise ValueError(f"drop_masks: one (B,) rowscale for each of the blocks 1 .. {n - 1}, got "
                                 f"{len(drop_masks)}")
            plan.masks = [m.to(device=dev, dtype=torch.float32) for m in drop_masks]
        plan.lead, plan.batch = bool(lead), B
        free = _drop_hosts.setdefault((dev, n - 1, B), [])
        # pinned staging, reused from step to step: the factors down, the maps (and boundary 1's samples) up.  Both
        # copies run on the side stream, and a plan overwrites a pair it took from the pool only after it has waited
        # for its own factors, which that stream copies down behind the previous owner's upload.
        host = free.pop() if free else (torch.empty(n - 1, B, dtype=torch.float32).pin_memory(),
                                        torch.empty(n, B, dtype=torch.int32).pin_memory())
        plan.host = host
        main, side = torch.cuda.current_stream(dev), self._drop_stream(dev)
        if drop_masks is not None:
            side.wait_stream(main)                          # handed-in factors come from the caller's stream
        with torch.cuda.stream(side):
            host[0].copy_(torch.stack(plan.masks), non_blocking=True)
            plan.event = torch.cuda.Event()
            plan.event.record(side)
        for m in plan.masks:
            m.record_stream(main)
        plan.sizes = plan.maps = plan.sel = None
        return plan

    def _drop_stream(self, dev):
        """The stream the factors are drawn and copied on.  A draw depends on nothing the device has still to compute
        (the generator's offset advances on the host when the draw is launched), so it need not queue behind the
        previous step's backward on the caller's stream: the host then waits for a few tiny kernels, not for the
        device to catch up, and keeps running ahead of it as it does on the full route."""
        st = _drop_streams.get(dev)
        if st is None:
            st = _drop_streams[dev] = torch.cuda.Stream(device=dev)
        return st

    def _finish_plan(self, plan, dev):
        """Wait for the factors (the one host synchronisation of the step: for the side stream's copy, not for the
        caller's stream), form every boundary's compact batch and slot map on the host and upload all maps in one
        copy."""
        plan.event.synchronize()
        B, bucket = plan.batch, _lib.DROP_PATH_BUCKET
        down, up = plan.host
        check = _lib.load().simamba_add_layer_norm_check_slots
        sizes, rows = [], []
        for j, row in enumerate(down.tolist()):
            kept = [b for b, v in enumerate(row) if v != 0.0]
            k = len(kept)
            size = min(B, bucket * ((k + bucket - 1) // bucket))
            sizes.append(size)
            if size == B:
                rows.append([0] * B)                       # not used: the boundary runs on the whole batch
                continue
            # kept samples first, in order; the spare slots of the bucket go to dropped samples, which stay in with
            # their factor of 0 exactly as on the full route
            dropped = [b for b, v in enumerate(row) if v == 0.0]
            members = kept + dropped[:size - k]
            slot = [-1] * B
            for s_, b in enumerate(members):
                slot[b] = s_
            rows.append(slot)
            if j == 0:
                sel = members + [0] * (B - size)
        if sizes[0] == B:
            sel = list(range(B))
        up.copy_(torch.tensor(rows + [sel], dtype=torch.int32))
        for j, size in enumerate(sizes):
            if size < B:
                _lib.check(check(up[j].data_ptr(), B, size), "simamba_add_layer_norm_check_slots")
        main, side = torch.cuda.current_stream(dev), self._drop_stream(dev)
        with torch.cuda.stream(side):
            maps = up.to(dev, non_blocking=True)
        main.wait_stream(side)                              # the maps, and the factors drawn before them
        maps.record_stream(main)
        _drop_hosts[(dev, len(sizes), B)].append(plan.host)  # back to the pool (see draw_drop_plan on the order)
        plan.host = None
        plan.sizes = sizes
        plan.maps = [maps[j] if size < B else None for j, size in enumerate(sizes)]
        plan.sel = maps[len(sizes), :sizes[0]]
        return plan

    def _first_block_on_distinct_tokens(self, tokens, pos, token_index, A=None, emit_y=False, keep=None):
        """Block 0 when the sequence is ``gather(tokens + pos, token_index)``: Add + LayerNorm + in_proj on the G
        distinct tokens, expanded to the L positions by a copy kernel (seq_expand.py).  -> (hidden, residual) of
        block 0 as the reference's Block.forward returns them (``emit_y``: the mixer's output before out_proj in
        place of hidden, see _chain).  For routes with ``first_on_tokens`` (_first_block_applies, which holds L % G == 0
        among its conditions).  ``keep`` = (samples (n,) int32, n): the mixer runs on these samples only and ``hidden``
        holds them in this order (None when n == 0); the residual keeps the whole batch."""
        from . import seq_expand
        layer = self.layers[0]
        mixer = layer.mixer
        inv32 = seq_expand.inverse_positions(token_index, tokens.shape[1])
        idx32 = token_index.to(torch.int32).contiguous()
        # residual_0 = tokens + pos and its LayerNorm in one pass over the G tokens.  (Low-precision operands: the
        # reference's `input_ids + pos` rounds the sum to that dtype first -- keep that rounding.)
        if tokens.dtype == torch.float32:
            normed, res0 = _fused_norm(tokens, pos, layer.norm)
        else:
            normed, res0 = _fused_norm(tokens + pos, None, layer.norm)
        if keep is not None and keep[1] < tokens.shape[0]:
            # the per-token head and the mixer on the kept samples: (n, G, C) rows of three small tensors
            sel, nk = keep
            normed, idx32, inv32 = (t.index_select(0, sel) for t in (normed, idx32, inv32)) if nk else (None,) * 3
        if normed is None:
            hidden = None
        else:
            xz = seq_expand.seq_gather_last(mixer.in_proj_xz(normed), idx32, inv32)      # (B, 2D, L)
            hidden = mixer.forward_xz(xz, A=A, emit_y=emit_y)
        return hidden, take(res0, token_index)

    def _precompute_A(self):
        """A = -exp(A_log) of every layer in three launches (stack, exp, neg) instead of two per layer, and one
        exp / neg backward for all of them.  -> per-layer list (slices of one tensor) handed to the blocks as an
        ARGUMENT, or a list of None when the layers are not uniform Mamba mixers on the GPU (each then forms its own)."""
        mixers = [layer.mixer for layer in self.layers]
        if (len(mixers) > 1 and all(type(m) is Mamba for m in mixers) and mixers[0].A_log.is_cuda
                and all(m.A_log.shape == mixers[0].A_log.shape for m in mixers)):
            return list((-torch.exp(torch.stack([m.A_log for m in mixers]).float())).unbind(0))
        return [None] * len(mixers)

    def _chain_ok(self, x):
        """Can the stack run as  add+LN -> [in_proj -> mixer body -> (out_proj + add + LN)] * n  with the bracketed
        out_proj / add / LayerNorm as ONE kernel (out_norm.py)?  bf16 compute (autocast or bf16 modules), plain
        LayerNorm (or RMSNorm) blocks around fast-path Mamba mixers without an out_proj bias, nothing between the
        blocks."""
        if not (_lib.fuse_out_norm_enabled() and x.is_cuda and x.dim() == 3
                and isinstance(self.drop_out_in_block, nn.Identity) and type(self.norm_f) in _KERNEL_NORMS):
            return False
        # the dtype the projections compute in: autocast's, else the parameters'
        io = (torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda")
              else self.layers[0].mixer.in_proj.weight.dtype)
        if io != torch.bfloat16:
            return False
        d_model = x.shape[-1]
        for layer in self.layers:
            m = layer.mixer
            if not (type(layer) is Block and type(layer.norm) in _KERNEL_NORMS and type(m) is Mamba and m.use_fast_path
                    and m.out_proj.bias is None and m.d_model == d_model and d_model % 128 == 0 and d_model <= 384
                    and m.d_inner % 64 == 0):
                return False
        return True

    def _chain(self, first, hidden_states, residual, A_all):
        """Blocks ``first``.. of the stack and its final norm on the fused route.  ``hidden_states``: the stack's input
        when ``first == 0`` (block 0's add + norm opens the chain with ``normed``, the LayerNorm output a block feeds
        its mixer), else ``y``, block ``first - 1``'s mixer output before out_proj (B, d_inner, L); ``residual`` is the
        fp32 residual stream that goes with it.  What the reference computes across each
        block boundary -- out_proj (models/block.py:72), residual = drop_path(hidden) + residual and norm(residual) at
        the top of the next block (:56-58), or norm_f after the last (models/point_mamba.py:257-258) -- is one kernel;
        shapes it does not take run the same three ops through the library GEMM and the add + LayerNorm kernel."""
        y = normed = None
        if first == 0:
            l0 = self.layers[0]
            scale = l0.drop_path.rowscale(hidden_states) if isinstance(l0.drop_path, DropPath) else None
            normed, residual = _fused_norm(hidden_states, None, l0.norm, rowscale=scale)
        else:
            y = hidden_states
        n = len(self.layers)
        i = first
        while True:
            if y is not None:                               # close block i - 1, open block i (or finish the stack)
                prev = self.layers[i - 1].mixer
                if i < n:
                    norm, dp = self.layers[i].norm, self.layers[i].drop_path
                    scale = dp.rowscale(y) if isinstance(dp, DropPath) else None
                    out_dtype = y.dtype                     # what add_layer_norm_fn hands a block's in_proj
                else:
                    norm, scale, out_dtype = self.norm_f, None, self.norm_f.weight.dtype
                if out_proj_add_ln_ok(y, prev.out_proj.weight, prev.d_model):
                    rms = type(norm) is RMSNorm
                    _lib.count("out_proj_add_rms" if rms else "out_proj_add_ln")
                    normed, residual = out_proj_add_ln_fn(y, prev.out_proj.weight, residual, norm.weight, norm.bias,
                                                          norm.eps, rowscale=scale, out_dtype=out_dtype, rms=rms)
                else:
                    hidden = torch.matmul(y.transpose(1, 2), prev.out_proj.weight.t().to(y.dtype))
                    normed, residual = _fused_norm(hidden, residual, norm, rowscale=scale, out_dtype=out_dtype)
                if i == n:
                    return normed
            mixer = self.layers[i].mixer
            y = mixer.forward_xz(mixer.in_proj_xz(normed), A=A_all[i], emit_y=True)
            i += 1

    def forward(self, input_ids, pos, inference_params=None, token_index=None, balanced_index=False, *,
                route=None, drop_plan=None, drop_masks=None):
        """Reference signature (models/point_mamba.py:247).  ``token_index`` (B, L) int64, optional and specific to
        this implementation: when given, ``input_ids`` / ``pos`` are the G DISTINCT tokens (B, G, C) and the sequence
        the reference would be handed is their gather by ``token_index``; the result is the same.
        ``balanced_index=True`` is the caller's statement that every token occurs exactly L / G times in every row of
        ``token_index`` (a concatenation of permutations, which is what the SAST / MAMBA assemblies are): only then
        does the first block's per-token head run on the G tokens (the adjoint of that expansion sums a fixed number
        of positions per token); any other index takes the reference's route on the gathered sequence.

        ``route``, ``drop_plan`` (keyword-only, specific to this implementation): route()'s answer for this forward
        and what draw_drop_plan returned for it, when the caller asked and drew early (PointMamba does, ahead of its
        tokeniser, so that the copy to the host is long done here); without them the route is decided and the factors
        are drawn on entry.  ``drop_masks``: a test hook, the (B,) rowscales of blocks 1 .. n - 1 to use in place of
        drawn ones, on the compact and on the full route."""
        if route is None:
            route = self.route(input_ids, token_index.shape[1] if (token_index is not None and balanced_index) else None,
                               inference_params)
        plan = drop_plan
        if plan is None:
            plan = self.draw_drop_plan(input_ids, lead=route.lead, drop_masks=drop_masks, route=route)
        elif route.stack != "compact" or plan.lead != route.lead or plan.batch != input_ids.shape[0]:
            raise ValueError("MixerModel.forward: drop_plan was drawn for another route or batch")
        if plan is not None:
            self._finish_plan(plan, input_ids.device)
            _lib.count("drop_path_compact")
        A_all = self._precompute_A()
        if route.stack == "chain" and drop_masks is not None:
            raise NotImplementedError("MixerModel.forward(drop_masks=...): the fused bf16 chain draws its own factors")
        if route.first_on_tokens:
            hidden_states, residual = self._first_block_on_distinct_tokens(
                input_ids, pos, token_index, A=A_all[0], emit_y=route.stack == "chain",
                keep=None if plan is None else (plan.sel, plan.sizes[0]))
            if plan is not None:
                residual = self._compact_ran(0, hidden_states, residual)
            hidden_states = self.drop_out_in_block(hidden_states)
            first = 1
        else:
            if token_index is not None:                     # the reference's route on the expanded sequence
                input_ids, pos = take(input_ids, token_index), take(pos, token_index)
            hidden_states, residual, first = input_ids + pos, None, 0
        if route.stack == "chain":
            return self._chain(first, hidden_states, residual, A_all)
        if plan is not None:
            return self._compact_stack(first, hidden_states, residual, A_all, plan)
        return self._layer_stack(first, hidden_states, residual, A_all, inference_params, drop_masks)

    def _layer_stack(self, first, hidden_states, residual, A_all, inference_params=None, drop_masks=None):
        """Blocks ``first``.. and the final norm, every block drawing its own factors (``drop_masks``: those)."""
        for i in range(first, len(self.layers)):
            scale = drop_masks[i - 1] if (drop_masks is not None and i > 0) else None
            hidden_states, residual = self.layers[i](hidden_states, residual, inference_params=inference_params,
                                                     A=A_all[i], rowscale=scale)
            hidden_states = self.drop_out_in_block(hidden_states)
        return self._final_norm(hidden_states, residual)

    def _final_norm(self, hidden_states, residual):
        """norm_f(hidden_states + residual), the stack's output (and the segmentation stack's taps): the add + norm
        kernel on the GPU, the reference's composed torch ops otherwise."""
        if hidden_states.is_cuda and type(self.norm_f) in _KERNEL_NORMS and hidden_states.dim() == 3:
            # the stack's output norm returns the parameter dtype (fp32) under autocast too, as F.layer_norm does
            # there; the block norms feed a GEMM and may hand over the autocast dtype directly
            return _fused_norm(hidden_states, residual, self.norm_f, out_dtype=self.norm_f.weight.dtype)[0]
        residual = (hidden_states + residual) if residual is not None else hidden_states
        return self.norm_f(residual.to(dtype=self.norm_f.weight.dtype))

    def _compact_ran(self, i, hidden_states, residual):
        """Mixer ``i``'s compact batch is counted; one that ran on no sample gets zero gradients.  -> residual"""
        if hidden_states is None:
            return _SkippedMixerFn.apply(residual, *self.layers[i].mixer.parameters())
        size = hidden_states.shape[0]
        _lib.compact_sizes[size] = _lib.compact_sizes.get(size, 0) + 1
        return residual

    def _compact_stack(self, first, hidden_states, residual, A_all, plan):
        """Blocks ``first``.. and the final norm with every mixer on its boundary's compact batch (DropPlan).
        ``hidden_states`` is block ``first - 1``'s compact output (None: it ran on no sample), or the stack's input
        when ``first == 0``."""
        n, B = len(self.layers), plan.batch
        io = hidden_states.dtype if hidden_states is not None else self.layers[0].mixer.out_proj.weight.dtype
        for i in range(first, n):
            compact = {}
            if i > 0 and plan.sizes[i - 1] < B:            # hidden holds boundary i's samples
                compact.update(hidden_slot=plan.maps[i - 1], hidden_dtype=io)
            if i < n - 1 and plan.sizes[i] < B:            # mixer i runs on boundary i + 1's
                compact.update(normed_slot=plan.maps[i], normed_batch=plan.sizes[i])
            # draw=False: with a plan no block draws, block 0 included (on its own route through Block.forward it
            # would draw a rowscale it never applies; the plan's ``lead`` draw stands for that one)
            hidden_states, residual = self.layers[i](hidden_states, residual, A=A_all[i],
                                                     rowscale=plan.masks[i - 1] if i > 0 else None,
                                                     draw=False, compact=compact)
            residual = self._compact_ran(i, hidden_states, residual)
            if hidden_states is not None:
                io = hidden_states.dtype
        return self._final_norm(hidden_states, residual)


class MixerModel_add(MixerModel):
    """reference models/point_mamba.py:281-428, the stack behind ``add_after_layer: True``: after every block the 2 k
    copies of each patch token in the SAST sequence are summed and laid out again in the same 2 k orderings
    (cross_merge.py).  Constructor, parameter names, state-dict keys (``layers.*``, ``norm_f.*``) and initialisation are
    MixerModel's.  The stack runs layer by layer in every precision: the fused out_proj + add + LayerNorm chain of
    MixerModel does not apply, the merge sits between out_proj and the add.

    ``composed`` (a test and benchmark hook): True runs the reference's own sequence of torch ops in place of the
    kernel."""

    composed = False

    def forward(self, input_ids, pos, top_k_eigenvectors, N_k_top_eigenvectors, reverse, inference_params=None, *,
                order=None):
        """Reference signature (:383).  ``input_ids`` / ``pos`` (B, L, C) in SAST sequence order, L = 2 k G;
        ``top_k_eigenvectors`` (B, G, k).  ``order`` (B, k, G), optional and specific to this implementation: the
        argsort of the eigenvectors when the caller already holds it (``spectral.spectral_order``); the reference
        re-sorts at every layer."""
        if not reverse:
            raise ValueError("MixerModel_add: add_after_layer needs reverse=True (with reverse=False the reference "
                             "discards the merge)")
        k = int(N_k_top_eigenvectors)
        if order is None:
            vecs = top_k_eigenvectors[:, :, :k]
            B, G = vecs.shape[:2]
            order = argsort_rows(vecs.transpose(1, 2).reshape(B * k, G)).view(B, k, G)
        if order.shape[1] != k or 2 * k * order.shape[2] != input_ids.shape[1]:
            raise ValueError(f"MixerModel_add: a sequence of {input_ids.shape[1]} tokens is not 2 k G with orders "
                             f"{tuple(order.shape)} and k = {k}")
        maps = None if self.composed else cross_merge_maps(order)      # once per forward, shared by all layers
        hidden_states = input_ids + pos
        residual = None
        A_all = self._precompute_A()
        for i, layer in enumerate(self.layers):
            hidden_states, residual = layer(hidden_states, residual, inference_params=inference_params, A=A_all[i])
            hidden_states = self.drop_out_in_block(hidden_states)
            hidden_states = (cross_merge_composed(hidden_states, order) if self.composed
                             else cross_merge(hidden_states, maps))
        return self._final_norm(hidden_states, residual)
