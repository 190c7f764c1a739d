"""Caller of the hot path: the reference's ``PointMamba`` classifier.

Mirrors reference models/point_mamba.py ``PointMamba`` (:431-562 constructor, :843-1125 forward with
``method`` in {"SAST" (canonical), "HLT", "MAMBA"}, ``use_wavelets=False``, ``tau=None``) with the parameter names and shapes of the
reference's own checkpoint table (logs/finetuned_hardest.log:100-426, 12.29 M parameters), so a
reference state_dict loads unchanged.  What runs on the HIP kernels: the spectral ordering
(``spectral.spectral_order``) and every Mamba mixer of ``blocks``.  ``method: "CURVE"`` is not in the reference: the
SAST route on space-filling-curve orders (``spectral.curve_order``), the baseline the method is compared with.

``Group`` (farthest-point sampling + k-NN grouping) and ``Encoder`` (mini-PointNet) sit BEFORE the
hot path ("next" row 1).  The reference gets FPS / k-NN from pytorch3d CUDA ops
(:93, :96), which are absent here: FPS and the k-NN grouping are the HIP kernels of csrc/fps.hip and
csrc/knn_group.hip, the encoder is library GEMMs around the HIP BatchNorm+ReLU / per-patch max kernels
(csrc/bn_relu.hip).
"""
from __future__ import annotations

from types import SimpleNamespace

import torch
import torch.nn as nn

from . import grouping, spectral
from .block import MixerModel, MixerModel_add
from .add_norm import add_layer_norm_fn
from .encoder_ops import bn_relu_fn, group_max_fn, token_linear, token_linear_group_max


class Group(nn.Module):
    """(B,N,3) -> neighborhood (B,G,M,3) centred, center (B,G,3), neighborhood_org; reference :76-111.

    Farthest-point sampling and the k-NN grouping run on HIP kernels (grouping.sample_farthest_points /
    grouping.knn_group, the counterparts of the pytorch3d calls at :93 and :96; clouds of up to 8192 points,
    larger ones and CPU tensors take cdist + topk).  ``fps_fn`` can be swapped (bench.py's CPU baseline plugs
    the oracle in).

    ``lengths`` (B,): ragged batches, clouds padded to a common N with ``lengths[b]`` real points each.  The padding is
    never read, and every cloud's patches are those of the cloud alone at its true length.  Every cloud needs at least
    ``max(num_group, group_size)`` points, so that all G patches of M points exist and everything downstream keeps its
    fixed shapes; that is checked with one host read of ``lengths.min()`` (not during a stream capture).
    """

    def __init__(self, num_group, group_size):
        super().__init__()
        self.num_group = num_group
        self.group_size = group_size
        self.fps_fn = grouping.sample_farthest_points

    @torch.no_grad()
    def _indices(self, xyz, lengths=None):
        if lengths is not None:
            if not (xyz.is_cuda and xyz.shape[1] <= 8192):
                raise NotImplementedError("Group: lengths are taken by the HIP kernels only (a ROCm device, clouds of "
                                          "up to 8192 points)")
            need = max(self.num_group, self.group_size)
            if not torch.cuda.is_current_stream_capturing():
                shortest = int(lengths.min())
                if shortest < need:
                    raise ValueError(f"Group: the shortest cloud has {shortest} points, every cloud needs at least "
                                     f"{need} (max of num_group = {self.num_group} and group_size = {self.group_size})")
            center, _ = self.fps_fn(xyz, self.num_group, lengths=lengths)
            return center, grouping.knn_group(center, xyz, self.group_size, lengths=lengths)
        center, _ = self.fps_fn(xyz, self.num_group)
        if xyz.is_cuda and xyz.shape[1] <= 8192:
            return center, grouping.knn_group(center, xyz, self.group_size)
        d = torch.cdist(center, xyz)
        nn_idx = d.topk(self.group_size, dim=-1, largest=False, sorted=False)[1]
        return center, nn_idx

    def forward(self, xyz, *, lengths=None):
        B, N, _ = xyz.shape
        center, nn_idx = self._indices(xyz, lengths)
        flat = (nn_idx + torch.arange(B, device=xyz.device).view(-1, 1, 1) * N).view(-1)
        nb = xyz.reshape(B * N, -1)[flat].view(B, self.num_group, self.group_size, 3).contiguous()
        return nb - center.unsqueeze(2), center, nb


class Encoder(nn.Module):
    """Mini-PointNet patch embedding; reference :42-73 (same layer names)."""

    def __init__(self, encoder_channel):
        super().__init__()
        self.encoder_channel = encoder_channel
        self.fused = True          # HIP BatchNorm+ReLU / max kernels on the GPU (False: composed torch ops)
        self.first_conv = nn.Sequential(nn.Conv1d(3, 128, 1), nn.BatchNorm1d(128), nn.ReLU(inplace=True),
                                        nn.Conv1d(128, 256, 1))
        self.second_conv = nn.Sequential(nn.Conv1d(512, 512, 1), nn.BatchNorm1d(512), nn.ReLU(inplace=True),
                                         nn.Conv1d(512, self.encoder_channel, 1))

    def forward(self, point_groups):
        """(B, G, n, 3) -> (B, G, C).  The four 1x1 convolutions are plain GEMMs on the (B*G*n, C)
        token-major view (same Conv1d / BatchNorm1d parameters, same arithmetic); this avoids the
        NCHW<->NHWC transposes MIOpen inserts around its implicit-GEMM kernels.  On the GPU the
        BatchNorm+ReLU pairs and the per-patch max run on the HIP streaming kernels (encoder_ops.py) and
        the concat of the global feature (:64-66) becomes a per-patch additive term of the second BN:
        cat([g, f]) @ W^T == f @ W[:, C:]^T + g @ W[:, :C]^T."""
        bs, g, n, _ = point_groups.shape
        c1, bn1, _, c2 = self.first_conv
        c3, bn2, _, c4 = self.second_conv
        lin = torch.nn.functional.linear
        x = point_groups.reshape(bs * g * n, 3)
        if self.fused and x.is_cuda and 256 % n == 0:
            lin = token_linear                            # same product; split-K weight gradient (encoder_ops.py)
            x = bn_relu_fn(lin(x, c1.weight.squeeze(-1), c1.bias), bn1)
            f = lin(x, c2.weight.squeeze(-1), c2.bias)                                  # (B*G*n, 256)
            cf = f.shape[1]
            fg = group_max_fn(f.view(bs * g, n, cf))                                     # (B*G, 256)
            w3 = c3.weight.squeeze(-1)
            gterm = lin(fg, w3[:, :cf], c3.bias)                                         # (B*G, 512): global half + bias
            x = bn_relu_fn(lin(f, w3[:, cf:]), bn2, gterm=gterm, group=n)
            # last layer and its max as one node: same forward; in fp32 a backward without the zeros behind the max
            return token_linear_group_max(x, c4.weight.squeeze(-1), c4.bias, n).reshape(bs, g, self.encoder_channel)
        x = torch.relu(bn1(lin(x, c1.weight.squeeze(-1), c1.bias)))
        f = lin(x, c2.weight.squeeze(-1), c2.bias).view(bs * g, n, 256)
        fg = f.max(dim=1, keepdim=True)[0]
        x = torch.cat([fg.expand(-1, n, -1), f], dim=2).reshape(bs * g * n, 512)
        x = torch.relu(bn2(lin(x, c3.weight.squeeze(-1), c3.bias)))
        f = lin(x, c4.weight.squeeze(-1), c4.bias).view(bs * g, n, self.encoder_channel)
        return f.max(dim=1)[0].reshape(bs, g, self.encoder_channel)


def default_config(**over):
    """cfgs/finetune_scan_hardest.yaml:22-49 (the config the 12.29 M parameter table belongs to)."""
    cfg = dict(trans_dim=384, depth=12, cls_dim=15, group_size=32, num_group=128, encoder_dims=384,
               rms_norm=False, drop_path=0.1, drop_out=0., method="SAST", reverse=True, knn_graph=20,
               k_top_eigenvectors=4, alpha=10., smallest=True, symmetric=True, self_loop=False,
               binary=True, matrix="laplacian")
    cfg.update(over)
    return SimpleNamespace(**cfg)


def plackett_luce_dist(logits):
    """log-probability of the identity permutation under a Plackett-Luce model (reference :2131-2132)."""
    return torch.sum(logits - torch.logcumsumexp(logits.flip(-1), dim=-1).flip(-1), dim=-1)


class PointMamba(nn.Module):
    def __init__(self, config, **kwargs):
        super().__init__()
        self.config = config
        self.trans_dim = config.trans_dim
        self.depth = config.depth
        self.cls_dim = config.cls_dim
        self.group_size = config.group_size
        self.num_group = config.num_group
        self.encoder_dims = config.encoder_dims
        self.group_divider = Group(num_group=self.num_group, group_size=self.group_size)
        self.encoder = Encoder(encoder_channel=self.encoder_dims)
        self.drop_path = getattr(config, "drop_path", 0.)
        self.rms_norm = getattr(config, "rms_norm", False)
        self.drop_out_in_block = getattr(config, "drop_out_in_block", 0.)
        self.pos_embed = nn.Sequential(nn.Linear(3, 128), nn.GELU(), nn.Linear(128, self.trans_dim))
        # add_after_layer (reference :465-480): the stack that cross-merges the orderings after every block
        self.add_after_layer = getattr(config, "add_after_layer", False)
        if self.add_after_layer and not (config.method == "SAST" and config.reverse):
            raise ValueError(f"add_after_layer=True needs method='SAST' and reverse=True, got method="
                             f"{config.method!r}, reverse={config.reverse!r}: the merge sums the 2 k orderings of a "
                             "SAST sequence (with reverse=False the reference discards it, and an HLT or MAMBA "
                             "sequence is not 2 k orderings)")
        stack = MixerModel_add if self.add_after_layer else MixerModel
        self.blocks = stack(d_model=self.trans_dim, n_layer=self.depth, rms_norm=self.rms_norm,
                            drop_out_in_block=self.drop_out_in_block, drop_path=self.drop_path)
        self.norm = nn.LayerNorm(self.trans_dim)
        self.cls_head_finetune = nn.Sequential(
            nn.Linear(self.trans_dim, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5),
            nn.Linear(256, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5),
            nn.Linear(256, self.cls_dim))
        self.loss_ce = nn.CrossEntropyLoss()
        self.drop_out = nn.Dropout(getattr(config, "drop_out", 0.))
        self.method = config.method
        self.reverse = config.reverse
        self.k_top_eigenvectors = config.k_top_eigenvectors
        self.smallest = config.smallest
        self.knn_graph = config.knn_graph
        self.symmetric = config.symmetric
        self.self_loop = config.self_loop
        self.alpha = config.alpha
        self.binary = config.binary
        self.matrix = config.matrix
        if self.method not in ("SAST", "HLT", "MAMBA", "CURVE"):
            raise NotImplementedError(f"ordering method {self.method!r}: SAST (:868), HLT (:1054) and MAMBA (:850) "
                                      "are built; the wavelet / RL research branches are out of scope")
        # method "CURVE" (not in the reference): the SAST route with space-filling-curve orders in the eigen-orders'
        # place (spectral.curve_order), one ordering per curve -- k_top_eigenvectors is not consulted
        self.curves = tuple(getattr(config, "curves", spectral.DEFAULT_CURVES))
        self.curve_bits = getattr(config, "curve_bits", 10)
        self.curve_box = getattr(config, "curve_box", "cloud")
        if self.method == "CURVE":
            spectral.curve_ids(self.curves)                                     # unknown names are refused here
        self.hlt_rand = True          # the reference's torch.rand tie-break of HLT (:1062); tests switch it off

    def get_loss_acc(self, ret, gt):
        loss = self.loss_ce(ret, gt.long())
        pred = ret.argmax(-1)
        acc = (pred == gt).sum() / float(gt.size(0))
        return loss, acc * 100

    def spectral_eigs(self, center):
        """(vals (B,k), vecs (B,G,k), order (B,k,G)) of the fused graph + eigen + argsort kernels."""
        return spectral.spectral_order(center, self.knn_graph, self.alpha, self.k_top_eigenvectors,
                                       smallest=self.smallest, symmetric=self.symmetric,
                                       self_loop=self.self_loop, binary=self.binary, matrix=self.matrix)

    def spectral_order(self, center):
        """The (B, n_orders(), G) orders the sequence is gathered by: the eigen-orders (SAST) or the curve orders."""
        if self.method == "CURVE":
            return spectral.curve_order(center, self.curves, self.curve_bits, self.curve_box)
        return self.spectral_eigs(center)[2]

    def n_orders(self):
        """Orderings in a SAST / CURVE sequence (each once more flipped with ``reverse``)."""
        return len(self.curves) if self.method == "CURVE" else self.k_top_eigenvectors

    def _on_tokens(self):
        """Is the stack handed the G distinct tokens plus an index map (SAST / CURVE / MAMBA: the sequence is a pure gather
        of them), not the assembled sequence?  Not with input dropout, which acts on every position by itself, and not
        with add_after_layer, whose stack merges whole sequences."""
        return (not self.add_after_layer and self.method in ("SAST", "CURVE", "MAMBA")
                and not (self.training and self.drop_out.p > 0))

    def seq_len(self):
        """Length of token_index()'s rows, known before the centres are."""
        if self.method == "MAMBA":
            return spectral.XYZ_ORDERS * self.num_group
        return spectral.sast_len(self.n_orders(), self.num_group, self.reverse)

    def token_index(self, center, order=None):
        """(B, seq_len()) int64 patch index of every sequence position for the routes that are pure gathers (SAST
        :868-989, MAMBA :850-866); None for HLT, whose assembly also writes zeros (:1075-1112)."""
        if self.method in ("SAST", "CURVE"):
            if order is None:
                order = self.spectral_order(center)
            return spectral.sast_index_map(order, self.reverse)
        if self.method == "MAMBA":
            return spectral.xyz_sorted_index(center)
        return None

    def order_tokens(self, tokens, pos, center, order=None):
        """Tokens and positions in sequence order for ``self.method`` (reference :850-1112)."""
        if self.method in ("SAST", "CURVE") and order is None:
            order = self.spectral_order(center)
        elif self.method == "HLT":                                              # :1054-1057: the eigenvectors
            adj = spectral.create_graph_from_centers(center, self.knn_graph, self.alpha, self.symmetric,
                                                     self.self_loop, self.binary)
            order = spectral._eig(adj, self.k_top_eigenvectors, self.smallest, False, want_all=False)[1]
        return spectral.order_tokens(self.method, (tokens, pos), center, order, self.n_orders(), self.reverse,
                                     self.hlt_rand)

    def forward(self, pts, gt=None, tau=None, use_wavelets=False, save_pts_dir=None, epoch=None, *, lengths=None,
                return_features=False):
        """Reference signature (models/point_mamba.py:843; the runner calls
        ``base_model(points, gt=None, tau=None, use_wavelets=True)``, tools/runner_finetune.py:201).  Built: the
        published spectral route (``tau is None``, ``use_wavelets=False``).  ``gt`` given -> ``(logits, policy)``
        with the reference's Plackett-Luce log-probability of the eigen-ordering (:953-955).  The learned-permutation
        (``tau``) and wavelet-traversal (``use_wavelets``) research branches are outside the hot-path scope
        (the wavelet branch calls a function the reference never defines, :879) and are
        refused by name rather than silently replaced.  ``save_pts_dir`` / ``epoch`` only feed the reference's
        point-dump visualisation and are ignored.  ``lengths`` (B,), keyword-only and not in the reference: the point
        count of every cloud of a padded batch (``Group``); only the tokeniser sees it.  ``return_features``,
        keyword-only and off by default: also return the pooled (B, trans_dim) vector the head consumes (the
        ``concat_f`` the reference's t-SNE call site, tools/runner_finetune.py:605, expects): ``(logits, features)``,
        or ``(logits, policy, features)`` with ``gt``."""
        if tau is not None:
            raise NotImplementedError("PointMamba.forward(tau=...): the learned-permutation branch (reference "
                                      "models/point_mamba.py:902-952) is outside the SI-Mamba hot-path scope")
        if use_wavelets:
            raise NotImplementedError("PointMamba.forward(use_wavelets=True): the wavelet-traversal orders (reference "
                                      "models/point_mamba.py:874-880, 957-980) are outside the SI-Mamba hot-path scope; "
                                      "call with use_wavelets=False for the spectral ordering")
        want_policy = gt is not None
        if want_policy and self.method != "SAST":
            raise NotImplementedError("PointMamba.forward(gt=...): the reference defines `policy` on the SAST route only")
        on_tokens = self._on_tokens()
        route = drop_plan = None
        if on_tokens:
            # The stack's route, asked before the tokeniser from the shape and device of the tokens it will be handed
            # (no storage behind the stand-in), and on the compact route its DropPath factors, drawn here
            # (MixerModel.draw_drop_plan): their copy to the host, which the stack waits for to plan its compact
            # batches, then finishes underneath FPS, grouping and the encoder.  Nothing between here and the blocks
            # draws from the generator on this route, so every draw keeps its place in the sequence; every other route
            # leaves the draw to the stack's entry.
            like = torch.empty_strided((pts.shape[0], self.num_group, self.trans_dim), (0, 0, 0), device=pts.device)
            route = self.blocks.route(like, self.seq_len())
            drop_plan = self.blocks.draw_drop_plan(like, lead=route.lead, route=route)
        neighborhood, center, _ = self.group_divider(pts, lengths=lengths)
        # The eigen-ordering depends only on the centres and is latency-bound on B of the 256 CUs: run it
        # on a side HIP stream underneath the (MFMA-bound) patch encoder, join before the gather.
        join = None
        if center.is_cuda and self.method == "SAST":
            join = spectral.run_on_side_stream(lambda: self.spectral_eigs(center), center)
        elif center.is_cuda and self.method == "CURVE":                         # the orders alone: no eigenpairs
            join = spectral.run_on_side_stream(lambda: (None, None, self.spectral_order(center)), center)
        tokens = self.encoder(neighborhood)
        pos = self.pos_embed(center)
        spec = join() if join is not None else None
        order = None if spec is None else spec[2]
        if self.add_after_layer:
            # :1118-1119: the stack merges the orderings after every block, so it takes the whole sequence (every
            # position through block 0, not the distinct tokens) plus the eigenvectors and their argsort
            if spec is None:
                spec = self.spectral_eigs(center)
            x, pos = self.order_tokens(tokens, pos, center, spec[2])
            x = self.drop_out(x)
            x = self.blocks(x, pos, spec[1], self.k_top_eigenvectors, self.reverse, order=spec[2])
        elif on_tokens:
            # the sequence is a gather of the G patch tokens: the stack takes the distinct tokens plus the index map
            # and runs the first block's per-token head on G instead of L positions (seq_expand.py); same result
            x = self.blocks(tokens, pos, token_index=self.token_index(center, order),
                            balanced_index=True,                                    # concatenated permutations
                            route=route, drop_plan=drop_plan)
        else:
            x, pos = self.order_tokens(tokens, pos, center, order)
            x = self.drop_out(x)
            x = self.blocks(x, pos)
        if x.is_cuda and type(self.norm) is nn.LayerNorm and x.dim() == 3:
            # the same LayerNorm through the one-pass kernels of add_norm.py (no residual: nothing is added or copied)
            x = add_layer_norm_fn(x, None, self.norm.weight, self.norm.bias, self.norm.eps,
                                  out_dtype=self.norm.weight.dtype)[0]
        else:
            x = self.norm(x)
        features = x.mean(1)
        ret = self.cls_head_finetune(features)
        if not want_policy:
            return (ret, features) if return_features else ret
        if spec is None:
            spec = self.spectral_eigs(center)
        vals, vecs, _ = spec
        ordered_vecs = torch.sort(vecs.transpose(1, 2), dim=-1)[0]                 # :954
        policy = plackett_luce_dist(-ordered_vecs).sum(-1) + plackett_luce_dist(vals)
        return (ret, policy, features) if return_features else (ret, policy)
