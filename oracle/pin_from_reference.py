"""Pin the oracle to the reference's OWN code: run the reference's function bodies here, save what they return.

    python -m oracle.pin_from_reference          # from the repo root, in the build container (needs /root/reference)
    python -m oracle.pin_from_reference --check  # regenerate into a temporary directory, report every array that differs

TEST INFRASTRUCTURE.  Writes tests/golden/ref_*; nothing of the reference's source is copied into the repository
-- the functions are read from /root/reference at run time, executed, and only their inputs and outputs are kept.

Why not ``import models.point_mamba``: its module-level imports need timm, pytorch3d, mamba_ssm and easydict, none of
which exist in this image (an ordinary ImportError, nothing was denied).  The functions on the hot path need none of
them.  So this script
  * parses the two reference files with ``ast`` and takes the definitions it needs BY NAME -- methods of
    ``PointMamba`` (models/point_mamba.py:620-841: create_graph_from_centers,
    create_graph_from_feature_space_gpu_weighted_adjacency, calc_top_k_eigenvalues_eigenvectors[_symmetric],
    sort_points_by_fiedler, multilevel_travers), the SAST token assembly and the HLT ordering / block assembly out of
    ``PointMamba.forward`` (the statements at :889-898, :982-989 and :1059-1112), ``_init_weights``, ``create_block``,
    ``MixerModel`` (:115-272) and ``Block`` (models/block.py:17-76);
  * compiles them UNMODIFIED and calls them with stock CPU torch under a ``TorchFunctionMode`` that maps the hard-coded
    ``device='cuda'`` / ``.cuda()`` / ``.to('cuda')`` to the CPU (this container has no GPU);
  * gives ``create_block`` the oracle's ``MambaRef`` as its ``Mamba`` (the real one lives in the absent mamba-ssm wheel:
    that half stays "parity unpinned") and ``Block`` a pass-through ``DropPath`` (never executed at drop_path = 0).

What the fixtures pin: adjacency, eigenpairs (same LAPACK as tests/test_oracle_spectral.py runs), orderings, the SAST
index map, the HLT order and slot map, the Add -> LayerNorm -> mixer data flow of Block / MixerModel and the
initialisation contract of _init_weights.  tests/test_oracle_pinned.py holds the oracle to them on the CPU;
tests/test_gpu_pinned.py holds the HIP path to the same files on the GPU box (where /root/reference does not exist).

The second half of this file does the same for the segmentation head, the encoder, the MAE token layout, the transforms
and the scoring (ref_seg_interp, ref_seg_fp, ref_seg_head, ref_encoder, ref_mae_flow, ref_transforms, ref_part_metrics):
modules that import cleanly (part_segmentation/models/pointnet2_utils.py, datasets/data_transforms.py) are imported whole
from their files, the rest is taken by name or by statement range with an assertion on an anchor statement.  Every float
fixture holds a float32 and a float64 run of the reference on the same fp32 inputs and ``ref32_err``, the former's error
against the latter under the metric the tests use; weights too large to commit come from tests/helpers.formula_parameters,
which the tests call as well.  tests/test_oracle_pinned_heads.py and tests/test_gpu_pinned.py read the committed files only.
"""
from __future__ import annotations

import ast
import math
import os
import sys
from functools import partial
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor
from torch.overrides import TorchFunctionMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = GOLDEN                                   # --check points this at a temporary directory
REF = "/root/reference"
REF_MODEL = os.path.join(REF, "models", "point_mamba.py")
REF_BLOCK = os.path.join(REF, "models", "block.py")

SPECTRAL_METHODS = ("create_graph_from_centers", "create_graph_from_feature_space_gpu_weighted_adjacency",
                    "calc_top_k_eigenvalues_eigenvectors", "calc_top_k_eigenvalues_eigenvectors_symmetric",
                    "sort_points_by_fiedler", "multilevel_travers")


def reference_present():
    return os.path.exists(REF_MODEL) and os.path.exists(REF_BLOCK)


class CudaToCpu(TorchFunctionMode):
    """device='cuda' -> cpu, tensor.cuda() / tensor.to('cuda') -> the tensor itself."""

    @staticmethod
    def _is_cuda(d):
        return (isinstance(d, str) and d.startswith("cuda")) or (isinstance(d, torch.device) and d.type == "cuda")

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = dict(kwargs or {})
        if func is torch.Tensor.cuda:
            return args[0]
        if func is torch.Tensor.to and len(args) >= 2 and self._is_cuda(args[1]):
            return args[0] if len(args) == 2 and not kwargs else func(args[0], "cpu", *args[2:], **kwargs)
        if self._is_cuda(kwargs.get("device")):
            kwargs["device"] = "cpu"
        return func(*args, **kwargs)


def _parse(path):
    with open(path, "r") as fh:
        return ast.parse(fh.read(), filename=path)


def _find(body, kind, name):
    for node in body:
        if isinstance(node, kind) and node.name == name:
            return node
    raise LookupError(f"{name} not found in the reference")


def _exec_defs(nodes, scope, filename):
    mod = ast.Module(body=list(nodes), type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, filename, "exec"), scope)
    return scope


def _stmts_between(fn, first, last):
    """Statements of a function body (searched recursively through if / elif / for bodies) that start in [first, last]
    at the nesting depth of the first one found."""
    def walk(body):
        hit = [n for n in body if first <= n.lineno <= last]
        if hit and hit[0].lineno == first:
            return hit
        for n in body:
            for field in ("body", "orelse"):
                sub = getattr(n, field, None)
                if isinstance(sub, list) and sub and isinstance(sub[0], ast.stmt):
                    r = walk(sub)
                    if r:
                        return r
        return None
    r = walk(fn.body)
    if not r:
        raise LookupError(f"no statement starts at line {first} of {fn.name}")
    return r


class _DropPath(nn.Module):
    """Stand-in for timm.models.layers.DropPath at drop_prob = 0 (the reference builds nn.Identity then; this class
    only has to exist so that the module-level name resolves)."""

    def __init__(self, drop_prob=0.0):
        super().__init__()
        assert drop_prob == 0.0, "the pinned fixtures are generated at drop_path = 0"

    def forward(self, x):
        return x


def load_reference():
    """-> (methods: name -> function(self, ...), sast: callable, hlt: callable, scope with Block / MixerModel / ...)."""
    from oracle.scan_ref import MambaRef

    def Mamba(d_model, layer_idx=None, device=None, dtype=None, **kw):
        """create_block passes upstream's factory keywords (models/point_mamba.py:161-162); the oracle mixer is CPU fp32."""
        assert device is None and dtype is None
        return MambaRef(d_model, layer_idx=layer_idx, **kw)

    tree = _parse(REF_MODEL)
    cls = _find(tree.body, ast.ClassDef, "PointMamba")
    scope = {"torch": torch, "nn": nn, "F": F, "np": np, "math": math, "partial": partial, "Tensor": Tensor,
             "Optional": Optional, "Mamba": Mamba, "DropPath": _DropPath, "RMSNorm": None, "layer_norm_fn": None,
             "rms_norm_fn": None}
    _exec_defs([_find(cls.body, ast.FunctionDef, m) for m in SPECTRAL_METHODS], scope, REF_MODEL)
    methods = {m: scope[m] for m in SPECTRAL_METHODS}

    # the token assembly of the SAST branch and the HLT branch, cut out of PointMamba.forward as they stand
    fwd = _find(cls.body, ast.FunctionDef, "forward")
    sast_loop = _stmts_between(fwd, 889, 898)
    sast_rev = _stmts_between(fwd, 982, 989)
    assert isinstance(sast_loop[0], ast.For) and "sort_points_by_fiedler" in ast.unparse(sast_loop[0]), \
        "reference layout changed: SAST ordering loop not at models/point_mamba.py:889"
    assert isinstance(sast_rev[0], ast.If) and "reverse" in ast.unparse(sast_rev[0].test), \
        "reference layout changed: SAST reverse block not at models/point_mamba.py:982"
    hlt = _stmts_between(fwd, 1059, 1112)
    assert "multilevel_travers" in ast.unparse(hlt[0]), "reference layout changed: HLT block not at :1059"

    def make(name, stmts, argnames, result):
        fn = ast.FunctionDef(name=name, args=ast.arguments(posonlyargs=[], args=[ast.arg(arg=a) for a in argnames],
                                                           kwonlyargs=[], kw_defaults=[], defaults=[]),
                             body=list(stmts) + [ast.Return(value=ast.Tuple(
                                 elts=[ast.Name(id=r, ctx=ast.Load()) for r in result], ctx=ast.Load()))],
                             decorator_list=[])
        _exec_defs([fn], scope, REF_MODEL)
        return scope[name]

    sast = make("_ref_sast", [sast_loop[0], sast_rev[0]], ["self", "group_input_tokens", "pos", "top_k_eigenvectors"],
                ["group_input_tokens", "pos"])
    hlt_fn = make("_ref_hlt", hlt, ["self", "group_input_tokens", "pos", "center", "top_k_eigenvectors"],
                  ["group_input_tokens", "pos", "sorted_center", "integers_arg_sort", "integers_before_random"])

    # Block (models/block.py) and the stack builders (models/point_mamba.py)
    btree = _parse(REF_BLOCK)
    _exec_defs([_find(btree.body, ast.ClassDef, "Block")], scope, REF_BLOCK)
    _exec_defs([_find(tree.body, ast.FunctionDef, "_init_weights"), _find(tree.body, ast.FunctionDef, "create_block"),
                _find(tree.body, ast.ClassDef, "MixerModel")], scope, REF_MODEL)
    return methods, sast, hlt_fn, scope


class RefSelf:
    """The attributes of PointMamba the extracted code reads, and its methods bound."""

    def __init__(self, methods, **attrs):
        self.k_top_eigenvectors, self.reverse, self.alpha = 4, True, 10.0
        for k, v in attrs.items():
            setattr(self, k, v)
        for name, fn in methods.items():
            setattr(self, name, fn.__get__(self))


def index_tokens(B, G, base):
    """(B, G, 384) tokens whose every channel is base + the token's index: what a gather leaves in channel 0 IS the
    index map it applied (sort_points_by_fiedler hard-codes 384 channels, models/point_mamba.py:822)."""
    return (base + torch.arange(G, dtype=torch.float32))[None, :, None].expand(B, G, 384).contiguous()


def spectral_fixture(name, methods, sast, hlt_fn):
    """Reference outputs on the centres of an existing fixture tests/golden/<name>.npz -> ref_<name>.npz."""
    from oracle.gen_golden import SPECTRAL_COMBOS
    centers = torch.from_numpy(np.load(os.path.join(GOLDEN, name + ".npz"))["centers"])
    B, G, _ = centers.shape
    k = 4
    # eigh's last bits depend on the LAPACK build and its thread count: recorded so that a consumer can reproduce them
    rec = {"centers": centers.numpy(), "lapack_threads": np.array(torch.get_num_threads()),
           "torch_version": np.array(torch.__version__)}
    tok, pos = index_tokens(B, G, 0.0), index_tokens(B, G, 1000.0)
    with CudaToCpu():
        for cb in SPECTRAL_COMBOS:
            me = RefSelf(methods, alpha=cb["alpha"])
            adj = me.create_graph_from_feature_space_gpu_weighted_adjacency(
                centers, cb["knn"], cb["alpha"], cb["symmetric"], cb["self_loop"], cb["binary"])
            vals, vecs, all_vals, all_vecs = me.calc_top_k_eigenvalues_eigenvectors(adj, k, True)
            order = torch.stack([me.sort_points_by_fiedler(tok, vecs[:, :, i])[:, :, 0] for i in range(k)], 1)
            x, p = sast(me, tok, pos, vecs)
            assert torch.equal(p, x + 1000.0)                  # tokens and pos go through the same map
            t = cb["tag"]
            rec[f"{t}.adj"] = adj.numpy()
            rec[f"{t}.vals"], rec[f"{t}.vecs"] = vals.numpy(), vecs.numpy()
            rec[f"{t}.all_vals"] = all_vals.numpy()
            rec[f"{t}.order"] = order.long().numpy()           # (B, k, G)
            rec[f"{t}.sast_index"] = x[:, :, 0].long().numpy()  # (B, 2 k G)
        cb = SPECTRAL_COMBOS[0]
        me = RefSelf(methods, alpha=cb["alpha"])
        adj = me.create_graph_from_feature_space_gpu_weighted_adjacency(
            centers, cb["knn"], cb["alpha"], cb["symmetric"], cb["self_loop"], cb["binary"])
        v, e, _, _ = me.calc_top_k_eigenvalues_eigenvectors_symmetric(adj, k, True)
        rec["hardest.sym.vals"], rec["hardest.sym.vecs"] = v.numpy(), e.numpy()
        v, e, _, _ = me.calc_top_k_eigenvalues_eigenvectors(adj, k, False)
        rec["hardest.largest.vals"], rec["hardest.largest.vecs"] = v.numpy(), e.numpy()
        # create_graph_from_centers: the alpha == 0 branch reads self.alpha (sigma = mean distance of the batch), and
        # the weighted form the segmentation config uses
        me0 = RefSelf(methods, alpha=0)
        rec["sigma_mean.adj"] = me0.create_graph_from_centers(centers, 10, 0.0, True, True, False).numpy()
        mew = RefSelf(methods, alpha=10.0)
        adjc = mew.create_graph_from_centers(centers, 10, 10.0, True, True, False)
        rec["centers_graph.adj"] = adjc.numpy()
        # HLT (models/point_mamba.py:1056-1112) on that graph, k = 3 levels, with the reference's own torch.rand
        # tie-break drawn from a seeded generator: the consumer redraws it with the same seed
        meh = RefSelf(methods, alpha=10.0, k_top_eigenvectors=3)
        _, hv, _, _ = meh.calc_top_k_eigenvalues_eigenvectors(adjc, 3, True)
        torch.manual_seed(1234)
        ht, hp, hc, horder, hcodes = hlt_fn(meh, index_tokens(B, G, 1.0), index_tokens(B, G, 1001.0), centers, hv)
        rec["hlt.vecs"] = hv.numpy()
        rec["hlt.codes"] = hcodes.long().numpy()
        rec["hlt.order"] = horder.long().numpy()
        rec["hlt.tokens_index"] = ht[:, :, 0].numpy()          # (B, 2 G): 1 + token index per slot, 0 where nothing is written
        rec["hlt.pos_index"] = hp[:, :, 0].numpy()
        rec["hlt.center"] = hc.numpy()
        rec["hlt.rand_seed"] = np.array(1234)
    np.savez_compressed(os.path.join(OUT, "ref_" + name + ".npz"), **rec)
    return rec


def stack_fixture(scope):
    """The reference's own create_block / Block / MixerModel / _init_weights around the oracle mixer -> ref_stack.npz."""
    MixerModel, create_block = scope["MixerModel"], scope["create_block"]
    d, n_layer, B, L = 64, 3, 2, 24
    torch.manual_seed(7)
    with CudaToCpu():
        model = MixerModel(d_model=d, n_layer=n_layer, rms_norm=False, drop_path=0.0)
        g = torch.Generator().manual_seed(8)
        x = torch.randn(B, L, d, generator=g, requires_grad=True)
        pos = torch.randn(B, L, d, generator=g, requires_grad=True)
        dout = torch.randn(B, L, d, generator=g)
        out = model(x, pos)
        out.backward(dout)
        # one Block on its own, both call forms (models/block.py:56-58)
        blk = create_block(d, layer_idx=0)
        blk.load_state_dict(model.layers[0].state_dict())
        h = torch.randn(B, L, d, generator=g)
        r = torch.randn(B, L, d, generator=g)
        h1, r1 = blk(h, None)
        h2, r2 = blk(h, r)
    rec = {"x": x.detach().numpy(), "pos": pos.detach().numpy(), "dout": dout.numpy(), "out": out.detach().numpy(),
           "grad_x": x.grad.numpy(), "grad_pos": pos.grad.numpy(),
           "block.h": h.numpy(), "block.r": r.numpy(), "block.first.h": h1.detach().numpy(),
           "block.first.r": r1.detach().numpy(), "block.next.h": h2.detach().numpy(),
           "block.next.r": r2.detach().numpy(), "dims": np.array([d, n_layer, B, L])}
    names = []
    for k, v in model.state_dict().items():
        rec["param." + k] = v.numpy()
        names.append(k)
    for k, p_ in model.named_parameters():
        rec["grad." + k] = p_.grad.numpy()
    rec["param_names"] = np.array(names)
    # what _init_weights leaves behind (models/point_mamba.py:122-144): Linear biases zero unless _no_reinit,
    # out_proj.weight re-drawn kaiming_uniform(a = sqrt 5) / sqrt(n_layer)
    bound = 1.0 / math.sqrt(2 * d) / math.sqrt(n_layer)       # kaiming_uniform(a = sqrt 5): U(+-1/sqrt(fan_in))
    rec["init.out_proj_bound"] = np.array(bound)
    rec["init.out_proj_absmax"] = np.array([model.layers[i].mixer.out_proj.weight.abs().max().item()
                                            for i in range(n_layer)])
    np.savez_compressed(os.path.join(OUT, "ref_stack.npz"), **rec)
    return rec


def create_block_fixture():
    """The reference's own create_block / Block / _init_weights building THIS package's Mamba through the import shim
    -> ref_create_block.json: the call create_block makes to Mamba, the block's state-dict names and shapes in order,
    and which parameters _init_weights re-draws."""
    import json
    import si_mamba_amd
    si_mamba_amd.install_shim()
    from mamba_ssm.modules.mamba_simple import Mamba          # the reference's import line, models/point_mamba.py:25
    calls = []

    def recording_mamba(*args, **kwargs):
        calls.append({"args": list(args), "kwargs": kwargs})
        return Mamba(*args, **kwargs)

    scope = {"torch": torch, "nn": nn, "F": F, "math": math, "partial": partial, "Tensor": Tensor,
             "Optional": Optional, "Mamba": recording_mamba, "DropPath": _DropPath, "RMSNorm": None,
             "layer_norm_fn": None, "rms_norm_fn": None}
    _exec_defs([_find(_parse(REF_BLOCK).body, ast.ClassDef, "Block")], scope, REF_BLOCK)
    tree = _parse(REF_MODEL)
    _exec_defs([_find(tree.body, ast.FunctionDef, "_init_weights"),
                _find(tree.body, ast.FunctionDef, "create_block")], scope, REF_MODEL)
    torch.manual_seed(0)
    blk = scope["create_block"](384, layer_idx=0, drop_path=0.0)
    before = {k: v.clone() for k, v in blk.state_dict().items()}
    blk.apply(partial(scope["_init_weights"], n_layer=12))
    rec = {"source": "reference models/point_mamba.py create_block, _init_weights; models/block.py Block",
           "create_block": {"d_model": 384, "layer_idx": 0, "drop_path": 0.0}, "init_n_layer": 12,
           "mamba_calls": calls, "block_layer_idx": blk.layer_idx,
           "state_dict": [[k, list(v.shape)] for k, v in blk.state_dict().items()],
           "reinitialised": [k for k, v in blk.state_dict().items() if not torch.equal(v, before[k])]}
    with open(os.path.join(OUT, "ref_create_block.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    return rec


# ---- the segmentation, encoder, transform and scoring half ------------------------------------------------------------
REF_FP = os.path.join(REF, "part_segmentation", "models", "pointnet2_utils.py")
REF_TRANSFORMS = os.path.join(REF, "datasets", "data_transforms.py")
REF_SEG_MAIN = os.path.join(REF, "part_segmentation", "main.py")


def _helpers():
    """tests/helpers.py (the metrics and the integer-formula parameters the tests use as well)."""
    tests = os.path.join(ROOT, "tests")
    if tests not in sys.path:
        sys.path.insert(0, tests)
    import helpers
    return helpers


def _pinned_cases():
    _helpers()
    import pinned_cases
    return pinned_cases


def _import_file(name, path):
    """A reference module that imports cleanly, loaded whole from its file."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _make_fn(scope, name, stmts, argnames, result, filename):
    """Extracted statements as the body of a function of ``argnames`` that returns the names in ``result``."""
    fn = ast.FunctionDef(name=name, args=ast.arguments(posonlyargs=[], args=[ast.arg(arg=a) for a in argnames],
                                                       kwonlyargs=[], kw_defaults=[], defaults=[]),
                         body=list(stmts) + [ast.Return(value=ast.Tuple(
                             elts=[ast.Name(id=r, ctx=ast.Load()) for r in result], ctx=ast.Load()))],
                         decorator_list=[])
    _exec_defs([fn], scope, filename)
    return scope[name]


class deterministic_backward:
    """The reference's gather ``points2[batch_indices, idx, :]`` has an index_put with accumulation as its backward; on
    the CPU that adds in thread order unless torch is told to be deterministic, and the fp32 gradient (hence ref32_err)
    would differ from run to run."""

    def __enter__(self):
        self.before = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(True)

    def __exit__(self, *exc):
        torch.use_deterministic_algorithms(self.before)
        return False


class RecordInterp(TorchFunctionMode):
    """What PointNetFeaturePropagation.forward holds between its sort and its weighted sum, taken from the module's
    own calls: the sort's first three columns (pointnet2_utils.py:294-295), the weights as they enter
    ``weight.view(B, N, 3, 1)`` (:300).  Nothing is computed again."""

    def __init__(self):
        super().__init__()
        self.rec = {}

    def __torch_function__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if func is torch.Tensor.sort:
            self.rec["d"], self.rec["idx"] = out[0][:, :, :3].clone(), out[1][:, :, :3].clone()
            self.rec["d_all"] = out[0].clone()
        elif func is torch.Tensor.view and len(args) == 5 and tuple(args[3:]) == (3, 1):
            self.rec["w"] = args[0].clone()
        return out


def interp_inputs():
    """The four cases of ref_seg_interp.npz: name -> (points (B,N,3), centres (B,S,3), feats (B,S,C)), fp32."""
    h = _helpers()
    B, N, S, C = 2, 300, 37, 36
    g = torch.Generator().manual_seed(41)
    pts = h.clouds_from(B, N, g)
    pick = torch.stack([torch.randperm(N, generator=g)[:S] for _ in range(B)])
    centres = torch.stack([pts[b, pick[b]] for b in range(B)])                  # a subset of the points, as after FPS
    p1, p2 = torch.randperm(S, generator=g), torch.randperm(S, generator=g)
    sequence = torch.cat([centres, centres.flip(1), centres[:, p1], centres[:, p2]], 1)   # every centre four times
    feats = lambda s: torch.randn(B, s, C, generator=g)                         # noqa: E731
    return {"distinct": (pts, centres, feats(S)), "sequence": (pts, sequence, feats(4 * S)),
            "three": (pts, centres[:, :3].contiguous(), feats(3)), "one": (pts, centres[:, :1].contiguous(), feats(1))}


def interp_fixture(fp_mod):
    """pointnet2_utils.PointNetFeaturePropagation with an empty MLP and points1 = None: the bare interpolation, in
    float32 and in float64 on the same fp32 inputs -> ref_seg_interp.npz."""
    h = _helpers()
    rec = {}
    for case, (pts, centres, feats) in interp_inputs().items():
        rec[f"{case}.xyz2"], rec[f"{case}.feats"] = centres.numpy(), feats.numpy()
        dout = torch.randn(pts.shape[0], pts.shape[1], feats.shape[-1], generator=torch.Generator().manual_seed(47))
        rec["xyz1"], rec["dout"] = pts.numpy(), dout.numpy()                    # the same for every case
        got = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            fp = fp_mod.PointNetFeaturePropagation(feats.shape[-1], [])
            f = feats.to(dt).transpose(1, 2).contiguous().requires_grad_(True)
            with CudaToCpu(), deterministic_backward(), RecordInterp() as r:
                out = fp(pts.to(dt).transpose(1, 2), centres.to(dt).transpose(1, 2), None, f)
                out.backward(dout.to(dt).transpose(1, 2))                     # the reference's own autograd
            got[tag] = dict(r.rec, out=out.detach().transpose(1, 2).contiguous(),
                            dfeats=f.grad.transpose(1, 2).contiguous())
            for k, v in got[tag].items():
                if k != "d_all" and (k, tag) != ("dfeats", "32"):
                    rec[f"{case}.{k}{tag}"] = v.numpy()
        rec[f"{case}.ref32_err.out"] = np.array(h.peak_err(got["32"]["out"], got["64"]["out"]))
        rec[f"{case}.ref32_err.dfeats"] = np.array(h.peak_err(got["32"]["dfeats"], got["64"]["dfeats"]))
        if "d" in got["32"]:
            rec[f"{case}.ref32_err.d"] = np.array(h.peak_err(got["32"]["d"], got["64"]["d"]))
            rec[f"{case}.ref32_err.w"] = np.array(h.peak_err(got["32"]["w"], got["64"]["w"]))
            rec[f"{case}.d_min32"] = np.array(got["32"]["d_all"].min().item())      # negative at coincident points
            if got["32"]["d_all"].shape[-1] > 3:
                rec[f"{case}.d4_32"] = got["32"]["d_all"][:, :, 3].numpy()             # the fourth distance: tie detector
    np.savez_compressed(os.path.join(OUT, "ref_seg_interp.npz"), **rec)
    return rec


def _grads(module, leaves):
    out = {"grad." + k: p.grad.detach().clone() for k, p in module.named_parameters()}
    out.update({"grad." + k: v.grad.detach().clone() for k, v in leaves.items()})
    return out


def fp_fixture(fp_mod):
    """The full propagation, MLP [32, 16], points1 = the points, centres of the ``distinct`` case, parameters from
    helpers.formula_parameters(salt 100) -> ref_seg_fp.npz: train mode (forward, updated running statistics, the
    reference's own autograd gradients) and eval mode on formula running statistics, each in float32 and float64."""
    h = _helpers()
    pts, centres, feats = interp_inputs()["distinct"]
    B, N, _ = pts.shape
    dout = torch.randn(B, 16, N, generator=torch.Generator().manual_seed(42))
    rec = {"xyz1": pts.numpy(), "xyz2": centres.numpy(), "points2": feats.numpy(), "dout": dout.numpy(),
           "mlp": np.array([32, 16]), "salt": np.array(100)}
    for mode in ("train", "eval"):
        got = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            fp = h.formula_parameters(fp_mod.PointNetFeaturePropagation(3 + feats.shape[-1], [32, 16]), 100,
                                      running=(mode == "eval")).to(dt)
            fp.train(mode == "train")
            p2 = feats.to(dt).transpose(1, 2).contiguous().requires_grad_(True)
            x1 = pts.to(dt).transpose(1, 2)
            with CudaToCpu(), deterministic_backward():
                out = fp(x1, centres.to(dt).transpose(1, 2), x1, p2)
                out.backward(dout.to(dt))
            g = {"out": out.detach().transpose(1, 2).contiguous()}                 # token-major (B, N, 16)
            g.update(_grads(fp, {}))
            g["grad.points2"] = p2.grad.transpose(1, 2).contiguous()                  # (B, S, C)
            for k, b in fp.named_buffers():
                if "running" in k:
                    g["stat." + k] = b.detach().clone()
            got[tag] = g
        for k in got["64"]:
            rec[f"{mode}.{k}64"] = got["64"][k].numpy()
            rec[f"{mode}.ref32_err.{k}"] = np.array(h.nerr(got["32"][k], got["64"][k]))
        rec[f"{mode}.out32"] = got["32"]["out"].numpy()
    np.savez_compressed(os.path.join(OUT, "ref_seg_fp.npz"), **rec)
    return rec


def encoder_inputs():
    """name -> point groups (B, G, n, 3) of ref_encoder.npz; patch (0, 1) holds point 3 again at row 7, so that both max
    reductions of the encoder see an exact tie there."""
    out = {}
    for name, n, seed in (("n32", 32, 43), ("n16", 16, 44)):
        g = torch.Generator().manual_seed(seed)
        pg = 0.3 * torch.randn(2, 5, n, 3, generator=g)
        pg[0, 1, 7] = pg[0, 1, 3]
        out[name] = pg
    return out


ENCODER_DUP = (0, 1, 3, 7)          # (sample, patch, row, the row that repeats it)


def encoder_fixture():
    """models/point_mamba.py Encoder (:42-73), the class extracted by name (the module needs absent wheels), at
    encoder_channel 384 with parameters from helpers.formula_parameters(salt 200) -> ref_encoder.npz."""
    h = _helpers()
    tree = _parse(REF_MODEL)
    node = _find(tree.body, ast.ClassDef, "Encoder")
    assert "first_conv" in ast.unparse(node) and "second_conv" in ast.unparse(node), "reference layout changed: Encoder"
    scope = _exec_defs([node], {"torch": torch, "nn": nn}, REF_MODEL)
    rec = {"salt": np.array(200), "encoder_channel": np.array(384), "dup": np.array(ENCODER_DUP)}
    for name, pg in encoder_inputs().items():
        bs, g_, n, _ = pg.shape
        dout = torch.randn(bs, g_, 384, generator=torch.Generator().manual_seed(45))
        rec[f"{name}.points"], rec[f"{name}.dout"] = pg.numpy(), dout.numpy()
        for mode in ("train", "eval"):
            got = {}
            for tag, dt in (("32", torch.float32), ("64", torch.float64)):
                enc = h.formula_parameters(scope["Encoder"](384), 200, running=(mode == "eval")).to(dt)
                enc.train(mode == "train")
                x = pg.to(dt).clone().requires_grad_(True)
                with CudaToCpu():
                    out = enc(x)
                    out.backward(dout.to(dt))
                gp = x.grad.clone()
                b, p, r0, r1 = ENCODER_DUP
                gp[b, p, r0] += gp[b, p, r1]               # which duplicate the max's gradient goes to is unspecified
                gp[b, p, r1] = 0
                res = {"out": out.detach(), "grad.points_dupsum": gp}
                for k, prm in enc.named_parameters():
                    res["gnorm." + k] = prm.grad.norm().reshape(1)
                    res["gsample." + k] = prm.grad.flatten()[::_pinned_cases().sample_stride(prm.numel())].clone()
                for k, buf in enc.named_buffers():
                    if "running" in k:
                        res["stat." + k] = buf.detach().clone()
                got[tag] = res
            for k in got["64"]:
                rec[f"{name}.{mode}.{k}64"] = got["64"][k].numpy()
                rec[f"{name}.{mode}.ref32_err.{k}"] = np.array(h.nerr(got["32"][k], got["64"][k]))
            rec[f"{name}.{mode}.out32"] = got["32"]["out"].numpy()
    np.savez_compressed(os.path.join(OUT, "ref_encoder.npz"), **rec)
    return rec


class _RecordedNumpy:
    """Stand-in for the transforms module's ``np``: numpy itself, except that ``np.random`` draws from a seeded
    RandomState and keeps every draw in order."""

    class _Random:
        def __init__(self, seed, log):
            self._rs, self._log = np.random.RandomState(seed), log

        def uniform(self, low=0.0, high=1.0, size=None):
            v = self._rs.uniform(low, high, size)
            self._log.append(np.atleast_1d(np.asarray(v, dtype=np.float64)).copy())
            return v

        def random(self, size=None):
            v = self._rs.random_sample(size)
            self._log.append(np.atleast_1d(np.asarray(v, dtype=np.float64)).copy())
            return v

    def __init__(self, seed, log):
        self.random = self._Random(seed, log)

    def __getattr__(self, name):
        return getattr(np, name)


class _RecordedRandom:
    """Stand-in for the transforms module's ``random``."""

    def __init__(self, seed, log):
        import random as _random
        self._r, self._log = _random.Random(seed), log

    def random(self):
        v = self._r.random()
        self._log.append(np.array([v]))
        return v


class RecordNormal(TorchFunctionMode):
    """Keeps what PointcloudJitter's own ``normal_`` returned (before its clamp)."""

    def __init__(self):
        super().__init__()
        self.noise = []

    def __torch_function__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if func is torch.Tensor.normal_:
            self.noise.append(out.clone())
        return out


TRANSFORMS = ("PointcloudRotate", "PointcloudScaleAndTranslate", "PointcloudJitter", "PointcloudScale",
              "PointcloudTranslate", "PointcloudRandomInputDropout", "RandomHorizontalFlip")


def transforms_fixture():
    """datasets/data_transforms.py imported whole; its module-level ``np`` / ``random`` replaced by recording stand-ins
    -> ref_transforms.npz: per class the input (3, 50, 3), the draws of every cloud in call order, the output."""
    h = _helpers()
    mod = _import_file("_ref_data_transforms", REF_TRANSFORMS)
    B, N = 3, 50
    rec = {"classes": np.array(TRANSFORMS)}
    for k, name in enumerate(TRANSFORMS):
        log = []
        mod.np, mod.random = _RecordedNumpy(500 + k, log), _RecordedRandom(600 + k, log)
        pc = h.clouds(B, N, 50 + k)
        rec[f"{name}.in"] = pc.numpy().copy()
        torch.manual_seed(700 + k)
        with CudaToCpu(), RecordNormal() as rn:
            out = getattr(mod, name)()(pc.clone())
        rec[f"{name}.out"] = out.numpy()
        rec[f"{name}.draws"] = np.concatenate(log) if log else np.zeros(0)
        rec[f"{name}.draw_lens"] = np.array([len(v) for v in log], dtype=np.int64)
        if rn.noise:
            rec[f"{name}.noise"] = torch.stack(rn.noise).numpy()                    # (B, N, 3), already times std
    flipped = (rec["RandomHorizontalFlip.in"] != rec["RandomHorizontalFlip.out"]).any(1)[:, :2]
    assert flipped.any() and not flipped.all(), "choose seeds so that the flip both fires and does not"
    dropped = (rec["PointcloudRandomInputDropout.in"] != rec["PointcloudRandomInputDropout.out"]).any(-1).sum(1)
    assert (dropped > 0).all(), "choose seeds so that every cloud drops points"
    np.savez_compressed(os.path.join(OUT, "ref_transforms.npz"), **rec)
    return rec


def part_metrics_inputs(seg_classes):
    """Two batches (4, 64, 50) of logits and (4, 64) targets.  Shape 0 of batch 0 (Motorbike) never holds part 35 and
    its logit is pushed down (absent and unpredicted: IoU 1.0); shape 1 (Chair) never holds part 15 but is free to
    predict it (predicted but absent); eight shapes over six categories leave most of the 50 labels unseen."""
    g = torch.Generator().manual_seed(46)
    cats = [["Motorbike", "Chair", "Airplane", "Lamp"], ["Table", "Motorbike", "Mug", "Chair"]]
    batches = []
    for names in cats:
        logits = torch.randn(4, 64, 50, generator=g)
        target = torch.zeros(4, 64, dtype=torch.int64)
        for i, c in enumerate(names):
            labels = torch.tensor(seg_classes[c])
            target[i] = labels[torch.randint(0, len(labels), (64,), generator=g)]
            hit = torch.rand(64, generator=g) < 0.6                       # most points predicted right
            logits[i, hit, target[i, hit]] += 4.0
        batches.append((logits, target))
    l0, t0 = batches[0]
    t0[0][t0[0] == 35] = 30
    l0[0, :, 35] = -50.0
    t0[1][t0[1] == 15] = 12
    l0[1, :8, 15] = 50.0
    return batches


def part_metrics_fixture():
    """The evaluation statements part_segmentation/main.py:270-334, extracted as they stand, over the two batches ->
    ref_part_metrics.npz."""
    import json
    import warnings
    with open(os.path.join(GOLDEN, "shapenetpart_seg_classes.json")) as fh:
        seg_classes = json.load(fh)
    fn_main = _find(_parse(REF_SEG_MAIN).body, ast.FunctionDef, "main")
    stmts = _stmts_between(fn_main, 270, 334)
    assert "test_metrics" in ast.unparse(stmts[0]) and "inctance_avg_iou" in ast.unparse(stmts[-1]), \
        "reference layout changed: evaluation loop not at part_segmentation/main.py:270-334"
    batches = part_metrics_inputs(seg_classes)

    class Classifier:
        def __init__(self):
            self.queue = [b[0] for b in batches]

        def eval(self):
            return self

        def __call__(self, points, label):
            return self.queue.pop(0)

    scope = {"np": np, "torch": torch, "tqdm": lambda it, **kw: it, "log_string": lambda s: None,
             "to_categorical": lambda y, n: None, "seg_classes": seg_classes, "num_part": 50, "num_classes": 16}
    fn = _make_fn(scope, "_ref_eval", stmts, ["classifier", "testDataLoader"],
                  ["test_metrics", "shape_ious", "all_shape_ious", "total_seen_class", "total_correct_class"],
                  REF_SEG_MAIN)
    loader = [(torch.zeros(4, 64, 3), torch.zeros(4, 1), t) for _, t in batches]
    with CudaToCpu(), warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")                       # the reference's own 0/0 and mean of an empty list
        metrics, cat_iou, all_ious, seen, correct = fn(Classifier(), loader)
    rec = {"categories": np.array(list(cat_iou.keys())),
           "category_iou": np.array([float(v) for v in cat_iou.values()]),
           "all_shape_ious": np.array(all_ious, dtype=np.float64),
           "seen_class": np.array(seen, dtype=np.int64), "correct_class": np.array(correct, dtype=np.int64)}
    for k, v in metrics.items():
        rec["metric." + k] = np.array(float(v))
    for i, (lg, t) in enumerate(batches):
        rec[f"batch{i}.logits"], rec[f"batch{i}.target"] = lg.numpy(), t.numpy()
    np.savez_compressed(os.path.join(OUT, "ref_part_metrics.npz"), **rec)
    return rec


REF_SEG_MODEL = os.path.join(REF, "part_segmentation", "models", "pt_mamba.py")
# get_model's own layer sizes at trans_dim = 64 (pt_mamba.py: propagation_0 mlp [4 trans_dim, 1024], convs 512 / 256)
HEAD_DIMS = dict(d=64, n_layer=4, fetch_idx=(1, 2, 3), B=2, L=24, N=128, cls_dim=50, fp_mlp=(256, 1024), c1=512, c2=256)


def head_fixture(fp_mod):
    """-> ref_seg_head.npz, two parts.
    (a) MixerModelForSegmentation.forward (part_segmentation/models/pt_mamba.py:390-416) over that file's own Block /
        create_block / MixerModel / _init_weights, with the oracle's MambaRef standing in for Mamba: the taps.
    (b) the head statements get_model.forward :768-787, extracted as statements; ``self`` carries plain torch modules with
        helpers.formula_head(salt 300) parameters and the reference's PointNetFeaturePropagation as ``propagation_0``.  The
        L centres are distinct (ties belong to ref_seg_interp's ``sequence``).  Eval mode, and train mode with dp1 at p = 0
        (the dropout's draws cannot be compared)."""
    from typing import Tuple
    from oracle.scan_ref import MambaRef
    h = _helpers()
    D = HEAD_DIMS
    d, B, L, N = D["d"], D["B"], D["L"], D["N"]

    def Mamba(d_model, layer_idx=None, device=None, dtype=None, **kw):
        assert device is None and dtype is None
        return MambaRef(d_model, layer_idx=layer_idx, **kw)

    tree = _parse(REF_SEG_MODEL)
    scope = {"torch": torch, "nn": nn, "F": F, "math": math, "partial": partial, "Tensor": Tensor, "Optional": Optional,
             "Tuple": Tuple, "Mamba": Mamba, "DropPath": _DropPath, "RMSNorm": None, "layer_norm_fn": None,
             "rms_norm_fn": None}
    _exec_defs([_find(tree.body, ast.ClassDef, "Block"), _find(tree.body, ast.FunctionDef, "create_block"),
                _find(tree.body, ast.FunctionDef, "_init_weights"), _find(tree.body, ast.ClassDef, "MixerModel"),
                _find(tree.body, ast.ClassDef, "MixerModelForSegmentation")], scope, REF_SEG_MODEL)
    fwd = _find(_find(tree.body, ast.ClassDef, "get_model").body, ast.FunctionDef, "forward")
    stmts = _stmts_between(fwd, 768, 787)
    assert "self.norm" in ast.unparse(stmts[0]) and isinstance(stmts[-1], ast.Return) \
        and "permute" in ast.unparse(stmts[-2]), \
        "reference layout changed: head not at part_segmentation/models/pt_mamba.py:768-787"
    head = _make_fn(scope, "_ref_head", stmts, ["self", "feature_list", "pts", "cls_label", "sorted_center", "B", "N"],
                    ["x"], REF_SEG_MODEL)                      # the statements end in the reference's own ``return x``

    g = torch.Generator().manual_seed(48)
    x, pos = torch.randn(B, L, d, generator=g), torch.randn(B, L, d, generator=g)
    pts = h.clouds_from(B, N, g)
    centres = torch.stack([pts[b, torch.randperm(N, generator=g)[:L]] for b in range(B)])
    label = torch.nn.functional.one_hot(torch.tensor([3, 7]), 16).float()
    rec = {"x": x.numpy(), "pos": pos.numpy(), "pts": pts.numpy(), "sorted_center": centres.numpy(),
           "cls_label": label.numpy(), "salt": np.array(300)}
    torch.manual_seed(9)
    with CudaToCpu():
        model = scope["MixerModelForSegmentation"](d_model=d, n_layer=D["n_layer"], rms_norm=False, drop_path=0.0,
                                                   fetch_idx=list(D["fetch_idx"]))
    names = []
    for k, v in model.state_dict().items():
        rec["param." + k] = v.numpy().copy()
        names.append(k)
    rec["param_names"] = np.array(names)

    class HeadSelf(nn.Module):
        def __init__(self):
            super().__init__()
            nf = len(D["fetch_idx"]) * d
            self.norm = nn.LayerNorm(d)
            self.label_conv = nn.Sequential(nn.Conv1d(16, 64, kernel_size=1, bias=False), nn.BatchNorm1d(64),
                                            nn.LeakyReLU(0.2))
            self.propagation_0 = fp_mod.PointNetFeaturePropagation(in_channel=nf + 3, mlp=list(D["fp_mlp"]))
            self.convs1 = nn.Conv1d(D["fp_mlp"][-1] + 2 * nf + 64, D["c1"], 1)
            self.bns1 = nn.BatchNorm1d(D["c1"])
            self.convs2 = nn.Conv1d(D["c1"], D["c2"], 1)
            self.bns2 = nn.BatchNorm1d(D["c2"])
            self.convs3 = nn.Conv1d(D["c2"], D["cls_dim"], 1)
            self.relu = nn.ReLU()

    taps = {}
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        m = model.to(dt)
        with CudaToCpu(), torch.no_grad():
            taps[tag] = [t.clone() for t in m(x.to(dt), pos.to(dt))]
    model.float()
    for i in range(len(D["fetch_idx"])):
        rec[f"tap{i}.32"], rec[f"tap{i}.out64"] = taps["32"][i].numpy(), taps["64"][i].numpy()
        rec[f"tap{i}.ref32_err.out"] = np.array(h.nerr(taps["32"][i], taps["64"][i]))
    for mode in ("train", "eval"):
        got = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            me = h.formula_head(HeadSelf(), 300, running=(mode == "eval"))
            me.dp1 = nn.Dropout(0.5 if mode == "eval" else 0.0)
            me = me.to(dt).train(mode == "train")
            with CudaToCpu(), torch.no_grad():
                out = head(me, [t.to(dt) for t in taps["32"]], pts.to(dt), label.to(dt), centres.to(dt), B, N)
            res = {"out": out.clone()}
            for k, buf in me.named_buffers():
                if "running" in k:
                    res["stat." + k] = buf.detach().clone()
            got[tag] = res
        for k in got["64"]:
            rec[f"{mode}.{k}64"] = got["64"][k].numpy()
            rec[f"{mode}.ref32_err.{k}"] = np.array(h.nerr(got["32"][k], got["64"][k]))
        rec[f"{mode}.out32"] = got["32"]["out"].numpy()
    np.savez_compressed(os.path.join(OUT, "ref_seg_head.npz"), **rec)
    return rec


MAE_DIMS = dict(B=2, G=16, k=4, M=4, C=3, mask_ratio=0.6)


def mae_inputs():
    """Index-coded tensors (the trick of index_tokens): what a gather leaves in channel 0 IS the index map it applied.
    tokens 1 + g, pos 1001 + g, neighbourhoods 2001 + g, centres 3001 + g, mask token -1; orders: k random permutations."""
    D = MAE_DIMS
    B, G, k, M, C = D["B"], D["G"], D["k"], D["M"], D["C"]
    gen = torch.Generator().manual_seed(49)
    orders = torch.stack([torch.stack([torch.randperm(G, generator=gen) for _ in range(k)]) for _ in range(B)])
    code = lambda base, *tail: (base + torch.arange(G, dtype=torch.float32)).view(1, G, *[1] * len(tail)).expand(
        B, G, *tail).contiguous()                                                      # noqa: E731
    return dict(orders=orders, tokens=code(1.0, C), pos=code(1001.0, C), neighborhood=code(2001.0, M, 3),
                center=code(3001.0, 3), geometry=_helpers().clouds_from(B, G, gen))   # real centres for the block mask


def mae_fixture():
    """-> ref_mae_flow.npz.  MaskMamba_2._mask_center_rand (:2232-2255) under np.random.seed and _mask_center_block
    (:2203-2230) under random.seed; the ``orders`` branch of MaskMamba_2.forward (:2453-2538) and the restore loop, the
    final mask and the ground-truth selection of Point_MAE_Mamba.forward (:3139-3202), all extracted as they stand and
    run on index-coded tokens with identity ``blocks`` / ``norm`` / ``MAE_decoder`` / ``increase_dim``.  k = 4: the
    restore loop hard-codes ``cnt = 4`` (:3174) and cannot run at another k.  Chamfer (pytorch3d, absent) stays unpinned."""
    import random as _random
    from types import SimpleNamespace
    D = MAE_DIMS
    B, G, k = D["B"], D["G"], D["k"]
    tree = _parse(REF_MODEL)
    enc_cls = _find(tree.body, ast.ClassDef, "MaskMamba_2")
    scope = {"torch": torch, "np": np, "random": _random, "nn": nn, "F": F}
    _exec_defs([_find(enc_cls.body, ast.FunctionDef, "_mask_center_rand"),
                _find(enc_cls.body, ast.FunctionDef, "_mask_center_block")], scope, REF_MODEL)
    enc_fwd = _find(enc_cls.body, ast.FunctionDef, "forward")
    enc_stmts = _stmts_between(enc_fwd, 2453, 2538)
    assert isinstance(enc_stmts[0], ast.If) and "orders is not None" in ast.unparse(enc_stmts[0].test) \
        and "self.norm" in ast.unparse(enc_stmts[-1]), "reference layout changed: orders branch not at :2453-2538"
    encoder = _make_fn(scope, "_ref_mae_encoder", enc_stmts,
                       ["self", "orders", "orders_soft", "bool_masked_pos", "group_input_tokens", "pos", "neighborhood",
                        "center", "batch_size", "C", "reverse"],
                       ["x_vis", "sorted_bool_masked_pos_list", "sorted_pos_mask", "sorted_pos_full",
                        "sorted_bool_masked_pos_tensor", "sorted_neighborhood"], REF_MODEL)
    mae_fwd = _find(_find(tree.body, ast.ClassDef, "Point_MAE_Mamba").body, ast.FunctionDef, "forward")
    dec_stmts = _stmts_between(mae_fwd, 3139, 3202)
    assert "x_vis.shape" in ast.unparse(dec_stmts[0]) and "gt_points" in ast.unparse(dec_stmts[-1]) \
        and "cnt = 4" in ast.unparse(dec_stmts), "reference layout changed: restore loop not at :3139-3202"
    decoder = _make_fn(scope, "_ref_mae_decoder", dec_stmts,
                       ["self", "x_vis", "mask_ratio", "neighborhood_org", "noaug", "sorted_pos_mask",
                        "sorted_bool_masked_pos_list", "center", "sorted_bool_masked_pos_tensor", "sorted_pos_full",
                        "sorted_neighborhood"],
                       ["x_full_tensor", "sorted_bool_masked_pos_tensor_final", "gt_points", "x_rec"], REF_MODEL)
    inp = mae_inputs()
    me = SimpleNamespace(mask_ratio=D["mask_ratio"], training=False, blocks=lambda x, pos: x, norm=lambda x: x)
    np.random.seed(5)
    _random.seed(6)
    with CudaToCpu():
        mask_rand = scope["_mask_center_rand"](me, inp["geometry"])
        mask_block = scope["_mask_center_block"](me, inp["geometry"])
    rec = {"orders": inp["orders"].numpy(), "geometry": inp["geometry"].numpy(), "mask_rand": mask_rand.numpy(),
           "mask_block": mask_block.numpy(), "np_seed": np.array(5), "random_seed": np.array(6),
           "dims": np.array([B, G, k, D["M"], D["C"]]), "mask_ratio": np.array(D["mask_ratio"])}
    _random.seed(6)
    rec["block_seed_index"] = np.array([_random.randint(0, G - 1) for _ in range(B)])     # the draws :2217 made
    P = torch.nn.functional.one_hot(inp["orders"], G).float()
    for name, mask in (("rand", mask_rand), ("block", mask_block)):
        with CudaToCpu():
            x_vis, mlist, pos_mask, pos_full, mtensor, nbh = encoder(
                me, P, None, mask, inp["tokens"], inp["pos"], inp["neighborhood"], inp["center"], B, D["C"], True)
            dec_self = SimpleNamespace(mask_token=torch.full((1, 1, D["C"]), -1.0), MAE_decoder=lambda x, pos, n: x,
                                       increase_dim=lambda t: t)
            x_full, final, gt, x_rec = decoder(dec_self, x_vis, D["mask_ratio"], inp["neighborhood"], False, pos_mask,
                                               mlist, inp["center"], mtensor, pos_full, nbh)
        assert bool((x_rec == -1).all())                      # the decoder's selection takes mask tokens only
        rec[f"{name}.x_vis_index"] = x_vis[:, :, 0].long().numpy()            # 1 + patch id per visible slot
        rec[f"{name}.pos_mask_index"] = pos_mask[:, :, 0].long().numpy()      # 1001 + patch id per masked slot
        rec[f"{name}.pos_full_index"] = pos_full[:, :, 0].long().numpy()
        rec[f"{name}.sorted_mask"] = torch.stack(mlist, 1).numpy()            # (B, k, G)
        rec[f"{name}.sorted_mask_flipped"] = mtensor.numpy()                  # (B, k G)
        rec[f"{name}.neighborhood_index"] = nbh[:, :, 0, 0].long().numpy()    # 2001 + patch id per slot
        rec[f"{name}.x_full_index"] = x_full[:, :, 0].long().numpy()          # -1 at mask tokens, else 1 + patch id
        rec[f"{name}.final_mask"] = final.numpy()                             # (B, 2 k G)
        rec[f"{name}.gt_index"] = gt[:, 0, 0].long().numpy()                  # 2001 + patch id per rebuilt patch
    np.savez_compressed(os.path.join(OUT, "ref_mae_flow.npz"), **rec)
    return rec


def generate():
    """Every fixture into OUT; -> printed summary lines."""
    torch.set_num_threads(4)
    methods, sast, hlt_fn, scope = load_reference()
    for name in ("spectral_g64", "spectral_g128", "spectral_g128_surface"):
        rec = spectral_fixture(name, methods, sast, hlt_fn)
        print(f"ref_{name}.npz: {len(rec)} arrays")
    rec = stack_fixture(scope)
    print(f"ref_stack.npz: {len(rec)} arrays")
    rec = create_block_fixture()
    print(f"ref_create_block.json: {len(rec['state_dict'])} parameters")
    fp_mod = _import_file("_ref_pointnet2_utils", REF_FP)
    for name, make in (("ref_seg_interp", lambda: interp_fixture(fp_mod)), ("ref_seg_fp", lambda: fp_fixture(fp_mod)),
                       ("ref_seg_head", lambda: head_fixture(fp_mod)), ("ref_encoder", encoder_fixture),
                       ("ref_mae_flow", mae_fixture), ("ref_transforms", transforms_fixture),
                       ("ref_part_metrics", part_metrics_fixture)):
        rec = make()
        print(f"{name}.npz: {len(rec)} arrays")


def check():
    """Regenerate into a temporary directory and report every array that differs from the committed one."""
    import json
    import tempfile
    global OUT
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        OUT = tmp
        try:
            generate()
        finally:
            OUT = GOLDEN
        for fname in sorted(os.listdir(tmp)):
            old = os.path.join(GOLDEN, fname)
            if not os.path.exists(old):
                print(f"CHECK {fname}: not committed")
                bad += 1
                continue
            if fname.endswith(".json"):
                with open(old) as a, open(os.path.join(tmp, fname)) as b:
                    diff = [] if json.load(a) == json.load(b) else ["<contents>"]
            else:
                a, b = np.load(old), np.load(os.path.join(tmp, fname))
                diff = sorted(set(a.files) ^ set(b.files))
                diff += [k for k in a.files if k in b.files and not (
                    a[k].shape == b[k].shape and a[k].dtype == b[k].dtype
                    and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"))]
            print(f"CHECK {fname}: " + ("identical" if not diff else "DIFFERS in " + ", ".join(diff)))
            bad += bool(diff)
    print("CHECK: every regenerated fixture equals the committed one" if not bad else f"CHECK: {bad} file(s) differ")
    return 1 if bad else 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not reference_present():
        print("reference not present: keeping the committed ref_* fixtures", file=sys.stderr)
        return 1
    if "--check" in argv:
        return check()
    from oracle.gen_golden import record_cpu_platform
    record_cpu_platform()
    generate()
    return 0


if __name__ == "__main__":
    sys.exit(main())
