"""What the CPU and the GPU tests of the reference-pinned head fixtures share (tests/test_oracle_pinned_heads.py,
tests/test_gpu_pinned.py): the bounds, the lowest-copy rule of a repeated centre, the multiset comparison of chosen
centres and the list of quantities ref_encoder.npz records.

TEST INFRASTRUCTURE.  Every float assertion is ``metric(got, float64 fixture) <= helpers.pinned_bound(ref32_err, cap)``
with ``ref32_err`` read from the fixture and ``cap`` what the op's older test file allows."""
import numpy as np
import torch

from helpers import nerr, pinned_bound

INTERP_CAP, HEAD_CAP = 2e-4, 1e-3           # peak_err in tests/test_gpu_seg.py; nerr for the encoder and the head
BF16_INTERP, BF16_HEAD = 2e-2, 1e-2         # the project's bf16 figures, against the float64 fixture


def tensor(a, device=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if device is None else t.to(device)


def lowest_copies(xyz2, ref_idx):
    """(B, N, 3) the three lowest slots that hold the coordinates of the reference's nearest centre (a sequence in which
    every centre stands at least three times): the documented tie rule of oracle/seg_ref.py and csrc/interp.hip."""
    B, N, _ = ref_idx.shape
    S = xyz2.shape[1]
    out = torch.empty(B, N, 3, dtype=torch.int64)
    for b in range(B):
        near = xyz2[b, ref_idx[b, :, 0]]                                      # (N, 3)
        same = (xyz2[b][None, :, :] == near[:, None, :]).all(-1)              # (N, S)
        slots = torch.where(same, torch.arange(S)[None, :], S)
        out[b] = slots.sort(-1)[0][:, :3]
    return out


def same_multiset(a, b):
    """a, b (..., 3, 3): three chosen centres each.  True per query where both hold the same coordinates the same number
    of times, whatever the order and whichever copy of a repeated centre was taken."""
    eq = lambda p, q: (p.unsqueeze(-2) == q.unsqueeze(-3)).all(-1).sum(-1)     # noqa: E731  count of p_k in q
    return ((eq(a, a) == eq(a, b)) & (eq(b, b) == eq(b, a))).all(-1)


def gather_interp(feats, idx, w):
    """sum_k w[b,n,k] feats[b, idx[b,n,k]] in float64."""
    B = feats.shape[0]
    f = feats.double()
    rows = torch.stack([f[b][idx[b].long()] for b in range(B)])                # (B, N, 3, C)
    return (rows * w.double().unsqueeze(-1)).sum(2)


def scatter_interp(dout, idx, w, S):
    """The gradient of gather_interp with respect to feats, in float64: (B, S, C)."""
    B, N, C = dout.shape
    out = torch.zeros(B, S, C, dtype=torch.float64)
    for b in range(B):
        for k in range(3):
            out[b].index_add_(0, idx[b, :, k].long(), dout[b].double() * w[b, :, k].double().unsqueeze(-1))
    return out


def sample_stride(numel, cap=256):
    """The fixed stride of a parameter-gradient sample of at most ``cap`` elements: flat[::stride] (the recipe's rule)."""
    return max(1, -(-numel // cap))


def encoder_results(enc, pts, dout, dup):
    """What ref_encoder.npz records, from a forward + backward of ``enc``: name -> tensor.  The point gradients are summed
    over the rows of the duplicated point: which duplicate receives the max's gradient is not specified."""
    x = pts.clone().requires_grad_(True)
    out = enc(x)
    out.backward(dout)
    gp = x.grad.clone()
    b, p, r0, r1 = (int(v) for v in dup)
    gp[b, p, r0] += gp[b, p, r1]
    gp[b, p, r1] = 0
    res = {"out": out.detach(), "grad.points_dupsum": gp}
    for k, prm in enc.named_parameters():
        res["gnorm." + k] = prm.grad.norm().reshape(1)
        res["gsample." + k] = prm.grad.flatten()[::sample_stride(prm.numel())]
    res.update({"stat." + k: buf for k, buf in enc.named_buffers() if "running" in k})
    return res


def assert_recorded(g, prefix, res, cap=HEAD_CAP, report=None):
    """Every ``<prefix>.<name>64`` of the fixture ``g`` against ``res[name]``: nerr <= pinned_bound(ref32_err.<name>).
    Prints each figure (pytest -s shows them) before asserting on all of them together."""
    keys = [k[len(prefix) + 1:-2] for k in g if k.startswith(prefix + ".") and k.endswith("64") and ".ref32_err." not in k]
    assert sorted(keys) == sorted(res), (sorted(keys), sorted(res))
    bad = []
    for k in keys:
        err, bound = nerr(res[k], tensor(g[f"{prefix}.{k}64"])), pinned_bound(g[f"{prefix}.ref32_err.{k}"], cap)
        print(f"PINNED {report or prefix} {k}: err {err:.3e} ref32_err {float(g[f'{prefix}.ref32_err.{k}']):.3e} "
              f"bound {bound:.3e}")
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


def mae_coded(g):
    """The index-coded inputs ref_mae_flow.npz was run on (oracle/pin_from_reference.py mae_inputs): tokens 1 + g,
    pos 1001 + g, neighbourhoods 2001 + g, centres 3001 + g over (B, G)."""
    B, G, k, M, C = (int(v) for v in g["dims"])
    code = lambda base, *tail: (base + torch.arange(G, dtype=torch.float32)).view(1, G, *[1] * len(tail)).expand(
        B, G, *tail).contiguous()                                                      # noqa: E731
    return dict(tokens=code(1.0, C), pos=code(1001.0, C), neighborhood=code(2001.0, M, 3), center=code(3001.0, 3))
