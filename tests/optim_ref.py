"""float64 restatement of the optimizer tail (si_mamba_amd/optim/, csrc/optim.hip): clip_grad_norm_'s coefficient and
torch.optim.AdamW's decoupled update, and the shared case of the parity tests.  A helper module: pytest collects nothing
from it.

TEST INFRASTRUCTURE.  ``ref_run`` is the reference the device results are held to; ``torch_tail`` is torch's own tail on
the CPU (``clip_grad_norm_`` + ``torch.optim.AdamW``) in a dtype of choice: in float64 it pins the restatement
(test_optim_abi.py), in float32 against float64 it gives the reference's own rounding error the bounds are built from.
"""
import math

import torch

from helpers import max_scaled, pinned_bound

STEP_SCALES = (1.0, 0.01, 3.0, 1e-4, 0.5)     # the gradients of step k are N(0, 1) * STEP_SCALES[k]
CLIP = 10.0
LR, BETAS, EPS = 0.05, (0.9, 0.999), 1e-8
WEIGHT_DECAYS = (0.0, 0.05)                   # group 0, group 1
HALF_ZERO, TINY = 3, 9                        # tensor 3: every second gradient zero; tensor 9: gradients of order 1e-9


def case_shapes(chunk):
    C = int(chunk)
    return [(1,), (3,), (5,), (127,), (C - 1,), (C,), (C + 1,), (2 * C + 7,), (96, 40), (384,)]


class Case:
    """Parameters 0.02 * N(0, 1) of ``case_shapes(chunk)``, alternately in group 0 (no decay) and group 1 (decay 0.05),
    and five steps of gradients.  Everything fp32 on the CPU, drawn once; nothing here is modified by a run."""

    def __init__(self, chunk, seed=20240, shapes=None):
        gen = torch.Generator().manual_seed(seed)
        self.shapes = case_shapes(chunk) if shapes is None else list(shapes)
        self.params = [0.02 * torch.randn(s, generator=gen) for s in self.shapes]
        self.group_of = [i % 2 for i in range(len(self.shapes))]
        self.grads = []
        for scale in STEP_SCALES:
            gs = [scale * torch.randn(s, generator=gen) for s in self.shapes]
            gs[HALF_ZERO][1::2] = 0.0
            gs[TINY] = gs[TINY] * 1e-9
            self.grads.append(gs)

    def groups(self, params, lr=LR):
        """param_groups over ``params`` (this case's tensors in order) for any AdamW."""
        return [dict(params=[p for p, g in zip(params, self.group_of) if g == k], lr=lr, betas=BETAS, eps=EPS,
                     weight_decay=WEIGHT_DECAYS[k]) for k in range(2)]


def clip_coef(norm, clip):
    """min(1, clip / (norm + 1e-6)) as torch.clamp takes it: a NaN stays a NaN."""
    if clip is None:
        return 1.0
    c = clip / (norm + 1e-6)
    return c if (c <= 1.0 or math.isnan(c)) else 1.0


def ref_step(P, M, V, T, grads, group_of, lrs, clip=None, grad_scale=1.0, betas=BETAS, eps=EPS, wds=WEIGHT_DECAYS):
    """One update in place on float64 lists; ``grads[i] is None``: tensor i took no gradient.  ``lrs``: one rate per
    group.  Returns the norm before clipping."""
    gs = [None if g is None else grad_scale * g.double() for g in grads]
    total = sum(float(g.square().sum()) for g in gs if g is not None)
    norm = math.sqrt(total) if not math.isnan(total) else float("nan")
    coef = clip_coef(norm, clip)
    b1, b2 = betas
    for i, g in enumerate(gs):
        if g is None:
            continue
        g = g * coef
        lr, wd = lrs[group_of[i]], wds[group_of[i]]
        T[i] += 1
        P[i].mul_(1.0 - lr * wd)
        M[i].mul_(b1).add_(g, alpha=1.0 - b1)
        V[i].mul_(b2).add_(g * g, alpha=1.0 - b2)
        bc1, bc2 = 1.0 - b1 ** T[i], 1.0 - b2 ** T[i]
        P[i].sub_((lr / bc1) * (M[i] / (V[i].sqrt() / math.sqrt(bc2) + eps)))
    return norm


def ref_run(case, steps=5, clip=CLIP, lrs=None, grad_scale=1.0, start=None):
    """-> dict(p, m, v: lists of float64 tensors, norms: list, t: list).  ``lrs``: per step, one rate per group (default
    LR throughout); ``start``: (P, M, V, T) to continue from."""
    if start is None:
        P = [p.double().clone() for p in case.params]
        M = [torch.zeros_like(p) for p in P]
        V = [torch.zeros_like(p) for p in P]
        T = [0] * len(P)
    else:
        P, M, V = ([t.double().clone() for t in ts] for ts in start[:3])
        T = list(start[3])
    norms = []
    for k in range(steps):
        rate = (LR, LR) if lrs is None else lrs[k]
        norms.append(ref_step(P, M, V, T, case.grads[k], case.group_of, rate, clip, grad_scale))
    return dict(p=P, m=M, v=V, norms=norms, t=T)


def torch_tail(case, dtype, steps=5, clip=CLIP, grads=None):
    """torch's tail on the CPU in ``dtype``: clip_grad_norm_(foreach=False) + torch.optim.AdamW.  Same dict as ref_run
    (tensors in ``dtype``).  ``grads``: per step lists in place of the case's."""
    params = [torch.nn.Parameter(p.to(dtype).clone()) for p in case.params]
    opt = torch.optim.AdamW(case.groups(params), foreach=False)
    norms = []
    for k in range(steps):
        for p, g in zip(params, (case.grads if grads is None else grads)[k]):
            p.grad = g.to(dtype).clone()
        if clip is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, clip, foreach=False)))
        opt.step()
    return dict(p=[p.detach() for p in params], m=[opt.state[p]["exp_avg"] for p in params],
                v=[opt.state[p]["exp_avg_sq"] for p in params], norms=norms,
                t=[int(opt.state[p]["step"]) for p in params])


def worst(got, want):
    """The largest max_scaled over the tensors of two lists."""
    return max(max_scaled(a, b) for a, b in zip(got, want))


def norm_err(got, want):
    return max(abs(float(a) - float(b)) / abs(float(b)) for a, b in zip(got, want))


def bounds(case, steps=5, cap=1e-5):
    """pinned_bound per quantity from torch's own fp32 tail against its float64 tail on the CPU."""
    r32, r64 = torch_tail(case, torch.float32, steps), torch_tail(case, torch.float64, steps)
    err = dict(p=worst(r32["p"], r64["p"]), m=worst(r32["m"], r64["m"]), v=worst(r32["v"], r64["v"]),
               norm=norm_err(r32["norms"], r64["norms"]))
    return {k: pinned_bound(e, cap) for k, e in err.items()}, err
