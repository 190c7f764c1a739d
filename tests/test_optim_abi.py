"""CPU: the optimizer entry points (csrc/optim.hip) validate their arguments before touching a device -- flags, shapes,
null pointers, the workspace, alignment, in that order -- and the host side of si_mamba_amd/optim/: the reference's
schedule and parameter groups, the refusals, the state dict's layout against torch.optim.AdamW's, and the float64
restatement of tests/optim_ref.py against torch's own float64 tail."""
import ctypes
import math

import pytest
import torch

import optim_ref
from abi_tables import (E_ALIGN, E_NULLPTR, E_SHAPE, E_VARIANT, E_WORKSPACE, OFF, P, check_rows, declared_params,
                        header_code)
from si_mamba_amd import _lib, optim

NAN, INF = float("nan"), float("inf")
WS = 16 + 16 * 2 + 16 * 10            # the workspace of 10 segments and 4 chunks



def first_chunk(*counts, segments=10):
    """The HOST array of a call: chunk counts per segment (the rest own none) as first-chunk offsets."""
    counts = list(counts) + [0] * (segments - len(counts))
    return (ctypes.c_int * (segments + 1))(0, *[sum(counts[:i + 1]) for i in range(segments)])


GRADS = (ctypes.c_void_p * 65536)()            # HOST: one address per segment, NULL = no gradient; never launched with
BIG = (ctypes.c_int * 65537)(*([0] * 65536), 1 << 20)
STEP = dict(segments=P, chunks=P, groups=P, updates=P, schedule=None, grad_norm=P, grads=GRADS,
            first_chunk=first_chunk(1, 1, 2), workspace=P, workspace_bytes=WS,
            n_segments=10, n_chunks=4, n_groups=2, schedule_n=0, steps_per_epoch=1, max_norm=10.0, grad_scale=1.0,
            flags=0, stream=None)
STEP_ROWS = [
    (dict(flags=2), E_VARIANT), (dict(flags=-1), E_VARIANT),
    (dict(n_segments=0), E_SHAPE), (dict(n_segments=-3), E_SHAPE), (dict(n_segments=65537), E_SHAPE),
    (dict(n_chunks=0), E_SHAPE), (dict(n_chunks=(1 << 20) + 1), E_SHAPE),
    (dict(n_groups=0), E_SHAPE), (dict(n_groups=257), E_SHAPE),
    (dict(schedule_n=-1), E_SHAPE), (dict(schedule_n=(1 << 20) + 1, schedule=P), E_SHAPE),
    (dict(schedule_n=3, schedule=P, steps_per_epoch=0), E_SHAPE),
    (dict(max_norm=NAN), E_SHAPE), (dict(grad_scale=NAN), E_SHAPE), (dict(grad_scale=INF), E_SHAPE),
    (dict(first_chunk=first_chunk(1, 1, 1)), E_SHAPE), (dict(first_chunk=first_chunk(2, 1, 2)), E_SHAPE),
    (dict(first_chunk=(ctypes.c_int * 11)(1, 1, 2, 4, 4, 4, 4, 4, 4, 4, 4)), E_SHAPE),
    (dict(first_chunk=(ctypes.c_int * 11)(0, 3, 2, 4, 4, 4, 4, 4, 4, 4, 4)), E_SHAPE),
    *[({k: None}, E_NULLPTR) for k in ("segments", "chunks", "groups", "updates", "grad_norm", "grads", "first_chunk")],
    (dict(schedule_n=3), E_NULLPTR),                                  # a schedule length without a table
    (dict(workspace=None), E_WORKSPACE), (dict(workspace_bytes=WS - 1), E_WORKSPACE), (dict(workspace_bytes=0), E_WORKSPACE),
    (dict(workspace=OFF), E_ALIGN), (dict(segments=OFF), E_ALIGN), (dict(groups=OFF), E_ALIGN),
    (dict(chunks=OFF), E_ALIGN), (dict(updates=OFF), E_ALIGN), (dict(schedule_n=3, schedule=OFF), E_ALIGN),
    (dict(grad_norm=P + 2), E_ALIGN),
    # the limits pass the shape checks: the next fault ends the call
    (dict(n_segments=65536, n_chunks=1 << 20, n_groups=256, first_chunk=BIG, updates=None), E_NULLPTR),
    (dict(n_segments=65536, n_chunks=1 << 20, first_chunk=BIG), E_WORKSPACE),
    (dict(max_norm=-1.0, grad_scale=0.125, flags=1, schedule_n=1 << 20, schedule=P, steps_per_epoch=2 ** 31 - 1,
          workspace=None), E_WORKSPACE),
    (dict(max_norm=INF, grad_norm=None), E_NULLPTR),
    # two faults: flags, shape, null pointer, workspace, alignment in that order
    (dict(flags=4, n_segments=0), E_VARIANT), (dict(n_chunks=0, segments=None), E_SHAPE),
    (dict(max_norm=NAN, workspace=None), E_SHAPE), (dict(groups=None, workspace=None), E_NULLPTR),
    (dict(first_chunk=first_chunk(4), grads=None), E_NULLPTR), (dict(first_chunk=first_chunk(3), grads=None), E_SHAPE),
    (dict(chunks=None, workspace=OFF), E_NULLPTR), (dict(workspace_bytes=8, segments=OFF), E_WORKSPACE),
    (dict(workspace=None, updates=OFF), E_WORKSPACE),
]


def test_step_return_codes_without_a_device():
    check_rows("simamba_optim_adamw_step", STEP, STEP_ROWS)


def test_workspace_query():
    lib = _lib.load()
    q = lib.simamba_optim_workspace_bytes
    # [16 bytes of scalars | chunks doubles rounded up to 16 bytes | 16 bytes per segment]; 0 = refused
    assert q(0, 0) == 16 and q(1, 0) == 32 and q(0, 1) == 32 and q(1, 1) == 48 and q(1, 2) == 48 and q(3, 5) == 16 + 48 + 48
    assert q(10, 4) == WS
    assert q(65536, 1 << 20) == 16 + 8 * (1 << 20) + 16 * 65536
    for bad in ((-1, 1), (1, -1), (65537, 1), (1, (1 << 20) + 1)):
        assert q(*bad) == 0
    assert all(q(s, c) % 16 == 0 for s in range(0, 9) for c in range(0, 9))
    checked_call_table = dict(n_segments=1, n_chunks=1)
    check_rows("simamba_optim_workspace_bytes", checked_call_table, [({}, 48), (dict(n_chunks=3), 64)])


def test_abi_is_still_9_and_the_new_prototypes_are_bound():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 9 and lib.simamba_abi_version() == 9
    new = [n for n in declared_params() if n.startswith("simamba_optim_")]
    assert sorted(new) == ["simamba_optim_adamw_step", "simamba_optim_workspace_bytes"]
    for name in new:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == len(declared_params()[name])
    code = header_code()
    assert f"#define SIMAMBA_OPTIM_CHUNK {_lib.OPTIM_CHUNK}" in code
    assert f"#define SIMAMBA_OPTIM_MAX_SEGMENTS {_lib.OPTIM_MAX_SEGMENTS}" in code
    assert f"#define SIMAMBA_OPTIM_MAX_CHUNKS {_lib.OPTIM_MAX_CHUNKS}" in code
    assert f"#define SIMAMBA_OPTIM_MAX_GROUPS {_lib.OPTIM_MAX_GROUPS}" in code
    assert f"#define SIMAMBA_OPTIM_ZERO_GRADS {_lib.OPTIM_ZERO_GRADS}" in code
    assert _lib.OPTIM_CHUNK % 1024 == 0
    import si_mamba_amd
    assert si_mamba_amd.optim is optim and "optim" in si_mamba_amd.__all__


# ---- the schedule ----------------------------------------------------------------------------------------------------
def test_cos_lr_values_literals():
    v = optim.cos_lr_values(3e-4, 300, 10)
    assert len(v) == 301
    want = {0: 1e-6, 5: 1.505e-4, 10: 2.991810233575568e-4, 150: 1.505e-4, 299: 1.0081971798559346e-6, 300: 1e-6}
    for t, w in want.items():
        assert abs(v[t] - w) <= 1e-12 * w, (t, v[t], w)
    # linear warm-up, then monotone down to lr_min
    assert all(abs(v[t] - (1e-6 + t * (3e-4 - 1e-6) / 10)) <= 1e-18 for t in range(10))
    assert all(v[t] > v[t + 1] for t in range(10, 300))
    other = optim.cos_lr_values(1e-3, 20, 0, lr_min=1e-5, warmup_lr_init=1e-7)
    assert other[0] == 1e-5 + 0.5 * (1e-3 - 1e-5) * 2.0 and other[20] == 1e-5
    with pytest.raises(ValueError):
        optim.cos_lr_values(1e-3, 0, 0)


def test_runner_epoch_values_shift():
    v = optim.cos_lr_values(3e-4, 300, 10)
    r = optim.runner_epoch_values(v, 300)
    assert len(r) == 301
    assert r[0] == v[0] and r[1] == v[0] and r[2] == v[1] and r[11] == v[10] and r[300] == v[299]
    assert all(r[e] == v[e - 1] for e in range(1, 301))
    assert optim.runner_epoch_values([3.0, 2.0], 4) == [3.0, 3.0, 2.0, 2.0, 2.0]
    with pytest.raises(ValueError):
        optim.runner_epoch_values([], 3)


# ---- the reference's groups ------------------------------------------------------------------------------------------
class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(4, 3)                                      # fc.weight decays, fc.bias does not
        self.scale = torch.nn.Parameter(torch.ones(5))                       # 1-D, not a bias
        self.cls_token = torch.nn.Parameter(torch.zeros(1, 1, 4))            # 'token' in the name
        self.frozen = torch.nn.Parameter(torch.zeros(2, 2), requires_grad=False)
        self.pos = torch.nn.Linear(3, 4, bias=False)                         # pos.weight: in the skip list
        self.odd = torch.nn.Module()
        self.odd.bias = torch.nn.Parameter(torch.zeros(2, 2))                # 2-D, but the name ends in .bias


def test_reference_param_groups():
    toy = _Toy()
    no_decay, decay = optim.reference_param_groups(toy, 0.05, skip_list=("pos.weight",))
    assert no_decay["weight_decay"] == 0.0 and decay["weight_decay"] == 0.05
    ids = lambda ps: [id(p) for p in ps]
    assert ids(decay["params"]) == ids([toy.fc.weight])
    assert ids(no_decay["params"]) == ids([toy.scale, toy.cls_token, toy.fc.bias, toy.pos.weight, toy.odd.bias])
    assert id(toy.frozen) not in ids(decay["params"]) + ids(no_decay["params"])
    no_decay, decay = optim.reference_param_groups(toy, 0.1)
    assert ids(decay["params"]) == ids([toy.fc.weight, toy.pos.weight]) and decay["weight_decay"] == 0.1


# ---- refusals --------------------------------------------------------------------------------------------------------
def _param(*shape, **kw):
    return torch.nn.Parameter(torch.zeros(*shape, **kw))


def test_refusals_by_name():
    with pytest.raises(ValueError, match="amsgrad"):
        optim.AdamW([_param(3)], amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        optim.AdamW([_param(3)], maximize=True)
    with pytest.raises(ValueError, match="float32"):
        optim.AdamW([_param(3, dtype=torch.float64)])
    with pytest.raises(ValueError, match="float32"):
        optim.AdamW([_param(3, dtype=torch.bfloat16)])
    with pytest.raises(ValueError, match="non-contiguous"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4, 6).t())])
    with pytest.raises(ValueError, match="several devices"):
        optim.AdamW([_param(3), _param(3, device="meta")])
    with pytest.raises(ValueError, match="sparse"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4, 6).to_sparse())])
    with pytest.raises(ValueError, match="betas"):
        optim.AdamW([_param(3)], betas=(1.0, 0.999))
    with pytest.raises(ValueError, match="learning rate"):
        optim.AdamW([_param(3)], lr=-1.0)
    # options a loaded state dict or the user set on a group later
    for key in ("amsgrad", "maximize"):
        opt = optim.AdamW([_param(3)])
        opt.param_groups[0][key] = True
        sd = opt.state_dict()
        with pytest.raises(ValueError, match=key):
            optim.AdamW([_param(3)]).load_state_dict(sd)


def test_step_refuses_cpu_tensors():
    p = _param(5)
    opt = optim.AdamW([p], lr=1e-3)
    p.grad = torch.ones(5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step(clip=10.0, zero_grads=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.prepare()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.set_schedule([1e-3, 1e-4], steps_per_epoch=2)
    assert torch.equal(p.detach(), torch.zeros(5)) and not opt.state
    with pytest.raises(ValueError, match="clip"):
        opt.step(clip=-1.0)
    with pytest.raises(ValueError, match="grad_scale"):
        opt.step(grad_scale=INF)


# ---- state dict ------------------------------------------------------------------------------------------------------
def _pair():
    ours = [_param(4, 3), _param(3), _param(2, 2)]
    theirs = [_param(4, 3), _param(3), _param(2, 2)]
    groups = lambda ps: [dict(params=ps[:2], weight_decay=0.0), dict(params=ps[2:], weight_decay=0.05, lr=2e-3)]
    return (optim.AdamW(groups(ours), lr=1e-3, betas=(0.8, 0.99), eps=1e-7),
            torch.optim.AdamW(groups(theirs), lr=1e-3, betas=(0.8, 0.99), eps=1e-7), ours, theirs)


def test_state_dict_structure_matches_torch_both_ways():
    ours, theirs, po, pt = _pair()
    a, b = ours.state_dict(), theirs.state_dict()
    assert set(a) == set(b) == {"state", "param_groups"}
    for ga, gb in zip(a["param_groups"], b["param_groups"]):
        assert set(ga) == set(gb) | {"updates"} and ga["updates"] == 0
        for k in ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "differentiable", "params"):
            assert ga[k] == gb[k], k
        assert ga["capturable"] is True
    # torch's optimizer, stepped on the CPU -> ours: the state's keys, values and the update count it implies
    for p in pt:
        p.grad = torch.ones_like(p)
    theirs.step()
    theirs.step()
    b = theirs.state_dict()
    ours.load_state_dict(b)
    assert ours.update_count() == 2
    a = ours.state_dict()
    assert sorted(a["state"]) == sorted(b["state"]) == [0, 1, 2]
    for k in a["state"]:
        assert set(a["state"][k]) == set(b["state"][k]) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(a["state"][k]["step"]) == 2.0
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a["state"][k][name], b["state"][k][name])
    assert all(g["updates"] == 2 for g in a["param_groups"])
    # ours -> torch's (a fresh one) -> ours: the options arrive, the update count survives
    fresh = torch.optim.AdamW([dict(params=[_param(4, 3), _param(3)]), dict(params=[_param(2, 2)])])
    fresh.load_state_dict(a)
    for g, want in zip(fresh.param_groups, a["param_groups"]):
        assert g["betas"] == (0.8, 0.99) and g["eps"] == 1e-7 and g["lr"] == want["lr"]
        assert g["weight_decay"] == want["weight_decay"] and g["capturable"] is True
    assert [float(fresh.state[p]["step"]) for g in fresh.param_groups for p in g["params"]] == [2.0, 2.0, 2.0]
    back = optim.AdamW([dict(params=[_param(4, 3), _param(3)]), dict(params=[_param(2, 2)])])
    back.load_state_dict(fresh.state_dict())
    assert back.update_count() == 2 and back.param_groups[1]["lr"] == 2e-3
    assert "updates" not in back.param_groups[0]


# ---- the restatement -------------------------------------------------------------------------------------------------
def test_restatement_equals_torch_in_float64():
    """tests/optim_ref.py against clip_grad_norm_ + torch.optim.AdamW in float64 on the CPU, and the clip's pattern the
    parity tests rely on: active at steps 0, 2 and 4, idle at 1 and 3."""
    case = optim_ref.Case(_lib.OPTIM_CHUNK)
    ref = optim_ref.ref_run(case)
    want = optim_ref.torch_tail(case, torch.float64)
    assert [n > optim_ref.CLIP for n in ref["norms"]] == [True, False, True, False, True]
    assert optim_ref.norm_err(ref["norms"], want["norms"]) < 1e-12
    for k in "pmv":
        assert optim_ref.worst(ref[k], want[k]) < 1e-12, k
    assert ref["t"] == want["t"] == [5] * len(case.params)
    assert float(case.grads[0][optim_ref.TINY].abs().max()) < 1e-8
    assert bool((case.grads[2][optim_ref.HALF_ZERO][1::2] == 0).all())
    assert math.isnan(optim_ref.clip_coef(NAN, 10.0)) and optim_ref.clip_coef(INF, 10.0) == 0.0
    assert optim_ref.clip_coef(5.0, 10.0) == 1.0 and optim_ref.clip_coef(5.0, None) == 1.0
