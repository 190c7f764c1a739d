"""GPU: MixerModel with every mixer on the samples the next block's DropPath keeps (block.py: draw_drop_plan,
_compact_stack; compact add + norm kernels) against the same stack on the whole batch, which is the reference's route.

The two routes do the same arithmetic per kept sample and multiply nothing by the dropped ones' zeros, so they are held
to the bounds tests/test_gpu_model.py::test_first_block_on_distinct_tokens_equals_reference_route uses for two routes of
the same arithmetic: outputs nerr < 1e-5, input and parameter gradients nerr < 1e-4 (fp32).
"""
import copy

import pytest
import torch

from helpers import nerr
from si_mamba_amd import _lib
from si_mamba_amd.block import MixerModel

pytestmark = pytest.mark.gpu

B, G, K, D, NL = 6, 64, 4, 128, 4
KEEP = 0.9


def _mask(dropped):
    m = torch.full((B,), 1.0 / KEEP)
    m[list(dropped)] = 0.0
    return m


# masks of blocks 1 .. 3 and the compact batch each boundary must come to (bucket 4, B = 6): nothing dropped -> 6; one
# dropped -> 5 kept, rounded up to 8, capped at B = 6; three dropped -> 3 kept -> 4 (one dropped sample rides along);
# everything dropped -> 0, the mixer is not called
MASK_SETS = {
    "none_one_three": ([_mask(()), _mask((2,)), _mask((0, 3, 5))], [6, 6, 4]),
    "three_all_none": ([_mask((1, 2, 4)), _mask(range(B)), _mask(())], [4, 0, 6]),
}


def _inputs(device):
    g = torch.Generator().manual_seed(1)
    tokens, pos = torch.randn(B, G, D, generator=g).to(device), torch.randn(B, G, D, generator=g).to(device)
    order = torch.stack([torch.stack([torch.randperm(G, generator=g) for _ in range(K)]) for _ in range(B)]).to(device)
    idx = torch.cat((order.flatten(1), order.flatten(1).flip(1)), 1)                      # (B, 2 K G) = (6, 512)
    w = torch.randn(B, idx.shape[1], D, generator=g).to(device)
    return tokens, pos, idx, w


@pytest.fixture(scope="module")
def model(device):
    torch.manual_seed(0)
    return MixerModel(d_model=D, n_layer=NL).to(device).train()


class _MixerCalls:
    """Batch size of every mixer body that runs (mamba_simple.mamba_inner_fn), forward order."""

    def __enter__(self):
        from si_mamba_amd import mamba_simple
        self.mod, self.real, self.sizes = mamba_simple, mamba_simple.mamba_inner_fn, []
        mamba_simple.mamba_inner_fn = lambda xz, *a, **k: (self.sizes.append(xz.shape[0]), self.real(xz, *a, **k))[1]
        return self

    def __exit__(self, *exc):
        self.mod.mamba_inner_fn = self.real
        return False


def _run(m, route, tokens, pos, idx, w, masks, amp=False):
    t, p = tokens.clone().requires_grad_(True), pos.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        if route == "tokens":
            out = m(t, p, token_index=idx, balanced_index=True, drop_masks=masks)
        else:
            ex = idx.unsqueeze(-1).expand(-1, -1, D)
            out = m(torch.gather(t, 1, ex), torch.gather(p, 1, ex), drop_masks=masks)
    (out.float() * w).sum().backward()
    return out, t.grad, p.grad


@pytest.mark.parametrize("masks_id", sorted(MASK_SETS))
@pytest.mark.parametrize("route", ["tokens", "plain"])
def test_compact_stack_equals_the_full_stack(model, route, masks_id, device):
    masks, sizes = MASK_SETS[masks_id]
    masks = [m.to(device) for m in masks]
    tokens, pos, idx, w = _inputs(device)
    a, b = copy.deepcopy(model), copy.deepcopy(model)
    c0 = _lib.counters.get("drop_path_compact", 0)
    s0 = dict(_lib.compact_sizes)
    with _MixerCalls() as calls:
        oa, ta, pa = _run(a, route, tokens, pos, idx, w, masks)
    assert _lib.counters.get("drop_path_compact", 0) == c0 + 1, "the compact route was not taken"
    want_calls = [s for s in sizes if s] + [B]              # mixers 0 .. 2 at their boundary's size, the last at B
    assert calls.sizes == want_calls
    for s in set(want_calls):
        assert _lib.compact_sizes.get(s, 0) - s0.get(s, 0) == want_calls.count(s)
    with _lib.drop_path_compact(False), _MixerCalls() as calls:
        ob, tb, pb = _run(b, route, tokens, pos, idx, w, masks)
    assert _lib.counters.get("drop_path_compact", 0) == c0 + 1, "switched off, the full route runs"
    assert calls.sizes == [B] * NL
    e_out, e_t, e_p = nerr(oa, ob), nerr(ta, tb), nerr(pa, pb)
    print(f"{route} {masks_id}: out {e_out:.2e} dtokens {e_t:.2e} dpos {e_p:.2e}")
    assert e_out < 1e-5
    assert e_t < 1e-4 and e_p < 1e-4
    for (ka, qa), (_, qb) in zip(a.named_parameters(), b.named_parameters()):
        # a mixer that ran on no sample gets the full route's exact zeros, not None
        assert (qa.grad is None) == (qb.grad is None), ka
        if qb.grad is None:
            continue
        e = nerr(qa.grad, qb.grad)
        assert e < 1e-4, (ka, e)


@pytest.mark.parametrize("lead", [False, True])
def test_early_draw_keeps_the_generator_order(model, lead, device):
    """After the same seed, draw_drop_plan's factors are those of the blocks' own successive DropPath.rowscale calls
    (``lead``: block 0 draws first and its draw is not used)."""
    x = torch.empty(B, G, D, device=device)
    torch.manual_seed(7)
    plan = model.draw_drop_plan(x, lead=lead)
    assert plan is not None and len(plan.masks) == NL - 1
    plan.event.synchronize()                                 # the draw runs on the plan's own stream
    after_plan = torch.rand(3, device=device)
    torch.manual_seed(7)
    want = [model.layers[i].drop_path.rowscale(x) for i in range(0 if lead else 1, NL)][-(NL - 1):]
    after_blocks = torch.rand(3, device=device)
    for g, w_ in zip(plan.masks, want):
        assert torch.equal(g, w_)
    assert torch.equal(after_plan, after_blocks)            # and the generator stands where it stood
    torch.cuda.synchronize()


def _two_steps(m, route, tokens, pos, idx):
    """Two training forwards in a row with the stack's own draws -> (outputs, a draw made right after them)."""
    outs = []
    with torch.no_grad():
        for _ in range(2):
            if route == "tokens":
                outs.append(m(tokens, pos, token_index=idx, balanced_index=True))
            else:
                ex = idx.unsqueeze(-1).expand(-1, -1, D)
                outs.append(m(torch.gather(tokens, 1, ex), torch.gather(pos, 1, ex)))
        return outs, torch.rand(5, device=tokens.device)


@pytest.mark.parametrize("route", ["plain", "tokens"])
def test_whole_forward_draws_what_the_full_route_draws(route, device):
    """No injected masks: after the same seed, a compact forward and a switched-off forward make the same number of
    draws (a torch.rand behind them gives the same numbers) and use the same masks (the outputs agree, in the first
    step and in the one after it).  On the plain route block 0 goes through Block.forward, which draws a rowscale it
    never applies: with a plan that draw is the plan's lead draw and block 0 must not draw again, whether boundary 1 is
    compact (sizes[0] < B) or not (sizes[0] == B).  drop_path = 0.3 at B = 6 makes both cases frequent; the seeds are
    walked until both have been seen."""
    torch.manual_seed(0)
    m = MixerModel(d_model=D, n_layer=NL, drop_path=0.3).to(device).train()
    tokens, pos, idx, _ = _inputs(device)
    seen = set()
    real = MixerModel._finish_plan

    def spy(self, plan, dev):
        real(self, plan, dev)
        first.append(plan.sizes[0])
        return plan
    MixerModel._finish_plan = spy
    try:
        for seed in range(12):
            first = []
            torch.manual_seed(100 + seed)
            oa, ra = _two_steps(m, route, tokens, pos, idx)
            assert len(first) == 2, "the compact route was not taken"
            torch.manual_seed(100 + seed)
            with _lib.drop_path_compact(False):
                ob, rb = _two_steps(m, route, tokens, pos, idx)
            assert len(first) == 2
            assert torch.equal(ra, rb), (seed, first)
            for x, y in zip(oa, ob):
                assert nerr(x, y) < 1e-5, (seed, first)
            seen.add(first[0] == B)
            if seen == {True, False} and seed >= 3:
                break
    finally:
        MixerModel._finish_plan = real
    assert seen == {True, False}, "both cases of boundary 1 (compact and whole batch) have to occur"


def test_two_plans_in_flight_do_not_share_staging(model, device):
    """A second plan drawn before the first is finished (two stacks of one shape, or a plan that is dropped) must not
    overwrite the factors the first is planned from."""
    a, b = copy.deepcopy(model), copy.deepcopy(model)
    x = torch.empty(B, G, D, device=device)
    m1 = [_mask((0, 3, 5)), _mask(()), _mask((1,))]
    m2 = [_mask(()), _mask(range(B)), _mask((0, 1, 2))]
    p1 = a.draw_drop_plan(x, drop_masks=[t.to(device) for t in m1])
    p2 = b.draw_drop_plan(x, drop_masks=[t.to(device) for t in m2])
    a._finish_plan(p1, x.device)
    b._finish_plan(p2, x.device)
    assert p1.sizes == [4, 6, 6] and p2.sizes == [6, 0, 4]
    assert p1.maps[0].tolist() == [3, 0, 1, -1, 2, -1]      # kept 1, 2, 4 first, then one dropped sample (0)
    torch.cuda.synchronize()


def test_full_route_in_eval_under_capture_and_switched_off(model, device):
    tokens, pos, idx, _ = _inputs(device)
    m = copy.deepcopy(model)

    def fwd():
        return m(tokens, pos, token_index=idx, balanced_index=True)
    c0 = _lib.counters.get("drop_path_compact", 0)
    with torch.no_grad():
        with _lib.drop_path_compact(False):
            fwd()
        m.eval()
        fwd()
        m.train()
        assert _lib.counters.get("drop_path_compact", 0) == c0
        # stream capture: the plan needs the factors on the host, so the captured forward is the full one
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side), _lib.drop_path_compact(False):
            fwd()                                            # warm-up of the route the capture takes
        torch.cuda.current_stream(device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fwd()
        graph.replay()
        torch.cuda.synchronize()
        assert _lib.counters.get("drop_path_compact", 0) == c0
        assert bool(torch.isfinite(out).all())
        fwd()
        assert _lib.counters.get("drop_path_compact", 0) == c0 + 1     # and eager, in training, it is on by default


def test_bf16_layer_by_layer(model, device):
    """bf16 autocast with the fused out_proj + add + LayerNorm chain off: the layer-by-layer route, compact against
    full, at the project's bf16 bound."""
    masks, sizes = MASK_SETS["three_all_none"]
    masks = [m.to(device) for m in masks]
    tokens, pos, idx, w = _inputs(device)
    a, b = copy.deepcopy(model), copy.deepcopy(model)
    c0 = _lib.counters.get("drop_path_compact", 0)
    with _lib.fuse_out_norm(False):
        oa, ta, pa = _run(a, "tokens", tokens, pos, idx, w, masks, amp=True)
        assert _lib.counters.get("drop_path_compact", 0) == c0 + 1
        with _lib.drop_path_compact(False):
            ob, tb, pb = _run(b, "tokens", tokens, pos, idx, w, masks, amp=True)
    e = [nerr(oa.float(), ob.float()), nerr(ta, tb), nerr(pa, pb)]
    print(f"bf16: out {e[0]:.2e} dtokens {e[1]:.2e} dpos {e[2]:.2e}")
    assert max(e) < 1e-2
    for (ka, qa), (_, qb) in zip(a.named_parameters(), b.named_parameters()):
        assert (qa.grad is None) == (qb.grad is None), ka
        if qb.grad is not None:
            assert nerr(qa.grad, qb.grad) < 1e-2, ka


# ---- the classifier: its early route decision and draw against what the stack then does ------------------------------
# (config overrides, does the stack take the compact route).  SAST / MAMBA at 16 patches: block 0 on the distinct tokens,
# a plan without a lead draw, drawn ahead of the tokeniser; 18 patches (G % 4 != 0): the gathered route, a lead draw;
# input dropout, HLT, add_after_layer: nothing is drawn early -- the plain stack draws on entry, the merging stack of
# add_after_layer has no compact route.
POINT_MAMBA_CASES = {
    "sast": (dict(method="SAST"), True),
    "mamba": (dict(method="MAMBA"), True),
    "sast_18_patches": (dict(method="SAST", num_group=18), True),
    "input_dropout": (dict(method="SAST", drop_out=0.1), True),
    "hlt": (dict(method="HLT"), True),
    "add_after_layer": (dict(method="SAST", add_after_layer=True), False),
}


def _point_mamba(device, **over):
    from si_mamba_amd.point_mamba import PointMamba, default_config
    from si_mamba_amd.synthetic import make_clouds
    cfg = dict(trans_dim=128, encoder_dims=128, depth=3, group_size=8, num_group=16, knn_graph=4, drop_path=0.3,
               cls_dim=5)
    cfg.update(over)
    torch.manual_seed(0)
    return PointMamba(default_config(**cfg)).to(device).train(), make_clouds(B, 128, seed=0, device=device)


@pytest.mark.parametrize("case", sorted(POINT_MAMBA_CASES))
def test_point_mamba_early_draw_agrees_with_the_stack(case, device):
    """PointMamba decides the stack's route and draws the plan before its tokeniser; the stack must then take exactly
    that route (no ValueError from its guard), make the full route's draws and give the full route's logits."""
    over, compact = POINT_MAMBA_CASES[case]
    m, pts = _point_mamba(device, **over)
    c0 = _lib.counters.get("drop_path_compact", 0)
    s0 = dict(_lib.compact_sizes)
    for n, seed in enumerate((11, 12, 13), 1):
        with torch.no_grad():
            torch.manual_seed(seed)
            a = m(pts)
            ra = torch.rand(5, device=device)
            assert _lib.counters.get("drop_path_compact", 0) == c0 + n * int(compact)
            torch.manual_seed(seed)
            with _lib.drop_path_compact(False):
                b = m(pts)
            rb = torch.rand(5, device=device)
        assert _lib.counters.get("drop_path_compact", 0) == c0 + n * int(compact)
        e = nerr(a, b)
        print(f"{case} seed {seed}: logits {e:.2e}")
        assert e < 1e-5
        assert torch.equal(ra, rb)
    sizes = {k: v - s0.get(k, 0) for k, v in _lib.compact_sizes.items() if v != s0.get(k, 0)}
    print(f"{case}: mixer batches {sizes}")
    # drop_path = 0.3 at B = 6: over three seeds some boundary keeps at most four samples (a compact batch of 4)
    assert any(k < B for k in sizes) == compact


def test_route_predicates_run_once_per_forward(device, monkeypatch):
    m, pts = _point_mamba(device, method="SAST")
    calls = {}
    for name in ("_compact_ok", "_chain_ok", "_first_block_applies"):
        def spy(self, *a, _real=getattr(MixerModel, name), _name=name, **k):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(self, *a, **k)
        monkeypatch.setattr(MixerModel, name, spy)
    c0 = _lib.counters.get("drop_path_compact", 0)
    with torch.no_grad():
        m(pts)
    assert _lib.counters.get("drop_path_compact", 0) == c0 + 1
    print(calls)
    assert calls and all(n <= 1 for n in calls.values()), calls
