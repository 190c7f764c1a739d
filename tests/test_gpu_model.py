"""GPU: the PointMamba caller runs on the HIP ops (BASELINE configs 2/3 in reduced and full size)."""
import pytest
import torch

from helpers import clouds, nerr
from oracle import fps_ref, scan_ref, spectral_ref as sr

pytestmark = pytest.mark.gpu


def test_pointmamba_small_forward_matches_oracle_composition(device):
    """Small config: same weights, CPU oracle for ordering + mixers, torch for the rest."""
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    cfg = default_config(trans_dim=64, encoder_dims=64, depth=2, num_group=32, group_size=16, drop_path=0.,
                         knn_graph=8)
    m = PointMamba(cfg).to(device).eval()
    pts = clouds(3, 256, 0)
    with torch.no_grad():
        got = m(pts.to(device)).cpu()
        nb, center, _ = m.group_divider(pts.to(device))
        tokens, pos = m.encoder(nb).cpu(), m.pos_embed(center).cpu()
        center = center.cpu()
    adj = sr.create_graph_from_feature_space(center, 8, cfg.alpha, True, False, True)
    _, vecs, _, _ = sr.calc_top_k_eigenvalues_eigenvectors(adj, 4, True)
    # adopt the device solver's sign convention (largest-magnitude component positive)
    idx = vecs.abs().argmax(dim=1, keepdim=True)
    vecs = vecs * torch.sign(torch.gather(vecs, 1, idx))
    x, p = sr.sast_assemble(tokens, pos, vecs, reverse=True)
    h, res = x + p, None
    cpu = m.cpu()
    with torch.no_grad():
        for layer in cpu.blocks.layers:
            r = scan_ref.MambaRef(64)
            r.load_state_dict(layer.mixer.state_dict())
            res = h if res is None else h + res
            h = r(layer.norm(res))
        want = cpu.cls_head_finetune(cpu.norm(cpu.blocks.norm_f(h + res)).mean(1))
    assert (got - want).abs().max() < 2e-3 * max(1.0, want.abs().max().item())


def test_pointmamba_full_config_train_step(device):
    """BASELINE config 2/3 architecture (12 blocks, d=384, 128 patches -> L=1024): one fwd+bwd+AdamW step."""
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    m = PointMamba(default_config()).to(device).train()
    opt = torch.optim.AdamW(m.parameters(), lr=5e-4, weight_decay=0.05)
    pts = clouds(8, 1024, 1).to(device)
    gt = torch.randint(0, 15, (8,), device=device)
    logits = m(pts)
    assert logits.shape == (8, 15)
    loss, _ = m.get_loss_acc(logits, gt)
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    opt.step()
    assert torch.isfinite(loss)


@pytest.mark.parametrize("shape", [(64, 1024, 128), (5, 2048, 128), (3, 100, 17), (2, 4096, 64), (1, 8, 8)])
def test_farthest_point_sampling_matches_oracle(shape, device):
    """Index work: bit-exact against the restatement of pytorch3d's algorithm (start at 0, squared distances
    accumulated without FMA, first maximum on ties)."""
    from si_mamba_amd import grouping
    B, N, K = shape
    pts = clouds(B, N, seed=N + K)
    centers, idx = grouping.sample_farthest_points(pts.to(device), K)
    wc, widx = fps_ref.sample_farthest_points(pts, K)
    assert torch.equal(idx.cpu(), widx)
    assert torch.equal(centers.cpu(), wc)
    assert (idx[:, 0] == 0).all() and all(len(set(r.tolist())) == K for r in idx.cpu())


def test_graphed_inference_matches_eager(device):
    """The whole PointMamba forward (HIP kernels, GEMMs, side-stream ordering) captured as one hipGraph."""
    from si_mamba_amd.graphed import GraphedForward
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    m = PointMamba(default_config(depth=4, drop_path=0.)).to(device).eval()
    a, b = clouds(4, 1024, 2).to(device), clouds(4, 1024, 3).to(device)
    with torch.no_grad():
        ea, eb = m(a).clone(), m(b).clone()
    g = GraphedForward(m, a)
    ga = g(a).clone()
    gb = g(b).clone()
    assert (ga - ea).abs().max() < 1e-4 and (gb - eb).abs().max() < 1e-4
    assert (ea - eb).abs().max() > 1e-3          # the two inputs really give different outputs


def test_training_reduces_loss_on_separable_clouds(device):
    """End-to-end consistency of forward, backward and optimizer through every HIP op: a small PointMamba has to
    learn two trivially separable synthetic classes (flat discs vs elongated rods) within 40 AdamW steps."""
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    cfg = default_config(trans_dim=64, encoder_dims=64, depth=3, num_group=32, group_size=16, cls_dim=2,
                         drop_path=0., knn_graph=8)
    m = PointMamba(cfg).to(device).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    opt = torch.optim.AdamW(m.parameters(), lr=2e-3, weight_decay=0.0)
    g = torch.Generator().manual_seed(3)

    def batch(B):
        y = torch.randint(0, 2, (B,), generator=g)
        p = torch.randn(B, 256, 3, generator=g)
        scale = torch.where(y[:, None, None] == 0, torch.tensor([1.0, 1.0, 0.05]), torch.tensor([0.1, 0.1, 1.0]))
        p = p * scale
        p = p / p.norm(dim=-1).max(dim=1)[0][:, None, None]
        return p.to(device), y.to(device)

    first = last = None
    for it in range(40):
        pts, y = batch(16)
        loss, acc = m.get_loss_acc(m(pts), y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        if it < 3:
            first = loss.item() if first is None else max(first, loss.item())
        last = loss.item()
    m.eval()
    with torch.no_grad():
        pts, y = batch(64)
        acc = float((m(pts).argmax(-1) == y).float().mean())
    assert last < 0.5 * first and acc > 0.9, (first, last, acc)


@pytest.mark.parametrize("B,N,G,K", [(4, 1024, 128, 32), (2, 2048, 128, 32), (3, 100, 17, 9), (1, 5000, 64, 32),
                                     (2, 64, 8, 64)])
def test_knn_group_matches_exact_neighbours(B, N, G, K, device):
    """Neighbour sets of csrc/knn_group.hip against a float64 brute force (the reference's pytorch3d knn_points,
    return_sorted=False, leaves the order open); output order ascending, ties to the lower index."""
    from si_mamba_amd.grouping import knn_group
    pts = clouds(B, N, N + K)
    centers = pts[:, :G].clone()
    idx = knn_group(centers.to(device), pts.to(device), K).cpu()
    d64 = ((centers.double().unsqueeze(2) - pts.double().unsqueeze(1)) ** 2).sum(-1)          # (B,G,N)
    d32 = (((centers.unsqueeze(2) - pts.unsqueeze(1)) ** 2)[..., 0] + ((centers.unsqueeze(2) - pts.unsqueeze(1)) ** 2)[..., 1]
           + ((centers.unsqueeze(2) - pts.unsqueeze(1)) ** 2)[..., 2])
    picked = torch.gather(d32, 2, idx)
    assert bool((picked[:, :, 1:] >= picked[:, :, :-1]).all())                      # ascending
    assert bool((idx.sort(-1)[0][:, :, 1:] != idx.sort(-1)[0][:, :, :-1]).all())    # distinct
    srt = d64.sort(-1)[0]
    if K < N:
        clear = (srt[:, :, K] - srt[:, :, K - 1]) > 1e-9                            # boundary not a near-tie
        want = d64.topk(K, dim=-1, largest=False)[1].sort(-1)[0]
        same = (idx.sort(-1)[0] == want).all(-1)
        assert bool(same[clear].all()) and float(clear.float().mean()) > 0.9
    else:
        assert bool((idx.sort(-1)[0] == torch.arange(N)).all())


@pytest.mark.parametrize("method", ["HLT", "MAMBA"])
def test_pointmamba_other_orderings_match_oracle_composition(method, device):
    """The classifier's HLT (:1054-1112) and MAMBA (:850-866) routes against the oracle's restatements."""
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    cfg = default_config(trans_dim=64, encoder_dims=64, depth=2, num_group=32, group_size=16, drop_path=0.,
                         knn_graph=8, method=method, k_top_eigenvectors=3)
    m = PointMamba(cfg).to(device).eval()
    m.hlt_rand = False
    pts = clouds(3, 256, 4)
    with torch.no_grad():
        got = m(pts.to(device)).cpu()
        nb, center, _ = m.group_divider(pts.to(device))
        tokens, pos = m.encoder(nb).cpu(), m.pos_embed(center).cpu()
        center = center.cpu()
    if method == "HLT":
        adj = sr.create_graph_from_centers(center, 8, cfg.alpha, True, False, True)
        _, vecs, _, _ = sr.calc_top_k_eigenvalues_eigenvectors(adj, 3, True)
        idx = vecs.abs().argmax(dim=1, keepdim=True)
        vecs = vecs * torch.sign(torch.gather(vecs, 1, idx))                 # the device solver's sign convention
        x, p, _, _ = sr.hlt_order_and_assemble(tokens, pos, center, vecs, 3)
    else:
        ids = [center[:, :, a].argsort(dim=-1)[:, :, None] for a in range(3)]
        x = torch.cat([tokens.gather(1, torch.tile(i, (1, 1, tokens.shape[-1]))) for i in ids], dim=1)
        p = torch.cat([pos.gather(1, torch.tile(i, (1, 1, pos.shape[-1]))) for i in ids], dim=1)
    h, res = x + p, None
    cpu = m.cpu()
    with torch.no_grad():
        for layer in cpu.blocks.layers:
            r = scan_ref.MambaRef(64)
            r.load_state_dict(layer.mixer.state_dict())
            res = h if res is None else h + res
            h = r(layer.norm(res))
        want = cpu.cls_head_finetune(cpu.norm(cpu.blocks.norm_f(h + res)).mean(1))
    assert (got - want).abs().max() < 2e-3 * max(1.0, want.abs().max().item())


def test_pytorch3d_shim_call_forms(device):
    """install_shim(pytorch3d=True): the reference's three pytorch3d calls, in its argument forms."""
    import si_mamba_amd
    si_mamba_amd.install_shim(pytorch3d=True)
    from pytorch3d.loss import chamfer_distance
    from pytorch3d.ops import knn_points, sample_farthest_points
    xyz = clouds(2, 512, 9).to(device)
    center = sample_farthest_points(points=xyz, K=32)[0]                       # models/point_mamba.py:93-94
    idx = knn_points(center, xyz, K=16, return_sorted=False).idx               # :96-97
    assert center.shape == (2, 32, 3) and idx.shape == (2, 32, 16) and idx.dtype == torch.int64
    want = torch.cdist(center.double(), xyz.double()).topk(16, dim=-1, largest=False)[1].sort(-1)[0]
    assert float((idx.sort(-1)[0] == want).float().mean()) > 0.99
    a, b = torch.randn(7, 32, 3, device=device), torch.randn(7, 32, 3, device=device)
    d = chamfer_distance(a, b, batch_reduction=None)[0]                        # :3203
    ref = ((a.unsqueeze(2) - b.unsqueeze(1)) ** 2).sum(-1)
    assert torch.allclose(d, ref.min(2)[0].mean(1) + ref.min(1)[0].mean(1), rtol=1e-5, atol=1e-6)


def test_graphed_train_step_matches_eager(device):
    """Whole training step (zero_grad, forward with the side-stream ordering, backward through every HIP op, gradient
    clipping, optimizer step) captured in one hipGraph: same losses and parameters as the eager step."""
    import copy
    from si_mamba_amd.graphed import GraphedTrainStep
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    cfg = default_config(trans_dim=64, encoder_dims=64, depth=2, num_group=32, group_size=16, cls_dim=5,
                         drop_path=0., knn_graph=8)
    ma = PointMamba(cfg).to(device).train()
    for mod in ma.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    mb = copy.deepcopy(ma)
    # plain SGD: Adam's normalised update turns the last-bit differences of the float-atomic reductions into
    # +-lr steps on near-zero gradients, which makes two correct runs drift apart by themselves
    oa = torch.optim.SGD(ma.parameters(), lr=0.002)
    ob = torch.optim.SGD(mb.parameters(), lr=0.002)
    data = [(clouds(8, 256, 20 + i).to(device), torch.randint(0, 5, (8,), generator=torch.Generator().manual_seed(i)).to(device))
            for i in range(7)]
    step = GraphedTrainStep(lambda p, y: ma.get_loss_acc(ma(p), y)[0], oa, data[0], clip=10.0, warmup=3)
    la, lb = [], []
    # the graphed object has already taken its 3 warm-up steps on data[0] (capture itself executes nothing):
    # mirror them eagerly
    for _ in range(3):
        ob.zero_grad(set_to_none=True)
        loss = mb.get_loss_acc(mb(data[0][0]), data[0][1])[0]
        loss.backward()
        torch.nn.utils.clip_grad_norm_(mb.parameters(), 10.0)
        ob.step()
    for p, y in data[1:]:
        la.append(step(p, y).item())
        ob.zero_grad(set_to_none=True)
        loss = mb.get_loss_acc(mb(p), y)[0]
        loss.backward()
        torch.nn.utils.clip_grad_norm_(mb.parameters(), 10.0)
        ob.step()
        lb.append(loss.item())
    assert max(abs(a - b) for a, b in zip(la, lb)) < 2e-3, (la, lb)
    worst = max(float((pa - pb).abs().max()) for pa, pb in zip(ma.parameters(), mb.parameters()))
    assert worst < 5e-3, worst


# ---- full architecture (12 blocks, d = 384): BASELINE configs 2 and 3 ------------------------------------------------
def _sign_convention(vecs):
    """the device solver's eigenvector sign (largest-magnitude component positive) on oracle vectors"""
    idx = vecs.abs().argmax(dim=1, keepdim=True)
    return vecs * torch.sign(torch.gather(vecs, 1, idx))


@pytest.mark.parametrize("npoints", [1024, 2048])
def test_pointmamba_full_depth_forward_matches_oracle(npoints, device):
    """Configs 2 (1024 points) and 3 (2048 points) architecture at B = 2: FPS + k-NN grouping and the patch encoder on
    the device (covered on their own), then the oracle's graph / eigh / argsort ordering, the oracle's SAST assembly
    and 12 oracle mixers at L = 1024 against the device forward.  fp32, 1e-3 on the normalised error."""
    from compose import oracle_stack, sast_gather_by_order
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    cfg = default_config(drop_path=0.)
    m = PointMamba(cfg).to(device).eval()
    pts = clouds(2, npoints, npoints)
    with torch.no_grad():
        got = m(pts.to(device)).cpu()
        nb, center, _ = m.group_divider(pts.to(device))
        tokens, pos = m.encoder(nb).cpu(), m.pos_embed(center).cpu()
        order_dev = m.spectral_order(center).cpu()
        center = center.cpu()
    adj = sr.create_graph_from_feature_space(center, cfg.knn_graph, cfg.alpha, cfg.symmetric, cfg.self_loop, cfg.binary)
    _, vecs, _, _ = sr.calc_top_k_eigenvalues_eigenvectors(adj, cfg.k_top_eigenvectors, cfg.smallest)
    order = sr.spectral_orders(_sign_convention(vecs))
    # the two orders may differ only inside near-ties of an eigenvector (fp32 solver error); the mixers then see the
    # oracle's order, and a swapped pair of near-identical tokens stays far inside the tolerance
    assert (order == order_dev).float().mean() > 0.99
    x, p = sast_gather_by_order(tokens, pos, order, reverse=cfg.reverse)
    assert x.shape == (2, 1024, 384)
    cpu = m.cpu()
    with torch.no_grad():
        h = oracle_stack(cpu.blocks, 384)(x, p)
        want = cpu.cls_head_finetune(cpu.norm(h).mean(1))
    assert nerr(got, want) < 1e-3


def test_config3_full_batch_step(device):
    """BASELINE config 3 as a whole step: B = 128 clouds of 2048 points -> 128 patches, 12 blocks at L = 1024, forward
    + backward.  Size-independent properties tie the full-size run to the B = 2 case checked against the oracle:
      * eval-mode logits of samples 0-1 inside the batch of 128 equal those of the same model run on just those two;
      * with frozen statistics the summed loss is additive over samples, so every parameter gradient of the batch of
        128 equals grad(first 64) + grad(last 64) (exercises the backward's batch reductions at two grid sizes);
      * the training-mode step (batch statistics, DropPath, dropout) gives finite gradients for every parameter."""
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    m = PointMamba(default_config(drop_path=0.)).to(device).eval()
    pts = clouds(128, 2048, 33).to(device)
    gt = torch.randint(0, 15, (128,), generator=torch.Generator().manual_seed(5)).to(device)
    with torch.no_grad():
        full = m(pts)
        two = m(pts[:2])
    assert nerr(full[:2], two) < 1e-3

    def grads(sl):
        m.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(m(pts[sl]), gt[sl], reduction="sum").backward()
        return {k: p.grad.clone() for k, p in m.named_parameters()}

    g_all, g_a, g_b = grads(slice(0, 128)), grads(slice(0, 64)), grads(slice(64, 128))
    for k in g_all:
        assert nerr(g_all[k], g_a[k] + g_b[k]) < 1e-3, k
    m.train()
    m.zero_grad(set_to_none=True)
    loss, _ = m.get_loss_acc(m(pts), gt)
    loss.backward()
    assert torch.isfinite(loss)
    bad = [k for k, p in m.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not bad, bad


def test_pointmamba_reference_call_surface(device):
    """The reference's forward signature (models/point_mamba.py:843) and the runner's call form
    (tools/runner_finetune.py:201): keywords are accepted, out-of-scope branches are refused by name, ``gt`` returns
    (logits, policy) with the reference's Plackett-Luce term (:953-955)."""
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    cfg = default_config(trans_dim=64, encoder_dims=64, depth=2, num_group=32, group_size=16, drop_path=0., knn_graph=8)
    m = PointMamba(cfg).to(device).eval()
    pts = clouds(3, 256, 1).to(device)
    with torch.no_grad():
        a = m(pts)
        b = m(pts, gt=None, tau=None, use_wavelets=False, save_pts_dir=None, epoch=3)
        assert torch.equal(a, b)
        ret, policy = m(pts, gt=torch.zeros(3, dtype=torch.long, device=device))
        assert torch.equal(ret, a) and policy.shape == (3,)
        center = m.group_divider(pts)[1].cpu()
    adj = sr.create_graph_from_feature_space(center, 8, cfg.alpha, True, False, True)
    vals, vecs, _, _ = sr.calc_top_k_eigenvalues_eigenvectors(adj, 4, True)
    ov = torch.sort(_sign_convention(vecs).transpose(1, 2), dim=-1)[0]
    pl = lambda l: torch.sum(l - torch.logcumsumexp(l.flip(-1), dim=-1).flip(-1), dim=-1)      # reference :2131-2132
    want = pl(-ov).sum(-1) + pl(vals)
    assert (policy.cpu() - want).abs().max() < 1e-3 * max(1.0, want.abs().max().item())
    with pytest.raises(NotImplementedError, match="use_wavelets"):
        m(pts, gt=None, tau=None, use_wavelets=True)
    with pytest.raises(NotImplementedError, match="tau"):
        m(pts, tau=0.5)


def test_first_block_on_distinct_tokens_equals_reference_route(device):
    """MixerModel.forward(tokens, pos, token_index=idx) -- Add + LayerNorm + in_proj of block 0 on the G distinct tokens,
    expanded by the copy kernels of csrc/seq_gather.hip -- against the reference's route on the gathered sequence
    (models/point_mamba.py:889-898, :982-989 then :247-258): outputs, input gradients and every parameter gradient."""
    import copy
    from si_mamba_amd.block import MixerModel
    torch.manual_seed(0)
    a = MixerModel(d_model=128, n_layer=2, drop_path=0.).to(device)
    b = copy.deepcopy(a)
    B, G, k = 3, 64, 4
    g = torch.Generator().manual_seed(1)
    tokens, pos = torch.randn(B, G, 128, generator=g).to(device), torch.randn(B, G, 128, generator=g).to(device)
    order = torch.stack([torch.stack([torch.randperm(G, generator=g) for _ in range(k)]) for _ in range(B)]).to(device)
    idx = torch.cat((order.flatten(1), order.flatten(1).flip(1)), 1)                      # (B, 2 k G)
    calls = []
    from si_mamba_amd import seq_expand
    real = seq_expand.seq_gather_last
    seq_expand.seq_gather_last = lambda *x: (calls.append(1), real(*x))[1]
    try:
        ta, pa = tokens.clone().requires_grad_(True), pos.clone().requires_grad_(True)
        oa = a(ta, pa, token_index=idx, balanced_index=True)
    finally:
        seq_expand.seq_gather_last = real
    assert calls, "the distinct-token route was not taken"
    tb, pb = tokens.clone().requires_grad_(True), pos.clone().requires_grad_(True)
    ex = idx.unsqueeze(-1).expand(-1, -1, 128)
    ob = b(torch.gather(tb, 1, ex), torch.gather(pb, 1, ex))
    w = torch.randn(oa.shape, generator=g).to(device)
    (oa * w).sum().backward()
    (ob * w).sum().backward()
    assert nerr(oa, ob) < 1e-5
    assert nerr(ta.grad, tb.grad) < 1e-4 and nerr(pa.grad, pb.grad) < 1e-4
    for (ka, qa), (_, qb) in zip(a.named_parameters(), b.named_parameters()):
        assert nerr(qa.grad, qb.grad) < 1e-4, ka
    # Any index the caller has not declared balanced (every token exactly L / G times per row) takes the reference's
    # route: here one token is duplicated and one missing -- with the distinct-token adjoint this would sum the wrong
    # positions.  Outputs AND gradients, against the reference composition.
    idx2 = idx.clone()
    idx2[:, 0] = idx2[:, 1]
    calls.clear()
    seq_expand.seq_gather_last = lambda *x: (calls.append(1), real(*x))[1]
    try:
        for mm in (a, b):
            mm.zero_grad(set_to_none=True)
        t2, p2 = tokens.clone().requires_grad_(True), pos.clone().requires_grad_(True)
        o2 = a(t2, p2, token_index=idx2)
    finally:
        seq_expand.seq_gather_last = real
    assert not calls, "an undeclared index must not take the distinct-token route"
    t3, p3 = tokens.clone().requires_grad_(True), pos.clone().requires_grad_(True)
    ex2 = idx2.unsqueeze(-1).expand(-1, -1, 128)
    o3 = b(torch.gather(t3, 1, ex2), torch.gather(p3, 1, ex2))
    (o2 * w).sum().backward()
    (o3 * w).sum().backward()
    assert nerr(o2, o3) < 1e-5
    assert nerr(t2.grad, t3.grad) < 1e-4 and nerr(p2.grad, p3.grad) < 1e-4
    for (ka, qa), (_, qb) in zip(a.named_parameters(), b.named_parameters()):
        assert nerr(qa.grad, qb.grad) < 1e-4, ka


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,C,G,R", [(3, 40, 128, 8), (2, 1536, 64, 8), (1, 5, 256, 8), (2, 16, 32, 4)])
def test_seq_gather_kernels(B, C, G, R, dtype, device):
    from si_mamba_amd import seq_expand
    g = torch.Generator().manual_seed(G + C)
    L = G * R
    x = torch.randn(B, C, G, generator=g).to(device).to(dtype).requires_grad_(True)
    idx = torch.stack([torch.cat([torch.randperm(G, generator=g) for _ in range(R)]) for _ in range(B)]).to(device)
    inv = seq_expand.inverse_positions(idx, G)
    assert torch.equal(torch.gather(idx, 1, inv.flatten(1).long()).view(B, G, R),
                       torch.arange(G, device=device)[None, :, None].expand(B, G, R))
    out = seq_expand.seq_gather_last(x, idx.to(torch.int32), inv)
    want = torch.gather(x.detach(), 2, idx.unsqueeze(1).expand(-1, C, -1))
    assert torch.equal(out, want)                                                   # a copy: bit-exact
    dout = torch.randn(B, C, L, generator=g).to(device).to(dtype)
    out.backward(dout)
    wgrad = torch.zeros(B, C, G, device=device, dtype=torch.float32).scatter_add_(
        2, idx.unsqueeze(1).expand(-1, C, -1), dout.float())
    assert (x.grad.float() - wgrad).abs().max() < (1e-5 if dtype == torch.float32 else 6e-2) * max(1.0, wgrad.abs().max().item())


def test_stack_precomputed_A_matches_per_layer(device):
    """MixerModel forms A = -exp(A_log) of all its layers in one batched op and hands each mixer its slice
    (block.py:_precompute_A): outputs equal the per-layer computation bit for bit, gradients to the rounding of the
    scan backward's atomic accumulation order (which differs from run to run on its own)."""
    from si_mamba_amd.block import MixerModel
    torch.manual_seed(3)
    a = MixerModel(d_model=128, n_layer=3, drop_path=0.).to(device)
    b = MixerModel(d_model=128, n_layer=3, drop_path=0.).to(device)
    b.load_state_dict(a.state_dict())
    b._precompute_A = lambda: [None] * len(b.layers)      # every mixer computes its own A
    x = torch.randn(2, 64, 128, device=device)
    pos = torch.randn(2, 64, 128, device=device)
    ya, yb = a(x, pos), b(x, pos)
    assert torch.equal(ya, yb)
    ya.square().mean().backward()
    yb.square().mean().backward()
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert p.grad is not None and q.grad is not None, k
        scale = max(q.grad.abs().max().item(), 1e-30)
        assert ((p.grad - q.grad).abs().max().item() / scale) < 1e-4, k
    # A travels as an argument: nothing is parked on the modules, so a forward that raises half way leaves no state
    assert all("_A_pre" not in layer.mixer.__dict__ for layer in a.layers)
    boom = a.layers[2].mixer.forward
    a.layers[2].mixer.forward = lambda *x, **k: (_ for _ in ()).throw(RuntimeError("boom"))
    with pytest.raises(RuntimeError, match="boom"):
        a(x, pos)
    a.layers[2].mixer.forward = boom
    a.zero_grad(set_to_none=True)
    assert torch.equal(a(x, pos), yb)                       # and the next forward is unaffected
    assert torch.equal(a.layers[1](x, None)[0], b.layers[1](x, None)[0])       # a Block called on its own
