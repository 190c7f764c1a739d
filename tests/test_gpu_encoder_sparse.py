"""GPU: the encoder's last layer and its max as one node (encoder_ops.token_linear_group_max) -- forward bit-equal to
F.linear + group_max_fn, gradients of the sparse backward (csrc/encoder_sparse.hip) against the same ops in float64 on
the CPU.  Tolerances are those of test_gpu_encoder.py: 5e-4 fp32 / 1e-1 bf16 of the largest reference entry; for bf16
the reference is built from the bf16-rounded operands."""
import pytest
import torch

from helpers import peak_err

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 64, 8),          # one column block, one patch
          (3, 32, 128, 384),       # two column blocks, G no multiple of any slab
          (70, 17, 64, 12),        # several slabs with a remainder, n no power of two
          (64, 32, 512, 384)]      # the workload's channel counts


def _operands(G, n, cin, cout, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + G + cin)
    x = torch.randn(G * n, cin, generator=g).to(dtype)
    w = (torch.randn(cout, cin, generator=g) / cin ** 0.5).to(dtype)
    b = torch.randn(cout, generator=g).to(dtype)
    dy = torch.randn(G, cout, generator=g).to(dtype)
    return x, w, b, dy


def _reference(x, w, b, dy, n):
    """float64 on the CPU: linear, max(dim=1), autograd through both."""
    xr, wr, br = (t.double().clone().requires_grad_(True) for t in (x, w, b))
    y = torch.nn.functional.linear(xr, wr, br)
    out = y.view(-1, n, y.shape[1]).max(dim=1)[0]
    out.backward(dy.double())
    return out.detach(), xr.grad, wr.grad, br.grad


def _ours(x, w, b, dy, n, device):
    from si_mamba_amd import _lib
    from si_mamba_amd.encoder_ops import token_linear_group_max
    xa, wa, ba = (t.to(device).clone().requires_grad_(True) for t in (x, w, b))
    with _lib.sparse_max_linear(True):               # the route is chosen in the forward
        out = token_linear_group_max(xa, wa, ba, n)
    out.backward(dy.to(device))
    return out.detach(), xa.grad, wa.grad, ba.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("G,n,cin,cout", SHAPES)
def test_parity_with_float64(G, n, cin, cout, dtype, device):
    from si_mamba_amd import _lib
    from si_mamba_amd.encoder_ops import group_max_fn
    x, w, b, dy = _operands(G, n, cin, cout, dtype)
    before = _lib.counters.get("max_linear_sparse", 0)
    out, dx, dw, db = _ours(x, w, b, dy, n, device)
    assert _lib.counters.get("max_linear_sparse", 0) == before + 1
    # forward: bit-equal to the two ops on the device
    y = torch.nn.functional.linear(x.to(device), w.to(device), b.to(device))
    assert torch.equal(out, group_max_fn(y.view(G, n, cout)))
    ro, rdx, rdw, rdb = _reference(x, w, b, dy, n)
    if dtype == torch.bfloat16:
        # bf16 rounds the product BEFORE the max: among 32 values of 8 significant bits the largest two often round to
        # the same number, and the gradient goes to the first of them, not to the row that wins in float64 (a whole
        # row of dx apart).  The reference therefore takes its winners from the rounded product the forward produced
        # (just shown bit-equal to F.linear's) and is float64 from there on.
        xr, wr, br = (t.double().clone().requires_grad_(True) for t in (x, w, b))
        yr = torch.nn.functional.linear(xr, wr, br).view(G, n, cout)
        pick = y.detach().double().cpu().view(G, n, cout)
        first = (pick == pick.max(dim=1, keepdim=True)[0]).double().argmax(dim=1, keepdim=True)   # first maximum
        yr.gather(1, first).squeeze(1).backward(dy.double())
        rdx, rdw, rdb = xr.grad, wr.grad, br.grad
    tol = 5e-4 if dtype == torch.float32 else 1e-1
    print(f"nerr out {peak_err(out, ro):.3e} dx {peak_err(dx, rdx):.3e} dw {peak_err(dw, rdw):.3e} db {peak_err(db, rdb):.3e}")
    assert peak_err(out, ro) < (1e-4 if dtype == torch.float32 else 2e-2)
    assert dx.dtype == dtype and dw.dtype == dtype and db.dtype == dtype
    assert peak_err(dx, rdx) < tol
    assert peak_err(dw, rdw) < tol
    assert peak_err(db, rdb) < tol


def _planted(G, n, cin, cout, rows):
    """x and W with y[g n + r][c] = 9 where rows[g][c] lists r (two r: an exact tie in patch 0, whose other products are
    exactly 0) and small elsewhere: column i of W reaches row i of x alone."""
    x = torch.zeros(G * n, cin)
    w = 0.01 * torch.randn(cout, cin, generator=torch.Generator().manual_seed(3))
    w[:, :G * n] = 0.
    for g in range(G):
        for c in range(cout):
            for r in rows[g][c]:
                w[c, g * n + r] = 9.0
    x[torch.arange(G * n), torch.arange(G * n)] = 1.0
    x[n:, G * n:] = torch.randn((G - 1) * n, cin - G * n, generator=torch.Generator().manual_seed(4))
    return x, w


def test_edge_cases_ties_and_empty_rows(device):
    """A tie: the first maximum takes the gradient.  A patch whose channels all pick one row, and rows no channel
    picks: their dx rows are exactly zero."""
    G, n, cin, cout = 2, 8, 64, 8
    rows = [[[3, 5]] * cout,                                    # patch 0: every channel ties rows 3 and 5 -> row 3
            [[c % 2] for c in range(cout)]]                     # patch 1: rows 0 and 1 only
    x, w = _planted(G, n, cin, cout, rows)
    b = torch.zeros(cout)
    dy = torch.randn(G, cout, generator=torch.Generator().manual_seed(5))
    out, dx, dw, db = _ours(x, w, b, dy, n, device)
    dx = dx.cpu()
    want = torch.zeros(G * n, cin, dtype=torch.float64)
    want[3] = dy[0].double() @ w.double()
    want[n + 0] = dy[1, 0::2].double() @ w[0::2].double()
    want[n + 1] = dy[1, 1::2].double() @ w[1::2].double()
    for r in range(G * n):
        if r not in (3, n, n + 1):
            assert torch.equal(dx[r], torch.zeros(cin)), r      # exact zeros, the tied row 5 included
    assert peak_err(dx, want) < 5e-4
    wantw = torch.zeros(cout, cin, dtype=torch.float64)
    for c in range(cout):
        wantw[c] = dy[0, c].double() * x[3].double() + dy[1, c].double() * x[n + c % 2].double()
    assert peak_err(dw, wantw) < 5e-4
    assert peak_err(db, dy.double().sum(0)) < 5e-4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_backward_is_bitwise_repeatable(dtype, device):
    x, w, b, dy = _operands(70, 17, 128, 384, dtype, seed=1)
    a = _ours(x, w, b, dy, 17, device)
    c = _ours(x, w, b, dy, 17, device)
    for u, v in zip(a, c):
        assert torch.equal(u, v)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_autocast_rounds_like_the_dense_route(dtype, device):
    """fp32 parameters under autocast: the forward is the dense route's bit for bit, gradients come back in the
    parameters' dtype and match the dense route to the tolerance."""
    from si_mamba_amd import _lib
    x, w, b, dy = _operands(16, 32, 128, 64, torch.float32, seed=2)
    res = []
    for sparse in (True, False):
        with _lib.sparse_max_linear(sparse), torch.autocast("cuda", dtype=torch.bfloat16,
                                                            enabled=dtype == torch.bfloat16):
            xa, wa, ba = (t.to(device).clone().requires_grad_(True) for t in (x, w, b))
            from si_mamba_amd.encoder_ops import token_linear_group_max
            out = token_linear_group_max(xa, wa, ba, 32)
        out.backward(dy.to(device).to(out.dtype))
        res.append((out.detach(), xa.grad, wa.grad, ba.grad))
    assert res[0][0].dtype == dtype and torch.equal(res[0][0], res[1][0])
    tol = 5e-4 if dtype == torch.float32 else 1e-1
    for got, want in zip(res[0][1:], res[1][1:]):
        assert got.dtype == want.dtype == torch.float32
        assert peak_err(got, want) < tol


def test_fallback_outside_the_shape_limits(device):
    """C_in = 96 is no multiple of 64: token_linear + group_max_fn run, with the same results as calling them."""
    from si_mamba_amd import _lib
    from si_mamba_amd.encoder_ops import group_max_fn, token_linear, token_linear_group_max_ok
    x, w, b, dy = _operands(5, 32, 96, 16, torch.float32)
    with _lib.sparse_max_linear(True):
        assert not token_linear_group_max_ok(x.to(device), w.to(device), 32)
        assert token_linear_group_max_ok(x[:, :64].contiguous().to(device), w[:, :64].contiguous().to(device), 32)
    dense, sparse = _lib.counters.get("max_linear_dense", 0), _lib.counters.get("max_linear_sparse", 0)
    got = _ours(x, w, b, dy, 32, device)
    assert _lib.counters.get("max_linear_dense", 0) == dense + 1
    assert _lib.counters.get("max_linear_sparse", 0) == sparse
    xa, wa, ba = (t.to(device).clone().requires_grad_(True) for t in (x, w, b))
    out = group_max_fn(token_linear(xa, wa, ba).view(5, 32, 16))
    out.backward(dy.to(device))
    for u, v in zip(got, (out.detach(), xa.grad, wa.grad, ba.grad)):
        assert torch.equal(u, v)


def test_argument_errors(device):
    from si_mamba_amd import _lib
    lib = _lib.load()
    G, n, cin, cout = 2, 32, 64, 8
    f = torch.zeros(G * n * cin, device=device)
    idx = torch.zeros(G, cout, dtype=torch.uint8, device=device)
    p, i = f.data_ptr(), idx.data_ptr()
    dx = lambda *a: lib.simamba_max_linear_bwd_dx(*a, None)
    dw = lambda *a: lib.simamba_max_linear_bwd_dw(*a, None)
    o1, o2, o3 = (torch.zeros(G * n * cin, device=device) for _ in range(3))     # outputs of the two valid calls
    assert dx(p, i, p, o1.data_ptr(), G, n, cin, cout, 0) == 0
    assert dw(p, i, p, o2.data_ptr(), o3.data_ptr(), G, n, cin, cout, 0) == 0
    assert dx(None, i, p, p, G, n, cin, cout, 0) == -1 and dx(p, None, p, p, G, n, cin, cout, 0) == -1
    assert dx(p, i, None, p, G, n, cin, cout, 0) == -1 and dx(p, i, p, None, G, n, cin, cout, 0) == -1
    assert dw(p, i, None, p, p, G, n, cin, cout, 0) == -1 and dw(p, i, p, None, p, G, n, cin, cout, 0) == -1
    assert dw(p, i, p, p, None, G, n, cin, cout, 0) == -1
    for call in (lambda **k: dx(p, i, p, p, k.get("G", G), k.get("n", n), k.get("cin", cin), k.get("cout", cout),
                                k.get("dt", 0)),
                 lambda **k: dw(p, i, p, p, p, k.get("G", G), k.get("n", n), k.get("cin", cin), k.get("cout", cout),
                                k.get("dt", 0))):
        assert call(cin=96) == -2 and call(cin=32) == -2                    # C_in % 64
        assert call(n=0) == -2 and call(n=33) == -2                         # n out of range
        assert call(cout=6) == -2 and call(cout=388) == -2
        assert call(G=-1) == -2 and call(dt=7) == -3
        assert call(G=0) == 0                                               # nothing to do
    assert dx(p + 4, i, p, p, G, n, cin, cout, 0) == -8                     # alignment
    torch.cuda.synchronize()


def test_bad_index_buffer_contributes_nothing(device):
    """An idx entry >= n takes part in no sum (and in no address), whatever the rows of x hold."""
    from si_mamba_amd import _lib
    lib = _lib.load()
    G, n, cin, cout = 2, 4, 64, 8
    g = torch.Generator().manual_seed(9)
    d = torch.randn(G, cout, generator=g).to(device)
    w = torch.randn(cout, cin, generator=g).to(device)
    x = torch.randn(G * n, cin, generator=g).to(device)
    x[0], x[n] = float("inf"), float("nan")           # rows nobody validly chose: they must not reach any sum
    idx = torch.full((G, cout), 200, dtype=torch.uint8, device=device)
    idx[0, 1] = 2
    dx = torch.full((G * n, cin), 7.0, device=device)
    dw = torch.full((cout, cin), 7.0, device=device)
    part = torch.empty(lib.simamba_max_linear_bwd_slabs(G, cin), cout, cin, device=device)
    st = _lib.stream_ptr(device)
    assert lib.simamba_max_linear_bwd_dx(d.data_ptr(), idx.data_ptr(), w.data_ptr(), dx.data_ptr(), G, n, cin, cout, 0,
                                         st) == 0
    assert lib.simamba_max_linear_bwd_dw(d.data_ptr(), idx.data_ptr(), x.data_ptr(), dw.data_ptr(), part.data_ptr(), G,
                                         n, cin, cout, 0, st) == 0
    wantx = torch.zeros(G * n, cin, device=device)
    wantx[2] = d[0, 1] * w[1]
    wantw = torch.zeros(cout, cin, device=device)
    wantw[1] = d[0, 1] * x[2]
    assert torch.equal(dx, wantx) and torch.equal(dw, wantw)
