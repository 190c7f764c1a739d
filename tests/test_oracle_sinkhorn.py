"""CPU: the dense restatement of the Sinkhorn divergence the GPU tests lean on (sinkhorn_ref.py) has the properties of
the thing it restates: the one-point case in closed form, S(x, x) = 0, a marginal error that falls with the iterations,
and a gradient formula (potentials held fixed) that is the derivative of the converged value."""
import pytest
import torch

import sinkhorn_ref as sr


def test_scaling_steps():
    assert [sr.scaling_steps(e) for e in (1.0, 0.5, 0.3, 2.0 ** -6, 0.05, 0.005, 2.0 ** -9)] == [0, 1, 2, 6, 5, 8, 9]


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-14), (torch.float32, 1e-6)])
def test_one_point_against_one_point(dtype, tol):
    g = torch.Generator().manual_seed(1)
    for _ in range(4):
        x, y = torch.randn(1, 3, generator=g), torch.randn(1, 3, generator=g)
        want = ((x.double() - y.double()) ** 2).sum().item()
        for eps_rel, iters in ((2.0 ** -6, 16), (0.3, 0), (1.0, 3)):
            r = sr.sinkhorn_pair(x, y, eps_rel=eps_rel, iters=iters, dtype=dtype)
            assert abs(r["div"].item() - want) <= tol * want
            assert abs(r["ot_xy"].item() - want) <= tol * want
            assert r["merr"].item() <= tol


@pytest.mark.parametrize("n", [1, 5, 40])
def test_a_set_against_itself(n):
    x = sr.gaussian_sets(1, n, n, 3)[0][0]
    for dtype in (torch.float64, torch.float32):
        r = sr.sinkhorn_pair(x, x.clone(), dtype=dtype)
        assert r["div"].item() == 0.0
        assert not r["dx"].any() and not r["dy"].any()


def test_marginal_error_falls_with_the_iterations():
    x, y = (t[0] for t in sr.gaussian_sets(1, 30, 47, 5))
    merr = [sr.sinkhorn_pair(x, y, eps_rel=2.0 ** -4, iters=k)["merr"].item() for k in (0, 2, 8, 32)]
    assert all(b < a for a, b in zip(merr, merr[1:])), merr
    assert merr[0] > 1e-3 and merr[-1] < 1e-12, merr


@pytest.mark.parametrize("debias", [True, False])
def test_gradient_formula_against_central_differences(debias):
    """Central differences of the float64 value with step h = 2^-15, the temperature held at the unperturbed pair's
    (the formula holds potentials and temperature fixed; the bounding box moves with its extreme points).  What the
    differences resolve: truncation h^2 / 6 |S'''| with |S'''| <= 100 (one coordinate of one point of mass a_i enters
    as a_i 8 R^3 / eps^2 through the third cumulant of the plan's row, R <= 5 the spread of a coordinate and
    eps >= 2.5 here, a few times that with the potentials' response), and rounding 10 ulp64 |OT| / h with |OT| <= 10.
    The iteration count makes merr < 1e-10, so the fixed-potential formula is the derivative to that order."""
    n, m, eps_rel, iters = 7, 9, 2.0 ** -3, 60
    h = 2.0 ** -15
    tol = h * h / 6 * 100 + 10 * 2.2e-16 * 10 / h
    x, y = (t[0] for t in sr.gaussian_sets(1, n, m, 11))
    base = sr.sinkhorn_pair(x, y, eps_rel=eps_rel, iters=iters, debias=debias)
    assert base["merr"].item() < 1e-10
    d2 = base["diam2"].item()
    assert d2 * eps_rel >= 2.5

    def value(xx, yy):
        return sr.sinkhorn_pair(xx, yy, eps_rel=eps_rel, iters=iters, debias=debias, diam2=d2)["div"].item()

    worst = 0.0
    for which, grad in (("x", base["dx"]), ("y", base["dy"])):
        for i in range(grad.shape[0]):
            for c in range(3):
                xp, xm, yp, ym = x.double(), x.double(), y.double(), y.double()
                if which == "x":
                    xp, xm = xp.clone(), xm.clone()
                    xp[i, c] += h
                    xm[i, c] -= h
                else:
                    yp, ym = yp.clone(), ym.clone()
                    yp[i, c] += h
                    ym[i, c] -= h
                step = (xp - xm)[i, c].item() if which == "x" else (yp - ym)[i, c].item()
                fd = (value(xp, yp) - value(xm, ym)) / step
                worst = max(worst, abs(fd - grad[i, c].item()))
    print(f"debias={debias}: worst |fd - formula| {worst:.3e}, tolerance {tol:.3e}")
    assert worst <= tol
