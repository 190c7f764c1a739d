"""CPU: the guarded allocator of the memory-contract tests (tests/guarded_alloc.py) on its own, and on four stand-in
"ops" in plain torch -- one correct, three each broken in the one way a check of the harness is meant to catch."""
import re

import pytest
import torch

from guarded_alloc import GUARD, LARGE, SENTINEL, ZERO, guarded, place, same_bits

CPU = ("cpu",)
DTYPES = [torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.uint8]
REAL = (torch.empty, torch.empty_like, torch.empty_strided)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("poison", [ZERO, SENTINEL], ids=lambda p: p.name)
def test_shape_dtype_layout_and_poison(dtype, poison):
    like = torch.zeros(4, 6, dtype=dtype).t()                        # (6, 4), strides (1, 6)
    with guarded(poison, devices=CPU) as g:
        a = torch.empty(3, 5, 7, dtype=dtype)
        b = torch.empty((11,), dtype=dtype, device="cpu")
        c = torch.empty_like(a)
        d = torch.empty_like(like)
        e = torch.empty_strided((2, 3), (3, 1), dtype=dtype)
        f = torch.empty_like(a, dtype=torch.float32)
        assert len(g.records) == 6
        g.verify()
    want = poison.value(dtype)
    for t, shape in ((a, (3, 5, 7)), (b, (11,)), (c, (3, 5, 7)), (e, (2, 3))):
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
        assert t._base is None and t.data_ptr() % 64 == 0
        assert bool((t == want).all())
    assert d.shape == like.shape and d.stride() == like.stride() and d._base is None     # what torch.empty_like gives
    assert bool((d == want).all())
    assert f.dtype == torch.float32 and bool((f == poison.value(torch.float32)).all())


def test_large_poison_is_finite_and_exact():
    with guarded(LARGE, devices=CPU):
        a = torch.empty(5)
        b = torch.empty(5, dtype=torch.bfloat16)
    assert bool((a == 2.0 ** 100).all()) and bool((b.float() == 2.0 ** 100).all())


def test_zero_elements_and_other_devices():
    with guarded(SENTINEL, devices=CPU) as g:
        z = torch.empty(0, 4)
        m = torch.empty(3, device="meta")                             # not a listed device type: the real function
        g.verify()
        assert len(g.records) == 1
    assert z.shape == (0, 4) and z._base is None and m.device.type == "meta"
    with guarded(SENTINEL) as g:                                      # cuda only: CPU tensors are left alone
        torch.empty(3)
        assert g.records == []


def test_real_functions_come_back():
    with guarded(ZERO, devices=CPU):
        assert torch.empty is not REAL[0]
    assert (torch.empty, torch.empty_like, torch.empty_strided) == REAL
    with pytest.raises(KeyError):
        with guarded(ZERO, devices=CPU):
            raise KeyError("inside")
    assert (torch.empty, torch.empty_like, torch.empty_strided) == REAL
    with pytest.raises(RuntimeError):
        place(torch.zeros(2))                                         # no context is active any more


def test_autograd_sees_a_plain_tensor():
    class Twice(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            out = torch.empty_like(x)
            out.copy_(2 * x)
            return out

        @staticmethod
        def backward(ctx, g):
            dx = torch.empty_like(g)
            dx.copy_(2 * g)
            return dx

    with guarded(SENTINEL, devices=CPU) as g:
        x = place(torch.arange(6.0)).requires_grad_(True)
        y = Twice.apply(x)
        y += 1.0                                                      # legal only on a tensor that is no view
        y.sum().backward()
        g.verify()
    assert torch.equal(x.grad, torch.full((6,), 2.0)) and torch.equal(y.detach(), 2 * torch.arange(6.0) + 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.int64], ids=lambda d: str(d).split(".")[-1])
def test_verify_names_the_allocation(dtype):
    with guarded(SENTINEL, devices=CPU) as g:
        t = torch.empty(5, 3, dtype=dtype)
        other = torch.empty(4, dtype=dtype)
        g.verify()
        past = t.as_strided((1,), (1,), t.storage_offset() + t.numel())          # the raw buffer's own memory
        past.fill_(7)
        with pytest.raises(AssertionError) as err:
            g.verify()
        msg = str(err.value)
        assert "back guard" in msg and "test_guarded_alloc.py" in msg
        assert 0 <= int(re.search(r"byte (\d+) bytes past the end", msg).group(1)) < t.element_size()
        assert "(5, 3)" in msg and str(dtype) in msg and "test_verify_names_the_allocation" in msg
        past.fill_(SENTINEL.value(dtype))
        g.verify()
        before = other.as_strided((1,), (1,), other.storage_offset() - 1)
        before.fill_(7)
        with pytest.raises(AssertionError) as err:
            g.verify()
        msg = str(err.value)
        assert "front guard" in msg and "(4,)" in msg
        assert 0 < int(re.search(r"byte (\d+) bytes before the start", msg).group(1)) <= t.element_size()
    assert GUARD == 4096


def test_place_and_same_bits():
    src = torch.arange(12.0).reshape(3, 4).t()
    with guarded(ZERO, devices=CPU) as g:
        p = place(src)
        assert p._base is None and p.is_contiguous() and torch.equal(p, src) and len(g.records) == 1
    zero = torch.tensor([0.0])
    assert same_bits(zero, zero.clone()) and not same_bits(zero, torch.tensor([-0.0]))
    nan = torch.tensor([float("nan")])
    assert same_bits(nan, nan.clone()) and not same_bits(torch.zeros(2), torch.zeros(3))
    assert not same_bits(torch.zeros(2), torch.zeros(2, dtype=torch.int32))


# ---- stand-in ops: what the harness is for ---------------------------------------------------------------------------
def _op_correct(x):
    out = torch.empty(x.numel())
    out.copy_(3 * x)
    return out


def _op_skips_last(x):                       # (a) leaves the last element of its output unwritten
    out = torch.empty(x.numel())
    out[:-1] = 3 * x[:-1]
    return out


def _op_writes_past(x):                      # (b) one store past the end of its output
    out = torch.empty(x.numel())
    out.as_strided((x.numel() + 1,), (1,), out.storage_offset())[:] = torch.cat([3 * x, x[-1:]])
    return out


def _op_reads_past(x):                       # (c) one load past the end of its input, added into the result
    out = torch.empty(x.numel())
    wide = x.as_strided((x.numel() + 1,), (1,), x.storage_offset())
    out.copy_(3 * x)
    out[-1] += wide[-1]
    return out


def _contract(op):
    """-> (two-poison comparison holds, guards hold) for ``op`` on one seeded input."""
    x = torch.randn(37, generator=torch.Generator().manual_seed(0))
    got, guards = [], True
    for poison in (ZERO, SENTINEL):
        with guarded(poison, devices=CPU) as g:
            got.append(op(place(x)))
            try:
                g.verify()
            except AssertionError:
                guards = False
    return same_bits(got[0], got[1]), guards


def test_the_harness_catches_what_it_is_for():
    assert _contract(_op_correct) == (True, True)
    assert _contract(_op_skips_last)[0] is False
    assert _contract(_op_writes_past)[1] is False
    assert _contract(_op_reads_past)[0] is False
    # each broken op fails only the check meant for it: (a) and (c) leave the guards alone, (b) computes the same values
    assert _contract(_op_skips_last)[1] is True and _contract(_op_reads_past)[1] is True
    assert _contract(_op_writes_past)[0] is True
