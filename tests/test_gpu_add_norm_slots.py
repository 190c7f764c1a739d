"""GPU: the add + norm kernels on compact batches (simamba_add_layer_norm_fwd_slots / _bwd_slots, csrc/add_norm.hip)
against the SAME build's null-map kernels on expanded operands, bitwise.

Expanded operands: ``hidden`` holds arbitrary finite values under a rowscale of 0 where the compact call has no hidden
rows, ``dnormed`` holds zeros where it has no normed rows.  The arithmetic per row and the order in which a lane
accumulates the weight / bias partials are the same, and a skipped row adds exact zeros, so everything both calls
produce is torch.equal -- residual_out, the mapped normed rows, mean / rstd of the mapped rows, dresidual, the mapped
dhidden rows and the partials.  Sentinels: the compact buffers carry one slot of slack, and no call may touch it.
"""
import ctypes

import pytest
import torch

from si_mamba_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = -12288.0          # exact in bf16 too

# (B, rows, dim): (5, 7, 384) the model width; (3, 5, 96) one partial 16-byte-chunk round (24 of 64 lanes);
# (2, 3, 2048) eight chunks per lane
SHAPES = [(5, 7, 384), (3, 5, 96), (2, 3, 2048)]


def _maps(B, kind):
    """-> (hidden_slot | None, hidden_batch, normed_slot | None, normed_batch) as Python lists."""
    if kind == "hidden_one_out":          # one -1; slots in descending order; the last mapped sample gets scale 0
        hs = [-1] + list(range(B - 2, -1, -1))
        return hs, B - 1, None, B
    if kind == "normed_some_out":
        ns = [-1 if b % 2 else 0 for b in range(B)]
        n = 0
        for b in range(B - 1, -1, -1):     # not ascending: later samples get the lower slots
            if ns[b] == 0:
                ns[b] = n
                n += 1
        return None, B, ns, n
    if kind == "both":                     # one unmapped hidden, another sample's normed unmapped, orders differ
        hs = list(range(B - 1)) + [-1]
        ns = [-1] + list(range(B - 2, -1, -1))
        return hs, B - 1, ns, B - 1
    if kind == "normed_none":
        return None, B, [-1] * B, 0
    if kind == "hidden_none":
        return [-1] * B, 0, None, B
    raise AssertionError(kind)


KINDS = ["hidden_one_out", "normed_some_out", "both", "normed_none", "hidden_none"]
# without a residual there is nothing a sample without hidden rows could take: the normed maps only
# (test_bad_arguments has the refusal)
RES_KINDS = [(True, k) for k in KINDS] + [(False, k) for k in ("normed_some_out", "normed_none")]


def _case(B, L, d, dtype, device, seed):
    g = torch.Generator().manual_seed(seed)
    t = dict(h=torch.randn(B, L, d, generator=g).to(dtype), r=torch.randn(B, L, d, generator=g),
             s=(torch.rand(B, generator=g) > 0.3).float() / 0.7, w=1 + 0.1 * torch.randn(d, generator=g),
             b=0.1 * torch.randn(d, generator=g), dn=torch.randn(B, L, d, generator=g).to(dtype),
             dr=torch.randn(B, L, d, generator=g))
    return {k: v.to(device) for k, v in t.items()}


def _p(t):
    return None if t is None else t.data_ptr()


def _run(lib, st, c, has_res, rms, hslot, hb, nslot, nb, hidden, dnormed, dtype, slots):
    """One forward + backward through the *_slots entry points (``slots``) or the *_ex ones; hidden / dnormed are the
    operands to hand over; compact buffers get one slot of slack filled with the sentinel."""
    B, L, d = c["r"].shape
    dev = c["r"].device
    code = _lib.dtype_code(dtype)
    flags = _lib.NORM_RMS if rms else 0
    ro = torch.full((B, L, d), SENTINEL, device=dev)
    nm = torch.full((nb + 1, L, d), SENTINEL, device=dev, dtype=dtype)
    mean = torch.full((B * L,), SENTINEL, device=dev)
    rstd = torch.full((B * L,), SENTINEL, device=dev)
    dres = torch.full((B, L, d), SENTINEL, device=dev)
    dhid = torch.full((hb + 1, L, d), SENTINEL, device=dev, dtype=dtype)
    grid = lib.simamba_add_layer_norm_grid(B, L)
    part = torch.full((grid, 2, d), SENTINEL, device=dev)
    res = c["r"] if has_res else None
    rs = c["s"] if has_res else None
    bias = None if rms else c["b"]
    head = (_p(hidden), _p(res), _p(rs), _p(c["w"]), _p(bias), _p(ro), _p(nm), None if rms else _p(mean), _p(rstd))
    if slots:
        rc = lib.simamba_add_layer_norm_fwd_slots(*head, _p(hslot), hb, _p(nslot), nb, B, L, d, 1e-5, code, code,
                                                  flags, st)
    else:
        rc = lib.simamba_add_layer_norm_fwd_ex(*head, B, L, d, 1e-5, code, code, flags, st)
    assert rc == 0
    head = (_p(dnormed), _p(c["dr"]), _p(ro), None if rms else _p(mean), _p(rstd), _p(c["w"]), _p(rs),
            _p(dres) if has_res else None, _p(dhid), _p(part))
    if slots:
        rc = lib.simamba_add_layer_norm_bwd_slots(*head, _p(hslot), hb, _p(nslot), nb, B, L, d, code, code, flags, st)
    else:
        rc = lib.simamba_add_layer_norm_bwd_ex(*head, B, L, d, code, code, flags, st)
    assert rc == 0
    torch.cuda.synchronize()
    return dict(ro=ro, nm=nm, mean=mean, rstd=rstd, dres=dres, dhid=dhid, part=part)


@pytest.mark.parametrize("has_res,kind", RES_KINDS, ids=[("res-" if r else "nores-") + k for r, k in RES_KINDS])
@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_slots_equal_the_null_map_kernels_on_expanded_operands(shape, dtype, rms, has_res, kind, device):
    lib = _lib.load()
    st = _lib.stream_ptr(device)
    B, L, d = shape
    hs, hb, ns, nb = _maps(B, kind)
    c = _case(B, L, d, dtype, device, seed=B * 1000 + d)
    if hs is not None:
        # every unmapped sample has scale 0, and so has one mapped sample (it stays in with its zeros)
        mapped = [b for b in range(B) if hs[b] >= 0]
        for b in range(B):
            if hs[b] < 0:
                c["s"][b] = 0.0
        if mapped:
            c["s"][mapped[-1]] = 0.0
    # the reference: null maps, whole batch; dnormed zero where the compact call has none
    dn_full = c["dn"].clone()
    if ns is not None:
        for b in range(B):
            if ns[b] < 0:
                dn_full[b] = 0
    want = _run(lib, st, c, has_res, rms, None, B, None, B, c["h"], dn_full, dtype, slots=False)
    # the compact operands (slack slot = sentinel; a finite value, so reading it would not go unnoticed either)
    hidden, hslot = c["h"], None
    if hs is not None:
        hslot = torch.tensor(hs, dtype=torch.int32, device=device)
        hidden = torch.full((hb + 1, L, d), SENTINEL, device=device, dtype=dtype)
        for b in range(B):
            if hs[b] >= 0:
                hidden[hs[b]] = c["h"][b]
    dnormed, nslot = c["dn"], None
    if ns is not None:
        nslot = torch.tensor(ns, dtype=torch.int32, device=device)
        dnormed = torch.full((nb + 1, L, d), SENTINEL, device=device, dtype=dtype)
        for b in range(B):
            if ns[b] >= 0:
                dnormed[ns[b]] = c["dn"][b]
    got = _run(lib, st, c, has_res, rms, hslot, hb, nslot, nb, hidden, dnormed, dtype, slots=True)

    hmap = hs if hs is not None else list(range(B))
    nmap = ns if ns is not None else list(range(B))
    assert torch.equal(got["ro"], want["ro"])
    if has_res:
        assert torch.equal(got["dres"], want["dres"])
    assert torch.equal(got["part"][:, :1 if rms else 2], want["part"][:, :1 if rms else 2])
    for b in range(B):
        rows = slice(b * L, (b + 1) * L)
        if nmap[b] >= 0:
            assert torch.equal(got["nm"][nmap[b]], want["nm"][b]), b
            assert torch.equal(got["rstd"][rows], want["rstd"][rows]), b
            if not rms:
                assert torch.equal(got["mean"][rows], want["mean"][rows]), b
        if hmap[b] >= 0:
            assert torch.equal(got["dhid"][hmap[b]], want["dhid"][b]), b
    # nothing outside the mapped slots was written: the slack, and slots no sample maps to
    for buf, smap, n in ((got["nm"], nmap, nb), (got["dhid"], hmap, hb)):
        taken = {s for s in smap if s >= 0}
        for s in range(n + 1):
            if s not in taken:
                assert bool((buf[s].float() == SENTINEL).all()), s


# Null maps: the *_ex entry points ARE the *_slots ones with null maps (they forward), so there is nothing to compare
# within one build; that null maps compute what they computed before rests on the existing float64 and oracle tests of
# the add + norm kernels (test_gpu_add_norm.py, test_gpu_rms_norm.py, test_gpu_out_norm.py).


def test_bad_arguments(device):
    """Validation in front of the launch: nothing below is dereferenced on the device."""
    lib = _lib.load()
    n = None
    one = ctypes.c_void_p(16)
    B = 4

    def fwd(hidden=one, residual=one, res_out=one, normed=one, hslot=one, hb=2, nslot=one, nb=2):
        return lib.simamba_add_layer_norm_fwd_slots(hidden, residual, n, one, n, res_out, normed, one, one, hslot, hb,
                                                    nslot, nb, B, 8, 64, 1e-5, 0, 0, 0, n)

    def bwd(dnormed=one, dhidden=one, dres=one, hslot=one, hb=2, nslot=one, nb=2):
        return lib.simamba_add_layer_norm_bwd_slots(dnormed, n, one, one, one, one, n, dres, dhidden, one, hslot, hb,
                                                    nslot, nb, B, 8, 64, 0, 0, 0, n)
    # a compact batch outside [0, batch]
    assert fwd(hb=B + 1) == -2 and fwd(nb=-1) == -2 and bwd(hb=-1) == -2 and bwd(nb=B + 1) == -2
    # a null map with a compact batch set
    assert fwd(hslot=n, hb=2) == -1 and fwd(nslot=n, nb=0) == -1 and bwd(hslot=n, hb=3) == -1 and bwd(nslot=n) == -1
    # a compact hidden without a residual (or nowhere to put the sum)
    assert fwd(residual=n) == -1 and fwd(res_out=n) == -1
    # missing tensors count only where the compact batch has samples
    assert fwd(hidden=n) == -1 and fwd(normed=n) == -1 and bwd(dnormed=n) == -1
    assert bwd(dhidden=n, dres=n) == -1 and bwd(dhidden=one, dres=n, hb=0) == -1
    # the host-checked map: range, duplicates, null
    chk = lib.simamba_add_layer_norm_check_slots
    arr = (ctypes.c_int * 4)

    def at(*v):
        return ctypes.cast(arr(*v), ctypes.c_void_p)
    assert chk(at(0, -1, 1, -1), 4, 2) == 0
    assert chk(at(1, -1, 0, -1), 4, 2) == 0                   # any order
    assert chk(at(-1, -1, -1, -1), 4, 0) == 0
    assert chk(at(0, -1, 2, -1), 4, 2) == -2                  # slot >= compact batch
    assert chk(at(0, -2, 1, -1), 4, 2) == -2
    assert chk(at(0, 0, 1, -1), 4, 2) == -2                   # one slot, two samples
    assert chk(at(0, 1, 2, 3), 4, 5) == -2 and chk(at(0, 1, 2, 3), 4, -1) == -2
    assert chk(n, 4, 2) == -1
    # the Python op refuses a compact hidden without a residual before any launch
    from si_mamba_amd.add_norm import add_layer_norm_fn
    h = torch.zeros(2, 8, 64, device=device)
    with pytest.raises(ValueError):
        add_layer_norm_fn(h, None, torch.ones(64, device=device), None,
                          hidden_slot=torch.zeros(4, dtype=torch.int32, device=device))
