"""GPU parity against fixtures produced by the REFERENCE'S OWN CODE (tests/golden/ref_*.npz, written by
oracle/pin_from_reference.py from /root/reference/models/point_mamba.py and models/block.py; the reference itself is
not on the GPU box -- only these files travel).

The graph / eigen / ordering kernels are held to the ref_spectral_* files by tests/test_gpu_spectral.py (every test
there runs against both fixture families).  Here: the token assembly (SAST index map, HLT order + slot map) and the
block stack -- the reference's Block / MixerModel / create_block / _init_weights around the oracle mixer -- against the
product's Block / MixerModel on the HIP kernels.  The mixer's scan / conv arithmetic is upstream mamba-ssm's (absent):
that part of the comparison is against the oracle's restatement, "parity unpinned" (oracle/__init__.py).
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import nerr

pytestmark = pytest.mark.gpu

NAMES = ["spectral_g64", "spectral_g128", "spectral_g128_surface"]


@pytest.mark.parametrize("name", NAMES)
def test_sast_assembly_equals_reference_index_map(name, device):
    """models/point_mamba.py:889-898 + :982-989 as the reference ran them (index-coded tokens) vs spectral.sast_gather
    and sast_index_map on the reference's orders: index work, bit-exact."""
    from si_mamba_amd import spectral
    from oracle.gen_golden import SPECTRAL_COMBOS
    g = load_golden("ref_" + name)
    B, G = g["centers"].shape[:2]
    tok = torch.arange(G, dtype=torch.float32, device=device)[None, :, None].expand(B, G, 384).contiguous()
    for cb in SPECTRAL_COMBOS:
        t = cb["tag"]
        order = torch.from_numpy(g[f"{t}.order"]).to(device)
        want = torch.from_numpy(g[f"{t}.sast_index"])
        assert torch.equal(spectral.sast_index_map(order, reverse=True).cpu(), want)
        x, p = spectral.sast_gather(tok, tok + 1000.0, order, reverse=True)
        assert torch.equal(x[:, :, 0].long().cpu(), want) and torch.equal(x[:, :, 383].long().cpu(), want)
        assert torch.equal(p[:, :, 5].long().cpu(), want + 1000)
        # sort_points_by_fiedler (:817-826) on the reference's eigenvectors reproduces the reference's orders
        vecs = torch.from_numpy(g[f"{t}.vecs"]).to(device)
        for i in range(4):
            got = spectral.sort_points_by_fiedler(tok, vecs[:, :, i].contiguous())[:, :, 0].long().cpu()
            assert torch.equal(got, torch.from_numpy(g[f"{t}.order"])[:, i]), (t, i)


@pytest.mark.parametrize("name", NAMES)
def test_hlt_equals_reference_outputs(name, device):
    """models/point_mamba.py:1059-1112 as the reference ran it (its own torch.rand tie-break redrawn from the recorded
    seed) vs spectral.multilevel_travers / hlt_assemble: codes, order and the overlapping block assembly, bit-exact."""
    from si_mamba_amd import spectral
    g = load_golden("ref_" + name)
    centers = torch.from_numpy(g["centers"]).to(device)
    vecs = torch.from_numpy(g["hlt.vecs"]).to(device)
    B, G = centers.shape[:2]
    assert torch.equal(spectral.multilevel_travers(vecs, 3).cpu(), torch.from_numpy(g["hlt.codes"]))
    torch.manual_seed(int(g["hlt.rand_seed"]))
    rand = torch.rand(B, G).to(device)                       # the CPU generator the reference's run drew from
    tok = (1.0 + torch.arange(G, dtype=torch.float32, device=device))[None, :, None].expand(B, G, 8).contiguous()
    out_t, out_p, out_c, order = spectral.hlt_assemble(tok, tok + 1000.0, centers, vecs, 3, rand)
    assert torch.equal(order.cpu(), torch.from_numpy(g["hlt.order"]))
    np.testing.assert_array_equal(out_t[:, :, 0].cpu().numpy(), g["hlt.tokens_index"])
    np.testing.assert_array_equal(out_p[:, :, 0].cpu().numpy(), g["hlt.pos_index"])
    np.testing.assert_array_equal(out_c.cpu().numpy(), g["hlt.center"])


def test_block_stack_on_hip_equals_reference_block_and_mixermodel(device):
    """The reference's MixerModel / Block / create_block / _init_weights (models/point_mamba.py:115-272,
    models/block.py:17-76), run from its own files around the oracle mixer, vs this package's MixerModel and Block with
    the same weights on the HIP kernels: forward, input gradients, every parameter gradient, and both Block call forms."""
    from si_mamba_amd.block import MixerModel
    g = load_golden("ref_stack")
    d, n_layer, B, L = (int(v) for v in g["dims"])
    model = MixerModel(d_model=d, n_layer=n_layer, rms_norm=False, drop_path=0.0).to(device)
    sd = {k[len("param."):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param.")}
    assert list(model.state_dict().keys()) == [str(n) for n in g["param_names"]]
    model.load_state_dict(sd)
    x = torch.from_numpy(g["x"]).to(device).requires_grad_(True)
    pos = torch.from_numpy(g["pos"]).to(device).requires_grad_(True)
    out = model(x, pos)
    out.backward(torch.from_numpy(g["dout"]).to(device))
    assert nerr(out, torch.from_numpy(g["out"])) < 1e-3
    assert nerr(x.grad, torch.from_numpy(g["grad_x"])) < 1e-3
    assert nerr(pos.grad, torch.from_numpy(g["grad_pos"])) < 1e-3
    for k, p in model.named_parameters():
        assert nerr(p.grad, torch.from_numpy(g["grad." + k])) < 1e-3, k
    blk = model.layers[0]
    h, r = torch.from_numpy(g["block.h"]).to(device), torch.from_numpy(g["block.r"]).to(device)
    h1, r1 = blk(h, None)
    assert nerr(h1, torch.from_numpy(g["block.first.h"])) < 1e-3 and torch.equal(r1.detach().cpu(), torch.from_numpy(g["block.first.r"]))
    h2, r2 = blk(h, r)
    assert nerr(h2, torch.from_numpy(g["block.next.h"])) < 1e-3
    np.testing.assert_allclose(r2.detach().cpu().numpy(), g["block.next.r"], rtol=0, atol=1e-6)
