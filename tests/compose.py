"""Shared pieces of the model-level parity tests: the oracle composition of the reference's block stack.

TEST INFRASTRUCTURE.  ``oracle_stack`` restates MixerModel.forward (reference models/point_mamba.py:247-258) and
Block.forward (models/block.py:47-73) around CPU oracle mixers (oracle.scan_ref.MambaRef) that carry the device
model's weights.  ``io_dtype=torch.bfloat16`` restates the same stack as it runs under ``torch.autocast`` on the
reference's CUDA path: LayerNorm computes and returns fp32 (autocast's fp32 list), the residual stream is fp32
(``residual = drop_path(hidden) + residual`` promotes), every mixer op reads and writes bf16 with fp32
accumulation (MambaRef.forward's ``io_dtype``), and ``input_ids + pos`` follows torch's type promotion (a bf16 add
when both operands arrive as bf16).
"""
import torch

from helpers import scaled_err
from oracle import scan_ref


def mixer_oracle_run(ref, h, dout, io_dtype=None, f64=False):
    """{'out', 'hidden', <parameter names>}: forward, input gradient and parameter gradients of one CPU oracle run of
    the mixer ``ref`` (scan_ref.MambaRef): fp32, the bf16-autocast restatement (``io_dtype``), or -- ``f64`` -- the
    float64 statement of the same weights and inputs, with float64 gradients."""
    m = scan_ref.mamba_ref_f64(ref) if f64 else ref
    m.zero_grad(set_to_none=True)
    hh = (h.double() if f64 else h.clone()).requires_grad_(True)
    out = m(hh, io_dtype=io_dtype, acc_dtype=torch.float64 if f64 else torch.float32)
    out.backward(dout.double() if f64 else dout)
    res = {"out": out.detach(), "hidden": hh.grad}
    res.update({k: p.grad for k, p in m.named_parameters()})
    m.zero_grad(set_to_none=True)
    return res


def mixer_scaled_bound_violations(ref, h, dout, got, dtype, names):
    """The scale-aware bound of tests/test_gpu_mixer_routes.py (see its docstring for the reasoning) on the tensors
    ``names`` of a device result ``got``: E_dev <= 16 * max(E_ref, 2^-23) in fp32, <= 4 * E_ref under bf16 autocast,
    both errors measured against the float64 mixer, E_ref being the CPU oracle of that dtype.  -> list of violations."""
    want = mixer_oracle_run(ref, h, dout, f64=True)
    cpu = mixer_oracle_run(ref, h, dout, io_dtype=None if dtype == torch.float32 else dtype)
    factor, floor = (16.0, 2.0 ** -23) if dtype == torch.float32 else (4.0, 0.0)
    bad = []
    for k in names:
        e_ref, e_dev = scaled_err(cpu[k], want[k]), scaled_err(got[k], want[k])
        print(f"{k}: E_ref {e_ref[0]:.3e} / {e_ref[1]:.3e}  E_dev {e_dev[0]:.3e} / {e_dev[1]:.3e}")
        bad += [(k, what, d, r) for what, d, r in zip(("max", "rms"), e_dev, e_ref) if not d <= factor * max(r, floor)]
    return bad


def oracle_mixers(layers, d, d_state=16):
    refs = []
    for layer in layers:
        r = scan_ref.MambaRef(d, d_state=d_state)
        r.load_state_dict({k: v.detach().cpu() for k, v in layer.mixer.state_dict().items()})
        refs.append(r.eval())
    return refs


def oracle_stack(mixer_model, d, io_dtype=None, taps=None):
    """-> run(x, pos): norm_f(h + residual) after the last layer, or the list of taps after the layers in ``taps``
    (MixerModelForSegmentation.forward, part_segmentation/models/pt_mamba.py:390-416)."""
    refs = oracle_mixers(mixer_model.layers, d)
    r = (lambda t: t) if io_dtype is None else (lambda t: t.to(io_dtype).float())
    ln = torch.nn.functional.layer_norm

    def norm(mod, t):
        return ln(t.float(), (d,), mod.weight.detach().float().cpu(), mod.bias.detach().float().cpu(), mod.eps)

    def run(x, pos):
        # input_ids + pos with torch's own promotion: a bf16 + bf16 add rounds to bf16, anything else is an fp32 add
        h, res, feats = (x.cpu() + pos.cpu()).float(), None, []
        for i, (layer, ref) in enumerate(zip(mixer_model.layers, refs)):
            res = h if res is None else h + res
            h = ref(norm(layer.norm, res), io_dtype=io_dtype)
            if taps is not None and i in taps:
                feats.append(norm(mixer_model.norm_f, h + res))
        return feats if taps is not None else norm(mixer_model.norm_f, h + res)
    return run


def sast_gather_by_order(tokens, pos, order, reverse=True):
    """Token assembly of reference :889-898 + :982-989 from (B,k,G) orders: the k gathers concatenated, then their
    flip -- written out with the reference's own ops."""
    xs, ps = [], []
    for i in range(order.shape[1]):
        idx = order[:, i].unsqueeze(-1)
        xs.append(torch.gather(tokens, 1, idx.expand(-1, -1, tokens.shape[-1])))
        ps.append(torch.gather(pos, 1, idx.expand(-1, -1, pos.shape[-1])))
    x, p = torch.cat(xs, 1), torch.cat(ps, 1)
    if reverse:
        x, p = torch.cat((x, x.flip(1)), 1), torch.cat((p, p.flip(1)), 1)
    return x, p
