"""Bit-level digests of one training step of every model assembly, for comparing two versions of the package.

For each row: seed, build the model at a small shape, run one training step (forward, loss, backward) under
torch.use_deterministic_algorithms(True), and print one JSON line with the row's name and the sha256 of
  state   the initial state dict (keys and tensors, in order)
  output  what the model returns
  loss    the scalar the backward starts from
  grads   every parameter gradient, in named_parameters order (a missing one is marked as such)
  rand    a torch.rand(4) drawn on the device after the step: where the generator stands
A tolerance against an oracle does not notice a reordered random draw or a swapped gather; equal digests do.  Run this
file from the root of each version in a fresh process and compare the lines (tools/model_digest.py --compare A B
prints the rows and fields that differ).  ``--dump DIR`` also saves each row's tensors, for rows that are not
bit-stable between two runs of one version and have to be compared by their error instead.
"""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def _sha(tensors):
    h = hashlib.sha256()
    for name, t in tensors:
        h.update(name.encode())
        if t is None:
            h.update(b"<none>")
            continue
        t = t.detach().cpu().contiguous()
        h.update(f"{t.dtype}{tuple(t.shape)}".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _clouds(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(B, N, 3, generator=g)
    p = p - p.mean(1, keepdim=True)
    return p / p.norm(dim=-1).max(dim=1)[0][:, None, None]


def _classifier(dev, train=True, amp=False, **over):
    from si_mamba_amd.point_mamba import PointMamba, default_config
    cfg = dict(trans_dim=128, encoder_dims=128, depth=3, group_size=8, num_group=16, knn_graph=4, drop_path=0.3,
               cls_dim=5)
    cfg.update(over)
    m = PointMamba(default_config(**cfg)).to(dev).train(train)
    pts = _clouds(6, 128, 1).to(dev)
    gt = torch.randint(0, 5, (6,), generator=torch.Generator().manual_seed(2)).to(dev)

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            out = m(pts)
            return out, m.get_loss_acc(out, gt)[0]
    return m, step


def _partseg(dev, method):
    from si_mamba_amd.seg import PartSegMamba, default_seg_config, get_loss
    cfg = default_seg_config(trans_dim=64, depth=3, fetch_idx=(0, 1, 2), num_group=32, group_size=16, drop_path=0.,
                             drop_path_rate=0., knn_graph=6, method=method, k_top_eigenvectors=3)
    m = PartSegMamba(50, cfg).to(dev).train()
    B, N = 2, 512
    pts = _clouds(B, N, 3).transpose(1, 2).contiguous().to(dev)
    label = F.one_hot(torch.tensor([3, 7]), 16).float().to(dev)
    target = torch.randint(0, 50, (B, N), generator=torch.Generator().manual_seed(3)).to(dev)
    crit = get_loss()

    def step():
        out = m(pts, label)
        return out, crit(out.reshape(-1, 50), target.view(-1))
    return m, step


def _mae(dev):
    from si_mamba_amd.mae import Point_MAE_Mamba, default_mae_config
    cfg = default_mae_config(trans_dim=64, encoder_dims=64, depth=2, decoder_depth=2, num_group=32, group_size=16,
                             knn_graph=6, k_top_eigenvectors=3, drop_path=0.)
    m = Point_MAE_Mamba(cfg).to(dev).train()
    pts = _clouds(3, 256, 7).to(dev)

    def step():
        loss = m(pts)
        return loss, loss
    return m, step


ROWS = {
    "cls_sast": lambda d: _classifier(d, method="SAST"),
    "cls_mamba": lambda d: _classifier(d, method="MAMBA"),
    "cls_sast_18_patches": lambda d: _classifier(d, method="SAST", num_group=18),
    "cls_input_dropout": lambda d: _classifier(d, method="SAST", drop_out=0.1),
    "cls_hlt": lambda d: _classifier(d, method="HLT"),
    "cls_add_after_layer": lambda d: _classifier(d, method="SAST", add_after_layer=True),
    "cls_sast_eval": lambda d: _classifier(d, train=False, method="SAST"),
    "cls_sast_bf16": lambda d: _classifier(d, amp=True, method="SAST"),
    "cls_sast_rms_norm": lambda d: _classifier(d, method="SAST", rms_norm=True),
    "seg_hlt": lambda d: _partseg(d, "HLT"),
    "seg_sast": lambda d: _partseg(d, "SAST"),
    "seg_point_mamba": lambda d: _partseg(d, "Point_MAMBA"),
    "mae_cdl2": _mae,
}


def run(names, dump=None):
    dev = torch.device("cuda:0")
    torch.use_deterministic_algorithms(True)
    for name in names:
        torch.manual_seed(0)
        m, step = ROWS[name](dev)
        state = [(k, v.clone()) for k, v in m.state_dict().items()]
        torch.manual_seed(1)
        out, loss = step()
        loss.backward()
        rand = torch.rand(4, device=dev)
        torch.cuda.synchronize()
        grads = [(k, p.grad) for k, p in m.named_parameters()]
        parts = dict(state=state, output=[("output", out)], loss=[("loss", loss)], grads=grads, rand=[("rand", rand)])
        print(json.dumps(dict(row=name, **{k: _sha(v) for k, v in parts.items()})), flush=True)
        if dump:
            os.makedirs(dump, exist_ok=True)
            torch.save({k: [(n, None if t is None else t.detach().cpu()) for n, t in v] for k, v in parts.items()},
                       os.path.join(dump, name + ".pt"))


def _nerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / max(1.0, float(b.abs().max()))) if a.numel() else 0.0


def _lines(path):
    with open(path) as f:
        return {r["row"]: r for r in (json.loads(line) for line in f if line.startswith("{"))}


def compare(path_a, path_b, dump_a=None, dump_b=None):
    """Rows and fields whose digests differ between two outputs of this tool; with the two dump directories, the
    largest normalised error of every tensor behind a differing field.  -> number of differing rows"""
    a, b = _lines(path_a), _lines(path_b)
    bad = 0
    for row in a:
        fields = [k for k in a[row] if k != "row" and a[row][k] != b.get(row, {}).get(k)]
        if not fields:
            continue
        bad += 1
        rec = dict(row=row, differ=fields)
        if dump_a and dump_b:
            ta, tb = (torch.load(os.path.join(d, row + ".pt")) for d in (dump_a, dump_b))
            rec["nerr"] = {k: max(_nerr(x, y) for (_, x), (_, y) in zip(ta[k], tb[k]) if x is not None)
                           for k in fields}
        print(json.dumps(rec))
    print(json.dumps(dict(compared=len(a), differing=bad)))
    return bad


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", nargs="*", default=list(ROWS), choices=list(ROWS))
    ap.add_argument("--dump", help="directory to save each row's tensors in")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two outputs instead of running")
    ap.add_argument("--dumps", nargs=2, metavar=("DIR_A", "DIR_B"), help="with --compare: the two runs' --dump dirs")
    args = ap.parse_args()
    if args.compare:
        sys.exit(1 if compare(*args.compare, *(args.dumps or ())) else 0)
    run(args.rows, args.dump)
