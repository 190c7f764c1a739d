"""From dataset to batch (csrc/dataset.hip, si_mamba_amd/data.py) on one GPU, B = 64.

(a) The call time of DeviceLoader.fetch() at three stores generated on the device from a seed:
      modelnet     S =  9 843 clouds of 8 192 points, K = 1 024, permute
      shapenet55   S = 52 470 clouds of 8 192 points, K = 1 024, permute + unit_sphere
      shapenetpart S = 14 000 clouds of 2 000 - 3 000 points (ragged), K = 2 048, choice
    A round is `--calls` calls between a device synchronise in front and one behind, timed with the host clock (what a
    training loop waits for, enqueue included); the rounds of the three alternate; [median, min, max] us per call.
    `kernel_us`: the fetch kernel and the step kernel behind it between a pair of device events around each launch.

(b) Clouds/s of the bf16-autocast PointMamba training step in a captured graph (GraphedTrainStep, default_config, 1 024
    points), fed three ways on the same machine, the windows of the three alternating:
      static    one batch that sits on the device, replayed: what bench.py and the other tools here measure
      device    the loader inside the graph (modelnet store, permute + unit_sphere); no input is copied
      host      a torch DataLoader written anew in the shape of the reference's (tools/builder.py: shuffle, drop_last,
                persistent workers; pageable memory, the 786 KB batch is one copy) over in-memory numpy arrays of the same size, every item shuffling
                its point indices, taking K of them and normalising them with numpy as datasets/ShapeNet55Dataset.py
                does, with min(16, CPUs) workers; the batch is copied to the device and into the step's static input
    `host_alone` is the host loader drained with no step behind it (clouds/s it can produce at all).
    The workers are forked before this process touches the GPU, so none of them has it open.

    python tools/bench_loader.py [--calls 200] [--rounds 5] [--steps 40] [--out profiles/device_loader.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import measure  # noqa: E402

B = 64
CLASSES = 15          # default_config().cls_dim: a label outside [0, cls_dim) traps in torch's nll_loss kernel


class HostClouds(torch.utils.data.Dataset):
    """In-memory (S, n, 3) float32; an item is K shuffled rows, centred and scaled, and a label."""

    def __init__(self, S, n, K, seed=0):
        rng = np.random.default_rng(seed)
        self.points = rng.random((S, n, 3), dtype=np.float32) * 2 - 1
        self.labels = rng.integers(0, CLASSES, S)
        self.K = K

    def __len__(self):
        return len(self.points)

    def __getitem__(self, i):
        idx = np.arange(self.points.shape[1])
        np.random.shuffle(idx)
        pc = self.points[i, idx[:self.K]]
        pc = pc - np.mean(pc, axis=0)
        pc = pc / np.max(np.sqrt(np.sum(pc ** 2, axis=1)))
        return torch.from_numpy(pc).float(), int(self.labels[i])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40, help="training steps per window of part (b)")
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--host-clouds", type=int, default=9843)
    ap.add_argument("--skip-fetch", action="store_true")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--deviations", default=None, help="JSON file with what the GPU tests printed, copied into the result")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_loader.json"))
    args = ap.parse_args()

    # the host loader first: its workers fork here, before this process opens the GPU
    host_iter = None
    if not args.skip_train:
        host_set = HostClouds(args.host_clouds, 8192, 1024)
        host_loader = torch.utils.data.DataLoader(host_set, batch_size=B, shuffle=True, drop_last=True,
                                                  num_workers=args.workers, persistent_workers=args.workers > 1,
                                                  pin_memory=False)
        host_iter = iter(host_loader)
        first = next(host_iter)                              # every worker is up

    measure.require_gpu("bench_loader.py")
    from si_mamba_amd import _lib
    from si_mamba_amd.data import DeviceDataset, DeviceLoader
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), batch=B)

    def device_store(S, n, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        pts = torch.rand(S, n, 3, device=dev, generator=g) * 2 - 1
        labels = torch.randint(0, CLASSES, (S,), device=dev, generator=g)
        return DeviceDataset.from_arrays(pts, labels, device=dev)

    def ragged_store(S, lo, hi, seed):
        g = torch.Generator().manual_seed(seed)
        counts = torch.randint(lo, hi + 1, (S,), generator=g)
        total = int(counts.sum())
        gd = torch.Generator(device=dev).manual_seed(seed)
        pts = torch.rand(total, 3, device=dev, generator=gd) * 2 - 1
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)]).to(dev)
        seg = torch.randint(0, 50, (total,), device=dev, generator=gd).int()
        return DeviceDataset(pts, offsets, 0, torch.randint(0, 16, (S,), device=dev, generator=gd), seg)

    modelnet = device_store(9843, 8192, 1)

    if not args.skip_fetch:
        shapes = {
            "modelnet": (modelnet, dict(npoints=1024, subsample="permute")),
            "shapenet55": (device_store(52470, 8192, 2), dict(npoints=1024, subsample="permute", normalize="unit_sphere")),
            "shapenetpart": (ragged_store(14000, 2000, 3000, 3), dict(npoints=2048, subsample="choice")),
        }
        loaders, outs = {}, {}
        for name, (store, kw) in shapes.items():
            loaders[name] = DeviceLoader(store, B, seed=5, **kw)
            outs[name] = loaders[name].fetch()
            for _ in range(3):
                loaders[name].fetch(out=outs[name])
        us = measure.rounds({name: (lambda name=name: measure.host_clock(
            lambda: loaders[name].fetch(out=outs[name]), steps=args.calls, warmup=0) * 1e3) for name in shapes},
            args.rounds)
        rows = []
        for name, (store, kw) in shapes.items():
            _lib.enable_kernel_timing(True, only=["dataset_fetch"])
            for _ in range(50):
                loaders[name].fetch(out=outs[name])
            torch.cuda.synchronize()
            _, kernel_ms = _lib.kernel_times()["dataset_fetch"]
            _lib.enable_kernel_timing(False)
            rows.append(dict(store=name, clouds=len(store), store_GB=round(store.nbytes / 1e9, 3), **kw,
                             fetch_us=measure.stats(us[name], 2), kernel_us=round(kernel_ms * 1e3, 2), launches_per_call=2,
                             h2d_copies_per_call=0, host_reads_per_call=0))
            print(json.dumps(rows[-1]), flush=True)
        res["fetch"] = dict(calls=args.calls, rounds=args.rounds, rows=rows)
        del shapes, loaders, outs

    if not args.skip_train:
        from si_mamba_amd.graphed import GraphedTrainStep
        from si_mamba_amd.point_mamba import PointMamba, default_config
        amp = torch.autocast("cuda", dtype=torch.bfloat16)
        if default_config().cls_dim != CLASSES:
            raise SystemExit(f"the stores' labels are drawn from {CLASSES} classes, the model has {default_config().cls_dim}")
        loader = DeviceLoader(modelnet, B, 1024, subsample="permute", normalize="unit_sphere", seed=7)

        def build(loss_of, example):
            torch.manual_seed(0)
            model = PointMamba(default_config(drop_path=0.)).to(dev).train()
            opt = torch.optim.AdamW(model.parameters(), lr=5e-4, weight_decay=0.05, capturable=True)

            def loss_fn(*inputs):
                pts, gt = loss_of(*inputs)
                with amp:
                    return model.get_loss_acc(model(pts), gt)[0]
            return GraphedTrainStep(loss_fn, opt, example, clip=10.0, warmup=3)

        pts0, gt0 = first[0].to(dev), first[1].to(dev)

        def from_loader(_):
            b = loader.fetch()
            return b.points, b.label

        static_step = build(lambda p, y: (p, y), (pts0, gt0))
        host_step = build(lambda p, y: (p, y), (pts0, gt0))
        device_step = build(from_loader, (torch.zeros(1, device=dev),))

        def host_batches():
            nonlocal host_iter
            while True:
                for batch in host_iter:
                    yield batch
                host_iter = iter(host_loader)
        feed = host_batches()

        def host_fed():
            p, y = next(feed)
            host_step(p.to(dev, non_blocking=True), y.to(dev, non_blocking=True))
        one = {"static": static_step, "device": device_step, "host": host_fed, "host_alone": lambda: next(feed)}

        def window(kind):
            return B / measure.host_clock(one[kind], steps=args.steps, warmup=0) * 1e3

        kinds = ["static", "device", "host", "host_alone"]
        for k in kinds:
            window(k)
        rate = {k: [] for k in kinds}
        for _ in range(args.rounds):
            for k in kinds:
                rate[k].append(window(k))
                print(k, round(rate[k][-1], 1), flush=True)
        res["train"] = dict(steps_per_window=args.steps, rounds=args.rounds, workers=args.workers,
                            cpus=os.cpu_count(), host_clouds=args.host_clouds,
                            clouds_per_s={k: measure.stats(v, 1) for k, v in rate.items()})

    if args.deviations:
        with open(args.deviations) as fh:
            res["deviations"] = json.load(fh)
    res["what"] = ("fetch: [median, min, max] us per DeviceLoader.fetch() call, host clock between two device "
                   "synchronises, rounds alternating over the stores; kernel_us between device events.  train: "
                   "[median, min, max] clouds/s of the bf16 PointMamba GraphedTrainStep at B = 64 x 1024 points over "
                   "alternating windows: static batch | device loader inside the graph | host DataLoader + H2D copy; "
                   "host_alone: the host DataLoader drained without a step")
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    if host_iter is not None:
        del host_iter, host_loader


if __name__ == "__main__":
    main()
