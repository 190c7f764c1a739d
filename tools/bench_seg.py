"""Part-segmentation train step (BASELINE config 5 shapes: 2048 points -> 128 patches, HLT ordering L=256 or SAST
L=1024), fwd+bwd+AdamW: clouds/s on one GPU (tuning / reporting tool, not the judged bench).  ``--dp``: the data-parallel
step, one rank by default or one per GPU under torchrun (clouds/s of this rank) -- with ``--graph`` the two-graph
GraphedTrainStep around one all-reduce, without it DistributedDataParallel (wrap_ddp)."""
import argparse, os, sys, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tools import measure
from si_mamba_amd.seg import PartSegMamba, default_seg_config, get_loss
from si_mamba_amd.synthetic import make_clouds

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--npoints", type=int, default=2048)
ap.add_argument("--method", default="HLT")
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--graph", action="store_true", help="capture the whole step in one hipGraph (GraphedTrainStep)")
ap.add_argument("--dp", action="store_true", help="data-parallel step over torch.distributed (RCCL)")
args = ap.parse_args()
measure.require_gpu("bench_seg.py")
dev = torch.device("cuda:0")
rank, world = 0, 1
if args.dp:
    import torch.distributed as dist
    from si_mamba_amd.dist import init_dist, one_rank_env, wrap_ddp
    one_rank_env()
    rank, world = init_dist("nccl")
    dev = torch.device("cuda", torch.cuda.current_device())
torch.manual_seed(0)
m = PartSegMamba(50, default_seg_config(method=args.method)).to(dev).train()
opt = torch.optim.AdamW(m.parameters(), lr=2e-4, weight_decay=0.05, fused=True, capturable=args.graph)
pts = make_clouds(args.batch, args.npoints, rank).to(dev).transpose(1, 2).contiguous()
label = torch.nn.functional.one_hot(torch.randint(0, 16, (args.batch,)), 16).float().to(dev)
target = torch.randint(0, 50, (args.batch, args.npoints), device=dev)
crit = get_loss()
amp = torch.autocast("cuda", dtype=torch.bfloat16, enabled=args.dtype == "bf16")

net = wrap_ddp(m, dev) if args.dp and not args.graph else m

def step():
    opt.zero_grad(set_to_none=True)
    with amp:
        out = net(pts, label)
    loss = crit(out.reshape(-1, 50), target.view(-1))
    loss.backward()
    opt.step()
    return loss

if args.graph:
    from si_mamba_amd.graphed import GraphedTrainStep

    def loss_fn(p, lab, tgt):
        with amp:
            out = m(p, lab)
        return crit(out.reshape(-1, 50), tgt.view(-1))
    dp = dict(process_group=dist.group.WORLD, module=m) if args.dp else {}
    gstep = GraphedTrainStep(loss_fn, opt, (pts, label, target), **dp)
    step = lambda: gstep(pts, label, target)
for _ in range(6):                                        # (allocator growth and library one-offs reach into step 3)
    step()
import gc; gc.collect()     # (a full collection costs ~80 ms here: outside the timed steps)
def timed_step():
    global loss
    loss = step()
dt = measure.host_clock(timed_step, steps=args.steps, warmup=0) / 1e3
if rank == 0:
    print(json.dumps({"workload": f"part segmentation train step, {args.method}, {args.npoints} pts, B={args.batch}, {args.dtype}" + (", hipGraph" if args.graph else "") + (f", data-parallel, {world} rank(s)" if args.dp else ""),
                      "ms_per_step": round(dt * 1e3, 2), "clouds_per_s": round(args.batch / dt, 1), "loss": float(loss)}))
if args.dp:
    dist.destroy_process_group()
