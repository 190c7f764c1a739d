"""MAE pre-training step (BASELINE config 4 shapes: 1024 points -> 64 patches, mask 0.6, encoder L=208, decoder
L=512, bf16 autocast), fwd+bwd+AdamW: clouds/s on one GPU (tuning / reporting tool, not the judged bench).
``--dp``: the data-parallel step, one rank by default or one per GPU under torchrun (clouds/s of this rank) -- with
``--graph`` the two-graph GraphedTrainStep around one all-reduce, without it DistributedDataParallel (wrap_ddp).
Reference log for scale: 0.79-0.83 s per batch of 128 (~160 clouds/s, logs/pretrain_part_1.log:123-125)."""
import argparse, os, sys, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tools import measure
from si_mamba_amd.mae import Point_MAE_Mamba, default_mae_config
from si_mamba_amd.synthetic import make_clouds

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--loss", default="cdl2", help="config.loss: cdl1, cdl2 or emd")
ap.add_argument("--graph", action="store_true", help="capture the whole step in one hipGraph (GraphedTrainStep)")
ap.add_argument("--dp", action="store_true", help="data-parallel step over torch.distributed (RCCL)")
args = ap.parse_args()
measure.require_gpu("bench_mae.py")
dev = torch.device("cuda:0")
rank, world = 0, 1
if args.dp:
    import torch.distributed as dist
    from si_mamba_amd.dist import init_dist, one_rank_env, wrap_ddp
    one_rank_env()
    rank, world = init_dist("nccl")
    dev = torch.device("cuda", torch.cuda.current_device())
torch.manual_seed(0)
m = Point_MAE_Mamba(default_mae_config(loss=args.loss)).to(dev).train()
params = [p for k, p in m.named_parameters() if not k.startswith("decoder_pos_embed.")]
opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=0.05, fused=True, capturable=args.graph)
pts = make_clouds(args.batch, 1024, rank).to(dev)
amp = torch.autocast("cuda", dtype=torch.bfloat16, enabled=args.dtype == "bf16")

net = wrap_ddp(m, dev) if args.dp and not args.graph else m

def step():
    opt.zero_grad(set_to_none=True)
    with amp:
        loss = net(pts)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(params, 10.0)
    opt.step()
    return loss

if args.graph:
    from si_mamba_amd.graphed import GraphedTrainStep

    def loss_fn(p):
        with amp:
            return m(p)
    dp = dict(process_group=dist.group.WORLD, module=m) if args.dp else {}
    gstep = GraphedTrainStep(loss_fn, opt, (pts,), params=params, clip=10.0, **dp)
    step = lambda: gstep(pts)
for _ in range(6):                                        # (allocator growth and library one-offs reach into step 3)
    step()
import gc; gc.collect()     # (a full collection costs ~80 ms here: outside the timed steps)
def timed_step():
    global loss
    loss = step()
dt = measure.host_clock(timed_step, steps=args.steps, warmup=0) / 1e3
if rank == 0:
    print(json.dumps({"workload": f"MAE pre-train step, B={args.batch}, 1024 pts -> 64 patches, {args.dtype}, loss {args.loss}" + (", hipGraph" if args.graph else "") + (f", data-parallel, {world} rank(s)" if args.dp else ""),
                      "ms_per_step": round(dt * 1e3, 2), "clouds_per_s": round(args.batch / dt, 1), "loss": float(loss)}))
if args.dp:
    dist.destroy_process_group()
