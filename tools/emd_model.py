"""A numpy restatement of csrc/emd.hip, round for round (CPU; no GPU code runs here).

What it is for: the round counts behind the default ``max_rounds`` of ``earth_movers_distance``, and how
many bidders are unassigned in a round (what decides whether spreading one bidder's object scan over idle lanes could
pay).  fp32 prices, fp32 costs (dx*dx + dy*dy) + dz*dz, the bid (price + (best - second)) + eps, the new price
max(bid, nextafter(old)), equal bids to the lowest bidder, phases cmax/2, cmax/8, ... clamped at eps_final, the cap.

  python tools/emd_model.py            # the table of DESIGN.md
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

F = np.float32


def emd_model(x, y, eps=0.0, max_rounds=1 << 30):
    """(n, 3), (n, 3) fp32 -> dict(assign, rounds, converged, bidders): ``bidders`` is the number of unassigned bidders
    of every round."""
    x, y = np.asarray(x, dtype=F), np.asarray(y, dtype=F)
    n = x.shape[0]
    d = x[:, None, :] - y[None, :, :]
    cost = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    if n == 1:
        return dict(assign=np.zeros(1, dtype=np.int64), rounds=0, converged=True, bidders=[])
    cmax = cost.max()
    eps_final = F(eps) if eps > 0 else max(cmax * F(1.0 / 16384.0), F(1e-30))
    price = np.zeros(n, dtype=F)
    rounds, conv, bidders = 0, False, []
    e = F(0.5) * cmax
    while not conv:
        e = max(e, eps_final)
        last = not e > eps_final
        owner = np.full(n, -1, dtype=np.int64)
        my = np.full(n, -1, dtype=np.int64)
        while True:
            u = np.flatnonzero(my < 0)
            bidders.append(len(u))
            val = -cost[u] - price[None, :]
            jb = val.argmax(1)                                   # the first maximum
            best = val[np.arange(len(u)), jb]
            val[np.arange(len(u)), jb] = -np.inf
            second = val.max(1)
            bid = (price[jb] + (best - second)) + e
            top = np.full(n, -np.inf, dtype=F)
            np.maximum.at(top, jb, bid)
            wins = bid == top[jb]
            winner = np.full(n, n, dtype=np.int64)
            np.minimum.at(winner, jb[wins], u[wins])
            got = np.flatnonzero(winner < n)
            evicted = owner[got]
            my[evicted[evicted >= 0]] = -1
            owner[got] = winner[got]
            my[winner[got]] = got
            price[got] = np.maximum(top[got], np.nextafter(price[got], F(np.inf)))
            rounds += 1
            if (owner >= 0).all() or rounds >= max_rounds:
                break
        if not (owner >= 0).all():
            break
        if last:
            conv = True
        elif rounds >= max_rounds:
            break
        e = e * F(0.25)
    if not conv:
        free = np.flatnonzero(owner < 0)
        my[np.flatnonzero(my < 0)] = free
    return dict(assign=my, rounds=rounds, converged=conv, bidders=bidders)


def main():
    """Every pair the GPU tests run (tests/test_gpu_emd.py: assignment_ref.EMD_SIZES, both kinds of input)."""
    import assignment_ref as ar
    from si_mamba_amd.emd import default_max_rounds
    print("n kind eps max_rounds_of_the_pairs cap/max max_gap/bound mean_bidders_per_round share_of_rounds_with<=4_bidders")
    for n in ar.EMD_SIZES:
        for kind in ("gaussian", "lattice"):
            pairs = ar.emd_pairs(n)
            x, y, opt, cmax = ar.solved(kind, pairs, n, ar.emd_seed(n))
            eps = ar.lattice_eps(n) if kind == "lattice" else 0.0
            most, ratio, bid = 0, 0.0, []
            for p in range(pairs):
                r = emd_model(x[p].numpy(), y[p].numpy(), eps)
                assert r["converged"] and ar.is_permutation(r["assign"])
                gap = ar.matched_cost(x[p].numpy(), y[p].numpy(), r["assign"]) - opt[p]
                bound = n * (eps if eps > 0 else cmax[p] / 16384.0)
                most, ratio = max(most, r["rounds"]), max(ratio, gap / bound if bound > 0 else 0.0)
                bid += r["bidders"]
            b = np.array(bid if bid else [0])
            print(n, kind, f"{eps:.3g}", most, f"{default_max_rounds(n) / max(most, 1):.1f}", f"{ratio:.4f}",
                  f"{b.mean():.1f}", f"{(b <= 4).mean():.2f}", flush=True)


if __name__ == "__main__":
    main()
