#!/usr/bin/env python3
"""GPU box: the 1-D Gaussian KDE log-density kernel (ops.kde_logpdf: k_kde_partial + k_kde_merge) at the workload's
shapes, (M, Ns) = (256, 1e5) and (10 000, 1e5) — the training batch handed to ``evaluate`` against num_samples_init_max
radii (MSGM_higherDim.py:64) — next to the same-GPU torch composition
    torch.logsumexp(-0.5 * ((q[:, None] - r[None, :]) / h) ** 2, 1)
at M = 256 (at M = 10 000 its (M, Ns) temporaries would need 4 GB each, so it is not run there).
Each timed window runs ``--iters`` calls between two device events after a warm-up; the candidates are alternated round
by round in one process and the medians over ``--rounds`` rounds are reported with their spread.  Also reports the
algorithmic rate: M * Ns pairs, one exponential each.  Writes one JSON line per case and, with --out FILE, the list."""
import argparse, json, math, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdeflow_light_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--Ns", type=int, default=100000)
ap.add_argument("--Ms", default="256,10000")
ap.add_argument("--torch-M", type=int, default=256, help="the torch composition runs at this M only")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--out", default="")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_kde.py measures on the GPU; none found")
dev = "cuda"
torch.manual_seed(0)
r = (torch.randn(a.Ns, 4, device=dev) * 1.5).norm(dim=1)            # radii of a d = 4 Gaussian cloud, as the tests use
h = 0.1 * float(r.std())
norm = -math.log(a.Ns) - math.log(h) - 0.5 * math.log(2 * math.pi)


def timeit(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(a.iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / a.iters * 1e-3


cases = []
for M in [int(x) for x in a.Ms.split(",")]:
    q = (torch.randn(M, 4, device=dev) * 1.5).norm(dim=1)
    fns = {"kernel": lambda q=q: ops.kde_logpdf(q, r, h)}
    if M == a.torch_M:
        fns["torch"] = lambda q=q: torch.logsumexp(-0.5 * ((q[:, None] - r[None, :]) / h) ** 2, 1) + norm
        err = float((fns["kernel"]() - fns["torch"]()).abs().max())      # same inputs, same answer (fp32 rounding apart)
    else:
        err = None
    for fn in fns.values():                                              # warm-up: code objects, workspace, allocator
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    cases.append(dict(M=M, fns=fns, t={k: [] for k in fns}, err=err))

for _ in range(a.rounds):                                                # candidates and shapes alternated round by round
    for c in cases:
        for k, fn in c["fns"].items():
            c["t"][k].append(timeit(fn))

res = []
for c in cases:
    tk = statistics.median(c["t"]["kernel"])
    rec = dict(M=c["M"], Ns=a.Ns, h=h, rounds=a.rounds, iters=a.iters, kernel_us=tk * 1e6,
               kernel_spread=(max(c["t"]["kernel"]) - min(c["t"]["kernel"])) / tk, gpairs_per_s=c["M"] * a.Ns / tk / 1e9)
    if "torch" in c["t"]:
        tt = statistics.median(c["t"]["torch"])
        rec.update(torch_us=tt * 1e6, torch_spread=(max(c["t"]["torch"]) - min(c["t"]["torch"])) / tt,
                   torch_over_kernel=tt / tk, max_abs_diff_vs_torch=c["err"])
    res.append(rec)
    print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in rec.items()}), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
