#!/usr/bin/env python3
"""Wall time of the MLP samplers at the driver's sizes (MSGM_higherDim.py:903: B = 10 000, N = 128, keep_all_samples=True):
the one-launch loop (msgm_mlp_sde_loop / msgm_mlp_xw_sde_loop / msgm_mlp_dense_sde_loop, what the public samplers route to) against the composed
path (score net, stage kernels and glue as separate launches), alternated round by round in ONE process, device-synchronised, after a warm-up.
The composed path is also timed against itself (a second call in every round): the difference of the two medians is the
spread a routing decision has to beat.

    python tools/time_mlp_sde.py [--rounds 7] [--B 10000] [--steps 128] [--only TEXT] [--out FILE]

Times cover the sampler up to the device synchronisation (set-up, every launch, trajectory capture), not the copy of
the trajectory to the host, which both routes share.  One JSON line per (configuration, method)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

NLR = "NormalizeLogRadius"
CONFIGS = [  # (name, SDE family, d, premodule, norm correction)
    ("sgm d=2", "sgm", 2, None, False),
    ("dense d=2 NLR nc", "dense", 2, NLR, True),
    ("sparse d=6 NLR nc", "sparse", 6, NLR, True),
    ("sparse d=20 nc", "sparse", 20, None, True),
] + [c for d in (40, 64, 90, 128) for c in (   # the extra-wide class (msgm_mlp_xw_sde_loop): the widths of the real data sets
    (f"sgm d={d}", "sgm", d, None, False), (f"sparse d={d} NLR nc", "sparse", d, NLR, True))] + [
    # dense tensors above n = 16 (msgm_mlp_dense_sde_loop): the driver's default model at its real-data widths
    (f"dense d={d} NLR nc", "dense", d, NLR, True) for d in (17, 24, 30)]


def make_gen(kind, d, pre, dev):
    from sdeflow_light_amd.NN import MLP
    from sdeflow_light_amd.SDEs import SGMsde, MSGMsde, PluginReverseSDE
    T = torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)
    if kind == "sgm":
        base = SGMsde(T=T, num_steps_forward=16, device=dev)
    else:
        base = MSGMsde(torch.randn(64, d), T=T, num_steps_forward=16, device=dev, denseTensor=(kind == "dense"), norm_map="log")
    gen = PluginReverseSDE(base, MLP(d, premodule=pre).to(dev), T, deviceReverseSDE=dev).to(dev)
    with torch.no_grad():                       # an untrained net at full size makes the multiplicative SDEs overflow
        gen.a.main[6].weight.mul_(0.1)
        gen.a.main[6].bias.mul_(0.1)
    return gen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--B", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--only", default="", help="time the configurations whose name contains this text")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from sdeflow_light_amd import ops, sde_scheme as SS
    ops.mlp_xw_sde_loop_preferred = ops.mlp_xw_sde_loop_supported   # time the loop wherever the kernel takes the shape
    ops.mlp_dense_sde_loop_preferred = ops.mlp_dense_sde_loop_supported
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    out = open(a.out, "w") if a.out else None

    def run(method, gen, x0, nc, loop):
        args = (gen, x0, a.steps, 0.0, True, None, False, -1, nc, None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if method == "em":
            if loop:
                r = SS._em(*args)
            else:                                   # the composed Euler-Maruyama steps: the loop is the shape rule's choice
                r = SS._Run(*args)
                other = torch.empty_like(r.x)
                for i in range(a.steps):
                    if SS._em_step(r.clock(i), r.x, other, r.norm0) is other:
                        r.x, other = other, r.x
                    r.after_step(i)
        elif method == "heun":
            r = SS._integrate(SS._heun_step, (1.0,), 4, *args, loop="heun" if loop else None)
        else:
            r = SS._rk4(*args, loop="rk4" if loop else None)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        r.result()                                   # advances the Philox stream as the public sampler does
        return dt * 1e3

    for name, kind, d, pre, nc in CONFIGS:
        if a.only not in name:
            continue
        gen = make_gen(kind, d, pre, dev)
        x0 = torch.randn(a.B, d, device=dev)
        for method in ("rk4", "heun") + (("em",) if kind != "sgm" else ()):
            for loop in (True, False):              # warm-up: code objects, allocator
                run(method, gen, x0, nc, loop)
            t = {"loop": [], "composed": [], "composed_again": []}
            for _ in range(a.rounds):
                t["loop"].append(run(method, gen, x0, nc, True))
                t["composed"].append(run(method, gen, x0, nc, False))
                t["composed_again"].append(run(method, gen, x0, nc, False))
            med = {k: statistics.median(v) for k, v in t.items()}
            spread = abs(med["composed"] - med["composed_again"])
            rec = {"config": name, "method": method, "B": a.B, "steps": a.steps, "rounds": a.rounds,
                   "loop_ms": round(med["loop"], 3), "composed_ms": round(med["composed"], 3),
                   "composed_again_ms": round(med["composed_again"], 3), "spread_ms": round(spread, 3),
                   "loop_range_ms": [round(min(t["loop"]), 3), round(max(t["loop"]), 3)],
                   "composed_range_ms": [round(min(t["composed"] + t["composed_again"]), 3),
                                         round(max(t["composed"] + t["composed_again"]), 3)],
                   "speedup": round(med["composed"] / med["loop"], 2),
                   "loop_wins": bool(med["composed"] - med["loop"] > spread)}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
