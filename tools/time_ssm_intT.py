#!/usr/bin/env python3
"""Time the integrated SSM loss (PluginReverseSDE(ssm_intT=True)) against existing code:
    python tools/time_ssm_intT.py [out.json] [--quick]
parent_compare.timed_rounds alternates (yardstick, yardstick again, new) and the verdict of the new route is taken against
the largest yardstick-vs-yardstick difference of a round.  Every number is a device-event time of eager calls (host
launches included) unless it says "queued".

  (a) msgm_forward_paths against msgm_forward_paths_composed per call, nsf = 16, Philox noise, every state kept: the
      composed chain (6 nsf launches that each stream the state) is existing code and the yardstick
  (b) the captured MLPScoreTrainer step at EQUAL TRAINING ROWS per step: ssm_intT with B = 4096 / nsf' paths against the
      default trainer at 4096 rows (the yardstick), d = 6 sparse and d = 16 dense, nsf = 16.  The two are different
      estimators: equal in rows per step, not in what they optimise — a cost ratio, no statement about convergence
  (c) the forward launch alone at those sizes: msgm_forward_paths on 4096 / nsf' paths against msgm_forward_perturb on
      4096 rows, as eager calls and as 20 launches queued behind each other through the C ABI (the kernels' own time)
"""
import json, os, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from parent_compare import timed_rounds  # noqa: E402
from sdeflow_light_amd import ops, sde_scheme as SS, _lib as L  # noqa: E402
from sdeflow_light_amd.SDEs import MSGMsde, PluginReverseSDE  # noqa: E402

DEV = torch.device("cuda", 0)
QUICK = "--quick" in sys.argv
NSF, ROWS = 16, 4096
PATHS = [("sparse", 4096, 1024), ("sparse", 256, 12288), ("dense", 4096, 16), ("dense", 4096, 64)]
STEPS = [("sparse", 6, "NormalizeLogRadius"), ("dense", 16, None)]


def Tp():
    return torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)


def base_for(kind, n, T=None):
    return MSGMsde(torch.randn(1024, n), beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=T or Tp(), num_steps_forward=NSF, device=DEV,
                   denseTensor=(kind == "dense"), norm_map="log").to(DEV)


def line(tag, row, old, new):
    b = row["builds"][new]
    print(f"{tag:<46} {old} {row['parent_median_us']:10.1f} us (vs itself {row['parent_vs_parent_max_us']:7.1f}) | {new} "
          f"{b['median_us']:10.1f} us ({b['percent']:+.1f} %, x{row['parent_median_us'] / b['median_us']:.2f}) {b['verdict']}", flush=True)


def queued(launch, reps=20):
    """Microseconds per launch when `reps` are queued behind each other: the kernel's own time, launch latency hidden."""
    for _ in range(3):
        launch()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        launch()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def c_paths(base, x0):
    ts, delta = SS._forward_grid(base, NSF, x0.device)
    B, n = x0.shape
    y, st, lib = torch.empty(NSF, B, n, device=DEV), base.struct(), L.lib()
    return lambda: L.check(lib.msgm_forward_paths(L.ptr(x0), L.ptr(y), B, n, st, NSF, 0, L.ptr(ts), float(delta), float(delta ** 0.5),
                                                  float(delta * 0.5), float(delta * 1.0), None, base.rng.ptr(), L.stream()), "msgm_forward_paths")


def c_perturb(base, x0, t):
    ts, delta = SS._forward_grid(base, NSF, x0.device)
    B, n = x0.shape
    y, st, lib = torch.empty_like(x0), base.struct(), L.lib()
    return lambda: L.check(lib.msgm_forward_perturb(L.ptr(x0), L.ptr(t), L.ptr(y), None, B, n, st, NSF, L.ptr(ts), float(delta),
                                                    float(delta ** 0.5), float(delta * 0.5), float(delta * 1.0), None, None,
                                                    base.rng.ptr(), L.stream()), "msgm_forward_perturb")


def paths_alone(kind, B, n, rounds, reps, warm):
    torch.manual_seed(0)
    base = base_for(kind, n)
    base.rng = L.PhiloxState(7, DEV)
    x0 = torch.randn(B, n, device=DEV) * 1.5
    route = {"composed": SS.msgm_forward_paths_composed, "kernel": SS.msgm_forward_paths}
    s0 = base.rng.state.clone()
    ref = route["composed"](base, x0)
    base.rng.state.copy_(s0)
    same = bool(torch.equal(route["kernel"](base, x0), ref))
    del ref
    row = timed_rounds(lambda r: route[r](base, x0), "composed", [("kernel", "kernel")], rounds, reps, warm)
    kus = queued(c_paths(base, x0))
    row.update(kind=kind, B=B, n=n, nsf=NSF, bitwise_equal=same, launches_composed=6 * NSF, kernel_queued_us=round(kus, 2),
               kernel_effective_hbm_GBps=round(4.0 * (1 + NSF) * B * n / (kus * 1e-6) / 1e9, 1))
    line(f"(a) paths {kind} B={B} n={n} nsf={NSF}", row, "composed", "kernel")
    print(f"      kernel alone, 20 launches queued: {kus:.1f} us each = {row['kernel_effective_hbm_GBps']} GB/s of the "
          f"4 (1 + nsf) B/element it must move", flush=True)
    return row


def trainer(kind, d, pre, intT):
    from sdeflow_light_amd.NN import MLP
    from sdeflow_light_amd.train import MLPScoreTrainer
    torch.manual_seed(0)
    T = Tp()
    gen = PluginReverseSDE(base_for(kind, d, T), MLP(d, premodule=pre).to(DEV), T, ssm_intT=intT, deviceReverseSDE=DEV).to(DEV)
    B = ROWS // NSF if intT else ROWS
    tr = MLPScoreTrainer(gen, B, lr=1e-4, seed=1)
    tr.set_data(torch.randn(B, d, device=DEV) * 1.5)
    first = float(tr.step())                                  # warm-up step + capture
    assert tr.rows == ROWS and first == first
    return tr


def step_and_forward(kind, d, pre, rounds, reps, warm):
    tr = {"default": trainer(kind, d, pre, False), "ssm_intT": trainer(kind, d, pre, True)}
    row = timed_rounds(lambda r: tr[r].step(), "default", [("ssm_intT", "ssm_intT")], rounds, reps, warm)
    row.update(kind=kind, d=d, nsf=NSF, rows_per_step=ROWS, paths_per_step=ROWS // NSF,
               graph_kernel_nodes={r: ops.graph_node_kinds(tr[r].graph).get("kernel") for r in tr},
               step_ratio_default_over_intT=round(row["parent_median_us"] / row["builds"]["ssm_intT"]["median_us"], 3))
    line(f"(b) captured MLP step {kind} d={d}, {ROWS} rows", row, "default", "ssm_intT")
    # (c) the forward launch alone
    base = base_for(kind, d)
    base.rng = L.PhiloxState(7, DEV)
    xr, xp = torch.randn(ROWS, d, device=DEV) * 1.5, torch.randn(ROWS // NSF, d, device=DEV) * 1.5
    t = torch.rand(ROWS, device=DEV).clamp(min=1e-3)
    call = {"perturb": lambda: SS.msgm_forward_perturb(base, t, xr), "paths": lambda: SS.msgm_forward_paths(base, xp)}
    fwd = timed_rounds(lambda r: call[r](), "perturb", [("paths", "paths")], rounds, reps, warm)
    q_perturb, q_paths = queued(c_perturb(base, xr, t)), queued(c_paths(base, xp))
    fwd.update(kind=kind, d=d, nsf=NSF, rows=ROWS, paths=ROWS // NSF, perturb_queued_us=round(q_perturb, 2), paths_queued_us=round(q_paths, 2),
               queued_ratio_perturb_over_paths=round(q_perturb / q_paths, 3), expected_ratio_nsf_over_2=NSF / 2)
    line(f"(c) forward alone {kind} d={d}, {ROWS} rows", fwd, "perturb", "paths")
    print(f"      queued through the C ABI: perturb {q_perturb:.1f} us, paths {q_paths:.1f} us: x{q_perturb / q_paths:.2f} "
          f"per training row (nsf / 2 = {NSF / 2:.0f})", flush=True)
    del tr
    torch.cuda.empty_cache()
    return row, fwd


def main():
    out = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    rounds, reps, warm = (1, 3, 1) if QUICK else (3, 7, 2)
    res = dict(device=torch.cuda.get_device_name(0), rounds=rounds, reps=reps, warmup=warm, dropped_warmup_rounds=1,
               unit="microseconds; verdict of the new route against the yardstick's own spread", paths=[], step=[], forward=[])
    for kind, B, n in PATHS:
        res["paths"].append(paths_alone(kind, B, n, rounds, reps, warm))
    for kind, d, pre in STEPS:
        s, f = step_and_forward(kind, d, pre, rounds, reps, warm)
        res["step"].append(s)
        res["forward"].append(f)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
