#!/usr/bin/env python3
"""Time the dense stage on the matrix cores (msgm_sde_stage_dense_mm, csrc/sde_dense_mm_kernels.hip) against
the composed parent it replaces (msgm_sde_stage: the dense branch of k_stage_rows), in one process and one build:
    python tools/time_stage_dense.py [out.json] [--quick]          (out.txt is written next to out.json)
Alternated rounds, medians, the parent route against itself as the yardstick (parent_compare.timed_rounds: "holds" means
the difference is inside that spread and nothing is claimed).

  (a) per launch, the reverse process in Stratonovich form with norm correction, base = x and inc_out (an RK4 / Heun stage),
      noise as dW, n = 31, 32, 40, 48, 64 and B = 160, 1 000, 10 000.  One timed call replays a hipGraph of LAUNCHES stage
      launches and the figures are divided by it, so the host's launch rate is not what is timed.
  (b) the public RK4 / Heun / Euler-Maruyama samplers (MLP with NormalizeLogRadius, norm correction, N = 128, B = 10 000,
      final state only) with ops.stage_dense_mm_preferred as it is and patched to False — how the tests switch routes.
"""
import json, os, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from parent_compare import timed_rounds  # noqa: E402
from sdeflow_light_amd import _lib as L, ops, sde_scheme as SS  # noqa: E402

DEV = torch.device("cuda", 0)
QUICK = "--quick" in sys.argv
LAUNCHES = 10
WIDTHS = (31, 32, 40, 48, 64)
BATCHES = (160, 1000, 10000)
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def dense_tensor(n):
    """A skew tensor scaled as the model's (trace(L_G) = -n/2), from a seed."""
    from sdeflow_light_amd.SDEs import MSGMsde
    torch.manual_seed(1000 + n)
    G = MSGMsde.new_G(n).float()
    L_G = (0.5 * torch.einsum("ijk,jmk->im", G.double(), G.double())).float()
    return G.to(DEV).contiguous(), L_G.to(DEV).contiguous()


def per_launch(row):
    def div(x):
        return [round(v / LAUNCHES, 3) for v in x] if isinstance(x, list) else round(x / LAUNCHES, 3)
    for k in ("parent_us", "parent_again_us", "parent_median_us", "parent_vs_parent_max_us"):
        row[k] = div(row[k])
    for b in row["builds"].values():
        for k in ("us", "median_us", "minus_parent_us"):
            b[k] = div(b[k])
    return row


def stage(n, B, rounds, reps, warm):
    G, L_G = dense_tensor(n)
    packed = ops.pack_dense_g_stage(G, L_G)
    st = L.sde_struct(L.SDE_MSGM_DENSE, 0.1, 20.0, 1.0, 1e-3, G, L_G)
    g = torch.Generator(device=DEV).manual_seed(n * 100003 + B)
    x, a, dW = (torch.randn(B, n, generator=g, device=DEV) for _ in range(3))
    dW *= 1.0 / 128 ** 0.5
    norm0 = ops.row_norm(x)
    out, inc = torch.empty_like(x), torch.empty_like(x)
    kw = dict(dW=dW, norm0=norm0, inc_out=inc)
    args = (out, x, 0.5, x, a, st, L.PROC_REVERSE, True, 0.37, 1.0 / 128, 0.0)
    work = {"rows": lambda: ops.sde_stage(*args, **kw), "mm": lambda: ops.sde_stage_dense_mm(*args, packed=packed, **kw)}
    graphs = {}
    for route, fn in work.items():
        fn()
        torch.cuda.synchronize()
        graphs[route] = ops.new_graph()
        with torch.cuda.graph(graphs[route]):
            for _ in range(LAUNCHES):
                fn()
    row = per_launch(timed_rounds(lambda r: graphs[r].replay(), "rows", [("mm", "mm")], rounds, reps, warm))
    b = row["builds"]["mm"]
    flop = 2.0 * n ** 3 * B * (1 + 1.0 / n)                    # the T GEMM and the L_G block; the 4 n^2 B contraction fmas besides
    row.update(n=n, B=B, launches_per_timed_call=LAUNCHES, speedup=round(row["parent_median_us"] / b["median_us"], 2),
               mm_gflop=round(flop * 1e-9, 3), mm_tflops=round(flop / b["median_us"] * 1e-6, 2))
    say(f"stage n={n:2d} B={B:5d}: k_stage_rows {row['parent_median_us']:9.2f} us (vs itself {row['parent_vs_parent_max_us']:.2f}) | "
        f"k_stage_dense_mm {b['median_us']:8.2f} us ({row['speedup']:.1f}x, {row['mm_tflops']:.1f} TFLOP/s fp32 MFMA) {b['verdict']}")
    return row


def make_gen(d):
    from sdeflow_light_amd.NN import MLP
    from sdeflow_light_amd.SDEs import MSGMsde, PluginReverseSDE
    torch.manual_seed(d)
    Tp = torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)
    base = MSGMsde(torch.randn(64, d), beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=Tp, num_steps_forward=16, device=DEV,
                   denseTensor=True, norm_map="log")
    gen = PluginReverseSDE(base, MLP(d, premodule="NormalizeLogRadius").to(DEV), Tp, deviceReverseSDE=DEV).to(DEV)
    with torch.no_grad():                                       # an untrained net with a small output: the state stays finite
        gen.a.main[6].weight.mul_(0.1)
        gen.a.main[6].bias.mul_(0.1)
    return gen


def samplers(d, B, N, rounds, reps, warm):
    gen = make_gen(d)
    x0 = torch.randn(B, d, device=DEV)
    real = ops.stage_dense_mm_preferred
    rows = {}
    for name, fn in (("rk4", SS.rk4_stratonovich_sampler), ("heun", SS.heun_sampler), ("em", SS.euler_maruyama_sampler)):
        def call(route):
            ops.stage_dense_mm_preferred = real if route == "mm" else (lambda *a: False)
            try:
                fn(gen, x0, num_steps=N, keep_all_samples=False, norm_correction=True)
            finally:
                ops.stage_dense_mm_preferred = real
        row = timed_rounds(call, "rows", [("mm", "mm")], rounds, reps, warm)
        b = row["builds"]["mm"]
        row.update(d=d, B=B, N=N, method=name, speedup=round(row["parent_median_us"] / b["median_us"], 2))
        say(f"sampler {name:4s} d={d} B={B} N={N}: composed on k_stage_rows {row['parent_median_us'] / 1e3:9.2f} ms (vs itself "
            f"{row['parent_vs_parent_max_us'] / 1e3:.2f}) | on k_stage_dense_mm {b['median_us'] / 1e3:8.2f} ms ({row['speedup']:.1f}x) {b['verdict']}")
        rows[name] = row
    return rows


def main():
    out = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    rounds, reps, warm = (1, 3, 1) if QUICK else (3, 5, 1)
    widths, batches = ((33, 64), (160, 10000)) if QUICK else (WIDTHS, BATCHES)
    res = dict(device=torch.cuda.get_device_name(0), rounds=rounds, reps=reps, warmup=warm, dropped_warmup_rounds=1,
               unit="microseconds per stage launch (a) / per sampler call (b); verdicts against the parent route's own spread",
               stages=[stage(n, B, rounds, reps, warm) for n in widths for B in batches],
               samplers=[samplers(d, 10000, 16 if QUICK else 128, 1 if QUICK else 2, 3, 1) for d in ((32,) if QUICK else (32, 48, 64))])
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.splitext(out)[0] + ".txt", "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
