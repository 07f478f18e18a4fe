#!/usr/bin/env python3
"""Time the optimizer stage (csrc/optim_kernels.hip) against the plain fused Adam it extends:
    python tools/time_optim_stage.py [out.json] [--quick]
Alternated rounds in one process (parent_compare.timed_rounds: the yardstick is msgm_adam_step against itself).

  (a) per launch, at the three nets' parameter counts n = 33 794 (C2 MLP), 819 265 (C3 1-D U-Net) and 4 023 233 (C4 2-D
      U-Net): msgm_adam_step against [grad_sqnorm +] adam_step_ex for clip, EMA, and both.  One timed call queues
      LAUNCHES updates behind each other, the figures are divided by it: launch latency is hidden by the queue, the
      clip variants still pay their second launch.  The model to compare with is the byte ratio: 28 B per parameter
      for Adam (p, g, m, v in; p, m, v out), +4 for the norm's read of g, +8 for the EMA (in, out).
  (b) the captured step of the C2 MLP trainer and of the C4 U-Net trainer at its 32-row shard, default against all
      options on (clipping at a norm it never reaches would still run both kernels: max_grad_norm = 1.0, EMA 0.999 and
      a schedule).
"""
import json, os, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from parent_compare import timed_rounds  # noqa: E402
from sdeflow_light_amd import ops  # noqa: E402
from sdeflow_light_amd.train import MLPScoreTrainer, UNetScoreTrainer, warmup_cosine  # noqa: E402

DEV = torch.device("cuda", 0)
QUICK = "--quick" in sys.argv
LAUNCHES = 20
SIZES = (33794, 819265, 4023233)
BYTES = {"adam": 28, "clip": 32, "ema": 36, "clip_ema": 40}


def per_launch(row):
    """timed_rounds' microseconds per call -> per update (a call queues LAUNCHES of them)."""
    def div(x):
        return [round(v / LAUNCHES, 3) for v in x] if isinstance(x, list) else round(x / LAUNCHES, 3)
    for k in ("parent_us", "parent_again_us", "parent_median_us", "parent_vs_parent_max_us"):
        row[k] = div(row[k])
    for b in row["builds"].values():
        for k in ("us", "median_us", "minus_parent_us"):
            b[k] = div(b[k])
    return row


def kernels(n, rounds, reps, warm):
    g0 = torch.Generator(device=DEV).manual_seed(n)
    p, g = torch.randn(n, device=DEV, generator=g0) * 0.1, torch.randn(n, device=DEV, generator=g0) * 0.01
    m, v, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    step = torch.ones(1, dtype=torch.int64, device=DEV)
    hyper = ops.opt_hyper(DEV, 1e-4, max_grad_norm=1.0, ema_rate=0.999)
    parts, norm = torch.zeros(ops.grad_sqnorm_partials(n), dtype=torch.float64, device=DEV), torch.zeros((), device=DEV)

    def call(which):
        for _ in range(LAUNCHES):
            if which == "adam":
                ops.adam_step(p, g, m, v, step=0, lr=1e-4, step_dev=step)
                continue
            clip = "clip" in which
            if clip:
                ops.grad_sqnorm(g, 1.0, parts)
            ops.adam_step_ex(p, g, m, v, hyper, step, ema=ema if "ema" in which else None,
                             partials=parts if clip else None, grad_norm_out=norm if clip else None)
    row = per_launch(timed_rounds(call, "adam", [(w, w) for w in ("clip", "ema", "clip_ema")], rounds, reps, warm))
    row.update(n=n, launches_per_timed_call=LAUNCHES, n_partials=parts.numel(),
               model_bytes_per_param=BYTES, model_ratio={k: round(b / 28, 3) for k, b in BYTES.items() if k != "adam"},
               adam_effective_hbm_GBps=round(28.0 * n / (row["parent_median_us"] * 1e-6) / 1e9, 1))
    print(f"n = {n:8d}: adam {row['parent_median_us']:8.2f} us (vs itself {row['parent_vs_parent_max_us']:.2f})  " +
          "  ".join(f"{k} {b['median_us']:8.2f} us (x{b['median_us'] / row['parent_median_us']:.2f}, model x{BYTES[k] / 28:.2f})"
                    for k, b in row["builds"].items()), flush=True)
    return row


def trainers(which, rounds, reps, warm):
    from sdeflow_light_amd.data import gaussian_mixture_2d, random_images
    opts = dict(max_grad_norm=1.0, ema_rate=0.999, lr_schedule=warmup_cosine(1e-4, 100, 100000))
    tr = {}
    for name, kw in (("default", {}), ("options", opts)):
        torch.manual_seed(0)
        if which == "c2_mlp":
            gen, B = bench.build_mlp(DEV), bench.B_C2
            tr[name] = MLPScoreTrainer(gen, B, lr=1e-3, seed=1, **kw)
            tr[name].set_data(gaussian_mixture_2d(B, seed=1234, device=DEV))
        else:
            (gen, d), B = bench.build_unet("c4", DEV), 32
            tr[name] = UNetScoreTrainer(gen, B, d, lr=1e-4, world=1, seed=1, **kw)
            tr[name].set_data(random_images(B, seed=1234, device=DEV))
        tr[name].step()                                           # warm-up step + capture
    row = timed_rounds(lambda r: tr[r].step(), "default", [("options", "options")], rounds, reps, warm)
    row.update(trainer=which, B=tr["default"].B, n_params=tr["default"].n,
               graph_kernel_nodes={r: ops.graph_node_kinds(t.graph).get("kernel") for r, t in tr.items()})
    b = row["builds"]["options"]
    print(f"trainer {which}: default {row['parent_median_us']:10.1f} us (vs itself {row['parent_vs_parent_max_us']:.1f}) | "
          f"all options {b['median_us']:10.1f} us ({b['percent']:+.2f} %) {b['verdict']}", flush=True)
    tr.clear()
    torch.cuda.empty_cache()
    return row


def main():
    out = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    rounds, reps, warm = (1, 3, 1) if QUICK else (3, 7, 2)
    res = dict(device=torch.cuda.get_device_name(0), rounds=rounds, reps=reps, warmup=warm, dropped_warmup_rounds=1,
               unit="microseconds per update (kernels) / per captured step (trainers); verdicts against the parent's own spread",
               kernels=[kernels(n, rounds, reps, warm) for n in SIZES],
               trainer=[trainers(w, rounds, 5 if not QUICK else 3, 1) for w in ("c2_mlp", "c4_unet2d_b32")])
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
