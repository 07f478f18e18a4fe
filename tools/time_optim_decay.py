#!/usr/bin/env python3
"""Time msgm_optim_step's instantiations (weight decay, non-finite guard, EMA warm-up) against the PARENT commit's
msgm_adam_step_ex, both libraries loaded into one process (tools/parent_compare.py):
    python tools/time_optim_decay.py <parent libmsgm_hip.so> [out.json] [--quick]
Alternated rounds, the yardstick is the parent against itself (parent_compare.timed_rounds).

  (a) per update at n = 33 794, 819 265 and 4 023 233, every variant with clipping and EMA on (grad_sqnorm + the update:
      40 B per parameter, the same bytes for all of them, so the model ratio is 1 throughout): the parent's
      msgm_adam_step_ex; this tree's msgm_adam_step_ex (the all-off instantiation); msgm_optim_step with everything off,
      with L2 decay, decoupled decay, warm-up, the guard, and all three; and a SKIPPED step (all three on, one NaN in the
      gradient: the norm launch plus an update that leaves in its prologue, model 4 B per parameter).  One timed call
      queues LAUNCHES updates.
  (b) the captured step of the C2 MLP trainer and of the C4 U-Net trainer at its 32-row shard: the present option route
      (clipping, EMA, a schedule) against the same plus weight decay, skip_nonfinite and ema_warmup.
"""
import json, os, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from parent_compare import load, use, timed_rounds  # noqa: E402
from sdeflow_light_amd import _lib, ops  # noqa: E402
from sdeflow_light_amd.train import MLPScoreTrainer, UNetScoreTrainer, warmup_cosine  # noqa: E402
from time_optim_stage import LAUNCHES, SIZES, per_launch  # noqa: E402

DEV = torch.device("cuda", 0)
QUICK = "--quick" in sys.argv
VARIANTS = {                     # name: (decay_mode, guard, warm-up); None = msgm_adam_step_ex
    "this_tree_adam_step_ex": None,
    "optim_step_all_off": (ops.DECAY_NONE, False, False),
    "l2": (ops.DECAY_L2, False, False),
    "adamw": (ops.DECAY_DECOUPLED, False, False),
    "warmup": (ops.DECAY_NONE, False, True),
    "guard": (ops.DECAY_NONE, True, False),
    "adamw_guard_warmup": (ops.DECAY_DECOUPLED, True, True),
    "skipped_step": (ops.DECAY_DECOUPLED, True, True),
}


def kernels(n, new, parent, rounds, reps, warm):
    g0 = torch.Generator(device=DEV).manual_seed(n)
    p, g = torch.randn(n, device=DEV, generator=g0) * 0.1, torch.randn(n, device=DEV, generator=g0) * 0.01
    bad = g.clone()
    bad[n - 1] = float("nan")
    m, v, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    step = torch.ones(1, dtype=torch.int64, device=DEV)
    h6 = ops.opt_hyper(DEV, 1e-4, max_grad_norm=1.0, ema_rate=0.999)
    h7 = ops.optim_hyper(DEV, 1e-4, max_grad_norm=1.0, ema_rate=0.999, weight_decay=0.01)
    skipped = ops.skipped_counter(DEV)
    parts, norm = torch.zeros(ops.grad_sqnorm_partials(n), dtype=torch.float64, device=DEV), torch.zeros((), device=DEV)

    def call(which):
        lib, name = which
        use(lib)
        opt = VARIANTS.get(name)
        gg = bad if name == "skipped_step" else g
        for _ in range(LAUNCHES):
            ops.grad_sqnorm(gg, 1.0, parts)
            if opt is None:
                ops.adam_step_ex(p, gg, m, v, h6, step, ema=ema, partials=parts, grad_norm_out=norm)
            else:
                ops.optim_step(p, gg, m, v, h7, step, ema=ema, partials=parts, grad_norm_out=norm, clip=True,
                               decay_mode=opt[0], skipped=skipped if opt[1] else None, ema_warmup=opt[2])
    row = per_launch(timed_rounds(call, (parent, "parent"), [(k, (new, k)) for k in VARIANTS], rounds, reps, warm))
    use(new)
    assert bool(torch.isfinite(p).all()), "a timed variant damaged the parameters"
    row.update(n=n, launches_per_timed_call=LAUNCHES, model_bytes_per_param=dict(update=40, skipped_step=4))
    print(f"n = {n:8d}: parent clip+ema {row['parent_median_us']:8.2f} us (vs itself {row['parent_vs_parent_max_us']:.2f})  " +
          "  ".join(f"{k} {b['median_us']:.2f} ({b['percent']:+.1f} % {b['verdict']})" for k, b in row["builds"].items()),
          flush=True)
    return row


def trainers(which, rounds, reps, warm):
    from sdeflow_light_amd.data import gaussian_mixture_2d, random_images
    opts = dict(max_grad_norm=1.0, ema_rate=0.999, lr_schedule=warmup_cosine(1e-4, 100, 100000))
    every = dict(opts, weight_decay=0.01, skip_nonfinite=True, ema_warmup=True)
    tr = {}
    for name, kw in (("options", opts), ("every_option", every)):
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
    row = timed_rounds(lambda r: tr[r].step(), "options", [("every_option", "every_option")], rounds, reps, warm)
    row.update(trainer=which, B=tr["options"].B, n_params=tr["options"].n, skipped_steps=tr["every_option"].skipped_steps,
               graph_kernel_nodes={r: ops.graph_node_kinds(t.graph).get("kernel") for r, t in tr.items()})
    b = row["builds"]["every_option"]
    print(f"trainer {which}: clip + EMA + schedule {row['parent_median_us']:10.1f} us (vs itself "
          f"{row['parent_vs_parent_max_us']:.1f}) | plus decay, guard, warm-up {b['median_us']:10.1f} us ({b['percent']:+.2f} %) "
          f"{b['verdict']}", flush=True)
    tr.clear()
    torch.cuda.empty_cache()
    return row


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    new, parent = _lib.lib(), load(args[0])
    out = args[1] if len(args) > 1 else None
    rounds, reps, warm = (1, 3, 1) if QUICK else (3, 7, 2)
    res = dict(device=torch.cuda.get_device_name(0), rounds=rounds, reps=reps, warmup=warm, dropped_warmup_rounds=1,
               unit="microseconds per update (kernels) / per captured step (trainers); verdicts against the parent's own spread",
               kernels=[kernels(n, new, parent, rounds, reps, warm) for n in SIZES],
               trainer=[trainers(w, rounds, 5 if not QUICK else 3, 1) for w in ("c2_mlp", "c4_unet2d_b32")])
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
