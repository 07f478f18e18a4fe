#!/usr/bin/env python3
"""Time the data stage (csrc/data_kernels.hip):
    python tools/time_data_stage.py [out.json] [--quick]          (out.txt is written next to out.json)
Alternated rounds in one process (parent_compare.timed_rounds: the yardstick is the first variant against itself).

  (a) per launch: msgm_data_gather at 65 536 x 2 from a 10^6 x 2 table and at 32 x 12 288 from a 2 10^4 x 12 288 table,
      next to msgm_data_gather_epoch (the whole table, and its first 2^k + 1 rows: the longest cycle walk),
      msgm_ssm_prep alone and the fused msgm_ssm_prep_gather at the same shapes.  One timed call replays a hipGraph
      of LAUNCHES launches (each at its own stream offset: other rows every launch) and the figures are divided by it,
      so the host's launch rate is not what is timed.  The byte model of the gather is the rows read plus
      the rows written, 8 B d per row (a 2-float row still costs the memory system a whole line: the model is a floor).
  (b) the captured steps of the C2 MLP trainer and of the C4 U-Net trainer at its 32-row shard:
        fixed      the fixed-batch step (a trainer without data=: the launches of the parent commit)
        data       data=ArrayData — the gather rides in the prep launch
        unfused    data=ArrayData with the gather as a launch of its own ahead of the unchanged prep
        epoch      data=ArrayData(replace=False): msgm_data_gather_epoch, the cursor advance, then the unchanged prep
        host       the fixed-batch step with a host-side sample (numpy index draw + fancy-index copy, data.py:691-693)
                   and set_data before each replay: what a driver without the data stage has to do
"""
import json, os, sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from parent_compare import timed_rounds  # noqa: E402
from sdeflow_light_amd import _lib as L, ops  # noqa: E402
from sdeflow_light_amd.data import ArrayData  # noqa: E402
from sdeflow_light_amd.train import MLPScoreTrainer, UNetScoreTrainer  # noqa: E402

DEV = torch.device("cuda", 0)
QUICK = "--quick" in sys.argv
LAUNCHES = 20
SHAPES = ((65536, 2, 10 ** 6), (32, 12288, 2 * 10 ** 4))
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def per_launch(row):
    def div(x):
        return [round(v / LAUNCHES, 3) for v in x] if isinstance(x, list) else round(x / LAUNCHES, 3)
    for k in ("parent_us", "parent_again_us", "parent_median_us", "parent_vs_parent_max_us"):
        row[k] = div(row[k])
    for b in row["builds"].values():
        for k in ("us", "median_us", "minus_parent_us"):
            b[k] = div(b[k])
    return row


def kernels(B, d, N, rounds, reps, warm):
    tab = torch.randn(N, d, device=DEV)
    x, y, v = (torch.empty(B, d, device=DEV) for _ in range(3))
    t, ctr = torch.empty(B, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    st = L.sde_struct(L.SDE_SGM, 0.1, 20.0, 1.0, 1e-3)
    rngs = [L.PhiloxState(1, DEV, offset=i) for i in range(LAUNCHES)]      # other rows every launch, no advance launch

    # the epoch route: other stream positions every launch (cursors a stride of B apart, the advance not timed), on the
    # whole table and on its first 2^k + 1 rows — the table size with the longest cycle walk, two passes on average
    cursors = [torch.tensor([i * B], dtype=torch.int64, device=DEV) for i in range(LAUNCHES)]
    Nw = (1 << ((N - 1).bit_length() - 1)) + 1

    def launches(which):
        for rng, cur in zip(rngs, cursors):
            if which == "gather":
                ops.data_gather(tab, x, rng=rng)
            elif which == "gather_epoch":
                ops.data_gather_epoch(tab, x, rng, cur)
            elif which == "gather_epoch_worst":
                ops.data_gather_epoch(tab[:Nw], x, rng, cur)
            elif which == "prep":
                L.check(L.lib().msgm_ssm_prep(x.data_ptr(), y.data_ptr(), t.data_ptr(), v.data_ptr(), B, d, st, rng.ptr(),
                                              ctr.data_ptr(), L.stream()), "msgm_ssm_prep")
            else:
                ops.ssm_prep_gather(tab, x, y, t, v, st, rng, ctr)
    graphs = {}
    others = ("gather_epoch", "gather_epoch_worst", "prep", "prep_gather")
    for which in ("gather",) + others:                                     # LAUNCHES kernel nodes: no host launch rate in the figure
        launches(which)
        torch.cuda.synchronize()
        graphs[which] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[which]):
            launches(which)
    call = lambda which: graphs[which].replay()
    row = per_launch(timed_rounds(call, "gather", [(w, w) for w in others], rounds, reps, warm))
    g, p, f = row["parent_median_us"], row["builds"]["prep"]["median_us"], row["builds"]["prep_gather"]["median_us"]
    ge, gw = row["builds"]["gather_epoch"], row["builds"]["gather_epoch_worst"]
    model = 8.0 * B * d
    row.update(B=B, d=d, N=N, worst_case_rows=Nw, launches_per_timed_call=LAUNCHES, gather_model_bytes=model,
               gather_effective_GBps=round(model / (g * 1e-6) / 1e9, 1), gather_plus_prep_us=round(g + p, 3),
               fused_minus_two_launches_us=round(f - (g + p), 3),
               note="a timed call replays a hipGraph of LAUNCHES kernel nodes, each at its own stream offset")
    say(f"{B:6d} x {d:5d} from {N:8d} rows: gather {g:7.2f} us (vs itself {row['parent_vs_parent_max_us']:.2f}; model "
        f"{model / 1e6:.2f} MB -> {row['gather_effective_GBps']:.0f} GB/s) | prep {p:7.2f} us | fused prep+gather {f:7.2f} us "
        f"(gather + prep {g + p:7.2f} us)")
    say(f"{'':33s} epoch gather {ge['median_us']:7.2f} us ({ge['minus_parent_us']:+.2f} us against the gather, {ge['verdict']}) | "
        f"from {Nw} rows (2^k + 1) {gw['median_us']:7.2f} us ({gw['minus_parent_us']:+.2f} us, {gw['verdict']})")
    return row


def trainers(which, rounds, reps, warm):
    from sdeflow_light_amd.data import gaussian_mixture_2d, random_images
    tr, host = {}, {}
    for name in ("fixed", "data", "unfused", "epoch", "host"):
        torch.manual_seed(0)
        if which == "c2_mlp":
            B, d, N = bench.B_C2, 2, 10 ** 5
            tab = gaussian_mixture_2d(N, seed=1234, device=DEV)
            mk = lambda **kw: MLPScoreTrainer(bench.build_mlp(DEV), B, lr=1e-3, seed=1, **kw)
        else:
            B, d, N = 32, 12288, 2000
            tab = random_images(N, seed=1234, device=DEV)
            mk = lambda **kw: UNetScoreTrainer(bench.build_unet("c4", DEV)[0], B, d, lr=1e-4, world=1, seed=1, **kw)
        t = tr[name] = (mk(data=ArrayData(tab)) if name in ("data", "unfused") else
                        mk(data=ArrayData(tab, replace=False)) if name == "epoch" else mk())
        if name == "unfused":
            t._table = None                                    # the sampler's own launch ahead of the unchanged prep
        if name in ("fixed", "host"):
            t.set_data(tab[:B])
        if name == "host":
            host["np"] = tab.cpu().numpy()
        t.step()                                               # warm-up step + capture

    def call(name):
        if name == "host":
            a = host["np"]
            idx = np.random.randint(0, a.shape[0], size=B)
            tr[name].set_data(torch.from_numpy(a[idx, :]).to(torch.float32).to(DEV))
        tr[name].step()
    row = timed_rounds(call, "fixed", [(w, w) for w in ("data", "unfused", "epoch", "host")], rounds, reps, warm)
    row.update(trainer=which, B=B, d=d, table_rows=N,
               graph_kernel_nodes={r: ops.graph_node_kinds(t.graph).get("kernel") for r, t in tr.items()})
    b = row["builds"]
    row["fused_minus_unfused_us"] = round(b["data"]["median_us"] - b["unfused"]["median_us"], 2)
    row["epoch_minus_data_us"] = round(b["epoch"]["median_us"] - b["data"]["median_us"], 2)
    say(f"trainer {which}: fixed batch {row['parent_median_us']:10.1f} us (vs itself {row['parent_vs_parent_max_us']:.1f}) | " +
        " | ".join(f"{k} {v['minus_parent_us']:+9.1f} us ({v['percent']:+.2f} %) {v['verdict']}" for k, v in b.items()) +
        f" | kernel nodes {row['graph_kernel_nodes']}")
    tr.clear()
    torch.cuda.empty_cache()
    return row


def main():
    out = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    rounds, reps, warm = (1, 3, 1) if QUICK else (3, 7, 2)
    res = dict(device=torch.cuda.get_device_name(0), rounds=rounds, reps=reps, warmup=warm, dropped_warmup_rounds=1,
               unit="microseconds per launch (kernels) / per captured step (trainers); verdicts against the first variant's own spread",
               kernels=[kernels(B, d, N, rounds, reps, warm) for B, d, N in SHAPES],
               trainer=[trainers(w, rounds, 5 if not QUICK else 3, 1) for w in ("c2_mlp", "c4_unet2d_b32")])
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.splitext(out)[0] + ".txt", "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
