#!/usr/bin/env python3
"""Per-call kernel times of one tools/bench_mlp_wide.py run under rocprofv3 (--rounds 1): reads the kernel trace CSV and
assigns the k_mlp* dispatches, in order, to the tool's (d, premodule) cases — 1 + iters dispatches per call, the calls
in the order training pass, forward, EM loop.  The first dispatch of every call is the warm-up and is left out.
    python tools/mlp_wide_trace_table.py TRACE.csv OUT.csv [--dims 16,30,32,64,128] [--iters 5]"""
import argparse, csv, statistics

ap = argparse.ArgumentParser()
ap.add_argument("trace"); ap.add_argument("out")
ap.add_argument("--dims", default="16,30,32,64,128"); ap.add_argument("--iters", type=int, default=5)
a = ap.parse_args()
rows = sorted((r for r in csv.DictReader(open(a.trace)) if "k_mlp" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
cases = [(int(d), p) for d in a.dims.split(",") for p in (False, True)]
per = 1 + a.iters
assert len(rows) == 3 * per * len(cases), (len(rows), 3 * per * len(cases))
out = []
for i, (d, p) in enumerate(cases):
    for j, call in enumerate(("msgm_mlp_ssm_partial", "msgm_mlp_forward", "msgm_mlp_em_loop (16 steps)")):
        ks = rows[(3 * i + j) * per:(3 * i + j + 1) * per]
        assert len({k["Kernel_Name"] for k in ks}) == 1
        us = [(int(k["End_Timestamp"]) - int(k["Start_Timestamp"])) / 1e3 for k in ks[1:]]
        out.append(dict(d=d, premodule=p, call=call, kernel=ks[0]["Kernel_Name"], lds_bytes=ks[0].get("LDS_Block_Size", ""),
                        scratch_bytes=ks[0].get("Scratch_Size", ""), dispatches=len(us), mean_us=round(statistics.mean(us), 2),
                        min_us=round(min(us), 2), max_us=round(max(us), 2)))
with open(a.out, "w", newline="") as f:
    w = csv.DictWriter(f, fieldnames=list(out[0])); w.writeheader(); w.writerows(out)
for o in out:
    print(o["d"], o["premodule"], o["call"], o["kernel"], o["mean_us"])
