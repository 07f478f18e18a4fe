#!/usr/bin/env python3
"""GPU box: the fused MLP kernels across the width classes (narrow d <= 15, wide d <= 30, extra-wide 31 <= d <= 128),
premodule off / on, at B = 65 536.  Times msgm_mlp_ssm_partial (the training pass), msgm_mlp_forward and
msgm_mlp_em_loop (16 steps in one launch), with the shapes alternated round by round in one process, and reports the
algorithmic rate: forward = 2*128*(in_dim + 128 + 128 + d) FLOP per sample, a training pass = 6 x forward
(bench.py / SURVEY App. A).  Writes one JSON line per (d, premodule) and, with --out FILE, the list as JSON."""
import argparse, ctypes as C, json, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdeflow_light_amd import ops
from sdeflow_light_amd.NN import MLP
from sdeflow_light_amd.SDEs import SGMsde

ap = argparse.ArgumentParser()
ap.add_argument("--dims", default="16,30,32,64,128")
ap.add_argument("--B", type=int, default=65536)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--em-steps", type=int, default=16)
ap.add_argument("--out", default="")
a = ap.parse_args()
dev = "cuda"
B = a.B
torch.manual_seed(0)
T = torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)
st = SGMsde(beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=T, num_steps_forward=16, device=dev).struct()
lib, stream = ops.lib(), ops.stream()


def timeit(fn):
    fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for s, e in ev:
        s.record(); fn(); e.record()
    torch.cuda.synchronize()
    return sum(s.elapsed_time(e) for s, e in ev) / a.iters * 1e-3


cases = []
for d in [int(x) for x in a.dims.split(",")]:
    for pre in (False, True):
        net = MLP(d, premodule="NormalizeLogRadius" if pre else None).to(dev)
        P = net.kernel_params()
        y, v = torch.randn(B, d, device=dev), torch.randn(B, d, device=dev).sign()
        t = torch.rand(B, device=dev) * 0.99 + 0.01
        x = torch.randn(B, d, device=dev)
        out = torch.empty(B, d, device=dev)
        ws = ops.mlp_ssm_workspace(d, pre, dev)
        nsl = C.c_int32(0)
        ts = (torch.linspace(0, 1, a.em_steps + 1) * 0.999).to(dev)
        rng = torch.zeros(2, dtype=torch.int64, device=dev)
        in_dim = d + 1 + int(pre)
        flop_fwd = 2.0 * 128 * (in_dim + 128 + 128 + d)

        def train(P=P, y=y, t=t, v=v, ws=ws, nsl=nsl):
            ops.check(lib.msgm_mlp_ssm_partial(P, y.data_ptr(), t.data_ptr(), v.data_ptr(), None, None, B, st, 1.0 / B, None,
                                               ws.data_ptr(), ws.numel() * 4, C.byref(nsl), stream), "msgm_mlp_ssm_partial")

        def fwd(P=P, y=y, t=t, out=out):
            ops.check(lib.msgm_mlp_forward(P, y.data_ptr(), t.data_ptr(), out.data_ptr(), B, stream), "msgm_mlp_forward")

        def em(P=P, x=x, ts=ts, rng=rng):
            ops.check(lib.msgm_mlp_em_loop(P, x.data_ptr(), B, st, ts.data_ptr(), a.em_steps, 1.0 / a.em_steps, 0.0,
                                           rng.data_ptr(), 0, stream), "msgm_mlp_em_loop")
        cases.append(dict(d=d, premodule=pre, in_dim=in_dim, flop_fwd=flop_fwd, fns=(train, fwd, em), t=([], [], [])))

for _ in range(a.rounds):                 # shapes alternated round by round
    for c in cases:
        for k, fn in enumerate(c["fns"]):
            c["t"][k].append(timeit(fn))

res = []
for c in cases:
    tt, tf, te = (statistics.median(x) for x in c["t"])
    r = dict(d=c["d"], premodule=c["premodule"], B=B,
             train_us=tt * 1e6, train_tflops=6 * c["flop_fwd"] * B / tt / 1e12,
             train_spread=(max(c["t"][0]) - min(c["t"][0])) / tt,
             fwd_us=tf * 1e6, fwd_tflops=c["flop_fwd"] * B / tf / 1e12,
             em_loop_us_per_step=te / a.em_steps * 1e6, em_loop_tflops=c["flop_fwd"] * B * a.em_steps / te / 1e12)
    res.append(r)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
