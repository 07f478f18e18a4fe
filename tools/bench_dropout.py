#!/usr/bin/env python3
"""GPU box: dropout in the 2-D U-Net (ResBlock out_layers) at the C4 shapes.
  1. the GroupNorm+SiLU kernels of out_layers with and without the DROP build: dual forward (k_gn_fwd_reduce + k_gn_fwd_apply)
     and dual backward (k_gn_bwd_reduce + k_gn_bwd_apply + the slot reduction) at Bp = 32 and 256;
  2. the C4 training step (VorticityUNet 64x64x3, SGM, SSM + Adam, captured hipGraph) at B = 256 and at the 32-row shard;
  3. one train-mode EM sampler step (GraphedStepSampler, 4096 rows),
at p = 0 and p = 0.1.
    python tools/bench_dropout.py [--skip-net]"""
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sdeflow_light_amd import _lib as L, ops  # noqa: E402

dev = torch.device("cuda:0")
PS = (0.0, 0.1)


def timeit(fn, it=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(it)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)[it // 2] * 1e-3


def kernels():
    rng = L.PhiloxState(1, dev)
    for Bp in (32, 256):
        for P, C in ((4096, 32), (1024, 64), (256, 128)):
            G = 32
            torch.manual_seed(0)
            x = torch.randn(2 * Bp * P * C, device=dev)
            gout = torch.randn_like(x)
            gx = torch.empty_like(x)
            gam, bet = torch.ones(C, device=dev), torch.zeros(C, device=dev)
            dga, dbe = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
            st = torch.empty(Bp * G * 4, device=dev)
            out = torch.empty_like(x)
            row = []
            for drop in (None, ops.dropout_desc(rng, 0, 0.1)):
                tf = timeit(lambda: ops.groupnorm_dual_forward(x, gam, bet, Bp, P, C, G, True, True, stats=st, out=out, dropout=drop))

                def bwd():
                    with ops.DeferredReduces.on(dev):
                        ops.groupnorm_dual_backward(x, gam, bet, st, gout, dga, dbe, Bp, P, C, G, True, gx=gx, dropout=drop)
                tb = timeit(bwd)
                row.append((tf, tb))
            mb = x.numel() * 4 / 1e6
            (f0, b0), (f1, b1) = row
            print(f"Bp={Bp:3d} P={P:4d} C={C:3d} ({mb:6.1f} MB dual input): fwd {f0 * 1e6:7.1f} -> {f1 * 1e6:7.1f} us "
                  f"({f1 / f0:5.3f}x) | bwd {b0 * 1e6:7.1f} -> {b1 * 1e6:7.1f} us ({b1 / b0:5.3f}x)", flush=True)
            del x, gout, gx, out


def build(p):
    from sdeflow_light_amd.NNUnet import VorticityUNet
    from sdeflow_light_amd.SDEs import SGMsde, PluginReverseSDE
    torch.manual_seed(0)
    net = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, in_space=64, attention_resolutions=(2, 4),
                        flatten_order="F", channels=3, dropout=p).to(dev)
    with torch.no_grad():                                   # as bench.py: no zero-initialised layer
        for q in net.parameters():
            if q.dim() > 1 and float(q.abs().sum()) == 0.0:
                q.normal_(0, 0.02)
    T = torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)
    sde = SGMsde(beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=T, num_steps_forward=16, device=dev)
    return PluginReverseSDE(sde, net, T, vtype="rademacher", deviceReverseSDE=dev).to(dev), 3 * 64 * 64


def net_steps():
    from sdeflow_light_amd.train import UNetScoreTrainer
    from sdeflow_light_amd.sde_scheme import GraphedStepSampler
    for p in PS:
        res = {}
        for B in (256, 32):
            gen, d = build(p)
            tr = UNetScoreTrainer(gen, B, d, lr=1e-4, seed=1)
            tr.set_data(torch.randn(B, d, device=dev))
            for _ in range(3):
                tr.step()
            torch.cuda.synchronize()
            n = 10 if B == 256 else 30
            t0 = time.perf_counter()
            for _ in range(n):
                tr.step()
            torch.cuda.synchronize()
            res[B] = (time.perf_counter() - t0) / n * 1e3
            assert math.isfinite(float(tr.loss))
            del tr, gen
        gen, d = build(p)
        rows, N = 4096, 8
        gs = GraphedStepSampler(gen, rows, d, N)
        x = gen.latent_sample(rows, d)
        gs.run(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = gs.run(x)
        torch.cuda.synchronize()
        em = (time.perf_counter() - t0) / N * 1e3
        # the route that was timed: with dropout the net's stream moved once per score call (warm-up + 2 x N replays) and
        # every ResBlock's out_layers went through the materialised dropout GroupNorm instead of conv2's folded staging
        net = gen.a
        if p > 0:
            assert net.dropout_rng.state_dict()["offset"] == 1 + 2 * N, net.dropout_rng.state_dict()
        calls, real = [], ops.groupnorm_dual_forward
        ops.groupnorm_dual_forward = lambda *a, **k: (calls.append(k.get("dropout") is not None), real(*a, **k))[1]
        try:
            with torch.no_grad():
                net(x, torch.full((rows,), 0.5, device=dev))
        finally:
            ops.groupnorm_dual_forward = real
        print(f"dropout={p}: C4 train step B=256 {res[256]:7.2f} ms | B=32 shard {res[32]:6.2f} ms | "
              f"train-mode EM sampler step (4096 rows) {em:6.2f} ms | finite {bool(torch.isfinite(y).all())} | "
              f"one sampler forward: {sum(calls)} dropout GroupNorm launches, {len(calls) - sum(calls)} plain", flush=True)
        del gs, gen


if __name__ == "__main__":
    kernels()
    if "--skip-net" not in sys.argv:
        net_steps()
