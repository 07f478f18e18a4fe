#!/usr/bin/env python3
"""GPU box: multi-head attention (AttentionBlock num_heads = H) at the C4 shapes, H in {1, 2, 4}.
  1. fused kernels at the C4 attention blocks (T = 1024, C = 64 and T = 256, C = 128; D = C / H), Bp = 256: sampler forward
     (msgm_attention_mh_forward, 2 products of 2 T^2 D per (sample, head)), dual forward (6) and dual backward (15 executed,
     12 as written upstream) in TFLOP/s — the FLOPs do not change with H;
  2. the C4 training step (VorticityUNet 64x64x3, SGM, SSM + Adam, captured hipGraph) at B = 256 and at the 32-row shard, and
     one EM sampler step (GraphedStepSampler, 4096 rows), at num_heads = 1, 2, 4.
    python tools/bench_attn_heads.py [--skip-net]
    python tools/bench_attn_heads.py --profile H      # 5 C4 steps at B = 256, num_heads = H only (under rocprofv3 --kernel-trace --stats)"""
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sdeflow_light_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
HEADS = (1, 2, 4)


def timeit(fn, it=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(it)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in ev) / it * 1e-3


def kernels(Bp=256):
    for T, C in ((1024, 64), (256, 128)):
        torch.manual_seed(0)
        qkv = torch.randn(2 * Bp * T * 3 * C, device=dev)
        datt = torch.randn(2 * Bp * T * C, device=dev)
        out = torch.empty(2 * Bp * T * C, device=dev)
        for H in HEADS:
            D = C // H
            s2 = 1.0 / math.sqrt(D)
            att, stats = ops.attention_dual_mh_forward(qkv, Bp, T, H, D, s2)
            ops.attention_dual_mh_backward(qkv, att, datt, stats, Bp, T, H, D, s2)
            prod = 2.0 * T * T * C * Bp                   # one T x T x D product over all (sample, head) pairs
            ts = timeit(lambda: ops.attention_mh_forward(qkv, out, 2 * Bp, T, H, D, s2))
            tf = timeit(lambda: ops.attention_dual_mh_forward(qkv, Bp, T, H, D, s2))
            tb = timeit(lambda: ops.attention_dual_mh_backward(qkv, att, datt, stats, Bp, T, H, D, s2))
            print(f"T={T:4d} C={C:3d} H={H} D={D:3d} Bp={Bp}: sampler fwd (N={2 * Bp}) {ts * 1e3:7.3f} ms = "
                  f"{2 * 2 * prod / ts / 1e12:6.1f} TF/s | dual fwd {tf * 1e3:7.3f} ms = {6 * prod / tf / 1e12:6.1f} TF/s | "
                  f"dual bwd {tb * 1e3:7.3f} ms = {15 * prod / tb / 1e12:6.1f} TF/s executed ({12 * prod / tb / 1e12:6.1f} as written)",
                  flush=True)
        del qkv, datt, out


def build(H):
    from sdeflow_light_amd.NNUnet import VorticityUNet
    from sdeflow_light_amd.SDEs import SGMsde, PluginReverseSDE
    torch.manual_seed(0)
    net = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, in_space=64, attention_resolutions=(2, 4),
                        num_heads=H, flatten_order="F", channels=3).to(dev)
    with torch.no_grad():                                   # as bench.py: no zero-initialised layer
        for p in net.parameters():
            if p.dim() > 1 and float(p.abs().sum()) == 0.0:
                p.normal_(0, 0.02)
    T = torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)
    sde = SGMsde(beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=T, num_steps_forward=16, device=dev)
    return PluginReverseSDE(sde, net, T, vtype="rademacher", deviceReverseSDE=dev).to(dev), 3 * 64 * 64


def net_steps():
    from sdeflow_light_amd.train import UNetScoreTrainer
    from sdeflow_light_amd.sde_scheme import GraphedStepSampler
    for H in HEADS:
        res = {}
        for B in (256, 32):
            gen, d = build(H)
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
        gen, d = build(H)
        rows, N = 4096, 8
        gs = GraphedStepSampler(gen, rows, d, N)
        x = gen.latent_sample(rows, d)
        gs.run(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = gs.run(x)
        torch.cuda.synchronize()
        em = (time.perf_counter() - t0) / N * 1e3
        print(f"num_heads={H}: C4 train step B=256 {res[256]:7.2f} ms | B=32 shard {res[32]:6.2f} ms | "
              f"EM sampler step (4096 rows) {em:6.2f} ms | finite {bool(torch.isfinite(y).all())}", flush=True)
        del gs, gen


def profile(H, steps=5):
    from sdeflow_light_amd.train import UNetScoreTrainer
    gen, d = build(H)
    tr = UNetScoreTrainer(gen, 256, d, lr=1e-4, seed=1)
    tr.set_data(torch.randn(256, d, device=dev))
    for _ in range(steps):
        tr.step()
    torch.cuda.synchronize()
    print(f"num_heads={H}: {steps} C4 steps, loss {float(tr.loss):.4f}")


if __name__ == "__main__":
    if "--profile" in sys.argv:
        profile(int(sys.argv[sys.argv.index("--profile") + 1]))
        sys.exit(0)
    kernels()
    if "--skip-net" not in sys.argv:
        net_steps()
