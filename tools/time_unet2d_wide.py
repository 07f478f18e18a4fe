#!/usr/bin/env python3
"""Time what the GroupNorm kernels' C <= 1024 range opened, in one process and one build:
    python tools/time_unet2d_wide.py [out.json] [--quick]          (out.txt is written next to out.json)

  (a) the GroupNorm entries at C = 256, 512, 1024 (pixel lanes PL = 4, 2, 1), P = 256 and 1024, Bp = 32 (dual: 64 rows):
      effective GB/s = the bytes the launches must move / the median time of one call inside a replayed hipGraph of LAUNCHES
      calls.  forward reduce: groupnorm_affine (k_gn_fwd_reduce over the Bp primal rows + the per-channel finalise; reads x
      once); forward: k_gn_fwd_reduce + k_gn_fwd_apply, dual, SiLU (x read twice, out written once); backward:
      k_gn_bwd_reduce + k_gn_bwd_apply in the slots form (x and the cotangent read twice, the input cotangent written once).
  (b) W64 (base 64, (1, 2, 4)) and D4 (32, (1, 2, 4, 8)) at in_space 64, B = 32: the captured UNetScoreTrainer step and one
      captured Euler-Maruyama sampler step, and the share of the step's kernel time per kernel family from one eager step
      under torch.profiler — among them the composed attention chain (k_bmm* + k_softmax_dual*) that the single-head
      blocks at head width 256 run.
Reported, not gated: the parent commit refuses every one of these shapes."""
import json, os, statistics, sys, time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sdeflow_light_amd import ops  # noqa: E402
from sdeflow_light_amd.NNUnet import VorticityUNet  # noqa: E402

DEV = torch.device("cuda", 0)
QUICK = "--quick" in sys.argv
LAUNCHES = 20
LINES = []
NETS = {"W64": (64, (1, 2, 4)), "D4": (32, (1, 2, 4, 8))}
FAMILIES = (("composed attention (k_bmm, k_softmax_dual)", ("k_bmm", "k_softmax_dual")), ("fused attention", ("k_attn",)),
            ("GroupNorm", ("k_gn_",)), ("weight gradients", ("wgrad",)), ("slot reductions", ("slot_reduce",)),
            ("convolutions", ("conv", "wino")))


def say(line):
    print(line, flush=True)
    LINES.append(line)


def median_us(call, reps, warm):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts), min(ts), max(ts)


def graphed(fn):
    fn()
    torch.cuda.synchronize()
    g = ops.new_graph()
    with torch.cuda.graph(g):
        for _ in range(LAUNCHES):
            fn()
    return g


def groupnorm(reps, warm):
    rows, Bp, G = [], 32, 32
    for P in (256, 1024):
        for C in (256, 512, 1024):
            torch.manual_seed(C + P)
            n = 2 * Bp * P * C
            x, gout = torch.randn(n, device=DEV) * 1.5 + 0.3, torch.randn(n, device=DEV)
            gamma, beta = 1 + 0.2 * torch.randn(C, device=DEV), 0.2 * torch.randn(C, device=DEV)
            out, gx, stats = torch.empty_like(x), torch.empty_like(x), torch.empty(Bp * G * 4, device=DEV)
            dga, dbe = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
            ops.groupnorm_dual_forward(x, gamma, beta, Bp, P, C, G, True, True, stats=stats, out=out)

            def bwd():
                with ops.DeferredReduces.on(DEV):
                    ops.groupnorm_dual_backward(x, gamma, beta, stats, gout, dga, dbe, Bp, P, C, G, True, gx=gx)
            tensor = 4.0 * n                                   # bytes of the dual tensor
            work = (("forward reduce (affine, primal rows)", lambda: ops.groupnorm_affine(x[: n // 2], C, gamma, beta, Bp, P, G), tensor / 2),
                    ("forward reduce + apply", lambda: ops.groupnorm_dual_forward(x, gamma, beta, Bp, P, C, G, True, True, stats=stats, out=out),
                     3 * tensor),
                    ("backward reduce + apply (slots)", bwd, 5 * tensor))
            for name, fn, nbytes in work:
                g = graphed(fn)
                med, lo, hi = median_us(g.replay, reps, warm)
                med, lo, hi = med / LAUNCHES, lo / LAUNCHES, hi / LAUNCHES
                gbs = nbytes / (med * 1e-6) / 1e9
                rows.append(dict(entry=name, C=C, P=P, Bp=Bp, pixel_lanes=256 // (C // 4), us=round(med, 2), us_min=round(lo, 2),
                                 us_max=round(hi, 2), bytes=nbytes, GBps=round(gbs, 1)))
                say(f"GroupNorm {name:38s} C={C:4d} (PL={256 // (C // 4)}) P={P:4d} Bp={Bp}: {med:8.2f} us [{lo:.2f}, {hi:.2f}]  "
                    f"{nbytes / 2**20:7.1f} MiB  {gbs:7.1f} GB/s")
                del g
            torch.cuda.empty_cache()
    return rows


def make_gen(tag, S):
    from sdeflow_light_amd.SDEs import SGMsde, PluginReverseSDE
    base, mults = NETS[tag]
    torch.manual_seed(0)
    net = VorticityUNet(base_channels=base, channel_mults=mults, num_res_blocks=2, premodule=None, in_space=S,
                        attention_resolutions=(2, 4), flatten_order="F").to(DEV)
    with torch.no_grad():        # non-zero "zero-init" layers so every kernel does real work
        for prm in net.parameters():
            if float(prm.abs().sum()) == 0.0:
                prm.normal_(0.0, 0.02)
    Tp = torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)
    return PluginReverseSDE(SGMsde(T=Tp, num_steps_forward=16, device=DEV), net, Tp, deviceReverseSDE=DEV).to(DEV)


def shares(step):
    """Share of the kernel time of one eager call of `step` per kernel family (torch.profiler), or None if it cannot trace."""
    try:
        from torch.profiler import ProfilerActivity, profile
        step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        per = {}
        for ev in prof.key_averages():
            t = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0))
            if t > 0:
                per[ev.key] = per.get(ev.key, 0.0) + t
    except Exception as e:                                   # noqa: BLE001
        say(f"  kernel shares: profiler unavailable ({type(e).__name__}: {e})")
        return None
    total = sum(per.values())
    if total <= 0:
        say("  kernel shares: the profiler recorded no kernel time")
        return None
    fam = {}
    for k, t in per.items():
        name = next((f for f, keys in FAMILIES if any(s in k for s in keys)), "other")
        fam[name] = fam.get(name, 0.0) + t
    top = sorted(per.items(), key=lambda kv: -kv[1])[:8]
    return dict(total_us=round(total, 1), families={k: round(100 * v / total, 2) for k, v in sorted(fam.items(), key=lambda kv: -kv[1])},
                top_kernels=[(k[:90], round(100 * t / total, 2)) for k, t in top])


def networks(reps, warm):
    from sdeflow_light_amd.train import UNetScoreTrainer
    from sdeflow_light_amd.sde_scheme import GraphedStepSampler
    S, B = 64, 32
    d, rows = S * S, {}
    for tag in NETS:
        tr = UNetScoreTrainer(make_gen(tag, S), B, d, lr=1e-4, seed=1, use_graph=True)
        torch.manual_seed(1)
        tr.set_data(torch.randn(B, d, device=DEV))
        tr.step(); tr.step()                                      # eager step, then the capture
        med, lo, hi = median_us(tr.step, reps, warm)
        say(f"{tag} {S}x{S} B={B} captured train step: {med / 1e3:8.2f} ms [{lo / 1e3:.2f}, {hi / 1e3:.2f}]  kernel nodes "
            f"{ops.graph_node_kinds(tr.graph).get('kernel')}")
        te = UNetScoreTrainer(make_gen(tag, S), B, d, lr=1e-4, seed=1, use_graph=False)
        te.set_data(torch.randn(B, d, device=DEV))
        sh_t = shares(te.step)
        del tr, te
        torch.cuda.empty_cache()
        sm = GraphedStepSampler(make_gen(tag, S), B, d, 16, method="em")
        sm.run(torch.randn(B, d, device=DEV))
        med_s, lo_s, hi_s = median_us(sm.graph.replay, reps, warm)
        say(f"{tag} {S}x{S} B={B} captured EM sampler step: {med_s / 1e3:8.2f} ms [{lo_s / 1e3:.2f}, {hi_s / 1e3:.2f}]  kernel nodes "
            f"{ops.graph_node_kinds(sm.graph).get('kernel')}")
        net, x, t = sm.sde.a, torch.randn(B, d, device=DEV), torch.full((B,), 0.5, device=DEV)
        net.eval()
        sh_s = shares(lambda: net(x, t))
        for what, sh in (("train step", sh_t), ("sampler score call", sh_s)):
            if sh:
                say(f"  {tag} {what} kernel time {sh['total_us'] / 1e3:.2f} ms, shares: " + ", ".join(f"{k} {v:.1f} %" for k, v in sh["families"].items()))
        rows[tag] = dict(train_step_ms=round(med / 1e3, 3), train_step_range_ms=[round(lo / 1e3, 3), round(hi / 1e3, 3)],
                         sampler_step_ms=round(med_s / 1e3, 3), sampler_step_range_ms=[round(lo_s / 1e3, 3), round(hi_s / 1e3, 3)],
                         train_step_shares=sh_t, sampler_call_shares=sh_s)
        del sm, net
        torch.cuda.empty_cache()
    return rows


def main():
    out = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    reps, warm = (3, 1) if QUICK else (15, 3)
    res = dict(device=torch.cuda.get_device_name(0), reps=reps, warmup=warm, launches_per_timed_groupnorm_call=LAUNCHES,
               groupnorm=groupnorm(reps, warm), networks=networks(reps, warm))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.splitext(out)[0] + ".txt", "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
