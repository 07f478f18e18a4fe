#!/usr/bin/env python3
"""Time the one-launch forward perturbation of the multiplicative SDE against the composed route it replaces:
    python tools/time_forward_perturb.py [out.json] [--quick]
The composed route is the parent's code, kept as sde_scheme.msgm_forward_perturb_composed, so it is the yardstick:
parent_compare.timed_rounds alternates (composed, composed again, kernel) and the verdict of the kernel route is taken
against the largest composed-vs-composed difference of a round.

  (a) the perturbation alone, Philox noise, as the trainers and SDE.sample_scheme call it (host launches included: the
      composed route is 6 nsf + 9 launches and an eager call pays for each)
  (b) the hipGraph-captured trainer step on both routes: MLPScoreTrainer d = 6 at B = 4096, UNetScoreTrainer on UNet1D
      d = 1024 at B = 4096 and on the C4 net (VorticityUNet 64 x 64 x 3) at B = 256, the last two configured as bench.py's
      leg_msgm; both trainers of a pair hold the same data and the same seeds
  (c) the kernel's effective HBM rate: only the 8 B per element it must move (x0 in, y out) over the kernel's own time,
      taken from 20 launches queued behind each other through the C ABI
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
ALONE = [("sparse", 4096, 1024, 16), ("sparse", 256, 12288, 16), ("sparse", 32, 12288, 16), ("sparse", 4096, 6, 16),
         ("sparse", 4096, 6, 100), ("dense", 4096, 16, 16)]


def Tp():
    return torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)


def base_for(kind, n, nsf, y0=None):
    y0 = torch.randn(1024, n) if y0 is None else y0
    return MSGMsde(y0, beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=Tp(), num_steps_forward=nsf, device=DEV,
                   denseTensor=(kind == "dense"), norm_map="log").to(DEV)


def line(tag, row):
    b = row["builds"]["kernel"]
    print(f"{tag:<44} composed {row['parent_median_us']:10.1f} us (vs itself {row['parent_vs_parent_max_us']:7.1f}) | kernel "
          f"{b['median_us']:10.1f} us ({b['percent']:+.1f} %) {b['verdict']}", flush=True)


def back_to_back(base, x0, t, reps=20):
    """Microseconds per msgm_forward_perturb launch when `reps` of them are queued behind each other through the C ABI on one
    output buffer (Philox noise, no allocation, no stream advance): the kernel's own time, launch latency hidden by the queue."""
    nsf = base.num_steps_forward
    ts, delta = SS._forward_grid(base, nsf, x0.device)
    y, st, lib, B, n = torch.empty_like(x0), base.struct(), L.lib(), x0.shape[0], x0.shape[1]

    def launch():
        L.check(lib.msgm_forward_perturb(L.ptr(x0), L.ptr(t), L.ptr(y), None, B, n, st, nsf, L.ptr(ts), float(delta), float(delta ** 0.5),
                                         float(delta * 0.5), float(delta * 1.0), None, None, base.rng.ptr(), L.stream()), "msgm_forward_perturb")
    for _ in range(3):
        launch()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        launch()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def alone(kind, B, n, nsf, rounds, reps, warm):
    torch.manual_seed(0)
    base = base_for(kind, n, nsf)
    base.rng = L.PhiloxState(7, DEV)
    x0 = torch.randn(B, n, device=DEV) * 1.5
    t = (torch.rand(B, device=DEV)).clamp(min=1e-3)          # uniform times as sample_t draws them
    route = {"composed": SS.msgm_forward_perturb_composed, "kernel": SS.msgm_forward_perturb}
    s0 = base.rng.state.clone()
    ref = route["composed"](base, t, x0)
    base.rng.state.copy_(s0)
    same = bool(torch.equal(route["kernel"](base, t, x0), ref))
    row = timed_rounds(lambda r: route[r](base, t, x0), "composed", [("kernel", "kernel")], rounds, reps, warm)
    kus = back_to_back(base, x0, t.reshape(-1).contiguous())
    row.update(kind=kind, B=B, n=n, nsf=nsf, bitwise_equal=same, launches_composed=6 * nsf + 9,
               kernel_back_to_back_us=round(kus, 2), kernel_effective_hbm_GBps=round(8.0 * B * n / (kus * 1e-6) / 1e9, 1))
    line(f"alone {kind} B={B} n={n} nsf={nsf}", row)
    print(f"      kernel alone, 20 launches queued: {kus:.1f} us each = {row['kernel_effective_hbm_GBps']} GB/s of the 8 B/element", flush=True)
    return row


def trainer_pair(which):
    """(kernel-route trainer, composed-route trainer): the composed one is captured with forward_perturb_supported off."""
    from sdeflow_light_amd.train import MLPScoreTrainer, UNetScoreTrainer
    from sdeflow_light_amd.data import signals_1d, random_images
    pair = []
    for composed in (False, True):
        torch.manual_seed(0)
        if which == "mlp_d6":
            from sdeflow_light_amd.NN import MLP
            B, d, nsf = 4096, 6, 16
            net, x = MLP(d, premodule="NormalizeLogRadius").to(DEV), torch.randn(B, d, device=DEV) * 1.5
        elif which == "unet1d_d1024":
            from sdeflow_light_amd.NNUnet1D import UNet1D
            B, d, nsf = 4096, 1024, 16
            net = UNet1D(input_dim=d, base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, emb_dim=128,
                         premodule="NormalizeLogRadius").to(DEV)
            x = signals_1d(B, seed=1234, device=DEV)
        else:
            from sdeflow_light_amd.NNUnet import VorticityUNet
            B, d, nsf = 256, 3 * 64 * 64, 16
            net = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, in_space=64,
                                attention_resolutions=(2, 4), flatten_order="F", channels=3, premodule="NormalizeLogRadius").to(DEV)
            with torch.no_grad():
                for p_ in net.parameters():
                    if p_.dim() > 1 and float(p_.abs().sum()) == 0.0:
                        p_.normal_(0, 0.02)
            x = random_images(B, seed=1234, device=DEV)
        T = Tp()
        base = MSGMsde(x[:1024].cpu(), beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=T, num_steps_forward=nsf, device=DEV,
                       denseTensor=False, norm_map="log")
        gen = PluginReverseSDE(base, net, T, vtype="rademacher", deviceReverseSDE=DEV).to(DEV)
        tr = MLPScoreTrainer(gen, B, lr=1e-4, seed=1) if which == "mlp_d6" else UNetScoreTrainer(gen, B, d, lr=1e-4, world=1, seed=1)
        tr.set_data(x)
        real = ops.forward_perturb_supported
        if composed:
            ops.forward_perturb_supported = lambda kind, n: False
        try:
            first = float(tr.step())                          # warm-up step + capture
        finally:
            ops.forward_perturb_supported = real
        pair.append((tr, first))
    return pair, B, d, nsf


def trainer(which, rounds, reps, warm):
    ((tk, fk), (tc, fc)), B, d, nsf = trainer_pair(which)
    tr = {"kernel": tk, "composed": tc}
    row = timed_rounds(lambda r: tr[r].step(), "composed", [("kernel", "kernel")], rounds, reps, warm)
    row.update(trainer=which, B=B, d=d, nsf=nsf, first_loss_equal=(fk == fc),
               graph_kernel_nodes={r: ops.graph_node_kinds(tr[r].graph).get("kernel") for r in tr})
    line(f"trainer {which} B={B}", row)
    del tk, tc, tr
    torch.cuda.empty_cache()
    return row


def main():
    out = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    rounds, reps, warm = (1, 3, 1) if QUICK else (3, 7, 2)
    res = dict(device=torch.cuda.get_device_name(0), rounds=rounds, reps=reps, warmup=warm, dropped_warmup_rounds=1,
               unit="microseconds; verdict of the kernel route against the composed route's own spread", alone=[], trainer=[])
    for kind, B, n, nsf in ALONE:
        res["alone"].append(alone(kind, B, n, nsf, rounds, reps, warm))
    for which in ("mlp_d6", "unet1d_d1024", "unet2d_d12288"):
        res["trainer"].append(trainer(which, rounds, 3 if QUICK else 5, 1))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
