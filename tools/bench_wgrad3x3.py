"""3x3 weight gradients of the C4 training step (GPU box): every distinct 3x3 stride-1 wgrad call of one eager step is
recorded (ops.conv_wgrad wrapped), then each is event-timed on the Winograd kernel (k_wgrad_wino) and on the direct one
(k_wgrad_tile9), slot reduction included, as tools/bench_wgrad1x1.py times the 1x1 form.
Usage: python tools/bench_wgrad3x3.py [B]      (dual batch 2B: the forward-mode tangent rides as extra rows)"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdeflow_light_amd import ops
from sdeflow_light_amd.NNUnet import VorticityUNet
from sdeflow_light_amd.SDEs import SGMsde, PluginReverseSDE
from sdeflow_light_amd.train import UNetScoreTrainer
from sdeflow_light_amd.data import random_images

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
dev = torch.device("cuda")
torch.manual_seed(0)
net = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, in_space=64, attention_resolutions=(2, 4),
                    flatten_order="F", channels=3).to(dev)
T = torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)
gen = PluginReverseSDE(SGMsde(T=T, num_steps_forward=16, device=dev), net, T, deviceReverseSDE=dev).to(dev)
tr = UNetScoreTrainer(gen, B, 3 * 64 * 64, lr=1e-4, use_graph=False)
tr.set_data(random_images(B, 3, 64, 64, device=dev))

# --------------------------------------------------------------------------------------------- census of one step
seen = {}
orig = ops.conv_wgrad


def spy(geom, gy, src, C, koff, dWp, Cout, CoutP, Ktot, dbias=None, n_bias=0, tapmask_c32=None, tapmask_co32=None, wino=False):
    if geom.KH == 3 and geom.KW == 3 and geom.strideH == 1 and geom.strideW == 1:
        key = (geom.N, geom.Hi, geom.Wi, geom.Ho, geom.Wo, geom.ups, C, koff, Cout, CoutP, Ktot, dbias is not None, n_bias)
        seen[key] = seen.get(key, (0, wino))[0] + 1, wino
    return orig(geom, gy, src, C, koff, dWp, Cout, CoutP, Ktot, dbias=dbias, n_bias=n_bias, tapmask_c32=tapmask_c32,
                tapmask_co32=tapmask_co32, wino=wino)


ops.conv_wgrad = spy
tr.step()
torch.cuda.synchronize()
ops.conv_wgrad = orig


def timeit(f, reps=20):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


tot = {True: 0.0, False: 0.0}
print(f"{len(seen)} distinct 3x3 wgrad calls, {sum(n for n, _ in seen.values())} per step (dual batch {2 * B})", flush=True)
for key, (cnt, routed) in sorted(seen.items(), key=lambda kv: (-kv[0][3], kv[0][6], kv[0][8])):
    N, Hi, Wi, Ho, Wo, ups, C, koff, Cout, CoutP, Ktot, has_b, nb = key
    geom = ops.conv_geom(N, Hi, Wi, Ho, Wo, 3, 3, 1, 1, 0, ups)
    gy = torch.randn(N * Ho * Wo * Cout, device=dev)
    x = torch.randn(N * Hi * Wi * C, device=dev)
    dWp = torch.zeros(9 * CoutP * Ktot, device=dev)
    db = torch.zeros(Cout, device=dev) if has_b else None
    fl = 2.0 * 9 * N * Ho * Wo * C * Cout                  # as written (direct form)
    us = {}
    for w in (False, True):
        us[w] = timeit(lambda: ops.conv_wgrad(geom, gy, x, C, koff, dWp, Cout, CoutP, Ktot, dbias=db, n_bias=nb, wino=w))
        tot[w] += cnt * us[w]
    print(f"wgrad3x3 {Ho:3d}x{Wo:<3d} ups={ups} C={C:4d} koff={koff:4d} Cout={Cout:4d} x{cnt} (step routes wino={routed}): "
          f"direct {us[False]:8.1f} us {fl / us[False] / 1e6:6.1f} TFLOP/s | wino {us[True]:8.1f} us "
          f"{fl / us[True] / 1e6:6.1f} TFLOP/s as written | x{us[False] / us[True]:.2f}", flush=True)
print(f"per step: direct {tot[False] / 1e3:.2f} ms, wino {tot[True] / 1e3:.2f} ms")
