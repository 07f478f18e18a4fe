#!/usr/bin/env python3
"""Time the one-launch T = 16 attention kernels (csrc/attention_small_kernels.hip) against the composed
bmm / softmax chain they replace, in one process and one build:
    python tools/time_attn_small.py [out.json] [--quick]          (out.txt is written next to out.json)
Alternated rounds, medians, the composed route against itself as the yardstick (parent_compare.timed_rounds: "holds" means
the difference is inside that spread and nothing is claimed).

  (a) per attention block at T = 16, (heads, D) = (1,128), (2,64), (4,32), Bp = 32, 128, 1024: sampler forward, dual forward
      and dual backward, the new entry against the chain of NNUnet._attn_fwd / _attn_bwd_composed.  One timed call replays a
      hipGraph of LAUNCHES block calls and the figures are divided by it, so the host's launch rate is not what is timed.
  (b) the driver's 16x16 U-Net (base 32, mults (1,2,4), attention at 8x8 and 4x4; six of its eleven attention blocks are
      T = 16): the captured UNetScoreTrainer step (SGM, B = 128) and one captured GraphedStepSampler Euler-Maruyama step at
      1024 rows.  The composed route is the same build with ops.attention_small_supported patched to False while the
      model is built and its step captured — how the tests switch routes.
"""
import json, math, os, sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from parent_compare import timed_rounds  # noqa: E402
from sdeflow_light_amd import ops  # noqa: E402
from sdeflow_light_amd.NNUnet import VorticityUNet  # noqa: E402

DEV = torch.device("cuda", 0)
QUICK = "--quick" in sys.argv
LAUNCHES = 20
T = 16
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def composed_forward(qkv, N, Bp, nh, D, dual):
    """NNUnet._attn_fwd's composed chain on a given qkv: (att, P, Wd, Pd)."""
    C, s2 = nh * D, 1.0 / math.sqrt(D)
    ld = 3 * C
    nb = Bp if dual else N                                     # batch of the chain: the sampler has no tangent half
    half, btt = Bp * T * ld, nb * T * T
    S = torch.empty(nh * btt, device=DEV)
    sq, sk, sS = (T * ld, ld, 1), (T * ld, 1, ld), (T * T, T, 1)
    for h in range(nh):
        ops.bmm(qkv, 3 * D * h, qkv, 3 * D * h + D, S, h * btt, T, T, D, nb, sq, sk, sS, alpha=s2)
    Wd = Pd = None
    if dual:
        Wd, Pd = torch.empty_like(S), torch.empty_like(S)
        for h in range(nh):
            qo, ko = 3 * D * h, 3 * D * h + D
            ops.bmm(qkv, half + qo, qkv, ko, Wd, h * btt, T, T, D, nb, sq, sk, sS, alpha=s2, pair2=(qkv, qo, qkv, half + ko))
    ops.softmax_dual_forward(S, T, Wd, Pd)
    att = torch.empty(N * T * C, device=DEV)
    sP, sv, sa = (T * T, T, 1), (T * ld, ld, 1), (T * C, C, 1)
    for h in range(nh):
        vo, ao = 3 * D * h + 2 * D, D * h
        if dual:
            ops.bmm(S, h * btt, qkv, half + vo, att, Bp * T * C + ao, T, D, T, nb, sP, sv, sa, pair2=(Pd, h * btt, qkv, vo),
                    third=(qkv, vo, att, ao))
        else:
            ops.bmm(S, h * btt, qkv, vo, att, ao, T, D, T, nb, sP, sv, sa)
    return att, S, Wd, Pd


def per_launch(row):
    def div(x):
        return [round(v / LAUNCHES, 3) for v in x] if isinstance(x, list) else round(x / LAUNCHES, 3)
    for k in ("parent_us", "parent_again_us", "parent_median_us", "parent_vs_parent_max_us"):
        row[k] = div(row[k])
    for b in row["builds"].values():
        for k in ("us", "median_us", "minus_parent_us"):
            b[k] = div(b[k])
    return row


def block(nh, D, Bp, rounds, reps, warm):
    C, N, s2 = nh * D, 2 * Bp, 1.0 / math.sqrt(D)
    torch.manual_seed(nh + D + Bp)
    qkv = torch.randn(N * T * 3 * C, device=DEV) * 1.2
    datt = torch.randn(N * T * C, device=DEV)
    out = torch.empty(N * T * C, device=DEV)
    _, P, Wd, Pd = composed_forward(qkv, N, Bp, nh, D, True)
    rec = SimpleNamespace(qkv=qkv, P=P, Wd=Wd, Pd=Pd, H=4, W=4, a=SimpleNamespace(c=C, nh=nh, d=D))
    work = {("sampler", "composed"): lambda: composed_forward(qkv, N, Bp, nh, D, False),
            ("sampler", "small"): lambda: ops.attention_small_forward(qkv, out, N, T, nh, D, s2),
            ("dual_fwd", "composed"): lambda: composed_forward(qkv, N, Bp, nh, D, True),
            ("dual_fwd", "small"): lambda: ops.attention_small_dual_forward(qkv, Bp, T, nh, D, s2),
            ("dual_bwd", "composed"): lambda: VorticityUNet._attn_bwd_composed(None, rec, datt, N, Bp),
            ("dual_bwd", "small"): lambda: ops.attention_small_dual_backward(qkv, datt, Bp, T, nh, D, s2)}
    rows = {}
    for what in ("sampler", "dual_fwd", "dual_bwd"):
        graphs = {}
        for route in ("composed", "small"):                    # LAUNCHES block calls per replay
            fn = work[(what, route)]
            fn()
            torch.cuda.synchronize()
            graphs[route] = ops.new_graph()
            with torch.cuda.graph(graphs[route]):
                for _ in range(LAUNCHES):
                    fn()
        row = per_launch(timed_rounds(lambda r: graphs[r].replay(), "composed", [("small", "small")], rounds, reps, warm))
        row.update(what=what, heads=nh, D=D, Bp=Bp, launches_per_timed_call=LAUNCHES,
                   kernel_nodes_per_block={r: ops.graph_node_kinds(g).get("kernel", 0) // LAUNCHES for r, g in graphs.items()})
        b = row["builds"]["small"]
        say(f"block heads={nh} D={D:3d} Bp={Bp:4d} {what:8s}: composed {row['parent_median_us']:8.2f} us "
            f"(vs itself {row['parent_vs_parent_max_us']:.2f}) | small {b['median_us']:8.2f} us ({b['percent']:+.1f} %) {b['verdict']}"
            f" | launches {row['kernel_nodes_per_block']}")
        rows[what] = row
    return rows


def driver_net():
    from sdeflow_light_amd.SDEs import SGMsde, PluginReverseSDE
    torch.manual_seed(0)
    net = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, premodule=None, in_space=16,
                        attention_resolutions=(2, 4), flatten_order="F").to(DEV)
    Tp = torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)
    return PluginReverseSDE(SGMsde(T=Tp, num_steps_forward=16, device=DEV), net, Tp, deviceReverseSDE=DEV).to(DEV)


def network(rounds, reps, warm):
    from sdeflow_light_amd.train import UNetScoreTrainer
    from sdeflow_light_amd.sde_scheme import GraphedStepSampler
    real = ops.attention_small_supported
    tr, sm = {}, {}
    for route in ("composed", "small"):
        ops.attention_small_supported = real if route == "small" else (lambda T_, h, D: False)
        try:
            t = tr[route] = UNetScoreTrainer(driver_net(), 128, 256, lr=1e-4, seed=1, use_graph=True)
            torch.manual_seed(1)
            t.set_data(torch.randn(128, 256, device=DEV))
            t.step(); t.step()                                      # eager step, then the capture
            s = sm[route] = GraphedStepSampler(driver_net(), 1024, 256, 16, method="em")
            s.run(torch.randn(1024, 256, device=DEV))
        finally:
            ops.attention_small_supported = real
    rows = {}
    for name, call, objs in (("train step B=128", lambda r: tr[r].step(), tr), ("EM step 1024 rows", lambda r: sm[r].graph.replay(), sm)):
        row = timed_rounds(call, "composed", [("small", "small")], rounds, reps, warm)
        row["graph_kernel_nodes"] = {r: ops.graph_node_kinds(o.graph).get("kernel") for r, o in objs.items()}
        b = row["builds"]["small"]
        say(f"16x16 U-Net {name}: composed {row['parent_median_us']:9.1f} us (vs itself {row['parent_vs_parent_max_us']:.1f}) | "
            f"small {b['median_us']:9.1f} us ({b['minus_parent_us']:+.1f} us, {b['percent']:+.2f} %) {b['verdict']} | kernel nodes "
            f"{row['graph_kernel_nodes']}")
        rows[name] = row
    return rows


def main():
    out = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    rounds, reps, warm = (1, 3, 1) if QUICK else (3, 7, 2)
    res = dict(device=torch.cuda.get_device_name(0), rounds=rounds, reps=reps, warmup=warm, dropped_warmup_rounds=1,
               unit="microseconds per block call (a) / per captured step (b); verdicts against the composed route's own spread",
               blocks=[block(nh, D, Bp, rounds, reps, warm) for nh, D in ((1, 128), (2, 64), (4, 32)) for Bp in (32, 128, 1024)],
               network=network(rounds, reps, warm))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.splitext(out)[0] + ".txt", "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
