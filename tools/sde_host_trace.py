"""Host-side trace of the integrators (sde_scheme.py): which C-ABI calls a sampler makes, in which order and with which
arguments, and the bits it returns.  Run on two trees with the same library, the two JSON files are byte-identical exactly
when the Python that schedules the kernels did not change what it launches.

    python tools/sde_host_trace.py OUT.json [--calls CALLS.txt]

The recording proxy is the one of tools/unet_host_trace.py (per call: entry, scalars, struct scalars, null-ness of pointers,
integer result); here it also stands in for _lib.lib, which PhiloxState.advance resolves the library through.  OUT.json
holds, per configuration, the SHA-256 of the call sequence, the calls per entry and a bit digest of the returned tensor;
--calls writes the calls themselves for a diff when two hashes differ.  Every configuration: B = 5 rows, 3 steps, an MLP
score net at d = 8 (so both the additive SDE and the sparse multiplicative one run), unless its name says otherwise."""
import hashlib
import itertools
import json
import os
import sys

import torch

from unet_host_trace import Proxy, digest                      # puts the repository root and tests/ on sys.path
from oracle.det_params import load_init_like_  # noqa: E402
from sdeflow_light_amd import _lib, ops, sde_scheme as SS  # noqa: E402
from sdeflow_light_amd.NN import MLP  # noqa: E402
from sdeflow_light_amd.SDEs import MSGMsde, PluginReverseSDE, SGMsde, forward_SDE  # noqa: E402

DEV = "cuda"
B, N, D, NSF = 5, 3, 8, 4
# The graphed samplers stay alive until the process ends.  Each is a reference cycle (its captured body refers to it), so a
# dropped one is freed whenever the collector next runs; inside a later capture that destroys a hipGraph during a
# global-mode stream capture, which the runtime refuses, and the error escapes a destructor: the process aborts.
KEEP = []


def kept(sampler):
    KEEP.append(sampler)
    return sampler


def make_gen(kind):
    torch.manual_seed(11)                                      # the base SDE's Philox state is seeded from torch's seed
    net = MLP(D)
    load_init_like_(net)
    T = torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)
    kw = dict(beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=T, num_steps_forward=NSF, device=DEV)
    if kind == "sgm":
        base = SGMsde(**kw)
    else:
        base = MSGMsde(torch.randn(32, D, generator=torch.Generator().manual_seed(5)), denseTensor=False, **kw)
    return PluginReverseSDE(base, net.to(DEV), T, deviceReverseSDE=DEV).to(DEV)


def inputs(rows):
    g = torch.Generator().manual_seed(3)
    return torch.randn(rows, D, generator=g).to(DEV), torch.randn(N, rows, D, generator=g).to(DEV)


def configurations():
    """(name, function returning the tensor to digest), in a fixed order: the Philox states carry over between them."""
    gens = {k: make_gen(k) for k in ("sgm", "sparse")}
    x0, z = inputs(B)
    samplers = (("em", SS.euler_maruyama_sampler), ("heun", SS.heun_sampler), ("rk4", SS.rk4_stratonovich_sampler))
    keeps = {"all": dict(keep_all_samples=True), "kept": dict(keep_all_samples=False, samplesToKeep=[1, 2, 3, 0, 2], include_t0=True),
             "final": dict(keep_all_samples=False)}
    for (sname, fn), kind, nc, keep, noise, rev in itertools.product(samplers, gens, (False, True), keeps, (True, False), (True, False)):
        gen = gens[kind]
        sde = gen if rev else forward_SDE(gen.base_sde, gen.base_sde.T)
        yield (f"{sname} {kind} {'reverse' if rev else 'forward'} norm_correction={nc} {keep} {'noise=' if noise else 'philox'}",
               lambda: fn(sde, x0, num_steps=N, lmbd=0.25 if rev else 0.0, norm_correction=nc, noise=z if noise else None, **keeps[keep]))
    x33, _ = inputs(33)
    yield "em sgm reverse fused mlp_em_loop B=33", lambda: SS.euler_maruyama_sampler(gens["sgm"], x33, num_steps=N, keep_all_samples=False)
    base = gens["sparse"].base_sde
    t = torch.tensor([0.01, 0.1, 0.3, 0.6, 1.0], device=DEV)   # k_b = trunc(NSF t_b) = 0, 0, 1, 2, 4
    g = torch.Generator().manual_seed(9)
    zm, zs = torch.randn(NSF, B, D, generator=g).to(DEV), torch.randn(B, D, generator=g).to(DEV)
    yield "msgm_forward_perturb noise=", lambda: SS.msgm_forward_perturb(base, t, x0, zm, zs)
    yield "msgm_forward_perturb philox", lambda: SS.msgm_forward_perturb(base, t, x0)
    for method, kind, nc in itertools.product(("em", "heun", "rk4"), gens, (False, True)):
        yield (f"GraphedStepSampler {method} {kind} norm_correction={nc}: warm-up, capture, {N} replays",
               lambda: kept(SS.GraphedStepSampler(gens[kind], B, D, N, lmbd=0.25, norm_correction=nc, method=method)).run(x0).clone())
    for rows, x in ((B, x0), (33, x33)):
        yield (f"GraphedEMSampler B={rows}: warm-up, capture, replay",
               lambda: kept(SS.GraphedEMSampler(gens["sgm"], rows, N, lmbd=0.25)).run(x).clone())


def main():
    out = sys.argv[1]
    proxy = Proxy(_lib.lib())
    ops.lib = _lib.lib = lambda: proxy                         # ops.* and PhiloxState.advance resolve the library through these
    proxy.take()
    passes = []
    for name, fn in configurations():                          # a configuration runs while the generator is suspended at it
        proxy.take()                                           # drop what building the configuration launched
        y = fn()
        torch.cuda.synchronize()
        passes.append({"config": name, "digest": digest(y.float()), "shape": list(y.shape), "calls": proxy.take()})
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    listing = [[json.dumps(c, separators=(",", ":")) for c in p.pop("calls")] for p in passes]
    for p, calls in zip(passes, listing):
        names = [json.loads(c)[0] for c in calls]
        p.update(n_calls=len(calls), calls_sha256=hashlib.sha256("\n".join(calls).encode()).hexdigest(),
                 entries={n: names.count(n) for n in sorted(set(names))})
    with open(out, "w") as f:
        f.write('{"passes": [\n' + ",\n".join(json.dumps(p, sort_keys=True) for p in passes) + "\n]}\n")
    if "--calls" in sys.argv:
        with open(sys.argv[sys.argv.index("--calls") + 1], "w") as f:
            for p, calls in zip(passes, listing):
                f.write(f"# {p['config']}\n" + "".join(c + "\n" for c in calls))
    print(f"{len(passes)} configurations, {sum(p['n_calls'] for p in passes)} calls -> {out}")


if __name__ == "__main__":
    main()
