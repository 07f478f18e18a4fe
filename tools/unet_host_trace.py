"""Host-side trace of the U-Net pipelines (NNUnet.py, NNUnet1D.py): which C-ABI calls a pass makes, in which order and with
which arguments, and the bits it computes.  Run on two trees with the same library, the two JSON files are byte-identical
exactly when the Python that schedules the kernels did not change what it launches.

    python tools/unet_host_trace.py OUT.json [--coverage REPORT.txt] [--calls CALLS.txt]

ops.lib is replaced by a recording proxy around the real library.  Per call: the entry name, the scalar arguments, the scalar
fields of struct arguments (in declaration order), for every pointer only whether it is null, and the integer result.
OUT.json holds, per pass, the SHA-256 of that call sequence, the number of calls per entry and bit digests
(tests/test_layer_census_gpu.py:digest) of the output, the per-sample losses and the flat gradient bucket; --calls writes
the calls themselves, one per line, for a diff when two hashes differ.  One trainer configuration adds ops.graph_node_kinds of
its captured step, which also counts torch's own cat / zero / copy launches.

--coverage runs everything under the stdlib ``trace`` module and writes the statements of the pass functions (FUNCS below) that
no configuration executed, ``raise`` statements aside; an empty report means the configurations reach every branch.  Some
branches are reachable only the way the tests reach them, so four more runs carry the tests' monkeypatches (see PATCHED); one of
them, a two-source block whose conv2 cannot fold, needs a patch of its own: no network built from 16-multiple channel counts
gives conv1's twin and conv2 different answers."""
import ast
import ctypes
import hashlib
import inspect
import json
import os
import sys
import textwrap
import trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from oracle.det_params import load_init_like_  # noqa: E402
from sdeflow_light_amd import _lib, ops  # noqa: E402
from sdeflow_light_amd.convnet import ConvOp  # noqa: E402
from sdeflow_light_amd.NNUnet import VorticityUNet  # noqa: E402
from sdeflow_light_amd.NNUnet1D import UNet1D  # noqa: E402
from test_layer_census_gpu import digest  # noqa: E402

DEV = "cuda"
B = 3
FUNCS = {VorticityUNet: ("_res_fwd", "_attn_fwd", "_run", "_backward", "_attn_bwd", "_attn_bwd_composed", "_gn_fold"),
         UNet1D: ("_run", "_backward")}


# ------------------------------------------------------------------------------------------------ the recording proxy
def _fields(s):
    """A struct as the list of its fields' values in declaration order (pointers as below, an all-zero array as 0)."""
    out = []
    for name, ftype in s._fields_:
        v = getattr(s, name)
        if ftype is ctypes.c_void_p:
            out.append("p" if v else None)
        elif isinstance(v, ctypes.Array):
            out.append(list(v) if any(v) else 0)
        else:
            out.append(v)
    return out


def _arg(argtype, a):
    """What the trace keeps of one argument: scalars as they are, a pointer as "p" or null, a struct as its fields."""
    if argtype is ctypes.c_void_p:
        return list(a) if isinstance(a, ctypes.Array) else "p" if a else None      # a host array (tap masks): its values
    if isinstance(argtype, type) and issubclass(argtype, ctypes._Pointer):
        if a is None:
            return None
        obj = getattr(a, "_obj", a)                                   # byref(x) keeps x as _obj
        if isinstance(obj, ctypes._Pointer):
            obj = obj.contents if obj else None
        if isinstance(obj, ctypes.Structure):
            return _fields(obj)
        if isinstance(obj, ctypes.Array):
            return [_fields(e) if isinstance(e, ctypes.Structure) else e for e in obj]
        return "p"
    return int(a) if isinstance(a, bool) else a


class Proxy:
    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn, argtypes = getattr(self.real, name), _lib.SIGNATURES[name][1]

        def call(*args):
            rec = [name] + [_arg(t, a) for t, a in zip(argtypes, args)]
            ret = fn(*args)
            self.calls.append(rec + [ret if isinstance(ret, int) else None])          # last: the integer result
            return ret
        return call

    def take(self):
        calls, self.calls = self.calls, []
        return calls


# ------------------------------------------------------------------------------------------------ configurations
def unet2d(mults, S, channels, heads, pre, p):
    return dict(kind="2d", base_channels=32, channel_mults=mults, num_res_blocks=1, in_space=S, attention_resolutions=(2, 4),
                channels=channels, num_heads=heads, premodule=pre, dropout=p, flatten_order="F")


NLR = "NormalizeLogRadius"
CONFIGS = [
    ("2d_m12_s16", unet2d((1, 2), 16, 1, 1, None, 0.0)),
    ("2d_m124_s16_rgb_h2_nlr_drop", unet2d((1, 2, 4), 16, 3, 2, NLR, 0.3)),       # 4x4 level: no fold, composed attention
    ("2d_m12_s32_h2_drop", unet2d((1, 2), 32, 1, 2, None, 0.3)),
    ("2d_m124_s32_rgb_nlr", unet2d((1, 2, 4), 32, 3, 1, NLR, 0.0)),
    ("1d_l64_nlr", dict(kind="1d", input_dim=64, base_channels=16, channel_mults=(1, 2), emb_dim=32, premodule=NLR)),
    ("1d_l50", dict(kind="1d", input_dim=50, base_channels=16, channel_mults=(1, 2), emb_dim=32, premodule=None)),   # 25 -> 12 -> 24: padded
]
# (name, configuration, patch): branches the tests reach by monkeypatching
PATCHED = [
    ("2d_m124_s32_rgb_nlr/no_input_transform", CONFIGS[3][1], "no_transform"),          # every GroupNorm a pass of its own
    ("2d_m12_s32_h2_drop/two_source_transform_only", CONFIGS[2][1], "two_source_only"),  # two-source block, conv2 cannot fold
    ("2d_m12_s16/decoder_concatenates", CONFIGS[0][1], "no_set2t"),                      # training through cat([h, skip])
    ("2d_m12_s16/no_fused_attention", CONFIGS[0][1], "no_fused_attention"),              # composed attention at T = 64
]


def make_net(cfg):
    cfg = dict(cfg)
    kind = cfg.pop("kind")
    torch.manual_seed(0)                                  # the net's own dropout stream is seeded from torch's seed
    net = VorticityUNet(**cfg) if kind == "2d" else UNet1D(**cfg)
    load_init_like_(net)
    d = cfg["channels"] * cfg["in_space"] ** 2 if kind == "2d" else cfg["input_dim"]
    return net.to(DEV), d


def apply_patch(mp, patch, net):
    if patch == "no_transform":
        mp.setattr(ConvOp, "can_transform_input", lambda self, N, Hi, Wi: False)
    elif patch == "two_source_only":
        mp.setattr(ConvOp, "can_transform_input", lambda self, N, Hi, Wi: len(self.srcC) == 2)
    elif patch == "no_set2t":
        mp.setitem(net._build(), "set2t", None)
    elif patch == "no_fused_attention":
        for name in ("attention_supported", "attention_mh_supported", "attention_dual_supported", "attention_dual_mh_supported"):
            mp.setattr(ops, name, lambda *a: False)


class Patches:
    """The two operations of pytest's MonkeyPatch this tool needs, undone in reverse order."""

    def __init__(self):
        self.undo_list = []

    def setattr(self, obj, name, value):
        self.undo_list.append((setattr, obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def setitem(self, d, key, value):
        self.undo_list.append((lambda dd, k, v: dd.__setitem__(k, v), d, key, d[key]))
        d[key] = value

    def undo(self):
        for fn, obj, name, old in reversed(self.undo_list):
            fn(obj, name, old)
        self.undo_list = []


def run_config(name, cfg, proxy, patch=None):
    net, d = make_net(cfg)
    g = torch.Generator().manual_seed(7)
    x, v, u = (torch.randn(B, d, generator=g).to(DEV) for _ in range(3))
    t, cst = (torch.rand(B, generator=g) * 0.9 + 0.05).to(DEV), torch.randn(B, generator=g).to(DEV)
    mp = Patches()
    passes = []
    try:
        if patch is not None:
            proxy.take()
            apply_patch(mp, patch, net)
            passes.append({"config": name, "pass": "build (before the patch)", "calls": proxy.take()})
        for mode, train in (("forward, eval mode", False), ("forward, train mode", True), ("ssm_grad", True)):
            net.train(train)
            if mode == "ssm_grad":
                per = net.ssm_grad(x, t, v, u, cst, 1.0 / B)
                out = {"per_sample_loss": digest(per), "grad_bucket": digest(net.flat_parameters()[1])}
            else:
                out = {"output": digest(net(x, t))}
            torch.cuda.synchronize()
            passes.append({"config": name, "pass": mode, "digests": out, "calls": proxy.take()})
    finally:
        mp.undo()
    return passes


def run_trainer(proxy):
    """One captured training step (2-D U-Net with dropout under the additive SDE): what the graph holds and what it computes."""
    from sdeflow_light_amd.SDEs import PluginReverseSDE, SGMsde
    from sdeflow_light_amd.train import UNetScoreTrainer
    net, d = make_net(unet2d((1, 2), 16, 1, 1, None, 0.3))
    T = torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)
    base = SGMsde(beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=T, num_steps_forward=16, device=DEV)
    gen = PluginReverseSDE(base, net, T, deviceReverseSDE=DEV).to(DEV)
    tr = UNetScoreTrainer(gen, 8, d, lr=1e-3, use_graph=True, seed=5)
    tr.set_data(torch.randn(8, d, generator=torch.Generator().manual_seed(3)).to(DEV))
    losses = [float(tr.step()) for _ in range(3)]
    torch.cuda.synchronize()
    return {"config": "trainer 2d_m12_s16_drop, B = 8, captured", "pass": "3 steps", "graph_node_kinds": ops.graph_node_kinds(tr.graph),
            "digests": {"losses": [x.hex() for x in losses], "parameters": digest(net.flat_parameters()[0])}, "calls": proxy.take()}


def run_all():
    proxy = Proxy(_lib.lib())
    ops.lib = lambda: proxy                                # every ops.* wrapper resolves the library through this name
    passes = []
    for name, cfg in CONFIGS:
        passes += run_config(name, cfg, proxy)
    for name, cfg, patch in PATCHED:
        passes += run_config(name, cfg, proxy, patch)
    passes.append(run_trainer(proxy))
    return passes


# ------------------------------------------------------------------------------------------------ coverage
def statements(fn):
    """{line: source} of the first line of every statement in fn, docstrings and ``raise`` statements aside."""
    src, first = inspect.getsourcelines(fn)
    path = inspect.getsourcefile(fn)
    tree = ast.parse(textwrap.dedent("".join(src)))
    out = {}
    for node in ast.walk(tree):
        if not isinstance(node, ast.stmt) or isinstance(node, ast.Raise):
            continue
        if isinstance(node, ast.Expr) and isinstance(node.value, ast.Constant) and isinstance(node.value.value, str):
            continue
        if isinstance(node, ast.FunctionDef) and node.lineno == 1:
            continue                                       # the function's own def line
        out[first + node.lineno - 1] = src[node.lineno - 1].rstrip()
    return path, out


def uncovered(counts):
    lines = []
    for cls, names in FUNCS.items():
        for name in names:
            if not hasattr(cls, name):
                continue
            path, stmts = statements(getattr(cls, name))
            hit = {ln for (f, ln), n in counts.items() if n and os.path.realpath(f) == os.path.realpath(path)}
            lines += [f"{os.path.relpath(path, ROOT)}:{ln}: {cls.__name__}.{name}: {text.strip()}" for ln, text in sorted(stmts.items())
                      if ln not in hit]
    return lines


def main():
    out = sys.argv[1]
    cov = sys.argv[sys.argv.index("--coverage") + 1] if "--coverage" in sys.argv else None
    if cov:
        tracer = trace.Trace(count=1, trace=0, ignoredirs=[sys.prefix, sys.exec_prefix],
                             ignoremods=["ops", "convnet", "_lib", "train", "SDEs", "NN", "optim", "parallel", "det_params", "layer_ref",
                                        "test_layer_census_gpu"])
        passes = tracer.runfunc(run_all)
        counts = {k: v for k, v in tracer.results().counts.items() if k[0].endswith(("NNUnet.py", "NNUnet1D.py"))}
        report = uncovered(counts)
        with open(cov, "w") as f:
            f.write("".join(line + "\n" for line in report))
        print(f"{len(report)} statements of the pass functions were not executed -> {cov}")
    else:
        passes = run_all()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    listing = [[json.dumps(c, separators=(",", ":")) for c in p.pop("calls")] for p in passes]
    for p, calls in zip(passes, listing):                   # OUT.json: one line per pass, the call sequence as its SHA-256
        names = [json.loads(c)[0] for c in calls]
        p.update(n_calls=len(calls), calls_sha256=hashlib.sha256("\n".join(calls).encode()).hexdigest(),
                 entries={n: names.count(n) for n in sorted(set(names))})
    with open(out, "w") as f:
        f.write('{"passes": [\n' + ",\n".join(json.dumps(p, sort_keys=True) for p in passes) + "\n]}\n")
    if "--calls" in sys.argv:                               # the calls themselves, one per line: diff two of these
        with open(sys.argv[sys.argv.index("--calls") + 1], "w") as f:
            for p, calls in zip(passes, listing):
                f.write(f"# {p['config']}: {p['pass']}\n" + "".join(c + "\n" for c in calls))
    print(f"{len(passes)} passes, {sum(p['n_calls'] for p in passes)} calls -> {out}")


if __name__ == "__main__":
    main()
