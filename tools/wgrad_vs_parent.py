#!/usr/bin/env python3
"""GPU box: the Winograd 3x3 weight gradient (k_wgrad_wino) of this tree's library against another build of it (the parent
commit's libmsgm_hip.so, built into a scratch path), both loaded into one process, as tools/conv_vs_parent.py does for the
forward kernels:
    python tools/wgrad_vs_parent.py <parent.so> [B]                          bitwise: slabs, dW and dbias, torch.equal
    python tools/wgrad_vs_parent.py <parent.so> [B] --time [name=variant.so ...]
                                                                             timing: parent / parent again / this tree (/ further
                                                                             builds, e.g. a rejected form), alternated
The cases are every distinct 3x3 stride-1 wgrad call of one eager C4 training step at batch B (default 256; recorded as
tools/bench_wgrad3x3.py records them) and the shapes of tests/test_wgrad_wino_paths_gpu.py.  Bitwise goes through the raw ABI
(msgm_conv_wgrad_det with a workspace of its own, NaN-filled first, so the slabs can be compared and a skipped store shows)
and through ops.conv_wgrad under DeferredReduces; timing goes through ops.conv_wgrad (slot reduction included)."""
import ctypes, importlib.util, os, statistics, sys, time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sdeflow_light_amd import _lib, ops  # noqa: E402

DEV = "cuda"
args = [a for a in sys.argv[1:] if a != "--time"]
TIME = "--time" in sys.argv
VARIANTS = [a.split("=", 1) for a in args if "=" in a]
args = [a for a in args if "=" not in a]
B = int(args[1]) if len(args) > 1 else 256


def load(path):
    h = ctypes.CDLL(path)
    for name, (res, at) in _lib.SIGNATURES.items():
        fn = getattr(h, name)
        fn.restype, fn.argtypes = res, at
    return h


NEW = _lib.lib()
PARENT = load(os.path.abspath(args[0]))


def use(h):
    _lib._lib = h                       # ops.* resolves the library through _lib.lib()


def step_calls():
    """(N, Hi, Wi, Ho, Wo, ups, C, koff, Cout, CoutP, Ktot, has_bias, n_bias) -> launches per step, of the calls routed to wino."""
    from sdeflow_light_amd.NNUnet import VorticityUNet
    from sdeflow_light_amd.SDEs import SGMsde, PluginReverseSDE
    from sdeflow_light_amd.train import UNetScoreTrainer
    from sdeflow_light_amd.data import random_images
    dev = torch.device(DEV)
    torch.manual_seed(0)
    net = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, in_space=64, attention_resolutions=(2, 4),
                        flatten_order="F", channels=3).to(dev)
    T = torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)
    gen = PluginReverseSDE(SGMsde(T=T, num_steps_forward=16, device=dev), net, T, deviceReverseSDE=dev).to(dev)
    tr = UNetScoreTrainer(gen, B, 3 * 64 * 64, lr=1e-4, use_graph=False)
    tr.set_data(random_images(B, 3, 64, 64, device=dev))
    seen, orig = {}, ops.conv_wgrad

    def spy(geom, gy, src, C, koff, dWp, Cout, CoutP, Ktot, dbias=None, n_bias=0, tapmask_c32=None, tapmask_co32=None, wino=False):
        if wino and geom.KH == 3 and geom.KW == 3 and geom.strideH == 1 and geom.strideW == 1 and C % 4 == 0 and Cout % 4 == 0:
            key = (geom.N, geom.Hi, geom.Wi, geom.Ho, geom.Wo, geom.ups, C, koff, Cout, CoutP, Ktot, dbias is not None, n_bias)
            seen[key] = seen.get(key, 0) + 1
        return orig(geom, gy, src, C, koff, dWp, Cout, CoutP, Ktot, dbias=dbias, n_bias=n_bias, tapmask_c32=tapmask_c32,
                    tapmask_co32=tapmask_co32, wino=wino)

    ops.conv_wgrad = spy
    tr.step()
    torch.cuda.synchronize()
    ops.conv_wgrad = orig
    del tr, gen, net
    torch.cuda.empty_cache()
    return sorted(seen.items(), key=lambda kv: (-kv[0][3], kv[0][6], kv[0][8], kv[0][7]))


def test_calls():
    spec = importlib.util.spec_from_file_location("paths", os.path.join(ROOT, "tests", "test_wgrad_wino_paths_gpu.py"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    out = []
    for (N, nb, H, W, ups, srcC, Cout) in m.CASES:
        Hi, Wi = (H // 2, W // 2) if ups else (H, W)
        Ktot, koff = ops.pad16(sum(srcC)), 0
        for s, C in enumerate(srcC):
            out.append(((N, Hi, Wi, H, W, int(ups), C, koff, Cout, ops.pad16(Cout), Ktot, s == 0, nb if s == 0 else 0), 1))
            koff += C
    return out


class Case:
    def __init__(self, key, cnt, seed):
        (self.N, self.Hi, self.Wi, self.Ho, self.Wo, self.ups, self.C, self.koff, self.Cout, self.CoutP, self.Ktot, self.has_b,
         self.nb) = key
        self.cnt = cnt
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.geom = ops.conv_geom(self.N, self.Hi, self.Wi, self.Ho, self.Wo, 3, 3, 1, 1, 0, self.ups)
        self.gy = torch.randn(self.N * self.Ho * self.Wo * self.Cout, device=DEV, generator=g)
        self.x = torch.randn(self.N * self.Hi * self.Wi * self.C, device=DEV, generator=g)
        self.base = torch.randn(9 * self.CoutP * self.Ktot, device=DEV, generator=g)
        self.db0 = torch.randn(self.Cout, device=DEV, generator=g) if self.has_b else None
        self.desc = (f"N={self.N} {self.Hi}x{self.Wi}->{self.Ho}x{self.Wo} ups={self.ups} C={self.C} koff={self.koff} Cout={self.Cout}/"
                     f"{self.CoutP} Ktot={self.Ktot} bias={int(self.has_b)} n_bias={self.nb} x{cnt}")

    def raw(self, h):
        """msgm_conv_wgrad_det on a NaN-filled workspace: (slabs, dW, dbias)."""
        L = _lib
        nbias = self.nb if self.has_b else 0
        need = int(h.msgm_conv_wgrad_workspace(self.geom, self.C, self.Cout, self.CoutP, nbias, 1))
        ws = torch.full((need // 4,), float("nan"), device=DEV)
        dWp, db = self.base.clone(), (self.db0.clone() if self.has_b else None)
        rc = h.msgm_conv_wgrad_det(self.geom, L.ptr(self.gy), L.ptr(self.x), self.C, self.koff, L.ptr(dWp), self.Cout, self.CoutP,
                                   self.Ktot, L.ptr(db), nbias, None, None, L.ptr(ws), ws.numel() * 4, 1, L.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return ws, dWp, db

    def via_ops(self, h, deferred, dWp=None, db=None):
        use(h)
        if dWp is None:
            dWp, db = self.base.clone(), (self.db0.clone() if self.has_b else None)
        call = lambda: ops.conv_wgrad(self.geom, self.gy, self.x, self.C, self.koff, dWp, self.Cout, self.CoutP, self.Ktot,  # noqa: E731
                                      dbias=db, n_bias=self.nb if self.has_b else 0, wino=True)
        if deferred:
            with ops.DeferredReduces.on(DEV):
                call()
        else:
            call()
        return dWp, db


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    # slabs: every slot either kernel writes is finite; NaN marks what neither wrote, and must sit at the same places
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def bitwise(cases):
    t0, bad = time.time(), 0
    for c in cases:
        sp, wp, bp = c.raw(PARENT)
        sn, wn, bn = c.raw(NEW)
        ok = same(sp, sn) and torch.equal(wp, wn) and bool(torch.isfinite(wn).all()) and (bp is None or torch.equal(bp, bn))
        what = [] if ok else [n for n, a, b in (("slabs", sp, sn), ("dW", wp, wn), ("dbias", bp, bn)) if not same(a, b)]
        wdp, bdp = c.via_ops(PARENT, True)
        wdn, bdn = c.via_ops(NEW, True)
        torch.cuda.synchronize()
        okd = torch.equal(wdp, wdn) and torch.equal(wdn, wn) and (bdp is None or (torch.equal(bdp, bdn) and torch.equal(bdn, bn)))
        if not okd:
            what.append("deferred reduction")
        bad += not (ok and okd)
        print(f"{'equal' if ok and okd else 'DIFFERENT ' + ' '.join(what):<9} {c.desc}", flush=True)
    print(f"cases run {len(cases)}, bit-identical to the parent (slabs, dW, dbias; per-call and deferred reduction) {len(cases) - bad}, "
          f"different {bad} ({time.time() - t0:.0f} s)")
    return bad


def timing(cases):
    """Per case: ROUNDS + 1 rounds of (parent, parent again, this tree, then every variant), each the median of REPS event-timed
    calls after WARM untimed ones; round 0 is dropped.  pp = the largest |parent - parent again| of one round."""
    ROUNDS, REPS, WARM = 5, 20, 3
    builds = [("new", NEW)] + [(n, load(os.path.abspath(f))) for n, f in VARIANTS]
    tot = {n: 0.0 for n, _ in builds}
    totp = 0.0
    for c in cases:
        dWp, db = c.base.clone(), (c.db0.clone() if c.has_b else None)

        def med(h):
            for _ in range(WARM):
                c.via_ops(h, False, dWp, db)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
            for a, b in ev:
                a.record(); c.via_ops(h, False, dWp, db); b.record()
            torch.cuda.synchronize()
            return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3
        p1, p2, t = [], [], {n: [] for n, _ in builds}
        for r in range(ROUNDS + 1):
            x1, x2 = med(PARENT), med(PARENT)
            xs = [med(h) for _, h in builds]
            if r:
                p1.append(x1); p2.append(x2)
                for (n, _), x in zip(builds, xs):
                    t[n].append(x)
        mp = statistics.median(p1 + p2)
        pp = max(abs(a - b) for a, b in zip(p1, p2))
        fl = 2.0 * 9 * c.N * c.Ho * c.Wo * c.C * c.Cout
        line = f"{c.desc:<86} parent {mp:7.1f} us {fl / mp / 1e6:6.1f} TFLOP/s as written (pp {pp:4.1f})"
        totp += c.cnt * mp
        for n, _ in builds:
            x = statistics.median(t[n])
            tot[n] += c.cnt * x
            line += f" | {n} {x:7.1f} us {fl / x / 1e6:6.1f} ({100 * (x - mp) / mp:+.1f} %)"
        print(line, flush=True)
    print(f"per step (launches x median): parent {totp / 1e3:.2f} ms" + "".join(f", {n} {v / 1e3:.2f} ms" for n, v in tot.items()))
    return 0


if __name__ == "__main__":
    step = [Case(k, n, 100 + i) for i, (k, n) in enumerate(step_calls())]
    print(f"{len(step)} distinct Winograd 3x3 wgrad calls, {sum(c.cnt for c in step)} per step (dual batch {2 * B})", flush=True)
    if TIME:
        sys.exit(timing(step))
    small = [Case(k, n, 900 + i) for i, (k, n) in enumerate(test_calls())]
    sys.exit(1 if bitwise(step + small) else 0)
