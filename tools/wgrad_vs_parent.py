#!/usr/bin/env python3
"""GPU box: every weight-gradient kernel of this tree's library against another build of it (the parent commit's
libmsgm_hip.so, built into a scratch path), both loaded into one process, as tools/conv_vs_parent.py does for the forward
kernels (the shared parts: tools/parent_compare.py):
    python tools/wgrad_vs_parent.py <parent.so> [B]                          bitwise: slabs, dW and dbias, torch.equal
    python tools/wgrad_vs_parent.py <parent.so> [B] [--only NAME[,NAME]] [--skip NAME[,NAME]] --time [out.json] [name=variant.so ...]
                                                                             timing: parent / parent again / this tree (/ further
                                                                             builds, e.g. a rejected form), alternated; --only keeps
                                                                             the cases whose expected kernel contains a NAME, --skip
                                                                             drops them (e.g. kernels whose machine code is the parent's)
Bitwise cases: every distinct conv_wgrad call of one eager C4 training step at batch B (default 256) and SMALL below — each
kernel at the smallest shapes at which it can go wrong.  Each goes through the raw ABI (msgm_conv_wgrad_det with a workspace
of its own, NaN-filled first, so the slabs can be compared and a skipped store shows) and through ops.conv_wgrad under
DeferredReduces.  Timing (ops.conv_wgrad, slot reduction included): the step's calls and timed_extra() below.  The kernel printed with a case is what this script EXPECTS
wgrad_plan / wgrad_impl to pick (their conditions, restated in expect()), not something observed."""
import ctypes, sys, time

import torch

from parent_compare import load, use, same, test_module, timed_rounds, timing_line, write_timing, timing_args
from sdeflow_light_amd import _lib, ops  # noqa: E402

DEV = "cuda"
TIME = "--time" in sys.argv
args = sys.argv[1:sys.argv.index("--time")] if TIME else sys.argv[1:]
ONLY = args.pop(args.index("--only") + 1).split(",") if "--only" in args else [""]
SKIP = args.pop(args.index("--skip") + 1).split(",") if "--skip" in args else []
args = [a for a in args if a not in ("--only", "--skip")]
B = int(args[1]) if len(args) > 1 else 256
NEW = _lib.lib()
PARENT = load(args[0])


def expect(g, C, Cout, nb, wino, masks):
    taps, two_d, aligned = g.KH * g.KW, g.Ho > 1, C % 4 == 0 and Cout % 4 == 0
    same_ = (g.mode == 0 and g.strideH == 1 and g.strideW == 1 and (g.Hi << g.ups) == g.Ho and (g.Wi << g.ups) == g.Wo and g.KH in (1, 3)
             and g.KW in (1, 3) and g.padH == (g.KH - 1) // 2 and g.padW == (g.KW - 1) // 2)
    if taps == 1 and same_ and not g.ups and (nb * g.Ho * g.Wo) % 16 == 0 and C in (32, 64, 128, 256):
        if Cout == 32 and C <= 128:
            return f"k_wgrad1x1<1,{C // 32},2>"
        if Cout % 64 == 0:
            return f"k_wgrad1x1<{1 if C == 256 else (3 if Cout % 192 == 0 else (2 if Cout % 128 == 0 else 1))},{C // 16},4>"
    if not (same_ and (aligned or (taps == 9 and two_d)) and g.Ho * g.Wo >= 64 and (taps in (1, 3) or (taps == 9 and two_d))
            and (two_d or g.KH == 1)):
        return "k_conv_wgrad<2,4>"
    if two_d and taps == 9:
        if not aligned:
            if not g.ups and not masks and (C, Cout) in ((3, 32), (32, 3)):
                return f"k_wgrad3<{'true' if C == 3 else 'false'}>"
            return "k_wgrad_tile<8,16,9,true>"
        return "k_wgrad_wino" if wino else "k_wgrad_tile9"
    return f"k_wgrad_tile<{'8,16' if two_d else '1,128'},{taps}>"


class Case:
    """One conv_wgrad call: geometry (the 13 fields of msgm_conv_geom_t), channels, place in the packed image, bias gradient,
    tap masks, Winograd preference; the inputs are drawn once from a seeded generator."""

    def __init__(self, geom, C, Cout, koff=0, Ktot=None, CoutP=None, nb=0, wino=False, mc=None, mo=None, cnt=1, seed=0):
        self.geom = g = _lib.ConvGeomT(*geom)
        self.C, self.Cout, self.koff, self.nb, self.wino, self.mc, self.mo, self.cnt = C, Cout, koff, nb, bool(wino), mc, mo, cnt
        self.Ktot, self.CoutP = Ktot or ops.pad16(koff + C), CoutP or ops.pad16(Cout)
        self.taps = g.KH * g.KW
        self.kernel = expect(g, C, Cout, nb, wino, mc or mo)
        gen = torch.Generator(device=DEV).manual_seed(seed)
        self.gy = torch.randn(g.N * g.Ho * g.Wo * Cout, device=DEV, generator=gen)
        self.x = torch.randn(g.N * g.Hi * g.Wi * C, device=DEV, generator=gen)
        self.base = torch.randn(self.taps * self.CoutP * self.Ktot, device=DEV, generator=gen)
        self.db0 = torch.randn(Cout, device=DEV, generator=gen) if nb else None
        self.flops = 2.0 * self.taps * g.N * g.Ho * g.Wo * C * Cout
        self.desc = (f"{self.kernel:<26} N={g.N} {g.Hi}x{g.Wi}->{g.Ho}x{g.Wo} k{g.KH}x{g.KW} s{g.strideW} ups={g.ups} C={C} koff={koff} "
                     f"Cout={Cout}/{self.CoutP} Ktot={self.Ktot} n_bias={nb} masks={mc or mo} wino={int(self.wino)} x{cnt}")

    def fresh(self):
        return self.base.clone(), (self.db0.clone() if self.nb else None)

    def raw(self, h):
        """msgm_conv_wgrad_det on a NaN-filled workspace: (slabs, dW, dbias)."""
        L = _lib
        need = int(h.msgm_conv_wgrad_workspace(self.geom, self.C, self.Cout, self.CoutP, self.nb, int(self.wino)))
        ws = torch.full((need // 4,), float("nan"), device=DEV)
        dWp, db = self.fresh()
        mc = (ctypes.c_uint16 * len(self.mc))(*self.mc) if self.mc else None
        mo = (ctypes.c_uint16 * len(self.mo))(*self.mo) if self.mo else None
        rc = h.msgm_conv_wgrad_det(self.geom, L.ptr(self.gy), L.ptr(self.x), self.C, self.koff, L.ptr(dWp), self.Cout, self.CoutP,
                                   self.Ktot, L.ptr(db), self.nb, mc, mo, L.ptr(ws), ws.numel() * 4, int(self.wino), L.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return ws, dWp, db

    def via_ops(self, h, deferred, dWp=None, db=None):
        use(h)
        if dWp is None:
            dWp, db = self.fresh()
        call = lambda: ops.conv_wgrad(self.geom, self.gy, self.x, self.C, self.koff, dWp, self.Cout, self.CoutP, self.Ktot,  # noqa: E731
                                      dbias=db, n_bias=self.nb, tapmask_c32=self.mc, tapmask_co32=self.mo, wino=self.wino)
        if deferred:
            with ops.DeferredReduces.on(DEV):
                call()
        else:
            call()
        return dWp, db


def geom2d(N, H, W, k=3, ups=0, stride=1):
    """A "same" k x k convolution with H x W output (input at half the size under the folded upsample), or — stride 2 —
    a 3x3 pad-1 convolution of an H x W input."""
    if stride == 2:
        return (N, H, W, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 3, 3, 2, 1, 2, 1, 0, 0)
    p = (k - 1) // 2
    return (N, H >> ups, W >> ups, H, W, k, k, 1, p, 1, p, 0, ups)


def geom1d(N, L, k):
    return (N, 1, L, 1, L, 1, k, 1, 0, 1, (k - 1) // 2, 0, 0)


def step_calls():
    """Every distinct conv_wgrad call of one eager C4 training step at batch B, with its number of launches."""
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
        key = (tuple(getattr(geom, f) for f, _ in geom._fields_), C, Cout, koff, Ktot, CoutP, n_bias if dbias is not None else 0, bool(wino))
        seen[key] = seen.get(key, 0) + 1
        return orig(geom, gy, src, C, koff, dWp, Cout, CoutP, Ktot, dbias=dbias, n_bias=n_bias, tapmask_c32=tapmask_c32,
                    tapmask_co32=tapmask_co32, wino=wino)

    ops.conv_wgrad = spy
    tr.step()
    torch.cuda.synchronize()
    ops.conv_wgrad = orig
    del tr, gen, net
    torch.cuda.empty_cache()
    rows = sorted(seen.items(), key=lambda kv: (-kv[0][0][3], kv[0][0][5], kv[0][1], kv[0][2], kv[0][3]))
    return [Case(k[0], k[1], k[2], koff=k[3], Ktot=k[4], CoutP=k[5], nb=k[6], wino=k[7], cnt=n, seed=100 + i) for i, (k, n) in enumerate(rows)]


def wino_test_rows():
    """The rows of tests/test_wgrad_wino_paths_gpu.py and the 9 x 11 row of tests/test_wgrad_wino_gpu.py, one call per source."""
    rows = list(test_module("test_wgrad_wino_paths_gpu").CASES) + [c for c in test_module("test_wgrad_wino_gpu").CASES if c[2:4] == (9, 11)]
    for (N, nb, H, W, ups, srcC, Cout) in rows:
        koff = 0
        for s, C in enumerate(srcC):
            yield dict(geom=geom2d(N, H, W, ups=int(ups)), C=C, Cout=Cout, koff=koff, Ktot=ops.pad16(sum(srcC)), nb=nb if s == 0 else 0)
            koff += C


# The stride-2 pair op's tap masks as convnet.py builds them (Stride2PairOp: bit t = tap t present, per 32 channels of the paired
# axis): a conv with 32 input channels has [x[2j] | x[2j+1]] = 64 paired inputs, a transposed conv with 32 outputs 64 paired outputs
MASK_CONV, MASK_CONVT = [0b110, 0b011], [0b011, 0b110]


def small_cases():
    rows = [
        # k_conv_wgrad<2, 4>: the stride-2 3x3 of test_conv2d_fwd_bwd; 80 -> 45 channels (partial 64- / 32-channel blocks) over
        # 6 x 48 = 288 positions = chunks of 256 + 32 (position 256 is inside a row of 6); a "same" 3x3 on 6 x 6 = 36 < 64 pixels
        dict(geom=geom2d(2, 16, 12, stride=2), C=32, Cout=32, nb=2),
        dict(geom=geom2d(6, 16, 12, stride=2), C=80, Cout=45, nb=3),
        dict(geom=geom2d(9, 6, 6), C=40, Cout=24, nb=4),
        dict(geom=geom2d(2, 6, 6), C=32, Cout=32, koff=16, Ktot=48),
        # k_wgrad_tile<8, 16, 9, true>: ragged channel counts; 20 x 24 = 3 x 2 ragged tiles; one tile in all; three tiles
        dict(geom=geom2d(2, 20, 24), C=1, Cout=32, nb=1),
        dict(geom=geom2d(2, 20, 24), C=32, Cout=1, nb=1),
        dict(geom=geom2d(2, 16, 16), C=3, Cout=48, nb=2),
        dict(geom=geom2d(2, 20, 24, ups=1), C=1, Cout=32, nb=1),
        dict(geom=geom2d(1, 8, 16), C=1, Cout=32, nb=1),
        dict(geom=geom2d(1, 8, 40), C=32, Cout=1, nb=1),
        # k_wgrad_tile<8, 16, 1>: a 2-D 1x1 the streaming kernel declines (48 input channels); one tile; three tiles
        dict(geom=geom2d(2, 16, 16, k=1), C=48, Cout=32, nb=1),
        dict(geom=geom2d(1, 8, 16, k=1), C=48, Cout=64, nb=1),
        dict(geom=geom2d(3, 8, 16, k=1), C=48, Cout=32, koff=16, Ktot=64),
        # k_wgrad_tile<8, 16, 3>: three vertical taps, through the raw geometry only (ops.conv_geom cannot express it)
        dict(geom=(2, 16, 16, 16, 16, 3, 1, 1, 1, 1, 0, 0, 0), C=32, Cout=32, nb=1),
        dict(geom=(1, 8, 16, 8, 16, 3, 1, 1, 1, 1, 0, 0, 0), C=36, Cout=44, nb=1),
        # k_wgrad_tile<1, 128, 3>: L = 100 (one ragged tile per sample; three tiles, one tile), the pair op's masks, a second source
        # at a K offset; L = 37 < 64 positions falls to k_conv_wgrad
        dict(geom=geom1d(3, 100, 3), C=32, Cout=32, nb=2),
        dict(geom=geom1d(1, 100, 3), C=64, Cout=128, nb=1),
        dict(geom=geom1d(3, 100, 3), C=64, Cout=32, nb=2, mc=MASK_CONV),
        dict(geom=geom1d(2, 100, 3), C=32, Cout=64, nb=1, mo=MASK_CONVT),
        dict(geom=geom1d(2, 300, 3), C=32, Cout=32, koff=32, Ktot=64),
        dict(geom=geom1d(2, 37, 3), C=64, Cout=128, nb=1),
        dict(geom=geom1d(2, 37, 3), C=64, Cout=32, nb=1, mc=MASK_CONV),
        # k_wgrad_tile<1, 128, 1>: 48 input channels (the streaming kernel declines)
        dict(geom=geom1d(3, 100, 1), C=48, Cout=32, nb=2),
        dict(geom=geom1d(1, 100, 1), C=48, Cout=64, koff=16, Ktot=64),
        dict(geom=geom1d(2, 37, 1), C=48, Cout=32, nb=1),
    ]
    # k_wgrad_tile9 (wino = 0) and k_wgrad_wino (wino = 1)
    rows += [dict(r, wino=w) for r in wino_test_rows() for w in (0, 1)]
    # k_wgrad3<true / false>: the shapes of test_wgrad3_parity
    rows += [dict(geom=geom2d(2, H, H), C=C, Cout=Co, nb=1) for H in (16, 24) for (C, Co) in ((3, 32), (32, 3))]
    return [Case(seed=900 + i, **r) for i, r in enumerate(rows)]


def timed_extra():
    """A shape of a size a user would run for every changed kernel that the C4 step does not launch (dual batch 512; the 1-D
    shapes are those of the 1-D U-Net at batch 1024)."""
    rows = [dict(r, wino=0) for r in (dict(geom=geom2d(2 * B, H, H), C=C, Cout=C, nb=B) for H, C in ((64, 32), (32, 64), (16, 128)))]   # k_wgrad_tile9
    rows += [
        dict(geom=geom2d(2 * B, 64, 64), C=1, Cout=32, nb=B),                   # k_wgrad_tile<8,16,9,true>
        dict(geom=geom2d(2 * B, 64, 64), C=32, Cout=1, nb=B),
        dict(geom=geom2d(2 * B, 32, 32, k=1), C=48, Cout=64, nb=B),             # k_wgrad_tile<8,16,1>
        dict(geom=(2 * B, 32, 32, 32, 32, 3, 1, 1, 1, 1, 0, 0, 0), C=64, Cout=64, nb=B),   # k_wgrad_tile<8,16,3>
        dict(geom=geom1d(2048, 512, 3), C=64, Cout=64, nb=1024),                 # k_wgrad_tile<1,128,3>
        dict(geom=geom1d(2048, 256, 3), C=128, Cout=64, nb=1024, mc=[0b110, 0b110, 0b011, 0b011]),
        dict(geom=geom1d(2048, 1024, 1), C=48, Cout=32, nb=1024),                # k_wgrad_tile<1,128,1>
    ]
    return [Case(seed=700 + i, **r) for i, r in enumerate(rows)]


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


def timing(cases, path, variants):
    ROUNDS, REPS, WARM = 5, 20, 3
    rows, tot = [], {}
    for c in cases:
        dWp, db = c.fresh()
        row = timed_rounds(lambda h: c.via_ops(h, False, dWp, db), PARENT, [("new", NEW)] + variants, ROUNDS, REPS, WARM)
        rows.append(dict(kernel=c.kernel, case=c.desc, launches_per_step=c.cnt, **row))
        print(f"{timing_line(c.kernel, row)}   {c.flops / row['parent_median_us'] / 1e6:6.1f} TFLOP/s as written   {c.desc[27:]}", flush=True)
        for n, us in [("parent", row["parent_median_us"])] + [(n, b["median_us"]) for n, b in row["builds"].items()]:
            tot[n] = tot.get(n, 0.0) + c.cnt * us
    print("launches x median over these cases: " + ", ".join(f"{n} {v / 1e3:.2f} ms" for n, v in tot.items()))
    if path:
        write_timing(path, rows, variants, ROUNDS, REPS, WARM)
    return 0


if __name__ == "__main__":
    keep = lambda c: any(n in c.kernel for n in ONLY) and not any(n in c.kernel for n in SKIP)   # noqa: E731
    step = step_calls()
    print(f"{len(step)} distinct conv_wgrad calls, {sum(c.cnt for c in step)} per C4 step (dual batch {2 * B})", flush=True)
    if TIME:
        sys.exit(timing([c for c in step + timed_extra() if keep(c)], *timing_args(sys.argv)))
    sys.exit(1 if bitwise([c for c in step + small_cases() if keep(c)]) else 0)
