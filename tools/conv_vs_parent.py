#!/usr/bin/env python3
"""GPU box: the forward / dgrad convolution kernels of this tree's library against another build of it (the parent commit's
libmsgm_hip.so, built into a scratch path), both loaded into one process:
    python tools/conv_vs_parent.py <parent.so>                      bitwise: outputs and channel statistics, torch.equal
    python tools/conv_vs_parent.py <parent.so> --time [out.json] [name=variant.so ...]
                                                                    timing: parent / parent again / this tree (/ further builds,
                                                                    e.g. a form that was tried and rejected), alternated
    python tools/conv_vs_parent.py <parent.so> --only k_conv_wino [--time ...]
                                                                    either mode, only the cases whose kernel name contains the word
Every case runs on the same inputs through the same entry points (SIGNATURES of _lib.py); outputs start NaN-filled (or from
the same random values where the call accumulates), so a skipped store shows.  The cases are chosen to reach
every k_conv_tile form, k_dgrad_s2, k_conv3x3_cout_small, k_conv_wino (register / LDS weights), k_conv_wino_p32 and
k_conv_wino_pipe.  The kernel name printed with a case is what this script EXPECTS conv_route / msgm_conv_forward_wino to pick
for it (their conditions, restated here), not something observed: check it against a kernel trace if the routing changes.
A diagnostic: it swaps the library under ops.* (tools/parent_compare.py, shared with wgrad_vs_parent.py) and takes the C4 call
list from tests/test_wino_pipe_gpu.py."""
import itertools, sys, time

import torch

from parent_compare import load, use, test_module, timed_rounds, timing_line, write_timing, timing_args
from sdeflow_light_amd import _lib, ops  # noqa: E402

DEV = "cuda"
ONLY = ""
if "--only" in sys.argv:
    i = sys.argv.index("--only")
    ONLY = sys.argv[i + 1]
    del sys.argv[i:i + 2]
NEW = _lib.lib()
PARENT = load(sys.argv[1])


class Case:
    """One ops.conv_forward call: geometry, channels and fused options; the inputs are drawn once from a seeded generator."""

    def __init__(self, kernel, N, Hi, Wi, Ho, Wo, KH, KW, C0, Cout, C1=0, stride=1, pad=None, mode=0, ups=0, CoutP=None, wino=False,
                 b6=False, bias=False, samp=False, acc=False, res=False, aff=None, act=0, stats=False, seed=0):
        self.kernel, self.wino, self.b6, self.acc = kernel, wino, b6, acc
        g = torch.Generator(device=DEV).manual_seed(seed)
        rnd = lambda n: torch.randn(n, device=DEV, generator=g)   # noqa: E731
        pad = (KW - 1) // 2 if pad is None else pad
        self.geom = ops.conv_geom(N, Hi, Wi, Ho, Wo, KH, KW, stride, pad, mode, ups)
        self.C0, self.C1, self.Cout = C0, C1, Cout
        self.CoutP = ops.pad16(Cout) if CoutP is None else CoutP
        Ktot = ops.pad16(C0) + (ops.pad16(C1) if C1 else 0)
        taps = 16 if wino else KH * KW
        self.Wp = rnd((3 if b6 else 1) * taps * self.CoutP * Ktot) * (1.0 / (taps * Ktot)) ** 0.5
        if b6:
            self.Wp = self.Wp.to(torch.bfloat16)
        self.src0 = rnd(N * Hi * Wi * C0)
        self.src1 = rnd(N * Hi * Wi * C1) if C1 else None
        self.n_out = N * Ho * Wo * Cout
        self.out0 = rnd(self.n_out) if acc else None
        kw = dict(src1=self.src1, C1=C1, CoutP=self.CoutP, wino=wino, b6=b6, accumulate=acc)
        if bias:
            kw.update(bias=rnd(Cout), n_bias=max(1, N // 2))
        if samp:
            ns = max(1, N // 3)
            kw.update(samp_bias=rnd(ns * Cout), n_samp=ns)
        if res:
            kw.update(residual=rnd(self.n_out))
        ctot = C0 + C1
        if aff == "identity":
            kw.update(in_scale=torch.ones(N * ctot, device=DEV), in_shift=torch.zeros(N * ctot, device=DEV))
        elif aff:
            kw.update(in_scale=1 + 0.3 * rnd(N * ctot), in_shift=0.2 * rnd(N * ctot), in_act=act)
        self.kw = kw
        self.S = ops.conv_chanstats_slots(self.geom, C0, C1, Cout, self.CoutP, wino=wino or b6) if stats else 0
        self.N = N
        self.desc = (f"{kernel:<34} N={N} {Hi}x{Wi}->{Ho}x{Wo} k{KH}x{KW} {C0}+{C1}->{Cout}/{self.CoutP} mode={mode} ups={ups} "
                     f"bias={int(bias)} samp={int(samp)} acc={int(acc)} res={int(res)} aff={aff} act={act} stats={self.S}")

    def run(self, h, out=None, cs=None):
        use(h)
        if out is None:
            out = self.out0.clone() if self.acc else torch.full((self.n_out,), float("nan"), device=DEV)
            cs = torch.full((self.N * self.S * 2 * self.Cout,), float("nan"), device=DEV) if self.S else None
        ops.conv_forward(self.geom, self.src0, self.C0, self.Wp, self.Cout, out, chanstats=cs, **self.kw)
        return out, cs


def tile_cases():
    """Every k_conv_tile instantiation: <TH, TW, NCO, KS, PT, DB> as conv_route picks them (see its conditions)."""
    full = dict(bias=True, samp=True, res=True, aff=True, act=1, stats=True)
    plain = dict(stats=True)
    acc = dict(bias=True, acc=True)
    both = dict(acc=True, res=True)                        # accumulate AND residual keep a 1x1 off the pixel-stationary kernel
    rows = [
        # 2-D 3x3, 256-pixel tiles (>= 512 of them), ragged image edges
        ("k_conv_tile<16,16,2,3,4,0>", dict(N=32, Hi=60, Wi=60, KH=3, KW=3, C0=32, Cout=32), (full, plain, acc)),
        ("k_conv_tile<16,16,4,3,4,0>", dict(N=32, Hi=60, Wi=60, KH=3, KW=3, C0=64, C1=32, Cout=64), (full, plain)),
        ("k_conv_tile<16,16,2,3,4,0> ups", dict(N=32, Hi=32, Wi=32, Ho=64, Wo=64, ups=1, KH=3, KW=3, C0=48, Cout=30, CoutP=32), (full, acc)),
        # 2-D, 128-pixel double-buffered tiles: the shapes of test_conv2d_fwd_bwd and small 1x1
        ("k_conv_tile<8,16,2,3,2,1>", dict(N=3, Hi=20, Wi=24, KH=3, KW=3, C0=32, Cout=32), (full, plain, acc)),
        ("k_conv_tile<8,16,2,3,2,1>", dict(N=1, Hi=8, Wi=8, KH=3, KW=3, C0=96, Cout=64), (full, plain)),
        ("k_conv_tile<8,16,2,3,2,1> ragged", dict(N=2, Hi=16, Wi=12, KH=3, KW=3, C0=80, Cout=45, CoutP=64), (full, acc)),
        ("k_conv_tile<8,16,4,3,2,1>", dict(N=512, Hi=8, Wi=16, KH=3, KW=3, C0=32, Cout=64), (full, plain)),
        ("k_conv_tile<8,16,2,1,2,1>", dict(N=2, Hi=16, Wi=16, KH=1, KW=1, C0=64, C1=32, Cout=32), (full, plain)),
        ("k_conv_tile<8,16,4,1,2,1>", dict(N=64, Hi=32, Wi=32, KH=1, KW=1, C0=64, Cout=64), (both,)),
        # 1-D (H = 1): the shapes of test_conv1d_fwd_bwd and the wide / four-tile forms
        ("k_conv_tile<1,128,2,3,2,1>", dict(N=3, Hi=1, Wi=100, KH=1, KW=3, C0=32, Cout=32), (full, plain, acc)),
        ("k_conv_tile<1,128,2,3,2,1>", dict(N=2, Hi=1, Wi=74, KH=1, KW=3, C0=64, Cout=128), (full,)),
        ("k_conv_tile<1,128,4,3,2,1>", dict(N=256, Hi=1, Wi=200, KH=1, KW=3, C0=32, Cout=64), (full, plain)),
        ("k_conv_tile<1,128,2,1,2,1>", dict(N=3, Hi=1, Wi=100, KH=1, KW=1, C0=32, Cout=32), (full, plain)),
        ("k_conv_tile<1,128,4,1,2,1>", dict(N=256, Hi=1, Wi=200, KH=1, KW=1, C0=32, Cout=64), (both,)),
        ("k_conv_tile<1,256,2,3,4,0>", dict(N=128, Hi=1, Wi=1000, KH=1, KW=3, C0=32, Cout=32), (full, plain)),
        ("k_conv_tile<1,256,4,3,4,0>", dict(N=128, Hi=1, Wi=1000, KH=1, KW=3, C0=32, Cout=64), (full, plain)),
    ]
    cases = []
    for i, (name, shp, opts) in enumerate(rows):
        shp = dict(shp)
        shp.setdefault("Ho", shp["Hi"]); shp.setdefault("Wo", shp["Wi"])
        for j, o in enumerate(opts):
            cases.append(Case(name, seed=100 * i + j, **shp, **o))
            if not shp.get("ups") and "aff" not in o:         # the dgrad of the same convolution: transposed gather (flip)
                cases.append(Case(name + " dgrad", seed=100 * i + j + 50, mode=1, **shp, **{k: v for k, v in o.items() if k != "stats"}))
    # the bf16-split form (B6), both output-channel widths
    for i, (C, nm) in enumerate(((32, "k_conv_tile<16,16,2,3,4,0,B6>"), (64, "k_conv_tile<16,16,4,3,4,0,B6>"))):
        cases.append(Case(nm, N=2, Hi=32, Wi=32, Ho=32, Wo=32, KH=3, KW=3, C0=C, Cout=C, b6=True, seed=900 + i, **full))
    return cases


def small_cases():
    cases = []
    for N in (2, 6):                                       # the k_dgrad_s2 shapes of tests/test_conv_tail_gpu.py
        for i, (Cin, Cout, H) in enumerate(((32, 32, 16), (64, 64, 8), (32, 32, 24))):
            for j, o in enumerate((dict(), dict(bias=True), dict(samp=True), dict(acc=True), dict(res=True, bias=True))):
                cases.append(Case("k_dgrad_s2", N=N, Hi=H // 2, Wi=H // 2, Ho=H, Wo=H, KH=3, KW=3, stride=2, pad=1, mode=1, C0=Cout,
                                  Cout=Cin, seed=2000 + 100 * i + 10 * j + N, **o))
    for CO in (1, 2, 3, 4):                                # the U-Net's output convolution, with the folded GroupNorm + SiLU
        cases.append(Case(f"k_conv3x3_cout_small<{CO}>", N=4, Hi=20, Wi=24, Ho=20, Wo=24, KH=3, KW=3, C0=32, Cout=CO, bias=True, samp=True,
                          res=True, aff=True, act=1, seed=3000 + CO))
        cases.append(Case(f"k_conv3x3_cout_small<{CO}>", N=3, Hi=64, Wi=64, Ho=64, Wo=64, KH=3, KW=3, C0=32, Cout=CO, acc=True, seed=3010 + CO))
    return cases


def wino_kernel(C0, C1, CoutP, N, H, aff):
    if not aff:
        return "k_conv_wino_pipe"
    if not C1 and C0 == 32 and CoutP == 32 and N * (H // 16) ** 2 >= 1024:
        return "k_conv_wino_p32"
    return "k_conv_wino<2,LDS weights>" if ops.pad16(C0) + ops.pad16(C1) >= 64 else "k_conv_wino<2,register weights>"


def wino_cases():
    cases = []
    use(NEW)
    calls = test_module("test_wino_pipe_gpu")._c4_winograd_calls()          # what one C4 training step sends to the Winograd entry
    for i, (C0, C1, Cout, CoutP, H, ups, acc, res, bias, samp, stats) in enumerate(calls):
        for N in (2, 13):
            for aff in (None, "identity"):
                Hi = H // 2 if ups else H
                cases.append(Case(wino_kernel(C0, C1, CoutP, N, H, aff), N=N, Hi=Hi, Wi=Hi, Ho=H, Wo=H, KH=3, KW=3, C0=C0, C1=C1, Cout=Cout,
                                  CoutP=CoutP, ups=int(ups), wino=True, acc=acc, res=res, bias=bias, samp=samp, stats=stats, aff=aff,
                                  seed=4000 + 10 * i + N))
    rows = [(32, 0, 32, 32), (32, 0, 64, 64), (32, 0, 96, 96), (48, 16, 80, 96), (16, 0, 30, 32), (64, 32, 32, 32), (128, 128, 128, 128)]
    for i, (C0, C1, Cout, CoutP) in enumerate(rows):       # the rows of test_wino_pipe_shapes_and_fused_options, real affine + SiLU
        for ups in (0, 1):
            for (N, H, o) in ((3, 32, dict(acc=True, res=True, bias=True, samp=True)), (5, 16, dict(bias=True))):
                for aff in (True, None):
                    Hi = H // 2 if ups else H
                    cases.append(Case(wino_kernel(C0, C1, CoutP, N, H, aff), N=N, Hi=Hi, Wi=Hi, Ho=H, Wo=H, KH=3, KW=3, C0=C0, C1=C1,
                                      Cout=Cout, CoutP=CoutP, ups=ups, wino=True, stats=Cout % 4 == 0, aff=aff, act=1 if aff else 0,
                                      seed=5000 + 10 * i + ups, **o))
    # the persistent 32 -> 32 form: 1040 tiles (a ragged last round), real affine + SiLU
    cases.append(Case("k_conv_wino_p32", N=65, Hi=64, Wi=64, Ho=64, Wo=64, KH=3, KW=3, C0=32, Cout=32, wino=True, bias=True, samp=True,
                      res=True, stats=True, aff=True, act=1, seed=6000))
    # every body of the shared epilogue (wino_epilogue: each subset of bias / per-sample bias / accumulate / residual, with and
    # without statistics) on every kernel that calls it; Cout = 30 takes the per-quad path (no statistics: Cout % 4 != 0)
    rows = [(3, 32, 16, 16, 32, 32, None), (3, 16, 32, 0, 64, 64, None), (3, 16, 16, 0, 30, 32, None),     # k_conv_wino_pipe
            (3, 32, 32, 0, 32, 32, "identity"), (3, 32, 64, 0, 64, 64, "identity"), (3, 16, 32, 0, 30, 32, "identity"),
            (256, 32, 32, 0, 32, 32, "identity")]                                                           # 1024 tiles: k_conv_wino_p32
    for i, (N, H, C0, C1, Cout, CoutP, aff) in enumerate(rows):
        for k, o in enumerate(itertools.product((False, True), repeat=4)):
            for stats in ((False, True) if Cout % 4 == 0 and N < 256 else (Cout % 4 == 0,)):
                cases.append(Case(wino_kernel(C0, C1, CoutP, N, H, aff), N=N, Hi=H, Wi=H, Ho=H, Wo=H, KH=3, KW=3, C0=C0, C1=C1, Cout=Cout,
                                  CoutP=CoutP, wino=True, bias=o[0], samp=o[1], acc=o[2], res=o[3], stats=stats, aff=aff,
                                  seed=7000 + 100 * i + k))
    return cases


def bitwise():
    t0 = time.time()
    n = bad = 0
    for group in (tile_cases, small_cases, wino_cases):
        for c in group():
            if ONLY not in c.kernel:
                continue
            o_p, s_p = c.run(PARENT)
            o_n, s_n = c.run(NEW)
            torch.cuda.synchronize()
            ok = bool(torch.isfinite(o_n).all()) and torch.equal(o_p, o_n)
            if c.S:
                ok = ok and bool(torch.isfinite(s_n).all()) and torch.equal(s_p, s_n)
            n += 1
            bad += not ok
            print(f"{'equal' if ok else 'DIFFERENT':<9} {c.desc}", flush=True)
    print(f"cases run {n}, bit-identical to the parent (outputs and channel statistics) {n - bad}, different or non-finite {bad} "
          f"({time.time() - t0:.0f} s)")
    return bad


def time_cases():
    N = 1024                                               # the shapes of tools/bench_wino.py 1024, with and without the folded transform
    for (H, C0, C1, Co) in ((64, 32, 0, 32), (64, 64, 32, 32), (32, 64, 0, 64), (32, 128, 64, 64), (16, 128, 0, 128), (16, 128, 128, 128)):
        for aff in (True, None):
            yield Case(wino_kernel(C0, C1, Co, N, H, aff), N=N, Hi=H, Wi=H, Ho=H, Wo=H, KH=3, KW=3, C0=C0, C1=C1, Cout=Co, wino=True,
                       aff=aff, act=1 if aff else 0, seed=H + C0)
    B = 512                                                # the C4 step: 256 samples, primal + tangent rows
    # its Winograd shapes through k_conv_wino_pipe, with the option sets of the step: a dgrad or tangent-only call (plain), a
    # ResBlock's conv1 (bias + per-sample bias) and conv2 (bias + residual), a dgrad that accumulates
    for (H, C0, C1, Co) in ((64, 32, 0, 32), (64, 64, 32, 32), (32, 64, 0, 64), (32, 128, 64, 64), (16, 128, 0, 128), (16, 128, 128, 128)):
        for j, o in enumerate((dict(), dict(bias=True, samp=True, stats=True), dict(bias=True, res=True, stats=True), dict(acc=True))):
            yield Case(wino_kernel(C0, C1, Co, B, H, None), N=B, Hi=H, Wi=H, Ho=H, Wo=H, KH=3, KW=3, C0=C0, C1=C1, Cout=Co, wino=True,
                       seed=8000 + H + C0 + j, **o)
    full = dict(bias=True, res=True, stats=True)
    for (H, C0, C1, Co) in ((64, 32, 0, 32), (32, 64, 0, 64), (32, 64, 32, 64), (16, 128, 0, 128), (8, 128, 0, 128)):
        nco = 4 if Co % 64 == 0 else 2
        name = f"k_conv_tile<16,16,{nco},3,4,0>" if H >= 16 else f"k_conv_tile<8,16,{nco},3,2,1>"
        yield Case(name, N=B, Hi=H, Wi=H, Ho=H, Wo=H, KH=3, KW=3, C0=C0, C1=C1, Cout=Co, seed=H, **full)
        if not C1:
            yield Case(name + " dgrad", N=B, Hi=H, Wi=H, Ho=H, Wo=H, KH=3, KW=3, C0=C0, Cout=Co, mode=1, acc=True, seed=H + 1)
    yield Case("k_conv_tile<8,16,4,1,2,1>", N=B, Hi=32, Wi=32, Ho=32, Wo=32, KH=1, KW=1, C0=64, Cout=64, acc=True, res=True, seed=7)
    for (H, C) in ((64, 32), (32, 64)):                    # dgrad of the two stride-2 downsampling convolutions
        yield Case("k_dgrad_s2", N=B, Hi=H // 2, Wi=H // 2, Ho=H, Wo=H, KH=3, KW=3, stride=2, pad=1, mode=1, C0=C, Cout=C, acc=True, seed=H)
    for CO in (1, 2, 3, 4):
        yield Case(f"k_conv3x3_cout_small<{CO}>", N=B, Hi=64, Wi=64, Ho=64, Wo=64, KH=3, KW=3, C0=32, Cout=CO, bias=True, aff=True, act=1, seed=9)
    # the register-weight Winograd form: one 32-channel chunk, below the persistent form's 1024 tiles
    yield Case(wino_kernel(32, 0, 32, 60, 64, True), N=60, Hi=64, Wi=64, Ho=64, Wo=64, KH=3, KW=3, C0=32, Cout=32, wino=True, aff=True, act=1, seed=11)
    for (H, C) in ((64, 32), (32, 64)):                    # bf16-split forms
        yield Case(f"k_conv_tile<16,16,{C // 16},3,4,0,B6>", N=256, Hi=H, Wi=H, Ho=H, Wo=H, KH=3, KW=3, C0=C, Cout=C, b6=True, aff=True, act=1,
                   stats=True, seed=12)
    both = dict(acc=True, res=True)
    for C in (32, 64):                                     # the remaining 2-D forms and the 1-D ones (UNet1D shapes)
        nco = C // 16
        yield Case(f"k_conv_tile<8,16,{nco},3,2,1>", N=B, Hi=8, Wi=16, Ho=8, Wo=16, KH=3, KW=3, C0=C, Cout=C, seed=13, **full)
        yield Case(f"k_conv_tile<8,16,{nco},1,2,1>", N=B, Hi=16, Wi=16, Ho=16, Wo=16, KH=1, KW=1, C0=C, Cout=C, seed=14, **both)
        yield Case(f"k_conv_tile<1,256,{nco},3,4,0>", N=1024, Hi=1, Wi=1024, Ho=1, Wo=1024, KH=1, KW=3, C0=C, Cout=C, seed=15, **full)
        yield Case(f"k_conv_tile<1,128,{nco},3,2,1>", N=2048, Hi=1, Wi=128, Ho=1, Wo=128, KH=1, KW=3, C0=C, Cout=C, seed=16, **full)
        yield Case(f"k_conv_tile<1,128,{nco},1,2,1>", N=2048, Hi=1, Wi=128, Ho=1, Wo=128, KH=1, KW=1, C0=C, Cout=C, seed=17, **both)


def timing(path, variants):
    """Every case of time_cases() through parent_compare.timed_rounds (parent / parent again / this tree / variants, alternated;
    the yardstick is the parent against itself), the rounds in the JSON."""
    ROUNDS, REPS, WARM = 7, 20, 5
    rows = []
    for c in time_cases():
        if ONLY not in c.kernel:
            continue
        out, cs = c.run(NEW)                               # buffers reused by every timed launch
        row = timed_rounds(lambda h: c.run(h, out, cs), PARENT, [("new", NEW)] + variants, ROUNDS, REPS, WARM)
        rows.append(dict(kernel=c.kernel, case=c.desc, **row))
        print(timing_line(c.kernel, row), flush=True)
    if path:
        write_timing(path, rows, variants, ROUNDS, REPS, WARM)
    return 0


if __name__ == "__main__":
    if "--time" in sys.argv:
        sys.exit(timing(*timing_args(sys.argv)))
    sys.exit(1 if bitwise() else 0)
