#!/usr/bin/env python3
"""GPU box: the GroupNorm and attention kernels of this tree's library against another build of it (the parent commit's
libmsgm_hip.so, built into a scratch path), both loaded into one process, as conv_vs_parent.py / wgrad_vs_parent.py do for the
convolutions (the shared parts: tools/parent_compare.py):
    python tools/unet_vs_parent.py <parent.so> [--only NAME]        bitwise: every output, workspace slab and job descriptor
    python tools/unet_vs_parent.py <parent.so> [--only NAME] --time [out.json] [name=variant.so ...]
                                                                    timing: parent / parent again / this tree (/ further builds,
                                                                    e.g. one phase routed through its shared function),
                                                                    alternated; --only keeps the rows whose kernel contains NAME
Every case goes through the raw ABI on the same seeded inputs; all outputs and workspaces start NaN-filled (so a skipped store
shows) and are the SAME buffers for both builds (so the reduction job descriptors, which hold addresses, compare byte for
byte).  The kernels printed with a case are what this script EXPECTS the launchers to pick (their conditions, restated in
gn_expect / attn_expect), not something observed."""
import ctypes, sys, time

import torch

from parent_compare import load, same, timed_rounds, timing_line, write_timing, timing_args
from sdeflow_light_amd import _lib as L, ops  # noqa: E402

DEV = "cuda"
NEW = L.lib()
PARENT = load(sys.argv[1])
NAN = float("nan")
ONLY = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""


def nans(n):
    return torch.full((int(n),), NAN, device=DEV)


def check(rc):
    assert rc == 0, rc


# ------------------------------------------------------------------------------------------------ GroupNorm
def gn_chunks(Bp, P):
    """gn_chunks of unet2d_kernels.hip: (pixels per reduce workgroup, workgroups per sample)."""
    c = min(max((P + 31) // 32, 64), P)
    m = max(((P + c - 1) // c) // max((512 + Bp - 1) // Bp, 1), 1)
    return m * c, (P + m * c - 1) // (m * c)


def gn_expect(C, C0, drop, Bp, P, affine=False):
    vec = C % 4 == 0 and (not affine or C0 % 4 == 0)
    chunk, nch = gn_chunks(Bp, P)
    return f"<{'VEC' if vec else 'scalar'}{',DROP' if drop else ''}> {nch} chunk(s) of {chunk}{' (last ragged)' if P % chunk else ''}"


class Gn:
    """One GroupNorm layer: x [2Bp][P][C] (or two sources C0 | C1), seeded inputs, one set of NaN-refilled output buffers."""

    def __init__(self, Bp, P, C, G, C1=0, seed=0):
        self.Bp, self.P, self.C0, self.C1, self.C, self.G = Bp, P, C - C1, C1, C, G
        g = torch.Generator(device=DEV).manual_seed(seed)
        rnd = lambda n: torch.randn(n, device=DEV, generator=g)   # noqa: E731
        n = 2 * Bp * P
        self.x0, self.x1 = rnd(n * self.C0) * 1.5 + 0.3, (rnd(n * C1) if C1 else None)
        self.gamma, self.beta = 1 + 0.2 * rnd(C), 0.2 * rnd(C)
        self.gout, self.res, self.res2 = rnd(n * C), rnd(n * C), rnd(n * C)
        self.rng = L.PhiloxState(1234 + seed, DEV, offset=77)
        self.drop = ops.dropout_desc(self.rng, 3, 0.1)
        self.ws = torch.empty(int(NEW.msgm_groupnorm_workspace(Bp, G)) // 4, device=DEV)
        self.out, self.stats, self.gx0, self.gx1 = nans(n * C), nans(Bp * G * 4), nans(n * self.C0), (nans(n * C1) if C1 else None)
        self.dga, self.dbe, self.scale, self.shift = nans(C), nans(C), nans(Bp * C), nans(Bp * C)
        self.ps = nans(int(NEW.msgm_groupnorm_param_slots_bytes(Bp, P, C)) // 4)
        self.lean = False            # timing: launches only (no refill, no synchronize, no copies; backward reuses self.stats)

    def _fill(self, *ts):
        if self.lean:
            return
        self.ws.fill_(NAN)
        for t in ts:
            if t is not None:
                t.fill_(NAN)

    def forward(self, h, dual, silu, drop=False):
        self._fill(self.out, self.stats)
        p, a = L.ptr, (self.Bp, self.P)
        tail = (int(dual), int(silu), 1e-5, p(self.ws), self.ws.numel() * 4)
        if self.C1:
            check(h.msgm_groupnorm_dual_forward2(p(self.x0), self.C0, p(self.x1), self.C1, p(self.gamma), p(self.beta), p(self.out), p(self.stats),
                                                 *a, self.G, *tail, L.stream()))
        elif drop:
            check(h.msgm_groupnorm_dual_forward_dropout(p(self.x0), p(self.gamma), p(self.beta), p(self.out), p(self.stats), *a, self.C, self.G,
                                                        *tail, ctypes.byref(self.drop), L.stream()))
        else:
            check(h.msgm_groupnorm_dual_forward(p(self.x0), p(self.gamma), p(self.beta), p(self.out), p(self.stats), *a, self.C, self.G, *tail,
                                                L.stream()))
        if self.lean:
            return [None, self.stats]
        torch.cuda.synchronize()
        n = (2 if dual else 1) * self.Bp * self.P * self.C
        return [self.out[:n].clone(), self.stats.clone(), self.ws.clone()]

    def backward(self, h, silu, form, drop=False):
        """form "own": msgm_groupnorm_dual_backward(2) with its own parameter reduction (+ residual, single source);
        "slots": the DeferredReduces form (+ residual and residual2, single source), the job descriptors compared too."""
        stats = self.stats if self.lean else self.forward(h, True, silu, drop)[1]
        self._fill(self.gx0, self.gx1, self.ps)
        if not self.lean:
            self.dga.fill_(0.5); self.dbe.fill_(-0.25)        # the own reduction ADDS to them
        p, two = L.ptr, bool(self.C1)
        head = (p(self.gamma), p(self.beta), p(stats), p(self.gout))
        res, res2 = (None if two else p(self.res)), (None if two else p(self.res2))
        wsb, extra = (p(self.ws), self.ws.numel() * 4), []
        if form == "own" and two:
            check(h.msgm_groupnorm_dual_backward2(p(self.x0), self.C0, p(self.x1), self.C1, *head, p(self.gx0), p(self.gx1), p(self.dga), p(self.dbe),
                                                  self.Bp, self.P, self.G, int(silu), 1e-5, *wsb, L.stream()))
        elif form == "own":
            check(h.msgm_groupnorm_dual_backward(p(self.x0), *head, p(self.gx0), p(self.dga), p(self.dbe), self.Bp, self.P, self.C, self.G,
                                                 int(silu), 1e-5, res, *wsb, L.stream()))
        else:
            jobs, nj = (L.ReduceJobT * 2)(), ctypes.c_int32(0)
            rest = (int(silu), 1e-5, res, res2, *wsb, p(self.ps), self.ps.numel() * 4, jobs, ctypes.byref(nj))
            if drop:
                check(h.msgm_groupnorm_dual_backward_slots_dropout(p(self.x0), *head, p(self.gx0), p(self.dga), p(self.dbe), self.Bp, self.P, self.C,
                                                                   self.G, *rest, ctypes.byref(self.drop), L.stream()))
            else:
                check(h.msgm_groupnorm_dual_backward_slots(p(self.x0), self.C0, p(self.x1), self.C1, *head, p(self.gx0), p(self.gx1), p(self.dga),
                                                           p(self.dbe), self.Bp, self.P, self.G, *rest, L.stream()))
            extra = [] if self.lean else [torch.tensor(list(bytes(jobs)) + [nj.value], dtype=torch.float32), self.ps.clone()]
        if self.lean:
            return None
        torch.cuda.synchronize()
        return [self.gx0.clone(), None if self.gx1 is None else self.gx1.clone(), self.dga.clone(), self.dbe.clone(), self.ws.clone()] + extra

    def affine(self, h):
        self._fill(self.scale, self.shift)
        p = L.ptr
        check(h.msgm_groupnorm_affine(p(self.x0), self.C0, p(self.x1), self.C1, p(self.gamma), p(self.beta), p(self.scale), p(self.shift),
                                      self.Bp, self.P, self.G, 1e-5, p(self.ws), self.ws.numel() * 4, L.stream()))
        torch.cuda.synchronize()
        return [self.scale.clone(), self.shift.clone(), self.ws.clone()]

    def affine_cs(self, h, S=3):
        """The same map from channel sums (k_gn_affine_cs): cs [Bp][S][2][C] per source, fp32 sums over the pixels p = s mod S."""
        self._fill(self.scale, self.shift)
        p, n = L.ptr, self.Bp * self.P

        def sums(x, C):
            x = x[: n * C].view(self.Bp, self.P, C)
            return torch.stack([torch.stack([x[:, s::S].sum(1), (x[:, s::S] ** 2).sum(1)], 1) for s in range(S)], 1).contiguous()
        cs0 = sums(self.x0, self.C0)
        cs1 = sums(self.x1, self.C1) if self.C1 else None
        check(h.msgm_groupnorm_affine_chanstats(p(cs0), S, self.C0, p(cs1), S if self.C1 else 0, self.C1, p(self.gamma), p(self.beta),
                                                p(self.scale), p(self.shift), self.Bp, self.P, self.G, 1e-5, L.stream()))
        torch.cuda.synchronize()
        return [self.scale.clone(), self.shift.clone()]

    def mask(self, h):
        self._fill(self.out)
        check(h.msgm_dropout_mask(ctypes.byref(self.drop), self.Bp, self.P, self.C, L.ptr(self.out), L.stream()))
        torch.cuda.synchronize()
        return [self.out[:self.Bp * self.P * self.C].clone()]


def gn_cases(Bp=3):
    """(description, callable(library) -> outputs).  P = 64 / 100 / 128: one chunk, two with the second ragged, two full;
    C = 96 leaves dead threads, C = 256 has PL = 4 pixel lanes, C = 6 is the scalar build."""
    for i, P in enumerate((64, 100, 128)):
        for C, G in ((32, 32), (96, 32), (256, 32), (6, 6)):
            gn, e = Gn(Bp, P, C, G, seed=10 * i + C), gn_expect(C, C, False, Bp, P)
            tag = f"Bp={Bp} P={P} C={C} G={G}"
            for silu in (0, 1):
                for dual in (0, 1):
                    yield f"k_gn_fwd_reduce/apply{e} {tag} dual={dual} silu={silu}", lambda h, gn=gn, d=dual, s=silu: gn.forward(h, d, s)
                yield f"k_gn_bwd_reduce/apply{e} + k_gn_param_reduce {tag} silu={silu} residual", lambda h, gn=gn, s=silu: gn.backward(h, s, "own")
                yield f"k_gn_bwd_reduce/apply{e} slots {tag} silu={silu} residual+residual2", lambda h, gn=gn, s=silu: gn.backward(h, s, "slots")
            yield f"k_gn_fwd_reduce{gn_expect(C, C, False, Bp, P, True)} + k_gn_affine {tag}", gn.affine
            yield f"k_gn_affine_cs 3 slots {tag}", gn.affine_cs
            if C % 4 == 0:
                ed = gn_expect(C, C, True, Bp, P)
                yield f"k_gn_fwd_reduce<VEC> k_gn_fwd_apply{ed} {tag} dual=1 silu=1 p=0.1", lambda h, gn=gn: gn.forward(h, 1, 1, True)
                yield f"k_gn_fwd_apply{ed} {tag} dual=0 silu=1 p=0.1", lambda h, gn=gn: gn.forward(h, 0, 1, True)
                yield f"k_gn_bwd_reduce/apply{ed} slots {tag} silu=1 p=0.1 residual+residual2", lambda h, gn=gn: gn.backward(h, 1, "slots", True)
                yield f"k_dropout_mask {tag}", gn.mask
        gn, e, tag = Gn(Bp, P, 96, 32, C1=64, seed=500 + i), gn_expect(96, 32, False, Bp, P), f"Bp={Bp} P={P} C=32+64 G=32"
        for silu in (0, 1):
            for dual in (0, 1):
                yield f"k_gn_fwd_reduce/apply{e} two-source {tag} dual={dual} silu={silu}", lambda h, gn=gn, d=dual, s=silu: gn.forward(h, d, s)
            yield f"k_gn_bwd_reduce/apply{e} + k_gn_param_reduce two-source {tag} silu={silu}", lambda h, gn=gn, s=silu: gn.backward(h, s, "own")
            yield f"k_gn_bwd_reduce/apply{e} slots two-source {tag} silu={silu}", lambda h, gn=gn, s=silu: gn.backward(h, s, "slots")
        yield f"k_gn_fwd_reduce{gn_expect(96, 32, False, Bp, P, True)} + k_gn_affine two-source {tag}", gn.affine
        yield f"k_gn_affine_cs 3 | 3 slots two-source {tag}", gn.affine_cs


# ------------------------------------------------------------------------------------------------ attention
def attn_expect(kind, N, T, H, D, mh):
    """The instantiations attention_kernels.hip / attention_train_kernels.hip pick (N = samples, or dual pairs Bp)."""
    single = not mh or (H == 1 and D != 16)
    m, nh = ("false" if single else "true"), (1 if single else H)
    if kind == "sampler":
        return f"k_attn_fwd<{D // 16},{2 if T % 128 == 0 and D != 128 else 1},{m}>"
    if kind == "fwd":
        kb, nw = {16: 64, 32: 64, 64: 32, 128: 16}[D], (2 if D == 128 and not (T % 64 == 0 and N * nh * (T // 64) >= 512) else 4)
        return f"k_attn_dual_fwd<{D // 16},1,{kb},{nw},{m}>"
    kg = 2 if D == 128 else 4
    nkb = T // (16 * kg)
    kseq = 2 if nkb % 2 == 0 and N * nh * (nkb // 2) >= 1024 else 1
    return f"k_attn_dual_bwd<{D // 16},{kg},false{'+true' if kseq == 2 else ''},{m}> kseq={kseq} + k_attn_dual_delta/dq_reduce<{m}>"


class Attn:
    """One attention shape through the single-head (mh = False) or the multi-head entries."""

    def __init__(self, N, T, H, D, mh, seed=0):
        self.N, self.T, self.H, self.D, self.mh, self.C = N, T, H, D, mh, H * D
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.qkv = torch.randn(2 * N * T * 3 * self.C, device=DEV, generator=g)
        self.datt = torch.randn(2 * N * T * self.C, device=DEV, generator=g)
        self.scale = float(D) ** -0.5
        self.hd = (H, D) if mh else (D,)
        self.tag = f"N={N} T={T} " + (f"heads={H} D={D}" if mh else f"C={D}")
        self.bufs = None

    def sampler(self, h):
        out = nans(self.N * self.T * self.C)
        check((h.msgm_attention_mh_forward if self.mh else h.msgm_attention_forward)(L.ptr(self.qkv), L.ptr(out), self.N, self.T, *self.hd,
                                                                                   self.scale, L.stream()))
        torch.cuda.synchronize()
        return [out]

    def alloc(self):
        if self.bufs is None:
            need = int((NEW.msgm_attention_dual_mh_workspace if self.mh else NEW.msgm_attention_dual_workspace)(self.N, self.T, *self.hd))
            self.bufs = (nans(2 * self.N * self.T * self.C), nans(2 * self.N * self.H * self.T), nans(2 * self.N * self.T * 3 * self.C),
                         nans(need // 4))
        return self.bufs

    def fwd(self, h, fill=True):
        att, stats, _, _ = self.alloc()
        if fill:
            att.fill_(NAN); stats.fill_(NAN)
        check((h.msgm_attention_dual_mh_forward if self.mh else h.msgm_attention_dual_forward)(L.ptr(self.qkv), L.ptr(att), L.ptr(stats), self.N,
                                                                                             self.T, *self.hd, self.scale, L.stream()))

    def bwd(self, h, fill=True):
        att, stats, dqkv, ws = self.alloc()
        if fill:
            dqkv.fill_(NAN); ws.fill_(NAN)
        check((h.msgm_attention_dual_mh_backward if self.mh else h.msgm_attention_dual_backward)(
            L.ptr(self.qkv), L.ptr(att), L.ptr(self.datt), L.ptr(stats), L.ptr(dqkv), self.N, self.T, *self.hd, self.scale, L.ptr(ws),
            ws.numel() * 4, L.stream()))

    def dual(self, h):
        """att, stats, dqkv and the backward workspace (row scalars c | delta and the query-gradient slabs)."""
        self.fwd(h); self.bwd(h)
        torch.cuda.synchronize()
        return [t.clone() for t in self.bufs]


SAMPLER = [(3, 64, 1, 32, 0), (2, 128, 1, 32, 0), (3, 64, 1, 64, 0), (2, 128, 1, 64, 0), (2, 64, 1, 128, 0)] + \
          [(2, T, 2, D, 1) for D in (16, 32, 64) for T in (64, 128)] + [(2, 128, 2, 128, 1)]
DUAL = [(3, 64, 1, 32, 0), (3, 64, 1, 64, 0), (9, 96, 1, 128, 0), (1, 32, 1, 128, 0), (512, 64, 1, 128, 0), (1024, 128, 1, 32, 0),
        (1024, 64, 1, 128, 0), (3, 64, 2, 16, 1), (3, 64, 2, 32, 1), (2, 64, 2, 64, 1), (5, 96, 2, 128, 1), (256, 64, 2, 128, 1),
        (256, 128, 4, 32, 1), (3, 64, 1, 64, 1), (3, 64, 1, 16, 1),      # these two: one head through the multi-head entries
        # tests/test_attn_dual_paths_gpu.py: one key block, an odd count, the decode's tail, C = 64 with kseq = 2, D = 64 at two heads
        (1, 64, 1, 64, 0), (3, 192, 1, 64, 0), (9, 128, 1, 64, 0), (1024, 128, 1, 64, 0), (5, 128, 2, 64, 1),
        # tests/test_attn_dual_c128_gpu.py ((1, 32, 1, 128) is above): T no multiple of 64, the decode's tail, the NW = 4 forward with
        # the two-launch backward at two slab groups, the multi-head builds at NW = 2 and NW = 4; then the benchmark's own shape
        (3, 96, 1, 128, 0), (9, 64, 1, 128, 0), (512, 128, 1, 128, 0), (5, 64, 2, 128, 1), (256, 64, 2, 128, 1), (256, 256, 1, 128, 0)]


def attn_cases():
    for i, (N, T, H, D, mh) in enumerate(SAMPLER):
        a = Attn(N, T, H, D, mh, seed=300 + i)
        yield f"{attn_expect('sampler', N, T, H, D, mh)} {a.tag}", a.sampler
    for i, (N, T, H, D, mh) in enumerate(DUAL):
        yield (f"{attn_expect('fwd', N, T, H, D, mh)} {attn_expect('bwd', N, T, H, D, mh)} Bp={N} T={T} " + (f"heads={H} D={D}" if mh else f"C={D}"),
               lambda h, s=(N, T, H, D, mh, 400 + i): Attn(*s).dual(h))


def bitwise():
    t0, n, bad = time.time(), 0, 0
    for gen in (gn_cases, attn_cases):
        for desc, run in gen():
            if ONLY not in desc:
                continue
            a, b = run(PARENT), run(NEW)
            ok = len(a) == len(b) and all(same(x, y) for x, y in zip(a, b)) and bool(torch.isfinite(b[0]).all())
            n += 1; bad += not ok
            print(f"{'equal' if ok else 'DIFFERENT':<9} {desc}", flush=True)
            del a, b
            torch.cuda.empty_cache()
    print(f"cases run {n}, bit-identical to the parent (outputs, statistics, workspaces, job descriptors) {n - bad}, different {bad} "
          f"({time.time() - t0:.0f} s)")
    return bad


# ------------------------------------------------------------------------------------------------ timing
def timing(path, variants):
    """GroupNorm at the benchmark's C4 64x64x32 layer (dual batch 512) and at the 32-row shard, every attention family at the C4
    network's two attention shapes (32x32 at 64 channels, 16x16 at 128; two heads for the multi-head builds, of 32, 64 and 128
    channels), the kseq = 2 cases."""
    ROUNDS, REPS, WARM = 5, 20, 3
    rows = []

    def go(kernel, call):
        if ONLY not in kernel:
            return
        row = timed_rounds(call, PARENT, [("new", NEW)] + variants, ROUNDS, REPS, WARM)
        rows.append(dict(kernel=kernel, **row))
        print(timing_line(kernel, row), flush=True)

    for Bp in (256, 32):
        gn = Gn(Bp, 4096, 32, 32, seed=Bp)
        gn.forward(PARENT, 1, 1)                             # statistics for the lean backward calls
        gn.lean = True
        for name, call in (("fwd", lambda h: gn.forward(h, 1, 1)), ("fwd dropout", lambda h: gn.forward(h, 1, 1, True)),
                           ("bwd own reduction", lambda h: gn.backward(h, 1, "own")), ("bwd slots", lambda h: gn.backward(h, 1, "slots"))):
            go(f"GroupNorm {name} Bp={Bp} P=4096 C=32", call)
        del gn
        torch.cuda.empty_cache()
    for (N, T, H, D, mh) in ((256, 1024, 1, 64, 0), (256, 256, 1, 128, 0), (256, 1024, 2, 32, 1), (256, 256, 2, 64, 1), (256, 256, 2, 128, 1),
                             (1024, 128, 1, 32, 0), (1024, 64, 1, 128, 0)):
        a = Attn(N, T, H, D, mh, seed=N + T)
        if N == 256:
            go(f"{attn_expect('sampler', N, T, H, D, mh)} {a.tag}", lambda h: check((h.msgm_attention_mh_forward if mh else h.msgm_attention_forward)(
                L.ptr(a.qkv), L.ptr(a.alloc()[0]), N, T, *a.hd, a.scale, L.stream())))
        go(f"{attn_expect('fwd', N, T, H, D, mh)} {a.tag}", lambda h: a.fwd(h, False))
        go(f"{attn_expect('bwd', N, T, H, D, mh)} {a.tag}", lambda h: a.bwd(h, False))
        del a
        torch.cuda.empty_cache()
    if path:
        write_timing(path, rows, variants, ROUNDS, REPS, WARM)
    return 0


if __name__ == "__main__":
    sys.exit(timing(*timing_args(sys.argv)) if "--time" in sys.argv else (1 if bitwise() else 0))
