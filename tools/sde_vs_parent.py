#!/usr/bin/env python3
"""GPU box: every kernel of csrc/sde_kernels.hip in this tree's library against another build of it (the parent commit's
libmsgm_hip.so, built into a scratch path), both loaded into one process (the shared parts: tools/parent_compare.py):
    python tools/sde_vs_parent.py <parent.so> [list.txt]                      bitwise: every output, parent_compare.same
    python tools/sde_vs_parent.py <parent.so> --time [out.json]               timing: parent / parent again / this tree, alternated
The bitwise cases are those of tests/test_sde_paths_gpu.py — its shape lists, its input makers and its C-ABI callers, imported,
not copied — plus msgm_ssm_prep at the test's shapes.  A case is a function that launches on inputs drawn once from a seeded
generator and returns its outputs (NaN-filled before the launch); it runs once under each library.  The run stops at the
first HIP error (a Python exception): nothing is launched after it."""
import sys, time

import numpy as np
import torch

from parent_compare import load, use, same, test_module, timed_rounds, timing_line, write_timing, timing_args
from sdeflow_light_amd import _lib as L, ops  # noqa: E402

DEV = "cuda"
TIME = "--time" in sys.argv
NEW = L.lib()
PARENT = load(sys.argv[1])
T = test_module("test_sde_paths_gpu")
R, nan, shifted = T.R, T.nan, T.shifted


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def stage_cases():
    def one(tag, kind, B, n, combos, seed=None, shift=False, **opt):
        d = R.stage_inputs(B, n, 131 * n + B if seed is None else seed, DEV)
        if kind == "dense":
            opt = dict(opt, **dict(zip(("G", "L_G"), R.dense_G(n, device=DEV))))
        if shift:
            opt["x"] = shifted(d["x"])
        for proc, strato, lmbd in combos:
            yield (f"stage {tag} {kind} ({B},{n}) {proc} strato={strato} lmbd={lmbd}",
                   lambda p=proc, s=strato, l=lmbd, o=dict(opt): T.run_stage(ops, L, kind, p, s, l, d, **o))

    for kind, B, n, shift in T.FLAT:
        yield from one("flat" + (" shifted-x" if shift else ""), kind, B, n, R.COMBOS, shift=shift)
    yield from one("flat scalar body, grid stride", "sgm", 699051, 3, R.COMBOS[:2])
    for n in (3, 4, 6):
        yield from one("fallback", "sparse", 33, n, R.COMBOS)
    yield from one("fallback norm0", "sparse", 33, 8, R.COMBOS, norm0=True)
    for dr in (False, True):
        yield from one(f"fallback shifted-x dr={dr}", "sparse", 33, 8, R.COMBOS, seed=77, shift=True, base="third", c_out=0.5, dr=dr)
    for variant, (kind, opt) in T.ROWS_VARIANTS.items():
        for B, n in R.row_shapes():
            yield from one(variant, kind, B, n, R.COMBOS if B * n < 1_000_000 else R.COMBOS[1::4] + R.COMBOS[4:5], **opt)
    for n in R.DENSE_N:
        for B in (1, 9):
            for nc in (False, True):
                yield from one("dense", "dense", B, n, R.COMBOS, norm0=nc)
    for kind, B, n, opt in T.OPT_SHAPES:
        for base in ("none", "x", "third"):
            for c_out in (1.0, 0.5):
                yield from one(f"options base={base} c_out={c_out}", kind, B, n, R.COMBOS[3:5], base=base, c_out=c_out, **opt)
        for tf in (0.0, 0.5, 1.0):
            yield from one(f"options delta_rows t_frac={tf}", kind, B, n, R.COMBOS[1::2], dr=True, t_frac=tf, base="third", **opt)
        d5 = R.stage_inputs(B, n, 5, DEV)
        dW = torch.tensor(np.float32(R.DELTA ** 0.5), device=DEV) * d5["z"]
        t_dev = torch.tensor([np.float32(R.T0)], device=DEV)
        yield from one("options dW=", kind, B, n, R.COMBOS[1::2], seed=5, base="third", noise="dW", dW=dW, **opt)
        yield from one("options t_dev=", kind, B, n, R.COMBOS[1::2], seed=5, base="third", t=0.9, t_dev=t_dev, **opt)
        if kind == "sgm":
            for proc, strato, lmbd in R.COMBOS[1::2]:
                def inplace(p=proc, s=strato, l=lmbd, o=dict(opt), d=d5):
                    xi = d["x"].clone()
                    return T.run_stage(ops, L, "sgm", p, s, l, d, x=xi, out=xi, **o)
                yield f"stage options in place sgm ({B},{n}) {proc} strato={strato} lmbd={lmbd} {opt}", inplace
    for kind, B, n, opt, path in T.NOISE_CASES:
        for row_base in (0, 4):
            rng = L.PhiloxState(T.SEED, DEV, T.OFFSET, row_base, n)
            step_dev = torch.tensor([T.STEP], dtype=torch.int64, device=DEV)
            tag = f"in-kernel noise, {path}, row_base={row_base}"
            yield from one(tag, kind, B, n, R.COMBOS[1::2], seed=3 * n + B, base="third", noise="rng", rng=rng, rng_step=T.STEP, **opt)
            yield from one(tag + ", step_dev", kind, B, n, R.COMBOS[1::2], seed=3 * n + B, base="third", noise="rng", rng=rng,
                           rng_step=999, step_dev=step_dev, **opt)


def row_cases():
    for B, n in R.row_shapes():
        g = gen(17 * n + B)
        x, k1, k2, k3, k4, a, ad = (torch.randn(B, n, generator=g, device=DEV) for _ in range(7))
        v = (torch.rand(B, n, generator=g, device=DEV) >= 0.5).float() * 2 - 1
        t = R.clamp_time(torch.rand(B, generator=g, device=DEV))
        n0, out, w, tag = x.double().norm(dim=1).float(), torch.cat([a, ad]).contiguous(), 1.0 / B, f"({B},{n})"
        yield "rk4_combine " + tag, lambda: (ops.rk4_combine(nan(B, n), x, k1, k2, k3, k4),)
        yield "rk4_combine rows (shifted k1) " + tag, lambda s=shifted(k1): (ops.rk4_combine(nan(B, n), x, s, k2, k3, k4),)
        yield "rk4_combine norm0 " + tag, lambda: (ops.rk4_combine(nan(B, n), x, k1, k2, k3, k4, norm0=n0),)
        yield "row_norm " + tag, lambda: (T.c_row_norm(L, x),)
        for kind in ("sgm", "sparse"):
            def terms_loss(kind=kind):
                u, cst = T.c_ssm_terms(L, x, v, t, T.sde(L, kind))
                return (u, cst) + T.c_ssm_loss(L, out, u, cst, w)
            yield f"ssm_terms + ssm_loss {kind} " + tag, terms_loss
        yield "ssm_loss_diag " + tag, lambda: T.c_ssm_loss_diag(L, out, v, t, T.sde(L, "sgm"), w)
    for n in (2, 7, 64):
        for B in (1, 9):
            g = gen(n + B)
            G, L_G = R.dense_G(n, device=DEV)
            y, v = torch.randn(B, n, generator=g, device=DEV), torch.randn(B, n, generator=g, device=DEV)
            t = R.clamp_time(torch.rand(B, generator=g, device=DEV))
            yield f"ssm_terms dense ({B},{n})", lambda: T.c_ssm_terms(L, y, v, t, T.sde(L, "dense", G, L_G))


def elementwise_cases():
    st = T.sde(L, "sgm")
    for d in (1, 2, 3, 5, 1024):
        g = gen(d)
        x0, eps = torch.randn(37, d, generator=g, device=DEV), torch.randn(37, d, generator=g, device=DEV)
        t = torch.rand(37, generator=g, device=DEV)
        rng = L.PhiloxState(T.SEED, DEV, T.OFFSET)
        yield f"perturb_vp d={d}", lambda: T.c_perturb_vp(L, x0, st, t, eps)
        yield f"perturb_vp_at eps= d={d}", lambda: (T.c_perturb_vp_at(L, x0, st, t, eps=eps),)
        yield f"perturb_vp_at rng= d={d}", lambda: T.c_perturb_vp_at(L, x0, st, t, rng=rng)
    for B, d in T.SSM_PREP_SHAPES:
        for row_base in (0, 4):
            x0 = torch.randn(B, d, generator=gen(31 * B + d), device=DEV)
            rng = L.PhiloxState(T.SEED, DEV, T.OFFSET, row_base, d)

            def prep():
                ctr = torch.tensor([41], dtype=torch.int64, device=DEV)
                return T.c_ssm_prep(L, x0, st, rng, ctr) + (ctr.float(),)
            yield f"ssm_prep ({B},{d}) row_base={row_base}", prep
    ts = (0.37 + 0.0371 * torch.arange(17, dtype=torch.float64)).float().to(DEV)
    for B in (1, 255, 257, 65541):
        for step in (0, 16, 20):
            for t_add in (0.0, float(np.float32(0.0371 / 2)), float(np.float32(0.0371))):
                def tick(step=step, t_add=t_add):
                    t_dev, s_out = nan(1), nan(B)
                    ops.time_tick(ts, torch.tensor([step], dtype=torch.int64, device=DEV), R.T_END, t_dev, s_out, t_add)
                    return t_dev, s_out
                yield f"time_tick B={B} step={step} t_add={t_add:.5f}", tick
    for n in (1, 1023, 524289):
        g = gen(n)
        a, b, c = (torch.randn(n, generator=g, device=DEV) for _ in range(3))
        yield f"lincomb n={n}", lambda: (ops.lincomb(nan(n), a, 0.5), ops.lincomb(nan(n), a, 0.5, b, -2.0),
                                         ops.lincomb(nan(n), a, 0.5, b, -2.0, c, 1.0 / 3))
    for B, n in ((37, 1), (37, 10), (8193, 10)):
        g = gen(B + n)
        x = torch.randn(B, n, generator=g, device=DEV)
        stop = torch.randint(0, 3, (B,), generator=g, device=DEV, dtype=torch.int32)
        yield f"keep_rows ({B},{n})", lambda: (ops.keep_rows(nan(B, n), x, stop, 1),)
    for n in (4, 7, 4096, 2097156):
        g = gen(n)
        p, gr = torch.randn(n, generator=g, device=DEV) * 0.1, torch.randn(n, generator=g, device=DEV) * 0.01
        m, v = torch.randn(n, generator=g, device=DEV) * 0.01, torch.rand(n, generator=g, device=DEV) * 1e-4
        for body, f in (("vector body" if n % 4 == 0 else "scalar body", lambda x: x.clone()), ("scalar body (shifted)", shifted)):
            for dev_step in (False, True):
                def adam(f=f, dev_step=dev_step):
                    pp, mm, vv = f(p), f(m), f(v)
                    sd = torch.tensor([3], dtype=torch.int64, device=DEV) if dev_step else None
                    ops.adam_step(pp, f(gr), mm, vv, 0 if dev_step else 3, gscale=0.5, step_dev=sd)
                    return pp, mm, vv
                yield f"adam n={n} {body}{', step_dev' if dev_step else ''}", adam
    rng = L.PhiloxState(T.SEED, DEV, T.OFFSET)
    for name, fill in (("fill_normal", ops.fill_normal), ("fill_uniform", ops.fill_uniform)):
        for n in (1, 2, 3, 1025, 1026, 1027, 1028):
            def both(n=n, fill=fill):
                buf = nan(n + 8)
                fill(buf[1:1 + n], rng, 21)                                    # 4-byte aligned: the scalar stores
                return fill(nan(n), rng, 21), buf
            yield f"{name} n={n} aligned and misaligned", both


def bitwise(path):
    t0, lines, bad = time.time(), [], 0
    for cases in (stage_cases(), row_cases(), elementwise_cases()):
        for name, fn in cases:                              # a case runs while its generator is suspended at it: it reads the
            outs = []                                       # generator's variables of that moment
            for h in (PARENT, NEW):
                use(h)
                outs.append(fn())
                torch.cuda.synchronize()
            ok = len(outs[0]) == len(outs[1]) and all(same(a, b) for a, b in zip(*outs))
            bad += not ok
            lines.append(f"{'equal' if ok else 'DIFFERENT':<9} {name}")
            print(lines[-1], flush=True)
    lines.append(f"cases run {len(lines)}, bit-identical to the parent in every output {len(lines) - bad}, different {bad} "
                 f"({time.time() - t0:.0f} s)")
    print(lines[-1])
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    return bad


def timed_cases():
    """(kernel, case, call(library)).  The kernels whose machine code differs from the parent's (profiles/sde_shared/
    asm_vs_parent.txt: k_adam, k_stage_diag_flat, k_stage_sparse_flat) and, though they are the parent's machine code,
    k_stage_rows with norm0, k_rk4_combine_flat, k_ssm_prep and k_ssm_loss_diag, at the two sizes of bench.py's hbm_rooflines
    (4096 x 12288, 65536 x 2; at n = 2 the sparse SDE without norm0 falls back to the row kernel); k_stage_sparse_flat also
    at n = 8, 16, 32 with 2^25 / n rows."""
    st, sp = T.sde(L, "sgm"), T.sde(L, "sparse")
    rng = L.PhiloxState(7, DEV)
    npar = 4023233 + 9 * 3 * 32 * 2                                            # the C4 net's bucket, as hbm_rooflines
    p, g, m, v = (torch.randn(npar, device=DEV) for _ in range(4))
    v.abs_()
    yield "k_adam", f"{npar} parameters", lambda: ops.adam_step(p, g, m, v, step=3, lr=1e-4)
    del p, g, m, v
    stage = lambda out, x, a, s, strato, **kw: ops.sde_stage(out, x, 0.5 if strato else 1.0, x, a, s, L.PROC_REVERSE, strato, 0.5, 1e-3, 0.0,  # noqa: E731
                                                             rng=rng, rng_step=1, **kw)
    for B, n, every in [(4096, 12288, True), (65536, 2, True)] + [((1 << 25) // n, n, False) for n in (8, 16, 32)]:
        x, a, o, y = (torch.randn(B, n, device=DEV) for _ in range(4))
        t, per, n0 = torch.rand(B, device=DEV), torch.empty(B, device=DEV), torch.ones(B, device=DEV)
        step = torch.zeros(1, dtype=torch.int64, device=DEV)
        gs, tag = f"<{R.group_width(n)}>", f"{B} x {n}"
        if every:
            yield "k_stage_diag_flat", tag, lambda: stage(x, x, a, st, False)
            yield "k_rk4_combine_flat", tag, lambda: ops.rk4_combine(o, x, a, y, a, y)
            yield "k_ssm_prep", tag, lambda: L.check(L.lib().msgm_ssm_prep(x.data_ptr(), y.data_ptr(), t.data_ptr(), o.data_ptr(), B, n, st,
                                                                      rng.ptr(), step.data_ptr(), L.stream()), "msgm_ssm_prep")
            B2 = B // 2                                                        # out = [a ; adot] = x: 2 B2 rows; g = o
            yield "k_ssm_loss_diag" + gs, f"{B2} x {n}", lambda: L.check(L.lib().msgm_ssm_loss_diag(
                x.data_ptr(), a.data_ptr(), t.data_ptr(), per.data_ptr(), o.data_ptr(), B2, n, st, 1.0 / B2, L.stream()), "msgm_ssm_loss_diag")
        # without norm0 the sparse SDE runs flat where n % 4 == 0 and n >= 8, else msgm_sde_stage falls back to the row kernel
        yield "k_stage_sparse_flat" if n % 4 == 0 and n >= 8 else "k_stage_rows" + gs, tag + " sparse", lambda: stage(o, x, a, sp, True)
        if every:
            yield "k_stage_rows" + gs, tag + " sgm norm0", lambda: stage(o, x, a, st, False, norm0=n0)
            yield "k_stage_rows" + gs, tag + " sparse norm0", lambda: stage(o, x, a, sp, True, norm0=n0)
        del x, a, o, y


def timing(path):
    ROUNDS, REPS, WARM = 5, 20, 3
    rows = []
    for kernel, case, call in timed_cases():
        def run(h):
            use(h)
            call()
        row = timed_rounds(run, PARENT, [("new", NEW)], ROUNDS, REPS, WARM)
        rows.append(dict(kernel=kernel, case=case, **row))
        print(f"{timing_line(kernel, row)}   {case}", flush=True)
    if path:
        write_timing(path, rows, [], ROUNDS, REPS, WARM)
    return 0


if __name__ == "__main__":
    if TIME:
        sys.exit(timing(timing_args(sys.argv)[0]))
    sys.exit(1 if bitwise(sys.argv[2] if len(sys.argv) > 2 else None) else 0)
