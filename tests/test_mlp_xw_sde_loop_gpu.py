"""The one-launch sampler loop of the extra-wide MLP class (msgm_mlp_xw_sde_loop, k_mlp_xw's sampler-loop mode: 31 <= d <=
128, SGM and the sparse tensor): routing of the public samplers, bits against the composed path on the Philox stream, the
float64 oracle with the composed path of the same build as the yardstick, row independence and bounds, captures, shard
invariance, refusals and graph capture."""
import itertools

import pytest
import torch

from conftest import rel_l2
from test_mlp_sde_loop_gpu import DEV, NLR, make_gen, oracle_traj

pytestmark = pytest.mark.gpu


def run_loop(gen, method, x0, N, *, lmbd=0.0, z=None, rng=None, nc=False, keep_all=True, include_t0=True, keep=None,
             workspace=None):
    """ops.mlp_xw_sde_loop as _Run.mlp_loop calls it; returns (final state, trajectory or kept rows or None), on the device."""
    from sdeflow_light_amd import ops
    base = gen.base_sde
    T = base.T_float()
    ts = (torch.linspace(0, 1, N + 1) * T).to(DEV)
    x = x0.to(DEV).clone()
    B, d = x.shape
    norm0 = ops.row_norm(x) if nc else None
    traj = kept = None
    if keep_all:
        traj = torch.zeros(N + int(include_t0), B, d, device=DEV)
        if include_t0:
            traj[0].copy_(x)
    elif keep is not None:
        keep = keep.to(torch.int32).to(DEV).contiguous()
        kept = torch.zeros(B, d, device=DEV)
    ops.mlp_xw_sde_loop(gen.a.kernel_params(), x, base.struct(), method, ts, T / N, lmbd, z=None if z is None else z.to(DEV),
                        rng=rng, norm0=norm0, traj=traj, include_t0=include_t0, keep=keep, kept=kept, workspace=workspace)
    return x, (traj if keep_all else kept)


def record_both(monkeypatch, run=True):
    """Records the method of every call of the two loop entries as ("xw" | "narrow", method)."""
    from sdeflow_light_amd import ops
    calls = []
    for tag, name in (("xw", "mlp_xw_sde_loop"), ("narrow", "mlp_sde_loop")):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _t=tag, _r=real, **k: (calls.append((_t, a[3])), _r(*a, **k) if run else None)[1])
    return calls


# ------------------------------------------------------------------ 1. route
ROUTE = [("sparse", 40, NLR, True), ("sgm", 64, None, False)]


@pytest.mark.parametrize("kind,d,pre,nc", ROUTE, ids=[f"{k}-{d}" for k, d, _, _ in ROUTE])
def test_public_samplers_take_the_extra_wide_loop(monkeypatch, kind, d, pre, nc):
    from sdeflow_light_amd import sde_scheme as SS
    torch.manual_seed(1)
    gen = make_gen(kind, d, pre, out_scale=0.1)
    calls = record_both(monkeypatch)
    x0 = torch.randn(160, d, device=DEV)
    kw = dict(num_steps=5, keep_all_samples=True, include_t0=True, norm_correction=nc)
    for method, public, composed in (("rk4", SS.rk4_stratonovich_sampler, SS.rk4_stratonovich_composed),
                                     ("heun", SS.heun_sampler, SS.heun_composed)):
        del calls[:]
        assert torch.isfinite(public(gen, x0, **kw)).all()
        assert calls == [("xw", method)]
        composed(gen, x0, **kw)
        assert calls == [("xw", method)]                        # the composed functions stay composed
    del calls[:]
    assert torch.isfinite(SS.euler_maruyama_sampler(gen, x0, **kw)).all()
    assert calls == ([("xw", "em")] if kind != "sgm" else [])  # the additive SDE's Euler-Maruyama keeps its own kernels
    del calls[:]
    SS.rk4_stratonovich_sampler(gen, x0, noise=torch.randn(5, 160, d), **kw)     # noise= stays composed
    SS.rk4_stratonovich_sampler(gen, x0[:32], **kw)                               # and so does B <= 32
    assert calls == []


@pytest.mark.parametrize("kind,d,pre,nc", [("sgm", 90, None, False), ("sparse", 64, NLR, True), ("sparse", 128, NLR, True)])
def test_widths_measured_slower_stay_composed(monkeypatch, kind, d, pre, nc):
    """Supported by the entry, not routed to it (ops.mlp_xw_sde_loop_preferred; DESIGN §4 has the measurements)."""
    from sdeflow_light_amd import sde_scheme as SS
    torch.manual_seed(2)
    gen = make_gen(kind, d, pre, out_scale=0.1)
    calls = record_both(monkeypatch, run=False)
    x0 = torch.randn(160, d, device=DEV)
    kw = dict(num_steps=3, keep_all_samples=True, norm_correction=nc)
    for fn in (SS.rk4_stratonovich_sampler, SS.heun_sampler, SS.euler_maruyama_sampler):
        assert torch.isfinite(fn(gen, x0, **kw)).all()
    assert calls == []


# ------------------------------------------------------------------ 2. bits against the composed path, Philox stream
BITS = [("sgm", 31, None, False), ("sgm", 64, None, False), ("sgm", 128, None, False), ("sgm", 128, NLR, False),
        ("sparse", 40, NLR, False), ("sparse", 40, NLR, True), ("sparse", 128, NLR, True)]


@pytest.mark.parametrize("kind,d,pre,nc", BITS, ids=[f"{k}-{d}-{'nlr' if p else 'none'}-nc{int(n)}" for k, d, p, n in BITS])
@pytest.mark.parametrize("method", ["rk4", "heun"])
def test_loop_against_composed_on_the_philox_stream(method, kind, d, pre, nc):
    """Same stream state: the loop's trajectory equals the composed path's bit for bit wherever no norm correction is applied
    (the forward phases are k_mlp_xw<FWD>'s, the stage arithmetic sde_stage.h's); under norm correction the row sum is taken
    in another order and the two agree to rel-L2 2e-6, the narrow loop's bound.  The loop is called as _Run.mlp_loop calls it
    (not every width is routed to it); the public sampler gives the bits of the route its shape takes."""
    from sdeflow_light_amd import ops, sde_scheme as SS
    torch.manual_seed(3)
    gen = make_gen(kind, d, pre, out_scale=0.1)
    public, composed = {"rk4": (SS.rk4_stratonovich_sampler, SS.rk4_stratonovich_composed),
                        "heun": (SS.heun_sampler, SS.heun_composed)}[method]
    N, B = 5, 160
    x0 = torch.randn(B, d, device=DEV)
    rng = gen.base_sde.philox(DEV)
    st = rng.state.clone()
    kw = dict(num_steps=N, keep_all_samples=True, include_t0=True, norm_correction=nc)

    def loop():
        traj = run_loop(gen, method, x0, N, rng=rng, nc=nc)[1].cpu()
        rng.advance(N)
        return traj

    a = loop()
    off_loop = rng.state.clone()
    rng.state.copy_(st)
    ref = composed(gen, x0, **kw)
    assert torch.equal(rng.state, off_loop)                     # the stream advances by N either way
    assert int(off_loop[1] - st[1]) == N
    e = rel_l2(a, ref)
    nbad = int((a != ref).sum())
    print(f"{method} {kind} d={d} pre={pre} nc={int(nc)}: loop vs composed on the Philox stream rel-L2 {e:.2e}, "
          f"{nbad} of {a.numel()} elements differ ({'bound 2e-6' if nc else 'must be equal'})")
    assert a.shape == ref.shape == (N + 1, B, d) and torch.isfinite(ref).all()
    if nc:
        assert e <= 2e-6
    else:
        assert torch.equal(a, ref)
    b = loop()                                                  # second run: fresh noise
    assert not torch.equal(a, b) and torch.isfinite(b).all()
    rng.state.copy_(st)
    assert torch.equal(loop(), a)                               # same state: the same bits
    rng.state.copy_(st)
    routed = ops.mlp_xw_sde_loop_preferred(d, pre is not None, gen.base_sde.struct().kind, d, B)
    assert torch.equal(public(gen, x0, **kw), a if routed else ref)
    assert torch.equal(rng.state, off_loop)


# ------------------------------------------------------------------ 3. float64 yardstick
YARD = [(31, None, "sgm"), (31, NLR, "sparse"), (33, None, "sparse"), (48, NLR, "sparse"), (64, NLR, "sgm"), (65, None, "sparse"),
        (127, NLR, "sparse"), (128, None, "sparse"), (128, NLR, "sgm"), (128, NLR, "sparse")]
# 768 tiles on the 256 workgroups the entry launches (min(tiles / 2, 256)): a third sweep for every one, the last tile ragged
B_THREE_SWEEPS = 32 * 767 + 7


@pytest.mark.parametrize("d,pre,kind", YARD, ids=[f"d{d}-{'nlr' if p else 'none'}-{k}" for d, p, k in YARD])
def test_float64_yardstick(d, pre, kind):
    """The narrow loop's rule: truth = the oracle integrators with nets_ref.mlp_forward in float64; the loop may be no
    further from it than 2 x the larger of the composed path of this build (public sampler with noise=z) and the float32
    oracle.  B = 33: a second tile with one live row; 65: three tiles in one workgroup; 160: a 3 / 2 split; every (method,
    lmbd, norm correction) at those; B_THREE_SWEEPS with RK4, lmbd 0.5 and (sparse) norm correction.  Heun and RK4 at N = 4,
    Euler-Maruyama at N = 6 for the sparse tensor.  The net is the untrained one with its output layer scaled by 0.1."""
    from sdeflow_light_amd import sde_scheme as SS
    torch.manual_seed(100 * d + len(kind))
    gen = make_gen(kind, d, pre, out_scale=0.1)
    msgm = kind != "sgm"
    public = {"em": SS.euler_maruyama_sampler, "heun": SS.heun_sampler, "rk4": SS.rk4_stratonovich_sampler}
    methods = [("heun", 4), ("rk4", 4)] + ([("em", 6)] if msgm else [])
    cases = list(itertools.product((33, 65, 160), methods, (0.0, 0.5), (False, True) if msgm else (False,)))
    cases.append((B_THREE_SWEEPS, ("rk4", 4), 0.5, msgm))
    worst = 0.0
    for B, (method, N), lmbd, nc in cases:
        x0, z = torch.randn(B, d), torch.randn(N, B, d)
        truth = oracle_traj(gen, kind, pre, method, x0, z, lmbd, nc, torch.float64)
        assert torch.isfinite(truth).all()
        e32 = rel_l2(oracle_traj(gen, kind, pre, method, x0, z, lmbd, nc, torch.float32), truth)
        comp = public[method](gen, x0.to(DEV), num_steps=N, lmbd=lmbd, keep_all_samples=True, include_t0=True,
                              norm_correction=nc, noise=z)
        ec = rel_l2(comp, truth)
        _, traj = run_loop(gen, method, x0, N, lmbd=lmbd, z=z, nc=nc)
        el = rel_l2(traj.cpu(), truth)
        print(f"yardstick d={d} pre={pre} {kind} B={B} {method} N={N} lmbd={lmbd} nc={int(nc)}: "
              f"loop {el:.3e} | composed {ec:.3e} | float32 oracle {e32:.3e}  (vs float64)")
        worst = max(worst, el / max(ec, e32))
        assert torch.isfinite(traj).all()
        assert el <= 2.0 * max(ec, e32), (B, method, lmbd, nc, el, ec, e32)
    print(f"yardstick d={d} pre={pre} {kind}: worst loop / max(composed, float32 oracle) = {worst:.2f}")


# ------------------------------------------------------------------ 4. rows are independent, nothing past B is touched
@pytest.mark.parametrize("method,N", [("rk4", 3), ("heun", 3), ("em", 3)])
def test_repeated_block_gives_equal_copies(method, N):
    """One 32-row block five times, the last copy cut to 23 rows: five tiles on two workgroups, the last one ragged."""
    torch.manual_seed(8)
    d, B = 40, 151
    gen = make_gen("sparse", d, NLR, out_scale=0.1)
    blk, zb = torch.randn(32, d), torch.randn(N, 32, d)
    x, traj = run_loop(gen, method, blk.repeat(5, 1)[:B], N, z=zb.repeat(1, 5, 1)[:, :B].contiguous(), nc=True)
    assert torch.isfinite(traj).all() and not torch.equal(traj[-1], traj[0])
    for k in range(1, 5):
        n = min(32, B - 32 * k)
        assert torch.equal(traj[:, 32 * k:32 * k + n], traj[:, :n]), k
    assert torch.equal(x, traj[-1])


def test_nothing_past_B_is_read_or_written():
    """NaN rows behind x, z and norm0; a sentinel behind x, the trajectory, kept and the workspace."""
    from sdeflow_light_amd import ops
    torch.manual_seed(9)
    d, B, N, PAD = 40, 70, 3, 64
    gen = make_gen("sparse", d, NLR, out_scale=0.1)
    base = gen.base_sde
    T = base.T_float()
    ts = (torch.linspace(0, 1, N + 1) * T).to(DEV)
    x0, z0 = torch.randn(B, d, device=DEV), torch.randn(N, B, d, device=DEV)
    keep = (torch.arange(B, dtype=torch.int32, device=DEV) % N) + 1
    P, st = gen.a.kernel_params(), base.struct()

    def padded(n, fill):
        buf = torch.full((n + PAD * d,), fill, device=DEV)
        return buf, buf[:n]

    SENT = 12345.0
    xb, x = padded(B * d, float("nan"))
    zb, z = padded(N * B * d, float("nan"))
    nb, norm0 = padded(B, float("nan"))
    tb, traj = padded((N + 1) * B * d, SENT)
    kb, kept = padded(B * d, SENT)
    wb, ws = padded(3 * B * d, SENT)
    x, z, traj, kept = x.view(B, d), z.view(N, B, d), traj.view(N + 1, B, d), kept.view(B, d)
    x.copy_(x0)
    z.copy_(z0)
    norm0.copy_(ops.row_norm(x0))
    traj.zero_()
    kept.zero_()
    ops.mlp_xw_sde_loop(P, x, st, "rk4", ts, T / N, 0.5, z=z, norm0=norm0, traj=traj, include_t0=True, keep=keep, kept=kept,
                        workspace=ws)
    torch.cuda.synchronize()
    # the same call on exact-size buffers
    x2, traj2, kept2 = x0.clone(), torch.zeros(N + 1, B, d, device=DEV), torch.zeros(B, d, device=DEV)
    ops.mlp_xw_sde_loop(P, x2, st, "rk4", ts, T / N, 0.5, z=z0, norm0=ops.row_norm(x0), traj=traj2, include_t0=True, keep=keep,
                        kept=kept2)
    assert torch.isfinite(x).all() and torch.isfinite(traj).all() and torch.isfinite(kept).all()
    assert torch.equal(x, x2) and torch.equal(traj, traj2) and torch.equal(kept, kept2)
    assert kept.abs().sum() > 0 and torch.equal(kept[0], traj[1, 0]) and torch.equal(kept[2], traj[3, 2])
    assert torch.isnan(xb[B * d:]).all() and torch.isnan(zb[N * B * d:]).all() and torch.isnan(nb[B:]).all()
    for buf, n in ((tb, (N + 1) * B * d), (kb, B * d), (wb, 3 * B * d)):
        assert (buf[n:] == SENT).all()


# ------------------------------------------------------------------ 5. captures
def test_final_state_alone_and_kept_rows_against_composed():
    from sdeflow_light_amd import sde_scheme as SS
    torch.manual_seed(10)
    d, B, N = 64, 160, 5
    gen = make_gen("sgm", d, None, out_scale=0.1)
    x0 = torch.randn(B, d, device=DEV)
    rng = gen.base_sde.philox(DEV)
    st = rng.state.clone()
    full = SS.heun_composed(gen, x0, num_steps=N, keep_all_samples=True, include_t0=False)
    rng.state.copy_(st)
    last = SS.heun_sampler(gen, x0, num_steps=N, keep_all_samples=False)
    assert last.shape == (B, d) and torch.equal(last, full[-1])
    x, none = run_loop(gen, "heun", x0, N, z=torch.randn(N, B, d), keep_all=False)
    assert none is None and torch.isfinite(x).all()
    for inc in (False, True):
        idx = (torch.arange(B) % N) + int(inc)                  # stop indices among the rows the loop writes
        rng.state.copy_(st)
        a = SS.rk4_stratonovich_sampler(gen, x0, num_steps=N, keep_all_samples=False, samplesToKeep=idx, include_t0=inc)
        rng.state.copy_(st)
        b = SS.rk4_stratonovich_composed(gen, x0, num_steps=N, keep_all_samples=False, samplesToKeep=idx, include_t0=inc)
        assert a.shape == (B, d) and torch.isfinite(b).all() and a.abs().sum() > 0
        assert torch.equal(a, b), inc


# ------------------------------------------------------------------ 6. shard invariance
def test_shard_invariance():
    """Rows [0, 64) and [64, 128) as two calls with a shard base draw the numbers of the 128-row call."""
    from sdeflow_light_amd._lib import PhiloxState
    torch.manual_seed(5)
    d = 40
    gen = make_gen("sparse", d, NLR, out_scale=0.1)
    x0 = torch.randn(128, d)
    xf, tf = run_loop(gen, "rk4", x0, 3, rng=PhiloxState(11, DEV), nc=True)
    for lo in (0, 64):
        xs, tsh = run_loop(gen, "rk4", x0[lo:lo + 64], 3, rng=PhiloxState(11, DEV, row_base=lo, n=d), nc=True)
        assert torch.equal(xs, xf[lo:lo + 64]) and torch.equal(tsh, tf[:, lo:lo + 64])
    assert torch.isfinite(tf).all() and not torch.equal(tf[:, :64], tf[:, 64:])


# ------------------------------------------------------------------ 7. refusals
def test_refusals_come_before_any_launch():
    from sdeflow_light_amd import ops
    from sdeflow_light_amd._lib import MsgmError
    torch.manual_seed(6)
    for d, pre, B in ((30, NLR, 64), (40, None, 32)):           # the wide class (the narrow entry's); one tile
        gen = make_gen("sgm", d, pre)
        x0 = torch.randn(B, d, device=DEV)
        x = x0.clone()
        with pytest.raises(MsgmError, match=r"\(-2\)"):
            ops.mlp_xw_sde_loop(gen.a.kernel_params(), x, gen.base_sde.struct(), "rk4", torch.linspace(0, 1, 4).to(DEV), 1 / 3,
                                z=torch.randn(3, B, d, device=DEV))
        torch.cuda.synchronize()
        assert torch.equal(x, x0)
    gen = make_gen("sgm", 40, None)
    x0 = torch.randn(64, 40, device=DEV)
    x = x0.clone()
    small = torch.zeros(3 * 64 * 40 - 1, device=DEV)
    with pytest.raises(MsgmError, match=r"\(-3\)"):             # MSGM_E_WORKSPACE
        ops.mlp_xw_sde_loop(gen.a.kernel_params(), x, gen.base_sde.struct(), "rk4", torch.linspace(0, 1, 4).to(DEV), 1 / 3,
                            z=torch.randn(3, 64, 40, device=DEV), workspace=small)
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and not small.any()


# ------------------------------------------------------------------ 8. graph capture
def test_graph_capture_is_one_kernel_chain():
    from sdeflow_light_amd import ops, sde_scheme as SS
    torch.manual_seed(7)
    N, B, d = 4, 160, 40
    gen = make_gen("sparse", d, NLR, out_scale=0.1)
    base = gen.base_sde
    T = base.T_float()
    ts = (torch.linspace(0, 1, N + 1) * T).to(DEV)
    x0 = torch.randn(B, d, device=DEV)
    x = x0.clone()
    norm0 = ops.row_norm(x)
    traj = torch.zeros(N + 1, B, d, device=DEV)
    ws = ops.mlp_xw_sde_loop_workspace(B, d, "rk4", DEV)
    rng = base.philox(DEV)
    P, st = gen.a.kernel_params(), base.struct()

    def body():
        ops.mlp_xw_sde_loop(P, x, st, "rk4", ts, T / N, 0.0, rng=rng, norm0=norm0, traj=traj, include_t0=True, workspace=ws)
        rng.advance(N)

    graph = SS._capture(body, DEV)
    kinds = ops.graph_node_kinds(graph)
    print(f"captured extra-wide sampler loop = {kinds}")
    assert set(kinds) == {"kernel"}, kinds
    state = rng.state.clone()
    x.copy_(x0)
    traj.zero_()
    body()
    eager_x, eager_traj, after = x.clone(), traj.clone(), rng.state.clone()
    rng.state.copy_(state)
    x.copy_(x0)
    traj.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(x, eager_x) and torch.equal(traj, eager_traj) and torch.equal(rng.state, after)
    assert torch.isfinite(x).all() and not torch.equal(x, x0)
