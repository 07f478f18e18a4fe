"""The one-launch sampler loop for dense tensors with 17 <= n <= 30 (msgm_mlp_dense_sde_loop: the contraction of a 32-row tile
on the matrix cores inside k_mlp's sampler-loop mode): routing of the public samplers, the float64 oracle with the composed
path of the same build as the yardstick, the Philox stream, row independence and bounds, kept rows, shard invariance and
graph capture.  An fp32 MFMA sums in another order than the composed path's dense stage, so nothing here compares the two
to the bit: parity of this route is to float64, and bit-equality is asked of the entry against itself."""
import itertools

import pytest
import torch

from conftest import rel_l2
from test_mlp_sde_loop_gpu import DEV, NLR, make_gen, oracle_traj

pytestmark = pytest.mark.gpu

ENTRIES = (("dense", "mlp_dense_sde_loop"), ("xw", "mlp_xw_sde_loop"), ("narrow", "mlp_sde_loop"))


def run_loop(gen, method, x0, N, *, lmbd=0.0, z=None, rng=None, nc=False, keep_all=True, include_t0=True, keep=None,
             workspace=None):
    """ops.mlp_dense_sde_loop as _Run.mlp_loop calls it; returns (final state, trajectory or kept rows or None), on the device."""
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
    ops.mlp_dense_sde_loop(gen.a.kernel_params(), x, base.struct(), method, ts, T / N, lmbd, z=None if z is None else z.to(DEV),
                           rng=rng, norm0=norm0, traj=traj, include_t0=include_t0, keep=keep, kept=kept, workspace=workspace,
                           packed=base.packed_G())
    return x, (traj if keep_all else kept)


def record_all(monkeypatch):
    """Records every call of the three loop entries as (entry, method)."""
    from sdeflow_light_amd import ops
    calls = []
    for tag, name in ENTRIES:
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _t=tag, _r=real, **k: (calls.append((_t, a[3])), _r(*a, **k))[1])
    return calls


# ------------------------------------------------------------------ 1. route
@pytest.mark.parametrize("d,pre,nc", [(17, None, False), (30, NLR, True)], ids=["d17-none", "d30-nlr-nc"])
def test_public_samplers_take_the_dense_loop(monkeypatch, d, pre, nc):
    """Where ops.mlp_dense_sde_loop_preferred says yes each public sampler calls the new entry exactly once and neither old
    one; where the measurement left it false they call none of the three.  The composed functions, noise=, B = 64 and
    d = 31 never reach a loop entry."""
    from sdeflow_light_amd import ops, sde_scheme as SS
    torch.manual_seed(1)
    gen = make_gen("dense", d, pre, out_scale=0.1)
    calls = record_all(monkeypatch)
    B, N = 160, 5
    x0 = torch.randn(B, d, device=DEV)
    kw = dict(num_steps=N, keep_all_samples=True, include_t0=True, norm_correction=nc)
    routed = ops.mlp_dense_sde_loop_preferred(d, pre is not None, gen.base_sde.struct().kind, d, B)
    print(f"dense d={d} pre={pre} B={B}: preferred = {routed}")
    for method, public, composed in (("rk4", SS.rk4_stratonovich_sampler, SS.rk4_stratonovich_composed),
                                     ("heun", SS.heun_sampler, SS.heun_composed),
                                     ("em", SS.euler_maruyama_sampler, None)):
        del calls[:]
        out = public(gen, x0, **kw)
        assert out.shape == (N + 1, B, d) and torch.isfinite(out).all()
        assert calls == ([("dense", method)] if routed else [])
        if composed is not None:
            del calls[:]
            composed(gen, x0, **kw)
            assert calls == []                                  # the composed functions stay composed
    del calls[:]
    SS.rk4_stratonovich_sampler(gen, x0, noise=torch.randn(N, B, d), **kw)       # noise= stays composed
    SS.rk4_stratonovich_sampler(gen, x0[:64], **kw)                               # and so does B <= 64
    SS.heun_sampler(gen, x0[:64], **kw)
    assert calls == []


def test_dense_31_stays_composed(monkeypatch):
    from sdeflow_light_amd import sde_scheme as SS
    torch.manual_seed(2)
    gen = make_gen("dense", 31, None, out_scale=0.1)
    calls = record_all(monkeypatch)
    x0 = torch.randn(160, 31, device=DEV)
    for fn in (SS.rk4_stratonovich_sampler, SS.heun_sampler, SS.euler_maruyama_sampler):
        assert torch.isfinite(fn(gen, x0, num_steps=3, keep_all_samples=True, norm_correction=True)).all()
    assert calls == []


# ------------------------------------------------------------------ 2. float64 yardstick
YARD = [(17, None), (24, NLR), (30, NLR), (30, None)]


@pytest.mark.parametrize("d,pre", YARD, ids=[f"d{d}-{'nlr' if p else 'none'}" for d, p in YARD])
def test_float64_yardstick(d, pre):
    """The narrow loop's rule: truth = the oracle integrators with nets_ref.mlp_forward in float64; the loop may be no
    further from it than 2 x the larger of the composed path of this build (public sampler with noise=z) and the float32
    oracle.  B = 65: three tiles, one live row in the last; 97: four tiles; 160: a 3 / 2 split of tiles across two
    workgroups; every (method, lmbd, norm correction) at those; B = 1000 (many workgroups) with RK4, lmbd 0 and norm
    correction.  Heun and RK4 at N = 4, Euler-Maruyama at N = 6; include_t0 trajectories, explicit z.  The net is the
    untrained one with its output layer scaled by 0.1 (see test_mlp_sde_loop_gpu.test_float64_yardstick).
    Measured on an MI355X (profiles/mlp_dense_sde_loop/parity_measured.txt): the worst ratio per case."""
    from sdeflow_light_amd import sde_scheme as SS
    torch.manual_seed(100 * d + 5)
    kind = "dense"
    gen = make_gen(kind, d, pre, out_scale=0.1)
    public = {"em": SS.euler_maruyama_sampler, "heun": SS.heun_sampler, "rk4": SS.rk4_stratonovich_sampler}
    cases = list(itertools.product((65, 97, 160), (("heun", 4), ("rk4", 4), ("em", 6)), (0.0, 0.5), (False, True)))
    cases.append((1000, ("rk4", 4), 0.0, True))
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


# ------------------------------------------------------------------ 3. the Philox stream
@pytest.mark.parametrize("d,pre,nc", [(30, NLR, True), (17, None, False)], ids=["d30-nlr-nc", "d17-none"])
@pytest.mark.parametrize("method", ["rk4", "heun", "em"])
def test_philox_stream(method, d, pre, nc):
    """The entry with rng= equals, bit for bit, the entry given z[i] = the device fill of RNG_STREAM_DW at offset + i (the
    identity test_sde_paths_gpu uses for dW_out), which carries the float64 bound over to the Philox path; the stream
    advances by N as on the composed path; same state, same bits; a second call draws fresh numbers; the public sampler
    from the same state gives the bits of the route its shape takes."""
    from sdeflow_light_amd import _lib as L, ops, sde_scheme as SS
    torch.manual_seed(3)
    gen = make_gen("dense", d, pre, out_scale=0.1)
    public, composed = {"rk4": (SS.rk4_stratonovich_sampler, SS.rk4_stratonovich_composed),
                        "heun": (SS.heun_sampler, SS.heun_composed),
                        "em": (SS.euler_maruyama_sampler, None)}[method]
    N, B = 5, 160
    x0 = torch.randn(B, d, device=DEV)
    rng = gen.base_sde.philox(DEV)
    st = rng.state.clone()
    seed, offset = int(st[0]), int(st[1])
    kw = dict(num_steps=N, keep_all_samples=True, include_t0=True, norm_correction=nc)

    def loop():
        traj = run_loop(gen, method, x0, N, rng=rng, nc=nc)[1].cpu()
        rng.advance(N)
        return traj

    a = loop()
    off_loop = rng.state.clone()
    assert int(off_loop[1] - st[1]) == N
    z = torch.stack([ops.fill_normal(torch.full((B, d), float("nan"), device=DEV), L.PhiloxState(seed, DEV, offset + i),
                                     L.RNG_STREAM_DW) for i in range(N)])
    assert torch.isfinite(z).all()
    assert torch.equal(run_loop(gen, method, x0, N, z=z, nc=nc)[1].cpu(), a)
    assert a.shape == (N + 1, B, d) and torch.isfinite(a).all()
    b = loop()                                                  # second run: fresh noise
    assert not torch.equal(a, b) and torch.isfinite(b).all()
    rng.state.copy_(st)
    assert torch.equal(loop(), a)                               # same state: the same bits
    if composed is not None:
        rng.state.copy_(st)
        ref = composed(gen, x0, **kw)
        assert torch.equal(rng.state, off_loop)                 # the stream advances by N either way
    else:
        rng.state.copy_(st)
        ref = SS.euler_maruyama_sampler(gen, x0, noise=z, **kw)
    print(f"{method} dense d={d} pre={pre} nc={int(nc)}: loop vs composed on the Philox stream rel-L2 {rel_l2(a, ref):.2e} "
          f"(printed only: the bound is the float64 yardstick's, carried over by the z identity above)")
    rng.state.copy_(st)
    routed = ops.mlp_dense_sde_loop_preferred(d, pre is not None, gen.base_sde.struct().kind, d, B)
    out = public(gen, x0, **kw)
    assert torch.equal(rng.state, off_loop)
    if routed:
        assert torch.equal(out, a)
    elif composed is not None:
        assert torch.equal(out, ref)


# ------------------------------------------------------------------ 4. rows and bounds
def test_rows_are_independent():
    """Changing x0[b] and z[:, b] changes row b of the trajectory and no other: b at both ends of a tile and of the batch."""
    torch.manual_seed(8)
    d, B, N = 29, 70, 3
    gen = make_gen("dense", d, NLR, out_scale=0.1)
    x0, z = torch.randn(B, d), torch.randn(N, B, d)
    _, base = run_loop(gen, "rk4", x0, N, lmbd=0.5, z=z, nc=True)
    assert torch.isfinite(base).all()
    for b in (0, 31, 32, 69):
        x1, z1 = x0.clone(), z.clone()
        x1[b] = torch.randn(d)
        z1[:, b] = torch.randn(N, d)
        _, t1 = run_loop(gen, "rk4", x1, N, lmbd=0.5, z=z1, nc=True)
        others = [r for r in range(B) if r != b]
        assert torch.equal(t1[:, others], base[:, others]), b
        assert not torch.equal(t1[1:, b], base[1:, b]), b


def test_nothing_past_B_is_written_and_kept_rows_match_the_trajectory():
    """x, the trajectory and kept sit in front of a NaN-filled guard that stays NaN (NaN rows behind x, z and norm0 are never
    read: every output is finite); keep= rows at mixed stop indices equal the rows of the full trajectory."""
    from sdeflow_light_amd import ops
    torch.manual_seed(9)
    d, B, N, PAD = 29, 70, 3, 64
    gen = make_gen("dense", d, NLR, out_scale=0.1)
    base = gen.base_sde
    T = base.T_float()
    ts = (torch.linspace(0, 1, N + 1) * T).to(DEV)
    x0, z0 = torch.randn(B, d, device=DEV), torch.randn(N, B, d, device=DEV)
    keep = (torch.arange(B, dtype=torch.int32, device=DEV) % N) + 1
    P, st, packed = gen.a.kernel_params(), base.struct(), base.packed_G()

    def padded(n):
        buf = torch.full((n + PAD * d,), float("nan"), device=DEV)
        return buf, buf[:n]

    xb, x = padded(B * d)
    zb, z = padded(N * B * d)
    nb, norm0 = padded(B)
    tb, traj = padded((N + 1) * B * d)
    kb, kept = padded(B * d)
    wb, ws = padded(3 * B * d)
    x, z, traj, kept = x.view(B, d), z.view(N, B, d), traj.view(N + 1, B, d), kept.view(B, d)
    x.copy_(x0)
    z.copy_(z0)
    norm0.copy_(ops.row_norm(x0))
    traj.zero_()
    kept.zero_()
    ops.mlp_dense_sde_loop(P, x, st, "rk4", ts, T / N, 0.5, z=z, norm0=norm0, traj=traj, include_t0=True, keep=keep, kept=kept,
                           workspace=ws, packed=packed)
    torch.cuda.synchronize()
    x2, traj2, kept2 = x0.clone(), torch.zeros(N + 1, B, d, device=DEV), torch.zeros(B, d, device=DEV)   # exact-size buffers
    ops.mlp_dense_sde_loop(P, x2, st, "rk4", ts, T / N, 0.5, z=z0, norm0=ops.row_norm(x0), traj=traj2, include_t0=True, keep=keep,
                           kept=kept2, packed=packed)
    assert torch.isfinite(x).all() and torch.isfinite(traj[1:]).all() and torch.isfinite(kept).all()
    assert torch.equal(x, x2) and torch.equal(traj, traj2) and torch.equal(kept, kept2)
    for buf, n in ((xb, B * d), (zb, N * B * d), (nb, B), (tb, (N + 1) * B * d), (kb, B * d), (wb, 3 * B * d)):
        assert torch.isnan(buf[n:]).all()
    rows = torch.arange(B, device=DEV)
    assert kept.abs().sum() > 0 and torch.equal(kept, traj[keep.long(), rows])


# ------------------------------------------------------------------ 5. shard invariance
def test_shard_invariance():
    """Rows [0, 96) and [96, 192) as two calls with a shard base draw the numbers of the 192-row call."""
    from sdeflow_light_amd._lib import PhiloxState
    torch.manual_seed(5)
    d = 24
    gen = make_gen("dense", d, NLR, out_scale=0.1)
    x0 = torch.randn(192, d)
    xf, tf = run_loop(gen, "rk4", x0, 3, rng=PhiloxState(11, DEV), nc=True)
    for lo in (0, 96):
        xs, tsh = run_loop(gen, "rk4", x0[lo:lo + 96], 3, rng=PhiloxState(11, DEV, row_base=lo, n=d), nc=True)
        assert torch.equal(xs, xf[lo:lo + 96]) and torch.equal(tsh, tf[:, lo:lo + 96])
    assert torch.isfinite(tf).all() and not torch.equal(tf[:, :96], tf[:, 96:])


# ------------------------------------------------------------------ 6. refusals
def test_refusals_come_before_any_launch():
    from sdeflow_light_amd import ops
    from sdeflow_light_amd._lib import MsgmError
    torch.manual_seed(6)
    ts = torch.linspace(0, 1, 4).to(DEV)
    for d, B in ((30, 64), (31, 160), (16, 160)):              # one workgroup; the extra-wide class; the narrow entry's
        gen = make_gen("dense", d, None)
        x0 = torch.randn(B, d, device=DEV)
        x = x0.clone()
        with pytest.raises(MsgmError, match=r"\(-2\)"):         # MSGM_E_UNSUPPORTED
            ops.mlp_dense_sde_loop(gen.a.kernel_params(), x, gen.base_sde.struct(), "rk4", ts, 1 / 3,
                                   z=torch.randn(3, B, d, device=DEV), packed=gen.base_sde.packed_G())
        torch.cuda.synchronize()
        assert torch.equal(x, x0)
    gen = make_gen("dense", 24, None)
    x0 = torch.randn(160, 24, device=DEV)
    x = x0.clone()
    z = torch.randn(3, 160, 24, device=DEV)
    with pytest.raises(MsgmError, match=r"\(-1\)"):             # MSGM_E_BADARG: no packed tensor
        ops.mlp_dense_sde_loop(gen.a.kernel_params(), x, gen.base_sde.struct(), "rk4", ts, 1 / 3, z=z)
    small = torch.zeros(3 * 160 * 24 - 1, device=DEV)
    with pytest.raises(MsgmError, match=r"\(-3\)"):             # MSGM_E_WORKSPACE
        ops.mlp_dense_sde_loop(gen.a.kernel_params(), x, gen.base_sde.struct(), "rk4", ts, 1 / 3, z=z, workspace=small,
                               packed=gen.base_sde.packed_G())
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and not small.any()


# ------------------------------------------------------------------ 7. graph capture
def test_graph_capture_is_one_kernel_node():
    from sdeflow_light_amd import ops, sde_scheme as SS
    torch.manual_seed(7)
    N, B, d = 4, 97, 17
    gen = make_gen("dense", d, None, out_scale=0.1)
    base = gen.base_sde
    T = base.T_float()
    ts = (torch.linspace(0, 1, N + 1) * T).to(DEV)
    x0 = torch.randn(B, d, device=DEV)
    x = x0.clone()
    norm0 = ops.row_norm(x)
    traj = torch.zeros(N + 1, B, d, device=DEV)
    ws = ops.mlp_dense_sde_loop_workspace(B, d, "rk4", DEV)
    z = torch.randn(N, B, d, device=DEV)
    P, st, packed = gen.a.kernel_params(), base.struct(), base.packed_G()

    def body():
        ops.mlp_dense_sde_loop(P, x, st, "rk4", ts, T / N, 0.0, z=z, norm0=norm0, traj=traj, include_t0=True, workspace=ws,
                               packed=packed)

    graph = SS._capture(body, DEV)
    kinds = ops.graph_node_kinds(graph)
    print(f"captured dense sampler loop = {kinds}")
    assert kinds == {"kernel": 1}, kinds
    x.copy_(x0)
    traj.zero_()
    body()
    eager_x, eager_traj = x.clone(), traj.clone()
    x.copy_(x0)
    traj.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(x, eager_x) and torch.equal(traj, eager_traj)
    assert torch.isfinite(x).all() and not torch.equal(x, x0)
