"""The one-launch forward perturbation of the multiplicative SDE (csrc/sde_forward_kernels.hip, msgm_forward_perturb)
against the composed route it replaces (sde_scheme.msgm_forward_perturb_composed: index kernel, nsf RK4 steps of four
stage launches, a combine and a masked capture each, then the short step of the rows with k = 0).

Every comparison with the composed route is BITWISE (torch.equal): both routes evaluate the functions of
csrc/sde_stage.h in the same order under -ffp-contract=off.  The kernel's output buffer is pre-filled with NaN and
asserted finite over its whole extent first; the ops wrapper allocates its output itself, so the parity cases call the
C ABI on their own buffer and one assertion per case ties the wrapper to it.

Row times.  The times of every case contain, by construction, t_epsilon, a value below T / nsf (k = 0), exact grid
points i T / nsf, T itself (k = nsf) and random values.  A case with fewer rows than that list is run as several calls
that go through the list B rows at a time (the last call is filled up with random times), and the assertion that
k = 0, k = nsf and an interior k occur is made over the calls of the case.  nsf = 1 has the indices 0 and 1 only:
there the interior index does not exist and is not asked for.

Shape -> kernel (launch conditions of msgm_forward_perturb):
  sparse n <= 256                 k_forward_perturb_sparse<4, lane groups>: (1,1) one lane; (5,3) (5,6) ragged chunks,
                                  n % 4 != 0: scalar loads, per-element Philox; (33,8) (33,12) (67,36): float4 loads,
                                  Philox quads, 2 / 4 / 16 lanes per row, rows of one wave stopping at different k,
                                  more than one workgroup; (2,256): 64 lanes, the regime's last n
  sparse 256 < n <= 4096          k_forward_perturb_sparse<4, workgroup>: (2,257) the first n, scalar body, a ragged last
                                  chunk; (3,1024); (2,4096) 1024 threads, the form's last n
  sparse 4096 < n <= 12288        k_forward_perturb_sparse<16, workgroup>: (2,4100) the first n, a ragged last chunk;
                                  (3,12288) the supported bound (768 threads x 16 registers per array)
  dense n <= 16 / n <= 64         k_forward_perturb_dense<G in LDS> n 2, 4, 7, 16; <G through L2> n 17, 64; B 1 and 9
"""
import ctypes

import pytest
import torch

import sde_stage_ref as R
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
T_END, T_EPS = 1.0, 1e-3


@pytest.fixture(scope="module")
def ops():
    from sdeflow_light_amd import ops as _ops
    _ops.lib()
    return _ops


@pytest.fixture(scope="module")
def L():
    from sdeflow_light_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def SS():
    from sdeflow_light_amd import sde_scheme
    return sde_scheme


def Tp():
    return torch.nn.Parameter(torch.FloatTensor([T_END]), requires_grad=False)


_BASES = {}


def make_base(kind, n, nsf):
    """MSGMsde on the device, one per (kind, n, nsf); the dense tensor as tests/test_sde_paths_gpu.py::test_stage_dense has it."""
    from sdeflow_light_amd.SDEs import MSGMsde
    key = (kind, n, nsf)
    if key not in _BASES:
        g = torch.Generator().manual_seed(n)
        G = R.dense_G(n)[0] if kind == "dense" else None
        _BASES[key] = MSGMsde(torch.randn(64, n, generator=g), beta_min=R.B0, beta_max=R.B1, t_epsilon=T_EPS, T=Tp(),
                              num_steps_forward=nsf, device=DEV, denseTensor=(kind == "dense"), norm_map="log", G=G).to(DEV)
    return _BASES[key]


def time_pool(nsf, gen):
    """The row times every case must see (module docstring), as an fp32 tensor."""
    grid = sorted({1, nsf // 2, nsf - 1} - {0, nsf})
    fixed = [T_EPS, 0.4 * T_END / nsf] + [i * T_END / nsf for i in grid] + [T_END]
    return torch.cat([torch.tensor(fixed, dtype=torch.float32), torch.rand(3, generator=gen) * T_END])


def time_rounds(B, nsf, seed):
    """Row-time vectors of B rows each that together go through time_pool(nsf)."""
    gen = torch.Generator().manual_seed(seed)
    pool = time_pool(nsf, gen)
    rounds = []
    for i in range(0, max(len(pool), 1), B):
        t = pool[i:i + B]
        if len(t) < B:
            t = torch.cat([t, torch.rand(B - len(t), generator=gen) * T_END])
        rounds.append(t.clamp(min=T_EPS).to(DEV))
    return rounds


def c_forward_perturb(L, SS, base, x0, t, zm=None, zs=None, rng=None, want_k=True):
    """msgm_forward_perturb through the C ABI on a NaN-filled y (asserted finite everywhere) -> (y, k)."""
    B, n = x0.shape
    nsf = base.num_steps_forward
    ts, delta = SS._forward_grid(base, nsf, x0.device)
    y = torch.full((B, n), float("nan"), device=DEV)
    k = torch.full((B,), -7, dtype=torch.int32, device=DEV) if want_k else None
    st = base.struct()
    L.check(L.lib().msgm_forward_perturb(L.ptr(x0), L.ptr(t), L.ptr(y), L.ptr(k), B, n, st, nsf, L.ptr(ts), float(delta),
                                         float(delta ** 0.5), float(delta * 0.5), float(delta * 1.0), L.ptr(zm), L.ptr(zs),
                                         None if rng is None else rng.ptr(), L.stream()), "msgm_forward_perturb")
    assert bool(torch.isfinite(y).all()), "the kernel left part of y unwritten (or not finite)"
    return y, k


def parity_case(ops, L, SS, kind, B, n, nsf):
    """Kernel vs composed route on injected noise and on Philox draws from the same stream state, bitwise."""
    base = make_base(kind, n, nsf)
    assert ops.forward_perturb_supported(base.kind, n)
    gen = torch.Generator().manual_seed(1000 * n + 10 * B + nsf)
    seen = set()
    for r, t in enumerate(time_rounds(B, nsf, 7 * n + B + nsf)):
        x0 = (torch.randn(B, n, generator=gen) * 1.5).to(DEV)
        zm, zs = torch.randn(nsf, B, n, generator=gen).to(DEV), torch.randn(B, n, generator=gen).to(DEV)
        k_ref = ops.forward_step_index(t, nsf, T_END)
        seen |= set(k_ref.tolist())
        # injected noise
        want = SS.msgm_forward_perturb_composed(base, t, x0, zm, zs)
        got, k = c_forward_perturb(L, SS, base, x0, t, zm, zs)
        assert torch.equal(k, k_ref)
        assert torch.equal(got, want), (kind, B, n, nsf, r, "injected", float((got - want).abs().max()))
        assert torch.equal(ops.forward_perturb(x0, t, base.struct(), nsf, *SS._forward_grid(base, nsf, x0.device), z_main=zm,
                                               z_short=zs), got)
        # Philox: composed, the kernel on its own buffer, and the public function, each from the same stream state
        base.rng = L.PhiloxState(4242 + r, DEV, offset=5)
        s0 = base.rng.state.clone()
        want = SS.msgm_forward_perturb_composed(base, t, x0)
        s_composed = base.rng.state.clone()
        base.rng.state.copy_(s0)
        got, _ = c_forward_perturb(L, SS, base, x0, t, rng=base.rng, want_k=False)
        assert torch.equal(base.rng.state, s0)                       # the C entry reads the stream, the caller advances it
        assert torch.equal(got, want), (kind, B, n, nsf, r, "philox", float((got - want).abs().max()))
        got2 = SS.msgm_forward_perturb(base, t, x0)
        assert torch.equal(got2, want)
        assert torch.equal(base.rng.state, s_composed)
        assert int(s_composed[1]) - int(s0[1]) == 2 * nsf + 2 and torch.equal(s_composed[[0, 2, 3]], s0[[0, 2, 3]])
        # mixed: main steps injected, the short step drawn
        base.rng.state.copy_(s0)
        want = SS.msgm_forward_perturb_composed(base, t, x0, zm, None)
        base.rng.state.copy_(s0)
        assert torch.equal(c_forward_perturb(L, SS, base, x0, t, zm, None, rng=base.rng, want_k=False)[0], want)
    assert 0 in seen and nsf in seen, seen
    if nsf > 1:
        assert any(0 < k < nsf for k in seen), seen


SPARSE_SMALL = [(1, 1), (5, 3), (5, 6), (33, 8), (33, 12), (67, 36)]
SPARSE_LONG = [(2, 256), (2, 257), (3, 1024), (2, 4096), (2, 4100), (3, 12288)]


@pytest.mark.parametrize("nsf", [1, 4, 16])
@pytest.mark.parametrize("B,n", SPARSE_SMALL)
def test_sparse_small_bitwise_equals_composed(ops, L, SS, B, n, nsf):
    parity_case(ops, L, SS, "sparse", B, n, nsf)


@pytest.mark.parametrize("B,n", SPARSE_LONG)
def test_sparse_long_bitwise_equals_composed(ops, L, SS, B, n):
    parity_case(ops, L, SS, "sparse", B, n, 4)


@pytest.mark.parametrize("nsf", [1, 4, 16])
@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("n", [2, 4, 7, 16, 17, 64])
def test_dense_bitwise_equals_composed(ops, L, SS, n, B, nsf):
    parity_case(ops, L, SS, "dense", B, n, nsf)


@pytest.mark.parametrize("tag,kind,n", [("sp", "sparse", 6), ("dn", "dense", 4)])
def test_golden_g08(ops, SS, tag, kind, n):
    """SDE.sample_scheme as the reference recorded it (g08), through ops.forward_perturb directly; the bound is the one
    tests/test_host_gpu.py::test_msgm_forward_perturb_golden uses for the same data."""
    from sdeflow_light_amd.SDEs import MSGMsde
    g = load_golden("g08_sample_scheme")
    base = MSGMsde(torch.randn(64, n), T=Tp(), num_steps_forward=4, device=DEV, denseTensor=(kind == "dense"),
                   norm_map="log", G=g.get("dn_G") if kind == "dense" else None).to(DEV)
    ts, delta = SS._forward_grid(base, 4, torch.device(DEV, torch.cuda.current_device()))
    k = torch.full((12,), -7, dtype=torch.int32, device=DEV)
    y = ops.forward_perturb(g[f"{tag}_x0"].to(DEV), g[f"{tag}_t"].to(DEV), base.struct(), 4, ts, delta,
                            z_main=g[f"{tag}_z_main"].to(DEV), z_short=g[f"{tag}_z_short"].to(DEV), k_out=k)
    assert torch.equal(k.cpu(), g[f"{tag}_k"])
    e = rel_l2(y.cpu(), g[f"{tag}_y"])
    print(f"g08 {tag}: rel-L2 {e:.2e}")
    assert e <= 1e-4


@pytest.mark.parametrize("n", [8, 6])
def test_shard_invariance(ops, L, SS, n):
    """Rows [0, 32) and [32, 64) as two calls whose Philox states carry the shard base draw what the 64-row call draws."""
    nsf = 4
    base = make_base("sparse", n, nsf)
    gen = torch.Generator().manual_seed(n)
    x0 = torch.randn(64, n, generator=gen).to(DEV)
    t = torch.cat([time_pool(nsf, gen), torch.rand(64, generator=gen)])[:64].clamp(min=T_EPS).to(DEV)
    grid = SS._forward_grid(base, nsf, x0.device)
    whole = ops.forward_perturb(x0, t, base.struct(), nsf, *grid, rng=L.PhiloxState(99, DEV, offset=3))
    parts = [ops.forward_perturb(x0[b:b + 32].contiguous(), t[b:b + 32].contiguous(), base.struct(), nsf, *grid,
                                 rng=L.PhiloxState(99, DEV, offset=3, row_base=b, n=n)) for b in (0, 32)]
    assert bool(torch.isfinite(whole).all()) and torch.equal(torch.cat(parts), whole)


def _recorded(monkeypatch, ops):
    calls = []
    real = ops.forward_perturb

    def rec(*a, **kw):
        calls.append(a[0].shape)
        return real(*a, **kw)
    monkeypatch.setattr(ops, "forward_perturb", rec)
    return calls


def test_routing(ops, L, SS, monkeypatch):
    calls = _recorded(monkeypatch, ops)
    nsf = 4
    base = make_base("sparse", 8, nsf)
    gen = torch.Generator().manual_seed(0)
    x0, t = torch.randn(33, 8, generator=gen).to(DEV), (torch.rand(33, generator=gen) * T_END).clamp(min=T_EPS).to(DEV)
    zm, zs = torch.randn(nsf, 33, 8, generator=gen).to(DEV), torch.randn(33, 8, generator=gen).to(DEV)
    want = SS.msgm_forward_perturb_composed(base, t, x0, zm, zs)
    assert calls == []
    assert torch.equal(SS.msgm_forward_perturb(base, t, x0, zm, zs), want) and len(calls) == 1
    base.rng = L.PhiloxState(5, DEV)
    SS.msgm_forward_perturb(base, t.view(-1, 1), x0)                     # the Philox route and a (B,1) time column
    assert len(calls) == 2
    with monkeypatch.context() as m:
        m.setattr(ops, "forward_perturb_supported", lambda kind, n: False)
        assert torch.equal(SS.msgm_forward_perturb(base, t, x0, zm, zs), want) and len(calls) == 2
    # a row past the bound (and one past 4096 that is no multiple of 4) keeps the composed route
    for n in (12292, 4099):
        big = make_base("sparse", n, 1)
        assert not ops.forward_perturb_supported(big.kind, n)
        xb, tb = torch.randn(1, n, generator=gen).to(DEV), torch.tensor([0.7], device=DEV)
        zb, zsb = torch.randn(1, 1, n, generator=gen).to(DEV), torch.randn(1, n, generator=gen).to(DEV)
        got = SS.msgm_forward_perturb(big, tb, xb, zb, zsb)
        assert len(calls) == 2 and bool(torch.isfinite(got).all())
        assert torch.equal(got, SS.msgm_forward_perturb_composed(big, tb, xb, zb, zsb))
    assert ops.forward_perturb_supported(L.SDE_MSGM_SPARSE, 12288) and ops.forward_perturb_supported(L.SDE_MSGM_DENSE, 64)
    assert not ops.forward_perturb_supported(L.SDE_SGM, 8) and not ops.forward_perturb_supported(L.SDE_MSGM_DENSE, 65)


def test_c_entry_refusals(ops, L, SS):
    BADARG = -1
    nsf = 4
    lib = L.lib()

    def rc(st, x0, t, y, n, zm, zs, rng, ts):
        B = x0.shape[0]
        return lib.msgm_forward_perturb(L.ptr(x0), L.ptr(t), L.ptr(y), None, B, n, st, nsf, L.ptr(ts), 0.25, 0.5, 0.125, 0.25,
                                        L.ptr(zm), L.ptr(zs), None if rng is None else rng.ptr(), L.stream())

    ts = (torch.linspace(0, 1, nsf + 1) * T_END).to(DEV)
    rng = L.PhiloxState(1, DEV)
    t = torch.full((2,), 0.5, device=DEV)

    def bufs(n):
        return torch.zeros(2, n, device=DEV), torch.zeros(2, n, device=DEV), torch.zeros(nsf, 2, n, device=DEV)

    x, y, zm = bufs(8)
    sparse = L.sde_struct(L.SDE_MSGM_SPARSE, R.B0, R.B1, T_END, T_EPS)
    assert rc(sparse, x, t, y, 8, zm, x, None, ts) == L.MSGM_OK
    assert rc(L.sde_struct(L.SDE_SGM, R.B0, R.B1, T_END, T_EPS), x, t, y, 8, zm, x, rng, ts) == L.MSGM_E_UNSUPPORTED
    assert rc(sparse, x, t, x, 8, zm, x, rng, ts) == BADARG                       # y == x0: the entry cannot work in place
    assert rc(sparse, x, t, y, 8, None, None, None, ts) == BADARG                 # neither noise nor a stream
    assert rc(sparse, x, t, y, 8, zm, None, None, ts) == BADARG                   # the short step has neither
    assert rc(sparse, x, t, y, 8, zm, x, rng, None) == BADARG                     # no time grid
    G65, LG65 = torch.zeros(65, 65, 65, device=DEV), torch.zeros(65, 65, device=DEV)
    x, y, zm = bufs(65)
    assert rc(L.sde_struct(L.SDE_MSGM_DENSE, R.B0, R.B1, T_END, T_EPS, G65, LG65), x, t, y, 65, zm, x, rng, ts) == L.MSGM_E_UNSUPPORTED
    assert rc(L.sde_struct(L.SDE_MSGM_DENSE, R.B0, R.B1, T_END, T_EPS), x, t, y, 65, zm, x, rng, ts) == BADARG   # no tensor
    x, y, zm = bufs(12292)
    assert rc(sparse, x, t, y, 12292, zm, x, rng, ts) == L.MSGM_E_UNSUPPORTED
    torch.cuda.synchronize()


def test_repeatable(ops, L, SS):
    """Two calls from the same stream state give identical bits."""
    for kind, B, n in (("sparse", 67, 36), ("sparse", 3, 1024), ("dense", 9, 7)):
        nsf = 4
        base = make_base(kind, n, nsf)
        gen = torch.Generator().manual_seed(n)
        x0 = torch.randn(B, n, generator=gen).to(DEV)
        t = time_rounds(B, nsf, n)[0]
        rng = L.PhiloxState(31, DEV, offset=9)
        grid = SS._forward_grid(base, nsf, x0.device)
        a = ops.forward_perturb(x0, t, base.struct(), nsf, *grid, rng=rng)
        b = ops.forward_perturb(x0, t, base.struct(), nsf, *grid, rng=rng)
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


def _gen(net, n, nsf):
    from sdeflow_light_amd.SDEs import MSGMsde, PluginReverseSDE
    T = Tp()
    base = MSGMsde(torch.randn(64, n), beta_min=R.B0, beta_max=R.B1, t_epsilon=T_EPS, T=T, num_steps_forward=nsf, device=DEV,
                   denseTensor=False, norm_map="log")
    return PluginReverseSDE(base, net.to(DEV), T, deviceReverseSDE=DEV).to(DEV)


def _train(which, steps, nsf):
    from sdeflow_light_amd.train import MLPScoreTrainer, UNetScoreTrainer
    torch.manual_seed(3)
    if which == "mlp":
        from sdeflow_light_amd.NN import MLP
        B, d = 64, 6
        tr = MLPScoreTrainer(_gen(MLP(d, premodule="NormalizeLogRadius"), d, nsf), B, lr=1e-3, seed=11, use_graph=True)
    else:
        from sdeflow_light_amd.NNUnet1D import UNet1D
        B, d = 8, 8
        net = UNet1D(input_dim=d, base_channels=16, channel_mults=(1, 2), emb_dim=32, premodule="NormalizeLogRadius")
        tr = UNetScoreTrainer(_gen(net, d, nsf), B, d, lr=1e-3, seed=11, use_graph=True)
    torch.manual_seed(5)
    tr.set_data(torch.randn(B, d, device=DEV) * 1.5)
    losses = [float(tr.step()) for _ in range(steps)]
    return losses, tr.flat.clone(), tr.rng.state.clone(), tr


@pytest.mark.parametrize("which,steps", [("mlp", 3), ("unet1d", 2)])
def test_trainer_kernel_route_equals_composed(ops, SS, monkeypatch, which, steps):
    """The graph-captured trainers on both routes: the same losses and parameters bit for bit, kernel nodes only, and the
    kernel route's graph is shorter by the composed chain (6 nsf + 9 launches) less the at most 2 launches that replace it."""
    nsf = 4
    calls = _recorded(monkeypatch, ops)
    l1, p1, s1, tr1 = _train(which, steps, nsf)
    assert len(calls) == 2                                   # the warm-up step and the capture; replays call nothing
    with monkeypatch.context() as m:
        m.setattr(ops, "forward_perturb_supported", lambda kind, n: False)
        l0, p0, s0, tr0 = _train(which, steps, nsf)
    assert len(calls) == 2
    assert all(v == v for v in l1) and l1 == l0
    assert torch.equal(p1, p0) and torch.equal(s1, s0)
    k1, k0 = ops.graph_node_kinds(tr1.graph), ops.graph_node_kinds(tr0.graph)
    print(f"{which}: captured step, kernel route {k1}, composed route {k0}")
    assert set(k1) == {"kernel"} and set(k0) == {"kernel"}
    assert k0["kernel"] - k1["kernel"] >= 6 * nsf
