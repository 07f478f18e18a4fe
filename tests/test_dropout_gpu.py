"""Dropout in the 2-D U-Net on the GPU: the mask rule's device anchors, the dropout builds of the GroupNorm+SiLU kernels
against PyTorch, eval mode / p = 0 against the existing route, the network against the float64 oracle with the masks
injected (test_dropout_oracle.dropout_gn_silu), and the stream contract (graph replay, fresh masks per pass, shards,
the graphed sampler)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2, within, parity_vs_fp64
import philox_np as PX

pytestmark = pytest.mark.gpu
DEV = "cuda"


def cl(x):    # (N,C,H,W) -> [N][H*W][C] flat
    return x.permute(0, 2, 3, 1).contiguous().reshape(-1)


# ------------------------------------------------------------------------------------------------------------ anchors
@pytest.mark.parametrize("seed,offset,row_base,n", [(12345, 0, 0, 0), ((1 << 62) + 977, (1 << 33) + 5, 4, 12)])
def test_restatement_equals_device_fill_uniform(seed, offset, row_base, n):
    """The NumPy Philox restatement against the device's fill_uniform stream (code this feature does not change)."""
    from sdeflow_light_amd import _lib as L, ops
    rng = L.PhiloxState(seed, DEV, offset=offset, row_base=row_base, n=n)
    for stream in (L.RNG_STREAM_USER, L.RNG_STREAM_DROPOUT + 3):
        got = ops.fill_uniform(torch.empty(4099, device=DEV), rng, stream).cpu().numpy()
        want = PX.fill_uniform(seed, offset, stream, 4099, base=row_base * n)
        assert np.array_equal(got, want), stream


@pytest.mark.parametrize("seed,offset,row_base,layer,Bp,P,C,p", [
    (7, 0, 0, 0, 2, 256, 32, 0.1), (123456789, 3, 4, 5, 3, 64, 64, 0.3), ((1 << 62) + 11, (1 << 32) + 9, 8, 18, 2, 16, 128, 0.5),
    (99, 1, 12, 7, 1, 1024, 4, 0.9)])
def test_mask_entry_equals_rule(seed, offset, row_base, layer, Bp, P, C, p):
    from sdeflow_light_amd import _lib as L, ops
    rng = L.PhiloxState(seed, DEV, offset=offset, row_base=row_base, n=4)
    keep = ops.dropout_mask(ops.dropout_desc(rng, layer, p), Bp, P, C, DEV).cpu().numpy().reshape(Bp, P, C)
    assert np.array_equal(keep, PX.dropout_keep(seed, offset, row_base, layer, p, Bp, P, C))


def test_keep_rate():
    from sdeflow_light_amd import _lib as L, ops
    rng = L.PhiloxState(2024, DEV, offset=17)
    for p in (0.1, 0.5):
        keep = ops.dropout_mask(ops.dropout_desc(rng, 2, p), 64, 4096, 64, DEV)
        n = keep.numel()
        assert n >= 10 ** 7
        rate = float(keep.double().mean())
        sd = math.sqrt(p * (1 - p) / n)
        print(f"p = {p}: keep rate {rate:.6f} over {n} elements ({(rate - (1 - p)) / sd:+.2f} sigma)")
        assert abs(rate - (1 - p)) <= 5 * sd


# ------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("C,H,p", [(32, 8, 0.1), (64, 4, 0.3), (128, 16, 0.5), (256, 4, 0.2)])
def test_groupnorm_dropout_forward_backward(C, H, p):
    """GN -> SiLU -> mask * scale against PyTorch fp32 (tangent by torch.func.jvp, cotangents by autograd), at the
    tolerances of test_unet2d_gpu.test_groupnorm_dual_forward_backward."""
    from sdeflow_light_amd import _lib as L, ops
    torch.manual_seed(C)
    B, G, P = 3, min(C, 32), H * H
    rng = L.PhiloxState(31 + C, DEV, offset=2, row_base=4, n=4)
    desc = ops.dropout_desc(rng, 3, p)
    m = torch.from_numpy(PX.dropout_multiplier(31 + C, 2, 4, 3, p, B, H, H, C))
    x, xd = torch.randn(B, C, H, H) * 1.5 + 0.3, torch.randn(B, C, H, H)
    gam, bet = 1 + 0.2 * torch.randn(C), 0.2 * torch.randn(C)

    def f(xx, g_, b_):
        y = F.group_norm(xx, G, g_, b_, eps=1e-5)
        return torch.sigmoid(y) * y * m
    xg, xdg = x.clone().requires_grad_(True), xd.clone().requires_grad_(True)
    gg, bg = gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
    yp, yt = torch.func.jvp(lambda a: f(a, gg, bg), (xg,), (xdg,))
    xs = torch.cat([cl(x), cl(xd)]).to(DEV)
    stats = torch.empty(B * G * 4, device=DEV)
    out = ops.groupnorm_dual_forward(xs, gam.to(DEV), bet.to(DEV), B, P, C, G, True, True, stats=stats, dropout=desc)
    half = B * P * C
    assert rel_l2(out[:half].cpu(), cl(yp.detach())) <= 1e-5
    assert rel_l2(out[half:].cpu(), cl(yt.detach())) <= 1e-5
    zero = cl((m == 0).float()) > 0
    assert torch.equal(out[:half].cpu() == 0, zero) and torch.equal(out[half:].cpu() == 0, zero)   # same positions, both halves
    out1 = ops.groupnorm_dual_forward(cl(x).to(DEV), gam.to(DEV), bet.to(DEV), B, P, C, G, False, True, dropout=desc)
    assert torch.equal(out1, out[:half])                                 # the sampler's (no tangent) build: same primal bits
    gp, gt = torch.randn_like(yp), torch.randn_like(yt)
    ((yp * gp).sum() + (yt * gt).sum()).backward()
    gout = torch.cat([cl(gp), cl(gt)]).to(DEV)
    dga, dbe = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    gx = ops.groupnorm_dual_backward(xs, gam.to(DEV), bet.to(DEV), stats, gout, dga, dbe, B, P, C, G, True, dropout=desc)
    assert rel_l2(gx[:half].cpu(), cl(xg.grad)) <= 2e-5, rel_l2(gx[:half].cpu(), cl(xg.grad))
    assert rel_l2(gx[half:].cpu(), cl(xdg.grad)) <= 2e-5
    assert rel_l2(dga.cpu(), gg.grad) <= 2e-5 and rel_l2(dbe.cpu(), bg.grad) <= 2e-5


def test_groupnorm_dropout_at_p0_equals_the_existing_entries():
    from sdeflow_light_amd import _lib as L, ops
    torch.manual_seed(3)
    B, C, P = 4, 64, 256
    G = 32
    rng = L.PhiloxState(5, DEV)
    desc = ops.dropout_desc(rng, 0, 0.0)
    xs = torch.randn(2 * B * P * C, device=DEV)
    gam, bet = 1 + 0.2 * torch.randn(C, device=DEV), 0.2 * torch.randn(C, device=DEV)
    st0, st1 = torch.empty(B * G * 4, device=DEV), torch.empty(B * G * 4, device=DEV)
    o0 = ops.groupnorm_dual_forward(xs, gam, bet, B, P, C, G, True, True, stats=st0)
    o1 = ops.groupnorm_dual_forward(xs, gam, bet, B, P, C, G, True, True, stats=st1, dropout=desc)
    assert torch.equal(o0, o1) and torch.equal(st0, st1)
    gout = torch.randn_like(xs)
    res = []
    for d in (None, desc):
        dga, dbe = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        with ops.DeferredReduces.on(DEV):
            gx = ops.groupnorm_dual_backward(xs, gam, bet, st0, gout, dga, dbe, B, P, C, G, True, gx=torch.empty_like(xs),
                                             dropout=d)
        res.append((gx, dga, dbe))
    assert all(torch.equal(a, b) for a, b in zip(*res))


def test_dropout_entries_refuse_unsupported_shapes():
    from sdeflow_light_amd import _lib as L, ops
    from sdeflow_light_amd._lib import MsgmError
    rng = L.PhiloxState(5, DEV)
    with pytest.raises(MsgmError):
        ops.dropout_desc(rng, 0, 1.0)
    with pytest.raises(MsgmError):
        ops.dropout_mask(ops.dropout_desc(rng, 0, 0.1), 1, 16, 6, DEV)          # C % 4 != 0
    x = torch.zeros(2 * 16 * 6, device=DEV)
    with pytest.raises(MsgmError):
        ops.groupnorm_dual_forward(x, torch.ones(6, device=DEV), torch.zeros(6, device=DEV), 1, 16, 6, 3, True, True,
                                   dropout=ops.dropout_desc(rng, 0, 0.1))


# ------------------------------------------------------------------------------------------------------------ network
def _vunet(S_, p, premodule=None):
    from sdeflow_light_amd.NNUnet import VorticityUNet
    from oracle.det_params import load_init_like_
    net = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, premodule=premodule, in_space=S_,
                        attention_resolutions=(2, 4), flatten_order="F", dropout=p)
    load_init_like_(net)
    return net.to(DEV)


def _draws(B, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, d, generator=g) * 3, torch.rand(B, generator=g), torch.randn(B, d, generator=g),
            torch.rand(B, d, generator=g))


def _ssm(gen, x, u, eps, uv):
    gen.zero_grad()
    per = gen.ssm(x.to(DEV), u=u.to(DEV), eps=eps.to(DEV), u_v=uv.to(DEV))
    per.mean().backward()
    return per.detach().clone(), {k: q.grad.detach().clone() for k, q in gen.a.named_parameters()}


def test_eval_mode_and_p0_change_nothing():
    """A dropout=0.2 net in eval() is the dropout=0 net bit for bit: forward, per-sample SSM loss and every gradient."""
    from test_host_gpu import make_gen
    x, u, eps, uv = _draws(2, 256, 1)
    t = torch.tensor([0.2, 0.6], device=DEV)
    res = []
    for p in (0.0, 0.2):
        torch.manual_seed(8)
        gen = make_gen("sgm", _vunet(16, p))
        if p:
            gen.a.eval()
        assert not gen.a.dropout_active()
        y = gen.a(x.to(DEV), t).clone()
        res.append((y,) + _ssm(gen, x, u, eps, uv))
    (y0, per0, g0), (y1, per1, g1) = res
    assert torch.equal(y0, y1) and torch.equal(per0, per1)
    assert all(torch.equal(g0[k], g1[k]) for k in g0)


def _oracle_score(S_, premodule):
    from oracle import nets_ref as N
    cfg = N.UNet2DConfig(in_space=S_, use_log_norm=premodule is not None)
    return lambda prm, yy, tt: N.vorticity_unet_forward(prm, yy, tt, cfg, premodule, "F")


@pytest.mark.parametrize("S_,p,premodule", [(16, 0.1, None), (16, 0.3, "NormalizeLogRadius"), (32, 0.1, None)])
def test_train_mode_ssm_vs_fp64_oracle(S_, p, premodule, monkeypatch):
    """Train-mode SSM (masks drawn from the SDE's stream at its current offset) against the float32 / float64 oracle with
    the rule's masks injected, conftest.parity_vs_fp64 at its DEFAULT slack: encoder / middle ResBlocks (single source) and
    the decoder's two-source blocks."""
    from oracle import nets_ref as N, sde_ref as S, ssm_ref as LR
    from test_host_gpu import make_gen
    from test_dropout_oracle import dropout_gn_silu
    torch.manual_seed(9)
    net = _vunet(S_, p, premodule)
    gen = make_gen("sgm", net)
    rng = gen.base_sde.philox(DEV)
    seed, offset = rng.state_dict()["seed"], 5
    B, d = 2, S_ * S_
    x, u, eps, uv = _draws(B, d, 2)
    params = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    monkeypatch.setattr(N, "_gn_silu", dropout_gn_silu(seed, offset, 0, p))
    score = _oracle_score(S_, premodule)
    sp = S.SdeSpec()
    torch.set_num_threads(min(16, torch.get_num_threads()))

    def hip():
        rng.load_state_dict({"seed": seed, "offset": offset})
        per, g = _ssm(gen, x, u, eps, uv)
        assert rng.state_dict()["offset"] == offset + 1          # the pass advanced the stream once
        return per, g

    def oracle(dt):
        t = S.clamp_time(sp, u.reshape(B, 1))
        y = S.vp_perturb(sp, t, x, eps)
        v = S.rademacher_from_uniform(uv)
        _, per, g = LR.ssm_mean_and_grads(sp, score, {k: w.to(dt) for k, w in params.items()}, t.to(dt), y.to(dt), v.to(dt))
        return per, g
    assert gen.a._build()["set2t"] is not None                   # the two-source decoder blocks are on this path
    parity_vs_fp64(hip, oracle, f"train-mode dropout p={p}, {S_}x{S_}, premodule={premodule}, B=2")


@pytest.mark.parametrize("S_,p,premodule", [(16, 0.3, None), (32, 0.1, "NormalizeLogRadius")])
def test_train_mode_forward_vs_oracle(S_, p, premodule, monkeypatch):
    """The sampler route in train mode (out_layers materialised with the mask, conv2 unfused) against the float64 oracle;
    successive calls draw fresh masks from the net's own stream."""
    from oracle import nets_ref as N
    from sdeflow_light_amd import _lib as L
    from test_dropout_oracle import dropout_gn_silu
    net = _vunet(S_, p, premodule)
    net.dropout_rng = L.PhiloxState(4321, DEV, offset=6)
    x, _, _, _ = _draws(3, S_ * S_, 3)
    t = torch.tensor([0.05, 0.4, 0.9])
    y = net(x.to(DEV), t.to(DEV)).cpu()
    assert net.dropout_rng.state_dict()["offset"] == 7
    monkeypatch.setattr(N, "_gn_silu", dropout_gn_silu(4321, 6, 0, p))
    params = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    with torch.no_grad():
        ref = _oracle_score(S_, premodule)(params, x.double(), t.double())
    within(rel_l2(y, ref), 1e-5, f"train-mode forward p={p} {S_}x{S_} {premodule} vs float64 oracle")
    y2 = net(x.to(DEV), t.to(DEV)).cpu()
    assert rel_l2(y2, y) > 1e-3                                   # the next pass drew other masks
    net.eval()
    assert torch.equal(net(x.to(DEV), t.to(DEV)), net(x.to(DEV), t.to(DEV)))


def test_consecutive_passes_draw_different_masks_and_runs_repeat():
    from test_host_gpu import make_gen
    x, u, eps, uv = _draws(2, 256, 4)
    runs = []
    for _ in range(2):
        torch.manual_seed(10)
        gen = make_gen("sgm", _vunet(16, 0.2))
        a = _ssm(gen, x, u, eps, uv)
        b = _ssm(gen, x, u, eps, uv)
        assert rel_l2(b[0].cpu(), a[0].cpu()) > 1e-4               # same data, same weights: the masks moved on
        runs.append((a, b))
    for r0, r1 in zip(*runs):
        assert torch.equal(r0[0], r1[0]) and all(torch.equal(r0[1][k], r1[1][k]) for k in r0[1])


def test_trainer_graph_replay_equals_eager_and_repeats():
    from sdeflow_light_amd import ops
    from sdeflow_light_amd.train import UNetScoreTrainer
    from test_host_gpu import make_gen
    out = {}
    for use_graph in (False, True, True):
        torch.manual_seed(11)
        net = _vunet(16, 0.2)
        gen = make_gen("sgm", net)
        tr = UNetScoreTrainer(gen, 8, 256, lr=1e-3, use_graph=use_graph, seed=5)
        torch.manual_seed(0)
        tr.set_data(torch.randn(8, 256, device=DEV))
        losses = [float(tr.step()) for _ in range(3)]
        if use_graph:
            assert set(ops.graph_node_kinds(tr.graph)) == {"kernel"}
        res = (losses, net.flat_parameters()[0].clone().cpu(), tr.rng.state_dict()["offset"])
        if use_graph in out:
            assert res[0] == out[use_graph][0] and torch.equal(res[1], out[use_graph][1])
        out[use_graph] = res
    assert all(math.isfinite(v) for v in out[True][0])
    assert out[True][0] == out[False][0] and torch.equal(out[True][1], out[False][1])
    assert out[True][2] == out[False][2] == 6                      # per step: the masks' advance + the update's


def test_shards_reproduce_the_full_batch_rows():
    """Rows [4, 8) on a shard at row_base 4 draw the masks the 8-row pass draws for them: same per-sample loss, bit for bit."""
    from test_host_gpu import make_gen
    x, u, eps, uv = _draws(8, 256, 5)
    pers = {}
    for rb, rows in ((None, slice(0, 8)), (0, slice(0, 4)), (4, slice(4, 8)), ("wrong", slice(4, 8))):
        torch.manual_seed(12)
        gen = make_gen("sgm", _vunet(16, 0.3))
        if rb is not None:
            gen.base_sde.set_shard(0 if rb == "wrong" else rb, 256)
        gen.zero_grad()
        pers[rb] = gen.ssm(x[rows].to(DEV), u=u[rows].to(DEV), eps=eps[rows].to(DEV), u_v=uv[rows].to(DEV)).detach().cpu()
    print("shard rows vs full batch, max |diff|:", float((pers[0] - pers[None][:4]).abs().max()),
          float((pers[4] - pers[None][4:]).abs().max()))
    assert torch.equal(pers[0], pers[None][:4]) and torch.equal(pers[4], pers[None][4:])
    assert rel_l2(pers["wrong"], pers[None][4:]) > 1e-4


def test_graphed_sampler_train_mode_equals_eager_steps():
    from sdeflow_light_amd import _lib as L, ops
    from sdeflow_light_amd.sde_scheme import GraphedStepSampler
    from test_host_gpu import make_gen
    B, n, steps = 4, 256, 3

    def make():
        torch.manual_seed(21)
        net = _vunet(16, 0.2)
        net.dropout_rng = L.PhiloxState(77, DEV)
        gen = make_gen("sgm", net)
        return gen, GraphedStepSampler(gen, B, n, steps, method="em")
    x0 = torch.randn(B, n, generator=torch.Generator().manual_seed(2)).to(DEV)
    gA, sA = make()
    outA = sA.run(x0).clone()
    gB, sB = make()
    ops.lincomb(sB.x, x0, 1.0)
    sB.step.zero_()
    for _ in range(steps):
        sB._body()
    sB.rng.advance(steps)
    assert torch.equal(outA, sB.x)
    assert gA.a.dropout_rng.state_dict()["offset"] == gB.a.dropout_rng.state_dict()["offset"] == 1 + steps
    t = torch.full((B,), 0.5, device=DEV)
    assert not torch.equal(gA.a(x0, t), gA.a(x0, t))              # every score call draws fresh masks


@pytest.mark.parametrize("tag,S_,pre", [("s32", 32, None), ("s16m", 16, "NormalizeLogRadius")])
def test_vs_reference_g19(tag, S_, pre):
    """Against the reference's VorticityUNet(dropout=p) in train mode with the rule's masks forced into its Dropout modules
    (g19): train-mode forward, and per-sample SSM loss and gradients at row_base 0 and 4 (SGM with the draws forced; the
    sparse MSGM SDE through ssm_loss(t, x, y)), at the g18 tolerances."""
    from conftest import load_golden, check_digest
    from sdeflow_light_amd import _lib as L
    from test_host_gpu import make_gen
    from test_dropout_oracle import g19_case, g19_worst
    g = load_golden("g19_dropout")
    p, seed, off, off_fwd = g19_case(g, tag)
    d = S_ * S_
    net = _vunet(S_, p, pre)
    gen = make_gen("sgm", net) if tag == "s32" else make_gen("sparse", net, n=d, nsf=4)
    net.dropout_rng = L.PhiloxState(seed, DEV, offset=off_fwd)
    out = gen.a(g[tag + "_fwd_x"].to(DEV), g[tag + "_fwd_t"].to(DEV))
    within(rel_l2(out.cpu(), g[tag + "_fwd"]), 5e-6, f"g19 {tag}: train-mode forward vs reference")
    rng = gen.base_sde.philox(DEV)
    for rb in (0, 4):
        gen.base_sde.set_shard(rb, d)
        rng.load_state_dict({"seed": seed, "offset": off})
        gen.zero_grad()
        if tag == "s32":
            per = gen.ssm(g[tag + "_x"].to(DEV), u=g[tag + "_u_t"].reshape(-1).to(DEV), eps=g[tag + "_eps"].to(DEV),
                          u_v=g[tag + "_u_v"].to(DEV))
        else:
            per = gen.ssm_loss(g[tag + "_t"].to(DEV), g[tag + "_y"].to(DEV), g[tag + "_y"].to(DEV), u_v=g[tag + "_u_v"].to(DEV))
        within(rel_l2(per.detach().cpu(), g[f"{tag}_rb{rb}_per"]), 1e-5, f"g19 {tag} row_base {rb}: per-sample SSM loss")
        per.mean().backward()
        grads = {k: q.grad.cpu() for k, q in gen.a.named_parameters()}
        if rb == 0:
            e, k = g19_worst(g, f"{tag}_rb0", grads)
            within(e, 1e-4, f"g19 {tag}: worst stored gradient ({k})")
        check_digest(g, f"{tag}_rb{rb}", grads, "a.", 1e-4)


def test_trainer_shards_reproduce_the_full_batch_rows(monkeypatch):
    """Two UNetScoreTrainers of 4 rows at row_base 0 and 4 draw (t, eps, v) and the dropout masks the 8-row trainer draws for
    those rows: the per-sample losses of one step are equal row for row, bit for bit."""
    from sdeflow_light_amd.NNUnet import VorticityUNet
    from sdeflow_light_amd.train import UNetScoreTrainer
    from test_host_gpu import make_gen
    seen = []
    real = VorticityUNet.ssm_grad

    def spy(self, *a, **k):
        per = real(self, *a, **k)
        seen.append(per.detach().clone().cpu())
        return per
    monkeypatch.setattr(VorticityUNet, "ssm_grad", spy)
    x = torch.randn(8, 256, generator=torch.Generator().manual_seed(6)).to(DEV) * 3
    pers = {}
    for rb, rows in ((None, slice(0, 8)), (0, slice(0, 4)), (4, slice(4, 8))):
        torch.manual_seed(13)
        gen = make_gen("sgm", _vunet(16, 0.3))
        tr = UNetScoreTrainer(gen, rows.stop - rows.start, 256, lr=1e-3, use_graph=False, seed=7, row_base=rb or 0)
        tr.set_data(x[rows])
        seen.clear()
        tr.step()
        pers[rb] = seen[0]
    print("trainer shards vs 8-row trainer, max |diff|:", float((pers[0] - pers[None][:4]).abs().max()),
          float((pers[4] - pers[None][4:]).abs().max()))
    assert torch.equal(pers[0], pers[None][:4]) and torch.equal(pers[4], pers[None][4:])
