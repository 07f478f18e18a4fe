"""Multi-head attention (AttentionBlock num_heads > 1, model/unet.py:220-250) on the HIP path: the fused multi-head kernels
(sampler forward, dual-number forward / backward), their one-head identity with the single-head entries, the composed
per-head fallback, and the whole VorticityUNet(num_heads=H) against the reference fixture g18 and the float64 oracle.
Head h owns the qkv columns [3Dh, 3D(h+1)) (q | k | v of D = C / H each) and the output columns [Dh, D(h+1))."""
import math

import pytest
import torch

from conftest import load_golden, rel_l2, within, check_digest

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

FWD_SHAPES = [(3, 64, 2, 16), (2, 256, 2, 32), (2, 256, 4, 16), (1, 1024, 2, 32), (1, 1024, 4, 16), (5, 256, 2, 64), (2, 64, 4, 32)]
# + launches big enough for the backward's second pass over the key blocks: Bp * H * T / keys-per-workgroup >= 2048
DUAL_SHAPES = FWD_SHAPES + [(3, 64, 2, 128), (2, 96, 2, 128), (512, 256, 2, 32), (256, 256, 4, 16), (512, 64, 2, 128)]


def heads_view(x, H, D):
    """[N][T][3C] -> q, k, v as [N][H][T][D] (head h = columns [3Dh, 3D(h+1)))."""
    N, T = x.shape[:2]
    y = x.reshape(N, T, H, 3, D).permute(0, 2, 3, 1, 4)
    return y[:, :, 0], y[:, :, 1], y[:, :, 2]


def mh_attention_ref(x, H, D):
    """QKVAttention on the reshaped (B*H, 3D, T) slabs in plain PyTorch fp32 -> [N][T][C] (head h at columns [Dh, D(h+1)))."""
    q, k, v = heads_view(x, H, D)
    s = D ** -0.25
    o = torch.einsum("nhts,nhsd->nhtd", torch.softmax(torch.einsum("nhtd,nhsd->nhts", q * s, k * s), -1), v)
    return o.permute(0, 2, 1, 3).reshape(x.shape[0], x.shape[1], H * D)


def make_qkv(N, T, H, D, seed, amp=1.5, peak=4.0):
    torch.manual_seed(seed)
    qkv = torch.randn(N, T, 3 * H * D) * amp
    qkv[0, : T // 2, :D] *= peak                      # peaked rows of head 0: exercises the running-max rescale
    qkv[-1, T // 4:, 3 * D * (H - 1): 3 * D * (H - 1) + D] *= peak      # and of the last head
    return qkv


# ------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("N,T,H,D", FWD_SHAPES + [(2, 128, 2, 128), (3, 192, 4, 64)])
def test_mh_attention_forward(N, T, H, D):
    from sdeflow_light_amd import ops
    qkv = make_qkv(N, T, H, D, seed=T + H + D)
    ref = mh_attention_ref(qkv, H, D)
    assert ops.attention_mh_supported(T, H, D)
    out = torch.full((N * T * H * D,), float("nan"), device=DEV)
    ops.attention_mh_forward(qkv.to(DEV).contiguous().view(-1), out, N, T, H, D, 1.0 / math.sqrt(D))
    within(rel_l2(out.view(N, T, H * D).cpu(), ref), 2e-5, f"mh forward N={N} T={T} H={H} D={D}")


@pytest.mark.parametrize("Bp,T,H,D", DUAL_SHAPES)
def test_mh_dual_attention_forward_backward(Bp, T, H, D):
    from sdeflow_light_amd import ops
    C = H * D
    qkv = make_qkv(2 * Bp, T, H, D, seed=T + H + D + Bp, amp=1.2, peak=3.0)
    xp, xt = qkv[:Bp].clone().requires_grad_(True), qkv[Bp:].clone().requires_grad_(True)
    o, od = torch.func.jvp(lambda a: mh_attention_ref(a, H, D), (xp,), (xt,))
    assert ops.attention_dual_mh_supported(T, H, D)
    s2 = 1.0 / math.sqrt(D)
    dev_qkv = qkv.to(DEV).contiguous().view(-1)
    att, stats = ops.attention_dual_mh_forward(dev_qkv, Bp, T, H, D, s2)
    a = att.view(2 * Bp, T, C).cpu()
    e_o, e_od = rel_l2(a[:Bp], o.detach()), rel_l2(a[Bp:], od.detach())
    torch.manual_seed(1)
    g = torch.randn(2 * Bp, T, C)
    ((o * g[:Bp]).sum() + (od * g[Bp:]).sum()).backward()
    gd = g.to(DEV).contiguous().view(-1)
    dq = ops.attention_dual_mh_backward(dev_qkv, att, gd, stats, Bp, T, H, D, s2)
    d = dq.view(2 * Bp, T, 3 * C).cpu()
    errs = {}
    for i, nm in enumerate(("q", "k", "v")):
        cols = torch.cat([torch.arange(3 * D * h + i * D, 3 * D * h + (i + 1) * D) for h in range(H)])
        errs[nm] = rel_l2(d[:Bp][..., cols], xp.grad[..., cols])
        errs[nm + "dot"] = rel_l2(d[Bp:][..., cols], xt.grad[..., cols])
    print(f"mh dual attention Bp={Bp} T={T} H={H} D={D}: o {e_o:.1e} odot {e_od:.1e} | "
          + " ".join(f"{k}bar {v:.1e}" for k, v in errs.items()))
    assert e_o <= 2e-5 and e_od <= 2e-5
    assert max(errs.values()) <= 2e-5, errs
    dq2 = ops.attention_dual_mh_backward(dev_qkv, att, gd, stats, Bp, T, H, D, s2)
    assert torch.equal(dq, dq2)


@pytest.mark.parametrize("Bp,T,C", [(3, 64, 32), (2, 256, 64), (5, 256, 128), (1, 1024, 64), (2, 96, 128), (512, 256, 64)])
def test_mh_entries_at_one_head_equal_single_head_bitwise(Bp, T, C):
    from sdeflow_light_amd import ops
    qkv = make_qkv(2 * Bp, T, 1, C, seed=7 + T + C).to(DEV).contiguous().view(-1)
    s2 = 1.0 / math.sqrt(C)
    if ops.attention_supported(T, C):
        a1 = ops.attention_forward(qkv, torch.empty(2 * Bp * T * C, device=DEV), 2 * Bp, T, C, s2)
        a2 = ops.attention_mh_forward(qkv, torch.empty(2 * Bp * T * C, device=DEV), 2 * Bp, T, 1, C, s2)
        assert torch.equal(a1, a2)
    att1, st1 = ops.attention_dual_forward(qkv, Bp, T, C, s2)
    att2, st2 = ops.attention_dual_mh_forward(qkv, Bp, T, 1, C, s2)
    assert torch.equal(att1, att2) and torch.equal(st1, st2)
    torch.manual_seed(2)
    g = torch.randn(2 * Bp * T * C, device=DEV)
    d1 = ops.attention_dual_backward(qkv, att1, g, st1, Bp, T, C, s2)
    d2 = ops.attention_dual_mh_backward(qkv, att2, g, st2, Bp, T, 1, C, s2)
    assert torch.equal(d1, d2)


def test_mh_attention_unsupported_shapes_fail_loudly():
    from sdeflow_light_amd import ops
    from sdeflow_light_amd._lib import MsgmError
    assert not ops.attention_mh_supported(80, 2, 32) and not ops.attention_mh_supported(64, 8, 8)
    assert not ops.attention_mh_supported(16, 2, 64) and not ops.attention_mh_supported(64, 2, 48)
    assert not ops.attention_dual_mh_supported(96, 2, 64) and ops.attention_dual_mh_supported(96, 2, 128)
    assert not ops.attention_dual_mh_supported(64, 8, 8)
    with pytest.raises(MsgmError):
        ops.attention_mh_forward(torch.zeros(2 * 80 * 192, device=DEV), torch.zeros(2 * 80 * 64, device=DEV), 2, 80, 2, 32, 1.0)
    with pytest.raises(MsgmError):
        ops.attention_dual_mh_forward(torch.zeros(2 * 64 * 192, device=DEV), 1, 64, 8, 8, 1.0)


# ------------------------------------------------------------------------------------------------------------ network
def _vunet(S_, H, fill="init_like", channels=1):
    from sdeflow_light_amd.NNUnet import VorticityUNet
    from oracle.det_params import load_init_like_
    net = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, premodule=None, in_space=S_,
                        attention_resolutions=(2, 4), num_heads=H, flatten_order="F", channels=channels)
    if fill == "init_like":
        load_init_like_(net)
    return net.to(DEV)


G18 = [("s32h2", 32, 2), ("s32h4", 32, 4), ("s16h2", 16, 2)]


@pytest.mark.parametrize("tag,S_,H", G18)
def test_vorticity_unet_multihead_vs_reference_g18(tag, S_, H):
    """VorticityUNet(num_heads=H) on the HIP path against the reference's own outputs (g18): forward, per-sample SSM loss,
    the stored attention-parameter gradients (every row of the weights), digests of all gradients — the tolerances the CPU oracle meets
    against the same fixture (test_multihead_oracle.py)."""
    from test_host_gpu import make_gen
    g = load_golden("g18_multihead")
    gen = make_gen("sgm", _vunet(S_, H))
    out = gen.a(g[tag + "_x"].to(DEV), g[tag + "_fwd_t"].to(DEV))
    within(rel_l2(out.cpu(), g[tag + "_fwd"]), 5e-6, f"VorticityUNet {S_}x{S_} H={H} forward vs reference")
    gen.zero_grad()
    per = gen.ssm(g[tag + "_x"].to(DEV), u=g[tag + "_u_t"].reshape(-1).to(DEV), eps=g[tag + "_eps"].to(DEV),
                  u_v=g[tag + "_u_v"].to(DEV))
    within(rel_l2(per.detach().cpu(), g[tag + "_per"]), 1e-5, f"VorticityUNet {S_}x{S_} H={H} per-sample SSM loss vs reference")
    per.mean().backward()
    grads = {k: p.grad.cpu() for k, p in gen.a.named_parameters()}
    from test_multihead_oracle import g18_attention_grads
    worst = max(rel_l2(got, ref) for _, got, ref in g18_attention_grads(g, tag, grads))
    within(worst, 1e-4, f"{tag}: worst stored attention-parameter gradient vs reference")
    check_digest(g, tag, grads, "a.", 1e-4)


@pytest.mark.parametrize("tag,S_,H", G18)
def test_vorticity_unet_multihead_vs_fp64_oracle(tag, S_, H, monkeypatch):
    """The same against the multi-head oracle in float32 / float64 (conftest.parity_vs_fp64 at its DEFAULT slack 2 / 4)."""
    from test_host_gpu import make_gen
    from test_round2_gpu import ssm_parity_vs_fp64
    from test_multihead_oracle import mh_attention_block, g18_params
    from oracle import nets_ref as N
    g = load_golden("g18_multihead")
    monkeypatch.setattr(N, "attention_block", mh_attention_block(H))
    cfg = N.UNet2DConfig(in_space=S_)
    score = lambda prm, yy, tt: N.vorticity_unet_forward(prm, yy, tt, cfg, None, "F")
    gen = make_gen("sgm", _vunet(S_, H))
    ssm_parity_vs_fp64(gen, score, g18_params(S_), g[tag + "_x"], g[tag + "_u_t"].reshape(-1), g[tag + "_eps"], g[tag + "_u_v"],
                       f"VorticityUNet {S_}x{S_} num_heads={H}, B=2")


def test_attention_branch_is_live():
    """Same weights, num_heads 1 vs 2: outputs differ by far more than any tolerance above (a net that ignored num_heads
    would otherwise pass)."""
    torch.manual_seed(4)
    n1, n2 = _vunet(32, 1), _vunet(32, 2)
    n2.load_state_dict(n1.state_dict())
    x, t = torch.randn(2, 1024, device=DEV) * 3, torch.full((2,), 0.37, device=DEV)
    e = rel_l2(n2(x, t).cpu(), n1(x, t).cpu())
    print(f"num_heads 2 vs 1 at the same weights: rel-L2 {e:.2e}")
    assert e > 1e-3


def test_sampler_fused_equals_composed_two_heads(monkeypatch):
    from sdeflow_light_amd import ops
    net = _vunet(32, 2)
    torch.manual_seed(5)
    x, t = torch.randn(4, 1024, device=DEV) * 3, torch.rand(4, device=DEV)
    calls = []
    real = ops.attention_mh_forward
    monkeypatch.setattr(ops, "attention_mh_forward", lambda *a, **k: (calls.append(a[4]), real(*a, **k))[1])
    fused = net(x, t).clone()
    assert calls, "the fused multi-head forward was not taken"
    monkeypatch.setattr(ops, "attention_mh_supported", lambda T, H, D: False)
    composed = net(x, t)
    within(rel_l2(fused.cpu(), composed.cpu()), 1e-4, "sampler forward H=2, fused vs composed per-head attention")


def test_training_fused_equals_composed_two_heads(monkeypatch):
    from sdeflow_light_amd import ops
    from test_host_gpu import make_gen
    gen = make_gen("sgm", _vunet(32, 2))
    torch.manual_seed(6)
    B, d = 2, 1024
    x, u, eps, uv = (torch.randn(B, d, device=DEV) * 3, torch.rand(B, device=DEV), torch.randn(B, d, device=DEV),
                     torch.rand(B, d, device=DEV))

    def run():
        gen.zero_grad()
        per = gen.ssm(x, u=u, eps=eps, u_v=uv)
        per.mean().backward()
        return per.detach().clone(), torch.cat([p.grad.reshape(-1) for p in gen.a.parameters()]).clone()
    calls = []
    real = ops.attention_dual_mh_backward
    monkeypatch.setattr(ops, "attention_dual_mh_backward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    pf, gf = run()
    assert calls, "the fused multi-head dual attention was not taken"
    n_fused = len(calls)
    monkeypatch.setattr(ops, "attention_dual_mh_supported", lambda T, H, D: False)
    pc, gc = run()
    assert len(calls) == n_fused, "the composed per-head attention was not taken"
    within(rel_l2(pf.cpu(), pc.cpu()), 1e-5, "training H=2: per-sample loss, fused vs composed")
    within(rel_l2(gf.cpu(), gc.cpu()), 1e-4, "training H=2: all gradients, fused vs composed")


def test_trainer_two_heads_graph_replay_equals_eager_and_repeats():
    from sdeflow_light_amd import ops
    from sdeflow_light_amd.train import UNetScoreTrainer
    from test_host_gpu import make_gen
    out = {}
    for use_graph in (False, True, True):
        torch.manual_seed(11)
        net = _vunet(16, 2)
        gen = make_gen("sgm", net)
        tr = UNetScoreTrainer(gen, 8, 256, lr=1e-3, use_graph=use_graph, seed=5)
        torch.manual_seed(0)
        tr.set_data(torch.randn(8, 256, device=DEV))
        losses = [float(tr.step()) for _ in range(3)]
        if use_graph:
            assert set(ops.graph_node_kinds(tr.graph)) == {"kernel"}
        res = (losses, net.flat_parameters()[0].clone().cpu(), net.flat_parameters()[1].clone().cpu())
        if use_graph in out:
            assert res[0] == out[use_graph][0] and torch.equal(res[1], out[use_graph][1]) and torch.equal(res[2], out[use_graph][2])
        out[use_graph] = res
    assert all(math.isfinite(v) for v in out[True][0])
    assert out[True][0] == out[False][0]
    assert torch.equal(out[True][1], out[False][1]) and torch.equal(out[True][2], out[False][2])


def test_c4_shape_step_four_heads_is_finite():
    """One training step of the C4 network (64x64x3) at num_heads = 4 on the 32-row shard: attention at T = 1024 (D = 16)
    and T = 256 (D = 32) on the fused multi-head kernels."""
    from sdeflow_light_amd import ops
    from sdeflow_light_amd.train import UNetScoreTrainer
    from test_host_gpu import make_gen
    torch.manual_seed(12)
    net = _vunet(64, 4, channels=3)
    gen = make_gen("sgm", net)
    tr = UNetScoreTrainer(gen, 32, 3 * 64 * 64, lr=1e-4, seed=1)
    tr.set_data(torch.randn(32, 3 * 64 * 64, device=DEV))
    loss = float(tr.step())
    flat, gflat = net.flat_parameters()
    assert math.isfinite(loss) and bool(torch.isfinite(flat).all()) and bool(torch.isfinite(gflat).all())
    assert float(gflat.abs().max()) > 0


def test_constructor_checks_heads():
    from sdeflow_light_amd.NNUnet import VorticityUNet, UNetModelWithLogNorm
    from sdeflow_light_amd._lib import MsgmError
    with pytest.raises(MsgmError, match="64 channels"):
        VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), in_space=16, num_heads=3)
    kw = dict(in_channels=1, model_channels=32, out_channels=1, in_space=16, num_res_blocks=2, attention_resolutions=(2, 4),
              channel_mult=(1, 2, 4))
    UNetModelWithLogNorm(num_heads=4, **kw)
    with pytest.raises(MsgmError, match="num_heads = 3"):
        UNetModelWithLogNorm(num_heads=2, num_heads_upsample=3, **kw)          # decoder blocks only
    core = UNetModelWithLogNorm(num_heads=2, num_heads_upsample=4, **kw)
    heads = {k: m.num_heads for k, m in core.named_modules() if hasattr(m, "num_heads") and k}
    assert all(v == (4 if k.startswith("output_blocks.") else 2) for k, v in heads.items()) and len(heads) == 4 + 1 + 6
    one = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), in_space=16, num_heads=1).state_dict()
    four = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), in_space=16, num_heads=4).state_dict()
    assert {k: v.shape for k, v in one.items()} == {k: v.shape for k, v in four.items()}
