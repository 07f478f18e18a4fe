"""The driver's 16x16 U-Net (base_channels 32, channel_mults (1, 2, 4), two ResBlocks per level, attention at 8x8 and 4x4):
its six attention blocks at 4x4 (T = 16 tokens, C = 128) run the one-launch kernels of csrc/attention_small_kernels.hip, the
five at 8x8 (T = 64, C = 64) the flash kernels as before, and nothing runs the composed bmm / softmax chain.  Route spies as
in tests/test_unet2d_sizes_gpu.py; the composed route of the same build is obtained by patching
ops.attention_small_supported to False.  End-to-end parity against the reference fixtures and the float64 oracle is held by
the existing 16x16 tests (test_unet2d_gpu, test_round2_gpu, test_dropout_gpu, test_multihead_attention_gpu s16h2,
test_optim_stage_gpu), which take the new route unchanged."""
import math

import pytest
import torch

from conftest import rel_l2, within
from sdeflow_light_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = ("attention_small_forward", "attention_small_dual_forward", "attention_small_dual_backward")
FLASH = ("attention_forward", "attention_dual_forward", "attention_dual_backward", "attention_mh_forward",
         "attention_dual_mh_forward", "attention_dual_mh_backward")
COMPOSED = ("bmm", "softmax_dual_forward", "softmax_dual_backward")


def _net(H):
    from sdeflow_light_amd.NNUnet import VorticityUNet
    from oracle.det_params import load_init_like_
    net = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, premodule=None, in_space=16,
                        attention_resolutions=(2, 4), num_heads=H, flatten_order="F")
    load_init_like_(net)
    return net.to(DEV)


def _spy(monkeypatch):
    calls = {k: 0 for k in SMALL + FLASH + COMPOSED}

    def count(name):
        real = getattr(ops, name)

        def w(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        monkeypatch.setattr(ops, name, w)
    for name in calls:
        count(name)
    return calls


def _train_inputs(seed, B=2, d=256):
    torch.manual_seed(seed)
    return (torch.randn(B, d, device=DEV) * 3, torch.rand(B, device=DEV), torch.randn(B, d, device=DEV),
            torch.rand(B, d, device=DEV))


def _train(gen, x, u, eps, uv):
    gen.zero_grad()
    per = gen.ssm(x, u=u, eps=eps, u_v=uv)
    per.mean().backward()
    return per.detach().clone(), torch.cat([p.grad.reshape(-1) for p in gen.a.parameters()]).clone()


@pytest.mark.parametrize("H", [1, 2, 4])
def test_routes(H, monkeypatch):
    """One sampler forward (B = 3) and one ssm(...).mean().backward() (B = 2): six calls of each new entry, five of the
    flash entries of the head count, none of the composed chain."""
    from test_host_gpu import make_gen
    gen = make_gen("sgm", _net(H))
    mh = "mh_" if H > 1 else ""
    torch.manual_seed(3)
    x, t = torch.randn(3, 256, device=DEV) * 3, torch.rand(3, device=DEV)
    calls = _spy(monkeypatch)
    y = gen.a(x, t)
    assert bool(torch.isfinite(y).all())
    assert calls["attention_small_forward"] == 6 and calls[f"attention_{mh}forward"] == 5, calls
    assert sum(calls.values()) == 11, calls
    for k in calls:
        calls[k] = 0
    per, grad = _train(gen, *_train_inputs(4))
    assert bool(torch.isfinite(per).all()) and bool(torch.isfinite(grad).all())
    assert calls["attention_small_dual_forward"] == 6 and calls["attention_small_dual_backward"] == 6, calls
    assert calls[f"attention_dual_{mh}forward"] == 5 and calls[f"attention_dual_{mh}backward"] == 5, calls
    assert sum(calls.values()) == 22, calls


@pytest.mark.parametrize("H", [1, 2])
def test_new_route_equals_composed_route(H, monkeypatch):
    """Same weights and inputs on both routes, at the tolerances of the flash-vs-composed tests
    (test_multihead_attention_gpu.py): sampler output rel-L2 <= 1e-4, per-sample loss <= 1e-5, all gradients <= 1e-4."""
    from test_host_gpu import make_gen
    gen = make_gen("sgm", _net(H))
    torch.manual_seed(5)
    x, t = torch.randn(4, 256, device=DEV) * 3, torch.rand(4, device=DEV)
    inp = _train_inputs(6)
    calls = _spy(monkeypatch)
    y_new = gen.a(x, t).clone()
    p_new, g_new = _train(gen, *inp)
    assert calls["attention_small_forward"] == 6 and calls["attention_small_dual_backward"] == 6 and calls["bmm"] == 0, calls
    monkeypatch.setattr(ops, "attention_small_supported", lambda T, heads, D: False)
    for k in calls:
        calls[k] = 0
    y_old = gen.a(x, t).clone()
    p_old, g_old = _train(gen, *inp)
    assert all(calls[k] == 0 for k in SMALL) and all(calls[k] > 0 for k in COMPOSED), calls
    within(rel_l2(y_new.cpu(), y_old.cpu()), 1e-4, f"16x16 H={H}: sampler forward, T = 16 kernels vs composed")
    within(rel_l2(p_new.cpu(), p_old.cpu()), 1e-5, f"16x16 H={H}: per-sample loss, T = 16 kernels vs composed")
    within(rel_l2(g_new.cpu(), g_old.cpu()), 1e-4, f"16x16 H={H}: all gradients, T = 16 kernels vs composed")


def test_trainer_graph_replay_equals_eager_and_repeats(monkeypatch):
    """UNetScoreTrainer(gen, 3, 256), three steps: the captured step replays the eager one bit for bit, a second graphed run
    repeats the first, the graph holds kernel nodes only, and the new route took the T = 16 blocks in every run."""
    from sdeflow_light_amd.train import UNetScoreTrainer
    from test_host_gpu import make_gen
    calls = _spy(monkeypatch)
    out = {}
    for use_graph in (False, True, True):
        torch.manual_seed(11)
        net = _net(1)
        gen = make_gen("sgm", net)
        for k in calls:
            calls[k] = 0
        tr = UNetScoreTrainer(gen, 3, 256, lr=1e-3, use_graph=use_graph, seed=5)
        torch.manual_seed(0)
        tr.set_data(torch.randn(3, 256, device=DEV))
        losses = [float(tr.step()) for _ in range(3)]
        assert calls["attention_small_dual_backward"] >= 6 and all(calls[k] == 0 for k in COMPOSED), calls
        if use_graph:
            assert tr.graph is not None and set(ops.graph_node_kinds(tr.graph)) == {"kernel"}
        res = (losses, net.flat_parameters()[0].clone().cpu(), net.flat_parameters()[1].clone().cpu())
        if use_graph in out:
            assert res[0] == out[use_graph][0] and torch.equal(res[1], out[use_graph][1]) and torch.equal(res[2], out[use_graph][2])
        out[use_graph] = res
    assert all(math.isfinite(v) for v in out[True][0])
    assert out[True][0] == out[False][0]
    assert torch.equal(out[True][1], out[False][1]) and torch.equal(out[True][2], out[False][2])
