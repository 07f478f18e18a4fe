#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the ACTUAL reference on CPU.

Build-container only: imports /root/reference (read-only) with the
plotting / IO-only dependencies it cannot import here stubbed out
(seaborn, netCDF4, torchvision — SURVEY.md App. C; the stubs never touch
arithmetic).  Every random draw on the hot path (torch.rand / randn /
randn_like: SDEs.py:141,515,518,522,688; sde_scheme.py:84,144,227) is
recorded in call order and stored next to the inputs and the reference's
outputs, so the oracle and the HIP kernels can be fed identical noise.

The reference never travels to the GPU box: only the .npz vectors written
here (inputs + expected outputs, no source) are committed.

Usage:  python tools/make_golden.py            # rewrites tests/golden/
"""
import importlib.machinery as mach
import os
import sys
import types

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")


def _stub(name):
    m = types.ModuleType(name)
    m.__spec__ = mach.ModuleSpec(name, None)
    m.__path__ = []
    sys.modules[name] = m
    return m


_stub("seaborn")
_stub("netCDF4").Dataset = object
_tv = _stub("torchvision")
for _s in ("datasets", "transforms", "utils"):
    setattr(_tv, _s, _stub("torchvision." + _s))
sys.modules["torchvision.utils"].save_image = lambda *a, **k: None
sys.path.insert(0, "/root/reference")

from NN import MLP  # noqa: E402
from NNUnet import VorticityUNet, UNetModelWithLogNorm  # noqa: E402
from NNUnet1D import UNet1D  # noqa: E402
from SDEs import SGMsde, MSGMsde, PluginReverseSDE, forward_SDE, sample_rademacher, randu_on_sphere  # noqa: E402
from sde_scheme import EMstep, euler_maruyama_sampler, heun_sampler, rk4_stratonovich_sampler  # noqa: E402
from model.nn_utils import timestep_embedding  # noqa: E402

from oracle.det_params import load_det_, load_init_like_  # noqa: E402


class Recorder:
    """Patch torch.rand / randn / randn_like and log every draw in order."""

    def __init__(self):
        self.draws = []

    def __enter__(self):
        self._o = (torch.rand, torch.randn, torch.randn_like)
        rec = self.draws

        def wrap(fn, kind):
            def f(*a, **k):
                out = fn(*a, **k)
                rec.append((kind, out.detach().clone()))
                return out
            return f
        torch.rand, torch.randn, torch.randn_like = (wrap(self._o[0], "rand"), wrap(self._o[1], "randn"),
                                                     wrap(self._o[2], "randn_like"))
        return self

    def __exit__(self, *a):
        torch.rand, torch.randn, torch.randn_like = self._o


def npy(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def save(name, **arrs):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **{k: npy(v) for k, v in arrs.items()})
    print(f"{name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")


def Tparam(T0=1.0):
    return torch.nn.Parameter(torch.FloatTensor([T0]), requires_grad=False)


def sgm(nsf=16):
    return SGMsde(beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=Tparam(), num_steps_forward=nsf, device="cpu")


def msgm(x_init, dense, nsf=16, norm_map="log"):
    return MSGMsde(x_init, beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=Tparam(), num_steps_forward=nsf,
                   device="cpu", estim_cst_norm_dens_r_T=False, norm_sampler="ecdf", norm_map=norm_map,
                   denseTensor=dense, plot_validate=False)


def sd_np(sd, skip=("T", "base_sde.T")):
    return {k: npy(v) for k, v in sd.items() if k not in skip}


# ---------------------------------------------------------------------------

def g01_schedule():
    s = sgm()
    t = torch.cat([torch.tensor([0.0, 1e-3, 1.0]), torch.linspace(0, 1, 254)]).reshape(-1, 1)
    save("g01_schedule", t=t, beta=s.beta(t), mean_weight=s.mean_weight(t), var=s.var(t))


def g02_sample_t():
    torch.manual_seed(2)
    s = sgm()
    rev = PluginReverseSDE(s, MLP(2), Tparam())
    x = torch.zeros(4096, 2)
    with Recorder() as r:
        t = rev.sample_t(x)
    u = r.draws[0][1].clone()
    # force a few raw draws onto / below the clamp edge
    u2 = u.clone()
    u2[:4, 0] = torch.tensor([0.0, 1e-3, 9.99e-4, 1.0001e-3])
    orig = torch.rand
    torch.rand = lambda *a, **k: u2.clone()
    t2 = rev.sample_t(x)
    torch.rand = orig
    save("g02_sample_t", u=u, t=t, u_edge=u2, t_edge=t2)


def g03_step_index():
    out = {}
    for nsf in (4, 16, 128):
        s = sgm(nsf)
        grid = torch.cat([torch.arange(0, nsf + 1, dtype=torch.float32) / nsf,
                          torch.tensor([5e-4, 0.06, 0.0625, 0.99, 1.0, 0.999999, 1e-3]),
                          torch.linspace(0, 1, 301)]).reshape(-1, 1)
        k = torch.trunc(s.num_steps_forward * grid / s.T).to(torch.int).to("cpu")      # SDEs.py:89-90
        for b in range(grid.shape[0]):
            if grid[b] >= s.T:
                k[b] = nsf
        out[f"t_{nsf}"] = grid
        out[f"k_{nsf}"] = k.reshape(-1).to(torch.int32)
    save("g03_step_index", **out)


def g04_vp_perturb():
    torch.manual_seed(4)
    s = sgm()
    out = {}
    for d, B in ((2, 512), (1024, 8)):
        x0 = torch.randn(B, d) * 2
        t = torch.rand(B, 1).clamp_min(1e-3)
        with Recorder() as r:
            y = s.sample(t, x0)
        out.update({f"x0_{d}": x0, f"t_{d}": t, f"eps_{d}": r.draws[0][1], f"y_{d}": y})
    save("g04_vp_perturb", **out)


def g05_drift_diffusion():
    torch.manual_seed(5)
    out = {}
    s = sgm()
    y = torch.randn(16, 3)
    t = torch.rand(16, 1)
    out.update(sgm_y=y, sgm_t=t, sgm_f=s.f(t, y), sgm_fs=s.f_strato(t, y), sgm_div=s.div_Sigma(t, y), sgm_g=s.g(t, y))
    xi = torch.randn(64, 4)
    with Recorder() as r:
        md = msgm(xi, dense=True)
    gen = torch.stack([d[1] for d in r.draws if d[0] == "randn" and tuple(d[1].shape) == (4, 4)][:4])
    y = torch.randn(16, 4)
    t = torch.rand(16, 1)
    out.update(dense_gen=gen, dense_G=md.G, dense_LG=md.L_G, dense_y=y, dense_t=t, dense_f=md.f(t, y),
               dense_fs=md.f_strato(t, y), dense_div=md.div_Sigma(t, y), dense_g=md.g(t, y))
    for n, B in ((6, 16), (1024, 2)):
        ms = msgm(torch.randn(32, n), dense=False)
        y = torch.randn(B, n)
        t = torch.rand(B, 1)
        I, J, K = ms.IJK()
        out.update({f"sp{n}_I": I, f"sp{n}_J": J, f"sp{n}_K": K, f"sp{n}_V": ms.G_V, f"sp{n}_y": y, f"sp{n}_t": t,
                    f"sp{n}_f": ms.f(t, y), f"sp{n}_div": ms.div_Sigma(t, y), f"sp{n}_g": ms.g(t, y, sparse=True)})
    save("g05_drift_diffusion", **out)


def g06_emstep():
    torch.manual_seed(6)
    B, n = 8, 6
    mu, dW = torch.randn(B, n), torch.randn(B, n)
    sd, sn, ss = torch.rand(B, n), torch.randn(B, n, n), torch.randn(B, 2 * n)
    ms = msgm(torch.randn(32, n), dense=False)
    I, J, K = ms.IJK()
    save("g06_emstep", mu=mu, dW=dW, delta=np.float64(0.0625), sig_diag=sd, sig_dense=sn, sig_sparse=ss,
         out_diag=EMstep(mu, 0.0625, sd, dW), out_dense=EMstep(mu, 0.0625, sn, dW),
         out_sparse=EMstep(mu, 0.0625, ss, dW, sparse=True, I=I, K=K))


def _run_sampler(fn, sde, x0, steps, **kw):
    with Recorder() as r:
        xs = fn(sde, x0, num_steps=steps, **kw)
    z = torch.stack([d[1] for d in r.draws if d[0] == "randn_like"])
    return xs, z


def g07_samplers():
    torch.manual_seed(7)
    out = {}
    # SGM + MLP d=2
    net = MLP(2)
    rev = PluginReverseSDE(sgm(), net, Tparam())
    out.update({"sgm::" + k: v for k, v in sd_np(rev.state_dict()).items()})
    x0 = torch.randn(32, 2)
    out["sgm_x0"] = x0
    for tag, fn, steps in (("em", euler_maruyama_sampler, 8), ("heun", heun_sampler, 4), ("rk4", rk4_stratonovich_sampler, 4)):
        xs, z = _run_sampler(fn, rev, x0, steps, keep_all_samples=True, include_t0=True)
        out[f"sgm_{tag}_traj"], out[f"sgm_{tag}_z"] = xs, z
    xs, z = _run_sampler(euler_maruyama_sampler, rev, x0, 8, keep_all_samples=True, include_t0=False, lmbd=0.5)
    out["sgm_em_l05_traj"], out["sgm_em_l05_z"] = xs, z
    xs, z = _run_sampler(euler_maruyama_sampler, rev, x0, 8, keep_all_samples=False)
    out["sgm_em_final"], out["sgm_em_final_z"] = xs, z
    # MSGM sparse + MLP d=6 (NormalizeLogRadius), norm_correction on/off
    net6 = MLP(6, premodule="NormalizeLogRadius")
    ms = msgm(torch.randn(64, 6) * 1.5, dense=False)
    rev6 = PluginReverseSDE(ms, net6, Tparam())
    out.update({"sp::" + k: v for k, v in sd_np(rev6.state_dict()).items()})
    x0 = torch.randn(16, 6)
    out["sp_x0"] = x0
    for nc in (False, True):
        for tag, fn, steps in (("em", euler_maruyama_sampler, 8), ("heun", heun_sampler, 4), ("rk4", rk4_stratonovich_sampler, 4)):
            xs, z = _run_sampler(fn, rev6, x0, steps, keep_all_samples=True, include_t0=True, norm_correction=nc)
            out[f"sp_{tag}_nc{int(nc)}_traj"], out[f"sp_{tag}_nc{int(nc)}_z"] = xs, z
    # MSGM dense + MLP d=4
    net4 = MLP(4)
    xi = torch.randn(64, 4)
    md = msgm(xi, dense=True)
    rev4 = PluginReverseSDE(md, net4, Tparam())
    out.update({"dn::" + k: v for k, v in sd_np(rev4.state_dict()).items()})
    out["dn_G"] = md.G
    x0 = torch.randn(16, 4)
    out["dn_x0"] = x0
    for tag, fn, steps in (("em", euler_maruyama_sampler, 8), ("rk4", rk4_stratonovich_sampler, 4)):
        xs, z = _run_sampler(fn, rev4, x0, steps, keep_all_samples=True, include_t0=True, norm_correction=True)
        out[f"dn_{tag}_traj"], out[f"dn_{tag}_z"] = xs, z
    # forward process (noising) with RK4, as the driver does (MSGM_higherDim.py:783)
    xs, z = _run_sampler(rk4_stratonovich_sampler, forward_SDE(ms, Tparam()), out["sp_x0"], 4,
                         keep_all_samples=True, include_t0=True, norm_correction=True, lmbd=0.)
    out["sp_fwd_rk4_traj"], out["sp_fwd_rk4_z"] = xs, z
    # samplesToKeep error behaviour is tested on the host side; store a valid masked run
    keep = torch.tensor([1, 2, 3, 4] * 8, dtype=torch.int32)
    xs, z = _run_sampler(euler_maruyama_sampler, rev, out["sgm_x0"], 8, keep_all_samples=False, samplesToKeep=keep)
    out["sgm_em_keep_idx"], out["sgm_em_keep"], out["sgm_em_keep_z"] = keep, xs, z
    save("g07_samplers", **out)


def g08_sample_scheme():
    torch.manual_seed(8)
    out = {}
    for tag, dense, n in (("sp", False, 6), ("dn", True, 4)):
        ms = msgm(torch.randn(64, n), dense=dense, nsf=4)
        B = 12
        x0 = torch.randn(B, n)
        t = torch.tensor([0.001, 0.1, 0.24, 0.25, 0.3, 0.5, 0.74, 0.75, 0.99, 1.0, 0.6, 0.2]).reshape(B, 1)
        with Recorder() as r:
            y = ms.sample(t, x0)
        z_main = torch.stack([d[1] for d in r.draws[:4]])
        z_short = torch.zeros(B, n)
        k = torch.trunc(4 * t / ms.T).to(torch.int).reshape(-1)
        k[t.reshape(-1) >= 1.0] = 4
        rest = [d[1] for d in r.draws[4:]]
        rows0 = [b for b in range(B) if int(k[b]) == 0]
        assert len(rest) == len(rows0), (len(rest), rows0)
        for b, d in zip(rows0, rest):
            z_short[b] = d[0]
        out.update({f"{tag}_x0": x0, f"{tag}_t": t, f"{tag}_y": y, f"{tag}_k": k.to(torch.int32),
                    f"{tag}_z_main": z_main, f"{tag}_z_short": z_short})
        if dense:
            out["dn_G"] = ms.G
    save("g08_sample_scheme", **out)


def g09_nets():
    torch.manual_seed(9)
    out = {}
    # MLP — stored state (small)
    for tag, d, pre in (("mlp2", 2, None), ("mlp2n", 2, "NormalizeLogRadius"), ("mlp6n", 6, "NormalizeLogRadius"), ("mlp16", 16, None)):
        net = MLP(d, premodule=pre)
        x, t = torch.randn(64, d) * 1.5, torch.rand(64)
        out.update({f"{tag}::" + k: npy(v) for k, v in net.state_dict().items()})
        out.update({f"{tag}_x": x, f"{tag}_t": t, f"{tag}_out": net(x, t)})
    save("g09_mlp", **out)

    out = {}
    # UNet1D — deterministic fill, only I/O stored
    for tag, L, pre in (("u1d", 1024, None), ("u1dn", 1024, "NormalizeLogRadius"), ("u1d_odd", 1001, None), ("u1d_small", 64, None)):
        net = UNet1D(input_dim=L, base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, premodule=pre, emb_dim=128)
        load_det_(net)
        x, t = torch.randn(2, L), torch.rand(2)
        with torch.no_grad():
            y = net(x, t)
        out.update({f"{tag}_x": x, f"{tag}_t": t, f"{tag}_out": y})
    save("g09_unet1d", **out)

    out = {}
    for tag, S, pre, order in (("u2d16C", 16, None, "C"), ("u2d16F", 16, None, "F"), ("u2d16Fn", 16, "NormalizeLogRadius", "F"),
                               ("u2d32F", 32, None, "F")):
        net = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, premodule=pre, in_space=S,
                            attention_resolutions=(2, 4), flatten_order=order)
        load_det_(net)
        x, t = torch.randn(2, S * S) * 3, torch.rand(2)
        with torch.no_grad():
            y = net(x, t)
        out.update({f"{tag}_x": x, f"{tag}_t": t, f"{tag}_out": y})
    # 3-channel 64x64 core (config C4 shape) — the wrapper upstream is 1-channel only (NNUnet.py:177-179)
    core = UNetModelWithLogNorm(in_channels=3, model_channels=32, out_channels=3, in_space=64, num_res_blocks=2,
                                attention_resolutions=(2, 4), dropout=0.0, channel_mult=(1, 2, 4), conv_resample=True,
                                dims=2, num_classes=None, use_checkpoint=False, num_heads=1, use_scale_shift_norm=False,
                                learn_potential=False, use_log_norm=False)
    load_det_(core)
    x, t = torch.randn(1, 3, 64, 64), torch.rand(1)
    with torch.no_grad():
        y = core(x, timesteps=t)
    out.update(core64_x=x, core64_t=t, core64_out=y)
    save("g09_unet2d", **out)


def _grad_digest(named_grads):
    """Per-tensor L2 norm, sum, and the first 8 entries — enough to pin a
    4M-parameter gradient without committing 16 MB."""
    names = sorted(named_grads)
    norms = np.array([float(named_grads[k].double().norm()) for k in names])
    sums = np.array([float(named_grads[k].double().sum()) for k in names])
    heads = np.stack([np.pad(npy(named_grads[k].reshape(-1)[:8]), (0, max(0, 8 - named_grads[k].numel()))) for k in names])
    return dict(names=np.array(names), norms=norms, sums=sums, heads=heads)


def _ssm_case(rev, x, u_t, eps, u_v, full_grads):
    """Run the reference ssm() with the three draws forced."""
    seq = [u_t, eps, u_v] if eps is not None else None
    o = (torch.rand, torch.randn_like)
    it = iter(seq)
    torch.rand = lambda *a, **k: next(it).clone()
    torch.randn_like = lambda *a, **k: next(it).clone()
    try:
        rev.zero_grad()
        per = rev.ssm(x)
        per.mean().backward()
    finally:
        torch.rand, torch.randn_like = o
    grads = {k: p.grad.detach().clone() for k, p in rev.named_parameters() if p.grad is not None}
    res = dict(per=per.detach(), loss=per.mean().detach())
    if full_grads:
        res.update({"grad::" + k: v for k, v in grads.items()})
    else:
        res.update({"gd_" + k: v for k, v in _grad_digest(grads).items()})
    return res


def g10_ssm():
    torch.manual_seed(10)
    out = {}
    B = 64
    for tag, d, pre in (("mlp2", 2, None), ("mlp6n", 6, "NormalizeLogRadius")):
        net = MLP(d, premodule=pre)
        rev = PluginReverseSDE(sgm(), net, Tparam())
        x, u_t, eps, u_v = torch.randn(B, d) * 1.5, torch.rand(B, 1), torch.randn(B, d), torch.rand(B, d)
        res = _ssm_case(rev, x, u_t, eps, u_v, full_grads=True)
        out.update({f"{tag}::" + k: v for k, v in sd_np(rev.state_dict()).items()})
        out.update({f"{tag}_x": x, f"{tag}_u_t": u_t, f"{tag}_eps": eps, f"{tag}_u_v": u_v})
        out.update({f"{tag}_{k}": v for k, v in res.items()})
    save("g10_ssm_mlp", **out)

    out = {}
    net = UNet1D(input_dim=256, base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, premodule=None, emb_dim=128)
    load_det_(net)
    rev = PluginReverseSDE(sgm(), net, Tparam())
    B, d = 4, 256
    x, u_t, eps, u_v = torch.randn(B, d), torch.rand(B, 1), torch.randn(B, d), torch.rand(B, d)
    res = _ssm_case(rev, x, u_t, eps, u_v, full_grads=False)
    out.update(u1d_x=x, u1d_u_t=u_t, u1d_eps=eps, u1d_u_v=u_v)
    out.update({f"u1d_{k}": v for k, v in res.items()})
    net = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, premodule=None, in_space=16,
                        attention_resolutions=(2, 4), flatten_order="F")
    load_det_(net)
    rev = PluginReverseSDE(sgm(), net, Tparam())
    B, d = 2, 256
    x, u_t, eps, u_v = torch.randn(B, d) * 3, torch.rand(B, 1), torch.randn(B, d), torch.rand(B, d)
    res = _ssm_case(rev, x, u_t, eps, u_v, full_grads=False)
    out.update(u2d_x=x, u2d_u_t=u_t, u2d_eps=eps, u2d_u_v=u_v)
    out.update({f"u2d_{k}": v for k, v in res.items()})
    save("g10_ssm_unets", **out)


def g14_ssm_msgm():
    """SSM loss of the multiplicative SDE (sparse + dense tensor) with an MLP: ssm_loss(t, x, y) with the
    probe draw forced (SDEs.py:616-646)."""
    torch.manual_seed(14)
    out = {}
    B = 48
    for tag, d, dense, pre in (("sp", 6, False, "NormalizeLogRadius"), ("dn", 4, True, None)):
        net = MLP(d, premodule=pre)
        base = msgm(torch.randn(64, d) * 1.5, dense=dense, nsf=4)
        rev = PluginReverseSDE(base, net, Tparam())
        t_ = torch.rand(B, 1).clamp_min(1e-3)
        y = torch.randn(B, d) * 1.3
        u_v = torch.rand(B, d)
        o = torch.rand
        torch.rand = lambda *a, **k: u_v.clone()
        try:
            rev.zero_grad()
            yy = y.clone().requires_grad_(True)
            per = rev.ssm_loss(t_, y, yy)
            per.mean().backward()
        finally:
            torch.rand = o
        out.update({f"{tag}::" + k: v for k, v in sd_np(rev.state_dict()).items()})
        out.update({f"{tag}_t": t_, f"{tag}_y": y, f"{tag}_u_v": u_v, f"{tag}_per": per.detach()})
        out.update({f"{tag}_grad::" + k: p.grad.detach().clone() for k, p in rev.named_parameters() if p.grad is not None})
        if dense:
            out["dn_G"] = base.G
    save("g14_ssm_msgm", **out)


def g15_metrics():
    """Reporting metrics next to the hot path: RBF-kernel MMD (quantitative_comparison.py:22-46),
    Gaussian latent log-density (SDEs.py:209-215) and the ELBO slice estimate (SDEs.py:708-721) with every draw
    recorded in call order."""
    from quantitative_comparison import compute_kernel, compute_mmd
    torch.manual_seed(15)
    out = {}
    for tag, nx, ny, d in (("a", 37, 53, 2), ("b", 64, 40, 7), ("c", 20, 20, 300)):
        x, y = torch.randn(nx, d) * 1.3, torch.randn(ny, d) * 0.9 + 0.4
        out.update({f"mmd_{tag}_x": x, f"mmd_{tag}_y": y, f"mmd_{tag}_Kxy": compute_kernel(x, y),
                    f"mmd_{tag}": compute_mmd(x, y).reshape(1)})
    yT = torch.randn(19, 5) * 1.7
    out.update(lp_y=yT, lp=sgm().log_latent_pdf(yT))
    B, d = 96, 2
    net = MLP(d)
    rev = PluginReverseSDE(sgm(), net, Tparam())
    x = torch.randn(B, d) * 1.5
    with Recorder() as r:
        elbo = rev.elbo_random_t_slice(x)
    out.update({"elbo::" + k: v for k, v in sd_np(rev.state_dict()).items()})
    out.update(elbo_x=x, elbo=elbo.detach())
    for i, (kind, val) in enumerate(r.draws):
        out[f"elbo_draw{i}_{kind}"] = val
    save("g15_metrics", **out)


def g11_train3():
    torch.manual_seed(11)
    B, d, steps = 128, 2, 3
    net = MLP(d)
    rev = PluginReverseSDE(sgm(), net, Tparam())
    opt = torch.optim.Adam(rev.parameters(), lr=1e-3)
    out = {"init::" + k: npy(v).copy() for k, v in rev.state_dict().items() if k not in ("T", "base_sde.T")}
    xs, uts, epss, uvs, losses = [], [], [], [], []
    for i in range(steps):
        x, u_t, eps, u_v = torch.randn(B, d) * 1.5, torch.rand(B, 1), torch.randn(B, d), torch.rand(B, d)
        seq = iter([u_t, eps, u_v])
        o = (torch.rand, torch.randn_like)
        torch.rand = lambda *a, **k: next(seq).clone()
        torch.randn_like = lambda *a, **k: next(seq).clone()
        try:
            opt.zero_grad()
            loss = rev.ssm(x).mean()
            loss.backward()
            opt.step()
        finally:
            torch.rand, torch.randn_like = o
        xs.append(x); uts.append(u_t); epss.append(eps); uvs.append(u_v); losses.append(loss.detach())
    out.update(x=torch.stack(xs), u_t=torch.stack(uts), eps=torch.stack(epss), u_v=torch.stack(uvs), loss=torch.stack(losses))
    out.update({"final::" + k: npy(v) for k, v in rev.state_dict().items() if k not in ("T", "base_sde.T")})
    save("g11_train3", **out)


def g12_embedding():
    t = torch.cat([torch.linspace(0, 1, 33), torch.tensor([-13.8, -2.5, -0.3, 0.7, 3.1])])
    save("g12_embedding", t=t, emb32=timestep_embedding(t, 32), emb7=timestep_embedding(t, 7))


def g13_misc():
    torch.manual_seed(13)
    with Recorder() as r:
        v = sample_rademacher((32, 5), "cpu")
    u = r.draws[0][1]
    with Recorder() as r:
        s = randu_on_sphere((32, 5), "cpu")
    z = r.draws[0][1]
    # MSGM latent sample (ecdf + log map)                                   SDEs.py:438-471
    xi = torch.randn(500, 6) * 2
    ms = msgm(xi, dense=False)
    with Recorder() as r:
        x0 = ms.latent_sample(40, 6)
    save("g13_misc", rad_u=u, rad_v=v, sph_z=z, sph_s=s, lat_xinit=xi, lat_rT=ms.r_T, lat_u=r.draws[0][1],
         lat_z=r.draws[1][1], lat_x0=x0)


def g16_round2():
    """Round-2 pins: (a) the reference integrators driving the 2-D U-Net (sde_scheme.py:43-99,174-269 x
    NNUnet.py:195-245) with recorded noise; (b) a 256-step MLP Euler-Maruyama run (error growth over a long
    reverse-SDE trajectory); (c) the SSM loss with the Gaussian and the sphere probe (SDEs.py:517-536)."""
    torch.manual_seed(16)
    out = {}
    net = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, premodule=None, in_space=16,
                        attention_resolutions=(2, 4), flatten_order="F")
    load_det_(net)
    rev = PluginReverseSDE(sgm(), net, Tparam())
    x0 = torch.randn(4, 256)
    out["u2d_x0"] = x0
    with torch.no_grad():
        xs, z = _run_sampler(euler_maruyama_sampler, rev, x0, 8, keep_all_samples=True, include_t0=True)
        out["u2d_em_traj"], out["u2d_em_z"] = xs, z
        xs, z = _run_sampler(rk4_stratonovich_sampler, rev, x0, 4, keep_all_samples=True, include_t0=True)
        out["u2d_rk4_traj"], out["u2d_rk4_z"] = xs, z
        xs, z = _run_sampler(heun_sampler, rev, x0, 4, keep_all_samples=True, include_t0=True)
        out["u2d_heun_traj"], out["u2d_heun_z"] = xs, z
    # (b) long MLP trajectory: every 32nd state of 256 EM steps
    netm = MLP(2)
    revm = PluginReverseSDE(sgm(), netm, Tparam())
    out.update({"mlp::" + k: v for k, v in sd_np(revm.state_dict()).items()})
    x0 = torch.randn(16, 2)
    with torch.no_grad():
        xs, z = _run_sampler(euler_maruyama_sampler, revm, x0, 256, keep_all_samples=True, include_t0=True)
    out["mlp_x0"], out["mlp_em256_z"], out["mlp_em256_every32"] = x0, z, xs[::32]
    # (c) SSM with the two non-Rademacher probes
    B, d = 48, 2
    for vt in ("gaussian", "uniform"):
        revv = PluginReverseSDE(sgm(), netm, Tparam(), vtype=vt)
        x = torch.randn(B, d) * 1.5
        with Recorder() as r:
            revv.zero_grad()
            per = revv.ssm(x)
            per.mean().backward()
        kinds = [k for k, _ in r.draws]
        assert kinds == ["rand", "randn_like", "randn"], kinds
        u_t, eps, zv = (t for _, t in r.draws)
        out.update({f"ssm_{vt}_x": x, f"ssm_{vt}_u_t": u_t, f"ssm_{vt}_eps": eps, f"ssm_{vt}_zv": zv, f"ssm_{vt}_per": per.detach()})
        out.update({f"ssm_{vt}_grad::" + k: p.grad.detach().clone() for k, p in revv.named_parameters() if p.grad is not None})
    # (d) SGMsde.sample(t, y0) with times BELOW t_epsilon: upstream uses t as given, no clamp (SDEs.py:134-146,196-199)
    s0 = sgm()
    x0 = torch.randn(8, 5)
    t = torch.tensor([1e-5, 1e-4, 5e-4, 9.99e-4, 1e-3, 2e-3, 0.5, 1.0]).reshape(8, 1)
    with Recorder() as r:
        y = s0.sample(t, x0)
    out.update(smallt_x0=x0, smallt_t=t, smallt_eps=r.draws[0][1], smallt_y=y)
    save("g16_round2", **out)


def g17_ssm_wellconditioned():
    """VERDICT r2 #5a: SSM per-sample loss + gradient digests of the reference's VorticityUNet at 32x32 and at 64x64
    (attention at T = 1024 / 256, i.e. the C4 network's attention shapes) on a WELL-CONDITIONED parameter set
    (oracle.det_params.load_init_like_: the statistics of the reference's default init, zero-init layers re-randomised
    small) — the fixture the HIP path is held to with an ABSOLUTE tolerance."""
    torch.manual_seed(17)
    out = {}
    for tag, S_, B in (("w32", 32, 2), ("w64", 64, 2)):
        net = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, premodule=None, in_space=S_,
                            attention_resolutions=(2, 4), flatten_order="F")
        load_init_like_(net)
        rev = PluginReverseSDE(sgm(), net, Tparam())
        d = S_ * S_
        x, u_t, eps, u_v = torch.randn(B, d) * 3, torch.rand(B, 1), torch.randn(B, d), torch.rand(B, d)
        res = _ssm_case(rev, x, u_t, eps, u_v, full_grads=False)
        out.update({f"{tag}_x": x, f"{tag}_u_t": u_t, f"{tag}_eps": eps, f"{tag}_u_v": u_v})
        out.update({f"{tag}_{k}": v for k, v in res.items()})
        with torch.no_grad():
            t = torch.full((B,), 0.37)
            out[f"{tag}_fwd_t"], out[f"{tag}_fwd"] = t, net(x, t)
        print(tag, "loss", float(res["loss"]), "per", res["per"].tolist())
    save("g17_ssm_wellconditioned", **out)


G18_FULL = ("core.input_blocks.4.1.", "core.input_blocks.7.1.", "core.middle_block.1.")   # first encoder attention per level + middle
G18_COLS = 16      # weight gradients: every row (all heads' q / k / v rows of qkv, all output channels of proj_out), 16 input columns


def g18_multihead():
    """Multi-head attention (AttentionBlock num_heads = H, model/unet.py:220-250): the reference's VorticityUNet(num_heads=H)
    on the well-conditioned parameter set (load_init_like_: proj_out re-randomised small, so the attention branch reaches the
    output and the q / k / v gradients are not zero).  in_space 32 at H = 2 / 4 (attention at T = 256, C = 64 and T = 64,
    C = 128: D = 32 / 16 and 64 / 32), in_space 16 at H = 2 (T = 16: the composed per-head path).  Forward at a fixed t, the
    SSM per-sample loss with the three draws forced, the gradients of the attention parameters (norm, qkv, proj_out) of the
    first encoder attention block of each level and of the middle block — the vectors in full, the two (rows, C, 1) weights
    with every row and the G18_COLS input columns arange(0, C, C / G18_COLS) (stored next to them as _cols::), which are
    spread over all heads; the whole weights would make the file 1.8 MB — and digests of all gradients."""
    torch.manual_seed(18)
    out = {}
    for tag, S_, H, B in (("s32h2", 32, 2, 2), ("s32h4", 32, 4, 2), ("s16h2", 16, 2, 2)):
        net = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, premodule=None, in_space=S_,
                            attention_resolutions=(2, 4), num_heads=H, flatten_order="F")
        load_init_like_(net)
        rev = PluginReverseSDE(sgm(), net, Tparam())
        d = S_ * S_
        x, u_t, eps, u_v = torch.randn(B, d) * 3, torch.rand(B, 1), torch.randn(B, d), torch.rand(B, d)
        res = _ssm_case(rev, x, u_t, eps, u_v, full_grads=True)
        grads = {k[len("grad::"):]: v for k, v in res.items() if k.startswith("grad::")}
        full = {k: v for k, v in grads.items() if k[len("a."):].startswith(G18_FULL)}
        assert len(full) == 3 * 6 and all(float(v.norm()) > 0 for v in full.values()), sorted(full)
        out.update({f"{tag}_x": x, f"{tag}_u_t": u_t, f"{tag}_eps": eps, f"{tag}_u_v": u_v, f"{tag}_heads": np.array(H),
                    f"{tag}_per": res["per"], f"{tag}_loss": res["loss"]})
        for k, v in full.items():
            if v.dim() == 3:                                   # (rows, C, 1) conv1d weight: a fixed set of input columns
                cols = torch.arange(0, v.shape[1], v.shape[1] // G18_COLS)
                out[f"{tag}_cols::{k}"], v = cols, v[:, cols]
            out[f"{tag}_grad::{k}"] = v
        out.update({f"{tag}_gd_{k}": v for k, v in _grad_digest(grads).items()})
        with torch.no_grad():
            t = torch.full((B,), 0.37)
            out[f"{tag}_fwd_t"], out[f"{tag}_fwd"] = t, net(x, t)
        print(tag, "loss", float(res["loss"]), "per", res["per"].tolist())
    save("g18_multihead", **out)


G19_FULL = ("core.input_blocks.1.0.", "core.input_blocks.4.0.", "core.input_blocks.7.0.", "core.output_blocks.0.0.")
G19_PARTS = ("out_layers.0.", "out_layers.3.", "in_layers.2.")
G19_SUB = 16       # (Co, Ci, 3, 3) weight gradients: G19_SUB output rows x G19_SUB input columns, evenly spaced


def _force_dropout(net, seed, offset, row_base, p):
    """Replace the forward of every reference Dropout (ResBlock out_layers[2], model/unet.py:152-158) by a multiply with the
    mask the rule gives for that ResBlock's index l (its position among all ResBlocks in named_modules() order) at
    (seed, offset, row_base) — tests/philox_np.py, the restatement the tests use.  Returns the indices in order."""
    import philox_np as PX
    from model.unet import ResBlock as RefResBlock
    blocks = [m for m in net.modules() if isinstance(m, RefResBlock)]
    for l, blk in enumerate(blocks):
        drop = blk.out_layers[2]
        assert isinstance(drop, torch.nn.Dropout) and drop.p == p

        def fwd(h, l=l):
            B, C, H, W = h.shape
            return h * torch.from_numpy(PX.dropout_multiplier(seed, offset, row_base, l, p, B, H, W, C)).to(h.dtype)
        drop.forward = fwd
    return len(blocks)


def _g19_store(out, tag, grads, detail):
    if detail:
        full = {k: v for k, v in grads.items() if k[len("a."):].startswith(G19_FULL) and
                k[len("a."):].split(".", 4)[-1].startswith(G19_PARTS)}
        assert len(full) == 4 * 6 and all(float(v.norm()) > 0 for v in full.values()), sorted(full)
        for k, v in full.items():
            if v.dim() == 4:
                rows = torch.arange(0, v.shape[0], max(1, v.shape[0] // G19_SUB))
                cols = torch.arange(0, v.shape[1], max(1, v.shape[1] // G19_SUB))
                out[f"{tag}_rows::{k}"], out[f"{tag}_cols::{k}"] = rows, cols
                v = v[rows][:, cols]
            out[f"{tag}_grad::{k}"] = v
    out.update({f"{tag}_gd_{k}": v for k, v in _grad_digest(grads).items()})


def g19_dropout():
    """Dropout(p) in every ResBlock's out_layers (model/unet.py:152-158): the reference's VorticityUNet(dropout=p) in TRAIN
    mode on the well-conditioned fill, each Dropout forced to the mask rule (include/msgm_hip.h, msgm_dropout_t) at a
    recorded (seed, offset) and at row_base 0 and 4.  Cases: in_space 32, p = 0.1, SGM (ssm with the three draws forced);
    in_space 16, p = 0.3, NormalizeLogRadius, the MSGM sparse SDE (ssm_loss(t, x, y) with the probe forced, as g14).  Stored:
    the per-sample loss, the gradients of out_layers.{0,3} and in_layers.2 of the first ResBlock of each level and of the
    first decoder block (skip conv) — vectors in full, conv weights at G19_SUB rows x G19_SUB columns (_rows:: / _cols::) —
    at row_base 0, digests of all gradients at both row_bases, and one train-mode forward at a fixed t (row_base 0)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    torch.manual_seed(19)
    out = {}
    seed, off_ssm, off_fwd = 0x5DE5_1234_9ABC, 3, 8
    for tag, S_, p, pre, kind in (("s32", 32, 0.1, None, "sgm"), ("s16m", 16, 0.3, "NormalizeLogRadius", "sparse")):
        B, d = 2, S_ * S_
        net = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, dropout=p, premodule=pre, in_space=S_,
                            attention_resolutions=(2, 4), flatten_order="F")
        load_init_like_(net)
        net.train()
        if kind == "sgm":
            rev = PluginReverseSDE(sgm(), net, Tparam())
            x, u_t, eps, u_v = torch.randn(B, d) * 3, torch.rand(B, 1), torch.randn(B, d), torch.rand(B, d)
            out.update({f"{tag}_x": x, f"{tag}_u_t": u_t, f"{tag}_eps": eps, f"{tag}_u_v": u_v})
        else:
            base = msgm(torch.randn(64, d) * 1.5, dense=False, nsf=4)
            rev = PluginReverseSDE(base, net, Tparam())
            t_, y, u_v = torch.rand(B, 1).clamp_min(1e-3), torch.randn(B, d) * 1.3, torch.rand(B, d)
            out.update({f"{tag}_t": t_, f"{tag}_y": y, f"{tag}_u_v": u_v})
            out.update({f"{tag}_base::" + k: v for k, v in sd_np(rev.state_dict()).items() if not k.startswith("a.")})
        for rb in (0, 4):
            nl = _force_dropout(net, seed, off_ssm, rb, p)
            if kind == "sgm":
                res = _ssm_case(rev, x, u_t, eps, u_v, full_grads=True)
                per = res["per"]
                grads = {k[len("grad::"):]: v for k, v in res.items() if k.startswith("grad::")}
            else:
                o = torch.rand
                torch.rand = lambda *a, **k: u_v.clone()
                try:
                    rev.zero_grad()
                    per = rev.ssm_loss(t_, y, y.clone().requires_grad_(True))
                    per.mean().backward()
                finally:
                    torch.rand = o
                per = per.detach()
                grads = {k: q.grad.detach().clone() for k, q in rev.named_parameters() if q.grad is not None}
            out[f"{tag}_rb{rb}_per"] = per
            _g19_store(out, f"{tag}_rb{rb}", grads, detail=rb == 0)
            print(tag, "row_base", rb, "per", per.tolist(), "ResBlocks", nl)
        out.update({f"{tag}_p": np.array(p), f"{tag}_seed": np.array(seed, dtype=np.int64),
                    f"{tag}_offset": np.array(off_ssm, dtype=np.int64), f"{tag}_fwd_offset": np.array(off_fwd, dtype=np.int64)})
        _force_dropout(net, seed, off_fwd, 0, p)
        with torch.no_grad():
            xf = torch.randn(B, d) * 3
            t = torch.full((B,), 0.37)
            out[f"{tag}_fwd_x"], out[f"{tag}_fwd_t"], out[f"{tag}_fwd"] = xf, t, net(xf, t)
    save("g19_dropout", **out)


def g20_mlp_wide():
    """The MLP at 31 <= d <= 128 (the extra-wide kernel class).  Weights are rebuilt from oracle.det_params
    (load_init_like_ on the reference module) and not stored; only their names and shapes are, so the port's
    state_dict layout can be checked without a GPU."""
    torch.manual_seed(20)
    out = {}

    def net_of(d, pre):
        net = MLP(d, premodule=pre)
        load_init_like_(net)
        return net

    for tag, d, pre in (("f31", 31, None), ("f32", 32, None), ("f64n", 64, "NormalizeLogRadius"), ("f128", 128, None)):
        net = net_of(d, pre)
        x, t = torch.randn(40, d) * 1.5, torch.rand(40)
        with torch.no_grad():
            y = net(x, t)
        out.update({f"{tag}_x": x, f"{tag}_t": t, f"{tag}_out": y})
        out[f"{tag}_names"] = np.array(list(net.state_dict()))
        out[f"{tag}_shapes"] = np.array([list(v.shape) + [0] * (2 - v.dim()) for v in net.state_dict().values()])
    # ssm(x): full gradients at d = 32, the digest at d = 128 with premodule
    for tag, d, pre, B, full in (("s32", 32, None, 48, True), ("s128n", 128, "NormalizeLogRadius", 40, False)):
        rev = PluginReverseSDE(sgm(), net_of(d, pre), Tparam())
        x, u_t, eps, u_v = torch.randn(B, d) * 1.5, torch.rand(B, 1), torch.randn(B, d), torch.rand(B, d)
        res = _ssm_case(rev, x, u_t, eps, u_v, full_grads=full)
        out.update({f"{tag}_x": x, f"{tag}_u_t": u_t, f"{tag}_eps": eps, f"{tag}_u_v": u_v})
        out.update({f"{tag}_{k}": v for k, v in res.items()})
    # ssm_loss(t, x, y) of the multiplicative SDE: dense tensor at d = 32, sparse at d = 128
    for tag, d, dense, B in (("m32d", 32, True, 32), ("m128s", 128, False, 24)):
        xi = torch.randn(64, d) * 1.5
        base = msgm(xi, dense=dense, nsf=4)
        rev = PluginReverseSDE(base, net_of(d, None), Tparam())
        t_ = torch.rand(B, 1).clamp_min(1e-3)
        y = torch.randn(B, d) * 1.3
        u_v = torch.rand(B, d)
        o = torch.rand
        torch.rand = lambda *a, **k: u_v.clone()
        try:
            rev.zero_grad()
            per = rev.ssm_loss(t_, y, y.clone().requires_grad_(True))
            per.mean().backward()
        finally:
            torch.rand = o
        grads = {k: p.grad.detach().clone() for k, p in rev.named_parameters() if p.grad is not None}
        out.update({f"{tag}_t": t_, f"{tag}_y": y, f"{tag}_u_v": u_v, f"{tag}_per": per.detach(),
                    f"{tag}_x_init": xi})
        out.update({f"{tag}_gd_" + k: v for k, v in _grad_digest(grads).items()})
        if dense:
            out[f"{tag}_G"] = base.G
    # three SSM + Adam steps at d = 32 (as g11)
    B, d = 64, 32
    rev = PluginReverseSDE(sgm(), net_of(d, None), Tparam())
    opt = torch.optim.Adam(rev.parameters(), lr=1e-3)
    xs, uts, epss, uvs, losses = [], [], [], [], []
    for i in range(3):
        x, u_t, eps, u_v = torch.randn(B, d) * 1.5, torch.rand(B, 1), torch.randn(B, d), torch.rand(B, d)
        seq = iter([u_t, eps, u_v])
        o = (torch.rand, torch.randn_like)
        torch.rand = lambda *a, **k: next(seq).clone()
        torch.randn_like = lambda *a, **k: next(seq).clone()
        try:
            opt.zero_grad()
            loss = rev.ssm(x).mean()
            loss.backward()
            opt.step()
        finally:
            torch.rand, torch.randn_like = o
        xs.append(x); uts.append(u_t); epss.append(eps); uvs.append(u_v); losses.append(loss.detach())
    out.update(tr_x=torch.stack(xs), tr_u_t=torch.stack(uts), tr_eps=torch.stack(epss), tr_u_v=torch.stack(uvs),
               tr_loss=torch.stack(losses))
    out.update({"tr_final_gd_" + k: v for k, v in _grad_digest({k: v for k, v in rev.state_dict().items()
                                                              if k not in ("T", "base_sde.T")}).items()})
    save("g20_mlp_wide", **out)


def g21_kde():
    """Latent log-density and ELBO of the multiplicative SDE: the sklearn KernelDensity of the radii (SDEs.py:239-265,
    503-509) on CPU.  Density cases (a) norm_map=None with cst_log_dens estimated, (b) norm_map="log" without (the driver's
    configuration, MSGM_higherDim.py:57): Ns = 257 rows of d = 4, a query batch of 65 rows of which some are scaled by
    10 and by 0.01 (far outside the samples).  lp64 is the estimator's own float64 output at the fp32 row norms, before
    upstream's cast to float32.  ELBO cases shaped like g14: ssm_loss(t, x, y) with the probe forced, yT from
    cond_latent_sample, elbo = lp - per * T (SDEs.py:708-721)."""
    torch.manual_seed(21)
    out = {}
    for tag, norm_map, estim in (("a", None, True), ("b", "log", False)):
        y0 = torch.randn(257, 4) * 1.5
        base = MSGMsde(y0, beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=Tparam(), num_steps_forward=4, device="cpu",
                       estim_cst_norm_dens_r_T=estim, norm_sampler="ecdf", norm_map=norm_map, denseTensor=False,
                       plot_validate=False)
        yT = torch.randn(65, 4) * 1.5
        yT[40:52] *= 10.0
        yT[52:] *= 0.01
        r_yT = torch.linalg.norm(yT, dim=1).reshape(-1, 1)
        out.update({f"{tag}_y0": y0, f"{tag}_r_T": base.r_T, f"{tag}_bandwidth": np.float64(base.kde.bandwidth),
                    f"{tag}_cst_log_dens": torch.as_tensor(base.cst_log_dens, dtype=torch.float32).reshape(1),
                    f"{tag}_yT": yT, f"{tag}_lp": base.log_latent_pdf(yT),
                    f"{tag}_lp64": np.asarray(base.kde.score_samples(r_yT.numpy()), dtype=np.float64)})
    B = 48
    for tag, d, dense, pre in (("sp", 6, False, "NormalizeLogRadius"), ("dn", 4, True, None)):
        net = MLP(d, premodule=pre)
        y0 = torch.randn(64, d) * 1.5
        base = msgm(y0, dense=dense, nsf=4)
        rev = PluginReverseSDE(base, net, Tparam())
        x = torch.randn(B, d) * 1.5
        t_ = torch.rand(B, 1).clamp_min(1e-3)
        y = torch.randn(B, d) * 1.3
        u_v = torch.rand(B, d)
        o = torch.rand
        torch.rand = lambda *a, **k: u_v.clone()
        try:
            per = rev.ssm_loss(t_, x, y.clone().requires_grad_(True)).detach()
        finally:
            torch.rand = o
        yT = rev.cond_latent_sample(t_, base.T, x)
        lp = base.log_latent_pdf(yT).view(B, -1).sum(1)
        out.update({f"{tag}::" + k: v for k, v in sd_np(rev.state_dict()).items()})
        out.update({f"{tag}_y0": y0, f"{tag}_x": x, f"{tag}_t": t_, f"{tag}_y": y, f"{tag}_u_v": u_v, f"{tag}_per": per,
                    f"{tag}_yT": yT, f"{tag}_lp": lp, f"{tag}_elbo": lp - per * rev.T})
        if dense:
            out["dn_G"] = base.G
    save("g21_kde", **out)


def g22_unet1d_deep():
    """The reference's UNet1D where every level counts (load_init_like_(gain=3.0): tests/unet1d_deep.py) at lengths that are
    no multiple of 8 — cases B (L = 37), C (37 + NormalizeLogRadius), D (9 + NormalizeLogRadius: middle block at one position)
    and G (13, two levels, 16 | 32 channels, emb 32): forward output, the three forced SSM draws, per-sample loss and the
    gradient digest.  The weights are the closed form, not stored."""
    out = {}
    for tag, L, B, pre, base, mults, emb in (("B", 37, 3, None, 32, (1, 2, 4), 128), ("C", 37, 3, "NormalizeLogRadius", 32, (1, 2, 4), 128),
                                             ("D", 9, 3, "NormalizeLogRadius", 32, (1, 2, 4), 128),
                                             ("G", 13, 3, "NormalizeLogRadius", 16, (1, 2), 32)):
        net = UNet1D(input_dim=L, base_channels=base, channel_mults=mults, num_res_blocks=2, premodule=pre, emb_dim=emb)
        load_init_like_(net, gain=3.0)
        rev = PluginReverseSDE(sgm(), net, Tparam())
        torch.manual_seed(L)
        x, u_t, eps, u_v = torch.randn(B, L) * 3, torch.rand(B), torch.randn(B, L), torch.rand(B, L)
        u_t = u_t.reshape(B, 1)
        res = _ssm_case(rev, x, u_t, eps, u_v, full_grads=False)
        out.update({f"{tag}_x": x, f"{tag}_u_t": u_t, f"{tag}_eps": eps, f"{tag}_u_v": u_v})
        out.update({f"{tag}_{k}": v for k, v in res.items()})
        torch.manual_seed(1000 + L)
        xf, t = torch.randn(5, L) * 3, torch.rand(5) * 0.9 + 0.05
        with torch.no_grad():
            out[f"{tag}_fwd_x"], out[f"{tag}_fwd_t"], out[f"{tag}_fwd"] = xf, t, net(xf, t)
        print(tag, "loss", float(res["loss"]), "per", res["per"].tolist())
    save("g22_unet1d_deep", **out)


G23_FULL = ("a.core.output_blocks.0.0.in_layers.0.weight", "a.core.output_blocks.0.0.in_layers.0.bias")
G23_NETS = (("W64", 64, (1, 2, 4)), ("D4", 32, (1, 2, 4, 8)))


def g23_unet2d_wide():
    """The reference's VorticityUNet wider than the driver's: W64 (base_channels 64, (1, 2, 4)) and D4 (32, (1, 2, 4, 8)) at
    in_space 16, B = 2, on the well-conditioned parameter set (load_init_like_).  Both have a widest GroupNorm of 512
    channels, the in-norm of output_blocks.0 over cat([h, skip]).  Forward at t = 0.37, the per-sample SSM loss with the
    three draws forced, digests of all gradients, the gradients of that widest norm's weight and bias in full, and the
    parameter names and shapes — the weights are the closed form, not stored."""
    torch.manual_seed(23)
    out = {}
    for tag, base, mults in G23_NETS:
        net = VorticityUNet(base_channels=base, channel_mults=mults, num_res_blocks=2, premodule=None, in_space=16,
                            attention_resolutions=(2, 4), flatten_order="F")
        load_init_like_(net)
        rev = PluginReverseSDE(sgm(), net, Tparam())
        B, d = 2, 256
        x, u_t, eps, u_v = torch.randn(B, d) * 3, torch.rand(B, 1), torch.randn(B, d), torch.rand(B, d)
        res = _ssm_case(rev, x, u_t, eps, u_v, full_grads=True)
        grads = {k[len("grad::"):]: v for k, v in res.items() if k.startswith("grad::")}
        out.update({f"{tag}_x": x, f"{tag}_u_t": u_t, f"{tag}_eps": eps, f"{tag}_u_v": u_v, f"{tag}_per": res["per"],
                    f"{tag}_loss": res["loss"]})
        for k in G23_FULL:
            assert grads[k].numel() == 512 and float(grads[k].norm()) > 0, k
            out[f"{tag}_grad::{k}"] = grads[k]
        out.update({f"{tag}_gd_{k}": v for k, v in _grad_digest(grads).items()})
        sd = {k: v for k, v in net.state_dict().items()}
        out[f"{tag}_param_names"] = np.array(sorted(sd))
        out[f"{tag}_param_shapes"] = np.array([",".join(str(int(s)) for s in sd[k].shape) for k in sorted(sd)])
        with torch.no_grad():
            t = torch.full((B,), 0.37)
            out[f"{tag}_fwd_t"], out[f"{tag}_fwd"] = t, net(x, t)
        print(tag, "parameters", sum(v.numel() for v in sd.values()), "loss", float(res["loss"]), "per", res["per"].tolist())
    save("g23_unet2d_wide", **out)


def _tap(obj, name, log):
    """Record what obj.name(...) returns (an instance attribute over the method; the reference is not edited)."""
    fn = getattr(obj, name)

    def f(*a, **k):
        out = fn(*a, **k)
        log.append(out)
        return out
    setattr(obj, name, f)


def g24_ssm_intT():
    """The time-integrated SSM loss, PluginReverseSDE(ssm_intT=True) (SDEs.py:648-706): one RK4 path of the forward process
    per row, every grid state with t > t_epsilon a training row, time-major.  B = 3, nsf = 4, T = 1 (grid 0.25 .. 1).
    MLP cases sp (sparse tensor, d = 6, NormalizeLogRadius) and dn (dense, d = 4), each with t_epsilon = 0.3 (`drop`: the
    first grid time goes) and 1e-3 (`all`): x, the path noise eps (nsf, B, d), the probe uniforms u_v, then (t, y) of
    sample_txy, the per-row losses and the parameter gradients of their mean.  One elbo_random_t_slice / evaluate case per
    SDE family (sg additive d = 2, sp, dn; t_epsilon = 1e-3): upstream draws a second path there only to tile x, then the
    latent sample; stored are the first path's noise, u_v, yT, the latent term, the ELBO rows and evaluate's two numbers."""
    import SDEs as ref_sdes
    import NN as ref_nn
    # upstream's sample_t_linspace (SDEs.py:700) names a global `device` that exists in the driver module and not in SDEs.py:
    # the one defect of ssm_intT.  Supplied from outside, the reference itself stays as it is.
    ref_sdes.device = torch.device("cpu")
    torch.manual_seed(24)
    out = {}
    B, nsf = 3, 4

    def family(tag, d, dense, pre):
        y0 = torch.randn(64, d) * 1.5
        base = sgm(nsf) if tag == "sg" else msgm(y0, dense=dense, nsf=nsf)
        net = MLP(d, premodule=pre)
        load_det_(net)                               # the closed-form weights: not stored
        rev = PluginReverseSDE(base, net, Tparam(), ssm_intT=True)
        if tag != "sg":
            out[f"{tag}_y0"] = y0
        if dense:
            out["dn_G"] = base.G
        return base, rev

    for tag, d, dense, pre in (("sg", 2, False, None), ("sp", 6, False, "NormalizeLogRadius"), ("dn", 4, True, None)):
        base, rev = family(tag, d, dense, pre)
        txy = []
        _tap(rev, "sample_txy", txy)
        for sub, t_eps, kept in (("drop", 0.3, 3), ("all", 1e-3, 4)) if tag != "sg" else ():
            base.t_epsilon = t_eps
            x = torch.randn(B, d) * 1.5
            del txy[:]
            with Recorder() as r:
                rev.zero_grad()
                per = rev.ssm(x)
                per.mean().backward()
            assert [k for k, _ in r.draws] == ["randn_like"] * nsf + ["rand"] and per.shape == (kept * B,)
            t_, xt, y = txy[0]
            assert torch.equal(xt, x.repeat(kept, 1))
            key = f"{tag}_{sub}"
            out.update({f"{key}_x": x, f"{key}_eps": torch.stack([v for _, v in r.draws[:nsf]]), f"{key}_u_v": r.draws[nsf][1],
                        f"{key}_t": t_, f"{key}_y": y.detach(), f"{key}_per": per.detach(), f"{key}_t_epsilon": np.float64(t_eps)})
            out.update({f"{key}_grad::" + k: p.grad.detach().clone() for k, p in rev.named_parameters() if p.grad is not None})
            print(key, "rows", per.numel(), "loss", float(per.mean()))
        base.t_epsilon = 1e-3
        x = torch.randn(B, d) * 1.5
        latent, lps = [], []
        _tap(rev, "cond_latent_sample", latent)
        _tap(base, "log_latent_pdf", lps)
        del txy[:]
        st = torch.get_rng_state()
        with Recorder() as r:
            elbo = rev.elbo_random_t_slice(x)
        assert [k for k, _ in r.draws[:nsf + 1]] == ["randn_like"] * nsf + ["rand"] and elbo.shape == (nsf * B,)
        torch.set_rng_state(st)
        mean, sem = ref_nn.evaluate(rev, x)                 # the same draws again
        assert rev.training and float(mean.detach()) == float(elbo.detach().mean())
        key = f"{tag}_ev"
        out.update({f"{key}_x": x, f"{key}_eps": torch.stack([v for _, v in r.draws[:nsf]]), f"{key}_u_v": r.draws[nsf][1],
                    f"{key}_t": txy[0][0], f"{key}_y": txy[0][2].detach(), f"{key}_yT": latent[0], f"{key}_lp": lps[0].view(nsf * B, -1).sum(1),
                    f"{key}_elbo": elbo.detach(), f"{key}_mean": mean.detach(), f"{key}_sem": sem.detach()})
        print(key, "mean", float(mean), "sem", float(sem))
    save("g24_ssm_intT", **out)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    only = sys.argv[1:]
    for name, fn in list(globals().items()):
        if name.startswith("g") and name[1:3].isdigit() and callable(fn):
            if only and not any(name.startswith(o) for o in only):
                continue
            fn()
