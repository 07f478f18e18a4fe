"""CPU restatement of the time-integrated SSM loss, PluginReverseSDE(ssm_intT=True) (SDEs.py:648-706), composed from the
oracle's own functions: the grid and its ``<=`` mask, one RK4-Stratonovich path of the forward process per row with all
states kept, the time-major flatten, and ``ssm_mean_and_grads`` on the flattened rows.  Pinned to the reference by
tests/test_ssm_intT_ref.py (fixture g24); the GPU tests compare the HIP path against it where no fixture exists."""
import torch

from oracle import sde_ref as S
from oracle import ssm_ref as LR


def grid_and_mask(spec: S.SdeSpec):
    """(t_grid (nsf,) fp32, mask of the dropped entries): linspace(T/nsf, T, nsf), dropped where t <= t_epsilon."""
    nsf, T = spec.num_steps_forward, float(spec.T)
    t = torch.linspace(T / nsf, T, nsf)
    return t, t <= spec.t_epsilon


def kept_grid(spec: S.SdeSpec):
    """(kept times (nsf',), k0).  The dropped entries are a prefix (the grid increases); none left is an error."""
    t, mask = grid_and_mask(spec)
    k0 = int(mask.sum())
    assert not bool(mask[k0:].any())
    if k0 == t.numel():
        raise ValueError(f"every grid time is <= t_epsilon = {spec.t_epsilon}: no training row is left")
    return t[k0:], k0


def sample_txy(spec: S.SdeSpec, x, eps):
    """(t (nsf'B, 1), x tiled (nsf'B, n), y (nsf'B, n)), row j B + b = (t_grid[k0 + j], x[b], y[k0 + j, b]); eps (nsf, B, n)."""
    tk, k0 = kept_grid(spec)
    B = x.shape[0]
    traj = S.rk4_stratonovich(S.ForwardProcess(spec), x, spec.num_steps_forward, eps, keep_all=True, include_t0=False)
    y = traj[k0:]
    return tk.repeat_interleave(B).reshape(-1, 1), x.repeat(tk.numel(), 1), y.reshape(tk.numel() * B, -1)


def ssm(spec: S.SdeSpec, score, params, x, eps, u_v, form="jvp"):
    """(t, y, mean loss, per-row losses (nsf'B,), parameter gradients of the mean); u_v (nsf'B, n) probe uniforms."""
    t, _, y = sample_txy(spec, x, eps)
    loss, per, grads = LR.ssm_mean_and_grads(spec, score, params, t, y, S.rademacher_from_uniform(u_v), form=form)
    return t, y, loss, per, grads
