"""tests/ssm_intT_ref.py against the reference's own ssm() with ssm_intT=True (fixture g24), and the mask rule at its edges.
No GPU.  Bounds: those tests/test_oracle_golden.py applies to the same oracle functions — the RK4 forward trajectory (g08:
5e-6), the per-row SSM loss (g14: 1e-5) and its parameter gradients (g14: 5e-5); t is formed by the same fp32 linspace and
must be equal."""
import pytest
import torch

import ssm_intT_ref as R
from conftest import load_golden, rel_l2
from oracle import nets_ref as N
from oracle import sde_ref as S
from oracle.det_params import load_det_

B, NSF = 3, 4
CASES = [("sp", S.MSGM_SPARSE, 6, "NormalizeLogRadius"), ("dn", S.MSGM_DENSE, 4, None)]
SUBS = [("drop", 0.3, 1), ("all", 1e-3, 0)]


@pytest.fixture(scope="module")
def g():
    return load_golden("g24_ssm_intT")


def mlp_params(d, pre):
    from sdeflow_light_amd.NN import MLP
    return {k: v.clone() for k, v in load_det_(MLP(d, premodule=pre)).items()}


def spec(g, kind, d, t_eps):
    return S.SdeSpec(kind=kind, n=d, num_steps_forward=NSF, t_epsilon=t_eps, G=g.get("dn_G") if kind == S.MSGM_DENSE else None)


@pytest.mark.parametrize("sub,t_eps,k0", SUBS)
@pytest.mark.parametrize("tag,kind,d,pre", CASES)
def test_g24_ssm(g, tag, kind, d, pre, sub, t_eps, k0):
    key = f"{tag}_{sub}"
    assert float(g[key + "_t_epsilon"]) == t_eps
    sp = spec(g, kind, d, t_eps)
    score = lambda prm, yy, tt: N.mlp_forward(prm, yy, tt, pre)
    t, y, loss, per, grads = R.ssm(sp, score, mlp_params(d, pre), g[key + "_x"], g[key + "_eps"], g[key + "_u_v"])
    rows = (NSF - k0) * B
    assert t.shape == (rows, 1) and y.shape == (rows, d) and per.shape == (rows,)
    assert torch.equal(t, g[key + "_t"])
    assert torch.equal(t.reshape(NSF - k0, B)[:, 0], torch.linspace(0.25, 1.0, NSF)[k0:])       # time-major
    e_y, e_per = rel_l2(y, g[key + "_y"]), rel_l2(per, g[key + "_per"])
    print(f"g24 {key}: y rel-L2 {e_y:.2e}, per-row loss {e_per:.2e}")
    assert e_y <= 5e-6 and e_per <= 1e-5
    for k, gr in grads.items():
        e = rel_l2(gr, g[f"{key}_grad::a.{k}"])
        assert e <= 5e-5, (k, e)


@pytest.mark.parametrize("tag,kind,d", [("sg", S.SGM, 2), ("sp", S.MSGM_SPARSE, 6), ("dn", S.MSGM_DENSE, 4)])
def test_g24_evaluate_rows(g, tag, kind, d):
    """The evaluate cases: the rows of sample_txy, and evaluate's two numbers from the stored ELBO rows (its standard error
    divides by the DATA rows B, not by the nsf' B training rows: NN.py:124-129)."""
    key = f"{tag}_ev"
    t, xt, y = R.sample_txy(spec(g, kind, d, 1e-3), g[key + "_x"], g[key + "_eps"])
    assert torch.equal(t, g[key + "_t"]) and torch.equal(xt, g[key + "_x"].repeat(NSF, 1))
    assert rel_l2(y, g[key + "_y"]) <= 5e-6
    elbo = g[key + "_elbo"]
    assert elbo.shape == (NSF * B,) and g[key + "_yT"].shape == (NSF * B, d) and g[key + "_lp"].shape == (NSF * B,)
    assert float(elbo.mean()) == float(g[key + "_mean"])
    assert abs(float(elbo.std() / B ** 0.5) - float(g[key + "_sem"])) <= 1e-6 * abs(float(g[key + "_sem"]))


def test_mask_rule_edges():
    """<=: a t_epsilon exactly on a grid time drops that time; nothing kept is an error."""
    for t_eps, k0 in ((0.25, 1), (0.5, 2), (0.24999, 0), (0.75, 3), (1e-3, 0)):
        tk, k = R.kept_grid(S.SdeSpec(num_steps_forward=NSF, t_epsilon=t_eps))
        assert k == k0 and torch.equal(tk, torch.linspace(0.25, 1.0, NSF)[k0:]), (t_eps, k)
    for t_eps in (1.0, 1.5):
        with pytest.raises(ValueError):
            R.kept_grid(S.SdeSpec(num_steps_forward=NSF, t_epsilon=t_eps))
    # a horizon other than 1, and a grid whose first entry is not exact in fp32
    tk, k = R.kept_grid(S.SdeSpec(num_steps_forward=3, T=2.0, t_epsilon=float(torch.linspace(2.0 / 3, 2.0, 3)[0])))
    assert k == 1 and tk.numel() == 2


def test_host_mirror_agrees_on_the_grid():
    """SDEs.intT_kept_grid (what PluginReverseSDE.intT_grid caches on the device) is host arithmetic: the same kept times and
    prefix length, the same error; sample_t_linspace agrees.  The flag itself needs a cuda device at construction."""
    from sdeflow_light_amd.NN import MLP
    from sdeflow_light_amd.SDEs import MsgmError, PluginReverseSDE, SGMsde, intT_kept_grid
    T = torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)
    for t_eps, k0 in ((0.25, 1), (0.5, 2), (0.3, 1), (1e-3, 0), (0.75, 3)):
        tk, k = intT_kept_grid(NSF, 1.0, t_eps)
        want, kw = R.kept_grid(S.SdeSpec(num_steps_forward=NSF, t_epsilon=t_eps))
        assert k == kw == k0 and torch.equal(tk, want)
        gen = PluginReverseSDE(SGMsde(T=T, t_epsilon=t_eps, num_steps_forward=NSF), MLP(2), T)
        assert gen.ssm_intT is False and torch.equal(gen.sample_t_linspace(torch.zeros(1))[0], want)
    for t_eps in (1.0, 1.5):
        with pytest.raises(MsgmError):
            intT_kept_grid(NSF, 1.0, t_eps)
    with pytest.raises(MsgmError, match="cuda"):
        PluginReverseSDE(SGMsde(T=T, num_steps_forward=NSF), MLP(2), T, ssm_intT=True)
