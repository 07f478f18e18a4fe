"""CPU side of the 1-D U-Net deep-level parity (tests/unet1d_deep.py, tests/test_unet1d_deep_gpu.py): the conditions the
gain-3 fill must meet at the seven cases for the GPU tests to see every level, the proof that the yardstick
(conftest.parity_vs_fp64(floor_frac=1e-4), default slack) rejects one wiring mistake at the deepest level, the record of why
the sinusoidal fill could not, and the oracle against the reference's own results (tests/golden/g22_unet1d_deep.npz)."""
import pytest
import torch

import unet1d_deep as U
from conftest import check_digest, load_golden, parity_vs_fp64, rel_l2
from oracle import sde_ref as S, ssm_ref as LR
from oracle.det_params import det_state_dict, init_like_state_dict, init_like_tensor
from oracle.shapes import unet1d_shapes


def test_gain_scales_the_weights_only_and_defaults_to_the_old_fill():
    sh = unet1d_shapes(37, U.NLR)
    one, dflt, three = init_like_state_dict(sh, gain=1.0), init_like_state_dict(sh), init_like_state_dict(sh, gain=3.0)
    assert set(one) == set(sh)
    for k, s in sh.items():
        assert torch.equal(one[k], dflt[k]) and torch.equal(dflt[k], init_like_tensor(k, s, sh))
        if len(s) >= 2:
            # the gain is applied in float64 before the one rounding to float32: rd(3 v) against 3 rd(v), each rounding at most
            # 2^-24 relative, so 6 x 2^-24 |v|
            assert float((three[k].double() - 3.0 * one[k].double()).abs().max()) <= 6 * 2.0 ** -24 * float(one[k].abs().max())
            assert float(three[k].norm()) > 2.9 * float(one[k].norm())
        else:
            assert torch.equal(three[k], one[k])


@pytest.mark.parametrize("case", list(U.CASES))
def test_fill_conditions(case):
    """Conditions on the INPUTS of the GPU tests (float64 oracle only): no parameter tensor's gradient norm is under 1e-4 of
    the largest (measured least ratios A 1.7e-3, B 4.6e-3, C 5.5e-4, D 6.3e-4, E 1.6e-3, F 4.9e-3, G 6.2e-3), and the
    deepest transposed convolution matters (zeroing up_convs.0.weight moves the 5-row forward output by 0.23 .. 0.94)."""
    _, g64 = U.oracle(case, torch.float64)
    assert set(g64) == set(U.shapes(case))
    norms = {k: float(v.norm()) for k, v in g64.items()}
    lo = min(norms, key=norms.get)
    ratio = norms[lo] / max(norms.values())
    x, t = U.forward_draws(case)
    p = {k: w.double() for k, w in U.params(case).items()}
    cut = dict(p, **{"up_convs.0.weight": torch.zeros_like(p["up_convs.0.weight"])})
    with torch.no_grad():
        y, y0 = U.score(case)(p, x.double(), t.double()), U.score(case)(cut, x.double(), t.double())
    moved = rel_l2(y0, y)
    print(f"case {case}: least gradient-norm ratio {ratio:.2e} ({lo}); output moved by {moved:.2e} without up_convs.0.weight")
    assert bool(torch.isfinite(y).all()) and ratio >= 1e-4 and moved >= 1e-2, (lo, ratio, moved)


@pytest.mark.parametrize("case", list(U.CASES))
def test_restated_forward_without_a_mistake_is_the_oracle(case):
    x, t = U.forward_draws(case)
    p = U.params(case)
    with torch.no_grad():
        assert torch.equal(U.score(case, None)(p, x, t), U.forward_with_mistake(p, x, t, U.CASES[case]["pre"], U.levels(case), None))


# down_tap at D: downs.2 maps 2 positions to 1 there, and its last tap reads the right zero pad only (see the next test)
SENSITIVITY = [(c, m) for c in ("A", "B", "C", "D", "G") for m in U.MISTAKES if (c, m) != ("D", "down_tap")]


@pytest.mark.parametrize("case,mistake", SENSITIVITY)
def test_yardstick_rejects_a_wiring_mistake_at_the_deepest_level(case, mistake):
    """The HIP side of the yardstick replaced by the float32 oracle with one wiring mistake: rejected at the default slack.
    The float32 oracle without a mistake passes (it is the reference side itself)."""
    parity_vs_fp64(lambda: U.oracle(case, torch.float32), U.oracle_fn(case), f"case {case}, float32 oracle", floor_frac=U.FLOOR_FRAC)
    with pytest.raises(AssertionError):
        parity_vs_fp64(lambda: U.ssm_oracle(case, torch.float32, mistake), U.oracle_fn(case), f"case {case} with {mistake}",
                       floor_frac=U.FLOOR_FRAC)


def test_last_tap_of_the_deepest_downsampling_reads_padding_only_at_two_positions():
    per, g = U.ssm_oracle("D", torch.float64, "down_tap")
    per0, g0 = U.oracle("D", torch.float64)
    w = g0["downs.2.weight"]
    assert torch.equal(per, per0) and float(w[..., 3].abs().max()) == 0.0 and float(w[..., :3].abs().max()) > 0
    assert all(torch.equal(g[k], g0[k]) for k in g0)


def test_sinusoidal_fill_hides_the_same_mistake():
    """Why the new fill: under det_state_dict at L = 64 (B = 3; downs.2 maps 16 positions to 8, its last tap reads data) the
    net without the last tap of downs.2 moves the float64 per-sample loss, the flat gradient and the worst tensor (relative to
    max(own norm, 1e-3 x largest), check_digest's scale) by less than the det-fill tests allow: 1e-7 on the loss and 5e-7 per
    tensor (test_unet1d_ssm_golden), 2e-6 on the flat gradient (test_ssm_unet1d_msgm_sparse_vs_oracle).  Measured: 0.0,
    2.8e-13, 2.1e-10.  Under the gain-3 fill the same mistake moves downs.2.weight by 1.0 of its norm (case B)."""
    L, B = 64, 3
    torch.manual_seed(L)
    x, u, eps, uv = torch.randn(B, L), torch.rand(B), torch.randn(B, L), torch.rand(B, L)
    sp = S.SdeSpec()
    t = S.clamp_time(sp, u.reshape(B, 1))
    y, v = S.vp_perturb(sp, t, x, eps), S.rademacher_from_uniform(uv)
    p = {k: w.double() for k, w in det_state_dict(unet1d_shapes(L, None)).items()}

    def run(mistake):
        sc = lambda prm, yy, tt: U.forward_with_mistake(prm, yy, tt, None, 3, mistake)      # noqa: E731
        _, per, g = LR.ssm_mean_and_grads(sp, sc, p, t.double(), y.double(), v.double())
        return per, g
    (per0, g0), (per, g) = run(None), run("down_tap")
    keys = list(g0)
    cat = lambda gr: torch.cat([gr[k].reshape(-1) for k in keys])                            # noqa: E731
    top = max(float(g0[k].norm()) for k in keys)
    e_per, e_flat = rel_l2(per, per0), rel_l2(cat(g), cat(g0))
    e_t = max(float((g[k] - g0[k]).norm()) / max(float(g0[k].norm()), 1e-3 * top) for k in keys)
    under = sum(float(g0[k].norm()) < 1e-3 * top for k in keys)
    print(f"det fill, L = 64, downs.2 without its last tap: loss moved {e_per:.2e}, flat gradient {e_flat:.2e}, worst tensor "
          f"{e_t:.2e}; {under} of {len(keys)} tensors under 1e-3 of the largest gradient norm")
    assert float(g0["downs.2.weight"][..., 3].abs().max()) > 0
    assert e_per <= 1e-7 and e_flat <= 2e-6 and e_t <= 5e-7


@pytest.mark.parametrize("case", ["B", "C", "D", "G"])
def test_g22_oracle_reproduces_the_reference(case):
    """The reference's UNet1D under the same fill (tools/make_golden.py:g22_unet1d_deep, float32 on the CPU).  The oracle is
    the same ATen calls in the same order: the forward is equal to the bit where this was recorded, and is held to 1e-6 (a
    few float32 roundings, should another CPU's kernels order a sum differently); per-sample loss and gradient digest
    (reference: double backward, oracle: jvp) to the tolerances of test_g10_ssm_unet1d."""
    g = load_golden("g22_unet1d_deep")
    x, u, eps, uv = U.draws(case)
    xf, tf = U.forward_draws(case)
    for mine, key in ((x, "x"), (u.reshape(-1, 1), "u_t"), (eps, "eps"), (uv, "u_v"), (xf, "fwd_x"), (tf, "fwd_t")):
        assert torch.equal(mine, g[f"{case}_{key}"]), key                     # the shared cases ARE the recorded inputs
    with torch.no_grad():
        yf = U.score(case)(U.params(case), xf, tf)
    e = rel_l2(yf, g[f"{case}_fwd"])
    print(f"case {case}: forward vs the reference rel-L2 {e:.2e}")
    assert yf.shape == g[f"{case}_fwd"].shape and e <= 1e-6
    per, grads = U.oracle(case, torch.float32)
    assert rel_l2(per, g[f"{case}_per"]) <= 2e-5, rel_l2(per, g[f"{case}_per"])
    check_digest(g, case, grads, "a.", 1e-4)
