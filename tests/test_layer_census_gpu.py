"""Per-layer float64 parity of every kernel call the benchmarked steps make.

1. Census: one eager step of each benchmarked configuration, built as bench.py:build_unet builds it — C4 (2-D U-Net
   training, B = 256 and its 32-row shard), C3 (1-D U-Net training, B = 4096), C5 (the 2-D sampler forward at 4096 and
   1024 rows) — with the layer entry points wrapped, so that every call leaves a SIGNATURE (op configuration, row count,
   image size, the options passed, whether a DeferredReduces pass was active).  The census asserts that every
   convolution of each net appears in it.
2. Replay: every distinct signature runs again on a fresh op with random He-scaled weights and unit-variance inputs and
   cotangents, at the recorded row count and at a small ragged one (13 samples), outputs pre-filled with NaN, and every
   output is compared with the float64 references of tests/layer_ref.py: rel-L2 over the tensor, the worst per-row
   rel-L2, and the worst element relative to the reference RMS.  Every output is first asserted finite over its whole
   extent (no NaN pre-fill left anywhere in the launch).  The comparison of per-row outputs — forward outputs and the
   attention backward's dqkv — uses sampled rows (the first two, both sides of the primal / tangent boundary, the middle,
   the last 8: the last partial tiles and chunks); the conv and GroupNorm input cotangents and every reduction over rows
   (weight, bias, per-sample bias, embedding, gamma / beta gradients) are compared over all rows.
   The replay always hands the op caller-owned output / cotangent buffers (NaN, or the base of an accumulation), so a
   signature does not record whether the net passed its own buffer; forward calls do not record the DeferredReduces
   state either (only backward work is deferred).
3. The signatures replayed in reverse order give the same bits as in forward order (no kernel reads state it did not
   write).
4. The comparator rejects a one-element 1e-3 x RMS change in the last row of a real C4-size output and a swap of two
   channels of one pixel — changes a tensor-wide rel-L2 or a norm + head digest would not see."""
import gc
import inspect
import math

import pytest
import torch

import layer_ref as R
from sdeflow_light_amd import ops
from sdeflow_light_amd.convnet import ConvOp, ConvOpSet, Stride2PairOp

pytestmark = pytest.mark.gpu
DEV = "cuda"
RAGGED = 13                   # samples of the second replay: tile / workgroup / chunk counts that do not divide
CONFIGS = ("c4_b256", "c4_b32", "c3_b4096", "c5_4096", "c5_1024", "v24_b3", "v24_fwd5", "u1d37_b3", "u1d37_fwd5")

# ------------------------------------------------------------------------------------------------ bounds
# Output families and their bounds on (rel-L2 over the tensor, worst per-row rel-L2, worst element / reference RMS).
# Caps: the unit tests' bounds against fp32 PyTorch — 1e-5 for conv forward / dgrad / wgrad / bias gradients (and the
# embedding bank and activations built on the same arithmetic), 2e-5 for GroupNorm and attention.  Within them every bound
# is <= 3x the worst value measured over the five configurations, full and ragged row counts, on the first MI355X run
# ("measured": rel-L2 / row / element).  The largest weight-gradient error is the 1-D U-Net's paired-stride transposed
# conv at 8192 rows x 256 positions (rel-L2 1.9e-6: fp32 sums over 2M products); the attention's worst elements sit on
# the peaked softmax rows.
BOUNDS = {
    "conv_fwd": (1.4e-6, 1.5e-6, 1.4e-5),       # measured 4.7e-7 / 5.0e-7 / 4.9e-6
    "conv_dgrad": (1.2e-6, 1.2e-6, 2.1e-5),     # measured 4.1e-7 / 4.2e-7 / 7.2e-6
    "conv_wgrad": (5.7e-6, 6.0e-6, 2.7e-5),     # measured 1.9e-6 / 2.2e-6 / 9.2e-6
    "conv_bias": (2.6e-6, 2.6e-6, 6.6e-6),      # measured 8.9e-7 / 8.9e-7 / 2.2e-6   (bias, dsamp_bias, demb)
    "conv_stats": (2.2e-7, 2.6e-7, 4.5e-6),     # measured 7.5e-8 / 8.7e-8 / 1.5e-6   (channel sums for the folded GroupNorm)
    "gn_fwd": (2.5e-7, 2.6e-7, 8.1e-6),         # measured 8.4e-8 / 8.9e-8 / 2.7e-6
    "gn_bwd": (2.8e-7, 3.3e-7, 1.3e-5),         # measured 9.6e-8 / 1.1e-7 / 4.6e-6
    "gn_param": (9.3e-7, 9.3e-7, 3.9e-6),       # measured 3.1e-7 / 3.1e-7 / 1.3e-6   (gamma / beta over all samples)
    "gn_affine": (1.7e-7, 2.1e-7, 9.9e-7),      # measured 5.9e-8 / 7.1e-8 / 3.3e-7
    "attn_fwd": (2.9e-6, 3.3e-6, 2.5e-4),       # measured 9.8e-7 / 1.1e-6 / 8.4e-5
    "attn_bwd": (2.3e-6, 2.8e-6, 2.3e-4),       # measured 7.8e-7 / 9.5e-7 / 7.7e-5
    "emb": (1.1e-6, 1.3e-6, 7.8e-6),            # measured 3.9e-7 / 4.5e-7 / 2.6e-6
    "act": (2.4e-7, 2.4e-7, 1.2e-5),            # measured 8.3e-8 / 8.3e-8 / 4.0e-6
}


# ------------------------------------------------------------------------------------------------ comparator
class Cmp:
    """Error metrics of one output, accumulated over row chunks: kernel rows y (fp32) against reference rows r (fp64).
    A row is the first index (a sample; an output channel of a weight gradient).  The per-row rel-L2 divides by the row's
    reference norm floored at 0.1 x the RMS row norm: a row that is itself a near-cancelling sum (one entry of a weight
    gradient over 4096 samples, 100x under the typical entry) measures conditioning, not the kernel; the worst-element
    metric still covers it."""

    def __init__(self):
        self.e2 = self.r2 = 0.0
        self.amax = 0.0
        self.n = 0
        self.rows_e, self.rows_r = [], []
        self.nonfinite = False

    def add(self, y, r):
        y, r = y.double().reshape(r.shape[0], -1), r.reshape(r.shape[0], -1)
        if not bool(torch.isfinite(y).all()):
            self.nonfinite = True
            return
        d = y - r
        de, rn = (d * d).sum(1), (r * r).sum(1)
        self.e2 += float(de.sum())
        self.r2 += float(rn.sum())
        self.rows_e.append(de.cpu())
        self.rows_r.append(rn.cpu())
        self.amax = max(self.amax, float(d.abs().max()))
        self.n += r.numel()

    def metrics(self):
        if self.nonfinite:
            return (math.inf, math.inf, math.inf)
        rms = math.sqrt(self.r2 / max(self.n, 1))
        de, rn = torch.cat(self.rows_e), torch.cat(self.rows_r)
        floor = 0.1 * math.sqrt(self.r2 / max(rn.numel(), 1))
        row = float((de.sqrt() / rn.sqrt().clamp_min(max(floor, 1e-300))).max())
        return (math.sqrt(self.e2 / max(self.r2, 1e-300)), row, self.amax / max(rms, 1e-300))


def cmp(y, r):
    c = Cmp()
    c.add(y, r)
    return c


def within_bounds(metrics, family):
    return all(m <= b for m, b in zip(metrics, BOUNDS[family]))


def digest(t):
    """Order-sensitive digest of the bits of a float32 tensor (the reverse-order replay compares these)."""
    b = t.detach().contiguous().view(-1).view(torch.int32)
    n, step = b.numel(), 1 << 24
    w = (torch.arange(1, min(n, step) + 1, device=b.device, dtype=torch.int64) * 0x9E3779B1) | 1
    s1 = s2 = 0
    for c0 in range(0, n, step):
        c = b[c0:c0 + step].to(torch.int64)
        s1 += int(c.sum())
        s2 = (s2 * 1000003 + int((c * w[: c.numel()]).sum())) & ((1 << 64) - 1)
    return (n, s1, s2)


def _finished(outs):
    """After a replay: every output tensor is finite over its WHOLE extent (the comparisons may look at sampled rows only;
    a NaN pre-fill left by a skipped tile / workgroup / chunk anywhere in the launch fails here), then the bit digests."""
    torch.cuda.synchronize()
    for k, (_, v) in outs.items():
        assert bool(torch.isfinite(v).all()), f"output {k}: non-finite values (an unwritten NaN pre-fill?)"
    return {k: digest(v) for k, (_, v) in outs.items()}


# ------------------------------------------------------------------------------------------------ recorder
def _opcfg(op):
    if isinstance(op, Stride2PairOp):
        return ("Stride2PairOp", op.kind, tuple(op.weight.shape), op.bias is not None, 1, 4, 2, 1, (op.C,), 0, False, False,
                op.CoutP)
    return ("ConvOp", op.kind, tuple(op.weight.shape), op.bias is not None, op.KH, op.KW, op.stride, op.pad, tuple(op.srcC),
            op.embC, bool(op.ups), bool(op.train_wino), op.CoutP)


def _deferred():
    return ops.DeferredReduces.active is not None


class Recorder:
    def __init__(self):
        self.sigs = {}                 # signature -> None (insertion ordered)
        self.fwd_ops, self.bwd_ops = set(), set()

    def add(self, sig):
        self.sigs.setdefault(sig, None)

    def patches(self, mp):
        rec = self

        def wrap_method(cls, name, make_sig, fwd=None):
            real = getattr(cls, name)
            sg = inspect.signature(real)

            def w(self_, *a, **kw):
                ba = sg.bind(self_, *a, **kw)
                ba.apply_defaults()
                rec.add(make_sig(self_, ba.arguments))
                if fwd is True:
                    rec.fwd_ops.add(id(self_))
                elif fwd is False:
                    rec.bwd_ops.add(id(self_))
                return real(self_, *a, **kw)
            mp.setattr(cls, name, w)

        def wrap_fn(name, make_sig):
            real = getattr(ops, name)
            sg = inspect.signature(real)

            def w(*a, **kw):
                ba = sg.bind(*a, **kw)
                ba.apply_defaults()
                rec.add(make_sig(ba.arguments))
                return real(*a, **kw)
            mp.setattr(ops, name, w)

        has = lambda v: v is not None                     # noqa: E731
        conv_f = lambda o, A: ("conv_fwd", _opcfg(o), A["N"], A["Hi"], A["Wi"], A["n_bias"],  # noqa: E731
                               A.get("emb_rows") if A.get("emb_rows") is not None else A["n_bias"],
                               has(A.get("emb")), has(A.get("samp_bias")), bool(A.get("accumulate")),
                               has(A.get("residual")), has(A.get("in_affine")), int(A.get("in_act") or 0),
                               bool(A.get("wino")), bool(A.get("stats")))

        def conv_b(o, A):
            zeroed = bool(A.get("bias_grad_zeroed")) or bool(o._bias_zeroed)
            need = tuple(A["need"]) if A.get("need") is not None else None
            dacc = tuple(bool(d) for d in A["dacc"]) if A.get("dacc") is not None else None
            return ("conv_bwd", _opcfg(o), A["N"], A["Hi"], A["Wi"], A["n_bias"],
                    A.get("emb_rows") if A.get("emb_rows") is not None else A["n_bias"], has(A.get("emb")), has(A.get("demb")),
                    need, dacc, has(A.get("dsamp_bias")), zeroed, bool(A.get("bias_grad_elsewhere")), _deferred())

        def conv_bu(o, A):
            zeroed = bool(A.get("bias_grad_zeroed")) or bool(o._bias_zeroed)
            return ("conv_bwd_ups", _opcfg(o), A["N"], A["Hi"], A["Wi"], A["n_bias"], zeroed, _deferred())

        for cls in (ConvOp, Stride2PairOp):
            wrap_method(cls, "forward", conv_f, fwd=True)
            wrap_method(cls, "backward", conv_b, fwd=False)
        wrap_method(ConvOp, "backward_ups", conv_bu, fwd=False)

        bank = lambda b, A: ((b.K, tuple(b.cos), tuple(cb is not None for _, _, cb in b.items)), A["rows"], A["n_bias"])  # noqa: E731
        wrap_method(ops.EmbBank, "forward", lambda b, A: ("emb_fwd",) + bank(b, A))
        wrap_method(ops.EmbBank, "backward", lambda b, A: ("emb_bwd",) + bank(b, A) + (_deferred(),))

        wrap_fn("groupnorm_dual_forward", lambda A: ("gn_fwd", A["Bp"], A["P"], A["C"], A["G"], bool(A["dual"]), bool(A["silu"]),
                                                     has(A["stats"]), has(A["dropout"])))
        wrap_fn("groupnorm_dual_backward", lambda A: ("gn_bwd", A["Bp"], A["P"], A["C"], A["G"], bool(A["silu"]),
                                                      has(A["residual"]), has(A["residual2"]), has(A["dropout"]), _deferred()))
        wrap_fn("groupnorm_dual_forward2", lambda A: ("gn_fwd2", A["Bp"], A["P"], A["C0"], A["C1"], A["G"], bool(A["dual"]),
                                                      bool(A["silu"]), has(A["stats"])))
        wrap_fn("groupnorm_dual_backward2", lambda A: ("gn_bwd2", A["Bp"], A["P"], A["C0"], A["C1"], A["G"], bool(A["silu"]),
                                                       _deferred()))
        wrap_fn("groupnorm_affine", lambda A: ("gn_affine", A["Bp"], A["P"], A["C0"], A["C1"] if has(A["x1"]) else 0, A["G"]))
        wrap_fn("groupnorm_affine_cs", lambda A: ("gn_affine_cs", A["Bp"], A["P"], A["S0"], A["C0"],
                                                  A["S1"] if has(A["cs1"]) else 0, A["C1"] if has(A["cs1"]) else 0, A["G"]))
        wrap_fn("attention_dual_forward", lambda A: ("attn_dual_fwd", A["Bp"], A["T"], A["C"], float(A["scale"])))
        wrap_fn("attention_dual_backward", lambda A: ("attn_dual_bwd", A["Bp"], A["T"], A["C"], float(A["scale"])))
        wrap_fn("attention_forward", lambda A: ("attn_fwd", A["N"], A["T"], A["C"], float(A["scale"])))
        wrap_fn("act_dual_forward", lambda A: ("act_fwd", int(A["act"]), A["z"].numel(), bool(A["dual"])))
        wrap_fn("act_dual_backward", lambda A: ("act_bwd", int(A["act"]), A["z"].numel()))

        # the composed attention (no fused kernel for the shape): every operand offset is kept — it decides the alignment
        def bmm_sig(A):
            p2, th = A["pair2"], A["third"]
            assert th is None or th[2] is A["Cm"]                      # both outputs in one tensor, as the replay lays them out
            return ("bmm", A["M"], A["N"], A["K"], A["batch"], tuple(A["sA"]), tuple(A["sB"]), tuple(A["sC"]), A["a_off"], A["b_off"],
                    A["c_off"], float(A["alpha"]), bool(A["accumulate"]), (p2[1], p2[3]) if p2 is not None else None,
                    (th[1], th[3]) if th is not None else None)
        wrap_fn("bmm", bmm_sig)
        wrap_fn("softmax_dual_forward", lambda A: ("softmax_fwd", A["S"].numel() // A["T"], A["T"], has(A["Wd"])))
        wrap_fn("softmax_dual_backward", lambda A: ("softmax_bwd", A["Pm"].numel() // A["T"], A["T"]))


def _unet_ops(net):
    """Every ConvOp / Stride2PairOp of a net, each with the ops that may take its place on a path (the decoder twins)."""
    if hasattr(net, "_ops") and not hasattr(net, "core"):                     # UNet1D
        return [(o, ()) for o in net._build().values()]
    x = net._build()
    alts = {}
    for blk in x["outb"]:
        kind, r = blk[0]
        if kind == "res" and r.split is not None:
            alts[id(r.conv1)] = (r.conv1_2,)
            alts[id(r.skip)] = (r.skip_2, r.skip_2t)
    return [(o, alts.get(id(o), ())) for o in x["all"]]


def _build_v24():
    """The 24x24 one-channel net of tests/test_unet2d_sizes_gpu.py (bench.build_unet builds the benchmarked 64x64x3 one only)."""
    from oracle.det_params import load_det_
    from sdeflow_light_amd.NNUnet import VorticityUNet
    from sdeflow_light_amd.SDEs import SGMsde, PluginReverseSDE
    torch.manual_seed(0)
    net = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, attention_resolutions=(2, 4), in_space=24,
                        flatten_order="F")
    load_det_(net)
    T = torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)
    sde = SGMsde(beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=T, num_steps_forward=16, device=DEV)
    return PluginReverseSDE(sde, net.to(DEV), T, vtype="rademacher", deviceReverseSDE=DEV).to(DEV), 576


def _build_u1d37():
    """Case C of tests/test_unet1d_deep_gpu.py: the 1-D U-Net at L = 37 (levels 37 / 18 / 9 / 4: the unpaired k = 4, s = 2
    convolutions and transposed convolutions, no level on a halo-tile kernel) with NormalizeLogRadius."""
    import unet1d_deep as U
    from oracle.det_params import load_init_like_
    from sdeflow_light_amd.NNUnet1D import UNet1D
    from sdeflow_light_amd.SDEs import SGMsde, PluginReverseSDE
    c = U.CASES["C"]
    torch.manual_seed(0)
    net = UNet1D(input_dim=c["L"], base_channels=c["base"], channel_mults=c["mults"], num_res_blocks=2, premodule=c["pre"],
                 emb_dim=c["emb"])
    load_init_like_(net, gain=U.GAIN)
    T = torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)
    sde = SGMsde(beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=T, num_steps_forward=16, device=DEV)
    return PluginReverseSDE(sde, net.to(DEV), T, vtype="rademacher", deviceReverseSDE=DEV).to(DEV), c["L"]


def _record(config):
    import bench
    from sdeflow_light_amd.train import UNetScoreTrainer
    from sdeflow_light_amd.data import signals_1d, random_images
    rec = Recorder()
    u37 = config.startswith("u1d37")
    v24 = config.startswith("v24") or u37                                  # the nets bench.build_unet does not build
    fwd_only = config.startswith("c5") or config.endswith("_fwd5")
    gen, d = (_build_u1d37() if u37 else _build_v24() if v24 else
              bench.build_unet("c3" if config.startswith("c3") else "c4", torch.device(DEV)))
    net = gen.a
    with pytest.MonkeyPatch.context() as mp:
        rec.patches(mp)
        if fwd_only:
            rows = 5 if v24 else int(config.split("_")[1])
            g = torch.Generator(device=DEV).manual_seed(3)
            x = torch.randn(rows, d, device=DEV, generator=g)
            t = torch.rand(rows, device=DEV, generator=g) * 0.9 + 0.05
            with torch.no_grad():
                y = net(x, t)
            assert torch.isfinite(y).all()
            del x, y
        else:
            B = int(config.split("_b")[1])
            tr = UNetScoreTrainer(gen, B, d, lr=1e-4, world=1, seed=1, use_graph=False)
            tr.set_data(torch.randn(B, d, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1234)) if v24 else
                        signals_1d(B, seed=1234, device=DEV) if config.startswith("c3") else random_images(B, seed=1234, device=DEV))
            tr.step()
            del tr
    torch.cuda.synchronize()
    missing_f, missing_b = [], []
    for o, alts in _unet_ops(net):
        ids = {id(o)} | {id(a) for a in alts if a is not None}
        if not ids & rec.fwd_ops:
            missing_f.append(_opcfg(o))
        if not fwd_only and not ids & rec.bwd_ops:
            missing_b.append(_opcfg(o))
    del gen, net
    gc.collect()
    torch.cuda.empty_cache()
    return list(rec.sigs), missing_f, missing_b


_CENSUS = {}


def census(config):
    if config not in _CENSUS:
        _CENSUS[config] = _record(config)
    return _CENSUS[config]


# ------------------------------------------------------------------------------------------------ replay
class Rand:
    def __init__(self, seed):
        self.g = torch.Generator(device=DEV).manual_seed(seed)

    def n(self, *shape, scale=1.0, shift=0.0):
        return torch.randn(*shape, device=DEV, generator=self.g) * scale + shift


def _nan(n):
    return torch.full((n,), float("nan"), device=DEV)


def _chunks(n, per_row, budget=2.5e7):
    step = max(1, int(budget // max(per_row, 1)))
    return [torch.arange(a, min(n, a + step), device=DEV) for a in range(0, n, step)]


def _sample_rows(N, n_bias):
    if N <= 64:
        return torch.arange(N, device=DEV)
    s = sorted({0, 1, n_bias - 1, n_bias, min(N - 1, n_bias + 1), N // 2} | set(range(N - 8, N)))
    return torch.tensor([r for r in s if 0 <= r < N], device=DEV)


def _split(idx, per_row, budget=2.5e7):
    step = max(1, int(budget // max(per_row, 1)))
    return [idx[a:a + step] for a in range(0, idx.numel(), step)]


def _scale_rows(sig_N, n_bias, er, new_b):
    """(N, n_bias, emb_rows) of the ragged replay: the same ratios, new_b samples."""
    f = lambda v: new_b * v // n_bias if n_bias else v     # noqa: E731
    return f(sig_N), new_b, f(er)


def _make_conv(cfg, rnd, wino_fwd):
    cls, kind, wshape, has_b, KH, KW, stride, pad, srcC, embC, ups, train_wino, _ = cfg
    fan_in = (wshape[0] if kind == "convT" else wshape[1]) * math.prod(wshape[2:])
    W = torch.nn.Parameter(rnd.n(*wshape, scale=math.sqrt(2.0 / fan_in)))
    Cout = wshape[1] if kind == "convT" else wshape[0]
    b = torch.nn.Parameter(rnd.n(Cout, scale=0.5)) if has_b else None
    if cls == "Stride2PairOp":
        op = Stride2PairOp(W, b, kind)
    else:
        ks = (1,) if len(wshape) == 2 else (wshape[2],) if len(wshape) == 3 else (KH, KW)
        op = ConvOp(W, b, kind, ks, stride, pad, list(srcC), emb_channels=embC, ups=ups)
    st = ConvOpSet([op])
    st.pack()
    if train_wino:
        st.pack_wino(train=True)
        assert op.train_wino
    elif wino_fwd:
        st.pack_wino(train=False)
    return op, st, W, b, Cout


def _conv_ref_kw(cfg, rows, n_bias, er):
    _, kind, _, _, _, _, stride, pad, _, _, ups, _, _ = cfg
    return dict(kind="convT" if kind == "convT" else "conv", stride=stride, pad=pad, ups=ups, rows=rows, n_bias=n_bias,
                emb_rows=er)


def replay_conv_fwd(sig, rnd, ragged=False, with_ref=True):
    _, cfg, N, Hi, Wi, n_bias, er, f_emb, f_sb, f_acc, f_res, f_aff, in_act, wino, stats = sig
    if ragged:
        N, n_bias, er = _scale_rows(N, n_bias, er, RAGGED)
    op, _, W, b, Cout = _make_conv(cfg, rnd, wino)
    srcC, embC = cfg[8], cfg[9]
    Ho, Wo = op.out_hw(Hi, Wi)
    srcs = [rnd.n(N * Hi * Wi * C) for C in srcC]
    ctot = sum(srcC)
    kw = dict(out=rnd.n(N * Ho * Wo * Cout) if f_acc else _nan(N * Ho * Wo * Cout), accumulate=f_acc)
    base = kw["out"].clone() if f_acc else None
    emb = rnd.n(er * embC) if embC else None
    sb = rnd.n(er * Cout) if f_sb else None
    res = rnd.n(N * Ho * Wo * Cout) if f_res else None
    aff = (rnd.n(N * ctot, scale=0.5, shift=1.0), rnd.n(N * ctot, scale=0.5)) if f_aff else None
    if isinstance(op, ConvOp):
        kw.update(emb=emb, samp_bias=sb, emb_rows=er, residual=res, in_affine=aff, in_act=in_act, wino=wino, stats=stats)
    out, _, _ = op.forward(srcs, N, Hi, Wi, n_bias, **kw)
    outs = {"out": ("conv_fwd", out)}
    cs = getattr(out, "_msgm_cs", None)
    if cs is not None:              # the statistics buffer is the op's own (torch.empty): checked whole for finiteness
        outs["chanstats"] = ("conv_stats", cs[0][: N * cs[1] * 2 * Cout])
    dig = _finished(outs)
    if not with_ref:
        return None, dig
    rows = _sample_rows(N, n_bias)
    d = lambda t, C, H, Wd: t.view(N, H, Wd, C)[rows].double()    # noqa: E731
    ref = R.conv_forward([d(s, C, Hi, Wi) for s, C in zip(srcs, srcC)], W.detach().double(),
                         b.detach().double() if b is not None else None,
                         emb=emb.view(er, embC).double() if emb is not None else None,
                         samp_bias=sb.view(er, Cout).double() if sb is not None else None,
                         in_affine=(aff[0].view(N, ctot)[rows].double(), aff[1].view(N, ctot)[rows].double()) if aff else None,
                         in_act=in_act, residual=d(res, Cout, Ho, Wo) if res is not None else None,
                         base=d(base, Cout, Ho, Wo) if base is not None else None, **_conv_ref_kw(cfg, rows, n_bias, er))
    res_m = {"out": ("conv_fwd", cmp(out.view(N, Ho, Wo, Cout)[rows], ref).metrics())}
    if cs is not None:
        # channel statistics by-product [N][S][{sum, sum of squares}][Cout], summed over the slots, against the output's
        csv = cs[0].view(N, cs[1], 2, Cout)[rows].double().sum(1)
        r2 = torch.stack([ref.sum((1, 2)), (ref * ref).sum((1, 2))], 1)
        res_m["chanstats"] = ("conv_stats", cmp(csv, r2).metrics())
    return res_m, dig


def replay_conv_bwd(sig, rnd, ragged=False, with_ref=True, ups_form=False):
    if ups_form:
        _, cfg, N, Hi, Wi, n_bias, zeroed, deferred = sig
        er, f_emb, f_demb, need, dacc, f_dsb, elsewhere = n_bias, False, False, None, None, False, False
    else:
        _, cfg, N, Hi, Wi, n_bias, er, f_emb, f_demb, need, dacc, f_dsb, zeroed, elsewhere, deferred = sig
    if ragged:
        N, n_bias, er = _scale_rows(N, n_bias, er, RAGGED)
    op, st, W, b, Cout = _make_conv(cfg, rnd, False)
    cls, kind, srcC, embC = cfg[0], cfg[1], cfg[8], cfg[9]
    Ho, Wo = op.out_hw(Hi, Wi)
    srcs = [rnd.n(N * Hi * Wi * C) for C in srcC]
    gy = rnd.n(N * Ho * Wo * Cout)
    W.grad = _nan(W.numel()).view(W.shape)
    fuse_bias = b is not None and not embC and not f_dsb
    bias_written = b is not None and not (elsewhere and f_dsb)
    if b is not None:
        acc_bias = (cls == "Stride2PairOp" and kind == "convT") or (fuse_bias and zeroed)
        b.grad = torch.zeros(Cout, device=DEV) if acc_bias else _nan(Cout)
    emb = rnd.n(er * embC) if embC else None
    demb0 = rnd.n(er * embC) if f_demb else None
    demb = demb0.clone() if f_demb else None
    dsb = _nan(er * Cout) if f_dsb else None
    need_l = list(need) if need is not None else [True] * len(srcC)
    acc_l = list(dacc) if dacc is not None else [False] * len(srcC)
    base = [rnd.n(N * Hi * Wi * C) if (need_l[s] and acc_l[s]) else None for s, C in enumerate(srcC)]
    dsrc = [None if not need_l[s] else (base[s].clone() if acc_l[s] else _nan(N * Hi * Wi * C)) for s, C in enumerate(srcC)]
    ctx = ops.DeferredReduces.on(DEV) if deferred else _Null()
    with ctx:
        if ups_form:
            d0 = op.backward_ups(gy, srcs[0], N, Hi, Wi, n_bias, bias_grad_zeroed=zeroed)
            dsrc = [d0]
        elif cls == "Stride2PairOp":
            dsrc = op.backward(gy, srcs, N, Hi, Wi, n_bias, need=need, dsrc=dsrc, dacc=acc_l, bias_grad_zeroed=zeroed)
        else:
            dsrc = op.backward(gy, srcs, N, Hi, Wi, n_bias, emb=emb, demb=demb, need=need_l, dsrc=dsrc, dacc=acc_l,
                               dsamp_bias=dsb, emb_rows=er, bias_grad_zeroed=zeroed, bias_grad_elsewhere=elsewhere)
    st.unpack_grads()
    outs = {"weight.grad": ("conv_wgrad", W.grad)}
    if bias_written:
        outs["bias.grad"] = ("conv_bias", b.grad)
    if f_dsb:
        outs["dsamp_bias"] = ("conv_bias", dsb)
    if f_demb:
        outs["demb"] = ("conv_bias", demb)
    for s, dd in enumerate(dsrc):
        if dd is not None:
            outs[f"dsrc{s}"] = ("conv_dgrad", dd)
    dig = _finished(outs)
    if not with_ref:
        return None, dig
    # reference: autograd of the float64 forward, reductions over ALL rows (chunked), dgrad compared row by row
    W64, b64 = W.detach().double(), b.detach().double() if b is not None else None
    emb64 = emb.view(er, embC).double() if emb is not None else None
    sb64 = torch.zeros(er, Cout, device=DEV, dtype=torch.float64) if f_dsb else None
    acc = {}
    cm = {k: Cmp() for k in outs if k.startswith("dsrc")}
    per_row = Hi * Wi * (sum(srcC) + embC) * (4 if cfg[10] else 1) + Ho * Wo * Cout
    for rows in _chunks(N, per_row):
        n = rows.numel()
        xs = [s.view(N, Hi, Wi, C)[rows].double() for s, C in zip(srcs, srcC)]
        g = R.conv_grads(gy.view(N, Ho, Wo, Cout)[rows].double(), xs, W64, b64, emb=emb64, samp_bias=sb64,
                         **_conv_ref_kw(cfg, rows, n_bias, er))
        for k in ("weight", "bias", "emb", "samp_bias"):
            if k in g:
                acc[k] = acc[k] + g[k] if k in acc else g[k]
        for s, C in enumerate(srcC):
            if f"dsrc{s}" in cm:
                r = g[f"src{s}"] + (base[s].view(N, Hi, Wi, C)[rows].double() if base[s] is not None else 0)
                cm[f"dsrc{s}"].add(dsrc[s].view(N, Hi, Wi, C)[rows], r)
        del g, xs
    res_m = {k: ("conv_dgrad", c.metrics()) for k, c in cm.items()}
    res_m["weight.grad"] = ("conv_wgrad", cmp(W.grad, acc["weight"]).metrics())
    if bias_written:
        res_m["bias.grad"] = ("conv_bias", cmp(b.grad.view(1, -1), acc["bias"].view(1, -1)).metrics())
    if f_dsb:
        res_m["dsamp_bias"] = ("conv_bias", cmp(dsb.view(er, Cout), acc["samp_bias"]).metrics())
    if f_demb:
        res_m["demb"] = ("conv_bias", cmp(demb.view(er, embC), acc["emb"] + demb0.view(er, embC).double()).metrics())
    return res_m, dig


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def replay_gn(sig, rnd, ragged=False, with_ref=True):
    kind = sig[0]
    two = kind in ("gn_fwd2", "gn_bwd2")
    if two:
        Bp, P, C0, C1, G = sig[1:6]
    else:
        Bp, P, C0, G = sig[1:5]
        C1 = 0
    C = C0 + C1
    if kind == "gn_fwd":
        dual, silu, f_stats, f_drop = sig[5:9]
    elif kind == "gn_fwd2":
        dual, silu, f_stats = sig[6:9]
    elif kind == "gn_bwd":
        silu, f_res, f_res2, f_drop, deferred = sig[5:10]
        dual = True
    else:
        silu, deferred = sig[6:8]
        dual = True
    assert not (kind == "gn_fwd" and f_drop) and not (kind == "gn_bwd" and f_drop), "dropout is not on a benchmarked line"
    if ragged:
        Bp = RAGGED
    Nr = 2 * Bp if dual else Bp
    x0 = rnd.n(Nr * P * C0, scale=1.5, shift=0.3)
    x1 = rnd.n(Nr * P * C1, scale=1.5, shift=0.3) if two else None
    gam, bet = rnd.n(C, scale=0.2, shift=1.0), rnd.n(C, scale=0.2)
    stats = torch.empty(Bp * G * 4, device=DEV)
    outs = {}
    if kind in ("gn_fwd", "gn_bwd"):
        y = _nan(Nr * P * C)
        ops.groupnorm_dual_forward(x0, gam, bet, Bp, P, C, G, dual, silu, stats=stats, out=y)
    else:
        y = ops.groupnorm_dual_forward2(x0, C0, x1, C1, gam, bet, Bp, P, G, dual, silu, stats=stats)
    if kind in ("gn_fwd", "gn_fwd2"):
        outs["out"] = ("gn_fwd", y)
    else:
        gout = rnd.n(Nr * P * C)
        g0 = gout.clone()
        dga, dbe = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        r1 = rnd.n(Nr * P * C) if kind == "gn_bwd" and f_res else None
        r2 = rnd.n(Nr * P * C) if kind == "gn_bwd" and f_res2 else None
        with (ops.DeferredReduces.on(DEV) if deferred else _Null()):
            if kind == "gn_bwd":
                gx = ops.groupnorm_dual_backward(x0, gam, bet, stats, gout, dga, dbe, Bp, P, C, G, silu, residual=r1, residual2=r2)
                outs["dx"] = ("gn_bwd", gx)
            else:
                gx0, gx1 = ops.groupnorm_dual_backward2(x0, C0, x1, C1, gam, bet, stats, gout, dga, dbe, Bp, P, G, silu)
                outs["dx0"], outs["dx1"] = ("gn_bwd", gx0), ("gn_bwd", gx1)
        outs["dgamma"], outs["dbeta"] = ("gn_param", dga), ("gn_param", dbe)
    dig = _finished(outs)
    if not with_ref:
        return None, dig
    view = lambda t, Cx: t.view(Nr, P, Cx)          # noqa: E731
    xcat = lambda idx: torch.cat([view(x0, C0)[idx]] + ([view(x1, C1)[idx]] if two else []), -1).double()  # noqa: E731
    g64, b64 = gam.double(), bet.double()
    cm = {k: Cmp() for k in outs if not k.startswith("dg") and not k.startswith("db")}
    pacc = [0, 0]
    fwd = kind in ("gn_fwd", "gn_fwd2")
    for bi in (_split(_sample_rows(Bp, Bp), P * C * 12) if fwd else _chunks(Bp, P * C * 12)):
        if kind in ("gn_fwd", "gn_fwd2"):
            if dual:
                rp, rt = R.gn_dual_forward(xcat(bi), xcat(bi + Bp), g64, b64, G, silu)
                cm["out"].add(view(y, C)[bi], rp)
                cm["out"].add(view(y, C)[bi + Bp], rt)
            else:
                cm["out"].add(view(y, C)[bi], R.gn_act(xcat(bi), g64, b64, G, silu))
            continue
        gg = view(g0, C)
        dxp, dxt, dga_r, dbe_r = R.gn_dual_backward(xcat(bi), xcat(bi + Bp), g64, b64, G, silu, gg[bi].double(),
                                                    gg[bi + Bp].double())
        pacc = [pacc[0] + dga_r, pacc[1] + dbe_r]
        for idx, r in ((bi, dxp), (bi + Bp, dxt)):
            if kind == "gn_bwd":
                r = r + (view(r1, C)[idx].double() if r1 is not None else 0) + (view(r2, C)[idx].double() if r2 is not None else 0)
                cm["dx"].add(view(outs["dx"][1], C)[idx], r)
            else:
                cm["dx0"].add(view(outs["dx0"][1], C0)[idx], r[..., :C0])
                cm["dx1"].add(view(outs["dx1"][1], C1)[idx], r[..., C0:])
    res_m = {k: (outs[k][0], c.metrics()) for k, c in cm.items()}
    if kind in ("gn_bwd", "gn_bwd2"):
        res_m["dgamma"] = ("gn_param", cmp(dga.view(1, -1), pacc[0].view(1, -1)).metrics())
        res_m["dbeta"] = ("gn_param", cmp(dbe.view(1, -1), pacc[1].view(1, -1)).metrics())
    return res_m, dig


def replay_gn_affine(sig, rnd, ragged=False, with_ref=True):
    if sig[0] == "gn_affine":
        _, Bp, P, C0, C1, G = sig
        S0 = S1 = 0
    else:
        _, Bp, P, S0, C0, S1, C1, G = sig
    if ragged:
        Bp = RAGGED
    C = C0 + C1
    x0 = rnd.n(Bp * P * C0, scale=1.5, shift=0.3).view(Bp, P, C0)
    x1 = rnd.n(Bp * P * C1, scale=1.5, shift=0.3).view(Bp, P, C1) if C1 else None
    gam, bet = rnd.n(C, scale=0.2, shift=1.0), rnd.n(C, scale=0.2)
    if sig[0] == "gn_affine":
        sc, sh = ops.groupnorm_affine(x0.reshape(-1), C0, gam, bet, Bp, P, G, x1=x1.reshape(-1) if C1 else None, C1=C1)
    else:
        def cs_of(x, S):                        # per-slot fp32 channel sums, as a producing conv leaves them
            parts = torch.tensor_split(x.double(), S, dim=1)
            return torch.stack([torch.stack([p.sum(1), (p * p).sum(1)], 1) for p in parts], 1).float().reshape(-1)
        sc, sh = ops.groupnorm_affine_cs(cs_of(x0, S0), S0, C0, gam, bet, Bp, P, G, cs1=cs_of(x1, S1) if C1 else None, S1=S1, C1=C1)
    dig = _finished({"scale": ("gn_affine", sc), "shift": ("gn_affine", sh)})
    if not with_ref:
        return None, dig
    xc = torch.cat([x0] + ([x1] if C1 else []), -1).double()
    rs, rh = R.groupnorm_affine(xc, gam.double(), bet.double(), G)
    return {"scale": ("gn_affine", cmp(sc.view(Bp, C), rs).metrics()),
            "shift": ("gn_affine", cmp(sh.view(Bp, C), rh).metrics())}, dig


def replay_attn(sig, rnd, ragged=False, with_ref=True):
    kind = sig[0]
    Bp, T, C, scale = sig[1:5]
    if ragged:
        Bp = RAGGED
    Nr = Bp if kind == "attn_fwd" else 2 * Bp
    qkv = rnd.n(Nr * T * 3 * C, scale=1.2)
    outs = {}
    if kind == "attn_fwd":
        att = ops.attention_forward(qkv, _nan(Nr * T * C), Nr, T, C, scale)
        outs["out"] = ("attn_fwd", att)
    else:
        att, stats = ops.attention_dual_forward(qkv, Bp, T, C, scale)
        if kind == "attn_dual_fwd":
            outs["out"] = ("attn_fwd", att)
        else:
            datt = rnd.n(Nr * T * C)
            outs["dqkv"] = ("attn_bwd", ops.attention_dual_backward(qkv, att, datt, stats, Bp, T, C, scale))
    dig = _finished(outs)
    if not with_ref:
        return None, dig
    q = qkv.view(Nr, T, 3 * C)
    c = Cmp()
    for bi in _split(_sample_rows(Bp, Bp), T * T * 24):
        if kind == "attn_fwd":
            c.add(att.view(Nr, T, C)[bi], R.attention(q[bi].double(), scale))
        elif kind == "attn_dual_fwd":
            o, od = R.attention_dual_forward(q[bi].double(), q[bi + Bp].double(), scale)
            c.add(att.view(Nr, T, C)[bi], o)
            c.add(att.view(Nr, T, C)[bi + Bp], od)
        else:
            dv = datt.view(Nr, T, C)
            dp, dt = R.attention_dual_backward(q[bi].double(), q[bi + Bp].double(), scale, dv[bi].double(), dv[bi + Bp].double())
            dq = outs["dqkv"][1].view(Nr, T, 3 * C)
            c.add(dq[bi], dp)
            c.add(dq[bi + Bp], dt)
    k = next(iter(outs))
    return {k: (outs[k][0], c.metrics())}, dig


def replay_emb(sig, rnd, ragged=False, with_ref=True):
    kind, (K, cos, has_cb), rows, n_bias = sig[:4]
    deferred = sig[4] if kind == "emb_bwd" else False
    if ragged:
        rows, n_bias = (2 * RAGGED if rows == 2 * n_bias else RAGGED), RAGGED
    items, params = [], []
    for co, hc in zip(cos, has_cb):
        w = torch.nn.Parameter(rnd.n(co, K, scale=K ** -0.5))
        b = torch.nn.Parameter(rnd.n(co, scale=0.5))
        cb = torch.nn.Parameter(rnd.n(co)) if hc else None
        for p in (w, b, cb):
            if p is not None:
                p.grad = _nan(p.numel()).view(p.shape)
        items.append((w, b, cb))
    bank = ops.EmbBank(items, K)
    semb = rnd.n(rows * K)
    eo = [o.clone() for o in bank.forward(semb, rows, n_bias)]
    outs = {}
    if kind == "emb_fwd":
        outs = {f"out{i}": ("emb", o) for i, o in enumerate(eo)}
    else:
        douts = [rnd.n(rows * co) for co in cos]
        for d, dd in zip(bank.dout, douts):
            d.copy_(dd)
        dsemb = _nan(rows * K)
        with (ops.DeferredReduces.on(DEV) if deferred else _Null()):
            bank.backward(semb, dsemb, rows, n_bias)
        outs["dsemb"] = ("emb", dsemb)
        for i, (w, b, cb) in enumerate(items):
            outs[f"dW{i}"], outs[f"db{i}"] = ("emb", w.grad), ("emb", b.grad)
            if cb is not None:
                outs[f"dconvb{i}"] = ("emb", cb.grad)
    dig = _finished(outs)
    if not with_ref:
        return None, dig
    s64 = semb.view(rows, K).double()
    it64 = [(w.detach().double(), b.detach().double()) for w, b, _ in items]
    res_m = {}
    if kind == "emb_fwd":
        for i, r in enumerate(R.emb_bank_forward(s64, it64, n_bias)):
            res_m[f"out{i}"] = ("emb", cmp(eo[i].view(rows, -1), r).metrics())
    else:
        ds, wb = R.emb_bank_backward(s64, it64, n_bias, [d.view(rows, -1).double() for d in douts])
        res_m["dsemb"] = ("emb", cmp(dsemb.view(rows, K), ds).metrics())
        for i, (w, b, cb) in enumerate(items):
            res_m[f"dW{i}"] = ("emb", cmp(w.grad, wb[i][0]).metrics())
            res_m[f"db{i}"] = ("emb", cmp(b.grad.view(1, -1), wb[i][1].view(1, -1)).metrics())
            if cb is not None:
                res_m[f"dconvb{i}"] = ("emb", cmp(cb.grad.view(1, -1), wb[i][1].view(1, -1)).metrics())
    return res_m, dig


def replay_act(sig, rnd, ragged=False, with_ref=True):
    kind, act, numel = sig[:3]
    dual = sig[3] if kind == "act_fwd" else True
    if ragged:
        numel = (2 if dual else 1) * 4 * RAGGED * 7
    z = rnd.n(numel, scale=2.0)
    half = numel // 2 if dual else numel
    if kind == "act_fwd":
        h = ops.act_dual_forward(act, z, _nan(numel), dual)
        outs = {"out": ("act", h)}
    else:
        g = rnd.n(numel)
        g0 = g.clone()
        ops.act_dual_backward(act, z, g)
        outs = {"dz": ("act", g)}
    dig = _finished(outs)
    if not with_ref:
        return None, dig
    z64 = z.double()
    if kind == "act_fwd":
        if dual:
            hp, ht = R.act_dual_forward(act, z64[:half], z64[half:])
            r = torch.cat([hp, ht])
        else:
            r = R.ACTS[act](z64)
        return {"out": ("act", cmp(h.view(1, -1), r.view(1, -1)).metrics())}, dig
    dp, dt = R.act_dual_backward(act, z64[:half], z64[half:], g0[:half].double(), g0[half:].double())
    return {"dz": ("act", cmp(g.view(1, -1), torch.cat([dp, dt]).view(1, -1)).metrics())}, dig


def replay_bmm(sig, rnd, ragged=False, with_ref=True):
    """A recorded ops.bmm call on random operands through the per-element float64 checker of the composed-attention tests
    (it asserts by itself: the GEMM bound is a-priori, not one of BOUNDS).  Ragged: 13 batches; an offset that is a multiple of
    the recorded batch extent (the tangent half, a head's tiles) moves with the batch count."""
    from test_composed_attention_gpu import run_bmm_case
    _, M, N, K, batch, sA, sB, sC, a_off, b_off, c_off, alpha, acc, p2, th = sig
    nb = RAGGED if ragged else batch
    mv = lambda off, s: off % (batch * s[0]) + (off // (batch * s[0])) * nb * s[0]          # noqa: E731
    case = dict(name=" ".join(str(v) for v in sig[1:]) + (f" ragged({RAGGED})" if ragged else ""), M=M, N=N, K=K, batch=nb, sA=sA,
                sB=sB, sC=sC, a_off=mv(a_off, sA), b_off=mv(b_off, sB), c_off=mv(c_off, sC), alpha=alpha, acc=acc,
                pair2=p2 is not None, third=th is not None, a2_off=mv(p2[0], sA) if p2 else 0, b2_off=mv(p2[1], sB) if p2 else 0,
                b3_off=mv(th[0], sB) if th else 0, c3_off=mv(th[1], sC) if th else 0)
    label, out = run_bmm_case(ops, case, seed=int(rnd.g.initial_seed()))
    assert label != "unsupported"
    return {}, {"C": digest(out)}


def replay_softmax(sig, rnd, ragged=False, with_ref=True):
    """The dual softmax at the recorded row count (forward without and with the tangent, and the backward, whichever of them
    was recorded) through the per-element float64 checker of the composed-attention tests."""
    import attn_composed_ref as AR
    from test_composed_attention_gpu import run_softmax
    rows, T = sig[1:3]
    rows = RAGGED * T if ragged else rows
    outs = run_softmax(ops, *AR.softmax_inputs(T, int(rnd.g.initial_seed()), rows), f"{sig[0]} rows={rows} T={T}")
    return {}, {k: digest(v) for k, v in outs.items()}


REPLAY = {"bmm": replay_bmm, "softmax_fwd": replay_softmax, "softmax_bwd": replay_softmax, "conv_fwd": replay_conv_fwd, "conv_bwd": replay_conv_bwd,
          "conv_bwd_ups": lambda s, r, **k: replay_conv_bwd(s, r, ups_form=True, **k),
          "gn_fwd": replay_gn, "gn_bwd": replay_gn, "gn_fwd2": replay_gn, "gn_bwd2": replay_gn,
          "gn_affine": replay_gn_affine, "gn_affine_cs": replay_gn_affine,
          "attn_fwd": replay_attn, "attn_dual_fwd": replay_attn, "attn_dual_bwd": replay_attn,
          "emb_fwd": replay_emb, "emb_bwd": replay_emb, "act_fwd": replay_act, "act_bwd": replay_act}


def _seed(i, ragged):
    return 1000 * i + (7 if ragged else 0)


def _label(sig):
    if sig[0].startswith("conv"):
        cfg = sig[1]
        return f"{sig[0]} {cfg[0][:6]} {cfg[1]} k{cfg[4]}x{cfg[5]} s{cfg[6]} src{list(cfg[8])} emb{cfg[9]} ups{int(cfg[10])} " \
               f"wino{int(cfg[11])} Co{cfg[2][1] if cfg[1] == 'convT' else cfg[2][0]} N{sig[2]} {sig[3]}x{sig[4]}"
    return " ".join(str(v) for v in sig)


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("config", CONFIGS)
def test_census_is_complete(config):
    sigs, missing_f, missing_b = census(config)
    kinds = {}
    for s in sigs:
        kinds[s[0]] = kinds.get(s[0], 0) + 1
    print(f"\n{config}: {len(sigs)} distinct signatures " + " ".join(f"{k}:{v}" for k, v in sorted(kinds.items())))
    assert not missing_f, f"convolutions of the net that no forward call reached: {missing_f}"
    assert not missing_b, f"convolutions of the net that no backward call reached: {missing_b}"
    assert all(s[0] in REPLAY for s in sigs)


@pytest.mark.parametrize("config", CONFIGS)
def test_every_layer_vs_float64(config):
    sigs, _, _ = census(config)
    print(f"\n{config}: {len(sigs)} distinct signatures; per output: rel-L2 | worst row rel-L2 | worst elem / RMS  (bounds)")
    bad = []
    worst = {}
    for i, sig in enumerate(sigs):
        for ragged in (False, True):
            res, _ = REPLAY[sig[0]](sig, Rand(_seed(i, ragged)), ragged=ragged)
            for name, (fam, m) in res.items():
                b = BOUNDS[fam]
                ok = all(v <= bb for v, bb in zip(m, b))
                w = worst.setdefault(fam, [0.0, 0.0, 0.0])
                worst[fam] = [max(x, y) for x, y in zip(w, m)]
                print(f"  {f'ragged({RAGGED}) ' if ragged else ''}{_label(sig)} {name}: {m[0]:.2e} | {m[1]:.2e} | {m[2]:.2e}  "
                      f"({b[0]:.0e} {b[1]:.0e} {b[2]:.0e}){'' if ok else '  <-- OUT OF BOUNDS'}")
                if not ok:
                    bad.append((config, ragged, sig, name, m))
            gc.collect()
            torch.cuda.empty_cache()
    print(f"{config} worst per family: " + "; ".join(f"{k} {v[0]:.1e}/{v[1]:.1e}/{v[2]:.1e}" for k, v in sorted(worst.items())))
    assert not bad, bad


@pytest.mark.parametrize("config", CONFIGS)
def test_reverse_order_replay_is_bitwise(config):
    """Every signature replayed after all the others (reverse order, fresh NaN pre-fills) gives the bits of its replay in
    census order: no kernel's result depends on what ran before it (workspaces, arenas, caches)."""
    sigs, _, _ = census(config)
    first = [REPLAY[s[0]](s, Rand(_seed(i, False)), with_ref=False)[1] for i, s in enumerate(sigs)]
    torch.cuda.empty_cache()
    diff = []
    for i in reversed(range(len(sigs))):
        d = REPLAY[sigs[i][0]](sigs[i], Rand(_seed(i, False)), with_ref=False)[1]
        if d != first[i]:
            diff.append((_label(sigs[i]), [k for k in d if d[k] != first[i].get(k)]))
    assert not diff, diff


def test_comparator_rejects_small_localised_errors():
    """A real kernel output at the C4 row count (a plain 3x3 forward of the C4 step: 512 dual rows of 64x64): (a) one
    element of the last row's last tile moved by 1e-3 x RMS, (b) two channels of one pixel swapped (norms preserved).
    The per-element / per-row metrics reject both, though the tensor-wide rel-L2 of (a) and the norm and head of (b) do
    not move past fp32 noise."""
    sigs, _, _ = census("c4_b256")
    sig = next(s for s in sigs if s[0] == "conv_fwd" and s[1][4] == 3 and s[2] == 512 and s[3] == 64 and len(s[1][8]) == 1
               and not s[1][10] and not any(s[7:12]))
    _, cfg, N, Hi, Wi, n_bias = sig[:6]
    rnd = Rand(5)
    op, _, W, b, Cout = _make_conv(cfg, rnd, False)
    C = cfg[8][0]
    x = rnd.n(N * Hi * Wi * C)
    out, Ho, Wo = op.forward([x], N, Hi, Wi, n_bias, out=_nan(N * Hi * Wi * Cout))
    ref = torch.cat([R.conv_forward([x.view(N, Hi, Wi, C)[rows].double()], W.detach().double(), b.detach().double(), pad=1,
                                    rows=rows, n_bias=n_bias) for rows in _chunks(N, Hi * Wi * (C + Cout))])
    y = out.view(N, Ho, Wo, Cout)
    m0 = cmp(y, ref).metrics()
    assert within_bounds(m0, "conv_fwd"), m0
    rms = float(ref.pow(2).mean().sqrt())
    ya = y.clone()
    ya[N - 1, Ho - 1, Wo - 1, Cout - 1] += 1e-3 * rms
    ma = cmp(ya, ref).metrics()
    yb = y.clone()
    yb[N - 1, Ho - 1, Wo - 2, [0, 1]] = y[N - 1, Ho - 1, Wo - 2, [1, 0]]
    mb = cmp(yb, ref).metrics()
    print(f"\nunchanged {m0}\n(a) one element +1e-3 RMS {ma}\n(b) two channels of one pixel swapped {mb}")
    assert ma[0] <= BOUNDS["conv_fwd"][0], "the tensor-wide rel-L2 alone would have caught (a)"
    assert abs(float(yb.norm()) / float(y.norm()) - 1) <= 1e-6 and torch.equal(yb.view(-1)[:8], y.view(-1)[:8])   # norm, head
    assert not within_bounds(ma, "conv_fwd") and not within_bounds(mb, "conv_fwd")
