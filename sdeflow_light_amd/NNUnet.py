"""2-D U-Net score network on HIP kernels — host mirror of the reference's
``NNUnet.py`` + ``model/unet.py`` (``VorticityUNet`` / ``UNetModelWithLogNorm``):
same constructor signature and ``state_dict`` keys (``core.time_embed.*``,
``core.input_blocks.N.0.{in_layers,emb_layers,out_layers,skip_connection}.*``,
``…N.1.{norm,qkv,proj_out}.*``, ``…N.0.op.*``, ``core.middle_block.*``,
``core.output_blocks.N.K.*`` (``.conv`` for Upsample), ``core.out.{0,2}.*``;
model/unet.py:338-446).

The ``nn`` children only hold parameters (PyTorch layouts); the computation is a
hand-scheduled pipeline of the implicit-GEMM conv kernels, the dual GroupNorm+SiLU
kernels and the attention pieces (batched MFMA GEMM + dual softmax), channels-last,
with the forward-mode tangent as the second half of the batch and a hand-written
backward (no autograd tape, no double backward).

Extension over the reference wrapper: ``channels`` (default
1) lets the flat state be ``(B, channels*H*W)`` — needed for the 64x64x3 config;
the core UNet upstream already supports any ``in_channels``.
"""
from __future__ import annotations

import math
import os
from typing import List, Literal, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from ._lib import MsgmError, PhiloxState
from .NN import FlatParamMixin
from .convnet import ConvOp, ConvOpSet

SILU = ops.ACT_SILU
scale_image = 5          # NNUnet.py:19
# the kernels' width limits (csrc/unet2d_kernels.hip: GN_MAX_C, gn_max_c; k_emb_bank's K), checked by VorticityUNet._build
GN_MAX_C, GN_MAX_C_SCALAR, EMB_MAX_K = 1024, 256, 512


def flat_to_img(x: torch.Tensor, H: int, W: int, order: Literal["C", "F"] = "C") -> torch.Tensor:
    """x (B, H*W) / scale_image -> (B, 1, H, W), C or F (column-major) ordering (NNUnet.py:26-51) — one kernel."""
    B, d = x.shape
    assert d == H * W, f"Expected d={H * W}, got {d}"
    return ops.flat_to_image(x.contiguous().float(), B, 1, H, W, order == "F", 1.0 / scale_image).view(B, 1, H, W)


def img_to_flat(y: torch.Tensor, order: Literal["C", "F"] = "C") -> torch.Tensor:
    """y (B, 1, H, W) * scale_image -> (B, H*W) (NNUnet.py:53-77)."""
    B, C, H, W = y.shape
    assert C == 1, f"Expected 1 channel, got {C}"
    return ops.image_to_flat(y.contiguous().float().view(-1), B, 1, H, W, order == "F", float(scale_image))


def zero_module(m):
    for p in m.parameters():
        p.detach().zero_()
    return m


def _norm(c):            # normalization(): GroupNorm32(min(c,32), c)      model/nn_utils.py:107-114
    return nn.GroupNorm(min(c, 32), c)


class ResBlock(nn.Module):
    """Parameter holder with the reference's child names (model/unet.py:139-168).  out_layers[2] is the reference's
    Dropout(p) (no parameters; train() / eval() switch it as in torch); the HIP path applies it inside the GroupNorm+SiLU
    kernels of out_layers[0]."""

    def __init__(self, channels, emb_channels, out_channels, dropout=0.0):
        super().__init__()
        self.channels, self.out_channels = channels, out_channels
        self.in_layers = nn.Sequential(_norm(channels), nn.Identity(), nn.Conv2d(channels, out_channels, 3, padding=1))
        self.emb_layers = nn.Sequential(nn.Identity(), nn.Linear(emb_channels, out_channels))
        self.out_layers = nn.Sequential(_norm(out_channels), nn.Identity(), nn.Dropout(p=dropout),
                                        zero_module(nn.Conv2d(out_channels, out_channels, 3, padding=1)))
        self.skip_connection = nn.Identity() if out_channels == channels else nn.Conv2d(channels, out_channels, 1)


class AttentionBlock(nn.Module):
    """model/unet.py:197-231.  num_heads splits the C channels into heads of D = C / num_heads: head h owns the qkv channels
    [3Dh, 3D(h+1)) (q | k | v of D each; qkv.reshape(B*H, 3D, T), unet.py:225) and the output channels [Dh, D(h+1))."""

    def __init__(self, channels, num_heads=1):
        super().__init__()
        if num_heads < 1 or channels % num_heads != 0:
            raise MsgmError(f"AttentionBlock: {channels} channels do not split into num_heads = {num_heads} heads")
        self.channels, self.num_heads = channels, num_heads
        self.norm = _norm(channels)
        self.qkv = nn.Conv1d(channels, channels * 3, 1)
        self.proj_out = zero_module(nn.Conv1d(channels, channels, 1))


class Downsample(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.op = nn.Conv2d(channels, channels, 3, stride=2, padding=1)


class Upsample(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.conv = nn.Conv2d(channels, channels, 3, padding=1)


class UNetModelWithLogNorm(nn.Module):
    """Topology of UNetModel.__init__ (model/unet.py:300-446) for dims=2, conv_resample, no scale-shift norm, no classes;
    any num_heads / num_heads_upsample whose heads divide the channel counts of the attention blocks; any dropout in [0, 1)
    (every ResBlock's out_layers, model/unet.py:152-158)."""

    def __init__(self, in_channels, model_channels, out_channels, in_space, num_res_blocks, attention_resolutions,
                 dropout=0, channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, num_classes=None, use_checkpoint=False,
                 num_heads=1, num_heads_upsample=-1, use_scale_shift_norm=False, learn_potential=False, use_log_norm=False):
        super().__init__()
        if dims != 2 or not conv_resample or num_classes is not None or use_scale_shift_norm or learn_potential:
            raise MsgmError("HIP U-Net is built for the driver's options (dims=2, conv_resample, no scale-shift norm, "
                            "no learn_potential, no classes)")
        dropout = float(dropout)
        if not 0.0 <= dropout < 1.0:
            raise MsgmError(f"dropout {dropout} outside [0, 1)")
        self.dropout = dropout
        if num_heads_upsample == -1:                                    # model/unet.py:321-322
            num_heads_upsample = num_heads
        self.num_heads, self.num_heads_upsample = num_heads, num_heads_upsample
        self.use_log_norm = use_log_norm
        self.in_channels, self.model_channels, self.out_channels = in_channels, model_channels, out_channels
        self.channel_mult, self.num_res_blocks = tuple(channel_mult), num_res_blocks
        self.attention_resolutions = tuple(attention_resolutions)
        ted = model_channels * 4
        self.time_embed = nn.Sequential(nn.Linear(model_channels, ted), nn.Identity(), nn.Linear(ted, ted))
        if use_log_norm:               # mirrors the time MLP for log||x|| (NNUnet.py:88-94)
            self.scale_embed = nn.Sequential(nn.Linear(model_channels, ted), nn.Identity(), nn.Linear(ted, ted))
        ch = model_channels * channel_mult[0]
        self.input_blocks = nn.ModuleList([nn.Sequential(nn.Conv2d(in_channels, ch, 3, padding=1))])
        chans, ds = [ch], 1
        for level, mult in enumerate(channel_mult):
            for _ in range(num_res_blocks):
                layers = [ResBlock(ch, ted, mult * model_channels, dropout)]
                ch = mult * model_channels
                if ds in attention_resolutions:
                    layers.append(AttentionBlock(ch, num_heads))
                self.input_blocks.append(nn.Sequential(*layers))
                chans.append(ch)
            if level != len(channel_mult) - 1:
                self.input_blocks.append(nn.Sequential(Downsample(ch)))
                chans.append(ch)
                ds *= 2
        self.middle_block = nn.Sequential(ResBlock(ch, ted, ch, dropout), AttentionBlock(ch, num_heads),
                                          ResBlock(ch, ted, ch, dropout))
        self.output_blocks = nn.ModuleList([])
        for level, mult in list(enumerate(channel_mult))[::-1]:
            for i in range(num_res_blocks + 1):
                layers = [ResBlock(ch + chans.pop(), ted, model_channels * mult, dropout)]
                ch = model_channels * mult
                if ds in attention_resolutions:
                    layers.append(AttentionBlock(ch, num_heads_upsample))
                if level and i == num_res_blocks:
                    layers.append(Upsample(ch))
                    ds //= 2
                self.output_blocks.append(nn.Sequential(*layers))
        self.out = nn.Sequential(_norm(ch), nn.Identity(), zero_module(nn.Conv2d(model_channels * channel_mult[0], out_channels, 3, padding=1)))


# ----------------------------------------------------------------------------- executable ops
class _TwoSrc(NamedTuple):
    """The two-source twins of a decoder ResBlock whose input is (h, skip) with ``split`` = (C0, C1) channels."""
    split: Tuple[int, int]
    conv1: ConvOp            # sampler: conv1 on the two tensors
    skip: ConvOp             # sampler: the 1x1 skip conv on the two tensors
    skip_t: ConvOp           # training: the same, with a gradient image of its own


class _Res:
    def __init__(self, m: ResBlock):
        self.m = m
        ci, co = m.channels, m.out_channels
        self.ci, self.co = ci, co
        self.conv1 = ConvOp(m.in_layers[2].weight, m.in_layers[2].bias, "conv", (3, 3), 1, 1, [ci])
        # the embedding projection emb_layers[1] runs in the network's ops.EmbBank (one launch for all ResBlocks);
        # bank_i = this block's index in it
        self.bank_i = -1
        self.conv2 = ConvOp(m.out_layers[3].weight, m.out_layers[3].bias, "conv", (3, 3), 1, 1, [co])
        self.skip = None if isinstance(m.skip_connection, nn.Identity) else \
            ConvOp(m.skip_connection.weight, m.skip_connection.bias, "conv", (1, 1), 1, 0, [ci])
        self.ops = [self.conv1, self.conv2] + ([self.skip] if self.skip else [])
        self.two: Optional[_TwoSrc] = None     # decoder blocks that can read (h, skip) without the concatenation

    def make_two_source(self, C0: int, C1: int):
        """Decoder ResBlocks read cat([h, skip]) (model/unet.py:514).  The concatenation is never materialised: GroupNorm
        (statistics), the 1x1 skip conv and, on the sampler path, conv1 read the two tensors directly.  The twins share the
        weight Parameters and only differ in the packed layout (each source padded to 16 channels)."""
        m = self.m
        if self.skip is None or C0 + C1 != self.ci:
            raise MsgmError("two-source twins are for decoder ResBlocks with a skip convolution")
        conv = lambda src, k, pad: ConvOp(src.weight, src.bias, "conv", (k, k), 1, pad, [C0, C1])       # noqa: E731
        # training: GroupNorm reads the two tensors and writes ONE normalised tensor (conv1 stays single-source); only the
        # 1x1 skip conv needs a two-source twin, with its own gradient image (it REPLACES self.skip on that path)
        self.two = _TwoSrc((C0, C1), conv(m.in_layers[2], 3, 1), conv(m.skip_connection, 1, 0), conv(m.skip_connection, 1, 0))

    # the twins under the names the layer census knows them by
    split = property(lambda self: self.two.split if self.two else None)
    conv1_2 = property(lambda self: self.two.conv1 if self.two else None)
    skip_2 = property(lambda self: self.two.skip if self.two else None)
    skip_2t = property(lambda self: self.two.skip_t if self.two else None)


class _Attn:
    def __init__(self, m: AttentionBlock):
        self.m, self.c = m, m.channels
        self.nh = m.num_heads
        self.d = m.channels // m.num_heads             # channels per head
        self.qkv = ConvOp(m.qkv.weight, m.qkv.bias, "conv", (1,), 1, 0, [m.channels])
        self.proj = ConvOp(m.proj_out.weight, m.proj_out.bias, "conv", (1,), 1, 0, [m.channels])
        self.ops = [self.qkv, self.proj]


def _attn_kernel(a: _Attn, dual: bool):
    """(supported, forward, backward, head arguments) of the fused attention kernels for a's head count: the single-head
    entries take (T, C), the multi-head ones (T, heads, D).  Looked up on ``ops`` at every call."""
    if dual:
        fns = (ops.attention_dual_supported, ops.attention_dual_forward, ops.attention_dual_backward) if a.nh == 1 else \
            (ops.attention_dual_mh_supported, ops.attention_dual_mh_forward, ops.attention_dual_mh_backward)
    else:
        fns = (ops.attention_supported, ops.attention_forward, None) if a.nh == 1 else \
            (ops.attention_mh_supported, ops.attention_mh_forward, None)
    return fns + ((a.c,) if a.nh == 1 else (a.nh, a.d),)


def _attn_small(a: _Attn, T: int) -> bool:
    """True when the one-launch T = 16 kernels (ops.attention_small_*) take the block: decided by shape alone, at any head
    count.  Looked up on ``ops`` at every call."""
    return T == 16 and ops.attention_small_supported(T, a.nh, a.d)


class _Pass:
    """What one pass through the network shares.  There are two modes: the sampler (``tape`` None: no tangent, nothing
    kept) and training (``tape`` a list: dual numbers, the tangent being the second half of the N = 2 Bp rows, and every
    forward piece leaves its record on the tape for _backward)."""
    def __init__(self, N: int, Bp: int, tape: Optional[list], drop: Optional[PhiloxState]):
        self.N, self.Bp, self.tape, self.train = N, Bp, tape, tape is not None
        self.drop = drop                 # Philox state the pass draws its dropout masks from (None: dropout inactive)
        self.er, self.eo = Bp, None      # set by _run: rows that carry an embedding, the embedding bank's output per ResBlock


_SAVE_SKIP = ("save_skip",)              # tape marker: the tensor the record in front produced also went on the skip stack


class VorticityUNet(nn.Module, FlatParamMixin):
    def __init__(self, base_channels: int = 32, channel_mults=(1, 2, 4), num_res_blocks: int = 2, emb_dim_ignored: int = 128,
                 dropout: float = 0.0, premodule: Optional[str] = None, in_space: int = 16, attention_resolutions=(2, 4),
                 conv_resample: bool = True, num_heads: int = 1, use_checkpoint: bool = False, learn_potential: bool = False,
                 flatten_order: Literal["C", "F"] = "C", channels: int = 1):
        super().__init__()
        assert premodule in (None, "NormalizeLogRadius")
        self.pre = premodule == "NormalizeLogRadius" or None
        self.in_space = int(in_space)
        assert flatten_order in ("C", "F")
        self.flatten_order = flatten_order
        self.channels = channels
        self.core = UNetModelWithLogNorm(in_channels=channels, model_channels=base_channels, out_channels=channels,
                                         in_space=in_space, num_res_blocks=num_res_blocks,
                                         attention_resolutions=attention_resolutions, dropout=dropout,
                                         channel_mult=tuple(channel_mults), conv_resample=conv_resample, dims=2,
                                         num_classes=None, use_checkpoint=use_checkpoint, num_heads=num_heads,
                                         use_scale_shift_norm=False, learn_potential=learn_potential,
                                         use_log_norm=(premodule == "NormalizeLogRadius"))
        self._x = None
        self._flat = None
        self.dropout_rng: Optional[PhiloxState] = None     # the net's own mask stream (train-mode forward); replaceable

    def dropout_active(self) -> bool:
        """Dropout draws masks iff the net is in training mode and p > 0 (torch Dropout semantics)."""
        return self.training and self.core.dropout > 0

    def dropout_stream(self, device) -> PhiloxState:
        """The stream a train-mode ``forward`` draws its masks from: created on first use (like SDE.philox), replaceable by
        assigning ``dropout_rng``.  A pass advances it by 1."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.dropout_rng is None or self.dropout_rng.state.device != device:
            if torch.cuda.is_current_stream_capturing():
                raise MsgmError("the U-Net's dropout stream is created for the first time inside a graph capture; "
                                "run one eager step first")
            self.dropout_rng = PhiloxState(int(torch.initial_seed()) ^ 0xD409, device)
        return self.dropout_rng

    # ------------------------------------------------------------------ build
    def _check_widths(self):
        """What the kernels cannot run, found on the plan before the first launch of the first pass (inside a capture too):
        the GroupNorm kernels take C <= GN_MAX_C channels when C % 4 == 0 and C <= GN_MAX_C_SCALAR otherwise (a decoder
        ResBlock's in-norm sees cat([h, skip])), the embedding bank K = 4 model_channels <= EMB_MAX_K."""
        core = self.core
        if self._x is not None:          # a built plan passed
            return
        if 4 * core.model_channels > EMB_MAX_K:
            raise MsgmError(f"core.time_embed: 4 * model_channels = {4 * core.model_channels} is wider than the embedding bank's "
                            f"K <= {EMB_MAX_K} (base_channels <= {EMB_MAX_K // 4})")
        for name, m in core.named_modules():
            if not isinstance(m, nn.GroupNorm):
                continue
            C = m.num_channels
            if C > GN_MAX_C:
                raise MsgmError(f"core.{name}: GroupNorm over {C} channels; the GroupNorm kernels take C <= {GN_MAX_C}")
            if C > GN_MAX_C_SCALAR and C % 4:
                raise MsgmError(f"core.{name}: GroupNorm over {C} channels; above {GN_MAX_C_SCALAR} channels the GroupNorm "
                                f"kernels take only C % 4 == 0")

    def _build(self):
        self._check_widths()
        self.flat_parameters()
        core = self.core
        first = core.time_embed[0].weight
        if self._x is not None and self._x["t0"].weight is first and self._x["t0"].Wp.device == first.device:
            return self._x
        mc = core.model_channels
        x = {"t0": ConvOp(core.time_embed[0].weight, core.time_embed[0].bias, "linear", (1,), 1, 0, [mc]),
             "t2": ConvOp(core.time_embed[2].weight, core.time_embed[2].bias, "linear", (1,), 1, 0, [4 * mc])}
        if core.use_log_norm:
            x["s0"] = ConvOp(core.scale_embed[0].weight, core.scale_embed[0].bias, "linear", (1,), 1, 0, [mc])
            x["s2"] = ConvOp(core.scale_embed[2].weight, core.scale_embed[2].bias, "linear", (1,), 1, 0, [4 * mc])

        def wrap(seq):
            out = []
            for layer in seq:
                if isinstance(layer, ResBlock):
                    out.append(("res", _Res(layer)))
                elif isinstance(layer, AttentionBlock):
                    out.append(("attn", _Attn(layer)))
                elif isinstance(layer, Downsample):
                    c = layer.op.in_channels
                    out.append(("down", ConvOp(layer.op.weight, layer.op.bias, "conv", (3, 3), 2, 1, [c])))
                elif isinstance(layer, Upsample):
                    c = layer.conv.in_channels
                    out.append(("up", ConvOp(layer.conv.weight, layer.conv.bias, "conv", (3, 3), 1, 1, [c], ups=True)))
                elif isinstance(layer, nn.Conv2d):
                    out.append(("conv", ConvOp(layer.weight, layer.bias, "conv", (3, 3), 1, 1, [layer.in_channels])))
                else:
                    raise MsgmError(f"unexpected layer {type(layer)}")
            return out
        x["in"] = [wrap(b) for b in core.input_blocks]
        x["mid"] = wrap(core.middle_block)
        x["outb"] = [wrap(b) for b in core.output_blocks]
        x["fin"] = ConvOp(core.out[2].weight, core.out[2].bias, "conv", (3, 3), 1, 1, [core.out[2].in_channels])
        allops = [x["t0"], x["t2"], x["fin"]] + ([x["s0"], x["s2"]] if core.use_log_norm else [])
        for blk in x["in"] + [x["mid"]] + x["outb"]:
            for kind, o in blk:
                allops += o.ops if kind in ("res", "attn") else [o]
        x["all"] = allops
        x["set"] = ConvOpSet(allops)
        res = [o for blk in x["in"] + [x["mid"]] + x["outb"] for kind, o in blk if kind == "res"]
        for i, r in enumerate(res):
            r.bank_i = i
        x["bank"] = ops.EmbBank([(r.m.emb_layers[1].weight, r.m.emb_layers[1].bias, r.m.in_layers[2].bias) for r in res], 4 * mc)
        # channel count after every input block = the skip tensors the decoder pops (model/unet.py:506-514)
        chans = []
        for blk in x["in"]:
            kind, o = blk[-1] if blk[-1][0] != "attn" else blk[-2]
            chans.append(o.co if kind == "res" else o.Cout)
        twins = []
        for blk in x["outb"]:
            Cs = chans.pop()
            kind, res = blk[0]
            if kind == "res" and res.skip is not None and res.ci > Cs and (res.ci - Cs) % 16 == 0 and Cs % 16 == 0:
                res.make_two_source(res.ci - Cs, Cs)
                twins.append(res.two)
        # the twins' own op sets, one per mode; None (no twins, or a test's switch): the decoder concatenates
        x["set2"] = ConvOpSet([o for tw in twins for o in (tw.conv1, tw.skip)]) if twins else None
        x["set2t"] = ConvOpSet([tw.skip_t for tw in twins]) if twins else None
        self._x = x
        return x

    # ------------------------------------------------------------------ forward pieces
    def _gn(self, ctx: _Pass, gnm: nn.GroupNorm, h, P, C, silu, dropout=None):
        """GroupNorm (+SiLU) as a pass of its own; the training pass keeps the statistics for the backward."""
        G = gnm.num_groups
        stats = torch.empty(ctx.Bp * G * 4, device=h.device) if ctx.train else None
        return ops.groupnorm_dual_forward(h, gnm.weight.detach(), gnm.bias.detach(), ctx.Bp, P, C, G, ctx.train, silu, stats=stats,
                                          dropout=dropout), stats

    def _gn_fold(self, gnm: nn.GroupNorm, x, Bp, P, C, x1=None, C1=0):
        """GroupNorm as a per-(sample, channel) affine map for a conv that applies it while staging its input.  When the
        convolution(s) that produced x (and x1, the concatenated second source) left their per-channel sums on the tensor
        (ConvOp.forward(stats=True)), the statistics come from those few KB instead of a pass over the tensor."""
        cs = getattr(x, "_msgm_cs", None)
        cs1 = getattr(x1, "_msgm_cs", None) if x1 is not None else None
        if cs is not None and (x1 is None or cs1 is not None):
            return ops.groupnorm_affine_cs(cs[0], cs[1], C, gnm.weight.detach(), gnm.bias.detach(), Bp, P, gnm.num_groups,
                                           cs1=cs1[0] if cs1 is not None else None, S1=cs1[1] if cs1 is not None else 0, C1=C1)
        return ops.groupnorm_affine(x, C, gnm.weight.detach(), gnm.bias.detach(), Bp, P, gnm.num_groups, x1=x1, C1=C1)

    class ResRec(NamedTuple):
        """Tape record of one ResBlock, on one source ([x]) or two ([h, skip], a decoder block without the concatenation)."""
        r: _Res
        srcs: List[torch.Tensor]
        H: int
        W: int
        h1: torch.Tensor                 # in_layers' GroupNorm + SiLU = conv1's input, and its statistics
        st1: torch.Tensor
        h2: torch.Tensor                 # conv1's output
        st2: torch.Tensor
        h3: torch.Tensor                 # out_layers' GroupNorm + SiLU (+ dropout) = conv2's input
        dd: Optional[object]             # msgm_dropout_t of the block's masks (None: no dropout)

    def _res_fwd(self, ctx: _Pass, r: _Res, srcs, H, W):
        """One ResBlock on srcs = [x], or [h, skip] for a decoder block that never materialises cat([h, skip]) (_run enters
        that way only where the twins exist and, on the sampler path, conv1's twin can transform its input).  DESIGN §4e has
        the decisions below as a table."""
        N, Bp, P, train = ctx.N, ctx.Bp, H * W, ctx.train
        two = r.two if len(srcs) == 2 else None
        C0, C1 = two.split if two else (r.ci, 0)
        gn1, gn2 = r.m.in_layers[0], r.m.out_layers[0]
        eo = ctx.eo[r.bank_i]                                    # emb_layers projection, er rows (N with log-radius conditioning)
        dd = None if ctx.drop is None else ops.dropout_desc(ctx.drop, r.bank_i, self.core.dropout)
        skip = r.skip if two is None else two.skip_t if train else two.skip
        # in-norm.  Sampler: GroupNorm + SiLU are applied by conv1 while it stages its input tile (the normalised tensor never
        # exists); a single-source block does so only when conv2 can as well, a block that folds also takes the Winograd
        # kernels and leaves channel sums for the next GroupNorm.  Training: materialised, with the statistics kept.
        fold = not train and (two is not None or (r.conv1.can_transform_input(N, H, W) and r.conv2.can_transform_input(N, H, W)))
        aff = h1 = st1 = None
        if fold:
            aff = self._gn_fold(gn1, srcs[0], Bp, P, C0, x1=srcs[1] if two else None, C1=C1)
        elif two:
            st1 = torch.empty(Bp * gn1.num_groups * 4, device=srcs[0].device)
            h1 = ops.groupnorm_dual_forward2(srcs[0], C0, srcs[1], C1, gn1.weight.detach(), gn1.bias.detach(), Bp, P, gn1.num_groups,
                                             True, True, stats=st1)
        else:
            h1, st1 = self._gn(ctx, gn1, srcs[0], P, r.ci, True)
        # training: conv1 stays single-source on the one tensor the two-source GroupNorm wrote
        conv1 = two.conv1 if two and fold else r.conv1
        h2, _, _ = conv1.forward(srcs if fold else [h1], N, H, W, Bp, samp_bias=eo, emb_rows=ctx.er, in_affine=aff, in_act=int(fold),
                                 wino=fold, stats=fold)
        # skip: the 1x1 skip conv writes `out` and conv2 accumulates onto it; without one the residual is added in conv2's
        # epilogue (unet.py:187).  The two-source sampler block launches it here, every other block after the out-norm.
        run_skip = lambda: skip.forward(srcs, N, H, W, Bp)[0] if skip is not None else None        # noqa: E731
        out = run_skip() if two is not None and not train else None
        # out-norm: folded into conv2 like the in-norm (a two-source block asks conv2 on its own), materialised otherwise;
        # dropout always materialises it: the GroupNorm kernel applies the mask and conv2 reads the result unfused
        fold2 = fold and dd is None and (two is None or r.conv2.can_transform_input(N, H, W))
        aff2 = h3 = st2 = None
        if fold2:
            aff2 = self._gn_fold(gn2, h2, Bp, P, r.co)
        else:
            h3, st2 = self._gn(ctx, gn2, h2, P, r.co, True, dropout=dd)
        if out is None:
            out = run_skip()
        out, _, _ = r.conv2.forward([h2 if fold2 else h3], N, H, W, Bp, out=out, accumulate=skip is not None,
                                    residual=None if skip is not None else srcs[0], in_affine=aff2, in_act=int(fold2),
                                    wino=fold, stats=fold)
        if train:
            ctx.tape.append(self.ResRec(r, srcs, H, W, h1, st1, h2, st2, h3, dd))
        return out

    class AttnRec(NamedTuple):
        """Tape record of one attention block.  The fused kernel keeps its per-query statistics (``row_stats``), the composed
        form its (T, T) tensors (``P``, ``Wd``, ``Pd``, every head's); the other group is None.  The fused T = 16 kernels keep
        neither (``small``): their backward recomputes the one 16x16 tile."""
        a: _Attn
        x: torch.Tensor
        H: int
        W: int
        hn: torch.Tensor                 # GroupNorm output = the qkv conv's input, and its statistics
        st: torch.Tensor
        qkv: torch.Tensor
        att: torch.Tensor
        row_stats: Optional[torch.Tensor] = None     # fused: per-query (log-sum-exp, rbar)
        P: Optional[torch.Tensor] = None             # composed: softmax, the logits' tangent, the softmax's tangent
        Wd: Optional[torch.Tensor] = None
        Pd: Optional[torch.Tensor] = None
        small: bool = False                          # fused at T = 16: nothing kept

    def _attn_fwd(self, ctx: _Pass, a: _Attn, x, H, W):
        N, Bp, dual = ctx.N, ctx.Bp, ctx.train
        T, C = H * W, a.c
        nh, D = a.nh, a.d                                                # heads, channels per head
        dev = x.device
        s2 = 1.0 / math.sqrt(D)                                          # (ch^-1/4)^2, ch = D   model/unet.py:245-248
        small = _attn_small(a, T)                                        # T = 16: the one-launch kernels, any head count
        supported, forward, _, hd = _attn_kernel(a, False)
        if (small or supported(T, *hd)) and not dual:                    # sampler: nothing to keep, no tangent
            if a.qkv.can_transform_input(N, 1, T):
                qkv, _, _ = a.qkv.forward([x], N, 1, T, Bp, in_affine=self._gn_fold(a.m.norm, x, Bp, T, C))   # GN folded in
            else:
                hn, _ = self._gn(ctx, a.m.norm, x, T, C, False)
                qkv, _, _ = a.qkv.forward([hn], N, 1, T, Bp)
            if small:
                att = ops.attention_small_forward(qkv, torch.empty(N * T * C, device=dev), N, T, nh, D, s2)
            else:
                att = forward(qkv, torch.empty(N * T * C, device=dev), N, T, *hd, s2)
            out, _, _ = a.proj.forward([att], N, 1, T, Bp, residual=x, stats=True)    # x + proj(.) in the epilogue (unet.py:232)
            return out
        hn, st = self._gn(ctx, a.m.norm, x, T, C, False)
        qkv, _, _ = a.qkv.forward([hn], N, 1, T, Bp)                     # [N][T][3C]: per head q | k | v channel slices
        if small and dual:
            # training at T = 16: the pair's logits are one MFMA tile; nothing is kept, the backward recomputes the tile
            att = ops.attention_small_dual_forward(qkv, Bp, T, nh, D, s2)
            out, _, _ = a.proj.forward([att], N, 1, T, Bp, residual=x)
            ctx.tape.append(self.AttnRec(a, x, H, W, hn, st, qkv, att, small=True))
            return out
        supported, forward, _, hd = _attn_kernel(a, True)
        if supported(T, *hd) and dual:
            # training: ONE kernel for the six products of the dual forward, nothing of size (T,T) written; the
            # backward recomputes the logits from q, k and the per-query (log-sum-exp, rbar) kept here
            att, stats = forward(qkv, Bp, T, *hd, s2)
            out, _, _ = a.proj.forward([att], N, 1, T, Bp, residual=x)
            ctx.tape.append(self.AttnRec(a, x, H, W, hn, st, qkv, att, row_stats=stats))
            return out
        # composed form, one bmm chain per head: head h reads q | k | v at columns 3Dh, 3Dh + D, 3Dh + 2D (contraction D),
        # keeps its (T,T) tiles at offset h*Bp*T*T of S / Wd / Pd and writes att columns [Dh, D(h+1))
        ld = 3 * C
        half = Bp * T * ld                                               # offset of the tangent rows
        btt = Bp * T * T
        S = torch.empty(nh * btt, device=dev)
        sq, sk, sS = (T * ld, ld, 1), (T * ld, 1, ld), (T * T, T, 1)
        for h in range(nh):
            ops.bmm(qkv, 3 * D * h, qkv, 3 * D * h + D, S, h * btt, T, T, D, Bp, sq, sk, sS, alpha=s2)
        Wd = Pd = None
        if dual:
            Wd, Pd = torch.empty_like(S), torch.empty_like(S)
            for h in range(nh):
                qo, ko = 3 * D * h, 3 * D * h + D
                ops.bmm(qkv, half + qo, qkv, ko, Wd, h * btt, T, T, D, Bp, sq, sk, sS, alpha=s2,     # qdot k^T + q kdot^T
                        pair2=(qkv, qo, qkv, half + ko))
        ops.softmax_dual_forward(S, T, Wd, Pd)                           # S <- P (every head's rows)
        att = torch.empty(N * T * C, device=dev)
        sP, sv, sa = (T * T, T, 1), (T * ld, ld, 1), (T * C, C, 1)
        for h in range(nh):
            vo, ao = 3 * D * h + 2 * D, D * h
            if dual:
                # adot = P vdot + Pdot v and a = P v in ONE pass over P (msgm_bmm_dual)
                offa = Bp * T * C
                ops.bmm(S, h * btt, qkv, half + vo, att, offa + ao, T, D, T, Bp, sP, sv, sa, pair2=(Pd, h * btt, qkv, vo),
                        third=(qkv, vo, att, ao))
            else:
                ops.bmm(S, h * btt, qkv, vo, att, ao, T, D, T, Bp, sP, sv, sa)                       # a = P v
        out, _, _ = a.proj.forward([att], N, 1, T, Bp, residual=x)
        if dual:
            ctx.tape.append(self.AttnRec(a, x, H, W, hn, st, qkv, att, P=S, Wd=Wd, Pd=Pd))
        return out

    # the embedding MLPs (first on the tape): pre = (le, zs, as_) of the log-radius MLP or None, er = rows with an embedding
    EmbRec = NamedTuple("EmbRec", [("e0", torch.Tensor), ("z1", torch.Tensor), ("a1", torch.Tensor), ("emb", torch.Tensor),
                                   ("semb", torch.Tensor), ("pre", Optional[tuple]), ("er", int)])
    # a plain convolution on x: kind "conv" (the input conv), "down" (stride 2) or "up" (nearest x2 folded into the conv)
    ConvRec = NamedTuple("ConvRec", [("kind", str), ("op", ConvOp), ("x", torch.Tensor), ("H", int), ("W", int)])
    # cat([h, skip]) of C + Cs channels in front of a decoder block (model/unet.py:514)
    CatRec = NamedTuple("CatRec", [("C", int), ("Cs", int), ("H", int), ("W", int)])
    # the output GroupNorm + SiLU: input h, statistics, output hf
    FinRec = NamedTuple("FinRec", [("h", torch.Tensor), ("st", torch.Tensor), ("hf", torch.Tensor), ("H", int), ("W", int), ("C", int)])

    def _run(self, img, t, N, Bp, tape, drop, logr=None):
        """img: channels-last [N][H][W][Cin].  Returns channels-last [N][H][W][Cout].
        tape: None for the sampler, a list for the training pass (see _Pass); drop: the pass's dropout stream or None.
        logr: [log r ; rdot/r] (N,) with NormalizeLogRadius conditioning."""
        ctx = _Pass(N, Bp, tape, drop)
        train, sampler = ctx.train, not ctx.train
        x = self._build()
        x["set"].pack()
        # sampler path (no tangent, nothing kept): the 3x3 stride-1 convolutions on 16-multiple images take the Winograd
        # F(2x2,3x3) forward kernel — 2.25x fewer MFMAs, all fp32, 1.13-1.26x the direct kernel with the folded GroupNorm +
        # SiLU staging (tools/bench_wino.py), same fused options and statistics by-product; it differs from the direct form
        # by the rounding of its transforms (2-6e-7 per conv) and every sampler parity test runs through it.
        # r3: the TRAINING pass's 3x3 stride-1 convolutions — forward and dgrad, primal and tangent rows alike — take the
        # Winograd kernel too (the dgrad as a Winograd forward of the cotangent with the flipped, transposed kernels): C4 step
        # 122.5 -> 116.9 ms at B = 256, 19.9 -> 18.6 ms at the 32-row shard.  fp32 throughout; its transforms round about twice
        # as much as the direct kernel (per conv 4-8e-7 against 3-4e-7 vs float64; on the ill-conditioned det_params benchmark
        # the per-sample loss is 2.2x the fp32 oracle's own distance from float64 instead of 1.07x — tests/test_round2_gpu.py;
        # the well-conditioned reference fixture g17 holds its absolute tolerances).
        x["set"].pack_wino(train=train)
        # opt-in experiment (never the default): the sampler's 3x3 convolutions with 32-multiple channel counts
        # in bf16-split arithmetic (six bf16 MFMA products per fp32 product, fp32 accumulate) instead of Winograd
        b6 = sampler and bool(os.environ.get("MSGM_SAMPLER_BF16X3"))
        x["set"].pack_b6(b6)
        core, mc = self.core, self.core.model_channels
        H = W = self.in_space
        e0 = ops.timestep_embedding(t, mc)
        z1, _, _ = x["t0"].forward([e0.view(-1)], Bp, 1, 1, Bp)
        a1 = ops.act_dual_forward(SILU, z1, torch.empty_like(z1), False)
        emb, _, _ = x["t2"].forward([a1], Bp, 1, 1, Bp)
        er, pre = Bp, None
        if core.use_log_norm:
            # emb += scale_embed(timestep_embedding(log r)) — it has a tangent (rows Bp..N-1)        NNUnet.py:101-105
            le = ops.timestep_embedding_dual(logr, Bp, mc) if train else ops.timestep_embedding(logr, mc)
            zs, _, _ = x["s0"].forward([le.view(-1)], N, 1, 1, Bp)
            as_ = ops.act_dual_forward(SILU, zs, torch.empty_like(zs), train)
            es, _, _ = x["s2"].forward([as_], N, 1, 1, Bp)
            pv = es[: emb.numel()]
            ops.lincomb(pv, pv, 1.0, emb, 1.0)
            pre = (le, zs, as_)
            emb, er = es, N
        semb = ops.act_dual_forward(SILU, emb, torch.empty_like(emb), train and er == N and N != Bp)   # emb_layers[0] = SiLU
        ctx.er, ctx.eo = er, x["bank"].forward(semb, er, Bp)     # every ResBlock's emb_layers[1] in ONE launch
        if train:
            tape.append(self.EmbRec(e0, z1, a1, emb, semb, pre, er))

        def run_block(blk, h, C, H, W):
            for kind, o in blk:
                if kind == "res":
                    h = self._res_fwd(ctx, o, [h], H, W)
                    C = o.co
                elif kind == "attn":
                    h = self._attn_fwd(ctx, o, h, H, W)
                else:                                            # "conv", "down", "up"
                    if train:
                        tape.append(self.ConvRec(kind, o, h, H, W))
                    h, H, W = o.forward([h], N, H, W, Bp, wino=sampler and kind != "conv", stats=sampler)
                    C = o.Cout
            return h, C, H, W

        h, C = img, core.in_channels
        hs = []
        for blk in x["in"]:
            h, C, H, W = run_block(blk, h, C, H, W)
            hs.append((h, C))
            if train:
                tape.append(_SAVE_SKIP)
        h, C, H, W = run_block(x["mid"], h, C, H, W)
        # decoder ResBlocks with twins read h and the skip tensor as two sources, through the twin set of this pass's mode
        set2 = x["set2"] if sampler else x["set2t"]
        if set2 is not None:
            set2.pack()
            set2.pack_wino(train=train)
            set2.pack_b6(b6)
        for blk in x["outb"]:
            s, Cs = hs.pop()
            kind0, r0 = blk[0]
            if (set2 is not None and kind0 == "res" and r0.two is not None and r0.two.split == (C, Cs)
                    and (train or r0.two.conv1.can_transform_input(N, H, W))):
                h, C, blk = self._res_fwd(ctx, r0, [h, s], H, W), r0.co, blk[1:]
            else:
                if train:
                    tape.append(self.CatRec(C, Cs, H, W))
                h, C = torch.cat([h.view(N, H * W, C), s.view(N, H * W, Cs)], dim=2).reshape(-1), C + Cs    # model/unet.py:514
            h, C, H, W = run_block(blk, h, C, H, W)
        if sampler and x["fin"].can_transform_input(N, H, W):
            # sampler: the output GroupNorm + SiLU (model/unet.py:442-444) applied by the output conv while it stages its input
            out, _, _ = x["fin"].forward([h], N, H, W, Bp, in_affine=self._gn_fold(core.out[0], h, Bp, H * W, C), in_act=1)
            return out
        hf, stf = self._gn(ctx, core.out[0], h, H * W, C, True)
        if train:
            tape.append(self.FinRec(h, stf, hf, H, W, C))
        out, _, _ = x["fin"].forward([hf], N, H, W, Bp)
        return out

    @torch.no_grad()
    def forward(self, x: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        """x: (B, channels*H*W) flat or (B,channels,H,W); t: (B,) or (B,1) (NNUnet.py:195-245)."""
        self._check_widths()             # refused before any launch
        t = t.reshape(-1).float().contiguous()
        S_, Cc = self.in_space, self.channels
        need_flat = x.dim() == 2
        if need_flat:
            B, d = x.shape
            assert d == Cc * S_ * S_, f"Flat dim {d} != {Cc}*{S_}*{S_}"
            flat, forder, sc_in, sc_out = x.contiguous().float(), self.flatten_order == "F", 1.0 / scale_image, float(scale_image)
        elif x.dim() == 4:
            B = x.shape[0]
            assert x.size(1) == Cc
            flat, forder, sc_in, sc_out = x.contiguous().float().reshape(B, -1), False, 1.0, 1.0
        else:
            raise ValueError(f"Unexpected input shape {tuple(x.shape)}")
        if t.numel() == 1 and B != 1:
            t = t.expand(B).contiguous()
        logr = None
        if self.pre:
            d = flat.shape[1]
            flat, logr = ops.normalize_dual(flat, B, d, False, float(d) ** 0.5)      # NNUnet.py:203-205
        img = ops.flat_to_image(flat, B, Cc, S_, S_, forder, sc_in)
        # train mode with dropout (how the reference driver samples): masks from the net's own stream, which then moves on
        drop = self.dropout_stream(img.device) if self.dropout_active() else None
        out = self._run(img, t, B, B, None, drop, logr=logr)
        if drop is not None:
            drop.advance(1)
        y = ops.image_to_flat(out, B, Cc, S_, S_, forder, sc_out)
        return y if need_flat else y.view(B, Cc, S_, S_)

    # ------------------------------------------------------------------ training
    @torch.no_grad()
    def ssm_grad(self, y, t, v, u, cst, inv_batch, rng: Optional[PhiloxState] = None, *,
                 row_weight: Optional[torch.Tensor] = None):
        """Per-sample SSM loss (B,) in the general form loss_b = adot.u + cst + |a|^2/2 (u, cst from
        ``msgm_ssm_terms``: any SDE family); gradients of sum_b loss_b*inv_batch into .grad.
        With dropout active the masks are drawn from ``rng`` (the caller's training stream, shard base included; the net's
        own stream when None) at its current offset — the forward and the backward use the same masks, primal and tangent
        share them — and the stream is advanced by 1 afterwards.
        ``row_weight`` (B,) float32 on the device: gradients of sum_b w_b loss_b*inv_batch — the weight enters at the loss
        seed, everything after it is linear in the seed; the returned losses stay unweighted."""
        B, d = y.shape
        N = 2 * B
        ops._row_weight(row_weight, B)   # refused before any launch
        self._check_widths()
        S_, Cc = self.in_space, self.channels
        self.flat_parameters()
        for p in self.parameters():
            if p.grad is None:
                self._flatten_parameters()
                break
        x = self._build()
        x["set"].zero_grad_images(bias_grads_zeroed=True)
        if x["set2t"] is not None:
            x["set2t"].zero_grad_images(bias_grads_zeroed=True)
        flat, gflat = self.flat_parameters()
        gflat.zero_()                    # GroupNorm parameter gradients are accumulated with atomics; one memset for all
        forder = self.flatten_order == "F"
        stacked = torch.cat([y.contiguous().float(), v.contiguous().float()], 0)
        logr = None
        if self.pre:
            stacked, logr = ops.normalize_dual(stacked, B, d, True, float(d) ** 0.5)
        img = ops.flat_to_image(stacked, N, Cc, S_, S_, forder, 1.0 / scale_image)
        tape = []
        tt = t.reshape(-1).contiguous().float()
        drop = (rng if rng is not None else self.dropout_stream(y.device)) if self.dropout_active() else None
        out = self._run(img, tt, N, B, tape, drop, logr=logr)
        a_flat = ops.image_to_flat(out, N, Cc, S_, S_, forder, float(scale_image))      # [2B][d]: a | adot
        per, g = ops.ssm_loss(a_flat.view(-1), u, cst, inv_batch, row_weight=row_weight)
        gimg = ops.flat_to_image(g.view(N, d), N, Cc, S_, S_, forder, float(scale_image))   # adjoint of (x5, unflatten)
        with ops.DeferredReduces.on(y.device):           # the ~140 slot reductions of the weight / bias gradients: one launch
            self._backward(tape, gimg, N, B)
        if drop is not None:
            drop.advance(1)                              # after the backward: it regenerates the forward's masks
        x["set"].unpack_grads()
        if x["set2t"] is not None and any(isinstance(rec, self.ResRec) and len(rec.srcs) == 2 for rec in tape):
            x["set2t"].unpack_grads()            # after "set": the twins' images replace the (unused, zero) single-source ones
        return per

    def _gn_bwd(self, gnm, xin, stats, g, Bp, P, C, silu, residual=None, residual2=None, dropout=None):
        return ops.groupnorm_dual_backward(xin, gnm.weight.detach(), gnm.bias.detach(), stats, g, gnm.weight.grad, gnm.bias.grad,
                                           Bp, P, C, gnm.num_groups, silu, residual=residual, residual2=residual2, dropout=dropout)

    def _backward(self, tape, g, N, Bp):
        x = self._x
        e0, z1, a1, emb, semb, pre, er = tape[0]
        dsemb = torch.empty_like(semb)       # written (not accumulated) by the embedding bank's backward after the loop
        deo_all = x["bank"].dout
        dh = g
        pend = []                       # gradients w.r.t. the skip (hs) tensors, in pop order
        todo = tape[1:]                 # consumed from the end

        def skip_cotangent():
            """For a record whose INPUT also went on the skip stack (the marker in front of it on the tape): takes the marker
            and returns the cotangent that comes back through the stack, which the caller fuses into a pass of its own."""
            if todo and todo[-1] is _SAVE_SKIP:
                todo.pop()
                return pend.pop()
            return None

        while todo:
            r = todo.pop()
            if isinstance(r, self.FinRec):
                (dhf,) = x["fin"].backward(dh, [r.hf], N, r.H, r.W, Bp)
                dh = self._gn_bwd(self.core.out[0], r.h, r.st, dhf, Bp, r.H * r.W, r.C, True)
            elif isinstance(r, self.ResRec):
                rb, H, W, P = r.r, r.H, r.W, r.H * r.W
                gn1 = rb.m.in_layers[0]
                (dh3,) = rb.conv2.backward(dh, [r.h3], N, H, W, Bp)
                dh2 = self._gn_bwd(rb.m.out_layers[0], r.h2, r.st2, dh3, Bp, P, rb.co, True, dropout=r.dd)
                (dh1,) = rb.conv1.backward(dh2, [r.h1], N, H, W, Bp, dsamp_bias=deo_all[rb.bank_i], emb_rows=er,
                                           bias_grad_elsewhere=True)
                if len(r.srcs) == 2:                                # decoder ResBlock on (h, skip) without the concatenation
                    (h0, s0), (C0, C1), skip = r.srcs, rb.two.split, rb.two.skip_t
                    dxs = ops.groupnorm_dual_backward2(h0, C0, s0, C1, gn1.weight.detach(), gn1.bias.detach(), r.st1, dh1,
                                                       gn1.weight.grad, gn1.bias.grad, Bp, P, gn1.num_groups, True)
                    pend.append(dxs[1])                             # cotangent of the skip tensor, consumed by the encoder
                else:
                    # identity skip: the `h + x` cotangent is added in the GroupNorm apply pass (no separate axpy); so is the
                    # cotangent that reaches this block's input through the skip stack
                    skip = rb.skip
                    dxs = (self._gn_bwd(gn1, r.srcs[0], r.st1, dh1, Bp, P, rb.ci, True, residual=None if skip is not None else dh,
                                        residual2=skip_cotangent()),)
                if skip is not None:
                    skip.backward(dh, r.srcs, N, H, W, Bp, dsrc=list(dxs), dacc=[True] * len(dxs))
                dh = dxs[0]
            elif isinstance(r, self.AttnRec):
                dh = self._attn_bwd(r, dh, N, Bp)
            elif isinstance(r, self.CatRec):
                gg = dh.view(N, r.H * r.W, r.C + r.Cs)
                pend.append(gg[:, :, r.C:].contiguous().view(-1))
                dh = gg[:, :, :r.C].contiguous().view(-1)
            elif r is _SAVE_SKIP:
                # the next encoder block or the middle block starts with a ResBlock or a downsample, which takes the marker
                raise MsgmError("U-Net tape: a skip-stack marker was not consumed by the block behind it")
            elif r.kind == "conv":
                r.op.backward(dh, [r.x], N, r.H, r.W, Bp, need=[False])
                dh = None
            elif r.kind == "down":
                sk = skip_cotangent()                               # the dgrad accumulates onto the skip-stack cotangent
                (dh,) = r.op.backward(dh, [r.x], N, r.H, r.W, Bp, dsrc=[sk], dacc=[sk is not None])
            else:                                                   # "up"
                dh = r.op.backward_ups(dh, r.x, N, r.H, r.W, Bp)
        # emb_layers[1] of every ResBlock: weight / bias gradients (+ the conv1 biases, same gradient) and dsemb, 2 launches
        x["bank"].backward(semb, dsemb, er, Bp)
        # embedding MLPs: Linear -> SiLU -> Linear -> SiLU (shared emb_layers[0])
        if pre is not None:
            le, zs, as_ = pre
            ops.act_dual_backward(SILU, emb, dsemb)                       # (primal | tangent) rows
            ge = dsemb
            (das,) = x["s2"].backward(ge, [as_], N, 1, 1, Bp)
            ops.act_dual_backward(SILU, zs, das)
            x["s0"].backward(das, [le.view(-1)], N, 1, 1, Bp, need=[False])
        else:
            z = torch.zeros_like(emb)
            ge = torch.cat([dsemb, z])
            ops.act_dual_backward(SILU, torch.cat([emb, z]), ge)
        (da1,) = x["t2"].backward(ge[: z1.numel()].contiguous(), [a1], Bp, 1, 1, Bp)
        z1z = torch.zeros_like(z1)
        g1 = torch.cat([da1, z1z])
        ops.act_dual_backward(SILU, torch.cat([z1, z1z]), g1)
        x["t0"].backward(g1[: z1.numel()].contiguous(), [e0.view(-1)], Bp, 1, 1, Bp, need=[False])
        return dh

    def _attn_bwd(self, r: "VorticityUNet.AttnRec", dout, N, Bp):
        a, T = r.a, r.H * r.W
        (datt,) = a.proj.backward(dout, [r.att], N, 1, T, Bp)           # [N][T][C]: abar | adotbar
        if r.small:                                                     # fused dual attention at T = 16
            dqkv = ops.attention_small_dual_backward(r.qkv, datt, Bp, T, a.nh, a.d, 1.0 / math.sqrt(a.d))
        elif r.row_stats is not None:                                   # fused dual attention
            _, _, backward, hd = _attn_kernel(a, True)
            dqkv = backward(r.qkv, r.att, datt, r.row_stats, Bp, T, *hd, 1.0 / math.sqrt(a.d))
        else:
            dqkv = self._attn_bwd_composed(r, datt, N, Bp)
        (dhn,) = a.qkv.backward(dqkv, [r.hn], N, 1, T, Bp)
        return self._gn_bwd(a.m.norm, r.x, r.st, dhn, Bp, T, a.c, False, residual=dout)     # x + proj(.): skip cotangent fused

    def _attn_bwd_composed(self, r: "VorticityUNet.AttnRec", datt, N, Bp):
        """dqkv of the composed form from the kept (T, T) tensors, one bmm chain per head."""
        qkv, Pm, Wd, Pd = r.qkv, r.P, r.Wd, r.Pd
        T, C, nh, D = r.H * r.W, r.a.c, r.a.nh, r.a.d
        s2 = 1.0 / math.sqrt(D)
        ld = 3 * C
        half, offa = Bp * T * ld, Bp * T * C
        dqkv = torch.empty(N * T * ld, device=datt.device)                   # every slice is written exactly once below
        sP, sPt = (T * T, T, 1), (T * T, 1, T)                          # P(t,s) / P^T(s,t)
        sa, sq = (T * C, C, 1), (T * ld, ld, 1)
        btt = Bp * T * T                                                # head h's (T,T) tiles start at h*btt
        hoff = lambda h: (3 * D * h, 3 * D * h + D, 3 * D * h + 2 * D, D * h, h * btt)      # q, k, v, att, P offsets
        # vbar = P^T abar + Pdot^T adotbar ; vdotbar = P^T adotbar
        for h in range(nh):
            qo, ko, vo, ao, po = hoff(h)
            ops.bmm(Pm, po, datt, ao, dqkv, vo, T, D, T, Bp, sPt, sa, sq, pair2=(Pd, po, datt, offa + ao),
                    third=(datt, offa + ao, dqkv, half + vo))            # both from one pass over P^T
        # Pbar = abar v^T + adotbar vdot^T ; Pdotbar = adotbar v^T
        Pb, Pdb = torch.empty_like(Pm), torch.empty_like(Pm)
        svT = (T * ld, 1, ld)                                            # B(k=c, j=s) = v[s][c]
        for h in range(nh):
            qo, ko, vo, ao, po = hoff(h)
            ops.bmm(datt, ao, qkv, vo, Pb, po, T, T, D, Bp, sa, svT, sP, pair2=(datt, offa + ao, qkv, half + vo))
            ops.bmm(datt, offa + ao, qkv, vo, Pdb, po, T, T, D, Bp, sa, svT, sP)
        ops.softmax_dual_backward(Pm, Wd, Pb, Pdb, T)                   # Pb <- Wbar, Pdb <- Wdotbar
        for h in range(nh):
            qo, ko, vo, ao, po = hoff(h)
            # qbar = s2 (Wbar k + Wdotbar kdot) ; qdotbar = s2 Wdotbar k
            ops.bmm(Pdb, po, qkv, half + ko, dqkv, qo, T, D, T, Bp, sP, sq, sq, alpha=s2, pair2=(Pb, po, qkv, ko),
                    third=(qkv, ko, dqkv, half + qo))                    # Wdotbar streamed once for both
            # kbar = s2 (Wbar^T q + Wdotbar^T qdot) ; kdotbar = s2 Wdotbar^T q
            ops.bmm(Pdb, po, qkv, half + qo, dqkv, ko, T, D, T, Bp, sPt, sq, sq, alpha=s2, pair2=(Pb, po, qkv, qo),
                    third=(qkv, qo, dqkv, half + ko))
        return dqkv
