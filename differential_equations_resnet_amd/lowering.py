"""Lowering of a graph Model onto the native executor (asr_net_*).

The pattern recognised is the reference's single-block ResNet as built by
get_single_block_resnet_build_function with one stage of identity blocks
(tfkeras_resnets.py:547-597), which is what every antisymmetric experiment
runs (_v6.ipynb cells 5-9):

    Input -> Lambda* (elementwise affine: identity / x-mean / x/std)
          -> Conv2D k1 x k1 'same' stride 1 (conv1), k1 in {3, 5, 7} -> relu
          -> L x [ conv (Conv2DAntisymmetric3By3 | Conv2DAntisymmetric(k) | Conv2D k x k, k in {3, 5, 7})
                   -> relu -> Lambda(h*x)? -> add(branch, block input) ]
          -> GlobalAveragePooling2D -> Dense(K, softmax)

or, with integrator="rk2" (extension, BASELINE config 5), every block as
the midpoint step built by single_layer_identity_block:

          xm = add(Lambda(h/2*x)?(relu(conv(x))), x);  add(Lambda(h*x)?(relu(conv(xm))), x)

with the SAME conv layer applied twice (3 x 3 blocks only).

All blocks share one kernel size; conv1's is free of it (the reference's
builder passes its kernel_size to conv1 and, with kernel_type='regular', to
every block conv; its antisymmetric blocks are the 3by3 layer).  Blocks of
size 5 / 7 run in float32 at any shape and in bfloat16 at C in {16, 32, 64},
W in {8, 16, 32}; 3 x 3 Euler blocks run in bfloat16 at C in {16, 32, 64, 128,
256} and W == 8 or any multiple of 16 (column-strip kernels from W = 48 on;
at C >= 128 W is streamed from its pack and rounded to nearest), RK2 blocks
at W == 32 and C <= 64 (asr_net_config's accepted set; the executor refuses the rest).

With num_stages > 2 (e.g. the He-style ResNet-32, blocks [10, 10, 10] at
32^2 x 16, 16^2 x 32, 8^2 x 64; tfkeras_resnets.py:575-593) a stage whose
filters or stride change opens with single_layer_conv_block
(tfkeras_resnets.py:204-269):

          add(relu(Conv2D 3x3 'same' stride s (..._branch2)), Conv2D 1x1 'valid' stride s (..._branch1))

and the model lowers onto the multi-stage executor (asr_stages_*, fp32,
Euler blocks) as a StagesPlan.  Multi-stage nets are 3 x 3 only: conv1, blocks
and transitions.

Anything else (BN, pooling, strided stem, convs that are not square 3 / 5 / 7,
per-block differing kernel size/h/gamma/integrator, RK2 blocks in a multi-stage
net or at kernel size 5 / 7) raises AsrUnsupported
naming the layer: there is no fallback executor.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import warnings

import numpy as np

from . import _lib
from .graph import (L2, Activation, Add, Conv2D, Dense, GlobalAveragePooling2D, InputLayer, Lambda, Model,
                    SymbolicTensor)
from .layers._antisymmetric import AntisymmetricConvBase

__all__ = ["NetPlan", "StagesPlan", "analyze", "NativeModel"]


@dataclass
class NetPlan:
    H: int
    W: int
    Cin: int
    C: int
    L: int
    num_classes: int
    h: float
    gamma: float
    subtract_mean: float | None
    divide_by_stddev: float | None
    param_kind: int
    antisymmetric: bool
    integrator: str = "euler"
    conv1: Conv2D = None
    blocks: list = field(default_factory=list)
    fc: Dense = None
    kernel_size: int = 3        # the blocks' (asr_net_config.kernel_size)
    conv1_kernel_size: int = 3  # conv1's (asr_net_config.conv1_kernel_size)
    smoothness_regularization: float = 0.0  # the blocks' alpha (single_layer_identity_block)

    def weight_vars(self):
        """Variables in the executor's flat order (Keras get_weights order)."""
        out = [self.conv1.kernel, self.conv1.bias]
        for conv in self.blocks:
            out += conv.weights
        out += [self.fc.kernel, self.fc.bias]
        return out

    def block_theta_sizes(self):
        """Per block: number of theta (kernel) floats, excluding the bias."""
        return [sum(v.value.size for v in conv.weights) - self.C for conv in self.blocks]

    def regularization_segments(self):
        """The asr_reg_segment rows (offset, count, layer_stride, layers, l2, smooth) of this
        model's regularisers over weight_vars(); [] when every coefficient is zero."""
        return _regularization_segments(self, [(None, self.blocks)])


@dataclass
class StagesPlan:
    """A multi-stage single-block ResNet (asr_stages_config): stage 0 holds
    conv1's filters; every later stage may open with a transition."""
    H: int
    W: int
    Cin: int
    num_classes: int
    h: float
    gamma: float
    subtract_mean: float | None
    divide_by_stddev: float | None
    param_kind: int
    antisymmetric: bool
    stages: list                 # [(C, L, stride)], stride 0 = no transition
    transitions: list            # per stage: None or (conv_3x3 '..._branch2', conv_1x1 '..._branch1')
    stage_blocks: list           # per stage: the identity blocks' convs
    integrator: str = "euler"
    conv1: Conv2D = None
    fc: Dense = None
    smoothness_regularization: float = 0.0  # the blocks' alpha (single_layer_identity_block)

    @property
    def blocks(self):
        return [b for bl in self.stage_blocks for b in bl]

    @property
    def L(self):
        return len(self.blocks)

    @property
    def C(self):
        return self.stages[-1][0]

    def stages_bf16_ok(self):
        """Whether the bf16 block kernels take every stage with blocks (C in
        {16, 32, 64, 128, 256}, W == 8 or a multiple of 16; asr_stages_config.dtype)."""
        W = self.W
        for C, L, S in self.stages:
            if S:
                W = (W + S - 1) // S
            if L > 0 and (C not in (16, 32, 64, 128, 256) or not (W == 8 or (W >= 16 and W % 16 == 0))):
                return False
            if C % 8:
                return False
        return True

    def weight_vars(self):
        """Variables in the executor's flat order (asr_stages_config)."""
        out = [self.conv1.kernel, self.conv1.bias]
        for tr, blocks in zip(self.transitions, self.stage_blocks):
            if tr is not None:
                c2, c1 = tr
                out += [c2.kernel, c2.bias, c1.kernel, c1.bias]
            for conv in blocks:
                out += conv.weights
        out += [self.fc.kernel, self.fc.bias]
        return out

    def regularization_segments(self):
        """As NetPlan.regularization_segments; the smoothness penalty joins the identity blocks of
        one stage only, never two stages across a transition."""
        return _regularization_segments(self, list(zip(self.transitions, self.stage_blocks)))


def _l2_coefficient(v) -> float:
    """The l2 coefficient of a variable's regulariser (0.0 without one), as the float32 the ABI carries."""
    r = v.regularizer
    if r is None:
        return 0.0
    if v.name.endswith("/bias"):
        raise _lib.AsrUnsupported(f"{v.name}: a bias_regularizer is not supported (kernel_regularizer=l2(...) is)")
    if not isinstance(r, L2):
        raise _lib.AsrUnsupported(f"{v.name}: regulariser {r!r} is not supported (graph.l2 is)")
    if not (r.l2 >= 0.0 and np.isfinite(r.l2)):
        raise ValueError(f"{v.name}: l2 coefficient {r.l2!r} must be finite and >= 0")
    return float(np.float32(r.l2))


def _regularization_segments(plan, stages):
    """stages: [(transition convs or None, the stage's identity-block convs)] in weight_vars() order.

    A plain variable with l2 > 0 is one segment of one layer.  The identity blocks of a stage lie
    back to back, each [theta variables..., bias], so the thetas of consecutive blocks with equal
    coefficients are ONE strided segment (layers = blocks, layer_stride = n_theta + C): a deep net
    stays far below the table's 256 rows.  With smoothness_regularization = alpha > 0 that segment
    carries smooth = alpha / (2h), and a second one at the same stride covers the biases."""
    pos, off = {}, 0
    for v in plan.weight_vars():
        pos[id(v)] = off
        off += v.value.size
    coef = {id(v): _l2_coefficient(v) for v in plan.weight_vars()}
    alpha = float(plan.smoothness_regularization)
    smooth = float(np.float32(alpha / (2.0 * plan.h))) if alpha > 0.0 else 0.0
    segs = []

    def plain(v):
        if coef[id(v)] > 0.0:
            segs.append((pos[id(v)], v.value.size, v.value.size, 1, coef[id(v)], 0.0))

    def runs(conv):
        """A block's theta variables as (offset in the block, count, l2), neighbours with one l2 merged."""
        out, rel = [], 0
        for v in conv.weights[:-1]:
            if out and out[-1][2] == coef[id(v)]:
                out[-1] = (out[-1][0], out[-1][1] + v.value.size, out[-1][2])
            else:
                out.append((rel, v.value.size, coef[id(v)]))
            rel += v.value.size
        return out, rel, conv.weights[-1].value.size

    plain(plan.conv1.kernel)
    for tr, blocks in stages:
        if tr is not None:
            plain(tr[0].kernel)
            plain(tr[1].kernel)
        groups = []  # consecutive blocks of one layout: [first block, its runs, n_theta, C, count]
        for conv in blocks:
            r, nt, C = runs(conv)
            if groups and groups[-1][1:4] == [r, nt, C]:
                groups[-1][4] += 1
            else:
                groups.append([conv, r, nt, C, 1])
        if smooth > 0.0 and len(groups) > 1:
            raise _unsupported(groups[1][0], "smoothness_regularization needs the identity blocks of a stage to "
                                             "share their l2 coefficients")
        for conv, r, nt, C, n in groups:
            base, sm = pos[id(conv.weights[0])], (smooth if n > 1 else 0.0)
            for rel, count, c in r:
                if c > 0.0 or sm > 0.0:
                    segs.append((base + rel, count, nt + C, n, c, sm))
            if sm > 0.0:
                segs.append((base + nt, C, nt + C, n, 0.0, sm))
    plain(plan.fc.kernel)
    if len(segs) > _lib.ASR_REG_MAX_SEGMENTS:
        raise _lib.AsrUnsupported(f"{len(segs)} regulariser segments (at most {_lib.ASR_REG_MAX_SEGMENTS})")
    return segs


def _transition(t: SymbolicTensor):
    """Match t = add(relu(conv_3x3(x)), conv_1x1(x)) (single_layer_conv_block,
    tfkeras_resnets.py:238-269); return (conv_3x3, conv_1x1, x) or None."""
    if len(t.inbound) != 2:
        return None
    branch, short = t.inbound
    if not (isinstance(short.layer, Conv2D) and short.layer.kernel_size == (1, 1) and _is_relu(branch)
            and isinstance(branch.inbound[0].layer, Conv2D)):
        return None
    c2, c1 = branch.inbound[0].layer, short.layer
    x = short.inbound[0]
    if branch.inbound[0].inbound[0] is not x:
        raise _unsupported(t.layer, "transition branches must read the same tensor")
    if c2.kernel_size != (3, 3) or c2.padding != "same" or not c2.use_bias or c2.activation not in (None, "linear"):
        raise _unsupported(c2, "transition conv must be a 3x3 'same' conv with bias, no activation")
    if c1.padding != "valid" or not c1.use_bias or c1.activation not in (None, "linear"):
        raise _unsupported(c1, "transition shortcut must be a 1x1 'valid' conv with bias")
    if c2.strides != c1.strides or c2.strides[0] != c2.strides[1] or c2.strides[0] not in (1, 2):
        raise _unsupported(c2, f"transition strides {c2.strides} / {c1.strides} (equal, 1 or 2)")
    if c2.dilation_rate != (1, 1) or c1.dilation_rate != (1, 1) or c2.filters != c1.filters:
        raise _unsupported(c2, "transition convs must be undilated with equal filters")
    return c2, c1, x


def _unsupported(layer, why):
    return _lib.AsrUnsupported(f"cannot lower layer {layer.name} ({type(layer).__name__}): {why}")


def _is_relu(t: SymbolicTensor):
    return isinstance(t.layer, Activation) and t.layer.activation == "relu"


def _affine_scalar(layer: Lambda, shape):
    aff = layer.affine(shape[1:])
    if aff is None:
        raise _unsupported(layer, "not an elementwise affine function")
    s, t = aff
    if not (np.all(s == s.flat[0]) and np.all(t == t.flat[0])):
        raise _unsupported(layer, "per-element/per-channel normalisation (the native stem takes scalars)")
    return float(s.flat[0]), float(t.flat[0])


NET_KERNEL_SIZES = (3, 5, 7)


def _conv_same(layer: Conv2D, what) -> int:
    """A square 'same' stride-1 conv with bias of size 3, 5 or 7: its size."""
    ks = tuple(layer.kernel_size)
    if ks[0] != ks[1] or ks[0] not in NET_KERNEL_SIZES or layer.strides != (1, 1) or layer.padding != "same" \
            or not layer.use_bias:
        raise _unsupported(layer, f"{what} must be a square 'same' stride-1 conv with bias of kernel size 3, 5 or 7 "
                                  f"(kernel_size {ks})")
    if layer.dilation_rate != (1, 1):
        raise _unsupported(layer, "dilated conv")
    return int(ks[0])


def _block_kernel_size(conv) -> int:
    if isinstance(conv, AntisymmetricConvBase):
        return int(conv.kernel_size)
    return int(conv.kernel_size[0])


def _euler_step(t: SymbolicTensor):
    """Match t = add(Lambda(h*x)?(relu(conv(inner))), skip); return (conv, h, inner)."""
    if len(t.inbound) != 2:
        raise _unsupported(t.layer, "add of more than two tensors")
    branch, skip = t.inbound
    h = 1.0
    if isinstance(branch.layer, Lambda):
        s, off = _affine_scalar(branch.layer, branch.shape)
        if off != 0.0:
            raise _unsupported(branch.layer, "block scaling must be h*x")
        h = s
        branch = branch.inbound[0]
    if not _is_relu(branch):
        raise _unsupported(branch.layer, "expected relu in the block branch (BN is not supported)")
    conv_t = branch.inbound[0]
    conv = conv_t.layer
    if isinstance(conv, AntisymmetricConvBase):
        if conv.kernel_size not in NET_KERNEL_SIZES or tuple(conv.strides) != (1, 1) or not conv.use_bias:
            raise _unsupported(conv, f"antisymmetric block conv must have kernel size 3, 5 or 7 (kernel_size "
                                     f"{conv.kernel_size}), stride 1 and a bias")
    elif isinstance(conv, Conv2D):
        _conv_same(conv, "regular block conv")
        if conv.activation not in (None, "linear"):
            raise _unsupported(conv, "conv activation inside an identity block")
    else:
        raise _unsupported(conv, "unsupported block conv")
    return conv, h, conv_t.inbound[0]


def analyze(model: Model) -> NetPlan:
    if len(model.inputs) != 1 or len(model.outputs) != 1:
        raise _lib.AsrUnsupported("the native executor runs single-input single-output models")
    t = model.outputs[0]
    # head: Dense(K, softmax) <- GAP
    if not isinstance(t.layer, Dense):
        raise _unsupported(t.layer, "model output must be the Dense 'fc' layer (include_top=True)")
    fc = t.layer
    if fc.activation != "softmax" or not fc.use_bias:
        raise _unsupported(fc, "the head must be Dense(num_classes, activation='softmax') with bias")
    t = t.inbound[0]
    if not isinstance(t.layer, GlobalAveragePooling2D):
        raise _unsupported(t.layer, "expected GlobalAveragePooling2D before fc")
    t = t.inbound[0]
    # identity blocks (and stage transitions), last to first
    blocks, hs, integ = [], [], []
    segs = []  # completed stages, top first: (transition, blocks top first)
    while isinstance(t.layer, Add):
        tr = _transition(t)
        if tr is not None:
            segs.append(((tr[0], tr[1]), blocks))
            blocks = []
            t = tr[2]
            continue
        conv, h, inner = _euler_step(t)
        skip = t.inbound[1]
        if inner is skip:
            integ.append("euler")
        else:
            # RK2: the conv's input is the midpoint xm = x + (h/2) relu(conv(x))
            if not isinstance(inner.layer, Add) or inner.inbound[1] is not skip:
                raise _unsupported(conv, "block branch must start at the block input (or its RK2 midpoint)")
            conv1_, h1, inner1 = _euler_step(inner)
            if conv1_ is not conv or inner1 is not skip:
                raise _unsupported(inner.layer, "RK2 midpoint must apply the block's own conv to the block input")
            if abs(h1 - 0.5 * h) > 1e-12 * max(1.0, abs(h)):
                raise _unsupported(inner.layer, f"RK2 midpoint scale {h1} is not h/2 (h = {h})")
            integ.append("rk2")
        blocks.append(conv)
        hs.append(h)
        t = skip
    segs.append((None, blocks))
    segs.reverse()
    blocks = [b for _, bl in segs for b in reversed(bl)]
    hs.reverse()
    if not blocks:
        raise _lib.AsrUnsupported("no identity blocks found")
    # stem: relu <- conv1 <- Lambda* <- Input
    if _is_relu(t):
        t = t.inbound[0]
        if not isinstance(t.layer, Conv2D) or t.layer.activation not in (None, "linear"):
            raise _unsupported(t.layer, "expected conv1 before the stem relu (BN is not supported)")
    elif not (isinstance(t.layer, Conv2D) and t.layer.activation == "relu"):
        raise _unsupported(t.layer, "expected relu(conv1) before the first block")
    conv1 = t.layer
    k1 = _conv_same(conv1, "conv1")
    t = t.inbound[0]
    scale, shift = 1.0, 0.0
    while isinstance(t.layer, Lambda):
        s, off = _affine_scalar(t.layer, t.shape)
        scale, shift = scale * s, scale * off + shift  # walking backwards: acc o f
        t = t.inbound[0]
    if not isinstance(t.layer, InputLayer):
        raise _unsupported(t.layer, "unsupported stem layer")
    _, H, W, Cin = t.shape
    C = conv1.filters
    if scale == 0.0:
        raise _lib.AsrUnsupported("input normalisation scales by zero")
    # executor: (v - mean) * (1/std) == scale*v + shift
    mean = None if (scale == 1.0 and shift == 0.0) else -shift / scale
    std = None if mean is None else 1.0 / scale
    first = blocks[0]
    kinds = {(type(b), getattr(b, "param_kind", _lib.ASR_PARAM_REGULAR), getattr(b, "antisymmetric", False),
              float(getattr(b, "gamma", 0.0))) for b in blocks}
    if len(kinds) != 1 or len(set(hs)) != 1 or len(set(integ)) != 1:
        raise _lib.AsrUnsupported("all identity blocks must share conv type, gamma, h and integrator")
    alphas = sorted({float(getattr(b, "smoothness_regularization", 0.0)) for b in blocks})
    if len(alphas) != 1:
        raise _lib.AsrUnsupported(f"all identity blocks must share one smoothness_regularization (got {alphas})")
    kb = _block_kernel_size(first)
    for b in blocks:
        if _block_kernel_size(b) != kb:
            raise _unsupported(b, f"all identity blocks must share one kernel size (kernel_size "
                                  f"{_block_kernel_size(b)}, the first block has {kb})")
    if isinstance(first, AntisymmetricConvBase):
        kind, anti, gamma = first.param_kind, bool(first.antisymmetric), float(first.gamma)
    else:
        kind, anti, gamma = _lib.ASR_PARAM_REGULAR, False, 0.0
    if len(segs) > 1:
        for layer, k in [(conv1, k1)] + [(b, kb) for b in blocks[:1]]:
            if k != 3:
                raise _unsupported(layer, f"multi-stage nets run 3x3 convs only (conv1, blocks and transitions; "
                                          f"kernel_size {k})")
        return _stages_plan(segs, int(H), int(W), int(Cin), int(C), fc, float(hs[0]), gamma, mean, std, kind, anti,
                            integ[0], conv1, alphas[0])
    plan = NetPlan(H=int(H), W=int(W), Cin=int(Cin), C=int(C), L=len(blocks), num_classes=fc.units, h=float(hs[0]),
                   gamma=gamma, subtract_mean=mean, divide_by_stddev=std, param_kind=kind, antisymmetric=anti,
                   integrator=integ[0], conv1=conv1, blocks=blocks, fc=fc, kernel_size=kb, conv1_kernel_size=k1,
                   smoothness_regularization=alphas[0])
    if kb != 3 and integ[0] != "euler":
        raise _unsupported(first, f"RK2 blocks need kernel size 3 (kernel_size {kb})")
    for b in blocks:
        if b.weights[-1].shape != (C,):
            raise _unsupported(b, f"block channels must equal conv1 filters ({C})")
    return plan


def _stages_plan(segs, H, W, Cin, C0, fc, h, gamma, mean, std, kind, anti, integrator, conv1, alpha=0.0) -> StagesPlan:
    if integrator != "euler":
        raise _lib.AsrUnsupported("multi-stage nets run Euler identity blocks (integrator='rk2' is single-stage)")
    if len(segs) > _lib.ASR_STAGES_MAX:
        raise _lib.AsrUnsupported(f"{len(segs)} stages (at most {_lib.ASR_STAGES_MAX})")
    stages, transitions, stage_blocks = [], [], []
    Cp = C0
    for s, (tr, bl) in enumerate(segs):
        bl = list(reversed(bl))
        if tr is None:
            C, S = Cp, 0
        else:
            C, S = tr[0].filters, tr[0].strides[0]
        for b in bl:
            if b.weights[-1].shape != (C,):
                raise _unsupported(b, f"block channels must equal the stage's filters ({C})")
        stages.append((C, len(bl), S))
        transitions.append(tr)
        stage_blocks.append(bl)
        Cp = C
    return StagesPlan(H=H, W=W, Cin=Cin, num_classes=fc.units, h=h, gamma=gamma, subtract_mean=mean,
                      divide_by_stddev=std, param_kind=kind, antisymmetric=anti, stages=stages,
                      transitions=transitions, stage_blocks=stage_blocks, integrator=integrator, conv1=conv1, fc=fc,
                      smoothness_regularization=alpha)


class NativeModel:
    """The device state of one Model lowered onto the native executor.

    ONE instance per Model owns the flat fp32 device parameters (Keras
    order), the Adam moments and step (apply_adam) or the Keras optimiser's
    state buffer (apply_optimizer), and every executor built for it,
    keyed by (batch size, activation dtype, input kind) — so a predict() at
    another batch size or dtype reads the trained parameters and a
    set_weights()/load_variables() reaches every executor.  Host-side
    Variables and the device buffer are kept coherent through
    push_weights/pull_weights.  Callers use views (view(batch, dtype)) that
    fix the batch size and dtype of their calls."""

    def __init__(self, model: Model, device=None):
        from . import runtime
        import torch
        self.model = model
        self.plan = analyze(model)
        self.device = device or runtime.require_gpu()
        self._torch = torch
        self._rt = runtime
        self._executors = {}
        self._warned_stages_dtype = False
        self.vars = self.plan.weight_vars()
        self.n_params = int(sum(v.value.size for v in self.vars))
        self.params = torch.empty(self.n_params, dtype=torch.float32, device=self.device)
        self.m = None
        self.v = None
        self.step = 0
        self.opt = None        # the optimizers.Optimizer whose state opt_state holds
        self.opt_state = None  # [slots * n_params] float32, apply_optimizer
        self._reg = None       # runtime.RegTable of plan.regularization_segments(), regularizer()
        self._host_stale = False
        self.push_weights()

    def resolve_dtype(self, dtype):
        """The activation dtype an executor of this model runs in.  None: the
        plan's own (bfloat16 single-stage, float32 multi-stage: the reference's
        precision).  A multi-stage net runs in bfloat16 when asked and every
        stage with blocks is on the bf16 kernels' shapes (stages_bf16_ok);
        otherwise the request is warned about once and mapped to float32, so
        train and predict views share one executor per batch size."""
        if isinstance(self.plan, StagesPlan):
            if dtype in (None, "float32"):
                return "float32"
            if dtype == "bfloat16" and self.plan.stages_bf16_ok():
                return "bfloat16"
            if not self._warned_stages_dtype:
                warnings.warn(f"this multi-stage net runs in float32 on the native executor (dtype={dtype!r} "
                              "requested: bf16 needs C in {16, 32, 64, 128, 256} and W == 8 or W % 16 == 0 at every stage "
                              "with blocks)", stacklevel=3)
                self._warned_stages_dtype = True
            return "float32"
        return "bfloat16" if dtype is None else dtype

    def view(self, batch_size: int, dtype=None) -> "NativeView":
        return NativeView(self, int(batch_size), self.resolve_dtype(dtype))

    def check_status(self):
        """Blocking: synchronise and check every executor built for this model
        (a failed launch raises AsrError)."""
        for ex in self._executors.values():
            ex.check_status()

    # -- weights ---------------------------------------------------------------
    def push_weights(self):
        flat = np.concatenate([v.value.ravel() for v in self.vars]).astype(np.float32)
        self.params.copy_(self._torch.from_numpy(flat))
        self._host_stale = False

    def pull_weights(self):
        if not self._host_stale:
            return
        flat = self.params.detach().cpu().numpy()
        off = 0
        for v in self.vars:
            n = v.value.size
            v.assign(flat[off:off + n].reshape(v.shape))
            off += n
        for layer in self.model.layers:
            layer._weights_changed()
        self._host_stale = False

    def mark_updated(self):
        self._host_stale = True

    # -- execution ---------------------------------------------------------------
    def executor(self, batch_size: int, dtype, input_u8: bool, inference: bool = False):
        """The executor for (batch, dtype, input kind); inference=True gives the
        forward-only one (bounded workspace: x_0 + two activation slots)."""
        dtype = self.resolve_dtype(dtype)
        key = (int(batch_size), dtype, bool(input_u8), bool(inference))
        ex = self._executors.get(key)
        if ex is None and isinstance(self.plan, StagesPlan):
            p = self.plan
            ex = self._rt.StagesExecutor(int(batch_size), p.H, p.W, p.Cin, p.stages, p.num_classes, p.h, p.gamma,
                                         subtract_mean=p.subtract_mean, divide_by_stddev=p.divide_by_stddev,
                                         dtype=dtype, input_u8=input_u8, device=self.device,
                                         param_kind=p.param_kind, antisymmetric=p.antisymmetric, inference=inference)
            if ex.n_params != self.n_params:
                raise _lib.AsrError(f"executor expects {ex.n_params} parameters, model has {self.n_params}")
            self._executors[key] = ex
        if ex is None:
            p = self.plan
            ex = self._rt.NetExecutor(int(batch_size), p.H, p.W, p.Cin, p.C, p.L, p.num_classes, p.h, p.gamma,
                                      subtract_mean=p.subtract_mean, divide_by_stddev=p.divide_by_stddev,
                                      dtype=dtype, input_u8=input_u8, device=self.device,
                                      param_kind=p.param_kind, antisymmetric=p.antisymmetric,
                                      integrator=p.integrator, inference=inference, kernel_size=p.kernel_size,
                                      conv1_kernel_size=p.conv1_kernel_size)
            if ex.n_params != self.n_params:
                raise _lib.AsrError(f"executor expects {ex.n_params} parameters, model has {self.n_params}")
            self._executors[key] = ex
        return ex

    def _images(self, x):
        torch = self._torch
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if x.dtype not in (torch.uint8, torch.float32):
            x = x.float()
        return x.to(self.device, non_blocking=True).contiguous()

    def regularizer(self):
        """The model's regulariser segments on the device (runtime.RegTable; checked, uploaded and
        given their workspace on first use), or None when the model has none: then no call is made
        and a step is the step of a model built without regularisers."""
        if self._reg is None:
            self._reg = self._rt.RegTable(self.plan.regularization_segments(), self.n_params, self.device)
        return self._reg if self._reg.n else None

    def regularize(self, grads=None, grad_scale=1.0, loss=None):
        """grads += dR / grad_scale and loss[0] += R for the model's penalty R (asr_regularize);
        nothing without regularisers."""
        reg = self.regularizer()
        if reg is not None:
            self._rt.regularize(reg, self.params, grads, grad_scale, loss)

    def apply_adam(self, grads, lr, beta1=0.9, beta2=0.999, epsilon=1e-7, grad_scale=1.0):
        torch = self._torch
        if self.m is None:
            self.m = torch.zeros_like(self.params)
            self.v = torch.zeros_like(self.params)
        self.step += 1
        self._rt.adam_update(self.params, grads, self.m, self.v, lr, beta1, beta2, epsilon, self.step, grad_scale)
        self._host_stale = True

    def apply_optimizer(self, opt, grads, lr=None, grad_scale=1.0):
        """One update of the parameters by the optimizers.Optimizer `opt` (one launch,
        asr_optimizer_update).  `lr` replaces opt.lr (a schedule's value; opt.decay still
        applies).  The state buffer belongs to this NativeModel, so every batch-size view
        shares it; it is allocated, zeroed, on first use and again when another optimiser
        object arrives."""
        if self.opt is not opt or self.opt_state is None:
            self.opt_state = self._torch.zeros(opt.slots() * self.n_params, dtype=self._torch.float32,
                                               device=self.device)
            self.opt = opt
        self._rt.optimizer_update(opt.next_config(lr, grad_scale), self.params, grads, self.opt_state)
        opt.iterations += 1
        self._host_stale = True


class NativeView:
    """A NativeModel at a fixed batch size and dtype.  Everything else
    (parameters, Adam state, weight sync) is the shared NativeModel's."""

    _SHARED = ("params", "m", "v", "step", "opt", "opt_state")

    def __init__(self, state: NativeModel, batch_size: int, dtype):
        object.__setattr__(self, "state", state)
        object.__setattr__(self, "batch_size", int(batch_size))
        object.__setattr__(self, "dtype", dtype)

    def __getattr__(self, name):
        return getattr(self.state, name)

    def __setattr__(self, name, value):
        if name in self._SHARED:
            setattr(self.state, name, value)
        else:
            object.__setattr__(self, name, value)

    def matches(self, batch_size, dtype):
        return self.batch_size == int(batch_size) and self.dtype == self.state.resolve_dtype(dtype)

    def executor(self, input_u8: bool, inference: bool = False):
        return self.state.executor(self.batch_size, self.dtype, input_u8, inference)

    def predict(self, x):
        """Softmax outputs [n, K] (numpy) for n images, in batches of
        batch_size (the last batch is zero-padded), on the forward-only
        executor: device memory is one batch of images plus the inference
        workspace, whatever n is (host arrays are copied batch by batch)."""
        torch = self._torch
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if x.dtype not in (torch.uint8, torch.float32):
            x = x.float()
        n = int(x.shape[0])
        ex = self.executor(x.dtype == torch.uint8, inference=True)
        out = np.empty((n, ex.cfg.num_classes), dtype=np.float32)
        B = self.batch_size
        buf = torch.zeros((B,) + tuple(x.shape[1:]), dtype=x.dtype, device=self.device)
        for i in range(0, n, B):
            m = min(B, n - i)
            buf[:m].copy_(x[i:i + m])
            if m < B:
                buf[m:].zero_()
            out[i:i + m] = ex.forward(self.params, buf)[:m].cpu().numpy()
        return out

    def forward_backward(self, images, targets, want_probs=False):
        """(loss, grads, probs): loss [1] and grads [n_params] are views of
        executor buffers, overwritten by the next call."""
        torch = self._torch
        x = self._images(images)
        if isinstance(targets, np.ndarray):
            targets = torch.from_numpy(np.ascontiguousarray(targets, dtype=np.float32))
        targets = targets.to(self.device, non_blocking=True).float().contiguous()
        ex = self.executor(x.dtype == torch.uint8)
        loss, grads = ex.forward_backward(self.params, x, targets, want_probs=want_probs)
        return loss, grads, ex.probs
