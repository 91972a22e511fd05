"""The single-block ResNet with a k1 x k1 conv1 and kb x kb block convs, restated in fp64 numpy from the
oracle's primitives (oracle/asr_oracle.py's NetSpec / net_forward / net_backward are 3 x 3 only):

    x0 = relu(conv_k1((v - mean) / std, K1) + b1);  x_{l+1} = x_l + h relu(conv_kb(x_l, W(theta_l)) + b_l)
    probs = softmax(GAP(x_L) @ Kfc + bfc);  loss = mean Keras categorical cross-entropy

(get_single_block_resnet_build_function with kernel_size = k, tfkeras_resnets.py:547-602; the blocks are
Conv2DAntisymmetric3By3, Conv2DAntisymmetric(kernel_size = kb) or a regular Conv2D.)  At k1 = kb = 3 it equals
O.net_forward / O.net_backward (tests/test_kxk_net_cpu.py); at other sizes it is pinned by finite differences.

`rnd` / `rnd_w` (callables, default identity) emulate bf16 storage: rnd_w rounds every block's W, rnd rounds the
activations after the stem and after every block, and dz and dx in the backward.
"""
import math
from dataclasses import dataclass

import numpy as np

from oracle import asr_oracle as O


@dataclass
class KNetSpec:
    C: int = 16
    L: int = 2
    h: float = 0.25
    gamma: float = 0.0
    num_classes: int = 10
    H: int = 32
    W: int = 32
    Cin: int = 3
    subtract_mean: float | None = 127.5
    divide_by_stddev: float | None = 127.5
    kind: str = "general"        # "3by3" | "general" | "regular"
    antisymmetric: bool = True
    k1: int = 3                  # conv1's kernel size
    kb: int = 3                  # the blocks'

    def theta_shapes(self):
        if self.kind == "3by3":
            assert self.kb == 3
            return O.theta_shapes_3by3(self.C)
        if self.kind == "general":
            return O.theta_shapes_general(self.C, self.kb, self.antisymmetric)[0]
        if self.kind == "regular":
            return [(self.kb, self.kb, self.C, self.C)]
        raise ValueError(self.kind)

    def operator_antisymmetric(self):
        return self.kind == "3by3" or (self.kind == "general" and self.antisymmetric)

    def param_shapes(self):
        s = [(self.k1, self.k1, self.Cin, self.C), (self.C,)]
        for _ in range(self.L):
            s += self.theta_shapes() + [(self.C,)]
        return s + [(self.C, self.num_classes), (self.num_classes,)]

    def n_params(self):
        return int(sum(np.prod(x) for x in self.param_shapes()))

    def n_theta(self):
        return int(sum(np.prod(x) for x in self.theta_shapes()))

    # the executor's names for the same things
    def param_kind(self):
        return {"3by3": 0, "general": 1, "regular": 2}[self.kind]

    def map(self):
        """(src, sign) of W(theta), O.param_map's convention."""
        key = (self.C, self.kind, self.kb, self.antisymmetric)
        if key not in _MAPS:
            n = self.kb * self.kb * self.C * self.C
            _MAPS[key] = ((np.arange(n), np.ones(n, dtype=np.int64)) if self.kind == "regular"
                          else O.param_map(self.C, self.kind, self.kb, self.antisymmetric))
        return _MAPS[key]


_MAPS = {}


def _ident(a):
    return a


def init_params(spec: KNetSpec, rng, bias_std=0.05):
    """he_normal (truncated) kernels, biases bias_std * N(0, 1); every value a float32 number, in fp64."""
    def bias(n):
        return rng.standard_normal(n) * bias_std
    out = [O.truncated_normal(rng, (spec.k1, spec.k1, spec.Cin, spec.C), math.sqrt(2.0 / (spec.k1 ** 2 * spec.Cin))),
           bias(spec.C)]
    std = math.sqrt(2.0 / (spec.kb ** 2 * spec.C))
    for _ in range(spec.L):
        if spec.kind == "3by3":
            out += O.init_theta_3by3(spec.C, rng)
        else:
            out += [O.truncated_normal(rng, sh, std) for sh in spec.theta_shapes()]
        out.append(bias(spec.C))
    out += [O.truncated_normal(rng, (spec.C, spec.num_classes), math.sqrt(2.0 / spec.C)), bias(spec.num_classes)]
    return [np.asarray(p, np.float64).astype(np.float32).astype(np.float64) for p in out]


def split_params(spec: KNetSpec, params):
    nt = len(spec.theta_shapes())
    blocks, i = [], 2
    for _ in range(spec.L):
        blocks.append((params[i:i + nt], params[i + nt]))
        i += nt + 1
    return params[0], params[1], blocks, params[i], params[i + 1]


def block_W(spec: KNetSpec, theta):
    """W [kb, kb, C, C] of one block: the layers' literal assembly where it is cheap, else through the map
    (the two agree: tests/test_oracle.py, tests/test_kxk_net_cpu.py)."""
    if spec.kind == "regular":
        return np.asarray(theta[0])
    if spec.kind == "3by3" and spec.C <= 8:
        return O.assemble_3by3_literal(theta, spec.gamma)
    if spec.kind == "general" and spec.C <= 8:
        return O.assemble_general_literal(theta, spec.C, spec.kb, spec.gamma, spec.antisymmetric)
    src, sign = spec.map()
    return O.assemble_from_map(O.flatten(theta), spec.C, src, sign, spec.gamma, spec.kb)


def normalize(spec: KNetSpec, images):
    x = np.asarray(images).astype(np.float64)
    if spec.subtract_mean is not None:
        x = x - spec.subtract_mean
    if spec.divide_by_stddev is not None:
        x = x / spec.divide_by_stddev
    return x


def net_forward(spec: KNetSpec, params, images, rnd=_ident, rnd_w=_ident):
    conv1_k, conv1_b, blocks, fc_k, fc_b = split_params(spec, params)
    x0 = normalize(spec, images)
    z1 = O.conv2d_same(x0, conv1_k) + conv1_b
    x = rnd(np.maximum(z1, 0))
    xs, zs, Ws = [x], [], []
    for theta, b in blocks:
        W = rnd_w(block_W(spec, theta))
        z = O.conv2d_same(x, W) + np.asarray(b)
        x = rnd(x + spec.h * np.maximum(z, 0))
        xs.append(x)
        zs.append(z)
        Ws.append(W)
    gap = x.mean(axis=(1, 2))
    logits = gap @ fc_k + fc_b
    probs = O.softmax(logits)
    return probs, dict(x0=x0, z1=z1, xs=xs, zs=zs, Ws=Ws, gap=gap, logits=logits, probs=probs)


def net_loss(probs, onehot):
    return float(O.keras_cce(probs, onehot).mean())


def net_backward(spec: KNetSpec, params, cache, onehot, rnd=_ident, dWs=None):
    """Gradients of the mean loss in Keras weight order (param_shapes).  dWs (a list): every block's unprojected
    dW [kb, kb, C, C] is appended to it, first block first."""
    _, _, _, fc_k, _ = split_params(spec, params)
    Nb = onehot.shape[0]
    dlogits = O.keras_cce_grad_logits(cache["probs"], onehot, 1.0 / Nb)
    d_fck = cache["gap"].T @ dlogits
    d_fcb = dlogits.sum(axis=0)
    dgap = dlogits @ fc_k.T
    xL = cache["xs"][-1]
    dx = rnd(np.broadcast_to(dgap[:, None, None, :] / (spec.H * spec.W), xL.shape).copy())
    src, sign = spec.map()
    shapes, ntheta = spec.theta_shapes(), spec.n_theta()
    block_grads = []
    for li in range(spec.L - 1, -1, -1):
        x_in, z, W = cache["xs"][li], cache["zs"][li], cache["Ws"][li]
        dz = rnd(spec.h * (dx * (z > 0)))
        if spec.operator_antisymmetric():  # A^T = -A + 2 gamma I (O.euler_bwd)
            dx = rnd(dx - O.conv2d_same(dz, W) + 2.0 * spec.gamma * dz)
        else:                              # (O.euler_bwd_generic)
            dx = rnd(dx + O.conv2d_backprop_input(dz, W, x_in.shape))
        dW = O.conv2d_backprop_filter(x_in, dz, spec.kb)
        if dWs is not None:
            dWs.insert(0, dW)
        block_grads.append((O.unflatten(O.project_dW(dW, src, sign, ntheta), shapes), dz.sum(axis=(0, 1, 2))))
    block_grads.reverse()
    dz1 = dx * (cache["z1"] > 0)
    grads = [O.conv2d_backprop_filter(cache["x0"], dz1, spec.k1), dz1.sum(axis=(0, 1, 2))]
    for dth, db in block_grads:
        grads += dth + [db]
    return grads + [d_fck, d_fcb]


def worst_condition(spec: KNetSpec, params, cache, onehot):
    """The largest cancellation a block gradient tensor suffers: over every block's theta tensors, (the largest
    sum of |dW| entries that one theta of the tensor is projected from) / (the tensor's max |gradient|).  A
    one-element tensor of the general kind (a centro-symmetric scalar) is dW[a] - dW[mirror a]; where the two
    nearly cancel, a bar relative to the tensor's own max asks for that many more digits of dW than it states."""
    dWs = []
    g = net_backward(spec, params, cache, onehot, dWs=dWs)
    src, sign = spec.map()
    shapes, nt = spec.theta_shapes(), len(spec.theta_shapes())
    worst = 0.0
    for b, dW in enumerate(dWs):
        S = O.unflatten(O.project_dW(np.abs(dW), src, np.abs(sign), spec.n_theta()), shapes)
        for gt, st in zip(g[2 + b * (nt + 1):], S):
            if np.abs(gt).max() > 0:
                worst = max(worst, float(np.abs(st).max() / np.abs(gt).max()))
    return worst


def make_batch(spec: KNetSpec, N, rng, u8=True):
    """(images, onehot): uint8 images, or float32 ones in [0, 255)."""
    if u8:
        imgs = rng.integers(0, 256, (N, spec.H, spec.W, spec.Cin), dtype=np.uint8)
    else:
        imgs = rng.uniform(0.0, 255.0, (N, spec.H, spec.W, spec.Cin)).astype(np.float32)
    return imgs, np.eye(spec.num_classes)[rng.integers(0, spec.num_classes, N)]


# The bf16 parity cases (GPU test B; the CPU emulation keeps each under 0.6 of the 2e-2 bar):
# (k1, kb, kind, antisymmetric, C, H, W, N, L)
BF16_CASES = [
    (5, 5, "general", True, 16, 32, 32, 8, 3),
    (7, 7, "general", True, 16, 32, 32, 8, 3),
    (7, 7, "general", False, 32, 16, 16, 8, 3),
    (5, 5, "regular", False, 16, 32, 32, 8, 3),
    (7, 7, "general", True, 64, 16, 16, 8, 3),
    (7, 5, "general", True, 32, 32, 32, 8, 2),
    (5, 3, "3by3", True, 16, 32, 32, 8, 3),
    (5, 3, "3by3", True, 64, 32, 32, 8, 3),
    (7, 3, "3by3", True, 64, 32, 32, 8, 3),
]


def bf16_case(i, seed=1):
    """(spec, params, images u8, onehot) of BF16_CASES[i]: h = 0.25, gamma = -0.05 for the antisymmetric
    operators, mean / std 127.5."""
    k1, kb, kind, anti, C, H, W, N, L = BF16_CASES[i]
    spec = KNetSpec(C=C, L=L, h=0.25, gamma=-0.05 if (kind != "regular" and anti) else 0.0, H=H, W=W, kind=kind,
                    antisymmetric=anti, k1=k1, kb=kb)
    rng = np.random.default_rng(1000 + 17 * i + seed)
    params = init_params(spec, rng)
    imgs, onehot = make_batch(spec, N, rng)
    return spec, params, imgs, onehot


def hand_built_model(ks, C=16, hw=16, h=0.25, gamma=-0.05, normalise=False):
    """Input -> [x - 127.5 -> x / 127.5] -> conv1 (kernel size ks[0]) -> relu -> one Euler block of
    Conv2DAntisymmetric(kernel_size = k) per further entry of ks -> GAP -> Dense(10, softmax)."""
    from differential_equations_resnet_amd import graph as G
    from differential_equations_resnet_amd.layers import Conv2DAntisymmetric
    inp = G.Input((hw, hw, 3))
    x = inp
    if normalise:
        x = G.Lambda(lambda t: t - 127.5, name="sub_mean")(x)
        x = G.Lambda(lambda t: t / 127.5, name="div_std")(x)
    x = G.Conv2D(filters=C, kernel_size=ks[0], padding="same", name="conv1")(x)
    x = G.Activation("relu")(x)
    for b, k in enumerate(ks[1:]):
        y = G.Activation("relu")(Conv2DAntisymmetric(kernel_size=k, gamma=gamma, name=f"blk{b}")(x))
        y = G.Lambda(lambda t, s=h: s * t, name=f"scale{b}")(y)
        x = G.add([y, x])
    x = G.GlobalAveragePooling2D()(x)
    return G.Model(inp, G.Dense(10, activation="softmax", name="fc")(x))
