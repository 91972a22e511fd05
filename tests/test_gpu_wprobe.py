"""The backward of the bf16 3 x 3 conv kernels reads the W that the forward read: one-hot probes.

Black box: nothing here knows the weight pack's layout or its rounding.  In CONV mode with zero bias

    y[n, p, o]  = sum_{t, i} x[n, p + d(t), i] W[t][i][o]        (tap t = 3 ky + kx, d(t) = (ky - 1, kx - 1), SAME)
    dx[n, p, i] = sum_{t, o} dy[n, p - d(t), o] W[t][i][o]       (dx = A^T dy)

so with N = C images, image n one-hot (1.0) in channel n at pixel q,

    y[i, q - d(t), o]   = W[t][i][o]      and, for dy one-hot the same way at pixel q',
    dx[o, q' + d(t), i] = W[t][i][o]

exactly: every sum has one non-zero term, the accumulation is fp32 and a bf16 W entry is a bf16 value.
The two must agree bit for bit at every tap whose position is inside the image on both sides.  (Float
comparison: +0 and -0 compare equal; every other value has one bit pattern.)  An antisymmetric operator's
backward applies -A + 2 gamma I with the forward W in fp32, so gamma must be a bf16 value: 0 and -0.125.
Other operators pass the transposed operator's W (runtime.theta_to_w_transposed) with gamma 0: where
the forward pack is balanced (C <= 64, the general kind with antisymmetric=False) that W must be the
forward pack's mirror, not a second, independently balanced pack.

Euler mode (dx = dy + h A^T (mask dy)): the same probes with an all-ones mask and h = 0.5 give
dx[o, q' + d(t), i] = 0.5 W[t][i][o] exactly, except at each probe's own element (t = 4, i = o), where
1 + h w rounds; that element is left out.

test_probe_algebra (CPU) checks the relations above against the fp64 oracle."""
import numpy as np
import pytest

from oracle import asr_oracle as O

gpu = pytest.mark.gpu

KINDS = {"3by3": (0, True), "general": (1, True), "general_false": (1, False), "regular": (2, False)}
H_EULER = 0.5


def _pixels(where, H, W):
    """(q, q'): the forward's and the backward's probe pixel.  The backward's is the forward's mirror
    image, so that the same taps fall inside the image on both sides: all 9 at the centre, at a corner
    the 4 that do not reach into the padding (the other 5 read it)."""
    q = (H // 2, W // 2) if where == "centre" else (0, 0)
    return q, (H - 1 - q[0], W - 1 - q[1]) if where == "corner" else q


def _onehot(C, H, W, q):
    x = np.zeros((C, H, W, C), np.float32)
    x[np.arange(C), q[0], q[1], np.arange(C)] = 1.0
    return x


def _w_from_y(y, q):
    """W[t][i][o] = y[i, q - d(t), o]; (W [9, C, C], seen [9]: the taps inside the image)"""
    C, H, W, _ = y.shape
    out, seen = np.zeros((9, C, C), y.dtype), np.zeros(9, bool)
    for t in range(9):
        py, px = q[0] - (t // 3 - 1), q[1] - (t % 3 - 1)
        if 0 <= py < H and 0 <= px < W:
            out[t], seen[t] = y[:, py, px, :], True
    return out, seen


def _w_from_dx(dx, q):
    """W[t][i][o] = dx[o, q + d(t), i]"""
    C, H, W, _ = dx.shape
    out, seen = np.zeros((9, C, C), dx.dtype), np.zeros(9, bool)
    for t in range(9):
        py, px = q[0] + (t // 3 - 1), q[1] + (t % 3 - 1)
        if 0 <= py < H and 0 <= px < W:
            out[t], seen[t] = dx[:, py, px, :].T, True
    return out, seen


@pytest.mark.parametrize("where,taps", [("centre", 9), ("corner", 4)])
def test_probe_algebra(where, taps):
    """The probes' reading of y and dx against the oracle's conv and its input gradient (fp64, exact:
    one term per sum), for a W without any symmetry."""
    C, H, W = 4, 3, 8
    Wk = np.random.default_rng(0).standard_normal((3, 3, C, C))
    q, qb = _pixels(where, H, W)
    x = _onehot(C, H, W, q).astype(np.float64)
    dy = _onehot(C, H, W, qb).astype(np.float64)
    wf, sf = _w_from_y(O.conv2d_same(x, Wk), q)
    wb, sb = _w_from_dx(O.conv2d_backprop_input(dy, Wk, x.shape), qb)
    assert np.array_equal(sf, sb) and int(sf.sum()) == taps
    assert np.array_equal(wf[sf], Wk.reshape(9, C, C)[sf]) and np.array_equal(wb[sb], Wk.reshape(9, C, C)[sb])


@pytest.fixture(scope="module")
def rt():
    from differential_equations_resnet_amd import runtime
    runtime.require_gpu()
    return runtime


def _f32(t):
    return t.float().cpu().numpy()


@gpu
@pytest.mark.parametrize("where", ["centre", "corner"])
@pytest.mark.parametrize("HW", [(3, 8), (3, 32)])
@pytest.mark.parametrize("C", [16, 32, 64])
@pytest.mark.parametrize("gamma", [0.0, -0.125])
@pytest.mark.parametrize("kind", list(KINDS))
def test_backward_reads_the_forwards_w(rt, kind, gamma, C, HW, where):
    import torch
    H, W = HW
    k, anti = KINDS[kind]
    pm = rt.param_map(C, k, anti)
    rng = np.random.default_rng(1000 * C + 10 * k + W)
    theta = torch.from_numpy((rng.standard_normal(pm.n_theta) * 0.2).astype(np.float32)).cuda()
    q, qb = _pixels(where, H, W)
    x = torch.from_numpy(_onehot(C, H, W, q)).cuda().to(torch.bfloat16)
    dy = torch.from_numpy(_onehot(C, H, W, qb)).cuda().to(torch.bfloat16)
    bias = torch.zeros(C, device="cuda")
    w = rt.theta_to_w(theta, C, pm, gamma, rt.ASR_BF16)
    y = rt.conv_forward(rt.ASR_MODE_CONV, x, w, bias, 1.0)
    if rt._lib.load().asr_param_is_antisymmetric(k, int(anti)):
        wb, gb = w, gamma  # A^T = -A + 2 gamma I with the forward W
    else:
        wb, gb = rt.theta_to_w_transposed(theta, C, pm, rt.ASR_BF16), 0.0
    dx, *_ = rt.conv_backward(rt.ASR_MODE_CONV, dy, x, None, wb, pm, 1.0, gb, want_dtheta=False, want_dbias=False)
    mask = torch.full((rt.mask_bytes(C, H, W, C),), 0xFF, dtype=torch.uint8, device="cuda")
    dxe, *_ = rt.conv_backward(rt.ASR_MODE_EULER, dy, x, mask, wb, pm, H_EULER, gb, want_dtheta=False,
                               want_dbias=False)
    wf, sf = _w_from_y(_f32(y), q)
    wd, sd = _w_from_dx(_f32(dx), qb)
    we, se = _w_from_dx(_f32(dxe), qb)
    assert np.array_equal(sf, sd) and np.array_equal(sf, se) and sf.sum() == (9 if where == "centre" else 4)
    assert np.abs(wf[sf]).max() > 0.1  # the probes read something
    bad = wd[sf] != wf[sf]
    assert not bad.any(), (f"CONV: the backward read another W than the forward at {int(bad.sum())} of {bad.size} "
                           f"entries (largest difference {np.abs(wd[sf] - wf[sf]).max():.3e})")
    own = np.zeros((9, C, C), bool)
    own[4, np.arange(C), np.arange(C)] = True
    keep = sf[:, None, None] & ~own
    bad = we[keep] != np.float32(H_EULER) * wf[keep]
    assert not bad.any(), f"EULER: the backward read another W than the forward at {int(bad.sum())} of {bad.size} entries"


@gpu
def test_eager_layer_backward_reads_the_forwards_w():
    """Conv2DAntisymmetric(3, antisymmetric=False) in bf16 through torch.autograd: one forward on the
    one-hot x, one backward of the one-hot dy."""
    import torch
    from differential_equations_resnet_amd import graph
    from differential_equations_resnet_amd.graph import Input
    from differential_equations_resnet_amd.layers import Conv2DAntisymmetric
    C, H, W = 32, 3, 32
    graph.set_seed(3)
    layer = Conv2DAntisymmetric(3, antisymmetric=False, use_bias=False)
    layer(Input(shape=(H, W, C)))
    q, qb = _pixels("centre", H, W)
    x = torch.from_numpy(_onehot(C, H, W, q)).cuda().to(torch.bfloat16).requires_grad_(True)
    y = layer(x)
    y.backward(torch.from_numpy(_onehot(C, H, W, qb)).cuda().to(torch.bfloat16))
    wf, sf = _w_from_y(_f32(y.detach()), q)
    wd, sd = _w_from_dx(_f32(x.grad), qb)
    assert sf.all() and sd.all() and np.abs(wf).max() > 0
    bad = wd != wf
    assert not bad.any(), f"the layer's backward read another W than its forward at {int(bad.sum())} of {bad.size} entries"
