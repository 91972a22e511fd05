"""GPU parity of the bf16 3 x 3 Euler block / bare conv at image widths beyond
32 (k_convb / k_wgradb over column strips: W >= 48, W % 16 == 0)
against the numpy oracle, through every layer above them: the conv ABI, the
stack ABI, NetExecutor, StagesExecutor, the Model API and the eager layer.

Bars: test_gpu_kernels.py's bf16 bars, unchanged (the oracle is fed the same
bf16-rounded inputs and W): outputs and dx within 2^-8 |oracle| + 4e-3
max|oracle| per element, the relu mask exact wherever |z| > 2e-2 max|z|, dW,
dtheta and db within 1e-3 of their max|oracle|.  Networks: the bars of
test_gpu_network.py::test_network_bf16_close (probabilities 2e-2, loss 1e-2
relative, 2e-2 relative L2 per gradient group) and, for the staged net,
test_gpu_stages.py::_assert_bf16_net.

Shapes (the smallest at which each failure can show):
  (2, 5, 48, 16)    a full strip plus a 16-wide strip, a partial band
  (1, 9, 64, 32)    two full strips
  (2, 6, 48, 64)    the C = 64 padding / swizzle with a short strip
  (1, 4, 80, 64)    three strips: interior, interior, short
  (40, 32, 128, 16) 40 * 8 bands * 4 strips = 1280 items.  The forward / dgrad grid is at most
                    4 workgroups per CU (1024 on 256 CUs) and the weight gradient's at most
                    kMaxBlockSlabs = 512 (wgrad_strip_grid: min(items / 1 at C = 16, 2 per CU, 512)),
                    so every weight-gradient workgroup owns 2 or 3 items and the forward's
                    workgroups walk several: the prefetch of the next item runs.
"""
import functools

import numpy as np
import pytest

from helpers import assert_close, assert_grad_groups_rel_l2, bf16_round, decode_mask, w_bf16_balanced
from oracle import asr_oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHAPES = [(2, 5, 48, 16), (1, 9, 64, 32), (2, 6, 48, 64), (1, 4, 80, 64), (40, 32, 128, 16)]
GAMMA_H = [(0.0, 0.25), (-0.1, 1.0)]


@pytest.fixture(scope="module")
def rt():
    from differential_equations_resnet_amd import runtime
    runtime.require_gpu()
    return runtime


def _theta(C, seed):
    return O.flatten(O.init_theta_3by3(C, np.random.default_rng(seed), np.float64)).astype(np.float32)


def _oracle_W(th, C, gamma):
    src, sign = O.param_map(C)
    return w_bf16_balanced(O.assemble_from_map(th.astype(np.float64), C, src, sign, gamma), src, sign).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _case(shape, gamma, seam=False):
    """Inputs and the oracle's pre-activation, computed once per (shape, gamma) and left unchanged:
    (x, dy, theta, bias float32; W, z float64).  seam: x zero except columns 31 and 32, dy zero
    except column 47 (what random data could hide at a strip boundary and at the last column)."""
    C = shape[-1]
    rng = np.random.default_rng(abs(hash((shape, gamma))) % 2**32)
    x = rng.standard_normal(shape).astype(np.float32)
    dy = rng.standard_normal(shape).astype(np.float32)
    if seam:
        keep = np.zeros(shape[2], bool)
        keep[[31, 32]] = True
        x[:, :, ~keep, :] = 0
        keep = np.zeros(shape[2], bool)
        keep[47] = True
        dy[:, :, ~keep, :] = 0
    th = _theta(C, 7)
    b = (rng.standard_normal(C) * 0.1).astype(np.float32)
    Wo = _oracle_W(th, C, gamma)
    z = O.conv2d_same(bf16_round(x).astype(np.float64), Wo) + b
    for a in (x, dy, th, b, Wo, z):
        a.setflags(write=False)
    return x, dy, th, b, Wo, z


def _forward(rt, mode, x_np, th, b, C, gamma, h):
    dev = torch.device("cuda")
    pm = rt.param_map(C)
    x = torch.tensor(x_np, device=dev).to(torch.bfloat16).contiguous()  # (torch.tensor copies: the case is read-only)
    w = rt.theta_to_w(torch.tensor(th, device=dev), C, pm, gamma, rt.ASR_BF16)
    N, H, W_, _ = x_np.shape
    mask = torch.zeros(rt.mask_bytes(N, H, W_, C), dtype=torch.uint8, device=dev)
    y = rt.conv_forward(mode, x, w, torch.tensor(b, device=dev), h, mask if mode == rt.ASR_MODE_EULER else None)
    return x, w, y, mask, pm


def _check_forward(rt, shape, mode_name, gamma, h, seam=False):
    N, H, W_, C = shape
    x_np, _, th, b, Wo, z = _case(shape, gamma, seam)
    mode = rt.ASR_MODE_EULER if mode_name == "euler" else rt.ASR_MODE_CONV
    _, _, y, mask, _ = _forward(rt, mode, x_np, th, b, C, gamma, h)
    xo = bf16_round(x_np).astype(np.float64)
    want = xo + h * np.maximum(z, 0) if mode == rt.ASR_MODE_EULER else z
    assert_close(y.float().cpu().numpy(), want, rtol=2 ** -8, atol=4e-3 * np.abs(want).max(), what="bf16 forward")
    if mode == rt.ASR_MODE_EULER:
        m = decode_mask(mask.cpu().numpy(), N, H, W_, C)
        sure = np.abs(z) > 2e-2 * np.abs(z).max()
        assert np.array_equal(m[sure], (z > 0)[sure]), "relu mask mismatch"


def _check_backward(rt, shape, mode_name, gamma, h, seam=False):
    N, H, W_, C = shape
    x_np, dy_np, th, b, Wo, _ = _case(shape, gamma, seam)
    mode = rt.ASR_MODE_EULER if mode_name == "euler" else rt.ASR_MODE_CONV
    x, w, _, mask, pm = _forward(rt, rt.ASR_MODE_EULER, x_np, th, b, C, gamma, h)
    dy = torch.tensor(dy_np, device="cuda").to(torch.bfloat16).contiguous()
    dx, dth, db, dw = rt.conv_backward(mode, dy, x, mask if mode == rt.ASR_MODE_EULER else None, w, pm, h, gamma,
                                       want_dw=True)
    # the oracle, fed the GPU's mask (the mask itself is checked by the forward tests)
    xo = bf16_round(x_np).astype(np.float64)
    dyo = bf16_round(dy_np).astype(np.float64)
    dz_f = h * dyo * decode_mask(mask.cpu().numpy(), N, H, W_, C) if mode == rt.ASR_MODE_EULER else dyo
    dz_q = bf16_round(dz_f).astype(np.float64)
    dx_want = (dyo if mode == rt.ASR_MODE_EULER else 0.0) - O.conv2d_same(dz_q, Wo) + 2 * gamma * dz_q
    dW_want = O.conv2d_backprop_filter(xo, dz_q)
    db_want = dz_f.sum(axis=(0, 1, 2))
    src, sign = O.param_map(C)
    dth_want = O.project_dW(dW_want, src, sign, pm.n_theta)
    assert_close(dx.float().cpu().numpy(), dx_want, rtol=2 ** -8, atol=4e-3 * np.abs(dx_want).max(), what="bf16 dx")
    assert_close(dw.cpu().numpy(), dW_want, rtol=0, atol=1e-3 * np.abs(dW_want).max(), what="dW")
    assert_close(dth.cpu().numpy(), dth_want, rtol=0, atol=1e-3 * np.abs(dth_want).max(), what="dtheta")
    assert_close(db.cpu().numpy(), db_want, rtol=0, atol=1e-3 * np.abs(db_want).max(), what="dbias")
    return dW_want


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode_name", ["euler", "conv"])
@pytest.mark.parametrize("gamma,h", GAMMA_H)
def test_forward_parity(rt, shape, mode_name, gamma, h):
    _check_forward(rt, shape, mode_name, gamma, h)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode_name", ["euler", "conv"])
@pytest.mark.parametrize("gamma,h", GAMMA_H)
def test_backward_parity(rt, shape, mode_name, gamma, h):
    """(40, 32, 128, 16) is the case where every workgroup of the weight-gradient grid owns more than
    one item: 1280 items on a grid of at most 512 (see the module docstring)."""
    _check_backward(rt, shape, mode_name, gamma, h)


@pytest.mark.parametrize("mode_name", ["euler", "conv"])
def test_seam(rt, mode_name):
    """x lives in columns 31 and 32 only (the last column of strip 0 and the first of strip 1: each
    strip's halo column is the other's pixel), dy in column 47 only (the last column of the 16-wide
    strip of a W = 48 image).  x and dz never meet, so the oracle's dW is exactly 0 and the bar
    1e-3 x max|dW| = 0 asks the GPU for exact zeros (the columns past the image contribute nothing)."""
    shape, gamma, h = (2, 5, 48, 16), -0.1, 0.5
    _check_forward(rt, shape, mode_name, gamma, h, seam=True)
    dW_want = _check_backward(rt, shape, mode_name, gamma, h, seam=True)
    assert np.abs(dW_want).max() == 0


def test_stack_abi_equals_single_blocks(rt):
    """asr_block_stack_forward / _backward at a wide shape run the per-block kernels in a loop:
    bitwise the L single-block calls."""
    N, H, W_, C, L, h, gamma = 2, 6, 48, 32, 3, 0.5, -0.05
    rng = np.random.default_rng(3)
    pm = rt.param_map(C)
    stride = pm.n_theta + C
    flat = np.zeros(L * stride, np.float32)
    for l in range(L):
        flat[l * stride:l * stride + pm.n_theta] = _theta(C, 20 + l)
        flat[l * stride + pm.n_theta:(l + 1) * stride] = rng.standard_normal(C) * 0.1
    fl = torch.from_numpy(flat).cuda()
    w = rt.theta_to_w(fl, C, pm, gamma, rt.ASR_BF16, layers=L, theta_stride=stride)
    bias = fl.view(L, stride)[:, pm.n_theta:].contiguous()
    x0 = torch.from_numpy(rng.standard_normal((N, H, W_, C)).astype(np.float32)).cuda().to(torch.bfloat16)
    dyL = torch.from_numpy(rng.standard_normal((N, H, W_, C)).astype(np.float32)).cuda().to(torch.bfloat16)
    ys, masks = rt.block_stack_forward(x0, w, bias, h)
    dx0, dparams = rt.block_stack_backward(dyL, x0, ys, masks, w, pm, h, gamma)
    xs, ms = [x0], []
    for l in range(L):
        m = torch.zeros_like(masks[l])
        xs.append(rt.conv_forward(rt.ASR_MODE_EULER, xs[l], w[l:l + 1], bias[l].contiguous(), h, m))
        ms.append(m)
        assert torch.equal(xs[l + 1], ys[l]) and torch.equal(m, masks[l]), f"layer {l}"
    d = dyL
    for l in range(L - 1, -1, -1):
        d, dth, db, _ = rt.conv_backward(rt.ASR_MODE_EULER, d, xs[l], ms[l], w[l:l + 1], pm, h, gamma)
        assert torch.equal(dparams[l, :pm.n_theta], dth) and torch.equal(dparams[l, pm.n_theta:], db), f"layer {l}"
    assert torch.equal(dx0, d)


def _net_setup(C, L, N, H, W, h=0.25, seed=0):
    spec = O.NetSpec(C=C, L=L, h=h, gamma=0.0, H=H, W=W)
    rng = np.random.default_rng(seed)
    params = [p.astype(np.float32).astype(np.float64) for p in O.init_params(spec, rng, np.float64, bias_std=0.05)]
    imgs = rng.integers(0, 256, (N, H, W, 3)).astype(np.uint8)
    onehot = np.eye(10)[rng.integers(0, 10, N)]
    return spec, params, imgs, onehot


def _net_executor(spec, N, **kw):
    from differential_equations_resnet_amd.runtime import NetExecutor
    return NetExecutor(N, spec.H, spec.W, 3, spec.C, spec.L, spec.num_classes, spec.h, spec.gamma, subtract_mean=127.5,
                       divide_by_stddev=127.5, dtype="bfloat16", input_u8=True, **kw)


@pytest.mark.parametrize("N,H,W,C,L", [(4, 12, 48, 16, 2), (2, 8, 64, 64, 2), (4, 16, 16, 32, 2)])
def test_network_bf16_vs_oracle(N, H, W, C, L):
    """NetExecutor in bf16 off W = 32 (per-block forward and backward, the generic / VALU stem arms):
    test_network_bf16_close's bars against the fp64 oracle."""
    spec, params, imgs, onehot = _net_setup(C, L, N, H, W)
    ex = _net_executor(spec, N)
    flat = torch.from_numpy(O.flatten(params).astype(np.float32)).cuda()
    assert flat.numel() == ex.n_params == spec.n_params()
    probs_gpu = ex.forward(flat, torch.from_numpy(imgs).cuda()).cpu().numpy()
    probs, cache = O.net_forward(spec, params, imgs)
    print(f"\nprobs max err {np.abs(probs_gpu - probs).max():.3e}")
    assert np.abs(probs_gpu - probs).max() < 2e-2
    loss, grads = ex.forward_backward(flat, torch.from_numpy(imgs).cuda(),
                                      torch.from_numpy(onehot.astype(np.float32)).cuda())
    want_loss = O.net_loss(probs, onehot)
    print(f"loss rel err {abs(loss.item() - want_loss) / abs(want_loss):.3e}")
    assert abs(loss.item() - want_loss) <= 1e-2 * abs(want_loss)
    g_want = O.net_backward(spec, params, cache, onehot)
    g_got = O.unflatten(grads.cpu().numpy().astype(np.float64), [p.shape for p in params])
    assert_grad_groups_rel_l2(spec, g_got, g_want, 2e-2)


def test_stages_bf16_wide_vs_oracle():
    """The He layout on a 16 x 64 input: stages at W = 64 (column strips), 32 (deep16 does not take
    H = 16: k_convb) and 16 (k_convb; 4 x 16 is no image-resident shape), the 64 -> 32 transition on the
    fp32 kernels.  The bar is test_gpu_stages.py's _assert_bf16_net, whole: this two-blocks-per-stage
    composition is the one whose conv1 gradient bf16 storage itself moves past 2e-2, so the per-layer
    gradient bar is that function's max(2e-2, 1.5 x the bf16-storage oracle's own deviation), the same
    expression and no new constant."""
    import test_gpu_stages as S
    from differential_equations_resnet_amd.runtime import StagesExecutor
    stages = [(16, 2, 0), (32, 2, 2), (64, 2, 2)]
    spec, params, imgs, onehot = S._stages_setup(stages, "3by3", True, h=0.25, N=8, H=16, W=64)
    ex = StagesExecutor(imgs.shape[0], spec.H, spec.W, 3, stages, 10, spec.h, spec.gamma, subtract_mean=127.5,
                        divide_by_stddev=127.5, input_u8=True, param_kind=0, antisymmetric=True, dtype="bfloat16")
    S._assert_bf16_net(ex, spec, params, imgs, onehot)


def test_inference_forward_is_the_training_forward():
    spec, params, imgs, onehot = _net_setup(16, 2, 4, 12, 48)
    flat = torch.from_numpy(O.flatten(params).astype(np.float32)).cuda()
    x = torch.from_numpy(imgs).cuda()
    ex = _net_executor(spec, 4)
    ex.forward_backward(flat, x, torch.from_numpy(onehot.astype(np.float32)).cuda(), want_probs=True)
    p_train = ex.probs.cpu().numpy().copy()
    p_inf = _net_executor(spec, 4, inference=True).forward(flat, x).cpu().numpy()
    assert np.array_equal(p_inf, p_train)


def test_model_api_trains_in_bf16_at_width_48():
    """A (16, 48, 3) single-stage model through Training in bfloat16: the step's loss is the loss of
    NetExecutor called directly on the same batch and parameters."""
    from differential_equations_resnet_amd import graph
    from differential_equations_resnet_amd.dataset_utils import ArrayDataset
    from differential_equations_resnet_amd.models import tfkeras_resnets as R
    from differential_equations_resnet_amd.training import AdamOptimizer, Training
    rng = np.random.default_rng(4)
    B, C, L, h = 4, 16, 2, 0.25
    feats = rng.integers(0, 256, (B, 16, 48, 3)).astype(np.uint8)
    labels = rng.integers(0, 10, B)
    ds = ArrayDataset(feats, labels, B, shuffle=False, num_classes=10)
    graph.set_seed(2)
    build = R.get_single_block_resnet_build_function(h=h, num_stages=2, blocks_per_stage=[L], filters_per_block=[C],
                                                     strides=[(1, 1)], subtract_mean=127.5, divide_by_stddev=127.5,
                                                     num_classes=10)
    tr = Training(build, "antisymmetric", AdamOptimizer(epsilon=1e-7), train_dataset=ds, record_summaries=False,
                  dtype="bfloat16")
    assert (tr.native.plan.H, tr.native.plan.W) == (16, 48)
    spec = O.NetSpec(C=C, L=L, h=h, H=16, W=48)
    flat = torch.from_numpy(np.concatenate([w.ravel() for w in tr.model.get_weights()]).astype(np.float32)).cuda()
    ex = _net_executor(spec, B)
    assert flat.numel() == ex.n_params
    want, _ = ex.forward_backward(flat, torch.from_numpy(feats).cuda(),
                                  torch.from_numpy(np.eye(10, dtype=np.float32)[labels]).cuda())
    want = want.item()
    tr._reset_metrics()
    tr.train_step(1e-3)
    got, _ = tr._metric_values()
    assert np.isfinite(want) and want > 0
    assert abs(got - want) <= 1e-6 * want, (got, want)  # (the same kernels on the same batch and parameters)
    tr.close()


def test_eager_layer_at_width_48():
    """Conv2DAntisymmetric3By3 called on a (1, 8, 48, 16) bf16 device tensor: the forward bar."""
    from differential_equations_resnet_amd import graph
    from differential_equations_resnet_amd.graph import Input
    from differential_equations_resnet_amd.layers import Conv2DAntisymmetric3By3
    N, H, W_, C = 1, 8, 48, 16
    graph.set_seed(5)
    layer = Conv2DAntisymmetric3By3(gamma=-0.1)
    layer(Input(shape=(H, W_, C)))
    rng = np.random.default_rng(5)
    layer.bias.assign(rng.standard_normal(C) * 0.1)
    x_np = rng.standard_normal((N, H, W_, C)).astype(np.float32)
    y = layer(torch.from_numpy(x_np).cuda().to(torch.bfloat16))
    src = layer.param_map().w_src
    sign, osrc = np.where(src & 1, -1, 1), np.where(src >= 0, src >> 1, -1)
    Wo = w_bf16_balanced(layer.get_kernel().astype(np.float64), osrc, sign).astype(np.float64)
    want = O.conv2d_same(bf16_round(x_np).astype(np.float64), Wo) + layer.bias.value.astype(np.float64)
    assert_close(y.float().detach().cpu().numpy(), want, rtol=2 ** -8, atol=4e-3 * np.abs(want).max(), what="bf16 y")


def test_refusals(rt):
    """Every shape still outside the bf16 set raises AsrUnsupported from the config / argument check,
    before any launch of the library (the executors are refused at construction, the layer calls
    by asr_conv_forward's / asr_rk2_forward's own shape check or in Python)."""
    from differential_equations_resnet_amd._lib import AsrUnsupported
    from differential_equations_resnet_amd.runtime import NetExecutor

    def net(W, **kw):
        return NetExecutor(2, 8, W, 3, 16, 2, 10, 0.5, dtype="bfloat16", **kw)

    for W in (24, 40):
        with pytest.raises(AsrUnsupported, match=f"W={W}"):
            net(W)
        x = torch.zeros(1, 4, W, 16, dtype=torch.bfloat16, device="cuda")
        w = torch.zeros(rt.wpack_elems(16), dtype=torch.bfloat16, device="cuda")
        with pytest.raises(AsrUnsupported, match=f"W={W}"):
            rt.conv_forward(rt.ASR_MODE_CONV, x, w, None)
    with pytest.raises(AsrUnsupported, match="RK2"):
        net(48, integrator="rk2")
    x = torch.zeros(1, 4, 48, 16, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(rt.wpack_elems(16), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(AsrUnsupported, match="W=48"):
        rt.rk2_forward(x, w, None, 0.5)
    with pytest.raises(AsrUnsupported, match="W=48"):
        net(48, kernel_size=5, param_kind=rt.ASR_PARAM_GENERAL)
    with pytest.raises(AsrUnsupported, match="W=48"):
        rt.conv_forward(rt.ASR_MODE_CONV, x, w, None, k=5)
