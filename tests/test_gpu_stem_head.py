"""GPU parity of the kernels around the blocks -- the stem (k_stem_fwd,
k_stem_wgrad, their MFMA forms, the k_normalize + conv_f32 fallback) and the
head (k_head, k_head_param_grads) -- against the fp64 oracle, at the shapes the
executors accept: L=1 networks (the stem and head dominate) through
runtime.NetExecutor, one multi-stage net through StagesExecutor.

Tolerances: those of tests/test_gpu_network.py.  fp32 -- probabilities rtol
1e-5 + atol 1e-6, loss 1e-5 relative, every gradient tensor within 1e-4 of
its max |oracle| value; bf16 -- probabilities 2e-2 absolute, loss 1 %,
relative L2 <= 2e-2 per gradient group.  Parameters are rounded to fp32
before the oracle sees them; the fc kernel is scaled so the logits stay O(1).

Measured on an MI355X, bf16 at C = 16 / 64, H = 8, relative L2 of the conv1
kernel gradient (the largest of the groups): u8 images, mean 127.5 (v - mean
exact in bf16) 9.4e-3 / 9.5e-3; u8 images, mean 120.3 / std 64 (v - mean
rounded to bf16 by the MFMA stems) 1.4e-2 / 1.7e-2; float images drawn from
[0, 255) (rounded likewise) 1.99e-2 / 1.86e-2, against the bar of 2e-2.
"""
import numpy as np
import pytest

from helpers import assert_close, clip_case, clip_classes, grad_groups, rel_l2
from oracle import asr_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _case(C, Cin=3, K=10, N=3, H=5, W=7, input_u8=True, mean=127.5, std=127.5, seed=0, integrator="euler"):
    spec = O.NetSpec(C=C, L=1, h=0.5, gamma=0.0, num_classes=K, H=H, W=W, Cin=Cin, subtract_mean=mean,
                     divide_by_stddev=std, integrator=integrator)
    rng = np.random.default_rng(seed)
    params = O.init_params(spec, rng, np.float64, bias_std=0.05)
    params[-2] = params[-2] * 0.5
    params[-1] = rng.standard_normal(K) * 0.05
    params = [p.astype(np.float32).astype(np.float64) for p in params]
    if input_u8:
        imgs = rng.integers(0, 256, (N, H, W, Cin)).astype(np.uint8)
    elif mean is None:
        imgs = rng.random((N, H, W, Cin)).astype(np.float32)  # [0, 1), not normalised
    else:
        imgs = (rng.random((N, H, W, Cin)) * 255).astype(np.float32)
    onehot = np.eye(K)[rng.integers(0, K, N)]
    return spec, params, imgs, onehot


def _executor(spec, N, dtype, input_u8):
    from differential_equations_resnet_amd.runtime import NetExecutor
    return NetExecutor(N, spec.H, spec.W, spec.Cin, spec.C, spec.L, spec.num_classes, spec.h, spec.gamma,
                       subtract_mean=spec.subtract_mean, divide_by_stddev=spec.divide_by_stddev, dtype=dtype,
                       input_u8=input_u8, integrator=spec.integrator)


def _run(spec, params, imgs, onehot, dtype):
    ex = _executor(spec, imgs.shape[0], dtype, imgs.dtype == np.uint8)
    flat = torch.from_numpy(O.flatten(params).astype(np.float32)).cuda()
    assert flat.numel() == ex.n_params == spec.n_params()
    x = torch.from_numpy(imgs).cuda()
    probs_fwd = ex.forward(flat, x).cpu().numpy()
    loss, grads = ex.forward_backward(flat, x, torch.from_numpy(onehot.astype(np.float32)).cuda(), want_probs=True)
    ex.check_status()
    g_got = O.unflatten(grads.cpu().numpy().astype(np.float64), [p.shape for p in params])
    return probs_fwd, ex.probs.cpu().numpy(), loss.item(), g_got


def _check_fp32(spec, params, imgs, onehot, probs_too=True, loss_scale=None):
    probs_fwd, probs_tr, loss, g_got = _run(spec, params, imgs, onehot, "float32")
    probs, cache = O.net_forward(spec, params, imgs)
    if probs_too:
        assert_close(probs_fwd, probs, rtol=1e-5, atol=1e-6, what="probs")
        assert_close(probs_tr, probs, rtol=1e-5, atol=1e-6, what="probs (training call)")
    want_loss = O.net_loss(probs, onehot)
    print(f"loss {loss!r} oracle {want_loss!r}")
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss)
    g_want = O.net_backward(spec, params, cache, onehot)
    for i, (a, b) in enumerate(zip(g_got, g_want)):
        print(f"grad[{i}] {b.shape}: max err / max|oracle| = {np.abs(a - b).max() / max(np.abs(b).max(), 1e-300):.3e}")
    for i, (a, b) in enumerate(zip(g_got, g_want)):
        assert_close(a, b, rtol=0, atol=1e-4 * max(np.abs(b).max(), 1e-12), what=f"grad[{i}] {b.shape}")


def _check_bf16(spec, params, imgs, onehot):
    probs_fwd, _, loss, g_got = _run(spec, params, imgs, onehot, "bfloat16")
    probs, cache = O.net_forward(spec, params, imgs)
    want_loss = O.net_loss(probs, onehot)
    g_want = O.net_backward(spec, params, cache, onehot)
    errs = [(name, rel_l2(a, b), float(np.linalg.norm(b)))
            for (name, a), (_, b) in zip(grad_groups(spec, g_got), grad_groups(spec, g_want))]
    print(f"probs max err {np.abs(probs_fwd - probs).max():.3e}  loss rel err {abs(loss - want_loss) / want_loss:.3e}  "
          + "  ".join(f"{n} {e:.3e}" for n, e, _ in errs))
    assert np.abs(probs_fwd - probs).max() < 2e-2
    assert abs(loss - want_loss) <= 1e-2 * abs(want_loss)
    assert all(nb > 0 for _, _, nb in errs)
    bad = [f"{n}: rel-L2 {e:.3e}" for n, e, _ in errs if not e <= 2e-2]
    assert not bad, "; ".join(bad)


# --- fp32 fast stem: k_stem_fwd + k_stem_wgrad --------------------------------------------------------------
# C = 12, 24, 48: C/4 channel groups is no power of two.  Odd images: every image but the first starts off
# a 16-byte boundary (stage_image's scalar path); the first takes the vector path and its nel % EPV tail.
@pytest.mark.parametrize("input_u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("H,W", [(5, 7), (6, 9)])
@pytest.mark.parametrize("Cin", [1, 3])
@pytest.mark.parametrize("C", [4, 8, 12, 24, 48, 64])
def test_fp32_fast_stem(C, Cin, H, W, input_u8):
    _check_fp32(*_case(C, Cin=Cin, H=H, W=W, input_u8=input_u8, seed=C + Cin))


@pytest.mark.parametrize("C", [8, 12])
def test_fp32_fast_stem_unnormalised_float(C):
    _check_fp32(*_case(C, input_u8=False, mean=None, std=None, seed=1))


@pytest.mark.parametrize("C", [8, 24])
def test_fp32_fast_stem_non_half_integer_mean(C):
    _check_fp32(*_case(C, mean=120.3, std=64.0, seed=2))


def test_fp32_fast_stem_more_images_than_slabs():
    """N = 515 > kMaxStemSlabs = 512: three workgroups loop over two images."""
    _check_fp32(*_case(8, N=515, H=4, W=4, seed=3))


# --- fp32 generic stem: k_normalize + conv_f32 + make_dz + wgrad_f32 (Cin = 2 is not stem_supported) --------
@pytest.mark.parametrize("input_u8", [True, False], ids=["u8", "f32"])
def test_fp32_generic_stem(input_u8):
    _check_fp32(*_case(8, Cin=2, input_u8=input_u8, seed=4))


# --- head: k_head + k_head_param_grads ----------------------------------------------------------------------
# K = 200: one image lane in k_head_param_grads; K = 17 and C/VEC = 5, 3 do not divide 256; C = 5: VEC = 1.
@pytest.mark.parametrize("C", [5, 12, 64])
@pytest.mark.parametrize("K", [1, 2, 3, 10, 17, 200, 256])
def test_fp32_head(K, C):
    _check_fp32(*_case(C, K=K, H=4, W=5, seed=K + C))


@pytest.mark.parametrize("N,K,C", [(1, 10, 12), (1, 1, 5), (300, 17, 12), (300, 200, 5)])
def test_fp32_head_batch_sizes(N, K, C):
    """N = 300: the loss reduction strides by 256 and the image lanes of k_head_param_grads wrap."""
    _check_fp32(*_case(C, K=K, N=N, H=4, W=5, seed=N + K))


def test_head_rejects_257_classes():
    from differential_equations_resnet_amd._lib import AsrError
    from differential_equations_resnet_amd.runtime import NetExecutor
    with pytest.raises(AsrError, match="num_classes <= 256"):
        NetExecutor(2, 4, 5, 3, 8, 1, 257, 0.5, dtype="float32")


def test_fp32_head_keras_clip():
    """Images whose true class is clipped from below, from above, and not at
    all (helpers.clip_case); loss and gradients against the oracle's TF clip
    gradient.  The loss is compared relative to the batch mean."""
    spec, params, imgs, onehot = clip_case()
    probs, _ = O.net_forward(spec, params, imgs)
    low, high, unsat, clear = clip_classes(probs, onehot)
    assert clear and low.any() and high.any() and unsat.any()
    _check_fp32(spec, params, imgs, onehot, probs_too=False)


# --- the multi-stage executor: the second caller of stem_wgrad ----------------------------------------------
def test_fp32_stages_stem_C12():
    from differential_equations_resnet_amd.runtime import StagesExecutor
    from test_gpu_stages import KINDS, _check_net, _stages_setup
    stages = [(12, 1, 0), (24, 1, 2)]
    spec, params, imgs, onehot = _stages_setup(stages, N=3, H=7, W=7, seed=6)
    ex = StagesExecutor(3, 7, 7, 3, stages, 10, spec.h, spec.gamma, subtract_mean=127.5, divide_by_stddev=127.5,
                        input_u8=True, param_kind=KINDS["3by3"], antisymmetric=True)
    _check_net(ex, spec, params, imgs, onehot)


# --- bf16 stems, W = 32 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,input_u8,integrator", [
    (16, 8, True, "euler"), (64, 8, True, "euler"), (16, 16, True, "euler"), (64, 16, True, "euler"),  # k_stem_wgrad_mfma: 1, 2 bands
    (16, 8, False, "euler"), (64, 8, False, "euler"),                                                     # ... float images
    (16, 5, True, "euler"), (64, 5, True, "euler"), (16, 11, True, "euler"), (64, 11, True, "euler"),    # MFMA forward, VALU weight gradient
    (32, 8, True, "euler"),                                                                                # VALU stem, bf16 activations
    (16, 8, True, "rk2"),                                                                                  # k_relu_grad_bf16
])
def test_bf16_stem(C, H, input_u8, integrator):
    _check_bf16(*_case(C, H=H, W=32, input_u8=input_u8, seed=C + H, integrator=integrator))


@pytest.mark.parametrize("C", [16, 64])
def test_bf16_stem_non_half_integer_mean(C):
    """v - 120.3 is not exact in bf16 (the MFMA stems stage the image so): the same bars hold."""
    _check_bf16(*_case(C, H=8, W=32, mean=120.3, std=64.0, seed=7))
