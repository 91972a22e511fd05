"""GPU tests of the networks with 5 x 5 and 7 x 7 convs on the native executor (asr_net_config.kernel_size /
conv1_kernel_size), against the fp64 restatement tests/kxk_net_oracle.py.

Bars (tests/test_gpu_network.py's): fp32: probabilities rtol 1e-5 + atol 1e-6, loss 1e-5 relative, every gradient
tensor within 1e-4 of its max (fp32 sums of at most 7*7*64 = 3136 products sit orders of magnitude below); bf16:
probabilities 2e-2 absolute, loss 1 %, relative L2 <= 2e-2 per gradient group (the CPU emulation of these cases
stays at or below 1.2e-2: tests/test_kxk_net_cpu.py).
"""
import numpy as np
import pytest

import kxk_net_oracle as KO
from helpers import assert_close, assert_grad_groups_rel_l2, grad_groups, rel_l2
from oracle import asr_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _executor(spec, N, dtype, u8=True, **kw):
    from differential_equations_resnet_amd.runtime import NetExecutor
    return NetExecutor(N, spec.H, spec.W, spec.Cin, spec.C, spec.L, spec.num_classes, spec.h, spec.gamma,
                       subtract_mean=spec.subtract_mean, divide_by_stddev=spec.divide_by_stddev, dtype=dtype,
                       input_u8=u8, param_kind=spec.param_kind(), antisymmetric=spec.antisymmetric,
                       kernel_size=spec.kb, conv1_kernel_size=spec.k1, **kw)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


# ---- A. fp32 parity ------------------------------------------------------------------------------------------------
# (k1, kb, kind, antisymmetric, C, H, W, N, L, u8 images).  The general kind has one-element theta tensors (the
# centro-symmetric scalars), whose gradient is a difference of two dW entries: those cases stay at small shapes, as
# tests/test_gpu_network.py's, and C = 16 at 8 x 32 goes to the kinds whose tensors have many entries.
FP32_CASES = [
    (5, 5, "general", True, 4, 5, 8, 2, 2, True),
    (7, 7, "general", False, 5, 7, 9, 3, 1, True),
    (5, 7, "regular", False, 6, 6, 6, 2, 2, True),
    (7, 3, "3by3", True, 8, 3, 8, 2, 2, True),       # H < k1
    (3, 5, "general", True, 6, 6, 6, 2, 1, True),
    (3, 5, "regular", False, 16, 8, 32, 2, 1, True),
    (7, 7, "general", True, 6, 3, 8, 1, 1, False),   # H < k, float images, mean 120.3 / std 64
    (5, 5, "regular", False, 16, 8, 32, 3, 2, True),
    (7, 3, "3by3", True, 16, 8, 32, 2, 2, True),     # 3 x 3 blocks on the fp32 matrix-core kernels, 7 x 7 conv1
]


# The per-tensor bar and cancellation.  A one-element theta tensor of the general kind is dW[a] - dW[mirror a], and
# fp32 holds each dW entry to 2^-24 of itself at best.  Where KO.worst_condition (sum |dW| over the tensor's max
# |gradient|) stays at or below 800, 1e-4 of the tensor's max leaves room for two such roundings
# (1e-4 / (800 * 2^-24) = 2.1); beyond about 1700 no fp32 executor can meet the bar.  The inputs are therefore
# chosen, from the fp64 restatement alone, with a condition of at most 800.
MAX_CONDITION = 800.0


def _fp32_case(k1, kb, kind, anti, C, H, W, N, L, u8):
    """(spec, params, images, onehot, probs, cache, gradients) of one case, the last three from the restatement;
    the first seed whose gradients are conditioned (MAX_CONDITION)."""
    gamma = -0.05 if (kind != "regular" and anti) else 0.0
    mean, std = (127.5, 127.5) if u8 else (120.3, 64.0)
    spec = KO.KNetSpec(C=C, L=L, h=0.5, gamma=gamma, H=H, W=W, kind=kind, antisymmetric=anti, k1=k1, kb=kb,
                       subtract_mean=mean, divide_by_stddev=std)
    for seed in range(50):
        rng = np.random.default_rng(1000 * seed + 100 * k1 + 10 * kb + C)
        params = KO.init_params(spec, rng)
        imgs, onehot = KO.make_batch(spec, N, rng, u8)
        probs, cache = KO.net_forward(spec, params, imgs)
        if KO.worst_condition(spec, params, cache, onehot) <= MAX_CONDITION:
            return spec, params, imgs, onehot, probs, cache, KO.net_backward(spec, params, cache, onehot)
    raise AssertionError("no conditioned seed")


@pytest.mark.parametrize("k1,kb,kind,anti,C,H,W,N,L,u8", FP32_CASES)
def test_fp32_parity(k1, kb, kind, anti, C, H, W, N, L, u8):
    spec, params, imgs, onehot, probs, cache, g_want = _fp32_case(k1, kb, kind, anti, C, H, W, N, L, u8)
    flat = _dev(O.flatten(params), torch.float32)
    ex = _executor(spec, N, "float32", u8)
    assert flat.numel() == ex.n_params == spec.n_params()
    got = ex.forward(flat, _dev(imgs)).cpu().numpy()
    assert_close(got, probs, rtol=1e-5, atol=1e-6, what="probs")
    inf = _executor(spec, N, "float32", u8, inference=True)
    assert inf.ws_bytes < ex.ws_bytes
    assert_close(inf.forward(flat, _dev(imgs)).cpu().numpy(), probs, rtol=1e-5, atol=1e-6, what="inference probs")
    loss, grads = ex.forward_backward(flat, _dev(imgs), _dev(onehot, torch.float32), want_probs=True)
    want_loss = KO.net_loss(probs, onehot)
    assert abs(loss.item() - want_loss) <= 1e-5 * abs(want_loss)
    assert_close(ex.probs.cpu().numpy(), probs, rtol=1e-5, atol=1e-6, what="training probs")
    g_got = O.unflatten(grads.cpu().numpy().astype(np.float64), [p.shape for p in params])
    for i, (a, b) in enumerate(zip(g_got, g_want)):
        assert_close(a, b, rtol=0, atol=1e-4 * max(np.abs(b).max(), 1e-12), what=f"grad[{i}] {b.shape}")
    ex.check_status()


# ---- B. bf16 parity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(KO.BF16_CASES)))
def test_bf16_parity(case):
    spec, params, imgs, onehot = KO.bf16_case(case)
    N = imgs.shape[0]
    ex = _executor(spec, N, "bfloat16")
    flat = _dev(O.flatten(params), torch.float32)
    assert flat.numel() == ex.n_params == spec.n_params()
    probs, cache = KO.net_forward(spec, params, imgs)
    got = ex.forward(flat, _dev(imgs)).cpu().numpy()
    loss, grads = ex.forward_backward(flat, _dev(imgs), _dev(onehot, torch.float32))
    g_want = KO.net_backward(spec, params, cache, onehot)
    g_got = O.unflatten(grads.cpu().numpy().astype(np.float64), [p.shape for p in params])
    worst = max((rel_l2(a, b), name) for (name, a), (_, b) in zip(grad_groups(spec, g_got), grad_groups(spec, g_want)))
    want_loss = KO.net_loss(probs, onehot)
    print(f"bf16 case {case} {KO.BF16_CASES[case]}: probs max|d| {np.abs(got - probs).max():.2e}, loss rel "
          f"{abs(loss.item() - want_loss) / want_loss:.2e}, worst group {worst[1]} rel-L2 {worst[0]:.2e}")
    assert np.abs(got - probs).max() < 2e-2
    assert abs(loss.item() - want_loss) <= 1e-2 * abs(want_loss)
    assert_grad_groups_rel_l2(spec, g_got, g_want, 2e-2)
    inf = _executor(spec, N, "bfloat16", inference=True)
    assert np.abs(inf.forward(flat, _dev(imgs)).cpu().numpy() - probs).max() < 2e-2
    ex.check_status()


# ---- C. the k x k stem kernels: matrix-core arm against the generic arm ------------------------------------------------
def _stem_arms(spec, N, u8, seed):
    """Both arms of both stem kernels on one executor (tests/test_gpu_fullsize.py's test_stem_*_matches_fp32_path,
    with its bars).  Forward: probabilities within 1e-3 absolute of the ASR_VARIANT_STEM_FWD_VALU arm (k_normalize +
    the generic fp32 k x k conv).  Weight gradient: against ASR_VARIANT_STEM_WGRAD_VALU (make_dz + the generic fp32
    weight gradient) the loss and every other gradient are bitwise equal, the stem's within 1e-5 of their max for u8
    images (bf16 (v - mean) is exact there) and 1e-3 for float images."""
    from differential_equations_resnet_amd import runtime as rt
    rng = np.random.default_rng(seed)
    params = _dev(O.flatten(KO.init_params(spec, rng)), torch.float32)
    raw, onehot = KO.make_batch(spec, N, rng, u8)
    imgs, tgt = _dev(raw), _dev(onehot, torch.float32)
    ex = _executor(spec, N, "bfloat16", u8)
    p = ex.forward(params, imgs).clone()
    ex.variant = rt.ASR_VARIANT_STEM_FWD_VALU
    p1 = ex.forward(params, imgs).clone()
    ex.variant = 0
    loss, g = ex.forward_backward(params, imgs, tgt)
    loss, g = loss.clone(), g.clone()
    ex.variant = rt.ASR_VARIANT_STEM_WGRAD_VALU
    loss1, g1 = ex.forward_backward(params, imgs, tgt)
    loss1, g1 = loss1.clone(), g1.clone()
    ex.variant = 0
    ex.check_status()
    a, b = p.cpu().numpy(), p1.cpu().numpy()
    assert np.isfinite(a).all() and np.abs(a - b).max() <= 1e-3, np.abs(a - b).max()
    E1 = spec.k1 * spec.k1 * spec.Cin * spec.C + spec.C
    assert torch.equal(loss, loss1)
    assert torch.equal(g[E1:], g1[E1:]), "only the stem gradients may differ"
    st, st1 = g[:E1].cpu().numpy(), g1[:E1].cpu().numpy()
    assert np.isfinite(st).all() and np.abs(st1).max() > 0
    tol = (1e-5 if u8 else 1e-3) * np.abs(st1).max()
    assert np.abs(st - st1).max() <= tol, (np.abs(st - st1).max(), tol)


def _stem_spec(K, C, H, W, kb=None, kind="general", L=1):
    return KO.KNetSpec(C=C, L=L, h=0.25, gamma=-0.05, H=H, W=W, kind=kind, k1=K, kb=K if kb is None else kb)


@pytest.mark.parametrize("W", [8, 16, 32])
@pytest.mark.parametrize("C", [16, 32, 64])
@pytest.mark.parametrize("K", [5, 7])
def test_stem_kxk_matches_generic_arm(K, C, W):
    """Every (K, C, W) of the kernels' set, at H < K, H a band's multiple and an odd H, one and three images."""
    for H, N in ((3, 3), (8, 1), (11, 3)):
        _stem_arms(_stem_spec(K, C, H, W), N, True, 1000 * K + 10 * C + W + H)


@pytest.mark.parametrize("K,C,H,W,N,u8", [(7, 16, 8, 8, 515, True),   # more images than weight-gradient slabs
                                          (5, 32, 8, 16, 3, False), (7, 64, 11, 32, 3, False),  # float images
                                          (5, 16, 40, 32, 2, True)])   # several bands per image, the last partial
def test_stem_kxk_matches_generic_arm_more(K, C, H, W, N, u8):
    _stem_arms(_stem_spec(K, C, H, W), N, u8, 7)


def test_stem_kxk_with_the_stacked_3x3_backward():
    """k1 = 5 over the C = 64 stack: the stem's relu' is fused into the first block's backward (ro0)."""
    _stem_arms(_stem_spec(5, 64, 32, 32, kb=3, kind="3by3", L=2), 8, True, 3)


# ---- D. determinism ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 7])
def test_forward_backward_is_deterministic(K):
    spec = KO.KNetSpec(C=64, L=2, h=0.25, gamma=-0.05, H=16, W=16, kind="general", k1=K, kb=K)
    rng = np.random.default_rng(K)
    params = KO.init_params(spec, rng)
    imgs, onehot = KO.make_batch(spec, 4, rng)
    ex = _executor(spec, 4, "bfloat16")
    flat, x, t = _dev(O.flatten(params), torch.float32), _dev(imgs), _dev(onehot, torch.float32)
    loss, grads = ex.forward_backward(flat, x, t)
    l0, g0 = loss.clone(), grads.clone()
    loss, grads = ex.forward_backward(flat, x, t)
    assert torch.equal(l0, loss) and torch.equal(g0, grads)
    assert torch.isfinite(g0).all() and float(g0.abs().max()) > 0
    ex.check_status()


# ---- E. the model API ------------------------------------------------------------------------------------------------
def _check_model(m, spec, N, hw, seed):
    """predict and compile_native(...).forward_backward of m against the restatement, at the fp32 bars.  seed: of
    the biases and the batch (conditioned as the cases of test_fp32_parity: asserted below)."""
    rng = np.random.default_rng(seed)
    ws = [w if w.ndim > 1 else (rng.standard_normal(w.shape) * 0.05).astype(np.float32) for w in m.get_weights()]
    m.set_weights(ws)
    params = [w.astype(np.float64) for w in m.get_weights()]
    assert [p.shape for p in params] == [tuple(s) for s in spec.param_shapes()]
    imgs = rng.integers(0, 256, (N, hw, hw, 3)).astype(np.uint8)
    onehot = np.eye(10)[rng.integers(0, 10, N)]
    probs, cache = KO.net_forward(spec, params, imgs)
    assert KO.worst_condition(spec, params, cache, onehot) <= MAX_CONDITION
    got = m.predict(imgs, batch_size=N - 1, dtype="float32")  # 2 batches, the last zero-padded
    assert_close(got, probs, rtol=1e-5, atol=1e-6, what="predict")
    nm = m.compile_native(N, "float32")
    loss, grads, _ = nm.forward_backward(imgs, onehot.astype(np.float32))
    want_loss = KO.net_loss(probs, onehot)
    assert abs(loss.item() - want_loss) <= 1e-5 * want_loss
    g_want = KO.net_backward(spec, params, cache, onehot)
    g_got = O.unflatten(grads.cpu().numpy().astype(np.float64), [p.shape for p in params])
    for i, (a, b) in enumerate(zip(g_got, g_want)):
        assert_close(a, b, rtol=0, atol=1e-4 * max(np.abs(b).max(), 1e-12), what=f"grad[{i}]")


def _builder(kernel_type, kernel_size, C, L, h, gamma=0.0):
    from differential_equations_resnet_amd.models import tfkeras_resnets as R
    return R.get_single_block_resnet_build_function(kernel_type=kernel_type, kernel_size=kernel_size, h=h, gamma=gamma,
                                                    num_stages=2, blocks_per_stage=[L], filters_per_block=[C],
                                                    strides=[(1, 1)], subtract_mean=127.5, divide_by_stddev=127.5,
                                                    num_classes=10)


@pytest.mark.parametrize("kernel_type", ["antisymmetric", "regular"])
def test_builder_model_with_kernel_size_5(kernel_type):
    from differential_equations_resnet_amd import graph
    anti = kernel_type == "antisymmetric"
    graph.set_seed(4)
    m = _builder(kernel_type, 5, 16, 2, 0.5, -0.05 if anti else 0.0)(graph.Input(shape=(32, 32, 3)))
    spec = KO.KNetSpec(C=16, L=2, h=0.5, gamma=-0.05 if anti else 0.0, kind="3by3" if anti else "regular",
                       antisymmetric=anti, k1=5, kb=3 if anti else 5)
    _check_model(m, spec, 5, 32, 1)


def test_hand_built_model_with_7x7_antisymmetric_blocks():
    from differential_equations_resnet_amd import graph
    graph.set_seed(5)
    m = KO.hand_built_model([7, 7, 7], C=16, hw=16, h=0.25, gamma=-0.05, normalise=True)
    spec = KO.KNetSpec(C=16, L=2, h=0.25, gamma=-0.05, H=16, W=16, kind="general", k1=7, kb=7)
    _check_model(m, spec, 5, 16, 120)  # (the first conditioned seed of 0..299 for graph seed 5: 614)


def test_training_bf16_overfits_one_batch_and_round_trips(tmp_path):
    """Training in bfloat16 on a kernel_size=5 model (5 x 5 conv1, 3by3 blocks), as test_training_overfits_one_batch:
    the loss falls below 0.9 of its start within 60 steps; save / load_variables round-trips the weights."""
    from differential_equations_resnet_amd import graph
    from differential_equations_resnet_amd.dataset_utils import ArrayDataset
    from differential_equations_resnet_amd.training import AdamOptimizer, Training
    rng = np.random.default_rng(2)
    labels = rng.integers(0, 4, 32)  # learnable: the class sets the image brightness
    feats = np.clip(labels[:, None, None, None] * 60 + 20 + rng.integers(-15, 16, (32, 32, 32, 3)), 0,
                    255).astype(np.uint8)
    ds = ArrayDataset(feats, labels, 32, shuffle=False, num_classes=10)
    graph.set_seed(0)
    tr = Training(_builder("antisymmetric", 5, 16, 4, 0.25), "antisymmetric", AdamOptimizer(epsilon=1e-7),
                  train_dataset=ds, record_summaries=False)
    assert (tr.native.plan.conv1_kernel_size, tr.native.plan.kernel_size) == (5, 3)
    first = tr.evaluate("train", 1)["mean_loss"]
    for _ in range(60):
        tr.train_step(3e-3)
    last = tr.evaluate("train", 1)["mean_loss"]
    assert last < 0.9 * first, (first, last)
    path = tr.save(str(tmp_path / "ckpt"), "train_saver")
    before = tr.model.get_weights()
    assert before[0].shape == (5, 5, 3, 16)
    tr.train_step(3e-3)
    tr.load_variables(path)
    for a, b in zip(tr.model.get_weights(), before):
        np.testing.assert_array_equal(a, b)
    tr.close()


# ---- F. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    from differential_equations_resnet_amd._lib import AsrUnsupported
    from differential_equations_resnet_amd.runtime import NetExecutor
    kw = dict(param_kind=1, dtype="bfloat16")
    with pytest.raises(AsrUnsupported, match=r"W in \{8, 16, 32\}"):
        NetExecutor(2, 24, 24, 3, 16, 2, 10, 0.25, kernel_size=5, **kw)
    with pytest.raises(AsrUnsupported, match=r"RK2.*\{0 \(= 3\), 3, 5, 7\}"):
        NetExecutor(2, 32, 32, 3, 16, 2, 10, 0.25, kernel_size=5, integrator="rk2", **kw)
    torch.cuda.synchronize()
