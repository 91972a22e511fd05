"""GPU parity of the multi-stage single-block ResNet (asr_stages_*,
asr_transition_*) against the oracle's restatement of
get_single_block_resnet_build_function with num_stages > 2
(tfkeras_resnets.py:547-597) and single_layer_conv_block
(tfkeras_resnets.py:204-269).

Tolerances (fp32, the reference's precision, vs the fp64 oracle on the
same fp32-representable inputs): transition outputs / gradients within
1e-5 of the tensor's max |oracle| value and the relu mask exact (the few
pre-activations within 1e-5 of 0 excepted); network probabilities within
1e-5 relative, loss within 1e-5 relative, every gradient within 1e-4 of
its tensor's max |oracle| value (the single-stage fp32 bar,
test_gpu_network.py).

bf16 nets (asr_stages_config.dtype = ASR_BF16: the identity blocks in bf16,
fp32 accumulation; stem, transitions, head and weight gradients in fp32):
see _assert_bf16_net -- a tight bar against the oracle with the executor's
bf16 storage rounding, and the bf16 network bar against the plain oracle.
"""
import numpy as np
import pytest

from helpers import assert_close, assert_grad_tensors_max, bf16_round, rel_l2, w_bf16_balanced
from oracle import asr_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KINDS = {"3by3": 0, "general": 1, "regular": 2}


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).cuda()


@pytest.mark.parametrize("N,H,W,Ci,Co,S", [(3, 32, 32, 16, 32, 2), (2, 16, 16, 32, 64, 2), (2, 7, 9, 5, 6, 2),
                                           (2, 8, 8, 6, 4, 1), (1, 1, 1, 3, 5, 2)])
def test_transition_vs_oracle(N, H, W, Ci, Co, S):
    from differential_equations_resnet_amd import runtime as rt
    rng = np.random.default_rng(N * 100 + H + Ci)
    x = rng.standard_normal((N, H, W, Ci)).astype(np.float32).astype(np.float64)
    K2 = (rng.standard_normal((3, 3, Ci, Co)) * np.sqrt(2 / (9 * Ci))).astype(np.float32).astype(np.float64)
    K1 = (rng.standard_normal((1, 1, Ci, Co)) * np.sqrt(2 / Ci)).astype(np.float32).astype(np.float64)
    b2 = (rng.standard_normal(Co) * 0.1).astype(np.float32).astype(np.float64)
    b1 = (rng.standard_normal(Co) * 0.1).astype(np.float32).astype(np.float64)
    y_want, z = O.transition_fwd(x, K2, b2, K1, b1, S)
    y, mask = rt.transition_forward(_t(x), _t(K2), _t(b2), _t(K1), _t(b1), S)
    assert tuple(y.shape) == y_want.shape
    assert_close(y.cpu().numpy(), y_want, rtol=0, atol=1e-5 * np.abs(y_want).max(), what="y")
    m = mask.cpu().numpy().astype(bool)
    near = np.abs(z) < 1e-5
    assert np.array_equal(m[~near], (z > 0)[~near])
    dy = rng.standard_normal(y_want.shape).astype(np.float32).astype(np.float64)
    # the oracle backward on the kernel's own mask (ties at 0 decided as the GPU did)
    zz = np.where(m, 1.0, -1.0)
    dx_want, g_want = O.transition_bwd(dy, x, zz, K2, K1, S)
    dx, dp = rt.transition_backward(_t(dy), _t(x), mask, _t(K2), _t(K1), S)
    assert_close(dx.cpu().numpy(), dx_want, rtol=0, atol=1e-5 * np.abs(dx_want).max(), what="dx")
    got = O.unflatten(dp.cpu().numpy().astype(np.float64), [g.shape for g in g_want])
    for name, a, b in zip(("dK2", "db2", "dK1", "db1"), got, g_want):
        assert_close(a, b, rtol=0, atol=1e-5 * max(np.abs(b).max(), 1e-12), what=name)


def _stages_setup(stages, kind="3by3", anti=True, h=0.5, gamma=0.0, N=4, H=32, W=32, seed=0):
    spec = O.StagesSpec(stages=stages, h=h, gamma=gamma, H=H, W=W, kind=kind, antisymmetric=anti)
    rng = np.random.default_rng(seed)
    params = O.stages_init_params(spec, rng, np.float64, bias_std=0.05)
    # a smaller fc kernel keeps the logits O(1) (the deeper stages grow the activations; saturated
    # softmaxes would turn fp32 rounding of the logits into probability errors above the bar)
    params[-2] = params[-2] * 0.05
    params = [p.astype(np.float32).astype(np.float64) for p in params]
    imgs = rng.integers(0, 256, (N, H, W, 3)).astype(np.uint8)
    onehot = np.eye(10)[rng.integers(0, 10, N)]
    return spec, params, imgs, onehot


def _check_net(ex, spec, params, imgs, onehot):
    flat = _t(O.flatten(params))
    assert flat.numel() == ex.n_params == spec.n_params()
    probs_gpu = ex.forward(flat, torch.from_numpy(imgs).cuda()).cpu().numpy()
    probs, cache = O.stages_forward(spec, params, imgs)
    assert_close(probs_gpu, probs, rtol=1e-5, atol=1e-6, what="probs")
    loss, grads = ex.forward_backward(flat, torch.from_numpy(imgs).cuda(), _t(onehot), want_probs=True)
    want_loss = O.net_loss(probs, onehot)
    assert abs(loss.item() - want_loss) <= 1e-5 * abs(want_loss)
    assert_close(ex.probs.cpu().numpy(), probs, rtol=1e-5, atol=1e-6, what="probs (training call)")
    g_want = O.stages_backward(spec, params, cache, onehot)
    g_got = O.unflatten(grads.cpu().numpy().astype(np.float64), [p.shape for p in params])
    for i, (a, b) in enumerate(zip(g_got, g_want)):
        assert_close(a, b, rtol=0, atol=1e-4 * max(np.abs(b).max(), 1e-12), what=f"grad[{i}] {b.shape}")


@pytest.mark.parametrize("stages,kind,anti,gamma", [
    ([(16, 2, 0), (32, 2, 2), (64, 2, 2)], "3by3", True, 0.0),     # He-style ResNet-32 layout, 2 blocks per stage
    ([(16, 2, 0), (32, 2, 2), (64, 2, 2)], "3by3", True, -0.05),
    ([(16, 1, 0), (32, 1, 2), (32, 1, 0), (64, 0, 2)], "regular", False, 0.0),  # no-transition stage, empty stage
    ([(8, 1, 0), (12, 2, 1)], "general", False, 0.0),               # stride-1 transition, generic shapes
])
def test_stages_network_vs_oracle(stages, kind, anti, gamma):
    from differential_equations_resnet_amd.runtime import StagesExecutor
    spec, params, imgs, onehot = _stages_setup(stages, kind, anti, gamma=gamma)
    ex = StagesExecutor(imgs.shape[0], spec.H, spec.W, 3, stages, 10, spec.h, spec.gamma, subtract_mean=127.5,
                        divide_by_stddev=127.5, input_u8=True, param_kind=KINDS[kind], antisymmetric=anti)
    _check_net(ex, spec, params, imgs, onehot)


def _unsaturate(nv):
    """The he_normal-initialised 28-block net's logits reach the hundreds: the
    softmax saturates, Keras' probability clip zeroes every gradient and the
    comparison would be vacuous.  A smaller fc kernel (as _stages_setup)
    keeps the logits O(1)."""
    fc = nv.state.plan.fc.kernel
    fc.assign(fc.value * 1e-3)
    nv.state.push_weights()


def test_resnet32_he_model_lowers_and_matches_oracle():
    """The He-style ResNet-32 as the reference builds it (num_stages=4, blocks
    [10,10,10] at 32^2 x 16, 16^2 x 32, 8^2 x 64, tfkeras_resnets.py:575-593),
    through the drop-in Model API: compile_native -> forward_backward, Adam."""
    from differential_equations_resnet_amd import graph
    from differential_equations_resnet_amd.graph import Input
    from differential_equations_resnet_amd.lowering import StagesPlan
    from differential_equations_resnet_amd.models import tfkeras_resnets as R
    graph.set_seed(3)
    fn = R.get_single_block_resnet_build_function(kernel_type="antisymmetric", h=0.5, num_stages=4,
                                                  blocks_per_stage=[10, 10, 10], filters_per_block=[16, 32, 64],
                                                  strides=[(1, 1), (2, 2), (2, 2)], subtract_mean=127.5,
                                                  divide_by_stddev=127.5, num_classes=10)
    m = fn(Input(shape=(32, 32, 3)))
    nv = m.compile_native(6)
    assert isinstance(nv.state.plan, StagesPlan) and nv.state.plan.stages == [(16, 10, 0), (32, 9, 2), (64, 9, 2)]
    _unsaturate(nv)
    spec = O.StagesSpec(stages=nv.state.plan.stages, h=0.5)
    params = [v.value.astype(np.float64) for v in nv.state.plan.weight_vars()]
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, (6, 32, 32, 3)).astype(np.uint8)
    onehot = np.eye(10)[rng.integers(0, 10, 6)]
    loss, grads, probs = nv.forward_backward(imgs, onehot.astype(np.float32), want_probs=True)
    p_want, cache = O.stages_forward(spec, params, imgs)
    assert_close(probs.cpu().numpy(), p_want, rtol=1e-5, atol=1e-6, what="probs")
    assert abs(loss.item() - O.net_loss(p_want, onehot)) <= 1e-5 * O.net_loss(p_want, onehot)
    g_want = O.stages_backward(spec, params, cache, onehot)
    assert all(np.abs(g).max() > 0 for g in g_want[:2])  # the stem's gradient reaches through all 28 blocks
    g_got = O.unflatten(grads.cpu().numpy().astype(np.float64), [p.shape for p in params])
    for i, (a, b) in enumerate(zip(g_got, g_want)):
        assert_close(a, b, rtol=0, atol=1e-4 * max(np.abs(b).max(), 1e-12), what=f"grad[{i}] {b.shape}")
    # one TF1 Adam step through the native update, then predict() on the inference executor.  The
    # update is checked on the gradients it was given (checked against the oracle above): Adam's first
    # step moves an element by lr * g / (|g| + eps), ill-conditioned where |g| is O(eps), so feeding it
    # the oracle's gradient would test the gradient again at a tolerance it is not held to
    m0 = [p.copy() for p in params]
    nv.apply_adam(grads, 1e-3)
    mm = [np.zeros_like(p) for p in params]
    vv = [np.zeros_like(p) for p in params]
    O.adam_tf1(m0, g_got, mm, vv, 1)
    got = O.unflatten(nv.params.cpu().numpy().astype(np.float64), [p.shape for p in params])
    for a, b in zip(got, m0):
        assert_close(a, b, rtol=0, atol=1e-5 * max(np.abs(b).max(), 1e-12), what="adam")
    pr = nv.predict(imgs)
    p2, _ = O.stages_forward(spec, got, imgs)
    assert_close(pr, p2, rtol=1e-5, atol=1e-6, what="predict after adam")


def test_training_multistage_overfits_one_batch(tmp_path):
    """The reference's Training loop over a multi-stage net (default dtype:
    the multi-stage executor computes in fp32): gradient mean-norm CSV rows
    include the transition-free identity blocks of every stage, and the loss
    of a learnable batch falls."""
    import csv
    from differential_equations_resnet_amd import graph
    from differential_equations_resnet_amd.dataset_utils import ArrayDataset
    from differential_equations_resnet_amd.models import tfkeras_resnets as R
    from differential_equations_resnet_amd.training import AdamOptimizer, Training
    rng = np.random.default_rng(2)
    labels = rng.integers(0, 4, 32)  # learnable: the class sets the image brightness
    feats = np.clip(labels[:, None, None, None] * 60 + 20 + rng.integers(-15, 16, (32, 32, 32, 3)), 0,
                    255).astype(np.uint8)
    ds = ArrayDataset(feats, labels, 32, shuffle=False, num_classes=10)
    graph.set_seed(0)
    build = R.get_single_block_resnet_build_function(h=0.25, num_stages=4, blocks_per_stage=[2, 2, 2],
                                                     filters_per_block=[16, 32, 64],
                                                     strides=[(1, 1), (2, 2), (2, 2)], subtract_mean=127.5,
                                                     divide_by_stddev=127.5, num_classes=10)
    tr = Training(build, "antisymmetric", AdamOptimizer(epsilon=1e-7), train_dataset=ds,
                  summaries_dir=str(tmp_path), summaries_name="run", csv_logger_dir=str(tmp_path),
                  csv_logger_name="gradient_history")
    first = tr.evaluate("train", 1)["mean_loss"]
    norms = tr.train_step(3e-3, with_norms=True)
    assert len(norms) == 1 + 4  # conv1 + the 4 identity blocks (2 + 1 + 1)
    for _ in range(60):
        tr.train_step(3e-3)
    last = tr.evaluate("train", 1)["mean_loss"]
    assert last < 0.5 * first, (first, last)
    tr.train(epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: 1e-3, summaries_frequency=1)
    rows = list(csv.reader(open(tmp_path / "run_gradient_history.csv"), delimiter=" "))
    assert rows[0][3] == "conv1_kernel_gradient_mean_norm" and "res4_1_branch2_kernel_gradient_mean_norm" in rows[0]


def _stage_group_indices(spec):
    """(name, [parameter indices]) per layer: conv1 kernel + bias, each
    transition's four tensors, each block's theta variables + bias, fc
    kernel + bias -- the per-layer groups of the reference's gradient norms
    (training.py:385-409)."""
    out = [("conv1", [0, 1])]
    i = 2
    for si, (C, L, S) in enumerate(spec.stages):
        if S:
            out.append((f"stage{si}/transition", list(range(i, i + 4))))
            i += 4
        nt = len(spec.block_spec(C).theta_shapes())
        for b in range(L):
            out.append((f"stage{si}/block{b}", list(range(i, i + nt + 1))))
            i += nt + 1
    out.append(("fc", [i, i + 1]))
    return out


def _stage_groups(spec, g):
    """(name, flat array) per layer group (_stage_group_indices)."""
    return [(name, np.concatenate([np.ravel(g[j]) for j in idx])) for name, idx in _stage_group_indices(spec)]


def _bf16_net_errors(ex, spec, params, imgs, onehot, rnd=None):
    """(max |probs - oracle|, |loss - oracle| / oracle, {layer: grad rel-L2})
    of the bf16 executor vs the fp64 oracle (rnd: the oracle's bf16 storage
    rounding, O.stages_forward)."""
    flat = _t(O.flatten(params))
    assert flat.numel() == ex.n_params == spec.n_params()
    probs_gpu = ex.forward(flat, torch.from_numpy(imgs).cuda()).cpu().numpy()
    probs, cache = O.stages_forward(spec, params, imgs, rnd=rnd, rnd_w=w_bf16_balanced if rnd else None)
    loss, grads = ex.forward_backward(flat, torch.from_numpy(imgs).cuda(), _t(onehot), want_probs=True)
    assert np.array_equal(ex.probs.cpu().numpy(), probs_gpu)  # the training call's forward is the same kernels
    want_loss = O.net_loss(probs, onehot)
    g_want = O.stages_backward(spec, params, cache, onehot)
    assert np.abs(g_want[0]).max() > 0  # not saturated: the stem's gradient is live
    g_got = O.unflatten(grads.cpu().numpy().astype(np.float64), [p.shape for p in params])
    errs = {name: rel_l2(a, b) for (name, a), (_, b) in zip(_stage_groups(spec, g_got), _stage_groups(spec, g_want))}
    return float(np.abs(probs_gpu - probs).max()), abs(loss.item() - want_loss) / abs(want_loss), errs, g_got, g_want


def _assert_bf16_net(ex, spec, params, imgs, onehot):
    """Two bars.  (1) Against the oracle with the executor's bf16 storage
    rounding (helpers.bf16_round at every stored activation and chain
    gradient, helpers.w_bf16_balanced for the blocks' W): what remains is
    fp32 accumulation order and the bf16 roundings it flips -- probabilities
    within 2e-3, loss within 1e-3
    relative, every layer's gradient within 2e-2 relative L2.
    (2) Against the plain fp64 oracle (the reference's math): probabilities
    within 2e-2, loss within 1e-2 relative, and every layer's gradient within
    max(2e-2, 1.5 x the same layer's deviation of the bf16-storage oracle from
    the plain one) relative L2 -- the SURVEY §8c bar, widened only for a layer
    whose gradient bf16 storage itself moves further (measured: conv1 of the
    two-blocks-per-stage nets, 3.7e-2 in the CPU emulation, a sum over every
    flipped relu of the net: tools/bf16_depth_emulate.py); the He
    ResNet-32 itself meets 2e-2 everywhere (1.2e-2).  Plus per tensor max |err|
    <= 5e-2 x its layer's max |ref| (helpers.assert_grad_tensors_max: a wrong
    tensor that matters to its layer fails even where the layer's relative L2
    dilutes it)."""
    dp, dl, errs, _, g_store = _bf16_net_errors(ex, spec, params, imgs, onehot, rnd=bf16_round)
    print(f"\nbf16-storage oracle: probs {dp:.2e} loss {dl:.2e} worst grad {max(errs.values()):.2e} "
          f"({max(errs, key=errs.get)})")
    assert dp < 2e-3 and dl < 1e-3, (dp, dl)
    bad = {k: v for k, v in errs.items() if not v <= 2e-2}
    assert not bad, bad
    dp, dl, errs, g_got, g_want = _bf16_net_errors(ex, spec, params, imgs, onehot)
    floor = {name: rel_l2(a, b) for (name, a), (_, b) in zip(_stage_groups(spec, g_store), _stage_groups(spec, g_want))}
    worst_t = assert_grad_tensors_max(None, g_got, g_want, 5e-2, report_only=True, groups=_stage_group_indices(spec))
    print(f"fp64 oracle: probs {dp:.2e} loss {dl:.2e} worst grad {max(errs.values()):.2e} ({max(errs, key=errs.get)}; "
          f"bf16-storage floor there {floor[max(errs, key=errs.get)]:.2e}), worst tensor {worst_t[1]:.2e} ({worst_t[0]})")
    assert dp < 2e-2 and dl < 1e-2, (dp, dl)
    bad = {k: (v, floor[k]) for k, v in errs.items() if not v <= max(2e-2, 1.5 * floor[k])}
    assert not bad, bad
    assert_grad_tensors_max(None, g_got, g_want, 5e-2, groups=_stage_group_indices(spec))
    return errs


@pytest.mark.parametrize("stages,kind,anti,gamma", [
    ([(16, 2, 0), (32, 2, 2), (64, 2, 2)], "3by3", True, 0.0),     # He-style ResNet-32 layout, 2 blocks per stage
    ([(16, 2, 0), (32, 2, 2), (64, 2, 2)], "3by3", True, -0.05),
    ([(16, 1, 0), (32, 1, 2), (32, 1, 0), (64, 0, 2)], "regular", False, 0.0),  # no-transition stage, empty stage
    ([(32, 1, 0), (64, 2, 2), (64, 1, 2)], "general", False, 0.0),  # W = 32 / 16 / 8 at C = 64
])
def test_stages_network_bf16_vs_oracle(stages, kind, anti, gamma):
    from differential_equations_resnet_amd.runtime import StagesExecutor
    spec, params, imgs, onehot = _stages_setup(stages, kind, anti, h=0.25, gamma=gamma, N=8)
    ex = StagesExecutor(imgs.shape[0], spec.H, spec.W, 3, stages, 10, spec.h, spec.gamma, subtract_mean=127.5,
                        divide_by_stddev=127.5, input_u8=True, param_kind=KINDS[kind], antisymmetric=anti,
                        dtype="bfloat16")
    _assert_bf16_net(ex, spec, params, imgs, onehot)


def test_stages_network_bf16_odd_batch():
    """An odd batch: the image-resident stage kernels' last workgroup holds one image of two."""
    from differential_equations_resnet_amd.runtime import StagesExecutor
    stages, kind, anti, gamma = [(16, 1, 0), (32, 2, 2), (64, 2, 2)], "3by3", True, 0.0
    spec, params, imgs, onehot = _stages_setup(stages, kind, anti, h=0.25, gamma=gamma, N=5, seed=4)
    ex = StagesExecutor(imgs.shape[0], spec.H, spec.W, 3, stages, 10, spec.h, spec.gamma, subtract_mean=127.5,
                        divide_by_stddev=127.5, input_u8=True, param_kind=KINDS[kind], antisymmetric=anti,
                        dtype="bfloat16")
    _assert_bf16_net(ex, spec, params, imgs, onehot)


STAGES_8x8x32 = [(16, 1, 0), (32, 2, 2)]  # on a 16 x 16 input: 16^2 x 16, then 8^2 x 32


def test_stages_network_bf16_8x8x32():
    """The 8 x 8 x 32 image-resident stage (k_stagef<32, 8> / k_stageb<32, 8>), which no 32 x 32 input
    of the He layout reaches: a 16 x 16 input, an odd batch."""
    from differential_equations_resnet_amd.runtime import StagesExecutor
    spec, params, imgs, onehot = _stages_setup(STAGES_8x8x32, "3by3", True, h=0.25, H=16, W=16, N=5)
    ex = StagesExecutor(imgs.shape[0], spec.H, spec.W, 3, STAGES_8x8x32, 10, spec.h, spec.gamma, subtract_mean=127.5,
                        divide_by_stddev=127.5, input_u8=True, param_kind=KINDS["3by3"], antisymmetric=True,
                        dtype="bfloat16")
    _assert_bf16_net(ex, spec, params, imgs, onehot)


def test_stages_network_fp32_8x8x32():
    """The same stages in fp32 (8 x 8 x 32 is not an fp32 image-resident shape: the per-block kernels)."""
    from differential_equations_resnet_amd.runtime import StagesExecutor
    spec, params, imgs, onehot = _stages_setup(STAGES_8x8x32, "3by3", True, H=16, W=16, N=5)
    ex = StagesExecutor(imgs.shape[0], spec.H, spec.W, 3, STAGES_8x8x32, 10, spec.h, spec.gamma, subtract_mean=127.5,
                        divide_by_stddev=127.5, input_u8=True, param_kind=KINDS["3by3"], antisymmetric=True)
    _check_net(ex, spec, params, imgs, onehot)


def test_stages_bf16_unsupported_width_raises():
    from differential_equations_resnet_amd import _lib
    from differential_equations_resnet_amd.runtime import StagesExecutor
    with pytest.raises(_lib.AsrUnsupported, match="W=4"):  # W = 4 after two stride-2 transitions of a 16x16 input
        StagesExecutor(2, 16, 16, 3, [(16, 1, 0), (32, 1, 2), (64, 1, 2)], 10, 0.5, dtype="bfloat16")


def test_resnet32_he_model_bf16_matches_oracle():
    """The He-style ResNet-32 (tfkeras_resnets.py:575-593, blocks [10,10,10])
    through the drop-in Model API in bf16 (compile_native(dtype="bfloat16")),
    at the bf16 network bar."""
    from differential_equations_resnet_amd import graph
    from differential_equations_resnet_amd.graph import Input
    from differential_equations_resnet_amd.models import tfkeras_resnets as R
    graph.set_seed(3)
    fn = R.get_single_block_resnet_build_function(kernel_type="antisymmetric", h=0.5, num_stages=4,
                                                  blocks_per_stage=[10, 10, 10], filters_per_block=[16, 32, 64],
                                                  strides=[(1, 1), (2, 2), (2, 2)], subtract_mean=127.5,
                                                  divide_by_stddev=127.5, num_classes=10)
    m = fn(Input(shape=(32, 32, 3)))
    nv = m.compile_native(8, dtype="bfloat16")
    assert nv.dtype == "bfloat16"
    _unsaturate(nv)
    spec = O.StagesSpec(stages=nv.state.plan.stages, h=0.5)
    params = [v.value.astype(np.float64) for v in nv.state.plan.weight_vars()]
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, (8, 32, 32, 3)).astype(np.uint8)
    onehot = np.eye(10)[rng.integers(0, 10, 8)]
    ex = nv.state.executor(8, "bfloat16", True)
    assert ex.dtype == "bfloat16"
    errs = _assert_bf16_net(ex, spec, params, imgs, onehot)
    assert max(errs.values()) <= 2e-2, errs  # the He ResNet-32 at the plain SURVEY §8c bar, no floor
    # the Model API's own call runs the same executor
    loss, grads, probs = nv.forward_backward(imgs, onehot.astype(np.float32), want_probs=True)
    p_want, _ = O.stages_forward(spec, params, imgs)
    assert np.abs(probs.cpu().numpy() - p_want).max() < 2e-2


def test_workspace_on_another_device_fails_before_launch():
    """The executors' workspace layout follows the CU count of the device it was
    sized on (the weight-gradient slab rows), so a call whose workspace is not
    device memory of the current device fails with ASR_E_WORKSPACE before any
    launch (check_ws_device).  A pinned host buffer stands in for
    another device's memory on the one-GPU box."""
    import ctypes as ct

    from differential_equations_resnet_amd import _lib
    from differential_equations_resnet_amd.runtime import NetExecutor, StagesExecutor, _p, _stream
    for ex, fn in [(StagesExecutor(2, 32, 32, 3, [(16, 1, 0), (32, 1, 2)], 10, 0.5, dtype="bfloat16"),
                    "asr_stages_forward"),
                   (NetExecutor(2, 32, 32, 3, 16, 2, 10, 0.5, dtype="bfloat16"), "asr_net_forward")]:
        host = torch.empty(ex.ws_bytes, dtype=torch.uint8, pin_memory=True)
        params = torch.zeros(ex.n_params, dtype=torch.float32, device="cuda")
        imgs = torch.zeros(2, 32, 32, 3, dtype=torch.uint8, device="cuda")
        rc = getattr(_lib.load(), fn)(ct.byref(ex.cfg), _p(params), _p(imgs), _p(ex.probs), host.data_ptr(),
                                      ex.ws_bytes, _stream())
        assert rc == _lib.ASR_E_WORKSPACE, (fn, rc)
        assert "current device" in _lib.last_error()
        ex.forward(params, imgs)  # its own workspace still works
        torch.cuda.synchronize()
