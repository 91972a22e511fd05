"""GPU tests of the Keras training surface: the optimiser kernel
(asr_optimizer_update) against an fp64 numpy restatement of the Keras 2.1.6-tf
update rules, and Model.compile / fit / evaluate / train_on_batch /
test_on_batch and Training with the new optimisers against a hand-rolled loop
on a twin model (the existing forward_backward + the fp64 update below).

Tolerances: the optimiser kernel rtol 1e-6 + atol 1e-7 on the parameters and
every state buffer (k_adam's, tests/test_gpu_small_kernels.py); trained weights
1e-5 of each tensor's max and losses 1e-5 relative (tests/test_gpu_distributed.py's
bars for the same kind of comparison); accuracies exact.
"""
import numpy as np
import pytest

from helpers import assert_close
from oracle import asr_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from differential_equations_resnet_amd import _lib, graph, optimizers  # noqa: E402
from differential_equations_resnet_amd.graph import Input  # noqa: E402
from differential_equations_resnet_amd.models import tfkeras_resnets as R  # noqa: E402

SGD, ADAM, RMS = _lib.ASR_OPT_SGD, _lib.ASR_OPT_ADAM, _lib.ASR_OPT_RMSPROP
NESTEROV, AMSGRAD = _lib.ASR_OPT_NESTEROV, _lib.ASR_OPT_AMSGRAD


@pytest.fixture(scope="module")
def rt():
    from differential_equations_resnet_amd import runtime
    runtime.require_gpu()
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _f32(v):
    """The value the ABI's float argument carries: the fp64 reference gets what the kernel gets."""
    return float(np.float32(v))


# --------------------------------------------------------------------------
# the specification, restated in fp64
# --------------------------------------------------------------------------
def ref_update(kind, flags, lr, a, b, eps, t, grad_scale, p, g, state):
    """One update in place on fp64 arrays; state: list of `slots` arrays."""
    g = g * grad_scale
    if kind == SGD:
        m, = state
        v = a * m - lr * g
        m[...] = v
        p += (a * v - lr * g) if flags & NESTEROV else v
    elif kind == ADAM:
        lr_t = lr * np.sqrt(1.0 - b ** t) / (1.0 - a ** t)
        m, v = state[:2]
        m[...] = a * m + (1.0 - a) * g
        v[...] = b * v + (1.0 - b) * g * g
        if flags & AMSGRAD:
            vh = state[2]
            vh[...] = np.maximum(vh, v)
            p -= lr_t * m / (np.sqrt(vh) + eps)
        else:
            p -= lr_t * m / (np.sqrt(v) + eps)
    else:
        acc, = state
        acc[...] = a * acc + (1.0 - a) * g * g
        p -= lr * g / (np.sqrt(acc) + eps)


# (id, kind, flags, lr, a, b, eps)
KINDS = [
    ("sgd", SGD, 0, 0.01, 0.0, 0.0, 0.0),
    ("sgd-momentum", SGD, 0, 0.01, 0.9, 0.0, 0.0),
    ("sgd-nesterov-m0", SGD, NESTEROV, 0.01, 0.0, 0.0, 0.0),
    ("sgd-nesterov", SGD, NESTEROV, 0.01, 0.9, 0.0, 0.0),
    ("adam", ADAM, 0, 1e-3, 0.9, 0.999, 1e-7),
    ("adam-amsgrad", ADAM, AMSGRAD, 1e-3, 0.9, 0.999, 1e-7),
    ("rmsprop", RMS, 0, 1e-3, 0.9, 0.0, 1e-7),
]
SIZES = [1, 4096 * 256 + 300]  # the grid is capped at 4096 x 256 threads: the loop wraps


def _run(rt, kind, flags, hp, p, gs, state, steps, grad_scale):
    lr, a, b, eps = (_f32(v) for v in hp)
    n = p.size
    P, S = _cuda(p), _cuda(np.concatenate(state))
    p64, s64 = p.astype(np.float64), [s.astype(np.float64) for s in state]
    for t, g in zip(steps, gs):
        cfg = _lib.OptimizerConfig(kind, flags, lr, a, b, eps, t, grad_scale)
        rt.optimizer_update(cfg, P, _cuda(g), S)
        ref_update(kind, flags, lr, a, b, eps, t, grad_scale, p64, g.astype(np.float64), s64)
    assert_close(P.cpu().numpy(), p64, rtol=1e-6, atol=1e-7, what="params")
    got = S.cpu().numpy()
    for i, s in enumerate(s64):
        assert_close(got[i * n:(i + 1) * n], s, rtol=1e-6, atol=1e-7, what=f"state[{i}]")


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name,kind,flags,lr,a,b,eps", KINDS, ids=[k[0] for k in KINDS])
def test_optimizer_first_steps(rt, name, kind, flags, lr, a, b, eps, n, grad_scale):
    """Steps 1 and 2 from zero state."""
    rng = np.random.default_rng(n % 1000 + kind)
    p = rng.standard_normal(n).astype(np.float32)
    gs = [rng.standard_normal(n).astype(np.float32) for _ in range(2)]
    state = [np.zeros(n, np.float32) for _ in range(rt.optimizer_slots(kind, flags))]
    _run(rt, kind, flags, (lr, a, b, eps), p, gs, state, [1, 2], grad_scale)


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name,kind,flags,lr,a,b,eps", KINDS, ids=[k[0] for k in KINDS])
def test_optimizer_step_10000(rt, name, kind, flags, lr, a, b, eps, n, grad_scale):
    """One step at t = 10000 from a random state; AMSGrad's v-hat has entries above and below the new v."""
    rng = np.random.default_rng(n % 1000 + kind + 10)
    p = rng.standard_normal(n).astype(np.float32)
    g = rng.standard_normal(n).astype(np.float32)
    if kind == SGD:
        state = [(rng.standard_normal(n) * 0.1).astype(np.float32)]
    elif kind == RMS:
        state = [rng.uniform(1e-3, 1.0, n).astype(np.float32)]
    else:
        state = [(rng.standard_normal(n) * 0.1).astype(np.float32), rng.uniform(1e-3, 1.0, n).astype(np.float32)]
        if flags & AMSGRAD:
            vh = rng.uniform(1e-3, 1.0, n).astype(np.float32)
            state.append(vh)
            v_new = _f32(b) * state[1].astype(np.float64) + (1 - _f32(b)) * (g.astype(np.float64) * grad_scale) ** 2
            if n > 1:
                assert (vh > v_new).any() and (vh < v_new).any()
    _run(rt, kind, flags, (lr, a, b, eps), p, [g], state, [10000], grad_scale)


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("n", SIZES)
def test_adam_equals_adam_update_bitwise(rt, n, grad_scale):
    """Adam without AMSGRAD == asr_adam_update on the same inputs, bit for bit (steps 1, 2, 10000)."""
    rng = np.random.default_rng(n % 1000 + 7)
    p = rng.standard_normal(n).astype(np.float32)
    m = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v = rng.uniform(1e-3, 1.0, n).astype(np.float32)
    P1, M1, V1 = _cuda(p), _cuda(m), _cuda(v)
    P2, S2 = _cuda(p), _cuda(np.concatenate([m, v]))
    for t in (1, 2, 10000):
        G = _cuda(rng.standard_normal(n).astype(np.float32))
        rt.adam_update(P1, G, M1, V1, 1e-3, 0.9, 0.999, 1e-7, t, grad_scale)
        rt.optimizer_update(_lib.OptimizerConfig(ADAM, 0, 1e-3, 0.9, 0.999, 1e-7, t, grad_scale), P2, G, S2)
    np.testing.assert_array_equal(P1.cpu().numpy(), P2.cpu().numpy())
    np.testing.assert_array_equal(M1.cpu().numpy(), S2[:n].cpu().numpy())
    np.testing.assert_array_equal(V1.cpu().numpy(), S2[n:].cpu().numpy())


def test_optimizer_update_checks_buffers(rt):
    P, G = _cuda(np.zeros(8, np.float32)), _cuda(np.zeros(8, np.float32))
    cfg = _lib.OptimizerConfig(ADAM, AMSGRAD, 1e-3, 0.9, 0.999, 1e-7, 1, 1.0)
    with pytest.raises(ValueError, match="state"):
        rt.optimizer_update(cfg, P, G, _cuda(np.zeros(16, np.float32)))  # AMSGrad keeps 3 buffers
    cfg.step = 0
    with pytest.raises(ValueError, match="asr_optimizer_update"):
        rt.optimizer_update(cfg, P, G, _cuda(np.zeros(24, np.float32)))


# --------------------------------------------------------------------------
# fit / evaluate against a hand-rolled loop on a twin model
# --------------------------------------------------------------------------
K = 10


def _single(seed=0, hw=32, L=3):
    graph.set_seed(seed)
    fn = R.get_single_block_resnet_build_function(h=0.5, num_stages=2, blocks_per_stage=[L], filters_per_block=[16],
                                                  strides=[(1, 1)], subtract_mean=127.5, divide_by_stddev=127.5,
                                                  num_classes=K)
    return fn(Input(shape=(hw, hw, 3)))


def _multi(seed=0):
    """The smallest multi-stage float32 layout of tests/test_gpu_stages.py: [(8, 1, 0), (12, 2, 1)]."""
    graph.set_seed(seed)
    fn = R.get_single_block_resnet_build_function(h=0.5, num_stages=3, blocks_per_stage=[1, 3],
                                                  filters_per_block=[8, 12], strides=[(1, 1), (1, 1)],
                                                  subtract_mean=127.5, divide_by_stddev=127.5, num_classes=K)
    return fn(Input(shape=(32, 32, 3)))


def _data(n, seed, hw=32):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (n, hw, hw, 3)).astype(np.uint8)
    labels = rng.integers(0, K, n)
    return x, optimizers.to_categorical(labels, K), labels


class Twin:
    """The yardstick: a model with the same initial weights, stepped by hand with
    compile_native(B, 'float32').forward_backward (existing code) and the fp64 SGD above; the
    parameters are rounded to float32 after every step, as the device stores them."""

    def __init__(self, model, like, lr, momentum):
        model.set_weights(like.get_weights())
        self.model, self.lr, self.momentum = model, _f32(lr), _f32(momentum)
        self.state = model.compile_native(1, "float32").state
        self.m = [np.zeros(self.state.n_params)]
        self.losses, self.sizes, self.correct = [], [], 0

    def step(self, x, y):
        nv = self.model.compile_native(len(x), "float32")
        loss, grads, probs = nv.forward_backward(x, y, want_probs=True)
        self.losses.append(float(loss.item()))
        self.sizes.append(len(x))
        self.correct += int((probs.cpu().numpy().argmax(1) == y.argmax(1)).sum())
        p = self.state.params.cpu().numpy().astype(np.float64)
        ref_update(SGD, 0, self.lr, self.momentum, 0.0, 0.0, len(self.losses), 1.0, p,
                   grads.cpu().numpy().astype(np.float64), self.m)
        self.state.params.copy_(torch.from_numpy(p.astype(np.float32)))
        self.state.mark_updated()

    def epoch(self, x, y, B, order=None):
        """One pass in batches of B (the last partial); returns (sample-weighted loss, accuracy)."""
        first, self.correct = len(self.losses), 0
        order = np.arange(len(x)) if order is None else order
        for i in range(0, len(x), B):
            sel = order[i:i + B]
            self.step(x[sel], y[sel])
        w = np.array(self.sizes[first:], np.float64)
        return float((np.array(self.losses[first:]) * w).sum() / w.sum()), self.correct / len(x)


def _assert_weights(got_model, want_model):
    got, want = got_model.get_weights(), want_model.get_weights()
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        err = np.abs(a.astype(np.float64) - b).max()
        print(f"weights[{i}] {b.shape}: max err {err:.3e}, max |w| {np.abs(b).max():.3e}")
        assert err <= 1e-5 * np.abs(b).max(), (i, err)


def _assert_rel(got, want, what):
    print(f"{what}: got {got!r} want {want!r} rel {abs(got - want) / abs(want):.3e}")
    assert abs(got - want) <= 1e-5 * abs(want), what


@pytest.mark.parametrize("make", [_single, _multi], ids=["single-stage", "multi-stage"])
def test_fit_in_order_matches_hand_rolled_loop(make):
    """n = 20 in batches of 8, 8, 4 (the tail through a second executor, unpadded), SGD with momentum."""
    x, y, _ = _data(20, 1)
    m = make()
    w0 = m.get_weights()
    twin = Twin(make(), m, 0.05, 0.9)
    m.compile(optimizers.SGD(lr=0.05, momentum=0.9), loss="categorical_crossentropy", metrics=["accuracy"],
              dtype="float32")
    h = m.fit(x, y, batch_size=8, epochs=1, shuffle=False, verbose=0)
    want_loss, want_acc = twin.epoch(x, y, 8)
    assert twin.sizes == [8, 8, 4] and m.optimizer.iterations == 3
    assert list(h.history) == ["loss", "acc"] and h.epoch == [0] and h.params["samples"] == 20
    assert any(np.abs(a - b).max() > 0 for a, b in zip(m.get_weights(), w0))  # it trained
    _assert_weights(m, twin.model)
    _assert_rel(h.history["loss"][0], want_loss, "loss")
    assert h.history["acc"][0] == want_acc


def test_fit_shuffled_two_epochs_matches_hand_rolled_loop():
    """shuffle=True draws np.random.permutation(n) once per epoch from the global generator."""
    x, y, _ = _data(20, 2)
    m = _single()
    twin = Twin(_single(), m, 0.05, 0.9)
    m.compile(optimizers.SGD(lr=0.05, momentum=0.9), metrics=["acc"], dtype="float32")
    np.random.seed(3)
    h = m.fit(x, y, batch_size=8, epochs=2, shuffle=True, verbose=0)
    np.random.seed(3)
    want = [twin.epoch(x, y, 8, np.random.permutation(20)) for _ in range(2)]
    assert m.optimizer.iterations == 6 and h.epoch == [0, 1]
    _assert_weights(m, twin.model)
    for e in range(2):
        _assert_rel(h.history["loss"][e], want[e][0], f"epoch {e} loss")
        assert h.history["acc"][e] == want[e][1]


@pytest.fixture(scope="module")
def trained():
    """A compiled float32 model after one fit epoch with validation data (12 samples: batches 8, 4)."""
    x, y, _ = _data(20, 3)
    xv, yv, lv = _data(12, 4)
    m = _single(seed=1)
    m.compile(optimizers.SGD(lr=0.05, momentum=0.9), metrics=["accuracy"], dtype="float32")
    h = m.fit(x, y, batch_size=8, epochs=1, shuffle=False, validation_data=(xv, yv), verbose=0)
    return m, h, (x, y), (xv, yv, lv)


def test_validation_metrics(trained):
    m, h, _, (xv, yv, lv) = trained
    assert list(h.history) == ["loss", "acc", "val_loss", "val_acc"]
    loss, acc = m.evaluate(xv, yv, batch_size=8, verbose=0)
    _assert_rel(h.history["val_loss"][0], loss, "val_loss vs evaluate")
    assert h.history["val_acc"][0] == acc
    probs = m.predict(xv, dtype="float32").astype(np.float64)
    _assert_rel(loss, float(O.keras_cce(probs, yv.astype(np.float64)).mean()), "evaluate vs numpy CCE")
    assert acc == float((probs.argmax(1) == lv).mean())
    # without metrics: the scalar loss
    m2 = _single(seed=1)
    m2.set_weights(m.get_weights())
    m2.compile("sgd", dtype="float32")
    _assert_rel(m2.evaluate(xv, yv, batch_size=8, verbose=0), loss, "evaluate without metrics")


def test_evaluate_and_test_on_batch_leave_the_weights(trained):
    m, _, (x, y), (xv, yv, _) = trained
    before = m.get_weights()
    it = m.optimizer.iterations
    m.evaluate(xv, yv, batch_size=8, verbose=0)
    m.test_on_batch(x[:5], y[:5])
    m._native.mark_updated()  # read the device parameters back, not the host copies
    for a, b in zip(m.get_weights(), before):
        np.testing.assert_array_equal(a, b)
    assert m.optimizer.iterations == it


def test_train_on_batch():
    x, y, _ = _data(8, 9)
    m = _single(seed=2)
    m.compile(optimizers.SGD(lr=0.05, momentum=0.9), metrics=["accuracy"], dtype="float32")
    before = m.get_weights()
    it = m.optimizer.iterations
    t_loss, t_acc = m.test_on_batch(x[:8], y[:8])
    loss, acc = m.train_on_batch(x[:8], y[:8])
    _assert_rel(loss, t_loss, "train_on_batch loss vs test_on_batch before it")
    assert acc == t_acc and m.optimizer.iterations == it + 1
    assert any(np.abs(a - b).max() > 0 for a, b in zip(m.get_weights(), before))
    assert m.test_on_batch(x[:8], y[:8])[0] != t_loss


def test_fit_dataset_form():
    from differential_equations_resnet_amd.dataset_utils import ArrayDataset
    x, _, labels = _data(32, 5)
    ds = ArrayDataset(x, labels, 8, seed=1, num_classes=K)
    m = _single()
    m.compile(optimizers.SGD(lr=0.01), metrics=["accuracy"], dtype="float32")
    with pytest.raises(ValueError, match="steps_per_epoch"):
        m.fit(ds, verbose=0)
    assert m.optimizer.iterations == 0
    h = m.fit(ds, steps_per_epoch=3, epochs=2, validation_data=ds, validation_steps=2, verbose=0)
    assert m.optimizer.iterations == 6
    assert h.params["steps"] == 3 and len(h.history["loss"]) == 2 and len(h.history["val_acc"]) == 2
    assert np.isfinite(h.history["loss"]).all() and np.isfinite(h.history["val_loss"]).all()


def test_fit_default_dtype_learns():
    """The default executor dtype (bfloat16 single-stage) at 16 x 16, 'adam', learnable data (the
    class sets the image brightness, as test_training_overfits_one_batch's): the loss falls."""
    rng = np.random.default_rng(2)
    labels = rng.integers(0, 4, 24)
    x = np.clip(labels[:, None, None, None] * 60 + 20 + rng.integers(-15, 16, (24, 16, 16, 3)), 0, 255).astype(np.uint8)
    m = _single(hw=16, L=2)
    m.compile(optimizer="adam", loss="categorical_crossentropy", metrics=["accuracy"])
    h = m.fit(x, optimizers.to_categorical(labels, K), batch_size=8, epochs=2, verbose=0)
    assert m._native.resolve_dtype(None) == "bfloat16" and m.optimizer.iterations == 6
    print("losses", h.history["loss"], "acc", h.history["acc"])
    assert np.isfinite(h.history["loss"]).all()
    m._native.check_status()
    assert h.history["loss"][1] < h.history["loss"][0]


def test_fit_verbose_bar(capsys):
    x, y, _ = _data(12, 6)
    m = _single()
    m.compile("sgd", metrics=["accuracy"], dtype="float32")
    m.fit(x, y, batch_size=8, epochs=1, verbose=1)
    assert "Epoch 1/1" in capsys.readouterr().out


# --------------------------------------------------------------------------
# Training with the new optimisers
# --------------------------------------------------------------------------
def _training(optimizer, x, labels, tmp_path):
    from differential_equations_resnet_amd.dataset_utils import ArrayDataset
    from differential_equations_resnet_amd.training import Training
    ds = ArrayDataset(x, labels, 8, shuffle=False, num_classes=K)
    graph.set_seed(0)
    build = R.get_single_block_resnet_build_function(h=0.5, num_stages=2, blocks_per_stage=[3],
                                                     filters_per_block=[16], strides=[(1, 1)], subtract_mean=127.5,
                                                     divide_by_stddev=127.5, num_classes=K)
    return Training(build, "antisymmetric", optimizer, train_dataset=ds, record_summaries=False, dtype="float32")


def test_training_with_sgd(tmp_path):
    x, y, labels = _data(24, 7)
    opt = optimizers.SGD(lr=123.0, momentum=0.9)  # the schedule's rate replaces lr
    tr = _training(opt, x, labels, tmp_path)
    twin = Twin(_single(), tr.model, 0.05, 0.9)
    for i in range(2):
        tr.train_step(0.05)
        twin.step(x[8 * i:8 * i + 8], y[8 * i:8 * i + 8])
    assert opt.iterations == 2 and tr.g_step == 2
    _assert_weights(tr.model, twin.model)
    # save -> one more step -> load_variables: weights, optimiser state and iterations come back bitwise
    path = tr.save(str(tmp_path / "ckpt"), "train_saver")
    w = tr.model.get_weights()
    s = tr.native.opt_state.cpu().numpy().copy()
    tr.train_step(0.05)
    assert opt.iterations == 3 and np.abs(tr.native.opt_state.cpu().numpy() - s).max() > 0
    tr.load_variables(path)
    for a, b in zip(tr.model.get_weights(), w):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(tr.native.opt_state.cpu().numpy(), s)
    assert opt.iterations == 2 and tr.g_step == 2
    # and the next step continues from that state: it equals the twin's third step (the dataset
    # went on: batches 0, 1, 2 are drawn, the stream repeats with batch 0)
    tr.train_step(0.05)
    twin.step(x[0:8], y[0:8])
    _assert_weights(tr.model, twin.model)
    tr.close()


def test_training_with_adam_optimizer_is_unchanged(rt, tmp_path):
    """AdamOptimizer still runs asr_adam_update: two steps give the parameters runtime.adam_update
    gives by hand on a twin, bit for bit."""
    from differential_equations_resnet_amd.training import AdamOptimizer
    x, y, labels = _data(16, 8)
    tr = _training(AdamOptimizer(epsilon=1e-7), x, labels, tmp_path)
    twin = _single()
    twin.set_weights(tr.model.get_weights())
    nv = twin.compile_native(8, "float32")
    m, v = torch.zeros_like(nv.params), torch.zeros_like(nv.params)
    for t in (1, 2):
        tr.train_step(1e-3)
        _, grads, _ = nv.forward_backward(x[8 * t - 8:8 * t], y[8 * t - 8:8 * t])
        rt.adam_update(nv.params, grads, m, v, 1e-3, 0.9, 0.999, 1e-7, t)
    assert tr.native.opt_state is None and tr.native.step == 2
    np.testing.assert_array_equal(tr.native.params.cpu().numpy(), nv.params.cpu().numpy())
    tr.close()
