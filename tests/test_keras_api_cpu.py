"""CPU tests of the Keras training surface: the optimiser C ABI's host side
(asr_optimizer_slots, asr_optimizer_update's argument checks: no launch is made),
optimizers.SGD / Adam / RMSprop / get / to_categorical, and what Model.compile /
fit / evaluate decide on the host before any device use."""
import ctypes as ct

import numpy as np
import pytest

from differential_equations_resnet_amd import _lib, graph, optimizers
from differential_equations_resnet_amd.graph import Input
from differential_equations_resnet_amd.models import tfkeras_resnets as R

SGD, ADAM, RMS = _lib.ASR_OPT_SGD, _lib.ASR_OPT_ADAM, _lib.ASR_OPT_RMSPROP
NESTEROV, AMSGRAD = _lib.ASR_OPT_NESTEROV, _lib.ASR_OPT_AMSGRAD


@pytest.fixture(scope="module")
def lib():
    return _lib.load(build_if_missing=True)


def test_abi_version(lib):
    assert lib.asr_abi_version() == 13


@pytest.mark.parametrize("kind,flags,want", [
    (SGD, 0, 1), (SGD, NESTEROV, 1), (ADAM, 0, 2), (ADAM, AMSGRAD, 3), (RMS, 0, 1),
    (SGD, AMSGRAD, -1), (SGD, NESTEROV | AMSGRAD, -1), (ADAM, NESTEROV, -1), (RMS, NESTEROV, -1), (RMS, AMSGRAD, -1),
    (SGD, 4, -1), (3, 0, -1), (-1, 0, -1),
])
def test_optimizer_slots(lib, kind, flags, want):
    assert lib.asr_optimizer_slots(kind, flags) == want


def _cfg(kind=SGD, flags=0, step=1):
    return _lib.OptimizerConfig(kind, flags, 0.01, 0.9, 0.999, 1e-7, step, 1.0)


def test_optimizer_config_layout():
    """asr_optimizer_config as the C compiler lays it out on LP64: step is 8-byte aligned."""
    C = _lib.OptimizerConfig
    assert (C.kind.offset, C.flags.offset, C.lr.offset, C.a.offset, C.b.offset, C.eps.offset) == (0, 4, 8, 12, 16, 20)
    assert (C.step.offset, C.grad_scale.offset, ct.sizeof(C)) == (24, 32, 40)


@pytest.mark.parametrize("what,kw", [
    ("cfg", dict(cfg=None)), ("params", dict(params=None)), ("grads", dict(grads=None)), ("state", dict(state=None)),
    ("n", dict(n=-1)), ("step 0", dict(cfg=_cfg(step=0))), ("step < 0", dict(cfg=_cfg(step=-3))),
    ("kind 3", dict(cfg=_cfg(kind=3))), ("kind -1", dict(cfg=_cfg(kind=-1))),
    ("sgd + amsgrad", dict(cfg=_cfg(SGD, AMSGRAD))), ("adam + nesterov", dict(cfg=_cfg(ADAM, NESTEROV))),
    ("rmsprop + nesterov", dict(cfg=_cfg(RMS, NESTEROV))), ("rmsprop + amsgrad", dict(cfg=_cfg(RMS, AMSGRAD))),
    ("unknown flag", dict(cfg=_cfg(ADAM, 4))),
])
def test_optimizer_update_bad_arguments(lib, what, kw):
    """ASR_E_ARG before any launch (there is no device here; the pointers are never dereferenced),
    with the function's name in asr_last_error()."""
    fake = ct.c_void_p(256)
    args = dict(cfg=_cfg(), params=fake, grads=fake, state=fake, n=8)
    args.update(kw)
    cfg = None if args["cfg"] is None else ct.byref(args["cfg"])
    lib.asr_param_map(0, 0, 1, None, None)  # another call's message first
    rc = lib.asr_optimizer_update(cfg, args["params"], args["grads"], args["state"], args["n"], None)
    assert rc == _lib.ASR_E_ARG, what
    assert b"asr_optimizer_update" in lib.asr_last_error()


@pytest.mark.parametrize("kind,flags", [(SGD, 0), (SGD, NESTEROV), (ADAM, 0), (ADAM, AMSGRAD), (RMS, 0)])
def test_optimizer_update_empty_is_ok(lib, kind, flags):
    fake = ct.c_void_p(256)
    assert lib.asr_optimizer_update(ct.byref(_cfg(kind, flags)), fake, fake, fake, 0, None) == _lib.ASR_OK


def test_optimizer_defaults_and_config():
    assert optimizers.SGD().get_config() == {"lr": 0.01, "momentum": 0.0, "decay": 0.0, "nesterov": False}
    assert optimizers.Adam().get_config() == {"lr": 0.001, "beta_1": 0.9, "beta_2": 0.999, "decay": 0.0,
                                              "epsilon": 1e-7, "amsgrad": False}
    assert optimizers.RMSprop().get_config() == {"lr": 0.001, "rho": 0.9, "decay": 0.0, "epsilon": 1e-7}
    assert optimizers.Adam(epsilon=1e-3).epsilon == 1e-3 and optimizers.RMSprop(epsilon=1e-4).epsilon == 1e-4
    for o in (optimizers.SGD(), optimizers.Adam(), optimizers.RMSprop()):
        assert o.iterations == 0
        assert type(o)(**o.get_config()).get_config() == o.get_config()
    assert [o.slots() for o in (optimizers.SGD(), optimizers.SGD(nesterov=True), optimizers.Adam(),
                                optimizers.Adam(amsgrad=True), optimizers.RMSprop())] == [1, 1, 2, 3, 1]
    with pytest.raises(ValueError, match="lr"):
        optimizers.SGD(lr="fast")
    with pytest.raises(ValueError, match="decay"):
        optimizers.SGD(decay=-1.0)


def test_get():
    from differential_equations_resnet_amd.training import AdamOptimizer
    for name, cls in (("sgd", optimizers.SGD), ("adam", optimizers.Adam), ("rmsprop", optimizers.RMSprop),
                      ("Adam", optimizers.Adam), ("SGD", optimizers.SGD), ("RMSprop", optimizers.RMSprop)):
        o = optimizers.get(name)
        assert type(o) is cls and o.get_config() == cls().get_config()
    inst = optimizers.SGD(lr=0.5, momentum=0.9)
    assert optimizers.get(inst) is inst
    with pytest.raises(ValueError, match="adagrad"):
        optimizers.get("adagrad")
    with pytest.raises(ValueError):
        optimizers.get(3)
    a = optimizers.get(AdamOptimizer(2e-3, beta1=0.8, beta2=0.99, epsilon=1e-6))
    assert type(a) is optimizers.Adam
    assert a.get_config() == {"lr": 2e-3, "beta_1": 0.8, "beta_2": 0.99, "decay": 0.0, "epsilon": 1e-6,
                              "amsgrad": False}
    with pytest.raises(ValueError, match="learning_rate"):
        optimizers.get(AdamOptimizer(learning_rate=lambda step: 1e-3))


def test_decayed_learning_rate_and_filled_config():
    """lr = lr0 / (1 + decay * iterations) with iterations the updates already applied; step is
    iterations + 1; a passed lr replaces lr0 and decays the same way."""
    o = optimizers.SGD(lr=0.1, momentum=0.9, decay=0.01, nesterov=True)
    for k in (0, 1, 7, 1000):
        o.iterations = k
        c = o.next_config()
        assert c.lr == np.float32(0.1 / (1 + 0.01 * k)) and c.step == k + 1
        assert o.next_config(lr=0.5).lr == np.float32(0.5 / (1 + 0.01 * k))
        assert o.iterations == k  # filling a config is pure
    assert (c.kind, c.flags, c.a, c.b, c.eps, c.grad_scale) == (SGD, NESTEROV, np.float32(0.9), 0.0, 0.0, 1.0)
    assert optimizers.SGD().next_config().flags == 0
    a = optimizers.Adam(lr=2e-3, beta_1=0.8, beta_2=0.99, epsilon=1e-6, amsgrad=True)
    a.iterations = 4
    c = a.next_config(grad_scale=0.125)
    assert (c.kind, c.flags, c.lr, c.a, c.b, c.eps, c.step, c.grad_scale) == \
        (ADAM, AMSGRAD, np.float32(2e-3), np.float32(0.8), np.float32(0.99), np.float32(1e-6), 5, 0.125)
    assert optimizers.Adam().next_config().flags == 0 and optimizers.Adam().next_config().eps == np.float32(1e-7)
    c = optimizers.RMSprop(lr=3e-3, rho=0.95, decay=0.5).next_config()
    assert (c.kind, c.flags, c.lr, c.a, c.eps, c.step) == (RMS, 0, np.float32(3e-3), np.float32(0.95),
                                                            np.float32(1e-7), 1)


def test_to_categorical():
    y = optimizers.to_categorical([0, 2, 1, 2])
    assert y.dtype == np.float32 and y.shape == (4, 3)
    np.testing.assert_array_equal(y, np.eye(3, dtype=np.float32)[[0, 2, 1, 2]])
    y = optimizers.to_categorical(np.array([[1], [0]]), num_classes=10)  # CIFAR-10's [n, 1] label column
    assert y.shape == (2, 10) and y[0, 1] == 1 and y[1, 0] == 1 and y.sum() == 2
    assert optimizers.to_categorical(np.array([[0, 1], [2, 0]])).shape == (2, 2, 3)
    with pytest.raises(ValueError):
        optimizers.to_categorical([0, 3], num_classes=3)
    with pytest.raises(ValueError):
        optimizers.to_categorical([-1, 0])


def _model():
    graph.set_seed(0)
    fn = R.get_single_block_resnet_build_function(h=0.5, num_stages=2, blocks_per_stage=[2], filters_per_block=[16],
                                                  strides=[(1, 1)], subtract_mean=127.5, divide_by_stddev=127.5,
                                                  num_classes=10)
    return fn(Input(shape=(16, 16, 3)))


X = np.zeros((6, 16, 16, 3), np.uint8)
Y = np.eye(10, dtype=np.float32)[[0, 1, 2, 3, 4, 5]]


def test_compile_needs_no_gpu_and_checks_its_arguments():
    m = _model()
    assert m.optimizer is None
    m.compile(optimizer="adam", loss="categorical_crossentropy", metrics=["accuracy"])
    assert type(m.optimizer) is optimizers.Adam and m._native is None  # nothing lowered
    opt = optimizers.SGD(lr=0.05, momentum=0.9)
    for metrics in (None, [], ["accuracy"], ["acc"]):
        m.compile(opt, metrics=metrics, dtype="float32")
        assert m.optimizer is opt
    with pytest.raises(ValueError, match="loss"):
        m.compile("adam", loss="mse")
    with pytest.raises(ValueError, match="loss"):
        m.compile("adam", loss=lambda a, b: 0)
    with pytest.raises(ValueError, match="metrics"):
        m.compile("adam", metrics=["mae"])
    with pytest.raises(ValueError, match="metrics"):
        m.compile("adam", metrics=["accuracy", "acc"])
    with pytest.raises(ValueError, match="optimizer"):
        m.compile("adagrad")
    with pytest.raises(ValueError, match="dtype"):
        m.compile("adam", dtype="float16")
    assert m.optimizer is opt  # a refused compile leaves the last one in place


def test_training_calls_before_compile():
    m = _model()
    for call in (lambda: m.fit(X, Y), lambda: m.evaluate(X, Y), lambda: m.train_on_batch(X, Y),
                 lambda: m.test_on_batch(X, Y)):
        with pytest.raises(RuntimeError, match="You must compile a model before training/testing"):
            call()


@pytest.mark.parametrize("name,kw", [
    ("callbacks", dict(callbacks=[object()])), ("validation_split", dict(validation_split=0.1)),
    ("class_weight", dict(class_weight={0: 2.0})), ("sample_weight", dict(sample_weight=np.ones(6))),
])
def test_fit_refused_arguments(name, kw):
    """Refused before any device use (this test has no device)."""
    m = _model()
    m.compile("sgd")
    with pytest.raises(_lib.AsrUnsupported, match=name):
        m.fit(X, Y, verbose=0, **kw)
    assert m._native is None and m.optimizer.iterations == 0


def test_fit_refused_while_distributed(monkeypatch):
    from differential_equations_resnet_amd import distributed
    m = _model()
    m.compile("sgd")
    monkeypatch.setattr(distributed, "is_initialized", lambda: True)
    with pytest.raises(_lib.AsrUnsupported, match="distributed"):
        m.fit(X, Y, verbose=0)
    assert m._native is None


def test_fit_argument_errors_before_device_use():
    m = _model()
    m.compile("sgd")
    with pytest.raises(ValueError, match="to_categorical"):
        m.fit(X, np.arange(6), verbose=0)
    with pytest.raises(ValueError, match="to_categorical"):
        m.evaluate(X, np.arange(6), verbose=0)
    with pytest.raises(ValueError, match="verbose"):
        m.fit(X, Y, verbose=2)
    with pytest.raises(ValueError, match="samples"):
        m.fit(X, Y[:5], verbose=0)

    class FakeDataset:  # what fit reads of a dataset before it draws a batch
        output_shapes = ((2, 16, 16, 3), (2, 10))

        def __iter__(self):
            raise AssertionError("no batch may be drawn")

    with pytest.raises(ValueError, match="steps_per_epoch"):
        m.fit(FakeDataset(), verbose=0)
    with pytest.raises(ValueError, match="validation_steps"):
        m.fit(X, Y, validation_data=FakeDataset(), verbose=0)
    assert m._native is None
    # empty callbacks, a zero split and no weights are Keras' defaults, not refusals: they pass the
    # host checks and fail only at the device
    from differential_equations_resnet_amd._lib import AsrError
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(AsrError, match="gfx950"):
            m.fit(X, Y, verbose=0, callbacks=[], validation_split=0.0)
