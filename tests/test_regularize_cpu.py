"""CPU tests of the weight regularisers: the asr_regularize binding and its host-side table check, the
segment tables lowering builds from a model's l2 regularisers and smoothness_regularization, and
Model.losses against tests/reg_ref.py.  No kernel is launched (tests/test_gpu_regularize.py does that)."""
import ctypes as ct
import inspect

import numpy as np
import pytest

import reg_ref
from differential_equations_resnet_amd import _lib, graph, lowering
from differential_equations_resnet_amd.graph import Input
from differential_equations_resnet_amd.models import tfkeras_resnets as R

K = 10


@pytest.fixture(scope="module")
def lib():
    return _lib.load(build_if_missing=True)


def _check(lib, rows, n_params):
    tab = (_lib.RegSegment * max(len(rows), 1))(*[_lib.RegSegment(*r) for r in rows])
    return lib.asr_regularize_check(ct.cast(tab, ct.c_void_p), len(rows), n_params)


# --------------------------------------------------------------------------
# binding and check
# --------------------------------------------------------------------------
def test_binding_exists_and_abi_version(lib):
    bound = {n for n, _, _ in _lib.SIGNATURES}
    assert {"asr_regularize_check", "asr_regularize_workspace_bytes", "asr_regularize"} <= bound
    assert _lib.ABI_VERSION == 13 and lib.asr_abi_version() == 13
    assert _lib.ASR_REG_MAX_SEGMENTS == 256 and ct.sizeof(_lib.RegSegment) == 40


OK = (10, 5, 5, 1, 0.1, 0.0)
MALFORMED = [
    ("count", (10, 0, 5, 1, 0.1, 0.0)),
    ("layers", (10, 5, 5, 0, 0.1, 0.0)),
    ("layer_stride", (10, 5, 4, 2, 0.1, 0.0)),
    ("end-plain", (96, 5, 5, 1, 0.1, 0.0)),
    ("end-stack", (10, 5, 30, 4, 0.1, 0.0)),  # the last layer ends at 10 + 3 * 30 + 5 = 105 > 100
    ("negative-offset", (-1, 5, 5, 1, 0.1, 0.0)),
    ("negative-l2", (10, 5, 5, 1, -0.1, 0.0)),
    ("nan-l2", (10, 5, 5, 1, float("nan"), 0.0)),
    ("inf-smooth", (10, 5, 5, 2, 0.0, float("inf"))),
    ("negative-smooth", (10, 5, 5, 2, 0.0, -1.0)),
]


@pytest.mark.parametrize("name,row", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_check_refuses_a_malformed_segment_and_names_it(lib, name, row):
    assert _check(lib, [OK], 100) == _lib.ASR_OK
    assert _check(lib, [(0, 5, 5, 1, 0.1, 0.0), row], 100) == _lib.ASR_E_ARG
    msg = lib.asr_last_error().decode()
    assert "asr_regularize_check" in msg and "segment 1" in msg, msg


def test_check_segment_count_bounds(lib):
    assert _check(lib, [], 100) == _lib.ASR_OK  # an empty table
    assert lib.asr_regularize_check(None, 0, 0) == _lib.ASR_OK
    assert lib.asr_regularize_check(None, -1, 100) == _lib.ASR_E_ARG
    rows = [(i, 1, 1, 1, 0.1, 0.0) for i in range(257)]
    assert _check(lib, rows[:256], 300) == _lib.ASR_OK
    assert _check(lib, rows, 300) == _lib.ASR_E_ARG
    assert "n_segments" in lib.asr_last_error().decode()


def test_check_overlap(lib):
    nt, C = 37, 8  # thetas and biases of 4 blocks at one stride: interleaved, not overlapping
    theta, bias = (3, nt, nt + C, 4, 0.1, 0.2), (3 + nt, C, nt + C, 4, 0.0, 0.2)
    n = 3 + 4 * (nt + C)
    assert _check(lib, [theta, bias], n) == _lib.ASR_OK
    assert _check(lib, [bias, theta], n) == _lib.ASR_OK
    for other in [(3 + nt - 1, C, nt + C, 4, 0.0, 0.2),          # the biases one float early: on every theta's end
                  (3 + 2 * (nt + C) + 5, 1, 1, 1, 0.1, 0.0),     # one float inside the third theta
                  (0, 4, 4, 1, 0.1, 0.0),                        # the last float on the first theta's first
                  (3 + 3 * (nt + C) + nt - 1, 2, 2, 1, 0.1, 0.0)]:  # straddles the last theta's end
        for rows in ([theta, other], [other, theta]):
            assert _check(lib, rows, n) == _lib.ASR_E_ARG, other
            msg = lib.asr_last_error().decode()
            assert "segments 0 and 1 overlap" in msg, msg
    # touching is not overlapping
    assert _check(lib, [theta, (0, 3, 3, 1, 0.1, 0.0), (3 + nt, 1, 1, 1, 0.1, 0.0)], n) == _lib.ASR_OK
    assert _check(lib, [OK, OK], 100) == _lib.ASR_E_ARG


def test_check_overlap_against_brute_force(lib):
    """Random pairs of small segments: the check's answer is the coverage masks' intersection."""
    rng = np.random.default_rng(0)
    n, seen = 64, set()
    for _ in range(400):
        rows = []
        for _ in range(2):
            count, layers = int(rng.integers(1, 5)), int(rng.integers(1, 5))
            stride = count + int(rng.integers(0, 6))
            offset = int(rng.integers(0, n - ((layers - 1) * stride + count) + 1))
            rows.append((offset, count, stride, layers, 0.1, 0.1))
        a, b = (reg_ref.covered([r], n) for r in rows)
        want = _lib.ASR_E_ARG if (a & b).any() else _lib.ASR_OK
        assert _check(lib, rows, n) == want, rows
        seen.add(want)
    assert seen == {_lib.ASR_OK, _lib.ASR_E_ARG}


def test_workspace_bytes(lib):
    assert lib.asr_regularize_workspace_bytes(1, 1) > 0
    assert lib.asr_regularize_workspace_bytes(3, 600000) >= lib.asr_regularize_workspace_bytes(3, 2000) > 0
    assert lib.asr_regularize_workspace_bytes(0, 100) == 0
    assert lib.asr_regularize_workspace_bytes(257, 100) == 0


def test_regularize_argument_checks_come_before_any_launch(lib):
    fake = ct.c_void_p(256)  # never dereferenced
    f = ct.c_float
    assert lib.asr_regularize(None, 0, None, None, f(1.0), None, None, None, 0, None) == _lib.ASR_OK
    assert lib.asr_regularize(fake, 257, fake, fake, f(1.0), None, None, fake, 64, None) == _lib.ASR_E_ARG
    assert lib.asr_regularize(fake, 2, None, fake, f(1.0), None, None, fake, 64, None) == _lib.ASR_E_ARG
    assert lib.asr_regularize(fake, 2, fake, fake, f(0.0), None, None, fake, 64, None) == _lib.ASR_E_ARG
    assert "grad_scale" in lib.asr_last_error().decode()
    assert lib.asr_regularize(fake, 2, fake, fake, f(1.0), None, None, fake, 4, None) == _lib.ASR_E_WORKSPACE
    assert lib.asr_regularize(fake, 2, fake, fake, f(1.0), None, None, None, 64, None) == _lib.ASR_E_WORKSPACE


# --------------------------------------------------------------------------
# segments from a model
# --------------------------------------------------------------------------
def _single(l2=0.0, alpha=0.0, seed=0, L=3, C=16, **kw):
    graph.set_seed(seed)
    fn = R.get_single_block_resnet_build_function(h=0.5, num_stages=2, blocks_per_stage=[L], filters_per_block=[C],
                                                  strides=[(1, 1)], subtract_mean=127.5, divide_by_stddev=127.5,
                                                  num_classes=K, l2_regularization=l2,
                                                  smoothness_regularization=alpha, **kw)
    return fn(Input(shape=(32, 32, 3)))


def _offsets(plan):
    pos, off = {}, 0
    for v in plan.weight_vars():
        pos[v.name] = (off, v.value.size)
        off += v.value.size
    return pos, off


def test_l2_segments_of_a_single_stage_model(lib):
    m = _single(l2=0.01)
    plan = lowering.analyze(m)
    segs = plan.regularization_segments()
    pos, n = _offsets(plan)
    C, L = 16, 3
    nt = plan.block_theta_sizes()[0]
    l2 = float(np.float32(0.01))
    first_theta = pos[plan.blocks[0].weights[0].name][0]
    assert segs == [(0, 27 * C, 27 * C, 1, l2, 0.0),
                    (first_theta, nt, nt + C, L, l2, 0.0),
                    (pos["fc/kernel"][0], C * K, C * K, 1, l2, 0.0)]
    assert _check(lib, segs, n) == _lib.ASR_OK
    # exactly the kernels are covered: conv1's, every block's thetas, fc's; no bias
    want = np.zeros(n, bool)
    for v in plan.weight_vars():
        o, sz = pos[v.name]
        want[o:o + sz] = not v.name.endswith("/bias")
    assert want.sum() == 27 * C + L * nt + C * K
    np.testing.assert_array_equal(reg_ref.covered(segs, n), want)


def test_model_losses_equal_the_reference_per_variable():
    m = _single(l2=0.01, seed=3)
    regd = [w for w in m.weights if not w.name.endswith("/bias")]
    assert len(regd) > 3 and all(w.regularizer is not None for w in regd)
    got = m.losses
    assert len(got) == len(regd) and all(isinstance(v, float) for v in got)
    for g, w in zip(got, regd):
        want = reg_ref.l2_loss(w.value, 0.01)
        assert want > 0 and abs(g - want) <= 1e-12 * want, w.name
    # and their sum is the reference's R over the model's segments
    plan = lowering.analyze(m)
    flat = np.concatenate([v.value.ravel() for v in plan.weight_vars()])
    Rref, _ = reg_ref.penalty(flat, plan.regularization_segments())
    assert abs(sum(got) - Rref) <= 1e-12 * Rref


def test_zero_coefficients_give_no_segments_and_no_losses():
    m = _single(l2=0.0)
    assert lowering.analyze(m).regularization_segments() == []
    assert m.losses == []
    assert lowering.analyze(_single()).smoothness_regularization == 0.0


def _he(alpha, l2=0.0, blocks=(3, 3, 2)):
    graph.set_seed(0)
    fn = R.get_single_block_resnet_build_function(h=0.5, num_stages=4, blocks_per_stage=list(blocks),
                                                  filters_per_block=[16, 32, 64],
                                                  strides=[(1, 1), (2, 2), (2, 2)], num_classes=K,
                                                  l2_regularization=l2, smoothness_regularization=alpha)
    return fn(Input(shape=(32, 32, 3)))


def test_smoothness_segments_of_a_three_stage_model(lib):
    """Stages of 3, 2 and 1 identity blocks (the later stages open with a transition): one theta and one
    bias segment for each of the first two, nothing for the third, nothing across a transition."""
    plan = lowering.analyze(_he(0.1))
    assert isinstance(plan, lowering.StagesPlan) and plan.smoothness_regularization == 0.1
    assert [len(b) for b in plan.stage_blocks] == [3, 2, 1]
    segs = plan.regularization_segments()
    pos, n = _offsets(plan)
    smooth = float(np.float32(0.1 / (2 * 0.5)))
    want = []
    for blocks in plan.stage_blocks[:2]:
        C = blocks[0].weights[-1].value.size
        nt = sum(v.value.size for v in blocks[0].weights[:-1])
        o = pos[blocks[0].weights[0].name][0]
        want += [(o, nt, nt + C, len(blocks), 0.0, smooth), (o + nt, C, nt + C, len(blocks), 0.0, smooth)]
    assert segs == want
    assert _check(lib, segs, n) == _lib.ASR_OK
    cov = reg_ref.covered(segs, n)
    for name in ["conv1/kernel", "conv1/bias", "fc/kernel", "fc/bias"] + \
            [c.kernel.name for tr in plan.transitions if tr for c in tr] + \
            [v.name for v in plan.stage_blocks[2][0].weights]:
        o, sz = pos[name]
        assert not cov[o:o + sz].any(), name
    for blocks in plan.stage_blocks[:2]:
        for b in blocks:
            for v in b.weights:
                o, sz = pos[v.name]
                assert cov[o:o + sz].all(), v.name


def test_smoothness_with_l2_shares_the_theta_segment():
    plan = lowering.analyze(_he(0.1, l2=0.01))
    segs = plan.regularization_segments()
    l2, smooth = float(np.float32(0.01)), float(np.float32(0.1))
    carrying = [s for s in segs if s[5] > 0]
    assert len(carrying) == 4 and all(s[5] == smooth for s in carrying)
    assert sorted(s[4] for s in carrying) == [0.0, 0.0, l2, l2]  # theta with l2, bias without
    plain = [s for s in segs if s[5] == 0]
    # conv1, two transitions' two kernels, the single block of the last stage, fc: l2 only
    assert len(plain) == 1 + 4 + 1 + 1 and all(s[4] == l2 for s in plain)
    assert all(s[3] == 1 for s in plain)


def test_single_stage_smoothness_and_rk2():
    for kw in ({}, {"integrator": "rk2"}):
        plan = lowering.analyze(_single(alpha=0.5, **kw))
        segs = plan.regularization_segments()
        nt, C = plan.block_theta_sizes()[0], 16
        o = 27 * C + C
        s = float(np.float32(0.5))
        assert segs == [(o, nt, nt + C, 3, 0.0, s), (o + nt, C, nt + C, 3, 0.0, s)]
    assert lowering.analyze(_single(alpha=0.5, L=1)).regularization_segments() == []


def test_mixed_alpha_is_refused():
    m = _single(alpha=0.5)
    lowering.analyze(m)
    m.get_layer("res2_1_branch2").smoothness_regularization = 0.25
    with pytest.raises(_lib.AsrUnsupported, match="smoothness_regularization"):
        lowering.analyze(m)
    with pytest.raises(ValueError, match="smoothness_regularization"):
        _single(alpha=-1.0)


def test_unsupported_regularisers_are_refused():
    m = _single(l2=0.01)
    plan = lowering.analyze(m)
    plan.conv1.bias.regularizer = graph.l2(0.01)
    with pytest.raises(_lib.AsrUnsupported, match="bias_regularizer"):
        plan.regularization_segments()
    plan.conv1.bias.regularizer = None
    plan.fc.kernel.regularizer = object()  # an l1 or activity regulariser: anything that is not graph.L2
    with pytest.raises(_lib.AsrUnsupported, match="fc/kernel"):
        plan.regularization_segments()


def test_training_drops_regularisation_losses_by_default():
    from differential_equations_resnet_amd.training import Training
    p = inspect.signature(Training.__init__).parameters["regularization_losses"]
    assert p.default is False


@pytest.mark.parametrize("on", [False, True])
def test_training_step_calls_the_regulariser_only_when_asked(monkeypatch, on):
    """train_step on a stand-in for the native model (no device): regularize is called once, after the
    all-reduce and before the update, with grad_scale = 1 / world, only with regularization_losses."""
    torch = pytest.importorskip("torch")
    from differential_equations_resnet_amd import distributed, runtime
    from differential_equations_resnet_amd.training import AdamOptimizer, Training
    calls = []

    class Native:
        device = torch.device("cpu")

        def forward_backward(self, images, labels, want_probs=False):
            calls.append("forward_backward")
            return "loss", "grads", "probs"

        def regularize(self, grads, grad_scale, loss):
            calls.append(("regularize", grads, grad_scale, loss))

        def apply_adam(self, grads, *a, **kw):
            calls.append(("update", kw["grad_scale"]))

    monkeypatch.setattr(distributed, "allreduce_grads", lambda g: calls.append("allreduce"))
    monkeypatch.setattr(runtime, "batch_metrics", lambda *a: calls.append("metrics"))
    tr = object.__new__(Training)
    tr._torch, tr.native, tr.world, tr.batch_size = torch, Native(), 4, 2
    tr.optimizer, tr.g_step, tr.regularization_losses = AdamOptimizer(), 0, on
    tr._train_iter = iter([(np.zeros((2, 4, 4, 3), np.uint8), np.eye(2, K, dtype=np.float32))])
    tr._accum = None
    tr.train_step(1e-3)
    reg = [("regularize", "grads", 0.25, "loss")] if on else []
    assert calls == ["forward_backward", "allreduce"] + reg + [("update", 0.25), "metrics"]
