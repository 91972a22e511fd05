"""GPU tests of the weight regularisers: the asr_regularize kernels against tests/reg_ref.py (fp64), the
call's contract (reproducible bits, stale workspace, side stream, HIP graph), and compile / fit /
evaluate / train_on_batch / test_on_batch and Training on a model built with l2_regularization and
smoothness_regularization against the oracle's cross-entropy and gradients plus reg_ref's R and dR.

End-to-end bars are those of tests/test_gpu_keras_api.py: trained weights 1e-5 of each tensor's max,
losses 1e-5 relative.  That file has no numeric bfloat16 bar; the bfloat16 case takes the loss bar of
tests/test_gpu_network.py's bfloat16 parity (1 % relative against the fp64 oracle) and compares the
parameters with a twin stepped without regularisers by the same executor, at the float32 weight bar
(the penalty acts on the fp32 parameters: p_reg = p_twin - lr * dR whatever the activation dtype).
"""
import ctypes as ct

import numpy as np
import pytest

import reg_ref
from oracle import asr_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from differential_equations_resnet_amd import _lib, graph, lowering, optimizers  # noqa: E402
from differential_equations_resnet_amd.graph import Input  # noqa: E402
from differential_equations_resnet_amd.models import tfkeras_resnets as R  # noqa: E402

U = 2.0 ** -24


@pytest.fixture(scope="module")
def rt():
    from differential_equations_resnet_amd import runtime
    runtime.require_gpu()
    return runtime


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the fixtures' arrays are read-only)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# --------------------------------------------------------------------------
# the kernel against reg_ref
# --------------------------------------------------------------------------
# (offset, count, layer_stride, layers, l2, smooth)
TABLE = [
    (3, 1, 1, 1, 0.3, 0.0),                 # one float
    (7, 5, 5, 1, 0.02, 0.0),                # odd offset: no 16-byte access
    (16, 6, 8, 2, 0.01, 0.4),               # two layers: one neighbour each
    (33, 8, 8, 3, 0.0, 0.25),               # three layers back to back, odd offset: the first interior layer
    (64, 8, 12, 3, 0.05, 0.25),             # the same on the 16-byte path (offset, count, stride % 4 == 0)
    (100, 1027, 1027 + 16, 4, 0.003, 0.2),  # thetas with gaps, odd count: scalar, more than one chunk per layer
    (100 + 1027, 12, 1027 + 16, 4, 0.0, 0.3),  # 'biases' in those gaps (4 floats of each stay uncovered)
    (4272, 2048, 2048 + 16, 3, 0.001, 0.1),    # a stack on the 16-byte path, two chunks per layer
    (10452, 300001, 300001, 1, 1e-4, 0.0),     # many workgroups, 16-byte body and a scalar tail
]
N_PARAMS = 10452 + 300001 + 7


@pytest.fixture(scope="module")
def case():
    """The operands and the fp64 reference, computed once and never written."""
    rng = np.random.default_rng([2024, 1])
    p = rng.standard_normal(N_PARAMS).astype(np.float32)
    g = (rng.standard_normal(N_PARAMS) * 0.1).astype(np.float32)  # the pattern grads holds before the call
    Rref, dR = reg_ref.penalty(p, TABLE)
    cov = reg_ref.covered(TABLE, N_PARAMS)
    assert 0 < (~cov).sum() and Rref > 0 and (dR[~cov] == 0).all()
    for a in (p, g, dR, cov):
        a.setflags(write=False)
    return p, g, Rref, dR, cov


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_kernel_matches_reference(rt, case, grad_scale):
    """Launch geometry: 1024-float chunks, one per workgroup pass, 256 threads of 4 floats.  R and dR are
    formed in fp64 from the fp32 operands and every partial sum (thread, LDS tree, workgroup partials) is
    fp64, so the longest chain of fp32 roundings behind R is k = 1 (the final conversion) and behind
    loss_inout 1 more; the bars are 2 * 2^-24 relative for both (the issue's 1e-4 holds a fortiori).  A
    gradient is rounded twice (dR / grad_scale to fp32, the add).  Measured on an MI355X: R relative
    error 2.3e-8, loss_inout 4.6e-8, the worst gradient at 0.43 of its bar."""
    p, g, Rref, dR, cov = case
    tab = rt.RegTable(TABLE, N_PARAMS)
    assert tab.ws_bytes == _lib.load().asr_regularize_workspace_bytes(len(TABLE), N_PARAMS) > 0
    P, G = _cuda(p), _cuda(g)
    loss0 = np.float32(1.7)
    loss, pen = _cuda(np.array([loss0], np.float32)), _cuda(np.array([np.nan], np.float32))
    tab.ws.fill_(0xFF)
    rt.regularize(tab, P, G, grad_scale, loss, pen)
    torch.cuda.synchronize()
    got = G.cpu().numpy()
    # floats in gaps and outside all segments: bitwise unchanged; the parameters are only read
    np.testing.assert_array_equal(got.view(np.uint32)[~cov], g.view(np.uint32)[~cov])
    np.testing.assert_array_equal(_bits(P), p.view(np.uint32))
    want = g.astype(np.float64) + dR / grad_scale
    bar = 4 * U * (np.abs(g.astype(np.float64)) + np.abs(dR / grad_scale))
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err[cov] / bar[cov]).max())
    print(f"grad_scale {grad_scale}: worst gradient error {worst:.3f} of its bar")
    assert (err[cov] <= bar[cov]).all(), worst
    assert np.abs(got[cov] - g[cov]).max() > 0
    r_err = abs(float(pen.item()) - Rref) / Rref
    l_err = abs(float(loss.item()) - (float(loss0) + Rref)) / (float(loss0) + Rref)
    print(f"R = {Rref:.9g}: relative error {r_err:.3e}; loss_inout relative error {l_err:.3e}")
    assert r_err <= 2 * U and r_err <= 1e-4
    assert l_err <= 2 * U


def test_forward_only_leaves_the_gradients(rt, case):
    p, g, Rref, _, _ = case
    tab = rt.RegTable(TABLE, N_PARAMS)
    P, G = _cuda(p), _cuda(g)
    pen, loss = _cuda(np.array([np.nan], np.float32)), _cuda(np.array([0.25], np.float32))
    tab.ws.fill_(0xFF)
    rt.regularize(tab, P, None, 1.0, None, pen)
    torch.cuda.synchronize()
    assert abs(float(pen.item()) - Rref) <= 2 * U * Rref
    np.testing.assert_array_equal(_bits(G), g.view(np.uint32))
    np.testing.assert_array_equal(_bits(P), p.view(np.uint32))
    assert float(loss.item()) == 0.25
    # and the same R as the call with gradients gives
    pen2 = torch.empty_like(pen)
    rt.regularize(tab, P, G, 1.0, None, pen2)
    assert _bits(pen2)[0] == _bits(pen)[0]


def _run(rt, tab, p, g, grad_scale=0.5):
    """One call on the current stream into fresh buffers: (grads, loss, penalty) tensors."""
    P, G = _cuda(p), _cuda(g)
    loss, pen = _cuda(np.array([0.5], np.float32)), _cuda(np.array([np.nan], np.float32))
    tab.ws.fill_(0xFF)
    rt.regularize(tab, P, G, grad_scale, loss, pen)
    return G, loss, pen


def test_bitwise_reproducible_on_a_side_stream_and_under_graph_replay(rt, case):
    """Two eager runs give the same bits; so does a run on a side stream and, as tests/test_gpu_streams.py's
    test_graph_replay does it, the call captured into a HIP graph (global capture error mode: a call that
    synchronised or allocated would fail the capture) and replayed twice on restored operands with the
    workspace set to 0xFF before each run."""
    p, g, _, _, _ = case
    tab = rt.RegTable(TABLE, N_PARAMS)
    first = [_bits(t).copy() for t in _run(rt, tab, p, g)]
    second = [_bits(t).copy() for t in _run(rt, tab, p, g)]
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = _run(rt, tab, p, g)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for a, t in zip(first, on_side):
        np.testing.assert_array_equal(a, _bits(t))
    # capture: fixed buffers, the operands restored before every replay
    P, G = _cuda(p), _cuda(g)
    G0 = G.clone()
    loss, pen = _cuda(np.array([0.5], np.float32)), _cuda(np.array([np.nan], np.float32))
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        rt.regularize(tab, P, G, 0.5, loss, pen)
    for n in range(2):
        G.copy_(G0)
        loss.fill_(0.5)
        pen.fill_(float("nan"))
        tab.ws.fill_(0xFF)
        gr.replay()
        torch.cuda.synchronize()
        for a, t, what in zip(first, (G, loss, pen), ("grads", "loss", "penalty")):
            np.testing.assert_array_equal(a, _bits(t), err_msg=f"replay {n + 1}: {what}")


def test_empty_table_touches_nothing(rt, case):
    p, g, _, _, _ = case
    P, G = _cuda(p), _cuda(g)
    loss = _cuda(np.array([0.5, np.nan], np.float32))
    ws = torch.full((64,), 0xFF, dtype=torch.uint8, device="cuda")
    tab = rt.RegTable([], N_PARAMS)
    assert tab.n == 0 and tab.ws_bytes == 0
    rt.regularize(tab, P, G, 1.0, loss[:1], loss[1:])
    rc = _lib.load().asr_regularize(P.data_ptr(), 0, P.data_ptr(), G.data_ptr(), ct.c_float(1.0), loss.data_ptr(),
                                    loss[1:].data_ptr(), ws.data_ptr(), 64, None)
    assert rc == _lib.ASR_OK
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(G), g.view(np.uint32))
    np.testing.assert_array_equal(_bits(P), p.view(np.uint32))
    np.testing.assert_array_equal(_bits(loss), np.array([0.5, np.nan], np.float32).view(np.uint32))
    assert (ws.cpu().numpy() == 0xFF).all()


def test_wrapper_checks_the_table_before_any_upload(rt):
    with pytest.raises(ValueError, match="segment 1"):
        rt.RegTable([(0, 4, 4, 1, 0.1, 0.0), (90, 20, 20, 1, 0.1, 0.0)], 100)
    with pytest.raises(ValueError, match="overlap"):
        rt.RegTable([(0, 4, 4, 1, 0.1, 0.0), (2, 4, 4, 1, 0.1, 0.0)], 100)
    tab = rt.RegTable([(0, 4, 4, 1, 0.1, 0.0)], 100)
    with pytest.raises(ValueError, match="params"):
        rt.regularize(tab, torch.zeros(99, device="cuda"))


# --------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------
K, LR, L2C, ALPHA, H = 10, 0.1, 0.05, 0.5, 0.5
SPEC = O.NetSpec(C=16, L=3, h=H)


def _model(l2=L2C, alpha=ALPHA, seed=2, defaults=False):
    """tests/test_gpu_keras_api.py's small model (_single), with the regularisers.  The biases, zero as
    built, get values (tests/test_gpu_network.py's bias_std): the smoothness penalty acts on them too."""
    graph.set_seed(seed)
    kw = {} if defaults else dict(l2_regularization=l2, smoothness_regularization=alpha)
    fn = R.get_single_block_resnet_build_function(h=H, num_stages=2, blocks_per_stage=[3], filters_per_block=[16],
                                                  strides=[(1, 1)], subtract_mean=127.5, divide_by_stddev=127.5,
                                                  num_classes=K, **kw)
    m = fn(Input(shape=(32, 32, 3)))
    _set_biases(m, seed)
    return m


def _set_biases(m, seed):
    rng = np.random.default_rng([seed, 77])
    for w in m.weights:
        if w.name.endswith("/bias"):
            w.assign((rng.standard_normal(w.shape) * 0.05).astype(np.float32))
    m._push()


def _data(n=8, seed=9):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (n, 32, 32, 3)).astype(np.uint8)
    labels = rng.integers(0, K, n)
    return x, optimizers.to_categorical(labels, K), labels


def _vars(m):
    return lowering.analyze(m).weight_vars()


def _flat(arrays):
    return np.concatenate([np.asarray(a, np.float64).ravel() for a in arrays])


@pytest.fixture(scope="module")
def ref():
    """The yardstick, computed once: the oracle's cross-entropy and gradients of the model's initial
    weights on the batch, reg_ref's R and dR, and the weights one SGD step on."""
    x, y, labels = _data()
    m = _model()
    plan = lowering.analyze(m)
    segs = plan.regularization_segments()
    assert len(segs) == 4  # conv1, thetas (l2 + smooth), biases (smooth), fc
    w0 = [v.value.copy() for v in plan.weight_vars()]
    p64 = [w.astype(np.float64) for w in w0]
    probs, cache = O.net_forward(SPEC, p64, x)
    ce = float(O.net_loss(probs, y.astype(np.float64)))
    g = _flat(O.net_backward(SPEC, p64, cache, y.astype(np.float64)))
    Rv, dR = reg_ref.penalty(_flat(p64), segs)
    lr = float(np.float32(LR))
    p1 = _flat(p64) - lr * (g + dR)
    shapes = [w.shape for w in w0]
    w1 = O.unflatten(p1, shapes)
    probs1, _ = O.net_forward(SPEC, w1, x)
    ce1 = float(O.net_loss(probs1, y.astype(np.float64)))
    R1, _ = reg_ref.penalty(p1, segs)
    return dict(x=x, y=y, labels=labels, w0=w0, ce=ce, R=Rv, dR=dR, g=g, w1=w1, ce1=ce1, R1=R1, lr=lr, segs=segs,
                w1_plain=O.unflatten(_flat(p64) - lr * g, shapes))


def _rel(got, want, what, bar=1e-5):
    print(f"{what}: got {got!r} want {want!r} rel {abs(got - want) / abs(want):.3e}")
    assert abs(got - want) <= bar * abs(want), what


def _weights(m, want, bar=1e-5):
    m._native.mark_updated()
    m.get_weights()  # (pulls the device parameters into the variables)
    got = [v.value for v in _vars(m)]
    assert len(got) == len(want)
    worst = 0.0
    for i, (a, b) in enumerate(zip(got, want)):
        err = np.abs(a.astype(np.float64) - b).max()
        worst = max(worst, err / np.abs(b).max())
        assert err <= bar * np.abs(b).max(), (i, b.shape, err, np.abs(b).max())
    print(f"weights: worst max err / max |w| over {len(want)} tensors {worst:.3e} (bar {bar:.0e})")


def test_the_penalty_is_far_above_the_bars(ref):
    """A step that dropped the penalty cannot pass: R is at least 10 x the loss bar, and lr * max|dR| of
    every regularised tensor at least 10 x that tensor's weight bar."""
    assert ref["R"] >= 10 * 1e-5 * (ref["ce"] + ref["R"])
    assert ref["R"] >= 10 * 1e-2 * (ref["ce"] + ref["R"])  # the bfloat16 loss bar too
    cov = reg_ref.covered(ref["segs"], ref["dR"].size)
    off = hit = 0
    for w in ref["w1"]:
        sl = slice(off, off + w.size)
        off += w.size
        assert cov[sl].all() or not cov[sl].any()
        if cov[sl].any():  # conv1's and fc's kernels, every block's thetas and bias
            hit += 1
            assert ref["lr"] * np.abs(ref["dR"][sl]).max() >= 10 * 1e-5 * np.abs(w).max()
    assert hit == len(ref["w1"]) - 2  # all but conv1's and fc's bias
    print(f"CE {ref['ce']:.6f}, R {ref['R']:.6f}, lr*max|dR| {ref['lr'] * np.abs(ref['dR']).max():.3e}")


def test_train_on_batch_trains_the_keras_objective(ref):
    x, y = ref["x"], ref["y"]
    m = _model()
    m.compile(optimizers.SGD(lr=LR), metrics=["accuracy"], dtype="float32")
    want = ref["ce"] + ref["R"]
    _rel(m.test_on_batch(x, y)[0], want, "test_on_batch loss")
    _rel(m.evaluate(x, y, batch_size=3, verbose=0)[0], want, "evaluate loss (batches 3, 3, 2)")
    l2_only = [s[:5] + (0.0,) for s in ref["segs"] if s[4] > 0]
    _rel(sum(m.losses), reg_ref.penalty(_flat(ref["w0"]), l2_only)[0], "sum(model.losses): the l2 terms", bar=1e-6)
    loss, _ = m.train_on_batch(x, y)
    _rel(loss, want, "train_on_batch loss")
    _weights(m, ref["w1"])
    _rel(m.test_on_batch(x, y)[0], ref["ce1"] + ref["R1"], "test_on_batch loss after the step")


def test_fit_history_includes_the_penalty(ref):
    x, y = ref["x"], ref["y"]
    m = _model()
    m.compile(optimizers.SGD(lr=LR), dtype="float32")
    h = m.fit(x, y, batch_size=8, epochs=1, shuffle=False, validation_data=(x, y), verbose=0)
    _rel(h.history["loss"][0], ref["ce"] + ref["R"], "history loss")
    _rel(h.history["val_loss"][0], ref["ce1"] + ref["R1"], "history val_loss")
    _weights(m, ref["w1"])


def test_zero_coefficients_are_the_default_step_bitwise(ref):
    x, y = ref["x"], ref["y"]
    out = []
    for defaults in (False, True):
        m = _model(l2=0.0, alpha=0.0, defaults=defaults)
        m.compile(optimizers.SGD(lr=LR), dtype="float32")
        loss = m.train_on_batch(x, y)
        assert m._native.regularizer() is None
        out.append((loss, m._native.params.cpu().numpy().view(np.uint32)))
    assert out[0][0] == out[1][0]
    np.testing.assert_array_equal(out[0][1], out[1][1])
    _rel(out[0][0], ref["ce"], "the loss without regularisers")
    _weights(m, ref["w1_plain"])


def _training(ref, **kw):
    from differential_equations_resnet_amd.dataset_utils import ArrayDataset
    from differential_equations_resnet_amd.training import Training
    ds = ArrayDataset(ref["x"], ref["labels"], 8, shuffle=False, num_classes=K)
    graph.set_seed(2)
    build = R.get_single_block_resnet_build_function(h=H, num_stages=2, blocks_per_stage=[3], filters_per_block=[16],
                                                     strides=[(1, 1)], subtract_mean=127.5, divide_by_stddev=127.5,
                                                     num_classes=K, l2_regularization=L2C,
                                                     smoothness_regularization=ALPHA)
    tr = Training(build, "antisymmetric", optimizers.SGD(lr=123.0), train_dataset=ds, record_summaries=False,
                  dtype="float32", **kw)
    _set_biases(tr.model, 2)
    for a, b in zip([v.value for v in tr.native.plan.weight_vars()], ref["w0"]):
        np.testing.assert_array_equal(a, b)  # the same seed: the yardstick's weights
    return tr


def test_training_adds_the_penalty_only_when_asked(ref):
    tr = _training(ref, regularization_losses=True)
    tr.train_step(LR)
    _rel(tr._metric_values()[0], ref["ce"] + ref["R"], "Training(regularization_losses=True) mean_loss")
    _weights(tr.model, ref["w1"])
    got = tr.evaluate("train", 1)["mean_loss"]
    _rel(got, ref["ce1"] + ref["R1"], "Training.evaluate mean_loss")
    tr.close()
    tr = _training(ref)
    assert tr.regularization_losses is False
    tr.train_step(LR)
    _rel(tr._metric_values()[0], ref["ce"], "Training default mean_loss: the cross-entropy alone")
    _weights(tr.model, ref["w1_plain"])
    tr.close()


def test_bfloat16_step(ref):
    """bfloat16 activations: the loss within 1 % of the fp64 oracle's CE + R (tests/test_gpu_network.py's
    bfloat16 loss bar; R is asserted above to be 10 x that), and the parameters against a twin without
    regularisers stepped by the same bfloat16 executor: p_reg = p_twin - lr * dR at the float32 weight
    bar, the loss difference R at 1e-5 of the loss."""
    x, y = ref["x"], ref["y"]
    m, twin = _model(), _model(defaults=True)
    losses = []
    for mm in (m, twin):
        mm.compile(optimizers.SGD(lr=LR), dtype="bfloat16")
        losses.append(mm.train_on_batch(x, y))
        assert mm._native.resolve_dtype("bfloat16") == "bfloat16"
    _rel(losses[0], ref["ce"] + ref["R"], "bfloat16 train_on_batch loss", bar=1e-2)
    print(f"loss difference {losses[0] - losses[1]!r}, R {ref['R']!r}")
    assert abs((losses[0] - losses[1]) - ref["R"]) <= 1e-5 * abs(losses[0])
    twin._native.mark_updated()
    twin.get_weights()
    p_twin = _flat([v.value for v in _vars(twin)])
    want = O.unflatten(p_twin - ref["lr"] * ref["dR"], [w.shape for w in ref["w0"]])
    _weights(m, want)
