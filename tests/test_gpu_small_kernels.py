"""GPU parity of the small kernels -- k_adam (asr_optim.hip), k_segment_sq_norms,
k_batch_metrics (asr_api.hip) -- against numpy fp64, each called directly through runtime.

Tolerances: Adam rtol 1e-6 + atol 1e-7 (tests/test_gpu_kernels.py) on the
parameters and both moments; segment norms rtol 1e-5 (the bar of
test_training_metrics_match_oracle; at 20000 elements the fp32 worst case is
about (20000/256 + 10) * 2^-24 = 5e-6); the metrics' loss 1e-5 relative, their
counts exact.
"""
import numpy as np
import pytest

from helpers import assert_close, metrics_case, tie_rows
from oracle import asr_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# the ABI takes the hyper-parameters as floats: the fp64 reference gets the values the kernel gets
# (1 - float(0.999) is 1.3e-5 off 1 - 0.999: a hyper-parameter's rounding, not the kernel's arithmetic)
ADAM = {k: float(np.float32(v)) for k, v in dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7).items()}


@pytest.fixture(scope="module")
def rt():
    from differential_equations_resnet_amd import runtime
    runtime.require_gpu()
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _adam_check(rt, p, g, m, v, steps, grad_scale):
    """Apply `steps` (1-based step counts, one fresh gradient each) on the GPU
    and in fp64 from the same fp32 state; compare p, m and v."""
    ps, ms, vs = [p.astype(np.float64)], [m.astype(np.float64)], [v.astype(np.float64)]
    P, M, V = _cuda(p), _cuda(m), _cuda(v)
    for t, gt in zip(steps, g):
        rt.adam_update(P, _cuda(gt), M, V, ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"], t, grad_scale)
        O.adam_tf1(ps, [gt.astype(np.float64) * grad_scale], ms, vs, t, **ADAM)
    for name, got, want in (("p", P, ps[0]), ("m", M, ms[0]), ("v", V, vs[0])):
        assert_close(got.cpu().numpy(), want, rtol=1e-6, atol=1e-7, what=f"adam {name}")


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("n", [1, 4096 * 256 + 300])  # the grid is capped at 4096 x 256 threads: the loop wraps
def test_adam_first_steps(rt, n, grad_scale):
    rng = np.random.default_rng(n % 1000)
    p = rng.standard_normal(n).astype(np.float32)
    g = [rng.standard_normal(n).astype(np.float32) for _ in range(2)]
    _adam_check(rt, p, g, np.zeros(n, np.float32), np.zeros(n, np.float32), [1, 2], grad_scale)


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("n", [1, 4096 * 256 + 300])
def test_adam_step_10000(rt, n, grad_scale):
    """One step at t = 10000 from a random moment state (lr_t = lr to 2e-5)."""
    rng = np.random.default_rng(n % 1000 + 1)
    p = rng.standard_normal(n).astype(np.float32)
    m = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v = rng.uniform(1e-3, 1.0, n).astype(np.float32)
    _adam_check(rt, p, [rng.standard_normal(n).astype(np.float32)], m, v, [10000], grad_scale)


def test_adam_empty_and_step_zero(rt):
    from differential_equations_resnet_amd import _lib
    rng = np.random.default_rng(0)
    a = [rng.standard_normal(8).astype(np.float32) for _ in range(4)]
    P, G, M, V = (_cuda(x) for x in a)
    # n = 0 (on live buffers: an empty tensor has no address): ASR_OK, nothing written
    _lib.call("asr_adam_update", P.data_ptr(), G.data_ptr(), M.data_ptr(), V.data_ptr(), 0, 1e-3, 0.9, 0.999, 1e-7, 1,
              1.0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for t, x in zip((P, G, M, V), a):
        np.testing.assert_array_equal(t.cpu().numpy(), x)
    with pytest.raises(ValueError, match="asr_adam_update"):
        rt.adam_update(P, G, M, V, 1e-3, 0.9, 0.999, 1e-7, 0)
    torch.cuda.synchronize()
    for t, x in zip((P, G, M, V), a):
        np.testing.assert_array_equal(t.cpu().numpy(), x)


SENTINEL = np.float32(1e6)


def test_segment_sq_norms(rt):
    """One call: segments of 0 .. 20000 elements at unaligned offsets inside a
    longer buffer.  A run of sentinels (1e6: 1e12 squared) lies before, between
    and after them; the runs between are segments of the call themselves (the
    offsets are consecutive), so one element taken from a neighbour shows in
    both."""
    rng = np.random.default_rng(0)
    lengths = [0, 1, 63, 255, 256, 257, 20000]
    gaps = [3, 1, 5, 1, 2, 7, 1, 9]  # before each segment, and after the last
    x = np.full(sum(lengths) + sum(gaps), SENTINEL, np.float32)
    off, data, pos = [gaps[0]], [], gaps[0]
    for i, n in enumerate(lengths):
        x[pos:pos + n] = rng.standard_normal(n).astype(np.float32)
        data.append(len(off) - 1)  # index of this data segment in the call
        pos += n
        off.append(pos)
        if i + 1 < len(lengths):
            pos += gaps[i + 1]
            off.append(pos)
    assert pos + gaps[-1] == x.size and any(off[i] % 4 for i in data)
    off = np.array(off, np.int64)
    got = rt.segment_sq_norms(_cuda(x), _cuda(off)).cpu().numpy()
    want = np.array([(x[a:b].astype(np.float64) ** 2).sum() for a, b in zip(off[:-1], off[1:])])
    assert got.shape == want.shape == (2 * len(lengths) - 1,)
    assert got[data[0]] == 0.0 and lengths[0] == 0  # the empty segment: exactly 0
    assert want[data].max() < 1e5  # (no sentinel in a data segment)
    assert_close(got, want, rtol=1e-5, what="segment norms")


def test_segment_sq_norms_no_segments(rt):
    from differential_equations_resnet_amd import _lib
    x, off = _cuda(np.ones(4, np.float32)), _cuda(np.array([2], np.int64))
    assert rt.segment_sq_norms(x, off).numel() == 0
    out = _cuda(np.full(2, 7.0, np.float32))  # the ABI itself: ASR_OK, out untouched
    _lib.call("asr_segment_sq_norms", x.data_ptr(), off.data_ptr(), 0, out.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), [7.0, 7.0])


@pytest.mark.parametrize("with_loss", [True, False], ids=["loss-given", "loss-from-probs"])
@pytest.mark.parametrize("N,K", [(1, 1), (255, 2), (257, 10), (600, 17)])
def test_batch_metrics(rt, N, K, with_loss):
    accum = torch.zeros(4, device="cuda")
    want = np.zeros(4)
    ties = 0
    for call in range(3):
        p, t = metrics_case(N, K, seed=call)
        ties += len(tie_rows(N, K))
        p64 = p.astype(np.float64)
        loss_np = np.float32(0.25 + call) if with_loss else None
        rt.batch_metrics(_cuda(p), _cuda(t), _cuda(np.array([loss_np])) if with_loss else None, accum)
        want += [float(loss_np) if with_loss else O.keras_cce(p64, t.astype(np.float64)).mean(),
                 (np.argmax(p, axis=-1) == np.argmax(t, axis=-1)).sum(), N, 1]
    assert ties > 0 or K == 1
    got = accum.cpu().numpy().astype(np.float64)
    print(f"accum {got} want {want}")
    np.testing.assert_array_equal(got[1:], want[1:])
    assert abs(got[0] - want[0]) <= 1e-5 * abs(want[0])
