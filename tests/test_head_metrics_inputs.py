"""Conditioning of the inputs of the Keras-clip head test (tests/
test_gpu_stem_head.py) and of the batch-metrics tie test (tests/
test_gpu_small_kernels.py), on the fp64 oracle alone (no GPU): the GPU tests
mean what they say only if these hold."""
import numpy as np

from helpers import CLIP_BAND, clip_case, clip_classes, metrics_case, tie_rows
from oracle import asr_oracle as O

METRIC_SHAPES = [(1, 1), (255, 2), (257, 10), (600, 17)]


def test_clip_case_is_conditioned():
    spec, params, imgs, onehot = clip_case()
    assert all(np.array_equal(p, p.astype(np.float32)) for p in params)
    probs, _ = O.net_forward(spec, params, imgs)
    low, high, unsat, clear = clip_classes(probs, onehot)
    # no renormalised q or 1 - q within a factor 10 of Keras' epsilon: fp32 and fp64 clip the same entries
    assert clear, CLIP_BAND
    assert low.any() and high.any() and unsat.any(), (low, high, unsat)
    assert np.all(low.astype(int) + high + unsat == 1), "every image in exactly one saturation class"
    # the clip gradient: a saturated image contributes nothing, an unsaturated one does
    dl = O.keras_cce_grad_logits(probs, onehot, 1.0 / len(probs))
    assert np.all(dl[low | high] == 0) and np.all(np.abs(dl[unsat]).max(axis=-1) > 1e-3)
    # the batch-mean loss is carried by the unsaturated and the low images
    per = O.keras_cce(probs, onehot)
    assert per[high].max() < 2e-7 and per[low].min() > 16.0 and O.net_loss(probs, onehot) > 1.0


def test_metrics_case_ties_are_bit_equal():
    seen = 0
    for N, K in METRIC_SHAPES:
        for call in range(3):
            p, t = metrics_case(N, K, seed=call)
            assert p.dtype == np.float32 and t.dtype == np.float32 and p.shape == t.shape == (N, K)
            assert np.all(t.sum(axis=-1) == 1)
            first = last = 0
            for r, i, j in tie_rows(N, K):
                assert i < j and p[r, i].view(np.uint32) == p[r, j].view(np.uint32)
                assert p[r, i] == p[r].max() and (p[r] == p[r, i]).sum() == 2
                assert np.argmax(p[r]) == i
                first += int(t[r, i] == 1)
                last += int(t[r, j] == 1)
                seen += 1
            if K >= 2 and N >= 12:  # a last-maximum argmax would count differently
                assert first > 0 and last > 0
            if K >= 4 and N >= 12:
                assert {(i, j) for _, i, j in tie_rows(N, K)} == {(0, 3), (2, K - 1)}
            if N >= 12:
                s = p.astype(np.float64).sum(axis=-1)
                assert (s < 0.8).any() and (s > 1.2).any()            # renormalisation matters
                assert (p < 1e-7).any() and ((p < 1e-7) & (t == 1)).any()  # the clip matters
    assert seen > 0
