"""GPU checks of the fused augmentation kernel (asr_augment_batch) against the float64 numpy
restatement of tests/augment_ref.py, on its fixed inputs and hand-built tables (the smallest shapes
at which the kernel can still go wrong: odd image sizes, 3-byte pixels at unaligned offsets, rows
that are no multiple of the 16-B store run, more runs than one workgroup, N = 1 and N = 13,
repeated and unordered rows), and end to end through ArrayDataset and Training.

Bars
  exact       crop / flip only: the kernel copies, so uint8 and float32 are bit-exact.
  lerp        resize and brightness in float32 vs the float64 restatement: atol 2e-4 on the 0..255
              scale (three lerps of one float32 rounding each at magnitude <= 255, with margin).
  saturation  the HSV round trip has no derivable bar: the float64 restatement against its own
              float32 evaluation on these inputs, the end-to-end dataset's batches included, is at
              most 1.2365e-4 (batch 4 of that dataset; tests/test_augment_cpu.py asserts that the
              measurement reproduces this figure to 1 %); the bar is four times it, 4.946e-4.
  u8 colour   uint8 results truncate, so a value next to an integer boundary may land one step off:
              every element within 1 of the restatement and at most 0.1 % of the elements differing
              (the restatement's float32 and float64 evaluations agree within that on the CPU).
"""
import numpy as np
import pytest

import augment_ref as A

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CASES = A.cases()


@pytest.fixture(scope="module")
def want():
    """The float64 restatement of every case, computed once."""
    return {name: A.augment(src, table, plan, np.float64) for name, src, plan, table, _ in CASES}


def run(src, plan, table, feats=None):
    from differential_equations_resnet_amd import runtime
    feats = torch.from_numpy(src).cuda() if feats is None else feats
    items = torch.from_numpy(table.view(np.uint8)).cuda()
    out = runtime.augment_batch(feats, plan, items)
    assert tuple(out.shape) == (len(table),) + tuple(plan.out_shape)
    assert out.dtype == (torch.uint8 if np.dtype(plan.out_dtype) == np.uint8 else torch.float32)
    return out.cpu().numpy()


def hold(got, ref, bar, name):
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    print(f"{name}: {bar}: max |diff| {d.max():.3e}, {int((d > 0).sum())} of {d.size} differ")
    if bar == A.EXACT:
        assert got.dtype == (np.uint8 if ref.dtype == np.uint8 else np.float32)
        assert np.array_equal(got, ref.astype(got.dtype)), name
    elif bar == A.LERP:
        assert d.max() <= A.LERP_ATOL, (name, d.max())
    elif bar == A.SATURATION:
        assert d.max() <= A.SAT_ATOL, (name, d.max())
    else:
        assert got.dtype == np.uint8 and d.max() <= A.U8_MAX_STEP, (name, d.max())
        assert (d > 0).mean() <= A.U8_MAX_DIFFERING, (name, int((d > 0).sum()), d.size)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_matches_the_restatement(case, want):
    name, src, plan, table, bar = case
    hold(run(src, plan, table), want[name], bar, name)


def test_launch_is_a_pure_function_of_its_table():
    """The same table twice gives the same bytes; rows of the table are independent (a permuted
    table gives the permuted batch)."""
    name, src, plan, table, _ = next(c for c in CASES if c[0] == "chain_u8_resize_bright_sat")
    a, b = run(src, plan, table), run(src, plan, table)
    assert a.tobytes() == b.tobytes()
    perm = np.random.default_rng(0).permutation(len(table))
    assert np.array_equal(run(src, plan, table[perm]), a[perm])


def test_out_of_range_table_is_clamped(want):
    """items must hold in-range values; a table that does not gets the clamped row and window (wrong
    pixels by contract): the result is the in-range table's, which is the restatement's.  The 7-row
    source is a view in the middle of one larger zero-filled allocation (rows 50..56 of 1200), so that
    an unclamped index (row -5, row 1000, a 40-row window) would still read allocated memory and show up
    as wrong values, not as an access outside an allocation."""
    name, src, plan, table, _ = next(c for c in CASES if c[0] == "crop_up_flipsrc_u8")
    arena = torch.zeros((1200,) + src.shape[1:], dtype=torch.uint8, device="cuda")
    feats = arena[50:50 + len(src)]
    feats.copy_(torch.from_numpy(src))
    assert feats.is_contiguous() and feats.data_ptr() == arena.data_ptr() + 50 * src[0].size
    bad, good = table.copy(), table.copy()
    bad["src"][0], good["src"][0] = 1000, len(src) - 1
    bad["src"][1], good["src"][1] = -5, 0
    bad["y0"][2], good["y0"][2] = 7, 1
    bad["x0"][3], good["x0"][3] = -2, 0
    bad["ch"][4], good["ch"][4] = 40, 9
    good["y0"][4] = 0                      # (the origin is clamped for the clamped size)
    bad["cw"][5], good["cw"][5] = 0, 1
    got = run(src, plan, good, feats)
    assert np.array_equal(run(src, plan, bad, feats), got)
    hold(got, A.augment(src, good, plan, np.float64), A.LERP, "clamped table")
    assert np.array_equal(run(src, plan, table, feats), run(src, plan, table))   # (the view is the array)


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def _dataset(seed=A.DS_SEED, B=A.DS_BATCH, **kw):
    """The fixed end-to-end dataset of tests/augment_ref.py (40 images of 12 x 12 x 3, the reference-style chain)."""
    from differential_equations_resnet_amd.dataset_utils import create_tf_dataset_from_arrays
    ds, _, _ = create_tf_dataset_from_arrays(A.DS_FEATS, A.DS_LABELS, B, preprocessors=A.dataset_chain(), seed=seed,
                                             num_classes=10, **kw)
    return ds, A.DS_FEATS, A.DS_LABELS


def test_dataset_batches_are_the_restatement_of_the_drawn_table():
    """ArrayDataset with the reference-style chain: every batch equals the restatement applied to the
    dataset's own table (saturation bar: the chain ends in the HSV round trip; the bar's CPU figure
    covers these batches because the dataset draws exactly the tables tests/augment_ref.py restates),
    the table's rows are the permutation's, labels follow, and the draws vary."""
    ds, feats, labels = _dataset()
    fixed = A.dataset_cases()
    assert ds.output_shapes == ((8, 16, 16, 3), (8, 10)) and ds.output_dtype == np.float32
    assert ds.aug_plan.crop == (10, 10)
    it = iter(ds)
    order = np.random.default_rng(3).permutation(40)
    seen = []
    for k in range(6):   # runs across the epoch boundary (40 images, batches of 8)
        x, y = next(it)
        t = ds.last_table.copy()
        assert t.tobytes() == fixed[k][3].tobytes()
        assert x.dtype == torch.float32 and tuple(x.shape) == (8, 16, 16, 3) and x.is_cuda
        if k < 5:
            assert np.array_equal(t["src"], order[8 * k:8 * k + 8])
        assert np.array_equal(y.cpu().numpy(), np.eye(10, dtype=np.float32)[labels[t["src"]]])
        ref = A.augment(feats, t, ds.aug_plan, np.float64)
        hold(x.cpu().numpy(), ref, A.SATURATION, f"dataset batch {k}")
        seen.append(t)
    allt = np.concatenate(seen)
    assert set(allt["flip"]) == {0, 1} and set(allt["y0"]) == {0, 1, 2} and len(set(allt["brightness"])) == 48


def test_same_seed_same_batches_and_plain_callables_still_run():
    a, _, _ = _dataset(seed=5)
    b, _, _ = _dataset(seed=5)
    c, _, _ = _dataset(seed=6)
    ia, ib, ic = iter(a), iter(b), iter(c)
    for _ in range(3):
        (xa, ya), (xb, yb), (xc, _) = next(ia), next(ib), next(ic)
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
        assert not torch.equal(xa, xc)
    # a plain callable listed after the native preprocessors runs on the augmented batch
    from differential_equations_resnet_amd.dataset_utils import ArrayDataset, RandomFlipLeftRight
    feats = np.arange(4 * 5 * 6, dtype=np.uint8).reshape(4, 5, 6, 1)
    ds = ArrayDataset(feats, np.arange(4), 4, preprocessors=[RandomFlipLeftRight(), lambda x, y: (x.float() + 1, y)],
                      shuffle=False)
    x, _ = next(iter(ds))
    t = ds.last_table
    assert x.dtype == torch.float32 and ds.output_dtype == np.uint8   # (the callable's own change is its own)
    assert np.array_equal(x.cpu().numpy(), A.augment(feats, t, ds.aug_plan).astype(np.float32) + 1)


def test_rank_slices_are_the_single_process_batch():
    """Two ranks of a world-size-2 dataset (built in one process) together yield the single-process
    batches of the global batch size, bit for bit."""
    one, _, _ = _dataset(seed=9, B=8)
    r0, _, _ = _dataset(seed=9, B=4, rank=0, world_size=2)
    r1, _, _ = _dataset(seed=9, B=4, rank=1, world_size=2)
    i1, i2, i3 = iter(one), iter(r0), iter(r1)
    for _ in range(2):
        (x, y), (x0, y0), (x1, y1) = next(i1), next(i2), next(i3)
        assert torch.equal(x, torch.cat([x0, x1])) and torch.equal(y, torch.cat([y0, y1]))


def test_training_runs_on_the_augmented_shape():
    """Two Training steps of a tiny single-stage model (C = 16, L = 2) on a 12 x 12 uint8 source
    resized to 16 x 16: the model is built at the augmented shape and takes float32 batches; loss
    and gradients are finite."""
    from differential_equations_resnet_amd import graph
    from differential_equations_resnet_amd.dataset_utils import (ConvertLabelsToOneHot, RandomBrightness, RandomCrop,
                                                                 RandomFlipLeftRight, RandomSaturation, Resize,
                                                                 create_tf_dataset_from_arrays)
    from differential_equations_resnet_amd.models import tfkeras_resnets as R
    from differential_equations_resnet_amd.training import AdamOptimizer, Training
    rng = np.random.default_rng(4)
    B, C, L = 4, 16, 2
    feats = rng.integers(0, 256, (8, 12, 12, 3), dtype=np.uint8)
    labels = rng.integers(0, 10, 8)
    pre = [RandomCrop(scale=0.9), Resize((16, 16)), RandomFlipLeftRight(), RandomBrightness(), RandomSaturation(),
           ConvertLabelsToOneHot(10)]
    ds, _, _ = create_tf_dataset_from_arrays(feats, labels, B, preprocessors=pre)
    assert ds.output_shapes == ((B, 16, 16, 3), (B, 10)) and ds.output_dtype == np.float32
    graph.set_seed(2)
    build = R.get_single_block_resnet_build_function(h=0.25, num_stages=2, blocks_per_stage=[L], filters_per_block=[C],
                                                     strides=[(1, 1)], subtract_mean=127.5, divide_by_stddev=127.5,
                                                     num_classes=10)
    tr = Training(build, "antisymmetric", AdamOptimizer(epsilon=1e-7), train_dataset=ds, record_summaries=False)
    assert (tr.native.plan.H, tr.native.plan.W) == (16, 16)
    assert tuple(tr.input_tensor.shape[-3:]) == (16, 16, 3)
    tr._reset_metrics()
    for _ in range(2):
        norms = tr.train_step(1e-3, with_norms=True)
        assert len(norms) == L + 1 and all(np.isfinite(n) and n > 0 for n in norms)
    loss, _ = tr._metric_values()
    assert np.isfinite(loss) and loss > 0
    assert not tr.native.executor(False).cfg.input_u8
    tr.close()
