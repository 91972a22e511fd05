"""CPU checks of the device-side augmentation (no GPU needed): the compile step of the mirrored
preprocessor module (output shape / dtype, every refusal of the grammar by its message), the host
draws, the host-side argument checks of asr_augment_batch, and the numpy restatement
(tests/augment_ref.py) checked against itself -- which also establishes that the fixed inputs of
tests/test_augment_gpu.py are fit for its bars."""
import ctypes as ct

import numpy as np
import pytest

import augment_ref as A
from differential_equations_resnet_amd import _lib
from differential_equations_resnet_amd.dataset_utils import (ArrayDataset, ConvertLabelsToOneHot, DecodeImages,
                                                             DecodeJPEGImages, RandomBrightness, RandomCrop,
                                                             RandomFlipLeftRight, RandomSaturation, Resize,
                                                             ResizeWithPad, UnpackImagesLabels,
                                                             compile_preprocessors, create_tf_dataset_from_arrays)
from differential_equations_resnet_amd.dataset_utils import tf_dataset_preprocessors_image_classification as pp


def chain():
    return [RandomCrop(scale=0.9), Resize((32, 32)), RandomFlipLeftRight(), RandomBrightness(), RandomSaturation()]


# ---------------------------------------------------------------------------
# plan compilation
# ---------------------------------------------------------------------------
def test_reference_chain_compiles():
    p = compile_preprocessors(chain(), (32, 32, 3), np.uint8)
    assert p.crop == (28, 28) and p.random_crop
    assert p.out_shape == (32, 32, 3) and p.out_dtype == np.float32
    assert p.resize == pp.RESIZE_BILINEAR and p.flip and not p.flip_src
    assert p.color == [pp.COLOR_BRIGHTNESS, pp.COLOR_SATURATION]
    assert (p.max_delta, p.lower, p.upper) == (0.5, 0.5, 1.5)
    q = compile_preprocessors(chain(), (9, 11, 3), np.uint8)
    assert q.crop == (8, 8) and q.out_shape == (32, 32, 3) and q.out_dtype == np.float32
    # the reference's side: int(float32(min(H, W)) * float32(scale))
    assert RandomCrop(scale=0.9).side(32, 32) == 28 and RandomCrop(scale=0.9).side(9, 11) == 8
    assert RandomCrop(scale=1.0).side(9, 11) == 9 and RandomCrop(scale=0.5).side(224, 256) == 112


def test_constructor_signatures_are_the_references():
    assert RandomCrop(1, 0.9, 3, None).scale == 0.9 and RandomCrop().channels == 3
    assert Resize((4, 5), False, 2).target_size == (4, 5) and not Resize((4, 5)).preserve_aspect_ratio
    assert ResizeWithPad((4, 5), 2).target_size == (4, 5)
    assert RandomFlipLeftRight(4).num_parallel_calls == 4
    assert RandomBrightness().max_delta == 0.5 and RandomBrightness(0.1, 3).max_delta == 0.1
    assert (RandomSaturation().lower, RandomSaturation().upper) == (0.5, 1.5)
    assert ConvertLabelsToOneHot(10, 2).num_classes == 10


def test_output_dtype_rule():
    """uint8 when the source is uint8 and no resize ran (an identity Resize is none), float32 otherwise."""
    p = compile_preprocessors([RandomCrop(scale=0.9), RandomFlipLeftRight(), RandomBrightness()], (9, 11, 3), np.uint8)
    assert p.out_shape == (8, 8, 3) and p.out_dtype == np.uint8 and p.resize == pp.RESIZE_NONE
    p = compile_preprocessors([RandomCrop(scale=0.9), Resize((8, 8))], (9, 11, 3), np.uint8)
    assert p.resize == pp.RESIZE_NONE and p.out_dtype == np.uint8 and p.out_shape == (8, 8, 3)
    p = compile_preprocessors([Resize((8, 8))], (9, 11, 3), np.uint8)
    assert p.resize == pp.RESIZE_BILINEAR and p.out_dtype == np.float32 and p.crop == (9, 11) and not p.random_crop
    p = compile_preprocessors([RandomFlipLeftRight()], (5, 6, 1), np.float32)
    assert p.out_dtype == np.float32 and p.out_shape == (5, 6, 1)


def test_resize_with_pad_extent():
    """ratio = max(w / tw, h / th), extent floor(h / ratio) x floor(w / ratio), pad floor((t - r) / 2)."""
    p = compile_preprocessors([ResizeWithPad((12, 16))], (9, 11, 3), np.uint8)
    assert (p.resize, p.resized, p.pad, p.out_shape) == (pp.RESIZE_PAD, (12, 14), (0, 1), (12, 16, 3))
    p = compile_preprocessors([RandomCrop(scale=0.9), ResizeWithPad((16, 10))], (9, 11, 3), np.float32)
    assert (p.resize, p.resized, p.pad, p.out_shape) == (pp.RESIZE_PAD, (10, 10), (3, 0), (16, 10, 3))
    assert p.out_dtype == np.float32
    p = compile_preprocessors([ResizeWithPad((224, 224))], (200, 256, 3), np.uint8)
    assert p.resized == (175, 224) and p.pad == (24, 0)
    # the extent is exact integer arithmetic: floor(h * tw / w) where the width binds, and the binding side
    # fills the target (a double-precision w / (w / tw) rounds below tw at these sizes and would lose a pixel)
    p = compile_preprocessors([ResizeWithPad((93, 93))], (1, 1, 3), np.float32)
    assert p.resized == (93, 93) and p.pad == (0, 0)
    p = compile_preprocessors([ResizeWithPad((224, 224))], (100, 300, 3), np.uint8)
    assert p.resized == (74, 224) and p.pad == (75, 0)
    p = compile_preprocessors([ResizeWithPad((49, 98))], (3, 7, 3), np.uint8)
    assert p.resized == (42, 98) and p.pad == (3, 0)
    for h, w, th, tw in ((1, 1, 93, 93), (3, 7, 49, 98), (5, 3, 41, 7), (200, 256, 224, 224), (9, 11, 12, 16)):
        p = compile_preprocessors([ResizeWithPad((th, tw))], (h, w, 3), np.float32)
        rh, rw = (th, w * th // h) if h * tw >= w * th else (h * tw // w, tw)
        assert (p.resized if p.resize else (h, w)) == (rh, rw), (h, w, th, tw)
    # the window already has the target size: nothing runs
    p = compile_preprocessors([ResizeWithPad((9, 11))], (9, 11, 3), np.uint8)
    assert p.resize == pp.RESIZE_NONE and p.out_dtype == np.uint8


def test_flip_may_stand_anywhere():
    for pos in range(4):
        c = [RandomCrop(scale=0.9), Resize((12, 16)), RandomBrightness()]
        c.insert(pos, RandomFlipLeftRight())
        p = compile_preprocessors(c, (9, 11, 3), np.uint8)
        assert p.flip and p.flip_src == (pos < 2) and p.out_shape == (12, 16, 3)
    # colour operations in either order
    p = compile_preprocessors([Resize((12, 16)), RandomSaturation(), RandomBrightness()], (9, 11, 3), np.uint8)
    assert p.color == [pp.COLOR_SATURATION, pp.COLOR_BRIGHTNESS]


@pytest.mark.parametrize("build,match", [
    (lambda: [RandomFlipLeftRight(), RandomFlipLeftRight()], "RandomFlipLeftRight: listed twice"),
    (lambda: [RandomCrop(), Resize((8, 8)), RandomCrop()], "RandomCrop: listed twice"),
    (lambda: [Resize((8, 8)), RandomCrop()], "RandomCrop: must come before Resize"),
    (lambda: [ResizeWithPad((8, 8)), RandomCrop()], "RandomCrop: must come before ResizeWithPad"),
    (lambda: [Resize((8, 8)), ResizeWithPad((8, 8))], "at most one of Resize and ResizeWithPad"),
    (lambda: [Resize((8, 8), preserve_aspect_ratio=True)], "Resize: preserve_aspect_ratio=True would give 7 x 8"),
    (lambda: [RandomBrightness(), Resize((8, 8))], "RandomBrightness: colour operations come after Resize"),
    (lambda: [RandomSaturation(), ResizeWithPad((8, 8))], "RandomSaturation: colour operations come after ResizeWith"),
    (lambda: [ResizeWithPad((12, 11))], "ResizeWithPad: padding a uint8 9 x 11 window to 12 x 11 without resizing"),
    (lambda: [lambda x, y: (x, y)], "not a preprocessor of this module"),
])
def test_grammar_refusals(build, match):
    with pytest.raises(_lib.AsrUnsupported, match=match):
        compile_preprocessors(build(), (9, 11, 3), np.uint8)


def test_other_refusals():
    with pytest.raises(_lib.AsrUnsupported, match="RandomSaturation: needs 3 channels, the images have 1"):
        compile_preprocessors([RandomSaturation()], (5, 6, 1), np.uint8)
    with pytest.raises(_lib.AsrUnsupported, match="2 image channels"):
        compile_preprocessors([RandomFlipLeftRight()], (5, 6, 2), np.uint8)
    with pytest.raises(_lib.AsrUnsupported, match="image dtype float64"):
        compile_preprocessors([RandomFlipLeftRight()], (5, 6, 3), np.float64)
    with pytest.raises(ValueError, match="RandomCrop: scale 1.5"):
        compile_preprocessors([RandomCrop(scale=1.5)], (9, 11, 3), np.uint8)
    with pytest.raises(ValueError, match="max_delta must be non-negative"):
        compile_preprocessors([RandomBrightness(-1)], (9, 11, 3), np.uint8)
    with pytest.raises(ValueError, match="0 <= lower < upper"):
        compile_preprocessors([RandomSaturation(1.5, 0.5)], (9, 11, 3), np.uint8)
    # preserve_aspect_ratio=True is accepted where it gives the same size
    p = compile_preprocessors([RandomCrop(), Resize((16, 16), preserve_aspect_ratio=True)], (9, 11, 3), np.uint8)
    assert p.out_shape == (16, 16, 3)


@pytest.mark.parametrize("cls", [UnpackImagesLabels, DecodeImages, DecodeJPEGImages])
def test_tfrecord_and_jpeg_input_is_out_of_scope(cls):
    with pytest.raises(_lib.AsrUnsupported, match="TFRecord/JPEG input is out of scope"):
        cls()
    with pytest.raises(_lib.AsrUnsupported, match=cls.__name__):
        cls(num_parallel_calls=4)


# ---------------------------------------------------------------------------
# the dataset, as far as it goes without a GPU
# ---------------------------------------------------------------------------
def _arrays(n=8):
    rng = np.random.default_rng(0)
    return rng.integers(0, 256, (n, 9, 11, 3), dtype=np.uint8), rng.integers(0, 4, n)


def test_dataset_refusals_on_a_cpu_device():
    import torch
    from differential_equations_resnet_amd import runtime
    f, l = _arrays()
    cpu = torch.device("cpu")
    with pytest.raises(_lib.AsrUnsupported, match="RandomFlipLeftRight: listed after a plain callable"):
        ArrayDataset(f, l, 4, preprocessors=[RandomCrop(), lambda x, y: (x, y), RandomFlipLeftRight()], device=cpu)
    with pytest.raises(_lib.AsrError) as e:
        ArrayDataset(f, l, 4, preprocessors=chain(), device=cpu)
    assert str(e.value) == runtime.NO_GPU
    if not torch.cuda.is_available():
        with pytest.raises(_lib.AsrError) as e2:
            runtime.require_gpu()
        assert str(e2.value) == str(e.value)


def test_one_hot_preprocessor_sets_num_classes_and_launches_nothing():
    import torch
    f, l = _arrays()
    ds, _, _ = create_tf_dataset_from_arrays(f, l, 4, preprocessors=[ConvertLabelsToOneHot(7)], shuffle=False,
                                             device=torch.device("cpu"))
    assert ds.aug_plan is None and ds.output_shapes == ((4, 9, 11, 3), (4, 7)) and ds.output_dtype == np.uint8
    x, y = next(iter(ds))
    assert np.array_equal(x.numpy(), f[:4]) and np.array_equal(y.numpy(), np.eye(7, dtype=np.float32)[l[:4]])


# ---------------------------------------------------------------------------
# draws
# ---------------------------------------------------------------------------
def test_draws_stay_in_range_and_hit_both_extremes():
    p = compile_preprocessors(chain(), (9, 11, 3), np.uint8)
    t = p.draw(np.random.default_rng(3), 4000)
    assert t.dtype == pp.ITEM_DTYPE and t.dtype.itemsize == ct.sizeof(_lib.AugItem) == 32
    assert [n for n, _ in _lib.AugItem._fields_] == list(pp.ITEM_DTYPE.names)
    assert np.all(t["src"] == 0) and np.all(t["ch"] == 8) and np.all(t["cw"] == 8)
    assert set(np.unique(t["y0"])) == {0, 1} and set(np.unique(t["x0"])) == {0, 1, 2, 3}
    assert set(np.unique(t["flip"])) == {0, 1} and 0.45 < t["flip"].mean() < 0.55
    assert t["brightness"].min() >= -0.5 and t["brightness"].max() < 0.5 and t["brightness"].min() < -0.45
    assert t["saturation"].min() >= 0.5 and t["saturation"].max() < 1.5 and t["saturation"].max() > 1.45
    # operations that are not in the chain draw nothing and keep their neutral values
    q = compile_preprocessors([Resize((4, 4))], (9, 11, 3), np.uint8)
    u = q.draw(np.random.default_rng(3), 5)
    assert np.all(u["y0"] == 0) and np.all(u["x0"] == 0) and np.all(u["ch"] == 9) and np.all(u["cw"] == 11)
    assert np.all(u["flip"] == 0) and np.all(u["brightness"] == 0) and np.all(u["saturation"] == 1)


def test_same_seed_same_table_and_rank_slices():
    p = compile_preprocessors(chain(), (32, 32, 3), np.uint8)
    a, b = p.draw(np.random.default_rng(11), 16), p.draw(np.random.default_rng(11), 16)
    assert a.tobytes() == b.tobytes()
    assert a.tobytes() != p.draw(np.random.default_rng(12), 16).tobytes()
    # every rank of a world-size-2 run draws the global table and takes its slice: together they are
    # the single-process table
    B = 8
    ranks = [p.draw(np.random.default_rng(11), 2 * B)[r * B:(r + 1) * B] for r in range(2)]
    assert np.concatenate(ranks).tobytes() == a.tobytes()


# ---------------------------------------------------------------------------
# the C ABI's host checks (no launch: the pointers are never dereferenced)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return _lib.load(build_if_missing=True)


def _cfg(Hs=9, Ws=11, C=3, sdt=_lib.ASR_U8, Ho=8, Wo=8, ddt=_lib.ASR_U8, resize=0, rh=0, rw=0, pt=0, pl=0, fs=0,
         color=(0, 0)):
    return _lib.AugPlanConfig(Hs, Ws, C, sdt, Ho, Wo, ddt, resize, rh, rw, pt, pl, fs, (ct.c_int * 2)(*color))


def test_abi_argument_checks(lib):
    p = ct.c_void_p(256)
    F, U = _lib.ASR_F32, _lib.ASR_U8

    def call(cfg=None, src=p, items=p, dst=p, N=4, n_src=7, **kw):
        cfg = cfg if cfg is not None else _cfg(**kw)
        return lib.asr_augment_batch(src, n_src, ct.byref(cfg), items, N, dst, None)

    assert lib.asr_augment_batch(p, 7, None, p, 4, p, None) == _lib.ASR_E_ARG
    for rc in (call(src=None), call(items=None), call(dst=None), call(N=0), call(N=-3), call(n_src=0),
               call(Hs=0), call(Wo=0),
               call(Ho=10), call(Wo=12),                                  # a window outside the source
               call(resize=3), call(resize=-1),
               call(color=(3, 0)), call(color=(1, 1)), call(color=(2, 2)),
               call(ddt=F),                                               # uint8 without a resize writes uint8
               call(resize=1, Ho=12, Wo=16),                              # (dst_dtype uint8) a resize writes float32
               call(sdt=F, ddt=U),
               call(resize=2, ddt=F, Ho=12, Wo=16, rh=12, rw=14, pt=0, pl=3),   # extent outside the output
               call(resize=2, ddt=F, Ho=12, Wo=16, rh=13, rw=14),
               call(resize=2, ddt=F, Ho=12, Wo=16, rh=0, rw=14),
               call(resize=2, ddt=F, Ho=12, Wo=16, rh=12, rw=14, pt=-1),
               call(dst=ct.c_void_p(264)), call(sdt=F, ddt=F, src=ct.c_void_p(258))):
        assert rc == _lib.ASR_E_ARG, lib.asr_last_error()
        assert b"asr_augment_batch" in lib.asr_last_error()
    for kw, names in ((dict(C=2), "2 channels"), (dict(C=4), "4 channels"), (dict(C=0), "0 channels"),
                      (dict(C=1, color=(2, 0)), "saturation on 1 channel"),
                      (dict(C=1, color=(1, 2)), "saturation on 1 channel"),
                      (dict(sdt=1), "source dtype 1"), (dict(sdt=7), "source dtype 7"), (dict(ddt=5), "output dtype 5"),
                      (dict(N=1 << 20, Hs=64, Ws=64, Ho=64, Wo=64), "4294967296 output pixels")):
        assert call(**kw) == _lib.ASR_E_UNSUPPORTED, kw
        assert names in lib.asr_last_error().decode(), lib.asr_last_error()


# ---------------------------------------------------------------------------
# the restatement against itself, and the fixed inputs against the GPU test's bars
# ---------------------------------------------------------------------------
def test_restatement_identities():
    rng = np.random.default_rng(5)
    img = rng.uniform(0, 255, (9, 11, 3)).astype(np.float32)
    for ft in (np.float32, np.float64):
        assert np.array_equal(A.resize_bilinear(img.astype(ft), 9, 11, ft), img.astype(ft))   # identity resize
        const = np.full((5, 6, 3), 37.25, ft)
        assert np.array_equal(A.resize_bilinear(const, 10, 12, ft), np.full((10, 12, 3), 37.25, ft))
        # legacy coordinates: a 2x upscale reads d / 2; the last output repeats the edge
        ramp = np.arange(4, dtype=ft).reshape(1, 4, 1)
        assert np.array_equal(A.resize_bilinear(ramp, 1, 8, ft).ravel(), [0, .5, 1, 1.5, 2, 2.5, 3, 3])
    # saturation with factor 1 is the identity within rounding
    unit = rng.uniform(0, 1, (64, 64, 3))
    assert np.abs(A.adjust_saturation(unit, 1.0, np.float64) - unit).max() < 1e-14
    assert np.abs(A.adjust_saturation(unit, 1.0, np.float32) - unit).max() < 1e-6
    # factor 0 gives grey at the value (max) channel; a grey pixel stays
    assert np.allclose(A.adjust_saturation(unit, 0.0), unit.max(-1, keepdims=True).repeat(3, -1), atol=1e-15)
    grey = np.full((2, 2, 3), 0.3)
    assert np.array_equal(A.adjust_saturation(grey, 1.7), grey)
    # the uint8 round trip is the identity
    u = np.arange(256, dtype=np.uint8)
    for ft in (np.float32, np.float64):
        assert np.array_equal(A.quant_u8(A.to_unit(u, ft), ft), u)


def test_flip_twice_is_the_identity():
    for name, src, plan, table, bar in A.cases():
        if bar != A.EXACT:
            continue
        once = A.augment(src, table, plan)
        t2 = table.copy()
        t2["flip"] = 1 - t2["flip"]
        other = A.augment(src, t2, plan)
        assert np.array_equal(other[:, :, ::-1], once), name
        assert once.dtype == (np.uint8 if src.dtype == np.uint8 else np.float64)


def test_tables_hit_every_path():
    by = {name: (src, plan, table) for name, src, plan, table, _ in A.cases()}
    src, plan, t = by["crop_flip_u8_n13"]
    assert len(t) == 13 and len(by["crop_flip_u8_n1"][2]) == 1
    assert {0, 1} <= set(t["y0"]) and {0, 3} <= set(t["x0"]) and set(t["flip"]) == {0, 1}   # offset 0 and the maximum
    assert len(set(t["src"])) < 13 and list(t["src"]) != sorted(t["src"])                 # repeated, out of order
    # (0, 0) and (max, max) occur as pairs too
    assert (0, 0) in set(zip(t["y0"], t["x0"])) and (1, 3) in set(zip(t["y0"], t["x0"]))
    assert by["pad_width_u8"][1].pad == (0, 1) and by["pad_height_u8"][1].pad == (3, 0)
    # the hand-written extents are what the compile step gives
    assert compile_preprocessors([ResizeWithPad((12, 16))], (9, 11, 3), np.uint8).resized == (12, 14)
    assert compile_preprocessors([RandomCrop(), ResizeWithPad((16, 10))], (9, 11, 3), np.uint8).resized == (10, 10)
    # odd sizes: 3-byte pixels of 9 x 11 images start at odd byte offsets; the wide rows leave a tail
    assert (9 * 11 * 3) % 2 == 1
    assert (13 * 46) % 4 and (13 * 46) % 16 and (13 * 13 * 46) % 4 and (13 * 13 * 46) % 16
    # more 4-pixel runs than one 256-thread workgroup takes in one pass
    assert 13 * 13 * 46 // 4 > 256 and 13 * 12 * 16 // 4 > 256


def test_fixed_inputs_are_fit_for_the_gpu_bars():
    """The restatement's own float32 evaluation against its float64 one, on the inputs of the GPU
    test: inside the lerp bar; the saturation figure the GPU bar is four times of; and the uint8
    colour results within one step with at most 0.1 % of the elements differing."""
    worst_sat, worst_name = 0.0, None
    for name, src, plan, table, bar in A.cases():
        a, b = A.augment(src, table, plan, np.float64), A.augment(src, table, plan, np.float32)
        assert a.shape == (len(table),) + tuple(plan.out_shape) and a.shape == b.shape
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        if bar == A.EXACT:
            assert d.max() == 0
        elif bar == A.LERP:
            assert d.max() <= A.LERP_ATOL, (name, d.max())
        elif bar == A.SATURATION:
            if d.max() > worst_sat:
                worst_sat, worst_name = d.max(), name
        else:
            assert a.dtype == np.uint8 and d.max() <= A.U8_MAX_STEP, name
            assert (d > 0).mean() <= A.U8_MAX_DIFFERING, (name, (d > 0).sum())
    # the recorded figure is the measurement (to 1 %), and the bar four times it
    assert abs(worst_sat - A.SAT_F32_VS_F64) <= 1e-2 * A.SAT_F32_VS_F64, worst_sat
    assert worst_name == A.SAT_WORST_CASE
    assert A.SAT_ATOL == 4 * A.SAT_F32_VS_F64
