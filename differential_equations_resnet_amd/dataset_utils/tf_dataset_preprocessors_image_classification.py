"""Image preprocessors for ArrayDataset: the classes of the reference's
dataset_utils/tf_dataset_preprocessors_image_classification.py, by name and
constructor signature.

The reference wraps each one in a `dataset.map` of a TF 1.12 image op.  Here
they are descriptions: ArrayDataset compiles the list into one AugPlan
(compile_preprocessors) and every batch is produced by one launch of the fused
augmentation kernel (asr_augment_batch, include/asr.h) straight from the
dataset array in HBM.  The random draws are made on the host (AugPlan.draw),
one table row per image; the kernel applies them.

What the fused kernel expresses is one chain
    crop -> resize | resize with pad -> colour operations, a flip anywhere,
so compile_preprocessors refuses any other arrangement with AsrUnsupported
naming the preprocessor and the rule.  TFRecord / JPEG input
(UnpackImagesLabels, DecodeImages, DecodeJPEGImages) is out of scope: the
dataset is an in-memory array.

This module needs numpy only (no GPU) up to the launch itself.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from .._lib import AsrUnsupported

__all__ = ["UnpackImagesLabels", "ConvertLabelsToOneHot", "DecodeImages", "DecodeJPEGImages", "RandomCrop", "Resize",
           "ResizeWithPad", "RandomFlipLeftRight", "RandomBrightness", "RandomSaturation", "AugPlan", "ITEM_DTYPE",
           "compile_preprocessors", "is_native_preprocessor"]

# asr_aug_item (include/asr.h), 32 bytes
ITEM_DTYPE = np.dtype([("src", "<i4"), ("y0", "<i4"), ("x0", "<i4"), ("ch", "<i4"), ("cw", "<i4"), ("flip", "<i4"),
                       ("brightness", "<f4"), ("saturation", "<f4")])
assert ITEM_DTYPE.itemsize == 32

RESIZE_NONE, RESIZE_BILINEAR, RESIZE_PAD = 0, 1, 2  # ASR_AUG_RESIZE_*
COLOR_NONE, COLOR_BRIGHTNESS, COLOR_SATURATION = 0, 1, 2  # ASR_AUG_*


class _Preprocessor:
    """A description the dataset compiles; calling it on a tf.data.Dataset is the reference's
    use and has no meaning here."""

    def __call__(self, *args, **kwargs):
        raise AsrUnsupported(f"{type(self).__name__} is compiled by ArrayDataset (pass it in `preprocessors=`); "
                             "it is not a map over a tf.data.Dataset")


class _OutOfScope(_Preprocessor):
    def __init__(self, *args, **kwargs):
        raise AsrUnsupported(f"{type(self).__name__}: TFRecord/JPEG input is out of scope; the dataset is an "
                             "in-memory array (ArrayDataset, create_tf_dataset_from_arrays)")


class UnpackImagesLabels(_OutOfScope):
    pass


class DecodeImages(_OutOfScope):
    pass


class DecodeJPEGImages(_OutOfScope):
    pass


class ConvertLabelsToOneHot(_Preprocessor):
    """Sets the dataset's num_classes (integer labels become one-hot rows once, at construction);
    launches nothing."""

    def __init__(self, num_classes, num_parallel_calls=None):
        self.num_classes = num_classes
        self.num_parallel_calls = num_parallel_calls


class RandomCrop(_Preprocessor):
    """A square window of side int(float32(min(H, W)) * float32(scale)) at a uniform offset.
    `aspect_ratio` is unused, as in the reference."""

    def __init__(self, aspect_ratio=1, scale=0.9, channels=3, num_parallel_calls=None):
        self.aspect_ratio = aspect_ratio
        self.scale = scale
        self.channels = channels
        self.num_parallel_calls = num_parallel_calls

    def side(self, H, W):
        return int(np.float32(min(H, W)) * np.float32(self.scale))


class Resize(_Preprocessor):
    def __init__(self, target_size, preserve_aspect_ratio=False, num_parallel_calls=None):
        self.target_size = target_size
        self.preserve_aspect_ratio = preserve_aspect_ratio
        self.num_parallel_calls = num_parallel_calls


class ResizeWithPad(_Preprocessor):
    def __init__(self, target_size, num_parallel_calls=None):
        self.target_size = target_size
        self.num_parallel_calls = num_parallel_calls


class RandomFlipLeftRight(_Preprocessor):
    def __init__(self, num_parallel_calls=None):
        self.num_parallel_calls = num_parallel_calls


class RandomBrightness(_Preprocessor):
    def __init__(self, max_delta=0.5, num_parallel_calls=None):
        self.max_delta = max_delta
        self.num_parallel_calls = num_parallel_calls


class RandomSaturation(_Preprocessor):
    def __init__(self, lower=0.5, upper=1.5, num_parallel_calls=None):
        self.lower = lower
        self.upper = upper
        self.num_parallel_calls = num_parallel_calls


def is_native_preprocessor(p) -> bool:
    return isinstance(p, _Preprocessor)


@dataclass
class AugPlan:
    """One compiled preprocessor chain: everything of asr_aug_plan plus the ranges of the draws."""
    in_shape: tuple           # (Hs, Ws, C)
    in_dtype: np.dtype        # uint8 or float32
    out_shape: tuple          # (Ho, Wo, C)
    out_dtype: np.dtype
    crop: tuple               # (ch, cw): the window (the whole image without RandomCrop)
    random_crop: bool = False
    resize: int = RESIZE_NONE
    resized: tuple = (0, 0)   # RESIZE_PAD: (rh, rw)
    pad: tuple = (0, 0)       # RESIZE_PAD: (top, left)
    flip: bool = False
    flip_src: bool = False    # the flip is listed before the resize: it mirrors the window
    color: list = field(default_factory=list)  # COLOR_* in the order they run
    max_delta: float = 0.0
    lower: float = 1.0
    upper: float = 1.0
    num_classes: int | None = None

    @property
    def launches(self) -> bool:
        """False for a chain that changes no pixel (e.g. only ConvertLabelsToOneHot)."""
        return self.random_crop or self.resize != RESIZE_NONE or self.flip or bool(self.color) or \
            tuple(self.crop) != tuple(self.in_shape[:2])

    def draw(self, rng: np.random.Generator, n: int) -> np.ndarray:
        """The table of n images (ITEM_DTYPE; `src` is left 0 for the caller's indices): offsets
        uniform on [0, dim - size], flip with probability 0.5, the brightness delta uniform on
        [-max_delta, max_delta), the saturation factor uniform on [lower, upper).  Only the
        operations of the chain consume draws."""
        t = np.zeros(int(n), dtype=ITEM_DTYPE)
        ch, cw = self.crop
        t["ch"], t["cw"] = ch, cw
        t["saturation"] = 1.0
        if self.random_crop:
            t["y0"] = rng.integers(0, self.in_shape[0] - ch + 1, size=n)
            t["x0"] = rng.integers(0, self.in_shape[1] - cw + 1, size=n)
        if self.flip:
            t["flip"] = rng.random(n) < 0.5
        if COLOR_BRIGHTNESS in self.color:
            t["brightness"] = rng.uniform(-self.max_delta, self.max_delta, size=n)
        if COLOR_SATURATION in self.color:
            t["saturation"] = rng.uniform(self.lower, self.upper, size=n)
        return t


def _size2(p, what):
    try:
        h, w = (int(v) for v in what)
    except (TypeError, ValueError):
        raise ValueError(f"{type(p).__name__}: target_size must be (height, width), got {what!r}") from None
    if h < 1 or w < 1:
        raise ValueError(f"{type(p).__name__}: target_size must be positive, got {what!r}")
    return h, w


def compile_preprocessors(preprocessors, in_shape, in_dtype) -> AugPlan:
    """Compile a list of this module's preprocessors for images of in_shape (H, W, C) and in_dtype
    (uint8 or float32) into one AugPlan: fixes the output shape and dtype, and refuses (AsrUnsupported,
    naming the preprocessor and the rule) what one launch of the fused kernel does not express."""
    Hs, Ws, C = (int(v) for v in in_shape)
    in_dtype = np.dtype(in_dtype)
    if in_dtype not in (np.dtype(np.uint8), np.dtype(np.float32)):
        raise AsrUnsupported(f"preprocessors: image dtype {in_dtype} (uint8 or float32)")
    if C not in (1, 3):
        raise AsrUnsupported(f"preprocessors: {C} image channels (1 or 3)")
    seen = {}
    for pos, p in enumerate(preprocessors):
        if not is_native_preprocessor(p):
            raise AsrUnsupported(f"{type(p).__name__}: not a preprocessor of this module")
        name = type(p).__name__
        if name in seen:
            raise AsrUnsupported(f"{name}: listed twice; each preprocessor may appear at most once")
        seen[name] = pos
    by = {type(p).__name__: p for p in preprocessors}
    if "Resize" in by and "ResizeWithPad" in by:
        raise AsrUnsupported("ResizeWithPad: at most one of Resize and ResizeWithPad in one chain")
    rname = "Resize" if "Resize" in by else "ResizeWithPad" if "ResizeWithPad" in by else None
    rpos = seen.get(rname)
    if rname and "RandomCrop" in by and seen["RandomCrop"] > rpos:
        raise AsrUnsupported(f"RandomCrop: must come before {rname} (the kernel crops, then resizes)")
    for cname in ("RandomBrightness", "RandomSaturation"):
        if rname and cname in by and seen[cname] < rpos:
            raise AsrUnsupported(f"{cname}: colour operations come after {rname} (the kernel resizes first)")

    plan = AugPlan(in_shape=(Hs, Ws, C), in_dtype=in_dtype, out_shape=(Hs, Ws, C), out_dtype=in_dtype, crop=(Hs, Ws))
    if "ConvertLabelsToOneHot" in by:
        plan.num_classes = int(by["ConvertLabelsToOneHot"].num_classes)
    if "RandomCrop" in by:
        side = by["RandomCrop"].side(Hs, Ws)
        if not 1 <= side <= min(Hs, Ws):
            raise ValueError(f"RandomCrop: scale {by['RandomCrop'].scale!r} gives side {side} for a {Hs} x {Ws} image")
        plan.crop, plan.random_crop = (side, side), True
    ch, cw = plan.crop
    Ho, Wo = ch, cw
    if rname == "Resize":
        r = by["Resize"]
        Ho, Wo = _size2(r, r.target_size)
        if r.preserve_aspect_ratio:
            # tf.image.resize_images: scale = min(th / h, tw / w), size = round(scale * (h, w))
            s = min(Ho / ch, Wo / cw)
            kept = (int(round(s * ch)), int(round(s * cw)))
            if kept != (Ho, Wo):
                raise AsrUnsupported(f"Resize: preserve_aspect_ratio=True would give {kept[0]} x {kept[1]}, not the "
                                     f"{Ho} x {Wo} asked for, from a {ch} x {cw} window (accepted only where both "
                                     "agree: use ResizeWithPad)")
        if (Ho, Wo) != (ch, cw):
            plan.resize = RESIZE_BILINEAR
    elif rname == "ResizeWithPad":
        r = by["ResizeWithPad"]
        Ho, Wo = _size2(r, r.target_size)
        # tf.image.resize_image_with_pad: ratio = max(w / tw, h / th), extent floor(h / ratio) x floor(w / ratio),
        # in exact integer arithmetic: the binding side fills the target and the other is floor(side * t / binding).
        # A deliberate difference from TF, whose float32 w / (w / tw) rounds just below tw at some sizes and then
        # loses a pixel of the binding side (a float64 evaluation does the same at other sizes).
        if cw * Ho >= ch * Wo:
            rh, rw = ch * Wo // cw, Wo
        else:
            rh, rw = Ho, cw * Ho // ch
        rh, rw = max(1, rh), max(1, rw)
        if (rh, rw) != (Ho, Wo) or (rh, rw) != (ch, cw):
            if (rh, rw) == (ch, cw) and in_dtype == np.uint8:
                raise AsrUnsupported(f"ResizeWithPad: padding a uint8 {ch} x {cw} window to {Ho} x {Wo} without "
                                     "resizing it keeps uint8 in TF; the kernel's padded mode writes float32")
            plan.resize = RESIZE_PAD
            plan.resized = (rh, rw)
            plan.pad = ((Ho - rh) // 2, (Wo - rw) // 2)
    plan.out_shape = (Ho, Wo, C)
    if plan.resize != RESIZE_NONE:
        plan.out_dtype = np.dtype(np.float32)
    if "RandomFlipLeftRight" in by:
        plan.flip = True
        # before the resize the flip mirrors the window (before the crop too: the offset is uniform, so
        # mirroring the image and then cropping is mirroring the window in distribution)
        plan.flip_src = plan.resize != RESIZE_NONE and seen["RandomFlipLeftRight"] < rpos
    for name in sorted((n for n in ("RandomBrightness", "RandomSaturation") if n in by), key=seen.get):
        p = by[name]
        if name == "RandomBrightness":
            if not p.max_delta >= 0:
                raise ValueError(f"RandomBrightness: max_delta must be non-negative, got {p.max_delta!r}")
            plan.max_delta = float(p.max_delta)
            plan.color.append(COLOR_BRIGHTNESS)
        else:
            if C != 3:
                raise AsrUnsupported(f"RandomSaturation: needs 3 channels, the images have {C}")
            if not 0 <= p.lower < p.upper:
                raise ValueError(f"RandomSaturation: needs 0 <= lower < upper, got {p.lower!r}, {p.upper!r}")
            plan.lower, plan.upper = float(p.lower), float(p.upper)
            plan.color.append(COLOR_SATURATION)
    return plan
