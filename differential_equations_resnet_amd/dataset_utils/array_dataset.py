"""Device-resident dataset from in-memory arrays: the replacement of
dataset_utils/tf_dataset_creator_from_arrays.py:22-58 (from_tensor_slices ->
shuffle(full buffer, reshuffle each iteration) -> repeat -> batch).

The whole uint8 image array lives in HBM (CIFAR-10 train: 153.6 MB); a batch
is an index gather on the device, so no host copy sits on the training step.
As with shuffle -> repeat -> batch, batches run across epoch boundaries
(successive independent permutations) and are always full.  For data
parallelism every rank draws the same permutation stream and takes its own
contiguous slice of each global batch (rank r of R gets images
[r*B, (r+1)*B) of the R*B-image global batch).

Preprocessor objects of tf_dataset_preprocessors_image_classification
(RandomCrop, Resize, ...) are compiled into one AugPlan at construction; a
batch is then one launch of the fused augmentation kernel on the dataset array
(runtime.augment_batch) instead of the index gather.  The per-image parameters
are drawn on the host for the whole global batch, from a generator seeded by
the dataset seed, and sliced by rank like the permutation.  Plain callables
(x, y) -> (x, y) listed after them run on the result, as they do without them.
"""
from __future__ import annotations

import numpy as np

__all__ = ["ArrayDataset", "create_tf_dataset_from_arrays"]


class ArrayDataset:
    def __init__(self, features, labels, batch_size, preprocessors=None, repeat=True, num_epochs=None, shuffle=True,
                 seed=0, num_classes=None, rank=0, world_size=1, device=None):
        import torch
        from . import tf_dataset_preprocessors_image_classification as pp
        features = np.asarray(features)
        labels = np.asarray(labels)
        preprocessors = list(preprocessors or [])
        native = [p for p in preprocessors if pp.is_native_preprocessor(p)]
        if native != preprocessors[:len(native)]:
            late = next(p for p in preprocessors[len(native):] if pp.is_native_preprocessor(p))
            raise pp.AsrUnsupported(f"{type(late).__name__}: listed after a plain callable; the fused kernel reads "
                                    "the dataset array, so this module's preprocessors come first")
        self.aug_plan = pp.compile_preprocessors(native, features.shape[1:], features.dtype) if native else None
        if self.aug_plan is not None and self.aug_plan.num_classes is not None:
            num_classes = self.aug_plan.num_classes
        if features.shape[0] != labels.shape[0]:
            raise ValueError("features and labels must have the same number of rows")
        if labels.ndim == 1:
            if num_classes is None:
                num_classes = int(labels.max()) + 1
            labels = np.eye(num_classes, dtype=np.float32)[labels]
        self.n = int(features.shape[0])
        self.batch_size = int(batch_size)
        self.preprocessors = preprocessors[len(native):]  # the plain callables
        self.repeat = repeat
        self.num_epochs = num_epochs
        self.shuffle = shuffle
        self.seed = int(seed)
        self.rank, self.world_size = int(rank), int(world_size)
        if self.batch_size * self.world_size > self.n:
            raise ValueError("global batch larger than the dataset")
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        fdt = torch.uint8 if features.dtype == np.uint8 else torch.float32
        self.features = torch.from_numpy(np.ascontiguousarray(features)).to(self.device, fdt)
        self.labels = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.float32)).to(self.device)
        img_shape = tuple(features.shape[1:])
        self.output_dtype = np.dtype(np.uint8 if fdt == torch.uint8 else np.float32)  # of the image batches
        if self.aug_plan is not None and not self.aug_plan.launches:
            self.aug_plan = None  # e.g. ConvertLabelsToOneHot alone: the index gather is the batch
        if self.aug_plan is not None:
            if self.device.type != "cuda":
                from .. import _lib, runtime
                raise _lib.AsrError(runtime.NO_GPU)
            img_shape, self.output_dtype = tuple(self.aug_plan.out_shape), self.aug_plan.out_dtype
        self.output_shapes = ((self.batch_size,) + img_shape, (self.batch_size, labels.shape[1]))
        self.last_table = None  # this rank's table (ITEM_DTYPE) of the batch yielded last

    def _augmented(self, idx, rng):
        """One launch: rows idx of the dataset array through the compiled chain.  Every rank draws
        the global batch's table and takes its slice."""
        import torch
        from .. import runtime
        B = self.batch_size
        table = self.aug_plan.draw(rng, B * self.world_size)[self.rank * B:(self.rank + 1) * B].copy()
        table["src"] = idx
        self.last_table = table
        items = torch.from_numpy(table.view(np.uint8)).to(self.device, non_blocking=True)
        return runtime.augment_batch(self.features, self.aug_plan, items)

    def _order(self):
        rng = np.random.default_rng(self.seed)
        epoch = 0
        while self.num_epochs is None or epoch < self.num_epochs:
            yield rng.permutation(self.n) if self.shuffle else np.arange(self.n)
            epoch += 1
            if not self.repeat:
                return

    def __iter__(self):
        import torch
        G = self.batch_size * self.world_size
        pending = np.empty(0, dtype=np.int64)
        aug_rng = np.random.default_rng([self.seed, 1]) if self.aug_plan is not None else None
        for perm in self._order():
            pending = np.concatenate([pending, perm])
            while pending.size >= G:
                idx = pending[self.rank * self.batch_size:(self.rank + 1) * self.batch_size]
                pending = pending[G:]
                it = torch.from_numpy(idx).to(self.device, non_blocking=True)
                x = self.features.index_select(0, it) if aug_rng is None else self._augmented(idx, aug_rng)
                y = self.labels.index_select(0, it)
                for p in self.preprocessors:
                    x, y = p(x, y)
                yield x, y
        # a non-repeating stream ends with its (dropped) partial batch


def create_tf_dataset_from_arrays(features, labels, batch_size, preprocessors=None, repeat=True, num_epochs=None,
                                  shuffle=True, prefetch=None, **kwargs):
    """Same call as the reference; returns (dataset, features, labels) where
    the reference returned its two feed placeholders (nothing needs feeding
    here)."""
    ds = ArrayDataset(features, labels, batch_size, preprocessors=preprocessors, repeat=repeat,
                      num_epochs=num_epochs, shuffle=shuffle, **kwargs)
    return ds, features, labels
