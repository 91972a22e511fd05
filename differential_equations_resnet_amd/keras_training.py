"""The Keras training calls of graph.Model -- compile / fit / evaluate /
train_on_batch / test_on_batch -- over the native executor, as the reference
notebooks make them (model.compile(optimizer=..., loss='categorical_crossentropy',
metrics=['accuracy']); model.fit(x, y, batch_size=32, shuffle=True,
validation_data=(xv, yv))).

A step is the executor's fused forward+backward, one optimiser launch
(asr_optimizer_update) and one metrics launch (asr_batch_metrics); an evaluation
step is the forward-only executor's forward and the metrics launch.  A model
with regularisers (l2_regularization, smoothness_regularization) also runs
asr_regularize in each: between the backward and the update it adds the
penalty's gradient to the executor's gradients and the penalty R to its loss,
and in an evaluation step it adds R to the accumulated loss, so 'loss' and
'val_loss' are Keras' loss + sum(model.losses).  A model without them makes no
such call.  The arrays
go to device memory once and a batch is an index gather there.  An epoch's last
batch may be partial: it runs at its own size through a second executor (never
padded: the loss is a mean over the batch).  asr_batch_metrics accumulates
per-batch means and counts, so the full-size batches and the odd-size one are
accumulated apart and combined on the host into Keras' sample-weighted epoch
means.  The host reads the device once per epoch (all accumulators in one
copy), and with verbose=1 once more per progress-bar refresh.
"""
from __future__ import annotations

import sys
import time

import numpy as np

from . import _lib

__all__ = ["History", "compile_model", "fit", "evaluate", "train_on_batch", "test_on_batch"]

NOT_COMPILED = "You must compile a model before training/testing. Use `model.compile(optimizer, loss)`."
BAR_REFRESH_SECONDS = 1.0  # verbose=1: at most one metric read per this many seconds


class History:
    """tf.keras.callbacks.History as fit() returns it."""

    def __init__(self, params):
        self.params = params
        self.epoch = []
        self.history = {}

    def _append(self, epoch, logs):
        self.epoch.append(epoch)
        for k, v in logs.items():
            self.history.setdefault(k, []).append(v)


class _Compiled:
    def __init__(self, optimizer, want_acc, dtype):
        self.optimizer, self.want_acc, self.dtype = optimizer, want_acc, dtype

    @property
    def metric_names(self):
        return ["loss", "acc"] if self.want_acc else ["loss"]


def compile_model(model, optimizer, loss="categorical_crossentropy", metrics=None, dtype=None):
    """Model.compile: host only (nothing is lowered before the first step)."""
    from . import optimizers
    from .runtime import dtype_code
    if loss != "categorical_crossentropy":
        raise ValueError(f"`loss` must be 'categorical_crossentropy' (the native executor's loss), got {loss!r}")
    if metrics is not None and list(metrics) not in ([], ["accuracy"], ["acc"]):
        raise ValueError(f"`metrics` must be None, [], ['accuracy'] or ['acc'], got {metrics!r}")
    if dtype is not None:
        try:
            dtype_code(dtype)
        except (ValueError, TypeError):
            raise ValueError(f"`dtype` must be None, 'float32' or 'bfloat16', got {dtype!r}") from None
    try:
        opt = optimizers.get(optimizer)
    except ValueError as e:
        raise ValueError(f"`optimizer`: {e}") from None
    model._compiled = _Compiled(opt, bool(metrics), dtype)


def _compiled(model) -> _Compiled:
    c = getattr(model, "_compiled", None)
    if c is None:
        raise RuntimeError(NOT_COMPILED)
    return c


def _is_dataset(x):
    return hasattr(x, "output_shapes") and hasattr(x, "__iter__")


def _check_arrays(x, y, what="x"):
    """Shapes and dtypes of an (images, one-hot labels) pair, on the host (no device use)."""
    if x is None or y is None:
        raise ValueError(f"`{what}` and `y` must both be given (arrays), or `{what}` a dataset with `y` None")
    if not hasattr(x, "shape") or not hasattr(y, "shape"):
        raise ValueError(f"`{what}` and `y` must be numpy arrays or tensors")
    if len(y.shape) != 2:
        raise ValueError(f"`y` must be one-hot rows [n, num_classes], got shape {tuple(y.shape)}: convert class "
                         "indices with optimizers.to_categorical")
    if len(x.shape) != 4:
        raise ValueError(f"`{what}` must be NHWC images [n, H, W, C], got shape {tuple(x.shape)}")
    if int(x.shape[0]) != int(y.shape[0]) or int(x.shape[0]) < 1:
        raise ValueError(f"`{what}` has {int(x.shape[0])} samples and `y` {int(y.shape[0])} (equal, at least 1)")


class _Arrays:
    """An (images, labels) pair resident on the device, served in index-gathered batches."""

    def __init__(self, native, x, y):
        import torch
        self.x = native._images(x)
        if isinstance(y, np.ndarray):
            y = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))
        self.y = y.to(native.device, dtype=torch.float32).contiguous()
        self.n = int(self.x.shape[0])
        self.device = native.device

    def batches(self, batch_size, order=None):
        """(images, labels) batches of one pass; order: a host permutation (one upload) or None."""
        import torch
        idx = None if order is None else torch.from_numpy(np.ascontiguousarray(order, dtype=np.int64)).to(self.device)
        for i in range(0, self.n, batch_size):
            if idx is None:
                yield self.x[i:i + batch_size], self.y[i:i + batch_size]
            else:
                sel = idx[i:i + batch_size]
                yield self.x.index_select(0, sel), self.y.index_select(0, sel)


def _dataset_batches(it, steps):
    for _ in range(steps):
        try:
            yield next(it)
        except StopIteration:
            raise RuntimeError("dataset exhausted before `steps_per_epoch` / `validation_steps` / `steps` batches "
                               "(use repeat=True)") from None


class _Runner:
    """The per-model device state of the Keras calls: two metric accumulators per stream (row 0 the
    batches of the main size, row 1 any other size), train rows 0-1, evaluation rows 2-3."""

    def __init__(self, model, dtype):
        import torch
        from . import runtime
        self.rt = runtime
        self.torch = torch
        self.native = model.compile_native(1, dtype).state
        self.dtype = self.native.resolve_dtype(dtype)
        self.accum = torch.zeros(4, 4, dtype=torch.float32, device=self.native.device)

    def _labels(self, labels, n):
        torch = self.torch
        if isinstance(labels, np.ndarray):
            labels = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.float32))
        t = labels.to(self.native.device, dtype=torch.float32).contiguous()
        K = self.native.plan.num_classes
        if t.dim() != 2 or tuple(t.shape) != (n, K):
            raise ValueError(f"labels must be one-hot [{n}, {K}], got {tuple(t.shape)}")
        return t

    def train_step(self, opt, images, labels, main):
        images = self.native._images(images)
        n = int(images.shape[0])
        labels = self._labels(labels, n)
        ex = self.native.executor(n, self.dtype, images.dtype == self.torch.uint8)
        loss, grads = ex.forward_backward(self.native.params, images, labels, want_probs=True)
        self.native.regularize(grads, 1.0, loss)
        self.native.apply_optimizer(opt, grads)
        self.rt.batch_metrics(ex.probs, labels, loss, self.accum[0 if n == main else 1])

    def test_step(self, images, labels, main):
        images = self.native._images(images)
        n = int(images.shape[0])
        labels = self._labels(labels, n)
        ex = self.native.executor(n, self.dtype, images.dtype == self.torch.uint8, inference=True)
        probs = ex.forward(self.native.params, images)
        row = self.accum[2 if n == main else 3]
        self.rt.batch_metrics(probs, labels, None, row)
        self.native.regularize(None, 1.0, row)  # row[0], the sum of the batches' losses, += R

    def rows(self):
        """One device read: the four accumulator rows [sum of batch-mean losses, correct, samples, batches]."""
        return self.accum.cpu().double().numpy()


def _runner(model, c) -> _Runner:
    r = getattr(model, "_keras_runner", None)
    if r is None or r.dtype != model.compile_native(1, c.dtype).dtype:
        r = model._keras_runner = _Runner(model, c.dtype)
    return r


def _logs(c, prefix, vals):
    loss, acc = vals
    out = {prefix + "loss": loss}
    if c.want_acc:
        out[prefix + "acc"] = acc
    return out


def fit(model, x=None, y=None, batch_size=None, epochs=1, verbose=1, callbacks=None, validation_split=0.0,
        validation_data=None, shuffle=True, class_weight=None, sample_weight=None, initial_epoch=0,
        steps_per_epoch=None, validation_steps=None):
    from . import distributed
    c = _compiled(model)
    # everything refused or malformed is found here, before any device use
    if callbacks:
        raise _lib.AsrUnsupported("fit: `callbacks` are not supported (History is returned; use Training for logs)")
    if validation_split:
        raise _lib.AsrUnsupported("fit: `validation_split` is not supported (pass `validation_data`)")
    if class_weight is not None:
        raise _lib.AsrUnsupported("fit: `class_weight` is not supported (the executor's loss is unweighted)")
    if sample_weight is not None:
        raise _lib.AsrUnsupported("fit: `sample_weight` is not supported (the executor's loss is unweighted)")
    if distributed.is_initialized():
        raise _lib.AsrUnsupported("fit: data-parallel training (distributed.is_initialized()) runs through Training")
    if verbose not in (0, 1):
        raise ValueError(f"`verbose` must be 0 or 1, got {verbose!r}")
    epochs, initial_epoch = int(epochs), int(initial_epoch)
    ds_form = _is_dataset(x)
    if ds_form:
        if y is not None:
            raise ValueError("`y` must be None when `x` is a dataset (it yields the labels)")
        if steps_per_epoch is None:
            raise ValueError("`steps_per_epoch` is required when `x` is a dataset")
        if batch_size is not None:
            raise ValueError("`batch_size` must be None when `x` is a dataset (it batches itself)")
        steps_per_epoch = int(steps_per_epoch)
        B = int(x.output_shapes[0][0])
        n_train = steps_per_epoch * B
    else:
        _check_arrays(x, y)
        if steps_per_epoch is not None:
            raise ValueError("`steps_per_epoch` goes with a dataset `x`; arrays are batched by `batch_size`")
        B = int(batch_size or 32)
        if B < 1:
            raise ValueError(f"`batch_size` must be >= 1, got {batch_size!r}")
        n_train = int(x.shape[0])
        steps_per_epoch = -(-n_train // B)
    val_ds = val_arrays = None
    if validation_data is not None:
        if _is_dataset(validation_data):
            if validation_steps is None:
                raise ValueError("`validation_steps` is required when `validation_data` is a dataset")
            val_ds = validation_data
            VB, vsteps = int(val_ds.output_shapes[0][0]), int(validation_steps)
        else:
            if not isinstance(validation_data, (tuple, list)) or len(validation_data) != 2:
                raise ValueError("`validation_data` must be (x_val, y_val) or a dataset with `validation_steps`")
            _check_arrays(validation_data[0], validation_data[1], "validation_data[0]")
            VB = B
    names = c.metric_names + (["val_" + m for m in c.metric_names] if validation_data is not None else [])
    hist = History({"batch_size": None if ds_form else B, "epochs": epochs, "steps": steps_per_epoch,
                    "samples": n_train, "verbose": verbose, "do_validation": validation_data is not None,
                    "metrics": names})

    run = _runner(model, c)
    opt = c.optimizer
    data = None if ds_form else _Arrays(run.native, x, y)
    train_it = iter(x) if ds_form else None
    if val_ds is not None:
        val_it = iter(val_ds)
    elif validation_data is not None:
        val_arrays = _Arrays(run.native, *validation_data)
    for epoch in range(initial_epoch, epochs):
        run.accum.zero_()
        if ds_form:
            batches = _dataset_batches(train_it, steps_per_epoch)
        else:
            batches = data.batches(B, np.random.permutation(data.n) if shuffle else None)
        bar = None
        if verbose:
            from tqdm import tqdm
            bar = tqdm(total=steps_per_epoch, file=sys.stdout, desc=f"Epoch {epoch + 1}/{epochs}")
            shown = time.monotonic()
        for images, labels in batches:
            run.train_step(opt, images, labels, B)
            if bar is not None:
                bar.update(1)
                if time.monotonic() - shown >= BAR_REFRESH_SECONDS:  # (reads the device metrics: synchronises)
                    a = run.rows()
                    bar.set_postfix(_logs(c, "", _combine(a[0], a[1])), refresh=False)
                    shown = time.monotonic()
        if validation_data is not None:
            vb = _dataset_batches(val_it, vsteps) if val_ds is not None else val_arrays.batches(VB)
            for images, labels in vb:
                run.test_step(images, labels, VB)
        a = run.rows()  # the epoch's one read
        logs = _logs(c, "", _combine(a[0], a[1]))
        if validation_data is not None:
            logs.update(_logs(c, "val_", _combine(a[2], a[3])))
        run.native.check_status()  # after the read: the launches have completed, a failed one raises here
        if bar is not None:
            bar.set_postfix(logs)
            bar.close()
        hist._append(epoch, logs)
    return hist


def _combine(full, tail):
    """Keras' sample-weighted (loss, accuracy) from two accumulator rows [sum of batch-mean losses,
    correct, samples, batches].  Every batch of a row has one size, samples / batches, so the row's
    sum of batch means times that size is its sum over samples."""
    samples = full[2] + tail[2]
    if samples == 0:
        raise RuntimeError("no batch was run")
    loss = sum(r[0] * r[2] / r[3] for r in (full, tail) if r[3] > 0)
    return float(loss / samples), float((full[1] + tail[1]) / samples)


def _result(c, vals):
    return [vals[0], vals[1]] if c.want_acc else vals[0]


def evaluate(model, x=None, y=None, batch_size=None, verbose=1, steps=None):
    c = _compiled(model)
    if verbose not in (0, 1):
        raise ValueError(f"`verbose` must be 0 or 1, got {verbose!r}")
    ds_form = _is_dataset(x)
    if ds_form:
        if y is not None or steps is None or batch_size is not None:
            raise ValueError("a dataset `x` takes `steps`, and neither `y` nor `batch_size`")
        B, steps = int(x.output_shapes[0][0]), int(steps)
    else:
        _check_arrays(x, y)
        if steps is not None:
            raise ValueError("`steps` goes with a dataset `x`; arrays are batched by `batch_size`")
        B = int(batch_size or 32)
        steps = -(-int(x.shape[0]) // B)
    run = _runner(model, c)
    run.accum.zero_()
    batches = _dataset_batches(iter(x), steps) if ds_form else _Arrays(run.native, x, y).batches(B)
    if verbose:
        from tqdm import tqdm
        batches = tqdm(batches, total=steps, file=sys.stdout, desc="Evaluation")
    for images, labels in batches:
        run.test_step(images, labels, B)
    a = run.rows()
    run.native.check_status()
    return _result(c, _combine(a[2], a[3]))


def train_on_batch(model, x, y):
    """One update on one batch; returns its loss (and accuracy) from before the update."""
    c = _compiled(model)
    _check_arrays(x, y)
    run = _runner(model, c)
    run.accum.zero_()
    n = int(x.shape[0])
    run.train_step(c.optimizer, x, y, n)
    a = run.rows()
    return _result(c, _combine(a[0], a[1]))


def test_on_batch(model, x, y):
    c = _compiled(model)
    _check_arrays(x, y)
    run = _runner(model, c)
    run.accum.zero_()
    n = int(x.shape[0])
    run.test_step(x, y, n)
    a = run.rows()
    return _result(c, _combine(a[2], a[3]))
