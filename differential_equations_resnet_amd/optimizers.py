"""tf.keras.optimizers.SGD / Adam / RMSprop and tf.keras.utils.to_categorical
for Model.compile / fit and Training: the Keras 2.1.6-tf (TF 1.12) argument
names, defaults and update rules, applied on the device in one launch per step
(asr_optimizer_update, include/asr.h).

An optimiser object holds hyper-parameters and its `iterations` count only, on
the host.  Its state buffers live with the parameters they belong to
(lowering.NativeModel.apply_optimizer).  `next_config` is pure host code: it
fills the asr_optimizer_config of the next update, Keras' learning-rate decay
lr / (1 + decay * iterations) included.
"""
from __future__ import annotations

import numpy as np

from . import _lib

__all__ = ["Optimizer", "SGD", "Adam", "RMSprop", "get", "to_categorical", "KERAS_EPSILON"]

KERAS_EPSILON = 1e-7  # tf.keras.backend.epsilon(): what epsilon=None means


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"`{name}` must be a number, got {v!r}")
    return float(v)


class Optimizer:
    kind: int = -1

    def __init__(self, lr, decay):
        self.lr = _number("lr", lr)
        self.decay = _number("decay", decay)
        if self.decay < 0:
            raise ValueError(f"`decay` must be >= 0, got {decay!r}")
        self.iterations = 0  # updates applied so far

    @property
    def flags(self) -> int:
        return 0

    def _ab(self):
        raise NotImplementedError

    def slots(self) -> int:
        """How many parameter-sized state buffers the update keeps (host only)."""
        return int(_lib.load().asr_optimizer_slots(self.kind, self.flags))

    def current_lr(self, lr=None) -> float:
        """The next update's learning rate: `lr` (default self.lr) after Keras' decay."""
        base = self.lr if lr is None else _number("lr", lr)
        return base / (1.0 + self.decay * self.iterations)

    def next_config(self, lr=None, grad_scale=1.0) -> _lib.OptimizerConfig:
        """The asr_optimizer_config of the next update (step = iterations + 1).  `lr` replaces self.lr
        (a schedule's value); decay applies to either."""
        a, b, eps = self._ab()
        return _lib.OptimizerConfig(self.kind, self.flags, self.current_lr(lr), a, b, eps, self.iterations + 1,
                                    float(grad_scale))

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={v!r}' for k, v in self.get_config().items())})"


class SGD(Optimizer):
    """tf.keras.optimizers.SGD: v = momentum*m - lr*g; p += momentum*v - lr*g (nesterov) or p += v."""
    kind = _lib.ASR_OPT_SGD

    def __init__(self, lr=0.01, momentum=0.0, decay=0.0, nesterov=False):
        super().__init__(lr, decay)
        self.momentum = _number("momentum", momentum)
        self.nesterov = bool(nesterov)

    @property
    def flags(self):
        return _lib.ASR_OPT_NESTEROV if self.nesterov else 0

    def _ab(self):
        return self.momentum, 0.0, 0.0

    def get_config(self):
        return {"lr": self.lr, "momentum": self.momentum, "decay": self.decay, "nesterov": self.nesterov}


class Adam(Optimizer):
    """tf.keras.optimizers.Adam (the epsilon-hat form, as tf.train.AdamOptimizer), with AMSGrad."""
    kind = _lib.ASR_OPT_ADAM

    def __init__(self, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0.0, amsgrad=False):
        super().__init__(lr, decay)
        self.beta_1, self.beta_2 = _number("beta_1", beta_1), _number("beta_2", beta_2)
        self.epsilon = KERAS_EPSILON if epsilon is None else _number("epsilon", epsilon)
        self.amsgrad = bool(amsgrad)

    @property
    def flags(self):
        return _lib.ASR_OPT_AMSGRAD if self.amsgrad else 0

    def _ab(self):
        return self.beta_1, self.beta_2, self.epsilon

    def get_config(self):
        return {"lr": self.lr, "beta_1": self.beta_1, "beta_2": self.beta_2, "decay": self.decay,
                "epsilon": self.epsilon, "amsgrad": self.amsgrad}


class RMSprop(Optimizer):
    """tf.keras.optimizers.RMSprop: a = rho*a + (1 - rho)*g^2; p -= lr*g/(sqrt(a) + epsilon)."""
    kind = _lib.ASR_OPT_RMSPROP

    def __init__(self, lr=0.001, rho=0.9, epsilon=None, decay=0.0):
        super().__init__(lr, decay)
        self.rho = _number("rho", rho)
        self.epsilon = KERAS_EPSILON if epsilon is None else _number("epsilon", epsilon)

    def _ab(self):
        return self.rho, 0.0, self.epsilon

    def get_config(self):
        return {"lr": self.lr, "rho": self.rho, "decay": self.decay, "epsilon": self.epsilon}


_BY_NAME = {"sgd": SGD, "adam": Adam, "rmsprop": RMSprop}


def get(identifier) -> Optimizer:
    """tf.keras.optimizers.get: 'sgd' | 'adam' | 'rmsprop' (any case) with the defaults, an
    Optimizer instance as it is, or a training.AdamOptimizer as Adam with its hyper-parameters."""
    from .training.training import AdamOptimizer
    if isinstance(identifier, Optimizer):
        return identifier
    if isinstance(identifier, AdamOptimizer):
        try:
            lr = _number("learning_rate", identifier.learning_rate)
        except ValueError:
            raise ValueError("AdamOptimizer.learning_rate must be a number to be used as a Keras optimizer, got "
                             f"{identifier.learning_rate!r}") from None
        return Adam(lr=lr, beta_1=identifier.beta1, beta_2=identifier.beta2, epsilon=identifier.epsilon)
    if isinstance(identifier, str):
        cls = _BY_NAME.get(identifier.lower())
        if cls is None:
            raise ValueError(f"Unknown optimizer: {identifier!r} (one of {sorted(_BY_NAME)})")
        return cls()
    raise ValueError(f"Could not interpret optimizer identifier: {identifier!r}")


def to_categorical(y, num_classes=None):
    """tf.keras.utils.to_categorical: integer class vector -> float32 one-hot rows [..., num_classes]."""
    y = np.asarray(y)
    if y.size and not np.all(y == np.floor(y)):
        raise ValueError("to_categorical: class indices must be integers")
    y = y.astype(np.int64)
    shape = y.shape
    if len(shape) > 1 and shape[-1] == 1:
        shape = shape[:-1]
    y = y.ravel()
    if y.size and y.min() < 0:
        raise ValueError("to_categorical: class indices must be >= 0")
    if num_classes is None:
        num_classes = int(y.max()) + 1 if y.size else 0
    num_classes = int(num_classes)
    if y.size and y.max() >= num_classes:
        raise ValueError(f"to_categorical: class index {int(y.max())} with num_classes={num_classes}")
    out = np.zeros((y.size, num_classes), dtype=np.float32)
    out[np.arange(y.size), y] = 1.0
    return out.reshape(shape + (num_classes,))
