"""The specification of asr_regularize (include/asr.h), restated in numpy fp64.

A segment is (offset, count, layer_stride, layers, l2, smooth): `layers` runs of `count` floats of the
flat parameter buffer, layer_stride apart.  With p_l the floats of layer l,

    R  = sum over segments of  l2 * sum p^2  +  smooth * sum_{l >= 1} ||p_l - p_{l-1}||^2
    dR/dp_l = 2 l2 p_l + 2 smooth ((p_l - p_{l-1}) [l > 0] + (p_l - p_{l+1}) [l < layers - 1])

The coefficients are the float32 values the ABI's struct carries, so the reference gets what the kernel
gets; everything else is fp64.
"""
import numpy as np


def _f32(v):
    return float(np.float32(v))


def layers_of(seg):
    """The index arrays of a segment's layers: [layers, count] positions in the flat buffer."""
    offset, count, stride, layers = (int(v) for v in seg[:4])
    return offset + stride * np.arange(layers)[:, None] + np.arange(count)[None, :]


def covered(segments, n):
    """Boolean [n]: the floats some segment covers."""
    m = np.zeros(n, bool)
    for s in segments:
        m[layers_of(s).ravel()] = True
    return m


def penalty(params, segments):
    """(R, dR): the fp64 penalty and its gradient over the whole buffer (zero off the segments)."""
    p = np.asarray(params, np.float64)
    dR = np.zeros_like(p)
    R = 0.0
    for s in segments:
        idx = layers_of(s)
        l2, smooth = _f32(s[4]), _f32(s[5])
        v = p[idx]  # [layers, count]
        R += l2 * np.sum(v * v)
        g = 2.0 * l2 * v
        if idx.shape[0] > 1:
            d = v[1:] - v[:-1]
            R += smooth * np.sum(d * d)
            g[1:] += 2.0 * smooth * d
            g[:-1] -= 2.0 * smooth * d
        dR[idx] += g
    return float(R), dR


def l2_loss(value, l2):
    """Keras' l2(l) penalty of one variable: l * sum(v ** 2)."""
    return _f32(l2) * float(np.sum(np.asarray(value, np.float64) ** 2))
