"""Shared test utilities: bf16 rounding in numpy, mask decoding, tolerances, guarded buffers."""
import numpy as np

GUARD = 256  # bytes on either side of a carved buffer (keeps the allocation's 256-byte alignment for the view)


def carve(shape, dtype, dev, fill=0xA5, guard_fill=0xA5):
    """A contiguous tensor of `shape` and `dtype` of exactly its documented byte size, GUARD bytes into
    a larger uint8 buffer: (buffer, view).  The interior bytes are `fill`, the GUARD bytes on either
    side `guard_fill` (0xFF: NaN as fp32 and as bf16, all-ones mask bits, -1 as int32)."""
    import torch
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
    n = int(np.prod(shape, dtype=np.int64)) * torch.empty(0, dtype=dtype).element_size()
    buf = torch.empty(GUARD + n + GUARD, dtype=torch.uint8, device=dev)
    buf[:GUARD] = guard_fill
    buf[GUARD:GUARD + n] = fill
    buf[GUARD + n:] = guard_fill
    return buf, buf[GUARD:GUARD + n].view(dtype).view(shape)


def carve_like(t, guard_fill=0xFF):
    """An input buffer: the contents of the tensor `t` (moved to its device's carved buffer bit for
    bit), exactly its byte size, between two guards of `guard_fill`: (buffer, view)."""
    t = t.contiguous()
    buf, view = carve(tuple(t.shape), t.dtype, t.device, 0, guard_fill)
    view.copy_(t)
    return buf, view


def guards_intact(buf, nbytes, what, guard_fill=0xA5):
    """Assert that the GUARD bytes before and after the `nbytes` interior of a carved buffer still hold
    `guard_fill`.  Only the two guard slices are copied to the host (workspaces reach tens of MB)."""
    assert buf.numel() == GUARD + nbytes + GUARD, f"{what}: not a carved buffer of {nbytes} bytes"
    before = buf[:GUARD].cpu().numpy()
    after = buf[GUARD + nbytes:].cpu().numpy()
    bad = np.flatnonzero(before != guard_fill)
    assert bad.size == 0, (f"{what}: bytes before the buffer overwritten ({bad.size} of {GUARD}, nearest "
                           f"{GUARD - int(bad[-1])} bytes before its start)")
    bad = np.flatnonzero(after != guard_fill)
    assert bad.size == 0, (f"{what}: bytes after the buffer overwritten ({bad.size} of {GUARD}, first "
                           f"{int(bad[0])} bytes past its end)")


def bf16_round(x):
    """Round float32 -> bfloat16 (RNE) and back, in numpy."""
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(a.shape)


def _pairs_antisymmetric(src, sign, C):
    """Every off-diagonal W[t][i][o] (i > o) and W[8-t][o][i] read the same
    theta with opposite signs (the 3by3 and general maps, either
    `antisymmetric` flag; not the regular kind)."""
    s = np.asarray(src).reshape(9, C, C)
    g = np.asarray(sign).reshape(9, C, C)
    i, o = np.triu_indices(C, 1)[::-1]  # i > o
    a, b = s[:, i, o], s[::-1][:, o, i]
    return bool(np.all(a >= 0) and np.all(a == b) and np.all(g[:, i, o] == -g[::-1][:, o, i]))


def w_bf16_balanced(W, src=None, sign=None, mirrored=False):
    """The bf16 W of the executor's weight pack (asr_theta.hip,
    k_theta_to_w_pack_bal), bit-exact.  Maps whose off-diagonal entries come
    in antisymmetric pairs (W[t][i][o] = -W[8-t][o][i]) round each pair to one
    of its two bf16 neighbours, chosen so that every output channel's sum of
    rounding errors stays near zero: round-to-nearest perturbs each output
    channel by a fixed sum that every pixel of every image sees, and over a
    deep stack that coherent error dominates (tools/bf16_depth_emulate.py,
    DESIGN §3g).  Diagonal entries round to nearest and their errors (taps
    0..8, float32) start each channel's error sum e; the pairs are then
    visited in the round-robin order of the kernel (C-1 rounds of C/2 disjoint
    channel pairs); within a pair (o, i), D = e_o - e_i, and per tap 0..8 the
    upper neighbour iff D + (d_lo + d_hi) < 0, else the lower (a bf16 value
    stays), D += 2d; then e_o += S, e_i -= S for the pair's S = sum d, all in
    float32.  A map without the pairing (or src=None) rounds to nearest.
    mirrored (PackJob::mirror, asr_theta_to_w_mirror): W is W_bwd =
    -flip(V)^T of a forward V and src, sign its transposed map; the sums then
    start from V's diagonal errors, term t from the negated entry of W at tap
    8 - t (V[t][o][o] itself), so every pair takes V's decision and the
    result is -flip(w_bf16_balanced(V))^T bit for bit."""
    W32 = np.asarray(W, np.float32).reshape(3, 3, W.shape[2], W.shape[3])
    C = W32.shape[2]
    Q = bf16_round(W32).reshape(9, C, C).copy()
    if src is None or C % 2 or not _pairs_antisymmetric(src, sign, C):
        return Q.reshape(W32.shape)
    X = W32.reshape(9, C, C)
    err = np.zeros(C, np.float32)
    dg = np.arange(C)
    for t in range(9):  # the error sums start from the diagonal entries' (nearest) rounding
        x = -X[8 - t, dg, dg] if mirrored else X[t, dg, dg]
        err = err + (bf16_round(x) - x)
    q = np.arange(1, C // 2)
    for r in range(C - 1):
        a = np.concatenate([[C - 1], (r + q) % (C - 1)])
        b = np.concatenate([[r], (r - q) % (C - 1)])
        o, i = np.minimum(a, b), np.maximum(a, b)
        eo, ei = err[o].copy(), err[i].copy()
        D, S = eo - ei, np.zeros_like(eo)
        for t in range(9):
            x = X[t, i, o]
            bits = x.view(np.uint32)
            exact = (bits & np.uint32(0xFFFF)) == 0
            dtz = (bits & np.uint32(0xFFFF0000)).view(np.float32) - x
            daw = ((bits & np.uint32(0xFFFF0000)) + np.uint32(0x10000)).view(np.float32) - x
            zero = np.float32(0)
            d_lo = np.where(exact, zero, np.where(x > 0, dtz, daw)).astype(np.float32)
            d_hi = np.where(exact, zero, np.where(x > 0, daw, dtz)).astype(np.float32)
            sd = np.where(exact, zero, dtz + daw).astype(np.float32)
            d = np.where(D + sd < 0, d_hi, d_lo).astype(np.float32)
            D = (D + np.float32(2) * d).astype(np.float32)
            S = (S + d).astype(np.float32)
            qv = (x + d).astype(np.float32)
            Q[t, i, o] = qv
            Q[8 - t, o, i] = -qv
        err[o], err[i] = eo + S, ei - S
    return Q.reshape(W32.shape)


def w_mirror(W):
    """-flip(W)^T of an HWIO [3, 3, C, C] array: the transposed operator's W (asr_param_map_transpose)."""
    return -np.asarray(W)[::-1, ::-1].transpose(0, 1, 3, 2)


def transpose_map(src, sign, C):
    """(src, sign) of W_bwd = -flip(W)^T (asr_param_map_transpose, for a map without constant entries)."""
    s = np.asarray(src).reshape(3, 3, C, C)[::-1, ::-1].transpose(0, 1, 3, 2)
    g = -np.asarray(sign).reshape(3, 3, C, C)[::-1, ::-1].transpose(0, 1, 3, 2)
    return np.ascontiguousarray(s).reshape(np.shape(src)), np.ascontiguousarray(g).reshape(np.shape(sign))


def decode_mask(mask_bytes, N, H, W, C):
    """Inverse of the relu-mask layout (include/asr.h): bit (pixel*C + o),
    LSB first, pixel = (n*H + y)*W + x.  Returns bool [N,H,W,C]."""
    b = np.asarray(mask_bytes).view(np.uint8)
    bits = np.unpackbits(b, bitorder="little")[: N * H * W * C]
    return bits.reshape(N, H, W, C).astype(bool)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def assert_close(got, want, rtol, atol=0.0, what=""):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    lim = atol + rtol * np.abs(want)
    bad = err > lim
    if bad.any():
        i = np.unravel_index(np.argmax(err - lim), err.shape)
        raise AssertionError(f"{what}: {bad.sum()} / {bad.size} elements outside tolerance "
                             f"(rtol={rtol}, atol={atol}); worst at {i}: got {got[i]!r} want {want[i]!r}")


def rel_l2(got, want):
    """||got - want||_2 / ||want||_2 over the flattened arrays."""
    got = np.asarray(got, np.float64).ravel()
    want = np.asarray(want, np.float64).ravel()
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))


def grad_groups(spec, g):
    """(name, flat array) per gradient group in Keras weight order: conv1
    kernel and bias, per block its merged theta (all kernel variables) and
    bias, fc kernel and bias — the per-layer groups of the reference's
    gradient norms (training.py:385-409)."""
    nt = len(spec.theta_shapes())
    out = [("conv1/kernel", np.ravel(g[0])), ("conv1/bias", np.ravel(g[1]))]
    i = 2
    for b in range(spec.L):
        out.append((f"block{b}/theta", np.concatenate([np.ravel(a) for a in g[i:i + nt]])))
        out.append((f"block{b}/bias", np.ravel(g[i + nt])))
        i += nt + 1
    out += [("fc/kernel", np.ravel(g[i])), ("fc/bias", np.ravel(g[i + 1]))]
    return out


def assert_grad_tensors_max(spec, got, want, tol, report_only=False, groups=None):
    """Per-tensor bar inside the per-group one: every gradient tensor's
    max |got - want| <= tol x max |want| over the tensor's gradient group.
    A group's relative L2 dilutes a few wrong scalars (a zeroed channel of
    one theta variable) among thousands of kernel entries; this bar does
    not.  `groups`: [(name, [tensor indices])]; default: the network's
    (conv1, per block theta + bias, fc).  report_only: return the worst
    (name, ratio) instead of asserting."""
    if groups is None:
        nt = len(spec.theta_shapes())
        groups = [("conv1", [0, 1])]
        i = 2
        for b in range(spec.L):
            groups.append((f"block{b}", list(range(i, i + nt + 1))))
            i += nt + 1
        groups.append(("fc", [i, i + 1]))
    worst, bad = ("", 0.0), []
    for name, idx in groups:
        scale = max(float(np.abs(want[i]).max()) for i in idx)
        if scale == 0:
            continue
        for i in idx:
            r = float(np.abs(np.asarray(got[i], np.float64) - want[i]).max()) / scale
            if r > worst[1]:
                worst = (f"{name}/tensor{i} {np.shape(want[i])}", r)
            if not r <= tol:
                bad.append(f"{name}/tensor{i} {np.shape(want[i])}: {r:.3e}")
    if report_only:
        return worst
    assert not bad, f"per-tensor max|err| > {tol} x group max: " + "; ".join(bad[:12])
    return worst


CLIP_BAND = (1e-8, 1e-6)  # no renormalised q or 1 - q of a clip case may lie here (Keras' epsilon is 1e-7)


def clip_case(seed=0):
    """A batch that exercises Keras' probability clip in the head (k_head):
    (spec, params, images float32, onehot).  fp32 net, float images, no
    input normalisation, L=1, fc bias (+24, -24, 0, ...).  Conv1's channel 0
    has an all-positive kernel, so the pooled feature 0 measures brightness;
    fc row 0 is -bias / (feature 0 of a bright image).  The 4 bright images'
    logits are therefore O(1) (unsaturated), the 8 dim images' logits are the
    bias: true class 0 there has probability > 1 - 1e-9, any other true class
    < 1e-9.  clip_classes() says which image is which; test_clip_case_is_
    conditioned (CPU) asserts the margins."""
    from oracle import asr_oracle as O
    rng = np.random.default_rng(seed)
    K, C, N = 10, 16, 12
    spec = O.NetSpec(C=C, L=1, h=0.5, gamma=0.0, num_classes=K, H=6, W=7, Cin=3, subtract_mean=None,
                     divide_by_stddev=None)
    params = O.init_params(spec, rng, np.float64, bias_std=0.05)
    params[0][..., 0] = np.abs(params[0][..., 0])
    params[1][0] = 0.0
    imgs = rng.uniform(0.5, 1.0, (N, spec.H, spec.W, 3)).astype(np.float32)
    imgs[4:] *= np.float32(0.01)
    bias = np.zeros(K)
    bias[0], bias[1] = 24.0, -24.0
    params[-1] = bias
    params[-2] = params[-2] * 0.05
    params = [p.astype(np.float32).astype(np.float64) for p in params]
    _, cache = O.net_forward(spec, params, imgs)
    gbar = cache["gap"][:4, 0].mean()
    params[-2][0] = (-bias / gbar).astype(np.float32).astype(np.float64)
    labels = np.array([0, 1, 5, 9, 0, 0, 0, 1, 1, 4, 7, 9])
    return spec, params, imgs, np.eye(K)[labels]


def clip_classes(probs, onehot):
    """(low, high, unsaturated) boolean masks over the images, from fp64
    probabilities: true-class renormalised q < 1e-9, 1 - q < 1e-9, or
    1e-6 < q < 1 - 1e-6; and the smallest distance factor of any q or 1 - q
    to CLIP_BAND as a bool `clear` (True: nothing inside the band)."""
    q = probs / probs.sum(axis=-1, keepdims=True)
    qt = (q * onehot).sum(axis=-1)
    omt = ((1.0 - q) * onehot).sum(axis=-1)
    lo, hi = CLIP_BAND
    clear = not (((q >= lo) & (q <= hi)).any() or ((1.0 - q >= lo) & (1.0 - q <= hi)).any())
    return qt < 1e-9, omt < 1e-9, (qt > hi) & (omt > hi), clear


def metrics_case(N, K, seed=0):
    """One batch for asr_batch_metrics: (probs float32 [N, K], onehot float32).
    Rows that do not sum to 1 (scaled by 0.7 / 1.3: renormalisation), entries
    of 1e-9 (below the clip, on the true class in every 7th row), and in
    every 3rd row an exactly tied maximum at the index pairs (0, 3) and
    (2, K-1) alternately ((0, K-1) where K < 4), the target on the first
    index in one tied row and on the second in the next: the count must
    follow np.argmax (first maximum).  tie_rows() lists the tied rows."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 1.0, (N, K))
    p /= p.sum(axis=-1, keepdims=True)
    labels = rng.integers(0, K, N)
    p *= np.where(np.arange(N) % 4 == 1, 0.7, np.where(np.arange(N) % 4 == 2, 1.3, 1.0))[:, None]
    p = p.astype(np.float32)
    for r, i, j in tie_rows(N, K):
        p[r, i] = p[r, j] = np.float32(2.0) * p[r].max()
        labels[r] = i if (r // 3) % 4 < 2 else j
    for r in range(1, N, 7):  # (rows r % 3 == 0 are the tied ones)
        if r % 3:
            p[r, labels[r]] = np.float32(1e-9)
        if (r + 2) % 3 and K > 1 and r + 2 < N:
            p[r + 2, (labels[r + 2] + 1) % K] = np.float32(1e-9)
    return p, np.eye(K, dtype=np.float32)[labels]


def tie_rows(N, K):
    """[(row, i, j)]: rows of metrics_case whose maximum is tied at i < j."""
    if K < 2:
        return []
    pairs = [(0, 3), (2, K - 1)] if K >= 4 else [(0, K - 1)]
    return [(r, *pairs[(r // 3) % len(pairs)]) for r in range(0, N, 3)]


def assert_grad_groups_rel_l2(spec, got, want, tol=2e-2):
    """bf16 network gradients vs the fp64 oracle: relative L2 <= tol per
    gradient group."""
    bad = []
    for (name, a), (_, b) in zip(grad_groups(spec, got), grad_groups(spec, want)):
        if np.linalg.norm(b) == 0:
            assert np.linalg.norm(a) == 0, name
            continue
        e = rel_l2(a, b)
        if not e <= tol:
            bad.append(f"{name}: rel-L2 {e:.3e}")
    assert not bad, "; ".join(bad)
