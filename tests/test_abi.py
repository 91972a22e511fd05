"""CPU tests of the C ABI: libasr.so builds/loads, exports every symbol
declared in include/asr.h, and its host-side pure functions (parameter maps,
sizes) agree with the oracle.  No kernel is launched here (no GPU)."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from oracle import asr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from differential_equations_resnet_amd import _lib
    return _lib.load(build_if_missing=True)


def header_functions():
    text = open(os.path.join(ROOT, "include", "asr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(asr_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported(lib):
    names = header_functions()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/asr.h but not exported"


def test_python_binding_covers_header():
    from differential_equations_resnet_amd import _lib
    bound = {n for n, _, _ in _lib.SIGNATURES}
    assert bound == set(header_functions())


def test_abi_version_and_errors(lib):
    from differential_equations_resnet_amd import _lib
    assert lib.asr_abi_version() == _lib.ABI_VERSION
    assert lib.asr_theta_count(0, 0, 1) < 0
    # a bad-argument call reports through asr_last_error without a GPU
    rc = lib.asr_param_map(0, 0, 1, None, None)
    assert rc == -1
    assert b"asr_param_map" in lib.asr_last_error()


@pytest.mark.parametrize("C", [1, 2, 5, 16, 64])
def test_param_map_3by3_matches_oracle(lib, C):
    n = lib.asr_theta_count(C, 0, 1)
    assert n == O.theta_count_3by3(C)
    w_src = np.empty(9 * C * C, np.int32)
    dst = np.empty(2 * n, np.int32)
    assert lib.asr_param_map(C, 0, 1, w_src.ctypes.data, dst.ctypes.data) == 0
    src, sign = O.param_map(C)
    want = np.where(src >= 0, (src << 1) | (sign < 0), -1)
    assert np.array_equal(w_src, want)
    # theta_dst is the exact inverse: every theta entry feeds 2 W entries with opposite-sign pairs
    for j in range(n):
        es = [v >> 1 for v in dst[2 * j:2 * j + 2] if v >= 0]
        assert len(es) == 2
        for e in es:
            assert w_src[e] >> 1 == j


@pytest.mark.parametrize("C,anti", [(3, True), (6, True), (4, False)])
def test_param_map_general_matches_oracle(lib, C, anti):
    n = lib.asr_theta_count(C, 1, int(anti))
    assert n == O.theta_count_general(C, 3, anti)
    w_src = np.empty(9 * C * C, np.int32)
    dst = np.empty(2 * n, np.int32)
    assert lib.asr_param_map(C, 1, int(anti), w_src.ctypes.data, dst.ctypes.data) == 0
    src, sign = O.param_map(C, "general", 3, anti)
    assert np.array_equal(w_src, np.where(src >= 0, (src << 1) | (sign < 0), -1))


def test_projection_through_map_is_autodiff(lib):
    """dtheta from the ABI's theta_dst pull-back == oracle project_dW."""
    C = 5
    n = lib.asr_theta_count(C, 0, 1)
    w_src = np.empty(9 * C * C, np.int32)
    dst = np.empty(2 * n, np.int32)
    lib.asr_param_map(C, 0, 1, w_src.ctypes.data, dst.ctypes.data)
    dW = np.random.default_rng(0).standard_normal(9 * C * C)
    got = np.zeros(n)
    for j in range(n):
        for v in dst[2 * j:2 * j + 2]:
            if v >= 0:
                got[j] += -dW[v >> 1] if v & 1 else dW[v >> 1]
    src, sign = O.param_map(C)
    assert np.allclose(got, O.project_dW(dW, src, sign, n))


def test_sizes(lib):
    from differential_equations_resnet_amd import _lib
    assert lib.asr_wpack_elems(64) == 4 * 18 * 64 * 8
    assert lib.asr_wpack_elems(16) == 1 * 5 * 64 * 8
    assert lib.asr_wpack_elems(20) < 0
    assert lib.asr_mask_bytes(2, 32, 32, 64) == 2 * 32 * 32 * 64 // 8
    assert lib.asr_conv_backward_workspace_bytes(2, 32, 32, 64, 1) > 0
    cfg = _lib.NetConfig(512, 32, 32, 3, 64, 30, 10, 8 / 30, 0.0, 127.5, 127.5, 1, 1, 1, 0, 1)
    assert lib.asr_net_param_count(ct.byref(cfg)) == O.NetSpec(C=64, L=30).n_params()
    ws = lib.asr_net_workspace_bytes(ct.byref(cfg))
    assert 2e9 < ws < 8e9  # activations of 31 layers + masks + slabs
    bad = _lib.NetConfig(512, 32, 24, 3, 64, 30, 10, 0.1, 0.0, 0.0, 1.0, 0, 1, 1, 0, 1)  # bf16 needs W == 32
    assert lib.asr_net_workspace_bytes(ct.byref(bad)) == 0


def test_netparams_layout_matches_oracle():
    from differential_equations_resnet_amd import netparams
    assert netparams.net_param_shapes(16, 3) == O.NetSpec(C=16, L=3).param_shapes()
    flat = netparams.init_net_params(16, 3, seed=1)
    assert flat.dtype == np.float32 and flat.size == O.NetSpec(C=16, L=3).n_params()


def test_net_param_count_per_kind(lib):
    from differential_equations_resnet_amd import _lib
    for kind, anti in [(0, 1), (1, 1), (1, 0), (2, 0)]:
        cfg = _lib.NetConfig(4, 8, 8, 3, 6, 2, 10, 0.5, 0.0, 0.0, 1.0, 0, 0, 1, kind, anti)
        nt = lib.asr_theta_count(6, kind, anti)
        assert lib.asr_net_param_count(ct.byref(cfg)) == 27 * 6 + 6 + 2 * (nt + 6) + 6 * 10 + 10
    bad = _lib.NetConfig(4, 8, 8, 3, 6, 2, 10, 0.5, 0.0, 0.0, 1.0, 0, 0, 1, 0, 0)
    assert lib.asr_net_param_count(ct.byref(bad)) == -1


@pytest.mark.parametrize("kind,anti", [(0, 1), (1, 1), (1, 0), (2, 0)])
def test_transposed_operator_map(lib, kind, anti):
    """asr_param_map_transpose gives W_bwd = -flip(W)^T; for antisymmetric
    kinds that equals W with the centre negated (so A^T = -A + 2 gamma I)."""
    C = 5
    n = lib.asr_theta_count(C, kind, anti)
    w_src = np.empty(9 * C * C, np.int32)
    lib.asr_param_map(C, kind, anti, w_src.ctypes.data, None)
    th = np.random.default_rng(kind).standard_normal(n)
    W = np.where(w_src >= 0, th[np.maximum(w_src, 0) >> 1] * np.where(w_src & 1, -1.0, 1.0), 0.3).reshape(3, 3, C, C)
    want = -W[::-1, ::-1].transpose(0, 1, 3, 2)
    assert lib.asr_param_is_antisymmetric(kind, anti) == (1 if (kind == 0 or (kind == 1 and anti)) else 0)
    wb = np.empty_like(w_src)
    rc = lib.asr_param_map_transpose(C, w_src.ctypes.data, wb.ctypes.data)
    if lib.asr_param_is_antisymmetric(kind, anti):
        assert rc == -1  # constant centre: the forward W (with the identity) is used instead
        Wg = W.copy()
        for o in range(C):
            Wg[1, 1, o, o] = -0.3
        assert np.array_equal(want, Wg)
    else:
        assert rc == 0
        Wb = (th[wb >> 1] * np.where(wb & 1, -1.0, 1.0)).reshape(3, 3, C, C)
        assert np.array_equal(Wb, want)


def test_theta_to_w_mirror_checks_its_arguments(lib):
    """asr_theta_to_w_mirror (ABI 13: W_bwd as the forward pack's mirror) refuses bad arguments before
    any launch, under its own name."""
    from differential_equations_resnet_amd import _lib
    fake = ct.c_void_p(16)  # never dereferenced: the checks come first
    n = lib.asr_wpack_elems(16)
    assert lib.asr_theta_to_w_mirror(None, 10, 1, 16, fake, fake, n, _lib.ASR_BF16, None) == _lib.ASR_E_ARG
    assert b"asr_theta_to_w_mirror" in lib.asr_last_error()
    assert lib.asr_theta_to_w_mirror(fake, 10, 1, 16, fake, fake, n - 1, _lib.ASR_BF16, None) == _lib.ASR_E_ARG
    assert b"w_stride" in lib.asr_last_error()
    assert lib.asr_theta_to_w_mirror(fake, 10, 1, 20, fake, fake, n, _lib.ASR_BF16, None) == _lib.ASR_E_UNSUPPORTED
    assert lib.asr_theta_to_w_mirror(fake, 10, 1, 16, fake, fake, n, 7, None) == _lib.ASR_E_ARG  # dtype


def test_status_and_measurement_entry_points_without_gpu(lib):
    """Without a device the degraded-hand-off count cannot be read (an error
    code, not a count); kernel times need a recorded ASR_VARIANT_TIMED call on
    the current device; the test knob checks its range (no kernel launches)."""
    from differential_equations_resnet_amd import _lib
    assert lib.asr_stack_status(0) < 0
    out = (ct.c_float * 3)()
    assert lib.asr_net_kernel_times(ct.cast(out, ct.c_void_p)) in (_lib.ASR_E_ARG, _lib.ASR_E_HIP)
    assert lib.asr_debug_stack_backward(-1) == _lib.ASR_E_ARG
    assert lib.asr_debug_stack_backward(513) == _lib.ASR_E_ARG
    assert lib.asr_debug_stack_backward(0) == 0


def test_inference_workspace_is_bounded(lib):
    """ASR_VARIANT_INFERENCE: x_0 + two activation slots instead of L+1
    activations, masks and backward buffers; unknown variant bits fail."""
    from differential_equations_resnet_amd import _lib
    for C, L, dt in ((64, 30, 1), (16, 18, 0), (16, 108, 1)):
        tr = _lib.NetConfig(512, 32, 32, 3, C, L, 10, 8 / L, 0.0, 127.5, 127.5, 1, dt, 1, 0, 1, 0, 0)
        inf = _lib.NetConfig(512, 32, 32, 3, C, L, 10, 8 / L, 0.0, 127.5, 127.5, 1, dt, 1, 0, 1, 0,
                             _lib.ASR_VARIANT_INFERENCE)
        a, b = lib.asr_net_workspace_bytes(ct.byref(tr)), lib.asr_net_workspace_bytes(ct.byref(inf))
        act = 512 * 32 * 32 * C * (2 if dt else 4)
        assert 0 < b < a and b < 3 * act + 64 * 2 ** 20, (C, L, a, b)
    bad = _lib.NetConfig(512, 32, 32, 3, 64, 30, 10, 0.1, 0.0, 127.5, 127.5, 1, 1, 1, 0, 1, 0, 1 << 12)
    assert lib.asr_net_workspace_bytes(ct.byref(bad)) == 0


def test_fused_c16_forward_checks_weight_stride(lib):
    """The fused C=16 stack reads packed per-layer weights back to back, so
    asr_block_stack_forward refuses any other w_stride (as the backward
    does) before launching anything."""
    from differential_equations_resnet_amd import _lib
    C, N, L = 16, 2, 3
    fake = ct.c_void_p(16)  # never dereferenced: the check comes first
    act = N * 32 * 32 * C
    rc = lib.asr_block_stack_forward(fake, fake, act, None, 0, fake, lib.asr_wpack_elems(C) + 8, None, 0,
                                     ct.c_float(0.1), N, 32, 32, C, L, _lib.ASR_BF16, 1, None)
    assert rc == _lib.ASR_E_ARG


STAGE_IMG_SHAPES = [(1, 16, 32), (1, 8, 64), (1, 8, 32), (0, 16, 32), (0, 8, 64)]  # (dtype, H = W, C), asr_api.hip


@pytest.mark.parametrize("dt,HW,C", STAGE_IMG_SHAPES)
def test_stage_img_stack_checks_strides(lib, dt, HW, C):
    """At an image-resident stage shape the stack ABI refuses, before any launch, every per-layer
    stride its kernels' vector accesses cannot take: y_stride % 4 (8-B / 16-B y stores),
    mask_stride % 2 (2-B mask stores), bias_stride % 4 (16-B loads), x_stride % 8 (bf16) or % 4
    (fp32) in the backward's weight gradient and, in bf16, w_stride % 8 (16-B fragment loads; the
    fp32 kernels read W with scalar loads)."""
    from differential_equations_resnet_amd import _lib
    N, L = 3, 2
    fake = ct.c_void_p(256)  # never dereferenced: the checks come first
    P, mb = N * HW * HW * C, lib.asr_mask_bytes(N, HW, HW, C)
    wst = lib.asr_wpack_elems(C) if dt == _lib.ASR_BF16 else 9 * C * C
    assert P % 8 == 0 and mb % 2 == 0 and wst % 8 == 0

    def fwd(y=P, m=mb, w=wst, b=C):
        return lib.asr_block_stack_forward(fake, fake, y, fake, m, fake, w, fake, b, ct.c_float(0.1), N, HW, HW, C, L,
                                           dt, 1, None)

    bad = [("y_stride", dict(y=P + 2)), ("mask_stride", dict(m=mb + 1)), ("bias_stride", dict(b=C + 2))]
    if dt == _lib.ASR_BF16:
        bad.append(("w_stride", dict(w=wst + 4)))
    for name, kw in bad:
        assert fwd(**kw) == _lib.ASR_E_ARG, kw
        assert name in lib.asr_last_error().decode()
    need = lib.asr_block_stack_backward_workspace_bytes(N, HW, HW, C, L, dt)

    def bwd(x=P, w=wst, ws_bytes=need):
        return lib.asr_block_stack_backward(fake, fake, x, fake, mb, fake, w, fake, 8, ct.c_float(0.1),
                                            ct.c_float(0.0), N, HW, HW, C, L, dt, fake, fake, fake, ws_bytes, None)

    assert bwd(x=P + (4 if dt == _lib.ASR_BF16 else 2)) == _lib.ASR_E_ARG
    if dt == _lib.ASR_BF16:
        assert bwd(w=wst + 4) == _lib.ASR_E_ARG
    assert bwd(ws_bytes=need - 1) == _lib.ASR_E_WORKSPACE


@pytest.mark.parametrize("dt,HW,C", STAGE_IMG_SHAPES)
def test_stage_img_stack_workspace_size(lib, dt, HW, C):
    """asr_block_stack_backward_workspace_bytes at an image-resident stage shape holds the
    gradient entering every layer (L activations) and L layers' weight-gradient slabs of at
    least one [dW | db] row each; it grows with L by at least that much."""
    from differential_equations_resnet_amd import _lib
    N = 5
    act = N * HW * HW * C * (2 if dt == _lib.ASR_BF16 else 4)
    row = (9 * C * C + C) * 4
    sizes = [lib.asr_block_stack_backward_workspace_bytes(N, HW, HW, C, L, dt) for L in (1, 2, 3)]
    for L, b in zip((1, 2, 3), sizes):
        assert b >= L * (act + row), (L, b)
    assert sizes[1] - sizes[0] >= act + row and sizes[2] - sizes[1] >= act + row


def test_forward_backward_rejects_inference_workspace_before_launching(lib):
    """asr_net_forward_backward on an ASR_VARIANT_INFERENCE workspace fails with
    ASR_E_ARG before any launch, for every parameter kind (the regular kind's
    inference layout has no transposed-operator map: a late check let its
    W_bwd materialisation read the absent map first)."""
    from differential_equations_resnet_amd import _lib
    fake = ct.c_void_p(16)  # never dereferenced: the check comes first
    for kind, anti in ((_lib.ASR_PARAM_REGULAR, 0), (_lib.ASR_PARAM_GENERAL, 0), (_lib.ASR_PARAM_3BY3, 1)):
        cfg = _lib.NetConfig(8, 32, 32, 3, 64, 3, 10, 0.1, 0.0, 127.5, 127.5, 1, _lib.ASR_BF16, 1, kind, anti, 0,
                             _lib.ASR_VARIANT_INFERENCE)
        wsb = lib.asr_net_workspace_bytes(ct.byref(cfg))
        assert wsb > 0
        rc = lib.asr_net_forward_backward(ct.byref(cfg), fake, fake, fake, fake, fake, None, fake, wsb, None)
        assert rc == _lib.ASR_E_ARG, (kind, rc)
        assert "INFERENCE" in lib.asr_last_error().decode()


def _pair_slab_from_dW(dW):
    """The pair-local slab of the C=64 stacked backward (asr.h, asr_param_map_pair),
    restated from its documented layout: 74 tiles of D = dW - dW*^T, then db."""
    C = 64
    W = dW.reshape(9, C, C)
    slab = np.zeros(74 * 256)

    def put(T, tile):  # element (r, c) of tile T at T*256 + ((r/4)*16 + c)*4 + r%4
        r, c = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
        slab[T * 256 + ((r // 4) * 16 + c) * 4 + r % 4] = tile

    for p in range(4):
        for a in range(4):
            for b in range(4):
                put(16 * p + 4 * a + b, W[p, 16 * a:16 * a + 16, 16 * b:16 * b + 16]
                    - W[8 - p, 16 * b:16 * b + 16, 16 * a:16 * a + 16].T)
    for k, (a, b) in enumerate([(1, 0), (2, 0), (3, 1), (3, 2), (1, 2), (0, 3)]):
        put(64 + k, W[4, 16 * a:16 * a + 16, 16 * b:16 * b + 16] - W[4, 16 * b:16 * b + 16, 16 * a:16 * a + 16].T)
    for c in range(4):
        X = W[4, 16 * c:16 * c + 16, 16 * c:16 * c + 16]
        put(70 + c, X.T if c & 1 else X)
    return slab


@pytest.mark.parametrize("kind,anti", [(0, 1), (1, 1)])
def test_pair_map_projects_like_the_full_dW(lib, kind, anti):
    """asr_param_map_pair (the stacked backward's pull-back from its pair-local
    slabs) gives every theta the same dtheta as the full-dW projection (the
    oracle's project_dW), exactly in float64 (the same two terms); a
    non-antisymmetric parametrisation is refused."""
    C = 64
    n = lib.asr_theta_count(C, kind, anti)
    w_src = np.empty(9 * C * C, np.int32)
    dst = np.empty(2 * n, np.int32)
    assert lib.asr_param_map(C, kind, anti, w_src.ctypes.data, dst.ctypes.data) == 0
    pr = np.empty(2 * n, np.int32)
    assert lib.asr_param_map_pair(C, dst.ctypes.data, n, pr.ctypes.data) == 0
    dW = np.random.default_rng(3).standard_normal(9 * C * C)
    slab = _pair_slab_from_dW(dW)
    got = np.zeros(n)
    for q in range(2):
        v = pr[q::2]
        ok = v >= 0
        got[ok] += np.where(v[ok] & 1, -1.0, 1.0) * slab[v[ok] >> 1]
    src, sign = O.param_map(C, "3by3" if kind == 0 else "general", 3, bool(anti))
    assert np.array_equal(got, O.project_dW(dW, src, sign, n))
    # the regular kind (no antisymmetry) has no pair-local pull-back
    nr = lib.asr_theta_count(C, 2, 0)
    w2 = np.empty(9 * C * C, np.int32)
    d2 = np.empty(2 * nr, np.int32)
    assert lib.asr_param_map(C, 2, 0, w2.ctypes.data, d2.ctypes.data) == 0
    p2 = np.empty(2 * nr, np.int32)
    from differential_equations_resnet_amd import _lib
    assert lib.asr_param_map_pair(C, d2.ctypes.data, nr, p2.ctypes.data) == _lib.ASR_E_ARG


@pytest.mark.parametrize("k", [1, 5, 7])
@pytest.mark.parametrize("anti", [True, False])
def test_general_k_param_map_matches_oracle(lib, k, anti):
    """asr_param_map_k for Conv2DAntisymmetric(kernel_size=k) == the oracle's
    map of …Conv2DAntisymmetric.py:109-145, :216-270 (exact), theta counts
    included; the 3by3 kind takes only k=3, even sizes are refused."""
    from differential_equations_resnet_amd import _lib
    C = 6
    n = lib.asr_theta_count_k(C, k, 1, int(anti))
    assert n == sum(int(np.prod(s)) for s in O.theta_shapes_general(C, k, anti)[0])
    w_src = np.empty(k * k * C * C, np.int32)
    dst = np.empty(2 * n, np.int32)
    assert lib.asr_param_map_k(C, k, 1, int(anti), w_src.ctypes.data, dst.ctypes.data) == 0
    src, sign = O.param_map(C, "general", k, anti)
    assert np.array_equal(w_src, np.where(src >= 0, (src << 1) | (sign < 0), -1))
    assert lib.asr_theta_count_k(C, 5, 0, 1) < 0 and lib.asr_theta_count_k(C, 4, 1, 1) < 0
    assert lib.asr_param_map_k(C, 4, 1, 1, w_src.ctypes.data, None) == _lib.ASR_E_ARG
