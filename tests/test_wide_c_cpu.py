"""Host-side acceptance of bf16 3 x 3 Euler blocks and networks at C in {128, 256} (no launch: the
config checks and workspace sizes of include/asr.h, the lowering's plan).  k_convbw / k_wgradbw take
these channel counts at every width of the bf16 set (W == 8 or W % 16 == 0); RK2, kernel_size 5 / 7
and every other channel count stay refused.
"""
import ctypes as ct

import pytest

from differential_equations_resnet_amd import _lib

MB = 1 << 20


@pytest.fixture(scope="module")
def lib():
    return _lib.load(build_if_missing=True)


def _net(C, W, N=4, H=8, L=2, integrator=0, kernel_size=0, param_kind=0, variant=0):
    return _lib.NetConfig(N, H, W, 3, C, L, 10, 0.5, 0.0, 0.0, 1.0, 0, _lib.ASR_BF16, 0, param_kind, 1, integrator,
                          variant, kernel_size, 0)


def test_abi_version(lib):
    assert lib.asr_abi_version() == 13 == _lib.ABI_VERSION


@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("W", [8, 16, 32, 48])
def test_wide_c_bf16_net_is_accepted_and_sized(lib, C, W):
    cfg = _net(C, W)
    assert lib.asr_net_workspace_bytes(ct.byref(cfg)) > 0, lib.asr_last_error()
    # the config check passes: the call gets as far as the workspace check
    assert lib.asr_net_prepare(ct.byref(cfg), None, 0) == _lib.ASR_E_WORKSPACE, lib.asr_last_error()
    assert lib.asr_net_param_count(ct.byref(cfg)) > 0


def test_wide_c_stages_check(lib):
    c = _lib.StagesConfig()
    c.N, c.H, c.W, c.Cin, c.num_classes, c.n_stages = 4, 32, 32, 3, 10, 3
    for i, (C, L, S) in enumerate([(64, 1, 0), (128, 1, 2), (256, 1, 2)]):
        c.C[i], c.L[i], c.stride[i] = C, L, S
    c.h, c.divide_by_stddev, c.dtype = 0.5, 1.0, _lib.ASR_BF16
    assert lib.asr_stages_check(ct.byref(c)) == _lib.ASR_OK, lib.asr_last_error()
    # no stage sizes anything by 512 slab rows (2.4 MB a row at C = 256: 1.2 GB)
    assert 0 < lib.asr_stages_workspace_bytes(ct.byref(c)) < 512 * MB


@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("shape", [(2, 5, 16), (512, 32, 32)])
def test_wide_c_conv_backward_workspace_is_bounded(lib, C, shape):
    """At most 48 MB of slabs (<= 81 rows of 590 KB at C = 128, <= 20 of 2.36 MB at 256) plus
    reduce_and_project's group rows: 64 MB at most, whatever N, H, W."""
    n = lib.asr_conv_backward_workspace_bytes(*shape, C, _lib.ASR_BF16)
    assert 0 < n <= 64 * MB, n
    # the stack ABI's per-block sequence: that workspace and two gradient buffers
    act = shape[0] * shape[1] * shape[2] * C * 2
    assert n < lib.asr_block_stack_backward_workspace_bytes(*shape, C, 2, _lib.ASR_BF16) <= n + 2 * act + 1024


def test_wide_c_net_workspace_has_no_512_row_term(lib):
    """(N=4, H=8, W=16, Cin=3, C=256, L=2, training): <= 64 MB backward workspace, <= 48 MB alternate
    slab set, < 30 MB for everything else at this size (two 1.18 MB packs, two 2.36 MB index maps,
    group rows, the stem's 512 x 7168-float slabs = 14.7 MB, activations of 0.26 MB)."""
    n = lib.asr_net_workspace_bytes(ct.byref(_net(256, 16)))
    assert 0 < n < 192 * MB, n


def _refused(lib, cfg, *needles):
    assert lib.asr_net_workspace_bytes(ct.byref(cfg)) == 0
    assert lib.asr_net_prepare(ct.byref(cfg), None, 0) == _lib.ASR_E_UNSUPPORTED
    msg = lib.asr_last_error()
    for s in needles:
        assert s.encode() in msg, msg


def test_still_refused(lib):
    _refused(lib, _net(128, 32, integrator=1), "RK2", "C=128")
    _refused(lib, _net(128, 16, kernel_size=5, param_kind=_lib.ASR_PARAM_GENERAL), "C=128")
    _refused(lib, _net(48, 16), "C=48")
    _refused(lib, _net(96, 16), "C=96")
    _refused(lib, _net(512, 16), "C=512")
    # the single-layer ABI too, before any launch (the pointers are never dereferenced)
    p = ct.c_void_p(256)
    for C in (48, 96, 512):
        assert lib.asr_conv_forward(_lib.ASR_MODE_EULER, p, p, None, p, None, 0.5, 1, 4, 16, C, _lib.ASR_BF16,
                                    None) == _lib.ASR_E_UNSUPPORTED
        assert f"C={C}".encode() in lib.asr_last_error()
    assert lib.asr_rk2_forward(p, ct.c_void_p(512), ct.c_void_p(1024), None, None, p, None, 0.5, 1, 4, 32, 128,
                               _lib.ASR_BF16, None) == _lib.ASR_E_UNSUPPORTED
    assert b"C=128" in lib.asr_last_error()


def test_wide_c_model_plans_in_bf16():
    from differential_equations_resnet_amd.graph import Input
    from differential_equations_resnet_amd.lowering import StagesPlan, analyze
    from differential_equations_resnet_amd.models import tfkeras_resnets as R
    fn = R.get_single_block_resnet_build_function(kernel_type="antisymmetric", h=0.5, num_stages=4,
                                                  blocks_per_stage=[1, 2, 2], filters_per_block=[64, 128, 256],
                                                  strides=[(1, 1), (2, 2), (2, 2)], subtract_mean=127.5,
                                                  divide_by_stddev=127.5, num_classes=10)
    p = analyze(fn(Input(shape=(32, 32, 3))))
    # (a stage that changes shape spends its first block on the transition: [1, 2, 2] is one Euler block each)
    assert isinstance(p, StagesPlan) and [tuple(s) for s in p.stages] == [(64, 1, 0), (128, 1, 2), (256, 1, 2)]
    assert p.stages_bf16_ok()  # what NativeModel.resolve_dtype("bfloat16") asks: bf16 with no warning
