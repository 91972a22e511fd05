"""Host-side acceptance of bf16 3 x 3 Euler blocks and networks at image
widths beyond 32 (no launch: the config checks and workspace sizes of
include/asr.h, the lowering's plan).  The column-strip kernels take every
W >= 48 with W % 16 == 0; W in {32, 16, 8} keep their kernels; any other
width stays refused.
"""
import ctypes as ct

import pytest

from differential_equations_resnet_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load(build_if_missing=True)


def _net(W, dtype=1, H=32, integrator=0, kernel_size=0):
    # test_abi.py::test_sizes' network (512 x 32 x W x 3, C = 64, L = 30, 3by3 antisymmetric, u8 input)
    return _lib.NetConfig(512, H, W, 3, 64, 30, 10, 8 / 30, 0.0, 127.5, 127.5, 1, dtype, 1, 0, 1, integrator, 0,
                          kernel_size, 0)


def test_wide_bf16_net_is_sized(lib):
    ws32 = lib.asr_net_workspace_bytes(ct.byref(_net(32)))
    ws48 = lib.asr_net_workspace_bytes(ct.byref(_net(48)))
    assert 2e9 < ws32 < 8e9  # (test_sizes' figure)
    assert ws48 > 0
    # activations, masks and gradients scale with W (x 1.5); the slab areas do not
    assert 1.3 * ws32 < ws48 < 1.6 * ws32, (ws32, ws48)
    assert lib.asr_net_param_count(ct.byref(_net(48))) == lib.asr_net_param_count(ct.byref(_net(32)))
    # W in {16, 8}: the kernels existed, the network check refused them
    for W in (16, 8):
        assert lib.asr_net_workspace_bytes(ct.byref(_net(W))) > 0, W


@pytest.mark.parametrize("W", [24, 40])
def test_width_not_a_multiple_of_16_stays_refused(lib, W):
    cfg = _net(W)
    assert lib.asr_net_workspace_bytes(ct.byref(cfg)) == 0
    assert lib.asr_net_prepare(ct.byref(cfg), None, 0) == _lib.ASR_E_UNSUPPORTED
    assert f"W={W}".encode() in lib.asr_last_error()


def test_wide_refusals_name_the_shape(lib):
    rk2 = _net(48, integrator=1)
    assert lib.asr_net_prepare(ct.byref(rk2), None, 0) == _lib.ASR_E_UNSUPPORTED
    assert b"RK2" in lib.asr_last_error() and b"W=48" in lib.asr_last_error()
    assert lib.asr_net_workspace_bytes(ct.byref(_net(32, integrator=1))) > 0
    k5 = _lib.NetConfig(8, 16, 48, 3, 64, 2, 10, 0.5, 0.0, 0.0, 1.0, 0, 1, 1, 1, 1, 0, 0, 5, 0)  # general kind, k = 5
    assert lib.asr_net_prepare(ct.byref(k5), None, 0) == _lib.ASR_E_UNSUPPORTED
    assert b"W=48" in lib.asr_last_error()
    c48 = _lib.NetConfig(8, 16, 48, 3, 48, 2, 10, 0.5, 0.0, 0.0, 1.0, 0, 1, 1, 0, 1)  # C = 48
    assert lib.asr_net_prepare(ct.byref(c48), None, 0) == _lib.ASR_E_UNSUPPORTED
    assert b"C=48" in lib.asr_last_error()


def _stages(W, stages, H=16, dtype=_lib.ASR_BF16):
    c = _lib.StagesConfig()
    c.N, c.H, c.W, c.Cin, c.num_classes, c.n_stages = 4, H, W, 3, 10, len(stages)
    for i, (C, L, S) in enumerate(stages):
        c.C[i], c.L[i], c.stride[i] = C, L, S
    c.h, c.divide_by_stddev, c.dtype = 0.5, 1.0, dtype
    return c


def test_wide_bf16_stages_check(lib):
    he = [(16, 2, 0), (32, 2, 2), (64, 2, 2)]  # W = 64 / 32 / 16 on a 16 x 64 input
    c = _stages(64, he)
    assert lib.asr_stages_check(ct.byref(c)) == _lib.ASR_OK
    bf_ws = lib.asr_stages_workspace_bytes(ct.byref(c))
    assert 0 < bf_ws < lib.asr_stages_workspace_bytes(ct.byref(_stages(64, he, dtype=_lib.ASR_F32)))
    # one more stride-2 stage: 64 / 32 / 16 / 8 is fine, from a 32-wide input the last stage is at W = 4
    deeper = he + [(64, 1, 2)]
    assert lib.asr_stages_check(ct.byref(_stages(64, deeper))) == _lib.ASR_OK
    assert lib.asr_stages_check(ct.byref(_stages(32, deeper, H=32))) == _lib.ASR_E_UNSUPPORTED
    assert b"W=4" in lib.asr_last_error()
    assert lib.asr_stages_check(ct.byref(_stages(40, he))) == _lib.ASR_E_UNSUPPORTED
    assert b"W=40" in lib.asr_last_error()


def test_wide_he_model_plans_in_bf16():
    from differential_equations_resnet_amd.graph import Input
    from differential_equations_resnet_amd.lowering import StagesPlan, analyze
    from differential_equations_resnet_amd.models import tfkeras_resnets as R
    fn = R.get_single_block_resnet_build_function(kernel_type="antisymmetric", h=0.5, num_stages=4,
                                                  blocks_per_stage=[2, 2, 2], filters_per_block=[16, 32, 64],
                                                  strides=[(1, 1), (2, 2), (2, 2)], subtract_mean=127.5,
                                                  divide_by_stddev=127.5, num_classes=10)
    p = analyze(fn(Input(shape=(16, 64, 3))))
    assert isinstance(p, StagesPlan) and (p.H, p.W) == (16, 64) and [s[0] for s in p.stages] == [16, 32, 64]
    assert p.stages_bf16_ok()  # what NativeModel.resolve_dtype("bfloat16") asks: bf16 with no warning
    p40 = analyze(fn(Input(shape=(16, 40, 3))))
    assert not p40.stages_bf16_ok()  # W = 40: float32, warned about


def test_wide_conv_backward_workspace(lib):
    assert lib.asr_conv_backward_workspace_bytes(2, 5, 48, 16, _lib.ASR_BF16) > 0
    assert lib.asr_block_stack_backward_workspace_bytes(2, 6, 48, 32, 3, _lib.ASR_BF16) > 0
