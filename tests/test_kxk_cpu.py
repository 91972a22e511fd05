"""CPU checks of the bf16 k x k path (asr_conv_kxk.hip; no GPU needed): the sizes and argument
checks of its C entry points, and the gfx950 ISA of its kernels (the audits of tests/test_isa.py:
no early read of an inline-asm LDS read or of an MFMA result, no spills, no scratch)."""
import ctypes as ct
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "differential_equations_resnet_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import asm_lds_audit  # noqa: E402
import asm_mfma_audit  # noqa: E402

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SUPPORTED = [(k, C, W) for k in (5, 7) for C in (16, 32, 64) for W in (8, 16, 32)]


@pytest.fixture(scope="module")
def lib():
    from differential_equations_resnet_amd import _lib
    return _lib.load(build_if_missing=True)


def test_wpack_elems_k(lib):
    for k, C, _ in SUPPORTED:
        assert lib.asr_wpack_elems_k(C, k) == (C // 16) * ((k * k * C + 31) // 32) * 512
    for C, k in ((64, 1), (64, 3), (64, 9), (64, 15), (64, 6), (12, 5), (48, 7), (128, 5), (0, 5)):
        assert lib.asr_wpack_elems_k(C, k) < 0, (C, k)


def test_backward_workspace_is_bounded(lib):
    """Positive and <= 64 MB over the supported set at N = 512, H = 32 (asr.h: the slab count is
    bounded by 48 MB of slabs); 0 outside the set."""
    for k, C, W in SUPPORTED:
        for N, H in ((512, 32), (1, 1), (3, 7)):
            b = lib.asr_conv_backward_workspace_bytes_k_bf16(N, H, W, C, k)
            assert 0 < b <= 64 * 2 ** 20, (k, C, W, N, H, b)
            assert b >= (k * k * C * C + C) * 4
    for N, H, W, C, k in ((2, 8, 16, 16, 9), (2, 8, 16, 16, 3), (2, 8, 12, 16, 5), (2, 8, 16, 12, 5), (0, 8, 16, 16, 5)):
        assert lib.asr_conv_backward_workspace_bytes_k_bf16(N, H, W, C, k) == 0


def test_argument_checks(lib):
    """Null and bad arguments return ASR_E_ARG, the unsupported set ASR_E_UNSUPPORTED with a message
    naming the supported one -- before any launch (the pointers are never dereferenced)."""
    from differential_equations_resnet_amd import _lib
    p = ct.c_void_p(16)
    h = ct.c_float(0.5)
    g = ct.c_float(0.0)

    def fwd(mode=0, k=5, x=p, y=p, w=p, N=2, H=8, W=16, C=16):
        return lib.asr_conv_forward_k_bf16(mode, k, x, y, None, w, None, h, N, H, W, C, None)

    def bwd(mode=1, k=5, dy=p, x=p, mask=None, w=p, tdst=p, dth=None, N=2, H=8, W=16, C=16, ws=p, wsb=1 << 30):
        return lib.asr_conv_backward_k_bf16(mode, k, dy, x, mask, w, tdst, 10, h, g, N, H, W, C, p, dth, None, None,
                                            ws, wsb, None)

    def pack(k=5, C=16, theta=p, src=p, out=p, L=1, stride=1 << 30):
        return lib.asr_theta_to_w_k_bf16(theta, 10, L, C, k, src, g, out, stride, None)

    for rc in (fwd(x=None), fwd(y=None), fwd(w=None), fwd(mode=2), fwd(k=4), fwd(k=17), fwd(k=0), fwd(N=0),
               bwd(dy=None), bwd(w=None), bwd(mode=0, mask=None), bwd(mode=3), bwd(k=6), bwd(H=0),
               bwd(dth=p, x=None), bwd(dth=p, tdst=None),
               pack(theta=None), pack(src=None), pack(out=None), pack(L=0), pack(k=4), pack(stride=8)):
        assert rc == _lib.ASR_E_ARG
    assert bwd(ws=None) == _lib.ASR_E_WORKSPACE and bwd(wsb=1024) == _lib.ASR_E_WORKSPACE
    for call in (lambda: fwd(k=9), lambda: fwd(k=1), lambda: fwd(k=3), lambda: fwd(C=12), lambda: fwd(W=12),
                 lambda: fwd(C=128), lambda: bwd(k=9), lambda: bwd(k=15), lambda: bwd(C=48), lambda: bwd(W=64),
                 lambda: pack(k=9), lambda: pack(C=12)):
        assert call() == _lib.ASR_E_UNSUPPORTED
        msg = lib.asr_last_error().decode()
        assert "kernel_size in {5, 7}" in msg and "C in {16, 32, 64}" in msg and "W in {8, 16, 32}" in msg, msg


def test_python_entry_points_refuse_without_touching_the_device():
    from differential_equations_resnet_amd import _lib, runtime
    for C, k in ((16, 9), (12, 5), (16, 1)):
        with pytest.raises(_lib.AsrUnsupported, match="5, 7"):
            runtime.wpack_elems_k(C, k)
    assert runtime.wpack_elems_k(64, 7) == 4 * 98 * 512


@pytest.fixture(scope="module")
def kxk_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    from test_isa import FLAGS
    out = str(tmp_path_factory.mktemp("kxk") / "asr_conv_kxk.s")
    res = subprocess.run([HIPCC] + FLAGS + ["-o", out, os.path.join(CSRC, "asr_conv_kxk.hip")], capture_output=True,
                         text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return open(out).read()


def test_kxk_isa_audits_clean(kxk_asm):
    bad, findings = asm_lds_audit.audit(kxk_asm)
    assert bad == 0, "\n".join(findings[:10])
    bad, findings = asm_mfma_audit.audit(kxk_asm)
    assert bad == 0, "\n".join(findings[:10])
    assert kxk_asm.count("v_mfma_f32_16x16x32_bf16") > 1000


def test_kxk_kernels_do_not_spill(kxk_asm):
    """Every kernel of the file: 0 VGPR spills, 0 scratch bytes; all 72 conv and 36 weight-gradient
    instantiations of the supported set are in the build."""
    from test_isa import kernel_metadata
    md = kernel_metadata(kxk_asm)
    conv = [n for n in md if "k_convk" in n]
    wgrad = [n for n in md if "k_wgradk" in n]
    assert len(conv) == 72 and len(wgrad) == 36 and len(md) == 108, (len(conv), len(wgrad), len(md))
    for name, m in md.items():
        assert m["vgpr_spill"] == 0 and m["scratch"] == 0, (name, m)
