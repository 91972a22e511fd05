"""CPU checks on the gfx950 ISA of the product kernels (no GPU needed).

The C=64 and C=16 stack kernels rely on hand-counted waits around inline-asm
LDS reads and LDS-DMA, which the compiler cannot see:
  * an inline-asm LDS read's result register must not be read (copied,
    spilled to scratch or AGPRs, or used) before an `s_waitcnt lgkmcnt` that
    retires it: hipcc treats an asm output as available at once.  The audit
    (tools/asm_lds_audit.py) models lgkmcnt as an in-order queue per basic
    block; it must find nothing in any product source, and it must flag a
    kernel that reintroduces the hazard (self-test below);
  * the same for the untracked global loads (gload128_untracked /
    gload32_untracked: the stacks' per-block weight and bias reloads, which
    the next item's barrier_vm retires): tools/asm_vmem_audit.py walks the
    control-flow graph from each such load and flags any instruction that
    touches its registers before a retiring vmcnt wait or barrier_vm's
    barrier (self-test below);
  * MFMA results: no instruction may read or write an MFMA's D registers
    before the result's wait states have passed, on any control-flow path
    from the MFMA (tools/asm_mfma_audit.py).  hipcc pads a join block for one
    predecessor only: the shipped fp32 k_conv32 forward read its accumulator
    2 states early on one epilogue path and a persistent-band k_conv32 (the
    fixture under tests/fixtures/) 5-6 early, which failed GPU parity;
  * register spills: a compiler-inserted scratch access only ever adds
    vector-memory ops, which makes a counted `vmcnt(n)` wait MORE conservative
    (it retires the oldest ops first), never less; but a spill is also where
    an asm result can be copied early, and it costs bandwidth.  The hot
    kernels are held to an explicit allow-list of spill counts and scratch
    bytes (the numbers of the measured production build, with the reason);
    any growth fails here and needs a new audit and a GPU parity run.
"""
import importlib.util
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "differential_equations_resnet_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import asm_lds_audit  # noqa: E402
import asm_mfma_audit  # noqa: E402
import asm_vmem_audit  # noqa: E402

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-w"]


def _build_sources():
    """_build.SOURCES, the one list of HIP sources (loaded by path: importing the package would build the library)"""
    spec = importlib.util.spec_from_file_location("_asr_build", os.path.join(os.path.dirname(CSRC), "_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.SOURCES)


KERNEL_SOURCES = _build_sources()  # every product source

# (kernel-name regex) -> (max VGPR spills, max scratch bytes, why)
SPILL_ALLOW = {
    r"k_bwd3_stackILi64ELi32ELi4ELb[01]ELb0E": (0, 0, "12-wave C=64 stacked backward at the 168-register cap of 3 "
                                                     "waves per SIMD, full-dW slabs: no spills (the wgrad operands' "
                                                     "two pixel tiles share one address register)"),
    r"k_bwd3_stackILi64ELi32ELi4ELb0ELb1E": (0, 0, "the production C=64 stacked backward (Euler, pair-local slabs): no "
                                                   "spills (a 16-channel tile's operand address is tile 0's XOR bits "
                                                   "5-6: one register per operand row)"),
    r"k_bwd3_stackILi64ELi32ELi4ELb1ELb1E": (0, 0, "its RK2 instantiation: no spills (the row-pipelined pair wgrad "
                                                   "accumulates D = X - Y^T in 40 registers instead of 72)"),
    r"k_bwd16_fusedILb0E": (8, 28, "12-wave fused C=16 backward at 168 registers (fp32 dx of 8 layers in the "
                                   "dgrad waves)"),
    r"k_bwd16_fusedILb1E": (12, 36, "its gamma != 0 instantiation (+ the dz tile term)"),
    r"k_bwd3ILi64ELi32ELi4ELi2ELb0ELb1E": (4, 20, "per-block backward, first RK2 stage (extra dx term in registers)"),
    r"k_fwd3_stack": (0, 0, "forward stack: no spills"),
    r"k_fwd16_fused": (0, 0, "fused C=16 forward: no spills"),
    r"k_fwd3I": (0, 0, "per-block forward: no spills"),
    r"k_bwd3ILi64ELi32ELi4ELi[23]ELb[01]ELb0E": (0, 0, "per-block backward (Euler, conv, relu'): no spills"),
}


def _compile(src, out):
    res = subprocess.run([HIPCC] + FLAGS + ["-o", out, src], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def asm_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa")
    jobs = [(os.path.join(CSRC, s), str(d / (s + ".s"))) for s in KERNEL_SOURCES]
    with ThreadPoolExecutor(min(len(jobs), os.cpu_count() or 1)) as pool:
        return list(pool.map(lambda a: _compile(*a), jobs))


def kernel_metadata(asm_text):
    out = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)(?=\n  - |\n\.end_amdgpu_metadata)", asm_text, re.S):
        body = m.group(2)

        def g(k):
            mm = re.search(r"\." + k + r":\s+(\d+)", body)
            return int(mm.group(1)) if mm else 0
        out[m.group(1)] = {"vgpr_spill": g("vgpr_spill_count"), "scratch": g("private_segment_fixed_size"),
                           "vgpr": g("vgpr_count")}
    return out


def test_asm_lds_audit_clean(asm_files):
    for f in asm_files:
        bad, findings = asm_lds_audit.audit(open(f).read())
        assert bad == 0, f"{os.path.basename(f)}: " + "\n".join(findings[:10])


def test_asm_lds_audit_catches_early_use(tmp_path):
    """A kernel that consumes an inline-asm LDS read before its lgkmcnt wait
    (the hazard class) is flagged; the same kernel with the wait first is not."""
    tmpl = r'''
#include <hip/hip_runtime.h>
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
extern "C" __global__ void k(unsigned* out, unsigned a) {
  __shared__ unsigned buf[1024];
  buf[threadIdx.x] = threadIdx.x;
  __syncthreads();
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(a + threadIdx.x * 16));
  WAIT
  out[threadIdx.x] = v[0] + v[1] + v[2] + v[3];
}
'''
    for wait, want_bad in (("", True), ('asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");', False)):
        src = tmp_path / ("k%d.hip" % want_bad)
        src.write_text(tmpl.replace("WAIT", wait))
        asm = _compile(str(src), str(src) + ".s")
        bad, _ = asm_lds_audit.audit(open(asm).read())
        assert (bad > 0) == want_bad, (wait, bad)


def test_asm_lds_audit_follows_branches():
    """The round-3 stacked-backward bug: an asm LDS read issued before a branch,
    its register copied after the join, its wait later.  The audit carries the
    pending read across the branch and the label, and flags the copy."""
    asm = """_Z1kv:                                   ; @_Z1kv
\t;;#ASMSTART
\tds_read_b128 v[114:117], v114
\t;;#ASMEND
\ts_cbranch_scc1 .LBB0_2
\ts_nop 0
.LBB0_2:
\tv_mov_b64_e32 v[110:111], v[114:115]
\ts_waitcnt lgkmcnt(0)
\ts_endpgm
"""
    bad, findings = asm_lds_audit.audit(asm)
    assert bad >= 1, findings
    assert asm_lds_audit.audit(asm.replace("\ts_nop 0\n", "\ts_waitcnt lgkmcnt(0)\n").replace(
        "\ts_cbranch_scc1 .LBB0_2\n", "\ts_waitcnt lgkmcnt(0)\n\ts_cbranch_scc1 .LBB0_2\n"))[0] == 0


def test_asm_vmem_audit_clean(asm_files):
    n_loads = 0
    for f in asm_files:
        text = open(f).read()
        n_loads += len(re.findall(r"global_load_dword\w* v", text.split(".end_amdgpu_metadata")[0]))
        bad, findings = asm_vmem_audit.audit(text)
        assert bad == 0, f"{os.path.basename(f)}: " + "\n".join(findings[:10])
    assert n_loads > 0


def test_asm_vmem_audit_catches_early_use(tmp_path):
    """An untracked global load whose result is used before any vmcnt wait is
    flagged; with the wait (or a barrier_vm-style wait + barrier) first it is not."""
    tmpl = r'''
#include <hip/hip_runtime.h>
extern "C" __global__ void k(float* out, const float* p) {
  float v = 0.f;
  asm volatile("global_load_dword %0, %1, off" : "+v"(v) : "v"(p + threadIdx.x) : "memory");
  WAIT
  out[threadIdx.x] = v * 2.f;
}
'''
    cases = (("", True), ('asm volatile("s_waitcnt vmcnt(0)" ::: "memory");', False),
             ('asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); asm volatile("s_waitcnt lgkmcnt(0)\\n\\ts_barrier" ::: "memory");',
              False))
    for i, (wait, want_bad) in enumerate(cases):
        src = tmp_path / ("v%d.hip" % i)
        src.write_text(tmpl.replace("WAIT", wait))
        asm = _compile(str(src), str(src) + ".s")
        bad, _ = asm_vmem_audit.audit(open(asm).read())
        assert (bad > 0) == want_bad, (wait, bad)


def test_hot_kernels_spill_allow_list(asm_files):
    seen = {k: 0 for k in SPILL_ALLOW}
    for f in asm_files:
        for name, md in kernel_metadata(open(f).read()).items():
            for pat, (vmax, smax, why) in SPILL_ALLOW.items():
                if re.search(pat, name):
                    seen[pat] += 1
                    assert md["vgpr_spill"] <= vmax and md["scratch"] <= smax, (
                        f"{name}: {md['vgpr_spill']} VGPR spills / {md['scratch']} B scratch exceed the allow-list "
                        f"({vmax} / {smax}: {why}); re-run the audit and the GPU parity tests before raising it")
    missing = [k for k, v in seen.items() if v == 0]
    assert not missing, f"allow-listed kernels not found in the build: {missing}"


def _probe_required(op_builtin, a_ty, tmp_path):
    """wait states hipcc puts between an MFMA and a dependent VALU read on a
    straight line (the audit's requirement table must match the toolchain)."""
    src = tmp_path / "probe.hip"
    src.write_text(r"""
#include <hip/hip_runtime.h>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
extern "C" __global__ void k(float* out, const A_TY* a) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = OP(a[threadIdx.x], a[threadIdx.x + 64], acc, 0, 0, 0);
  out[threadIdx.x] = acc[3] * 2.f;
}
""".replace("A_TY", a_ty).replace("OP", op_builtin))
    asm = open(_compile(str(src), str(src) + ".s")).read()
    m = re.search(r"v_mfma\w+[^\n]*\n\s*s_nop (\d+)\n\s*v_\w+[^\n]*v\d", asm)
    assert m, asm[:2000]
    return int(m.group(1)) + 1


def test_mfma_wait_state_table_matches_compiler(asm_files, tmp_path):
    probes = {"v_mfma_f32_16x16x32_bf16": ("__builtin_amdgcn_mfma_f32_16x16x32_bf16", "bf16x8"),
              "v_mfma_f32_16x16x4_f32": ("__builtin_amdgcn_mfma_f32_16x16x4f32", "float")}
    used = set()
    for f in asm_files:
        used |= set(re.findall(r"\b(v_mfma_\w+)", open(f).read()))
    assert used and used <= set(asm_mfma_audit.REQUIRED), f"MFMA opcodes without a requirement: {used - set(asm_mfma_audit.REQUIRED)}"
    for op, (builtin, ty) in probes.items():
        assert _probe_required(builtin, ty, tmp_path) == asm_mfma_audit.REQUIRED[op], op


def test_asm_mfma_audit_clean(asm_files):
    n_mfma = 0
    for f in asm_files:
        text = open(f).read()
        n_mfma += len(re.findall(r"\bv_mfma_", text))
        bad, findings = asm_mfma_audit.audit(text)
        assert bad == 0, f"{os.path.basename(f)}: " + "\n".join(findings[:10])
    assert n_mfma > 10000


def test_asm_mfma_audit_flags_persistent_band_fixture():
    """The reconstructed persistent-band k_conv32 (tools/pb_fixture.py): the
    epilogue reads a3 after 4-5 of the 10 states, on the path that enters the
    join by a branch from the last MFMA."""
    text = open(os.path.join(ROOT, "tests", "fixtures", "isa_k_conv32p_persistent_band.s")).read()
    bad, findings = asm_mfma_audit.audit(text)
    assert bad >= 1 and all("k_conv32p" in f and "v_accvgpr_read_b32" in f for f in findings), findings


def test_asm_mfma_audit_follows_branches():
    """Short path through a branch to the join: flagged; with the states
    spent before the branch: clean; an accumulate chain: clean."""
    asm = """_Z1kv:                                   ; @_Z1kv
\tv_mfma_f32_16x16x4_f32 a[0:3], v1, v2, a[0:3]
\tPAD
\ts_cbranch_vccnz .LBB0_2
\tv_mov_b32_e32 v9, 0
\tv_mov_b32_e32 v9, 1
\tv_mov_b32_e32 v9, 2
\tv_mov_b32_e32 v9, 3
.LBB0_2:
\ts_nop 4
\tv_accvgpr_read_b32 v5, a3
\ts_endpgm
"""
    assert asm_mfma_audit.audit(asm.replace("\tPAD\n", ""))[0] == 1
    assert asm_mfma_audit.audit(asm.replace("PAD", "s_nop 9"))[0] == 0
    chain = asm.replace("\tPAD\n", "\tv_mfma_f32_16x16x4_f32 a[4:7], v1, v2, a[0:3]\n\ts_nop 9\n").replace(
        "v_accvgpr_read_b32 v5, a3", "v_accvgpr_read_b32 v5, a7")
    assert asm_mfma_audit.audit(chain)[0] == 0
