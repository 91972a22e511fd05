"""CPU checks of tools/isa_equiv.py (no GPU needed): kernels are matched by symbol across a
tree's sources, so that a kernel moved to another file compares as unchanged, a changed
instruction is pinned to its kernel, and a symbol that two sources of one side define (a
kernel template instantiated in two translation units) is reported."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_equiv  # noqa: E402

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

SCALE = "__global__ void k_scale(float* p, float s) { p[threadIdx.x] *= s; }"
SHIFT = "__global__ void k_shift(float* p, float s) { p[threadIdx.x] += s; }"


def tree(root, name, files):
    """a tree with the sources {file: [kernel definitions]} in its csrc directory"""
    d = root / name / isa_equiv.CSRC
    d.mkdir(parents=True)
    for f, kernels in files.items():
        (d / f).write_text("#include <hip/hip_runtime.h>\nnamespace asr {\n" + "\n".join(kernels) + "\n}\n")
    return str(root / name)


def compare(tmp_path, capsys, a, b, aliases=()):
    """(number of differences, the DIFF lines) of isa_equiv.compare on the trees a and b"""
    out = tmp_path / "asm"
    out.mkdir()
    n = isa_equiv.compare(tree(tmp_path, "a", a), tree(tmp_path, "b", b), str(out), aliases)
    lines = capsys.readouterr().out.strip().split("\n")
    assert lines[-1].startswith("isa_equiv: ") and lines[-1].endswith(f"{n} DIFF")
    return n, [l for l in lines[:-1] if not l.startswith("same ")]


def test_a_moved_kernel_is_the_same(tmp_path, capsys):
    n, diff = compare(tmp_path, capsys, {"one.hip": [SCALE, SHIFT]}, {"one.hip": [SHIFT], "two.hip": [SCALE]})
    assert n == 0 and diff == []


def test_a_moved_kernel_names_both_files(tmp_path, capsys):
    out = tmp_path / "asm"
    out.mkdir()
    assert isa_equiv.compare(tree(tmp_path, "a", {"one.hip": [SCALE]}), tree(tmp_path, "b", {"two.hip": [SCALE]}),
                             str(out)) == 0
    line = [l for l in capsys.readouterr().out.split("\n") if "k_scale" in l]
    assert len(line) == 1 and line[0].startswith("same one.hip -> two.hip ")


def test_a_changed_instruction_is_reported_for_its_kernel_alone(tmp_path, capsys):
    changed = SCALE.replace("*= s", "*= s + 1.f")
    n, diff = compare(tmp_path, capsys, {"one.hip": [SCALE, SHIFT]}, {"one.hip": [SHIFT], "two.hip": [changed]})
    assert n == 1 and len(diff) == 1
    assert diff[0].startswith("DIFF (instructions: ") and "k_scale" in diff[0] and "k_shift" not in diff[0]


def test_a_symbol_in_two_sources_of_one_side_is_reported(tmp_path, capsys):
    n, diff = compare(tmp_path, capsys, {"one.hip": [SCALE, SHIFT]}, {"one.hip": [SCALE, SHIFT], "two.hip": [SCALE]})
    assert n == 1 and len(diff) == 1
    assert diff[0].startswith("DIFF (defined in one.hip and two.hip of B)") and "k_scale" in diff[0]


def test_alias_maps_a_renamed_kernel_onto_its_predecessor(tmp_path, capsys):
    renamed = SCALE.replace("k_scale", "k_scale2")
    n, diff = compare(tmp_path, capsys, {"one.hip": [SCALE]}, {"two.hip": [renamed]}, [("8k_scale2", "7k_scale")])
    assert n == 0 and diff == []
