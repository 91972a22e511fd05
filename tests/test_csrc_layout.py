"""CPU checks on the layout of the HIP sources (no GPU needed).

  * every header of csrc/ compiles on its own (it includes what it uses);
  * every host function shared between translation units is declared once, in
    asr_internal.h, and defined once, in the .hip file the header groups it
    under: no .hip file re-declares it (a copy's default arguments could drift
    without any error);
  * the shared constants (the fp32 conv modes, the slab caps) are defined in
    asr_internal.h only;
  * _build.SOURCES, the one list of HIP sources, is the set of csrc/*.hip.
"""
import glob
import importlib.util
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "differential_equations_resnet_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

HEADERS = sorted(glob.glob(os.path.join(CSRC, "*.h")))
HIP = {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")))}


def test_headers_compile_alone():
    def check(h):
        res = subprocess.run([HIPCC, "-x", "hip", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only",
                              "-fsyntax-only", h], capture_output=True, text=True)
        return os.path.basename(h), res.returncode, res.stderr[-2000:]
    assert len(HEADERS) >= 8
    with ThreadPoolExecutor(min(len(HEADERS), os.cpu_count() or 1)) as pool:
        for name, rc, err in pool.map(check, HEADERS):
            assert rc == 0, f"{name} does not compile on its own:\n{err}"


# what else may start at column 0 of asr_internal.h: comments, the preprocessor, the namespace,
# the shared constants, and the one helper defined inline
OTHER_LINES = re.compile(r"$|//|#|namespace asr \{$|\}  // namespace asr$|enum \{ F_EULER|constexpr int k\w+ = |"
                         r"inline int launch_cus\(\) \{.*\}$")


def internal_declarations():
    """[(defining file, return type, name)] of asr_internal.h, by its '// ---- file.hip ----' groups, and of
    asr_common.h (set_error and fail of asr_theta.hip, which its inline hip_check needs).  Every line of
    asr_internal.h that starts at column 0 is a declaration's first line or one of OTHER_LINES: a
    declaration in a form this parser does not read fails here instead of going unchecked."""
    out, group = [], None
    for line in open(os.path.join(CSRC, "asr_internal.h")).read().split("\n"):
        g = re.match(r"// ---- (\w+\.hip) -+$", line)
        if g:
            group = g.group(1)
        m = re.match(r"(int|long|bool|size_t|BwdWs) (\w+)\(", line)  # (BwdWs: a layout struct of asr_common.h)
        if m:
            assert group, f"{m.group(2)} is declared above the first file group"
            out.append((group, m.group(1), m.group(2)))
        else:
            assert line[:1] in (" ", "\t") or OTHER_LINES.match(line), f"asr_internal.h: unaccounted line: {line!r}"
    common = open(os.path.join(CSRC, "asr_common.h")).read()
    for ret, name in (("void", "set_error"), ("int", "fail")):
        assert len(re.findall(r"^" + ret + " " + name + r"\(", common, re.M)) == 1
        out.append(("asr_theta.hip", ret, name))
    return out


def test_shared_functions_declared_once_defined_where_grouped():
    decls = internal_declarations()
    assert len(decls) >= 60 and len({n for _, _, n in decls}) == len(decls)
    assert {f for f, _, _ in decls} <= set(HIP)
    for want, ret, name in decls:
        pat = re.compile(r"^" + re.escape(ret) + r" " + name + r"\(", re.M)
        hits = [(f, t.count("\n", 0, m.start()) + 1) for f, t in HIP.items() for m in pat.finditer(t)]
        assert len(hits) == 1 and hits[0][0] == want, f"{ret} {name}(: expected once, in {want}; found at {hits}"
        # the one occurrence is the definition: a body follows its parameter list
        t = HIP[want]
        i = t.index("(", pat.search(t).start())
        depth = 0
        while True:
            depth += (t[i] == "(") - (t[i] == ")")
            i += 1
            if depth == 0:
                break
        assert t[i:].lstrip().startswith("{"), f"{name} in {want} is a declaration, not the definition"


def test_build_sources_are_the_hip_files_of_csrc():
    """_build.SOURCES is the one list of HIP sources (the build, tests/test_isa.py and tools/build_variants.sh
    read it): every *.hip of csrc/ once, and nothing else."""
    spec = importlib.util.spec_from_file_location("_asr_build", os.path.join(os.path.dirname(CSRC), "_build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert len(set(build.SOURCES)) == len(build.SOURCES)
    assert set(build.SOURCES) == set(HIP)


def test_shared_constants_defined_in_the_header_only():
    for f, t in HIP.items():
        assert "enum { F_EULER" not in t, f"{f} defines the conv mode enum (asr_internal.h has it)"
        m = re.search(r"^\s*(?:static )?(?:constexpr|const) \w+ kMax\w*Slabs\w*\s*=", t, re.M)
        assert not m, f"{f} defines {m.group(0).strip()} (asr_internal.h has the slab caps)"
    internal = open(os.path.join(CSRC, "asr_internal.h")).read()
    assert internal.count("enum { F_EULER") == 1
    assert len(re.findall(r"^constexpr int kMax\w*Slabs\w* =", internal, re.M)) == 2
