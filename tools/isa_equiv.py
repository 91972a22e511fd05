"""Do two git revisions compile the product kernels to the same gfx950
instruction streams and the same kernel metadata?  (A refactor claimed neutral
must: round 4's switch cleanup 6c75dab compiles every stack kernel
bit-identically to f540cc2, the measured tree before it.)  Labels are
renumbered, comments and directives dropped.  Prints one same/DIFF line per
kernel (a kernel of one side only is a DIFF) and a summary; exit status 1 on
any difference.  --alias REGEX=REPLACEMENT (repeatable) rewrites the kernel
symbols of both sides with re.sub before they are matched: a renamed or
re-parameterised kernel against its predecessor.  A kernel whose instructions
differ comes with the number of differing lines.
usage: python tools/isa_equiv.py [--alias REGEX=REPLACEMENT ...] REV_A REV_B [source.hip ...]
       (default: every product source)"""
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "differential_equations_resnet_amd/csrc"
SOURCES = ["asr_theta.hip", "asr_block_mfma.hip", "asr_conv_f32.hip", "asr_conv_kxk.hip", "asr_stem_head.hip",
           "asr_api.hip", "asr_dist.hip", "asr_deep16.hip", "asr_stages.hip"]
META = ["vgpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"]


def kernels(asm):
    """{kernel symbol: [instruction and label lines]}"""
    out = {}
    for f in re.split(r'\n(?=_Z[\w]+:|[A-Za-z_]\w*:\s+; @)', asm):
        name = f.split(':', 1)[0]
        if not name.startswith('_Z') or 's_endpgm' not in f:
            continue  # (data symbols and the metadata that follows them)
        # (a label's "; in Loop: Header=BBn_m" comment carries the function's index in its file)
        # (the file's metadata notes follow its last kernel: kernel_metadata reads them, per kernel)
        f = f.split('.amdgpu_metadata', 1)[0]
        body = [re.sub(r'\.LBB\d+_\d+', 'L', l.split(';', 1)[0].strip()) for l in f.split('\n')[1:]]
        # (the trailing __hip_cuid_<hash of the source file> symbol is not code)
        out[name] = [l for l in body if l and not l.startswith(('.', '__hip_cuid_'))]
    return out


def kernel_metadata(asm):
    """{kernel symbol: {META key: value}} from the .amdgpu_metadata notes (as tests/test_isa.py reads them)"""
    out = {}
    # (one "  - " entry per kernel, keys sorted: group_segment_fixed_size stands before .name)
    for entry in re.split(r"\n  - ", asm.split("amdhsa.kernels:", 1)[-1].split(".end_amdgpu_metadata", 1)[0]):
        name = re.search(r"^    \.name:\s+(\S+)", entry, re.M)
        if name:
            vals = {k: re.search(r"^    \." + k + r":\s+(\d+)", entry, re.M) for k in META}
            out[name.group(1)] = {k: int(v.group(1)) if v else 0 for k, v in vals.items()}
    return out


def compile_tree(tree, src, out):
    """(kernels, metadata) of tree/CSRC/src, compiled to the assembly file `out`"""
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    "-w", "-o", out, os.path.join(tree, CSRC, src)], check=True)
    asm = open(out).read()
    return kernels(asm), kernel_metadata(asm)


def export(rev, d):
    dst = os.path.join(d, rev)
    os.makedirs(dst, exist_ok=True)
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC, "include"], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", dst], input=tar, check=True)
    return dst


def renamed(table, aliases):
    """`table`'s kernel symbols after every (regex, replacement) of `aliases`"""
    out = {}
    for k, v in table.items():
        for pat, rep in aliases:
            k = re.sub(pat, rep, k)
        assert k not in out, f"--alias maps two kernels of one side onto {k}"
        out[k] = v
    return out


def differing_lines(a, b):
    """lines in the changed blocks of a line diff (a replaced block counts its longer side)"""
    return sum(j - i if op == "delete" else l - k if op == "insert" else max(j - i, l - k)
               for op, i, j, k, l in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes()
               if op != "equal")


def compare(tree_a, tree_b, srcs, d, aliases=()):
    """Print one line per kernel and the summary; the number of differing kernels."""
    jobs = [(t, s, os.path.join(d, f"{i}_{s}.s")) for s in srcs for i, t in enumerate((tree_a, tree_b))]
    with ThreadPoolExecutor(min(len(jobs), os.cpu_count() or 1, 16)) as pool:
        res = [tuple(renamed(t, aliases) for t in r) for r in pool.map(lambda j: compile_tree(*j), jobs)]
    total = diffs = 0
    for n, src in enumerate(srcs):
        (ka, ma), (kb, mb) = res[2 * n], res[2 * n + 1]
        for k in sorted(set(ka) | set(kb)):
            if k not in ka or k not in kb:
                tag = "DIFF (only in %s)" % ("A" if k in ka else "B")
            elif ka[k] != kb[k]:
                tag = "DIFF (instructions: %d lines of %d -> %d differ)" % (differing_lines(ka[k], kb[k]), len(ka[k]),
                                                                          len(kb[k]))
            elif k not in ma or k not in mb:
                tag = "DIFF (no metadata entry in %s)" % " and ".join(s for s, m in (("A", ma), ("B", mb)) if k not in m)
            elif ma[k] != mb[k]:
                tag = "DIFF (metadata: " + ", ".join(f"{m} {ma[k][m]} -> {mb[k][m]}" for m in META
                                                     if ma[k][m] != mb[k][m]) + ")"
            else:
                tag = "same"
            total += 1
            diffs += tag != "same"
            print(f"{tag} {src} {k[:90]}")
    print(f"isa_equiv: {total} kernels in {len(srcs)} sources, {total - diffs} same, {diffs} DIFF")
    return diffs


if __name__ == "__main__":
    args, aliases = sys.argv[1:], []
    while "--alias" in args:
        i = args.index("--alias")
        aliases.append(tuple(args[i + 1].split("=", 1)))
        del args[i:i + 2]
    a, b = args[0], args[1]
    with tempfile.TemporaryDirectory() as d:
        sys.exit(1 if compare(export(a, d), export(b, d), args[2:] or SOURCES, d, aliases) else 0)
