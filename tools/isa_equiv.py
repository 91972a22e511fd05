"""Do two git revisions compile the product kernels to the same gfx950
instruction streams and the same kernel metadata?  (A refactor claimed neutral
must: round 4's switch cleanup 6c75dab compiles every stack kernel
bit-identically to f540cc2, the measured tree before it.)  Labels are
renumbered, comments and directives dropped.  Each side's sources are its own
csrc/*.hip and kernels are matched by symbol across the whole tree, so a kernel
moved to another file is `same`; a symbol that two sources of one side define
(a kernel template instantiated in two translation units) is a DIFF.  Prints
one same/DIFF line per kernel with its file on each side (a kernel of one side
only is a DIFF) and a summary; exit status 1 on any difference.
--alias REGEX=REPLACEMENT (repeatable) rewrites the kernel symbols of both
sides with re.sub before they are matched: a renamed or re-parameterised kernel
against its predecessor.  A kernel whose instructions differ comes with the
number of differing lines.
usage: python tools/isa_equiv.py [--alias REGEX=REPLACEMENT ...] REV_A REV_B
       (a revision, or a directory holding a tree: `.` is the working tree)"""
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "differential_equations_resnet_amd/csrc"
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
    """the tree of a git revision, or `rev` itself where it is a directory (a working tree)"""
    if os.path.isdir(rev):
        return rev
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


def sources(tree):
    """the tree's own HIP sources"""
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(tree, CSRC, "*.hip")))


def side(tree, tag, d, aliases):
    """({kernel symbol: (source, instructions, metadata or None)}, {symbol defined twice: its sources}, number of
    sources) of every HIP source of `tree`"""
    srcs = sources(tree)
    with ThreadPoolExecutor(min(len(srcs), os.cpu_count() or 1, 16)) as pool:
        res = list(pool.map(lambda s: compile_tree(tree, s, os.path.join(d, f"{tag}_{s}.s")), srcs))
    table, twice = {}, {}
    for src, (ks, ms) in zip(srcs, res):
        ms = renamed(ms, aliases)
        for k, body in renamed(ks, aliases).items():
            if k in table:
                twice.setdefault(k, [table[k][0]]).append(src)
            table[k] = (src, body, ms.get(k))
    return table, twice, len(srcs)


def compare(tree_a, tree_b, d, aliases=()):
    """Print one line per kernel and the summary; the number of differing kernels."""
    (ta, dup_a, na), (tb, dup_b, nb) = side(tree_a, "a", d, aliases), side(tree_b, "b", d, aliases)
    total = diffs = 0
    for k in sorted(set(ta) | set(tb)):
        (fa, ka, ma), (fb, kb, mb) = ta.get(k, ("-", None, None)), tb.get(k, ("-", None, None))
        if k in dup_a or k in dup_b:
            tag = "DIFF (defined in " + "; ".join(f"{' and '.join(dup[k])} of {s}" for s, dup in (("A", dup_a), ("B", dup_b))
                                                  if k in dup) + ")"
        elif ka is None or kb is None:
            tag = "DIFF (only in %s)" % ("A" if kb is None else "B")
        elif ka != kb:
            tag = "DIFF (instructions: %d lines of %d -> %d differ)" % (differing_lines(ka, kb), len(ka), len(kb))
        elif ma is None or mb is None:
            tag = "DIFF (no metadata entry in %s)" % " and ".join(s for s, m in (("A", ma), ("B", mb)) if m is None)
        elif ma != mb:
            tag = "DIFF (metadata: " + ", ".join(f"{m} {ma[m]} -> {mb[m]}" for m in META if ma[m] != mb[m]) + ")"
        else:
            tag = "same"
        total += 1
        diffs += tag != "same"
        print(f"{tag} {fa if fa == fb else fa + ' -> ' + fb} {k[:90]}")
    print(f"isa_equiv: {total} kernels ({len(ta)} in {na} sources -> {len(tb)} in {nb} sources), {total - diffs} same, "
          f"{diffs} DIFF")
    return diffs


if __name__ == "__main__":
    args, aliases = sys.argv[1:], []
    while "--alias" in args:
        i = args.index("--alias")
        aliases.append(tuple(args[i + 1].split("=", 1)))
        del args[i:i + 2]
    a, b = args[0], args[1]
    with tempfile.TemporaryDirectory() as d:
        sys.exit(1 if compare(export(a, d), export(b, d), d, aliases) else 0)
