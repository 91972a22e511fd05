"""CPU check of the stream contract of include/asr.h over the HIP sources (no GPU needed; the GPU half is
tests/test_gpu_streams.py).

  * every hipLaunchKernelGGL names a stream (its fifth argument, launches in macro bodies included) and
    every hipMemsetAsync / hipMemcpyAsync one as its last argument, and none of them is the null stream
    written out (0, nullptr, NULL, hipStreamDefault): a launch on the null stream runs in order in every
    test that uses no other stream, and races on any other;
  * the calls that block the host or allocate appear only inside the entry points documented as
    blocking or as debug readers (BLOCKING_ALLOWED, by function name): any other call can be recorded
    into a HIP graph.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "differential_equations_resnet_amd", "csrc")

NULL_STREAMS = {"0", "nullptr", "NULL", "hipStreamDefault", "(hipStream_t)0", "hipStream_t(0)", "(hipStream_t)nullptr",
                ""}
BLOCKING = ("hipMemcpy(", "hipMemset(", "hipDeviceSynchronize", "hipStreamSynchronize", "hipMalloc", "hipFree",
            "hipMemcpyFromSymbol")
# function name (a trailing * matches the rest of the name): why it may block
BLOCKING_ALLOWED = {
    "asr_net_prepare": "documented blocking: uploads the element maps into the workspace once per executor",
    "asr_stages_prepare": "documented blocking: uploads the element maps of every stage once per executor",
    "asr_net_check_status": "documented blocking: synchronises the stream to report a failed launch",
    "asr_net_kernel_times": "documented blocking: reads the events of the last ASR_VARIANT_TIMED call",
    "asr_stack_status": "documented blocking: reads (and resets) the degraded hand-off counter",
    "asr_debug_*": "debug readers of device-side traces, never on a hot path",
}


def strip_comments(text):
    """`text` without // and /* */ comments and without the contents of string literals; newlines kept, so
    offsets still give line numbers."""
    def blank(m):
        s = m.group(0)
        if s.startswith('"'):
            return '"' + re.sub(r"[^\n]", " ", s[1:-1]) + '"'
        return re.sub(r"[^\n]", " ", s)
    return re.sub(r'//[^\n]*|/\*.*?\*/|"(?:\\.|[^"\\\n])*"', blank, text, flags=re.S)


def call_arguments(text, open_paren):
    """The top-level arguments of the call whose '(' is at text[open_paren], backslash-newlines of a
    macro body removed."""
    depth, args, start = 0, [], open_paren + 1
    for i in range(open_paren, len(text)):
        c = text[i]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                args.append(text[start:i])
                return [re.sub(r"\\\n|\s+", " ", a).strip() for a in args]
        elif c == "," and depth == 1:
            args.append(text[start:i])
            start = i + 1
    raise AssertionError("unbalanced call")


def enclosing_function(text, pos):
    """Name of the function whose definition encloses text[pos]: the nearest line above that starts at
    column 0 with a declarator `name(` (the sources keep every definition's first line there), provided
    no body has closed (a '}' at column 0) in between."""
    head = text[:pos]
    defs = list(re.finditer(r"^(?!namespace\b|typedef\b|using\b)[A-Za-z_][^\n;]*?\b(\w+)\(", head, re.M))
    assert defs, "a call outside any function"
    d = defs[-1]
    assert not re.search(r"^\}", head[d.start():], re.M), f"a call outside any function, after {d.group(1)}"
    return d.group(1)


def sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(files) >= 20
    return [(os.path.basename(p), strip_comments(open(p).read())) for p in files]


def stream_sites(text):
    """[(line, call, its stream argument or None if it has too few arguments)]"""
    out = []
    for m in re.finditer(r"\b(hipLaunchKernelGGL|hipMemsetAsync|hipMemcpyAsync)\s*\(", text):
        args = call_arguments(text, m.end() - 1)
        if m.group(1) == "hipLaunchKernelGGL":
            s = args[4] if len(args) >= 5 else None
        else:
            s = args[-1] if len(args) == (4 if m.group(1) == "hipMemsetAsync" else 5) else None
        out.append((text.count("\n", 0, m.start()) + 1, m.group(1), s))
    return out


def test_every_launch_and_async_copy_names_the_callers_stream():
    n = {"hipLaunchKernelGGL": 0, "hipMemsetAsync": 0, "hipMemcpyAsync": 0}
    for name, text in sources():
        for line, call, s in stream_sites(text):
            n[call] += 1
            assert s is not None, f"{name}:{line}: {call} without a stream argument"
            assert s not in NULL_STREAMS, f"{name}:{line}: {call} on the null stream ({s!r}), not the caller's"
    assert n["hipLaunchKernelGGL"] >= 80 and n["hipMemcpyAsync"] >= 5, n


def test_no_memset_nodes():
    """hipMemsetAsync keeps its stream, but recorded into a HIP graph its memset node ran out of order with
    the work enqueued before the replay (test_gpu_streams.test_graph_replay, the fp32 relu masks): buffers
    are zeroed by zero_words (asr_theta.hip), a kernel."""
    for name, text in sources():
        for line, call, _ in stream_sites(text):
            assert call != "hipMemsetAsync", f"{name}:{line}: hipMemsetAsync: zero with zero_words (asr_internal.h)"


def test_blocking_calls_only_in_the_documented_entry_points():
    pat = re.compile("|".join(re.escape(b) for b in BLOCKING))  # (prefixes: hipMallocAsync, hipFreeAsync, ... too)
    found = set()
    for name, text in sources():
        for m in pat.finditer(text):
            if m.start() and (text[m.start() - 1].isalnum() or text[m.start() - 1] == "_"):
                continue  # (part of a longer identifier)
            fn = enclosing_function(text, m.start())
            line = text.count("\n", 0, m.start()) + 1
            ok = any(fn == a or (a.endswith("*") and fn.startswith(a[:-1])) for a in BLOCKING_ALLOWED)
            assert ok, (f"{name}:{line}: {m.group(0)} in {fn}, which is not documented as blocking: the call could no "
                        f"longer be recorded into a HIP graph")
            found.add(fn)
    assert {"asr_net_prepare", "asr_stages_prepare", "asr_net_check_status", "asr_stack_status"} <= found


def test_the_checks_notice_what_they_look_for():
    """The parsers on small texts: a launch in a macro body, a launch on stream 0, a blocking call in a helper."""
    macro = strip_comments("#define L(K) \\\n  hipLaunchKernelGGL((k<1, 2>), dim3(g), dim3(256), lds, s, a, f(b, c))  // 0\n")
    assert stream_sites(macro) == [(2, "hipLaunchKernelGGL", "s")]
    null = strip_comments("int f(hipStream_t s) {\n  hipLaunchKernelGGL(k, dim3(g), dim3(256), 0, 0, a);\n"
                          "  hipMemsetAsync(p, 0, n, s);\n  hipMemcpyAsync(d, e, n, hipMemcpyDeviceToDevice);\n}\n")
    assert [s for _, _, s in stream_sites(null)] == ["0", "s", None]
    text = strip_comments("namespace asr {\nstatic int helper(int a,\n                  int b) {\n  if (a) {\n"
                          "    hipStreamSynchronize(s);  // hipFree\n  }\n  return 0;\n}\nint other() {\n  return 1;\n}\n")
    assert enclosing_function(text, text.index("hipStreamSynchronize")) == "helper"
    assert "hipFree" not in text
