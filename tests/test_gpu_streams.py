"""The stream half of the ABI contract of include/asr.h: "every call is a stateless launch on the caller's
stream".  Every launch and async copy of a call is issued on the stream the caller passed and nowhere
else, no call synchronises or allocates, so a call can run on a side stream and be recorded into a HIP
graph and replayed.  The other GPU tests run everything on the legacy null stream, where a launch that
dropped its stream argument still runs in order.

The inventory is the one of tests/test_gpu_buffers.py (one case per launch path, its tables and case
builders, shapes unchanged), plus the stride-1 transition of test_gpu_stages.py and asr_segment_sq_norms
and asr_batch_metrics at one shape of test_gpu_small_kernels.py.  Not covered: asr_dist_* (RCCL orders
itself), the asr_debug_* readers, ASR_VARIANT_TIMED (records events) and the calls documented as
blocking (asr_net_prepare, asr_stages_prepare, asr_net_check_status, asr_net_kernel_times,
asr_stack_status).

Every case calls the C ABI directly, also where runtime.py has a wrapper: a wrapper allocates its outputs
and workspace inside the call (they could not be prefilled, nor a graph's buffers rewritten between
replays) and ParamMap.device uploads a cached host table on first use.  A case builder of the buffers
test is run against a Plan, which hands it plain buffers and records the call instead of making it; the
recorded call is then issued on whichever stream is current.

Data discipline, all three tests: two independent draws of the data operands from the family's own
distribution, A (stale) and B (fresh), seeded by a sequence [the case's seed, salt] that no other test
uses.  Index tables (w_src, theta_dst, augmentation items, segment offsets, what *_prepare wrote into a
workspace) are the same in A and B and never overwritten.  The buffers hold A, outputs and workspaces
0xFF, when the run under test copies B in and makes the call; no result of B exists anywhere in device
memory before that.  The reference is the same recorded call on other buffers on the default stream,
made after the run under test was synchronised and its outputs cloned.  Comparisons are bitwise
(test_gpu_buffers._same) over every output the buffers test compares.

The side-stream gate is torch.cuda._sleep, calibrated per module run with two events.  Measured on an
MI355X: 2.40e6 sleep cycles per millisecond; the slowest host-side issue of a call of this module is the
stages executors' forward_backward, 0.08 - 0.14 ms (every other call under 0.07 ms), so 20 x that stays
under the gate's floor of 50 ms.  The side stream is one that does not share the default stream's
hardware queue (_free_side_stream): on a shared queue the probe fails, as it should.

The same tests against a build whose k_optimizer launches go to stream 0: test_side_stream fails on the
outputs with the probe intact, test_graph_replay on the first replay (the capture stream is non-blocking,
so the stray launch is legal during capture: it runs at once and is missing from the graph).
"""
import ctypes as ct
import time

import numpy as np
import pytest

import test_gpu_buffers as TB
from helpers import metrics_case
from test_gpu_buffers import _bytes, _p, _same, _stream

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

INDEX_TABLES = ("w_src", "theta_dst", "items", "offsets")
GATE_FLOOR_MS, GATE_FACTOR = 50.0, 20.0
SLOWEST = "executor-stages-bf16"  # the longest host-side issue of the module (printed per case by test_side_stream)


@pytest.fixture(scope="module")
def rt():
    from differential_equations_resnet_amd import runtime
    runtime.require_gpu()
    return runtime


class Plan:
    """What a case builder of test_gpu_buffers.py sees in place of its Bufs: inputs are copies of the
    case's operands, outputs and workspaces plain tensors, and the ABI call is recorded without its
    stream argument (the last one of every entry point) to be issued later by launch()."""

    def __init__(self, build):
        self.inputs, self.outputs, self.calls, self.prepares = [], [], [], []
        self.outs = {k: v for k, v in build(self).items() if v is not None}
        assert self.calls and self.outs
        self.poison()

    def inp(self, t, what):
        if t is None:
            return None
        v = t.contiguous().clone()
        self.inputs.append((what, v))
        return v

    def out(self, shape, dtype, what):
        v = torch.empty(tuple(int(s) for s in shape), dtype=dtype, device="cuda")
        self.outputs.append(v)
        return v

    def call(self, name, *args):
        self.calls.append((name, args[:-1]))

    def prepare(self, name, *args):
        """A blocking *_prepare call that fills the index tables of a workspace: made by poison()."""
        self.prepares.append((name, args))

    def poison(self):
        """Outputs and workspaces 0xFF on the current stream; the tables of a prepared workspace again."""
        for v in self.outputs:
            _bytes(v).fill_(0xFF)
        if self.prepares:
            torch.cuda.current_stream().synchronize()  # (prepare copies on the null stream)
            for name, args in self.prepares:
                TB._call(name, *args)

    def load(self, other):
        """The data operands of `other` into this plan's buffers, on the current stream."""
        assert [w for w, _ in self.inputs] == [w for w, _ in other.inputs]
        for (what, dst), (_, src) in zip(self.inputs, other.inputs):
            if what not in INDEX_TABLES:
                dst.copy_(src)

    def launch(self):
        for name, args in self.calls:
            TB._call(name, *args, _stream())

    def results(self):
        return {k: v.clone() for k, v in self.outs.items()}


def _equal(got, want, what):
    assert got.keys() == want.keys()
    for k in got:
        assert _same(got[k], want[k]), f"{what}: {k} differs from the default-stream result on the same operands"


def _differ(a, b):
    return any(not _same(a[k], b[k]) for k in a)


# ---------------------------------------------------------------------------
# The cases: (id, make), make(rt, salt) -> the builder of that draw of the operands
# ---------------------------------------------------------------------------
def _conv(case, mode_name, direction):
    def make(rt, salt):
        c = TB._conv_case(rt, case, salt)
        euler = mode_name == "euler"
        mode = rt.ASR_MODE_EULER if euler else rt.ASR_MODE_CONV
        if direction == "fwd":
            return lambda B: c.forward(B, mode, euler)
        return lambda B: c.backward(B, mode, euler)
    return make


def _rk2(dtype, shape, direction):
    def make(rt, salt):
        d = TB._rk2_case(rt, dtype, shape, salt)
        return lambda B: (TB._rk2_forward if direction == "fwd" else TB._rk2_backward)(B, d, shape)
    return make


def _stack(name, direction):
    def make(rt, salt):
        d = TB._stack_case(rt, name, salt)
        if direction == "fwd":
            return lambda B: dict(zip(("ys", "masks"), TB._stack_forward(B, d)[:2]))
        return lambda B: TB._stack_backward(B, d)
    return make


def _rk2_stack(direction):
    def make(rt, salt):
        d = TB._rk2_stack_case(rt, salt)
        return lambda B: (TB._rk2_stack_forward if direction == "fwd" else TB._rk2_stack_backward)(B, rt, d)
    return make


def _transition(dims, S, direction):
    def make(rt, salt):
        d = TB._transition_case(rt, dims, S, salt)
        return lambda B: (TB._transition_forward if direction == "fwd" else TB._transition_backward)(B, d)
    return make


def _theta(bf, k, C):
    def make(rt, salt):
        d = TB._theta_case(rt, bf, k, C, salt)
        return lambda B: TB._theta_to_w(B, d)
    return make


def _optimizer(name, n):
    def make(rt, salt):
        from differential_equations_resnet_amd import _lib
        _, kind, flags, lr, a, b, eps = next(o for o in TB.OPT if o[0] == name)
        cfg = _lib.OptimizerConfig(kind, flags, lr, a, b, eps, 3, 0.125)
        p, grads, state = TB._opt_data(n, rt.optimizer_slots(kind, flags), 50000 + 100 * salt + kind)
        return lambda B: TB._optimizer_update(B, cfg, p, grads, state)
    return make


def _adam(n):
    def make(rt, salt):
        p, grads, state = TB._opt_data(n, 2, 50007 + 100 * salt)
        m, v = state[:n].clone(), state[n:].clone()
        return lambda B: TB._adam_update(B, p, grads, m, v, (1e-3, 0.9, 0.999, 1e-7, 3, 0.125))
    return make


def _segment_sq_norms(rt, salt):
    """The segments of test_gpu_small_kernels.test_segment_sq_norms (0 .. 20000 elements, unaligned offsets)."""
    lengths, gaps = [0, 1, 63, 255, 256, 257, 20000], [3, 1, 5, 1, 2, 7, 1, 9]
    off = [gaps[0]]
    for i, n in enumerate(lengths):
        off.append(off[-1] + n)
        if i + 1 < len(lengths):
            off.append(off[-1] + gaps[i + 1])
    x = TB._dev(TB._rng(0, salt).standard_normal(off[-1] + gaps[-1]).astype(np.float32))
    offsets = TB._dev(np.array(off, np.int64))

    def build(B):
        xi, oi = B.inp(x, "x"), B.inp(offsets, "offsets")
        out = B.out((len(off) - 1,), torch.float32, "out")
        B.call("asr_segment_sq_norms", _p(xi), _p(oi), len(off) - 1, _p(out), _stream())
        return {"out": out}
    return build


def _batch_metrics(rt, salt):
    """N, K = 257, 10 of test_gpu_small_kernels.test_batch_metrics, the loss from probs; accum is read-modify-write."""
    N, K = 257, 10
    p, t = metrics_case(N, K, seed=1000 + salt)
    p, t = TB._dev(p), TB._dev(t)
    accum = TB._dev(TB._rng(N, salt).uniform(0, 100, 4).astype(np.float32))

    def build(B):
        pi, ti, ai = B.inp(p, "probs"), B.inp(t, "targets"), B.inp(accum, "accum")
        B.call("asr_batch_metrics", _p(pi), _p(ti), None, N, K, _p(ai), _stream())
        return {"accum": ai}
    return build


def _augment(name):
    def make(rt, salt):
        d = TB._augment_case(name, salt)
        return lambda B: TB._augment_batch(B, d)
    return make


def _executor(name):
    """forward_backward with probs (forward for the inference executor) as runtime.py's executors call it,
    on a workspace of the plan's own: 0xFF, then the executor's prepare call."""
    def make(rt, salt):
        ex, params, rng, prepare = TB.EXECUTORS[name](rt, salt)
        c, entry = ex.cfg, prepare.replace("_prepare", "")
        imgs = torch.from_numpy(rng.integers(0, 256, (c.N, c.H, c.W, 3), dtype=np.uint8)).cuda()
        tgt = TB._dev(np.eye(10, dtype=np.float32)[rng.integers(0, 10, c.N)])

        def build(B):
            p, im = B.inp(params, "params"), B.inp(imgs, "images")
            ws = B.out((ex.ws_bytes,), torch.uint8, "workspace")
            B.prepare(prepare, ct.byref(c), _p(ws), ex.ws_bytes)
            probs = B.out((c.N, 10), torch.float32, "probs")
            if ex.inference:
                B.call(entry + "_forward", ct.byref(c), _p(p), _p(im), _p(probs), _p(ws), ex.ws_bytes, _stream())
                return {"probs": probs}
            t = B.inp(tgt, "targets")
            grads, loss = B.out((ex.n_params,), torch.float32, "grads"), B.out((1,), torch.float32, "loss")
            B.call(entry + "_forward_backward", ct.byref(c), _p(p), _p(im), _p(t), _p(grads), _p(loss), _p(probs),
                   _p(ws), ex.ws_bytes, _stream())
            return {"loss": loss, "grads": grads, "probs": probs}
        return build
    return make


def _conv_cases(table):
    return [(f"conv-{case[0]}-{m}-{d}", _conv(case, m, d)) for case in table for m in ("euler", "conv")
            for d in ("fwd", "bwd")]


OTHERS = (
    [(f"rk2-{i}-{d}", _rk2(dt, shape, d)) for (dt, shape), i in zip(TB.RK2, TB.RK2_IDS) for d in ("fwd", "bwd")]
    + [(f"stack-{s[0]}-{d}", _stack(s[0], d)) for s in TB.STACKS for d in ("fwd", "bwd")]
    + [(f"rk2-stack-{d}", _rk2_stack(d)) for d in ("fwd", "bwd")]
    + [(f"transition-s{S}-{d}", _transition(dims, S, d)) for dims, S in ((TB.TRANSITIONS[0], 2), ((2, 8, 8, 6, 4), 1))
       for d in ("fwd", "bwd")]
    + [(f"theta-{name}", _theta(bf, k, C)) for name, bf, k, C in TB.THETA]
    + [(f"opt-{o[0]}-{TB.OPT_SIZES[0]}", _optimizer(o[0], TB.OPT_SIZES[0])) for o in TB.OPT]
    + [(f"opt-adam-{TB.OPT_SIZES[1]}", _optimizer("adam", TB.OPT_SIZES[1])),  # the wrapped grid
       (f"adam-{TB.OPT_SIZES[0]}", _adam(TB.OPT_SIZES[0])),
       ("segment-sq-norms", _segment_sq_norms), ("batch-metrics", _batch_metrics)]
    + [(f"augment-{name}", _augment(name)) for name in TB.AUGMENT]
    + [(f"executor-{name}", _executor(name)) for name in TB.EXECUTORS]
)
ALL = _conv_cases(TB.CONV) + OTHERS
GRAPH = _conv_cases(TB.CONV_SKIP) + OTHERS  # one conv shape per backward path
CASES = dict(ALL)
assert len(CASES) == len(ALL) and SLOWEST in CASES


def _params(cases):
    return pytest.mark.parametrize("make", [c[1] for c in cases], ids=[c[0] for c in cases])


# ---------------------------------------------------------------------------
# a. on a side stream, behind a gate
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gate(rt):
    """Cycles of torch.cuda._sleep that hold a stream for GATE_FACTOR x the host-side issue time of the
    slowest call of the module, GATE_FLOOR_MS at least."""
    cycles = 20_000_000
    torch.cuda._sleep(cycles)  # (the sleep kernel's first launch)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(cycles)
    t1.record()
    torch.cuda.synchronize()
    per_ms = cycles / t0.elapsed_time(t1)
    P = Plan(CASES[SLOWEST](rt, 1))
    P.launch()
    torch.cuda.synchronize()
    h0 = time.perf_counter()
    P.launch()
    issue_ms = (time.perf_counter() - h0) * 1e3
    torch.cuda.synchronize()
    ms = max(GATE_FLOOR_MS, GATE_FACTOR * issue_ms)
    print(f"gate: {per_ms:.0f} sleep cycles per ms, {SLOWEST} issues in {issue_ms:.3f} ms, gate {ms:.1f} ms")
    return int(ms * per_ms)


def _free_side_stream(cycles):
    """A fresh stream that the device does not serve from the hardware queue of the default stream.  The
    runtime spreads its streams over a few hardware queues (four by default), each first in, first out: on
    the default stream's own queue the probe, and a launch that wrongly went to the default stream, would
    wait behind the gate like the rest of the call, and the test would show nothing (measured: every
    fourth stream of torch's pool).  Such a stream is told apart without a clock: work of the default
    stream enqueued behind a sleeping stream finishes before the sleep only from another queue."""
    for _ in range(8):
        side = torch.cuda.Stream()
        slept, passed = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(side):
            torch.cuda._sleep(cycles)
            slept.record()
        passed.record()  # (on the default stream)
        passed.synchronize()
        free = not slept.query()
        side.synchronize()
        if free:
            return side
    pytest.fail("no stream of eight runs beside the default stream: the gate cannot be built (this says nothing about "
                "the kernels)")


@_params(ALL)
def test_side_stream(rt, gate, make):
    """The call on a fresh side stream whose operands still hold A while the host issues it: the stream
    first sleeps, then copies B in.  A launch that went to another stream reads A (or writes before the
    poisoned outputs' other writers) and fails the comparison; the probe shows that the gate was shut."""
    P, Q = Plan(make(rt, 11)), Plan(make(rt, 12))
    P.launch()  # the kernels' first launch (code loading, occupancy queries) is not part of the issue time
    torch.cuda.synchronize()
    stale_outs = P.results()
    P.poison()
    written = {v.data_ptr() for v in P.outs.values()}  # (a read-modify-write operand is no probe: the call changes it)
    i = next(i for i, (what, v) in enumerate(P.inputs)
             if what not in INDEX_TABLES and v.numel() and v.data_ptr() not in written)
    stale, probe = P.inputs[i][1].clone(), torch.empty_like(P.inputs[i][1])
    assert not _same(stale, Q.inputs[i][1])
    torch.cuda.synchronize()
    side = _free_side_stream(gate // 10)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.cuda._sleep(gate)
        P.load(Q)
        h0 = time.perf_counter()
        P.launch()
        issue_ms = (time.perf_counter() - h0) * 1e3
    # on the default stream, waiting for nothing (into a buffer made before: an allocation may synchronise)
    probe.copy_(P.inputs[i][1])
    torch.cuda.synchronize()
    print(f"issue {issue_ms:.3f} ms")
    assert _same(probe, stale), (f"the gate was too short: {P.inputs[i][0]} already held the fresh operands when the "
                                 f"host had issued the call ({issue_ms:.3f} ms); this says nothing about the kernels")
    got = P.results()
    Q.launch()
    torch.cuda.synchronize()
    _equal(got, Q.outs, "side stream")
    assert _differ(stale_outs, Q.outs), "the stale and the fresh operands give the same outputs: the case shows nothing"


# ---------------------------------------------------------------------------
# b. recorded into a HIP graph and replayed
# ---------------------------------------------------------------------------
@_params(GRAPH)
def test_graph_replay(rt, make):
    """As bench.py's block_roofline.timed does: one warm-up call on a side stream, then the call captured
    (global capture error mode: a call that synchronises or allocates fails the capture; a launch that
    went to another stream is missing from the graph, which the replays show) into a graph of one linear
    chain.  The graph is replayed twice on fresh operands and
    poisoned outputs and workspaces."""
    P, Q = Plan(make(rt, 21)), Plan(make(rt, 22))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        P.launch()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        P.launch()
    got = []
    for _ in range(2):
        P.load(Q)  # (also the params and state a read-modify-write call updated)
        P.poison()
        g.replay()
        torch.cuda.synchronize()
        got.append(P.results())
    Q.launch()
    torch.cuda.synchronize()
    for n, r in enumerate(got):
        _equal(r, Q.outs, f"replay {n + 1}")


# ---------------------------------------------------------------------------
# c. two calls at once on two streams
# ---------------------------------------------------------------------------
PAIRS = {
    # the same persistent kernel twice: its slab hand-off poll is bounded and a timed-out fold gives the same bits
    "c64-stack-bwd-twice": ([_stack("c64", "bwd")], [_stack("c64", "bwd")]),
    "deep16-stack-fwd-bwd+f32-mfma-conv-bwd": ([_stack("deep16", "fwd"), _stack("deep16", "bwd")],
                                               [_conv(next(c for c in TB.CONV if c[0] == "f32-mfma-1x6x32x64"),
                                                      "euler", "bwd")]),
    "two-c64-euler-executors": ([_executor("net-bf16-c64-euler")], [_executor("net-bf16-c64-euler")]),
}


@pytest.mark.parametrize("pair", list(PAIRS))
def test_two_streams_concurrent(rt, pair):
    """Each lane's calls on a side stream of its own, the lanes issued alternately four times, operands,
    outputs and workspaces separate: all eight results equal that call's serial default-stream result
    (device state that two calls share would show here)."""
    lanes = [[(Plan(m(rt, 31 + 2 * j)), Plan(m(rt, 32 + 2 * j))) for m in makes] for j, makes in enumerate(PAIRS[pair])]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s, lane in zip(streams, lanes):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for P, Q in lane:
                P.load(Q)
    got = [[], []]
    for _ in range(4):
        for j, (s, lane) in enumerate(zip(streams, lanes)):
            with torch.cuda.stream(s):
                for P, _ in lane:
                    P.poison()
                    P.launch()
                got[j].append([P.results() for P, _ in lane])
    torch.cuda.synchronize()
    for lane in lanes:
        for _, Q in lane:
            Q.launch()
    torch.cuda.synchronize()
    for j, lane in enumerate(lanes):
        for n, rep in enumerate(got[j]):
            for r, (_, Q) in zip(rep, lane):
                _equal(r, Q.outs, f"lane {j}, repetition {n + 1}")
