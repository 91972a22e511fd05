"""Buffer containment and stale-memory independence of every kernel family, through the C ABI.

The parity tests reach the kernels through runtime.py, whose outputs and workspaces are exactly sized
torch.empty tensors (a write a few bytes past the end lands in the allocator's slack), whose relu
masks are torch.zeros (a kernel that ORs bits in, or skips the bytes of a partial band, passes) and
whose inputs start their allocation (a halo read before image 0 reads small finite values).  Here
every buffer handed to a call is carved (helpers.carve) out of a larger one, GUARD bytes from either
end, with exactly its documented size:

  inputs     valid contents between guards of 0xFF bytes (NaN as fp32 and bf16, -1 as int32, set
             mask bits): an out-of-bounds read that reaches arithmetic shows in the result;
  outputs and workspaces  twice, once with interior and guards 0x00 and once 0xFF.

Asserted per case, in this order: the call returns ASR_OK and, after a synchronize, every guard of
every buffer is intact; the outputs of the two prefills are bitwise identical over their whole
documented size (mask padding bits included); both equal, bitwise, the runtime.py wrapper's result
on the same inputs (what the parity tests hold to the fp64 oracle) and every float output is finite.
Workspace contents are not compared.  No tolerance appears: every path is documented deterministic
(slabs reduced in a fixed order, no float atomics).

gamma = -0.1, h = 0.5, with bias; inputs and theta as the family's parity test draws them.
"""
import ctypes as ct

import numpy as np
import pytest

import augment_ref as A
import kxk_net_oracle as KO
from helpers import carve, carve_like, guards_intact
from oracle import asr_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GAMMA, H_STEP = -0.1, 0.5
PREFILLS = (0x00, 0xFF)


@pytest.fixture(scope="module")
def rt():
    from differential_equations_resnet_amd import runtime
    runtime.require_gpu()
    return runtime


def _call(name, *args):
    from differential_equations_resnet_amd import _lib
    assert _lib.call(name, *args) == _lib.ASR_OK


def _lib_():
    from differential_equations_resnet_amd import _lib
    return _lib.load()


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nbytes(t):
    return t.numel() * t.element_size()


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _same(a, b):
    return a.dtype == b.dtype and a.numel() == b.numel() and torch.equal(_bytes(a), _bytes(b))


class Bufs:
    """The carved buffers of one call: inputs (0xFF guards), outputs and workspaces (`fill` inside and in the guards)."""

    def __init__(self, fill):
        self.fill, self.dev, self.all = fill, torch.device("cuda"), []

    def inp(self, t, what):
        if t is None:
            return None
        buf, v = carve_like(t, 0xFF)
        self.all.append((buf, _nbytes(v), what, 0xFF))
        return v

    def out(self, shape, dtype, what):
        buf, v = carve(shape, dtype, self.dev, self.fill, self.fill)
        self.all.append((buf, _nbytes(v), what, self.fill))
        return v

    def call(self, name, *args):
        """The launch of a case builder (tests/test_gpu_streams.py records it instead, to issue it later)."""
        _call(name, *args)

    def check(self):
        torch.cuda.synchronize()
        for buf, n, what, g in self.all:
            guards_intact(buf, n, f"{what} (prefill 0x{self.fill:02X})", g)


def _equal_wrapper(got, want):
    """Every output in `got` equals the wrapper's (where `want` has it) bitwise, and is finite."""
    for k in got:
        if k in want:
            assert _same(got[k], want[k]), f"{k}: differs from the runtime.py wrapper's result"
        if got[k].is_floating_point():
            assert bool(torch.isfinite(got[k].float()).all()), f"{k}: not finite"


def _check_outputs(got, want):
    """got: the outputs of the 0x00 and of the 0xFF run ({name: tensor}); want: the wrapper's."""
    a, b = got
    assert a.keys() == b.keys()
    for k in a:
        assert _same(a[k], b[k]), f"{k}: the 0x00- and the 0xFF-prefilled runs differ"
    _equal_wrapper(b, want)
    return b


def _both(launch, want):
    got = []
    for fill in PREFILLS:
        B = Bufs(fill)
        outs = launch(B)
        B.check()
        got.append({k: v for k, v in outs.items() if v is not None})
    return _check_outputs(got, want)


def _dev(a, bf=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(torch.bfloat16).contiguous() if bf else t


def _rng(seed, salt=None):
    """The case's generator; with a salt, an independent one (a seed sequence no integer seed equals)."""
    return np.random.default_rng(seed if salt is None else [seed, salt])


def _rand_bytes(rng, *shape, below=256):
    return _dev(rng.integers(0, below, shape, dtype=np.uint8))


def _theta3(C, rng, L=1):
    """test_gpu_kernels._theta / test_gpu_deep16._stack_inputs: the reference's 3by3 initialisation."""
    return np.concatenate([O.flatten(O.init_theta_3by3(C, rng, np.float64)) for _ in range(L)]).astype(np.float32)


# ---------------------------------------------------------------------------
# asr_conv_forward / asr_conv_backward and their k x k forms
# ---------------------------------------------------------------------------
# (id, dtype, k, (N, H, W, C))
CONV = [
    ("f32-valu-1x7x13x5", "f32", 3, (1, 7, 13, 5)),          # mask bits not byte-aligned per pixel, padded last word
    ("f32-mfma-2x5x8x16", "f32", 3, (2, 5, 8, 16)),
    ("f32-mfma-1x5x16x32", "f32", 3, (1, 5, 16, 32)),
    ("f32-mfma-1x6x32x64", "f32", 3, (1, 6, 32, 64)),        # partial band
    ("bf16-w32-2x5x32x16", "bf16", 3, (2, 5, 32, 16)),
    ("bf16-w32-1x6x32x64", "bf16", 3, (1, 6, 32, 64)),
    ("bf16-rows-1x5x8x64", "bf16", 3, (1, 5, 8, 64)),        # a tile spans two rows and the last is absent
    ("bf16-rows-2x5x16x32", "bf16", 3, (2, 5, 16, 32)),
    ("bf16-strips-1x5x48x16", "bf16", 3, (1, 5, 48, 16)),    # a full strip plus a 16-column strip
    ("bf16-strips-1x4x80x64", "bf16", 3, (1, 4, 80, 64)),
    ("bf16-wide-1x5x8x128", "bf16", 3, (1, 5, 8, 128)),
    ("bf16-wide-3x5x16x128", "bf16", 3, (3, 5, 16, 128)),    # two items a pass with one left over
    ("bf16-wide-1x5x48x256", "bf16", 3, (1, 5, 48, 256)),
    ("bf16-wide-3x32x32x256", "bf16", 3, (3, 32, 32, 256)),  # 3 slab rows (test_wgrad_more_items_than_slab_rows)
    ("f32-k5-1x5x7x3", "f32", 5, (1, 5, 7, 3)),
    ("bf16-k5-2x5x16x32", "bf16", 5, (2, 5, 16, 32)),
    ("bf16-k7-1x5x8x16", "bf16", 7, (1, 5, 8, 16)),
]
CONV_IDS = [c[0] for c in CONV]
# one shape per asr_conv_backward path for the single-output requests
CONV_SKIP = [c for c in CONV if c[0] in ("f32-valu-1x7x13x5", "f32-mfma-2x5x8x16", "bf16-w32-2x5x32x16",
                                         "bf16-rows-1x5x8x64", "bf16-strips-1x5x48x16", "bf16-wide-3x5x16x128",
                                         "f32-k5-1x5x7x3", "bf16-k5-2x5x16x32")]

_CONV_DATA = {}


class ConvCase:
    """Operands of one conv case on the GPU (never modified) and the wrapper's results.

    With a `salt` (tests/test_gpu_streams.py): another, independent draw of the same operands and
    nothing computed from them; the backward's mask is then random bits."""

    def __init__(self, rt, name, dtype, k, shape, salt=None):
        N, H, W, C = shape
        self.k, self.shape, self.bf = k, shape, dtype == "bf16"
        self.dt = rt.ASR_BF16 if self.bf else rt.ASR_F32
        self.tdt = rt.torch_dtype(self.dt)
        rng = _rng(sum(map(ord, name)), salt)
        if k == 3:
            self.pm = rt.param_map(C)
            th = _theta3(C, rng)
        else:  # test_gpu_kxk_bf16._case
            self.pm = rt.param_map(C, rt.ASR_PARAM_GENERAL, True, k)
            th = (0.2 * rng.standard_normal(self.pm.n_theta)).astype(np.float32)
        self.w = rt.theta_to_w(_dev(th), C, self.pm, GAMMA, self.dt)
        self.x = _dev(rng.standard_normal(shape).astype(np.float32), self.bf)
        self.dy = _dev(rng.standard_normal(shape).astype(np.float32), self.bf)
        self.bias = _dev((rng.standard_normal(C) * 0.1).astype(np.float32))
        self.mb = rt.mask_bytes(N, H, W, C)
        self.theta_dst = self.pm.device(self.x.device)[1]
        if salt is not None:
            self.mask = _rand_bytes(rng, self.mb)
            return
        # the wrapper's results: forward (zeroed mask), then the backward on that mask
        self.want_fwd, self.want_bwd = {}, {}
        for mode in (rt.ASR_MODE_EULER, rt.ASR_MODE_CONV):
            m = torch.zeros(self.mb, dtype=torch.uint8, device="cuda") if mode == rt.ASR_MODE_EULER else None
            y = rt.conv_forward(mode, self.x, self.w, self.bias, H_STEP, m, k=k)
            self.want_fwd[mode] = {"y": y, "mask": m}
        self.mask = self.want_fwd[rt.ASR_MODE_EULER]["mask"]

    def wrapper_backward(self, rt, mode):
        if mode not in self.want_bwd:
            m = self.mask if mode == rt.ASR_MODE_EULER else None
            dx, dth, db, dw = rt.conv_backward(mode, self.dy, self.x, m, self.w, self.pm, H_STEP, GAMMA, want_dw=True)
            self.want_bwd[mode] = {"dx": dx, "dtheta": dth, "dbias": db, "dw": dw}
        return self.want_bwd[mode]

    def ws_bytes(self):
        lib = _lib_()
        N, H, W, C = self.shape
        if self.k == 3:
            return int(lib.asr_conv_backward_workspace_bytes(N, H, W, C, self.dt))
        if self.bf:
            return int(lib.asr_conv_backward_workspace_bytes_k_bf16(N, H, W, C, self.k))
        return int(lib.asr_conv_backward_workspace_bytes_k(N, H, W, C, self.k))

    def forward(self, B, mode, euler):
        N, H, W, C = self.shape
        x, w, b = B.inp(self.x, "x"), B.inp(self.w, "w"), B.inp(self.bias, "bias")
        y = B.out(self.shape, self.tdt, "y")
        mask = B.out((self.mb,), torch.uint8, "mask") if euler else None
        if self.k == 3:
            B.call("asr_conv_forward", mode, _p(x), _p(y), _p(mask), _p(w), _p(b), H_STEP, N, H, W, C, self.dt, _stream())
        else:
            B.call("asr_conv_forward_k_bf16" if self.bf else "asr_conv_forward_k", mode, self.k, _p(x), _p(y), _p(mask),
                   _p(w), _p(b), H_STEP, N, H, W, C, _stream())
        return {"y": y, "mask": mask}

    def backward(self, B, mode, euler, outs=("dx", "dtheta", "dbias", "dw")):
        N, H, W, C = self.shape
        k = self.k
        dy, x, w = B.inp(self.dy, "dy"), B.inp(self.x, "x"), B.inp(self.w, "w")
        mask = B.inp(self.mask, "mask") if euler else None
        tdst = B.inp(self.theta_dst, "theta_dst")
        dx = B.out(self.shape, self.tdt, "dx") if "dx" in outs else None
        dth = B.out((self.pm.n_theta,), torch.float32, "dtheta") if "dtheta" in outs else None
        db = B.out((C,), torch.float32, "dbias") if "dbias" in outs else None
        dw = B.out((k, k, C, C), torch.float32, "dw") if "dw" in outs else None
        wsb = self.ws_bytes()
        ws = B.out((wsb,), torch.uint8, "workspace")
        if k == 3:
            B.call("asr_conv_backward", mode, _p(dy), _p(x), _p(mask), _p(w), _p(tdst), self.pm.n_theta, H_STEP, GAMMA,
                   N, H, W, C, self.dt, _p(dx), _p(dth), _p(db), _p(dw), _p(ws), wsb, _stream())
        else:
            B.call("asr_conv_backward_k_bf16" if self.bf else "asr_conv_backward_k", mode, k, _p(dy), _p(x), _p(mask),
                   _p(w), _p(tdst), self.pm.n_theta, H_STEP, GAMMA, N, H, W, C, _p(dx), _p(dth), _p(db), _p(dw), _p(ws),
                   wsb, _stream())
        return {"dx": dx, "dtheta": dth, "dbias": db, "dw": dw}


def _conv_case(rt, case, salt=None):
    if (case[0], salt) not in _CONV_DATA:
        _CONV_DATA[case[0], salt] = ConvCase(rt, *case, salt=salt)
    return _CONV_DATA[case[0], salt]


@pytest.mark.parametrize("mode_name", ["euler", "conv"])
@pytest.mark.parametrize("case", CONV, ids=CONV_IDS)
def test_conv_forward(rt, case, mode_name):
    """y and, in EULER mode, the mask (never pre-zeroed here; its padding bits up to asr_mask_bytes included)."""
    c = _conv_case(rt, case)
    euler = mode_name == "euler"
    mode = rt.ASR_MODE_EULER if euler else rt.ASR_MODE_CONV
    want = {k: v for k, v in c.want_fwd[mode].items() if v is not None}
    _both(lambda B: c.forward(B, mode, euler), want)


@pytest.mark.parametrize("mode_name", ["euler", "conv"])
@pytest.mark.parametrize("case", CONV, ids=CONV_IDS)
def test_conv_backward(rt, case, mode_name):
    """dx, dtheta, dbias and dw with the slab workspace prefilled 0x00 and 0xFF (a reduction that reads a
    slab row nobody wrote, or a row partly written, sums NaNs in the second run)."""
    c = _conv_case(rt, case)
    euler = mode_name == "euler"
    mode = rt.ASR_MODE_EULER if euler else rt.ASR_MODE_CONV
    _both(lambda B: c.backward(B, mode, euler), c.wrapper_backward(rt, mode))


@pytest.mark.parametrize("only", ["dx", "dtheta", "dbias", "dw"])
@pytest.mark.parametrize("case", CONV_SKIP, ids=[c[0] for c in CONV_SKIP])
def test_conv_backward_single_output(rt, case, only):
    """dx, dtheta, dbias and dw_hwio may each be NULL (include/asr.h): each requested alone, on a 0xFF
    workspace, equals the same output of the all-outputs call bitwise."""
    c = _conv_case(rt, case)
    want = c.wrapper_backward(rt, rt.ASR_MODE_EULER)
    B = Bufs(0xFF)
    got = c.backward(B, rt.ASR_MODE_EULER, True, outs=(only,))
    B.check()
    assert _same(got[only], want[only]), f"{only} requested alone differs from the all-outputs run"


# ---------------------------------------------------------------------------
# RK2 block
# ---------------------------------------------------------------------------
RK2 = [("f32", (1, 7, 13, 5)), ("bf16", (2, 5, 32, 16)), ("bf16", (1, 8, 32, 64))]
RK2_IDS = [f"{d}-{'x'.join(map(str, s))}" for d, s in RK2]
_RK2_DATA = {}


def _rk2_case(rt, dtype, shape, salt=None):
    """With a salt: an independent draw, nothing computed from it (x_mid random values, the masks random bits)."""
    key = (dtype, shape, salt)
    if key not in _RK2_DATA:
        N, H, W, C = shape
        bf = dtype == "bf16"
        rng = _rng(C * 100 + H, salt)
        d = dict(bf=bf, dt=rt.ASR_BF16 if bf else rt.ASR_F32, pm=rt.param_map(C))
        d["tdt"] = rt.torch_dtype(d["dt"])
        d["w"] = rt.theta_to_w(_dev(_theta3(C, rng)), C, d["pm"], GAMMA, d["dt"])
        d["x"] = _dev(rng.standard_normal(shape).astype(np.float32), bf)
        d["dy"] = _dev(rng.standard_normal(shape).astype(np.float32), bf)
        d["bias"] = _dev((rng.standard_normal(C) * 0.1).astype(np.float32))
        d["mb"] = rt.mask_bytes(N, H, W, C)
        _RK2_DATA[key] = d
        if salt is not None:
            d["fwd"] = {"xmid": _dev(rng.standard_normal(shape).astype(np.float32), bf),
                        "mask1": _rand_bytes(rng, d["mb"]), "mask2": _rand_bytes(rng, d["mb"])}
            return d
        y, xm, m1, m2 = rt.rk2_forward(d["x"], d["w"], d["bias"], H_STEP)
        d["fwd"] = {"y": y, "xmid": xm, "mask1": m1, "mask2": m2}
        dx, dth, db, dw = rt.rk2_backward(d["dy"], d["x"], xm, m1, m2, d["w"], d["pm"], H_STEP, GAMMA, want_dw=True)
        d["bwd"] = {"dx": dx, "dtheta": dth, "dbias": db, "dw": dw}
    return _RK2_DATA[key]


def _rk2_forward(B, d, shape):
    N, H, W, C = shape
    x, w, b = B.inp(d["x"], "x"), B.inp(d["w"], "w"), B.inp(d["bias"], "bias")
    xm, y = B.out(shape, d["tdt"], "xmid"), B.out(shape, d["tdt"], "y")
    m1, m2 = B.out((d["mb"],), torch.uint8, "mask1"), B.out((d["mb"],), torch.uint8, "mask2")
    B.call("asr_rk2_forward", _p(x), _p(xm), _p(y), _p(m1), _p(m2), _p(w), _p(b), H_STEP, N, H, W, C, d["dt"], _stream())
    return {"y": y, "xmid": xm, "mask1": m1, "mask2": m2}


def _rk2_backward(B, d, shape, outs=("dx", "dtheta", "dbias", "dw")):
    N, H, W, C = shape
    pm, f = d["pm"], d["fwd"]
    dy, x, xm = B.inp(d["dy"], "dy"), B.inp(d["x"], "x"), B.inp(f["xmid"], "xmid")
    m1, m2, w = B.inp(f["mask1"], "mask1"), B.inp(f["mask2"], "mask2"), B.inp(d["w"], "w")
    tdst = B.inp(pm.device(dy.device)[1], "theta_dst")
    dx = B.out(shape, d["tdt"], "dx") if "dx" in outs else None
    dth = B.out((pm.n_theta,), torch.float32, "dtheta") if "dtheta" in outs else None
    db = B.out((C,), torch.float32, "dbias") if "dbias" in outs else None
    dw = B.out((3, 3, C, C), torch.float32, "dw") if "dw" in outs else None
    wsb = int(_lib_().asr_rk2_backward_workspace_bytes(N, H, W, C, d["dt"]))
    ws = B.out((wsb,), torch.uint8, "workspace")
    B.call("asr_rk2_backward", _p(dy), _p(x), _p(xm), _p(m1), _p(m2), _p(w), _p(tdst), pm.n_theta, H_STEP, GAMMA, N, H,
           W, C, d["dt"], _p(dx), _p(dth), _p(db), _p(dw), _p(ws), wsb, _stream())
    return {"dx": dx, "dtheta": dth, "dbias": db, "dw": dw}


@pytest.mark.parametrize("dtype,shape", RK2, ids=RK2_IDS)
def test_rk2_forward(rt, dtype, shape):
    d = _rk2_case(rt, dtype, shape)
    _both(lambda B: _rk2_forward(B, d, shape), d["fwd"])


@pytest.mark.parametrize("dtype,shape", RK2, ids=RK2_IDS)
def test_rk2_backward(rt, dtype, shape):
    """Both stages' slabs (the second stage's added onto the first's) on a 0x00 and a 0xFF workspace."""
    d = _rk2_case(rt, dtype, shape)
    _both(lambda B: _rk2_backward(B, d, shape), d["bwd"])


@pytest.mark.parametrize("only", ["dx", "dtheta", "dbias", "dw"])
@pytest.mark.parametrize("dtype,shape", RK2[:2], ids=RK2_IDS[:2])
def test_rk2_backward_single_output(rt, dtype, shape, only):
    d = _rk2_case(rt, dtype, shape)
    B = Bufs(0xFF)
    got = _rk2_backward(B, d, shape, outs=(only,))
    B.check()
    assert _same(got[only], d["bwd"][only]), f"{only} requested alone differs from the all-outputs run"


# ---------------------------------------------------------------------------
# Block stacks (asr_block_stack_*, asr_rk2_stack_*)
# ---------------------------------------------------------------------------
# (id, dtype, (N, H, W, C), L)
STACKS = [
    ("deep16", "bf16", (3, 32, 32, 16), 3),            # one fused launch, images resident in LDS
    ("c64", "bf16", (2, 16, 32, 64), 2),               # k_fwd3_stack / k_bwd3_stack, in-launch slab reduction
    ("per-block-c128", "bf16", (2, 6, 16, 128), 2),    # the per-block fallback
    ("stage-img-bf16", "bf16", (3, 8, 8, 32), 3),      # image-resident stage kernels (strided calls below)
    ("stage-img-f32", "f32", (3, 16, 16, 32), 3),
]
_STACK_DATA = {}


def _stack_case(rt, name, salt=None):
    """With a salt: an independent draw, nothing computed from it (the blocks' inputs random values, the masks
    random bits)."""
    if (name, salt) not in _STACK_DATA:
        _, dtype, shape, L = next(s for s in STACKS if s[0] == name)
        N, H, W, C = shape
        bf = dtype == "bf16"
        rng = _rng(1000 * C + 10 * N + L, salt)
        d = dict(shape=shape, L=L, bf=bf, dt=rt.ASR_BF16 if bf else rt.ASR_F32, pm=rt.param_map(C))
        d["tdt"] = rt.torch_dtype(d["dt"])
        d["w"] = rt.theta_to_w(_dev(_theta3(C, rng, L)), C, d["pm"], GAMMA, d["dt"], layers=L).reshape(L, -1)
        d["bias"] = _dev((rng.standard_normal((L, C)) * 0.1).astype(np.float32))
        d["x0"] = _dev(rng.standard_normal(shape).astype(np.float32), bf)
        d["dyL"] = _dev((rng.standard_normal(shape) * 0.1).astype(np.float32), bf)
        d["P"], d["mb"], d["per"] = N * H * W * C, rt.mask_bytes(N, H, W, C), d["w"][0].numel()
        _STACK_DATA[name, salt] = d
        if salt is not None:
            d["xs"] = _dev(rng.standard_normal((L,) + shape).astype(np.float32), bf)
            d["masks"] = _rand_bytes(rng, L, d["mb"])
            return d
        ys, masks = rt.block_stack_forward(d["x0"], d["w"], d["bias"], H_STEP)
        d["ys"], d["masks"] = ys, masks
        d["xs"] = torch.cat([d["x0"].unsqueeze(0), ys[:L - 1]]).contiguous()
        dx0, dp = rt.block_stack_backward(d["dyL"], d["x0"], ys, masks, d["w"], d["pm"], H_STEP, GAMMA)
        d["dx0"], d["dp"] = dx0, dp
    return _STACK_DATA[name, salt]


def _strided(t, L, per, stride):
    """[L, per] rows `stride` elements apart in a flat tensor of (L-1)*stride + per elements (gaps: 0xFF bytes)."""
    flat = torch.empty((L - 1) * stride + per, dtype=t.dtype, device=t.device)
    flat.view(-1).view(torch.uint8).fill_(0xFF)
    for l in range(L):
        flat[l * stride:l * stride + per] = t[l].reshape(-1)
    return flat


def _rows(flat, L, per, stride):
    return torch.stack([flat[l * stride:l * stride + per] for l in range(L)])


def _gaps_keep(flat, L, per, stride, fill, what):
    g = _bytes(flat)
    e = flat.element_size()
    for l in range(L - 1):
        gap = g[(l * stride + per) * e:(l + 1) * stride * e]
        assert bool((gap == fill).all()), f"{what}: the gap after layer {l} lost its prefill"


def _stack_forward(B, d, ys_extra=0, mask_extra=0, bias_extra=0):
    N, H, W, C = d["shape"]
    L, P, mb, per = d["L"], d["P"], d["mb"], d["per"]
    ystr, mstr, bstr = P + ys_extra, mb + mask_extra, C + bias_extra
    x0, w = B.inp(d["x0"], "x0"), B.inp(d["w"], "w")
    bias = B.inp(_strided(d["bias"], L, C, bstr), "bias")
    ys = B.out(((L - 1) * ystr + P,), d["tdt"], "ys")
    masks = B.out(((L - 1) * mstr + mb,), torch.uint8, "masks")
    B.call("asr_block_stack_forward", _p(x0), _p(ys), ystr, _p(masks), mstr, _p(w), per, _p(bias), bstr, H_STEP, N, H, W,
           C, L, d["dt"], 1, _stream())
    return ys, masks, ystr, mstr


def _stack_backward(B, d, x_extra=0, want_dparams=True):
    N, H, W, C = d["shape"]
    L, P, mb, per, pm = d["L"], d["P"], d["mb"], d["per"], d["pm"]
    xstr = P + x_extra
    dyL, w = B.inp(d["dyL"], "dyL"), B.inp(d["w"], "w")
    xs = B.inp(_strided(d["xs"], L, P, xstr), "xs")
    masks = B.inp(d["masks"], "masks")
    tdst = B.inp(pm.device(dyL.device)[1], "theta_dst")
    wsb = int(_lib_().asr_block_stack_backward_workspace_bytes(N, H, W, C, L, d["dt"]))
    dx0 = B.out(d["shape"], d["tdt"], "dx0")
    dp = B.out((L, pm.n_theta + C), torch.float32, "dparams") if want_dparams else None
    ws = B.out((wsb,), torch.uint8, "workspace")
    B.call("asr_block_stack_backward", _p(dyL), _p(xs), xstr, _p(masks), mb, _p(w), per, _p(tdst), pm.n_theta, H_STEP,
           GAMMA, N, H, W, C, L, d["dt"], _p(dx0), _p(dp), _p(ws), wsb, _stream())
    return {"dx0": dx0, "dparams": dp}


STACK_TABLE = ["deep16", "c64", "per-block-c128"]


@pytest.mark.parametrize("name", STACK_TABLE)
def test_block_stack_forward(rt, name):
    d = _stack_case(rt, name)

    def launch(B):
        ys, masks, _, _ = _stack_forward(B, d)
        return {"ys": ys, "masks": masks}

    _both(launch, {"ys": d["ys"], "masks": d["masks"]})


@pytest.mark.parametrize("name,dparams", [("deep16", True), ("c64", True), ("c64", False), ("per-block-c128", True)])
def test_block_stack_backward(rt, name, dparams):
    """dx0 and dparams; at C = 64 also with dparams = NULL.  The C = 64 workspace reserves 512 slab rows
    per block of which a launch writes one per workgroup: the 0xFF run fails if the reduction reads more."""
    d = _stack_case(rt, name)
    want = {"dx0": d["dx0"], "dparams": d["dp"]}
    _both(lambda B: _stack_backward(B, d, want_dparams=dparams), want)


@pytest.mark.parametrize("name", ["deep16", "c64", "stage-img-bf16", "stage-img-f32"])
def test_block_stack_forward_strided(rt, name):
    """y_stride = P + 64 elements, mask_stride = mask bytes + 64, bias_stride = C + 4 (the documented
    alignment rules hold): the layers equal the naturally strided run and the gaps keep their prefill."""
    d = _stack_case(rt, name)
    L, P, mb = d["L"], d["P"], d["mb"]
    got = []
    for fill in PREFILLS:
        B = Bufs(fill)
        ys, masks, ystr, mstr = _stack_forward(B, d, 64, 64, 4)
        B.check()
        _gaps_keep(ys, L, P, ystr, fill, "ys")
        _gaps_keep(masks, L, mb, mstr, fill, "masks")
        got.append({"ys": _rows(ys, L, P, ystr), "masks": _rows(masks, L, mb, mstr)})
    _check_outputs(got, {"ys": d["ys"].reshape(L, -1), "masks": d["masks"]})


@pytest.mark.parametrize("name", ["deep16", "c64", "stage-img-bf16", "stage-img-f32"])
def test_block_stack_backward_strided(rt, name):
    """x_stride = P + 64 elements, the gaps between the layers' inputs NaN."""
    d = _stack_case(rt, name)
    _both(lambda B: _stack_backward(B, d, x_extra=64), {"dx0": d["dx0"], "dparams": d["dp"]})


_RK2S = {}


def _rk2_stack_case(rt, salt=None):
    """With a salt: an independent draw, nothing computed from it (as _stack_case)."""
    if salt not in _RK2S:
        N, H, W, C, L = 2, 16, 32, 64, 2
        shape = (N, H, W, C)
        rng = _rng(N * 5 + L, salt)
        d = _RK2S[salt] = {}
        d.update(shape=shape, L=L, pm=rt.param_map(C), P=N * H * W * C, mb=rt.mask_bytes(N, H, W, C))
        d["w"] = rt.theta_to_w(_dev(_theta3(C, rng, L)), C, d["pm"], GAMMA, rt.ASR_BF16, layers=L).reshape(L, -1)
        d["bias"] = _dev((rng.standard_normal((L, C)) * 0.1).astype(np.float32))
        d["x0"] = _dev(rng.standard_normal(shape).astype(np.float32), True)
        d["dyL"] = _dev((rng.standard_normal(shape) * 0.1).astype(np.float32), True)
        if salt is not None:
            d["xs"] = _dev(rng.standard_normal((L,) + shape).astype(np.float32), True)
            d["xm"] = _dev(rng.standard_normal((L,) + shape).astype(np.float32), True)
            d["m1"], d["m2"] = _rand_bytes(rng, L, d["mb"]), _rand_bytes(rng, L, d["mb"])
            return d
        d["ys"], d["xm"], d["m1"], d["m2"] = rt.rk2_stack_forward(d["x0"], d["w"], d["bias"], H_STEP)
        d["xs"] = torch.cat([d["x0"].unsqueeze(0), d["ys"][:L - 1]]).contiguous()
        d["dx0"], d["dp"] = rt.rk2_stack_backward(d["dyL"], d["x0"], d["ys"], d["xm"], d["m1"], d["m2"], d["w"], d["pm"],
                                                  H_STEP, GAMMA)
    return _RK2S[salt]


def _rk2_stack_forward(B, rt, d):
    N, H, W, C = d["shape"]
    L, P, mb = d["L"], d["P"], d["mb"]
    x0, w, bias = B.inp(d["x0"], "x0"), B.inp(d["w"], "w"), B.inp(d["bias"], "bias")
    ys, xm = B.out((L,) + d["shape"], torch.bfloat16, "ys"), B.out((L,) + d["shape"], torch.bfloat16, "xmids")
    m1, m2 = B.out((L, mb), torch.uint8, "masks1"), B.out((L, mb), torch.uint8, "masks2")
    B.call("asr_rk2_stack_forward", _p(x0), _p(ys), _p(xm), P, _p(m1), _p(m2), mb, _p(w), d["w"][0].numel(), _p(bias),
           C, H_STEP, N, H, W, C, L, rt.ASR_BF16, _stream())
    return {"ys": ys, "xmids": xm, "masks1": m1, "masks2": m2}


def _rk2_stack_backward(B, rt, d):
    N, H, W, C = d["shape"]
    L, P, mb, pm = d["L"], d["P"], d["mb"], d["pm"]
    dyL, xs, xm = B.inp(d["dyL"], "dyL"), B.inp(d["xs"], "xs"), B.inp(d["xm"], "xmids")
    m1, m2, w = B.inp(d["m1"], "masks1"), B.inp(d["m2"], "masks2"), B.inp(d["w"], "w")
    tdst = B.inp(pm.device(dyL.device)[1], "theta_dst")
    wsb = int(_lib_().asr_rk2_stack_backward_workspace_bytes(N, H, W, C, L, rt.ASR_BF16))
    dx0, dp = B.out(d["shape"], torch.bfloat16, "dx0"), B.out((L, pm.n_theta + C), torch.float32, "dparams")
    ws = B.out((wsb,), torch.uint8, "workspace")
    B.call("asr_rk2_stack_backward", _p(dyL), _p(xs), _p(xm), P, _p(m1), _p(m2), mb, _p(w), d["w"][0].numel(),
           _p(tdst), pm.n_theta, H_STEP, GAMMA, N, H, W, C, L, rt.ASR_BF16, _p(dx0), _p(dp), _p(ws), wsb, _stream())
    return {"dx0": dx0, "dparams": dp}


def test_rk2_stack_forward(rt):
    d = _rk2_stack_case(rt)
    _both(lambda B: _rk2_stack_forward(B, rt, d), {"ys": d["ys"], "xmids": d["xm"], "masks1": d["m1"], "masks2": d["m2"]})


def test_rk2_stack_backward(rt):
    d = _rk2_stack_case(rt)
    _both(lambda B: _rk2_stack_backward(B, rt, d), {"dx0": d["dx0"], "dparams": d["dp"]})


# ---------------------------------------------------------------------------
# Transitions (fp32, stride 2: TF's asymmetric padding)
# ---------------------------------------------------------------------------
def _transition_case(rt, dims, S=2, salt=None):
    """Operands of one transition and, without a salt, the wrapper's results (with one: an independent draw,
    nothing computed from it, the mask's bytes random 0 / 1)."""
    N, H, W, Ci, Co = dims
    rng = _rng(N * 100 + H + Ci, salt)  # test_gpu_stages.test_transition_vs_oracle
    d = dict(dims=dims, S=S, out_shape=(N, -(-H // S), -(-W // S), Co))
    d["x"] = _dev(rng.standard_normal((N, H, W, Ci)).astype(np.float32))
    d["k2"] = _dev((rng.standard_normal((3, 3, Ci, Co)) * np.sqrt(2 / (9 * Ci))).astype(np.float32))
    d["k1"] = _dev((rng.standard_normal((1, 1, Ci, Co)) * np.sqrt(2 / Ci)).astype(np.float32))
    d["b2"] = _dev((rng.standard_normal(Co) * 0.1).astype(np.float32))
    d["b1"] = _dev((rng.standard_normal(Co) * 0.1).astype(np.float32))
    d["dy"] = _dev(rng.standard_normal(d["out_shape"]).astype(np.float32))
    if salt is not None:
        d["mask"] = _rand_bytes(rng, *d["out_shape"], below=2)
        return d
    d["y"], d["mask"] = rt.transition_forward(d["x"], d["k2"], d["b2"], d["k1"], d["b1"], S)
    d["dx"], d["dparams"] = rt.transition_backward(d["dy"], d["x"], d["mask"], d["k2"], d["k1"], S)
    return d


def _transition_forward(B, d):
    N, H, W, Ci, Co = d["dims"]
    xi, k2i, b2i, k1i, b1i = (B.inp(d[n], n) for n in ("x", "k2", "b2", "k1", "b1"))
    y, mask = B.out(d["out_shape"], torch.float32, "y"), B.out(d["out_shape"], torch.uint8, "mask")
    B.call("asr_transition_forward", _p(xi), _p(y), _p(mask), _p(k2i), _p(b2i), _p(k1i), _p(b1i), N, H, W, Ci, Co, d["S"],
           _stream())
    return {"y": y, "mask": mask}


def _transition_backward(B, d):
    N, H, W, Ci, Co = d["dims"]
    dyi, xi, mi, k2i, k1i = (B.inp(d[n], n) for n in ("dy", "x", "mask", "k2", "k1"))
    dx = B.out((N, H, W, Ci), torch.float32, "dx")
    dp = B.out((9 * Ci * Co + Co + Ci * Co + Co,), torch.float32, "dparams")
    nb = int(_lib_().asr_transition_backward_workspace_bytes(N, H, W, Ci, Co, d["S"]))
    ws = B.out((max(nb, 1),), torch.uint8, "workspace")
    B.call("asr_transition_backward", _p(dyi), _p(xi), _p(mi), _p(k2i), _p(k1i), N, H, W, Ci, Co, d["S"], _p(dx), _p(dp),
           _p(ws), nb, _stream())
    return {"dx": dx, "dparams": dp}


TRANSITIONS = [(2, 7, 9, 5, 6), (2, 16, 16, 32, 64), (1, 8, 8, 64, 128)]


@pytest.mark.parametrize("N,H,W,Ci,Co", TRANSITIONS)
def test_transition(rt, N, H, W, Ci, Co):
    d = _transition_case(rt, (N, H, W, Ci, Co))
    _both(lambda B: _transition_forward(B, d), {"y": d["y"], "mask": d["mask"]})
    _both(lambda B: _transition_backward(B, d), {"dx": d["dx"], "dparams": d["dparams"]})


# ---------------------------------------------------------------------------
# asr_theta_to_w, _k, _k_bf16 with layer strides
# ---------------------------------------------------------------------------
THETA = [("f32-hwio", False, 3, 5), ("bf16-balanced-c64", True, 3, 64), ("bf16-nearest-c128", True, 3, 128),
         ("f32-k5", False, 5, 3), ("bf16-k5-pack", True, 5, 16)]


def _theta_case(rt, bf, k, C, salt=None):
    """L = 2 strided thetas (the gap NaN) and the strides; `salt`: an independent draw."""
    L = 2
    dt = rt.ASR_BF16 if bf else rt.ASR_F32
    pm = rt.param_map(C) if k == 3 else rt.param_map(C, rt.ASR_PARAM_GENERAL, True, k)
    nt = pm.n_theta
    rng = _rng(C + k, salt)
    th = _theta3(C, rng, L) if k == 3 else (0.2 * rng.standard_normal(L * nt)).astype(np.float32)
    th = _dev(th).reshape(L, nt)
    per = (rt.wpack_elems(C) if k == 3 else rt.wpack_elems_k(C, k)) if bf else k * k * C * C
    tstr, wstr = nt + C + 3, per + 64
    return dict(L=L, C=C, k=k, bf=bf, dt=dt, pm=pm, th=th, per=per, tstr=tstr, wstr=wstr,
                theta=_strided(th, L, nt, tstr), w_src=pm.device(th.device)[0])


def _theta_to_w(B, d):
    L, C, k, per, tstr, wstr = d["L"], d["C"], d["k"], d["per"], d["tstr"], d["wstr"]
    t_in, src = B.inp(d["theta"], "theta"), B.inp(d["w_src"], "w_src")
    w = B.out(((L - 1) * wstr + per,), torch.bfloat16 if d["bf"] else torch.float32, "w_out")
    if k == 3:
        B.call("asr_theta_to_w", _p(t_in), tstr, L, C, _p(src), GAMMA, _p(w), wstr, d["dt"], _stream())
    else:
        B.call("asr_theta_to_w_k_bf16" if d["bf"] else "asr_theta_to_w_k", _p(t_in), tstr, L, C, k, _p(src), GAMMA, _p(w),
               wstr, _stream())
    return {"w_out": w}


@pytest.mark.parametrize("name,bf,k,C", THETA)
def test_theta_to_w_strided(rt, name, bf, k, C):
    """L = 2, w_stride = per-layer elements + 64, theta_stride = n_theta + C + 3 (the gap between the
    thetas NaN): each layer equals the naturally strided run's, the gap in w keeps its prefill."""
    d = _theta_case(rt, bf, k, C)
    L, per, wstr = d["L"], d["per"], d["wstr"]
    want = rt.theta_to_w(d["th"].reshape(-1), C, d["pm"], GAMMA, d["dt"], layers=L).reshape(L, -1)
    assert want[0].numel() == per and want.dtype == (torch.bfloat16 if bf else torch.float32)
    got = []
    for fill in PREFILLS:
        B = Bufs(fill)
        w = _theta_to_w(B, d)["w_out"]
        B.check()
        _gaps_keep(w, L, per, wstr, fill, "w_out")
        got.append({"w": _rows(w, L, per, wstr)})
    _check_outputs(got, {"w": want})


# ---------------------------------------------------------------------------
# Optimiser kernels: params and state are read-modify-write (valid contents, 0xFF guards)
# ---------------------------------------------------------------------------
OPT = [("sgd-momentum", 0, 0, 0.01, 0.9, 0.0, 0.0), ("sgd-nesterov", 0, 1, 0.01, 0.9, 0.0, 0.0),
       ("adam", 1, 0, 1e-3, 0.9, 0.999, 1e-7), ("adam-amsgrad", 1, 2, 1e-3, 0.9, 0.999, 1e-7),
       ("rmsprop", 2, 0, 1e-3, 0.9, 0.0, 1e-7)]
OPT_SIZES = [1000, 4096 * 256 + 300]  # the grid is capped at 4096 x 256 threads: the loop wraps


def _opt_data(n, slots, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    p = torch.randn(n, device="cuda", generator=g)
    grads = torch.randn(n, device="cuda", generator=g)
    state = torch.randn(slots * n, device="cuda", generator=g).abs_() * 0.1  # (second moments are >= 0)
    return p, grads, state


def _optimizer_update(B, cfg, p, grads, state):
    pi, gi, si = B.inp(p, "params"), B.inp(grads, "grads"), B.inp(state, "state")
    B.call("asr_optimizer_update", ct.byref(cfg), _p(pi), _p(gi), _p(si), p.numel(), _stream())
    return {"params": pi, "state": si}


def _adam_update(B, p, grads, m, v, hp):
    pi, gi, mi, vi = B.inp(p, "params"), B.inp(grads, "grads"), B.inp(m, "m"), B.inp(v, "v")
    B.call("asr_adam_update", _p(pi), _p(gi), _p(mi), _p(vi), p.numel(), *hp, _stream())
    return {"params": pi, "m": mi, "v": vi}


@pytest.mark.parametrize("n", OPT_SIZES)
@pytest.mark.parametrize("name,kind,flags,lr,a,b,eps", OPT, ids=[o[0] for o in OPT])
def test_optimizer_update(rt, name, kind, flags, lr, a, b, eps, n):
    """All five kinds / flags, `state` carved at exactly slots * n floats.  params and state are
    read-modify-write, so there is no prefill to vary: valid contents between NaN guards, one run,
    equal bitwise to the wrapper's update of copies."""
    from differential_equations_resnet_amd import _lib
    slots = rt.optimizer_slots(kind, flags)
    p, grads, state = _opt_data(n, slots, n % 1000 + kind)
    cfg = _lib.OptimizerConfig(kind, flags, lr, a, b, eps, 3, 0.125)
    p_want, s_want = p.clone(), state.clone()
    rt.optimizer_update(cfg, p_want, grads, s_want)
    B = Bufs(0xFF)
    got = _optimizer_update(B, cfg, p, grads, state)
    assert got["state"].numel() == slots * n
    B.check()
    _equal_wrapper(got, {"params": p_want, "state": s_want})
    assert not _same(got["params"], p)


@pytest.mark.parametrize("n", OPT_SIZES)
def test_adam_update(rt, n):
    p, grads, state = _opt_data(n, 2, n % 1000 + 7)
    m, v = state[:n].clone(), state[n:].clone()
    hp = (1e-3, 0.9, 0.999, 1e-7, 3, 0.125)
    p_want, m_want, v_want = p.clone(), m.clone(), v.clone()
    rt.adam_update(p_want, grads, m_want, v_want, *hp)
    B = Bufs(0xFF)
    got = _adam_update(B, p, grads, m, v, hp)
    B.check()
    _equal_wrapper(got, {"params": p_want, "m": m_want, "v": v_want})
    assert not _same(got["params"], p)


# ---------------------------------------------------------------------------
# The augmentation launch
# ---------------------------------------------------------------------------
AUGMENT = ["crop_flip_u8_n1", "pad_height_u8"]


def _augment_case(name, salt=None):
    """The plan, its config and item table, and the source images (`salt`: other random images, the same table)."""
    from differential_equations_resnet_amd import _lib
    _, src, plan, table, _ = next(c for c in A.cases() if c[0] == name)
    if salt is not None:
        src = _rng(len(name), salt).integers(0, 256, src.shape, dtype=src.dtype)
    Hs, Ws, C = plan.in_shape
    Ho, Wo, _ = plan.out_shape
    out_u8 = np.dtype(plan.out_dtype) == np.uint8
    color = list(plan.color) + [_lib.ASR_AUG_NONE] * (2 - len(plan.color))
    cfg = _lib.AugPlanConfig(Hs, Ws, C, _lib.ASR_U8, Ho, Wo, _lib.ASR_U8 if out_u8 else _lib.ASR_F32, int(plan.resize),
                             int(plan.resized[0]), int(plan.resized[1]), int(plan.pad[0]), int(plan.pad[1]),
                             int(bool(plan.flip_src)), (ct.c_int * 2)(*color))
    return dict(plan=plan, cfg=cfg, N=len(table), out_shape=(len(table), Ho, Wo, C),
                out_dtype=torch.uint8 if out_u8 else torch.float32, feats=torch.from_numpy(src).cuda(),
                items=torch.from_numpy(table.view(np.uint8).copy()).cuda())


def _augment_batch(B, d):
    f, it = B.inp(d["feats"], "src"), B.inp(d["items"], "items")
    out = B.out(d["out_shape"], d["out_dtype"], "out")
    B.call("asr_augment_batch", _p(f), int(d["feats"].shape[0]), ct.byref(d["cfg"]), _p(it), d["N"], _p(out), _stream())
    return {"out": out}


@pytest.mark.parametrize("name", AUGMENT)
def test_augment_batch(rt, name):
    """The smallest cropping plan with uint8 output and the smallest cropping + padding plan (float32
    output, whose zero border the kernel writes itself) of tests/test_augment_gpu.py."""
    d = _augment_case(name)
    want = rt.augment_batch(d["feats"], d["plan"], d["items"])
    assert (d["out_dtype"] == torch.uint8) == (name == "crop_flip_u8_n1") and want.dtype == d["out_dtype"]
    _both(lambda B: _augment_batch(B, d), {"out": want})


# ---------------------------------------------------------------------------
# The executors' workspaces
# ---------------------------------------------------------------------------
def _net_executor(rt, dtype, N, H, W, C, L, k=3, integrator="euler", inference=False, salt=None):
    """(executor, params, the generator for images and targets, its prepare call); `salt`: independent draws."""
    kw = dict(param_kind=rt.ASR_PARAM_GENERAL, kernel_size=k) if k != 3 else {}
    ex = rt.NetExecutor(N, H, W, 3, C, L, 10, H_STEP, GAMMA, subtract_mean=127.5, divide_by_stddev=127.5, dtype=dtype,
                        integrator=integrator, inference=inference, **kw)
    rng = _rng(C + L + k, salt)
    if k == 3:
        from differential_equations_resnet_amd.netparams import init_net_params
        params = init_net_params(C, L, 3, 10, seed=5 if salt is None else 1000 + salt, bias_std=0.05)
    else:
        spec = KO.KNetSpec(C=C, L=L, h=H_STEP, gamma=GAMMA, H=H, W=W, kind="general", k1=3, kb=k)
        params = O.flatten(KO.init_params(spec, rng))
    return ex, _dev(np.asarray(params, np.float32)), rng, "asr_net_prepare"


def _stages_executor(rt, dtype, salt=None):
    stages = [(16, 1, 0), (32, 1, 2), (64, 1, 2)]
    ex = rt.StagesExecutor(2, 32, 32, 3, stages, 10, H_STEP, GAMMA, subtract_mean=127.5, divide_by_stddev=127.5,
                           dtype=dtype)
    spec = O.StagesSpec(stages=stages, h=H_STEP, gamma=GAMMA, H=32, W=32, kind="3by3", antisymmetric=True)
    rng = _rng(0, salt)
    params = O.stages_init_params(spec, rng, np.float64, bias_std=0.05)  # test_gpu_stages._stages_setup
    params[-2] = params[-2] * 0.05
    return ex, _dev(O.flatten(params).astype(np.float32)), rng, "asr_stages_prepare"


EXECUTORS = {
    "net-bf16-c16": lambda rt, salt=None: _net_executor(rt, "bfloat16", 2, 32, 32, 16, 2, salt=salt),
    "net-bf16-c64-euler": lambda rt, salt=None: _net_executor(rt, "bfloat16", 2, 32, 32, 64, 2, salt=salt),
    "net-bf16-c64-rk2": lambda rt, salt=None: _net_executor(rt, "bfloat16", 2, 32, 32, 64, 2, integrator="rk2",
                                                            salt=salt),
    "net-bf16-c128": lambda rt, salt=None: _net_executor(rt, "bfloat16", 2, 8, 16, 128, 2, salt=salt),
    "net-bf16-k5": lambda rt, salt=None: _net_executor(rt, "bfloat16", 2, 16, 16, 16, 2, k=5, salt=salt),
    "net-f32": lambda rt, salt=None: _net_executor(rt, "float32", 2, 7, 9, 5, 2, salt=salt),
    "stages-f32": lambda rt, salt=None: _stages_executor(rt, "float32", salt=salt),
    "stages-bf16": lambda rt, salt=None: _stages_executor(rt, "bfloat16", salt=salt),
    "net-bf16-c64-inference": lambda rt, salt=None: _net_executor(rt, "bfloat16", 2, 32, 32, 64, 2, inference=True,
                                                                  salt=salt),
}


@pytest.mark.parametrize("name", list(EXECUTORS))
def test_executor_workspace(rt, name):
    """The executor's workspace (masks, activations, slabs, group rows: carved from one reused buffer
    that nothing zeroes), grads, loss and probs prefilled 0x00 and 0xFF, two consecutive steps each on
    the same inputs: loss, grads and probs of the four runs are bitwise equal (and equal the executor's
    own freshly allocated run), finite, and the guards of all four buffers are intact."""
    ex, params, rng, prepare = EXECUTORS[name](rt)
    c = ex.cfg
    imgs = torch.from_numpy(rng.integers(0, 256, (c.N, c.H, c.W, 3), dtype=np.uint8)).cuda()
    tgt = _dev(np.eye(10, dtype=np.float32)[rng.integers(0, 10, c.N)])

    def step():
        if ex.inference:
            ex.forward(params, imgs)
            return {"probs": ex.probs.clone()}
        ex.forward_backward(params, imgs, tgt, want_probs=True)
        return {"loss": ex.loss.clone(), "grads": ex.grads.clone(), "probs": ex.probs.clone()}

    want = step()
    torch.cuda.synchronize()
    inputs = Bufs(0xFF)  # params, images and targets between NaN guards for the carved runs
    params, imgs, tgt = inputs.inp(params, "params"), inputs.inp(imgs, "images"), inputs.inp(tgt, "targets")
    runs = []
    for fill in PREFILLS:
        B = Bufs(fill)
        ex.ws = B.out((ex.ws_bytes,), torch.uint8, "workspace")
        _call(prepare, ct.byref(ex.cfg), _p(ex.ws), ex.ws_bytes)
        if not ex.inference:
            ex.grads = B.out((ex.n_params,), torch.float32, "grads")
        ex.loss = B.out((1,), torch.float32, "loss")
        ex.probs = B.out((c.N, 10), torch.float32, "probs")
        for _ in range(2):  # the second step reuses the first's workspace
            runs.append(step())
            B.check()
            inputs.check()
    for i in range(0, 4, 2):
        for k in runs[i]:
            assert _same(runs[i][k], runs[i + 1][k]), f"{k}: the second step on the same workspace differs"
    _check_outputs([runs[0], runs[2]], want)
    if not ex.inference:
        assert float(runs[0]["grads"].abs().max()) > 0
