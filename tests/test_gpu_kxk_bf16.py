"""GPU parity of the bf16 k x k kernels (asr_conv_kxk.hip: Conv2DAntisymmetric(kernel_size = 5 / 7)
in bf16 with fp32 accumulation) against the numpy oracle, through runtime.* and the eager layer.

Inputs (seeded): theta = 0.2 N(0,1); x, dy = N(0,1) rounded to bf16; bias = 0.1 N(0,1);
h in {0.25, 1.0} (powers of two: the order of applying h is exact).  The oracle is fed the same
bf16 x / dy and the nearest-rounded bf16 W (the pack's rounding), so

  outputs (bf16)   : |gpu - oracle| <= 2^-8 |oracle| + 4e-3 max|oracle| (tests/test_gpu_kernels.py's
                     bf16 bar: the output is rounded once; fp32 accumulation error at reduction
                     length 3136 is orders of magnitude below it, so the bar does not depend on k);
  dW, dtheta (fp32): within 1e-3 max|oracle|;   db: within 2e-5 max(|oracle|, 1);
  relu mask        : exact wherever |z| > 1e-3 max|z|, and that leaves out <= 1 % of the elements.

The cases cover every C and W of the supported set, partial bands, H < k and a halo wider than
the image (k = 7 at W = 8)."""
import numpy as np
import pytest

from helpers import assert_close, bf16_round, decode_mask
from oracle import asr_oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# (k, (N, H, W, C), antisymmetric, gamma)
CASES = [
    (5, (2, 5, 8, 16), True, 0.0),
    (7, (1, 9, 8, 32), True, -0.1),
    (5, (2, 16, 16, 32), False, 0.0),
    (7, (3, 7, 16, 16), True, 0.0),
    (7, (2, 8, 8, 64), True, 0.0),
    (5, (1, 11, 32, 64), True, -0.1),
    (7, (2, 6, 32, 16), False, 0.0),
]
IDS = [f"k{k}-{'x'.join(map(str, s))}-{'anti' if a else 'gen'}-g{g}" for k, s, a, g in CASES]
# (mode, h): both Euler step sizes and the bare conv
MODES = [("euler", 0.25), ("euler", 1.0), ("conv", 1.0)]
MODE_IDS = ["euler-h0.25", "euler-h1", "conv"]


@pytest.fixture(scope="module")
def rt():
    from differential_equations_resnet_amd import runtime
    runtime.require_gpu()
    return runtime


_DATA = {}


def _case(ci):
    """Inputs and the forward oracle of case ci, computed once and never modified."""
    if ci not in _DATA:
        k, shape, anti, gamma = CASES[ci]
        C = shape[3]
        rng = np.random.default_rng(1000 + ci)
        src, sign = O.param_map(C, "general", k, anti)
        n_theta = O.theta_count_general(C, k, anti)
        th = (0.2 * rng.standard_normal(n_theta)).astype(np.float32)
        x = bf16_round(rng.standard_normal(shape).astype(np.float32))
        dy = bf16_round(rng.standard_normal(shape).astype(np.float32))
        b = (0.1 * rng.standard_normal(C)).astype(np.float32)
        W32 = O.assemble_from_map(th.astype(np.float64), C, src, sign, gamma, k=k).astype(np.float32)
        Wq = bf16_round(W32)
        z = O.conv2d_same(x.astype(np.float64), Wq.astype(np.float64)) + b
        d = dict(k=k, shape=shape, anti=anti, gamma=gamma, C=C, src=src, sign=sign, n_theta=n_theta, th=th, x=x,
                 dy=dy, b=b, W32=W32, Wq=Wq, z=z)
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _DATA[ci] = d
    return _DATA[ci]


def _unpack(pack_f32, C, k):
    """The k x k MFMA pack (include/asr.h) back to HWIO [k, k, C, C] float32."""
    KS = (k * k * C + 31) // 32
    o, kappa = np.meshgrid(np.arange(C), np.arange(k * k * C), indexing="ij")
    idx = (((o // 16) * KS + kappa // 32) * 64 + (o % 16) + 16 * ((kappa % 32) // 8)) * 8 + kappa % 8
    return pack_f32[idx].reshape(C, k * k, C).transpose(1, 2, 0).reshape(k, k, C, C), idx


def _pack_f32(w):
    return (w.view(torch.int16).cpu().numpy().ravel().astype(np.uint16).astype(np.uint32) << 16).view(np.float32)


def _dev(a, bf=False):
    t = torch.tensor(a).cuda()  # (a copy: the shared inputs are read-only)
    return t.to(torch.bfloat16).contiguous() if bf else t


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_pack_is_exact(rt, ci):
    d = _case(ci)
    k, C = d["k"], d["C"]
    pm = rt.param_map(C, rt.ASR_PARAM_GENERAL, d["anti"], k)
    th = _dev(d["th"])
    w = rt.theta_to_w(th, C, pm, d["gamma"], rt.ASR_BF16)
    assert w.dtype == torch.bfloat16 and w.numel() == (C // 16) * ((k * k * C + 31) // 32) * 512
    flat = _pack_f32(w)
    got, idx = _unpack(flat, C, k)
    np.testing.assert_array_equal(got.view(np.uint32), d["Wq"].view(np.uint32))
    pad = np.ones(flat.size, bool)
    pad[idx.ravel()] = False
    assert not flat[pad].view(np.uint32).any(), "padding of the pack is not zero"
    # nearest rounding keeps W exactly antisymmetric off the diagonal
    Wt = got.reshape(k * k, C, C)
    mirror = -Wt[::-1].transpose(0, 2, 1)
    if d["anti"]:
        off = ~np.eye(C, dtype=bool)
        assert np.array_equal(Wt[:, off], mirror[:, off])
    else:  # the transposed map's pack is -flip(W)^T of the forward pack, bit for bit
        wb = rt.theta_to_w_transposed(th, C, pm, rt.ASR_BF16)
        gotb, _ = _unpack(_pack_f32(wb), C, k)
        np.testing.assert_array_equal(gotb.reshape(k * k, C, C).view(np.uint32), (mirror + 0.0).view(np.uint32))


def _forward(rt, d, mode, h):
    k, C = d["k"], d["C"]
    N, H, W_, _ = d["shape"]
    pm = rt.param_map(C, rt.ASR_PARAM_GENERAL, d["anti"], k)
    x = _dev(d["x"], True)
    th = _dev(d["th"])
    w = rt.theta_to_w(th, C, pm, d["gamma"], rt.ASR_BF16)
    mask = torch.zeros(rt.mask_bytes(N, H, W_, C), dtype=torch.uint8, device="cuda")
    y = rt.conv_forward(mode, x, w, _dev(d["b"]), h, mask if mode == rt.ASR_MODE_EULER else None, k=k)
    return pm, x, th, w, y, mask


@pytest.mark.parametrize("mode_name,h", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_forward_parity(rt, ci, mode_name, h):
    d = _case(ci)
    N, H, W_, C = d["shape"]
    mode = rt.ASR_MODE_EULER if mode_name == "euler" else rt.ASR_MODE_CONV
    _, _, _, _, y, mask = _forward(rt, d, mode, h)
    z = d["z"]
    want = d["x"].astype(np.float64) + h * np.maximum(z, 0) if mode == rt.ASR_MODE_EULER else z
    got = y.float().cpu().numpy()
    print(f"forward {IDS[ci]} {mode_name} h={h}: max|err| / max|want| = "
          f"{np.abs(got - want).max() / np.abs(want).max():.3e}")
    assert_close(got, want, rtol=2 ** -8, atol=4e-3 * np.abs(want).max(), what="bf16 k x k forward")
    if mode == rt.ASR_MODE_EULER:
        m = decode_mask(mask.cpu().numpy(), N, H, W_, C)
        sure = np.abs(z) > 1e-3 * np.abs(z).max()
        share = 1.0 - sure.mean()
        print(f"  mask: {share:.4%} of the elements within 1e-3 max|z| of zero")
        assert share <= 0.01
        assert np.array_equal(m[sure], (z > 0)[sure]), "relu mask mismatch"


@pytest.mark.parametrize("mode_name,h", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_backward_parity(rt, ci, mode_name, h):
    d = _case(ci)
    N, H, W_, C = d["shape"]
    k, gamma = d["k"], d["gamma"]
    mode = rt.ASR_MODE_EULER if mode_name == "euler" else rt.ASR_MODE_CONV
    pm, x, th, w, _, mask = _forward(rt, d, rt.ASR_MODE_EULER, h)
    if pm.operator_antisymmetric:
        wb, gb = w, gamma  # A^T = -A + 2 gamma I with the forward W
    else:
        wb, gb = rt.theta_to_w_transposed(th, C, pm, rt.ASR_BF16), 0.0
    dy = _dev(d["dy"], True)
    dx, dth, db, dw = rt.conv_backward(mode, dy, x, mask if mode == rt.ASR_MODE_EULER else None, wb, pm, h, gb,
                                       want_dw=True)
    # oracle, fed the GPU's mask (the mask itself is checked in test_forward_parity)
    xo, dyo, Wo = d["x"].astype(np.float64), d["dy"].astype(np.float64), d["Wq"].astype(np.float64)
    if mode == rt.ASR_MODE_EULER:
        dz_f = h * dyo * decode_mask(mask.cpu().numpy(), N, H, W_, C)
    else:
        dz_f = dyo
    dz_q = bf16_round(dz_f).astype(np.float64)
    if pm.operator_antisymmetric:  # A^T dz = -conv(dz, W) + 2 gamma dz (tests/test_gpu_kernels.py's form)
        at_dz = -O.conv2d_same(dz_q, Wo) + 2 * gamma * dz_q
    else:
        at_dz = O.conv2d_backprop_input(dz_q, Wo, xo.shape)
    dx_want = (dyo if mode == rt.ASR_MODE_EULER else 0.0) + at_dz
    dW_want = O.conv2d_backprop_filter(xo, dz_q, k)
    db_want = dz_f.sum(axis=(0, 1, 2))
    dth_want = O.project_dW(dW_want, d["src"], d["sign"], pm.n_theta)
    sc = np.abs(dx_want).max()
    got_dx, got_dw = dx.float().cpu().numpy(), dw.cpu().numpy()
    print(f"backward {IDS[ci]} {mode_name} h={h}: dx {np.abs(got_dx - dx_want).max() / sc:.3e}  "
          f"dW {np.abs(got_dw - dW_want).max() / np.abs(dW_want).max():.3e}  "
          f"dtheta {np.abs(dth.cpu().numpy() - dth_want).max() / np.abs(dth_want).max():.3e}  "
          f"db {np.abs(db.cpu().numpy() - db_want).max() / max(np.abs(db_want).max(), 1):.3e}")
    assert_close(got_dx, dx_want, rtol=2 ** -8, atol=4e-3 * sc, what="bf16 k x k dx")
    assert_close(got_dw, dW_want, rtol=0, atol=1e-3 * np.abs(dW_want).max(), what="dW")
    assert_close(dth.cpu().numpy(), dth_want, rtol=0, atol=1e-3 * np.abs(dth_want).max(), what="dtheta")
    assert_close(db.cpu().numpy(), db_want, rtol=0, atol=2e-5 * max(np.abs(db_want).max(), 1), what="dbias")


@pytest.mark.parametrize("k,shape,anti,gamma", [(5, (2, 9, 16, 32), True, -0.1), (7, (2, 6, 8, 16), False, 0.0)],
                         ids=["k5-anti", "k7-general"])
def test_layer_eager_bf16(rt, k, shape, anti, gamma):
    """Conv2DAntisymmetric(k) called on a bf16 device tensor, forward and backward(), at the bars of
    tests/test_gpu_api.py's eager-layer test."""
    from differential_equations_resnet_amd import graph
    from differential_equations_resnet_amd.graph import Input
    from differential_equations_resnet_amd.layers import Conv2DAntisymmetric
    N, H, W_, C = shape
    layer = Conv2DAntisymmetric(k, gamma=gamma, antisymmetric=anti)
    graph.set_seed(3)
    layer(Input(shape=(H, W_, C)))
    rng = np.random.default_rng(k)
    layer.bias.assign(rng.standard_normal(C) * 0.1)
    x_np = bf16_round(rng.standard_normal(shape).astype(np.float32))
    r_np = bf16_round(rng.standard_normal(shape).astype(np.float32))
    x = torch.from_numpy(x_np).cuda().to(torch.bfloat16).requires_grad_(True)
    y = layer(x)
    assert y.dtype == torch.bfloat16
    y.backward(torch.from_numpy(r_np).cuda().to(torch.bfloat16))
    th, b = layer.device_variables(x.device)
    src = layer.param_map().w_src
    sign, osrc = np.where(src & 1, -1, 1), np.where(src >= 0, src >> 1, -1)
    xo, ro = x_np.astype(np.float64), r_np.astype(np.float64)
    Wo = bf16_round(layer.get_kernel()).astype(np.float64)
    want_y = O.conv2d_same(xo, Wo) + layer.bias.value.astype(np.float64)
    want_dx = O.conv2d_backprop_input(ro, Wo, xo.shape)
    want_dth = O.project_dW(O.conv2d_backprop_filter(xo, ro, k), osrc, sign, layer.theta_flat().size)
    want_db = ro.sum(axis=(0, 1, 2))
    assert_close(y.float().detach().cpu().numpy(), want_y, rtol=2 ** -8, atol=4e-3 * np.abs(want_y).max(), what="y")
    assert_close(x.grad.float().cpu().numpy(), want_dx, rtol=2 ** -8, atol=4e-3 * np.abs(want_dx).max(), what="dx")
    assert_close(th.grad.cpu().numpy(), want_dth, rtol=0, atol=1e-3 * np.abs(want_dth).max(), what="dtheta")
    assert_close(b.grad.cpu().numpy(), want_db, rtol=0, atol=1e-3 * max(np.abs(want_db).max(), 1), what="dbias")


def test_refusals(rt):
    """Outside the supported set bf16 still raises AsrUnsupported: k = 9, C = 12, W = 12."""
    from differential_equations_resnet_amd._lib import AsrUnsupported
    for k, (N, H, W_, C) in ((9, (1, 8, 16, 16)), (5, (1, 8, 16, 12)), (5, (1, 8, 12, 16))):
        pm = rt.param_map(C, rt.ASR_PARAM_GENERAL, True, k)
        th = torch.zeros(pm.n_theta, device="cuda")
        x = torch.zeros(N, H, W_, C, device="cuda", dtype=torch.bfloat16)
        with pytest.raises(AsrUnsupported):
            w = rt.theta_to_w(th, C, pm, 0.0, rt.ASR_BF16)
            rt.conv_forward(rt.ASR_MODE_CONV, x, w, None, 1.0, k=k)
        with pytest.raises(AsrUnsupported):
            w = torch.zeros(1, 4096, device="cuda", dtype=torch.bfloat16)
            rt.conv_backward(rt.ASR_MODE_CONV, x, x, None, w, pm, 1.0, 0.0)
    from differential_equations_resnet_amd.graph import Input
    from differential_equations_resnet_amd.layers import Conv2DAntisymmetric
    layer = Conv2DAntisymmetric(9)
    layer(Input(shape=(8, 16, 16)))
    with pytest.raises(AsrUnsupported):
        layer(torch.zeros(1, 8, 16, 16, device="cuda", dtype=torch.bfloat16))
