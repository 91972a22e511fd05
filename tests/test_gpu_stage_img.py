"""GPU parity of the image-resident stage kernels, layer by layer, through the
block-stack ABI (asr_block_stack_forward / _backward): k_stagef / k_stageb
(bf16 at 16x16x32, 8x8x64, 8x8x32), k_stagef32 / k_stageb32 (fp32 at 16x16x32,
8x8x64) and the all-layers weight gradients of wgrad_layers (asr_stage_img.hip;
k_wgradb of asr_conv_bf16.hip / k_wgrad32 of asr_conv_f32.hip).  The stages executor runs the same kernels
(test_gpu_stages.py checks them only through whole networks).

Every layer is compared with the fp64 oracle's Euler step
(models/tfkeras_resnets.py:69-92) fed the GPU's own input of that layer, at
the per-block kernels' bounds (test_gpu_kernels.py), and with the per-block
kernels themselves (asr_conv_forward / asr_conv_backward: k_convb / k_conv32)
on the same operands.

Conventions read off the kernels and implemented by the oracle side here:
  forward   y = x + h relu(conv(x, W) + b), relu bit = [conv + b > 0] on the
            fp32 accumulator, bit index pixel*C + channel;
  k_stageb  dz = dy & mask (dy's bf16 value or 0: exact, h not yet applied);
            dx = dy - h conv(dz, W) + (2 gamma h) dz in fp32, one bf16
            rounding, W the forward's pack (A^T = -A + 2 gamma I);
  k_stageb32 dz = h dy [bit] in fp32; dx = dy - conv(dz, W) + 2 gamma dz
            (the same value in exact arithmetic);
  k_wgradb / k_wgrad32  dW = h sum_px x[px + tap] (x) (dy & mask), db = h sum dz,
            one [dW | db] slab per workgroup in a fixed order, the slabs summed
            in a fixed order (no atomics): a repeated call gives the same bits.

Measured on an MI355X (worst error as a fraction of its bound, forward y / dx):
bf16 16x16x32 0.46 / 0.36, 8x8x64 0.44 / 0.38, 8x8x32 0.35 / 0.38; fp32 16x16x32
0.009 / 0.005, 8x8x64 0.012 / 0.007; dtheta and dbias below 0.03 of theirs.  The
fused results equal the per-block kernels' bit for bit (y, masks, dx0, dparams).
"""
import numpy as np
import pytest

from helpers import GUARD, assert_close, carve, decode_mask, guards_intact, rel_l2, w_bf16_balanced
from oracle import asr_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H_STEP = 0.25
SHAPES = [("bf16", 16, 32), ("bf16", 8, 64), ("bf16", 8, 32), ("f32", 16, 32), ("f32", 8, 64)]
SHAPE_IDS = [f"{d}-{hw}x{hw}x{c}" for d, hw, c in SHAPES]


@pytest.fixture(scope="module")
def rt():
    from differential_equations_resnet_amd import runtime
    runtime.require_gpu()
    return runtime


class Case:
    """One stack's operands on the GPU and what the oracle needs of them."""

    def __init__(self, rt, dtype, HW, C, N, L, gamma, seed):
        self.bf = dtype == "bf16"
        self.dt = rt.ASR_BF16 if self.bf else rt.ASR_F32
        self.N, self.HW, self.C, self.L, self.gamma = N, HW, C, L, gamma
        rng = np.random.default_rng(seed)
        dev = torch.device("cuda")
        self.pm = rt.param_map(C)
        th = np.concatenate([O.flatten(O.init_theta_3by3(C, rng, np.float64)) for _ in range(L)]).astype(np.float32)
        self.th = th.reshape(L, -1)
        self.w = rt.theta_to_w(torch.from_numpy(th).to(dev), C, self.pm, gamma, self.dt, layers=L)
        self.b = (rng.standard_normal((L, C)) * 0.1).astype(np.float32)
        self.bias = torch.from_numpy(self.b).to(dev)
        tdt = rt.torch_dtype(self.dt)
        self.x0 = torch.from_numpy(rng.standard_normal((N, HW, HW, C)).astype(np.float32)).to(dev).to(tdt)
        self.dyL = torch.from_numpy((rng.standard_normal((N, HW, HW, C)) * 0.1).astype(np.float32)).to(dev).to(tdt)
        self.src, self.sign = O.param_map(C)
        self._W = {}

    def W(self, l):
        """The oracle's operator of layer l: the fp32 theta assembled in fp64; bf16: the pack's
        balanced rounding (helpers.w_bf16_balanced, bit-exact)."""
        if l not in self._W:
            Wl = O.assemble_from_map(self.th[l].astype(np.float64), self.C, self.src, self.sign, self.gamma)
            if self.bf:
                Wl = w_bf16_balanced(Wl, self.src, self.sign).astype(np.float64)
            self._W[l] = Wl
        return self._W[l]

    def x_in(self, ys, l):
        return self.x0 if l == 0 else ys[l - 1]

    def tol(self):
        """(rtol, atol / max|want|, relu-bit margin / max|z|, dtheta tol): the per-block bounds."""
        return (2 ** -8, 4e-3, 2e-2, 1e-3) if self.bf else (1e-5, 2e-5, 1e-4, 2e-5)


def _np64(t):
    return t.float().cpu().numpy().astype(np.float64)


def _frac_of_bound(got, want, rtol, atol):
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())


def _ulps(a, b):
    """Largest distance between two tensors in units in the last place of their dtype
    (bf16: 16-bit patterns, fp32: 32-bit), on the sign-magnitude number line."""
    it = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    mag = 0x7FFF if a.dtype == torch.bfloat16 else 0x7FFFFFFF

    def line(t):
        i = t.contiguous().view(it).to(torch.int64)
        return torch.where(i < 0, -(i & mag), i)

    return int((line(a) - line(b)).abs().max().item())


def _check_forward(rt, c, ys, masks, images=None):
    """Every layer against the oracle (on `images`, default all) and against the per-block call.
    Returns (worst error / bound, worst per-block difference in ulps, differing mask bytes)."""
    N, HW, C = c.N, c.HW, c.C
    rtol, atol_s, margin, _ = c.tol()
    sel = np.arange(N) if images is None else np.asarray(images)
    worst, ulps, mdiff = 0.0, 0, 0
    for l in range(c.L):
        xin = c.x_in(ys, l).contiguous()
        m = torch.zeros(rt.mask_bytes(N, HW, HW, C), dtype=torch.uint8, device=xin.device)
        y = rt.conv_forward(rt.ASR_MODE_EULER, xin, c.w[l:l + 1], c.bias[l].contiguous(), H_STEP, m)
        xo = _np64(xin)[sel]
        z = O.conv2d_same(xo, c.W(l)) + c.b[l].astype(np.float64)
        want = xo + H_STEP * np.maximum(z, 0)
        atol = atol_s * np.abs(want).max()
        got = _np64(ys[l])[sel]
        worst = max(worst, _frac_of_bound(got, want, rtol, atol))
        assert_close(got, want, rtol=rtol, atol=atol, what=f"layer {l}")
        mk = decode_mask(masks[l].cpu().numpy(), N, HW, HW, C)[sel]
        sure = np.abs(z) > margin * np.abs(z).max()
        assert np.array_equal(mk[sure], (z > 0)[sure]), f"layer {l}: relu mask"
        # the per-block kernel on the same input: both sides meet the oracle bound
        ulps = max(ulps, _ulps(y, ys[l]))
        mdiff += int((m != masks[l]).sum().item())
        yo = _np64(y)[sel]
        assert np.all(np.abs(yo - got) <= 2 * (atol + rtol * np.abs(want))), f"layer {l}: stack vs per-block"
        mp = decode_mask(m.cpu().numpy(), N, HW, HW, C)[sel]
        assert np.array_equal(mp[sure], mk[sure]), f"layer {l}: stack vs per-block relu mask"
    print(f"\nSTAT fwd {'bf16' if c.bf else 'f32'} {HW}x{HW}x{C} N={N} L={c.L}: err/bound {worst:.3f}, "
          f"per-block ulps {ulps}, mask bytes differing {mdiff}")
    return worst, ulps, mdiff


@pytest.mark.parametrize("N,L,gamma", [(1, 1, 0.0), (5, 2, -0.1), (5, 3, 0.0), (2, 4, 0.0)])
@pytest.mark.parametrize("dtype,HW,C", SHAPES, ids=SHAPE_IDS)
def test_stage_forward_layers_vs_oracle(rt, dtype, HW, C, N, L, gamma):
    """One launch over L layers (N = 1 and odd N; L = 1 .. 4: both parities of the LDS ping-pong and
    its wrap) against the oracle per layer: bf16 2^-8 relative + 4e-3 max|want|, relu bits equal where
    |z| > 2e-2 max|z|; fp32 1e-5 relative + 2e-5 max|want|, bits equal where |z| > 1e-4 max|z|.
    Against the per-block kernels (k_convb / k_conv32 through asr_conv_forward) on the same input:
    y and the mask bit-identical (measured at all five shapes: the same MFMA chain per output tile
    and the same epilogue arithmetic)."""
    c = Case(rt, dtype, HW, C, N, L, gamma, seed=1000 * HW + 10 * N + L)
    ys, masks = rt.block_stack_forward(c.x0, c.w, c.bias, H_STEP)
    assert tuple(ys.shape) == (L, N, HW, HW, C) and ys.dtype == c.x0.dtype
    worst, ulps, mdiff = _check_forward(rt, c, ys, masks)
    assert ulps == 0 and mdiff == 0, (ulps, mdiff)


@pytest.mark.parametrize("HW,C", [(8, 64), (8, 32)])
def test_stage_forward_many_images(rt, HW, C):
    """More workgroups than compute units (a workgroup per image): N = 300, L = 2, every image against
    the per-block kernels and the first, a middle and the last image against the oracle."""
    N, L = 300, 2
    c = Case(rt, "bf16", HW, C, N, L, 0.0, seed=HW + C)
    ys, masks = rt.block_stack_forward(c.x0, c.w, c.bias, H_STEP)
    worst, ulps, mdiff = _check_forward(rt, c, ys, masks, images=[0, 150, 299])
    assert ulps == 0 and mdiff == 0, (ulps, mdiff)


@pytest.mark.parametrize("N,L,gamma", [(1, 1, 0.0), (5, 3, -0.1), (3, 4, 0.0)])
@pytest.mark.parametrize("dtype,HW,C", SHAPES, ids=SHAPE_IDS)
def test_stage_backward_layers_vs_oracle(rt, dtype, HW, C, N, L, gamma):
    """The fused backward, layer by layer.  The gradient entering layer l - 1 is the dx0 of the
    sub-stack of layers l .. L-1 (the kernel takes each image top-down, so the same arithmetic); its
    dparams rows equal the full call's rows l .. L-1 exactly (fixed-order slabs and sums, no atomics).
    Per layer, with the GPU's mask, dy and x_l (conventions in the module docstring: dz = dy & mask,
    dx = dy - h conv(dz, W) + 2 gamma h dz, dW = h backprop_filter(x_l, dz), db = h sum dz, dtheta =
    project_dW): dx bf16 2^-8 relative + 4e-3 max, fp32 1e-5 relative + 2e-5 max; dtheta within 1e-3
    (bf16) / 2e-5 (fp32) of max|want|; db within 2e-5 max(max|want|, 1).  The full call's dx0 and
    dparams against the chain of per-block asr_conv_backward calls (k_convb / k_conv32 and the same
    weight-gradient kernels, one layer per launch): bit-identical, measured at all five shapes."""
    c = Case(rt, dtype, HW, C, N, L, gamma, seed=2000 * HW + 10 * N + L)
    rtol, atol_s, _, ttol = c.tol()
    pm, nt = c.pm, c.pm.n_theta
    ys, masks = rt.block_stack_forward(c.x0, c.w, c.bias, H_STEP)
    dx0, dp = rt.block_stack_backward(c.dyL, c.x0, ys, masks, c.w, pm, H_STEP, gamma)
    assert tuple(dp.shape) == (L, nt + C)
    # the gradient entering every layer, from the GPU itself
    dys = [None] * L
    dys[L - 1] = c.dyL
    for l in range(1, L):
        dys[l - 1], dpl = rt.block_stack_backward(c.dyL, ys[l - 1].contiguous(), ys[l:], masks[l:], c.w[l:], pm,
                                                  H_STEP, gamma)
        assert torch.equal(dpl, dp[l:]), f"sub-stack {l}..{L - 1}: dparams rows differ from the full call's"
    w_dx = w_th = w_db = 0.0
    for l in range(L):
        xo = _np64(c.x_in(ys, l))
        mk = decode_mask(masks[l].cpu().numpy(), N, HW, HW, C)
        dy = _np64(dys[l])
        dz = dy * mk
        dx_want = dy - H_STEP * O.conv2d_same(dz, c.W(l)) + 2.0 * gamma * H_STEP * dz
        dW_want = H_STEP * O.conv2d_backprop_filter(xo, dz)
        db_want = H_STEP * dz.sum(axis=(0, 1, 2))
        dth_want = O.project_dW(dW_want, c.src, c.sign, nt)
        dx_got = _np64(dx0 if l == 0 else dys[l - 1])
        atol = atol_s * np.abs(dx_want).max()
        w_dx = max(w_dx, _frac_of_bound(dx_got, dx_want, rtol, atol))
        dth_got, db_got = dp[l, :nt].cpu().numpy(), dp[l, nt:].cpu().numpy()
        w_th = max(w_th, np.abs(dth_got - dth_want).max() / (ttol * np.abs(dth_want).max()))
        w_db = max(w_db, np.abs(db_got - db_want).max() / (2e-5 * max(np.abs(db_want).max(), 1)))
        assert_close(dx_got, dx_want, rtol=rtol, atol=atol, what=f"layer {l} dx")
        assert_close(dth_got, dth_want, rtol=0, atol=ttol * np.abs(dth_want).max(), what=f"layer {l} dtheta")
        assert_close(db_got, db_want, rtol=0, atol=2e-5 * max(np.abs(db_want).max(), 1), what=f"layer {l} dbias")
    # the chain of per-block backward calls
    dy = c.dyL
    same_dp = True
    for l in range(L - 1, -1, -1):
        dy, dth, db, _ = rt.conv_backward(rt.ASR_MODE_EULER, dy, c.x_in(ys, l).contiguous(), masks[l], c.w[l:l + 1], pm,
                                          H_STEP, gamma)
        same_dp = same_dp and torch.equal(dth, dp[l, :nt]) and torch.equal(db, dp[l, nt:])
    a, b = _np64(dx0), _np64(dy)
    r2, mx, ul = rel_l2(a, b), float(np.abs(a - b).max() / np.abs(b).max()), _ulps(dx0, dy)
    print(f"\nSTAT bwd {dtype} {HW}x{HW}x{C} N={N} L={L}: dx err/bound {w_dx:.3f}, dtheta {w_th:.3f}, db {w_db:.3f}; "
          f"dx0 vs per-block chain: rel-L2 {r2:.2e}, max {mx:.2e}, ulps {ul}, dparams identical {same_dp}")
    assert torch.equal(dx0, dy) and same_dp, (r2, mx, ul, same_dp)


def _carve(shape, dtype, dev):
    """A tensor of `shape` in the middle of a larger buffer filled with 0xA5 bytes: (buffer, view)."""
    return carve(shape, dtype, dev, 0xA5, 0xA5)


def _guards_intact(buf, what):
    guards_intact(buf, buf.numel() - 2 * GUARD, what, 0xA5)


@pytest.mark.parametrize("dtype,HW,C", [("bf16", 8, 32), ("f32", 16, 32)])
def test_stage_kernels_stay_inside_their_buffers(rt, dtype, HW, C):
    """ys (8-B / 16-B stores), masks (2-B stores), dx0 (16-B stores), dparams and the workspace (the
    gradients entering each layer, slabs, group rows), each carved out of a larger buffer of 0xA5
    bytes with exactly its documented size: no byte outside is touched and every byte inside is
    written (equal to the run on wrapper-allocated buffers, whose kernels are deterministic)."""
    from differential_equations_resnet_amd import _lib
    from differential_equations_resnet_amd.runtime import _p, _stream
    N, L, gamma = 3, 3, -0.1
    c = Case(rt, dtype, HW, C, N, L, gamma, seed=77)
    dev, pm = c.x0.device, c.pm
    P, mb, per = N * HW * HW * C, rt.mask_bytes(N, HW, HW, C), c.w[0].numel()
    assert mb * 8 == P  # no padding bytes in a layer's mask: every byte has a writer
    ys_want, masks_want = rt.block_stack_forward(c.x0, c.w, c.bias, H_STEP)
    dx0_want, dp_want = rt.block_stack_backward(c.dyL, c.x0, ys_want, masks_want, c.w, pm, H_STEP, gamma)
    ys_buf, ys = _carve((L, N, HW, HW, C), c.x0.dtype, dev)
    mk_buf, masks = _carve((L, mb), torch.uint8, dev)
    _lib.call("asr_block_stack_forward", _p(c.x0), _p(ys), P, _p(masks), mb, _p(c.w), per, _p(c.bias), C,
              float(H_STEP), N, HW, HW, C, L, c.dt, 1, _stream())
    torch.cuda.synchronize()
    _guards_intact(ys_buf, "ys")
    _guards_intact(mk_buf, "masks")
    assert torch.equal(ys, ys_want) and torch.equal(masks, masks_want)
    xs = torch.cat([c.x0.unsqueeze(0), ys_want[:L - 1]]).contiguous()
    wsb = int(_lib.load().asr_block_stack_backward_workspace_bytes(N, HW, HW, C, L, c.dt))
    dx_buf, dx0 = _carve((N, HW, HW, C), c.x0.dtype, dev)
    dp_buf, dp = _carve((L, pm.n_theta + C), torch.float32, dev)
    ws_buf, ws = _carve((wsb,), torch.uint8, dev)
    _, theta_dst = pm.device(dev)
    _lib.call("asr_block_stack_backward", _p(c.dyL), _p(xs), P, _p(masks_want), mb, _p(c.w), per, _p(theta_dst),
              pm.n_theta, float(H_STEP), float(gamma), N, HW, HW, C, L, c.dt, _p(dx0), _p(dp), _p(ws), wsb, _stream())
    torch.cuda.synchronize()
    _guards_intact(dx_buf, "dx0")
    _guards_intact(dp_buf, "dparams")
    _guards_intact(ws_buf, "workspace")
    assert torch.equal(dx0, dx0_want) and torch.equal(dp, dp_want)


def _per_block_forward(rt, c, bias, with_masks):
    N, HW, C = c.N, c.HW, c.C
    x, ys, ms = c.x0, [], []
    for l in range(c.L):
        m = torch.zeros(rt.mask_bytes(N, HW, HW, C), dtype=torch.uint8, device=x.device) if with_masks else None
        x = rt.conv_forward(rt.ASR_MODE_EULER, x, c.w[l:l + 1], bias[l].contiguous() if bias is not None else None,
                            H_STEP, m)
        ys.append(x)
        ms.append(m)
    return ys, ms


@pytest.mark.parametrize("dtype,HW,C", [("bf16", 8, 32), ("f32", 8, 64)])
def test_stack_abi_fallbacks(rt, dtype, HW, C):
    """At a fused shape, a call without bias or without masks (the stage kernels read / write both
    unconditionally) runs the per-block sequence: the results of the asr_conv_forward calls, bitwise."""
    c = Case(rt, dtype, HW, C, 3, 3, 0.0, seed=5)
    ys, masks = rt.block_stack_forward(c.x0, c.w, None, H_STEP)
    want, wm = _per_block_forward(rt, c, None, True)
    for l in range(c.L):
        assert torch.equal(ys[l], want[l]) and torch.equal(masks[l], wm[l]), f"bias=None, layer {l}"
    ys, none = rt.block_stack_forward(c.x0, c.w, c.bias, H_STEP, want_masks=False)
    assert none is None
    want, _ = _per_block_forward(rt, c, c.bias, False)
    for l in range(c.L):
        assert torch.equal(ys[l], want[l]), f"want_masks=False, layer {l}"


def test_stack_abi_runs_other_bf16_widths_per_block(rt):
    """bf16 16 x 16 x 64 is not image-resident (and W != 32): the stack ABI runs the any-width
    per-block kernels in sequence, forward and backward, with the single calls' results bitwise."""
    c = Case(rt, "bf16", 16, 64, 2, 2, 0.0, seed=9)
    ys, masks = rt.block_stack_forward(c.x0, c.w, c.bias, H_STEP)
    want, wm = _per_block_forward(rt, c, c.bias, True)
    for l in range(c.L):
        assert torch.equal(ys[l], want[l]) and torch.equal(masks[l], wm[l]), f"layer {l}"
    dx0, dp = rt.block_stack_backward(c.dyL, c.x0, ys, masks, c.w, c.pm, H_STEP, 0.0)
    dy, nt = c.dyL, c.pm.n_theta
    for l in range(c.L - 1, -1, -1):
        dy, dth, db, _ = rt.conv_backward(rt.ASR_MODE_EULER, dy, c.x_in(ys, l).contiguous(), masks[l], c.w[l:l + 1],
                                          c.pm, H_STEP, 0.0)
        assert torch.equal(dth, dp[l, :nt]) and torch.equal(db, dp[l, nt:]), f"layer {l} dparams"
    assert torch.equal(dy, dx0)
