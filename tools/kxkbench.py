"""Forward + backward time of one Conv2DAntisymmetric(kernel_size = k) Euler block, fp32 `_k` path
(VALU kernels) against the bf16 path (matrix cores, asr_conv_kxk.hip), at one shape.

Both paths run in this process, alternating round by round after a warm-up; each round is timed
with device events over `--reps` forward+backward calls (weights already materialised: the layer's
conv kernels and weight-gradient reduction only).  Prints one JSON line: the median and spread of
each path's time per forward+backward, their ratio, and the bf16 path's rate against the bf16 MFMA
peak from 3 * 2 * k^2 * C^2 * N * H * W FLOP (forward, data gradient, weight gradient).  Needs a
GPU: without one it fails.

  python tools/kxkbench.py                 # k = 5, C = 64, N = 64, 32 x 32
  python tools/kxkbench.py --k 7
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from differential_equations_resnet_amd import runtime as rt  # noqa: E402

BF16_MFMA_PEAK = 2.5e15  # dense bf16 FLOP/s of an MI355X


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--C", type=int, default=64)
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--H", type=int, default=32)
    ap.add_argument("--W", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10, help="forward+backward calls per timed round")
    ap.add_argument("--rounds", type=int, default=7, help="timed rounds per path (alternating)")
    ap.add_argument("--warmup", type=int, default=3, help="untimed forward+backward calls per path")
    a = ap.parse_args()
    dev = rt.require_gpu()  # raises without a GPU
    k, C, N, H, W = a.k, a.C, a.N, a.H, a.W
    h, gamma = 0.25, 0.0
    pm = rt.param_map(C, rt.ASR_PARAM_GENERAL, True, k)
    g = torch.Generator(device=dev).manual_seed(11)
    theta = torch.randn(pm.n_theta, device=dev, generator=g) * 0.05
    bias = torch.randn(C, device=dev, generator=g) * 0.1
    # bf16-representable inputs, so both paths see the same x and dy (W and the relu mask still differ)
    x32 = torch.randn(N, H, W, C, device=dev, generator=g).to(torch.bfloat16).float()
    dy32 = torch.randn(N, H, W, C, device=dev, generator=g).to(torch.bfloat16).float()

    def make(dtype):
        code = rt.dtype_code(dtype)
        x, dy = x32.to(dtype).contiguous(), dy32.to(dtype).contiguous()
        w = rt.theta_to_w(theta, C, pm, gamma, code)
        mask = torch.zeros(rt.mask_bytes(N, H, W, C), dtype=torch.uint8, device=dev)

        def step():
            rt.conv_forward(rt.ASR_MODE_EULER, x, w, bias, h, mask, k=k)
            return rt.conv_backward(rt.ASR_MODE_EULER, dy, x, mask, w, pm, h, gamma)
        return step

    paths = {"f32": make(torch.float32), "bf16": make(torch.bfloat16)}
    outs = {}
    for name, step in paths.items():
        for _ in range(a.warmup):
            outs[name] = step()
    torch.cuda.synchronize()
    # a coarse agreement figure only (the bf16 W moves relu bits, and a moved bit drops a whole term:
    # percents here are expected; parity is tests/test_gpu_kxk_bf16.py's job)
    dth32, dthb = outs["f32"][1], outs["bf16"][1]
    rel = float((dth32 - dthb).norm() / dth32.norm())
    times = {name: [] for name in paths}
    for _ in range(a.rounds):
        for name, step in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                step()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.reps)
    flop = 3 * 2 * k * k * C * C * N * H * W
    med = {n: statistics.median(t) for n, t in times.items()}
    print(json.dumps({
        "tool": "kxkbench", "k": k, "N": N, "H": H, "W": W, "C": C, "reps": a.reps, "rounds": a.rounds,
        "f32_ms": round(med["f32"], 4), "f32_ms_min_max": [round(min(times["f32"]), 4), round(max(times["f32"]), 4)],
        "bf16_ms": round(med["bf16"], 4),
        "bf16_ms_min_max": [round(min(times["bf16"]), 4), round(max(times["bf16"]), 4)],
        "speedup_bf16_over_f32": round(med["f32"] / med["bf16"], 2),
        "flop_fwd_bwd": flop, "bf16_tflops": round(flop / (med["bf16"] * 1e-3) / 1e12, 2),
        "bf16_share_of_mfma_peak": round(flop / (med["bf16"] * 1e-3) / BF16_MFMA_PEAK, 4),
        "dtheta_rel_l2_bf16_vs_f32": round(rel, 5),
    }))


if __name__ == "__main__":
    main()
