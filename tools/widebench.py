"""Training-step time of a single-stage 3 x 3 network at an image width off 32 (asr_net_*: bfloat16 on
k_convb / k_wgradb over column strips from W = 48 on, float32 on the generic fp32 kernels).

Each round is timed with device events over --reps steps (forward_backward + Adam) after --warmup untimed
steps; prints the median and spread of a step as one JSON line.  --lib loads another build of libasr.so (a
build of the parent commit, to time its float32 fallback in the same call).  Kernel times come from a
rocprofv3 --kernel-trace --stats run of this tool (a run of its own: tracing slows the host).  Needs a GPU:
without one it fails.

  python tools/widebench.py                                   # bf16, N = 128, 64 x 64, C = 64, L = 8
  python tools/widebench.py --dtype float32 --lib /path/to/parent/libasr.so
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from differential_equations_resnet_amd import _lib  # noqa: E402


def he_params(n_params, C, L, n_theta, num_classes, seed):
    """Flat parameters in the executor's order: he-normal kernels, biases 0.05 N(0, 1)."""
    rng = np.random.default_rng(seed)
    parts = [rng.standard_normal(27 * C) * np.sqrt(2.0 / 27), rng.standard_normal(C) * 0.05]
    for _ in range(L):
        parts += [rng.standard_normal(n_theta) * np.sqrt(2.0 / (9 * C)), rng.standard_normal(C) * 0.05]
    parts += [rng.standard_normal(C * num_classes) * np.sqrt(2.0 / C), np.zeros(num_classes)]
    flat = np.concatenate(parts).astype(np.float32)
    assert flat.size == n_params, (flat.size, n_params)
    return flat


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dtype", choices=["bfloat16", "float32"], default="bfloat16")
    ap.add_argument("--lib", default=None, help="another build of libasr.so to load (default: this tree's)")
    ap.add_argument("--C", type=int, default=64)
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--H", type=int, default=64)
    ap.add_argument("--W", type=int, default=64)
    ap.add_argument("--L", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5, help="steps per timed round")
    ap.add_argument("--rounds", type=int, default=7, help="timed rounds")
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps")
    a = ap.parse_args()
    _lib.load(path=os.path.abspath(a.lib) if a.lib else None)  # (before the runtime's first load)
    from differential_equations_resnet_amd import runtime as rt
    dev = rt.require_gpu()  # raises without a GPU
    ex = rt.NetExecutor(a.N, a.H, a.W, 3, a.C, a.L, 10, 0.25, -0.05, subtract_mean=127.5, divide_by_stddev=127.5,
                        dtype=a.dtype, input_u8=True, device=dev)
    n_theta = rt.theta_count(a.C, rt.ASR_PARAM_3BY3, True, 3)
    params = torch.from_numpy(he_params(ex.n_params, a.C, a.L, n_theta, 10, 5)).to(dev)
    rng = np.random.default_rng(6)
    imgs = torch.from_numpy(rng.integers(0, 256, (a.N, a.H, a.W, 3), dtype=np.uint8)).to(dev)
    tgt = torch.from_numpy(np.eye(10, dtype=np.float32)[rng.integers(0, 10, a.N)]).to(dev)
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    step_no = [0]

    def step():
        _, g = ex.forward_backward(params, imgs, tgt)
        step_no[0] += 1
        rt.adam_update(params, g, m, v, 1e-4, 0.9, 0.999, 1e-7, step_no[0])
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t = [timed(step, a.reps) for _ in range(a.rounds)]
    ex.check_status()
    med = statistics.median(t)
    print(json.dumps({"tool": "widebench", "lib": a.lib or "this tree", "N": a.N, "H": a.H, "W": a.W, "C": a.C,
                      "L": a.L, "dtype": a.dtype, "reps": a.reps, "rounds": a.rounds, "step_ms": round(med, 4),
                      "step_ms_min_max": [round(min(t), 4), round(max(t), 4)],
                      "images_per_s": round(a.N / (med * 1e-3), 1), "loss": round(float(ex.loss.item()), 5)}))


if __name__ == "__main__":
    main()
