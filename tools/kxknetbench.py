"""Training-step time of a network with a k x k conv1 and k x k blocks (asr_net_config.kernel_size /
conv1_kernel_size) in bfloat16, and the k x k stem's matrix-core kernels against the generic arm.

  --mode stem-ab (default)  one executor, its two stem arms alternating round by round after a warm-up: the
      matrix-core stem (k_stem_fwd_kxk, k_stem_wgrad_kxk) against ASR_VARIANT_STEM_FWD_VALU |
      ASR_VARIANT_STEM_WGRAD_VALU (k_normalize + the generic fp32 k x k conv, make_dz + the generic fp32 weight
      gradient).  Each round is timed with device events over --reps forward_backward calls.  Prints the median
      and spread of a step with each arm and their difference.
  --mode step               images/s of the whole step (forward_backward + Adam) of one network.

One JSON line per run.  Kernel times come from a rocprofv3 --kernel-trace --stats run of this tool (a run of
its own: tracing slows the host).  Needs a GPU: without one it fails.

  python tools/kxknetbench.py --k 7                          # stem A/B at N = 512, 32 x 32, C = 64, L = 2
  python tools/kxknetbench.py --mode step --k 5 --N 64 --L 30
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from differential_equations_resnet_amd import runtime as rt  # noqa: E402


def he_params(n_params, k1, kb, C, L, n_theta, num_classes, seed):
    """Flat parameters in the executor's order: he-normal kernels, biases 0.05 N(0, 1)."""
    rng = np.random.default_rng(seed)
    parts = [rng.standard_normal(k1 * k1 * 3 * C) * np.sqrt(2.0 / (k1 * k1 * 3)), rng.standard_normal(C) * 0.05]
    for _ in range(L):
        parts += [rng.standard_normal(n_theta) * np.sqrt(2.0 / (kb * kb * C)), rng.standard_normal(C) * 0.05]
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
    ap.add_argument("--mode", choices=["stem-ab", "step"], default="stem-ab")
    ap.add_argument("--k", type=int, default=5, help="conv1's and the blocks' kernel size")
    ap.add_argument("--kb", type=int, default=None, help="the blocks' kernel size where it differs")
    ap.add_argument("--C", type=int, default=64)
    ap.add_argument("--N", type=int, default=512)
    ap.add_argument("--H", type=int, default=32)
    ap.add_argument("--W", type=int, default=32)
    ap.add_argument("--L", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5, help="steps per timed round")
    ap.add_argument("--rounds", type=int, default=7, help="timed rounds (per arm, alternating)")
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps (per arm)")
    a = ap.parse_args()
    dev = rt.require_gpu()  # raises without a GPU
    k1, kb = a.k, a.k if a.kb is None else a.kb
    kind = rt.ASR_PARAM_3BY3 if kb == 3 else rt.ASR_PARAM_GENERAL
    ex = rt.NetExecutor(a.N, a.H, a.W, 3, a.C, a.L, 10, 0.25, -0.05, subtract_mean=127.5, divide_by_stddev=127.5,
                        dtype="bfloat16", input_u8=True, device=dev, param_kind=kind, kernel_size=kb,
                        conv1_kernel_size=k1)
    n_theta = rt.theta_count(a.C, kind, True, kb)
    params = torch.from_numpy(he_params(ex.n_params, k1, kb, a.C, a.L, n_theta, 10, 5)).to(dev)
    rng = np.random.default_rng(6)
    imgs = torch.from_numpy(rng.integers(0, 256, (a.N, a.H, a.W, 3), dtype=np.uint8)).to(dev)
    tgt = torch.from_numpy(np.eye(10, dtype=np.float32)[rng.integers(0, 10, a.N)]).to(dev)
    base = {"tool": "kxknetbench", "mode": a.mode, "k1": k1, "kb": kb, "N": a.N, "H": a.H, "W": a.W, "C": a.C,
            "L": a.L, "dtype": "bfloat16", "reps": a.reps, "rounds": a.rounds}
    if a.mode == "step":
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
        print(json.dumps(dict(base, step_ms=round(med, 4), step_ms_min_max=[round(min(t), 4), round(max(t), 4)],
                              images_per_s=round(a.N / (med * 1e-3), 1), loss=round(float(ex.loss.item()), 5))))
        return
    arms = {"mfma": 0, "generic": rt.ASR_VARIANT_STEM_FWD_VALU | rt.ASR_VARIANT_STEM_WGRAD_VALU}
    loss = {}

    def step():
        ex.forward_backward(params, imgs, tgt)
    for name, bits in arms.items():
        ex.variant = bits
        for _ in range(a.warmup):
            step()
        loss[name] = float(ex.loss.item())
    times = {name: [] for name in arms}
    for _ in range(a.rounds):
        for name, bits in arms.items():
            ex.variant = bits
            times[name].append(timed(step, a.reps))
    ex.variant = 0
    ex.check_status()
    med = {n: statistics.median(t) for n, t in times.items()}
    print(json.dumps(dict(
        base, mfma_step_ms=round(med["mfma"], 4),
        mfma_step_ms_min_max=[round(min(times["mfma"]), 4), round(max(times["mfma"]), 4)],
        generic_step_ms=round(med["generic"], 4),
        generic_step_ms_min_max=[round(min(times["generic"]), 4), round(max(times["generic"]), 4)],
        generic_minus_mfma_us=round((med["generic"] - med["mfma"]) * 1e3, 1),
        loss_mfma=round(loss["mfma"], 5), loss_generic=round(loss["generic"], 5))))


if __name__ == "__main__":
    main()
