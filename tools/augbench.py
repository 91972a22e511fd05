"""Batch production time of the fused augmentation kernel (asr_augment_batch) against the plain
index_select batch ArrayDataset yields without preprocessors, on device events.

Two shapes, each with the reference-style chain [RandomCrop(0.9), Resize, RandomFlipLeftRight,
RandomBrightness, RandomSaturation]:
  cifar   50 000 x 32 x 32 x 3 uint8, batch 512, crop 28 -> 32 x 32
  wide    --wide-n x 256 x 256 x 3 uint8, batch 128, crop 230 -> 224 x 224

The tables and index vectors of --batches different batches are drawn and uploaded before timing, so
a timed launch is the kernel alone.  After --warmup untimed passes the two arms alternate in one call:
each round times --reps passes over the batches of the augmentation arm, then of the index_select arm;
the medians over --rounds rounds are reported.  Algorithmic bytes of one batch: every source window
read once, the output written once, the table read once; `frac_of_8TBs` is bytes / time / 8e12.
With --c2 (default) one training step of the flagship workload (C = 64, 30 blocks, batch 512, bf16)
is timed the same way, for scale.  The tool's own check: the timed batches equal the untimed ones.
Prints one JSON line per shape.  Needs a GPU: without one it fails.

  python tools/augbench.py
  python tools/augbench.py --shapes cifar --no-c2
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from differential_equations_resnet_amd.dataset_utils import (RandomBrightness, RandomCrop,  # noqa: E402
                                                             RandomFlipLeftRight, RandomSaturation, Resize,
                                                             compile_preprocessors)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def c2_step_ms(rt, dev, reps, rounds, warmup):
    """One training step (forward_backward + Adam) of C = 64, L = 30, batch 512, bf16, uint8 input."""
    C, L, N = 64, 30, 512
    ex = rt.NetExecutor(N, 32, 32, 3, C, L, 10, 8.0 / L, 0.0, subtract_mean=127.5, divide_by_stddev=127.5,
                        dtype="bfloat16", input_u8=True, device=dev)
    rng = np.random.default_rng(5)
    n_theta = rt.theta_count(C, rt.ASR_PARAM_3BY3, True, 3)
    parts = [rng.standard_normal(27 * C) * np.sqrt(2.0 / 27), rng.standard_normal(C) * 0.05]
    for _ in range(L):
        parts += [rng.standard_normal(n_theta) * np.sqrt(2.0 / (9 * C)), rng.standard_normal(C) * 0.05]
    parts += [rng.standard_normal(C * 10) * np.sqrt(2.0 / C), np.zeros(10)]
    params = torch.from_numpy(np.concatenate(parts).astype(np.float32)).to(dev)
    assert params.numel() == ex.n_params
    imgs = torch.from_numpy(rng.integers(0, 256, (N, 32, 32, 3), dtype=np.uint8)).to(dev)
    tgt = torch.from_numpy(np.eye(10, dtype=np.float32)[rng.integers(0, 10, N)]).to(dev)
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    n = [0]

    def step():
        _, g = ex.forward_backward(params, imgs, tgt)
        n[0] += 1
        rt.adam_update(params, g, m, v, 1e-4, 0.9, 0.999, 1e-7, n[0])
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    return statistics.median(timed(step, reps) for _ in range(rounds))


def bench_shape(rt, dev, name, n_src, HW, out_hw, B, a):
    rng = np.random.default_rng(7)
    feats = torch.empty((n_src, HW, HW, 3), dtype=torch.uint8, device=dev)
    chunk = max(1, (64 << 20) // (HW * HW * 3))
    for i in range(0, n_src, chunk):  # random pixels, filled in host-sized pieces
        k = min(chunk, n_src - i)
        feats[i:i + k] = torch.from_numpy(rng.integers(0, 256, (k, HW, HW, 3), dtype=np.uint8)).to(dev)
    plan = compile_preprocessors([RandomCrop(scale=0.9), Resize(out_hw), RandomFlipLeftRight(), RandomBrightness(),
                                  RandomSaturation()], (HW, HW, 3), np.uint8)
    tables, idxs = [], []
    for _ in range(a.batches):
        t = plan.draw(rng, B)
        t["src"] = rng.permutation(n_src)[:B]
        tables.append(torch.from_numpy(t.view(np.uint8)).to(dev))
        idxs.append(torch.from_numpy(t["src"].astype(np.int64)).to(dev))
    out = torch.empty((B,) + tuple(plan.out_shape), dtype=torch.float32, device=dev)
    untimed = [rt.augment_batch(feats, plan, t).clone() for t in tables]
    plain = [None]

    def aug_pass():
        for t in tables:
            rt.augment_batch(feats, plan, t, out=out)

    def sel_pass():
        for i in idxs:
            plain[0] = feats.index_select(0, i)
    for _ in range(a.warmup):
        aug_pass()
        sel_pass()
    torch.cuda.synchronize()
    ta, ts = [], []
    for _ in range(a.rounds):  # the arms alternate
        ta.append(timed(aug_pass, a.reps) / a.batches)
        ts.append(timed(sel_pass, a.reps) / a.batches)
    # the timed batches are the untimed ones (the last pass left the last table's batch in `out`)
    assert torch.equal(out, untimed[-1]), "a timed batch differs from the untimed one"
    for t, u in zip(tables, untimed):
        assert torch.equal(rt.augment_batch(feats, plan, t), u), "a repeated batch differs"
    assert torch.equal(plain[0], feats[idxs[-1]])
    ch, cw = plan.crop
    nbytes = B * (ch * cw * 3 + plan.out_shape[0] * plan.out_shape[1] * 3 * 4 + 32)
    med = statistics.median(ta)
    return {"tool": "augbench", "shape": name, "source": [n_src, HW, HW, 3], "batch": B, "crop": [ch, cw],
            "out": list(plan.out_shape), "batches": a.batches, "reps": a.reps, "rounds": a.rounds,
            "augment_us": round(med * 1e3, 2), "augment_us_min_max": [round(min(ta) * 1e3, 2), round(max(ta) * 1e3, 2)],
            "algorithmic_bytes": nbytes, "frac_of_8TBs": round(nbytes / (med * 1e-3) / 8e12, 4),
            "index_select_us": round(statistics.median(ts) * 1e3, 2),
            "index_select_bytes": 2 * B * HW * HW * 3}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="cifar,wide")
    ap.add_argument("--wide-n", type=int, default=2048, help="images of the wide dataset array")
    ap.add_argument("--batches", type=int, default=8, help="different batches per pass")
    ap.add_argument("--reps", type=int, default=10, help="passes per timed round")
    ap.add_argument("--rounds", type=int, default=9, help="timed rounds per arm")
    ap.add_argument("--warmup", type=int, default=3, help="untimed passes")
    ap.add_argument("--no-c2", dest="c2", action="store_false", help="skip the flagship step's time")
    a = ap.parse_args()
    from differential_equations_resnet_amd import runtime as rt
    dev = rt.require_gpu()  # raises without a GPU
    c2 = round(c2_step_ms(rt, dev, 5, 7, 3) * 1e3, 1) if a.c2 else None
    for name in a.shapes.split(","):
        if name == "cifar":
            r = bench_shape(rt, dev, name, 50000, 32, (32, 32), 512, a)
        elif name == "wide":
            r = bench_shape(rt, dev, name, a.wide_n, 256, (224, 224), 128, a)
        else:
            raise SystemExit(f"unknown shape {name!r} (cifar, wide)")
        r["c2_step_us"] = c2
        if c2 and name == "cifar":  # the same 512 images: the batch's share of the step it feeds
            r["augment_over_c2_step"] = round(r["augment_us"] / c2, 4)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
