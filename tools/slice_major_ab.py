#!/usr/bin/env python3
"""A/B of the replica-packed ELL rollout's schedules at the bench shape (d=4
RRG, N=1e6, R=4096): one slice, node-major slices (the round-1 experiment,
profiles/r01_slice_sweep.log, in the same build) and the slice-major
intermediate state (mjx_rollout_ell_rp_sm) with S in {2, 4, 8, 16, 32} and
both first-sweep variants, each at 2 and 3 sweeps per step.

A step is bench.py's: counts.zero_() + one rollout with the fused count.
HIP events around blocks of 20 steps; the configurations take turns block by
block (a slow spell of the box then falls on all of them) and each reports
the median of its blocks.  Algorithmic bytes per sweep as in DESIGN.md
section 3: 4*n*d + 8*W*n*(d + 2).

Writes <out-dir>/slice_major_ab.log (the table) and slice_major_ab.json.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def configs():
    out = [("one slice", dict(slices=1))]
    out += [(f"node-major S={S}", dict(slices=S)) for S in (4, 8)]
    for S in (2, 4, 8, 16, 32):
        for fs in (False, True):
            out.append((f"slice-major S={S} first {'sliced' if fs else 'unsliced'}",
                        dict(slices=S, layout="slice", first_sliced=fs)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=4)
    ap.add_argument("--replicas", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-steps", type=int, default=20)
    ap.add_argument("--sweeps", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    if args.blocks < 5:
        ap.error("--blocks must be at least 5")

    import numpy as np
    import torch
    import mjx
    if not torch.cuda.is_available():
        sys.exit("slice_major_ab.py: no GPU (timings are taken on the device only)")
    dev = torch.device("cuda", 0)
    n, d, R = args.n, args.d, args.replicas
    W = (R + 63) // 64
    g = mjx.Graph.ell(mjx.random_regular_graph(d, n, seed=0))
    gen = torch.Generator(device=dev).manual_seed(5)
    s0 = torch.randint(-2 ** 62, 2 ** 62, (n * W,), dtype=torch.int64, device=dev, generator=gen)
    out, tmp = torch.empty_like(s0), torch.empty_like(s0)
    counts = torch.zeros(W * 64, dtype=torch.int64, device=dev)
    sweep_bytes = 4 * n * d + 8 * W * n * (d + 2)

    rows = [(name, kw, T) for T in args.sweeps for name, kw in configs()]
    ref = {}

    def step(kw, T):
        counts.zero_()
        mjx.rollout(g, s0, T, words=W, out=out, tmp=tmp, counts=counts, **kw)

    # warm-up of every configuration, and its result against the one-slice one
    for name, kw, T in rows:
        step(kw, T)
        torch.cuda.synchronize()
        if T not in ref:
            ref[T] = (out.clone(), counts.clone())
        elif not (torch.equal(out, ref[T][0]) and torch.equal(counts, ref[T][1])):
            sys.exit(f"slice_major_ab.py: {name} at {T} sweeps differs from one slice")
    del ref

    ms = {i: [] for i in range(len(rows))}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.blocks):
        for i, (name, kw, T) in enumerate(rows):
            e0.record()
            for _ in range(args.block_steps):
                step(kw, T)
            e1.record()
            torch.cuda.synchronize()
            ms[i].append(e0.elapsed_time(e1) / args.block_steps)

    lines = [f"# d={d} RRG N={n} R={R}: ms per step (counts.zero_ + rollout with the fused count), median of "
             f"{args.blocks} blocks of {args.block_steps} steps, configurations taking turns; {torch.cuda.get_device_name(0)}",
             f"{'configuration':44s} {'sweeps':>6s} {'ms/step':>9s} {'min':>8s} {'max':>8s} {'GB/s alg.':>10s}"]
    table = []
    for i, (name, kw, T) in enumerate(rows):
        med = float(np.median(ms[i]))
        gbs = sweep_bytes * T / (med / 1e3) / 1e9
        lines.append(f"{name:44s} {T:6d} {med:9.4f} {min(ms[i]):8.4f} {max(ms[i]):8.4f} {gbs:10.0f}")
        table.append({"config": name, "args": {k: (int(v) if k != "layout" else v) for k, v in kw.items()},
                      "sweeps": T, "ms_per_step": med, "ms_blocks": ms[i], "algorithmic_GBps": gbs})
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "slice_major_ab.log"), "w") as f:
        f.write(text + "\n")
    with open(os.path.join(args.out_dir, "slice_major_ab.json"), "w") as f:
        json.dump({"n": n, "d": d, "replicas": R, "blocks": args.blocks, "block_steps": args.block_steps,
                   "algorithmic_bytes_per_sweep": sweep_bytes, "device": torch.cuda.get_device_name(0),
                   "rows": table}, f, indent=1)


if __name__ == "__main__":
    main()
