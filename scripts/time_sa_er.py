"""Time the light-cone SA step on an Erdos-Renyi graph against the regular-graph
general path, and print ONE JSON line.

Workload: G(N, 5/(N-1)) from the device sampler, p=2, c=1, R replicas,
``SAReplicasER(mode="lightcone")``.  Baseline, same process: ``SAReplicas`` on a
d=6 random regular graph of the same N, R, p, c with ``mode="lightcone",
layout="levels", tape=0`` (the general kernel, proposals drawn in the step).

Timing: HIP events around ``steps(k)``, one warm-up call, the median of
``--reps`` calls.  us_per_step = time of a call / k (every replica makes one
proposal per step); proposals_per_s = R * k / time.

Expected bound of the ratio ER / baseline: 1.5 * rho, where
rho = E[max over 64 random nodes of the radius-2 ball size] / 37 (37 = the
radius-2 ball of the d=6 tree; a wave advances at the pace of its largest ball)
is computed on the host from the benchmark graph, and 1.5 is the CSR walk's
third dependent load (row_ptr) on top of the ELL walk's two per level.

    python scripts/time_sa_er.py [--n 1000000] [--replicas 4096] [--steps 2000] [--out file.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, reps):
    import torch
    fn()                                    # warm-up (first launch, LDS opt-in, allocator)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), [round(x, 4) for x in out]


def ball2_stats(rp, col, groups=2000, seed=0):
    """(mean radius-2 ball size, E[max over 64 random nodes]) of a CSR graph, from
    ``groups`` x 64 sampled nodes (distinct nodes within distance 2, the node included)."""
    rng = np.random.default_rng(seed)
    n = rp.shape[0] - 1
    nodes = rng.integers(0, n, size=groups * 64)
    size = np.empty(nodes.shape[0], dtype=np.int64)
    for j, v in enumerate(nodes):
        nb = col[rp[v]:rp[v + 1]]
        parts = [np.array([v]), nb] + [col[rp[k]:rp[k + 1]] for k in nb]
        size[j] = np.unique(np.concatenate(parts)).shape[0]
    return float(size.mean()), float(size.reshape(groups, 64).max(axis=1).mean())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--deg", type=float, default=5.0)
    ap.add_argument("--replicas", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rollout-n", type=int, default=100_000, help="size of the rollout-mode orientation run (0: skip)")
    ap.add_argument("--rollout-steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import mjx
    from mjx.sa_er import lightcone_stats

    p, c, R = 2, 1, a.replicas
    seeds = list(range(R))
    res = {"workload": {"n": a.n, "mean_degree": a.deg, "p": p, "c": c, "replicas": R, "steps_per_call": a.steps,
                        "reps": a.reps}, "device": torch.cuda.get_device_name(0)}

    g = mjx.erdos_renyi_device(a.n, a.deg / (a.n - 1), seed=1)
    rp, col = g.row_ptr.cpu().numpy(), g.col.cpu().numpy()
    mean2, max64 = ball2_stats(rp, col)
    rho = max64 / 37.0
    er = mjx.SAReplicasER(g, p, c, seeds, mode="lightcone")
    lightcone_stats(reset=True)
    ms, all_ms = median_ms(lambda: er.steps(a.steps), a.reps)
    props, spilled = lightcone_stats(reset=True)
    res["er_lightcone"] = {"ms_per_call": ms, "calls_ms": all_ms, "us_per_step": 1e3 * ms / a.steps,
                           "proposals_per_s": R * a.steps / (ms * 1e-3), "caps": er.caps,
                           "spill_bytes": er.spill_bytes, "max_degree": int(np.diff(rp).max()),
                           "proposals": props, "spilled": spilled, "spill_rate": spilled / max(props, 1)}
    del er
    torch.cuda.empty_cache()

    rrg = mjx.random_regular_graph_device(6, a.n, seed=1)
    base = mjx.SAReplicas(rrg, p, c, seeds, mode="lightcone", layout="levels", tape=0)
    ms_b, all_b = median_ms(lambda: base.steps(a.steps), a.reps)
    res["rrg_d6_levels_notape"] = {"ms_per_call": ms_b, "calls_ms": all_b, "us_per_step": 1e3 * ms_b / a.steps,
                                   "proposals_per_s": R * a.steps / (ms_b * 1e-3)}
    del base, rrg
    torch.cuda.empty_cache()

    res["ball2"] = {"mean": mean2, "mean_max_of_64": max64, "rrg_d6": 37, "rho": rho}
    res["ratio"] = ms / ms_b
    res["bound_1p5_rho"] = 1.5 * rho
    res["within_bound"] = bool(ms / ms_b <= 1.5 * rho)

    if a.rollout_n:
        g2 = mjx.erdos_renyi_device(a.rollout_n, a.deg / (a.rollout_n - 1), seed=1)
        ro = mjx.SAReplicasER(g2, p, c, seeds, mode="rollout")
        ms_r, all_r = median_ms(lambda: ro.steps(a.rollout_steps), max(3, a.reps // 2))
        res["er_rollout"] = {"n": a.rollout_n, "steps_per_call": a.rollout_steps, "ms_per_call": ms_r,
                             "calls_ms": all_r, "us_per_step": 1e3 * ms_r / a.rollout_steps,
                             "proposals_per_s": R * a.rollout_steps / (ms_r * 1e-3)}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
