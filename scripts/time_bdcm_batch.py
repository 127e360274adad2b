"""Time BDCM sweeps over G graphs as one union (``bdcm_converge_batch``) against
the same G graphs through the single-plan ``bdcm_converge`` one after the
other, and print ONE JSON line.

Workload (the notebook's regime, nb:455-515): G(n, deg/(n-1)) core graphs from
this package's sampler, n = 1000, mean degree 5, p = c = 1, lambda = 0.5,
damping 0.1, uniform random normalised messages.  eps = 0 and T_max = K, so
every instance does exactly K sweeps in both paths (asserted); both replay a
captured hipGraph of 32 sweeps and read their control block once per replay.

Timing: per G one warm-up run of each path (graph capture, LDS opt-in,
allocator), then ``--reps`` timed runs of each, the two paths alternating; the
host clock around a run that begins after a device synchronise and ends in one
(the runs end in a device->host read of the control block anyway).  Reported
per path: median and min/max of the runs, instance-sweeps per second from the
median; per G the ratio sequential / batch and whether the gap exceeds the
spread (the slowest batch run is faster than the fastest sequential run).
``single_vs_batch_g1`` sets the batch path at G = 1 beside the single-plan path
on the same graph.

    python scripts/time_bdcm_batch.py [--sizes 1 8 32 128] [--sweeps 512] [--reps 3] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(runs, work):
    med = float(np.median(runs))
    return {"runs_s": [round(x, 6) for x in runs], "median_s": med, "min_s": float(min(runs)),
            "max_s": float(max(runs)), "instance_sweeps_per_s": work / med}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--deg", type=float, default=5.0)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--sweeps", type=int, default=512, help="K: sweeps per instance and run")
    ap.add_argument("--batch-sweeps", type=int, default=32, help="sweeps per captured graph")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.reps < 3:
        ap.error("--reps must be at least 3")
    import torch
    import mjx

    p, c, lm, damp, K = 1, 1, 0.5, 0.1, a.sweeps
    rng = np.random.default_rng(0)
    plans, chi0 = [], []
    for g in range(max(a.sizes)):
        pl = mjx.bdcm_er_plan(a.n, a.deg / (a.n - 1), seed=1000 + g)
        x = rng.random((2 * pl.E, 4 ** (p + c)))
        plans.append(pl)
        chi0.append(x / x.sum(axis=1, keepdims=True))
    res = {"workload": {"n": a.n, "mean_degree": a.deg, "p": p, "c": c, "lmbd": lm, "damppar": damp, "eps": 0.0,
                        "sweeps_per_run": K, "sweeps_per_graph_replay": a.batch_sweeps, "reps": a.reps,
                        "rows_per_instance_mean": float(np.mean([2 * pl.E for pl in plans])),
                        "edge_classes_instance0": len(plans[0].classes)},
           "device": torch.cuda.get_device_name(0), "sizes": {}}

    for G in a.sizes:
        bt = mjx.BDCMBatch(plans[:G], p, c)
        chi_b = bt.chi_from(chi0[:G])
        chi_s = [torch.from_numpy(x).to(bt.device) for x in chi0[:G]]

        def run_batch():
            t, _ = mjx.bdcm_converge_batch(chi_b, bt, p, c, 1, lm, damp, 0.0, K, batch_sweeps=a.batch_sweeps)
            assert np.all(t == K), t

        def run_seq():
            for ch, pl in zip(chi_s, plans[:G]):
                t, _ = mjx.bdcm_converge(ch, pl, p, c, 1, lm, damp, 0.0, K, batch=a.batch_sweeps)
                assert t == K, t

        run_batch()
        run_seq()
        tb, ts = [], []
        for _ in range(a.reps):
            tb.append(timed(run_batch))
            ts.append(timed(run_seq))
        # both paths did the same sweeps from the same messages: the same bits
        same = all(torch.equal(v, s) for v, s in zip(bt.views(chi_b), chi_s))
        sb, ss = stats(tb, G * K), stats(ts, G * K)
        res["sizes"][str(G)] = {"batch": sb, "sequential": ss, "ratio_sequential_over_batch": ss["median_s"] / sb["median_s"],
                                "gap_exceeds_spread": bool(sb["max_s"] < ss["min_s"]), "same_messages": bool(same),
                                "union_classes": len(bt.classes), "union_rows": bt.rows_total}
        if G == 1:
            res["single_vs_batch_g1"] = {"single_plan_sweep_us": 1e6 * ss["median_s"] / K,
                                         "batch_sweep_us": 1e6 * sb["median_s"] / K}
        del bt, chi_b, chi_s
        torch.cuda.empty_cache()

    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
