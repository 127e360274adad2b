"""Time ``quench(schedule="regions")`` against the sequential pass on the two
shapes of scripts/time_quench.py, and write profiles/quench_regions_timing.json.

Workload, as there: a d-regular random graph from the device generator (seed
1), R replicas of random starts (``random_spins``, seed 2) at the first m_init
of ``--m-grid`` where more than half the replicas reach consensus, T = p + c - 1
with c = 1, the identity order.

  small   n = 1e4, R = 64    (one word column),  median of 7 calls
  large   n = 1e6, R = 4096  (64 word columns),  median of 3 calls

Per shape: ``quench(..., schedule="sequential")`` end to end (the path the
package had before the regions pass: ``k_quench``), then for the
default window and the ``--window-factors`` multiples of it the regions pass
end to end and alone (``_quench_regions_pass`` on levels, mask and candidates
prepared beforehand), with its rounds, window and commits per round.  Every
regions result is compared with the sequential one (``torch.equal`` on the
packed state, ``array_equal`` on flipped and consensus); a difference ends the
script with an error.

Timing: HIP events, one warm-up call, the median of the timed calls.

    python scripts/time_quench_regions.py [--shapes small large] [--out profiles/quench_regions_timing.json]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"small": {"n": 10_000, "replicas": 64, "reps": 7}, "large": {"n": 1_000_000, "replicas": 4096, "reps": 3}}


def median_ms(fn, reps, before=None):
    import torch
    if before is not None:
        before()
    fn()                                    # warm-up (first launch, allocator)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), [round(x, 4) for x in out]


def run_shape(name, a):
    import torch
    import mjx
    from mjx import _device as D
    Q = importlib.import_module("mjx.quench")       # the module (mjx.quench is the function)
    n, R, reps = SHAPES[name]["n"], SHAPES[name]["replicas"], SHAPES[name]["reps"]
    d, p, c = a.d, a.p, 1
    T = p + c - 1
    W = D.words_for(R)
    g = mjx.random_regular_graph_device(d, n, seed=1)
    share, m_q, bits = 0.0, None, None
    for m_q in a.m_grid:
        bits = mjx.random_spins(n, R, m_q, seed=2)
        cnt = torch.zeros(64 * W, dtype=torch.int64, device="cuda")
        mjx.rollout(g, bits, T, words=W, counts=cnt)
        share = float((cnt[:R] == n).sum().item()) / R
        if share > 0.5:
            break
    res = {"workload": {"n": n, "d": d, "p": p, "c": c, "T": T, "replicas": R, "words": W, "reps": reps,
                        "m_init": m_q, "consensus_share": share, "order": "identity"}}
    out = {}

    def sequential():
        out["seq"] = mjx.quench(g, bits, p, c, words=W, validate=False)

    ms, calls = median_ms(sequential, reps)
    seq = out["seq"]
    res["sequential"] = {"end_to_end_ms": ms, "end_to_end_calls_ms": calls, "visited": seq["visited"],
                         "workgroups": W, "flipped_total": int(seq["flipped"].sum().item())}
    caps = Q._caps(g, T)
    default = Q.default_window(n, caps[T])
    prep = {}

    def prepare():
        levels, _, removable = Q._quench_prepare(g, bits, R, W, p, c, T, 0)
        prep["v"] = (levels, removable, Q._union_candidates(removable, n, W, None)[0])

    ms_prep, _ = median_ms(prepare, reps)
    res["prepare_ms"] = ms_prep
    res["regions"] = []
    for f in a.window_factors:
        window = max(1, int(round(default * f)))

        def regions():
            out["reg"] = mjx.quench(g, bits, p, c, words=W, validate=False, schedule="regions", window=window)

        def the_pass():
            levels, removable, cand = prep["v"]
            Q._quench_regions_pass(g, levels, R, W, p, c, T, caps, removable, cand, window, 0)

        ms, calls = median_ms(regions, reps)
        ms_pass, calls_pass = median_ms(the_pass, reps, before=prepare)
        reg = out["reg"]
        equal = bool(torch.equal(reg["state"], seq["state"]) and torch.equal(reg["flipped"], seq["flipped"]) and
                     torch.equal(reg["consensus"], seq["consensus"]) and reg["visited"] == seq["visited"])
        union = int(prep["v"][2].numel())
        res["regions"].append({"window": reg["window"], "window_factor": f, "default_window": default,
                               "end_to_end_ms": ms, "end_to_end_calls_ms": calls, "pass_ms": ms_pass,
                               "pass_calls_ms": calls_pass, "rounds": reg["rounds"], "max_commits": reg["max_commits"],
                               "union_candidates": union, "commits_per_round": union / max(1, reg["rounds"]),
                               "equal_to_sequential": equal,
                               "sequential_over_regions": res["sequential"]["end_to_end_ms"] / ms})
        if not equal:
            raise SystemExit(f"{name}: the regions pass at window {window} differs from the sequential pass")
    del prep, out
    torch.cuda.empty_cache()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", nargs="+", choices=sorted(SHAPES), default=["small", "large"])
    ap.add_argument("--d", type=int, default=4)
    ap.add_argument("--p", type=int, default=3, help="T = p (c = 1)")
    ap.add_argument("--m-grid", type=float, nargs="+", default=[0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.98])
    ap.add_argument("--window-factors", type=float, nargs="+", default=[0.25, 1.0, 4.0],
                    help="windows to time, as multiples of the default window")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "quench_regions_timing.json"))
    a = ap.parse_args(argv)
    import torch
    res = {}
    if os.path.exists(a.out):               # a run of one shape keeps the other's record
        with open(a.out) as f:
            res = json.load(f)
    res["device"] = torch.cuda.get_device_name(0)
    for name in a.shapes:
        res[name] = run_shape(name, a)
        print(json.dumps({name: res[name]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
