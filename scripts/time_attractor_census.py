"""Time the attractor census (csrc/mjx_census.hip, k_attractor_census: all 2^n
configurations generated in the kernel and run until s(t+2) = s(t)) and write
ONE JSON file.  Random regular graphs of d = 3 and d = 4 at n = 32, t_max = 32,
graph seed 1, all 2^32 configurations.

  census    per graph, in one process and in turns: the device loop of
            ``attractor_census`` (``census._run_attractor``, launches of
            ``chunk_blocks`` blocks) and of ``census(graph, 3, 1)``
            (``census._run``) under HIP events, one warm-up each, the median of
            ``--reps``; the mean number of sweeps a wave made (the kernel's
            stats words), the ratio of the two times next to sweeps / 3, every
            launch of one more pass timed on its own (``longest_launch_ms``),
            and the findings: class totals, p_plus around the transition,
            min_plus_ever against census's min_plus[3], p_longest.
  baseline  what the package offered before: the top 2^``--baseline-log2``
            configurations built on the host in pieces of 2^20 rows, run
            through ``attractor`` and binned; the bins must equal the kernel's
            for the same block range (asserted).  The time of 2^n
            configurations is EXTRAPOLATED from the sub-range
            (``extrapolated``: true).

Every step that uses the GPU runs in a child process under its own time limit;
the first that fails ends the script.

    python scripts/time_attractor_census.py [--reps 3] [--out profiles/attractor_census_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [("census3", 240), ("census4", 240), ("baseline3", 300), ("baseline4", 300)]     # (step, seconds)


def timed_ms(fn, reps):
    import torch
    fn()                                    # warm-up (first launch, allocator)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def step_census(a, d, mjx, cs):
    import torch
    n, t_max = a.n, a.t_max
    g = mjx.Graph.ell(mjx.random_regular_graph(d, n, seed=1))
    B = 1 << (n - 6)
    t0 = time.perf_counter()
    res = mjx.attractor_census(g, t_max)
    api_s = time.perf_counter() - t0
    cen = mjx.census(g, 3, 1)
    # in turns: a pass of each per repetition, one warm-up of each first
    ac_ms, ce_ms = [], []
    cs._run_attractor(g, t_max, 0, B, cs.CHUNK_BLOCKS, 0)
    cs._run(g, 3, 1, 0, B, cs.CHUNK_BLOCKS, 0)
    for _ in range(a.reps):
        ac_ms += timed_ms(lambda: cs._run_attractor(g, t_max, 0, B, cs.CHUNK_BLOCKS, 0), 1)
        ce_ms += timed_ms(lambda: cs._run(g, 3, 1, 0, B, cs.CHUNK_BLOCKS, 0), 1)
    ac, ce = float(np.median(ac_ms)), float(np.median(ce_ms))
    # one more pass, launch by launch
    dev = g.adj.device
    hist = torch.zeros((4, t_max + 1, n + 1), dtype=torch.int64, device=dev)
    uns = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    keys = torch.tensor([-1, 0], dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    st = cs._device.stream_handle()
    ev = []
    for lo in range(0, B, cs.CHUNK_BLOCKS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        cs._lib.call("mjx_attractor_census_ell", cs._device.ptr(g.adj), n, d, t_max, lo, min(B, lo + cs.CHUNK_BLOCKS), 0,
                     cs._device.ptr(hist), cs._device.ptr(uns), cs._device.ptr(keys), cs._device.ptr(flag), None, st)
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    launches = [e0.elapsed_time(e1) for e0, e1 in ev]
    assert int(flag.item()) == 0 and np.array_equal(hist.cpu().numpy(), res["hist"])
    totals = res["hist"].sum(axis=(1, 2))
    by_p = res["hist"].sum(axis=(0, 2))
    assert np.array_equal(res["reach_plus"][3], cen["counts"][3]), "the horizon-3 level of both kernels"
    k0 = int(np.flatnonzero(res["p_plus"] > 0)[0])
    return {"d": d, "graph_seed": 1, "n": n, "t_max": t_max, "configs": 1 << n, "chunk_blocks": cs.CHUNK_BLOCKS,
            "lds_bytes": cs.attractor_census_lds(n, t_max), "api_s": round(api_s, 4),
            "device_ms": round(ac, 3), "device_ms_all": [round(x, 3) for x in ac_ms],
            "configs_per_s": (1 << n) / (ac / 1e3), "mean_sweeps": res["mean_sweeps"],
            "census_p3_device_ms": round(ce, 3), "census_p3_device_ms_all": [round(x, 3) for x in ce_ms],
            "time_ratio_to_census_p3": ac / ce, "sweep_ratio_to_census_p3": res["mean_sweeps"] / 3,
            "cost_per_sweep_relative_to_census": (ac / ce) / (res["mean_sweeps"] / 3),
            "launches": len(launches), "longest_launch_ms": round(max(launches), 3),
            "median_launch_ms": round(float(np.median(launches)), 3),
            "findings": {"classes": dict(zip(res["classes"], totals.tolist())),
                         "unsettled": int(res["unsettled"].sum()), "configs_by_transient": by_p.tolist(),
                         "p_longest": res["p_longest"],
                         "witness_longest_x": int(sum(1 << v for v in np.flatnonzero(res["witness_longest"] == 1))),
                         "min_plus_ever": res["min_plus_ever"], "m_min_ever": res["m_min_ever"],
                         "census_min_plus_p3": int(cen["min_plus"][3]), "first_k_with_p_plus": k0,
                         "p_plus": {str(k): float(res["p_plus"][k]) for k in range(k0, n + 1)}}}


def step_baseline(a, d, mjx, cs):
    import torch
    n, t_max = a.n, a.t_max
    g = mjx.Graph.ell(mjx.random_regular_graph(d, n, seed=1))
    sub = 1 << a.baseline_log2
    lo, piece = (1 << n) - sub, 1 << 20
    want, wuns, _, _ = cs._run_attractor(g, t_max, lo // 64, 1 << (n - 6), cs.CHUNK_BLOCKS, 0)
    hist = torch.zeros(4 * (t_max + 1) * (n + 1), dtype=torch.int64, device="cuda")
    uns = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for x0 in range(lo, 1 << n, piece):
        x = np.arange(x0, x0 + piece, dtype="<u8")
        bits = np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")[:, :n]
        S = torch.from_numpy(2 * bits.astype(np.int8) - 1).cuda()
        r = mjx.attractor(g, S, t_max)
        p, c, s0 = r["p"], r["c"], r["sum_att"][:, 0]
        k = (S == 1).sum(dim=1)
        cls = torch.where(c == 2, 3, torch.where(s0 == n, 0, torch.where(s0 == -n, 1, 2)))
        done = p >= 0
        hist += torch.bincount(((cls[done] * (t_max + 1) + p[done]) * (n + 1) + k[done]), minlength=hist.numel())
        uns += torch.bincount(k[~done], minlength=n + 1)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    assert np.array_equal(hist.cpu().numpy().reshape(4, t_max + 1, n + 1), want.cpu().numpy()), \
        "attractor and the attractor census disagree on the sub-range"
    assert np.array_equal(uns.cpu().numpy(), wuns.cpu().numpy())
    return {"d": d, "configs": sub, "wall_s": round(wall, 4), "configs_per_s": sub / wall, "extrapolated": True,
            "wall_s_full": wall * ((1 << n) / sub), "equal_to_kernel_on_the_range": True}


def child(a):
    import importlib
    import torch
    import mjx
    cs = importlib.import_module("mjx.census")
    fn = step_census if a.step.startswith("census") else step_baseline
    out = fn(a, int(a.step[-1]), mjx, cs)
    out["device"] = torch.cuda.get_device_name(0)
    with open(a.json, "w") as f:
        json.dump(out, f)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--t-max", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-log2", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attractor_census_timing.json"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--json", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.step:
        return child(a)
    res = {"n": a.n, "t_max": a.t_max, "reps": a.reps, "cases": {}}
    rc = 0
    with tempfile.TemporaryDirectory() as tmp:
        for step, limit in STEPS:
            path = os.path.join(tmp, step + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--json", path, "--n", str(a.n),
                   "--t-max", str(a.t_max), "--reps", str(a.reps), "--baseline-log2", str(a.baseline_log2)]
            try:
                rc = subprocess.run(cmd, timeout=limit, cwd=ROOT).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:                             # a fault, an abort, a time limit: nothing more runs
                res["stopped_at"] = {"step": step, "returncode": rc}
                break
            with open(path) as f:
                res["cases"][step] = json.load(f)
            res["device"] = res["cases"][step].pop("device")
            print(json.dumps({step: res["cases"][step]}), flush=True)
    for d in (3, 4):
        c, b = res["cases"].get(f"census{d}"), res["cases"].get(f"baseline{d}")
        if c and b:
            c["speedup_vs_attractor_baseline"] = {"extrapolated": True,
                                                  "value": b["wall_s_full"] / (c["device_ms"] / 1e3)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out, "stopped_at": res.get("stopped_at")}), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
