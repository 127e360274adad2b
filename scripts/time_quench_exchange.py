"""Time ``quench_exchange`` (the (1, 2) exchange descent behind the quench jobs)
and print ONE JSON line.

  (a) a graph per replica, the shape of SA's result files: G graphs of N
      nodes (d-regular, the device generator), one random start each at
      ``--m-init``, one order.
  (b) one graph, R starts, K orders per start (job (r, k) walks
      ``default_rng([seed, r, k]).permutation(n)``).
  (host) the first pass of job (0, 0) of (b) driven from the host through the
      public calls: for every -1 node j of the order, ``quench`` on the state
      with j turned to +1, in the job's order with j moved to its end (behind
      two drops j is refused, behind fewer it is dropped or the call flipped
      one spin: the add stays exactly when the call flipped two or more).  Its
      configuration must equal the kernel's with ``max_passes=1`` (asserted);
      its time per add, times the adds of all jobs and passes of (b), is the
      ``extrapolated`` cost of the whole descent driven that way.

Every step runs in a child process of its own under a time limit; the steps
are chained, and after a step that fails nothing else is started (the JSON
then says where it stopped).

For (a) and (b): the device call alone (``_run_jobs`` on packed starts and
orders already on the device), in turns with ``quench_restarts``' call on the
same jobs, HIP events, one warm-up, the median of ``--reps``.  The split into
quench phase and exchange phase comes from the kernel's own clock readings
(``stats``): all jobs run side by side, so the call lasts as long as its
slowest job, and the call's time is divided in the proportion of that job's
ticks.  ``us_per_try``: a job's phase time over the flips it tried in it (quench
phase: the +1 spins of the start; exchange phase: adds + candidate drops; the
candidate search and the restoring flips are in the time, not in the count),
with ticks turned into time by the rate that makes the slowest job last the
call (``ticks_per_ms``).

    python scripts/time_quench_exchange.py [--n 10000] [--graphs 64] [--restarts 8] [--out file.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("a", 420), ("b", 420), ("host", 540))          # step, its time limit in seconds
MAX_PASSES = 8


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def starts(R, n, m_init, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((R, n)) < (1.0 + m_init) / 2.0, 1, -1).astype(np.int64)


def spread(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "max_ms": float(np.max(xs)),
            "calls_ms": [round(float(x), 3) for x in xs]}


def measure(a, mjx, Q, g_any, adj_t, R, K, S, orders, cons):
    """The jobs' device call, exchange and restarts in turns -> the step's dict."""
    import torch
    n, p, c, T = a.n, a.p, 1, a.p
    caps, cap2T = Q._caps(g_any, T), int(Q._caps(g_any, 2 * T)[2 * T])
    t = torch.from_numpy(S).cuda()
    s_np = torch.stack([mjx.pack(t[r]) for r in range(R)])
    order_t = torch.from_numpy(orders).cuda()

    def old():
        return Q._run_jobs(g_any, adj_t, R, K, p, c, caps, s_np, order_t)

    def new():
        return Q._run_jobs(g_any, adj_t, R, K, p, c, caps, s_np, order_t, (cap2T, MAX_PASSES, True),
                           "quench_exchange")

    old(), new()                                    # warm-up (first launch, allocator)
    torch.cuda.synchronize()
    ms_old, ms_new = [], []
    for _ in range(a.reps):
        ms, res_old = timed(old)
        ms_old.append(ms)
        ms, res_new = timed(new)
        ms_new.append(ms)
    _, flipped_old, plus_old, _ = res_old
    _, flipped, plus, _, more = res_new
    assert torch.equal(flipped, flipped_old) and torch.equal(more["plus_quench"], plus_old), \
        "the quench phase and quench_restarts disagree"
    stats = more["stats"].cpu().numpy().astype(np.float64)           # adds, tries, quench ticks, exchange ticks
    jobs = np.repeat(cons, K)                                        # the jobs of consensus starts
    ticks = stats[:, 2] + stats[:, 3]
    slow = int(np.argmax(ticks))
    new_ms = float(np.median(ms_new))
    ticks_per_ms = ticks[slow] / new_ms
    quench_ms, exchange_ms = new_ms * stats[slow, 2] / ticks[slow], new_ms * stats[slow, 3] / ticks[slow]
    tries_q = np.repeat((S == 1).sum(axis=1), K).astype(np.float64)
    tries_x = stats[:, 0] + stats[:, 1]
    us_q = stats[jobs, 2] / ticks_per_ms * 1e3 / tries_q[jobs]
    us_x = stats[jobs, 3] / ticks_per_ms * 1e3 / np.maximum(tries_x[jobs], 1)
    passes, exchanges = more["passes"].cpu().numpy(), more["exchanges"].cpu().numpy()
    mag_q = (2 * more["plus_quench"].cpu().numpy() - n) / n
    mag_x = (2 * plus.cpu().numpy() - n) / n
    old_s = spread(ms_old)
    gap = quench_ms - old_s["median_ms"]
    return {
        "jobs": R * K, "consensus_share": float(cons.mean()), "max_passes": MAX_PASSES,
        "lds_bytes_per_job": int(mjx.load_library().mjx_quench_exchange_jobs_lds(n, T, caps, cap2T)), "cap2T": cap2T,
        "exchange_call": spread(ms_new), "quench_restarts_call": old_s,
        "slowest_job": {"job": slow, "ticks_per_ms": ticks_per_ms, "quench_phase_ms": quench_ms,
                        "exchange_phase_ms": exchange_ms, "passes": int(passes[slow]), "adds": int(stats[slow, 0]),
                        "tries": int(stats[slow, 1])},
        "per_consensus_job": {"passes": float(passes[jobs].mean()), "passes_max": int(passes[jobs].max()),
                              "exchanges": float(exchanges[jobs].mean()), "adds": float(stats[jobs, 0].mean()),
                              "candidate_tries": float(stats[jobs, 1].mean()),
                              "tries_per_add": float(stats[jobs, 1].sum() / max(stats[jobs, 0].sum(), 1)),
                              "quench_phase_ms": float((stats[jobs, 2] / ticks_per_ms).mean()),
                              "exchange_phase_ms": float((stats[jobs, 3] / ticks_per_ms).mean()),
                              "us_per_try_quench": float(us_q.mean()), "us_per_try_exchange": float(us_x.mean()),
                              "all_converged": bool(more["converged"].cpu().numpy()[jobs].all())},
        "quench_phase_vs_quench_restarts": {
            "quench_phase_ms": quench_ms, "quench_restarts_ms": old_s["median_ms"], "gap_ms": gap,
            "quench_restarts_spread_ms": old_s["max_ms"] - old_s["min_ms"],
            "within_spread": bool(abs(gap) <= old_s["max_ms"] - old_s["min_ms"]),
            "note": "quench_phase_ms is the share of the exchange call's time its slowest job spent in the quench "
                    "phase by its own clock; quench_restarts_ms is the parent kernel's whole call"},
        "mean_mag_start": float(S[cons].mean()), "mean_mag_quench": float(mag_q[jobs].mean()),
        "mean_mag_exchange": float(mag_x[jobs].mean()),
        "mean_mag_best_quench": float(mag_q.reshape(R, K).min(axis=1)[cons].mean()),
        "mean_mag_best_exchange": float(mag_x.reshape(R, K).min(axis=1)[cons].mean()),
    }


def consensus_of(mjx, graph_of, S, p):
    return np.array([bool((mjx.s_endstate(graph_of(k), S[k], p, 1) == 1).all()) for k in range(S.shape[0])])


def step_a(a, mjx, Q):
    import torch
    n, d, G = a.n, a.d, a.graphs
    stack = np.stack([mjx.random_regular_graph_device(d, n, seed=100 + k).adj.cpu().numpy() for k in range(G)])
    S = starts(G, n, a.m_init, 2)
    cons = consensus_of(mjx, lambda k: stack[k], S, a.p)
    adj_t = torch.from_numpy(stack).cuda()
    g_any = mjx.Graph("ell", n, d=d, adj=adj_t[0])
    orders = np.random.default_rng(5).permutation(n).astype(np.int32).reshape(1, 1, n)
    return dict(measure(a, mjx, Q, g_any, adj_t, G, 1, S, orders, cons), m_init=a.m_init, graphs=G)


def shape_b(a, mjx, Q):
    g0 = mjx.random_regular_graph_device(a.d, a.n, seed=1)
    S = starts(a.graphs, a.n, a.m_init, 3)
    return g0, S, Q._check_orders(None, 7, a.restarts, a.graphs, a.n)


def step_b(a, mjx, Q):
    g0, S, orders = shape_b(a, mjx, Q)
    cons = consensus_of(mjx, lambda k: g0, S, a.p)
    return dict(measure(a, mjx, Q, g0, None, a.graphs, a.restarts, S, orders, cons), m_init=a.m_init,
                starts=a.graphs, restarts=a.restarts)


def step_host(a, mjx, Q):
    """Pass 1 of job (0, 0) of (b), or of the first consensus start's first job, from the host."""
    g0, S, orders = shape_b(a, mjx, Q)
    n, p = a.n, a.p
    r = int(np.flatnonzero(consensus_of(mjx, lambda k: g0, S, p))[0])
    order = orders[r, 0].astype(np.int64)
    kernel = mjx.quench_exchange(g0, S[r], p, 1, orders=order, max_passes=1, validate=False)
    x = mjx.quench(g0, S[r], p, 1, order=order, validate=False)["conf"].copy()
    assert (2 * (x == 1).sum() - n) / n == kernel["mag_quench"][0, 0]
    mjx.quench(g0, x, p, 1, order=order, validate=False)             # warm-up
    adds = kept = 0

    def descent():
        nonlocal adds, kept, x
        for pos in range(n):
            j = order[pos]
            if x[j] != -1:
                continue
            y = x.copy()
            y[j] = 1
            q = mjx.quench(g0, y, p, 1, order=np.concatenate([order[:pos], order[pos + 1:], order[pos:pos + 1]]),
                           validate=False)
            adds += 1
            if int(q["flipped"][0]) >= 2:
                x = q["conf"]
                kept += 1

    ms, _ = timed(descent)
    assert np.array_equal(x, kernel["conf_best"]), "the host-driven pass and the kernel's first pass disagree"
    assert kept == int(kernel["exchanges"][0, 0])
    return {"start": r, "adds_timed": adds, "exchanges": kept, "same_configuration": True, "seconds": ms * 1e-3,
            "ms_per_add": ms / max(adds, 1)}


def child(a):
    import importlib
    import torch
    import mjx
    Q = importlib.import_module("mjx.quench")       # the module (mjx.quench is the function)
    out = {"a": step_a, "b": step_b, "host": step_host}[a.step](a, mjx, Q)
    out["device"] = torch.cuda.get_device_name(0)
    with open(a.json, "w") as f:
        json.dump(out, f)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=10_000)
    ap.add_argument("--d", type=int, default=4)
    ap.add_argument("--p", type=int, default=3, help="T = p (c = 1)")
    ap.add_argument("--graphs", type=int, default=64, help="(a): graphs = replicas; (b): starts on one graph")
    ap.add_argument("--restarts", type=int, default=8, help="(b): orders per start")
    ap.add_argument("--m-init", type=float, default=0.8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--json", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.step:
        return child(a)
    res = {"workload": {"n": a.n, "d": a.d, "p": a.p, "c": 1, "T": a.p, "graphs": a.graphs, "restarts": a.restarts,
                        "m_init": a.m_init, "reps": a.reps}}
    names = {"a": "a_graph_per_replica", "b": "b_restarts", "host": "host_driven_first_pass"}
    rc = 0
    with tempfile.TemporaryDirectory() as tmp:
        for step, limit in STEPS:
            path = os.path.join(tmp, step + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--json", path]
            for k in ("n", "d", "p", "graphs", "restarts", "m_init", "reps"):
                cmd += ["--" + k.replace("_", "-"), str(getattr(a, k))]
            try:
                rc = subprocess.run(cmd, timeout=limit, cwd=ROOT).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:                             # a fault, an abort, a time limit: nothing more runs
                res["stopped_at"] = {"step": step, "returncode": rc}
                break
            with open(path) as f:
                res[names[step]] = json.load(f)
            res["device"] = res[names[step]].pop("device")
    if "b_restarts" in res and "host_driven_first_pass" in res:
        b, h = res["b_restarts"], res["host_driven_first_pass"]
        adds_all = b["per_consensus_job"]["adds"] * b["consensus_share"] * b["jobs"]
        host_s = h["ms_per_add"] * 1e-3 * adds_all
        res["host_driven_vs_kernel"] = {
            "extrapolated": True, "adds_timed": h["adds_timed"], "adds_of_all_jobs_and_passes": adds_all,
            "host_driven_seconds": host_s, "kernel_exchange_phase_seconds": b["slowest_job"]["exchange_phase_ms"] * 1e-3,
            "host_over_kernel": host_s / (b["slowest_job"]["exchange_phase_ms"] * 1e-3),
            "note": "ms_per_add of the timed first pass of one job times the adds of (b)'s jobs in all their passes, "
                    "one job after the other as the host loop would run them"}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
