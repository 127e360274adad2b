"""Time ``quench_anneal`` (Metropolis add / drop sweeps inside the consensus set
behind the quench jobs) and print ONE JSON line.

The two configurations of scripts/time_quench_exchange.py:

  (a) a graph per replica, the shape of SA's result files: G graphs of N
      nodes (d-regular, the device generator), one random start each at
      ``--m-init``, one order.
  (b) one graph, R starts, K orders per start (job (r, k) walks
      ``default_rng([seed, r, k]).permutation(n)``).

For each, in one process: the device call alone (``_run_jobs`` on packed
starts and orders already on the device, HIP events, after one warm-up call
with a single sweep) for every rung of ``--sweeps``, default beta; then
``quench_exchange``'s device call on the same jobs.  Per rung: device seconds,
microseconds per proposal (the call lasts as long as its slowest job, and a job
makes sweeps x n proposals one after the other; the quench pass in front and
the closing pass are in the time, not in the count) and the mean m of the
consensus starts after the quench pass and after the walk.  A long call is
timed once: its spread is not measured.

  (parent) with ``--parent-lib`` (a libmjx.so built from the parent commit):
      ``mjx_quench_jobs_ell`` on the jobs of (b), this build and the parent's
      in turns in one process, one warm-up each, ``--reps`` calls each.

Every step runs in a child process of its own under a time limit; the steps
are chained, and after a step that fails nothing else is started (the JSON
then says where it stopped).

    python scripts/time_quench_anneal.py [--n 10000] [--graphs 64] [--restarts 8] [--sweeps 25 100 400]
                                         [--steps a b parent] [--parent-lib libmjx.so] [--out file.json]
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

LIMITS = {"a": 900, "b": 900, "parent": 300}            # step -> its time limit in seconds
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


def packed(mjx, S, orders):
    import torch
    t = torch.from_numpy(S).cuda()
    return torch.stack([mjx.pack(t[r]) for r in range(S.shape[0])]), torch.from_numpy(orders).cuda()


def measure(a, mjx, Q, g_any, adj_t, R, K, S, orders, cons):
    """The ladder and the exchange descent on the same jobs -> the step's dict."""
    import torch
    n, p, c, T = a.n, a.p, 1, a.p
    caps, cap2T = Q._caps(g_any, T), int(Q._caps(g_any, 2 * T)[2 * T])
    s_np, order_t = packed(mjx, S, orders)
    jobs = np.repeat(cons, K)

    def mean_m(plus):
        return float(((2 * plus.cpu().numpy() - n) / n)[jobs].mean())

    def best_m(plus):
        return float(((2 * plus.cpu().numpy() - n) / n).reshape(R, K).min(axis=1)[cons].mean())

    def anneal(U):
        thr, seed = Q._check_anneal(U, None, None, a.anneal_seed)
        thr_t = torch.from_numpy(thr.view(np.int32)).cuda()
        return Q._run_jobs(g_any, adj_t, R, K, p, c, caps, s_np, order_t, None, "quench_anneal", (thr_t, seed, False))

    anneal(1)                                       # warm-up (first launch, allocator)
    torch.cuda.synchronize()
    rungs = []
    for U in a.sweeps:
        ms, (_, _, plus, _, more) = timed(lambda: anneal(U))
        moves = more["moves"].cpu().numpy()[jobs].astype(np.float64)
        rungs.append({"sweeps": U, "device_seconds": ms * 1e-3, "us_per_proposal": ms * 1e3 / (U * n),
                      "ms_per_sweep": ms / U, "mean_mag_quench": mean_m(more["plus_quench"]),
                      "mean_mag_best_sweep": mean_m(more["plus_best"]), "mean_mag_anneal": mean_m(plus),
                      "mean_mag_best_anneal": best_m(plus),
                      "mean_best_sweep": float(more["best_sweep"].cpu().numpy()[jobs].mean()),
                      "per_consensus_job": {"adds": float(moves[:, 0].mean()), "drops": float(moves[:, 1].mean()),
                                            "refused": float(moves[:, 2].mean())}})
        print(f"anneal {U} sweeps: {ms * 1e-3:.2f} s", file=sys.stderr, flush=True)
    ms, (_, _, plus, _, more) = timed(lambda: Q._run_jobs(g_any, adj_t, R, K, p, c, caps, s_np, order_t,
                                                          (cap2T, MAX_PASSES, False), "quench_exchange"))
    lib = mjx.load_library()
    return {"jobs": R * K, "consensus_share": float(cons.mean()), "beta": list(Q.ANNEAL_BETA),
            "lds_bytes_per_job": int(lib.mjx_quench_anneal_jobs_lds(n, T, caps)),
            "lds_bytes_per_quench_job": int(lib.mjx_quench_jobs_lds(n, T, caps)),
            "mean_mag_start": float(S[cons].mean()), "ladder": rungs,
            "quench_exchange": {"device_seconds": ms * 1e-3, "max_passes": MAX_PASSES,
                                "mean_mag_quench": mean_m(more["plus_quench"]), "mean_mag_exchange": mean_m(plus),
                                "mean_mag_best_exchange": best_m(plus),
                                "passes": float(more["passes"].cpu().numpy()[jobs].mean())}}


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


def step_parent(a, mjx, Q):
    """quench_restarts' device call on the jobs of (b): this build and the parent's, in turns."""
    import torch
    g0, S, orders = shape_b(a, mjx, Q)
    n, R, K, T = a.n, a.graphs, a.restarts, a.p
    caps = Q._caps(g0, T)
    s_np, order_t = packed(mjx, S, orders)
    libs = {"this": mjx.load_library(), "parent": mjx._lib.open_library(os.path.abspath(a.parent_lib), verify=False)}
    dev = s_np.device
    outs = {}

    def call(which):
        o = outs.setdefault(which, (torch.empty((R * K, (n + 63) // 64), dtype=torch.int64, device=dev),
                                    torch.empty(R * K, dtype=torch.int64, device=dev),
                                    torch.empty(R * K, dtype=torch.int64, device=dev),
                                    torch.empty(R, dtype=torch.uint8, device=dev),
                                    torch.empty(R * K, dtype=torch.int32, device=dev)))
        rc = libs[which].mjx_quench_jobs_ell(g0.adj.data_ptr(), n, g0.d, 0, R, K, T, 1, caps, s_np.data_ptr(),
                                             order_t.data_ptr(), K * n, *[t.data_ptr() for t in o], None)
        assert rc == 0, (which, rc)

    for which in libs:
        call(which)                                 # warm-up
    torch.cuda.synchronize()
    ms = {which: [] for which in libs}
    for _ in range(a.reps):
        for which in libs:
            ms[which].append(timed(lambda: call(which))[0])
    for x, y in zip(outs["this"], outs["parent"]):
        assert torch.equal(x, y), "the two builds disagree"
    this, parent = spread(ms["this"]), spread(ms["parent"])
    gap = this["median_ms"] - parent["median_ms"]
    return {"jobs": R * K, "reps": a.reps, "this_build": this, "parent_build": parent, "gap_ms": gap,
            "parent_spread_ms": parent["max_ms"] - parent["min_ms"],
            "within_parent_spread": bool(gap <= parent["max_ms"] - parent["min_ms"]), "same_results": True}


def child(a):
    import importlib
    import torch
    import mjx
    Q = importlib.import_module("mjx.quench")       # the module (mjx.quench is the function)
    out = {"a": step_a, "b": step_b, "parent": step_parent}[a.step](a, mjx, Q)
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
    ap.add_argument("--sweeps", type=int, nargs="+", default=[25, 100, 400])
    ap.add_argument("--anneal-seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=9, help="(parent): timed calls per build")
    ap.add_argument("--steps", nargs="+", choices=sorted(LIMITS), default=None,
                    help="default: a b, and parent when --parent-lib is given")
    ap.add_argument("--parent-lib", default=None, help="a libmjx.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=sorted(LIMITS), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--json", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if min(a.sweeps) < 1:
        ap.error("--sweeps: every rung must be >= 1 (the figures are per sweep and per proposal)")
    if a.step:
        return child(a)
    steps = a.steps or (["a", "b"] + (["parent"] if a.parent_lib else []))
    if "parent" in steps and not a.parent_lib:
        ap.error("the parent step needs --parent-lib")
    res = {"workload": {"n": a.n, "d": a.d, "p": a.p, "c": 1, "T": a.p, "graphs": a.graphs, "restarts": a.restarts,
                        "m_init": a.m_init, "sweeps": a.sweeps, "anneal_seed": a.anneal_seed}}
    names = {"a": "a_graph_per_replica", "b": "b_restarts", "parent": "quench_restarts_vs_parent"}
    rc = 0
    with tempfile.TemporaryDirectory() as tmp:
        for step in steps:
            path = os.path.join(tmp, step + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--json", path, "--sweeps"]
            cmd += [str(u) for u in a.sweeps]
            for k in ("n", "d", "p", "graphs", "restarts", "m_init", "anneal_seed", "reps"):
                cmd += ["--" + k.replace("_", "-"), str(getattr(a, k))]
            if a.parent_lib:
                cmd += ["--parent-lib", a.parent_lib]
            try:
                rc = subprocess.run(cmd, timeout=LIMITS[step], cwd=ROOT).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:                             # a fault, an abort, a time limit: nothing more runs
                res["stopped_at"] = {"step": step, "returncode": rc}
                break
            with open(path) as f:
                res[names[step]] = json.load(f)
            res["device"] = res[names[step]].pop("device")
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
