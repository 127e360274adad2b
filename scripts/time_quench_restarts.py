"""Time ``quench_restarts`` (a job per (start, order), the state in LDS)
against the loops of ``quench`` calls it replaces, and print ONE JSON line.

  (a) a graph per replica, the shape of SA's result files: G graphs of N
      nodes (d-regular, the device generator), one random start each at the
      first m_init of ``--m-grid`` where more than half reach consensus, one
      order.  ONE ``quench_restarts(stack, S, p, 1, orders=o)`` call against
      the loop ``python -m mjx quench`` runs on such a file:
      ``quench(graphs[k], S[k:k+1], p, 1, order=o)`` for every k.  Both must
      give the same configurations (asserted before anything is timed).
  (b) one graph, R starts, K orders per start (``seed``: job (r, k) walks
      ``default_rng([seed, r, k]).permutation(n)``): one ``quench_restarts``
      call of R K jobs against K ``quench`` calls of the R starts with K
      orders.  ``--loop-calls`` of the K calls are timed and the total is
      their median times K (``extrapolated``: true) unless all K are run.
      Also: the mean over the consensus starts of ``mag`` at k = 0 and of
      ``mag_best`` -- what the restarts buy.

``device_ms`` is the jobs' device call alone (``_run_jobs`` on packed starts
and orders already on the device); ``api_ms`` is the whole call with the
host-side order checks, the upload, the symmetry check and the unpacking.
``visited`` counts the flips tried: for the jobs every +1 spin of a consensus
start, for ``quench`` the nodes of the removable masks.

Timing: HIP events, one warm-up call, the median of ``--reps`` calls.

    python scripts/time_quench_restarts.py [--n 10000] [--graphs 64] [--restarts 64] [--out file.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, reps):
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
    return float(np.median(out)), [round(x, 3) for x in out]


def starts(R, n, m_init, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((R, n)) < (1.0 + m_init) / 2.0, 1, -1).astype(np.int64)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=10_000)
    ap.add_argument("--d", type=int, default=4)
    ap.add_argument("--p", type=int, default=3, help="T = p (c = 1)")
    ap.add_argument("--graphs", type=int, default=64, help="(a): graphs = replicas; (b): starts on one graph")
    ap.add_argument("--restarts", type=int, default=64, help="(b): orders per start")
    ap.add_argument("--m-grid", type=float, nargs="+", default=[0.8, 0.9, 0.95, 0.98],
                    help="the starts are drawn at the first of these where more than half reach consensus")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop-reps", type=int, default=None, help="timed runs of the quench loops (default: --reps)")
    ap.add_argument("--loop-calls", type=int, default=8, help="(b): quench calls timed out of --restarts")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import importlib
    import torch
    import mjx
    Q = importlib.import_module("mjx.quench")       # the module (mjx.quench is the function)

    n, d, p, c, G, K = a.n, a.d, a.p, 1, a.graphs, a.restarts
    T = p + c - 1
    loop_reps = a.reps if a.loop_reps is None else a.loop_reps
    lib = mjx.load_library()
    g0 = mjx.random_regular_graph_device(d, n, seed=1)
    caps = Q._caps(g0, T)
    lds = int(lib.mjx_quench_jobs_lds(n, T, caps))
    # one-wave workgroups: 8 waves on each of a CU's 4 SIMDs, 160 KiB of LDS per CU
    res = {"workload": {"n": n, "d": d, "p": p, "c": c, "T": T, "graphs": G, "restarts": K, "reps": a.reps,
                        "loop_reps": loop_reps},
           "device": torch.cuda.get_device_name(0),
           "lds_bytes_per_job": lds, "caps": list(caps),
           "resident_jobs_per_cu": {"by_lds": (160 * 1024) // lds, "by_waves": 32,
                                    "allowed": min(32, (160 * 1024) // lds)}}

    def pick_starts(graph_of, seed):
        """Starts at the first m_init where more than half of them reach consensus."""
        for m_init in a.m_grid:
            S = starts(G, n, m_init, seed)
            cons = np.array([bool((mjx.s_endstate(graph_of(k), S[k], p, c) == 1).all()) for k in range(G)])
            if cons.mean() > 0.5:
                break
        return S, m_init, cons

    def packed(S):
        t = torch.from_numpy(S).cuda()
        return torch.stack([mjx.pack(t[r]) for r in range(S.shape[0])])

    def per_candidate(ms, visited):
        return {"seconds": ms * 1e-3, "us_per_visited": ms * 1e3 / max(visited, 1)}

    # ---- (a) a graph per replica --------------------------------------------
    stack = np.stack([mjx.random_regular_graph_device(d, n, seed=100 + k).adj.cpu().numpy() for k in range(G)])
    S, m_a, cons = pick_starts(lambda k: stack[k], 2)
    order = np.random.default_rng(5).permutation(n)
    out = {}

    def loop():
        out["loop"] = [mjx.quench(stack[k], S[k:k + 1], p, c, order=order) for k in range(G)]

    def one_call():
        out["new"] = mjx.quench_restarts(stack, S, p, c, orders=order)

    loop()
    one_call()
    want = np.concatenate([r["conf"] for r in out["loop"]])
    assert np.array_equal(out["new"]["conf_best"], want), "(a): quench_restarts and the quench loop disagree"
    assert np.array_equal(out["new"]["flipped"][:, 0], np.concatenate([r["flipped"] for r in out["loop"]]))
    adj_t = torch.from_numpy(stack).cuda()
    g_any = mjx.Graph("ell", n, d=d, adj=adj_t[0])
    s_np, order_t = packed(S), torch.from_numpy(order.astype(np.int32)).cuda().view(1, 1, n)
    ms_dev, all_dev = median_ms(lambda: Q._run_jobs(g_any, adj_t, G, 1, p, c, caps, s_np, order_t), a.reps)
    ms_api, all_api = median_ms(one_call, a.reps)
    ms_loop, all_loop = median_ms(loop, loop_reps)
    vis_new = int((S[cons] == 1).sum())
    vis_loop = int(sum(r["visited"] for r in out["loop"]))
    res["a_graph_per_replica"] = {
        "m_init": m_a, "consensus_share": float(cons.mean()), "jobs": G, "same_configurations": True,
        "flipped_total": int(out["new"]["flipped"].sum()),
        "restarts_device": dict(per_candidate(ms_dev, vis_new), calls_ms=all_dev, jobs_per_s=G / (ms_dev * 1e-3),
                                visited=vis_new),
        "restarts_api": dict(per_candidate(ms_api, vis_new), calls_ms=all_api, jobs_per_s=G / (ms_api * 1e-3)),
        "quench_loop": dict(per_candidate(ms_loop, vis_loop), calls_ms=all_loop, jobs_per_s=G / (ms_loop * 1e-3),
                            visited=vis_loop, calls=G),
        "loop_over_restarts_api": ms_loop / ms_api, "loop_over_restarts_device": ms_loop / ms_dev}
    del adj_t, s_np, out["loop"]

    # ---- (b) one graph, R starts, K orders each -------------------------------
    R = G
    S, m_b, cons = pick_starts(lambda k: g0, 3)
    seed = 7
    orders = Q._check_orders(None, seed, K, R, n)

    def restarts_call():
        out["b"] = mjx.quench_restarts(g0, S, p, c, restarts=K, orders=orders, validate=False)

    s_np, order_t = packed(S), torch.from_numpy(orders).cuda()
    ms_dev, all_dev = median_ms(lambda: Q._run_jobs(g0, None, R, K, p, c, caps, s_np, order_t), a.reps)
    ms_api, all_api = median_ms(restarts_call, a.reps)
    calls = min(K, a.loop_calls)

    def quench_calls():
        # restart k of every start in one replica-packed call needs one order for all starts: start 0's
        out["q"] = [mjx.quench(g0, S, p, c, order=orders[0, k].astype(np.int64), validate=False) for k in range(calls)]

    ms_q, all_q = median_ms(quench_calls, loop_reps)
    full = calls == K
    ms_loop = ms_q if full else ms_q / calls * K
    vis_new = int((S[cons] == 1).sum()) * K
    vis_loop = int(sum(r["visited"] for r in out["q"])) * K // calls
    mag = out["b"]["mag"]
    res["b_restarts"] = {
        "m_init": m_b, "consensus_share": float(cons.mean()), "starts": R, "restarts": K, "jobs": R * K,
        "restarts_device": dict(per_candidate(ms_dev, vis_new), calls_ms=all_dev, jobs_per_s=R * K / (ms_dev * 1e-3),
                                visited=vis_new),
        "restarts_api": dict(per_candidate(ms_api, vis_new), calls_ms=all_api, jobs_per_s=R * K / (ms_api * 1e-3)),
        "quench_calls": dict(per_candidate(ms_loop, vis_loop), calls_timed=calls, calls_total=K,
                             extrapolated=not full, timed_ms=all_q, jobs_per_s=R * K / (ms_loop * 1e-3),
                             visited=vis_loop,
                             note="one order per call shared by the R starts: the loop cannot give a start its own"),
        "loop_over_restarts_api": ms_loop / ms_api, "loop_over_restarts_device": ms_loop / ms_dev,
        "mean_mag_start": float(S[cons].mean()) if cons.any() else None,
        "mean_mag_k0": float(mag[cons, 0].mean()) if cons.any() else None,
        "mean_mag_best": float(out["b"]["mag_best"][cons].mean()) if cons.any() else None}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
