"""Time the flip gains and the greedy quench against the brute force the
package offered before them, and print ONE JSON line.

Workload: a d-regular random graph of N nodes from the device generator, R
replicas of random starts (``random_spins``), T = p + c - 1 with c = 1.

  flip_gains   ``flip_gains(g, bits, p, 1, words=W, gain=...)``: the levels
               (T rollout steps), the consensus count and the light-cone
               kernel over all (node, word column) pairs; ``kernel_ms`` is
               the entry point alone on levels built beforehand.
  brute force  the same table from ``rollout`` alone: per base replica the n
               single-flip copies in chunks of 4096 flips (64 words per node),
               ``rollout(..., T, counts=...)``, gain = 2 counts - n - F.  A full
               table is R * ceil(n / 4096) chunks; all of them are run while
               that is at most ``--brute-chunks``, else that many are timed
               and the total is the per-chunk median times the chunk count
               (``extrapolated``: true).
  quench       ``quench(g, bits, p, 1, words=W)`` end to end at the first
               m_init of ``--m-grid`` where more than half the replicas reach
               consensus, and its two parts: prepare (levels, removable mask,
               candidate lists; parallel) and the sequential pass (one
               workgroup per word column).

Timing: HIP events, one warm-up call, the median of ``--reps`` calls.

    python scripts/time_quench.py [--n 10000] [--d 4] [--p 3] [--replicas 64] [--out file.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=10_000)
    ap.add_argument("--d", type=int, default=4)
    ap.add_argument("--p", type=int, default=3, help="T = p (c = 1)")
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--m-init", type=float, default=0.5, help="starts of the flip-gain timing")
    ap.add_argument("--m-grid", type=float, nargs="+", default=[0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.98],
                    help="the quench runs at the first of these where most replicas reach consensus")
    ap.add_argument("--no-gain-table", action="store_true", help="masks only (the table is 4 n R bytes)")
    ap.add_argument("--brute-chunks", type=int, default=256, help="brute-force chunks to run at most")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quench-reps", type=int, default=None, help="timed calls of the quench (default: --reps)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import mjx
    from mjx import _device as D
    import importlib
    Q = importlib.import_module("mjx.quench")       # the module (mjx.quench is the function)

    n, d, R, p, c = a.n, a.d, a.replicas, a.p, 1
    T = p + c - 1
    W = D.words_for(R)
    g = mjx.random_regular_graph_device(d, n, seed=1)
    res = {"workload": {"n": n, "d": d, "p": p, "c": c, "T": T, "replicas": R, "words": W, "reps": a.reps,
                        "quench_reps": a.reps if a.quench_reps is None else a.quench_reps},
           "device": torch.cuda.get_device_name(0)}

    # ---- 1. flip gains -------------------------------------------------------
    bits = mjx.random_spins(n, R, a.m_init, seed=1)
    caps = Q._caps(g, T)
    levels = Q._levels(g, bits, W, T, copy=False)
    fg = {"m_init": a.m_init, "caps": list(caps), "pairs": n * W}
    for gain in ([False] if a.no_gain_table else [False, True]):
        key = "gain_table" if gain else "masks_only"
        ms_api, all_api = median_ms(lambda: mjx.flip_gains(g, bits, p, c, words=W, gain=gain, validate=False), a.reps)
        ms_k, all_k = median_ms(lambda: Q._flip_gains_packed(g, levels, R, W, p, c, T, caps, 0, gain), a.reps)
        fg[key] = {"api_ms": ms_api, "api_calls_ms": all_api, "kernel_ms": ms_k, "kernel_calls_ms": all_k,
                   "pairs_per_s": n * W / (ms_k * 1e-3), "node_replica_gains_per_s": n * R / (ms_api * 1e-3)}
    res["flip_gains"] = fg

    # ---- 2. the brute force from rollout -----------------------------------
    M = 4096
    chunks_per_replica = -(-n // M)
    total_chunks = R * chunks_per_replica
    run_chunks = min(total_chunks, a.brute_chunks)
    base_cnt = mjx.popcount(levels[T], n, words=W)
    bw = bits.view(n, W)
    node = torch.arange(n, device="cuda")
    check = mjx.flip_gains(g, bits, p, c, words=W, validate=False)["gain"] if not a.no_gain_table else None
    state = {"k": 0, "mismatch": 0}

    def brute_chunk():
        k = state["k"] % total_chunks
        state["k"] += 1
        r, i0 = k // chunks_per_replica, (k % chunks_per_replica) * M
        m = min(M, n - i0)
        base = (bw[:, r >> 6] >> (r & 63)) & 1
        flips = (-base)[:, None].repeat(1, M // 64)             # every replica of the chunk = base replica r
        j = torch.arange(m, device="cuda")
        flips[node[i0:i0 + m], j >> 6] ^= (torch.ones_like(j) << (j & 63))
        counts = torch.zeros(M, dtype=torch.int64, device="cuda")
        mjx.rollout(g, flips.view(-1), T, words=M // 64, counts=counts)
        gain = 2 * counts[:m] - 2 * base_cnt[r]
        if check is not None:
            state["mismatch"] += int((gain != check[r, i0:i0 + m]).sum().item())
        return gain

    brute_chunk()                                               # warm-up
    torch.cuda.synchronize()
    state["k"] = 0
    per = []
    for _ in range(run_chunks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        brute_chunk()
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1))
    full = run_chunks == total_chunks
    brute_ms = float(np.sum(per)) if full else float(np.median(per)) * total_chunks
    res["brute_force"] = {"chunk_flips": M, "chunks_total": total_chunks, "chunks_run": run_chunks,
                          "chunk_ms_median": float(np.median(per)), "total_ms": brute_ms, "extrapolated": not full,
                          "gain_mismatches": state["mismatch"] if check is not None else None,
                          "node_replica_gains_per_s": n * R / (brute_ms * 1e-3)}
    res["speedup_vs_brute_force"] = {k: brute_ms / fg[k]["api_ms"] for k in ("masks_only", "gain_table") if k in fg}
    del check, levels
    torch.cuda.empty_cache()

    # ---- 3. quench end to end ----------------------------------------------
    share, m_q, qbits = 0.0, None, None
    for m_q in a.m_grid:
        qbits = mjx.random_spins(n, R, m_q, seed=2)
        cnt = torch.zeros(64 * W, dtype=torch.int64, device="cuda")
        mjx.rollout(g, qbits, T, words=W, counts=cnt)
        share = float((cnt[:R] == n).sum().item()) / R
        if share > 0.5:
            break
    out = {}
    qreps = a.reps if a.quench_reps is None else a.quench_reps

    def end_to_end():
        out["q"] = mjx.quench(g, qbits, p, c, words=W, validate=False)

    ms_q, all_q = median_ms(end_to_end, qreps)
    prep = {}

    def prepare():
        levels, caps_q, removable = Q._quench_prepare(g, qbits, R, W, p, c, T, 0)
        prep["v"] = (levels, caps_q, *Q._candidates(removable, n, W, None))

    ms_prep, all_prep = median_ms(prepare, qreps)
    ms_pass, all_pass = median_ms(lambda: Q._quench_pass(g, prep["v"][0], R, W, p, c, T, *prep["v"][1:], 0), qreps,
                                  before=prepare)
    q = out["q"]
    cons = q["consensus"]
    before = (2.0 * mjx.popcount(qbits, n, words=W)[:R].double() - n) / n
    res["quench"] = {"m_init": m_q, "consensus_share": share, "end_to_end_ms": ms_q, "end_to_end_calls_ms": all_q,
                     "prepare_ms": ms_prep, "prepare_calls_ms": all_prep, "pass_ms": ms_pass,
                     "pass_calls_ms": all_pass, "pass_share": ms_pass / (ms_pass + ms_prep),
                     "candidates_visited": q["visited"], "candidates_per_s": q["visited"] / (ms_pass * 1e-3),
                     "workgroups": W, "flipped_total": int(q["flipped"].sum().item()),
                     "mean_mag_before": float(before[cons].mean().item()) if bool(cons.any()) else None,
                     "mean_mag_after": float(q["mag"][cons].mean().item()) if bool(cons.any()) else None}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
