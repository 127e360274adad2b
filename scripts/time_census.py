"""Time the consensus census (csrc/mjx_census.hip: all 2^n configurations
generated in the kernel) against the same census through the API as it stood
before -- the host builds the configurations, ``pack`` packs them and
``rollout(..., counts=)`` steps them level by level -- and write ONE JSON file.

  census    d = 3 and d = 4 random regular graphs at n = 32, T = p + c - 1 = 3:
            2^32 configurations each (``--n36``: also n = 36, d = 3).  The
            device loop of ``census`` (``census._run``: launches of
            ``chunk_blocks`` blocks) under HIP events, one warm-up, the median of
            ``--reps``; ``api_s`` is one whole ``census`` call by the wall clock.
  baseline  the top 2^``--baseline-log2`` configurations (the last blocks: the
            nodes above bit 26 all +1, where most of the counted configurations
            live) in pieces of 2^20: numpy builds the +-1 rows, ``pack``,
            ``popcount`` for the weights, T ``rollout`` steps with ``counts=``,
            a histogram of the weights of the rows whose count is n.  Its
            counts must equal the census of the same blocks (asserted).  The
            time of 2^n configurations is EXTRAPOLATED from the sub-range
            (``extrapolated``: true); ``device_s`` leaves the host's row
            building and the upload out.

Rates: configurations/s and config-node-updates/s = configurations * n * T / s.
``bound``: the LDS cycles the layout needs per node and wave (d ds_read_b64 at 2
cycles + 1 ds_write_b64 at 6) turned into config-node-updates/s for the chip,
derived, not measured, and the measured fraction of it.

    python scripts/time_census.py [--reps 7] [--n36] [--out profiles/census_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def rows(lo, hi, n):
    """Configurations lo .. hi-1 as int8 +-1 rows (hi - lo, n), on the host."""
    x = np.arange(lo, hi, dtype="<u8")
    bits = np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")[:, :n]
    return (2 * bits.astype(np.int8) - 1)


def baseline(mjx, g, n, T, lo, hi, piece=1 << 20):
    """The census of configurations [lo, hi) through pack / popcount / rollout.
    -> (counts (T+1, n+1), wall seconds, device seconds)."""
    import torch
    counts = torch.zeros((T + 1, n + 1), dtype=torch.int64, device="cuda")
    dev_ms = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for a in range(lo, hi, piece):
        b = min(hi, a + piece)
        S = torch.from_numpy(rows(a, b, n)).cuda()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        R = b - a
        W = (R + 63) // 64
        cur = mjx.pack(S)
        k = mjx.popcount(cur, n, words=W)[:R]
        nxt, cnt = torch.empty_like(cur), torch.zeros(64 * W, dtype=torch.int64, device="cuda")
        for t in range(T + 1):
            if t:
                cnt.zero_()
                mjx.rollout(g, cur, 1, words=W, out=nxt, counts=cnt)
                cur, nxt = nxt, cur
                plus = cnt[:R]
            else:
                plus = k
            counts[t] += torch.bincount(k[plus == n], minlength=n + 1)
        e1.record()
        e1.synchronize()
        dev_ms += e0.elapsed_time(e1)
    torch.cuda.synchronize()
    return counts.cpu().numpy(), time.perf_counter() - t0, dev_ms / 1e3


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--p", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline-log2", type=int, default=26)
    ap.add_argument("--n36", action="store_true", help="also d = 3 at n = 36 (one timed run)")
    ap.add_argument("--grids", type=int, nargs="*", default=[], help="also time these forced grids (0 = the library's)")
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "census_timing.json"))
    a = ap.parse_args(argv)
    import torch
    import mjx
    import importlib
    cs = importlib.import_module("mjx.census")
    n, p, c, T = a.n, a.p, 1, a.p
    res = {"n": n, "p": p, "c": c, "T": T, "configs": 1 << n, "chunk_blocks": cs.CHUNK_BLOCKS, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "cases": []}
    for d in (3, 4):
        adj = mjx.random_regular_graph(d, n, seed=1)
        g = mjx.Graph.ell(adj)
        B = 1 << (n - 6)
        t0 = time.perf_counter()
        out = mjx.census(g, p, c)
        api_s = time.perf_counter() - t0
        ms, all_ms = median_ms(lambda: cs._run(g, p, c, 0, B, cs.CHUNK_BLOCKS, 0), a.reps)
        upd = (1 << n) * n * T
        # the layout's LDS cycles per node and wave: d reads of 2 cycles, one write of 6 (one LDS per CU, a
        # wave-instruction serves 64 blocks of 64 configurations)
        cyc = 2 * d + 6
        bound = a.cus * a.clock_ghz * 1e9 / cyc * 64 * 64
        case = {"d": d, "graph_seed": 1, "min_plus": out["min_plus"].tolist(), "m_min": out["m_min"].tolist(),
                "reached": out["counts"].sum(axis=1).tolist(), "device_ms": round(ms, 3), "device_ms_all": all_ms,
                "api_s": round(api_s, 4), "configs_per_s": (1 << n) / (ms / 1e3),
                "config_node_updates_per_s": upd / (ms / 1e3),
                "bound": {"derived": True, "lds_cycles_per_node_and_wave": cyc, "cus": a.cus,
                          "clock_ghz": a.clock_ghz, "config_node_updates_per_s": bound,
                          "measured_fraction": upd / (ms / 1e3) / bound}}
        if a.grids:
            case["grid_sweep_ms"] = {str(gr): round(median_ms(lambda: cs._run(g, p, c, 0, B, cs.CHUNK_BLOCKS, gr), 3)[0], 3)
                                     for gr in a.grids}
        # the baseline on the top sub-range, checked against the census of the same blocks
        sub = min(1 << a.baseline_log2, 1 << n)
        lo = (1 << n) - sub
        want, _ = cs._run(g, p, c, lo // 64, B, cs.CHUNK_BLOCKS, 0)
        got, wall_s, dev_s = baseline(mjx, g, n, T, lo, 1 << n)
        assert np.array_equal(got, want.cpu().numpy()), "baseline and census disagree on the sub-range"
        scale = (1 << n) / sub
        case["baseline"] = {"configs": sub, "counted": int(got[T].sum()), "wall_s": round(wall_s, 4),
                            "device_s": round(dev_s, 4), "extrapolated": True,
                            "wall_s_full": wall_s * scale, "device_s_full": dev_s * scale,
                            "configs_per_s": sub / wall_s, "configs_per_s_device": sub / dev_s}
        case["speedup_vs_baseline_wall"] = wall_s * scale / (ms / 1e3)
        case["speedup_vs_baseline_device"] = dev_s * scale / (ms / 1e3)
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    if a.n36:
        adj = mjx.random_regular_graph(3, 36, seed=1)
        t0 = time.perf_counter()
        out = mjx.census(adj, p, c)
        s = time.perf_counter() - t0
        res["n36"] = {"d": 3, "api_s": round(s, 3), "min_plus": out["min_plus"].tolist(),
                      "configs_per_s": (1 << 36) / s, "config_node_updates_per_s": (1 << 36) * 36 * T / s}
        print(json.dumps(res["n36"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out, "device_ms": [k["device_ms"] for k in res["cases"]]}))


if __name__ == "__main__":
    main()
