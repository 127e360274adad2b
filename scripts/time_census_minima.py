"""Time the census of the minimal consensus sets (``census_minima``,
csrc/mjx_census.hip) on d = 3 and d = 4 random regular graphs at n = 32,
T = p + c - 1 = 3, the shapes of scripts/time_census.py.  HIP events, one
warm-up, the median of ``--reps``.

  pass 1    the census that keeps its bits (mjx_census_mask_ell) against
            ``census`` of the same build and, with ``--parent-lib``, against
            ``census`` of another build of the library (the parent commit's),
            all run in turns in one process; ``mask_over_census`` is the ratio.
  pass 2    mjx_census_minima over the whole bitmap: the time, its rate in the
            bytes of the byte model (derived, not measured: per level at most
            2^(n-3) (1 + (n-12)/2) bytes) and the share of waves whose 64 words
            are all zero at a level (they read nothing more).
  baseline  what a user had before: the counted configurations of the top
            ``--baseline-log2`` configurations are unpacked to +-1 rows and
            ``flip_gains(..., gain=False)`` is asked for an empty removable
            mask.  Its minima by weight must equal pass 2 on the same blocks
            (asserted); the time per counted configuration is EXTRAPOLATED to
            all of U_T and labelled so.

    python scripts/time_census_minima.py [--reps 7] [--parent-lib FILE] [--out profiles/census_minima_timing.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def in_turns(fns, reps):
    """name -> fn, run one after the other ``reps`` times after one warm-up each, every turn starting with
    another of them -> name -> (median, all)."""
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    names = list(fns)
    for r in range(reps):
        for k in names[r % len(names):] + names[:r % len(names)]:
            out[k].append(timed_ms(fns[k]))
    return {k: (float(np.median(v)), [round(x, 3) for x in v]) for k, v in out.items()}


def spins_of(x, n):
    """Configuration indices -> int8 +-1 rows (len(x), n), on the host."""
    bits = np.unpackbits(np.ascontiguousarray(x, dtype="<u8").view(np.uint8).reshape(-1, 8), axis=1,
                         bitorder="little")[:, :n]
    return 2 * bits.astype(np.int8) - 1


def members(words, first_block):
    """The configurations whose bit is set in ``words`` (uint64, blocks first_block ..), ascending."""
    bits = np.unpackbits(words.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little").reshape(-1)
    return (np.flatnonzero(bits) + 64 * first_block).astype(np.uint64)


def baseline(mjx, g, n, p, c, x, piece=1 << 19):
    """The minima among the configurations x by weight, through flip_gains -> (minima (n+1,), wall seconds)."""
    import torch
    minima = np.zeros(n + 1, np.int64)
    mjx.flip_gains(g, spins_of(x[:64], n), p, c, gain=False, validate=False)     # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for a in range(0, x.size, piece):
        S = spins_of(x[a:a + piece], n)
        fg = mjx.flip_gains(g, S, p, c, gain=False, validate=False)
        least = np.asarray(fg["consensus"]) & (np.asarray(fg["n_removable"]) == 0)
        minima += np.bincount((S[least] == 1).sum(axis=1), minlength=n + 1)
    torch.cuda.synchronize()
    return minima, time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--p", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline-log2", type=int, default=24)
    ap.add_argument("--parent-lib", default=None, help="a libmjx.so built from the parent commit: its census is timed "
                                                       "in turns with this build's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "census_minima_timing.json"))
    a = ap.parse_args(argv)
    import torch
    import mjx
    cs = importlib.import_module("mjx.census")
    lib_mod = importlib.import_module("mjx._lib")
    dev_mod = importlib.import_module("mjx._device")
    n, p, c, T = a.n, a.p, 1, a.p
    B = 1 << (n - 6)
    parent = lib_mod.open_library(a.parent_lib, verify=False) if a.parent_lib else None
    model = (T + 1) * (1 << (n - 3)) * (1 + (n - 12) / 2)
    res = {"n": n, "p": p, "c": c, "T": T, "configs": 1 << n, "chunk_blocks": cs.CHUNK_BLOCKS, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "mask_bytes": (T + 1) * B * 8,
           "byte_model": {"derived": True, "bytes_all_levels": model}, "parent_lib": bool(parent), "cases": []}
    for d in (3, 4):
        adj = mjx.random_regular_graph(d, n, seed=1)
        g = mjx.Graph.ell(adj)
        t0 = time.perf_counter()
        out = mjx.census_minima(g, p, c, return_mask=True)
        api_s = time.perf_counter() - t0
        mask = out.pop("mask")
        cen = mjx.census(g, p, c)
        assert all(np.array_equal(out[k], cen[k]) for k in cen), "census_minima and census disagree"

        def parent_census():
            counts = torch.zeros((T + 1, n + 1), dtype=torch.int64, device="cuda")
            keys = torch.full((T + 1,), -1, dtype=torch.int64, device="cuda")
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")
            for lo in range(0, B, cs.CHUNK_BLOCKS):
                rc = parent.mjx_census_ell(g.adj.data_ptr(), n, d, p, c, lo, min(B, lo + cs.CHUNK_BLOCKS), 0,
                                           counts.data_ptr(), keys.data_ptr(), flag.data_ptr(),
                                           dev_mod.stream_handle())
                assert rc == 0
            return counts

        fns = {"census": lambda: cs._run(g, p, c, 0, B, cs.CHUNK_BLOCKS, 0),
               "mask": lambda: cs._run(g, p, c, 0, B, cs.CHUNK_BLOCKS, 0, mask=mask)}
        if parent:
            assert np.array_equal(parent_census().cpu().numpy(), cen["counts"]), "the parent's census differs"
            fns["census_parent"] = parent_census
        turns = in_turns(fns, a.reps)

        minima = torch.zeros((T + 1, n + 1), dtype=torch.int64, device="cuda")
        heavy = torch.zeros((T + 1,), dtype=torch.int64, device="cuda")

        def pass2(lo=0):
            for b0 in range(lo, B, cs.CHUNK_BLOCKS):
                lib_mod.call("mjx_census_minima", mask.data_ptr(), n, T, b0, min(B, b0 + cs.CHUNK_BLOCKS), 0,
                             minima.data_ptr(), heavy.data_ptr(), dev_mod.stream_handle())

        p2 = in_turns({"minima": pass2}, a.reps)["minima"]
        skipped = [1.0 - float(mask[t].view(B // 64, 64).ne(0).any(dim=1).float().mean()) for t in range(T + 1)]
        k_opt = int(out["min_plus"][T])
        case = {"d": d, "graph_seed": 1, "api_s": round(api_s, 4), "min_plus": out["min_plus"].tolist(),
                "max_plus": out["max_plus"].tolist(), "mean_plus": out["mean_plus"].tolist(),
                "minima_total": out["minima_total"].tolist(),
                "minima_T": {str(k): int(v) for k, v in enumerate(out["minima"][T]) if v},
                "optimal_share_T": float(out["minima"][T, k_opt] / out["minima_total"][T]),
                "reached_T": int(out["counts"][T].sum()),
                "census_ms": round(turns["census"][0], 3), "census_ms_all": turns["census"][1],
                "mask_ms": round(turns["mask"][0], 3), "mask_ms_all": turns["mask"][1],
                "mask_over_census": turns["mask"][0] / turns["census"][0],
                "minima_ms": round(p2[0], 3), "minima_ms_all": p2[1],
                "minima_model_bytes_per_s": model / (p2[0] / 1e3), "waves_skipped_share": skipped,
                "both_passes_ms": round(turns["mask"][0] + p2[0], 3)}
        if parent:
            case.update(census_parent_ms=round(turns["census_parent"][0], 3),
                        census_parent_ms_all=turns["census_parent"][1],
                        census_over_parent=turns["census"][0] / turns["census_parent"][0])
        # the baseline on the counted configurations of the top blocks, against pass 2 on the same blocks
        sub_blocks = max(64, min(B, (1 << a.baseline_log2) // 64))
        lo = B - sub_blocks
        x = members(mask[T, lo:].cpu().numpy().view(np.uint64), lo)
        minima.zero_()
        pass2(lo)
        want = minima[T].cpu().numpy()
        got, wall_s = baseline(mjx, g, n, p, c, x)
        assert np.array_equal(got, want), "baseline and pass 2 disagree on the sub-range"
        full = wall_s / x.size * case["reached_T"]
        case["baseline"] = {"blocks": sub_blocks, "counted": int(x.size), "minima": int(got.sum()),
                            "wall_s": round(wall_s, 4), "extrapolated": True, "wall_s_all_of_U_T": full,
                            "over_both_passes": full / ((turns["mask"][0] + p2[0]) / 1e3)}
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        del mask, out
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out, "mask_ms": [k["mask_ms"] for k in res["cases"]],
                      "minima_ms": [k["minima_ms"] for k in res["cases"]]}))


if __name__ == "__main__":
    main()
