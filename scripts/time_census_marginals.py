"""Time the census marginals (``census_marginals``, csrc/mjx_census.hip) on
d = 3 and d = 4 random regular graphs at n = 32, T = p + c - 1 = 3, the shapes
of scripts/time_census.py.  HIP events, one warm-up, the median of ``--reps``.

  marginals  the census that also counts level T per node
             (mjx_census_nodes_ell) against ``census`` of the same build and,
             with ``--parent-lib``, against ``census`` of another build of the
             library (the parent commit's), all run in turns in one process;
             ``marginals_over_census`` and ``census_over_parent`` are the ratios.
  baseline   the same node counts without the kernel: the bitmap of
             ``census_minima(..., return_mask=True)`` reduced per node and
             weight with torch ops on the top ``--baseline-log2``
             configurations.  They must equal the kernel's on the same blocks
             (asserted); the time is EXTRAPOLATED to all 2^n and labelled so
             (the bitmap pass itself, ``mask_ms``, is not part of it).

    python scripts/time_census_marginals.py [--reps 7] [--parent-lib FILE] [--out profiles/census_marginals_timing.json]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from time_census_minima import in_turns, timed_ms          # noqa: E402


def node_counts_torch(words, first_block, n, piece=1 << 14):
    """node_counts (n+1, n) of the configurations whose bit is set in ``words`` (device int64, the blocks
    first_block ..), by torch ops: the bits unpacked to (blocks, 64), their weights, one bincount per node."""
    import torch
    dev = words.device
    j = torch.arange(64, device=dev)
    kj = sum((j >> i) & 1 for i in range(6))                                 # weight of the low six bits
    out = torch.zeros((n + 1, n), dtype=torch.int64, device=dev)
    for a in range(0, words.numel(), piece):
        w = words[a:a + piece]
        b = torch.arange(first_block + a, first_block + a + w.numel(), device=dev)
        member = ((w[:, None] >> j[None, :]) & 1).bool()                     # (blocks, 64)
        kb = sum((b >> i) & 1 for i in range(max(n - 6, 0)))
        k = kb[:, None] + kj[None, :]
        for v in range(n):
            up = ((j >> v) & 1).bool()[None, :] if v < 6 else ((b >> (v - 6)) & 1).bool()[:, None]
            out[:, v] += torch.bincount(k[member & up], minlength=n + 1)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--p", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline-log2", type=int, default=26)
    ap.add_argument("--parent-lib", default=None, help="a libmjx.so built from the parent commit: its census is timed "
                                                       "in turns with this build's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "census_marginals_timing.json"))
    a = ap.parse_args(argv)
    import torch
    import mjx
    cs = importlib.import_module("mjx.census")
    lib_mod = importlib.import_module("mjx._lib")
    dev_mod = importlib.import_module("mjx._device")
    n, p, c, T = a.n, a.p, 1, a.p
    B = 1 << (n - 6)
    parent = lib_mod.open_library(a.parent_lib, verify=False) if a.parent_lib else None
    res = {"n": n, "p": p, "c": c, "T": T, "t_node": T, "configs": 1 << n, "chunk_blocks": cs.CHUNK_BLOCKS,
           "reps": a.reps, "device": torch.cuda.get_device_name(0), "lds_bytes": cs.census_nodes_lds(n),
           "census_lds_bytes": int(lib_mod.load().mjx_census_lds(n)), "parent_lib": bool(parent), "cases": []}
    for d in (3, 4):
        adj = mjx.random_regular_graph(d, n, seed=1)
        g = mjx.Graph.ell(adj)
        out = mjx.census_marginals(g, p, c)
        cen = mjx.census(g, p, c)
        assert all(np.array_equal(out[k], cen[k]) for k in cen), "census_marginals and census disagree"
        assert np.array_equal(out["node_counts"][0].sum(axis=1), cen["counts"][T] * np.arange(n + 1))

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
               "marginals": lambda: cs._run_nodes(g, p, c, T, 0, B, cs.CHUNK_BLOCKS, 0)}
        if parent:
            assert np.array_equal(parent_census().cpu().numpy(), cen["counts"]), "the parent's census differs"
            fns["census_parent"] = parent_census
        turns = in_turns(fns, a.reps)
        k_opt = int(out["min_plus"][T])
        case = {"d": d, "graph_seed": 1, "min_plus": out["min_plus"].tolist(), "optimal_T": int(out["optimal"][0]),
                "backbone_plus_T": int(out["backbone_plus"][0].sum()),
                "backbone_minus_T": int(out["backbone_minus"][0].sum()),
                "node_counts_at_optimum_T": out["node_counts"][0, k_opt].tolist(),
                "reached_T": int(out["counts"][T].sum()),
                "census_ms": round(turns["census"][0], 3), "census_ms_all": turns["census"][1],
                "marginals_ms": round(turns["marginals"][0], 3), "marginals_ms_all": turns["marginals"][1],
                "marginals_over_census": turns["marginals"][0] / turns["census"][0]}
        if parent:
            case.update(census_parent_ms=round(turns["census_parent"][0], 3),
                        census_parent_ms_all=turns["census_parent"][1],
                        census_over_parent=turns["census"][0] / turns["census_parent"][0])
        # the baseline: level T of the bitmap on the top blocks, against the kernel on the same blocks
        sub_blocks = max(64, min(B, (1 << a.baseline_log2) // 64))
        lo = B - sub_blocks
        mask = torch.empty((T + 1, B), dtype=torch.int64, device="cuda")
        mask_ms = timed_ms(lambda: cs._run(g, p, c, 0, B, cs.CHUNK_BLOCKS, 0, mask=mask))
        words = mask[T, lo:].clone()
        del mask
        want = cs._run_nodes(g, p, c, T, lo, B, cs.CHUNK_BLOCKS, 0)[2].cpu().numpy()
        node_counts_torch(words[:1024], lo, n)                               # warm-up
        got = [None]

        def torch_baseline():
            got[0] = node_counts_torch(words, lo, n)

        base_ms = timed_ms(torch_baseline)
        assert np.array_equal(got[0].cpu().numpy(), want), "the torch baseline and the kernel disagree on the sub-range"
        full_ms = base_ms * (B / sub_blocks)
        case["baseline"] = {"blocks": sub_blocks, "configs": 64 * sub_blocks, "ms": round(base_ms, 3),
                            "extrapolated": True, "ms_all_configs": full_ms, "mask_ms": round(mask_ms, 3),
                            "over_marginals": full_ms / turns["marginals"][0]}
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out, "census_ms": [k["census_ms"] for k in res["cases"]],
                      "marginals_ms": [k["marginals_ms"] for k in res["cases"]]}))


if __name__ == "__main__":
    main()
