"""Time HPR on G graphs as one union (``HPRBatch``) against the same G graphs one
after the other through the single-graph ``HPRState`` graph-replay path, and
print ONE JSON line.

Workload (code/HPR_pytorch_RRG.py's own size, :224-237): random 4-regular
graphs on n = 10 000 nodes, p = c = 1, fp32, batches of 16 iterations replayed
as a hipGraph, the per-iteration rand(n) continued on the device on a side
stream one batch ahead -- in both paths.  Every run makes a fixed number of
iterations (512) of every instance whatever its consensus test says (the loop
is not stopped and the union is never compacted), so both paths do the same
work; both start from the same messages, biases and generator states, and the
messages they end with are compared bit for bit.

Timing: per G one warm-up run of each path (graph capture, jump tables,
allocator), then ``--reps`` timed runs of each, the two paths alternating, the
host clock around a run that begins after a device synchronise and ends in
one.  Reported per path: median and min/max of the runs and
instance-iterations per second from the median; per G the ratio sequential /
batch and whether the gap exceeds the spread (the slowest batch run is faster
than the fastest sequential run).

    python scripts/time_hpr_batch.py [--sizes 1 8 32 128] [--iters 512] [--reps 3] [--out file.json]
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
            "max_s": float(max(runs)), "instance_iterations_per_s": work / med}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=10_000)
    ap.add_argument("--d", type=int, default=4)
    ap.add_argument("--p", type=int, default=1)
    ap.add_argument("--c", type=int, default=1)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--iters", type=int, default=512, help="iterations per instance and run")
    ap.add_argument("--batch", type=int, default=16, help="iterations per captured graph")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.reps < 3:
        ap.error("--reps must be at least 3")
    if a.batch % 2 or a.iters % a.batch:
        ap.error("--batch must be even and divide --iters")
    import torch
    import mjx

    n, d, p, c, B, nb = a.n, a.d, a.p, a.c, a.batch, a.iters // a.batch
    dtype, never = torch.float32, 10 ** 12
    E, nc = n * d // 2, 4 ** (p + c)
    edges, chi0, b0, gstate = [], [], [], []
    for g in range(max(a.sizes)):
        edges.append(mjx.random_regular_edges(d, n, seed=1000 + g))
        gen = torch.Generator().manual_seed(2000 + g)
        x = torch.rand((2 * E, nc), dtype=torch.float64, generator=gen)
        chi0.append(x / x.sum(1, keepdim=True))
        b = torch.rand((n, 2), dtype=torch.float64, generator=gen)
        b0.append(b / b.sum(1, keepdim=True))
        gstate.append(gen.get_state())

    def gens(G):
        out = []
        for g in range(G):
            gen = torch.Generator()
            gen.set_state(gstate[g])
            out.append(gen)
        return out

    res = {"workload": {"n": n, "d": d, "p": p, "c": c, "dtype": "float32", "iterations_per_run": a.iters,
                        "iterations_per_graph_replay": B, "reps": a.reps, "rows_per_instance": 2 * E,
                        "message_bytes_per_instance": 2 * E * nc * 4},
           "device": torch.cuda.get_device_name(0), "sizes": {}}

    for G in a.sizes:
        hb = mjx.HPRBatch(d, n, p, c, edges[:G], chi0[:G], b0[:G], gens(G), dtype=dtype, TT=never, batch=B,
                          compact=0.0)
        seq = []
        for g, gen in enumerate(gens(G)):
            st = mjx.HPRState(mjx.HPRPlan(edges[g], n, d), p, c, chi0[g], b0[g], dtype=dtype)
            st._batch_buffers(B)
            st.rng_attach(gen)
            seq.append([st, st.draw_batch_device(B)])

        def run_batch():
            hb.run(max_batches=nb, stop=False)

        def run_seq():
            # hpr_run's loop without its stop: launch, draw the next batch beside it, one host read
            for item in seq:
                st = item[0]
                for _ in range(nb):
                    st.launch_batch(item[1])
                    item[1] = st.draw_batch_device(B, st.t)
                    st.collect_batch()

        run_batch()
        run_seq()
        tb, ts = [], []
        for _ in range(a.reps):
            tb.append(timed(run_batch))
            ts.append(timed(run_seq))
        # both paths made the same iterations from the same start: the same bits
        assert hb.st.t == seq[0][0].t == (1 + a.reps) * a.iters
        un, Et = hb.st.messages(), G * E
        same = all(torch.equal(torch.cat([un[g * E:(g + 1) * E], un[Et + g * E:Et + (g + 1) * E]]),
                               item[0].messages()) for g, item in enumerate(seq))
        sb, ss = stats(tb, G * a.iters), stats(ts, G * a.iters)
        res["sizes"][str(G)] = {"batch": sb, "sequential": ss,
                                "ratio_sequential_over_batch": ss["median_s"] / sb["median_s"],
                                "gap_exceeds_spread": bool(sb["max_s"] < ss["min_s"]), "same_messages": bool(same),
                                "layout": hb.st.layout, "union_rows": 2 * Et,
                                "instances_past_their_consensus_test": int(G - hb.live),
                                "batch_iteration_us": 1e6 * sb["median_s"] / a.iters,
                                "sequential_iteration_us": 1e6 * ss["median_s"] / (G * a.iters)}
        print(f"G={G}: batch {sb['median_s']:.4f} s, sequential {ss['median_s']:.4f} s", file=sys.stderr, flush=True)
        del hb, seq, un
        torch.cuda.synchronize()
        torch.cuda.empty_cache()

    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
