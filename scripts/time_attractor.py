"""Time the tracked replica-packed sweep against the counting sweep, and the
run to the attractor end to end, and print ONE JSON line.

Workload: a d-regular random graph of N nodes from the device generator, R
replicas of random starts at magnetisation m_init (``random_spins``).

  counting  one ``rollout(g, a, 1, words=W, out=b, counts=cnt)`` per sweep,
            ping-ponging two buffers: the sweep with the fused +1 counts.
  tracked   one ``mjx_sweep_track_ell_rp`` per sweep with the same counts and
            the two flag halves, s_out aliasing s_prev (the ping-pong case).
  attractor ``attractor(g, bits, t_max, chunk, words=W)``: tracked sweeps, the
            bookkeeping kernel after each, one host read per chunk.

Timing: HIP events around ``--sweeps`` back-to-back sweeps (the count and flag
buffers are zeroed outside the timed region), one warm-up call, the median of
``--reps`` calls.  Byte model of a sweep per node and 8*W-byte row: d gathered
rows + own + written (+ the streamed s_prev row when tracked) + 4*d index
bytes, so tracked / counting = (d + 3) / (d + 2) for wide rows.

    python scripts/time_attractor.py [--n 1000000] [--d 4] [--replicas 4096] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, reps, before=None):
    import torch
    fn()                                    # warm-up (first launch, occupancy query, allocator)
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
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=4)
    ap.add_argument("--replicas", type=int, default=4096)
    ap.add_argument("--m-init", type=float, default=0.0)
    ap.add_argument("--sweeps", type=int, default=20, help="sweeps per timed call")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--t-max", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import mjx
    from mjx import _device as D, _lib as L

    n, d, R, K = a.n, a.d, a.replicas, a.sweeps
    W = D.words_for(R)
    g = mjx.random_regular_graph_device(d, n, seed=1)
    bits = mjx.random_spins(n, R, a.m_init, seed=1)
    st = D.stream_handle()
    row = 8 * W
    res = {"workload": {"n": n, "d": d, "replicas": R, "words": W, "m_init": a.m_init, "sweeps_per_call": K,
                        "reps": a.reps}, "device": torch.cuda.get_device_name(0)}

    bufs = [bits.clone(), torch.empty_like(bits)]
    cnts = torch.zeros((K, 64 * W), dtype=torch.int64, device="cuda")
    diffs = torch.zeros((K, 2 * W), dtype=torch.int64, device="cuda")

    def zero():
        cnts.zero_()
        diffs.zero_()

    def counting():
        for k in range(K):
            mjx.rollout(g, bufs[k & 1], 1, words=W, out=bufs[(k + 1) & 1], counts=cnts[k])

    def tracked():
        # sweep k reads bufs[k & 1] and writes s(k+1) over s(k-1) in the other buffer
        for k in range(K):
            prev = bufs[(k + 1) & 1]
            L.call("mjx_sweep_track_ell_rp", D.ptr(g.adj), n, d, W, D.ptr(bufs[k & 1]), D.ptr(prev), D.ptr(prev),
                   D.ptr(cnts[k]), D.ptr(diffs[k]), st)

    ms_c, all_c = median_ms(counting, a.reps, zero)
    bufs[0].copy_(bits)
    ms_t, all_t = median_ms(tracked, a.reps, zero)
    bytes_c = n * ((d + 2) * row + 4 * d)
    bytes_t = n * ((d + 3) * row + 4 * d)
    res["counting"] = {"ms_per_sweep": ms_c / K, "calls_ms": all_c, "model_bytes": bytes_c,
                       "model_TBps": bytes_c / (ms_c / K * 1e-3) / 1e12}
    res["tracked"] = {"ms_per_sweep": ms_t / K, "calls_ms": all_t, "model_bytes": bytes_t,
                      "model_TBps": bytes_t / (ms_t / K * 1e-3) / 1e12}
    res["ratio"] = ms_t / ms_c
    res["model_ratio"] = bytes_t / bytes_c
    del bufs, cnts, diffs
    torch.cuda.empty_cache()

    runs = []
    for _ in range(max(2, a.reps // 2)):     # the first run is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = mjx.attractor(g, bits, t_max=a.t_max, chunk=a.chunk, words=W)
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
    sec = float(np.median(runs[1:]))
    p = out["p"].cpu().numpy()[:R]
    c = out["c"].cpu().numpy()[:R]
    res["attractor"] = {"seconds": sec, "runs_s": [round(x, 5) for x in runs], "t_end": out["t_end"],
                        "ms_per_sweep": 1e3 * sec / out["t_end"],
                        "replica_sweeps_per_s": R * out["t_end"] / sec,
                        "max_p": int(p.max()), "unsettled": int((p < 0).sum()),
                        "c1": int((c == 1).sum()), "c2": int((c == 2).sum())}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
