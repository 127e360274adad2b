"""Script-shaped fronts: ``python -m mjx sa|sa-er|hpr|bdcm|attractor|quench|census|attractor-census`` run the reference's three
experiments with its module constants as flags -- same names, same defaults --
and write its np.savez keys.

  sa    code/SA_RRG.py:44-52 (n, d, p, c, par_a, par_b, N_stat), loop :58-88,
        output :92 ("MCMC_p{p}_d{d}.npz": mag_reached, num_steps, conf, graphs)
  sa-er the same SA loop on one Erdos-Renyi graph (n, deg = mean degree, p, c,
        par_a, par_b, N_stat), scored with the notebook's ER end state
        (nb:113-123); output "SA_ER_p{p}.npz": mag_reached, num_steps, conf,
        done, near_ties, wall_s, row_ptr, col, n_iso
  hpr   code/HPR_pytorch_RRG.py:224-237 (n, d, p, c, damppar, attr_value,
        lmbd_in, pie, gamma, TT) and :251 (n_rep), output :377
        ("hpr_d{d}_p{p}.npz": mag_reached, conf, num_steps, graphs, time);
        ``--batch B`` runs the replicas B at a time as one union graph
        (hpr_batch.hpr_run_batch), the same arrays
  bdcm  code/ER_BDCM_entropy.ipynb raw lines 456-481 (n, deg, num_rep, p, c,
        eps, damppar, attr_value, epsilon, T_max, a, dl), output :515
        ("ER_p{p}.npz": m_init, ent1, ent, ... T_max, num_rep)
  attractor  no reference script: the random-initialisation baseline
        (attractor.consensus_curve) on one random regular or Erdos-Renyi
        graph; output "attractor_{graph}.npz": m_init, consensus, c1, c2,
        unsettled, p, c, sum_att, init_plus
  quench  no reference script: the greedy zero-temperature clean-up
        (quench.quench) of the ``conf`` of an SA / HPR result file (``graphs``:
        one graph per replica, run replica by replica) or an sa-er file
        (``row_ptr``, ``col``: one call); output: the input's arrays plus
        conf_quenched, mag_quenched, flipped, consensus.  ``--restarts K``
        (with ``--order-seed``): best of K orders per replica, all (replica,
        order) jobs in one call (quench.quench_restarts), a graph per replica
        for ``graphs`` files; the same keys for the best restart plus
        mag_restarts (R, K) and best.  ``--exchange [--max-passes P]`` (with
        ``--restarts K``): the (1, 2) exchange descent behind every job's pass
        (quench.quench_exchange); adds mag_quench, exchanges, passes, converged
        (R, K).  ``--anneal SWEEPS [--beta B0 B1] [--anneal-seed A]`` (with
        ``--restarts K``): Metropolis add / drop sweeps inside the consensus
        set behind every job's pass (quench.quench_anneal); adds mag_quench,
        mag_best_sweep, best_sweep, adds, drops, refused (R, K).
        ``--schedule regions [--window K]``:
        the single pass in rounds (same output; quench.quench's schedule)
  census  no reference script: the exact consensus census (census.census) of
        one small random regular or Erdos-Renyi graph (n <= 48, isolated nodes
        kept), every one of the 2^n starts run p + c - 1 steps; output
        "census_{graph}.npz": counts, min_plus, m_min, witness, entropy,
        configs, edges.  ``--minima`` adds the census of the minimal consensus
        sets, the local minima of the quenches (census.census_minima): minima,
        minima_total, max_plus, m_max, witness_max, mean_plus.
        ``--marginals [--levels T ...] [--lam L ...]`` counts the levels per
        +1 node instead (census.census_marginals): levels, node_counts, optimal,
        backbone_plus, backbone_minus and, with ``--lam``, the exact Boltzmann
        averages of every level and lambda (census.census_boltzmann): lam,
        phi, m_init, ent1 (levels, lambdas), p_plus, m_node (levels, lambdas, n)
  attractor-census  no reference script: the attractor census
        (census.attractor_census) of one such graph, every one of the 2^n
        starts run until s(t+2) = s(t) (at most t_max + 2 steps); output
        "attractor_census_{graph}.npz": hist, unsettled, configs, classes,
        reach_plus, p_plus, min_plus_ever, m_min_ever, witness_plus, p_longest,
        witness_longest, mean_sweeps, edges

Added beside the reference's constants: ``--seed`` (the reference seeds
nothing), ``--graph-seed``, ``--replicas`` (N_stat / n_rep / num_rep by
another name), ``--gpus`` (replicas spread over that many devices of this
node: independent SA streams, HPR replicas), ``--out``.  Graphs are this
package's own random regular / Erdos-Renyi generators (the reference uses
networkx with seed=None: the dynamics depend only on the edge set).
"""
import argparse
import sys
import time

import numpy as np

# the reference's module constants (name -> default), cited line by line
SA_DEFAULTS = {            # code/SA_RRG.py
    "n": 10000,            # :44
    "d": 4,                # :45
    "p": 3,                # :46
    "c": 1,                # :47
    "par_a": 1.0005,       # :49
    "par_b": 1.0005,       # :50
    "N_stat": 5,           # :52
}
SA_ER_DEFAULTS = {         # code/SA_RRG.py's constants on the notebook's graph (nb:456-459)
    "n": 1000,             # nb:456
    "deg": 2.0,            # nb:459 (one mean degree; prob = deg/(n-1), nb:280)
    "p": 1,                # nb:466
    "c": 1,                # nb:467
    "par_a": 1.0005,       # code/SA_RRG.py:49
    "par_b": 1.0005,       # :50
    "N_stat": 5,           # :52
}
HPR_DEFAULTS = {           # code/HPR_pytorch_RRG.py
    "n": 10000,            # :224
    "d": 4,                # :225
    "p": 1,                # :226
    "c": 1,                # :227
    "damppar": 0.4,        # :229
    "attr_value": 1,       # :230
    "lmbd_in": None,       # :231  (25*n)
    "pie": 0.3,            # :235
    "gamma": 0.1,          # :236
    "TT": 10000,           # :237
    "n_rep": 1,            # :251
}
BDCM_DEFAULTS = {          # code/ER_BDCM_entropy.ipynb (raw JSON lines)
    "n": 1000,             # nb:456
    "deg": [1.0, 1.5, 2.0],  # nb:459 np.linspace(1,2,3)
    "num_rep": 3,          # nb:463
    "p": 1,                # nb:466
    "c": 1,                # nb:467
    "eps": 1e-6,           # nb:470
    "damppar": 0.1,        # nb:471
    "attr_value": 1,       # nb:472
    "epsilon": 0.0,        # nb:473
    "T_max": 1300,         # nb:478
    "a": 12,               # nb:480
    "dl": 0.1,             # nb:481
}


def _common(ap):
    ap.add_argument("--seed", type=int, default=0, help="numpy / torch seed (the reference seeds nothing)")
    ap.add_argument("--graph-seed", type=int, default=None, help="seed of the first replica's graph (+k for replica k)")
    ap.add_argument("--replicas", type=int, default=None, help="replica count (overrides N_stat / n_rep / num_rep)")
    ap.add_argument("--gpus", type=int, default=1, help="devices of this node to spread the replicas over")
    ap.add_argument("--out", default=None, help="output .npz (default: the reference's file name)")


class _Parser(argparse.ArgumentParser):
    """Checks that span two options, after the parse."""

    def parse_args(self, args=None, namespace=None):
        a = super().parse_args(args, namespace)
        if a.cmd == "quench":
            if a.restarts < 0:
                self.error("--restarts must be >= 0")
            if a.restarts >= 1 and a.order_seed is None:
                self.error("--restarts K needs --order-seed: the K orders are drawn from it")
            if a.window is not None and (a.schedule != "regions" or a.window < 1):
                self.error("--window K (K >= 1) belongs to --schedule regions")
            if a.schedule == "regions" and a.restarts >= 1:
                self.error("--schedule regions is a schedule of the single pass: not with --restarts")
            if a.exchange and a.restarts < 1:
                self.error("--exchange runs behind the jobs of --restarts K --order-seed S (K >= 1)")
            if a.exchange and a.schedule == "regions":
                self.error("--schedule regions is a schedule of the single pass: not with --exchange")
            if a.max_passes is not None and (not a.exchange or a.max_passes < 1):
                self.error("--max-passes P (P >= 1) belongs to --exchange")
            if a.anneal is not None:
                if a.anneal < 0:
                    self.error("--anneal SWEEPS must be >= 0")
                if a.restarts < 1:
                    self.error("--anneal runs behind the jobs of --restarts K --order-seed S (K >= 1)")
                if a.exchange:
                    self.error("--anneal and --exchange are two walks behind the same pass: one of them")
                if a.schedule == "regions":
                    self.error("--schedule regions is a schedule of the single pass: not with --anneal")
                if a.anneal_seed is not None and not 0 <= a.anneal_seed < 2 ** 64:
                    self.error("--anneal-seed A: 0 <= A < 2^64")
                if a.beta is not None and (min(a.beta) < 0 or not all(np.isfinite(a.beta))):
                    self.error("--beta B0 B1: finite inverse temperatures >= 0")
            elif a.beta is not None or a.anneal_seed is not None:
                self.error("--beta and --anneal-seed belong to --anneal SWEEPS")
        return a


def build_parser():
    ap = _Parser(prog="python -m mjx", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    sa = sub.add_parser("sa", help="code/SA_RRG.py")
    for k, v in SA_DEFAULTS.items():
        sa.add_argument(f"--{k}", type=type(v), default=v)
    sa.add_argument("--stream", choices=("global", "independent"), default="global",
                    help="global: ONE numpy stream, replicas back to back (the script's own semantics); "
                         "independent: replica k seeded seed+k, all at once")
    sa.add_argument("--max-steps", type=int, default=None, help="proposal cap per replica (the script's is 2n^3)")
    sa.add_argument("--max-seconds", type=float, default=None)
    _common(sa)
    se = sub.add_parser("sa-er", help="code/SA_RRG.py's loop on an Erdos-Renyi graph")
    for k, v in SA_ER_DEFAULTS.items():
        se.add_argument(f"--{k}", type=type(v), default=v)
    se.add_argument("--mode", choices=("auto", "lightcone", "rollout"), default="auto")
    se.add_argument("--keep-isolated", action="store_true",
                    help="keep degree-0 nodes (the notebook drops and relabels them, nb:283-291)")
    se.add_argument("--max-steps", type=int, default=None, help="proposal cap per replica (the script's is 2n^3)")
    se.add_argument("--max-seconds", type=float, default=None)
    _common(se)
    hp = sub.add_parser("hpr", help="code/HPR_pytorch_RRG.py")
    for k, v in HPR_DEFAULTS.items():
        hp.add_argument(f"--{k}", type=(int if k == "lmbd_in" else type(v)), default=v)
    hp.add_argument("--dtype", choices=("float32", "float64"), default="float32",
                    help="message precision (the reference's is float64, :11)")
    hp.add_argument("--batch", type=int, default=0,
                    help="run that many replicas at a time as one union graph (0: one after the other); same output")
    _common(hp)
    bd = sub.add_parser("bdcm", help="code/ER_BDCM_entropy.ipynb")
    for k, v in BDCM_DEFAULTS.items():
        if k == "deg":
            bd.add_argument("--deg", type=float, nargs="+", default=list(v))
        else:        # a (the lambda range's end) may be given as a float too
            bd.add_argument(f"--{k}", type=float if k == "a" else type(v), default=v)
    bd.add_argument("--batch", type=int, default=0,
                    help="run that many graphs at a time as one union graph (0: one after the other); same output")
    _common(bd)
    at = sub.add_parser("attractor", help="random starts run to their attractors (no reference script)")
    at.add_argument("--graph", choices=("rrg", "er"), default="rrg")
    at.add_argument("--n", type=int, default=10000)
    at.add_argument("--d", type=int, default=4, help="degree (rrg)")
    at.add_argument("--deg", type=float, default=2.0, help="mean degree (er; prob = deg/(n-1))")
    at.add_argument("--m-init", type=float, nargs="+", default=[0.0], help="initial magnetisations")
    at.add_argument("--t-max", type=int, default=4096, help="sweep budget: p > t_max is reported as -1")
    at.add_argument("--chunk", type=int, default=16, help="sweeps between two host reads of the unsettled counter")
    at.add_argument("--batch", type=int, default=None, help="m_inits per replica-packed batch (default: all)")
    _common(at)
    qu = sub.add_parser("quench", help="drop the +1 spins a consensus configuration does not need (no reference script)")
    qu.add_argument("--in", dest="inp", required=True, help="result .npz of sa / hpr (graphs, conf) or sa-er "
                                                             "(row_ptr, col, conf)")
    qu.add_argument("--p", type=int, required=True)
    qu.add_argument("--c", type=int, required=True)
    qu.add_argument("--order-seed", type=int, default=None,
                    help="visit the nodes in np.random.default_rng(S).permutation(n) order (default: 0, 1, ...)")
    qu.add_argument("--restarts", type=int, default=0,
                    help="K >= 1: best of K orders per replica in one call (quench.quench_restarts), job (r, k) "
                         "walking np.random.default_rng([S, r, k]).permutation(n) with S = --order-seed (required); "
                         "0: one pass as above")
    qu.add_argument("--exchange", action="store_true",
                    help="with --restarts K: leave every job's local minimum downwards by (1, 2) exchanges, one -1 "
                         "spin to +1 and two +1 spins dropped (quench.quench_exchange); p + c - 1 <= 3")
    qu.add_argument("--max-passes", type=int, default=None,
                    help="--exchange: passes over the order at most (default 8); they end with the first that "
                         "commits nothing")
    qu.add_argument("--anneal", type=int, default=None, metavar="SWEEPS",
                    help="with --restarts K: SWEEPS Metropolis sweeps of n add / drop proposals inside the consensus "
                         "set behind every job's pass, closed by a pass from the lightest sweep end "
                         "(quench.quench_anneal)")
    qu.add_argument("--beta", type=float, nargs=2, default=None, metavar=("B0", "B1"),
                    help="--anneal: inverse temperature from B0 (first sweep) to B1 (last), linear (default 1.5 6.0)")
    qu.add_argument("--anneal-seed", type=int, default=None, help="--anneal: key of the proposal stream (default 0)")
    qu.add_argument("--schedule", choices=("sequential", "regions"), default="sequential",
                    help="of the single pass (--restarts 0): regions commits candidates whose balls do not meet in "
                         "the same round; same output, faster on large graphs")
    qu.add_argument("--window", type=int, default=None,
                    help="--schedule regions: pending candidates that compete per round (default: from n and the "
                         "ball bound)")
    qu.add_argument("--out", default=None, help="output .npz (default: the input's name + _quenched)")
    ce = sub.add_parser("census", help="count the starts of a small graph that reach consensus, all 2^n of them "
                                       "(no reference script)")
    ce.add_argument("--graph", choices=("rrg", "er"), default="rrg")
    ce.add_argument("--n", type=int, default=24, help="nodes (at most 48; 2^n configurations are run)")
    ce.add_argument("--d", type=int, default=3, help="degree (rrg)")
    ce.add_argument("--deg", type=float, default=2.0, help="mean degree (er; prob = deg/(n-1))")
    ce.add_argument("--graph-seed", type=int, default=0, help="seed of the graph")
    ce.add_argument("--p", type=int, required=True)
    ce.add_argument("--c", type=int, required=True)
    ce.add_argument("--max-configs", type=int, default=None,
                    help="refuse a larger 2^n (default 2^36; 2^34 with --minima, whose bitmap takes (T+1) 2^n / 8 "
                         "bytes)")
    ce.add_argument("--minima", action="store_true",
                    help="also count the minimal consensus sets of every level, the local minima of the quenches")
    ce.add_argument("--marginals", action="store_true",
                    help="also count the configurations of the levels per +1 node: node counts and the backbone of "
                         "the optimum")
    ce.add_argument("--levels", type=int, nargs="+", default=None,
                    help="--marginals: the step counts to count per node (default: p + c - 1), one enumeration each")
    ce.add_argument("--lam", type=float, nargs="+", default=None,
                    help="--marginals: also the exact phi, m_init, ent1 and node marginals at these lambdas")
    ce.add_argument("--out", default=None, help="output .npz (default: census_{graph}.npz)")
    ac = sub.add_parser("attractor-census", help="run all 2^n starts of a small graph to their attractors and count "
                                                 "them by class, transient and weight (no reference script)")
    ac.add_argument("--graph", choices=("rrg", "er"), default="rrg")
    ac.add_argument("--n", type=int, default=24, help="nodes (at most 48; 2^n configurations are run)")
    ac.add_argument("--d", type=int, default=3, help="degree (rrg)")
    ac.add_argument("--deg", type=float, default=2.0, help="mean degree (er; prob = deg/(n-1))")
    ac.add_argument("--graph-seed", type=int, default=0, help="seed of the graph")
    ac.add_argument("--t-max", type=int, default=32, help="a transient p > t_max is counted as unsettled")
    ac.add_argument("--max-configs", type=int, default=None, help="refuse a larger 2^n (default 2^36)")
    ac.add_argument("--out", default=None, help="output .npz (default: attractor_census_{graph}.npz)")
    return ap


def _devices(k):
    import torch
    have = torch.cuda.device_count()
    if k < 1 or k > max(have, 0):
        raise SystemExit(f"--gpus {k}: this node has {have} device(s)")
    return list(range(k))


def run_sa(a):
    import torch
    from .graph import random_regular_graph
    from .npz import save_sa_npz
    from .sa import SAReplicas, sa_run
    R = a.replicas if a.replicas is not None else a.N_stat
    gs = a.graph_seed if a.graph_seed is not None else a.seed
    if a.stream == "global" and a.gpus > 1:
        # one numpy stream seeded once (code/SA_RRG.py:58-88): replica k+1's draws
        # start where replica k's end, so the replicas cannot run side by side
        raise SystemExit(f"--gpus {a.gpus} with --stream global: the global stream is serial and runs on one "
                         "device; use --stream independent to spread replicas over devices")
    t0 = time.time()
    if a.stream == "global" or a.gpus == 1:
        res = sa_run(a.d, a.n, a.p, a.c, par_a=a.par_a, par_b=a.par_b, N_stat=R, seed=a.seed, graph_seed=gs,
                     stream=a.stream, max_steps=a.max_steps, max_seconds=a.max_seconds)
    else:
        # independent streams over several devices: one SAReplicas per device,
        # stepped round-robin (launches are asynchronous, so the devices overlap)
        devs = _devices(a.gpus)
        graphs = [random_regular_graph(a.d, a.n, seed=gs + k) for k in range(R)]
        parts = [list(range(R))[j::len(devs)] for j in range(len(devs))]
        runs = []
        for dev, idx in zip(devs, parts):
            if not idx:
                continue
            with torch.cuda.device(dev):
                runs.append((dev, idx, SAReplicas([graphs[k] for k in idx], a.p, a.c, [a.seed + k for k in idx],
                                                  par_a=a.par_a, par_b=a.par_b)))
        chunk, taken = 256, 0
        while True:
            live = [(dev, sa) for dev, _, sa in runs if not sa.all_done()]
            if not live or (a.max_steps is not None and taken >= a.max_steps) or \
                    (a.max_seconds is not None and time.time() - t0 >= a.max_seconds):
                break
            k = chunk if a.max_steps is None else min(chunk, a.max_steps - taken)
            for dev, sa in live:
                with torch.cuda.device(dev):
                    sa.steps(k)
            taken += k
            chunk = min(2 * chunk, 16384)
        res = {"mag_reached": np.zeros(R), "num_steps": np.zeros(R), "conf": np.zeros((R, a.n)),
               "done": np.zeros(R, dtype=np.int32)}
        for dev, idx, sa in runs:
            with torch.cuda.device(dev):
                out = sa.results()
            for j, k in enumerate(idx):
                for key in res:
                    res[key][k] = out[key][j]
        res["graphs"] = np.stack([g.astype(int) for g in graphs])
    out = a.out or f"MCMC_p{a.p}_d{a.d}.npz"
    save_sa_npz(out, res)
    print(f"sa: {R} replicas, num_steps {res['num_steps'].astype(np.int64).tolist()}, "
          f"mag_reached {np.round(res['mag_reached'], 4).tolist()}, {time.time() - t0:.1f} s -> {out}", flush=True)
    return res


def run_sa_er(a):
    from .sa_er import sa_er_run
    R = a.replicas if a.replicas is not None else a.N_stat
    gs = a.graph_seed if a.graph_seed is not None else a.seed
    _devices(a.gpus)                        # one graph shared by every replica: the current device
    t0 = time.time()
    res = sa_er_run(a.n, a.deg / (a.n - 1), a.p, a.c, par_a=a.par_a, par_b=a.par_b, N_stat=R, seed=a.seed,
                    graph_seed=gs, drop_isolated=not a.keep_isolated, max_steps=a.max_steps,
                    max_seconds=a.max_seconds, mode=a.mode)
    out = a.out or f"SA_ER_p{a.p}.npz"
    np.savez(out, **res)
    print(f"sa-er: {R} replicas on {res['row_ptr'].shape[0] - 1} nodes ({int(res['n_iso'])} isolated dropped), "
          f"num_steps {res['num_steps'].astype(np.int64).tolist()}, "
          f"mag_reached {np.round(res['mag_reached'], 4).tolist()}, {time.time() - t0:.1f} s -> {out}", flush=True)
    return res


def run_hpr(a):
    import torch
    from .graph import random_regular_edges
    from .hpr import hpr_run
    from .hpr_batch import hpr_run_batch
    from .npz import save_hpr_npz
    R = a.replicas if a.replicas is not None else a.n_rep
    gs = a.graph_seed if a.graph_seed is not None else a.seed
    devs = _devices(a.gpus)
    dtype = torch.float32 if a.dtype == "float32" else torch.float64
    res = {"mag_reached": np.zeros(R), "num_steps": np.zeros(R), "conf": np.zeros((R, a.n)),
           "graphs": np.zeros((R, a.n, a.d))}
    t0 = time.time()
    B = max(0, a.batch)
    for j, k0 in enumerate(range(0, R, B) if B else ()):
        # replicas k0 .. k0+B-1 as one union graph, consecutive groups round-robin over the devices
        ks = list(range(k0, min(R, k0 + B)))
        with torch.cuda.device(devs[j % len(devs)]):
            r = hpr_run_batch(a.d, a.n, a.p, a.c, [random_regular_edges(a.d, a.n, seed=gs + k) for k in ks],
                              [a.seed + k for k in ks], damppar=a.damppar, attr_value=a.attr_value,
                              lmbd_in=a.lmbd_in, pie=a.pie, gamma=a.gamma, TT=a.TT, dtype=dtype)
        for key in res:
            res[key][ks] = r[key]
    for k in (() if B else range(R)):       # HPR_pytorch_RRG.py:259, one graph per replica
        with torch.cuda.device(devs[k % len(devs)]):
            edges = random_regular_edges(a.d, a.n, seed=gs + k)
            r = hpr_run(a.d, a.n, a.p, a.c, damppar=a.damppar, attr_value=a.attr_value, lmbd_in=a.lmbd_in,
                        pie=a.pie, gamma=a.gamma, TT=a.TT, edges=edges, seed=a.seed + k, dtype=dtype)
        for key in res:
            res[key][k] = r[key][0]
    out = a.out or f"hpr_d{a.d}_p{a.p}.npz"
    save_hpr_npz(out, res, time=time.time() - t0)
    print(f"hpr: {R} replicas, num_steps {res['num_steps'].astype(np.int64).tolist()}, "
          f"mag_reached {np.round(res['mag_reached'], 4).tolist()}, {time.time() - t0:.1f} s -> {out}", flush=True)
    return res


def run_bdcm(a):
    from .bdcm import bdcm_er_run
    from .npz import save_bdcm_npz
    R = a.replicas if a.replicas is not None else a.num_rep
    _devices(a.gpus)                        # notebook-sized graphs: replicas run on the current device
    t0 = time.time()
    res = bdcm_er_run(n=a.n, deg=tuple(a.deg), num_rep=R, p=a.p, c=a.c, eps=a.eps, damppar=a.damppar,
                      attr_value=a.attr_value, epsilon=a.epsilon, T_max=a.T_max, a=a.a, dl=a.dl, seed=a.seed,
                      batch=a.batch)
    out = a.out or f"ER_p{a.p}.npz"
    save_bdcm_npz(out, res)
    print(f"bdcm: deg {list(a.deg)} x {R} replicas, {time.time() - t0:.1f} s -> {out}", flush=True)
    return res


def run_attractor(a):
    from .attractor import consensus_curve
    from .graph import Graph, erdos_renyi, random_regular_graph
    R = a.replicas if a.replicas is not None else 64
    gs = a.graph_seed if a.graph_seed is not None else a.seed
    _devices(a.gpus)                        # one graph shared by every replica: the current device
    t0 = time.time()
    if a.graph == "rrg":
        g = random_regular_graph(a.d, a.n, seed=gs)
    else:
        g = Graph.csr(*erdos_renyi(a.n, a.deg / (a.n - 1), seed=gs))
    res = consensus_curve(g, a.m_init, R, a.seed, t_max=a.t_max, chunk=a.chunk, batch=a.batch)
    out = a.out or f"attractor_{a.graph}.npz"
    np.savez(out, **res)
    print(f"attractor: {a.graph} n={a.n}, m_init {list(a.m_init)} x {R} replicas, consensus "
          f"{res['consensus'].tolist()}, c=1 {res['c1'].tolist()}, c=2 {res['c2'].tolist()}, unsettled "
          f"{res['unsettled'].tolist()}, max p {int(res['p'].max())}, {time.time() - t0:.1f} s -> {out}", flush=True)
    return res


def run_quench(a):
    from .graph import Graph
    from .quench import quench
    t0 = time.time()
    with np.load(a.inp, allow_pickle=False) as z:
        res = {k: z[k] for k in z.files}
    if "conf" not in res or not ("graphs" in res or ("row_ptr" in res and "col" in res)):
        raise SystemExit(f"{a.inp}: need conf with graphs (sa / hpr files) or with row_ptr, col (sa-er files)")
    conf = np.atleast_2d(res["conf"])
    S = conf.astype(np.int64)                   # the result files hold +-1 as floats
    if "graphs" in res and res["graphs"].shape[0] != S.shape[0]:
        raise SystemExit(f"{a.inp}: {res['graphs'].shape[0]} graphs for {S.shape[0]} configurations")
    how = {"schedule": a.schedule, "window": a.window} if a.schedule != "sequential" else {}
    if a.restarts >= 1:
        # best of K orders per replica, every (replica, order) a job of one call; SA / HPR files: the
        # (R, n, d) stack, a graph per replica
        from .quench import quench_anneal, quench_exchange, quench_restarts
        g = res["graphs"].astype(np.int32) if "graphs" in res else Graph.csr(res["row_ptr"], res["col"])
        if a.exchange:
            qr = quench_exchange(g, S, a.p, a.c, restarts=a.restarts, seed=a.order_seed,
                                 max_passes=8 if a.max_passes is None else a.max_passes)
            for key in ("mag_quench", "exchanges", "passes", "converged"):
                res[key] = qr[key]
        elif a.anneal is not None:
            qr = quench_anneal(g, S, a.p, a.c, a.anneal, beta=None if a.beta is None else tuple(a.beta),
                               restarts=a.restarts, seed=a.order_seed, anneal_seed=a.anneal_seed or 0)
            for key in ("mag_quench", "mag_best_sweep", "best_sweep", "adds", "drops", "refused"):
                res[key] = qr[key]
        else:
            qr = quench_restarts(g, S, a.p, a.c, restarts=a.restarts, seed=a.order_seed)
        q = {"conf": qr["conf_best"], "mag": qr["mag_best"], "consensus": qr["consensus"],
             "flipped": qr["flipped"][np.arange(S.shape[0]), qr["best"]]}      # of the restart that is kept
        res["mag_restarts"], res["best"] = qr["mag"], qr["best"]
    elif "graphs" in res:
        # one graph per replica (code/SA_RRG.py:58-62): replica by replica
        runs = [quench(res["graphs"][k].astype(np.int32), S[k:k + 1], a.p, a.c, seed=a.order_seed, **how)
                for k in range(S.shape[0])]
        q = {k: np.concatenate([r[k] for r in runs]) for k in ("conf", "mag", "flipped", "consensus")}
    else:
        q = quench(Graph.csr(res["row_ptr"], res["col"]), S, a.p, a.c, seed=a.order_seed, **how)
    res["conf_quenched"] = q["conf"].astype(conf.dtype)
    res["mag_quenched"], res["flipped"], res["consensus"] = q["mag"], q["flipped"], q["consensus"]
    out = a.out or (a.inp[:-4] if a.inp.endswith(".npz") else a.inp) + "_quenched.npz"
    np.savez(out, **res)
    print(f"quench: {S.shape[0]} replicas, consensus {res['consensus'].astype(int).tolist()}, flipped "
          f"{res['flipped'].tolist()}, mag {np.round(S.mean(axis=1), 4).tolist()} -> "
          f"{np.round(res['mag_quenched'], 4).tolist()}, {time.time() - t0:.1f} s -> {out}", flush=True)
    return res


def _small_graph(a):
    """The graph of the census subcommands -> (graph, its edges u < v as int64 (m, 2))."""
    from .graph import Graph, erdos_renyi, random_regular_graph
    if a.graph == "rrg":
        adj = random_regular_graph(a.d, a.n, seed=a.graph_seed)
        g = adj
        u = np.repeat(np.arange(a.n), a.d)
        v = np.asarray(adj).reshape(-1)
    else:
        rp, col = erdos_renyi(a.n, a.deg / (a.n - 1), seed=a.graph_seed)[:2]
        g = Graph.csr(rp, col)
        u = np.repeat(np.arange(a.n), np.diff(rp))
        v = np.asarray(col)
    keep = u < v
    return g, np.stack([u[keep], v[keep]], axis=1).astype(np.int64)


def run_census(a):
    from .census import census, census_boltzmann, census_marginals, census_minima
    if a.marginals and a.minima:
        raise SystemExit("census: --marginals and --minima are separate enumerations; run them one at a time")
    if not a.marginals and (a.levels is not None or a.lam is not None):
        raise SystemExit("census: --levels and --lam belong to --marginals")
    t0 = time.time()
    g, edges = _small_graph(a)
    limit = {} if a.max_configs is None else {"max_configs": a.max_configs}
    if a.marginals:
        res = census_marginals(g, a.p, a.c, levels=a.levels, **limit)
        if a.lam is not None:
            per = [census_boltzmann(res, a.lam, level=i) for i in range(len(res["levels"]))]
            res.update(lam=np.asarray(a.lam, dtype=np.float64), **{k: np.stack([b[k] for b in per]) for k in per[0]})
    else:
        res = (census_minima if a.minima else census)(g, a.p, a.c, **limit)
    res["edges"] = edges
    out = a.out or f"census_{a.graph}.npz"
    np.savez(out, **res)
    print(f"census: {a.graph} n={a.n}, 2^{a.n} configurations, p={a.p} c={a.c}: min_plus "
          f"{res['min_plus'].tolist()}, m_min {np.round(res['m_min'], 4).tolist()}, reached "
          f"{res['counts'].sum(axis=1).tolist()}, {time.time() - t0:.1f} s -> {out}", flush=True)
    if a.minima:
        print(f"census: minimal consensus sets {res['minima_total'].tolist()}, of them optimal "
              f"{[int(res['minima'][t, k]) for t, k in enumerate(res['min_plus'])]}, max_plus "
              f"{res['max_plus'].tolist()}, mean_plus {np.round(res['mean_plus'], 3).tolist()}", flush=True)
    if a.marginals:
        print(f"census: levels {res['levels']}, optimal configurations {res['optimal'].tolist()}, backbone +1 "
              f"{res['backbone_plus'].sum(axis=1).tolist()} and -1 {res['backbone_minus'].sum(axis=1).tolist()} of "
              f"{a.n} nodes", flush=True)
    return res


def run_attractor_census(a):
    from .census import attractor_census
    t0 = time.time()
    g, edges = _small_graph(a)
    limit = {} if a.max_configs is None else {"max_configs": a.max_configs}
    res = attractor_census(g, a.t_max, **limit)
    res["edges"] = edges
    out = a.out or f"attractor_census_{a.graph}.npz"
    np.savez(out, **res)
    print(f"attractor-census: {a.graph} n={a.n}, 2^{a.n} configurations, t_max={a.t_max}: "
          f"{dict(zip(res['classes'], res['hist'].sum(axis=(1, 2)).tolist()))}, unsettled "
          f"{int(res['unsettled'].sum())}, min_plus_ever {res['min_plus_ever']} (m_min {res['m_min_ever']:.4f}), "
          f"longest transient {res['p_longest']}, {res['mean_sweeps']:.2f} sweeps a wave, "
          f"{time.time() - t0:.1f} s -> {out}", flush=True)
    return res


def main(argv=None):
    a = build_parser().parse_args(argv)
    return {"sa": run_sa, "sa-er": run_sa_er, "hpr": run_hpr, "bdcm": run_bdcm, "attractor": run_attractor,
            "quench": run_quench, "census": run_census, "attractor-census": run_attractor_census}[a.cmd](a)


if __name__ == "__main__":
    main(sys.argv[1:])
