"""A plain bench.py run on the device (small sizes): it prints the headline
line alone -- none of the --full legs, no detail file -- and --dump-outputs
writes what the last timed step returned, held here against the numpy oracle
on the bench's own seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_and_dumps_the_last_step(mjx_mod, tmp_path):
    import torch
    import bench
    from oracle import majority as orc
    n, d, R, p, c, seed = 20_000, 4, 130, 2, 1, 3
    W = (R + 63) // 64
    dump = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup",
                          "1", "--n", str(n), "--d", str(d), "--replicas", str(R), "--p", str(p), "--c", str(c),
                          "--seed", str(seed), "--dump-outputs", str(dump)],
                         capture_output=True, text=True, timeout=240, env=env, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr[-3000:]
    (line,) = [json.loads(x) for x in run.stdout.splitlines() if x.strip().startswith("{")]
    assert line["unit"] == "node-updates/s" and line["higher_is_better"] is True and line["full"] is False
    assert line["metric"].startswith("node-updates/s, d=4 RRG majority rollout")
    assert line["dtype"] == "u64 bit-packed spins (int32 indices)"
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: updates of the 3 timed steps over their wall time
    assert line["value"] == pytest.approx(n * R * (p + c - 1) / (line["ms_per_step"] / 1e3), rel=1e-9)
    for leg in bench.LEG_KEYS + ("cpu_baseline", "summary", "detail_file"):
        assert leg not in line, leg
    assert sorted(os.listdir(tmp_path)) == ["dump"]                      # no detail file beside the dump
    assert sorted(os.listdir(dump)) == ["counts.npy", "s_end_sample.npy"]

    # the bench's inputs again: graph and s0 from the same seeds
    adj = mjx_mod.random_regular_graph(d, n, seed=seed)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    s0 = torch.randint(-2 ** 62, 2 ** 62, (n * W,), dtype=torch.int64, device="cuda", generator=gen)
    words = s0.cpu().numpy().view(np.uint8).reshape(n, 8 * W)
    # every bit of the W words is a replica to the sweep: 64 W of them, the first R dumped as spins
    S0 = 2 * np.unpackbits(words, axis=1, bitorder="little").T.astype(np.int64) - 1             # (64 W, n)
    want = orc.s_endstate_batch(adj, S0, p, c)
    counts = np.load(dump / "counts.npy")
    sample = np.load(dump / "s_end_sample.npy")
    assert counts.dtype == np.float64 and np.array_equal(counts, (want == 1).sum(axis=1))
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(n, size=bench.DUMP_NODES, replace=False))
    assert sample.dtype == np.float32 and np.array_equal(sample, want[:R, idx].T.astype(np.float32))
