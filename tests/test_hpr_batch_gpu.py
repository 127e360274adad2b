"""HPR on a batch of graphs as one union graph (hpr_batch.py) against the
single-graph path (hpr_run) on the same device and dtype, bit for bit: stop
iterations, configurations and generator positions; the record and batched
mask kernels at the ABI; the ``--batch`` front."""
import importlib
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

KEYS = ("num_steps", "conf", "mag_reached", "graphs")


def singles(mjx_mod, n, d, p, c, TT, G, dtype, extra=4):
    """G hpr_run calls (graph seeds 100 + k, torch seeds 200 + k): the stacked
    results and ``extra`` further draws of each generator."""
    res, tails = [], []
    for k in range(G):
        gen = torch.Generator().manual_seed(200 + k)
        res.append(mjx_mod.hpr_run(d, n, p, c, TT=TT, edges=mjx_mod.random_regular_edges(d, n, seed=100 + k),
                                   dtype=dtype, generator=gen))
        tails.append(torch.rand(extra, dtype=torch.float64, generator=gen))
    return {key: np.concatenate([r[key] for r in res]) for key in KEYS}, torch.stack(tails)


def batched(mjx_mod, n, d, p, c, TT, G, dtype, extra=4, **kw):
    gens = [torch.Generator().manual_seed(200 + k) for k in range(G)]
    res = mjx_mod.hpr_run_batch(d, n, p, c, [mjx_mod.random_regular_edges(d, n, seed=100 + k) for k in range(G)],
                                TT=TT, dtype=dtype, generators=gens, **kw)
    return res, torch.stack([torch.rand(extra, dtype=torch.float64, generator=g) for g in gens])


def same(a, b):
    for key in KEYS:
        assert a[0][key].shape == b[0][key].shape, key
        assert np.array_equal(a[0][key], b[0][key]), (key, a[0]["num_steps"], b[0]["num_steps"])
    assert torch.equal(a[1], b[1])


CASE1 = dict(n=40, d=4, p=1, c=1, TT=120, G=8, dtype=torch.float64)
CASE2 = dict(n=40, d=4, p=2, c=2, TT=200, G=6)


@pytest.fixture(scope="module")
def ref1(mjx_mod):
    return singles(mjx_mod, **CASE1)


@pytest.fixture(scope="module")
def ref2(mjx_mod):
    return {dt: singles(mjx_mod, dtype=dt, **CASE2) for dt in (torch.float32, torch.float64)}


def test_fp64_ref_layout_equals_eight_single_runs(mjx_mod, ref1):
    """Early stops, the TT cap and instances sharing a 64-bit word of the packed
    end state (n = 40): the float64 oracle stops these at [121, 121, 121, 116,
    57, 121, 121, 112]."""
    got = batched(mjx_mod, **CASE1)
    steps = ref1[0]["num_steps"]
    print("num_steps", steps.tolist(), got[0]["num_steps"].tolist())
    assert got[0]["num_steps"].shape == (8,) and got[0]["conf"].shape == (8, 40)
    assert got[0]["graphs"].shape == (8, 40, 4) and got[0]["mag_reached"].shape == (8,)
    same(got, ref1)
    assert len(set(steps.tolist())) >= 2 and steps.min() < CASE1["TT"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_compaction_does_not_change_the_results(mjx_mod, ref2, dtype):
    """p = c = 2: fp32 runs the decay-split ("q") layout, fp64 the reference
    layout.  The float64 oracle stops at [53, 53, 201, 71, 84, 52], so compact
    = 0.5 rebuilds the union after iteration 64 and again later; the results
    equal the single runs whether and whenever the union is rebuilt."""
    ref = ref2[dtype]
    print("num_steps", ref[0]["num_steps"].tolist())
    for compact in (0.0, 0.5, 1.0):
        got = batched(mjx_mod, dtype=dtype, compact=compact, **CASE2)
        same(got, ref)


def test_compaction_is_triggered(mjx_mod, ref2):
    """The case above does rebuild the union: with compact = 0.5 the loop ends on
    a union smaller than the batch, with compact = 0 on the whole batch; and the
    fp32 run is on the decay-split layout."""
    steps = ref2[torch.float32][0]["num_steps"]
    assert np.sum(steps <= 64) >= 3 and steps.max() > 64 + 16, steps
    sizes = {}
    for compact in (0.0, 0.5):
        hb, _ = make_batch(mjx_mod, 40, 4, 2, 2, 6, dtype=torch.float32, TT=200, compact=compact)
        assert hb.st.layout == "q"
        assert hb.run() == 0
        sizes[compact] = len(hb.inst)
        assert np.array_equal(hb.results()["num_steps"], steps)
    assert sizes[0.0] == 6 and sizes[0.5] < 6, sizes


def make_batch(mjx_mod, n, d, p, c, G, **kw):
    """An HPRBatch started as hpr_run_batch starts it, and its generators."""
    gens = [torch.Generator().manual_seed(200 + k) for k in range(G)]
    chi0s, b0s = [], []
    for g in gens:
        x = torch.rand((n * d, 4 ** (p + c)), dtype=torch.float64, generator=g)
        chi0s.append(x / x.sum(1, keepdim=True))
        b = torch.rand((n, 2), dtype=torch.float64, generator=g)
        b0s.append(b / b.sum(1, keepdim=True))
    edges = [mjx_mod.random_regular_edges(d, n, seed=100 + k) for k in range(G)]
    return mjx_mod.HPRBatch(d, n, p, c, edges, chi0s, b0s, gens, **kw), gens


def test_batch_start_snapshots_are_the_cpu_streams(mjx_mod):
    """rng_state_bytes: the engine of every instance at the start of the batch
    drawn ahead is its CPU generator after one rand(n) per iteration made."""
    n, G, k = 40, 3, 8
    hb, gens = make_batch(mjx_mod, n, 4, 1, 1, G, dtype=torch.float64, TT=10 ** 6, batch=k, compact=0.0)
    cpu = []
    for g in gens:
        h = torch.Generator()
        h.set_state(g.get_state())
        cpu.append(h)
    hb.run(max_batches=2, stop=False)
    assert hb.st.t == 2 * k and hb._drawn["t0"] == 2 * k
    for i, h in enumerate(cpu):
        for _ in range(2 * k):
            torch.rand(n, dtype=torch.float64, generator=h)
        g2 = torch.Generator()
        g2.set_state(hb.rng_state_bytes(hb._drawn["slot"], i))
        assert torch.equal(torch.rand(9, dtype=torch.float64, generator=g2),
                           torch.rand(9, dtype=torch.float64, generator=h))
    torch.cuda.synchronize()


def test_graph_replay_equals_eager_launches_and_batch_sizes(mjx_mod, ref1):
    same(batched(mjx_mod, graph=False, **CASE1), ref1)
    same(batched(mjx_mod, batch=8, **CASE1), ref1)
    same(batched(mjx_mod, batch=8, graph=False, compact=1.0, **CASE1), ref1)


def test_class_kernel_shapes_raise(mjx_mod):
    """d = 7 is beyond the register update kernels (hpr_run falls back to the
    per-degree-class kernel): the batch path says so."""
    edges = [mjx_mod.random_regular_edges(7, 20, seed=k) for k in range(2)]
    with pytest.raises(mjx_mod.MjxError, match="register update kernels"):
        mjx_mod.hpr_run_batch(7, 20, 1, 1, edges, [0, 1], TT=4, dtype=torch.float64)


# ---- mjx_hpr_batch_record at the ABI ----------------------------------------------
@pytest.mark.parametrize("n", [1, 40, 64, 100, 130])
@pytest.mark.parametrize("G", [1, 3, 5])
def test_batch_record_abi(mjx_mod, n, G):
    lib = mjx_mod.load_library()
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(1000 * n + G)
    N = G * n
    TT = 7

    def packed(b):
        w = np.zeros((N + 63) // 64 * 64, dtype=np.uint8)
        w[:N] = b
        w = w.reshape(-1, 64).astype(np.uint64)
        words = (w << np.arange(64, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
        return torch.from_numpy(words.view(np.int64)).cuda()

    counts = torch.full((G,), -1, dtype=torch.int64, device="cuda")
    done = torch.zeros(G, dtype=torch.int32, device="cuda")
    t_stop = torch.full((G,), -1, dtype=torch.int64, device="cuda")
    conf = torch.zeros((G, n), dtype=torch.int32, device="cuda")
    live = torch.full((1,), G, dtype=torch.int64, device="cuda")
    t_base = torch.tensor([2], dtype=torch.int64, device="cuda")

    def call(bits, s, t_add, base=t_base):
        assert lib.mjx_hpr_batch_record(bits.data_ptr(), s.data_ptr(), n, G, None, base.data_ptr() if base is not None
                                        else None, t_add, TT, counts.data_ptr(), done.data_ptr(), t_stop.data_ptr(),
                                        conf.data_ptr(), live.data_ptr(), st) == 0

    # t = 3: random bits, instance 0 at consensus (unless n == 1 leaves nothing random: then all stop or not by their bit)
    b = rng.integers(0, 2, N).astype(np.uint8)
    b[:n] = 1
    if n > 1:
        for g in range(1, G):
            b[g * n + int(rng.integers(0, n))] = 0             # the others one spin short at least
    s1 = torch.from_numpy(rng.integers(0, 2, N).astype(np.int32) * 2 - 1).cuda()
    call(packed(b), s1, 1)
    want = b.reshape(G, n).sum(axis=1)
    assert np.array_equal(counts.cpu().numpy(), want)
    stopped = want == n
    assert np.array_equal(done.cpu().numpy(), stopped.astype(np.int32))
    assert np.array_equal(t_stop.cpu().numpy(), np.where(stopped, 3, -1))
    assert np.array_equal(conf.cpu().numpy(), np.where(stopped[:, None], s1.cpu().numpy().reshape(G, n), 0))
    assert int(live.item()) == G - int(stopped.sum())
    # t = 5: other bits, every instance at consensus but the last; the done one is not written again
    b2 = np.ones(N, dtype=np.uint8)
    if G > 1:
        b2[(G - 1) * n] = 0
    s2 = torch.from_numpy(rng.integers(0, 2, N).astype(np.int32) * 2 - 1).cuda()
    call(packed(b2), s2, 3)
    assert np.array_equal(counts.cpu().numpy(), b2.reshape(G, n).sum(axis=1))
    now = (b2.reshape(G, n).sum(axis=1) == n) & ~stopped
    assert np.array_equal(t_stop.cpu().numpy(), np.where(stopped, 3, np.where(now, 5, -1)))
    exp = np.where(stopped[:, None], s1.cpu().numpy().reshape(G, n),
                   np.where(now[:, None], s2.cpu().numpy().reshape(G, n), 0))
    assert np.array_equal(conf.cpu().numpy(), exp)
    assert np.array_equal(done.cpu().numpy(), (stopped | now).astype(np.int32))
    # t = TT + 1 at consensus everywhere: the cap wins (done = 2) for whoever still runs
    last = ~(stopped | now)
    s3 = torch.from_numpy(rng.integers(0, 2, N).astype(np.int32) * 2 - 1).cuda()
    call(packed(np.ones(N, dtype=np.uint8)), s3, TT + 1, base=None)
    assert np.array_equal(counts.cpu().numpy(), np.full(G, n))
    assert np.array_equal(done.cpu().numpy(), np.where(last, 2, 1).astype(np.int32))
    assert np.array_equal(t_stop.cpu().numpy(), np.where(stopped, 3, np.where(now, 5, TT + 1)))
    exp = np.where(last[:, None], s3.cpu().numpy().reshape(G, n), exp)
    assert np.array_equal(conf.cpu().numpy(), exp)
    assert int(live.item()) == 0


def test_batch_record_slot_map(mjx_mod):
    """inst maps the slots of a compacted union to the instances' result rows."""
    lib = mjx_mod.load_library()
    n, G, total = 70, 2, 5
    inst = torch.tensor([3, 1], dtype=torch.int32, device="cuda")
    bits = torch.full(((G * n + 63) // 64,), -1, dtype=torch.int64, device="cuda")
    s = torch.arange(G * n, dtype=torch.int32, device="cuda")
    counts = torch.zeros(G, dtype=torch.int64, device="cuda")
    done = torch.zeros(total, dtype=torch.int32, device="cuda")
    done[1] = 1
    t_stop = torch.zeros(total, dtype=torch.int64, device="cuda")
    conf = torch.zeros((total, n), dtype=torch.int32, device="cuda")
    live = torch.tensor([4], dtype=torch.int64, device="cuda")
    assert lib.mjx_hpr_batch_record(bits.data_ptr(), s.data_ptr(), n, G, inst.data_ptr(), None, 9, 100,
                                    counts.data_ptr(), done.data_ptr(), t_stop.data_ptr(), conf.data_ptr(),
                                    live.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    assert counts.tolist() == [n, n] and done.tolist() == [0, 1, 0, 1, 0] and t_stop.tolist() == [0, 0, 0, 9, 0]
    assert int(live.item()) == 3
    want = np.zeros((total, n), dtype=np.int32)
    want[3] = np.arange(n)
    assert np.array_equal(conf.cpu().numpy(), want)


# ---- mjx_hpr_refresh_masks_jump_batch ---------------------------------------------
def engine(gen):
    b = gen.get_state().numpy()
    words = b[24:24 + 624 * 8].view(np.uint64).astype(np.uint32).view(np.int32)
    return words.copy(), [int(b[8:12].view(np.int32)[0]), int(b[16:24].view(np.uint64)[0])]


@pytest.mark.parametrize("n,k,chunks", [(40, 16, 1), (1000, 4, 4)])
def test_jump_batch_equals_separate_jump_calls(mjx_mod, n, k, chunks):
    """Three streams standing at different places of their 624-word block (0, 1
    and 311 doubles drawn): masks, output states and left/next equal three
    mjx_hpr_refresh_masks_jump calls; one chunk, and four chunks that jump."""
    lib = mjx_mod.load_library()
    st = torch.cuda.current_stream().cuda_stream
    G = 3
    L, used = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32)
    assert lib.mjx_mt_jump_geometry(n, k, chunks, L.ctypes.data, used.ctypes.data) == 0
    assert int(used[0]) == chunks
    words = lib.mjx_mt_jump_table_words(n, k, chunks)
    assert (words > 0) == (chunks > 1)
    table = None
    if words:
        host = np.zeros(words, dtype=np.uint64)
        assert lib.mjx_mt_jump_table(n, k, chunks, host.ctypes.data) == 0
        table = torch.from_numpy(host.view(np.int64)).cuda()
    tp = table.data_ptr() if table is not None else None
    mts, lns = [], []
    for g, pre in enumerate((0, 1, 311)):
        gen = torch.Generator().manual_seed(30 + g)
        if pre:
            torch.rand(pre, dtype=torch.float64, generator=gen)
        w, ln = engine(gen)
        mts.append(w)
        lns.append(ln)
    assert len({ln[0] for ln in lns}) == 3                      # three different `left`
    mt = torch.from_numpy(np.stack(mts)).cuda()
    ln = torch.tensor(lns, dtype=torch.int32, device="cuda")
    th = torch.tensor([0.05 + 0.9 * j / k for j in range(k)], dtype=torch.float64, device="cuda")
    want_mask = torch.empty((k, G, n), dtype=torch.uint8, device="cuda")
    want_mt, want_ln = torch.empty_like(mt), torch.empty_like(ln)
    for g in range(G):
        m1 = torch.empty((k, n), dtype=torch.uint8, device="cuda")
        assert lib.mjx_hpr_refresh_masks_jump(mt[g].data_ptr(), ln[g].data_ptr(), want_mt[g].data_ptr(),
                                              want_ln[g].data_ptr(), n, k, chunks, tp, th.data_ptr(), m1.data_ptr(),
                                              st) == 0
        want_mask[:, g] = m1
    mask = torch.full((k, G, n), 7, dtype=torch.uint8, device="cuda")
    mt_out, ln_out = torch.zeros_like(mt), torch.zeros_like(ln)
    assert lib.mjx_hpr_refresh_masks_jump_batch(mt.data_ptr(), ln.data_ptr(), mt_out.data_ptr(), ln_out.data_ptr(), n,
                                                k, chunks, G, tp, th.data_ptr(), mask.data_ptr(), st) == 0
    assert torch.equal(mask, want_mask)
    assert 0 < int(mask.sum()) < mask.numel()
    assert torch.equal(mt_out, want_mt) and torch.equal(ln_out, want_ln)


# ---- the front --------------------------------------------------------------------
def test_front_batch_writes_the_arrays_of_batch_0(mjx_mod, tmp_path):
    """--batch 3 over 4 replicas (groups of 3 + 1) in a child process against
    --batch 0."""
    args = ["hpr", "--n", "40", "--d", "4", "--TT", "60", "--replicas", "4", "--dtype", "float64"]
    out_b, out_0 = tmp_path / "b.npz", tmp_path / "z.npz"
    run = subprocess.run([sys.executable, "-m", "mjx"] + args + ["--batch", "3", "--out", str(out_b)],
                         capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    importlib.import_module("mjx.cli").main(args + ["--batch", "0", "--out", str(out_0)])
    with np.load(out_b, allow_pickle=False) as b, np.load(out_0, allow_pickle=False) as z:
        assert sorted(b.files) == sorted(z.files) == ["conf", "graphs", "mag_reached", "num_steps", "time"]
        for key in KEYS:
            assert b[key].shape == z[key].shape and np.array_equal(b[key], z[key]), key
        assert b["conf"].shape == (4, 40)
