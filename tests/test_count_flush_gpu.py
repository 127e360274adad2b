"""The fused per-replica counters past their mid-loop flush.

Every counting sweep keeps the +1 counts of a thread's nodes in a bit-sliced
VertCounter<VW, NK> and must flush it when ``added == F = 2**NK - 1`` (F = 255
at 8 planes, 63 in k_sweep_cls_all_rp, 1023 in the runtime-degree / CSR
sweeps).  A thread owns one unit (two words for even W, one for odd W) of every
``slots``-th node with ``slots = grid * 256 // Us``; a CU holds at most 2048
threads, so ``slots <= slots_max = CUs * 2048 // Us`` whatever the occupancy.
Each case takes ``n >= (F + 1) * slots_max + 1`` nodes: every active thread
then walks more than F nodes and flushes mid-loop at least once.  The case
asserts that inequality, so a change of the grid policy or of a plane count
cannot turn it back into a below-threshold test unnoticed.

Per case, one sweep (two state buffers) of
  * all +1 (every counter plane saturates before each flush: a lost carry or
    a missed flush shows here): output == input, every live replica counts n,
    added to a non-zero counts tensor;
  * seeded random bits: counts == a plain torch bit-sum of the output (not
    mjx.popcount, which shares the counter), sampled replicas == the CPU
    oracle, padding replicas count 0.
"""
import numpy as np
import pytest
import torch

from oracle import fast

pytestmark = pytest.mark.gpu

THREADS_PER_CU = 2048          # 8 waves x 4 SIMDs x 64 lanes: the hardware maximum


def _geometry(F, R):
    """(n, W) with n past the flush threshold of an F-node counter at R replicas."""
    from mjx import _device
    W = (R + 63) // 64
    Us = W // 2 if W % 2 == 0 else W
    slots_max = _device.cu_count() * THREADS_PER_CU // Us
    n = (F + 1) * slots_max + 1
    n += n & 1                                   # n * d even for every d
    assert n >= (F + 1) * slots_max + 1          # reachability: > F nodes per thread at any occupancy
    return n, W


def _last_word_mask(R):
    return (1 << (R % 64)) - 1 if R % 64 else -1


def _ones(n, W, R):
    x = torch.full((n, W), -1, dtype=torch.int64, device="cuda")
    x[:, -1] = _last_word_mask(R)
    return x.view(-1)


def _random(n, W, R, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randint(-2 ** 63, 2 ** 63 - 1, (n, W), dtype=torch.int64, device="cuda", generator=gen)
    if R % 64:
        x[:, -1] &= _last_word_mask(R)           # padding replicas are -1 spins (bit 0), as pack() leaves them
    return x.view(-1)


def _bit_sums(bits, n, W):
    """Per-replica +1 counts (64 * W,) by shifting and summing in torch."""
    x = bits.view(n, W)
    ref = torch.zeros(W, 64, dtype=torch.int64, device=bits.device)
    rows = max(1, (1 << 24) // W)
    for i in range(0, n, rows):
        c = x[i:i + rows]
        for b in range(64):
            ref[:, b] += ((c >> b) & 1).sum(0)
    return ref.view(-1)


def _or_rows(x):
    while x.shape[0] > 1:
        h = x.shape[0] // 2
        y = x[:h] | x[h:2 * h]
        if x.shape[0] & 1:
            y[0] |= x[-1]
        x = y
    return x[0]


def _or_over_nodes(a, b, n, W):
    """OR over the nodes of a ^ b (a alone for b = None): (W,) flag words."""
    acc = torch.zeros(W, dtype=torch.int64, device=a.device)
    rows = max(1, (1 << 24) // W)
    for i in range(0, n, rows):
        x = a.view(n, W)[i:i + rows]
        acc |= _or_rows(x ^ b.view(n, W)[i:i + rows] if b is not None else x)
    return acc


def _replica(bits, n, W, r):
    col = bits.view(n, W)[:, r >> 6]
    return (((col >> (r & 63)) & 1) * 2 - 1).cpu().numpy()


class _Case:
    """One counting sweep ``run(s_in, s_out, counts)`` over n nodes, its oracle
    ``step(spins) -> spins`` for one replica and, for a tracked sweep, the flag
    words it left (``diff``, 2W) with what s_out held before (``prev``)."""
    tracked = False

    def __init__(self, n, W, R, run, step):
        self.n, self.W, self.R, self.run, self.step = n, W, R, run, step


def _check(case, seed):
    n, W, R = case.n, case.W, case.R
    torch.cuda.reset_peak_memory_stats()
    live = torch.arange(64 * W, device="cuda") < R
    # all +1: a fixed point, every live replica counts n; counts are added to
    s_in = _ones(n, W, R)
    out = torch.empty_like(s_in)
    init = torch.arange(64 * W, dtype=torch.int64, device="cuda") * 3 + 1
    cnt = init.clone()
    if case.tracked:
        out.copy_(s_in)                          # s_prev aliases s_out: s(t-1) = s(t)
    diff = case.run(s_in, out, cnt)
    assert torch.equal(out, s_in)
    assert torch.equal(cnt - init, torch.where(live, n, 0))
    if case.tracked:
        assert not diff.any()
    del s_in
    # random bits
    s_in = _random(n, W, R, seed)
    cnt = torch.zeros(64 * W, dtype=torch.int64, device="cuda")
    if case.tracked:
        out.zero_()                              # s(t-1) = all -1
    diff = case.run(s_in, out, cnt)
    assert torch.equal(cnt, _bit_sums(out, n, W))
    assert not cnt[R:].any()
    if case.tracked:
        assert torch.equal(diff[:W], _or_over_nodes(out, s_in, n, W))
        assert torch.equal(diff[W:], _or_over_nodes(out, None, n, W))
    for r in (1, R - 1):
        assert np.array_equal(_replica(out, n, W, r), case.step(_replica(s_in, n, W, r))), r
    print(f"n={n} W={W} peak={torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    del s_in, out
    torch.cuda.empty_cache()


def _as_csr(mjx_mod, g, isolated=0):
    """The d-regular ELL graph as a CSR Graph, plus ``isolated`` edgeless nodes."""
    rp = torch.arange(g.n + 1, dtype=torch.int64, device="cuda") * g.d
    if isolated:
        rp = torch.cat([rp, rp[-1:].expand(isolated)])
    return mjx_mod.Graph.csr_device(rp, g.adj.reshape(-1))


def _ell_step(g):
    adj = g.adj.cpu().numpy()
    return lambda s: fast.s_endstate(adj, s, 1, 1)


def _csr_step(g):
    rp, col = g.row_ptr.cpu().numpy(), g.col.cpu().numpy()
    return lambda s: fast.s_endstate_er(rp, col, s, 1, 1)


def _rollout(mjx_mod, g, W):
    def run(s_in, out, cnt):
        mjx_mod.rollout(g, s_in, 1, words=W, out=out, counts=cnt)
    return run


# (F, d, R): the launchers pick the kernel from d, the parity of W and R
ELL = {
    "ell_d3_R4096": (255, 3, 4096),          # k_sweep_ell_rp<3,2,true>, LDS counters, rotated
    "ell_d4_R8192": (255, 4, 8192),          # k_sweep_ell_rp<4,2,true>, all 32 KiB of LDS counters (units 0..63)
    "ell_d6_R4096": (255, 6, 4096),          # k_sweep_ell_rp<6,2,true>
    "ell_d3_R16384": (255, 3, 16384),        # k_sweep_ell_rp<3,2,true>, use_lds = 0: flushes straight to global
    "ell_d4_R4000": (255, 4, 4000),          # k_sweep_ell_rp<4,1,true>: W = 63, 8-byte units, 32 padding replicas
    "gen_d5_R4000": (1023, 5, 4000),         # k_sweep_gen_rp<1,true,false>: runtime degree, 10 planes
}


@pytest.mark.parametrize("name", list(ELL))
def test_ell_counts_past_the_flush(mjx_mod, name):
    F, d, R = ELL[name]
    n, W = _geometry(F, R)
    g = mjx_mod.random_regular_graph_device(d, n, seed=d)
    _check(_Case(n, W, R, _rollout(mjx_mod, g, W), _ell_step(g)), seed=R + d)


# (F, d, R, rp_layout, isolated nodes)
CSR = {
    # one class D = 4: the per-class counting launch k_sweep_cls_rp<4,2,true>
    "cls_d4_R4096": (255, 4, 4096, "class", 0),
    # one class D = 10 > 8: k_sweep_cls_gen_rp<2,true>
    "clsgen_d10_R4096": (255, 10, 4096, "class", 0),
    # classes D = 0 and D = 4: k_sweep_cls_all_rp<2>, 6 planes
    "clsall_d4_iso_R4096": (63, 4, 4096, "class", 1000),
    # row_ptr/col sweep k_sweep_gen_rp<1,true,true>, 10 planes (W = 63)
    "csr_d4_R4000": (1023, 4, 4000, "csr", 0),
}


@pytest.mark.parametrize("name", list(CSR))
def test_csr_counts_past_the_flush(mjx_mod, name):
    F, d, R, layout, iso = CSR[name]
    n, W = _geometry(F, R)
    g = _as_csr(mjx_mod, mjx_mod.random_regular_graph_device(d, n - iso, seed=d), iso)
    assert g.n == n
    g.rp_layout = layout
    if layout == "class":
        classes = g.class_ell()[2]
        assert classes[:, 2].tolist() == ([0, d] if iso else [d])
    _check(_Case(n, W, R, _rollout(mjx_mod, g, W), _csr_step(g)), seed=R + d)


# (F, d, R, entry point)
TRACK = {
    "track_ell_d4_R4096": (255, 4, 4096, "ell"),      # k_sweep_ell_rp<4,2,true>, TRACK
    "track_gen_d5_R4000": (1023, 5, 4000, "ell"),     # k_sweep_gen_rp<1,true,false>, TRACK
    "track_csr_d4_R4000": (1023, 4, 4000, "csr"),     # k_sweep_gen_rp<1,true,true>, TRACK
}


@pytest.mark.parametrize("name", list(TRACK))
def test_tracked_counts_past_the_flush(mjx_mod, name):
    """mjx_sweep_track_ell_rp / mjx_sweep_track_csr_rp with s_prev aliasing
    s_out: counts as above; the flag rows are zero on the fixed point and equal
    the OR over nodes of out ^ in and of out ^ prev on the random input."""
    from mjx import _lib as L, _device as D
    F, d, R, entry = TRACK[name]
    n, W = _geometry(F, R)
    g = mjx_mod.random_regular_graph_device(d, n, seed=d)
    step = _ell_step(g)
    if entry == "csr":
        g = _as_csr(mjx_mod, g)

    def run(s_in, out, cnt):
        diff = torch.zeros(2 * W, dtype=torch.int64, device="cuda")
        if entry == "ell":
            L.call("mjx_sweep_track_ell_rp", D.ptr(g.adj), n, d, W, D.ptr(s_in), D.ptr(out), D.ptr(out), D.ptr(cnt),
                   D.ptr(diff), D.stream_handle())
        else:
            L.call("mjx_sweep_track_csr_rp", D.ptr(g.row_ptr), D.ptr(g.col), D.ptr(g.order), n, W, D.ptr(s_in),
                   D.ptr(out), D.ptr(out), D.ptr(cnt), D.ptr(diff), D.stream_handle())
        return diff

    case = _Case(n, W, R, run, step)
    case.tracked = True
    _check(case, seed=R + d)


@pytest.mark.parametrize("R", [4096, 16384])
def test_popcount_past_the_flush(mjx_mod, R):
    """k_popcount_rp<2> (R = 4096: LDS counters; R = 16384: global) against the
    torch bit-sum."""
    n, W = _geometry(255, R)

    def run(s_in, out, cnt):
        out.copy_(s_in)
        mjx_mod.popcount(out, n, words=W, counts=cnt)

    _check(_Case(n, W, R, run, lambda s: s), seed=R)
