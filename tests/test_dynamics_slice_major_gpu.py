"""The replica-packed ELL rollout over a slice-major intermediate state
(mjx_rollout_ell_rp_sm): bit-exact against the one-slice rollout and the numpy
oracle, state and counts (added into a non-zero start), for every view
instantiation of the sweep kernels -- node->slice (whole rows and pieces),
slice->slice, slice->node -- the specialised degrees 3, 4, 6 and the runtime
degree 5, 16-byte and 8-byte units, one unit a slice, and the count path that
changes from global atomics to LDS when the row is sliced.

n = 257 for the even degrees; an odd-degree regular graph needs an even n, so
d = 3 and 5 run at 258 instead.  n = 1000 for all.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import majority as orc

pytestmark = pytest.mark.gpu

STEPS = (1, 2, 3, 4)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _init_counts(W):
    return torch.arange(64 * W, dtype=torch.int64, device="cuda") * 3 + 7


def _plus(S):
    return torch.from_numpy((S > 0).sum(axis=1).astype(np.int64)).cuda()


@functools.lru_cache(maxsize=None)
def _states(n, d, R):
    """(adj, [s(0), ..., s(4)]) of R random replicas on a d-regular graph, by the oracle."""
    import mjx
    adj = mjx.random_regular_graph(d, n, seed=7 * n + d)
    S = [(2 * np.random.default_rng(100 * n + 10 * d + R).integers(0, 2, (R, n)) - 1).astype(np.int8)]
    for _ in range(max(STEPS)):
        nxt = np.empty_like(S[-1])
        for r0 in range(0, R, 1024):           # rows are independent: bounds the oracle's (R, n, d) temporary
            nxt[r0:r0 + 1024] = orc.s_endstate_batch(adj, S[-1][r0:r0 + 1024], 1, 1)
        S.append(nxt)
    return adj, S


def _check(mjx_mod, n, d, R, slice_counts):
    adj, S = _states(n, d, R)
    g = mjx_mod.as_graph(adj)
    W = (R + 63) // 64
    bits = mjx_mod.pack(_cuda(S[0]))
    keep = bits.clone()
    for T in STEPS:
        init = _init_counts(W)
        c1 = init.clone()
        whole = mjx_mod.rollout(g, bits, T, words=W, counts=c1, slices=1)
        assert torch.equal(whole, mjx_mod.pack(_cuda(S[T]))), (n, d, R, T)
        assert torch.equal((c1 - init)[:R], _plus(S[T])) and not (c1 - init)[R:].any(), (n, d, R, T)
        for slices in slice_counts:
            for first_sliced in (False, True):
                cs = init.clone()
                out = torch.full_like(bits, 0x5555555555555555)          # every word must be written
                tmp = torch.full_like(bits, 0x3333333333333333)
                got = mjx_mod.rollout(g, bits, T, words=W, out=out, tmp=tmp, counts=cs, slices=slices,
                                      layout="slice", first_sliced=first_sliced)
                assert torch.equal(got, whole), (n, d, R, T, slices, first_sliced)
                assert torch.equal(cs, c1), (n, d, R, T, slices, first_sliced)
                assert torch.equal(bits, keep), "the input state was written"


def _n_for(n, d):
    return n + 1 if (n * d) % 2 else n


@pytest.mark.parametrize("n", [257, 1000])
@pytest.mark.parametrize("d", [3, 4, 6, 5])
@pytest.mark.parametrize("R,slice_counts", [(256, (2,)), (512, (2, 4)), (4096, (2, 8, 32)), (320, (5,))])
def test_slice_major_rollout(mjx_mod, n, d, R, slice_counts):
    """R = 256: U = 2, a slice is one 16-byte unit; R = 512: S = 2 keeps two
    units a slice; R = 4096: U = 32 down to one unit a slice; R = 320: W = 5
    is odd, 8-byte units, S = 5."""
    _check(mjx_mod, _n_for(n, d), d, R, slice_counts)


def test_slice_major_rollout_counters_fit_lds_only_per_slice(mjx_mod):
    """R = 16384 (U = 128): the whole row's counters take the global-atomic
    path, a half's 8192 replicas are exactly kMaxLdsReplicas and take the LDS
    one, a quarter's are below it."""
    _check(mjx_mod, 200, 4, 16384, (2, 4))


def test_slice_major_rollout_arguments(mjx_mod):
    adj, S = _states(1000, 4, 256)
    g = mjx_mod.as_graph(adj)
    L, D = mjx_mod._lib, mjx_mod._device
    bits = mjx_mod.pack(_cuda(S[0]))
    out, tmp = torch.empty_like(bits), torch.empty_like(bits)
    # S must divide U (W = 4: two units), for every step count and both variants
    for slices in (3, 4, 64):
        for T in STEPS:
            for fs in (False, True):
                with pytest.raises(mjx_mod.MjxError, match="invalid argument"):
                    mjx_mod.rollout(g, bits, T, words=4, slices=slices, layout="slice", first_sliced=fs)
    with pytest.raises(ValueError):
        mjx_mod.rollout(g, bits, 2, words=4, slices=2, layout="rows")

    def sm(s_in, s_out, scratch, steps, slices=2, fs=0):
        return L.load().mjx_rollout_ell_rp_sm(D.ptr(g.adj), g.n, g.d, 4, D.ptr(s_in), D.ptr(s_out),
                                              D.ptr(scratch) if scratch is not None else None, steps, slices, fs,
                                              None, D.stream_handle())

    # aliasing of s_in, s_out and tmp is refused; steps >= 2 needs tmp; slices = 0 is the plan's, not this call's
    for fs in (0, 1):
        assert sm(bits, bits, tmp, 2, fs=fs) == L.MJX_EINVAL
        assert sm(bits, out, bits, 2, fs=fs) == L.MJX_EINVAL
        assert sm(bits, out, out, 2, fs=fs) == L.MJX_EINVAL
        assert sm(bits, out, None, 2, fs=fs) == L.MJX_EINVAL
        assert sm(bits, out, tmp, 2, slices=0, fs=fs) == L.MJX_EINVAL
        assert sm(bits, out, tmp, -1, fs=fs) == L.MJX_EINVAL
        assert sm(bits, out, None, 1, fs=fs) == L.MJX_OK                 # one sweep needs no scratch
        torch.cuda.synchronize()
        assert torch.equal(out, mjx_mod.pack(_cuda(S[1])))
    # steps = 0: a copy and a popcount, as the node-major call
    init = _init_counts(4)
    cnt = init.clone()
    got = mjx_mod.rollout(g, bits, 0, words=4, counts=cnt, slices=2, layout="slice")
    assert got.data_ptr() != bits.data_ptr() and torch.equal(got, bits)
    assert torch.equal(cnt - init, _plus(S[0]))


def test_automatic_plan_matches_one_slice(mjx_mod):
    """slices=None (what mjx.rollout and mjx_rollout_ell_rp run) gives the
    one-slice result, whatever the plan picks."""
    adj, S = _states(1000, 4, 4096)
    g = mjx_mod.as_graph(adj)
    bits = mjx_mod.pack(_cuda(S[0]))
    for T in STEPS:
        init = _init_counts(64)
        ca = init.clone()
        got = mjx_mod.rollout(g, bits, T, words=64, counts=ca)
        assert torch.equal(got, mjx_mod.pack(_cuda(S[T])))
        assert torch.equal((ca - init), _plus(S[T]))
