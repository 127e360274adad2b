"""mjx_rollout_ell_rp_plan: what the replica-packed ELL rollout runs when it is
given slices = 0 (mjx_rollout_ell_rp, mjx.rollout).  Host only: no device call."""
import ctypes


def _plan(mjx_mod, n, d, words, steps):
    lib = mjx_mod.load_library()
    s, sm, fs = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.mjx_rollout_ell_rp_plan(n, d, words, steps, ctypes.byref(s), ctypes.byref(sm), ctypes.byref(fs))
    assert rc == 0
    return s.value, sm.value, fs.value


ONE_SLICE = (1, 0, 0)


def test_bench_shape_runs_the_measured_winner(mjx_mod):
    """d=4, N=1e6, R=4096, two sweeps: profiles/slice_major_ab.log's fastest
    row is the slice-major state in 2 slices with the first sweep sliced; the
    same at three sweeps and at the SA rollout mode's d=3."""
    assert _plan(mjx_mod, 1_000_000, 4, 64, 2) == (2, 1, 1)
    assert _plan(mjx_mod, 1_000_000, 4, 64, 3) == (2, 1, 1)
    assert _plan(mjx_mod, 1_000_000, 3, 64, 2) == (2, 1, 1)


def test_state_that_fits_the_cache_runs_one_slice(mjx_mod):
    assert _plan(mjx_mod, 100_000, 4, 64, 2) == ONE_SLICE          # 51 MB
    assert _plan(mjx_mod, 400_000, 4, 64, 3) == ONE_SLICE          # 205 MB + 6 MB of adjacency
    assert _plan(mjx_mod, 1236, 4, 64, 4) == ONE_SLICE


def test_a_single_sweep_runs_one_slice(mjx_mod):
    assert _plan(mjx_mod, 1_000_000, 4, 64, 1) == ONE_SLICE
    assert _plan(mjx_mod, 1_000_000, 4, 64, 0) == ONE_SLICE


def test_no_admissible_slice_count_runs_one_slice(mjx_mod):
    assert _plan(mjx_mod, 40_000_000, 4, 2, 2) == ONE_SLICE        # U = 1: nothing divides it
    assert _plan(mjx_mod, 10_000_000, 4, 6, 2) == ONE_SLICE        # U = 3: a third of a row is 16 bytes
    assert _plan(mjx_mod, 1_000_000, 4, 62, 2) == ONE_SLICE        # U = 31 is prime: one-unit slices only
    assert _plan(mjx_mod, 4_000_000, 4, 64, 2) == ONE_SLICE        # half rows of 256 B, but 2 GB a sliced sweep


def test_arguments(mjx_mod):
    lib = mjx_mod.load_library()
    x = ctypes.c_int(0)
    assert lib.mjx_rollout_ell_rp_plan(10, 4, 0, 2, ctypes.byref(x), ctypes.byref(x), ctypes.byref(x)) == 1
    assert lib.mjx_rollout_ell_rp_plan(10, 4, 4, 2, None, ctypes.byref(x), ctypes.byref(x)) == 1
