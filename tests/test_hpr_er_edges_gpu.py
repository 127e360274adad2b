"""The ER ("general") HPR where its launch shapes change: chunked launches
from a small scratch slab, the last class whose count table fits LDS and the
first that does not (per dtype), the whole loop against the oracle's chain,
equality with the register kernels on regular graphs, and what the ABI
refuses.  Graphs are built with known degree classes (tests/hpr_er_cases.py);
every comparison is against oracle/hpr.py (float64 numpy).  Bars: messages
1e-12 (float64) / 1e-5 (float32) row-normalised, marginals the same absolute;
s, conf and num_steps exactly."""
import numpy as np
import pytest
import torch

import hpr_er_cases as hc
from oracle import hpr as orc

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
TOL = {F32: 1e-5, F64: 1e-12}
ID = {F32: "f32", F64: "f64"}
OK, EINVAL, ERANGE = 0, 1, 3                              # include/mjx.h


def rownorm_err(got, ref):
    got = np.asarray(got, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.max(np.abs(ref), axis=1, keepdims=True)))


def code(mjx, dtype):
    return mjx._lib.MJX_F32 if dtype == F32 else mjx._lib.MJX_F64


def dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def step(mjx, plan, chi, b, p, c, attr, dtype):
    return mjx.HPr_dp_er(dev(chi, dtype), dev(b, dtype), plan, p, c, attr, 25 * plan.n, 0.4)


# ---- B: the hub's class in several launches from a slab of 1, 2, 3 tables ----
@pytest.mark.parametrize("dtype", [F64, F32], ids=ID.get)
@pytest.mark.parametrize("name,p,c,D", [("slab_t4", 2, 2, 10), ("slab_t3", 1, 2, 21)])
def test_chunked_slab_launches_equal_the_full_slab(mjx_mod, name, p, c, D, dtype):
    """A hub of degree D + 1 whose class takes its count tables from the global
    slab.  With the default slab every table is in flight at once (e0 = 0
    only); with room for k = 1, 2, 3 tables the class runs in ceil(m / k)
    launches at e0 = k, 2k, ... (k = 3 ends in a short chunk: m = 11 -> 2, m =
    22 -> 1).  A message is computed by one workgroup in one order whatever
    the chunk, so every chunked result equals the full one bit for bit, and
    the full one meets the oracle.  The slab is filled with NaN bytes before
    every call: the kernel zeroes its own table."""
    G = hc.built(name)
    plan = hc.plan(mjx_mod, G)
    lib = mjx_mod.load_library()
    tab = lib.mjx_hpr_er_scratch_bytes(code(mjx_mod, dtype), D, p, c)
    assert tab == hc.table_bytes(dtype, D, p + c) > 0
    assert max(G.class_set) == D
    rows = G.rows_of(D)
    m = rows.size
    assert m >= D + 1
    for attr in (1, -1):
        chi, b, want, _ = hc.oracle_step(name, p, c, attr)
        plan.__dict__.pop("SCRATCH_CAP", None)           # the class default: 256 MB
        plan._scratch_key = None
        sc = plan.scratch(dtype, p, c)
        assert sc.numel() == m * tab                      # the whole class at once
        sc.fill_(0xFF)
        full = step(mjx_mod, plan, chi, b, p, c, attr, dtype)
        err, err_hub = rownorm_err(full.cpu().numpy(), want), rownorm_err(full.cpu().numpy()[rows], want[rows])
        print(f"B {name} p={p} c={c} {ID[dtype]} attr={attr}: err {err:.3e} (class {D}: {err_hub:.3e}) bar {TOL[dtype]}")
        assert err_hub <= TOL[dtype], (attr, "hub class")
        assert err <= TOL[dtype], attr
        for k in (1, 2, 3):
            plan.SCRATCH_CAP = k * tab
            plan._scratch_key = None
            sc = plan.scratch(dtype, p, c)
            per = sc.numel() // tab
            assert sc.numel() == k * tab and per == k
            launches = -(-m // per)
            assert launches > 1 and (k != 3 or m % per != 0)
            sc.fill_(0xFF)
            got = step(mjx_mod, plan, chi, b, p, c, attr, dtype)
            assert torch.equal(got, full), (attr, k, launches)


# ---- C: the last LDS class and the first slab class of each dtype ----
def _boundary_cases():
    out = []
    for T, (name, d_lds, d_slab) in hc.BOUNDARY.items():
        more, extra = hc.MORE_SLAB[T]
        for dtype in (F64, F32):
            cases = [(name, d_lds, "lds"), (name, d_slab, "slab")]
            cases += [(more, D, "slab") for D in extra] if dtype == F32 else []
            for graph, D, side in cases:
                for p, c in hc.SPLITS[T]:
                    out.append(pytest.param(graph, T, dtype, D, side, p, c,
                                            id=f"T{T}-{ID[dtype]}-D{D}-{side}-p{p}c{c}"))
    return out


@pytest.mark.parametrize("name,T,dtype,D,side,p,c", _boundary_cases())
def test_classes_on_both_sides_of_the_lds_boundary(mjx_mod, name, T, dtype, D, side, p, c):
    """One step and the marginals on a graph with a hub in class D, which is
    first shown to lie on the side of the 160 KiB LDS budget that the case is
    named for (a change of the budget or of the layout fails here instead of
    testing another path).  The table is double for float messages too, so
    both dtypes share the boundary: D = 6 | 7 at T = 4, 16 | 17 at T = 3;
    float also runs D = 8, 9 and D = 20, 21 on the slab.  The rows of class D
    are compared on their own, then all rows.  attr = +1 where p is odd, -1
    where it is even."""
    G = hc.built(name)
    assert D in G.class_set and p + c == T
    lib = mjx_mod.load_library()
    got_bytes = lib.mjx_hpr_er_scratch_bytes(code(mjx_mod, dtype), D, p, c)
    lds = hc.table_bytes(dtype, D, T) + hc.incoming_bytes(dtype, D, T)
    if side == "lds":
        assert got_bytes == 0 and lds <= hc.K_MAX_LDS
    else:
        assert got_bytes == hc.table_bytes(dtype, D, T) > 0 and lds > hc.K_MAX_LDS
    attr = 1 if p % 2 else -1
    chi, b, want, want_marg = hc.oracle_step(name, p, c, attr)
    plan = hc.plan(mjx_mod, G)
    got = step(mjx_mod, plan, chi, b, p, c, attr, dtype).cpu().numpy()
    rows = G.rows_of(D)
    err, err_cls = rownorm_err(got, want), rownorm_err(got[rows], want[rows])
    marg = mjx_mod.marginals_comp_er(dev(want, dtype), plan, p, c).cpu().numpy()
    err_marg = float(np.max(np.abs(marg - want_marg)))
    print(f"C T={T} {ID[dtype]} D={D} {side} p={p} c={c}: class {err_cls:.3e} all {err:.3e} marg {err_marg:.3e} "
          f"bar {TOL[dtype]}")
    assert np.all(np.isfinite(got[rows]))
    assert err_cls <= TOL[dtype], f"class D={D} ({side})"
    assert err <= TOL[dtype]
    assert err_marg <= TOL[dtype]


# ---- D: the loop against the oracle's chain ----
@pytest.mark.parametrize("key", list(hc.LOOPS), ids=lambda k: f"{k[0]}-p{k[1]}c{k[2]}-lm{k[5]}")
def test_loop_equals_the_oracle_chain(mjx_mod, key):
    """hpr_er_run's loop restated with the oracle's parts on torch's CPU stream
    (chi0, biases0, then rand(n) per iteration).  float64: the device parts
    chained by hand give the oracle's s after every iteration, and hpr_er_run
    as a whole returns the oracle's num_steps, conf and mag_reached and leaves
    the generator where the oracle's is.  float32: the same s up to the first
    iteration whose oracle margin is below 1e-4 (61, 42, 27, 26 and 61
    iterations).  The float64 comparison needs a margin >= 1e-9 throughout;
    the pinned runs have it.  (With the count table in float the float32
    loop left the oracle at iteration 42 of the first run, margins >= 8e-4:
    the products of D saturating messages fell into float's denormals.)"""
    name, p, c, TT, seed, lm = key
    steps = hc.LOOPS[key][0]
    ref, upto32 = hc.check_loop(key)
    G = hc.built(name)
    plan = hc.plan(mjx_mod, G)
    for dtype in (F64, F32):
        upto = steps if dtype == F64 else upto32
        chi0, b0, gen = hc.initial_state(G, p, c, seed)
        chi, b = chi0.to(dtype).cuda(), b0.to(dtype).cuda()
        left = None
        for t in range(steps):
            chi = mjx_mod.HPr_dp_er(chi, b, plan, p, c, 1, lm * G.n, 0.4)
            marg = mjx_mod.marginals_comp_er(chi, plan, p, c)
            _, s = mjx_mod.new_biases_i(b, 0.3, 0.1, marg, t, generator=gen)
            same = np.array_equal(s.cpu().numpy(), ref["s"][t])
            assert same or t >= upto, (ID[dtype], t)
            if not same:
                left = t
                break
        print(f"D {key} {ID[dtype]}: compared on {upto} of {steps} iterations, leaves the oracle at {left}")
    gen = torch.Generator().manual_seed(seed)
    res = mjx_mod.hpr_er_run(plan=plan, p=p, c=c, TT=TT, seed=seed, dtype=F64, generator=gen,
                             lmbd_in=None if lm == 25 else lm * G.n)
    assert res["num_steps"][0] == steps
    assert np.array_equal(res["conf"][0], ref["conf"])
    assert res["mag_reached"][0] == ref["mag_reached"]
    assert torch.equal(torch.rand(4, dtype=F64, generator=gen), ref["next_rand"])


# ---- E: the register kernels and the class kernel on the same regular graph ----
@pytest.mark.parametrize("dtype", [F64, F32], ids=ID.get)
@pytest.mark.parametrize("d,p,c", [(3, 2, 1), (4, 1, 2)])
def test_class_kernel_equals_register_kernel_on_regular_graphs(mjx_mod, d, p, c, dtype):
    """Where the register kernels take the shape (mjx_hpr_update returns OK,
    so HPr_dp does not fall back), they and the class kernel on plan.er_plan
    agree to the dtype's bar, messages and marginals, and both meet the oracle."""
    n = 40
    edges = mjx_mod.random_regular_edges(d, n, seed=10 * d + p)
    plan = mjx_mod.HPRPlan(edges, n, d)
    inr, src = orc.incoming_rows(edges, plan.nbrs_host)
    ep = orc.edges_pos(edges, plan.nbrs_host)
    nc = 4 ** (p + c)
    for seed in (0, 1):
        g = torch.Generator().manual_seed(seed)
        chi0 = torch.rand((2 * plan.E, nc), dtype=F64, generator=g)
        chi0 = chi0 / chi0.sum(1, keepdim=True)
        b0 = torch.rand((n, 2), dtype=F64, generator=g)
        b0 = b0 / b0.sum(1, keepdim=True)
        chi, b = chi0.to(dtype).cuda(), b0.to(dtype).cuda()
        out = torch.empty_like(chi)
        wp, wm = mjx_mod.hpr._weights(25 * n, n)
        rc = mjx_mod.load_library().mjx_hpr_update(code(mjx_mod, dtype), chi.data_ptr(), out.data_ptr(), b.data_ptr(),
                                                   plan.nbr.data_ptr(), plan.in_row.data_ptr(),
                                                   plan.out_row.data_ptr(), n, d, p, c, 1, wp, wm, 0.4, None)
        assert rc == OK, "the register kernels take this shape"
        reg = mjx_mod.HPr_dp(chi, b, plan, p, c, 1, 25 * n, 0.4).cpu().numpy().astype(np.float64)
        assert np.array_equal(reg, out.cpu().numpy())
        cls = mjx_mod.HPr_dp_er(chi, b, plan.er_plan, p, c, 1, 25 * n, 0.4).cpu().numpy().astype(np.float64)
        want = orc.HPr_dp(chi0.numpy(), b0.numpy(), inr, src, n, d, p, c, 1, 25 * n, 0.4)
        errs = rownorm_err(cls, reg), rownorm_err(reg, want), rownorm_err(cls, want)
        m_reg = mjx_mod.marginals_comp(dev(want, dtype), plan, p, c).cpu().numpy().astype(np.float64)
        m_cls = mjx_mod.marginals_comp_er(dev(want, dtype), plan.er_plan, p, c).cpu().numpy().astype(np.float64)
        m_want = orc.marginals_comp(want, ep, p, c)
        merrs = [float(np.max(np.abs(x - y))) for x, y in ((m_cls, m_reg), (m_reg, m_want), (m_cls, m_want))]
        print(f"E d={d} p={p} c={c} {ID[dtype]} seed={seed}: chi {errs} marg {merrs} bar {TOL[dtype]}")
        assert max(errs) <= TOL[dtype], (seed, errs)
        assert max(merrs) <= TOL[dtype], (seed, merrs)


# ---- F: refusals, degenerate classes, a node of degree 40 ----
def test_scratch_bytes_limits_and_boundary_values(mjx_mod):
    """mjx_hpr_er_scratch_bytes: what it refuses, and its exact value at the
    classes on both sides of the LDS budget against the formula written out
    (tests/hpr_er_cases.py).  No (float64, T, D) is refused by the incoming
    messages' bytes alone: D * 2^(T-1) * 2^T * 8 > 160 KiB needs D >= 161 at
    T = 4 (the table limit refuses D >= 45), D >= 641 at T = 3 and more below
    (D <= 255 refuses them); so that branch is pinned only through the formula."""
    lib = mjx_mod.load_library()
    L = mjx_mod._lib
    sb = lib.mjx_hpr_er_scratch_bytes
    for dtype in (F32, F64):
        dt = code(mjx_mod, dtype)
        assert sb(dt, 256, 1, 1) == -1                    # D > 255
        assert sb(dt, 255, 1, 1) == hc.scratch_bytes(dtype, 255, 2) == 2 * 256 ** 2 * hc.SIZEOF[dtype]
        assert sb(dt, 0, 1, 1) == 0 and sb(dt, 0, 2, 2) == 0
        assert sb(dt, -1, 1, 1) == -1
        assert sb(dt, 3, 2, 3) == -1 and sb(dt, 3, 4, 1) == -1      # T = 5
        assert sb(dt, 3, 0, 2) == -1 and sb(dt, 3, 2, 0) == -1
        assert sb(dt, 45, 2, 2) == -1                     # 46^4 > 2^22 table entries
        assert sb(dt, 161, 2, 2) == -1
    assert 45 ** 4 <= 1 << 22 < 46 ** 4
    assert sb(L.MJX_F64, 44, 2, 2) == sb(L.MJX_F32, 44, 2, 2) == 8 * 45 ** 4 * 8     # double entries for both
    for bad in (0, 4, 8, 100, 105):
        assert sb(bad, 3, 1, 1) == -1, bad
    assert all(hc.incoming_bytes(F64, D, T) <= hc.K_MAX_LDS for T in (2, 3, 4) for D in range(256)
               if (D + 1) ** T <= 1 << 22)
    for T, (_, d_lds, d_slab) in hc.BOUNDARY.items():
        for dtype in (F64, F32):
            for p, c in hc.SPLITS[T]:
                for D in (d_lds - 1, d_lds, d_slab, d_slab + 1) + hc.MORE_SLAB[T][1]:
                    assert sb(code(mjx_mod, dtype), D, p, c) == hc.scratch_bytes(dtype, D, T), (T, dtype, D)
            assert hc.scratch_bytes(dtype, d_lds, T) == 0 < hc.scratch_bytes(dtype, d_slab, T)
    assert hc.scratch_bytes(F32, 7, 4) == 262144 and hc.scratch_bytes(F32, 17, 3) == 186624
    # T = 4, D = 6: (8 * 7^4 + 6 * 8 * 16) * 8 B; T = 3, D = 16 is the largest request for dynamic LDS of any class
    assert hc.table_bytes(F64, 6, 4) + hc.incoming_bytes(F64, 6, 4) == 159808 <= hc.K_MAX_LDS
    assert hc.table_bytes(F64, 16, 3) + hc.incoming_bytes(F64, 16, 3) == 161312 <= hc.K_MAX_LDS


def test_update_class_refusals_leave_the_output_alone(mjx_mod):
    """Every call here returns before a launch (mjx_hpr_er_update_class checks
    m, the pointers, the geometry, then update_impl the slab, in that order);
    the pointers are those of a real class all the same."""
    G = hc.built("slab_t4")
    plan = hc.plan(mjx_mod, G)
    lib = mjx_mod.load_library()
    L = mjx_mod._lib
    p, c = 2, 2
    D, rows, inc, src, m = plan.classes[-1]
    assert D == 10
    chi0, b0, _, _ = hc.oracle_step("slab_t4", p, c, 1)
    for dtype in (F64, F32):
        dt = code(mjx_mod, dtype)
        chi, b = dev(chi0, dtype), dev(b0, dtype)
        out = torch.full_like(chi, -7.0)
        tab = lib.mjx_hpr_er_scratch_bytes(dt, D, p, c)
        slab = torch.empty(tab, dtype=torch.uint8, device="cuda")

        def call(chi_in=chi.data_ptr(), chi_out=out.data_ptr(), m=m, D=D, attr=1, scratch=slab.data_ptr(),
                 nbytes=tab, dt=dt, inc_=inc.data_ptr()):
            return lib.mjx_hpr_er_update_class(dt, chi_in, chi_out, b.data_ptr(), rows.data_ptr(), inc_,
                                               src.data_ptr(), m, D, p, c, attr, 1.0, 1.0, 0.4, scratch, nbytes, None)

        assert lib.mjx_hpr_er_update_class(dt, None, None, None, None, None, None, -1, D, p, c, 1, 1.0, 1.0, 0.4,
                                           None, 0, None) == EINVAL
        assert lib.mjx_hpr_er_update_class(dt, None, None, None, None, None, None, 0, D, p, c, 1, 1.0, 1.0, 0.4,
                                           None, 0, None) == OK
        assert call(m=-1) == EINVAL
        assert call(chi_out=chi.data_ptr()) == EINVAL      # in place
        assert call(chi_in=None) == EINVAL
        assert call(inc_=None) == EINVAL                   # D > 0 needs the incoming rows
        assert call(attr=0) == ERANGE
        assert call(D=256) == ERANGE
        assert call(D=45) == ERANGE
        assert call(scratch=None, nbytes=0) == ERANGE      # a slab class without a slab
        assert call(scratch=None, nbytes=tab) == ERANGE
        assert call(nbytes=tab - 1) == ERANGE              # a slab smaller than one table
        assert call(dt=0) == EINVAL
        torch.cuda.synchronize()
        assert torch.equal(out, torch.full_like(chi, -7.0))
    assert L.MJX_EINVAL == EINVAL and L.MJX_ERANGE == ERANGE


def test_plan_scratch_names_the_unsupported_class(mjx_mod):
    plan = hc.plan(mjx_mod, hc.built("path3"))
    assert plan.scratch(F64, 2, 2) is None                # classes 0 and 1: LDS
    held = plan.classes
    plan.classes = held + [(45, None, None, None, 3)]     # patched on the host: nothing is uploaded or run
    try:
        with pytest.raises(mjx_mod.MjxError, match="D=45"):
            plan.scratch(F64, 2, 2)
        with pytest.raises(mjx_mod.MjxError, match="D=45"):
            plan.check_sizes(F32, 1, 3)
        assert plan.scratch(F64, 2, 1) is not None        # 46^3 entries: a slab class at T = 3
    finally:
        plan.classes = held


@pytest.mark.parametrize("dtype", [F64, F32], ids=ID.get)
@pytest.mark.parametrize("name,p,c", [("edge2", 1, 1), ("edge2", 2, 2), ("path3", 1, 1), ("path3", 1, 2),
                                       ("path3", 3, 1)])
def test_leaf_messages_on_the_smallest_graphs(mjx_mod, name, p, c, dtype):
    """A single edge (both messages in class D = 0, n = 2) and a path of three
    nodes (classes 0 and 1): one step and the marginals, attr = +1 and -1."""
    G = hc.built(name)
    assert G.class_set == ((0,) if name == "edge2" else (0, 1))
    plan = hc.plan(mjx_mod, G)
    for attr in (1, -1):
        chi, b, want, want_marg = hc.oracle_step(name, p, c, attr)
        got = step(mjx_mod, plan, chi, b, p, c, attr, dtype).cpu().numpy()
        assert rownorm_err(got, want) <= TOL[dtype], attr
        marg = mjx_mod.marginals_comp_er(dev(want, dtype), plan, p, c).cpu().numpy()
        assert float(np.max(np.abs(marg - want_marg))) <= TOL[dtype], attr


@pytest.mark.parametrize("dtype", [F64, F32], ids=ID.get)
def test_marginals_of_a_degree_40_node(mjx_mod, dtype):
    """A node of degree 40 (class D = 39, in LDS at T = 2): k_hpr_node_marg_csr
    multiplies 40 factors in the working dtype.  Marginals of the random start
    (factors near 1/2: the centre's two products are of one size) and of the
    messages after a step (one product far below the other), and the step."""
    G = hc.built("star40")
    hub = G.hubs[0]
    assert G.deg[hub] == 40 and mjx_mod.load_library().mjx_hpr_er_scratch_bytes(code(mjx_mod, dtype), 39, 1, 1) == 0
    plan = hc.plan(mjx_mod, G)
    for attr in (1, -1):
        chi, b, want, want_marg = hc.oracle_step("star40", 1, 1, attr)
        got = step(mjx_mod, plan, chi, b, 1, 1, attr, dtype).cpu().numpy()
        rows = G.rows_of(39)
        err, err_hub = rownorm_err(got, want), rownorm_err(got[rows], want[rows])
        marg0 = orc.marginals_comp_csr(chi, G.rp, G.out_rows, 1, 1)
        e0 = np.abs(mjx_mod.marginals_comp_er(dev(chi, dtype), plan, 1, 1).cpu().numpy() - marg0)
        e1 = np.abs(mjx_mod.marginals_comp_er(dev(want, dtype), plan, 1, 1).cpu().numpy() - want_marg)
        print(f"F star40 {ID[dtype]} attr={attr}: step {err:.3e} (class 39: {err_hub:.3e}); marginals start "
              f"{e0.max():.3e} (centre {e0[hub].max():.3e}, centre = {marg0[hub]}), after a step {e1.max():.3e} "
              f"(centre {e1[hub].max():.3e}); bar {TOL[dtype]}")
        assert err_hub <= TOL[dtype] and err <= TOL[dtype], attr
        assert e0[hub].max() <= TOL[dtype] and e1[hub].max() <= TOL[dtype], "the centre"
        assert e0.max() <= TOL[dtype] and e1.max() <= TOL[dtype], attr
