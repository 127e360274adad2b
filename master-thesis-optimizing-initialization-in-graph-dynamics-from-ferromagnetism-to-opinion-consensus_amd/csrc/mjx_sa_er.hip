// Simulated annealing on irregular graphs (CSR: Erdos-Renyi and any other
// symmetric adjacency), the loop of code/SA_RRG.py:65-85 scored with the
// notebook's ER end state (code/ER_BDCM_entropy.ipynb nb:113-123: sign(2S+s),
// a degree-0 node keeps its spin).  Row entries count with multiplicity, so a
// self-loop or a doubled edge contributes as often as it is listed.
//
// The MT19937 replay, the Metropolis test and the schedule are the ones of the
// regular-graph unit (mjx_sa_core.h); the full-rollout step reuses its propose
// and accept kernels around mjx_rollout_csr_rp.  New here is the light-cone
// step for graphs whose balls have no d-regular size bound:
//
//   * mjx_sa_csr_ball_bound computes cap_t = min(n, max_v B_t(v)) with
//     B_0 = 1, B_t(v) = 1 + sum_{k in row(v)} B_{t-1}(k): the number of walks of
//     length <= t from v.  Every node within distance t of a proposal is the end
//     of such a walk, so cap_t bounds the candidates of level t and hence the
//     nodes changed at level t, for any proposal and any configuration.
//   * k_sa_er_lightcone keeps, per lane (replica), T+2 lists: the changed nodes
//     of levels 0..T and the candidate list.  Entry q of a list lives in LDS
//     for q < E ([list][q][lane], conflict free) and in the caller's HBM spill
//     area beyond ([column][slot][lane]: the lanes of a wave touch one 256-B
//     row per slot), sized by the caps.  Nothing is truncated: a graph within
//     its caps is evaluated exactly, in LDS or not.
//
// A flip at i changes level t only where the flip's level-(t-1) changes are
// in-neighbours; the candidates are gathered from the changed nodes' own rows,
// which is why the adjacency must be symmetric (as a multiset of directed
// entries): row(v) then lists every node that reads v.
//
// Compiled with -ffp-contract=off (delta_H's operation order, mjx_sa_core.h).
#include "mjx_sa_core.h"
#include <algorithm>

#pragma clang fp contract(off)

namespace mjx {

constexpr int ER_MAXT = 6;
constexpr int ER_LDS_DEFAULT = 32;          // list entries per lane kept in LDS (lds_entries = 0)
constexpr size_t kErLdsMax = 150 * 1024;

struct ErCone {
    u64* s[ER_MAXT + 1];          // s[0] = configuration, s[t] = onestep^t(s[0]); word (v, col) at v*W + col
    int E;                        // entries per lane and list in LDS
    int cap[ER_MAXT + 2];         // capacity of list l: changed nodes of level l (l <= T), candidates (l = T+1)
    int64_t soff[ER_MAXT + 2];    // first spill slot of list l
    int64_t S;                    // spill slots per replica
    uint32_t* spill;              // [W][S][64]
};

// proposals evaluated / proposals with a list longer than the LDS part
__device__ unsigned long long mjx_sa_er_stats[2];

// B_t from B_{t-1} (prev == nullptr: B_0 = 1 everywhere), saturating at n, and its maximum
__global__ void __launch_bounds__(kBlock) k_er_ball_level(const int64_t* __restrict__ row_ptr,
                                                          const int32_t* __restrict__ col, int64_t n,
                                                          const int64_t* __restrict__ prev, int64_t* __restrict__ cur,
                                                          unsigned long long* __restrict__ mx) {
    int64_t best = 0;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        int64_t acc = 1;
        if (prev) {
            const int64_t e1 = row_ptr[v + 1];
            for (int64_t e = row_ptr[v]; e < e1 && acc < n; ++e) {
                acc += prev[col[e]];                 // both <= n: no overflow
                if (acc > n) acc = n;
            }
        }
        if (acc > n) acc = n;
        cur[v] = acc;
        best = acc > best ? acc : best;
    }
    if (best > 0) atomicMax(mx, (unsigned long long)best);
}

// One wave = the replicas of one word column (or 64/split of them), persistent
// over nsteps; proposals are drawn in the step (the stream stands exactly where
// numpy's would).  done = 3: a list outgrew its cap (caps not from
// mjx_sa_csr_ball_bound of this graph); the replica stops, nothing is written
// out of bounds.
__global__ void __launch_bounds__(64) k_sa_er_lightcone(const int64_t* __restrict__ row_ptr,
                                                        const int32_t* __restrict__ colidx, int64_t n, int64_t R,
                                                        int64_t W, ErCone C, int T, mjx_sa_state st, int64_t nsteps,
                                                        double par_a, double par_b, double a_cap, double b_cap,
                                                        int64_t t_cap, int split) {
    extern __shared__ uint32_t er_lists[];
    __shared__ uint32_t twist_buf[MT_N];
    const int lane = threadIdx.x;
    const int per = 64 / split;
    const int64_t col = blockIdx.x % W;
    const int rl = (int)(blockIdx.x / W) * per + lane;        // bit of this lane's replica in the column
    const int64_t r = col * 64 + rl;
    const bool live = lane < per && r < R;
    const u64 bit = 1ull << (rl & 63);
    const int E = C.E;
    uint32_t* lds = er_lists + lane;
    uint32_t* sp = C.spill + col * C.S * 64 + (rl & 63);
    auto get = [&](int l, int q) -> uint32_t {
        return q < E ? lds[(l * E + q) * 64] : sp[(C.soff[l] + (q - E)) * 64];
    };
    auto put = [&](int l, int q, uint32_t x) {
        if (q < E) lds[(l * E + q) * 64] = x;
        else sp[(C.soff[l] + (q - E)) * 64] = x;
    };
    // index of the entry of list l (cntl entries) whose node is `key`, else -1.  The LDS
    // part is scanned entry by entry; the spill part in batches of eight loads issued
    // together (a hub's 200-entry lists otherwise cost one memory round trip per entry)
    auto find = [&](int l, int cntl, uint32_t key) -> int {
        const uint32_t* pl = lds + l * E * 64;
        const int nl = cntl < E ? cntl : E;
        for (int q = 0; q < nl; ++q)
            if ((pl[q * 64] & 0x7fffffffu) == key) return q;
        const int m = cntl - E;
        if (m > 0) {
            const uint32_t* ps = sp + C.soff[l] * 64;
            for (int q0 = 0; q0 < m; q0 += 8) {
                uint32_t x[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int q = (q0 + k < m) ? q0 + k : m - 1;          // never past the list
                    x[k] = ps[(int64_t)q * 64];
                }
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if ((x[k] & 0x7fffffffu) == key) return E + ((q0 + k < m) ? q0 + k : m - 1);
            }
        }
        return -1;
    };
    WaveMT g{st.mt, twist_buf, r, live ? st.mt_idx[r] : MT_N, lane};
    double a = live ? st.a[r] : 0.0, b = live ? st.b[r] : 0.0;
    int64_t t = live ? st.t[r] : 0, sum_end = live ? st.sum_end[r] : 0;
    int done = live ? st.done[r] : 1;
    int ties = 0;
    unsigned long long n_prop = 0, n_spill = 0;
    const int UL = T + 1;                                     // the candidate list
    for (int64_t step = 0; step < nsteps; ++step) {
        const bool active = live && done == 0;
        uint32_t i = 0;
        double u = 0.0;
        g.propose(active, n, i, u);
        if (active) {
            int cnt[ER_MAXT + 1];
            bool ovf = false;
            int longest = 1;
            // level 0: the flip itself (entry = node | new value << 31)
            const u64 w0 = ld_word(C.s[0] + (int64_t)i * W + col);
            const int old_i = (w0 & bit) ? 1 : 0;
            put(0, 0, i | (old_i ? 0u : 0x80000000u));
            cnt[0] = 1;
            int lv = 1;
            for (; lv <= T && !ovf; ++lv) {
                const int np = cnt[lv - 1];
                const u64* prevw = C.s[lv - 1];
                // value of node k at level lv-1 as the proposal sees it: its entry in the
                // level's change list if it has one, else the cached word w
                auto val = [&](int32_t k, u64 w) -> uint32_t {
                    const int q = find(lv - 1, np, (uint32_t)k);
                    if (q >= 0) return get(lv - 1, q) >> 31;
                    return (w & bit) ? 1u : 0u;
                };
                // rows are read eight entries at a time, the eight loads issued together, and
                // so are the level words of those eight neighbours: a row costs a few memory
                // round trips instead of two per entry (indices clamped to the row, never past it)
                // candidates: the nodes changed at level lv-1 and the nodes of their rows
                int nu = 0;
                auto add = [&](int32_t v) {
                    if (find(UL, nu, (uint32_t)v) >= 0) return;
                    if (nu >= C.cap[UL]) { ovf = true; return; }
                    put(UL, nu, (uint32_t)v);
                    ++nu;
                };
                for (int q = 0; q < np && !ovf; ++q) {
                    const int32_t v = (int32_t)(get(lv - 1, q) & 0x7fffffffu);
                    add(v);
                    const int64_t e1 = row_ptr[v + 1];
                    for (int64_t e = row_ptr[v]; e < e1 && !ovf; e += 8) {
                        int32_t k[8];
#pragma unroll
                        for (int m = 0; m < 8; ++m) k[m] = colidx[(e + m < e1) ? e + m : e1 - 1];
#pragma unroll
                        for (int m = 0; m < 8; ++m)
                            if (e + m < e1 && !ovf) add(k[m]);
                    }
                }
                longest = nu > longest ? nu : longest;
                int nc = 0;
                for (int q = 0; q < nu && !ovf; ++q) {
                    const int32_t j = (int32_t)get(UL, q);
                    const int64_t e0 = row_ptr[j], e1 = row_ptr[j + 1];
                    const int64_t dd = e1 - e0;
                    const u64 wown = ld_word(prevw + (int64_t)j * W + col);
                    const u64 wnext = ld_word(C.s[lv] + (int64_t)j * W + col);
                    int64_t ones = 0;
                    for (int64_t e = e0; e < e1; e += 8) {
                        int32_t k[8];
                        u64 w[8];
#pragma unroll
                        for (int m = 0; m < 8; ++m) k[m] = colidx[(e + m < e1) ? e + m : e1 - 1];
#pragma unroll
                        for (int m = 0; m < 8; ++m) w[m] = ld_word(prevw + (int64_t)k[m] * W + col);
#pragma unroll
                        for (int m = 0; m < 8; ++m)
                            if (e + m < e1) ones += (int64_t)val(k[m], w[m]);
                    }
                    const uint32_t own = val(j, wown);
                    // sign(2S + s), S = 2*ones - dd (nb:113-117); dd = 0 keeps the spin
                    const uint32_t nb = (2 * ones > dd) ? 1u : ((2 * ones < dd) ? 0u : own);
                    const uint32_t ob = (wnext & bit) ? 1u : 0u;
                    if (nb != ob) {
                        if (nc >= C.cap[lv]) { ovf = true; break; }
                        put(lv, nc, (uint32_t)j | (nb << 31));
                        ++nc;
                    }
                }
                cnt[lv] = nc;
                if (nc == 0) break;          // nothing propagates further
            }
            const bool reached = lv > T;     // level T has changes (else the walk stopped at level lv)
            for (int q = lv + 1; q <= T; ++q) cnt[q] = 0;
            ++n_prop;
            if (longest > E) ++n_spill;
            if (ovf) {
                done = 3;
                if (st.tr_i) st.tr_i[step * R + r] = (int32_t)i;
                if (st.tr_acc) st.tr_acc[step * R + r] = -1;
                if (st.tr_sum) st.tr_sum[step * R + r] = sum_end;
                if (st.tr_dE) st.tr_dE[step * R + r] = 0.0;
            } else {
                int64_t ds = 0;
                if (reached)
                    for (int q = 0; q < cnt[T]; ++q) ds += (get(T, q) >> 31) ? 2 : -2;
                const int64_t sum_new = sum_end + ds;
                const SaVerdict vd = sa_metropolis(a, b, old_i ? 1.0 : -1.0, sum_end, sum_new, n, u);
                if (vd.tie) ++ties;
                if (vd.acc) {                                            // (code/SA_RRG.py:77)
                    for (int l = 0; l <= T; ++l)
                        for (int q = 0; q < cnt[l]; ++q) {
                            const int64_t j = (int64_t)(get(l, q) & 0x7fffffffu);
                            atomicXor((unsigned long long*)(C.s[l] + j * W + col), (unsigned long long)bit);
                        }
                    sum_end = sum_new;
                }
                sa_advance(a, b, t, done, sum_end, n, par_a, par_b, a_cap, b_cap, t_cap);   // (code/SA_RRG.py:80-85)
                if (st.tr_i) st.tr_i[step * R + r] = (int32_t)i;
                if (st.tr_acc) st.tr_acc[step * R + r] = vd.acc ? 1 : 0;
                if (st.tr_sum) st.tr_sum[step * R + r] = sum_end;
                if (st.tr_dE) st.tr_dE[step * R + r] = vd.dE;
            }
        } else if (live) {
            if (st.tr_i) st.tr_i[step * R + r] = -1;
            if (st.tr_acc) st.tr_acc[step * R + r] = -1;
            if (st.tr_sum) st.tr_sum[step * R + r] = sum_end;
            if (st.tr_dE) st.tr_dE[step * R + r] = 0.0;
        }
        // this wave's flips must land before its next reads of the same words
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (live) {
        st.mt_idx[r] = g.idx;
        st.a[r] = a;
        st.b[r] = b;
        st.t[r] = t;
        st.sum_end[r] = sum_end;
        st.done[r] = done;
        if (st.tr_tie) st.tr_tie[r] += ties;
        if (n_prop) atomicAdd(&mjx_sa_er_stats[0], n_prop);
        if (n_spill) atomicAdd(&mjx_sa_er_stats[1], n_spill);
    }
}

// list capacities, LDS part and spill slots from the caps of mjx_sa_csr_ball_bound
static int er_plan(int T, const int64_t* caps, int lds_entries, ErCone& C) {
    if (T < 1 || T > ER_MAXT || !caps || lds_entries < 0) return MJX_EINVAL;
    C.E = lds_entries ? lds_entries : ER_LDS_DEFAULT;
    if ((size_t)(T + 2) * (size_t)C.E * 64 * 4 > kErLdsMax) return MJX_EINVAL;
    int64_t S = 0;
    for (int l = 0; l <= T + 1; ++l) {
        const int64_t cap = (l == 0) ? 1 : caps[l <= T ? l : T];
        if (cap < 1 || cap > (int64_t)INT32_MAX) return MJX_EINVAL;
        C.cap[l] = (int)cap;
        C.soff[l] = S;
        S += std::max<int64_t>(0, cap - C.E);
    }
    for (int l = T + 2; l < ER_MAXT + 2; ++l) { C.cap[l] = 0; C.soff[l] = S; }
    C.S = S;
    return MJX_OK;
}

// waves per word column: fill the CUs with about two waves each (LDS allowing)
static int er_split(int64_t W, size_t lds) {
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(2, (int64_t)(160 * 1024) / (int64_t)std::max<size_t>(lds, 1)));
    const int64_t target = (int64_t)device_cus() * per_cu;
    int s = 1;
    while (s < 64 && W * s * 2 <= target) s *= 2;
    return s;
}

}  // namespace mjx

using namespace mjx;

static int csr_init_finish(const int64_t* row_ptr, const int32_t* col, int64_t n, int T, int64_t R, double a0,
                           double b0, uint64_t* s, uint64_t* tmp1, uint64_t* tmp2, const mjx_sa_state& st,
                           void* stream) {
    hipStream_t hs = as_stream(stream);
    MJX_HIP(hipMemsetAsync(st.cnt, 0, (size_t)R * sizeof(unsigned long long), hs), "sa_csr_init memset");
    const int rc = mjx_rollout_csr_rp(row_ptr, col, n, (R + 63) / 64, s, tmp1, tmp2, T, st.cnt, stream);
    if (rc) return rc;
    return sa_init_state(n, R, a0, b0, st, hs);
}

static int csr_args(const int64_t* row_ptr, const int32_t* col, int64_t n, int p, int c, int64_t R) {
    (void)col;                                   // a graph without edges has no col array
    if (!row_ptr || n < 2 || R < 1 || p < 0 || c < 0 || p + c < 1) return MJX_EINVAL;
    if (n > (int64_t)INT32_MAX) return MJX_ERANGE;
    return MJX_OK;
}

extern "C" int mjx_sa_csr_init(const int64_t* row_ptr, const int32_t* col, int64_t n, int p, int c, int64_t R,
                               const uint32_t* seeds, double a0, double b0, uint64_t* s, uint64_t* tmp1,
                               uint64_t* tmp2, mjx_sa_state* stp, void* stream) {
    if (int rc = csr_args(row_ptr, col, n, p, c, R)) return rc;
    if (!stp || !seeds || !s || !tmp1) return MJX_EINVAL;
    const mjx_sa_state st = *stp;
    const int T = p + c - 1;
    if (!sa_state_complete(st) || st.rep_graph || (T >= 2 && !tmp2)) return MJX_EINVAL;
    if (int rc = sa_draw_s0(n, R, seeds, s, tmp1, st, as_stream(stream))) return rc;
    return csr_init_finish(row_ptr, col, n, T, R, a0, b0, s, tmp1, tmp2, st, stream);
}

extern "C" int mjx_sa_csr_init_mt(const int64_t* row_ptr, const int32_t* col, int64_t n, int p, int c, int64_t R,
                                  const uint32_t* mt_in, const int32_t* idx_in, double a0, double b0, uint64_t* s,
                                  uint64_t* tmp1, uint64_t* tmp2, mjx_sa_state* stp, void* stream) {
    if (int rc = csr_args(row_ptr, col, n, p, c, R)) return rc;
    if (!stp || !mt_in || !idx_in || !s || !tmp1) return MJX_EINVAL;
    const mjx_sa_state st = *stp;
    const int T = p + c - 1;
    if (!sa_state_complete(st) || st.rep_graph || (T >= 2 && !tmp2)) return MJX_EINVAL;
    if (int rc = sa_draw_s0_mt(n, R, mt_in, idx_in, s, st, as_stream(stream))) return rc;
    return csr_init_finish(row_ptr, col, n, T, R, a0, b0, s, tmp1, tmp2, st, stream);
}

extern "C" int mjx_sa_csr_steps(const int64_t* row_ptr, const int32_t* col, int64_t n, int p, int c, int64_t R,
                                uint64_t* s, uint64_t* tmp1, uint64_t* tmp2, mjx_sa_state* stp, int64_t nsteps,
                                double par_a, double par_b, double a_cap, double b_cap, int64_t t_cap, void* stream) {
    if (int rc = csr_args(row_ptr, col, n, p, c, R)) return rc;
    if (!stp || !s || !tmp1 || nsteps < 0) return MJX_EINVAL;
    const mjx_sa_state st = *stp;
    const int T = p + c - 1;
    if (!sa_state_complete(st) || st.rep_graph || st.philox_key || (T >= 2 && !tmp2)) return MJX_EINVAL;
    hipStream_t hs = as_stream(stream);
    for (int64_t k = 0; k < nsteps; ++k) {
        int rc = sa_propose(n, R, s, st, k, hs);
        if (rc) return rc;
        MJX_HIP(hipMemsetAsync(st.cnt, 0, (size_t)R * sizeof(unsigned long long), hs), "sa_csr_steps memset");
        if ((rc = mjx_rollout_csr_rp(row_ptr, col, n, (R + 63) / 64, s, tmp1, tmp2, T, st.cnt, stream))) return rc;
        if ((rc = sa_accept(n, R, s, st, k, par_a, par_b, a_cap, b_cap, t_cap, hs))) return rc;
    }
    return MJX_OK;
}

extern "C" int64_t mjx_sa_csr_ball_work_bytes(int64_t n) {
    return n < 0 ? -1 : (2 * n + ER_MAXT + 2) * (int64_t)sizeof(int64_t);
}

extern "C" int mjx_sa_csr_ball_bound(const int64_t* row_ptr, const int32_t* col, int64_t n, int T, void* work,
                                     int64_t* bound_out, void* stream) {
    if (!row_ptr || !work || !bound_out || n < 1 || T < 0 || T > ER_MAXT) return MJX_EINVAL;
    if (n > (int64_t)INT32_MAX) return MJX_ERANGE;
    hipStream_t hs = as_stream(stream);
    int64_t* B[2] = {(int64_t*)work, (int64_t*)work + n};
    unsigned long long* mx = (unsigned long long*)((int64_t*)work + 2 * n);
    MJX_HIP(hipMemsetAsync(mx, 0, (size_t)(T + 1) * sizeof(unsigned long long), hs), "ball_bound memset");
    for (int t = 0; t <= T; ++t) {
        k_er_ball_level<<<grid_for(n), kBlock, 0, hs>>>(row_ptr, col, n, t ? B[(t - 1) & 1] : nullptr, B[t & 1], mx + t);
        MJX_LAUNCH_CHECK("k_er_ball_level");
    }
    MJX_HIP(hipMemcpyAsync(bound_out, mx, (size_t)(T + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, hs),
            "ball_bound copy");
    MJX_HIP(hipStreamSynchronize(hs), "ball_bound sync");       // setup call: the caps size the spill area
    return MJX_OK;
}

extern "C" int64_t mjx_sa_csr_lightcone_lds(int T, int lds_entries) {
    if (T < 1 || T > ER_MAXT || lds_entries < 0) return -1;
    const size_t b = (size_t)(T + 2) * (size_t)(lds_entries ? lds_entries : ER_LDS_DEFAULT) * 64 * 4;
    return b > kErLdsMax ? -1 : (int64_t)b;
}

extern "C" int64_t mjx_sa_csr_lightcone_scratch_bytes(int64_t R, int T, const int64_t* caps, int lds_entries) {
    ErCone C;
    if (R < 1 || er_plan(T, caps, lds_entries, C)) return -1;
    return ((R + 63) / 64) * C.S * 64 * (int64_t)sizeof(uint32_t);
}

extern "C" int mjx_sa_csr_lightcone_prepare(const int64_t* row_ptr, const int32_t* col, int64_t n, int p, int c,
                                            int64_t R, const uint64_t* s, uint64_t* const* levels, void* stream) {
    const int T = p + c - 1;
    if (!row_ptr || !s || !levels || n < 2 || R < 1 || T < 1 || T > ER_MAXT) return MJX_EINVAL;
    const uint64_t* src = s;
    for (int t = 0; t < T; ++t) {
        if (!levels[t]) return MJX_EINVAL;
        const int rc = mjx_rollout_csr_rp(row_ptr, col, n, (R + 63) / 64, src, levels[t], nullptr, 1, nullptr, stream);
        if (rc) return rc;
        src = levels[t];
    }
    return MJX_OK;
}

extern "C" int mjx_sa_csr_lightcone_steps(const int64_t* row_ptr, const int32_t* col, int64_t n, int p, int c,
                                          int64_t R, uint64_t* s, uint64_t* const* levels, mjx_sa_state* stp,
                                          int64_t nsteps, double par_a, double par_b, double a_cap, double b_cap,
                                          int64_t t_cap, const int64_t* caps, int lds_entries, void* spill,
                                          int64_t spill_bytes, void* stream) {
    const int T = p + c - 1;
    if (!stp || !row_ptr || !s || !levels || !caps || n < 2 || R < 1 || p < 0 || c < 0 || nsteps < 0)
        return MJX_EINVAL;
    if (T < 1 || T > ER_MAXT) return MJX_EINVAL;
    if (n > (int64_t)INT32_MAX) return MJX_ERANGE;
    const mjx_sa_state st = *stp;
    if (st.rep_graph || st.philox_key || !sa_state_complete(st)) return MJX_EINVAL;
    ErCone C;
    if (int rc = er_plan(T, caps, lds_entries, C)) return rc;
    const int64_t W = (R + 63) / 64;
    const int64_t need = W * C.S * 64 * (int64_t)sizeof(uint32_t);
    if (spill_bytes < need || (need > 0 && !spill)) return MJX_EINVAL;
    C.spill = (uint32_t*)spill;
    C.s[0] = (u64*)s;
    for (int t = 1; t <= ER_MAXT; ++t) C.s[t] = nullptr;
    for (int t = 1; t <= T; ++t) {
        if (!levels[t - 1]) return MJX_EINVAL;
        C.s[t] = (u64*)levels[t - 1];
    }
    if (nsteps == 0) return MJX_OK;
    const size_t lds = (size_t)(T + 2) * (size_t)C.E * 64 * 4;
    const int split = st.opt_split ? st.opt_split : er_split(W, lds);
    if (split < 1 || split > 64 || (64 % split)) return MJX_EINVAL;
    if (W * split > (int64_t)INT32_MAX) return MJX_ERANGE;
    MJX_HIP(set_max_lds(k_sa_er_lightcone, (int)lds), "sa_csr_lightcone lds");
    k_sa_er_lightcone<<<(unsigned)(W * split), 64, lds, as_stream(stream)>>>(row_ptr, col, n, R, W, C, T, st, nsteps,
                                                                              par_a, par_b, a_cap, b_cap, t_cap, split);
    MJX_LAUNCH_CHECK("k_sa_er_lightcone");
    return MJX_OK;
}

extern "C" int mjx_sa_csr_lightcone_stats(unsigned long long* out2, int reset) {
    if (!out2) return MJX_EINVAL;
    MJX_HIP(hipMemcpyFromSymbol(out2, HIP_SYMBOL(mjx_sa_er_stats), 2 * sizeof(unsigned long long)), "sa_csr stats read");
    if (reset) {
        const unsigned long long z[2] = {0, 0};
        MJX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(mjx_sa_er_stats), z, sizeof(z)), "sa_csr stats reset");
    }
    return MJX_OK;
}
