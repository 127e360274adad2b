// Pieces shared by the simulated-annealing translation units (mjx_sa.hip: random
// regular graphs, ELL; mjx_sa_er.hip: irregular graphs, CSR): the in-step
// MT19937 draw of a wave's replicas, the Metropolis test with delta_H in the
// reference's float64 operation order (code/SA_RRG.py:37,75-76), the annealing
// schedule and termination tests (:80-85), and the host launchers of the
// graph-independent kernels that live in mjx_sa.hip.  Every includer is
// compiled with -ffp-contract=off.
#pragma once
#include "mjx_common.h"
#include "mjx_mt.h"
#include <math.h>

#pragma clang fp contract(off)

namespace mjx {

__device__ __forceinline__ uint32_t ld_nc(const uint32_t* p) {
    // bypass the CU's L1: the words may have been rewritten by this wave's
    // own cooperative twist earlier in this launch
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// level / configuration words: agent-scope (L1 bypassing) loads, because the
// wave's own accepted flips are atomics performed in L2
__device__ __forceinline__ u64 ld_word(const u64* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline void coop_twist(uint32_t* __restrict__ g, uint32_t* buf, int lane) {
    for (int k = lane; k < MT_N; k += 64) buf[k] = ld_nc(g + k);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    lds_twist(buf, lane);
    for (int k = lane; k < MT_N; k += 64) g[k] = buf[k];
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One thread per replica, MT state replica-major in global memory
// mt[r*624 + k].  A lane that runs out of words gets its state twisted
// cooperatively by its whole wave through a 624-word LDS buffer.
struct WaveMT {
    uint32_t* mt;      // all replicas
    uint32_t* buf;     // this wave's LDS twist buffer
    int64_t r;
    int idx;
    int lane;
    // wave-uniform call: lanes with want == false still participate
    __device__ __forceinline__ uint32_t draw(bool want) {
        const bool tw = want && idx >= MT_N;
        u64 m = __ballot(tw);
        const int64_t base = r - lane;
        while (m) {
            const int l = __ffsll((unsigned long long)m) - 1;
            coop_twist(mt + (base + l) * MT_N, buf, lane);
            m &= m - 1;
        }
        if (tw) idx = 0;
        uint32_t y = 0;
        if (want) y = mt_temper(ld_nc(mt + r * MT_N + idx++));
        return y;
    }
    // randint(low=0, high=n) (code/SA_RRG.py:73: numpy legacy masked rejection on
    // 32-bit words) then rand() (:76); wave-uniform call, `active` lanes draw
    __device__ __forceinline__ void propose(bool active, int64_t n, uint32_t& i, double& u) {
        const uint64_t rng = (uint64_t)(n - 1);
        uint32_t mask = (uint32_t)rng;
        mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
        bool pending = active && rng > 0;
        i = 0;
        while (__ballot(pending)) {
            const uint32_t y = draw(pending);
            if (pending) {
                const uint32_t v = y & mask;
                if (v <= (uint32_t)rng) { i = v; pending = false; }
            }
        }
        const uint32_t w1 = draw(active);
        const uint32_t w2 = draw(active);
        u = mt_double(w1, w2);
    }
};

// The Metropolis test of one proposal (code/SA_RRG.py:37,75-76):
// delta_H = ((-2*a)*s_i + b*(sum(s_end) - sum(s_end of the flip)))/n with
// separately rounded operations, prob_accept = min(1, exp(-delta_H)), accepted
// when u < prob_accept.  `tie`: u within 4 ulp of exp(-delta_H) (a decision a
// differently rounded exp could turn; counted in tr_tie).
struct SaVerdict {
    double dE;
    bool acc;
    bool tie;
};

__device__ __forceinline__ SaVerdict sa_metropolis(double a, double b, double si, int64_t sum_old, int64_t sum_new,
                                                   int64_t n, double u) {
    const double t1 = (-2.0 * a) * si;
    const double t2 = b * (double)(sum_old - sum_new);
    const double dE = (t1 + t2) / (double)n;
    const double e = exp(-dE);
    const double prob = (e < 1.0) ? e : 1.0;
    SaVerdict v;
    v.dE = dE;
    v.acc = u < prob;
    v.tie = e < 1.0 && fabs(u - e) <= 4.0 * (nextafter(e, 2.0) - e);
    return v;
}

// annealing schedule (code/SA_RRG.py:80-81), step count (:82) and the loop's
// termination tests (:84 t cap -> 2, :85/:72 consensus of the end state -> 1)
__device__ __forceinline__ void sa_advance(double& a, double& b, int64_t& t, int& done, int64_t sum_cur, int64_t n,
                                           double par_a, double par_b, double a_cap, double b_cap, int64_t t_cap) {
    if (a < a_cap) a = par_a * a;
    if (b < b_cap) b = par_b * b;
    t += 1;
    if (t > t_cap) done = 2;
    else if (sum_cur == n) done = 1;
}

// Host launchers of kernels in mjx_sa.hip that do not read the graph:
// s0 = 2*binomial(1, .5, n) - 1 of every replica from its seed (tmp: n*W words
// of scratch) or from a given stream, the loop state from the +1 counts of the
// end state in st.cnt, and the two halves of a full-rollout step.
int sa_draw_s0(int64_t n, int64_t R, const uint32_t* seeds, uint64_t* s, uint64_t* tmp, const mjx_sa_state& st,
               hipStream_t hs);
int sa_draw_s0_mt(int64_t n, int64_t R, const uint32_t* mt_in, const int32_t* idx_in, uint64_t* s,
                  const mjx_sa_state& st, hipStream_t hs);
int sa_init_state(int64_t n, int64_t R, double a0, double b0, const mjx_sa_state& st, hipStream_t hs);
int sa_propose(int64_t n, int64_t R, uint64_t* s, const mjx_sa_state& st, int64_t step, hipStream_t hs);
int sa_accept(int64_t n, int64_t R, uint64_t* s, const mjx_sa_state& st, int64_t step, double par_a, double par_b,
              double a_cap, double b_cap, int64_t t_cap, hipStream_t hs);
bool sa_state_complete(const mjx_sa_state& st);

}  // namespace mjx
