// The greedy quench as independent jobs with the state in LDS (no reference
// counterpart; definitions in include/mjx.h): a job is (start r, restart k)
// with its own visiting order and, for an ELL stack, its own graph.
//
// mjx_quench.hip packs 64 replicas into every word, so all of them share one
// graph and one order.  Here a job holds its single replica node-packed in LDS
// (bit v of a bitmap = spin of node v): the T+1 levels L_t = onestep^t(s), a
// bitmap of marks and T+2 node lists bounded by the ball bound.  The adjacency
// stays in global memory.
//
// A flip of node i is tried in place.  Bit i of L_0 is turned; level t
// recomputes the nodes changed at level t-1 and the nodes of their rows (the
// adjacency is symmetric) from L_{t-1}, which already holds the pending
// changes, and turns the bits of L_t that differ.  L_T is all +1 and the rule
// is monotone, so a change that reaches level T means "refuse": the lists of
// the levels below are walked once more and every turned bit is turned back.
// Otherwise the change died out below T and the levels already hold the
// accepted state.
//
// The wave is the whole workgroup, so its lanes see each other's LDS stores
// after a workgroup barrier.  Bits of one word may belong to several lanes:
// they are turned with LDS atomics, whole words are stored by one lane.
// Everything is integer.
#include "mjx_quench_parts.h"
#include "mjx_philox.h"
#include <algorithm>

namespace mjx {
namespace {

constexpr int QJ_MAXT = 6;
constexpr int64_t kQjLdsMax = 64 * 1024;      // the ceiling of mjx_quench.hip: no dynamic-LDS opt-in
constexpr int QJ_OVERFLOW = 1;                // flag bits of a job
constexpr int QJ_BAD_INDEX = 2;
constexpr int QJ_RESTORE = 4;                 // exchange only: a restoring flip did not commit
constexpr int QJ_ADD = QJ_RESTORE;            // anneal only: an accepted add did not commit; bit 2 on purpose, as
                                              // QJ_RESTORE: "a flip that must commit did not", one kernel raises one
constexpr int QX_MAXT = 3;                    // exchange only: the candidate list is a ball of radius 2T <= 6

struct QjPlan {
    int T;
    int W32;                      // 32-bit words of a bitmap: 2 * ceil(n / 64)
    int cap[QJ_MAXT + 2];         // list l: changed nodes of level l (l <= T), candidates (l = T + 1)
    int off[QJ_MAXT + 2];         // first 32-bit word of list l behind the bitmaps
    int64_t bytes;                // LDS of a job
};

__device__ __forceinline__ bool qj_bit(const uint32_t* L, int v) { return (L[v >> 5] >> (v & 31)) & 1u; }

// sign(2 S + s_v) > 0 on level Lp: rows with multiplicity, degree 0 keeps the spin
// (2 S + s_v is odd).  An entry outside 0..n-1 is skipped; the caller's lists never hold one.
template <class Adj>
__device__ __forceinline__ bool qj_new(const Adj& A, const uint32_t* Lp, int v, int n) {
    const int dg = A.deg(v);
    const int32_t* row = A.row(v);
    int S = 0;
    for (int e = 0; e < dg; ++e) {
        const uint32_t k = (uint32_t)row[e];
        if (k < (uint32_t)n) S += qj_bit(Lp, (int)k) ? 1 : -1;
    }
    return 2 * S + (qj_bit(Lp, v) ? 1 : -1) > 0;
}

// Try the flip of node i (L_0[i] = +1, L_T all +1).  Wave-uniform; returns 1
// when the flip is committed, 0 when it is refused (the levels are as before),
// -QJ_OVERFLOW / -QJ_BAD_INDEX when the job has to stop (the levels are void).
// Counts: a committed flip leaves the sizes of its lists in cnt_out[0 .. QJ_MAXT]
// (list l = the nodes whose level-l value the flip changed; 0 from the level it died out at).
template <class Adj, bool Counts = false>
__device__ int qj_try(const Adj& A, const QjPlan& P, uint32_t* lds, int n, int i, int* cnt_out = nullptr) {
    const int lane = threadIdx.x;
    const u64 below = (1ull << lane) - 1;
    const int T = P.T, W32 = P.W32;
    uint32_t* mark = lds + (T + 1) * W32;
    uint32_t* lists = mark + W32;
    uint32_t* cand = lists + P.off[T + 1];
    int cnt[QJ_MAXT + 1];
#pragma unroll
    for (int l = 0; l <= QJ_MAXT; ++l) cnt[l] = 0;
    if (lane == 0) {
        lists[P.off[0]] = (uint32_t)i;
        lds[i >> 5] ^= 1u << (i & 31);
    }
    cnt[0] = 1;
    __syncthreads();
    int np = 1, applied = 0, err = 0;
    bool refuse = false;
    for (int lv = 1; lv <= T; ++lv) {
        // candidates: the nodes changed at level lv-1 and the nodes of their rows, each once
        // (a mark per node).  A lane per changed node, the lanes walking their rows together.
        const uint32_t* prev = lists + P.off[lv - 1];
        int nu = 0;
        for (int base = 0; base < np && !err; base += 64) {
            const bool have = base + lane < np;
            const int v = have ? (int)prev[base + lane] : 0;
            const int dg = have ? A.deg(v) : -1;
            const int32_t* row = have ? A.row(v) : nullptr;
            const int longest = qn_wave_max(dg);
            for (int e = 0; e <= longest && !err; ++e) {
                bool valid = e <= dg;
                const uint32_t x = valid ? (e == 0 ? (uint32_t)v : (uint32_t)row[e - 1]) : 0u;
                const bool bad = valid && x >= (uint32_t)n;
                valid = valid && !bad;
                bool fresh = false;
                if (valid) {
                    const uint32_t b = 1u << (x & 31);
                    fresh = !(atomicOr(&mark[x >> 5], b) & b);
                }
                const u64 mask = __ballot(fresh);
                const int pos = nu + __popcll(mask & below);
                const int total = nu + __popcll(mask);
                if (__ballot(bad)) err = QJ_BAD_INDEX;
                else if (total > P.cap[T + 1]) err = QJ_OVERFLOW;
                else if (fresh) cand[pos] = x;
                nu = err ? nu : total;
            }
        }
        if (err) break;
        __syncthreads();
        // recompute the candidates on L_{lv-1}; keep those that differ from L_lv
        const uint32_t* Lp = lds + (lv - 1) * W32;
        uint32_t* Ln = lds + lv * W32;
        uint32_t* cur = lists + P.off[lv];
        int nc = 0;
        for (int base = 0; base < nu && !err; base += 64) {
            const int q = base + lane;
            const bool has = q < nu;
            const int j = has ? (int)cand[q] : 0;
            bool ch = false;
            if (has) {
                mark[j >> 5] = 0;                            // every mark belongs to a candidate
                ch = qj_new(A, Lp, j, n) != qj_bit(Ln, j);
            }
            const u64 mask = __ballot(ch);
            const int pos = nc + __popcll(mask & below);
            const int total = nc + __popcll(mask);
            if (total > P.cap[lv]) err = QJ_OVERFLOW;
            else if (ch) cur[pos] = (uint32_t)j;
            nc = err ? nc : total;
        }
        if (err) break;
        __syncthreads();
        if (nc == 0) break;                                  // nothing propagates further: accept
        if (lv == T) {                                       // L_T would lose a +1
            refuse = true;
            break;
        }
        for (int q = lane; q < nc; q += 64) atomicXor(&Ln[cur[q] >> 5], 1u << (cur[q] & 31));
        cnt[lv] = nc;
        applied = lv;
        np = nc;
        __syncthreads();
    }
    if (err) return -err;
    if (!refuse) {
        if constexpr (Counts) {
#pragma unroll
            for (int l = 0; l <= QJ_MAXT; ++l) cnt_out[l] = cnt[l];
        }
        return 1;
    }
#pragma unroll
    for (int l = 0; l < QJ_MAXT; ++l) {                      // level T is never turned
        if (l > applied) break;
        const uint32_t* lst = lists + P.off[l];
        uint32_t* L = lds + l * W32;
        for (int q = lane; q < cnt[l]; q += 64) atomicXor(&L[lst[q] >> 5], 1u << (lst[q] & 31));
    }
    __syncthreads();
    return 0;
}

// valid bits of bitmap word w
__device__ __forceinline__ uint32_t qj_valid(int n, int w) {
    const int left = n - w * 32;
    return left >= 32 ? ~0u : (left <= 0 ? 0u : ((1u << left) - 1u));
}

// Steps 1-4 of a job: the start into L_0, the T sweeps, the consensus test and the
// walk over `ord`.  s_np / r: the starts and the job's row of them.  Returns the job's
// flag (0, QJ_OVERFLOW or QJ_BAD_INDEX).  Load = false: steps 2-4 on the L_0 that is in
// LDS already (padding bits 0, marks clear); s_np and r are not read.
template <class Adj, bool Load = true>
__device__ __forceinline__ int qj_quench_phase(const Adj& A, const QjPlan& P, int n, const uint32_t* __restrict__ s_np,
                                               int64_t r, const int32_t* __restrict__ ord, uint32_t* qj_lds,
                                               bool& cons, long long& nflip) {
    const int lane = threadIdx.x;
    const int T = P.T, W32 = P.W32;
    if constexpr (Load) {
        uint32_t* mark = qj_lds + (T + 1) * W32;
        // 1. the start (padding bits 0 whatever the caller left there), marks cleared
        for (int w = lane; w < W32; w += 64) {
            qj_lds[w] = s_np[r * W32 + w] & qj_valid(n, w);
            mark[w] = 0;
        }
        __syncthreads();
    }
    // 2. L_1 .. L_T: 64 nodes at a time, the wave's ballot is their node-packed word
    for (int t = 1; t <= T; ++t) {
        const uint32_t* Lp = qj_lds + (t - 1) * W32;
        uint32_t* Ln = qj_lds + t * W32;
        for (int base = 0; base < n; base += 64) {
            const int v = base + lane;
            const bool b = v < n && qj_new(A, Lp, v, n);
            const u64 word = __ballot(b);
            if (lane == 0) {
                Ln[base >> 5] = (uint32_t)word;
                Ln[(base >> 5) + 1] = (uint32_t)(word >> 32);
            }
        }
        __syncthreads();
    }
    // 3. consensus: every valid bit of L_T set
    bool all = true;
    for (int w = lane; w < W32; w += 64) all = all && qj_lds[T * W32 + w] == qj_valid(n, w);
    cons = __ballot(!all) == 0;
    // 4. the walk.  Node i is visited once and only its own flip turns bit i of L_0, so the
    //    +1 test of 64 order entries at a time holds when their turn comes.
    nflip = 0;
    int err = 0;
    if (cons && T > 0) {
        for (int base = 0; base < n && !err; base += 64) {
            const int q = base + lane;
            const int oi = q < n ? ord[q] : 0;
            const bool bad = q < n && (uint32_t)oi >= (uint32_t)n;
            if (__ballot(bad)) {
                err = QJ_BAD_INDEX;
                break;
            }
            u64 todo = __ballot(q < n && qj_bit(qj_lds, oi));
            while (todo) {
                const int m = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int i = __builtin_amdgcn_readlane(oi, m);
                const int res = qj_try(A, P, qj_lds, n, i);
                if (res < 0) {
                    err = -res;
                    break;
                }
                nflip += res;
            }
        }
    }
    return err;
}

// Step 5, the result: L_0 to the job's row of out_np; returns its +1 spins.  A stopped
// job (flag != 0) writes words of no meaning, all in bounds.
__device__ __forceinline__ int qj_store(const uint32_t* qj_lds, int W32, uint32_t* __restrict__ out_np, int64_t job) {
    const int lane = threadIdx.x;
    int ones = 0;
    for (int w = lane; w < W32; w += 64) {
        const uint32_t x = qj_lds[w];
        out_np[job * W32 + w] = x;
        ones += __popc(x);
    }
    for (int off = 32; off; off >>= 1) ones += __shfl_xor(ones, off);
    return ones;
}

template <class Adj>
__global__ void __launch_bounds__(64) k_quench_jobs(Adj A0, QjPlan P, int n, int64_t graph_stride, int K,
                                                    const uint32_t* __restrict__ s_np,
                                                    const int32_t* __restrict__ order, int64_t order_stride_r,
                                                    uint32_t* __restrict__ out_np, long long* __restrict__ flipped,
                                                    long long* __restrict__ plus, uint8_t* __restrict__ consensus,
                                                    int32_t* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) uint32_t qj_lds[];
    const int64_t job = blockIdx.x;
    const int64_t r = job / K;
    const int k = (int)(job - r * K);
    const Adj A = A0.at(r * graph_stride);
    const int32_t* ord = order + r * order_stride_r + (int64_t)k * n;
    bool cons;
    long long nflip;
    const int err = qj_quench_phase(A, P, n, s_np, r, ord, qj_lds, cons, nflip);
    const int ones = qj_store(qj_lds, P.W32, out_np, job);
    if (threadIdx.x == 0) {
        flipped[job] = nflip;
        plus[job] = ones;
        flag[job] = err;
        if (k == 0) consensus[r] = cons ? 1 : 0;
    }
}

// ---- the (1, 2) exchange descent behind the quench pass (definitions: include/mjx.h) ----
__device__ __forceinline__ int qx_wave_min(int x) { return -qn_wave_max(-x); }

// One offer round of the candidate search: lanes with `valid` offer node x; an offer
// without a mark gets one and is appended to xl[0 .. qn).  Returns false, with nothing
// appended, when the list would outgrow cap.  No barrier.
__device__ __forceinline__ bool qx_offer(uint32_t* mark, uint32_t* xl, int& qn, int cap, uint32_t x, bool valid) {
    const u64 below = (1ull << threadIdx.x) - 1;
    bool fresh = false;
    if (valid) {
        const uint32_t b = 1u << (x & 31);
        fresh = !(atomicOr(&mark[x >> 5], b) & b);
    }
    const u64 mask = __ballot(fresh);
    const int total = qn + __popcll(mask);
    if (total > cap) return false;
    if (fresh) xl[qn + __popcll(mask & below)] = x;
    qn = total;
    return true;
}

// Add node j (L_0[j] = -1, L_T all +1, L_0 a single-flip local minimum) and drop what
// the add allows.  The candidates are the +1 nodes within t + 2 hops of a node whose
// level-t value the add changed (t < T), tried in ascending rank = position in `ord`
// (xl holds the ranks: ord[rank] is the node).  Wave-uniform; returns 1 when two or more
// nodes dropped (the exchange stays), 0 when the levels are as before, -flag when the
// job has to stop.
template <class Adj>
__device__ int qx_add(const Adj& A, const QjPlan& P, uint32_t* lds, uint32_t* xl, int xcap, int n, int j,
                      const int32_t* __restrict__ ord, const int32_t* rank, long long& ntry) {
    const int lane = threadIdx.x;
    const u64 below = (1ull << lane) - 1;
    const int T = P.T, W32 = P.W32;
    uint32_t* mark = lds + (T + 1) * W32;
    const uint32_t* lists = mark + W32;
    int cnt[QJ_MAXT + 1];
    int res = qj_try<Adj, true>(A, P, lds, n, j, cnt);
    if (res != 1) return res < 0 ? res : -QJ_RESTORE;        // an add changes nothing at level T
    // the search, by remaining hops h = T + 1 .. 1: the frontier xl[fs .. qn) is what the
    // frontier of h + 1 reached plus the changed nodes of level h - 2; a node's first
    // visit is the one with the most hops left, so a mark per node is enough
    int qn = 0, fs = 0, err = 0;
#pragma unroll
    for (int t = QX_MAXT - 1; t >= -1; --t) {
        if (t >= T || err) continue;
        if (t >= 0) {
            const uint32_t* src = lists + P.off[t];
            for (int base = 0; base < cnt[t] && !err; base += 64) {
                const bool have = base + lane < cnt[t];
                if (!qx_offer(mark, xl, qn, xcap, have ? src[base + lane] : 0u, have)) err = QJ_OVERFLOW;
            }
        }
        __syncthreads();
        const int fe = qn;
        for (int base = fs; base < fe && !err; base += 64) {
            const bool have = base + lane < fe;
            const int v = have ? (int)xl[base + lane] : 0;
            const int dg = have ? A.deg(v) : 0;
            const int32_t* row = have ? A.row(v) : nullptr;
            const int longest = qn_wave_max(dg);
            for (int e = 0; e < longest && !err; ++e) {
                const bool in = e < dg;
                const uint32_t x = in ? (uint32_t)row[e] : 0u;
                const bool bad = in && x >= (uint32_t)n;
                if (__ballot(bad)) err = QJ_BAD_INDEX;
                else if (!qx_offer(mark, xl, qn, xcap, x, in)) err = QJ_OVERFLOW;
            }
        }
        fs = fe;
    }
    if (err) return -err;
    __syncthreads();
    // marks cleared; the +1 nodes other than j stay, as ranks
    int nk = 0;
    for (int base = 0; base < qn; base += 64) {
        const bool has = base + lane < qn;
        const int v = has ? (int)xl[base + lane] : 0;
        bool keep = false;
        if (has) {
            mark[v >> 5] = 0;
            keep = v != j && qj_bit(lds, v);
        }
        const int rk = keep ? rank[v] : 0;
        const u64 mask = __ballot(keep);                     // every lane has read its entry here
        if (keep) xl[nk + __popcll(mask & below)] = (uint32_t)rk;
        nk += __popcll(mask);
    }
    __syncthreads();
    int dropped = 0, first = -1, prev = -1;
    for (int it = 0; it < nk && dropped + (nk - it) >= 2; ++it) {      // one drop is no exchange
        int best = INT32_MAX;
        for (int q = lane; q < nk; q += 64) {
            const int rk = (int)xl[q];
            if (rk > prev && rk < best) best = rk;
        }
        best = qx_wave_min(best);
        if (best >= n) return -QJ_BAD_INDEX;                 // ranks of an order that is no permutation
        prev = best;
        const int a = ord[best];
        if ((uint32_t)a >= (uint32_t)n || a == j || !qj_bit(lds, a)) return -QJ_BAD_INDEX;
        res = qj_try(A, P, lds, n, a);
        ++ntry;
        if (res < 0) return res;
        if (res && !dropped) first = a;
        dropped += res;
    }
    if (dropped >= 2) return 1;
    // as before: the single drop back, then j out; both commit by construction
    if (dropped == 1) {
        res = qj_try(A, P, lds, n, first);
        if (res != 1) return res < 0 ? res : -QJ_RESTORE;
    }
    res = qj_try(A, P, lds, n, j);
    if (res != 1) return res < 0 ? res : -QJ_RESTORE;
    return 0;
}

// stats (may be NULL): int64 [jobs][4] = adds, candidate tries, device clock ticks of
// the quench phase and of the exchange phase
template <class Adj>
__global__ void __launch_bounds__(64)
k_quench_exchange_jobs(Adj A0, QjPlan P, int xcap, int xoff, int n, int64_t graph_stride, int K, int max_passes,
                       const uint32_t* __restrict__ s_np, const int32_t* __restrict__ order, int64_t order_stride_r,
                       int32_t* rank_work, uint32_t* __restrict__ out_np, long long* __restrict__ flipped,
                       long long* __restrict__ plus, long long* __restrict__ plus_quench,
                       long long* __restrict__ exchanges, long long* __restrict__ passes,
                       uint8_t* __restrict__ converged, uint8_t* __restrict__ consensus, int32_t* __restrict__ flag,
                       long long* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) uint32_t qj_lds[];
    const int lane = threadIdx.x;
    const int64_t job = blockIdx.x;
    const int64_t r = job / K;
    const int k = (int)(job - r * K);
    const Adj A = A0.at(r * graph_stride);
    const int32_t* ord = order + r * order_stride_r + (int64_t)k * n;
    const long long t0 = (long long)wall_clock64();
    bool cons;
    long long nflip;
    int err = qj_quench_phase(A, P, n, s_np, r, ord, qj_lds, cons, nflip);
    int ones_q = 0;
    for (int w = lane; w < P.W32; w += 64) ones_q += __popc(qj_lds[w]);
    for (int off = 32; off; off >>= 1) ones_q += __shfl_xor(ones_q, off);
    const long long t1 = (long long)wall_clock64();
    // 5. the passes.  A committed exchange turns other nodes to -1, so the -1 test of the
    //    64 order entries is taken again after it; the order was checked by the walk.
    long long nex = 0, nadd = 0, ntry = 0;
    int npass = cons && P.T == 0 ? 1 : 0;                    // T = 0: all +1, a pass without an add
    bool conv = true;
    if (cons && P.T > 0 && !err) {
        conv = false;
        int32_t* rank = rank_work + job * n;
        for (int q = lane; q < n; q += 64) rank[ord[q]] = q;
        __syncthreads();
        uint32_t* xl = qj_lds + xoff;
        for (int ps = 1; ps <= max_passes && !err && !conv; ++ps) {
            bool moved = false;
            for (int base = 0; base < n && !err; base += 64) {
                const int q = base + lane;
                const int oi = q < n ? ord[q] : 0;
                u64 todo = __ballot(q < n && !qj_bit(qj_lds, oi));
                while (todo) {
                    const int m = __ffsll((long long)todo) - 1;
                    const int j = __builtin_amdgcn_readlane(oi, m);
                    const int res = qx_add(A, P, qj_lds, xl, xcap, n, j, ord, rank, ntry);
                    ++nadd;
                    if (res < 0) {
                        err = -res;
                        break;
                    }
                    if (res) {
                        ++nex;
                        moved = true;
                        todo = __ballot(q < n && !qj_bit(qj_lds, oi)) & ~((2ull << m) - 1);
                    } else {
                        todo &= todo - 1;
                    }
                }
            }
            npass = ps;
            conv = !err && !moved;
        }
    }
    const int ones = qj_store(qj_lds, P.W32, out_np, job);
    if (lane == 0) {
        flipped[job] = nflip;
        plus[job] = ones;
        plus_quench[job] = ones_q;
        exchanges[job] = nex;
        passes[job] = npass;
        converged[job] = conv ? 1 : 0;
        flag[job] = err;
        if (k == 0) consensus[r] = cons ? 1 : 0;
        if (stats) {
            stats[job * 4 + 0] = nadd;
            stats[job * 4 + 1] = ntry;
            stats[job * 4 + 2] = t1 - t0;
            stats[job * 4 + 3] = (long long)wall_clock64() - t1;
        }
    }
}

// ---- Metropolis add / drop inside the consensus set (definitions: include/mjx.h) ----
// what the anneal entry points take on top of the quench ones
struct QaArgs {
    int sweeps;
    const uint32_t* thr;           // device uint32 [sweeps]: an add is accepted when its word is below thr[u]
    uint64_t seed;
    int64_t *plus_quench, *plus_best, *best_sweep, *moves;
    int32_t* trace;                // may be NULL
};

// +1 spins of bitmap L, wave-uniform
__device__ __forceinline__ int qa_ones(const uint32_t* L, int W32) {
    int ones = 0;
    for (int w = threadIdx.x; w < W32; w += 64) ones += __popc(L[w]);
    for (int off = 32; off; off >>= 1) ones += __shfl_xor(ones, off);
    return ones;
}

// One wave, one job: the quench pass, `sweeps` sweeps of n proposals each, the lightest
// sweep end kept in a snapshot bitmap behind the job's LDS (word `boff`), and the quench
// pass again from the snapshot.  Proposal q of sweep u is Philox word 0 (the node) and
// word 1 (the add's accept test) of counter (q, u, r, k): lane l draws q = base + l, the
// wave takes the 64 in turn.  A +1 node is one qj_try (a refusal leaves the levels as they
// were); an accepted add is one qj_try, which commits because the rule is monotone.
template <class Adj>
__global__ void __launch_bounds__(64)
k_quench_anneal_jobs(Adj A0, QjPlan P, int boff, int n, int64_t graph_stride, int K, QaArgs X,
                     const uint32_t* __restrict__ s_np, const int32_t* __restrict__ order, int64_t order_stride_r,
                     uint32_t* __restrict__ out_np, long long* __restrict__ flipped, long long* __restrict__ plus,
                     uint8_t* __restrict__ consensus, int32_t* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) uint32_t qj_lds[];
    const int lane = threadIdx.x;
    const int64_t job = blockIdx.x;
    const int64_t r = job / K;
    const int k = (int)(job - r * K);
    const Adj A = A0.at(r * graph_stride);
    const int32_t* ord = order + r * order_stride_r + (int64_t)k * n;
    const int T = P.T, W32 = P.W32, U = X.sweeps;
    uint32_t* snap = qj_lds + boff;
    int32_t* trace = X.trace ? X.trace + job * U : nullptr;
    bool cons;
    long long nflip;
    int err = qj_quench_phase(A, P, n, s_np, r, ord, qj_lds, cons, nflip);
    int ones = qa_ones(qj_lds, W32);                         // the weight, wave-uniform from here on
    const int ones_q = ones;
    int ones_best = ones, best_u = 0;
    long long nadd = 0, ndrop = 0, nref = 0;
    if (!cons || err) {
        // no consensus (or a stopped job): the start stays, the trace is flat
        if (trace)
            for (int u = lane; u < U; u += 64) trace[u] = ones;
    } else {
        for (int w = lane; w < W32; w += 64) snap[w] = qj_lds[w];
        const uint32_t k0 = (uint32_t)X.seed, k1 = (uint32_t)(X.seed >> 32);
        for (int u = 0; u < U && !err; ++u) {
            const uint32_t thr = X.thr[u];
            for (int base = 0; base < n && !err; base += 64) {
                uint32_t x[4];
                philox4x32_10((uint32_t)(base + lane), (uint32_t)u, (uint32_t)r, (uint32_t)k, k0, k1, x);
                const int node = (int)__umulhi(x[0], (uint32_t)n);          // < n
                const u64 yes = __ballot(x[1] < thr);
                const int m_end = min(64, n - base);
                for (int m = 0; m < m_end; ++m) {
                    const int i = __builtin_amdgcn_readlane(node, m);
                    if (qj_bit(qj_lds, i)) {
                        const int res = T == 0 ? 0 : qj_try(A, P, qj_lds, n, i);   // T = 0: all +1, no drop keeps it
                        if (res < 0) {
                            err = -res;
                            break;
                        }
                        ndrop += res;
                        nref += 1 - res;
                        ones -= res;
                    } else if ((yes >> m) & 1) {
                        const int res = qj_try(A, P, qj_lds, n, i);
                        if (res != 1) {                      // an add changes nothing at level T
                            err = res < 0 ? -res : QJ_ADD;
                            break;
                        }
                        ++nadd;
                        ++ones;
                    }
                }
            }
            if (err) break;
            if (trace && lane == 0) trace[u] = ones;
            if (ones < ones_best) {
                for (int w = lane; w < W32; w += 64) snap[w] = qj_lds[w];
                ones_best = ones;
                best_u = u + 1;
            }
        }
        if (!err) {
            // the closing pass: the snapshot back into L_0 (the marks are clear after every try)
            __syncthreads();
            for (int w = lane; w < W32; w += 64) qj_lds[w] = snap[w];
            __syncthreads();
            bool cons2;
            long long nflip2;
            err = qj_quench_phase<Adj, false>(A, P, n, nullptr, 0, ord, qj_lds, cons2, nflip2);
        }
    }
    ones = qj_store(qj_lds, W32, out_np, job);
    if (lane == 0) {
        flipped[job] = nflip;
        plus[job] = ones;
        X.plus_quench[job] = ones_q;
        X.plus_best[job] = ones_best;
        X.best_sweep[job] = best_u;
        X.moves[job * 3 + 0] = nadd;
        X.moves[job * 3 + 1] = ndrop;
        X.moves[job * 3 + 2] = nref;
        flag[job] = err;
        if (k == 0) consensus[r] = cons ? 1 : 0;
    }
}

// bitmaps and list capacities from the caps (HOST int64 [T+1])
int qj_plan(int64_t n, int T, const int64_t* caps, QjPlan& P) {
    if (T < 0 || T > QJ_MAXT || !caps || n < 1 || n > (int64_t)INT32_MAX) return MJX_EINVAL;
    const int64_t W32 = 2 * ((n + 63) / 64);
    int64_t off = 0;
    for (int l = 0; l <= T + 1; ++l) {
        const int64_t cap = (l == 0) ? 1 : std::min<int64_t>(n, caps[l <= T ? l : T]);
        if (cap < 1) return MJX_EINVAL;
        P.cap[l] = (int)cap;
        P.off[l] = (int)std::min<int64_t>(off, INT32_MAX);
        off += cap;
    }
    for (int l = T + 2; l < QJ_MAXT + 2; ++l) P.cap[l] = P.off[l] = 0;
    P.T = T;
    P.bytes = (((T + 2) * W32 + off) * 4 + 15) / 16 * 16;
    if (P.bytes > kQjLdsMax) return MJX_EINVAL;
    P.W32 = (int)W32;
    return MJX_OK;
}

// what the exchange entry points take on top of the quench ones
struct QxArgs {
    int64_t cap2T;
    int max_passes;
    int32_t* rank_work;
    int64_t *plus_quench, *exchanges, *passes;
    uint8_t* converged;
    int64_t* stats;                // may be NULL
};

// the exchange's LDS: the quench job's, then the candidate list of min(n, cap2T) entries
int qx_plan(int64_t n, int T, const int64_t* caps, int64_t cap2T, QjPlan& P, int& xcap, int64_t& bytes) {
    if (T > QX_MAXT || cap2T < 1) return MJX_EINVAL;
    if (int rc = qj_plan(n, T, caps, P)) return rc;
    xcap = (int)std::min<int64_t>(n, cap2T);
    bytes = (P.bytes + 4 * (int64_t)xcap + 15) / 16 * 16;
    return bytes > kQjLdsMax ? MJX_EINVAL : MJX_OK;
}

// the anneal's LDS: the quench job's, then the snapshot bitmap
int qa_plan(int64_t n, int T, const int64_t* caps, QjPlan& P, int64_t& bytes) {
    if (int rc = qj_plan(n, T, caps, P)) return rc;
    bytes = (P.bytes + 4 * (int64_t)P.W32 + 15) / 16 * 16;
    return bytes > kQjLdsMax ? MJX_EINVAL : MJX_OK;
}

template <class Adj>
int quench_jobs_run(Adj A, int64_t n, int64_t graph_stride, int64_t R, int64_t K, int p, int c, const int64_t* caps,
                    const uint64_t* s_np, const int32_t* order, int64_t order_stride_r, uint64_t* out_np,
                    int64_t* flipped, int64_t* plus, uint8_t* consensus, int32_t* flag, void* stream,
                    const QxArgs* X = nullptr, const QaArgs* Y = nullptr) {
    const int T = p + c - 1;
    if (p < 0 || c < 0 || R < 1 || K < 1 || K > (int64_t)INT32_MAX || R * K > (int64_t)INT32_MAX || !s_np || !order ||
        !out_np || !flipped || !plus || !consensus || !flag)
        return MJX_EINVAL;
    if (graph_stride < 0 || (order_stride_r != 0 && order_stride_r != K * n)) return MJX_EINVAL;
    QjPlan P;
    if (X) {
        if (X->max_passes < 1 || !X->rank_work || !X->plus_quench || !X->exchanges || !X->passes || !X->converged)
            return MJX_EINVAL;
        int xcap;
        int64_t bytes;
        if (int rc = qx_plan(n, T, caps, X->cap2T, P, xcap, bytes)) return rc;
        k_quench_exchange_jobs<Adj><<<(unsigned)(R * K), 64, (size_t)bytes, as_stream(stream)>>>(
            A, P, xcap, (int)(P.bytes / 4), (int)n, graph_stride, (int)K, X->max_passes, (const uint32_t*)s_np, order,
            order_stride_r, X->rank_work, (uint32_t*)out_np, (long long*)flipped, (long long*)plus,
            (long long*)X->plus_quench, (long long*)X->exchanges, (long long*)X->passes, X->converged, consensus, flag,
            (long long*)X->stats);
        MJX_LAUNCH_CHECK("k_quench_exchange_jobs");
        return MJX_OK;
    }
    if (Y) {
        if (Y->sweeps < 0 || (Y->sweeps > 0 && !Y->thr) || !Y->plus_quench || !Y->plus_best || !Y->best_sweep ||
            !Y->moves)
            return MJX_EINVAL;
        int64_t bytes;
        if (int rc = qa_plan(n, T, caps, P, bytes)) return rc;
        k_quench_anneal_jobs<Adj><<<(unsigned)(R * K), 64, (size_t)bytes, as_stream(stream)>>>(
            A, P, (int)(P.bytes / 4), (int)n, graph_stride, (int)K, *Y, (const uint32_t*)s_np, order, order_stride_r,
            (uint32_t*)out_np, (long long*)flipped, (long long*)plus, consensus, flag);
        MJX_LAUNCH_CHECK("k_quench_anneal_jobs");
        return MJX_OK;
    }
    if (int rc = qj_plan(n, T, caps, P)) return rc;
    k_quench_jobs<Adj><<<(unsigned)(R * K), 64, (size_t)P.bytes, as_stream(stream)>>>(
        A, P, (int)n, graph_stride, (int)K, (const uint32_t*)s_np, order, order_stride_r, (uint32_t*)out_np,
        (long long*)flipped, (long long*)plus, consensus, flag);
    MJX_LAUNCH_CHECK("k_quench_jobs");
    return MJX_OK;
}

}  // namespace
}  // namespace mjx

using namespace mjx;

extern "C" int64_t mjx_quench_jobs_lds(int64_t n, int T, const int64_t* caps) {
    QjPlan P;
    return qj_plan(n, T, caps, P) ? -1 : P.bytes;
}

extern "C" int mjx_quench_jobs_ell(const int32_t* adj, int64_t n, int d, int64_t graph_stride, int64_t R, int64_t K,
                                   int p, int c, const int64_t* caps, const uint64_t* s_np, const int32_t* order,
                                   int64_t order_stride_r, uint64_t* out_np, int64_t* flipped, int64_t* plus,
                                   uint8_t* consensus, int32_t* flag, void* stream) {
    if (!adj_ell_ok(adj, d) || (graph_stride != 0 && graph_stride != n * d)) return MJX_EINVAL;
    return quench_jobs_run(AdjEll{adj, d}, n, graph_stride, R, K, p, c, caps, s_np, order, order_stride_r, out_np,
                           flipped, plus, consensus, flag, stream);
}

extern "C" int mjx_quench_jobs_csr(const int64_t* row_ptr, const int32_t* col, int64_t n, int64_t R, int64_t K, int p,
                                   int c, const int64_t* caps, const uint64_t* s_np, const int32_t* order,
                                   int64_t order_stride_r, uint64_t* out_np, int64_t* flipped, int64_t* plus,
                                   uint8_t* consensus, int32_t* flag, void* stream) {
    if (!adj_csr_ok(row_ptr)) return MJX_EINVAL;
    return quench_jobs_run(AdjCsr{row_ptr, col}, n, 0, R, K, p, c, caps, s_np, order, order_stride_r, out_np, flipped,
                           plus, consensus, flag, stream);
}

extern "C" int64_t mjx_quench_exchange_jobs_lds(int64_t n, int T, const int64_t* caps, int64_t cap2T) {
    QjPlan P;
    int xcap;
    int64_t bytes;
    return qx_plan(n, T, caps, cap2T, P, xcap, bytes) ? -1 : bytes;
}

extern "C" int mjx_quench_exchange_jobs_ell(const int32_t* adj, int64_t n, int d, int64_t graph_stride, int64_t R,
                                            int64_t K, int p, int c, const int64_t* caps, int64_t cap2T,
                                            int max_passes, const uint64_t* s_np, const int32_t* order,
                                            int64_t order_stride_r, int32_t* rank_work, uint64_t* out_np,
                                            int64_t* flipped, int64_t* plus, int64_t* plus_quench, int64_t* exchanges,
                                            int64_t* passes, uint8_t* converged, uint8_t* consensus, int32_t* flag,
                                            int64_t* stats, void* stream) {
    if (!adj_ell_ok(adj, d) || (graph_stride != 0 && graph_stride != n * d)) return MJX_EINVAL;
    const QxArgs X{cap2T, max_passes, rank_work, plus_quench, exchanges, passes, converged, stats};
    return quench_jobs_run(AdjEll{adj, d}, n, graph_stride, R, K, p, c, caps, s_np, order, order_stride_r, out_np,
                           flipped, plus, consensus, flag, stream, &X);
}

extern "C" int mjx_quench_exchange_jobs_csr(const int64_t* row_ptr, const int32_t* col, int64_t n, int64_t R, int64_t K,
                                            int p, int c, const int64_t* caps, int64_t cap2T, int max_passes,
                                            const uint64_t* s_np, const int32_t* order, int64_t order_stride_r,
                                            int32_t* rank_work, uint64_t* out_np, int64_t* flipped, int64_t* plus,
                                            int64_t* plus_quench, int64_t* exchanges, int64_t* passes,
                                            uint8_t* converged, uint8_t* consensus, int32_t* flag, int64_t* stats,
                                            void* stream) {
    if (!adj_csr_ok(row_ptr)) return MJX_EINVAL;
    const QxArgs X{cap2T, max_passes, rank_work, plus_quench, exchanges, passes, converged, stats};
    return quench_jobs_run(AdjCsr{row_ptr, col}, n, 0, R, K, p, c, caps, s_np, order, order_stride_r, out_np, flipped,
                           plus, consensus, flag, stream, &X);
}

extern "C" int64_t mjx_quench_anneal_jobs_lds(int64_t n, int T, const int64_t* caps) {
    QjPlan P;
    int64_t bytes;
    return qa_plan(n, T, caps, P, bytes) ? -1 : bytes;
}

extern "C" int mjx_quench_anneal_jobs_ell(const int32_t* adj, int64_t n, int d, int64_t graph_stride, int64_t R,
                                          int64_t K, int p, int c, const int64_t* caps, int64_t sweeps,
                                          const uint32_t* thr, uint64_t seed, const uint64_t* s_np,
                                          const int32_t* order, int64_t order_stride_r, uint64_t* out_np,
                                          int64_t* flipped, int64_t* plus, int64_t* plus_quench, int64_t* plus_best,
                                          int64_t* best_sweep, int64_t* moves, int32_t* trace, uint8_t* consensus,
                                          int32_t* flag, void* stream) {
    if (!adj_ell_ok(adj, d) || (graph_stride != 0 && graph_stride != n * d) || sweeps < 0 ||
        sweeps > (int64_t)INT32_MAX)
        return MJX_EINVAL;
    const QaArgs Y{(int)sweeps, thr, seed, plus_quench, plus_best, best_sweep, moves, trace};
    return quench_jobs_run(AdjEll{adj, d}, n, graph_stride, R, K, p, c, caps, s_np, order, order_stride_r, out_np,
                           flipped, plus, consensus, flag, stream, nullptr, &Y);
}

extern "C" int mjx_quench_anneal_jobs_csr(const int64_t* row_ptr, const int32_t* col, int64_t n, int64_t R, int64_t K,
                                          int p, int c, const int64_t* caps, int64_t sweeps, const uint32_t* thr,
                                          uint64_t seed, const uint64_t* s_np, const int32_t* order,
                                          int64_t order_stride_r, uint64_t* out_np, int64_t* flipped, int64_t* plus,
                                          int64_t* plus_quench, int64_t* plus_best, int64_t* best_sweep,
                                          int64_t* moves, int32_t* trace, uint8_t* consensus, int32_t* flag,
                                          void* stream) {
    if (!adj_csr_ok(row_ptr) || sweeps < 0 || sweeps > (int64_t)INT32_MAX) return MJX_EINVAL;
    const QaArgs Y{(int)sweeps, thr, seed, plus_quench, plus_best, best_sweep, moves, trace};
    return quench_jobs_run(AdjCsr{row_ptr, col}, n, 0, R, K, p, c, caps, s_np, order, order_stride_r, out_np, flipped,
                           plus, consensus, flag, stream, nullptr, &Y);
}
