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
#include <algorithm>

namespace mjx {
namespace {

constexpr int QJ_MAXT = 6;
constexpr int64_t kQjLdsMax = 64 * 1024;      // the ceiling of mjx_quench.hip: no dynamic-LDS opt-in
constexpr int QJ_OVERFLOW = 1;                // flag bits of a job
constexpr int QJ_BAD_INDEX = 2;

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
template <class Adj>
__device__ int qj_try(const Adj& A, const QjPlan& P, uint32_t* lds, int n, int i) {
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
    if (!refuse) return 1;
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

template <class Adj>
__global__ void __launch_bounds__(64) k_quench_jobs(Adj A0, QjPlan P, int n, int64_t graph_stride, int K,
                                                    const uint32_t* __restrict__ s_np,
                                                    const int32_t* __restrict__ order, int64_t order_stride_r,
                                                    uint32_t* __restrict__ out_np, long long* __restrict__ flipped,
                                                    long long* __restrict__ plus, uint8_t* __restrict__ consensus,
                                                    int32_t* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) uint32_t qj_lds[];
    const int lane = threadIdx.x;
    const int T = P.T, W32 = P.W32;
    const int64_t job = blockIdx.x;
    const int64_t r = job / K;
    const int k = (int)(job - r * K);
    const Adj A = A0.at(r * graph_stride);
    const int32_t* ord = order + r * order_stride_r + (int64_t)k * n;
    uint32_t* mark = qj_lds + (T + 1) * W32;

    // valid bits of bitmap word w
    auto valid = [&](int w) -> uint32_t {
        const int left = n - w * 32;
        return left >= 32 ? ~0u : (left <= 0 ? 0u : ((1u << left) - 1u));
    };
    // 1. the start (padding bits 0 whatever the caller left there), marks cleared
    for (int w = lane; w < W32; w += 64) {
        qj_lds[w] = s_np[r * W32 + w] & valid(w);
        mark[w] = 0;
    }
    __syncthreads();
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
    for (int w = lane; w < W32; w += 64) all = all && qj_lds[T * W32 + w] == valid(w);
    const bool cons = __ballot(!all) == 0;
    // 4. the walk.  Node i is visited once and only its own flip turns bit i of L_0, so the
    //    +1 test of 64 order entries at a time holds when their turn comes.
    long long nflip = 0;
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
    // 5. the result; a stopped job (flag != 0) writes words of no meaning, all in bounds
    int ones = 0;
    for (int w = lane; w < W32; w += 64) {
        const uint32_t x = qj_lds[w];
        out_np[job * W32 + w] = x;
        ones += __popc(x);
    }
    for (int off = 32; off; off >>= 1) ones += __shfl_xor(ones, off);
    if (lane == 0) {
        flipped[job] = nflip;
        plus[job] = ones;
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

template <class Adj>
int quench_jobs_run(Adj A, int64_t n, int64_t graph_stride, int64_t R, int64_t K, int p, int c, const int64_t* caps,
                    const uint64_t* s_np, const int32_t* order, int64_t order_stride_r, uint64_t* out_np,
                    int64_t* flipped, int64_t* plus, uint8_t* consensus, int32_t* flag, void* stream) {
    const int T = p + c - 1;
    if (p < 0 || c < 0 || R < 1 || K < 1 || K > (int64_t)INT32_MAX || R * K > (int64_t)INT32_MAX || !s_np || !order ||
        !out_np || !flipped || !plus || !consensus || !flag)
        return MJX_EINVAL;
    if (graph_stride < 0 || (order_stride_r != 0 && order_stride_r != K * n)) return MJX_EINVAL;
    QjPlan P;
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
