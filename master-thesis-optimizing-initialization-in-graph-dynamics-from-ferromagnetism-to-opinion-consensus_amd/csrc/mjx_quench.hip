// Flip gains and the greedy quench (no reference counterpart; definitions in
// include/mjx.h): for every node i and replica r the change of F(s) = sum of
// onestep^T(s) when spin i alone is flipped, the mask of +1 spins a consensus
// replica can drop, and the zero-temperature pass that drops them: sequential
// (a workgroup per word column) or in rounds of region-parallel commits.
//
// One evaluator serves all of it.  A wave owns one (node i, word column) pair:
// the 64 replicas of the column are the 64 bits of every word it touches, its
// 64 lanes share the candidates of a level.  With the cached levels L_0 = s,
// L_t = onestep^t(s) the flip is a level-0 difference {i: d0}; level t
// recomputes only the nodes changed at level t-1 and the nodes of their rows
// (the adjacency is symmetric, so row(v) lists every node that reads v) from
// L_{t-1}[k] ^ diff_{t-1}[k] with the bit-sliced majority of mjx_common.h and
// keeps (node, diff word) where the result differs from L_t.  The lists are
// the union over the column's replicas, so they are bounded by the ball bound
// (mjx_sa_csr_ball_bound; min(n, sum_{k<=t} d^k) on a d-regular graph).  Entry
// q of a list lives in LDS for q < E and in the wave's part of the caller's
// scratch area beyond; nothing is truncated.
//
// The wave is the whole workgroup, so the lanes see each other's plain stores
// to LDS, scratch and (quench) the levels after a workgroup barrier: one CU,
// one vector L1.  Everything is integer; no flags needed.
#include "mjx_quench_parts.h"
#include <algorithm>

namespace mjx {

constexpr int QN_MAXT = 6;
constexpr int QN_LDS_DEFAULT = 64;            // list entries kept in LDS (lds_entries = 0)
constexpr size_t kQnLdsMax = 64 * 1024;       // no dynamic-LDS opt-in needed
constexpr int64_t kQnMaxBlocks = 8192;        // flip-gain grid: 32 waves on each of 256 CUs

struct QnCone {
    u64* L[QN_MAXT + 1];          // L[t] = onestep^t(s); word (v, col) at v*W + col
    int E;                        // entries per list in LDS
    int cap[QN_MAXT + 2];         // capacity of list l: changed nodes of level l (l <= T), candidates (l = T+1)
    int64_t soff[QN_MAXT + 2];    // first scratch slot of list l
    int64_t Sd;                   // scratch slots of the T+1 change lists of a workgroup
    int64_t Sc;                   // scratch slots of its candidate list
    int64_t stride;               // bytes of scratch per workgroup (multiple of 8)
    unsigned char* lists;         // scratch behind the header
    u64* header;                  // [0] overflow flag, [1, 1+64W) +1 counts of L_T, [1+64W, 1+65W) consensus words
};

// The lists of one workgroup (= one wave): LDS part and scratch part.
struct QnLists {
    u64* ldiff;                   // LDS [(T+1)][E]
    uint32_t* lnode;              // LDS [(T+1)][E]
    uint32_t* lcand;              // LDS [E]
    u64* sdiff;                   // scratch [Sd]
    uint32_t* snode;              // scratch [Sd]
    uint32_t* scand;              // scratch [Sc]
    int E;
    const int64_t* soff;
    __device__ __forceinline__ uint32_t node(int l, int q) const {
        return q < E ? lnode[l * E + q] : snode[soff[l] + (q - E)];
    }
    __device__ __forceinline__ u64 diff(int l, int q) const {
        return q < E ? ldiff[l * E + q] : sdiff[soff[l] + (q - E)];
    }
    __device__ __forceinline__ void put(int l, int q, uint32_t v, u64 dw) const {
        if (q < E) { lnode[l * E + q] = v; ldiff[l * E + q] = dw; }
        else { snode[soff[l] + (q - E)] = v; sdiff[soff[l] + (q - E)] = dw; }
    }
    __device__ __forceinline__ uint32_t cand(int q) const { return q < E ? lcand[q] : scand[q - E]; }
    __device__ __forceinline__ void put_cand(int q, uint32_t v) const {
        if (q < E) lcand[q] = v;
        else scand[q - E] = v;
    }
};

__device__ __forceinline__ QnLists qn_lists(const QnCone& C, int T, unsigned char* lds, int64_t wg) {
    QnLists S;
    S.E = C.E;
    S.soff = C.soff;
    S.ldiff = (u64*)lds;
    S.lnode = (uint32_t*)(S.ldiff + (size_t)(T + 1) * C.E);
    S.lcand = S.lnode + (size_t)(T + 1) * C.E;
    unsigned char* base = C.lists + wg * C.stride;
    S.sdiff = (u64*)base;
    S.snode = (uint32_t*)(S.sdiff + C.Sd);
    S.scand = S.snode + C.Sd;
    return S;
}

__device__ __forceinline__ u64 qn_lane64(u64 x, int m) {
    return (u64)qn_lane32((uint32_t)x, m) | ((u64)qn_lane32((uint32_t)(x >> 32), m) << 32);
}

// Difference word of node k in change list l (np entries; 0 when it has none),
// for every lane's own k at once: the lanes load 64 entries together and the
// entries are then broadcast from registers, so the scan waits for LDS once per
// 64 entries, not once per entry.  Wave-uniform call; k = kQnNoNode gives 0.
__device__ __forceinline__ u64 qn_patch(const QnLists& S, int l, int np, uint32_t k) {
    const int lane = threadIdx.x;
    u64 x = 0;
    for (int b = 0; b < np; b += 64) {
        const bool in = b + lane < np;
        const uint32_t ln = in ? S.node(l, b + lane) : 0xfffffffeu;
        const u64 ld = in ? S.diff(l, b + lane) : 0;
        const int cc = (np - b) < 64 ? (np - b) : 64;
        for (int m = 0; m < cc; ++m) {
            const uint32_t nq = qn_lane32(ln, m);
            const u64 dq = qn_lane64(ld, m);
            x ^= (k == nq) ? dq : 0;
        }
    }
    return x;
}

// New word at level lv of every lane's candidate j (kQnNoNode: none) from level
// lv-1 with the change list applied.  Wave-uniform call.
template <class Adj>
__device__ __forceinline__ u64 qn_new_word(const Adj& A, const QnLists& S, const u64* Lp, int64_t W, int64_t col,
                                           int lv, int np, uint32_t j) {
    const bool has = j != kQnNoNode;
    auto word = [&](uint32_t k) -> u64 {
        return (k != kQnNoNode ? Lp[(int64_t)k * W + col] : 0) ^ qn_patch(S, lv - 1, np, k);
    };
    const u64 own = word(j);
    if (A.fixed() == 3) {
        u64 x[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) x[e] = word(has ? A.nbr(j, e) : kQnNoNode);
        return majority_fixed<3>(x, own);
    }
    if (A.fixed() == 4) {
        u64 x[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = word(has ? A.nbr(j, e) : kQnNoNode);
        return majority_fixed<4>(x, own);
    }
    const int dg = has ? A.deg(j) : 0;
    const int longest = qn_wave_max(dg);
    BitCounter<8> bc;                            // degree <= 255; degree 0 keeps the word
    bc.reset();
    for (int e = 0; e < longest; ++e) bc.add(word(e < dg ? A.nbr(j, e) : kQnNoNode));   // a lane past its row adds 0
    return bc.majority(dg, own);
}

// Light cone of the level-0 difference {i: d0} in word column col.  On return
// cnt[l] entries of list l (l = 0..T) hold the changed nodes of level l and
// their difference words.  Wave-uniform control flow; all 64 lanes take part.
// Returns false when a list outgrew its cap (caps not of this graph): nothing
// is written out of bounds, the lists are then incomplete.
template <class Adj>
__device__ bool qn_cone(const Adj& A, const QnCone& C, const QnLists& S, int T, int64_t W, int64_t col, uint32_t i,
                        u64 d0, int* cnt) {
    const int lane = threadIdx.x;
    const u64 below = (1ull << lane) - 1;
    for (int l = 0; l <= T; ++l) cnt[l] = 0;
    if (d0 == 0) return true;
    if (lane == 0) S.put(0, 0, i, d0);
    cnt[0] = 1;
    __syncthreads();
    bool ok = true;
    for (int lv = 1; lv <= T && ok; ++lv) {
        const int np = cnt[lv - 1];
        if (np == 0) break;                                  // nothing propagates further
        // candidates: the nodes changed at level lv-1 and the nodes of their rows, each once.
        // A lane per changed node, the lanes walking their rows together: round e offers
        // the node itself (e = 0) or entry e-1 of every lane's row, so a level costs
        // (longest row + 1) rounds per 64 changed nodes, the rows' loads in flight together.
        int nu = 0;
        for (int base = 0; base < np && ok; base += 64) {
            const bool have = base + lane < np;
            const uint32_t v = have ? S.node(lv - 1, base + lane) : 0u;
            const int dg = have ? A.deg(v) : -1;
            const int longest = qn_wave_max(dg);
            const int lanes = (np - base) < 64 ? (np - base) : 64;
            for (int e = 0; e <= longest && ok; ++e) {
                const bool valid = e <= dg;
                const uint32_t x = valid ? (e == 0 ? v : A.nbr(v, e - 1)) : kQnNoNode;
                ok = qn_offer(x, valid, lanes, nu, C.cap[T + 1], [&](int q) { return S.cand(q); },
                              [&](int q, uint32_t y) { S.put_cand(q, y); });
            }
        }
        // recompute the candidates; keep those whose word differs from the cached level
        int nc = 0;
        const u64* Lp = C.L[lv - 1];
        const u64* Ln = C.L[lv];
        for (int base = 0; base < nu && ok; base += 64) {
            const int q = base + lane;
            const uint32_t j = q < nu ? S.cand(q) : kQnNoNode;
            const u64 nw = qn_new_word(A, S, Lp, W, col, lv, np, j);
            const u64 dw = q < nu ? nw ^ Ln[(int64_t)j * W + col] : 0;
            const u64 mask = __ballot(dw != 0);
            const int pos = nc + __popcll(mask & below);
            const int total = nc + __popcll(mask);
            if (total > C.cap[lv]) ok = false;
            else if (dw != 0) S.put(lv, pos, j, dw);
            nc = ok ? total : nc;
        }
        cnt[lv] = nc;
        __syncthreads();
    }
    return ok;
}

__device__ __forceinline__ u64 qn_valid(int64_t col, int64_t W, int64_t R) {
    const int tail = (int)(R & 63);
    return (col == W - 1 && tail) ? ((1ull << tail) - 1) : ~0ull;
}

// Try the flip {i: d0} in word column col and commit it in the replicas where
// consensus survives it: the cone, the OR of the level-T differences, acc =
// d0 & ~OR, the differences masked by acc XORed into every level, a barrier
// (the commits land, and the lists are free, before the next try).  Returns
// false on overflow: the header's flag is set, nothing is committed and acc
// is 0.  cnt is the caller's [QN_MAXT + 1], declared once outside its loop
// (declared here it costs 7 VGPRs and three of the four kernels an occupancy step).
template <class Adj>
__device__ __forceinline__ bool qn_try_commit(const Adj& A, const QnCone& C, const QnLists& S, int T, int64_t W,
                                              int64_t col, uint32_t i, u64 d0, int* cnt, u64& acc) {
    const int lane = threadIdx.x;
    const bool ok = qn_cone(A, C, S, T, W, col, i, d0, cnt);
    acc = 0;
    if (!ok) {
        if (lane == 0) C.header[0] = 1;
    } else {
        u64 orT = 0;
        for (int q = lane; q < cnt[T]; q += 64) orT |= S.diff(T, q);
        acc = d0 & ~qn_wave_or(orT);
        if (acc)
            for (int l = 0; l <= T; ++l)
                for (int q = lane; q < cnt[l]; q += 64) {    // the nodes of a list are distinct: one lane per word
                    const u64 dq = S.diff(l, q) & acc;
                    if (dq) C.L[l][(int64_t)S.node(l, q) * W + col] ^= dq;
                }
    }
    __syncthreads();
    return ok;
}

// consensus[r] = (+1 count of L_T == n), and the same as a word per column
__global__ void __launch_bounds__(64) k_qn_consensus(const u64* __restrict__ counts, int64_t n, int64_t R,
                                                     u64* __restrict__ words, uint8_t* __restrict__ consensus) {
    const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool c = r < R && counts[r] == (u64)n;
    if (r < R) consensus[r] = c ? 1 : 0;
    const u64 m = __ballot(c);
    if (threadIdx.x == 0) words[blockIdx.x] = m;
}

template <class Adj>
__global__ void __launch_bounds__(64) k_flip_gain(Adj A, QnCone C, int T, int64_t n, int64_t W, int64_t R,
                                                  u64* __restrict__ removable, int32_t* __restrict__ gain) {
    extern __shared__ __align__(8) unsigned char qn_lds[];
    const QnLists S = qn_lists(C, T, qn_lds, blockIdx.x);
    const int lane = threadIdx.x;
    const u64* cons = C.header + 1 + 64 * W;
    const int64_t pairs = n * W;
    int cnt[QN_MAXT + 1];
    for (int64_t pid = blockIdx.x; pid < pairs; pid += gridDim.x) {
        const int64_t i = pid / W, col = pid - i * W;
        const u64 valid = qn_valid(col, W, R);
        const bool ok = qn_cone(A, C, S, T, W, col, (uint32_t)i, valid, cnt);
        if (!ok) {
            if (lane == 0) C.header[0] = 1;
            break;
        }
        // the level-T entries, 64 at a time in registers: their OR, and per lane (= replica)
        // +-2 for every entry that holds its bit
        u64 orT = 0;
        int g = 0;
        for (int b = 0; b < cnt[T]; b += 64) {
            const bool in = b + lane < cnt[T];
            const u64 mine = in ? S.diff(T, b + lane) : 0;
            const u64 was = (gain && in) ? C.L[T][(int64_t)S.node(T, b + lane) * W + col] : 0;
            const int cc = (cnt[T] - b) < 64 ? (cnt[T] - b) : 64;
            for (int m = 0; m < cc; ++m) {
                const u64 dq = qn_lane64(mine, m), old = qn_lane64(was, m);
                orT |= dq;
                if ((dq >> lane) & 1) g += ((old >> lane) & 1) ? -2 : 2;
            }
        }
        if (lane == 0) removable[pid] = C.L[0][pid] & cons[col] & ~orT & valid;
        if (gain) gain[(i * W + col) * 64 + lane] = g;
        __syncthreads();                                     // the lists are reused by the next pair
    }
}

template <class Adj>
__global__ void __launch_bounds__(64) k_quench(Adj A, QnCone C, int T, int64_t n, int64_t W, int64_t R,
                                               const int32_t* __restrict__ cand, const int64_t* __restrict__ cand_ptr,
                                               long long* __restrict__ flipped) {
    extern __shared__ __align__(8) unsigned char qn_lds[];
    const QnLists S = qn_lists(C, T, qn_lds, blockIdx.x);
    const int lane = threadIdx.x;
    const int64_t col = blockIdx.x;
    const u64 valid = qn_valid(col, W, R);
    const u64 cons = C.header[1 + 64 * W + col] & valid;
    int cnt[QN_MAXT + 1];
    long long mine = 0;
    const int64_t c1 = cand_ptr[col + 1];
    for (int64_t c = cand_ptr[col]; c < c1; ++c) {
        const uint32_t i = (uint32_t)cand[c];
        // the flip is tried in the replicas where it can count: s_i = +1 and consensus
        const u64 d0 = C.L[0][(int64_t)i * W + col] & cons;
        if (d0 == 0) continue;
        u64 acc;
        if (!qn_try_commit(A, C, S, T, W, col, i, d0, cnt, acc)) break;
        mine += (long long)((acc >> lane) & 1);
    }
    flipped[col * 64 + lane] = mine;
}

// ---- the region-parallel pass ---------------------------------------------
// The candidates of ALL word columns (the union, in `order` order; candidate
// k has rank k) are committed in rounds.  Trying candidate i writes level l
// within distance l of i (l <= T-1; an accepted replica has no level-T diff)
// and reads it within distance l+2, so two candidates further apart than 2T
// have disjoint read and write sets and commute: both may run in the same
// round, on different workgroups.  dist(i, j) <= 2T exactly when the radius-T
// balls of i and j meet.  A window of K slots holds the K pending candidates of
// lowest rank.  Per round (three launches; stream order is the only
// synchronisation between workgroups):
//   reserve  every slot writes its key into claim[v] for every node v of its
//            ball with an atomic max.  key = (round + 1) << 32 | ~rank: within
//            a round the lowest rank wins, and a key of an earlier round never
//            survives a later one, so nothing is reset;
//   check    a slot that reads its own key back on its whole ball has no
//            pending candidate of lower rank within 2T: its node goes to the
//            ready list and the slot takes the next candidate (an atomic
//            cursor into the order) and walks its ball, once per candidate;
//   commit   a wave per (ready node, word column) runs qn_try_commit, as k_quench does.
// The pending candidate of lowest rank always wins its ball, so a round with
// anything pending commits at least one candidate.
struct QrState {
    unsigned long long* stats;    // caller's [4]: candidates left, rounds that committed, most commits of a
                                  // round, cursor (the next rank to hand out; it runs on past the end)
    unsigned long long* claim;    // [n] keys
    int32_t* nready;              // [1] entries of `ready`
    int32_t* rank;                // [K] rank of the slot's candidate, -1: empty
    int32_t* bcnt;                // [K] nodes of its ball
    int32_t* ready;               // [K] the nodes that commit in this round
    int32_t* ball;                // [K][capB] the balls, each node once
    int capB;                     // caps[T]
    int K;
};

__device__ __forceinline__ unsigned long long qr_key(long long round, int32_t rank) {
    return ((unsigned long long)(round + 1) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)rank);
}

// The nodes within distance T of i, each once, into ball[0 .. cap): the cone's
// candidate walk (a lane per frontier node, the lanes walking their rows
// together) on one plain list that grows level by level.  Returns the count;
// ok = false when the ball outgrew cap or a row names a node >= n (nothing is
// written out of bounds, the ball is then incomplete).  Wave-uniform.
template <class Adj>
__device__ int qr_ball(const Adj& A, int T, int64_t n, uint32_t i, int32_t* ball, int cap, bool& ok) {
    const int lane = threadIdx.x;
    if (lane == 0) ball[0] = (int32_t)i;
    __syncthreads();
    int nu = 1, f0 = 0;
    for (int lv = 1; lv <= T && ok; ++lv) {
        const int f1 = nu;
        for (int base = f0; base < f1 && ok; base += 64) {
            const bool have = base + lane < f1;
            const uint32_t v = have ? (uint32_t)ball[base + lane] : 0u;
            const int dg = have ? A.deg(v) : 0;
            const int longest = qn_wave_max(dg);
            const int lanes = (f1 - base) < 64 ? (f1 - base) : 64;
            for (int e = 0; e < longest && ok; ++e) {
                const bool valid = e < dg;
                const uint32_t x = valid ? A.nbr(v, e) : kQnNoNode;
                ok = !__ballot(valid && x >= (uint32_t)n) &&
                     qn_offer(x, valid, lanes, nu, cap, [&](int q) { return (uint32_t)ball[q]; },
                              [&](int q, uint32_t y) { ball[q] = (int32_t)y; });
            }
        }
        f0 = f1;
    }
    return nu;
}

__global__ void __launch_bounds__(64) k_qr_init(QrState Q, int64_t ncand) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t < Q.K) Q.rank[t] = -1;
    if (t == 0) {
        Q.stats[0] = (unsigned long long)ncand;
        Q.stats[1] = Q.stats[2] = Q.stats[3] = 0;
        *Q.nready = 0;
    }
}

__global__ void __launch_bounds__(64) k_qr_reserve(QrState Q, long long round) {
    const int slot = blockIdx.x, lane = threadIdx.x;
    if (slot == 0 && lane == 0) *Q.nready = 0;              // the ready list of the round before is spent
    const int32_t rk = Q.rank[slot];
    if (rk < 0) return;
    const unsigned long long key = qr_key(round, rk);
    const int32_t* ball = Q.ball + (int64_t)slot * Q.capB;
    const int cnt = Q.bcnt[slot];
    for (int q = lane; q < cnt; q += 64) atomicMax(&Q.claim[ball[q]], key);
}

// round < 0: the first fill, nothing to check
template <class Adj>
__global__ void __launch_bounds__(64) k_qr_check(Adj A, QrState Q, int T, int64_t n, const int32_t* __restrict__ cand,
                                                 int64_t ncand, long long round, u64* __restrict__ flag) {
    const int slot = blockIdx.x, lane = threadIdx.x;
    int32_t* ball = Q.ball + (int64_t)slot * Q.capB;
    const int32_t rk = Q.rank[slot];
    if (rk >= 0) {
        const unsigned long long key = qr_key(round, rk);
        const int cnt = Q.bcnt[slot];
        bool lost = false;
        for (int q = lane; q < cnt; q += 64) lost |= Q.claim[ball[q]] != key;
        if (__ballot(lost)) return;                          // a pending candidate of lower rank within 2T: wait
        if (lane == 0) Q.ready[atomicAdd(Q.nready, 1)] = cand[rk];
    }
    // the slot is free: the next candidate of the order and its ball
    unsigned long long nx = 0;
    if (lane == 0) nx = atomicAdd(&Q.stats[3], 1ull);
    nx = qn_lane64(nx, 0);
    if (nx >= (unsigned long long)ncand) {
        if (lane == 0) Q.rank[slot] = -1;
        return;
    }
    bool ok = true;
    const int cnt = qr_ball(A, T, n, (uint32_t)cand[nx], ball, Q.capB, ok);
    if (lane == 0) {
        Q.rank[slot] = (int32_t)nx;
        Q.bcnt[slot] = cnt;
        if (!ok) *flag = 1;
    }
}

// The try-and-commit of k_quench for every (ready node, word column) pair.  The
// ready nodes are further apart than 2T, so no pair reads a word another writes.
template <class Adj>
__global__ void __launch_bounds__(64) k_qr_commit(Adj A, QnCone C, QrState Q, int T, int64_t n, int64_t W, int64_t R,
                                                  const u64* __restrict__ removable,
                                                  unsigned long long* __restrict__ flipped) {
    extern __shared__ __align__(8) unsigned char qn_lds[];
    const QnLists S = qn_lists(C, T, qn_lds, blockIdx.x);
    const int lane = threadIdx.x;
    const int nr = *Q.nready;
    if (blockIdx.x == 0 && lane == 0 && nr > 0) {
        Q.stats[0] -= (unsigned long long)nr;
        Q.stats[1] += 1;
        if ((unsigned long long)nr > Q.stats[2]) Q.stats[2] = (unsigned long long)nr;
    }
    int cnt[QN_MAXT + 1];
    const int64_t pairs = (int64_t)nr * W;
    for (int64_t pid = blockIdx.x; pid < pairs; pid += gridDim.x) {
        const int64_t q = pid / W, col = pid - q * W;
        const uint32_t i = (uint32_t)Q.ready[q];
        if (removable[(int64_t)i * W + col] == 0) continue;  // no candidate of this column: the pass skips it
        const u64 cons = C.header[1 + 64 * W + col] & qn_valid(col, W, R);
        const u64 d0 = C.L[0][(int64_t)i * W + col] & cons;
        if (d0 == 0) continue;
        u64 acc;                                             // an overflow is flagged; the other pairs go on
        qn_try_commit(A, C, S, T, W, col, i, d0, cnt, acc);
        if ((acc >> lane) & 1) atomicAdd(&flipped[col * 64 + lane], 1ull);
    }
}

// list capacities, LDS part and scratch slots from the caps (HOST int64 [T+1])
static int qn_plan(int T, const int64_t* caps, int lds_entries, QnCone& C) {
    if (T < 0 || T > QN_MAXT || !caps || lds_entries < 0) return MJX_EINVAL;
    C.E = lds_entries ? lds_entries : QN_LDS_DEFAULT;
    if ((size_t)C.E * ((size_t)(T + 1) * 12 + 4) > kQnLdsMax) return MJX_EINVAL;
    int64_t S = 0;
    for (int l = 0; l <= T + 1; ++l) {
        const int64_t cap = (l == 0) ? 1 : caps[l <= T ? l : T];
        if (cap < 1 || cap > (int64_t)INT32_MAX) return MJX_EINVAL;
        C.cap[l] = (int)cap;
        C.soff[l] = (l <= T) ? S : 0;
        if (l <= T) S += std::max<int64_t>(0, cap - C.E);
    }
    for (int l = T + 2; l < QN_MAXT + 2; ++l) { C.cap[l] = 0; C.soff[l] = 0; }
    C.Sd = S;
    C.Sc = std::max<int64_t>(0, (int64_t)C.cap[T + 1] - C.E);
    C.stride = ((C.Sd * 12 + C.Sc * 4 + 7) / 8) * 8;
    return MJX_OK;
}

static size_t qn_lds_bytes(int T, int E) { return (size_t)E * ((size_t)(T + 1) * 12 + 4); }

static int64_t qn_header_bytes(int64_t W) { return (1 + 65 * W) * (int64_t)sizeof(u64); }

static int64_t qn_flip_blocks(int64_t n, int64_t W) { return std::min<int64_t>(n * W, kQnMaxBlocks); }

// arguments common to the four entry points; fills C but for the adjacency
static int qn_setup(int64_t n, int64_t R, int p, int c, uint64_t* const* levels, const int64_t* caps, int lds_entries,
                    void* scratch, int64_t scratch_bytes, int64_t blocks, QnCone& C) {
    const int T = p + c - 1;
    if (p < 0 || c < 0 || T < 0 || T > QN_MAXT || n < 1 || n > (int64_t)INT32_MAX || R < 1 || !levels || !caps ||
        !scratch)
        return MJX_EINVAL;
    if (int rc = qn_plan(T, caps, lds_entries, C)) return rc;
    const int64_t W = (R + 63) / 64;
    if (scratch_bytes < qn_header_bytes(W) + blocks * C.stride) return MJX_EINVAL;
    for (int t = 0; t <= QN_MAXT; ++t) C.L[t] = nullptr;
    for (int t = 0; t <= T; ++t) {
        if (!levels[t]) return MJX_EINVAL;
        C.L[t] = (u64*)levels[t];
    }
    C.header = (u64*)scratch;
    C.lists = (unsigned char*)scratch + qn_header_bytes(W);
    return MJX_OK;
}

// header: overflow flag and +1 counts zeroed, counts of L_T, consensus bytes and words
static int qn_consensus(const QnCone& C, int T, int64_t n, int64_t R, uint8_t* consensus, void* stream) {
    const int64_t W = (R + 63) / 64;
    hipStream_t hs = as_stream(stream);
    MJX_HIP(hipMemsetAsync(C.header, 0, (size_t)(1 + 64 * W) * sizeof(u64), hs), "quench header memset");
    if (int rc = mjx_popcount_rp((const uint64_t*)C.L[T], n, W, (unsigned long long*)(C.header + 1), stream)) return rc;
    k_qn_consensus<<<(unsigned)W, 64, 0, hs>>>(C.header + 1, n, R, C.header + 1 + 64 * W, consensus);
    MJX_LAUNCH_CHECK("k_qn_consensus");
    return MJX_OK;
}

template <class Adj>
static int flip_gain_run(Adj A, int64_t n, int64_t R, int p, int c, const uint64_t* const* levels,
                         const int64_t* caps, int lds_entries, void* scratch, int64_t scratch_bytes,
                         uint64_t* removable, uint8_t* consensus, int32_t* gain, void* stream) {
    if (!removable || !consensus) return MJX_EINVAL;
    const int64_t W = (R + 63) / 64;
    if (R < 1 || n < 1 || W > (int64_t)INT32_MAX) return MJX_EINVAL;
    const int64_t blocks = qn_flip_blocks(n, W);
    QnCone C;
    if (int rc = qn_setup(n, R, p, c, (uint64_t* const*)levels, caps, lds_entries, scratch, scratch_bytes, blocks, C))
        return rc;
    const int T = p + c - 1;
    if (int rc = qn_consensus(C, T, n, R, consensus, stream)) return rc;
    k_flip_gain<Adj><<<(unsigned)blocks, 64, qn_lds_bytes(T, C.E), as_stream(stream)>>>(A, C, T, n, W, R,
                                                                                      (u64*)removable, gain);
    MJX_LAUNCH_CHECK("k_flip_gain");
    return MJX_OK;
}

template <class Adj>
static int quench_run(Adj A, int64_t n, int64_t R, int p, int c, uint64_t* const* levels, const int64_t* caps,
                      int lds_entries, void* scratch, int64_t scratch_bytes, const int32_t* cand,
                      const int64_t* cand_ptr, uint8_t* consensus, int64_t* flipped, void* stream) {
    if (!cand_ptr || !consensus || !flipped) return MJX_EINVAL;
    const int64_t W = (R + 63) / 64;
    if (R < 1 || n < 1 || W > (int64_t)INT32_MAX) return MJX_EINVAL;
    QnCone C;
    if (int rc = qn_setup(n, R, p, c, levels, caps, lds_entries, scratch, scratch_bytes, W, C)) return rc;
    const int T = p + c - 1;
    if (int rc = qn_consensus(C, T, n, R, consensus, stream)) return rc;
    k_quench<Adj><<<(unsigned)W, 64, qn_lds_bytes(T, C.E), as_stream(stream)>>>(A, C, T, n, W, R, cand, cand_ptr,
                                                                              (long long*)flipped);
    MJX_LAUNCH_CHECK("k_quench");
    return MJX_OK;
}

// region-parallel pass: workgroups of the commit kernel, and the scratch behind
// the header: their lists, then claim[n], nready (8 bytes), rank, bcnt, ready
// [K] and ball[K][caps[T]]
static int64_t qr_commit_blocks(int64_t K, int64_t W) { return std::min<int64_t>(K * W, kQnMaxBlocks); }

static int64_t qr_state_bytes(int64_t n, int64_t K, int64_t capB) {
    return 8 * n + 8 + ((4 * K * (3 + capB) + 7) / 8) * 8;
}

static bool qr_shape_ok(int64_t n, int64_t R, int64_t window) {
    return n >= 1 && n <= (int64_t)INT32_MAX && R >= 1 && (R + 63) / 64 <= (int64_t)INT32_MAX && window >= 1 &&
           window <= (int64_t)INT32_MAX;
}

template <class Adj>
static int quench_regions_run(Adj A, int64_t n, int64_t R, int p, int c, uint64_t* const* levels, const int64_t* caps,
                              int lds_entries, void* scratch, int64_t scratch_bytes, int64_t window,
                              const uint64_t* removable, const int32_t* cand, int64_t ncand, uint8_t* consensus,
                              int64_t* flipped, int64_t* stats, int64_t round0, int64_t rounds, void* stream) {
    if (!removable || !consensus || !flipped || !stats || !qr_shape_ok(n, R, window) || ncand < 0 || ncand > n ||
        (ncand > 0 && !cand) || round0 < 0 || rounds < 0 || round0 + rounds > (int64_t)INT32_MAX)
        return MJX_EINVAL;
    const int64_t W = (R + 63) / 64, K = window;
    const int64_t blocks = qr_commit_blocks(K, W);
    QnCone C;
    if (int rc = qn_setup(n, R, p, c, levels, caps, lds_entries, scratch, scratch_bytes, blocks, C)) return rc;
    const int T = p + c - 1;
    const int64_t capB = C.cap[T + 1];                       // caps[T]
    if (scratch_bytes < qn_header_bytes(W) + blocks * C.stride + qr_state_bytes(n, K, capB)) return MJX_EINVAL;
    QrState Q;
    unsigned char* at = C.lists + blocks * C.stride;
    Q.stats = (unsigned long long*)stats;
    Q.claim = (unsigned long long*)at;
    Q.nready = (int32_t*)(at + 8 * n);
    Q.rank = (int32_t*)(at + 8 * n + 8);
    Q.bcnt = Q.rank + K;
    Q.ready = Q.bcnt + K;
    Q.ball = Q.ready + K;
    Q.capB = (int)capB;
    Q.K = (int)K;
    hipStream_t hs = as_stream(stream);
    if (round0 == 0) {
        if (int rc = qn_consensus(C, T, n, R, consensus, stream)) return rc;
        MJX_HIP(hipMemsetAsync(flipped, 0, (size_t)(64 * W) * sizeof(int64_t), hs), "quench regions flipped memset");
        MJX_HIP(hipMemsetAsync(Q.claim, 0, (size_t)n * 8, hs), "quench regions claim memset");
        k_qr_init<<<(unsigned)((K + 63) / 64), 64, 0, hs>>>(Q, ncand);
        MJX_LAUNCH_CHECK("k_qr_init");
        if (ncand > 0) {
            k_qr_check<Adj><<<(unsigned)K, 64, 0, hs>>>(A, Q, T, n, cand, ncand, -1, C.header);
            MJX_LAUNCH_CHECK("k_qr_check (fill)");
        }
    }
    if (ncand == 0) return MJX_OK;
    for (int64_t r = round0; r < round0 + rounds; ++r) {
        k_qr_reserve<<<(unsigned)K, 64, 0, hs>>>(Q, (long long)r);
        MJX_LAUNCH_CHECK("k_qr_reserve");
        k_qr_check<Adj><<<(unsigned)K, 64, 0, hs>>>(A, Q, T, n, cand, ncand, (long long)r, C.header);
        MJX_LAUNCH_CHECK("k_qr_check");
        k_qr_commit<Adj><<<(unsigned)blocks, 64, qn_lds_bytes(T, C.E), hs>>>(A, C, Q, T, n, W, R, (const u64*)removable,
                                                                            (unsigned long long*)flipped);
        MJX_LAUNCH_CHECK("k_qr_commit");
    }
    return MJX_OK;
}

}  // namespace mjx

using namespace mjx;

extern "C" int mjx_ell_ball_bound(int64_t n, int d, int T, int64_t* bound_out) {
    if (!bound_out || n < 1 || d < 0 || T < 0 || T > QN_MAXT) return MJX_EINVAL;
    int64_t pw = 1, acc = 1;
    for (int t = 0; t <= T; ++t) {
        bound_out[t] = std::min<int64_t>(n, acc);
        pw = (pw > n) ? pw : pw * d;                        // saturating: acc is cut at n anyway
        acc = std::min<int64_t>(n, acc + pw);
    }
    return MJX_OK;
}

extern "C" int64_t mjx_quench_lds(int T, int lds_entries) {
    if (T < 0 || T > QN_MAXT || lds_entries < 0) return -1;
    const size_t b = qn_lds_bytes(T, lds_entries ? lds_entries : QN_LDS_DEFAULT);
    return b > kQnLdsMax ? -1 : (int64_t)b;
}

extern "C" int64_t mjx_flip_gain_scratch_bytes(int64_t n, int64_t R, int T, const int64_t* caps, int lds_entries) {
    QnCone C;
    if (n < 1 || R < 1 || qn_plan(T, caps, lds_entries, C)) return -1;
    const int64_t W = (R + 63) / 64;
    return qn_header_bytes(W) + qn_flip_blocks(n, W) * C.stride;
}

extern "C" int64_t mjx_quench_scratch_bytes(int64_t R, int T, const int64_t* caps, int lds_entries) {
    QnCone C;
    if (R < 1 || qn_plan(T, caps, lds_entries, C)) return -1;
    const int64_t W = (R + 63) / 64;
    return qn_header_bytes(W) + W * C.stride;
}

extern "C" int mjx_flip_gain_ell_rp(const int32_t* adj, int64_t n, int d, int64_t R, int p, int c,
                                    const uint64_t* const* levels, const int64_t* caps, int lds_entries,
                                    void* scratch, int64_t scratch_bytes, uint64_t* removable, uint8_t* consensus,
                                    int32_t* gain, void* stream) {
    if (!adj_ell_ok(adj, d)) return MJX_EINVAL;
    return flip_gain_run(AdjEll{adj, d}, n, R, p, c, levels, caps, lds_entries, scratch, scratch_bytes, removable,
                         consensus, gain, stream);
}

extern "C" int mjx_flip_gain_csr_rp(const int64_t* row_ptr, const int32_t* col, int64_t n, int64_t R, int p, int c,
                                    const uint64_t* const* levels, const int64_t* caps, int lds_entries,
                                    void* scratch, int64_t scratch_bytes, uint64_t* removable, uint8_t* consensus,
                                    int32_t* gain, void* stream) {
    if (!adj_csr_ok(row_ptr)) return MJX_EINVAL;
    return flip_gain_run(AdjCsr{row_ptr, col}, n, R, p, c, levels, caps, lds_entries, scratch, scratch_bytes,
                         removable, consensus, gain, stream);
}

extern "C" int mjx_quench_ell_rp(const int32_t* adj, int64_t n, int d, int64_t R, int p, int c,
                                 uint64_t* const* levels, const int64_t* caps, int lds_entries, void* scratch,
                                 int64_t scratch_bytes, const int32_t* cand, const int64_t* cand_ptr,
                                 uint8_t* consensus, int64_t* flipped, void* stream) {
    if (!adj_ell_ok(adj, d)) return MJX_EINVAL;
    return quench_run(AdjEll{adj, d}, n, R, p, c, levels, caps, lds_entries, scratch, scratch_bytes, cand, cand_ptr,
                      consensus, flipped, stream);
}

extern "C" int mjx_quench_csr_rp(const int64_t* row_ptr, const int32_t* col, int64_t n, int64_t R, int p, int c,
                                 uint64_t* const* levels, const int64_t* caps, int lds_entries, void* scratch,
                                 int64_t scratch_bytes, const int32_t* cand, const int64_t* cand_ptr,
                                 uint8_t* consensus, int64_t* flipped, void* stream) {
    if (!adj_csr_ok(row_ptr)) return MJX_EINVAL;
    return quench_run(AdjCsr{row_ptr, col}, n, R, p, c, levels, caps, lds_entries, scratch, scratch_bytes, cand,
                      cand_ptr, consensus, flipped, stream);
}

extern "C" int64_t mjx_quench_regions_scratch_bytes(int64_t n, int64_t R, int T, const int64_t* caps, int lds_entries,
                                                    int64_t window) {
    QnCone C;
    if (!qr_shape_ok(n, R, window) || qn_plan(T, caps, lds_entries, C)) return -1;
    const int64_t W = (R + 63) / 64;
    return qn_header_bytes(W) + qr_commit_blocks(window, W) * C.stride + qr_state_bytes(n, window, C.cap[T + 1]);
}

extern "C" int mjx_quench_regions_ell_rp(const int32_t* adj, int64_t n, int d, int64_t R, int p, int c,
                                         uint64_t* const* levels, const int64_t* caps, int lds_entries, void* scratch,
                                         int64_t scratch_bytes, int64_t window, const uint64_t* removable,
                                         const int32_t* cand, int64_t ncand, uint8_t* consensus, int64_t* flipped,
                                         int64_t* stats, int64_t round0, int64_t rounds, void* stream) {
    if (!adj_ell_ok(adj, d)) return MJX_EINVAL;
    return quench_regions_run(AdjEll{adj, d}, n, R, p, c, levels, caps, lds_entries, scratch, scratch_bytes, window,
                              removable, cand, ncand, consensus, flipped, stats, round0, rounds, stream);
}

extern "C" int mjx_quench_regions_csr_rp(const int64_t* row_ptr, const int32_t* col, int64_t n, int64_t R, int p, int c,
                                         uint64_t* const* levels, const int64_t* caps, int lds_entries, void* scratch,
                                         int64_t scratch_bytes, int64_t window, const uint64_t* removable,
                                         const int32_t* cand, int64_t ncand, uint8_t* consensus, int64_t* flipped,
                                         int64_t* stats, int64_t round0, int64_t rounds, void* stream) {
    if (!adj_csr_ok(row_ptr)) return MJX_EINVAL;
    return quench_regions_run(AdjCsr{row_ptr, col}, n, R, p, c, levels, caps, lds_entries, scratch, scratch_bytes,
                              window, removable, cand, ncand, consensus, flipped, stats, round0, rounds, stream);
}
