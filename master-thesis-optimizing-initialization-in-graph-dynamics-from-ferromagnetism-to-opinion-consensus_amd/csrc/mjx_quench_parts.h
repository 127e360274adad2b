// What the two quench units (mjx_quench.hip, mjx_quench_lds.hip) share: the
// adjacency pair, the wave reductions and one offer round of a candidate walk.
// Every device function here is wave-uniform: one wave = the workgroup.
#pragma once
#include "mjx_common.h"

namespace mjx {

// A node index keeps each unit's own type, uint32_t in the cone unit (deg, nbr)
// and int in the LDS unit (deg, row): row(uint32_t) would cost k_quench_jobs a
// second 64-bit multiply-add per row address (v zero-extended times d
// sign-extended) and 2 % of its time.
struct AdjEll {
    const int32_t* adj;
    int d;
    __device__ __forceinline__ AdjEll at(int64_t shift) const { return AdjEll{adj ? adj + shift : adj, d}; }
    template <class V> __device__ __forceinline__ int deg(V) const { return d; }
    __device__ __forceinline__ const int32_t* row(int v) const { return adj + (int64_t)v * d; }
    __device__ __forceinline__ uint32_t nbr(uint32_t v, int e) const { return (uint32_t)adj[(int64_t)v * d + e]; }
    __device__ __forceinline__ int fixed() const { return d; }
};

struct AdjCsr {
    const int64_t* row_ptr;
    const int32_t* col;
    __device__ __forceinline__ AdjCsr at(int64_t) const { return *this; }
    template <class V> __device__ __forceinline__ int deg(V v) const { return (int)(row_ptr[v + 1] - row_ptr[v]); }
    __device__ __forceinline__ const int32_t* row(int v) const { return col + row_ptr[v]; }
    __device__ __forceinline__ uint32_t nbr(uint32_t v, int e) const { return (uint32_t)col[row_ptr[v] + e]; }
    __device__ __forceinline__ int fixed() const { return 0; }
};

// the graph checks of the entry points (HOST)
inline bool adj_ell_ok(const int32_t* adj, int d) { return d >= 0 && d <= 255 && (d == 0 || adj); }
inline bool adj_csr_ok(const int64_t* row_ptr) { return row_ptr != nullptr; }   // no edges: no col array

__device__ __forceinline__ int qn_wave_max(int x) {
    for (int off = 32; off; off >>= 1) {
        const int o = __shfl_xor(x, off);
        x = o > x ? o : x;
    }
    return x;
}

__device__ __forceinline__ u64 qn_wave_or(u64 x) {
    for (int off = 32; off; off >>= 1) x |= (u64)__shfl_xor((long long)x, off);
    return x;
}

constexpr uint32_t kQnNoNode = 0xffffffffu;    // never a node (n < 2^31)

// register of lane m (wave-uniform m)
__device__ __forceinline__ uint32_t qn_lane32(uint32_t x, int m) {
    return (uint32_t)__builtin_amdgcn_readlane((int)x, m);
}

// One offer round of a candidate walk.  Lanes 0 .. lanes-1 offer node x each
// (valid: the lane has one; else x = kQnNoNode); the list so far has nu entries,
// entry q read with get(q).  An offer that is neither in the list nor made by
// a lower lane is appended with put(q, x) and nu grows.  Returns false, with
// nothing appended, when the list would outgrow cap.  Ends with a barrier.
template <class Get, class Put>
__device__ __forceinline__ bool qn_offer(uint32_t x, bool valid, int lanes, int& nu, int cap, Get get, Put put) {
    const int lane = threadIdx.x;
    // bit m of seen: lane m's offer is in the list already, or a lower lane offers it too
    u64 seen = 0;
    for (int m = 0; m < lanes; ++m) {
        const uint32_t y = qn_lane32(x, m);
        if (__ballot(x == y) & ((1ull << m) - 1)) seen |= 1ull << m;
    }
    for (int b = 0; b < nu; b += 64) {
        const uint32_t have = (b + lane < nu) ? get(b + lane) : 0xfffffffeu;
        for (int m = 0; m < lanes; ++m) {
            const uint32_t y = qn_lane32(x, m);
            if (__ballot(have == y)) seen |= 1ull << m;
        }
    }
    const bool fresh = valid && !((seen >> lane) & 1);
    const u64 mask = __ballot(fresh);
    const int total = nu + __popcll(mask);
    const bool ok = total <= cap;
    if (ok && fresh) put(nu + __popcll(mask & ((1ull << lane) - 1)), x);
    nu = ok ? total : nu;
    __syncthreads();
    return ok;
}

}  // namespace mjx
