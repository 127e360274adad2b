// Exact enumerations of a small graph (no reference counterpart; definitions
// in include/mjx.h): every configuration x in [0, 2^n) is run under the
// always-stay majority rule.  k_census runs T steps and counts, in
// counts[t][popcount(x)], the x whose onestep^t(x) is all +1, and with CnNodeArgs
// also counts those of one level per +1 node; k_census_minima
// counts the minimal elements of those levels from their bitmap;
// k_attractor_census runs every x until s(t+2) = s(t) and counts it by class,
// transient and weight.
//
// The frame the kernels share.  A lane owns one 64-config block b at a time:
// bit j of every word it touches is configuration x = 64 b + j, and a wave
// walks the rows of 64 blocks of its launch's range (cn_first, cn_stride).
// Level 0 is never stored: node v < 6 is the constant pattern "bit v of j" (a table of n
// words in LDS, 0 for v >= 6), node v >= 6 is all ones iff bit v-6 of b is set
// -- one OR of the two, no branch on v (cn_level0).  Later levels ping-pong
// between two LDS buffers laid out [node][lane] u64: the lanes of a wave read
// node u at base(u) + 8 lane (conflict-free ds_read_b64, the neighbour index is
// wave-uniform), and a lane only ever reads the words it wrote itself, so the
// sweeps need no barrier.  The adjacency sits in LDS as bytes (n <= 48) behind
// u16 row offsets, and cn_rows walks it with wave-uniform control flow.
// cn_frame sets all of this up; the kernel's own cells (histogram, keys) lie
// behind the two levels in LDS and go to global memory once, at the end.
// cn_bin adds a word of configurations to a histogram row by weight
// (popcount(x) = popcount(b) + the weight of the low six bits) and keeps the
// wave's lightest or heaviest key (k << 48) | x.
//
// The workgroup is one wave.  Everything is integer.
#include "mjx_common.h"
#include <algorithm>

namespace mjx {

constexpr int CN_MAXN = 48;
constexpr int CN_MAXT = 6;
constexpr int CN_MAXDEG = 47;                 // BitCounter<6>; a simple graph on 48 nodes has no longer row
constexpr size_t kCnLdsMax = 64 * 1024;       // no dynamic-LDS opt-in needed
constexpr size_t kCnLdsPerCu = 160 * 1024;    // gfx950: what the workgroups resident on a CU share

constexpr int CN_FLAG_RANGE = 2;              // an adjacency entry outside 0..n-1 (bit 1, as mjx_quench_jobs_*)
constexpr int CN_FLAG_ROW = 4;                // a row longer than CN_MAXDEG, or a decreasing row_ptr

// C_w: the bit positions j of a word with popcount(j) = w
constexpr u64 cn_weight_mask(int w) {
    u64 m = 0;
    for (int j = 0; j < 64; ++j) {
        int pc = 0;
        for (int k = 0; k < 6; ++k) pc += (j >> k) & 1;
        if (pc == w) m |= 1ull << j;
    }
    return m;
}

constexpr u64 kCnWeight[7] = {cn_weight_mask(0), cn_weight_mask(1), cn_weight_mask(2), cn_weight_mask(3),
                              cn_weight_mask(4), cn_weight_mask(5), cn_weight_mask(6)};

__device__ __forceinline__ u64 cn_weight(int w) {
    switch (w) {
        case 0: return kCnWeight[0];
        case 1: return kCnWeight[1];
        case 2: return kCnWeight[2];
        case 3: return kCnWeight[3];
        case 4: return kCnWeight[4];
        case 5: return kCnWeight[5];
        default: return kCnWeight[6];
    }
}

// bytes of the graph part of a workgroup's LDS, in this order; the kernel's own cells lie between `state`
// and `pat`.  Every part is a multiple of 8 bytes.
struct CnLds {
    size_t state, pat, off, nbr;
    __host__ __device__ size_t total() const { return state + pat + off + nbr; }
};

__host__ __device__ inline CnLds cn_lds(int64_t n) {
    CnLds L;
    L.state = (size_t)2 * n * 64 * sizeof(u64);                      // two levels [node][lane]
    L.pat = (size_t)n * sizeof(u64);                                 // level-0 patterns of the nodes
    L.off = ((size_t)(n + 1) * sizeof(uint16_t) + 7) / 8 * 8;        // row offsets
    L.nbr = ((size_t)n * CN_MAXDEG + 7) / 8 * 8;                     // neighbour indices, a byte each
    return L;
}

// blocks of 64 configurations; n < 6: the 2^n configurations are the low bits of block 0 (cn_valid)
__host__ __device__ inline int64_t cn_blocks(int64_t n) { return (int64_t)1 << (n > 6 ? n - 6 : 0); }
__device__ __forceinline__ u64 cn_valid(int n) { return n < 6 ? ((1ull << (1 << n)) - 1) : ~0ull; }

// The accessors copy the adjacency into LDS (off[v] .. off[v+1] of nbr) with
// every entry checked; all 64 lanes call, the result is wave-uniform: 0 or
// the flag bits.  Nothing is read or written out of bounds either way.
struct CnEll {
    const int32_t* adj;
    int d;
    __device__ __forceinline__ int fixed() const { return d; }
    __device__ int load(int n, uint16_t* off, uint8_t* nbr) const {
        const int lane = threadIdx.x;
        bool bad = false;
        for (int v = lane; v <= n; v += 64) off[v] = (uint16_t)(v * d);
        for (int i = lane; i < n * d; i += 64) {
            const int32_t u = adj[i];
            bad |= u < 0 || u >= n;
            nbr[i] = (uint8_t)u;
        }
        return __ballot(bad) ? CN_FLAG_RANGE : 0;
    }
};

struct CnCsr {
    const int64_t* row_ptr;
    const int32_t* col;
    __device__ __forceinline__ int fixed() const { return 0; }
    __device__ int load(int n, uint16_t* off, uint8_t* nbr) const {
        const int lane = threadIdx.x;                                // n + 1 <= 49 row pointers: a lane each
        const int64_t base = row_ptr[0];
        const int64_t mine = row_ptr[lane <= n ? lane : n] - base;
        const int64_t next = row_ptr[lane < n ? lane + 1 : n] - base;
        const bool bad_row = base != 0 || (lane < n && (next < mine || next - mine > CN_MAXDEG));
        if (__ballot(bad_row)) return CN_FLAG_ROW;
        if (lane <= n) off[lane] = (uint16_t)mine;                   // <= n * CN_MAXDEG
        const int total = (int)(row_ptr[n] - base);
        bool bad = false;
        for (int i = lane; i < total; i += 64) {
            const int32_t u = col[base + i];
            bad |= u < 0 || u >= n;
            nbr[i] = (uint8_t)u;
        }
        return __ballot(bad) ? CN_FLAG_RANGE : 0;
    }
};

// level-0 pattern of node u: bit j set iff bit u of j is (u < 6); 0 for the nodes a block index decides
__device__ __forceinline__ u64 cn_pattern(int u) {
    const u64 pat[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull,
                        0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};
    u64 x = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) x = (u == k) ? pat[k] : x;
    return x;
}

// level-0 word of node u in block b from the pattern table (b < 2^42, so bit (u + 58) mod 64 of b is bit
// u-6 for u >= 6 and 0 below)
__device__ __forceinline__ u64 cn_level0(const u64* pat, int u, u64 b) {
    return pat[u] | (0 - ((b >> ((u + 58) & 63)) & 1));
}

struct CnFrame {
    u64* buf;                    // the two levels
    const u64* pat;
    const uint16_t* off;
    const uint8_t* nbr;
    int fixed;                   // the degree of every row (3 and 4 have loops of their own), or 0
};

// Carves the workgroup's LDS, copies the adjacency in, fills the pattern table and has init(own) set the
// kernel's own cells, `own_bytes` of them.  false (wave-uniform, after raising the flag bits): the
// adjacency is bad, return.
template <class Adj, class Init>
__device__ __forceinline__ bool cn_frame(const Adj& A, int n, int32_t* flag, CnFrame& F, size_t own_bytes,
                                         Init init) {
    extern __shared__ __align__(8) unsigned char cn_smem[];
    const CnLds L = cn_lds(n);
    unsigned char* own = cn_smem + L.state;
    u64* pat = (u64*)(own + own_bytes);
    uint16_t* off = (uint16_t*)(own + own_bytes + L.pat);
    uint8_t* nbr = own + own_bytes + L.pat + L.off;
    const int lane = threadIdx.x;
    const int bad = A.load(n, off, nbr);
    if (bad) {
        if (lane == 0) atomicOr(flag, bad);
        return false;
    }
    init(own);
    if (lane < n) pat[lane] = cn_pattern(lane);
    __syncthreads();
    F = {(u64*)cn_smem, pat, off, nbr, A.fixed()};
    return true;
}

// the rows of 64 blocks that this workgroup walks: for (first = cn_first(block_lo); first < block_hi;
// first += cn_stride())
__device__ __forceinline__ u64 cn_first(u64 block_lo) { return block_lo + (u64)blockIdx.x * 64; }
__device__ __forceinline__ u64 cn_stride() { return (u64)gridDim.x * 64; }

// the smallest, or the LARGEST, x of the wave, in every lane
template <bool LARGEST>
__device__ __forceinline__ u64 cn_wave_pick(u64 x) {
    for (int off = 32; off; off >>= 1) {
        const u64 o = (u64)__shfl_xor((long long)x, off);
        x = (LARGEST ? o > x : o < x) ? o : x;
    }
    return x;
}

// The configurations m of the lane's block b into row[k], k = kb + the weight of the low six bits, and
// the wave's key (k << 48) | x into *best: the smallest (k, x) of m under an atomic min (CN_LIGHTEST; an
// empty *best is all ones) or the largest under an atomic max (CN_HEAVIEST; empty is 0).  Nothing is
// touched when m is empty in every lane.
enum CnKey { CN_NO_KEY, CN_LIGHTEST, CN_HEAVIEST };

template <CnKey KEY, class Cell>
__device__ __forceinline__ void cn_bin(Cell* row, u64 m, int kb, u64 b, u64* best = nullptr) {
    if (__ballot(m != 0) == 0) return;
    u64 key = KEY == CN_LIGHTEST ? ~0ull : 0;                        // of the last weight that has a configuration
#pragma unroll
    for (int i = 0; i <= 6; ++i) {
        const int w = KEY == CN_LIGHTEST ? 6 - i : i;
        const u64 x = m & cn_weight(w);
        if (x) {
            atomicAdd(&row[kb + w], (Cell)__popcll(x));
            const int j = KEY == CN_LIGHTEST ? __builtin_ctzll(x) : 63 - __builtin_clzll(x);
            if (KEY != CN_NO_KEY) key = ((u64)(kb + w) << 48) | (b * 64 + (u64)j);
        }
    }
    if (KEY == CN_NO_KEY) return;
    key = cn_wave_pick<KEY == CN_HEAVIEST>(key);
    if (threadIdx.x == 0) KEY == CN_LIGHTEST ? atomicMin(best, key) : atomicMax(best, key);
}

// One pass over the nodes: put(v, new word of v, own) with the neighbours' and the own word from word(u).
// OWN: put reads `own` even where the majority does not (odd fixed degree); without it, it is 0 there and
// never loaded.  Wave-uniform control flow (v, the row and its entries are the same in every lane).  The
// regular degrees keep eight nodes' reads in flight together (a lone wave per SIMD waits for every LDS
// round trip it does not overlap).
template <bool OWN, class Word, class Put>
__device__ __forceinline__ void cn_rows(int n, int fixed, const uint16_t* __restrict__ off,
                                        const uint8_t* __restrict__ nbr, Word word, Put put) {
    if (fixed == 3) {
#pragma unroll 8
        for (int v = 0; v < n; ++v) {
            const uint8_t* row = nbr + 3 * v;
            const u64 x[3] = {word(row[0]), word(row[1]), word(row[2])};
            put(v, majority_fixed<3>(x, 0), OWN ? word(v) : 0);
        }
    } else if (fixed == 4) {
#pragma unroll 8
        for (int v = 0; v < n; ++v) {
            const uint8_t* row = nbr + 4 * v;
            const u64 x[4] = {word(row[0]), word(row[1]), word(row[2]), word(row[3])};
            const u64 own = word(v);
            put(v, majority_fixed<4>(x, own), own);
        }
    } else {
        for (int v = 0; v < n; ++v) {
            const int e0 = off[v], e1 = off[v + 1];
            BitCounter<6> bc;                                        // degree <= 47; degree 0 keeps the word
            bc.reset();
            for (int e = e0; e < e1; ++e) bc.add(word(nbr[e]));
            const u64 own = word(v);
            put(v, bc.majority(e1 - e0, own), own);
        }
    }
}

// One sweep: level lv (>= 1) of the lane's block into `dst`, from level lv-1.  FIRST: the source is level
// 0, generated from b and the pattern table `src`; else the other LDS buffer `src`.  Returns the AND of
// the new words.
template <bool FIRST>
__device__ __forceinline__ u64 cn_sweep(const CnFrame& F, int n, const u64* __restrict__ src,
                                        u64* __restrict__ dst, u64 b, int lane) {
    u64 all = ~0ull;
    cn_rows<false>(
        n, F.fixed, F.off, F.nbr, [&](int u) -> u64 { return FIRST ? cn_level0(src, u, b) : src[u * 64 + lane]; },
        [&](int v, u64 nw, u64) {
            dst[v * 64 + lane] = nw;
            all &= nw;
        });
    return all;
}

// k_census's own cells: hist[CN_MAXT + 1][n + 1] and the smallest key of every level, u64
__host__ __device__ inline size_t cn_cells(int64_t n) { return (size_t)(CN_MAXT + 1) * (n + 2) * sizeof(u64); }

// the node cells behind k_census's own when it counts per node: node[n + 1][n], 32 bits each (n (n + 1) is
// even: a multiple of 8 bytes)
__host__ __device__ inline size_t cn_node_cells(int64_t n) { return (size_t)(n + 1) * n * sizeof(uint32_t); }

// The configurations m of the lane's block b into node[k][v] for every +1 node v of each, k as in cn_bin.
// Node v < 6 is a bit of the position in the word: the level-0 pattern picks its configurations.  Node
// v >= 6 is bit v - 6 of b: set, it takes the whole word.  A row that starts at a multiple of 64 (`first`,
// wave-uniform) has the bits from 6 on of b the same in every lane, so the words of the wave are summed by
// weight once -- k = popcount(first >> 6) + j, j = popcount(lane) + the weight in the word = 0..12 -- and
// lane l adds the 13 sums for node 12 + l; in any other row every lane adds for its own b.  Nothing is
// touched when m is empty in every lane.
__device__ __forceinline__ void cn_bin_nodes(uint32_t* node, int n, u64 m, int kb, u64 b, u64 first) {
    if (__ballot(m != 0) == 0) return;
    const int lane = threadIdx.x;
    const bool aligned = (first & 63) == 0;
    const int own_end = (aligned && n > 12) ? 12 : n;                // below: the nodes a lane adds for itself
    int cw[7];
#pragma unroll
    for (int w = 0; w <= 6; ++w) {
        const u64 x = m & cn_weight(w);
        cw[w] = __popcll(x);
        if (x) {
            uint32_t* row = node + (kb + w) * n;
#pragma unroll
            for (int v = 0; v < 6; ++v) {
                const int in = __popcll(x & cn_pattern(v));
                if (v < n && in) atomicAdd(&row[v], (uint32_t)in);
            }
            for (int v = 6; v < own_end; ++v)
                if ((b >> (v - 6)) & 1) atomicAdd(&row[v], (uint32_t)cw[w]);
        }
    }
    if (own_end == n) return;
    const int pl = __popc(lane), v = 12 + lane;
    const bool mine = v < n && ((first >> (v < n ? v - 6 : 0)) & 1);
    uint32_t* col = node + __popcll(first >> 6) * n + (mine ? v : 0);
#pragma unroll
    for (int j = 0; j <= 12; ++j) {
        int s = 0;
#pragma unroll
        for (int w = 0; w <= 6; ++w) s = (j - pl == w) ? cw[w] : s;
        for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
        if (mine && s) atomicAdd(&col[j * n], (uint32_t)s);
    }
}

// k_census's trailing argument when it also counts per node: the level, and node_counts[n + 1][n]
struct CnNodeArgs {
    int t_node;
    u64* out;
};
__device__ __forceinline__ CnNodeArgs cn_node_args() { return {0, nullptr}; }
__device__ __forceinline__ CnNodeArgs cn_node_args(CnNodeArgs a) { return a; }

// A full block stays full (all +1 is a fixed point), so a row is swept only while some lane's is not.
// MASK: the level's word of every block of the range is stored at bits[t * B + b], the words of the
// levels that are not swept (zero words, full blocks) included; without it no mask code is compiled.
// Nodes: nothing, or CnNodeArgs: the configurations of level t_node are also counted per +1 node, in
// 32-bit cells behind the keys that are added to `out` at the end.  An empty pack leaves the kernel's
// arguments and code as they are without it.
template <class Adj, bool MASK, class... Nodes>
__global__ void __launch_bounds__(64) k_census(Adj A, int n, int T, u64 block_lo, u64 block_hi,
                                               u64* __restrict__ counts, u64* __restrict__ witness,
                                               int32_t* __restrict__ flag, u64* __restrict__ bits, Nodes... nodes) {
    constexpr bool NODES = sizeof...(Nodes) > 0;
    const int lane = threadIdx.x;
    const int cells = (T + 1) * (n + 1);
    CnFrame F;
    u64 *hist, *best;
    uint32_t* node;
    if (!cn_frame(A, n, flag, F, cn_cells(n) + (NODES ? cn_node_cells(n) : 0), [&](unsigned char* own) {
            hist = (u64*)own;
            best = hist + (CN_MAXT + 1) * (n + 1);
            for (int i = lane; i < cells; i += 64) hist[i] = 0;
            if (lane <= CN_MAXT) best[lane] = ~0ull;
            if (NODES) {
                node = (uint32_t*)(own + cn_cells(n));
                for (int i = lane; i < (n + 1) * n; i += 64) node[i] = 0;
            }
        }))
        return;

    const u64 valid = cn_valid(n), B = cn_blocks(n);
    const u64 last_bit = 1ull << ((n < 6 ? (1 << n) : 64) - 1);     // level 0: all +1 ends the last block
    for (u64 first = cn_first(block_lo); first < block_hi; first += cn_stride()) {
        const u64 b = first + lane;
        const bool active = b < block_hi;
        const int kb = __popcll(b);                                  // weight of the nodes >= 6
        u64 mask = (active && b == B - 1) ? last_bit : 0;
#pragma unroll 1
        for (int t = 0; t <= T; ++t) {
            if (t > 0 && __ballot(active && mask != valid)) {
                u64* dst = F.buf + (size_t)((t - 1) & 1) * n * 64;
                const u64* src = F.buf + (size_t)(t & 1) * n * 64;
                const u64 all = (t == 1) ? cn_sweep<true>(F, n, F.pat, dst, b, lane)
                                         : cn_sweep<false>(F, n, src, dst, b, lane);
                mask = active ? (all & valid) : 0;
            }
            if (MASK && active) bits[(u64)t * B + b] = mask;
            cn_bin<CN_LIGHTEST>(hist + t * (n + 1), mask, kb, b, &best[t]);
            if (NODES && t == cn_node_args(nodes...).t_node) cn_bin_nodes(node, n, mask, kb, b, first);
        }
    }
    __syncthreads();
    for (int i = lane; i < cells; i += 64)
        if (hist[i]) atomicAdd(&counts[i], hist[i]);
    if (lane <= T && best[lane] != ~0ull) atomicMin(&witness[lane], best[lane]);
    if (NODES)
        for (int i = lane; i < (n + 1) * n; i += 64)
            if (node[i]) atomicAdd(&cn_node_args(nodes...).out[i], (u64)node[i]);
}

// The minimal elements of a bitmap's levels.  No adjacency and no sweep: a wave owns the 64 consecutive
// blocks first .. first + 63 (first a multiple of 64, so lane = the low six bits of b) and
// builds r, the word of the configurations that stay in the set when some +1 node v is dropped, from the
// words of the blocks b with bit v cleared: inside its own word (v < 6), in lane ^ 2^(v-6) (v < 12),
// and in the row of 64 words at first ^ 2^(v-6) (v >= 12: that bit of b is the same in the whole wave,
// four such rows are loaded together).  Minimal is mask & ~r.
constexpr int CN_MIN_ROWS = 4;
constexpr int CN_MIN_CELLS = (CN_MAXT + 1) * (CN_MAXN + 1);
constexpr size_t kCnMinimaLds = (CN_MIN_CELLS + CN_MAXT + 1) * sizeof(u64);    // its static LDS, before padding

__global__ void __launch_bounds__(64) k_census_minima(const u64* __restrict__ bits, int n, int T, u64 block_lo,
                                                      u64 block_hi, u64* __restrict__ minima,
                                                      u64* __restrict__ heaviest) {
    __shared__ u64 hist[CN_MIN_CELLS];
    __shared__ u64 best[CN_MAXT + 1];                                // largest key of level t in this workgroup
    const int lane = threadIdx.x;
    const int cells = (T + 1) * (n + 1);
    for (int i = lane; i < cells; i += 64) hist[i] = 0;
    if (lane <= CN_MAXT) best[lane] = 0;
    __syncthreads();

    const u64 valid = cn_valid(n), B = cn_blocks(n);
    const int in_word = n < 6 ? n : 6, in_wave = n < 12 ? n : 12;
    for (u64 first = cn_first(block_lo); first < block_hi; first += cn_stride()) {
        const u64 b = first + lane;
        const bool active = b < block_hi;                            // a last row shorter than 64: B < 64
        const int kb = __popcll(b);
#pragma unroll 1
        for (int t = 0; t <= T; ++t) {
            const u64* row = bits + (u64)t * B;
            const u64 m = active ? row[b] & valid : 0;
            if (__ballot(m != 0) == 0) continue;                     // nothing counted here: no neighbour is read
            u64 r = 0;
            for (int v = 0; v < in_word; ++v) r |= (m << (1 << v)) & cn_pattern(v);
            for (int v = 6; v < in_wave; ++v) {
                const u64 o = (u64)__shfl_xor((long long)m, 1 << (v - 6));
                r |= ((lane >> (v - 6)) & 1) ? o : 0;
            }
            // the set bits of first >> 6 are the nodes v >= 12 that are +1 in the whole wave; the partner
            // rows lie below first, inside [0, B).  A round without a node left reads the own row again.
            u64 up = first >> 6;
            while (up && __ballot((m & ~r) != 0)) {
                u64 o[CN_MIN_ROWS];
#pragma unroll
                for (int i = 0; i < CN_MIN_ROWS; ++i) {
                    const u64 bit = up & (0 - up);
                    up ^= bit;
                    const u64 w = row[(first ^ (bit << 6)) + lane];
                    o[i] = bit ? w : 0;
                }
#pragma unroll
                for (int i = 0; i < CN_MIN_ROWS; ++i) r |= o[i];
            }
            cn_bin<CN_HEAVIEST>(hist + t * (n + 1), m & ~r, kb, b, &best[t]);
        }
    }
    __syncthreads();
    for (int i = lane; i < cells; i += 64)
        if (hist[i]) atomicAdd(&minima[i], hist[i]);
    if (lane <= T && best[lane]) atomicMax(&heaviest[lane], best[lane]);
}

// ---- attractor census ----------------------------------------------------------------------------
// Run to the attractor instead of a fixed horizon.  Sweep t reads s(t-1) from buf[(t-1) & 1] and writes
// s(t) over s(t-2) in buf[t & 1], and before the store ORs new ^ s(t-2) into chg2 and new ^ s(t-1) into
// chg1 and keeps the AND and the OR of the new words.  Sweep 1 is cn_sweep<true> (from the generated
// level 0), sweep 2 compares against the generated level 0, from sweep 3 on everything is in place.  A bit
// of the lane's word `unsettled` leaves after the first sweep t >= 2 whose chg2 bit is 0: p = t - 2, and
// chg1 / AND / OR of that sweep name the class.
constexpr int ACN_MAXT = 1024;                // t_max at most; the LDS ceiling is reached sooner for n >= 4
constexpr int64_t ACN_MAXBLOCKS = (int64_t)1 << 25;    // blocks per launch: the LDS cells are 32 bits wide

// bytes of k_attractor_census's own cells, in this order
struct AcCells {
    size_t hist, uns, keys;
    __host__ __device__ size_t total() const { return hist + uns + keys; }
};

__host__ __device__ inline AcCells ac_cells(int64_t n, int64_t t_max) {
    AcCells C;
    C.hist = (size_t)4 * (t_max + 1) * (n + 1) * sizeof(uint32_t);   // [class][p][k], a multiple of 8
    C.uns = ((size_t)(n + 1) * sizeof(uint32_t) + 7) / 8 * 8;        // unsettled[k]
    C.keys = 2 * sizeof(u64);                                        // lightest plus, longest
    return C;
}

struct AcTrack {
    u64 chg1, chg2, all, any;    // OR of new ^ s(t-1), OR of new ^ s(t-2), AND and OR of the new words
};

// One tracked sweep: level t (>= 2) of the lane's block from level t-1 in `src`, written over level t-2
// in `dst` (no __restrict__: dst is read before it is written).  SECOND (t = 2): level t-2 is
// level 0, generated from b and the pattern table `pat`; else it is the word the store replaces.
template <bool SECOND>
__device__ __forceinline__ AcTrack ac_sweep(const CnFrame& F, int n, const u64* __restrict__ pat, const u64* src,
                                            u64* dst, u64 b, int lane) {
    AcTrack k = {0, 0, ~0ull, 0};
    cn_rows<true>(
        n, F.fixed, F.off, F.nbr, [&](int u) -> u64 { return src[u * 64 + lane]; },
        [&](int v, u64 nw, u64 own) {
            const u64 old = SECOND ? cn_level0(pat, v, b) : dst[v * 64 + lane];
            k.chg2 |= nw ^ old;
            k.chg1 |= nw ^ own;
            k.all &= nw;
            k.any |= nw;
            dst[v * 64 + lane] = nw;
        });
    return k;
}

template <class Adj>
__global__ void __launch_bounds__(64) k_attractor_census(Adj A, int n, int t_max, u64 block_lo, u64 block_hi,
                                                         u64* __restrict__ hist_out, u64* __restrict__ uns_out,
                                                         u64* __restrict__ keys, int32_t* __restrict__ flag,
                                                         u64* __restrict__ stats) {
    const int lane = threadIdx.x;
    const int row = n + 1, plane = (t_max + 1) * row, cells = 4 * plane;
    CnFrame F;
    uint32_t *hist, *uns;
    u64* best;                                                       // [0] smallest plus key, [1] largest (p, x) key
    const AcCells C = ac_cells(n, t_max);
    if (!cn_frame(A, n, flag, F, C.total(), [&](unsigned char* own) {
            hist = (uint32_t*)own;
            uns = (uint32_t*)(own + C.hist);
            best = (u64*)(own + C.hist + C.uns);
            for (int i = lane; i < cells; i += 64) hist[i] = 0;
            if (lane < row) uns[lane] = 0;
            if (lane == 0) best[0] = ~0ull, best[1] = 0;
        }))
        return;

    const u64 valid = cn_valid(n);
    u64 rows = 0, sweeps = 0;                                        // wave-uniform: for stats
    for (u64 first = cn_first(block_lo); first < block_hi; first += cn_stride()) {
        const u64 b = first + lane;
        const int kb = __popcll(b);                                  // weight of the nodes >= 6
        u64 unsettled = b < block_hi ? valid : 0;
        cn_sweep<true>(F, n, F.pat, F.buf + (size_t)n * 64, b, lane);    // s(1)
        int t = 1;
#pragma unroll 1
        while (t < t_max + 2 && __ballot(unsettled != 0)) {
            ++t;
            u64* dst = F.buf + (size_t)(t & 1) * n * 64;
            const u64* src = F.buf + (size_t)((t - 1) & 1) * n * 64;
            const AcTrack k = (t == 2) ? ac_sweep<true>(F, n, F.pat, src, dst, b, lane)
                                       : ac_sweep<false>(F, n, F.pat, src, dst, b, lane);
            const u64 newly = unsettled & ~k.chg2;                   // s(t) = s(t-2) for the first time: p = t - 2
            unsettled &= k.chg2;
            if (__ballot(newly != 0) == 0) continue;
            uint32_t* at = hist + (t - 2) * row;
            const u64 plus = newly & k.all, minus = newly & ~k.any, cycle = newly & k.chg1;
            cn_bin<CN_NO_KEY>(at + plane, minus, kb, b);
            cn_bin<CN_NO_KEY>(at + 2 * plane, newly & ~(plus | minus | cycle), kb, b);
            cn_bin<CN_NO_KEY>(at + 3 * plane, cycle, kb, b);
            cn_bin<CN_LIGHTEST>(at, plus, kb, b, &best[0]);
            const u64 far = newly ? ((u64)(t - 2) << 48) | (b * 64 + (u64)(63 - __builtin_clzll(newly))) : 0;
            const u64 longest = cn_wave_pick<true>(far);
            if (lane == 0) atomicMax(&best[1], longest);
        }
        cn_bin<CN_NO_KEY>(uns, unsettled, kb, b);                    // p > t_max
        ++rows;
        sweeps += (u64)t;
    }
    __syncthreads();
    for (int i = lane; i < cells; i += 64)
        if (hist[i]) atomicAdd(&hist_out[i], (u64)hist[i]);
    if (lane < row && uns[lane]) atomicAdd(&uns_out[lane], (u64)uns[lane]);
    if (lane == 0) {
        if (best[0] != ~0ull) atomicMin(&keys[0], best[0]);
        if (best[1]) atomicMax(&keys[1], best[1]);
        if (stats) {
            atomicAdd(&stats[0], rows);
            atomicAdd(&stats[1], sweeps);
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------
static int cn_check_ell(const int32_t* adj, int d) {
    if (d < 0 || (d > 0 && !adj)) return MJX_EINVAL;
    return d > CN_MAXDEG ? MJX_ERANGE : MJX_OK;
}

static int cn_check_csr(const int64_t* row_ptr) {
    return row_ptr ? MJX_OK : MJX_EINVAL;                            // a graph without edges has no col array
}

static bool cn_range_ok(int64_t n, int64_t block_lo, int64_t block_hi) {
    return block_lo >= 0 && block_lo <= block_hi && block_hi <= cn_blocks(n);
}

// `grid`, or the library's: the workgroups the LDS lets a CU hold at once (at most 8 a SIMD), every lane
// walking its share of the `blocks` of the launch
static int cn_grid(size_t lds_bytes, int64_t blocks, int grid) {
    if (grid) return grid;
    const int64_t per = std::min<int64_t>(32, (int64_t)(kCnLdsPerCu / lds_bytes));
    return (int)std::max<int64_t>(1, std::min<int64_t>((blocks + 63) / 64, device_cus() * per));
}

template <class Adj>
static int census_run(int rc, Adj A, int64_t n, int p, int c, int64_t block_lo, int64_t block_hi, int grid,
                      unsigned long long* counts, unsigned long long* witness_key, int32_t* flag, bool keep,
                      uint64_t* mask, void* stream) {
    if (rc) return rc;
    if (p < 0 || c < 0 || p + c - 1 < 0 || n < 1 || !counts || !witness_key || !flag || grid < 0) return MJX_EINVAL;
    if (keep && !mask) return MJX_EINVAL;
    if (n > CN_MAXN || p + c - 1 > CN_MAXT) return MJX_ERANGE;
    if (!cn_range_ok(n, block_lo, block_hi)) return MJX_EINVAL;
    if (block_lo == block_hi) return MJX_OK;
    const size_t lds = cn_lds(n).total() + cn_cells(n);
    const int g = cn_grid(lds, block_hi - block_lo, grid);
    if (keep)
        k_census<Adj, true><<<(unsigned)g, 64, lds, as_stream(stream)>>>(
            A, (int)n, p + c - 1, (u64)block_lo, (u64)block_hi, counts, witness_key, flag, (u64*)mask);
    else
        k_census<Adj, false><<<(unsigned)g, 64, lds, as_stream(stream)>>>(
            A, (int)n, p + c - 1, (u64)block_lo, (u64)block_hi, counts, witness_key, flag, nullptr);
    MJX_LAUNCH_CHECK("k_census");
    return MJX_OK;
}

template <class Adj>
static int census_nodes_run(int rc, Adj A, int64_t n, int p, int c, int t_node, int64_t block_lo, int64_t block_hi,
                            int grid, unsigned long long* counts, unsigned long long* witness_key,
                            unsigned long long* node_counts, int32_t* flag, void* stream) {
    if (rc) return rc;
    if (p < 0 || c < 0 || p + c - 1 < 0 || n < 1 || !counts || !witness_key || !node_counts || !flag || grid < 0)
        return MJX_EINVAL;
    if (n > CN_MAXN || p + c - 1 > CN_MAXT) return MJX_ERANGE;
    if (t_node < 0 || t_node > p + c - 1) return MJX_EINVAL;
    const size_t lds = cn_lds(n).total() + cn_cells(n) + cn_node_cells(n);
    if (lds > kCnLdsMax) return MJX_EINVAL;
    if (!cn_range_ok(n, block_lo, block_hi)) return MJX_EINVAL;
    // a workgroup's 32-bit node cell counts at most the 64 * 2^25 = 2^31 configurations of the launch
    if (block_hi - block_lo > ACN_MAXBLOCKS) return MJX_ERANGE;
    if (block_lo == block_hi) return MJX_OK;
    const int g = cn_grid(lds, block_hi - block_lo, grid);
    k_census<Adj, false, CnNodeArgs><<<(unsigned)g, 64, lds, as_stream(stream)>>>(
        A, (int)n, p + c - 1, (u64)block_lo, (u64)block_hi, counts, witness_key, flag, nullptr,
        CnNodeArgs{t_node, (u64*)node_counts});
    MJX_LAUNCH_CHECK("k_census<nodes>");
    return MJX_OK;
}

template <class Adj>
static int attractor_census_run(int rc, Adj A, int64_t n, int t_max, int64_t block_lo, int64_t block_hi, int grid,
                                unsigned long long* hist, unsigned long long* unsettled, unsigned long long* keys,
                                int32_t* flag, unsigned long long* stats, void* stream) {
    if (rc) return rc;
    if (t_max < 0 || n < 1 || !hist || !unsettled || !keys || !flag || grid < 0) return MJX_EINVAL;
    if (n > CN_MAXN || t_max > ACN_MAXT) return MJX_ERANGE;
    const size_t lds = cn_lds(n).total() + ac_cells(n, t_max).total();
    if (lds > kCnLdsMax) return MJX_EINVAL;
    if (!cn_range_ok(n, block_lo, block_hi)) return MJX_EINVAL;
    // a workgroup's 32-bit LDS cell counts at most the 64 * 2^25 = 2^31 configurations of the launch
    if (block_hi - block_lo > ACN_MAXBLOCKS) return MJX_ERANGE;
    if (block_lo == block_hi) return MJX_OK;
    const int g = cn_grid(lds, block_hi - block_lo, grid);
    k_attractor_census<Adj><<<(unsigned)g, 64, lds, as_stream(stream)>>>(
        A, (int)n, t_max, (u64)block_lo, (u64)block_hi, hist, unsettled, keys, flag, stats);
    MJX_LAUNCH_CHECK("k_attractor_census");
    return MJX_OK;
}

}  // namespace mjx

using namespace mjx;

extern "C" int64_t mjx_attractor_census_lds(int64_t n, int t_max) {
    if (n < 1 || n > CN_MAXN || t_max < 0 || t_max > ACN_MAXT) return -1;
    const size_t b = cn_lds(n).total() + ac_cells(n, t_max).total();
    return b > kCnLdsMax ? -1 : (int64_t)b;
}

extern "C" int mjx_attractor_census_ell(const int32_t* adj, int64_t n, int d, int t_max, int64_t block_lo,
                                        int64_t block_hi, int grid, unsigned long long* hist,
                                        unsigned long long* unsettled, unsigned long long* keys, int32_t* flag,
                                        unsigned long long* stats, void* stream) {
    return attractor_census_run(cn_check_ell(adj, d), CnEll{adj, d}, n, t_max, block_lo, block_hi, grid, hist,
                                unsettled, keys, flag, stats, stream);
}

extern "C" int mjx_attractor_census_csr(const int64_t* row_ptr, const int32_t* col, int64_t n, int t_max,
                                        int64_t block_lo, int64_t block_hi, int grid, unsigned long long* hist,
                                        unsigned long long* unsettled, unsigned long long* keys, int32_t* flag,
                                        unsigned long long* stats, void* stream) {
    return attractor_census_run(cn_check_csr(row_ptr), CnCsr{row_ptr, col}, n, t_max, block_lo, block_hi, grid, hist,
                                unsettled, keys, flag, stats, stream);
}

extern "C" int64_t mjx_census_lds(int64_t n) {
    if (n < 1 || n > CN_MAXN) return -1;
    const size_t b = cn_lds(n).total() + cn_cells(n);
    return b > kCnLdsMax ? -1 : (int64_t)b;
}

extern "C" int mjx_census_ell(const int32_t* adj, int64_t n, int d, int p, int c, int64_t block_lo, int64_t block_hi,
                              int grid, unsigned long long* counts, unsigned long long* witness_key, int32_t* flag,
                              void* stream) {
    return census_run(cn_check_ell(adj, d), CnEll{adj, d}, n, p, c, block_lo, block_hi, grid, counts, witness_key,
                      flag, false, nullptr, stream);
}

extern "C" int mjx_census_csr(const int64_t* row_ptr, const int32_t* col, int64_t n, int p, int c, int64_t block_lo,
                              int64_t block_hi, int grid, unsigned long long* counts, unsigned long long* witness_key,
                              int32_t* flag, void* stream) {
    return census_run(cn_check_csr(row_ptr), CnCsr{row_ptr, col}, n, p, c, block_lo, block_hi, grid, counts,
                      witness_key, flag, false, nullptr, stream);
}

extern "C" int mjx_census_mask_ell(const int32_t* adj, int64_t n, int d, int p, int c, int64_t block_lo,
                                   int64_t block_hi, int grid, unsigned long long* counts,
                                   unsigned long long* witness_key, int32_t* flag, uint64_t* mask, void* stream) {
    return census_run(cn_check_ell(adj, d), CnEll{adj, d}, n, p, c, block_lo, block_hi, grid, counts, witness_key,
                      flag, true, mask, stream);
}

extern "C" int mjx_census_mask_csr(const int64_t* row_ptr, const int32_t* col, int64_t n, int p, int c,
                                   int64_t block_lo, int64_t block_hi, int grid, unsigned long long* counts,
                                   unsigned long long* witness_key, int32_t* flag, uint64_t* mask, void* stream) {
    return census_run(cn_check_csr(row_ptr), CnCsr{row_ptr, col}, n, p, c, block_lo, block_hi, grid, counts,
                      witness_key, flag, true, mask, stream);
}

extern "C" int64_t mjx_census_nodes_lds(int64_t n) {
    if (n < 1 || n > CN_MAXN) return -1;
    const size_t b = cn_lds(n).total() + cn_cells(n) + cn_node_cells(n);
    return b > kCnLdsMax ? -1 : (int64_t)b;
}

extern "C" int mjx_census_nodes_ell(const int32_t* adj, int64_t n, int d, int p, int c, int t_node, int64_t block_lo,
                                    int64_t block_hi, int grid, unsigned long long* counts,
                                    unsigned long long* witness_key, unsigned long long* node_counts, int32_t* flag,
                                    void* stream) {
    return census_nodes_run(cn_check_ell(adj, d), CnEll{adj, d}, n, p, c, t_node, block_lo, block_hi, grid, counts,
                            witness_key, node_counts, flag, stream);
}

extern "C" int mjx_census_nodes_csr(const int64_t* row_ptr, const int32_t* col, int64_t n, int p, int c, int t_node,
                                    int64_t block_lo, int64_t block_hi, int grid, unsigned long long* counts,
                                    unsigned long long* witness_key, unsigned long long* node_counts, int32_t* flag,
                                    void* stream) {
    return census_nodes_run(cn_check_csr(row_ptr), CnCsr{row_ptr, col}, n, p, c, t_node, block_lo, block_hi, grid,
                            counts, witness_key, node_counts, flag, stream);
}

extern "C" int mjx_census_minima(const uint64_t* mask, int64_t n, int T, int64_t block_lo, int64_t block_hi, int grid,
                                 unsigned long long* minima, unsigned long long* heaviest_key, void* stream) {
    if (!mask || !minima || !heaviest_key || n < 1 || T < 0 || grid < 0) return MJX_EINVAL;
    if (n > CN_MAXN || T > CN_MAXT) return MJX_ERANGE;
    if (!cn_range_ok(n, block_lo, block_hi)) return MJX_EINVAL;
    // a wave's 64 blocks go together
    if (block_lo % 64 || (block_hi % 64 && block_hi != cn_blocks(n))) return MJX_EINVAL;
    if (block_lo == block_hi) return MJX_OK;
    // kCnLdsPerCu / kCnMinimaLds = 163840 / 2800 = 58 (as with the few bytes of padding between the two
    // arrays): the LDS allows more than the 32 one-wave workgroups a CU holds, so cn_grid takes 32 a CU
    k_census_minima<<<(unsigned)cn_grid(kCnMinimaLds, block_hi - block_lo, grid), 64, 0, as_stream(stream)>>>(
        (const u64*)mask, (int)n, T, (u64)block_lo, (u64)block_hi, minima, heaviest_key);
    MJX_LAUNCH_CHECK("k_census_minima");
    return MJX_OK;
}
