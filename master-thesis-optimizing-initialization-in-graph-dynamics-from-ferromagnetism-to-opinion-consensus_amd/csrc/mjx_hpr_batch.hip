// HPR on a union of G graphs (hpr_batch.py): the per-instance consensus test and
// stop of the main loop (code/HPR_pytorch_RRG.py:352-356) on the device.
//
// The union's rollout leaves one node-packed end state of G*n bits; instance g
// owns the bit range [g*n, (g+1)*n), whose ends fall anywhere inside a 64-bit
// word.  One workgroup per instance counts its +1 bits and, for an instance
// that has not stopped yet, applies the reference's test in the reference's
// order (t > TT first, then sum(s_end)/n >= 1), records the stop iteration and
// keeps the trial configuration the loop stops with.
#include "mjx_common.h"

namespace mjx {
namespace hprb {

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads) k_hpr_batch_record(const u64* __restrict__ bits,
                                                               const int32_t* __restrict__ s, int64_t n,
                                                               const int32_t* __restrict__ inst,
                                                               const int64_t* __restrict__ t_base, int64_t t_add,
                                                               int64_t TT, u64* __restrict__ counts,
                                                               int32_t* __restrict__ done, int64_t* __restrict__ t_stop,
                                                               int32_t* __restrict__ conf, u64* __restrict__ live) {
    __shared__ int part[kThreads / 64];
    __shared__ int verdict;                    // 0 leave alone, 1 consensus, 2 iteration cap
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    const int64_t o = inst ? (int64_t)inst[g] : g;     // where this instance's results go
    const int64_t lo = g * n, hi = lo + n;             // its bits
    const int64_t w0 = lo >> 6, w1 = (hi - 1) >> 6;
    int c = 0;
    for (int64_t w = w0 + tid; w <= w1; w += kThreads) {
        u64 x = bits[w];
        if (w == w0) x &= ~0ull << (lo & 63);
        if (w == w1 && (hi & 63)) x &= ~0ull >> (64 - (hi & 63));
        c += __popcll(x);
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((tid & 63) == 0) part[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
        for (int k = 0; k < kThreads / 64; ++k) tot += part[k];
        counts[g] = (u64)tot;
        const int64_t t = (t_base ? *t_base : 0) + t_add;
        int v = 0;
        if (done[o] == 0) v = t > TT ? 2 : ((int64_t)tot == n ? 1 : 0);
        verdict = v;
        if (v) t_stop[o] = t;
    }
    __syncthreads();
    const int v = verdict;
    if (!v) return;
    for (int64_t i = tid; i < n; i += kThreads) conf[o * n + i] = s[lo + i];
    if (tid == 0) {
        done[o] = v;                           // read by this workgroup only
        atomicAdd(live, ~0ull);                // *live -= 1
    }
}

}  // namespace hprb
}  // namespace mjx

using namespace mjx;

extern "C" int mjx_hpr_batch_record(const uint64_t* bits, const int32_t* s, int64_t n, int64_t G,
                                    const int32_t* inst, const int64_t* t_base, int64_t t_add, int64_t TT,
                                    unsigned long long* counts, int32_t* done, int64_t* t_stop, int32_t* conf,
                                    unsigned long long* live, void* stream) {
    if (n < 1 || G < 0 || G > (int64_t)INT32_MAX || n > (int64_t)INT32_MAX) return MJX_EINVAL;
    if (G == 0) return MJX_OK;
    if (!bits || !s || !counts || !done || !t_stop || !conf || !live) return MJX_EINVAL;
    hprb::k_hpr_batch_record<<<(unsigned)G, hprb::kThreads, 0, as_stream(stream)>>>(
        (const u64*)bits, s, n, inst, t_base, t_add, TT, counts, done, t_stop, conf, live);
    MJX_LAUNCH_CHECK("k_hpr_batch_record");
    return MJX_OK;
}
