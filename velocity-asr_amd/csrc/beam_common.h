// Shared by beam.hip and beam_shortlist.hip: the candidate record of the prefix beam search, its
// order (the reference's stable sort: score descending, insertion position ascending) and the
// 256-thread block reductions.  block_reduce_f fixes the order in which a row's exp-sum is formed
// (256 strided partials, xor butterfly, then the four waves left to right); both files' log-softmax
// go through it, which is what makes their log-probabilities the same bits.
#pragma once
#include "vasr_internal.h"

namespace vasr {
namespace {

constexpr int kBeamThreads = 256;
constexpr int kMaxBeam = 32;

struct Cand {
    double s;
    long long idx;  // insertion position; -1 = none
};

__device__ __forceinline__ bool better(const Cand& a, const Cand& b) {  // a before b in the sorted order
    if (a.idx < 0) return false;
    if (b.idx < 0) return true;
    return a.s > b.s || (a.s == b.s && a.idx < b.idx);
}

__device__ Cand block_best(Cand c, Cand* red) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Cand d;
        d.s = __shfl_xor(c.s, o, 64);
        d.idx = __shfl_xor(c.idx, o, 64);
        if (better(d, c)) c = d;
    }
    if ((tid & 63) == 0) red[tid >> 6] = c;
    __syncthreads();
    Cand best = red[0];
    for (int w = 1; w < kBeamThreads / 64; ++w)
        if (better(red[w], best)) best = red[w];
    __syncthreads();
    return best;
}

__device__ float block_reduce_f(float v, float* red, bool is_max) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float u = __shfl_xor(v, o, 64);
        v = is_max ? fmaxf(v, u) : v + u;
    }
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < kBeamThreads / 64; ++w) r = is_max ? fmaxf(r, red[w]) : r + red[w];
    __syncthreads();
    return r;
}

}  // namespace
}  // namespace vasr
