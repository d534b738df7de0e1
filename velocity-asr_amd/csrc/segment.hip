// Long-form segmentation on the device: block energies, the greedy cut plan and the gather of the
// planned segments into the zero-padded batch the front end reads.  The rule is the one
// velocity_asr.audio.plan_segments_host states in numpy; every sum here has that rule's order, so the
// cuts are the host's exactly.
//
// Arithmetic contract.  A block is kSegBlk = 320 samples (one token row: two mel hops).
//   E[k]     = sum_{i = 0 .. 319, ascending} (double)x[320 k + i] * (double)x[320 k + i], ONE fp64
//              chain from +0.  A product of two fp32 values is exact in fp64, so fma(x, x, acc) and
//              acc + x * x round alike and the chain is the only rounding.
//   score(c) = E[c - W/2] + ... + E[c + W/2 - 1], ascending into one fp64 that starts at 0, recomputed
//              for every candidate (a sliding sum would round in another order); NaN counts as +inf.
//   plan     : p = 0; while n - 320 p > M: c* = the candidate of [p + mB, min(p + MB, nB - mB)] with
//              the smallest (score, c), lexicographically; cut at 320 c*; p = c*.
// The lexicographic minimum is associative and commutative, so the workgroup may reduce it in any order.
#include <climits>
#include <cmath>

#include "vasr_internal.h"

namespace vasr {
namespace {

constexpr int kSegBlk = 320;
constexpr int kSegTile = 32;             // blocks per workgroup of the energy kernel
constexpr int kSegPitch = kSegBlk + 1;   // LDS row pitch: lanes 0..31 at one column hit 32 banks, not one
constexpr int kSegThreads = 256;
constexpr int kSegVec = kSegBlk / 4;     // float4 per block
constexpr int kGatherTile = 4096;        // outputs per workgroup of the gather

__device__ __forceinline__ int seg_samples(const int32_t* __restrict__ samples, int b, int S) {
    if (!samples) return S;
    const int n = samples[b];
    return n < 0 ? 0 : (n > S ? S : n);  // never read outside the row
}

// grid (tiles of kSegTile blocks, B).  VEC: rows are 16-byte aligned (x and ld_x), so a block is 80 float4.
template <bool VEC>
__global__ __launch_bounds__(kSegThreads) void block_energy_kernel(const float* __restrict__ x, int64_t ld_x, int S,
                                                                   const int32_t* __restrict__ samples,
                                                                   double* __restrict__ E, int64_t ld_e) {
    __shared__ __attribute__((aligned(16))) float tile[kSegTile * kSegPitch];
    const int b = blockIdx.y;
    const int nb_row = S / kSegBlk;                                  // blocks of E's row
    const int nB = seg_samples(samples, b, S) / kSegBlk;             // full blocks of the recording
    const int k0 = blockIdx.x * kSegTile;                            // first block of the tile
    const int kt = min(kSegTile, nb_row - k0);                       // blocks of the tile in the row
    const int kv = max(0, min(kt, nB - k0));                         // ... that are full blocks of the recording
    const float* xt = x + (int64_t)b * ld_x + (int64_t)k0 * kSegBlk;
    if (VEC) {
        const float4* x4 = reinterpret_cast<const float4*>(xt);
        for (int i = threadIdx.x; i < kv * kSegVec; i += kSegThreads) {
            const float4 v = x4[i];
            const int r = i / kSegVec, c = (i - r * kSegVec) * 4;
            float* t = tile + r * kSegPitch + c;
            t[0] = v.x, t[1] = v.y, t[2] = v.z, t[3] = v.w;
        }
    } else {
        for (int i = threadIdx.x; i < kv * kSegBlk; i += kSegThreads) {
            const int r = i / kSegBlk;
            tile[r * kSegPitch + (i - r * kSegBlk)] = xt[i];
        }
    }
    __syncthreads();
    if (threadIdx.x < kt) {
        double acc = 0.0;
        if (threadIdx.x < kv) {
            const float* t = tile + threadIdx.x * kSegPitch;
#pragma unroll 8
            for (int i = 0; i < kSegBlk; ++i) {
                const double v = (double)t[i];
                acc = fma(v, v, acc);
            }
        }
        E[(int64_t)b * ld_e + k0 + threadIdx.x] = acc;  // blocks past nB: 0
    }
}

struct Cand {
    double s;
    int c;
};
__device__ __forceinline__ bool cand_less(double s, int c, const Cand& o) { return s < o.s || (s == o.s && c < o.c); }

// One workgroup per recording; the loop over cuts is sequential, its trip count bounded by max_cuts.
__global__ __launch_bounds__(kSegThreads) void segment_plan_kernel(const double* __restrict__ E, int64_t ld_e, int S,
                                                                   const int32_t* __restrict__ samples, int64_t M,
                                                                   int mB, int MB, int W, int64_t* __restrict__ cuts,
                                                                   int64_t ld_cuts, int max_cuts,
                                                                   int32_t* __restrict__ n_cuts) {
    __shared__ double ws[kSegThreads / kWave];
    __shared__ int wc[kSegThreads / kWave];
    const int b = blockIdx.x;
    const int64_t n = seg_samples(samples, b, S);
    const int nB = (int)(n / kSegBlk);
    const double* Eb = E + (int64_t)b * ld_e;
    const int h = W / 2;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int p = 0, nc = 0;
    while (n - (int64_t)p * kSegBlk > M && nc < max_cuts) {
        const int lo = p + mB, hi = min(p + MB, nB - mB);
        Cand best{INFINITY, INT_MAX};
        for (int c = lo + (int)threadIdx.x; c <= hi; c += kSegThreads) {
            double s = 0.0;
            for (int k = c - h; k < c + h; ++k) s += Eb[k];
            if (s != s) s = INFINITY;
            if (cand_less(s, c, best)) best = Cand{s, c};
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double s2 = __shfl_xor(best.s, o, kWave);
            const int c2 = __shfl_xor(best.c, o, kWave);
            if (cand_less(s2, c2, best)) best = Cand{s2, c2};
        }
        __syncthreads();  // the previous round's reads of ws / wc are done
        if (lane == 0) ws[wave] = best.s, wc[wave] = best.c;
        __syncthreads();
        best = Cand{ws[0], wc[0]};
#pragma unroll
        for (int w = 1; w < kSegThreads / kWave; ++w)
            if (cand_less(ws[w], wc[w], best)) best = Cand{ws[w], wc[w]};
        if (best.c == INT_MAX) break;  // empty candidate range: parameters the host checks rule this out
        if (threadIdx.x == 0) cuts[(int64_t)b * ld_cuts + nc] = (int64_t)best.c * kSegBlk;
        p = best.c;
        ++nc;
    }
    if (threadIdx.x == 0) n_cuts[b] = nc;
}

// grid (tiles of kGatherTile outputs, segments).  A table row that does not lie inside its recording
// or its output row is written as zeros: a bad table cannot make the kernel read or write out of bounds.
__global__ __launch_bounds__(kSegThreads) void segment_gather_kernel(const float* __restrict__ x, int64_t ld_x, int B, int S,
                                                                     const int64_t* __restrict__ table,
                                                                     float* __restrict__ y, int64_t ld_y, int S_seg) {
    const int g = blockIdx.y;
    const int64_t rec = table[3 * (int64_t)g], start = table[3 * (int64_t)g + 1];
    int64_t len = table[3 * (int64_t)g + 2];
    if (rec < 0 || rec >= B || start < 0 || len < 0 || len > S_seg || start > S || len > S - start) len = 0;
    const float* xs = x + rec * (len ? ld_x : 0) + (len ? start : 0);
    float* yr = y + (int64_t)g * ld_y;
    const int o0 = blockIdx.x * kGatherTile;
    const int o1 = min(o0 + kGatherTile, S_seg);
    const bool vec = ((reinterpret_cast<uintptr_t>(xs) | reinterpret_cast<uintptr_t>(yr)) & 15) == 0;
    if (vec) {  // workgroup-uniform: both rows 16-byte aligned (o0 is a multiple of 4)
        const int q1 = o0 + (o1 - o0) / 4 * 4;
        for (int o = o0 + 4 * (int)threadIdx.x; o < q1; o += 4 * kSegThreads) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (o + 4 <= len) {
                v = *reinterpret_cast<const float4*>(xs + o);
            } else if (o < len) {
                v.x = xs[o];
                if (o + 1 < len) v.y = xs[o + 1];
                if (o + 2 < len) v.z = xs[o + 2];
            }
            *reinterpret_cast<float4*>(yr + o) = v;
        }
        for (int o = q1 + (int)threadIdx.x; o < o1; o += kSegThreads) yr[o] = o < len ? xs[o] : 0.f;
    } else {
        for (int o = o0 + (int)threadIdx.x; o < o1; o += kSegThreads) yr[o] = o < len ? xs[o] : 0.f;
    }
}

}  // namespace
}  // namespace vasr

VASR_API int vasr_segment_block(void) { return vasr::kSegBlk; }

VASR_API int vasr_segment_tile_blocks(void) { return vasr::kSegTile; }

VASR_API int64_t vasr_segment_max_cuts(int64_t n, int64_t min_samples) {
    using namespace vasr;
    if (n < 0 || min_samples < 1) return -1;
    const int64_t mB = (min_samples + kSegBlk - 1) / kSegBlk;
    return (n / kSegBlk) / mB;
}

VASR_API int vasr_block_energy_f64(const float* x, int64_t ld_x, int B, int S, const int32_t* samples, double* E,
                                   int64_t ld_e, void* stream) {
    using namespace vasr;
    VASR_CHECK_ARG(x && E, "vasr_block_energy_f64: null pointer");
    VASR_CHECK_ARG(B > 0 && S > 0, "vasr_block_energy_f64: bad sizes");
    VASR_CHECK_ARG(B <= 65535, "vasr_block_energy_f64: at most 65535 recordings per launch, got %d", B);
    VASR_CHECK_ARG(ld_x >= S, "vasr_block_energy_f64: ld_x %lld < %d samples", (long long)ld_x, S);
    const int nb = S / kSegBlk;
    VASR_CHECK_ARG(ld_e >= nb, "vasr_block_energy_f64: ld_e %lld < %d blocks", (long long)ld_e, nb);
    if (nb == 0) return VASR_OK;  // no full block: E has no entries
    const dim3 grid((unsigned)((nb + kSegTile - 1) / kSegTile), (unsigned)B);
    hipStream_t s = as_stream(stream);
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0 && ld_x % 4 == 0)
        hipLaunchKernelGGL(block_energy_kernel<true>, grid, dim3(kSegThreads), 0, s, x, ld_x, S, samples, E, ld_e);
    else
        hipLaunchKernelGGL(block_energy_kernel<false>, grid, dim3(kSegThreads), 0, s, x, ld_x, S, samples, E, ld_e);
    return launch_status("vasr_block_energy_f64");
}

VASR_API int vasr_segment_plan(const double* E, int64_t ld_e, int B, int S, const int32_t* samples, int64_t max_samples,
                               int64_t min_samples, int window_blocks, int64_t* cuts, int64_t ld_cuts, int max_cuts,
                               int32_t* n_cuts, void* stream) {
    using namespace vasr;
    VASR_CHECK_ARG(E && cuts && n_cuts, "vasr_segment_plan: null pointer");
    VASR_CHECK_ARG(B > 0 && S > 0, "vasr_segment_plan: bad sizes");
    VASR_CHECK_ARG(B <= 65535, "vasr_segment_plan: at most 65535 recordings per launch, got %d", B);
    VASR_CHECK_ARG(window_blocks >= 2 && window_blocks % 2 == 0,
                   "vasr_segment_plan: window_blocks must be even and at least 2, got %d", window_blocks);
    VASR_CHECK_ARG(min_samples >= 1 && max_samples >= 1, "vasr_segment_plan: bad segment bounds");
    const int64_t mB = (min_samples + kSegBlk - 1) / kSegBlk, MB = max_samples / kSegBlk;
    VASR_CHECK_ARG(mB >= window_blocks / 2, "vasr_segment_plan: min_samples %lld is under half the window of %d blocks",
                   (long long)min_samples, window_blocks);
    VASR_CHECK_ARG(MB >= 2 * mB, "vasr_segment_plan: max_samples %lld holds %lld blocks, fewer than twice the %lld of "
                   "min_samples %lld", (long long)max_samples, (long long)MB, (long long)mB, (long long)min_samples);
    VASR_CHECK_ARG(ld_e >= S / kSegBlk, "vasr_segment_plan: ld_e %lld < %d blocks", (long long)ld_e, S / kSegBlk);
    const int64_t need = (S / kSegBlk) / mB;
    VASR_CHECK_ARG(max_cuts >= need && max_cuts >= 1 && ld_cuts >= max_cuts,
                   "vasr_segment_plan: a cuts table of %d columns (ld %lld) is too narrow for %d samples: %lld needed",
                   max_cuts, (long long)ld_cuts, S, (long long)(need > 1 ? need : 1));
    // S is an int, so the block counts fit one too
    const int mBi = (int)mB, MBi = (int)(MB > S / kSegBlk + 1 ? S / kSegBlk + 1 : MB);
    hipLaunchKernelGGL(segment_plan_kernel, dim3((unsigned)B), dim3(kSegThreads), 0, as_stream(stream), E, ld_e, S, samples,
                       max_samples, mBi, MBi, window_blocks, cuts, ld_cuts, max_cuts, n_cuts);
    return launch_status("vasr_segment_plan");
}

VASR_API int vasr_segment_gather_f32(const float* x, int64_t ld_x, int B, int S, const int64_t* table, int n_seg, float* y,
                                     int64_t ld_y, int S_seg, void* stream) {
    using namespace vasr;
    VASR_CHECK_ARG(x && table && y, "vasr_segment_gather_f32: null pointer");
    VASR_CHECK_ARG(B > 0 && S > 0 && n_seg > 0 && S_seg > 0, "vasr_segment_gather_f32: bad sizes");
    VASR_CHECK_ARG(B <= 65535, "vasr_segment_gather_f32: at most 65535 recordings per launch, got %d", B);
    VASR_CHECK_ARG(n_seg <= 65535, "vasr_segment_gather_f32: at most 65535 segments per launch, got %d", n_seg);
    VASR_CHECK_ARG(ld_x >= S, "vasr_segment_gather_f32: ld_x %lld < %d samples", (long long)ld_x, S);
    VASR_CHECK_ARG(ld_y >= S_seg, "vasr_segment_gather_f32: ld_y %lld < %d samples", (long long)ld_y, S_seg);
    const dim3 grid((unsigned)((S_seg + kGatherTile - 1) / kGatherTile), (unsigned)n_seg);
    hipLaunchKernelGGL(segment_gather_kernel, grid, dim3(kSegThreads), 0, as_stream(stream), x, ld_x, B, S, table, y, ld_y,
                       S_seg);
    return launch_status("vasr_segment_gather_f32");
}
