// Device sample-rate conversion with a fused channel downmix: vasr_resample_mix_f32, the device
// form of vasr_resample_f32 (audio_io.cpp) for a zero-padded batch of clips.
//
// Arithmetic contract.  m[i] = (x_0[i] + ... + x_{C-1}[i]) / C in fp32 (ascending channels, IEEE
// division), 0 outside [0, samples[b]).  Output o = fr * nw + j of clip b is
//     y[o] = (float) sum_{k = 0 .. klen-1, ascending} (double)taps[j][k] * (double)m[fr * orig - width + k]
// as ONE fp64 chain.  A product of two fp32 values is exact in fp64, so fma(tap, x, acc) and
// acc + tap * x round alike, and a zero-padded tap adds +-0 to a chain that started at +0: the
// result is the host resampler's, bit for bit (it clamps the tap range instead of padding).
//
// Tiling.  A frame is `orig` inputs and `nw` outputs.  A workgroup (16 waves) owns F consecutive
// frames of one clip: it downmixes the span [f0 * orig - width, (f0 + F) * orig + width) once into
// LDS and runs every chain from there.  The span is stored by phase: input i of the span sits at
// (i % orig) * L + i / orig, so the 64 lanes of a wave, which hold 64 consecutive frames and read
// inputs `orig` apart, read 64 consecutive dwords whatever orig is (stride orig itself would be a
// 2-way bank conflict at orig 2 or 6 and 4-way at 12).  A wave takes units of R tap rows x 64 Q
// frames: the R rows are wave-uniform, so their taps come through the scalar cache straight from
// the row-major table (no transposed copy; 304 KB at 44.1 -> 16 kHz never has to fit in LDS), each
// LDS read feeds R chains and each tap Q chains: R * Q = 4 independent fp64 chains per thread.
#include <mutex>

#include "vasr_internal.h"

namespace vasr {
namespace {

constexpr int kRsThreads = 1024;
constexpr int kRsWaves = kRsThreads / kWave;
constexpr size_t kRsLdsBudget = 144 * 1024;  // of the CU's 160 KiB
constexpr int kRsCopyTile = 1024;            // outputs per workgroup when the rates are equal

struct RsTile {
    int R, Q;     // tap rows and 64-frame blocks per thread
    int F;        // frames per workgroup, a multiple of 64 * Q
    int L;        // dwords per phase row of the LDS image (odd)
    size_t lds;   // bytes
};

// The tile of a geometry; false when even the smallest one does not fit in LDS.
bool rs_tile(int orig, int nw, int width, RsTile& t) {
    t.R = nw % 4 == 0 ? 4 : (nw % 2 == 0 ? 2 : 1);
    t.Q = 4 / t.R;
    const int64_t klen = 2 * (int64_t)width + orig;
    const int rowgroups = nw / t.R;
    // enough 64 * Q frame blocks to give every wave a unit, halved until the span fits
    for (int fb = (kRsWaves + rowgroups - 1) / rowgroups; fb >= 1; fb = fb == 1 ? 0 : (fb + 1) / 2) {
        const int64_t F = (int64_t)64 * t.Q * fb;
        const int64_t L = (F + (klen - 1) / orig + 1) | 1;
        const int64_t lds = (int64_t)orig * L * (int64_t)sizeof(float);
        if (lds <= (int64_t)kRsLdsBudget && F * nw <= (int64_t)1 << 30) {
            t.F = (int)F;
            t.L = (int)L;
            t.lds = (size_t)lds;
            return true;
        }
    }
    return false;
}

__device__ __forceinline__ float downmix(const float* __restrict__ xb, int64_t ld_chan, int C, int64_t g) {
    float s = xb[g];
    for (int c = 1; c < C; ++c) s += xb[c * ld_chan + g];
    return s / (float)C;
}

__device__ __forceinline__ int clip_samples(const int32_t* __restrict__ samples, int b, int S_in) {
    if (!samples) return S_in;
    const int n = samples[b];
    return n < 1 ? 1 : (n > S_in ? S_in : n);  // the contract is [1, S_in]; never read outside the clip
}

// equal rates: downmix and copy
__global__ __launch_bounds__(256) void downmix_copy_kernel(const float* __restrict__ x, int64_t ld_clip, int64_t ld_chan,
                                                           int C, int S_in, const int32_t* __restrict__ samples,
                                                           float* __restrict__ y, int64_t ld_y, int S_out) {
    const int b = blockIdx.y;
    const int n = clip_samples(samples, b, S_in);
    const float* xb = x + (int64_t)b * ld_clip;
    float* yb = y + (int64_t)b * ld_y;
    const int o0 = blockIdx.x * kRsCopyTile;
    for (int o = o0 + threadIdx.x; o < min(o0 + kRsCopyTile, S_out); o += 256) yb[o] = o < n ? downmix(xb, ld_chan, C, o) : 0.f;
}

template <int R, int Q>
__global__ __launch_bounds__(kRsThreads) void resample_mix_kernel(
    const float* __restrict__ x, int64_t ld_clip, int64_t ld_chan, int C, int S_in, const int32_t* __restrict__ samples,
    const float* __restrict__ taps, int orig, int nw, int width, int F, int L, float* __restrict__ y, int64_t ld_y,
    int S_out) {
    extern __shared__ __attribute__((aligned(16))) float img[];  // [orig][L]: input i at (i % orig) * L + i / orig
    const int b = blockIdx.y;
    const int n = clip_samples(samples, b, S_in);
    const int64_t out_len = ((int64_t)nw * n + orig - 1) / orig;  // vasr_resample_length of the clip
    const int64_t f0 = (int64_t)blockIdx.x * F;                   // first frame of the tile
    const int64_t o0 = f0 * nw;                                   // first output of the tile
    const int64_t tile_out = (int64_t)F * nw;
    float* yb = y + (int64_t)b * ld_y;
    if (o0 >= out_len) {  // wholly past the clip: zero fill
        const int64_t end = min(o0 + tile_out, (int64_t)S_out);
        for (int64_t o = o0 + threadIdx.x; o < end; o += kRsThreads) yb[o] = 0.f;
        return;
    }
    const int klen = 2 * width + orig;
    // frames of the tile that hold outputs of the clip, and the inputs they read
    const int fv = (int)min((int64_t)F, (out_len - o0 + nw - 1) / nw);
    const int span = (fv - 1) * orig + klen;
    const int64_t g0 = f0 * orig - width;  // clip index of span input 0
    const float* xb = x + (int64_t)b * ld_clip;
    for (int i = threadIdx.x; i < span; i += kRsThreads) {
        const int64_t g = g0 + i;
        const int q = i / orig;
        img[(i - q * orig) * L + q] = (g >= 0 && g < n) ? downmix(xb, ld_chan, C, g) : 0.f;
    }
    __syncthreads();

    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int rowgroups = nw / R;
    const int units = rowgroups * (F / (kWave * Q));
    for (int u = wave; u < units; u += kRsWaves) {
        const int fb = u / rowgroups;
        const int j0 = (u - fb * rowgroups) * R;  // first tap row of the unit
        const int fl = fb * (kWave * Q);          // first frame of the unit, within the tile
        if (fl >= fv) break;                      // later units hold later frames or the same ones
        double acc[R][Q];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int q = 0; q < Q; ++q) acc[r][q] = 0.0;
        const float* __restrict__ tj = taps + (int64_t)j0 * klen;
        const float* xl = img + fl + lane;
        // k = kq * orig + ph ascending: span input fr * orig + k sits at off = ph * L + kq past fr
        // (ph, off: wave-uniform scalars)
        const int wrap = orig * L - 1;
        int ph = 0, off = 0;
#pragma unroll 4
        for (int k = 0; k < klen; ++k) {
            double xv[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) xv[q] = (double)xl[off + q * kWave];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double t = (double)tj[r * klen + k];
#pragma unroll
                for (int q = 0; q < Q; ++q) acc[r][q] = fma(t, xv[q], acc[r][q]);
            }
            off += L;
            if (++ph == orig) {
                ph = 0;
                off -= wrap;
            }
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int64_t o = (f0 + fl + q * kWave + lane) * nw + j0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (o + r < out_len) yb[o + r] = (float)acc[r][q];
                else if (o + r < S_out) yb[o + r] = 0.f;
            }
        }
    }
    // frames of the tile past the clip's last one: zero fill
    const int64_t z0 = o0 + (int64_t)((fv + kWave * Q - 1) / (kWave * Q)) * (kWave * Q) * nw;
    const int64_t z1 = min(o0 + tile_out, (int64_t)S_out);
    for (int64_t o = z0 + threadIdx.x; o < z1; o += kRsThreads) yb[o] = 0.f;
}

template <int R, int Q>
int launch_resample(const float* x, int64_t ld_clip, int64_t ld_chan, int B, int C, int S_in, const int32_t* samples,
                    const float* taps, int orig, int nw, int width, const RsTile& t, float* y, int64_t ld_y, int S_out,
                    hipStream_t s) {
    static std::once_flag once;
    static hipError_t attr = hipSuccess;
    std::call_once(once, [] {  // raise the dynamic LDS limit once per instance
        attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&resample_mix_kernel<R, Q>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRsLdsBudget);
    });
    if (attr != hipSuccess) {
        set_error("vasr_resample_mix_f32: %s", hipGetErrorString(attr));
        return (int)attr;
    }
    const int64_t tile_out = (int64_t)t.F * nw;
    const dim3 grid((unsigned)((S_out + tile_out - 1) / tile_out), (unsigned)B);
    hipLaunchKernelGGL((resample_mix_kernel<R, Q>), grid, dim3(kRsThreads), t.lds, s, x, ld_clip, ld_chan, C, S_in, samples,
                       taps, orig, nw, width, t.F, t.L, y, ld_y, S_out);
    return launch_status("vasr_resample_mix_f32");
}

}  // namespace
}  // namespace vasr

VASR_API int vasr_resample_tile_outputs(int orig, int nw) {
    using namespace vasr;
    if (orig <= 0 || nw <= 0) return 0;
    if (orig == nw) return kRsCopyTile;
    // width as vasr_resample_plan derives it from the reduced pair
    const double base = (double)(orig < nw ? orig : nw) * 0.99;
    const int width = (int)ceil(6.0 * orig / base);
    RsTile t;
    return rs_tile(orig, nw, width, t) ? t.F * nw : 0;
}

VASR_API int vasr_resample_mix_f32(const float* x, int64_t ld_clip, int64_t ld_chan, int B, int C, int S_in,
                                   const int32_t* samples, const float* taps, int orig, int nw, int width, float* y,
                                   int64_t ld_y, int S_out, void* stream) {
    using namespace vasr;
    VASR_CHECK_ARG(x && y, "vasr_resample_mix_f32: null pointer");
    VASR_CHECK_ARG(B > 0 && S_in > 0 && orig > 0 && nw > 0 && width >= 0, "vasr_resample_mix_f32: bad sizes");
    VASR_CHECK_ARG(B <= 65535, "vasr_resample_mix_f32: at most 65535 clips per launch, got %d", B);
    VASR_CHECK_ARG(C >= 1 && C <= 8, "vasr_resample_mix_f32: %d channels, 1 to 8 supported", C);
    VASR_CHECK_ARG(ld_chan >= S_in || C == 1, "vasr_resample_mix_f32: ld_chan %lld < %d samples", (long long)ld_chan, S_in);
    VASR_CHECK_ARG(ld_clip >= S_in, "vasr_resample_mix_f32: ld_clip %lld < %d samples", (long long)ld_clip, S_in);
    VASR_CHECK_ARG(ld_y >= S_out, "vasr_resample_mix_f32: ld_y %lld < %d outputs", (long long)ld_y, S_out);
    const int64_t need = ((int64_t)nw * S_in + orig - 1) / orig;
    VASR_CHECK_ARG(S_out >= need, "vasr_resample_mix_f32: S_out %d < %lld outputs of %d samples", S_out, (long long)need,
                   S_in);
    hipStream_t s = as_stream(stream);
    if (orig == nw) {
        const dim3 grid((unsigned)((S_out + kRsCopyTile - 1) / kRsCopyTile), (unsigned)B);
        hipLaunchKernelGGL(downmix_copy_kernel, grid, dim3(256), 0, s, x, ld_clip, ld_chan, C, S_in, samples, y, ld_y, S_out);
        return launch_status("vasr_resample_mix_f32");
    }
    VASR_CHECK_ARG(taps, "vasr_resample_mix_f32: null pointer");
    RsTile t;
    VASR_CHECK_ARG(rs_tile(orig, nw, width, t),
                   "vasr_resample_mix_f32: %d -> %d with width %d: the input span of 64 frames does not fit in LDS "
                   "(%zu bytes)", orig, nw, width, kRsLdsBudget);
    if (t.R == 4) return launch_resample<4, 1>(x, ld_clip, ld_chan, B, C, S_in, samples, taps, orig, nw, width, t, y, ld_y, S_out, s);
    if (t.R == 2) return launch_resample<2, 2>(x, ld_clip, ld_chan, B, C, S_in, samples, taps, orig, nw, width, t, y, ld_y, S_out, s);
    return launch_resample<1, 4>(x, ld_clip, ld_chan, B, C, S_in, samples, taps, orig, nw, width, t, y, ld_y, S_out, s);
}
