// CTC loss, its gradient with respect to the logits, and CTC forced alignment against a known
// transcript (reference velocity_asr/training.py:47-104: F.log_softmax + nn.CTCLoss; the Viterbi
// form of the same lattice is the forced alignment that belongs beside decode.py:74-125).
//
// Two stages forward (the backward's are described above its kernels, at the end of the file).
//   1. ctc_emissions_kernel: the only part that touches the (B, L, V) logits.  One wave per
//      logit row reads the row once (16-byte loads where the row is 16-byte aligned, scalar
//      loads otherwise -- the element -> lane assignment and the arithmetic are the same in
//      both, so the result does not depend on the alignment), keeps a running (max, sum of
//      exp) per lane, combines the 64 lanes, and gathers the blank's and the target tokens'
//      log-probabilities into the compact emis (B, L, Smax + 1).  No (B, L, V) log-softmax
//      tensor exists.  The row loop is branch-free and unrolled by 4, so a 1000-wide row's four
//      loads per lane are in flight together (18.9 us against 21.0 us rolled at 32 x 501 x 1000).
//   2. ctc_lattice_kernel: one workgroup per utterance walks the frames over the extended
//      label sequence (S' = 2 tlen + 1 states, blanks interleaved).  Lane l keeps the R
//      consecutive states l R .. l R + R - 1 in registers; R is even, so a lane's even slots
//      are blanks and the only value it needs from outside is its left neighbour's last state,
//      fetched with one DPP wave shift per frame.  One wave holds 64 R states; a longer
//      target takes several waves, which hand that one boundary value over through LDS with one
//      barrier per frame.  Emissions of the next eight frames (four at R = 8) are loaded while the
//      current ones are consumed (the recursion is a serial chain per frame; an exposed load per frame
//      would dominate it).  LOSS: log-sum-exp of the sources (fp32, maximum subtracted, -inf
//      stays -inf) on the hardware exp2 / log2 (~1 ulp each; the rounding of alpha + emission at
//      |alpha| in the hundreds to thousands is what sets the accuracy).  ALIGN:
//      maximum of the sources with a 2-bit back-pointer per (t, s) in the caller's workspace, then
//      a backtrack by thread 0.
#include "vasr_internal.h"

namespace vasr {
namespace {

constexpr int kMaxFrames = 8192;
constexpr int kMaxTarget = 2048;
constexpr int kEmisWaves = 4;   // logit rows per workgroup of ctc_emissions_kernel

// ------------------------------------------------------------------ emissions

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
    return v;
}

// fold four more elements into a running (maximum m, sum s of exp(x - m))
__device__ __forceinline__ void lse_fold(float& m, float& s, float x0, float x1, float x2, float x3) {
    const float mn = fmaxf(fmaxf(m, fmaxf(x0, x1)), fmaxf(x2, x3));
    const float ms = mn == -INFINITY ? 0.f : mn;  // all -inf so far: no inf - inf
    s = s * fast_exp(m - ms) + ((fast_exp(x0 - ms) + fast_exp(x1 - ms)) + (fast_exp(x2 - ms) + fast_exp(x3 - ms)));
    m = mn;
}

// Log-sum-exp of one logit row by one wave: returns lse of the row shifted by Ms (the row's
// maximum, 0 if every element is -inf), so log_softmax(x) = (x - Ms) - lse.  `wide`: the row is
// 16-byte aligned.  Shared by the emissions pass and the gradient pass, which must agree bitwise.
__device__ __forceinline__ float row_lse(const float* __restrict__ row, int V, int lane, bool wide, float& Ms) {
    // running maximum m and sum s of exp(x - m) over this lane's elements: group g = 64 c + lane
    // of 4 consecutive elements, c = 0, 1, ...  The loops are branch-free (a lane past the last
    // whole group loads that group again and folds in -inf, which changes nothing), so the
    // unrolled loads of a row are all in flight together.
    float m = -INFINITY, s = 0.f;
    const int nfull = V >> 2, nch = (nfull + kWave - 1) / kWave;
    if (wide) {
        const float4* row4 = reinterpret_cast<const float4*>(row);
#pragma unroll 4
        for (int c = 0; c < nch; ++c) {
            const int g = c * kWave + lane;
            const float4 q = row4[min(g, nfull - 1)];
            const bool in = g < nfull;
            lse_fold(m, s, in ? q.x : -INFINITY, in ? q.y : -INFINITY, in ? q.z : -INFINITY, in ? q.w : -INFINITY);
        }
    } else {
#pragma unroll 4
        for (int c = 0; c < nch; ++c) {
            const int g = c * kWave + lane;
            const float* p = row + 4 * min(g, nfull - 1);
            const float x0 = p[0], x1 = p[1], x2 = p[2], x3 = p[3];
            const bool in = g < nfull;
            lse_fold(m, s, in ? x0 : -INFINITY, in ? x1 : -INFINITY, in ? x2 : -INFINITY, in ? x3 : -INFINITY);
        }
    }
    if ((V & 3) && lane == (nfull & (kWave - 1))) {  // the last, partial group: after that lane's whole ones
        const float* p = row + 4 * nfull;
        lse_fold(m, s, p[0], (V & 3) > 1 ? p[1] : -INFINITY, (V & 3) > 2 ? p[2] : -INFINITY, -INFINITY);
    }
    const float M = wave_max(m);
    Ms = M == -INFINITY ? 0.f : M;
    return logf(wave_sum(s * fast_exp(m - Ms)));  // of the row shifted by M
}

__global__ __launch_bounds__(kEmisWaves* kWave) void ctc_emissions_kernel(
    const float* __restrict__ logits, int64_t ld_row, int64_t ld_utt, int B, int L, int V,
    const int32_t* __restrict__ targets, int Smax, const int32_t* __restrict__ frames,
    const int32_t* __restrict__ tlen, int blank, float* __restrict__ emis) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = (int64_t)blockIdx.x * kEmisWaves + (threadIdx.x >> 6);
    if (r >= (int64_t)B * L) return;
    const int b = (int)(r / L), t = (int)(r - (int64_t)b * L);
    if (t >= min(max(frames[b], 0), L)) return;  // padding rows are never read
    const float* row = logits + (int64_t)b * ld_utt + (int64_t)t * ld_row;
    const bool wide = (reinterpret_cast<uintptr_t>(row) & 15) == 0;

    float Ms;
    const float lse = row_lse(row, V, lane, wide, Ms);

    float* e = emis + r * (int64_t)(Smax + 1);
    const int n = min(max(tlen[b], 0), Smax);
    const int32_t* tg = targets + (int64_t)b * Smax;
    for (int j = lane; j <= n; j += kWave) {
        const int tok = j == 0 ? blank : tg[j - 1];
        // a token id outside [0, V) is not read: its emission is -inf
        e[j] = (tok >= 0 && tok < V) ? (row[tok] - Ms) - lse : -INFINITY;
    }
}

// ------------------------------------------------------------------ lattice

// v of lane - 1; lane 0 of the wave gets `first`.  (DPP wave_shr:1, bound_ctrl off: the lane
// without a source keeps the old value.)
__device__ __forceinline__ float from_left_lane(float v, float first) {
    return __int_as_float(
        __builtin_amdgcn_update_dpp(__float_as_int(first), __float_as_int(v), 0x138, 0xF, 0xF, false));
}

__device__ __forceinline__ float fast_log(float x) { return __builtin_amdgcn_logf(x) * 0.69314718055994531f; }

// log(exp(a) + exp(b)) and log(exp(a) + exp(b) + exp(c)); -inf if every argument is
__device__ __forceinline__ float lse2(float a, float b) {
    const float m = fmaxf(a, b);
    const float r = m + fast_log(1.0f + fast_exp(fminf(a, b) - m));
    return m == -INFINITY ? m : r;
}
__device__ __forceinline__ float lse3(float a, float b, float c) {
    const float m = fmaxf(a, fmaxf(b, c));
    const float r = m + fast_log((fast_exp(a - m) + fast_exp(b - m)) + fast_exp(c - m));
    return m == -INFINITY ? m : r;
}

// R states per lane (even), ALIGN: Viterbi with back-pointers instead of the sum.  STORE (loss
// only): every frame's alpha is also written to alpha (B, L, 2 Smax + 1), states s < S' of rows
// t < T; the arithmetic is untouched, so the loss is bitwise the one without the store.
// blockDim.x = 64 * waves with 64 * waves * R >= 2 * Smax + 1.
template <int R, bool ALIGN, bool STORE>
__global__ __launch_bounds__(640) void ctc_lattice_kernel(
    const float* __restrict__ emis, int L, int Smax, const int32_t* __restrict__ targets,
    const int32_t* __restrict__ frames, const int32_t* __restrict__ tlen, float* __restrict__ out,
    uint8_t* __restrict__ bp, int bp_row, int32_t* __restrict__ frame_state, int32_t* __restrict__ out_start,
    int32_t* __restrict__ out_end, float* __restrict__ alpha) {
    static_assert(!(ALIGN && STORE), "alpha is stored by the loss form only");
    constexpr int H = R / 2;  // labels per lane
    constexpr int kFrameGroup = R == 8 ? 4 : 8;  // frames whose emissions are in flight together (registers)
    __shared__ float edge[2][16];
    __shared__ float fin[2];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int nwaves = blockDim.x >> 6;
    const int T = min(max(frames[b], 0), L);
    const int n = min(max(tlen[b], 0), Smax);
    const int S = 2 * n + 1;
    const int E = Smax + 1;
    const float* e = emis + (int64_t)b * L * E;
    const int32_t* tg = targets + (int64_t)b * Smax;
    const int s0 = tid * R;  // first state of this lane
    const int j0 = tid * H;  // label of its first odd state

    // label j may be entered from label j - 1 directly (no blank between) iff they differ
    bool skip[H], live[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int j = j0 + h;
        live[h] = j < n;
        skip[h] = live[h] && j >= 1 && tg[j] != tg[j - 1];
    }
    if (tid == 0) fin[0] = fin[1] = -INFINITY;
    if (ALIGN) {
        for (int t = tid; t < L; t += blockDim.x) frame_state[(int64_t)b * L + t] = -1;
        for (int j = tid; j < Smax; j += blockDim.x) out_start[(int64_t)b * Smax + j] = out_end[(int64_t)b * Smax + j] = -1;
    }

    // frame -1: all the mass in state 0, so frame 0 comes out of the same recursion
    float a[R];
#pragma unroll
    for (int k = 0; k < R; ++k) a[k] = (s0 + k == 0) ? 0.f : -INFINITY;

    // emissions of a group of frames: the blank's and this lane's labels'
    float eb[2][kFrameGroup], el[2][kFrameGroup][H];
    auto fetch = [&](int buf, int t0) {
#pragma unroll
        for (int g = 0; g < kFrameGroup; ++g) {
            const int t = t0 + g;
            const float* et = e + (int64_t)t * E;
            eb[buf][g] = t < T ? et[0] : 0.f;
#pragma unroll
            for (int h = 0; h < H; ++h) el[buf][g][h] = (t < T && live[h]) ? et[1 + j0 + h] : -INFINITY;
        }
    };
    auto step = [&](int t, float ebt, const float* elt) {
        float first = -INFINITY;
        if (nwaves > 1) {  // uniform per launch
            if (lane == kWave - 1) edge[t & 1][wave] = a[R - 1];
            __syncthreads();
            if (wave > 0) first = edge[t & 1][wave - 1];
        }
        const float left = from_left_lane(a[R - 1], first);
        float nw[R];
        unsigned bits = 0;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const float c0 = a[k];
            const float c1 = k >= 1 ? a[k - 1] : left;
            const float c2 = (k & 1) && skip[k >> 1] ? (k >= 2 ? a[k - 2] : left) : -INFINITY;
            const float em = (k & 1) ? elt[k >> 1] : ebt;
            if (ALIGN) {
                // ties go to the smaller source state: s, then s - 1, then s - 2
                float best = c0;
                unsigned from = 0;
                if (c1 > best) best = c1, from = 1;
                if (c2 > best) best = c2, from = 2;
                nw[k] = best + em;
                bits |= from << (2 * k);
            } else {
                nw[k] = ((k & 1) ? lse3(c0, c1, c2) : lse2(c0, c1)) + em;  // a blank has two sources
            }
        }
#pragma unroll
        for (int k = 0; k < R; ++k) a[k] = nw[k];
        if (STORE) {
            float* ar = alpha + ((int64_t)b * L + t) * (2 * Smax + 1);
#pragma unroll
            for (int k = 0; k < R; ++k)
                if (s0 + k < S) ar[s0 + k] = a[k];
        }
        if (ALIGN) {  // 4 states per byte: byte s / 4 of row (b, t), bits 2 (s % 4)
            uint8_t* rowp = bp + ((int64_t)b * L + t) * bp_row;
            if (R == 4) {
                if (tid < bp_row) rowp[tid] = (uint8_t)bits;
            } else {
                if (2 * tid < bp_row) reinterpret_cast<uint16_t*>(rowp)[tid] = (uint16_t)bits;
            }
        }
    };

    __syncthreads();  // fin
    fetch(0, 0);
    for (int t0 = 0; t0 < T; t0 += 2 * kFrameGroup) {  // two groups per trip: the buffers stay in registers
        fetch(1, t0 + kFrameGroup);
#pragma unroll
        for (int g = 0; g < kFrameGroup; ++g)
            if (t0 + g < T) step(t0 + g, eb[0][g], el[0][g]);
        fetch(0, t0 + 2 * kFrameGroup);
#pragma unroll
        for (int g = 0; g < kFrameGroup; ++g)
            if (t0 + kFrameGroup + g < T) step(t0 + kFrameGroup + g, eb[1][g], el[1][g]);
    }

    // the last two states
#pragma unroll
    for (int k = 0; k < R; ++k) {
        if (s0 + k == S - 1) fin[0] = a[k];
        if (s0 + k == S - 2) fin[1] = a[k];
    }
    __syncthreads();
    if (tid != 0) return;
    const float hi = fin[0], lo = fin[1];  // states S - 1, S - 2
    if (!ALIGN) {
        const float m = fmaxf(hi, lo);
        out[b] = m == -INFINITY ? INFINITY : -(m + logf(expf(hi - m) + expf(lo - m)));
        return;
    }
    const float score = fmaxf(hi, lo);
    out[b] = score;
    if (score == -INFINITY) return;  // infeasible: everything stays -1
    int s = lo >= hi ? S - 2 : S - 1;  // tie: the smaller state
    int32_t* fs = frame_state + (int64_t)b * L;
    int32_t* st = out_start + (int64_t)b * Smax;
    int32_t* en = out_end + (int64_t)b * Smax;
    int last = -1;
    for (int t = T - 1; t >= 0; --t) {
        if (s & 1) {
            const int j = s >> 1;
            fs[t] = j;
            if (j != last) en[j] = t + 1, last = j;
            st[j] = t;
        }
        const uint8_t w = bp[((int64_t)b * L + t) * bp_row + (s >> 2)];
        s -= (w >> (2 * (s & 3))) & 3;
    }
}

int check_lattice(const char* who, const float* emis, int B, int L, int Smax, const int32_t* targets,
                  const int32_t* frames, const int32_t* tlen) {
    VASR_CHECK_ARG(emis && frames && tlen && (targets || Smax == 0), "%s: null pointer", who);
    VASR_CHECK_ARG(B >= 0 && L >= 1 && L <= kMaxFrames && Smax >= 0, "%s: bad shape B=%d L=%d (1..%d) Smax=%d", who,
                   B, L, kMaxFrames, Smax);
    if (Smax > kMaxTarget) {
        set_error("%s: Smax=%d above the supported %d", who, Smax, kMaxTarget);
        return VASR_EUNSUPPORTED;
    }
    return VASR_OK;
}

// 4 back-pointers per byte, rows padded to whole 32-bit words
inline int bp_row_bytes(int Smax) { return 4 * ((2 * Smax + 1 + 15) / 16); }

}  // namespace
}  // namespace vasr

VASR_API int vasr_ctc_emissions_f32(const float* logits, int64_t ld_row, int64_t ld_utt, int B, int L, int V,
                                    const int32_t* targets, int Smax, const int32_t* frames, const int32_t* tlen,
                                    int blank, float* emis, void* stream) {
    using namespace vasr;
    VASR_CHECK_ARG(logits && frames && tlen && emis && (targets || Smax == 0), "vasr_ctc_emissions_f32: null pointer");
    VASR_CHECK_ARG(B >= 0 && L >= 1 && L <= kMaxFrames && V >= 1 && Smax >= 0 && ld_row >= V,
                   "vasr_ctc_emissions_f32: bad shape B=%d L=%d (1..%d) V=%d Smax=%d ld_row=%lld", B, L, kMaxFrames, V,
                   Smax, (long long)ld_row);
    VASR_CHECK_ARG(blank >= 0 && blank < V, "vasr_ctc_emissions_f32: blank=%d outside [0, %d)", blank, V);
    if (Smax > kMaxTarget) {
        set_error("vasr_ctc_emissions_f32: Smax=%d above the supported %d", Smax, kMaxTarget);
        return VASR_EUNSUPPORTED;
    }
    if (B == 0) return VASR_OK;
    const int64_t rows = (int64_t)B * L;
    hipLaunchKernelGGL(ctc_emissions_kernel, dim3((unsigned)((rows + kEmisWaves - 1) / kEmisWaves)),
                       dim3(kEmisWaves * kWave), 0, as_stream(stream), logits, ld_row, ld_utt, B, L, V, targets, Smax,
                       frames, tlen, blank, emis);
    return launch_status("vasr_ctc_emissions_f32");
}

namespace vasr {
namespace {

template <bool ALIGN, bool STORE = false>
void launch_lattice(const float* emis, int B, int L, int Smax, const int32_t* targets, const int32_t* frames,
                    const int32_t* tlen, float* out, uint8_t* bp, int32_t* frame_state, int32_t* out_start,
                    int32_t* out_end, float* alpha, hipStream_t s) {
    const int S = 2 * Smax + 1;
    const int row = bp_row_bytes(Smax);
#define VASR_LATTICE(R, THREADS)                                                                                   \
    hipLaunchKernelGGL((ctc_lattice_kernel<R, ALIGN, STORE>), dim3(B), dim3(THREADS), 0, s, emis, L, Smax, targets, \
                       frames, tlen, out, bp, row, frame_state, out_start, out_end, alpha)
    // the fewest waves that hold the lattice; within one wave, the fewest states per lane
    if constexpr (!ALIGN) {  // (a lane's back-pointers fill whole bytes from R = 4 on)
        if (S <= 2 * kWave) {
            VASR_LATTICE(2, kWave);
            return;
        }
    }
    if (S <= 4 * kWave) {
        VASR_LATTICE(4, kWave);
    } else {
        VASR_LATTICE(8, kWave * ((S + 8 * kWave - 1) / (8 * kWave)));  // <= 9 waves at Smax = 2048
    }
#undef VASR_LATTICE
}

}  // namespace
}  // namespace vasr

VASR_API int vasr_ctc_loss_f32(const float* emis, int B, int L, int Smax, const int32_t* targets,
                               const int32_t* frames, const int32_t* tlen, float* out_nll, void* stream) {
    using namespace vasr;
    const int rc = check_lattice("vasr_ctc_loss_f32", emis, B, L, Smax, targets, frames, tlen);
    if (rc != VASR_OK) return rc;
    VASR_CHECK_ARG(out_nll, "vasr_ctc_loss_f32: null pointer");
    if (B == 0) return VASR_OK;
    launch_lattice<false>(emis, B, L, Smax, targets, frames, tlen, out_nll, nullptr, nullptr, nullptr, nullptr,
                          nullptr, as_stream(stream));
    return launch_status("vasr_ctc_loss_f32");
}

VASR_API int64_t vasr_ctc_align_workspace_bytes(int B, int L, int Smax) {
    if (B < 0 || L < 0 || Smax < 0) return 0;
    return (int64_t)B * L * vasr::bp_row_bytes(Smax);
}

VASR_API int vasr_ctc_align_f32(const float* emis, int B, int L, int Smax, const int32_t* targets,
                                const int32_t* frames, const int32_t* tlen, void* workspace, int64_t workspace_bytes,
                                int32_t* frame_state, int32_t* out_start, int32_t* out_end, float* out_score,
                                void* stream) {
    using namespace vasr;
    const int rc = check_lattice("vasr_ctc_align_f32", emis, B, L, Smax, targets, frames, tlen);
    if (rc != VASR_OK) return rc;
    VASR_CHECK_ARG(workspace && frame_state && out_score && ((out_start && out_end) || Smax == 0),
                   "vasr_ctc_align_f32: null pointer");
    VASR_CHECK_ARG(workspace_bytes >= vasr_ctc_align_workspace_bytes(B, L, Smax),
                   "vasr_ctc_align_f32: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                   (long long)vasr_ctc_align_workspace_bytes(B, L, Smax));
    if (B == 0) return VASR_OK;
    launch_lattice<true>(emis, B, L, Smax, targets, frames, tlen, out_score, static_cast<uint8_t*>(workspace),
                         frame_state, out_start, out_end, nullptr, as_stream(stream));
    return launch_status("vasr_ctc_align_f32");
}

// ------------------------------------------------------------------ backward: occupancy and logit gradient
//
// The gradient of nll_b with respect to the logits of frame t < T is
//     softmax(logits[b][t])[v] - sum over the slots whose token is v of occ[b][t][slot],
// with occ the posterior occupancy of the blank (slot 0, summed over the blank states) and of each
// label (slot 1 + j):  gamma[t][s] = exp(alpha[t][s] + beta[t][s] - e[t][s] + nll).
//   - vasr_ctc_loss_alpha_f32: the loss kernel with STORE, which keeps every frame's alpha.
//   - ctc_occupancy_kernel: beta by the forward kernel's own layout walked from frame T - 1 down to
//     0 over the MIRRORED state index m = S' - 1 - s: beta's sources (s, s + 1, s + 2) become
//     (m, m - 1, m - 2) and even slots stay blanks, so from_left_lane, the edge hand-over and the
//     grouped prefetch are the forward's; alpha of the frame group is prefetched beside the emissions.
//   - ctc_chain_kernel + ctc_grad_logits_kernel: one wave per logit row recomputes the row's
//     log-sum-exp (row_lse, bitwise the emissions pass's), writes scale * softmax, and then
//     overwrites the blank's and the target tokens' columns.  Slots that share a token are summed
//     in ascending order by the lane of the first of them, along a next-same-token chain built
//     once per utterance; no atomics, one writer per column.
namespace vasr {
namespace {

template <int R>
__global__ __launch_bounds__(640) void ctc_occupancy_kernel(
    const float* __restrict__ emis, const float* __restrict__ alpha, const float* __restrict__ nll, int L, int Smax,
    const int32_t* __restrict__ targets, const int32_t* __restrict__ frames, const int32_t* __restrict__ tlen,
    float* __restrict__ occ) {
    constexpr int H = R / 2;                     // labels per lane
    constexpr int kFrameGroup = R == 8 ? 4 : 8;  // as ctc_lattice_kernel
    __shared__ float edge[2][16];
    __shared__ float bsum[2][kFrameGroup][16];  // per-wave sums of the blank states, by group parity

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int nwaves = blockDim.x >> 6;
    const int T = min(max(frames[b], 0), L);
    const int n = min(max(tlen[b], 0), Smax);
    const int S = 2 * n + 1;
    const int E = Smax + 1;
    const float nl = nll[b];
    float* o = occ + (int64_t)b * L * E;

    // padding rows, and every row of an infeasible utterance: exact zeros
    const int Tz = nl == INFINITY ? 0 : T;
    for (int64_t i = (int64_t)Tz * E + tid; i < (int64_t)L * E; i += blockDim.x) o[i] = 0.f;
    if (Tz == 0) return;  // uniform

    const float* e = emis + (int64_t)b * L * E;
    const float* al = alpha + (int64_t)b * L * (2 * Smax + 1);
    const int32_t* tg = targets + (int64_t)b * Smax;
    const int m0 = tid * R;  // first mirrored state of this lane
    const int i0 = tid * H;  // mirrored index of its first label: label j = n - 1 - i

    // mirrored label i may be entered from i - 1 directly iff labels j and j + 1 differ
    bool skip[H], live[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int i = i0 + h;
        live[h] = i < n;
        skip[h] = live[h] && i >= 1 && tg[n - 1 - i] != tg[n - i];
    }

    // "frame T": all the mass in mirrored state 0, so frame T - 1 comes out of the same recursion
    // with beta = e in states S' - 1 and S' - 2
    float a[R];
#pragma unroll
    for (int k = 0; k < R; ++k) a[k] = (m0 + k == 0) ? 0.f : -INFINITY;

    // step q = 0, 1, ... is frame T - 1 - q
    float eb[2][kFrameGroup], el[2][kFrameGroup][H], af[2][kFrameGroup][R];
    // The loads are unconditional, at indices clamped into the utterance's own written range (frame
    // 0 .. T - 1, slot 0 .. n, state 0 .. S' - 1): a lane-varying branch around each of a group's
    // 40-odd loads costs more than the loads.  What a dead label or a state past S' loaded is
    // replaced by -inf where it is used (step), so nothing waits for a load here.
    auto fetch = [&](int buf, int q0) {
#pragma unroll
        for (int g = 0; g < kFrameGroup; ++g) {
            const int t = max(T - 1 - (q0 + g), 0);
            const float* et = e + (int64_t)t * E;
            const float* at = al + (int64_t)t * (2 * Smax + 1);
            eb[buf][g] = et[0];
#pragma unroll
            for (int h = 0; h < H; ++h) el[buf][g][h] = et[max(n - i0 - h, 0)];
#pragma unroll
            for (int k = 0; k < R; ++k) af[buf][g][k] = at[max(S - 1 - m0 - k, 0)];
        }
    };
    // one frame: beta, then this lane's occupancies; returns the sum over its blank states
    auto step = [&](int q, float ebt, const float* elt, const float* aft) -> float {
        float first = -INFINITY;
        if (nwaves > 1) {  // uniform per launch
            if (lane == kWave - 1) edge[q & 1][wave] = a[R - 1];
            __syncthreads();
            if (wave > 0) first = edge[q & 1][wave - 1];
        }
        const float left = from_left_lane(a[R - 1], first);
        float nw[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const float c0 = a[k];
            const float c1 = k >= 1 ? a[k - 1] : left;
            const float c2 = (k & 1) && skip[k >> 1] ? (k >= 2 ? a[k - 2] : left) : -INFINITY;
            const float em = (k & 1) ? (live[k >> 1] ? elt[k >> 1] : -INFINITY) : ebt;
            nw[k] = ((k & 1) ? lse3(c0, c1, c2) : lse2(c0, c1)) + em;
        }
        float* orow = o + (int64_t)(T - 1 - q) * E;
        float blanks = 0.f;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            a[k] = nw[k];
            const float em = (k & 1) ? elt[k >> 1] : ebt;
            const float ak = m0 + k < S ? aft[k] : -INFINITY;
            // alpha + beta is the one sum at the magnitude of nll; states past S' have alpha = -inf.
            // A posterior is at most 1: the rounding of alpha + beta in the thousands can put it
            // 1e-4 above, and the clamp only moves a value towards the exact one (NaN stays NaN).
            float gam = (ak == -INFINITY || a[k] == -INFINITY) ? 0.f : fast_exp(((ak + a[k]) + nl) - em);
            gam = gam > 1.f ? 1.f : gam;
            if (k & 1) {
                // live labels fill slots 1 .. n, the other lanes' zero slots n + 1 .. Smax
                const int i = i0 + (k >> 1);
                if (i < Smax) orow[live[k >> 1] ? n - i : 1 + i] = live[k >> 1] ? gam : 0.f;
            } else {
                blanks += gam;
            }
        }
        return blanks;
    };
    // the blank column of a group's frames: wave reduction, then the waves in wave order
    auto flush = [&](int q0, int par, const float* bl) {
        float w[kFrameGroup];
#pragma unroll
        for (int g = 0; g < kFrameGroup; ++g) w[g] = wave_sum(bl[g]);
        if (nwaves == 1) {
#pragma unroll
            for (int g = 0; g < kFrameGroup; ++g)
                if (lane == 0 && q0 + g < T) o[(int64_t)(T - 1 - q0 - g) * E] = w[g] > 1.f ? 1.f : w[g];
            return;
        }
        // bsum[par] is next written two groups on, after the barrier of the group between
        if (lane == 0) {
#pragma unroll
            for (int g = 0; g < kFrameGroup; ++g) bsum[par][g][wave] = w[g];
        }
        __syncthreads();
        if (tid < kFrameGroup && q0 + tid < T) {
            float sum = bsum[par][tid][0];
            for (int v = 1; v < nwaves; ++v) sum += bsum[par][tid][v];
            o[(int64_t)(T - 1 - q0 - tid) * E] = sum > 1.f ? 1.f : sum;
        }
    };

    fetch(0, 0);
    for (int q0 = 0; q0 < T; q0 += 2 * kFrameGroup) {  // two groups per trip: the buffers stay in registers
        float bl[kFrameGroup];
        fetch(1, q0 + kFrameGroup);
#pragma unroll
        for (int g = 0; g < kFrameGroup; ++g) bl[g] = q0 + g < T ? step(q0 + g, eb[0][g], el[0][g], af[0][g]) : 0.f;
        flush(q0, 0, bl);
        fetch(0, q0 + 2 * kFrameGroup);
#pragma unroll
        for (int g = 0; g < kFrameGroup; ++g)
            bl[g] = q0 + kFrameGroup + g < T ? step(q0 + kFrameGroup + g, eb[1][g], el[1][g], af[1][g]) : 0.f;
        flush(q0 + kFrameGroup, 1, bl);
    }
}

// chain[b][slot], slot 0 = the blank, slot 1 + j = label j (slot <= tlen[b]): the next slot with the
// same token (0: none) in the low bits; the sign bit is set for a slot that is not the first of its
// token, and for a token outside [0, V), which is never used as an index.
constexpr int kChainThreads = 256;
__global__ __launch_bounds__(kChainThreads) void ctc_chain_kernel(
    const int32_t* __restrict__ targets, int Smax, const int32_t* __restrict__ tlen, int blank, int V,
    int32_t* __restrict__ chain) {
    __shared__ int32_t tok[kMaxTarget + 1];
    __shared__ int32_t nxt[kMaxTarget + 1];
    __shared__ int32_t later[kMaxTarget + 1];  // 1: an earlier slot has this token
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(tlen[b], 0), Smax);
    const int32_t* tg = targets + (int64_t)b * Smax;
    for (int j = tid; j <= n; j += kChainThreads) {
        tok[j] = j == 0 ? blank : tg[j - 1];
        later[j] = 0;
    }
    __syncthreads();
    for (int j = tid; j <= n; j += kChainThreads) {
        const int mine = tok[j];
        int k = 0;
        if (mine >= 0 && mine < V) {
            for (k = j + 1; k <= n && tok[k] != mine; ++k) {}
            if (k > n) k = 0;
            if (k) later[k] = 1;  // one writer: slot k has one predecessor
        } else {
            later[j] = 1;  // only slot j itself writes here: no chain reaches an invalid token
        }
        nxt[j] = k;
    }
    __syncthreads();
    for (int j = tid; j <= n; j += kChainThreads)
        chain[(int64_t)b * (Smax + 1) + j] = nxt[j] | (later[j] ? (int32_t)0x80000000 : 0);
}

__global__ __launch_bounds__(kEmisWaves* kWave) void ctc_grad_logits_kernel(
    const float* __restrict__ logits, int64_t ld_row, int64_t ld_utt, int B, int L, int V,
    const int32_t* __restrict__ targets, int Smax, const int32_t* __restrict__ frames,
    const int32_t* __restrict__ tlen, int blank, const float* __restrict__ occ, const int32_t* __restrict__ chain,
    const float* __restrict__ scale, float* __restrict__ grad) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = (int64_t)blockIdx.x * kEmisWaves + (threadIdx.x >> 6);
    const bool inside = r < (int64_t)B * L;
    const int b = inside ? (int)(r / L) : 0, t = (int)(r - (int64_t)b * L);
    const bool valid = inside && t < min(max(frames[b], 0), L);  // a predicate: the barrier below is for every wave
    const float* row = logits + (int64_t)b * ld_utt + (int64_t)t * ld_row;
    float* gr = grad + r * (int64_t)V;
    const int nfull = V >> 2, nch = (nfull + kWave - 1) / kWave;
    const bool gwide = (reinterpret_cast<uintptr_t>(gr) & 15) == 0;
    float Ms = 0.f, lse = 0.f, sc = 0.f;

    if (inside && !valid) {  // padding rows are never read, and their gradient is zero
        for (int c = 0; c < nch; ++c) {
            const int g = c * kWave + lane;
            if (g >= nfull) break;
            if (gwide) {
                reinterpret_cast<float4*>(gr)[g] = make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                gr[4 * g] = gr[4 * g + 1] = gr[4 * g + 2] = gr[4 * g + 3] = 0.f;
            }
        }
        if (lane < (V & 3)) gr[4 * nfull + lane] = 0.f;
    }
    if (valid) {
        const bool wide = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
        lse = row_lse(row, V, lane, wide, Ms);
        sc = scale[b];
        // scale * softmax over the whole row, the same element -> lane assignment as the first pass
#pragma unroll 4
        for (int c = 0; c < nch; ++c) {
            const int g = c * kWave + lane;
            if (g < nfull) {
                float4 q;
                if (wide) {
                    q = reinterpret_cast<const float4*>(row)[g];
                } else {
                    q = make_float4(row[4 * g], row[4 * g + 1], row[4 * g + 2], row[4 * g + 3]);
                }
                q.x = sc * fast_exp((q.x - Ms) - lse);
                q.y = sc * fast_exp((q.y - Ms) - lse);
                q.z = sc * fast_exp((q.z - Ms) - lse);
                q.w = sc * fast_exp((q.w - Ms) - lse);
                if (gwide) {
                    reinterpret_cast<float4*>(gr)[g] = q;
                } else {
                    gr[4 * g] = q.x, gr[4 * g + 1] = q.y, gr[4 * g + 2] = q.z, gr[4 * g + 3] = q.w;
                }
            }
        }
        if (lane < (V & 3)) gr[4 * nfull + lane] = sc * fast_exp((row[4 * nfull + lane] - Ms) - lse);
    }
    // the target columns below are written a second time, by other lanes: this wave's stores above
    // have to be complete first (the barrier waits for them)
    __syncthreads();
    if (valid) {
        const int E = Smax + 1;
        const int n = min(max(tlen[b], 0), Smax);
        const int32_t* tg = targets + (int64_t)b * Smax;
        const int32_t* ch = chain + (int64_t)b * E;
        const float* oc = occ + r * (int64_t)E;
        for (int j = lane; j <= n; j += kWave) {
            const int32_t c = ch[j];
            if (c < 0) continue;  // a later slot of its token, or a token outside [0, V)
            float sum = oc[j];    // this token's slots in ascending order
            for (int k = c; k != 0; k = ch[k] & 0x7fffffff) sum += oc[k];
            const int v = j == 0 ? blank : tg[j - 1];
            gr[v] = sc * (fast_exp((row[v] - Ms) - lse) - sum);
        }
    }
}

void launch_occupancy(const float* emis, const float* alpha, const float* nll, int B, int L, int Smax,
                      const int32_t* targets, const int32_t* frames, const int32_t* tlen, float* occ, hipStream_t s) {
    const int S = 2 * Smax + 1;
#define VASR_OCCUPANCY(R, THREADS)                                                                             \
    hipLaunchKernelGGL((ctc_occupancy_kernel<R>), dim3(B), dim3(THREADS), 0, s, emis, alpha, nll, L, Smax, targets, \
                       frames, tlen, occ)
    if (S <= 2 * kWave) {  // as launch_lattice
        VASR_OCCUPANCY(2, kWave);
    } else if (S <= 4 * kWave) {
        VASR_OCCUPANCY(4, kWave);
    } else {
        VASR_OCCUPANCY(8, kWave * ((S + 8 * kWave - 1) / (8 * kWave)));
    }
#undef VASR_OCCUPANCY
}

}  // namespace
}  // namespace vasr

VASR_API int vasr_ctc_loss_alpha_f32(const float* emis, int B, int L, int Smax, const int32_t* targets,
                                     const int32_t* frames, const int32_t* tlen, float* out_nll, float* alpha,
                                     int64_t alpha_elems, void* stream) {
    using namespace vasr;
    const int rc = check_lattice("vasr_ctc_loss_alpha_f32", emis, B, L, Smax, targets, frames, tlen);
    if (rc != VASR_OK) return rc;
    VASR_CHECK_ARG(out_nll && alpha, "vasr_ctc_loss_alpha_f32: null pointer");
    VASR_CHECK_ARG(alpha_elems >= (int64_t)B * L * (2 * Smax + 1),
                   "vasr_ctc_loss_alpha_f32: alpha of %lld floats, %lld needed", (long long)alpha_elems,
                   (long long)B * L * (2 * Smax + 1));
    if (B == 0) return VASR_OK;
    launch_lattice<false, true>(emis, B, L, Smax, targets, frames, tlen, out_nll, nullptr, nullptr, nullptr, nullptr,
                                alpha, as_stream(stream));
    return launch_status("vasr_ctc_loss_alpha_f32");
}

VASR_API int vasr_ctc_occupancy_f32(const float* emis, const float* alpha, int64_t alpha_elems, const float* nll, int B,
                                    int L, int Smax, const int32_t* targets, const int32_t* frames,
                                    const int32_t* tlen, float* occ, void* stream) {
    using namespace vasr;
    const int rc = check_lattice("vasr_ctc_occupancy_f32", emis, B, L, Smax, targets, frames, tlen);
    if (rc != VASR_OK) return rc;
    VASR_CHECK_ARG(alpha && nll && occ, "vasr_ctc_occupancy_f32: null pointer");
    VASR_CHECK_ARG(alpha_elems >= (int64_t)B * L * (2 * Smax + 1),
                   "vasr_ctc_occupancy_f32: alpha of %lld floats, %lld needed", (long long)alpha_elems,
                   (long long)B * L * (2 * Smax + 1));
    if (B == 0) return VASR_OK;
    launch_occupancy(emis, alpha, nll, B, L, Smax, targets, frames, tlen, occ, as_stream(stream));
    return launch_status("vasr_ctc_occupancy_f32");
}

VASR_API int vasr_ctc_grad_logits_f32(const float* logits, int64_t ld_row, int64_t ld_utt, int B, int L, int V,
                                      const int32_t* targets, int Smax, const int32_t* frames, const int32_t* tlen,
                                      int blank, const float* occ, const float* scale, int32_t* workspace,
                                      int64_t workspace_elems, float* grad, void* stream) {
    using namespace vasr;
    VASR_CHECK_ARG(logits && frames && tlen && occ && scale && workspace && grad && (targets || Smax == 0),
                   "vasr_ctc_grad_logits_f32: null pointer");
    VASR_CHECK_ARG(B >= 0 && L >= 1 && L <= kMaxFrames && V >= 1 && Smax >= 0 && ld_row >= V,
                   "vasr_ctc_grad_logits_f32: bad shape B=%d L=%d (1..%d) V=%d Smax=%d ld_row=%lld", B, L, kMaxFrames,
                   V, Smax, (long long)ld_row);
    VASR_CHECK_ARG(blank >= 0 && blank < V, "vasr_ctc_grad_logits_f32: blank=%d outside [0, %d)", blank, V);
    if (Smax > kMaxTarget) {
        set_error("vasr_ctc_grad_logits_f32: Smax=%d above the supported %d", Smax, kMaxTarget);
        return VASR_EUNSUPPORTED;
    }
    VASR_CHECK_ARG(workspace_elems >= (int64_t)B * (Smax + 1),
                   "vasr_ctc_grad_logits_f32: workspace of %lld int32, %lld needed", (long long)workspace_elems,
                   (long long)B * (Smax + 1));
    if (B == 0) return VASR_OK;
    hipLaunchKernelGGL(ctc_chain_kernel, dim3(B), dim3(kChainThreads), 0, as_stream(stream), targets, Smax, tlen, blank,
                       V, workspace);
    const int64_t rows = (int64_t)B * L;
    hipLaunchKernelGGL(ctc_grad_logits_kernel, dim3((unsigned)((rows + kEmisWaves - 1) / kEmisWaves)),
                       dim3(kEmisWaves * kWave), 0, as_stream(stream), logits, ld_row, ld_utt, B, L, V, targets, Smax,
                       frames, tlen, blank, occ, workspace, scale, grad);
    return launch_status("vasr_ctc_grad_logits_f32");
}

// ------------------------------------------------------------------ the loss on the head, without logits
//
// The CTC head's logits are xn W^T + bias with xn the head's normalised rows.  The loss needs, per
// row, the log-sum-exp over the vocabulary and the blank's and the target tokens' logits:
//   - the GEMM with VASR_EPI_LSE (gemm_common.h) leaves one {m, s} pair per 32 columns of each row;
//     lse_combine_kernel folds a row's pairs into stats[row] = {Ms, lse}, row_lse's two values;
//   - ctc_head_emissions_kernel recomputes only the Smax + 1 needed logits per row as dot products
//     of the fp32 inputs accumulated in fp64, and writes the emissions vasr_ctc_emissions_f32
//     would have gathered;
//   - ctc_grad_logits_stats_kernel is the logit gradient over one chunk of recomputed logits, in
//     place, with the row statistics read from stats.
namespace vasr {
namespace {

constexpr int kCombineWaves = 4;

__global__ __launch_bounds__(kCombineWaves* kWave) void lse_combine_kernel(const float2* __restrict__ pairs, int64_t ld,
                                                                           int slots, int M, float* __restrict__ stats) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = (int64_t)blockIdx.x * kCombineWaves + (threadIdx.x >> 6);
    if (r >= M) return;
    // running (m, s) per lane over slots lane, lane + 64, ...; then the 64 lanes as row_lse does
    float Ms;
    const float lse = lse_pairs_fold(pairs + r * ld, 1, slots, lane, Ms);
    if (lane == 0) reinterpret_cast<float2*>(stats)[r] = make_float2(Ms, lse);
}

constexpr int kHeadRows = 64;     // frames per workgroup: one per lane
constexpr int kHeadWaves = 8;     // waves per workgroup, each on its own tokens
constexpr int kHeadTok = 4;       // tokens a wave carries through one pass over K
constexpr int kHeadLds = 65536;   // bytes of LDS a workgroup may ask for

// One workgroup per (utterance, block of 64 frames).  The block's rows of xn sit in LDS k-major,
// xs[k][row] with rows padded to 65 floats: the staging writes (lanes along k) and the dot
// products' reads (lanes along rows) are both conflict-free.  Lane = frame; a wave takes four
// tokens at a time, whose W rows are wave-uniform (scalar loads), so every W row is read once per
// block and every LDS read feeds four multiply-adds.  The products are accumulated in fp64 and the
// emission is rounded once: a token's logit then carries no error of its own into the lattice.  (A
// per-frame error, as the one of lse, shifts every path alike and cancels in the occupancy; a
// per-token error of fp32-dot size does not, and showed in the gradient: DESIGN.md §4.)
__global__ __launch_bounds__(kHeadWaves* kWave) void ctc_head_emissions_kernel(
    const float* __restrict__ xn, int64_t ld_x, const float* __restrict__ W, int64_t ldw,
    const float* __restrict__ bias, const float* __restrict__ stats, int L, int V, int K,
    const int32_t* __restrict__ targets, int Smax, const int32_t* __restrict__ frames,
    const int32_t* __restrict__ tlen, int blank, float* __restrict__ emis) {
    extern __shared__ float xs[];
    constexpr int LDR = kHeadRows + 1;
    const int blocks_per_utt = (L + kHeadRows - 1) / kHeadRows;
    const int b = blockIdx.x / blocks_per_utt, t0 = (blockIdx.x - b * blocks_per_utt) * kHeadRows;
    const int T = min(max(frames[b], 0), L);
    if (t0 >= T) return;  // uniform: padding rows are never read
    const int nrows = min(kHeadRows, T - t0);
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    const float* xb = xn + ((int64_t)b * L + t0) * ld_x;
    for (int i = threadIdx.x; i < nrows * K; i += kHeadWaves * kWave) {
        const int row = i / K, k = i - row * K;
        xs[k * LDR + row] = xb[(int64_t)row * ld_x + k];
    }
    __syncthreads();
    if (lane >= nrows) return;  // no barrier below

    const int64_t r = (int64_t)b * L + t0 + lane;
    const float Ms = stats[2 * r], lse = stats[2 * r + 1];
    float* e = emis + r * (int64_t)(Smax + 1);
    const int n = min(max(tlen[b], 0), Smax);
    const int32_t* tg = targets + (int64_t)b * Smax;
    const float* xl = xs + lane;
    for (int j0 = wave * kHeadTok; j0 <= n; j0 += kHeadWaves * kHeadTok) {
        int tok[kHeadTok];
        const float* w[kHeadTok];
        double a[kHeadTok];
#pragma unroll
        for (int q = 0; q < kHeadTok; ++q) {
            const int j = min(j0 + q, n);  // past the last slot: slot n again, not stored
            tok[q] = j == 0 ? blank : tg[j - 1];
            // a token id outside [0, V) is not used as an index: its emission is -inf
            w[q] = W + (int64_t)((tok[q] >= 0 && tok[q] < V) ? tok[q] : 0) * ldw;
            a[q] = 0.0;
        }
#pragma unroll 8
        for (int k = 0; k < K; ++k) {
            const double x = (double)xl[k * LDR];
#pragma unroll
            for (int q = 0; q < kHeadTok; ++q) a[q] = __builtin_fma(x, (double)w[q][k], a[q]);
        }
#pragma unroll
        for (int q = 0; q < kHeadTok; ++q) {
            if (j0 + q > n) break;
            const bool ok = tok[q] >= 0 && tok[q] < V;
            double v = a[q];
            if (bias) v += (double)bias[ok ? tok[q] : 0];
            e[j0 + q] = ok ? (float)((v - (double)Ms) - (double)lse) : -INFINITY;
        }
    }
}

// ctc_grad_logits_kernel over a buffer that holds the logits and receives the gradient (x), with
// the row's Ms and lse read from stats (no pass for them).  Each lane reads an element before it
// writes it.  The target columns: pass one left sc * softmax there, so the final value is that
// minus sc * (the token's summed occupancy), one fused multiply-add on the stored value -- the
// original logit is not needed again (within one rounding of sc * softmax of the unfused
// kernel's sc * (softmax - sum)).  Padding rows: exact zeros, never read.
__global__ __launch_bounds__(kEmisWaves* kWave) void ctc_grad_logits_stats_kernel(
    float* x, int64_t ld_row, int64_t ld_utt, int B, int L, int V, const float* __restrict__ stats,
    const int32_t* __restrict__ targets, int Smax, const int32_t* __restrict__ frames,
    const int32_t* __restrict__ tlen, int blank, const float* __restrict__ occ, const int32_t* __restrict__ chain,
    const float* __restrict__ scale) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = (int64_t)blockIdx.x * kEmisWaves + (threadIdx.x >> 6);
    const bool inside = r < (int64_t)B * L;
    const int b = inside ? (int)(r / L) : 0, t = (int)(r - (int64_t)b * L);
    const bool valid = inside && t < min(max(frames[b], 0), L);  // a predicate: the barrier below is for every wave
    float* row = x + (int64_t)b * ld_utt + (int64_t)t * ld_row;
    const int nfull = V >> 2, nch = (nfull + kWave - 1) / kWave;
    const bool wide = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    float sc = 0.f;

    if (inside && !valid) {
        for (int c = 0; c < nch; ++c) {
            const int g = c * kWave + lane;
            if (g >= nfull) break;
            if (wide) {
                reinterpret_cast<float4*>(row)[g] = make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                row[4 * g] = row[4 * g + 1] = row[4 * g + 2] = row[4 * g + 3] = 0.f;
            }
        }
        if (lane < (V & 3)) row[4 * nfull + lane] = 0.f;
    }
    if (valid) {
        const float Ms = stats[2 * r], lse = stats[2 * r + 1];
        sc = scale[b];
#pragma unroll 4
        for (int c = 0; c < nch; ++c) {
            const int g = c * kWave + lane;
            if (g < nfull) {
                float4 q;
                if (wide) {
                    q = reinterpret_cast<const float4*>(row)[g];
                } else {
                    q = make_float4(row[4 * g], row[4 * g + 1], row[4 * g + 2], row[4 * g + 3]);
                }
                q.x = sc * fast_exp((q.x - Ms) - lse);
                q.y = sc * fast_exp((q.y - Ms) - lse);
                q.z = sc * fast_exp((q.z - Ms) - lse);
                q.w = sc * fast_exp((q.w - Ms) - lse);
                if (wide) {
                    reinterpret_cast<float4*>(row)[g] = q;
                } else {
                    row[4 * g] = q.x, row[4 * g + 1] = q.y, row[4 * g + 2] = q.z, row[4 * g + 3] = q.w;
                }
            }
        }
        if (lane < (V & 3)) row[4 * nfull + lane] = sc * fast_exp((row[4 * nfull + lane] - Ms) - lse);
    }
    // the target columns below are updated by other lanes: this wave's stores above have to be
    // complete first (the barrier waits for them)
    __syncthreads();
    if (valid) {
        const int E = Smax + 1;
        const int n = min(max(tlen[b], 0), Smax);
        const int32_t* tg = targets + (int64_t)b * Smax;
        const int32_t* ch = chain + (int64_t)b * E;
        const float* oc = occ + r * (int64_t)E;
        for (int j = lane; j <= n; j += kWave) {
            const int32_t c = ch[j];
            if (c < 0) continue;  // a later slot of its token, or a token outside [0, V)
            float sum = oc[j];    // this token's slots in ascending order
            for (int k = c; k != 0; k = ch[k] & 0x7fffffff) sum += oc[k];
            const int v = j == 0 ? blank : tg[j - 1];
            row[v] = __builtin_fmaf(-sc, sum, row[v]);
        }
    }
}

}  // namespace
}  // namespace vasr

VASR_API int vasr_lse_combine_f32(const float* pairs, int64_t ld, int slots, int M, float* stats, void* stream) {
    using namespace vasr;
    VASR_CHECK_ARG(pairs && stats, "vasr_lse_combine_f32: null pointer");
    VASR_CHECK_ARG((reinterpret_cast<uintptr_t>(pairs) & 7) == 0 && (reinterpret_cast<uintptr_t>(stats) & 7) == 0,
                   "vasr_lse_combine_f32: pairs and stats must be 8-byte aligned");
    VASR_CHECK_ARG(M >= 0 && slots >= 1 && ld >= slots, "vasr_lse_combine_f32: bad shape M=%d slots=%d ld=%lld", M, slots,
                   (long long)ld);
    if (M == 0) return VASR_OK;
    hipLaunchKernelGGL(lse_combine_kernel, dim3((M + kCombineWaves - 1) / kCombineWaves), dim3(kCombineWaves * kWave), 0,
                       as_stream(stream), reinterpret_cast<const float2*>(pairs), ld, slots, M, stats);
    return launch_status("vasr_lse_combine_f32");
}

VASR_API int vasr_ctc_head_emissions_f32(const float* xn, int64_t ld_x, const float* W, int64_t ldw, const float* bias,
                                         const float* stats, int B, int L, int V, int K, const int32_t* targets,
                                         int Smax, const int32_t* frames, const int32_t* tlen, int blank, float* emis,
                                         void* stream) {
    using namespace vasr;
    VASR_CHECK_ARG(xn && W && stats && frames && tlen && emis && (targets || Smax == 0),
                   "vasr_ctc_head_emissions_f32: null pointer");
    VASR_CHECK_ARG(B >= 0 && L >= 1 && L <= kMaxFrames && V >= 1 && K >= 1 && Smax >= 0 && ld_x >= K && ldw >= K,
                   "vasr_ctc_head_emissions_f32: bad shape B=%d L=%d (1..%d) V=%d K=%d Smax=%d ld_x=%lld ldw=%lld", B, L,
                   kMaxFrames, V, K, Smax, (long long)ld_x, (long long)ldw);
    VASR_CHECK_ARG(blank >= 0 && blank < V, "vasr_ctc_head_emissions_f32: blank=%d outside [0, %d)", blank, V);
    if (Smax > kMaxTarget) {
        set_error("vasr_ctc_head_emissions_f32: Smax=%d above the supported %d", Smax, kMaxTarget);
        return VASR_EUNSUPPORTED;
    }
    const int64_t lds = (int64_t)K * (kHeadRows + 1) * 4;
    if (lds > kHeadLds) {
        set_error("vasr_ctc_head_emissions_f32: K=%d needs %lld bytes of LDS for a block of %d rows, %d available", K,
                  (long long)lds, kHeadRows, kHeadLds);
        return VASR_EUNSUPPORTED;
    }
    if (B == 0) return VASR_OK;
    const int blocks = B * ((L + kHeadRows - 1) / kHeadRows);
    hipLaunchKernelGGL(ctc_head_emissions_kernel, dim3(blocks), dim3(kHeadWaves * kWave), (size_t)lds, as_stream(stream),
                       xn, ld_x, W, ldw, bias, stats, L, V, K, targets, Smax, frames, tlen, blank, emis);
    return launch_status("vasr_ctc_head_emissions_f32");
}

VASR_API int vasr_ctc_grad_logits_stats_f32(float* logits, int64_t ld_row, int64_t ld_utt, int B, int L, int V,
                                            const float* stats, const int32_t* targets, int Smax, const int32_t* frames,
                                            const int32_t* tlen, int blank, const float* occ, const float* scale,
                                            int32_t* workspace, int64_t workspace_elems, void* stream) {
    using namespace vasr;
    VASR_CHECK_ARG(logits && stats && frames && tlen && occ && scale && workspace && (targets || Smax == 0),
                   "vasr_ctc_grad_logits_stats_f32: null pointer");
    VASR_CHECK_ARG(B >= 0 && L >= 1 && L <= kMaxFrames && V >= 1 && Smax >= 0 && ld_row >= V,
                   "vasr_ctc_grad_logits_stats_f32: bad shape B=%d L=%d (1..%d) V=%d Smax=%d ld_row=%lld", B, L,
                   kMaxFrames, V, Smax, (long long)ld_row);
    VASR_CHECK_ARG(blank >= 0 && blank < V, "vasr_ctc_grad_logits_stats_f32: blank=%d outside [0, %d)", blank, V);
    if (Smax > kMaxTarget) {
        set_error("vasr_ctc_grad_logits_stats_f32: Smax=%d above the supported %d", Smax, kMaxTarget);
        return VASR_EUNSUPPORTED;
    }
    VASR_CHECK_ARG(workspace_elems >= (int64_t)B * (Smax + 1),
                   "vasr_ctc_grad_logits_stats_f32: workspace of %lld int32, %lld needed", (long long)workspace_elems,
                   (long long)B * (Smax + 1));
    if (B == 0) return VASR_OK;
    hipLaunchKernelGGL(ctc_chain_kernel, dim3(B), dim3(kChainThreads), 0, as_stream(stream), targets, Smax, tlen, blank,
                       V, workspace);
    const int64_t rows = (int64_t)B * L;
    hipLaunchKernelGGL(ctc_grad_logits_stats_kernel, dim3((unsigned)((rows + kEmisWaves - 1) / kEmisWaves)),
                       dim3(kEmisWaves * kWave), 0, as_stream(stream), logits, ld_row, ld_utt, B, L, V, stats, targets,
                       Smax, frames, tlen, blank, occ, workspace, scale);
    return launch_status("vasr_ctc_grad_logits_stats_f32");
}
