// Backward pass of the selective scan's true recurrence (mode 1; include/vasr.h):
//   vasr_ssm_scan_save_f32  the forward that also keeps the state h at every 16-step chunk boundary
//                           (scan_body.inc's ssm_scan_kernel with SAVE: the plain kernel's arithmetic),
//   vasr_ssm_scan_bwd_f32   the reverse-time walk that turns d loss / d out into the gradients of
//                           x, dt, z, B, C and per-workgroup partial sums of those of A and D.
//
// Backward decomposition: the forward's.  A workgroup owns (utterance b, DPB channels); G = N/4
// lanes share a channel and each lane owns 4 state indices as two float2 pairs.  Chunks are walked
// from the last to the first.  Per chunk the workgroup stages x, dt, B, C, gy = g silu(z) and the
// dz factor g sigma (1 + z (1 - sigma)) in LDS, re-runs the recurrence from the chunk's checkpoint
// with the forward's float operations (so h is bitwise the forward's) keeping the 17 states
// h_{t0-1} .. h_{t0+15} in registers (68 VGPRs), and then walks the chunk backwards carrying
// a_{t+1} gh_{t+1} across steps and chunks in registers.  No (B, L, Di, N) array is formed.
//
// Reductions, all in a fixed order (no atomics: the gradients are run-to-run bitwise):
//   sum_n   (dx, ddt, and y for dz): DPP butterfly over the channel's G lanes (group_sum);
//   sum_d   (dB, dC): a lane-xor butterfly over the wave's channels, the four waves' rows summed
//           0..3 from an LDS tile every 8 steps into partials[b][t][workgroup][n], and a second
//           kernel sums the Di / DPB workgroups of an utterance in index order;
//   dA, dD: per (utterance, channel) partial sums over t (per chunk, then over the chunks), left to
//           the caller to sum over (b, d) and b (a deterministic reduction of a small array).
// Contraction is off for scan*.hip; nothing here relies on a fused multiply-add.
#include "scan_kernels.h"

namespace vasr {
namespace {

constexpr int FB = 8;  // steps per dB / dC flush of the cross-wave tile

template <int N, bool GATE>
__global__ __launch_bounds__(256, 3) void ssm_scan_bwd_kernel(
    const float* __restrict__ x, int64_t ld_x, const float* __restrict__ z, int64_t ld_z,
    const float* __restrict__ dt, int64_t ld_dt, const float* __restrict__ bc, int64_t ld_bc,
    const float* __restrict__ Ag, const float* __restrict__ A2g, const float* __restrict__ Dg,
    const float* __restrict__ gout, int64_t ld_g, const float* __restrict__ ckpt, float* __restrict__ dx,
    float* __restrict__ ddt, float* __restrict__ dz, float* __restrict__ dBpart, float* __restrict__ dCpart,
    float* __restrict__ dApart, float* __restrict__ dDpart, int B, int L, int Di) {
#pragma clang fp contract(off)
    constexpr int NPL = 4, NP = 2;
    constexpr int G = N / NPL;     // lanes per channel
    constexpr int DPW = 64 / G;    // channels per wave
    constexpr int DPB = NW * DPW;  // channels per workgroup
    constexpr int TC = T;
    __shared__ float xs[TC * DPB], dts[TC * DPB], gys[TC * DPB], dzc[TC * DPB];
    __shared__ __attribute__((aligned(16))) float bs[TC * N], cs[TC * N];
    __shared__ float o_dx[TC * DPB], o_ddt[TC * DPB], o_dz[TC * DPB];
    __shared__ __attribute__((aligned(16))) float red[NW * FB * 2 * N];

    const int nd = Di / DPB;
    const int b = blockIdx.x / nd;
    const int blk = blockIdx.x - b * nd;
    const int d0 = blk * DPB;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int g = lane % G;
    const int dl = wave * DPW + lane / G;
    const int nch = (L + TC - 1) / TC;
    const int64_t row0 = (int64_t)b * L;

    f2 A2[NP], Av[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        A2[p] = f2{A2g[g * NPL + 2 * p], A2g[g * NPL + 2 * p + 1]};
        Av[p] = f2{Ag[g * NPL + 2 * p], Ag[g * NPL + 2 * p + 1]};
    }
    const float Dd = Dg[d0 + dl];

    f2 agh[NP], dAtot[NP];  // a_{t+1} gh_{t+1}; sum over the chunks done of gh a h_{t-1} dt
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        agh[p] = f2{0.0f, 0.0f};
        dAtot[p] = f2{0.0f, 0.0f};
    }
    float dDtot = 0.0f;

    for (int c = nch - 1; c >= 0; --c) {
        const int t0 = c * TC;
        const int nvalid = min(TC, L - t0);
        // stage the chunk; rows past L are zeros and are never used
        for (int idx = tid; idx < TC * DPB; idx += 64 * NW) {
            const int t = idx / DPB, d = idx - t * DPB;
            float xv = 0.0f, dv = 0.0f, gy = 0.0f, zc = 0.0f;
            if (t < nvalid) {
                const int64_t row = row0 + t0 + t;
                xv = x[row * ld_x + d0 + d];
                dv = dt[row * ld_dt + d0 + d];
                const float gv = gout[row * ld_g + d0 + d];
                if constexpr (GATE) {
                    const float zv = z[row * ld_z + d0 + d];
                    const float sg = 1.0f / (1.0f + expf(-zv));
                    gy = gv * silu_of<1>(zv);
                    zc = gv * (sg * (1.0f + zv * (1.0f - sg)));
                } else {
                    gy = gv;
                }
            }
            xs[idx] = xv;
            dts[idx] = dv;
            gys[idx] = gy;
            dzc[idx] = zc;
        }
        for (int idx = tid; idx < TC * N; idx += 64 * NW) {
            const int t = idx / N, n = idx - t * N;
            float bv = 0.0f, cv = 0.0f;
            if (t < nvalid) {
                const float* r = bc + (row0 + t0 + t) * ld_bc;
                bv = r[n];
                cv = r[N + n];
            }
            bs[idx] = bv;
            cs[idx] = cv;
        }
        __syncthreads();

        // the chunk's states again, from its checkpoint: hs[i] = h before step i, hs[i + 1] after
        f2 hs[TC + 1][NP];
        {
            const float4 h0 = *reinterpret_cast<const float4*>(
                ckpt + (((int64_t)b * nch + c) * Di + d0 + dl) * N + g * NPL);
            hs[0][0] = f2{h0.x, h0.y};
            hs[0][1] = f2{h0.z, h0.w};
        }
#pragma unroll
        for (int i = 0; i < TC; ++i) {
            const float xv = xs[i * DPB + dl];
            const float dv = dts[i * DPB + dl];
            const float4 bv = *reinterpret_cast<const float4*>(bs + i * N + g * NPL);
            const f2 dv2 = {dv, dv}, xv2 = {xv, xv};
            const f2 Bn[NP] = {f2{bv.x, bv.y}, f2{bv.z, bv.w}};
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const f2 dA = exp2v(dv2 * A2[p]);
                const f2 dB = dv2 * Bn[p];
                hs[i + 1][p] = dA * hs[i][p] + xv2 * dB;  // the forward's operations (scan_body.inc, mode 1)
            }
        }

        f2 dAc[NP] = {f2{0.0f, 0.0f}, f2{0.0f, 0.0f}};
        float dDc = 0.0f;
#pragma unroll
        for (int i = TC - 1; i >= 0; --i) {
            if (i < nvalid) {  // block-uniform
                const float xv = xs[i * DPB + dl];
                const float dv = dts[i * DPB + dl];
                const float gy = gys[i * DPB + dl];
                const float4 bv = *reinterpret_cast<const float4*>(bs + i * N + g * NPL);
                const float4 cv = *reinterpret_cast<const float4*>(cs + i * N + g * NPL);
                const f2 Bn[NP] = {f2{bv.x, bv.y}, f2{bv.z, bv.w}};
                const f2 Cn[NP] = {f2{cv.x, cv.y}, f2{cv.z, cv.w}};
                const f2 dv2 = {dv, dv}, gy2 = {gy, gy};
                const float xdt = dv * xv;
                const f2 xdt2 = {xdt, xdt};
                f2 s1 = {0.0f, 0.0f}, s2 = {0.0f, 0.0f}, yp = {0.0f, 0.0f};
                f2 dBv[NP], dCv[NP];
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const f2 a = exp2v(dv2 * A2[p]);
                    const f2 gh = gy2 * Cn[p] + agh[p];
                    dCv[p] = gy2 * hs[i + 1][p];
                    dBv[p] = gh * xdt2;
                    s1 = s1 + gh * Bn[p];
                    const f2 w = gh * (a * hs[i][p]);
                    s2 = s2 + w * Av[p];
                    dAc[p] = dAc[p] + w * dv2;
                    agh[p] = a * gh;
                    if constexpr (GATE) yp = yp + hs[i + 1][p] * Cn[p];
                }
                const float s1s = group_sum<G>(s1.x + s1.y);
                const float s2s = group_sum<G>(s2.x + s2.y);
                dDc += gy * xv;
                if constexpr (GATE) {
                    const float ys = group_sum<G>(yp.x + yp.y);
                    if (g == 0) o_dz[i * DPB + dl] = dzc[i * DPB + dl] * (ys + xv * Dd);
                }
                if (g == 0) {
                    o_dx[i * DPB + dl] = gy * Dd + dv * s1s;
                    o_ddt[i * DPB + dl] = xv * s1s + s2s;
                }
                // sum over the wave's channels (lanes g, g + G, ...), then one row per wave
                float v[8] = {dBv[0].x, dBv[0].y, dBv[1].x, dBv[1].y, dCv[0].x, dCv[0].y, dCv[1].x, dCv[1].y};
#pragma unroll
                for (int off = G; off < 64; off <<= 1) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] += __shfl_xor(v[j], off, 64);
                }
                if (lane < G) {
                    float* r = red + ((wave * FB + (i % FB)) * 2) * N + g * NPL;
                    *reinterpret_cast<float4*>(r) = make_float4(v[0], v[1], v[2], v[3]);
                    *reinterpret_cast<float4*>(r + N) = make_float4(v[4], v[5], v[6], v[7]);
                }
            }
            if (i % FB == 0) {  // steps i .. i + FB - 1 are in the tile: sum the waves 0..3
                __syncthreads();
                for (int idx = tid; idx < FB * 2 * N; idx += 64 * NW) {
                    const int tt = idx / (2 * N), rem = idx - tt * 2 * N;
                    const int t = i + tt;
                    if (t < nvalid) {
                        float acc = red[(0 * FB + tt) * 2 * N + rem];
#pragma unroll
                        for (int w = 1; w < NW; ++w) acc += red[(w * FB + tt) * 2 * N + rem];
                        const int which = rem / N, n = rem - which * N;
                        float* dst = which ? dCpart : dBpart;
                        dst[((row0 + t0 + t) * nd + blk) * N + n] = acc;
                    }
                }
                __syncthreads();
            }
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) dAtot[p] = dAtot[p] + dAc[p];
        dDtot += dDc;
        // the chunk's dx, ddt, dz rows, coalesced along d (visible: the barriers of the last flush)
        for (int idx = tid; idx < TC * DPB; idx += 64 * NW) {
            const int t = idx / DPB, d = idx - t * DPB;
            if (t < nvalid) {
                const int64_t o = (row0 + t0 + t) * Di + d0 + d;
                dx[o] = o_dx[idx];
                ddt[o] = o_ddt[idx];
                if constexpr (GATE) dz[o] = o_dz[idx];
            }
        }
        __syncthreads();  // staging and output tiles are free for the next chunk
    }
    *reinterpret_cast<float4*>(dApart + ((int64_t)b * Di + d0 + dl) * N + g * NPL) =
        make_float4(dAtot[0].x, dAtot[0].y, dAtot[1].x, dAtot[1].y);
    if (g == 0) dDpart[(int64_t)b * Di + d0 + dl] = dDtot;
}

// dB[r][n] = sum_w dBpart[r][w][n] over the nd workgroups of the row's utterance, in index order
// (the same for dC); r = b L + t.
__global__ __launch_bounds__(256) void scan_bwd_reduce_kernel(const float* __restrict__ dBpart,
                                                              const float* __restrict__ dCpart,
                                                              float* __restrict__ dB, float* __restrict__ dC,
                                                              int64_t total, int nd, int N) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t r = i / N;
    const int n = (int)(i - r * N);
    const float* pb = dBpart + r * nd * N + n;
    const float* pc = dCpart + r * nd * N + n;
    float sb = pb[0], sc = pc[0];
    for (int w = 1; w < nd; ++w) {
        sb += pb[(int64_t)w * N];
        sc += pc[(int64_t)w * N];
    }
    dB[i] = sb;
    dC[i] = sc;
}

constexpr int dpb4(int N) { return NW * (64 / (N / 4)); }  // channels per backward workgroup

template <int N>
int launch_bwd(const float* x, int64_t ld_x, const float* z, int64_t ld_z, const float* dt, int64_t ld_dt,
               const float* bc, int64_t ld_bc, const float* A, const float* A2, const float* D, const float* g,
               int64_t ld_g, const float* ckpt, float* dx, float* ddt, float* dz, float* dB, float* dC, float* dApart,
               float* dDpart, float* ws, int B, int L, int Di, hipStream_t s) {
    constexpr int DPB = dpb4(N);
    const int nd = Di / DPB;
    float* dBpart = ws;
    float* dCpart = ws + (int64_t)B * L * nd * N;
    const dim3 grid(B * nd), block(64 * NW);
    if (z)
        hipLaunchKernelGGL((ssm_scan_bwd_kernel<N, true>), grid, block, 0, s, x, ld_x, z, ld_z, dt, ld_dt, bc, ld_bc, A,
                           A2, D, g, ld_g, ckpt, dx, ddt, dz, dBpart, dCpart, dApart, dDpart, B, L, Di);
    else
        hipLaunchKernelGGL((ssm_scan_bwd_kernel<N, false>), grid, block, 0, s, x, ld_x, z, ld_z, dt, ld_dt, bc, ld_bc, A,
                           A2, D, g, ld_g, ckpt, dx, ddt, dz, dBpart, dCpart, dApart, dDpart, B, L, Di);
    int rc = launch_status("vasr_ssm_scan_bwd_f32");
    if (rc != VASR_OK) return rc;
    const int64_t total = (int64_t)B * L * N;
    hipLaunchKernelGGL(scan_bwd_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, dBpart, dCpart,
                       dB, dC, total, nd, N);
    return launch_status("vasr_ssm_scan_bwd_f32");
}

template <int N>
int launch_save(bool two, bool gated, const float* xz, int64_t ld_xz, const float* dt, int64_t ld_dt, const float* bc,
                int64_t ld_bc, const float* A2, const float* D, float* out, int64_t ld_out, int B, int L, int Di,
                float* ckpt, hipStream_t s) {
    if constexpr (N <= 64) {
        if (two)
            return gated ? npl2::launch_save_n<N, true>(xz, ld_xz, dt, ld_dt, bc, ld_bc, A2, D, out, ld_out, B, L, Di, ckpt, s)
                         : npl2::launch_save_n<N, false>(xz, ld_xz, dt, ld_dt, bc, ld_bc, A2, D, out, ld_out, B, L, Di, ckpt, s);
    }
    return gated ? npl4::launch_save_n<N, true>(xz, ld_xz, dt, ld_dt, bc, ld_bc, A2, D, out, ld_out, B, L, Di, ckpt, s)
                 : npl4::launch_save_n<N, false>(xz, ld_xz, dt, ld_dt, bc, ld_bc, A2, D, out, ld_out, B, L, Di, ckpt, s);
}

bool state_dim_ok(int N) { return N == 16 || N == 32 || N == 64 || N == 128; }

}  // namespace
}  // namespace vasr

VASR_API int64_t vasr_ssm_scan_checkpoint_floats(int B, int L, int Di, int N) {
    if (B <= 0 || L <= 0 || Di <= 0 || N <= 0) return 0;
    return (int64_t)B * ((L + vasr::T - 1) / vasr::T) * Di * N;
}

VASR_API int64_t vasr_ssm_scan_bwd_workspace_floats(int B, int L, int Di, int N) {
    if (B <= 0 || L <= 0 || Di <= 0 || !vasr::state_dim_ok(N)) return 0;
    const int dpb = vasr::dpb4(N);
    return 2 * (int64_t)B * L * ((Di + dpb - 1) / dpb) * N;  // the dB and dC partials
}

VASR_API int vasr_ssm_scan_save_f32(const float* xz, int64_t ld_xz, const float* dt, int64_t ld_dt, const float* bc,
                                    int64_t ld_bc, const float* A2, const float* D, float* out, int64_t ld_out, int B,
                                    int L, int Di, int N, int gated, float* ckpt, int64_t ckpt_floats, void* stream) {
    using namespace vasr;
    VASR_CHECK_ARG(xz && dt && bc && A2 && D && out, "vasr_ssm_scan_save_f32: null pointer");
    VASR_CHECK_ARG(gated == 0 || gated == 1, "vasr_ssm_scan_save_f32: gated must be 0 or 1");
    VASR_CHECK_ARG(B >= 0 && L >= 0 && L <= 8192 && Di > 0, "vasr_ssm_scan_save_f32: bad shape B=%d L=%d Di=%d", B, L, Di);
    VASR_CHECK_ARG(ld_xz % 4 == 0 && ld_dt % 4 == 0 && ld_bc % 4 == 0 && Di % 4 == 0,
                   "vasr_ssm_scan_save_f32: leading dims and Di must be multiples of 4");
    VASR_CHECK_ARG(ld_xz >= (gated ? 2 : 1) * (int64_t)Di && ld_dt >= Di && ld_bc >= 2 * N && ld_out >= Di,
                   "vasr_ssm_scan_save_f32: leading dims too small");
    VASR_CHECK_ARG(((reinterpret_cast<uintptr_t>(xz) | reinterpret_cast<uintptr_t>(dt) | reinterpret_cast<uintptr_t>(bc) |
                     reinterpret_cast<uintptr_t>(ckpt)) & 15) == 0,
                   "vasr_ssm_scan_save_f32: inputs and checkpoints must be 16-byte aligned");
    if (!state_dim_ok(N)) {
        set_error("vasr_ssm_scan_save_f32: state dim N=%d not supported (16, 32, 64, 128; zero-pad B, C and A2)", N);
        return VASR_EUNSUPPORTED;
    }
    if (B == 0 || L == 0) return VASR_OK;
    const int64_t need = vasr_ssm_scan_checkpoint_floats(B, L, Di, N);
    VASR_CHECK_ARG(ckpt != nullptr && ckpt_floats >= need, "vasr_ssm_scan_save_f32: checkpoints of %lld floats, %lld needed",
                   (long long)ckpt_floats, (long long)need);
    hipStream_t s = as_stream(stream);
    const bool two = streaming_two(B, Di, N);  // vasr_ssm_scan_f32's layout: the same out, bitwise
    switch (N) {
        case 16: return launch_save<16>(two, gated, xz, ld_xz, dt, ld_dt, bc, ld_bc, A2, D, out, ld_out, B, L, Di, ckpt, s);
        case 32: return launch_save<32>(two, gated, xz, ld_xz, dt, ld_dt, bc, ld_bc, A2, D, out, ld_out, B, L, Di, ckpt, s);
        case 64: return launch_save<64>(two, gated, xz, ld_xz, dt, ld_dt, bc, ld_bc, A2, D, out, ld_out, B, L, Di, ckpt, s);
        default: return launch_save<128>(two, gated, xz, ld_xz, dt, ld_dt, bc, ld_bc, A2, D, out, ld_out, B, L, Di, ckpt, s);
    }
}

VASR_API int vasr_ssm_scan_bwd_f32(const float* x, int64_t ld_x, const float* z, int64_t ld_z, const float* dt,
                                   int64_t ld_dt, const float* bc, int64_t ld_bc, const float* A, const float* A2,
                                   const float* D, const float* g, int64_t ld_g, const float* ckpt, float* dx,
                                   float* ddt, float* dz, float* dB, float* dC, float* dA_part, float* dD_part,
                                   float* workspace, int64_t workspace_floats, int B, int L, int Di, int N,
                                   void* stream) {
    using namespace vasr;
    VASR_CHECK_ARG(x && dt && bc && A && A2 && D && g && ckpt && dx && ddt && dB && dC && dA_part && dD_part,
                   "vasr_ssm_scan_bwd_f32: null pointer");
    VASR_CHECK_ARG((z == nullptr) == (dz == nullptr), "vasr_ssm_scan_bwd_f32: z and dz go together (both or neither)");
    VASR_CHECK_ARG(B >= 0 && L >= 0 && L <= 8192 && Di > 0, "vasr_ssm_scan_bwd_f32: bad shape B=%d L=%d Di=%d", B, L, Di);
    VASR_CHECK_ARG(ld_x >= Di && ld_dt >= Di && ld_g >= Di && ld_bc >= 2 * N && (!z || ld_z >= Di),
                   "vasr_ssm_scan_bwd_f32: leading dims too small");
    VASR_CHECK_ARG(((reinterpret_cast<uintptr_t>(ckpt) | reinterpret_cast<uintptr_t>(dA_part)) & 15) == 0,
                   "vasr_ssm_scan_bwd_f32: checkpoints and dA_part must be 16-byte aligned");
    if (!state_dim_ok(N)) {
        set_error("vasr_ssm_scan_bwd_f32: state dim N=%d not supported (16, 32, 64, 128; zero-pad B, C, A and A2)", N);
        return VASR_EUNSUPPORTED;
    }
    if (Di % dpb4(N) != 0) {
        set_error("vasr_ssm_scan_bwd_f32: Di=%d must be a multiple of %d for N=%d", Di, dpb4(N), N);
        return VASR_EUNSUPPORTED;
    }
    if (B == 0 || L == 0) return VASR_OK;
    const int64_t need = vasr_ssm_scan_bwd_workspace_floats(B, L, Di, N);
    VASR_CHECK_ARG(workspace != nullptr && workspace_floats >= need,
                   "vasr_ssm_scan_bwd_f32: workspace of %lld floats, %lld needed", (long long)workspace_floats,
                   (long long)need);
    hipStream_t s = as_stream(stream);
#define VASR_BWD_N(NN)                                                                                               \
    launch_bwd<NN>(x, ld_x, z, ld_z, dt, ld_dt, bc, ld_bc, A, A2, D, g, ld_g, ckpt, dx, ddt, dz, dB, dC, dA_part, \
                   dD_part, workspace, B, L, Di, s)
    switch (N) {
        case 16: return VASR_BWD_N(16);
        case 32: return VASR_BWD_N(32);
        case 64: return VASR_BWD_N(64);
        default: return VASR_BWD_N(128);
    }
#undef VASR_BWD_N
}
