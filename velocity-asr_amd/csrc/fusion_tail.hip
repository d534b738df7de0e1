// The gated fusion of the global context and the CTC head's LayerNorm as ONE kernel
// (attention.py GatedFusion.forward_attention + model.py CTCOutputHead's norm):
//
//     t     = local w_local^T                      (B L, 384): [gate_l | local_proj] in 32-column pairs
//     g     = o w_glob^T                           (B L, 384): [gate_g | global_proj] (o Wo^T folded in)
//     gate  = sigmoid((t_gate + g_gate) + b_gate)
//     fused = gate (t_local + b_local) + (1 - gate) (g_glob + b_glob)
//     out   = fused Wo^T + bo                      (B L, 192)
//     y     = LayerNorm(out)
//
// The unfused form is three GEMM launches and a LayerNorm launch that write and re-read t (1536 B per
// token), fused and out (768 B each) through HBM.  Here one workgroup owns 32 or 64 token rows and keeps
// them on chip: local and o are staged once into LDS as their three bf16 planes, fused overwrites the
// planes of local as out_proj's A operand, out goes through an fp32 LDS scratch into the LayerNorm.
// HBM traffic per token: local in (768 B), o in (192 B), y out (768 B), out (768 B) only when asked for.
//
// Arithmetic: every product is the tile engine's (gemm_x3.hip) -- per 32 x 32 chunk, k-steps of 16 in
// ascending order, the six v_mfma_f32_32x32x16_bf16 split products small terms first, from a zero
// accumulator (o's K = 48 is three k-steps: the tile engine's fourth multiplies zero planes) -- the blend
// is VASR_EPI_PAIR_FUSION's float operations (gemm_common.h), the bias add and the LayerNorm those of
// the plain epilogue and of vasr_layer_norm_f32: y and out are bitwise the four launches'.
//
// Work decomposition: 6 waves per 32-row tile; wave w owns the chunk pair (2w, 2w + 1) of t and g, i.e.
// gate and branch of fused columns 32 w .. 32 w + 31, then chunk w of out.  t and g are formed
// transposed (operands exchanged: the same dot products in the same k order), so a lane holds 16
// columns of ONE token in four runs of four and fused leaves as one 8-B LDS store per run and plane.
// Weights go global -> VGPRs from vasr_split_weights_bf16x3's fragment layout, PD k-steps ahead; the 27
// k-steps (g 3, t 12, out 12) form one stream, so the prefetch runs across the phase boundaries.
#include "ssm_fused.h"

namespace vasr {
namespace {

using namespace fused;
typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int TA = 48;      // attention dim: the width of o
constexpr int OW = 64;      // o's planes are 64 wide in LDS (chunks 6, 7 never read)
constexpr int XLD = 200;    // row stride of the fp32 out scratch (rows 4 apart land 32 banks apart)
constexpr int NST = 27;     // g 3 k-steps, t 12, out 12
constexpr int SG = 3, ST = 15;

// weight prefetch distance in k-steps (tools/build_variant_lib.sh -DVASR_FT_PD32=<n>): 1, 2 and 3 measured
// within 0.2 us of each other in the 32-row form; 2 spills in the 64-row form
#ifndef VASR_FT_PD32
#define VASR_FT_PD32 2  // 32 rows, 6 waves
#endif
#ifndef VASR_FT_PD64
#define VASR_FT_PD64 1  // 64 rows, 12 waves (three per SIMD: 168 registers)
#endif

struct FusionParams {
    const float* local;
    int64_t ldl;
    const float* o;
    int64_t ldo;
    const uint16_t* wl;  // w_local (384 x 192) planes
    const uint16_t* wg;  // w_glob (384 x 48) planes, Kp = 64
    const float* bg;     // paired bias of g (384)
    const float* bl;     // local_proj bias (192)
    const uint16_t* wo;  // out_proj (192 x 192) planes
    const float* bo;
    const float* ln_w;
    const float* ln_b;
    float ln_eps;
    float* y;            // LayerNorm(out)
    int64_t ldy;
    float* out;          // optional
    int64_t ldout;
    int M;
};

// RT = 32-row tiles per workgroup
template <int RT>
struct FusionCtx {
    static constexpr int NWV = 6 * RT;
    static constexpr int ROWS = 32 * RT;
    static constexpr int PD = RT == 1 ? VASR_FT_PD32 : VASR_FT_PD64;
    static constexpr int RING = PD + 1;
    static constexpr int PL = ROWS * TD * 2;  // one plane of local / fused
    static constexpr int PO = ROWS * OW * 2;  // one plane of o
    const FusionParams& P;
    char* A;          // planes of local, then fused
    char* O;          // planes of o
    const float* sb;  // LDS: bg (384) | bl (192) | bo (192)
    float* xs;        // LDS: out rows, fp32
    int lane, w, row, zh, m0;  // row: this lane's token row of the workgroup (operand row / column)
    floatx16 g[2], t[2], oc;
    bf16x8 a[2][3];
    bf16x8 wf[RING][2][3];
};

template <int S, int RT>
__device__ __forceinline__ void load_w(FusionCtx<RT>& c) {
    constexpr int slot = S % FusionCtx<RT>::RING;
    if constexpr (S < ST) {
        const char* W = reinterpret_cast<const char*>(S < SG ? c.P.wg : c.P.wl);
        constexpr int KS = S < SG ? 4 : TD / 16, ks = S < SG ? S : S - SG;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                c.wf[slot][j][pl] = *reinterpret_cast<const bf16x8*>(
                    W + ((int64_t)((2 * c.w + j) * KS + ks) * 3 + pl) * 1024 + c.lane * 16);
    } else {
        const char* W = reinterpret_cast<const char*>(c.P.wo);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            c.wf[slot][0][pl] = *reinterpret_cast<const bf16x8*>(
                W + ((int64_t)(c.w * (TD / 16) + (S - ST)) * 3 + pl) * 1024 + c.lane * 16);
    }
}

template <int S, int RT>
__device__ __forceinline__ void load_first(FusionCtx<RT>& c) {
    load_w<S, RT>(c);
    if constexpr (S + 1 < FusionCtx<RT>::PD) load_first<S + 1, RT>(c);
}

// A fragment of k-step S: this lane's token row, k = 16 ks + 8 zh .. + 7, three planes
template <int S, int RT>
__device__ __forceinline__ void read_a(FusionCtx<RT>& c, bf16x8 (&a)[3]) {
    using Ctx = FusionCtx<RT>;
    if constexpr (S < SG) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            a[pl] = *reinterpret_cast<const bf16x8*>(c.O + pl * Ctx::PO + c.row * OW * 2 +
                                                     (((2 * S + c.zh) ^ ((c.row >> 1) & 7)) << 4));
    } else {
        constexpr int ks = S < ST ? S - SG : S - ST;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            a[pl] = *reinterpret_cast<const bf16x8*>(c.A + pl * Ctx::PL + c.row * TD * 2 +
                                                     (((2 * ks + c.zh) ^ (c.row & 7)) << 4));
    }
}

// fused = gate * lt + (1 - gate) * gt of four consecutive columns of one token, split into A's planes.
// VASR_EPI_PAIR_FUSION's operations one by one: the tile engine's epilogue multiplies and adds them
// unfused, and the split must see the rounded fp32 value the unfused path stores.
__device__ __forceinline__ void blend_store4(char* plane0, int plane_bytes, int off, const float (&tg)[4],
                                             const float (&tl)[4], const float (&gg)[4], const float (&gl)[4],
                                             const float4& bg, const float4& bgl, const float4& b2) {
#pragma clang fp contract(off)
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    const float bgv[4] = {bg.x, bg.y, bg.z, bg.w}, bglv[4] = {bgl.x, bgl.y, bgl.z, bgl.w};
    const float b2v[4] = {b2.x, b2.y, b2.z, b2.w};
    bf16x4 hi, mid, lo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float gp = (tg[i] + gg[i]) + bgv[i];
        const float lt = tl[i] + b2v[i];
        const float gt = gl[i] + bglv[i];
        const float gate = sigmoid_fast(gp);
        const float v = gate * lt + (1.0f - gate) * gt;
        hi[i] = (__bf16)v;
        const float r1 = v - (float)hi[i];
        mid[i] = (__bf16)r1;
        lo[i] = (__bf16)(r1 - (float)mid[i]);
    }
    *reinterpret_cast<bf16x4*>(plane0 + off) = hi;
    *reinterpret_cast<bf16x4*>(plane0 + plane_bytes + off) = mid;
    *reinterpret_cast<bf16x4*>(plane0 + 2 * plane_bytes + off) = lo;
}

// acc[j] += W_j (3 planes) x a (3 planes) with the operands exchanged (acc^T): the engine's six products,
// small terms first, then the leading hi * hi; the two chunks interleaved (independent accumulators)
__device__ __forceinline__ void mac_pair_t(floatx16 (&acc)[2], const bf16x8 (&w)[2][3], const bf16x8 (&a)[3]) {
    constexpr int pa[6] = {2, 0, 1, 1, 0, 0}, pw[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[j][pw[p]], a[pa[p]], acc[j], 0, 0, 0);
}

// acc += a x W, the same six products, token rows down the accumulator
__device__ __forceinline__ floatx16 mac_chunk(floatx16 acc, const bf16x8 (&a)[3], const bf16x8 (&w)[3]) {
    constexpr int pa[6] = {2, 0, 1, 1, 0, 0}, pw[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int p = 0; p < 6; ++p) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[pa[p]], w[pw[p]], acc, 0, 0, 0);
    return acc;
}

template <int S, int RT>
__device__ __forceinline__ void fusion_step(FusionCtx<RT>& c) {
    using Ctx = FusionCtx<RT>;
    constexpr int PD = Ctx::PD;
    if constexpr (S + PD < NST) load_w<S + PD, RT>(c);
    __builtin_amdgcn_sched_barrier(0);  // keep the prefetch where it is (ssm_tail.hip)
    // A fragments one step ahead of their MFMAs; steps 0 and ST start on an image completed by the
    // barrier just before them and read their own
    if constexpr (S == 0 || S == ST) read_a<S, RT>(c, c.a[S & 1]);
    if constexpr (S + 1 < NST && S + 1 != ST) read_a<S + 1, RT>(c, c.a[(S + 1) & 1]);
    __builtin_amdgcn_sched_barrier(0);
    const bf16x8(&a)[3] = c.a[S & 1];
    const bf16x8(&w)[2][3] = c.wf[S % Ctx::RING];
    if constexpr (S < SG) {
        mac_pair_t(c.g, w, a);
    } else if constexpr (S < ST) {
        if constexpr (S == SG) {
#pragma unroll
            for (int i = 0; i < 16; ++i) c.t[0][i] = c.t[1][i] = 0.f;
        }
        mac_pair_t(c.t, w, a);
    } else {
        if constexpr (S == ST) {
#pragma unroll
            for (int i = 0; i < 16; ++i) c.oc[i] = 0.f;
        }
        c.oc = mac_chunk(c.oc, a, w[0]);
    }

    if constexpr (S == ST - 1) {
        // every wave is past its last read of local's planes; fused takes their place.  Element i of
        // the transposed accumulators is pair column (i & 3) + 8 (i >> 2) + 4 zh of this lane's token.
        lds_barrier();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cc = 8 * j + 4 * c.zh;
            const float4 bg = *reinterpret_cast<const float4*>(c.sb + 64 * c.w + cc);
            const float4 bgl = *reinterpret_cast<const float4*>(c.sb + 64 * c.w + 32 + cc);
            const float4 b2 = *reinterpret_cast<const float4*>(c.sb + 2 * TD + 32 * c.w + cc);
            const float tg[4] = {c.t[0][4 * j], c.t[0][4 * j + 1], c.t[0][4 * j + 2], c.t[0][4 * j + 3]};
            const float tl[4] = {c.t[1][4 * j], c.t[1][4 * j + 1], c.t[1][4 * j + 2], c.t[1][4 * j + 3]};
            const float gg[4] = {c.g[0][4 * j], c.g[0][4 * j + 1], c.g[0][4 * j + 2], c.g[0][4 * j + 3]};
            const float gl[4] = {c.g[1][4 * j], c.g[1][4 * j + 1], c.g[1][4 * j + 2], c.g[1][4 * j + 3]};
            blend_store4(c.A, Ctx::PL, poff<TD>(c.row, 32 * c.w + cc), tg, tl, gg, gl, bg, bgl, b2);
        }
        lds_barrier();  // fused complete before out_proj reads it
    }
    if constexpr (S + 1 < NST) fusion_step<S + 1, RT>(c);
}

template <int RT>
__global__ __launch_bounds__(384 * RT, 1) void fusion_tail_kernel(FusionParams P) {
    using Ctx = FusionCtx<RT>;
    constexpr int NT = 64 * Ctx::NWV;
    __shared__ __attribute__((aligned(16))) char A[3 * Ctx::PL];
    __shared__ __attribute__((aligned(16))) char O[3 * Ctx::PO];
    __shared__ __attribute__((aligned(16))) float xs[Ctx::ROWS * XLD];
    __shared__ __attribute__((aligned(16))) float sb[4 * TD];
    Ctx c{P, A, O, sb, xs};
    c.lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    c.w = wave % 6;
    c.row = 32 * (wave / 6) + (c.lane & 31);
    c.zh = c.lane >> 5;
    c.m0 = blockIdx.x * Ctx::ROWS;
    load_first<0, RT>(c);
    __builtin_amdgcn_sched_barrier(0);
    // stage local (24 chunks of 8 floats a row) and o (6 chunks a row), each split once; rows past M
    // repeat row M - 1 and are never stored
    constexpr int UNITS = Ctx::ROWS * (TD / 8);
    static_assert(UNITS % NT == 0, "whole staging rounds");
#pragma unroll
    for (int k = 0; k < UNITS / NT; ++k) {
        const int u = threadIdx.x + NT * k;
        const int rr = u / (TD / 8), ch = u - rr * (TD / 8);
        const float* src = P.local + (int64_t)min(c.m0 + rr, P.M - 1) * P.ldl + 8 * ch;
        const float4 v0 = *reinterpret_cast<const float4*>(src);
        const float4 v1 = *reinterpret_cast<const float4*>(src + 4);
        split_store8<3>(A, Ctx::PL, rr * TD * 2 + ((ch ^ (rr & 7)) << 4), v0, v1);
    }
    if (threadIdx.x < Ctx::ROWS * (TA / 8)) {
        const int rr = threadIdx.x / (TA / 8), ch = threadIdx.x - rr * (TA / 8);
        const float* src = P.o + (int64_t)min(c.m0 + rr, P.M - 1) * P.ldo + 8 * ch;
        const float4 v0 = *reinterpret_cast<const float4*>(src);
        const float4 v1 = *reinterpret_cast<const float4*>(src + 4);
        split_store8<3>(O, Ctx::PO, rr * OW * 2 + ((ch ^ ((rr >> 1) & 7)) << 4), v0, v1);
    }
    for (int i = threadIdx.x; i < 4 * TD; i += NT)
        sb[i] = i < 2 * TD ? P.bg[i] : i < 3 * TD ? P.bl[i - 2 * TD] : P.bo[i - 3 * TD];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        c.g[0][i] = 0.f;
        c.g[1][i] = 0.f;
    }
    lds_barrier();  // planes and biases complete
    fusion_step<0, RT>(c);
    // out = fused Wo^T + bo: element i is row (i & 3) + 8 (i >> 2) + 4 zh of the tile, column 32 w + r
    // (the lane index afresh from mbcnt: nothing of the prologue's stays live across the steps)
    const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    {
        const int col = 32 * c.w + (ln & 31);
        const int r0 = 32 * (wave / 6) + 4 * (ln >> 5);
        const float bo = sb[3 * TD + col];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int rr = r0 + (i & 3) + 8 * (i >> 2);
            const float v = c.oc[i] + bo;
            xs[rr * XLD + col] = v;
            if (P.out && c.m0 + rr < P.M) P.out[(int64_t)(c.m0 + rr) * P.ldout + col] = v;
        }
    }
    lds_barrier();
    // y = LayerNorm(out): one wave per row, vasr_layer_norm_f32's operations (norm.hip ln_vals)
    float lw[3], lb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        lw[i] = P.ln_w[ln + 64 * i];
        lb[i] = P.ln_b[ln + 64 * i];
    }
    for (int rr = wave; rr < Ctx::ROWS && c.m0 + rr < P.M; rr += Ctx::NWV) {
        float v[3];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            v[i] = xs[rr * XLD + ln + 64 * i];
            s += v[i];
        }
        const float mean = wave_sum(s) / (float)TD;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float d = v[i] - mean;
            q = __builtin_fmaf(d, d, q);
        }
        const float var = wave_sum(q) / (float)TD;
        const float rstd = 1.0f / sqrtf(var + P.ln_eps);
        float* yr = P.y + (int64_t)(c.m0 + rr) * P.ldy;
#pragma unroll
        for (int i = 0; i < 3; ++i) yr[ln + 64 * i] = __builtin_fmaf((v[i] - mean) * rstd, lw[i], lb[i]);
    }
}

// Rows per workgroup: 64 (12 waves) while that still fills the CUs, 32 (6 waves) below
int fusion_rows(int M) { return M > 8192 ? 64 : 32; }

}  // namespace
}  // namespace vasr

VASR_API int vasr_fusion_tail_f32(const float* local, int64_t ldl, const float* o, int64_t ldo,
                                  const uint16_t* w_local, const uint16_t* w_glob, const float* b_glob,
                                  const float* b_local, const uint16_t* w_out, const float* b_out, const float* ln_w,
                                  const float* ln_b, float ln_eps, float* y, int64_t ldy, float* out, int64_t ldout,
                                  int M, int D, int A, int rows, void* stream) {
    using namespace vasr;
    VASR_CHECK_ARG(local && o && w_local && w_glob && b_glob && b_local && w_out && b_out && ln_w && ln_b && y,
                   "vasr_fusion_tail_f32: null pointer");
    VASR_CHECK_ARG(D == TD && A == TA, "vasr_fusion_tail_f32: built for d_model %d, attention dim %d (got %d, %d)", TD, TA,
                   D, A);
    VASR_CHECK_ARG(M >= 0 && ldl >= D && ldo >= A && ldy >= D && (!out || ldout >= D) && ldl % 4 == 0 && ldo % 4 == 0,
                   "vasr_fusion_tail_f32: bad shape M=%d ldl=%lld ldo=%lld ldy=%lld ldout=%lld", M, (long long)ldl,
                   (long long)ldo, (long long)ldy, (long long)ldout);
    VASR_CHECK_ARG(((reinterpret_cast<uintptr_t>(local) | reinterpret_cast<uintptr_t>(o) |
                     reinterpret_cast<uintptr_t>(w_local) | reinterpret_cast<uintptr_t>(w_glob) |
                     reinterpret_cast<uintptr_t>(w_out)) & 15) == 0,
                   "vasr_fusion_tail_f32: local, o and the weight planes must be 16-byte aligned");
    VASR_CHECK_ARG(rows == 0 || rows == 32 || rows == 64, "vasr_fusion_tail_f32: rows must be 0 (automatic), 32 or 64");
    if (M == 0) return VASR_OK;
    const FusionParams p{local, ldl, o, ldo, w_local, w_glob, b_glob, b_local, w_out, b_out, ln_w, ln_b, ln_eps,
                         y, ldy, out, ldout, M};
    const int r = rows ? rows : fusion_rows(M);
    const dim3 grid((unsigned)((M + r - 1) / r));
    if (r == 64) hipLaunchKernelGGL((fusion_tail_kernel<2>), grid, dim3(768), 0, as_stream(stream), p);
    else hipLaunchKernelGGL((fusion_tail_kernel<1>), grid, dim3(384), 0, as_stream(stream), p);
    return launch_status("vasr_fusion_tail_f32");
}
