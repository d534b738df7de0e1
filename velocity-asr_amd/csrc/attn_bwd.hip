// Backward of the global context's two non-GEMM kernels (attn.hip; include/vasr.h, "global context,
// backward"):
//   vasr_pooled_attention_bwd_f32   d loss / d out -> dq and [dK | dV] of out = softmax(q k^T / sqrt(hd)) v
//   vasr_adaptive_pool_bwd_f32      d loss / d pooled -> dx of the adaptive average pooling
//
// Attention.  Per (utterance, head), with s_k = q . k_k / sqrt(hd), p = softmax(s) over the
// utterance's Kb keys, dP_k = dout . v_k and delta = sum_k p_k dP_k (= dout . out):
//   dS_k = p_k (dP_k - delta),            dq   = sum_k dS_k k_k / sqrt(hd),
//   dK_k = sum_t dS_tk q_t / sqrt(hd),    dV_k = sum_t p_tk dout_t.
// The forward's p is recomputed from q and kv with the forward's own operations (the same fused
// dot products, s / sqrt(hd), expf(s - max)); nothing of the forward is kept.
//
// Mapping.  A workgroup is one wave and owns (a tile of TB = 64 tokens, one head, one utterance); the
// head's K and V columns sit in LDS.
//   1. Lane = token.  Three passes over the keys: s_k, dP_k and the maximum; e_k = exp(s_k - max), their
//      sum and sum_k e_k dP_k; then p_k, dS_k (both left in LDS, [key][token]) and dq, written by the lane
//      itself: dq needs no reduction.  The lane's q and dout rows go to LDS as well.
//   2. Lanes remapped to (key, column of [dK | dV]), four of them per lane at a time (independent
//      chains; the tile is latency bound): each sums the tile's tokens in token order into
//      the tile's partial (B, tiles, Kp, 2A) in the workspace -- or, when the utterance is one tile
//      (L <= 64), straight into dkv.
//   3. pooled_attention_bwd_sum_kernel (L > 64): lane = (utterance, key, column), the tiles' partials
//      added in tile order.
// No atomics; every sum runs in a fixed order that depends on nothing outside the utterance, so the
// gradients are run-to-run bitwise and an utterance's rows do not depend on the rest of the batch.
// Rows k >= kps[b] of dkv are written as 0 (stage 2 writes zeros there, stage 3 adds zeros).
//
// LDS per workgroup, floats: 2 Kp hd (K | V of the head) + 2 Kp (TB + 1) (dS, p) + TB (2 hd | 1)
// (q | dout): 16.6 KiB at the model's Kp 16, hd 12 and 64.75 KiB at the limits Kp 64, hd 32, for which
// the launcher raises the kernel's dynamic LDS limit.  The pads (TB + 1, 2 hd | 1) keep both stages'
// accesses on distinct banks.
#include "vasr_internal.h"

namespace vasr {
namespace {

constexpr int kMaxKeys = 64;
constexpr int kMaxHd = 32;
constexpr int kMaxA = 256;
constexpr int TB = 64;       // tokens per tile = lanes per workgroup
constexpr int PS = TB + 1;   // row stride of the dS / p tile
constexpr int IB = 4;        // (key, column) sums a lane carries at once in stage 2

__host__ __device__ constexpr int qd_stride(int hd) { return (2 * hd) | 1; }
size_t attn_bwd_lds(int Kp, int hd) {
    return sizeof(float) * ((size_t)2 * Kp * hd + (size_t)2 * Kp * PS + (size_t)TB * qd_stride(hd));
}

// grid (tiles, heads, B), block 64.  HD = head_dim at compile time (8, 12, 16), 0 = runtime
// head_dim <= kMaxHd with guarded loops, as the forward.  part: (B, tiles, Kp, 2A).
template <int HD>
__global__ __launch_bounds__(TB) void pooled_attention_bwd_kernel(const float* __restrict__ q, int64_t ld_q,
                                                                  const float* __restrict__ kv,
                                                                  const float* __restrict__ dout,
                                                                  float* __restrict__ dq, float* __restrict__ part,
                                                                  int L, int Kp, int heads, int hd_rt,
                                                                  const int32_t* __restrict__ kps) {
    constexpr int JM = HD ? HD : kMaxHd;
    const int hd = HD ? HD : hd_rt;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* kvs = lds;                    // [Kp][2 hd]: k_k | v_k of this head
    float* sp = kvs + 2 * Kp * hd;       // [Kp][2][PS]: dS_k | p_k of every token
    float* qd = sp + 2 * Kp * PS;        // [TB][QS]: q_t | dout_t of this head
    const int QS = qd_stride(hd);
    const int tile = blockIdx.x, hh = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
    const int A = heads * hd;
    const int t0 = tile * TB, nvalid = min(TB, L - t0);
    const bool live = lane < nvalid;
    const int64_t row = (int64_t)b * L + t0 + (live ? lane : 0);
    const float* qr = q + row * ld_q + hh * hd;
    const float* gr = dout + row * A + hh * hd;
    float qv[JM], gv[JM];
#pragma unroll
    for (int j = 0; j < JM; ++j) {
        qv[j] = (live && j < hd) ? qr[j] : 0.f;
        gv[j] = (live && j < hd) ? gr[j] : 0.f;
    }
    const int Kb = kps ? min(max(kps[b], 1), Kp) : Kp;
    const float* kvb = kv + (int64_t)b * Kp * 2 * A + hh * hd;
    for (int i = lane; i < Kp * 2 * hd; i += TB) {
        const int k = i / (2 * hd), r = i - k * 2 * hd;
        kvs[i] = kvb[(int64_t)k * 2 * A + (r < hd ? r : A + r - hd)];
    }
#pragma unroll
    for (int j = 0; j < JM; ++j)
        if (j < hd) {
            qd[lane * QS + j] = qv[j];
            qd[lane * QS + hd + j] = gv[j];
        }
    __syncthreads();

    // ---- 1: lane = token
    const float scale = sqrtf((float)hd);
    float mx = -INFINITY;
    for (int k = 0; k < Kb; ++k) {  // s_k and dP_k (two independent chains), kept in the lane's own column
        const float* kr = kvs + k * 2 * hd;
        const float* vr = kr + hd;
        float s = 0.f, dp = 0.f;
#pragma unroll
        for (int j = 0; j < JM; ++j)
            if (j < hd) {
                s = __builtin_fmaf(qv[j], kr[j], s);
                dp = __builtin_fmaf(gv[j], vr[j], dp);
            }
        s = s / scale;
        mx = fmaxf(mx, s);
        sp[(2 * k) * PS + lane] = dp;
        sp[(2 * k + 1) * PS + lane] = s;
    }
    float sum = 0.f, ed = 0.f;
    for (int k = 0; k < Kb; ++k) {
        const float e = expf(sp[(2 * k + 1) * PS + lane] - mx);
        sum += e;
        ed = __builtin_fmaf(e, sp[(2 * k) * PS + lane], ed);
        sp[(2 * k + 1) * PS + lane] = e;
    }
    const float inv = 1.0f / sum;
    const float delta = ed * inv;
    float acc[JM];
#pragma unroll
    for (int j = 0; j < JM; ++j) acc[j] = 0.f;
    for (int k = 0; k < Kb; ++k) {
        const float* kr = kvs + k * 2 * hd;
        const float p = sp[(2 * k + 1) * PS + lane] * inv;
        const float ds = p * (sp[(2 * k) * PS + lane] - delta);
        sp[(2 * k) * PS + lane] = ds;
        sp[(2 * k + 1) * PS + lane] = p;
#pragma unroll
        for (int j = 0; j < JM; ++j)
            if (j < hd) acc[j] = __builtin_fmaf(ds, kr[j], acc[j]);
    }
    if (live) {
        float* orow = dq + row * A + hh * hd;
#pragma unroll
        for (int j = 0; j < JM; ++j)
            if (j < hd) orow[j] = acc[j] / scale;
    }
    __syncthreads();

    // ---- 2: lane = (key, column of [dK | dV]); tokens in order
    float* pb = part + (((int64_t)b * gridDim.x + tile) * Kp) * 2 * A + hh * hd;
    const int n = Kp * 2 * hd;
    for (int i0 = lane; i0 < n; i0 += IB * TB) {  // IB items per lane at a time: independent chains
        const float* w[IB];
        const float* x[IB];
        float s[IB];
#pragma unroll
        for (int m = 0; m < IB; ++m) {
            const int i = min(i0 + m * TB, n - 1);
            const int k = i / (2 * hd), r = i - k * 2 * hd;
            w[m] = sp + (2 * (k < Kb ? k : 0) + (r >= hd ? 1 : 0)) * PS;  // (a dead key: row 0, result unused)
            x[m] = qd + r;
            s[m] = 0.f;
        }
        for (int t = 0; t < nvalid; ++t) {
#pragma unroll
            for (int m = 0; m < IB; ++m) s[m] = __builtin_fmaf(w[m][t], x[m][t * QS], s[m]);
        }
#pragma unroll
        for (int m = 0; m < IB; ++m) {
            const int i = i0 + m * TB;
            if (i < n) {
                const int k = i / (2 * hd), r = i - k * 2 * hd;
                const bool isv = r >= hd;
                pb[(int64_t)k * 2 * A + (isv ? A + r - hd : r)] = k < Kb ? (isv ? s[m] : s[m] / scale) : 0.f;
            }
        }
    }
}

// dkv[b][k][c] = sum over the tiles in order of part[b][tile][k][c]
__global__ __launch_bounds__(256) void pooled_attention_bwd_sum_kernel(const float* __restrict__ part,
                                                                       float* __restrict__ dkv, int B, int tiles,
                                                                       int64_t KA) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)B * KA) return;
    const int64_t b = idx / KA, r = idx - b * KA;
    const float* p = part + b * tiles * KA + r;
    float s = p[0];
    for (int i = 1; i < tiles; ++i) s += p[i * KA];
    dkv[idx] = s;
}

// One lane per dx element: the (at most two for K <= L) bins that hold row t, ascending.
__global__ __launch_bounds__(256) void adaptive_pool_bwd_kernel(const float* __restrict__ g, float* __restrict__ dx, int B,
                                                                int L, int C, int K, const int32_t* __restrict__ lens,
                                                                const int32_t* __restrict__ ks) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)B * L * C;
    if (idx >= total) return;
    const int c = idx % C;
    const int64_t bt = idx / C;
    const int t = bt % L;
    const int b = bt / L;
    const int Lb = lens ? min(max(lens[b], 1), L) : L;
    const int Kb = ks ? min(max(ks[b], 1), K) : K;
    if (t >= Lb) {
        dx[idx] = 0.f;
        return;
    }
    // floor(i Lb / Kb) <= t < ceil((i + 1) Lb / Kb)  <=>  floor(t Kb / Lb) <= i <= ceil((t + 1) Kb / Lb) - 1
    const int lo = (int)(((int64_t)t * Kb) / Lb);
    const int hi = min((int)((((int64_t)t + 1) * Kb - 1) / Lb), Kb - 1);
    const float* gb = g + ((int64_t)b * K) * C + c;
    float acc = 0.f;
    for (int i = lo; i <= hi; ++i) {
        const int s = (int)(((int64_t)i * Lb) / Kb);
        const int e = (int)(((int64_t)(i + 1) * Lb + Kb - 1) / Kb);
        acc += gb[(int64_t)i * C] / (float)(e - s);
    }
    dx[idx] = acc;
}

template <int HD>
int launch_attn_bwd(const float* q, int64_t ld_q, const float* kv, const float* dout, float* dq, float* part, int L,
                    int Kp, int heads, int hd, const int32_t* kps, dim3 grid, size_t lds, hipStream_t s,
                    const char* who) {
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&pooled_attention_bwd_kernel<HD>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            set_error("%s: %s", who, hipGetErrorString(e));
            return (int)e;
        }
    }
    hipLaunchKernelGGL(pooled_attention_bwd_kernel<HD>, grid, dim3(TB), lds, s, q, ld_q, kv, dout, dq, part, L, Kp,
                       heads, hd, kps);
    return launch_status(who);
}

}  // namespace
}  // namespace vasr

VASR_API int64_t vasr_pooled_attention_bwd_workspace_floats(int B, int L, int Kp, int heads, int head_dim) {
    if (B <= 0 || L <= vasr::TB || Kp <= 0 || heads <= 0 || head_dim <= 0) return 0;  // one tile: no partials
    return (int64_t)B * ((L + vasr::TB - 1) / vasr::TB) * Kp * 2 * heads * head_dim;
}

VASR_API int vasr_pooled_attention_bwd_f32(const float* q, int64_t ld_q, const float* kv, const float* dout, float* dq,
                                           float* dkv, float* workspace, int64_t workspace_floats, int B, int L, int Kp,
                                           int heads, int head_dim, const int32_t* kps, void* stream) {
    using namespace vasr;
    const char* who = "vasr_pooled_attention_bwd_f32";
    // (an empty batch has no kv / dkv, an empty utterance no q / dout / dq: their pointers may be null)
    VASR_CHECK_ARG((B <= 0 || (kv && dkv)) && (B <= 0 || L <= 0 || (q && dout && dq)), "%s: null pointer", who);
    VASR_CHECK_ARG(Kp >= 1 && Kp <= kMaxKeys && head_dim >= 1 && head_dim <= kMaxHd && heads >= 1 &&
                       heads * head_dim <= kMaxA && L >= 0 && B >= 0,
                   "%s: unsupported shape Kp=%d heads=%d head_dim=%d", who, Kp, heads, head_dim);
    const int A = heads * head_dim;
    VASR_CHECK_ARG(ld_q >= A, "%s: ld_q=%lld below heads*head_dim=%d", who, (long long)ld_q, A);
    VASR_CHECK_ARG((size_t)Kp * 2 * A * sizeof(float) <= 65536, "%s: K/V set exceeds 64 KiB of LDS", who);
    VASR_CHECK_ARG(A % 4 == 0 && (reinterpret_cast<uintptr_t>(kv) & 15) == 0,
                   "%s: heads*head_dim must be a multiple of 4 and kv 16-byte aligned", who);
    const int64_t need = vasr_pooled_attention_bwd_workspace_floats(B, L, Kp, heads, head_dim);
    VASR_CHECK_ARG(need == 0 || (workspace != nullptr && workspace_floats >= need),
                   "%s: workspace of %lld floats, %lld needed", who, (long long)workspace_floats, (long long)need);
    VASR_CHECK_ARG(B <= 65535, "%s: batch %d too large", who, B);
    if (B == 0) return VASR_OK;
    hipStream_t s = as_stream(stream);
    const int64_t KA = (int64_t)Kp * 2 * A;
    if (L == 0) {  // no tokens: the sums are empty
        const hipError_t e = hipMemsetAsync(dkv, 0, (size_t)B * KA * sizeof(float), s);
        if (e != hipSuccess) {
            set_error("%s: %s", who, hipGetErrorString(e));
            return (int)e;
        }
        return VASR_OK;
    }
    const int tiles = (L + TB - 1) / TB;
    const dim3 grid(tiles, heads, B);
    float* part = tiles == 1 ? dkv : workspace;
    const size_t lds = attn_bwd_lds(Kp, head_dim);
    int rc;
    switch (head_dim) {
        case 8: rc = launch_attn_bwd<8>(q, ld_q, kv, dout, dq, part, L, Kp, heads, 8, kps, grid, lds, s, who); break;
        case 12: rc = launch_attn_bwd<12>(q, ld_q, kv, dout, dq, part, L, Kp, heads, 12, kps, grid, lds, s, who); break;
        case 16: rc = launch_attn_bwd<16>(q, ld_q, kv, dout, dq, part, L, Kp, heads, 16, kps, grid, lds, s, who); break;
        default: rc = launch_attn_bwd<0>(q, ld_q, kv, dout, dq, part, L, Kp, heads, head_dim, kps, grid, lds, s, who);
    }
    if (rc != VASR_OK || tiles == 1) return rc;
    hipLaunchKernelGGL(pooled_attention_bwd_sum_kernel, dim3((unsigned)((B * KA + 255) / 256)), dim3(256), 0, s, workspace,
                       dkv, B, tiles, KA);
    return launch_status(who);
}

VASR_API int vasr_adaptive_pool_bwd_f32(const float* g, float* dx, int B, int L, int C, int K, const int32_t* lens,
                                        const int32_t* ks, void* stream) {
    using namespace vasr;
    const char* who = "vasr_adaptive_pool_bwd_f32";
    VASR_CHECK_ARG(g && dx, "%s: null pointer", who);
    VASR_CHECK_ARG(B >= 0 && L >= 1 && C >= 1 && K >= 1 && K <= L, "%s: need 1 <= K <= L (K=%d L=%d)", who, K, L);
    VASR_CHECK_ARG((lens == nullptr) == (ks == nullptr), "%s: lens and ks go together (both or neither)", who);
    if (B == 0) return VASR_OK;
    const int64_t total = (int64_t)B * L * C;
    hipLaunchKernelGGL(adaptive_pool_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), g,
                       dx, B, L, C, K, lens, ks);
    return launch_status(who);
}
