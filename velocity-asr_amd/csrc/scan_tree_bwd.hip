// Backward pass of the default tree scan (modes 0 / 2, scan_mode="parallel"; include/vasr.h):
//   vasr_ssm_tree_bwd_f32   d loss / d out -> the gradients of x, dt, z, B, C and per-(utterance,
//                           channel) partial sums of those of A and D.
//
// The function ("Backward of the tree scan").  Per (utterance, channel d, state n), with
// a_t = exp(dt_t A_n), b_t = x_t dt_t B_t[n], P_e = prod_{r <= e} a_r, and for an aligned block S of
// 2^k steps R_S = its local inclusive scan (restarting at its first step):
//   h_t = sum over the set bits k of t of P_{e_S} R_S,  S = [t with bits 0..k cleared, + 2^k),
// so only left children S of the tree contribute, each the same scalar V_S = P_{e_S} R_S to every
// step of its right sibling.  With gh_t = gy_t C_t[n]:
//   w_S = P_{e_S} sum_{t in sibling(S)} gh_t,   lambda_S(s) = w_S prod_{s < r <= e_S} a_r,
//   d/db_s      = sum_{left S containing s} lambda_S(s),
//   d/d(dt A)_r = sum_{left S : e_S >= r} w_S R_S + sum_{left S containing r} lambda_S(r - 1) rho^S_{r-1},
// rho^S_r the local scan of S up to r.  Nothing divides by a_r (it underflows to 0).
//
// Decomposition: time in 16-step chunks, padded with the identity (a, b) = (1, 0).  With the chunk
// composites alpha_c = prod a, beta_c = the chunk's local scan end and Pi_c = prod_{c' < c} alpha_c',
//   h_{16 c + i} = H_c + Pi_c inner_c(i),
// H the same tree function of the composites, inner_c the tree over the chunk's own 16 steps.  Four
// launches, none of which forms a (B, L, Di, N) array (7 floats per chunk, state and channel):
//   1. tree_bwd_chunk_kernel  per (utterance, chunk, channel block): alpha, beta, G_c = sum_i gh,
//                             J_c = sum_i gh inner_c(i);
//   2. tree_bwd_outer_kernel  per (utterance, channel, state) lane, level by level over the <= 512
//                             composites: H_c, Pi_c and the adjoints of beta_c and log alpha_c (the
//                             outer tree's with upstream G, plus sum_{c' > c} Pi_c' J_c'); up to
//                             32 composites (L <= 512) the lane's columns live in registers
//                             (tree_bwd_outer_reg_kernel), beyond that in the workspace;
//   3. tree_bwd_inner_kernel  per (utterance, chunk), looping over the channel blocks: the inner tree
//                             forwards (h for dC and dz, the local scans and products kept in
//                             registers) and backwards (one lambda register per level, level 4 the
//                             composite beta's), giving dx, ddt, dz and the chunk's rows of dB and dC;
//   4. tree_bwd_sum_kernel    the per-chunk partials of dA and dD summed over the chunks in order.
//
// Lane layout: scan_bwd.hip's.  A workgroup holds DPB = 1024 / N channels; G = N / 4 lanes share a
// channel and own 4 state indices each.  Reductions, all in a fixed order (no atomics):
//   sum_n  DPP butterfly over the channel's G lanes (group_sum);
//   sum_d  (dB, dC) lane-xor butterfly over the wave's channels, the four waves' rows summed 0..3
//          from an LDS tile every 8 steps into per-thread accumulators that run over the channel
//          blocks 0 .. Di / DPB - 1 in index order: the workgroup writes the final rows itself.
// Contraction is off for scan*.hip; nothing here relies on a fused multiply-add.  Modes 0 and 2
// differ only in the forward's rounding: one backward serves both.
#include <type_traits>

#include "scan_kernels.h"

// outer_tree's loops carry `#pragma unroll` for its register instance (compile-time M); its
// workspace instance has a run-time M, where the request cannot be met and is not needed
#pragma clang diagnostic ignored "-Wpass-failed"

namespace vasr {
namespace {

constexpr int TFB = 8;  // steps per flush of the cross-wave dB / dC tile
// workspace slots of B nch Di N floats each; (after the outer kernel) [after the inner kernel]
enum Slot { S_ALPHA = 0 /* (Pi) */, S_BETA, S_G /* [dA partial] */, S_J /* (d log alpha) */, S_DBETA, S_LOCAL,
            S_H /* scratch, (H) */, NSLOT };

template <int I, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < E) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, E>(f);
    }
}
template <int I, int E, class F>  // E - 1 down to I
__device__ __forceinline__ void static_rfor(F&& f) {
    if constexpr (I < E) {
        f(std::integral_constant<int, E - 1>{});
        static_rfor<I, E - 1>(f);
    }
}

// The local scan of level k at step i restarts at i with its low k bits cleared; levels whose
// restart coincides hold the same value, kept once at the lowest such level.
constexpr int canon(int k, int i) {
    for (int q = 0; q < k; ++q)
        if (((i >> q) << q) == ((i >> k) << k)) return q;
    return k;
}

constexpr int dpb4(int N) { return NW * (64 / (N / 4)); }  // channels per workgroup
bool state_dim_ok(int N) { return N == 16 || N == 32 || N == 64 || N == 128; }

// Stage a chunk's x, dt, gy = g silu(z), the dz factor g sigma (1 + z (1 - sigma)), B and C rows in
// LDS; rows past the utterance's end are zeros: a = exp(0) = 1 and b = 0, the identity, gh = 0.
template <int N, bool GATE>
__device__ __forceinline__ void stage_chunk(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ z,
                                            int64_t ld_z, const float* __restrict__ dt, int64_t ld_dt,
                                            const float* __restrict__ bc, int64_t ld_bc,
                                            const float* __restrict__ gout, int64_t ld_g, int64_t row0, int nvalid,
                                            int d0, int tid, float* xs, float* dts, float* gys, float* dzc, float* bs,
                                            float* cs) {
#pragma clang fp contract(off)
    constexpr int DPB = dpb4(N);
    for (int idx = tid; idx < T * DPB; idx += 64 * NW) {
        const int t = idx / DPB, d = idx - t * DPB;
        float xv = 0.0f, dv = 0.0f, gy = 0.0f, zc = 0.0f;
        if (t < nvalid) {
            const int64_t row = row0 + t;
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
    for (int idx = tid; idx < T * N; idx += 64 * NW) {
        const int t = idx / N, n = idx - t * N;
        float bv = 0.0f, cv = 0.0f;
        if (t < nvalid) {
            const float* r = bc + (row0 + t) * ld_bc;
            bv = r[n];
            cv = r[N + n];
        }
        bs[idx] = bv;
        cs[idx] = cv;
    }
}

// One step of the five local scans r[k] (level k restarts where i is a multiple of 2^k; r[0] = b).
template <int I>
__device__ __forceinline__ void scan_step(float (&r)[5], float a, float b) {
#pragma clang fp contract(off)
    r[0] = b;
    static_for<1, 5>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        if constexpr (I % (1 << k) == 0) r[k] = b;
        else r[k] = a * r[k] + b;
    });
}

// inner(i): the sum over the set bits k of i of the latest V at level k
template <int I>
__device__ __forceinline__ float inner_of(const float (&V)[4]) {
    float s = 0.0f;
    static_for<0, 4>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        if constexpr ((I >> k) & 1) s += V[k];
    });
    return s;
}

// ---------------------------------------------------------------- 1: the chunk composites
template <int N, bool GATE>
__global__ __launch_bounds__(256) void tree_bwd_chunk_kernel(
    const float* __restrict__ x, int64_t ld_x, const float* __restrict__ z, int64_t ld_z,
    const float* __restrict__ dt, int64_t ld_dt, const float* __restrict__ bc, int64_t ld_bc,
    const float* __restrict__ A2g, const float* __restrict__ gout, int64_t ld_g, float* __restrict__ ws, int B, int L,
    int Di) {
#pragma clang fp contract(off)
    constexpr int G = N / 4, DPW = 64 / G, DPB = NW * DPW;
    __shared__ float xs[T * DPB], dts[T * DPB], gys[T * DPB], dzc[T * DPB];
    __shared__ __attribute__((aligned(16))) float bs[T * N], cs[T * N];
    const int nd = Di / DPB, nch = (L + T - 1) / T;
    const int blk = blockIdx.x % nd;
    const int bcix = blockIdx.x / nd;  // b nch + c
    const int b = bcix / nch, c = bcix - b * nch;
    const int d0 = blk * DPB, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane % G, dl = wave * DPW + lane / G;
    const int nvalid = min(T, L - c * T);
    stage_chunk<N, GATE>(x, ld_x, z, ld_z, dt, ld_dt, bc, ld_bc, gout, ld_g, (int64_t)b * L + c * T, nvalid, d0, tid, xs,
                         dts, gys, dzc, bs, cs);
    __syncthreads();
    float A2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) A2[j] = A2g[g * 4 + j];
    float p[4], r[4][5], V[4][4], Gs[4], Js[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        p[j] = 1.0f;
        Gs[j] = 0.0f;
        Js[j] = 0.0f;
    }
    static_for<0, T>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const float xv = xs[i * DPB + dl], dv = dts[i * DPB + dl], gy = gys[i * DPB + dl];
        const float4 bv = *reinterpret_cast<const float4*>(bs + i * N + g * 4);
        const float4 cv = *reinterpret_cast<const float4*>(cs + i * N + g * 4);
        const float Bn[4] = {bv.x, bv.y, bv.z, bv.w}, Cn[4] = {cv.x, cv.y, cv.z, cv.w};
        const float xdt = dv * xv;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = __builtin_amdgcn_exp2f(dv * A2[j]);
            p[j] = p[j] * a;
            scan_step<i>(r[j], a, xdt * Bn[j]);
            const float gh = gy * Cn[j];
            Gs[j] += gh;
            Js[j] += gh * inner_of<i>(V[j]);
            constexpr int kk = ctz_c(i + 1);
            if constexpr (kk < 4) V[j][kk] = p[j] * r[j][kk];
        }
    });
    const int64_t S1 = (int64_t)B * nch * Di * N;
    float* o = ws + ((int64_t)bcix * Di + d0 + dl) * N + g * 4;
    *reinterpret_cast<float4*>(o + S_ALPHA * S1) = make_float4(p[0], p[1], p[2], p[3]);
    *reinterpret_cast<float4*>(o + S_BETA * S1) = make_float4(r[0][4], r[1][4], r[2][4], r[3][4]);
    *reinterpret_cast<float4*>(o + S_G * S1) = make_float4(Gs[0], Gs[1], Gs[2], Gs[3]);
    *reinterpret_cast<float4*>(o + S_J * S1) = make_float4(Js[0], Js[1], Js[2], Js[3]);
}

// ---------------------------------------------------------------- 2: the outer tree, one lane per thread
// The tree function and its gradient on the M = nch composites of one (utterance, channel, state),
// level by level.  In: alpha (al), beta (be), G (gg), J (jk).  Out: Pi (over al), H (hh), d beta (db),
// and d log alpha (over jk) = the outer tree's + sum_{c' > c} Pi_c' J_c'; lt: scratch.  Arr: the
// lane's column of each workspace slot (Strided), or registers (float[MC], MC = M at compile time:
// every loop unrolls and every index is a constant).
struct Strided {
    float* p;
    int64_t s;
    __device__ __forceinline__ float& operator[](int c) const { return p[c * s]; }
};

template <int MC, class Arr>
__device__ __forceinline__ void outer_tree(Arr& al, Arr& be, Arr& gg, Arr& jk, Arr& db, Arr& lt, Arr& hh, int Mrt) {
#pragma clang fp contract(off)
    const int M = MC > 0 ? MC : Mrt;
    // jk[c] <- what every r <= c receives: Pi_{c+1} J_{c+1}, later + w_S R_S of the left block ending at c
    float p = 1.0f;
#pragma unroll
    for (int c = 0; c < M; ++c) {
        if (c > 0) jk[c - 1] = p * jk[c];
        p = p * al[c];
        db[c] = 0.0f;
        lt[c] = 0.0f;
    }
    jk[M - 1] = 0.0f;
    // gradient, level k: left blocks S = [base, base + 2^k) whose sibling is not empty (hh: rho^S)
#pragma unroll
    for (int k = 0; k < 9; ++k) {  // M <= 512
        const int len = 1 << k;
        if (len >= M) break;
        float P = 1.0f;  // prod of alpha over [0, pos)
        int pos = 0;
#pragma unroll
        for (int base = 0; base + len < M; base += 2 * len) {
#pragma unroll
            for (; pos < base; ++pos) P = P * al[pos];
            float rho = 0.0f;
#pragma unroll
            for (; pos < base + len; ++pos) {
                const float a = al[pos];
                rho = a * rho + be[pos];
                P = P * a;
                hh[pos] = rho;
            }
            const int e = base + len - 1, hi = min(base + 2 * len, M);
            float sg = 0.0f;
#pragma unroll
            for (int c = e + 1; c < hi; ++c) sg += gg[c];
            const float w = P * sg;
            jk[e] += w * rho;
            float lam = w;
#pragma unroll
            for (int s = e; s >= base; --s) {
                db[s] += lam;
                if (s > base) {
                    lam = al[s] * lam;
                    lt[s] += lam * hh[s - 1];
                }
            }
        }
    }
    float run = 0.0f;
#pragma unroll
    for (int c = M - 1; c >= 0; --c) {
        run += jk[c];
        jk[c] = run + lt[c];
    }
    // H_c: V_S = P_{e_S} R_S added to every c of S's sibling, levels ascending
#pragma unroll
    for (int c = 0; c < M; ++c) hh[c] = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int len = 1 << k;
        if (len >= M) break;
        float P = 1.0f;
        int pos = 0;
#pragma unroll
        for (int base = 0; base + len < M; base += 2 * len) {
#pragma unroll
            for (; pos < base; ++pos) P = P * al[pos];
            float rho = 0.0f;
#pragma unroll
            for (; pos < base + len; ++pos) {
                const float a = al[pos];
                rho = a * rho + be[pos];
                P = P * a;
            }
            const float V = P * rho;
            const int hi = min(base + 2 * len, M);
#pragma unroll
            for (int c = base + len; c < hi; ++c) hh[c] += V;
        }
    }
    p = 1.0f;
#pragma unroll
    for (int c = 0; c < M; ++c) {
        const float a = al[c];
        al[c] = p;
        p = p * a;
    }
}

// Any M <= 512: the lane's columns stay in the workspace.
__global__ __launch_bounds__(256) void tree_bwd_outer_kernel(float* ws, int B, int M, int64_t DN) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)B * DN) return;
    const int64_t b = idx / DN, S1 = (int64_t)B * M * DN;
    float* q = ws + b * M * DN + (idx - b * DN);
    Strided al{q, DN}, be{q + S_BETA * S1, DN}, gg{q + S_G * S1, DN}, jk{q + S_J * S1, DN}, db{q + S_DBETA * S1, DN},
        lt{q + S_LOCAL * S1, DN}, hh{q + S_H * S1, DN};
    outer_tree<0>(al, be, gg, jk, db, lt, hh, M);
}

// M <= MP (L <= 16 MP): the columns in registers, padded to MP composites with the identity
// (alpha, beta) = (1, 0) and G = J = 0 -- the tree is causal, and a block whose sibling is all padding
// adds exact zeros.  Each workspace element is read once and written once.
constexpr int OUTER_REG = 32;
template <int MP>
__global__ __launch_bounds__(256) void tree_bwd_outer_reg_kernel(float* ws, int B, int M, int64_t DN) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)B * DN) return;
    const int64_t b = idx / DN, S1 = (int64_t)B * M * DN;
    float* q = ws + b * M * DN + (idx - b * DN);
    float al[MP], be[MP], gg[MP], jk[MP], db[MP], lt[MP], hh[MP];
#pragma unroll
    for (int c = 0; c < MP; ++c) {
        const bool in = c < M;
        al[c] = in ? q[c * DN] : 1.0f;
        be[c] = in ? q[S_BETA * S1 + c * DN] : 0.0f;
        gg[c] = in ? q[S_G * S1 + c * DN] : 0.0f;
        jk[c] = in ? q[S_J * S1 + c * DN] : 0.0f;
    }
    outer_tree<MP>(al, be, gg, jk, db, lt, hh, MP);
#pragma unroll
    for (int c = 0; c < MP; ++c) {
        if (c < M) {
            q[c * DN] = al[c];
            q[S_H * S1 + c * DN] = hh[c];
            q[S_DBETA * S1 + c * DN] = db[c];
            q[S_J * S1 + c * DN] = jk[c];
        }
    }
}

// ---------------------------------------------------------------- 3: the inner tree, both ways
// Sum v over the wave's channels and leave the wave's row of step `slot` in the tile.
template <int N>
__device__ __forceinline__ void put_row(float (&v)[4], int slot, int wave, int lane, int g, float* red) {
    constexpr int G = N / 4;
#pragma unroll
    for (int off = G; off < 64; off <<= 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] += __shfl_xor(v[j], off, 64);
    }
    if (lane < G)
        *reinterpret_cast<float4*>(red + (wave * TFB + slot) * N + g * 4) = make_float4(v[0], v[1], v[2], v[3]);
}

// The tile's TFB rows, waves summed 0..3, added to the thread's accumulators (element tid + 256 m).
template <int N, int NA>
__device__ __forceinline__ void drain(float (&acc)[NA], const float* red, int tid) {
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NA; ++m) {
        const int idx = tid + m * 256;
        if (idx < TFB * N) {
            float s = red[idx];
#pragma unroll
            for (int w = 1; w < NW; ++w) s += red[w * TFB * N + idx];
            acc[m] += s;
        }
    }
    __syncthreads();
}

// Two waves per SIMD: left to itself the kernel takes 266 - 272 registers, one wave per SIMD, and the
// launch at B 32, L 501, Di 384, N 64 1363 us; capped at 256 (8 - 35 registers spilled) 874 us.
template <int N, bool GATE>
__global__ __launch_bounds__(256, 2) void tree_bwd_inner_kernel(
    const float* __restrict__ x, int64_t ld_x, const float* __restrict__ z, int64_t ld_z,
    const float* __restrict__ dt, int64_t ld_dt, const float* __restrict__ bc, int64_t ld_bc,
    const float* __restrict__ Ag, const float* __restrict__ A2g, const float* __restrict__ Dg,
    const float* __restrict__ gout, int64_t ld_g, float* ws, float* __restrict__ dx, float* __restrict__ ddt,
    float* __restrict__ dz, float* __restrict__ dB, float* __restrict__ dC, int B, int L, int Di) {
#pragma clang fp contract(off)
    constexpr int G = N / 4, DPW = 64 / G, DPB = NW * DPW;
    constexpr int NA = (TFB * N + 255) / 256;  // dB / dC tile elements per thread
    __shared__ float xs[T * DPB], dts[T * DPB], gys[T * DPB], dzc[T * DPB];
    __shared__ __attribute__((aligned(16))) float bs[T * N], cs[T * N];
    __shared__ float o_dx[T * DPB], o_ddt[T * DPB], o_dz[T * DPB];
    __shared__ __attribute__((aligned(16))) float red[NW * TFB * N];

    const int nd = Di / DPB, nch = (L + T - 1) / T;
    const int bcix = blockIdx.x;  // b nch + c
    const int b = bcix / nch, c = bcix - b * nch;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane % G, dl = wave * DPW + lane / G;
    const int nvalid = min(T, L - c * T);
    const int64_t row0 = (int64_t)b * L + c * T;
    const int64_t S1 = (int64_t)B * nch * Di * N;
    float* dDws = ws + NSLOT * S1;

    float A2[4], Av[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        A2[j] = A2g[g * 4 + j];
        Av[j] = Ag[g * 4 + j];
    }
    float accB[2][NA], accC[2][NA];
#pragma unroll
    for (int m = 0; m < NA; ++m) accB[0][m] = accB[1][m] = accC[0][m] = accC[1][m] = 0.0f;

    for (int blk = 0; blk < nd; ++blk) {
        const int d0 = blk * DPB;
        stage_chunk<N, GATE>(x, ld_x, z, ld_z, dt, ld_dt, bc, ld_bc, gout, ld_g, row0, nvalid, d0, tid, xs, dts, gys, dzc,
                             bs, cs);
        __syncthreads();
        float* o = ws + ((int64_t)bcix * Di + d0 + dl) * N + g * 4;
        const float4 q0 = *reinterpret_cast<const float4*>(o + S_ALPHA * S1);
        const float4 q1 = *reinterpret_cast<const float4*>(o + S_H * S1);
        const float4 q2 = *reinterpret_cast<const float4*>(o + S_DBETA * S1);
        const float4 q3 = *reinterpret_cast<const float4*>(o + S_J * S1);
        const float Pi[4] = {q0.x, q0.y, q0.z, q0.w}, Hc[4] = {q1.x, q1.y, q1.z, q1.w};
        const float dbe[4] = {q2.x, q2.y, q2.z, q2.w}, dla[4] = {q3.x, q3.y, q3.z, q3.w};
        const float Dd = Dg[d0 + dl];

        // forwards: h for dC and dz; the products p_i and the local scans the way back needs
        float p[4], r[4][5], V[4][4];
        float Ps[T][4], RH[5][T][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = 1.0f;
        static_for<0, T>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            const float xv = xs[i * DPB + dl], dv = dts[i * DPB + dl], gy = gys[i * DPB + dl];
            const float4 bv = *reinterpret_cast<const float4*>(bs + i * N + g * 4);
            const float4 cv = *reinterpret_cast<const float4*>(cs + i * N + g * 4);
            const float Bn[4] = {bv.x, bv.y, bv.z, bv.w}, Cn[4] = {cv.x, cv.y, cv.z, cv.w};
            const float xdt = dv * xv;
            float dCv[4], yp = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float a = __builtin_amdgcn_exp2f(dv * A2[j]);
                p[j] = p[j] * a;
                Ps[i][j] = p[j];
                scan_step<i>(r[j], a, xdt * Bn[j]);
                static_for<0, 5>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    if constexpr (canon(k, i) == k) RH[k][i][j] = r[j][k];
                });
                const float h = Hc[j] + Pi[j] * inner_of<i>(V[j]);
                dCv[j] = gy * h;
                yp += h * Cn[j];
                constexpr int kk = ctz_c(i + 1);
                if constexpr (kk < 4) V[j][kk] = p[j] * r[j][kk];
            }
            if constexpr (GATE) {
                const float ys = group_sum<G>(yp);
                if (g == 0) o_dz[i * DPB + dl] = dzc[i * DPB + dl] * (ys + xv * Dd);
            }
            put_row<N>(dCv, i % TFB, wave, lane, g, red);
            if constexpr (i % TFB == TFB - 1) drain<N, NA>(accC[i / TFB], red, tid);
        });

        // backwards: lam[k] = lambda of the level-k left block around the step (level 4: the
        // composite beta's, from d beta), Sf[k] = sum of gh over the aligned 2^k steps last completed
        float lam[4][5], Sf[4][4], Q[4], dAc[4], dDc = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lam[j][4] = dbe[j];
            Q[j] = 0.0f;
            dAc[j] = 0.0f;
        }
        static_rfor<0, T>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            const float xv = xs[i * DPB + dl], dv = dts[i * DPB + dl], gy = gys[i * DPB + dl];
            const float4 bv = *reinterpret_cast<const float4*>(bs + i * N + g * 4);
            const float4 cv = *reinterpret_cast<const float4*>(cs + i * N + g * 4);
            const float Bn[4] = {bv.x, bv.y, bv.z, bv.w}, Cn[4] = {cv.x, cv.y, cv.z, cv.w};
            const float xdt = dv * xv;
            float dBv[4], s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float a = __builtin_amdgcn_exp2f(dv * A2[j]);
                const float gh = Pi[j] * (gy * Cn[j]);
                if constexpr (i < T - 1) {  // the left block ending here starts its lambda
                    constexpr int kk = ctz_c(i + 1);
                    const float w = Ps[i][j] * Sf[j][kk];
                    lam[j][kk] = w;
                    float R;
                    if constexpr (kk == 0) R = xdt * Bn[j];
                    else R = RH[canon(kk, i)][i][j];
                    Q[j] += w * R;
                }
                if constexpr (i >= 1) {  // the aligned block of 2^ctz(i) steps that starts here is complete
                    float tot = gh;
                    static_for<0, ctz_c(i)>([&](auto mc) { tot += Sf[j][decltype(mc)::value]; });
                    Sf[j][ctz_c(i)] = tot;
                }
                float gb = 0.0f, dd = Q[j] + dla[j];
                static_for<0, 5>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    if constexpr (k == 4 || !((i >> k) & 1)) {
                        gb += lam[j][k];
                        const float al = a * lam[j][k];  // lambda(i - 1)
                        if constexpr (i % (1 << k) != 0) dd += al * RH[canon(k, i - 1)][i - 1][j];
                        lam[j][k] = al;
                    }
                });
                dBv[j] = gb * xdt;
                s1 += gb * Bn[j];
                s2 += dd * Av[j];
                dAc[j] += dd * dv;
            }
            const float s1s = group_sum<G>(s1);
            const float s2s = group_sum<G>(s2);
            dDc += gy * xv;
            if (g == 0) {
                o_dx[i * DPB + dl] = gy * Dd + dv * s1s;
                o_ddt[i * DPB + dl] = xv * s1s + s2s;
            }
            put_row<N>(dBv, i % TFB, wave, lane, g, red);
            if constexpr (i % TFB == 0) drain<N, NA>(accB[i / TFB], red, tid);
        });
        // the chunk's dx, ddt, dz rows, coalesced along d (visible: the barriers of the last drain)
        for (int idx = tid; idx < T * DPB; idx += 64 * NW) {
            const int t = idx / DPB, d = idx - t * DPB;
            if (t < nvalid) {
                const int64_t oo = (row0 + t) * Di + d0 + d;
                dx[oo] = o_dx[idx];
                ddt[oo] = o_ddt[idx];
                if constexpr (GATE) dz[oo] = o_dz[idx];
            }
        }
        // the chunk's share of dA and dD (S_G is free: the outer kernel was its last reader)
        *reinterpret_cast<float4*>(o + S_G * S1) = make_float4(dAc[0], dAc[1], dAc[2], dAc[3]);
        if (g == 0) dDws[(int64_t)bcix * Di + d0 + dl] = dDc;
        __syncthreads();  // staging and output tiles are free for the next channel block
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int m = 0; m < NA; ++m) {
            const int idx = tid + m * 256;
            const int tt = idx / N, n = idx - tt * N, t = half * TFB + tt;
            if (idx < TFB * N && t < nvalid) {
                dB[(row0 + t) * N + n] = accB[half][m];
                dC[(row0 + t) * N + n] = accC[half][m];
            }
        }
    }
}

// ---------------------------------------------------------------- 4: dA and dD partials over the chunks
__global__ __launch_bounds__(256) void tree_bwd_sum_kernel(const float* __restrict__ ws, float* __restrict__ dApart,
                                                           float* __restrict__ dDpart, int B, int M, int Di, int N) {
#pragma clang fp contract(off)
    const int64_t DN = (int64_t)Di * N, S1 = (int64_t)B * M * DN;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)B * DN) return;
    const int64_t b = idx / DN, r = idx - b * DN;
    const float* pa = ws + S_G * S1 + b * M * DN + r;
    float s = pa[0];
    for (int c = 1; c < M; ++c) s += pa[c * DN];
    dApart[idx] = s;
    if (r % N == 0) {
        const int64_t d = r / N;
        const float* pd = ws + NSLOT * S1 + b * M * Di + d;
        float sd = pd[0];
        for (int c = 1; c < M; ++c) sd += pd[(int64_t)c * Di];
        dDpart[b * Di + d] = sd;
    }
}

template <int N>
int launch_tree_bwd(const float* x, int64_t ld_x, const float* z, int64_t ld_z, const float* dt, int64_t ld_dt,
                    const float* bc, int64_t ld_bc, const float* A, const float* A2, const float* D, const float* g,
                    int64_t ld_g, float* dx, float* ddt, float* dz, float* dB, float* dC, float* dApart, float* dDpart,
                    float* ws, int B, int L, int Di, hipStream_t s) {
    const char* what = "vasr_ssm_tree_bwd_f32";
    const int nd = Di / dpb4(N), nch = (L + T - 1) / T;
    const dim3 block(64 * NW), lanes((unsigned)(((int64_t)B * Di * N + 255) / 256));
    if (z)
        hipLaunchKernelGGL((tree_bwd_chunk_kernel<N, true>), dim3(B * nch * nd), block, 0, s, x, ld_x, z, ld_z, dt, ld_dt,
                           bc, ld_bc, A2, g, ld_g, ws, B, L, Di);
    else
        hipLaunchKernelGGL((tree_bwd_chunk_kernel<N, false>), dim3(B * nch * nd), block, 0, s, x, ld_x, z, ld_z, dt,
                           ld_dt, bc, ld_bc, A2, g, ld_g, ws, B, L, Di);
    int rc = launch_status(what);
    if (rc != VASR_OK) return rc;
    if (nch <= OUTER_REG)
        hipLaunchKernelGGL(tree_bwd_outer_reg_kernel<OUTER_REG>, lanes, dim3(256), 0, s, ws, B, nch, (int64_t)Di * N);
    else
        hipLaunchKernelGGL(tree_bwd_outer_kernel, lanes, dim3(256), 0, s, ws, B, nch, (int64_t)Di * N);
    rc = launch_status(what);
    if (rc != VASR_OK) return rc;
    if (z)
        hipLaunchKernelGGL((tree_bwd_inner_kernel<N, true>), dim3(B * nch), block, 0, s, x, ld_x, z, ld_z, dt, ld_dt, bc,
                           ld_bc, A, A2, D, g, ld_g, ws, dx, ddt, dz, dB, dC, B, L, Di);
    else
        hipLaunchKernelGGL((tree_bwd_inner_kernel<N, false>), dim3(B * nch), block, 0, s, x, ld_x, z, ld_z, dt, ld_dt, bc,
                           ld_bc, A, A2, D, g, ld_g, ws, dx, ddt, dz, dB, dC, B, L, Di);
    rc = launch_status(what);
    if (rc != VASR_OK) return rc;
    hipLaunchKernelGGL(tree_bwd_sum_kernel, lanes, dim3(256), 0, s, ws, dApart, dDpart, B, nch, Di, N);
    return launch_status(what);
}

}  // namespace
}  // namespace vasr

VASR_API int64_t vasr_ssm_tree_bwd_workspace_floats(int B, int L, int Di, int N) {
    if (B <= 0 || L <= 0 || Di <= 0 || !vasr::state_dim_ok(N)) return 0;
    // NSLOT floats per (chunk, channel, state) and the dD partial per (chunk, channel)
    return (int64_t)B * ((L + vasr::T - 1) / vasr::T) * Di * (vasr::NSLOT * N + 1);
}

VASR_API int vasr_ssm_tree_bwd_f32(const float* x, int64_t ld_x, const float* z, int64_t ld_z, const float* dt,
                                   int64_t ld_dt, const float* bc, int64_t ld_bc, const float* A, const float* A2,
                                   const float* D, const float* g, int64_t ld_g, float* dx, float* ddt, float* dz,
                                   float* dB, float* dC, float* dA_part, float* dD_part, float* workspace,
                                   int64_t workspace_floats, int B, int L, int Di, int N, void* stream) {
    using namespace vasr;
    VASR_CHECK_ARG(x && dt && bc && A && A2 && D && g && dx && ddt && dB && dC && dA_part && dD_part,
                   "vasr_ssm_tree_bwd_f32: null pointer");
    VASR_CHECK_ARG((z == nullptr) == (dz == nullptr), "vasr_ssm_tree_bwd_f32: z and dz go together (both or neither)");
    VASR_CHECK_ARG(B >= 0 && L >= 0 && L <= 8192 && Di > 0, "vasr_ssm_tree_bwd_f32: bad shape B=%d L=%d Di=%d", B, L, Di);
    VASR_CHECK_ARG(ld_x >= Di && ld_dt >= Di && ld_g >= Di && ld_bc >= 2 * N && (!z || ld_z >= Di),
                   "vasr_ssm_tree_bwd_f32: leading dims too small");
    if (!state_dim_ok(N)) {
        set_error("vasr_ssm_tree_bwd_f32: state dim N=%d not supported (16, 32, 64, 128; zero-pad B, C, A and A2)", N);
        return VASR_EUNSUPPORTED;
    }
    if (Di % dpb4(N) != 0) {
        set_error("vasr_ssm_tree_bwd_f32: Di=%d must be a multiple of %d for N=%d", Di, dpb4(N), N);
        return VASR_EUNSUPPORTED;
    }
    if (B == 0 || L == 0) return VASR_OK;
    const int64_t need = vasr_ssm_tree_bwd_workspace_floats(B, L, Di, N);
    VASR_CHECK_ARG(workspace != nullptr && workspace_floats >= need,
                   "vasr_ssm_tree_bwd_f32: workspace of %lld floats, %lld needed", (long long)workspace_floats,
                   (long long)need);
    VASR_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
                   "vasr_ssm_tree_bwd_f32: workspace must be 16-byte aligned");
    hipStream_t s = as_stream(stream);
#define VASR_TREE_BWD_N(NN)                                                                                          \
    launch_tree_bwd<NN>(x, ld_x, z, ld_z, dt, ld_dt, bc, ld_bc, A, A2, D, g, ld_g, dx, ddt, dz, dB, dC, dA_part, \
                        dD_part, workspace, B, L, Di, s)
    switch (N) {
        case 16: return VASR_TREE_BWD_N(16);
        case 32: return VASR_TREE_BWD_N(32);
        case 64: return VASR_TREE_BWD_N(64);
        default: return VASR_TREE_BWD_N(128);
    }
#undef VASR_TREE_BWD_N
}
