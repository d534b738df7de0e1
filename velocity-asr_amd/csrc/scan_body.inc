// Body of the selective-scan kernel for one lane layout, included by scan.hip once per
// NPL (state indices per lane, a constexpr of the including namespace): 4 = two packed pairs
// per lane (G = N/4 lanes per channel), 2 = one pair per lane (G = N/2: twice the waves for
// the same work, for launches too small to fill the SIMDs).  Everything in here is the same
// float arithmetic for either layout except the order of the y = sum_n h C partial sums.

constexpr int NP = NPL / 2;  // packed state pairs per lane
typedef float vecN __attribute__((ext_vector_type(NPL)));

template <int MAXUP, int LG = 4>
struct TreeState {
    f2 la[LG][NP], lb[LG][NP], ca[LG][NP], cb[LG][NP];  // in-chunk levels 0..LG-1
    f2 ula[MAXUP][NP], ulb[MAXUP][NP];              // chunk-level blocks
    f2 pa[NP], pb[NP];                              // prefix after the upper stack
};

struct Smem {
    const float* xs;
    const float* dts;
    const float* bcs;
    float* yp;  // per-channel partial sums y[t] = sum_n h C: [DPB][TP]
};

// Per-step operands of one lane, read from the staged chunk one step ahead of use.  In the
// fused-multiply-add mode (2) x holds the product x * dt (each lane forms it: round 3 formed it
// once per (step, channel) in a {dt, x * dt} LDS slab, whose chunk-0 values read back wrong for
// the last channel of a wave beside co-resident MFMA kernels of another stream -- the concurrent
// utterance-group race; profiles/r04g/).
struct StepIn {
    float x, dt;
    vecN bv, cv;
};

// BCS: float stride of the staged bc rows (2N: B | C; N: B only, the up-sweep of the time-split form)
template <int I, int N, int DPB, bool FMA = false, int BCS = 2 * N>
__device__ __forceinline__ StepIn load_step(const Smem& sm, int dl, int g) {
    StepIn in;
    if constexpr (FMA) {
        in.dt = sm.dts[I * DPB + dl];
        in.x = sm.xs[I * DPB + dl] * in.dt;  // x * dt, rounded once
    } else {
        in.x = sm.xs[I * DPB + dl];
        in.dt = sm.dts[I * DPB + dl];
    }
    if constexpr (VASR_SCAN_ABLATE & 4) {
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            in.bv[j] = j & 1 ? in.dt : in.x;
            in.cv[j] = j & 1 ? in.x : in.dt;
        }
    } else {
        in.bv = *reinterpret_cast<const vecN*>(sm.bcs + I * BCS + g * NPL);
        if constexpr (BCS == 2 * N) in.cv = *reinterpret_cast<const vecN*>(sm.bcs + I * BCS + N + g * NPL);
        else in.cv = in.bv;  // B-only rows: the up-sweep reads no C
    }
    return in;
}

// The state-independent part of a step: dA = exp2(dt A2), dBx = x (dt B), and C.
struct StepElem {
    f2 a[NP], b[NP];
    vecN cv;
};

// FMA (mode 2) forms x dt once per lane and scales B by it: one packed multiply per pair
// instead of two, rounded differently from the reference's x (dt B).
template <bool FMA>
__device__ __forceinline__ StepElem make_elem(const StepIn& in, const f2 (&A2)[NP]) {
#pragma clang fp contract(off)
    StepElem e;
    const f2 dt2 = {in.dt, in.dt};
    const f2 x2 = {in.x, in.x};
    const float xdt = in.x;  // FMA: x * dt (load_step)
    const f2 xdt2 = {xdt, xdt};
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const f2 Bn = {in.bv[2 * p], in.bv[2 * p + 1]};
        e.a[p] = (VASR_SCAN_ABLATE & 1) ? dt2 * A2[p] : exp2v(dt2 * A2[p]);
        if constexpr (FMA) {
            e.b[p] = xdt2 * Bn;
        } else {
            const f2 dB = dt2 * Bn;
            e.b[p] = x2 * dB;
        }
    }
    e.cv = in.cv;
    return e;
}

// One push of the streaming tree scan at in-chunk step I; leaves this lane's partial y in yv[I].
// UP: the up-sweep part only (block composites; no y, no down-sweep prefixes): the chunk
// composites of the chunk-parallel form.
template <int I, int MAXUP, int N, int DPB, bool FMA, bool UP = false, int TC = T>
__device__ __forceinline__ void tree_step(TreeState<MAXUP, log2_c(TC)>& s, const Smem& sm, const StepElem& el, int dl,
                                          int g, f2 (&chunk_a)[NP], f2 (&chunk_b)[NP], float (&yv)[TC]) {
#pragma clang fp contract(off)
    constexpr int G = N / NPL;
    constexpr int LG = log2_c(TC);  // in-chunk stack levels
    // y contribution of h[t] (the exclusive prefix = cb of the current top block)
    if constexpr (!UP && NP == 1) {
        const f2 hp = I == 0 ? s.pb[0] : s.cb[ctz_c(I)][0];
        yv[I] = __builtin_fmaf(hp.y, el.cv[1], hp.x * el.cv[0]);
    } else if constexpr (!UP) {
        // packed: pair-wise partial sums (one v_pk_mul + v_pk_fma per two pairs), then one add
        f2 acc;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const f2 hp = I == 0 ? s.pb[p] : s.cb[ctz_c(I)][p];
            const f2 cp = {el.cv[2 * p], el.cv[2 * p + 1]};
            acc = p == 0 ? hp * cp : mad2<true>(hp, cp, acc);
        }
        yv[I] = N == 128 ? add_f32(acc.x, acc.y) : acc.x + acc.y;  // add_f32: see scan_kernels.h
    }
    if constexpr (I % 8 == 7 && I != TC - 1 && !UP) flush_half<G, I / 8, TC>(yv, sm.yp, dl, g);

    constexpr int J = trailing_ones(I);
    if constexpr (VASR_SCAN_ABLATE & 16) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            s.pb[p] = s.pb[p] + el.b[p];
            s.pa[p] = el.a[p];
        }
        if constexpr (I == TC - 1) flush_half<G, I / 8, TC>(yv, sm.yp, dl, g);
        return;
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        f2 cur_a = el.a[p];
        f2 cur_b = el.b[p];
#pragma unroll
        for (int k = 0; k < J; ++k) {  // up-sweep: (a_r, b_r) <- (a_r a_l, a_r b_l + b_r)
            cur_b = mad2<FMA>(cur_a, s.lb[k][p], cur_b);
            cur_a = cur_a * s.la[k][p];
        }
        if constexpr (J < LG && UP) {
            s.la[J][p] = cur_a;
            s.lb[J][p] = cur_b;
        } else if constexpr (J < LG) {
            s.la[J][p] = cur_a;
            s.lb[J][p] = cur_b;
            constexpr int BL = below_level(I, J, LG);
            f2 Pa, Pb;
            if constexpr (BL >= 0) {
                Pa = s.ca[BL][p];
                Pb = s.cb[BL][p];
            } else {
                Pa = s.pa[p];
                Pb = s.pb[p];
            }
            const f2 c_a = Pa * cur_a;  // down-sweep: a_r <- a_p a_l ; b_r <- a_r b_l + b_p
            s.ca[J][p] = c_a;
            s.cb[J][p] = mad2<FMA>(c_a, cur_b, Pb);
        } else {
            chunk_a[p] = cur_a;
            chunk_b[p] = cur_b;
        }
    }
    if constexpr (I == TC - 1 && !UP) flush_half<G, I / 8, TC>(yv, sm.yp, dl, g);
}

// Upper (chunk-level) stack levels >= UPPER_REG live in LDS, one float4 {a.x, a.y, b.x, b.y} per
// (level, pair) and thread at up[((u - UPPER_REG) * NP + pair) * 256]; the lower levels in registers.
// Levels >= 5 exist from 32 chunks on (L > 512 at 16-step chunks): held in registers they took the
// 16-step kernel from 168 to 202 VGPRs, i.e. from three waves per SIMD to two.
constexpr int UPPER_REG = VASR_SCAN_UPPER_REG;

template <int U, int MAXUP, int LG>
__device__ __forceinline__ void up_get(const TreeState<MAXUP, LG>& s, const float4* up, int p, f2& a, f2& b) {
    if constexpr (U < UPPER_REG) {
        a = s.ula[U][p];
        b = s.ulb[U][p];
    } else {
        const float4 v = up[((U - UPPER_REG) * NP + p) * 256];
        a = f2{v.x, v.y};
        b = f2{v.z, v.w};
    }
}

template <int U, int MAXUP, int LG>
__device__ __forceinline__ void up_set(TreeState<MAXUP, LG>& s, float4* up, int p, f2 a, f2 b) {
    if constexpr (U < UPPER_REG) {
        s.ula[U][p] = a;
        s.ulb[U][p] = b;
    } else {
        up[((U - UPPER_REG) * NP + p) * 256] = make_float4(a.x, a.y, b.x, b.y);
    }
}

template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}

// Merge the finished chunk block into the upper (chunk-level) stack when the chunk counter
// cc has J trailing ones (J = levels to merge, a wave-uniform value: one switch case runs),
// then rebuild the prefix after the upper stack bottom-up from the stream form's (1, 0)
// start: the same float operations as carrying (ca, cb) per upper entry.  The levels set in
// cc + 1 are J and those above J that were set in cc; the uniform per-level tests branch.
//
// Levels >= UPPER_REG live in LDS (L > 512 at 16-step chunks).  The prefix fold runs highest level
// first, so its part over those levels is the same float operations on the same operands until a
// merge reaches them (J >= UPPER_REG, every 32 chunks): it is kept in one more LDS slot per pair
// (HICACHE, read once before the chunk's merges, where its latency overlaps them) instead of
// re-read level by level at the head of every chunk's dependent fold.  Bitwise the same prefix.
#ifndef VASR_SCAN_HICACHE
#define VASR_SCAN_HICACHE 1
#endif
// (not for the 32-step kernel beyond 128 chunks: its 8 KiB more LDS would leave one block per CU)
template <int MAXUP, int LG>
constexpr bool hicache() { return VASR_SCAN_HICACHE && MAXUP > UPPER_REG && !(LG > 4 && MAXUP > 7); }
template <int MAXUP>
__device__ __forceinline__ float4* hicache_slot(float4* up, int p) {
    return up + ((MAXUP - UPPER_REG) * NP + p) * 256;
}

template <int J, int MAXUP, bool FMA, int LG>
__device__ __forceinline__ void merge_upper_j(TreeState<MAXUP, LG>& s, float4* up, const f2 (&chunk_a)[NP],
                                              const f2 (&chunk_b)[NP], int cc1, const float4 (&hi)[NP]) {
#pragma clang fp contract(off)
    f2 na[NP], nb[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        f2 cur_a = chunk_a[p], cur_b = chunk_b[p];
        static_for<0, J>([&](auto Uc) {
            constexpr int u = decltype(Uc)::value;
            f2 la, lb;
            up_get<u>(s, up, p, la, lb);
            cur_b = mad2<FMA>(cur_a, lb, cur_b);
            cur_a = cur_a * la;
        });
        up_set<J>(s, up, p, cur_a, cur_b);
        na[p] = cur_a;
        nb[p] = cur_b;
    }
    constexpr bool CACHED = hicache<MAXUP, LG>() && J < UPPER_REG;  // the fold of the LDS levels is the cache
    f2 pa[NP], pb[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        if constexpr (CACHED) {
            pa[p] = f2{hi[p].x, hi[p].y};
            pb[p] = f2{hi[p].z, hi[p].w};
        } else {
            pa[p] = f2{1.0f, 1.0f};
            pb[p] = f2{0.0f, 0.0f};
        }
    }
    constexpr int TOP = CACHED ? UPPER_REG - 1 : MAXUP - 1;  // highest level folded here
    static_for<0, TOP - J>([&](auto Kc) {
        constexpr int u = TOP - decltype(Kc)::value;
        if ((cc1 >> u) & 1) {  // uniform: a scalar branch, so clear levels cost nothing
            // the empty volatile asm keeps the level a branch: if-converted (all levels computed,
            // then 8 v_cndmask per level) the fold took ~44 VALU per chunk instead of ~4 per set level
            asm volatile("");
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                f2 la, lb;
                up_get<u>(s, up, p, la, lb);
                pa[p] = pa[p] * la;
                pb[p] = mad2<FMA>(pa[p], lb, pb[p]);
            }
        }
    });
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        s.pa[p] = pa[p] * na[p];
        s.pb[p] = mad2<FMA>(s.pa[p], nb[p], pb[p]);
        // J >= UPPER_REG: every level below J is clear in cc + 1, so the prefix just formed is the
        // fold over the LDS levels: the new cache
        if constexpr (hicache<MAXUP, LG>() && J >= UPPER_REG)
            *hicache_slot<MAXUP>(up, p) = make_float4(s.pa[p].x, s.pa[p].y, s.pb[p].x, s.pb[p].y);
    }
}

template <int MAXUP, bool FMA, int LG>
__device__ __forceinline__ void merge_upper(TreeState<MAXUP, LG>& s, float4* up, const f2 (&chunk_a)[NP],
                                            const f2 (&chunk_b)[NP], int cc) {
    const int cc1 = cc + 1;
    float4 hi[NP];
    if constexpr (hicache<MAXUP, LG>()) {
#pragma unroll
        for (int p = 0; p < NP; ++p) hi[p] = *hicache_slot<MAXUP>(up, p);
    }
    switch (__builtin_ctz(~cc)) {
        case 0: merge_upper_j<0, MAXUP, FMA, LG>(s, up, chunk_a, chunk_b, cc1, hi); break;
        case 1: if constexpr (MAXUP > 1) merge_upper_j<1, MAXUP, FMA, LG>(s, up, chunk_a, chunk_b, cc1, hi); break;
        case 2: if constexpr (MAXUP > 2) merge_upper_j<2, MAXUP, FMA, LG>(s, up, chunk_a, chunk_b, cc1, hi); break;
        case 3: if constexpr (MAXUP > 3) merge_upper_j<3, MAXUP, FMA, LG>(s, up, chunk_a, chunk_b, cc1, hi); break;
        case 4: if constexpr (MAXUP > 4) merge_upper_j<4, MAXUP, FMA, LG>(s, up, chunk_a, chunk_b, cc1, hi); break;
        case 5: if constexpr (MAXUP > 5) merge_upper_j<5, MAXUP, FMA, LG>(s, up, chunk_a, chunk_b, cc1, hi); break;
        case 6: if constexpr (MAXUP > 6) merge_upper_j<6, MAXUP, FMA, LG>(s, up, chunk_a, chunk_b, cc1, hi); break;
        case 7: if constexpr (MAXUP > 7) merge_upper_j<7, MAXUP, FMA, LG>(s, up, chunk_a, chunk_b, cc1, hi); break;
        default: if constexpr (MAXUP > 8) merge_upper_j<8, MAXUP, FMA, LG>(s, up, chunk_a, chunk_b, cc1, hi); break;
    }
}

// Two-stage software pipeline over the chunk's 16 steps: operands of step I+2 are read from
// LDS and the state-independent part of step I+1 (exp2, dB, x*dB) is computed while step I's
// tree update runs, so the LDS and v_exp latencies overlap the dependent tree arithmetic.
template <int I, int MAXUP, int N, int DPB, bool FULL, bool FMA, bool UP = false, int TC = T, int BCS = 2 * N>
struct TreeChunk {
    __device__ __forceinline__ static void run(TreeState<MAXUP, log2_c(TC)>& s, const Smem& sm, const StepIn& raw_next,
                                               const StepElem& el, const f2 (&A2)[NP], int dl, int g, int nvalid,
                                               f2 (&ca)[NP], f2 (&cb)[NP], float (&yv)[TC]) {
        if constexpr (I < TC) {
            if (FULL || I < nvalid) {
                StepIn raw2;
                if constexpr (I + 2 < TC) raw2 = load_step<I + 2, N, DPB, FMA, BCS>(sm, dl, g);
                StepElem el_next;
                if constexpr (I + 1 < TC) el_next = make_elem<FMA>(raw_next, A2);
                tree_step<I, MAXUP, N, DPB, FMA, UP, TC>(s, sm, el, dl, g, ca, cb, yv);
                TreeChunk<I + 1, MAXUP, N, DPB, FULL, FMA, UP, TC, BCS>::run(s, sm, raw2, el_next, A2, dl, g, nvalid, ca, cb,
                                                                         yv);
            } else if constexpr (!FULL && !UP) {
                // ragged last chunk: flush the partial sums of the 8-step part the run stopped in
                // (the steps that did not run are 0)
                flush_half<N / NPL, I / 8, TC>(yv, sm.yp, dl, g);
            }
        }
    }
};

__device__ __forceinline__ float* ckpt_of(float* p) { return p; }

// GATE = false: the ungated form for the z-in-tail block (vasr_ssm_scan_ungated_f32): out = y + x D,
// no z slab staged (x | dt | bc only), no silu; the fused tail applies the gate (ssm_tail.hip).
// SAVE (mode 1 only; the checkpointing forward of the backward pass, scan_bwd.hip): one more argument,
// float* ckpt, receives the state h every chunk starts from, ckpt[b][chunk][d][n] ((B, ceil(L / TC), Di,
// N) floats).  The argument is a pack so that the plain kernels keep their signature and their code.
template <int N, int MODE, int MAXUP, int TC = T, bool GATE = true, bool SAVE = false, class... CK>
__global__ __launch_bounds__(256, TC != T ? VASR_SCAN_WAVES_TC32 : NPL == 4 ? (MAXUP <= 7 ? VASR_SCAN_WAVES : 2) : (MAXUP <= 7 ? VASR_SCAN_WAVES_NPL2 : 3))
void ssm_scan_kernel(const float* __restrict__ xz, int64_t ld_xz, const float* __restrict__ dt, int64_t ld_dt,
                     const float* __restrict__ bc, int64_t ld_bc, const float* __restrict__ A2g,
                     const float* __restrict__ Dg, float* __restrict__ out, int64_t ld_out, int B, int L, int Di,
                     CK... ck) {
#pragma clang fp contract(off)
    static_assert(SAVE ? MODE == 1 && sizeof...(CK) == 1 : sizeof...(CK) == 0, "checkpoints: the recurrence only");
    constexpr int G = N / NPL;       // lanes per channel
    constexpr int TPC = TC + 1;      // partial-sum tile row
    constexpr int DPW = 64 / G;      // channels per wave
    constexpr int DPB = NW * DPW;    // channels per block
    // LDS: two staging buffers {x, dt, z: TC x DPB; bc: TC x 2N} (padded to whole 1-KiB
    // LDS-DMA pieces), partial sums DPB x TPC.  The buffers are distinct objects and the chunk
    // loop is unrolled by two, so the compiler can tell that reads of one buffer do not alias
    // the LDS-DMA into the other and does not drain the prefetch (vmcnt(0)) before them.
    constexpr int NSL = GATE ? 3 : 2;  // channel slabs staged: x | dt (| z)
    constexpr int BUF0 = NSL * TC * DPB + TC * 2 * N;
    constexpr int BUF = (BUF0 + 255) / 256 * 256;
    __shared__ __attribute__((aligned(16))) float sbuf0[BUF];
    __shared__ __attribute__((aligned(16))) float sbuf1[BUF];
    __shared__ __attribute__((aligned(16))) float ypart[DPB * TPC];
    // the upper-stack levels >= UPPER_REG of each thread (merge_upper)
    // (+ one slot per pair for the cached fold of those levels, merge_upper_j)
    __shared__ float4 upl[MAXUP > UPPER_REG ? (MAXUP - UPPER_REG + (hicache<MAXUP, log2_c(TC)>() ? 1 : 0)) * NP * 256 : 1];
    float4* const up = upl + threadIdx.x;
    if constexpr (hicache<MAXUP, log2_c(TC)>()) {
#pragma unroll
        for (int p = 0; p < NP; ++p) *hicache_slot<MAXUP>(up, p) = make_float4(1.0f, 1.0f, 0.0f, 0.0f);  // no level set
    }

    // XCD-aware block mapping: blocks id, id+8, id+16, ... share an XCD; give each such
    // group consecutive (b, channel-block) work items so one utterance stays on one L2.
    const int nd = Di / DPB;
    const int nblk = B * nd;
    const int id = blockIdx.x;
    const int q8 = nblk / 8, r8 = nblk % 8, xg = id % 8;
    const int wid = (xg < r8 ? xg * (q8 + 1) : r8 * (q8 + 1) + (xg - r8) * q8) + id / 8;
    const int b = wid / nd;
    const int d0 = (wid - b * nd) * DPB;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int g = lane % G;
    const int dl = wave * DPW + lane / G;
#ifdef VASR_SCAN_STAMPS
    const uint64_t stamp_t0 = __builtin_amdgcn_s_memtime(), stamp_r0 = __builtin_amdgcn_s_memrealtime();
#endif

    f2 A2[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) A2[p] = f2{A2g[g * NPL + 2 * p], A2g[g * NPL + 2 * p + 1]};

    const int64_t row0 = (int64_t)b * L;
    // Chunk staging by LDS-DMA (global_load_lds_dwordx4): each wave-instruction moves 1 KiB
    // into a lane-linear LDS range; slabs x | dt | z (TC x DPB) and bc (TC x 2N) are
    // contiguous, so instruction k of a chunk covers floats [256k, 256k + 256) of the buffer
    // (pieces past BUF0 re-read the last bc piece into the padding).
    constexpr int SLAB = TC * DPB;
    constexpr int NINSTR = BUF / 256;
    static_assert(SLAB % 4 == 0 && DPB % 4 == 0 && (2 * N) % 4 == 0, "16-B staging pieces");
    // Per-lane source pointers of the next chunk to stage, one per staging instruction of this
    // wave, advanced by TC rows per chunk: full chunks cost one 64-bit add per instruction
    // instead of the index arithmetic below (which the ablation with no staging after chunk 0
    // showed to be ~13 % of the kernel's VALU time); the ragged last chunk takes the clamped path.
    constexpr int KPW = (NINSTR + NW - 1) / NW;  // staging instructions per wave (at most)
    const float* nsrc[KPW];
    int64_t nstep[KPW];
    auto src_of = [&](int k, int t0) -> const float* {
        const int off = k * 256 + lane * 4;  // float offset inside the buffer
        if (off < NSL * SLAB) {
            const int arr = off / SLAB, rem = off - arr * SLAB;
            const int t = rem / DPB, c = rem - t * DPB;
            const int64_t row = row0 + min(t0 + t, L - 1);
            return arr == 0 ? xz + row * ld_xz + d0 + c
                 : arr == 1 ? dt + row * ld_dt + d0 + c
                            : xz + row * ld_xz + Di + d0 + c;
        }
        const int rem = min(off - NSL * SLAB, TC * 2 * N - 4);
        const int t = rem / (2 * N), c = rem - t * (2 * N);
        return bc + (row0 + min(t0 + t, L - 1)) * ld_bc + c;
    };
#pragma unroll
    for (int i = 0; i < KPW; ++i) {
        const int k = wave + i * NW;
        const int off = k * 256 + lane * 4;
        nsrc[i] = src_of(min(k, NINSTR - 1), TC);  // chunk 1 (chunk 0 is staged by the clamped path)
        nstep[i] = (off < 2 * SLAB && off >= SLAB) ? (int64_t)TC * ld_dt
                 : off < NSL * SLAB ? (int64_t)TC * ld_xz : (int64_t)TC * ld_bc;
    }
    auto load_chunk_fast = [&](float* buf) {  // the chunk nsrc points at; all TC rows valid
#pragma unroll
        for (int i = 0; i < KPW; ++i) {
            const int k = wave + i * NW;
            if (k < NINSTR)
                __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(nsrc[i]),
                                                 (lds_void*)(buf + k * 256), 16, 0, 0);
            nsrc[i] += nstep[i];
        }
    };
    auto load_chunk = [&](int t0, float* buf) {
        for (int k = wave; k < NINSTR; k += NW) {
            const int off = k * 256 + lane * 4;  // float offset inside the buffer
            const float* src;
            if (off < NSL * SLAB) {
                const int arr = off / SLAB, rem = off - arr * SLAB;
                const int t = rem / DPB, c = rem - t * DPB;
                const int64_t row = row0 + min(t0 + t, L - 1);
                src = arr == 0 ? xz + row * ld_xz + d0 + c
                    : arr == 1 ? dt + row * ld_dt + d0 + c
                               : xz + row * ld_xz + Di + d0 + c;
            } else {
                const int rem = min(off - NSL * SLAB, TC * 2 * N - 4);
                const int t = rem / (2 * N), c = rem - t * (2 * N);
                src = bc + (row0 + min(t0 + t, L - 1)) * ld_bc + c;
            }
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(src),
                                             (lds_void*)(buf + k * 256), 16, 0, 0);
        }
    };

    const int nchunks = (L + TC - 1) / TC;
    load_chunk(0, sbuf0);
    __syncthreads();
    const float Dd = Dg[d0 + tid % DPB];
    // gated-output pass: thread tid owns column d_thr of rows t_thr + j * RPI of each chunk
    static_assert((64 * NW) % DPB == 0, "output tiling");
    constexpr int RPI = (64 * NW) / DPB;  // rows per pass of the 256 threads
    const int t_thr = tid / DPB, d_thr = tid - (tid / DPB) * DPB;
    float* outp = out + (row0 + t_thr) * ld_out + d0 + d_thr;

    TreeState<MAXUP, log2_c(TC)> st;
    f2 h[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        st.pa[p] = f2{1.0f, 1.0f};
        st.pb[p] = f2{0.0f, 0.0f};
        h[p] = f2{0.0f, 0.0f};
    }

    auto chunk = [&](int c, float* buf, float* nbuf) {
        if constexpr (VASR_SCAN_PRIO != 0) {
            // Wave priority between the blocks that share a CU.  They are dispatched together and
            // do equal work, but the SIMDs arbitrate VALU issue by age: left alone the oldest block
            // runs at nearly its solo speed and the three finish one after another (52 / 72 / 96 us
            // at 32 clips), the last third with one wave per SIMD.  Where three blocks share a CU
            // the blocks that have done fewer chunks get the higher priority (3..1 in the first three
            // quarters of the sequence, then by youth); with two, priorities rotate with the chunk
            // index (blocks b and b + 256 share a CU in dispatch order: speed only, never
            // correctness).  Outputs are unchanged.  profiles/r05q-r05s, r05ah: 32-clip launch
            // 95 -> 87.5-89 us, 16-clip 70 -> 63.5 us.
            const int slot = (int)(blockIdx.x >> 8) % 3;
            const int q4 = min(3, 4 * c / nchunks);  // quarter of the sequence this chunk is in
            // fewer chunks first; in the last quarter the youngest block first (by age alone the
            // oldest would finish first again: exits 87 / 94 / 101 us vs 96 / 86 / 97 with this,
            // profiles/r05ah/)
            const int desc = q4 < 3 ? 3 - q4 : slot;
            const int pr = VASR_SCAN_PRIO == 1 ? (int)((__builtin_amdgcn_s_memtime() >> VASR_SCAN_PRIO_SHIFT) + slot) % 3
                         : VASR_SCAN_PRIO == 2 ? (c + slot) % 3
                         : VASR_SCAN_PRIO == 3 ? 3 - q4
                         : VASR_SCAN_PRIO == 5 ? desc
                         : gridDim.x >= 3 * 256 ? desc : (c + slot) % VASR_SCAN_PRIO_ROT;
            switch (pr) {
                case 0: __builtin_amdgcn_s_setprio(0); break;
                case 1: __builtin_amdgcn_s_setprio(1); break;
                case 2: __builtin_amdgcn_s_setprio(2); break;
                default: __builtin_amdgcn_s_setprio(3); break;
            }
        }
        Smem sm{buf, buf + TC * DPB, buf + NSL * TC * DPB, ypart};
        const float* zs = buf + 2 * TC * DPB;  // GATE only
        const int t0 = c * TC;
        const int nvalid = min(TC, L - t0);
        if (c + 1 < nchunks && !((VASR_SCAN_ABLATE & 8) && c > 0)) {
            if (VASR_SCAN_FASTSTAGE && t0 + 2 * TC <= L) load_chunk_fast(nbuf);
            else load_chunk(t0 + TC, nbuf);
        }

        if constexpr (MODE != 1) {
            constexpr bool FMA = MODE == 2;
            f2 cha[NP], chb[NP];
            float yv[TC];
            const StepIn r0 = load_step<0, N, DPB, FMA>(sm, dl, g);
            const StepIn r1 = load_step<1, N, DPB, FMA>(sm, dl, g);
            const StepElem e0 = make_elem<FMA>(r0, A2);
            if (nvalid == TC) {
                TreeChunk<0, MAXUP, N, DPB, true, FMA, false, TC>::run(st, sm, r1, e0, A2, dl, g, nvalid, cha, chb, yv);
            } else {
#pragma unroll
                for (int j = 0; j < TC; ++j) yv[j] = 0.0f;
                TreeChunk<0, MAXUP, N, DPB, false, FMA, false, TC>::run(st, sm, r1, e0, A2, dl, g, nvalid, cha, chb, yv);
            }
            if (c + 1 < nchunks) merge_upper<MAXUP, FMA, log2_c(TC)>(st, up, cha, chb, c);
        } else {
            if constexpr (SAVE) {  // h before this chunk's first step
                float* cp = ckpt_of(ck...) + (((int64_t)b * nchunks + c) * Di + d0 + dl) * N + g * NPL;
#pragma unroll
                for (int p = 0; p < NP; ++p) *reinterpret_cast<f2*>(cp + 2 * p) = h[p];
            }
            for (int i = 0; i < nvalid; ++i) {
                const float xv = sm.xs[i * DPB + dl];
                const float dv = sm.dts[i * DPB + dl];
                const vecN bv = *reinterpret_cast<const vecN*>(sm.bcs + i * 2 * N + g * NPL);
                const vecN cv = *reinterpret_cast<const vecN*>(sm.bcs + i * 2 * N + N + g * NPL);
                const f2 dv2 = {dv, dv}, xv2 = {xv, xv};
                f2 part = {0.f, 0.f};
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const f2 Bn = {bv[2 * p], bv[2 * p + 1]};
                    const f2 Cn = {cv[2 * p], cv[2 * p + 1]};
                    const f2 dA = exp2v(dv2 * A2[p]);
                    const f2 dB = dv2 * Bn;
                    h[p] = dA * h[p] + xv2 * dB;
                    part = part + h[p] * Cn;
                }
                const float y = group_sum<G>(part.x + part.y);
                if (g == 0) ypart[dl * TPC + i] = y;
            }
        }
        // partial sums visible to all waves, and the LDS-DMA of chunk c+1 landed: vmcnt(0) here,
        // before this chunk's output stores are issued.  vmcnt counts loads and stores together
        // and a store may complete before an older load, so a count that has stores younger than
        // the awaited LDS-DMA does not prove the DMA landed (the compiler's own waitcnt model
        // treats mixed pending loads and stores as out of order too).  Counting the chunk's
        // output stores at the chunk end instead (rounds 1-3) let the next chunk read staging
        // slots whose DMA was still in flight when a co-resident kernel slowed the loads: wrong
        // scan outputs under concurrent streams (tools/diag/interference.py, profiles/r04b/).
        // The DMA was issued a whole chunk of tree steps ago and the previous chunk's stores
        // as long ago, so this wait is normally already satisfied.
        __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0) lgkmcnt(0)
        if constexpr (!(VASR_SCAN_ABLATE & 64)) __builtin_amdgcn_s_barrier();
        // gated output of this chunk: (sum_g partials + x D) * silu(z), coalesced along d
        // (each thread's rows are t_thr + j * RPI: outp advances TC rows per chunk, no 64-bit
        // row arithmetic per output)
#pragma unroll
        for (int j = 0; j < (TC * DPB + 64 * NW - 1) / (64 * NW); ++j) {  // t < nvalid <= TC guards the rest
            const int t = t_thr + j * RPI, d = d_thr;
            if (t < nvalid) {
                const float ysum = ypart[d * TPC + t];
                if ((VASR_SCAN_ABLATE & 32) && ysum != 1.2345f) continue;
                const float xv = sm.xs[t * DPB + d];
                const float y = ysum + xv * Dd;
                if constexpr (GATE) {
                    const float zv = zs[t * DPB + d];
                    outp[(int64_t)j * RPI * ld_out] = y * silu_of<MODE>(zv);
                } else {
                    outp[(int64_t)j * RPI * ld_out] = y;  // the tail gates it (vasr_ssm_block_tail_gated_f32)
                }
            }
        }
        outp += TC * ld_out;
        // Before the next chunk every wave must be done reading this chunk's buffers (its LDS
        // reads complete: lgkmcnt(0)); chunk c+1's staging already landed (the vmcnt(0) above),
        // and this chunk's output stores stay in flight.
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0) only
        if constexpr (!(VASR_SCAN_ABLATE & 64)) __builtin_amdgcn_s_barrier();
    };
    for (int c = 0; c < nchunks; c += 2) {
        chunk(c, sbuf0, sbuf1);
        if (c + 1 < nchunks) chunk(c + 1, sbuf1, sbuf0);
    }
#ifdef VASR_SCAN_STAMPS
    if (tid == 0 && g_scan_stamps) {
        const uint64_t t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        uint32_t xcc, hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        int64_t* o = g_scan_stamps + 5 * (int64_t)blockIdx.x;
        o[0] = (int64_t)(xcc & 0xF) | ((int64_t)hw << 8);
        o[1] = (int64_t)stamp_t0;
        o[2] = (int64_t)stamp_r0;
        o[3] = (int64_t)t1;
        o[4] = (int64_t)r1;
    }
#endif
}

// The checkpointing forward of the recurrence (vasr_ssm_scan_save_f32): the mode-1 kernel launch_n
// runs, with SAVE.
template <int N, bool GATE>
int launch_save_n(const float* xz, int64_t ld_xz, const float* dt, int64_t ld_dt, const float* bc, int64_t ld_bc,
                  const float* A2, const float* D, float* out, int64_t ld_out, int B, int L, int Di, float* ckpt,
                  hipStream_t s) {
    constexpr int G = N / NPL;
    constexpr int DPB = NW * (64 / G);
    if (Di % DPB != 0) {
        set_error("vasr_ssm_scan_save_f32: Di=%d must be a multiple of %d for N=%d", Di, DPB, N);
        return VASR_EUNSUPPORTED;
    }
    hipLaunchKernelGGL((ssm_scan_kernel<N, 1, 5, T, GATE, true, float*>), dim3(B * (Di / DPB)), dim3(64 * NW), 0, s, xz,
                       ld_xz, dt, ld_dt, bc, ld_bc, A2, D, out, ld_out, B, L, Di, ckpt);
    return launch_status("vasr_ssm_scan_save_f32");
}

template <int N, int MODE, bool GATE = true>
int launch_n(const float* xz, int64_t ld_xz, const float* dt, int64_t ld_dt, const float* bc, int64_t ld_bc,
             const float* A2, const float* D, float* out, int64_t ld_out, int B, int L, int Di, hipStream_t s) {
    constexpr int G = N / NPL;
    constexpr int DPB = NW * (64 / G);
    if (Di % DPB != 0) {
        set_error("vasr_ssm_scan_f32: Di=%d must be a multiple of %d for N=%d", Di, DPB, N);
        return VASR_EUNSUPPORTED;
    }
    dim3 grid(B * (Di / DPB));
    dim3 block(64 * NW);
    // Chunk length: 32 steps while the launch has at most two waves per SIMD (the 32-step
    // kernel's extra stack level takes 206 VGPRs: two waves per SIMD), else 16.  The same float
    // operations either way (the in-chunk / upper-stack split does not change the tree), and
    // half the per-chunk barriers, output passes, staging waits and upper-stack merges: 76.5 vs
    // 80.6 us per 16-clip launch, 214 vs 231 us at 30 s, C2 141.4k vs 135.9k RTFx
    // (profiles/r02e/scan_t32/).  At 32 clips (three waves per SIMD) 16 stays (115 vs 117 us).
    // vasr_set_option(VASR_OPT_SCAN_CHUNK, 16|32) (env VASR_SCAN_T) forces one.
    const int tc_opt = option(VASR_OPT_SCAN_CHUNK);
    const long waves = (long)grid.x * NW;
    const bool t32 = MODE != 1 && (tc_opt ? tc_opt == 32 : waves <= 2 * 1024);
    if (t32) {
        const int nch32 = (L + 31) / 32;
        if (nch32 <= 32)
            hipLaunchKernelGGL((ssm_scan_kernel<N, MODE, 5, 32, GATE>), grid, block, 0, s, xz, ld_xz, dt, ld_dt, bc, ld_bc,
                               A2, D, out, ld_out, B, L, Di);
        else if (nch32 <= 128)
            hipLaunchKernelGGL((ssm_scan_kernel<N, MODE, 7, 32, GATE>), grid, block, 0, s, xz, ld_xz, dt, ld_dt, bc, ld_bc,
                               A2, D, out, ld_out, B, L, Di);
        else
            hipLaunchKernelGGL((ssm_scan_kernel<N, MODE, 9, 32, GATE>), grid, block, 0, s, xz, ld_xz, dt, ld_dt, bc, ld_bc,
                               A2, D, out, ld_out, B, L, Di);
        return launch_status("vasr_ssm_scan_f32");
    }
    const int nchunks = (L + T - 1) / T;
    if (MODE == 1 || nchunks <= 32)
        hipLaunchKernelGGL((ssm_scan_kernel<N, MODE, 5, T, GATE>), grid, block, 0, s, xz, ld_xz, dt, ld_dt, bc, ld_bc, A2, D,
                           out, ld_out, B, L, Di);
    else if (nchunks <= 128)
        hipLaunchKernelGGL((ssm_scan_kernel<N, MODE, 7, T, GATE>), grid, block, 0, s, xz, ld_xz, dt, ld_dt, bc, ld_bc, A2, D,
                           out, ld_out, B, L, Di);
    else
        hipLaunchKernelGGL((ssm_scan_kernel<N, MODE, 9, T, GATE>), grid, block, 0, s, xz, ld_xz, dt, ld_dt, bc, ld_bc, A2, D,
                           out, ld_out, B, L, Di);
    return launch_status("vasr_ssm_scan_f32");
}

// ----------------------------------------------------------------------------------------
// Chunk-parallel form of the tree scan (modes 0 and 2), for launches too small to fill the
// chip (B * Di * N / 256 waves well under one per SIMD: one utterance at a time, as the
// reference's scripts/transcribe.py:69-78 and evaluate.py:91-98 call the model).  The
// streaming kernel above runs time serially per state lane; here time is cut at its 16-step
// chunks and the same float operations run in three launches:
//   1. ssm_scan_chunk_kernel<PHASE 1>: per (utterance, channel block, chunk) the chunk's
//      up-sweep composite (la, lb) -- exactly the (chunk_a, chunk_b) the streaming kernel
//      forms at step 15 -- into level 0 of the workspace (the last chunk's is never needed);
//   2. scan_levels_kernel: per state lane, the composites of the aligned blocks of 2^k chunks,
//      level by level (block = merge(left half, right half), the up-sweep op): these are the
//      entries the streaming kernel's chunk-level stack holds, formed by the same merges;
//   3. ssm_scan_chunk_kernel<PHASE 3>: per (utterance, channel block, chunk c) the prefix
//      chunk c starts from -- the fold over the blocks of c's binary decomposition, highest
//      first, as merge_upper folds the stack -- then the in-chunk tree from that prefix, the
//      y = sum_n h C reduction and the gated output, as the streaming kernel does.
// Every state value is therefore the same float operation on the same operands as in the
// streaming kernel of the same lane layout: outputs are bitwise equal to it.
// Workspace: ws_a, ws_b = [B][2 * nchunks][Di][N] floats each: level k (k = 0, 1, ...) holds
// n_k = floor(n_{k-1} / 2) block composites (n_0 = nchunks - 1) starting at slot
// sum_{i<k} n_i.
template <int N, int MODE, int PHASE>
__global__ __launch_bounds__(256) void ssm_scan_chunk_kernel(
    const float* __restrict__ xz, int64_t ld_xz, const float* __restrict__ dt, int64_t ld_dt,
    const float* __restrict__ bc, int64_t ld_bc, const float* __restrict__ A2g, const float* __restrict__ Dg,
    float* __restrict__ out, int64_t ld_out, int B, int L, int Di, float* __restrict__ ws_a,
    float* __restrict__ ws_b) {
#pragma clang fp contract(off)
    static_assert(PHASE == 1 || PHASE == 3, "phase 1 (composites) or 3 (outputs)");
    static_assert(MODE == 0 || MODE == 2, "tree modes only");
    constexpr bool FMA = MODE == 2;
    constexpr bool UP = PHASE == 1;
    constexpr int G = N / NPL;
    constexpr int DPW = 64 / G;
    constexpr int DPB = NW * DPW;
    constexpr int BUF0 = 3 * T * DPB + T * 2 * N;
    constexpr int BUF = (BUF0 + 255) / 256 * 256;
    constexpr int SLAB = T * DPB;
    constexpr int NINSTR = BUF / 256;
    __shared__ __attribute__((aligned(16))) float sbuf[BUF];
    __shared__ __attribute__((aligned(16))) float ypart[PHASE == 3 ? DPB * TP : 4];

    const int nd = Di / DPB;
    const int nch = (L + T - 1) / T;
    const int nblk = B * nch * nd;
    // XCD-aware: consecutive work items (the channel blocks of one chunk, then the chunks of
    // one utterance) share an XCD and its L2 (the chunk's B / C rows are read by all of them)
    const int id = blockIdx.x;
    const int q8 = nblk / 8, r8 = nblk % 8, xg = id % 8;
    const int wid = (xg < r8 ? xg * (q8 + 1) : r8 * (q8 + 1) + (xg - r8) * q8) + id / 8;
    const int b = wid / (nch * nd);
    const int rem = wid - b * nch * nd;
    const int c = rem / nd;
    const int d0 = (rem - c * nd) * DPB;
    if (PHASE == 1 && c >= nch - 1) return;  // block-uniform: the last chunk's composite is unused

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int g = lane % G;
    const int dl = wave * DPW + lane / G;

    f2 A2[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) A2[p] = f2{A2g[g * NPL + 2 * p], A2g[g * NPL + 2 * p + 1]};

    const int64_t row0 = (int64_t)b * L;
    const int t0 = c * T;
    const int nvalid = min(T, L - t0);
    // stage the chunk (same layout as the streaming kernel's buffers; rows past L re-read L-1)
    for (int k = wave; k < NINSTR; k += NW) {
        const int off = k * 256 + lane * 4;
        const float* src;
        if (off < 3 * SLAB) {
            const int arr = off / SLAB, r = off - arr * SLAB;
            const int t = r / DPB, cc = r - t * DPB;
            const int64_t row = row0 + min(t0 + t, L - 1);
            src = arr == 0 ? xz + row * ld_xz + d0 + cc : arr == 1 ? dt + row * ld_dt + d0 + cc
                                                                 : xz + row * ld_xz + Di + d0 + cc;
        } else {
            const int r = min(off - 3 * SLAB, T * 2 * N - 4);
            const int t = r / (2 * N), cc = r - t * (2 * N);
            src = bc + (row0 + min(t0 + t, L - 1)) * ld_bc + cc;
        }
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(src), (lds_void*)(sbuf + k * 256), 16, 0, 0);
    }
    __syncthreads();  // vmcnt(0) + barrier: the chunk is in LDS

    TreeState<1> st;
    // this lane's state indices g*NPL .. g*NPL + NPL-1 of channel d0 + dl, chunk slot c - 1
    const int64_t wrow = (int64_t)Di * N;
    const int64_t wl = (int64_t)(d0 + dl) * N + g * NPL;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        st.pa[p] = f2{1.0f, 1.0f};
        st.pb[p] = f2{0.0f, 0.0f};
    }
    if (PHASE == 3 && c > 0) {
        // prefix of chunk c: fold the level composites of c's set bits, highest first
        // (merge_upper's fold of the stack after chunk c - 1)
        int off[16], cnt = nch - 1, top = 0;
        off[0] = 0;
        while ((2 << top) <= c) {  // levels 0 .. floor(log2 c)
            off[top + 1] = off[top] + cnt;
            cnt >>= 1;
            ++top;
        }
        const int64_t wb = (int64_t)b * 2 * nch * wrow + wl;
        for (int u = top; u >= 0; --u) {
            if ((c >> u) & 1) {
                const int64_t o = wb + (int64_t)(off[u] + (c >> u) - 1) * wrow;
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const f2 la = *reinterpret_cast<const f2*>(ws_a + o + 2 * p);
                    const f2 lb = *reinterpret_cast<const f2*>(ws_b + o + 2 * p);
                    st.pa[p] = st.pa[p] * la;
                    st.pb[p] = mad2<FMA>(st.pa[p], lb, st.pb[p]);
                }
            }
        }
    }
    Smem sm{sbuf, sbuf + T * DPB, sbuf + 3 * T * DPB, ypart};
    f2 cha[NP], chb[NP];
    float yv[T];
    const StepIn r0 = load_step<0, N, DPB, FMA>(sm, dl, g);
    const StepIn r1 = load_step<1, N, DPB, FMA>(sm, dl, g);
    const StepElem e0 = make_elem<FMA>(r0, A2);
    if (UP || nvalid == T) {  // phase 1 runs full chunks only (c < nch - 1)
        TreeChunk<0, 1, N, DPB, true, FMA, UP>::run(st, sm, r1, e0, A2, dl, g, nvalid, cha, chb, yv);
    } else {
#pragma unroll
        for (int j = 0; j < T; ++j) yv[j] = 0.0f;
        TreeChunk<0, 1, N, DPB, false, FMA, UP>::run(st, sm, r1, e0, A2, dl, g, nvalid, cha, chb, yv);
    }
    if constexpr (PHASE == 1) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int64_t o = ((int64_t)b * 2 * nch + c) * wrow + wl + 2 * p;
            *reinterpret_cast<f2*>(ws_a + o) = cha[p];
            *reinterpret_cast<f2*>(ws_b + o) = chb[p];
        }
    } else {
        __syncthreads();  // partial sums visible to all waves
        const float* zs = sbuf + 2 * T * DPB;
        for (int idx = tid; idx < T * DPB; idx += 64 * NW) {
            const int t = idx / DPB, d = idx - t * DPB;
            if (t < nvalid) {
                const float ysum = ypart[d * TP + t];
                const float xv = sm.xs[t * DPB + d];
                const float zv = zs[t * DPB + d];
                const float y = ysum + xv * Dg[d0 + d];
                out[(row0 + t0 + t) * ld_out + d0 + d] = y * silu_of<MODE>(zv);
            }
        }
    }
}

// Phase 2: a workgroup takes LP consecutive state pairs of one utterance, stages their chunk
// composites in LDS (one wave of loads), and forms the block composites level by level in
// place (level k's block j replaces its left half's slot j * 2^k), 256 threads sharing each
// level's independent merges; every level is also written to its workspace slots for phase 3.
constexpr int LP = 16;  // state pairs per workgroup: (nchunks - 1) x 16 x 16 B of LDS (<= 128 KiB)
template <bool FMA>
__global__ __launch_bounds__(256) void scan_levels_kernel(float* __restrict__ ws_a, float* __restrict__ ws_b, int B,
                                                          int nch, int Di, int N) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float4 lv[];  // [slot][LP] {la.x, la.y, lb.x, lb.y}
    const int64_t per_b = (int64_t)Di * N / 2;   // state pairs per utterance (a multiple of LP)
    const int64_t q0 = (int64_t)blockIdx.x * LP;  // first pair of this workgroup
    const int64_t b = q0 / per_b;
    const int64_t e0 = (q0 - b * per_b) * 2;
    const int64_t slot = (int64_t)Di * N;
    float* __restrict__ A = ws_a + b * 2 * nch * slot + e0;
    float* __restrict__ Bv = ws_b + b * 2 * nch * slot + e0;
    const int tid = threadIdx.x;
    const int n0 = nch - 1;
    for (int i = tid; i < n0 * LP; i += 256) {
        const int sl = i / LP, pp = i - sl * LP;
        const f2 la = *reinterpret_cast<const f2*>(A + sl * slot + 2 * pp);
        const f2 lb = *reinterpret_cast<const f2*>(Bv + sl * slot + 2 * pp);
        lv[i] = make_float4(la.x, la.y, lb.x, lb.y);
    }
    __syncthreads();
    int dst = n0, cnt = n0, k = 1;
    while (cnt >= 2) {
        const int n = cnt >> 1;
        const int half = 1 << (k - 1);
        for (int i = tid; i < n * LP; i += 256) {
            const int j = i / LP, pp = i - j * LP;
            const float4 l = lv[(2 * j * half) * LP + pp];
            const float4 r = lv[((2 * j + 1) * half) * LP + pp];
            const f2 la = {l.x, l.y}, lb = {l.z, l.w}, ra = {r.x, r.y}, rb = {r.z, r.w};
            const f2 ob = mad2<FMA>(ra, lb, rb);  // up-sweep: (a_r, b_r) <- (a_r a_l, a_r b_l + b_r)
            const f2 oa = ra * la;
            lv[(2 * j * half) * LP + pp] = make_float4(oa.x, oa.y, ob.x, ob.y);
            *reinterpret_cast<f2*>(A + (int64_t)(dst + j) * slot + 2 * pp) = oa;
            *reinterpret_cast<f2*>(Bv + (int64_t)(dst + j) * slot + 2 * pp) = ob;
        }
        __syncthreads();
        dst += n;
        cnt = n;
        ++k;
    }
}

template <int N, int MODE>
int launch_chunked_n(const float* xz, int64_t ld_xz, const float* dt, int64_t ld_dt, const float* bc, int64_t ld_bc,
                     const float* A2, const float* D, float* out, int64_t ld_out, int B, int L, int Di, float* ws_a,
                     float* ws_b, hipStream_t s) {
    constexpr int G = N / NPL;
    constexpr int DPB = NW * (64 / G);
    if (Di % DPB != 0) {
        set_error("vasr_ssm_scan_chunked_f32: Di=%d must be a multiple of %d for N=%d", Di, DPB, N);
        return VASR_EUNSUPPORTED;
    }
    const int nch = (L + T - 1) / T;
    const dim3 grid(B * nch * (Di / DPB)), block(64 * NW);
    if (nch > 1) {
        hipLaunchKernelGGL((ssm_scan_chunk_kernel<N, MODE, 1>), grid, block, 0, s, xz, ld_xz, dt, ld_dt, bc, ld_bc, A2, D,
                           out, ld_out, B, L, Di, ws_a, ws_b);
        if (int rc = launch_status("vasr_ssm_scan_chunked_f32")) return rc;
        const int64_t pairs = (int64_t)B * Di * N / 2;
        const size_t lds = (size_t)(nch - 1) * npl2::LP * sizeof(float4);
        if (lds > 65536) {  // long clips (L > 4096): raise the dynamic LDS limit (<= 128 KiB here)
            const hipError_t e = hipFuncSetAttribute(
                reinterpret_cast<const void*>(&npl2::scan_levels_kernel<MODE == 2>),
                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) {
                set_error("vasr_ssm_scan_chunked_f32: %s", hipGetErrorString(e));
                return (int)e;
            }
        }
        hipLaunchKernelGGL((npl2::scan_levels_kernel<MODE == 2>), dim3((unsigned)(pairs / npl2::LP)), dim3(256), lds, s,
                           ws_a, ws_b, B, nch, Di, N);
        if (int rc = launch_status("vasr_ssm_scan_chunked_f32")) return rc;
    }
    hipLaunchKernelGGL((ssm_scan_chunk_kernel<N, MODE, 3>), grid, block, 0, s, xz, ld_xz, dt, ld_dt, bc, ld_bc, A2, D,
                       out, ld_out, B, L, Di, ws_a, ws_b);
    return launch_status("vasr_ssm_scan_chunked_f32");
}


// ----------------------------------------------------------------------------------------
// One-launch time-split form of the chunk-parallel scan.  At one utterance the three launches
// above cost 5-7 us each whatever their work (B = 1, 10 s: 5.8 + 5.5 + 6.8 us per scan, eight
// scans per utterance).  Here one workgroup owns the DPW channels of one wave (all their state
// lanes) of one utterance, and its waves split time: wave w owns the K = 2^KL chunks of TS steps
// from chunk c0 = w K.  Range boundaries are boundaries of the tree's aligned chunk blocks, so:
//   phase 1: wave w forms its range's up-sweep composite -- the chunk composites folded as the
//            streaming kernel's chunk-level stack folds them -- where a later range needs it;
//   levels:  wave w, once the waves before it have published their composites (LDS ready
//            flags, no workgroup barrier), forms the composites of the aligned blocks of 2^j
//            ranges in its own decomposition (the up-sweep merge, pairwise as a segment tree);
//   phase 3: wave w holds the stack the streaming kernel holds after chunk c0 - 1 (the blocks of
//            c0's binary decomposition, all at levels >= KL: their prefix fold is formed once)
//            and runs its chunks as the streaming kernel does, with an in-wave stack of KL levels.
// Every state value is the same float operation on the same operands as in the streaming kernel
// of the same lane layout (any chunk length: the in-chunk / chunk-level split does not change
// the tree), so the outputs are bitwise equal to it.  Memory: each wave streams its own range
// through a private LDS region by LDS-DMA -- phase 1 as one or a few whole super-chunks (x, dt and
// the B rows only), phase 3 as double-buffered chunks whose first two are in flight while the
// levels are formed: a wave's chain is a few chunks long, so its staging latency is the cost to
// hide (r05al: chunk-by-chunk staging in both phases took 17.8 us at B = 1, 10 s).
constexpr int TS = 8;  // steps per chunk of the time-split form

constexpr int split_round64(int v) { return (v + 63) / 64 * 64; }

template <int N>
struct SplitLds {
    static constexpr int SWM = 16;                          // waves (time ranges) per workgroup, at most
    static constexpr int LOGSW = 4;
    static constexpr int G = N / NPL;
    static constexpr int DPW = 64 / G;                      // channels per workgroup
    static constexpr int SLABS = 3 * TS * DPW;              // phase 3: x | dt | z slabs, TS x DPW each
    static constexpr int SLABP = split_round64(SLABS);      // whole 4-B LDS-DMA instructions (64 floats)
    static constexpr int BUFW = SLABP + TS * 2 * N;         // + the bc rows (whole 16-B instructions)
    static constexpr int NI = SLABP / 64 + TS * 2 * N / 256;  // LDS-DMA instructions per phase-3 chunk
    static constexpr int REG = 2 * BUFW;                    // one wave's region: two chunk buffers
    // phase 1: super-chunks of P1C chunks, x | dt slabs and B rows (N floats a step) in the region
    static constexpr int p1_size(int c) { return split_round64(2 * c * TS * DPW) + (c * TS * N + 255) / 256 * 256; }
    static constexpr int P1C = p1_size(4) <= REG ? 4 : p1_size(2) <= REG ? 2 : 1;
    static constexpr int SEG = SWM * NP * 64 * 4;           // range composites: a float4 per range, pair and lane
    static constexpr int YP = DPW * (TS + 1);               // partial-sum tile of one wave
    static constexpr int TOTAL = SWM * REG + SEG + SWM * YP + SWM;  // + a ready flag per wave
    static_assert(TS * 2 * N % 256 == 0 && TS * DPW <= 64 && p1_size(1) <= REG, "time-split layout");
    static_assert(TOTAL * 4 <= 160 * 1024, "time-split LDS");
};

// Fold a finished chunk composite (a, b) with the in-wave stack levels 0 .. J-1 (the up-sweep
// merge, left siblings innermost first: merge_upper_j's loop)
template <int J, int MU, bool FMA, int LG>
__device__ __forceinline__ void split_up(const TreeState<MU, LG>& s, f2 (&a)[NP], f2 (&b)[NP]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int p = 0; p < NP; ++p)
        static_for<0, J>([&](auto Uc) {
            constexpr int u = decltype(Uc)::value;
            b[p] = mad2<FMA>(a[p], s.ulb[u][p], b[p]);
            a[p] = a[p] * s.ula[u][p];
        });
}

// Phase 1: push chunk lc's composite (J = trailing ones of lc < KL levels to fold)
template <int J, int MU, bool FMA, int LG>
__device__ __forceinline__ void split_push_j(TreeState<MU, LG>& s, const f2 (&ca)[NP], const f2 (&cb)[NP]) {
    f2 a[NP], b[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) a[p] = ca[p], b[p] = cb[p];
    split_up<J, MU, FMA, LG>(s, a, b);
#pragma unroll
    for (int p = 0; p < NP; ++p) s.ula[J][p] = a[p], s.ulb[J][p] = b[p];
}

// Phase 3: merge_upper_j of the streaming kernel with the stack levels >= KL folded once into
// (pah, pbh): the prefix fold runs highest level first, so those levels are its first steps
template <int J, int MU, bool FMA, int LG>
__device__ __forceinline__ void split_merge_j(TreeState<MU, LG>& s, const f2 (&ca)[NP], const f2 (&cb)[NP], int lc1,
                                              const f2 (&pah)[NP], const f2 (&pbh)[NP]) {
#pragma clang fp contract(off)
    f2 na[NP], nb[NP], pa[NP], pb[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) na[p] = ca[p], nb[p] = cb[p], pa[p] = pah[p], pb[p] = pbh[p];
    split_up<J, MU, FMA, LG>(s, na, nb);
#pragma unroll
    for (int p = 0; p < NP; ++p) s.ula[J][p] = na[p], s.ulb[J][p] = nb[p];
    static_for<0, MU - 1 - J>([&](auto Kc) {
        constexpr int u = MU - 1 - decltype(Kc)::value;
        if ((lc1 >> u) & 1) {
            asm volatile("");  // a uniform branch (see merge_upper_j)
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                pa[p] = pa[p] * s.ula[u][p];
                pb[p] = mad2<FMA>(pa[p], s.ulb[u][p], pb[p]);
            }
        }
    });
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        s.pa[p] = pa[p] * na[p];
        s.pb[p] = mad2<FMA>(s.pa[p], nb[p], pb[p]);
    }
}

template <int N, int MODE, int KL>
__global__ __launch_bounds__(64 * SplitLds<N>::SWM) void ssm_scan_split_kernel(
    const float* __restrict__ xz, int64_t ld_xz, const float* __restrict__ dt, int64_t ld_dt,
    const float* __restrict__ bc, int64_t ld_bc, const float* __restrict__ A2g, const float* __restrict__ Dg,
    float* __restrict__ out, int64_t ld_out, int B, int L, int Di) {
#pragma clang fp contract(off)
    static_assert(MODE == 0 || MODE == 2, "tree modes only");
    constexpr bool FMA = MODE == 2;
    using Lay = SplitLds<N>;
    constexpr int G = Lay::G, DPW = Lay::DPW, SWM = Lay::SWM;
    constexpr int K = 1 << KL;
    constexpr int MU = KL > 0 ? KL : 1;  // in-wave stack levels (registers)
    constexpr int LG = log2_c(TS);
    constexpr int C1 = Lay::P1C < K ? Lay::P1C : K;  // chunks per phase-1 super-chunk
    constexpr int S1 = C1 * TS;
    constexpr int SL1 = 2 * S1 * DPW;
    constexpr int SL1P = split_round64(SL1);
    constexpr int NB1 = (S1 * N + 255) / 256;
    // vmcnt(NI): every load but the last chunk's NI LDS-DMA instructions landed
    constexpr int WAIT_NI = 0x0F70 | (Lay::NI & 15) | ((Lay::NI >> 4) << 14);
    __shared__ __attribute__((aligned(16))) float lds[Lay::TOTAL];

    // XCD-aware map as the other forms (the channel groups of one utterance share an L2)
    const int nd = Di / DPW;
    const int nblk = B * nd;
    const int id = blockIdx.x;
    const int q8 = nblk / 8, r8 = nblk % 8, xg = id % 8;
    const int wid = (xg < r8 ? xg * (q8 + 1) : r8 * (q8 + 1) + (xg - r8) * q8) + id / 8;
    const int b = wid / nd;
    const int d0 = (wid - b * nd) * DPW;

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int g = lane % G;
    const int dl = lane / G;
    float* const reg = lds + w * Lay::REG;
    float* const sb0 = reg;
    float* const sb1 = reg + Lay::BUFW;
    float4* const seg = reinterpret_cast<float4*>(lds + SWM * Lay::REG);
    float* const yp = lds + SWM * Lay::REG + Lay::SEG + w * Lay::YP;
    int* const flg = reinterpret_cast<int*>(lds + SWM * Lay::REG + Lay::SEG + SWM * Lay::YP);  // ready flags

    f2 A2[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) A2[p] = f2{A2g[g * NPL + 2 * p], A2g[g * NPL + 2 * p + 1]};
    const int t_thr = lane / DPW, d_thr = lane - (lane / DPW) * DPW;  // gated-output pass: one (row, channel) per lane
    const float Dd = Dg[d0 + d_thr];

#ifdef VASR_SCAN_STAMPS
    int64_t stamp[7];
    stamp[0] = (int64_t)__builtin_amdgcn_s_memrealtime();
#define VASR_SPLIT_STAMP(i) stamp[i] = (int64_t)__builtin_amdgcn_s_memrealtime()
#else
#define VASR_SPLIT_STAMP(i)
#endif
    const int64_t row0 = (int64_t)b * L;
    const int nch = (L + TS - 1) / TS;
    const int c0 = w * K;
    const int nloc = min(K, nch - c0);  // >= 1: the launcher sizes the workgroup

    // phase 3: the TS rows from t0 into buf -- x | dt | z slabs by 4-B LDS-DMA, bc rows by 16-B
    // (rows past L re-read L-1)
    auto stage = [&](int t0, float* buf) {
#pragma unroll
        for (int k = 0; k < Lay::SLABP / 64; ++k) {
            const int off = k * 64 + lane;
            const float* src = xz + row0 * ld_xz + d0;
            if (off < Lay::SLABS) {
                const int arr = off / (TS * DPW), r = off - arr * (TS * DPW);
                const int t = r / DPW, cc = r - t * DPW;
                const int64_t row = row0 + min(t0 + t, L - 1);
                src = arr == 0 ? xz + row * ld_xz + d0 + cc : arr == 1 ? dt + row * ld_dt + d0 + cc
                                                                       : xz + row * ld_xz + Di + d0 + cc;
            }
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(src), (lds_void*)(buf + k * 64), 4, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < TS * 2 * N / 256; ++k) {
            const int off = k * 256 + lane * 4;
            const int t = off / (2 * N), cc = off - t * (2 * N);
            const float* src = bc + (row0 + min(t0 + t, L - 1)) * ld_bc + cc;
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(src),
                                             (lds_void*)(buf + Lay::SLABP + k * 256), 16, 0, 0);
        }
    };
    // phase 1: the S1 rows from t0 into the region -- x | dt slabs and the B half of the bc rows
    auto stage1 = [&](int t0) {
#pragma unroll
        for (int k = 0; k < SL1P / 64; ++k) {
            const int off = k * 64 + lane;
            const float* src = xz + row0 * ld_xz + d0;
            if (off < SL1) {
                const int arr = off / (S1 * DPW), r = off - arr * (S1 * DPW);
                const int t = r / DPW, cc = r - t * DPW;
                const int64_t row = row0 + min(t0 + t, L - 1);
                src = arr == 0 ? xz + row * ld_xz + d0 + cc : dt + row * ld_dt + d0 + cc;
            }
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(src), (lds_void*)(reg + k * 64), 4, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < NB1; ++k) {
            const int off = min(k * 256 + lane * 4, S1 * N - 4);
            const int t = off / N, cc = off - t * N;
            const float* src = bc + (row0 + min(t0 + t, L - 1)) * ld_bc + cc;
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(src),
                                             (lds_void*)(reg + SL1P + k * 256), 16, 0, 0);
        }
    };

    TreeState<MU, LG> st;
    f2 cha[NP], chb[NP];
    float yv[TS];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        st.pa[p] = f2{1.0f, 1.0f};
        st.pb[p] = f2{0.0f, 0.0f};
    }

    // ---- phase 1: this range's composite, if a later range follows (its chunks are all full)
    f2 ra[NP], rb[NP];
    const bool need = (w + 1) * K < nch;
    // ready flags: cleared before any wave can set one (a stale LDS value from an earlier
    // workgroup must not read as set).  The flags are atomics (an atomic clear cannot be dropped
    // as a dead store), published after a release fence and read before an acquire fence, both
    // limited to LDS ("local"), so the seg stores / loads they guard are ordered by the memory
    // model, not by the waitcnt placement of today's codegen (ADVICE r05).  The clear goes before
    // the first LDS-DMA is issued: the compiler orders an LDS atomic after LDS-DMA in flight
    // (vmcnt(0)), which would hold the barrier for the slowest wave's first super-chunk.
    if (lane == 0) __hip_atomic_store(flg + w, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (need) stage1(c0 * TS);  // the first super-chunk's DMA is in flight across the barrier
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();
    // Wave priority: the range composites are what later waves wait for, so phase 1 runs above
    // every phase 3 (left to age arbitration wave 0's phase 3 held back the phase 1 of the waves
    // sharing its SIMD: p1 done at 4.6 us median, 9.7 us max, r05ao); in phase 3 the waves that
    // started last (higher w: longer waits) go first.  Speed only.
    __builtin_amdgcn_s_setprio(3);
    if (need) {
        for (int sc = 0; sc < K; sc += C1) {
            if (sc > 0) {
                __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the previous super-chunk is read
                stage1((c0 + sc) * TS);
            }
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
            if (sc == 0) VASR_SPLIT_STAMP(1);
#pragma unroll 1
            for (int li = 0; li < C1; ++li) {
                const int lc = sc + li;
                const Smem sm{reg + li * TS * DPW, reg + S1 * DPW + li * TS * DPW, reg + SL1P + li * TS * N, yp};
                const StepIn r0 = load_step<0, N, DPW, FMA, N>(sm, dl, g);
                const StepIn r1 = load_step<1, N, DPW, FMA, N>(sm, dl, g);
                const StepElem e0 = make_elem<FMA>(r0, A2);
                TreeChunk<0, MU, N, DPW, true, FMA, true, TS, N>::run(st, sm, r1, e0, A2, dl, g, TS, cha, chb, yv);
                if (lc + 1 < K) {
                    switch (__builtin_ctz(~lc)) {
                        case 0: split_push_j<0, MU, FMA, LG>(st, cha, chb); break;
                        case 1: if constexpr (KL > 1) split_push_j<1, MU, FMA, LG>(st, cha, chb); break;
                        case 2: if constexpr (KL > 2) split_push_j<2, MU, FMA, LG>(st, cha, chb); break;
                        case 3: if constexpr (KL > 3) split_push_j<3, MU, FMA, LG>(st, cha, chb); break;
                        case 4: if constexpr (KL > 4) split_push_j<4, MU, FMA, LG>(st, cha, chb); break;
                        default: if constexpr (KL > 5) split_push_j<5, MU, FMA, LG>(st, cha, chb); break;
                    }
                } else {
#pragma unroll
                    for (int p = 0; p < NP; ++p) ra[p] = cha[p], rb[p] = chb[p];
                    split_up<KL, MU, FMA, LG>(st, ra, rb);
                }
            }
        }
        // publish: the composite, then (release: its LDS writes complete first) the flag
#pragma unroll
        for (int p = 0; p < NP; ++p) seg[(w * NP + p) * 64 + lane] = make_float4(ra[p].x, ra[p].y, rb[p].x, rb[p].y);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        if (lane == 0) __hip_atomic_store(flg + w, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    VASR_SPLIT_STAMP(2);
    switch (min(2, w >> 2)) {
        case 0: __builtin_amdgcn_s_setprio(0); break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        default: __builtin_amdgcn_s_setprio(2); break;
    }
    // phase 3's first two chunks, in flight while the prefix is formed
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the region is read
    stage(c0 * TS, sb0);
    if (nloc > 1) stage((c0 + 1) * TS, sb1);

    // ---- prefix before chunk c0: the blocks of c0's binary decomposition, highest first.  Bit j
    // of w set: the block of ranges [((w >> j) - 1) 2^j, (w >> j) 2^j), its composite the pairwise
    // tree of their composites (the segment tree's merges: entry i of level j + 1 = merge(entries
    // 2i, 2i + 1 of level j)), formed by this wave as soon as the ranges before it have published
    // (no workgroup barrier: wave 0 starts phase 3 at once, wave w waits only for waves < w).
    for (int v = 0; v < w; ++v)
        while (__hip_atomic_load(flg + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");  // the seg loads below see the published composites
    f2 pah[NP], pbh[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        pah[p] = f2{1.0f, 1.0f};
        pbh[p] = f2{0.0f, 0.0f};
    }
#pragma unroll
    for (int j = Lay::LOGSW - 1; j >= 0; --j) {
        if ((w >> j) & 1) {
            const int s0 = ((w >> j) - 1) << j;
            constexpr int MB = 1 << (Lay::LOGSW - 1);  // largest block (ranges)
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                float4 e[MB];
#pragma unroll
                for (int i = 0; i < MB; ++i)
                    if (i < (1 << j)) e[i] = seg[((s0 + i) * NP + p) * 64 + lane];
#pragma unroll
                for (int h = 1; h < MB; h <<= 1)
                    if (h < (1 << j)) {
#pragma unroll
                        for (int i = 0; i + h < MB; i += 2 * h) {
                            const f2 la = {e[i].x, e[i].y}, lb = {e[i].z, e[i].w};
                            const f2 rra = {e[i + h].x, e[i + h].y}, rrb = {e[i + h].z, e[i + h].w};
                            const f2 ob = mad2<FMA>(rra, lb, rrb);  // up-sweep: (a_r a_l, a_r b_l + b_r)
                            const f2 oa = rra * la;
                            e[i] = make_float4(oa.x, oa.y, ob.x, ob.y);
                        }
                    }
                pah[p] = pah[p] * f2{e[0].x, e[0].y};
                pbh[p] = mad2<FMA>(pah[p], f2{e[0].z, e[0].w}, pbh[p]);
            }
        }
    }

    VASR_SPLIT_STAMP(3);
    // ---- phase 3: the streaming kernel over chunks c0 .. c0 + nloc - 1
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        st.pa[p] = pah[p];
        st.pb[p] = pbh[p];
    }
    float* outp = out + (row0 + (int64_t)c0 * TS + t_thr) * ld_out + d0 + d_thr;
    if (nloc > 1) __builtin_amdgcn_s_waitcnt(WAIT_NI);  // chunk c0 landed (c0 + 1 may be in flight)
    else __builtin_amdgcn_s_waitcnt(0x0F70);
    VASR_SPLIT_STAMP(4);
    for (int lc = 0; lc < nloc; ++lc) {
        float* const buf = (lc & 1) ? sb1 : sb0;
        const int t0 = (c0 + lc) * TS;
        const int nvalid = min(TS, L - t0);
        if (lc >= 1 && lc + 1 < nloc) stage(t0 + TS, (lc & 1) ? sb0 : sb1);
        const Smem sm{buf, buf + TS * DPW, buf + Lay::SLABP, yp};
        const StepIn r0 = load_step<0, N, DPW, FMA>(sm, dl, g);
        const StepIn r1 = load_step<1, N, DPW, FMA>(sm, dl, g);
        const StepElem e0 = make_elem<FMA>(r0, A2);
        if (nvalid == TS) {
            TreeChunk<0, MU, N, DPW, true, FMA, false, TS>::run(st, sm, r1, e0, A2, dl, g, nvalid, cha, chb, yv);
        } else {
#pragma unroll
            for (int j = 0; j < TS; ++j) yv[j] = 0.0f;
            TreeChunk<0, MU, N, DPW, false, FMA, false, TS>::run(st, sm, r1, e0, A2, dl, g, nvalid, cha, chb, yv);
        }
        if (lc + 1 < nloc) {
            const int lc1 = lc + 1;
            switch (__builtin_ctz(~lc)) {
                case 0: if constexpr (KL > 0) split_merge_j<0, MU, FMA, LG>(st, cha, chb, lc1, pah, pbh); break;
                case 1: if constexpr (KL > 1) split_merge_j<1, MU, FMA, LG>(st, cha, chb, lc1, pah, pbh); break;
                case 2: if constexpr (KL > 2) split_merge_j<2, MU, FMA, LG>(st, cha, chb, lc1, pah, pbh); break;
                case 3: if constexpr (KL > 3) split_merge_j<3, MU, FMA, LG>(st, cha, chb, lc1, pah, pbh); break;
                case 4: if constexpr (KL > 4) split_merge_j<4, MU, FMA, LG>(st, cha, chb, lc1, pah, pbh); break;
                default: if constexpr (KL > 5) split_merge_j<5, MU, FMA, LG>(st, cha, chb, lc1, pah, pbh); break;
            }
        }
        // the next chunk landed and this chunk's partial sums are in the tile (vmcnt also counts
        // the previous chunk's output stores: see the streaming kernel)
        __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0) lgkmcnt(0)
        if (lane < TS * DPW && t_thr < nvalid) {
            const float ysum = yp[d_thr * (TS + 1) + t_thr];
            const float xv = sm.xs[t_thr * DPW + d_thr];
            const float zv = buf[2 * TS * DPW + t_thr * DPW + d_thr];
            const float y = ysum + xv * Dd;
            *outp = y * silu_of<MODE>(zv);
        }
        outp += TS * ld_out;
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): buf read before it is staged again
    }
#ifdef VASR_SCAN_STAMPS
    VASR_SPLIT_STAMP(5);
    __builtin_amdgcn_s_waitcnt(0x0F70);
    VASR_SPLIT_STAMP(6);
    if (lane == 0 && g_scan_stamps) {
        uint32_t xcc, hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        int64_t* o = g_scan_stamps + 8 * ((int64_t)blockIdx.x * SWM + w);
        o[0] = (int64_t)(xcc & 0xF) | ((int64_t)hw << 8);
#pragma unroll
        for (int i = 0; i < 7; ++i) o[1 + i] = stamp[i];
    }
#endif
#undef VASR_SPLIT_STAMP
}

template <int N, int MODE>
int launch_split_n(const float* xz, int64_t ld_xz, const float* dt, int64_t ld_dt, const float* bc, int64_t ld_bc,
                   const float* A2, const float* D, float* out, int64_t ld_out, int B, int L, int Di, hipStream_t s) {
    using Lay = SplitLds<N>;
    if (Di % Lay::DPW != 0) {
        set_error("vasr_ssm_scan_chunked_f32: Di=%d must be a multiple of %d for N=%d", Di, Lay::DPW, N);
        return VASR_EUNSUPPORTED;
    }
    const int nch = (L + TS - 1) / TS;
    int kl = 0;
    while ((Lay::SWM << kl) < nch) ++kl;  // L <= 8192: kl <= 6
    const int sw = (nch + (1 << kl) - 1) >> kl;
    const dim3 grid((unsigned)(B * (Di / Lay::DPW))), block(64 * sw);
#define VASR_SPLIT(KLV)                                                                                              \
    hipLaunchKernelGGL((ssm_scan_split_kernel<N, MODE, KLV>), grid, block, 0, s, xz, ld_xz, dt, ld_dt, bc, ld_bc, A2, \
                       D, out, ld_out, B, L, Di)
    switch (kl) {
        case 0: VASR_SPLIT(0); break;
        case 1: VASR_SPLIT(1); break;
        case 2: VASR_SPLIT(2); break;
        case 3: VASR_SPLIT(3); break;
        case 4: VASR_SPLIT(4); break;
        case 5: VASR_SPLIT(5); break;
        default: VASR_SPLIT(6); break;
    }
#undef VASR_SPLIT
    return launch_status("vasr_ssm_scan_chunked_f32");
}
