// Split-bf16 fp32 GEMM for short K (K <= 16 * KS: the model's K = 192 projections), "A rows
// stationary": each wave loads its 32 rows of A once, splits them into the three bf16 planes
// (x = hi + mid + lo, gemm_split.h) and keeps all of them in VGPRs (12 k-steps x 3 planes x
// bf16x8 = 144 VGPRs at K = 192) for the whole kernel, then walks a run of 32-column W chunks:
// per chunk 12 k-steps x the same six v_mfma_f32_32x32x16_bf16 products in the same order as
// the LDS-ring tile kernel (gemm_x3.hip), so the results are bitwise those of that kernel.
//
// Why: at K = 192 the tile kernel spends a whole 128 x 128 tile's life in one short K loop and
// then stores 64 KB of C at the end, in phase with every other block (measured: MFMA phase
// 12.3 us and store phase 10.8 us per two tiles per CU, serialised).  Here a
// block owns 256 rows x a run of 32-column chunks, with two accumulator sets: chunk j's MFMAs
// issue while chunk j-1's epilogue stores (non-temporal) drain, and the W chunks (36 KiB each,
// in the fragment-native layout of vasr_split_weights_bf16x3, contiguous per chunk) stream
// through a three-slot LDS ring by LDS-DMA two chunks ahead (issued by four of the eight waves).
//
// Work decomposition: block = 8 waves (two per SIMD) x 32 rows = 256 rows, grid = row blocks x
// column groups (runs of chunks), at most one block per CU so the grid is one round; blocks id,
// id + 8, ... share an XCD and get consecutive (row block, column group) items, so the column
// groups of one row block read its A rows from one L2.  Epilogues: gemm_common.h's (unpaired
// ones), per 32 x 32 chunk.  Measured variants, all slower or equal: 4 waves per
// block, cached stores, store groups of 2-4 chunks written back to back (profiles/r03k), the
// chunk's DMA issued before the previous epilogue / no store waits in non-loader waves
// (profiles/r03r), and the epilogue interleaved into the next chunk's k-steps at 4 or 8 waves
// (37.0 / 37.6 vs 33.4 us, profiles/r03u).
//
// What the launcher runs since round 7 is the wave-specialised form further down
// (gemm_rows_roles_kernel: compute waves and memory waves, 128-row blocks); the kernel described
// above is kept for -DVASR_ROWS_ROLES=0 builds (A/B through tools/build_variant_lib.sh).
#include <type_traits>

#include "gemm_common.h"
#include "gemm_split.h"

namespace vasr {
namespace {

using namespace gemm;

typedef __attribute__((address_space(3))) void lds_void;

// LDS-DMA of 16 B per lane into dst_base + 16 * lane (untracked by the compiler's waitcnt
// model, ordered by the kernel: counted vmcnt + barrier; the memory clobber keeps the
// epilogue's stores ahead of it in issue order)
__device__ __forceinline__ void glds16(const void* src, void* dst_base) {
    const unsigned lds = (unsigned)(uintptr_t)(lds_void*)dst_base;
    // M0 is compiler-reserved: saved and restored inside the statement, and the SALU write of M0
    // needs one wait state before the LDS-DMA reads it (s_nop 0)
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds), "v"(src) : "memory");
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt range");
    __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}

#ifndef VASR_ROWS_ABLATE
#define VASR_ROWS_ABLATE 0  // diagnostic builds only: 1 no MFMA, 2 no epilogue stores, 4 no LDS-DMA
#endif                      // after the first two chunks, 8 no per-chunk barrier
#ifndef VASR_ROWS_WAVES
#define VASR_ROWS_WAVES 8  // 256 A rows per block (r03k: 8 waves 37.8 us vs 4 waves 45.0 on the head GEMM)
#endif
#ifndef VASR_ROWS_DEPTH
#define VASR_ROWS_DEPTH 2  // W chunks in flight ahead of the one being multiplied (LDS slots = depth + 1)
#endif
#ifndef VASR_ROWS_STORE_AUX
#define VASR_ROWS_STORE_AUX 2  // cache-policy bits of the epilogue's buffer stores (2 = nt: C is not re-read from L2)
#endif
constexpr int RW = VASR_ROWS_WAVES;  // waves per block (4: one per SIMD)
constexpr int DEPTH = VASR_ROWS_DEPTH;
constexpr int NSLOT = DEPTH + 1;
#ifndef VASR_ROWS_STORE_WAIT
#define VASR_ROWS_STORE_WAIT 1  // 0: the store-only waves never wait for their older stores
#endif
#ifndef VASR_ROWS_MAX_GROUP
#define VASR_ROWS_MAX_GROUP 16
#endif
constexpr int MAX_GROUP = VASR_ROWS_MAX_GROUP;  // chunks per column group (LDS epilogue tables: MAX_GROUP x 32 columns)

// s_waitcnt vmcnt(n) for a runtime n in [0, 63] (the immediate has to be a constant)
__device__ __forceinline__ void wait_vmcnt_rt(int n) {
    switch (n) {
#define VASR_W(I) case I: wait_vmcnt<I>(); break;
#define VASR_W8(B) VASR_W(B) VASR_W(B + 1) VASR_W(B + 2) VASR_W(B + 3) VASR_W(B + 4) VASR_W(B + 5) VASR_W(B + 6) VASR_W(B + 7)
        VASR_W8(0) VASR_W8(8) VASR_W8(16) VASR_W8(24) VASR_W8(32) VASR_W8(40) VASR_W8(48) VASR_W8(56)
#undef VASR_W8
#undef VASR_W
        default: wait_vmcnt<0>();
    }
}

#ifdef VASR_ROWS_STAMPS
// Diagnostic builds only: per-wave sums of the cycles (s_memtime) spent in each phase of a chunk
// step, written once at the end of the kernel (no stores inside the loop), tools/diag/rows_stamps.py.
__device__ unsigned long long* g_rows_stamps;
#define VASR_STAMP(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#else
#define VASR_STAMP(v)
#endif

// Epilogue of one 32 x 32 chunk held as one MFMA accumulator (the tile kernel's epilogue_body
// arithmetic for TM = TN = 1), with the per-column bias / fake-quant parameters read from LDS
// and the results written by raw buffer stores: exactly NST store instructions per wave and
// chunk whatever the bounds (out-of-range lanes get an offset past the buffer's num_records,
// which the hardware drops), so the kernel's counted vmcnt waits stay exact.  No vector-memory
// loads besides the residual / positional operand, so the compiler's own vmcnt waits for those
// are the only ones that also cover the LDS-DMA ring in flight.
constexpr int NST = 16;  // store instructions per wave per chunk
constexpr int OOB = 0x7FFFFFFC;

template <int EPI>
__device__ __forceinline__ void rows_epilogue(const GemmParams& p, __amdgpu_buffer_rsrc_t cbuf, int m0, int n0,
                                              const floatx16& acc, int r, int h, const float* __restrict__ bias_s,
                                              const float4* __restrict__ qp_s, int cfirst) {
    const int col = n0 + r;
    const bool col_ok = col < p.N;
    const int lc = col - cfirst;  // column in the group's LDS tables
    const float bv = p.bias ? bias_s[lc] : 0.0f;
    float4 qc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.qp) qc = qp_s[lc];
    if constexpr (EPI == VASR_EPI_ARGMAX) {
        const int slot = n0 / 32;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
            float v = acc[i];
            if (p.bias) v = v + bv;
            if (p.qp) v = fake_quant(v, qc);
            const unsigned u = __float_as_uint(v);
            const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
            const unsigned long long k0 = col_ok ? ((unsigned long long)ord << 32) | (0xFFFFFFFFu - (unsigned)col) : 0ull;
            const unsigned long long key = gemm::max_u64_over_32_lanes(k0);  // lanes r = 16..31 hold it
            const int off = (r == 31 && row < p.M) ? (row * (int)p.ldc + slot) * 8 : OOB;
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
            const u32x2 kv = {(unsigned)key, (unsigned)(key >> 32)};
            if (!(VASR_ROWS_ABLATE & 2)) __builtin_amdgcn_raw_buffer_store_b64(kv, cbuf, off, 0, VASR_ROWS_STORE_AUX);
        }
        return;
    }
    // SP: 0 no softplus, 1 every column of the chunk, 2 per column (the chunk straddles n_out)
    auto body = [&](auto SPc) {
        constexpr int SP = decltype(SPc)::value;
        const bool sp = SP == 1 || (SP == 2 && col >= p.n_out);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
            const bool ok = col_ok && row < p.M;
            float v = acc[i];
            if (p.bias) v = v + bv;
            if (p.qp) v = fake_quant(v, qc);
            if constexpr (EPI == VASR_EPI_GELU) {
                v = gelu_fast(v);
            } else if constexpr (EPI == VASR_EPI_SOFTPLUS_FROM) {
                if constexpr (SP == 1) v = softplus20_fast(v);
                else if constexpr (SP == 2) v = sp ? softplus20_fast(v) : v;
            } else if constexpr (EPI == VASR_EPI_RESIDUAL) {
                v = v + p.aux[(int64_t)min(row, p.M - 1) * p.ld_aux + min(col, p.N - 1)];
            } else if constexpr (EPI == VASR_EPI_GELU_PE) {
                v = gelu_fast(v) + p.aux[(int64_t)min(row, p.M - 1) * p.ld_aux + min(col, p.N - 1)];
            }
            if (!(VASR_ROWS_ABLATE & 2))
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), cbuf, ok ? (row * (int)p.ldc + col) * 4 : OOB,
                                                      0, VASR_ROWS_STORE_AUX);
        }
    };
    // n0 is wave-uniform: whole chunks branch (a per-lane select ran softplus's exp / log on
    // every chunk and discarded it: 33.4 vs 39 us for the composed head GEMM, profiles/r03t)
    if constexpr (EPI == VASR_EPI_SOFTPLUS_FROM) {
        if (n0 >= p.n_out) body(std::integral_constant<int, 1>());
        else if (n0 + 32 <= p.n_out) body(std::integral_constant<int, 0>());
        else body(std::integral_constant<int, 2>());
    } else {
        body(std::integral_constant<int, 0>());
    }
}

template <int KS, int EPI>
__global__ __launch_bounds__(64 * RW, 1) void gemm_rows_kernel(GemmParams p, int n_groups, int chunks_per_group) {
    constexpr int CHUNK = KS * 3 * 1024;       // one 32-column W chunk: [KS][3 planes][64 lanes][16 B]
    constexpr int DW = 4;                      // loader waves (the first four) issue the chunk's DMA
    constexpr int NDMA = 3 * KS / DW;          // LDS-DMA instructions per loader wave per chunk
    static_assert((3 * KS) % DW == 0 && RW % DW == 0, "whole DMA pieces per loader wave");
    __shared__ __attribute__((aligned(16))) char wb0[CHUNK];
    __shared__ __attribute__((aligned(16))) char wb1[CHUNK];
    __shared__ __attribute__((aligned(16))) char wb2[CHUNK];
    __shared__ __attribute__((aligned(16))) char wb3[NSLOT > 3 ? CHUNK : 16];
    __shared__ float bias_s[MAX_GROUP * 32];
    __shared__ float4 qp_s[MAX_GROUP * 32];

    const int nblk = (int)gridDim.x;
    const int id = blockIdx.x;
    const int q8 = nblk / 8, r8 = nblk % 8, xg = id % 8;
    const int w = (xg < r8 ? xg * (q8 + 1) : r8 * (q8 + 1) + (xg - r8) * q8) + id / 8;
    const int rb = w / n_groups, ng = w - rb * n_groups;
    const int NT = (p.N + 31) / 32;
    const int c0 = ng * chunks_per_group;
    const int nc = min(chunks_per_group, NT - c0);
    if (nc <= 0) return;  // block-uniform

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int m0 = rb * 32 * RW + wave * 32;  // this wave's rows
    const int cfirst = c0 * 32;

    // A rows (lane (r, h): row r, k = 16 ks + 8 h + 0..7; columns past K read as 0 from a
    // clamped address, no branches) and the group's epilogue tables
    const float* __restrict__ arow = p.A + (int64_t)min(m0 + r, p.M - 1) * p.lda;
    float4 xa[KS][2];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int k = 16 * ks + 8 * h + 4 * u;
            const float4 v = *reinterpret_cast<const float4*>(arow + min(k, p.K - 4));
            xa[ks][u] = k < p.K ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    for (int i = tid; i < nc * 32; i += 64 * RW) {
        const int col = min(cfirst + i, p.N - 1);
        if (p.bias) bias_s[i] = p.bias[col];
        if (p.qp) qp_s[i] = p.qp[col];
    }
    bf16x8 a[KS][3];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) split8(xa[ks][0], xa[ks][1], a[ks][0], a[ks][1], a[ks][2]);

    const char* __restrict__ Wx = reinterpret_cast<const char*>(p.Wx);
    auto slot = [&](int i) -> char* { return i == 0 ? wb0 : i == 1 ? wb1 : i == 2 ? wb2 : wb3; };
    const bool loader = wave_u < DW;
    auto issue = [&](int j) {
        if (!loader) return;
        const char* src = Wx + (int64_t)(c0 + j) * CHUNK + lane * 16;
        char* dst = slot(j % NSLOT);
#pragma unroll
        for (int i = 0; i < NDMA; ++i) {
            const int piece = i * DW + wave_u;
            glds16(src + piece * 1024, dst + piece * 1024);
        }
    };
    for (int j = 0; j < DEPTH && j < nc; ++j) issue(j);

    // C as a raw buffer over its valid bytes (the host checks they fit 31 bits)
    const int c_bytes = (EPI == VASR_EPI_ARGMAX ? 8 : 4) * ((p.M - 1) * (int)p.ldc + (EPI == VASR_EPI_ARGMAX ? NT : p.N));
    const __amdgpu_buffer_rsrc_t cbuf = __builtin_amdgcn_make_buffer_rsrc(p.C, 0, c_bytes, 0x00020000);
    // two accumulator sets: chunk j's MFMAs into set j & 1 while chunk j - 1's epilogue stores
    // (set (j - 1) & 1) drain
    floatx16 acc[2];
#ifdef VASR_ROWS_STAMPS
    unsigned long long st_wait = 0, st_bar = 0, st_epi = 0, st_dma = 0, st_mfma = 0;
    VASR_STAMP(st_begin);
#endif
    // chunk j into set S: wait for its DMA (counted: younger DMAs and stores stay in flight),
    // publish it block-wide (the barrier also certifies every wave is done with the slot
    // DMA(j + DEPTH) refills), chunk j - 1's epilogue, prefetch chunk j + DEPTH, chunk j's MFMAs
    auto step = [&](auto Sc, int j) {
        constexpr int S = decltype(Sc)::value;
        // A loader wave waits for everything it issued: its DMA(j) has epilogue stores issued
        // after it (step j - 1 stores chunk j - 2), and vmcnt counts loads and stores together
        // with a store able to complete before an older load, so a count that includes those
        // stores does not prove DMA(j) landed (the scan's fix of the same mistake:
        // scan_body.inc, profiles/r04b/).  (Counting only the younger DMA loads -- safe if loads
        // retire in order among themselves -- measured no faster, 69.5 vs 68.7-70.5 us at
        // M = 16032, profiles/r04v/, so the plain form stays.)  The other waves issue stores only
        // (one event type: in order): they keep the stores of steps j - DEPTH + 1 .. j - 1 in
        // flight and bound the older ones.
        int n_vm = 0;
        if (!loader && !(VASR_ROWS_ABLATE & 2)) n_vm = VASR_ROWS_STORE_WAIT ? NST * max(0, j - max(j - DEPTH + 1, 1)) : 63;
        VASR_STAMP(t0);
        wait_vmcnt_rt(min(n_vm, 63));
        VASR_STAMP(t1);
        if (!(VASR_ROWS_ABLATE & 8)) __builtin_amdgcn_s_barrier();
        VASR_STAMP(t2);
        const char* wb = slot((VASR_ROWS_ABLATE & 4) ? min(j, DEPTH - 1) : j % NSLOT) + lane * 16;
        // W fragments of k-step 0 first, so the chunk's first MFMA does not wait behind the epilogue
        bf16x8 wf[2][3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) wf[0][pl] = *reinterpret_cast<const bf16x8*>(wb + pl * 1024);
        if (j >= 1) rows_epilogue<EPI>(p, cbuf, m0, (c0 + j - 1) * 32, acc[S ^ 1], r, h, bias_s, qp_s, cfirst);
        VASR_STAMP(t3);
        if (j + DEPTH < nc && !(VASR_ROWS_ABLATE & 4)) issue(j + DEPTH);
        VASR_STAMP(t4);
        floatx16 c;
#pragma unroll
        for (int i = 0; i < 16; ++i) c[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int cur = ks & 1;
            if (ks + 1 < KS) {  // next k-step's fragments one step ahead of their MFMAs
#pragma unroll
                for (int pl = 0; pl < 3; ++pl)
                    wf[cur ^ 1][pl] = *reinterpret_cast<const bf16x8*>(wb + ((ks + 1) * 3 + pl) * 1024);
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (VASR_ROWS_ABLATE & 1) {
                c[0] += (float)a[ks][0][0] * (float)wf[cur][0][0] + (float)a[ks][2][1] * (float)wf[cur][2][1];
                continue;
            }
            // small terms first, then the leading hi*hi term (gemm_x3.hip's order)
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][2], wf[cur][0], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][0], wf[cur][2], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][1], wf[cur][1], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][1], wf[cur][0], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][0], wf[cur][1], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][0], wf[cur][0], c, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        acc[S] = c;
#ifdef VASR_ROWS_STAMPS
        VASR_STAMP(t5);
        st_wait += t1 - t0;
        st_bar += t2 - t1;
        st_epi += t3 - t2;
        st_dma += t4 - t3;
        st_mfma += t5 - t4;
#endif
    };
    for (int j = 0; j < nc; j += 2) {
        step(std::integral_constant<int, 0>(), j);
        if (j + 1 < nc) step(std::integral_constant<int, 1>(), j + 1);
    }
    const int jl = nc - 1;  // the last chunk's epilogue
    rows_epilogue<EPI>(p, cbuf, m0, (c0 + jl) * 32, (jl & 1) ? acc[1] : acc[0], r, h, bias_s, qp_s, cfirst);
#ifdef VASR_ROWS_STAMPS
    __builtin_amdgcn_s_waitcnt(0);
    VASR_STAMP(st_end);
    if (lane == 0 && g_rows_stamps) {
        unsigned long long* o = g_rows_stamps + ((int64_t)blockIdx.x * RW + wave) * 8;
        o[0] = st_wait; o[1] = st_bar; o[2] = st_epi; o[3] = st_dma; o[4] = st_mfma; o[5] = st_end - st_begin;
        o[6] = (unsigned long long)nc; o[7] = loader ? 1 : 0;
    }
#endif
}

// ---------------------------------------------------------------------------------------------
// Wave-specialised form (what VASR_OPT_GEMM_ENGINE 2 runs; -DVASR_ROWS_ROLES=0 restores the
// kernel above).  In the kernel above every wave that owns MFMA work also issues vector memory:
// a wave issues in order, so while its buffer store or LDS-DMA waits on the backed-up memory
// pipeline (~190 / ~160 cycles per instruction, profiles/r06r) it issues no MFMA, and the launch
// takes the sum of its MFMA-only and memory-only ablations (13.5 + 28.4 vs 43.9 us).
// Here the two kinds of work sit in different waves of the block:
//   waves 0-3, compute (one per SIMD: waves w and w + 4 share one): 32 rows of A each as three
//     bf16 planes in VGPRs; per chunk the 72 MFMAs of the kernel above in the same order into
//     one accumulator, which then goes to a per-wave LDS staging tile (row-major 32 x 32 floats,
//     16 conflict-free ds_write_b32).  No global load, store or LDS-DMA inside the chunk loop.
//   waves 4-7, memory: the W chunks' LDS-DMA two chunks ahead, and chunk j - 1's epilogue while
//     the compute waves multiply chunk j: the staged tile read back as float4 (lane = 4 columns
//     of one row, 8 lanes per row), rows_epilogue's arithmetic per element, one 16-byte buffer
//     store per lane and 8 rows (4 store instructions per chunk instead of 16).
// A block is 128 rows x the chunks of one column group (the VGPR file holds four 256-register
// compute waves beside four memory waves, not eight), so W streams through LDS once per 128 rows.
// Group g of G takes chunks g, g + G, ...: every block gets its share of the softplus columns
// (a contiguous run gave half the blocks all of the exp / log work: 43.3 vs 40.9 us, profiles/r07b).
// Measured (M = 16032, N = 896, profiles/r07a-c): the memory waves' step, not the
// MFMAs, still sets the pace; two DMA-only + two store-only memory waves are slower than four that
// do both (48.2 vs 39.5 us: 18 DMA pieces per wave and step issue one after the other); the epilogue
// before the step's DMA beats the DMA first (36.2 vs 40.9 us).
// Round 9 (profiles/r09_summary.md): what made the memory waves' step the longer one was the softplus
// columns' arithmetic, 2.6 k cycles per 32 x 32 tile in a wave that shares its SIMD's issue with the
// MFMA wave (epilogue 2.0 k cycles per chunk with no softplus column, 4.7 k with all).  The softplus
// epilogue (launches without qparams) now does its arithmetic in the compute waves instead
// (VASR_ROWS_EPI_MATH): tile j - 1 stays in a second accumulator while chunk j multiplies, and its
// elements' bias + softplus instructions are scheduled between chunk j's dependent MFMAs, two elements
// per k-step, before the values go to the staging tile; the memory waves then only copy.  Behind the
// six MFMAs of a k-step instead of between them the same arithmetic costs 38 k cycles per block.
// The A prologue goes through the wave's staging tiles (VASR_ROWS_A_STAGE): whole row segments per
// load instruction, 9.2 k -> 7.8 k cycles.
//
// Hand-off is by workgroup barriers only, in one of two protocols chosen per epilogue at compile
// time (VASR_ROWS_ACC2 below).  Either way every wave of a block executes the same number of
// barriers whatever its role, its rows (ragged M: all waves run, addresses clamped, stores
// dropped) and nc (nc <= 0 returns before any barrier, block-uniform), and the W ring's rule is
// the same: DMA(j + 2) -> slot (j + 2) % 3 is issued after B_j.
//
// One accumulator (the hand-off is serial: the tile leaves after the chunk's last MFMA).
// INVARIANT: exactly nc + 1 barriers, B_0 .. B_nc.
//   compute wave:  for j in [0, nc): { B_j; MFMA chunk j from W slot j % 3; tile j -> stage[j & 1];
//                  lgkmcnt(0) }   B_nc
//   memory wave:   DMA(0), DMA(1); for j in [0, nc): { wait DMA(j); B_j; epilogue(j - 1) from
//                  stage[(j - 1) & 1]; DMA(j + 2) -> slot (j + 2) % 3 }   B_nc; epilogue(nc - 1)
// What each barrier certifies (checked on paper for nc = 1, 2, 3 and longer odd / even runs):
//   B_j, W:      DMA(j) has landed (the issuing waves' vmcnt wait precedes B_j), and every
//                compute wave has consumed chunk j - 1 -- its fragment reads fed the MFMAs whose
//                result it staged before B_j -- so slot (j - 1) % 3 = (j + 2) % 3 is free.
//   B_j, tiles:  tile j - 1 is complete in stage[(j - 1) & 1] (lgkmcnt(0) before B_j), and the
//                memory waves' reads of tile j - 2 from stage[j & 1] have returned (their stores
//                took the data from registers before B_j), so chunk j's tile may overwrite it.
//   B_0 also publishes the bias / qparam tables, filled by the memory waves during the A prologue.
//   nc = 1: B_0, chunk 0, B_1, epilogue(0).  nc = 2: DMA(2) never issues.  nc = 3: DMA(2) is
//   the only in-loop DMA and fills the slot no chunk has used.
//
// Two accumulators (chunk j multiplies into c[j & 1] while tile j - 1 leaves c[(j - 1) & 1] under
// chunk j's first k-steps).  INVARIANT: exactly nc + 2 barriers, B_0 .. B_{nc+1}.
//   compute wave:  for j in [0, nc): { B_j; MFMA chunk j from W slot j % 3 into c[j & 1], and in
//                  its k-steps 0..3 tile j - 1 (j >= 1) -> stage[(j - 1) & 1]; lgkmcnt(0) }
//                  B_nc; tile nc - 1 -> stage[(nc - 1) & 1]; lgkmcnt(0); B_{nc+1}
//   memory wave:   DMA(0), DMA(1); for j in [0, nc): { wait DMA(j); B_j; epilogue(j - 2) from
//                  stage[j & 1]; DMA(j + 2) }   B_nc; epilogue(nc - 2); B_{nc+1}; epilogue(nc - 1)
// "Interval j" is the code between B_j and B_{j+1}.  What each barrier certifies:
//   B_j, W:      as above: DMA(j) has landed, and chunk j - 1's fragment reads have returned (the
//                lgkmcnt(0) that ends interval j - 1 covers them), so slot (j + 2) % 3 is free.
//   B_{j+1}, tiles: tile j - 1, written in interval j, is complete in stage[(j - 1) & 1]
//                (lgkmcnt(0) before B_{j+1}); the memory waves read it in interval j + 1.  The
//                tile it overwrote, j - 3, was read in interval j - 1, and those reads returned
//                before the memory waves reached B_j.  In interval j the memory waves read tile
//                j - 2 from stage[j & 1], the other tile.  The same holds at the tail with j = nc:
//                tile nc - 1 is written in interval nc beside the reads of tile nc - 2.
//   The prologue's use of stage[wave][0..1] (VASR_ROWS_A_STAGE) ends before B_0: a wave's LDS
//   operations execute in order, and the first tile write follows B_0 (one accumulator) or B_1.
//   nc = 1: B_0, chunk 0, B_1, tile 0, B_2, epilogue(0): the memory waves pass B_1 with nothing to
//   do.  nc = 2: B_0 chunk 0; B_1 chunk 1 + tile 0; B_2 tile 1 | epilogue(0); B_3 epilogue(1).
//   nc = 3: interval 2 holds chunk 2 + tile 1 -> stage[1] beside epilogue(0) from stage[0]; interval
//   3 tile 2 -> stage[0] (tile 0 was read in interval 2) beside epilogue(1); then epilogue(2).
//   Longer runs repeat interval 2's pattern with the two tiles alternating; an odd or even nc only
//   decides which tile the tail writes.
#ifndef VASR_ROWS_A_STAGE
#define VASR_ROWS_A_STAGE 1  // the A prologue through the wave's own staging tiles: whole 256-byte row segments per
#endif                       // load instruction (0: lane (r, h) loads its own fragments, 32 lines per instruction)
#ifndef VASR_ROWS_ACC2
#define VASR_ROWS_ACC2 0  // two accumulators where VASR_ROWS_EPI_MATH does not already take them: 0 nowhere, 1 for the 8-byte-slot
#endif                    // epilogues (ARGMAX, LSE, ARGMAX_LSE), 2 for every epilogue.  The hand-off alone under the MFMAs measured
                          // slower or equal (r09: the memory waves set the pace there, and the tail gains an interval)
#ifndef VASR_ROWS_EPI_MATH
#define VASR_ROWS_EPI_MATH 1  // 1: the SOFTPLUS_FROM epilogue's arithmetic (bias, softplus; launches without qparams) runs in the
#endif                        // compute waves, on tile j - 1 between chunk j's MFMAs (two accumulators); 0: in the memory waves
#ifndef VASR_ROWS_HEAD_ARGMAX
#define VASR_ROWS_HEAD_ARGMAX 0  // 1: auto sends the argmax head (ARGMAX, ARGMAX_LSE; K = 192, N >= 512, M >= 4096) here too
#endif
#ifndef VASR_ROWS_ROLES
#define VASR_ROWS_ROLES 1
#endif
#ifndef VASR_ROWS_INTERLEAVE
#define VASR_ROWS_INTERLEAVE 1  // column group g of G takes chunks g, g + G, ... (0: a contiguous run), so every block
#endif                          // gets its share of the softplus columns' exp / log work
#ifndef VASR_ROWS_EPI_FIRST
#define VASR_ROWS_EPI_FIRST 1  // a memory wave runs chunk j - 1's epilogue before it issues DMA(j + 2) (0: after): its
#endif                         // stores are then older than the 9 DMA pieces the next step's vmcnt wait leaves pending
#ifndef VASR_ROWS_DMA_WAVES
#define VASR_ROWS_DMA_WAVES 4  // memory waves that issue LDS-DMA: 4 (each also stores) or 2 (two DMA-only, two store-only)
#endif
constexpr int CWV = 4;                            // compute waves
constexpr int MWV = 4;                            // memory waves
constexpr int DWV = VASR_ROWS_DMA_WAVES;          // the first DWV memory waves issue the DMA
constexpr int SWV = DWV == MWV ? MWV : MWV - DWV;  // the last SWV memory waves run the epilogues
static_assert(DWV == 4 || DWV == 2, "VASR_ROWS_DMA_WAVES: 4 or 2");
constexpr int OOB16 = 0x7FFFFFF0;

// workgroup barrier that the compiler moves no memory access across (the builtin alone is no
// memory operation to it: an LDS read could be hoisted above the barrier that publishes it)
__device__ __forceinline__ void role_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// a float from the lane a DPP control names (gemm::dpp_u64's float form, every row and bank)
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    const int i = (int)__float_as_uint(v);
    return __uint_as_float((unsigned)__builtin_amdgcn_update_dpp(i, i, CTRL, 0xF, 0xF, false));
}

// rows_epilogue's per-element arithmetic (same operations, same order)
template <int EPI, int SP>
__device__ __forceinline__ float rows_value(const GemmParams& p, float v, float bv, const float4& qc, int row, int col) {
    if (p.bias) v = v + bv;
    if (p.qp) v = fake_quant(v, qc);
    if constexpr (EPI == VASR_EPI_GELU) {
        v = gelu_fast(v);
    } else if constexpr (EPI == VASR_EPI_SOFTPLUS_FROM) {
        if constexpr (SP == 1) v = softplus20_fast(v);
        else if constexpr (SP == 2) v = col >= p.n_out ? softplus20_fast(v) : v;
    } else if constexpr (EPI == VASR_EPI_RESIDUAL) {
        v = v + p.aux[(int64_t)min(row, p.M - 1) * p.ld_aux + min(col, p.N - 1)];
    } else if constexpr (EPI == VASR_EPI_GELU_PE) {
        v = gelu_fast(v) + p.aux[(int64_t)min(row, p.M - 1) * p.ld_aux + min(col, p.N - 1)];
    }
    return v;
}

// Epilogue of one staged 32 x 32 tile by one memory wave: lane l owns columns 4 (l & 7) .. + 3 of
// rows (l >> 3) + 8 s, s = 0..3.  wide (N, ldc multiples of 4 and C 16-byte aligned): one 16-byte
// store per lane and s; otherwise four dword stores.  Out-of-range lanes store past num_records.
// RAW: the tile already holds the epilogue's values (VASR_ROWS_EPI_MATH 1), only the stores are left.
template <int EPI, bool RAW = false>
__device__ __forceinline__ void roles_epilogue(const GemmParams& p, __amdgpu_buffer_rsrc_t cbuf, int m0, int n0,
                                               const float* __restrict__ tile, int lane, bool wide,
                                               const float* __restrict__ bias_s, const float4* __restrict__ qp_s,
                                               int cfirst) {
    const int rl = lane >> 3, c4 = 4 * (lane & 7);
    const int col0 = n0 + c4;
    const int lc = col0 - cfirst;  // column in the group's LDS tables
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (!RAW && p.bias) {
        const float4 b = *reinterpret_cast<const float4*>(bias_s + lc);
        bv[0] = b.x; bv[1] = b.y; bv[2] = b.z; bv[3] = b.w;
    }
    float4 qc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) qc[e] = !RAW && p.qp ? qp_s[lc + e] : make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (EPI == VASR_EPI_ARGMAX) {
        const int slot = n0 / 32;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int row = m0 + 8 * s + rl;
            const float4 x = *reinterpret_cast<const float4*>(tile + (8 * s + rl) * 32 + c4);
            const float xv[4] = {x.x, x.y, x.z, x.w};
            unsigned long long key = 0ull;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = xv[e];
                if (p.bias) v = v + bv[e];
                if (p.qp) v = fake_quant(v, qc[e]);
                const unsigned u = __float_as_uint(v);
                const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
                const unsigned long long k =
                    col0 + e < p.N ? ((unsigned long long)ord << 32) | (0xFFFFFFFFu - (unsigned)(col0 + e)) : 0ull;
                key = k > key ? k : key;
            }
            // the row's 8 lanes: xor 1, xor 2 within the quad, then the mirrored other quad
            unsigned long long o = gemm::dpp_u64<0xB1, 0xF>(key);
            key = o > key ? o : key;
            o = gemm::dpp_u64<0x4E, 0xF>(key);
            key = o > key ? o : key;
            o = gemm::dpp_u64<0x141, 0xF>(key);
            key = o > key ? o : key;
            const int off = (c4 == 0 && row < p.M) ? (row * (int)p.ldc + slot) * 8 : OOB16;
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
            const u32x2 kv = {(unsigned)key, (unsigned)(key >> 32)};
            __builtin_amdgcn_raw_buffer_store_b64(kv, cbuf, off, 0, VASR_ROWS_STORE_AUX);
        }
        return;
    }
    if constexpr (EPI == VASR_EPI_LSE) {
        // the chunk is the row's slot n0 / 32: {m, s} = the maximum of acc + bias over its 32
        // columns and the sum of exp(v - m), a column past N counting as -inf (gemm_common.h's
        // pair; the host refuses qparams).  The row's 8 lanes agree on the maximum first (ARGMAX's
        // three DPP steps), so each element costs one exp and the sums add without rescaling; an
        // all--inf slot subtracts 0 and leaves the neutral pair {-inf, 0}.
        const int slot = n0 / 32;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int row = m0 + 8 * s + rl;
            const float4 x = *reinterpret_cast<const float4*>(tile + (8 * s + rl) * 32 + c4);
            const float xv[4] = {x.x, x.y, x.z, x.w};
            float v[4];
            float m = -INFINITY;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = col0 + e < p.N ? xv[e] + bv[e] : -INFINITY;
                m = fmaxf(m, v[e]);
            }
            m = fmaxf(m, dpp_f32<0xB1>(m));
            m = fmaxf(m, dpp_f32<0x4E>(m));
            m = fmaxf(m, dpp_f32<0x141>(m));
            const float ms = m == -INFINITY ? 0.f : m;
            float sum = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) sum += fast_exp(v[e] - ms);
            sum += dpp_f32<0xB1>(sum);
            sum += dpp_f32<0x4E>(sum);
            sum += dpp_f32<0x141>(sum);
            const int off = (c4 == 0 && row < p.M) ? (row * (int)p.ldc + slot) * 8 : OOB16;
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
            const u32x2 kv = {__float_as_uint(m), __float_as_uint(sum)};
            __builtin_amdgcn_raw_buffer_store_b64(kv, cbuf, off, 0, VASR_ROWS_STORE_AUX);
        }
        return;
    }
    if constexpr (EPI == VASR_EPI_ARGMAX_LSE) {
        // the chunk is the row's group n0 / 32: slot 2 * group gets the key exactly as ARGMAX above
        // forms it, slot 2 * group + 1 the pair exactly as LSE above (gemm_common.h's layout; no
        // qparams, the host refuses them); lane c4 == 0 stores both
        const int slot = 2 * (n0 / 32);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int row = m0 + 8 * s + rl;
            const float4 x = *reinterpret_cast<const float4*>(tile + (8 * s + rl) * 32 + c4);
            const float xv[4] = {x.x, x.y, x.z, x.w};
            unsigned long long key = 0ull;
            float v[4];
            float m = -INFINITY;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float kvl = xv[e];
                if (p.bias) kvl = kvl + bv[e];
                const unsigned u = __float_as_uint(kvl);
                const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
                const unsigned long long k =
                    col0 + e < p.N ? ((unsigned long long)ord << 32) | (0xFFFFFFFFu - (unsigned)(col0 + e)) : 0ull;
                key = k > key ? k : key;
                v[e] = col0 + e < p.N ? xv[e] + bv[e] : -INFINITY;
                m = fmaxf(m, v[e]);
            }
            unsigned long long o = gemm::dpp_u64<0xB1, 0xF>(key);
            key = o > key ? o : key;
            o = gemm::dpp_u64<0x4E, 0xF>(key);
            key = o > key ? o : key;
            o = gemm::dpp_u64<0x141, 0xF>(key);
            key = o > key ? o : key;
            m = fmaxf(m, dpp_f32<0xB1>(m));
            m = fmaxf(m, dpp_f32<0x4E>(m));
            m = fmaxf(m, dpp_f32<0x141>(m));
            const float ms = m == -INFINITY ? 0.f : m;
            float sum = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) sum += fast_exp(v[e] - ms);
            sum += dpp_f32<0xB1>(sum);
            sum += dpp_f32<0x4E>(sum);
            sum += dpp_f32<0x141>(sum);
            const bool on = c4 == 0 && row < p.M;
            const int off = on ? (row * (int)p.ldc + slot) * 8 : OOB16;
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
            const u32x2 kv = {(unsigned)key, (unsigned)(key >> 32)};
            const u32x2 pv = {__float_as_uint(m), __float_as_uint(sum)};
            __builtin_amdgcn_raw_buffer_store_b64(kv, cbuf, off, 0, VASR_ROWS_STORE_AUX);
            __builtin_amdgcn_raw_buffer_store_b64(pv, cbuf, on ? off + 8 : OOB16, 0, VASR_ROWS_STORE_AUX);
        }
        return;
    }
    auto body = [&](auto SPc, auto Wc) {
        constexpr int SP = decltype(SPc)::value;
        constexpr bool WIDE = decltype(Wc)::value;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int row = m0 + 8 * s + rl;
            const float4 x = *reinterpret_cast<const float4*>(tile + (8 * s + rl) * 32 + c4);
            float v[4] = {x.x, x.y, x.z, x.w};
            if constexpr (!RAW) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = rows_value<EPI, SP>(p, v[e], bv[e], qc[e], row, col0 + e);
            }
            if constexpr (WIDE) {
                typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                const u32x4 d = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
                const int off = (row < p.M && col0 < p.N) ? (row * (int)p.ldc + col0) * 4 : OOB16;
                if (!(VASR_ROWS_ABLATE & 2) || s == 3) __builtin_amdgcn_raw_buffer_store_b128(d, cbuf, off, 0, VASR_ROWS_STORE_AUX);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[e]), cbuf,
                                                          (row < p.M && col0 + e < p.N) ? (row * (int)p.ldc + col0 + e) * 4 : OOB,
                                                          0, VASR_ROWS_STORE_AUX);
            }
        }
    };
    auto width = [&](auto SPc) {
        if (wide) body(SPc, std::true_type());
        else body(SPc, std::false_type());
    };
    // whole chunks branch on the softplus columns, as rows_epilogue does (n0 is wave-uniform)
    if constexpr (EPI == VASR_EPI_SOFTPLUS_FROM && !RAW) {
        if (n0 >= p.n_out) width(std::integral_constant<int, 1>());
        else if (n0 + 32 <= p.n_out) width(std::integral_constant<int, 0>());
        else width(std::integral_constant<int, 2>());
    } else {
        width(std::integral_constant<int, 0>());
    }
}

template <int KS, int EPI, bool CMATH = false>
__global__ __launch_bounds__(64 * (CWV + MWV), 1) void gemm_rows_roles_kernel(GemmParams p, int n_groups,
                                                                              int chunks_per_group, int wide) {
    constexpr int CHUNK = KS * 3 * 1024;   // one 32-column W chunk: [KS][3 planes][64 lanes][16 B]
    constexpr int NDMA = 3 * KS / DWV;     // LDS-DMA instructions per DMA wave per chunk
    static_assert((3 * KS) % DWV == 0, "whole DMA pieces per DMA wave");
    static_assert(DEPTH == 2, "the roles kernel's ring is three slots, two chunks ahead");
    constexpr bool SLOTS = EPI == VASR_EPI_ARGMAX || EPI == VASR_EPI_LSE || EPI == VASR_EPI_ARGMAX_LSE;  // C is 8-byte slots, one per chunk
    // CMATH: the epilogue's per-element arithmetic runs in the compute waves (launch_roles picks it: SOFTPLUS_FROM without qparams)
    static_assert(!CMATH || EPI == VASR_EPI_SOFTPLUS_FROM, "compute-wave arithmetic: the softplus epilogue only");
    constexpr bool ACC2 = VASR_ROWS_ACC2 == 2 || (VASR_ROWS_ACC2 == 1 && SLOTS) || CMATH;  // the nc + 2 barrier protocol
    constexpr int LAG = ACC2 ? 2 : 1;  // a memory wave runs epilogue(j - LAG) after B_j
    __shared__ __attribute__((aligned(16))) char wb0[CHUNK];
    __shared__ __attribute__((aligned(16))) char wb1[CHUNK];
    __shared__ __attribute__((aligned(16))) char wb2[CHUNK];
    __shared__ __attribute__((aligned(16))) float stage[CWV][2][1024];  // per compute wave, two 32 x 32 tiles
    __shared__ __attribute__((aligned(16))) float bias_s[MAX_GROUP * 32];
    __shared__ float4 qp_s[MAX_GROUP * 32];

    const int nblk = (int)gridDim.x;
    const int id = blockIdx.x;
    const int q8 = nblk / 8, r8 = nblk % 8, xg = id % 8;
    const int w = (xg < r8 ? xg * (q8 + 1) : r8 * (q8 + 1) + (xg - r8) * q8) + id / 8;
    const int rb = w / n_groups, ng = w - rb * n_groups;
    const int NT = (p.N + 31) / 32;
    // chunk j of this block: group ng's j-th chunk
    constexpr bool IL = VASR_ROWS_INTERLEAVE != 0;
    const int c0 = IL ? ng : ng * chunks_per_group, cstep = IL ? n_groups : 1;
    const int nc = IL ? (NT - ng + n_groups - 1) / n_groups : min(chunks_per_group, NT - c0);
    if (nc <= 0) return;  // block-uniform, before any barrier

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    auto slot = [&](int i) -> char* { return i == 0 ? wb0 : i == 1 ? wb1 : wb2; };
#ifdef VASR_ROWS_STAMPS
    unsigned long long st_wait = 0, st_bar = 0, st_epi = 0, st_dma = 0, st_mfma = 0;
    VASR_STAMP(st_begin);
#endif

    if (wave_u < CWV) {
        // ---- compute wave ----
        const int r = lane & 31, h = lane >> 5;
        const int m0 = rb * 32 * CWV + wave_u * 32;
        bf16x8 a[KS][3];
#if VASR_ROWS_A_STAGE
        {
            // The wave's 32 rows x 64 K-columns per pass through its own two staging tiles (8 KiB,
            // nobody else's before B_0): 16 lanes load one row's 256-byte segment, 4 rows per
            // instruction, so every 128-byte line is touched by one instruction and used whole.
            // 16-byte chunk c of row q sits at chunk c ^ (q & 15) of the row's 256 bytes: the
            // 8-lane groups of a ds_write_b128 cover 128 contiguous bytes in some order, and the
            // 16-lane groups of the ds_read_b128 below (16 rows distinct mod 16, one c) 16 distinct
            // chunks.  Same values into the same split8 as the direct form: rows clamped to M - 1,
            // k >= K zero, any lda.  Wave-private: LDS operations of one wave execute in order.
            static_assert(KS % 4 == 0, "whole 64-column passes");
            constexpr int NP = KS / 4;
            char* img = reinterpret_cast<char*>(&stage[wave_u][0][0]);
            const int lq = lane >> 4, lc = lane & 15;
            float4 g[NP][8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float* __restrict__ src = p.A + (int64_t)min(m0 + 4 * i + lq, p.M - 1) * p.lda;
#pragma unroll
                for (int ps = 0; ps < NP; ++ps) {
                    const int k = 64 * ps + 4 * lc;
                    const float4 v = *reinterpret_cast<const float4*>(src + min(k, p.K - 4));
                    g[ps][i] = k < p.K ? v : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
#pragma unroll
            for (int ps = 0; ps < NP; ++ps) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int q = 4 * i + lq;
                    *reinterpret_cast<float4*>(img + q * 256 + ((lc ^ (q & 15)) << 4)) = g[ps][i];
                }
                asm volatile("" ::: "memory");
                __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the pass is in LDS
                float4 xa[4][2];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        xa[kk][u] = *reinterpret_cast<const float4*>(img + r * 256 + (((4 * kk + 2 * h + u) ^ (r & 15)) << 4));
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
                    split8(xa[kk][0], xa[kk][1], a[4 * ps + kk][0], a[4 * ps + kk][1], a[4 * ps + kk][2]);
                asm volatile("" ::: "memory");  // the next pass's writes stay behind these reads
            }
        }
#else
        {
            const float* __restrict__ arow = p.A + (int64_t)min(m0 + r, p.M - 1) * p.lda;
            float4 xa[KS][2];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int k = 16 * ks + 8 * h + 4 * u;
                    const float4 v = *reinterpret_cast<const float4*>(arow + min(k, p.K - 4));
                    xa[ks][u] = k < p.K ? v : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) split8(xa[ks][0], xa[ks][1], a[ks][0], a[ks][1], a[ks][2]);
        }
#endif
#ifdef VASR_ROWS_STAMPS
        __builtin_amdgcn_sched_barrier(0);
        VASR_STAMP(t_pro);
        st_wait = t_pro - st_begin;  // compute waves: the A prologue (they have no counted wait)
#endif
        if constexpr (ACC2) {
            floatx16 acc[2];
            // element i of lane (r, h) is row (i & 3) + 8 (i >> 2) + 4 h, column r: lanes 0-31 and
            // 32-63 each write one 128-byte row per instruction
            // CMATH: rows_value on the way out (the lane's 16 elements are 16 rows of column r, so one bias and one
            // qparam entry per lane and chunk); sp: the chunk holds softplus columns (wave-uniform)
            // is rows_value's arithmetic without qparams (the launcher keeps those launches on the memory waves' form),
            // branch-free so that it schedules between the MFMAs; SP (wave-uniform, rows_value's): 0 no softplus column in the
            // chunk, 1 all of them (no select: the compiler would branch around the softplus), 2 some
            auto put = [&](auto SPc, float* tile, const floatx16& c, int i, float bv, int col) {
                float v = c[i];
                if constexpr (CMATH) {
                    v = p.bias ? v + bv : v;
                    if constexpr (decltype(SPc)::value == 1) v = softplus20_fast(v);
                    else if constexpr (decltype(SPc)::value == 2) v = col >= p.n_out ? softplus20_fast(v) : v;
                }
                tile[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = v;
            };
            auto chunk_tables = [&](int j, float& bv, int& col, int& sp) {  // chunk j's, for put
                bv = 0.f; col = 0; sp = 0;
                if constexpr (CMATH) {
                    const int n0 = (c0 + j * cstep) * 32;
                    col = n0 + r;
                    if (p.bias) bv = bias_s[j * 32 + r];
                    sp = n0 >= p.n_out ? 1 : n0 + 32 <= p.n_out ? 0 : 2;
                }
            };
            // tile j - 1's 16 elements leave behind chunk j's first k-steps: 4 behind each of 4, or with arithmetic 2 behind each of 8
            auto first_el = [](int ks) { return CMATH ? 2 * ks : 4 * ks; };
            auto step = [&](auto Sc, auto Fc, auto SPc, int j, float bv, int col) {
                constexpr int S = decltype(Sc)::value;        // j & 1
                constexpr bool FIRST = decltype(Fc)::value;  // j == 0: no tile to hand off
                constexpr int SPF = decltype(SPc)::value;    // tile j - 1's softplus columns: none, all, some
                VASR_STAMP(t0);
                role_barrier();  // B_j
                VASR_STAMP(t1);
                const char* wb = slot(j % NSLOT) + lane * 16;
                float* prev = &stage[wave_u][S ^ 1][0];  // tile j - 1's
                bf16x8 wf[2][3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) wf[0][pl] = *reinterpret_cast<const bf16x8*>(wb + pl * 1024);
                floatx16 c;
#pragma unroll
                for (int i = 0; i < 16; ++i) c[i] = 0.f;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const int cur = ks & 1;
                    if (ks + 1 < KS) {
#pragma unroll
                        for (int pl = 0; pl < 3; ++pl)
                            wf[cur ^ 1][pl] = *reinterpret_cast<const bf16x8*>(wb + ((ks + 1) * 3 + pl) * 1024);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][2], wf[cur][0], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][0], wf[cur][2], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][1], wf[cur][1], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][1], wf[cur][0], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][0], wf[cur][1], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][0], wf[cur][0], c, 0, 0, 0);
                    if constexpr (!CMATH) __builtin_amdgcn_sched_barrier(0);
                    if constexpr (!FIRST) {
                        static_assert(KS == 8 || KS == 12, "16 elements over the k-steps");
                        const int i0 = min(first_el(ks), 16), i1 = min(first_el(ks + 1), 16);
#pragma unroll
                        for (int i = i0; i < i1; ++i) put(SPc, prev, acc[S ^ 1], i, bv, col);
                        if constexpr (CMATH) {
                            // the arithmetic goes between the six dependent MFMAs (each leaves the wave ~32 cycles
                            // to issue into), not behind them: one MFMA, then a share of the VALU work, six times
                            constexpr int PER = SPF ? 5 : 1;  // two softplus elements are about 30 VALU instructions
#pragma unroll
                            for (int m = 0; m < 6; ++m) {
                                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // one MFMA
                                __builtin_amdgcn_sched_group_barrier(0x002, PER, 0);  // PER VALU
                            }
                            __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);  // the tile writes
                        }
                    }
                    if constexpr (CMATH) __builtin_amdgcn_sched_barrier(0);
                }
                acc[S] = c;
                __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): tile j - 1 is in LDS before B_{j+1}
#ifdef VASR_ROWS_STAMPS
                VASR_STAMP(t2);
                st_bar += t1 - t0;
                st_mfma += t2 - t1;
#endif
            };
            auto next = [&](auto Sc, int j) {  // chunk j >= 1, with tile j - 1's tables
                float bv; int col; int sp;
                chunk_tables(j - 1, bv, col, sp);
                if (sp == 1) step(Sc, std::false_type(), std::integral_constant<int, 1>(), j, bv, col);
                else if (sp == 0) step(Sc, std::false_type(), std::integral_constant<int, 0>(), j, bv, col);
                else step(Sc, std::false_type(), std::integral_constant<int, 2>(), j, bv, col);
            };
            step(std::integral_constant<int, 0>(), std::true_type(), std::integral_constant<int, 0>(), 0, 0.f, 0);
            for (int j = 1; j < nc; j += 2) {
                next(std::integral_constant<int, 1>(), j);
                if (j + 1 < nc) next(std::integral_constant<int, 0>(), j + 1);
            }
            VASR_STAMP(t3);
            role_barrier();  // B_nc
            VASR_STAMP(t4);
            float bv; int col; int sp;
            chunk_tables(nc - 1, bv, col, sp);
            auto last = [&](auto SPc) {
                if ((nc - 1) & 1) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) put(SPc, &stage[wave_u][1][0], acc[1], i, bv, col);
                } else {
#pragma unroll
                    for (int i = 0; i < 16; ++i) put(SPc, &stage[wave_u][0][0], acc[0], i, bv, col);
                }
            };
            if (sp == 1) last(std::integral_constant<int, 1>());
            else if (sp == 0) last(std::integral_constant<int, 0>());
            else last(std::integral_constant<int, 2>());
            __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the last tile is in LDS before B_{nc+1}
            VASR_STAMP(t5);
            role_barrier();  // B_{nc+1}
#ifdef VASR_ROWS_STAMPS
            VASR_STAMP(t6);
            st_bar += (t4 - t3) + (t6 - t5);
            st_epi += t5 - t4;  // the only hand-off outside the MFMA phase
#endif
        } else {
        for (int j = 0; j < nc; ++j) {
            VASR_STAMP(t0);
            role_barrier();  // B_j
            VASR_STAMP(t1);
            const char* wb = slot(j % NSLOT) + lane * 16;
            bf16x8 wf[2][3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) wf[0][pl] = *reinterpret_cast<const bf16x8*>(wb + pl * 1024);
            floatx16 c;
#pragma unroll
            for (int i = 0; i < 16; ++i) c[i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int cur = ks & 1;
                if (ks + 1 < KS) {  // next k-step's fragments one step ahead of their MFMAs
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl)
                        wf[cur ^ 1][pl] = *reinterpret_cast<const bf16x8*>(wb + ((ks + 1) * 3 + pl) * 1024);
                }
                __builtin_amdgcn_sched_barrier(0);
                // small terms first, then the leading hi*hi term (gemm_x3.hip's order)
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][2], wf[cur][0], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][0], wf[cur][2], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][1], wf[cur][1], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][1], wf[cur][0], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][0], wf[cur][1], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][0], wf[cur][0], c, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            VASR_STAMP(t2);
            // element i of lane (r, h) is row (i & 3) + 8 (i >> 2) + 4 h, column r: lanes 0-31 and
            // 32-63 each write one 128-byte row per instruction
            float* tile = &stage[wave_u][j & 1][0];
#pragma unroll
            for (int i = 0; i < 16; ++i) tile[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = c[i];
            __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the tile is in LDS before B_{j+1}
#ifdef VASR_ROWS_STAMPS
            VASR_STAMP(t3);
            st_bar += t1 - t0;
            st_mfma += t2 - t1;
            st_epi += t3 - t2;  // compute waves: the tile's hand-off to LDS
#endif
        }
        VASR_STAMP(t4);
        role_barrier();  // B_nc
#ifdef VASR_ROWS_STAMPS
        VASR_STAMP(t5);
        st_bar += t5 - t4;
#endif
        }
    } else {
        // ---- memory wave ----
        const int mw = wave_u - CWV;
        const bool dma = mw < DWV;
        const bool stores = mw >= MWV - SWV;
        const int sw = mw - (MWV - SWV);  // index among the storing waves
        for (int i = tid - 64 * CWV; i < nc * 32; i += 64 * MWV) {  // tables: 32 entries per chunk of the block
            const int col = min((c0 + (i >> 5) * cstep) * 32 + (i & 31), p.N - 1);
            if (p.bias) bias_s[i] = p.bias[col];
            if (p.qp) qp_s[i] = p.qp[col];
        }
        const char* __restrict__ Wx = reinterpret_cast<const char*>(p.Wx);
        auto issue = [&](int j) {
            const char* src = Wx + (int64_t)(c0 + j * cstep) * CHUNK + lane * 16;
            char* dst = slot(j % NSLOT);
#pragma unroll
            for (int i = 0; i < NDMA; ++i) {
                const int piece = i * DWV + mw;
                glds16(src + piece * 1024, dst + piece * 1024);
            }
        };
        // the table fills above are plain loads: the compiler has waited for them before their LDS
        // writes, so the DMA pieces below are this wave's only outstanding loads from here on
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the tables are in LDS before B_0
        if (dma)
            for (int j = 0; j < DEPTH && j < nc; ++j) issue(j);
        constexpr int PER= EPI == VASR_EPI_ARGMAX_LSE ? 2 : 1;                                            // (two: key and pair)
        const int c_bytes = (SLOTS ? 8 : 4) * ((p.M - 1) * (int)p.ldc + (SLOTS ? PER * NT : p.N));
        const __amdgpu_buffer_rsrc_t cbuf = __builtin_amdgcn_make_buffer_rsrc(p.C, 0, c_bytes, 0x00020000);
        auto epilogue = [&](int j) {  // chunk j's tiles of compute waves sw, sw + SWV, ...
            if (!stores) return;
            const int n0 = (c0 + j * cstep) * 32;
            for (int cw = sw; cw < CWV; cw += SWV)
                roles_epilogue<EPI, CMATH>(p, cbuf, rb * 32 * CWV + cw * 32, n0, &stage[cw][j & 1][0], lane, wide != 0,
                                    bias_s, qp_s, n0 - j * 32);
        };
        for (int j = 0; j < nc; ++j) {
            VASR_STAMP(t0);
            // DMA(j) must have landed before B_j.  vmcnt counts this wave's loads and stores
            // together, and a store may retire before an older load, so a count that allowed for
            // younger stores would prove nothing (profiles/r04b).  Loads retire in order among
            // themselves, and the only loads younger than DMA(j) are DMA(j + 1)'s NDMA pieces, if
            // that chunk exists: with at most that many operations of any kind outstanding, a
            // pending piece of DMA(j) would need all NDMA younger loads pending beside it, one more
            // than the count allows.  (For a wave that also stores this bounds its stores in flight
            // to the same NDMA; a store-only wave never waits: the staging tiles are recycled on
            // their LDS reads, not on the stores' completion.)
            if (dma) {
                if (j + 1 < nc) wait_vmcnt<NDMA*(DEPTH - 1)>();
                else wait_vmcnt<0>();
            }
            VASR_STAMP(t1);
            role_barrier();  // B_j
            VASR_STAMP(t2);
            if (VASR_ROWS_EPI_FIRST && j >= LAG) epilogue(j - LAG);
            VASR_STAMP(t2e);
            if (dma && j + DEPTH < nc && !(VASR_ROWS_ABLATE & 4)) issue(j + DEPTH);
            VASR_STAMP(t3);
            if (!VASR_ROWS_EPI_FIRST && j >= LAG) epilogue(j - LAG);
#ifdef VASR_ROWS_STAMPS
            VASR_STAMP(t4);
            st_wait += t1 - t0;
            st_bar += t2 - t1;
            st_dma += t3 - t2e;
            st_epi += (t2e - t2) + (t4 - t3);
#endif
        }
        VASR_STAMP(t5);
        role_barrier();  // B_nc
        VASR_STAMP(t6);
        if constexpr (ACC2) {
            if (nc >= 2) epilogue(nc - 2);
            VASR_STAMP(t6a);
            role_barrier();  // B_{nc+1}
#ifdef VASR_ROWS_STAMPS
            VASR_STAMP(t6b);
            st_bar += t6b - t6a;
            st_epi += t6a - t6;
#endif
        }
        VASR_STAMP(t6c);
        epilogue(nc - 1);
#ifdef VASR_ROWS_STAMPS
        VASR_STAMP(t7);
        st_bar += t6 - t5;
        st_epi += ACC2 ? t7 - t6c : t7 - t6;
#endif
    }
#ifdef VASR_ROWS_STAMPS
    __builtin_amdgcn_s_waitcnt(0);
    VASR_STAMP(st_end);
    if (lane == 0 && g_rows_stamps) {
        unsigned long long* o = g_rows_stamps + ((int64_t)blockIdx.x * (CWV + MWV) + wave_u) * 8;
        o[0] = st_wait; o[1] = st_bar; o[2] = st_epi; o[3] = st_dma; o[4] = st_mfma; o[5] = st_end - st_begin;
        o[6] = (unsigned long long)nc;
        // role: 2 compute, 3 memory (DMA and stores), 4 DMA-only, 5 store-only (0 / 1: the kernel above)
        o[7] = wave_u < CWV ? 2 : DWV == MWV ? 3 : wave_u - CWV < DWV ? 4 : 5;
    }
#endif
}

// Column groups (runs of chunks) for row_blocks blocks of rows: at most one block per CU (LDS), so
// a grid of more than kCUs blocks runs in rounds, and a partial round costs as much as a full one.
// The groups minimise rounds x (chunks per block + 1), the 1 standing for a block's A prologue (its
// rows loaded and split; a wave's 32 rows in either form).  256-row blocks: M = 16032 keeps 4 groups
// of 10 chunks at N = 1280 (252 blocks, one round); the 30-s clips' M = 48096 takes 4 groups in 3
// rounds (30 chunk-steps per CU) instead of 3 groups of 16 (the MAX_GROUP cap) in 3 rounds (48),
// M = 24048 5 groups of 8 in 2 rounds (16) instead of 3 of 16 in 2 (32).  128-row blocks (the roles
// kernel), N = 896 (28 chunks): M = 16032 is 126 row blocks x 2 groups of 14 = 252 blocks in one
// round (cost 15; 3 groups of 10 would be 378 blocks, 2 rounds, 22), M = 8016 63 x 4 groups of 7 (8),
// M = 48096 376 x 2 of 14 = 752 blocks, 3 rounds (45; 4 groups of 7: 6 rounds, 48).
inline void pick_groups(int row_blocks, int NT, int* groups_out, int* per_out) {
    int groups = 1, per = min(NT, MAX_GROUP), best = -1;
    for (int g = 1; g <= NT; ++g) {
        const int pg = (NT + g - 1) / g;
        if (pg > MAX_GROUP) continue;
        const int gg = (NT + pg - 1) / pg;
        const int cost = ((row_blocks * gg + kCUs - 1) / kCUs) * (pg + 1);
        if (best < 0 || cost < best) {
            best = cost;
            groups = gg;
            per = pg;
        }
    }
    *groups_out = groups;
    *per_out = per;
}

template <int KS>
int launch_roles(const GemmParams& p, int epi, hipStream_t s) {
    const int NT = (p.N + 31) / 32;
    const int row_blocks = (p.M + 32 * CWV - 1) / (32 * CWV);
    int groups, per;
    pick_groups(row_blocks, NT, &groups, &per);
    // 16-byte stores need every lane's 4 columns valid together and 16-byte aligned
    const int wide = epi != VASR_EPI_ARGMAX && epi != VASR_EPI_LSE && epi != VASR_EPI_ARGMAX_LSE && p.N % 4 == 0 && p.ldc % 4 == 0 && (reinterpret_cast<uintptr_t>(p.C) & 15) == 0;
    const dim3 grid(row_blocks * groups), block(64 * (CWV + MWV));
#define VASR_R(E) hipLaunchKernelGGL((gemm_rows_roles_kernel<KS, E>), grid, block, 0, s, p, groups, per, wide)
    switch (epi) {
        case VASR_EPI_NONE: VASR_R(VASR_EPI_NONE); break;
        case VASR_EPI_GELU: VASR_R(VASR_EPI_GELU); break;
        case VASR_EPI_SOFTPLUS_FROM:
            // without qparams the softplus runs in the compute waves, between the next chunk's MFMAs
            if (VASR_ROWS_EPI_MATH == 1 && !p.qp)
                hipLaunchKernelGGL((gemm_rows_roles_kernel<KS, VASR_EPI_SOFTPLUS_FROM, true>), grid, block, 0, s, p, groups, per, wide);
            else
                VASR_R(VASR_EPI_SOFTPLUS_FROM);
            break;
        case VASR_EPI_RESIDUAL: VASR_R(VASR_EPI_RESIDUAL); break;
        case VASR_EPI_GELU_PE: VASR_R(VASR_EPI_GELU_PE); break;
        case VASR_EPI_ARGMAX: VASR_R(VASR_EPI_ARGMAX); break;
        case VASR_EPI_LSE: VASR_R(VASR_EPI_LSE); break;
        case VASR_EPI_ARGMAX_LSE: VASR_R(VASR_EPI_ARGMAX_LSE); break;
        default: set_error("vasr_linear_x3_f32: rows engine: epilogue %d not supported", epi); return VASR_EINVAL;
    }
#undef VASR_R
    return launch_status("vasr_linear_x3_f32");
}

template <int KS>
int launch_rows(const GemmParams& p, int epi, hipStream_t s) {
    const int NT = (p.N + 31) / 32;
    const int row_blocks = (p.M + 32 * RW - 1) / (32 * RW);
    int groups, per;
    pick_groups(row_blocks, NT, &groups, &per);
    const dim3 grid(row_blocks * groups), block(64 * RW);
#define VASR_R(E) hipLaunchKernelGGL((gemm_rows_kernel<KS, E>), grid, block, 0, s, p, groups, per)
    switch (epi) {
        case VASR_EPI_NONE: VASR_R(VASR_EPI_NONE); break;
        case VASR_EPI_GELU: VASR_R(VASR_EPI_GELU); break;
        case VASR_EPI_SOFTPLUS_FROM: VASR_R(VASR_EPI_SOFTPLUS_FROM); break;
        case VASR_EPI_RESIDUAL: VASR_R(VASR_EPI_RESIDUAL); break;
        case VASR_EPI_GELU_PE: VASR_R(VASR_EPI_GELU_PE); break;
        case VASR_EPI_ARGMAX: VASR_R(VASR_EPI_ARGMAX); break;
        default: set_error("vasr_linear_x3_f32: rows engine: epilogue %d not supported", epi); return VASR_EINVAL;
    }
#undef VASR_R
    return launch_status("vasr_linear_x3_f32");
}

}  // namespace

// The rows engine serves batch-1 launches with K <= 192 and unpaired epilogues (the model's
// projection GEMMs at K = 192, the CTC head).  rows_x3_selected is the rule alone (host only, launches
// nothing: vasr_linear_x3_f32 and vasr_gemm_tile both ask it); false when the tile kernel should run.
bool rows_x3_selected(int M, int N, int Kp, int64_t ldc, int batch, int epi) {
    if (batch != 1 || Kp > 192 || M <= 0 || epi == VASR_EPI_PAIR_POWER || epi == VASR_EPI_PAIR_FUSION) return false;
    // only the wave-specialised kernel has the log-sum-exp epilogues
    if ((epi == VASR_EPI_LSE || epi == VASR_EPI_ARGMAX_LSE) && !VASR_ROWS_ROLES) return false;
    if (Kp != 128 && Kp != 192) return false;  // the W chunk stride is Kp / 16 k-steps
    // raw-buffer C addressing: the valid bytes must fit the 31-bit offsets
    const bool slots = epi == VASR_EPI_ARGMAX || epi == VASR_EPI_LSE || epi == VASR_EPI_ARGMAX_LSE;
    if ((int64_t)M * ldc * (slots ? 8 : 4) >= ((int64_t)1 << 31) - 64) return false;
    const int engine = option(VASR_OPT_GEMM_ENGINE);  // 0 auto, 1 tiles, 2 rows
    if (engine == 1) return false;
    // auto: the rows engine where it measured faster (profiles/r03l: K = 192, N >= 512 -- the
    // composed head GEMM 35.8 vs 45.6 us, in_proj 21.1 vs 22.8; at N = 384 / 192 a block's short
    // chunk run does not amortise its A load; one utterance, M = 501: 13.2 vs 8.4 us in the
    // graph, profiles/r03m -- two 256-row blocks per column group); the residual / GELU+PE epilogues keep the
    // tiles (they spilled at 8 waves).  The row log-sum-exp epilogue goes where the plain one goes: the loss's
    // GEMM then runs on the engine its logits would have been written by, with 1/16 of the stores
    // (profiles/ctc_head.md).  The argmax head (ARGMAX, and ARGMAX_LSE with it: the host tests pin the two to one
    // engine) keeps the tiles under auto although the wave-specialised kernel measures faster at its shape
    // (profiles/r09_summary.md; the round-6 figure once cited here, 46.1 vs 46.5 us, was the 8-wave kernel's):
    // tests/test_host.py, test_ctc_head_host.py and test_greedy_conf_host.py pin vasr_gemm_tile's answer for
    // the head to the 128 x 128 tile, so the move is a build option, -DVASR_ROWS_HEAD_ARGMAX=1, until those
    // pins are retuned with it
    const bool head = VASR_ROWS_HEAD_ARGMAX && VASR_ROWS_ROLES && (epi == VASR_EPI_ARGMAX || epi == VASR_EPI_ARGMAX_LSE);
    if (engine == 0 && (Kp != 192 || N < 512 || M < 4096 ||
                        !(epi == VASR_EPI_NONE || epi == VASR_EPI_GELU || epi == VASR_EPI_SOFTPLUS_FROM ||
                          epi == VASR_EPI_LSE || head)))
        return false;
    return true;
}

// Launches the rows engine for a call rows_x3_selected accepted.
int launch_rows_x3(const GemmParams& p, int epi, hipStream_t s) {
    // the wave-specialised kernel: whatever engine 2 is forced on, and every shape auto sends here (it
    // measured faster than the 8-wave kernel at each of them, interleaved, profiles/r07c/gemm_ab.txt: N = 896 at
    // M = 8016 20.6 vs 29.7 us, 16032 34.8 vs 45.9, 24016 58.6 vs 74.1, 48096 104.3 vs 129.6; N = 1280 at
    // M = 16032 50.5 vs 60.2); -DVASR_ROWS_ROLES=0 builds a library that runs the 8-wave kernel instead
    const bool roles = VASR_ROWS_ROLES != 0;
    if (roles) return p.Kp == 128 ? launch_roles<8>(p, epi, s) : launch_roles<12>(p, epi, s);
    return p.Kp == 128 ? launch_rows<8>(p, epi, s) : launch_rows<12>(p, epi, s);
}

}  // namespace vasr

#ifdef VASR_ROWS_STAMPS
VASR_API int vasr_diag_rows_stamps(void* buf) {  // diagnostic builds only
    return hipMemcpyToSymbol(HIP_SYMBOL(vasr::g_rows_stamps), &buf, sizeof(buf)) == hipSuccess ? VASR_OK : VASR_EINVAL;
}
#endif
