// WER / CER scoring on the device: substitution, deletion and insertion counts of many independent
// pairs of int32 id sequences.  The rule is the one velocity_asr.training.edit_counts_host states; all
// arithmetic is integer, so the counts are the host's exactly.
//
// Rule.  c[i][j] = counts of hyp[:i] against ref[:j].  c[i][0] = i insertions, c[0][j] = j deletions.
//   hyp[i-1] == ref[j-1]: c[i][j] = c[i-1][j-1], unconditionally.  Otherwise the candidate of the
//   smallest S + D + I among substitution (c[i-1][j-1]), deletion (c[i][j-1]) and insertion (c[i-1][j]),
//   ties to the first in that order.
// Cell.  One 64-bit word: cost S + D + I in bits 48..63, S in 32..47, D in 16..31, I in 0..15.  Lengths
//   are at most 65535, so no field of a cell that reaches the result overflows; a step adds one constant.
// Sweep.  The reference lies on the columns.  A lane owns a strip of kEditStrip consecutive columns
//   in registers and takes row t - lane at step t: it needs its left neighbour's last cell of the same
//   row (made one step earlier) and of the row above (the cell it received the step before), and the
//   row's hypothesis item, which travels along the lanes with the cell.  Within a wave the hand-off is a
//   __shfl_up; between the waves of a workgroup one LDS slot per wave (two copies, by step parity) and
//   one barrier per step.  Columns past the reference's end hold values nothing to their left reads.
// Regimes.  edit_wave_kernel: one wave per pair of at most kEditWaveCols columns, no barrier.
//   edit_long_kernel: one workgroup per wider pair, in passes of kEditTileCols columns; the last column
//   of a pass is written to the workspace (one cell per row, two copies by pass parity) and is the left
//   boundary of the next.  Each kernel skips the other's pairs, so one call takes any mix.
//
// Alignment (vasr_edit_align_i32; the rule is training.edit_alignment_host's).  Both kernels have a
//   second instance (REC) that also keeps every cell's choice as a 2-bit code: 0 hit, 1 substitution,
//   2 deletion, 3 insertion.  A (row i, strip s) of kEditStrip columns is one 16-bit word, column k of
//   the strip in bits 2k, 2k + 1.  At a step every lane of a sweep works on the same anti-diagonal
//   i + s, so a pair's table is laid out by step: word (i, s) lies at ((i - 1 + s) mod m) * S + s, with
//   m rows and S = ceil(n / kEditStrip) strips.  For one s the m rows map to m different lines of S
//   words, so the table is exactly m * S words, and the words a wave stores at one step are contiguous
//   (row-major they would lie in 64 different rows).  Cells of row 0 and column 0 are not stored: their
//   choice is fixed.  edit_back_kernel then walks each pair from (m, n) with one wave, through a window
//   of kBackRows x kBackStrips words fetched into LDS by all lanes at once, and writes the codes in
//   forward order: the path has ref_len + I operations and I is in the counts already.
#include <cstdlib>

#include "vasr_internal.h"

namespace vasr {
namespace {

constexpr int kEditStrip = 8;                                   // columns per lane
constexpr int kEditWaveCols = kWave * kEditStrip;               // 512: widest pair of the one-wave form
constexpr int kEditWavePairs = 4;                               // pairs (waves) per workgroup of the one-wave form
constexpr int kEditLongThreads = 1024;
constexpr int kEditLongWaves = kEditLongThreads / kWave;
constexpr int kEditTileCols = kEditLongThreads * kEditStrip;    // 8192 columns per pass
constexpr int kEditLongGrid = 128;                              // workgroups of the long form: each owns a workspace slice
constexpr int kEditMaxLen = 65535;

typedef unsigned long long cell_t;
constexpr cell_t kCellSub = (1ull << 48) | (1ull << 32);
constexpr cell_t kCellDel = (1ull << 48) | (1ull << 16);
constexpr cell_t kCellIns = (1ull << 48) | 1ull;

__device__ __forceinline__ unsigned cell_cost(cell_t v) { return (unsigned)(v >> 48); }

__device__ __forceinline__ int edit_len(const int32_t* __restrict__ lens, int p, int mx) {
    const int n = lens[p];
    return n < 0 ? 0 : (n > mx ? mx : n);  // never read outside the row
}

__device__ __forceinline__ void edit_store(int32_t* __restrict__ out, cell_t v) {
    out[0] = (int)((v >> 32) & 0xffff);
    out[1] = (int)((v >> 16) & 0xffff);
    out[2] = (int)(v & 0xffff);
}

// The choice table of one pair (REC instances and the backtrace): bytes of m rows x ceil(n / kEditStrip)
// 16-bit words, and whether [off, off + extent) is a usable part of a table of `bytes` bytes.
__host__ __device__ __forceinline__ int64_t edit_table_extent(int m, int n) {
    return (int64_t)m * ((n + kEditStrip - 1) / kEditStrip) * (int64_t)sizeof(uint16_t);
}

__device__ __forceinline__ bool edit_table_ok(int64_t off, int m, int n, int64_t bytes) {
    return off >= 0 && (off & 1) == 0 && off <= bytes && edit_table_extent(m, n) <= bytes - off;
}

// The argument only the REC instances take: the sweeps end in a parameter pack that is this for REC and
// empty otherwise, so the counts-only instances keep the signature and the code they had without it.
struct EditTable {
    const int64_t* __restrict__ offset;  // (P,) byte offset of each pair's table
    char* __restrict__ base;
    int64_t bytes;
};

// The pair's table, or null when [offset[p], + extent) is no usable part of it.
__device__ __forceinline__ uint16_t* edit_table_of(const EditTable& tb, int p, int m, int n) {
    const int64_t off = tb.offset[p];
    return edit_table_ok(off, m, n, tb.bytes) ? reinterpret_cast<uint16_t*>(tb.base + off) : nullptr;
}
__device__ __forceinline__ uint16_t* edit_table_of(int, int, int) { return nullptr; }  // counts only

// One row of a strip: row[] holds the row above on entry and this row on return.  diag = the cell above
// the left boundary, left = the left boundary of this row.
// REC: returns the strip's eight choices, 2 bits each (0 hit, 1 substitution, 2 deletion, 3 insertion).
template <bool REC>
__device__ __forceinline__ unsigned strip_step(cell_t (&row)[kEditStrip], const int (&r)[kEditStrip], int h, cell_t diag,
                                               cell_t left) {
    unsigned word = 0;
#pragma unroll
    for (int k = 0; k < kEditStrip; ++k) {
        const cell_t up = row[k];
        cell_t best = diag + kCellSub;
        unsigned c = cell_cost(diag);
        unsigned code = 1;
        if (cell_cost(left) < c) best = left + kCellDel, c = cell_cost(left), code = 2;
        if (cell_cost(up) < c) best = up + kCellIns, code = 3;
        const bool hit = h == r[k];
        const cell_t v = hit ? diag : best;
        if (REC) word |= (hit ? 0u : code) << (2 * k);
        diag = up;
        row[k] = left = v;
    }
    return word;
}

// row[k] for a run-time k, as a chain of selects.  The empty asm keeps the compiler from folding the
// chain back into an indexed read of an array, which would move the strip out of registers into LDS.
__device__ __forceinline__ cell_t strip_pick(const cell_t (&row)[kEditStrip], int k) {
    cell_t v = row[0];
#pragma unroll
    for (int q = 1; q < kEditStrip; ++q) {
        cell_t x = row[q];
        asm volatile("" : "+v"(x));
        if (q == k) v = x;
    }
    return v;
}

// Strip of the columns base + 1 .. base + kEditStrip of a reference of n items: its items, row 0, and
// the cell above its left boundary.
__device__ __forceinline__ cell_t strip_init(cell_t (&row)[kEditStrip], int (&r)[kEditStrip], const int32_t* __restrict__ rp,
                                             int base, int n) {
#pragma unroll
    for (int k = 0; k < kEditStrip; ++k) {
        const int j = base + k + 1;
        r[k] = j <= n ? rp[j - 1] : 0;
        row[k] = (cell_t)j * kCellDel;
    }
    return (cell_t)base * kCellDel;
}

template <bool REC, typename... TB>
__global__ __launch_bounds__(kWave* kEditWavePairs) void edit_wave_kernel(
    const int32_t* __restrict__ hyp, int64_t ld_hyp, const int32_t* __restrict__ hyp_len, int max_hyp,
    const int32_t* __restrict__ ref, int64_t ld_ref, const int32_t* __restrict__ ref_len, int max_ref, int P,
    int32_t* __restrict__ counts, TB... tb) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int p = blockIdx.x * kEditWavePairs + wave;
    if (p >= P) return;  // no barrier in this kernel: a wave may leave
    const int m = edit_len(hyp_len, p, max_hyp), n = edit_len(ref_len, p, max_ref);
    if (n > kEditWaveCols) return;  // edit_long_kernel's pair
    int32_t* out = counts + 3 * (int64_t)p;
    if (m == 0 || n == 0) {  // all deletions or all insertions
        if (lane == 0) out[0] = 0, out[1] = n, out[2] = m;
        return;
    }
    const int32_t* hp = hyp + (int64_t)p * ld_hyp;
    const int32_t* rp = ref + (int64_t)p * ld_ref;
    int r[kEditStrip];
    cell_t row[kEditStrip];
    cell_t diag = strip_init(row, r, rp, lane * kEditStrip, n);
    const int lo = (n - 1) / kEditStrip;  // the lane that owns column n
    const int steps = m + lo;
    cell_t last = 0;
    int h = 0;
    // REC: this lane's word of step t lies in line (t - 1) mod m of the pair's table (null: a refused pair)
    uint16_t* tab = edit_table_of(tb..., p, m, n);
    if (tab) tab += lane;
    int line = 0;
    // hypothesis items 64 at a time, one ahead: lane 0 takes item t - 1 at step t
    int hcur = lane < m ? hp[lane] : 0;
    int hnext = kWave + lane < m ? hp[kWave + lane] : 0;
    for (int t = 1; t <= steps; ++t) {
        const int q = (t - 1) & (kWave - 1);
        if (q == 0 && t > 1) {
            hcur = hnext;
            const int i2 = t - 1 + kWave + lane;
            hnext = i2 < m ? hp[i2] : 0;
        }
        cell_t left = __shfl_up(last, 1, kWave);
        int hin = __shfl_up(h, 1, kWave);
        const int h0 = __shfl(hcur, q, kWave);
        if (lane == 0) left = (cell_t)t * kCellIns, hin = h0;
        h = hin;
        const int i = t - lane;
        if (i >= 1 && i <= m && lane <= lo) {
            const unsigned word = strip_step<REC>(row, r, h, diag, left);
            diag = left;
            last = row[kEditStrip - 1];
            if (REC && tab) tab[(int64_t)line * (lo + 1)] = (uint16_t)word;
        }
        if (REC && ++line == m) line = 0;
    }
    if (lane == lo) edit_store(out, strip_pick(row, n - 1 - lo * kEditStrip));
}

// grid: min(P, kEditLongGrid) workgroups; workgroup b takes the wide pairs among b, b + grid, ...
// ws: per workgroup two columns of max_hyp + 1 cells (NULL when max_ref fits one pass).
template <bool REC, typename... TB>
__global__ __launch_bounds__(kEditLongThreads) void edit_long_kernel(
    const int32_t* __restrict__ hyp, int64_t ld_hyp, const int32_t* __restrict__ hyp_len, int max_hyp,
    const int32_t* __restrict__ ref, int64_t ld_ref, const int32_t* __restrict__ ref_len, int max_ref, int P,
    int32_t* __restrict__ counts, cell_t* ws, TB... tb) {
    __shared__ cell_t slot_cell[2][kEditLongWaves];
    __shared__ int slot_h[2][kEditLongWaves];
    const int g = threadIdx.x, lane = g & (kWave - 1), wave = g / kWave;
    const int64_t col_cells = (int64_t)max_hyp + 1;
    for (int p = blockIdx.x; p < P; p += gridDim.x) {
        const int m = edit_len(hyp_len, p, max_hyp), n = edit_len(ref_len, p, max_ref);
        if (n <= kEditWaveCols) continue;  // edit_wave_kernel's pair (uniform over the workgroup)
        int32_t* out = counts + 3 * (int64_t)p;
        if (m == 0) {
            if (g == 0) out[0] = 0, out[1] = n, out[2] = 0;
            continue;
        }
        const int32_t* hp = hyp + (int64_t)p * ld_hyp;
        const int32_t* rp = ref + (int64_t)p * ld_ref;
        const int passes = (n + kEditTileCols - 1) / kEditTileCols;
        const int strips = (n + kEditStrip - 1) / kEditStrip;
        uint16_t* tab = edit_table_of(tb..., p, m, n);  // REC: this pair's table (null: a refused pair)
        for (int pass = 0; pass < passes; ++pass) {
            const int c0 = pass * kEditTileCols;
            const bool lastp = pass == passes - 1;
            // passes > 1 only with max_ref > kEditTileCols, and then the launcher has checked ws
            const cell_t* cin = pass > 0 ? ws + (2 * (int64_t)blockIdx.x + (pass & 1)) * col_cells : nullptr;
            cell_t* cout = !lastp ? ws + (2 * (int64_t)blockIdx.x + ((pass + 1) & 1)) * col_cells : nullptr;
            int r[kEditStrip];
            cell_t row[kEditStrip];
            cell_t diag = strip_init(row, r, rp, c0 + g * kEditStrip, n);
            const int glast = lastp ? (n - 1 - c0) / kEditStrip : kEditLongThreads - 1;  // last thread that works
            const int steps = m + glast;
            cell_t last = 0;
            int h = 0;
            // REC: strip pass * kEditLongThreads + g of step t lies in line (t - 1 + pass * kEditLongThreads) mod m
            int line = REC ? (pass * kEditLongThreads) % m : 0;
            uint16_t* tcol = REC && tab ? tab + pass * kEditLongThreads + g : nullptr;
            // wave 0: hypothesis items and the boundary column 64 at a time, one ahead
            int hcur = 0, hnext = 0;
            cell_t ccur = 0, cnext = 0;
            if (wave == 0) {
                hcur = lane < m ? hp[lane] : 0;
                hnext = kWave + lane < m ? hp[kWave + lane] : 0;
                if (pass > 0) {
                    ccur = 1 + lane <= m ? cin[1 + lane] : 0;
                    cnext = 1 + kWave + lane <= m ? cin[1 + kWave + lane] : 0;
                }
            }
            __syncthreads();  // the slots' last reads (previous pass or pair) are done
            for (int t = 1; t <= steps; ++t) {
                const int q = (t - 1) & (kWave - 1);
                if (wave == 0 && q == 0 && t > 1) {
                    hcur = hnext;
                    const int i2 = t - 1 + kWave + lane;
                    hnext = i2 < m ? hp[i2] : 0;
                    if (pass > 0) {
                        ccur = cnext;
                        cnext = i2 + 1 <= m ? cin[i2 + 1] : 0;
                    }
                }
                cell_t left = __shfl_up(last, 1, kWave);
                int hin = __shfl_up(h, 1, kWave);
                if (wave == 0) {
                    const int h0 = __shfl(hcur, q, kWave);
                    const cell_t cb = __shfl(ccur, q, kWave);
                    if (lane == 0) left = pass > 0 ? cb : (cell_t)t * kCellIns, hin = h0;
                } else if (lane == 0) {
                    left = slot_cell[(t - 1) & 1][wave - 1];
                    hin = slot_h[(t - 1) & 1][wave - 1];
                }
                h = hin;
                const int i = t - g;
                if (i >= 1 && i <= m && g <= glast) {
                    const unsigned word = strip_step<REC>(row, r, h, diag, left);
                    diag = left;
                    last = row[kEditStrip - 1];
                    if (!lastp && g == kEditLongThreads - 1) cout[i] = last;
                    if (REC && tcol) tcol[(int64_t)line * strips] = (uint16_t)word;
                }
                if (REC && ++line == m) line = 0;
                if (lane == kWave - 1) slot_cell[t & 1][wave] = last, slot_h[t & 1][wave] = h;
                __syncthreads();
            }
            if (lastp && g == glast) edit_store(out, strip_pick(row, n - 1 - c0 - glast * kEditStrip));
        }
    }
}

// The backtrace's window: kBackRows rows x kBackStrips strips of words ending at the walk's cell.  1 x 1 is
// the plain chain of one dependent load per operation (tools/align_time.py measures both).
#ifndef VASR_EDIT_BACK_ROWS
#define VASR_EDIT_BACK_ROWS 16
#endif
#ifndef VASR_EDIT_BACK_STRIPS
#define VASR_EDIT_BACK_STRIPS 16
#endif
constexpr int kBackRows = VASR_EDIT_BACK_ROWS;
constexpr int kBackStrips = VASR_EDIT_BACK_STRIPS;
constexpr int kBackWords = kBackRows * kBackStrips;
constexpr int kBackPairs = 4;  // pairs (waves) per workgroup

// One wave per pair, after the REC sweeps of the same call: walks the choices back from (m, n) and writes
// ops[p][0 .. K) in forward order, K = n + I = ops_len[p].  The walk is uniform over the wave: the lanes
// fetch a window of the table into LDS together, every lane reads the walk's word from it, lane 0 stores
// the operation.  Once a side is used up the rest is one run of deletions or insertions, filled by all lanes.
__global__ __launch_bounds__(kWave* kBackPairs) void edit_back_kernel(
    const int32_t* __restrict__ hyp_len, int max_hyp, const int32_t* __restrict__ ref_len, int max_ref, int P,
    const int32_t* __restrict__ counts, uint8_t* __restrict__ ops, int64_t ld_ops, int32_t* __restrict__ ops_len,
    EditTable tb) {
    __shared__ uint16_t win_all[kBackPairs][kBackWords];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int p = blockIdx.x * kBackPairs + wave;
    if (p >= P) return;  // no barrier in this kernel
    const int m = edit_len(hyp_len, p, max_hyp), n = edit_len(ref_len, p, max_ref);
    const uint16_t* __restrict__ tab = edit_table_of(tb, p, m, n);
    if (!tab) {
        if (lane == 0) ops_len[p] = -1;
        return;
    }
    const int K = n + counts[3 * (int64_t)p + 2];
    if (lane == 0) ops_len[p] = K;
    uint8_t* __restrict__ op = ops + (int64_t)p * ld_ops;
    uint16_t* win = win_all[wave];
    const unsigned S = (unsigned)(n + kEditStrip - 1) / kEditStrip;
    int i = m, j = n, pos = K - 1;
    int wi = 0, wsr = -1;  // the window holds rows (wi - kBackRows, wi] of strips (wsr - kBackStrips, wsr]
    while (i > 0 && j > 0 && pos >= 0) {
        const int s = (j - 1) / kEditStrip;
        if (i > wi || i <= wi - kBackRows || s > wsr || s <= wsr - kBackStrips) {
            wi = i, wsr = s;
            __builtin_amdgcn_wave_barrier();  // the reads of the window before are done
            for (int q = lane; q < kBackWords; q += kWave) {
                const int ii = wi - q / kBackStrips, ss = wsr - q % kBackStrips;
                if (ii >= 1 && ss >= 0) win[q] = tab[(int64_t)((unsigned)(ii - 1 + ss) % (unsigned)m) * S + ss];
            }
            __builtin_amdgcn_wave_barrier();
        }
        const unsigned word = win[(wi - i) * kBackStrips + (wsr - s)];
        const int code = __builtin_amdgcn_readfirstlane((word >> (2 * ((j - 1) & (kEditStrip - 1)))) & 3u);
        if (lane == 0) op[pos] = (uint8_t)code;
        --pos;
        i -= code != 2;
        j -= code != 3;
    }
    // i == 0: j deletions are left; j == 0: i insertions.  They are the path's first i + j = pos + 1 operations.
    const int rest = i + j < pos + 1 ? i + j : pos + 1;
    const uint8_t fill = i > 0 ? 3 : 2;
    for (int q = lane; q < rest; q += kWave) op[q] = fill;
}

int64_t edit_workspace_bytes(int P, int max_hyp, int max_ref) {
    if (P < 1 || P > kEditMaxLen || max_hyp < 0 || max_hyp > kEditMaxLen || max_ref < 0 || max_ref > kEditMaxLen) return -1;
    if (max_ref <= kEditTileCols) return 0;
    const int64_t grid = P < kEditLongGrid ? P : kEditLongGrid;
    return grid * 2 * ((int64_t)max_hyp + 1) * (int64_t)sizeof(cell_t);
}

// The two sweeps of one call; REC also fills the pairs' choice tables.
template <typename... TB>
int edit_sweep(const char* what, hipStream_t s, const int32_t* hyp, int64_t ld_hyp, const int32_t* hyp_len, int max_hyp,
               const int32_t* ref, int64_t ld_ref, const int32_t* ref_len, int max_ref, int P, int32_t* counts, cell_t* ws,
               TB... tb) {
    constexpr bool REC = sizeof...(TB) != 0;
    hipLaunchKernelGGL((edit_wave_kernel<REC, TB...>), dim3((unsigned)((P + kEditWavePairs - 1) / kEditWavePairs)),
                       dim3(kWave * kEditWavePairs), 0, s, hyp, ld_hyp, hyp_len, max_hyp, ref, ld_ref, ref_len, max_ref, P,
                       counts, tb...);
    int rc = launch_status(what);
    if (rc != VASR_OK || max_ref <= kEditWaveCols) return rc;
    hipLaunchKernelGGL((edit_long_kernel<REC, TB...>), dim3((unsigned)(P < kEditLongGrid ? P : kEditLongGrid)),
                       dim3(kEditLongThreads), 0, s, hyp, ld_hyp, hyp_len, max_hyp, ref, ld_ref, ref_len, max_ref, P, counts, ws,
                       tb...);
    return launch_status(what);
}

}  // namespace
}  // namespace vasr

VASR_API int vasr_edit_wave_cols(void) { return vasr::kEditWaveCols; }

VASR_API int vasr_edit_tile_cols(void) { return vasr::kEditTileCols; }

VASR_API int64_t vasr_edit_workspace_bytes(int P, int max_hyp, int max_ref) {
    return vasr::edit_workspace_bytes(P, max_hyp, max_ref);
}

VASR_API int vasr_edit_counts_i32(const int32_t* hyp, int64_t ld_hyp, const int32_t* hyp_len, int max_hyp,
                                  const int32_t* ref, int64_t ld_ref, const int32_t* ref_len, int max_ref, int P,
                                  int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream) {
    using namespace vasr;
    VASR_CHECK_ARG(hyp && hyp_len && ref && ref_len && counts, "vasr_edit_counts_i32: null pointer");
    VASR_CHECK_ARG(P >= 1 && P <= kEditMaxLen, "vasr_edit_counts_i32: 1 to 65535 pairs per call, got %d", P);
    VASR_CHECK_ARG(max_hyp >= 0 && max_ref >= 0, "vasr_edit_counts_i32: negative length (%d, %d)", max_hyp, max_ref);
    VASR_CHECK_ARG(max_hyp <= kEditMaxLen && max_ref <= kEditMaxLen,
                   "vasr_edit_counts_i32: at most 65535 items per sequence, got (%d, %d)", max_hyp, max_ref);
    VASR_CHECK_ARG(ld_hyp >= max_hyp, "vasr_edit_counts_i32: ld_hyp %lld < %d items", (long long)ld_hyp, max_hyp);
    VASR_CHECK_ARG(ld_ref >= max_ref, "vasr_edit_counts_i32: ld_ref %lld < %d items", (long long)ld_ref, max_ref);
    const int64_t need = edit_workspace_bytes(P, max_hyp, max_ref);
    VASR_CHECK_ARG(need == 0 || (workspace && workspace_bytes >= need),
                   "vasr_edit_counts_i32: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    VASR_CHECK_ARG(need == 0 || (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                   "vasr_edit_counts_i32: workspace is not 8-byte aligned");
    return edit_sweep("vasr_edit_counts_i32", as_stream(stream), hyp, ld_hyp, hyp_len, max_hyp, ref, ld_ref, ref_len, max_ref,
                      P, counts, need ? static_cast<cell_t*>(workspace) : nullptr);
}

VASR_API int64_t vasr_edit_align_table_bytes(int hyp_len, int ref_len) {
    using namespace vasr;
    if (hyp_len < 0 || hyp_len > kEditMaxLen || ref_len < 0 || ref_len > kEditMaxLen) return -1;
    return edit_table_extent(hyp_len, ref_len);
}

VASR_API int vasr_edit_align_i32(const int32_t* hyp, int64_t ld_hyp, const int32_t* hyp_len, int max_hyp,
                                 const int32_t* ref, int64_t ld_ref, const int32_t* ref_len, int max_ref, int P,
                                 int32_t* counts, uint8_t* ops, int64_t ld_ops, int32_t* ops_len,
                                 const int64_t* table_offset, void* table, int64_t table_bytes, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
    using namespace vasr;
    VASR_CHECK_ARG(hyp && hyp_len && ref && ref_len && counts && ops && ops_len && table_offset,
                   "vasr_edit_align_i32: null pointer");
    VASR_CHECK_ARG(P >= 1 && P <= kEditMaxLen, "vasr_edit_align_i32: 1 to 65535 pairs per call, got %d", P);
    VASR_CHECK_ARG(max_hyp >= 0 && max_ref >= 0, "vasr_edit_align_i32: negative length (%d, %d)", max_hyp, max_ref);
    VASR_CHECK_ARG(max_hyp <= kEditMaxLen && max_ref <= kEditMaxLen,
                   "vasr_edit_align_i32: at most 65535 items per sequence, got (%d, %d)", max_hyp, max_ref);
    VASR_CHECK_ARG(ld_hyp >= max_hyp, "vasr_edit_align_i32: ld_hyp %lld < %d items", (long long)ld_hyp, max_hyp);
    VASR_CHECK_ARG(ld_ref >= max_ref, "vasr_edit_align_i32: ld_ref %lld < %d items", (long long)ld_ref, max_ref);
    VASR_CHECK_ARG(ld_ops >= (int64_t)max_hyp + max_ref, "vasr_edit_align_i32: ld_ops %lld < %d + %d operations",
                   (long long)ld_ops, max_hyp, max_ref);
    VASR_CHECK_ARG(table && table_bytes >= 0, "vasr_edit_align_i32: table of %lld bytes at %p", (long long)table_bytes, table);
    VASR_CHECK_ARG((reinterpret_cast<uintptr_t>(table) & 1) == 0, "vasr_edit_align_i32: table is not 2-byte aligned");
    const int64_t need = edit_workspace_bytes(P, max_hyp, max_ref);
    VASR_CHECK_ARG(need == 0 || (workspace && workspace_bytes >= need),
                   "vasr_edit_align_i32: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    VASR_CHECK_ARG(need == 0 || (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                   "vasr_edit_align_i32: workspace is not 8-byte aligned");
    const EditTable tb{table_offset, static_cast<char*>(table), table_bytes};
    hipStream_t s = as_stream(stream);
    // VASR_EDIT_ALIGN_STAGE, for timing the two stages apart (tools/align_time.py): 1 runs the sweeps only, 2 the
    // walk only, over the table and the counts an earlier call left in the same buffers.
    const char* env = getenv("VASR_EDIT_ALIGN_STAGE");
    const int stage = env ? atoi(env) : 0;
    int rc = VASR_OK;
    if (stage != 2)
        rc = edit_sweep("vasr_edit_align_i32", s, hyp, ld_hyp, hyp_len, max_hyp, ref, ld_ref, ref_len, max_ref, P, counts,
                        need ? static_cast<cell_t*>(workspace) : nullptr, tb);
    if (rc != VASR_OK || stage == 1) return rc;
    hipLaunchKernelGGL(edit_back_kernel, dim3((unsigned)((P + kBackPairs - 1) / kBackPairs)), dim3(kWave * kBackPairs), 0, s,
                       hyp_len, max_hyp, ref_len, max_ref, P, counts, ops, ld_ops, ops_len, tb);
    return launch_status("vasr_edit_align_i32");
}
