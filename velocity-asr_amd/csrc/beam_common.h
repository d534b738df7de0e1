// The frame step of the CTC prefix beam search (reference velocity_asr/decode.py:128-217), once, for
// the three searches built on it: beam.hip's dense kernel over logits (log-softmax formed into LDS,
// optional bigram LM), the same kernel over ready log-probability rows, and beam_shortlist.hip's
// one-wave search over K shortlisted tokens per frame.  A search supplies a frame source -- the
// blank's log-probability and lookup(tok, v) -- and its candidates; everything exact lives here: the
// beam state, the merged records with their tie rules (beam_merge), the W maxima (beam_select), the
// new beam set and trie nodes (beam_commit), the write-out, and the row log-softmax that the dense
// kernel and the shortlist kernel share.
//
// One workgroup per utterance walks the frames.  The reference keys its beams by the collapsed prefix
// tuple; here each prefix is a node of a per-utterance trie (parent node, appended token) held in
// caller-owned workspace, so key equality is node equality: an extension prefix_i + (tok) equals a
// live beam j's prefix exactly when j's node has parent node_i and token tok.  Scores are float64 sums
// of float32 log-probabilities, as the reference's Python floats.
#pragma once
#include "vasr_internal.h"

namespace vasr {

// beam.hip: launches the dense search on checked arguments, B > 0.  lm_table != NULL: with the LM.
// out_uncertified != NULL: x holds ready log-probability rows, not logits (no LDS row, any V), and
// out_uncertified[b] = 0 is written -- the complete mode of vasr_ctc_beam_search_shortlist.
void beam_launch(const float* x, int64_t ld_row, int64_t ld_utt, int B, int L, int V, int W, int blank, const int32_t* frames,
                 const float* lm_table, int64_t ld_lm, double lm_weight, int32_t* trie, int32_t* out_tokens, int32_t* out_len,
                 double* out_score, int32_t* out_nbeams, int32_t* out_uncertified, void* stream);

namespace {

constexpr int kBeamThreads = 256;
constexpr int kMaxBeam = 32;
constexpr int kMaxStagedVocab = 16384;  // a row of log-probabilities in 64 KiB of LDS

// The checks every search entry makes; ptrs: the entry's own non-null test.
inline int beam_check_args(const char* who, bool ptrs, int B, int L, int V, int max_v, int W, int blank) {
    VASR_CHECK_ARG(ptrs, "%s: null pointer", who);
    VASR_CHECK_ARG(B >= 0 && L >= 0 && V >= 1 && V <= max_v && W >= 1 && W <= kMaxBeam && blank >= 0 && blank < V,
                   "%s: bad shape B=%d L=%d V=%d W=%d blank=%d", who, B, L, V, W, blank);
    return VASR_OK;
}

// Utterance b's row count.  The clamp is here because a device-resident count is taken without a host
// look at it.
__device__ __forceinline__ int beam_frames(const int32_t* frames, int b, int L) {
    return frames ? min(max(frames[b], 0), L) : L;
}

struct Cand {
    double s;
    long long idx;  // insertion position; -1 = none
};

__device__ __forceinline__ bool better(const Cand& a, const Cand& b) {  // a before b in the sorted order
    if (a.idx < 0) return false;
    if (b.idx < 0) return true;
    return a.s > b.s || (a.s == b.s && a.idx < b.idx);
}

__device__ Cand block_best(Cand c, Cand* red) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Cand d;
        d.s = __shfl_xor(c.s, o, 64);
        d.idx = __shfl_xor(c.idx, o, 64);
        if (better(d, c)) c = d;
    }
    if ((tid & 63) == 0) red[tid >> 6] = c;
    __syncthreads();
    Cand best = red[0];
    for (int w = 1; w < kBeamThreads / 64; ++w)
        if (better(red[w], best)) best = red[w];
    __syncthreads();
    return best;
}

template <int THREADS>
__device__ __forceinline__ Cand group_best(Cand c, Cand* red) {
    if (THREADS == kBeamThreads) return block_best(c, red);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // one wave: after the butterfly every lane holds the best
        Cand d;
        d.s = __shfl_xor(c.s, o, 64);
        d.idx = __shfl_xor(c.idx, o, 64);
        if (better(d, c)) c = d;
    }
    return c;
}

__device__ float block_reduce_f(float v, float* red, bool is_max) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float u = __shfl_xor(v, o, 64);
        v = is_max ? fmaxf(v, u) : v + u;
    }
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < kBeamThreads / 64; ++w) r = is_max ? fmaxf(r, red[w]) : r + red[w];
    __syncthreads();
    return r;
}

// log_softmax of a row by a 256-thread workgroup: mx its maximum, lse the log of the sum of
// exp(x - mx) (256 strided partials, xor butterfly, then the four waves left to right), a
// log-probability (x - mx) - lse.  STAGED: the row is copied into lp (LDS) and left there as its
// log-probabilities, with no barrier after the last pass; otherwise every pass reads the row itself.
// The one definition of these values: the searches agree bit for bit because they all come from here.
template <bool STAGED>
__device__ __forceinline__ void row_log_softmax(const float* __restrict__ row, int V, float* lp, float* fred, float& mx,
                                                float& lse) {
    const int tid = threadIdx.x;
    mx = -INFINITY;
    for (int v = tid; v < V; v += kBeamThreads) {
        const float x = row[v];
        if (STAGED) lp[v] = x;
        mx = fmaxf(mx, x);
    }
    mx = block_reduce_f(mx, fred, true);
    float se = 0.f;
    for (int v = tid; v < V; v += kBeamThreads) se += expf((STAGED ? lp[v] : row[v]) - mx);
    se = block_reduce_f(se, fred, false);
    lse = logf(se);
    if (STAGED)
        for (int v = tid; v < V; v += kBeamThreads) lp[v] = (lp[v] - mx) - lse;
}

// Shallow fusion with a bigram table, the reference's lm_scorer hook (decode.py:187-190): row 0 after
// the sentence start, row 1 + tail otherwise.
struct BeamLM {
    const float* table;
    int64_t ld;
    double weight;
    __device__ double entry(int tail, int tok) const { return (double)table[(int64_t)(tail + 1) * ld + tok]; }
};

// base + w * S as the reference forms it (token_score += lm_weight * lm_score): a product rounded
// to float64, then a sum.  Contraction is off here: a fused multiply-add skips the product's
// rounding and separates candidates that tie exactly in the reference.
__device__ __forceinline__ double add_lm(double base, double w, double S) {
#pragma clang fp contract(off)
    const double term = w * S;
    return base + term;
}

// A frame's log-probabilities by token index, in LDS or in global memory.
struct RowSource {
    const float* lp;
    int blank;
    __device__ float blank_lp() const { return lp[blank]; }
    __device__ int lookup(int tok, float& v) const {  // always found
        v = lp[tok];
        return 0;
    }
};

// The live beams of one utterance (LDS), in the reference's sorted order.  Beam j's prefix is trie node
// node[j] = (pnode[j], ptok[j]); S(prefix) of the LM is carried next to the prefix's tail token.
template <bool LM>
struct BeamState {
    double sc[kMaxBeam], msc[kMaxBeam];
    double lms[LM ? kMaxBeam : 1];  // S(prefix) of every live beam
    long long midx[kMaxBeam];
    int last[kMaxBeam], node[kMaxBeam], pnode[kMaxBeam], ptok[kMaxBeam], mlast[kMaxBeam];
    int src_of[kMaxBeam];   // beam i whose extension reaches beam j's node, or -1
    int slot_of[kMaxBeam];  // the frame source's slot of that extension's token, or -1
    int nb, nodes;
};

// The single empty beam and trie node 0; par / tk: the utterance's parent-node and token arrays.
template <bool LM>
__device__ void beam_init(BeamState<LM>& st, int32_t* par, int32_t* tk) {
    if (threadIdx.x == 0) {
        st.sc[0] = 0.0;
        st.lms[0] = 0.0;
        st.last[0] = -1;  // None
        st.node[0] = 0;
        st.pnode[0] = -1;
        st.ptok[0] = -1;
        par[0] = -1;
        tk[0] = -1;
        st.nb = 1;
        st.nodes = 1;
    }
    __syncthreads();
}

// Step 2.  For every live beam j, the merged record of its own key: its blank extension, its repeat
// of the last token, and the extension of the beam whose node is j's parent -- max score, the first
// candidate in the reference's insertion order winning ties (strict `<` update), and the key's
// insertion position = its first candidate's.  A token the source does not hold offers no score, but
// the parent extension still offers its position, which a search over every token would have used:
// the position is structural, min(j (V + 1), src (V + 1) + ptok_j + 1).  With an LM
// both non-blank candidates keep key j, so both carry lm_weight * S[j]; the blank gets no term.
template <bool LM, class Source>
__device__ __forceinline__ void beam_merge(BeamState<LM>& st, const Source& f, int nb, int V, int blank,
                                           double lm_weight) {
    const int j = threadIdx.x;
    const long long VP = (long long)V + 1;
    if (j < nb) {
        int src = -1;
        for (int i = 0; i < nb; ++i)
            if (st.node[i] == st.pnode[j] && st.ptok[j] != st.last[i]) src = i;
        st.src_of[j] = src;
    }
    __syncthreads();
    if (j < nb) {
        // candidates in insertion order: (src, ptok) if src < j, (j, blank), (j, last), (src, ptok) if src > j
        Cand best{0.0, -1};
        int bl = -1;
        long long first = -1;
        auto place = [&](long long idx) {
            if (first < 0 || idx < first) first = idx;
        };
        auto offer = [&](double s, long long idx, int lt) {
            place(idx);
            if (best.idx < 0 || s > best.s || (s == best.s && idx < best.idx)) {
                best.s = s;
                best.idx = idx;
                bl = lt;
            }
        };
        auto lm = [&](double s) { return LM ? add_lm(s, lm_weight, st.lms[j]) : s; };
        const int src = st.src_of[j], last = st.last[j], ptok = st.ptok[j];
        float v = 0.f;
        int at = -1;
        offer(st.sc[j] + (double)f.blank_lp(), (long long)j * VP, blank);
        if (last >= 0 && last != blank && f.lookup(last, v) >= 0)
            offer(lm(st.sc[j] + (double)v), (long long)j * VP + last + 1, last);
        if (src >= 0) {
            const long long idx = (long long)src * VP + ptok + 1;
            at = f.lookup(ptok, v);
            if (at >= 0)
                offer(lm(st.sc[src] + (double)v), idx, ptok);
            else
                place(idx);  // the full search inserts the key here, whatever the score
        }
        st.slot_of[j] = at;
        st.msc[j] = best.s;
        st.midx[j] = first;
        st.mlast[j] = bl;
    }
    __syncthreads();
}

// Step 3.  The W best of candidates 0 .. ncand - 1 (cand(c).idx < 0: none) in the order of the
// reference's stable sort, score descending, insertion position ascending: W successive group-wide
// maxima, each strictly below the previous winner.  Returns their number; lane r keeps winner r in
// mywin and every thread the last one in lastwin.
template <int THREADS, class CandFn>
__device__ __forceinline__ int beam_select(int ncand, int W, CandFn cand, Cand* red, Cand& mywin, Cand& lastwin) {
    const int tid = threadIdx.x;
    Cand prev{INFINITY, -2};
    mywin = Cand{0.0, -1};
    int nw = 0;
    for (int r = 0; r < W; ++r) {
        Cand mine{0.0, -1};
        for (int c = tid; c < ncand; c += THREADS) {
            const Cand k = cand(c);
            if (k.idx < 0) continue;
            // below the previous winner in the sorted order
            if (prev.idx != -2 && !(prev.s > k.s || (prev.s == k.s && prev.idx < k.idx))) continue;
            if (better(k, mine)) mine = k;
        }
        const Cand w = group_best<THREADS>(mine, red);
        if (w.idx < 0) break;
        if (tid == r) mywin = w;
        prev = w;
        ++nw;
    }
    lastwin = prev;
    return nw;
}

// Step 4.  The new beam set in winner order, lane r forming beam r from winner r: a surviving key
// keeps its merged record, a new extension gets a fresh trie node and, with an LM,
// S(child) = S(parent) + table[1 + tail(parent)][tok].
template <bool LM>
__device__ __forceinline__ void beam_commit(BeamState<LM>& st, int nb, int nw, const Cand& mywin, int V, int32_t* par,
                                            int32_t* tk, const BeamLM& lm) {
    const int tid = threadIdx.x;
    const long long VP = (long long)V + 1;
    double rsc = 0.0, rlms = 0.0;
    int rlast = -1, rnode = 0, rpn = -1, rpt = -1;
    bool fresh = false;  // a new trie node
    if (tid < nw) {
        const long long idx = mywin.idx;
        const int i = (int)(idx / VP);
        int key_beam = -1;
        for (int j = 0; j < nb; ++j)
            if (st.midx[j] == idx) key_beam = j;
        if (key_beam >= 0) {
            const int j = key_beam;
            rsc = st.msc[j];
            if (LM) rlms = st.lms[j];
            rlast = st.mlast[j];
            rnode = st.node[j];
            rpn = st.pnode[j];
            rpt = st.ptok[j];
        } else {
            fresh = true;
            rsc = mywin.s;
            rlast = rpt = (int)(idx - (long long)i * VP) - 1;  // the position in beam i's run: 0 = blank, tok + 1 otherwise
            rpn = st.node[i];
            if (LM) rlms = st.lms[i] + lm.entry(st.ptok[i], rpt);
        }
    }
    // New nodes are numbered in winner order.  The ballot is one wave's: nw <= kMaxBeam = 32, so every
    // committing lane and thread 0 sit in wave 0, also in the 256-thread kernels.
    const unsigned long long fm = __ballot(fresh);
    const int base = st.nodes;
    if (fresh) rnode = base + __popcll(fm & ((1ull << tid) - 1));
    __syncthreads();  // every lane has read the old beams
    if (tid < nw) {
        st.sc[tid] = rsc;
        if (LM) st.lms[tid] = rlms;
        st.last[tid] = rlast;
        st.node[tid] = rnode;
        st.pnode[tid] = rpn;
        st.ptok[tid] = rpt;
        if (fresh) {
            par[rnode] = rpn;
            tk[rnode] = rpt;
        }
    }
    if (tid == 0) {
        st.nb = nw;
        st.nodes = base + __popcll(fm);
    }
    __syncthreads();
}

// Results: the beams are already in the reference's final sorted order.
template <bool LM>
__device__ void beam_write(const BeamState<LM>& st, const int32_t* par, const int32_t* tk, int b, int L, int W,
                           int32_t* __restrict__ out_tokens, int32_t* __restrict__ out_len,
                           double* __restrict__ out_score, int32_t* __restrict__ out_nbeams) {
    const int tid = threadIdx.x, nb = st.nb;
    if (tid < nb) {
        int len = 0;
        for (int n = st.node[tid]; n > 0; n = par[n]) ++len;
        int32_t* o = out_tokens + ((int64_t)b * W + tid) * L;
        int k = len;
        for (int n = st.node[tid]; n > 0; n = par[n]) o[--k] = tk[n];
        out_len[(int64_t)b * W + tid] = len;
        out_score[(int64_t)b * W + tid] = st.sc[tid];
    }
    if (tid == 0) out_nbeams[b] = nb;
}

}  // namespace
}  // namespace vasr
