// The frame step of the CTC prefix beam search (reference velocity_asr/decode.py:128-217), once, for
// the three searches built on it: beam.hip's dense kernel over logits (log-softmax formed into LDS,
// optional bigram LM), the same kernel over ready log-probability rows, and beam_shortlist.hip's
// one-wave search over K shortlisted tokens per frame.  A search supplies a frame source -- the
// blank's log-probability and lookup(tok, v) -- and its candidates; everything exact lives here: the
// beam state, the merged records with their tie rules (beam_merge), the W maxima (beam_select), the
// new beam set and trie nodes (beam_commit), the write-out, and the row log-softmax that the dense
// kernel and the shortlist kernel share.  The second half of the file is the frame step of the standard
// prefix beam search (beam_prefix.hip: summed alignments, per-token LM term, length bonus) on the same
// trie, frame sources, selection and output layout.
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

constexpr int kMaxShortlist = 64;

// A frame's shortlist in LDS (vasr_ctc_beam_shortlist_f32's arrays): a token is found by its place
// in it, or not at all.
struct ShortlistSource {
    const int* tok;
    const float* lp;
    const float* blank;
    int K;
    __device__ float blank_lp() const { return *blank; }
    __device__ int lookup(int t, float& v) const {
        int at = -1;
        for (int k = 0; k < K; ++k)
            if (tok[k] == t) {
                v = lp[k];
                at = k;
            }
        return at;
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

// ---------------------------------------------------------------------------------------------
// The standard CTC prefix beam search (beam_prefix.hip), on the same trie, frame
// sources, selection and output layout.  A live beam carries the summed log-probability of all
// alignments of its prefix, split into those ending in the blank (pb) and in the prefix's tail token
// (pnb); equal prefixes merge by logaddexp, the language model scores a token once, when it is
// appended (alpha * table entry), and every token earns a length bonus beta.  A key's rank is
// ((pb (+) pnb) + alpha * S(key)) + beta * len(key).
//
// A candidate's Cand::idx here is prefix_order(position, extension), not the bare position: at position
// i (V + 1) + tail_i + 1 beam i both repeats its tail (into its own key) and extends by it (into
// prefix + (tail)), the repeat first, so two keys can share a position -- they do whenever the blank is
// -inf and the own key's first contribution is the repeat.  The order value keeps the insertion order
// and names exactly one key: (i, slot, own) is beam i's key, (i, tok + 1, extension) is prefix_i + (tok).

__device__ __forceinline__ long long prefix_order(long long position, bool extension) {
    return 2 * position + (extension ? 1 : 0);
}

// log(exp(a) + exp(b)) in float64, x (+) -inf = x exactly.  Symmetric in its arguments.
__device__ __forceinline__ double log_add(double a, double b) {
    if (!(a > -INFINITY)) return b;
    if (!(b > -INFINITY)) return a;
    const double m = a >= b ? a : b, n = a >= b ? b : a;
    return m + log1p(exp(n - m));
}

// (tot + alpha * S) + bonus, bonus = beta * len already rounded: products rounded before the sums,
// as the float64 host arithmetic forms them (see add_lm).
template <bool LM>
__device__ __forceinline__ double prefix_rank(double tot, double alpha, double S, double bonus) {
#pragma clang fp contract(off)
    double s = tot;
    if (LM) {
        const double term = alpha * S;
        s = s + term;
    }
    return s + bonus;
}

__device__ __forceinline__ double length_bonus(double beta, int len) {
#pragma clang fp contract(off)
    return beta * (double)len;
}

// The live beams of one utterance (LDS), in sorted order, and the merged records of their keys.
template <bool LM>
struct PrefixState {
    double pb[kMaxBeam], pnb[kMaxBeam], tot[kMaxBeam], rank[kMaxBeam];
    double lms[LM ? kMaxBeam : 1];  // S(prefix)
    double bext[kMaxBeam];          // beta * (len + 1): the bonus of every extension of the beam
    double mpb[kMaxBeam], mpnb[kMaxBeam], mtot[kMaxBeam], mrank[kMaxBeam];
    long long midx[kMaxBeam];  // the key's prefix_order, -1: no finite contribution, no key
    int len[kMaxBeam], node[kMaxBeam], pnode[kMaxBeam], ptok[kMaxBeam];  // ptok: the prefix's tail token
    int src_of[kMaxBeam];  // the beam whose node is beam j's parent, or -1
    int fpar[kMaxBeam], ftok[kMaxBeam], found[kMaxBeam];  // prefix_commit: a winner's (parent, token), its old node
    int nb, nodes;
};

template <bool LM>
__device__ void prefix_init(PrefixState<LM>& st, int32_t* par, int32_t* tk) {
    if (threadIdx.x == 0) {
        st.pb[0] = 0.0;
        st.pnb[0] = -INFINITY;
        st.tot[0] = 0.0;
        st.rank[0] = 0.0;
        st.lms[0] = 0.0;
        st.len[0] = 0;
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

// The merged record of every live key j.  Three contributions can reach it: its own blank extension
// (to pb, at position j (V + 1)), its own repeat of the tail token (pnb_j + lp[tail], to pnb, at
// j (V + 1) + tail + 1) and the extension by that token of the one beam i whose node is j's parent
// ((tail_i == tail_j ? pb_i : tot_i) + lp[tail_j], to pnb, at i (V + 1) + tail_j + 1).  A contribution
// of -inf -- a token the source does not hold included -- is not made: it gives no position, and a key
// without a contribution does not exist in this frame.  The key's order is the smallest prefix_order of
// its contributions, the parent's being an extension.  The first barrier publishes the frame source.
template <bool LM, class Source>
__device__ __forceinline__ void prefix_merge(PrefixState<LM>& st, const Source& f, int nb, int V, double alpha,
                                             double beta) {
    const int j = threadIdx.x;
    const long long VP = (long long)V + 1;
    int src = -1;
    if (j < nb) {
        for (int i = 0; i < nb; ++i)
            if (st.node[i] == st.pnode[j]) src = i;
        st.src_of[j] = src;
        st.bext[j] = length_bonus(beta, st.len[j] + 1);
    }
    __syncthreads();
    if (j < nb) {
        long long first = -1;
        auto place = [&](long long idx) {
            if (first < 0 || idx < first) first = idx;
        };
        double mpb = st.tot[j] + (double)f.blank_lp(), mpnb = -INFINITY;
        if (mpb > -INFINITY)
            place(prefix_order((long long)j * VP, false));
        else
            mpb = -INFINITY;
        const int tail = st.ptok[j];
        float v = 0.f;
        if (tail >= 0 && f.lookup(tail, v) >= 0) {
            const double own = st.pnb[j] + (double)v;
            if (own > -INFINITY) {
                mpnb = own;
                place(prefix_order((long long)j * VP + tail + 1, false));
            }
            if (src >= 0) {
                const double ext = (st.ptok[src] == tail ? st.pb[src] : st.tot[src]) + (double)v;
                if (ext > -INFINITY) {
                    mpnb = log_add(mpnb, ext);
                    place(prefix_order((long long)src * VP + tail + 1, true));
                }
            }
        }
        const double mtot = log_add(mpb, mpnb);
        st.mpb[j] = mpb;
        st.mpnb[j] = mpnb;
        st.mtot[j] = mtot;
        st.mrank[j] = prefix_rank<LM>(mtot, alpha, LM ? st.lms[j] : 0.0, length_bonus(beta, st.len[j]));
        st.midx[j] = first;
    }
    __syncthreads();
}

// Beam i extended by a token of log-probability v that is not the blank: none when the extension
// reaches a live node (it is in that key's merged record) or is -inf, else the fresh key's rank, scored
// on the fly: after a repeat of the tail only the alignments ending in the blank go on.
template <bool LM>
__device__ __forceinline__ Cand prefix_fresh(const PrefixState<LM>& st, int nb, int i, int tok, float v, long long VP,
                                             const BeamLM& lm) {
    Cand k{0.0, -1};
    bool existing = false;
    for (int j = 0; j < nb; ++j)
        if (st.src_of[j] == i && st.ptok[j] == tok) existing = true;
    if (existing) return k;
    const double a = (tok == st.ptok[i] ? st.pb[i] : st.tot[i]) + (double)v;
    if (!(a > -INFINITY)) return k;
    k.s = prefix_rank<LM>(a, lm.weight, LM ? st.lms[i] + lm.entry(st.ptok[i], tok) : 0.0, st.bext[i]);
    k.idx = prefix_order((long long)i * VP + tok + 1, true);
    return k;
}

// The new beam set in winner order (beam_commit's numbering of new nodes).  A surviving key takes its
// merged record; an extension that reached no live node has pb = -inf, pnb = its one contribution,
// S(child) = S(parent) + table[1 + tail(parent)][tok] and one more token.  Its node is the trie's own
// (parent node, token) node where the prefix was live before, else a new one: with summed alignments a
// prefix can leave the beam while an extension of it stays and come back later, and the extension
// must still find it as its parent, so a prefix keeps one node for the whole search.  The old node is
// looked for by all threads among the nodes above the smallest parent (a child is younger than its
// parent): at most L W / 256 coalesced loads per thread and frame, each compared with the nw pairs in LDS,
// beside nb V / 256 candidates scored W times (timed with short prefixes live late: profiles/beam_prefix.md).
template <bool LM, class Source>
__device__ __forceinline__ void prefix_commit(PrefixState<LM>& st, const Source& f, int nb, int nw, const Cand& mywin, int V,
                                              int32_t* par, int32_t* tk, const BeamLM& lm) {
    const int tid = threadIdx.x;
    const long long VP = (long long)V + 1;
    double rpb = -INFINITY, rpnb = -INFINITY, rtot = -INFINITY, rlms = 0.0;
    int rlen = 0, rnode = 0, rpn = -1, rpt = -1;
    bool fresh = false;
    if (tid < nw) {
        const long long idx = mywin.idx, pos = idx >> 1;  // prefix_order: one key per value
        const int i = (int)(pos / VP);
        int key_beam = -1;
        for (int j = 0; j < nb; ++j)
            if (st.midx[j] == idx) key_beam = j;
        if (key_beam >= 0) {
            const int j = key_beam;
            rpb = st.mpb[j];
            rpnb = st.mpnb[j];
            rtot = st.mtot[j];
            if (LM) rlms = st.lms[j];
            rlen = st.len[j];
            rnode = st.node[j];
            rpn = st.pnode[j];
            rpt = st.ptok[j];
        } else {
            fresh = true;
            rpt = (int)(pos - (long long)i * VP) - 1;
            float v = 0.f;
            f.lookup(rpt, v);  // a winner's token is in the source
            rpnb = rtot = (rpt == st.ptok[i] ? st.pb[i] : st.tot[i]) + (double)v;
            rpn = st.node[i];
            rlen = st.len[i] + 1;
            if (LM) rlms = st.lms[i] + lm.entry(st.ptok[i], rpt);
        }
    }
    const int base = st.nodes;
    if (tid < nw) {
        st.fpar[tid] = fresh ? rpn : -1;
        st.ftok[tid] = rpt;
        st.found[tid] = -1;
    }
    __syncthreads();
    int lo = base;
    for (int r = 0; r < nw; ++r)
        if (st.fpar[r] >= 0) lo = min(lo, st.fpar[r] + 1);
    for (int n = lo + tid; n < base; n += kBeamThreads) {
        const int p = par[n], t = tk[n];
        for (int r = 0; r < nw; ++r)
            if (st.fpar[r] == p && st.ftok[r] == t) st.found[r] = n;  // at most one node per (parent, token)
    }
    __syncthreads();  // also: every lane has read the old beams
    if (fresh && st.found[tid] >= 0) {
        rnode = st.found[tid];
        fresh = false;
    }
    // as beam_commit: nw <= 32, so every committing lane and thread 0 sit in wave 0
    const unsigned long long fm = __ballot(fresh);
    if (fresh) rnode = base + __popcll(fm & ((1ull << tid) - 1));
    if (tid < nw) {
        st.pb[tid] = rpb;
        st.pnb[tid] = rpnb;
        st.tot[tid] = rtot;
        st.rank[tid] = mywin.s;
        if (LM) st.lms[tid] = rlms;
        st.len[tid] = rlen;
        st.node[tid] = rnode;
        st.pnode[tid] = rpn;
        st.ptok[tid] = rpt;
        if (fresh) {
            // at most W nodes are created per frame, so rnode <= L W: inside the 1 + L W nodes of
            // vasr_ctc_beam_workspace_elems, as in the reference-semantics searches
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

template <bool LM>
__device__ void prefix_write(const PrefixState<LM>& st, const int32_t* par, const int32_t* tk, int b, int L, int W,
                             int32_t* __restrict__ out_tokens, int32_t* __restrict__ out_len,
                             double* __restrict__ out_score, double* __restrict__ out_logp,
                             int32_t* __restrict__ out_nbeams) {
    const int tid = threadIdx.x, nb = st.nb;
    if (tid < nb) {
        const int len = st.len[tid];
        int32_t* o = out_tokens + ((int64_t)b * W + tid) * L;
        int k = len;
        for (int n = st.node[tid]; n > 0 && k > 0; n = par[n]) o[--k] = tk[n];
        out_len[(int64_t)b * W + tid] = len;
        out_score[(int64_t)b * W + tid] = st.rank[tid];
        out_logp[(int64_t)b * W + tid] = st.tot[tid];
    }
    if (tid == 0) out_nbeams[b] = nb;
}

}  // namespace
}  // namespace vasr
