// The standard CTC prefix beam search: every prefix carries the summed probability
// of all its alignments (pb: ending in the blank, pnb: ending in its tail token), equal prefixes merge
// by logaddexp, a bigram language model scores each token once, when it is appended, and every token
// earns a length bonus.  A sibling of beam.hip on beam_common.h: the same trie workspace, row
// log-softmax, W-fold selection, node numbering and (B, W, L) output layout; what differs is the
// merged record (prefix_merge), the fresh candidate's score (prefix_fresh) and that a prefix keeps one
// trie node for the whole search (prefix_commit).  Hypothesis scores are real log-probabilities:
// out_logp = log p(prefix | frames) under the search's pruning.
//
// One workgroup of 256 threads per utterance.  Two frame sources:
//   logits     the row's log_softmax is formed in fp32 into dynamic LDS (V <= 16384) and all nb * V
//              candidates are scored on the fly in each selection round, as in beam.hip;
//   shortlist  vasr_ctc_beam_shortlist_f32's arrays: a frame's K tokens, their log-probabilities and
//              the blank's, loaded a frame ahead; nb * (K + 1) candidates.  A token outside the
//              shortlist counts as -inf: token pruning, an approximation without a certificate.
// Only the merged records (at most 3 contributions for each of nb keys) need exp / log1p in float64;
// a candidate costs an add and a select, with an LM a table gather and two more adds.
#include "beam_common.h"

namespace vasr {
namespace {

template <bool LM, bool SHORT>
__global__ __launch_bounds__(kBeamThreads) void ctc_prefix_beam_kernel(
    const float* __restrict__ x, int64_t ld_row, int64_t ld_utt, const int32_t* __restrict__ tokT,
    const float* __restrict__ lpT, const float* __restrict__ blankT, int K, int L, int V, int W, int blank,
    const int32_t* __restrict__ frames, BeamLM lm, double beta, int32_t* __restrict__ trie, int64_t trie_stride,
    int32_t* __restrict__ out_tokens, int32_t* __restrict__ out_len, double* __restrict__ out_score,
    double* __restrict__ out_logp, int32_t* __restrict__ out_nbeams) {
    extern __shared__ __attribute__((aligned(16))) float lds_row[];  // V log-probabilities (!SHORT)
    __shared__ PrefixState<LM> st;
    __shared__ Cand red[kBeamThreads / 64];
    __shared__ float fred[kBeamThreads / 64];
    __shared__ int stok[SHORT ? kMaxShortlist : 1];
    __shared__ float slp[SHORT ? kMaxShortlist : 1];
    __shared__ float sblank;

    const int b = blockIdx.x, tid = threadIdx.x;
    int32_t* par = trie + (int64_t)b * trie_stride;  // parent node
    int32_t* tk = par + trie_stride / 2;             // appended token
    const long long VP = (long long)V + 1;
    prefix_init(st, par, tk);
    const int nf = beam_frames(frames, b, L);

    // shortlist: the next frame's entries are loaded a frame ahead
    const int64_t r0 = (int64_t)b * L;
    int ntok = -1;
    float nlp = -INFINITY, nbl = -INFINITY;
    if (SHORT && nf > 0) {
        if (tid < K) {
            ntok = tokT[r0 * K + tid];
            nlp = lpT[r0 * K + tid];
        }
        if (tid == 0) nbl = blankT[r0];
    }

    for (int t = 0; t < nf; ++t) {
        if (SHORT) {
            if (tid < K) {
                // a token that is the blank or outside 0 .. V - 1 is no candidate and indexes nothing
                const bool ok = ntok >= 0 && ntok < V && ntok != blank;
                stok[tid] = ok ? ntok : -1;
                slp[tid] = ok ? nlp : -INFINITY;
            }
            if (tid == 0) sblank = nbl;
            if (t + 1 < nf) {
                if (tid < K) {
                    ntok = tokT[(r0 + t + 1) * K + tid];
                    nlp = lpT[(r0 + t + 1) * K + tid];
                }
                if (tid == 0) nbl = blankT[r0 + t + 1];
            }
        } else {
            float mx, lse;
            row_log_softmax<true>(x + (int64_t)b * ld_utt + (int64_t)t * ld_row, V, lds_row, fred, mx, lse);
        }
        // prefix_merge's first barrier publishes either source
        const int nb = st.nb;
        Cand mywin, lastwin;
        int nw;
        if (SHORT) {
            const ShortlistSource f{stok, slp, &sblank, K};
            prefix_merge(st, f, nb, V, lm.weight, beta);
            const int K1 = K + 1;  // candidates per live beam: its key, then its K extensions
            auto candidate = [&](int c) {
                const int i = c / K1, k = c - i * K1;
                if (k == 0) return Cand{st.mrank[i], st.midx[i]};
                const int tok = stok[k - 1];
                if (tok < 0) return Cand{0.0, -1};
                return prefix_fresh(st, nb, i, tok, slp[k - 1], VP, lm);
            };
            nw = beam_select<kBeamThreads>(nb * K1, W, candidate, red, mywin, lastwin);
            prefix_commit(st, f, nb, nw, mywin, V, par, tk, lm);
        } else {
            const RowSource f{lds_row, blank};
            prefix_merge(st, f, nb, V, lm.weight, beta);
            auto candidate = [&](int c) {
                const int i = c / V, tok = c - i * V;
                if (tok == blank) return Cand{st.mrank[i], st.midx[i]};
                return prefix_fresh(st, nb, i, tok, lds_row[tok], VP, lm);  // the table gather is coalesced along tok
            };
            nw = beam_select<kBeamThreads>(nb * V, W, candidate, red, mywin, lastwin);
            prefix_commit(st, f, nb, nw, mywin, V, par, tk, lm);
        }
    }
    prefix_write(st, par, tk, b, L, W, out_tokens, out_len, out_score, out_logp, out_nbeams);
}

// The checks both entries share, before any launch.
int prefix_check(const char* who, bool ptrs, int B, int L, int V, int max_v, int W, int blank, const float* lm_table,
                 int64_t ld_lm, double alpha, double beta) {
    if (int rc = beam_check_args(who, ptrs, B, L, V, max_v, W, blank)) return rc;
    VASR_CHECK_ARG(!lm_table || ld_lm >= V, "%s: lm_table row stride ld_lm=%lld below V=%d", who, (long long)ld_lm, V);
    VASR_CHECK_ARG(alpha == alpha && beta == beta, "%s: alpha or beta is NaN", who);
    return VASR_OK;
}

}  // namespace
}  // namespace vasr

VASR_API int vasr_ctc_prefix_beam_search(const float* logits, int64_t ld_row, int64_t ld_utt, int B, int L, int V, int W,
                                         int blank, const int32_t* frames, const float* lm_table, int64_t ld_lm,
                                         double alpha, double beta, int32_t* trie, int32_t* out_tokens, int32_t* out_len,
                                         double* out_score, double* out_logp, int32_t* out_nbeams, void* stream) {
    using namespace vasr;
    const char* who = "vasr_ctc_prefix_beam_search";
    const bool ptrs = (logits || L == 0) && trie && out_tokens && out_len && out_score && out_logp && out_nbeams;
    if (int rc = prefix_check(who, ptrs, B, L, V, kMaxStagedVocab, W, blank, lm_table, ld_lm, alpha, beta)) return rc;
    if (B == 0) return VASR_OK;
    const bool lm = lm_table && alpha > 0;
    const auto kernel = lm ? ctc_prefix_beam_kernel<true, false> : ctc_prefix_beam_kernel<false, false>;
    hipLaunchKernelGGL(kernel, dim3(B), dim3(kBeamThreads), V * sizeof(float), as_stream(stream), logits, ld_row, ld_utt,
                       nullptr, nullptr, nullptr, 0, L, V, W, blank, frames, BeamLM{lm ? lm_table : nullptr, ld_lm, alpha},
                       beta, trie, vasr_ctc_beam_workspace_elems(L, W), out_tokens, out_len, out_score, out_logp, out_nbeams);
    return launch_status(who);
}

VASR_API int vasr_ctc_prefix_beam_search_shortlist(const int32_t* tok, const float* lp, const float* blank_lp, int K, int V,
                                                   int B, int L, int W, int blank, const int32_t* frames,
                                                   const float* lm_table, int64_t ld_lm, double alpha, double beta,
                                                   int32_t* trie, int32_t* out_tokens, int32_t* out_len, double* out_score,
                                                   double* out_logp, int32_t* out_nbeams, void* stream) {
    using namespace vasr;
    const char* who = "vasr_ctc_prefix_beam_search_shortlist";
    const bool ptrs = ((tok && lp && blank_lp) || (int64_t)B * L == 0) && trie && out_tokens && out_len && out_score &&
                      out_logp && out_nbeams;
    if (int rc = prefix_check(who, ptrs, B, L, V, 1 << 20, W, blank, lm_table, ld_lm, alpha, beta)) return rc;
    VASR_CHECK_ARG(K >= 1 && K <= kMaxShortlist && K <= V - 1, "%s: K=%d outside 1..min(%d, V - 1) for V=%d", who, K,
                   kMaxShortlist, V);
    if (B == 0) return VASR_OK;
    const bool lm = lm_table && alpha > 0;
    const auto kernel = lm ? ctc_prefix_beam_kernel<true, true> : ctc_prefix_beam_kernel<false, true>;
    hipLaunchKernelGGL(kernel, dim3(B), dim3(kBeamThreads), 0, as_stream(stream), nullptr, 0, 0, tok, lp, blank_lp, K, L, V,
                       W, blank, frames, BeamLM{lm ? lm_table : nullptr, ld_lm, alpha}, beta, trie,
                       vasr_ctc_beam_workspace_elems(L, W), out_tokens, out_len, out_score, out_logp, out_nbeams);
    return launch_status(who);
}
