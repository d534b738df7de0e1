// The dense CTC prefix beam search: beam_common.h's frame step over all nb * V
// candidates of a frame -- every live key, and every live beam extended by every token that is not
// the blank, not the beam's last token and not an existing node -- each scored on the fly in each of
// the W selection rounds.  256 threads per utterance.  Two frame sources:
//   logits  (vasr_ctc_beam_search[_lm])  the row's log_softmax is formed in fp32 into dynamic LDS, so
//           V <= 16384; optionally with a bigram LM;
//   rows    (vasr_ctc_beam_search_shortlist's complete mode)  ready log-probability rows are read
//           from global memory by token index: no dynamic LDS, V up to 2^20, no LM.
//
// vasr_ctc_beam_search_lm adds two things.  frames: workgroup b walks only its own first
// min(max(frames[b], 0), L) rows.  lm_table: shallow fusion with a bigram table: a non-blank candidate
// of key k scores (score + lp[tok]) + lm_weight * S(k), S(k) the table's score of the whole prefix k,
// added again in every frame; the blank extension gets no term.  S is carried per live beam (lms[])
// next to the prefix's tail token (ptok[]), and a new node's S is S(parent) + table[1 + tail][tok] --
// the left-to-right float64 sum the host scorer forms.  The kernel is a template on the LM flag, so
// the search without a table carries none of it.
#include "beam_common.h"

namespace vasr {
namespace {

template <bool LM, bool ROWS>
__global__ __launch_bounds__(kBeamThreads) void ctc_beam_kernel(const float* __restrict__ x, int64_t ld_row, int64_t ld_utt,
                                                               int L, int V, int W, int blank,
                                                               const int32_t* __restrict__ frames, BeamLM lm,
                                                               int32_t* __restrict__ trie, int64_t trie_stride,
                                                               int32_t* __restrict__ out_tokens,
                                                               int32_t* __restrict__ out_len, double* __restrict__ out_score,
                                                               int32_t* __restrict__ out_nbeams,
                                                               int32_t* __restrict__ out_uncertified) {
    extern __shared__ __attribute__((aligned(16))) float lds_row[];  // V log-probabilities (!ROWS)
    __shared__ BeamState<LM> st;
    __shared__ Cand red[kBeamThreads / 64];
    __shared__ float fred[kBeamThreads / 64];

    const int b = blockIdx.x, tid = threadIdx.x;
    int32_t* par = trie + (int64_t)b * trie_stride;  // parent node
    int32_t* tk = par + trie_stride / 2;             // appended token
    const long long VP = (long long)V + 1;
    beam_init(st, par, tk);
    const int nf = beam_frames(frames, b, L);

    for (int t = 0; t < nf; ++t) {
        const float* row = x + (int64_t)b * ld_utt + (int64_t)t * ld_row;
        float mx, lse;
        if (!ROWS) row_log_softmax<true>(row, V, lds_row, fred, mx, lse);  // beam_merge's first barrier publishes it
        const float* lp = ROWS ? row : lds_row;
        const int nb = st.nb;
        beam_merge(st, RowSource{lp, blank}, nb, V, blank, lm.weight);
        auto candidate = [&](int c) {
            const int i = c / V, tok = c - i * V;
            Cand k{0.0, -1};
            if (tok == blank) {
                k.s = st.msc[i];
                k.idx = st.midx[i];
                return k;
            }
            if (tok == st.last[i]) return k;
            bool existing = false;  // an existing node: merged into its key
            for (int j = 0; j < nb; ++j)
                if (st.src_of[j] == i && st.ptok[j] == tok) existing = true;
            if (existing) return k;
            k.s = st.sc[i] + (double)lp[tok];
            if (LM) k.s = add_lm(k.s, lm.weight, st.lms[i] + lm.entry(st.ptok[i], tok));  // coalesced along tok
            k.idx = (long long)i * VP + tok + 1;
            return k;
        };
        Cand mywin, lastwin;
        const int nw = beam_select<kBeamThreads>(nb * V, W, candidate, red, mywin, lastwin);
        beam_commit(st, nb, nw, mywin, V, par, tk, lm);
    }
    beam_write(st, par, tk, b, L, W, out_tokens, out_len, out_score, out_nbeams);
    if (ROWS && tid == 0) out_uncertified[b] = 0;
}

}  // namespace

void beam_launch(const float* x, int64_t ld_row, int64_t ld_utt, int B, int L, int V, int W, int blank, const int32_t* frames,
                 const float* lm_table, int64_t ld_lm, double lm_weight, int32_t* trie, int32_t* out_tokens, int32_t* out_len,
                 double* out_score, int32_t* out_nbeams, int32_t* out_uncertified, void* stream) {
    const bool rows = out_uncertified != nullptr;
    const auto kernel = rows       ? ctc_beam_kernel<false, true>
                        : lm_table ? ctc_beam_kernel<true, false>
                                   : ctc_beam_kernel<false, false>;
    hipLaunchKernelGGL(kernel, dim3(B), dim3(kBeamThreads), rows ? 0 : V * sizeof(float), as_stream(stream), x, ld_row,
                       ld_utt, L, V, W, blank, frames, BeamLM{lm_table, ld_lm, lm_weight}, trie,
                       vasr_ctc_beam_workspace_elems(L, W), out_tokens, out_len, out_score, out_nbeams, out_uncertified);
}

namespace {

int beam_search(const char* who, const float* logits, int64_t ld_row, int64_t ld_utt, int B, int L, int V, int W,
                int blank, const int32_t* frames, const float* lm_table, int64_t ld_lm, double lm_weight, int32_t* trie,
                int32_t* out_tokens, int32_t* out_len, double* out_score, int32_t* out_nbeams, void* stream) {
    if (int rc = beam_check_args(who, (logits || L == 0) && trie && out_tokens && out_len && out_score && out_nbeams, B, L, V,
                                 kMaxStagedVocab, W, blank))
        return rc;
    VASR_CHECK_ARG(!lm_table || ld_lm >= V, "%s: lm_table row stride ld_lm=%lld below V=%d", who, (long long)ld_lm, V);
    VASR_CHECK_ARG(lm_weight == lm_weight, "%s: lm_weight is NaN", who);
    if (B == 0) return VASR_OK;
    const bool lm = lm_table && lm_weight > 0;  // the reference's own test (decode.py:188)
    beam_launch(logits, ld_row, ld_utt, B, L, V, W, blank, frames, lm ? lm_table : nullptr, ld_lm, lm_weight, trie, out_tokens,
                out_len, out_score, out_nbeams, nullptr, stream);
    return launch_status(who);
}

}  // namespace
}  // namespace vasr

VASR_API int64_t vasr_ctc_beam_workspace_elems(int L, int W) { return 2 * ((int64_t)L * W + 1); }

VASR_API int vasr_ctc_beam_search(const float* logits, int64_t ld_row, int64_t ld_utt, int B, int L, int V, int W,
                                  int blank, int32_t* trie, int32_t* out_tokens, int32_t* out_len, double* out_score,
                                  int32_t* out_nbeams, void* stream) {
    return vasr::beam_search("vasr_ctc_beam_search", logits, ld_row, ld_utt, B, L, V, W, blank, nullptr, nullptr, 0, 0.0,
                             trie, out_tokens, out_len, out_score, out_nbeams, stream);
}

VASR_API int vasr_ctc_beam_search_lm(const float* logits, int64_t ld_row, int64_t ld_utt, int B, int L, int V, int W,
                                     int blank, const int32_t* frames, const float* lm_table, int64_t ld_lm,
                                     double lm_weight, int32_t* trie, int32_t* out_tokens, int32_t* out_len,
                                     double* out_score, int32_t* out_nbeams, void* stream) {
    return vasr::beam_search("vasr_ctc_beam_search_lm", logits, ld_row, ld_utt, B, L, V, W, blank, frames, lm_table,
                             ld_lm, lm_weight, trie, out_tokens, out_len, out_score, out_nbeams, stream);
}
