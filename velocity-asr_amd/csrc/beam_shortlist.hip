// Exact CTC prefix beam search from a per-frame shortlist.
//
// vasr_ctc_beam_shortlist_f32: one workgroup per (utterance, frame) row forms the row's log-softmax
// with beam_common.h's row_log_softmax, the dense search's own, and keeps the K best non-blank tokens,
// ordered by (log-probability descending, token ascending), with the blank's log-probability.  The
// selection is K block-wide maxima of an order-preserving 64-bit key (float bits, ~token); each
// thread keeps the best key of its own strided slice and only the winner's owner rescans its slice.
// K = 0 (complete mode) writes the whole log-probability rows instead.  Up to V = 16384 the row is
// staged in LDS, as in beam.hip; above that every pass re-reads it from global memory (L2).
//
// vasr_ctc_beam_search_shortlist: beam_common.h's frame step over nb * (K + 1) candidates -- every live
// key, and every live beam extended by the frame's K tokens -- instead of nb * V.  One wave per
// utterance.  What is this file's: the frame source (the shortlist of the frame in LDS, loaded a frame
// ahead; a token outside it is not found), the candidate cache (the candidates of a frame, at most
// 32 * 65, are scored once into LDS, the slot of an extension that reaches an existing node struck
// out by the live beam that owns the node, and the W winners are W wave-wide maxima over them), and the
// certificate.  After the W winners are known the frame is certified when the W-th winner's score is
// strictly above fl(s_i + theta) for every live beam i, theta the shortlist's smallest
// log-probability: no omitted candidate can then enter, raise a survivor or win its last label.
// Uncertified frames are counted per utterance; the search goes on either way and the caller decides.
// tok == NULL (complete mode) is not searched here: it is beam.hip's dense kernel reading the (B, L, V)
// log-probability rows by token index, the exact search for vocabularies whose row does not fit LDS.
#include "beam_common.h"

namespace vasr {
namespace {

__device__ __forceinline__ unsigned long long shortlist_key(float lp, int tok) {
    uint32_t u = __float_as_uint(lp + 0.0f);  // -0.0 orders as +0.0
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (uint32_t)~(uint32_t)tok;
}

__device__ unsigned long long block_max_key(unsigned long long k, unsigned long long* red) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long d = __shfl_xor(k, o, 64);
        k = d > k ? d : k;
    }
    if ((tid & 63) == 0) red[tid >> 6] = k;
    __syncthreads();
    unsigned long long best = red[0];
    for (int w = 1; w < kBeamThreads / 64; ++w) best = red[w] > best ? red[w] : best;
    __syncthreads();
    return best;
}

template <bool STAGED>
__global__ __launch_bounds__(kBeamThreads) void beam_shortlist_kernel(const float* __restrict__ logits, int64_t ld_row,
                                                                     int64_t ld_utt, int L, int V, int K, int blank,
                                                                     const int32_t* __restrict__ frames,
                                                                     int32_t* __restrict__ out_tok,
                                                                     float* __restrict__ out_lp,
                                                                     float* __restrict__ out_blank_lp) {
    extern __shared__ __attribute__((aligned(16))) float lp[];  // V log-probabilities (STAGED)
    __shared__ float fred[kBeamThreads / 64];
    __shared__ unsigned long long kred[kBeamThreads / 64];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / L, t = blockIdx.x - b * L;
    const int64_t r = blockIdx.x;
    if (t >= beam_frames(frames, b, L)) {  // a row past the utterance: never read; the shortlist gets a defined fill
        if (K > 0) {
            for (int k = tid; k < K; k += kBeamThreads) {
                out_tok[r * K + k] = -1;
                out_lp[r * K + k] = -INFINITY;
            }
            if (tid == 0) out_blank_lp[r] = -INFINITY;
        }
        return;
    }
    const float* row = logits + (int64_t)b * ld_utt + (int64_t)t * ld_row;
    float mx, lse;
    row_log_softmax<STAGED>(row, V, lp, fred, mx, lse);
    if (STAGED) __syncthreads();
    auto value = [&](int v) { return STAGED ? lp[v] : (row[v] - mx) - lse; };
    if (K == 0) {  // complete mode: the whole row
        float* o = out_lp + r * V;
        for (int v = tid; v < V; v += kBeamThreads) o[v] = value(v);
        return;
    }
    // K maxima; `mine` is the best key of this thread's slice below the previous winner
    auto scan = [&](bool bounded, unsigned long long below) {
        unsigned long long best = 0;  // no key is 0: ~tok is not
        for (int v = tid; v < V; v += kBeamThreads) {
            if (v == blank) continue;
            const unsigned long long k = shortlist_key(value(v), v);
            if (bounded && k >= below) continue;
            best = k > best ? k : best;
        }
        return best;
    };
    unsigned long long mine = scan(false, 0);
    for (int k = 0; k < K; ++k) {
        const unsigned long long w = block_max_key(mine, kred);
        const int tok = (int)~(uint32_t)w;
        if (w == 0) {  // cannot happen for K <= V - 1; keeps the outputs defined
            if (tid == 0) {
                out_tok[r * K + k] = -1;
                out_lp[r * K + k] = -INFINITY;
            }
            continue;
        }
        if (mine == w) {  // the owner: write the winner, then find the slice's next
            out_tok[r * K + k] = tok;
            out_lp[r * K + k] = value(tok);
            mine = scan(true, w);
        }
    }
    if (tid == 0) out_blank_lp[r] = value(blank);
}

__global__ __launch_bounds__(64) void beam_shortlist_search_kernel(
    const int32_t* __restrict__ tokT, const float* __restrict__ lpT, const float* __restrict__ blankT, int L, int K, int V,
    int W, int blank, const int32_t* __restrict__ frames, int32_t* __restrict__ trie, int64_t trie_stride,
    int32_t* __restrict__ out_tokens, int32_t* __restrict__ out_len, double* __restrict__ out_score,
    int32_t* __restrict__ out_nbeams, int32_t* __restrict__ out_uncertified) {
    constexpr int kSlots = kMaxBeam * (kMaxShortlist + 1);
    __shared__ double cs[kSlots];  // the frame's candidates, scored once
    __shared__ long long ci[kSlots];
    __shared__ int stok[kMaxShortlist];
    __shared__ float slp[kMaxShortlist];
    __shared__ float sblank;
    __shared__ BeamState<false> st;

    const int b = blockIdx.x, tid = threadIdx.x;
    int32_t* par = trie + (int64_t)b * trie_stride;  // parent node
    int32_t* tk = par + trie_stride / 2;             // appended token
    const long long VP = (long long)V + 1;
    const int K1 = K + 1;  // candidates per live beam
    beam_init(st, par, tk);
    const int nf = beam_frames(frames, b, L);
    int uncertified = 0;

    // the next frame's shortlist is loaded a frame ahead
    const int64_t r0 = (int64_t)b * L;
    int ntok = -1;
    float nlp = 0.f, nbl = 0.f;
    if (nf > 0) {
        if (tid < K) {
            ntok = tokT[r0 * K + tid];
            nlp = lpT[r0 * K + tid];
        }
        if (tid == 0) nbl = blankT[r0];
    }

    for (int t = 0; t < nf; ++t) {
        if (tid < K) {
            stok[tid] = ntok;
            slp[tid] = nlp;
        }
        if (tid == 0) sblank = nbl;
        if (t + 1 < nf) {
            if (tid < K) {
                ntok = tokT[(r0 + t + 1) * K + tid];
                nlp = lpT[(r0 + t + 1) * K + tid];
            }
            if (tid == 0) nbl = blankT[r0 + t + 1];
        }
        const int nb = st.nb;
        beam_merge(st, ShortlistSource{stok, slp, &sblank, K}, nb, V, blank, 0.0);
        // the candidates: slot i * K1 is live key i, slot i * K1 + k + 1 beam i extended by the k-th token
        const int ncand = nb * K1;
        for (int c = tid; c < ncand; c += 64) {
            const int i = c / K1, k = c - i * K1;
            Cand cd{0.0, -1};
            if (k == 0) {
                cd.s = st.msc[i];
                cd.idx = st.midx[i];
            } else if (stok[k - 1] != st.last[i]) {
                cd.s = st.sc[i] + (double)slp[k - 1];
                cd.idx = (long long)i * VP + stok[k - 1] + 1;
            }
            cs[c] = cd.s;
            ci[c] = cd.idx;
        }
        __syncthreads();
        if (tid < nb && st.slot_of[tid] >= 0) ci[st.src_of[tid] * K1 + st.slot_of[tid] + 1] = -1;  // merged into key tid
        __syncthreads();
        Cand mywin, sigma;  // sigma: the W-th winner where nw == W
        const int nw = beam_select<64>(ncand, W, [&](int c) { return Cand{cs[c], ci[c]}; }, nullptr, mywin, sigma);
        // the certificate, from the old scores
        if (K < V - 1) {
            bool bad = nw != W;
            if (!bad) bad = __ballot(tid < nb && !(sigma.s > st.sc[tid] + (double)slp[K - 1])) != 0;  // a NaN fails
            if (bad) ++uncertified;
        }
        beam_commit(st, nb, nw, mywin, V, par, tk, BeamLM{});
    }
    beam_write(st, par, tk, b, L, W, out_tokens, out_len, out_score, out_nbeams);
    if (tid == 0) out_uncertified[b] = uncertified;
}

}  // namespace
}  // namespace vasr

VASR_API int vasr_ctc_beam_shortlist_f32(const float* logits, int64_t ld_row, int64_t ld_utt, int B, int L, int V, int K,
                                         int blank, const int32_t* frames, int32_t* out_tok, float* out_lp,
                                         float* out_blank_lp, void* stream) {
    using namespace vasr;
    const char* who = "vasr_ctc_beam_shortlist_f32";
    VASR_CHECK_ARG(B >= 0 && L >= 0 && V >= 1 && V <= (1 << 20) && K >= 0 && K <= kMaxShortlist && blank >= 0 && blank < V &&
                       (int64_t)B * L <= 0x7fffffff,
                   "%s: bad shape B=%d L=%d V=%d K=%d blank=%d", who, B, L, V, K, blank);
    VASR_CHECK_ARG(K == 0 || V >= 2, "%s: a shortlist needs a non-blank token, V=%d", who, V);
    VASR_CHECK_ARG(ld_row >= V && ld_utt >= 0, "%s: bad strides ld_row=%lld ld_utt=%lld for V=%d", who, (long long)ld_row,
                   (long long)ld_utt, V);
    VASR_CHECK_ARG((logits || (int64_t)B * L == 0) && out_lp && (K == 0 || (out_tok && out_blank_lp)), "%s: null pointer",
                   who);
    if ((int64_t)B * L == 0) return VASR_OK;
    if (K > V - 1) K = V - 1;
    const bool staged = V <= kMaxStagedVocab;
    hipLaunchKernelGGL(staged ? beam_shortlist_kernel<true> : beam_shortlist_kernel<false>, dim3(B * L), dim3(kBeamThreads),
                       staged ? V * sizeof(float) : 0, as_stream(stream), logits, ld_row, ld_utt, L, V, K, blank, frames,
                       out_tok, out_lp, out_blank_lp);
    return launch_status(who);
}

VASR_API int vasr_ctc_beam_search_shortlist(const int32_t* tok, const float* lp, const float* blank_lp, int B, int L, int K,
                                            int V, int W, int blank, const int32_t* frames, int32_t* trie,
                                            int32_t* out_tokens, int32_t* out_len, double* out_score, int32_t* out_nbeams,
                                            int32_t* out_uncertified, void* stream) {
    using namespace vasr;
    const char* who = "vasr_ctc_beam_search_shortlist";
    if (int rc = beam_check_args(who, trie && out_tokens && out_len && out_score && out_nbeams && out_uncertified, B, L, V,
                                 1 << 20, W, blank))
        return rc;
    const bool complete = tok == nullptr;
    VASR_CHECK_ARG(lp || (int64_t)B * L == 0, "%s: null pointer", who);
    VASR_CHECK_ARG(complete || (blank_lp || (int64_t)B * L == 0), "%s: a shortlist without its blank column", who);
    VASR_CHECK_ARG(complete || (K >= 1 && K <= kMaxShortlist && K <= V - 1), "%s: K=%d outside 1..min(%d, V - 1) for V=%d",
                   who, K, kMaxShortlist, V);
    if (B == 0) return VASR_OK;
    if (complete)  // the dense kernel over the rows
        beam_launch(lp, V, (int64_t)L * V, B, L, V, W, blank, frames, nullptr, 0, 0.0, trie, out_tokens, out_len, out_score,
                    out_nbeams, out_uncertified, stream);
    else
        hipLaunchKernelGGL(beam_shortlist_search_kernel, dim3(B), dim3(64), 0, as_stream(stream), tok, lp, blank_lp, L, K, V, W,
                           blank, frames, trie, vasr_ctc_beam_workspace_elems(L, W), out_tokens, out_len, out_score, out_nbeams,
                           out_uncertified);
    return launch_status(who);
}
