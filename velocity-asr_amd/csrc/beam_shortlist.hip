// Exact CTC prefix beam search from a per-frame shortlist.
//
// vasr_ctc_beam_shortlist_f32: one workgroup per (utterance, frame) row forms the row's log-softmax
// exactly as ctc_beam_kernel (beam.hip) does -- the same 256 strided partial sums through the same
// block_reduce_f, so the same bits -- and keeps the K best non-blank tokens, ordered by
// (log-probability descending, token ascending), with the blank's log-probability.  The selection
// is K block-wide maxima of an order-preserving 64-bit key (float bits, ~token); each thread keeps
// the best key of its own strided slice and only the winner's owner rescans its slice.  K = 0
// (complete mode) writes the whole log-probability rows instead.  Up to V = 16384 the row is staged
// in LDS, as in beam.hip; above that every pass re-reads it from global memory (L2).
//
// vasr_ctc_beam_search_shortlist: ctc_beam_kernel<false>'s frame step over nb * (K + 1) candidates
// -- every live key, and every live beam extended by the frame's K tokens -- instead of nb * V.
// One wave per utterance: the candidates of a frame (at most 32 * 65) are scored once into LDS and
// the W winners are W wave-wide maxima over them.  Step 2 is beam.hip's and step 4 forms the same beam set
// with lane r building beam r (new trie nodes numbered in winner order by a ballot); a live beam's
// repeat or parent extension whose token is not in the frame's shortlist offers no score, but the
// parent extension still offers its insertion position, which the full search would have used
// (the key's position is structural: min(j (V + 1), src (V + 1) + ptok_j + 1)).  After the W winners
// are known the frame is certified when the W-th winner's score is strictly above
// fl(s_i + theta) for every live beam i, theta the shortlist's smallest log-probability: no omitted
// candidate can then enter, raise a survivor or win its last label.  Uncertified frames are
// counted per utterance; the search goes on either way and the caller decides.  The `complete`
// instance (tok == NULL) reads (B, L, V) log-probability rows by token index, evaluates no
// certificate and walks nb * V candidates with 256 threads, as beam.hip does: the exact search for
// vocabularies whose row does not fit beam.hip's LDS.
#include "beam_common.h"

namespace vasr {
namespace {

constexpr int kMaxShortlist = 64;

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
    const int nf = frames ? min(max(frames[b], 0), L) : L;
    if (t >= nf) {  // a row past the utterance: never read; the shortlist gets a defined fill
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
    // log_softmax of the row: beam.hip's step 1, operation for operation
    float mx = -INFINITY;
    for (int v = tid; v < V; v += kBeamThreads) {
        const float x = row[v];
        if (STAGED) lp[v] = x;
        mx = fmaxf(mx, x);
    }
    mx = block_reduce_f(mx, fred, true);
    float se = 0.f;
    for (int v = tid; v < V; v += kBeamThreads) se += expf((STAGED ? lp[v] : row[v]) - mx);
    se = block_reduce_f(se, fred, false);
    const float lse = logf(se);
    auto value = [&](int v) { return STAGED ? lp[v] : (row[v] - mx) - lse; };
    if (STAGED) {
        for (int v = tid; v < V; v += kBeamThreads) lp[v] = (lp[v] - mx) - lse;
        __syncthreads();
    }
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

template <bool COMPLETE, int THREADS>
__global__ __launch_bounds__(THREADS) void beam_shortlist_search_kernel(
    const int32_t* __restrict__ tokT, const float* __restrict__ lpT, const float* __restrict__ blankT, int L, int K, int V,
    int W, int blank, const int32_t* __restrict__ frames, int32_t* __restrict__ trie, int64_t trie_stride,
    int32_t* __restrict__ out_tokens, int32_t* __restrict__ out_len, double* __restrict__ out_score,
    int32_t* __restrict__ out_nbeams, int32_t* __restrict__ out_uncertified) {
    static_assert(COMPLETE ? THREADS == kBeamThreads : THREADS == 64, "one wave walks a shortlist");
    constexpr int kSlots = COMPLETE ? 1 : kMaxBeam * (kMaxShortlist + 1);
    __shared__ double cs[kSlots];  // the frame's candidates, scored once
    __shared__ long long ci[kSlots];
    __shared__ int stok[COMPLETE ? 1 : kMaxShortlist];
    __shared__ float slp[COMPLETE ? 1 : kMaxShortlist];
    __shared__ float sblank;
    __shared__ double sc[kMaxBeam], msc[kMaxBeam];
    __shared__ long long midx[kMaxBeam];
    __shared__ int last[kMaxBeam], node[kMaxBeam], pnode[kMaxBeam], ptok[kMaxBeam], mlast[kMaxBeam];
    __shared__ int src_of[kMaxBeam];  // beam i whose extension reaches beam j's node, or -1
    __shared__ Cand red[kBeamThreads / 64];
    __shared__ int slot_of[COMPLETE ? 1 : kMaxBeam];  // the shortlist slot merged into live key j, or -1
    __shared__ int nb_s, nodes_s;

    const int b = blockIdx.x, tid = threadIdx.x;
    int32_t* par = trie + (int64_t)b * trie_stride;  // parent node
    int32_t* tk = par + trie_stride / 2;             // appended token
    const long long VP = (long long)V + 1;
    const int K1 = COMPLETE ? V : K + 1;  // candidates per live beam
    if (tid == 0) {
        sc[0] = 0.0;
        last[0] = -1;  // None
        node[0] = 0;
        pnode[0] = -1;
        ptok[0] = -1;
        par[0] = -1;
        tk[0] = -1;
        nb_s = 1;
        nodes_s = 1;
    }
    __syncthreads();
    const int nf = frames ? min(max(frames[b], 0), L) : L;
    int uncertified = 0;  // thread 0's count

    // the next frame's shortlist is loaded a frame ahead
    const int64_t r0 = (int64_t)b * L;
    int ntok = -1;
    float nlp = 0.f, nbl = 0.f;
    if (!COMPLETE && nf > 0) {
        if (tid < K) {
            ntok = tokT[r0 * K + tid];
            nlp = lpT[r0 * K + tid];
        }
        if (tid == 0) nbl = blankT[r0];
    }

    for (int t = 0; t < nf; ++t) {
        const float* row = COMPLETE ? lpT + (r0 + t) * V : nullptr;
        if (!COMPLETE) {
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
        }
        const int nb = nb_s;
        // 2. merged record of every live key
        if (tid < nb) {
            const int j = tid;
            int src = -1;
            for (int i = 0; i < nb; ++i)
                if (node[i] == pnode[j] && ptok[j] != last[i]) src = i;
            src_of[j] = src;
        }
        __syncthreads();
        if (tid < nb) {
            const int j = tid;
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
            // the frame's log-probability of a token: by index, or by its place in the shortlist
            auto lookup = [&](int tok, float& v) {  // its place in the shortlist (any value >= 0 by index), or -1
                if (COMPLETE) {
                    v = row[tok];
                    return 0;
                }
                int at = -1;
                for (int k = 0; k < K; ++k)
                    if (stok[k] == tok) {
                        v = slp[k];
                        at = k;
                    }
                return at;
            };
            const int src = src_of[j];
            float v = 0.f;
            int merged = -1;  // the candidate slot of (src, ptok): an existing node, merged into key j
            offer(sc[j] + (double)(COMPLETE ? row[blank] : sblank), (long long)j * VP, blank);
            if (last[j] >= 0 && last[j] != blank && lookup(last[j], v) >= 0)
                offer(sc[j] + (double)v, (long long)j * VP + last[j] + 1, last[j]);
            if (src >= 0) {
                const long long idx = (long long)src * VP + ptok[j] + 1;
                const int at = lookup(ptok[j], v);
                if (at >= 0) {
                    offer(sc[src] + (double)v, idx, ptok[j]);
                    merged = src * K1 + at + 1;
                } else {
                    place(idx);  // the full search inserts the key here, whatever the score
                }
            }
            if (!COMPLETE) slot_of[j] = merged;
            msc[j] = best.s;
            midx[j] = first;
            mlast[j] = bl;
        }
        __syncthreads();
        // 3. W best candidates, each the maximum strictly below the previous winner
        const int ncand = nb * K1;
        auto candidate = [&](int c) {
            const int i = c / K1, k = c - i * K1;
            Cand cd{0.0, -1};
            if (COMPLETE ? k == blank : k == 0) {
                cd.s = msc[i];
                cd.idx = midx[i];
                return cd;
            }
            const int tok = COMPLETE ? k : stok[k - 1];
            if (tok == last[i]) return cd;
            if (COMPLETE)  // (the shortlist's slots of existing nodes are struck out below, by slot_of)
                for (int j = 0; j < nb; ++j)
                    if (src_of[j] == i && ptok[j] == tok) return cd;  // an existing node: merged into key j
            cd.s = sc[i] + (double)(COMPLETE ? row[tok] : slp[k - 1]);
            cd.idx = (long long)i * VP + tok + 1;
            return cd;
        };
        if (!COMPLETE) {
            for (int c = tid; c < ncand; c += THREADS) {
                const Cand cd = candidate(c);
                cs[c] = cd.s;
                ci[c] = cd.idx;
            }
            __syncthreads();
            if (tid < nb && slot_of[tid] >= 0) ci[slot_of[tid]] = -1;
            __syncthreads();
        }
        Cand prev{INFINITY, -2}, mywin{0.0, -1};  // lane r keeps winner r
        int nw = 0;
        for (int r = 0; r < W; ++r) {
            Cand mine{0.0, -1};
            for (int c = tid; c < ncand; c += THREADS) {
                Cand k;
                if (COMPLETE) {
                    k = candidate(c);
                } else {  // this thread's own slots: no barrier needed
                    k.s = cs[c];
                    k.idx = ci[c];
                }
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
        // 4. the new beam set in winner order, lane r forming beam r, and the certificate
        double rsc = 0.0;
        int rlast = -1, rnode = 0, rpn = -1, rpt = -1;
        bool fresh = false;  // a new trie node
        if (tid < nw) {
            const long long idx = mywin.idx;
            const int i = (int)(idx / VP);
            const int pos = (int)(idx - (long long)i * VP);  // 0 = blank, tok + 1 otherwise
            int key_beam = -1;
            for (int j = 0; j < nb; ++j)
                if (midx[j] == idx) key_beam = j;
            if (key_beam >= 0) {
                const int j = key_beam;
                rsc = msc[j];
                rlast = mlast[j];
                rnode = node[j];
                rpn = pnode[j];
                rpt = ptok[j];
            } else {
                fresh = true;
                rsc = mywin.s;
                rlast = rpt = pos - 1;
                rpn = node[i];
            }
        }
        // new nodes are numbered in winner order (lanes r < nw <= 32 are all in the first wave)
        const unsigned long long fm = __ballot(fresh);
        const int base = nodes_s;
        if (fresh) rnode = base + __popcll(fm & ((1ull << tid) - 1));
        bool bad = false;
        if (!COMPLETE && K < V - 1) {
            bad = nw != W;
            if (!bad) {  // prev is the W-th winner
                const double sigma = prev.s, theta = (double)slp[K - 1];
                bad = __ballot(tid < nb && !(sigma > sc[tid] + theta)) != 0;  // a NaN fails
            }
        }
        __syncthreads();  // every lane has read the old beams
        if (tid < nw) {
            sc[tid] = rsc;
            last[tid] = rlast;
            node[tid] = rnode;
            pnode[tid] = rpn;
            ptok[tid] = rpt;
            if (fresh) {
                par[rnode] = rpn;
                tk[rnode] = rpt;
            }
        }
        if (tid == 0) {
            nb_s = nw;
            nodes_s = base + __popcll(fm);
            if (bad) ++uncertified;
        }
        __syncthreads();
    }
    // results: beams are already in the reference's final sorted order
    const int nb = nb_s;
    if (tid < nb) {
        int len = 0;
        for (int n = node[tid]; n > 0; n = par[n]) ++len;
        int32_t* o = out_tokens + ((int64_t)b * W + tid) * L;
        int k = len;
        for (int n = node[tid]; n > 0; n = par[n]) o[--k] = tk[n];
        out_len[(int64_t)b * W + tid] = len;
        out_score[(int64_t)b * W + tid] = sc[tid];
    }
    if (tid == 0) {
        out_nbeams[b] = nb;
        out_uncertified[b] = uncertified;
    }
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
    const bool staged = V <= 16384;  // beam.hip's limit: the row in 64 KiB of LDS
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
    VASR_CHECK_ARG(trie && out_tokens && out_len && out_score && out_nbeams && out_uncertified, "%s: null pointer", who);
    VASR_CHECK_ARG(B >= 0 && L >= 0 && V >= 1 && V <= (1 << 20) && W >= 1 && W <= kMaxBeam && blank >= 0 && blank < V,
                   "%s: bad shape B=%d L=%d V=%d W=%d blank=%d", who, B, L, V, W, blank);
    const bool complete = tok == nullptr;
    VASR_CHECK_ARG(lp || (int64_t)B * L == 0, "%s: null pointer", who);
    VASR_CHECK_ARG(complete || (blank_lp || (int64_t)B * L == 0), "%s: a shortlist without its blank column", who);
    VASR_CHECK_ARG(complete || (K >= 1 && K <= kMaxShortlist && K <= V - 1), "%s: K=%d outside 1..min(%d, V - 1) for V=%d",
                   who, K, kMaxShortlist, V);
    if (B == 0) return VASR_OK;
    const int64_t stride = vasr_ctc_beam_workspace_elems(L, W);
    if (complete)
        hipLaunchKernelGGL((beam_shortlist_search_kernel<true, kBeamThreads>), dim3(B), dim3(kBeamThreads), 0,
                           as_stream(stream), tok, lp, blank_lp, L, K, V, W, blank, frames, trie, stride, out_tokens, out_len,
                           out_score, out_nbeams, out_uncertified);
    else
        hipLaunchKernelGGL((beam_shortlist_search_kernel<false, 64>), dim3(B), dim3(64), 0, as_stream(stream), tok, lp,
                           blank_lp, L, K, V, W, blank, frames, trie, stride, out_tokens, out_len, out_score, out_nbeams,
                           out_uncertified);
    return launch_status(who);
}
