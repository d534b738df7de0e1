"""CTC decoding (drop-in for reference velocity_asr/decode.py).

Greedy decoding runs on the device: an argmax kernel over the vocabulary and a
per-utterance collapse kernel (blank removal, repeat collapse, optional run
timestamps), so only the kept token ids cross PCIe instead of (B, L, V) logits.
ctc_forced_align scores and aligns a known transcript on the device (not in the reference).
Token -> text conversion is host string handling, as in the reference.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib, ops

BLANK_TOKEN = 0

# The package's own __all__ stays the reference's list (tests/test_host.py); extensions are
# imported from here.
__all__ = ["BLANK_TOKEN", "DecodingResult", "ctc_greedy_decode", "ctc_greedy_decode_with_timestamps",
           "ctc_beam_search", "ctc_forced_align", "BigramLM", "CTCDecoder", "create_default_vocabulary",
           "greedy_token_ids", "ScoredDecoding", "ctc_greedy_decode_with_confidence", "token_confidences",
           "AGGREGATIONS", "ctc_prefix_beam_search"]


@dataclass
class DecodingResult:
    """Result of CTC decoding (reference decode.py:18-24)."""

    text: str
    tokens: List[int]
    score: float
    timestamps: Optional[List[Tuple[int, int]]] = None
    logp: Optional[float] = None  # ctc_prefix_beam_search: log p(tokens | frames), all alignments summed


def _on_device(logits: torch.Tensor) -> torch.Tensor:
    if logits.device.type != "cuda":
        _lib.require_device()
        logits = logits.to(torch.device("cuda", torch.cuda.current_device()))
    if logits.dtype != torch.float32:
        logits = logits.float()
    return logits


def greedy_token_ids(logits: torch.Tensor, blank_token: int = BLANK_TOKEN, collapse_repeated: bool = True,
                     timestamps: bool = False):
    """Device argmax + collapse; returns (tokens (B,L) int32, lengths (B,), start, end) on the device."""
    logits = _on_device(logits)
    pred = ops.argmax(logits).view(logits.shape[0], -1)
    return ops.ctc_collapse(pred, blank_token, collapse_repeated, timestamps)


def ctc_greedy_decode(logits: torch.Tensor, blank_token: int = BLANK_TOKEN,
                      collapse_repeated: bool = True) -> List[List[int]]:
    """Greedy CTC decoding (reference decode.py:27-71)."""
    toks, lens, _, _ = greedy_token_ids(logits, blank_token, collapse_repeated)
    toks, lens = toks.cpu().numpy(), lens.cpu().numpy()
    return [toks[b, : lens[b]].tolist() for b in range(toks.shape[0])]


def ctc_greedy_decode_with_timestamps(logits: torch.Tensor,
                                      blank_token: int = BLANK_TOKEN) -> List[Tuple[List[int], List[Tuple[int, int]]]]:
    """Greedy decoding with (start_frame, end_frame) per token (reference decode.py:74-125)."""
    toks, lens, st, en = greedy_token_ids(logits, blank_token, True, timestamps=True)
    toks, lens, st, en = toks.cpu().numpy(), lens.cpu().numpy(), st.cpu().numpy(), en.cpu().numpy()
    out = []
    for b in range(toks.shape[0]):
        n = int(lens[b])
        out.append((toks[b, :n].tolist(), [(int(s), int(e)) for s, e in zip(st[b, :n], en[b, :n])]))
    return out


@dataclass
class ScoredDecoding:
    """Greedy decoding of one utterance with confidences (not in the reference): the kept tokens,
    their (start_frame, end_frame) spans, one confidence in (0, 1] per token, and `score`, the
    log-probability of the greedy path (the sum over the utterance's frames, blank ones included,
    of the log-softmax value at the argmax)."""

    tokens: List[int]
    timestamps: List[Tuple[int, int]]
    confidences: List[float]
    score: float


AGGREGATIONS = ("mean", "min", "prod")


def token_confidences(logp_sum, logp_min, run_lengths, aggregation: str = "mean") -> List[float]:
    """Per-token confidences from the device's per-token values (host arithmetic, float64): the sum
    and the minimum of the frame log-probabilities over a token's run and the run's length.
    "mean": exp(sum / length), the geometric mean of the frame probabilities; "min": exp(min), the
    weakest frame; "prod": exp(sum), the probability of the whole run."""
    if aggregation not in AGGREGATIONS:
        raise ValueError(f"aggregation must be one of {AGGREGATIONS}, got {aggregation!r}")
    s = np.asarray(logp_sum, dtype=np.float64)
    if aggregation == "mean":
        v = s / np.maximum(np.asarray(run_lengths, dtype=np.float64), 1.0)
    elif aggregation == "min":
        v = np.asarray(logp_min, dtype=np.float64)
    else:
        v = s
    return np.exp(v).tolist()


def _scored_from_device(res, aggregation: str) -> List[ScoredDecoding]:
    """ops.ctc_collapse_conf's device tuple -> one ScoredDecoding per utterance."""
    if aggregation not in AGGREGATIONS:
        raise ValueError(f"aggregation must be one of {AGGREGATIONS}, got {aggregation!r}")
    toks, lens, st, en, lsum, lmin, path = (t.cpu().numpy() for t in res)
    out = []
    for b in range(toks.shape[0]):
        n = int(lens[b])
        spans = [(int(s), int(e)) for s, e in zip(st[b, :n], en[b, :n])]
        conf = token_confidences(lsum[b, :n], lmin[b, :n], [e - s for s, e in spans], aggregation)
        out.append(ScoredDecoding(toks[b, :n].tolist(), spans, conf, float(path[b])))
    return out


def ctc_greedy_decode_with_confidence(logits: torch.Tensor, blank_token: int = BLANK_TOKEN, input_lengths=None,
                                      aggregation: str = "mean") -> List[ScoredDecoding]:
    """ctc_greedy_decode_with_timestamps plus a confidence per token and the greedy path's
    log-probability per utterance, all reduced on the device (vasr_argmax_logp_f32,
    vasr_ctc_collapse_conf).  input_lengths (B,): row counts of a padded batch.  A model decodes
    without logits through VELOCITYASR.greedy_scored instead."""
    logits = _on_device(logits)
    if logits.dim() != 3:
        raise ValueError("ctc_greedy_decode_with_confidence: logits must be (B, L, V)")
    if aggregation not in AGGREGATIONS:
        raise ValueError(f"aggregation must be one of {AGGREGATIONS}, got {aggregation!r}")
    if input_lengths is not None:
        if not isinstance(input_lengths, torch.Tensor):
            input_lengths = torch.tensor([int(n) for n in input_lengths], dtype=torch.int32)
        input_lengths = input_lengths.to(device=logits.device, dtype=torch.int32).contiguous()
    pred, lp = ops.argmax_logp(logits)
    return _scored_from_device(ops.ctc_collapse_conf(pred, lp, blank_token, frames=input_lengths), aggregation)


class BigramLM:
    """Bigram language model for shallow fusion in ctc_beam_search (not in the reference, whose
    lm_scorer is any object with score(tokens)).

    table: float32 (V + 1, V); row 0 is log p(tok | sentence start), row 1 + p is
    log p(tok | previous token p).  score() is the left-to-right float64 sum of the prefix's
    entries, so an instance is a valid lm_scorer for the host search and the reference's own; given
    to ctc_beam_search it is searched on the device from device_table().
    """

    def __init__(self, table):
        table = np.ascontiguousarray(np.asarray(table, dtype=np.float32))
        if table.ndim != 2 or table.shape[0] != table.shape[1] + 1 or table.shape[1] < 1:
            raise ValueError(f"BigramLM: table must be (V + 1, V), got {table.shape}")
        self.table = table
        self._device: Dict[Any, torch.Tensor] = {}

    @property
    def vocab_size(self) -> int:
        return self.table.shape[1]

    def score(self, tokens: list) -> float:
        s = 0.0
        row = 0
        for tok in tokens:
            s += float(self.table[row, tok])
            row = 1 + tok
        return s

    def device_table(self, device) -> torch.Tensor:
        """The table on `device`, copied up once."""
        key = torch.device(device)
        if key.type == "cuda" and key.index is None:
            key = torch.device("cuda", torch.cuda.current_device())
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.table).to(key)
        return self._device[key]

    @classmethod
    def from_token_sequences(cls, seqs, vocab_size: int, blank: int = BLANK_TOKEN, alpha: float = 1.0) -> "BigramLM":
        """Add-alpha smoothed bigram counts of token sequences; every row is normalised over the
        non-blank tokens, and the blank column is -inf (the search never reads it)."""
        V = int(vocab_size)
        if not 0 <= blank < V or V < 2:
            raise ValueError(f"BigramLM: blank {blank} outside a vocabulary of {V} (at least 2 tokens)")
        if not alpha > 0:
            raise ValueError("BigramLM: alpha must be positive")
        counts = np.zeros((V + 1, V), dtype=np.float64)
        for seq in seqs:
            row = 0
            for tok in seq:
                tok = int(tok)
                if not 0 <= tok < V or tok == blank:
                    raise ValueError(f"BigramLM: token {tok} is the blank or outside 0..{V - 1}")
                counts[row, tok] += 1.0
                row = 1 + tok
        counts += alpha
        counts[:, blank] = 0.0
        with np.errstate(divide="ignore"):
            table = np.log(counts) - np.log(counts.sum(axis=1, keepdims=True))
        return cls(table.astype(np.float32))

    def save(self, path) -> None:
        """Write the table as a .npz archive; `path` is used as given, so name it *.npz."""
        with open(path, "wb") as f:
            np.savez(f, table=self.table)

    @classmethod
    def load(cls, path) -> "BigramLM":
        with np.load(path) as z:
            return cls(z["table"])


def beam_shortlist_size(shortlist, vocab_size: int, beam_width: int) -> int:
    """The K of a `shortlist=` argument: an int (1..64), or "auto" = max(16, 2 * beam_width); never
    above vocab_size - 1, where the shortlist is every non-blank token."""
    if isinstance(shortlist, str):
        if shortlist != "auto":
            raise ValueError(f'shortlist must be None, "auto" or an int, got {shortlist!r}')
        K = max(16, 2 * int(beam_width))
    else:
        K = int(shortlist)
    if not 1 <= K <= ops.BEAM_SHORTLIST_MAX:
        raise ValueError(f"shortlist must lie in 1..{ops.BEAM_SHORTLIST_MAX}, got {K}")
    return min(K, int(vocab_size) - 1)


def _beam_search_exact(logits: torch.Tensor, beam_width: int, blank: int, frames):
    """The full search (every token a candidate in every frame) of the utterances a shortlist did
    not certify: the dense kernel on the logits where a row fits its LDS, else complete
    log-probability rows and the same kernel reading those (the shortlist entry's complete mode)."""
    V = logits.shape[-1]
    if V <= ops.BEAM_DENSE_MAX_VOCAB:
        return ops.ctc_beam_search(logits, beam_width, blank, frames=frames)
    rows = ops.ctc_beam_shortlist(logits, 0, blank, frames)
    return ops.ctc_beam_search_shortlist(None, rows, None, V, beam_width, blank, frames)[:4]


def _beam_search_from_shortlist(short, vocab_size: int, beam_width: int, blank: int, frames, exact_of):
    """One search launch over a batch's shortlist arrays `short` = ops.ctc_beam_shortlist's three,
    then the exact search of the utterances with an uncertified frame: exact_of(indices, their
    frames) gives _beam_search_exact's tensors for them.  Returns ops.ctc_beam_search's four
    tensors: bitwise the full search's, by the certificate where it holds and by the second search
    where it does not."""
    toks, lens, scores, nb, unc = ops.ctc_beam_search_shortlist(*short, vocab_size, beam_width, blank, frames)
    bad = torch.nonzero(unc.cpu()).flatten().tolist()
    if bad:
        idx = torch.tensor(bad, device=toks.device)
        exact = exact_of(bad, None if frames is None else frames[idx])
        for dst, src in zip((toks, lens, scores, nb), exact):
            dst[idx] = src
    return toks, lens, scores, nb


def _beam_results(toks, lens, scores, nb) -> List[List[DecodingResult]]:
    toks, lens, scores, nb = toks.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy(), nb.cpu().numpy()
    return [[DecodingResult(text="", tokens=toks[b, r, :lens[b, r]].tolist(), score=float(scores[b, r]))
             for r in range(int(nb[b]))] for b in range(toks.shape[0])]


def _check_shortlist(who: str, shortlist, beam_width: int, lm_on: bool) -> None:
    if lm_on:
        raise ValueError(f"{who}: shortlist cannot be combined with a language model: with lm_weight > 0 a "
                         "candidate outside the acoustic shortlist can win on its language-model term, so the "
                         "per-frame certificate does not hold (DESIGN.md §3.6f); pass shortlist=None")
    if not 1 <= beam_width <= 32:
        raise ValueError(f"{who}: shortlist needs a beam width of 1..32, got {beam_width}")


def ctc_beam_search(logits: torch.Tensor, beam_width: int = 10, blank_token: int = BLANK_TOKEN,
                    lm_weight: float = 0.0, lm_scorer: Optional[Any] = None,
                    input_lengths=None, shortlist=None) -> List[List[DecodingResult]]:
    """Prefix beam search (reference decode.py:128-217) on the HIP device.

    For widths 1..32 the whole search runs in one launch, one workgroup per utterance, prefixes
    as trie nodes, the reference's insertion-order tie rules: vasr_ctc_beam_search, or
    vasr_ctc_beam_search_lm when input_lengths or a BigramLM with lm_weight > 0 is given.
    input_lengths (B,) are the row counts of a padded batch (a device tensor is taken without a
    host synchronisation); utterance b is searched over its first input_lengths[b] rows, as the
    reference on logits[b:b+1, :input_lengths[b]].  A BigramLM is fused on the device with the
    reference's semantics: lm_weight * lm_scorer.score(prefix) is added to every non-blank
    candidate in every frame, not to the blank extension.

    Any other lm_scorer is a Python object the device cannot call, so with one (and lm_weight > 0),
    or with beam_width > 32, the search runs on the host with the same bookkeeping over
    device-computed log-probabilities -- one score() call per (beam, token, frame).

    shortlist (extension): None is the search above.  An int K (1..64) or "auto"
    (max(16, 2 * beam_width)) first reduces every frame to its K most probable non-blank tokens
    (vasr_ctc_beam_shortlist_f32, one launch for all frames) and searches those
    (vasr_ctc_beam_search_shortlist), which proves frame by frame that no other token could have
    reached the beam; an utterance with a frame it cannot prove is searched again in full, so the
    result is bitwise that of shortlist=None -- faster, and open to vocabularies above 16384, which
    shortlist=None refuses.  Not with an active language model (ValueError), nor above width 32.
    """
    logits = _on_device(logits)
    lm_on = lm_scorer is not None and lm_weight > 0
    if shortlist is not None and logits.dim() == 3 and logits.shape[-1] >= 2:
        _check_shortlist("ctc_beam_search", shortlist, beam_width, lm_on)
        x = logits.float()
        B, L, V = x.shape
        frames = ops._beam_frames("ctc_beam_search", input_lengths, B, L, x.device)
        short = ops.ctc_beam_shortlist(x, beam_shortlist_size(shortlist, V, beam_width), blank_token, frames)
        return _beam_results(*_beam_search_from_shortlist(
            short, V, beam_width, blank_token, frames, lambda bad, fr: _beam_search_exact(x[bad], beam_width, blank_token, fr)))
    if (not lm_on or isinstance(lm_scorer, BigramLM)) and 1 <= beam_width <= 32:
        table = lm_scorer.device_table(logits.device) if lm_on else None
        return _beam_results(*ops.ctc_beam_search(logits.float(), beam_width, blank_token, frames=input_lengths,
                                                  lm_table=table, lm_weight=float(lm_weight) if lm_on else 0.0))
    return _ctc_beam_search_host(logits, beam_width, blank_token, lm_weight, lm_scorer, input_lengths)


def _ctc_beam_search_host(logits: torch.Tensor, beam_width: int, blank_token: int, lm_weight: float,
                          lm_scorer: Optional[Any], input_lengths=None) -> List[List[DecodingResult]]:
    """Host form of the same search (used with a Python lm_scorer)."""
    B, L, V = logits.shape
    if input_lengths is None:
        frames = [L] * B
    else:
        frames = [int(n) for n in (input_lengths.tolist() if isinstance(input_lengths, torch.Tensor) else input_lengths)]
        if len(frames) != B or any(not 0 <= n <= L for n in frames):
            raise ValueError(f"ctc_beam_search: input_lengths must be {B} counts in 0..{L}, got {frames}")
    all_results = []
    for b in range(B):
        # rows past an utterance's count are junk by contract: they are not even normalised
        log_probs = torch.log_softmax(logits[b, :frames[b]], dim=-1).cpu().numpy().astype(np.float64)
        beams: Dict[Tuple[int, ...], Tuple[float, Optional[int]]] = {(): (0.0, None)}
        for t in range(frames[b]):
            lp = log_probs[t]
            new_beams: Dict[Tuple[int, ...], Tuple[float, Optional[int]]] = {}
            for prefix, (score, last) in beams.items():
                blank_score = score + lp[blank_token]
                cur = new_beams.get(prefix)
                if cur is None or cur[0] < blank_score:
                    new_beams[prefix] = (blank_score, blank_token)
                scores = (score + lp).tolist()
                for token in range(V):
                    if token == blank_token:
                        continue
                    key = prefix if last == token else prefix + (token,)
                    s = scores[token]
                    if lm_scorer is not None and lm_weight > 0:
                        s += lm_weight * lm_scorer.score(list(key))
                    cur = new_beams.get(key)
                    if cur is None or cur[0] < s:
                        new_beams[key] = (s, token)
            beams = dict(sorted(new_beams.items(), key=lambda x: x[1][0], reverse=True)[:beam_width])
        results = [DecodingResult(text="", tokens=list(prefix), score=score)
                   for prefix, (score, _) in sorted(beams.items(), key=lambda x: x[1][0], reverse=True)]
        all_results.append(results)
    return all_results


def _logaddexp(a: float, b: float) -> float:
    if a == -math.inf:
        return b
    if b == -math.inf:
        return a
    m, n = (a, b) if a >= b else (b, a)
    return m + math.log1p(math.exp(n - m))


def ctc_prefix_beam_search(logits: torch.Tensor, beam_width: int = 10, blank_token: int = BLANK_TOKEN,
                           lm_scorer: Optional[Any] = None, lm_weight: float = 0.0, length_bonus: float = 0.0,
                           input_lengths=None, token_topk=None) -> List[List[DecodingResult]]:
    """The standard CTC prefix beam search (extension), where ctc_beam_search is the
    reference's: every prefix carries the summed probability of ALL its alignments (split into those
    ending in the blank and in its last token), the language model scores each token once, when it
    is appended (lm_weight * log p(tok | previous)), and every token earns length_bonus.  Results per
    utterance, best first: tokens, logp = log p(tokens | frames) and score = (logp + lm_weight *
    lm_scorer.score(tokens)) + length_bonus * len(tokens), the rank the beam was pruned by.

    Device logits with no scorer or a BigramLM, widths 1..32, run in one launch
    (vasr_ctc_prefix_beam_search; a row of V <= 16384 log-probabilities lives in LDS).  token_topk = K
    (1..64) or "auto" (max(16, 2 * beam_width)) prunes every frame to its K most probable non-blank
    tokens first (vasr_ctc_beam_shortlist_f32, then vasr_ctc_prefix_beam_search_shortlist): the usual
    token pruning, an approximation with no certificate and no fallback, and open to any vocabulary.
    Any other scorer, a wider beam, or CPU logits run the same algorithm on the host, with
    lm_scorer.score(prefix + [tok]) - lm_scorer.score(prefix) as the per-token term."""
    if logits.dim() != 3:
        raise ValueError("ctc_prefix_beam_search: logits must be (B, L, V)")
    W = int(beam_width)
    if W < 1:
        raise ValueError(f"ctc_prefix_beam_search: beam_width must be positive, got {beam_width}")
    lm_on = lm_scorer is not None and lm_weight > 0
    V = logits.shape[-1]
    K = None if token_topk is None or V < 2 else beam_shortlist_size(token_topk, V, W)
    if logits.device.type != "cuda" or (lm_on and not isinstance(lm_scorer, BigramLM)) or W > 32:
        return _ctc_prefix_beam_search_host(logits, W, blank_token, lm_scorer, lm_weight, length_bonus, input_lengths, K)
    x = logits.float()
    kw = dict(frames=input_lengths, lm_table=lm_scorer.device_table(x.device) if lm_on else None,
              alpha=float(lm_weight) if lm_on else 0.0, beta=float(length_bonus))
    if K is None:
        return _prefix_beam_results(*ops.ctc_prefix_beam_search(x, W, blank_token, **kw))
    kw["frames"] = ops._beam_frames("ctc_prefix_beam_search", input_lengths, x.shape[0], x.shape[1], x.device)
    short = ops.ctc_beam_shortlist(x, K, blank_token, kw["frames"])
    return _prefix_beam_results(*ops.ctc_prefix_beam_search_shortlist(*short, V, W, blank_token, **kw))


def _prefix_beam_results(toks, lens, scores, logp, nb) -> List[List[DecodingResult]]:
    toks, lens, scores, logp, nb = (t.cpu().numpy() for t in (toks, lens, scores, logp, nb))
    return [[DecodingResult(text="", tokens=toks[b, r, :lens[b, r]].tolist(), score=float(scores[b, r]),
                            logp=float(logp[b, r])) for r in range(int(nb[b]))] for b in range(toks.shape[0])]


def _ctc_prefix_beam_search_host(logits: torch.Tensor, beam_width: int, blank_token: int, lm_scorer: Optional[Any],
                                 lm_weight: float, length_bonus: float, input_lengths=None,
                                 token_topk: Optional[int] = None) -> List[List[DecodingResult]]:
    """Host form of ctc_prefix_beam_search, for a Python lm_scorer: float64 over float32
    log-probabilities.  A beam is (prefix, pb, pnb, S), S the sum of its tokens' language-model terms;
    contributions are joined by logaddexp in insertion order, one of -inf is not made, and the
    beam_width keys of largest rank survive, the earlier inserted first among equals (a stable sort
    over a dict).  token_topk: only each frame's K most probable non-blank tokens (log-probability
    descending, token ascending) are extended."""
    B, L, V = logits.shape
    if input_lengths is None:
        frames = [L] * B
    else:
        counts = input_lengths.tolist() if isinstance(input_lengths, torch.Tensor) else input_lengths
        frames = [int(n) for n in counts]
        if len(frames) != B or any(not 0 <= n <= L for n in frames):
            raise ValueError(f"ctc_prefix_beam_search: input_lengths must be {B} counts in 0..{L}, got {frames}")
    lm_on = lm_scorer is not None and lm_weight > 0
    alpha, beta, NEG = float(lm_weight), float(length_bonus), -math.inf
    all_results = []
    for b in range(B):
        log_probs = torch.log_softmax(logits[b, :frames[b]].float(), dim=-1).cpu().numpy()
        whole: Dict[Tuple[int, ...], float] = {(): lm_scorer.score([]) if lm_on else 0.0}  # scorer's value per prefix
        beams = [((), 0.0, NEG, 0.0)]
        for t in range(frames[b]):
            lp = log_probs[t].tolist()
            if token_topk is None:
                tokens = [tok for tok in range(V) if tok != blank_token]
            else:
                order = sorted((tok for tok in range(V) if tok != blank_token), key=lambda tok: (-lp[tok], tok))
                tokens = sorted(order[:token_topk])
            new: Dict[Tuple[int, ...], List[float]] = {}  # key -> [pb, pnb, S]

            def add(key, which, v, parent, S):
                if v == NEG:
                    return
                e = new.get(key)
                if e is None:
                    if lm_on and S is None:  # a new token: the scorer's term for it, once
                        if key not in whole:
                            whole[key] = lm_scorer.score(list(key))
                        S = parent[3] + (whole[key] - whole[parent[0]])
                    e = new[key] = [NEG, NEG, S if lm_on else 0.0]
                e[which] = _logaddexp(e[which], v)

            for beam in beams:
                prefix, pb, pnb, S = beam
                tot = _logaddexp(pb, pnb)
                add(prefix, 0, tot + lp[blank_token], beam, S)
                tail = prefix[-1] if prefix else None
                for tok in tokens:
                    if tok == tail:
                        add(prefix, 1, pnb + lp[tok], beam, S)
                        add(prefix + (tok,), 1, pb + lp[tok], beam, None)
                    else:
                        add(prefix + (tok,), 1, tot + lp[tok], beam, None)

            def rank(kv):
                key, (pb, pnb, S) = kv
                s = _logaddexp(pb, pnb)
                if lm_on:
                    s = s + alpha * S
                return s + beta * len(key)

            beams = [(key, e[0], e[1], e[2]) for key, e in sorted(new.items(), key=rank, reverse=True)[:beam_width]]
        results = []
        for prefix, pb, pnb, S in beams:
            logp = _logaddexp(pb, pnb)
            results.append(DecodingResult(text="", tokens=list(prefix), logp=logp,
                                          score=((logp + alpha * S) if lm_on else logp) + beta * len(prefix)))
        all_results.append(results)
    return all_results


def _align_targets(targets, target_lengths, blank_token: int):
    """A list of token lists as a blank-padded (B, Smax) int32 tensor, with its lengths unless given."""
    if not isinstance(targets, torch.Tensor):
        rows = [list(r) for r in targets]
        if target_lengths is None:
            target_lengths = [len(r) for r in rows]
        width = max((len(r) for r in rows), default=0)
        targets = torch.tensor([r + [blank_token] * (width - len(r)) for r in rows], dtype=torch.int32).reshape(
            len(rows), width)
    return targets, target_lengths


def _align_emissions(emis, tg, frames, tlen):
    """The Viterbi lattice over emissions (ops.ctc_emissions' or ops.ctc_head_emissions') as
    ctc_forced_align's result."""
    state, st, en, score = ops.ctc_align(emis, tg, frames, tlen)
    state, st, en, score = state.cpu().numpy(), st.cpu().numpy(), en.cpu().numpy(), score.cpu().numpy()
    tlen = tlen.cpu().numpy().clip(0, tg.shape[1])
    return [(float(score[b]), [(int(s), int(e)) for s, e in zip(st[b, :tlen[b]], en[b, :tlen[b]])],
             state[b].tolist()) for b in range(emis.shape[0])]


def ctc_forced_align(logits: torch.Tensor, targets, input_lengths=None, target_lengths=None,
                     blank_token: int = BLANK_TOKEN) -> List[Tuple[float, List[Tuple[int, int]], List[int]]]:
    """CTC forced alignment of a KNOWN transcript: the most probable path through the CTC lattice
    of `targets` (vasr_ctc_emissions_f32 + vasr_ctc_align_f32), where
    ctc_greedy_decode_with_timestamps only timestamps the model's own guess.

    logits (B, L, V); targets (B, Smax) token ids (a tensor, or a list of token lists, which also
    gives target_lengths); input_lengths / target_lengths (B,), default L / Smax.  Returns per
    utterance (score, [(start_frame, end_frame), ...] per target token, frame_labels): the path's
    log-probability; each token's first frame and one past its last, the convention of
    ctc_greedy_decode_with_timestamps; and for each of the L frames the target INDEX it emits,
    -1 for blank and past input_lengths.
    A transcript that does not fit its frames has score -inf and (-1, -1) spans.
    """
    logits = _on_device(logits)
    if logits.dim() != 3:
        raise ValueError("ctc_forced_align: logits must be (B, L, V)")
    targets, target_lengths = _align_targets(targets, target_lengths, blank_token)
    return _align_emissions(*ops.ctc_emissions(logits, targets, input_lengths, target_lengths, blank_token))


class CTCDecoder:
    """CTC decoder with vocabulary (reference decode.py:220-327)."""

    def __init__(self, vocabulary: List[str], blank_token: int = BLANK_TOKEN):
        self.vocabulary = vocabulary
        self.blank_token = blank_token
        self.vocab_size = len(vocabulary)
        self.token_to_idx = {token: idx for idx, token in enumerate(vocabulary)}

    def decode_greedy(self, logits: torch.Tensor, collapse_repeated: bool = True) -> List[str]:
        seqs = ctc_greedy_decode(logits, blank_token=self.blank_token, collapse_repeated=collapse_repeated)
        return [self._tokens_to_text(t) for t in seqs]

    def decode_greedy_scored(self, logits: torch.Tensor, input_lengths=None) -> List[DecodingResult]:
        """Greedy decoding as DecodingResults (extension): text, tokens, score = the greedy path's
        log-probability, and the tokens' (start_frame, end_frame) spans."""
        scored = ctc_greedy_decode_with_confidence(logits, blank_token=self.blank_token, input_lengths=input_lengths)
        return [DecodingResult(text=self._tokens_to_text(r.tokens), tokens=r.tokens, score=r.score,
                               timestamps=r.timestamps) for r in scored]

    def decode_beam_search(self, logits: torch.Tensor, beam_width: int = 10, return_all_beams: bool = False, *,
                           input_lengths=None, lm_scorer: Optional[Any] = None, lm_weight: float = 0.0, shortlist=None):
        beam_results = ctc_beam_search(logits, beam_width=beam_width, blank_token=self.blank_token,
                                       lm_weight=lm_weight, lm_scorer=lm_scorer, input_lengths=input_lengths,
                                       shortlist=shortlist)
        return self._beam_texts(beam_results, return_all_beams)

    def decode_prefix_beam_search(self, logits: torch.Tensor, beam_width: int = 10, return_all_beams: bool = False, *,
                                  input_lengths=None, lm_scorer: Optional[Any] = None, lm_weight: float = 0.0,
                                  length_bonus: float = 0.0, token_topk=None):
        """decode_beam_search with the standard prefix beam search (ctc_prefix_beam_search): texts, or
        with return_all_beams the DecodingResults (score = rank, logp = the prefix's log-probability)."""
        beam_results = ctc_prefix_beam_search(logits, beam_width=beam_width, blank_token=self.blank_token,
                                              lm_scorer=lm_scorer, lm_weight=lm_weight, length_bonus=length_bonus,
                                              input_lengths=input_lengths, token_topk=token_topk)
        return self._beam_texts(beam_results, return_all_beams)

    def _beam_texts(self, beam_results, return_all_beams: bool):
        """ctc_beam_search's results as decode_beam_search returns them."""
        if return_all_beams:
            for batch_results in beam_results:
                for result in batch_results:
                    result.text = self._tokens_to_text(result.tokens)
            return beam_results
        return [self._tokens_to_text(results[0].tokens) if results else "" for results in beam_results]

    def align(self, logits: torch.Tensor, texts: List[str], input_lengths=None):
        """Forced alignment of one transcript per utterance (text_to_tokens, then ctc_forced_align)."""
        return ctc_forced_align(logits, [self.text_to_tokens(t) for t in texts], input_lengths=input_lengths,
                                blank_token=self.blank_token)

    def _tokens_to_text(self, tokens: List[int]) -> str:
        chars = [self.vocabulary[t] if 0 <= t < self.vocab_size else "<unk>" for t in tokens]
        return "".join(chars).replace("▁", " ").strip()

    def text_to_tokens(self, text: str) -> List[int]:
        tokens = []
        for char in text:
            if char in self.token_to_idx:
                tokens.append(self.token_to_idx[char])
            elif "<unk>" in self.token_to_idx:
                tokens.append(self.token_to_idx["<unk>"])
        return tokens


def create_default_vocabulary(vocab_size: int = 50000) -> List[str]:
    """Character vocabulary + placeholders (reference decode.py:330-362)."""
    vocab = ["<blank>", "<unk>", "<pad>", " "]
    vocab.extend(list("abcdefghijklmnopqrstuvwxyz"))
    vocab.extend(list("ABCDEFGHIJKLMNOPQRSTUVWXYZ"))
    vocab.extend(list("0123456789"))
    vocab.extend(list(".,!?;:'\"()-"))
    for i in range(len(vocab), vocab_size):
        vocab.append(f"<token_{i}>")
    return vocab
