"""The standard CTC prefix beam search on the device (csrc/beam_prefix.hip) against
its Python specification (beam_prefix_cases, which test_beam_prefix_host.py pins to torch's ctc_loss).

Bars.  The dense entry forms its own float32 log-softmax, which differs from numpy's in the last
place, so against the specification on numpy's values a case counts where it is decided
(test_beam_sweep's rule: the same prefixes under the three other roundings of the log-softmax):
there prefixes and order are identical and score and logp lie within 1e-4, the sweep's bar (a
float32 log-probability near -10 carries 1e-6, and at most 65 of them are summed).  The pruned
entry is compared on the device's own shortlist arrays, where the specification adds the very same
float32 values: identical prefixes where decided and 1e-9 on score and logp, which leaves room only
for the order of float64 operations and the last place of exp / log1p (|values| < 1e3, eps 2e-16).
"""

import numpy as np
import pytest
import torch

import beam_lm_cases as F
import beam_prefix_cases as P
from test_beam_shortlist_gpu import SAMPLES, padded_mel, small_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
ids = lambda c: c["name"]  # noqa: E731
SCORE_ATOL = 1e-4  # tests/test_beam_sweep.py
ORDER_ATOL = 1e-9


@pytest.fixture(scope="module")
def ops():
    from velocity_asr import _lib, ops
    _lib.require_device()
    _lib.load()
    return ops


def beams_of(toks, lens, scores, logp, nb):
    """The five device tensors as the specification's per-utterance [(tokens, logp, score)]; rows
    past an utterance's beam count must be untouched."""
    toks, lens, scores, logp, nb = (t.cpu().numpy() for t in (toks, lens, scores, logp, nb))
    out = []
    for b in range(toks.shape[0]):
        n = int(nb[b])
        assert not lens[b, n:].any() and not scores[b, n:].any() and not logp[b, n:].any() and not toks[b, n:].any()
        out.append([(toks[b, r, :lens[b, r]].tolist(), float(logp[b, r]), float(scores[b, r])) for r in range(n)])
    return out


def compare(got, want, decided, atol, what):
    worst = 0.0
    assert len(got) == len(want), what
    for gb, wb in zip(got, want):
        assert len(gb) == len(wb), what
        if decided:
            assert [p for p, _, _ in gb] == [p for p, _, _ in wb], what
            for (_, gl, gs), (_, wl, ws) in zip(gb, wb):
                worst = max(worst, abs(gl - wl), abs(gs - ws))
    assert worst <= atol, (what, worst)
    return worst


def same_bits(a, b, what=""):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x, y), what
    for k in (2, 3):  # score and logp as bit patterns
        assert torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)), what


def run(ops, c, lg=None, **kw):
    lg = torch.tensor(c["logits"], device=DEV) if lg is None else lg
    table = None if c["table"] is None else torch.tensor(c["table"], device=DEV)
    return ops.ctc_prefix_beam_search(lg, c["W"], c["blank"], lm_table=table, alpha=c["alpha"], beta=c["beta"], **kw)


# ----------------------------------------------------------------------------- dense entry
@pytest.mark.parametrize("c", P.exhaustive_cases() + P.device_cases(), ids=ids)
def test_dense_entry_vs_specification(ops, c):
    want, decided = P.expected(c)
    got = run(ops, c)
    worst = compare(beams_of(*got), want, decided, SCORE_ATOL, c["name"])
    same_bits(run(ops, c), got, "run to run")
    print(f"{c['name']}: decided {decided}, worst |d score|, |d logp| {worst:.2e}")


@pytest.mark.parametrize("c", P.exhaustive_cases(), ids=ids)
def test_every_prefix_sums_to_one(ops, c):
    """W = 32 keeps every prefix of the exhaustive shapes: their probabilities sum to 1."""
    logp = run(ops, c)[3][0].cpu().numpy()
    n = len(P.expected(c)[0][0])
    assert abs(np.log(np.exp(logp[:n]).sum())) <= 1e-6


@pytest.mark.parametrize("c", P.uniform_cases(), ids=ids)
def test_uniform_rows_tie_bitwise(ops, c):
    """L = 1, all logits equal: every candidate ties, so the order is the positions' -- the empty
    prefix, then tokens ascending -- and all scores are one bit pattern."""
    got = beams_of(*run(ops, c))
    tokens = [t for t in range(c["V"]) if t != c["blank"]]
    assert [p for p, _, _ in got[0]] == ([[]] + [[t] for t in tokens])[:c["W"]]
    assert len({np.float64(s).view(np.int64).item() for _, _, s in got[0]}) == 1
    assert [s for _, _, s in got[0]] == [lp for _, lp, _ in got[0]]
    compare(got, P.expected(c)[0], True, SCORE_ATOL, c["name"])


@pytest.mark.parametrize("V,L,W,blank,alpha,beta", [(40, 25, 32, 7, 0.5, 0.5), (257, 12, 5, 256, 0.0, 0.0)])
def test_ragged_batch(ops, V, L, W, blank, alpha, beta):
    """B = 5 with counts [L, 1, 0, L - 1, 7] in a strided buffer whose rows past the counts are NaN
    or 1e30: each utterance bitwise the utterance alone, for device and for host counts; the
    specification on numpy's log-softmax where decided."""
    lg, frames = F.ragged_case(V, L, blank, seed=V + 3)
    table = F.random_table(np.random.default_rng(V), V, blank)
    big = torch.full((5, L + 3, V + 5), float("nan"), device=DEV)
    big[:, ::2] = 1e30
    view = big[:, 2:L + 2, 1:1 + V]
    for b, n in enumerate(frames):
        view[b, :n] = torch.from_numpy(lg[b, :n]).to(DEV)
    assert not view.is_contiguous()
    kw = dict(lm_table=torch.tensor(table, device=DEV), alpha=alpha, beta=beta)
    fr = torch.tensor(frames, dtype=torch.int32, device=DEV)
    batch = ops.ctc_prefix_beam_search(view, W, blank, frames=fr, **kw)
    same_bits(ops.ctc_prefix_beam_search(view, W, blank, frames=frames, **kw), batch, "host counts")
    got = beams_of(*batch)
    assert got[2] == [([], 0.0, 0.0)]  # no frames: the single empty beam
    for b, n in enumerate(frames):
        alone = ops.ctc_prefix_beam_search(torch.from_numpy(lg[b:b + 1, :n]).to(DEV), W, blank, **kw)
        for k, (x, y) in enumerate(zip(batch, alone)):
            assert torch.equal(x[b:b + 1, ..., :max(n, 1)] if k == 0 else x[b:b + 1], y), (b, k)
        c = dict(name=f"ragged-{V}-{b}", logits=lg[b:b + 1, :n], W=W, blank=blank, table=table, alpha=alpha, beta=beta)
        want, decided = P.expected(c)
        compare(got[b:b + 1], want, decided, SCORE_ATOL, c["name"])
    wild = torch.tensor([L + 9, 1, -4, L - 1, 7], dtype=torch.int32, device=DEV)  # clamped in the kernel
    same_bits(ops.ctc_prefix_beam_search(view, W, blank, frames=wild, **kw), batch, "clamped counts")


def test_minus_infinity_logits(ops):
    """A token that never occurs (a -inf column) and frames whose blank is -inf: such contributions
    are not made, so the keys they alone would create do not exist."""
    V, L, W, blank = 9, 10, 32, 2
    lg = (np.random.default_rng(5).standard_normal((1, L, V)) * 1.5).astype(np.float32)
    lg[:, :, 6] = -np.inf
    lg[:, 3:6, blank] = -np.inf
    lg[:, 0, blank] = -np.inf  # the empty prefix does not survive the first frame
    c = dict(name="minus-inf", logits=lg, W=W, blank=blank, table=None, alpha=0.0, beta=0.3)
    want, decided = P.expected(c)
    got = beams_of(*run(ops, c))
    assert all(6 not in p and p for p, _, _ in got[0])
    assert decided  # so that compare looks at the prefixes
    compare(got, want, decided, SCORE_ATOL, c["name"])
    one = dict(c, name="minus-inf-l1", logits=lg[:, :1])
    assert P.expected(one)[1]
    assert [p for p, _, _ in beams_of(*run(ops, one))[0]] == [p for p, _, _ in P.expected(one)[0][0]]
    assert len(P.expected(one)[0][0]) == V - 2  # neither the blank extension nor token 6


@pytest.mark.parametrize("c", P.blank_inf_cases(), ids=ids)
def test_blank_minus_infinity_at_a_narrow_width(ops, c):
    """V 5, L 8, W 6, the blank at -inf in three frames: a prefix without its blank contribution has
    its repeat's position, which its extension by the same token shares, and both survive some frame
    (test_beam_prefix_host.py asserts that, and that every case is decided).  A winner must resolve to
    its own key: the dense entry, and the shortlist entry with every token kept."""
    want, decided = P.expected(c)
    assert decided
    compare(beams_of(*run(ops, c)), want, decided, SCORE_ATOL, c["name"])
    lg = torch.tensor(c["logits"], device=DEV)
    short = ops.ctc_beam_shortlist(lg, c["V"] - 1, c["blank"])
    got = ops.ctc_prefix_beam_search_shortlist(*short, c["V"], c["W"], c["blank"], beta=c["beta"])
    compare(beams_of(*got), want, decided, SCORE_ATOL, c["name"] + " shortlist")


def test_dense_entry_at_its_lds_limit(ops):
    V, L, W = 16384, 2, 2
    lg = (np.random.default_rng(16).standard_normal((1, L, V + 1)) * 3.0).astype(np.float32)
    x = torch.from_numpy(lg).to(DEV)
    c = dict(name="v16384", logits=lg[..., :V], W=W, blank=0, table=None, alpha=0.0, beta=0.0)
    want, decided = P.expected(c)
    compare(beams_of(*ops.ctc_prefix_beam_search(x[..., :V], W, 0)), want, decided, SCORE_ATOL, c["name"])
    with pytest.raises(RuntimeError, match="vasr_ctc_prefix_beam_search: bad shape"):
        ops.ctc_prefix_beam_search(x, W, 0)


def test_refused_arguments(ops):
    lg = torch.zeros((1, 4, 6), device=DEV)
    with pytest.raises(RuntimeError, match="vasr_ctc_prefix_beam_search: bad shape"):
        ops.ctc_prefix_beam_search(lg, 33)
    with pytest.raises(RuntimeError, match="vasr_ctc_prefix_beam_search: bad shape"):
        ops.ctc_prefix_beam_search(lg, 4, blank=6)
    with pytest.raises(ValueError, match="lm_table must be"):
        ops.ctc_prefix_beam_search(lg, 4, lm_table=torch.zeros((6, 6), device=DEV), alpha=1.0)
    with pytest.raises(RuntimeError, match="NaN"):
        ops.ctc_prefix_beam_search(lg, 4, beta=float("nan"))
    with pytest.raises(ValueError, match="frames"):
        ops.ctc_prefix_beam_search(lg, 4, frames=[5])
    tok, lp, bl = ops.ctc_beam_shortlist(lg, 3)
    with pytest.raises(ValueError, match="K = 3 outside"):
        ops.ctc_prefix_beam_search_shortlist(tok, lp, bl, 3, 2)
    with pytest.raises(RuntimeError, match="vasr_ctc_prefix_beam_search_shortlist: bad shape"):
        ops.ctc_prefix_beam_search_shortlist(tok, lp, bl, 6, 33)
    with pytest.raises(ValueError, match="lm_table must be"):
        ops.ctc_prefix_beam_search_shortlist(tok, lp, bl, 6, 4, lm_table=torch.zeros((7, 5), device=DEV), alpha=1.0)
    with pytest.raises(ValueError, match="int32"):
        ops.ctc_prefix_beam_search_shortlist(tok.long(), lp, bl, 6, 4)


# ----------------------------------------------------------------------------- pruned entry
PRUNED = [c for c in P.device_cases() if (c["alpha"], c["beta"]) in ((0.0, 0.0), (0.5, 0.5)) and c["V"] > 2]


@pytest.mark.parametrize("c", PRUNED, ids=ids)
def test_pruned_entry_vs_specification(ops, c):
    """K = 2 W within 1..min(64, V - 2): the specification on rows rebuilt from the device's own
    shortlist arrays; then K = V - 1 (nothing pruned) against the dense entry."""
    lg = torch.tensor(c["logits"], device=DEV)
    table = torch.tensor(c["table"], device=DEV)
    V, W, blank = c["V"], c["W"], c["blank"]
    kw = dict(lm_table=table, alpha=c["alpha"], beta=c["beta"])
    args = dict(table=c["table"], alpha=c["alpha"], beta=c["beta"])
    K = max(1, min(2 * W, 64, V - 2))
    short = ops.ctc_beam_shortlist(lg, K, blank)
    got = ops.ctc_prefix_beam_search_shortlist(*short, V, W, blank, **kw)
    rows = P.rows_of_shortlist(*(t.cpu().numpy() for t in short), V, blank)
    margins = []
    want = P.search(rows, W, blank, margins=margins, **args)
    decided = margins[0] > 1e-7  # the order must not hang on the last places of a float64 sum
    worst = compare(beams_of(*got), want, decided, ORDER_ATOL, c["name"])
    same_bits(ops.ctc_prefix_beam_search_shortlist(*short, V, W, blank, **kw), got, "run to run")
    if V - 1 <= 64:
        full = ops.ctc_beam_shortlist(lg, V - 1, blank)
        margins = []
        P.search(P.rows_of_shortlist(*(t.cpu().numpy() for t in full), V, blank), W, blank, margins=margins, **args)
        compare(beams_of(*ops.ctc_prefix_beam_search_shortlist(*full, V, W, blank, **kw)), beams_of(*run(ops, c)),
                margins[0] > 1e-7, ORDER_ATOL, c["name"] + " K = V - 1")
    print(f"{c['name']}: K {K}, decided {decided}, worst {worst:.2e}")


def test_public_entry(ops):
    """decode.ctc_prefix_beam_search: a BigramLM on the device, token_topk through the shortlist
    launch, any other scorer and CPU logits on the host -- all the same beams."""
    from velocity_asr import decode
    c = [c for c in P.device_cases() if c["name"].startswith("v40-") and c["alpha"] == 0.5 and c["beta"] == 0.5][0]
    lg = torch.tensor(c["logits"], device=DEV)
    lm = decode.BigramLM(c["table"])
    kw = dict(beam_width=c["W"], blank_token=c["blank"], lm_weight=0.5, length_bonus=0.5)
    dev = decode.ctc_prefix_beam_search(lg, lm_scorer=lm, **kw)
    assert [(r.tokens, r.logp, r.score) for r in dev[0]] == beams_of(*run(ops, c))[0]

    class Other:
        score = staticmethod(lambda tokens: F.table_score(c["table"], tokens))

    for host in (decode.ctc_prefix_beam_search(lg, lm_scorer=Other(), **kw),
                 decode.ctc_prefix_beam_search(lg.cpu(), lm_scorer=lm, **kw)):
        assert [r.tokens for r in host[0]] == [r.tokens for r in dev[0]]
        assert max(abs(h.score - d.score) + abs(h.logp - d.logp) for h, d in zip(host[0], dev[0])) <= SCORE_ATOL
    pruned = decode.ctc_prefix_beam_search(lg, lm_scorer=lm, token_topk=12, **kw)
    short = ops.ctc_beam_shortlist(lg, 12, c["blank"])
    want = ops.ctc_prefix_beam_search_shortlist(*short, c["V"], c["W"], c["blank"],
                                                lm_table=torch.tensor(c["table"], device=DEV), alpha=0.5, beta=0.5)
    assert [(r.tokens, r.logp, r.score) for r in pruned[0]] == beams_of(*want)[0]
    dec = decode.CTCDecoder(decode.create_default_vocabulary(c["V"]), blank_token=c["blank"])
    assert dec.decode_prefix_beam_search(lg, c["W"], lm_scorer=lm, lm_weight=0.5, length_bonus=0.5) == \
        [dec._tokens_to_text(dev[0][0].tokens)]


# ----------------------------------------------------------------------------- model
def results(res):
    return [[(r.tokens, np.float64(r.score).view(np.int64).item(), np.float64(r.logp).view(np.int64).item()) for r in ub]
            for ub in res]


def test_model_prefix_beam_search_without_logits(ops, monkeypatch):
    """d_model 64, vocabulary 300, three clips of unequal length, chunk_bytes for one utterance at a
    time (three chunks): bitwise decode.ctc_prefix_beam_search(model(mel), token_topk=K), with a
    table, without ever holding (B, L, V)."""
    from velocity_asr import decode
    m = small_model()
    mel, frames = padded_mel(m, SAMPLES)
    rows = [m.get_output_length(f) for f in frames]
    logits = m(mel, frames=frames)
    B, L, V = logits.shape
    W, K = 10, 20
    lm = F.trained_table(np.random.default_rng(4), V, 0)
    kw = dict(lm_weight=0.5, length_bonus=0.25)
    want = decode.ctc_prefix_beam_search(logits, W, 0, lm, input_lengths=rows, token_topk=K, **kw)
    assert all(len(ub) == W and ub[0].logp <= 0.0 for ub in want)
    chunk = L * V * 4
    chunks = []
    real = ops.ctc_beam_shortlist
    monkeypatch.setattr(ops, "ctc_beam_shortlist", lambda x, *a, **k: chunks.append(tuple(x.shape)) or real(x, *a, **k))
    got = m.prefix_beam_search(mel, frames=frames, beam_width=W, token_topk=K, lm=lm, chunk_bytes=chunk, **kw)
    assert chunks == [(1, L, V)] * 3
    assert results(got) == results(want)
    monkeypatch.undo()
    assert results(m.prefix_beam_search(mel, frames=frames, beam_width=W, token_topk=K, lm=lm, **kw)) == results(want)
    auto = m.prefix_beam_search(mel, frames=frames, beam_width=W)
    assert results(auto) == results(decode.ctc_prefix_beam_search(logits, W, 0, input_lengths=rows, token_topk="auto"))
    del logits
    with torch.no_grad():
        _, x, normalized = m._local_global(mel.to(torch.float32), rows)
    lm.device_table(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = m.ctc_head.prefix_beam_search(x, W, 0, rows=rows, token_topk=K, lm=lm, chunk_bytes=chunk, normalized=normalized,
                                        **kw)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert results(res) == results(want)
    print(f"W {W} K {K}: peak {peak} bytes, (B, L, V) {B * L * V * 4}, chunk {chunk}")
    assert peak < B * L * V * 4 + chunk


def test_transcribe_files_with_the_prefix_search(ops, tmp_path, monkeypatch):
    import velocity_asr as va
    from velocity_asr import synthetic as S
    from velocity_asr import transcription as T
    from velocity_asr.audio import write_wav
    m = small_model()
    dec = va.CTCDecoder(va.create_default_vocabulary(m.config.vocab_size))
    paths = []
    for i, n in enumerate((24000, 16333)):
        paths.append(str(tmp_path / f"c{i}.wav"))
        write_wav(paths[-1], S.make_audio(1, n, seed=70 + i)[0])
    calls = []
    real = m.prefix_beam_search
    monkeypatch.setattr(m, "prefix_beam_search", lambda *a, **k: calls.append(k) or real(*a, **k))
    got = T.transcribe_files(m, paths, dec, DEV, beam_width=4, search="prefix", length_bonus=0.5, token_topk=8)
    assert len(calls) == 1 and calls[0]["length_bonus"] == 0.5 and calls[0]["token_topk"] == 8
    assert [r["file"] for r in got] == paths and all(isinstance(r["transcription"], str) for r in got)
    for p, r in zip(paths, got):  # a file alone gives the same text
        assert T.transcribe_files(m, [p], dec, DEV, beam_width=4, search="prefix", length_bonus=0.5, token_topk=8)[0] == r
    calls.clear()
    T.transcribe_files(m, paths, dec, DEV, beam_width=4)  # the default is the reference's search
    assert not calls
    with pytest.raises(ValueError, match="search must be"):
        T.transcribe_files(m, paths, dec, DEV, beam_width=4, search="standard")
