"""The shortlisted beam search on the device (csrc/beam_shortlist.hip) against its
numpy specification (beam_shortlist_cases, which test_beam_shortlist_host.py pins to the full
search) and against the dense device search (vasr_ctc_beam_search[_lm]), bit for bit.

Bars.  Everything the feature promises is exact, so everything here is compared as bits: token
lists, beam counts, float64 scores as int64 patterns.  The shortlist kernel's log-probabilities
must be the dense kernel's own values; that is checked end to end -- a certified shortlist search
has the dense search's score bits only if every log-probability it added was the same float32 --
and the complete-mode rows are checked against an fp64 log-softmax within
eps32 * (V / 256 + 12 + |lse| + |lp|): x - max is one rounding, the exp-sum is 256 strided partial
sums of V / 256 terms, a 6-step butterfly and 3 adds (each term and each add within one eps32
relative), logf adds one ulp of lse, and the last subtraction half an ulp of lp.  This envelope
contains test_beam_sweep's variants (fp64 rounded to fp32; the normaliser one ulp up or down).

The specification runs on the device's own shortlist arrays, so its pruned beams and its
uncertified-frame counts must equal the device's exactly, certified or not.

Measured on an MI355X: all 187 tests pass in 11 s, the slowest 1.3 s (V 1000, L 64,
width 32, with its dense reference); 0 of the 75 continuous cases with K >= W + 2 has an uncertified
frame; the tie families with K < V - 1 are uncertified in every frame except twolevel-v33-l6-w7-k14;
model.beam_search peaks at 0.29 / 0.23 MB for (W, K) = (10, auto) / (4, 6) (0.48 MB at (32, 64)) where the
(B, L, V) logits are 0.36 MB and the chunk 0.12 MB.
"""

import numpy as np
import pytest
import torch

import beam_lm_cases as F
import beam_shortlist_cases as C
from test_beam_lm_gpu import same_bits
from test_beam_sweep import SCORE_ATOL, device_beams

pytestmark = pytest.mark.gpu
DEV = "cuda"
ids = lambda c: c["name"]  # noqa: E731
EPS32 = 2.0 ** -23


@pytest.fixture(scope="module")
def ops():
    from velocity_asr import _lib, ops
    _lib.require_device()
    _lib.load()
    return ops


_dense = {}


def dense(ops, c):
    """The dense entry's four tensors for a case's logits, computed once."""
    key = (id(c["logits"]), c["W"], c["blank"])
    if key not in _dense:
        _dense[key] = ops.ctc_beam_search(torch.tensor(c["logits"], device=DEV), c["W"], c["blank"])
    return _dense[key]


def result_bits(res):
    """decode.ctc_beam_search's results with scores as bit patterns."""
    return [[(r.tokens, np.float64(r.score).view(np.int64).item()) for r in ub] for ub in res]


# ----------------------------------------------------------------------------- shortlist kernel
@pytest.mark.parametrize("blank_in_top", [True, False], ids=["blank-in", "blank-out"])
@pytest.mark.parametrize("V,L", [(5, 16), (257, 9), (1000, 16), (20000, 5)])
def test_shortlist_kernel_vs_specification(ops, V, L, blank_in_top):
    """B = 3 with counts [L, 0, min(5, L) - 1 ...] in a strided buffer whose rows past the counts (and
    whose padding) are NaN; K = 1, 12, 64 (clamped to V - 1).  The complete-mode rows against fp64;
    the token lists against the specification on those rows; the kept log-probabilities and the
    blank's as the rows' own bits; rows past a count filled with -1 / -inf."""
    rng = np.random.default_rng(V + L)
    blank = V // 3
    frames = [L, 0, min(5, L) - 1]
    lg = (rng.standard_normal((3, L, V)) * 3.0).astype(np.float32)
    lg[..., blank] += 8.0 if blank_in_top else -8.0
    lg[0, 0, : min(V, 4)] = lg[0, 0, 0]  # equal logits: token order decides
    big = torch.full((3, L + 2, V + 7), float("nan"), device=DEV)
    view = big[:, 1:L + 1, 3:3 + V]
    for b, n in enumerate(frames):
        view[b, :n] = torch.from_numpy(lg[b, :n]).to(DEV)
    assert not view.is_contiguous() and view.stride(2) == 1
    rows = ops.ctc_beam_shortlist(view, 0, blank, frames).cpu().numpy()
    x = lg.astype(np.float64)
    d = x - x.max(-1, keepdims=True)
    lse = np.log(np.exp(d).sum(-1, keepdims=True))
    want = d - lse
    for b, n in enumerate(frames):
        tol = EPS32 * (V / 256 + 12 + np.abs(lse[b, :n]) + np.abs(want[b, :n]))
        err = np.abs(rows[b, :n] - want[b, :n])
        assert (err <= tol).all(), (b, float((err / tol).max()))
        assert (np.abs(rows[b, :n] - F.log_softmax(lg[b, :n])) <= 2 * tol).all()
    for K in (1, 12, 64):
        tok, lp, bl = (t.cpu().numpy() for t in ops.ctc_beam_shortlist(view, K, blank, frames))
        Kc = min(K, V - 1)
        assert tok.shape == lp.shape == (3, L, Kc) and bl.shape == (3, L)
        for b, n in enumerate(frames):
            wt, wl, wb = C.shortlist(rows[b, :n], K, blank)
            assert np.array_equal(tok[b, :n], wt), (K, b)
            assert np.array_equal(lp[b, :n].view(np.int32), wl.view(np.int32)), (K, b)
            assert np.array_equal(bl[b, :n].view(np.int32), wb.view(np.int32)), (K, b)
            assert (tok[b, n:] == -1).all() and np.isneginf(lp[b, n:]).all() and np.isneginf(bl[b, n:]).all()
            assert not (tok[b, :n] == blank).any()
    # the same values whatever the batch and the strides
    alone = ops.ctc_beam_shortlist(torch.from_numpy(lg[2:3]).to(DEV), 12, blank, [frames[2]])
    batch = ops.ctc_beam_shortlist(view, 12, blank, frames)
    for a, bt in zip(alone, batch):
        n = frames[2]
        assert torch.equal(a[0, :n], bt[2, :n])


def test_shortlist_refused_arguments(ops):
    lg = torch.zeros((1, 4, 6), device=DEV)
    for K in (-1, 65):
        with pytest.raises(ValueError, match="K must be"):
            ops.ctc_beam_shortlist(lg, K)
    with pytest.raises(ValueError, match="non-blank"):
        ops.ctc_beam_shortlist(torch.zeros((1, 4, 1), device=DEV), 1)
    with pytest.raises(ValueError, match="frames"):
        ops.ctc_beam_shortlist(lg, 3, frames=[5])
    with pytest.raises(RuntimeError, match="vasr_ctc_beam_shortlist_f32: bad shape"):
        ops.ctc_beam_shortlist(lg, 3, blank=6)
    tok, lp, bl = ops.ctc_beam_shortlist(lg, 3)
    with pytest.raises(ValueError, match="out tokens"):
        ops.ctc_beam_shortlist(lg, 3, out=(tok.long(), lp, bl))
    with pytest.raises(ValueError, match="K = 3 outside"):
        ops.ctc_beam_search_shortlist(tok, lp, bl, 3, 2)
    with pytest.raises(RuntimeError, match="vasr_ctc_beam_search_shortlist: bad shape"):
        ops.ctc_beam_search_shortlist(tok, lp, bl, 6, 33)
    with pytest.raises(ValueError, match="complete rows"):
        ops.ctc_beam_search_shortlist(None, lp, None, 6, 2)


# ----------------------------------------------------------------------------- search
@pytest.mark.parametrize("c", C.device_cases() + C.tie_cases(), ids=ids)
def test_search_vs_dense_entry_and_specification(ops, c, monkeypatch):
    from velocity_asr import decode
    lg = torch.tensor(c["logits"], device=DEV)
    V, W, K, blank = c["V"], c["W"], c["K"], c["blank"]
    want = dense(ops, c)
    short = ops.ctc_beam_shortlist(lg, K, blank)
    got = ops.ctc_beam_search_shortlist(*short, V, W, blank)
    unc = got[4].cpu().tolist()
    # the specification on the device's own arrays: the same pruned search, the same certificate
    spec, spec_unc = C.search(*(t.cpu().numpy() for t in short), W, blank, V)
    assert unc == spec_unc, c["name"]
    assert device_beams(*got[:4]) == spec, c["name"]
    if unc == [0]:
        same_bits(got[:4], want, c["name"])
    same_bits(ops.ctc_beam_search_shortlist(*short, V, W, blank), got, "run to run")
    # the public entry equals shortlist=None in every case; certified ones never reach the exact search
    calls = []
    real = decode._beam_search_exact

    def exact(*a, **k):
        assert unc != [0], "the exact search ran on a certified utterance"
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(decode, "_beam_search_exact", exact)
    plain = decode.ctc_beam_search(lg, beam_width=W, blank_token=blank)
    assert result_bits(plain) == [[(t, np.float64(s).view(np.int64).item()) for t, s in ub]
                                  for ub in device_beams(*want)]
    res = decode.ctc_beam_search(lg, beam_width=W, blank_token=blank, shortlist=K)
    assert result_bits(res) == result_bits(plain), c["name"]
    assert len(calls) == (unc != [0])
    if c["name"].startswith("uniform") and K < V - 1:
        assert unc != [0], "every candidate of a frame ties: the strict certificate cannot hold"
    print(f"{c['name']}: uncertified frames {unc[0]} of {c['logits'].shape[1]}")


def test_uncertified_share_of_the_continuous_cases(ops):
    """The project's rule for undecided cases: at most 1 in 10 (here: of the cases with K >= W + 2,
    the sizes the search is meant for; the host file applies the same cap to the specification)."""
    cases = [c for c in C.device_cases() if c["K"] >= min(c["W"] + 2, c["V"] - 1)]
    bad = []
    for c in cases:
        lg = torch.tensor(c["logits"], device=DEV)
        unc = ops.ctc_beam_search_shortlist(*ops.ctc_beam_shortlist(lg, c["K"], c["blank"]), c["V"], c["W"], c["blank"])[4]
        if int(unc[0]):
            bad.append((c["name"], int(unc[0])))
    print(f"uncertified: {len(bad)} of {len(cases)}: {bad}")
    assert len(bad) * 10 <= len(cases), bad


@pytest.mark.parametrize("c", [c for c in C.device_cases() if c["K"] == min(c["W"] + 2, c["V"] - 1)] + C.tie_cases()[::2],
                         ids=ids)
def test_complete_mode_is_the_dense_entry(ops, c):
    lg = torch.tensor(c["logits"], device=DEV)
    rows = ops.ctc_beam_shortlist(lg, 0, c["blank"])
    got = ops.ctc_beam_search_shortlist(None, rows, None, c["V"], c["W"], c["blank"])
    assert got[4].cpu().tolist() == [0]
    same_bits(got[:4], dense(ops, c), c["name"])


@pytest.mark.parametrize("V,L,W,blank", [(40, 12, 32, 7), (257, 9, 5, 256)])
def test_complete_mode_on_a_ragged_batch(ops, V, L, W, blank):
    """B = 3, counts [L, 0, L - 1], NaN past the counts: the dense kernel reading rows is bitwise the
    dense kernel reading logits, for a device count tensor and for a host list, and certifies all."""
    lg, _ = F.ragged_case(V, L, blank, seed=V + 2, B=3)
    frames = [L, 0, L - 1]
    x = torch.full((3, L, V), float("nan"), device=DEV)
    for b, n in enumerate(frames):
        x[b, :n] = torch.from_numpy(lg[b, :n]).to(DEV)
    for fr in (torch.tensor(frames, dtype=torch.int32, device=DEV), frames):
        got = ops.ctc_beam_search_shortlist(None, ops.ctc_beam_shortlist(x, 0, blank, fr), None, V, W, blank, fr)
        assert got[4].cpu().tolist() == [0, 0, 0]
        same_bits(got[:4], ops.ctc_beam_search(x, W, blank, frames=fr), f"{type(fr).__name__} counts")
    assert device_beams(*got[:4])[1] == [([], 0.0)]


def test_dense_kernel_at_its_lds_limit(ops, monkeypatch):
    """V = 16384 is the largest row the dense kernel holds (64 KiB of dynamic LDS beside its static
    state): bitwise the complete mode on the same logits.  V = 16385 is refused there, and the exact
    search goes through the complete mode."""
    from velocity_asr import decode
    L, W, blank = 3, 2, 0
    assert ops.BEAM_DENSE_MAX_VOCAB == 16384
    lg = (np.random.default_rng(16384).standard_normal((1, L, 16385)) * 3.0).astype(np.float32)
    x = torch.from_numpy(lg).to(DEV)
    at = x[..., :16384]  # strided rows
    full = ops.ctc_beam_search_shortlist(None, ops.ctc_beam_shortlist(at, 0, blank), None, 16384, W, blank)
    assert full[4].cpu().tolist() == [0]
    same_bits(ops.ctc_beam_search(at, W, blank), full[:4], "V = 16384")
    with pytest.raises(RuntimeError, match="bad shape"):
        ops.ctc_beam_search(x, W, blank)
    over = ops.ctc_beam_search_shortlist(None, ops.ctc_beam_shortlist(x, 0, blank), None, 16385, W, blank)
    monkeypatch.setattr(ops, "ctc_beam_search", lambda *a, **k: pytest.fail("the dense entry above its limit"))
    same_bits(decode._beam_search_exact(x, W, blank, None), over[:4], "V = 16385")


def test_large_vocabulary(ops, monkeypatch):
    """V = 20 000 (the dense entry refuses it), L = 6, W = 4: the complete mode against the
    restatement of the reference, the shortlisted search bitwise the complete mode, and the public
    entry, whose exact search must be the complete mode when forced."""
    from velocity_asr import decode
    V, L, W, blank = 20000, 6, 4, 0
    lg = (np.random.default_rng(20).standard_normal((2, L, V)) * 3.0).astype(np.float32)
    x = torch.from_numpy(lg).to(DEV)
    with pytest.raises(RuntimeError, match="bad shape"):
        ops.ctc_beam_search(x, W, blank)
    rows = ops.ctc_beam_shortlist(x, 0, blank)
    full = ops.ctc_beam_search_shortlist(None, rows, None, V, W, blank)
    want = F.search(lg, W, blank)
    got = device_beams(*full[:4])
    for gb, wb in zip(got, want):
        assert [p for p, _ in gb] == [p for p, _ in wb]
        assert np.abs(np.array([s for _, s in gb]) - np.array([s for _, s in wb])).max() <= SCORE_ATOL
    for K in (6, 16, 64):
        short = ops.ctc_beam_search_shortlist(*ops.ctc_beam_shortlist(x, K, blank), V, W, blank)
        assert short[4].cpu().tolist() == [0, 0]
        same_bits(short[:4], full[:4], f"K = {K}")
    res = decode.ctc_beam_search(x, beam_width=W, blank_token=blank, shortlist="auto")
    assert [[(r.tokens, r.score) for r in ub] for ub in res] == got
    same_bits(decode._beam_search_exact(x, W, blank, None), full[:4], "the exact search above the dense limit")
    # K = 1 cannot certify width 4: both utterances go through the exact search, with the same result
    one = decode.ctc_beam_search(x, beam_width=W, blank_token=blank, shortlist=1)
    assert result_bits(one) == result_bits(res)


@pytest.mark.parametrize("V,L,W,blank,K", [(40, 25, 32, 7, 34), (257, 33, 5, 256, 7), (6, 30, 3, 0, 5), (1000, 12, 10, 0, 20)])
def test_ragged_batch(ops, V, L, W, blank, K):
    """B = 5, counts [L, 1, 0, L - 1, 7], NaN past the counts: each utterance bitwise the utterance
    searched alone, the shortlisted search and the public entry alike; a device count tensor and a
    host list give the same bits."""
    from velocity_asr import decode
    lg, frames = F.ragged_case(V, L, blank, seed=V + 1)
    x = torch.full((5, L, V), float("nan"), device=DEV)
    for b, n in enumerate(frames):
        x[b, :n] = torch.from_numpy(lg[b, :n]).to(DEV)
    fr = torch.tensor(frames, dtype=torch.int32, device=DEV)
    short = ops.ctc_beam_shortlist(x, K, blank, fr)
    batch = ops.ctc_beam_search_shortlist(*short, V, W, blank, fr)
    same_bits(ops.ctc_beam_search_shortlist(*ops.ctc_beam_shortlist(x, K, blank, frames), V, W, blank, frames), batch,
              "host counts")
    spec, spec_unc = C.search(*(t.cpu().numpy() for t in short), W, blank, V, frames)
    assert batch[4].cpu().tolist() == spec_unc and device_beams(*batch[:4]) == spec
    assert spec[2] == [([], 0.0)] and spec_unc[2] == 0  # no frames: the single empty beam
    dense_batch = ops.ctc_beam_search(x, W, blank, frames=fr)
    public = decode.ctc_beam_search(x, beam_width=W, blank_token=blank, input_lengths=fr, shortlist=K)
    assert result_bits(public) == result_bits(decode.ctc_beam_search(x, beam_width=W, blank_token=blank, input_lengths=fr))
    for b, n in enumerate(frames):
        xb = torch.from_numpy(lg[b:b + 1]).to(DEV)
        alone = ops.ctc_beam_search_shortlist(*ops.ctc_beam_shortlist(xb, K, blank, [n]), V, W, blank, [n])
        same_bits([t[b:b + 1] for t in batch], alone, f"utterance {b} alone")
        if spec_unc[b] == 0:
            same_bits([t[b:b + 1] for t in batch[:4]], [t[b:b + 1] for t in dense_batch], f"utterance {b} vs dense")
        one = decode.ctc_beam_search(xb, beam_width=W, blank_token=blank, input_lengths=[n], shortlist=K)
        assert result_bits(one) == result_bits(public[b:b + 1])
    assert batch[0].shape == (5, W, L)


def test_counts_outside_the_logits_are_clamped(ops):
    lg, _ = F.ragged_case(12, 9, 0, seed=1, B=3)
    x = torch.from_numpy(lg).to(DEV)
    wild = torch.tensor([-3, 9 + 50, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    a = ops.ctc_beam_shortlist(x, 6, 0, wild)
    b = ops.ctc_beam_shortlist(x, 6, 0, [0, 9, 9])
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    same_bits(ops.ctc_beam_search_shortlist(*a, 12, 4, 0, wild), ops.ctc_beam_search_shortlist(*b, 12, 4, 0, [0, 9, 9]))


def test_shortlist_with_a_language_model_is_refused(ops):
    from velocity_asr import decode
    V, blank = 40, 39
    lm = F.trained_table(np.random.default_rng(3), V, blank)
    x = torch.from_numpy(F.ragged_case(V, 10, blank, seed=2, B=2)[0]).to(DEV)
    with pytest.raises(ValueError, match="language model"):
        decode.ctc_beam_search(x, beam_width=4, blank_token=blank, lm_scorer=lm, lm_weight=0.5, shortlist="auto")
    dec = decode.CTCDecoder(decode.create_default_vocabulary(V), blank_token=blank)
    with pytest.raises(ValueError, match="language model"):
        dec.decode_beam_search(x, beam_width=4, lm_scorer=lm, lm_weight=0.5, shortlist=8)
    # weight 0 switches the scorer off, as without a shortlist
    off = decode.ctc_beam_search(x, beam_width=4, blank_token=blank, lm_scorer=lm, lm_weight=0.0, shortlist="auto")
    assert result_bits(off) == result_bits(decode.ctc_beam_search(x, beam_width=4, blank_token=blank))
    assert dec.decode_beam_search(x, beam_width=4, shortlist="auto") == dec.decode_beam_search(x, beam_width=4)


# ----------------------------------------------------------------------------- model
SMALL_CFG = dict(d_model=64, ssm_layers=2, ssm_state_dim=32, global_ssm_state_dim=16, attention_heads=2,
                 attention_dim=32, vocab_size=300)
SAMPLES = [32000, 20000, 27200]


def small_model():
    import velocity_asr as va
    from velocity_asr import synthetic as S
    m = va.VELOCITYASR(va.VelocityASRConfig(**SMALL_CFG))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.make_weights(SMALL_CFG, seed=5).items()}, strict=True)
    return m.to(DEV).eval()


def padded_mel(m, samples):
    from velocity_asr import synthetic as S
    from velocity_asr.audio import HOP_LENGTH, mel_on_device
    audio = torch.from_numpy(S.make_audio(len(samples), max(samples), seed=31)).to(DEV)
    for b, n in enumerate(samples):
        audio[b, n:] = 0
    mel = mel_on_device(audio, n_mels=m.config.mel_bins, lengths=samples, frame_pad=m.temporal_binding.conv_padding())
    return mel, [n // HOP_LENGTH + 1 for n in samples]


@pytest.mark.parametrize("W,K", [(10, "auto"), (4, 6), (32, 34)])
def test_model_beam_search_without_logits(ops, W, K, monkeypatch):
    """d_model 64, vocabulary 300, three clips of unequal length, chunk_bytes for one utterance at a
    time (three chunks): bitwise the path through model(mel), without ever holding (B, L, V)."""
    from velocity_asr import decode
    m = small_model()
    assert m.ctc_head.fusable()
    mel, frames = padded_mel(m, SAMPLES)
    rows = [m.get_output_length(f) for f in frames]
    logits = m(mel, frames=frames)
    B, L, V = logits.shape
    assert (B, V) == (3, 300) and max(rows) <= L
    want = decode.ctc_beam_search(logits, beam_width=W, blank_token=0, input_lengths=rows, shortlist=K)
    assert result_bits(want) == result_bits(decode.ctc_beam_search(logits, beam_width=W, blank_token=0, input_lengths=rows))
    chunk = L * V * 4
    chunks = []
    real = ops.ctc_beam_shortlist
    monkeypatch.setattr(ops, "ctc_beam_shortlist", lambda x, *a, **k: chunks.append(tuple(x.shape)) or real(x, *a, **k))
    got = m.beam_search(mel, frames=frames, beam_width=W, shortlist=K, chunk_bytes=chunk)
    assert [s for s in chunks if s[2] == V][:3] == [(1, L, V)] * 3
    assert result_bits(got) == result_bits(want)
    assert result_bits(m.beam_search(mel, frames=frames, beam_width=W, shortlist=K)) == result_bits(want)  # one chunk
    # the head alone, from the rows the model hands it: peak memory below one (B, L, V) tensor plus the chunk
    del logits
    with torch.no_grad():
        _, x, normalized = m._local_global(mel.to(torch.float32), rows)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = m.ctc_head.beam_search(x, W, 0, rows=rows, shortlist=K, chunk_bytes=chunk, normalized=normalized)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert result_bits(res) == result_bits(want)
    print(f"W {W} K {K}: peak {peak} bytes, (B, L, V) {B * L * V * 4}, chunk {chunk}")
    assert peak < B * L * V * 4 + chunk


def test_model_beam_search_through_the_logits_where_the_head_is_not_plain_fp32(ops):
    from velocity_asr import decode
    m = small_model().to(torch.bfloat16)
    assert not m.ctc_head.fusable()
    mel, frames = padded_mel(m, SAMPLES[:2])
    rows = [m.get_output_length(f) for f in frames]
    want = decode.ctc_beam_search(m(mel, frames=frames), beam_width=5, blank_token=0, input_lengths=rows, shortlist="auto")
    assert result_bits(m.beam_search(mel, frames=frames, beam_width=5)) == result_bits(want)


def test_decode_batch_gives_the_same_tokens_either_way(ops, monkeypatch):
    import velocity_asr as va
    from velocity_asr import synthetic as S
    from velocity_asr import transcription as T
    m = small_model()
    dec = va.CTCDecoder(va.create_default_vocabulary(m.config.vocab_size))
    audio = torch.from_numpy(S.make_audio(3, max(SAMPLES), seed=31)).to(DEV)
    for b, n in enumerate(SAMPLES):
        audio[b, n:] = 0
    out = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("VASR_BEAM_SHORTLIST", flag)
        searched = []
        real = m.beam_search
        monkeypatch.setattr(m, "beam_search", lambda *a, **k: searched.append(1) or real(*a, **k))
        out[flag] = (T._decode_batch(m, audio, dec, False, beam_width=6, lengths=SAMPLES, raw=True),
                     T._decode_batch(m, audio, dec, False, beam_width=6, lengths=SAMPLES))
        assert len(searched) == (2 if flag == "1" else 0)
        monkeypatch.undo()
    assert out["0"] == out["1"] and len(out["1"][0]) == 3
    # a language model keeps the dense search whatever the flag says
    monkeypatch.setenv("VASR_BEAM_SHORTLIST", "1")
    lm = F.trained_table(np.random.default_rng(9), m.config.vocab_size, 0)
    monkeypatch.setattr(m, "beam_search", lambda *a, **k: pytest.fail("shortlist with a language model"))
    assert len(T._decode_batch(m, audio, dec, False, beam_width=6, lengths=SAMPLES, lm=lm, lm_weight=0.5)) == 3
