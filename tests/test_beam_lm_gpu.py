"""vasr_ctc_beam_search_lm (csrc/beam.hip) on the device: per-utterance frame
counts and the bigram table, against the old entry (bitwise, where the extras are no-ops), against
the same utterance searched alone (bitwise) and against beam_lm_cases.search, the restatement that
test_beam_lm_host.py pins to the reference.

Bar, as tests/test_beam.py and tests/test_beam_sweep.py: the number of beams and every prefix
identical on decided cases, scores within 1e-4 absolute at L <= 65.  The LM adds exact float64
terms of float32 table entries -- lm_weight * S is one rounded product of values both sides hold
bit for bit -- so the only source of error is still the fp32 log-softmax the bar was set for.

Exact ties: in the tie cases every log-probability sum and every lm_weight * S is exact in
float64, so tied candidates tie bit for bit on both sides and insertion order alone decides; an LM
term on the wrong candidate, or missing from a repeat, changes the prefixes.  All tie cases are
decided and at most 1 in 10 continuous cases may be undecided (asserted in the host file; 0 of 28).

Measured on an MI355X: all 38 LM cases identical in prefixes and beam counts, worst
|score - restatement| 9.3e-6 (lm-v64-l64-w2-b0-x1.0-s2; 2.4e-6 in the tie families; 6.8e-6 ragged), 0.09
of the bar.
"""

import numpy as np
import pytest
import torch

import beam_lm_cases as C
from conftest import record_metric
from oracle import velocity_ref as R
from test_beam_sweep import SCORE_ATOL, device_beams

pytestmark = pytest.mark.gpu
DEV = "cuda"
ids = lambda c: c["name"]  # noqa: E731


@pytest.fixture(scope="module")
def ops():
    from velocity_asr import _lib, ops
    _lib.require_device()
    _lib.load()
    return ops


def compare(got, want, decided, what):
    """The sweep's rule: beam counts identical, prefixes identical where the case is decided, and
    scores within 1e-4 always -- rank by rank, which is prefix by prefix on a decided case.
    Returns the largest |dscore|."""
    worst = 0.0
    assert len(got) == len(want)
    for gb, wb in zip(got, want):
        assert len(gb) == len(wb), f"{what}: {len(gb)} beams, restatement {len(wb)}"
        if decided:
            assert [p for p, _ in gb] == [p for p, _ in wb], what
        if gb:
            d = np.abs(np.array([s for _, s in gb]) - np.array([s for _, s in wb]))
            worst = max(worst, float(d.max()))
            assert (d <= SCORE_ATOL).all(), f"{what}: score differs by {d.max():.3e}"
    return worst


def same_bits(a, b, what=""):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x, y), what
    # scores as bit patterns: torch.equal would let -0.0 pass for 0.0
    assert torch.equal(a[2].view(torch.int64), b[2].view(torch.int64)), what


def on_device(c):
    return torch.tensor(c["logits"], device=DEV), torch.tensor(c["table"], device=DEV)


# ----------------------------------------------------------------------------- no-op identities
@pytest.mark.parametrize("c", [C.continuous_cases()[k] for k in (3, 6, 9, 12)] + C.tie_cases()[2:4], ids=ids)
def test_extras_that_do_nothing_give_the_old_entrys_bits(ops, c):
    lg, table = on_device(c)
    lg = torch.cat([lg, lg.flip(1)])
    B, L, _ = lg.shape
    old = ops.ctc_beam_search(lg, c["W"], c["blank"])
    same_bits(ops.ctc_beam_search(lg, c["W"], c["blank"], frames=None, lm_table=None), old, "no extras")
    same_bits(ops.ctc_beam_search(lg, c["W"], c["blank"], lm_table=table, lm_weight=0.0), old, "weight 0")
    same_bits(ops.ctc_beam_search(lg, c["W"], c["blank"], frames=[L] * B), old, "frames = L, host")
    same_bits(ops.ctc_beam_search(lg, c["W"], c["blank"], frames=torch.full((B,), L, device=DEV)), old, "frames = L")


# ----------------------------------------------------------------------------- ragged
@pytest.mark.parametrize("V,L,W,blank", [(40, 25, 32, 7), (257, 65, 5, 256), (6, 30, 3, 0)])
def test_ragged_batch(ops, V, L, W, blank):
    """B = 5, frames [L, 1, 0, L - 1, 7], strided logits.  Each utterance: the oracle on its own
    slice; bitwise the utterance searched alone at B = 1; the same bits whatever lies in the rows
    past its count (NaN, +1e30); the same bits for a device int32 count tensor and a host list."""
    lg, frames = C.ragged_case(V, L, blank, seed=V)
    B = len(frames)
    runs = []
    for fill in (float("nan"), 1e30):
        big = torch.full((B, L + 2, V + 9), fill, device=DEV)
        view = big[:, 1:L + 1, 4:4 + V]
        for b, n in enumerate(frames):
            view[b, :n] = torch.from_numpy(lg[b, :n]).to(DEV)
        assert not view.is_contiguous() and view.stride(2) == 1
        runs.append(ops.ctc_beam_search(view, W, blank, frames=torch.tensor(frames, dtype=torch.int32, device=DEV)))
        runs.append(ops.ctc_beam_search(view, W, blank, frames=frames))
    for r in runs[1:]:
        same_bits(r, runs[0], "fill / count form")
    got = device_beams(*runs[0])
    worst = 0.0
    for b, n in enumerate(frames):
        c = dict(name=f"ragged-v{V}-l{L}-w{W}-b{blank}-u{b}", logits=lg[b:b + 1, :n], W=W, blank=blank)
        want, decided = C.expected(c)
        assert want == R.ctc_beam_search(lg[b:b + 1, :n], W, blank)  # the oracle itself
        worst = max(worst, compare(got[b:b + 1], want, decided, c["name"]))
        alone = ops.ctc_beam_search(torch.from_numpy(lg[b:b + 1]).to(DEV), W, blank, frames=[n])
        same_bits([x[b:b + 1] for x in runs[0]], alone, f"utterance {b} alone")
    assert got[2] == [([], 0.0)]  # no frames: the single empty beam
    toks = runs[0][0].cpu().numpy()
    assert toks.shape == (B, W, L)  # rows keep the (B, W, L) layout
    record_metric("beam_lm", case=f"ragged-v{V}-l{L}-w{W}", max_dscore=worst)
    print(f"ragged v{V} l{L} w{W}: max |dscore| {worst:.3e}")


def test_counts_outside_the_logits(ops):
    """A device count is taken without a look at it, so the kernel clamps it to 0..L; a host
    sequence outside 0..L is refused."""
    lg, _ = C.ragged_case(12, 9, 0, seed=1, B=3)
    x = torch.from_numpy(lg).to(DEV)
    got = ops.ctc_beam_search(x, 4, 0, frames=torch.tensor([-3, 9 + 50, 2 ** 31 - 1], dtype=torch.int32, device=DEV))
    same_bits(got, ops.ctc_beam_search(x, 4, 0, frames=[0, 9, 9]), "clamped")
    for bad in ([0, 10, 3], [-1, 2, 3]):
        with pytest.raises(ValueError, match="frames"):
            ops.ctc_beam_search(x, 4, 0, frames=bad)
    with pytest.raises(ValueError, match="frames"):
        ops.ctc_beam_search(x, 4, 0, frames=[1, 2])
    with pytest.raises(ValueError, match="lm_table"):
        ops.ctc_beam_search(x, 4, 0, lm_table=torch.zeros((12, 12), device=DEV), lm_weight=1.0)


# ----------------------------------------------------------------------------- language model
@pytest.mark.parametrize("c", C.continuous_cases() + C.tie_cases(), ids=ids)
def test_lm_search_vs_restatement(ops, c):
    want, decided = C.expected(c)
    assert decided or c["kind"] != "tie"
    lg, table = on_device(c)
    first = ops.ctc_beam_search(lg, c["W"], c["blank"], lm_table=table, lm_weight=c["lm_weight"])
    got = device_beams(*first)
    worst = compare(got, want, decided, c["name"])
    same_bits(ops.ctc_beam_search(lg, c["W"], c["blank"], lm_table=table, lm_weight=c["lm_weight"]), first, "run to run")
    # a table inside a wider buffer (row stride above V) is read in place
    wide = torch.full((table.shape[0], table.shape[1] + 5), float("nan"), device=DEV)
    wide[:, 2:2 + table.shape[1]] = table
    same_bits(ops.ctc_beam_search(lg, c["W"], c["blank"], lm_table=wide[:, 2:2 + table.shape[1]],
                                  lm_weight=c["lm_weight"]), first, "strided table")
    record_metric("beam_lm", case=c["name"], decided=decided, max_dscore=worst)
    print(f"{c['name']}: decided {decided}, {len(got[0])} beams, max |dscore| {worst:.3e}")


@pytest.mark.parametrize("W,weight", [(8, 1.0), (32, 0.3)])
def test_lm_with_ragged_batch(ops, W, weight):
    """B = 4 with counts [L, 1, 0, L - 1] and a table: the restatement per utterance, and bitwise
    the utterance alone."""
    V, L, blank = 40, 25, 39
    lg, frames = C.ragged_case(V, L, blank, seed=77, B=4)
    table = C.trained_table(np.random.default_rng(78), V, blank).table
    x = torch.from_numpy(lg).to(DEV)
    x[1, 1:] = float("nan")
    t = torch.from_numpy(table).to(DEV)
    batch = ops.ctc_beam_search(x, W, blank, frames=frames, lm_table=t, lm_weight=weight)
    got = device_beams(*batch)
    worst = 0.0
    for b, n in enumerate(frames):
        c = dict(name=f"lm-ragged-w{W}-x{weight}-u{b}", logits=lg[b:b + 1], lengths=[n], W=W, blank=blank, table=table,
                 lm_weight=weight)
        want, decided = C.expected(c)
        worst = max(worst, compare(got[b:b + 1], want, decided, c["name"]))
        alone = ops.ctc_beam_search(x[b:b + 1], W, blank, frames=[n], lm_table=t, lm_weight=weight)
        same_bits([y[b:b + 1] for y in batch], alone, f"utterance {b} alone")
    record_metric("beam_lm", case=f"lm-ragged-w{W}-x{weight}", max_dscore=worst)


def test_lm_commit_with_every_beam_live(ops):
    """W = 32 over V = 6, L = 30, a trained table at weight 0.3, B = 5 with counts [L, 1, 0, L - 1, 7]:
    the live set fills all 32 lanes within three frames and most winners of a frame are new nodes, so
    S(child) and the node numbers come from the lane-per-beam commit in nearly every lane.  The batch
    bitwise each utterance alone, and both the restatement."""
    V, L, W, blank, weight = 6, 30, 32, 0, 0.3
    lg, frames = C.ragged_case(V, L, blank, seed=V)
    table = C.trained_table(np.random.default_rng(61), V, blank).table
    x, t = torch.from_numpy(lg).to(DEV), torch.from_numpy(table).to(DEV)
    batch = ops.ctc_beam_search(x, W, blank, frames=frames, lm_table=t, lm_weight=weight)
    got = device_beams(*batch)
    assert len(got[0]) == W and len(got[3]) == W
    for b, n in enumerate(frames):
        c = dict(name=f"lm-commit-u{b}", logits=lg[b:b + 1], lengths=[n], W=W, blank=blank, table=table, lm_weight=weight)
        want, decided = C.expected(c)
        alone = ops.ctc_beam_search(x[b:b + 1], W, blank, frames=[n], lm_table=t, lm_weight=weight)
        same_bits([y[b:b + 1] for y in batch], alone, f"utterance {b} alone")
        compare(device_beams(*alone), want, decided, c["name"])
        compare(got[b:b + 1], want, decided, c["name"])


# ----------------------------------------------------------------------------- public interface
def test_public_search_runs_a_bigram_on_the_device(ops, monkeypatch):
    from velocity_asr import decode
    from velocity_asr.decode import BigramLM

    def refuse(*a, **k):
        raise AssertionError("the host search was called")

    monkeypatch.setattr(decode, "_ctc_beam_search_host", refuse)
    V, L, blank, W, weight = 40, 25, 39, 6, 1.0
    lg, frames = C.ragged_case(V, L, blank, seed=91, B=4)
    lm = C.trained_table(np.random.default_rng(92), V, blank)
    assert isinstance(lm, BigramLM)
    x = torch.from_numpy(lg).to(DEV)
    res = decode.ctc_beam_search(x, beam_width=W, blank_token=blank, lm_weight=weight, lm_scorer=lm,
                                 input_lengths=frames)
    for b, n in enumerate(frames):
        c = dict(name=f"api-u{b}", logits=lg[b:b + 1], lengths=[n], W=W, blank=blank, table=lm.table, lm_weight=weight)
        want, decided = C.expected(c)
        compare([[(r.tokens, r.score) for r in res[b]]], want, decided, c["name"])
    assert lm.device_table(x.device) is lm.device_table(x.device)  # copied up once
    dec = decode.CTCDecoder(decode.create_default_vocabulary(V), blank_token=blank)
    texts = dec.decode_beam_search(x, beam_width=W, input_lengths=frames, lm_scorer=lm, lm_weight=weight)
    assert texts == [dec._tokens_to_text(ub[0].tokens) for ub in res]
    # weight 0 switches the scorer off, as in the reference: the plain search
    off = decode.ctc_beam_search(x, beam_width=W, blank_token=blank, lm_weight=0.0, lm_scorer=lm)
    plain = decode.ctc_beam_search(x, beam_width=W, blank_token=blank)
    assert [[(r.tokens, r.score) for r in ub] for ub in off] == [[(r.tokens, r.score) for r in ub] for ub in plain]

    class Other:  # any other scorer still runs on the host
        def score(self, tokens):
            return 0.0

    with pytest.raises(AssertionError, match="host search"):
        decode.ctc_beam_search(x, beam_width=W, blank_token=blank, lm_weight=1.0, lm_scorer=Other())


def test_decode_batch_searches_a_padded_batch_in_one_launch(ops, default_weights, monkeypatch):
    """Two clips of unequal length, beam width 3: the padded batch gives the texts of the clips
    decoded alone, with one search call."""
    import velocity_asr as va
    from velocity_asr import synthetic as S
    from velocity_asr import transcription as T
    model = va.VELOCITYASR()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in default_weights.items()}, strict=True)
    model = model.to(DEV).eval()
    dec = va.CTCDecoder(va.create_default_vocabulary(model.config.vocab_size))
    audio = S.make_audio(2, 24000, seed=5)
    ns = [24000, 15000]
    padded = torch.from_numpy(audio).to(DEV)
    padded[1, ns[1]:] = 0.0
    calls = []
    real = ops.ctc_beam_search
    monkeypatch.setattr(ops, "ctc_beam_search", lambda *a, **k: calls.append(k.get("frames")) or real(*a, **k))
    both = T._decode_batch(model, padded, dec, False, beam_width=3, lengths=ns)
    assert len(calls) == 1 and list(calls[0]) == [model.get_output_length(n // T.HOP_LENGTH + 1) for n in ns]
    alone = [T._decode_batch(model, padded[b:b + 1, :n], dec, False, beam_width=3)[0] for b, n in enumerate(ns)]
    assert both == alone and all(w is None for _, w in both)


def test_evaluate_script_with_a_language_model(ops, default_weights, tmp_path, monkeypatch):
    """scripts/evaluate.py --beam-width 5 --lm lm.npz --lm-weight 0.5 on a directory of three clips of
    unequal length: one search launch for the batch, and the texts of the files transcribed one by one."""
    import importlib.util
    import os
    import velocity_asr as va
    from conftest import PKG_ROOT
    from velocity_asr import synthetic as S
    from velocity_asr import transcription as T
    from velocity_asr.audio import write_wav
    from velocity_asr.decode import BigramLM
    spec = importlib.util.spec_from_file_location("vasr_script_evaluate_lm", os.path.join(PKG_ROOT, "scripts", "evaluate.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    model = va.VELOCITYASR()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in default_weights.items()}, strict=True)
    model.save_pretrained(str(tmp_path / "model.pt"))
    clips = tmp_path / "clips"
    clips.mkdir()
    for i, n in enumerate((24000, 16333, 31000)):
        write_wav(str(clips / f"c{i}.wav"), S.make_audio(1, n, seed=60 + i)[0])
    rng = np.random.default_rng(61)
    V = model.config.vocab_size
    lm = BigramLM.from_token_sequences([rng.integers(1, V, size=20).tolist() for _ in range(200)], V)
    lm.save(tmp_path / "lm.npz")
    calls = []
    real = ops.ctc_beam_search
    monkeypatch.setattr(ops, "ctc_beam_search", lambda *a, **k: calls.append((a[0].shape[0], k.get("lm_table") is not None))
                        or real(*a, **k))
    out = tmp_path / "dir.tsv"
    assert ev.main(["--checkpoint", str(tmp_path / "model.pt"), "--audio-dir", str(clips), "--output", str(out),
                    "--beam-width", "5", "--lm", str(tmp_path / "lm.npz"), "--lm-weight", "0.5"]) == 0
    assert calls == [(3, True)]  # one launch, three utterances, the table on the device
    rows = dict(line.split("\t", 1) for line in out.read_text().splitlines())
    model = model.to(DEV).eval()
    dec = va.CTCDecoder(va.create_default_vocabulary(V))
    files = sorted(clips.iterdir())
    alone = T.transcribe_files(model, files, dec, DEV, False, 1, 5, lm=lm, lm_weight=0.5)
    assert rows == {p.name: r["transcription"] for p, r in zip(files, alone)}
