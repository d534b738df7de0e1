"""File-level transcription used by scripts/transcribe.py and scripts/evaluate.py.

The reference scripts run one file at a time: load -> mel on the host -> (1, F, 80) forward
-> greedy decode (reference scripts/transcribe.py:48-131, scripts/evaluate.py:60-107).
Here files are read on the host, sorted by length and cut into batches that go through the
device pipeline together (mel, forward, argmax, collapse all on the HIP device).  A batch of
clips of different lengths is zero-padded to its longest clip and carries each clip's own
length (pipeline.audio_to_token_ids(..., lengths=)): the mel statistics, pooling sizes,
attention keys and the collapse follow each clip's length and the SSM stacks are causal, so
the output for a file is the one the reference's per-file loop produces.  Where the front end
has no per-length kernels (VASR_STFT=gemm, n_mels > 85) batches hold clips of one length.
Files that are not at 16 kHz are downmixed and resampled on the device as well (grouped by rate
and channel count, audio.resample_on_device: the host resampler's values bit for bit) and their
16 kHz samples stay there; VASR_DEVICE_RESAMPLE=0 or an installed torchaudio keeps the host path.
With segment_seconds a recording longer than that is cut on the device at its quietest points
(audio.plan_segments), its segments join the batches as clips of their own and their tokens, spans
and log-probabilities are stitched back into one result (stitch_segments).
"""

from __future__ import annotations

import logging
import os
from pathlib import Path
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch

from . import _lib, ops
from .audio import (HOP_LENGTH, N_FFT, SAMPLE_RATE, SEGMENT_BLOCK, SEGMENT_WINDOW_BLOCKS, _FUSED_DOWNMIX_CHANNELS,
                    _to_host_rate, check_segment_params, device_resample_supported, load_audio, mel_on_device,
                    plan_segments, ragged_supported, read_audio, resample_on_device, segment_on_device)
from .decode import CTCDecoder, _scored_from_device, token_confidences

logger = logging.getLogger(__name__)

AUDIO_EXTENSIONS = {".wav", ".mp3", ".flac", ".ogg", ".m4a"}


def find_audio_files(directory: str) -> List[Path]:
    """Recursive listing with the reference's extension set (scripts/transcribe.py:233-238)."""
    return [p for p in Path(directory).rglob("*") if p.suffix.lower() in AUDIO_EXTENSIONS]


def frames_to_seconds(frame_idx: int, hop_length: int = HOP_LENGTH, sample_rate: int = SAMPLE_RATE) -> float:
    """Token frame -> seconds; tokens sit at stride 2 in mel frames (reference scripts/transcribe.py:42-45)."""
    return (frame_idx * 2 * hop_length) / sample_rate


def group_words(tokens: Sequence[int], spans: Sequence[Tuple[int, int]], vocabulary: Sequence[str],
                confidences: Optional[Sequence[float]] = None) -> List[Dict]:
    """Word segmentation of a timed token list (reference scripts/transcribe.py:83-117).

    A word is a run of non-separator characters (" " and "▁" separate). Its start is the
    first character's start frame; its end is the end frame of the separator that closes
    it, or of the utterance's last token for the final word — the reference's convention.
    confidences (extension): one value per token; each word then carries "confidence", the
    minimum over its own characters' tokens (separators do not count).
    """
    words: List[Dict] = []
    chars: List[str] = []
    confs: List[float] = []
    first: Optional[int] = None
    if confidences is not None and len(confidences) != len(tokens):
        raise ValueError(f"group_words: {len(confidences)} confidences for {len(tokens)} tokens")

    def flush(end_frame: int) -> None:
        text = "".join(chars).replace("▁", "")
        if text:
            word = {"word": text, "start": frames_to_seconds(first), "end": frames_to_seconds(end_frame)}
            if confidences is not None:
                word["confidence"] = min(confs)
            words.append(word)

    for k, (tok, (s, e)) in enumerate(zip(tokens, spans)):
        ch = vocabulary[tok] if 0 <= tok < len(vocabulary) else "<unk>"
        if ch in (" ", "▁"):
            if chars:
                flush(e)
                chars, confs, first = [], [], None
        else:
            if first is None:
                first = s
            chars.append(ch)
            if confidences is not None:
                confs.append(float(confidences[k]))
    if chars and spans:
        flush(spans[-1][1])
    return words


def _decode_batch(model, audio: torch.Tensor, decoder: CTCDecoder, timestamps: bool,
                  beam_width: int = 1, lengths: Optional[List[int]] = None, lm=None,
                  lm_weight: float = 0.0, confidence: bool = False, raw: bool = False, search: str = "reference",
                  length_bonus: float = 0.0, token_topk="auto") -> List:
    """(b, S) device audio -> [(text, words or None)] through the device pipeline.  lengths:
    per-clip sample counts when the clips were zero-padded to S.  lm / lm_weight: language model
    for the beam search (decode.BigramLM runs on the device).  VASR_BEAM_SHORTLIST=1 (read per call)
    sends a beam search without an active language model through model.beam_search: the same beams
    from per-frame shortlists, without the (B, L, V) logits.  confidence (greedy only):
    [(text, words with "confidence", path log-probability)] from model.greedy_scored.
    raw: per clip the integer arrays instead of text (a dict as stitch_segments takes and _render
    turns into the tuple above): what the segments of a long recording are stitched from.
    search = "prefix" (beam_width > 1): the standard prefix beam search through
    model.prefix_beam_search (summed alignments, lm_weight and length_bonus per token, token_topk
    pruning) instead of the reference's."""
    with torch.no_grad():
        mel = mel_on_device(audio, n_mels=model.config.mel_bins, lengths=lengths,
                            frame_pad=model.temporal_binding.conv_padding())
        frames = None if lengths is None else [n // HOP_LENGTH + 1 for n in lengths]
        if beam_width > 1 and search == "prefix":
            beams = model.prefix_beam_search(mel, frames=frames, beam_width=beam_width, blank=decoder.blank_token,
                                             token_topk=token_topk, lm=lm, lm_weight=lm_weight, length_bonus=length_bonus)
            if raw:
                return [{"tokens": list(r[0].tokens) if r else []} for r in beams]
            return [(t, None) for t in decoder._beam_texts(beams, False)]
        if 1 < beam_width <= 32 and not (lm is not None and lm_weight > 0) \
                and os.environ.get("VASR_BEAM_SHORTLIST", "0") == "1":
            # the same beams without the (B, L, V) logits: per-frame shortlists, then one search launch
            beams = model.beam_search(mel, frames=frames, beam_width=beam_width, blank=decoder.blank_token)
            if raw:
                return [{"tokens": list(r[0].tokens) if r else []} for r in beams]
            return [(t, None) for t in decoder._beam_texts(beams, False)]
        if beam_width > 1:
            logits = model(mel, frames=frames)
            # one search launch for the batch: each clip's workgroup stops at its own row count
            rows = None if frames is None else [model.get_output_length(f) for f in frames]
            if raw:  # each clip's best hypothesis
                beams = decoder.decode_beam_search(logits, beam_width=beam_width, return_all_beams=True,
                                                   input_lengths=rows, lm_scorer=lm, lm_weight=lm_weight)
                return [{"tokens": list(r[0].tokens) if r else []} for r in beams]
            return [(t, None) for t in decoder.decode_beam_search(logits, beam_width=beam_width, input_lengths=rows,
                                                                  lm_scorer=lm, lm_weight=lm_weight)]
        if confidence:
            # the head's GEMM leaves each frame's argmax and log-sum-exp (no logits in HBM either)
            if raw:
                res = model.greedy_scored(mel, frames=frames, blank=decoder.blank_token)
                toks, lens, st, en, lsum, lmin, path = (t.cpu().numpy() for t in res)
                return [{"tokens": toks[b, :n].tolist(), "start": st[b, :n].tolist(), "end": en[b, :n].tolist(),
                         "logp_sum": lsum[b, :n].tolist(), "logp_min": lmin[b, :n].tolist(),
                         "run_lengths": (en[b, :n] - st[b, :n]).tolist(), "path_logp": float(path[b])}
                        for b, n in enumerate(int(v) for v in lens)]
            scored = _scored_from_device(model.greedy_scored(mel, frames=frames, blank=decoder.blank_token), "mean")
            out = []
            for r in scored:
                words = group_words(r.tokens, r.timestamps, decoder.vocabulary, r.confidences)
                out.append((" ".join(w["word"] for w in words), words, r.score))
            return out
        # greedy: the CTC head's GEMM reduces each frame to its argmax (no logits in HBM)
        rows = None
        if frames is not None:
            rows = torch.tensor([model.get_output_length(f) for f in frames], dtype=torch.int32).to(audio.device)
        toks, lens, st, en = ops.ctc_collapse(model.token_ids(mel, frames=frames), decoder.blank_token, True,
                                              timestamps, frames=rows)
    toks, lens = toks.cpu().numpy(), lens.cpu().numpy()
    if timestamps:
        st, en = st.cpu().numpy(), en.cpu().numpy()
    if raw:
        out = []
        for b, n in enumerate(int(v) for v in lens):
            r = {"tokens": toks[b, :n].tolist()}
            if timestamps:
                r["start"], r["end"] = st[b, :n].tolist(), en[b, :n].tolist()
            out.append(r)
        return out
    out = []
    for b in range(toks.shape[0]):
        n = int(lens[b])
        ids = toks[b, :n].tolist()
        if timestamps:
            words = group_words(ids, list(zip(st[b, :n].tolist(), en[b, :n].tolist())), decoder.vocabulary)
            out.append((" ".join(w["word"] for w in words), words))
        else:
            out.append((decoder._tokens_to_text(ids), None))
    return out


def _render(r: Dict, decoder: CTCDecoder, timestamps: bool, confidence: bool) -> Tuple:
    """A raw decoding (_decode_batch(raw=True), or stitch_segments of several) -> the tuple
    _decode_batch returns for a clip: (text, words or None[, path log-probability])."""
    if "start" not in r or not timestamps:  # beam search, or greedy without time spans
        return (decoder._tokens_to_text(r["tokens"]), None)
    spans = [(int(s), int(e)) for s, e in zip(r["start"], r["end"])]
    if confidence:
        conf = token_confidences(r["logp_sum"], r["logp_min"], [e - s for s, e in spans], "mean")
        words = group_words(r["tokens"], spans, decoder.vocabulary, conf)
        return (" ".join(w["word"] for w in words), words, float(r["path_logp"]))
    words = group_words(r["tokens"], spans, decoder.vocabulary)
    return (" ".join(w["word"] for w in words), words)


_STITCH_LISTS = ("tokens", "start", "end", "logp_sum", "logp_min", "run_lengths")


def stitch_segments(segments: Sequence[Dict], starts: Sequence[int]) -> Dict:
    """Join the decodings of a recording's consecutive segments into one (pure host arithmetic).

    segments: one dict per segment, in order, with "tokens" and, where the decode produced them,
    "start" / "end" (token-row spans within the segment, as csrc/decode.hip writes them and
    group_words reads them: row t covers samples from 320 t), "logp_sum", "logp_min", "run_lengths"
    (one value per token) and "path_logp".  starts: each segment's first sample in the recording, a
    multiple of 320 (cuts are).  Returns one dict with the same keys: the lists concatenated in
    segment order, the spans shifted by start // 320 as integers (seconds are formed once, later,
    from the shifted rows) and path_logp the float64 sum of the segments' values in segment order.
    A segment without tokens contributes nothing but its path_logp.  Words are not formed here:
    group_words runs once over the joined stream, so a segment that begins inside a word continues
    it (word boundaries come from the separator tokens, not from the cuts)."""
    if len(segments) != len(starts) or not segments:
        raise ValueError(f"stitch_segments: {len(segments)} segments with {len(starts)} start samples")
    keys = [k for k in _STITCH_LISTS if k in segments[0]]
    out: Dict = {k: [] for k in keys}
    score = 0.0  # a Python float is a float64
    for seg, start in zip(segments, starts):
        start = int(start)
        if start < 0 or start % SEGMENT_BLOCK:
            raise ValueError(f"stitch_segments: segment start {start} is not a non-negative multiple of {SEGMENT_BLOCK}")
        n = len(seg["tokens"])
        shift = start // SEGMENT_BLOCK
        for k in keys:
            v = list(seg[k])
            if len(v) != n:
                raise ValueError(f"stitch_segments: {len(v)} values of {k!r} for {n} tokens")
            out[k] += [int(t) + shift for t in v] if k in ("start", "end") else v
        if "path_logp" in segments[0]:
            score = score + float(seg["path_logp"])
    if "path_logp" in segments[0]:
        out["path_logp"] = score
    return out


def _batches(items: List[Tuple[int, torch.Tensor]], batch_size: int, ragged: bool):
    """Consecutive batches of the length-sorted items: up to batch_size clips each, zero-padded
    to the longest when the front end takes per-clip lengths (ragged), else runs of clips of
    one sample count (the per-length kernels need the FFT front end with n_mels <= 85)."""
    k = 0
    while k < len(items):
        end = min(k + batch_size, len(items))
        if not ragged:
            n = items[k][1].numel()
            end = k + 1
            while end < len(items) and end - k < batch_size and items[end][1].numel() == n:
                end += 1
        yield items[k:end]
        k = end


def _device_resample_enabled() -> bool:
    """Files that are not at 16 kHz are resampled on the device when the library's own resampler
    is the one in use (torchaudio absent) and VASR_DEVICE_RESAMPLE is not "0" (read per call)."""
    if os.environ.get("VASR_DEVICE_RESAMPLE", "1") == "0":
        return False
    try:
        import torchaudio  # noqa: F401
        return False
    except ImportError:
        return True


def _resample_group(clips: List[torch.Tensor], sr: int, dev: torch.device) -> List[torch.Tensor]:
    """Host (C, n_i) clips of one rate and channel count -> their mono 16 kHz samples, one 1-D
    device tensor each: zero-padded to the longest, uploaded at their own rate, downmixed and
    resampled in one launch (resample_on_device).  More than _FUSED_DOWNMIX_CHANNELS channels are
    averaged by torch on the host first, as load_audio does."""
    if clips[0].size(0) > _FUSED_DOWNMIX_CHANNELS:
        clips = [w.mean(dim=0, keepdim=True) for w in clips]
    ns = [w.size(1) for w in clips]
    x = torch.zeros((len(clips), clips[0].size(0), max(ns)), dtype=torch.float32)
    for j, w in enumerate(clips):
        x[j, :, :ns[j]] = w
    y, outs = resample_on_device(x.to(dev), sr, SAMPLE_RATE, lengths=ns)
    return [y[j, :m] for j, m in enumerate(outs)]


def transcribe_files(model, paths: Iterable, decoder: CTCDecoder, device, timestamps: bool = False,
                     batch_size: int = 16, beam_width: int = 1, lm=None, lm_weight: float = 0.0,
                     confidence: bool = False, segment_seconds: Optional[float] = None,
                     min_segment_seconds: Optional[float] = None, search: str = "reference",
                     length_bonus: float = 0.0, token_topk="auto") -> List[Dict]:
    """Transcribe audio files; returns one result dict per file in input order.  lm / lm_weight:
    language model for beam_width > 1 (a decode.BigramLM is fused on the device).
    search (extension, beam_width > 1): "reference" is the reference's prefix beam search (best single
    alignment, the language model's score of the whole prefix added in every frame); "prefix" is the
    standard one (decode.ctc_prefix_beam_search: alignments summed, lm_weight * log p(tok | previous)
    and length_bonus once per token), run from per-frame shortlists of token_topk ("auto" or 1..64)
    tokens without the (B, L, V) logits.  length_bonus and token_topk belong to "prefix" alone.
    confidence (extension, greedy only; implies timestamps): each word also carries
    "confidence" in (0, 1], the minimum over its tokens of the geometric mean of the token's frame
    probabilities, and each result "score", the log-probability of the greedy path.

    A result is {"file", "duration", "transcription"} (+ "words" with timestamps), as the
    reference's transcribe_file returns; a file that fails gets {"file", "error"} instead,
    so callers can log it the way the reference's per-file try/except does.

    segment_seconds / min_segment_seconds (extension): None keeps a recording whole, and one over
    the model's positional table (about 100 s) fails.  With a value, every file longer than
    segment_seconds is cut on the device at its quietest points into segments of between
    min_segment_seconds (a third of segment_seconds when None) and segment_seconds
    (audio.plan_segments); the segments share the batches with the other files, each is decoded as
    a clip of its own (beam search: each alone, best hypotheses joined) and stitch_segments joins
    them, so "duration" is the recording's and words run across the cuts.  A file with a segment
    that fails gets {"file", "error"}.
    """
    if confidence and beam_width > 1:
        raise ValueError("transcribe_files: confidence is reported for greedy decoding (beam_width = 1)")
    if search not in ("reference", "prefix"):
        raise ValueError(f'transcribe_files: search must be "reference" or "prefix", got {search!r}')
    timestamps = timestamps or confidence
    seg_max = seg_min = None
    if segment_seconds is not None:
        seg_max = int(round(float(segment_seconds) * SAMPLE_RATE))
        seg_min = seg_max // 3 if min_segment_seconds is None else int(round(float(min_segment_seconds) * SAMPLE_RATE))
        pe = getattr(getattr(getattr(model, "temporal_binding", None), "pos_encoding", None), "pe_time", None)
        check_segment_params(seg_max, seg_min, SEGMENT_WINDOW_BLOCKS, max_rows=None if pe is None else pe.shape[0])
    elif min_segment_seconds is not None:
        raise ValueError("transcribe_files: min_segment_seconds needs segment_seconds")
    paths = [str(p) for p in paths]
    results: List[Optional[Dict]] = [None] * len(paths)
    items: List[Tuple[int, torch.Tensor]] = []
    dev = torch.device(device)
    on_device = _device_resample_enabled()
    native: Dict[Tuple[int, int], List[Tuple[int, torch.Tensor]]] = {}  # (rate, channels) -> clips to resample

    def check_length(n: int) -> None:
        if n < 2:
            raise ValueError(f"expected a mono clip of at least 2 samples, got shape {(n,)}")
        if n <= N_FFT // 2:  # the reference's reflect padding rejects it too
            raise RuntimeError(f"compute_mel_spectrogram: reflect padding of {N_FFT // 2} needs more than "
                               f"{N_FFT // 2} samples, got {n}")

    for i, p in enumerate(paths):
        try:
            if on_device:
                w, sr = read_audio(p)
                if sr != SAMPLE_RATE and device_resample_supported(sr, SAMPLE_RATE):
                    # the length the resampler will give decides, before anything is uploaded
                    check_length(int(_lib.lib().vasr_resample_length(w.size(1), sr, SAMPLE_RATE)))
                    native.setdefault((sr, w.size(0)), []).append((i, w))
                    continue
                a = _to_host_rate(w, sr)
            else:
                a = load_audio(p)
            if a.dim() != 1:
                raise ValueError(f"expected a mono clip of at least 2 samples, got shape {tuple(a.shape)}")
            check_length(a.numel())
            items.append((i, a))
        except Exception as e:  # reported per file, like the reference's loop
            results[i] = {"file": p, "error": str(e)}
    for (sr, _), clips in native.items():
        clips.sort(key=lambda it: it[1].size(1))
        for k in range(0, len(clips), max(1, batch_size)):
            chunk = clips[k:k + max(1, batch_size)]
            try:
                for (i, _), a in zip(chunk, _resample_group([w for _, w in chunk], sr, dev)):
                    items.append((i, a))
            except Exception as e:
                for i, _ in chunk:
                    results[i] = {"file": paths[i], "error": str(e)}
    # long recordings: planned and gathered where the audio is (or goes), keyed (file, k) from here on
    long_files: Dict[int, Tuple[int, List[int]]] = {}  # file -> (samples, start of each segment)
    seg_raw: Dict[Tuple[int, int], Dict] = {}
    seg_errors: Dict[int, str] = {}
    if seg_max is not None:
        whole, items = items, []
        for i, a in whole:
            n = a.numel()
            if n <= seg_max:
                items.append((i, a))
                continue
            try:
                rec = a.to(device=dev, dtype=torch.float32).unsqueeze(0)
                cuts = plan_segments(rec, [n], max_samples=seg_max, min_samples=seg_min)
                batch, seg_lengths, table = segment_on_device(rec, [n], cuts)
                long_files[i] = (n, [start for _, start, _ in table])
                items += [((i, k), batch[k, :m]) for k, m in enumerate(seg_lengths)]
            except Exception as e:
                results[i] = {"file": paths[i], "error": str(e)}
    items.sort(key=lambda it: it[1].numel())  # neighbours of similar length: little padding
    for chunk in _batches(items, max(1, batch_size), ragged_supported(model.config.mel_bins)):
        try:
            ns = [a.numel() for _, a in chunk]
            S = max(ns)
            # clips resampled on the device stay there: the batch is then assembled on it
            where = dev if any(a.device.type == "cuda" for _, a in chunk) else None
            audio = torch.zeros((len(chunk), S), dtype=torch.float32, device=where)
            for j, (_, a) in enumerate(chunk):
                audio[j, :ns[j]] = a.to(torch.float32)
            segmented = any(isinstance(key, tuple) for key, _ in chunk)
            decoded = _decode_batch(model, audio.to(dev), decoder, timestamps, beam_width,
                                    lengths=None if min(ns) == S else ns, lm=lm, lm_weight=lm_weight,
                                    confidence=confidence, raw=segmented, search=search, length_bonus=length_bonus,
                                    token_topk=token_topk)
            for (i, _), n, dec in zip(chunk, ns, decoded):
                if isinstance(i, tuple):  # a segment: kept raw until its file is whole
                    seg_raw[i] = dec
                    continue
                if segmented:
                    dec = _render(dec, decoder, timestamps, confidence)
                r = {"file": paths[i], "duration": n / SAMPLE_RATE, "transcription": dec[0]}
                if timestamps:
                    r["words"] = dec[1]
                if confidence:
                    r["score"] = dec[2]
                results[i] = r
        except Exception as e:
            for i, _ in chunk:
                if isinstance(i, tuple):
                    seg_errors.setdefault(i[0], str(e))
                else:
                    results[i] = {"file": paths[i], "error": str(e)}
    for i, (n, starts) in long_files.items():
        if i in seg_errors:
            results[i] = {"file": paths[i], "error": seg_errors[i]}
            continue
        dec = _render(stitch_segments([seg_raw[(i, k)] for k in range(len(starts))], starts), decoder, timestamps,
                      confidence)
        r = {"file": paths[i], "duration": n / SAMPLE_RATE, "transcription": dec[0]}
        if timestamps:
            r["words"] = dec[1]
        if confidence:
            r["score"] = dec[2]
        results[i] = r
    return results  # type: ignore[return-value]


def load_manifest(path: str) -> List[Tuple[str, str]]:
    """Test-set manifest: one `audio_path<TAB>reference text` per line (relative paths are
    resolved against the manifest's directory). The reference's load_test_data is a stub
    that returns [] (scripts/evaluate.py:41-57); a manifest file is the local equivalent."""
    p = Path(path)
    if not p.is_file():
        logger.warning(f"Dataset loading not implemented for '{path}'. Pass a TSV manifest file.")
        return []
    out = []
    for line in p.read_text(encoding="utf-8").splitlines():
        if not line.strip():
            continue
        audio, _, ref = line.partition("\t")
        a = Path(audio)
        out.append((str(a if a.is_absolute() else p.parent / a), ref))
    return out
