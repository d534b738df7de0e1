#!/usr/bin/env python3
"""Evaluate VELOCITY-ASR on an MI355X: transcribe a directory, or score WER/CER on a test set.

Same command line and printed report as the reference's scripts/evaluate.py:

    python scripts/evaluate.py --checkpoint model.pt --audio-dir ./test_audio [--output out.tsv]
    python scripts/evaluate.py --checkpoint model.pt --test-set manifest.tsv

--test-set takes a TSV manifest (`audio_path<TAB>reference text`); the reference's
dataset loader is a stub that loads nothing. --beam-width > 1 selects prefix beam search, one
launch per batch; --lm FILE.npz --lm-weight X fuses a bigram table (decode.BigramLM.save) into it.
--search prefix runs the standard CTC prefix beam search instead of the reference's (alignments summed,
the LM term and --length-bonus once per token, --token-topk tokens per frame).
WER and CER are scored on --device (one batched edit-distance launch per unit); --error-breakdown adds the
substitution / deletion / insertion totals to the report, --per-utterance FILE writes them per file.
--alignments FILE writes each file's word alignment (which word for which), --confusions N appends the most
frequent word confusions to the report; the edit paths come from the device too (training.error_alignments).
"""

import argparse
import logging
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from velocity_asr import VELOCITYASR, CTCDecoder, create_default_vocabulary  # noqa: E402
from velocity_asr.decode import BigramLM  # noqa: E402
from velocity_asr.training import confusions, error_alignments, error_counts, error_rate, format_alignment  # noqa: E402
from velocity_asr.transcription import find_audio_files, load_manifest, transcribe_files  # noqa: E402

logging.basicConfig(level=logging.INFO, format="%(asctime)s | %(levelname)s | %(message)s",
                    datefmt="%Y-%m-%d %H:%M:%S")
logger = logging.getLogger("evaluate")

RULE = "=" * 60


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Evaluate VELOCITY-ASR v2 (MI355X)")
    p.add_argument("--checkpoint", required=True, help="Path to model checkpoint")
    p.add_argument("--test-set", default=None, help="Test-set manifest (TSV: audio path, reference)")
    p.add_argument("--audio-dir", default=None, help="Directory containing audio files to transcribe")
    p.add_argument("--output", default=None, help="Output file for results")
    p.add_argument("--device", default="cuda", help="HIP device to run evaluation on")
    p.add_argument("--beam-width", type=int, default=1, help="Beam width for decoding (1 = greedy)")
    p.add_argument("--batch-size", type=int, default=16, help="Max equal-length files per device batch")
    p.add_argument("--lm", default=None, help="Bigram language model for beam search (.npz of BigramLM.save)")
    p.add_argument("--lm-weight", type=float, default=0.0, help="Weight of the language model score (0 = off)")
    p.add_argument("--search", choices=("reference", "prefix"), default="reference",
                   help="Beam search: the reference's, or the standard prefix beam search (summed alignments, "
                        "per-token LM term and length bonus)")
    p.add_argument("--length-bonus", type=float, default=0.0, help="Per-token bonus of --search prefix")
    p.add_argument("--token-topk", default="auto",
                   help='Tokens kept per frame by --search prefix: "auto" (max(16, 2 * beam width)) or 1..64')
    p.add_argument("--segment-seconds", type=float, default=None,
                   help="Cut files longer than this at their quietest points and stitch the results (off by default)")
    p.add_argument("--min-segment-seconds", type=float, default=None,
                   help="Shortest segment of a cut file (a third of --segment-seconds by default)")
    p.add_argument("--error-breakdown", action="store_true",
                   help="With --test-set: append the word and character substitution/deletion/insertion totals")
    p.add_argument("--per-utterance", default=None, metavar="FILE",
                   help="With --test-set: write one TSV row per scored file (path, reference words, word S, D, I, WER)")
    p.add_argument("--alignments", default=None, metavar="FILE",
                   help="With --test-set: write every scored file's word alignment (path, counts, REF/HYP view)")
    p.add_argument("--confusions", type=int, default=0, metavar="N",
                   help="With --test-set: append the N most frequent word substitutions, deletions and insertions")
    args = p.parse_args(argv)
    if args.test_set is None and args.audio_dir is None:
        p.error("Either --test-set or --audio-dir must be specified")
    return args


def main(argv=None) -> int:
    args = parse_args(argv)
    logger.info(f"Loading model from {args.checkpoint}")
    model = VELOCITYASR.from_pretrained(args.checkpoint)
    model.to(args.device)
    model.eval()
    logger.info(f"Model loaded with {model.count_parameters():,} parameters")
    decoder = CTCDecoder(create_default_vocabulary(model.config.vocab_size))
    lm = None
    if args.lm:
        lm = BigramLM.load(args.lm)
        if lm.vocab_size != model.config.vocab_size:
            raise SystemExit(f"--lm: table for {lm.vocab_size} tokens, model has {model.config.vocab_size}")
        if args.beam_width <= 1 or args.lm_weight <= 0:
            logger.warning("--lm takes effect only with --beam-width > 1 and --lm-weight > 0")

    prefix = dict(search=args.search, length_bonus=args.length_bonus,
                  token_topk=args.token_topk if args.token_topk == "auto" else int(args.token_topk))
    if args.audio_dir:
        files = find_audio_files(args.audio_dir)
        rows = []
        for path, r in zip(files, transcribe_files(model, files, decoder, args.device, False,
                                                    args.batch_size, args.beam_width, lm=lm,
                                                    lm_weight=args.lm_weight, segment_seconds=args.segment_seconds,
                                                    min_segment_seconds=args.min_segment_seconds, **prefix)):
            if "error" in r:
                logger.error(f"Error processing {path}: {r['error']}")
                rows.append((path.name, f"[ERROR: {r['error']}]"))
            else:
                rows.append((path.name, r["transcription"]))
        print("\n" + RULE)
        print("TRANSCRIPTION RESULTS")
        print(RULE)
        for name, text in rows:
            print(f"\n{name}:")
            print(f"  {text}")
        if args.output:
            with open(args.output, "w") as f:
                for name, text in rows:
                    f.write(f"{name}\t{text}\n")
            logger.info(f"Results saved to {args.output}")
        return 0

    data = load_manifest(args.test_set)
    if not data:
        logger.error("No test data loaded. Exiting.")
        return 0
    preds, refs, paths = [], [], []
    results = transcribe_files(model, [a for a, _ in data], decoder, args.device, False,
                               args.batch_size, args.beam_width, lm=lm, lm_weight=args.lm_weight,
                               segment_seconds=args.segment_seconds, min_segment_seconds=args.min_segment_seconds, **prefix)
    for (audio, ref), r in zip(data, results):
        if "error" in r:
            logger.error(f"Error processing {audio}: {r['error']}")
            continue
        preds.append(r["transcription"])
        refs.append(ref)
        paths.append(audio)
    # scored on the device when it is a HIP device (the same integers as the host rule, divided once)
    score_device = args.device if torch.device(args.device).type == "cuda" else None
    words = error_counts(preds, refs, "word", score_device)
    chars = error_counts(preds, refs, "char", score_device)
    wer, cer = error_rate(words), error_rate(chars)
    report = [f"Test Set: {args.test_set}", f"Samples: {len(preds)}",
              f"WER: {wer * 100:.2f}%", f"CER: {cer * 100:.2f}%"]
    if args.error_breakdown:
        for name, cs in (("Word", words), ("Char", chars)):
            report.append(f"{name} S/D/I/N: {sum(c.substitutions for c in cs)}/{sum(c.deletions for c in cs)}/"
                          f"{sum(c.insertions for c in cs)}/{sum(c.ref_length for c in cs)}")
    if args.per_utterance:
        with open(args.per_utterance, "w", encoding="utf-8") as f:
            for path, c in zip(paths, words):
                f.write(f"{path}\t{c.ref_length}\t{c.substitutions}\t{c.deletions}\t{c.insertions}\t{c.rate:.6f}\n")
        logger.info(f"Per-utterance counts saved to {args.per_utterance}")
    if args.alignments or args.confusions > 0:
        aligned = error_alignments(preds, refs, "word", score_device)  # the edit paths, walked back on the device
        if args.confusions > 0:
            sub, dele, ins = confusions(aligned)
            for name, counter, show in (("substitutions", sub, lambda k: f"{k[0]} -> {k[1]}"),
                                        ("deletions", dele, str), ("insertions", ins, str)):
                report.append(f"Top word {name}:")
                # most frequent first, equal counts in the order of first appearance
                report += [f"  {n:6d}  {show(k)}" for k, n in counter.most_common(args.confusions)]
        if args.alignments:
            with open(args.alignments, "w", encoding="utf-8") as f:
                for path, al in zip(paths, aligned):
                    c = al.counts
                    f.write(f"{path}\tN={c.ref_length} S={c.substitutions} D={c.deletions} I={c.insertions}\n"
                            f"{format_alignment(al)}\n\n")
            logger.info(f"Alignments saved to {args.alignments}")
    print("\n" + RULE)
    print("EVALUATION RESULTS")
    print(RULE)
    print("\n".join(report))
    print(RULE)
    if args.output:
        with open(args.output, "w") as f:
            f.write("\n".join(report) + "\n")
        logger.info(f"Results saved to {args.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
