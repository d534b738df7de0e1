"""Times the shortlisted beam search against the dense one at the model's shape
(V 1000, L 501, width 10), tools/beam_time.py's method: device events around batches of calls after a
warm-up, the candidates alternating inside a round, median with min - max over the rounds.
  from logits      B 1, 8, 32 full length and the ragged B 8 of beam_time.py: `dense`
                   (ops.ctc_beam_search) against `shortlist` (ops.ctc_beam_shortlist + ops.ctc_beam_search_shortlist),
                   and the two launches of `shortlist` on their own;
  end to end       B 1, 8, 32 ten-second clips through the synthetic model: `logits_dense`
                   (decode.ctc_beam_search(model(mel))), the parent's path, against `beam_search`
                   (model.beam_search(mel)), results included; per round whether the new path was faster;
  fallback         B 8 from logits through the public entry, with and without one utterance of equal logits
                   (every candidate ties, so its certificate fails and the exact search runs on it);
  V 50 000         B 8 from logits (no dense column: the dense kernel stops at V 16384), a CTCOutputHead of that
                   vocabulary end to end in chunks, and the complete-mode exact search of one utterance, once;
  certified share  of frames and of utterances, on the random logits and on the synthetic model's.
    python tools/beam_shortlist_time.py [--out FILE.json] [--md FILE.md]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "velocity-asr_amd"))
import torch  # noqa: E402

import velocity_asr as va  # noqa: E402
from velocity_asr import decode, ops  # noqa: E402
from velocity_asr import synthetic as S  # noqa: E402

V, L, W, BLANK = 1000, 501, 10, 0
LENGTHS = [501, 463, 402, 377, 318, 251, 190, 126]  # tools/beam_time.py's ragged batch
BIG_V = 50000


def timed(fns, reps, inner):
    """Per fn the us per call of every round: `reps` rounds, the fns alternating within a round."""
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3 / inner)
    return out


def stats(v):
    return dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1))


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def bits(res):
    return [[(r.tokens, float(r.score).hex()) for r in ub] for ub in res]


def share(unc, frames):
    """Certified share of frames and of utterances from an uncertified-frame count per utterance."""
    unc = [int(u) for u in unc]
    return dict(frames=sum(frames), uncertified_frames=sum(unc), utterances=len(unc),
                uncertified_utterances=sum(u > 0 for u in unc),
                certified_frame_share=round(1 - sum(unc) / max(sum(frames), 1), 6),
                certified_utterance_share=round(1 - sum(u > 0 for u in unc) / max(len(unc), 1), 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--md")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    K = decode.beam_shortlist_size("auto", V, W)
    res = dict(V=V, L=L, W=W, K=K, lengths=LENGTHS, reps=a.reps, inner=a.inner, clock=ops.probe_clock(dev))
    gen = torch.Generator(device="cuda").manual_seed(501)
    x32 = torch.randn(32, L, V, device="cuda", generator=gen) * 3.0

    # ------------------------------------------------------------------ from ready logits
    res["from_logits"] = {}
    for name, B, frames in (("B1", 1, None), ("B8", 8, None), ("B32", 32, None), ("B8_ragged", 8, LENGTHS)):
        x = x32[:B]
        fr = None if frames is None else torch.tensor(frames, dtype=torch.int32, device="cuda")
        short = ops.ctc_beam_shortlist(x, K, BLANK, fr)
        t = timed({"dense": lambda: ops.ctc_beam_search(x, W, BLANK, frames=fr),
                   "shortlist": lambda: ops.ctc_beam_search_shortlist(*ops.ctc_beam_shortlist(x, K, BLANK, fr), V, W, BLANK, fr),
                   "shortlist_launch": lambda: ops.ctc_beam_shortlist(x, K, BLANK, fr),
                   "search_launch": lambda: ops.ctc_beam_search_shortlist(*short, V, W, BLANK, fr)}, a.reps, a.inner)
        got = ops.ctc_beam_search_shortlist(*short, V, W, BLANK, fr)
        # a guard against timing something else: where every utterance is certified, the dense search's bits
        assert got[4].any() or same(got[:4], ops.ctc_beam_search(x, W, BLANK, frames=fr))
        r = {k: stats(v) for k, v in t.items()}
        r["dense_over_shortlist"] = round(r["dense"]["median_us"] / r["shortlist"]["median_us"], 1)
        r["certified"] = share(got[4].cpu().tolist(), frames or [L] * B)
        res["from_logits"][name] = r

    # ------------------------------------------------------------------ end to end through the model
    model = va.VELOCITYASR()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in S.make_weights(None, seed=0).items()}, strict=True)
    model = model.to(dev).eval()
    res["end_to_end"] = {}
    for B in (1, 8, 32):
        mel = va.compute_mel_spectrogram(torch.from_numpy(S.make_audio(B, 160000, seed=40 + B)).to(dev))
        old = lambda: decode.ctc_beam_search(model(mel), beam_width=W, blank_token=BLANK)  # noqa: E731
        new = lambda: model.beam_search(mel, beam_width=W, blank=BLANK)  # noqa: E731
        assert bits(old()) == bits(new())
        t = timed({"logits_dense": old, "beam_search": new}, a.reps, a.inner)
        r = {k: stats(v) for k, v in t.items()}
        r["rounds_us"] = {k: [round(u, 1) for u in v] for k, v in t.items()}
        r["faster_in_every_round"] = all(n < o for n, o in zip(t["beam_search"], t["logits_dense"]))
        r["old_over_new"] = round(r["logits_dense"]["median_us"] / r["beam_search"]["median_us"], 1)
        logits = model(mel)
        unc = ops.ctc_beam_search_shortlist(*ops.ctc_beam_shortlist(logits, K, BLANK), V, W, BLANK)[4]
        r["certified"] = share(unc.cpu().tolist(), [logits.shape[1]] * B)
        r["tokens_in_best_beams"] = sum(len(ub[0].tokens) for ub in new())
        res["end_to_end"][f"B{B}"] = r
        del logits, mel

    # ------------------------------------------------------------------ the fallback where it fires
    x8 = x32[:8].clone()
    tied = x8.clone()
    tied[3] = 0.0  # equal logits in every frame: the strict certificate cannot hold
    calls = []
    real = decode._beam_search_exact
    decode._beam_search_exact = lambda lg, *b, **k: calls.append(lg.shape[0]) or real(lg, *b, **k)
    t = timed({"all_certified": lambda: decode.ctc_beam_search(x8, beam_width=W, blank_token=BLANK, shortlist="auto"),
               "one_uncertified": lambda: decode.ctc_beam_search(tied, beam_width=W, blank_token=BLANK, shortlist="auto"),
               "dense": lambda: decode.ctc_beam_search(tied, beam_width=W, blank_token=BLANK)}, a.reps, a.inner)
    decode._beam_search_exact = real
    exact_sizes = sorted(set(calls))  # [1]: only the tied batch, only its one utterance
    assert bits(decode.ctc_beam_search(tied, beam_width=W, blank_token=BLANK, shortlist="auto")) == \
        bits(decode.ctc_beam_search(tied, beam_width=W, blank_token=BLANK))
    res["fallback"] = {k: stats(v) for k, v in t.items()}
    res["fallback"]["utterances_per_exact_search"] = exact_sizes
    del x32, x8, tied

    # ------------------------------------------------------------------ V 50 000
    Kb = decode.beam_shortlist_size("auto", BIG_V, W)
    xb = torch.randn(8, L, BIG_V, device="cuda", generator=gen) * 3.0
    shortb = ops.ctc_beam_shortlist(xb, Kb, BLANK)
    t = timed({"shortlist": lambda: ops.ctc_beam_search_shortlist(*ops.ctc_beam_shortlist(xb, Kb, BLANK), BIG_V, W, BLANK),
               "shortlist_launch": lambda: ops.ctc_beam_shortlist(xb, Kb, BLANK),
               "search_launch": lambda: ops.ctc_beam_search_shortlist(*shortb, BIG_V, W, BLANK)}, a.reps, a.inner)
    big = {k: stats(v) for k, v in t.items()}
    gotb = ops.ctc_beam_search_shortlist(*shortb, BIG_V, W, BLANK)
    big["certified"] = share(gotb[4].cpu().tolist(), [L] * 8)
    # the exact search above the dense limit, one utterance, once; it must agree with the certified shortlist
    a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a0.record()
    exact = decode._beam_search_exact(xb[:1], W, BLANK, None)
    a1.record()
    torch.cuda.synchronize()
    big["complete_mode_one_utterance_ms"] = round(a0.elapsed_time(a1), 1)
    big["complete_mode_equals_shortlist"] = bool(int(gotb[4][0]) == 0 and same([y[:1] for y in gotb[:4]], exact))
    del xb, shortb, gotb
    head = va.CTCOutputHead(d_model=192, vocab_size=BIG_V).to(dev).eval()
    feats = torch.randn(8, L, 192, device="cuda", generator=gen)
    t = timed({"head_beam_search": lambda: head.beam_search(feats, W, BLANK)}, a.reps, 1)
    big["head_beam_search"] = stats(t["head_beam_search"])
    big["head_chunk_utterances"] = max(1, (256 << 20) // (L * BIG_V * 4))
    res["V50000"] = big

    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if a.md:
        cell = lambda d: f"{d['median_us'] / 1e3:.2f} ({d['min_us'] / 1e3:.2f} - {d['max_us'] / 1e3:.2f})"  # noqa: E731
        cert = lambda c: (f"{c['frames'] - c['uncertified_frames']} of {c['frames']} frames, "  # noqa: E731
                          f"{c['utterances'] - c['uncertified_utterances']} of {c['utterances']} utterances")
        rows = [f"V {V}, L {L}, width {W}, shortlist K {K} (\"auto\"); ms per call, median (min - max) of {a.reps} rounds of "
                f"{a.inner} calls; random logits N(0, 3^2).", "",
                "| from ready logits | dense | shortlist launch + search | shortlist launch | search launch | dense / shortlist | "
                "certified |", "|---|---|---|---|---|---|---|"]
        for n, r in res["from_logits"].items():
            rows.append(f"| {n} | {cell(r['dense'])} | {cell(r['shortlist'])} | {cell(r['shortlist_launch'])} | "
                        f"{cell(r['search_launch'])} | {r['dense_over_shortlist']} | {cert(r['certified'])} |")
        rows += ["", "| end to end, 10 s clips, synthetic model | model(mel) + dense | model.beam_search | old / new | "
                     "new faster in every round | certified |", "|---|---|---|---|---|---|"]
        for n, r in res["end_to_end"].items():
            rows.append(f"| {n} | {cell(r['logits_dense'])} | {cell(r['beam_search'])} | {r['old_over_new']} | "
                        f"{r['faster_in_every_round']} | {cert(r['certified'])} |")
        f = res["fallback"]
        rows += ["", "| public entry, B 8 from logits | ms |", "|---|---|",
                 f"| shortlist, every utterance certified | {cell(f['all_certified'])} |",
                 f"| shortlist, one utterance of equal logits searched again exactly | {cell(f['one_uncertified'])} |",
                 f"| shortlist=None on that batch | {cell(f['dense'])} |"]
        b = res["V50000"]
        rows += ["", f"| V {BIG_V}, B 8, L {L}, K {Kb} | ms |", "|---|---|",
                 f"| shortlist launch + search from logits | {cell(b['shortlist'])} |",
                 f"| shortlist launch | {cell(b['shortlist_launch'])} |", f"| search launch | {cell(b['search_launch'])} |",
                 f"| CTCOutputHead.beam_search from (8, {L}, 192) rows, chunks of {b['head_chunk_utterances']} utterances | "
                 f"{cell(b['head_beam_search'])} |",
                 f"| exact search of one utterance (complete mode), once | {b['complete_mode_one_utterance_ms']:.1f} |",
                 "", f"Certified at V {BIG_V}: {cert(b['certified'])}; the complete mode's beams equal the shortlist's bit for "
                     f"bit: {b['complete_mode_equals_shortlist']}."]
        with open(a.md, "w") as fh:
            fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
