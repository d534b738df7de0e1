"""Times the standard CTC prefix beam search (csrc/beam_prefix.hip) at the model's shape
(V 1000, L 501, width 10), B = 1 and 8, beside the reference-semantics dense entry with a table, the yardstick:
  ref_lm           ops.ctc_beam_search with a bigram table (vasr_ctc_beam_search_lm);
  prefix_lm        ops.ctc_prefix_beam_search with the same table, alpha 0.5, beta 0.5;
  prefix_no_lm     the same without a table;
  pruned           ops.ctc_beam_shortlist + ops.ctc_prefix_beam_search_shortlist from the logits, K = "auto", with
                   the table; pruned_search is its second launch alone;
  end to end       model.prefix_beam_search(mel) with the table beside decode.ctc_prefix_beam_search(model(mel));
  short prefixes   ref_lm and prefix_lm at B = 1 with the blank's logit raised by 12: the beams stay a few tokens long,
                   so the trie's node lookup of the prefix search scans old nodes in every frame;
  V 50 000         the pruned entry from (8, L, 50 000) logits, and a 50 000-token head from its input.
Device events around batches of calls, after a warm-up; the candidates alternate inside a round; median with
min - max over the rounds.  The bar: prefix_lm at most 1.10 x ref_lm in the same session.
    python tools/beam_prefix_time.py [--out FILE.json] [--md FILE.md]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "velocity-asr_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import velocity_asr as va  # noqa: E402
from beam_time import timed  # noqa: E402
from velocity_asr import decode, ops  # noqa: E402
from velocity_asr import synthetic as S  # noqa: E402

V, L, W, BLANK, BIG_V = 1000, 501, 10, 0, 50000
ALPHA, BETA = 0.5, 0.5
BAR = 1.10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--md")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    K = decode.beam_shortlist_size("auto", V, W)
    res = dict(V=V, L=L, W=W, K=K, alpha=ALPHA, beta=BETA, reps=a.reps, inner=a.inner, clock=ops.probe_clock(dev))
    gen = torch.Generator(device="cuda").manual_seed(501)
    x8 = torch.randn(8, L, V, device="cuda", generator=gen) * 3.0
    rng = np.random.default_rng(7)
    lm = decode.BigramLM.from_token_sequences([rng.integers(1, V, size=int(rng.integers(5, 60))).tolist()
                                               for _ in range(2000)], V, blank=BLANK)
    table = lm.device_table(dev)
    kw = dict(lm_table=table, alpha=ALPHA, beta=BETA)

    res["from_logits"] = {}
    for B in (1, 8):
        x = x8[:B]
        short = ops.ctc_beam_shortlist(x, K, BLANK)
        t = timed({"ref_lm": lambda: ops.ctc_beam_search(x, W, BLANK, lm_table=table, lm_weight=ALPHA),
                   "prefix_lm": lambda: ops.ctc_prefix_beam_search(x, W, BLANK, **kw),
                   "prefix_no_lm": lambda: ops.ctc_prefix_beam_search(x, W, BLANK, beta=BETA),
                   "pruned": lambda: ops.ctc_prefix_beam_search_shortlist(*ops.ctc_beam_shortlist(x, K, BLANK), V, W, BLANK, **kw),
                   "pruned_search": lambda: ops.ctc_prefix_beam_search_shortlist(*short, V, W, BLANK, **kw)},
                  a.reps, a.inner)
        full, pruned = ops.ctc_prefix_beam_search(x, W, BLANK, **kw), ops.ctc_prefix_beam_search_shortlist(*short, V, W, BLANK, **kw)
        t["prefix_lm_over_ref_lm"] = round(t["prefix_lm"]["median_us"] / t["ref_lm"]["median_us"], 3)
        t["within_bar"] = t["prefix_lm_over_ref_lm"] <= BAR
        t["pruned_below_dense"] = t["pruned"]["median_us"] < t["prefix_lm"]["median_us"]
        t["best_prefix_tokens"] = dict(prefix=full[1][:, 0].cpu().tolist(), pruned=pruned[1][:, 0].cpu().tolist(),
                                       reference=ops.ctc_beam_search(x, W, BLANK, lm_table=table, lm_weight=ALPHA)[1][:, 0].cpu().tolist())
        t["pruned_best_equals_full"] = [bool(torch.equal(full[0][b, 0], pruned[0][b, 0])) for b in range(B)]
        res["from_logits"][f"B{B}"] = t

    # short prefixes live late: a dominant blank keeps the beams a few tokens long over all 501 frames, so nearly every
    # new extension has an old node as its parent and prefix_commit's node lookup scans most of the trie
    xs = x8[:1].clone()
    xs[..., BLANK] += 12.0
    t = timed({"ref_lm": lambda: ops.ctc_beam_search(xs, W, BLANK, lm_table=table, lm_weight=ALPHA),
               "prefix_lm": lambda: ops.ctc_prefix_beam_search(xs, W, BLANK, **kw)}, a.reps, a.inner)
    t["prefix_lm_over_ref_lm"] = round(t["prefix_lm"]["median_us"] / t["ref_lm"]["median_us"], 3)
    t["within_bar"] = t["prefix_lm_over_ref_lm"] <= BAR
    t["best_prefix_tokens"] = ops.ctc_prefix_beam_search(xs, W, BLANK, **kw)[1][:, 0].cpu().tolist()
    res["short_prefixes_B1"] = t
    del xs

    model = va.VELOCITYASR()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in S.make_weights(None, seed=0).items()}, strict=True)
    model = model.to(dev).eval()
    vocab = model.config.vocab_size
    mlm = lm if vocab == V else None
    res["end_to_end"] = dict(vocab=vocab, with_table=mlm is not None)
    for B in (1, 8):
        mel = va.compute_mel_spectrogram(torch.from_numpy(S.make_audio(B, 160000, seed=40 + B)).to(dev))
        args = dict(lm_weight=ALPHA if mlm is not None else 0.0, length_bonus=BETA)
        res["end_to_end"][f"B{B}"] = timed(
            {"prefix_beam_search": lambda: model.prefix_beam_search(mel, beam_width=W, lm=mlm, **args),
             "logits_pruned": lambda: decode.ctc_prefix_beam_search(model(mel), W, BLANK, mlm, token_topk="auto", **args),
             "beam_search": lambda: model.beam_search(mel, beam_width=W)}, a.reps, a.inner)
        del mel
    del x8

    Kb = decode.beam_shortlist_size("auto", BIG_V, W)
    xb = torch.randn(8, L, BIG_V, device="cuda", generator=gen) * 3.0
    shortb = ops.ctc_beam_shortlist(xb, Kb, BLANK)
    big = timed({"pruned": lambda: ops.ctc_prefix_beam_search_shortlist(*ops.ctc_beam_shortlist(xb, Kb, BLANK), BIG_V, W, BLANK, beta=BETA),
                 "pruned_search": lambda: ops.ctc_prefix_beam_search_shortlist(*shortb, BIG_V, W, BLANK, beta=BETA)}, a.reps, a.inner)
    del xb, shortb
    head = va.CTCOutputHead(d_model=192, vocab_size=BIG_V).to(dev).eval()
    feats = torch.randn(8, L, 192, device="cuda", generator=gen)
    big.update(timed({"head_prefix_beam_search": lambda: head.prefix_beam_search(feats, W, BLANK, length_bonus=BETA)}, a.reps, a.inner))
    res["V50000"] = dict(B=8, K=Kb, **big)

    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if a.md:
        cell = lambda d: f"{d['median_us'] / 1e3:.2f} ({d['min_us'] / 1e3:.2f} - {d['max_us'] / 1e3:.2f})"  # noqa: E731
        rows = [f"V {V}, L {L}, width {W}, K {K}, alpha {ALPHA}, beta {BETA}; ms per call, median (min - max) of {a.reps} "
                f"rounds of {a.inner} calls.", "",
                "| from logits | reference search, table | prefix, table | prefix, no table | pruned (2 launches) | "
                "pruned search alone | prefix / reference | within 1.10 |", "|---|---|---|---|---|---|---|---|"]
        for B, t in res["from_logits"].items():
            rows.append(f"| {B} | {cell(t['ref_lm'])} | {cell(t['prefix_lm'])} | {cell(t['prefix_no_lm'])} | {cell(t['pruned'])} | "
                        f"{cell(t['pruned_search'])} | {t['prefix_lm_over_ref_lm']} | {'yes' if t['within_bar'] else 'NO'} |")
        t = res["short_prefixes_B1"]
        rows += ["", f"Blank logit + 12 (best prefix {t['best_prefix_tokens'][0]} tokens after {L} frames, the node lookup scanning old "
                     f"nodes), B 1: reference search, table {cell(t['ref_lm'])}, prefix, table {cell(t['prefix_lm'])}, ratio "
                     f"{t['prefix_lm_over_ref_lm']} ({'within' if t['within_bar'] else 'ABOVE'} 1.10)."]
        rows += ["", f"| end to end (vocabulary {vocab}) | model.prefix_beam_search | model(mel) + pruned entry | model.beam_search |",
                 "|---|---|---|---|"]
        for B in ("B1", "B8"):
            t = res["end_to_end"][B]
            rows.append(f"| {B} | {cell(t['prefix_beam_search'])} | {cell(t['logits_pruned'])} | {cell(t['beam_search'])} |")
        b = res["V50000"]
        rows += ["", f"V 50 000, B 8, K {Kb}: pruned entry from logits {cell(b['pruned'])}, its search launch "
                     f"{cell(b['pruned_search'])}, a 50 000-token head from its input {cell(b['head_prefix_beam_search'])}."]
        with open(a.md, "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
