#!/usr/bin/env python
"""Generate tests/golden/score.json: the reference's own compute_wer / compute_cer values.

Build-machine tool, like gen_goldens.py: run it on the CPU with the REFERENCE package first on the
path,

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/gen_score_goldens.py

It calls the reference's velocity_asr.training.compute_wer and compute_cer (training.py:412-501) on
the string pairs of tests/score_cases.py (GOLDEN_PAIRS): each pair alone, and all of them as one
corpus.  Stored: the strings and the recorded floats, nothing else.  This file is this repository's
own code; only main() imports the reference, and asserts that it did.
"""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "score.json")
sys.path.insert(0, os.path.dirname(HERE))
import score_cases as C  # noqa: E402


def main():
    from velocity_asr import training as T
    assert "velocity-asr_amd" not in os.path.abspath(T.__file__), f"not the reference: {T.__file__}"
    pairs = [dict(prediction=p, reference=r, wer=T.compute_wer([p], [r]), cer=T.compute_cer([p], [r]))
             for p, r in C.GOLDEN_PAIRS]
    preds, refs = [p for p, _ in C.GOLDEN_PAIRS], [r for _, r in C.GOLDEN_PAIRS]
    doc = dict(source="reference velocity_asr.training.compute_wer / compute_cer", pairs=pairs,
               corpus=dict(wer=T.compute_wer(preds, refs), cer=T.compute_cer(preds, refs)))
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump(doc, f, ensure_ascii=False, indent=1)
        f.write("\n")
    print(f"wrote {OUT}: {len(pairs)} pairs")


if __name__ == "__main__":
    main()
