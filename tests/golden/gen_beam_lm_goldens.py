#!/usr/bin/env python
"""Generate tests/golden/beam_lm.json: the reference's ctc_beam_search with a language model.

Build-machine tool, like gen_goldens.py: run it on the CPU with the REFERENCE package first on
the path,

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/gen_beam_lm_goldens.py

It calls the reference's velocity_asr.decode.ctc_beam_search (decode.py:128-217) with lm_scorer
set to TableScorer below -- a bigram table scored left to right in Python floats, the contract of
velocity_asr.decode.BigramLM.score in this repository -- on the cases of tests/beam_lm_cases.py
(GOLD: V <= 12, L <= 20, blank 0 and not) at widths 1, 3, 10 and lm_weight 0.5, 2.0.  The reference
has no lengths argument, so the same cases cut to `lengths` are recorded by slicing:
ctc_beam_search(logits[b:b+1, :lengths[b]]).

Stored per case: the logits, the table and the reference's own F.log_softmax(logits) as base64
float32 (torch's and numpy's log-softmax differ in the last ulp, and the host test pins the
restatement to 1e-12, so it searches the reference's log-probabilities), and the beams.

TableScorer and the helpers are this repository's own code and import nothing of the reference;
the tests import them.  Only main() imports the reference, and asserts that it did.
"""

import base64
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "beam_lm.json")
sys.path.insert(0, os.path.dirname(HERE))
import beam_lm_cases as C  # noqa: E402


class TableScorer:
    """lm_scorer over a (V + 1, V) bigram table: row 0 after the sentence start, row 1 + p after
    token p; score(tokens) is the left-to-right Python-float sum, 0.0 for []."""

    def __init__(self, table):
        self.table = np.asarray(table, np.float32)

    def score(self, tokens):
        s, row = 0.0, 0
        for tok in tokens:
            s += float(self.table[row, tok])
            row = 1 + tok
        return s


def pack(a):
    return base64.b64encode(np.ascontiguousarray(a, np.float32).tobytes()).decode("ascii")


def unpack(text, shape):
    return np.frombuffer(base64.b64decode(text), np.float32).reshape(shape)


def key(width, weight):
    return f"w{width}_x{weight}"


def main():
    import torch
    import velocity_asr as ref
    from velocity_asr import decode as ref_decode
    here = os.path.realpath(os.path.dirname(os.path.dirname(HERE)))
    assert not os.path.realpath(ref.__file__).startswith(here), f"not the reference: {ref.__file__}"

    def beams(lg, blank, width, scorer, weight):
        res = ref_decode.ctc_beam_search(torch.from_numpy(np.ascontiguousarray(lg)), beam_width=width,
                                         blank_token=blank, lm_weight=weight, lm_scorer=scorer)
        return [[[list(map(int, d.tokens)), float(d.score)] for d in ub] for ub in res]

    out = {"meta": {"reference": "velocity_asr.decode.ctc_beam_search, lm_scorer=TableScorer(table)",
                    "torch": torch.__version__, "numpy": np.__version__}, "cases": {}}
    for name, c in C.GOLD.items():
        lg, table = C.gold_inputs(name)
        scorer = TableScorer(table)
        lp = torch.nn.functional.log_softmax(torch.from_numpy(lg), dim=-1).numpy()
        full, cut = {}, {}
        for width in C.GOLD_WIDTHS:
            for weight in C.GOLD_WEIGHTS:
                full[key(width, weight)] = beams(lg, c["blank"], width, scorer, weight)
                cut[key(width, weight)] = [beams(lg[b:b + 1, :n], c["blank"], width, scorer, weight)[0]
                                           for b, n in enumerate(c["lengths"])]
        out["cases"][name] = {"shape": list(lg.shape), "logits": pack(lg), "table": pack(table),
                              "log_probs": pack(lp), "full": full, "cut": cut}
    with open(OUT, "w") as f:
        json.dump(out, f)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
