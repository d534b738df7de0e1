"""Times the greedy decode with confidences on the CTC head, three forms alternating inside one process
(device events around batches of calls, after a warm-up of every shape; a window holds as many calls
as fill about 20 ms, so the events time the device, not the enqueue):
  plain      ops.gemm_ctc_greedy: the ARGMAX GEMM + vasr_ctc_collapse_keys (tokens only, no confidences)
  scored     ops.gemm_ctc_greedy_conf: the ARGMAX_LSE GEMM + vasr_ctc_collapse_keys_conf
  composed   the same result from launches that existed before: the ARGMAX GEMM, the LSE GEMM,
             vasr_lse_combine_f32, vasr_argmax_keys, the winning logit read back out of the keys (torch
             elementwise), then vasr_ctc_collapse_conf from pred / logp
and each GEMM alone.  scored - plain is the cost of confidences; the fused epilogue is kept only where
scored is not slower than composed.  Shapes are M:V rows x vocabulary at K = 192, M = B * 501 rows.
    python tools/greedy_conf_time.py [--shapes M:V,...] [--out profiles/greedy_conf]
writes <out>.json and <out>.md."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "velocity-asr_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from velocity_asr import _lib as L, ops  # noqa: E402

K, LQ = 192, 501
WINDOW_US = 20e3


def timed(fns, reps):
    """us per call of each fn: `reps` event-timed windows, the fns alternating; a window is as many
    calls as fill WINDOW_US by a first estimate (at least 3), the same number for every fn."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for fn in fns.values():
        for _ in range(5):
            fn()
    b.record()
    torch.cuda.synchronize()
    inner = max(3, min(1000, int(WINDOW_US / (a.elapsed_time(b) * 1e3 / (5 * len(fns))))))
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
    return {k: dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1),
                    windows=reps, calls_per_window=inner) for k, v in out.items()}


def key_floats(keys, pred):
    """The float each row's winning key carries (what vasr_ctc_collapse_keys_conf decodes in its launch)."""
    # the row's largest key as unsigned (a wave's key sits in the first slot of its columns, not
    # always the winning column's own): flip the sign bit, take the signed maximum, flip it back
    k = (keys ^ -2 ** 63).max(1).values ^ -2 ** 63
    assert torch.equal((0xFFFFFFFF - (k & 0xFFFFFFFF)).to(torch.int32), pred)
    o = (k >> 32) & 0xFFFFFFFF
    u = torch.where((o & 0x80000000) != 0, o & 0x7FFFFFFF, ~o & 0xFFFFFFFF)
    return torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32).view(torch.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16032:1000,16032:5000")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "greedy_conf"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = dict(clock_before=ops.probe_clock(dev), K=K, utterance_rows=LQ, shapes=[])
    for spec in a.shapes.split(","):
        M, V = (int(v) for v in spec.split(":"))
        B = M // LQ
        assert B * LQ == M, f"M={M} is not a whole number of {LQ}-row utterances"
        g = torch.Generator(device="cuda").manual_seed(M + V)
        x2 = F.layer_norm(torch.randn(M, K, device="cuda", generator=g), (K,))
        W = 0.3 * torch.randn(V, K, device="cuda", generator=g)
        b = 0.5 * torch.randn(V, device="cuda", generator=g)
        G = (V + 31) // 32
        dims, wdims = (M, K, K), (V, K)

        def plain():
            return ops.gemm_ctc_greedy(x2, W, b, B, timestamps=True)

        def scored():
            return ops.gemm_ctc_greedy_conf(x2, W, b, B)

        def composed():
            keys, _, _ = ops._gemm_argmax_keys(x2, W, b, None, None, "composed")
            pairs, _ = ops._gemm_lse_pairs(x2, W, b, dims, wdims)
            stats = ops.lse_combine(pairs, G)
            pred = torch.empty(M, device=dev, dtype=torch.int32)
            L.check(L.lib().vasr_argmax_keys(keys.data_ptr(), G, G, M, pred.data_ptr(), L.stream_of(keys)), "vasr_argmax_keys")
            logp = (key_floats(keys, pred) - stats[:, 0]) - stats[:, 1]
            return ops.ctc_collapse_conf(pred.view(B, LQ), logp.view(B, LQ))

        def gemm_argmax():
            return ops._gemm_argmax_keys(x2, W, b, None, None, "piece")[0]

        def gemm_lse():
            return ops._gemm_lse_pairs(x2, W, b, dims, wdims)[0]

        def gemm_argmax_lse():
            return ops.gemm_argmax_lse(x2, W, b)

        s, c, p = scored(), composed(), plain()
        lens = s[1].tolist()
        # the composed form's LSE GEMM may run on another engine (its pairs then differ in the last bits)
        same = torch.equal(s[1], c[1]) and all(torch.equal(s[k][i, :n], c[k][i, :n]) for k in (0, 2, 3)
                                               for i, n in enumerate(lens))
        diff = max(float((s[4][i, :n] - c[4][i, :n]).abs().max()) for i, n in enumerate(lens) if n)
        same_tokens = torch.equal(s[1], p[1]) and all(torch.equal(s[0][i, :n], p[0][i, :n]) for i, n in enumerate(lens))
        t = timed(dict(plain=plain, scored=scored, composed=composed), a.reps)
        t.update(timed(dict(gemm_argmax=gemm_argmax, gemm_lse=gemm_lse, gemm_argmax_lse=gemm_argmax_lse), a.reps))
        rec = dict(M=M, V=V, B=B, logits_bytes=M * V * 4, slot_bytes=M * 2 * G * 8,
                   kernel_argmax_lse=ops.gemm_tile(M, V, K, epilogue=L.EPI_ARGMAX_LSE),
                   kernel_argmax=ops.gemm_tile(M, V, K, epilogue=L.EPI_ARGMAX),
                   kernel_lse=ops.gemm_tile(M, V, K, epilogue=L.EPI_LSE),
                   scored_tokens_spans_equal_composed=bool(same), max_abs_logp_sum_diff_to_composed=diff,
                   scored_tokens_equal_plain=bool(same_tokens), times=t,
                   cost_of_confidences_us=round(t["scored"]["median_us"] - t["plain"]["median_us"], 1),
                   fused_not_slower_than_composed=t["scored"]["median_us"] <= t["composed"]["median_us"])
        res["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
        del x2, W, b
        torch.cuda.empty_cache()
    res["clock_after"] = ops.probe_clock(dev)
    res["fused_epilogue_kept"] = all(r["fused_not_slower_than_composed"] for r in res["shapes"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    with open(a.out + ".md", "w") as f:
        f.write("# Greedy decode with confidences: the fused epilogue against plain greedy and the composed form\n\n"
                f"tools/greedy_conf_time.py, K = {K}, utterances of {LQ} rows, medians of {a.reps} event-timed windows, the three\n"
                "forms alternating in one process.  Clock: see the JSON's clock_before / clock_after (ops.probe_clock).\n\n"
                "plain = ops.gemm_ctc_greedy with time spans (the ARGMAX GEMM + one collapse launch, no confidences); scored =\n"
                "ops.gemm_ctc_greedy_conf (the ARGMAX_LSE GEMM + one launch); composed = the same values from the ARGMAX GEMM,\n"
                "the LSE GEMM, vasr_lse_combine_f32, vasr_argmax_keys, the key's float in torch, vasr_ctc_collapse_conf.\n"
                "Kernel: what ops.gemm_tile names for the ARGMAX_LSE / ARGMAX / LSE GEMM (1 = the rows engine).\n\n"
                "| M | V | kernel | plain us | scored us | composed us | scored - plain us | ARGMAX GEMM us | LSE GEMM us | "
                "ARGMAX_LSE GEMM us | tokens, spans equal | max abs logp_sum diff to composed |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in res["shapes"]:
            t = r["times"]
            f.write(f"| {r['M']} | {r['V']} | {r['kernel_argmax_lse']} / {r['kernel_argmax']} / {r['kernel_lse']} | "
                    f"{t['plain']['median_us']} | {t['scored']['median_us']} | {t['composed']['median_us']} | "
                    f"{r['cost_of_confidences_us']} | {t['gemm_argmax']['median_us']} | {t['gemm_lse']['median_us']} | "
                    f"{t['gemm_argmax_lse']['median_us']} | {r['scored_tokens_spans_equal_composed'] and r['scored_tokens_equal_plain']} | "
                    f"{r['max_abs_logp_sum_diff_to_composed']:.2e} |\n")
        kept = res["fused_epilogue_kept"]
        f.write("\nShipped form: " + ("the fused epilogue (scored is not slower than composed at every shape).\n" if kept else
                                      "NOT decided for the fused epilogue: scored is slower than composed at a shape above.\n"))


if __name__ == "__main__":
    main()
