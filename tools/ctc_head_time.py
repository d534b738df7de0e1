"""Times the logit-free CTC loss on the head against the path through the logits, alternating the
two inside one process (device events around batches of calls, after a warm-up of every shape;
a window holds as many calls as fill about 20 ms, so the events time the device, not the enqueue):
  forward    ops.ctc_head_emissions            vs  ops.gemm + ops.ctc_emissions
  pieces     ops.gemm_lse, ops.gemm and ops.ctc_emissions of ready logits, each alone
  step       CTCHeadLoss(differentiable, fused) forward + backward
                                               vs  device F.linear + CTCLoss(differentiable=True)
and the peak device memory of one call of each above the level before it.  Shapes are
M:V:S rows x vocabulary x target length at K = 192, M = B * 501 rows of 501-token utterances.
    python tools/ctc_head_time.py [--shapes M:V:S,...] [--out profiles/ctc_head]
writes <out>.json and <out>.md; the default shapes are the ones profiles/ctc_head.* holds."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "velocity-asr_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from velocity_asr import _lib as L, ops  # noqa: E402
from velocity_asr.model import CTCOutputHead  # noqa: E402
from velocity_asr.training import CTCHeadLoss, CTCLoss  # noqa: E402

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


def peak_over(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16032:1000:120,16032:2000:120,16032:3000:120,16032:4000:120,16032:5000:120,16032:10000:120,"
                                        "4008:50000:120")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "ctc_head"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunk-bytes", type=int, default=256 << 20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = dict(clock_before=ops.probe_clock(dev), K=K, utterance_rows=LQ, chunk_bytes=a.chunk_bytes, shapes=[])
    for spec in a.shapes.split(","):
        M, V, S = (int(v) for v in spec.split(":"))
        B = M // LQ
        assert B * LQ == M, f"M={M} is not a whole number of {LQ}-row utterances"
        g = torch.Generator(device="cuda").manual_seed(M + V)
        xn = F.layer_norm(torch.randn(B, LQ, K, device="cuda", generator=g), (K,))
        head = CTCOutputHead(d_model=K, vocab_size=V, dropout=0.0).to(dev).eval()
        with torch.no_grad():
            head.proj[2].weight.copy_(0.3 * torch.randn(V, K, device="cuda", generator=g))
            head.proj[2].bias.copy_(0.5 * torch.randn(V, device="cuda", generator=g))
        W, b = head.proj[2].weight, head.proj[2].bias
        tg = torch.randint(1, V, (B, S), device="cuda", generator=g, dtype=torch.int32)
        ilen = torch.full((B,), LQ, device="cuda", dtype=torch.int32)
        tlen = torch.full((B,), S, device="cuda", dtype=torch.int32)
        x2 = xn.view(M, K)

        def fwd_fused():
            with torch.no_grad():
                return ops.ctc_head_emissions(x2, W, b, tg, ilen, tlen, B=B)[0]

        def fwd_unfused():
            with torch.no_grad():
                return ops.ctc_emissions(ops.gemm(x2, W, b).view(B, LQ, V), tg, ilen, tlen)[0]

        fused = CTCHeadLoss(head, differentiable=True, fused=True, chunk_bytes=a.chunk_bytes)
        unfused = CTCLoss(differentiable=True)

        def step_fused():
            x = xn.detach().requires_grad_(True)
            head.zero_grad(set_to_none=True)
            fused(x, tg, ilen, tlen, normalized=True).backward()
            return x.grad

        def step_unfused():
            x = xn.detach().requires_grad_(True)
            head.zero_grad(set_to_none=True)
            unfused(F.linear(x, W, b), tg, ilen, tlen).backward()
            return x.grad

        logits = ops.gemm(x2, W, b).view(B, LQ, V)

        def piece_lse():
            return ops.gemm_lse(x2, W, b)

        def piece_gemm():
            return ops.gemm(x2, W, b)

        def piece_emissions():
            return ops.ctc_emissions(logits, tg, ilen, tlen)[0]

        diff = float((fwd_fused() - fwd_unfused()).abs().max())
        t = timed(dict(forward_fused=fwd_fused, forward_unfused=fwd_unfused), a.reps)
        t.update(timed(dict(piece_lse_gemm=piece_lse, piece_plain_gemm=piece_gemm, piece_emissions=piece_emissions), a.reps))
        del logits
        t.update(timed(dict(step_fused=step_fused, step_unfused=step_unfused), a.reps))
        mem = {k: peak_over(fn) for k, fn in dict(forward_fused=fwd_fused, forward_unfused=fwd_unfused,
                                                  step_fused=step_fused, step_unfused=step_unfused).items()}
        rec = dict(M=M, V=V, S=S, B=B, logits_bytes=M * V * 4, engine_lse=ops.gemm_tile(M, V, K, epilogue=L.EPI_LSE),
                   engine_plain=ops.gemm_tile(M, V, K), max_abs_emission_diff=diff, times=t, peak_bytes=mem)
        res["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
        del head, fused, W, b
        torch.cuda.empty_cache()
    res["clock_after"] = ops.probe_clock(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    with open(a.out + ".md", "w") as f:
        f.write("# CTC loss on the head: logit-free against through the logits\n\n"
                f"tools/ctc_head_time.py, K = {K}, utterances of {LQ} rows, medians of {a.reps} event-timed windows, the two\n"
                f"paths alternating in one process; backward chunk {a.chunk_bytes >> 20} MiB.  Clock: see the JSON's\n"
                "clock_before / clock_after (ops.probe_clock).\n\n"
                "Engine: what ops.gemm_tile names for the log-sum-exp GEMM / the plain one (1 = the rows engine).\n\n"
                "| M | V | S | engine | forward fused us | forward unfused us | step fused us | step unfused us | "
                "peak fwd fused MB | peak fwd unfused MB | peak step fused MB | peak step unfused MB | "
                "lse GEMM us | plain GEMM us | emissions of logits us |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in res["shapes"]:
            t, m = r["times"], r["peak_bytes"]
            f.write(f"| {r['M']} | {r['V']} | {r['S']} | {r['engine_lse']} / {r['engine_plain']} | {t['forward_fused']['median_us']} | {t['forward_unfused']['median_us']} | "
                    f"{t['step_fused']['median_us']} | {t['step_unfused']['median_us']} | "
                    + " | ".join(f"{m[k] / 1e6:.1f}" for k in ("forward_fused", "forward_unfused", "step_fused", "step_unfused"))
                    + f" | {t['piece_lse_gemm']['median_us']} | {t['piece_plain_gemm']['median_us']} | "
                    f"{t['piece_emissions']['median_us']} |\n")


if __name__ == "__main__":
    main()
