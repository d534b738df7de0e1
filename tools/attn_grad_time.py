"""Times the pooled attention's training path at the workload's shape (L 501, Kp 16, 4 heads x 12):
  backward         vasr_pooled_attention_bwd_f32 alone (its two launches), preallocated outputs;
  forward          the inference kernel (ops.pooled_attention), for scale;
  op_fwd_bwd       velocity_asr.attention.pooled_attention forward + backward under autograd;
  torch_fwd_bwd    the same attention as torch ops (matmul, softmax, matmul) forward + backward under
                   torch autograd on the same device -- the yardstick: no earlier kernel existed.
Device events around batches of calls, after a warm-up; the four alternate inside a round; median with
min - max over the rounds.
    python tools/attn_grad_time.py [--shapes 32:501:16:4:12,1:501:16:4:12] [--out FILE.json] [--md FILE.md]"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "velocity-asr_amd"))
import torch  # noqa: E402

from velocity_asr import _lib, attention, ops  # noqa: E402


def timed(fns, reps, inner):
    """Median / min / max us per call of each fn: `reps` rounds, the fns alternating within a round."""
    for fn in fns.values():
        for _ in range(3):
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
    return {k: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2),
                    max_us=round(max(v), 2)) for k, v in out.items()}


def torch_attention(q, kv, heads):
    """softmax(q k^T / sqrt(hd)) v per head as torch ops (the reference's attention.py:143-161)."""
    B, L, A = q.shape
    Kp, hd = kv.shape[1], A // heads
    qh = q.view(B, L, heads, hd).transpose(1, 2)
    kh = kv[..., :A].reshape(B, Kp, heads, hd).transpose(1, 2)
    vh = kv[..., A:].reshape(B, Kp, heads, hd).transpose(1, 2)
    p = torch.softmax(torch.matmul(qh, kh.transpose(-2, -1)) / math.sqrt(hd), dim=-1)
    return torch.matmul(p, vh).transpose(1, 2).contiguous().view(B, L, A)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32:501:16:4:12,1:501:16:4:12")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--md")
    a = ap.parse_args()
    lib = _lib.lib()
    res = dict(clock=ops.probe_clock(torch.device("cuda", 0)), reps=a.reps, inner=a.inner, shapes=[])
    for spec in a.shapes.split(","):
        B, L, Kp, heads, hd = (int(v) for v in spec.split(":"))
        A = heads * hd
        gen = torch.Generator(device="cuda").manual_seed(B * 7 + L)
        rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)  # noqa: E731
        q, kv, g = rn(B, L, A), rn(B, Kp, 2 * A), rn(B, L, A)
        q2, kv2, g2 = q.view(B * L, A), kv.view(B * Kp, 2 * A), g.view(B * L, A)
        dq, dkv = torch.empty_like(q2), torch.empty_like(kv2)
        nws = int(lib.vasr_pooled_attention_bwd_workspace_floats(B, L, Kp, heads, hd))
        ws = torch.empty(nws, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        qr, kvr = q.clone().requires_grad_(), kv.clone().requires_grad_()

        def backward():
            rc = lib.vasr_pooled_attention_bwd_f32(q2.data_ptr(), A, kv2.data_ptr(), g2.data_ptr(), dq.data_ptr(),
                                                   dkv.data_ptr(), ws.data_ptr(), nws, B, L, Kp, heads, hd, None, st)
            assert rc == 0

        def forward():
            ops.pooled_attention(q2, kv2, B, L, Kp, heads)

        def op_fwd_bwd():
            qr.grad = kvr.grad = None
            attention.pooled_attention(qr, kvr, heads).backward(g)

        def torch_fwd_bwd():
            qr.grad = kvr.grad = None
            torch_attention(qr, kvr, heads).backward(g)

        t = timed({"backward": backward, "forward": forward, "op_fwd_bwd": op_fwd_bwd, "torch_fwd_bwd": torch_fwd_bwd},
                  a.reps, a.inner)
        # the two agree (same function): a guard against timing something else
        op_fwd_bwd()
        ours = (qr.grad.clone(), kvr.grad.clone())
        torch_fwd_bwd()
        torch.cuda.synchronize()
        assert torch.allclose(ours[0], qr.grad, atol=1e-4, rtol=1e-4) and torch.allclose(ours[1], kvr.grad, atol=1e-3, rtol=1e-4)
        assert torch.equal(ours[0].view(B * L, A), dq) and torch.equal(ours[1].view(B * Kp, 2 * A), dkv)
        # bytes of a backward: q, dout read, dq written, kv read per (tile, head), partials written and read, dkv written
        tiles = -(-L // ops.ATTN_BWD_TILE)
        moved = 4 * (3 * B * L * A + B * tiles * Kp * 2 * A * 3 + B * Kp * 2 * A)
        rec = dict(B=B, L=L, Kp=Kp, heads=heads, hd=hd, workspace_bytes=4 * nws, backward_bytes=moved,
                   torch_over_op_fwd_bwd=round(t["torch_fwd_bwd"]["median_us"] / t["op_fwd_bwd"]["median_us"], 2), times=t)
        res["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
    print(json.dumps(dict(clock=res["clock"])), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if a.md:
        cell = lambda d: f"{d['median_us']:.1f} ({d['min_us']:.1f} - {d['max_us']:.1f})"  # noqa: E731
        rows = ["| B : L : Kp : heads : hd | backward (2 launches) | forward | operator fwd + bwd | torch ops fwd + bwd | "
                "torch / operator | backward bytes |", "|---|---|---|---|---|---|---|"]
        for r in res["shapes"]:
            t = r["times"]
            rows.append(f"| {r['B']} : {r['L']} : {r['Kp']} : {r['heads']} : {r['hd']} | {cell(t['backward'])} | "
                        f"{cell(t['forward'])} | {cell(t['op_fwd_bwd'])} | {cell(t['torch_fwd_bwd'])} | "
                        f"{r['torch_over_op_fwd_bwd']} | {r['backward_bytes'] / 1e6:.1f} MB |")
        with open(a.md, "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
