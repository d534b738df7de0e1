"""Times the backward of the device CTC loss: the three new entry points alone (the lattice that
keeps alpha, beside the forward-only lattice it derives from; the occupancy; the logit gradient),
and the whole forward + backward of velocity_asr.training.CTCLoss(differentiable=True) against
F.log_softmax + F.ctc_loss forward + backward on the same device, interleaved inside a round.
Device events around batches of launches, after a warm-up; the logits and the gradient rotate
through enough buffers to exceed the 256 MiB Infinity Cache, so the gradient pass reads and writes HBM.
    python tools/ctc_grad_time.py [--shapes 32:501:1000:100,1:501:1000:100] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "velocity-asr_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from velocity_asr import _lib, ops  # noqa: E402
from velocity_asr.training import CTCLoss  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X


def timed(fns, reps=7, inner=20):
    """Median / min us per call of each fn: `reps` rounds, the fns alternating within a round."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32:501:1000:100,1:501:1000:100")
    ap.add_argument("--out")
    a = ap.parse_args()
    res = dict(clock=ops.probe_clock(torch.device("cuda", 0)), shapes=[])
    for spec in a.shapes.split(","):
        B, L, V, S = (int(v) for v in spec.split(":"))
        # logits + gradient of one turn: 2 buffers
        nbuf = max(2, -(-(320 << 20) // (2 * B * L * V * 4))) if B * L * V * 4 >= (8 << 20) else 2
        nbuf = min(nbuf, 8)
        g = torch.Generator(device="cuda").manual_seed(B * 7 + L)
        bufs = [torch.randn(B, L, V, device="cuda", generator=g).requires_grad_(True) for _ in range(nbuf)]
        grads = [torch.empty(B, L, V, device="cuda") for _ in range(nbuf)]
        tg = torch.randint(1, V, (B, S), device="cuda", generator=g, dtype=torch.int32)
        ilen = torch.full((B,), L, device="cuda", dtype=torch.int32)
        tlen = torch.full((B,), S, device="cuda", dtype=torch.int32)
        tg64, ilen64, tlen64 = tg.long(), ilen.long(), tlen.long()
        loss = CTCLoss(reduction="mean", differentiable=True)
        turn = [0]

        def nxt():
            turn[0] = (turn[0] + 1) % nbuf
            return turn[0]

        def ours_fwd_bwd():
            x = bufs[nxt()]
            x.grad = None
            loss(x, tg, ilen, tlen).backward()
            return x.grad

        def torch_fwd_bwd():
            x = bufs[nxt()]
            x.grad = None
            lp = F.log_softmax(x, dim=-1).transpose(0, 1)
            F.ctc_loss(lp, tg64, ilen64, tlen64, blank=0, reduction="mean", zero_infinity=True).backward()
            return x.grad

        turn[0] = 0
        g_ours = ours_fwd_bwd().clone()
        turn[0] = 0
        g_torch = torch_fwd_bwd().clone()
        diff = float((g_ours - g_torch).abs().max())

        # the launches alone: the C entry points on preallocated buffers (no wrapper work between them)
        lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
        with torch.no_grad():
            emis, _, _, _ = ops.ctc_emissions(bufs[0], tg, ilen, tlen)
        nll = torch.empty(B, device="cuda")
        alpha = torch.empty(B, L, 2 * S + 1, device="cuda")
        occ = torch.empty(B, L, S + 1, device="cuda")
        chain = torch.empty(B, S + 1, device="cuda", dtype=torch.int32)
        scale = torch.full((B,), 1.0 / (B * S), device="cuda")

        def lattice():
            rc = lib.vasr_ctc_loss_f32(emis.data_ptr(), B, L, S, tg.data_ptr(), ilen.data_ptr(), tlen.data_ptr(),
                                       nll.data_ptr(), st)
            assert rc == 0

        def lattice_alpha():
            rc = lib.vasr_ctc_loss_alpha_f32(emis.data_ptr(), B, L, S, tg.data_ptr(), ilen.data_ptr(), tlen.data_ptr(),
                                             nll.data_ptr(), alpha.data_ptr(), alpha.numel(), st)
            assert rc == 0

        def occupancy():
            rc = lib.vasr_ctc_occupancy_f32(emis.data_ptr(), alpha.data_ptr(), alpha.numel(), nll.data_ptr(), B, L, S,
                                            tg.data_ptr(), ilen.data_ptr(), tlen.data_ptr(), occ.data_ptr(), st)
            assert rc == 0

        def grad_logits():
            i = nxt()
            rc = lib.vasr_ctc_grad_logits_f32(bufs[i].data_ptr(), V, L * V, B, L, V, tg.data_ptr(), S, ilen.data_ptr(),
                                              tlen.data_ptr(), 0, occ.data_ptr(), scale.data_ptr(), chain.data_ptr(),
                                              chain.numel(), grads[i].data_ptr(), st)
            assert rc == 0

        lattice_alpha()
        occupancy()
        t = timed({
            "lattice_forward_only": lattice,
            "lattice_alpha": lattice_alpha,
            "occupancy": occupancy,
            "grad_logits": grad_logits,
            "CTCLoss_forward_backward": ours_fwd_bwd,
            "torch_log_softmax_ctc_loss_forward_backward": torch_fwd_bwd,
        })
        nbytes = B * L * V * 8  # one read and one write of (B, L, V); a row's second read comes from cache
        t["grad_logits"]["algorithmic_bytes"] = nbytes
        t["grad_logits"]["hbm_peak_frac"] = round(nbytes / (t["grad_logits"]["median_us"] * 1e-6) / HBM_PEAK, 4)
        rec = dict(B=B, L=L, V=V, S=S, buffers=nbuf, max_abs_diff_to_torch=diff, times=t)
        res["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
    print(json.dumps(dict(clock=res["clock"])), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
