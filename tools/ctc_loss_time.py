"""Times the device CTC loss: the emissions launch and the lattice launch alone, the whole
velocity_asr.training.CTCLoss call, and the same loss by torch.log_softmax + F.ctc_loss on the same
device, interleaved.  Device events around batches of launches, after a warm-up; the logits rotate
through enough buffers to exceed the 256 MiB Infinity Cache, so the emissions pass reads HBM.
    python tools/ctc_loss_time.py [--shapes 32:501:1000:100,1:501:1000:100] [--out FILE.json]"""
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
    return {k: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32:501:1000:100,1:501:1000:100")
    ap.add_argument("--out")
    a = ap.parse_args()
    res = dict(clock=ops.probe_clock(torch.device("cuda", 0)), shapes=[])
    for spec in a.shapes.split(","):
        B, L, V, S = (int(v) for v in spec.split(":"))
        nbuf = max(2, -(-(320 << 20) // (B * L * V * 4))) if B * L * V * 4 >= (8 << 20) else 2
        nbuf = min(nbuf, 8)
        g = torch.Generator(device="cuda").manual_seed(B * 7 + L)
        bufs = [torch.randn(B, L, V, device="cuda", generator=g) for _ in range(nbuf)]
        tg = torch.randint(1, V, (B, S), device="cuda", generator=g, dtype=torch.int32)
        ilen = torch.full((B,), L, device="cuda", dtype=torch.int32)
        tlen = torch.full((B,), S, device="cuda", dtype=torch.int32)
        tg64, ilen64, tlen64 = tg.long(), ilen.long(), tlen.long()
        emis, _, _, _ = ops.ctc_emissions(bufs[0], tg, ilen, tlen)
        loss = CTCLoss(reduction="mean")
        turn = [0]

        def nxt():
            turn[0] = (turn[0] + 1) % nbuf
            return bufs[turn[0]]

        def torch_loss():
            lp = F.log_softmax(nxt(), dim=-1).transpose(0, 1)
            return F.ctc_loss(lp, tg64, ilen64, tlen64, blank=0, reduction="mean", zero_infinity=True)

        ours = float(loss(bufs[0], tg, ilen, tlen))
        turn[0] = -1
        theirs = float(torch_loss())
        # the launches alone: the C entry points on preallocated buffers (no wrapper work between them)
        lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
        nll = torch.empty(B, device="cuda")
        ws = torch.empty(int(lib.vasr_ctc_align_workspace_bytes(B, L, S)) // 4, device="cuda", dtype=torch.int32)
        state = torch.empty(B, L, device="cuda", dtype=torch.int32)
        sp0, sp1 = torch.empty(B, S, device="cuda", dtype=torch.int32), torch.empty(B, S, device="cuda", dtype=torch.int32)

        def emissions():
            x = nxt()
            rc = lib.vasr_ctc_emissions_f32(x.data_ptr(), V, L * V, B, L, V, tg.data_ptr(), S, ilen.data_ptr(),
                                            tlen.data_ptr(), 0, emis.data_ptr(), st)
            assert rc == 0

        def lattice():
            rc = lib.vasr_ctc_loss_f32(emis.data_ptr(), B, L, S, tg.data_ptr(), ilen.data_ptr(), tlen.data_ptr(),
                                       nll.data_ptr(), st)
            assert rc == 0

        def align():
            rc = lib.vasr_ctc_align_f32(emis.data_ptr(), B, L, S, tg.data_ptr(), ilen.data_ptr(), tlen.data_ptr(),
                                        ws.data_ptr(), ws.numel() * 4, state.data_ptr(), sp0.data_ptr(), sp1.data_ptr(),
                                        nll.data_ptr(), st)
            assert rc == 0

        t = timed({
            "emissions": emissions,
            "lattice": lattice,
            "align": align,
            "CTCLoss": lambda: loss(nxt(), tg, ilen, tlen),
            "torch_log_softmax_ctc_loss": torch_loss,
            "torch_log_softmax_only": lambda: F.log_softmax(nxt(), dim=-1),
        })
        nbytes = B * L * V * 4
        t["emissions"]["algorithmic_bytes"] = nbytes
        t["emissions"]["hbm_peak_frac"] = round(nbytes / (t["emissions"]["median_us"] * 1e-6) / HBM_PEAK, 4)
        rec = dict(B=B, L=L, V=V, S=S, logits_buffers=nbuf, loss_ours=ours, loss_torch=theirs, times=t)
        res["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
    print(json.dumps(dict(clock=res["clock"])), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
