"""Times the selective scan's training kernels: the checkpointing forward (vasr_ssm_scan_save_f32), the
plain mode-1 forward of the same library in the same run (vasr_ssm_scan_f32, the baseline) and the
backward (vasr_ssm_scan_bwd_f32: the reverse-time kernel + the dB / dC second pass), the C entry points
on preallocated buffers, interleaved inside a round.  Device events around batches of launches, after
a warm-up; operands, checkpoints, outputs and workspace rotate through enough sets to exceed the
256 MiB Infinity Cache.
    python tools/scan_grad_time.py [--shapes 32:501:384:64,1:501:384:64,32:63:384:32] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "velocity-asr_amd"))
import torch  # noqa: E402

from velocity_asr import _lib, ops  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X


def timed(fns, reps=7, inner=10):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32:501:384:64,1:501:384:64,32:63:384:32")
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = _lib.lib()
    res = dict(clock=ops.probe_clock(torch.device("cuda", 0)), shapes=[])
    for spec in a.shapes.split(","):
        B, L, Di, N = (int(v) for v in spec.split(":"))
        M = B * L
        nd = Di // ops.scan_bwd_channels(N)
        nck = int(lib.vasr_ssm_scan_checkpoint_floats(B, L, Di, N))
        nws = int(lib.vasr_ssm_scan_bwd_workspace_floats(B, L, Di, N))
        # algorithmic bytes of the backward: operands read once (x, z, dt, g; B, C; A, A2, D), the seven
        # gradients written once (dx, ddt, dz; dB, dC; dA; dD), the checkpoints read once
        alg = 4 * (4 * M * Di + 2 * M * N + 2 * N + Di + 3 * M * Di + 2 * M * N + N + Di + nck)
        # what the launches move besides: the dB / dC partials written and read once, the dA / dD partials written
        moved = alg + 4 * (2 * nws + B * Di * N + B * Di)
        set_bytes = moved + 4 * M * Di  # + the forward's out
        nset = 2 if set_bytes >= (160 << 20) else min(8, -(-(320 << 20) // set_bytes))
        gen = torch.Generator(device="cuda").manual_seed(B * 7 + L)
        rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)  # noqa: E731
        A = -torch.arange(1, N + 1, device="cuda", dtype=torch.float32)
        A2 = A * torch.tensor(ops.LOG2E, dtype=torch.float32)
        D = rn(Di)
        sets = []
        for _ in range(nset):
            xz = rn(M, 2 * Di)
            s = dict(xz=xz, x=xz[:, :Di], z=xz[:, Di:], dt=torch.nn.functional.softplus(rn(M, Di) - 1.0), bc=rn(M, 2 * N),
                     g=rn(M, Di), out=torch.empty(M, Di, device="cuda"), out1=torch.empty(M, Di, device="cuda"),
                     ckpt=torch.empty(nck, device="cuda"), ws=torch.empty(nws, device="cuda"))
            for k, shape in (("dx", (M, Di)), ("ddt", (M, Di)), ("dz", (M, Di)), ("dB", (M, N)), ("dC", (M, N)),
                             ("dA_part", (B, Di, N)), ("dD_part", (B, Di))):
                s[k] = torch.empty(shape, device="cuda")
            sets.append(s)
        st = torch.cuda.current_stream().cuda_stream
        turn = [0]

        def nxt():
            turn[0] = (turn[0] + 1) % nset
            return sets[turn[0]]

        def save():
            s = nxt()
            rc = lib.vasr_ssm_scan_save_f32(s["xz"].data_ptr(), 2 * Di, s["dt"].data_ptr(), Di, s["bc"].data_ptr(), 2 * N,
                                            A2.data_ptr(), D.data_ptr(), s["out"].data_ptr(), Di, B, L, Di, N, 1,
                                            s["ckpt"].data_ptr(), nck, st)
            assert rc == 0

        def plain():
            s = nxt()
            rc = lib.vasr_ssm_scan_f32(s["xz"].data_ptr(), 2 * Di, s["dt"].data_ptr(), Di, s["bc"].data_ptr(), 2 * N,
                                       A2.data_ptr(), D.data_ptr(), s["out1"].data_ptr(), Di, B, L, Di, N, 1, st)
            assert rc == 0

        def bwd():
            s = nxt()
            rc = lib.vasr_ssm_scan_bwd_f32(s["x"].data_ptr(), 2 * Di, s["z"].data_ptr(), 2 * Di, s["dt"].data_ptr(), Di,
                                           s["bc"].data_ptr(), 2 * N, A.data_ptr(), A2.data_ptr(), D.data_ptr(),
                                           s["g"].data_ptr(), Di, s["ckpt"].data_ptr(), s["dx"].data_ptr(),
                                           s["ddt"].data_ptr(), s["dz"].data_ptr(), s["dB"].data_ptr(), s["dC"].data_ptr(),
                                           s["dA_part"].data_ptr(), s["dD_part"].data_ptr(), s["ws"].data_ptr(), nws, B, L,
                                           Di, N, st)
            assert rc == 0

        for _ in range(nset):  # every set's checkpoints exist before the backward is timed
            save()
        for _ in range(nset):
            plain()
        torch.cuda.synchronize()
        assert all(torch.equal(s["out"], s["out1"]) for s in sets)
        t = timed({"forward_plain_mode1": plain, "forward_checkpointing": save, "backward": bwd})
        assert all(bool(torch.isfinite(s[k]).all()) for s in sets for k in ("dx", "ddt", "dz", "dB", "dC", "dA_part"))
        us = t["backward"]["median_us"]
        t["backward"].update(algorithmic_bytes=alg, hbm_peak_frac=round(alg / (us * 1e-6) / HBM_PEAK, 4), moved_bytes=moved,
                             moved_hbm_peak_frac=round(moved / (us * 1e-6) / HBM_PEAK, 4))
        rec = dict(B=B, L=L, Di=Di, N=N, sets=nset, checkpoint_bytes=4 * nck, workspace_bytes=4 * nws,
                   backward_over_plain_forward=round(us / t["forward_plain_mode1"]["median_us"], 2),
                   checkpointing_over_plain_forward=round(t["forward_checkpointing"]["median_us"]
                                                          / t["forward_plain_mode1"]["median_us"], 3), times=t)
        res["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
        del sets
        torch.cuda.empty_cache()
    print(json.dumps(dict(clock=res["clock"])), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
