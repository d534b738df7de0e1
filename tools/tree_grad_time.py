"""Times the tree scan's training kernels (scan_mode="parallel"): its forward (the inference kernel,
ops.ssm_scan at the default tree mode 2, into a preallocated out) and its backward
(vasr_ssm_tree_bwd_f32: four launches), and beside them, in the same run, the recurrence's forward
(vasr_ssm_scan_f32 mode 1) and backward (vasr_ssm_scan_bwd_f32 from vasr_ssm_scan_save_f32's
checkpoints), interleaved inside a round.  Device events around batches of launches, after a warm-up;
operands, outputs and workspaces rotate through enough sets to exceed the 256 MiB Infinity Cache.
    python tools/tree_grad_time.py [--shapes 32:501:384:64,32:64:384:32] [--out FILE.json] [--md FILE.md]
The default shapes are the local block's scan and the global block's."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "velocity-asr_amd"))
import torch  # noqa: E402

from velocity_asr import _lib, ops  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X


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


def outer_accesses(M):
    """Float loads + stores per (utterance, channel, state) lane of the outer-tree kernel over M chunk
    composites: its loops (csrc/scan_tree_bwd.hip, tree_bwd_outer_kernel) counted, not timed."""
    n = 5 * M  # the first pass: alpha and J read; J, d beta and the local terms written
    for with_grad in (True, False):
        ln = 1
        while ln < M:
            pos = 0
            for base in range(0, M - ln, 2 * ln):
                n += base - pos            # alpha over the previous sibling
                pos = base + ln
                if with_grad:
                    n += 3 * ln            # alpha, beta read, rho written
                    n += min(base + 2 * ln, M) - pos + 2    # G over the sibling; one read-modify-write
                    n += 2 * ln + 4 * (ln - 1)              # d beta; alpha, rho, the local terms
                else:
                    n += 2 * ln + 2 * (min(base + 2 * ln, M) - pos)  # alpha, beta; H read-modify-write
            ln *= 2
    return n + 3 * M + M + 2 * M  # the suffix sum, H zeroed, Pi over alpha


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32:501:384:64,32:64:384:32")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--md")
    a = ap.parse_args()
    lib = _lib.lib()
    res = dict(clock=ops.probe_clock(torch.device("cuda", 0)), reps=a.reps, inner=a.inner, shapes=[])
    for spec in a.shapes.split(","):
        B, L, Di, N = (int(v) for v in spec.split(":"))
        M = B * L
        nch = -(-L // 16)
        nck = int(lib.vasr_ssm_scan_checkpoint_floats(B, L, Di, N))
        nws_rec = int(lib.vasr_ssm_scan_bwd_workspace_floats(B, L, Di, N))
        nws = int(lib.vasr_ssm_tree_bwd_workspace_floats(B, L, Di, N))
        # algorithmic bytes of a backward: operands read once (x, z, dt, g; B, C; A, A2, D), the seven
        # gradients written once (dx, ddt, dz; dB, dC; dA; dD)
        alg = 4 * (4 * M * Di + 2 * M * N + 2 * N + Di + 3 * M * Di + 2 * M * N + N + Di)
        # what the four launches move: the operands read twice (chunk and inner kernels), the chunk kernel's
        # four slots written, the outer kernel's accesses, the inner kernel's four slots read and its dA / dD
        # partials written, those read again, the per-(utterance, channel) dA / dD written
        slot = B * nch * Di * N
        # (up to 32 chunks the outer kernel keeps a lane's columns in registers: four slots read, four written)
        outer = B * Di * N * (8 * nch if nch <= 32 else outer_accesses(nch))
        moved = alg + 4 * (4 * M * Di + 2 * M * N + 4 * slot + outer + 5 * slot + 2 * B * nch * Di + slot
                           + B * Di * N + B * Di)
        set_bytes = moved // 2 + 4 * (nws + nws_rec + nck + 2 * M * Di)
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
                     ckpt=torch.empty(nck, device="cuda"), ws_rec=torch.empty(nws_rec, device="cuda"),
                     ws=torch.empty(nws, device="cuda"))
            for k, shape in (("dx", (M, Di)), ("ddt", (M, Di)), ("dz", (M, Di)), ("dB", (M, N)), ("dC", (M, N)),
                             ("dA_part", (B, Di, N)), ("dD_part", (B, Di))):
                s[k] = torch.empty(shape, device="cuda")
            sets.append(s)
        st = torch.cuda.current_stream().cuda_stream
        turn = [0]

        def nxt():
            turn[0] = (turn[0] + 1) % nset
            return sets[turn[0]]

        def tree_fwd():
            s = nxt()
            ops.ssm_scan(s["xz"], s["dt"], s["bc"], A2, D, B, L, 2, out=s["out"])

        def rec_fwd():
            s = nxt()
            rc = lib.vasr_ssm_scan_f32(s["xz"].data_ptr(), 2 * Di, s["dt"].data_ptr(), Di, s["bc"].data_ptr(), 2 * N,
                                       A2.data_ptr(), D.data_ptr(), s["out1"].data_ptr(), Di, B, L, Di, N, 1, st)
            assert rc == 0

        def save():
            s = nxt()
            rc = lib.vasr_ssm_scan_save_f32(s["xz"].data_ptr(), 2 * Di, s["dt"].data_ptr(), Di, s["bc"].data_ptr(), 2 * N,
                                            A2.data_ptr(), D.data_ptr(), s["out1"].data_ptr(), Di, B, L, Di, N, 1,
                                            s["ckpt"].data_ptr(), nck, st)
            assert rc == 0

        def grads(s):
            return (s["dx"].data_ptr(), s["ddt"].data_ptr(), s["dz"].data_ptr(), s["dB"].data_ptr(), s["dC"].data_ptr(),
                    s["dA_part"].data_ptr(), s["dD_part"].data_ptr())

        def operands(s):
            return (s["x"].data_ptr(), 2 * Di, s["z"].data_ptr(), 2 * Di, s["dt"].data_ptr(), Di, s["bc"].data_ptr(), 2 * N,
                    A.data_ptr(), A2.data_ptr(), D.data_ptr(), s["g"].data_ptr(), Di)

        def rec_bwd():
            s = nxt()
            rc = lib.vasr_ssm_scan_bwd_f32(*operands(s), s["ckpt"].data_ptr(), *grads(s), s["ws_rec"].data_ptr(), nws_rec,
                                           B, L, Di, N, st)
            assert rc == 0

        def tree_bwd():
            s = nxt()
            rc = lib.vasr_ssm_tree_bwd_f32(*operands(s), *grads(s), s["ws"].data_ptr(), nws, B, L, Di, N, st)
            assert rc == 0

        for _ in range(nset):  # every set's checkpoints exist before the recurrence's backward is timed
            save()
        torch.cuda.synchronize()
        t = timed({"tree_forward": tree_fwd, "tree_backward": tree_bwd, "recurrence_forward": rec_fwd,
                   "recurrence_backward": rec_bwd}, a.reps, a.inner)
        for _ in range(nset):  # the last writer of every set's gradients: the tree's backward
            tree_bwd()
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(s[k]).all()) for s in sets for k in ("dx", "ddt", "dz", "dB", "dC", "dA_part"))
        us = t["tree_backward"]["median_us"]
        t["tree_backward"].update(algorithmic_bytes=alg, hbm_peak_frac=round(alg / (us * 1e-6) / HBM_PEAK, 4),
                                  moved_bytes=moved, moved_hbm_peak_frac=round(moved / (us * 1e-6) / HBM_PEAK, 4),
                                  outer_kernel_bytes=4 * outer)
        rec = dict(B=B, L=L, Di=Di, N=N, sets=nset, workspace_bytes=4 * nws, state_array_bytes=4 * M * Di * N,
                   tree_backward_over_recurrence_backward=round(us / t["recurrence_backward"]["median_us"], 2),
                   tree_backward_over_tree_forward=round(us / t["tree_forward"]["median_us"], 2), times=t)
        res["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
        del sets
        torch.cuda.empty_cache()
    print(json.dumps(dict(clock=res["clock"])), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if a.md:
        cell = lambda d: f"{d['median_us']:.1f} ({d['min_us']:.1f} - {d['max_us']:.1f})"  # noqa: E731
        rows = ["| B : L : Di : N | tree forward | tree backward | recurrence forward | recurrence backward | "
                "tree / recurrence backward | workspace |", "|---|---|---|---|---|---|---|"]
        for r in res["shapes"]:
            t = r["times"]
            rows.append(f"| {r['B']} : {r['L']} : {r['Di']} : {r['N']} | {cell(t['tree_forward'])} | "
                        f"{cell(t['tree_backward'])} | {cell(t['recurrence_forward'])} | {cell(t['recurrence_backward'])} | "
                        f"{r['tree_backward_over_recurrence_backward']} | {r['workspace_bytes'] / 1e6:.1f} MB |")
        with open(a.md, "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
