#!/usr/bin/env python3
"""Launch time of the fused gated fusion + head LayerNorm (ops.fusion_tail) against the four launches
it replaces (gemm, gemm with EPI_PAIR_FUSION, gemm, layer_norm), per M: each candidate is 20 back-to-back
repetitions captured in one HIP graph, a replay between one HIP event pair, the candidates' order rotated
every round after a warm-up; median (min .. max) over the rounds, and the outputs compared bitwise.
    python tools/fusion_tail_time.py [rounds] [M ...]      (default 9 rounds, M = 16032 8016)"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "velocity-asr_amd"))
import torch  # noqa: E402

from velocity_asr import _lib, ops  # noqa: E402

REPS = 20


def main():
    _lib.require_device()
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    Ms = [int(v) for v in sys.argv[2:]] or [16032, 8016]
    dev = torch.device("cuda", 0)
    g0 = torch.Generator(device=dev).manual_seed(0)
    D, A = 192, 48
    r = lambda *s, sc=1.0: torch.randn(*s, device=dev, generator=g0) * sc  # noqa: E731
    P = dict(w_local=r(2 * D, D, sc=D ** -0.5), w_glob=r(2 * D, A, sc=A ** -0.5), b_glob=r(2 * D, sc=0.3),
             b_local=r(D, sc=0.3), w_out=r(D, D, sc=D ** -0.5), b_out=r(D, sc=0.3), ln_w=1 + r(D, sc=0.2),
             ln_b=r(D, sc=0.2))
    print(f"probe_clock {ops.probe_clock(dev)}", flush=True)
    for M in Ms:
        local, o = r(M, D), r(M, A)
        outs = {}

        def four():
            t1 = ops.gemm(local, P["w_local"])
            fused = ops.gemm(o, P["w_glob"], P["b_glob"], epilogue=_lib.EPI_PAIR_FUSION, aux=t1,
                             aux2=P["b_local"], n_out=D)
            out = ops.gemm(fused, P["w_out"], P["b_out"])
            outs["four"] = ops.layer_norm(out, P["ln_w"], P["ln_b"], 1e-5)

        def fused_rows(rows):
            def run():
                outs[f"fused{rows}"] = ops.fusion_tail(local, o, P["w_local"], P["w_glob"], P["b_glob"], P["b_local"],
                                                       P["w_out"], P["b_out"], P["ln_w"], P["ln_b"], 1e-5, rows=rows)[0]
            return run
        cands = [("four", four), ("fused32", fused_rows(32)), ("fused64", fused_rows(64))]
        graphs = []
        for name, fn in cands:
            for _ in range(3):
                fn()
            st = torch.cuda.Stream(dev)
            st.wait_stream(torch.cuda.current_stream(dev))
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=st):
                for _ in range(REPS):
                    fn()
            graphs.append((name, gr))
        torch.cuda.synchronize()
        for name in ("fused32", "fused64"):
            same = torch.equal(outs[name], outs["four"])
            print(f"M={M} {name}: output {'bitwise equal to' if same else 'DIFFERS from'} the four launches", flush=True)
        for _ in range(20):
            for _, gr in graphs:
                gr.replay()
        torch.cuda.synchronize()
        res = {n: [] for n, _ in graphs}
        for rd in range(rounds):
            k = rd % len(graphs)
            for name, gr in graphs[k:] + graphs[:k]:
                gr.replay()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                gr.replay()
                b.record()
                torch.cuda.synchronize()
                res[name].append(a.elapsed_time(b) / REPS * 1e3)
        for name, _ in graphs:
            v = sorted(res[name])
            print(f"M={M:6d} {name:8s} median {v[len(v) // 2]:7.2f} us ({v[0]:.2f} .. {v[-1]:.2f})", flush=True)


if __name__ == "__main__":
    main()
