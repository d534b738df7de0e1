"""Diagnostic (GPU box): where the rows engine's waves spend their cycles, from a build with
-DVASR_ROWS_STAMPS (tools/build_variant_lib.sh rowstamps -DVASR_ROWS_STAMPS; VASR_LIB=<that .so>).

Each wave sums s_memtime cycles per phase of its chunk steps -- the counted vmcnt wait, the block
barrier, the previous chunk's epilogue (bias / softplus, buffer stores issued), the DMA issue and
the chunk's 72 MFMAs + fragment reads -- and writes the sums once at the end.  Printed: per phase
the mean over the waves of each role, in cycles and as a share of the wave's whole kernel time.
Roles: the 8-wave kernel's loader and store-only waves (-DVASR_ROWS_ROLES=0), or the
wave-specialised kernel's compute waves (barrier, MFMA, and under "epilogue" the accumulator's
hand-off to LDS) and memory waves (wait, barrier, DMA issue, epilogue = store issue; with
-DVASR_ROWS_DMA_WAVES=2 DMA-only and store-only memory waves).
For the wave-specialised kernel's compute waves the first column is the A prologue (kernel start to
the last split8; they have no counted wait), and with two accumulators (VASR_ROWS_ACC2) "epilogue" is
only the last tile's hand-off: the others leave inside the MFMA phase.
Usage: rows_stamps.py [M ...] (composed head GEMM, K = 192; ROWS_N=896 the z-in-tail projection;
ROWS_NOUT=<column> moves the first softplus column; ROWS_EPI=argmax ROWS_N=1000: the CTC head's argmax GEMM, run under the forced rows engine).
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "velocity-asr_amd"))
import torch  # noqa: E402

from velocity_asr import _lib, ops  # noqa: E402

_lib.require_device()
lib = _lib.lib()
if not hasattr(lib, "vasr_diag_rows_stamps"):
    sys.exit("rows_stamps.py: the loaded library was not built with -DVASR_ROWS_STAMPS")
lib.vasr_diag_rows_stamps.argtypes = [ctypes.c_void_p]
Ms = [int(v) for v in sys.argv[1:]] or [8016, 16032]
g0 = torch.Generator(device="cuda").manual_seed(0)
# ROWS_N=896: the z-in-tail projection (x | B | C | dt, softplus from 512); default the 1280-column form
NC = int(os.environ.get("ROWS_N", "1280"))
ARGMAX = os.environ.get("ROWS_EPI", "softplus") == "argmax"
NOUT = int(os.environ.get("ROWS_NOUT", NC - 384))  # softplus from this column on
w = torch.randn(NC, 192, device="cuda", generator=g0) * 0.07
b = torch.cat([torch.zeros(NC - 384, device="cuda"), torch.randn(384, device="cuda", generator=g0) * 0.1])
buf = torch.zeros(4096 * 8 * 8, device="cuda", dtype=torch.int64)  # 8 counters per wave; grids here stay below 4096 blocks
NAMES = ("wait", "barrier", "epilogue", "dma", "mfma")
for M in Ms:
    u = torch.randn(M, 192, device="cuda", generator=g0)
    out = torch.empty(M, NC, device="cuda")

    def launch():
        if ARGMAX:
            with ops.option(_lib.OPT_GEMM_ENGINE, 2):
                ops._gemm_argmax_keys(u, w, b, None, None, "rows_stamps")
        else:
            ops.gemm(u, w, b, epilogue=_lib.EPI_SOFTPLUS_FROM, n_out=NOUT, out=out)
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    buf.zero_()
    assert lib.vasr_diag_rows_stamps(ctypes.c_void_p(buf.data_ptr())) == 0
    launch()
    torch.cuda.synchronize()
    assert lib.vasr_diag_rows_stamps(ctypes.c_void_p(0)) == 0
    st = buf.view(-1, 8).cpu()
    st = st[st[:, 5] > 0]
    ROLES = ((1, "loader"), (0, "store-only"), (2, "compute"), (3, "memory"), (4, "mem DMA-only"), (5, "mem store-only"))
    for kind, sel in ((name, st[:, 7] == code) for code, name in ROLES):
        if not sel.any():
            continue
        x = st[sel].double()
        tot = x[:, 5].mean().item()
        names = ("prologue",) + NAMES[1:] if kind == "compute" else NAMES
        parts = ", ".join(f"{n} {x[:, i].mean().item():.0f} ({x[:, i].mean().item() / tot:.0%})" for i, n in enumerate(names))
        print(f"M={M} {kind:14s} waves {int(sel.sum())}, chunks/wave {x[:, 6].mean().item():.1f}: total {tot:.0f} cyc; "
              f"{parts}; max total {x[:, 5].max().item():.0f}", flush=True)
