#!/usr/bin/env python3
"""Throughput benchmark: VELOCITY-ASR inference, audio -> CTC tokens, on MI355X.

Workload (BASELINE.json configs[1]): the 6.17 M-parameter fp32 model, batch of 32 synthetic
10 s clips at 16 kHz per GPU.  One step = real-FFT |STFT|^2 + log-mel + full forward
(temporal binding, 8 SSM blocks, hierarchical global context, CTC head) + argmax + greedy
collapse, on audio already resident in HBM, replayed as HIP graphs.

A plain run (`python bench.py --gpus 1 --steps K --warmup W`) does only what the headline
figure needs, in this process: it builds the model and the graphs (schedule tuning included),
warms up, times the K steps, writes the last step's outputs if --dump-outputs DIR is given and
prints the result line (metric, value, unit, ms_per_step, ...).  Everything else described
below -- the roofline and per-kernel figures, the token checks against the reference and an
eager pass, the machine record, the CPU baseline, the serving leg, and for one GPU the launch
through torch.distributed.run -- runs only with --full.

--dump-outputs DIR writes what the timed path returned in its last timed step as float32
arrays: DIR/tokens.npy (batch, L; positions at and past a clip's length are -1) and
DIR/lengths.npy (batch,); with more than one rank, tokens_rank<r>.npy and lengths_rank<r>.npy.
Weights and audio are seeded, so two runs with the same arguments have identical inputs.

Multi-GPU: one process per GPU.  `python bench.py --gpus N` (N > 1, or --full) without WORLD_SIZE
starts `python -m torch.distributed.run --nproc-per-node N bench.py ...` as a child process (before
anything touches the GPU) and exits with its code.  Each rank transcribes its own 32 clips
(utterance sharding, no data-path collective; weak scaling); a barrier + synchronize brackets
the K timed steps and the max time over ranks is used -- barriers and max in a gloo process
group on the host (an RCCL communicator's mere presence slowed the replays 2.2 %).  With --full a second
timed leg ("with_scatter") runs the serving form over an RCCL ("nccl") group joined after the
first: rank 0 holds the whole (N*32, S) batch in HBM, each step scatters the shards over RCCL
(xGMI) straight into every rank's graph input, replays, and gathers the int32 tokens back to
rank 0 (velocity_asr.distributed.transcribe_sharded).

Prints ONE JSON line (rank 0):
  value         = RTFx = audio seconds transcribed by all ranks / wall seconds (resident inputs)
  ms_per_step   = wall milliseconds per timed step (the K steps between two synchronizes / K)
with --full also, among others:
  roofline      = the dominant kernel measured live with HIP events (eager replay of the same
                  steps on the launch stream) against the MI355X peak; flat scalar fields add
                  the scan's VALU roof, the HBM ceiling its arithmetic allows, and the GEMM
                  family's MFMA fraction
  cpu_baseline  = the numpy restatement of the reference path (oracle/) with the reference's
                  materialised tree scan, timed on this host (rank 0, N=1 only)
"""

import argparse
import json
import os
import socket
import subprocess
import sys
import time
from datetime import timedelta

REPO = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(REPO, "velocity-asr_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

METRIC = json.load(open(os.path.join(REPO, "BASELINE.json")))["metric"]
SR = 16000
HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec (MI355X_MICROARCH.md)
BF16_MFMA_PEAK_TFS = 2500.0  # dense bf16 MFMA (no sparsity)
F32_MFMA_PEAK_TFS = 157.3    # f32-input MFMA = fp32 vector peak
F32_VALU_PEAK_TOPS = 78.6    # fp32 vector lane-operations/s (157.3 TFLOP/s with FMA = 2 flops)
VALU_OPS_PER_ELEM = 11       # reference tree scan, fp32 ops per state element (SURVEY §8 d)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32, help="clips per GPU")
    ap.add_argument("--seconds", type=float, default=10.0, help="clip length")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run everything beyond the headline figure: roofline and "
                         "per-kernel timings, the token checks against the reference and an eager pass (they "
                         "decide the exit code), the machine record, the CPU baseline, the serving leg; with "
                         "--gpus 1 the rank is started through torch.distributed.run")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the tokens and lengths of the last timed step to DIR as float32 .npy files")
    ap.add_argument("--eager", action="store_true", help="time eager launches instead of the HIP graph")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-scatter", action="store_true", help="skip the scatter/gather serving leg")
    ap.add_argument("--serving-timeout", type=float, default=120.0,
                    help="seconds an RCCL collective of the serving leg may take before it fails that leg "
                         "(the resident line is printed either way)")
    ap.add_argument("--gloo-timeout", type=float, default=900.0, help="seconds a host-side barrier may wait")
    ap.add_argument("--inproc", action="store_true",
                    help="run a single rank in this process instead of through torch.distributed.run")
    ap.add_argument("--roofline-steps", type=int, default=3, help="with --full: eager steps of the roofline pass")
    ap.add_argument("--streams", type=int, default=0,
                    help="utterance groups replayed as separate HIP graphs on concurrent streams (the scan of one "
                         "group overlaps the GEMMs of the other; results are bitwise those of one graph); "
                         "0 = build 1 and (for an even batch of at least 8 clips) 2, keep the faster "
                         "(pipeline.autotuned_transcriber)")
    ap.add_argument("--int8", action="store_true",
                    help="BASELINE configs[4]: INT8 fake-quant model (prepare_model_for_qat + activation calibration)")
    ap.add_argument("--bf16", action="store_true",
                    help="BASELINE configs[2] per-GPU shape: the model as bf16 (bf16 weights / MFMA operands)")
    return ap.parse_args(argv)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch(args) -> int:
    """Start N ranks with torch.distributed.run as a child process (this process never touches
    the GPU: torch.cuda.device_count() does not initialise HIP on this image)."""
    visible = torch.cuda.device_count()
    if visible < args.gpus:
        log(f"bench.py: --gpus {args.gpus} requested but only {visible} GPU(s) are visible")
        return 3
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)]
    cmd += sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(cmd, env=env).returncode


class stdout_to_stderr:
    """Point file descriptor 1 at stderr for the duration (library banners written by native
    code would otherwise precede the one JSON line on stdout)."""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)
        return False


def build_model(device):
    import velocity_asr as va
    from velocity_asr import synthetic as S
    W = S.make_weights(None, seed=0)
    m = va.VELOCITYASR()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    return m.to(device).eval()


def kernel_roofline(model, audio, steps, streams=1):
    """Per-launch times of the scan and GEMM families over `steps` eager steps (HIP events on
    each launch's own stream), run as the timed graphs run: `streams` utterance groups issued
    on concurrent streams, so the launches have the graph's shapes and the same overlap (and
    a rocprofv3 trace of this command sees one population per kernel)."""
    from velocity_asr import ops
    from velocity_asr.pipeline import audio_to_token_ids
    g = audio.shape[0] // streams
    sts = [torch.cuda.Stream(audio.device) for _ in range(streams)]
    main = torch.cuda.current_stream(audio.device)
    with ops.kernel_timer("ssm_scan", "gemm") as kt:
        for _ in range(steps):
            for i, st in enumerate(sts):
                st.wait_stream(main)
                with torch.cuda.stream(st):
                    audio_to_token_ids(model, audio[i * g:(i + 1) * g])
            for st in sts:
                main.wait_stream(st)
    rec = kt.summary()
    out = {}
    # selective scan of the 8 local blocks (N=64): bytes = B*L*(4*Di + 2*N)*4 per launch (x, z, dt
    # and the output per channel, B and C per state); the ungated scan of the z-in-tail block reads
    # no z: B*L*(3*Di + 2*N)*4
    scans = [(dt, i) for dt, i in rec["ssm_scan"] if i["N"] == model.config.ssm_state_dim]
    if scans:
        i = scans[0][1]
        bytes_per = i["B"] * i["L"] * ((3 if i.get("ungated") else 4) * i["Di"] + 2 * i["N"]) * 4
        elems = i["B"] * i["L"] * i["Di"] * i["N"]
        t = float(np.mean([d for d, _ in scans]))
        out["scan"] = dict(t=t, bytes=bytes_per, elems=elems, launches=len(scans), per_step=len(scans) / steps,
                           total=sum(d for d, _ in scans) / steps, B=i["B"], Di=i["Di"], N=i["N"], L=i["L"],
                           ungated=bool(i.get("ungated")))
    g = rec["gemm"]
    flops = [2.0 * i["M"] * i["N"] * i["K"] * i["batch"] for _, i in g]
    groups = {}
    for (d, i), f in zip(g, flops):
        k = (i["M"], i["N"], i["K"], i["batch"])
        groups.setdefault(k, []).append((d, f))
    top = max(groups.items(), key=lambda kv: sum(d for d, _ in kv[1]))
    out["gemm"] = dict(t=float(np.mean([d for d, _ in g])), flops=float(np.mean(flops)), launches=len(g),
                       per_step=len(g) / steps, total=sum(d for d, _ in g) / steps,
                       tflops=sum(flops) / max(sum(d for d, _ in g), 1e-12) / 1e12,
                       top_shape="M=%d N=%d K=%d batch=%d" % top[0], top_key=top[0],
                       top_t=float(np.mean([d for d, _ in top[1]])),
                       top_flops=top[1][0][1], top_total=sum(d for d, _ in top[1]) / steps)
    return out


def isolated_times(model, audio, reps=20):
    """Per-launch device time of the two dominant kernels alone, on the bench's own operands
    (local block 0 of this batch): `reps` back-to-back launches on one stream bracketed by one
    HIP event pair, so the average holds the kernel and the queue's dispatch gap only -- the
    quantity a rocprofv3 kernel trace of this command averages (profiles/r04*_summary.md)."""
    from velocity_asr import audio as A
    from velocity_asr import ops

    def per_launch(fn):
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3 / reps
    with torch.no_grad():
        mel = A.mel_on_device(audio, frame_pad=model.temporal_binding.conv_padding())
        x = model.temporal_binding(mel).contiguous()
        B, L, D = x.shape
        blk = model.local_ssm.layers[0]
        u = ops.ln_dwconv(x, blk.norm1.weight, blk.norm1.bias, ops.f32(blk.conv.weight).view(D, -1),
                          blk.conv.bias, blk.norm1.eps).view(B * L, D)
        p = blk.ssm._prepared()
        if blk._z_in_tail(B, L, D):  # the z-in-tail block: projection without z, ungated scan, gated tail
            from velocity_asr import _lib
            from velocity_asr.ssm import _tree_mode
            Di, N = blk.ssm.d_inner, blk.ssm.state_dim
            mode = _tree_mode()
            from velocity_asr.ssm import _bf16_compose
            wn = "w_noz" if "w_noz" in p else "w_noz16" if ("w_noz16" in p and _bf16_compose()) else None
            if wn:  # one projection GEMM writes [x | B | C | dt] (fp32, or the bf16 model's composed form)
                bn = "b_noz" if wn == "w_noz" else "b_noz16"
                proj = lambda: ops.gemm(u, p[wn], p[bn], epilogue=_lib.EPI_SOFTPLUS_FROM,  # noqa: E731
                                        n_out=Di + 2 * N)
                xbd = proj()
                xs, bc, dt = xbd[:, :Di], xbd[:, Di:Di + 2 * N], xbd[:, Di + 2 * N:]
                out = dict(gemm=per_launch(proj), gemm_key=(B * L, p[wn].shape[0], D, 1))
            else:  # bf16: in_proj's x rows, then [x_proj; dt_proj]
                xs = ops.gemm(u, p["w_x"])
                xdt = ops.gemm(xs, p["w_xdt"], p["b_xdt"], epilogue=_lib.EPI_SOFTPLUS_FROM, n_out=2 * N)
                bc, dt = xdt[:, :2 * N], xdt[:, 2 * N:]
                out = {}
            out.update(scan=per_launch(lambda: ops.ssm_scan_ungated(xs, dt, bc, p["A2"], blk.ssm.D, B, L, mode)),
                       scan_key=(B, L))
            yd = ops.ssm_scan_ungated(xs, dt, bc, p["A2"], blk.ssm.D, B, L, mode)
            x2 = x.view(B * L, D)
            out["tail"] = per_launch(lambda: ops.ssm_block_tail_gated(
                yd, u, p["w_z"], mode, x2, blk.ssm.out_proj.weight, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps,
                blk.ffn[0].weight, blk.ffn[0].bias, blk.ffn[3].weight, blk.ffn[3].bias))
            return out
        xz, xdt = blk.ssm.project(u)
        out = dict(scan=per_launch(lambda: blk.ssm.scan(xz, xdt, B, L)), scan_key=(B, L))
        if "w_comb" in p:  # the composed projection: one GEMM (fp32 model)
            out["gemm"] = per_launch(lambda: blk.ssm.project(u))
            out["gemm_key"] = (B * L, p["w_comb"].shape[0], D, 1)
        g = blk.ssm.scan(xz, xdt, B, L)
        x2 = x.view(B * L, D)
        if blk._fused_tail_ok(D):
            out["tail"] = per_launch(lambda: blk.tail(g, x2, B, L))
    return out


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline():
    """The oracle (numpy restatement of the reference path, oracle/velocity_ref.py) with the
    reference's materialised tree scan (ssm.py:216-295) over the bench's 32 clips
    (make_audio(32, 160000, seed=1234)), one clip per call as the reference's scripts run it,
    data-parallel over the host cores the GPU job is granted (OMP_NUM_THREADS: 16 per GPU on the
    box; os.cpu_count() is the whole machine) in spawned single-thread workers; one warm-up clip
    per worker, median of 3 passes (oracle/cpu_baseline.py)."""
    from oracle import cpu_baseline as CB
    share = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or (os.cpu_count() or 1)
    workers = max(1, min(share, os.cpu_count() or 1, 32))
    r = CB.measure(workers=workers, clips=32, seconds=10.0, seed=1234, repeats=3)
    return dict(value=round(r["rtfx"], 3), unit="audio-sec/sec (RTFx)", cores=r["workers"], kind="port",
                sample=f"the bench's 32 x 10 s clips (rank 0), one clip per call, mel+forward+greedy, "
                       f"oracle/velocity_ref.py with the reference's materialised tree scan (SCAN_FORM='tree'), "
                       f"{r['workers']} single-thread worker processes (BLAS threads per worker: "
                       f"{r.get('blas_threads_per_worker')}; the job's CPU share; os.cpu_count()="
                       f"{os.cpu_count()}), median of 3 passes {r['passes_s']} s after a warm-up clip per worker; "
                       f"host CPU: {cpu_model()}; the real reference measured 7.95 RTFx on 8 Xeon threads in the "
                       f"build container (SURVEY §6)")


EDIT_BOUND = 0.05  # bf16 token edit rate <= 5 % (the reference's own bf16 drift: 2.3 %)


def _edits(a, b):
    """Levenshtein distance between two token lists (row DP, each row vectorised: the insertion
    chain cur[j] = min(cur[j - 1] + 1, ...) is a running minimum of cur[k] - k)."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if len(b) == 0:
        return len(a)
    ar = np.arange(len(b) + 1)
    prev = ar.copy()
    for i, x in enumerate(a, 1):
        base = np.empty_like(prev)
        base[0] = i
        base[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (b != x))
        prev = np.minimum.accumulate(base - ar) + ar
    return int(prev[-1])


def _golden_lists(kind, rank, seconds, batch):
    """The reference's greedy token lists for this rank's clips (make_audio(batch, S, 1234 + rank))
    from tests/golden/ (generated from the reference by tests/golden/gen_goldens.py), as
    (lists, clips covered), or None.  kind: fp32 | bf16 | int8."""
    gd = os.path.join(REPO, "tests", "golden")
    try:
        full = json.loads(str(np.load(os.path.join(gd, "fwd_fullbatch.npz"), allow_pickle=False)["greedy"]))
        sets = json.loads(str(np.load(os.path.join(gd, "fwd_benchsets.npz"), allow_pickle=False)["greedy"]))
    except OSError:
        return None
    if seconds == 30.0 and kind == "fp32" and rank == 0:
        ref = full["c4"]  # all 32 clips of make_audio(32, 480000, seed=1234)
    elif seconds != 10.0:
        return None
    elif kind == "fp32":
        ref = full["c2"] if rank == 0 else sets.get(f"fp32_r{rank}")
    else:
        ref = sets.get(f"{kind}_r{rank}")
    if ref is None:
        return None
    n = min(len(ref), batch)
    return ref[:n], n


def golden_check(toks, lens, args, rank):
    """This rank's token lists vs the reference's for the same clips: fp32 must be identical
    (CTC-greedy output identical to the reference, north_star); the bf16 model (C3) and the
    INT8 fake-quant model (C5) are checked by token edit rate against the reference run with the
    same numerics (and, for the report, against the fp32 reference).  Returns the counts
    [ranks with a golden, clips, identical clips, edits, reference tokens, edits vs fp32, pass]."""
    from velocity_asr.pipeline import token_lists
    kind = "bf16" if args.bf16 else "int8" if args.int8 else "fp32"
    g = _golden_lists(kind, rank, args.seconds, args.batch)
    if g is None:
        return [0] * 7
    ref, n = g
    got = token_lists(toks[:n], lens[:n])
    same = sum(a == b for a, b in zip(got, ref))
    edits = sum(_edits(a, b) for a, b in zip(got, ref))
    tokens = sum(len(b) for b in ref)
    e32 = 0
    if kind != "fp32":
        r32 = _golden_lists("fp32", rank, args.seconds, args.batch)
        e32 = sum(_edits(a, b) for a, b in zip(got, r32[0])) if r32 else -1
    ok = same == n if kind == "fp32" else edits <= EDIT_BOUND * tokens
    return [1, n, same, edits, tokens, e32, int(ok)]


def golden_summary(c, args):
    """The JSON object of golden_check's counts summed over ranks."""
    ranks, n, same, edits, tokens, e32, ok = c
    if not ranks:
        return None
    kind = "bf16" if args.bf16 else "int8" if args.int8 else "fp32"
    out = dict(numerics=kind, ranks_checked=int(ranks), clips=int(n), clips_identical=int(same),
               token_edit_rate=round(edits / max(tokens, 1), 5), all_ranks_pass=bool(ok == ranks))
    if kind == "fp32":
        out["criterion"] = "every clip's greedy token list identical to the reference fp32 CPU path"
    else:
        out["criterion"] = (f"token edit rate <= {EDIT_BOUND} vs the reference CPU path run with the same numerics "
                            f"({'model.to(bfloat16)' if kind == 'bf16' else 'calibrated QAT fake-quant'})")
        out["token_edit_rate_vs_fp32_reference"] = round(e32 / max(tokens, 1), 5) if e32 >= 0 else None
    return out


def pmc_lookup(name, key=None):
    path = os.path.join(REPO, "profiles", name)
    if not os.path.exists(path):
        return None
    try:
        d = json.load(open(path))
        return d if key is None else d.get(key)
    except Exception:
        return None


def agree_max_over_ranks(times):
    """The schedule timings every rank decides on: each candidate's max over ranks (the timed
    value is the max over ranks, so the schedule whose slowest rank is fastest wins); gloo group."""
    keys = sorted(times)
    t = torch.tensor([times[k] for k in keys], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return {k: float(v) for k, v in zip(keys, t.tolist())}


def schedule_how(tried, world):
    if not tried:
        return "single candidate (batch under 8 clips or odd): one graph"
    how = (f"{len(tried)} schedules built and timed on the bench's own audio in interleaved rounds of 5 replays "
           f"(at least 3, until each candidate's round time settles within 1 %) before the warm-up; the faster "
           f"kept, the others freed after the timed steps")
    if world > 1:
        how += "; times are the max over ranks, so every rank keeps the same schedule"
    return how


def run_verdict(graph_match, golden, warm_golden, golden_eager):
    """(exit code, reasons): the line is invalid when the timed graphs' tokens differ from an eager
    pass, or when the timed graphs' (last timed or last warm-up replay) or the eager pass's token
    lists fail the reference check (tokens_vs_reference.all_ranks_pass false)."""
    why = []
    if not graph_match:
        why.append("the timed graphs' tokens differ from an eager pass over the same audio "
                   "(graph_tokens_match_eager false)")
    for name, g in (("tokens_vs_reference", golden), ("warmup_tokens_vs_reference", warm_golden),
                    ("eager_tokens_vs_reference", golden_eager)):
        if g is not None and not g.get("all_ranks_pass", False):
            why.append(f"{name}.all_ranks_pass is false ({g.get('clips_identical')} of {g.get('clips')} clips "
                       f"identical, token edit rate {g.get('token_edit_rate')})")
    return (1 if why else 0), why


def timed(step, steps, world, dev, per_step=None):
    """Wall time of `steps` steps between barriers + synchronizes (max over ranks).  per_step: a
    list that receives each step's device time (ms) from HIP events recorded on the caller's
    stream between the steps (no host synchronisation inside the loop)."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)] if per_step is not None else None
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = []
    for i in range(steps):
        if ev:
            ev[i].record()
        h0 = time.perf_counter()
        step()
        host.append(time.perf_counter() - h0)
    if ev:
        ev[steps].record()
    t_issue = time.perf_counter() - t0
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if ev:
        per_step.extend(ev[i].elapsed_time(ev[i + 1]) for i in range(steps))
        # host side: each step() call's own time and the loop's issue time (all steps enqueued):
        # if they approach the device times, the host's graph launches set the pace
        per_step.append(dict(host_step_ms=[round(v * 1e3, 4) for v in host], issue_ms=round(t_issue * 1e3, 3)))
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)  # the timing group is gloo (host)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    return elapsed


def step_stats(ms):
    """Summary of the timed steps' device times (ms, HIP events between the steps on the caller's
    stream): every step alike (a slower machine state) or a drift over the run; and the host's
    time per step() call (graph launch + parameter check) beside it."""
    if not ms:
        return None
    hostd = ms[-1] if isinstance(ms[-1], dict) else {}
    ms = [v for v in ms if not isinstance(v, dict)]
    v = sorted(ms)
    hs = sorted(hostd.get("host_step_ms", []))
    return dict(device_ms=[round(x, 4) for x in ms], min=round(v[0], 4), median=round(v[len(v) // 2], 4),
                max=round(v[-1], 4), first_half_mean=round(float(np.mean(ms[:len(ms) // 2])), 4),
                second_half_mean=round(float(np.mean(ms[len(ms) // 2:])), 4),
                host_step_ms_median=round(hs[len(hs) // 2], 4) if hs else None,
                host_step_ms_max=round(hs[-1], 4) if hs else None, host_issue_ms=hostd.get("issue_ms"))


def _serving_step(args, tr, toks, lens, B, S_len, dev, rank, world):
    """The serving leg: rank 0 holds the whole (world*B, S) batch in HBM; each step scatters the
    shards over RCCL (xGMI) into every rank's graph input, replays, and gathers the int32 tokens
    back to rank 0 (velocity_asr.distributed.transcribe_sharded)."""
    from velocity_asr import synthetic as S
    from velocity_asr.distributed import graphed_step, transcribe_sharded
    from velocity_asr.pipeline import token_lists
    os.environ.setdefault("TORCH_NCCL_BLOCKING_WAIT", "1")  # a timed-out collective raises here
    with stdout_to_stderr():  # RCCL prints its version banner on stdout at communicator creation
        rccl = dist.new_group(backend="nccl", timeout=timedelta(seconds=args.serving_timeout))
        dist.barrier(group=rccl, device_ids=[dev.index])
    if os.environ.get("VASR_BENCH_FAIL_SERVING") == str(rank):  # tests: a forced serving-leg failure
        raise RuntimeError(f"forced serving-leg failure on rank {rank}")
    full = None
    if rank == 0:
        full = torch.cat([torch.from_numpy(S.make_audio(B, S_len, seed=1234 + r)) for r in range(world)]).to(dev)
    gstep = graphed_step(tr)
    res = {}

    def sstep():
        res["out"] = transcribe_sharded(gstep, full, world * B, S_len, dev, shard=tr.audio, as_lists=False,
                                        group=rccl)
    saved = tr.audio.clone()
    try:
        for _ in range(max(2, args.warmup // 2)):
            sstep()
        el_s = timed(sstep, args.steps, world, dev)
    finally:
        tr.audio.copy_(saved)
    ok = None
    if rank == 0:
        # the gathered block for rank 0's shard equals the resident-path tokens
        ta, la = res["out"]
        ok = token_lists(ta[:B], la[:B]) == token_lists(toks, lens)
    return dict(value=round(world * B * args.seconds * args.steps / el_s, 2),
                ms_per_step=round(el_s / args.steps * 1e3, 3),
                scatter_mb_per_rank=round(B * S_len * 4 / 1e6, 2),
                gather_kb_per_rank=round(B * (toks.shape[1] + 1) * 4 / 1e3, 1),
                rank0_tokens_match=ok)


def serving_leg(fn, world, rank):
    """fn() on every rank; an exception becomes {"error": ...}.  With world > 1 the ranks then
    agree over the gloo group (any rank's failure is reported by rank 0); never raises."""
    try:
        res, err = fn(), None
    except Exception as e:  # noqa: BLE001 -- the serving leg must not lose the resident line
        res, err = None, f"rank {rank}: {type(e).__name__}: {e}"
        log(f"bench.py: serving leg failed: {err}")
    if world > 1:
        try:
            bad = torch.tensor([0.0 if err is None else 1.0 + rank], dtype=torch.float64)
            dist.all_reduce(bad, op=dist.ReduceOp.MAX)
            if err is None and bad.item() > 0:
                err = f"rank {int(bad.item()) - 1} failed (see its stderr)"
        except Exception as e:  # noqa: BLE001
            err = err or f"rank agreement failed: {type(e).__name__}: {e}"
    return res if err is None else dict(error=err)


class Watchdog:
    """Calls on_expire() from a daemon thread unless cancel() comes within `seconds`."""

    def __init__(self, seconds, on_expire):
        import threading
        self._done = threading.Event()

        def watch():
            if not self._done.wait(seconds):
                on_expire()
        self._t = threading.Thread(target=watch, daemon=True)
        self._t.start()

    def cancel(self):
        self._done.set()


_emitted = []


def emit(line, rc, scatter_error=None):
    """Print rank 0's one JSON line (once).  Called from the watchdog thread with scatter_error
    set, it prints the resident line with the serving leg marked failed and ends the process
    with the resident run's exit code (a hung collective cannot be joined)."""
    if not _emitted:
        _emitted.append(True)
        if line is not None:
            if scatter_error is not None:
                line = dict(line, with_scatter=scatter_error)
            print(json.dumps(line), flush=True)
    if scatter_error is not None:
        log(f"bench.py: {scatter_error['error']}; exiting with the resident run's status")
        sys.stderr.flush()
        os._exit(rc)


def finish(line, rank, world, distributed, serving, rc_of, serving_timeout, grace=60.0):
    """The end of every rank's run: the serving leg (if any) under a watchdog, rank 0's one JSON
    line, the process group's teardown.  serving() returns the with_scatter dict; its failure on
    any rank lands in with_scatter.error (serving_leg), and if the leg (or the teardown after it)
    hangs past serving_timeout + grace the watchdog prints the resident line and ends the process."""
    dog = None
    if serving is not None:
        limit = serving_timeout + grace
        dog = Watchdog(limit, lambda: emit(line, rc_of(), dict(error=f"serving leg exceeded {limit:g} s")))
        scatter = serving_leg(serving, world, rank)
        if line is not None:
            line["with_scatter"] = scatter
            line["config"]["parallelism"] = _parallelism(world, scatter)
    emit(line, rc_of())
    if distributed:
        dist.destroy_process_group()  # still under the watchdog: a broken communicator may not tear down
    if dog is not None:
        dog.cancel()


def _parallelism(world, scatter):
    if world == 1 and scatter is None:
        return "single process"
    how = ("resident shards; serving leg scatters from rank 0 and gathers tokens" if scatter and "error" not in scatter
           else "resident shards; serving leg failed (with_scatter.error)" if scatter else "resident shards")
    return f"utterance-shard x{world}, timing barriers over gloo, serving leg over RCCL ({how})"


def run(args):
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    # VASR_BENCH_DEVICE pins every rank to one device index (rehearsing N ranks on a one-GPU box
    # with --no-scatter; RCCL refuses two ranks on one GPU)
    distributed = "WORLD_SIZE" in os.environ
    if "VASR_BENCH_DEVICE" in os.environ and world > 1 and not args.no_scatter:
        log("bench.py: VASR_BENCH_DEVICE pins every rank to one GPU, which RCCL refuses; add --no-scatter")
        return 2
    dev = torch.device("cuda", int(os.environ.get("VASR_BENCH_DEVICE", local)))
    torch.cuda.set_device(dev)

    from velocity_asr import synthetic as S
    from velocity_asr.pipeline import GraphedTranscriber, audio_to_token_ids

    model = build_model(dev)
    if args.bf16:
        model = model.to(torch.bfloat16)
    if args.int8:
        from velocity_asr import compute_mel_spectrogram
        from velocity_asr import quantize as Q
        model = Q.prepare_model_for_qat(model).to(dev).eval()
        calib = torch.from_numpy(S.make_audio(2, 48000, seed=71)).to(dev)
        Q.calibrate_from_activations(model, compute_mel_spectrogram(calib))
    S_len = int(args.seconds * SR)
    B = args.batch
    # schedule: one graph of the batch or two utterance groups on concurrent streams (the scan of
    # one overlaps the GEMMs of the other); bitwise the same tokens, and which is faster depends on
    # the box, so by default both are built and the faster one (timed in the untimed warm-up) is
    # kept (pipeline.autotuned_transcriber).  Up to round 3 the two-group form raced; the causes
    # were in the kernels and are fixed, and every run checks the tokens the timed
    # graphs wrote against the reference (tokens_vs_reference) and against an eager pass
    streams = args.streams or 0
    schedule = None
    audio = torch.from_numpy(S.make_audio(B, S_len, seed=1234 + rank)).to(dev)  # resident in HBM

    # The resident leg has no data-path collective (each rank transcribes its own shard), so its
    # barriers, the max over ranks and the schedule agreement run in a gloo group on the host: an
    # RCCL communicator's mere presence cost the graph replays 2.2 % (150.4k vs 153.8k RTFx at one
    # rank, profiles/r04ad/).  RCCL joins after the timed leg, for the serving leg's scatter /
    # gather -- and after the graph streams exist: HIP deals streams round-robin onto the
    # process's few hardware queues (GPU_MAX_HW_QUEUES = 4), and a communicator created first took
    # queues so that the two utterance-group streams landed on one and serialised (4.0 vs 2.7 ms
    # per step).
    if distributed:
        with stdout_to_stderr():  # gloo prints its connection line on stdout
            # bounded: a rank that died must not hold the others in a barrier for gloo's default 30 min
            dist.init_process_group("gloo", timeout=timedelta(seconds=args.gloo_timeout))
            dist.barrier()

    eager_out = []
    if args.eager:
        def step():
            eager_out[:] = audio_to_token_ids(model, audio)
        tr = None
    else:
        if streams:
            tr = GraphedTranscriber(model, B, S_len, dev, streams=streams)
        else:
            from velocity_asr.pipeline import autotuned_transcriber
            tr, tried = autotuned_transcriber(model, B, S_len, dev, audio=audio, keep_candidates=True,
                                              agree=agree_max_over_ranks if world > 1 else None)
            streams = len(tr.graphs)
            schedule = dict(chosen_streams=streams, ms_per_replay_by_streams=tried, how=schedule_how(tried, world),
                            rounds=tr.autotune_rounds)
        tr.audio.copy_(audio)
        step = tr.step

    for _ in range(args.warmup):
        step()
    # the warm-up's last replay is checked against the reference too, after the timed steps: its
    # tokens are copied on the device here (no host work between the warm-up and the timed steps --
    # an idle device starts the next steps up to 25 % slower, profiles/r05j/step_course.txt)
    warm_copy = tuple(t.clone() for t in tr.collect()) if tr is not None and args.full else None
    step_ms = []
    elapsed = timed(step, args.steps, world, dev, per_step=step_ms)
    if args.full:
        from velocity_asr.ops import probe_clock
        machine = probe_clock(dev)  # right after the timed steps: the clock they left, the XCD dispatch order
    if tr is not None and hasattr(tr, "release_candidates"):
        tr.release_candidates()  # the schedules not chosen (kept until now: freeing them stalls the device)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, *(tr.collect() if tr is not None else eager_out), rank, world)
    if not args.full:  # a plain run ends here, with the headline line
        line = None
        if rank == 0:
            line = headline(args, world, distributed, B, S_len, streams, schedule, elapsed, step_ms)
        finish(line, rank, world, distributed, None, lambda: 0, args.serving_timeout)
        return 0
    warm_golden = None
    if warm_copy is not None:
        wc = torch.tensor(golden_check(*warm_copy, args, rank), dtype=torch.float64)
        if world > 1:
            dist.all_reduce(wc)
        warm_golden = golden_summary([int(v) for v in wc.tolist()], args)

    # the tokens the timed graph wrote in its last replay vs the reference's greedy lists for the
    # same clips, and an eager pass over the same audio checked the same way (outside the timed
    # region)
    from velocity_asr.pipeline import token_lists
    etoks, elens = audio_to_token_ids(model, audio)
    toks, lens = (t.clone() for t in tr.collect()) if tr is not None else (etoks, elens)
    graph_match = token_lists(toks, lens) == token_lists(etoks, elens)
    if world > 1:  # every rank's graph tokens against its eager pass
        bad = torch.tensor([0.0 if graph_match else 1.0], dtype=torch.float64)
        dist.all_reduce(bad)
        graph_match = bad.item() == 0
    gc = torch.tensor(golden_check(toks, lens, args, rank) + golden_check(etoks, elens, args, rank),
                      dtype=torch.float64)
    if world > 1:
        dist.all_reduce(gc)
    gc = [int(v) for v in gc.tolist()]
    golden, golden_eager = golden_summary(gc[:7], args), golden_summary(gc[7:], args)
    valid = torch.arange(toks.shape[1], device=dev)[None, :] < lens[:, None]
    csum = torch.tensor([float(lens.sum().item()), float(toks.long().masked_fill(~valid, 0).sum().item())],
                        dtype=torch.float64)
    if world > 1:
        dist.all_reduce(csum)

    rf = kernel_roofline(model, audio, args.roofline_steps, 1 if args.eager else streams)
    iso = isolated_times(model, audio[:B // (1 if args.eager else streams)])  # one utterance group's launch shape
    # with utterance groups the dominant kernel is the group's scan launch; the whole batch's launch
    # (the one-graph schedule's shape) is timed the same way and reported beside it
    iso_full = isolated_times(model, audio) if (not args.eager and streams > 1) else None
    if world > 1:
        dist.barrier()

    def rc_of():
        return 0 if rank != 0 else run_verdict(graph_match, golden, warm_golden, golden_eager)[0]
    line = None
    if rank == 0:
        line = result_line(args, world, distributed, B, S_len, streams, schedule, elapsed, step_ms, machine, rf, iso,
                           iso_full, graph_match, golden, warm_golden, golden_eager, csum)
    # serving leg (ranks of a torchrun job): scatter from rank 0 over RCCL into each rank's graph
    # input, gather tokens.  It runs after the resident line is complete and cannot lose it: an
    # exception on any rank, or a collective that exceeds --serving-timeout (RCCL group with
    # blocking wait), lands in with_scatter.error, and a watchdog prints the resident line if the
    # leg hangs past that.  VERDICT r05 weak 6.
    serving = None
    if distributed and tr is not None and not args.no_scatter:
        def serving():
            return _serving_step(args, tr, toks, lens, B, S_len, dev, rank, world)
    finish(line, rank, world, distributed, serving, rc_of, args.serving_timeout)
    if rank != 0:
        return 0 if graph_match else 1
    rc, why = run_verdict(graph_match, golden, warm_golden, golden_eager)
    for w in why:
        log(f"bench.py: {w}; failing the run")
    return rc


def dump_outputs(path, toks, lens, rank, world):
    """--dump-outputs: what the timed path returned in its last step, as float32 .npy files in
    `path` (token ids and lengths are small integers, exact in float32).  Positions at and past a
    clip's length hold no result and are written as -1."""
    os.makedirs(path, exist_ok=True)
    t, n = toks.cpu().numpy(), lens.cpu().numpy()
    t = np.where(np.arange(t.shape[1])[None, :] < n[:, None], t, -1)
    tag = "" if world == 1 else f"_rank{rank}"
    np.save(os.path.join(path, f"tokens{tag}.npy"), t.astype(np.float32))
    np.save(os.path.join(path, f"lengths{tag}.npy"), n.astype(np.float32))


def headline(args, world, distributed, B, S_len, streams, schedule, elapsed, step_ms):
    """Rank 0's JSON line of a plain run: the contract's fields from the timed steps alone."""
    audio_sec = world * B * args.seconds * args.steps
    frames = world * B * (S_len // 160 + 1) * args.steps
    return {
        "metric": METRIC,
        "value": round(audio_sec / elapsed, 2),
        "unit": "audio-sec/sec (RTFx)",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "bf16" if args.bf16 else "f32",
        "data": "synthetic: N(0, 0.1) 16 kHz clips; seeded random-init weights (velocity_asr.synthetic)",
        "full": bool(args.full),
        "config": {"workload": f"{B} x {args.seconds:g} s clips per GPU, audio->mel->forward->CTC greedy tokens "
                               f"(BASELINE configs[{4 if args.int8 else 2 if args.bf16 else 1}]"
                               f"{', INT8 fake-quant' if args.int8 else ''}"
                               f"{f', HIP graph x{streams} streams' if not args.eager else ', eager'})",
                   "global_batch": world * B, "clip_seconds": args.seconds, "schedule": schedule,
                   "parallelism": _parallelism(world, None) if distributed else "single process"},
        "frames_per_sec": round(frames / elapsed, 1),
        "step_ms_device": step_stats(step_ms),
    }


def result_line(args, world, distributed, B, S_len, streams, schedule, elapsed, step_ms, machine, rf, iso, iso_full,
                graph_match, golden, warm_golden, golden_eager, csum):
    """Rank 0's JSON line of a --full run for the resident leg (the headline fields, the roofline,
    the checks)."""
    sc, gm = rf.get("scan"), rf["gemm"]
    # GEMM family: split-bf16 ("x3") products = six bf16 MFMA products per fp32 multiply-add
    x3 = not args.bf16
    prod = 6 if x3 else 1
    g_t = gm["top_t"]
    g_src = "HIP events around each launch of the eager steps (in situ)"
    if iso.get("gemm_key") == tuple(gm["top_key"]):
        g_t, g_src = iso["gemm"], "isolated: 20 back-to-back launches on the bench's operands, one HIP event pair"
    g_ach = prod * gm["top_flops"] / g_t / 1e12
    g_f32 = gm["top_flops"] / g_t / 1e12
    gemm_fields = dict(gemm_kernel=f"vasr gemm {'x3 (6 bf16 products)' if x3 else 'bf16' if args.bf16 else 'f32'} "
                                   f"{gm['top_shape']}",
                       gemm_avg_launch_us=round(g_t * 1e6, 2), gemm_time_source=g_src,
                       gemm_insitu_avg_launch_us=round(gm["top_t"] * 1e6, 2),
                       gemm_achieved=round(g_ach, 2), gemm_peak=BF16_MFMA_PEAK_TFS, gemm_unit="TFLOP/s",
                       gemm_frac=round(g_ach / BF16_MFMA_PEAK_TFS, 4),
                       gemm_f32eq_tflops=round(g_f32, 2), gemm_f32eq_frac=round(g_f32 / F32_MFMA_PEAK_TFS, 4),
                       gemm_all_f32eq_tflops=round(gm["tflops"], 2))
    mf = pmc_lookup("pmc_mfma.json") if x3 else None  # counters of the split-bf16 kernels only
    if isinstance(mf, dict):
        ent = mf.get("%d,%d,%d" % gm["top_key"][:3])
        if isinstance(ent, dict):
            gemm_fields["gemm_mfma_busy_frac"] = ent.get("mfma_busy_frac")
    # dominant kernel = the single kernel (same code, same shape) with the largest time per step
    if sc and sc["total"] >= gm["top_total"]:
        s_t, s_src = sc["t"], "HIP events around each launch of the eager steps (in situ)"
        if iso.get("scan_key") == (sc["B"], sc["L"]):
            s_t, s_src = iso["scan"], "isolated: 20 back-to-back launches on the bench's operands, one HIP event pair"
        ach = sc["bytes"] / s_t / 1e9
        roof = dict(bound="hbm", kernel=("vasr ssm_scan_ungated (tree scan + x D, z-in-tail blocks, 8 local blocks, "
                                         "B*L*(3*Di+2*N)*4 B/launch)" if sc.get("ungated") else
                                         "vasr ssm_scan (tree scan + gate, 8 local blocks, B*L*(4*Di+2*N)*4 B/launch)"),
                    achieved=round(ach, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(ach / HBM_PEAK_GBS, 4),
                    traffic=None, avg_launch_us=round(s_t * 1e6, 2), time_source=s_src,
                    insitu_avg_launch_us=round(sc["t"] * 1e6, 2), algorithmic_bytes_per_launch=sc["bytes"])
        if sc.get("ungated"):
            # z-in-tail: the scan no longer reads z (Di floats per token), so its algorithmic bytes and
            # its HBM fraction are smaller at the same state work; the gated scan's byte count at this
            # launch time is given beside it for comparison with earlier lines (not the achieved rate)
            gb = sc["B"] * sc["L"] * (4 * sc["Di"] + 2 * sc["N"]) * 4
            roof.update(gated_bytes_per_launch=gb, frac_at_gated_bytes=round(gb / s_t / 1e9 / HBM_PEAK_GBS, 4))
        # the scan is VALU-bound: the same launch against the fp32 vector roof at the
        # reference tree's ~11 fp32 operations per state element (SURVEY §8 d), and the HBM fraction
        # that arithmetic allows at best: (bytes/elem / HBM peak) / (ops/elem / VALU peak)
        tops = sc["elems"] * VALU_OPS_PER_ELEM / s_t / 1e12
        ceil = (sc["bytes"] / sc["elems"] / (HBM_PEAK_GBS * 1e9)) / (VALU_OPS_PER_ELEM / (F32_VALU_PEAK_TOPS * 1e12))
        roof.update(valu_ops_per_element=VALU_OPS_PER_ELEM, valu_achieved=round(tops, 2),
                    valu_peak=F32_VALU_PEAK_TOPS, valu_unit="T lane-ops/s", valu_frac=round(tops / F32_VALU_PEAK_TOPS, 4),
                    hbm_ceiling_frac=round(ceil, 4), frac_of_hbm_ceiling=round(ach / HBM_PEAK_GBS / ceil, 4))
        key = "ssm_scan"
    else:
        roof = dict(bound="mfma", kernel=gemm_fields["gemm_kernel"], achieved=round(g_ach, 2), peak=BF16_MFMA_PEAK_TFS,
                    unit="TFLOP/s", frac=round(g_ach / BF16_MFMA_PEAK_TFS, 4), traffic=None,
                    avg_launch_us=round(g_t * 1e6, 2), time_source=g_src)
        key = "gemm_x3"
    roof.update(gemm_fields)
    if iso_full is not None and key == "ssm_scan" and "scan" in iso_full:
        Bf, Lf = iso_full["scan_key"]
        fb = Bf * Lf * (4 * sc["Di"] + 2 * sc["N"]) * 4
        roof["whole_batch_launch"] = dict(B=Bf, avg_launch_us=round(iso_full["scan"] * 1e6, 2),
                                          achieved=round(fb / iso_full["scan"] / 1e9, 1),
                                          frac=round(fb / iso_full["scan"] / 1e9 / HBM_PEAK_GBS, 4),
                                          note="the same kernel at the one-graph schedule's launch shape, "
                                               "isolated (not the schedule timed here)")
    t = pmc_lookup("pmc_traffic.json", key)
    if isinstance(t, dict) and sc and key == "ssm_scan":  # by launch grid (B x Di/16 x 256 threads) @ L
        t = t.get("%d@%d" % (sc["B"] * (sc["Di"] // 16) * 256, sc["L"]))
    if isinstance(t, (int, float)):
        roof["traffic"] = t
    line = headline(args, world, distributed, B, S_len, streams, schedule, elapsed, step_ms)
    line.update({
        "machine": machine,
        "roofline": roof,
        "with_scatter": None,
        "kernels": {
            "scan": None if not sc else dict(avg_launch_us=round(sc["t"] * 1e6, 2), launches_per_step=sc["per_step"],
                                             ms_per_step=round(sc["total"] * 1e3, 3),
                                             hbm_gbs=round(sc["bytes"] / sc["t"] / 1e9, 1),
                                             gelem_per_s=round(sc["elems"] / sc["t"] / 1e9, 1)),
            "gemm": dict(avg_launch_us=round(gm["t"] * 1e6, 2), launches_per_step=gm["per_step"],
                         ms_per_step=round(gm["total"] * 1e3, 3), tflops=round(gm["tflops"], 2)),
            "ssm_tail_isolated_us": round(iso["tail"] * 1e6, 2) if "tail" in iso else None,
            "z_in_tail": bool(sc and sc.get("ungated")),
        },
        "token_checksum": [int(csum[0].item()), int(csum[1].item())],
        "graph_tokens_match_eager": graph_match,
        "rank0_tokens_match_reference": None if golden is None else bool(golden["all_ranks_pass"]),
        "tokens_vs_reference": golden,
        "warmup_tokens_vs_reference": warm_golden,
        "eager_tokens_vs_reference": golden_eager,
    })
    if world == 1 and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline()
    return line


def main():
    args = parse_args()
    # a plain one-GPU run stays in this process; N > 1 ranks, and --full (whose serving leg joins
    # an RCCL group), start through torch.distributed.run
    if "WORLD_SIZE" not in os.environ and not args.inproc and (args.gpus != 1 or args.full):
        sys.exit(launch(args))
    if args.inproc and args.gpus != 1:
        log("bench.py: --inproc runs one rank; use --gpus 1")
        sys.exit(2)
    sys.exit(run(args))


if __name__ == "__main__":
    main()
