"""Times the long-form segmenter on one machine:
  (a) plan + gather on the device for 1 x 600 s and 8 x 600 s recordings at 16 kHz that are already
      there: the kernels by device events (block energy + plan, then gather), and the wall time of
      audio.plan_segments + audio.segment_on_device, which includes the one small device->host copy
      of the cut table and ends in a synchronise; median of 20 after 3 warm-ups;
  (b) the host rule on the same audio, as a caller without the kernels would run it: the device->host
      copy of the recordings, then audio.plan_segments_host per recording; wall, median of 5 after 1;
  (c) transcribe_files end to end on one 10-minute 44.1 kHz stereo float32 WAV with
      segment_seconds=30 (default model, synthetic weights): wall per call, median of 5 after 1.
    python tools/longform_time.py [--seconds 600] [--out profiles/longform]
writes <out>.json and <out>.md."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "velocity-asr_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import velocity_asr as va  # noqa: E402
from velocity_asr import _lib as L, audio, ops, synthetic as S  # noqa: E402
from velocity_asr.transcription import transcribe_files  # noqa: E402

M, m = 30 * 16000, 10 * 16000


def recordings(B, seconds):
    """Noise under a slow envelope with a short pause every ~7 s: quiet points exist, as in speech."""
    n = seconds * 16000
    x = S.make_audio(B, n, seed=600 + B)
    t = np.arange(n, dtype=np.float32) / 16000
    for b in range(B):
        x[b] *= (0.55 + 0.45 * np.sin(2 * np.pi * t / (7.0 + 0.3 * b))).astype(np.float32)
    return x


def events(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return ts


def wall(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def spread(ts, nd=1):
    return dict(median=round(statistics.median(ts), nd), min=round(min(ts), nd), max=round(max(ts), nd))


def plan_gather(B, seconds, dev):
    x = recordings(B, seconds)
    n = x.shape[1]
    xd = torch.from_numpy(x).to(dev)
    ns = [n] * B
    cuts = audio.plan_segments(xd, ns, max_samples=M, min_samples=m)
    table = torch.tensor(audio.segment_table(ns, cuts), dtype=torch.int64).to(dev)
    S_seg = int(table[:, 2].max())
    k_plan = events(lambda: ops.segment_plan(ops.block_energy(xd), n, M, m, 10))
    k_energy = events(lambda: ops.block_energy(xd))
    k_gather = events(lambda: ops.segment_gather(xd, table, S_seg))

    def device_path():
        c = audio.plan_segments(xd, ns, max_samples=M, min_samples=m)
        return audio.segment_on_device(xd, ns, c)

    def host_path():
        h = xd.cpu().numpy()
        return [audio.plan_segments_host(h[b], M, m) for b in range(B)]

    w_dev = wall(device_path, 20, 3)
    w_host = wall(host_path, 5, 1)
    w_copy = wall(lambda: xd.cpu(), 5, 1)
    same = host_path() == cuts
    e_us = statistics.median(k_energy)
    return dict(recordings=B, seconds=seconds, samples_each=n, segments=int(table.shape[0]), longest_segment=S_seg,
                cuts_equal_host=bool(same), energy_us=spread(k_energy), energy_plan_us=spread(k_plan),
                gather_us=spread(k_gather), energy_read_gb_per_s=round(4.0 * B * n / e_us / 1e3, 1),
                gather_gb_per_s=round(8.0 * B * n / statistics.median(k_gather) / 1e3, 1),
                device_plan_gather_wall_ms=spread(w_dev, 3), host_copy_plan_wall_ms=spread(w_host, 1),
                host_copy_alone_wall_ms=spread(w_copy, 1),
                host_over_device=round(statistics.median(w_host) / statistics.median(w_dev), 1))


def end_to_end(seconds, dev):
    W = S.make_weights(None, seed=0)
    model = va.VELOCITYASR()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    model = model.to(dev).eval()
    dec = va.CTCDecoder(va.create_default_vocabulary(model.config.vocab_size))
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "long.wav")
        n = 44100 * seconds
        x = S.make_audio(2, n, seed=77)
        x *= (0.55 + 0.45 * np.sin(2 * np.pi * np.arange(n, dtype=np.float32) / (44100 * 7.0))).astype(np.float32)
        audio.write_wav(p, x, 44100)
        out = []

        def run():
            out[:] = transcribe_files(model, [p], dec, dev, timestamps=True, segment_seconds=30)

        ts = wall(run, 5, 1)
        t_read = wall(lambda: audio.read_audio(p), 3, 1)
    r = out[0]
    return dict(file=f"{seconds} s 44.1 kHz stereo float32 WAV", segment_seconds=30, error=r.get("error"),
                duration=r.get("duration"), words=len(r.get("words", [])), wall_ms=spread(ts, 1),
                of_which_read_wav_ms=spread(t_read, 1),
                audio_seconds_per_second=round(seconds / (statistics.median(ts) / 1e3), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--out", default="profiles/longform")
    a = ap.parse_args()
    L.require_device()
    dev = torch.device("cuda", 0)
    out = dict(device=torch.cuda.get_device_name(0), max_samples=M, min_samples=m, window_blocks=10,
               plan_gather=[plan_gather(B, a.seconds, dev) for B in (1, 8)], transcribe_files=end_to_end(a.seconds, dev))
    with open(a.out + ".json", "w") as f:
        json.dump(out, f, indent=1)
    md = ["# Long-form segmenter: device plan + gather against the host rule", "",
          f"tools/longform_time.py on {out['device']}: recordings of {a.seconds} s at 16 kHz already on the device, segments of "
          "10 to 30 s, window 10 blocks.  Kernels: device events, median of 20 after 3 warm-ups (min - max).  Device wall: "
          "audio.plan_segments + audio.segment_on_device, the cut-table copy and a final synchronise included, median of 20.  "
          "Host wall: the recordings copied to the host, then audio.plan_segments_host on each (numpy), median of 5.", "",
          "| recordings | segments | energy us | energy + plan us | gather us | energy read GB/s | gather GB/s (read + write) | "
          "device wall ms | host copy + plan wall ms | of which the copy ms | host / device | same cuts |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|"]

    def cell(s):
        return f"{s['median']} ({s['min']} - {s['max']})"

    for r in out["plan_gather"]:
        md.append(f"| {r['recordings']} x {r['seconds']} s | {r['segments']} | {cell(r['energy_us'])} | "
                  f"{cell(r['energy_plan_us'])} | {cell(r['gather_us'])} | {r['energy_read_gb_per_s']} | {r['gather_gb_per_s']} | "
                  f"{cell(r['device_plan_gather_wall_ms'])} | {cell(r['host_copy_plan_wall_ms'])} | "
                  f"{cell(r['host_copy_alone_wall_ms'])} | {r['host_over_device']} | {r['cuts_equal_host']} |")
    beats = all(r["host_over_device"] > 1.0 for r in out["plan_gather"])
    md += ["", "The device planner " + ("beats" if beats else "does NOT beat") + " host copy + plan at these shapes "
           "(the host figure plans only; it would still have to cut the segments and upload them)."]
    t = out["transcribe_files"]
    md += ["", f"transcribe_files on one file ({t['file']}), segment_seconds=30, timestamps, batch_size 16, default model with "
           f"synthetic weights: {cell(t['wall_ms'])} ms wall per call (median of 5 after 1), of which reading the WAV on the "
           f"host takes {cell(t['of_which_read_wav_ms'])} ms; {t['audio_seconds_per_second']} audio seconds per second; "
           f"duration {t['duration']}, {t['words']} words, error {t['error']}."]
    with open(a.out + ".md", "w") as f:
        f.write("\n".join(md) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
