"""Times the device resampler against the host one it replaces, on one machine:
  (a) the vasr_resample_mix_f32 launch by device events, median of 20 after 3 warm-ups, for 32 clips
      x 10 s of 44.1 kHz stereo, 48 kHz mono and 8 kHz mono (-> 16 kHz);
  (b) the wall time of the host audio.resample on ONE such clip of each kind (stereo: after the
      host downmix, which is not timed);
  (c) transcribe_files over 32 synthetic 10 s 44.1 kHz stereo WAVs with VASR_DEVICE_RESAMPLE=1 and =0,
      alternating for four pairs (wall time per call, files on local disk, default model with
      synthetic weights, batch_size 32), after one untimed call of each.
--step-ms: the model's own step for the same 32 clips (bench.py's ms_per_step on this machine); the
report then says whether (a) at 44.1 kHz stays under a tenth of it.
    python tools/resample_ab.py [--step-ms 1.92] [--out profiles/resample]
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

CLIPS, SECONDS = 32, 10
KINDS = [("44.1 kHz stereo", 44100, 2), ("48 kHz mono", 48000, 1), ("8 kHz mono", 8000, 1)]


def launch_us(sr, ch, dev):
    n = sr * SECONDS
    x = torch.from_numpy(np.stack([S.make_audio(ch, n, seed=sr + b) for b in range(CLIPS)])).to(dev)
    tb = audio._resample_table(sr, 16000, x.device)
    fn = lambda: ops.resample_mix(x, tb.taps, tb.orig, tb.nw, tb.width)  # noqa: E731
    for _ in range(3):
        y = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    # one clip through the host path: the same bits, and its wall time
    m = x[0].cpu()
    m = (m[0] + m[1]) / 2 if ch == 2 else m[0]
    t0 = time.perf_counter()
    want = audio.resample(m, sr, 16000)
    host_ms = (time.perf_counter() - t0) * 1e3
    macs = CLIPS * y.shape[1] * tb.klen
    return dict(rate=sr, channels=ch, clips=CLIPS, seconds=SECONDS, taps_per_output=tb.klen, tap_rows=tb.nw,
                tile_outputs=tb.tile_outputs, device_us_median=round(statistics.median(ts), 1),
                device_us_min=round(min(ts), 1), device_us_max=round(max(ts), 1),
                gmac_per_s=round(macs / statistics.median(ts) / 1e3, 1),
                host_ms_one_clip=round(host_ms, 2), host_ms_32_clips=round(host_ms * CLIPS, 1),
                host_over_device=round(host_ms * CLIPS * 1e3 / statistics.median(ts), 1),
                bit_identical=bool(torch.equal(y[0].cpu(), want)))


def file_ab(dev, pairs=4):
    W = S.make_weights(None, seed=0)
    model = va.VELOCITYASR()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    model = model.to(dev).eval()
    dec = va.CTCDecoder(va.create_default_vocabulary(model.config.vocab_size))
    rows = []
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i in range(CLIPS):
            p = os.path.join(d, f"c{i:02d}.wav")
            audio.write_wav(p, S.make_audio(2, 44100 * SECONDS, seed=500 + i), 44100)
            paths.append(p)

        def run(flag):
            os.environ["VASR_DEVICE_RESAMPLE"] = flag
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = transcribe_files(model, paths, dec, dev, batch_size=CLIPS)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, r

        _, r1 = run("1")
        _, r0 = run("0")
        same = r1 == r0 and all("error" not in r for r in r1)
        for _ in range(pairs):
            t1, _ = run("1")
            t0, _ = run("0")
            rows.append(dict(device_ms=round(t1, 1), host_ms=round(t0, 1), host_over_device=round(t0 / t1, 2)))
        os.environ.pop("VASR_DEVICE_RESAMPLE", None)
    return dict(files=CLIPS, kind="10 s 44.1 kHz stereo float32 WAV", batch_size=CLIPS, results_identical=same, pairs=rows,
                device_never_slower=all(r["device_ms"] <= r["host_ms"] for r in rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step-ms", type=float, default=None, help="bench.py ms_per_step on this machine (32 x 10 s)")
    ap.add_argument("--out", default="profiles/resample")
    ap.add_argument("--skip-files", action="store_true", help="skip leg (c)")
    a = ap.parse_args()
    L.require_device()
    dev = torch.device("cuda", 0)
    out = dict(device=torch.cuda.get_device_name(0), launches=[dict(kind=k, **launch_us(sr, ch, dev)) for k, sr, ch in KINDS])
    if not a.skip_files:
        out["transcribe_files"] = file_ab(dev)
    if a.step_ms:
        us = out["launches"][0]["device_us_median"]
        out["model_step_ms"] = a.step_ms
        out["launch_441_over_step"] = round(us / (a.step_ms * 1e3), 3)
    with open(a.out + ".json", "w") as f:
        json.dump(out, f, indent=1)
    md = ["# Device resampler against the host resampler", "",
          f"tools/resample_ab.py on {out['device']}: {CLIPS} clips x {SECONDS} s -> 16 kHz.  Device: one "
          "vasr_resample_mix_f32 launch (downmix fused), device events, median of 20 after 3 warm-ups.  Host: wall time of "
          "audio.resample (vasr_resample_f32, one thread) on one clip, x 32.", "",
          "| input | taps x rows | outputs per workgroup | device us (min - max) | GMAC/s | host ms, one clip | host ms, 32 clips "
          "| host / device | same bits |", "|---|---|---|---|---|---|---|---|---|"]
    for r in out["launches"]:
        md.append(f"| {r['kind']} | {r['taps_per_output']} x {r['tap_rows']} | {r['tile_outputs']} | {r['device_us_median']} "
                  f"({r['device_us_min']} - {r['device_us_max']}) | {r['gmac_per_s']} | {r['host_ms_one_clip']} | "
                  f"{r['host_ms_32_clips']} | {r['host_over_device']} | {r['bit_identical']} |")
    if "transcribe_files" in out:
        t = out["transcribe_files"]
        md += ["", f"transcribe_files over {t['files']} files ({t['kind']}), batch_size {t['batch_size']}, wall ms per call, "
               "VASR_DEVICE_RESAMPLE=1 then =0, alternating:", "", "| pair | device ms | host ms | host / device |", "|---|---|---|---|"]
        md += [f"| {i + 1} | {r['device_ms']} | {r['host_ms']} | {r['host_over_device']} |" for i, r in enumerate(t["pairs"])]
        md += ["", f"Result dicts identical: {t['results_identical']}.  Device leg never slower: {t['device_never_slower']}."]
    if a.step_ms:
        md += ["", f"Model step for the same 32 clips (bench.py): {a.step_ms} ms; the 44.1 kHz launch is "
               f"{out['launch_441_over_step']} of it."]
    with open(a.out + ".md", "w") as f:
        f.write("\n".join(md) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
