"""Alignments on the device: vasr_edit_align_i32 against the specification training.edit_alignment_host,
exact equality of every path everywhere.  Ids come from an alphabet of 3, so cost ties are everywhere; seeds
are fixed.  The long side of a pair is matched with a short one: the pure-Python oracle keeps a whole table."""

import importlib.util
import os
import random

import numpy as np
import pytest
import torch

import score_cases as sc
from conftest import PKG_ROOT
from velocity_asr import synthetic as S
from velocity_asr import training as T

pytestmark = pytest.mark.gpu


def _lib():
    from velocity_asr import _lib
    return _lib.lib()


def _geometry():
    lib = _lib()
    return lib.vasr_edit_wave_cols(), lib.vasr_edit_tile_cols()


def _spec(pairs):
    return [T.edit_alignment_host(h, r) for h, r in pairs]


def _counts_of(paths):
    return [[p.count(1), p.count(2), p.count(3)] for p in paths]


def _matrices(pairs, fill=-1, extra_ld=0, width_h=None, width_r=None):
    wh = max([len(h) for h, _ in pairs] + [0]) if width_h is None else width_h
    wr = max([len(r) for _, r in pairs] + [0]) if width_r is None else width_r
    H, hl = sc.pad_batch([h for h, _ in pairs], wh, max(wh, 1) + extra_ld, fill)
    R, rl = sc.pad_batch([r for _, r in pairs], wr, max(wr, 1) + extra_ld, fill)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    return dev(H)[:, :wh], dev(R)[:, :wr], hl, rl


def _paths(ops, ops_len):
    ops, ops_len = ops.cpu().numpy(), ops_len.cpu().tolist()
    return [None if n < 0 else row[:n].tolist() for row, n in zip(ops, ops_len)]


def _device(pairs, lengths_on="host", table_bytes=None, **kw):
    """One ops.edit_alignment call on `pairs` -> (paths, counts); checks the shapes and that the counts beside
    the paths are ops.edit_counts' on the same inputs."""
    from velocity_asr import ops
    H, R, hl, rl = _matrices(pairs, **kw)
    hld, rld = torch.from_numpy(hl).cuda(), torch.from_numpy(rl).cuda()
    lens = (hl.tolist(), rl.tolist()) if lengths_on == "host" else (hld, rld)
    extra = {} if table_bytes is None else dict(table_bytes=table_bytes)
    counts, path, length = ops.edit_alignment(H, R, *lens, **extra)
    P = len(pairs)
    assert counts.dtype == torch.int32 and counts.shape == (P, 3) and counts.is_cuda
    assert path.dtype == torch.uint8 and path.shape == (P, max(1, H.shape[1] + R.shape[1])) and path.is_cuda
    assert length.dtype == torch.int32 and length.shape == (P,) and length.is_cuda
    assert torch.equal(counts, ops.edit_counts(H, R, hld, rld))
    return _paths(path, length), counts.cpu().tolist()


def _raw(pairs, stream=None, declared=None, skip=()):
    """The C entry point with the table, the ops array and the workspace filled with 0xFF beforehand.
    declared: the table_bytes passed (the buffer is always full size); the tables of `skip` are laid out last.
    -> (paths, counts, ops array, ops_len)."""
    lib = _lib()
    H, R, hl, rl = _matrices(pairs)
    P, mh, mr = len(pairs), H.shape[1], R.shape[1]
    order = [p for p in range(P) if p not in skip] + list(skip)
    offs, used = [0] * P, 0
    for p in order:
        offs[p] = used
        used += -(-lib.vasr_edit_align_table_bytes(int(hl[p]), int(rl[p])) // 16) * 16
    need = lib.vasr_edit_workspace_bytes(P, mh, mr)
    ff = lambda n, dt=torch.uint8: torch.full((max(n, 1),), 0xFF, device="cuda", dtype=torch.uint8).view(dt)  # noqa: E731
    hld, rld = torch.from_numpy(hl).cuda(), torch.from_numpy(rl).cuda()
    table, ws = ff(used), ff(max(need, 8))
    ops = ff(P * (mh + mr)).view(P, mh + mr)
    ops_len, counts = ff(4 * P, torch.int32), ff(12 * P, torch.int32).view(P, 3)
    offd = torch.tensor(offs, dtype=torch.int64).cuda()
    ldh = H.stride(0) if P > 1 else max(mh, 1)
    ldr = R.stride(0) if P > 1 else max(mr, 1)
    rc = lib.vasr_edit_align_i32(H.data_ptr(), ldh, hld.data_ptr(), mh, R.data_ptr(), ldr, rld.data_ptr(), mr, P,
                                 counts.data_ptr(), ops.data_ptr(), mh + mr, ops_len.data_ptr(), offd.data_ptr(),
                                 table.data_ptr(), used if declared is None else declared, ws.data_ptr() if need else None,
                                 need, stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.vasr_last_error()
    (stream or torch.cuda.current_stream()).synchronize()
    return _paths(ops, ops_len), counts.cpu().tolist(), ops.cpu().numpy(), ops_len.cpu().tolist(), offs


def _check_untouched(ops, ops_len):
    for row, n in zip(ops, ops_len):
        assert (row[max(n, 0):] == 0xFF).all()


@pytest.mark.parametrize("long_side", ["ref", "hyp"])
def test_boundary_lengths_in_one_batched_call(long_side):
    """Strip, wave, one-wave-limit and tile boundaries (and three passes) against 0, 1, 5 and 70 items on the
    other side; both orientations; every buffer poisoned, nothing written past a path's end."""
    w, t = _geometry()
    pairs = sc.boundary_pairs(w, t)
    assert {len(a) for a, _ in pairs} >= {0, 1, 2, 8, 63, 64, 65, w - 1, w, w + 1, t - 1, t, t + 1, 2 * t + 3}
    if long_side == "ref":
        pairs = [(b, a) for a, b in pairs]
    want = _spec(pairs)
    got, counts, ops, ops_len, _ = _raw(pairs)
    assert ops_len == [len(r) + c[2] for (_, r), c in zip(pairs, counts)]
    assert got == want and counts == _counts_of(want)
    _check_untouched(ops, ops_len)


def test_tall_and_wide_pair_fills_and_drains_several_waves():
    rng = random.Random(3)
    ref = sc.seq(rng, 1300)
    hyp = (sc.edited(rng, ref, 0.3) + sc.seq(rng, 200))[:1500]
    assert len(hyp) > 1300
    pairs = [(hyp, ref)]
    want = _spec(pairs)
    assert set(want[0]) == {0, 1, 2, 3}
    assert _device(pairs) == (want, _counts_of(want))


@pytest.mark.parametrize("n", [33, "w+1"])
def test_structured_contents(n):
    n = _geometry()[0] + 1 if n == "w+1" else n
    pairs = sc.content_pairs(n)
    want = _spec(pairs)
    assert want[0] == [0] * n and want[1].count(1) == n and want[1].count(2) == 2 and want[2].count(3) == 2
    assert sorted(want[4]) == [0] * n + [2] * 3 and sorted(want[5]) == [0] * n + [3] * 3
    assert _device(pairs, lengths_on="device") == (want, _counts_of(want))


def test_padding_content_and_leading_dimension_do_not_matter():
    pairs = sc.random_pairs(300, 200, seed=9)
    want = _spec(pairs)
    a = _device(pairs, fill=1, extra_ld=37)   # a symbol of the alphabet
    b = _device(pairs, fill=-1, extra_ld=37, lengths_on="device")
    assert a == b == (want, _counts_of(want))
    # matrices narrower than some stored lengths: the lengths clamp
    cut = [(h[:150], r[:120]) for h, r in pairs]
    assert any(len(h) > 150 for h, _ in pairs) and any(len(r) > 120 for _, r in pairs)
    for where in ("host", "device"):
        assert _device(pairs, fill=1, extra_ld=5, width_h=150, width_r=120, lengths_on=where)[0] == _spec(cut)


def _mixed():
    w, t = _geometry()
    rng = random.Random(21)
    pairs = sc.random_pairs(200, 90, seed=22)
    wide = [(sc.seq(rng, 40), sc.seq(rng, t + 9)), (sc.seq(rng, 33), sc.seq(rng, t + w + 1))]
    return pairs[:50] + wide[:1] + pairs[50:] + wide[1:]


def test_mixed_regimes_in_one_call_run_to_run_and_in_several_launches():
    from velocity_asr import ops
    lib = _lib()
    pairs = _mixed()
    want = _spec(pairs)
    first = _device(pairs)
    assert first == (want, _counts_of(want))
    assert _device(pairs) == first
    # a budget that holds the largest table but forces at least three launches
    sizes = [-(-lib.vasr_edit_align_table_bytes(len(h), len(r)) // 16) * 16 for h, r in pairs]
    budget = max(max(sizes), sum(sizes) // 4)
    calls = []
    real = lib.vasr_edit_align_i32
    try:
        lib.vasr_edit_align_i32 = lambda *a: calls.append(a[8]) or real(*a)
        assert _device(pairs, table_bytes=budget) == first
    finally:
        lib.vasr_edit_align_i32 = real
    assert len(calls) >= 3 and sum(calls) == len(pairs)
    assert ops.EDIT_ALIGN_TABLE_BYTES >= sum(sizes)


def test_a_pair_over_the_table_budget_comes_back_unaligned(monkeypatch):
    lib = _lib()
    pairs = sc.random_pairs(20, 60, seed=5)
    rng = random.Random(6)
    big = (sc.seq(rng, 300), sc.seq(rng, 310))
    pairs = pairs[:7] + [big] + pairs[7:]
    budget = lib.vasr_edit_align_table_bytes(300, 310) - 2
    assert all(lib.vasr_edit_align_table_bytes(len(h), len(r)) <= budget for h, r in pairs if (h, r) != big)
    want = _spec(pairs)
    got, counts = _device(pairs, table_bytes=budget)          # the counts are checked against ops.edit_counts inside
    assert got[7] is None and counts[7] == list(T.edit_counts_host(*big))
    assert got[:7] + got[8:] == want[:7] + want[8:]
    # the public path aligns that pair on the host
    monkeypatch.setattr(T, "ALIGN_MIN_DEVICE_CELLS", 0)
    monkeypatch.setattr(T, "ALIGN_TABLE_BYTES", budget)
    text = lambda s: " ".join("abc"[x] for x in s)  # noqa: E731
    als = T.error_alignments([text(h) for h, _ in pairs], [text(r) for _, r in pairs], "word", device="cuda")
    assert [a.ops for a in als] == want


def test_counts_only_entry_is_the_same_before_and_after_an_alignment():
    from velocity_asr import ops
    pairs = _mixed()
    H, R, hl, rl = _matrices(pairs)
    hld, rld = torch.from_numpy(hl).cuda(), torch.from_numpy(rl).cuda()
    before = ops.edit_counts(H, R, hld, rld).clone()
    ops.edit_alignment(H, R, hld, rld)
    after = ops.edit_counts(H, R, hld, rld)
    assert torch.equal(before, after)
    assert before.cpu().tolist() == [list(T.edit_counts_host(h, r)) for h, r in pairs]


def test_guard_skips_a_pair_whose_table_is_outside_the_declared_bytes():
    """The declared table_bytes leaves out the last-laid-out pair's table while the buffer is full size: that
    pair comes back with ops_len -1, its counts right and its ops row untouched; the others are right."""
    w, t = _geometry()
    pairs = sc.random_pairs(30, 80, seed=8)
    rng = random.Random(9)
    pairs[11] = (sc.seq(rng, 90), sc.seq(rng, 100))
    pairs[20] = (sc.seq(rng, 60), sc.seq(rng, w + 40))     # a pair of the long kernel, skipped too
    want = _spec(pairs)
    for skip in ((11,), (20,)):
        lib = _lib()
        full = _raw(pairs, skip=skip)
        assert full[0] == want
        offs = full[4]
        declared = offs[skip[0]] + lib.vasr_edit_align_table_bytes(len(pairs[skip[0]][0]), len(pairs[skip[0]][1])) - 2
        got, counts, ops, ops_len, _ = _raw(pairs, declared=declared, skip=skip)
        assert ops_len[skip[0]] == -1 and got[skip[0]] is None and (ops[skip[0]] == 0xFF).all()
        assert counts == _counts_of(want)
        assert [g for k, g in enumerate(got) if k not in skip] == [x for k, x in enumerate(want) if k not in skip]
        _check_untouched(ops, ops_len)


def test_non_default_stream():
    w, t = _geometry()
    rng = random.Random(31)
    pairs = [(sc.seq(rng, 50), sc.seq(rng, 2 * t + 5)), (sc.seq(rng, 9), sc.seq(rng, 12)), (sc.seq(rng, 64), sc.seq(rng, t + 1)),
             (sc.seq(rng, 300), sc.seq(rng, 200))]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got, counts, ops, ops_len, _ = _raw(pairs, stream=stream)
    want = _spec(pairs)
    assert got == want and counts == _counts_of(want)
    _check_untouched(ops, ops_len)


# --------------------------------------------------------------------------- the public path
@pytest.fixture
def always_on_device(monkeypatch):
    monkeypatch.setattr(T, "ALIGN_MIN_DEVICE_CELLS", 0)
    monkeypatch.setattr(T, "MIN_DEVICE_CELLS", 0)


def test_error_alignments_on_the_device_equal_the_host_path(always_on_device, monkeypatch):
    from velocity_asr import ops
    calls = []
    real = ops.edit_alignment
    monkeypatch.setattr(ops, "edit_alignment", lambda *a, **k: calls.append(a[0].shape[0]) or real(*a, **k))
    pairs = sc.sentence_pairs(50, 60, seed=13)
    preds, refs = [p for p, _ in pairs], [r for _, r in pairs]
    for unit in ("word", "char"):
        del calls[:]
        assert T.error_alignments(preds, refs, unit, device="cuda") == T.error_alignments(preds, refs, unit)
        assert sum(calls) == 50                         # every pair went through the kernels


# --------------------------------------------------------------------------- evaluate.py end to end
def test_evaluate_writes_alignments_from_the_device(tmp_path, capsys, always_on_device, monkeypatch):
    import velocity_asr as v
    from velocity_asr import ops
    from velocity_asr.audio import write_wav
    spec = importlib.util.spec_from_file_location("vasr_script_evaluate_align_gpu", os.path.join(PKG_ROOT, "scripts", "evaluate.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    m = v.VELOCITYASR()
    m.load_state_dict({k: torch.from_numpy(x) for k, x in S.make_weights(None, seed=0).items()})
    m.save_pretrained(str(tmp_path / "model.pt"))
    a = S.make_audio(2, 32000, seed=21)
    clips = [("c0.wav", a[0]), ("c1.wav", a[1]), ("e.wav", S.make_audio(1, 16333, seed=35)[0])]
    for name, x in clips:
        write_wav(str(tmp_path / name), x)
    dec = v.CTCDecoder(v.create_default_vocabulary(m.config.vocab_size))
    from velocity_asr.transcription import transcribe_files
    texts = [r["transcription"] for r in transcribe_files(m.cuda().eval(), [tmp_path / n for n, _ in clips], dec, "cuda")]
    refs = [texts[0], "zz " + texts[1] + " q", "one two three"]
    man = tmp_path / "m.tsv"
    man.write_text("".join(f"{tmp_path / n}\t{r}\n" for (n, _), r in zip(clips, refs)), encoding="utf-8")
    calls = []
    real = ops.edit_alignment
    monkeypatch.setattr(ops, "edit_alignment", lambda *a, **k: calls.append(1) or real(*a, **k))
    out, al = tmp_path / "report.txt", tmp_path / "al.txt"
    assert ev.main(["--checkpoint", str(tmp_path / "model.pt"), "--test-set", str(man), "--output", str(out),
                    "--alignments", str(al), "--confusions", "3"]) == 0
    assert calls
    host = T.error_alignments(texts, refs, "word")
    text = ""
    for (n, _), h in zip(clips, host):
        c = h.counts
        text += f"{tmp_path / n}\tN={c.ref_length} S={c.substitutions} D={c.deletions} I={c.insertions}\n"
        text += T.format_alignment(h) + "\n\n"
    assert al.read_text(encoding="utf-8") == text
    lines = out.read_text().splitlines()
    assert lines[2] == f"WER: {T.compute_wer(texts, refs) * 100:.2f}%"
    want = []
    for name, counter, show in zip(("substitutions", "deletions", "insertions"), T.confusions(host),
                                   (lambda k: f"{k[0]} -> {k[1]}", str, str)):
        want.append(f"Top word {name}:")
        want += [f"  {n:6d}  {show(k)}" for k, n in counter.most_common(3)]
    assert lines[4:] == want and sum(h.counts.deletions for h in host) >= 2
