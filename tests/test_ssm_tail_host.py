"""CPU check of the references the kernel-level SSM tail tests compare against (ssm_tail_cases.py), over
the GPU tests' own case lists: that ref_f32 and ref_f64 are the same function to fp32 rounding, that
the staged pair meets the row conditions the bf16 kernels are held to with the chosen seeds, and that
those conditions tell a wrong kernel from a reordered one (the errors are made on the CPU, in a copy of
ref_f32's result)."""

import numpy as np
import pytest
import torch

import ssm_tail_cases as C


@pytest.mark.parametrize("gated", [True, False], ids=["gated", "ungated"])
def test_unstaged_pair_within_fp32_bar(gated):
    """ref_f32 against ref_f64 without the bf16 staging: inside 2e-5 max(1, max |ref|) at every M of
    the GPU tests (the largest difference is a few 1e-6: the margin the fp32 kernel's bar leaves)."""
    worst = 0.0
    for M in C.MS:
        ref = C.case_ref(M, 0, gated, False)
        got = C.case_ref(M, 0, gated, False, True)
        worst = max(worst, float(np.abs(got - ref).max()))
        np.testing.assert_allclose(got, ref, atol=C.ATOL * max(1.0, np.abs(ref).max()), rtol=C.RTOL, err_msg=f"M={M}")
    assert worst < 2e-5, worst


@pytest.mark.parametrize("gated", [True, False], ids=["gated", "ungated"])
def test_staged_pair_meets_row_conditions(gated):
    """The staged pair over MS x SEEDS: most rows agree to the fp32 bar, a few per cent are loose by a
    bf16 rounding flip, and no row position is loose under all three seeds -- so conditions (a)-(c)
    with the pair's own figures are ones a correct third evaluation can meet.  (A seed that made the
    pair miss (c) would be changed here, not the condition.)"""
    pair = C.pair_stats(gated)
    fails, st = C.conditions(pair["per"], pair)
    assert not fails, fails
    assert pair["rows"] == len(C.SEEDS) * sum(C.MS)
    # flips exist and are rare: (b)'s cap 4 s_ref is neither 0 nor a licence for a wrong tile (one
    # tile of a 545-row case is 6 % of its rows, under all three seeds)
    assert 0.0 < pair["s_ref"] < 0.05, pair["s_ref"]
    # a flip moves an output by far more than fp32 rounding and far less than the outputs' size
    top = max(np.abs(C.case_ref(M, s, gated, True)).max() for M in C.MS for s in C.SEEDS)
    assert 10 * C.ATOL * top < pair["E_ref"] < 1e-2 * top, (pair["E_ref"], top)
    assert pair["tight"] <= C.ATOL * top + C.RTOL * top


def test_staging_is_visible_to_the_conditions():
    """The staged and the unstaged algorithm differ on every row by more than the fp32 bar: a kernel
    that skips one of the four roundings is not a reordering of the staged one."""
    for gated in (True, False):
        for M in (33, 257):
            _, loose = C.row_errors(C.case_ref(M, 0, gated, False), C.case_ref(M, 0, gated, True))
            assert loose.all()


def _mutants(M, seed, P):
    """Wrong kernels as edits of the staged float32 evaluation: name -> (M, 192) output."""
    yd, u, x = C.inputs(M, seed)
    good = C.case_ref(M, seed, True, True, True)
    out = {}
    out["dropped b2"] = good - P["b2"].astype(np.float64)
    # g handed to out_proj unrounded: the algorithm with g's rounding point removed
    F = torch.nn.functional
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float32))  # noqa: E731
    r = lambda a: a.to(torch.bfloat16).float()  # noqa: E731
    z = r(t(u)) @ r(t(P["wz"])).T
    g = t(yd) * (z * torch.sigmoid(z))
    x1 = g @ r(t(P["wo"])).T + t(x)
    h = F.layer_norm(x1, (C.D,), t(P["ln_w"]), t(P["ln_b"]), C.EPS)
    f = F.gelu(F.linear(r(h), r(t(P["w1"])), t(P["b1"])))
    out["g not rounded"] = (F.linear(r(f), r(t(P["w2"])), t(P["b2"])) + x1).double().numpy()
    if M > 96:
        sw = good.copy()
        sw[32:64], sw[64:96] = good[64:96], good[32:64]
        out["tiles 1 and 2 swapped"] = sw
        un = good.copy()
        un[64:96] = np.nan  # a tile no workgroup wrote: the NaN the tests pre-fill out with
        out["tile 2 unwritten"] = un
    if M % 32 == 1:
        lr = good.copy()
        lr[M - 1] = good[M - 2]  # the ragged tile's one row computed from the row before it
        out["last row from row M - 2"] = lr
    return out


def test_conditions_catch_wrong_kernels():
    """Each wrong kernel, made at every case of the pooled run, misses a condition; and made at the
    single case M = 257 (9 tiles), seeds 0-2, the positional ones still do."""
    P = C.params()
    pair = C.pair_stats(True)
    names = ["dropped b2", "g not rounded"]
    for name in names:
        per = {(M, s): C.row_errors(_mutants(M, s, P)[name], C.case_ref(M, s, True, True)) for M in C.MS for s in C.SEEDS}
        fails, _ = C.conditions(per, pair)
        assert fails, name
        if name == "dropped b2":
            assert any(f.startswith("(a)") for f in fails), fails
        assert any(f.startswith("(b)") for f in fails) and any(f.startswith("(c)") for f in fails), fails
    for name in ("tiles 1 and 2 swapped", "tile 2 unwritten", "last row from row M - 2"):
        per = dict(pair["per"])
        for s in C.SEEDS:
            per[(257, s)] = C.row_errors(_mutants(257, s, P)[name], C.case_ref(257, s, True, True))
        fails, _ = C.conditions(per, pair)
        assert any(f.startswith("(a) M=257") for f in fails) and any(f.startswith("(c) M=257") for f in fails), (name, fails)


def test_fp32_bar_catches_wrong_kernels():
    """The same errors against the unstaged reference, as the fp32 gated kernel's test would see them."""
    P = C.params()
    ref = C.case_ref(257, 0, True, False)
    good = C.case_ref(257, 0, True, False, True)
    bar = dict(atol=C.ATOL * max(1.0, np.abs(ref).max()), rtol=C.RTOL)
    np.testing.assert_allclose(good, ref, **bar)
    sw = good.copy()
    sw[32:64], sw[64:96] = good[64:96], good[32:64]
    lr = good.copy()
    lr[256] = good[255]
    for bad in (good - P["b2"].astype(np.float64), sw, lr):
        with pytest.raises(AssertionError):
            np.testing.assert_allclose(bad, ref, **bar)
