#!/usr/bin/env python
"""Generate tests/golden/scan_grad.npz: the gradients of the reference's sequential selective scan
(SelectiveSSM._sequential_scan, times silu(z) where the case is gated) on seeded cases, and of the
reference's whole SelectiveSSM module on one case.

Build-machine tool, run with the REFERENCE package first on the path,

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/gen_scan_grad_goldens.py

Per case it runs the reference on the CPU in float32 and in float64 under autograd with a seeded
upstream gradient g (loss = sum(out * g)) and stores, per gradient tensor k in dx ddt dA dB dC dD dz,

  <case>/e_ref/<k>   max |fp32 reference - fp64 reference|
  <case>/gmax/<k>    max |fp64 reference|
  <case>/<k>         the fp64 reference gradient in full where the case's per-frame gradients have at
                     most FULL_LIMIT elements (and dA, dD always);
  for the larger cases <case>/frames (B, NFRAMES), a seeded sample of frames of each utterance (the
  first and the last among them), <case>/<k>_at the per-frame gradients (dx ddt dz dB dC) at those
  frames, and <case>/<k>_rowsum (B, L) the sum of every frame's row;
  <case>/sha         SHA-256 of the regenerated float32 inputs (make_inputs).

`module/...` holds the module case: the reference's SelectiveSSM(d_model=8, state_dim=64,
expand_ratio=2, scan_mode="sequential") with the seeded state_dict of module_state(), B 2 x L 37,
and e_ref / gmax / the fp64 gradient of its six parameters and of its input.

Random float64 values do not compress; FULL_LIMIT = 6000 and NFRAMES = 10 keep the file near
0.4 MB.  The fixture only pins scan_grad_f64 below to the reference; the GPU tests compare the
device gradients with scan_grad_f64 over every entry of every case.

The helpers (make_inputs, scan_grad_f64, module_state, module_grad_f64) are our own numpy and import
nothing of the reference.  Only main() imports the reference, and asserts that it did.
"""

import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "scan_grad.npz")
FULL_LIMIT = 6000
NFRAMES = 10
GRADS = ("dx", "ddt", "dA", "dB", "dC", "dD", "dz")
PER_FRAME = ("dx", "ddt", "dz", "dB", "dC")

# Di: the smallest multiple the backward kernel accepts (1024 / kernel state dim) unless said otherwise
CASES = {
    "l1": dict(B=1, L=1, Di=16, N=64, seed=1),
    "l15": dict(B=1, L=15, Di=16, N=64, seed=2),
    "l16": dict(B=1, L=16, Di=16, N=64, seed=3),
    "l17": dict(B=1, L=17, Di=16, N=64, seed=4),
    "l33": dict(B=1, L=33, Di=16, N=64, seed=5),
    "l65": dict(B=1, L=65, Di=16, N=64, seed=6),
    "l501": dict(B=1, L=501, Di=16, N=64, seed=7),
    "n16": dict(B=2, L=37, Di=64, N=16, seed=8),
    "n32": dict(B=2, L=37, Di=32, N=32, seed=9),
    "n128": dict(B=2, L=37, Di=8, N=128, seed=10),
    "n48": dict(B=2, L=37, Di=16, N=48, seed=11),
    "di48_b2_l37": dict(B=2, L=37, Di=48, N=64, seed=12),
    "ungated": dict(B=2, L=37, Di=16, N=64, seed=13, gated=False),
    "big_dt": dict(B=2, L=37, Di=16, N=64, seed=14, big_dt=True),
    "x_only": dict(B=1, L=21, Di=16, N=64, seed=15),
}
MODULE = dict(B=2, L=37, d_model=8, state_dim=64, expand_ratio=2, seed=101)


def _softplus(v):
    return np.where(v > 20.0, v, np.log1p(np.exp(np.minimum(v, 20.0))))


def make_inputs(c):
    """A case's float32 inputs: x, z, B, C, D, g ~ N(0, 1), dt = softplus(N(0, 1) - 1) (big_dt: 6
    sigmoid(2 N(0, 1)), up to about 6, so a = exp(dt A) underflows for most n), A = -(1 .. N)."""
    r = np.random.RandomState(c["seed"])
    B, L, Di, N = c["B"], c["L"], c["Di"], c["N"]
    f = lambda *shape: r.standard_normal(shape).astype(np.float32)  # noqa: E731
    x, z, Bm, Cm, D, g, raw = f(B, L, Di), f(B, L, Di), f(B, L, N), f(B, L, N), f(Di), f(B, L, Di), f(B, L, Di)
    if c.get("big_dt"):
        dt = (6.0 / (1.0 + np.exp(-2.0 * raw.astype(np.float64)))).astype(np.float32)
    else:
        dt = _softplus(raw.astype(np.float64) - 1.0).astype(np.float32)
    A = -np.arange(1, N + 1, dtype=np.float32)
    return dict(x=x, dt=dt, A=A, B=Bm, C=Cm, D=D, z=z if c.get("gated", True) else None, g=g)


def inputs_sha(inp):
    h = hashlib.sha256()
    for k in ("x", "dt", "A", "B", "C", "D", "z", "g"):
        if inp[k] is not None:
            h.update(np.ascontiguousarray(inp[k]).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def scan_grad_f64(x, dt, A, B, C, D, z, g):
    """The selective scan and its gradients in float64 (our own formulas, the kernels' mathematics):
    returns (out, dict of dx ddt dA dB dC dD dz); z None: the ungated form, dz None.

      h_t = a_t h_{t-1} + dt_t x_t B_t,  a_t = exp(dt_t A),  y_t = sum_n h_t C_t + x_t D,
      out = y silu(z);  gy = g silu(z);  gh_t = gy_t C_t + a_{t+1} gh_{t+1}  (gh_L = 0)."""
    x, dt, A, B, C, D, g = (np.asarray(v, np.float64) for v in (x, dt, A, B, C, D, g))
    Bsz, L, Di = x.shape
    N = A.shape[0]
    a = np.exp(dt[..., None] * A)  # (B, L, Di, N)
    hs = np.zeros((Bsz, L + 1, Di, N))
    for t in range(L):
        hs[:, t + 1] = a[:, t] * hs[:, t] + (dt[:, t] * x[:, t])[..., None] * B[:, t, None, :]
    y = np.einsum("bldn,bln->bld", hs[:, 1:], C) + x * D
    if z is not None:
        z = np.asarray(z, np.float64)
        sg = 1.0 / (1.0 + np.exp(-z))
        out, gy, dz = y * z * sg, g * z * sg, g * y * sg * (1.0 + z * (1.0 - sg))
    else:
        out, gy, dz = y, g, None
    dx, ddt = gy * D, np.zeros_like(x)
    dB, dC = np.zeros_like(B), np.einsum("bld,bldn->bln", gy, hs[:, 1:])
    dA = np.zeros(N)
    carry = np.zeros((Bsz, Di, N))  # a_{t+1} gh_{t+1}
    for t in range(L - 1, -1, -1):
        gh = gy[:, t, :, None] * C[:, t, None, :] + carry
        s1 = np.einsum("bdn,bn->bd", gh, B[:, t])
        w = gh * a[:, t] * hs[:, t]
        dB[:, t] = np.einsum("bdn,bd->bn", gh, dt[:, t] * x[:, t])
        dx[:, t] += dt[:, t] * s1
        ddt[:, t] = x[:, t] * s1 + w @ A
        dA += np.einsum("bdn,bd->n", w, dt[:, t])
        carry = a[:, t] * gh
    return out, dict(dx=dx, ddt=ddt, dA=dA, dB=dB, dC=dC, dD=(gy * x).sum(axis=(0, 1)), dz=dz)


def case_grad_f64(name):
    """(inputs, fp64 gradients) of a case by scan_grad_f64."""
    inp = make_inputs(CASES[name])
    return inp, scan_grad_f64(**inp)[1]


def sample_frames(c):
    """(B, NFRAMES) frames of each utterance: the first, the last and a seeded draw of the others."""
    r = np.random.RandomState(c["seed"] + 23)
    return np.stack([np.sort(np.concatenate(([0, c["L"] - 1], r.randint(0, c["L"], size=NFRAMES - 2))))
                     for _ in range(c["B"])]).astype(np.int64)


def is_full(c):
    return c["B"] * c["L"] * (3 * c["Di"] + 2 * c["N"]) <= FULL_LIMIT


def module_state(m=MODULE):
    """Seeded float32 state_dict (numpy) of SelectiveSSM(d_model, state_dim, expand_ratio), and the
    module case's input x (B, L, d_model) and upstream gradient g of the same shape."""
    r = np.random.RandomState(m["seed"])
    dm, N, Di = m["d_model"], m["state_dim"], m["d_model"] * m["expand_ratio"]
    f = lambda scale, *shape: (scale * r.standard_normal(shape)).astype(np.float32)  # noqa: E731
    sd = {
        "in_proj.weight": f(dm ** -0.5, 2 * Di, dm),
        "x_proj.weight": f(Di ** -0.5, 2 * N, Di),
        "dt_proj.weight": f(Di ** -0.5, Di, Di),
        "dt_proj.bias": f(1.0, Di) - 1.0,
        "A_log": (np.log(np.arange(1, N + 1)) + 0.1 * r.standard_normal(N)).astype(np.float32),
        "D": f(1.0, Di),
        "out_proj.weight": f(Di ** -0.5, dm, Di),
    }
    return sd, f(1.0, m["B"], m["L"], dm), f(1.0, m["B"], m["L"], dm)


MODULE_GRADS = ("in_proj.weight", "x_proj.weight", "dt_proj.weight", "dt_proj.bias", "A_log", "D", "out_proj.weight",
                "input")


def module_grad_f64(sd, x, g):
    """float64 gradients of sum(SelectiveSSM(x) * g) (sequential scan) for the parameters and x, by
    scan_grad_f64 and the chain rule through the projections, softplus and A = -exp(A_log)."""
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    Di, N = sd["D"].shape[0], sd["A_log"].shape[0]
    xz = x @ sd["in_proj.weight"].T
    xp, z = xz[..., :Di], xz[..., Di:]
    bcm = xp @ sd["x_proj.weight"].T
    Bm, Cm = bcm[..., :N], bcm[..., N:]
    pre = xp @ sd["dt_proj.weight"].T + sd["dt_proj.bias"]
    dt = _softplus(pre)
    A = -np.exp(sd["A_log"])
    gy = g @ sd["out_proj.weight"]  # d loss / d (gated scan output)
    out, gr = scan_grad_f64(xp, dt, A, Bm, Cm, sd["D"], z, gy)
    flat = lambda v: v.reshape(-1, v.shape[-1])  # noqa: E731
    dpre = gr["ddt"] / (1.0 + np.exp(-pre))
    dbc = np.concatenate([gr["dB"], gr["dC"]], -1)
    dxp = gr["dx"] + dbc @ sd["x_proj.weight"] + dpre @ sd["dt_proj.weight"]
    dxz = np.concatenate([dxp, gr["dz"]], -1)
    return {
        "in_proj.weight": flat(dxz).T @ flat(x),
        "x_proj.weight": flat(dbc).T @ flat(xp),
        "dt_proj.weight": flat(dpre).T @ flat(xp),
        "dt_proj.bias": flat(dpre).sum(0),
        "A_log": gr["dA"] * A,
        "D": gr["dD"],
        "out_proj.weight": flat(g).T @ flat(out),
        "input": dxz @ sd["in_proj.weight"],
    }


def main():
    import torch
    import velocity_asr
    from velocity_asr import ssm as ref_ssm

    ours = os.path.realpath(os.path.join(HERE, "..", "..", "velocity-asr_amd"))
    assert not os.path.realpath(velocity_asr.__file__).startswith(ours) and hasattr(
        ref_ssm.SelectiveSSM, "_sequential_scan") and not hasattr(ref_ssm, "selective_scan"), \
        f"{velocity_asr.__file__} is not the reference package: put the reference first on PYTHONPATH"

    def reference(c, inp, dtype):
        m = ref_ssm.SelectiveSSM(d_model=c["Di"] // 2, state_dim=c["N"], expand_ratio=2, scan_mode="sequential").to(dtype)
        t = {k: torch.from_numpy(v).to(dtype).requires_grad_() for k, v in inp.items() if v is not None and k != "g"}
        with torch.no_grad():
            m.D.copy_(t["D"])
        y = m._sequential_scan(t["x"], t["dt"], t["A"], t["B"], t["C"])
        if "z" in t:
            y = y * torch.nn.functional.silu(t["z"])
        (y * torch.from_numpy(inp["g"]).to(dtype)).sum().backward()
        gr = {"d" + k: t[k].grad.numpy().astype(np.float64) for k in ("x", "dt", "A", "B", "C") + (("z",) if "z" in t else ())}
        gr["dD"] = m.D.grad.numpy().astype(np.float64)
        return gr

    out = {"names": np.array(sorted(CASES))}
    for name, c in CASES.items():
        inp = make_inputs(c)
        g32, g64 = reference(c, inp, torch.float32), reference(c, inp, torch.float64)
        own = scan_grad_f64(**inp)[1]
        out[f"{name}/sha"] = inputs_sha(inp)
        frames = sample_frames(c)
        if not is_full(c):
            out[f"{name}/frames"] = frames
        worst = 0.0
        for k in GRADS:
            if k not in g64:
                continue
            gmax = float(np.abs(g64[k]).max())
            out[f"{name}/e_ref/{k}"] = np.array(float(np.abs(g32[k] - g64[k]).max()), np.float64)
            out[f"{name}/gmax/{k}"] = np.array(gmax, np.float64)
            worst = max(worst, float(np.abs(own[k] - g64[k]).max()) / max(gmax, 1e-300))
            if k not in PER_FRAME or is_full(c):
                out[f"{name}/{k}"] = g64[k]
            else:
                out[f"{name}/{k}_at"] = np.stack([g64[k][b][frames[b]] for b in range(c["B"])])
                out[f"{name}/{k}_rowsum"] = g64[k].sum(axis=2)
        print(f"{name:12s} scan_grad_f64 vs fp64 reference {worst:.2e} of gmax;  e_ref " +
              " ".join(f"{k} {float(out[f'{name}/e_ref/{k}']):.2e}" for k in GRADS if f"{name}/e_ref/{k}" in out))

    sd, x, g = module_state()
    grads = {}
    for dtype in (torch.float32, torch.float64):
        m = ref_ssm.SelectiveSSM(d_model=MODULE["d_model"], state_dim=MODULE["state_dim"],
                                 expand_ratio=MODULE["expand_ratio"], scan_mode="sequential")
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        m = m.to(dtype)
        xt = torch.from_numpy(x).to(dtype).requires_grad_()
        (m(xt) * torch.from_numpy(g).to(dtype)).sum().backward()
        grads[dtype] = {k: p.grad.numpy().astype(np.float64) for k, p in m.named_parameters()}
        grads[dtype]["input"] = xt.grad.numpy().astype(np.float64)
    own = module_grad_f64(sd, x, g)
    worst = 0.0
    for k in MODULE_GRADS:
        g64 = grads[torch.float64][k]
        out[f"module/{k}"] = g64
        out[f"module/e_ref/{k}"] = np.array(float(np.abs(grads[torch.float32][k] - g64).max()), np.float64)
        out[f"module/gmax/{k}"] = np.array(float(np.abs(g64).max()), np.float64)
        worst = max(worst, float(np.abs(own[k] - g64).max() / np.abs(g64).max()))
    print(f"module       module_grad_f64 vs fp64 reference {worst:.2e} of gmax")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    sys.exit(main())
