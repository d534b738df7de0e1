#!/usr/bin/env python
"""Generate tests/golden/tree_grad.npz: the gradients of the reference's default tree scan
(SelectiveSSM._parallel_scan, times silu(z) where the case is gated) on seeded cases, and of the
reference's SelectiveSSM, SSMBlock and GlobalSSM modules (scan_mode "parallel") on one case each.

Build-machine tool, run with the REFERENCE package first on the path,

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/gen_tree_grad_goldens.py

The layout is gen_scan_grad_goldens.py's.  Per case the reference runs on the CPU in float32 and in
float64 under autograd with a seeded upstream gradient g (loss = sum(out * g)); per gradient tensor
k in dx ddt dA dB dC dD dz the file holds

  <case>/e_ref/<k>   max |fp32 reference - fp64 reference|
  <case>/gmax/<k>    max |fp64 reference|
  <case>/<k>         the fp64 reference gradient in full where the case's per-frame gradients have at
                     most FULL_LIMIT elements (and dA, dD always); for the larger cases
                     <case>/frames, <case>/<k>_at and <case>/<k>_rowsum as in scan_grad.npz;
  <case>/sha         SHA-256 of the regenerated float32 inputs.

`<module>/...` for module in MODULES holds e_ref / gmax / the fp64 gradient of every parameter and of
the input.  The fixture only pins tree_grad_f64 and module_grad_f64 below to the reference; the GPU
tests compare the device gradients with those two over every entry.

The helpers are our own numpy and import nothing of the reference.  Only main() imports the
reference, and asserts that it did.
"""

import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_scan_grad_goldens as SG  # noqa: E402  (shared helpers: checksums, frame samples, softplus)

OUT = os.path.join(HERE, "tree_grad.npz")
GRADS, PER_FRAME = SG.GRADS, SG.PER_FRAME
inputs_sha, sample_frames, is_full = SG.inputs_sha, SG.sample_frames, SG.is_full

# Di: the smallest multiple the backward kernel accepts (1024 / kernel state dim) unless said otherwise
CASES = {
    "l1": dict(B=1, L=1, Di=16, N=64, seed=1),      # h = 0: dA = dB = 0 exactly, dx = g D
    "l2": dict(B=1, L=2, Di=16, N=64, seed=2),      # the first tree levels
    "l3": dict(B=1, L=3, Di=16, N=64, seed=3),
    "l16": dict(B=1, L=16, Di=16, N=64, seed=4),    # the chunk boundary
    "l17": dict(B=1, L=17, Di=16, N=64, seed=5),
    "di48_b2_l37": dict(B=2, L=37, Di=48, N=64, seed=6),  # several workgroups / channel blocks
    "l257": dict(B=1, L=257, Di=16, N=64, seed=7),  # 17 chunks: the outer tree passes one radix-16 level
    "l501": dict(B=1, L=501, Di=16, N=64, seed=8),  # the workload's length; 32 chunks: the most the outer
                                                    # tree keeps in registers
    "l513": dict(B=1, L=513, Di=16, N=64, seed=16),  # 33 chunks: the outer tree works in the workspace
    "n16": dict(B=2, L=37, Di=64, N=16, seed=9),
    "n32": dict(B=2, L=37, Di=32, N=32, seed=10),
    "n128": dict(B=2, L=37, Di=8, N=128, seed=11),
    "n48": dict(B=2, L=37, Di=16, N=48, seed=12),   # zero-padded to 64
    "ungated": dict(B=2, L=37, Di=16, N=64, seed=13, gated=False),
    "big_dt": dict(B=2, L=37, Di=16, N=64, seed=14, big_dt=True),
    "x_only": dict(B=1, L=21, Di=16, N=64, seed=15),
}

MODULES = {
    "ssm": dict(kind="ssm", B=2, L=37, d_model=8, state_dim=64, seed=201),
    "block": dict(kind="block", B=2, L=37, d_model=16, state_dim=64, seed=202),
    "global": dict(kind="global", B=2, L=20, d_model=16, state_dim=32, layers=2, seed=203),
}
KERNEL_SIZE, EXPAND = 4, 2


def make_inputs(c):
    """A case's float32 inputs: x, z, B, C, D, g ~ N(0, 1), dt = softplus(N(0, 1) - 1) (big_dt: 4
    sigmoid(2 N(0, 1)), up to about 4, so a = exp(dt A) underflows for the larger n), A = -(1 .. N)."""
    r = np.random.RandomState(c["seed"])
    B, L, Di, N = c["B"], c["L"], c["Di"], c["N"]
    f = lambda *shape: r.standard_normal(shape).astype(np.float32)  # noqa: E731
    x, z, Bm, Cm, D, g, raw = f(B, L, Di), f(B, L, Di), f(B, L, N), f(B, L, N), f(Di), f(B, L, Di), f(B, L, Di)
    if c.get("big_dt"):
        dt = (4.0 / (1.0 + np.exp(-2.0 * raw.astype(np.float64)))).astype(np.float32)
    else:
        dt = SG._softplus(raw.astype(np.float64) - 1.0).astype(np.float32)
    A = -np.arange(1, N + 1, dtype=np.float32)
    return dict(x=x, dt=dt, A=A, B=Bm, C=Cm, D=D, z=z if c.get("gated", True) else None, g=g)


def tree_state_f64(a, b):
    """The tree scan's state in closed form, float64: a, b (B, L, Di, N) -> h with
    h_t = sum over the set bits k of t of P_{e_S} R_S, S = [t with bits 0..k cleared, + 2^k),
    P the inclusive product of a and R_S the local inclusive scan of S."""
    L = a.shape[1]
    P = np.cumprod(a, axis=1)
    h = np.zeros_like(b)
    ln = 1
    while ln < L:
        for base in range(0, L - ln, 2 * ln):
            rho = np.zeros_like(b[:, 0])
            for s in range(base, base + ln):
                rho = a[:, s] * rho + b[:, s]
            e = base + ln - 1
            h[:, e + 1:min(base + 2 * ln, L)] += (P[:, e] * rho)[:, None]
        ln *= 2
    return h


def tree_grad_f64(x, dt, A, B, C, D, z, g):
    """The tree scan and its gradients in float64 (our own formulas, the kernels' mathematics):
    returns (out, dict of dx ddt dA dB dC dD dz); z None: the ungated form, dz None.

      a_t = exp(dt_t A), b_t = x_t dt_t B_t, h = tree_state_f64(a, b), y_t = sum_n h_t C_t + x_t D,
      out = y silu(z); gy = g silu(z); gh_t = gy_t C_t;  per left block S (its right sibling not empty)
      w_S = P_{e_S} sum_{t in sibling} gh_t,  lambda_S(s) = w_S prod_{s < r <= e_S} a_r,
      d/db_s = sum_S lambda_S(s),  d/d(dt A)_r = sum_{e_S >= r} w_S R_S + sum_{S containing r} lambda_S(r-1) rho^S_{r-1}."""
    x, dt, A, B, C, D, g = (np.asarray(v, np.float64) for v in (x, dt, A, B, C, D, g))
    Bsz, L, Di = x.shape
    a = np.exp(dt[..., None] * A)  # (B, L, Di, N)
    b = (x * dt)[..., None] * B[:, :, None, :]
    h = tree_state_f64(a, b)
    y = np.einsum("bldn,bln->bld", h, C) + x * D
    if z is not None:
        z = np.asarray(z, np.float64)
        sg = 1.0 / (1.0 + np.exp(-z))
        out, gy, dz = y * z * sg, g * z * sg, g * y * sg * (1.0 + z * (1.0 - sg))
    else:
        out, gy, dz = y, g, None
    gh = gy[..., None] * C[:, :, None, :]
    P = np.cumprod(a, axis=1)
    db, dloc, X = np.zeros_like(b), np.zeros_like(b), np.zeros_like(b)
    ln = 1
    while ln < L:
        for base in range(0, L - ln, 2 * ln):
            e = base + ln - 1
            rho = np.zeros((ln,) + b[:, 0].shape)
            cur = np.zeros_like(b[:, 0])
            for s in range(base, base + ln):
                cur = a[:, s] * cur + b[:, s]
                rho[s - base] = cur
            w = P[:, e] * gh[:, e + 1:min(base + 2 * ln, L)].sum(axis=1)
            X[:, e] += w * cur
            lam = w
            for s in range(e, base - 1, -1):
                db[:, s] += lam
                if s > base:
                    lam = a[:, s] * lam
                    dloc[:, s] += lam * rho[s - 1 - base]
        ln *= 2
    ddelta = np.cumsum(X[:, ::-1], axis=1)[:, ::-1] + dloc
    s1 = np.einsum("bldn,bln->bld", db, B)
    grads = dict(dx=gy * D + dt * s1, ddt=x * s1 + ddelta @ A, dA=np.einsum("bldn,bld->n", ddelta, dt),
                 dB=np.einsum("bldn,bld->bln", db, x * dt), dC=np.einsum("bld,bldn->bln", gy, h),
                 dD=(gy * x).sum(axis=(0, 1)), dz=dz)
    return out, grads


def case_grad_f64(name):
    """(inputs, fp64 gradients) of a case by tree_grad_f64."""
    inp = make_inputs(CASES[name])
    return inp, tree_grad_f64(**inp)[1]


# ------------------------------------------------------------------ modules
def _ssm_state(r, dm, N, prefix=""):
    Di = dm * EXPAND
    f = lambda scale, *shape: (scale * r.standard_normal(shape)).astype(np.float32)  # noqa: E731
    return {
        prefix + "in_proj.weight": f(dm ** -0.5, 2 * Di, dm),
        prefix + "x_proj.weight": f(Di ** -0.5, 2 * N, Di),
        prefix + "dt_proj.weight": f(Di ** -0.5, Di, Di),
        prefix + "dt_proj.bias": f(1.0, Di) - 1.0,
        prefix + "A_log": (np.log(np.arange(1, N + 1)) + 0.1 * r.standard_normal(N)).astype(np.float32),
        prefix + "D": f(1.0, Di),
        prefix + "out_proj.weight": f(Di ** -0.5, dm, Di),
    }


def _block_state(r, dm, N, prefix=""):
    f = lambda scale, *shape: (scale * r.standard_normal(shape)).astype(np.float32)  # noqa: E731
    sd = {}
    for n in ("norm1", "norm2"):
        sd[prefix + n + ".weight"] = 1.0 + f(0.1, dm)
        sd[prefix + n + ".bias"] = f(0.1, dm)
    sd[prefix + "conv.weight"] = f(KERNEL_SIZE ** -0.5, dm, 1, KERNEL_SIZE)
    sd[prefix + "conv.bias"] = f(0.1, dm)
    sd.update(_ssm_state(r, dm, N, prefix + "ssm."))
    sd[prefix + "ffn.0.weight"] = f(dm ** -0.5, dm * EXPAND, dm)
    sd[prefix + "ffn.0.bias"] = f(0.1, dm * EXPAND)
    sd[prefix + "ffn.3.weight"] = f((dm * EXPAND) ** -0.5, dm, dm * EXPAND)
    sd[prefix + "ffn.3.bias"] = f(0.1, dm)
    return sd


def module_state(name):
    """Seeded float32 state_dict (numpy) of a module case, its input x (B, L, d_model) and the
    upstream gradient g of the same shape."""
    m = MODULES[name]
    r = np.random.RandomState(m["seed"])
    dm, N = m["d_model"], m["state_dim"]
    if m["kind"] == "ssm":
        sd = _ssm_state(r, dm, N)
    elif m["kind"] == "block":
        sd = _block_state(r, dm, N)
    else:
        sd = {}
        for i in range(m["layers"]):
            sd.update(_block_state(r, dm, N, f"layers.{i}."))
        sd["norm.weight"] = (1.0 + 0.1 * r.standard_normal(dm)).astype(np.float32)
        sd["norm.bias"] = (0.1 * r.standard_normal(dm)).astype(np.float32)
    f = lambda *shape: r.standard_normal(shape).astype(np.float32)  # noqa: E731
    return sd, f(m["B"], m["L"], dm), f(m["B"], m["L"], dm)


def module_grad_names(name):
    return sorted(list(module_state(name)[0]) + ["input"])


_flat = lambda v: v.reshape(-1, v.shape[-1])  # noqa: E731
_erf = np.vectorize(math.erf)


def _linear(x, W, b, grads, kW, kb):
    def back(gy):
        grads[kW] = grads.get(kW, 0.0) + _flat(gy).T @ _flat(x)
        if kb is not None:
            grads[kb] = grads.get(kb, 0.0) + _flat(gy).sum(0)
        return gy @ W
    return x @ W.T + (0.0 if b is None else b), back


def _layer_norm(x, w, b, grads, kw, kb, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    rs = 1.0 / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + eps)
    xh = (x - mu) * rs

    def back(gy):
        grads[kw] = grads.get(kw, 0.0) + _flat(gy * xh).sum(0)
        grads[kb] = grads.get(kb, 0.0) + _flat(gy).sum(0)
        gx = gy * w
        return (gx - gx.mean(-1, keepdims=True) - xh * (gx * xh).mean(-1, keepdims=True)) * rs
    return xh * w + b, back


def _dwconv(x, w, b, grads, kw, kb):
    """Causal depthwise conv (reference ssm.py:411-414): y_t = b + sum_j w[:, 0, j] x_{t + j - (K - 1)}."""
    Bsz, L, D = x.shape
    K = w.shape[2]
    xp = np.concatenate([np.zeros((Bsz, K - 1, D)), x], 1)
    y = b + sum(w[:, 0, j] * xp[:, j:j + L] for j in range(K))

    def back(gy):
        gw = np.stack([(gy * xp[:, j:j + L]).sum(axis=(0, 1)) for j in range(K)], -1)[:, None, :]
        grads[kw] = grads.get(kw, 0.0) + gw
        grads[kb] = grads.get(kb, 0.0) + gy.sum(axis=(0, 1))
        gxp = np.zeros_like(xp)
        for j in range(K):
            gxp[:, j:j + L] += gy * w[:, 0, j]
        return gxp[:, K - 1:]
    return y, back


def _gelu(x):
    cdf = 0.5 * (1.0 + _erf(x / math.sqrt(2.0)))
    return x * cdf, lambda gy: gy * (cdf + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))


def _ssm(sd, p, x, grads):
    """SelectiveSSM.forward (reference ssm.py:92-132, scan_mode "parallel") with tree_grad_f64."""
    Di, N = sd[p + "D"].shape[0], sd[p + "A_log"].shape[0]
    xz, b_in = _linear(x, sd[p + "in_proj.weight"], None, grads, p + "in_proj.weight", None)
    xp, z = xz[..., :Di], xz[..., Di:]
    bcm, b_x = _linear(xp, sd[p + "x_proj.weight"], None, grads, p + "x_proj.weight", None)
    pre, b_dt = _linear(xp, sd[p + "dt_proj.weight"], sd[p + "dt_proj.bias"], grads, p + "dt_proj.weight",
                        p + "dt_proj.bias")
    dt = SG._softplus(pre)
    A = -np.exp(sd[p + "A_log"])
    scan = lambda gy: tree_grad_f64(xp, dt, A, bcm[..., :N], bcm[..., N:], sd[p + "D"], z, gy)  # noqa: E731
    y = scan(np.zeros_like(xp))[0]
    out, b_out = _linear(y, sd[p + "out_proj.weight"], None, grads, p + "out_proj.weight", None)

    def back(gout):
        gr = scan(b_out(gout))[1]
        grads[p + "A_log"] = grads.get(p + "A_log", 0.0) + gr["dA"] * A
        grads[p + "D"] = grads.get(p + "D", 0.0) + gr["dD"]
        dxp = gr["dx"] + b_x(np.concatenate([gr["dB"], gr["dC"]], -1)) + b_dt(gr["ddt"] / (1.0 + np.exp(-pre)))
        return b_in(np.concatenate([dxp, gr["dz"]], -1))
    return out, back


def _block(sd, p, x, grads):
    """SSMBlock._forward_impl (reference ssm.py:404-427), dropout the identity (eval)."""
    n1, b_n1 = _layer_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"], grads, p + "norm1.weight", p + "norm1.bias")
    u, b_conv = _dwconv(n1, sd[p + "conv.weight"], sd[p + "conv.bias"], grads, p + "conv.weight", p + "conv.bias")
    s, b_ssm = _ssm(sd, p + "ssm.", u, grads)
    x1 = s + x
    n2, b_n2 = _layer_norm(x1, sd[p + "norm2.weight"], sd[p + "norm2.bias"], grads, p + "norm2.weight", p + "norm2.bias")
    f1, b_f1 = _linear(n2, sd[p + "ffn.0.weight"], sd[p + "ffn.0.bias"], grads, p + "ffn.0.weight", p + "ffn.0.bias")
    ge, b_ge = _gelu(f1)
    f2, b_f2 = _linear(ge, sd[p + "ffn.3.weight"], sd[p + "ffn.3.bias"], grads, p + "ffn.3.weight", p + "ffn.3.bias")

    def back(gy):
        gx1 = gy + b_n2(b_f1(b_ge(b_f2(gy))))
        return gx1 + b_n1(b_conv(b_ssm(gx1)))
    return f2 + x1, back


def module_grad_f64(name, sd=None, x=None, g=None):
    """float64 gradients of sum(module(x) * g) for every parameter and the input (key "input") of a
    MODULES case, by tree_grad_f64 and the chain rule through the torch-side layers."""
    if sd is None:
        sd, x, g = module_state(name)
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    kind, grads = MODULES[name]["kind"], {}
    if kind == "ssm":
        _, back = _ssm(sd, "", x, grads)
    elif kind == "block":
        _, back = _block(sd, "", x, grads)
    else:
        backs, h = [], x
        for i in range(MODULES[name]["layers"]):
            h, bk = _block(sd, f"layers.{i}.", h, grads)
            backs.append(bk)
        _, bk = _layer_norm(h, sd["norm.weight"], sd["norm.bias"], grads, "norm.weight", "norm.bias")
        backs.append(bk)

        def back(gy):
            for bk in reversed(backs):
                gy = bk(gy)
            return gy
    grads["input"] = back(g)
    return grads


def main():
    import torch
    import velocity_asr
    from velocity_asr import ssm as ref_ssm

    ours = os.path.realpath(os.path.join(HERE, "..", "..", "velocity-asr_amd"))
    assert not os.path.realpath(velocity_asr.__file__).startswith(ours) and hasattr(
        ref_ssm.SelectiveSSM, "_parallel_scan") and not hasattr(ref_ssm, "selective_scan"), \
        f"{velocity_asr.__file__} is not the reference package: put the reference first on PYTHONPATH"

    def reference(c, inp, dtype):
        m = ref_ssm.SelectiveSSM(d_model=c["Di"] // 2, state_dim=c["N"], expand_ratio=2, scan_mode="parallel").to(dtype)
        t = {k: torch.from_numpy(v).to(dtype).requires_grad_() for k, v in inp.items() if v is not None and k != "g"}
        with torch.no_grad():
            m.D.copy_(t["D"])
        y = m._parallel_scan(t["x"], t["dt"], t["A"], t["B"], t["C"])
        if "z" in t:
            y = y * torch.nn.functional.silu(t["z"])
        (y * torch.from_numpy(inp["g"]).to(dtype)).sum().backward()
        # (L = 1: h = 0 whatever the inputs, and autograd leaves the gradient of A unset: zeros)
        gr = {"d" + k: (torch.zeros_like(t[k]) if t[k].grad is None else t[k].grad).numpy().astype(np.float64)
              for k in ("x", "dt", "A", "B", "C") + (("z",) if "z" in t else ())}
        gr["dD"] = m.D.grad.numpy().astype(np.float64)
        return gr

    out = {"names": np.array(sorted(CASES)), "modules": np.array(sorted(MODULES))}
    for name, c in CASES.items():
        inp = make_inputs(c)
        g32, g64 = reference(c, inp, torch.float32), reference(c, inp, torch.float64)
        own = tree_grad_f64(**inp)[1]
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
        print(f"{name:12s} tree_grad_f64 vs fp64 reference {worst:.2e} of gmax;  e_ref " +
              " ".join(f"{k} {float(out[f'{name}/e_ref/{k}']):.2e}" for k in GRADS if f"{name}/e_ref/{k}" in out))

    for name, mc in MODULES.items():
        sd, x, g = module_state(name)
        grads = {}
        for dtype in (torch.float32, torch.float64):
            if mc["kind"] == "ssm":
                m = ref_ssm.SelectiveSSM(d_model=mc["d_model"], state_dim=mc["state_dim"], expand_ratio=EXPAND,
                                         scan_mode="parallel")
            elif mc["kind"] == "block":
                m = ref_ssm.SSMBlock(d_model=mc["d_model"], state_dim=mc["state_dim"], expand_ratio=EXPAND,
                                     kernel_size=KERNEL_SIZE, scan_mode="parallel")
            else:
                m = ref_ssm.GlobalSSM(d_model=mc["d_model"], num_layers=mc["layers"], state_dim=mc["state_dim"])
            m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            m = m.to(dtype).eval()
            xt = torch.from_numpy(x).to(dtype).requires_grad_()
            (m(xt) * torch.from_numpy(g).to(dtype)).sum().backward()
            grads[dtype] = {k: p.grad.numpy().astype(np.float64) for k, p in m.named_parameters()}
            grads[dtype]["input"] = xt.grad.numpy().astype(np.float64)
        own = module_grad_f64(name, sd, x, g)
        assert sorted(own) == sorted(grads[torch.float64]) == sorted(module_grad_names(name))
        worst = 0.0
        for k in module_grad_names(name):
            g64 = grads[torch.float64][k]
            out[f"{name}/{k}"] = g64
            out[f"{name}/e_ref/{k}"] = np.array(float(np.abs(grads[torch.float32][k] - g64).max()), np.float64)
            out[f"{name}/gmax/{k}"] = np.array(float(np.abs(g64).max()), np.float64)
            worst = max(worst, float(np.abs(own[k] - g64).max() / np.abs(g64).max()))
        print(f"{name:12s} module_grad_f64 vs fp64 reference {worst:.2e} of gmax")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    sys.exit(main())
