#!/usr/bin/env python
"""Generate tests/golden/attn_grad.npz: the gradients of the reference's pooled cross-attention core
(MultiHeadAttention with identity projections), of its adaptive average pooling (AdaptivePool with an
identity pool_proj) and of its MultiHeadAttention and HierarchicalGlobalContext modules on seeded
cases.

Build-machine tool, run with the REFERENCE package first on the path,

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/gen_attn_grad_goldens.py

The layout is gen_tree_grad_goldens.py's.  Per case the reference runs on the CPU in float32 and in
float64 under autograd with a seeded upstream gradient g (loss = sum(out * g)); per gradient tensor k
the file holds

  <case>/e_ref/<k>   max |fp32 reference - fp64 reference|
  <case>/gmax/<k>    max |fp64 reference|
  <case>/<k>         the fp64 reference gradient in full where it has at most FULL_LIMIT elements,
                     else <case>/<k>_at (its elements at sample_index(k, size), flat) and
                     <case>/<k>_rowsum (its sums over the last axis);
  <case>/sha         SHA-256 of the regenerated float32 inputs;
  <module>/S/cross_attention.k_proj.bias
                     max over columns c of sum_{b,k} |dK[b,k,c]| (fp64): the size of the terms of that
                     cancelling sum (its value is analytically 0: softmax is shift invariant).

k is dq dK dV for ATTN cases, dx for POOL cases, and every parameter name plus "input" (and "memory"
for mha) for MODULES.  Ragged cases run the reference on utterance b alone, on its first kps[b] keys
/ lens[b] rows, and sum the parameter gradients.  The fixture only pins attn_grad_f64, pool_grad_f64
and module_grad_f64 below to the reference; the GPU tests compare the device gradients with those
three over every entry.

The helpers are our own numpy and import nothing of the reference.  Only main() imports the
reference, and asserts that it did.
"""

import hashlib
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_tree_grad_goldens as TG  # noqa: E402  (the global stack in float64: _block, _linear, _layer_norm)

OUT = os.path.join(HERE, "attn_grad.npz")
FULL_LIMIT = 1024
NSAMPLES = 128
TILE = 64  # tokens per workgroup of the attention's backward kernel: its only token-tile edge

# B = 3 unless the shape says otherwise; heads x hd
ATTN = {
    "h4x8": dict(B=3, L=37, Kp=20, heads=4, hd=8, seed=1),      # the compile-time head dims
    "h4x12": dict(B=3, L=37, Kp=20, heads=4, hd=12, seed=2),
    "h4x16": dict(B=3, L=37, Kp=20, heads=4, hd=16, seed=3),
    "h4x1": dict(B=3, L=37, Kp=20, heads=4, hd=1, seed=4),      # the runtime head dim
    "h4x5": dict(B=3, L=37, Kp=20, heads=4, hd=5, seed=5),
    "h2x32": dict(B=3, L=37, Kp=20, heads=2, hd=32, seed=6),
    "h3x12_l129": dict(B=3, L=129, Kp=16, heads=3, hd=12, seed=7),  # a head group straddling a forward block
    "kp1": dict(B=3, L=37, Kp=1, heads=4, hd=12, seed=8),       # dq = dK = 0 exactly
    "kp2": dict(B=3, L=37, Kp=2, heads=4, hd=12, seed=9),
    "kp63": dict(B=3, L=37, Kp=63, heads=4, hd=12, seed=10),
    "kp64": dict(B=3, L=37, Kp=64, heads=4, hd=12, seed=11),
    "l1": dict(B=3, L=1, Kp=16, heads=4, hd=12, seed=12),
    "l63": dict(B=3, L=63, Kp=16, heads=4, hd=12, seed=13),     # one tile: dkv written by the tile itself
    "l64": dict(B=3, L=64, Kp=16, heads=4, hd=12, seed=14),
    "l65": dict(B=3, L=65, Kp=16, heads=4, hd=12, seed=15),     # two tiles: the workspace and the tile sum
    "l127": dict(B=3, L=127, Kp=16, heads=4, hd=12, seed=16),
    "l128": dict(B=3, L=128, Kp=16, heads=4, hd=12, seed=17),
    "l129": dict(B=3, L=129, Kp=16, heads=4, hd=12, seed=18),
    "workload": dict(B=2, L=501, Kp=16, heads=4, hd=12, seed=19),   # 8 tiles: the cross-tile sum
    "lds_kp32_a256": dict(B=3, L=33, Kp=32, heads=8, hd=32, seed=20),  # the K/V set at its 64 KiB limit
    "lds_kp64_a128": dict(B=3, L=33, Kp=64, heads=4, hd=32, seed=21),  # and the backward's LDS at its largest
    "ragged20": dict(B=3, L=37, Kp=20, heads=4, hd=12, seed=22, kps=[20, 1, 11]),
    "ragged64": dict(B=3, L=70, Kp=64, heads=4, hd=12, seed=23, kps=[64, 1, 37]),
    "q30": dict(B=3, L=65, Kp=64, heads=4, hd=12, seed=24, qscale=30.0),  # near one-hot softmax
}

POOL = {
    "p8_8": dict(B=3, L=8, K=8, C=5, seed=41),
    "p9_4": dict(B=3, L=9, K=4, C=5, seed=42),
    "p64_16": dict(B=3, L=64, K=16, C=5, seed=43),
    "p501_64": dict(B=2, L=501, K=64, C=16, seed=44),
    "p37_1": dict(B=3, L=37, K=1, C=5, seed=45),
    "p_ragged": dict(B=3, L=37, K=8, C=5, seed=46, lens=[37, 9, 20], ks=[8, 4, 8]),
}

MODULES = {
    "mha": dict(kind="mha", B=2, L=37, Kp=20, d_model=24, heads=4, attention_dim=48, seed=301),
    "ctx": dict(kind="ctx", B=2, L=137, d_model=16, heads=4, attention_dim=48, layers=1, state_dim=32, seed=302),
    "ctx_long": dict(kind="ctx", B=2, L=600, d_model=16, heads=4, attention_dim=48, layers=1, state_dim=32, seed=303),
    "ctx_ragged": dict(kind="ctx", B=2, L=600, lengths=[600, 137], d_model=16, heads=4, attention_dim=48, layers=1,
                       state_dim=32, seed=304),
}
KBIAS = "cross_attention.k_proj.bias"


def sha_of(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def sample_index(key, size):
    """NSAMPLES flat indices into a tensor of `size` elements, seeded by its name."""
    return np.sort(np.random.RandomState(zlib.crc32(key.encode()) & 0x7FFFFFFF).randint(0, size, size=NSAMPLES))


def store(out, key, arr):
    """The fp64 tensor in full, or its samples and last-axis sums (see the module docstring)."""
    if arr.size <= FULL_LIMIT:
        out[key] = arr
    else:
        out[key + "_at"] = arr.reshape(-1)[sample_index(key, arr.size)]
        out[key + "_rowsum"] = arr.sum(axis=-1)


def stored_error(gold, key, own):
    """max |own - stored| over what store() kept of a tensor, the row sums per term."""
    if key in gold.files:
        return float(np.abs(own - gold[key]).max())
    at = float(np.abs(own.reshape(-1)[sample_index(key, own.size)] - gold[key + "_at"]).max())
    return max(at, float(np.abs(own.sum(axis=-1) - gold[key + "_rowsum"]).max()) / own.shape[-1])


# ------------------------------------------------------------------ the two operators
def attn_inputs(c):
    """float32 q (B, L, A), k, v (B, Kp, A) and upstream g (B, L, A) ~ N(0, 1); q times qscale."""
    r = np.random.RandomState(c["seed"])
    A = c["heads"] * c["hd"]
    f = lambda *shape: r.standard_normal(shape).astype(np.float32)  # noqa: E731
    q, k, v, g = f(c["B"], c["L"], A), f(c["B"], c["Kp"], A), f(c["B"], c["Kp"], A), f(c["B"], c["L"], A)
    return dict(q=(q * np.float32(c.get("qscale", 1.0))), k=k, v=v, g=g)


def attn_grad_f64(q, k, v, g, heads, kps=None):
    """softmax(q k^T / sqrt(hd)) v per head and its gradients in float64 (the kernels' mathematics):
    returns (out, p (B, H, L, Kp), dict of dq dK dV).  kps: utterance b uses its first kps[b] keys."""
    q, k, v, g = (np.asarray(a, np.float64) for a in (q, k, v, g))
    B, L, A = q.shape
    Kp, hd = k.shape[1], A // heads
    qh, kh, vh, gh = (a.reshape(a.shape[0], a.shape[1], heads, hd) for a in (q, k, v, g))
    s = np.einsum("blhd,bkhd->bhlk", qh, kh) / np.sqrt(hd)
    if kps is not None:
        dead = np.arange(Kp)[None, :] >= np.asarray(kps)[:, None]  # (B, Kp)
        s = np.where(dead[:, None, None, :], -np.inf, s)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)
    out = np.einsum("bhlk,bkhd->blhd", p, vh).reshape(B, L, A)
    dP = np.einsum("blhd,bkhd->bhlk", gh, vh)
    dS = p * (dP - (p * dP).sum(axis=-1, keepdims=True))
    grads = dict(dq=np.einsum("bhlk,bkhd->blhd", dS, kh).reshape(B, L, A) / np.sqrt(hd),
                 dK=np.einsum("bhlk,blhd->bkhd", dS, qh).reshape(B, Kp, A) / np.sqrt(hd),
                 dV=np.einsum("bhlk,blhd->bkhd", p, gh).reshape(B, Kp, A))
    return out, p, grads


def attn_case_f64(name):
    """(inputs, fp64 gradients) of an ATTN case."""
    c = ATTN[name]
    inp = attn_inputs(c)
    return inp, attn_grad_f64(inp["q"], inp["k"], inp["v"], inp["g"], c["heads"], c.get("kps"))[2]


def pool_matrix(L, K):
    """(K, L): row i the weights 1 / (e_i - s_i) on [s_i, e_i) = [floor(i L / K), ceil((i + 1) L / K))."""
    P = np.zeros((K, L))
    for i in range(K):
        s, e = (i * L) // K, -((-(i + 1) * L) // K)
        P[i, s:e] = 1.0 / (e - s)
    return P


def pool_f64(x, K, lens=None, ks=None):
    """Adaptive average pooling (B, L, C) -> (B, K, C) in float64; bins past ks[b] are 0."""
    x = np.asarray(x, np.float64)
    out = np.zeros((x.shape[0], K, x.shape[2]))
    for b in range(x.shape[0]):
        Lb, Kb = (x.shape[1], K) if lens is None else (lens[b], ks[b])
        out[b, :Kb] = pool_matrix(Lb, Kb) @ x[b, :Lb]
    return out


def pool_grad_f64(g, L, lens=None, ks=None):
    """d x (B, L, C) of pool_f64 from g (B, K, C): rows past lens[b] are 0, bins past ks[b] unread."""
    g = np.asarray(g, np.float64)
    dx = np.zeros((g.shape[0], L, g.shape[2]))
    for b in range(g.shape[0]):
        Lb, Kb = (L, g.shape[1]) if lens is None else (lens[b], ks[b])
        dx[b, :Lb] = pool_matrix(Lb, Kb).T @ g[b, :Kb]
    return dx


def pool_inputs(c):
    r = np.random.RandomState(c["seed"])
    f = lambda *shape: r.standard_normal(shape).astype(np.float32)  # noqa: E731
    return dict(x=f(c["B"], c["L"], c["C"]), g=f(c["B"], c["K"], c["C"]))


# ------------------------------------------------------------------ modules
def _lin_state(r, prefix, n_out, n_in):
    return {prefix + ".weight": (n_in ** -0.5 * r.standard_normal((n_out, n_in))).astype(np.float32),
            prefix + ".bias": (0.1 * r.standard_normal(n_out)).astype(np.float32)}


def _mha_state(r, dm, A, prefix=""):
    sd = {}
    for n in ("q_proj", "k_proj", "v_proj"):
        sd.update(_lin_state(r, prefix + n, A, dm))
    sd.update(_lin_state(r, prefix + "out_proj", dm, A))
    return sd


def module_state(name):
    """Seeded float32 state_dict (numpy) of a module case and its tensors: mha -> (sd, query, memory,
    g), ctx -> (sd, x, g); a ragged case's x and g are zero past each utterance's length."""
    m = MODULES[name]
    r = np.random.RandomState(m["seed"])
    dm, A = m["d_model"], m["attention_dim"]
    f = lambda *shape: r.standard_normal(shape).astype(np.float32)  # noqa: E731
    if m["kind"] == "mha":
        sd = _mha_state(r, dm, A)
        return sd, f(m["B"], m["L"], dm), f(m["B"], m["Kp"], dm), f(m["B"], m["L"], dm)
    sd = _lin_state(r, "pool1.pool_proj", dm, dm)
    for i in range(m["layers"]):
        sd.update(TG._block_state(r, dm, m["state_dim"], f"global_ssm.layers.{i}."))
    for n in ("global_ssm.norm", "norm1", "norm2"):
        sd[n + ".weight"] = (1.0 + 0.1 * r.standard_normal(dm)).astype(np.float32)
        sd[n + ".bias"] = (0.1 * r.standard_normal(dm)).astype(np.float32)
    sd.update(_lin_state(r, "pool2.pool_proj", dm, dm))
    sd.update(_mha_state(r, dm, A, "cross_attention."))
    sd.update(_lin_state(r, "fusion.gate_proj.0", dm, 2 * dm))
    for n in ("local_proj", "global_proj", "out_proj"):
        sd.update(_lin_state(r, "fusion." + n, dm, dm))
    x, g = f(m["B"], m["L"], dm), f(m["B"], m["L"], dm)
    for b, n in enumerate(m.get("lengths", [])):
        x[b, n:] = 0.0
        g[b, n:] = 0.0
    return sd, x, g


def module_grad_names(name):
    return sorted(list(module_state(name)[0]) + ["input"] + (["memory"] if MODULES[name]["kind"] == "mha" else []))


def pool_sizes(L):
    """(K1, K2) of the two pooling levels at L tokens (reference attention.py:37-44, :64-67)."""
    k1 = min(max(64, L // 8), L)
    return k1, min(min(64, max(16, k1 // 4)), k1)


def _mha(sd, p, query, memory, heads, grads, extra):
    """MultiHeadAttention.forward (reference attention.py:116-164, eval) with key = value = memory."""
    q, b_q = TG._linear(query, sd[p + "q_proj.weight"], sd[p + "q_proj.bias"], grads, p + "q_proj.weight", p + "q_proj.bias")
    k, b_k = TG._linear(memory, sd[p + "k_proj.weight"], sd[p + "k_proj.bias"], grads, p + "k_proj.weight", p + "k_proj.bias")
    v, b_v = TG._linear(memory, sd[p + "v_proj.weight"], sd[p + "v_proj.bias"], grads, p + "v_proj.weight", p + "v_proj.bias")
    o = attn_grad_f64(q, k, v, np.zeros_like(q), heads)[0]
    out, b_o = TG._linear(o, sd[p + "out_proj.weight"], sd[p + "out_proj.bias"], grads, p + "out_proj.weight",
                          p + "out_proj.bias")

    def back(gy):
        gr = attn_grad_f64(q, k, v, b_o(gy), heads)[2]
        extra["S"] = extra.get("S", 0.0) + np.abs(gr["dK"]).sum(axis=(0, 1))
        return b_q(gr["dq"]), b_k(gr["dK"]) + b_v(gr["dV"])
    return out, back


def _ctx(sd, x, m, grads, extra):
    """HierarchicalGlobalContext.forward (reference attention.py:283-319, eval) on a full-length batch."""
    L = x.shape[1]
    k1, k2 = pool_sizes(L)
    p1, b_p1 = TG._linear(pool_f64(x, k1), sd["pool1.pool_proj.weight"], sd["pool1.pool_proj.bias"], grads,
                          "pool1.pool_proj.weight", "pool1.pool_proj.bias")
    backs, h = [], p1
    for i in range(m["layers"]):
        h, bk = TG._block(sd, f"global_ssm.layers.{i}.", h, grads)
        backs.append(bk)
    hs, b_gn = TG._layer_norm(h, sd["global_ssm.norm.weight"], sd["global_ssm.norm.bias"], grads, "global_ssm.norm.weight",
                              "global_ssm.norm.bias")
    p2, b_p2 = TG._linear(pool_f64(hs, k2), sd["pool2.pool_proj.weight"], sd["pool2.pool_proj.bias"], grads,
                          "pool2.pool_proj.weight", "pool2.pool_proj.bias")
    mem, b_n1 = TG._layer_norm(p2, sd["norm1.weight"], sd["norm1.bias"], grads, "norm1.weight", "norm1.bias")
    qry, b_n2 = TG._layer_norm(x, sd["norm2.weight"], sd["norm2.bias"], grads, "norm2.weight", "norm2.bias")
    gc, b_att = _mha(sd, "cross_attention.", qry, mem, m["heads"], grads, extra)
    cat = np.concatenate([x, gc], -1)
    pre, b_gate = TG._linear(cat, sd["fusion.gate_proj.0.weight"], sd["fusion.gate_proj.0.bias"], grads,
                             "fusion.gate_proj.0.weight", "fusion.gate_proj.0.bias")
    gate = 1.0 / (1.0 + np.exp(-pre))
    lt, b_l = TG._linear(x, sd["fusion.local_proj.weight"], sd["fusion.local_proj.bias"], grads, "fusion.local_proj.weight",
                         "fusion.local_proj.bias")
    gt, b_g = TG._linear(gc, sd["fusion.global_proj.weight"], sd["fusion.global_proj.bias"], grads,
                         "fusion.global_proj.weight", "fusion.global_proj.bias")
    out, b_out = TG._linear(gate * lt + (1.0 - gate) * gt, sd["fusion.out_proj.weight"], sd["fusion.out_proj.bias"], grads,
                            "fusion.out_proj.weight", "fusion.out_proj.bias")

    def back(gy):
        gf = b_out(gy)
        gcat = b_gate(gf * (lt - gt) * gate * (1.0 - gate))
        D = x.shape[-1]
        gx = gcat[..., :D] + b_l(gf * gate)
        ggc = gcat[..., D:] + b_g(gf * (1.0 - gate))
        gq, gmem = b_att(ggc)
        gx = gx + b_n2(gq)
        gh = b_gn(pool_grad_f64(b_p2(b_n1(gmem)), hs.shape[1]))
        for bk in reversed(backs):
            gh = bk(gh)
        return gx + pool_grad_f64(b_p1(gh), L)
    return out, back


def module_grad_f64(name, tensors=None):
    """float64 gradients of sum(module(...) * g) for every parameter and the input(s) of a MODULES
    case, and extra = {"S": sum_{b,k} |dK| per column, "out": the module's fp64 output (rows past an
    utterance's length 0)}; a ragged case utterance by utterance at its
    own length, the parameter gradients summed."""
    m = MODULES[name]
    sd, *rest = tensors if tensors is not None else module_state(name)
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    rest = [np.asarray(v, np.float64) for v in rest]
    grads, extra = {}, {}
    if m["kind"] == "mha":
        query, memory, g = rest
        extra["out"], back = _mha(sd, "", query, memory, m["heads"], grads, extra)
        grads["input"], grads["memory"] = back(g)
        return grads, extra
    x, g = rest
    gin, extra["out"] = np.zeros_like(x), np.zeros_like(x)
    for b, n in enumerate(m["lengths"]) if "lengths" in m else [(slice(None), x.shape[1])]:
        sel = slice(b, b + 1) if "lengths" in m else b
        extra["out"][sel, :n], back = _ctx(sd, x[sel, :n], m, grads, extra)
        gin[sel, :n] = back(g[sel, :n])
    grads["input"] = gin
    return grads, extra


def main():
    import torch
    import velocity_asr
    from velocity_asr import attention as ref

    ours = os.path.realpath(os.path.join(HERE, "..", "..", "velocity-asr_amd"))
    assert not os.path.realpath(velocity_asr.__file__).startswith(ours) and not hasattr(ref, "pooled_attention") \
        and not hasattr(ref.MultiHeadAttention, "forward_differentiable"), \
        f"{velocity_asr.__file__} is not the reference package: put the reference first on PYTHONPATH"

    out = {"attn": np.array(sorted(ATTN)), "pool": np.array(sorted(POOL)), "modules": np.array(sorted(MODULES))}

    def finish(name, keys, g32, g64, own, extra="", skip=None):
        worst = 0.0
        for k in keys:
            gmax = float(np.abs(g64[k]).max())
            out[f"{name}/e_ref/{k}"] = np.array(float(np.abs(g32[k] - g64[k]).max()), np.float64)
            out[f"{name}/gmax/{k}"] = np.array(gmax, np.float64)
            store(out, f"{name}/{k}", g64[k])
            if k != skip:  # (the cancelling sum: reported against S by the caller)
                worst = max(worst, float(np.abs(own[k] - g64[k]).max()) / max(gmax, 1e-300))
        rel = max(float(out[f"{name}/e_ref/{k}"]) / max(float(out[f"{name}/gmax/{k}"]), 1e-300) for k in keys if k != skip)
        print(f"{name:14s} own fp64 vs fp64 reference {worst:.2e} of gmax;  worst e_ref / gmax {rel:.2e}{extra}")

    # ---- the attention core: identity projections, separate key and value tensors
    def ref_attn(c, inp, dtype):
        A = c["heads"] * c["hd"]
        m = ref.MultiHeadAttention(d_model=A, num_heads=c["heads"], attention_dim=A, dropout=0.1).to(dtype).eval()
        with torch.no_grad():
            for lin in (m.q_proj, m.k_proj, m.v_proj, m.out_proj):
                lin.weight.copy_(torch.eye(A, dtype=dtype))
                lin.bias.zero_()
        gr = {k: np.zeros(inp[n].shape) for k, n in (("dq", "q"), ("dK", "k"), ("dV", "v"))}
        kps = c.get("kps")
        for b in range(c["B"]) if kps else [slice(None)]:
            sel = slice(b, b + 1) if kps else b
            nk = kps[b] if kps else c["Kp"]
            q, k, v = (torch.from_numpy(inp[n][sel]).to(dtype) for n in "qkv")
            q, k, v = q.requires_grad_(), k[:, :nk].clone().requires_grad_(), v[:, :nk].clone().requires_grad_()
            (m(q, k, v) * torch.from_numpy(inp["g"][sel]).to(dtype)).sum().backward()
            gr["dq"][sel] = q.grad.numpy()
            gr["dK"][sel, :nk] = k.grad.numpy()
            gr["dV"][sel, :nk] = v.grad.numpy()
        return gr

    for name, c in ATTN.items():
        inp = attn_inputs(c)
        out[f"{name}/sha"] = sha_of([inp[k] for k in "qkvg"])
        finish(name, ("dq", "dK", "dV"), ref_attn(c, inp, torch.float32), ref_attn(c, inp, torch.float64),
               attn_case_f64(name)[1])

    # ---- the pooling: AdaptivePool's F.adaptive_avg_pool1d call path, pool_proj the identity
    def ref_pool(c, inp, dtype):
        m = ref.AdaptivePool(level=1, d_model=c["C"]).to(dtype).eval()
        with torch.no_grad():
            m.pool_proj.weight.copy_(torch.eye(c["C"], dtype=dtype))
            m.pool_proj.bias.zero_()
        dx = np.zeros(inp["x"].shape)
        for b in range(c["B"]) if "lens" in c else [slice(None)]:
            sel = slice(b, b + 1) if "lens" in c else b
            n, K = (c["lens"][b], c["ks"][b]) if "lens" in c else (c["L"], c["K"])
            m._compute_pool_size = lambda seq_len, prev=None, K=K: K  # the case's size, not the model's rule
            x = torch.from_numpy(inp["x"][sel, :n]).to(dtype).requires_grad_()
            y, size = m(x)
            assert size == K and y.shape[1] == K
            (y * torch.from_numpy(inp["g"][sel, :K]).to(dtype)).sum().backward()
            dx[sel, :n] = x.grad.numpy()
        return dict(dx=dx)

    for name, c in POOL.items():
        inp = pool_inputs(c)
        out[f"{name}/sha"] = sha_of([inp["x"], inp["g"]])
        finish(name, ("dx",), ref_pool(c, inp, torch.float32), ref_pool(c, inp, torch.float64),
               dict(dx=pool_grad_f64(inp["g"], c["L"], c.get("lens"), c.get("ks"))))

    # ---- modules
    def ref_module(mc, tensors, dtype):
        sd, *rest = tensors
        if mc["kind"] == "mha":
            m = ref.MultiHeadAttention(d_model=mc["d_model"], num_heads=mc["heads"], attention_dim=mc["attention_dim"])
        else:
            m = ref.HierarchicalGlobalContext(d_model=mc["d_model"], num_heads=mc["heads"],
                                              attention_dim=mc["attention_dim"], global_ssm_layers=mc["layers"],
                                              global_ssm_state_dim=mc["state_dim"])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        m = m.to(dtype).eval()
        if mc["kind"] == "mha":
            query, memory, g = (torch.from_numpy(v).to(dtype) for v in rest)
            query, memory = query.requires_grad_(), memory.requires_grad_()
            (m(query, memory, memory) * g).sum().backward()
            gr = {"input": query.grad.numpy().astype(np.float64), "memory": memory.grad.numpy().astype(np.float64)}
        else:
            x, g = rest
            gin = np.zeros(x.shape)
            for b, n in enumerate(mc["lengths"]) if "lengths" in mc else [(slice(None), x.shape[1])]:
                sel = slice(b, b + 1) if "lengths" in mc else b
                xt = torch.from_numpy(x[sel, :n]).to(dtype).requires_grad_()
                (m(xt) * torch.from_numpy(g[sel, :n]).to(dtype)).sum().backward()  # .grad accumulates over b
                gin[sel, :n] = xt.grad.numpy()
            gr = {"input": gin}
        gr.update({k: p.grad.numpy().astype(np.float64) for k, p in m.named_parameters()})
        return gr

    for name, mc in MODULES.items():
        tensors = module_state(name)
        out[f"{name}/sha"] = sha_of(tensors[1:])
        g32, g64 = ref_module(mc, tensors, torch.float32), ref_module(mc, tensors, torch.float64)
        own, extra = module_grad_f64(name, tensors)
        assert sorted(own) == sorted(g64) == module_grad_names(name), name
        kb = KBIAS if mc["kind"] == "ctx" else "k_proj.bias"
        out[f"{name}/S/{kb}"] = np.array(float(extra["S"].max()), np.float64)
        finish(name, module_grad_names(name), g32, g64, own, skip=kb, extra=
               f";  {kb}: |fp64| {float(np.abs(g64[kb]).max()):.1e} e_ref {float(np.abs(g32[kb] - g64[kb]).max()):.1e} "
               f"S {float(extra['S'].max()):.1e}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    sys.exit(main())
