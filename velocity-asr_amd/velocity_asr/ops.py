"""Thin tensor-level wrappers over the HIP kernels of libvasr_hip.so.

Each wrapper validates device / dtype / layout on the host (raising ValueError or
RuntimeError like torch would), allocates its output with the torch caching allocator
and enqueues the kernel on the current HIP stream.  Nothing here computes on the CPU.
"""

from __future__ import annotations

import math
import os
import weakref
from typing import Optional, Tuple

import torch

from . import _lib as L
from ._lib import GemmArgs, check, ptr, stream_of

LOG2E = 1.4426950408889634

# Optional per-launch timing (bench.py roofline): while `_timing` is a dict, every launch of
# a timed op records a (start, end, info) triple of HIP events on the launch stream.
_timing = None


class kernel_timer:
    """Context manager: record HIP events around every launch of the named ops."""

    def __init__(self, *names):
        self.names = set(names)
        self.records = {n: [] for n in names}

    def __enter__(self):
        global _timing
        _timing = self
        return self

    def __exit__(self, *exc):
        global _timing
        _timing = None
        return False

    def summary(self):
        torch.cuda.synchronize()
        return {n: [(s.elapsed_time(e) * 1e-3, info) for s, e, info in recs] for n, recs in self.records.items()}


def _t0(name):
    if _timing is not None and name in _timing.names:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev
    return None


def _t1(name, start, info):
    if start is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        _timing.records[name].append((start, ev, info))


def _cuda_f32(name: str, t: torch.Tensor) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if t.device.type != "cuda":
        raise RuntimeError(
            f"{name}: tensor is on {t.device}; velocity_asr (MI355X build) runs on HIP devices only")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")


def _cuda_w(name: str, t: torch.Tensor) -> None:
    """GEMM weights: float32 (fp32 GEMM) or bfloat16 (bf16 model, vasr_linear_bf16)."""
    if isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16 and t.device.type == "cuda":
        return
    _cuda_f32(name, t)


def _dropper(cache: dict, key: int):
    """Weakref callback that drops `key` from `cache`.  The dict is bound into the closure (not
    looked up as a module global): at interpreter exit the module's globals are cleared before
    the last tensors die, and a global lookup then raised inside the callback."""
    def drop(_ref, cache=cache, key=key):
        cache.pop(key, None)
    return drop


# fp32 copies of bf16 parameters for the kernels that take fp32 operands (norm weights, biases,
# conv taps, D, tables): built once per (tensor, version), dropped with the tensor.
_f32_copies = {}


def f32(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """t itself if float32 (or None), else a cached float32 copy (bf16 models)."""
    if t is None or t.dtype == torch.float32:
        return t
    sig = (t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride()))
    ent = _f32_copies.get(id(t))
    if ent is not None and ent[0]() is t and ent[1] == sig:
        return ent[2]
    with torch.no_grad():
        c = t.detach().float().contiguous()
    key = id(t)
    _f32_copies[key] = (weakref.ref(t, _dropper(_f32_copies, key)), sig, c)
    return c


def _rows(name: str, t: torch.Tensor) -> Tuple[int, int, int]:
    """(rows, cols, row_stride) of a 2-D row-major view with unit column stride."""
    if t.dim() != 2:
        raise ValueError(f"{name}: expected a 2-D view, got shape {tuple(t.shape)}")
    if t.stride(1) != 1 and t.shape[1] > 1:
        raise ValueError(f"{name}: columns must be contiguous")
    return t.shape[0], t.shape[1], t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


class option:
    """Set a launcher tuning option (vasr_set_option; enum vasr_option in include/vasr.h) for the
    duration of a with-block, e.g. ``with ops.option(L.OPT_SCAN_CHUNK, 16): ...``.  Options
    change work decomposition only, never the computed values."""

    def __init__(self, key: int, value: int):
        self.key, self.value = key, value

    def __enter__(self):
        prev = L.lib().vasr_set_option(self.key, self.value)
        check(min(prev, 0), "vasr_set_option")
        self.prev = prev
        return self

    def __exit__(self, *exc):
        L.lib().vasr_set_option(self.key, self.prev)
        return False


# Split-bf16 planes of weight matrices, built once per (tensor, version) and dropped with the
# tensor.  Keys are tensor identities: the model passes parameters or cached derived weights.
_splits = {}


def split_weights(w: torch.Tensor) -> torch.Tensor:
    """[3][N][Kp] bf16 planes (as int16 storage) of a (N, K) fp32 weight view."""
    N, K, ldw = _rows("split.w", w)
    sig = (w.data_ptr(), w._version, N, K, ldw)
    ent = _splits.get(id(w))
    if ent is not None and ent[0]() is w and ent[1] == sig:
        return ent[2]
    planes = torch.empty(int(L.lib().vasr_split_weights_elems(N, K)), device=w.device, dtype=torch.int16)
    check(L.lib().vasr_split_weights_bf16x3(w.data_ptr(), ldw, N, K, planes.data_ptr(), stream_of(w)),
          "vasr_split_weights_bf16x3")
    key = id(w)
    _splits[key] = (weakref.ref(w, _dropper(_splits, key)), sig, planes)
    return planes


_splits16 = {}


def split_weights16(w: torch.Tensor) -> torch.Tensor:
    """Split-bf16 planes of a (N, K) fp32 weight in the v_mfma_f32_16x16x32_bf16 fragment
    layout (the fused SSMBlock tail), built once per (tensor, version)."""
    N, K, ldw = _rows("split16.w", w)
    sig = (w.data_ptr(), w._version, N, K, ldw)
    ent = _splits16.get(id(w))
    if ent is not None and ent[0]() is w and ent[1] == sig:
        return ent[2]
    planes = torch.empty(int(L.lib().vasr_split_weights16_elems(N, K)), device=w.device, dtype=torch.int16)
    check(L.lib().vasr_split_weights16_bf16x3(w.data_ptr(), ldw, N, K, planes.data_ptr(), stream_of(w)),
          "vasr_split_weights16_bf16x3")
    key = id(w)
    _splits16[key] = (weakref.ref(w, _dropper(_splits16, key)), sig, planes)
    return planes


def pack_weights16(w: torch.Tensor) -> torch.Tensor:
    """One bf16 plane of a (N, K) bf16 weight in the v_mfma_f32_16x16x32_bf16 fragment layout
    (the bf16 model's fused SSMBlock tail), built once per (tensor, version)."""
    N, K, ldw = _rows("pack16.w", w)
    sig = (w.data_ptr(), w._version, N, K, ldw)
    ent = _splits16.get(id(w))
    if ent is not None and ent[0]() is w and ent[1] == sig:
        return ent[2]
    packed = torch.empty(int(L.lib().vasr_pack_weights16_bf16_elems(N, K)), device=w.device, dtype=torch.int16)
    check(L.lib().vasr_pack_weights16_bf16(w.data_ptr(), ldw, N, K, packed.data_ptr(), stream_of(w)),
          "vasr_pack_weights16_bf16")
    key = id(w)
    _splits16[key] = (weakref.ref(w, _dropper(_splits16, key)), sig, packed)
    return packed


def ssm_block_tail(g: torch.Tensor, x: torch.Tensor, wo: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor,
                   ln_eps: float, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused SSMBlock tail (vasr_ssm_block_tail_f32, or _bf16 for bf16 weights): out =
    ffn(LN2(g Wo^T + x)) + (g Wo^T + x) for g (M, 384) and x (M, 192) row views (d_model 192,
    FFN width 384)."""
    bf16 = wo.dtype == torch.bfloat16
    if bf16:
        if not (w1.dtype == w2.dtype == torch.bfloat16):
            raise TypeError("ssm_block_tail: mixed weight dtypes")
        ln_w, ln_b, b1, b2 = f32(ln_w), f32(ln_b), f32(b1), f32(b2)
    for n, t in (("g", g), ("x", x), ("ln_w", ln_w), ("ln_b", ln_b), ("b1", b1), ("b2", b2)) + (
            () if bf16 else (("wo", wo), ("w1", w1), ("w2", w2))):
        _cuda_f32(f"ssm_block_tail.{n}", t)
    M, E, ldg = _rows("ssm_block_tail.g", g)
    Mx, D, ldx = _rows("ssm_block_tail.x", x)
    if Mx != M or tuple(wo.shape) != (D, E) or tuple(w1.shape) != (E, D) or tuple(w2.shape) != (D, E):
        raise ValueError("ssm_block_tail: inconsistent shapes")
    if out is None:
        out = torch.empty((M, D), device=g.device, dtype=torch.float32)
    _, _, ldo = _rows("ssm_block_tail.out", out)
    prep = pack_weights16 if bf16 else split_weights16
    fn = "vasr_ssm_block_tail_bf16" if bf16 else "vasr_ssm_block_tail_f32"
    ev = _t0("ssm_tail")
    check(getattr(L.lib(), fn)(g.data_ptr(), ldg, x.data_ptr(), ldx, prep(wo).data_ptr(), ln_w.contiguous().data_ptr(),
                               ln_b.contiguous().data_ptr(), float(ln_eps), prep(w1).data_ptr(),
                               b1.contiguous().data_ptr(), prep(w2).data_ptr(), b2.contiguous().data_ptr(),
                               out.data_ptr(), ldo, M, D, E, stream_of(g)), fn)
    _t1("ssm_tail", ev, dict(M=M, D=D, E=E))
    return out


def fusion_tail(local: torch.Tensor, o: torch.Tensor, w_local: torch.Tensor, w_glob: torch.Tensor,
                b_glob: torch.Tensor, b_local: torch.Tensor, w_out: torch.Tensor, b_out: torch.Tensor,
                ln_w: torch.Tensor, ln_b: torch.Tensor, ln_eps: float, *, want_out: bool = False, rows: int = 0):
    """The gated fusion and the LayerNorm that follows it in one launch (vasr_fusion_tail_f32), fp32
    weights, d_model 192, attention dim 48: (y, out) with out = gemm(fused, w_out, b_out), fused the
    EPI_PAIR_FUSION blend of gemm(local, w_local) and o @ w_glob.T (paired rows, GatedFusion._paired),
    and y = layer_norm(out, ln_w, ln_b, ln_eps) -- both bitwise those launches'.  out is formed only
    when want_out (else None).  rows: 32 or 64 token rows per workgroup, 0 = by M."""
    for n, t in (("local", local), ("o", o), ("w_local", w_local), ("w_glob", w_glob), ("b_glob", b_glob),
                 ("b_local", b_local), ("w_out", w_out), ("b_out", b_out), ("ln_w", ln_w), ("ln_b", ln_b)):
        _cuda_f32(f"fusion_tail.{n}", t)
    M, D, ldl = _rows("fusion_tail.local", local)
    Mo, A, ldo = _rows("fusion_tail.o", o)
    if Mo != M or tuple(w_local.shape) != (2 * D, D) or tuple(w_glob.shape) != (2 * D, A) \
            or tuple(w_out.shape) != (D, D) or b_glob.numel() != 2 * D \
            or any(t.numel() != D for t in (b_local, b_out, ln_w, ln_b)):
        raise ValueError("fusion_tail: inconsistent shapes")
    y = torch.empty((M, D), device=local.device, dtype=torch.float32)
    out = torch.empty((M, D), device=local.device, dtype=torch.float32) if want_out else None
    ev = _t0("fusion_tail")
    check(L.lib().vasr_fusion_tail_f32(local.data_ptr(), ldl, o.data_ptr(), ldo, split_weights(w_local).data_ptr(),
                                       split_weights(w_glob).data_ptr(), b_glob.contiguous().data_ptr(),
                                       b_local.contiguous().data_ptr(), split_weights(w_out).data_ptr(),
                                       b_out.contiguous().data_ptr(), ln_w.contiguous().data_ptr(),
                                       ln_b.contiguous().data_ptr(), float(ln_eps), y.data_ptr(), D, ptr(out), D,
                                       M, D, A, int(rows), stream_of(local)), "vasr_fusion_tail_f32")
    _t1("fusion_tail", ev, dict(M=M, D=D, A=A))
    return y, out


def pack_bf16(w: torch.Tensor) -> torch.Tensor:
    """One fragment-native bf16 plane (as int16 storage) of a (N, K) bf16 weight view."""
    N, K, ldw = _rows("pack.w", w)
    sig = (w.data_ptr(), w._version, N, K, ldw)
    ent = _splits.get(id(w))
    if ent is not None and ent[0]() is w and ent[1] == sig:
        return ent[2]
    packed = torch.empty(int(L.lib().vasr_pack_weights_bf16_elems(N, K)), device=w.device, dtype=torch.int16)
    check(L.lib().vasr_pack_weights_bf16(w.data_ptr(), ldw, N, K, packed.data_ptr(), stream_of(w)),
          "vasr_pack_weights_bf16")
    key = id(w)
    _splits[key] = (weakref.ref(w, _dropper(_splits, key)), sig, packed)
    return packed


def _linear(args: GemmArgs, w: torch.Tensor, stream) -> None:
    if w.dtype == torch.bfloat16:
        check(L.lib().vasr_linear_bf16(args, pack_bf16(w).data_ptr(), stream), "vasr_linear_bf16")
    else:
        check(L.lib().vasr_linear_x3_f32(args, split_weights(w).data_ptr(), stream), "vasr_linear_x3_f32")


def gemm_tile(M: int, N: int, K: int, *, batch: int = 1, epilogue: int = L.EPI_NONE, bf16: bool = False) -> int:
    """The kernel a gemm / gemm_batched call of this shape launches under the current options
    (vasr_gemm_tile; host only): 128128, 128064 or 64064 for the tile kernels, 1 for the rows
    engine.  bf16: the call passes bf16 weights."""
    k = L.lib().vasr_gemm_tile(int(M), int(N), int(K), int(batch), int(epilogue), int(bool(bf16)))
    check(min(k, 0), "vasr_gemm_tile")
    return k


def _ln_prologue(a: torch.Tensor, ln) -> torch.Tensor:
    """Row LayerNorm of `a` (vasr_layer_norm_f32) when ln = (weight, bias, eps) is given: the
    LayerNorm feeding a Linear (SSMBlock norm2 -> FFN, the CTC head).  Returns the A the GEMM
    reads.  (Fusing it into the GEMM's A read was bit-identical but slower end to end, 99.5k vs
    102.5k RTFx; removed in r03)"""
    if ln is None:
        return a
    ln_w, ln_b, eps = ln
    return layer_norm(a, f32(ln_w), f32(ln_b), eps)


def _qp(qparams: Optional[torch.Tensor], cols: int) -> Optional[int]:
    if qparams is None:
        return None
    _cuda_f32("gemm.qparams", qparams)
    if not qparams.is_contiguous() or tuple(qparams.shape) != (cols, 4):
        raise ValueError(f"gemm: qparams must be a contiguous ({cols}, 4) tensor, got {tuple(qparams.shape)}")
    return qparams.data_ptr()


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, epilogue: int = L.EPI_NONE,
         out: Optional[torch.Tensor] = None, aux: Optional[torch.Tensor] = None,
         aux2: Optional[torch.Tensor] = None, n_out: int = 0, n_cols_out: Optional[int] = None,
         qparams: Optional[torch.Tensor] = None, ln=None) -> torch.Tensor:
    """out = epilogue(fq(a @ w.T + bias)) for a (M, K) row view and w (N, K); fq is the
    per-column activation fake-quant of `qparams` ((ncols, 4) {scale, zp, qmin, qmax}) if given.
    ln = (weight, bias, eps): LayerNorm each row of `a` first."""
    _cuda_f32("gemm.a", a)
    args = GemmArgs()
    a = _ln_prologue(a, ln)
    _cuda_w("gemm.w", w)
    bias, aux, aux2 = f32(bias), f32(aux), f32(aux2)
    M, K, lda = _rows("gemm.a", a)
    N, Kw, ldw = _rows("gemm.w", w)
    if Kw != K:
        raise ValueError(f"gemm: a has K={K} but w has K={Kw}")
    cols = n_cols_out if n_cols_out is not None else (n_out if epilogue in (L.EPI_PAIR_POWER, L.EPI_PAIR_FUSION) else N)
    if out is None:
        out = torch.empty((M, cols), device=a.device, dtype=torch.float32)
    _, _, ldc = _rows("gemm.out", out)
    args.A, args.lda, args.stride_a = a.data_ptr(), lda, 0
    args.W, args.ldw = w.data_ptr(), ldw
    args.bias = ptr(bias)
    args.C, args.ldc, args.stride_c = out.data_ptr(), ldc, 0
    args.batch, args.M, args.N, args.K = 1, M, N, K
    args.epilogue = epilogue
    if aux is not None:
        _, _, ld_aux = _rows("gemm.aux", aux)
        args.aux, args.ld_aux, args.stride_aux = aux.data_ptr(), ld_aux, 0
    args.aux2 = ptr(aux2)
    args.n_out = n_out
    args.qparams = _qp(qparams, N + (n_out if epilogue == L.EPI_PAIR_FUSION else 0))
    ev = _t0("gemm")
    _linear(args, w, stream_of(a))
    _t1("gemm", ev, dict(M=M, N=N, K=K, batch=1))
    return out


def _gemm_argmax_keys(a: torch.Tensor, w: torch.Tensor, bias, qparams, ln, who: str):
    """The VASR_EPI_ARGMAX GEMM: (M, ceil(N/32)) uint64 partial keys of a @ w.T + bias per row."""
    _cuda_f32(f"{who}.a", a)
    args = GemmArgs()
    a = _ln_prologue(a, ln)
    _cuda_w(f"{who}.w", w)
    bias = f32(bias)
    M, K, lda = _rows(f"{who}.a", a)
    N, Kw, ldw = _rows(f"{who}.w", w)
    if Kw != K:
        raise ValueError(f"{who}: a has K={K} but w has K={Kw}")
    slots = (N + 31) // 32
    keys = torch.empty((M, slots), device=a.device, dtype=torch.int64)  # every slot is written
    args.A, args.lda, args.stride_a = a.data_ptr(), lda, 0
    args.W, args.ldw = w.data_ptr(), ldw
    args.bias = ptr(bias)
    args.C, args.ldc, args.stride_c = keys.data_ptr(), slots, 0
    args.batch, args.M, args.N, args.K = 1, M, N, K
    args.epilogue = L.EPI_ARGMAX
    args.qparams = _qp(qparams, N)
    ev = _t0("gemm")
    _linear(args, w, stream_of(a))
    _t1("gemm", ev, dict(M=M, N=N, K=K, batch=1))
    return keys, slots, M


def gemm_argmax(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
                qparams: Optional[torch.Tensor] = None, ln=None) -> torch.Tensor:
    """int32 argmax over the N outputs of a @ w.T + bias (after qparams) per row, fused into the
    GEMM epilogue (VASR_EPI_ARGMAX): the (M, N) product is never written.  Ties -> first index.
    ln = (weight, bias, eps): LayerNorm each row of `a` first."""
    keys, slots, M = _gemm_argmax_keys(a, w, bias, qparams, ln, "gemm_argmax")
    out = torch.empty(M, device=a.device, dtype=torch.int32)
    check(L.lib().vasr_argmax_keys(keys.data_ptr(), slots, slots, M, out.data_ptr(), stream_of(keys)), "vasr_argmax_keys")
    return out


def gemm_ctc_greedy(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], B: int, blank: int = 0, *,
                    qparams: Optional[torch.Tensor] = None, ln=None, collapse: bool = True, timestamps: bool = False,
                    out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, frames: Optional[torch.Tensor] = None):
    """Greedy CTC decode of B utterances (a: B * L rows) straight from the argmax GEMM's keys:
    argmax + collapse in one launch (vasr_ctc_collapse_keys); same results as gemm_argmax then
    ctc_collapse.  Returns (tokens, lengths, start, end) as ctc_collapse."""
    keys, slots, M = _gemm_argmax_keys(a, w, bias, qparams, ln, "gemm_ctc_greedy")
    if B <= 0 or M % B:
        raise ValueError(f"gemm_ctc_greedy: {M} rows do not split into B={B} utterances")
    Lq = M // B
    toks, lens, st, en, frames = _collapse_outputs("gemm_ctc_greedy", B, Lq, keys.device, out, timestamps, frames)
    check(L.lib().vasr_ctc_collapse_keys(keys.data_ptr(), slots, slots, B, Lq, ptr(frames), int(blank), int(collapse),
                                         None, toks.data_ptr(), lens.data_ptr(), ptr(st), ptr(en), stream_of(keys)),
          "vasr_ctc_collapse_keys")
    return toks, lens, st, en


def gemm_batched(a_base: torch.Tensor, lda: int, stride_a: int, rows: int, batch: int, K: int, w: torch.Tensor,
                 bias: Optional[torch.Tensor], out: torch.Tensor, ldc: int, stride_c: int, *,
                 epilogue: int = L.EPI_NONE, aux: Optional[torch.Tensor] = None, ld_aux: int = 0,
                 stride_aux: int = 0, n_out: int = 0, qparams: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Strided batched form: A[b] rows at a_base + b*stride_a + m*lda (overlapping rows allowed)."""
    _cuda_f32("gemm_batched.a", a_base)
    _cuda_w("gemm_batched.w", w)
    bias, aux = f32(bias), f32(aux)
    need = (batch - 1) * stride_a + (rows - 1) * lda + K
    avail = a_base.untyped_storage().nbytes() // 4 - a_base.storage_offset()
    if rows > 0 and batch > 0 and need > avail:
        raise ValueError(f"gemm_batched: A view needs {need} elements, {avail} available")
    N, Kw, ldw = _rows("gemm_batched.w", w)
    if Kw != K:
        raise ValueError("gemm_batched: K mismatch")
    args = GemmArgs()
    args.A, args.lda, args.stride_a = a_base.data_ptr(), lda, stride_a
    args.W, args.ldw = w.data_ptr(), ldw
    args.bias = ptr(bias)
    args.C, args.ldc, args.stride_c = out.data_ptr(), ldc, stride_c
    args.batch, args.M, args.N, args.K = batch, rows, N, K
    args.epilogue = epilogue
    if aux is not None:
        args.aux, args.ld_aux, args.stride_aux = aux.data_ptr(), ld_aux, stride_aux
    args.n_out = n_out
    args.qparams = _qp(qparams, N)
    ev = _t0("gemm")
    _linear(args, w, stream_of(a_base))
    _t1("gemm", ev, dict(M=rows, N=N, K=K, batch=batch))
    return out


def layer_norm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float = 1e-5,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _cuda_f32("layer_norm.x", x)
    w, b = f32(w), f32(b)
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    rows, _, ldx = _rows("layer_norm.x", x2)
    y = torch.empty((rows, C), device=x.device, dtype=torch.float32) if out is None else out.reshape(-1, C)
    _, _, ldy = _rows("layer_norm.out", y)
    check(L.lib().vasr_layer_norm_f32(x2.data_ptr(), ldx, w.data_ptr(), b.data_ptr(), y.data_ptr(), ldy, rows, C,
                                      float(eps), stream_of(x)), "vasr_layer_norm_f32")
    return y.view(*x.shape[:-1], C) if out is None else out


def layer_norm_pair(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, eps1: float, w2: torch.Tensor,
                    b2: torch.Tensor, eps2: float):
    """(LN1(x), LN2(LN1(x))) in one launch, each bitwise layer_norm's (vasr_layer_norm_pair_f32)."""
    _cuda_f32("layer_norm_pair.x", x)
    w1, b1, w2, b2 = f32(w1), f32(b1), f32(w2), f32(b2)
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    rows, _, ldx = _rows("layer_norm_pair.x", x2)
    y1 = torch.empty((rows, C), device=x.device, dtype=torch.float32)
    y2 = torch.empty((rows, C), device=x.device, dtype=torch.float32)
    check(L.lib().vasr_layer_norm_pair_f32(x2.data_ptr(), ldx, w1.data_ptr(), b1.data_ptr(), float(eps1),
                                           y1.data_ptr(), C, w2.data_ptr(), b2.data_ptr(), float(eps2),
                                           y2.data_ptr(), C, rows, C, stream_of(x)), "vasr_layer_norm_pair_f32")
    return y1.view(*x.shape[:-1], C), y2.view(*x.shape[:-1], C)


def add_table(x: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """x (B, L, C) + table (L, C) broadcast over the batch."""
    _cuda_f32("add_table.x", x)
    table = f32(table)
    _cuda_f32("add_table.table", table)
    x = x.contiguous()
    B, Lq, C = x.shape
    if tuple(table.shape) != (Lq, C):
        raise ValueError("add_table: table must be (L, C)")
    out = torch.empty_like(x)
    check(L.lib().vasr_add_table_f32(x.data_ptr(), table.contiguous().data_ptr(), out.data_ptr(), B, Lq, C,
                                     stream_of(x)), "vasr_add_table_f32")
    return out


def ln_dwconv(x: torch.Tensor, ln_w, ln_b, conv_w, conv_b, eps: float = 1e-5) -> torch.Tensor:
    """(B, L, C) -> causal depthwise conv of LayerNorm(x)."""
    _cuda_f32("ln_dwconv.x", x)
    ln_w, ln_b, conv_w, conv_b = f32(ln_w), f32(ln_b), f32(conv_w), f32(conv_b)
    x = x.contiguous()
    B, Lq, C = x.shape
    Kc = conv_w.shape[-1]
    y = torch.empty_like(x)
    check(L.lib().vasr_ln_dwconv_f32(x.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(),
                                     conv_w.contiguous().data_ptr(), conv_b.data_ptr(), y.data_ptr(), B, Lq, C, Kc,
                                     float(eps), stream_of(x)), "vasr_ln_dwconv_f32")
    return y


def ln_dwconv_prenorm(x: torch.Tensor, pre_w, pre_b, pre_eps: float, ln_w, ln_b, conv_w, conv_b,
                      eps: float = 1e-5):
    """(B, L, 192) -> (ln_dwconv(LN0(x)), LN0(x)) without LN0's own launch (vasr_ln_dwconv_prenorm_f32):
    both bitwise layer_norm + ln_dwconv.  Kc = 4 only."""
    _cuda_f32("ln_dwconv_prenorm.x", x)
    pre_w, pre_b = f32(pre_w), f32(pre_b)
    ln_w, ln_b, conv_w, conv_b = f32(ln_w), f32(ln_b), f32(conv_w), f32(conv_b)
    x = x.contiguous()
    B, Lq, C = x.shape
    Kc = conv_w.shape[-1]
    y, xo = torch.empty_like(x), torch.empty_like(x)
    check(L.lib().vasr_ln_dwconv_prenorm_f32(x.data_ptr(), pre_w.data_ptr(), pre_b.data_ptr(), float(pre_eps),
                                             xo.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(),
                                             conv_w.contiguous().data_ptr(), conv_b.data_ptr(), y.data_ptr(), B, Lq, C,
                                             Kc, float(eps), stream_of(x)), "vasr_ln_dwconv_prenorm_f32")
    return y, xo


# Chunk-parallel tree scan (vasr_ssm_scan_chunked_f32, bitwise equal to the streaming kernel)
# for launches under CHUNKED_MAX_WAVES waves of the streaming kernel (B * Di * N / 256 at 4 states
# per lane) over more than CHUNKED_MIN_L steps: one utterance at a time, as the reference's
# scripts feed the model.  Measured (profiles/r03ae/forms.txt, graph-timed): the streaming kernel
# takes ~4.8 + 0.067 L us at these sizes whatever B; the chunked form's three launches win from
# L ~ 150 while the launch is at most 192 waves (B = 1, 10 s: 14.7 vs 37.1 us at N = 32, 18.3 vs
# 37.0 at N = 64) and lose at 384 (B = 4, N = 64: 41.9 vs 39.1) and for short L (the global
# blocks' L = 64 at 10 s: 10.2 vs 6.8 us).
# scan_form("streaming" | "chunked" | None) forces one (default from VASR_SCAN_CHUNKED=0|1).
# Below CHUNKED_MIN_L the chunked entry point still wins where it runs as ONE launch (the
# time-split form: N <= 64, B * Di * N / 128 <= 256 workgroups, L <= 512; the library reports its
# own rule, vasr_ssm_scan_split_selected), e.g. the global blocks' L = 64 at B = 1
# (VASR_SCAN_SPLIT_SHORT=0 turns this off; profiles/r05aq).
CHUNKED_MAX_WAVES = 256
CHUNKED_MIN_L = 160
_SCAN_FORM = {"0": "streaming", "1": "chunked"}.get(os.environ.get("VASR_SCAN_CHUNKED", ""))
_SPLIT_SHORT = os.environ.get("VASR_SCAN_SPLIT_SHORT", "1") != "0"


def scan_form(form: Optional[str]) -> Optional[str]:
    """Force the streaming or chunk-parallel tree scan (None = by launch size); returns the
    previous setting.  Both give bitwise equal outputs."""
    global _SCAN_FORM
    if form not in (None, "streaming", "chunked"):
        raise ValueError(f"scan form {form!r}: expected None, 'streaming' or 'chunked'")
    prev, _SCAN_FORM = _SCAN_FORM, form
    return prev


def _use_chunked(B: int, Lq: int, Di: int, N: int, mode: int) -> bool:
    if mode not in (0, 2) or Lq <= 16:
        return False
    if _SCAN_FORM is not None:
        return _SCAN_FORM == "chunked"
    if _SPLIT_SHORT and _split_form(B, Lq, Di, N):
        return True
    return B * Di * N // 256 < CHUNKED_MAX_WAVES and Lq > CHUNKED_MIN_L


def _split_form(B: int, Lq: int, Di: int, N: int) -> bool:
    """vasr_ssm_scan_chunked_f32 runs this launch as one (the time-split form) under the current
    options: the library's own rule (vasr_ssm_scan_split_selected), not a copy of it."""
    return bool(L.lib().vasr_ssm_scan_split_selected(B, Lq, Di, N))


SCAN_STATE_DIMS = (16, 32, 64, 128)  # the scan kernels' state dims (include/vasr.h)


def scan_state_dim(N: int) -> int:
    """The kernel state dim a state dim N runs as: N itself, or the next size up with the
    padded states zero (they stay 0 and add nothing to y)."""
    for n in SCAN_STATE_DIMS:
        if N <= n:
            return n
    raise NotImplementedError(f"selective scan: state dim {N} > {SCAN_STATE_DIMS[-1]} not supported")


def ssm_scan(xz: torch.Tensor, dt: torch.Tensor, bc: torch.Tensor, A2: torch.Tensor, D: torch.Tensor, B: int,
             Lq: int, mode: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gated selective scan.  xz (B*L, 2Di) [x|z], dt (B*L, Di), bc (B*L, 2N) [B|C] (row views).
    Small launches of the tree modes take the chunk-parallel form (same results, bitwise).
    A state dim without a kernel instance (scan_state_dim) is zero-padded here, a copy of bc
    (the model avoids it: its projection GEMM writes the padded layout, SelectiveSSM._prepared)."""
    N0 = A2.numel()
    Np = scan_state_dim(N0)
    if Np != N0:
        Bm, Cm = bc[:, :N0], bc[:, N0:2 * N0]
        pad = torch.zeros((bc.shape[0], Np - N0), device=bc.device, dtype=bc.dtype)
        bc = torch.cat([Bm, pad, Cm, pad], 1)
        A2 = torch.cat([A2, torch.zeros(Np - N0, device=A2.device, dtype=A2.dtype)])
    D = f32(D)
    for n, t in (("xz", xz), ("dt", dt), ("bc", bc), ("A2", A2), ("D", D)):
        _cuda_f32(f"ssm_scan.{n}", t)
    M, two_di, ld_xz = _rows("ssm_scan.xz", xz)
    _, Di, ld_dt = _rows("ssm_scan.dt", dt)
    _, two_n, ld_bc = _rows("ssm_scan.bc", bc)
    if M != B * Lq or two_di != 2 * Di or two_n != 2 * A2.numel() or D.numel() != Di:
        raise ValueError("ssm_scan: inconsistent shapes")
    if out is None:
        out = torch.empty((M, Di), device=xz.device, dtype=torch.float32)
    _, _, ld_out = _rows("ssm_scan.out", out)
    N = A2.numel()
    chunked = _use_chunked(B, Lq, Di, N, int(mode))
    ws = None
    if chunked:
        nws = int(L.lib().vasr_ssm_scan_workspace_floats(B, Lq, Di, N))
        ws = torch.empty(nws, device=xz.device, dtype=torch.float32)
    ev = _t0("ssm_scan")
    if chunked:
        check(L.lib().vasr_ssm_scan_chunked_f32(xz.data_ptr(), ld_xz, dt.data_ptr(), ld_dt, bc.data_ptr(), ld_bc,
                                                A2.data_ptr(), D.data_ptr(), out.data_ptr(), ld_out, B, Lq, Di, N,
                                                int(mode), ws.data_ptr(), ws.numel(), stream_of(xz)),
              "vasr_ssm_scan_chunked_f32")
    else:
        check(L.lib().vasr_ssm_scan_f32(xz.data_ptr(), ld_xz, dt.data_ptr(), ld_dt, bc.data_ptr(), ld_bc, A2.data_ptr(),
                                        D.data_ptr(), out.data_ptr(), ld_out, B, Lq, Di, N, int(mode),
                                        stream_of(xz)), "vasr_ssm_scan_f32")
    _t1("ssm_scan", ev, dict(B=B, L=Lq, Di=Di, N=N, mode=int(mode), chunked=chunked))
    return out


def ssm_scan_ungated(x: torch.Tensor, dt: torch.Tensor, bc: torch.Tensor, A2: torch.Tensor, D: torch.Tensor, B: int,
                     Lq: int, mode: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The ungated tree scan (vasr_ssm_scan_ungated_f32, modes 0 / 2): y + x D for x (B*L, Di),
    dt (B*L, Di), bc (B*L, 2N) row views; no z.  The z-in-tail block's scan: the streaming
    kernels with the gated entry point's lane layout, so ssm_block_tail_gated's gate gives
    bitwise ssm_scan's output (the caller keeps to shapes where ssm_scan streams too)."""
    D = f32(D)
    for n, t in (("x", x), ("dt", dt), ("bc", bc), ("A2", A2), ("D", D)):
        _cuda_f32(f"ssm_scan_ungated.{n}", t)
    M, Di, ld_x = _rows("ssm_scan_ungated.x", x)
    _, Di2, ld_dt = _rows("ssm_scan_ungated.dt", dt)
    _, two_n, ld_bc = _rows("ssm_scan_ungated.bc", bc)
    N = A2.numel()
    if M != B * Lq or Di2 != Di or two_n != 2 * N or D.numel() != Di or N not in SCAN_STATE_DIMS:
        raise ValueError("ssm_scan_ungated: inconsistent shapes")
    if out is None:
        out = torch.empty((M, Di), device=x.device, dtype=torch.float32)
    _, _, ld_out = _rows("ssm_scan_ungated.out", out)
    ev = _t0("ssm_scan")
    check(L.lib().vasr_ssm_scan_ungated_f32(x.data_ptr(), ld_x, dt.data_ptr(), ld_dt, bc.data_ptr(), ld_bc,
                                            A2.data_ptr(), D.data_ptr(), out.data_ptr(), ld_out, B, Lq, Di, N,
                                            int(mode), stream_of(x)), "vasr_ssm_scan_ungated_f32")
    _t1("ssm_scan", ev, dict(B=B, L=Lq, Di=Di, N=N, mode=int(mode), chunked=False, ungated=True))
    return out


SCAN_BWD_CHUNK = 16  # time steps per checkpoint of ssm_scan_save (include/vasr.h)


def scan_bwd_channels(N: int) -> int:
    """Channels per workgroup of the scan's backward kernel at kernel state dim N: Di must be a
    multiple (4 state indices per lane: 1024 / N)."""
    return 1024 // N


def ssm_scan_save(x: torch.Tensor, z: Optional[torch.Tensor], dt: torch.Tensor, bc: torch.Tensor, A2: torch.Tensor,
                  D: torch.Tensor, B: int, Lq: int):
    """The recurrence's forward that keeps what its backward needs (vasr_ssm_scan_save_f32).
    x, dt (B*L, Di) and bc (B*L, 2N) [B|C] row views; z: the other half of x's rows (x and z are
    views [:, :Di] and [:, Di:] of one (B*L, 2Di) tensor, as in_proj writes them) or None for the
    ungated form.  Returns (out (B*L, Di), ckpt (B, ceil(L / 16), Di, N)): out bitwise
    ssm_scan(mode=1)'s (ungated: its value before the gate), ckpt the state every chunk starts from."""
    D = f32(D)
    for n, t in (("x", x), ("dt", dt), ("bc", bc), ("A2", A2), ("D", D)) + ((("z", z),) if z is not None else ()):
        _cuda_f32(f"ssm_scan_save.{n}", t)
    M, Di, ld_xz = _rows("ssm_scan_save.x", x)
    _, Di2, ld_dt = _rows("ssm_scan_save.dt", dt)
    _, two_n, ld_bc = _rows("ssm_scan_save.bc", bc)
    N = A2.numel()
    if M != B * Lq or Di2 != Di or two_n != 2 * N or D.numel() != Di or N not in SCAN_STATE_DIMS:
        raise ValueError("ssm_scan_save: inconsistent shapes")
    if z is not None:
        _, Dz, ld_z = _rows("ssm_scan_save.z", z)
        if Dz != Di or z.shape[0] != M or ld_z != ld_xz or z.data_ptr() != x.data_ptr() + 4 * Di:
            raise ValueError("ssm_scan_save: x and z must be the two halves of one (B*L, 2Di) tensor")
        ld_xz = max(ld_xz, 2 * Di)  # a single row reports its own width
    out = torch.empty((M, Di), device=x.device, dtype=torch.float32)
    nck = int(L.lib().vasr_ssm_scan_checkpoint_floats(B, Lq, Di, N))
    ckpt = torch.empty(nck, device=x.device, dtype=torch.float32)
    ev = _t0("ssm_scan_save")
    check(L.lib().vasr_ssm_scan_save_f32(x.data_ptr(), ld_xz, dt.data_ptr(), ld_dt, bc.data_ptr(), ld_bc, A2.data_ptr(),
                                         D.data_ptr(), out.data_ptr(), Di, B, Lq, Di, N, int(z is not None),
                                         ckpt.data_ptr(), ckpt.numel(), stream_of(x)), "vasr_ssm_scan_save_f32")
    _t1("ssm_scan_save", ev, dict(B=B, L=Lq, Di=Di, N=N, gated=z is not None))
    return out, ckpt.view(B, -1, Di, N) if nck else ckpt.view(B, 0, Di, N)


def _ssm_bwd(tag: str, x, z, dt, bc, A, A2, D, g, ckpt, B: int, Lq: int, out, workspace):
    """ssm_scan_bwd (ckpt given) and ssm_tree_bwd (ckpt None): the checks, the output dict and the call."""
    tree = ckpt is None
    entry = "vasr_ssm_tree_bwd" if tree else "vasr_ssm_scan_bwd"
    D = f32(D)
    ops_ = (("x", x), ("dt", dt), ("bc", bc), ("A", A), ("A2", A2), ("D", D), ("g", g)) + (() if tree else (("ckpt", ckpt),))
    for n, t in ops_ + ((("z", z),) if z is not None else ()):
        _cuda_f32(f"{tag}.{n}", t)
    M, Di, ld_x = _rows(f"{tag}.x", x)
    _, Di2, ld_dt = _rows(f"{tag}.dt", dt)
    _, Di3, ld_g = _rows(f"{tag}.g", g)
    _, two_n, ld_bc = _rows(f"{tag}.bc", bc)
    N = A2.numel()
    if (M != B * Lq or Di2 != Di or Di3 != Di or g.shape[0] != M or two_n != 2 * N or A.numel() != N
            or D.numel() != Di or N not in SCAN_STATE_DIMS):
        raise ValueError(f"{tag}: inconsistent shapes")
    if Di % scan_bwd_channels(N):
        raise ValueError(f"{tag}: Di={Di} must be a multiple of {scan_bwd_channels(N)} at N={N}")
    ld_z = 0
    if z is not None:
        _, Dz, ld_z = _rows(f"{tag}.z", z)
        if Dz != Di or z.shape[0] != M:
            raise ValueError(f"{tag}: inconsistent shapes")
    if not tree:
        nck = int(L.lib().vasr_ssm_scan_checkpoint_floats(B, Lq, Di, N))
        if ckpt.numel() != nck or not ckpt.is_contiguous():
            raise ValueError(f"{tag}: ckpt must be ssm_scan_save's ({nck} floats)")
    dev = x.device
    if out is None:
        out = dict(dx=torch.empty((M, Di), device=dev), ddt=torch.empty((M, Di), device=dev),
                   dz=torch.empty((M, Di), device=dev) if z is not None else None,
                   dB=torch.empty((M, N), device=dev), dC=torch.empty((M, N), device=dev),
                   dA_part=torch.empty((B, Di, N), device=dev), dD_part=torch.empty((B, Di), device=dev))
    for k, shape in (("dx", (M, Di)), ("ddt", (M, Di)), ("dz", (M, Di)), ("dB", (M, N)), ("dC", (M, N)),
                     ("dA_part", (B, Di, N)), ("dD_part", (B, Di))):
        t = out[k]
        if k == "dz" and z is None:
            if t is not None:
                raise ValueError(f"{tag}: dz without z")
            continue
        _cuda_f32(f"{tag}.{k}", t)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{tag}: {k} must be contiguous {shape}")
    nws = int(getattr(L.lib(), entry + "_workspace_floats")(B, Lq, Di, N))
    if workspace is None:
        workspace = torch.empty(nws, device=dev, dtype=torch.float32)
    _cuda_f32(f"{tag}.workspace", workspace)
    ev = _t0(tag)
    check(getattr(L.lib(), entry + "_f32")(
        x.data_ptr(), ld_x, ptr(z), ld_z, dt.data_ptr(), ld_dt, bc.data_ptr(), ld_bc, A.data_ptr(), A2.data_ptr(),
        D.data_ptr(), g.data_ptr(), ld_g, *(() if tree else (ckpt.data_ptr(),)), out["dx"].data_ptr(),
        out["ddt"].data_ptr(), ptr(out["dz"]), out["dB"].data_ptr(), out["dC"].data_ptr(), out["dA_part"].data_ptr(),
        out["dD_part"].data_ptr(), workspace.data_ptr(), workspace.numel(), B, Lq, Di, N, stream_of(x)), entry + "_f32")
    _t1(tag, ev, dict(B=B, L=Lq, Di=Di, N=N, gated=z is not None))
    return out


def ssm_scan_bwd(x: torch.Tensor, z: Optional[torch.Tensor], dt: torch.Tensor, bc: torch.Tensor, A: torch.Tensor,
                 A2: torch.Tensor, D: torch.Tensor, g: torch.Tensor, ckpt: torch.Tensor, B: int, Lq: int,
                 out: Optional[dict] = None, workspace: Optional[torch.Tensor] = None):
    """The recurrence's backward (vasr_ssm_scan_bwd_f32) from ssm_scan_save's checkpoints: g (B*L, Di)
    = d loss / d out.  Returns a dict: dx, ddt, dz (None without z) (B*L, Di); dB, dC (B*L, N);
    dA_part (B, Di, N) and dD_part (B, Di), the per-(utterance, channel) sums whose totals over
    (b, d) and over b are dA and dD.  Every sum runs in a fixed order (no atomics): run-to-run
    bitwise, and an utterance's rows do not depend on the rest of the batch.  out / workspace:
    preallocated outputs (the same keys) and partial-sum workspace."""
    if ckpt is None:
        raise ValueError("ssm_scan_bwd: ckpt must be ssm_scan_save's")
    return _ssm_bwd("ssm_scan_bwd", x, z, dt, bc, A, A2, D, g, ckpt, B, Lq, out, workspace)


def ssm_tree_bwd(x: torch.Tensor, z: Optional[torch.Tensor], dt: torch.Tensor, bc: torch.Tensor, A: torch.Tensor,
                 A2: torch.Tensor, D: torch.Tensor, g: torch.Tensor, B: int, Lq: int,
                 out: Optional[dict] = None, workspace: Optional[torch.Tensor] = None):
    """The tree scan's backward (vasr_ssm_tree_bwd_f32; modes 0 / 2, scan_mode="parallel"): the
    gradient of ssm_scan / ssm_scan_ungated at a tree mode from the inputs alone, no checkpoints.
    Operands, the returned dict, out / workspace and the guarantees are ssm_scan_bwd's; the workspace
    is vasr_ssm_tree_bwd_workspace_floats(B, L, Di, N) floats (7 per 16-step chunk, channel and state)."""
    return _ssm_bwd("ssm_tree_bwd", x, z, dt, bc, A, A2, D, g, None, B, Lq, out, workspace)


def ssm_block_tail_gated(yd: torch.Tensor, u: torch.Tensor, wz: torch.Tensor, mode: int, x: torch.Tensor,
                         wo: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, ln_eps: float, w1: torch.Tensor,
                         b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The z-in-tail block's tail (vasr_ssm_block_tail_gated_f32, or _bf16 for bf16 weights): z =
    u W_z^T (the projection GEMM's exact product: split planes for fp32 weights, the bf16 tile
    engine's one product for bf16), g = yd * silu(z) (scan mode `mode`'s gate), then
    ssm_block_tail on g -- for yd (M, 384) the ungated scan output, u (M, 192) the projection
    input, wz (384, 192) = in_proj rows Di..2Di-1 (a persistent tensor: its planes are cached by
    identity)."""
    bf16 = wo.dtype == torch.bfloat16
    if bf16:
        if not (wz.dtype == w1.dtype == w2.dtype == torch.bfloat16):
            raise TypeError("ssm_block_tail_gated: mixed weight dtypes")
        ln_w, ln_b, b1, b2 = f32(ln_w), f32(ln_b), f32(b1), f32(b2)
    for n, t in (("yd", yd), ("u", u), ("x", x), ("ln_w", ln_w), ("ln_b", ln_b), ("b1", b1), ("b2", b2)) + (
            () if bf16 else (("wz", wz), ("wo", wo), ("w1", w1), ("w2", w2))):
        _cuda_f32(f"ssm_block_tail_gated.{n}", t)
    M, E, ldy = _rows("ssm_block_tail_gated.yd", yd)
    Mu, D, ldu = _rows("ssm_block_tail_gated.u", u)
    Mx, Dx, ldx = _rows("ssm_block_tail_gated.x", x)
    if Mu != M or Mx != M or Dx != D or tuple(wz.shape) != (E, D) or tuple(wo.shape) != (D, E):
        raise ValueError("ssm_block_tail_gated: inconsistent shapes")
    if out is None:
        out = torch.empty((M, D), device=yd.device, dtype=torch.float32)
    _, _, ldo = _rows("ssm_block_tail_gated.out", out)
    zprep, prep = (pack_bf16, pack_weights16) if bf16 else (split_weights, split_weights16)
    fn = "vasr_ssm_block_tail_gated_bf16" if bf16 else "vasr_ssm_block_tail_gated_f32"
    ev = _t0("ssm_tail")
    check(getattr(L.lib(), fn)(yd.data_ptr(), ldy, u.data_ptr(), ldu, zprep(wz).data_ptr(), int(mode), x.data_ptr(),
                               ldx, prep(wo).data_ptr(), ln_w.contiguous().data_ptr(), ln_b.contiguous().data_ptr(),
                               float(ln_eps), prep(w1).data_ptr(), b1.contiguous().data_ptr(), prep(w2).data_ptr(),
                               b2.contiguous().data_ptr(), out.data_ptr(), ldo, M, D, E, stream_of(yd)), fn)
    _t1("ssm_tail", ev, dict(M=M, D=D, E=E, gated=True))
    return out


def reflect_pad(audio: torch.Tensor, pad: int, ld_out: int) -> torch.Tensor:
    _cuda_f32("reflect_pad.audio", audio)
    audio = audio.contiguous()
    B, S = audio.shape
    xp = torch.empty((B, ld_out), device=audio.device, dtype=torch.float32)
    check(L.lib().vasr_reflect_pad_f32(audio.data_ptr(), S, xp.data_ptr(), ld_out, B, S, pad, stream_of(audio)),
          "vasr_reflect_pad_f32")
    return xp


def _lens(name: str, t: Optional[torch.Tensor], B: int, device) -> Optional[torch.Tensor]:
    """Per-utterance size array of a zero-padded batch: a contiguous int32 (B,) tensor on the device."""
    if t is None:
        return None
    if t.device != device or t.dtype != torch.int32 or tuple(t.shape) != (B,) or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous int32 ({B},) tensor on {device}")
    return t


def stft_power_400(audio: torch.Tensor, window: torch.Tensor, samples: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, S) audio -> (B, S // 160 + 1, 201) |STFT|^2 (n_fft 400, hop 160, reflect pad, Hann).
    samples: per-utterance lengths (int32 (B,), each in (200, S]) of a zero-padded batch."""
    _cuda_f32("stft_power_400.audio", audio)
    _cuda_f32("stft_power_400.window", window)
    audio = audio.contiguous()
    B, S = audio.shape
    if window.numel() != 400:
        raise ValueError(f"stft_power_400: window must have 400 entries, got {window.numel()}")
    F = S // 160 + 1
    power = torch.empty((B, F, 201), device=audio.device, dtype=torch.float32)
    samples = _lens("stft_power_400.samples", samples, B, audio.device)
    if samples is None:
        check(L.lib().vasr_stft_power_400_f32(audio.data_ptr(), S, B, S, window.contiguous().data_ptr(),
                                              power.data_ptr(), 201, F * 201, stream_of(audio)),
              "vasr_stft_power_400_f32")
    else:
        check(L.lib().vasr_stft_power_400_var_f32(audio.data_ptr(), S, B, S, samples.data_ptr(),
                                                  window.contiguous().data_ptr(), power.data_ptr(), 201, F * 201,
                                                  stream_of(audio)), "vasr_stft_power_400_var_f32")
    return power


def resample_mix(x: torch.Tensor, taps: Optional[torch.Tensor], orig: int, nw: int, width: int,
                 samples: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Channel downmix + sample-rate conversion in one launch (vasr_resample_mix_f32).

    x (B, C, S_in) or (B, S_in) float32 with unit stride along samples (clip and channel strides
    are passed on, so views are read in place) -> (B, S_out), S_out = ceil(nw * S_in / orig).
    taps: the (nw, 2 * width + orig) table of vasr_resample_taps_f32 on x's device; (orig, nw,
    width) from vasr_resample_plan.  samples: per-clip sample counts (int32 (B,), each in
    [1, S_in]) of a zero-padded batch; row b then holds the clip's own outputs followed by zeros."""
    _cuda_f32("resample_mix.x", x)
    if x.dim() == 2:
        x = x.unsqueeze(1)
    if x.dim() != 3 or x.shape[0] < 1 or x.shape[2] < 1:
        raise ValueError(f"resample_mix: expected (B, C, S) or (B, S) with B, S >= 1, got {tuple(x.shape)}")
    B, C, S_in = x.shape
    # the stride of a dimension of size 1 is arbitrary (unsqueeze) and never used: pass S_in for it
    ld_clip = x.stride(0) if B > 1 else S_in
    ld_chan = x.stride(1) if C > 1 else S_in
    if (S_in > 1 and x.stride(2) != 1) or ld_clip < S_in or ld_chan < S_in:
        x = x.contiguous()
        ld_clip, ld_chan = C * S_in, S_in
    if orig != nw:
        _cuda_f32("resample_mix.taps", taps)
        if taps.device != x.device or not taps.is_contiguous() or taps.numel() != nw * (2 * width + orig):
            raise ValueError(f"resample_mix: taps must be a contiguous ({nw}, {2 * width + orig}) table on {x.device}")
    samples = _lens("resample_mix.samples", samples, B, x.device)
    S_out = (nw * S_in + orig - 1) // orig
    y = torch.empty((B, S_out), device=x.device, dtype=torch.float32)
    check(L.lib().vasr_resample_mix_f32(x.data_ptr(), ld_clip, ld_chan, B, C, S_in, ptr(samples), ptr(taps),
                                        orig, nw, width, y.data_ptr(), S_out, S_out, stream_of(x)),
          "vasr_resample_mix_f32")
    return y


SEGMENT_BLOCK = 320  # samples per block of the segmenter: one token row, two mel hops (vasr_segment_block)


def _recordings(name: str, audio: torch.Tensor) -> torch.Tensor:
    """(B, S) float32 HIP recordings with unit stride along samples; the row stride is passed on."""
    if not isinstance(audio, torch.Tensor):
        raise ValueError(f"{name}: expected a tensor")
    if audio.device.type != "cuda":
        raise RuntimeError(f"{name}: tensor is on {audio.device}; velocity_asr (MI355X build) runs on HIP devices only")
    if audio.dtype != torch.float32:
        raise ValueError(f"{name}: expected float32, got {audio.dtype}")
    if audio.dim() != 2 or audio.shape[0] < 1 or audio.shape[1] < 1:
        raise ValueError(f"{name}: expected (B, S) with B, S >= 1, got {tuple(audio.shape)}")
    if audio.shape[0] > 65535:
        raise ValueError(f"{name}: at most 65535 recordings per launch, got {audio.shape[0]}")
    if audio.shape[1] >= 2 ** 31:
        raise ValueError(f"{name}: at most 2^31 - 1 samples per recording, got {audio.shape[1]}")
    if (audio.shape[1] > 1 and audio.stride(1) != 1) or (audio.shape[0] > 1 and audio.stride(0) < audio.shape[1]):
        audio = audio.contiguous()
    return audio


def block_energy(audio: torch.Tensor, samples: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, S) float32 recordings -> E (B, S // 320) float64 (vasr_block_energy_f64): per block of 320
    samples the ascending float64 chain of its squared samples, 0 for blocks that are not wholly
    inside samples[b] (int32 (B,), all S when None).  Nothing at or past samples[b] is read."""
    audio = _recordings("block_energy.audio", audio)
    B, S = audio.shape
    samples = _lens("block_energy.samples", samples, B, audio.device)
    nb = S // SEGMENT_BLOCK
    E = torch.empty((B, nb), device=audio.device, dtype=torch.float64)
    if nb == 0:  # no full block
        return E
    check(L.lib().vasr_block_energy_f64(audio.data_ptr(), audio.stride(0) if B > 1 else S, B, S, ptr(samples),
                                        E.data_ptr(), nb, stream_of(audio)), "vasr_block_energy_f64")
    return E


def segment_plan(energy: torch.Tensor, S: int, max_samples: int, min_samples: int, window_blocks: int = 10,
                 samples: Optional[torch.Tensor] = None, max_cuts: Optional[int] = None):
    """The greedy cut plan on block energies (vasr_segment_plan): energy (B, S // 320) float64 from
    block_energy of (B, S) recordings -> (cuts (B, max_cuts) int64 in samples, n_cuts (B,) int32);
    only the first n_cuts[b] entries of a row are written.  max_cuts: columns of the table, by
    default what vasr_segment_max_cuts gives for S (a narrower table is refused)."""
    if not isinstance(energy, torch.Tensor) or energy.device.type != "cuda":
        raise RuntimeError("segment_plan.energy: expected a HIP tensor")
    if energy.dtype != torch.float64:
        raise ValueError(f"segment_plan.energy: expected float64, got {energy.dtype}")
    S, max_samples, min_samples, window_blocks = int(S), int(max_samples), int(min_samples), int(window_blocks)
    if energy.dim() != 2 or energy.shape[0] < 1 or S < 1 or S >= 2 ** 31 or energy.shape[1] != S // SEGMENT_BLOCK:
        raise ValueError(f"segment_plan: energy must be (B, {S // SEGMENT_BLOCK}) for {S} samples, got "
                         f"{tuple(energy.shape)}")
    if min_samples < 1 or max_samples < 1:
        raise ValueError(f"segment_plan: bad segment bounds ({min_samples}, {max_samples})")
    energy = energy.contiguous()
    B = energy.shape[0]
    samples = _lens("segment_plan.samples", samples, B, energy.device)
    if max_cuts is None:
        max_cuts = max(1, int(L.lib().vasr_segment_max_cuts(S, min_samples)))
    max_cuts = int(max_cuts)
    if max_cuts < 1:
        raise ValueError(f"segment_plan: max_cuts must be at least 1, got {max_cuts}")
    cuts = torch.zeros((B, max_cuts), device=energy.device, dtype=torch.int64)
    n_cuts = torch.zeros((B,), device=energy.device, dtype=torch.int32)
    rc = L.lib().vasr_segment_plan(energy.data_ptr(), energy.shape[1], B, S, ptr(samples), max_samples, min_samples,
                                   window_blocks, cuts.data_ptr(), max_cuts, max_cuts, n_cuts.data_ptr(),
                                   stream_of(energy))
    if rc == -1:  # a parameter or table-width error, stated by the library
        raise ValueError(L.lib().vasr_last_error().decode(errors="replace"))
    check(rc, "vasr_segment_plan")
    return cuts, n_cuts


def segment_gather(audio: torch.Tensor, table: torch.Tensor, S_seg: int) -> torch.Tensor:
    """(B, S) recordings and a device table (n_seg, 3) int64 of (recording, start, length) rows ->
    the (n_seg, S_seg) zero-padded batch of the segments in one launch (vasr_segment_gather_f32)."""
    audio = _recordings("segment_gather.audio", audio)
    if not isinstance(table, torch.Tensor) or table.device != audio.device or table.dtype != torch.int64 \
            or table.dim() != 2 or table.shape[1] != 3 or table.shape[0] < 1 or not table.is_contiguous():
        raise ValueError(f"segment_gather.table: expected a contiguous int64 (n_seg, 3) tensor on {audio.device}")
    S_seg = int(S_seg)
    if S_seg < 1 or table.shape[0] > 65535:
        raise ValueError(f"segment_gather: {table.shape[0]} segments of up to {S_seg} samples; 1 to 65535 segments of "
                         "at least one sample")
    B, S = audio.shape
    y = torch.empty((table.shape[0], S_seg), device=audio.device, dtype=torch.float32)
    check(L.lib().vasr_segment_gather_f32(audio.data_ptr(), audio.stride(0) if B > 1 else S, B, S, table.data_ptr(),
                                          table.shape[0], y.data_ptr(), S_seg, S_seg, stream_of(audio)),
          "vasr_segment_gather_f32")
    return y


EDIT_MAX_ITEMS = 65535  # items per sequence and pairs per launch of vasr_edit_counts_i32


def _id_rows(name: str, t: torch.Tensor):
    """(P, L) int32 HIP id rows with unit stride along items -> (tensor with data, row stride, L).  A
    width of 0 is legal (every sequence empty); the library still wants a pointer."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a tensor")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name}: tensor is on {t.device}; velocity_asr (MI355X build) runs on HIP devices only")
    if t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] < 1:
        raise ValueError(f"{name}: expected int32 (P, L) with P >= 1, got {t.dtype} {tuple(t.shape)}")
    P, n = t.shape
    if n > EDIT_MAX_ITEMS:
        raise ValueError(f"{name}: at most {EDIT_MAX_ITEMS} items per sequence, got {n}")
    if n == 0:
        return torch.empty((P, 1), device=t.device, dtype=torch.int32), 1, 0
    if (n > 1 and t.stride(1) != 1) or (P > 1 and t.stride(0) < n):
        t = t.contiguous()
    return t, (t.stride(0) if P > 1 else n), n


def edit_counts(hyp: torch.Tensor, ref: torch.Tensor, hyp_lengths: torch.Tensor, ref_lengths: torch.Tensor) -> torch.Tensor:
    """Substitution, deletion and insertion counts of P pairs (vasr_edit_counts_i32): hyp (P, Lh) and ref
    (P, Lr) int32 ids, lengths int32 (P,) clamped to [0, L]; rows may be views into wider matrices.
    -> (P, 3) int32 on the device, equal to training.edit_counts_host of each pair.  No synchronisation;
    more than 65535 pairs go in several launches."""
    hyp, ld_h, mh = _id_rows("edit_counts.hyp", hyp)
    ref, ld_r, mr = _id_rows("edit_counts.ref", ref)
    P = hyp.shape[0]
    if ref.shape[0] != P or ref.device != hyp.device:
        raise ValueError(f"edit_counts: hyp has {P} rows on {hyp.device}, ref {ref.shape[0]} on {ref.device}")
    hyp_lengths = _lens("edit_counts.hyp_lengths", hyp_lengths, P, hyp.device)
    ref_lengths = _lens("edit_counts.ref_lengths", ref_lengths, P, hyp.device)
    if hyp_lengths is None or ref_lengths is None:
        raise ValueError("edit_counts: hyp_lengths and ref_lengths are required")
    counts = torch.empty((P, 3), device=hyp.device, dtype=torch.int32)
    lib = L.lib()
    for p0 in range(0, P, EDIT_MAX_ITEMS):
        n = min(EDIT_MAX_ITEMS, P - p0)
        need = int(lib.vasr_edit_workspace_bytes(n, mh, mr))
        if need < 0:
            raise ValueError(f"edit_counts: sizes ({n}, {mh}, {mr}) outside the kernel's limits")
        ws = torch.empty((need // 8,), device=hyp.device, dtype=torch.int64) if need else None
        check(lib.vasr_edit_counts_i32(hyp[p0:].data_ptr(), ld_h, hyp_lengths[p0:].data_ptr(), mh, ref[p0:].data_ptr(),
                                       ld_r, ref_lengths[p0:].data_ptr(), mr, n, counts[p0:].data_ptr(), ptr(ws), need,
                                       stream_of(hyp)), "vasr_edit_counts_i32")
    return counts


# Default budget of edit_alignment's choice table per launch.  A pair's table is 2 * hyp_len * ceil(ref_len / 8)
# bytes (20 MB for 9000 x 9000, 1.07 GB for 65535 x 65535), so 1 GiB holds every pair but the very largest.
EDIT_ALIGN_TABLE_BYTES = 1 << 30
_EDIT_TABLE_ALIGN = 16  # the pairs' offsets inside the table


def _host_lens(name: str, t, P: int, width: int, device):
    """Lengths as a host sequence or a device tensor -> (contiguous int32 device tensor, clamped host list)."""
    if isinstance(t, torch.Tensor):
        dev = _lens(name, t, P, device)
        host = dev.cpu().tolist()
    else:
        host = [int(x) for x in t]
        if len(host) != P:
            raise ValueError(f"{name}: expected {P} lengths, got {len(host)}")
        dev = torch.tensor(host, dtype=torch.int32).to(device)
    return dev, [min(max(x, 0), width) for x in host]


def edit_alignment(hyp: torch.Tensor, ref: torch.Tensor, hyp_lengths, ref_lengths,
                   table_bytes: int = EDIT_ALIGN_TABLE_BYTES):
    """Edit paths of P pairs (vasr_edit_align_i32): hyp, ref as in edit_counts; the lengths are sequences of
    ints when the host knows them, or int32 (P,) device tensors, which are then read back once (the caller is
    about to download the paths anyway).  -> (counts (P, 3) int32, ops (P, max(1, Lh + Lr)) uint8, ops_len (P,)
    int32), all on the device: ops[p, :ops_len[p]] are the codes of training.edit_alignment_host (0 hit,
    1 substitution, 2 deletion, 3 insertion) and counts equals edit_counts'; ops past ops_len is unspecified.
    The choice table is sized by the sum of the pairs' own extents (vasr_edit_align_table_bytes) and the pairs
    are split into as many launches as fit `table_bytes` each (default EDIT_ALIGN_TABLE_BYTES, 1 GiB).  A single
    pair whose own table exceeds table_bytes is not aligned: its ops_len is -1 (its counts are still right)
    and the caller handles it."""
    hyp, ld_h, mh = _id_rows("edit_alignment.hyp", hyp)
    ref, ld_r, mr = _id_rows("edit_alignment.ref", ref)
    P = hyp.shape[0]
    if ref.shape[0] != P or ref.device != hyp.device:
        raise ValueError(f"edit_alignment: hyp has {P} rows on {hyp.device}, ref {ref.shape[0]} on {ref.device}")
    if hyp_lengths is None or ref_lengths is None:
        raise ValueError("edit_alignment: hyp_lengths and ref_lengths are required")
    table_bytes = int(table_bytes)
    if table_bytes < 0:
        raise ValueError(f"edit_alignment: table_bytes must not be negative, got {table_bytes}")
    hyp_lengths, hl = _host_lens("edit_alignment.hyp_lengths", hyp_lengths, P, mh, hyp.device)
    ref_lengths, rl = _host_lens("edit_alignment.ref_lengths", ref_lengths, P, mr, hyp.device)
    lib = L.lib()
    extent = [int(lib.vasr_edit_align_table_bytes(a, b)) for a, b in zip(hl, rl)]
    # launches: runs [p0, p1) of consecutive pairs whose tables fit the budget together; offset -1 marks a
    # pair that is over the budget alone, which ends a run and is left out
    offsets, runs, p0, used = [], [], 0, 0
    for p, e in enumerate(extent):
        e = -(-e // _EDIT_TABLE_ALIGN) * _EDIT_TABLE_ALIGN
        if e > table_bytes or used + e > table_bytes or p - p0 == EDIT_MAX_ITEMS:
            if p > p0:
                runs.append((p0, p, used))
            p0, used = p, 0
        if e > table_bytes:
            offsets.append(-1)
            p0 = p + 1
            continue
        offsets.append(used)
        used += e
    if P > p0:
        runs.append((p0, P, used))
    dev = hyp.device
    ld_ops = max(1, mh + mr)
    counts = torch.empty((P, 3), device=dev, dtype=torch.int32)
    ops = torch.empty((P, ld_ops), device=dev, dtype=torch.uint8)
    ops_len = torch.full((P,), -1, device=dev, dtype=torch.int32)
    offs = torch.tensor(offsets, dtype=torch.int64).to(dev)
    table = torch.empty((max([u for _, _, u in runs] + [_EDIT_TABLE_ALIGN]),), device=dev, dtype=torch.uint8)
    stream = stream_of(hyp)
    for p0, p1, used in runs:  # launches on one stream share the table: each writes its part before reading it
        n = p1 - p0
        need = int(lib.vasr_edit_workspace_bytes(n, mh, mr))
        if need < 0:
            raise ValueError(f"edit_alignment: sizes ({n}, {mh}, {mr}) outside the kernel's limits")
        ws = torch.empty((need // 8,), device=dev, dtype=torch.int64) if need else None
        check(lib.vasr_edit_align_i32(hyp[p0:].data_ptr(), ld_h, hyp_lengths[p0:].data_ptr(), mh, ref[p0:].data_ptr(), ld_r,
                                      ref_lengths[p0:].data_ptr(), mr, n, counts[p0:].data_ptr(), ops[p0:].data_ptr(), ld_ops,
                                      ops_len[p0:].data_ptr(), offs[p0:].data_ptr(), table.data_ptr(), used, ptr(ws), need,
                                      stream), "vasr_edit_align_i32")
    for p, o in enumerate(offsets):
        if o < 0:  # over the budget alone: counts only
            counts[p:p + 1] = edit_counts(hyp[p:p + 1], ref[p:p + 1], hyp_lengths[p:p + 1], ref_lengths[p:p + 1])
    return counts, ops, ops_len


def mel_log_norm(power: torch.Tensor, ld_power: int, stride_power: int, fb_csr, B: int, F: int, n_mels: int,
                 normalize: bool, frames: Optional[torch.Tensor] = None, frame_pad: int = 0) -> torch.Tensor:
    """frames: per-utterance frame counts (int32 (B,), each <= F); frames past them are 0.
    frame_pad > 0: the mel is written into a (B, F + 2 frame_pad, n_mels) buffer whose outer
    frames the kernel zero-fills, and the (B, F, n_mels) view into it is returned, marked as
    zero-framed (zero_framed()) so the temporal conv reads it without a padding copy."""
    rowptr, col, val = fb_csr
    Fo = F + 2 * frame_pad
    buf = torch.empty((B, Fo, n_mels), device=power.device, dtype=torch.float32)
    ws = torch.empty(int(L.lib().vasr_mel_workspace_floats(B, F, n_mels)), device=power.device, dtype=torch.float32)
    frames = _lens("mel_log_norm.frames", frames, B, power.device)
    if frames is None:
        check(L.lib().vasr_mel_log_norm_f32(power.data_ptr(), ld_power, stride_power, rowptr.data_ptr(),
                                            col.data_ptr(), val.data_ptr(), buf.data_ptr(), Fo * n_mels, frame_pad, B,
                                            F, n_mels, int(normalize), ws.data_ptr(), stream_of(power)),
              "vasr_mel_log_norm_f32")
    else:
        check(L.lib().vasr_mel_log_norm_var_f32(power.data_ptr(), ld_power, stride_power, rowptr.data_ptr(),
                                                col.data_ptr(), val.data_ptr(), buf.data_ptr(), Fo * n_mels, frame_pad,
                                                B, F, n_mels, int(normalize), frames.data_ptr(), ws.data_ptr(),
                                                stream_of(power)), "vasr_mel_log_norm_var_f32")
    if not frame_pad:
        return buf
    out = buf[:, frame_pad:frame_pad + F]
    out._vasr_zero_framed = (buf, frame_pad)
    return out


def zero_framed(x: torch.Tensor, pad: int):
    """The (B, F + 2 q, C) buffer of a (B, F, C) view written by mel_log_norm(..., frame_pad=q)
    with q >= pad zero frames on each side, sliced to `pad` zero frames, or None."""
    ent = getattr(x, "_vasr_zero_framed", None)
    if ent is None:
        return None
    buf, q = ent
    if q < pad or buf.data_ptr() + q * buf.shape[2] * 4 != x.data_ptr() or x.shape[1] + 2 * q != buf.shape[1]:
        return None
    return buf[:, q - pad:q + x.shape[1] + pad]


def pad_frames(x: torch.Tensor, out_frames: int, off: int) -> torch.Tensor:
    _cuda_f32("pad_frames.x", x)
    x = x.contiguous()
    B, F, C = x.shape
    out = torch.empty((B, out_frames, C), device=x.device, dtype=torch.float32)
    check(L.lib().vasr_pad_frames_f32(x.data_ptr(), out.data_ptr(), out_frames, off, B, F, C, stream_of(x)),
          "vasr_pad_frames_f32")
    return out


def adaptive_pool(x: torch.Tensor, K: int, lens: Optional[torch.Tensor] = None,
                  ks: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, L, C) -> (B, K, C) adaptive average pooling over time; with lens / ks (int32 (B,))
    utterance b pools its first lens[b] rows into ks[b] bins, later bins 0."""
    _cuda_f32("adaptive_pool.x", x)
    x = x.contiguous()
    B, Lq, C = x.shape
    out = torch.empty((B, K, C), device=x.device, dtype=torch.float32)
    if (lens is None) != (ks is None):
        raise ValueError("adaptive_pool: lens and ks go together")
    if lens is None:
        check(L.lib().vasr_adaptive_pool_f32(x.data_ptr(), out.data_ptr(), B, Lq, C, K, stream_of(x)),
              "vasr_adaptive_pool_f32")
    else:
        lens = _lens("adaptive_pool.lens", lens, B, x.device)
        ks = _lens("adaptive_pool.ks", ks, B, x.device)
        check(L.lib().vasr_adaptive_pool_var_f32(x.data_ptr(), out.data_ptr(), B, Lq, C, K, lens.data_ptr(),
                                                 ks.data_ptr(), stream_of(x)), "vasr_adaptive_pool_var_f32")
    return out


def ln_adaptive_pool(x: torch.Tensor, w, b, eps: float, K: int, lens: Optional[torch.Tensor] = None,
                     ks: Optional[torch.Tensor] = None) -> torch.Tensor:
    """adaptive_pool(layer_norm(x, w, b, eps), K, lens, ks) in one launch, bitwise the two
    (vasr_ln_adaptive_pool_f32)."""
    _cuda_f32("ln_adaptive_pool.x", x)
    w, b = f32(w), f32(b)
    x = x.contiguous()
    B, Lq, C = x.shape
    out = torch.empty((B, K, C), device=x.device, dtype=torch.float32)
    if (lens is None) != (ks is None):
        raise ValueError("ln_adaptive_pool: lens and ks go together")
    if lens is not None:
        lens = _lens("ln_adaptive_pool.lens", lens, B, x.device)
        ks = _lens("ln_adaptive_pool.ks", ks, B, x.device)
    check(L.lib().vasr_ln_adaptive_pool_f32(x.data_ptr(), w.data_ptr(), b.data_ptr(), float(eps), out.data_ptr(), B,
                                            Lq, C, K, None if lens is None else lens.data_ptr(),
                                            None if ks is None else ks.data_ptr(), stream_of(x)),
          "vasr_ln_adaptive_pool_f32")
    return out


def pooled_attention(q: torch.Tensor, kv: torch.Tensor, B: int, Lq: int, Kp: int, heads: int,
                     kps: Optional[torch.Tensor] = None) -> torch.Tensor:
    """kps: per-utterance key counts (int32 (B,), each in [1, Kp])."""
    _cuda_f32("pooled_attention.q", q)
    _cuda_f32("pooled_attention.kv", kv)
    M, A, ld_q = _rows("pooled_attention.q", q)
    kv = kv.contiguous()
    if kv.shape != (B * Kp, 2 * A) or M != B * Lq or A % heads:
        raise ValueError("pooled_attention: inconsistent shapes")
    out = torch.empty((M, A), device=q.device, dtype=torch.float32)
    kps = _lens("pooled_attention.kps", kps, B, q.device)
    if kps is None:
        check(L.lib().vasr_pooled_attention_f32(q.data_ptr(), ld_q, kv.data_ptr(), out.data_ptr(), B, Lq, Kp, heads,
                                                A // heads, stream_of(q)), "vasr_pooled_attention_f32")
    else:
        check(L.lib().vasr_pooled_attention_var_f32(q.data_ptr(), ld_q, kv.data_ptr(), out.data_ptr(), B, Lq, Kp,
                                                    heads, A // heads, kps.data_ptr(), stream_of(q)),
              "vasr_pooled_attention_var_f32")
    return out


ATTN_BWD_TILE = 64  # tokens per workgroup of the attention's backward (csrc/attn_bwd.hip)


def pooled_attention_bwd(q: torch.Tensor, kv: torch.Tensor, dout: torch.Tensor, B: int, Lq: int, Kp: int, heads: int,
                         kps: Optional[torch.Tensor] = None,
                         workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """pooled_attention's backward (vasr_pooled_attention_bwd_f32): dout (B*L, A) = d loss / d out ->
    (dq (B*L, A), dkv (B*Kp, 2A) [dK | dV]), rows past kps[b] of dkv 0.  q, kv, kps as the forward's;
    the softmax is recomputed.  No atomics: run-to-run bitwise, and an utterance's rows do not depend
    on the rest of the batch.  workspace: vasr_pooled_attention_bwd_workspace_floats floats (the
    per-tile [dK | dV] partials; none for L <= 64)."""
    _cuda_f32("pooled_attention_bwd.q", q)
    _cuda_f32("pooled_attention_bwd.kv", kv)
    _cuda_f32("pooled_attention_bwd.dout", dout)
    M, A, ld_q = _rows("pooled_attention_bwd.q", q)
    kv, dout = kv.contiguous(), dout.contiguous()
    if kv.shape != (B * Kp, 2 * A) or M != B * Lq or A % heads or dout.shape != (M, A):
        raise ValueError("pooled_attention_bwd: inconsistent shapes")
    kps = _lens("pooled_attention_bwd.kps", kps, B, q.device)
    dq = torch.empty((M, A), device=q.device, dtype=torch.float32)
    dkv = torch.empty((B * Kp, 2 * A), device=q.device, dtype=torch.float32)
    if workspace is None:
        nws = int(L.lib().vasr_pooled_attention_bwd_workspace_floats(B, Lq, Kp, heads, A // heads))
        workspace = torch.empty(nws, device=q.device, dtype=torch.float32)
    _cuda_f32("pooled_attention_bwd.workspace", workspace)
    ev = _t0("pooled_attention_bwd")
    check(L.lib().vasr_pooled_attention_bwd_f32(q.data_ptr(), ld_q, kv.data_ptr(), dout.data_ptr(), dq.data_ptr(),
                                                dkv.data_ptr(), workspace.data_ptr(), workspace.numel(), B, Lq, Kp,
                                                heads, A // heads, ptr(kps), stream_of(q)),
          "vasr_pooled_attention_bwd_f32")
    _t1("pooled_attention_bwd", ev, dict(B=B, L=Lq, Kp=Kp, heads=heads, hd=A // heads))
    return dq, dkv


def adaptive_pool_bwd(g: torch.Tensor, Lq: int, lens: Optional[torch.Tensor] = None,
                      ks: Optional[torch.Tensor] = None) -> torch.Tensor:
    """adaptive_pool's backward (vasr_adaptive_pool_bwd_f32): g (B, K, C) = d loss / d out -> dx
    (B, L, C); with lens / ks rows past lens[b] are 0 and bins past ks[b] of g are not read."""
    _cuda_f32("adaptive_pool_bwd.g", g)
    g = g.contiguous()
    B, K, C = g.shape
    if (lens is None) != (ks is None):
        raise ValueError("adaptive_pool_bwd: lens and ks go together")
    lens = _lens("adaptive_pool_bwd.lens", lens, B, g.device)
    ks = _lens("adaptive_pool_bwd.ks", ks, B, g.device)
    dx = torch.empty((B, Lq, C), device=g.device, dtype=torch.float32)
    check(L.lib().vasr_adaptive_pool_bwd_f32(g.data_ptr(), dx.data_ptr(), B, Lq, C, K, ptr(lens), ptr(ks),
                                             stream_of(g)), "vasr_adaptive_pool_bwd_f32")
    return dx


def probe_clock(device, blocks: int = 2048, iters: int = 20000) -> dict:
    """Machine state for a benchmark record (vasr_probe_clock): the shader clock over a fixed VALU
    chain (median over workgroups, GHz) and the XCD dispatch order.  The kernels' XCD-aware block
    maps need workgroups i and i + 8 on one XCD: round-robin dispatch, from whichever XCD the
    dispatcher's pointer starts at (the previous launch's grid moves it: profiles/r05d/)."""
    out = torch.zeros(3 * blocks, device=device, dtype=torch.int64)
    check(L.lib().vasr_probe_clock(out.data_ptr(), blocks, iters, torch.cuda.current_stream(device).cuda_stream),
          "vasr_probe_clock")
    o = out.view(blocks, 3).cpu()
    ghz = (o[:, 1].double() / o[:, 2].clamp(min=1).double() * 0.1).median().item()
    xcd = o[:, 0]
    ids = torch.arange(blocks)
    fr = [(xcd == (ids + k) % 8).double().mean().item() for k in range(8)]
    k = max(range(8), key=lambda j: fr[j])
    return dict(clock_ghz=round(ghz, 3), xcd_round_robin_frac=round(fr[k], 4), xcd_start=k,
                xcds_seen=int(xcd.unique().numel()))


def argmax(logits: torch.Tensor) -> torch.Tensor:
    """int32 argmax over the last dim (ties -> first index)."""
    _cuda_f32("argmax.logits", logits)
    V = logits.shape[-1]
    x2 = logits.reshape(-1, V)
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    rows = x2.shape[0]
    ld = x2.stride(0) if rows > 1 else V
    out = torch.empty(rows, device=logits.device, dtype=torch.int32)
    check(L.lib().vasr_argmax_f32(x2.data_ptr(), ld, rows, V, out.data_ptr(), stream_of(logits)), "vasr_argmax_f32")
    return out.view(logits.shape[:-1])


def _collapse_outputs(who: str, B: int, Lq: int, device, out, timestamps: bool, frames):
    """Output buffers (tokens, lengths, start, end) of a collapse and its checked frames."""
    if out is None:
        toks = torch.empty((B, Lq), device=device, dtype=torch.int32)
        lens = torch.empty((B,), device=device, dtype=torch.int32)
    else:
        toks, lens = out
        for n, t, shape in (("tokens", toks, (B, Lq)), ("lengths", lens, (B,))):
            if (t.device != device or t.dtype != torch.int32 or tuple(t.shape) != shape
                    or not t.is_contiguous()):
                raise ValueError(f"{who}: out {n} must be a contiguous int32 {shape} tensor on {device}")
    st = en = None
    if timestamps:
        st = torch.empty((B, Lq), device=device, dtype=torch.int32)
        en = torch.empty((B, Lq), device=device, dtype=torch.int32)
    return toks, lens, st, en, _lens(f"{who}.frames", frames, B, device)


def ctc_collapse(pred: torch.Tensor, blank: int = 0, collapse: bool = True, timestamps: bool = False,
                 out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, frames: Optional[torch.Tensor] = None):
    """Device-side greedy CTC collapse of (B, L) int32 predictions.  out = (tokens (B, L),
    lengths (B,)): contiguous int32 buffers to write into (e.g. row slices of a graph's
    static output).  frames: per-utterance row counts (int32 (B,)) of a padded batch."""
    if pred.device.type != "cuda" or pred.dtype != torch.int32:
        raise TypeError("ctc_collapse: expected a cuda int32 tensor")
    pred = pred.contiguous()
    B, Lq = pred.shape
    toks, lens, st, en, frames = _collapse_outputs("ctc_collapse", B, Lq, pred.device, out, timestamps, frames)
    if frames is None:
        check(L.lib().vasr_ctc_collapse(pred.data_ptr(), B, Lq, int(blank), int(collapse), toks.data_ptr(),
                                        lens.data_ptr(), ptr(st), ptr(en), stream_of(pred)), "vasr_ctc_collapse")
    else:
        check(L.lib().vasr_ctc_collapse_var(pred.data_ptr(), B, Lq, frames.data_ptr(), int(blank), int(collapse),
                                            toks.data_ptr(), lens.data_ptr(), ptr(st), ptr(en), stream_of(pred)),
              "vasr_ctc_collapse_var")
    return toks, lens, st, en


def fakequant(x: torch.Tensor, scale: torch.Tensor, zero_point: torch.Tensor, qmin: float, qmax: float,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """FakeQuantize (eval, calibrated) of x viewed as (dim0, rest): scale / zero_point hold
    dim0 entries (per-channel, channel_dim 0) or one (per-tensor)."""
    _cuda_f32("fakequant.x", x)
    _cuda_f32("fakequant.scale", scale)
    _cuda_f32("fakequant.zero_point", zero_point)
    x = x.contiguous()
    rows = x.shape[0] if x.dim() > 0 else 1
    x2 = x.reshape(rows, -1)
    cols = x2.shape[1]
    n = scale.numel()
    if zero_point.numel() != n or n not in (1, rows):
        raise ValueError(f"fakequant: scale/zero_point of {n} entries for a tensor with {rows} channels")
    y = torch.empty_like(x) if out is None else out
    check(L.lib().vasr_fakequant_f32(x2.data_ptr(), cols, y.data_ptr(), cols, rows, cols,
                                     scale.contiguous().data_ptr(), zero_point.contiguous().data_ptr(),
                                     int(n == rows and n > 1), float(qmin), float(qmax), stream_of(x)),
          "vasr_fakequant_f32")
    return y


def minmax(x: torch.Tensor, per_channel: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(min, max) over the whole tensor, or per channel of dim 0 (shape (dim0,))."""
    _cuda_f32("minmax.x", x)
    if x.numel() == 0:
        raise RuntimeError("minmax: empty tensor")
    x = x.contiguous()
    if per_channel and x.dim() >= 1:
        x2 = x.reshape(x.shape[0], -1)
    else:
        x2 = x.reshape(-1, x.shape[-1] if x.dim() >= 1 else 1)
    rows, cols, ld = _rows("minmax.x", x2)
    lo = torch.empty(rows, device=x.device, dtype=torch.float32)
    hi = torch.empty(rows, device=x.device, dtype=torch.float32)
    check(L.lib().vasr_minmax_f32(x2.data_ptr(), ld, rows, cols, lo.data_ptr(), hi.data_ptr(), stream_of(x)),
          "vasr_minmax_f32")
    if per_channel or rows == 1:
        return lo, hi
    lo1 = torch.empty(1, device=x.device, dtype=torch.float32)
    hi1 = torch.empty(1, device=x.device, dtype=torch.float32)
    lib = L.lib()
    check(lib.vasr_minmax_f32(lo.data_ptr(), rows, 1, rows, lo1.data_ptr(), hi1.data_ptr(), stream_of(x)),
          "vasr_minmax_f32")
    scratch = torch.empty(1, device=x.device, dtype=torch.float32)
    check(lib.vasr_minmax_f32(hi.data_ptr(), rows, 1, rows, scratch.data_ptr(), hi1.data_ptr(), stream_of(x)),
          "vasr_minmax_f32")
    return lo1, hi1


def ctc_beam_search(logits: torch.Tensor, beam_width: int, blank: int = 0, *, frames=None, lm_table=None,
                    lm_weight: float = 0.0):
    """Device prefix beam search over (B, L, V) logits -> (tokens (B, W, L) int32, lengths (B, W),
    scores (B, W) float64, beams per utterance (B,)), all on the device.

    frames: per-utterance row counts of a padded batch (rows at or past a count are never read; a
    device tensor is used without a host synchronisation and clamped to 0..L in the kernel, a host
    sequence must lie in 0..L).  lm_table: (V + 1, V) float32 bigram table (decode.BigramLM), in
    effect when lm_weight > 0.  With neither, the search is vasr_ctc_beam_search."""
    _cuda_f32("ctc_beam_search.logits", logits)
    if logits.dim() != 3:
        raise ValueError("ctc_beam_search: logits must be (B, L, V)")
    x = logits if logits.stride(-1) == 1 else logits.contiguous()
    B, Lq, V = x.shape
    W = int(beam_width)
    dev = x.device
    tab = None
    fr = _beam_frames("ctc_beam_search", frames, B, Lq, dev)
    if lm_table is not None:
        _cuda_f32("ctc_beam_search.lm_table", lm_table)
        if tuple(lm_table.shape) != (V + 1, V):
            raise ValueError(f"ctc_beam_search: lm_table must be ({V + 1}, {V}), got {tuple(lm_table.shape)}")
        tab = lm_table if lm_table.stride(-1) == 1 else lm_table.contiguous()
    trie, toks, lens, scores, nbeams = _beam_buffers(B, Lq, W, dev)
    if fr is None and tab is None:
        check(L.lib().vasr_ctc_beam_search(x.data_ptr(), x.stride(1), x.stride(0), B, Lq, V, W, int(blank),
                                           trie.data_ptr(), toks.data_ptr(), lens.data_ptr(), scores.data_ptr(),
                                           nbeams.data_ptr(), stream_of(x)), "vasr_ctc_beam_search")
    else:
        check(L.lib().vasr_ctc_beam_search_lm(x.data_ptr(), x.stride(1), x.stride(0), B, Lq, V, W, int(blank), L.ptr(fr),
                                              L.ptr(tab), 0 if tab is None else tab.stride(0), float(lm_weight),
                                              trie.data_ptr(), toks.data_ptr(), lens.data_ptr(), scores.data_ptr(),
                                              nbeams.data_ptr(), stream_of(x)), "vasr_ctc_beam_search_lm")
    return toks, lens, scores, nbeams


BEAM_SHORTLIST_MAX = 64  # tokens per frame of a shortlist (csrc/beam_shortlist.hip)
BEAM_DENSE_MAX_VOCAB = 16384  # vasr_ctc_beam_search[_lm]: the row's log-probabilities live in LDS


def _beam_buffers(B: int, Lq: int, W: int, dev):
    """The trie workspace of a beam search entry and its four outputs (tokens, lengths, scores, beams
    per utterance), zeroed."""
    trie = torch.empty(max(B, 1) * int(L.lib().vasr_ctc_beam_workspace_elems(Lq, W)), device=dev, dtype=torch.int32)
    toks = torch.zeros((B, W, max(Lq, 1)), device=dev, dtype=torch.int32)
    lens = torch.zeros((B, W), device=dev, dtype=torch.int32)
    scores = torch.zeros((B, W), device=dev, dtype=torch.float64)
    nbeams = torch.zeros((B,), device=dev, dtype=torch.int32)
    return trie, toks, lens, scores, nbeams


def _beam_frames(who: str, frames, B: int, Lq: int, device) -> Optional[torch.Tensor]:
    """ctc_beam_search's frames rule: a host sequence must lie in 0..L, a device tensor is taken as
    it is (the kernels clamp it)."""
    if frames is None:
        return None
    if not (isinstance(frames, torch.Tensor) and frames.device.type == "cuda"):
        host = torch.as_tensor(frames)
        if host.numel() and not host.dtype.is_floating_point and (int(host.min()) < 0 or int(host.max()) > Lq):
            raise ValueError(f"{who}.frames: counts must lie in 0..{Lq}, got {host.tolist()}")
    return _ctc_lengths(f"{who}.frames", frames, B, device, Lq)


def ctc_beam_shortlist(logits: torch.Tensor, K: int, blank: int = 0, frames=None, out=None):
    """Per-frame shortlist of (B, L, V) logits (vasr_ctc_beam_shortlist_f32) ->
    (tokens (B, L, K) int32, log-probabilities (B, L, K), blank log-probabilities (B, L)): each
    frame's K non-blank tokens of largest log-probability, ordered by (log-probability descending,
    token ascending); the log-probabilities are bitwise those ctc_beam_search forms.  K is 1..64 and
    is clamped to V - 1.  frames as ctc_beam_search; rows past a count are not read and hold token
    -1 and -inf.  out: the three tensors to write into (an utterance slice of a batch's arrays).
    K = 0 (complete mode) returns the whole (B, L, V) log-probability rows instead, rows past a
    count unwritten."""
    _cuda_f32("ctc_beam_shortlist.logits", logits)
    if logits.dim() != 3:
        raise ValueError("ctc_beam_shortlist: logits must be (B, L, V)")
    x = logits if logits.stride(-1) == 1 else logits.contiguous()
    B, Lq, V = x.shape
    K = int(K)
    if not 0 <= K <= BEAM_SHORTLIST_MAX:
        raise ValueError(f"ctc_beam_shortlist: K must be 1..{BEAM_SHORTLIST_MAX} (or 0: complete rows), got {K}")
    if K and V < 2:
        raise ValueError("ctc_beam_shortlist: a shortlist needs a non-blank token (V >= 2)")
    dev = x.device
    fr = _beam_frames("ctc_beam_shortlist", frames, B, Lq, dev)
    if K == 0:
        full = torch.empty((B, Lq, V), device=dev, dtype=torch.float32)
        check(L.lib().vasr_ctc_beam_shortlist_f32(x.data_ptr(), x.stride(1), x.stride(0), B, Lq, V, 0, int(blank), ptr(fr),
                                                  None, full.data_ptr(), None, stream_of(x)), "vasr_ctc_beam_shortlist_f32")
        return full
    K = min(K, V - 1)
    if out is None:
        out = (torch.empty((B, Lq, K), device=dev, dtype=torch.int32),
               torch.empty((B, Lq, K), device=dev, dtype=torch.float32),
               torch.empty((B, Lq), device=dev, dtype=torch.float32))
    tok, lp, bl = out
    for n, t, dt, shape in (("tokens", tok, torch.int32, (B, Lq, K)), ("log-probabilities", lp, torch.float32, (B, Lq, K)),
                            ("blank log-probabilities", bl, torch.float32, (B, Lq))):
        if t.device != dev or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"ctc_beam_shortlist: out {n} must be a contiguous {dt} {shape} tensor on {dev}")
    check(L.lib().vasr_ctc_beam_shortlist_f32(x.data_ptr(), x.stride(1), x.stride(0), B, Lq, V, K, int(blank), ptr(fr),
                                              tok.data_ptr(), lp.data_ptr(), bl.data_ptr(), stream_of(x)),
          "vasr_ctc_beam_shortlist_f32")
    return tok, lp, bl


def ctc_beam_search_shortlist(tok: Optional[torch.Tensor], lp: torch.Tensor, blank_lp: Optional[torch.Tensor], V: int,
                              beam_width: int, blank: int = 0, frames=None):
    """Prefix beam search over ctc_beam_shortlist's arrays (vasr_ctc_beam_search_shortlist) ->
    (tokens (B, W, L) int32, lengths (B, W), scores (B, W) float64, beams per utterance (B,),
    uncertified frames per utterance (B,)), all on the device.  Where uncertified[b] is 0, utterance
    b's results are bitwise ctc_beam_search's on the logits the shortlist came from; elsewhere they
    are not proved to be, and the caller searches b again.  V: the vocabulary size.  tok = None
    (complete): lp is the (B, L, V) rows of ctc_beam_shortlist(K=0) and the search is the exact one,
    for any V."""
    _cuda_f32("ctc_beam_search_shortlist.lp", lp)
    if lp.dim() != 3 or not lp.is_contiguous():
        raise ValueError("ctc_beam_search_shortlist: lp must be a contiguous (B, L, K) tensor")
    B, Lq, K = lp.shape
    V, W, dev = int(V), int(beam_width), lp.device
    if tok is None:
        if K != V:
            raise ValueError(f"ctc_beam_search_shortlist: complete rows must be (B, L, {V}), got {tuple(lp.shape)}")
    else:
        _cuda_f32("ctc_beam_search_shortlist.blank_lp", blank_lp)
        if (tok.device != dev or tok.dtype != torch.int32 or tok.shape != lp.shape or not tok.is_contiguous()
                or tuple(blank_lp.shape) != (B, Lq) or not blank_lp.is_contiguous()):
            raise ValueError("ctc_beam_search_shortlist: tok must be int32 (B, L, K) and blank_lp (B, L), contiguous, "
                             "beside lp")
        if not 1 <= K <= min(BEAM_SHORTLIST_MAX, V - 1):
            raise ValueError(f"ctc_beam_search_shortlist: K = {K} outside 1..{min(BEAM_SHORTLIST_MAX, V - 1)} for V = {V}")
    fr = _beam_frames("ctc_beam_search_shortlist", frames, B, Lq, dev)
    trie, toks, lens, scores, nbeams = _beam_buffers(B, Lq, W, dev)
    unc = torch.zeros((B,), device=dev, dtype=torch.int32)
    check(L.lib().vasr_ctc_beam_search_shortlist(ptr(tok), lp.data_ptr(), ptr(blank_lp), B, Lq, 0 if tok is None else K, V,
                                                 W, int(blank), ptr(fr), trie.data_ptr(), toks.data_ptr(), lens.data_ptr(),
                                                 scores.data_ptr(), nbeams.data_ptr(), unc.data_ptr(), stream_of(lp)),
          "vasr_ctc_beam_search_shortlist")
    return toks, lens, scores, nbeams, unc


def _ctc_lengths(name: str, t, B: int, device, default: int) -> torch.Tensor:
    """Per-utterance lengths as a contiguous int32 (B,) device tensor.  A device tensor is used
    (cast if needed) without any host synchronisation; a host tensor, a sequence or None (all
    `default`) is copied up."""
    if t is None:
        return torch.full((B,), int(default), device=device, dtype=torch.int32)
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    if t.dtype.is_floating_point or t.dtype == torch.bool or tuple(t.shape) != (B,):
        raise ValueError(f"{name}: expected {B} integer lengths, got {t.dtype} {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.int32).contiguous()


def _ctc_targets(who: str, targets: torch.Tensor, B: int, device) -> torch.Tensor:
    if not isinstance(targets, torch.Tensor) or targets.dim() != 2 or targets.shape[0] != B:
        raise ValueError(f"{who}: targets must be a (B, Smax) tensor")
    if targets.dtype.is_floating_point or targets.dtype == torch.bool:
        raise TypeError(f"{who}: targets must be integer token ids, got {targets.dtype}")
    return targets.to(device=device, dtype=torch.int32).contiguous()


def ctc_emissions(logits: torch.Tensor, targets: torch.Tensor, frames=None, tlen=None, blank: int = 0):
    """(B, L, V) logits + (B, Smax) targets -> (emis (B, L, Smax + 1), targets, frames, tlen): the
    log-softmax values of the blank and of each target token per frame, and the int32 device
    forms of the other arguments as ctc_loss / ctc_align take them.  One pass over the logits; no
    (B, L, V) log-softmax tensor.  Entries of frames >= frames[b] and slots > tlen[b] are
    unspecified.  frames / tlen: device or host lengths, None = L / Smax."""
    _cuda_f32("ctc_emissions.logits", logits)
    if logits.dim() != 3:
        raise ValueError("ctc_emissions: logits must be (B, L, V)")
    x = logits if logits.stride(-1) == 1 else logits.contiguous()
    B, Lq, V = x.shape
    dev = x.device
    tg = _ctc_targets("ctc_emissions", targets, B, dev)
    Smax = tg.shape[1]
    fr = _ctc_lengths("ctc_emissions.frames", frames, B, dev, Lq)
    tl = _ctc_lengths("ctc_emissions.tlen", tlen, B, dev, Smax)
    emis = torch.empty((B, Lq, Smax + 1), device=dev, dtype=torch.float32)
    check(L.lib().vasr_ctc_emissions_f32(x.data_ptr(), x.stride(1), x.stride(0), B, Lq, V, tg.data_ptr(), Smax,
                                         fr.data_ptr(), tl.data_ptr(), int(blank), emis.data_ptr(), stream_of(x)),
          "vasr_ctc_emissions_f32")
    return emis, tg, fr, tl


def _ctc_lattice_args(who: str, emis: torch.Tensor, targets: torch.Tensor, frames: torch.Tensor, tlen: torch.Tensor):
    _cuda_f32(f"{who}.emis", emis)
    if emis.dim() != 3 or not emis.is_contiguous():
        raise ValueError(f"{who}: emis must be a contiguous (B, L, Smax + 1) tensor")
    B, Lq, E = emis.shape
    dev = emis.device
    tg = _ctc_targets(who, targets, B, dev)
    if tg.shape[1] != E - 1:
        raise ValueError(f"{who}: targets of width {tg.shape[1]} for emissions of {E - 1} slots")
    fr = _ctc_lengths(f"{who}.frames", frames, B, dev, Lq)
    return B, Lq, E - 1, tg, fr, _ctc_lengths(f"{who}.tlen", tlen, B, dev, E - 1)


def ctc_loss(emis: torch.Tensor, targets: torch.Tensor, frames=None, tlen=None) -> torch.Tensor:
    """Negative log-likelihood (B,) float32 of each utterance's targets over ctc_emissions' output;
    +inf for an infeasible target.  Enqueued on the current stream, no host synchronisation."""
    B, Lq, Smax, tg, fr, tl = _ctc_lattice_args("ctc_loss", emis, targets, frames, tlen)
    nll = torch.empty((B,), device=emis.device, dtype=torch.float32)
    check(L.lib().vasr_ctc_loss_f32(emis.data_ptr(), B, Lq, Smax, tg.data_ptr(), fr.data_ptr(), tl.data_ptr(),
                                    nll.data_ptr(), stream_of(emis)), "vasr_ctc_loss_f32")
    return nll


def ctc_align(emis: torch.Tensor, targets: torch.Tensor, frames=None, tlen=None):
    """Best (Viterbi) CTC path of each utterance's targets over ctc_emissions' output ->
    (frame_state (B, L) int32: target index per frame, -1 = blank / padding; start, end (B, Smax)
    int32: token j's first frame and one past its last; score (B,) float32), all on the device.
    An infeasible target has score -inf and -1 everywhere."""
    B, Lq, Smax, tg, fr, tl = _ctc_lattice_args("ctc_align", emis, targets, frames, tlen)
    dev = emis.device
    nbytes = int(L.lib().vasr_ctc_align_workspace_bytes(B, Lq, Smax))
    ws = torch.empty(max(nbytes // 4, 1), device=dev, dtype=torch.int32)
    state = torch.empty((B, Lq), device=dev, dtype=torch.int32)
    st = torch.empty((B, Smax), device=dev, dtype=torch.int32)
    en = torch.empty((B, Smax), device=dev, dtype=torch.int32)
    score = torch.empty((B,), device=dev, dtype=torch.float32)
    check(L.lib().vasr_ctc_align_f32(emis.data_ptr(), B, Lq, Smax, tg.data_ptr(), fr.data_ptr(), tl.data_ptr(),
                                     ws.data_ptr(), nbytes, state.data_ptr(), st.data_ptr(), en.data_ptr(),
                                     score.data_ptr(), stream_of(emis)), "vasr_ctc_align_f32")
    return state, st, en, score


def ctc_loss_alpha(emis: torch.Tensor, targets: torch.Tensor, frames=None, tlen=None):
    """ctc_loss that also keeps the forward lattice -> (nll (B,), alpha (B, L, 2 Smax + 1) float32):
    nll is bitwise ctc_loss's; alpha[b][t][s] is written for t < frames[b], s <= 2 tlen[b] and
    unspecified elsewhere.  The forward half of the differentiable loss."""
    B, Lq, Smax, tg, fr, tl = _ctc_lattice_args("ctc_loss_alpha", emis, targets, frames, tlen)
    nll = torch.empty((B,), device=emis.device, dtype=torch.float32)
    alpha = torch.empty((B, Lq, 2 * Smax + 1), device=emis.device, dtype=torch.float32)
    check(L.lib().vasr_ctc_loss_alpha_f32(emis.data_ptr(), B, Lq, Smax, tg.data_ptr(), fr.data_ptr(), tl.data_ptr(),
                                          nll.data_ptr(), alpha.data_ptr(), alpha.numel(), stream_of(emis)),
          "vasr_ctc_loss_alpha_f32")
    return nll, alpha


def ctc_occupancy(emis: torch.Tensor, alpha: torch.Tensor, nll: torch.Tensor, targets: torch.Tensor, frames=None,
                  tlen=None) -> torch.Tensor:
    """Posterior occupancy (B, L, Smax + 1) float32 of the transcript per frame, from ctc_emissions'
    and ctc_loss_alpha's outputs: [..., 0] the blank (all blank states), [..., 1 + j] target j, in
    linear space.  Padding rows and slots, and an infeasible utterance (nll = +inf), are exact zeros."""
    B, Lq, Smax, tg, fr, tl = _ctc_lattice_args("ctc_occupancy", emis, targets, frames, tlen)
    _cuda_f32("ctc_occupancy.alpha", alpha)
    _cuda_f32("ctc_occupancy.nll", nll)
    if tuple(alpha.shape) != (B, Lq, 2 * Smax + 1) or not alpha.is_contiguous():
        raise ValueError(f"ctc_occupancy: alpha must be a contiguous ({B}, {Lq}, {2 * Smax + 1}) tensor")
    if tuple(nll.shape) != (B,) or not nll.is_contiguous():
        raise ValueError(f"ctc_occupancy: nll must be a contiguous ({B},) tensor")
    occ = torch.empty((B, Lq, Smax + 1), device=emis.device, dtype=torch.float32)
    check(L.lib().vasr_ctc_occupancy_f32(emis.data_ptr(), alpha.data_ptr(), alpha.numel(), nll.data_ptr(), B, Lq, Smax,
                                         tg.data_ptr(), fr.data_ptr(), tl.data_ptr(), occ.data_ptr(), stream_of(emis)),
          "vasr_ctc_occupancy_f32")
    return occ


def ctc_grad_logits(logits: torch.Tensor, occ: torch.Tensor, targets: torch.Tensor, frames, tlen,
                    scale: torch.Tensor, blank: int = 0) -> torch.Tensor:
    """d(sum_b scale[b] nll_b) / d logits -> contiguous (B, L, V) float32:
    scale[b] (softmax(logits[b, t]) - occupancy gathered per token) for t < frames[b], zeros after.
    One pass that recomputes each row's log-sum-exp; no (B, L, V) log-softmax tensor, no atomics."""
    _cuda_f32("ctc_grad_logits.logits", logits)
    if logits.dim() != 3:
        raise ValueError("ctc_grad_logits: logits must be (B, L, V)")
    x = logits if logits.stride(-1) == 1 else logits.contiguous()
    V = x.shape[2]
    B, Lq, Smax, tg, fr, tl = _ctc_lattice_args("ctc_grad_logits", occ, targets, frames, tlen)
    if tuple(x.shape[:2]) != (B, Lq):
        raise ValueError(f"ctc_grad_logits: logits {tuple(x.shape)} for an occupancy of {B} x {Lq} rows")
    _cuda_f32("ctc_grad_logits.scale", scale)
    if tuple(scale.shape) != (B,) or not scale.is_contiguous():
        raise ValueError(f"ctc_grad_logits: scale must be a contiguous ({B},) tensor")
    chain = torch.empty((B, Smax + 1), device=x.device, dtype=torch.int32)
    grad = torch.empty((B, Lq, V), device=x.device, dtype=torch.float32)
    check(L.lib().vasr_ctc_grad_logits_f32(x.data_ptr(), x.stride(1), x.stride(0), B, Lq, V, tg.data_ptr(), Smax,
                                           fr.data_ptr(), tl.data_ptr(), int(blank), occ.data_ptr(), scale.data_ptr(),
                                           chain.data_ptr(), chain.numel(), grad.data_ptr(), stream_of(x)),
          "vasr_ctc_grad_logits_f32")
    return grad


def _head_operands(who: str, a: torch.Tensor, w: torch.Tensor, bias, ln):
    """The fp32 operands of the logit-free head ops: (rows a after the optional LayerNorm, w, bias)."""
    _cuda_f32(f"{who}.a", a)
    _cuda_f32(f"{who}.w", w)
    if bias is not None:
        _cuda_f32(f"{who}.bias", bias)
        if bias.dim() != 1 or bias.shape[0] != w.shape[0] or not bias.is_contiguous():
            raise ValueError(f"{who}: bias must be a contiguous ({w.shape[0]},) tensor")
    a = _ln_prologue(a, ln)
    M, K, lda = _rows(f"{who}.a", a)
    N, Kw, ldw = _rows(f"{who}.w", w)
    if Kw != K:
        raise ValueError(f"{who}: a has K={K} but w has K={Kw}")
    return a, (M, K, lda), (N, ldw)


def _gemm_lse_pairs(a: torch.Tensor, w: torch.Tensor, bias, dims, wdims, pairs: Optional[torch.Tensor] = None):
    """The VASR_EPI_LSE GEMM: (M, ceil(N/32)) float pairs {m, s} of a @ w.T + bias per row."""
    (M, K, lda), (N, ldw) = dims, wdims
    slots = (N + 31) // 32
    if pairs is None:
        pairs = torch.empty((M, slots, 2), device=a.device, dtype=torch.float32)  # every slot is written
    args = GemmArgs()
    args.A, args.lda, args.stride_a = a.data_ptr(), lda, 0
    args.W, args.ldw = w.data_ptr(), ldw
    args.bias = ptr(bias)
    args.C, args.ldc, args.stride_c = pairs.data_ptr(), pairs.stride(0) // 2, 0
    args.batch, args.M, args.N, args.K = 1, M, N, K
    args.epilogue = L.EPI_LSE
    ev = _t0("gemm")
    _linear(args, w, stream_of(a))
    _t1("gemm", ev, dict(M=M, N=N, K=K, batch=1))
    return pairs, slots


def lse_combine(pairs: torch.Tensor, slots: int) -> torch.Tensor:
    """(M, ld, 2) float pairs of a VASR_EPI_LSE GEMM, `slots` used per row -> stats (M, 2) = {Ms, lse}."""
    _cuda_f32("lse_combine.pairs", pairs)
    if pairs.dim() != 3 or pairs.shape[2] != 2 or pairs.stride(2) != 1 or pairs.stride(1) != 2:
        raise ValueError("lse_combine: pairs must be (M, ld, 2) with contiguous slots")
    M = pairs.shape[0]
    stats = torch.empty((M, 2), device=pairs.device, dtype=torch.float32)
    check(L.lib().vasr_lse_combine_f32(pairs.data_ptr(), pairs.stride(0) // 2 if M > 1 else pairs.shape[1], int(slots), M,
                                       stats.data_ptr(), stream_of(pairs)), "vasr_lse_combine_f32")
    return stats


def gemm_lse(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, ln=None,
             pairs: Optional[torch.Tensor] = None) -> torch.Tensor:
    """stats (M, 2) = {Ms, lse} of the rows of a @ w.T + bias, fused into the GEMM epilogue
    (VASR_EPI_LSE) and one small combine: the (M, N) product is never written.  Ms is the row
    maximum (0 for a row of -inf), lse = log(sum(exp(x - Ms))): log_softmax(x) = (x - Ms) - lse.
    fp32 weights only.  ln = (weight, bias, eps): LayerNorm each row of `a` first.  pairs: a
    caller's (M, ld >= ceil(N/32), 2) float32 buffer for the GEMM's partial pairs."""
    a, dims, wdims = _head_operands("gemm_lse", a, w, bias, ln)
    if pairs is not None:
        _cuda_f32("gemm_lse.pairs", pairs)
        if pairs.dim() != 3 or pairs.shape[0] != dims[0] or pairs.shape[1] < (wdims[0] + 31) // 32 \
                or pairs.shape[2] != 2 or not pairs.is_contiguous():
            raise ValueError(f"gemm_lse: pairs must be a contiguous ({dims[0]}, >= {(wdims[0] + 31) // 32}, 2) tensor")
    pairs, slots = _gemm_lse_pairs(a, w, bias, dims, wdims, pairs)
    return lse_combine(pairs, slots)


def ctc_head_emissions(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], targets: torch.Tensor,
                       frames=None, tlen=None, blank: int = 0, *, B: int, ln=None):
    """ctc_emissions of the logits a @ w.T + bias (a: B * L rows, utterance-major) without the
    logits -> (emis (B, L, Smax + 1), stats (B * L, 2), targets, frames, tlen): the row statistics
    from gemm_lse, the blank's and the target tokens' logits as dot products accumulated in fp64
    (vasr_ctc_head_emissions_f32).  Memory does not grow with rows x vocabulary.  fp32 weights only."""
    a, dims, wdims = _head_operands("ctc_head_emissions", a, w, bias, ln)
    (M, K, lda), (V, ldw) = dims, wdims
    if B <= 0 or M % B:
        raise ValueError(f"ctc_head_emissions: {M} rows do not split into B={B} utterances")
    Lq = M // B
    dev = a.device
    tg = _ctc_targets("ctc_head_emissions", targets, B, dev)
    Smax = tg.shape[1]
    fr = _ctc_lengths("ctc_head_emissions.frames", frames, B, dev, Lq)
    tl = _ctc_lengths("ctc_head_emissions.tlen", tlen, B, dev, Smax)
    pairs, slots = _gemm_lse_pairs(a, w, bias, dims, wdims)
    stats = lse_combine(pairs, slots)
    del pairs
    emis = torch.empty((B, Lq, Smax + 1), device=dev, dtype=torch.float32)
    check(L.lib().vasr_ctc_head_emissions_f32(a.data_ptr(), lda, w.data_ptr(), ldw, ptr(bias), stats.data_ptr(), B, Lq, V,
                                              K, tg.data_ptr(), Smax, fr.data_ptr(), tl.data_ptr(), int(blank),
                                              emis.data_ptr(), stream_of(a)), "vasr_ctc_head_emissions_f32")
    return emis, stats, tg, fr, tl


def ctc_grad_logits_stats(logits: torch.Tensor, stats: torch.Tensor, occ: torch.Tensor, targets: torch.Tensor, frames,
                          tlen, scale: torch.Tensor, blank: int = 0) -> torch.Tensor:
    """ctc_grad_logits in place: `logits` (B, L, V) contiguous holds the logits on entry and the
    gradient on return (it is returned); the rows' {Ms, lse} come from stats (B * L, 2) instead of a
    pass over the row."""
    _cuda_f32("ctc_grad_logits_stats.logits", logits)
    if logits.dim() != 3 or not logits.is_contiguous():
        raise ValueError("ctc_grad_logits_stats: logits must be a contiguous (B, L, V) tensor")
    V = logits.shape[2]
    B, Lq, Smax, tg, fr, tl = _ctc_lattice_args("ctc_grad_logits_stats", occ, targets, frames, tlen)
    if tuple(logits.shape[:2]) != (B, Lq):
        raise ValueError(f"ctc_grad_logits_stats: logits {tuple(logits.shape)} for an occupancy of {B} x {Lq} rows")
    _cuda_f32("ctc_grad_logits_stats.stats", stats)
    if stats.numel() != B * Lq * 2 or not stats.is_contiguous():
        raise ValueError(f"ctc_grad_logits_stats: stats must be a contiguous ({B * Lq}, 2) tensor")
    _cuda_f32("ctc_grad_logits_stats.scale", scale)
    if tuple(scale.shape) != (B,) or not scale.is_contiguous():
        raise ValueError(f"ctc_grad_logits_stats: scale must be a contiguous ({B},) tensor")
    chain = torch.empty((B, Smax + 1), device=logits.device, dtype=torch.int32)
    check(L.lib().vasr_ctc_grad_logits_stats_f32(logits.data_ptr(), logits.stride(1), logits.stride(0), B, Lq, V,
                                                 stats.data_ptr(), tg.data_ptr(), Smax, fr.data_ptr(), tl.data_ptr(),
                                                 int(blank), occ.data_ptr(), scale.data_ptr(), chain.data_ptr(),
                                                 chain.numel(), stream_of(logits)), "vasr_ctc_grad_logits_stats_f32")
    return logits


# ---------------------------------------------------------------- greedy decode with confidences

def gemm_argmax_lse(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, ln=None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The VASR_EPI_ARGMAX_LSE GEMM of a @ w.T + bias: (M, ld) int64 slots, 2 * ceil(N/32) used per row,
    slot 2g the argmax key of columns 32g .. 32g + 31 and slot 2g + 1 their {m, s} float pair; the
    (M, N) product is never written.  fp32 weights only.  ln = (weight, bias, eps): LayerNorm each
    row of `a` first.  out: a caller's contiguous (M, ld >= 2 * ceil(N/32)) int64 buffer."""
    a, (M, K, lda), (N, ldw) = _head_operands("gemm_argmax_lse", a, w, bias, ln)
    nslots = 2 * ((N + 31) // 32)
    if out is None:
        out = torch.empty((M, nslots), device=a.device, dtype=torch.int64)  # every used slot is written
    elif (out.device != a.device or out.dtype != torch.int64 or out.dim() != 2 or out.shape[0] != M
          or out.shape[1] < nslots or not out.is_contiguous()):
        raise ValueError(f"gemm_argmax_lse: out must be a contiguous int64 ({M}, >= {nslots}) tensor on {a.device}")
    args = GemmArgs()
    args.A, args.lda, args.stride_a = a.data_ptr(), lda, 0
    args.W, args.ldw = w.data_ptr(), ldw
    args.bias = ptr(bias)
    args.C, args.ldc, args.stride_c = out.data_ptr(), out.shape[1], 0
    args.batch, args.M, args.N, args.K = 1, M, N, K
    args.epilogue = L.EPI_ARGMAX_LSE
    ev = _t0("gemm")
    _linear(args, w, stream_of(a))
    _t1("gemm", ev, dict(M=M, N=N, K=K, batch=1))
    return out


def argmax_logp(logits: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(int32 argmax over the last dim as `argmax`, float32 log-softmax value at it)."""
    _cuda_f32("argmax_logp.logits", logits)
    V = logits.shape[-1]
    x2 = logits.reshape(-1, V)
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    rows = x2.shape[0]
    ld = x2.stride(0) if rows > 1 else V
    idx = torch.empty(rows, device=logits.device, dtype=torch.int32)
    lp = torch.empty(rows, device=logits.device, dtype=torch.float32)
    check(L.lib().vasr_argmax_logp_f32(x2.data_ptr(), ld, rows, V, idx.data_ptr(), lp.data_ptr(), stream_of(logits)),
          "vasr_argmax_logp_f32")
    return idx.view(logits.shape[:-1]), lp.view(logits.shape[:-1])


def _conf_outputs(who: str, B: int, Lq: int, device, frames):
    toks, lens, st, en, frames = _collapse_outputs(who, B, Lq, device, None, True, frames)
    lsum = torch.empty((B, Lq), device=device, dtype=torch.float32)
    lmin = torch.empty((B, Lq), device=device, dtype=torch.float32)
    path = torch.empty((B,), device=device, dtype=torch.float32)
    return toks, lens, st, en, lsum, lmin, path, frames


def ctc_collapse_conf(pred: torch.Tensor, logp: torch.Tensor, blank: int = 0, frames: Optional[torch.Tensor] = None):
    """Greedy CTC collapse of (B, L) int32 predictions with the float32 log-probability of each ->
    (tokens, lengths, start, end, logp_sum, logp_min, path_logp): the first four as
    ctc_collapse(timestamps=True); logp_sum / logp_min (B, L) the sum / minimum of logp over each
    kept token's run of frames; path_logp (B,) the sum over the utterance's frames.  frames:
    per-utterance row counts (int32 (B,)) of a padded batch."""
    if pred.device.type != "cuda" or pred.dtype != torch.int32:
        raise TypeError("ctc_collapse_conf: expected a cuda int32 pred")
    _cuda_f32("ctc_collapse_conf.logp", logp)
    if pred.dim() != 2 or logp.shape != pred.shape or logp.device != pred.device:
        raise ValueError("ctc_collapse_conf: pred and logp must be (B, L) tensors on one device")
    pred, logp = pred.contiguous(), logp.contiguous()
    B, Lq = pred.shape
    toks, lens, st, en, lsum, lmin, path, frames = _conf_outputs("ctc_collapse_conf", B, Lq, pred.device, frames)
    check(L.lib().vasr_ctc_collapse_conf(pred.data_ptr(), logp.data_ptr(), B, Lq, ptr(frames), int(blank),
                                         toks.data_ptr(), lens.data_ptr(), st.data_ptr(), en.data_ptr(),
                                         lsum.data_ptr(), lmin.data_ptr(), path.data_ptr(), stream_of(pred)),
          "vasr_ctc_collapse_conf")
    return toks, lens, st, en, lsum, lmin, path


def ctc_collapse_slots_conf(slots: torch.Tensor, nslots: int, B: int, blank: int = 0,
                            frames: Optional[torch.Tensor] = None, per_frame: bool = False):
    """ctc_collapse_conf straight from gemm_argmax_lse's slots ((B * L, ld) int64, `nslots` used) in one
    launch (vasr_ctc_collapse_keys_conf).  per_frame: also return (pred, logp), the (B, L) per-frame
    argmax and its log-probability (rows past an utterance's `frames` are not written)."""
    if slots.device.type != "cuda" or slots.dtype != torch.int64 or slots.dim() != 2 or not slots.is_contiguous():
        raise TypeError("ctc_collapse_slots_conf: expected a contiguous cuda int64 (rows, ld) tensor")
    M, ld = slots.shape
    if B <= 0 or M % B:
        raise ValueError(f"ctc_collapse_slots_conf: {M} rows do not split into B={B} utterances")
    Lq = M // B
    toks, lens, st, en, lsum, lmin, path, frames = _conf_outputs("ctc_collapse_slots_conf", B, Lq, slots.device, frames)
    pred = lp = None
    if per_frame:
        pred = torch.empty((B, Lq), device=slots.device, dtype=torch.int32)
        lp = torch.empty((B, Lq), device=slots.device, dtype=torch.float32)
    check(L.lib().vasr_ctc_collapse_keys_conf(slots.data_ptr(), ld, int(nslots), B, Lq, ptr(frames), int(blank),
                                              ptr(pred), ptr(lp), toks.data_ptr(), lens.data_ptr(), st.data_ptr(),
                                              en.data_ptr(), lsum.data_ptr(), lmin.data_ptr(), path.data_ptr(),
                                              stream_of(slots)), "vasr_ctc_collapse_keys_conf")
    res = (toks, lens, st, en, lsum, lmin, path)
    return res + (pred, lp) if per_frame else res


def gemm_ctc_greedy_conf(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], B: int, blank: int = 0, *,
                         ln=None, frames: Optional[torch.Tensor] = None, per_frame: bool = False):
    """Greedy CTC decode of B utterances (a: B * L rows) with confidences and without logits: the
    VASR_EPI_ARGMAX_LSE GEMM, then one launch that folds its slots and collapses
    (ctc_collapse_slots_conf).  Returns ctc_collapse_conf's tuple (plus (pred, logp) with per_frame)."""
    slots = gemm_argmax_lse(a, w, bias, ln=ln)
    return ctc_collapse_slots_conf(slots, 2 * ((w.shape[0] + 31) // 32), B, blank, frames, per_frame)


def _prefix_beam_table(who: str, lm_table, V: int):
    if lm_table is None:
        return None
    _cuda_f32(f"{who}.lm_table", lm_table)
    if tuple(lm_table.shape) != (V + 1, V):
        raise ValueError(f"{who}: lm_table must be ({V + 1}, {V}), got {tuple(lm_table.shape)}")
    return lm_table if lm_table.stride(-1) == 1 else lm_table.contiguous()


def ctc_prefix_beam_search(logits: torch.Tensor, beam_width: int, blank: int = 0, *, frames=None, lm_table=None,
                           alpha: float = 0.0, beta: float = 0.0):
    """The standard CTC prefix beam search (vasr_ctc_prefix_beam_search) over (B, L, V)
    logits -> (tokens (B, W, L) int32, lengths (B, W), scores (B, W) float64, log-probabilities (B, W)
    float64, beams per utterance (B,)), all on the device.  A prefix carries the summed probability of
    its alignments; score = (logp + alpha * S(prefix)) + beta * len(prefix), S the (V + 1, V) bigram
    table's score (active when lm_table is given and alpha > 0), each token scored once.  frames as
    ctc_beam_search.  V <= 16384, beam_width <= 32."""
    who = "ctc_prefix_beam_search"
    _cuda_f32(f"{who}.logits", logits)
    if logits.dim() != 3:
        raise ValueError(f"{who}: logits must be (B, L, V)")
    x = logits if logits.stride(-1) == 1 else logits.contiguous()
    B, Lq, V = x.shape
    W, dev = int(beam_width), x.device
    fr = _beam_frames(who, frames, B, Lq, dev)
    tab = _prefix_beam_table(who, lm_table, V)
    trie, toks, lens, scores, nbeams = _beam_buffers(B, Lq, W, dev)
    logp = torch.zeros((B, W), device=dev, dtype=torch.float64)
    check(L.lib().vasr_ctc_prefix_beam_search(x.data_ptr(), x.stride(1), x.stride(0), B, Lq, V, W, int(blank), ptr(fr),
                                              ptr(tab), 0 if tab is None else tab.stride(0), float(alpha), float(beta),
                                              trie.data_ptr(), toks.data_ptr(), lens.data_ptr(), scores.data_ptr(),
                                              logp.data_ptr(), nbeams.data_ptr(), stream_of(x)),
          "vasr_ctc_prefix_beam_search")
    return toks, lens, scores, logp, nbeams


def ctc_prefix_beam_search_shortlist(tok: torch.Tensor, lp: torch.Tensor, blank_lp: torch.Tensor, V: int, beam_width: int,
                                     blank: int = 0, *, frames=None, lm_table=None, alpha: float = 0.0, beta: float = 0.0):
    """ctc_prefix_beam_search with token pruning (vasr_ctc_prefix_beam_search_shortlist): the search over
    ctc_beam_shortlist's arrays, every token outside a frame's K best counting as -inf.  An
    approximation, without a certificate.  V: the vocabulary size (up to 2^20).  Returns the same five
    tensors."""
    who = "ctc_prefix_beam_search_shortlist"
    _cuda_f32(f"{who}.lp", lp)
    _cuda_f32(f"{who}.blank_lp", blank_lp)
    if lp.dim() != 3 or not lp.is_contiguous():
        raise ValueError(f"{who}: lp must be a contiguous (B, L, K) tensor")
    B, Lq, K = lp.shape
    V, W, dev = int(V), int(beam_width), lp.device
    if (tok.device != dev or tok.dtype != torch.int32 or tok.shape != lp.shape or not tok.is_contiguous()
            or tuple(blank_lp.shape) != (B, Lq) or not blank_lp.is_contiguous()):
        raise ValueError(f"{who}: tok must be int32 (B, L, K) and blank_lp (B, L), contiguous, beside lp")
    if not 1 <= K <= min(BEAM_SHORTLIST_MAX, V - 1):
        raise ValueError(f"{who}: K = {K} outside 1..{min(BEAM_SHORTLIST_MAX, V - 1)} for V = {V}")
    fr = _beam_frames(who, frames, B, Lq, dev)
    tab = _prefix_beam_table(who, lm_table, V)
    trie, toks, lens, scores, nbeams = _beam_buffers(B, Lq, W, dev)
    logp = torch.zeros((B, W), device=dev, dtype=torch.float64)
    check(L.lib().vasr_ctc_prefix_beam_search_shortlist(tok.data_ptr(), lp.data_ptr(), blank_lp.data_ptr(), K, V, B, Lq, W,
                                                        int(blank), ptr(fr), ptr(tab), 0 if tab is None else tab.stride(0),
                                                        float(alpha), float(beta), trie.data_ptr(), toks.data_ptr(),
                                                        lens.data_ptr(), scores.data_ptr(), logp.data_ptr(),
                                                        nbeams.data_ptr(), stream_of(lp)),
          "vasr_ctc_prefix_beam_search_shortlist")
    return toks, lens, scores, logp, nbeams
