"""Selective SSM blocks (drop-in for reference velocity_asr/ssm.py) on MI355X kernels.

Same module tree, parameter names and shapes as the reference, so state_dicts load
unchanged.  Forward passes run the HIP kernels of libvasr_hip.so:

  SSMBlock:  LN1 + causal depthwise conv (one kernel)
             -> in_proj GEMM (fp32 MFMA)
             -> [x_proj; dt_proj] as ONE GEMM with bias + softplus fused on the dt columns
             -> gated selective scan (tree or recurrence) with D skip and y*silu(z) fused
             -> out_proj GEMM with the residual add fused
             -> LN2 -> FFN1 GEMM + GELU -> FFN2 GEMM + bias + residual
forward() is inference only: dropout is the identity (as in eval()), no autograd.  Training goes
through selective_scan -- either scan (the recurrence of "sequential" / "mamba", the tree of the
default "parallel") as an autograd operator with a HIP backward pass -- and the modules'
forward_differentiable (SelectiveSSM, SSMBlock, LocalSSMProcessor, GlobalSSM).
"""

from __future__ import annotations

import math
import os
import warnings
from typing import Literal, Optional

import torch
import torch.nn as nn

from . import _lib, ops
from ._prep import cached

ScanMode = Literal["sequential", "parallel", "mamba"]

# The reference imports mamba_ssm's selective_scan_fn for scan_mode="mamba"
# (ssm.py:20-26).  Here that operator contract is served by the HIP recurrence kernel
# (vasr_ssm_scan_f32 mode 1, the semantics selective_scan_fn computes), so the mode is
# always available.
MAMBA_AVAILABLE = True

_SCAN_MODE_ID = {"parallel": 0, "sequential": 1, "mamba": 1}


def _tree_mode() -> int:
    """Kernel mode of scan_mode="parallel": 2 (default) = the reference's tree with fused
    multiply-adds and (x*dt)*B (a third fewer state-update instructions: 97 vs 106 us per
    16-clip launch, tokens identical); 0 = the reference tree op for op (two roundings per
    a*b + c, x*(dt*B)).  VASR_SCAN_FMA=0|1 selects; read per call so tests can switch it."""
    return 0 if os.environ.get("VASR_SCAN_FMA", "1") == "0" else 2
_warned_training = False


def _bf16_compose() -> bool:
    """The bf16 model's composed projection (SelectiveSSM._prepared); VASR_BF16_COMPOSE=0 selects
    the two GEMMs (read per call so tests can compare the two)."""
    return os.environ.get("VASR_BF16_COMPOSE", "1") != "0"


def _check_eval(module: nn.Module) -> None:
    global _warned_training
    if module.training and not _warned_training:
        _warned_training = True
        warnings.warn("velocity_asr (MI355X build) is inference-only: dropout is treated as identity; "
                      "call model.eval() to silence this warning", stacklevel=3)


def _scan_operands(x, dt, A, B, C, D, z):
    """Validate selective_scan's arguments (ValueError) and return (batch, L, Di, N)."""
    names = (("x", x, 3), ("dt", dt, 3), ("A", A, 1), ("B", B, 3), ("C", C, 3), ("D", D, 1)) + (
        (("z", z, 3),) if z is not None else ())
    for n, t, rank in names:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"selective_scan: {n} must be a tensor")
        if t.dim() != rank:
            raise ValueError(f"selective_scan: {n} must have {rank} dimensions, got shape {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"selective_scan: {n} must be float32, got {t.dtype} (the operator is fp32 only)")
    batch, L, Di = x.shape
    N = A.shape[0]
    want = dict(dt=(batch, L, Di), B=(batch, L, N), C=(batch, L, N), D=(Di,), z=(batch, L, Di))
    for n, t, _ in names:
        if n in want and tuple(t.shape) != want[n]:
            raise ValueError(f"selective_scan: {n} has shape {tuple(t.shape)}, expected {want[n]}")
    if N < 1 or L > 8192:
        raise ValueError(f"selective_scan: state dim {N} / length {L} out of range (N >= 1, L <= 8192)")
    return batch, L, Di, N


def _pad_states(B, C, A, N, Np):
    """[B | C] rows (M, 2 Np) and A (Np,) with the state dim zero-padded to the kernel's (ops.ssm_scan's
    rule: A = 0, B = C = 0 there, so the padded states stay exactly 0)."""
    M = B.shape[0] * B.shape[1]
    Bm, Cm = B.reshape(M, N), C.reshape(M, N)
    if Np == N:
        return torch.cat([Bm, Cm], 1), A.contiguous()
    pad = torch.zeros((M, Np - N), device=B.device, dtype=B.dtype)
    return torch.cat([Bm, pad, Cm, pad], 1), torch.cat([A, torch.zeros(Np - N, device=A.device, dtype=A.dtype)])


def _input_grads(r, need, batch, L, Di, N):
    """ops.ssm_scan_bwd's / ops.ssm_tree_bwd's dict as the gradients of (x, dt, A, B, C, D, z): dA and dD summed
    from their per-(utterance, channel) partials, a padded state dim sliced back, None where not needed."""
    return (r["dx"].view(batch, L, Di) if need[0] else None,
            r["ddt"].view(batch, L, Di) if need[1] else None,
            r["dA_part"].sum(dim=(0, 1))[:N] if need[2] else None,
            r["dB"][:, :N].reshape(batch, L, N) if need[3] else None,
            r["dC"][:, :N].reshape(batch, L, N) if need[4] else None,
            r["dD_part"].sum(dim=0) if need[5] else None,
            r["dz"].view(batch, L, Di) if r["dz"] is not None and need[6] else None)


class _SelectiveScan(torch.autograd.Function):
    """out = selective scan (the true recurrence) with gradients to all seven inputs.  Forward:
    ops.ssm_scan_save (the mode-1 kernel, also keeping the state at every 16-step chunk boundary).
    Backward: ops.ssm_scan_bwd, the reverse-time walk from those checkpoints; dA and dD are the sums
    of its per-(utterance, channel) partials.  Enqueued on the current stream, no host sync."""

    @staticmethod
    def forward(ctx, x, dt, A, B, C, D, z):
        batch, L, Di, N = _scan_operands(x, dt, A, B, C, D, z)
        Np = ops.scan_state_dim(N)
        M = batch * L
        with torch.no_grad():
            if z is not None:
                xz = torch.cat([x.reshape(M, Di), z.reshape(M, Di)], 1)
                xs, zs = xz[:, :Di], xz[:, Di:]
            else:
                xs, zs = x.reshape(M, Di).contiguous(), None
            dts = dt.reshape(M, Di).contiguous()
            bc, Ap = _pad_states(B, C, A, N, Np)
            A2 = Ap * torch.tensor(ops.LOG2E, dtype=torch.float32)
            Dc = D.contiguous()
            out, ckpt = ops.ssm_scan_save(xs, zs, dts, bc, A2, Dc, batch, L)
        ctx.save_for_backward(xs, dts, bc, Ap, A2, Dc, ckpt, *(() if zs is None else (zs,)))
        ctx.dims = (batch, L, Di, N)
        return out.view(batch, L, Di)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        xs, dts, bc, Ap, A2, Dc, ckpt, *rest = ctx.saved_tensors
        zs = rest[0] if rest else None
        batch, L, Di, N = ctx.dims
        r = ops.ssm_scan_bwd(xs, zs, dts, bc, Ap, A2, Dc, g.to(torch.float32).reshape(batch * L, Di).contiguous(),
                             ckpt, batch, L)
        return _input_grads(r, ctx.needs_input_grad, batch, L, Di, N)


class _TreeScan(torch.autograd.Function):
    """out = the reference's tree scan (scan_mode="parallel") with gradients to all seven inputs.
    Forward: the inference kernel itself (ops.ssm_scan at _tree_mode(), ops.ssm_scan_ungated without
    z), so out is bitwise the inference value and only the inputs are saved.  Backward:
    ops.ssm_tree_bwd, which recomputes what it needs; dA and dD are the sums of its
    per-(utterance, channel) partials.  Enqueued on the current stream, no host sync."""

    @staticmethod
    def forward(ctx, x, dt, A, B, C, D, z):
        batch, L, Di, N = _scan_operands(x, dt, A, B, C, D, z)
        Np = ops.scan_state_dim(N)
        with torch.no_grad():
            xs, zs, dts, bc, Ap, A2, Dc, out = _tree_forward(x, dt, A, B, C, D, z, batch, L, Di, N, Np)
        ctx.save_for_backward(xs, dts, bc, Ap, A2, Dc, *(() if zs is None else (zs,)))
        ctx.dims = (batch, L, Di, N)
        return out.view(batch, L, Di)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        xs, dts, bc, Ap, A2, Dc, *rest = ctx.saved_tensors
        zs = rest[0] if rest else None
        batch, L, Di, N = ctx.dims
        r = ops.ssm_tree_bwd(xs, zs, dts, bc, Ap, A2, Dc, g.to(torch.float32).reshape(batch * L, Di).contiguous(),
                             batch, L)
        return _input_grads(r, ctx.needs_input_grad, batch, L, Di, N)


def _tree_forward(x, dt, A, B, C, D, z, batch, L, Di, N, Np):
    """The tree scan by the inference kernels on (B L, .) rows; returns the packed operands and out."""
    M = batch * L
    dts = dt.reshape(M, Di).contiguous()
    bc, Ap = _pad_states(B, C, A, N, Np)
    A2 = Ap * torch.tensor(ops.LOG2E, dtype=torch.float32)
    Dc = D.contiguous()
    if z is not None:
        xz = torch.cat([x.reshape(M, Di), z.reshape(M, Di)], 1)
        xs, zs = xz[:, :Di], xz[:, Di:]
        out = ops.ssm_scan(xz, dts, bc, A2, Dc, batch, L, _tree_mode())
    else:
        xs, zs = x.reshape(M, Di).contiguous(), None
        out = ops.ssm_scan_ungated(xs, dts, bc, A2, Dc, batch, L, _tree_mode())
    return xs, zs, dts, bc, Ap, A2, Dc, out


_UNIT_GATE = 128.0  # silu(128) == 128 exactly in fp32 (exp(-128) rounds to 0): y * 128 / 128 is y, bitwise


def selective_scan(x: torch.Tensor, dt: torch.Tensor, A: torch.Tensor, B: torch.Tensor, C: torch.Tensor,
                   D: torch.Tensor, z: Optional[torch.Tensor] = None, *,
                   scan_mode: ScanMode = "sequential") -> torch.Tensor:
    """The selective scan as a differentiable operator: the reference's SelectiveSSM._sequential_scan
    (ssm.py:134-171) with the D skip, times silu(z) when z is given -- what mamba_ssm's
    selective_scan_fn computes for a state matrix shared across channels.

        h_t = exp(dt_t A) h_{t-1} + dt_t x_t B_t,   out_t = (sum_n h_t C_t + x_t D) [* silu(z_t)]

    x, dt, z: (batch, L, Di); A: (N,); B, C: (batch, L, N); D: (Di,); float32 on a HIP device.  All
    seven inputs get gradients from the HIP backward kernel (vasr_ssm_scan_bwd_f32); the forward
    value is bitwise the inference kernel's (ops.ssm_scan, mode 1).  When nothing requires grad the
    inference kernel itself runs and no checkpoint is written.  A state dim without a kernel
    instance (e.g. 48) runs zero-padded to the next one and dA, dB, dC are sliced back.  Di must be
    a multiple of 1024 / N' channels (N' the kernel state dim), L <= 8192.

    scan_mode "sequential" and "mamba" are that recurrence.  "parallel" is the model's default, the
    reference's tree scan (_parallel_scan, ssm.py:173-295): with P_e = prod_{r <= e} exp(dt_r A),

        h_t = sum over the set bits k of t of P_{e_S} R_S,   S = [t with bits 0..k cleared, + 2^k),

    R_S the recurrence run over S alone from a zero state (so h_0 = 0); out as above.  Its forward
    is the inference kernel itself (ops.ssm_scan at the tree mode VASR_SCAN_FMA selects,
    ops.ssm_scan_ungated without z), bitwise, and only the inputs are kept; its gradients come from
    vasr_ssm_tree_bwd_f32.  Shapes, padding and limits are the same.

    Batches are full-length.  Either scan is causal, so for a padded batch zero the upstream gradient
    on the padded frames: the gradients of the valid frames and of the parameters are then exact."""
    batch, L, Di, N = _scan_operands(x, dt, A, B, C, D, z)
    if scan_mode not in _SCAN_MODE_ID:
        raise ValueError(f"selective_scan: unknown scan_mode {scan_mode!r} ('sequential', 'parallel' or 'mamba')")
    _lib.require_device()
    Np = ops.scan_state_dim(N)
    if Di % ops.scan_bwd_channels(Np):
        raise ValueError(f"selective_scan: Di={Di} must be a multiple of {ops.scan_bwd_channels(Np)} at state dim {N}")
    args = (x, dt, A, B, C, D) + ((z,) if z is not None else ())
    needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in args)
    if _SCAN_MODE_ID[scan_mode] == 0:
        if needs_grad:
            return _TreeScan.apply(x, dt, A, B, C, D, z)
        det = [t.detach() for t in (x, dt, A, B, C, D)] + [None if z is None else z.detach()]
        return _tree_forward(*det, batch, L, Di, N, Np)[-1].view(batch, L, Di)
    if needs_grad:
        return _SelectiveScan.apply(x, dt, A, B, C, D, z)
    M = batch * L
    gate = z.reshape(M, Di) if z is not None else torch.full((M, Di), _UNIT_GATE, device=x.device)
    xz = torch.cat([x.detach().reshape(M, Di), gate.detach()], 1)
    bc, Ap = _pad_states(B.detach(), C.detach(), A.detach(), N, Np)
    A2 = Ap * torch.tensor(ops.LOG2E, dtype=torch.float32)
    out = ops.ssm_scan(xz, dt.detach().reshape(M, Di).contiguous(), bc, A2, D.detach().contiguous(), batch, L, 1)
    if z is None:
        out = out / _UNIT_GATE  # the unit gate divided out: exact (a power of two)
    return out.view(batch, L, Di)


class SelectiveSSM(nn.Module):
    """Selective state space model (reference ssm.py:32-337)."""

    def __init__(self, d_model: int = 192, state_dim: int = 64, expand_ratio: int = 2,
                 scan_mode: ScanMode = "parallel"):
        super().__init__()
        self.d_model = d_model
        self.state_dim = state_dim
        self.d_inner = d_model * expand_ratio
        self.scan_mode = scan_mode
        if scan_mode not in _SCAN_MODE_ID:
            raise ValueError(f"Unknown scan_mode: {scan_mode}")
        self.in_proj = nn.Linear(d_model, self.d_inner * 2, bias=False)
        self.x_proj = nn.Linear(self.d_inner, state_dim * 2, bias=False)
        self.dt_proj = nn.Linear(self.d_inner, self.d_inner, bias=True)
        A = torch.arange(1, state_dim + 1, dtype=torch.float32)
        self.A_log = nn.Parameter(torch.log(A))
        self.D = nn.Parameter(torch.ones(self.d_inner))
        self.out_proj = nn.Linear(self.d_inner, d_model, bias=False)

    def _prepared(self):
        def build():
            dev = self.x_proj.weight.device
            N, Np = self.state_dim, ops.scan_state_dim(self.state_dim)
            xw = self.x_proj.weight
            if Np != N:
                # state dims the scan kernels are not built for run as the next size up: zero rows
                # make the GEMM write B and C with Np - N zero columns each, and A2 = 0 there, so
                # the padded states stay exactly 0 and add nothing to y (include/vasr.h)
                z = torch.zeros(Np - N, xw.shape[1], device=dev, dtype=xw.dtype)
                xw = torch.cat([xw[:N], z, xw[N:], z], 0)
            w = torch.cat([xw, self.dt_proj.weight], 0).contiguous()
            b = torch.cat([torch.zeros(2 * Np, device=dev), self.dt_proj.bias.float()]).contiguous()
            # A = -exp(A_log) exactly as the reference evaluates it (float32, ssm.py:116), then
            # pre-scaled by log2(e) so the kernel's dA is one v_exp_f32.
            A = -torch.exp(self.A_log.detach().float().cpu())
            A2 = torch.zeros(Np, dtype=torch.float32)
            A2[:N] = A * torch.tensor(ops.LOG2E, dtype=torch.float32)
            out = dict(w_xdt=w, b_xdt=b, A2=A2.to(dev))
            if w.dtype == torch.float32:
                # composed projection: [x_proj; dt_proj](in_proj_x(u)) = u @ (W_xdt W_in_x)^T, the
                # product formed in float64 and rounded once (see gated_scan)
                Di = self.d_inner
                wc = (w.detach().double() @ self.in_proj.weight.detach()[:Di].double()).float()
                out["w_comb"] = torch.cat([self.in_proj.weight.detach(), wc], 0).contiguous()
                out["b_comb"] = torch.cat([torch.zeros(2 * Di, device=dev), b]).contiguous()
                # the z-in-tail block (SSMBlock._z_in_tail): [x | B | C | dt] without the z rows, and
                # W_z for the tail's own z product (the same rows, so the same split planes)
                out["w_noz"] = torch.cat([self.in_proj.weight.detach()[:Di], wc], 0).contiguous()
                out["b_noz"] = torch.cat([torch.zeros(Di, device=dev), b]).contiguous()
                out["w_z"] = self.in_proj.weight.detach()[Di:].contiguous()
            elif w.dtype == torch.bfloat16 and self.in_proj.weight.dtype == torch.bfloat16:
                # the bf16 model's z-in-tail block: in_proj split into its x rows (the projection
                # GEMM) and its z rows (the tail's product); the bf16 engine's per-column result
                # does not depend on the other columns, so both are bitwise in_proj's
                Di = self.d_inner
                out["w_x"] = self.in_proj.weight.detach()[:Di].contiguous()
                out["w_z"] = self.in_proj.weight.detach()[Di:].contiguous()
                # composed form (default; VASR_BF16_COMPOSE=0: the two GEMMs): [W_in; W_xdt W_in,x] as
                # one bf16 GEMM, the product of the bf16 weights formed in float64 and rounded to bf16
                # once -- one bf16 rounding where the two GEMMs round x_p to bf16 at the second
                # GEMM's input (C3's token edit rate vs the reference 2.28 % vs 2.31 %, profiles/r06ad/)
                wc = (w.detach().double() @ out["w_x"].double()).to(torch.bfloat16)
                out["w_comb16"] = torch.cat([self.in_proj.weight.detach(), wc], 0).contiguous()
                out["b_comb16"] = torch.cat([torch.zeros(2 * Di, device=dev), b]).contiguous()
                out["w_noz16"] = torch.cat([out["w_x"], wc], 0).contiguous()
                out["b_noz16"] = torch.cat([torch.zeros(Di, device=dev), b]).contiguous()
            return out
        return cached(self, "ssm", (self.x_proj.weight, self.dt_proj.weight, self.dt_proj.bias, self.A_log,
                                    self.in_proj.weight), build)

    def gated_scan(self, u: torch.Tensor, B: int, L: int) -> torch.Tensor:
        """u (B*L, d_model) -> y * silu(z) of shape (B*L, d_inner), before out_proj."""
        xz, xdt = self.project(u)
        return self.scan(xz, xdt, B, L)

    def project(self, u: torch.Tensor):
        """u (B*L, d_model) -> (xz, xdt): the scan's operands, [x_p | z] and [B | C | dt]
        (views into one buffer for the composed projection).

        fp32 model (default): in_proj and [x_proj; dt_proj] as ONE GEMM of u against
        [W_in; W_xdt W_in_x] (N = 2 Di + 2N + Di, K = d_model), softplus on the dt columns: the
        composition of two linear maps, with the composed matrix formed in float64 and rounded
        once.  It skips the fp32 rounding of x_p between the two products (a ~1e-7 relative
        difference, the size of GEMM accumulation-order effects) and needs 29 % fewer MACs, one
        launch instead of two and no re-read of x_p.  VASR_XDT_COMPOSE=0 selects the two
        products as the reference evaluates them (ssm.py:105-113)."""
        p = self._prepared()
        Di, N = self.d_inner, ops.scan_state_dim(self.state_dim)
        if "w_comb" in p and os.environ.get("VASR_XDT_COMPOSE", "1") != "0":
            out = ops.gemm(u, p["w_comb"], p["b_comb"], epilogue=_lib.EPI_SOFTPLUS_FROM,
                           n_out=2 * Di + 2 * N)                                 # (M, 2Di + 2N + Di)
            return out[:, :2 * Di], out[:, 2 * Di:]
        if "w_comb16" in p and _bf16_compose():  # the bf16 model's composed form (see _prepared)
            out = ops.gemm(u, p["w_comb16"], p["b_comb16"], epilogue=_lib.EPI_SOFTPLUS_FROM, n_out=2 * Di + 2 * N)
            return out[:, :2 * Di], out[:, 2 * Di:]
        xz = ops.gemm(u, self.in_proj.weight)                                   # (M, 2Di) [x | z]
        xdt = ops.gemm(xz[:, :Di], p["w_xdt"], p["b_xdt"], epilogue=_lib.EPI_SOFTPLUS_FROM,
                       n_out=2 * N)                                              # (M, 2N + Di) [B | C | dt]
        return xz, xdt

    def scan(self, xz: torch.Tensor, xdt: torch.Tensor, B: int, L: int) -> torch.Tensor:
        """The gated scan over in_proj's [x | z] and [B | C | dt]."""
        p = self._prepared()
        N = ops.scan_state_dim(self.state_dim)
        mode = _SCAN_MODE_ID[self.scan_mode]
        return ops.ssm_scan(xz, xdt[:, 2 * N:], xdt[:, :2 * N], p["A2"], self.D, B, L,
                            _tree_mode() if mode == 0 else mode)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _check_eval(self)
        B, L, _ = x.shape
        g = self.gated_scan(x.reshape(B * L, -1), B, L)
        return ops.gemm(g, self.out_proj.weight).view(B, L, self.d_model)

    def forward_differentiable(self, x: torch.Tensor, *, tree_scan: bool = False) -> torch.Tensor:
        """The reference's forward (ssm.py:92-132) for training: the projections, softplus and
        A = -exp(A_log) as torch ops on this module's parameters (torch.autograd differentiates
        them), the scan as selective_scan (HIP forward and backward), then out_proj.  loss.backward()
        reaches all six parameters and x.  By default scan_mode "sequential" and "mamba" only:
        "parallel" reproduces the reference's mis-combined tree, a different function of its inputs
        whose gradient the recurrence's backward kernel does not compute.  tree_scan=True
        differentiates the module's own scan mode, whichever it is: the tree's gradient for
        "parallel" (selective_scan(scan_mode="parallel")), the recurrence's otherwise."""
        if _SCAN_MODE_ID[self.scan_mode] != 1 and not tree_scan:
            raise NotImplementedError(
                f"SelectiveSSM.forward_differentiable: scan_mode={self.scan_mode!r} is the reference's tree scan, "
                "which is not the recurrence the backward kernel differentiates; use 'sequential' or 'mamba', "
                "or pass tree_scan=True for the tree's own gradient")
        F = torch.nn.functional
        xp, z = F.linear(x, self.in_proj.weight).chunk(2, dim=-1)
        Bm, Cm = F.linear(xp, self.x_proj.weight).chunk(2, dim=-1)
        dt = F.softplus(F.linear(xp, self.dt_proj.weight, self.dt_proj.bias))
        A = -torch.exp(self.A_log)
        y = selective_scan(xp, dt, A, Bm, Cm, self.D, z, scan_mode=self.scan_mode)
        return F.linear(y, self.out_proj.weight)


class SSMBlock(nn.Module):
    """Pre-norm conv + SSM + FFN block (reference ssm.py:340-441)."""

    def __init__(self, d_model: int = 192, state_dim: int = 64, expand_ratio: int = 2, kernel_size: int = 4,
                 dropout: float = 0.1, use_checkpoint: bool = False, scan_mode: ScanMode = "parallel"):
        super().__init__()
        self.use_checkpoint = use_checkpoint
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.conv = nn.Conv1d(d_model, d_model, kernel_size=kernel_size, padding=kernel_size - 1, groups=d_model)
        self.ssm = SelectiveSSM(d_model=d_model, state_dim=state_dim, expand_ratio=expand_ratio, scan_mode=scan_mode)
        self.ffn = nn.Sequential(
            nn.Linear(d_model, d_model * expand_ratio),
            nn.GELU(),
            nn.Dropout(dropout),
            nn.Linear(d_model * expand_ratio, d_model),
            nn.Dropout(dropout),
        )
        self.dropout = nn.Dropout(dropout)

    def _fused_tail_ok(self, D: int) -> bool:
        """The one-launch tail (vasr_ssm_block_tail_f32 / _bf16) serves the fp32 and the bf16
        model at d_model 192 / FFN width 384; VASR_FUSED_TAIL=0 selects the launches below (read
        per call so tests can compare the two)."""
        w = self.ffn[0].weight
        dtype_ok = w.dtype in (torch.bfloat16, torch.float32)
        return (os.environ.get("VASR_FUSED_TAIL", "1") != "0" and dtype_ok and D == 192
                and tuple(w.shape) == (384, 192) and self.ssm.d_inner == 384
                and self.ssm.out_proj.weight.dtype == w.dtype == self.ffn[3].weight.dtype)

    def forward(self, x: torch.Tensor, pre_norm: Optional[nn.LayerNorm] = None) -> torch.Tensor:
        """pre_norm (extension): x is the temporal binding's row before its final LayerNorm, which
        this block applies inside its norm1 + conv launch (_norm_conv); the result is bitwise the
        same as for pre_norm(x)."""
        _check_eval(self)
        B, L, D = x.shape
        if self._z_in_tail(B, L, D):
            return self._forward_z_in_tail(x, pre_norm)
        x2, xz, xdt = self.head(x, pre_norm)
        g = self.ssm.scan(xz, xdt, B, L)
        return self.tail(g, x2, B, L)

    def forward_differentiable(self, x: torch.Tensor, *, tree_scan: bool = False) -> torch.Tensor:
        """The reference's _forward_impl (ssm.py:404-427) for training: LayerNorms, the causal
        depthwise conv, the FFN, the residuals and the dropout modules as torch ops on this module's
        parameters, around SelectiveSSM.forward_differentiable(tree_scan=...) (the scan's HIP
        forward and backward).  Dropout follows the module's train() / eval() state."""
        L = x.size(1)
        u = self.conv(self.norm1(x).transpose(1, 2))[:, :, :L].transpose(1, 2)
        x = self.dropout(self.ssm.forward_differentiable(u, tree_scan=tree_scan)) + x
        return self.ffn(self.norm2(x)) + x

    # z-in-tail: z = in_proj_z(u) feeds only the gate y * silu(z)
    # (ssm.py:106, :129).  The projection GEMM -- bound by its C stores -- then
    # skips the z columns, the scan writes the ungated y + x D, and the fused tail forms z itself
    # with the projection GEMM's exact product before applying the gate and the usual tail:
    # bitwise the three-launch block's output (tests/test_ssm_tail.py).  fp32 model: the composed
    # projection writes [x | B | C | dt] (896 of its 1280 columns).  bf16 model: in_proj writes x
    # alone (384 of 768 columns), [x_proj; dt_proj] reads it as before.  Where it runs: the tree
    # scan streamed (ops._use_chunked false) and the 32-row tail (M > 4096 token rows: the
    # bench's batches); VASR_Z_IN_TAIL=0 turns it off.
    Z_IN_TAIL_MIN_ROWS = 4097

    def _z_in_tail(self, B: int, L: int, D: int) -> bool:
        ssm = self.ssm
        if os.environ.get("VASR_Z_IN_TAIL", "1") == "0" or B * L < self.Z_IN_TAIL_MIN_ROWS:
            return False
        if _SCAN_MODE_ID[ssm.scan_mode] != 0:
            return False
        mods = (ssm.in_proj, ssm.x_proj, ssm.dt_proj, ssm.out_proj, self.ffn[0], self.ffn[3])
        dtype = ssm.in_proj.weight.dtype
        if dtype not in (torch.float32, torch.bfloat16) or not all(
                type(m) is nn.Linear and m.weight.dtype == dtype for m in mods):
            return False  # QAT (quantize.QuantizedLinear) and mixed-dtype models keep the gated scan
        if dtype == torch.float32 and os.environ.get("VASR_XDT_COMPOSE", "1") == "0":
            return False
        if not self._fused_tail_ok(D):
            return False
        N = ops.scan_state_dim(ssm.state_dim)
        if N != ssm.state_dim or ops._use_chunked(B, L, ssm.d_inner, N, _tree_mode()):
            return False
        return ("w_noz" if dtype == torch.float32 else "w_x") in ssm._prepared()

    def _norm_conv(self, x: torch.Tensor, pre_norm: Optional[nn.LayerNorm]):
        """(conv(norm1(x)), x) as (B, L, D) tensors; with pre_norm, x is first pre_norm(x), formed
        inside the same launch when the shape allows it (vasr_ln_dwconv_prenorm_f32: D = 192, 4
        taps), else by its own LayerNorm launch."""
        B, L, D = x.shape
        x = x.contiguous()
        cw = ops.f32(self.conv.weight).view(D, -1)
        if pre_norm is not None:
            if D == 192 and cw.shape[1] == 4:
                return ops.ln_dwconv_prenorm(x, pre_norm.weight, pre_norm.bias, pre_norm.eps, self.norm1.weight,
                                             self.norm1.bias, cw, self.conv.bias, self.norm1.eps)
            x = ops.layer_norm(x, pre_norm.weight, pre_norm.bias, pre_norm.eps)
        return ops.ln_dwconv(x, self.norm1.weight, self.norm1.bias, cw, self.conv.bias, self.norm1.eps), x

    def _forward_z_in_tail(self, x: torch.Tensor, pre_norm: Optional[nn.LayerNorm] = None) -> torch.Tensor:
        B, L, D = x.shape
        ssm = self.ssm
        Di, N = ssm.d_inner, ssm.state_dim
        p = ssm._prepared()
        u, x = self._norm_conv(x, pre_norm)
        x2 = x.view(B * L, D)
        u = u.view(B * L, D)
        if "w_noz" in p or ("w_noz16" in p and _bf16_compose()):
            w, b = (p["w_noz"], p["b_noz"]) if "w_noz" in p else (p["w_noz16"], p["b_noz16"])
            xbd = ops.gemm(u, w, b, epilogue=_lib.EPI_SOFTPLUS_FROM, n_out=Di + 2 * N)  # [x|B|C|dt]
            xs, bc, dt = xbd[:, :Di], xbd[:, Di:Di + 2 * N], xbd[:, Di + 2 * N:]
        else:
            xs = ops.gemm(u, p["w_x"])                                                 # (M, Di) x
            xdt = ops.gemm(xs, p["w_xdt"], p["b_xdt"], epilogue=_lib.EPI_SOFTPLUS_FROM, n_out=2 * N)  # [B|C|dt]
            bc, dt = xdt[:, :2 * N], xdt[:, 2 * N:]
        mode = _tree_mode()
        yd = ops.ssm_scan_ungated(xs, dt, bc, p["A2"], ssm.D, B, L, mode)
        out = ops.ssm_block_tail_gated(yd, u, p["w_z"], mode, x2, ssm.out_proj.weight, self.norm2.weight,
                                       self.norm2.bias, self.norm2.eps, self.ffn[0].weight, self.ffn[0].bias,
                                       self.ffn[3].weight, self.ffn[3].bias)
        return out.view(B, L, D)

    # The block in three stages -- head (LN1, causal dwconv, projections), the scan, tail (out_proj
    # + residual, LN2, FFN + residual).  (Issuing one utterance group's scans on a stream of their
    # own beside the other group's heads and tails measured slower than independent group
    # streams: profiles/r02_paired/.)
    def head(self, x: torch.Tensor, pre_norm: Optional[nn.LayerNorm] = None):
        """x (B, L, D) -> (x2 = x as (B*L, D) rows, xz, xdt): the scan's operands (pre_norm: forward's)."""
        _check_eval(self)
        B, L, D = x.shape
        u, x = self._norm_conv(x, pre_norm)
        x2 = x.view(B * L, D)
        xz, xdt = self.ssm.project(u.view(B * L, D))
        return x2, xz, xdt

    def tail(self, g: torch.Tensor, x2: torch.Tensor, B: int, L: int) -> torch.Tensor:
        """Gated scan output g (B*L, d_inner) and the block input rows x2 -> block output (B, L, D)."""
        D = x2.shape[1]
        if self._fused_tail_ok(D):
            # out_proj + residual -> LN2 -> FFN1 + GELU -> FFN2 + residual in one kernel:
            # x1 and the FFN intermediate stay on chip
            out = ops.ssm_block_tail(g, x2, self.ssm.out_proj.weight, self.norm2.weight, self.norm2.bias,
                                     self.norm2.eps, self.ffn[0].weight, self.ffn[0].bias, self.ffn[3].weight,
                                     self.ffn[3].bias)
            return out.view(B, L, D)
        x1 = ops.gemm(g, self.ssm.out_proj.weight, epilogue=_lib.EPI_RESIDUAL, aux=x2)
        # norm2 runs inside the FFN-in GEMM's A read (identical float operations)
        f = ops.gemm(x1, self.ffn[0].weight, self.ffn[0].bias, epilogue=_lib.EPI_GELU,
                     ln=(self.norm2.weight, self.norm2.bias, self.norm2.eps))
        out = ops.gemm(f, self.ffn[3].weight, self.ffn[3].bias, epilogue=_lib.EPI_RESIDUAL, aux=x1)
        return out.view(B, L, D)


class LocalSSMProcessor(nn.Module):
    """Stack of SSM blocks + final LayerNorm (reference ssm.py:444-505)."""

    def __init__(self, d_model: int = 192, num_layers: int = 8, state_dim: int = 64, expand_ratio: int = 2,
                 kernel_size: int = 4, dropout: float = 0.1, use_checkpoint: bool = False,
                 scan_mode: ScanMode = "parallel"):
        super().__init__()
        self.layers = nn.ModuleList([
            SSMBlock(d_model=d_model, state_dim=state_dim, expand_ratio=expand_ratio, kernel_size=kernel_size,
                     dropout=dropout, use_checkpoint=use_checkpoint, scan_mode=scan_mode)
            for _ in range(num_layers)
        ])
        self.norm = nn.LayerNorm(d_model)

    def forward(self, x: torch.Tensor, pre_norm: Optional[nn.LayerNorm] = None) -> torch.Tensor:
        """pre_norm (extension): the LayerNorm still to be applied to x, folded into the first
        block's norm1 + conv launch (SSMBlock.forward)."""
        for i, layer in enumerate(self.layers):
            x = layer(x, pre_norm) if i == 0 else layer(x)
        return ops.layer_norm(x, self.norm.weight, self.norm.bias, self.norm.eps)

    def forward_differentiable(self, x: torch.Tensor, *, tree_scan: bool = False) -> torch.Tensor:
        """The stack for training: every block's forward_differentiable(tree_scan=...), then the
        final LayerNorm as a torch op."""
        for layer in self.layers:
            x = layer.forward_differentiable(x, tree_scan=tree_scan)
        return self.norm(x)

    def forward_pair(self, x: torch.Tensor, norm2: nn.LayerNorm, pre_norm: Optional[nn.LayerNorm] = None):
        """(forward(x), norm2(forward(x))) with both LayerNorms in one launch (the global context's
        query norm right after this stack's final one, ops.layer_norm_pair): bitwise the same."""
        for i, layer in enumerate(self.layers):
            x = layer(x, pre_norm) if i == 0 else layer(x)
        return ops.layer_norm_pair(x, self.norm.weight, self.norm.bias, self.norm.eps, norm2.weight, norm2.bias,
                                   norm2.eps)


class GlobalSSM(nn.Module):
    """SSM over pooled tokens; always the default 'parallel' scan (reference ssm.py:508-556)."""

    def __init__(self, d_model: int = 192, num_layers: int = 2, state_dim: int = 32, dropout: float = 0.1):
        super().__init__()
        self.layers = nn.ModuleList([
            SSMBlock(d_model=d_model, state_dim=state_dim, expand_ratio=2, kernel_size=4, dropout=dropout)
            for _ in range(num_layers)
        ])
        self.norm = nn.LayerNorm(d_model)

    def forward(self, x: torch.Tensor, raw: bool = False) -> torch.Tensor:
        """raw (extension): the rows before the final LayerNorm (the global context applies it
        inside its second pooling launch)."""
        for layer in self.layers:
            x = layer(x)
        if raw:
            return x
        return ops.layer_norm(x, self.norm.weight, self.norm.bias, self.norm.eps)

    def forward_differentiable(self, x: torch.Tensor) -> torch.Tensor:
        """The stack for training.  Its scan is always the tree (reference ssm.py:530-537), so its
        blocks always run forward_differentiable(tree_scan=True); then the final LayerNorm."""
        for layer in self.layers:
            x = layer.forward_differentiable(x, tree_scan=True)
        return self.norm(x)
