"""Order agreement of two score vectors on the device (``ltr_order_agreement`` of libltr_hip.so): Kendall's tau-b, the pair
counts behind it and the score gaps of the discordant pairs.

The reference's training metric is ``scipy.stats.kendalltau(labels, predictions)`` (``train/trainer.py:195``), and the parity
reports of this project compare two queue orders (``benchmarks/benchmark_throughput_original.py:396-443``) by their discordant
pairs.  Both are one pass over all ``n (n - 1) / 2`` pairs; the scores are already on the GPU, so the pass runs there:

    r = order_agreement(labels, predictions)      # OrderAgreement: six exact int64 counts, gaps, tau_b
    tau = kendall_tau(labels, predictions)        # == scipy.stats.kendalltau(labels, predictions)[0]

``order_agreement_device`` is the same call without the read-back (no host synchronisation: usable inside a captured graph);
``OrderAgreement.from_bytes`` decodes what it wrote.  The p-value of ``kendalltau`` and tau-c are not computed."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib

MAX_N = 1 << 20                        # ltr_order_agreement's limit
RESULT_BYTES = C.sizeof(_lib.OrderAgreementResult)


@dataclass(frozen=True)
class OrderAgreement:
    """Every pair i < j counted once, by sx = sign(x_i - x_j) and sy = sign(y_i - y_j) (IEEE f32 comparison)."""
    concordant: int        # sx * sy > 0
    discordant: int        # sx * sy < 0
    tie_x: int             # sx == 0, sy != 0
    tie_y: int             # sx != 0, sy == 0
    tie_xy: int            # both 0
    unordered: int         # a NaN among the four values
    max_gap_x: float       # max |x_i - x_j| over the discordant pairs (f32); 0 without one
    max_gap_y: float
    gap_i: int             # the smallest (i, j) that attains max_gap_x; (-1, -1) without a discordant pair
    gap_j: int
    pairs: int             # n (n - 1) / 2 = the sum of the six counts
    tau_b: float           # scipy's formula; nan if a pair is unordered or x or y is constant

    @staticmethod
    def from_bytes(raw: bytes) -> "OrderAgreement":
        r = _lib.OrderAgreementResult.from_buffer_copy(raw)
        counts = [int(getattr(r, k)) for k in ("concordant", "discordant", "tie_x", "tie_y", "tie_xy", "unordered")]
        con, dis, tx, ty, txy, un = counts
        pairs = sum(counts)
        dx, dy = pairs - tx - txy, pairs - ty - txy              # pairs not tied in x / in y (scipy: tot - xtie, tot - ytie)
        if un or dx <= 0 or dy <= 0:
            tau = float("nan")
        else:
            tau = min(1.0, max(-1.0, (con - dis) / math.sqrt(dx) / math.sqrt(dy)))
        return OrderAgreement(*counts, float(r.max_gap_x), float(r.max_gap_y), int(r.gap_i), int(r.gap_j), pairs, tau)


def _check(x: torch.Tensor, y: torch.Tensor) -> int:
    for name, t in (("x", x), ("y", y)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"order_agreement: {name} must be a torch tensor, not {type(t).__name__}")
        if not t.is_cuda:
            raise _lib.LtrError("order_agreement needs device tensors (no CPU fallback on the product path)")
        if t.dtype != torch.float32 or t.dim() != 1:
            raise ValueError(f"order_agreement: {name} must be a 1-D float32 tensor, not {t.dtype} {tuple(t.shape)}")
    if x.shape != y.shape:
        raise ValueError(f"order_agreement: x has {x.numel()} elements, y {y.numel()}")
    if x.device != y.device:
        raise ValueError(f"order_agreement: x is on {x.device}, y on {y.device}")
    if x.numel() > MAX_N:
        raise ValueError(f"order_agreement: {x.numel()} elements, at most {MAX_N}")
    return int(x.numel())


def workspace_bytes(n: int) -> int:
    return int(_lib.load().ltr_order_agreement_workspace_bytes(int(n)))


def order_agreement_device(x: torch.Tensor, y: torch.Tensor, out: Optional[torch.Tensor] = None,
                           workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Enqueues the count on the current stream of ``x``'s device and returns the uint8 [64] device tensor the result is written
    to (``out`` if given).  ``workspace``: uint8 device tensor of at least ``workspace_bytes(n)`` bytes (allocated when None)."""
    n = _check(x, y)
    lib = _lib.load()
    dev = x.device
    x, y = x.contiguous(), y.contiguous()
    if out is None:
        out = torch.empty(RESULT_BYTES, dtype=torch.uint8, device=dev)
    elif out.device != dev or out.dtype != torch.uint8 or out.numel() < RESULT_BYTES or not out.is_contiguous():
        raise ValueError(f"order_agreement: out must be a contiguous uint8 tensor of {RESULT_BYTES} bytes on {dev}")
    need = workspace_bytes(n)
    if workspace is None:
        workspace = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    elif workspace.device != dev or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise ValueError(f"order_agreement: workspace must be a contiguous uint8 tensor on {dev}")
    with torch.cuda.device(dev):
        _lib.check(lib.ltr_order_agreement(x.data_ptr(), y.data_ptr(), n, out.data_ptr(), workspace.data_ptr(),
                                           workspace.numel(), torch.cuda.current_stream().cuda_stream), "ltr_order_agreement")
    return out


def order_agreement(x: torch.Tensor, y: torch.Tensor) -> OrderAgreement:
    """x, y: 1-D float32 tensors of one length on one ROCm device."""
    return OrderAgreement.from_bytes(bytes(order_agreement_device(x, y)[:RESULT_BYTES].cpu().numpy()))


def kendall_tau(x: torch.Tensor, y: torch.Tensor) -> float:
    """Kendall's tau-b of x and y: ``scipy.stats.kendalltau(x, y)[0]`` (trainer.py:195)."""
    return order_agreement(x, y).tau_b
