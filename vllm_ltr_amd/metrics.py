"""Order agreement of two score vectors on the device (``ltr_order_agreement`` of libltr_hip.so): Kendall's tau-b, the pair
counts behind it and the score gaps of the discordant pairs.

The reference's training metric is ``scipy.stats.kendalltau(labels, predictions)`` (``train/trainer.py:195``), and the parity
reports of this project compare two queue orders (``benchmarks/benchmark_throughput_original.py:396-443``) by their discordant
pairs.  Both are one pass over all ``n (n - 1) / 2`` pairs; the scores are already on the GPU, so the pass runs there:

    r = order_agreement(labels, predictions)      # OrderAgreement: six exact int64 counts, gaps, tau_b
    tau = kendall_tau(labels, predictions)        # == scipy.stats.kendalltau(labels, predictions)[0]

``order_agreement_device`` is the same call without the read-back (no host synchronisation: usable inside a captured graph);
``OrderAgreement.from_bytes`` decodes what it wrote.  The p-value of ``kendalltau`` and tau-c are not computed.

Slate metrics (``ltr_slate_metrics``): what allRank's loop computes at the end of every epoch
(``train/allrank/training/train_utils.py:48-72``: ``compute_metrics`` -> ``metric_on_epoch``) with ``ndcg``, ``dcg`` and ``mrr`` of
``train/allrank/models/metrics.py:65-171``, and what its scheduler and early stopping read (``config.val_metric``, e.g. ``ndcg_5``):

    per_slate = ndcg(y_pred, y_true, ats=[5, 10])                               # f32 [B, 2] on the device; dcg, mrr alike
    m = slate_metrics(y_pred, y_true, {"ndcg": [5, 10], "mrr": [1]})            # {"ndcg_5": .., "ndcg_10": .., "mrr_1": ..}

``y_pred``, ``y_true``: f32 ``[B, S]`` device tensors, S <= 4096; an item whose label is ``padding_indicator`` scores -inf and
has label 0.  Items are ranked by descending score, equal scores by ascending index (``torch.sort`` leaves ties open).  ``gain`` is
``"pow2"`` (2^label - 1, allRank's default) or ``"identity"``; allRank's callable ``gain_function`` is not built.  One quirk of
the reference is kept: ``mrr`` is 0 for the whole call when the largest labels of all its slates add up to 0, so a slate
without a relevant item inside a batch that has some gets ``mrr`` = 1 (``metrics.py:157-167``: the first maximum of an all-zero
row is position 0, and the mask is one scalar for the batch).  The definition is in ``include/ltr_hip.h``; the sums run in f64 in
a fixed order, so two calls give the same bits.  ``slate_metrics_device`` is ``slate_metrics`` without the read-back."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, Optional

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


# ---- slate metrics ------------------------------------------------------------------------------------------------------------
MAX_SLATE, MAX_SLATES, MAX_ATS = 4096, 1 << 20, 8          # ltr_slate_metrics' limits
SLATE_METRICS = ("ndcg", "dcg", "mrr")                      # the row order of mean_out


def _slate_call(y_pred: torch.Tensor, y_true: torch.Tensor, ats, gain: str, padding_indicator: float, filler_value: float,
                want: tuple, workspace: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """One ``ltr_slate_metrics`` call; ``want``: which of "ndcg", "dcg", "mrr" ([B, len(ats)]) and "mean" ([3, len(ats)]) to write."""
    if gain not in _lib.SLATE_GAINS:
        raise ValueError(f"slate metrics: gain {gain!r} (one of {sorted(_lib.SLATE_GAINS)}; a callable gain_function is not built)")
    for name, t in (("y_pred", y_pred), ("y_true", y_true)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"slate metrics: {name} must be a torch tensor, not {type(t).__name__}")
        if not t.is_cuda:
            raise _lib.LtrError("slate metrics need device tensors (no CPU fallback on the product path)")
        if t.dtype != torch.float32 or t.dim() != 2:
            raise ValueError(f"slate metrics: {name} must be a [B, S] float32 tensor, not {t.dtype} {tuple(t.shape)}")
    if y_pred.shape != y_true.shape or y_pred.device != y_true.device:
        raise ValueError(f"slate metrics: y_pred {tuple(y_pred.shape)} on {y_pred.device}, y_true {tuple(y_true.shape)} on {y_true.device}")
    B, S = y_pred.shape
    if not (1 <= S <= MAX_SLATE and 1 <= B <= MAX_SLATES):
        raise ValueError(f"slate metrics: [{B}, {S}] slates (1 <= S <= {MAX_SLATE}, 1 <= B <= {MAX_SLATES})")
    ats = [S] if ats is None else [int(a) for a in ats]
    if not 1 <= len(ats) <= MAX_ATS or min(ats) < 1:
        raise ValueError(f"slate metrics: ats {ats} (1 to {MAX_ATS} cut-offs, each at least 1)")
    cfg = _lib.SlateMetricsConfig(len(ats), (C.c_int32 * 8)(*ats), _lib.SLATE_GAINS[gain], float(padding_indicator), float(filler_value))
    lib, dev = _lib.load(), y_pred.device
    y_pred, y_true = y_pred.contiguous(), y_true.contiguous()
    out = {k: torch.empty((3 if k == "mean" else B, len(ats)), dtype=torch.float32, device=dev) for k in want}
    need = int(lib.ltr_slate_metrics_workspace_bytes(B, S))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif workspace.device != dev or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise ValueError(f"slate metrics: workspace must be a contiguous uint8 tensor on {dev}")
    ptr = lambda k: out[k].data_ptr() if k in out else None
    with torch.cuda.device(dev):
        _lib.check(lib.ltr_slate_metrics(y_pred.data_ptr(), y_true.data_ptr(), B, S, C.byref(cfg), ptr("ndcg"), ptr("dcg"), ptr("mrr"),
                                         ptr("mean"), workspace.data_ptr(), workspace.numel(),
                                         torch.cuda.current_stream().cuda_stream), "ltr_slate_metrics")
    return out


def slate_workspace_bytes(B: int, S: int) -> int:
    return int(_lib.load().ltr_slate_metrics_workspace_bytes(int(B), int(S)))


def ndcg(y_pred: torch.Tensor, y_true: torch.Tensor, ats=None, gain: str = "pow2", padding_indicator: float = -1,
         filler_value: float = 1.0) -> torch.Tensor:
    """NDCG at the cut-offs ``ats`` (None: the slate length), f32 [B, len(ats)] on the device (``metrics.py:65-86``);
    ``filler_value`` where a slate's ideal DCG is 0."""
    return _slate_call(y_pred, y_true, ats, gain, padding_indicator, filler_value, ("ndcg",))["ndcg"]


def dcg(y_pred: torch.Tensor, y_true: torch.Tensor, ats=None, gain: str = "pow2", padding_indicator: float = -1) -> torch.Tensor:
    """DCG at the cut-offs ``ats``, f32 [B, len(ats)] on the device (``metrics.py:99-135``)."""
    return _slate_call(y_pred, y_true, ats, gain, padding_indicator, 1.0, ("dcg",))["dcg"]


def mrr(y_pred: torch.Tensor, y_true: torch.Tensor, ats=None, padding_indicator: float = -1) -> torch.Tensor:
    """MRR at the cut-offs ``ats``, f32 [B, len(ats)] on the device (``metrics.py:138-171``), with the reference's batch-wide
    rule: all 0 when no slate of the call has a positive label, and 1 for a slate without one when another slate has."""
    return _slate_call(y_pred, y_true, ats, "pow2", padding_indicator, 1.0, ("mrr",))["mrr"]


def slate_metrics_device(y_pred: torch.Tensor, y_true: torch.Tensor, metrics: Dict[str, list], gain: str = "pow2",
                         padding_indicator: float = -1, filler_value: float = 1.0,
                         workspace: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """``slate_metrics`` without the read-back: the values are 0-dim views of the one ``mean_out`` the call wrote (no host
    synchronisation: usable inside a captured graph when ``workspace`` is given)."""
    for name in metrics:
        if name not in SLATE_METRICS:
            raise ValueError(f"slate metrics: metric {name!r} (one of {list(SLATE_METRICS)})")
    S = y_pred.shape[-1] if isinstance(y_pred, torch.Tensor) else 0
    asked = {name: [S if a is None else int(a) for a in (ats if ats is not None else [None])] for name, ats in metrics.items()}
    ats = sorted({a for v in asked.values() for a in v})
    mean = _slate_call(y_pred, y_true, ats, gain, padding_indicator, filler_value, ("mean",), workspace)["mean"]
    return {f"{name}_{a}": mean[SLATE_METRICS.index(name), ats.index(a)] for name, v in asked.items() for a in v}


def slate_metrics(y_pred: torch.Tensor, y_true: torch.Tensor, metrics: Dict[str, list], gain: str = "pow2",
                  padding_indicator: float = -1, filler_value: float = 1.0) -> Dict[str, float]:
    """``compute_metrics`` of one batch (``train_utils.py:48-72``): ``{"ndcg": [5, 10], "mrr": [1]}`` ->
    ``{"ndcg_5": .., "ndcg_10": .., "mrr_1": ..}``, each the mean over the B slates; all from one device call."""
    dev = slate_metrics_device(y_pred, y_true, metrics, gain, padding_indicator, filler_value)
    if not dev:
        return {}
    host = torch.stack(list(dev.values())).cpu().tolist()
    return dict(zip(dev.keys(), host))
