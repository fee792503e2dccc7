"""diag: ltr_slate_metrics (two launches: per-slate sort network + scan, then the means) against the same formulas written out in
torch on the same GPU - masked sort, gather, gains, discounts, cumsum, max - for the metrics {"ndcg": [5, 10], "mrr": [1]} of
allRank's default validation.  Device events around `inner` calls on one stream, the two sides in alternating windows, median of
`reps` windows after a warm-up; nothing is asserted.
    python tests/diag/slate_metrics_time.py [BxS ...]          (table also written to profiles/slate_metrics_time.txt with --write)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vllm_ltr_amd import metrics  # noqa: E402

ASK = {"ndcg": [5, 10], "mrr": [1]}


def dense(y_pred, y_true, ask=ASK, pad=-1.0, filler=1.0):
    """The definition of include/ltr_hip.h in torch ops; returns the means as a device tensor in the order of `ask`."""
    B, S = y_pred.shape
    mask = y_true == pad
    label = y_true.masked_fill(mask, 0.0)
    order = y_pred.masked_fill(mask, float("-inf")).argsort(dim=-1, descending=True, stable=True)
    by_score = label.gather(1, order)
    disc = 1.0 / torch.log2(torch.arange(2, S + 2, device=y_pred.device, dtype=torch.float32))
    out = []
    if "ndcg" in ask:
        at = torch.tensor([min(a, S) - 1 for a in ask["ndcg"]], device=y_pred.device)
        dcg = ((2.0 ** by_score - 1.0) * disc).cumsum(1)[:, at]
        idcg = ((2.0 ** label.sort(-1, descending=True).values - 1.0) * disc).cumsum(1)[:, at]
        out.append(torch.where(idcg == 0, torch.full_like(dcg, filler), dcg / idcg).mean(0))
    if "mrr" in ask:
        v, p = by_score.max(dim=1)
        at = torch.tensor(ask["mrr"], device=y_pred.device, dtype=torch.float32)
        rr = (1.0 / (p.float() + 1.0))[:, None] * (p.float()[:, None] < at[None, :])
        out.append((rr * (v.sum() != 0)).mean(0))
    return torch.cat(out)


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def main():
    args = [a for a in sys.argv[1:] if a != "--write"]
    shapes = [tuple(int(v) for v in a.split("x")) for a in args] or [(4096, 64), (1024, 256), (64, 4096)]
    lines = [f"{torch.cuda.get_device_name(0)}; means of {ASK}, labels 0 .. 4 with 15 % padded; us per call: median (min .. max)",
             f"{'B x S':>11} {'ltr_slate_metrics':>28} {'torch sort / gather / cumsum':>30} {'torch/ours':>10} {'max|d| of the means':>20}"]
    print("\n".join(lines))
    for B, S in shapes:
        g = torch.Generator().manual_seed(S)
        yp = (3.0 * torch.randn(B, S, generator=g)).cuda()
        yt = torch.randint(0, 5, (B, S), generator=g).float()
        yt[torch.rand(B, S, generator=g) < 0.15] = -1.0
        yt = yt.cuda()
        ws = torch.empty(metrics.slate_workspace_bytes(B, S), dtype=torch.uint8, device="cuda")
        ours = lambda: torch.stack(list(metrics.slate_metrics_device(yp, yt, ASK, workspace=ws).values()))
        sides = [ours, lambda: dense(yp, yt)]
        inner, reps = 200, 11
        for fn in sides * 3:
            fn()
        ts = [[], []]
        for _ in range(reps):
            for i, fn in enumerate(sides):
                ts[i].append(window(fn, inner))
        d = (sides[0]() - sides[1]()).abs().max().item()
        fmt = lambda t: f"{sorted(t)[len(t) // 2]:10.1f} ({min(t):.1f} .. {max(t):.1f})"
        lines.append(f"{f'{B} x {S}':>11} {fmt(ts[0]):>28} {fmt(ts[1]):>30} "
                     f"{sorted(ts[1])[reps // 2] / sorted(ts[0])[reps // 2]:>10.2f} {d:>20.2e}")
        print(lines[-1])
    if "--write" in sys.argv:
        out = os.environ.get("SLATE_METRICS_TIME_OUT") or os.path.join(ROOT, "profiles", "slate_metrics_time.txt")
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
