"""diag: ltr_lambdaloss (loss and gradient, three launches, no [B, S, S] memory) against the dense formulation in torch on the same
GPU - sort, gather, [B, S, S] score / label / gain differences, masks, weights, log2 of the clamped sigmoid powers, autograd for
the gradient - for the schemes none and ndcgLoss2PP_scheme.  Device events around `inner` calls on one stream, the two sides in
alternating windows, median of `reps` windows after a warm-up; nothing is asserted.
    python tests/diag/lambdaloss_time.py [BxS ...]          (table also written to profiles/lambdaloss_time.txt with --write)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vllm_ltr_amd import train_loss  # noqa: E402


def dense(y_pred, y_true, scheme, mu=10.0, eps=1e-10):
    """The definition of include/ltr_hip.h on [B, S, S] tensors; returns (loss, dloss / dy_pred)."""
    s = y_pred.detach().clone().requires_grad_(True)
    B, S = s.shape
    valid = y_true != -1
    order = torch.where(valid, s, torch.full_like(s, float("-inf"))).argsort(dim=-1, descending=True, stable=True)
    ss, ll, vv = s.gather(1, order), y_true.gather(1, order).clamp(min=0), valid.gather(1, order)
    inv_d = 1.0 / torch.log2(torch.arange(2, S + 2, device=s.device, dtype=torch.float32))
    ideal = torch.where(valid, y_true, torch.zeros_like(y_true)).sort(-1, descending=True).values
    gain = (2.0 ** ll - 1) / ((2.0 ** ideal - 1) * inv_d).sum(-1, keepdim=True).clamp(min=eps)
    sel = vv[:, :, None] & vv[:, None, :] & (ll[:, :, None] > ll[:, None, :])
    w = 1.0
    if scheme == "ndcgLoss2PP_scheme":
        pos = torch.arange(S, device=s.device)
        d = (pos[:, None] - pos[None, :]).abs()
        step = torch.where(d > 0, (inv_d[(d - 1).clamp(min=0)] - inv_d[d]).abs(), torch.zeros((), device=s.device))
        dg = (gain[:, :, None] - gain[:, None, :]).abs()
        w = mu * step[None] * dg + (inv_d[:, None] - inv_d[None, :]).abs()[None] * dg
    x = (ss[:, :, None] - ss[:, None, :]).clamp(-1e8, 1e8)
    loss = -torch.log2((torch.sigmoid(x).clamp(min=eps) ** w).clamp(min=eps))[sel].sum()
    loss.backward()
    return loss.detach(), s.grad


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
    shapes = [tuple(int(v) for v in a.split("x")) for a in args] or [(8, 256), (8, 1024), (2, 4096)]
    lines = [f"{torch.cuda.get_device_name(0)}; loss + gradient, labels 0 .. 4 with 10 % padded; us per call: median (min .. max)",
             f"{'B x S':>9} {'scheme':>20} {'ltr_lambdaloss':>28} {'torch dense [B, S, S]':>30} {'torch/ours':>10} {'loss rel. d':>12} {'grad max|d|/max|g|':>19}"]
    print("\n".join(lines))
    for B, S in shapes:
        g = torch.Generator().manual_seed(S)
        yp = (3.0 * torch.randn(B, S, generator=g)).cuda()
        yt = torch.randint(0, 5, (B, S), generator=g).float()
        yt[torch.rand(B, S, generator=g) < 0.1] = -1.0
        yt = yt.cuda()
        for scheme in (None, "ndcgLoss2PP_scheme"):
            sides = [lambda: train_loss.lambdaloss(yp, yt, scheme), lambda: dense(yp, yt, scheme)]
            inner, reps = (20 if S <= 1024 else 5), 11
            for fn in sides * 3:
                fn()
            ts = [[], []]
            for _ in range(reps):
                for i, fn in enumerate(sides):
                    ts[i].append(window(fn, inner))
            (l0, g0), (l1, g1) = sides[0](), sides[1]()
            dl = ((l0 - l1).abs() / l1.abs().clamp(min=1)).item()
            dg = ((g0 - g1).abs().max() / g1.abs().max()).item()
            fmt = lambda t: f"{sorted(t)[len(t) // 2]:10.1f} ({min(t):.1f} .. {max(t):.1f})"
            lines.append(f"{f'{B} x {S}':>9} {str(scheme):>20} {fmt(ts[0]):>28} {fmt(ts[1]):>30} "
                         f"{sorted(ts[1])[reps // 2] / sorted(ts[0])[reps // 2]:>10.2f} {dl:>12.2e} {dg:>19.2e}")
            print(lines[-1])
    if "--write" in sys.argv:
        out = os.environ.get("LAMBDALOSS_TIME_OUT") or os.path.join(ROOT, "profiles", "lambdaloss_time.txt")
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
