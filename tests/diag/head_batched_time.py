"""diag: the hidden-state head's row kernel (ltr_head_score) against the batched MFMA path (ltr_head_score_batched), fed f32
and fp16, on n_features = 4096, fc = [1024], d_output = 1, input_norm on.  Device events around `inner` calls on one stream,
median of `reps` windows after a warm-up; nothing is asserted.    python tests/diag/head_batched_time.py [N ...]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle.ltr_head import seeded_head_weights  # noqa: E402
from vllm_ltr_amd.ltr_head import HipLTRHead  # noqa: E402

NF, FC = 4096, {"sizes": [1024], "input_norm": True, "activation": "ReLU"}
head = HipLTRHead(NF, FC, {"d_output": 1, "output_activation": None}, seeded_head_weights(NF, FC["sizes"], True, 1, 0))
w_bytes = 2 * (NF * 1024 + 1024)


def timed(fn, inner, reps=15):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / inner)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


print(f"{torch.cuda.get_device_name(0)}; head {NF} -> 1024 -> 1, fp16 weights {w_bytes / 1e6:.1f} MB; us per call: median (min .. max)")
print(f"{'N':>5} {'row kernel f32':>26} {'batched f32':>26} {'batched fp16':>26} {'row/batched':>11} {'max|row - batched|':>18}")
for n in [int(a) for a in sys.argv[1:]] or [1, 16, 256, 2048]:
    x = torch.randn(n, NF, generator=torch.Generator().manual_seed(n)).half().float().cuda()
    xh = x.half()
    head.reserve(n)
    inner = 20 if n <= 256 else 5
    row = timed(lambda: head.score(x), inner)
    b32 = timed(lambda: head.score(x, batched=True), inner)
    b16 = timed(lambda: head.score(xh), inner)
    d = (head.score(x) - head.score(x, batched=True)).abs().max().item()
    same = torch.equal(head.score(x, batched=True), head.score(xh))
    fmt = lambda t: f"{t[0]:9.1f} ({t[1]:.1f} .. {t[2]:.1f})"
    print(f"{n:>5} {fmt(row):>26} {fmt(b32):>26} {fmt(b16):>26} {row[0] / b32[0]:>11.2f} {d:>18.2e}   f32 == fp16 input: {same}")
