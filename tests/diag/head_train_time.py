"""diag: one training step of the hidden-state head on the device (HipLTRHeadTrainer.step: forward, listMLE, backward on the
matrix cores, clip-free Adam) next to what a user has today - the same head in torch-ROCm f32 with autograd and
torch.optim.Adam, fed the dLoss/dscore of the same listMLE kernel - on n_features = 4096, fc = [1024], d_output = 1,
input_norm on.  The two are timed in alternating windows: device events around `inner` steps on one stream, median of
`reps` windows after a warm-up; nothing is asserted.    python tests/diag/head_train_time.py [B*S ...]"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle.ltr_head import seeded_head_weights  # noqa: E402
from vllm_ltr_amd import train_loss  # noqa: E402
from vllm_ltr_amd.ltr_head_trainer import HipLTRHeadTrainer  # noqa: E402

NF, FC, POST = 4096, {"sizes": [1024], "input_norm": True, "activation": "ReLU"}, {"d_output": 1, "output_activation": None}
S = 256                                  # slate length; B = rows / S
sd = seeded_head_weights(NF, FC["sizes"], True, 1, 0)
LR = 1e-4


def torch_head():
    p = {k: torch.tensor(v.astype("float32"), device="cuda", requires_grad=True) for k, v in sd.items()}
    opt = torch.optim.Adam(p.values(), lr=LR)

    def step(x, y, sh):
        opt.zero_grad(set_to_none=True)
        h = F.layer_norm(x, (NF,), p["input_layer.input_norm.weight"], p["input_layer.input_norm.bias"], 1e-5)
        h = F.relu(F.linear(h, p["input_layer.layers.0.weight"], p["input_layer.layers.0.bias"]))
        s = F.linear(h, p["output_layer.w_1.weight"], p["output_layer.w_1.bias"]).view(y.shape)
        _, g = train_loss.listmle(s, y, sh)
        s.backward(g)
        opt.step()
    return step


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def med(ts):
    ts = sorted(ts)
    return f"{ts[len(ts) // 2]:9.1f} ({ts[0]:.1f} .. {ts[-1]:.1f})", ts[len(ts) // 2]


print(f"{torch.cuda.get_device_name(0)}; head {NF} -> 1024 -> 1 with input_norm, listMLE on slates of {S}; us per step: median (min .. max)")
print(f"{'B*S':>6} {'device step':>30} {'torch f32 autograd + Adam':>30} {'torch/device':>12}")
for rows in [int(a) for a in sys.argv[1:]] or [256, 2048, 8192]:
    B = rows // S
    x = torch.randn(rows, NF, generator=torch.Generator().manual_seed(rows)).half().float().cuda()
    y = torch.randint(0, 5, (B, S), generator=torch.Generator().manual_seed(1)).float().cuda()
    sh = torch.randperm(S, generator=torch.Generator().manual_seed(2)).cuda()
    tr = HipLTRHeadTrainer(NF, FC, POST, sd, lr=LR)
    ref = torch_head()
    ours, theirs = (lambda: tr.step(x, y, shuffle=sh)), (lambda: ref(x, y, sh))
    inner = 10 if rows <= 2048 else 4
    for _ in range(3):
        ours(); theirs()
    to, tt = [], []
    for _ in range(11):                  # alternating windows
        to.append(window(ours, inner)); tt.append(window(theirs, inner))
    (so, mo), (st, mt) = med(to), med(tt)
    print(f"{rows:>6} {so:>30} {st:>30} {mt / mo:>12.2f}")
