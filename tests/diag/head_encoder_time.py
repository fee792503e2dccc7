"""diag: the head with a slate encoder (ltr_head_encoder_score) against the same model in torch fp16 eager on the same GPU:
n_features = 4096, fc = [1024] with input_norm, transformer N = 2, h = 8, d_ff = 2048, d_output = 1; one slate of n rows, fp16
hidden states.  Device events around `inner` calls on one stream, the two sides in alternating windows, median of `reps`
windows after a warm-up; nothing is asserted.    python tests/diag/head_encoder_time.py [n ...]"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle.ltr_head import seeded_head_weights  # noqa: E402
from vllm_ltr_amd.ltr_head import HipLTRHead  # noqa: E402

NF, D, H, DFF, NB = 4096, 1024, 8, 2048, 2
FC = {"sizes": [D], "input_norm": True, "activation": "ReLU"}
TR = {"N": NB, "d_ff": DFF, "h": H, "positional_encoding": None, "dropout": 0.0}
sd = seeded_head_weights(NF, FC["sizes"], True, 1, 0)
rs = np.random.RandomState(1)
for i in range(NB):
    p = f"encoder.layers.{i}."
    for name, (o, k) in {**{f"self_attn.linears.{j}": (D, D) for j in range(4)}, "feed_forward.w_1": (DFF, D),
                         "feed_forward.w_2": (D, DFF)}.items():
        sd[p + name + ".weight"] = (rs.standard_normal((o, k)) * (2.0 / (o + k)) ** 0.5).astype(np.float16)
        sd[p + name + ".bias"] = (0.05 * rs.standard_normal(o)).astype(np.float16)
for name in [f"encoder.layers.{i}.sublayer.{j}.norm" for i in range(NB) for j in range(2)] + ["encoder.norm"]:
    sd[name + ".a_2"], sd[name + ".b_2"] = np.ones(D, np.float16), np.zeros(D, np.float16)
head = HipLTRHead(NF, FC, {"d_output": 1, "output_activation": None}, sd, transformer=TR)
w = {k: torch.from_numpy(np.asarray(v, np.float32)).cuda().half() for k, v in sd.items()}


def torch_model(x):
    """the same model in fp16 eager (allRank's modules written out: transformer.py:75-97, 153-219)"""
    lin = lambda z, n: F.linear(z, w[n + ".weight"], w[n + ".bias"])
    an = lambda z, n: w[n + ".a_2"] * (z - z.mean(-1, keepdim=True)) / (z.std(-1, keepdim=True) + 1e-6) + w[n + ".b_2"]
    z = F.relu(lin(F.layer_norm(x, (NF,), w["input_layer.input_norm.weight"], w["input_layer.input_norm.bias"]),
                   "input_layer.layers.0"))
    n = z.shape[0]
    for i in range(NB):
        p = f"encoder.layers.{i}."
        y = an(z, p + "sublayer.0.norm")
        q, k, v = (lin(y, f"{p}self_attn.linears.{j}").view(n, H, -1).transpose(0, 1) for j in range(3))
        a = torch.softmax(q @ k.transpose(1, 2) / (D // H) ** 0.5, -1) @ v
        z = z + lin(a.transpose(0, 1).reshape(n, D), p + "self_attn.linears.3")
        z = z + lin(F.relu(lin(an(z, p + "sublayer.1.norm"), p + "feed_forward.w_1")), p + "feed_forward.w_2")
    return lin(an(z, "encoder.norm"), "output_layer.w_1")[:, 0]


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


print(f"{torch.cuda.get_device_name(0)}; head {NF} -> {D}, encoder N = {NB}, h = {H}, d_ff = {DFF}; one slate; "
      "us per call: median (min .. max)")
print(f"{'n':>5} {'ltr_head_encoder_score':>30} {'torch fp16 eager':>30} {'torch/ours':>10} {'max|ours - torch|':>18}")
for n in [int(a) for a in sys.argv[1:]] or [256, 2048, 8192]:
    x = torch.randn(n, NF, generator=torch.Generator().manual_seed(n)).half().cuda()
    head.reserve(n)
    sides = [lambda: head.score(x), lambda: torch_model(x)]
    inner, reps = (20 if n <= 256 else 5 if n <= 2048 else 2), 11
    for fn in sides * 3:
        fn()
    ts = [[], []]
    for _ in range(reps):
        for i, fn in enumerate(sides):
            ts[i].append(window(fn, inner))
    d = (head.score(x) - torch_model(x).float()).abs().max().item()
    fmt = lambda t: f"{sorted(t)[len(t) // 2]:10.1f} ({min(t):.1f} .. {max(t):.1f})"
    print(f"{n:>5} {fmt(ts[0]):>30} {fmt(ts[1]):>30} {sorted(ts[1])[reps // 2] / sorted(ts[0])[reps // 2]:>10.2f} {d:>18.2e}")
