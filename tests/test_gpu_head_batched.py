"""Batched MFMA path of the hidden-state head (ltr_head_score_batched) against OracleLTRHead in f64."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle.ltr_head import OracleLTRHead, seeded_head_weights
from util import GOLDEN

pytestmark = pytest.mark.gpu
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
HEADS = {"a": (96, {"sizes": [40], "input_norm": True, "activation": "ReLU"}, {"d_output": 1, "output_activation": None}),
         "b": (256, {"sizes": [128, 64], "input_norm": False, "activation": "Tanh"}, {"d_output": 3, "output_activation": None}),
         "c": (100, None, {"d_output": 1, "output_activation": None})}


@functools.lru_cache(None)
def _heads(name, mode="f16"):
    from vllm_ltr_amd.ltr_head import HipLTRHead
    nf, fc, post = HEADS[name]
    sd = seeded_head_weights(nf, fc["sizes"] if fc else None, bool(fc and fc["input_norm"]), post["d_output"], 11)
    return HipLTRHead(nf, fc, post, sd, "cuda:0", mode), OracleLTRHead(nf, fc, post, sd, dtype=torch.float64)


def _rows(n, nf, dtype, seed):
    """fp16-rounded values (exact in every dtype used), on the device in `dtype`."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, nf, generator=g).half().to(dtype).cuda()


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("n", [1, 17, 130])
@pytest.mark.parametrize("name", list(HEADS))
def test_parity(name, n, dt, residual):
    head, oracle = _heads(name)
    x = _rows(n, HEADS[name][0], DTYPES[dt], 1)
    r = _rows(n, HEADS[name][0], DTYPES[dt], 2) if residual else None
    want = oracle.score((x + r if residual else x).float().cpu().numpy())     # the sum rounded once to the input dtype
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(torch.int32)
    idx[-1] = idx[0]                                                          # out of order, one row twice
    got = head.score(x, None, r, batched=True).cpu().numpy()
    got_i = head.score(x, idx.cuda(), r, batched=True).cpu().numpy()
    err = max(np.abs(got - want).max(), np.abs(got_i - want[idx.numpy()]).max())
    print(f"head_batched {name} n={n} {dt} residual={residual}: max|d| = {err:.2e}")
    assert err <= 1e-4


@pytest.mark.parametrize("name", ["small_relu", "wide_tanh_sum", "no_fc", "gelu_nonorm"])
def test_golden_cases(name):
    from vllm_ltr_amd.ltr_head import HipLTRHead
    z = np.load(os.path.join(GOLDEN, f"ltr_head_{name}.npz"))
    cfg = json.loads(str(z["cfg"]))
    nf, fc, post = int(z["n_features"]), cfg["fc_model"], cfg["post_model"]
    sd = seeded_head_weights(nf, fc["sizes"] if fc else None, bool(fc and fc["input_norm"]), post["d_output"], int(z["seed"]))
    got = HipLTRHead(nf, fc, post, sd).score(torch.from_numpy(z["x"]).cuda(), batched=True).cpu().numpy()
    err = np.abs(got - z["score"]).max()
    print(f"head_batched golden {name}: max|d| = {err:.2e}")
    assert err <= 1e-4


def test_score_does_not_depend_on_the_batch():
    head, _ = _heads("a")
    x = _rows(130, 96, torch.float16, 4)
    full = head.score(x)
    assert torch.equal(head.score(x), full)
    for r in (0, 15, 16, 63, 64, 129):
        assert torch.equal(head.score(x[r:r + 1].contiguous()), full[r:r + 1]), r
    perm = torch.randperm(130, generator=torch.Generator().manual_seed(5)).to(torch.int32).cuda()
    assert torch.equal(head.score(x, perm), full[perm.long()])
    assert torch.equal(head.score(x, perm.long()), full[perm.long()])          # int64 indices, as the backbone has them


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_beyond_fp16_range(dt):
    head, oracle = _heads("c")
    x = _rows(33, 100, DTYPES[dt], 6)
    x[torch.arange(33), torch.arange(33) * 3] = 3e5
    wide = x.float()
    want = oracle.score(wide.cpu().numpy()).astype(np.float64)
    err_new = np.abs(head.score(x, batched=True).cpu().numpy() - want)
    err_row = np.abs(head.score(wide).cpu().numpy() - want)              # the row kernel: the yardstick
    w = oracle.w["output_layer.w_1.weight"][0].numpy()
    bound = np.maximum(4 * err_row, 2.0 ** -21 * (np.abs(wide.cpu().numpy().astype(np.float64)) * np.abs(w)).sum(1))
    print(f"head_batched range {dt}: batched max|d| = {err_new.max():.3e}, row kernel max|d| = {err_row.max():.3e}, "
          f"smallest bound = {bound.min():.3e}, worst err/bound = {(err_new / bound).max():.3f}")
    assert (err_new <= bound).all()


def test_graph_capture():
    from vllm_ltr_amd import _lib
    from vllm_ltr_amd.ltr_head import HipLTRHead
    head, _ = _heads("a")
    head.reserve(130)
    xs = _rows(130, 96, torch.float16, 7)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = head.score(xs)
    for seed in (8, 9):
        new = _rows(130, 96, torch.float16, seed)
        xs.copy_(new)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, head.score(new)), seed
    nf, fc, post = HEADS["a"]
    fresh = HipLTRHead(nf, fc, post, seeded_head_weights(nf, fc["sizes"], True, 1, 11))      # nothing reserved
    with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
        keep = xs + 0
        with pytest.raises(_lib.LtrError, match="reserve"):
            fresh.score(xs)


def test_argument_errors():
    from vllm_ltr_amd import _lib
    head, _ = _heads("a")
    lib = head.lib
    x = _rows(17, 96, torch.float16, 10)
    with pytest.raises(_lib.LtrError) as e:
        _heads("a", "f32")[0].score(x.float(), batched=True)
    assert e.value.code == _lib.LTR_E_INVAL and b"row path" in lib.ltr_last_error()
    need = lib.ltr_head_workspace_bytes(head._h, 17)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty(17, dtype=torch.float32, device="cuda")
    call = lambda dtype, nbytes: lib.ltr_head_score_batched(head._h, x.data_ptr(), None, dtype, None, 17, out.data_ptr(),
                                                            ws.data_ptr(), nbytes, None)
    assert call(_lib.LTR_HID_F16, need - 1) == _lib.LTR_E_NOMEM and b"workspace" in lib.ltr_last_error()
    assert call(7, need) == _lib.LTR_E_INVAL and b"hidden_dtype" in lib.ltr_last_error()
    assert call(_lib.LTR_HID_F16, need) == 0
    with pytest.raises(ValueError):
        head.score(x, batched=False)
