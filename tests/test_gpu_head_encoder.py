"""Slate encoder of the hidden-state head (ltr_head_encoder_score) against a float64 torch twin of allRank's
FCModel -> Encoder -> OutputLayer (train/allrank/models/transformer.py, model.py), slate by slate without padding, on the
same fp16-rounded weights and input rows.  Measured max|d| over the parity cases: see DESIGN.md 4.4."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.ltr_head import seeded_head_weights

pytestmark = pytest.mark.gpu
POST = {"d_output": 1, "output_activation": None}
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
LAYOUTS = [[1], [63], [64], [65], [130], [5, 0, 64, 1, 67]]


def _fc(d_model, norm=False):
    return {"sizes": [d_model], "input_norm": norm, "activation": "ReLU"}


def _weights(nf, fc, tr, seed=11):
    sd = seeded_head_weights(nf, fc["sizes"] if fc else None, bool(fc and fc["input_norm"]), POST["d_output"], seed)
    d, dff, rs = (fc["sizes"][-1] if fc else nf), tr["d_ff"], np.random.RandomState(seed + 1)
    lin = lambda o, i: (rs.standard_normal((o, i)) * (2.0 / (o + i)) ** 0.5, 0.05 * rs.standard_normal(o))
    vec = lambda: (1.0 + 0.1 * rs.standard_normal(d), 0.05 * rs.standard_normal(d))
    for i in range(tr["N"]):
        p = f"encoder.layers.{i}."
        named = {f"self_attn.linears.{j}": lin(d, d) for j in range(4)}
        named.update({"feed_forward.w_1": lin(dff, d), "feed_forward.w_2": lin(d, dff)})
        for k, (w, b) in named.items():
            sd[p + k + ".weight"], sd[p + k + ".bias"] = w, b
        for j in range(2):
            sd[p + f"sublayer.{j}.norm.a_2"], sd[p + f"sublayer.{j}.norm.b_2"] = vec()
    sd["encoder.norm.a_2"], sd["encoder.norm.b_2"] = vec()
    return {k: np.asarray(v).astype(np.float32).astype(np.float16) for k, v in sd.items()}


@functools.lru_cache(None)
def _model(nf, d_model, h, n_blocks, norm=False, mode="f16"):
    """(HipLTRHead, f64 weights, fc, transformer); d_model None: fc_model = None and d_model = nf"""
    from vllm_ltr_amd.ltr_head import HipLTRHead
    fc = _fc(d_model, norm) if d_model else None
    tr = {"N": n_blocks, "d_ff": 72, "h": h, "positional_encoding": None, "dropout": 0.1}
    sd = _weights(nf, fc, tr)
    w = {k: torch.from_numpy(v.astype(np.float64)) for k, v in sd.items()}
    return HipLTRHead(nf, fc, POST, sd, "cuda:0", mode, transformer=tr), w, fc, tr


def _twin(w, fc, tr, x, lens):
    """float64, one slate at a time"""
    lin = lambda z, name: F.linear(z, w[name + ".weight"], w[name + ".bias"])
    an = lambda z, name: w[name + ".a_2"] * (z - z.mean(-1, keepdim=True)) / (z.std(-1, keepdim=True) + 1e-6) + w[name + ".b_2"]
    out, s0 = [], 0
    for n in filter(None, lens):          # an empty slate contributes nothing
        z, s0 = x[s0:s0 + n].double(), s0 + n
        if fc:
            if fc["input_norm"]:
                z = F.layer_norm(z, z.shape[-1:], w["input_layer.input_norm.weight"], w["input_layer.input_norm.bias"], 1e-5)
            z = F.relu(lin(z, "input_layer.layers.0"))
        for i in range(tr["N"]):
            p, h = f"encoder.layers.{i}.", tr["h"]
            y = an(z, p + "sublayer.0.norm")
            q, k, v = (lin(y, f"{p}self_attn.linears.{j}").view(n, h, -1).transpose(0, 1) for j in range(3))
            a = torch.softmax(q @ k.transpose(1, 2) / q.shape[-1] ** 0.5, -1) @ v
            z = z + lin(a.transpose(0, 1).reshape(n, -1), p + "self_attn.linears.3")
            z = z + lin(F.relu(lin(an(z, p + "sublayer.1.norm"), p + "feed_forward.w_1")), p + "feed_forward.w_2")
        out.append(lin(an(z, "encoder.norm"), "output_layer.w_1").sum(-1))
    return torch.cat(out).numpy()


def _rows(n, nf, dtype, seed):
    return torch.randn(n, nf, generator=torch.Generator().manual_seed(seed)).half().to(dtype).cuda()


def _cu(lens):
    return torch.tensor(np.r_[0, np.cumsum(lens)], dtype=torch.int32).cuda()


def _check(model, nf, lens, dt="f32", extras=False):
    head, w, fc, tr = model
    n = sum(lens)
    x = _rows(n, nf, DTYPES[dt], 1)
    r = _rows(n, nf, DTYPES[dt], 2) if extras else None
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(torch.int32) if extras else None
    rows = (x + r if extras else x).float().cpu()                 # the sum rounded once to the input dtype
    want = _twin(w, fc, tr, rows[idx.long()] if extras else rows, lens)
    got = head.score(x, idx.cuda() if extras else None, r, cu_slates=_cu(lens)).cpu().numpy()
    err = np.abs(got - want).max()
    print(f"head_encoder nf={nf} {tr} lens={lens} {dt} extras={extras}: max|d| = {err:.2e}, max|score| = {np.abs(want).max():.2f}")
    assert err <= 1e-4


@pytest.mark.parametrize("n_blocks", [1, 2])
@pytest.mark.parametrize("lens", LAYOUTS, ids=str)
@pytest.mark.parametrize("d_model,h", [(64, 1), (64, 4), (96, 3), (128, 1)])
def test_parity(d_model, h, lens, n_blocks):
    _check(_model(40, d_model, h, n_blocks), 40, lens)


@pytest.mark.parametrize("nf,d_model,h,norm,dt,extras", [(40, 64, 2, True, "f32", False), (96, None, 1, False, "f32", False),
                                                         (96, None, 2, False, "f16", True), (40, 64, 2, True, "bf16", True)])
def test_parity_inputs(nf, d_model, h, norm, dt, extras):
    """FC stack behind the input LayerNorm; fc_model = None (d_k = 96, and 48: a padded head); fp16 and bf16 with a residual
    and a permuted row_index"""
    _check(_model(nf, d_model, h, 2, norm), nf, [5, 0, 64, 1, 67], dt, extras)


def test_slate_does_not_depend_on_the_call():
    head = _model(40, 64, 4, 2)[0]
    x = _rows(137, 40, torch.float32, 4)
    full = head.score(x, cu_slates=_cu([5, 0, 64, 1, 67]))
    assert torch.equal(head.score(x[5:69].contiguous()), full[5:69])          # the third of five, scored alone
    assert torch.equal(head.score(x, cu_slates=_cu([5, 0, 64, 1, 67]), max_slate=1), full)   # the hint sizes the grid only


def test_graph_capture():
    head = _model(40, 64, 4, 2)[0]
    head.reserve(137)
    xs, cu = _rows(137, 40, torch.float32, 7), _cu([5, 0, 64, 1, 67])
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = head.score(xs, cu_slates=cu, max_slate=67)
    new = _rows(137, 40, torch.float32, 8)
    xs.copy_(new)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, head.score(new, cu_slates=cu))


def test_argument_errors():
    from vllm_ltr_amd import _lib
    for kw, msg in [(dict(d_model=96, h=4), "d_k = 24"), (dict(d_model=64, h=4, mode="f32"), "LTR_W_F16")]:
        with pytest.raises(_lib.LtrError, match=msg) as e:
            _model(40, n_blocks=1, **kw)
        assert e.value.code == _lib.LTR_E_INVAL
    head, _, fc, tr = _model(40, 64, 4, 1)
    from vllm_ltr_amd.ltr_head import HipLTRHead
    with pytest.raises(_lib.LtrError, match="not built"):
        HipLTRHead(40, fc, POST, _weights(40, fc, tr), transformer=dict(tr, positional_encoding={"strategy": "fixed", "max_indices": 8}))
    x = _rows(17, 40, torch.float32, 10)
    with pytest.raises(ValueError, match="ascend from 0 to N"):
        head.score(x, cu_slates=_cu([5, 11]))
    lib, out = head.lib, torch.empty(17, dtype=torch.float32, device="cuda")
    need = lib.ltr_head_encoder_workspace_bytes(head._enc, 17)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    call = lambda nbytes: lib.ltr_head_encoder_score(head._enc, x.data_ptr(), None, _lib.LTR_HID_F32, None, 17, None, 1, 17,
                                                     out.data_ptr(), ws.data_ptr(), nbytes, None)
    assert call(need - 1) == _lib.LTR_E_NOMEM and b"workspace" in lib.ltr_last_error()
    assert call(need) == 0
