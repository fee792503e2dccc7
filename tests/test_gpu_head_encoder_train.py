"""Device training of the slate encoder (ltr_head_train_create_encoder, DESIGN 4.4 "training the encoder") against a float64
torch twin of allRank's FCModel -> Encoder -> OutputLayer with autograd on the CPU.  Weights and rows are fp16-rounded, so
they are exact in every dtype.  Bounds: tests/test_gpu_head_train.py's (gradients 2e-5 x max|g_ref| per tensor, scores 1e-4)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.ltr_head import seeded_head_weights

pytestmark = pytest.mark.gpu
POST = {"d_output": 1, "output_activation": None}
GRAD_TOL = 2e-5
NF = 40


def _config(d_model, h, n_blocks, fc=True):
    """(n_features, fc_model, transformer, fp16-rounded f32 weights); fc False: fc_model = None, d_model = n_features"""
    nf, fcm = (NF, {"sizes": [d_model], "input_norm": True, "activation": "ReLU"}) if fc else (d_model, None)
    tr = {"N": n_blocks, "d_ff": 72, "h": h, "positional_encoding": None}
    sd, rs = seeded_head_weights(nf, fcm["sizes"] if fc else None, fc, 1, 11), np.random.RandomState(12)
    mats = [(f"self_attn.linears.{j}", d_model, d_model) for j in range(4)]
    mats += [("feed_forward.w_1", tr["d_ff"], d_model), ("feed_forward.w_2", d_model, tr["d_ff"])]
    norms = [f"encoder.layers.{i}.sublayer.{j}.norm" for i in range(n_blocks) for j in range(2)] + ["encoder.norm"]
    for i in range(n_blocks):
        for k, o, n in mats:
            sd[f"encoder.layers.{i}.{k}.weight"] = rs.standard_normal((o, n)) * (2.0 / (o + n)) ** 0.5
            sd[f"encoder.layers.{i}.{k}.bias"] = 0.05 * rs.standard_normal(o)
    for k in norms:
        sd[k + ".a_2"], sd[k + ".b_2"] = 1.0 + 0.1 * rs.standard_normal(d_model), 0.05 * rs.standard_normal(d_model)
    return nf, fcm, tr, {k: np.asarray(v).astype(np.float16).astype(np.float32) for k, v in sd.items()}


def _twin(p, fc, tr, x, B, S, pad=None):
    """float64 scores [B, S]; pad: bool [B, S], True = the item is masked as a key (allRank's masked_fill(-inf))"""
    lin = lambda z, name: F.linear(z, p[name + ".weight"], p[name + ".bias"])
    an = lambda z, name: p[name + ".a_2"] * (z - z.mean(-1, keepdim=True)) / (z.std(-1, keepdim=True) + 1e-6) + p[name + ".b_2"]
    z = x
    if fc:
        z = F.layer_norm(z, z.shape[-1:], p["input_layer.input_norm.weight"], p["input_layer.input_norm.bias"], 1e-5)
        z = F.relu(lin(z, "input_layer.layers.0"))
    z, h = z.view(B, S, -1), tr["h"]
    for i in range(tr["N"]):
        pre = f"encoder.layers.{i}."
        y = an(z, pre + "sublayer.0.norm")
        q, k, v = (lin(y, f"{pre}self_attn.linears.{j}").view(B, S, h, -1).transpose(1, 2) for j in range(3))
        s = q @ k.transpose(-1, -2) / q.shape[-1] ** 0.5
        if pad is not None:
            s = s.masked_fill(pad[:, None, None, :], float("-inf"))
        z = z + lin((torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, S, -1), pre + "self_attn.linears.3")
        z = z + lin(F.relu(lin(an(z, pre + "sublayer.1.norm"), pre + "feed_forward.w_1")), pre + "feed_forward.w_2")
    return lin(an(z, "encoder.norm"), "output_layer.w_1").sum(-1)


def _params(sd):
    return {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in sd.items()}


def _trainer(cfg, **kw):
    from vllm_ltr_amd.ltr_head_trainer import HipLTRHeadTrainer
    nf, fc, tr, sd = cfg
    return HipLTRHeadTrainer(nf, fc, POST, sd, transformer=tr, **kw)


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _check_grads(tag, got, p):
    """The key projection's bias has the exact gradient 0 - softmax does not see a shift common to all keys - and the twin
    returns its own float64 rounding there (1e-16), which no f32 gradient can be measured against.  That gradient is
    sum_rows dK . 1 where the key weight's is sum_rows dK . norm(z) with |norm(z)| ~ 1, so it is held to the key weight's bound."""
    worst = 0.0
    for k, v in p.items():
        g = v.grad.numpy()
        scale = p[k.replace(".bias", ".weight")].grad.numpy() if k.endswith("self_attn.linears.1.bias") else g
        ref, err = np.abs(scale).max(), np.abs(got[k] - g).max()
        worst = max(worst, err / ref if ref else float(err > 0))
        assert err <= GRAD_TOL * ref, f"{tag} {k}: {err:.3e} > {GRAD_TOL * ref:.3e}"
    return worst


# d_model, h, S, B, n_blocks, fc, dtype: d_k = 64, 16, 32, 128, 96; S around the 32- and 64-row tiles
CASES = [(64, 1, 1, 1, 1, True, "f32"), (64, 4, 63, 3, 2, True, "f32"), (96, 3, 64, 1, 1, True, "f32"),
         (128, 1, 65, 3, 1, True, "f32"), (96, 1, 130, 1, 2, True, "f32"), (64, 1, 130, 3, 1, True, "f32"),
         (128, 1, 1, 3, 2, True, "f32"), (96, 3, 63, 3, 1, True, "f32"), (64, 4, 65, 3, 1, False, "f32"),
         (64, 4, 65, 3, 2, True, "f16")]


@pytest.mark.parametrize("dm,h,S,B,nb,fc,dt", CASES)
def test_gradient_parity(dm, h, S, B, nb, fc, dt):
    """Given dLoss/dscore ~ N(0, 1), no update.  fc False: the encoder's input gradient stops at the rows.  f16: fp16 rows with
    a residual and a permuted row_index."""
    cfg = _config(dm, h, nb, fc)
    nf, fcm, tr, sd = cfg
    x = _randn(B * S, nf, seed=1).half()
    r = idx = None
    rows = x
    if dt == "f16":
        r = _randn(B * S, nf, seed=2).half()
        idx = torch.randperm(B * S, generator=torch.Generator().manual_seed(3)).to(torch.int32)
        rows = (x + r)[idx.long()]
    else:
        x = x.float()
    ds, p = _randn(B, S, seed=4), _params(sd)
    want = _twin(p, fcm, tr, rows.double(), B, S)
    want.backward(ds.double())
    t = _trainer(cfg, loss="given")
    t.step(x.cuda(), ds.cuda(), None if idx is None else idx.cuda(), None if r is None else r.cuda(), apply_update=False)
    es = np.abs(t.scores.cpu().numpy() - want.detach().numpy()).max()
    worst = _check_grads(f"{dm}/{h} {B}x{S}", t.gradients(), p)
    print(f"encoder_train {dm}/{h} N={nb} {B}x{S} {dt}: scores max|d| = {es:.2e}, gradients max|d| / max|g| = {worst:.2e}")
    assert es <= 1e-4


def test_padding_mask():
    """listMLE on 3 x 65 with scattered padded items, a slate with one valid item and a slate with none padded: padded items
    are masked as keys, and what a padded row holds changes no gradient."""
    from vllm_ltr_amd import train_loss
    B, S = 3, 65
    cfg = _config(64, 4, 2)
    nf, fcm, tr, sd = cfg
    x = _randn(B * S, nf, seed=5).half().float()
    y = torch.randint(0, 5, (B, S), generator=torch.Generator().manual_seed(6)).float()
    y[0, [3, 31, 32, 64]] = -1.0
    y[1] = -1.0
    y[1, 40] = 2.0
    sh = torch.randperm(S, generator=torch.Generator().manual_seed(7))
    t = _trainer(cfg, loss="listMLE")
    t.step(x.cuda(), y.cuda(), shuffle=sh.cuda(), apply_update=False)
    got = t.gradients()
    _, ds = train_loss.listmle(t.scores, y.cuda(), sh.cuda())
    p = _params(sd)
    want = _twin(p, fcm, tr, x.double(), B, S, y == -1.0)
    want.backward(ds.cpu().double())
    valid = (y != -1.0).numpy()
    es = np.abs(t.scores.cpu().numpy() - want.detach().numpy())[valid].max()
    worst = _check_grads("mask", got, p)
    print(f"encoder_train mask: valid scores max|d| = {es:.2e}, gradients max|d| / max|g| = {worst:.2e}")
    assert es <= 1e-4
    x2 = x.clone()
    x2[torch.from_numpy(~valid).reshape(-1)] += 1.0
    t.step(x2.cuda(), y.cuda(), shuffle=sh.cuda(), apply_update=False)
    _check_grads("mask, other padded rows", t.gradients(), p)      # the twin's gradients of the first rows still hold


def test_adam_steps():
    """Three LambdaLoss steps against torch.optim.Adam on the twin fed the device's dLoss/dscore, by test_adam_steps' rule of
    the encoder-less head.  LambdaLoss does not see a shift of all scores, so the exact gradients of the output bias and of
    the final norm's b_2 are 0: Adam turns what rounding leaves of them into steps of size lr whose sign is noise, in the twin
    as on the device (measured: 4.3e-3 apart after three steps).  The same holds for every key projection's bias, whose exact
    gradient is 0 under any loss (_check_grads).  Those are held to Adam's own bound on three steps from the initial value."""
    from vllm_ltr_amd import train_loss
    lr, n_steps, B, S = 1e-3, 3, 2, 65
    cfg = _config(64, 4, 2)
    nf, fcm, tr, sd = cfg
    x = _randn(B * S, nf, seed=10).half().float()
    y = torch.randint(0, 5, (B, S), generator=torch.Generator().manual_seed(11)).float()
    t, p = _trainer(cfg, loss="lambdaLoss", lr=lr), _params(sd)
    opt = torch.optim.Adam(p.values(), lr=lr)
    for _ in range(n_steps):
        opt.zero_grad()
        s = _twin(p, fcm, tr, x.double(), B, S, y == -1.0)
        _, ds = train_loss.lambdaloss(s.detach().float().cuda(), y.cuda())
        s.backward(ds.cpu().double())
        opt.step()
        t.step(x.cuda(), y.cuda())
    for k, v in t.state_dict().items():
        d = np.abs(v - p[k].detach().numpy())
        if k in ("output_layer.w_1.bias", "encoder.norm.b_2") or k.endswith("self_attn.linears.1.bias"):
            assert np.abs(v - sd[k]).max() <= 1.01 * lr * n_steps, k
            continue
        tol = 0.02 * lr * n_steps
        print(f"encoder_train adam {k}: max|d| = {d.max():.2e}, beyond {tol:.0e}: {(d > tol).mean():.4f}")
        assert (d <= tol).mean() >= 0.995 and d.max() <= 1.01 * lr * n_steps, k


def test_determinism_and_round_trip():
    """Two trainers fed the same three slates hold identical bits; the trained weights, rounded to fp16, score one slate in
    HipLTRHead as the twin does."""
    B, S = 3, 65
    cfg = _config(64, 4, 2)
    nf, fcm, tr, _ = cfg
    x = _randn(B * S, nf, seed=13).half().float().cuda()
    y = torch.randint(0, 5, (B, S), generator=torch.Generator().manual_seed(14)).float().cuda()
    sh = torch.randperm(S, generator=torch.Generator().manual_seed(15)).cuda()
    a, b = _trainer(cfg, lr=1e-3), _trainer(cfg, lr=1e-3)
    for _ in range(3):
        a.step(x, y, shuffle=sh)
        b.step(x, y, shuffle=sh)
    sa, sb = a.state_dict(), b.state_dict()
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)
    got = a.to_head().score(x[:S], cu_slates=torch.tensor([0, S], dtype=torch.int32).cuda()).cpu().numpy()
    w = {k: torch.from_numpy((v.astype(np.float16) if v.ndim == 2 else v).astype(np.float64)) for k, v in sa.items()}   # the head keeps vectors in f32
    es = np.abs(got - _twin(w, fcm, tr, x[:S].cpu().double(), 1, S).numpy().reshape(-1)).max()
    print(f"encoder_train round trip: scores max|d| = {es:.2e}")
    assert es <= 1e-4


def test_argument_errors():
    from vllm_ltr_amd import _lib
    from vllm_ltr_amd.ltr_head_trainer import HipLTRHeadTrainer
    with pytest.raises(NotImplementedError):
        HipLTRHeadTrainer(64, None, POST, transformer={"N": 1, "d_ff": 72, "h": 1, "positional_encoding": None, "dropout": 0.1})
    lib = _lib.load()
    desc = _lib.HeadDesc(64, 0, (C.c_int32 * 8)(), 0, 0, 1, 0, _lib.LTR_W_F32)
    cfg = _lib.HeadTrainConfig(1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1e-10, -1.0, 0.0)
    buf = torch.zeros(64, device="cuda")
    ptrs, h = (C.c_void_p * 18)(*([buf.data_ptr()] * 18)), C.c_void_p()
    create = lambda enc, n: lib.ltr_head_train_create_encoder(C.byref(desc), C.byref(_lib.HeadEncoderDesc(*enc)), ptrs, n,
                                                              C.byref(cfg), None, C.byref(h))
    assert create((1, 72, 8, 0), 18) == _lib.LTR_E_INVAL      # d_k = 8: not a multiple of 16
    assert create((1, 72, 1, 1), 18) == _lib.LTR_E_INVAL      # positional encoding
    assert create((1, 72, 1, 0), 17) == _lib.LTR_E_INVAL      # 4 + 12 + 2 pointers are expected
    ptrs[9] = None
    assert create((1, 72, 1, 0), 18) == _lib.LTR_E_INVAL      # a NULL weight
    desc.n_features = 256
    assert create((1, 72, 1, 0), 18) == _lib.LTR_E_INVAL      # d_k = 256 > 128
