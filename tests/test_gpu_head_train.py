"""Device training of the hidden-state head (ltr_head_train_*, DESIGN 4.4 "training") against the same head in torch float64
with autograd on the CPU.  Inputs are fp16-rounded, so they are exact in f32, fp16 and bf16."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.ltr_head import OracleLTRHead, seeded_head_weights

pytestmark = pytest.mark.gpu
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
_A = lambda act, out=None: (96, {"sizes": [40], "input_norm": True, "activation": act}, {"d_output": 1, "output_activation": out})
HEADS = {"a": _A("ReLU"), "a_gelu": _A("GELU"), "a_silu": _A("SiLU"), "a_sigmoid": _A("Sigmoid", "Sigmoid"),
         "b": (256, {"sizes": [128, 64], "input_norm": False, "activation": "Tanh"}, {"d_output": 3, "output_activation": None}),
         "c": (100, None, {"d_output": 1, "output_activation": None})}
ACT = {None: lambda x: x, "ReLU": F.relu, "Sigmoid": torch.sigmoid, "Tanh": torch.tanh, "GELU": F.gelu, "SiLU": F.silu}
GRAD_TOL = 2e-5          # x max|g_ref| per tensor: the project's figure for f32-grade training gradients


def _weights(name):
    nf, fc, post = HEADS[name]
    return seeded_head_weights(nf, fc["sizes"] if fc else None, bool(fc and fc["input_norm"]), post["d_output"], 11)


def _trainer(name, **kw):
    from vllm_ltr_amd.ltr_head_trainer import HipLTRHeadTrainer
    nf, fc, post = HEADS[name]
    return HipLTRHeadTrainer(nf, fc, post, _weights(name), **kw)


def _twin(name):
    return {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in _weights(name).items()}


def _twin_scores(p, name, x):
    nf, fc, post = HEADS[name]
    h = x
    if fc:
        if fc["input_norm"]:
            h = F.layer_norm(h, (nf,), p["input_layer.input_norm.weight"], p["input_layer.input_norm.bias"], 1e-5)
        for i in range(len(fc["sizes"])):
            h = ACT[fc["activation"]](F.linear(h, p[f"input_layer.layers.{i}.weight"], p[f"input_layer.layers.{i}.bias"]))
    return ACT[post["output_activation"]](F.linear(h, p["output_layer.w_1.weight"], p["output_layer.w_1.bias"])).sum(-1)


def _twin_grads(name, x, dscore):
    p = _twin(name)
    s = _twin_scores(p, name, x)
    s.backward(dscore.double().reshape(-1))
    return s.detach().numpy(), {k: v.grad.numpy() for k, v in p.items()}


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _check_grads(tag, got, want, scale=1.0):
    worst = 0.0
    for k, g in want.items():
        ref = np.abs(g).max() * scale
        err = np.abs(got[k] - g * scale).max()
        worst = max(worst, err / ref if ref else float(err > 0))
        assert err <= GRAD_TOL * ref, f"{tag} {k}: {err:.3e} > {GRAD_TOL * ref:.3e}"
    return worst


CASES = [(n, bs, "f32") for n in HEADS for bs in [(1, 1), (1, 65), (2, 65), (8, 70)]] + [("a", (2, 65), "f16"), ("b", (2, 65), "bf16")]


@pytest.mark.parametrize("name,bs,dt", CASES)
def test_gradient_parity(name, bs, dt):
    """Given dLoss/dscore ~ N(0, 1).  8 x 70 rows span two 512-row parts of the narrow layers' weight gradients; fp16 / bf16
    rows come with a residual and a permuted row_index that names one row twice."""
    (B, S), nf, M = bs, HEADS[name][0], bs[0] * bs[1]
    x = _randn(M, nf, seed=1).half().to(DTYPES[dt])
    r = idx = None
    rows = x
    if dt != "f32":
        r = _randn(M, nf, seed=2).half().to(DTYPES[dt])
        idx = torch.randperm(M, generator=torch.Generator().manual_seed(3)).to(torch.int32)
        idx[-1] = idx[0]
        rows = (x + r)[idx.long()]                       # the sum rounded once to the input dtype
    ds = _randn(B, S, seed=4)
    want_s, want_g = _twin_grads(name, rows.double(), ds)
    tr = _trainer(name, loss="given")
    tr.step(x.cuda(), ds.cuda(), None if idx is None else idx.cuda(), None if r is None else r.cuda(), apply_update=False)
    es = np.abs(tr.scores.cpu().numpy().reshape(-1) - want_s).max()
    worst = _check_grads(f"{name} {bs} {dt}", tr.gradients(), want_g)
    print(f"head_train {name} {B}x{S} {dt}: scores max|d| = {es:.2e}, gradients max|d| / max|g| = {worst:.2e}")
    assert es <= 1e-4


@pytest.mark.parametrize("loss", ["listMLE", "neuralNDCG", "mse"])
def test_losses_are_wired(loss):
    from vllm_ltr_amd import train_loss
    B, S = 3, 17
    x = _randn(B * S, 96, seed=5).half().float()
    y = torch.randint(0, 5, (B, S), generator=torch.Generator().manual_seed(6)).float()
    y[1, 4] = -1.0                                       # one padded item
    sh = torch.randperm(S, generator=torch.Generator().manual_seed(7))
    tr = _trainer("a", loss=loss)
    got_loss = tr.step(x.cuda(), y.cuda(), shuffle=sh.cuda(), apply_update=False).item()
    if loss == "mse":
        s = torch.tensor(tr.scores.cpu().numpy(), dtype=torch.float64, requires_grad=True)
        ref = F.mse_loss(s, y.double())
        ref.backward()
        ref_loss, ds = ref.item(), s.grad
    else:
        fn = train_loss.listmle if loss == "listMLE" else train_loss.neuralndcg
        l, g = fn(tr.scores, y.cuda(), sh.cuda()) if loss == "listMLE" else fn(tr.scores, y.cuda())
        ref_loss, ds = l.item(), g.cpu()
    _, want_g = _twin_grads("a", x.double(), ds)
    worst = _check_grads(loss, tr.gradients(), want_g)
    print(f"head_train {loss}: loss {got_loss:.6f} vs {ref_loss:.6f}, gradients max|d| / max|g| = {worst:.2e}")
    assert abs(got_loss - ref_loss) <= GRAD_TOL * abs(ref_loss)


def test_clip_and_norm():
    x, ds = _randn(65, 96, seed=8).half().float(), _randn(1, 65, seed=9)
    _, want_g = _twin_grads("a", x.double(), ds)
    norm = float(np.sqrt(sum((g ** 2).sum() for g in want_g.values())))
    tr = _trainer("a", loss="given", clip_norm=0.5 * norm)
    tr.step(x.cuda(), ds.cuda(), apply_update=False)
    got = tr.grad_norm.item()
    print(f"head_train norm {got:.6f} vs {norm:.6f}")
    assert abs(got - norm) <= GRAD_TOL * norm
    _check_grads("clip", tr.gradients(), want_g, scale=0.5 * norm / (norm + 1e-6))


def test_adam_steps():
    """Three steps against torch.optim.Adam on the f64 twin, judged by the rule of test_train_step._final_close; a
    gradient-only call between them must move neither the parameters, the moments nor the step count."""
    lr, n_steps = 1e-3, 3
    x = _randn(130, 96, seed=10).half().float()
    tr = _trainer("a", loss="given", lr=lr, weight_decay=0.01)
    p = _twin("a")
    opt = torch.optim.Adam(p.values(), lr=lr, weight_decay=0.01)
    for st in range(n_steps):
        ds = _randn(2, 65, seed=20 + st)
        tr.step(x.cuda(), ds.cuda())
        opt.zero_grad()
        _twin_scores(p, "a", x.double()).backward(ds.double().reshape(-1))
        opt.step()
        if st == 0:
            before = tr.state_dict()
            tr.step(x.cuda(), _randn(2, 65, seed=30).cuda(), apply_update=False)
            assert all(np.array_equal(v, before[k]) for k, v in tr.state_dict().items())
    for k, v in tr.state_dict().items():
        d = np.abs(v - p[k].detach().numpy())
        tol = 0.02 * lr * n_steps
        print(f"head_train adam {k}: max|d| = {d.max():.2e}, beyond {tol:.0e}: {(d > tol).mean():.4f}")
        assert (d <= tol).mean() >= 0.995 and d.max() <= 1.01 * lr * n_steps, k


def test_two_trainers_are_bit_identical():
    x = _randn(8 * 70, 96, seed=11).half().float().cuda()
    y = torch.randint(0, 5, (8, 70), generator=torch.Generator().manual_seed(12)).float().cuda()
    sh = torch.randperm(70, generator=torch.Generator().manual_seed(13)).cuda()
    a, b = _trainer("a", lr=1e-3), _trainer("a", lr=1e-3)
    for _ in range(4):
        a.step(x, y, shuffle=sh)
        b.step(x, y, shuffle=sh)
    sa, sb = a.state_dict(), b.state_dict()
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)


def test_round_trip_to_the_scoring_head():
    """The no-FC head under MSE on labels linear in the rows is convex: the f64 twin's loss falls over the same 20 steps."""
    from vllm_ltr_amd import metrics
    B, S, lr = 4, 16, 1e-2
    x = _randn(B * S, 100, seed=14).half().float()
    y = (x @ _randn(100, seed=15) * 0.1 + 0.3).reshape(B, S)
    p = _twin("c")
    opt = torch.optim.Adam(p.values(), lr=lr)
    twin_losses = []
    for _ in range(20):
        opt.zero_grad()
        l = F.mse_loss(_twin_scores(p, "c", x.double()), y.double().reshape(-1))
        l.backward()
        opt.step()
        twin_losses.append(l.item())
    assert twin_losses[-1] < twin_losses[0]
    tr = _trainer("c", loss="mse", lr=lr)
    losses = [tr.step(x.cuda(), y.cuda()).item() for _ in range(20)]
    print(f"head_train round trip: loss {losses[0]:.4f} -> {losses[-1]:.4f} (twin {twin_losses[0]:.4f} -> {twin_losses[-1]:.4f})")
    assert losses[-1] < losses[0]
    nf, fc, post = HEADS["c"]
    got = tr.to_head("f32").score(x.cuda())
    want = OracleLTRHead(nf, fc, post, tr.state_dict(), torch.float64).score(x.numpy())
    assert np.abs(got.cpu().numpy() - want).max() <= 1e-4
    assert tr.evaluate(x.cuda(), y.cuda()) == metrics.kendall_tau(y.reshape(-1).cuda(), got)


def test_argument_errors():
    from vllm_ltr_amd import _lib
    from vllm_ltr_amd.ltr_head_trainer import HipLTRHeadTrainer
    with pytest.raises(NotImplementedError):
        HipLTRHeadTrainer(96, {"sizes": [40], "input_norm": True, "activation": "ReLU", "dropout": 0.1}, HEADS["a"][2])
    lib = _lib.load()
    desc = _lib.HeadDesc(96, 0, (C.c_int32 * 8)(), 0, 0, 1, 0, _lib.LTR_W_F16)
    cfg = _lib.HeadTrainConfig(1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1e-10, -1.0, 0.0)
    ptrs, h = (C.c_void_p * 4)(), C.c_void_p()
    assert lib.ltr_head_train_create(C.byref(desc), ptrs, 4, C.byref(cfg), None, C.byref(h)) == _lib.LTR_E_INVAL   # fp16 master weights
    desc.weight_dtype, cfg.loss = _lib.LTR_W_F32, _lib.LOSSES["crossentropy"]
    assert lib.ltr_head_train_create(C.byref(desc), ptrs, 4, C.byref(cfg), None, C.byref(h)) == _lib.LTR_E_INVAL
    x = torch.zeros(8, 96, device="cuda")
    y = torch.zeros(8, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.zeros(1, device="cuda")

    def step(tr, hidden, dtype, B, S, shuffle, ws_bytes):
        return lib.ltr_head_train_step(tr._h, hidden, None, dtype, None, B, S, y.data_ptr(), shuffle, 0, out.data_ptr(), None,
                                       None, ws.data_ptr(), ws_bytes, None)
    tr = _trainer("a")
    full = ws.numel()
    assert step(tr, None, 0, 1, 8, y.data_ptr(), full) == _lib.LTR_E_INVAL                  # NULL hidden
    assert step(tr, x.data_ptr(), 7, 1, 8, y.data_ptr(), full) == _lib.LTR_E_INVAL          # bad dtype
    assert step(tr, x.data_ptr(), 0, 1, 8, None, full) == _lib.LTR_E_INVAL                  # listMLE without shuffle
    assert step(tr, x.data_ptr(), 0, 1, 4097, y.data_ptr(), full) == _lib.LTR_E_INVAL       # listMLE S > 4096
    assert step(tr, x.data_ptr(), 0, 1, 8, y.data_ptr(), 64) == _lib.LTR_E_NOMEM            # short workspace
    assert step(tr, x.data_ptr(), 0, 0, 8, y.data_ptr(), full) == 0                         # B * S == 0
    assert step(_trainer("a", loss="neuralNDCG"), x.data_ptr(), 0, 8, 1, None, full) == _lib.LTR_E_INVAL   # S = 1
    torch.cuda.synchronize()
