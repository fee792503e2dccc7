"""LambdaLoss on the device (ltr_lambdaloss) against a float64 restatement of the definition in include/ltr_hip.h:
the plain double loop over the items of a slate in their original order.  Scores are 3 * randn, labels integers 0 .. 4 with
some -1 (padded): neither clamp is active, so parity compares smooth values; the clamp has its own case in test_edge_rules.

Measured on MI355X, worst over the parity cases: loss 1.1e-7 relative, gradient 2.5e-7 of its largest entry."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vllm_ltr_amd import _lib, train_loss

TOL = 2e-5            # test_listmle.py's loss bound and GRAD_TOL of test_gpu_head_train.py
PP = "ndcgLoss2PP_scheme"


def _twin(yp, yt, weighing_scheme=None, k=None, sigma=1.0, mu=10.0, reduction="sum", reduction_log="binary", eps=1e-10, pad=-1.0):
    yp, yt = np.asarray(yp, np.float64), np.asarray(yt, np.float64)
    B, S = yp.shape
    D = np.log2(np.arange(2, S + 2, dtype=np.float32)).astype(np.float64)       # f32 discounts, as the reference
    kk = S if not k or k > S else k
    c = math.log(2.0) if reduction_log == "binary" else 1.0
    loss, n, grad = 0.0, 0, np.zeros((B, S))
    for b in range(B):
        valid = [i for i in range(S) if yt[b, i] != pad]
        rank = {i: r for r, i in enumerate(sorted(valid, key=lambda i: (-yp[b, i], i)))}
        ideal = sorted((yt[b, i] for i in valid), reverse=True)[:kk]
        max_dcg = max(sum((2.0 ** l - 1.0) / D[p] for p, l in enumerate(ideal)), eps)
        G = (2.0 ** yt[b] - 1.0) / max_dcg
        for i in valid:
            for j in valid:
                ri, rj, li, lj = rank[i], rank[j], yt[b, i], yt[b, j]
                if ri >= kk or rj >= kk or (weighing_scheme != "ndcgLoss1_scheme" and not li > lj):
                    continue
                d = abs(ri - rj)
                l2 = abs(1.0 / D[d - 1] - 1.0 / D[d]) * abs(G[i] - G[j]) if d else 0.0
                lr = abs(1.0 / D[ri] - 1.0 / D[rj]) * abs(G[i] - G[j])
                w = {None: 1.0, "rankNet_scheme": 1.0, "ndcgLoss1_scheme": G[i] / D[ri], "ndcgLoss2_scheme": l2,
                     "lambdaRank_scheme": lr, PP: mu * l2 + lr, "rankNetWeightedByGTDiff_scheme": abs(li - lj),
                     "rankNetWeightedByGTDiffPowed_scheme": abs(li * li - lj * lj)}[weighing_scheme]
                x = min(max(yp[b, i] - yp[b, j], -1e8), 1e8)
                p0 = 1.0 / (1.0 + math.exp(-sigma * x))
                p = max(p0, eps)
                q0 = p ** w
                loss -= math.log(max(q0, eps)) / c
                n += 1
                if i != j and p0 >= eps and q0 >= eps and abs(yp[b, i] - yp[b, j]) <= 1e8:
                    g = w * sigma * (1.0 - p) / c
                    grad[b, i] -= g
                    grad[b, j] += g
    if reduction == "mean" and n:
        loss, grad = loss / n, grad / n
    return loss, grad


def _inputs(B, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    yp = 3.0 * torch.randn(B, S, generator=g)
    yt = torch.randint(0, 5, (B, S), generator=g).float()
    yt[torch.rand(B, S, generator=g) < 0.15] = -1.0
    if S >= 2:
        yt[:, 0], yt[:, 1] = 1.0, 3.0                    # every slate has a pair, the two-item slate exactly one
    return yp, yt


def _close(tag, got_loss, got_grad, want_loss, want_grad, yt):
    el, eg, ref = abs(got_loss - want_loss), np.abs(got_grad - want_grad).max(), np.abs(want_grad).max()
    print(f"lambdaloss {tag}: loss {got_loss:.6f} |d| = {el:.2e} ({el / max(1.0, abs(want_loss)):.2e} rel), "
          f"grad max|d| = {eg:.2e} ({eg / ref if ref else 0.0:.2e} of max|g| = {ref:.3e})")
    assert el <= TOL * max(1.0, abs(want_loss))
    assert eg <= TOL * ref
    assert (got_grad[np.asarray(yt) == -1.0] == 0.0).all()


SCHEMES = [None, "rankNet_scheme", "ndcgLoss1_scheme", "ndcgLoss2_scheme", "lambdaRank_scheme", "rankNetWeightedByGTDiff_scheme",
           "rankNetWeightedByGTDiffPowed_scheme"]
CASES = ([(B, S, {"weighing_scheme": PP}) for B, S in [(1, 1), (1, 2), (3, 63), (2, 64), (2, 65), (2, 257), (1, 300)]]
         + [(2, 65, {"weighing_scheme": s}) for s in SCHEMES]
         + [(1, 300, {"weighing_scheme": PP, "k": k}) for k in (5, 70)]       # (k = None at 1 x 300 is in the first row)
         + [(3, 63, {"weighing_scheme": PP, "reduction": "mean", "reduction_log": "natural", "sigma": 2.0})])


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,kw", CASES, ids=lambda v: "-".join(f"{x}" for x in v.values()) if isinstance(v, dict) else str(v))
def test_parity(B, S, kw):
    yp, yt = _inputs(B, S)
    want_loss, want_grad = _twin(yp.numpy(), yt.numpy(), **kw)
    loss, grad = train_loss.lambdaloss(yp.cuda(), yt.cuda(), **kw)
    _close(f"{B}x{S} {kw}", loss.item(), grad.cpu().numpy().astype(np.float64), want_loss, want_grad, yt)
    loss_only, none = train_loss.lambdaloss(yp.cuda(), yt.cuda(), with_grad=False, **kw)
    assert none is None and torch.equal(loss_only, loss)


@pytest.mark.gpu
def test_edge_rules():
    # equal scores: the lower index ranks first (a third item makes the two orders weigh differently)
    yp, yt = torch.tensor([[1.0, 1.0, 0.0]]), torch.tensor([[0.0, 2.0, 1.0]])
    want_loss, want_grad = _twin(yp.numpy(), yt.numpy(), "lambdaRank_scheme")
    loss, grad = train_loss.lambdaloss(yp.cuda(), yt.cuda(), "lambdaRank_scheme")
    _close("tie", loss.item(), grad.cpu().numpy().astype(np.float64), want_loss, want_grad, yt)
    # no selected pair: all labels equal, all padded
    yp, yt = _inputs(2, 5)[0], torch.tensor([[2.0] * 5, [-1.0] * 5])
    for reduction in ("sum", "mean"):
        loss, grad = train_loss.lambdaloss(yp.cuda(), yt.cuda(), PP, reduction=reduction)
        assert loss.item() == 0.0 and not grad.any().item(), reduction
    # the eps clamp: sigmoid(-40) < 1e-10
    loss, grad = train_loss.lambdaloss(torch.tensor([[-40.0, 0.0]]).cuda(), torch.tensor([[1.0, 0.0]]).cuda(), "rankNet_scheme", eps=1e-10)
    assert abs(loss.item() + math.log2(1e-10)) <= TOL * -math.log2(1e-10) and not grad.any().item()
    # two calls, identical bits
    yp, yt = (t.cuda() for t in _inputs(2, 257, seed=1))
    (l1, g1), (l2, g2) = train_loss.lambdaloss(yp, yt, PP), train_loss.lambdaloss(yp, yt, PP)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


@pytest.mark.gpu
def test_trainer_wiring():
    """Head `a` of test_gpu_head_train.py (96 features, LayerNorm, one FC of 40, ReLU): the step's loss is lambdaloss on its own
    scores, and its gradients are the float64 autograd twin's under that dscore."""
    from oracle.ltr_head import seeded_head_weights
    from vllm_ltr_amd.ltr_head_trainer import HipLTRHeadTrainer
    B, S, args = 3, 17, {"weighing_scheme": "lambdaRank_scheme", "k": 10}
    w = seeded_head_weights(96, [40], True, 1, 11)
    x = torch.randn(B * S, 96, generator=torch.Generator().manual_seed(5)).half().float()
    y = torch.randint(0, 5, (B, S), generator=torch.Generator().manual_seed(6)).float()
    y[1, 4] = -1.0
    tr = HipLTRHeadTrainer(96, {"sizes": [40], "input_norm": True, "activation": "ReLU"}, {"d_output": 1, "output_activation": None},
                           w, loss="lambdaLoss", loss_args=args)
    got = tr.step(x.cuda(), y.cuda(), apply_update=False).item()
    ref, ds = train_loss.lambdaloss(tr.scores, y.cuda(), **args)
    assert abs(got - ref.item()) <= TOL * abs(ref.item())
    p = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in w.items()}
    h = F.layer_norm(x.double(), (96,), p["input_layer.input_norm.weight"], p["input_layer.input_norm.bias"], 1e-5)
    h = F.relu(F.linear(h, p["input_layer.layers.0.weight"], p["input_layer.layers.0.bias"]))
    F.linear(h, p["output_layer.w_1.weight"], p["output_layer.w_1.bias"]).sum(-1).backward(ds.cpu().double().reshape(-1))
    for k, g in tr.gradients().items():
        want = p[k].grad.numpy()
        err, scale = np.abs(g - want).max(), np.abs(want).max()
        print(f"lambdaloss trainer {k}: max|d| / max|g| = {err / scale:.2e}")
        assert err <= TOL * scale, k


def test_argument_errors_without_a_device():
    import __graft_entry__ as entry
    import os
    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    lib = _lib.load()
    assert lib.ltr_lambdaloss_workspace_bytes(1, 4097) == 0
    need = lib.ltr_lambdaloss_workspace_bytes(2, 65)
    assert need > 0

    def call(cfg, y_pred=256, ws_bytes=need):             # (pointers are never followed: the checks come first)
        return lib.ltr_lambdaloss(y_pred, 256, 2, 65, C.byref(cfg), 256, None, 256, ws_bytes, None)
    assert call(_lib.LambdaLossConfig(8, 0, 1.0, 10.0, 0, 0, 1e-10, -1.0)) == _lib.LTR_E_INVAL
    assert call(_lib.LambdaLossConfig(5, 0, 1.0, 10.0, 2, 0, 1e-10, -1.0)) == _lib.LTR_E_INVAL
    good = _lib.lambdaloss_config(PP, k=10)
    assert call(good, y_pred=None) == _lib.LTR_E_INVAL
    assert call(good, ws_bytes=need - 1) == _lib.LTR_E_NOMEM
    with pytest.raises(ValueError, match="nope"):
        train_loss.lambdaloss(torch.zeros(1, 2), torch.zeros(1, 2), weighing_scheme="nope")
