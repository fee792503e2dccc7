"""Slate metrics on the device (ltr_slate_metrics) against a float64 restatement of the definition in include/ltr_hip.h:
stable argsort of (-score, index), f32 log2 discounts, cumulative sums.  Scores are 3 * randn, labels integers 0 .. 4, about 15 %
padded.  Bounds (derived, not measured: a few ulp per term, sums in f64): |d| <= 1e-5 max(1, dcg), 1e-5 on ndcg and the means,
mrr exact.  The mean of dcg is held to 1e-5 max(1, mean): f32, the type of mean_out, resolves 1.2e-4 at the ~1,800 of a
4096-item slate, so an absolute 1e-5 cannot be represented there; the means of ndcg and mrr are <= 1, where the two readings agree.

Measured on MI355X, worst over the parity cases: dcg 1.0e-7 relative, ndcg 1.0e-7, mrr 0; means: ndcg 7.3e-8, mrr 2.7e-8, dcg
6e-8 relative (1.1e-4 absolute at 1 x 4096)  (DESIGN.md 4.9 "Slate metrics")."""
import numpy as np
import pytest
import torch

from vllm_ltr_amd import metrics

pytestmark = pytest.mark.gpu
TOL = 1e-5
WORST = {}


def _twin(yp, yt, ats=None, gain="pow2", pad=-1.0, filler=1.0):
    yp, yt = np.asarray(yp, np.float64), np.asarray(yt, np.float64)
    B, S = yp.shape
    ats = [S] if ats is None else list(ats)
    disc = 1.0 / np.log2(np.arange(2, S + 2, dtype=np.float32)).astype(np.float64)
    g = (lambda l: 2.0 ** l - 1.0) if gain == "pow2" else (lambda l: l)
    dcg, ndcg, mrr = (np.zeros((B, len(ats))) for _ in range(3))
    v = np.zeros(B)
    for b in range(B):
        padded = yt[b] == pad
        s, l = np.where(padded, -np.inf, yp[b]) + 0.0, np.where(padded, 0.0, yt[b])
        by_score = l[np.argsort(-s, kind="stable")]
        cd, ci = np.cumsum(g(by_score) * disc), np.cumsum(g(np.sort(l)[::-1]) * disc)
        p, v[b] = int(np.argmax(by_score)), by_score.max()
        for j, a in enumerate(ats):
            c = min(a, S) - 1
            dcg[b, j], ndcg[b, j] = cd[c], (filler if ci[c] == 0 else cd[c] / ci[c])
            mrr[b, j] = np.float32(1) / np.float32(p + 1) if p < a else 0.0
    if v.sum() == 0:
        mrr[:] = 0.0
    return {"ndcg": ndcg, "dcg": dcg, "mrr": mrr}


def _inputs(B, S, seed=0, decimals=None):
    g = torch.Generator().manual_seed(seed)
    yp = 3.0 * torch.randn(B, S, generator=g)
    if decimals is not None:
        yp = torch.round(yp, decimals=decimals)
    yt = torch.randint(0, 5, (B, S), generator=g).float()
    yt[torch.rand(B, S, generator=g) < 0.15] = -1.0
    return yp, yt


def _close(tag, got, want, names=("ndcg", "dcg", "mrr")):
    for k in names:
        d = np.abs(np.asarray(got[k], np.float64) - want[k])
        bound = TOL * np.maximum(1.0, want[k]) if k == "dcg" else (0.0 if k == "mrr" else TOL)
        WORST[k] = max(WORST.get(k, 0.0), float((d / np.maximum(1.0, want[k])).max()))
        print(f"slate metrics {tag} {k}: max|d| = {d.max():.2e} (worst so far {WORST[k]:.2e})")
        assert (d <= bound).all(), (tag, k, float(d.max()))


def _device(yp, yt, ats, gain="pow2", **kw):
    yp, yt = yp.cuda(), yt.cuda()
    return {"ndcg": metrics.ndcg(yp, yt, ats, gain, **kw).cpu().numpy(), "dcg": metrics.dcg(yp, yt, ats, gain).cpu().numpy(),
            "mrr": metrics.mrr(yp, yt, ats).cpu().numpy()}


SHAPES = [(B, S) for S in (1, 2, 63, 64, 65, 257, 1000, 4096) for B in (1, 3)] + [(130, 64)]


@pytest.mark.parametrize("B,S", SHAPES)
def test_parity(B, S):
    yp, yt = _inputs(B, S)
    for gain in ("pow2", "identity"):
        for ats in ([1, 5, 10, S, S + 7], None):
            want = _twin(yp.numpy(), yt.numpy(), ats, gain)
            _close(f"{B}x{S} {gain} {ats}", _device(yp, yt, ats, gain), want)
        ats = sorted({1, 5, 10, S, S + 7})
        means = metrics.slate_metrics(yp.cuda(), yt.cuda(), {k: ats for k in want}, gain)
        want = _twin(yp.numpy(), yt.numpy(), ats, gain)
        for k in want:
            d = np.abs(np.array([means[f"{k}_{a}"] for a in ats]) - want[k].mean(0))
            print(f"slate metrics {B}x{S} {gain} mean {k}: max|d| = {d.max():.2e}")
            assert (d <= TOL * np.maximum(1.0, want[k].mean(0))).all(), (k, d)


@pytest.mark.parametrize("B,S", [(3, 64), (3, 257)])
def test_ties_rank_by_index(B, S):
    yp, yt = _inputs(B, S, seed=1, decimals=1)
    assert np.unique(yp.numpy()[0]).size < S * 0.8
    ats = [1, 5, 10, S]
    _close(f"ties {B}x{S}", _device(yp, yt, ats), _twin(yp.numpy(), yt.numpy(), ats), ("dcg", "mrr"))


@pytest.mark.parametrize("S", [5, 70])
def test_edge_rules(S):
    yp, yt = _inputs(4, S, seed=2)
    yt[0] = -1.0                                         # all padding
    yt[1] = 0.0                                          # no relevant item, next to slates that have some
    yt[2] = yt[2].clamp(min=0) * 0.37 + 0.25             # non-integer labels
    ats = [1, 3, S]
    got = _device(yp, yt, ats, filler_value=0.5)
    _close(f"edge {S}", got, _twin(yp.numpy(), yt.numpy(), ats, filler=0.5))
    assert (got["ndcg"][:2] == 0.5).all() and (got["dcg"][:2] == 0.0).all()
    assert (got["mrr"][1] == 1.0).all()                  # the reference's quirk: position 0 of an all-zero slate
    assert not metrics.mrr(yp[:2].cuda(), yt[:2].cuda(), ats).any().item()      # no relevant item in the whole call
    with pytest.raises(ValueError, match="cube"):
        metrics.ndcg(yp.cuda(), yt.cuda(), gain="cube")


@pytest.mark.parametrize("S", [64, 257])
def test_bits(S):
    yp, yt = (t.cuda() for t in _inputs(5, S, seed=3))
    ats, ask = [1, 5, S], {"ndcg": [5, 10], "mrr": [1]}
    for fn in (metrics.ndcg, metrics.dcg):
        many = fn(yp, yt, ats)
        assert torch.equal(fn(yp[2:3], yt[2:3], ats), many[2:3]) and torch.equal(fn(yp, yt, ats), many)
    eager = torch.stack(list(metrics.slate_metrics_device(yp, yt, ask).values()))
    ws = torch.empty(metrics.slate_workspace_bytes(5, S), dtype=torch.uint8, device="cuda")
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(g, stream=s):
        out = torch.stack(list(metrics.slate_metrics_device(yp, yt, ask, workspace=ws).values()))
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_trainer_compute_metrics():
    from oracle.ltr_head import seeded_head_weights
    from vllm_ltr_amd.ltr_head_trainer import HipLTRHeadTrainer
    B, S, ask = 3, 65, {"ndcg": [5, 10], "mrr": [1]}
    x = torch.randn(B * S, 96, generator=torch.Generator().manual_seed(5)).half().float().cuda()
    y = _inputs(B, S, seed=6)[1].cuda()
    tr = HipLTRHeadTrainer(96, {"sizes": [40], "input_norm": True, "activation": "ReLU"}, {"d_output": 1, "output_activation": None},
                           seeded_head_weights(96, [40], True, 1, 11), loss="mse")
    got = tr.compute_metrics(x, y, ask)
    assert set(got) == {"ndcg_5", "ndcg_10", "mrr_1"}
    assert got == metrics.slate_metrics(tr.to_head("f32").score(x).view(B, S), y, ask)
