"""ltr_order_agreement (csrc/ltr_metrics.hip, vllm_ltr_amd/metrics.py): the pair counts of Kendall's tau-b and the gaps of the
discordant pairs, against a plain numpy count over np.triu_indices and against scipy.stats.kendalltau (train/trainer.py:195).
Counts are integers and the gaps single f32 operations: compared exactly."""
import functools

import numpy as np
import pytest
import torch
from scipy.stats import kendalltau

from vllm_ltr_amd import _lib

pytestmark = pytest.mark.gpu

# wave and workgroup edges, the 1024 tile edge, three tiles with an off-diagonal workgroup whose J tile has one element
SIZES = [0, 1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2049]
FAMILIES = ["tied", "same", "reverse", "independent"]
COUNTS = ("concordant", "discordant", "tie_x", "tie_y", "tie_xy", "unordered")


def reference(x, y):
    i, j = np.triu_indices(len(x), 1)                      # row-major: the first maximum is the smallest (i, j)
    with np.errstate(invalid="ignore"):
        dx, dy = x[i] - x[j], y[i] - y[j]                  # f32
    nan = np.isnan(x[i]) | np.isnan(x[j]) | np.isnan(y[i]) | np.isnan(y[j])
    sx, sy = np.sign(dx), np.sign(dy)
    disc = ~nan & (sx * sy < 0)
    out = dict(concordant=(~nan & (sx * sy > 0)).sum(), discordant=disc.sum(), tie_x=(~nan & (sx == 0) & (sy != 0)).sum(),
               tie_y=(~nan & (sx != 0) & (sy == 0)).sum(), tie_xy=(~nan & (sx == 0) & (sy == 0)).sum(), unordered=nan.sum(),
               max_gap_x=np.float32(0), max_gap_y=np.float32(0), gap_i=-1, gap_j=-1)
    if disc.any():
        gx = np.where(disc, np.abs(dx), np.float32(-1))
        k = int(np.argmax(gx))
        out.update(max_gap_x=gx[k], max_gap_y=np.abs(dy)[disc].max(), gap_i=int(i[k]), gap_j=int(j[k]))
    return out


@functools.lru_cache(maxsize=None)
def case(family, n):
    r = np.random.RandomState(1000 + n)
    if family == "tied":
        x = r.randint(0, 40, n).astype(np.float32)
        y = np.rint(x + r.normal(0, 8, n)).astype(np.float32)
        x[:2] = np.array([0.0, -0.0], np.float32)[:n]
    else:
        x = r.permutation(n).astype(np.float32)
        y = {"same": x, "reverse": x[::-1].copy(), "independent": r.permutation(n).astype(np.float32)}[family]
    return x, y, reference(x, y)


def run(x, y):
    from vllm_ltr_amd.metrics import order_agreement
    return order_agreement(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())


def assert_matches(got, want):
    for k in COUNTS + ("gap_i", "gap_j"):
        assert getattr(got, k) == int(want[k]), (k, getattr(got, k), want[k])
    assert np.float32(got.max_gap_x) == want["max_gap_x"] and np.float32(got.max_gap_y) == want["max_gap_y"]
    assert sum(getattr(got, k) for k in COUNTS) == got.pairs


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", FAMILIES)
def test_counts_and_gaps_are_exact(family, n):
    x, y, want = case(family, n)
    got = run(x, y)
    assert got.pairs == n * (n - 1) // 2
    assert_matches(got, want)


@pytest.mark.parametrize("n", [n for n in SIZES if n >= 2])
@pytest.mark.parametrize("family", FAMILIES)
def test_tau_b_matches_scipy(family, n):
    x, y, _ = case(family, n)
    got, want = run(x, y).tau_b, kendalltau(x, y)[0]
    assert abs(got - want) <= 1e-12 or (np.isnan(got) and np.isnan(want))       # (n = 2, tied: x is +0, -0 - constant)


def test_tau_b_of_a_constant_vector_is_nan():
    x, y, _ = case("tied", 257)
    from vllm_ltr_amd.metrics import kendall_tau
    assert np.isnan(kendalltau(np.zeros_like(x), y)[0])
    assert np.isnan(kendall_tau(torch.zeros(257, device="cuda"), torch.from_numpy(y).cuda()))


def test_nan_is_unordered_and_infinities_are_ordered():
    x, y, _ = case("tied", 257)
    x, y = x.copy(), y.copy()
    x[5], y[10], y[200] = np.nan, np.inf, -np.inf
    got = run(x, y)
    assert got.unordered == 256 and np.isnan(got.tau_b)
    assert_matches(got, reference(x, y))


def test_result_is_reproducible_and_capture_safe():
    from vllm_ltr_amd.metrics import RESULT_BYTES, order_agreement_device, workspace_bytes
    x, y, want = case("tied", 2049)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    raw = lambda t: bytes(t.cpu().numpy())
    eager = raw(order_agreement_device(xd, yd))
    assert raw(order_agreement_device(xd, yd)) == eager
    out = torch.zeros(RESULT_BYTES, dtype=torch.uint8, device="cuda")
    ws = torch.empty(workspace_bytes(2049), dtype=torch.uint8, device="cuda")
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(g, stream=s):
        order_agreement_device(xd, yd, out, ws)
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert raw(out) == eager
    from vllm_ltr_amd.metrics import OrderAgreement
    assert_matches(OrderAgreement.from_bytes(eager), want)


def test_argument_errors_by_return_code():
    lib = _lib.load()
    x = torch.zeros(2049, device="cuda")
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    need = lib.ltr_order_agreement_workspace_bytes(2049)
    assert need == 6 * 64 and lib.ltr_order_agreement_workspace_bytes((1 << 20) + 1) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    call = lambda xp, n, nbytes: lib.ltr_order_agreement(xp, x.data_ptr(), n, out.data_ptr(), ws.data_ptr(), nbytes, None)
    assert call(x.data_ptr(), 2049, need - 1) == _lib.LTR_E_INVAL and b"workspace" in lib.ltr_last_error()
    assert call(x.data_ptr(), (1 << 20) + 1, need) == _lib.LTR_E_INVAL
    assert call(None, 2049, need) == _lib.LTR_E_INVAL
    assert call(x.data_ptr(), -1, need) == _lib.LTR_E_INVAL


def test_trainer_evaluate_matches_scipy_on_the_predictions():
    from vllm_ltr_amd.opt_spec import OPTSpec, seeded_checkpoint
    from vllm_ltr_amd.scorer import HipOPTScorer
    from vllm_ltr_amd.trainer import HipPredictorTrainer, len2label
    spec = OPTSpec.tiny_pre_ln()
    tr = HipPredictorTrainer(spec, seeded_checkpoint(spec, 78), "cuda:0", loss="listMLE")
    r = np.random.RandomState(0)
    test = [([2] + r.randint(40, spec.vocab_size, r.randint(2, 30)).tolist(), float(len2label(int(r.randint(4, 36)) * 20, 1024, 1)))
            for _ in range(40)]                                            # 40 examples in slates of 16: 16 + 16 + 8, tied labels
    rec = tr.evaluate(test, batch_size=16)
    preds = np.concatenate([tr.predict(*HipOPTScorer.pack([t[0] for t in test[b:b + 16]]))[:, 0] for b in range(0, 40, 16)])
    assert abs(rec["kendall_tau"] - kendalltau([t[1] for t in test], preds)[0]) <= 1e-12
    assert rec["pairs"] == 40 * 39 // 2 and rec["concordant"] + rec["discordant"] <= rec["pairs"]
    tr.close()
