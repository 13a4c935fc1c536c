"""Answer scoring on an MI355X (csrc/cti_score.hip through ops.score_rows / ops.score_mc and the public functions of score.py) against the
g15_score_* fixtures, which hold what the reference's own compute_score_with_logits / compute_score_mc return on the CPU.  Predictions, scores
and upper bounds are SELECTED values, so they are compared exactly; the meter's double sums are compared with float64 numpy sums."""
import collections
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils._python_dispatch import TorchDispatchMode

import cti_amd
from golden_util import load, model_case
from test_score_cpu import FFOE_FIXTURES, MC_FIXTURES, ffoe_rule, mc_rule

pytestmark = pytest.mark.gpu
DEV = "cuda"
ops = cti_amd.ops


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def row_scores(fx):
    return fx.o["dense"][np.arange(fx.o["dense"].shape[0]), fx.o["argmax"]]


@pytest.mark.parametrize("name", FFOE_FIXTURES)
def test_score_rows_equals_the_reference(name):
    fx = load(name)
    pred, score, upper = ops.score_rows(T(fx.i["logits"]), T(fx.i["labels"]))
    assert pred.dtype == torch.int64 and score.dtype == upper.dtype == torch.float32
    assert np.array_equal(N(pred), fx.o["argmax"]), (fx.cfg["rows"], N(pred), fx.o["argmax"])
    assert np.array_equal(N(score), row_scores(fx))
    assert np.array_equal(N(upper), fx.o["upper"])


@pytest.mark.parametrize("name", FFOE_FIXTURES)
def test_compute_score_with_logits_returns_the_reference_s_dense_tensor(name):
    fx = load(name)
    dense = cti_amd.compute_score_with_logits(T(fx.i["logits"]), T(fx.i["labels"]), None)
    assert dense.dtype == torch.float32 and tuple(dense.shape) == fx.o["dense"].shape
    assert np.array_equal(N(dense), fx.o["dense"])
    assert np.array_equal(N(cti_amd.compute_score_with_logits(T(fx.i["logits"]), T(fx.i["labels"]))), fx.o["dense"])     # ans_emb is optional


@pytest.mark.parametrize("name", MC_FIXTURES)
def test_score_mc_equals_the_reference(name):
    fx = load(name)
    rows = fx.i["logits"].shape[0]
    pred, score, upper = ops.score_mc(T(fx.i["logits"]), T(fx.i["labels"]))
    assert tuple(pred.shape) == tuple(score.shape) == (rows // 4,) and tuple(upper.shape) == (rows,)
    assert np.array_equal(N(pred), fx.o["argmax"]), (fx.cfg["groups"], N(pred), fx.o["argmax"])
    assert np.array_equal(N(score), fx.o["scores"])
    assert np.array_equal(N(upper), fx.o["upper"])                        # every row, the tail included
    out = cti_amd.compute_score_mc(T(fx.i["logits"]), T(fx.i["labels"]))
    assert out.dtype == torch.float32 and np.array_equal(N(out), fx.o["scores"])
    out64 = cti_amd.compute_score_mc(T(fx.i["logits"]), T(fx.i["labels"]).double())
    assert out64.dtype == torch.float64 and np.array_equal(N(out64), fx.o["scores"].astype(np.float64))
    # labels with more columns and a leading dimension of their own: only column 0 is read
    wide = torch.full((rows, 5), 7.0, device=DEV)
    wide[:, 0] = T(fx.i["labels"][:, 0])
    assert np.array_equal(N(ops.score_mc(T(fx.i["logits"]), wide[:, :3])[1]), fx.o["scores"])


@pytest.mark.parametrize("name", ["g15_score_ffoe_n3129", "g15_score_ffoe_n257"])
def test_rows_that_start_off_a_16_byte_boundary(name):
    """Row r of an (rows, 3129) array starts 12516 r bytes in; here not even row 0 is aligned, and logits and labels are misaligned differently."""
    fx = load(name)
    rows, n = fx.i["logits"].shape
    big = torch.zeros(rows + 1, n, device=DEV)
    logits = big[1:]
    logits.copy_(T(fx.i["logits"]))
    flat = torch.zeros(rows * n + 8, device=DEV)
    labels = flat[3:3 + rows * n].view(rows, n)
    labels.copy_(T(fx.i["labels"]))
    assert logits.data_ptr() % 16 == 4 and labels.data_ptr() % 16 == 12 and logits.is_contiguous() and labels.is_contiguous()
    pred, score, upper, dense = ops.score_rows(logits, labels, dense=True)
    assert np.array_equal(N(pred), fx.o["argmax"])
    assert np.array_equal(N(score), row_scores(fx))
    assert np.array_equal(N(upper), fx.o["upper"])
    assert np.array_equal(N(dense), fx.o["dense"])


def test_non_contiguous_inputs_and_an_empty_batch():
    fx = load("g15_score_ffoe_n65")
    lg = torch.zeros(7, 130, device=DEV)[:, ::2]
    lg.copy_(T(fx.i["logits"]))
    pred, score, upper = ops.score_rows(lg, T(fx.i["labels"]))
    assert np.array_equal(N(pred), fx.o["argmax"]) and np.array_equal(N(score), row_scores(fx))
    pred, score, upper = ops.score_rows(torch.zeros(0, 65, device=DEV), torch.zeros(0, 65, device=DEV))
    assert pred.numel() == score.numel() == upper.numel() == 0
    m = cti_amd.ScoreMeter(DEV)
    m.update(torch.zeros(0, 65, device=DEV), torch.zeros(0, 65, device=DEV))
    m.update_mc(torch.zeros(3, 2, device=DEV), torch.ones(3, 2, device=DEV))             # fewer than four rows: no group, three upper bounds
    assert m.result() == dict(score=0.0, upper_bound=3.0, samples=0, loss=0.0, grad_norm=0.0, updates=0)


def _meter_batches():
    fx = load("g15_score_ffoe_n65")
    lg, lb = fx.i["logits"], fx.i["labels"]
    return [(lg[:1], lb[:1]), (lg, lb), (np.tile(lg, (43, 1))[:300], np.tile(lb, (43, 1))[:300])]


def test_meter_sums_are_double_sums_and_bitwise_reproducible():
    batches = _meter_batches()
    want_s = want_u = 0.0
    results = []
    for _ in range(2):
        m = cti_amd.ScoreMeter(DEV)
        for lg, lb in batches:
            got = m.update(T(lg), T(lb))
            assert np.array_equal(N(got), ffoe_rule(lg, lb)[1])             # update returns the per-row scores
        results.append(m.result())
    want_s = sum(float(ffoe_rule(lg, lb)[1].astype(np.float64).sum()) for lg, lb in batches)
    want_u = sum(float(lb.max(1).astype(np.float64).sum()) for lg, lb in batches)
    r = results[0]
    print("meter: score %.17g (numpy %.17g)  upper %.17g (numpy %.17g)" % (r["score"], want_s, r["upper_bound"], want_u))
    assert want_s > 0 and want_u > want_s
    assert abs(r["score"] - want_s) <= 1e-11 * want_s                       # <= 1e4 additions x 2^-53 each
    assert abs(r["upper_bound"] - want_u) <= 1e-11 * want_u
    assert r["samples"] == 1 + 7 + 300 and r["updates"] == 0 and r["loss"] == 0.0 and r["grad_norm"] == 0.0
    assert results[1] == results[0]                                         # bit-identical doubles


def test_meter_scalars_add_in_order_in_double():
    vals = np.array([0.1, 2.5, 1e-3, 37.25, 3.3333333], np.float32)
    norms = np.array([7.5, 0.2, 1e4, 1e-4, 0.3], np.float32)
    m = cti_amd.ScoreMeter(DEV)
    for v, g in zip(vals, norms):
        m.add_loss(torch.tensor(float(v), device=DEV))                      # 0-dim
        m.add_grad_norm(torch.full((1,), float(g), device=DEV))             # 1-element, as FlatAdamaxDP.grad_norm
    want_l = want_g = 0.0
    for v, g in zip(vals, norms):
        want_l += float(v)
        want_g += float(g)
    r = m.result()
    assert r["loss"] == want_l and r["grad_norm"] == want_g and r["updates"] == 5
    assert r["score"] == 0.0 and r["upper_bound"] == 0.0 and r["samples"] == 0
    with pytest.raises(ValueError):
        m.add_loss(torch.zeros(2, device=DEV))
    with pytest.raises(TypeError):
        m.add_loss(torch.zeros((), device=DEV, dtype=torch.float64))
    m.update(T(_meter_batches()[1][0]), T(_meter_batches()[1][1]))
    m.reset()
    assert m.result() == dict(score=0.0, upper_bound=0.0, samples=0, loss=0.0, grad_norm=0.0, updates=0)


def test_update_captured_in_a_graph_accumulates_once_per_replay():
    fxs = [load("g15_score_ffoe_n63"), load("g15_score_ffoe_n64"), load("g15_score_ffoe_n65")]
    batches = [(fxs[0].i["logits"], fxs[0].i["labels"]), (fxs[1].i["logits"][:, :63], fxs[1].i["labels"][:, :63]),
               (fxs[2].i["logits"][:, 1:64], fxs[2].i["labels"][:, 1:64])]
    meter, eager = cti_amd.ScoreMeter(DEV), cti_amd.ScoreMeter(DEV)          # the blocks exist before the capture
    s_lg, s_lb = torch.zeros(7, 63, device=DEV), torch.zeros(7, 63, device=DEV)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        meter.update(s_lg, s_lb)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            static_score = meter.update(s_lg, s_lb)
    torch.cuda.current_stream().wait_stream(s)
    meter.reset()
    for lg, lb in batches:
        s_lg.copy_(T(lg)); s_lb.copy_(T(lb))
        g.replay()
        assert np.array_equal(N(static_score), N(eager.update(T(lg), T(lb))))
    r = meter.result()
    assert r == eager.result() and r["samples"] == 21 and r["score"] > 0


def test_meter_inside_the_captured_training_step():
    """GraphedTrainStep with a loss_fn that scores the batch and adds the loss: every replay accumulates once.  lr = 0: the parameters stay."""
    from test_dp_gpu import TinyCTI, make_batch
    cti_amd.set_precision("fp32")
    try:
        torch.manual_seed(11)
        m = TinyCTI().to(DEV)
        opt = cti_amd.FlatAdamaxDP(m, lr=0.0, clip_norm=0.25)
        meter = cti_amd.ScoreMeter(DEV)
        B = 8
        batch = tuple(t.to(DEV) for t in make_batch(B, 100))

        def loss_fn(logits, y):
            meter.update(logits, y)
            loss = nn.functional.binary_cross_entropy_with_logits(logits, y, reduction="sum") / logits.size(0)
            meter.add_loss(loss)
            return loss

        gs = cti_amd.GraphedTrainStep(m, opt, loss_fn, batch[:3], batch[3], warmup=2)
        meter.reset()                                                        # the warm-up steps ran loss_fn too
        for _ in range(3):
            loss = gs(batch[:3], batch[3])
        r = meter.result()
        with torch.no_grad():
            logits = m(*batch[:3])
        _, score, upper, _ = ffoe_rule(N(logits), N(batch[3]))
        assert r["samples"] == 3 * B and r["updates"] == 3
        assert r["score"] == 3.0 * float(score.astype(np.float64).sum())
        assert r["upper_bound"] == 3.0 * float(upper.astype(np.float64).sum())
        assert r["loss"] == 3.0 * float(loss) and r["loss"] > 0
    finally:
        cti_amd.set_precision("bf16x3")


VIEW_OPS = {"view", "_unsafe_view", "slice", "select", "detach", "alias", "expand", "as_strided", "t", "transpose", "unsqueeze", "squeeze", "reshape", "permute",
            "empty", "empty_like", "empty_strided", "new_empty", "sym_size", "sym_stride", "is_pinned", "_local_scalar_dense", "record_stream", "unbind", "split"}


class Spy(TorchDispatchMode):
    """tools/find_torch_ops.py's spy: every aten op that is not a view or an allocation."""

    def __init__(self):
        super().__init__()
        self.seen = collections.Counter()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        base = name.split(".")[1] if name.count(".") >= 1 else name
        if base not in VIEW_OPS:
            self.seen[name] += 1
        return func(*args, **(kwargs or {}))


def test_meter_updates_dispatch_no_aten_compute():
    fx, mc = load("g15_score_ffoe_n257"), load("g15_score_mc_g5_tail3")
    lg, lb, mlg, mlb = T(fx.i["logits"]), T(fx.i["labels"]), T(mc.i["logits"]), T(mc.i["labels"])
    loss = torch.tensor(1.5, device=DEV)
    m = cti_amd.ScoreMeter(DEV)
    m.update(lg, lb); m.update_mc(mlg, mlb)
    m.reset()
    with Spy() as spy:
        m.update(lg, lb)
        m.update_mc(mlg, mlb)
        m.add_loss(loss)
        m.add_grad_norm(loss)
    assert not spy.seen, dict(spy.seen)
    r = m.result()
    assert r["samples"] == 7 + 5 and r["updates"] == 1 and r["loss"] == 1.5


class _DS:
    def __init__(self, ntoken, v_dim, num_ans):
        self.dictionary = types.SimpleNamespace(ntoken=ntoken)
        self.v_dim = v_dim
        self.num_ans_candidates = num_ans


class _Loader(list):
    """A list of batch tuples with the `.dataset` the evaluation loops take the length of."""


def _build(name, builder):
    fx, p = model_case(name)
    c = fx.cfg
    m = getattr(cti_amd, builder)(types.SimpleNamespace(**c["args"]), _DS(c["ntoken"], c["v_dim"], c["num_ans"]))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, strict=True)
    return fx, m.to(DEV).eval()


def test_evaluate_follows_the_reference_loop():
    fx, m = _build("g10_ffoe_cti_step", "build_cti")
    v, q, ans, a = (torch.from_numpy(fx.i[k]) for k in ("v", "q", "ans", "target"))
    b = torch.zeros(v.shape[0], v.shape[1], 6)
    loader = _Loader((v[s], b[s], q[s], a[s], ans[s], None, None) for s in (slice(0, 2), slice(2, 5)))     # CPU batches, as a DataLoader yields them
    loader.dataset = range(7)
    args = types.SimpleNamespace(device=DEV, model="cti")
    score, bound = cti_amd.evaluate(m, loader, args)
    assert isinstance(score, float) and isinstance(bound, float)
    want_s = want_u = 0.0
    with torch.no_grad():
        for s in (slice(0, 2), slice(2, 5)):
            logits = m(v[s].to(DEV), q[s].to(DEV), ans[s].to(DEV))
            _, sc, up, _ = ffoe_rule(N(logits), a[s].numpy())
            want_s += float(sc.astype(np.float64).sum())
            want_u += float(up.astype(np.float64).sum())
    assert want_u > 0
    assert score == want_s / 7 and bound == want_u / 7
    with pytest.raises(ValueError):
        cti_amd.evaluate(m, loader, types.SimpleNamespace(device=DEV, model="mlp"))


def test_evaluate_mc_follows_the_reference_loop():
    fx, m = _build("g9_mc_cti", "build_mc_cti")
    v8, b8, q8, ans8 = (torch.from_numpy(fx.i[k]) for k in ("v", "b", "q", "ans"))
    # three images (the third: image 0 under question 1 with its own pick of candidate answers) in batches of 2 and 1
    v1 = torch.cat([v8[0::4], v8[0:1]])
    q1 = torch.cat([q8[0::4], q8[4:5]])
    ans_mc = torch.cat([ans8.view(2, 4, -1), ans8[[7, 2, 5, 0]].view(1, 4, -1)])
    a = torch.tensor([[0., 1., 0., 0.], [0., 0., 0., 1.], [1., 0., 0., 0.]])
    b1 = b8[:3]
    cuts = (slice(0, 2), slice(2, 3))
    loader = _Loader((v1[s], b1[s], q1[s], a[s], ans_mc[s], None) for s in cuts)
    loader.dataset = range(5)
    score, bound = cti_amd.evaluate_mc(m, loader, types.SimpleNamespace(device=DEV, model="cti"))
    assert isinstance(score, float) and isinstance(bound, float)
    want_s = want_u = 0.0
    with torch.no_grad():
        for s in cuts:
            k = v1[s].shape[0]
            v4 = v1[s].unsqueeze(1).expand(k, 4, v1.shape[1], v1.shape[2]).reshape(4 * k, v1.shape[1], v1.shape[2])
            q4 = q1[s].unsqueeze(1).expand(k, 4, q1.shape[1]).reshape(4 * k, q1.shape[1])
            logits, _ = m(v4.to(DEV), b1[s].to(DEV), q4.to(DEV), ans_mc[s].reshape(4 * k, -1).to(DEV))
            col = a[s].reshape(4 * k, 1)
            _, sc, up = mc_rule(N(logits), torch.cat([col, 1 - col], 1).numpy())
            want_s += float(sc.astype(np.float64).sum())
            want_u += float(up.astype(np.float64).sum())
    assert want_u == 3.0
    assert score == want_s / 5 and bound == want_u / 5
