"""Answer scoring without a GPU: the numpy restatement of the two rules that tests/test_score_gpu.py measures against reproduces every
g15_score_* fixture (= the reference's own functions run on the CPU) exactly; the new entry points check their arguments before launching;
the public functions keep the reference's signatures and refuse CPU tensors."""
import glob
import inspect
import os

import numpy as np
import pytest
import torch

import cti_amd
import golden_util as gu

L = cti_amd.pkg._lib
FFOE_NS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 3129)
FFOE_FIXTURES = ["g15_score_ffoe_n%d" % n for n in FFOE_NS]
MC_FIXTURES = ["g15_score_mc_g5", "g15_score_mc_g5_tail3"]


def first_argmax(x):
    """torch.max(x, 0)[1] on the CPU, spelt out: a NaN counts as the maximum, the lowest index among NaNs and among equal maxima."""
    best = 0
    for i in range(1, len(x)):
        if np.isnan(x[best]):
            break
        if np.isnan(x[i]) or x[i] > x[best]:
            best = i
    return best


def ffoe_rule(logits, labels):
    """(pred int64, per-row score, per-row upper bound, the reference's dense (rows, n) matrix)"""
    rows, n = logits.shape
    pred = np.array([first_argmax(logits[r]) for r in range(rows)], np.int64).reshape(rows)
    score = labels[np.arange(rows), pred] if rows else np.zeros(0, np.float32)
    dense = np.zeros_like(labels)
    dense[np.arange(rows), pred] = score
    return pred, score.astype(np.float32), labels.max(1), dense


def mc_rule(logits, labels):
    """(pred int64 (rows // 4,), score (rows // 4,), upper (rows,)): the comparison runs on the fp32 class-0 softmax probability."""
    x = logits.astype(np.float32)
    m = x.max(1, keepdims=True)
    e = np.exp(x - m, dtype=np.float32)
    p0 = (e[:, 0] / (e[:, 0] + e[:, 1])).astype(np.float32)
    groups = logits.shape[0] // 4
    pred = np.array([4 * g + first_argmax(p0[4 * g:4 * g + 4]) for g in range(groups)], np.int64).reshape(groups)
    return pred, labels[pred, 0], labels[:, 0].copy()


def test_every_fixture_is_listed():
    have = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(gu.GOLDEN, "g15_score_*.npz")))
    assert have == sorted(FFOE_FIXTURES + MC_FIXTURES)


@pytest.mark.parametrize("name", FFOE_FIXTURES)
def test_numpy_ffoe_rule_reproduces_the_reference(name):
    fx = gu.load(name)
    logits, labels = fx.i["logits"], fx.i["labels"]
    assert logits.shape == labels.shape == (len(fx.cfg["rows"]), fx.cfg["n"]) and 3 <= logits.shape[0] <= 7
    assert set(np.unique(labels)) <= set(np.array([0, 0.3, 0.6, 0.9, 1], np.float32))
    pred, score, upper, dense = ffoe_rule(logits, labels)
    assert np.array_equal(pred, fx.o["argmax"])
    assert np.array_equal(upper, fx.o["upper"])
    assert np.array_equal(dense, fx.o["dense"])
    assert np.array_equal(score, fx.o["dense"].sum(1))                    # one non-zero entry per row at most


def test_ffoe_fixtures_hold_the_rows_the_kernel_can_get_wrong():
    kinds, at_max, at_zero = set(), 0, 0
    for name in FFOE_FIXTURES:
        fx = gu.load(name)
        kinds |= set(fx.cfg["rows"])
        lab = fx.i["labels"][np.arange(len(fx.cfg["rows"])), fx.o["argmax"]]
        at_max += int((lab == fx.o["upper"]).sum())
        at_zero += int((lab == 0).sum())
    assert kinds == {"rand", "first", "last", "tie2", "tie3", "wtie2", "wtie3", "stride", "nan1", "nans", "neginf", "posinf2", "const"}
    assert at_max >= 10 and at_zero >= 10
    fx = gu.load("g15_score_ffoe_n3129")
    r = fx.cfg["rows"].index("stride")
    x = fx.i["logits"][r]
    assert x[100] == x[3000] == x.max() and fx.o["argmax"][r] == 100 and (x == x.max()).sum() == 2
    r = fx.cfg["rows"].index("nans")
    x = fx.i["logits"][r]
    first_nan = int(np.flatnonzero(np.isnan(x))[0])
    assert np.isnan(x).sum() == 3 and np.nanargmax(x) < first_nan == fx.o["argmax"][r]
    fx = gu.load("g15_score_ffoe_n256")
    r = fx.cfg["rows"].index("wtie3")
    assert np.array_equal(np.flatnonzero(fx.i["logits"][r] == fx.i["logits"][r].max()), [1, 128, 255]) and fx.o["argmax"][r] == 1


@pytest.mark.parametrize("name", MC_FIXTURES)
def test_numpy_mc_rule_reproduces_the_reference(name):
    fx = gu.load(name)
    logits, labels = fx.i["logits"], fx.i["labels"]
    assert logits.shape == labels.shape == (20 + fx.cfg["tail"], 2)
    pred, score, upper = mc_rule(logits, labels)
    assert np.array_equal(pred, fx.o["argmax"]) and pred.shape == (5,)
    assert np.array_equal(score, fx.o["scores"])
    assert np.array_equal(upper, fx.o["upper"]) and upper.shape == (logits.shape[0],)
    # the designed ties: saturation at 1.0f and 0.0f, and the exact 0.5 pair
    d = (logits[:, 0] - logits[:, 1]).reshape(-1)[:20].reshape(5, 4)
    g = fx.cfg["groups"]
    assert (d[g.index("sat1")] >= 20).sum() == 2 and (d[g.index("sat0")] <= -110).all() and (d[g.index("exact")] == 0).sum() == 2
    # a rule that compared x0 - x1 instead of the probability would select differently
    by_diff = np.array([4 * k + int(np.argmax(d[k])) for k in range(5)])
    assert (by_diff != pred).any()


def test_argument_errors_do_not_launch():
    lib = L.lib()
    one = 8                                                                # any non-NULL address: nothing is dereferenced before the checks
    assert lib.cti_score_rows(None, one, 4, 5, one, one, one, None, None) == -1
    assert b"NULL" in lib.cti_last_error_string()
    assert lib.cti_score_rows(one, None, 4, 5, one, one, one, None, None) == -1
    assert lib.cti_score_rows(one, one, 4, 5, None, one, one, None, None) == -1
    assert lib.cti_score_rows(one, one, 4, 5, one, None, one, None, None) == -1
    assert lib.cti_score_rows(one, one, 4, 5, one, one, None, None, None) == -1
    assert lib.cti_score_rows(one, one, 4, 0, one, one, one, None, None) == -2            # n = 0
    assert lib.cti_score_rows(one, one, -1, 5, one, one, one, None, None) == -2           # negative rows
    assert lib.cti_score_rows(one, one, 0, 5, one, one, one, None, None) == 0             # no rows: nothing to launch
    assert lib.cti_score_mc(None, one, 2, 8, one, one, one, None) == -1
    assert lib.cti_score_mc(one, None, 2, 8, one, one, one, None) == -1
    assert lib.cti_score_mc(one, one, 2, 8, None, one, one, None) == -1
    assert lib.cti_score_mc(one, one, 2, 8, one, one, None, None) == -1
    assert lib.cti_score_mc(one, one, 2, -4, one, one, one, None) == -2
    assert lib.cti_score_mc(one, one, 0, 8, one, one, one, None) == -2                   # labels without a leading dimension
    assert lib.cti_score_mc(one, one, 2, 0, None, None, one, None) == 0
    assert lib.cti_meter_add_scores(None, one, 1, one, 1, 1, None) == -1
    assert lib.cti_meter_add_scores(one, None, 1, one, 1, 1, None) == -1
    assert lib.cti_meter_add_scores(one, one, 1, None, 1, 1, None) == -1
    assert lib.cti_meter_add_scores(one, one, -1, one, 1, 1, None) == -2
    assert lib.cti_meter_add_scores(one, one, 1, one, 1, -1, None) == -2
    assert lib.cti_meter_add_scores(12, one, 1, one, 1, 1, None) == -3                     # block not 8-byte aligned
    assert lib.cti_meter_add_scalar(None, L.METER_LOSS, one, None) == -1
    assert lib.cti_meter_add_scalar(one, L.METER_LOSS, None, None) == -1
    assert lib.cti_meter_add_scalar(one, 4, one, None) == -2 and b"slot" in lib.cti_last_error_string()
    assert lib.cti_meter_add_scalar(one, -1, one, None) == -2
    assert (L.METER_SCORE, L.METER_UPPER, L.METER_LOSS, L.METER_GRAD_NORM, L.METER_BYTES) == (0, 1, 2, 3, 64)
    assert lib.cti_abi_version() == 1


def test_cpu_tensors_are_refused():
    lg, lb = torch.zeros(4, 5), torch.zeros(4, 5)
    with pytest.raises(cti_amd.CtiError):
        cti_amd.ops.score_rows(lg, lb)
    with pytest.raises(cti_amd.CtiError):
        cti_amd.ops.score_mc(torch.zeros(8, 2), torch.zeros(8, 2))
    with pytest.raises(cti_amd.CtiError):
        cti_amd.compute_score_with_logits(lg, lb)
    with pytest.raises(cti_amd.CtiError):
        cti_amd.compute_score_mc(torch.zeros(8, 2), torch.zeros(8, 2))
    with pytest.raises(cti_amd.CtiError):
        cti_amd.ScoreMeter("cpu")


def test_public_signatures_are_the_reference_s():
    def names(f):
        return list(inspect.signature(f).parameters)
    assert names(cti_amd.compute_score_with_logits) == ["logits", "labels", "ans_emb"]
    assert names(cti_amd.compute_score_mc) == ["logits", "labels"]
    assert names(cti_amd.evaluate) == names(cti_amd.evaluate_mc) == ["model", "dataloader", "args"]
    for n in ("update", "update_mc", "add_loss", "add_grad_norm", "reset", "result"):
        assert callable(getattr(cti_amd.ScoreMeter, n))
