"""The test pass and the TDIUC metric without a GPU: the numpy restatements that tests/test_predict_gpu.py measures against reproduce every g16_*
fixture (= the reference's own make_json / make_json_with_logits / mean_per_class run on the CPU) exactly; tdiuc_summary on the restated table
prints the reference's figures; the new entry points check their arguments before launching; the public classes refuse CPU devices."""
import glob
import json
import os
import types

import numpy as np
import pytest
import torch

import cti_amd
import golden_util as gu
from test_score_cpu import first_argmax

L = cti_amd.pkg._lib
PREDICT_NS = (1, 2, 7, 8, 9, 65, 257, 3129)
PREDICT_FIXTURES = ["g16_predict_n%d" % n for n in PREDICT_NS]
TDIUC_CASES = ["small", "wide", "onecell", "allmiss"]


def predict_rule(logits):
    """(answers int64, float16 rows): the arg-max on the fp32 values, numpy's round-to-nearest-even conversion."""
    rows = logits.shape[0]
    with np.errstate(over="ignore"):                                       # 65520 and beyond become inf: what is wanted
        half = logits.astype(np.float16)
    return np.array([first_argmax(logits[r]) for r in range(rows)], np.int64).reshape(rows), half


def same_halves(a, b):
    """bit for bit, NaNs by position (numpy and the device agree on every other bit pattern, and on the NaNs' too: checked on the GPU)"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.dtype == b.dtype == np.float16 and a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a.view(np.uint16)[~nan], b.view(np.uint16)[~nan])


def load_tdiuc(case):
    with open(os.path.join(gu.GOLDEN, "g16_tdiuc_%s.json" % case)) as f:
        d = json.load(f)
    i = d["i"]
    return types.SimpleNamespace(pred=np.array(i["pred"], np.int64), gt=np.array(i["gt"], np.int64), qtype=np.array(i["qtype"], np.int64),
                                 type_names=i["type_names"], K=i["K"], o=d["o"])


def tally_rule(pred, gt, qtype, T, K, lut=None):
    """The (T, K + 1, 2) table of the tally kernel in numpy."""
    table = np.zeros((T, K + 1, 2), np.int64)
    p = pred if lut is None else lut[pred]
    np.add.at(table, (qtype, gt + 1, 0), 1)
    hit = (gt >= 0) & (p == gt)
    np.add.at(table, (qtype[hit], gt[hit] + 1, 1), 1)
    return table


def printed(summary):
    """tdiuc_summary's dict in the shape and the %.2f format of the fixtures' parsed print-out"""
    def section(s, overall):
        return {"per_type": {k: "%.2f" % v for k, v in s["per_type"].items()}, "arithmetic": "%.2f" % s["arithmetic_mpt"],
                "harmonic": "%.2f" % s["harmonic_mpt"], "overall": "%.2f" % overall}
    return {"not_found": summary["not_found"], "plain": section(summary, summary["overall"]),
            "normalized": section(summary["normalized"], summary["overall"])}


def test_every_fixture_is_listed():
    have = sorted(os.path.basename(p) for p in glob.glob(os.path.join(gu.GOLDEN, "g16_*")))
    assert have == sorted([n + ".npz" for n in PREDICT_FIXTURES] + ["g16_tdiuc_%s.json" % c for c in TDIUC_CASES])
    for p in glob.glob(os.path.join(gu.GOLDEN, "g16_*")):
        assert os.path.getsize(p) < 200 * 1024


@pytest.mark.parametrize("name", PREDICT_FIXTURES)
def test_numpy_predict_rule_reproduces_the_reference(name):
    fx = gu.load(name)
    logits, qids = fx.i["logits"], fx.i["qids"]
    assert logits.dtype == np.float32 and logits.shape == (len(fx.cfg["rows"]), fx.cfg["n"]) and 5 <= logits.shape[0] <= 9
    assert qids.dtype == np.int64 and qids.min() > 2 ** 31 // 8 and (np.diff(qids) > 1).all()
    answers, half = predict_rule(logits)
    assert np.array_equal(answers, fx.o["answers"]) and fx.o["answers"].dtype == np.int64
    assert same_halves(half, fx.o["half"])
    assert np.array_equal(fx.o["qids"], qids)


def test_predict_fixtures_hold_the_values_the_conversion_can_get_wrong():
    seen = set()
    for name in PREDICT_FIXTURES:
        fx = gu.load(name)
        seen |= set(fx.cfg["rows"])
        pairs = {}
        for x, h in zip(fx.i["logits"].reshape(-1), fx.o["half"].reshape(-1).view(np.uint16)):
            pairs[np.float32(x).view(np.uint32).item()] = int(h)
        f = lambda v: np.float32(v).view(np.uint32).item()
        want = {f(1 + 2.0 ** -11): 0x3c00, f(1 + 3 * 2.0 ** -11): 0x3c02,                        # ties to even: down, up
                f(65504): 0x7bff, f(65519.996): 0x7bff, f(65520): 0x7c00, f(-65520): 0xfc00,      # overflow from 65520 upward
                f(2.0 ** -24): 0x0001, f(2.0 ** -25): 0x0000, f(2.0 ** -25 * (1 + 2.0 ** -23)): 0x0001, f(3 * 2.0 ** -25): 0x0002,
                f(-0.0): 0x8000, f(np.inf): 0x7c00, f(-np.inf): 0xfc00}
        if fx.cfg["n"] >= 32:
            for k, v in want.items():
                assert pairs[k] == v, (name, hex(k), hex(pairs[k]), hex(v))
        else:
            assert all(pairs[k] == v for k, v in want.items() if k in pairs)
        r = fx.cfg["rows"].index("halftie") if "halftie" in fx.cfg["rows"] else None
        if r is not None:
            x, h = fx.i["logits"][r], fx.o["half"][r]
            a = int(fx.o["answers"][r])
            first_of_rounded = int(np.flatnonzero(h == h.max())[0])
            assert (h == h.max()).sum() == 2 and first_of_rounded < a and x[a] > x[first_of_rounded]   # an arg-max after the rounding is wrong
        if "nan" in fx.cfg["rows"]:
            r = fx.cfg["rows"].index("nan")
            assert np.isnan(fx.i["logits"][r][fx.o["answers"][r]]) and np.nanargmax(fx.i["logits"][r]) != fx.o["answers"][r]
    assert seen == {"all", "noinf", "ordinary", "nan", "halftie", "subn", "neg", "seq"}


@pytest.mark.parametrize("case", TDIUC_CASES)
def test_tdiuc_summary_prints_the_reference_s_figures(case):
    c = load_tdiuc(case)
    T = len(c.type_names)
    assert c.pred.shape == c.gt.shape == c.qtype.shape and (c.gt == -1).any() == (case != "onecell")
    table = tally_rule(c.pred, c.gt, c.qtype, T, c.K)
    assert table[:, :, 0].sum() == len(c.pred) and (table[:, 0, 1] == 0).all()
    s = cti_amd.tdiuc_summary(table, c.type_names)
    assert printed(s) == c.o
    assert s["samples"] == len(c.pred) and s["not_found"] == int((c.gt == -1).sum())
    assert set(s["per_type"]) == set(c.type_names[t] for t in np.unique(c.qtype))              # types without a sample are left out
    if case == "allmiss":
        assert s["overall"] == 0.0 and 0 < s["harmonic_mpt"] < 1e-9 and 0 < s["arithmetic_mpt"] < 1e-9      # eps alone
    if case == "wide":
        assert len(s["per_type"]) == 11 and T == 12 and table.shape == (12, 1481, 2) and table[:, 1480].sum() > 0
    # the same table through a label_to_key permutation of the predictions
    rs = np.random.RandomState(3)
    perm = rs.permutation(c.K)
    lut = np.empty(c.K, np.int64)
    lut[perm] = np.arange(c.K)                                               # model label perm[k] is key answer k
    assert np.array_equal(tally_rule(perm[c.pred], c.gt, c.qtype, T, c.K, lut), table)


def test_tdiuc_summary_by_hand():
    # type a: truths {0: 3 seen 2 hit, 1: 1 seen 0 hit, -1: 1 seen}; type b: no sample; type c: truth 1: 4 seen 4 hit
    table = np.zeros((3, 3, 2), np.int64)
    table[0, 1] = (3, 2); table[0, 2] = (1, 0); table[0, 0] = (1, 0); table[2, 2] = (4, 4)
    s = cti_amd.tdiuc_summary(table, ["a", "b", "c"])
    assert s["per_type"] == {"a": 100 * (2 / 5), "c": 100.0}
    assert s["normalized"]["per_type"] == {"a": 100 * (2 / 3 + 0 + 0) / 3, "c": 100.0}
    eps = 1e-10
    assert abs(s["arithmetic_mpt"] - (70.0 + eps)) < 1e-12
    assert abs(s["harmonic_mpt"] - 2 / (1 / (40.0 + eps) + 1 / (100.0 + eps))) < 1e-12
    assert s["overall"] == 100 * (6 / 9) and s["not_found"] == 1 and s["samples"] == 9
    with pytest.raises(ValueError):
        cti_amd.tdiuc_summary(np.zeros((3, 3, 2), np.int64), ["a", "b", "c"])
    with pytest.raises(ValueError):
        cti_amd.tdiuc_summary(table, ["a", "b"])


def test_tdiuc_tables_by_hand():
    ann = [{"question_id": 11, "question_type": "color", "answers": [{"answer": "red"}]},
           {"question_id": 7, "question_type": "absurd", "answers": [{"answer": "doesnotapply"}]},
           {"question_id": 29, "question_type": "color", "answers": [{"answer": "mauve"}]},             # not in the key
           {"question_id": 3, "question_type": "counting", "answers": [{"answer": "two"}, {"answer": "ignored"}]}]
    answerkey = {"doesnotapply": "0", "red": "1", "two": "2", "yes": "3"}                           # the csv gives strings
    label2ans = ["yes", "two", "teal", "red", "doesnotapply"]
    names, per_q, lut = cti_amd.tdiuc_tables(ann, answerkey, label2ans)
    assert names == ["absurd", "color", "counting"]
    assert per_q == {11: (1, 1), 7: (0, 0), 29: (1, -1), 3: (2, 2)}
    assert lut.dtype == np.int64 and lut.tolist() == [3, 2, -1, 1, 0]


def test_argument_errors_do_not_launch():
    lib = L.lib()
    one = 8                                                                # any non-NULL, 8-byte aligned address: nothing is dereferenced before the checks
    assert lib.cti_predict_rows(None, one, 4, 5, one, one, one, one, None) == -1
    assert b"NULL" in lib.cti_last_error_string()
    assert lib.cti_predict_rows(one, None, 4, 5, one, one, one, one, None) == -1
    assert lib.cti_predict_rows(one, one, 4, 5, None, one, one, one, None) == -1
    assert lib.cti_predict_rows(one, one, 4, 5, one, None, one, one, None) == -1
    assert lib.cti_predict_rows(one, one, 4, 5, one, one, None, one, None) == -1
    assert lib.cti_predict_rows(one, one, 4, 0, one, one, one, one, None) == -2            # n = 0
    assert lib.cti_predict_rows(one, one, -1, 5, one, one, one, one, None) == -2           # negative rows
    assert lib.cti_predict_rows(one, one, 2 ** 31, 5, one, one, one, one, None) == -2      # more rows than a grid has workgroups
    assert lib.cti_predict_rows(one, one, 4, 5, 12, one, one, one, None) == -3             # state block not 8-byte aligned
    assert lib.cti_predict_rows(one, one, 4, 5, one, one, one, 9, None) == -3              # float16 table at an odd address
    assert lib.cti_predict_rows(one, one, 0, 5, one, one, one, None, None) == 0            # no rows: nothing to launch; the float16 table is optional
    assert lib.cti_predict_advance(None, 4, None) == -1
    assert lib.cti_predict_advance(one, -4, None) == -2
    assert lib.cti_predict_advance(12, 4, None) == -3
    assert lib.cti_predict_advance(one, 0, None) == 0
    assert lib.cti_type_tally(None, None, 0, one, one, 4, 3, 5, one, one, None) == -1
    assert lib.cti_type_tally(one, None, 0, None, one, 4, 3, 5, one, one, None) == -1
    assert lib.cti_type_tally(one, None, 0, one, None, 4, 3, 5, one, one, None) == -1
    assert lib.cti_type_tally(one, None, 0, one, one, 4, 3, 5, None, one, None) == -1
    assert lib.cti_type_tally(one, None, 0, one, one, 4, 3, 5, one, None, None) == -1
    assert lib.cti_type_tally(one, None, 0, one, one, -1, 3, 5, one, one, None) == -2
    assert lib.cti_type_tally(one, None, 0, one, one, 4, 0, 5, one, one, None) == -2      # no types
    assert lib.cti_type_tally(one, None, 0, one, one, 4, 3, 0, one, one, None) == -2      # no key answers
    assert lib.cti_type_tally(one, one, 0, one, one, 4, 3, 5, one, one, None) == -2       # a lut of no labels
    assert lib.cti_type_tally(one, None, 0, one, one, 4, 3, 5, 12, one, None) == -3
    assert lib.cti_type_tally(one, None, 0, one, one, 0, 3, 5, one, one, None) == 0
    assert (L.PREDICT_CURSOR, L.PREDICT_OVERFLOW, L.PREDICT_CAPACITY, L.PREDICT_N, L.PREDICT_STATE_BYTES) == (0, 1, 2, 3, 32)
    assert lib.cti_abi_version() == 1


class _Loader(list):
    pass


def test_cpu_devices_are_refused():
    with pytest.raises(cti_amd.CtiError):
        cti_amd.PredictionBuffer(8, 5, "cpu")
    with pytest.raises(cti_amd.CtiError):
        cti_amd.TypeMeter(["a", "b"], 4, "cpu")
    loader = _Loader()
    loader.dataset = type("DS", (list,), {"num_ans_candidates": 5})([0, 1, 2])
    with pytest.raises(cti_amd.CtiError):
        cti_amd.predict(types.SimpleNamespace(model="cti", device="cpu"), None, loader)
    with pytest.raises(cti_amd.CtiError):
        cti_amd.predict(types.SimpleNamespace(model="cti", device="cuda"), None, loader, device=torch.device("cpu"))
    with pytest.raises(cti_amd.CtiError):
        cti_amd.ops.predict_rows(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64), torch.zeros(4, dtype=torch.int64),
                                 torch.zeros(8, dtype=torch.int64), torch.zeros(8, dtype=torch.int64))
    with pytest.raises(cti_amd.CtiError):
        cti_amd.ops.type_tally(torch.zeros(25, dtype=torch.int64), 2, 5, torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64),
                               torch.zeros(2, dtype=torch.int64))


@pytest.mark.parametrize("name", ["g16_predict_n9", "g16_predict_n257"])
def test_predictions_give_the_reference_s_json_and_teacher_logits(name):
    """The fixtures hold make_json's output for label2ans = the identity and make_json_with_logits' vectors in order."""
    fx = gu.load(name)
    n = fx.cfg["n"]
    p = cti_amd.Predictions(fx.i["qids"], fx.o["answers"], fx.o["half"])
    assert len(p) == len(fx.i["qids"])
    js = p.to_json(list(range(n)))
    assert js == [{"question_id": int(q), "answer": int(a)} for q, a in zip(fx.o["qids"], fx.o["answers"])]
    assert all(type(e["question_id"]) is int for e in js)
    names = ["answer %d" % k for k in range(n)]
    assert [e["answer"] for e in p.to_json(names)] == [names[a] for a in fx.o["answers"]]
    json.dumps(p.to_json(names))                                           # serialisable as it stands
    t = p.teacher_logits()
    assert list(t) == [int(q) for q in fx.o["qids"]] and all(type(k) is int for k in t)
    for r, q in enumerate(fx.o["qids"]):
        assert same_halves(t[int(q)], fx.o["half"][r]) and t[int(q)].shape == (n,)
    # what teacher_logits.py reads back: float32 rows for the distillation loss
    batch = cti_amd.pkg.teacher_logit_batch(t, fx.o["qids"][:2])
    assert batch.dtype == torch.float32 and tuple(batch.shape) == (2, n)
    with pytest.raises(ValueError):
        cti_amd.Predictions(fx.i["qids"], fx.o["answers"]).teacher_logits()
