"""The test pass and the TDIUC tallies on an MI355X (csrc/cti_predict.hip through PredictionBuffer / TypeMeter / predict) against the g16_* fixtures,
which hold what the reference's make_json / make_json_with_logits / mean_per_class produce on the CPU.  Answers and question ids are selections,
the float16 rows one correctly rounded conversion, the tallies integers: everything is compared exactly."""
import types

import numpy as np
import pytest
import torch

import cti_amd
from golden_util import load, model_case
from test_predict_cpu import PREDICT_FIXTURES, TDIUC_CASES, load_tdiuc, predict_rule, printed, tally_rule
from test_score_cpu import FFOE_FIXTURES

pytestmark = pytest.mark.gpu
DEV = "cuda"
ops = cti_amd.ops
SENTINEL16, SENTINEL64 = 0x5A5A, -0x0123456789ABCDEF


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def bits(h):
    return np.ascontiguousarray(h).view(np.uint16)


@pytest.mark.parametrize("name", PREDICT_FIXTURES)
def test_append_equals_the_reference(name):
    fx = load(name)
    rows, n = fx.i["logits"].shape
    buf = cti_amd.PredictionBuffer(rows, n, DEV)
    buf.append(T(fx.i["logits"]), T(fx.i["qids"]))
    p = buf.result()
    assert p.answers.dtype == p.question_ids.dtype == np.int64 and p.logits.dtype == np.float16 and p.logits.shape == (rows, n)
    assert np.array_equal(p.answers, fx.o["answers"]), (fx.cfg["rows"], p.answers, fx.o["answers"])
    assert np.array_equal(p.question_ids, fx.o["qids"])
    bad = np.flatnonzero(bits(p.logits).reshape(-1) != bits(fx.o["half"]).reshape(-1))
    assert bad.size == 0, [(int(i), float(fx.i["logits"].reshape(-1)[i]), hex(bits(p.logits).reshape(-1)[i]), hex(bits(fx.o["half"]).reshape(-1)[i]))
                           for i in bad[:8]]
    # question ids as a DataLoader yields them (CPU, int32 here) and without the float16 table
    buf2 = cti_amd.PredictionBuffer(rows, n, DEV, keep_logits=False)
    buf2.append(T(fx.i["logits"]), torch.from_numpy(fx.i["qids"].astype(np.int32)))
    p2 = buf2.result()
    assert p2.logits is None and np.array_equal(p2.answers, fx.o["answers"]) and np.array_equal(p2.question_ids, fx.o["qids"])


@pytest.mark.parametrize("name", FFOE_FIXTURES)
def test_append_has_the_tie_and_nan_order_of_the_scoring_kernel(name):
    fx = load(name)
    rows, n = fx.i["logits"].shape
    buf = cti_amd.PredictionBuffer(rows, n, DEV)
    buf.append(T(fx.i["logits"]), torch.arange(rows))
    p = buf.result()
    assert np.array_equal(p.answers, fx.o["argmax"]), (fx.cfg["rows"], p.answers, fx.o["argmax"])
    assert np.array_equal(p.question_ids, np.arange(rows))
    want = predict_rule(fx.i["logits"])[1]
    assert np.array_equal(np.isnan(p.logits), np.isnan(want)) and np.array_equal(bits(p.logits)[~np.isnan(want)], bits(want)[~np.isnan(want)])


def _guarded(buf):
    """Swap the buffer's tables for views of allocations one row longer, everything filled with a sentinel; returns the three allocations."""
    cap, n = buf.capacity, buf.n_answers
    half = torch.full(((cap + 1) * n,), SENTINEL16, device=DEV, dtype=torch.int16).view(torch.float16)
    ans = torch.full((cap + 1,), SENTINEL64, device=DEV, dtype=torch.int64)
    qid = torch.full((cap + 1,), SENTINEL64, device=DEV, dtype=torch.int64)
    buf._half, buf._answers, buf._qids = half[:cap * n].view(cap, n), ans[:cap], qid[:cap]
    return half, ans, qid


@pytest.mark.parametrize("n", [1, 3, 7, 9, 3129])
def test_rows_at_every_alignment_and_nothing_past_the_capacity(n):
    """Row s of the float16 table starts 2 n s bytes in: for odd n the rows start at every 2-byte residue of a 16-byte line, and the batches are slices
    of one device array, so the input rows' alignment moves as well, differently."""
    sizes = [1, 2, 3, 5, 1, 2, 3, 5]
    cap = sum(sizes)
    rs = np.random.RandomState(1700 + n)
    x = (rs.standard_normal((cap, n)) * 3.0).astype(np.float32)
    special = np.array([65520, -65520, 2.0 ** -24, 2.0 ** -25, -0.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 6.0e-5, 65519.996], np.float32)
    flat = x.reshape(-1)
    flat[rs.choice(flat.size, size=min(flat.size, 4 * special.size), replace=False)] = np.resize(special, min(flat.size, 4 * special.size))
    qids = 524291000 + 13 * np.arange(cap, dtype=np.int64)
    buf = cti_amd.PredictionBuffer(cap, n, DEV)
    half, ans, qid = _guarded(buf)
    dx, dq = T(x), T(qids)
    at = 0
    for k in sizes:
        buf.append(dx[at:at + k], dq[at:at + k])
        at += k
    assert len({(buf._half.data_ptr() + 2 * r * n) % 16 for r in range(cap)}) == 8 and len({(dx.data_ptr() + 4 * r * n) % 16 for r in range(cap)}) == 4
    p = buf.result()
    want_ans, want_half = predict_rule(x)
    assert np.array_equal(p.answers, want_ans) and np.array_equal(p.question_ids, qids)
    assert np.array_equal(bits(p.logits), bits(want_half))
    assert (bits(half.cpu().numpy())[cap * n:] == SENTINEL16).all()
    assert ans[cap].item() == SENTINEL64 and qid[cap].item() == SENTINEL64


def test_capacity_is_enforced_on_the_device():
    n = 9
    rs = np.random.RandomState(1710)
    x = (rs.standard_normal((12, n)) * 3.0).astype(np.float32)
    dx, dq = T(x), T(100 + np.arange(12, dtype=np.int64))
    buf = cti_amd.PredictionBuffer(5, n, DEV)
    half, ans, qid = _guarded(buf)
    buf.append(dx[:3], dq[:3])
    buf.append(dx[3:5], dq[3:5])                                            # fits exactly
    p = buf.result()
    assert len(p) == 5 and np.array_equal(p.answers, predict_rule(x[:5])[0]) and np.array_equal(p.question_ids, 100 + np.arange(5))
    before = (half.clone(), ans.clone(), qid.clone())
    buf.append(dx[5:6], dq[5:6])                                            # one row too many
    assert buf._state.cpu().tolist() == [5, 1, 5, n]                        # the cursor stays, the overflow word is set
    assert torch.equal(half.view(torch.int16), before[0].view(torch.int16)) and torch.equal(ans, before[1]) and torch.equal(qid, before[2])
    with pytest.raises(cti_amd.CtiError, match="capacity 5"):
        buf.result()
    buf.reset()
    assert len(buf.result()) == 0
    # an append that fits only in part writes nothing at all, and the flag is sticky: a later append that would fit is dropped too
    buf.append(dx[6:9], dq[6:9])
    before = (half.clone(), ans.clone(), qid.clone())
    buf.append(dx[:4], dq[:4])
    buf.append(dx[9:10], dq[9:10])
    assert buf._state.cpu().tolist() == [3, 1, 5, n]
    assert torch.equal(half.view(torch.int16), before[0].view(torch.int16)) and torch.equal(ans, before[1]) and torch.equal(qid, before[2])
    with pytest.raises(cti_amd.CtiError):
        buf.result()
    buf.reset()
    buf.append(dx[10:12], dq[10:12])
    p = buf.result()
    assert np.array_equal(p.answers, predict_rule(x[10:12])[0]) and np.array_equal(p.question_ids, [110, 111])
    with pytest.raises(ValueError):
        buf.append(torch.zeros(2, n + 1, device=DEV), dq[:2])
    with pytest.raises(TypeError):
        buf.append(dx[:2], torch.zeros(2, device=DEV))


def test_appends_captured_in_a_graph_land_behind_each_other_at_every_replay():
    n = 65
    rs = np.random.RandomState(1720)
    x = (rs.standard_normal((15, n)) * 3.0).astype(np.float32)
    qids = 524291000 + 7 * np.arange(15, dtype=np.int64)
    buf = cti_amd.PredictionBuffer(15, n, DEV)                              # everything exists before the capture
    s_a, s_b = torch.zeros(2, n, device=DEV), torch.zeros(3, n, device=DEV)
    s_qa, s_qb = torch.zeros(2, device=DEV, dtype=torch.int64), torch.zeros(3, device=DEV, dtype=torch.int64)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        buf.append(s_a, s_qa)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            buf.append(s_a, s_qa)
            buf.append(s_b, s_qb)
    torch.cuda.current_stream().wait_stream(s)
    buf.reset()
    for k in range(3):
        lo = 5 * k
        s_a.copy_(T(x[lo:lo + 2])); s_qa.copy_(T(qids[lo:lo + 2]))
        s_b.copy_(T(x[lo + 2:lo + 5])); s_qb.copy_(T(qids[lo + 2:lo + 5]))
        g.replay()
    p = buf.result()
    want_ans, want_half = predict_rule(x)
    assert len(p) == 15 and np.array_equal(p.question_ids, qids) and np.array_equal(p.answers, want_ans)
    assert np.array_equal(bits(p.logits), bits(want_half))


def _cuts(rows):
    a, b = rows // 5, rows // 5 + (rows + 1) // 2
    return [(0, a), (a, b), (b, rows)]


@pytest.mark.parametrize("case", TDIUC_CASES)
def test_type_meter_equals_the_reference(case):
    c = load_tdiuc(case)
    Tn = len(c.type_names)
    meter = cti_amd.TypeMeter(c.type_names, c.K, DEV)
    for lo, hi in _cuts(len(c.pred)):                                       # three uneven updates; CPU and device tensors, int64 and int32
        meter.update(T(c.pred[lo:hi]), torch.from_numpy(c.gt[lo:hi]), torch.from_numpy(c.qtype[lo:hi].astype(np.int32)))
    table, invalid = meter.table()
    assert invalid == 0 and np.array_equal(table, tally_rule(c.pred, c.gt, c.qtype, Tn, c.K))
    assert printed(meter.result()) == c.o
    # the model's label indices through a label_to_key table: a non-identity permutation, three labels outside the key
    rs = np.random.RandomState(1730)
    n_labels = c.K + 3
    lut = np.full(n_labels, -1, np.int64)
    key_labels = rs.permutation(n_labels)[:c.K]                             # label key_labels[k] is key answer k
    lut[key_labels] = np.arange(c.K)
    outside = np.flatnonzero(lut < 0)
    assert len(outside) == 3 and not np.array_equal(lut[:c.K], np.arange(c.K))
    labels = key_labels[c.pred]
    labels[::7] = outside[np.arange(len(labels[::7])) % 3]                  # some answers the key does not hold: never correct
    m2 = cti_amd.TypeMeter(c.type_names, c.K, DEV, label_to_key=lut)
    for lo, hi in _cuts(len(c.pred)):
        m2.update(T(labels[lo:hi]), T(c.gt[lo:hi]), T(c.qtype[lo:hi]))
    t2, invalid = m2.table()
    want = tally_rule(labels, c.gt, c.qtype, Tn, c.K, lut)
    assert invalid == 0 and np.array_equal(t2, want)
    assert np.array_equal(t2[:, :, 0], table[:, :, 0]) and (t2[:, :, 1] <= table[:, :, 1]).all()
    m2.reset()
    assert m2.table()[0].sum() == 0


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257])
def test_type_tally_row_counts(rows):
    rs = np.random.RandomState(1740 + rows)
    Tn, K = 3, 4
    gt, qtype = rs.randint(-1, K, rows), rs.randint(0, Tn, rows)
    pred = np.where(rs.rand(rows) < 0.5, np.maximum(gt, 0), rs.randint(0, K, rows))
    meter = cti_amd.TypeMeter(["a", "b", "c"], K, DEV)
    meter.update(T(pred), T(gt), T(qtype))
    table, invalid = meter.table()
    assert invalid == 0 and np.array_equal(table, tally_rule(pred, gt, qtype, Tn, K)) and table[:, :, 0].sum() == rows
    assert meter.result()["samples"] == rows


def test_rows_out_of_range_are_counted_apart():
    Tn, K = 3, 4
    pred, gt, qtype = np.array([1, 2, 3, 0, 1]), np.array([1, -1, 3, 0, 2]), np.array([0, 1, 2, 2, 1])
    for what, row in (("qtype", (1, 1, Tn)), ("qtype", (1, 1, -1)), ("gt", (1, K, 0)), ("gt", (1, -2, 0)), ("pred", (K, 1, 0)), ("pred", (-1, 1, 0))):
        meter = cti_amd.TypeMeter(["a", "b", "c"], K, DEV)
        p, g, t = (np.concatenate([a[:2], [r], a[2:]]) for a, r in zip((pred, gt, qtype), row))
        meter.update(T(p), T(g), T(t))
        table, invalid = meter.table()
        assert invalid == 1 and np.array_equal(table, tally_rule(pred, gt, qtype, Tn, K)), what     # the other rows are tallied, this one nowhere
        with pytest.raises(cti_amd.CtiError, match="1 rows"):
            meter.result()
    lut = np.array([0, 1, 2, 3, K, -1], np.int64)                           # label 4 maps outside the key: invalid; label 5 is not in the key: a miss
    meter = cti_amd.TypeMeter(["a", "b", "c"], K, DEV, label_to_key=lut)
    meter.update(T(np.array([4, 5, 6, 1])), T(np.array([1, 1, 1, 1])), T(np.array([0, 0, 0, 0])))
    table, invalid = meter.table()
    assert invalid == 2 and table[0, 2].tolist() == [2, 1] and table.sum() == 3


class _DS:
    def __init__(self, ntoken, v_dim, num_ans, length):
        self.dictionary = types.SimpleNamespace(ntoken=ntoken)
        self.v_dim = v_dim
        self.num_ans_candidates = num_ans
        self.length = length

    def __len__(self):
        return self.length


class _Loader(list):
    """A list of batch tuples with the `.dataset` the test pass takes the capacity and the answer count from."""


@pytest.mark.parametrize("name,builder,model", [("g9_ffoe_cti", "build_cti", "cti"), ("g9_ffoe_ban", "build_ban", "ban")])
def test_predict_follows_the_reference_loop(name, builder, model):
    fx, p = model_case(name)
    c = fx.cfg
    ds = _DS(c["ntoken"], c["v_dim"], c["num_ans"], c["B"])
    m = getattr(cti_amd, builder)(types.SimpleNamespace(**c["args"]), ds)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, strict=True)
    m = m.to(DEV).eval()
    v, q = torch.from_numpy(fx.i["v"]), torch.from_numpy(fx.i["q"])
    b = torch.from_numpy(fx.i["b"]) if "b" in fx.i else torch.zeros(v.shape[0], v.shape[1], 6)
    ans = torch.from_numpy(fx.i["ans"]) if "ans" in fx.i else torch.zeros(v.shape[0], 3, dtype=torch.int64)
    qids = torch.tensor([524291003, 524291001, 262148000, 262148002, 393225001])     # int64 on the CPU, as a DataLoader yields them
    cuts = (slice(0, 1), slice(1, 4), slice(4, 5))
    loader = _Loader((v[s], b[s], q[s], None, ans[s], qids[s], None) for s in cuts)
    loader.dataset = ds
    args = types.SimpleNamespace(device=DEV, model=model)
    got = cti_amd.predict(args, m, loader)
    rows = []
    with torch.no_grad():
        for s in cuts:
            out = m(v[s].to(DEV), b[s].to(DEV), q[s].to(DEV), None)[0] if model == "ban" else m(v[s].to(DEV), q[s].to(DEV), ans[s].to(DEV))
            rows.append(out.float().cpu().numpy())
    want_ans, want_half = predict_rule(np.concatenate(rows))
    assert len(got) == c["B"] and np.array_equal(got.question_ids, qids.numpy())
    assert np.array_equal(got.answers, want_ans) and np.array_equal(bits(got.logits), bits(want_half))
    assert np.array_equal(want_ans, predict_rule(fx.o["logits"])[0])        # and the answers are the reference model's
    lean = cti_amd.predict(args, m, loader, device=torch.device(DEV), keep_logits=False)
    assert lean.logits is None and np.array_equal(lean.answers, want_ans) and np.array_equal(lean.question_ids, qids.numpy())
    js = got.to_json(["answer %d" % k for k in range(c["num_ans"])])
    assert js[2] == {"question_id": 262148000, "answer": "answer %d" % want_ans[2]}
    assert sorted(got.teacher_logits()) == sorted(int(x) for x in qids)
    with pytest.raises(ValueError):
        cti_amd.predict(types.SimpleNamespace(device=DEV, model="mlp"), m, loader)
