"""Predictions on the device: the reference's test pass (src/FFOE/test.py:78-130: `get_logits`, `make_json`, `make_json_with_logits`) and its TDIUC metric
(src/evaluate_TDIUC.py:26-94: `mean_per_class`) on the kernels of csrc/cti_predict.hip.

The reference copies every batch of logits to the host (`pred[idx:idx+B].copy_(logits)`, a blocking copy per batch) and then takes one host arg-max and
one `np.float16` per question.  Here one launch per batch reads the logits once and leaves the answer index, the question id and the float16 row in
device tables at a device-resident cursor; a one-thread launch moves the cursor.  `PredictionBuffer.result()` is the one host synchronisation of a
pass.  The TDIUC figures all derive from one integer table (question type x true answer x {seen, hit}) filled by 64-bit integer atomics, so they are
the same for any order of the rows; `TypeMeter.result()` copies it once and `tdiuc_summary` does the host arithmetic.  As with ScoreMeter, nothing
synchronises, allocates inside the library or passes a per-step value as a kernel argument: `append` / `update` can be captured and replayed."""
import numpy as np
import torch

from . import _lib as L
from . import ops


class Predictions:
    """What a test pass leaves on the host: `question_ids` (N,) int64, `answers` (N,) int64 label indices, `logits` (N, n) float16 or None."""

    __slots__ = ("question_ids", "answers", "logits")

    def __init__(self, question_ids, answers, logits=None):
        self.question_ids, self.answers, self.logits = question_ids, answers, logits

    def __len__(self):
        return len(self.question_ids)

    def to_json(self, label2ans):
        """The list `make_json` builds (src/FFOE/test.py:114-122): [{"question_id": int, "answer": label2ans[index]}, ...]."""
        return [{"question_id": int(q), "answer": label2ans[int(a)]} for q, a in zip(self.question_ids, self.answers)]

    def teacher_logits(self):
        """The dict `make_json_with_logits` builds (src/FFOE/test.py:125-130): {int(question id): float16 vector}; what teacher_logits.py dumps and loads."""
        if self.logits is None:
            raise ValueError("these predictions were taken with keep_logits=False")
        return {int(q): self.logits[i].copy() for i, q in enumerate(self.question_ids)}


class PredictionBuffer:
    """The answers of a test pass, gathered on the device.

        buf = cti_amd.PredictionBuffer(len(dataset), num_ans_candidates, device)     # allocates everything: create it BEFORE a capture
        buf.append(logits, question_ids)                                             # per batch; no sync
        p = buf.result()                                                             # the one sync: Predictions, cut to the rows appended

    `append` takes (rows, n_answers) logits (a non-fp32 dtype is converted with `.float()`) and `rows` question ids of any integer dtype on either
    device (an int64 device tensor is used as it stands).  An append past `capacity` writes nothing and sets a sticky flag that `result()` reports.
    `keep_logits=False` leaves out the (capacity, n_answers) float16 table.  One buffer belongs to one stream at a time."""

    def __init__(self, capacity, n_answers, device="cuda", keep_logits=True):
        self.capacity, self.n_answers = int(capacity), int(n_answers)
        self._state = ops.predict_state(self.capacity, self.n_answers, device)
        self.device = self._state.device
        self._answers = torch.zeros(self.capacity, device=self.device, dtype=torch.int64)
        self._qids = torch.zeros(self.capacity, device=self.device, dtype=torch.int64)
        self._half = torch.zeros(self.capacity, self.n_answers, device=self.device, dtype=torch.float16) if keep_logits else None

    def append(self, logits, qids):
        if logits.dtype != torch.float32:
            logits = logits.float()
        if not isinstance(qids, torch.Tensor):
            qids = torch.as_tensor(qids)
        if qids.dtype.is_floating_point or qids.dtype.is_complex or qids.dtype == torch.bool:
            raise TypeError("question ids must have an integer dtype, got %s" % qids.dtype)
        if qids.device != self.device or qids.dtype != torch.int64:
            qids = qids.to(device=self.device, dtype=torch.int64)
        if logits.dim() != 2 or logits.shape[1] != self.n_answers:
            raise ValueError("append: logits %s, expected (rows, %d)" % (tuple(logits.shape), self.n_answers))
        ops.predict_rows(logits, qids.reshape(-1), self._state, self._answers, self._qids, self._half)

    def reset(self):
        self._state[:2].zero_()                          # cursor and overflow; capacity and n stay

    def result(self):
        """The one host synchronisation: the state block, then the tables cut to the cursor."""
        cursor, overflow, capacity, _ = (int(x) for x in self._state.cpu().numpy())
        if overflow:
            raise L.CtiError("PredictionBuffer: an append did not fit (capacity %d, cursor %d); nothing was written from that append on"
                             % (capacity, cursor))
        half = self._half[:cursor].cpu().numpy() if self._half is not None else None
        return Predictions(self._qids[:cursor].cpu().numpy(), self._answers[:cursor].cpu().numpy(), half)


def _f32(t):
    return t if t.dtype == torch.float32 else t.float()


def predict(args, model, dataloader, device=None, keep_logits=True):
    """`get_logits` of the reference (src/FFOE/test.py:78-111) with one PredictionBuffer instead of a host copy per batch: the same batch tuples
    `(v, b, q, _, ans, i, _)`, the same dispatch on args.model ('ban' / 'cti' / 'stacked_attention'; 'san', the name the training scripts use, is taken
    too), capacity len(dataloader.dataset) x dataloader.dataset.num_ans_candidates.  Returns Predictions; one host synchronisation, at the end."""
    device = args.device if device is None else device
    buf = PredictionBuffer(len(dataloader.dataset), dataloader.dataset.num_ans_candidates, device, keep_logits=keep_logits)
    device = buf.device
    with torch.no_grad():
        for v, b, q, _, ans, i, _ in iter(dataloader):
            v, b, q, ans = v.to(device), b.to(device), q.to(device), ans.to(device)
            if args.model == "ban":
                logits, _ = model(v, b, q, None)
            elif args.model == "cti":
                logits = model(v, q, ans)
            elif args.model in ("san", "stacked_attention"):
                logits = model(v, q)
            else:
                raise ValueError("predict: args.model is %r, expected 'ban', 'cti', 'san' or 'stacked_attention'" % (args.model,))
            buf.append(_f32(logits), i)
    return buf.result()


def _means(accs):
    """The reference's two means over the per-type accuracies: eps added to every one before both, hmean = T / sum(1 / x) (scipy's formula)."""
    x = np.array([a + 1e-10 for a in accs], np.float64)
    return float(np.mean(x)), float(len(x) / np.sum(1.0 / x))


def tdiuc_summary(table, type_names):
    """Everything `mean_per_class` prints (src/evaluate_TDIUC.py:26-94), from the (T, K + 1, 2) int64 table of TypeMeter: cell [t][g + 1] = {how often g
    was the truth for type t, how often the prediction equalled it}; column 0 is g = -1, a true answer outside the answer key.

    Percentages, the reference's formulas: per type 100 * (hits / seen); eps = 1e-10 added to every per-type accuracy before the arithmetic and the
    harmonic mean; overall = 100 * (all hits / all rows).  Normalised accuracy of a type = 100 * mean over the DISTINCT truths seen for it (-1
    included) of hits / seen.  Types without a sample are left out, as the reference only knows the types of its annotations.  (The reference walks
    Python sets, so its floating-point sums may differ from these in the last bit; its printed %.2f figures are what the tests compare.)"""
    table = np.asarray(table)
    if table.ndim != 3 or table.shape[2] != 2 or table.shape[0] != len(type_names):
        raise ValueError("tdiuc_summary: table %s for %d types" % (table.shape, len(type_names)))
    seen, hits = table[:, :, 0].astype(np.int64), table[:, :, 1].astype(np.int64)
    per_type, per_type_norm = {}, {}
    for t, name in enumerate(type_names):
        total = int(seen[t].sum())
        if total == 0:
            continue
        per_type[name] = 100 * (int(hits[t].sum()) / total)
        truths = np.flatnonzero(seen[t])
        unq = 0.0
        for g in truths:
            unq += int(hits[t, g]) / int(seen[t, g])
        per_type_norm[name] = 100 * unq / len(truths)
    samples = int(seen.sum())
    if samples == 0:
        raise ValueError("tdiuc_summary: the table is empty")
    am, hm = _means(per_type.values())
    amn, hmn = _means(per_type_norm.values())
    return {"per_type": per_type, "arithmetic_mpt": am, "harmonic_mpt": hm, "overall": 100 * (int(hits.sum()) / samples),
            "normalized": {"per_type": per_type_norm, "arithmetic_mpt": amn, "harmonic_mpt": hmn},
            "not_found": int(seen[:, 0].sum()), "samples": samples}


def tdiuc_tables(gt_annotations, answerkey, label2ans):
    """Host tables for TypeMeter from what `evaluate_TDIUC.py` loads (:33-48, :105-107): the `annotations` list of the ground-truth JSON, the answer
    key {answer string: index (str or int)} and the model's label2ans list.  Returns (type_names sorted, {question_id: (type index, index of the true
    answer in the key or -1)}, label_to_key (len(label2ans),) int64 with -1 for a label that is not in the key)."""
    type_names = sorted(set(a["question_type"] for a in gt_annotations))
    index = {t: k for k, t in enumerate(type_names)}
    per_question = {}
    for a in gt_annotations:
        truth = a["answers"][0]["answer"]
        per_question[a["question_id"]] = (index[a["question_type"]], int(answerkey[truth]) if truth in answerkey else -1)
    lut = np.array([int(answerkey[s]) if s in answerkey else -1 for s in label2ans], np.int64).reshape(len(label2ans))
    return type_names, per_question, lut


class TypeMeter:
    """TDIUC's per-question-type accuracies, tallied on the device.

        names, per_question, lut = cti_amd.tdiuc_tables(annotations, answerkey, dataset.label2ans)
        meter = cti_amd.TypeMeter(names, num_key_answers, device, label_to_key=lut)  # allocates the table: create it BEFORE a capture
        meter.update(pred, gt, qtype)                                                # int64 per row; no sync
        r = meter.result()                                                           # the one sync; the dict of tdiuc_summary

    `pred` holds the model's label indices (PredictionBuffer's answers, ops.score_rows' pred) when `label_to_key` is given, else indices into the answer
    key; `gt` the index of the true answer in the key or -1, `qtype` the index into `type_names`.  A row out of range (qtype, gt, pred, or a
    label_to_key entry >= num_key_answers) is counted apart and makes `result()` raise."""

    def __init__(self, type_names, num_key_answers, device="cuda", label_to_key=None):
        self.type_names = list(type_names)
        self.T, self.K = len(self.type_names), int(num_key_answers)
        self._block = ops.type_table(self.T, self.K, device)
        self.device = self._block.device
        self._lut = None
        if label_to_key is not None:
            self._lut = torch.as_tensor(np.asarray(label_to_key), dtype=torch.int64).reshape(-1).contiguous().to(self.device)

    def _i64(self, t):
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(t)
        if t.device != self.device or t.dtype != torch.int64:
            t = t.to(device=self.device, dtype=torch.int64)
        return t.reshape(-1)

    def update(self, pred, gt, qtype):
        ops.type_tally(self._block, self.T, self.K, self._i64(pred), self._i64(gt), self._i64(qtype), self._lut)

    def reset(self):
        self._block.zero_()

    def table(self):
        """(table (T, K + 1, 2) int64 ndarray, invalid count): a host copy (synchronises)."""
        host = self._block.cpu().numpy()
        return host[:-1].reshape(self.T, self.K + 1, 2), int(host[-1])

    def result(self):
        """The one host synchronisation: copies the table and does the reference's arithmetic on it (tdiuc_summary)."""
        table, invalid = self.table()
        if invalid:
            raise L.CtiError("TypeMeter: %d rows had a question type, a true answer or a prediction out of range and were not tallied" % invalid)
        return tdiuc_summary(table, self.type_names)
