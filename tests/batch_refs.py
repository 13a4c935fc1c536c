"""Batch assembly restated in numpy for tests/test_batch_cpu.py and tests/test_batch_gpu.py: what `DeviceDataset.assemble` must produce from a
PackedDataset, for `pad_to=None` (trim_collate: the batch's largest cut count) and a fixed pad, on an fp32 or a bf16 feature table; and the way from a
g17_batch_* fixture (tests/golden/make_golden_batch.py) back to a reference-shaped data set object."""
import types

import numpy as np
import torch

from golden_util import load

CASES = ["vqa_d5_n7", "vqa_d1_n1", "vqa_d3_n2", "vqa_d4_n8", "vqa_d8_n9", "tdiuc_d5_n65", "vqa_d2048_n3129", "vqa_d5_n257", "v7w_d5", "v7w_fixed36_d8"]


def bf16_bits(x):
    """fp32 -> the uint16 bits of its bfloat16, round to nearest even: the rule of torch's fp32 -> bf16 copy, which the upload uses (finite values)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def dataset_from_fixture(fx):
    """A data set object with the attributes pack_dataset reads, as the reference's classes hold them after tensorize(): torch tables, entries as
    dicts of tensors; an empty answer has labels None; an entry without a teacher row has no `teacher_logit` key."""
    c, i = fx.cfg, fx.i
    ds = types.SimpleNamespace(features=torch.from_numpy(i["features"]), spatials=torch.from_numpy(i["spatials"]), adaptive=c["adaptive"],
                               num_ans_candidates=c["num_ans"], label2ans=["answer %d" % k for k in range(c["num_ans"])])
    if c["adaptive"]:
        ds.pos_boxes = i["pos_boxes"]
    setattr(ds, "max_box" if c["cls"] == "v7w" else "max_boxes", c["max_boxes"])
    ds.entries = []
    for k in range(len(i["image"])):
        e = {"image": int(i["image"][k]), "question_id": int(i["question_id"][k]), "q_token": torch.from_numpy(i["q_token"][k])}
        if c["cls"] == "v7w":
            e.update(ans_mc_token=torch.from_numpy(i["ans_mc"][k]), ans_gt_token=torch.from_numpy(i["ans_gt"][k]), label=torch.from_numpy(i["label"][k]),
                     answer=None)
        else:
            a, b = int(i["ans_off"][k]), int(i["ans_off"][k + 1])
            e["answer"] = ({"labels": torch.from_numpy(i["ans_labels"][a:b]), "scores": torch.from_numpy(i["ans_scores"][a:b])} if b > a
                           else {"labels": None, "scores": None})
            if c["cls"] == "vqa":
                e["ans_token"] = torch.from_numpy(i["ans_token"][k])
            if i["teacher_present"][k]:
                e["teacher_logit"] = i["teacher"][k]
        ds.entries.append(e)
    return ListDataset(ds)


class ListDataset:
    """The object of dataset_from_fixture: attributes and a len(), as evaluate() / predict() read them."""

    def __init__(self, ns):
        self.__dict__.update(ns.__dict__)

    def __len__(self):
        return len(self.entries)


def golden_batches(fx):
    """[[position 0, position 1, ...] per batch] of a fixture."""
    out = []
    while "b%d_0" % len(out) in fx.o:
        k, row = len(out), []
        while "b%d_%d" % (k, len(row)) in fx.o:
            row.append(fx.o["b%d_%d" % (k, len(row))])
        out.append(row)
    return out


def assemble(p, idx, pad_to=None, bf16=False):
    """The batch tuple of a PackedDataset as numpy arrays (a bf16 feature batch as its uint16 bits), plus counts (B,) int32 and mask (B, Vpad) uint8."""
    idx = np.asarray(idx, np.int64)
    B = len(idx)
    counts = p.counts[idx].astype(np.int32)
    Vpad = int(counts.max()) if pad_to is None else int(p.counts.max()) if pad_to == "max" else int(pad_to)
    feats = bf16_bits(p.features) if bf16 else p.features
    v = np.zeros((B, Vpad, feats.shape[1]), feats.dtype)
    b = np.zeros((B, Vpad, p.spatials.shape[1]), np.float32)
    for r, e in enumerate(idx):
        s = int(p.pos[p.image[e], 0])
        v[r, :counts[r]] = feats[s:s + counts[r]]
        b[r, :counts[r]] = p.spatials[s:s + counts[r]]
    mask = (np.arange(Vpad)[None, :] >= counts[:, None]).astype(np.uint8)
    q = p.q_token[idx].astype(np.int64)
    if p.kind == "mc":
        return (v, b, q, p.label[idx], p.ans_mc[idx].astype(np.int64), p.ans_gt[idx].astype(np.int64)), counts, mask
    target = np.zeros((B, p.num_ans_candidates), np.float32)
    for r, e in enumerate(idx):
        a, z = p.ans_off[e], p.ans_off[e + 1]
        target[r, p.ans_labels[a:z]] = p.ans_scores[a:z]
    teacher = np.zeros((B, p.num_ans_candidates), np.float32) if p.teacher is None else p.teacher[idx].astype(np.float32)
    if p.ans_token is None:
        return (v, b, q, target, p.question_id[idx], teacher), counts, mask
    return (v, b, q, target, p.ans_token[idx].astype(np.int64), p.question_id[idx], teacher), counts, mask


def same_bits(x, y):
    """Equal dtype, shape and bit pattern (NaNs by payload, -0 apart from +0)."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def matches_golden(got, want):
    """One position of a batch against the fixture.  The reference yields an int64 zero per sample where an entry has no teacher row; ours is the
    zero ROW (the position keeps its shape)."""
    if want.dtype == np.int64 and got.dtype == np.float32:
        return not want.any() and not got.view(np.uint32).any() and got.shape[0] == want.shape[0]
    return same_bits(got, want)


def fixture(name):
    return load("g17_batch_" + name)
