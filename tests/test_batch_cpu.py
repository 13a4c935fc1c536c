"""Host side of batch assembly (batch.py, csrc/cti_batch.hip's argument checks): pack_dataset and the numpy restatement tests/batch_refs.py against the
g17_batch_* fixtures, which hold what the reference's Dataset.__getitem__ + utils.trim_collate produce; the refusals of pack_dataset; the C entry
points' argument errors; the loader's arithmetic.  Everything is a copy, a zero, a scatter or an exact widening: compared bit for bit.  No GPU."""
import types

import numpy as np
import pytest
import torch

import cti_amd
import batch_refs as br

L = cti_amd.pkg._lib


def _batches(N, B):
    return [np.arange(lo, min(lo + B, N)) for lo in range(0, N, B)]


@pytest.mark.parametrize("name", br.CASES)
def test_pack_and_the_numpy_restatement_reproduce_the_reference_batches(name):
    fx = br.fixture(name)
    p = cti_amd.pack_dataset(br.dataset_from_fixture(fx))
    gold = br.golden_batches(fx)
    cuts = _batches(len(p), fx.cfg["B"])
    assert len(gold) == len(cuts) and p.kind == ("mc" if fx.cfg["cls"] == "v7w" else "ffoe")
    assert p.q_token.dtype == np.int32 and p.image.dtype == p.question_id.dtype == p.pos.dtype == np.int64 and p.counts.dtype == np.int32
    for idx, want in zip(cuts, gold):
        got, counts, mask = br.assemble(p, idx)
        assert len(got) == len(want)
        for j, (g, w) in enumerate(zip(got, want)):
            assert br.matches_golden(g, w), (name, idx[0], j)
        assert np.array_equal(counts, p.counts[idx]) and mask.shape == (len(idx), counts.max())
        # a fixed pad: the same rows, zero rows behind them
        wide, _, wmask = br.assemble(p, idx, pad_to=int(p.counts.max()) + 2)
        assert wide[0].shape[1] == p.counts.max() + 2 and np.array_equal(wide[0][:, :got[0].shape[1]], got[0])
        assert not wide[0][:, got[0].shape[1]:].any() and wmask[:, got[0].shape[1]:].all()


def test_packed_tables_of_the_mixed_case():
    fx = br.fixture("vqa_d5_n7")
    p = cti_amd.pack_dataset(br.dataset_from_fixture(fx))
    assert p.max_boxes == 4 and p.adaptive and p.num_ans_candidates == 7
    raw = np.array(fx.cfg["counts"])[fx.i["image"]]
    assert np.array_equal(p.counts, np.minimum(raw, 4)) and set(p.counts) == {0, 1, 2, 3, 4}
    assert np.array_equal(p.ans_off, fx.i["ans_off"]) and np.array_equal(p.ans_labels, fx.i["ans_labels"]) and p.ans_labels.dtype == np.int32
    assert br.same_bits(p.ans_scores, fx.i["ans_scores"]) and p.teacher.dtype == np.float16
    assert not p.teacher[10].view(np.uint16).any()                          # the entry without a teacher row: a zero row
    assert br.same_bits(p.teacher[:10], fx.i["teacher"][:10])
    fixed = cti_amd.pack_dataset(br.dataset_from_fixture(br.fixture("v7w_fixed36_d8")))
    assert not fixed.adaptive and fixed.features.shape == (3 * 36, 8) and np.array_equal(fixed.pos, [[0, 36], [36, 72], [72, 108]]) and (fixed.counts == 36).all()
    tdiuc = cti_amd.pack_dataset(br.dataset_from_fixture(br.fixture("tdiuc_d5_n65")))
    assert tdiuc.ans_token is None and 10 in np.diff(tdiuc.ans_off)


def test_the_bf16_restatement_rounds_like_the_upload():
    rs = np.random.RandomState(1750)
    x = np.concatenate([rs.standard_normal(4096).astype(np.float32) * 5, np.float32([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 0.0, -0.0])])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(br.bf16_bits(x), want)


def _toy(n=5):
    """Three images of 2, 0 and 3 objects, four FFOE entries."""
    feats = torch.arange(5 * 3, dtype=torch.float32).reshape(5, 3) + 1
    ds = types.SimpleNamespace(features=feats, spatials=torch.ones(5, 6), pos_boxes=np.array([[0, 2], [2, 2], [2, 5]]), adaptive=True, max_boxes=2,
                               num_ans_candidates=n)
    ds.entries = [{"image": k % 3, "question_id": 100 + k, "q_token": torch.tensor([1, 2, 0]), "ans_token": torch.tensor([3]),
                   "answer": {"labels": torch.tensor([0, n - 1]), "scores": torch.tensor([0.3, 1.0])}} for k in range(4)]
    return ds


def test_absent_answers_become_zero_rows_and_the_tuple_keeps_its_positions():
    ds = _toy()
    ds.entries[1]["answer"] = None                                          # the reference's test split
    ds.entries[2]["answer"] = {"labels": None, "scores": None}              # what tensorize() makes of an empty list
    p = cti_amd.pack_dataset(ds)
    assert p.teacher is None and np.array_equal(p.ans_off, [0, 2, 2, 2, 4]) and np.array_equal(p.counts, [2, 0, 2, 2])
    got, _, _ = br.assemble(p, [0, 1, 2, 3])
    assert len(got) == 7 and not got[3][1:3].any() and got[3][0].tolist() == [np.float32(0.3), 0, 0, 0, 1.0]
    assert got[6].shape == (4, 5) and not got[6].any()


def test_pack_refuses_what_the_kernels_could_not_take():
    ds = _toy()
    ds.entries[2]["answer"] = {"labels": torch.tensor([1, 3, 1]), "scores": torch.tensor([0.3, 1.0, 0.6])}
    with pytest.raises(ValueError, match="entry 2: duplicate labels"):
        cti_amd.pack_dataset(ds)
    ds = _toy()
    ds.pos_boxes = np.array([[0, 2], [2, 2], [2, 6]])
    with pytest.raises(ValueError, match=r"entry 2: pos_boxes\[2\]"):
        cti_amd.pack_dataset(ds)
    ds = _toy()
    ds.pos_boxes = np.array([[0, 2], [3, 2], [2, 5]])                       # end before start
    with pytest.raises(ValueError, match=r"entry 1: pos_boxes\[1\]"):
        cti_amd.pack_dataset(ds)
    ds = _toy()
    ds.entries[3]["image"] = 3
    with pytest.raises(ValueError, match="entry 3: image index 3"):
        cti_amd.pack_dataset(ds)
    ds = _toy()
    ds.entries[1]["q_token"] = torch.tensor([1, 2 ** 31, 0])
    with pytest.raises(ValueError, match="entry 1: q_token holds a token outside int32"):
        cti_amd.pack_dataset(ds)
    ds = _toy()
    ds.entries[0]["answer"] = {"labels": torch.tensor([5]), "scores": torch.tensor([1.0])}
    with pytest.raises(ValueError, match="entry 0: a label is outside"):
        cti_amd.pack_dataset(ds)
    ds = _toy()
    ds.entries[0]["teacher_logit"] = np.float32([0.1, 0, 0, 0, 0])          # float16 does not hold 0.1f
    with pytest.raises(ValueError, match="entry 0: teacher_logit"):
        cti_amd.pack_dataset(ds)


def test_argument_errors_do_not_launch():
    lib = L.lib()
    one = 64                                                                # any non-NULL aligned address: nothing is dereferenced before the checks
    ok = dict(table=one, rows=5, d=3, eb=4, idx=one, B=2, N=4, image=one, pos=one, n_img=3, mb=2, Vpad=2, out=one, counts=None, mask=None, state=one)

    def objects(**kw):
        a = dict(ok, **kw)
        return lib.cti_batch_objects(a["table"], a["rows"], a["d"], a["eb"], a["idx"], a["B"], a["N"], a["image"], a["pos"], a["n_img"], a["mb"], a["Vpad"],
                                     a["out"], a["counts"], a["mask"], a["state"], None)

    for name in ("table", "idx", "image", "pos", "out", "state"):
        assert objects(**{name: None}) == -1 and b"NULL" in lib.cti_last_error_string(), name
    for kw in (dict(rows=-1), dict(d=0), dict(eb=3), dict(eb=8), dict(B=-1), dict(N=0), dict(n_img=0), dict(mb=-1), dict(Vpad=0), dict(B=2 ** 31, Vpad=1)):
        assert objects(**kw) == -2, kw
    assert objects(out=66, eb=4) == -3 and objects(state=68) == -3 and objects(idx=68) == -3 and objects(counts=66) == -3
    assert objects(B=0) == 0                                               # an empty batch: nothing launched

    assert lib.cti_batch_targets(None, one, one, 3, one, 2, 4, 7, one, one, None) == -1
    assert lib.cti_batch_targets(one, None, one, 3, one, 2, 4, 7, one, one, None) == -1          # nnz > 0 needs labels
    assert lib.cti_batch_targets(one, None, None, 0, one, 0, 4, 7, one, one, None) == 0          # none when there is no answer at all
    assert lib.cti_batch_targets(one, one, one, 3, one, 2, 4, 0, one, one, None) == -2           # n = 0
    assert lib.cti_batch_targets(one, one, one, -1, one, 2, 4, 7, one, one, None) == -2
    assert lib.cti_batch_targets(one, one, one, 3, one, 2, 0, 7, one, one, None) == -2           # N = 0
    assert lib.cti_batch_targets(one, one, one, 3, one, 2, 4, 7, 66, one, None) == -3

    assert lib.cti_batch_rows(None, L.BATCH_I32_I64, one, 2, 4, 14, one, one, None) == -1
    assert lib.cti_batch_rows(one, L.BATCH_I32_I64, one, 2, 4, 0, one, one, None) == -2          # w = 0
    assert lib.cti_batch_rows(one, L.BATCH_I32_I64, one, -1, 4, 14, one, one, None) == -2
    assert lib.cti_batch_rows(one, 4, one, 2, 4, 14, one, one, None) == -4 and lib.cti_batch_rows(one, -1, one, 2, 4, 14, one, one, None) == -4
    assert lib.cti_batch_rows(one, L.BATCH_I32_I64, one, 2, 4, 14, 68, one, None) == -3          # int64 rows at a 4-byte address
    assert lib.cti_batch_rows(66, L.BATCH_F16_F32, one, 0, 4, 14, 68, one, None) == 0            # float16 rows at a 2-byte address, B = 0
    assert lib.cti_batch_rows(66, L.BATCH_F32_F32, one, 2, 4, 14, 68, one, None) == -3


def test_the_device_classes_have_no_cpu_path():
    p = cti_amd.pack_dataset(_toy())
    with pytest.raises(cti_amd.CtiError):
        cti_amd.DeviceDataset(p, device="cpu")
    with pytest.raises(cti_amd.CtiError):
        cti_amd.ops.batch_state("cpu")
    st, idx = torch.zeros(8, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(cti_amd.CtiError):
        cti_amd.ops.batch_rows(torch.zeros(4, 3, dtype=torch.int32), idx, st)
    with pytest.raises(cti_amd.CtiError):
        cti_amd.ops.batch_targets(torch.zeros(5, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0), idx, 7, st)
    with pytest.raises(cti_amd.CtiError):
        cti_amd.ops.batch_objects(torch.zeros(5, 3), idx, torch.zeros(3, 2, dtype=torch.int64), idx, 2, 2, st)


class _HostDS:
    """What DeviceLoader reads of a DeviceDataset before it iterates."""

    def __init__(self, N):
        self.N, self.packed = N, types.SimpleNamespace(dataset="the original")

    def __len__(self):
        return self.N


@pytest.mark.parametrize("world", [1, 2, 3])
def test_loader_arithmetic_on_the_host(world):
    N, bs = 23, 4
    seen = []
    for rank in range(world):
        local = len(range(rank, N, world))
        keep = cti_amd.DeviceLoader(_HostDS(N), bs, shuffle=True, generator=torch.Generator().manual_seed(7), rank=rank, world=world)
        drop = cti_amd.DeviceLoader(_HostDS(N), bs, drop_last=True, rank=rank, world=world)
        assert keep.dataset == "the original" and keep.local == local
        assert len(keep) == -(-local // bs) and len(drop) == local // bs
        order = keep.epoch_order()
        assert order.dtype == torch.int64 and order.is_contiguous() and len(order) == local
        seen.append(order.numpy())
        assert np.array_equal(drop.epoch_order().numpy(), np.arange(rank, N, world))          # unshuffled: the rank's stride
    assert sorted(np.concatenate(seen).tolist()) == list(range(N))         # the ranks partition the epoch: every index exactly once
    assert not np.array_equal(np.concatenate(seen), np.arange(N))
    with pytest.raises(ValueError):
        cti_amd.DeviceLoader(_HostDS(N), bs, rank=world, world=world)
    with pytest.raises(ValueError):
        cti_amd.DeviceLoader(_HostDS(N), 0)
