"""Batch assembly on an MI355X (csrc/cti_batch.hip through DeviceDataset / DeviceLoader) against the g17_batch_* fixtures, which hold what the
reference's Dataset.__getitem__ + utils.trim_collate produce on the CPU, and against the numpy restatement tests/batch_refs.py (which
tests/test_batch_cpu.py ties to the same fixtures).  Every output is a copy, a zero, a scatter of given values or an exact widening: everything is
compared bit for bit, dtype and shape included."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import cti_amd
import batch_refs as br
from golden_util import model_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def N_(t):
    """A device tensor on the host; bf16 as its uint16 bits."""
    t = t.cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()


@functools.lru_cache(maxsize=None)
def packed(name):
    fx = br.fixture(name)
    return fx, cti_amd.pack_dataset(br.dataset_from_fixture(fx))


def _cuts(N, B):
    return [np.arange(lo, min(lo + B, N)) for lo in range(0, N, B)]


def _equal(got, want, what):
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        assert br.same_bits(N_(g), w), (what, j, g.dtype, tuple(g.shape), w.dtype, w.shape)


@pytest.mark.parametrize("name", br.CASES)
def test_assemble_equals_the_reference(name):
    fx, p = packed(name)
    ds = cti_amd.DeviceDataset(p, DEV)
    gold = br.golden_batches(fx)
    vmax = int(p.counts.max())
    for k, idx in enumerate(_cuts(len(p), fx.cfg["B"])):
        got = ds.assemble(torch.from_numpy(idx))                            # pad_to=None: trim_collate, the indices on the host
        assert len(got) == len(gold[k]) == ds.positions
        for j, (g, w) in enumerate(zip(got, gold[k])):
            assert g.is_cuda and br.matches_golden(N_(g), w), (name, k, j, g.dtype, tuple(g.shape), w.dtype, w.shape)
        for pad in ("max", vmax + 3):                                       # a fixed pad, the indices on the device only
            B, Vpad = len(idx), vmax if pad == "max" else pad
            counts = torch.full((B,), -7, device=DEV, dtype=torch.int32)
            mask = torch.full((B, Vpad), 9, device=DEV, dtype=torch.uint8)
            got = ds.assemble(T(idx), pad_to=pad, counts=counts, mask=mask)
            want, wcounts, wmask = br.assemble(p, idx, pad_to=pad)
            _equal(got, want, (name, k, pad))
            assert br.same_bits(N_(counts), wcounts) and br.same_bits(N_(mask), wmask)
            for r, c in enumerate(wcounts):                                 # all padding exactly +0.0
                assert not N_(got[0])[r, c:].view(np.uint32).any() and not N_(got[1])[r, c:].view(np.uint32).any()
    ds.check()


@pytest.mark.parametrize("name", ["vqa_d5_n7", "vqa_d3_n2", "vqa_d2048_n3129", "v7w_fixed36_d8"])
def test_bf16_feature_table(name):
    fx, p = packed(name)
    ds = cti_amd.DeviceDataset(p, DEV, feature_dtype=torch.bfloat16)
    assert ds.features.dtype == torch.bfloat16 and br.same_bits(N_(ds.features), br.bf16_bits(p.features))
    for idx in _cuts(len(p), fx.cfg["B"]):
        got = ds.assemble(torch.from_numpy(idx))
        assert got[0].dtype == torch.bfloat16 and got[1].dtype == torch.float32
        _equal(got, br.assemble(p, idx, bf16=True)[0], (name, "trim"))
        _equal(ds.assemble(T(idx), pad_to="max"), br.assemble(p, idx, pad_to="max", bf16=True)[0], (name, "max"))
    ds.check()


@pytest.mark.parametrize("name", ["vqa_d5_n7", "tdiuc_d5_n65", "v7w_d5"])
def test_out_buffers_are_overwritten_whole(name):
    fx, p = packed(name)
    ds = cti_amd.DeviceDataset(p, DEV)
    idx = np.arange(min(len(p), fx.cfg["B"]))
    shapes = ds.assemble(T(idx), pad_to="max")
    out = []
    for t in shapes:                                                        # NaNs / an all-ones pattern everywhere
        out.append(torch.full_like(t, float("nan")) if t.dtype.is_floating_point else torch.full_like(t, -1))
    got = ds.assemble(T(idx), pad_to="max", out=out)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    _equal(out, br.assemble(p, idx, pad_to="max")[0], name)
    with pytest.raises(ValueError):
        ds.assemble(T(idx), pad_to="max", out=out[:-1])
    with pytest.raises(ValueError):
        ds.assemble(T(idx), pad_to=int(p.counts.max()) - 1)
    with pytest.raises(ValueError):
        ds.assemble(T(idx))                                                 # pad_to=None needs the indices on the host


def test_a_data_set_without_teacher_rows_gives_zero_rows_into_out():
    fx, p = packed("vqa_d5_n7")
    q = cti_amd.pack_dataset(br.dataset_from_fixture(fx))
    q.teacher = None
    ds = cti_amd.DeviceDataset(q, DEV)
    idx = np.array([3, 1, 4])
    got = ds.assemble(T(idx), pad_to="max")
    out = [torch.full_like(t, float("nan")) if t.dtype.is_floating_point else torch.full_like(t, -1) for t in got]
    ds.assemble(T(idx), pad_to="max", out=out)
    want = br.assemble(q, idx, pad_to="max")[0]
    _equal(got, want, "fresh")
    _equal(out, want, "out")
    assert not N_(out[6]).view(np.uint32).any()


def test_a_repeated_index_gives_equal_rows():
    fx, p = packed("vqa_d5_n7")
    ds = cti_amd.DeviceDataset(p, DEV)
    idx = np.array([4, 2, 4, 4, 0, 2])
    got = ds.assemble(T(idx), pad_to="max")
    _equal(got, br.assemble(p, idx, pad_to="max")[0], "repeated")
    for g in got:                                                           # by bit pattern: a teacher row holds a NaN
        g = N_(g)
        assert br.same_bits(g[0], g[2]) and br.same_bits(g[0], g[3]) and br.same_bits(g[1], g[5])
    ds.check()


@pytest.mark.parametrize("name", ["vqa_d5_n7", "v7w_d5"])
def test_indices_out_of_range_give_zero_samples_and_a_sticky_word(name):
    """The range check itself: -1 and N are compared, never used as an address."""
    fx, p = packed(name)
    N = len(p)
    ds = cti_amd.DeviceDataset(p, DEV)
    ds.check()                                                              # a fresh state block reports clean
    idx = np.array([2, -1, 4, N, 0])
    counts = torch.full((5,), -7, device=DEV, dtype=torch.int32)
    mask = torch.full((5, int(p.counts.max())), 9, device=DEV, dtype=torch.uint8)
    got = ds.assemble(T(idx), pad_to="max", counts=counts, mask=mask)
    want = br.assemble(p, np.array([2, 0, 4, 0, 0]), pad_to="max")[0]
    for j, (g, w) in enumerate(zip(got, want)):
        g = N_(g)
        w = w.copy()
        w[[1, 3]] = 0
        assert br.same_bits(g, w), (name, j)
        assert not g[[1, 3]].view(np.uint8).any()
    assert N_(counts)[[1, 3]].tolist() == [0, 0] and N_(mask)[[1, 3]].all()
    with pytest.raises(cti_amd.CtiError, match="entry index outside"):
        ds.check()
    with pytest.raises(cti_amd.CtiError):                                   # sticky
        ds.check()
    ds.reset()
    ds.check()
    _equal(ds.assemble(T(idx[[0, 2, 4]]), pad_to="max"), br.assemble(p, idx[[0, 2, 4]], pad_to="max")[0], "after reset")
    ds.check()


def test_tables_out_of_range_are_not_dereferenced():
    """An image number or a pos pair outside the table (pack_dataset refuses them; here they are planted on the device) is compared and flagged."""
    fx, p = packed("vqa_d5_n7")
    ds = cti_amd.DeviceDataset(p, DEV)
    idx = np.array([0, 1, 2, 3])
    ds.image[1] = len(p.pos)                                                # entry 1: an image past the table
    img2 = int(p.image[2])
    ds.pos[img2, 1] = p.features.shape[0] + 1                               # entry 2: a span that ends past the table
    got = ds.assemble(T(idx), pad_to="max")
    want = br.assemble(p, idx, pad_to="max")[0]
    for j in (0, 1):
        w = want[j].copy()
        w[[1, 2]] = 0
        assert br.same_bits(N_(got[j]), w), j
    _equal(got[2:], want[2:], "the rows do not depend on the image")
    with pytest.raises(cti_amd.CtiError, match="image index outside.*pos_boxes row outside"):
        ds.check()


def test_an_assemble_call_captured_in_a_graph_follows_the_index_vector():
    fx, p = packed("vqa_d5_n7")
    ds = cti_amd.DeviceDataset(p, DEV)
    B = 5
    idx_static = torch.zeros(B, device=DEV, dtype=torch.int64)
    out = [torch.zeros_like(t) for t in ds.assemble(idx_static, pad_to="max")]       # everything exists before the capture
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ds.assemble(idx_static, pad_to="max", out=out)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            ds.assemble(idx_static, pad_to="max", out=out)
    torch.cuda.current_stream().wait_stream(s)
    for idx in (np.array([10, 9, 8, 7, 6]), np.array([0, 1, 2, 3, 4]), np.array([5, 5, 0, 10, 3])):
        idx_static.copy_(T(idx))
        g.replay()
        eager = ds.assemble(T(idx), pad_to="max")
        for o, e in zip(out, eager):
            assert br.same_bits(N_(o), N_(e))
        _equal(out, br.assemble(p, idx, pad_to="max")[0], idx.tolist())
    ds.check()


def test_loader_visits_every_entry_once_and_ranks_partition_the_epoch():
    fx, p = packed("vqa_d5_n257")
    ds = cti_amd.DeviceDataset(p, DEV)
    N, bs = len(p), 50
    loader = cti_amd.DeviceLoader(ds, bs, shuffle=True, generator=torch.Generator().manual_seed(11), pad_to="max")
    assert len(loader) == 6 and loader.dataset is p.dataset and len(loader.dataset) == N
    sizes, qids = [], []
    for batch in loader:
        assert len(batch) == 7 and batch[0].shape[1:] == (int(p.counts.max()), 5)
        sizes.append(batch[0].shape[0])
        qids.append(N_(batch[5]))
    assert sizes == [50, 50, 50, 50, 50, 7]                                 # the last, short batch
    first = np.concatenate(qids)
    assert sorted(first.tolist()) == sorted(p.question_id.tolist()) and not np.array_equal(first, p.question_id)
    second = np.concatenate([N_(b[5]) for b in loader])                     # the generator has moved on: another order, again every entry once
    assert sorted(second.tolist()) == sorted(first.tolist()) and not np.array_equal(second, first)
    assert [b[0].shape[0] for b in cti_amd.DeviceLoader(ds, bs, drop_last=True, pad_to="max")] == [50] * 5
    # two ranks, the same seed: together every entry once; an unshuffled trim_collate pass equals the fixture-checked restatement
    seen = []
    for rank in (0, 1):
        ld = cti_amd.DeviceLoader(ds, bs, shuffle=True, generator=torch.Generator().manual_seed(12), pad_to="max", rank=rank, world=2)
        mine = np.concatenate([N_(b[5]) for b in ld])
        assert len(mine) == len(range(rank, N, 2)) and len(ld) == 3
        seen.append(mine)
    assert not set(seen[0]) & set(seen[1]) and sorted(np.concatenate(seen).tolist()) == sorted(p.question_id.tolist())
    for k, batch in enumerate(cti_amd.DeviceLoader(ds, 100)):
        idx = np.arange(100 * k, min(100 * k + 100, N))
        _equal(batch, br.assemble(p, idx)[0], ("trim", k))
    ds.check()


# ---- end to end at toy widths ------------------------------------------------------------------------------------------------------------------
class _ToyDS:
    """An adaptive FFOE data set at the widths of a g9 model fixture: image 0 has V objects, the others fewer; entry k looks at image k % n_img."""

    def __init__(self, c, N, seed):
        rs = np.random.RandomState(seed)
        V, n, A = c["V"], c["num_ans"], c.get("A", 3)
        counts = np.array([V, 1, V - 2, 3, V - 1])
        ends = np.cumsum(counts)
        self.pos_boxes = np.stack([ends - counts, ends], 1)
        self.features = torch.from_numpy(np.abs(rs.standard_normal((ends[-1], c["v_dim"]))).astype(np.float32))
        self.spatials = torch.from_numpy(rs.uniform(size=(ends[-1], 6)).astype(np.float32))
        self.adaptive, self.max_boxes, self.num_ans_candidates = True, V, n
        self.dictionary, self.v_dim = types.SimpleNamespace(ntoken=c["ntoken"]), c["v_dim"]
        self.label2ans = ["answer %d" % k for k in range(n)]
        self.entries = []
        for k in range(N):
            lab = rs.choice(n, size=min(n, 1 + k % 3), replace=False)
            self.entries.append({"image": k % len(counts), "question_id": 524291000 + 7 * k, "q_token": torch.from_numpy(rs.randint(0, c["ntoken"], c["Q"])),
                                 "ans_token": torch.from_numpy(rs.randint(0, c["ntoken"], A)),
                                 "answer": {"labels": torch.from_numpy(lab), "scores": torch.from_numpy((rs.randint(1, 9, len(lab)) / 8.0).astype(np.float32))},
                                 "teacher_logit": rs.standard_normal(n).astype(np.float16)})

    def __len__(self):
        return len(self.entries)


class _Loader(list):
    """A list of batch tuples with the `.dataset` evaluate() and predict() read."""


def _model(name, builder, ds):
    fx, params = model_case(name)
    m = getattr(cti_amd, builder)(types.SimpleNamespace(**fx.cfg["args"]), ds)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return m.to(DEV)


@pytest.mark.parametrize("name,builder,model", [("g9_ffoe_cti", "build_cti", "cti"), ("g9_ffoe_ban", "build_ban", "ban")])
def test_evaluate_and_predict_take_the_loader_for_a_dataloader(name, builder, model):
    c = model_case(name)[0].cfg
    toy = _ToyDS(c, 10, 1760)
    p = cti_amd.pack_dataset(toy)
    m = _model(name, builder, toy).eval()
    bs = 5                                                                  # entries 0 and 5 look at image 0: every batch pads to V, as trim_collate does
    host = _Loader(tuple(torch.from_numpy(t) for t in br.assemble(p, idx)[0]) for idx in _cuts(10, bs))
    host.dataset = toy
    assert all(b[0].shape[1] == c["V"] for b in host)
    loader = cti_amd.DeviceLoader(cti_amd.DeviceDataset(p, DEV), bs)
    args = types.SimpleNamespace(device=DEV, model=model)
    assert cti_amd.evaluate(m, loader, args) == cti_amd.evaluate(m, host, args)
    got, want = cti_amd.predict(args, m, loader), cti_amd.predict(args, m, host)
    assert len(got) == 10 and np.array_equal(got.question_ids, want.question_ids) and np.array_equal(got.answers, want.answers)
    assert br.same_bits(got.logits, want.logits)
    loader.ds.check()


def test_trainer_fed_by_the_loader_replays_one_graph_over_adaptive_features():
    cti_amd.set_precision("fp32")
    try:
        c = model_case("g9_ffoe_cti")[0].cfg
        toy = _ToyDS(c, 4 * 8 + 5, 1770)
        m = _model("g9_ffoe_cti", "build_cti", toy)
        for mod in m.modules():
            if isinstance(mod, nn.Dropout):
                mod.p = 0.0
        ds = cti_amd.DeviceDataset(cti_amd.pack_dataset(toy), DEV)
        loader = cti_amd.DeviceLoader(ds, 8, shuffle=True, generator=torch.Generator().manual_seed(5), pad_to="max")
        args = types.SimpleNamespace(device=DEV, model="cti", distillation=False, clip_norm=0.25, gamma=2)
        trainer = cti_amd.Trainer(args, m.train(), nn.BCEWithLogitsLoss(reduction="sum"), torch.optim.Adamax([q for q in m.parameters() if q.requires_grad], lr=2e-3),
                                  graph_after=2)
        steps = 0
        for i, (v, b, q, a, ans, _, t_logits) in enumerate(loader):
            assert v.shape[1] == c["V"]                                     # every batch alike, whatever its images hold
            loss, _, _ = trainer.train_step([v, b, q, a, ans, t_logits], update_params=True)
            assert torch.isfinite(loss).item()
            assert trainer.graphed == (i >= 2)                              # captured by the third full batch
            steps += 1
        assert steps == 5 and trainer.captures == 1 and trainer.get_num_updates() == 5
        assert trainer.meter.result()["samples"] == 4 * 8 + 5
        ds.check()
    finally:
        cti_amd.set_precision("bf16x3")
