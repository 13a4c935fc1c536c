"""Bucketed batching on an MI355X: DeviceLoader(pad_to='bucket') against the host rule (batch.bucket_plan) and the numpy restatement of batch
assembly (tests/batch_refs.py), evaluate() / predict() over a bucketed loader against an unbucketed one, and Trainer(max_graphs=K) replaying one
captured micro-step per width against the same trainer run eagerly."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import cti_amd
import batch_refs as br
from golden_util import model_case
from oracle.cti_oracle import norm_max_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def N_(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def packed(name):
    fx = br.fixture(name)
    return fx, cti_amd.pack_dataset(br.dataset_from_fixture(fx))


def _equal(got, want, what):
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        assert br.same_bits(N_(g), w), (what, j, g.dtype, tuple(g.shape), w.dtype, w.shape)


def test_bucketed_loader_follows_the_host_rule():
    fx, p = packed("vqa_d5_n257")
    ds = cti_amd.DeviceDataset(p, DEV)
    N, bs = len(p), 50
    widths = cti_amd.bucket_widths_for(p.counts, 3)
    assert len(widths) >= 2 and widths[-1] == p.counts.max()
    loader = cti_amd.DeviceLoader(ds, bs, shuffle=True, generator=torch.Generator().manual_seed(11), pad_to="bucket", bucket_widths=3)
    assert loader.widths == widths and len(loader) == 6 and loader.dataset is p.dataset
    g = torch.Generator().manual_seed(11)                                   # the plan, from the generator's draws: the epoch, then the order of the full batches
    order = torch.randperm(N, generator=g)
    visit = torch.randperm(5, generator=g).tolist() + [5]
    entries, groups = cti_amd.bucket_plan(order, p.counts, widths, bs)
    epochs = []
    for epoch in range(2):
        qids, seen_widths = [], []
        for k, batch in enumerate(loader):
            assert len(batch) == 7 and batch[0].shape[1] == loader.plan_widths[k] and batch[0].shape[1] in widths
            lo, hi = 50 * k, min(50 * k + 50, N)
            idx = loader.plan_entries[lo:hi].numpy()
            assert batch[0].shape[0] == hi - lo and p.counts[idx].max() <= batch[0].shape[1]
            if epoch == 0:
                glo, ghi, gwidth = groups[visit[k]]
                assert gwidth == loader.plan_widths[k] and np.array_equal(idx, entries[glo:ghi].numpy())
            _equal(batch, br.assemble(p, idx, pad_to=loader.plan_widths[k])[0], (epoch, k))
            qids.append(N_(batch[5]))
            seen_widths.append(batch[0].shape[1])
        assert len(qids) == 6 and len(qids[-1]) == 7 and seen_widths == loader.plan_widths
        assert len(set(seen_widths)) >= 2                                   # the fixture's counts do spread over the widths
        epochs.append(np.concatenate(qids))
        assert sorted(epochs[-1].tolist()) == sorted(p.question_id.tolist())                      # every question once
    assert not np.array_equal(epochs[0], epochs[1])
    # unshuffled: widths ascending, entries ascending within a bucket; drop_last drops the short group
    plain = cti_amd.DeviceLoader(ds, bs, pad_to="bucket", bucket_widths=widths)
    got = [b[0].shape[1] for b in plain]
    assert got[:-1] == sorted(got[:-1]) and got == plain.plan_widths
    assert [b[0].shape[0] for b in cti_amd.DeviceLoader(ds, bs, drop_last=True, pad_to="bucket", bucket_widths=widths)] == [50] * 5
    # two ranks, generators in the same state: equal widths batch for batch, together every question once
    seen, rank_widths = [], []
    for rank in (0, 1):
        ld = cti_amd.DeviceLoader(ds, 25, shuffle=True, generator=torch.Generator().manual_seed(12), pad_to="bucket", bucket_widths=widths, rank=rank, world=2)
        mine = [N_(b[5]) for b in ld]
        assert len(mine) == len(ld) == 6 and [len(m) for m in mine[:-1]] == [25] * 5
        seen.append(np.concatenate(mine))
        rank_widths.append(ld.plan_widths)
    assert rank_widths[0] == rank_widths[1] and [len(s) for s in seen] == [129, 128]
    assert not set(seen[0]) & set(seen[1]) and sorted(np.concatenate(seen).tolist()) == sorted(p.question_id.tolist())
    ds.check()


# ---- end to end at toy widths ------------------------------------------------------------------------------------------------------------------
class _ToyDS:
    """An adaptive FFOE data set at the widths of a g9 model fixture: image j has counts[j] objects, entry k looks at image k % n_img."""

    def __init__(self, c, N, seed, counts):
        rs = np.random.RandomState(seed)
        V, n, A = c["V"], c["num_ans"], c.get("A", 3)
        counts = np.asarray(counts)
        assert counts.max() == V
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


def _model(name, builder, ds):
    fx, params = model_case(name)
    m = getattr(cti_amd, builder)(types.SimpleNamespace(**fx.cfg["args"]), ds)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return m.to(DEV)


@pytest.mark.parametrize("name,builder,model", [("g9_ffoe_cti", "build_cti", "cti"), ("g9_ffoe_ban", "build_ban", "ban")])
def test_evaluate_and_predict_over_a_bucketed_loader(name, builder, model):
    """Which of the two holds for the logits: they differ by SUMMATION ORDER ONLY.  The padding rows are zeros in both loaders and the attention masks
    them out (an all-zero object row gets the logit -inf, so the probability exactly 0), hence the same terms are summed; but a sample sits at another row
    of another batch, next to other samples, under another object dimension, so the kernels that reduce over the objects of a sample (soft-max, the
    pools) and the GEMMs over B x V rows may associate those terms differently.  The logits are therefore compared within the tolerance of the
    full-model tests for this mode, tests/test_models_gpu.py: TOL = 1e-4 as the normalised max error, in 'fp32' -- on the float16 values predict()
    returns, whose answers (the arg-max) and hence the scores must be the same.  (Measured at these shapes: none of the 407 float16 values differs.)"""
    cti_amd.set_precision("fp32")
    try:
        c = model_case(name)[0].cfg
        toy = _ToyDS(c, 37, 1760, [6, 1, 4, 3, 5, 2])
        p = cti_amd.pack_dataset(toy)
        m = _model(name, builder, toy).eval()
        ds = cti_amd.DeviceDataset(p, DEV)
        whole = cti_amd.DeviceLoader(ds, 8, pad_to="max")
        bucketed = cti_amd.DeviceLoader(ds, 8, shuffle=True, generator=torch.Generator().manual_seed(4), pad_to="bucket", bucket_widths=(2, 4, 6))
        args = types.SimpleNamespace(device=DEV, model=model)
        want_score, got_score = cti_amd.evaluate(m, whole, args), cti_amd.evaluate(m, bucketed, args)
        assert sorted(set(bucketed.plan_widths)) == [2, 4, 6]
        want, got = cti_amd.predict(args, m, whole), cti_amd.predict(args, m, bucketed)
        assert sorted(set(bucketed.plan_widths)) == [2, 4, 6] and len(got) == len(want) == 37
        a, b = np.argsort(want.question_ids, kind="stable"), np.argsort(got.question_ids, kind="stable")
        assert np.array_equal(want.question_ids[a], got.question_ids[b]) and not np.array_equal(want.question_ids, got.question_ids)
        wl, gl = want.logits[a].astype(np.float32), got.logits[b].astype(np.float32)
        err = norm_max_err(gl, wl)
        print("%s: score %r / %r, logits normalised max error %.3g, %d of %d float16 values differ" % (name, got_score, want_score, err, (gl != wl).sum(), gl.size))
        assert got.logits.dtype == np.float16 and err < 1e-4
        assert np.array_equal(want.answers[a], got.answers[b])
        assert got_score == want_score                                      # sums of multiples of 1/8: exact in any order
        ds.check()
    finally:
        cti_amd.set_precision("bf16x3")


# ---- the trainer over several widths -------------------------------------------------------------------------------------------------------------
CLIP = 0.25


def _close(x, ref, rel):
    """As tests/test_trainer_gpu.py."""
    x, ref = (float(t.detach()) if isinstance(t, torch.Tensor) else float(t) for t in (x, ref))
    return abs(x - ref) <= rel * abs(ref)


def _same_parameters(m1, m2):
    """As tests/test_trainer_gpu.py."""
    for (n1, p1), (n2, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert n1 == n2
        assert torch.allclose(p1, p2, rtol=1e-4, atol=2e-6), n1


def _trainer(toy, **kw):
    m = _model("g9_ffoe_cti", "build_cti", toy)
    for mod in m.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0
    args = types.SimpleNamespace(device=DEV, model="cti", distillation=False, clip_norm=CLIP, gamma=2)
    return m, cti_amd.Trainer(args, m.train(), nn.BCEWithLogitsLoss(reduction="sum"),
                              torch.optim.Adamax([q for q in m.parameters() if q.requires_grad], lr=2e-3), **kw)


def _epoch(trainers, loader, update_freq, seen, log):
    """One epoch of the reference's loop (src/FFOE/train.py:70-86) through every trainer on the same batches.  `seen[t]` counts the full batches of
    each width trainer t has taken; `log[t]` collects (width, replayed?) per micro-batch and what each update folded."""
    batches = [[v, b, q, a, ans, t_logits] for v, b, q, a, ans, _, t_logits in loader]
    num_batches = len(batches)
    for t, trainer in enumerate(trainers):
        folded = []
        for i, sample in enumerate(batches):
            width, full = sample[0].shape[1], sample[0].shape[0] == loader.batch_size
            before = trainer.replays
            update = not (i < num_batches - 1 and (i + 1) % update_freq > 0)
            out = trainer.train_step(sample, update_params=update)
            replayed = trainer.replays == before + 1
            folded.append((width, replayed))
            if full:
                seen[t][width] = seen[t].get(width, 0) + 1
            log[t].append((width, full, seen[t].get(width, 0), replayed))
            if update:
                assert len(out) == 3 and torch.isfinite(out[0]).item()
                log[t].append(("update", tuple(folded)))
                folded = []
            else:
                assert out is None
    return sum(s[0].shape[0] for s in batches)


def test_trainer_replays_one_graph_per_width_and_agrees_with_the_eager_run():
    cti_amd.set_precision("fp32")
    try:
        c = model_case("g9_ffoe_cti")[0].cfg
        toy = _ToyDS(c, 7 * 8 + 5, 1770, [6, 1, 4, 3, 5, 2])                  # widths 2, 4, 6: about twenty entries each; seven full batches and a short one
        ds = cti_amd.DeviceDataset(cti_amd.pack_dataset(toy), DEV)
        m_e, eager = _trainer(toy, graph_after=None)
        m_g, graphed = _trainer(toy, graph_after=2, max_graphs=3)
        m_1, single = _trainer(toy, graph_after=2, max_graphs=1)
        assert graphed.max_graphs == 3 and single.max_graphs == 1 and cti_amd.Trainer.__init__.__kwdefaults__["max_graphs"] == 1
        trainers = [eager, graphed, single]
        loader = cti_amd.DeviceLoader(ds, 8, shuffle=True, generator=torch.Generator().manual_seed(5), pad_to="bucket", bucket_widths=(2, 4, 6))
        seen, log = [{}, {}, {}], [[], [], []]
        for epoch in range(3):
            samples = _epoch(trainers, loader, 2, seen, log)
            assert samples == len(toy) and sorted(set(loader.plan_widths)) == [2, 4, 6]
            for x in (graphed, single):
                _same_parameters(m_e, m_g if x is graphed else m_1)
            want = eager.meter.result()
            for x in (graphed, single):
                r = x.meter.result()
                print("epoch %d: loss %.8g / %.8g  grad_norm %.8g / %.8g  score %r / %r" % (epoch, r["loss"], want["loss"], r["grad_norm"], want["grad_norm"],
                                                                                          r["score"], want["score"]))
                assert r["updates"] == want["updates"] == 4 * (epoch + 1) and r["samples"] == want["samples"]
                assert _close(r["loss"], want["loss"], 1e-5) and _close(r["grad_norm"], want["grad_norm"], 1e-4)
                assert r["score"] == want["score"] and r["upper_bound"] == want["upper_bound"]
        # the eager one never captured; max_graphs=3: one capture per width, a full batch replayed from the third of its width on and never before,
        # the short batches (another batch size: a fourth shape with every graph taken) eager
        assert eager.captures == 0 and eager.replays == 0 and not eager.graphed
        assert graphed.captures == 3 and graphed.graphed and all(n >= 3 for n in seen[1].values()) and sorted(seen[1]) == [2, 4, 6]
        steps = [e for e in log[1] if e[0] != "update"]
        assert all(replayed == (full and nth >= 3) for _, full, nth, replayed in steps)
        assert graphed.replays == sum(n - 2 for n in seen[1].values())
        updates = [e[1] for e in log[1] if e[0] == "update"]
        assert any(len(u) == 2 and u[0][0] != u[1][0] and u[0][1] and u[1][1] for u in updates)       # two replayed widths in one update
        assert any(len(u) == 2 and u[0][1] != u[1][1] for u in updates)                                # a replayed and an eager micro-batch in one update
        # max_graphs=1, as before this argument existed: the first width to come a third time is captured, the others stay eager
        first = next(width for width, full, nth, _ in (e for e in log[2] if e[0] != "update") if full and nth == 3)
        assert single.captures == 1 and single.graphed
        assert all(replayed == (full and width == first and nth >= 3) for width, full, nth, replayed in (e for e in log[2] if e[0] != "update"))
        assert graphed.get_num_updates() == single.get_num_updates() == eager.get_num_updates() == 12
        # a fourth width with every graph taken: stays eager however often it comes, and the runs still agree
        other = cti_amd.DeviceLoader(ds, 8, drop_last=True, pad_to="bucket", bucket_widths=(3, 6))
        batches = [[v, b, q, a, ans, t_logits] for v, b, q, a, ans, _, t_logits in other][:3]
        assert [s[0].shape[1] for s in batches] == [3] * 3                    # thrice: a third time would capture if a graph were left
        for x in (eager, graphed):
            for sample in batches:
                x.train_step(sample, update_params=True)
        assert graphed.captures == 3 and graphed.replays == sum(n - 2 for n in seen[1].values())
        _same_parameters(m_e, m_g)
        ds.check()
    finally:
        cti_amd.set_precision("bf16x3")
