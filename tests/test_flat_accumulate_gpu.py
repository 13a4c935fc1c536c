"""Micro-batch accumulation on the device (the reference's --update_freq, src/FFOE/trainer.py:112-126): cti_flat_gather_acc / cti_flat_scale_sumsq_g /
cti_counter_set on their own, FlatAdamaxDP.accumulate() / update() / param_groups / from_torch, and GraphedTrainStep(accumulate=True).
Tolerances are the ones tests/test_dp_gpu.py uses for the same comparisons.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import cti_amd
from test_dp_gpu import TinyCTI, make_batch, loss_fn

pytestmark = pytest.mark.gpu
DEV = "cuda"
L = cti_amd.pkg._lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def test_flat_gather_acc_overwrites_then_adds_and_leaves_padding_null_and_in_place_entries_alone():
    """The layout of test_flat_gather_packs_zeroes_and_keeps_in_place_entries (403 entries = three launches, 64-float slots, odd counts, sources
    misaligned by 4 / 8 / 12 bytes, flat pre-filled with 7.0), three calls with the device counter at 0, 1, 2 and fresh sources each: overwrite, +=, +=.
    Entries i % 11 == 5 + call have no gradient in that call (so some are NULL first and present later, others the reverse), i % 13 == 7 live in
    their slot.  Bit-exact against numpy float32 over the whole buffer, padding included."""
    lib = L.lib()
    g = torch.Generator().manual_seed(3)
    counts = [int(c) for c in torch.randint(1, 700, (400,), generator=g)] + [70000, 1, 4097]
    offs, off = [], 0
    for c in counts:
        offs.append(off)
        off += (c + 63) // 64 * 64
    n = off
    flat = torch.full((n,), 7.0, device=DEV)
    micro = torch.zeros(1, device=DEV, dtype=torch.int64)
    want = np.full(n, 7.0, np.float32)
    for call in range(3):
        micro.fill_(call)
        rows, keep = [], []
        if call == 0:
            new = np.zeros(n, np.float32)
        for i, (c, o) in enumerate(zip(counts, offs)):
            if i % 11 == 5 + call:                                           # no gradient in this call
                rows += [0, o, c]
            elif i % 13 == 7:                                                # already in its slot
                rows += [flat.data_ptr() + 4 * o, o, c]
                if call == 0:
                    new[o:o + c] = want[o:o + c]
            else:
                base = torch.randn(c + 3, generator=g).to(DEV)
                src = base[i % 4:i % 4 + c]
                keep.append(base)
                rows += [src.data_ptr(), o, c]
                if call == 0:
                    new[o:o + c] = src.cpu().numpy()
                else:
                    want[o:o + c] = want[o:o + c] + src.cpu().numpy()        # one fp32 add per element
        if call == 0:
            want = new
        table = (ctypes.c_int64 * len(rows))(*rows)
        L.check(lib.cti_flat_gather_acc(table, len(counts), flat.data_ptr(), n, micro.data_ptr(), _stream()), "cti_flat_gather_acc")
        assert np.array_equal(flat.cpu().numpy(), want), "call %d" % call
        assert int(micro.item()) == call                                     # the gather reads the counter, the caller bumps it
    assert lib.cti_flat_gather_acc(table, len(counts), flat.data_ptr(), n, None, _stream()) == -1        # CTI_E_NULL before any launch
    bad = (ctypes.c_int64 * 6)(0, 0, 100, 0, 64, 10)                         # second slot starts inside the first
    assert lib.cti_flat_gather_acc(bad, 2, flat.data_ptr(), n, micro.data_ptr(), _stream()) == -2
    assert np.array_equal(flat.cpu().numpy(), want) and int(micro.item()) == 2
    L.check(lib.cti_counter_set(micro.data_ptr(), 0, _stream()), "cti_counter_set")
    assert int(micro.item()) == 0


@pytest.mark.parametrize("count", [0, 1, 3])
def test_flat_scale_sumsq_g_divides_by_world_times_the_device_count(count):
    lib = L.lib()
    n, world = 70004, 2
    g = torch.Generator().manual_seed(17 + count)
    x = torch.randn(n, generator=g)
    buf = x.to(DEV)
    micro = torch.full((1,), count, device=DEV, dtype=torch.int64)
    partial = torch.empty(lib.cti_optim_workspace_bytes() // 4, device=DEV)
    L.check(lib.cti_flat_scale_sumsq_g(buf.data_ptr(), n, world, micro.data_ptr(), partial.data_ptr(), _stream()), "cti_flat_scale_sumsq_g")
    want = x.numpy() / np.float32(world * max(count, 1))                      # count 0 behaves as 1
    assert np.allclose(buf.cpu().numpy(), want, rtol=1e-6, atol=0)
    norm = float(np.sqrt(np.sum(want.astype(np.float64) ** 2)))
    assert abs(float(np.sqrt(partial.double().sum().item())) - norm) <= 1e-5 * norm
    assert lib.cti_flat_scale_sumsq_g(buf.data_ptr(), n, 0, micro.data_ptr(), partial.data_ptr(), _stream()) == -2
    assert int(micro.item()) == count


def _fresh(freq=1, lr=2e-3):
    torch.manual_seed(11)
    m = TinyCTI().to(DEV)
    return m, cti_amd.FlatAdamaxDP(m, lr=lr, clip_norm=0.25, update_freq=freq)


def _micro(m, opt, b, sl=slice(None)):
    opt.zero_grad()
    loss = loss_fn(m(b[0][sl], b[1][sl], b[2][sl]), b[3][sl])
    loss.backward()
    opt.accumulate()
    return loss.detach()


def test_accumulate_three_micro_batches_and_update():
    cti_amd.set_precision("fp32")
    try:
        b = tuple(t.to(DEV) for t in make_batch(12, 100))
        parts = (slice(0, 4), slice(4, 8), slice(8, 12))
        m, opt = _fresh()
        with pytest.raises(RuntimeError):
            opt.update()                                                      # nothing buffered
        for sl in parts:
            _micro(m, opt, b, sl)
        assert opt.micro_count == 3 and int(opt.micro_dev.item()) == 3
        with pytest.raises(RuntimeError):
            opt.step()                                                        # something buffered
        gn = opt.update()
        assert opt.micro_count == 0 and int(opt.micro_dev.item()) == 0 and opt.steps_done() == 1
        # the eager update_freq = 3 route: autograd accumulates, step() divides by 3
        m2, opt2 = _fresh(freq=3)
        opt2.zero_grad()
        for sl in parts:
            loss_fn(m2(b[0][sl], b[1][sl], b[2][sl]), b[3][sl]).backward()
        gn2 = opt2.step()
        assert torch.allclose(opt.flat_p, opt2.flat_p, rtol=1e-5, atol=1e-7)
        assert torch.allclose(gn, gn2, rtol=1e-5)
        # one step on the whole batch of 12
        m3, opt3 = _fresh()
        opt3.zero_grad()
        loss_fn(m3(*b[:3]), b[3]).backward()
        opt3.step()
        assert torch.allclose(opt.flat_p, opt3.flat_p, rtol=2e-4, atol=2e-6)
        # another number of micro-batches on the same optimiser class: two
        m4, opt4 = _fresh()
        for sl in parts[:2]:
            _micro(m4, opt4, b, sl)
        opt4.update()
        m5, opt5 = _fresh(freq=2)
        opt5.zero_grad()
        for sl in parts[:2]:
            loss_fn(m5(b[0][sl], b[1][sl], b[2][sl]), b[3][sl]).backward()
        opt5.step()
        assert torch.allclose(opt4.flat_p, opt5.flat_p, rtol=1e-5, atol=1e-7)
        assert not torch.allclose(opt4.flat_p, opt.flat_p, rtol=1e-5, atol=1e-7)
    finally:
        cti_amd.set_precision("bf16x3")


def test_param_groups_write_through_and_from_torch():
    cti_amd.set_precision("fp32")
    try:
        b = tuple(t.to(DEV) for t in make_batch(8, 100))
        m, opt = _fresh()
        grp = opt.param_groups[0]
        assert len(opt.param_groups) == 1 and grp["lr"] == 2e-3 and grp["betas"] == (0.9, 0.999) and grp["eps"] == 1e-8 and grp["weight_decay"] == 0
        assert len(grp["params"]) == len(opt.params) and all(x is y for x, y in zip(grp["params"], opt.params))
        opt.param_groups[0]["lr"] *= 0.25                                     # src/FFOE/train.py:66
        assert abs(opt.lr - 5e-4) < 1e-12 and abs(float(opt.lr_dev.item()) - 5e-4) < 1e-10 and abs(opt.param_groups[0]["lr"] - 5e-4) < 1e-12
        with pytest.raises(KeyError):
            opt.param_groups[0]["betas"] = (0.5, 0.9)
        _micro(m, opt, b)
        opt.update()
        m2, opt2 = _fresh(lr=5e-4)
        _micro(m2, opt2, b)
        opt2.update()
        m3, opt3 = _fresh()
        _micro(m3, opt3, b)
        opt3.update()
        assert torch.allclose(opt.flat_p, opt2.flat_p, rtol=1e-5, atol=1e-7)   # the next update ran at the new rate
        assert not torch.allclose(opt.flat_p, opt3.flat_p, rtol=1e-5, atol=1e-7)

        torch.manual_seed(11)
        m4 = TinyCTI().to(DEV)
        with pytest.raises(TypeError):
            cti_amd.FlatAdamaxDP.from_torch(m4, torch.optim.SGD(m4.parameters(), lr=1e-2), 0.25)
        with pytest.raises(ValueError):
            cti_amd.FlatAdamaxDP.from_torch(m4, torch.optim.Adamax(m4.parameters(), lr=1e-2, weight_decay=1e-3), 0.25)
        fresh = cti_amd.FlatAdamaxDP.from_torch(m4, torch.optim.Adamax(m4.parameters(), lr=3e-3, betas=(0.8, 0.99), eps=1e-7), 0.5)
        assert abs(fresh.lr - 3e-3) < 1e-12 and fresh.betas == (0.8, 0.99) and fresh.eps == 1e-7 and fresh.clip_norm == 0.5 and fresh.steps_done() == 0

        # a stepped torch.optim.Adamax: two steps in torch, the third here and in torch
        def ref_step(mm, oo, batch):
            oo.zero_grad()
            loss_fn(mm(*batch[:3]), batch[3]).backward()
            flat = torch.cat([p.grad.reshape(-1) for p in mm.parameters() if p.grad is not None])
            coef = 0.25 / (flat.norm() + 1e-6)
            if coef < 1:
                for p in mm.parameters():
                    if p.grad is not None:
                        p.grad.mul_(coef)
            oo.step()
        batches = [tuple(t.to(DEV) for t in make_batch(8, 100 + s)) for s in range(3)]
        torch.manual_seed(11)
        m5, m6 = TinyCTI().to(DEV), TinyCTI().to(DEV)
        m6.load_state_dict(m5.state_dict())
        o5 = torch.optim.Adamax(m5.parameters(), lr=2e-3)
        o6 = torch.optim.Adamax(m6.parameters(), lr=2e-3)
        for s in range(2):
            ref_step(m5, o5, batches[s])
            ref_step(m6, o6, batches[s])
        mine = cti_amd.FlatAdamaxDP.from_torch(m6, o6, 0.25)
        assert mine.steps_done() == 2
        ref_step(m5, o5, batches[2])
        _micro(m6, mine, batches[2])
        mine.update()
        for (n5, p5), (_, p6) in zip(m5.named_parameters(), m6.named_parameters()):
            assert torch.allclose(p6, p5, rtol=1e-4, atol=2e-6), n5
    finally:
        cti_amd.set_precision("bf16x3")


def test_accumulating_graphs_replay_updates_of_two_one_and_three_micro_batches():
    """Graph M (micro-step) and graph U (update) captured once; updates after 2, 1 and 3 replayed micro-batches with a learning-rate change before the
    third == the same sequence through eager accumulate() / update().  The two warm-up steps are one micro-batch + one update each."""
    cti_amd.set_precision("fp32")
    try:
        batches = [tuple(t.to(DEV) for t in make_batch(8, 100 + s)) for s in range(7)]
        plan = [(1, False), (2, True), (3, True), (4, False), (5, False), (6, True)]
        m1, opt1 = _fresh()
        for _ in range(2):
            _micro(m1, opt1, batches[0])
            opt1.update()
        want = []
        for k, (s, upd) in enumerate(plan):
            if k == 3:
                opt1.lr = 1e-3
            want.append(float(_micro(m1, opt1, batches[s])))
            if upd:
                opt1.update()
        m2, opt2 = _fresh()
        gs = cti_amd.GraphedTrainStep(m2, opt2, loss_fn, batches[0][:3], batches[0][3], warmup=2, accumulate=True)
        got = []
        for k, (s, upd) in enumerate(plan):
            if k == 3:
                opt2.param_groups[0]["lr"] = 1e-3
            got.append(float(gs(batches[s][:3], batches[s][3], update_params=upd)))
            assert (opt2.micro_count == 0) == upd
        assert opt1.steps_done() == 5 and opt2.steps_done() == 5
        assert int(opt2.micro_dev.item()) == 0
        assert torch.allclose(opt1.flat_p, opt2.flat_p, rtol=1e-5, atol=1e-7)
        print("losses eager", want, "replayed", got)
        assert len(set(got)) == len(got)
        assert np.allclose(got, want, rtol=1e-4, atol=0)                     # each returned loss is its own micro-batch's
        # gs.update() alone: a micro-batch fed eagerly, then the collective + graph U
        _micro(m1, opt1, batches[0]); opt1.update()
        _micro(m2, opt2, batches[0]); gs.update()
        assert torch.allclose(opt1.flat_p, opt2.flat_p, rtol=1e-5, atol=1e-7)
        with pytest.raises(RuntimeError):
            gs.update()
        # a replayed and an eagerly fed micro-batch in ONE update (the eager forward right behind a buffering replay must see the current parameters)
        _micro(m1, opt1, batches[1]); _micro(m1, opt1, batches[2]); opt1.update()
        gs(batches[1][:3], batches[1][3], update_params=False); _micro(m2, opt2, batches[2]); gs.update()
        assert torch.allclose(opt1.flat_p, opt2.flat_p, rtol=1e-5, atol=1e-7)
        m3, opt3 = _fresh(freq=2)
        with pytest.raises(ValueError):
            cti_amd.GraphedTrainStep(m3, opt3, loss_fn, batches[0][:3], batches[0][3], warmup=0)
    finally:
        cti_amd.set_precision("bf16x3")


class _Drop(nn.Module):
    def __init__(self):
        super().__init__()
        self.net = cti_amd.FCNet([40, 40], "ReLU", 0.5)

    def forward(self, x):
        return self.net(x)


def test_replayed_micro_batches_draw_their_own_dropout_masks():
    torch.manual_seed(5)
    m = _Drop().to(DEV).train()
    opt = cti_amd.FlatAdamaxDP(m, lr=1e-3, clip_norm=0.25)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(16, 40, generator=g).to(DEV)
    y = torch.randn(16, 40, generator=g).to(DEV)
    mse = lambda out, t: ((out - t) ** 2).sum() / out.size(0)          # noqa: E731
    gs = cti_amd.GraphedTrainStep(m, opt, mse, (x,), y, warmup=2, accumulate=True)
    l1 = float(gs((x,), y, update_params=False))
    g1 = opt.flat_g.clone()
    l2 = float(gs((x,), y, update_params=False))
    g2 = opt.flat_g.clone()
    assert l1 != l2
    assert float(g1.abs().max()) > 0
    assert not torch.allclose(g2, 2 * g1, rtol=1e-3, atol=1e-6)
    gs.update()
    assert int(opt.micro_dev.item()) == 0
