"""Trainer / MCTrainer (the object of src/FFOE/train.py:50-82 and src/MC/train.py:47-87) on the tiny models of the g9 fixtures against the reference
recipe restated on stock torch: autograd accumulation over the buffered micro-batches, divide by the number buffered (src/FFOE/trainer.py:112,126), clip by
max_norm / (norm + 1e-6) (src/utils.py:323-328), torch.optim.Adamax on a copy of the model.  Tolerances as in tests/test_dp_gpu.py.  Needs an MI355X."""
import types

import pytest
import torch
import torch.nn as nn

import cti_amd
from golden_util import model_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
CLIP = 0.25


class _DS:
    def __init__(self, ntoken, v_dim, num_ans):
        self.dictionary = types.SimpleNamespace(ntoken=ntoken)
        self.v_dim = v_dim
        self.num_ans_candidates = num_ans


def _pair(name, builder):
    """Two copies of the fixture's model with the same parameters, every nn.Dropout at p = 0, in train mode on the device."""
    fx, p = model_case(name)
    c = fx.cfg
    out = []
    for _ in range(2):
        m = getattr(cti_amd, builder)(types.SimpleNamespace(**c["args"]), _DS(c["ntoken"], c["v_dim"], c["num_ans"]))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, strict=True)
        for mod in m.modules():
            if isinstance(mod, nn.Dropout):
                mod.p = 0.0
        out.append(m.to(DEV).train())
    return c, out[0], out[1]


def _ffoe_sample(c, B, seed):
    """[v, b, q, a, ans, t_logits] on the HOST (train_step moves it).  The soft scores are multiples of 1/8: their sums are exact in fp32 in any order,
    so the batch score compares the scoring RULE with `==`, not the association of a float sum."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, c["V"], c["v_dim"], generator=g).abs()
    v[:, c["V"] - 2:] = 0
    b = torch.rand(B, c["V"], 6, generator=g)
    q = torch.randint(0, c["ntoken"], (B, c["Q"]), generator=g)
    ans = torch.randint(0, c["ntoken"], (B, c["A"]), generator=g)
    a = torch.randint(0, 9, (B, c["num_ans"]), generator=g).float() / 8 * (torch.rand(B, c["num_ans"], generator=g) < 0.4).float()
    t = torch.randn(B, c["num_ans"], generator=g)
    return [v, b, q, a, ans, t]


def _args(model, gamma, distillation=False):
    return types.SimpleNamespace(device=DEV, model=model, distillation=distillation, clip_norm=CLIP, gamma=gamma)


def _trainable(m):
    return [p for p in m.parameters() if p.requires_grad]


def _ref_update(m2, opt2, buffered):
    """flat grads / number buffered, clip, Adamax, zero_grad (src/FFOE/trainer.py:221-269); returns the pre-clip norm."""
    grads = [p.grad for p in _trainable(m2) if p.grad is not None]
    for gr in grads:
        gr.div_(buffered)
    norm = torch.cat([gr.reshape(-1) for gr in grads]).norm()
    coef = CLIP / (norm + 1e-6)
    if coef < 1:
        for gr in grads:
            gr.mul_(coef)
    opt2.step()
    opt2.zero_grad()
    return float(norm)


def _close(x, ref, rel):
    x, ref = (float(t.detach()) if isinstance(t, torch.Tensor) else float(t) for t in (x, ref))
    return abs(x - ref) <= rel * abs(ref)


def _same_parameters(m1, m2):
    for (n1, p1), (n2, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert n1 == n2
        assert torch.allclose(p1, p2, rtol=1e-4, atol=2e-6), n1


def test_ffoe_trainer_follows_the_reference_loop_with_update_freq_two_and_a_short_last_batch():
    cti_amd.set_precision("fp32")
    try:
        c, m1, m2 = _pair("g9_ffoe_cti", "build_cti")
        crit = nn.BCEWithLogitsLoss(reduction="sum")                          # src/FFOE/train.py:40
        trainer = cti_amd.Trainer(_args("cti", 2), m1, crit, torch.optim.Adamax(_trainable(m1), lr=2e-3))
        assert isinstance(trainer.optimizer, cti_amd.FlatAdamaxDP) and abs(trainer.optimizer.param_groups[0]["lr"] - 2e-3) < 1e-12
        opt2 = torch.optim.Adamax(_trainable(m2), lr=2e-3)
        opt2.zero_grad()
        sizes, update_freq, batch_size = [8, 8, 8, 8, 5], 2, 8
        num_batches = int(sum(sizes) / batch_size + 1)                       # train.py:61
        assert num_batches == len(sizes)
        buffered, updates, sums = 0, 0, [0.0, 0.0, 0.0]
        for i, B in enumerate(sizes):
            sample = _ffoe_sample(c, B, 500 + i)
            v, _, q, a, ans, _ = (t.to(DEV) for t in sample)
            preds = m2(v, q, ans)
            ref_loss = crit(preds.float(), a) / a.size(0)
            ref_loss.backward()
            buffered += 1
            if i < num_batches - 1 and (i + 1) % update_freq > 0:            # train.py:78
                assert trainer.train_step(sample, update_params=False) is None
            else:
                loss, grad_norm, batch_score = trainer.train_step(sample, update_params=True)
                ref_norm = _ref_update(m2, opt2, buffered)
                assert (updates, buffered) in ((0, 2), (1, 2), (2, 1))
                buffered, updates = 0, updates + 1
                for t in (loss, grad_norm, batch_score):
                    assert t.dim() == 0 and t.is_cuda
                print("update %d: loss %.8g ref %.8g  norm %.8g ref %.8g" % (updates, float(loss), float(ref_loss.detach()), float(grad_norm), ref_norm))
                assert _close(loss, ref_loss, 1e-5)
                assert _close(grad_norm, ref_norm, 1e-4)
                assert float(batch_score) == float(cti_amd.compute_score_with_logits(preds.detach(), a).sum())
                sums = [sums[0] + float(loss), sums[1] + float(batch_score), sums[2] + float(grad_norm)]
            assert trainer.graphed == (i >= 2)                               # captured by the third same-shaped call
        assert trainer.captures == 1 and updates == 3 and trainer.get_num_updates() == 3
        _same_parameters(m1, m2)
        r = trainer.meter.result()
        assert r["updates"] == 3 and r["samples"] == 8 + 8 + 5
        assert _close(r["loss"], sums[0], 1e-6) and r["score"] == sums[1] and _close(r["grad_norm"], sums[2], 1e-6)
    finally:
        cti_amd.set_precision("bf16x3")


def test_ffoe_ban_trainer_with_distillation():
    cti_amd.set_precision("fp32")
    try:
        c, m1, m2 = _pair("g9_ffoe_ban", "build_ban")
        crit = cti_amd.Distillation_Loss(T=3.0, alpha=0.5)
        trainer = cti_amd.Trainer(_args("ban", 3, distillation=True), m1, crit, torch.optim.Adamax(_trainable(m1), lr=2e-3))
        opt2 = torch.optim.Adamax(_trainable(m2), lr=2e-3)
        opt2.zero_grad()
        sample = _ffoe_sample(c, 8, 600)
        v, b, q, a, _, t = (x.to(DEV) for x in sample)
        preds = m2(v, b, q, a)[0]
        ref_loss = crit(preds.float(), t.float(), a)                         # not divided again (src/FFOE/trainer.py:170-171)
        ref_loss.backward()
        loss, grad_norm, batch_score = trainer.train_step(sample, update_params=True)
        ref_norm = _ref_update(m2, opt2, 1)
        print("loss %.8g ref %.8g  norm %.8g ref %.8g" % (float(loss), float(ref_loss.detach()), float(grad_norm), ref_norm))
        assert _close(loss, ref_loss, 1e-5) and _close(grad_norm, ref_norm, 1e-4)
        assert float(batch_score) == float(cti_amd.compute_score_with_logits(preds.detach(), a).sum())
        _same_parameters(m1, m2)
    finally:
        cti_amd.set_precision("bf16x3")


def test_mc_trainer_dummy_step_then_two_updating_steps():
    cti_amd.set_precision("fp32")
    try:
        c, m1, m2 = _pair("g9_mc_cti", "build_mc_cti")
        crit = nn.BCEWithLogitsLoss(reduction="sum")
        trainer = cti_amd.MCTrainer(_args("cti", 2), m1, crit, torch.optim.Adamax(_trainable(m1), lr=2e-3))
        opt2 = torch.optim.Adamax(_trainable(m2), lr=2e-3)
        opt2.zero_grad()
        for step in range(2):
            g = torch.Generator().manual_seed(700 + step)
            B0 = 2                                                           # images; every one once per candidate answer (src/MC/train.py:74-83)
            v = torch.randn(B0, c["V"], c["v_dim"], generator=g).abs()
            v[:, c["V"] - 2:] = 0
            v = v.unsqueeze(1).expand(B0, 4, c["V"], c["v_dim"]).contiguous().view(B0 * 4, c["V"], c["v_dim"])
            b = torch.rand(B0 * 4, c["V"], 6, generator=g)
            q = torch.randint(0, c["ntoken"], (B0, c["Q"]), generator=g)
            q = q.unsqueeze(1).expand(B0, 4, c["Q"]).contiguous().view(B0 * 4, c["Q"])
            ans_mc = torch.randint(0, c["ntoken"], (B0 * 4, c["A"]), generator=g)
            a = torch.zeros(B0 * 4, 1)
            a[torch.arange(B0) * 4 + torch.randint(0, 4, (B0,), generator=g)] = 1
            labels = torch.cat([a, 1 - a], 1)
            sample = [v, b, q, labels, ans_mc]
            if step == 0:
                # the allocator warm-up of the reference's loops: a micro-step whose gradients are dropped; the reference run never sees it
                before = trainer.optimizer.flat_p.clone()
                trainer.dummy_train_step(sample)
                assert trainer.optimizer.micro_count == 0 and int(trainer.optimizer.micro_dev.item()) == 0
                assert torch.equal(trainer.optimizer.flat_p, before)
            dv, db, dq, dl, da = (x.to(DEV) for x in sample)
            preds = m2(dv, db, dq, da)[0]
            ref_loss = crit(preds.float(), dl) / dl.size(0)
            ref_loss.backward()
            loss, grad_norm, batch_score = trainer.train_step(sample, update_params=True)
            ref_norm = _ref_update(m2, opt2, 1)
            print("step %d: loss %.8g ref %.8g  norm %.8g ref %.8g" % (step, float(loss), float(ref_loss.detach()), float(grad_norm), ref_norm))
            assert _close(loss, ref_loss, 1e-5) and _close(grad_norm, ref_norm, 1e-4)
            assert float(batch_score) == float(cti_amd.compute_score_mc(preds.detach(), dl).sum())
        _same_parameters(m1, m2)
        assert trainer.meter.result()["updates"] == 2 and trainer.get_num_updates() == 2
        assert trainer.graphed and trainer.captures == 1                     # dummy + first step eager, the second step replayed
    finally:
        cti_amd.set_precision("bf16x3")
