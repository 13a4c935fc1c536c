"""The counting module on an MI355X: Counter (csrc/cti_counter.hip) against the reference's float64 outputs and gradients
(tests/golden/g14_cnt_*, make_golden_counter.py), the two BAN models built with a counter against the reference's (g14_*_ban_cnt*), the
glimpse loops against each other at real widths, strided inputs, reproducibility, hipGraph replay, the absence of aten arithmetic in an eval
forward and of any counter work in a model without one.

Tolerance: the project's bar, normalised max error <= 1e-4 against the float64 fixture values for the output and every gradient (the kernels are
fp32 throughout; the reference's own fp32 run sits at <= 1.4e-5).  Model-level checks use the tolerances of tests/test_models_gpu.py."""
import collections
import types

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import cti_amd
from cti_amd import ops
from golden_util import load, model_case
from oracle.cti_oracle import norm_max_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
UNIT = ["rand", "ones_v100", "v10", "padded", "sigmoided", "obj5", "negw"]


@pytest.fixture
def mode(request):
    old = cti_amd.get_precision()
    cti_amd.set_precision(request.param)
    yield request.param
    cti_amd.set_precision(old)


class _DS:
    def __init__(self, ntoken, v_dim, num_ans):
        self.dictionary = types.SimpleNamespace(ntoken=ntoken)
        self.v_dim = v_dim
        self.num_ans_candidates = num_ans


def T(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t.requires_grad_(True) if grad else t


def check(x, ref, tol=TOL, what=""):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    assert x.shape == tuple(np.shape(ref)), (what, x.shape, np.shape(ref))
    e = norm_max_err(x, ref)
    print("%-40s normalised max error %.3g" % (what, e))
    assert e <= tol, "%s: normalised max error %.3g > %.3g" % (what, e, tol)
    return e


def counter_of(fx):
    c = cti_amd.Counter(fx.cfg["objects"], already_sigmoided=fx.cfg["already_sigmoided"])
    with torch.no_grad():
        for f, w in zip(c.f, fx.p["weights"]):
            f.weight.copy_(torch.from_numpy(w))
    return c.to(DEV)


def boxes_of(fx):
    return T(fx.i["boxes"])[:, :, :4].transpose(1, 2)                        # the models' view of the stored rows


# ---- unit fixtures ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", UNIT)
def test_counter_matches_reference(name):
    fx = load("g14_cnt_" + name)
    c = counter_of(fx)
    with torch.no_grad():
        out = c(boxes_of(fx), T(fx.i["att"]))
    check(out, fx.o["out"], TOL, name + " out")
    att = T(fx.i["att"], grad=True)
    out2 = c(boxes_of(fx), att)
    assert torch.equal(out2.detach(), out)                                    # the autograd path runs the same launch
    (out2 * T(fx.i["gup"])).sum().backward()
    check(att.grad, fx.g["att"], TOL, name + " d attention")
    check(torch.stack([f.weight.grad for f in c.f]), fx.g["weights"], TOL, name + " d weights")
    if fx.cfg["real"] is not None:                                            # masked boxes: finite output, exactly zero gradient
        assert torch.isfinite(out).all() and float(att.grad[:, fx.cfg["real"]:].abs().max()) == 0.0


def test_counter_on_a_logit_block_matches_reference():
    fx = load("g14_cnt_block")
    c = counter_of(fx)
    b = T(fx.i["boxes"])
    with torch.no_grad():
        out = c.forward_logits(b, T(fx.i["att"]))
    check(out, fx.o["out"], TOL, "block out")
    lg = T(fx.i["att"], grad=True)
    out2 = c.forward_logits(b, lg)
    (out2 * T(fx.i["gup"])).sum().backward()
    check(lg.grad, fx.g["att"], TOL, "block d logits")
    check(torch.stack([f.weight.grad for f in c.f]), fx.g["weights"], TOL, "block d weights")
    # per glimpse through the plain module call on the reduced scores: the same numbers
    with torch.no_grad():
        for g in range(lg.shape[1]):
            one = c(b[:, :, :4].transpose(1, 2), lg.detach()[:, g].max(2)[0])
            assert torch.equal(one, out[:, g])


def test_all_masked_sample_gives_the_finite_count_zero_row():
    fx = load("g14_cnt_allinf")
    c = counter_of(fx)
    with torch.no_grad():
        out = c(boxes_of(fx), T(fx.i["att"]))
    assert torch.isfinite(out).all()
    check(out, fx.o["out"], TOL, "allinf out")
    row = out[fx.cfg["allinf"]].cpu().numpy()
    assert row[0] > 0 and np.abs(row[2:]).max() == 0.0


def test_ties_go_to_the_lower_box_index():
    V, m = 14, 10
    rs = np.random.RandomState(3)
    xy = rs.uniform(0, .6, size=(1, V, 2)); wh = rs.uniform(.05, .4, size=(1, V, 2))
    boxes = np.concatenate([xy, xy + wh], 2).astype(np.float32)
    att = np.full((1, V), 0.25, np.float32)                                  # every score equal: boxes 0 .. 9 are kept
    att[0, 12] = 2.0                                                         # ... after the one real maximum
    c = cti_amd.Counter(m).to(DEV)
    a = T(att, grad=True)
    out = c(T(boxes).transpose(1, 2), a)
    out.sum().backward()
    _, save = ops.counter_fwd(T(boxes).transpose(1, 2), T(att), [f.weight.detach() for f in c.f], m)
    assert save[:m].cpu().tolist() == [12] + list(range(9))
    ref = cti_amd.Counter(m).to(DEV)
    keep = [12] + list(range(9))
    with torch.no_grad():
        out_ref = ref(T(boxes[:, keep]).transpose(1, 2), T(att[:, keep]))
    assert torch.equal(out.detach(), out_ref)


def test_strided_inputs_equal_contiguous_copies_bit_for_bit_and_backward_is_reproducible():
    fx = load("g14_cnt_block")
    c = counter_of(fx)
    b = T(fx.i["boxes"])
    ws = [f.weight.detach() for f in c.f]
    lg = T(fx.i["att"])
    view = b[:, :, :4].transpose(1, 2)
    gup = T(fx.i["gup"])
    for g in range(lg.shape[1]):
        sl = lg[:, g:g + 1]                                                  # a glimpse of the block, read in place
        o1, s1 = ops.counter_fwd(view, sl, ws, 10)
        o2, s2 = ops.counter_fwd(view.contiguous(), sl.contiguous(), ws, 10)
        assert torch.equal(o1, o2) and torch.equal(s1, s2)
        r1 = ops.counter_bwd(gup[:, g:g + 1].contiguous(), view, ws, s1, 10, tuple(sl.shape))
        r2 = ops.counter_bwd(gup[:, g:g + 1].contiguous(), view.contiguous(), ws, s2, 10, tuple(sl.shape))
        r3 = ops.counter_bwd(gup[:, g:g + 1].contiguous(), view, ws, s1, 10, tuple(sl.shape))
        for x, y, z in zip(r1, r2, r3):
            assert torch.equal(x, y) and torch.equal(x, z)                    # no float atomics: bitwise from run to run
    with pytest.raises(ValueError):
        ops.counter_fwd(view[:, :, :9], lg[:, 0, :9, 0], ws, 10)              # fewer boxes than objects


def test_count_projection_takes_eleven_inputs():
    """c_prj[g]: an 11 -> num_hid weight-normalised Linear + ReLU on a strided (B, 11) view, forward and both gradient products, in every
    arithmetic mode, against float64."""
    rs = np.random.RandomState(11)
    B, G, H = 37, 3, 64
    x = rs.uniform(0, 1, size=(B, G, 11)).astype(np.float32)
    gy = rs.standard_normal(size=(B, H)).astype(np.float32)
    old = cti_amd.get_precision()
    try:
        for prec, tol in (("fp32", 1e-5), ("bf16x3", 1e-4), ("bf16", 2e-2)):
            cti_amd.set_precision(prec)
            torch.manual_seed(1)
            net = cti_amd.FCNet([11, H], 'ReLU', .0).to(DEV)
            lin = net.main[0]
            W = lin.weight_v.detach().double().cpu().numpy()
            s = float(lin.weight_g.detach()) / np.linalg.norm(W)
            xt = T(x, grad=True)
            with torch.no_grad():
                y0 = net(xt.detach()[:, 1])
            y = net(xt[:, 1])
            pre = x[:, 1].astype(np.float64) @ (s * W).T + lin.bias.detach().double().cpu().numpy()
            ref = np.maximum(pre, 0)
            check(y0, ref, tol, "c_prj eval [%s]" % prec)
            check(y, ref, tol, "c_prj autograd [%s]" % prec)
            (y * T(gy)).sum().backward()
            on = y.detach().cpu().numpy() > 0                                # the forward's own activation pattern: a pre-activation within the mode's
            assert np.array_equal(on, pre > 0) or prec == "bf16"             # rounding of 0 may fall on either side in the plain-bf16 mode
            assert (np.abs(pre[on != (pre > 0)]) <= tol * np.abs(pre).max()).all()
            dz = gy * on
            dx = np.zeros_like(x, dtype=np.float64)
            dx[:, 1] = dz @ (s * W)
            check(xt.grad, dx, tol, "c_prj dx [%s]" % prec)
            check(lin.bias.grad, dz.sum(0), tol, "c_prj dbias [%s]" % prec)
            Gm = dz.T @ x[:, 1].astype(np.float64)
            nv = np.linalg.norm(W)
            dg = (Gm * W).sum() / nv
            dV = s * Gm - (float(lin.weight_g.detach()) * (Gm * W).sum() / nv ** 3) * W
            check(lin.weight_v.grad, dV, tol, "c_prj dV [%s]" % prec)
            assert abs(float(lin.weight_g.grad) - dg) <= tol * max(1.0, abs(dg))
    finally:
        cti_amd.set_precision(old)


# ---- models -------------------------------------------------------------------------------------------------------------------------------
def build_model(name, counter=True):
    fx, p = model_case(name)
    c = fx.cfg
    a = dict(c["args"])
    ds = _DS(c["ntoken"], c["v_dim"], c["num_ans"])
    if "mc" in name:
        a["use_counter"] = counter
        m = cti_amd.build_mc_ban(types.SimpleNamespace(**a), ds)
    else:
        a["use_counter"] = False
        m = cti_amd.build_ban(types.SimpleNamespace(**a), ds, counter=cti_amd.Counter(10) if counter else None)
    if counter:
        m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, strict=True)
    else:
        m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items() if not (k.startswith("c_prj") or k.startswith("counter"))}, strict=True)
    return fx, m.to(DEV).eval()


def run_model(m, fx):
    if "ans" in fx.i and "mc" in fx.name:
        return m(T(fx.i["v"]), T(fx.i["b"]), T(fx.i["q"]), T(fx.i["ans"]))
    return m(T(fx.i["v"]), T(fx.i["b"]), T(fx.i["q"]), None)


@pytest.mark.parametrize("mode,tol", [("fp32", 1e-4), ("bf16x3", 1e-4), ("bf16", 2e-2)], indirect=["mode"])
@pytest.mark.parametrize("name", ["g14_ffoe_ban_cnt", "g14_mc_ban_cnt"])
def test_ban_models_with_a_counter(name, mode, tol):
    fx, m = build_model(name)
    with torch.no_grad():
        out, att = run_model(m, fx)
    check(out, fx.o["logits"], tol, "%s logits [%s]" % (name, mode))
    check(att, fx.o["att"], tol, "%s att [%s]" % (name, mode))
    out2, att2 = run_model(m, fx)                                            # autograd on: the literal loop through the Fn wrappers
    check(out2, fx.o["logits"], tol, "%s logits, autograd path [%s]" % (name, mode))
    out2.sum().backward()
    for k, prm in m.named_parameters():
        if k.startswith("counter") or k.startswith("c_prj"):
            assert prm.grad is not None and torch.isfinite(prm.grad).all(), k


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"], indirect=True)
def test_ffoe_ban_counter_train_step_matches_reference(mode):
    fx, m = build_model("g14_ffoe_ban_cnt_step")
    c = fx.cfg
    v, b, q, tgt = T(fx.i["v"]), T(fx.i["b"]), T(fx.i["q"]), T(fx.i["target"])
    opt = cti_amd.FlatAdamaxDP(m, lr=c["lr"], clip_norm=c["clip_norm"])
    opt.zero_grad()
    out, _ = m(v, b, q, None)
    check(out, fx.o["logits"], 1e-4, "logits")
    loss = cti_amd.BCEWithLogitsSum()(out, tgt) / c["B"]
    assert abs(float(loss) - float(fx.o["loss"])) < 1e-4 * float(fx.o["loss"])
    loss.backward()
    named = dict(m.named_parameters())
    assert any(n.startswith("counter.f.") for n in c["used"]) and any(n.startswith("c_prj.") for n in c["used"])
    prs = np.random.RandomState(c["proj_seed"])
    proj = {n: prs.standard_normal(size=tuple(prm.shape)).astype(np.float32) for n, prm in m.named_parameters() if prm.requires_grad}
    got_n = np.array([float(named[n].grad.norm()) for n in c["used"]])
    got_p = np.array([float((named[n].grad.double().cpu() * torch.from_numpy(proj[n]).double()).sum()) for n in c["used"]])
    ref_n, ref_p = fx.o["gnorm"], fx.o["gproj"]
    e_n = np.max(np.abs(got_n - ref_n) / (ref_n + 1e-3 * ref_n.max()))
    e_p = np.max(np.abs(got_p - ref_p)) / np.max(np.abs(ref_p))
    print("g14 BAN + counter train step [%s]: worst per-parameter gradient-norm deviation %.3g (%s), projection deviation %.3g"
          % (mode, e_n, c["used"][int(np.argmax(np.abs(got_n - ref_n) / (ref_n + 1e-3 * ref_n.max())))], e_p))
    assert e_n < 1e-4, "per-parameter gradient norms"
    assert e_p < 1e-4, "per-parameter gradient projections"
    opt.step()
    assert abs(float(opt.grad_norm) - float(fx.o["grad_norm"])) < 1e-4 * float(fx.o["grad_norm"])
    with torch.no_grad():
        loss2 = cti_amd.BCEWithLogitsSum()(m(v, b, q, None)[0], tgt) / c["B"]
    assert abs(float(loss2) - float(fx.o["loss_after"])) < 2e-4 * float(fx.o["loss_after"])


def _real_ban(counter, G=8, H=1024, Dv=2048, n_ans=3129, ntok=300):
    args = types.SimpleNamespace(op="", num_hid=H, gamma=G, activation="relu", dropout=0.5, use_counter=False)
    torch.manual_seed(0)
    return cti_amd.build_ban(args, _DS(ntok, Dv, n_ans), counter=cti_amd.Counter(10) if counter else None).to(DEV).eval()


def _real_inputs(B=256, V=36, Dv=2048, ntok=300):
    rs = np.random.RandomState(7)
    v = np.abs(rs.standard_normal(size=(B, V, Dv))).astype(np.float32)
    xy = rs.uniform(0, .6, size=(B, V, 2)); wh = rs.uniform(.05, .4, size=(B, V, 2))
    b = np.concatenate([xy, xy + wh, rs.uniform(size=(B, V, 2))], 2).astype(np.float32)
    for i in range(B):
        v[i, 10 + i % 27:] = 0
        b[i, 10 + i % 27:] = 0
    q = rs.randint(0, ntok, size=(B, 14)).astype(np.int64)
    return T(v), T(b), T(q)


def test_glimpse_loops_agree_at_real_widths_and_the_counter_is_one_launch():
    """B = 256, V = 36, 8 glimpses, num_hid 1024 in the bf16x3 mode: the hoisted loop (what a model with a counter takes in inference) against the
    literal loop, and the count terms must matter.  One counter launch per forward, not one per glimpse."""
    old = cti_amd.get_precision()
    cti_amd.set_precision("bf16x3")
    bm = cti_amd.pkg.glimpse_loops
    try:
        m = _real_ban(True)
        with torch.no_grad():
            for f in m.counter.f:
                f.weight.copy_(torch.rand(17, device=DEV) + 0.2)
        v, b, q = _real_inputs()
        seen = []
        orig = bm._ban_forward_hoisted

        def spy(self, *a, **k):
            r = orig(self, *a, **k)
            seen.append(r is not None)
            return r
        bm._ban_forward_hoisted = spy
        with torch.no_grad():
            m(v, b, q, None)
            ops.profile_start()
            hoisted, att = m(v, b, q, None)
            prof = ops.profile_stop()
        bm._ban_forward_hoisted = orig
        assert seen and all(seen)                                               # the hoisted loop ran (not a silent fall-through to the literal one)
        launches = [k for k in prof if k.startswith("counter_fwd")]
        assert len(launches) == 1 and len(prof[launches[0]]) == 1, prof.keys()
        hoist_flag = bm._HOIST_LOOP
        bm._HOIST_LOOP = False
        try:
            with torch.no_grad():
                literal, att2 = m(v, b, q, None)
        finally:
            bm._HOIST_LOOP = hoist_flag
        assert torch.equal(att, att2)
        check(hoisted, literal.cpu().numpy(), 1e-4, "hoisted vs literal loop with a counter")
        counter = m.counter
        m.counter = None                                                        # the same weights without the count terms: a different answer
        try:
            with torch.no_grad():
                plain, _ = m(v, b, q, None)
        finally:
            m.counter = counter
        assert norm_max_err(plain.cpu().numpy(), literal.cpu().numpy()) > 1e-3
    finally:
        cti_amd.set_precision(old)


def test_graphed_forward_replays_bit_for_bit():
    fx, m = build_model("g14_ffoe_ban_cnt")
    v, b, q = T(fx.i["v"]), T(fx.i["b"]), T(fx.i["q"])
    old = cti_amd.get_precision()
    cti_amd.set_precision("bf16x3")
    try:
        g = cti_amd.GraphedForward(lambda v_, b_, q_: m(v_, b_, q_, None)[0], (v, b, q))
        v2, b2, q2 = torch.roll(v, 1, 0) * 1.3, torch.roll(b, 1, 0), torch.roll(q, 1, 0)
        with torch.no_grad():
            ref1, ref2 = m(v2, b2, q2, None)[0].clone(), m(v, b, q, None)[0].clone()
        out = g(v2, b2, q2)
        torch.cuda.synchronize()
        assert torch.equal(out, ref1)
        out = g(v, b, q)
        torch.cuda.synchronize()
        assert torch.equal(out, ref2)
    finally:
        cti_amd.set_precision(old)


def test_graphed_train_step_runs_on_a_model_with_a_counter():
    fx, m = build_model("g14_ffoe_ban_cnt_step")
    c = fx.cfg
    v, b, q, tgt = T(fx.i["v"]), T(fx.i["b"]), T(fx.i["q"]), T(fx.i["target"])
    old = cti_amd.get_precision()
    cti_amd.set_precision("bf16x3")
    try:
        opt = cti_amd.FlatAdamaxDP(m, lr=c["lr"], clip_norm=c["clip_norm"])
        crit = cti_amd.BCEWithLogitsSum()
        w0 = m.counter.f[3].weight.detach().clone()
        step = cti_amd.GraphedTrainStep(m, opt, lambda o, t: crit(o[0], t) / c["B"], (v, b, q, torch.zeros(1, device=DEV)), tgt, warmup=1)
        losses = [float(step((v, b, q, torch.zeros(1, device=DEV)), tgt)) for _ in range(4)]
        torch.cuda.synchronize()
        assert all(np.isfinite(losses)) and losses[-1] < losses[0]
        assert not torch.equal(w0, m.counter.f[3].weight.detach())              # the counter's weights are in the flat buffers and move
    finally:
        cti_amd.set_precision(old)


_ALLOWED = {"view", "_unsafe_view", "slice", "select", "detach", "alias", "expand", "as_strided", "t", "transpose", "unsqueeze", "squeeze",
            "reshape", "permute", "empty", "empty_like", "empty_strided", "new_empty", "sym_size", "sym_stride", "is_pinned", "record_stream",
            "unbind", "split", "fill_", "fill", "zero_", "zeros", "zeros_like", "copy_", "_to_copy", "clone"}


class _Spy(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.seen = collections.Counter()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        base = name.split(".")[1] if name.count(".") >= 1 else name
        if base not in _ALLOWED:
            self.seen[name] += 1
        return func(*args, **(kwargs or {}))


@pytest.mark.parametrize("mode", ["bf16x3", "bf16", "fp32"], indirect=True)
def test_second_eval_forward_runs_no_aten_arithmetic(mode):
    fx, m = build_model("g14_ffoe_ban_cnt")
    fx2, m2 = build_model("g14_mc_ban_cnt")
    a1 = (T(fx.i["v"]), T(fx.i["b"]), T(fx.i["q"]), None)
    a2 = (T(fx2.i["v"]), T(fx2.i["b"]), T(fx2.i["q"]), T(fx2.i["ans"]))
    with torch.no_grad():
        m(*a1)
        m2(*a2)
        torch.cuda.synchronize()
        with _Spy() as spy:
            m(*a1)
            m2(*a2)
        torch.cuda.synchronize()
    assert not spy.seen, dict(spy.seen)


@pytest.mark.parametrize("name", ["g14_ffoe_ban_cnt", "g14_mc_ban_cnt"])
def test_a_model_without_a_counter_runs_no_counter_work(name):
    fx, m = build_model(name, counter=False)
    assert m.counter is None and not hasattr(m, "c_prj")
    with torch.no_grad():
        run_model(m, fx)
        ops.profile_start()
        out, _ = run_model(m, fx)
        prof = ops.profile_stop()
    assert torch.isfinite(out).all()
    assert not [k for k in prof if k.startswith("counter")], prof.keys()
    fx2, m2 = build_model(name, counter=True)
    with torch.no_grad():
        run_model(m2, fx2)
        ops.profile_start()
        run_model(m2, fx2)
        prof2 = ops.profile_stop()
    names = [k for k in prof2 if k.startswith("counter_fwd")]
    assert len(names) == 1 and len(prof2[names[0]]) == 1                     # ONE launch for every glimpse of the batch
