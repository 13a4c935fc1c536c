"""The SAN baseline on an MI355X: StackedAttention and the two SAN models against the reference's outputs and gradients
(tests/golden/g13_*, make_golden_san.py), the attention step (csrc/cti_san.hip) against a float64 evaluation written here, the real FFOE
widths, cache invalidation, hipGraph replay and the absence of aten arithmetic in an eval forward."""
import collections
import types

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import cti_amd
from cti_amd import ops
from golden_util import load
from oracle import cti_models as M
from oracle.cti_oracle import norm_max_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {"fp32": 1e-4, "bf16x3": 1e-4, "bf16": 2e-2}


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


def check(x, ref, tol, what=""):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    assert x.shape == tuple(np.shape(ref)), (what, x.shape, np.shape(ref))
    e = norm_max_err(x, ref)
    assert e <= tol, "%s: normalised max error %.3g > %.3g" % (what, e, tol)
    return e


def logit_bias(name):
    """The bias of a logit layer (fc13, layers[3s+2]): softmax does not see a constant shift, so its gradient is zero up to rounding."""
    parts = name.split(".")
    return parts[-1] == "bias" and (parts[-2] == "fc13" or (len(parts) >= 3 and parts[-3] == "layers" and int(parts[-2]) % 3 == 2))


def check_zero(x, ref, scale, tol, what=""):
    """A mathematically zero gradient: both sides are rounding noise, compared at tol times the scale of their layer's other gradients."""
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    assert x.shape == tuple(np.shape(ref)), (what, x.shape, np.shape(ref))
    assert np.abs(x.astype(np.float64) - ref).max() <= tol * scale, (what, x, ref, scale)


def san_state(keys_shapes, seed):
    """Identical copy of tests/golden/make_golden_san.py:san_state."""
    rs = np.random.RandomState(seed)
    shapes = {k: tuple(s) for k, s in keys_shapes}
    new = {}

    def normal(shape, scale):
        return (rs.standard_normal(size=shape).astype(np.float32) * np.float32(scale)).reshape(shape)

    for k, shape in keys_shapes:
        shape = tuple(shape)
        if ".rnn.weight" in k:
            x = normal(shape, 1.0 / np.sqrt(shape[-1]))
        elif ".rnn.bias" in k:
            x = normal(shape, 0.1)
        elif k.endswith("emb.weight") or k.endswith("emb_.weight"):
            x = normal(shape, 0.5)
        elif k.endswith("weight_v"):
            x = normal(shape, 1.0 / np.sqrt(shape[-1]))
        elif k.endswith("weight_g"):
            x = np.float32((abs(rs.standard_normal()) + 0.5) * np.sqrt(shapes[k[:-1] + "v"][0]))
        elif k.endswith("bias"):
            x = normal(shape, 0.1)
        else:
            x = normal(shape, 1.0)
        if "_att." in k and k.endswith(".weight"):
            x = x * np.float32(1.0 / np.sqrt(shape[-1]))
        new[k] = np.asarray(x, dtype=np.float32).reshape(shape)
    return new


def build_model(name, builder):
    fx = load(name)
    c = fx.cfg
    p = san_state([(k, tuple(s)) for k, s in c["state_keys"]], c["seed"])
    m = getattr(cti_amd, builder)(types.SimpleNamespace(**c["args"]), _DS(c["ntoken"], c["v_dim"], c["num_ans"]))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, strict=True)
    return fx, p, m.to(DEV).eval()


# ---- float64 statements of the reference (src/attention.py:90-152) ---------------------------------------------------------------------
def step64(P, qv, w, b, X, keep=None, p_drop=0.0, v_mask=True):
    P, qv, w, X = (np.asarray(t, np.float64) for t in (P, qv, w, X))
    h = np.tanh(qv[:, None, :] + P)
    s = np.ones_like(h) if keep is None else keep.astype(np.float64) / (1.0 - p_drop)
    hd = h * s
    l = hd @ w.reshape(-1) + float(np.asarray(b).reshape(-1)[0])
    if v_mask:
        l = np.where(np.abs(P).sum(2) == 0, -np.inf, l)
    with np.errstate(invalid="ignore"):
        e = np.exp(l - l.max(1, keepdims=True))
        pr = e / e.sum(1, keepdims=True)
    return np.einsum("bn,bnd->bd", pr, X), pr, l, (h, s, hd)


def step64_bwd(g, P, qv, w, X, pr, hs, x_is_p):
    h, s, hd = hs
    g = np.asarray(g, np.float64)
    dp = np.einsum("bd,bnd->bn", g, np.asarray(X, np.float64))
    dl = pr * (dp - (pr * dp).sum(1, keepdims=True))
    dz = dl[:, :, None] * np.asarray(w, np.float64).reshape(-1) * s * (1.0 - h * h)
    pool = pr[:, :, None] * g[:, None, :]
    dP = dz + pool if x_is_p else dz
    return dP, dz.sum(1), (dl[:, :, None] * hd).sum((0, 1)), np.array([dl.sum()]), pool


def san64(v, q, p, num_stacks, v_mask=True, prefix=""):
    f = lambda k: np.asarray(p[prefix + k], np.float64)
    v, q = np.asarray(v, np.float64), np.asarray(q, np.float64)
    qv = q @ f("fc11.weight").T + f("fc11.bias")
    P = v @ f("fc12.weight").T
    u = q @ f("fc14.weight").T + f("fc14.bias") + step64(P, qv, f("fc13.weight"), f("fc13.bias"), v @ f("fc15.weight").T, v_mask=v_mask)[0]
    for s in range(num_stacks - 1):
        qv = u @ f("layers.%d.weight" % (3 * s)).T + f("layers.%d.bias" % (3 * s))
        P = v @ f("layers.%d.weight" % (3 * s + 1)).T
        u = u + step64(P, qv, f("layers.%d.weight" % (3 * s + 2)), f("layers.%d.bias" % (3 * s + 2)), P, v_mask=v_mask)[0]
    return u


# ---- unit fixtures ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"], indirect=True)
@pytest.mark.parametrize("name", ["g13_san_s1", "g13_san_s2", "g13_san_s3", "g13_san_nomask"])
def test_stacked_attention_matches_reference(name, mode):
    fx = load(name)
    c = fx.cfg
    tol = TOL[mode]
    m = cti_amd.StackedAttention(c["num_stacks"], c["v_dim"], c["q_dim"], c["att"], 11, 0.0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in fx.p.items()}, strict=True)
    m = m.to(DEV).eval()
    with torch.no_grad():
        u = m(T(fx.i["v"]), T(fx.i["q"]), v_mask=c["v_mask"])
    check(u, fx.o["u"], tol, "u")                                            # (NaN row pattern exact)
    assert np.array_equal(np.isnan(u.cpu().numpy()), np.isnan(fx.o["u"]))
    ok = c["ok"]
    v, q = T(fx.i["v"][ok], grad=True), T(fx.i["q"][ok], grad=True)
    u_ok = m(v, q, v_mask=c["v_mask"])
    check(u_ok, fx.o["u_ok"], tol, "u (autograd path)")
    (u_ok * T(fx.i["gu"])).sum().backward()
    for k, prm in m.named_parameters():
        if logit_bias(k):
            check_zero(prm.grad, fx.g[k], np.abs(fx.g[k[:-4] + "weight"]).max(), tol, "d " + k)
        else:
            check(prm.grad, fx.g[k], tol, "d " + k)
    check(v.grad, fx.g["img_feat"], tol, "d img_feat")
    check(q.grad, fx.g["ques_feat"], tol, "d ques_feat")


# ---- the attention step against float64 ---------------------------------------------------------------------------------------------------
def _step_case(B, N, A, Dx, seed):
    rs = np.random.RandomState(seed)
    P_full = rs.standard_normal(size=(B, N, 3 * A)).astype(np.float32)
    if N > 2:
        for b in range(B):
            P_full[b, (N + 1) // 2 + b % 2:] = 0                    # zero (masked) rows
    qv = np.tanh(rs.standard_normal(size=(B, A))).astype(np.float32)
    w = (rs.standard_normal(size=(1, A)) / np.sqrt(A) * 2).astype(np.float32)
    b = np.array([0.3], np.float32)
    X = rs.standard_normal(size=(B, N, Dx)).astype(np.float32)
    keep = (rs.uniform(size=(B, N, A)) >= 0.5).astype(np.uint8)
    g = rs.standard_normal(size=(B, A)).astype(np.float32)
    gx = rs.standard_normal(size=(B, Dx)).astype(np.float32)
    return P_full, qv, w, b, X, keep, g, gx


@pytest.mark.parametrize("A,Dx", [(18, 22), (20, 24)])
@pytest.mark.parametrize("N", [1, 7, 36, 100])
@pytest.mark.parametrize("pool_v", [False, True])
def test_san_attend_against_float64(N, A, Dx, pool_v):
    B = 5
    P_full, qv, w, b, X, keep, g, gx = _step_case(B, N, A, Dx, 100 * N + A + int(pool_v))
    Pf = T(P_full)
    P = Pf[:, :, A:2 * A]                                   # a column slice of a wider projection, read in place
    Xt = T(X) if pool_v else None
    Pn = P_full[:, :, A:2 * A]
    Xn = X if pool_v else Pn
    pooled, prob, logits = ops.san_attend(P, T(qv), T(w), T(b), X=Xt, keep=T(keep), p_drop=0.5)
    ref, pr, l, hs = step64(Pn, qv, w, b, Xn, keep, 0.5)
    check(logits, l, 1e-5, "logits")
    check(prob, pr, 1e-5, "prob")
    check(pooled, ref, 1e-5, "pooled")
    gg = gx if pool_v else g
    runs = [ops.san_attend_bwd(T(gg), P, T(qv), T(w), prob, X=Xt, keep=T(keep), p_drop=0.5, need_dX=pool_v) for _ in range(2)]
    dP, dqv, dw, db, dX = runs[0]
    rP, rq, rw, rb, rX = step64_bwd(gg, Pn, qv, w, Xn, pr, hs, not pool_v)
    check(dP, rP, 1e-5, "dP")
    check(dqv, rq, 1e-5, "dqv")
    check(dw, rw, 1e-5, "dw")
    check_zero(db, rb, np.abs(rw).max(), 1e-5, "db")
    if pool_v:
        check(dX, rX, 1e-5, "dX")
    else:
        assert dX is None
    for a, b2 in zip(runs[0], runs[1]):                      # bitwise reproducible (no float atomics)
        assert (a is None and b2 is None) or torch.equal(a, b2)


def test_san_attend_all_masked_sample_is_nan_alone():
    B, N, A, Dx = 4, 9, 16, 16
    P_full, qv, w, b, X, keep, g, gx = _step_case(B, N, A, Dx, 5)
    P_full[2] = 0
    P_full[2, 3, A + 1] = -0.0                                # -0 still counts as zero
    pooled, prob, logits = ops.san_attend(T(P_full)[:, :, A:2 * A], T(qv), T(w), T(b))
    pooled, prob, logits = pooled.cpu().numpy(), prob.cpu().numpy(), logits.cpu().numpy()
    assert np.isnan(pooled[2]).all() and np.isnan(prob[2]).all() and np.isneginf(logits[2]).all()
    rest = [0, 1, 3]
    assert np.isfinite(pooled[rest]).all() and np.isfinite(prob[rest]).all()
    # v_mask = False: no -inf at all
    _, prob2, logits2 = ops.san_attend(T(P_full)[:, :, A:2 * A], T(qv), T(w), T(b), v_mask=False)
    assert torch.isfinite(logits2).all() and torch.isfinite(prob2).all()


# ---- models ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16x3"], indirect=True)
def test_ffoe_san_model(mode):
    fx, p, m = build_model("g13_ffoe_san", "build_san")
    with torch.no_grad():
        out = m(T(fx.i["v"]), T(fx.i["q"]))
    check(out, fx.o["logits"], 1e-4, "FFOE SAN logits")


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"], indirect=True)
def test_mc_san_model(mode):
    fx, p, m = build_model("g13_mc_san", "build_mc_san")
    with torch.no_grad():
        out = m(T(fx.i["v"]), T(fx.i["q"]), T(fx.i["ans"]))
    check(out, fx.o["logits"], 1e-4, "MC SAN logits (one shared V-side projection)")
    out2 = m(T(fx.i["v"]), T(fx.i["q"]), T(fx.i["ans"]))               # autograd path: per-block projections
    check(out2, fx.o["logits"], 1e-4, "MC SAN logits (autograd path)")


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"], indirect=True)
def test_ffoe_san_train_step_matches_reference(mode):
    fx, p, m = build_model("g13_ffoe_san_step", "build_san")
    c = fx.cfg
    v, q, tgt = T(fx.i["v"]), T(fx.i["q"]), T(fx.i["target"])
    opt = cti_amd.FlatAdamaxDP(m, lr=c["lr"], clip_norm=c["clip_norm"])
    opt.zero_grad()
    out = m(v, q)
    check(out, fx.o["logits"], 1e-4, "logits")
    loss = cti_amd.BCEWithLogitsSum()(out, tgt) / c["B"]
    assert abs(float(loss) - float(fx.o["loss"])) < 1e-4 * float(fx.o["loss"])
    loss.backward()
    named = dict(m.named_parameters())
    prs = np.random.RandomState(c["proj_seed"])
    proj = {n: prs.standard_normal(size=tuple(prm.shape)).astype(np.float32) for n, prm in m.named_parameters() if prm.requires_grad}
    got_n = np.array([float(named[n].grad.norm()) for n in c["used"]])
    got_p = np.array([float((named[n].grad.double().cpu() * torch.from_numpy(proj[n]).double()).sum()) for n in c["used"]])
    ref_n, ref_p = fx.o["gnorm"], fx.o["gproj"]
    zero = np.array([logit_bias(n) for n in c["used"]])
    assert zero.any() and np.all(got_n[zero] <= 1e-4 * ref_n.max())       # the logit biases: zero up to rounding on both sides
    got_n, ref_n = got_n[~zero], ref_n[~zero]
    e_n = np.max(np.abs(got_n - ref_n) / (ref_n + 1e-3 * ref_n.max()))
    e_p = np.max(np.abs(got_p - ref_p)) / np.max(np.abs(ref_p))
    print("g13 SAN train step: worst per-parameter gradient-norm deviation %.3g, projection deviation %.3g" % (e_n, e_p))
    assert e_n < 1e-4 and e_p < 1e-4
    opt.step()
    assert abs(float(opt.grad_norm) - float(fx.o["grad_norm"])) < 1e-4 * float(fx.o["grad_norm"])
    with torch.no_grad():
        loss2 = cti_amd.BCEWithLogitsSum()(m(v, q), tgt) / c["B"]
    assert abs(float(loss2) - float(fx.o["loss_after"])) < 2e-4 * float(fx.o["loss_after"])


def test_train_mode_draws_dropout_masks():
    fx, p, m = build_model("g13_ffoe_san", "build_san")
    m.train()
    torch.manual_seed(5)
    out1 = m(T(fx.i["v"]), T(fx.i["q"]))
    out2 = m(T(fx.i["v"]), T(fx.i["q"]))
    assert torch.isfinite(out1).all() and not torch.equal(out1, out2)
    out1.sum().backward()
    assert float(m.v_att.fc13.weight.grad.abs().sum()) > 0 and float(m.v_att.layers[2].weight.grad.abs().sum()) > 0


def test_real_ffoe_widths_against_float64():
    """B = 256, N = 36, v_dim 2048, num_hid 1024, 3129 answers, the default mode: eight spread samples against float64."""
    B, N, Dv, H, n_ans, ntok = 256, 36, 2048, 1024, 3129, 300
    args = types.SimpleNamespace(op="", num_hid=H, activation="relu", dropout=0.5, num_stacks=2)
    torch.manual_seed(0)
    m = cti_amd.build_san(args, _DS(ntok, Dv, n_ans))
    with torch.no_grad():
        for name, prm in m.named_parameters():
            if name.startswith("v_att.") and name.endswith("weight"):
                prm.mul_(3.0)                                              # spread logits (the default init leaves them ~ 0)
    m = m.to(DEV).eval()
    rs = np.random.RandomState(7)
    v = np.abs(rs.standard_normal(size=(B, N, Dv))).astype(np.float32)
    for b in range(B):
        v[b, 10 + b % 26:] = 0
    q = rs.randint(0, ntok, size=(B, 14)).astype(np.int64)
    with torch.no_grad():
        logits = m(T(v), T(q))
        q_emb = m.q_emb.forward_all(m.w_emb(T(q)))[:, -1]
        u = m.v_att(T(v), q_emb)
    torch.cuda.synchronize()
    idx = np.array([0, 37, 70, 101, 150, 199, 222, 255])
    p = {k: t.detach().cpu().numpy() for k, t in m.state_dict().items()}
    qe = q_emb.cpu().numpy()[idx]
    ref_q = M.question_embedding(M.word_embedding(q[idx], p, "w_emb.", dtype=np.float64), p, "q_emb.", dtype=np.float64)
    check(qe, ref_q, 1e-4, "q_emb")
    ref_u = san64(v[idx], qe, p, 2, prefix="v_att.")
    check(u.cpu().numpy()[idx], ref_u, 1e-4, "u at FFOE widths")
    ref_l = M.simple_classifier(ref_u, p, "classifier.", dtype=np.float64)
    check(logits.cpu().numpy()[idx], ref_l, 1e-4, "logits at FFOE widths")


def test_cached_stacked_weights_follow_an_optimizer_step():
    fx, p, m = build_model("g13_ffoe_san", "build_san")
    v, q = T(fx.i["v"]), T(fx.i["q"])
    att = m.v_att
    with torch.no_grad():
        q_emb = m.q_emb.forward_all(m.w_emb(q))[:, -1]
        u0 = att(v, q_emb).clone()
    opt = torch.optim.SGD(att.parameters(), lr=0.5)
    (att(v, q_emb) ** 2).sum().backward()
    opt.step()                                                  # in place: storage unchanged, versions bumped
    with torch.no_grad():
        u1 = att(v, q_emb)
    sd = {k: t.detach().cpu().numpy() for k, t in att.state_dict().items()}
    check(u1, san64(fx.i["v"], q_emb.cpu().numpy(), sd, att.num_stacks), 1e-4, "u after the step")
    assert not torch.equal(u0, u1)


def test_graphed_forward_replays_bit_for_bit():
    fx, p, m = build_model("g13_ffoe_san", "build_san")
    v, q = T(fx.i["v"]), T(fx.i["q"])
    g = cti_amd.GraphedForward(lambda v_, q_: m(v_, q_), (v, q))
    v2, q2 = v * 1.7, torch.roll(q, 1, 0)
    with torch.no_grad():
        ref1, ref2 = m(v2, q2).clone(), m(v, q).clone()
    out = g(v2, q2)
    torch.cuda.synchronize()
    assert torch.equal(out, ref1)
    out = g(v, q)
    torch.cuda.synchronize()
    assert torch.equal(out, ref2)


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
    fx, p, m = build_model("g13_ffoe_san", "build_san")
    v, q = T(fx.i["v"]), T(fx.i["q"])
    fx2, p2, m2 = build_model("g13_mc_san", "build_mc_san")
    v2, q2, a = T(fx2.i["v"]), T(fx2.i["q"]), T(fx2.i["ans"])
    with torch.no_grad():
        m(v, q)
        m2(v2, q2, a)
        torch.cuda.synchronize()
        with _Spy() as spy:
            m(v, q)
            m2(v2, q2, a)
        torch.cuda.synchronize()
    assert not spy.seen, dict(spy.seen)
