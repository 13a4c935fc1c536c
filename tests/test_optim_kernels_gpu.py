"""The update kernels of csrc/cti_optim.hip on an MI355X, entry by entry against the float64 references of tests/optim_refs.py (which
tests/test_optim_refs_cpu.py validates on the CPU): scale + per-workgroup sums of squares (cti_flat_scale_sumsq / _g), clip + Adamax
(cti_adamax_step / _g), the two counter kernels, and FlatAdamaxDP over a buffer of more than one pass of both grid-stride loops.  The kernels
are called directly through L.lib() on the current stream; every buffer carries 64 sentinel floats behind its n (and the offset views one in
front) which must come back untouched.

The scaled values are compared bit for bit; every other bound is  c * EPS32 * scale  with the scale computed in float64 from the inputs and c
the rounding count derived in optim_refs.  Each test prints its worst error / bound before it asserts and reports every failing case.

Which case reaches which branch:
  scale_sumsq_body    float4 branch: pointer offset 0, n >= 4; tail of n % 4 != 0 (element by element): n = 1, 3, 5, 1023, 1025, 2^20 - 1,
                      2 * 2^20 + 1027, 3 * 2^20 + 7; scalar branch for a misaligned base: pointer offset 1 (every small n, and 2 * 2^20 + 1027
                      over three passes); workgroups that own nothing (partial exactly 0): every n < 2^20 - 1020; second pass of the loop:
                      n = 2^20 + 4 (one float4 of workgroup 0), third: 2 * 2^20 + 1027, fourth: 3 * 2^20 + 7; the last thread of the grid:
                      n = 2^20 - 1 (a partial float4) and 2^20 (a whole one)
  its denominator     host form: 1 / (world * update_freq) for 1, 3, 8; device form: world = 2 and counts 0 (behaves as 1), 1, 3
  adamax_kernel       one workgroup: n = 1, 255, 256; two: 257; 4096 workgroups of one pass less one element: 2^20 - 1; exactly one pass: 2^20;
                      second pass (thread 0 alone): 2^20 + 1; fourth: 3 * 2^20 + 7
  its coefficient     regimes of optim_refs.REGIMES: min() takes 1 (below, zero), takes the quotient (above, edge, tiny), max_norm <= 0 (off),
                      inf norm -> 0 (inf), NaN norm -> 1 (nan)
  its step size       host form: lr_t formed by the launcher from `step`; device form: from lr_dev and steps_done_dev = step - 1 by every
                      workgroup; steps 1, 2, 10, 1000 and 10^6 (powf returns 0); grad_norm_out NULL and not
  its NaN select      test_nonfinite_gradient_entries: a NaN entry (NaN in exp_inf too: fmaxf alone dropped it), +inf and -inf

Measured on an MI355X, worst error / bound over all cases (the constants of optim_refs are the derived ones, not fitted to these; a correctly
rounded float32 evaluation reaches 0.5, the emulation on the CPU 0.099 / 0.499 / 0.470 / 0.500 / 0.072):
  scaled values  bit-exact     partials  0.099 (host form, n = 2^20), 0.083 (device form), 0.068 through FlatAdamaxDP
  param  0.499     exp_avg  0.470     exp_inf  0.500     norm  0.072      (both forms, every size; per test in its docstring)"""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import cti_amd
import optim_refs as R
from test_small_kernels_gpu import Cases, ratio

pytestmark = pytest.mark.gpu
DEV = "cuda"
L = cti_amd.pkg._lib
F32, F64 = np.float32, np.float64
EPS = R.EPS32
SENT = float(R.SENTINEL)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _buf(x, off=0):
    """numpy float32 -> (device buffer of off + n + 64 floats filled with the sentinel, its view [off, off + n) holding x)"""
    x = np.ascontiguousarray(x, F32)
    buf = torch.full((off + x.size + R.SENTINELS,), SENT, device=DEV, dtype=torch.float32)
    view = buf[off:off + x.size]
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 * off
    return buf, view


def _back(buf, off, n):
    """(the n values, whether every sentinel in front and behind is untouched)"""
    b = buf.cpu().numpy()
    return b[off:off + n], bool((b[:off] == SENT).all() and (b[off + n:] == SENT).all() and b.size == off + n + R.SENTINELS)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# =============================================================================================================================
# 1. scale + sums of squares
# =============================================================================================================================
@pytest.mark.parametrize("form", ["host", "dev"])
def test_scale_sumsq_values_bit_exact_and_every_partial(form):
    """Every case of R.scale_cases() of this form: the scaled values equal the float32 product bit for bit, each of the 1024 partials (written
    over NaN) is within (4 * passes + 8) * EPS32 of its float64 sum of squares, the partials of workgroups that own no element are exactly 0, the
    sentinels and (device form) the counter are untouched.  Measured: values bit-exact in all 96 cases; worst partial error / bound 0.099 (host
    form) and 0.083 (device form), both at n = 2^20."""
    lib = L.lib()
    c = Cases("scale_sumsq %s form" % form)
    for f, n, off, d, gscale in R.scale_cases():
        if f != form:
            continue
        case = (n, off, d, gscale)
        g = R.grad_input(n, gscale, off, d)
        buf, view = _buf(g, off)
        pbuf, part = _buf(np.full(R.OPT_BLOCKS, np.nan, F32))
        if form == "host":
            L.check(lib.cti_flat_scale_sumsq(view.data_ptr(), n, 1.0 / d, part.data_ptr(), _stream()), "cti_flat_scale_sumsq")
        else:
            micro = torch.full((1,), d, device=DEV, dtype=torch.int64)
            L.check(lib.cti_flat_scale_sumsq_g(view.data_ptr(), n, R.DEV_WORLD, micro.data_ptr(), part.data_ptr(), _stream()), "cti_flat_scale_sumsq_g")
            c.require(int(micro.item()) == d, case + ("counter unchanged",))
        got, ok = _back(buf, off, n)
        gp, okp = _back(pbuf, 0, R.OPT_BLOCKS)
        c.require(ok and okp, case + ("sentinels",))
        want = R.scale_ref(g, R.case_inv(form, d))
        c.require(_bits(got, want), case + ("values bit-exact",))
        ref = R.partials_ref(want)
        r = ratio(gp, ref, R.partials_c(n) * EPS * ref)
        if n > 1025:
            print("  %s n=%d offset %d: worst partial error / bound %.3f" % (form, n, off, r))
        c.add(r, case + ("partials",))
        e = R.empty_groups(n)
        c.require(e == 0 or bool((gp[R.OPT_BLOCKS - e:] == 0).all()), case + ("empty workgroups write 0",))
    c.done()


# =============================================================================================================================
# 2. clip + Adamax
# =============================================================================================================================
def _adamax(c, d, lib, norm_out=True, after=None):
    """launches one case (optim_refs.adamax_cases) on inputs d = (p, g, m, u, partial, max_norm); after(step_dev): queued behind the kernel.
    Returns the outputs and whether everything that must stay as it was did."""
    n = c["n"]
    bufs = [_buf(a) for a in d[:5]]
    ptr = [v.data_ptr() for _, v in bufs]
    nbuf, nview = _buf(np.full(1, np.nan, F32))
    nptr = nview.data_ptr() if norm_out else None
    same = True
    if c["form"] == "host":
        L.check(lib.cti_adamax_step(ptr[0], ptr[1], ptr[2], ptr[3], n, ptr[4], d[5], c["lr"], R.B1, R.B2, R.ADAM_EPS, c["step"], nptr, _stream()),
                "cti_adamax_step")
    else:
        lr_dev = torch.full((1,), c["lr"], device=DEV, dtype=torch.float32)
        step_dev = torch.full((1,), c["step"] - 1, device=DEV, dtype=torch.int64)
        L.check(lib.cti_adamax_step_g(ptr[0], ptr[1], ptr[2], ptr[3], n, ptr[4], d[5], lr_dev.data_ptr(), R.B1, R.B2, R.ADAM_EPS, step_dev.data_ptr(),
                                      nptr, _stream()), "cti_adamax_step_g")
        if after is not None:
            after(step_dev)
        else:
            same = int(step_dev.item()) == c["step"] - 1
        same = same and float(lr_dev.item()) == float(F32(c["lr"]))
    outs = [_back(b, 0, a.size) for (b, _), a in zip(bufs, d[:5])]
    norm, okn = _back(nbuf, 0, 1)
    same = same and all(ok for _, ok in outs) and okn and _bits(outs[1][0], d[1]) and _bits(outs[4][0], d[4])
    if not norm_out:
        same = same and math.isnan(norm[0])                                   # nothing was written
    return outs[0][0], outs[2][0], outs[3][0], float(norm[0]), same


def _check_adamax(cs, c, d, got, worst):
    p, m, u, norm, same = got
    case = tuple(c[k] for k in ("form", "n", "regime", "step", "lr", "later", "norm_out", "gscale"))
    r = R.case_ref(c, d)
    b = R.adamax_bounds(r)
    cs.require(same, case + ("sentinels, grad, partial and the device scalars untouched",))
    for k, g in (("p", p), ("m", m), ("u", u)):
        v = ratio(g, r[k], b[k])
        worst[k] = max(worst[k], v)
        cs.add(v, case + (k,))
    if c["norm_out"]:
        if c["regime"] == "inf":
            cs.require(math.isinf(norm) and norm > 0, case + ("norm is +inf",))
        elif c["regime"] == "nan":
            cs.require(math.isnan(norm), case + ("norm is NaN",))
        else:
            v = ratio([norm], [r["norm"]], b["norm"])
            worst["norm"] = max(worst["norm"], v)
            cs.add(v, case + ("norm",))
    still = (d[1] == 0) & (d[2] == 0)                                         # no gradient and no momentum: the parameter does not move
    cs.require(still.sum() >= (1 if c["n"] > 20 and not c["later"] else 0) and _bits(p[still], d[0][still]), case + ("p unchanged where g = m = 0",))
    u_still = np.maximum(float(F32(R.B2)) * d[3][still].astype(F64), float(F32(R.ADAM_EPS)))
    cs.add(ratio(u[still], u_still, b["u"][still]), case + ("exp_inf = max(b2 u, eps) where g = m = 0",))


@pytest.mark.parametrize("form", ["host", "dev"])
def test_adamax_every_entry_small_sizes(form):
    """n = 1, 255, 256, 257: every regime x step of this form, learning rate, state, gradient scale and grad_norm_out taking turns
    (R.adamax_cases).  Every entry of p, exp_avg and exp_inf and the norm within the bounds derived in optim_refs.  Measured worst error / bound: host form
    p 0.485, exp_avg 0.361, exp_inf 0.496, norm 0.072; device form p 0.493, exp_avg 0.353, exp_inf 0.491, norm 0.072."""
    lib = L.lib()
    cs = Cases("adamax %s form, small sizes" % form)
    worst = {"p": 0.0, "m": 0.0, "u": 0.0, "norm": 0.0}
    for c in R.adamax_cases():
        if c["form"] == form and c["n"] <= 257:
            d = R.case_data(c)
            _check_adamax(cs, c, d, _adamax(c, d, lib, c["norm_out"]), worst)
    print("  worst error / bound:", {k: "%.3f" % v for k, v in worst.items()})
    cs.done()


def test_adamax_every_entry_past_one_pass_of_the_grid():
    """n = 2^20 - 1, 2^20, 2^20 + 1 and 3 * 2^20 + 7, two cases each (R.adamax_cases): both forms, clipped and unclipped, first and 10^6-th step.  Measured worst error / bound: p 0.499, exp_avg 0.470, exp_inf 0.500, norm 0.071."""
    lib = L.lib()
    cs = Cases("adamax, multi-pass sizes")
    worst = {"p": 0.0, "m": 0.0, "u": 0.0, "norm": 0.0}
    for c in R.adamax_cases():
        if c["n"] > 257:
            d = R.case_data(c)
            _check_adamax(cs, c, d, _adamax(c, d, lib, c["norm_out"]), worst)
            print("  n=%d %s %s step %d: worst so far" % (c["n"], c["form"], c["regime"], c["step"]), {k: "%.3f" % v for k, v in worst.items()})
    cs.done()


@pytest.mark.parametrize("form", ["host", "dev"])
def test_nonfinite_gradient_entries(form):
    """One NaN, one +inf and one -inf among ordinary gradients, finite partials handed in (unclipped and clipped), first and later state: the NaN
    entry is NaN in p, exp_avg AND exp_inf (torch's amax keeps it; fmaxf alone dropped it), an inf entry gives exp_avg = +-inf, exp_inf = +inf and
    p = NaN (inf / inf), as float64 torch does, and every other entry meets its bound (measured worst error / bound 0.499).  With fmaxf alone
    in the kernel the exp_inf assertion of the NaN entry failed in all six cases of either form, and nothing else did."""
    lib = L.lib()
    cs = Cases("adamax %s form, non-finite gradient entries" % form)
    for n in (1000, R.PASS + 1):
        for regime in ("below", "above"):
            for later in ((False, True) if n == 1000 else (True,)):
                c = dict(form=form, n=n, regime=regime, step=3, lr=2e-3, later=later, norm_out=True, gscale=1.0, key=4242 + n % 7 + later)
                d = R.case_data(c)
                at = {17: math.nan, 500: math.inf, 77: -math.inf}
                for i, v in at.items():
                    d[1][i] = v
                p, m, u, norm, same = _adamax(c, d, lib)
                case = (n, regime, later)
                r = R.case_ref(c, d)
                b = R.adamax_bounds(r)
                cs.require(same, case + ("untouched",))
                cs.require(np.isnan(p[17]) and np.isnan(m[17]), case + ("NaN entry: p and exp_avg",))
                cs.require(bool(np.isnan(u[17])), case + ("NaN entry: exp_inf",))
                for i, sign in ((500, 1.0), (77, -1.0)):
                    cs.require(m[i] == sign * math.inf and u[i] == math.inf and np.isnan(p[i]), case + ("inf entry", i))
                    cs.require(r["m"][i] == sign * math.inf and r["u"][i] == math.inf and np.isnan(r["p"][i]), case + ("inf entry of the reference", i))
                cs.require(np.isnan(r["u"][17]) and np.isnan(r["p"][17]) and np.isnan(r["m"][17]), case + ("NaN entry of the reference",))
                rest = np.ones(n, bool)
                rest[list(at)] = False
                for k, g in (("p", p), ("m", m), ("u", u)):
                    cs.add(ratio(g[rest], r[k][rest], b[k][rest]), case + (k,))
                cs.add(ratio([norm], [r["norm"]], b["norm"]), case + ("norm",))
    cs.done()


# =============================================================================================================================
# 3. counters
# =============================================================================================================================
def test_counters_hold_64_bits_and_act_in_stream_order():
    """cti_counter_set / cti_counter_add past 2^31 and 2^32 and with a negative increment; an add and a set queued behind cti_adamax_step_g are
    not seen by it (the update is the one of the step count it was launched on), and are there afterwards."""
    lib = L.lib()
    ctr = torch.zeros(1 + 2, device=DEV, dtype=torch.int64)
    ctr[1:] = -77
    want = 0
    for op, v in (("set", (1 << 31) + 5), ("add", 1 << 32), ("add", (1 << 31) - 7), ("add", -(1 << 34)), ("add", -1), ("set", -(1 << 40)), ("add", (1 << 40) + 3),
                  ("set", (1 << 62) + 1), ("add", -(1 << 62))):
        if op == "set":
            L.check(lib.cti_counter_set(ctr.data_ptr(), v, _stream()), "cti_counter_set")
            want = v
        else:
            L.check(lib.cti_counter_add(ctr.data_ptr(), v, _stream()), "cti_counter_add")
            want += v
        assert ctr.tolist() == [want, -77, -77], (op, v)
    assert want == 1
    cs = Cases("counters behind cti_adamax_step_g")
    worst = {"p": 0.0, "m": 0.0, "u": 0.0, "norm": 0.0}
    seen = []

    def add(step_dev):
        L.check(lib.cti_counter_add(step_dev.data_ptr(), 4, _stream()), "cti_counter_add")
        seen.append(int(step_dev.item()))

    def set_(step_dev):
        L.check(lib.cti_counter_set(step_dev.data_ptr(), 1 << 33, _stream()), "cti_counter_set")
        seen.append(int(step_dev.item()))

    for n, after, step, then in ((R.PASS + 1, add, 1, 4), (257, set_, 2, 1 << 33), (3 * R.PASS + 7, set_, 1, 1 << 33)):
        c = dict(form="dev", n=n, regime="below", step=step, lr=2e-3, later=True, norm_out=True, gscale=1.0, key=900 + step)
        d = R.case_data(c)
        _check_adamax(cs, c, d, _adamax(c, d, lib, after=after), worst)          # against the reference of `step`: 5 or 2^33 + 1 would miss by far
        cs.require(seen[-1] == then, (n, "counter afterwards", seen[-1]))
    cs.done()


# =============================================================================================================================
# 4. FlatAdamaxDP over more than one pass
# =============================================================================================================================
SHAPES = [(1100, 1000), (70000,), (4097,), (3, 333), (1,)]


class _Bare(nn.Module):
    def __init__(self):
        super().__init__()
        rs = R.rng(31)
        ps = []
        for s in SHAPES:
            w = rs.standard_normal(s).astype(F32)
            w[rs.rand(*s) < 0.2] = 0
            ps.append(nn.Parameter(torch.from_numpy(w)))
        self.ps = nn.ParameterList(ps)


def _grads(scale, key, none=()):
    return [None if i in none else R.grad_input(int(np.prod(s)), scale, key, i).reshape(s) for i, s in enumerate(SHAPES)]


def test_flat_adamax_dp_updates_over_a_multi_pass_buffer():
    """A bare module of 1 175 296 floats after the 64-float padding (> 2^20: both kernels' loops wrap), gradients assigned by hand, four updates:
    step() with large gradients (clipped), step() with small ones (unclipped), two accumulate() + update() with one parameter without a gradient
    in both micro-batches (a zero gradient: its momentum continues) and one without in the second only, and step() after opt.lr changed.  Per
    update: the device state before it goes into the references, and afterwards flat_g equals the scaled UNCLIPPED sum bit for bit (p.grad a
    view of it), the 1024 partials, grad_norm and every entry of flat_p, exp_avg and exp_inf (padding included) are within the one-step bounds, and
    the padding is 0 in flat_p, flat_g and exp_avg and <= eps in exp_inf.  Measured worst error / bound over the four updates: partials 0.068,
    p 0.497, exp_avg 0.465, exp_inf 0.500, grad_norm 0.053."""
    model = _Bare().to(DEV)
    opt = cti_amd.FlatAdamaxDP(model, lr=2e-3, clip_norm=0.25, update_freq=3)
    n = opt.n
    assert n == sum((int(np.prod(s)) + 63) // 64 * 64 for s in SHAPES) == 1175296 and n > R.PASS
    pad = np.ones(n, bool)
    for p, o in zip(opt.params, opt.offsets):
        pad[o:o + p.numel()] = False
        assert p.data_ptr() == opt.flat_p.data_ptr() + 4 * o
    cs = Cases("FlatAdamaxDP, n = %d" % n)
    worst = {"p": 0.0, "m": 0.0, "u": 0.0, "norm": 0.0, "partials": 0.0}
    updates = [("step", [_grads(1.0, 1)], True, None), ("step", [_grads(1e-5, 2)], False, None),
               ("update", [_grads(1e-3, 3, none=(1,)), _grads(1e-3, 4, none=(1, 3))], True, None), ("step", [_grads(1e-4, 5)], False, 7e-4)]
    for k, (via, micro, clipped, new_lr) in enumerate(updates):
        step = k + 1
        if new_lr is not None:
            opt.lr = new_lr
            assert opt.param_groups[0]["lr"] == new_lr
        p0, m0, u0 = (t.cpu().numpy() for t in (opt.flat_p, opt.exp_avg, opt.exp_inf))
        flat = np.zeros(n, F32)
        for j, grads in enumerate(micro):
            for p, o, g in zip(opt.params, opt.offsets, grads):
                p.grad = None if g is None else torch.from_numpy(g).to(DEV)
                if g is not None:
                    flat[o:o + g.size] = g.reshape(-1) if j == 0 else flat[o:o + g.size] + g.reshape(-1)     # one float32 add per element
            norm_t = opt.step() if via == "step" else opt.accumulate()
        if via == "update":
            norm_t = opt.update()
        want_g = R.scale_ref(flat, R.inv_denom(3 if via == "step" else len(micro)))
        got_g, part = opt.flat_g.cpu().numpy(), opt.partial.cpu().numpy()
        cs.require(_bits(got_g, want_g), (step, "flat_g is the scaled, unclipped gradient bit for bit"))
        for p, o in zip(opt.params, opt.offsets):
            cs.require(p.grad is not None and p.grad.data_ptr() == opt.flat_g.data_ptr() + 4 * o and p.grad.shape == p.shape
                       and _bits(p.grad.cpu().numpy().reshape(-1), want_g[o:o + p.numel()]), (step, "p.grad is a view of flat_g", o))
        pref = R.partials_ref(want_g)
        v = ratio(part, pref, R.partials_c(n) * EPS * pref)
        worst["partials"] = max(worst["partials"], v)
        cs.add(v, (step, "partials"))
        r = R.adamax_ref(p0, want_g, m0, u0, part, 0.25, opt.lr, R.B1, R.B2, R.ADAM_EPS, step)      # the device's partials: an input of this kernel
        b = R.adamax_bounds(r)
        cs.require(bool(r["clipped"]) == clipped, (step, "regime", r["coef"]))
        got = {"p": opt.flat_p.cpu().numpy(), "m": opt.exp_avg.cpu().numpy(), "u": opt.exp_inf.cpu().numpy()}
        for key in ("p", "m", "u"):
            v = ratio(got[key], r[key], b[key])
            worst[key] = max(worst[key], v)
            cs.add(v, (step, key))
        gn = float(norm_t.item())
        v = ratio([gn], [r["norm"]], b["norm"])
        worst["norm"] = max(worst["norm"], v)
        cs.add(v, (step, "grad_norm against the norm of the device's partials"))
        true = math.sqrt(pref.sum())
        cs.add(ratio([gn], [true], (R.C_NORM + R.partials_c(n) / 2) * EPS * true), (step, "grad_norm against the float64 norm of the gradient"))
        cs.require(bool((got["p"][pad] == 0).all() and (got_g[pad] == 0).all() and (got["m"][pad] == 0).all()
                        and (got["u"][pad] <= F32(R.ADAM_EPS)).all()), (step, "padding"))
        cs.require(opt.steps_done() == step and opt.micro_count == 0 and int(opt.micro_dev.item()) == 0, (step, "counters"))
        if k == 2:                                                                    # the parameter without a gradient: zero gradient, the momentum goes on
            o, cnt = opt.offsets[1], opt.params[1].numel()
            cs.require(bool((want_g[o:o + cnt] == 0).all() and (m0[o:o + cnt] != 0).any() and (got["p"][o:o + cnt] != p0[o:o + cnt]).any()),
                       (step, "momentum continues without a gradient"))
        print("  update %d (%s): worst so far" % (step, via), {kk: "%.3f" % vv for kk, vv in worst.items()})
    cs.done()
