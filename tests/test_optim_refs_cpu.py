"""tests/optim_refs.py checked on the CPU: adamax_ref agrees with float64 torch.optim.Adamax behind the reference's clip over consecutive steps to
1e-12 (NaN and inf entries included, position by position); every input set of tests/test_optim_kernels_gpu.py gives finite references and
scales; a float32 transcription of both kernels' arithmetic stays at 0.6 of every bound on every one of those input sets (the bounds are
attainable) while eight deliberately wrong variants of it exceed a bound on some of them (the bounds discriminate); and the entry points
of csrc/cti_optim.hip return their error codes before anything is launched."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cti_amd
import optim_refs as R

F32, F64 = np.float32, np.float64
EPS = R.EPS32


# ---- 1. adamax_ref against torch --------------------------------------------------------------------------------------------------
def _clip64(t, max_norm):
    """the reference's clip (src/utils.py:323-328) on a float64 tensor, with the 1e-6 the kernel sees (float32); returns the norm"""
    norm = float(torch.norm(t))
    if norm > max_norm > 0:
        t.mul_(max_norm / (norm + float(F32(1e-6))))
    return norm


def _same(a, b, what):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (what, "NaN positions")
    inf = np.isinf(b)
    assert np.array_equal(np.isinf(a), inf) and np.array_equal(a[inf], b[inf]), (what, "inf entries")
    ok = np.isfinite(b)
    if ok.any():
        assert np.abs(a[ok] - b[ok]).max() <= 1e-12 * max(1.0, float(np.abs(b[ok]).max())), what


TORCH_CASES = [
    # name, max_norm, gradient scale, special entry
    ("below", 1e3, 1.0, None), ("above", 0.25, 1.0, None), ("off", 0.0, 1e3, None), ("zero", 0.25, 0.0, None), ("tiny", 2.5e-6, 1e-6, None),
    ("edge", None, 1e-3, None), ("nan entry", 0.25, 1.0, math.nan), ("inf entry", 0.25, 1.0, math.inf), ("-inf entry, no clip", 0.0, 1.0, -math.inf),
]


@pytest.mark.parametrize("name,max_norm,gscale,special", TORCH_CASES)
def test_adamax_ref_agrees_with_torch_over_consecutive_steps(name, max_norm, gscale, special):
    n, steps, lr = 777, 4, 2e-3
    b1, b2, eps = (float(F32(v)) for v in (R.B1, R.B2, R.ADAM_EPS))
    rs = R.rng(5, len(name), n)
    param = torch.nn.Parameter(torch.from_numpy(rs.standard_normal(n)))                       # float64
    opt = torch.optim.Adamax([param], lr=float(F32(lr)), betas=(b1, b2), eps=eps)
    p, m, u = param.detach().numpy().copy(), np.zeros(n), np.zeros(n)
    for step in range(1, steps + 1):
        g32 = R.grad_input(n, gscale, step, len(name)) if gscale else np.zeros(n, F32)
        if special is not None and step == (2 if math.isnan(special) else steps):    # a NaN is then carried by the state; an inf comes last, since
            g32[5] = special                                                          # torch's lerp_ turns a carried -inf into NaN one step later
        mn = max_norm
        if mn is None:                                                                        # the norm a relative 1e-3 above max_norm
            mn = float(F32(math.sqrt(float((g32.astype(F64) ** 2).sum())) / (1 + 1e-3)))
        part = R.partials_ref(g32)
        with R.quiet():
            norm = math.sqrt(part.sum())
        assert not (mn - 1e-6 < norm <= mn), "inside the band where the reference's `if` and the documented min(1, ...) differ"
        ref = R.adamax_ref(p, g32, m, u, part, mn, lr, R.B1, R.B2, R.ADAM_EPS, step)
        grad = torch.from_numpy(g32.astype(F64))
        tn = _clip64(grad, float(F32(mn)))
        param.grad = grad
        opt.step()
        st = opt.state[param]
        assert int(float(st["step"])) == step
        _same([ref["norm"]], [tn], (name, step, "norm"))
        _same(ref["m"], st["exp_avg"].numpy(), (name, step, "exp_avg"))
        _same(ref["u"], st["exp_inf"].numpy(), (name, step, "exp_inf"))
        _same(ref["p"], param.detach().numpy(), (name, step, "param"))
        p, m, u = (a.copy() for a in (param.detach().numpy(), st["exp_avg"].numpy(), st["exp_inf"].numpy()))
    if special is not None:
        assert np.isnan(p[5]) and not np.isfinite(u[5]) and not np.isfinite(m[5]) and np.isfinite(np.delete(p, 5)).all()
        assert np.isnan(u[5]) == (name != "-inf entry, no clip")                              # NaN * 1 and inf * 0 are NaN; -inf unclipped gives u = inf


def test_the_two_forms_hand_the_kernel_the_same_inverse_and_the_owner_map_is_the_grid():
    for d in (1, 2, 3, 6, 8, 24):
        assert ctypes.c_float(1.0 / d).value == float(R.inv_denom(d)) == float(F32(1.0 / d))
    o = R.owner(2 * R.PASS + 9)
    assert o[0] == o[3] == 0 and o[4] == 0 and o[1023] == 0 and o[1024] == 1 and o[R.PASS - 1] == 1023 and o[R.PASS] == 0 and o[2 * R.PASS + 8] == 0
    assert [R.empty_groups(n) for n in (1, 1024, 1025, R.PASS - 1024, R.PASS - 1023, R.PASS)] == [1023, 1023, 1022, 1, 0, 0]
    for n in (1, 1025, 5000):
        part = R.partials_ref(np.ones(n, F32))
        assert (part[R.OPT_BLOCKS - R.empty_groups(n):] == 0).all() and (part[:R.OPT_BLOCKS - R.empty_groups(n)] > 0).all() and part.sum() == n


# ---- 2. attainable and discriminating bounds ----------------------------------------------------------------------------------------
def test_scale_emulation_stays_at_0p6_of_the_partial_bound_on_every_gpu_input_and_a_skipped_element_is_caught():
    worst, caught = 0.0, 0
    for form, n, off, d, gscale in R.scale_cases():
        g = R.grad_input(n, gscale, off, d)
        inv = R.case_inv(form, d)
        gs, part = R.emu_scale_sumsq(g, inv, aligned=(off == 0))
        ref = R.partials_ref(gs)
        assert gs.dtype == F32 and np.isfinite(ref).all() and (gs[g != 0] != 0).all()
        assert (np.abs(gs[gs != 0]) >= 2.0 ** -126).all(), "a subnormal input"
        assert (part[ref == 0] == 0).all() and (ref[R.OPT_BLOCKS - R.empty_groups(n):] == 0).all()
        worst = max(worst, R.worst(part, ref, R.partials_c(n) * EPS * ref))
        if n <= 1025 or (n, off) == (2 * R.PASS + 1027, 0):
            skip = min(n, R.PASS) - 1 if n <= R.PASS else 2 * R.PASS - 1                     # the last element of a pass
            _, mut = R.emu_scale_sumsq(g, inv, aligned=(off == 0), skip=skip)
            caught += R.worst(mut, ref, R.partials_c(n) * EPS * ref) > 1.0
    print("scale emulation: worst error / bound %.3f; the skipped tail element caught in %d cases" % (worst, caught))
    assert worst <= 0.6 and caught >= 10


def _ratios(out, r):
    b = R.adamax_bounds(r)
    return {"p": R.worst(out[0], r["p"], b["p"]), "m": R.worst(out[1], r["m"], b["m"]), "u": R.worst(out[2], r["u"], b["u"]),
            "norm": R.worst([out[3]], [r["norm"]], b["norm"])}


def test_adamax_emulation_stays_at_0p6_of_every_bound_on_every_gpu_input_and_every_mutation_is_caught():
    worst = {"p": 0.0, "m": 0.0, "u": 0.0, "norm": 0.0}
    caught = {k: 0 for k in R.MUTATIONS}
    regimes = set()
    for c in R.adamax_cases():
        d = R.case_data(c)
        r = R.case_ref(c, d)
        args = d + (c["lr"], R.B1, R.B2, R.ADAM_EPS, c["step"])
        out = R.emu_adamax(*args)
        regimes.add(c["regime"])
        for a in d[:4]:
            assert a.dtype == F32 and (np.abs(a[a != 0]) >= 2.0 ** -126).all()
        if c["regime"] in R.FINITE_REGIMES:
            for k in ("p", "m", "u", "S_m", "S_u", "S_upd", "upd", "norm", "lr_t"):
                assert np.isfinite(r[k]).all(), (c, k)
            assert (r["u"] > 0).all() and not (d[5] - 1e-6 < r["norm"] <= d[5])
            assert r["clipped"] == (c["regime"] in ("above", "edge", "tiny"))
            for k, v in _ratios(out, r).items():
                worst[k] = max(worst[k], v)
                assert v <= 0.6, (c, k, v)
        else:                                                                                 # inf / NaN norm: the entries stay finite, the norm does not
            assert r["coef"] == (0.0 if c["regime"] == "inf" else 1.0) and not math.isfinite(r["norm"])
            rr = _ratios(out[:3] + (0.0,), dict(r, norm=0.0))
            assert max(rr.values()) <= 0.6, (c, rr)
            assert (math.isinf(out[3]) and out[3] > 0) if c["regime"] == "inf" else math.isnan(out[3])
        if c["n"] <= 257 and c["regime"] in R.FINITE_REGIMES:
            for mut in R.MUTATIONS:
                caught[mut] += max(_ratios(R.emu_adamax(*args, mutation=mut), r).values()) > 1.0
    print("adamax emulation: worst error / bound", {k: "%.3f" % v for k, v in worst.items()}, "; mutations caught in", caught, "cases")
    assert regimes == set(R.REGIMES)
    assert all(v >= 5 for v in caught.values()), caught


def test_the_bounds_do_not_depend_on_the_emulation_s_luck():
    """what the docstring of optim_refs derives, restated: the constants are the derived ones"""
    assert (R.C_NORM, R.C_COEF, R.C_G, R.C_LRT) == (8.5, 12.0, 13.0, 3.5) and (R.DIV_ULP, R.SQRT_ULP, R.K_POW) == (2.5, 3.0, 16.0)
    assert [R.partials_c(n) for n in (1, R.PASS, R.PASS + 1, 3 * R.PASS + 7)] == [12, 12, 16, 24]
    flags = " ".join(cti_amd.pkg._lib._build.FLAGS)
    assert "correctly-rounded" not in flags, "the build line now sets the rounding of fp32 division: revisit DIV_ULP / SQRT_ULP in optim_refs"


# ---- 3. argument checks before any launch -----------------------------------------------------------------------------------------
def test_optimiser_entry_points_check_their_arguments_before_any_launch():
    lib = cti_amd.pkg._lib.lib()
    al = 256                                                          # a non-NULL address: nothing is dereferenced before the checks
    err = lib.cti_last_error_string
    base = [al, al, al, al, 64, al, 0.25, 2e-3, 0.9, 0.999, 1e-8, 1, al, None]          # cti_adamax_step; grad_norm_out and stream may be NULL
    for i, name in ((0, b"param"), (1, b"grad"), (2, b"exp_avg"), (3, b"exp_inf"), (5, b"partial")):
        a = list(base); a[i] = None
        assert lib.cti_adamax_step(*a) == -1 and b"cti_adamax_step:" in err() and name in err() and b"NULL" in err()
    for n in (0, -5):
        a = list(base); a[4] = n
        assert lib.cti_adamax_step(*a) == -2 and b"cti_adamax_step:" in err()
    for step in (0, -1):
        a = list(base); a[11] = step
        assert lib.cti_adamax_step(*a) == -2 and b"cti_adamax_step:" in err() and b"step" in err()
    base = [al, al, al, al, 64, al, 0.25, al, 0.9, 0.999, 1e-8, al, al, None]           # cti_adamax_step_g: lr and the step count are device pointers
    for i, name in ((0, b"param"), (1, b"grad"), (2, b"exp_avg"), (3, b"exp_inf"), (5, b"partial"), (7, b"lr_dev"), (11, b"steps_done_dev")):
        a = list(base); a[i] = None
        assert lib.cti_adamax_step_g(*a) == -1 and b"cti_adamax_step_g:" in err() and name in err()
    for n in (0, -5):
        a = list(base); a[4] = n
        assert lib.cti_adamax_step_g(*a) == -2 and b"cti_adamax_step_g:" in err()
    assert lib.cti_flat_scale_sumsq(None, 64, 0.5, al, None) == -1 and b"cti_flat_scale_sumsq:" in err() and b"grad" in err()
    assert lib.cti_flat_scale_sumsq(al, 64, 0.5, None, None) == -1 and b"cti_flat_scale_sumsq:" in err() and b"partial" in err()
    for n in (0, -1):
        assert lib.cti_flat_scale_sumsq(al, n, 0.5, al, None) == -2 and b"cti_flat_scale_sumsq:" in err()
        assert lib.cti_flat_scale_sumsq_g(al, n, 2, al, al, None) == -2 and b"cti_flat_scale_sumsq_g:" in err()
    assert lib.cti_counter_add(None, 1, None) == -1 and b"cti_counter_add:" in err() and b"counter" in err()
    assert lib.cti_counter_set(None, 1, None) == -1 and b"cti_counter_set:" in err()
