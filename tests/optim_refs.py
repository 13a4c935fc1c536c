"""Float64 references, error bounds, float32 emulations and seeded inputs for the two update kernels of csrc/cti_optim.hip: scale + per-workgroup
sums of squares (cti_flat_scale_sumsq / _g) and clip + Adamax (cti_adamax_step / _g).  numpy only: no torch, no GPU, no import of the package, so
tests/test_optim_refs_cpu.py validates everything here on any machine and tests/test_optim_kernels_gpu.py compares the kernels with it.

A bound is  c * EPS32 * scale  (or a sum of such terms): the scale is computed here in float64 from the inputs, never from a kernel's output, and c
counts the float32 roundings on the longest path to the value.  Convention: ONE EPS32 per correctly rounded operation (its worst case is half of
that), which pays for the second-order terms and leaves a faithful float32 evaluation at about half of its bound.  Two operations are not taken as
correctly rounded:
  * fp32 division and square root: the build line (FLAGS in _build.py) does not pass -fhip-fp32-correctly-rounded-divide-sqrt, and a bound must
    not lean on a compiler default, so a division is allowed DIV_ULP = 2.5 and a square root SQRT_ULP = 3 (what OpenCL's full profile allows);
  * powf: no copy of HIP's math-function accuracy table is at hand, so K_POW = 16 ulp, the loosest OpenCL's full profile allows pow.  Its error
    in b1^t reaches lr_t amplified by b1^t / (1 - b1^t) (9 at step 1) and is carried as a term of its own in the parameter bound.

The counts (each derived from the kernel's source, in EPS32):
  partial[w]   4 * passes + 8     per thread four fma per pass of the grid-stride loop (passes = ceil(n / 2^20)), six butterfly additions, two
                                  additions across the four waves; every term is >= 0, so the relative error is the number of roundings
  norm         C_NORM = 8.5       each thread adds 4 partials (3 roundings, 0 + x is exact), 6 butterfly, 2 across waves = 11, halved by the
                                  square root, + SQRT_ULP
  coef         C_COEF = 12        C_NORM + 1 (norm + 1e-6) + DIV_ULP; exactly 1 (error 0) where the float64 coefficient is 1 or the norm is NaN
  g'           C_G = 13           C_COEF + 1 (the product); 0 where coef == 1 (a product with 1 is exact)
  exp_avg      (C_G + 2) S_m      the product (1 - b1) * g' and the fma; S_m = b1 |m| + (1 - b1) |g'|          (15 clipped, 2 not)
  exp_inf      (C_G + 1) S_u      b2 * u (1) or |g'| + eps (C_G on |g'|, 1 on the sum); S_u = u'                (14 clipped, 1 not)
  lr_t         C_LRT = 3.5        1 - b1^t (1) and the division (DIV_ULP), besides the powf term
  param        |p| + |upd|  +  (C_M + C_U + C_LRT + 1 + DIV_ULP) S_upd  +  K_POW b1^t / (1 - b1^t) |upd|
                                  the subtraction (1 on |p'| <= |p| + |upd|), then the update lr_t * m' / u': m' to C_M S_m, u' to C_U u', lr_t,
                                  the product lr_t * m' (1), the division; S_upd = lr_t S_m / u' >= |upd| = lr_t |m'| / u'.  The |p| term is
                                  kept apart from the update's (tighter than one constant times S_p = |p| + S_upd), so a parameter of size 1
                                  does not mask an error of the update."""
import math

import numpy as np

EPS32 = 2.0 ** -23
F32, F64 = np.float32, np.float64
OPT_BLOCKS = 1024                       # workgroups of the scale kernel = partial sums
PASS = 1 << 20                          # elements per pass of either grid-stride loop: 1024 * 256 * 4 floats (scale), 4096 * 256 (Adamax)
DIV_ULP, SQRT_ULP, K_POW = 2.5, 3.0, 16.0
C_NORM = 11 / 2 + SQRT_ULP
C_COEF = C_NORM + 1 + DIV_ULP
C_G = C_COEF + 1
C_LRT = 1 + DIV_ULP
SENTINELS = 64                          # floats beyond n every buffer of the GPU test carries
SENTINEL = F32(-12345.5)


def rng(*key):
    return np.random.RandomState(np.array([int(k) for k in key], dtype=np.uint32))


def quiet():
    return np.errstate(all="ignore")


# =============================================================================================================================
# 1. scale + sums of squares
# =============================================================================================================================
def inv_denom(denom):
    """what both forms hand the kernel: (float)(1.0 / (double)denom); denom = world * update_freq (host form, a c_float argument) or
    world * max(count, 1) (device form)"""
    return F32(1.0 / float(denom))


def scale_ref(g32, inv32):
    """the float32 product, one rounding per element: the kernel's values bit for bit"""
    g32 = np.asarray(g32)
    assert g32.dtype == F32
    return g32 * F32(inv32)


def owner(n):
    """workgroup of element e: thread (e // 4) % 2^18 of the grid, 256 threads per workgroup; the same for either pointer alignment"""
    e = np.arange(n, dtype=np.int64)
    return ((e // 4) % (OPT_BLOCKS * 256)) // 256


def partials_ref(gs32):
    """float64 sums of squares of the scaled float32 values per workgroup -> (1024,); a workgroup that owns no element gives exactly 0"""
    gs = np.asarray(gs32)
    assert gs.dtype == F32
    return np.bincount(owner(gs.size), weights=gs.astype(F64) ** 2, minlength=OPT_BLOCKS)


def passes(n):
    return (n + PASS - 1) // PASS


def partials_c(n):
    return 4 * passes(n) + 8


def empty_groups(n):
    """workgroups that own no element (n < 2^20 - 1020)"""
    return max(0, OPT_BLOCKS - (min(n, PASS) + 1023) // 1024)


def _fma32(a, b, c):
    """float32 fma through float64: a * b is exact there, the sum rounds to 53 bits and then to 24 (a double rounding, rare and half an ulp)"""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def _block_sum32(s):
    """(..., 256) float32 per-thread values -> (...,): xor butterfly 32, 16, .., 1 in each of the four waves, then (r0 + r1) + (r2 + r3)"""
    x = s.reshape(s.shape[:-1] + (4, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lane ^ o]
    r = x[..., 0]
    return (r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])


def emu_scale_sumsq(g32, inv32, aligned=True, skip=None):
    """float32 transcription of scale_sumsq_body's arithmetic -> (scaled values, 1024 partials).  aligned: a whole float4 goes w, z, y, x into
    the fma chain; the last, partial one and every one behind a misaligned pointer go element by element in ascending order.  skip: index of
    one element left out of the sum (a mutation for the CPU test)."""
    g32 = np.asarray(g32)
    n = g32.size
    gs = scale_ref(g32, inv32)
    x = np.zeros(passes(n) * PASS, F32)
    x[:n] = gs
    if skip is not None:
        x[skip] = 0
    x = x.reshape(passes(n), OPT_BLOCKS * 256, 4)
    full = (np.arange(passes(n) * PASS // 4) * 4 + 4 <= n).reshape(passes(n), OPT_BLOCKS * 256)
    s = np.zeros(OPT_BLOCKS * 256, F32)
    for k in range(passes(n)):
        down, up = s, s
        for j in (3, 2, 1, 0):
            down = _fma32(x[k, :, j], x[k, :, j], down)
        for j in (0, 1, 2, 3):                                      # zeros behind n leave the sum as it is: fma(0, 0, s) = s
            up = _fma32(x[k, :, j], x[k, :, j], up)
        s = np.where(full[k] & aligned, down, up)
    return gs, _block_sum32(s.reshape(OPT_BLOCKS, 256))


SCALE_SMALL_NS = (1, 3, 4, 5, 1023, 1024, 1025)
SCALE_LARGE_NS = (PASS - 1, PASS, PASS + 4, 2 * PASS + 1027, 3 * PASS + 7)
HOST_DENOMS = (1, 3, 8)                 # world * update_freq of the host form
DEV_WORLD, DEV_COUNTS = 2, (0, 1, 3)    # the device form: world and the micro-batch counts (0 behaves as 1)
GRAD_SCALES = (1e-6, 1e-3, 1.0, 1e3)


def scale_cases():
    """(form, n, pointer offset in floats, world * update_freq or the device count, gradient scale).  Small sizes: both offsets, every denominator
    and count; each large size once per form, the denominators and counts taking turns; 2 * 2^20 + 1027 also behind a misaligned pointer (the
    scalar branch over three passes)."""
    out, i = [], 0
    for n in SCALE_SMALL_NS:
        for off in (0, 1):
            for d in HOST_DENOMS:
                out.append(("host", n, off, d, GRAD_SCALES[i % 4])); i += 1
            for c in DEV_COUNTS:
                out.append(("dev", n, off, c, GRAD_SCALES[i % 4])); i += 1
    for j, n in enumerate(SCALE_LARGE_NS):
        out.append(("host", n, 0, HOST_DENOMS[j % 3], GRAD_SCALES[j % 4]))
        out.append(("dev", n, 0, DEV_COUNTS[(j + 1) % 3], GRAD_SCALES[(j + 2) % 4]))
    out.append(("host", 2 * PASS + 1027, 1, 3, 1.0))
    out.append(("dev", 2 * PASS + 1027, 1, 3, 1e-3))
    return out


def case_inv(form, d):
    return inv_denom(d if form == "host" else DEV_WORLD * max(d, 1))


def grad_input(n, scale, *key):
    """randn * scale with a fifth of the entries exactly 0; normal float32 throughout (the smallest non-zero magnitude is about 1e-7 * scale)"""
    rs = rng(n, *key)
    g = (rs.standard_normal(n) * scale).astype(F32)
    g[rs.rand(n) < 0.2] = 0
    return g


# =============================================================================================================================
# 2. clip + Adamax
# =============================================================================================================================
def adamax_ref(p, g, m, u, partial, max_norm, lr, b1, b2, eps, step):
    """float64 from the float32 inputs; the scalars are rounded to float32 first, as the kernel receives them (1 - b1 and 1e-6 in float32 too).
    A NaN in g' gives NaN in m', u' and p' (np.maximum keeps a NaN, like torch's amax); an inf norm gives coef 0, a NaN norm coef 1.
    Returns a dict: p, m, u, norm, coef, lr_t, clipped and the error scales S_m, S_u (= u'), S_upd (= lr_t S_m / u'), upd (= lr_t |m'| / u')."""
    p, g, m, u = (np.asarray(a, F64) for a in (p, g, m, u))
    b1, b2, eps, lr, max_norm = (float(F32(v)) for v in (b1, b2, eps, lr, max_norm))
    omb1, tiny = float(F32(1.0) - F32(b1)), float(F32(1e-6))
    with quiet():
        norm = math.sqrt(np.asarray(partial, F64).sum())
        c = max_norm / (norm + tiny) if max_norm > 0 else 1.0
        coef = c if c < 1.0 else 1.0
        gp = coef * g
        m1 = b1 * m + omb1 * gp
        u1 = np.maximum(b2 * u, np.abs(gp) + eps)
        lr_t = lr / (1.0 - b1 ** float(step))
        p1 = p - lr_t * m1 / u1
        S_m = b1 * np.abs(m) + omb1 * np.abs(gp)
        return {"p": p1, "m": m1, "u": u1, "norm": norm, "coef": coef, "lr_t": lr_t, "clipped": coef != 1.0, "gp": gp,
                "S_m": S_m, "S_u": u1, "S_upd": lr_t * S_m / u1, "upd": lr_t * np.abs(m1) / u1, "p0": np.abs(p),
                "pow_amp": b1 ** float(step) / (1.0 - b1 ** float(step))}


def adamax_bounds(r):
    """the bounds of the module docstring for one adamax_ref result -> dict m, u, p (arrays) and norm"""
    cg = C_G if r["clipped"] else 0.0
    c_m, c_u = cg + 2, cg + 1
    with quiet():
        return {"m": c_m * EPS32 * r["S_m"], "u": c_u * EPS32 * r["S_u"], "norm": C_NORM * EPS32 * r["norm"],
                "p": EPS32 * (r["p0"] + r["upd"] + (c_m + c_u + C_LRT + 1 + DIV_ULP) * r["S_upd"] + K_POW * r["pow_amp"] * r["upd"])}


def emu_adamax(p, g, m, u, partial, max_norm, lr, b1, b2, eps, step, mutation=None):
    """float32 transcription of adamax_kernel's arithmetic (numpy's correctly rounded division and square root, numpy's power) -> p, m, u, norm.
    mutation: one of MUTATIONS, a deliberately wrong variant the bounds must reject (tests/test_optim_refs_cpu.py)."""
    p, g, m, u, partial = (np.asarray(a, F32) for a in (p, g, m, u, partial))
    b1, b2, eps, lr, max_norm = (F32(v) for v in (b1, b2, eps, lr, max_norm))
    one = F32(1.0)
    with quiet():
        if mutation == "step-1":
            step -= 1
        if mutation == "step+1":
            step += 1
        lr_t = lr / (one - np.power(b1, F32(step)))
        part = partial.copy()
        if mutation == "last partial left out":
            part[-1] = 0
        s = np.zeros(256, F32)
        for k in range(OPT_BLOCKS // 256):
            s = s + part[256 * k:256 * k + 256]
        norm = np.sqrt(_block_sum32(s))
        c = (max_norm / (norm if mutation == "no 1e-6" else norm + F32(1e-6))) if max_norm > 0 else one
        coef = c if (c < one or (mutation == "coef >= 1 applied" and c == c)) else one
        gg = g * coef
        mm = _fma32(np.broadcast_to(b1, m.shape), m, (one - b1) * gg)
        ag = np.abs(gg) + eps
        if mutation == "eps after max":
            uu = np.maximum(b2 * u, np.abs(gg)) + eps
        elif mutation == "b2 on |g'|":
            uu = np.maximum(b2 * u, b2 * ag)
        else:
            uu = np.maximum(b2 * u, ag)
        return p - lr_t * mm / uu, mm, uu, norm


MUTATIONS = ("step-1", "step+1", "eps after max", "coef >= 1 applied", "no 1e-6", "b2 on |g'|", "last partial left out")

B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8     # torch.optim.Adamax defaults, what the reference trains with
LRS = (2e-3, 7e-4)
STEPS = (1, 2, 10, 1000, 10 ** 6)
ADAMAX_SMALL_NS = (1, 255, 256, 257)
ADAMAX_LARGE_NS = (PASS - 1, PASS, PASS + 1, 3 * PASS + 7)
# regime -> (max_norm, norm of the partials handed in, or "inf" / "nan": that value in one partial)
REGIMES = {
    "below": (0.25, 1e-3),              # coefficient exactly 1
    "above": (0.25, 50.0),              # coefficient 5e-3
    "off": (0.0, 1e6),                  # max_norm <= 0: no clipping whatever the norm
    "zero": (0.25, 0.0),                # all-zero partials: norm 0, coefficient 1
    "edge": (0.25, 0.25 * (1 + 1e-3)),  # a relative 1e-3 above max_norm
    "tiny": (2.5e-6, 1e-5),             # where the 1e-6 of the denominator is a tenth of it
    "inf": (0.25, "inf"),               # coefficient 0: m' = b1 m, u' = max(b2 u, eps)
    "nan": (0.25, "nan"),               # coefficient 1
}
FINITE_REGIMES = tuple(k for k in REGIMES if k not in ("inf", "nan"))


def partials_input(regime, *key):
    """1024 float32 partials, all > 0 and of one magnitude (so leaving one out moves the norm by 2.4e-4), whose float64 sum is norm^2"""
    max_norm, norm = REGIMES[regime]
    rs = rng(7, *key)
    w = rs.rand(OPT_BLOCKS) + 0.5
    if isinstance(norm, str):
        part = (w / w.sum() * 1e-2).astype(F32)
        part[int(rs.randint(OPT_BLOCKS))] = F32(norm)
    else:
        part = (w / w.sum() * norm * norm).astype(F32)
    return part, max_norm


def adamax_input(n, gscale, later, *key):
    """p, g, m, u float32.  g: grad_input; p: randn with a fifth exactly 0 (there the bound is the update's alone); first step m = u = 0, later
    step m = randn * gscale / 2 and u = (|randn| + 0.1) * gscale > 0"""
    rs = rng(n, 11, *key)
    g = grad_input(n, gscale, 13, *key)
    p = rs.standard_normal(n).astype(F32)
    p[rs.rand(n) < 0.2] = 0
    if later:
        m = (rs.standard_normal(n) * (0.5 * gscale)).astype(F32)
        u = ((np.abs(rs.standard_normal(n)) + 0.1) * gscale).astype(F32)
    else:
        m, u = np.zeros(n, F32), np.zeros(n, F32)
    return p, g, m, u


def adamax_cases():
    """dicts: form ('host' / 'dev'), n, regime, step, lr, later, norm_out, gscale, key.  Small sizes: every regime x step x form, the other axes
    taking turns (coprime periods, so every pair of values meets); large sizes: two cases each that between them hold both forms, the clipped
    and unclipped regimes, the first and the 10^6-th step and both states."""
    out, i = [], 0
    for n in ADAMAX_SMALL_NS:
        for regime in REGIMES:
            for step in STEPS:
                for form in ("host", "dev"):
                    out.append(dict(form=form, n=n, regime=regime, step=step, lr=LRS[(i // 2) % 2], later=bool((i // 3) % 2), norm_out=bool(i % 2 == (i // 5) % 2),
                                    gscale=GRAD_SCALES[(i // 7) % 4], key=i)); i += 1
    big = [("above", 1, False, "dev"), ("below", 10 ** 6, True, "host"), ("edge", 2, True, "dev"), ("off", 10, True, "host"),
           ("tiny", 1000, False, "host"), ("zero", 2, True, "dev"), ("inf", 10, True, "host"), ("above", 10 ** 6, True, "dev")]
    for j, (regime, step, later, form) in enumerate(big):
        n = ADAMAX_LARGE_NS[j % 4]
        out.append(dict(form=form, n=n, regime=regime, step=step, lr=LRS[j % 2], later=later, norm_out=bool(j % 3), gscale=GRAD_SCALES[(j + 1) % 4],
                        key=i)); i += 1
    return out


def case_data(c):
    """inputs of one adamax case: p, g, m, u, partial, max_norm"""
    part, max_norm = partials_input(c["regime"], c["key"])
    gscale = 1e-6 if c["regime"] == "tiny" else c["gscale"]            # eps and the 1e-6 matter only next to gradients of their size
    return adamax_input(c["n"], gscale, c["later"], c["key"]) + (part, max_norm)


def case_ref(c, d):
    return adamax_ref(d[0], d[1], d[2], d[3], d[4], d[5], c["lr"], B1, B2, ADAM_EPS, c["step"])


def worst(got, ref, bound):
    """worst |got - ref| / bound over the entries (numpy arrays; inf for a non-finite entry or an error where the bound is 0)"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return math.inf
    err = np.abs(got - ref)
    with quiet():
        r = np.where(err == 0, 0.0, err / np.broadcast_to(np.asarray(bound, F64), err.shape))
    return float(np.nan_to_num(r, nan=math.inf).max())
