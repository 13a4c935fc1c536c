"""The small kernels every training step runs, on an MI355X, entry by entry against the float64 references of tests/small_kernel_refs.py (which
tests/test_small_kernel_refs_cpu.py validates on the CPU): the two losses and the elementwise / sequence / embedding kernels of csrc/cti_model.hip
and the backward primitives of csrc/cti_backward.hip, called directly through ops.py at the sizes where their launchers change kernel.

Every entry of every output is compared; a bound is  c * EPS32 * scale  with the scale computed in float64 from the inputs.  Each test prints its
worst error / bound before it asserts; a parametrised test loops over its remaining axes, collects every failing case and reports them all.

Which case reaches which dispatch branch:
  cti_sum_batches      plain kernel: nb < 32, and (nb = 32, n = 2^20); tall kernel: nb >= 32 with n < 2^20, (32, 2^20 - 1) included; the loss
                       modules cross the switch at B = 32 (n = 1, nb = B)
  cti_act_bwd          column width 16: n = 1, 15, 16; 32: n = 17, 32; 64: n = 33, 64, 65, 255, 257, 258 and the misaligned n = 256 views;
                       float4: n = 256, 260, 512; row chunks capped at 1024 (65 rows per chunk): rows = 65 537
  cti_col_sum          row groups capped at 256: rows >= 8192; empty groups 249..255: rows = 8193 and 8449
  cti_wn_bwd           one workgroup: elems <= 4096; chunked float4: 4100, 8192; chunked scalar: 4097, 12 290 and the offset 8192 view
  embedding_bwd_kernel one 1024-column pass: dim <= 1024; two: 1025; three: 2049; several 256-token ballot chunks: every case (1000 tokens);
                       grid stride: 65 539 tokens
  cti_transpose_f32    z grid capped at 32 768: batch = 40 000
  cti_dropout          float4 route: 12 and 4096 elements per copy; scalar route: 13 and 4099"""
import math

import numpy as np
import pytest
import torch

import cti_amd
import small_kernel_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ops = cti_amd.ops
F32, F64 = np.float32, np.float64
EPS = R.EPS32


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def ratio(got, ref, bound):
    """worst |got - ref| / bound over every entry (inf for a non-finite entry or an error where the bound is 0)"""
    g = N(got).astype(F64) if isinstance(got, torch.Tensor) else np.asarray(got, F64)
    ref = np.asarray(ref, F64)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    if g.size == 0:
        return 0.0
    if not np.isfinite(g).all():
        return math.inf
    err = np.abs(g - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / np.broadcast_to(np.asarray(bound, F64), err.shape))
    return float(r.max())


class Cases:
    """collects the worst ratio and the failing cases of one test"""

    def __init__(self, what):
        self.what, self.worst, self.bad, self.count = what, 0.0, [], 0

    def add(self, r, case):
        self.count += 1
        self.worst = max(self.worst, r)
        if not r <= 1.0:
            self.bad.append((case, r))

    def require(self, ok, case):
        self.count += 1
        if not ok:
            self.bad.append((case, "property"))

    def done(self):
        print("%s: %d checks, worst error / bound %.3f" % (self.what, self.count, self.worst))
        assert not self.bad, (self.what, self.bad[:20], len(self.bad))


def rng(*key):
    return np.random.RandomState(np.array([int(k) for k in key], dtype=np.uint32))


def randn(rs, *shape):
    return rs.standard_normal(shape).astype(F32)


# =============================================================================================================================
# 1. losses
# =============================================================================================================================
@pytest.mark.parametrize("rows,n", R.LOSS_SHAPES)
def test_bce_rows_fwd_every_row(rows, n):
    """bce_rows_fwd_kernel per row against float64 at 4 * EPS32 * S (R.loss_ratio); every row finite, the +-100 and dominant rows included.
    Measured on an MI355X over all shapes and scales: worst error / (EPS32 * S) = 0.874 (shape (300, 7), std 8), against 0.806 for the float32
    emulation on the CPU: within the allowance of 4."""
    c = Cases("bce_rows_fwd (%d, %d)" % (rows, n))
    for std in R.LOSS_STDS:
        d = R.loss_inputs(rows, n, std)
        got = N(ops.bce_logits_sum(T(d["x"]), T(d["t"]))).astype(F64)
        assert got.shape == (rows + R.N_SPECIAL,)
        c.require(np.isfinite(got).all(), ("finite", std))
        r = R.loss_ratio(np.abs(got - R.bce_rows_ref(d["x"], d["t"])), R.bce_rows_scale(d["x"], d["t"]), n)
        print("  std %g: worst error / (eps32 S) = %.3f" % (std, r.max()))
        c.add(float(np.nan_to_num(r, nan=math.inf).max()) / R.LOSS_C_FWD, std)
    c.done()


@pytest.mark.parametrize("rows,n", R.LOSS_SHAPES)
def test_kd_rows_fwd_every_row(rows, n):
    """kd_rows_fwd_kernel per row against float64 at 4 * EPS32 * S for T in {0.5, 1.5, 4}; the student-equals-teacher row must be 0 within that
    bound and every row finite.  Measured on an MI355X over all shapes, scales and temperatures: worst error / (EPS32 * S) = 0.979 (shape
    (5, 63), std 1, T = 4), against 0.504 for the float32 emulation on the CPU: within the allowance of 4."""
    c = Cases("kd_rows_fwd (%d, %d)" % (rows, n))
    for std in R.LOSS_STDS:
        d = R.loss_inputs(rows, n, std)
        for Tk in R.KD_TEMPS:
            got = N(ops.kd_rows(T(d["x"]), T(d["k"]), Tk)).astype(F64)
            assert got.shape == (rows + R.N_SPECIAL,)
            c.require(np.isfinite(got).all(), ("finite", std, Tk))
            S = R.kd_rows_scale(d["x"], d["k"], Tk)
            r = R.loss_ratio(np.abs(got - R.kd_rows_ref(d["x"], d["k"], Tk)), S, n)
            print("  std %g T %g: worst error / (eps32 S) = %.3f" % (std, Tk, r.max()))
            c.add(float(np.nan_to_num(r, nan=math.inf).max()) / R.LOSS_C_FWD, (std, Tk))
            c.add(float(R.loss_ratio(abs(got[d["equal"]]), S[d["equal"]], n)) / R.LOSS_C_FWD, ("equal row", std, Tk))
    c.done()


def _bwd_variants(shape, seed):
    """(upstream tensor or None, its value, beta, prefilled dx, prefill as float64)"""
    pre = randn(rng(seed, 77), *shape)
    for up in (None, 3.0):
        upt = None if up is None else torch.tensor([up], device=DEV, dtype=torch.float32)
        yield upt, (1.0 if up is None else up), 0.0, torch.full(shape, float("nan"), device=DEV), np.zeros(shape)
        yield upt, (1.0 if up is None else up), 1.0, T(pre), pre.astype(F64)


@pytest.mark.parametrize("rows,n", R.LOSS_SHAPES)
def test_bce_bwd_every_entry(rows, n):
    """bce_bwd_kernel per entry at 8 * EPS32 * |coef * up| (+ EPS32 * |prefill| with beta = 1): upstream NULL and 3.0, beta = 0 over a NaN dx,
    beta = 1 onto a random dx."""
    c = Cases("bce_bwd (%d, %d)" % (rows, n))
    coef = 0.25
    for std in R.LOSS_STDS:
        d = R.loss_inputs(rows, n, std)
        x, t = T(d["x"]), T(d["t"])
        for upt, up, beta, dx, pre in _bwd_variants(d["x"].shape, rows + n):
            got = ops.bce_logits_bwd(x, t, upt, coef, dx=dx, beta=beta)
            assert got.data_ptr() == dx.data_ptr()
            ref = pre + R.bce_grad_ref(d["x"], d["t"], coef * up)
            c.add(ratio(got, ref, 8 * EPS * abs(coef * up) + EPS * np.abs(pre)), (std, up, beta))
        c.add(ratio(ops.bce_logits_bwd(x, t, None, coef), R.bce_grad_ref(d["x"], d["t"], coef), 8 * EPS * coef), (std, "fresh dx"))
    c.done()


@pytest.mark.parametrize("rows,n", R.LOSS_SHAPES)
def test_kd_rows_bwd_every_entry(rows, n):
    """kd_rows_bwd_kernel per entry at 16 * EPS32 * |coef * up / T| (+ EPS32 * |prefill| with beta = 1), same variants as the BCE gradient; the
    gradient of the student-equals-teacher row is 0 within that bound."""
    c = Cases("kd_rows_bwd (%d, %d)" % (rows, n))
    coef = 0.25
    for std in R.LOSS_STDS:
        d = R.loss_inputs(rows, n, std)
        x, k = T(d["x"]), T(d["k"])
        for Tk in R.KD_TEMPS:
            for upt, up, beta, dx, pre in _bwd_variants(d["x"].shape, rows + n + 1):
                got = ops.kd_rows_bwd(x, k, upt, coef, Tk, dx=dx, beta=beta)
                assert got.data_ptr() == dx.data_ptr()
                ref = pre + R.kd_grad_ref(d["x"], d["k"], Tk, coef * up)
                bound = 16 * EPS * abs(coef * up / Tk) + EPS * np.abs(pre)
                c.add(ratio(got, ref, bound), (std, Tk, up, beta))
                if beta == 0.0:
                    c.add(ratio(got[d["equal"]], np.zeros(n), 16 * EPS * abs(coef * up / Tk)), ("equal row", std, Tk, up))
    c.done()


@pytest.mark.parametrize("B", R.MODULE_BATCHES)
def test_loss_modules_scalar_and_gradient(B):
    """BCEWithLogitsSum and Distillation_Loss (alpha = 0.2, T = 1.5) at n = 37 with a non-unit upstream: the scalar at 4 * EPS32 * sum of the
    weighted row scales, x.grad at the per-entry bounds of the two gradient kernels.  B = 1, 31: plain cti_sum_batches kernel; 32, 33, 257: tall."""
    c = Cases("loss modules B=%d" % B)
    xn, kn, tn = R.module_inputs(B)
    up = 3.0
    x = T(xn).requires_grad_(True)
    bce = cti_amd.BCEWithLogitsSum()(x, T(tn))
    assert bce.dim() == 0
    c.add(ratio(bce.detach(), R.bce_rows_ref(xn, tn).sum(), R.LOSS_C_FWD * EPS * R.bce_rows_scale(xn, tn).sum()), "bce scalar")
    (bce * up).backward()
    c.add(ratio(x.grad, R.bce_grad_ref(xn, tn, up), 8 * EPS * up), "bce grad")
    x.grad = None
    Tk, alpha = 1.5, 0.2
    kd = cti_amd.Distillation_Loss(Tk, alpha)(x, T(kn), T(tn))
    loss, grad = R.distillation_ref(xn, kn, tn, Tk, alpha, up)
    ck, cb = alpha * Tk * Tk / B, (1.0 - alpha) / B
    c.add(ratio(kd.detach(), loss, R.LOSS_C_FWD * EPS * (ck * R.kd_rows_scale(xn, kn, Tk).sum() + cb * R.bce_rows_scale(xn, tn).sum())), "kd scalar")
    (kd * up).backward()
    kd_part = np.abs(R.kd_grad_ref(xn, kn, Tk, ck * up))             # what bce_bwd_kernel accumulates onto (beta = 1)
    c.add(ratio(x.grad, grad, 16 * EPS * ck * up / Tk + 8 * EPS * cb * up + EPS * kd_part), "kd grad")
    c.done()


# =============================================================================================================================
# 2. backward primitives.  Sums: 8 * EPS32 * sum |addends| per entry where the longest chain of additions (derived from the kernel, R.*_depth) has
#    at most 17 links, (depth / 2 + 4) * EPS32 * sum |addends| beyond (R.sum_c).
# =============================================================================================================================
@pytest.mark.parametrize("nb", [1, 3, 4, 5, 31, 32, 33, 45, 47, 48, 49, 64])
def test_sum_batches_every_entry(nb):
    """nb: the edges of the `b + 4 <= nb` loop (plain kernel, nb < 32: a chain of nb additions, so 31 takes the depth rule) and of the
    `b + 12 < nb` loop and the four batch lanes (tall kernel, nb >= 32: nb / 4 additions and two tree levels, the flat 8).  beta = 0 writes over NaN."""
    c = Cases("sum_batches nb=%d" % nb)
    for n in (1, 63, 64, 65, 300):
        rs = rng(nb, n)
        src = randn(rs, nb, n); out0 = randn(rs, n)
        for alpha, beta in ((1.0, 0.0), (0.5, 0.0), (2.0, 1.0), (1.0, -0.5)):
            out = torch.full((n,), float("nan"), device=DEV) if beta == 0.0 else T(out0)
            got = ops.sum_batches(T(src), nb, n, alpha=alpha, out=out, beta=beta)
            ref, sc = R.sum_batches_ref(src, alpha, beta, out0)
            c.add(ratio(got, ref, R.sum_c(R.sum_batches_depth(nb, n)) * EPS * sc), (n, alpha, beta))
        c.add(ratio(ops.sum_batches(T(src), nb, n), *_b(R.sum_batches_ref(src, 1.0, 0.0, None), R.sum_batches_depth(nb, n))), (n, "fresh out"))
    c.done()


def _b(ref_scale, depth):
    return ref_scale[0], R.sum_c(depth) * EPS * ref_scale[1]


_BIG = {}


def _big_source():
    """32 x 2^20 floats (128 MB), made once and shared by the two sizes either side of the n < 2^20 switch"""
    if not _BIG:
        g = torch.Generator().manual_seed(20)
        src = torch.randn(32 << 20, generator=g, dtype=torch.float32)
        _BIG["cpu"], _BIG["gpu"] = src, src.to(DEV)
    return _BIG["cpu"], _BIG["gpu"]


@pytest.mark.parametrize("n", [(1 << 20) - 1, 1 << 20])
def test_sum_batches_at_the_size_switch(n):
    """nb = 32: n = 2^20 - 1 is the last size of the tall kernel (8 additions and two levels: the flat 8), n = 2^20 the first of the plain one (a
    chain of 32: depth rule).  Over a NaN-prefilled out."""
    cpu, gpu = _big_source()
    src = cpu[:32 * n].view(32, n)
    assert R.sum_batches_tall(32, n) == (n < (1 << 20))
    out = torch.full((n,), float("nan"), device=DEV)
    got = ops.sum_batches(gpu[:32 * n], 32, n, alpha=1.0, out=out, beta=0.0)
    ref = src.sum(0, dtype=torch.float64).numpy(); sc = src.abs().sum(0, dtype=torch.float64).numpy()
    c = Cases("sum_batches (32, %d)" % n)
    c.add(ratio(got, ref, R.sum_c(R.sum_batches_depth(32, n)) * EPS * sc), n)
    c.done()


@pytest.mark.parametrize("rows", [1, 3, 32, 33, 321, 8192, 8193, 8449])
def test_col_sum_every_column(rows):
    """Two stages: row groups (at most 256: 8192 rows fill them, at 8193 and 8449 rows groups 249..255 are empty), then cti_sum_batches over the
    groups (its tall kernel from 32 groups = 993 rows on).  Depth rule: R.col_sum_depth, up to 64 additions over 256 groups."""
    c = Cases("col_sum rows=%d" % rows)
    assert R.col_sum_empty_groups(rows) == (7 if rows in (8193, 8449) else 0)
    for n in (1, 63, 64, 65, 130):
        x = randn(rng(rows, n), rows, n)
        for alpha in (1.0, 0.25):
            c.add(ratio(ops.col_sum(T(x), alpha), *_b(R.col_sum_ref(x, alpha), R.col_sum_depth(rows, n))), (n, alpha))
    c.done()


def _act_case(c, rows, n, n_mats, relu, case, offset=False):
    rs = rng(rows, n, 0 if n_mats is None else n_mats, relu)
    dy = randn(rs, rows, n); y = randn(rs, rows, n)
    if relu:                                                        # what a ReLU forward leaves, plus the values the gate must close
        y = np.maximum(y, 0).astype(F32)
        flat = y.reshape(-1)
        pos = (np.arange(8) * 37 + 5) % flat.size
        flat[pos] = np.array([0.0, -0.0, -1e-30, -1e-3, -0.0, 0.0, -2.5, -1e-20], F32)
    scale, div = None, 1
    if n_mats is not None:
        scale, div = (rs.rand(n_mats) + 0.5).astype(F32), n // n_mats
    if offset:                                                       # contiguous views one float into a larger buffer: 4-byte aligned only
        bd = torch.empty(rows * n + 1, device=DEV); by = torch.empty(rows * n + 1, device=DEV)
        dyt, yt = bd[1:].view(rows, n), by[1:].view(rows, n)
        dyt.copy_(T(dy)); yt.copy_(T(y))
        assert dyt.data_ptr() % 16 == 4 and dyt.is_contiguous()
    else:
        dyt, yt = T(dy), T(y)
    dzs, db = ops.act_bwd(dyt, yt, None if scale is None else T(scale), div, relu)
    rz, rb, sb, gate = R.act_bwd_ref(dy, y, scale, div, relu)
    c.add(ratio(dzs, rz, 2 * EPS * np.abs(rz)), case + ("dzs",))
    if relu:
        c.require(gate.sum() >= 1 and (N(dzs)[gate] == 0).all(), case + ("closed entries are exactly 0",))
    c.add(ratio(db, rb, R.sum_c(R.act_bwd_depth(rows, n, not offset)) * EPS * sb), case + ("dbias",))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 32, 33, 64, 65, 255, 256, 257, 258, 260, 512])
def test_act_bwd_every_entry(n):
    """dzs per entry at 2 * EPS32 * |ref| (one product), closed ReLU entries exactly 0, dbias at the sum bound (R.act_bwd_depth: the 16-column kernel
    adds its 16 row lanes in a row, so small n takes the depth rule).  scale = None and per-matrix scales with scale_div = n / n_mats for
    n_mats = 1 and, where 4 divides n, 4 (n = 260: scale_div = 65, a float4 straddles two scales)."""
    c = Cases("act_bwd n=%d (%s)" % (n, R.act_bwd_route(n)))
    for rows in (1, 63, 64, 65, 300):
        for n_mats in (None, 1, 4):
            if n_mats == 4 and n % 4:
                continue                                            # n / 4 is no integer: no such layer
            for relu in (False, True):
                _act_case(c, rows, n, n_mats, relu, (rows, n_mats, relu))
    c.done()


def test_act_bwd_more_rows_than_1024_chunks_of_64():
    """(65 537, 16): 1024 chunks of 65 rows; dbias sums 1024 chunk partials in the tall kernel (depth rule)"""
    c = Cases("act_bwd (65537, 16)")
    assert R.act_chunks(65537) == 1024
    for relu in (False, True):
        _act_case(c, 65537, 16, 4, relu, (65537, 4, relu))
    c.done()


def test_act_bwd_misaligned_views_take_the_scalar_kernel():
    """n = 256 would take the float4 kernel; views starting one float into their buffers must not (and must still be right)"""
    c = Cases("act_bwd n=256 offset views")
    for relu in (False, True):
        for n_mats in (None, 4):
            _act_case(c, 65, 256, n_mats, relu, (65, n_mats, relu, "offset"), offset=True)
    c.done()


def _wn_case(c, elems, n_mats, offset=False):
    rs = rng(elems, n_mats)
    G = randn(rs, n_mats, elems); V = randn(rs, n_mats, elems); g = (rs.rand(n_mats) + 0.5).astype(F32)
    if offset:
        bg = torch.empty(n_mats * elems + 1, device=DEV); bv = torch.empty(n_mats * elems + 1, device=DEV)
        Gt, Vt = bg[1:].view(n_mats, elems), bv[1:].view(n_mats, elems)
        Gt.copy_(T(G)); Vt.copy_(T(V))
        assert Gt.data_ptr() % 16 == 4 and Vt.is_contiguous()
    else:
        Gt, Vt = T(G), T(V)
    dV, dg = ops.wn_bwd(Gt, Vt, T(g), n_mats)
    rV, rg, sV, sg = R.wn_bwd_ref(G, V, g)
    c.add(ratio(dg, rg, R.sum_c(R.wn_bwd_depth(elems)) * EPS * sg), (elems, n_mats, "dg"))
    c.add(ratio(dV, rV, 4 * EPS * sV), (elems, n_mats, "dV"))


@pytest.mark.parametrize("elems", [1, 5, 1023, 1024, 1025, 4096, 4097, 4100, 8192, 12290])
def test_wn_bwd_every_entry(elems):
    """dg = <G, V> / g at the sum bound over sum |G V| / |g| (depth rule, R.wn_bwd_depth: the tree of the dot product alone has 22 links or more),
    dV = G - (<G, V> / |V|^2) V per entry at 4 * EPS32 * (|G| + sum |G V| / |V|^2 * |V|); n_mats = 1, 3, 32 matrices back to back."""
    c = Cases("wn_bwd elems=%d (%s)" % (elems, R.wn_bwd_route(elems)))
    for n_mats in (1, 3, 32):
        _wn_case(c, elems, n_mats)
    c.done()


def test_wn_bwd_offset_view_takes_the_chunked_scalar_route():
    c = Cases("wn_bwd 8192 offset view")
    _wn_case(c, 8192, 1, offset=True)
    c.done()


@pytest.mark.parametrize("rows,cols,batch", [(1, 1, 1), (31, 33, 2), (32, 32, 3), (65, 7, 5), (2, 3, 40000)])
def test_transpose_bit_exact_with_padded_pitches(rows, cols, batch):
    """dst[b][c][r] = src[b][r][c] bit for bit, packed and with padded ld_src / ld_dst (the padding columns of dst untouched); batch = 40 000 is
    more than the 32 768 planes of the grid"""
    rs = rng(rows, cols, batch)
    packed = randn(rs, batch, rows, cols)
    got = ops.transpose(T(packed), rows, cols, batch, s_src=rows * cols)
    assert tuple(got.shape) == (batch, cols, rows)
    assert np.array_equal(N(got).view(np.int32), np.ascontiguousarray(packed.transpose(0, 2, 1)).view(np.int32))
    lds, ldd = cols + 3, rows + 2
    src = randn(rs, batch, rows, lds); dst0 = np.full((batch, cols, ldd), -7.0, F32)
    dst = T(dst0)
    ops.transpose(T(src), rows, cols, batch, s_src=rows * lds, ld_src=lds, dst=dst, s_dst=cols * ldd, ld_dst=ldd)
    want = R.transpose_ref(src, dst0, rows, cols)
    assert np.array_equal(N(dst).view(np.int32), want.view(np.int32))
    assert (N(dst)[:, :, rows:] == -7.0).all()


@pytest.mark.parametrize("copies", [2, 5])
@pytest.mark.parametrize("numel", [12, 13, 4096, 4099])
def test_dropout_copies(numel, copies):
    """dropout(x, 0.3, copies=R): y[r] = x * mask[r] / (1 - p) within one ulp (EPS32 * |ref|, R.dropout_ref) and exactly 0 where dropped, the R
    masks pairwise different, the keep rate within 5 standard deviations of 0.7 at the two large sizes, and the backward form
    dropout(dy, p, mask) applies the same mask.  12 and 4096: float4 route (the period is a multiple of 4); 13 and 4099: scalar route."""
    p = 0.3
    torch.manual_seed(1204 + numel)
    rs = rng(numel, copies)
    x = randn(rs, numel)
    y, mask = ops.dropout(T(x), p, copies=copies)
    assert tuple(y.shape) == tuple(mask.shape) == (copies, numel) and mask.dtype == torch.uint8
    m = N(mask)
    assert set(np.unique(m).tolist()) <= {0, 1}
    c = Cases("dropout numel=%d copies=%d" % (numel, copies))
    ref = R.dropout_ref(x[None, :], m, p)
    c.add(ratio(y, ref, EPS * np.abs(ref)), "forward")
    c.require((N(y)[m == 0] == 0).all(), "dropped entries are 0")
    for a in range(copies):
        for b in range(a + 1, copies):
            c.require(not np.array_equal(m[a], m[b]), ("masks differ", a, b))
    if numel >= 4096:
        rate = m.mean()
        print("  keep rate %.4f (bound %.4f)" % (rate, R.keep_rate_bound(m.size, p)))
        c.require(abs(rate - (1 - p)) <= R.keep_rate_bound(m.size, p), ("keep rate", rate))
    dy = randn(rs, copies, numel)
    back = ops.dropout(T(dy), p, mask)
    refb = R.dropout_ref(dy, m, p)
    c.add(ratio(back, refb, EPS * np.abs(refb)), "backward")
    c.require((N(back)[m == 0] == 0).all(), "backward: dropped entries are 0")
    c.done()


# =============================================================================================================================
# 3. elementwise and sequence kernels
# =============================================================================================================================
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_swish_forward_and_backward(n):
    """per entry at 8 * EPS32 * max(|ref|, |dy|) (dy = 1 for the forward); x holds 0, +-1e-4, +-20, +-100 and every output is finite"""
    c = Cases("swish n=%d" % n)
    x, dy = R.swish_inputs(n)
    y = ops.swish(T(x))
    ref = R.swish_ref(x)
    c.add(ratio(y, ref, 8 * EPS * np.maximum(np.abs(ref), 1.0)), "forward")
    dx = ops.swish_bwd(T(x), T(dy))
    refb = R.swish_bwd_ref(x, dy)
    c.add(ratio(dx, refb, 8 * EPS * np.maximum(np.abs(refb), np.abs(dy.astype(F64)))), "backward")
    c.done()


SEQ_SHAPES = [(1, 1, 1), (3, 14, 5), (2, 0, 7), (4, 6, 257)]


@pytest.mark.parametrize("B,L,H", SEQ_SHAPES)
def test_seq_sum_every_entry(B, L, H):
    """out = beta * out + sum_l x[:, l, :] at the sum bound (a chain of L <= 14 additions: the flat 8); beta = 0 over NaN, beta = 1 onto a
    random out; an empty sequence (L = 0) leaves beta * out"""
    c = Cases("seq_sum (%d, %d, %d)" % (B, L, H))
    rs = rng(B, L, H)
    x = randn(rs, B, L, H); out0 = randn(rs, B, H)
    xt = torch.empty((B, L, H), device=DEV) if L == 0 else T(x)
    for beta in (0.0, 1.0):
        out = torch.full((B, H), float("nan"), device=DEV) if beta == 0.0 else T(out0)
        got = ops.seq_sum(xt, out=out, beta=beta)
        ref, sc = R.seq_sum_ref(x, beta, out0)
        c.add(ratio(got, ref, 8 * EPS * sc), beta)
    ref, sc = R.seq_sum_ref(x, 0.0, None)
    c.add(ratio(ops.seq_sum(xt), ref, 8 * EPS * sc), "fresh out")
    c.done()


@pytest.mark.parametrize("B,L,H", [s for s in SEQ_SHAPES if s[1] >= 1])
def test_seq_bcast_add_bit_exact(B, L, H):
    rs = rng(B, L, H, 1)
    x = randn(rs, B, L, H); y = randn(rs, B, H)
    got = N(ops.seq_bcast_add(T(x), T(y)))
    assert got.shape == (B, L, H) and np.array_equal(got.view(np.int32), R.seq_bcast_add_ref(x, y, L).view(np.int32))
    got = N(ops.seq_bcast_add(None, T(y), L))
    assert got.shape == (B, L, H) and np.array_equal(got.view(np.int32), R.seq_bcast_add_ref(None, y, L).view(np.int32))


@pytest.mark.parametrize("n", [1, 255, 257])
def test_axpby_every_entry_and_in_place(n):
    """a x + b y per entry at 2 * EPS32 * (|a x| + |b y|): into a fresh tensor, into x and into y (the model forwards call it both ways)"""
    c = Cases("axpby n=%d" % n)
    rs = rng(n, 9)
    x = randn(rs, n); y = randn(rs, n)
    for a, b in ((1.0, 1.0), (0.3, -1.7)):
        ref, sc = R.axpby_ref(x, a, y, b)
        c.add(ratio(ops.axpby(T(x), a, T(y), b), ref, 2 * EPS * sc), (a, b, "fresh"))
        xt, yt = T(x), T(y)
        out = ops.axpby(xt, a, yt, b, out=xt)
        c.require(out.data_ptr() == xt.data_ptr() and np.array_equal(N(yt), y), (a, b, "out is x: y untouched"))
        c.add(ratio(xt, ref, 2 * EPS * sc), (a, b, "out is x"))
        xt, yt = T(x), T(y)
        ops.axpby(xt, a, yt, b, out=yt)
        c.require(np.array_equal(N(xt), x), (a, b, "out is y: x untouched"))
        c.add(ratio(yt, ref, 2 * EPS * sc), (a, b, "out is y"))
    c.done()


def _emb_tables(dim):
    rs = rng(dim, 3)
    t0 = randn(rs, 9, dim) * F32(3.0); t1 = randn(rs, 9, dim) * F32(0.01)
    sp = np.array([1.00390625, 1.01171875, -0.0, 3.0e38, -1.00390625], F32)   # bf16 ties (to even: down, up), -0, the top binade
    t0.reshape(-1)[:min(t0.size, len(sp))] = sp[:min(t0.size, len(sp))]
    tok = np.array([[0, 8, -1, 3], [9, 3, 1 << 40, 0], [5, 5, 2, 7]], dtype=np.int64)
    return t0, t1, tok


@pytest.mark.parametrize("dim", [1, 255, 257])
def test_embedding_rows_bit_exact_and_nan_outside_the_table(dim):
    t0, t1, tok = _emb_tables(dim)
    for tabs in ((t0, None), (t0, t1)):
        ref, ok = R.embedding_ref(tok, *tabs)
        got = N(ops.embedding(T(tok), T(tabs[0]), None if tabs[1] is None else T(tabs[1])))
        assert got.shape == ref.shape and (~ok).sum() == 3
        assert np.array_equal(got[ok].view(np.int32), ref[ok].view(np.int32))
        assert np.isnan(got[~ok]).all()


@pytest.mark.parametrize("dim", [1, 255, 257])
def test_embedding_rows16_round_to_nearest_even_and_zero_padding(dim):
    """every in-width entry carries the bits of table.to(torch.bfloat16), rows of tokens outside the table are NaN, and the columns from the width up
    to the 32-multiple pitch are exact zeros"""
    t0, t1, tok = _emb_tables(dim)
    for tabs in ((t0, None), (t0, t1)):
        ref, ok = R.embedding_ref(tok, *tabs)
        width = ref.shape[-1]
        ld = (width + 31) // 32 * 32
        out = ops.embedding_rows16(T(tok), T(tabs[0]), None if tabs[1] is None else T(tabs[1]))
        assert out.dtype == torch.bfloat16 and tuple(out.shape) == tok.shape + (ld,)
        bits = N(out.view(torch.int16)).view(np.uint16)
        assert np.array_equal(bits[ok][:, :width], R.bf16_bits(ref[ok]))
        assert np.isnan(N(out.float())[~ok][:, :width]).all()
        assert (bits[..., width:] == 0).all()


def _emb_bwd_case(tok, dim, col_off, ld, rows, pad, seed):
    g = randn(rng(dim, col_off, seed), len(tok), ld)
    tt, gt = T(tok), T(g)
    a = N(ops.embedding_bwd(tt, gt, col_off, rows, dim, pad))
    b = N(ops.embedding_bwd(tt, gt, col_off, rows, dim, pad))
    want = R.embedding_bwd_emulated(tok, g, col_off, rows, dim, pad)
    assert a.shape == want.shape == (rows, dim)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), "two runs differ"
    diff = a.view(np.int32) != want.view(np.int32)
    assert not diff.any(), ("entries that differ from the documented order", int(diff.sum()), np.argwhere(diff)[:8].tolist())
    assert (a[pad] == 0).all()


@pytest.mark.parametrize("dim", [1, 255, 256, 257, 1024, 1025, 2049])
def test_embedding_bwd_bit_exact_in_the_documented_order(dim):
    """dtable bit for bit against the float32 accumulation in ascending position order (R.embedding_bwd_emulated), twice with identical bits: a
    token first met in the third 256-token chunk, one met more than 256 positions apart, one met 300 times, the padding row left zero, tokens outside
    the table ignored; plain layout and the concatenated one (col_off = dim, ld = 2 dim).  dim > 1024 takes several column passes."""
    tok = R.embedding_bwd_tokens()
    _emb_bwd_case(tok, dim, 0, dim, R.EMB_ROWS, R.EMB_PAD, 0)
    _emb_bwd_case(tok, dim, dim, 2 * dim, R.EMB_ROWS, R.EMB_PAD, 1)


def test_embedding_bwd_grid_stride_bit_exact():
    """65 539 tokens (more than the 65 535 workgroups), dim = 2, 50 distinct tokens of about 1300 occurrences each"""
    _emb_bwd_case(R.embedding_bwd_big_tokens(), 2, 0, 2, 64, 0, 2)
