"""The float64 references of tests/small_kernel_refs.py, checked on the CPU: each agrees with float64 torch.autograd or the torch function it
restates to 1e-12, every input set of tests/test_small_kernels_gpu.py gives finite references, the float32 emulation of the two loss kernels
stays under ratio 1 of the error scales S, and the sequential embedding sum is order-sensitive (so the bit-exact check on the GPU cannot pass by
accident)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_kernel_refs as R

F32, F64 = np.float32, np.float64


def rel(a, b):
    a = np.asarray(a, F64); b = np.asarray(b, F64)
    return float(np.abs(a - b).max() / max(1.0, float(np.abs(b).max())))


def loss_cases():
    for rows, n in R.LOSS_SHAPES:
        for std in R.LOSS_STDS:
            yield rows, n, std, R.loss_inputs(rows, n, std)


# ---- 1. losses -------------------------------------------------------------------------------------------------------------------
def test_loss_inputs_hold_the_special_rows():
    for rows, n, std, d in loss_cases():
        x, k, t = d["x"], d["k"], d["t"]
        assert x.shape == k.shape == t.shape == (rows + R.N_SPECIAL, n) and x.dtype == k.dtype == t.dtype == F32
        assert (x[d["plus"]] == 100).all() and (x[d["minus"]] == -100).all()
        row = x[d["dominant"]]
        assert n == 1 or np.sort(row)[-1] - np.sort(row)[-2] >= 60 - 1e-3
        assert x[d["equal"]].tobytes() == k[d["equal"]].tobytes()
        assert set(np.unique(t).tolist()) <= set(R.SOFT_SCORES.tolist())


def test_bce_references_agree_with_the_closed_forms_and_are_finite():
    for rows, n, std, d in loss_cases():
        x, t = d["x"].astype(F64), d["t"].astype(F64)
        ref = R.bce_rows_ref(d["x"], d["t"])
        closed = (np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))).sum(1)
        assert np.isfinite(ref).all() and rel(ref, closed) < 1e-12
        S = R.bce_rows_scale(d["x"], d["t"])
        assert np.isfinite(S).all() and (S >= np.abs(ref) * (1 - 1e-12)).all() and (S > 0).all()
        g = R.bce_grad_ref(d["x"], d["t"], 3.0 * 0.25)
        assert np.isfinite(g).all() and rel(g, (1.0 / (1.0 + np.exp(-x)) - t) * 0.75) < 1e-12


@pytest.mark.parametrize("T", R.KD_TEMPS)
def test_kd_references_agree_with_the_closed_forms_and_are_finite(T):
    for rows, n, std, d in loss_cases():
        a, b = d["x"].astype(F64) / T, d["k"].astype(F64) / T
        la = a - a.max(1, keepdims=True); la = la - np.log(np.exp(la).sum(1, keepdims=True))
        lb = b - b.max(1, keepdims=True); lb = lb - np.log(np.exp(lb).sum(1, keepdims=True))
        ref = R.kd_rows_ref(d["x"], d["k"], T)
        assert np.isfinite(ref).all() and rel(ref, (np.exp(lb) * (lb - la)).sum(1)) < 1e-12
        assert abs(ref[d["equal"]]) < 1e-12                          # the student-equals-teacher row
        S = R.kd_rows_scale(d["x"], d["k"], T)
        assert np.isfinite(S).all() and (S >= np.abs(ref)).all()
        g = R.kd_grad_ref(d["x"], d["k"], T, 0.75)
        assert np.isfinite(g).all() and rel(g, (np.exp(la) - np.exp(lb)) * 0.75 / T) < 1e-12
        assert np.abs(g[d["equal"]]).max() < 1e-15


def test_distillation_reference_is_the_weighted_sum_of_the_row_references():
    T, alpha, up = 1.5, 0.2, 3.0
    for B in R.MODULE_BATCHES:
        x, k, t = R.module_inputs(B)
        assert x.shape == k.shape == t.shape == (B, 37)
        loss, g = R.distillation_ref(x, k, t, T, alpha, up)
        want = R.kd_rows_ref(x, k, T).sum() / B * alpha * T * T + R.bce_rows_ref(x, t).sum() / B * (1 - alpha)
        assert math.isfinite(loss) and abs(loss - want) < 1e-12 * max(1.0, abs(want))
        gw = R.kd_grad_ref(x, k, T, up * alpha * T * T / B) + R.bce_grad_ref(x, t, up * (1 - alpha) / B)
        assert np.isfinite(g).all() and rel(g, gw) < 1e-12


def test_emulated_loss_kernels_stay_under_ratio_one():
    """The float32 emulation of bce_rows_fwd_kernel / kd_rows_fwd_kernel (their summation order, libm exp / log) against the float64 references,
    over the exact inputs of the GPU tests: error / (EPS32 * S) (loss_ratio: less one smallest normal per element) must stay below 1; the GPU
    tests allow LOSS_C_FWD = 4 times that."""
    worst_bce, worst_kd = 0.0, 0.0
    for rows, n, std, d in loss_cases():
        r = R.loss_ratio(np.abs(R.bce_rows_emulated(d["x"], d["t"]).astype(F64) - R.bce_rows_ref(d["x"], d["t"])), R.bce_rows_scale(d["x"], d["t"]), n)
        worst_bce = max(worst_bce, float(r.max()))
        for T in R.KD_TEMPS:
            e = R.kd_rows_emulated(d["x"], d["k"], T)
            assert np.isfinite(e).all()
            r = R.loss_ratio(np.abs(e.astype(F64) - R.kd_rows_ref(d["x"], d["k"], T)), R.kd_rows_scale(d["x"], d["k"], T), n)
            worst_kd = max(worst_kd, float(r.max()))
    print("emulated worst error / (eps32 S): bce %.3f, kd %.3f" % (worst_bce, worst_kd))
    assert worst_bce < 1.0 and worst_kd < 1.0, (worst_bce, worst_kd)


def test_emulated_block_sum_is_a_sum():
    rs = np.random.RandomState(3)
    p = rs.standard_normal((5, 256)).astype(F32)
    assert rel(R._emu_block_sum(p), p.astype(F64).sum(1)) < 1e-5


# ---- 2. backward primitives --------------------------------------------------------------------------------------------------------
def test_sum_references_and_depths():
    rs = np.random.RandomState(1)
    src = rs.standard_normal((5, 7)).astype(F32); out0 = rs.standard_normal(7).astype(F32)
    ref, sc = R.sum_batches_ref(src, 2.0, 1.0, out0)
    assert rel(ref, (2.0 * t_sum(src) + out0.astype(F64))) < 1e-12 and (sc >= np.abs(ref) - 1e-12).all()
    ref, sc = R.sum_batches_ref(src, 0.5, 0.0, np.full(7, np.nan))
    assert np.isfinite(ref).all() and np.isfinite(sc).all()
    ref, sc = R.col_sum_ref(src, 0.25)
    assert rel(ref, 0.25 * t_sum(src)) < 1e-12
    # the branch each size takes, restated from the launchers
    assert not R.sum_batches_tall(31, 1) and R.sum_batches_tall(32, 1) and R.sum_batches_tall(32, (1 << 20) - 1) and not R.sum_batches_tall(32, 1 << 20)
    assert R.sum_batches_depth(64, 300) == 18 and R.sum_batches_depth(31, 300) == 31
    assert R.col_groups(8192) == 256 and R.col_sum_empty_groups(8192) == 0 and R.col_sum_empty_groups(8193) == 7 and R.col_sum_empty_groups(8449) == 7
    assert R.act_chunks(65536) == 1024 and R.act_chunks(65537) == 1024 and (65537 + 1023) // 1024 == 65
    assert [R.act_bwd_route(n) for n in (1, 16, 17, 32, 33, 255, 256, 257, 258, 260)] == \
        ["cw16", "cw16", "cw32", "cw32", "cw64", "cw64", "v4", "cw64", "cw64", "v4"]
    assert R.act_bwd_route(256, aligned=False) == "cw64"
    assert [R.wn_bwd_route(e) for e in (4096, 4097, 4100, 8192, 12290)] == \
        ["one workgroup", "chunked scalar", "chunked float4", "chunked float4", "chunked scalar"]
    assert R.wn_bwd_route(8192, aligned=False) == "chunked scalar"
    assert R.sum_c(8) == 8.0 and R.sum_c(17) == 8.0 and R.sum_c(18) == 13.0 and R.sum_c(64) == 36.0


def t_sum(a):
    return torch.from_numpy(np.asarray(a, F64)).sum(0).numpy()


@pytest.mark.parametrize("relu", [False, True])
def test_act_bwd_reference_agrees_with_autograd(relu):
    rs = np.random.RandomState(5)
    rows, n, div = 9, 8, 2
    z = rs.standard_normal((rows, n)); dy = rs.standard_normal((rows, n)).astype(F32); scale = (rs.rand(n // div) + 0.5).astype(F32)
    z[0, 0] = 0.0; z[1, 1] = -0.0
    y = (np.maximum(z, 0) if relu else z).astype(F32)
    dzs, db, dbs, gate = R.act_bwd_ref(dy, y, scale, div, relu)
    # y = act(s * u + b): d/du and d/db of <dy, y> through torch
    u = torch.from_numpy(z / np.repeat(scale.astype(F64), div)[None, :]).requires_grad_(True)
    b = torch.zeros(n, dtype=torch.float64, requires_grad=True)
    pre = u * torch.from_numpy(np.repeat(scale.astype(F64), div))[None, :] + b
    out = torch.relu(pre) if relu else pre
    (out * torch.from_numpy(dy.astype(F64))).sum().backward()
    assert rel(dzs, u.grad.numpy()) < 1e-12 and rel(db, b.grad.numpy()) < 1e-12
    assert gate.sum() == (0 if not relu else (~(y > 0)).sum()) and (dzs[gate] == 0).all() and (dbs >= np.abs(db) - 1e-12).all()


@pytest.mark.parametrize("n_mats,elems", [(1, 1), (3, 5), (2, 1025)])
def test_wn_bwd_reference_agrees_with_autograd(n_mats, elems):
    rs = np.random.RandomState(11)
    G = rs.standard_normal((n_mats, elems)).astype(F32); V = rs.standard_normal((n_mats, elems)).astype(F32)
    g = (rs.rand(n_mats) + 0.5).astype(F32)
    dV, dg, sV, sg = R.wn_bwd_ref(G, V, g)
    aV, ag = R.wn_bwd_autograd(G, V, g)
    assert rel(dV, aV) < 1e-12 and rel(dg, ag) < 1e-12
    assert np.isfinite(sV).all() and np.isfinite(sg).all() and (sg >= np.abs(dg) - 1e-12).all()


def test_transpose_and_dropout_references():
    rs = np.random.RandomState(2)
    src = rs.standard_normal((3, 5, 9)).astype(F32); dst0 = np.full((3, 7, 6), -7.0, F32)
    out = R.transpose_ref(src, dst0, 5, 7)
    assert np.array_equal(out[:, :, :5], torch.from_numpy(src[:, :, :7]).transpose(1, 2).numpy()) and (out[:, :, 5:] == -7.0).all()
    x = rs.standard_normal(64).astype(F32); m = rs.randint(0, 2, 64).astype(np.uint8)
    ref = R.dropout_ref(x, m, 0.3)
    want = F.dropout(torch.ones(256, dtype=torch.float64), float(F32(0.3)), True).max().item()        # 1 / (1 - p) as torch scales it
    assert rel(ref, x.astype(F64) * m * want) < 1e-12
    # the kernel's own arithmetic (float32 1 / (1 - p), one product) is within EPS32 * |ref| of it for every float
    inv = F32(1) / (F32(1) - F32(0.3))
    xs = np.concatenate([x, np.linspace(1, 2, 4097).astype(F32)])
    assert (np.abs((xs * inv).astype(F32).astype(F64) - R.dropout_ref(xs, np.ones_like(xs), 0.3)) <= R.EPS32 * np.abs(xs)).all()
    assert abs(R.keep_rate_bound(2 * 4096, 0.3) - 5 * math.sqrt(0.21 / 8192)) < 1e-15


# ---- 3. elementwise and sequence kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_swish_references_agree_with_autograd(n):
    x, dy = R.swish_inputs(n)
    if n >= 7:
        assert set(R.SWISH_SPECIAL.tolist()) <= set(x.tolist())
    xx = torch.from_numpy(x.astype(F64)).requires_grad_(True)
    y = F.silu(xx)
    y.backward(torch.from_numpy(dy.astype(F64)))
    assert np.isfinite(R.swish_ref(x)).all() and rel(R.swish_ref(x), y.detach().numpy()) < 1e-12
    assert np.isfinite(R.swish_bwd_ref(x, dy)).all() and rel(R.swish_bwd_ref(x, dy), xx.grad.numpy()) < 1e-12


def test_sequence_and_axpby_references():
    rs = np.random.RandomState(8)
    x = rs.standard_normal((3, 14, 5)).astype(F32); o = rs.standard_normal((3, 5)).astype(F32); y = rs.standard_normal((3, 5)).astype(F32)
    ref, sc = R.seq_sum_ref(x, 1.0, o)
    assert rel(ref, (torch.from_numpy(x.astype(F64)).sum(1) + torch.from_numpy(o.astype(F64))).numpy()) < 1e-12 and (sc >= np.abs(ref) - 1e-12).all()
    ref, sc = R.seq_sum_ref(np.zeros((2, 0, 7), F32), 0.0, np.full((2, 7), np.nan, F32))
    assert (ref == 0).all() and (sc == 0).all()
    assert np.array_equal(R.seq_bcast_add_ref(x, y, 14), (torch.from_numpy(x) + torch.from_numpy(y)[:, None, :]).numpy())
    assert np.array_equal(R.seq_bcast_add_ref(None, y, 4), torch.from_numpy(y)[:, None, :].expand(3, 4, 5).numpy())
    ref, sc = R.axpby_ref(x, 0.3, x[::-1], -1.7)
    want = float(F32(0.3)) * x.astype(F64) + float(F32(-1.7)) * x[::-1].astype(F64)
    assert rel(ref, want) < 1e-12 and (sc >= np.abs(ref) - 1e-12).all()


def test_embedding_references():
    rs = np.random.RandomState(4)
    t0 = rs.standard_normal((6, 3)).astype(F32); t1 = rs.standard_normal((6, 3)).astype(F32)
    tok = np.array([[0, 5, -1], [6, 2, 2]], dtype=np.int64)
    out, ok = R.embedding_ref(tok, t0, t1)
    assert ok.tolist() == [[True, True, False], [False, True, True]] and out.shape == (2, 3, 6)
    want = torch.cat([F.embedding(torch.from_numpy(tok.clip(0, 5)), torch.from_numpy(t0)), F.embedding(torch.from_numpy(tok.clip(0, 5)), torch.from_numpy(t1))], -1).numpy()
    assert np.array_equal(out[ok], want[ok]) and np.isnan(out[~ok]).all()
    # bf16 bits: round to nearest even, ties included
    a = np.array([1.0, 1.00390625, 1.01171875, -3.140625, 0.0], F32)    # 1 + 2^-8 (tie -> even, down), 1 + 3 * 2^-8 (tie -> even, up)
    assert R.bf16_bits(a).tolist() == [0x3F80, 0x3F80, 0x3F82, 0xC049, 0x0000]


def test_embedding_bwd_emulation_is_the_scatter_add_and_depends_on_the_order():
    tok = R.embedding_bwd_tokens()
    assert (tok[:512] != 31).all() and tok[600] == 31 and (tok == 33).sum() == 300 and tok[3] == tok[700] == 32 and (tok == 32).sum() == 2
    assert (tok == R.EMB_PAD).any() and (tok < 0).any() and (tok >= R.EMB_ROWS).sum() == 2
    rs = np.random.RandomState(21)
    for dim, col_off, ld in ((5, 0, 5), (3, 3, 6)):
        g = rs.standard_normal((len(tok), ld)).astype(F32)
        fwd = R.embedding_bwd_emulated(tok, g, col_off, R.EMB_ROWS, dim, R.EMB_PAD)
        inr = (tok >= 0) & (tok < R.EMB_ROWS)
        w = torch.zeros(R.EMB_ROWS, dim, dtype=torch.float64, requires_grad=True)
        (F.embedding(torch.from_numpy(tok[inr]), w, padding_idx=R.EMB_PAD) * torch.from_numpy(g[inr, col_off:col_off + dim].astype(F64))).sum().backward()
        assert rel(fwd, w.grad.numpy()) < 1e-5 and (fwd[R.EMB_PAD] == 0).all()
        rev = R.embedding_bwd_emulated(tok, g, col_off, R.EMB_ROWS, dim, R.EMB_PAD, reverse=True)
        assert fwd.tobytes() != rev.tobytes()                         # some bit differs: the order matters for these gradients
        assert np.array_equal(fwd[32], rev[32])                       # (two addends commute)
    big = R.embedding_bwd_big_tokens()
    assert len(big) == 65539 and len(np.unique(big)) == 50
    g = np.random.RandomState(22).standard_normal((len(big), 2)).astype(F32)
    assert R.embedding_bwd_emulated(big, g, 0, 64, 2, 0).tobytes() != R.embedding_bwd_emulated(big, g, 0, 64, 2, 0, reverse=True).tobytes()
