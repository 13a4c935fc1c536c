"""Round-3 fusions on an MI355X against the float64 oracle / the unfused forms:
  * cti_triattention_forward with the attention's v projection taken from the caller (`v_tucker_out`), once per image (`v_rep`);
  * the MC / FFOE model forwards at h_mm / rank = 16 -- the shapes that reach the fused few-answer kernel (mask + softmax in its registers), the
    padded batched v projection and the per-image tri pool (the reference fixtures g9_* have h_mm / rank = 4 and take the generic kernels);
  * cti_linear_residual_pb (split-K reduce + broadcast-add + sequence sum in one pass), with and without a K split;
  * the range guard without an auxiliary stream (both scans on the launch stream)."""
import types

import numpy as np
import pytest
import torch

import cti_amd
from oracle import cti_models as OM
from oracle import cti_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
ops = cti_amd.ops


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def sd(m):
    return {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}


@pytest.fixture(params=["bf16x3", "f16f6"], autouse=True)
def precision(request):
    old = cti_amd.get_precision()
    cti_amd.set_precision(request.param)
    yield request.param
    cti_amd.set_precision(old)


@pytest.mark.parametrize("rep", [1, 2, 4])
def test_triattention_takes_the_hoisted_v_projection(rep):
    torch.manual_seed(5 + rep)
    att = cti_amd.TriAttention(40, 32, 24, 64, 1, 4, 2, 1).to(DEV).eval()            # h / R = 16, glimpse 2: the fused few-answer path for A <= 6
    rs = np.random.RandomState(rep)
    Bu, V, Q, A = 3, 7, 5, 3
    vu = np.abs(rs.standard_normal((Bu, V, 40))).astype(np.float32)
    vu[1, 5:] = 0
    v = np.repeat(vu, rep, axis=0)
    q = np.tanh(rs.standard_normal((Bu * rep, Q, 32))).astype(np.float32)
    a = np.tanh(rs.standard_normal((Bu * rep, A, 24))).astype(np.float32)
    assert cti_amd.pkg._lib.lib().cti_triattention_hoist_ok(Bu * rep, V, Q, A, 64, 4, 2, 1) == 1
    with torch.no_grad():
        p0, l0 = att(T(v), T(q), T(a))
        vt = att.TriAtt.v_tucker(T(vu))                                           # (Bu, V, 64): relu(v_tucker(v)), one block per image
        wide = torch.zeros(Bu, V, 96, device=DEV); wide[..., :64] = vt; wide[..., 64:] = 7.0   # a wider row (the padded batch): columns beyond h are ignored
        p1, l1 = att(T(v), T(q), T(a), _v_tucked=wide, _v_rep=rep)
    p_ref, l_ref = O.tri_attention(v, q, a, sd(att), dtype=np.float64)
    fin = np.isfinite(l_ref)
    for p, l, what in ((p0, l0, "plain"), (p1, l1, "hoisted v, rep %d" % rep)):
        assert np.array_equal(np.isfinite(l.cpu().numpy()), fin), what
        assert O.norm_max_err(np.where(fin, l.cpu().numpy(), 0), np.where(fin, l_ref, 0)) < TOL, what
        assert O.norm_max_err(p.cpu().numpy(), p_ref) < TOL, what
    assert float((p1 - p0).abs().max()) <= 2e-6 * float(p0.abs().max())


def _ds(ntoken, v_dim, num_ans):
    return types.SimpleNamespace(dictionary=types.SimpleNamespace(ntoken=ntoken), v_dim=v_dim, num_ans_candidates=num_ans)


def _args(gamma):
    # h_mm * 2 = num_hid like the reference's 512 / 1024 (the pooled (B, h_mm * k) vector feeds q_prj: FCNet([num_hid, num_hid])); h_mm / rank = 16
    return types.SimpleNamespace(op="c", num_hid=64, gamma=gamma, h_mm=32, rank=2, k=1, h_out=1, activation="relu", dropout=0.5, use_counter=False)


@pytest.mark.parametrize("rep", [1, 4])
def test_mc_model_on_the_fused_few_answer_path(rep):
    """MC TanModel with h_mm / rank = 16 (fused modes-1+2+3 kernel with mask + softmax inside, padded batched v projection, MFMA tri pool reading
    one v block per image, fused residual projections) against the float64 oracle of src/MC/base_model.py:128-152."""
    torch.manual_seed(31)
    m = cti_amd.build_mc_cti(_args(2), _ds(50, 48, 2)).to(DEV).eval()
    rs = np.random.RandomState(7)
    Bu = 3
    vu = np.abs(rs.standard_normal((Bu, 9, 48))).astype(np.float32)
    vu[2, 6:] = 0
    v = np.repeat(vu, 4, axis=0)
    q = np.repeat(rs.randint(0, 50, size=(Bu, 7)), 4, axis=0)
    a = rs.randint(0, 50, size=(Bu * 4, 6))
    a[:, 4:] = 50                                                                 # padding tokens
    m.v_replication = rep
    with torch.no_grad():
        out, att = m(T(v), None, T(q.astype(np.int64)), T(a.astype(np.int64)))
    ref, att_ref = OM.mc_tan_forward(v, q, a, sd(m), 2, dtype=np.float64)
    assert O.norm_max_err(att.cpu().numpy(), att_ref) < TOL
    assert O.norm_max_err(out.cpu().numpy(), ref) < TOL


def test_ffoe_models_on_the_fused_paths():
    torch.manual_seed(32)
    cti = cti_amd.build_cti(_args(2), _ds(50, 48, 11)).to(DEV).eval()
    ban = cti_amd.build_ban(_args(4), _ds(50, 48, 11)).to(DEV).eval()
    rs = np.random.RandomState(8)
    v = np.abs(rs.standard_normal((5, 9, 48))).astype(np.float32)
    v[0, 7:] = 0
    q = rs.randint(0, 50, size=(5, 8)).astype(np.int64)
    a = rs.randint(0, 50, size=(5, 3)).astype(np.int64)
    with torch.no_grad():
        lc = cti(T(v), T(q), T(a))
        lb, attb = ban(T(v), None, T(q), None)
    assert O.norm_max_err(lc.cpu().numpy(), OM.ffoe_cti_forward(v, q, a, sd(cti), 2, dtype=np.float64)) < TOL
    rb, ab = OM.ffoe_ban_forward(v, q, sd(ban), 4, dtype=np.float64)
    assert O.norm_max_err(attb.cpu().numpy(), ab) < 1.5e-4
    assert O.norm_max_err(lb.cpu().numpy(), rb) < 1.5e-4


@pytest.mark.parametrize("order", ["cti_first", "ban_first"])
def test_two_models_on_sibling_streams_equal_the_serial_forwards(order):
    """ops.run_concurrently (BASELINE configs[3]: BAN + CTI on one batch): same logits as one model after the other, eagerly and from a replayed
    hipGraph -- in both orders (a sibling under capture runs without the library's auxiliary stream)."""
    torch.manual_seed(33)
    cti = cti_amd.build_cti(_args(2), _ds(50, 48, 11)).to(DEV).eval()
    ban = cti_amd.build_ban(_args(4), _ds(50, 48, 11)).to(DEV).eval()
    rs = np.random.RandomState(9)
    v = T(np.abs(rs.standard_normal((6, 9, 48))).astype(np.float32))
    q = T(rs.randint(0, 50, size=(6, 8)).astype(np.int64))
    a = T(rs.randint(0, 50, size=(6, 3)).astype(np.int64))
    f_cti, f_ban = (lambda: cti(v, q, a)), (lambda: ban(v, None, q, None)[0])

    def both():
        if order == "cti_first":
            return ops.run_concurrently(f_cti, f_ban)
        b, c = ops.run_concurrently(f_ban, f_cti)
        return c, b
    with torch.no_grad():
        lc, lb = f_cti(), f_ban()
        torch.cuda.synchronize()
        for _ in range(3):
            c, b = both()
        torch.cuda.synchronize()
        assert torch.equal(c, lc) and torch.equal(b, lb)
        gr = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(gr, stream=side):
                cg, bg = both()
        torch.cuda.current_stream().wait_stream(side)
        cg.zero_(); bg.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(cg, lc) and torch.equal(bg, lb)


@pytest.mark.parametrize("B,V,Q,A,D,rep", [(5, 9, 7, 3, 64, 1), (4, 36, 14, 3, 1024, 1), (8, 36, 12, 6, 1024, 4), (8, 36, 12, 6, 1024, 1), (3, 10, 5, 4, 72, 1), (2, 36, 12, 3, 96, 1)])
def test_shifted_tri_pool_vs_float64(B, V, Q, A, D, rep):
    """cti_tri_pool_shift_fwd: the q / a operands are relu(row + add[b]) formed on load (product-table, MFMA and streaming kernels, one v block per image)."""
    rs = np.random.RandomState(B * 100 + A)
    vt = rs.standard_normal((B // rep, V, D)).astype(np.float32)
    qt, at = rs.standard_normal((B, Q, D)).astype(np.float32), rs.standard_normal((B, A, D)).astype(np.float32)
    qa, aa = rs.standard_normal((B, D)).astype(np.float32), rs.standard_normal((B, D)).astype(np.float32)
    w = rs.rand(B, V, Q, A, 2).astype(np.float32)
    for use_q, use_a in ((True, True), (False, True), (False, False)):
        out = ops.tri_pool_shift(T(vt), T(qt), T(at), T(qa) if use_q else None, T(aa) if use_a else None, T(w)[..., 1], v_rep=rep)
        assert out is not None
        q_ = np.maximum(qt.astype(np.float64) + (qa[:, None, :] if use_q else 0), 0)
        a_ = np.maximum(at.astype(np.float64) + (aa[:, None, :] if use_a else 0), 0)
        ref = np.einsum("bvd,bvqa,bqd,bad->bd", np.repeat(vt, rep, 0).astype(np.float64), w[..., 1].astype(np.float64), q_, a_)
        assert O.norm_max_err(out.cpu().numpy(), ref) < TOL, (use_q, use_a)


@pytest.mark.parametrize("B,V,Q,D", [(5, 9, 7, 64), (4, 36, 14, 1024), (3, 36, 12, 512), (2, 11, 16, 36)])
def test_shifted_bi_pool_vs_float64(B, V, Q, D):
    rs = np.random.RandomState(B * 10 + Q)
    vt, qt = rs.standard_normal((B, V, D)).astype(np.float32), rs.standard_normal((B, Q, D)).astype(np.float32)
    qa = rs.standard_normal((B, D)).astype(np.float32)
    w = rs.rand(B, 3, V, Q).astype(np.float32)
    for use_q in (True, False):
        out = ops.bi_pool_shift(T(vt), T(qt), T(qa) if use_q else None, T(w)[:, 1])
        assert out is not None
        q_ = np.maximum(qt.astype(np.float64) + (qa[:, None, :] if use_q else 0), 0)
        ref = np.einsum("bvd,bvq,bqd->bd", vt.astype(np.float64), w[:, 1].astype(np.float64), q_)
        assert O.norm_max_err(out.cpu().numpy(), ref) < TOL, use_q
    assert ops.bi_pool_shift(T(vt[:, :, :D - 2].copy()), T(qt[:, :, :D - 2].copy()), None, T(w)[:, 1]) is None      # D % 4 != 0: no kernel with the on-load shift


def test_hoisted_glimpse_loops_equal_the_literal_loops():
    """glimpse_loops' hoisted glimpse loops (q / a projections of the initial sequences in one batched GEMM, the residual's projection added in the pool)
    against the literal loops of src/FFOE/base_model.py:53-64,129-134 -- same module, knob off -- and against the float64 oracle."""
    bm = cti_amd.pkg.glimpse_loops
    torch.manual_seed(34)
    cti = cti_amd.build_cti(_args(3), _ds(50, 48, 11)).to(DEV).eval()
    ban = cti_amd.build_ban(_args(4), _ds(50, 48, 11)).to(DEV).eval()
    rs = np.random.RandomState(10)
    v = np.abs(rs.standard_normal((6, 9, 48))).astype(np.float32)
    v[1, 6:] = 0
    q = rs.randint(0, 50, size=(6, 8)).astype(np.int64)
    a = rs.randint(0, 50, size=(6, 3)).astype(np.int64)
    calls = {"tri": 0, "bi": 0, "multi": 0}
    tps, bps, mps = ops.tri_pool_shift, ops.bi_pool_shift, ops.bi_pool_shift_multi
    ops.tri_pool_shift = lambda *x, **k: (calls.__setitem__("tri", calls["tri"] + 1), tps(*x, **k))[1]
    ops.bi_pool_shift = lambda *x, **k: (calls.__setitem__("bi", calls["bi"] + 1), bps(*x, **k))[1]
    ops.bi_pool_shift_multi = lambda *x, **k: (calls.__setitem__("multi", calls["multi"] + 1), mps(*x, **k))[1]
    try:
        with torch.no_grad():
            lc, (lb, ab) = cti(T(v), T(q), T(a)), ban(T(v), None, T(q), None)
            assert calls == {"tri": 3, "bi": 0, "multi": 4}, calls         # BAN: the UNROLLED loop (round 5: two launches per glimpse on the dependent chain) is what ran
            assert getattr(cti, "_unroll_val", None) is not None           # ... and the CTI model's unrolled form (one product between two pools)
            bm._UNROLL = False
            lc1, (lb1, ab1) = cti(T(v), T(q), T(a)), ban(T(v), None, T(q), None)
            assert calls == {"tri": 6, "bi": 4, "multi": 4}, calls         # ... and with the knob off the hoisted forms of round 4
            bm._HOIST_LOOP = False
            lc0, (lb0, ab0) = cti(T(v), T(q), T(a)), ban(T(v), None, T(q), None)
            assert calls == {"tri": 6, "bi": 4, "multi": 4}
    finally:
        bm._HOIST_LOOP = True
        bm._UNROLL = True
        ops.tri_pool_shift, ops.bi_pool_shift, ops.bi_pool_shift_multi = tps, bps, mps
    assert O.norm_max_err(lc.cpu().numpy(), lc0.cpu().numpy()) < 2e-5 and O.norm_max_err(lb.cpu().numpy(), lb0.cpu().numpy()) < 2e-5
    assert O.norm_max_err(lb1.cpu().numpy(), lb0.cpu().numpy()) < 2e-5 and torch.equal(ab, ab0) and torch.equal(ab1, ab0)
    assert O.norm_max_err(lc1.cpu().numpy(), lc0.cpu().numpy()) < 2e-5
    assert O.norm_max_err(lc.cpu().numpy(), OM.ffoe_cti_forward(v, q, a, sd(cti), 3, dtype=np.float64)) < TOL
    assert O.norm_max_err(lb.cpu().numpy(), OM.ffoe_ban_forward(v, q, sd(ban), 4, dtype=np.float64)[0]) < 1.5e-4


@pytest.mark.parametrize("prec,tol", [("bf16x3", 3e-5), ("bf16", 6e-3), ("f16f6", 3e-5)])
def test_unrolled_ban_loop_at_full_widths_on_every_row(prec, tol):
    """The unrolled glimpse loop of BanModel (8 glimpses, 1 024 wide, B = 256: up to 30 split-K slabs summed inside a pool) against the hoisted loop it replaces and
    the literal loop of src/FFOE/base_model.py:53-61, every row of the logits; the weight-only products C[g][j] follow a parameter change (cache key)."""
    import types
    bm = cti_amd.pkg.glimpse_loops
    old = cti_amd.get_precision()
    cti_amd.set_precision(prec)
    try:
        torch.manual_seed(41)
        ds = types.SimpleNamespace(dictionary=types.SimpleNamespace(ntoken=2000), v_dim=2048, num_ans_candidates=3129)
        margs = types.SimpleNamespace(op="c", num_hid=1024, gamma=8, h_mm=512, rank=32, k=1, h_out=1, activation="relu", dropout=0.5, use_counter=False)
        ban = cti_amd.build_ban(margs, ds).to(DEV).eval()
        g = torch.Generator().manual_seed(42)
        v = torch.randn(256, 36, 2048, generator=g).abs()
        nv = torch.randint(10, 37, (256,), generator=g)
        v[torch.arange(36)[None, :] >= nv[:, None]] = 0
        v = v.to(DEV)
        q = torch.randint(0, 2000, (256, 14), generator=g).to(DEV)
        rel = lambda a, b: float(((a - b).abs().flatten(1).amax(1) / b.abs().max()).max())
        with torch.no_grad():
            lu = ban(v, None, q, None)[0]
            bm._UNROLL = False
            lh = ban(v, None, q, None)[0]
            bm._HOIST_LOOP = False
            ll = ban(v, None, q, None)[0]
            bm._HOIST_LOOP, bm._UNROLL = True, True
            print(prec, "unrolled vs hoisted %.2e, vs literal %.2e" % (rel(lu, lh), rel(lu, ll)))
            assert rel(lu, lh) < tol and rel(lu, ll) < tol
            # a parameter update must rebuild the weight-only products
            ban.q_prj[3].main[1].weight_g.data.mul_(1.5)
            cti_amd.ops.invalidate_caches()
            lu2 = ban(v, None, q, None)[0]
            bm._UNROLL = False
            lh2 = ban(v, None, q, None)[0]
            assert rel(lu2, lh2) < tol and rel(lu2, lu) > 3 * tol
    finally:
        bm._HOIST_LOOP, bm._UNROLL = True, True
        cti_amd.set_precision(old)


@pytest.mark.parametrize("prec,tol", [("bf16x3", 3e-5), ("bf16", 6e-3), ("f16f6", 3e-5)])
@pytest.mark.parametrize("glimpse", [2, 3])
def test_unrolled_tri_loop_at_full_widths_on_every_row(prec, tol, glimpse):
    """The unrolled glimpse loop of the CTI models (glimpse_loops._tri_loop_unrolled: ONE product between two pools, the accumulated residuals in one K-concatenated
    product behind the last pool) against the hoisted loop it replaces and the literal loop of src/MC/base_model.py:145-150, at the Visual7W shapes of
    BASELINE configs[2] (B = 256 rows = 64 images x 4 candidates, 1 024 wide), every row of the logits; a parameter update rebuilds the weight-only products."""
    import types
    bm = cti_amd.pkg.glimpse_loops
    old = cti_amd.get_precision()
    cti_amd.set_precision(prec)
    try:
        torch.manual_seed(43)
        ds = types.SimpleNamespace(dictionary=types.SimpleNamespace(ntoken=2000), v_dim=2048, num_ans_candidates=2)
        margs = types.SimpleNamespace(op="c", num_hid=1024, gamma=glimpse, h_mm=512, rank=32, k=1, h_out=1, activation="relu", dropout=0.5, use_counter=False)
        m = cti_amd.build_mc_cti(margs, ds).to(DEV).eval()
        g = torch.Generator().manual_seed(44)
        vi = torch.randn(64, 36, 2048, generator=g).abs()
        nv = torch.randint(10, 37, (64,), generator=g)
        vi[torch.arange(36)[None, :] >= nv[:, None]] = 0
        v = vi.unsqueeze(1).expand(-1, 4, -1, -1).contiguous().view(256, 36, 2048).to(DEV)
        q = torch.randint(0, 2000, (64, 12), generator=g).unsqueeze(1).expand(-1, 4, -1).contiguous().view(256, 12).to(DEV)
        a = torch.randint(0, 2000, (256, 6), generator=g).to(DEV)
        rel = lambda x, y: float(((x - y).abs().flatten(1).amax(1) / y.abs().max()).max())
        with torch.no_grad():
            lu = m(v, None, q, a)[0]
            assert getattr(m, "_unroll_val", None) is not None             # the unrolled form is what ran
            bm._UNROLL = False
            lh = m(v, None, q, a)[0]
            bm._HOIST_LOOP = False
            ll = m(v, None, q, a)[0]
            bm._HOIST_LOOP, bm._UNROLL = True, True
            print(prec, glimpse, "unrolled vs hoisted %.2e, vs literal %.2e" % (rel(lu, lh), rel(lu, ll)))
            assert rel(lu, lh) < tol and rel(lu, ll) < tol
            # a parameter update must rebuild the weight-only products: the updated unrolled loop follows the updated hoisted loop far more closely than the
            # update moved the logits (with stale products it would sit at the old logits)
            m.a_prj[0].main[1].weight_g.data.mul_(3.0)
            m.q_prj[0].main[1].weight_g.data.mul_(3.0)
            cti_amd.ops.invalidate_caches()
            lu2 = m(v, None, q, a)[0]
            bm._UNROLL = False
            lh2 = m(v, None, q, a)[0]
            print(prec, glimpse, "after the update: unrolled vs hoisted %.2e, moved by %.2e" % (rel(lu2, lh2), rel(lu2, lu)))
            assert rel(lu2, lh2) < tol and rel(lu2, lu) > 4 * rel(lu2, lh2)
    finally:
        bm._HOIST_LOOP, bm._UNROLL = True, True
        cti_amd.set_precision(old)


def test_mc_model_detects_replicated_images_by_itself():
    """TanModel.v_replication = 'auto' (the default; src/MC/train.py:75-79 repeats every image per candidate answer and tells the model nothing): every EAGER
    forward detects the factor of its own batch, the logits equal those of the explicit hint bit for bit and those of the literal all-rows forward to rounding;
    a later batch that is replicated differently -- or not at all -- is simply detected as such and still gives the oracle's logits (round 5, ADVICE r4: the
    factor used to be frozen from the first batch and every batch that broke it was NaN-filled)."""
    torch.manual_seed(35)
    m = cti_amd.build_mc_cti(_args(2), _ds(50, 48, 2)).to(DEV).eval()
    assert m.v_replication == "auto"
    rs = np.random.RandomState(11)
    vu = np.abs(rs.standard_normal((3, 9, 48))).astype(np.float32)
    v = np.repeat(vu, 4, axis=0)
    q = np.repeat(rs.randint(0, 50, size=(3, 7)), 4, axis=0).astype(np.int64)
    a = rs.randint(0, 50, size=(12, 6)).astype(np.int64)
    eq = ops.rows_equal_prev(T(v))
    assert eq.cpu().tolist() == [0, 1, 1, 1] * 3 and ops.replication_of(eq) == 4
    with torch.no_grad():
        out_auto, _ = m(T(v), None, T(q), T(a))
        assert m._v_rep_auto == 4
        m.v_replication = 4
        out_hint, _ = m(T(v), None, T(q), T(a))
        m.v_replication = 1
        out_off, _ = m(T(v), None, T(q), T(a))
        m.v_replication = "auto"
        assert torch.equal(out_auto, out_hint)
        assert O.norm_max_err(out_auto.cpu().numpy(), out_off.cpu().numpy()) < 2e-5
        assert O.norm_max_err(out_auto.cpu().numpy(), OM.mc_tan_forward(v, q, a, sd(m), 2, dtype=np.float64)[0]) < TOL
        v_bad = v.copy()
        v_bad[5, 2, 7] += 1.0                                                  # one element of one repeated row: this batch has no replication at all
        out_bad, _ = m(T(v_bad), None, T(q), T(a))
        assert bool(torch.isfinite(out_bad).all())
        assert O.norm_max_err(out_bad.cpu().numpy(), OM.mc_tan_forward(v_bad, q, a, sd(m), 2, dtype=np.float64)[0]) < TOL
        out_again, _ = m(T(v), None, T(q), T(a))
        assert torch.equal(out_again, out_auto)
        m2 = cti_amd.build_mc_cti(_args(2), _ds(50, 48, 2)).to(DEV).eval()
        v_plain = np.abs(rs.standard_normal((12, 9, 48))).astype(np.float32)
        out_plain, _ = m2(T(v_plain), None, T(q), T(a))
        assert m2._v_rep_auto == 1 and bool(torch.isfinite(out_plain).all())
        assert O.norm_max_err(out_plain.cpu().numpy(), OM.mc_tan_forward(v_plain, q, a, sd(m2), 2, dtype=np.float64)[0]) < TOL


def test_mc_model_auto_replication_first_batch_one_image_then_mixed():
    """The reference's eval loader is unshuffled and sorted by question id (consecutive Visual7W questions share an image): a first batch made of ONE image
    (r = 8 detected where the pipeline's factor is 4), then a batch that crosses an image boundary.  Both give the oracle's logits; what a captured graph would use
    afterwards is the gcd of what was seen (4)."""
    torch.manual_seed(36)
    m = cti_amd.build_mc_cti(_args(2), _ds(50, 48, 2)).to(DEV).eval()
    rs = np.random.RandomState(12)
    img = np.abs(rs.standard_normal((3, 9, 48))).astype(np.float32)
    v1 = np.repeat(img[:1], 8, axis=0)                                         # two questions about image 0, four candidates each
    v2 = np.concatenate([np.repeat(img[1:2], 4, axis=0), np.repeat(img[2:3], 4, axis=0)])    # one question each about images 1 and 2
    q = np.repeat(rs.randint(0, 50, size=(2, 7)), 4, axis=0).astype(np.int64)
    a = rs.randint(0, 50, size=(8, 6)).astype(np.int64)
    with torch.no_grad():
        o1, _ = m(T(v1), None, T(q), T(a))
        assert m._v_rep_auto == 8
        o2, _ = m(T(v2), None, T(q), T(a))
        assert m._v_rep_auto == 4
    for o, v in ((o1, v1), (o2, v2)):
        assert bool(torch.isfinite(o).all())
        assert O.norm_max_err(o.cpu().numpy(), OM.mc_tan_forward(v, q, a, sd(m), 2, dtype=np.float64)[0]) < TOL


def test_mc_model_auto_replication_under_graph_capture_checks_every_replay_on_the_device():
    """Under hipGraph capture the host cannot detect anything: the captured forward uses the factor the eager forwards have seen (their gcd), re-checks every
    replayed batch on the device and NaN-fills the logits of a batch that breaks it -- never a plausible wrong answer."""
    torch.manual_seed(37)
    m = cti_amd.build_mc_cti(_args(2), _ds(50, 48, 2)).to(DEV).eval()
    rs = np.random.RandomState(13)
    vu = np.abs(rs.standard_normal((3, 9, 48))).astype(np.float32)
    v = np.repeat(vu, 4, axis=0)
    q = np.repeat(rs.randint(0, 50, size=(3, 7)), 4, axis=0).astype(np.int64)
    a = rs.randint(0, 50, size=(12, 6)).astype(np.int64)
    vs, qs, as_ = T(v), T(q), T(a)
    with torch.no_grad():
        eager, _ = m(vs, None, qs, as_)
        assert m._v_rep_auto == 4
        gr = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(gr, stream=side):
                out, _ = m(vs, None, qs, as_)
        torch.cuda.current_stream().wait_stream(side)
        gr.replay(); torch.cuda.synchronize()
        assert torch.equal(out, eager)
        vs[5, 2, 7] += 1.0                                                     # the replayed batch no longer consists of groups of four identical images
        gr.replay(); torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())
        vs.copy_(T(v))
        gr.replay(); torch.cuda.synchronize()
        assert torch.equal(out, eager)


@pytest.mark.parametrize("B,G,V,Q,D", [(4, 8, 36, 14, 3072), (3, 2, 9, 7, 96), (2, 4, 50, 16, 128)])
def test_bi_logits_in_the_plain_bf16_mode(B, G, V, Q, D):
    """cti_bi_logits_prec_fwd with CTI_PREC_BF16: ONE bf16 product per pair (what set_precision('bf16') asks for) -- against the float64 contraction of the
    bf16-rounded operands (tight: only the accumulation order differs) and of the fp32 operands (the mode's 1e-2 class)."""
    rs = np.random.RandomState(B + D)
    vt, qt = rs.standard_normal((B, V, D)).astype(np.float32), rs.standard_normal((B, Q, D)).astype(np.float32)
    h, hb = (rs.standard_normal((G, D)) / np.sqrt(D)).astype(np.float32), rs.standard_normal(G).astype(np.float32)
    hs = np.array([1.3], np.float32)
    old = cti_amd.get_precision()
    try:
        cti_amd.set_precision("bf16")
        out = ops.bi_logits(T(vt), T(qt), T(h), T(hs), T(hb)).cpu().numpy()
        cti_amd.set_precision("bf16x3")
        out3 = ops.bi_logits(T(vt), T(qt), T(h), T(hs), T(hb)).cpu().numpy()
    finally:
        cti_amd.set_precision(old)
    bf = lambda x: torch.from_numpy(x).to(torch.bfloat16).to(torch.float64).numpy()
    hq = bf((h[None, :, None, :] * qt[:, None, :, :]).astype(np.float32))                      # (B, G, Q, D): the right operand is formed in fp32, then rounded
    ref_bf = 1.3 * np.einsum("bvd,bgqd->bgvq", bf(vt), hq) + hb[None, :, None, None]
    ref = 1.3 * np.einsum("bvd,gd,bqd->bgvq", vt.astype(np.float64), h.astype(np.float64), qt.astype(np.float64)) + hb[None, :, None, None]
    assert O.norm_max_err(out, ref_bf) < 2e-5
    assert O.norm_max_err(out, ref) < 1e-2
    assert O.norm_max_err(out3, ref) < TOL


@pytest.mark.parametrize("rows,K,N", [(256, 2048, 2), (7, 100, 1), (33, 513, 8), (5, 64, 3)])
def test_linear_with_a_handful_of_outputs(rows, K, N):
    """cti_linear_small_n (the MC models' answer head, src/classifier.py:26 with out_dim = 2): exact fp32, scale + bias + optional ReLU, against float64."""
    rs = np.random.RandomState(rows + N)
    x, w = rs.standard_normal((rows, K)).astype(np.float32), (rs.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias, scale = rs.standard_normal(N).astype(np.float32), np.array([0.7], np.float32)
    with torch.no_grad():
        for relu in (False, True):
            y = ops.wn_linear(T(x), T(w), T(scale), N, T(bias), relu)
            ref = 0.7 * (x.astype(np.float64) @ w.astype(np.float64).T) + bias
            assert O.norm_max_err(y.cpu().numpy(), np.maximum(ref, 0) if relu else ref) < 2e-6, relu
        y = ops.wn_linear(T(x), T(w), None, N, None, False)
        assert O.norm_max_err(y.cpu().numpy(), x.astype(np.float64) @ w.astype(np.float64).T) < 2e-6


def test_shifted_tri_pool_and_sums_in_the_plain_bf16_mode():
    """set_precision('bf16'): the MFMA tri pool with ONE bf16 product per pair (use_mfma = 2) in the mode's 1e-2 class; cti_joint_sums against float64."""
    rs = np.random.RandomState(77)
    B, V, Q, A, D = 8, 36, 12, 6, 1024
    vt, qt, at = rs.standard_normal((B, V, D)).astype(np.float32), rs.standard_normal((B, Q, D)).astype(np.float32), rs.standard_normal((B, A, D)).astype(np.float32)
    qa, aa = rs.standard_normal((B, D)).astype(np.float32), rs.standard_normal((B, D)).astype(np.float32)
    w = rs.rand(B, V, Q, A).astype(np.float32)
    ref = np.einsum("bvd,bvqa,bqd,bad->bd", vt.astype(np.float64), w.astype(np.float64), np.maximum(qt.astype(np.float64) + qa[:, None], 0), np.maximum(at.astype(np.float64) + aa[:, None], 0))
    old = cti_amd.get_precision()
    try:
        cti_amd.set_precision("bf16")
        out = ops.tri_pool_shift(T(vt), T(qt), T(at), T(qa), T(aa), T(w))
    finally:
        cti_amd.set_precision(old)
    assert out is not None and 1e-6 < O.norm_max_err(out.cpu().numpy(), ref) < 1e-2
    js = ops.joint_sums(T(qt), 2.0, T(at), 1.0, T(qa), 12.0, T(aa), 6.0).cpu().numpy()
    assert O.norm_max_err(js, 2.0 * qt.astype(np.float64).sum(1) + at.astype(np.float64).sum(1) + 12.0 * qa + 6.0 * aa) < 2e-6
    js = ops.joint_sums(T(qt), 8.0, Dq=T(qa), dq=14.0).cpu().numpy()
    assert O.norm_max_err(js, 8.0 * qt.astype(np.float64).sum(1) + 14.0 * qa) < 2e-6


@pytest.mark.parametrize("n,rows,K,N", [(2, 256, 1024, 1024), (3, 64, 512, 256), (2, 5, 96, 40)])
def test_batched_linears_with_and_without_a_k_split(n, rows, K, N):
    """fc.BatchedLinears (the CTI glimpse loop's paired projections): n layers on a shared input / on n stacked inputs as ONE batched GEMM -- at 2 x (256 x 1024 x 1024)
    the batch splits K too (partials [K range][batch][M][N], one batched reduce pass) -- against float64, every entry."""
    BatchedLinears, WNLinear = cti_amd.pkg.fc.BatchedLinears, cti_amd.WNLinear
    torch.manual_seed(40 + n)
    layers = [WNLinear(K, N).to(DEV) for _ in range(n)]
    for l in layers:
        l.bias.data.normal_()
    bl = BatchedLinears(layers)
    rs = np.random.RandomState(n * 7 + rows)
    x = rs.standard_normal((rows, K)).astype(np.float32)
    xs = rs.standard_normal((n, rows, K)).astype(np.float32)
    with torch.no_grad():
        ys, yt, yn = bl.shared(T(x)), bl.stacked(T(xs)), bl.stacked(T(xs), bias=False, relu=True)
    for i, l in enumerate(layers):
        w = l.weight_v.detach().cpu().numpy().astype(np.float64)
        sc = float(l.weight_g.detach().cpu()) / np.linalg.norm(w)
        b_ = l.bias.detach().cpu().numpy().astype(np.float64)
        assert O.norm_max_err(ys[i].cpu().numpy(), sc * (x.astype(np.float64) @ w.T) + b_) < TOL
        assert O.norm_max_err(yt[i].cpu().numpy(), sc * (xs[i].astype(np.float64) @ w.T) + b_) < TOL
        assert O.norm_max_err(yn[i].cpu().numpy(), np.maximum(sc * (xs[i].astype(np.float64) @ w.T), 0)) < TOL


def test_pools_beside_the_bf16x3_gru_on_another_stream():
    """Round 4: with the BAN and the CTI forward on sibling streams, bi-pool launches that ran while the other stream's fp32-grade GRU step kernel
    (gru_step_fused_kernel<3, 1>) was resident came back with 16 lanes of one register wrong -- the pool kept a zero float4 in SCRATCH (an lvalue
    conditional `c ? *p : z4`) and the 64-byte scratch row did not survive.  The pools are scratch-free now (tests/test_abi.py pins the list of kernels
    that have a private segment); this is the reproducer: 200 pool launches beside GRU forwards, every one bit-equal to a launch on an idle device."""
    import types
    old = cti_amd.get_precision()
    cti_amd.set_precision("bf16x3")
    try:
        g = torch.Generator().manual_seed(7)
        B = 256
        ds = types.SimpleNamespace(dictionary=types.SimpleNamespace(ntoken=2000), v_dim=2048, num_ans_candidates=16)
        ma = types.SimpleNamespace(op="c", num_hid=1024, gamma=2, h_mm=512, rank=32, k=1, h_out=1, activation="relu", dropout=0.5, use_counter=False)
        torch.manual_seed(3)
        m = cti_amd.build_cti(ma, ds).to(DEV).eval()
        q = torch.randint(0, 2000, (B, 14), generator=g).to(DEV)
        vp = torch.randn(B, 36, 1024, generator=g).to(DEV)
        qn = torch.randn(B, 14, 1024, generator=g).to(DEV)
        an = torch.randn(B, 3, 1024, generator=g).to(DEV)
        att = torch.rand(B, 36, 14, generator=g).to(DEV)
        att3 = torch.rand(B, 36, 14, 3, generator=g).to(DEV)
        v3 = torch.randn(B, 36, 3072, generator=g).to(DEV)
        q3 = torch.randn(B, 14, 3072, generator=g).to(DEV)
        big = torch.randn(6144, 6144, device=DEV)
        side = torch.cuda.Stream()
        with torch.no_grad():
            emb = m.w_emb(q)
            ref = [ops.bi_pool(vp, qn, att, 1).clone(), ops.bi_pool(v3, q3, att, 3).clone(), ops.tri_pool(vp, qn, an, att3).clone()]
            torch.cuda.synchronize()
            bad = 0
            for rep in range(5):
                cur = torch.cuda.current_stream()
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    _ = big @ big                                           # head start for the host: the pools below are still queued when the GRU starts
                    outs = [(ops.bi_pool(vp, qn, att, 1), ops.bi_pool(v3, q3, att, 3), ops.tri_pool(vp, qn, an, att3)) for _ in range(40)]
                m.q_emb.forward_all(emb)
                cur.wait_stream(side)
                torch.cuda.synchronize()
                bad += sum(0 if all(torch.equal(o, r) for o, r in zip(trip, ref)) else 1 for trip in outs)
        assert bad == 0, "%d of 200 pool launches differ from the launch on an idle device" % bad
    finally:
        cti_amd.set_precision(old)


@pytest.mark.parametrize("B,L,N,K", [(256, 14, 1024, 1024), (5, 3, 36, 40), (64, 12, 128, 96), (1, 1, 4, 8)])
def test_linear_residual_reduces_adds_and_sums_in_one_pass(B, L, N, K):
    """out = seq + (scale * x @ W^T + bias)[:, None, :]; acc = beta * acc + out.sum(1): with a K split (256 x 1024 x 1024) and without."""
    rs = np.random.RandomState(B + N)
    x = rs.standard_normal((B, K)).astype(np.float32)
    w = (rs.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rs.standard_normal(N).astype(np.float32)
    seq = rs.standard_normal((B, L, N)).astype(np.float32)
    acc0 = rs.standard_normal((B, N)).astype(np.float32)
    scale = np.float32(1.7)
    wp = ops.split_operand(T(w))
    acc = T(acc0.copy())
    out = ops.linear_residual(T(x), wp, T(np.array([scale], np.float32)), N, T(bias), T(seq), acc=acc, beta=0.5)
    assert out is not None
    y = scale * (x.astype(np.float64) @ w.astype(np.float64).T) + bias
    ref = seq + y[:, None, :]
    assert O.norm_max_err(out.cpu().numpy(), ref) < TOL
    assert O.norm_max_err(acc.cpu().numpy(), 0.5 * acc0 + ref.sum(1)) < TOL
    out2 = ops.linear_residual(T(x), wp, None, 1, None, T(seq))                 # no scale, no bias, no accumulator
    assert O.norm_max_err(out2.cpu().numpy(), seq + (x.astype(np.float64) @ w.astype(np.float64).T)[:, None, :]) < TOL


def test_linear_residual_declines_what_it_cannot_do():
    x, seq = torch.randn(4, 8, device=DEV), torch.randn(4, 3, 6, device=DEV)     # N % 4 != 0
    assert ops.linear_residual(x, ops.split_operand(torch.randn(6, 8, device=DEV)), None, 1, None, seq) is None


@pytest.mark.parametrize("mode", ["sync", "poison"])
def test_range_guard_reads_no_unwritten_workspace_without_an_auxiliary_stream(precision, mode):
    """with no auxiliary stream and per-call weights (prepared=None) the early scan used to read the a-side weights' scale planes BEFORE
    side(2) encoded them.  On a workspace pre-filled with 0xFF (saturated scale bytes) in-range inputs must neither trip ('sync') nor come back as
    NaN ('poison')."""
    if precision != "f16f6":
        pytest.skip("the guard belongs to the f16f6 kernels")
    torch.manual_seed(11)
    net = cti_amd.TCNet(48, 40, 24, 64, 1, 4, 2).to(DEV).eval()
    rs = np.random.RandomState(5)
    v = T(np.abs(rs.standard_normal((2, 9, 48))).astype(np.float32))
    q = T(rs.standard_normal((2, 5, 40)).astype(np.float32))
    a = T(rs.standard_normal((2, 40, 24)).astype(np.float32))
    tucker, rank = net._fused_args()
    old_aux, old_fill = ops.use_aux_stream, ops._debug_ws_fill
    ops.use_aux_stream = False
    ops._range_log.update(consecutive=0, skip=0)
    cti_amd.set_range_check(mode)
    try:
        with torch.no_grad():
            ref = net(v, q, a).cpu().numpy()                     # the module's own path (prepared block): the reference for this test
        before = ops.f16f6_range_status()
        ops._debug_ws_fill = 0xFF
        with torch.no_grad():
            out = ops.tcnet_forward(v, q, a, tucker, rank, net.T_g.detach(), prepared=None).cpu().numpy()
        after = ops.f16f6_range_status()
    finally:
        ops.use_aux_stream, ops._debug_ws_fill = old_aux, old_fill
        cti_amd.set_range_check("sync")
        ops._range_log.update(consecutive=0, skip=0)
    assert after["trips"] == before["trips"], after
    assert np.isfinite(out).all()
    assert np.max(np.abs(out - ref)) <= 1e-5 * np.max(np.abs(ref))


def test_range_guard_without_an_auxiliary_stream(precision):
    """CTI_NO_AUX_STREAM: both guard scans run on the launch stream; clean inputs pass, scaled inputs trip and the re-run is fp32-grade."""
    if precision != "f16f6":
        pytest.skip("the guard belongs to the f16f6 kernels")
    import warnings
    torch.manual_seed(9)
    net = cti_amd.TCNet(48, 40, 24, 64, 1, 4, 2).to(DEV).eval()
    rs = np.random.RandomState(3)
    v = np.abs(rs.standard_normal((2, 9, 48))).astype(np.float32)
    q = rs.standard_normal((2, 5, 40)).astype(np.float32)
    a = rs.standard_normal((2, 40, 24)).astype(np.float32)
    old = ops.use_aux_stream
    ops.use_aux_stream = False
    ops._range_log.update(consecutive=0, skip=0)
    try:
        before = ops.f16f6_range_status()
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            o1 = net(T(v), T(q), T(a)).cpu().numpy()
            mid = ops.f16f6_range_status()
            o2 = net(T(v * 1000), T(q * 1000), T(a * 1000)).cpu().numpy()
        after = ops.f16f6_range_status()
    finally:
        ops.use_aux_stream = old
        ops._range_log.update(consecutive=0, skip=0)
    assert mid["trips"] == before["trips"] and after["trips"] == mid["trips"] + 1
    assert O.norm_max_err(o1, O.tcnet_forward(v, q, a, sd(net), dtype=np.float64)) < TOL
    assert O.norm_max_err(o2, O.tcnet_forward(v * 1000, q * 1000, a * 1000, sd(net), dtype=np.float64)) < TOL


@pytest.mark.parametrize("B,V,Q,D", [(256, 36, 14, 3072), (3, 5, 4, 36), (2, 64, 16, 96), (4, 7, 3, 30)])
def test_bi_pool_k3_dedicated_kernel(B, V, Q, D):
    """BCNet(k=3).forward_with_weights (src/bc.py:73-77): out[b, n] = sum_{t<3} sum_vq vt[b,v,3n+t] w[b,v,q] qt[b,q,3n+t], a strided attention slice."""
    rs = np.random.RandomState(D + V)
    vt = rs.standard_normal((B, V, D)).astype(np.float32)
    qt = rs.standard_normal((B, Q, D)).astype(np.float32)
    att = rs.random_sample((B, 3, V, Q)).astype(np.float32)
    w = T(att)[:, 1]                                                              # (B, V, Q) view with a batch stride of 3 * V * Q
    out = ops.bi_pool(T(vt), T(qt), w, 3)
    ref = np.einsum("bvd,bvq,bqd->bd", vt.astype(np.float64), att[:, 1].astype(np.float64), qt.astype(np.float64)).reshape(B, D // 3, 3).sum(-1)
    assert tuple(out.shape) == (B, D // 3)
    assert O.norm_max_err(out.cpu().numpy(), ref) < 1e-5


@pytest.mark.parametrize("B,G,V,Q,D", [(5, 8, 36, 14, 3072), (3, 2, 36, 12, 1024), (2, 1, 1, 1, 32), (2, 8, 64, 16, 96), (4, 3, 17, 5, 992)])
def test_biattention_mask_and_softmax_inside_the_logits_launch(B, G, V, Q, D):
    """cti_biattention_fwd (logits + -inf fill + softmax in the logits kernel's launch; src/attention.py:29-40) against the separate kernels it replaces:
    both K-split forms (D >= 1024: two workgroups add into a sample's logits, the last one runs the softmax), a fully masked sample (the reference's NaN row),
    no mask, ragged shapes; twice in a row (the per-sample counters must come back to zero)."""
    import os
    ops = cti_amd.ops
    g = torch.Generator().manual_seed(B * 31 + D)
    vt = torch.randn(B, V, D, generator=g).to(DEV); qt = torch.randn(B, Q, D, generator=g).to(DEV)
    h = (torch.randn(G, D, generator=g) / 8).to(DEV); hb = torch.randn(G, generator=g).to(DEV); hs = torch.tensor([0.7], device=DEV)
    mask = (torch.rand(B, V, generator=g) < 0.3).to(torch.uint8)
    mask[0] = 1                                                           # sample 0: every object row masked
    if B > 1:
        mask[1] = 0
    mask = mask.to(DEV)
    old = ops.get_precision()
    try:
        ops.set_precision("bf16x3")
        for m in (mask, None):
            os.environ["CTI_BIATT_FUSED"] = "0"
            p_ref, l_ref = ops.biattention_forward(vt, qt, h, hs, hb, m)
            os.environ["CTI_BIATT_FUSED"] = "1"
            for _ in range(2):
                p, l = ops.biattention_forward(vt, qt, h, hs, hb, m)
                assert torch.equal(torch.isneginf(l), torch.isneginf(l_ref))
                assert torch.equal(torch.isnan(p), torch.isnan(p_ref))
                fin = ~torch.isneginf(l_ref)
                assert float((l[fin] - l_ref[fin]).abs().max()) <= 2e-5 * float(l_ref[fin].abs().max())
                ok = ~torch.isnan(p_ref)
                # (round 6: the separate logits launch is the barrier-free K-split kernel, the fused one the LDS form -- eight partial sums against two, so
                # the logits agree to fp32 rounding (above) and p is checked against the softmax of the fused launch's OWN logits)
                p_own = torch.softmax(l.double().reshape(B, G, V * Q), 2).reshape(p.shape)
                assert float((p[ok].double() - p_own[ok]).abs().max()) < 2e-6
                assert float((p[ok] - p_ref[ok]).abs().max()) < 5e-4
                if m is not None:
                    assert bool(torch.isnan(p[0]).all())                  # the fully masked sample
    finally:
        os.environ.pop("CTI_BIATT_FUSED", None)
        ops.set_precision(old)


@pytest.mark.parametrize("config", ["c3", "c4"])
def test_full_batch_model_forward_agrees_across_precisions_on_every_row(config):
    """BASELINE configs[2] / [3] at their full batch (256 rows): the plain-bf16 forward (what bench.py times), the bf16x3 and the f16f6 forwards against the exact-fp32 forward on EVERY row -- the
    oracle check of the bench line looks at the first four samples only, which is how a tile-geometry bug that zeroed the last rows of every 256-row GEMM tile
    went unseen."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    old = cti_amd.get_precision()
    try:
        outs = {}
        for prec in ("bf16", "bf16x3", "f16f6", "fp32"):
            cti_amd.set_precision(prec)
            torch.manual_seed(5)
            s = bench.model_setup(config, 256, 0, torch.device(DEV))
            with torch.no_grad():
                o = s["fwd"]()
            outs[prec] = [t.float() for t in (o if isinstance(o, (tuple, list)) else (o,))]
        for prec, tol in (("bf16", 2e-2), ("bf16x3", 1e-4), ("f16f6", 1e-4)):           # against the exact-fp32 mode, every row (north_star's tolerance)
            for a, b in zip(outs[prec], outs["fp32"]):
                assert a.shape == b.shape and torch.isfinite(a).all()
                per_row = (a - b).abs().flatten(1).amax(1) / b.abs().max()
                assert float(per_row.max()) < tol, (config, prec, float(per_row.max()), int(per_row.argmax()))
    finally:
        cti_amd.set_precision(old)


def test_an_initialiser_applied_through_module_apply_refreshes_the_derived_weight_caches():
    """VERDICT r5 #7c: the reference re-initialises networks with `net.apply(weights_init)` (src/utils.py:61-70,77), whose body writes through `param.data` --
    no autograd version moves, no storage changes, so the cache keys of the weight-norm scales, operand planes, packed rank nets and the unrolled loops' weight
    products would all still match.  The package's modules override .apply to bump the cache epoch: a forward after such an .apply equals a FRESH module
    loaded with the same parameters, in the unrolled BAN loop (the deepest stack of derived weights) and in the fused TCNet.forward."""
    def init(m):                                   # the reference's idiom on this package's parameter names (its nn.Linear weight is weight_v here)
        if isinstance(m, cti_amd.pkg.fc.WNLinear):
            m.weight_v.data.normal_(0.0, 0.02)
    ds = types.SimpleNamespace(dictionary=types.SimpleNamespace(ntoken=2000), v_dim=2048, num_ans_candidates=100)
    args = types.SimpleNamespace(op="c", num_hid=1024, gamma=4, h_mm=512, rank=32, k=1, h_out=1, activation="relu", dropout=0.5, use_counter=False)
    torch.manual_seed(3)
    ban = cti_amd.build_ban(args, ds).to(DEV).eval()
    g = torch.Generator().manual_seed(4)
    v = torch.randn(64, 36, 2048, generator=g).abs().to(DEV)
    q = torch.randint(0, 2000, (64, 14), generator=g).to(DEV)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    with torch.no_grad():
        before = ban(v, None, q, None)[0]
        torch.manual_seed(9)
        ban.apply(init)
        after = ban(v, None, q, None)[0]
        fresh = cti_amd.build_ban(args, ds).to(DEV).eval()
        fresh.load_state_dict(ban.state_dict())
        want = fresh(v, None, q, None)[0]
    assert rel(after, want) < 1e-6 and rel(after, before) > 1e-2, (rel(after, want), rel(after, before))
    torch.manual_seed(3)
    net = cti_amd.TCNet(2048, 1024, 300, 512, 1, 32, 2).to(DEV).eval()
    vv, qq, aa = torch.randn(2, 36, 2048, generator=g).to(DEV), torch.randn(2, 14, 1024, generator=g).to(DEV), torch.randn(2, 40, 300, generator=g).to(DEV)
    with torch.no_grad():
        b0 = net(vv, qq, aa)
        torch.manual_seed(9)
        net.apply(init)
        a0 = net(vv, qq, aa)
        fresh = cti_amd.TCNet(2048, 1024, 300, 512, 1, 32, 2).to(DEV).eval()
        fresh.load_state_dict(net.state_dict())
        w0 = fresh(vv, qq, aa)
    assert rel(a0, w0) < 1e-6 and rel(a0, b0) > 1e-2, (rel(a0, w0), rel(a0, b0))


@pytest.mark.parametrize("config", ["c3", "c4"])
@pytest.mark.parametrize("prec", ["bf16", "f16f6"])
def test_full_batch_model_forward_against_the_oracle_on_spread_rows(config, prec):
    """VERDICT r5 #7b: BASELINE configs[2] / [3] at their full batch against the ORACLE (oracle/cti_models.py, numpy fp32 restatement of src/MC/base_model.py:128-152
    and src/FFOE/base_model.py:37-67,112-136) inside pytest, on 17 rows spread over the batch (every 16th and the last) -- bench.py checks the first four of its timed
    forward, and the every-row tests above compare this package's modes with each other.  bf16 = the dtype the configs name (tolerance 2e-2 on the logits, as the
    bench line's), f16f6 = the package default (1e-4)."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    old = cti_amd.get_precision()
    try:
        cti_amd.set_precision(prec)
        torch.manual_seed(5)
        s = bench.model_setup(config, 256, 0, torch.device(DEV))
        with torch.no_grad():
            out = s["fwd"]()
        rows = list(range(0, 256, 16)) + [255]
        for name, got, ref in s["oracle"](len(rows), out, rows=rows):
            assert got.shape == ref.shape and np.isfinite(got).all()
            err = float(np.max(np.abs(got.astype(np.float64) - ref)) / np.max(np.abs(ref)))
            print("%s %s %s: %.2e over %d rows" % (config, prec, name, err, len(rows)))
            assert err < bench.MODEL_TOL[prec], (config, prec, name, err)
    finally:
        cti_amd.set_precision(old)


def test_full_batch_gradients_agree_across_precisions():
    """The CTI fusion block of `bench.py --mode train` at its full batch (256 rows, V = 36, Q = 12, A = 3): every parameter's gradient in the bf16x3 mode (matrix-core
    M-build backward, split-K weight-gradient GEMMs, 256-row tiles) against the exact-fp32 mode.  eval() keeps dropout out of the comparison; autograd still runs the
    op-by-op path.  Whole-launch coverage of the backward at the data-parallel step's shapes (BASELINE configs[4])."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    B = 256
    g = torch.Generator().manual_seed(11)
    v = torch.randn(B, 36, 2048, generator=g).abs_()
    for b in range(B):
        v[b, int(torch.randint(10, 37, (1,), generator=g)):] = 0
    v = v.to(DEV)
    q = torch.tanh(torch.randn(B, 12, 1024, generator=g)).to(DEV); a = torch.tanh(torch.randn(B, 3, 1024, generator=g)).to(DEV)
    y = (torch.rand(B, 3129, generator=g) > 0.999).float().to(DEV)
    crit = cti_amd.BCEWithLogitsSum()
    old = cti_amd.get_precision()
    grads = {}
    try:
        for prec in ("bf16x3", "bf16", "fp32"):
            cti_amd.set_precision(prec)
            torch.manual_seed(3)
            model = bench.CTIFusionBlock(cti_amd).to(DEV).eval()
            loss = crit(model(v, q, a), y) / B
            loss.backward()
            grads[prec] = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
            assert len(grads[prec]) > 20
    finally:
        cti_amd.set_precision(old)
    # Metric: relative L2 error per tensor.  The two modes' forward values differ by ~1e-6, so a handful of the 4.7 M pre-activations per layer that sit within
    # that distance of zero take the other side of the ReLU kink; each flip moves single gradient entries by O(1) of their size (measured: 2e-2 of a tensor's
    # largest entry, on WNLinearFn alone against float64 autograd), which a max-norm would report as a mismatch and an L2 norm weighs as what it is.
    for mode, t_tensor, t_total in (("bf16x3", 5e-2, 2e-3), ("bf16", 0.3, 5e-2)):
        worst = ("", 0.0)
        for n, g32 in grads["fp32"].items():
            gx = grads[mode][n]
            assert torch.isfinite(gx).all(), n
            den = float(g32.double().norm())
            if den == 0.0:
                assert float(gx.abs().max()) == 0.0, n
                continue
            e = float((gx.double() - g32.double()).norm()) / den
            if mode == "bf16" and g32.numel() == 1:
                continue                    # weight_g: <G, V> / g, a scalar left over from a million cancelling terms -- meaningless at 8 mantissa bits
            if e > worst[1]:
                worst = (n, e)
        assert worst[1] < t_tensor, (mode, worst)                                  # a tile of zeros / a dropped K tail shows up as 0.1-1 here (bf16x3), 0.5+ (bf16)
        flat32 = torch.cat([t.double().flatten() for t in grads["fp32"].values()])
        flatx = torch.cat([grads[mode][n].double().flatten() for n in grads["fp32"]])
        tot = float((flatx - flat32).norm() / flat32.norm())
        assert tot < t_total, (mode, tot)                                          # all 30 M gradient entries together


def test_full_batch_model_gradients_agree_across_precisions():
    """BAN (8 glimpses) and the CTI model of BASELINE configs[3] at B = 256, gradients enabled (eval(): no dropout noise): every parameter gradient -- word embedding,
    GRU, BiAttention / TriAttention, pooling networks, classifier -- in the bf16x3 mode against the exact-fp32 mode (L2 metrics, see the fusion-block test).  These
    are the shapes at which the weight-gradient GEMMs plan for 256 x 256 tiles and split K over the 9 216 rows."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    old = cti_amd.get_precision()
    try:
        grads = {}
        for prec in ("bf16x3", "fp32"):
            cti_amd.set_precision(prec)
            torch.manual_seed(5)
            s = bench.model_setup("c4", 256, 0, torch.device(DEV))
            outs = s["fwd"]()
            loss = sum((o.float() * torch.linspace(-1, 1, o.shape[-1], device=o.device)).sum() for o in outs) / 256
            loss.backward()
            grads[prec] = {}
            for mname, m in s["models"].items():
                for n, p in m.named_parameters():
                    if p.grad is not None:
                        grads[prec][mname + "." + n] = p.grad.detach().clone()
            assert len(grads[prec]) > 40
    finally:
        cti_amd.set_precision(old)
    flat32 = torch.cat([t.double().flatten() for t in grads["fp32"].values()])
    flatx = torch.cat([grads["bf16x3"][n].double().flatten() for n in grads["fp32"]])
    gnorm = float(flat32.norm())
    worst = ("", 0.0)
    for n, g32 in grads["fp32"].items():
        gx = grads["bf16x3"][n]
        assert torch.isfinite(gx).all(), n
        den = float(g32.double().norm())
        if den < 1e-5 * gnorm:              # e.g. the attention logits' bias: its gradient is the sum of a softmax backward, zero up to rounding in either mode
            assert float(gx.double().norm()) < 1e-4 * gnorm, n
            continue
        e = float((gx.double() - g32.double()).norm()) / den
        if e > worst[1]:
            worst = (n, e)
    assert worst[1] < 5e-2, worst
    tot = float((flatx - flat32).norm() / gnorm)
    assert tot < 2e-3, tot


@pytest.mark.parametrize("config", ["c3", "c4"])
@pytest.mark.parametrize("prec", ["bf16", "f16f6"])
def test_full_batch_graph_replay_equals_eager_on_every_row(config, prec):
    """What bench.py times for configs[2] / [3] is a hipGraph REPLAY of the forward (two streams inside: GRUs, the fused TriAttention's auxiliary chain): the replayed
    output must equal the eager one on all 256 rows, twice in a row (buffers re-used across replays, counters, guard words)."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    old = cti_amd.get_precision()
    try:
        cti_amd.set_precision(prec)
        torch.manual_seed(5)
        s = bench.model_setup(config, 256, 0, torch.device(DEV))
        holder = {}

        def step():
            holder["out"] = s["fwd"]()
        with torch.no_grad():
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            eager = [t.clone() for t in (holder["out"] if isinstance(holder["out"], (tuple, list)) else (holder["out"],))]
            gr = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                with torch.cuda.graph(gr, stream=side):
                    step()
            torch.cuda.current_stream().wait_stream(side)
            static = holder["out"] if isinstance(holder["out"], (tuple, list)) else (holder["out"],)
            for _ in range(2):
                for t in static:
                    t.fill_(float("nan"))
                gr.replay()
                torch.cuda.synchronize()
                for a, b in zip(static, eager):
                    assert torch.equal(a, b), (config, prec, float((a - b).abs().max()))
    finally:
        cti_amd.set_precision(old)


def test_mc_ban_full_batch_forward_and_gradients_across_precisions():
    """The fourth model family (MC BAN, src/MC/base_model.py: BiAttention with two glimpses over question + answer tokens) at B = 256: every row of the forward in
    the plain-bf16 / bf16x3 / f16f6 modes against the exact-fp32 mode, and every parameter gradient bf16x3 against fp32 (L2 metrics)."""
    import types
    B, ntoken = 256, 20000
    ds = types.SimpleNamespace(dictionary=types.SimpleNamespace(ntoken=ntoken), v_dim=2048, num_ans_candidates=2)
    margs = types.SimpleNamespace(op="c", num_hid=1024, gamma=2, h_mm=512, rank=32, k=1, h_out=1, activation="relu", dropout=0.5, use_counter=False)
    g = torch.Generator().manual_seed(21)
    v = torch.randn(B, 36, 2048, generator=g).abs()
    nv = torch.randint(10, 37, (B,), generator=g)
    v[torch.arange(36)[None, :] >= nv[:, None]] = 0
    v = v.to(DEV)

    def toks(L):
        t = torch.randint(0, ntoken, (B, L), generator=g)
        n = torch.randint(3, L + 1, (B,), generator=g)
        t[torch.arange(L)[None, :] >= n[:, None]] = ntoken
        return t.to(DEV)
    q, a = toks(12), toks(6)
    boxes = torch.rand(B, 36, 6, generator=g).to(DEV)
    old = cti_amd.get_precision()
    outs, grads = {}, {}
    try:
        for prec in ("bf16", "bf16x3", "f16f6", "fp32"):
            cti_amd.set_precision(prec)
            torch.manual_seed(8)
            m = cti_amd.build_mc_ban(margs, ds).to(DEV).eval()
            if prec in ("bf16x3", "fp32"):
                o = m(v, boxes, q, a)[0]
                (o * torch.tensor([1.0, -0.5], device=DEV)).sum().div(B).backward()
                grads[prec] = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
                outs[prec] = o.detach().float()
            else:
                with torch.no_grad():
                    outs[prec] = m(v, boxes, q, a)[0].float()
    finally:
        cti_amd.set_precision(old)
    for prec, tol in (("bf16", 2e-2), ("bf16x3", 1e-4), ("f16f6", 1e-4)):
        per_row = (outs[prec] - outs["fp32"]).abs().flatten(1).amax(1) / outs["fp32"].abs().max()
        assert float(per_row.max()) < tol, (prec, float(per_row.max()), int(per_row.argmax()))
    flat32 = torch.cat([t.double().flatten() for t in grads["fp32"].values()])
    flatx = torch.cat([grads["bf16x3"][n].double().flatten() for n in grads["fp32"]])
    gnorm = float(flat32.norm())
    assert float((flatx - flat32).norm()) / gnorm < 2e-3
    for n, g32 in grads["fp32"].items():
        den = float(g32.double().norm())
        if den < 1e-5 * gnorm:
            continue
        e = float((grads["bf16x3"][n].double() - g32.double()).norm()) / den
        assert e < 5e-2, (n, e)


def test_full_batch_training_mode_step_agrees_across_precisions():
    """The fusion block in TRAIN mode (dropout on: the rank nets' R masks per branch, the projections' input dropout) at B = 256: with the dropout streams reset to
    the same state the masks are identical in every precision mode, so loss and every gradient of the bf16x3 step (matrix-core rank-net forward, M-build backward)
    can be held against the exact-fp32 step (fp32-MFMA rank-net kernels, VALU M-build backward) -- the train-mode kernels at the data-parallel step's shapes."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    ops = cti_amd.pkg.ops
    B = 256
    g = torch.Generator().manual_seed(12)
    v = torch.randn(B, 36, 2048, generator=g).abs_()
    for b in range(B):
        v[b, int(torch.randint(10, 37, (1,), generator=g)):] = 0
    v = v.to(DEV)
    q = torch.tanh(torch.randn(B, 12, 1024, generator=g)).to(DEV); a = torch.tanh(torch.randn(B, 3, 1024, generator=g)).to(DEV)
    y = (torch.rand(B, 3129, generator=g) > 0.999).float().to(DEV)
    crit = cti_amd.BCEWithLogitsSum()
    old = cti_amd.get_precision()
    grads, losses = {}, {}
    try:
        for prec in ("bf16x3", "fp32"):
            cti_amd.set_precision(prec)
            torch.manual_seed(4)
            ops.reset_dropout_rng()
            model = bench.CTIFusionBlock(cti_amd).to(DEV).train()
            loss = crit(model(v, q, a), y) / B
            loss.backward()
            losses[prec] = float(loss.detach())
            grads[prec] = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    finally:
        cti_amd.set_precision(old)
    assert abs(losses["bf16x3"] - losses["fp32"]) < 1e-4 * abs(losses["fp32"]), losses          # same masks: the losses agree to fp32 grade
    flat32 = torch.cat([t.double().flatten() for t in grads["fp32"].values()])
    flatx = torch.cat([grads["bf16x3"][n].double().flatten() for n in grads["fp32"]])
    gnorm = float(flat32.norm())
    assert float((flatx - flat32).norm()) / gnorm < 2e-3
    for n, g32 in grads["fp32"].items():
        den = float(g32.double().norm())
        if den < 1e-5 * gnorm:
            continue
        e = float((grads["bf16x3"][n].double() - g32.double()).norm()) / den
        assert e < 5e-2, (n, e)


@pytest.mark.parametrize("B,Tn,I,H", [(256, 12, 600, 1024), (256, 6, 300, 1024), (64, 5, 300, 512), (128, 3, 64, 1024), (256, 2, 32, 64), (192, 7, 96, 160)])
def test_persistent_gru_is_bit_identical_to_one_launch_per_step(B, Tn, I, H, precision):
    """Round 6: the plain-bf16 GRU as ONE launch whose workgroups exchange h_t through `sc1` stores / `sc1` loads and a counter per row block
    (cti_gru.hip, gru_persistent_kernel; opt-in: CTI_TUNE_GRU_PERSISTENT).  Same products in the same order, same gate arithmetic: every bit of every state equals
    the per-step launches' -- a stale or torn read of another workgroup's h would show as a difference.  Checked on an idle device, 20 times back to back, and
    while another stream streams through the L2s and takes compute units away (uneven arrival at the counters)."""
    if precision != "bf16x3":
        pytest.skip("mode set explicitly below; run once")
    lib = ops.L.lib()
    torch.manual_seed(B + Tn)
    k = 1.0 / H ** 0.5
    x = torch.randn(B, Tn, I, device=DEV)
    w_ih, w_hh = (torch.rand(3 * H, I, device=DEV) * 2 - 1) * k, (torch.rand(3 * H, H, device=DEV) * 2 - 1) * k
    b_ih, b_hh = (torch.rand(3 * H, device=DEV) * 2 - 1) * k, (torch.rand(3 * H, device=DEV) * 2 - 1) * k

    def run():
        return ops.gru_forward(x, w_ih, w_hh, b_ih, b_hh, prec="bf16")[0]
    assert lib.cti_get_tuning(ops.L.TUNE_GRU_PERSISTENT) == 0
    kssplit = run()                                                     # the default: per-step launches, K split over the waves (partial sums in another order)
    ops.L.check(lib.cti_set_tuning(ops.L.TUNE_GRU_PERSISTENT, 2), "cti_set_tuning")     # per-step launches of the ring kernel: the persistent form's accumulation order
    ref = run()
    assert float((kssplit - ref).abs().max()) < 2e-3
    ops.L.check(lib.cti_set_tuning(ops.L.TUNE_GRU_PERSISTENT, 1), "cti_set_tuning")
    try:
        outs = [run() for _ in range(20)]
        torch.cuda.synchronize()
        assert all(torch.equal(o, ref) for o in outs)
        big = torch.randn(4096, 4096, device=DEV)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(6):
                _ = big @ big                                           # other work arriving and leaving while the persistent launches run
        outs = [run() for _ in range(20)]
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert all(torch.equal(o, ref) for o in outs)
        assert not any(bool(torch.isnan(o).any()) for o in outs)
    finally:
        ops.L.check(lib.cti_set_tuning(ops.L.TUNE_GRU_PERSISTENT, 0), "cti_set_tuning")


def test_persistent_gru_under_graph_replay(precision):
    """The persistent launch and the zeroing of its counters replay from a hipGraph (the counters count up from zero every replay)."""
    if precision != "bf16x3":
        pytest.skip("run once")
    lib = ops.L.lib()
    torch.manual_seed(5)
    B, Tn, I, H = 256, 12, 600, 1024
    k = 1.0 / H ** 0.5
    x = torch.randn(B, Tn, I, device=DEV)
    w_ih, w_hh = (torch.rand(3 * H, I, device=DEV) * 2 - 1) * k, (torch.rand(3 * H, H, device=DEV) * 2 - 1) * k
    b_ih, b_hh = (torch.rand(3 * H, device=DEV) * 2 - 1) * k, (torch.rand(3 * H, device=DEV) * 2 - 1) * k
    ops.L.check(lib.cti_set_tuning(ops.L.TUNE_GRU_PERSISTENT, 2), "cti_set_tuning")
    ref = ops.gru_forward(x, w_ih, w_hh, b_ih, b_hh, prec="bf16")[0]
    ops.L.check(lib.cti_set_tuning(ops.L.TUNE_GRU_PERSISTENT, 1), "cti_set_tuning")
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                ops.gru_forward(x, w_ih, w_hh, b_ih, b_hh, prec="bf16")
            graph = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=s):
                out = ops.gru_forward(x, w_ih, w_hh, b_ih, b_hh, prec="bf16")[0]
        torch.cuda.synchronize()
        for _ in range(5):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, ref)
    finally:
        ops.L.check(lib.cti_set_tuning(ops.L.TUNE_GRU_PERSISTENT, 0), "cti_set_tuning")


@pytest.mark.parametrize("B,G,V,Q,D", [(256, 8, 36, 14, 3072), (3, 1, 1, 1, 512), (2, 8, 48, 16, 544), (5, 3, 17, 9, 1024), (4, 2, 33, 14, 2048), (2, 7, 36, 12, 992)])
@pytest.mark.parametrize("mode,tol", [("bf16x3", 2e-5), ("bf16", 1e-2)])
def test_bi_logits_without_a_barrier_in_the_k_loop(B, G, V, Q, D, mode, tol, precision):
    """Round 6: bi_logits_ks_kernel -- a sample per workgroup, an eighth of K per wave, partial outputs summed in LDS in a fixed order -- against
    float64 for full and ragged shapes (one object, one question position, a K that leaves the last waves without work, G < 8), with fp32 and bf16 rows of vt,
    in both arithmetic modes; the run-to-run bits are equal (no atomics)."""
    if precision != "bf16x3":
        pytest.skip("mode set explicitly below; run once")
    g = torch.Generator().manual_seed(B * 7 + D)
    vt = torch.randn(B, V, D, generator=g).to(DEV); qt = torch.randn(B, Q, D, generator=g).to(DEV)
    h = (torch.randn(G, D, generator=g) / 8).to(DEV); hb = torch.randn(G, generator=g).to(DEV); hs = torch.tensor([0.7], device=DEV)
    old = ops.get_precision()
    try:
        ops.set_precision(mode)
        for v in (vt, vt.to(torch.bfloat16)):
            ref = torch.einsum("bvd,gd,bqd->bgvq", v.double(), h.double(), qt.double()) * 0.7 + hb.double().view(1, G, 1, 1)
            out = ops.bi_logits(v, qt, h, hs, hb)
            assert out.shape == (B, G, V, Q)
            assert float((out.double() - ref).abs().max() / ref.abs().max()) < tol
            assert torch.equal(out, ops.bi_logits(v, qt, h, hs, hb))
    finally:
        ops.set_precision(old)


@pytest.mark.parametrize("B,Tn,I,H", [(256, 12, 600, 1024), (100, 4, 300, 1000), (3, 3, 20, 48), (65, 2, 8, 16)])
@pytest.mark.parametrize("mode,tol", [("bf16x3", 2e-5), ("bf16", 2e-2)])
def test_gru_step_with_k_split_over_the_waves(B, Tn, I, H, mode, tol, precision):
    """Round 6: gru_step_ks_kernel (eight waves, an eighth of K each, operands straight from global memory, partial tiles summed in LDS in wave order) against
    torch's nn.GRU in float64 on the CPU for full and ragged shapes (rows beyond the batch, units beyond H, K shorter than eight steps), both arithmetic modes,
    with the training path's saved gates; the same bits on every run."""
    if precision != "bf16x3":
        pytest.skip("mode set explicitly below; run once")
    torch.manual_seed(B + H)
    ref = torch.nn.GRU(I, H, 1, batch_first=True).double()
    x = torch.randn(B, Tn, I)
    with torch.no_grad():
        yr, _ = ref(x.double())
    ps = [getattr(ref, n).detach().float().to(DEV) for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    old = ops.get_precision()
    try:
        ops.set_precision(mode)
        for want_save in (False, True):
            out, save = ops.gru_forward(x.to(DEV), *ps, want_save=want_save)
            assert float((out.double().cpu() - yr).abs().max()) < tol * max(1.0, float(yr.abs().max()))
            out2, save2 = ops.gru_forward(x.to(DEV), *ps, want_save=want_save)
            assert torch.equal(out, out2)
            if want_save:
                assert torch.equal(save, save2) and torch.equal(save[:, :, 4, :].transpose(0, 1), out)
    finally:
        ops.set_precision(old)


@pytest.mark.parametrize("B,Tn,dim,H,concat", [(256, 12, 300, 1024, True), (64, 6, 300, 512, False), (3, 5, 20, 48, True)])
def test_bf16_word_vectors_straight_into_the_gru(B, Tn, dim, H, concat, precision):
    """Round 6 (a first step): in the plain-bf16 mode the word embedding writes bf16 rows (pitch = width rounded up to 32, zeros beyond) and the GRU's
    input-side product reads them as they stand -- no fp32 word vectors, no split pass.  The same bf16 operands as the fp32-vectors path (the split pass rounds the same
    values to the same bf16), padding token rows included; outside the plain-bf16 mode the rows are widened and the result is the fp32 path's."""
    if precision != "bf16x3":
        pytest.skip("mode set explicitly below; run once")
    torch.manual_seed(B + dim)
    ntoken = 500
    emb = cti_amd.WordEmbedding(ntoken, dim, 0.0, op='c' if concat else '').to(DEV).eval()
    gru = cti_amd.QuestionEmbedding((2 if concat else 1) * dim, H, 1, False, 0.0).to(DEV).eval()
    with torch.no_grad():
        emb.emb.weight.normal_(); emb.emb.weight[ntoken].zero_()
        if concat:
            emb.emb_.weight.normal_(); emb.emb_.weight[ntoken].zero_()
    tok = torch.randint(0, ntoken + 1, (B, Tn), device=DEV)
    old = ops.get_precision()
    try:
        ops.set_precision("bf16")
        with torch.no_grad():
            rows = emb.rows16(tok)
            assert rows.dtype == torch.bfloat16 and rows.shape == (B, Tn, ((2 if concat else 1) * dim + 31) // 32 * 32)
            x32 = emb(tok)
            assert torch.equal(rows[:, :, :x32.shape[2]].float(), x32.to(torch.bfloat16).float())
            assert float(rows[:, :, x32.shape[2]:].float().abs().max() if rows.shape[2] > x32.shape[2] else 0.0) == 0.0
            a = gru.forward_all(rows)
            b = gru.forward_all(x32)
            # the same bf16 operands either way; at the model shape both input-side products run on the same kernel (every bit equal), at small shapes the fp32
            # path's product is the skinny kernel (another summation order: fp32 rounding, amplified by the recurrence's bf16 roundings of h)
            if B * Tn >= 1024:
                assert torch.equal(a, b)
            assert float((a - b).abs().max()) < 2e-3
        ops.set_precision("bf16x3")
        with torch.no_grad():
            assert emb.rows16(tok).dtype == torch.float32                      # not this mode's operand: the fp32 vectors
            c = gru.forward_all(rows)                                           # bf16 rows handed in anyway are widened
            d = gru.forward_all(rows[:, :, :x32.shape[2]].float().contiguous())
            assert torch.equal(c, d)
    finally:
        ops.set_precision(old)
