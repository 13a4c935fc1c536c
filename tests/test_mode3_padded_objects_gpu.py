"""The f16f6 mode-3 product skips the row tiles of a sample's zero-padded objects and a copy kernel fills them (csrc/cti_mode3_plan.hip, cti_set_tuning key
CTI_TUNE_MODE3_SKIP_PADDED).  The output must be what the product computes when it walks every tile (key 0) -- bit for bit: the filled rows are copies of rows
the same instruction sequence computed from bit-identical operands -- and the float64 oracle's within the f16f6 tolerance; every case also checks the plan's
totals against a host computation from the mask, so that a silently disabled path fails.  Needs an MI355X; the CPU half is tests/test_mode3_padded_objects_cpu.py."""
import numpy as np
import pytest
import torch

import cti_amd
from oracle import cti_oracle as O
from mode3_plan_host import BM, BN, host_plan, zero_object_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4                   # the project's bound for this arithmetic mode (bench.py MODEL_TOL["f16f6"]) against the float64 oracle
ops = cti_amd.ops
V, Q, G, H, R = 36, 14, 2, 512, 32          # V * Q * G = 1008 rows per sample: four row tiles of 256; an object is 28 rows, so object 9 straddles the first boundary
VD, QD, AD = 64, 48, 32


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def sd(m):
    return {k: t.detach().cpu().numpy().copy() for k, t in m.state_dict().items()}


@pytest.fixture(autouse=True)
def f16f6_mode():
    old, old_keep = cti_amd.get_precision(), ops._debug_keep_mode3_plan
    cti_amd.set_precision("f16f6")
    ops._debug_keep_mode3_plan = True
    ops._range_log.update(consecutive=0, skip=0); ops._range_owner.clear()
    yield
    ops._debug_keep_mode3_plan = old_keep
    cti_amd.set_precision(old)
    cti_amd.set_range_check("sync"); ops.set_poison_bits(23)
    ops._range_log.update(consecutive=0, skip=0); ops._range_owner.clear()


_nets = {}


def net_for(v_dim=VD, q_dim=QD, a_dim=AD, h=H, rank=R):
    key = (v_dim, q_dim, a_dim, h, rank)
    if key not in _nets:
        torch.manual_seed(1204)
        _nets[key] = cti_amd.TCNet(v_dim, q_dim, a_dim, h, 1, rank, G).to(DEV).eval()
    return _nets[key]


def inputs(B, A, seed, n_objs=V, n_q=Q, v_dim=VD, q_dim=QD, a_dim=AD):
    rs = np.random.RandomState(seed)
    v = np.abs(rs.standard_normal((B, n_objs, v_dim))).astype(np.float32) + np.float32(0.01)       # (no object is zero by accident)
    q = rs.standard_normal((B, n_q, q_dim)).astype(np.float32)
    a = rs.standard_normal((B, A, a_dim)).astype(np.float32)
    return v, q, a


def run(net, v, q, a, key):
    with ops.tuning(mode3_skip_padded=key), torch.no_grad():
        out = net(T(v), T(q), T(a))
        torch.cuda.synchronize()
        return out.cpu().numpy(), ops.last_mode3_plan()


def check_case(v, q, a, what, net=None, oracle=True):
    net = net or net_for()
    B, n_objs, A = v.shape[0], v.shape[1], a.shape[1]
    on, plan = run(net, v, q, a, 1)
    off, plan_off = run(net, v, q, a, 0)
    want = host_plan(zero_object_mask(v), q.shape[1], G, A)
    print("%s: plan %s (host %s); max |out| %.3g" % (what, plan, want, float(np.nanmax(np.abs(off)))))
    assert plan_off is None, what                                # key 0: no plan is built
    assert plan is not None, what + ": the call built no tile plan"
    assert plan == dict(want, samples=B), what
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32)), "%s: %d entries differ between the skipping walk and the full walk" % (
        what, int(np.sum(on.view(np.uint32) != off.view(np.uint32))))
    if oracle:
        ref = O.tcnet_forward(v, q, a, sd(net), dtype=np.float64)
        err = O.norm_max_err(on, ref)
        print("%s: normalised max error vs float64 %.3g" % (what, err))
        assert err < TOL, what
    return on, plan


@pytest.mark.parametrize("A", [384, 301])        # two whole column tiles of 192; a ragged last column tile with an odd last column
def test_no_zero_object_walks_every_tile(A):
    v, q, a = inputs(2, A, 1)
    _, plan = check_case(v, q, a, "no zero object, A=%d" % A)
    assert plan["live_row_tiles"] == 2 * 4 and plan["filled_rows"] == 0


def test_all_objects_zero():
    v, q, a = inputs(2, 301, 2)
    v[1] = 0
    out, plan = check_case(v, q, a, "all objects of sample 1 zero")
    assert plan["live_row_tiles"] == 4 + 1 and plan["filled_rows"] == 1008 - 256
    assert np.abs(out[1]).max() > 0                              # relu(bias) through the rank nets: padded objects' rows are not zero


@pytest.mark.parametrize("n_rep", [8, 9, 10, 18, 27, 35])
def test_trailing_run_of_zero_objects(n_rep):
    """The representative (object n_rep) in the first row tile (8), straddling its boundary (9: rows 252 .. 279), behind it (10), straddling the second (18) and the
    third boundary (27), and as the last object (35: nothing to fill)."""
    v, q, a = inputs(2, 301, 10 + n_rep)
    v[0, n_rep:] = 0
    v[1, n_rep:] = 0
    v[1, 3] = 0                                                  # ... and an interior zero object in front of it
    out, plan = check_case(v, q, a, "n_rep=%d" % n_rep)
    live = -(-(n_rep + 1) * Q * G // BM)
    assert plan["live_row_tiles"] == 2 * live
    for v_ in range(n_rep + 1, V):                               # every padded object's block equals the representative's
        assert np.array_equal(out[0, v_], out[0, n_rep])


def test_interior_zero_object_followed_by_live_ones_is_not_skipped():
    v, q, a = inputs(2, 384, 3)
    v[0, 20] = 0
    v[1, 5:30] = 0
    _, plan = check_case(v, q, a, "interior zero objects")
    assert plan["live_row_tiles"] == 8 and plan["filled_rows"] == 0


def test_padded_row_holding_minus_zero_is_padding():
    v, q, a = inputs(2, 301, 4)
    v[:, 12:] = 0
    v[0, 20, 7] = -0.0
    v[1, 12:, ::3] = -0.0
    _, plan = check_case(v, q, a, "-0.0 in padded rows")
    assert plan["live_row_tiles"] == 2 * 2


def test_padded_row_holding_a_nan_is_live():
    """A NaN in an otherwise zero row: the object is not padding (the mask is the bit-exact magnitude OR), so its tiles are walked and its NaN rows are computed, not
    copied over.  'sync' (the default): the guard sees the non-finite operand and the call is re-run in fp32, skipping or not -- the NaNs sit where the oracle puts
    them.  Without the host wait and with the NaN fill off, the f16f6 kernels' own output and the plan are compared."""
    v, q, a = inputs(2, 301, 5)
    v[:, 12:] = 0
    v[0, 30, 5] = np.nan
    net = net_for()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        on, _ = run(net, v, q, a, 1)
        ops._range_log.update(consecutive=0, skip=0); ops._range_owner.clear()
        off, _ = run(net, v, q, a, 0)
        ops._range_log.update(consecutive=0, skip=0); ops._range_owner.clear()
    ref = O.tcnet_forward(v, q, a, sd(net), dtype=np.float64)
    assert np.isnan(ref[0, 30]).all() and np.isfinite(ref[0, :30]).all() and np.isfinite(ref[0, 31:]).all()
    assert np.array_equal(on, off, equal_nan=True)
    assert O.norm_max_err(on, ref) < TOL
    cti_amd.set_range_check("poison"); ops.set_poison_bits(0)
    on, plan = run(net, v, q, a, 1)
    off, _ = run(net, v, q, a, 0)
    want = host_plan(zero_object_mask(v), Q, G, 301)
    print("NaN row: plan %s (host %s)" % (plan, want))
    assert plan == dict(want, samples=2)
    assert plan["live_row_tiles"] == 4 + 2                       # sample 0: objects 0 .. 30 and one padded object = 32 objects = 896 rows; sample 1: 13 objects
    assert np.array_equal(np.isnan(on), np.isnan(off))
    assert np.array_equal(on, off, equal_nan=True)


def test_samples_of_all_kinds_in_one_batch():
    v, q, a = inputs(9, 301, 6)
    v[1] = 0
    for b, n_rep in ((2, 8), (3, 9), (4, 18), (5, 27)):
        v[b, n_rep:] = 0
    v[6, 17] = 0
    v[7, 10:] = 0; v[7, 11, 3] = -0.0
    v[8, 1:] = 0
    _, plan = check_case(v, q, a, "mixed batch")
    assert plan["live_row_tiles"] == 4 + 1 + 1 + 2 + 3 + 4 + 4 + 2 + 1


def test_more_than_256_samples_cross_the_plan_kernels_chunks():
    """The plan kernel takes the samples in chunks of 256 and carries the row-tile count across them: B = 300 with every length of the trailing run.  (No oracle
    leg: the float64 restatement of 300 samples at these widths needs gigabytes; the cases above have it.)"""
    B = 300
    v, q, a = inputs(B, 193, 12)
    rs = np.random.RandomState(13)
    for b in range(B):
        v[b, int(rs.randint(0, V + 1)):] = 0
    _, plan = check_case(v, q, a, "B=300", oracle=False)
    assert plan["filled_rows"] > 0 and plan["live_row_tiles"] < 4 * B


def test_shape_that_takes_the_scalar_fill():
    """Q * A * G = 630 floats per object: not a multiple of four, so the fill copies float by float."""
    net = net_for(40, 32, 24, 512, 32)
    v, q, a = inputs(3, 45, 7, n_objs=40, n_q=7, v_dim=40, q_dim=32, a_dim=24)
    v[0, 5:] = 0
    v[2, 30:] = 0
    on, plan = run(net, v, q, a, 1)
    off, _ = run(net, v, q, a, 0)
    want = host_plan(zero_object_mask(v), 7, G, 45)
    assert plan == dict(want, samples=3) and plan["filled_rows"] > 0
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32))
    assert O.norm_max_err(on, O.tcnet_forward(v, q, a, sd(net), dtype=np.float64)) < TOL


def test_no_auxiliary_stream_and_unwritten_workspace():
    """Mask and plan run in line on the one stream, and both are written before they are read: a workspace pre-filled with 0xFF changes nothing."""
    v, q, a = inputs(2, 301, 8)
    v[0, 9:] = 0
    net = net_for()
    ref, _ = run(net, v, q, a, 0)
    old_aux, old_fill = ops.use_aux_stream, ops._debug_ws_fill
    try:
        ops.use_aux_stream = False
        ops._debug_ws_fill = 0xFF
        tucker, rank = net._fused_args()
        with ops.tuning(mode3_skip_padded=1), torch.no_grad():
            out = ops.tcnet_forward(T(v), T(q), T(a), tucker, rank, net.T_g.detach(), prepared=None)      # no zero_mask from the caller: the workspace's own
            torch.cuda.synchronize()
            plan = ops.last_mode3_plan()
            out_m, mask = ops.tcnet_forward(T(v), T(q), T(a), tucker, rank, net.T_g.detach(), prepared=None, want_mask=True)
            torch.cuda.synchronize()
            plan_m = ops.last_mode3_plan()
    finally:
        ops.use_aux_stream, ops._debug_ws_fill = old_aux, old_fill
    want = dict(host_plan(zero_object_mask(v), Q, G, 301), samples=2)
    assert plan == want and plan_m == want
    assert np.array_equal(mask.cpu().numpy().astype(bool), zero_object_mask(v))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(out_m.cpu().numpy().view(np.uint32), ref.view(np.uint32))


def test_graph_replay_follows_the_padding_it_finds():
    """The plan is rebuilt on the device in every call: a captured forward replayed with ANOTHER padding pattern in its static `v` walks that pattern's tiles."""
    net = net_for()
    v, q, a = inputs(3, 301, 9)
    v1 = v.copy(); v1[0, 30:] = 0
    v2 = v.copy(); v2[0, 9:] = 0; v2[1] = 0; v2[2, 20:] = 0
    eager1, _ = run(net, v1, q, a, 0)
    eager2, _ = run(net, v2, q, a, 0)
    want1 = dict(host_plan(zero_object_mask(v1), Q, G, 301), samples=3)
    want2 = dict(host_plan(zero_object_mask(v2), Q, G, 301), samples=3)
    assert want1 != want2
    tv, tq, ta = T(v1), T(q), T(a)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with ops.tuning(mode3_skip_padded=1):
        with torch.cuda.stream(s), torch.no_grad():
            net(tv, tq, ta)                                      # eager warm-up on the capture stream
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s), torch.no_grad():
            with torch.cuda.graph(gr, stream=s):
                o = net(tv, tq, ta)
        torch.cuda.current_stream().wait_stream(s)
        gr.replay()
        torch.cuda.synchronize()
        plan1 = ops.last_mode3_plan()                            # (a view of the captured call's workspace: it reads what the last replay left)
        out1 = o.cpu().numpy()
        tv.copy_(T(v2))
        gr.replay()
        torch.cuda.synchronize()
        plan2 = ops.last_mode3_plan()
        out2 = o.cpu().numpy()
    print("replays: plans %s, %s (host %s, %s)" % (plan1, plan2, want1, want2))
    assert plan1 == want1 and plan2 == want2
    assert np.array_equal(out1.view(np.uint32), eager1.view(np.uint32))
    assert np.array_equal(out2.view(np.uint32), eager2.view(np.uint32))


def test_full_configs1_shape_on_off_equal_and_live_tiles():
    """BASELINE configs[1] with the benchmark's own seeded inputs (rank 0: SEED + 1): the whole 3.2 GB output equal bit for bit between the two walks, compared on the
    device in slices; 798 of 1 024 row tiles are live = 13 566 tiles."""
    import bench
    c = bench.C2
    torch.manual_seed(bench.SEED)
    net = cti_amd.TCNet(c["v_dim"], c["q_dim"], c["a_dim"], c["h_mm"], 1, c["rank"], c["glimpse"]).to(DEV).eval()
    v, q, a = bench.synth_inputs(c, c["B"], bench.SEED + 1, DEV)
    want = host_plan(zero_object_mask(v.cpu().numpy()), c["Q"], c["glimpse"], c["A"])
    assert want["live_row_tiles"] == 798 and want["live_tiles"] == 13566
    with torch.no_grad():
        with ops.tuning(mode3_skip_padded=0):
            off = net(v, q, a)
            torch.cuda.synchronize()
            assert ops.last_mode3_plan() is None
        with ops.tuning(mode3_skip_padded=1):
            on = net(v, q, a)
            torch.cuda.synchronize()
            plan = ops.last_mode3_plan()
    print("configs[1]: plan %s" % plan)
    assert plan == dict(want, samples=c["B"])
    assert bool(torch.isfinite(on[0]).all())
    differing = 0
    for b0 in range(0, c["B"], 16):
        differing += int((on[b0:b0 + 16].view(torch.int32) != off[b0:b0 + 16].view(torch.int32)).sum())
    assert differing == 0, "%d entries differ between the skipping walk and the full walk" % differing
