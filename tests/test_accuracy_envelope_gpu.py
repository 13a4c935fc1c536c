"""Accuracy envelope of the f16f6 default INSIDE its range (the reference multiplies in fp32, src/Tensor.py:12-20): the product's error is
~2^-17 sum_k |M_k A^_k| per output, i.e. 1e-4 of the LARGEST output only while the mode-3 contraction does not cancel too heavily.  At the BASELINE
configs[1] WIDTHS against the float64 oracle: (a) T_g with a common offset, (b) an operand pair built to cancel (max |out| << sum |M| |A^|),
(c) a trained-like state (weight gains x3, biases x10, half the ReLUs dead) -- each either within 1e-4 as it stands or tripped by the guard's
cancellation estimate and re-run in a mode that is.  Needs an MI355X."""
import warnings

import numpy as np
import pytest
import torch

import cti_amd
import golden_util as gu
from oracle import cti_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
ops = cti_amd.ops
RHO_BF16X3, RHO_FP32 = 2.75, 5.5         # the library's default thresholds (cti_set_tuning keys 3 / 4)


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(autouse=True)
def f16f6_mode():
    old = cti_amd.get_precision()
    cti_amd.set_precision("f16f6")
    ops._range_log.update(consecutive=0, skip=0); ops._range_owner.clear()
    ops._range_debug = True
    yield
    ops._range_debug = False
    cti_amd.set_precision(old)
    cti_amd.set_range_check("sync")
    ops._range_log.update(consecutive=0, skip=0); ops._range_owner.clear()


def _case(A=640, B=2):
    fx, params, v, q, a, _ = gu.c2_case()
    return {k[len("TriAtt."):]: np.asarray(x).copy() for k, x in params.items() if k.startswith("TriAtt.")}, v[:B].copy(), q[:B].copy(), a[:B, :A].copy()


def _run(sd, v, q, a):
    c = gu.load("g3_tcnet_forward_c2").cfg
    m = cti_amd.TCNet(c["v_dim"], c["q_dim"], c["a_dim"], c["h_dim"], 1, c["rank"], c["glimpse"])
    m.load_state_dict({k: torch.from_numpy(x) for k, x in sd.items()})
    m = m.to(DEV).eval()
    ops._range_log.update(consecutive=0, skip=0); ops._range_owner.clear()     # (no repeat-offender shortcut across the cases of a sweep: every call is judged afresh)
    before = ops.f16f6_range_status()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.no_grad():
            out = m(T(v), T(q), T(a)).cpu().numpy()
    after = ops.f16f6_range_status()
    ref = O.tcnet_forward(v, q, a, sd, dtype=np.float64)
    err = float(np.max(np.abs(out - ref)) / np.max(np.abs(ref)))
    return err, after["trips"] - before["trips"], after["last_status"], after["last_ratio"]


def test_synthetic_inputs_sit_well_inside_the_envelope():
    sd, v, q, a = _case()
    err, trips, status, rho = _run(sd, v, q, a)
    print("benign: err %.2e rho %.1f" % (err, rho))
    assert trips == 0 and status == 0 and err < TOL
    assert 0.5 < rho < 0.7 * RHO_BF16X3                       # the trip threshold keeps a margin over the benign estimate


def test_core_tensor_with_a_common_offset():
    """(a) T_g + 8: every M entry carries a large common part; A^ >= 0 (ReLU), so the sum does not cancel -- the outputs grow with it"""
    sd, v, q, a = _case()
    sd["T_g"] = sd["T_g"] + 8.0
    err, trips, status, rho = _run(sd, v, q, a)
    print("T_g + 8: err %.2e rho %.1f trips %d status %d" % (err, rho, trips, status))
    assert err < TOL


def test_trained_like_state():
    """(c) weight gains x3, biases x10 with a negative shift that kills about half of the ReLUs"""
    sd, v, q, a = _case()
    rs = np.random.RandomState(3)
    for k in list(sd):
        if k.endswith("weight_g"):
            sd[k] = np.asarray(sd[k] * 3.0, dtype=np.float32)
        elif k.endswith("bias"):
            sd[k] = (sd[k] * 10.0 - 0.5 * np.abs(rs.standard_normal(sd[k].shape))).astype(np.float32)
    err, trips, status, rho = _run(sd, v, q, a)
    print("trained-like: err %.2e rho %.1f trips %d status %d" % (err, rho, trips, status))
    assert err < TOL


def _cancelling(sd, eps, pair_columns=None):
    """A^ (nearly) orthogonal to every row of M: the answer side's rank-net outputs come in equal pairs (k, k ^ 1), T_eff's matching k slices in opposite
    pairs, plus eps of the original signal.  pair_columns: pair the rank nets' weights on these input features only (the localised case below)."""
    R = 32
    hr = sd["T_g"].shape[2]
    for r in range(R):
        w = sd["a_net.%d.main.1.weight_v" % r]
        if pair_columns is None:
            w[1::2] = w[0::2]
        else:
            w[1::2, pair_columns] = w[0::2, pair_columns]
        b = sd["a_net.%d.main.1.bias" % r]
        b[1::2] = b[0::2]
    G = sd["T_g"].shape[5]
    imap = O.teff_index_map(hr, G).reshape(-1)
    Tg = sd["T_g"].copy()
    for r in range(R):
        flat = Tg[0, r, :, :, :, :, 0].reshape(-1)
        eff = flat[imap].reshape(hr, hr, hr, G)
        can = eff.copy()
        can[:, :, 1::2, :] = -can[:, :, 0::2, :]
        new = (can + eps * eff).reshape(-1)
        out_flat = np.empty_like(flat)
        out_flat[imap] = new
        Tg[0, r, :, :, :, :, 0] = out_flat.reshape(hr, hr, hr, G)
    sd["T_g"] = Tg.astype(np.float32)


def test_the_thresholds_keep_a_factor_two_under_the_tolerance():
    """round 4's thresholds (10 / 20) left no margin -- rho 9.0 measured 9.0e-5.  Sweep the cancelling construction through both
    thresholds' neighbourhoods: whatever the guard lets through as f16f6 (no trip) stays under HALF the tolerance, and so does what it re-runs as bf16x3."""
    worst = {0: 0.0, 8: 0.0, 24: 0.0}
    rows = []
    for eps in (1.0, 0.8, 0.7, 0.6, 0.5, 0.45, 0.4, 0.35, 0.3, 0.25, 0.2, 0.16, 0.13, 0.1):
        sd, v, q, a = _case()
        _cancelling(sd, eps)
        err, trips, status, rho = _run(sd, v, q, a)
        print("threshold sweep eps=%g: err %.2e rho %.2f trips %d status %d" % (eps, err, rho, trips, status))
        rows.append((eps, err, rho, trips, status))
        worst[status & 24] = max(worst[status & 24], err)
    for eps, err, rho, trips, status in rows:
        assert (status & 24) in (0, 8, 24)
        assert (rho > RHO_BF16X3) == bool(status & 8) and (rho > RHO_FP32) == bool(status & 16), (eps, rho, status)
        assert trips == (1 if status else 0)
    assert worst[0] < 0.5 * TOL and worst[8] < 0.5 * TOL and worst[24] < 0.5 * TOL, worst


def test_cancellation_confined_to_eight_answer_tokens_still_trips():
    """32 evenly spaced rows of A^ out of 3 129 cannot see a cancellation that lives in a few answer tokens.  Construction: input coordinate 0 is
    a switch (+20 on 8 "hot" tokens, -20 on the other 3 121) that the Tucker layer turns into disjoint active feature sets -- features 0 .. 255 live on hot
    tokens only, 256 .. 511 on ordinary ones (the wrong half sits ~4 sigma below the ReLU) --, and the rank nets' weights are paired (k, k ^ 1) on the hot
    features only.  With the core's k slices in opposite pairs the HOT tokens' outputs cancel to eps of their signal while the ordinary tokens' do not: max |out|
    is set by ordinary tokens, sum |M| |A^| by the hot ones (their Tucker gain on the switch is 6 x the ordinary tokens': A^ rows ~6 x larger).  Evenly spaced sampling (the round-4 estimate, behind CTI_TUNE_GUARD_STRATA = 0) reads
    an ordinary rho and lets an f16f6 result through whose error on the hot tokens exceeds the tolerance; the strata maxima put the hot tokens into the sample,
    the estimate trips and the re-run is within tolerance."""
    sd, v, q, a = _case(A=3129, B=1)
    hot_f, ord_f = np.arange(0, 256), np.arange(256, 512)
    Wt = sd["a_tucker.main.1.weight_v"]
    Wt[hot_f, 0], Wt[ord_f, 0] = 3.0, -0.5                                # (asymmetric gains: the hot tokens' Tucker features -- and their A^ rows -- come out ~6 x larger)
    _cancelling(sd, 0.02, pair_columns=hot_f)
    rs = np.random.RandomState(5)
    hot = np.sort(rs.choice(3129, size=8, replace=False))
    a = a.copy()
    a[:, :, 0] = -20.0
    a[:, hot, 0] = 20.0
    ref = O.tcnet_forward(v, q, a, sd, dtype=np.float64)
    big = float(np.max(np.abs(ref)))
    print("localised: max |out| %.3g, of which hot tokens %.3g" % (big, float(np.max(np.abs(ref[:, :, :, hot])))))
    assert float(np.max(np.abs(ref[:, :, :, hot]))) < 0.5 * big            # the hot tokens do cancel: they do not set the scale
    lib = cti_amd.pkg._lib.lib()
    L = cti_amd.pkg._lib
    # (1) round 4's sampling: nothing trips, and the f16f6 result it lets through is out of tolerance on the hot tokens
    lib.cti_set_tuning(L.TUNE_GUARD_STRATA, 0)
    try:
        err_even, trips_even, status_even, rho_even = _run(sd, v, q, a)
    finally:
        lib.cti_set_tuning(L.TUNE_GUARD_STRATA, 1)
    # (2) strata maxima
    err, trips, status, rho = _run(sd, v, q, a)
    print("localised: evenly spaced rows only: rho %.2f status %d err %.2e | with strata maxima: rho %.2f status %d trips %d err %.2e"
          % (rho_even, status_even, err_even, rho, status, trips, err))
    assert rho > RHO_BF16X3 and (status & 8) and trips == 1 and err < TOL
    assert rho > 1.5 * rho_even


def _module(sd):
    c = gu.load("g3_tcnet_forward_c2").cfg
    m = cti_amd.TCNet(c["v_dim"], c["q_dim"], c["a_dim"], c["h_dim"], 1, c["rank"], c["glimpse"])
    m.load_state_dict({k: torch.from_numpy(x) for k, x in sd.items()})
    return m.to(DEV).eval()


def test_poison_mode_keeps_only_a_mildly_cancelling_result():
    """with no host to re-run it (range check 'poison', hipGraph capture) a call that trips ONLY the mild cancellation bit (2.75 < rho <= 5.5)
    keeps its f16f6 result -- finite and, by the measured law ~1.8e-5 rho, still within 1e-4 -- and the device status word says so; beyond the heavy threshold
    rho has no upper bound, so bit 16 NaN-fills like the range bits do (default mask 23)."""
    sd, v, q, a = _case()
    _cancelling(sd, 0.35)
    cti_amd.set_range_check("poison")
    m = _module(sd)
    with torch.no_grad():
        out = m(T(v), T(q), T(a))
    st = ops.f16f6_device_status()
    ref = O.tcnet_forward(v, q, a, sd, dtype=np.float64)
    err = float(np.max(np.abs(out.cpu().numpy() - ref)) / np.max(np.abs(ref)))
    print("poison mode, cancelling eps=0.35: status %d rho %.1f err %.2e" % (st["status"], st["rho"], err))
    assert bool(torch.isfinite(out).all()) and st["status"] == 8 and RHO_BF16X3 < st["rho"] <= RHO_FP32 and err < TOL
    sd2, _, _, _ = _case()
    _cancelling(sd2, 0.13)                                     # rho ~ 11: bits 8 + 16
    m2 = _module(sd2)
    with torch.no_grad():
        out2 = m2(T(v), T(q), T(a))
    st2 = ops.f16f6_device_status()
    assert (st2["status"] & 24) == 24 and bool(torch.isnan(out2).all())
    ops.set_poison_bits(7)                                      # the range bits only: the heavy case keeps its (inaccurate) numbers -- a caller's explicit choice
    try:
        with torch.no_grad():
            out3 = m2(T(v), T(q), T(a))
        assert bool(torch.isfinite(out3).all())
    finally:
        ops.set_poison_bits(23)


@pytest.mark.parametrize("eps,bits", [(1.0, 0), (0.35, 8), (0.13, 24)])
def test_graph_replay_with_the_safety_net(eps, bits):
    """VERDICT r5 #7a: cti_amd.GraphedForward replays the captured forward, reads the status word that replay left on the device and re-runs a tripped call
    eagerly in the mode the verdict asks for -- so the cancelling construction that a bare replay would return as NaN (eps 0.13) or at ~1e-4 (eps 0.35) comes
    back fp32-grade; an untripped call is the replay's own output; twenty replays, every one checked; and a batch with an overflowing operand (range bit)."""
    sd, v, q, a = _case()
    if eps < 1.0:
        _cancelling(sd, eps)
    m = _module(sd)
    tv, tq, ta = T(v), T(q), T(a)
    g = cti_amd.GraphedForward(lambda x, y, z: m(x, y, z), (tv, tq, ta))
    ref = O.tcnet_forward(v, q, a, sd, dtype=np.float64)
    for rep in range(20):
        out = g(tv, tq, ta)
        err = float(np.max(np.abs(out.cpu().numpy() - ref)) / np.max(np.abs(ref)))
        assert err < TOL and g.last_status == bits and g.reruns == (rep + 1 if bits else 0), (rep, err, g.last_status, g.reruns)
    print("graph replay + safety net, eps=%g: status %d, %d re-runs, err %.2e" % (eps, g.last_status, g.reruns, err))
    a_big = a.copy(); a_big[0, 3, :] = 3e5                      # an answer token beyond the f16 range: saturation bit -> NaN from the replay -> bf16x3 eagerly
    before = g.reruns
    out = g(tv, tq, T(a_big))
    ref_big = O.tcnet_forward(v, q, a_big, sd, dtype=np.float64)
    err = float(np.max(np.abs(out.cpu().numpy() - ref_big)) / np.max(np.abs(ref_big)))
    assert (g.last_status & 7) and g.reruns == before + 1 and bool(torch.isfinite(out).all()) and err < TOL, (g.last_status, err)


@pytest.mark.parametrize("eps,bits", [(1.0, 0), (0.35, 8), (0.13, 24)])
def test_graph_safety_net_in_a_fresh_process(eps, bits):
    """The same three rows, each ALONE in a child process, so that GraphedForward is the first thing in the process to meet the guard, under the default
    'sync' range check: its warm-up forwards are waited for by the host and leave no status block behind, and a block cannot be born under capture -- the
    wrapper has to create it itself, or every replay comes back with last_status 0 and the NaN / ~1e-4 output of the bare graph (in this file's order the
    poison-mode test above creates the block first, which hid that).  Children run one after another; the node id selects the row (no -k: its
    expression parser trips over the dots, and would collect this launcher again)."""
    import os, subprocess, sys
    node = "%s::test_graph_replay_with_the_safety_net[%s-%d]" % (os.path.abspath(__file__), eps, bits)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", node], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:]


@pytest.mark.parametrize("first_cancels", [True, False])
def test_graph_with_two_guarded_calls_reports_the_first(first_cancels):
    """One captured forward with TWO guarded f16f6 calls, one of them built to cancel heavily (eps 0.13: bits 8 + 16, NaN-filled by the replay), the other
    untouched: every guarded call of the capture leaves its status word in a slot of its own and the wrapper ORs them, so the verdict of the FIRST call
    survives the second one's clean word (and the other way round); the eager re-run brings both outputs back within tolerance of their own float64 oracle."""
    sd_c, v, q, a = _case()
    _cancelling(sd_c, 0.13)
    sd_p, _, _, _ = _case()
    sds = (sd_c, sd_p) if first_cancels else (sd_p, sd_c)
    nets = [_module(sd) for sd in sds]
    refs = [O.tcnet_forward(v, q, a, sd, dtype=np.float64) for sd in sds]
    tv, tq, ta = T(v), T(q), T(a)
    g = cti_amd.GraphedForward(lambda x, y, z: (nets[0](x, y, z), nets[1](x, y, z)), (tv, tq, ta))
    for rep in range(3):
        outs = g(tv, tq, ta)
        errs = [float(np.max(np.abs(o.cpu().numpy() - r)) / np.max(np.abs(r))) for o, r in zip(outs, refs)]
        print("two guarded calls (first cancels: %s), replay %d: status %d, %d re-runs, errs %.2e %.2e" % (first_cancels, rep, g.last_status, g.reruns, errs[0], errs[1]))
        assert g.reruns == rep + 1 and (g.last_status & 24) == 24, (rep, g.reruns, g.last_status)
        assert max(errs) < TOL, errs
    assert (ops.f16f6_device_status()["status"] & 24) == (0 if first_cancels else 24)      # (f16f6_device_status() keeps returning the LAST call's word)


def test_bare_captures_after_a_graphed_forward_take_no_status_slots():
    """The status slots belong to the capture GraphedForward opens and closes: a bare torch.cuda.graph capture of a guarded forward (tests/test_range_guard_gpu.py,
    bench.py) writes the 256-byte copy only, as it always did -- so any number of them can follow a GraphedForward in one process (twenty here, more than
    ops.GUARD_SLOTS), each replay leaves its own verdict where f16f6_device_status() reads it, and the GraphedForward captured first still reports its own."""
    sd, v, q, a = _case()
    m = _module(sd)
    tv, tq, ta = T(v), T(q), T(a)
    g = cti_amd.GraphedForward(lambda x, y, z: m(x, y, z), (tv, tq, ta))
    clean = g(tv, tq, ta).clone()
    assert g.last_status == 0 and g.reruns == 0 and g._nslots == 1
    assert not ops._guard_capture_slots                         # closed with the capture
    big = T(a * np.float32(1e6))                               # beyond the f16 range: saturation bit, NaN fill
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        m(tv, tq, ta)                                           # eager warm-up on the capture stream
    torch.cuda.synchronize()
    for i in range(ops.GUARD_SLOTS + 4):
        gr = torch.cuda.CUDAGraph()
        xa = ta.clone()
        with torch.cuda.stream(s), torch.no_grad():
            with torch.cuda.graph(gr, stream=s):
                o = m(tv, tq, xa)
        torch.cuda.current_stream().wait_stream(s)
        gr.replay()
        assert ops.f16f6_device_status()["status"] == 0 and torch.equal(o, clean), i
        xa.copy_(big)
        gr.replay()
        assert (ops.f16f6_device_status()["status"] & 7) and bool(torch.isnan(o).all()), i
    assert not ops._guard_capture_slots
    out = g(tv, tq, ta)
    assert g.last_status == 0 and g.reruns == 0 and torch.equal(out, clean)
    out = g(tv, tq, big)
    assert (g.last_status & 7) and g.reruns == 1 and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("eps,expect", [(1.0, 0), (0.7, 0), (0.45, 8), (0.35, 8), (0.2, 24), (0.05, 24), (0.004, 24)])
def test_cancelling_contraction_trips_the_estimate_and_is_rerun(eps, expect):
    """(b) the rank nets' LAST layer of the answer side built so that A^ is (nearly) orthogonal to every row of M: columns come in equal pairs and
    T_g's matching k slices in opposite pairs, plus eps of the original signal.  max |out| shrinks with eps while sum |M| |A^| stays: the estimate
    must trip (bf16x3 at moderate, exact fp32 at heavy cancellation) before the error passes 1e-4."""
    sd, v, q, a = _case()
    _cancelling(sd, eps)
    err, trips, status, rho = _run(sd, v, q, a)
    print("cancelling eps=%g: err %.2e rho %.1f trips %d status %d" % (eps, err, rho, trips, status))
    assert err < TOL
    if expect:
        assert trips == 1 and (status & 24) == expect, (status, expect)
    else:
        assert trips == 0
