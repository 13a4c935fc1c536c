"""Host-side checks of the counting module (no GPU): Counter's state_dict and initial values, the BAN models' state_dict layout and same-seed
initial values with a counter against the reference's (tests/golden/g14_*, make_golden_counter.py), `c_prj` absent without one, the drop-in
import path, the builders, and the argument errors of cti_counter_fwd / cti_counter_bwd."""
import ctypes
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import cti_amd
from golden_util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = cti_amd.pkg._lib

E_NULL, E_SHAPE, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -4, -5


class _DS:
    def __init__(self, ntoken, v_dim, num_ans):
        self.dictionary = types.SimpleNamespace(ntoken=ntoken)
        self.v_dim = v_dim
        self.num_ans_candidates = num_ans


def _keys(m):
    return [(k, list(v.shape)) for k, v in m.state_dict().items()]


def test_counter_state_dict_and_initial_values():
    st = torch.get_rng_state()
    c = cti_amd.Counter(10)
    assert torch.equal(torch.get_rng_state(), st)                       # no RNG consumed
    assert c.objects == 10 and c.already_sigmoided is False
    assert _keys(c) == [("f.%d.weight" % i, [17]) for i in range(8)]
    for f in c.f:
        assert isinstance(f, cti_amd.PiecewiseLin) and f.n == 16
        assert float(f.weight.data[0]) == 0.0 and torch.equal(f.weight.data[1:], torch.ones(16))
        assert f.weight.requires_grad
    assert cti_amd.Counter(5, already_sigmoided=True).already_sigmoided is True
    with pytest.raises(NotImplementedError):
        c.f[0](torch.zeros(3))


_CHILD = r'''
import inspect, json, os, sys
root = sys.argv[1]
sys.path.insert(0, os.path.join(root, "dropin"))
from src.counting import Counter
import src.counting
import cti_amd
c = Counter(10)
sig = lambda f: [p.name for p in inspect.signature(f).parameters.values()]
print(json.dumps({"same": Counter is cti_amd.Counter, "init": sig(Counter.__init__), "forward": sig(Counter.forward),
                  "keys": [[k, list(v.shape)] for k, v in c.state_dict().items()], "file": os.path.relpath(src.counting.__file__, root)}))
'''


def test_counter_resolves_through_the_dropin_path():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["same"]
    assert out["init"] == ["self", "objects", "already_sigmoided"]
    assert out["forward"] == ["self", "boxes", "attention"]
    assert out["keys"] == [["f.%d.weight" % i, [17]] for i in range(8)]
    assert out["file"] == os.path.join("dropin", "src", "counting.py")


def _build(name, with_counter=True):
    c = load(name).cfg
    a = dict(c["args"])
    ds = _DS(c["ntoken"], c["v_dim"], c["num_ans"])
    torch.manual_seed(0)
    if "mc" in name:
        a["use_counter"] = with_counter
        return c, cti_amd.build_mc_ban(types.SimpleNamespace(**a), ds)
    a["use_counter"] = False
    return c, cti_amd.build_ban(types.SimpleNamespace(**a), ds, counter=cti_amd.Counter(10) if with_counter else None)


@pytest.mark.parametrize("name", ["g14_ffoe_ban_cnt", "g14_mc_ban_cnt", "g14_ffoe_ban_cnt_step"])
def test_models_with_a_counter_have_the_reference_layout_and_init(name):
    c, m = _build(name)
    assert isinstance(m.counter, cti_amd.Counter) and m.counter.objects == 10
    assert _keys(m) == [(k, list(s)) for k, s in c["state_keys"]]          # names, shapes AND order (c_prj before classifier, counter last)
    for k, v in m.state_dict().items():
        ref = c["init_sums"][k]
        assert abs(float(v.double().sum()) - ref) <= 1e-6 * max(1.0, abs(ref)), k


@pytest.mark.parametrize("name", ["g14_ffoe_ban_cnt", "g14_mc_ban_cnt"])
def test_models_without_a_counter_have_no_c_prj(name):
    c, m = _build(name, with_counter=False)
    assert m.counter is None and not hasattr(m, "c_prj")
    keys = [k for k, _ in _keys(m)]
    assert not any(k.startswith("c_prj") or k.startswith("counter") for k in keys)
    assert keys == [k for k, _ in c["state_keys"] if not (k.startswith("c_prj") or k.startswith("counter"))]
    # the same seed gives the same parameters with and without a counter (c_prj consumes its part of the stream either way)
    for k, v in m.state_dict().items():
        ref = c["init_sums"][k]
        assert abs(float(v.double().sum()) - ref) <= 1e-6 * max(1.0, abs(ref)), k


def test_builders_and_the_bare_ffoe_flag():
    c = load("g14_ffoe_ban_cnt").cfg
    ds = _DS(c["ntoken"], c["v_dim"], c["num_ans"])
    a = dict(c["args"]); a["use_counter"] = True
    cnt = cti_amd.Counter(10)
    m = cti_amd.build_ban(types.SimpleNamespace(**a), ds, counter=cnt)       # the flag with a counter handed in: builds
    assert m.counter is cnt and len(m.c_prj) == a["gamma"]
    with pytest.raises(NotImplementedError, match=r"counter=cti_amd\.Counter\(10\)"):
        cti_amd.build_ban(types.SimpleNamespace(**a), ds)                    # the bare flag still raises, and says what to pass
    m2 = cti_amd.build_mc_ban(types.SimpleNamespace(**a), _DS(c["ntoken"], c["v_dim"], 2))
    assert isinstance(m2.counter, cti_amd.Counter) and m2.counter.objects == 10 and len(m2.c_prj) == a["gamma"]
    m3 = cti_amd.build_mc_ban(types.SimpleNamespace(**a), _DS(c["ntoken"], c["v_dim"], 2), cnt)
    assert m3.counter is cnt
    assert not hasattr(cti_amd.base_model, "_no_counter")


def test_counter_refuses_cpu_tensors():
    c = cti_amd.Counter(10)
    boxes, att = torch.zeros(2, 4, 12), torch.zeros(2, 12)
    with pytest.raises(cti_amd.CtiError):
        c(boxes, att)
    with pytest.raises(cti_amd.CtiError):
        c.forward_logits(torch.zeros(2, 12, 6), torch.zeros(2, 3, 12, 5))
    with pytest.raises(cti_amd.CtiError):
        cti_amd.ops.counter_fwd(boxes, att, [f.weight for f in c.f], 10)
    with pytest.raises(ValueError):
        c(boxes, torch.zeros(2, 3, 12))                                      # the module call takes a (batch, boxes) attention


def _w8(missing=None):
    return (ctypes.c_void_p * 8)(*[None if i == missing else 8 for i in range(8)])


def _fwd(**kw):
    a = dict(logits=8, sLb=360, sLg=0, sLv=10, sLq=1, boxes=8, sBb=144, sBc=1, sBv=4, weights=_w8(), sig=0, out=8, sOb=11, sOg=22, save=8,
             save_bytes=1 << 20, B=2, G=1, V=36, Q=10, objects=10, n=16)
    a.update(kw)
    return L.lib().cti_counter_fwd(*a.values(), None)


def _bwd(**kw):
    a = dict(dout=8, boxes=8, sBb=144, sBc=1, sBv=4, weights=_w8(), sig=0, save=8, save_bytes=1 << 20, dlogits=8, dw_part=8,
             B=2, G=1, V=36, Q=10, objects=10, n=16)
    a.update(kw)
    return L.lib().cti_counter_bwd(*a.values(), None)


@pytest.mark.parametrize("kw,code", [
    (dict(logits=None), E_NULL), (dict(boxes=None), E_NULL), (dict(weights=None), E_NULL), (dict(out=None), E_NULL), (dict(save=None), E_NULL),
    (dict(weights=_w8(missing=5)), E_NULL),
    (dict(B=0), E_SHAPE), (dict(G=0), E_SHAPE), (dict(V=0), E_SHAPE), (dict(Q=0), E_SHAPE), (dict(objects=0), E_SHAPE),
    (dict(V=9), E_SHAPE), (dict(sLv=-1), E_SHAPE), (dict(sBv=-4), E_SHAPE), (dict(sOb=10), E_SHAPE), (dict(G=3, sOb=22, sOg=11), E_SHAPE),
    (dict(objects=17, V=40, sOb=18, sOg=36), E_UNSUPPORTED), (dict(n=8), E_UNSUPPORTED), (dict(V=10000), E_UNSUPPORTED),
    (dict(save_bytes=16), E_WORKSPACE),
])
def test_forward_argument_errors_do_not_launch(kw, code):
    assert _fwd(**kw) == code
    assert b"cti_counter_fwd" in L.lib().cti_last_error_string()


@pytest.mark.parametrize("kw,code", [
    (dict(dout=None), E_NULL), (dict(boxes=None), E_NULL), (dict(weights=None), E_NULL), (dict(save=None), E_NULL), (dict(dlogits=None), E_NULL),
    (dict(dw_part=None), E_NULL), (dict(weights=_w8(missing=0)), E_NULL),
    (dict(B=0), E_SHAPE), (dict(V=9), E_SHAPE), (dict(sBc=-1), E_SHAPE),
    (dict(objects=17, V=40), E_UNSUPPORTED), (dict(n=15), E_UNSUPPORTED),
    (dict(save_bytes=16), E_WORKSPACE),
])
def test_backward_argument_errors_do_not_launch(kw, code):
    assert _bwd(**kw) == code
    assert b"cti_counter_bwd" in L.lib().cti_last_error_string()


def test_fewer_boxes_than_objects_says_so():
    assert _fwd(V=9) == E_SHAPE
    msg = L.lib().cti_last_error_string()
    assert b"9 boxes" in msg and b"V >= objects" in msg
    assert L.lib().cti_counter_save_bytes(2048) == 2048 * 48 * 4 and L.lib().cti_counter_save_bytes(0) == 0


def test_header_and_ctypes_table_list_the_counter_entries():
    src = open(os.path.join(ROOT, "include", "cti_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cti_[a-z0-9_]+)\s*\(", src))
    for name in ("cti_counter_fwd", "cti_counter_bwd", "cti_counter_save_bytes"):
        assert name in declared and name in L.SIGNATURES and hasattr(L.lib(), name)


def test_fixtures_keep_their_selection_margins():
    """What the generator asserted, re-read from the committed files: unit fixtures 1e-3 of the row's spread, model fixtures 5e-2 of the largest
    finite logit magnitude, and the reference's own fp32 run within 5e-5 / 2e-5 of its float64 run."""
    for name in ("rand", "ones_v100", "v10", "padded", "sigmoided", "obj5", "negw", "block", "allinf"):
        c = load("g14_cnt_" + name).cfg
        assert c["margin"] is None or c["margin"] > 1e-3
        assert c["ref_fp32_err"][0] <= 5e-5 and all(e <= 2e-5 for e in c["ref_fp32_err"][1:])
    for name in ("g14_ffoe_ban_cnt", "g14_mc_ban_cnt", "g14_ffoe_ban_cnt_step"):
        assert load(name).cfg["margin"] > 5e-2
    fx = load("g14_cnt_allinf")
    assert np.isneginf(fx.i["att"][fx.cfg["allinf"]]).all() and np.isfinite(fx.o["out"]).all()
