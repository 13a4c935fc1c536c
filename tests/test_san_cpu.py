"""Host-side checks of the SAN baseline (no GPU): StackedAttention through the drop-in import path with the reference's signatures, the
builders' state_dict layout and same-seed initial values against the reference's (tests/golden/g13_*, make_golden_san.py), and the argument
errors of the two C-ABI entries of csrc/cti_san.hip."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

import cti_amd
from golden_util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = cti_amd.pkg._lib

E_NULL, E_SHAPE = -1, -2


class _DS:
    def __init__(self, ntoken, v_dim, num_ans):
        self.dictionary = types.SimpleNamespace(ntoken=ntoken)
        self.v_dim = v_dim
        self.num_ans_candidates = num_ans


def _keys(m):
    return [(k, list(v.shape)) for k, v in m.state_dict().items()]


_CHILD = r'''
import inspect, json, os, sys
root = sys.argv[1]
sys.path.insert(0, os.path.join(root, "dropin"))
from src.attention import StackedAttention
import cti_amd
m = StackedAttention(2, 24, 12, 20, 11, 0.0)
sig = lambda f: [p.name for p in inspect.signature(f).parameters.values() if not p.name.startswith("_")]
print(json.dumps({"same": StackedAttention is cti_amd.StackedAttention, "init": sig(StackedAttention.__init__), "forward": sig(StackedAttention.forward),
                  "keys": [[k, list(v.shape)] for k, v in m.state_dict().items()], "drop": m.dropout.p, "stacks": m.num_stacks}))
'''


def test_stacked_attention_constructs_through_the_dropin_path():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["same"]
    assert out["init"] == ["self", "num_stacks", "img_feat_size", "ques_feat_size", "att_size", "output_size", "drop_ratio"]
    assert out["forward"] == ["self", "img_feat", "ques_feat", "v_mask"]
    assert out["keys"] == [[k, list(s)] for k, s in load("g13_san_s2").cfg["state_keys"]]
    assert out["drop"] == 0.0 and out["stacks"] == 2


@pytest.mark.parametrize("name", ["g13_san_s1", "g13_san_s2", "g13_san_s3"])
def test_stacked_attention_state_dict_matches_reference(name):
    c = load(name).cfg
    m = cti_amd.StackedAttention(c["num_stacks"], c["v_dim"], c["q_dim"], c["att"], 11, 0.0)
    assert _keys(m) == [(k, list(s)) for k, s in c["state_keys"]]


@pytest.mark.parametrize("name,builder", [("g13_ffoe_san", "build_san"), ("g13_mc_san", "build_mc_san"), ("g13_ffoe_san_step", "build_san")])
def test_builder_layout_and_same_seed_init(name, builder):
    c = load(name).cfg
    args = types.SimpleNamespace(**c["args"])
    torch.manual_seed(0)
    m = getattr(cti_amd, builder)(args, _DS(c["ntoken"], c["v_dim"], c["num_ans"]))
    assert _keys(m) == [(k, list(s)) for k, s in c["state_keys"]]
    for k, v in m.state_dict().items():
        ref = c["init_sums"][k]
        assert abs(float(v.double().sum()) - ref) <= 1e-6 * max(1.0, abs(ref)), k


def test_san_models_refuse_cpu_tensors():
    c = load("g13_ffoe_san").cfg
    m = cti_amd.build_san(types.SimpleNamespace(**c["args"]), _DS(c["ntoken"], c["v_dim"], c["num_ans"])).eval()
    with pytest.raises(cti_amd.CtiError):
        with torch.no_grad():
            m.v_att(torch.zeros(2, 3, c["v_dim"]), torch.zeros(2, c["args"]["num_hid"]))


def _fwd(**kw):
    a = dict(P=1, ldp=8, sP=64, qv=1, sq=8, w=1, bias=None, keep=None, p_drop=0.0, v_mask=1, X=1, ldx=8, sX=64, logits=1, prob=1, pooled=1,
             ldo=8, B=2, N=8, A=8, Dx=8)
    a.update(kw)
    return L.lib().cti_san_attend_fwd(*a.values(), None)


def _bwd(**kw):
    a = dict(P=1, ldp=8, sP=64, qv=1, sq=8, w=1, keep=None, p_drop=0.0, X=1, ldx=8, sX=64, x_is_p=0, prob=1, dpooled=1, ldg=8, dP=1, lddp=8,
             sdP=64, dqv=1, sdq=8, dw_part=1, db_part=1, dlogit=1, dX=None, lddx=8, sdX=64, B=2, N=8, A=8, Dx=8)
    a.update(kw)
    return L.lib().cti_san_attend_bwd(*a.values(), None)


@pytest.mark.parametrize("kw,code", [
    (dict(P=None), E_NULL), (dict(qv=None), E_NULL), (dict(w=None), E_NULL), (dict(X=None), E_NULL), (dict(logits=None), E_NULL),
    (dict(prob=None), E_NULL), (dict(pooled=None), E_NULL),
    (dict(B=0), E_SHAPE), (dict(N=0), E_SHAPE), (dict(A=0), E_SHAPE), (dict(Dx=0), E_SHAPE), (dict(N=-3), E_SHAPE),
    (dict(ldp=7), E_SHAPE), (dict(sP=63), E_SHAPE), (dict(sq=7), E_SHAPE), (dict(ldx=7), E_SHAPE), (dict(sX=10), E_SHAPE), (dict(ldo=7), E_SHAPE),
    (dict(keep=1, p_drop=1.0), E_SHAPE), (dict(keep=1, p_drop=-0.1), E_SHAPE),
])
def test_forward_argument_errors_do_not_launch(kw, code):
    assert _fwd(**kw) == code
    assert b"cti_san_attend_fwd" in L.lib().cti_last_error_string()


@pytest.mark.parametrize("kw,code", [
    (dict(P=None), E_NULL), (dict(prob=None), E_NULL), (dict(dpooled=None), E_NULL), (dict(dP=None), E_NULL), (dict(dqv=None), E_NULL),
    (dict(dw_part=None), E_NULL), (dict(db_part=None), E_NULL), (dict(dlogit=None), E_NULL), (dict(X=None), E_NULL),
    (dict(B=0), E_SHAPE), (dict(N=0), E_SHAPE), (dict(A=0), E_SHAPE), (dict(Dx=0), E_SHAPE),
    (dict(x_is_p=1, Dx=4, ldg=4), E_SHAPE), (dict(x_is_p=1, dX=1), E_SHAPE), (dict(lddp=7), E_SHAPE), (dict(sdq=4), E_SHAPE),
    (dict(dX=1, lddx=4), E_SHAPE), (dict(ldg=7), E_SHAPE), (dict(keep=1, p_drop=1.5), E_SHAPE),
])
def test_backward_argument_errors_do_not_launch(kw, code):
    assert _bwd(**kw) == code
    assert b"cti_san_attend_bwd" in L.lib().cti_last_error_string()


def test_backward_pool_of_p_needs_no_x():
    # x_is_p: X may be NULL; the call still refuses before launching when another argument is wrong
    assert _bwd(x_is_p=1, X=None, B=0) == E_SHAPE
