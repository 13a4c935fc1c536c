"""The trainer's drop-in boundary without a GPU: the reference's import lines (src/FFOE/train.py:10, src/MC/train.py) resolve to the package's classes with
the reference's positional names, a CPU model is refused, and the accumulation entry points return their error codes before anything is launched.  The
import checks run in child processes (a top-level `src` namespace must not leak into the test session), as in tests/test_dropin_imports.py."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

import cti_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r'''
import inspect, json, os, sys
root = sys.argv[1]
sys.path.insert(0, os.path.join(root, "dropin"))
exec(sys.argv[2])
import cti_amd
pos = lambda f: [p.name for p in inspect.signature(f).parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
import src.%s.trainer as T
print(json.dumps({"cls": Trainer is getattr(cti_amd, sys.argv[3]), "init": pos(Trainer.__init__), "train_step": pos(Trainer.train_step),
                  "score": compute_score_with_logits is cti_amd.compute_score_with_logits,
                  "mc": getattr(T, "compute_score_mc", None) is cti_amd.compute_score_mc,
                  "file": os.path.relpath(T.__file__, root)}))
'''


def _run(flavour, line, cls):
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, "-c", _CHILD % flavour, ROOT, line, cls], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600, cwd=os.path.join(ROOT, "tests"))
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.parametrize("flavour,cls", [("FFOE", "Trainer"), ("MC", "MCTrainer")])
def test_reference_trainer_import_lines_resolve_to_the_package(flavour, cls):
    res = _run(flavour, "from src.%s.trainer import Trainer, compute_score_with_logits" % flavour, cls)
    assert res["cls"] and res["score"]
    assert res["mc"] == (flavour == "MC")
    assert res["init"] == ["self", "args", "model", "criterion", "optimizer"]            # src/FFOE/trainer.py:17
    assert res["train_step"] == ["self", "sample", "update_params"]                       # src/FFOE/trainer.py:97
    assert res["file"] == os.path.join("dropin", "src", flavour, "trainer.py")


def test_a_cpu_model_is_refused():
    args = types.SimpleNamespace(device="cpu", model="cti", distillation=False, clip_norm=0.25, gamma=2)
    for cls in (cti_amd.Trainer, cti_amd.MCTrainer):
        with pytest.raises(cti_amd.CtiError):
            cls(args, torch.nn.Linear(4, 3), torch.nn.BCEWithLogitsLoss(reduction="sum"))
    lin = torch.nn.Linear(4, 3)
    with pytest.raises(cti_amd.CtiError):
        cti_amd.FlatAdamaxDP.from_torch(lin, torch.optim.Adamax(lin.parameters()), 0.25)


def test_accumulation_entry_points_check_their_arguments_before_any_launch():
    import ctypes
    lib = cti_amd.pkg._lib.lib()
    one, al = 8, 256                                                          # non-NULL addresses: nothing is dereferenced before the checks
    tbl = (ctypes.c_int64 * 6)(0, 0, 100, 0, 128, 10)
    assert lib.cti_flat_gather_acc(tbl, 2, al, 1024, None, None) == -1        # NULL micro-batch count
    assert b"NULL" in lib.cti_last_error_string()
    assert lib.cti_flat_gather_acc(tbl, 2, None, 1024, one, None) == -1       # NULL flat buffer
    bad = (ctypes.c_int64 * 6)(0, 0, 100, 0, 64, 10)
    assert lib.cti_flat_gather_acc(bad, 2, al, 1024, one, None) == -2         # second slot starts inside the first
    assert b"cti_flat_gather_acc" in lib.cti_last_error_string()
    assert lib.cti_flat_gather_acc(tbl, 2, al, 130, one, None) == -2          # n not a multiple of 4
    assert lib.cti_flat_gather(bad, 2, al, 1024, None) == -2 and b"cti_flat_gather:" in lib.cti_last_error_string()
    assert lib.cti_flat_scale_sumsq_g(al, 64, 0, one, al, None) == -2         # world <= 0
    assert lib.cti_flat_scale_sumsq_g(al, 64, 2, None, al, None) == -1
    assert lib.cti_flat_scale_sumsq_g(None, 64, 2, one, al, None) == -1
    assert lib.cti_counter_set(None, 0, None) == -1
