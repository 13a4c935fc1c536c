"""bench.py's --dump-outputs on the host: which arrays a forward's output becomes, their dtypes, the 64 MB bound, and the options that
refuse it (no GPU: the helpers take CPU tensors, the refusals happen before anything touches a device)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_small_forward_output_is_dumped_whole():
    out = torch.randn(2, 3, 4, 5, 2)
    d = bench.forward_dump(out)
    assert list(d) == ["tcnet_out"] and d["tcnet_out"] is out


def test_large_forward_output_is_first_and_last_sample_plus_a_seeded_sample():
    out = torch.randn(5, 3, 4, 7, 2)
    d = bench.forward_dump(out, limit=out.numel() * 4 - 1, sample=50)
    assert sorted(d) == ["tcnet_out_first_sample", "tcnet_out_last_sample", "tcnet_out_sampled"]
    assert torch.equal(d["tcnet_out_first_sample"], out[0]) and torch.equal(d["tcnet_out_last_sample"], out[4])
    idx = np.sort(np.random.RandomState(bench.SEED).randint(0, out.numel(), size=50, dtype=np.int64))
    assert torch.equal(d["tcnet_out_sampled"], out.reshape(-1)[torch.from_numpy(idx)])
    again = bench.forward_dump(out.clone(), limit=out.numel() * 4 - 1, sample=50)
    assert torch.equal(again["tcnet_out_sampled"], d["tcnet_out_sampled"])          # same positions on every run


def test_configs1_output_dump_stays_under_64_mb():
    """At B = 256 the configs[1] output is 3.2 GB: what is written is two samples whole plus the sampled elements."""
    c = bench.C2
    per_sample = c["V"] * c["Q"] * c["A"] * c["glimpse"] * 4
    assert c["B"] * per_sample > bench.DUMP_LIMIT
    assert 2 * per_sample + bench.DUMP_SAMPLE * 4 <= bench.DUMP_LIMIT


def test_write_outputs_dtypes_and_limit(tmp_path):
    arrays = {"a": torch.randn(3, 4).to(torch.bfloat16), "b": torch.randn(5, dtype=torch.float64), "c": torch.arange(6, dtype=torch.int32)}
    n = bench.write_outputs(str(tmp_path / "out"), arrays)
    got = {k: np.load(str(tmp_path / "out" / (k + ".npy"))) for k in arrays}
    assert got["a"].dtype == np.float32 and got["b"].dtype == np.float64 and got["c"].dtype == np.float32
    assert np.array_equal(got["a"], arrays["a"].float().numpy()) and np.array_equal(got["b"], arrays["b"].numpy())
    assert n == sum(a.nbytes for a in got.values())
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "big"), {"x": torch.zeros(100)}, limit=399)
    assert not (tmp_path / "big").exists()


@pytest.mark.parametrize("extra", [["--mode", "train"], ["--dry-launch"]])
def test_dump_outputs_refused_where_nothing_is_returned(tmp_path, extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dump-outputs", str(tmp_path / "d")] + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 2 and "--dump-outputs" in r.stderr
    assert not (tmp_path / "d").exists()
