"""What skipping the mode-3 row tiles of zero-padded objects rests on, pinned where no GPU is needed (the GPU half is tests/test_mode3_padded_objects_gpu.py):
every image-side operation of TCNet.forward is per object row, so the oracle's output blocks of a sample's padded (all-zero) objects are equal bit for bit -- and
not zero; and the host restatement of the tile plan gives the live tile counts the GPU cases and the benchmark's seeded batch are held against."""
import numpy as np
import torch

import bench
import cti_amd
from oracle import cti_oracle as O
from mode3_plan_host import BM, host_plan, live_row_tiles, zero_object_mask


def test_oracle_blocks_of_padded_objects_are_equal_and_not_zero():
    torch.manual_seed(3)
    net = cti_amd.TCNet(24, 20, 12, 32, 1, 4, 2).eval()
    sd = {k: t.detach().numpy().copy() for k, t in net.state_dict().items()}
    rs = np.random.RandomState(0)
    v = np.abs(rs.standard_normal((2, 14, 24))).astype(np.float32)
    q = rs.standard_normal((2, 5, 20)).astype(np.float32)
    a = rs.standard_normal((2, 9, 12)).astype(np.float32)
    v[0, 9:] = 0                                                  # 5 and 9 trailing zero objects
    v[1, 5:] = 0
    v[1, 7, 3] = -0.0
    for dtype in (np.float32, np.float64):
        out = O.tcnet_forward(v, q, a, sd, dtype=dtype)
        for b, first in ((0, 9), (1, 5)):
            for obj in range(first + 1, 14):
                assert np.array_equal(out[b, obj], out[b, first]), (dtype, b, obj)
            assert np.abs(out[b, first]).max() > 0
            assert not np.array_equal(out[b, first], out[b, first - 1])


def test_plan_of_one_sample():
    z = lambda *idx: np.isin(np.arange(36), idx)                  # noqa: E731
    tail = lambda n: np.arange(36) >= n                           # noqa: E731
    assert live_row_tiles(tail(36), 28) == (4, 36)                # no zero object: every tile
    assert live_row_tiles(tail(0), 28) == (1, 0)                  # all zero: one object is computed
    assert [live_row_tiles(tail(n), 28)[0] for n in (8, 9, 10, 18, 27, 35)] == [1, 2, 2, 3, 4, 4]      # object 9 straddles row 256, 18 row 512, 27 row 768
    assert live_row_tiles(z(20), 28) == (4, 36)                   # an interior zero object is live
    assert live_row_tiles(z(3) | tail(12), 28) == (2, 12)
    m = np.stack([tail(36), tail(0), tail(9)])
    assert host_plan(m, 14, 2, 301) == {"live_tiles": 7 * 2, "live_row_tiles": 7, "filled_rows": (1008 - 256) + (1008 - 512)}


def test_mask_is_the_bit_exact_magnitude_or():
    v = np.zeros((1, 4, 8), np.float32)
    v[0, 1, 2] = -0.0
    v[0, 2, 5] = np.nan
    v[0, 3, 0] = 1e-45                                            # a subnormal is not zero
    assert zero_object_mask(v).tolist() == [[True, True, False, False]]


def test_live_tiles_of_the_benchmark_batch():
    """The object counts bench.synth_inputs draws at SEED + 1 (rank 0), re-drawn from the same generator in the same order (v, then nv) without the 1 GB of `a`:
    798 of the 1 024 row tiles are live, 13 566 of 17 408 tiles."""
    c = bench.C2
    g = torch.Generator(device="cpu").manual_seed(bench.SEED + 1)
    torch.randn(c["B"], c["V"], c["v_dim"], generator=g).abs_()
    nv = torch.randint(10, c["V"] + 1, (c["B"],), generator=g).numpy()
    mask = np.arange(c["V"])[None, :] >= nv[:, None]
    plan = host_plan(mask, c["Q"], c["glimpse"], c["A"])
    assert c["V"] * c["Q"] * c["glimpse"] == 1008 and BM == 256
    assert plan["live_row_tiles"] == 798 and plan["live_tiles"] == 13566
    assert plan["filled_rows"] == sum(max(0, 1008 - 256 * -(-min(36, int(n) + 1) * 28 // 256)) for n in nv)
