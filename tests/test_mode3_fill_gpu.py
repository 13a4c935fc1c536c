"""mode3_fill_kernel loads a chunk of the representative object's block once and stores it into every padded object of the sample (csrc/cti_mode3_plan.hip), and
mode3_plan_kernel finds a sample's trailing run of zero objects from independent loads.  Every case runs the fused f16f6 forward with the key
CTI_TUNE_MODE3_SKIP_PADDED on and at 0 and asserts that the WHOLE output is equal bit for bit: the full walk is the reference, both runs are the same arithmetic, no
tolerance.  The shapes are the smallest at which the fill can go wrong: a range that starts inside an object and on an object's boundary, a source block smaller
than a workgroup's chunk, no multiple of it, and a multiple plus one piece, the scalar path, neighbouring samples with everything and nothing to fill, B = 1 and a
batch across the plan kernel's 256-sample chunk.  Needs an MI355X; the sibling tests/test_mode3_padded_objects_gpu.py holds the oracle comparisons."""
import numpy as np
import pytest
import torch

import cti_amd
from mode3_plan_host import BM, host_plan, live_row_tiles, zero_object_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
ops = cti_amd.ops
V, G, H, R = 36, 2, 512, 32
VD, QD, AD = 64, 48, 32
CHUNK_FLOATS = 256 * 2 * 4                  # a fill workgroup's chunk of the source block: 256 threads x FILL_PIECES (2) pieces x 4 floats (csrc/cti_mode3_plan.hip)


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(autouse=True)
def f16f6_mode():
    old, old_keep = cti_amd.get_precision(), ops._debug_keep_mode3_plan
    cti_amd.set_precision("f16f6")
    ops._debug_keep_mode3_plan = True
    ops._range_log.update(consecutive=0, skip=0); ops._range_owner.clear()
    # no host wait for the range guard's verdict and no NaN fill: what is compared is the f16f6 kernels' own output.  (With most objects zero the output's maximum is
    # small and the guard's cancellation estimate may ask for a re-run in bf16x3, which builds no plan and would leave nothing of the fill to compare.)
    cti_amd.set_range_check("poison"); ops.set_poison_bits(0)
    yield
    ops._debug_keep_mode3_plan = old_keep
    cti_amd.set_precision(old)
    cti_amd.set_range_check("sync"); ops.set_poison_bits(23)
    ops._range_log.update(consecutive=0, skip=0); ops._range_owner.clear()


_nets = {}


def net_for(v_dim=VD, q_dim=QD, a_dim=AD):
    key = (v_dim, q_dim, a_dim)
    if key not in _nets:
        torch.manual_seed(1204)
        _nets[key] = cti_amd.TCNet(v_dim, q_dim, a_dim, H, 1, R, G).to(DEV).eval()
    return _nets[key]


def inputs(B, A, seed, n_objs=V, n_q=14, v_dim=VD, q_dim=QD, a_dim=AD):
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


def check_equal(v, q, a, what, net=None):
    """Key on against key 0 over the whole output; the plan's totals against the host's, so that a path that silently skips nothing fails."""
    net = net or net_for()
    on, plan = run(net, v, q, a, 1)
    off, plan_off = run(net, v, q, a, 0)
    want = dict(host_plan(zero_object_mask(v), q.shape[1], G, a.shape[1]), samples=v.shape[0])
    print("%s: plan %s (host %s)" % (what, plan, want))
    assert plan_off is None and plan == want, what
    assert np.isfinite(off).all(), what
    differ = on.view(np.uint32) != off.view(np.uint32)
    assert not differ.any(), "%s: %d entries differ between the skipping walk and the full walk, the first in sample %d" % (
        what, int(differ.sum()), int(np.argwhere(differ)[0][0]))
    return on, plan


@pytest.mark.parametrize("n_rep", [0, 1, 9, 10, 34, 35])
def test_range_starts_inside_an_object(n_rep):
    """Q = 14, G = 2: 28 rows per object, so every 256-row tile boundary falls inside an object (9, 18, 27).  n_rep 0 and 1: one live tile; 9 (rows 252 .. 279) and 10:
    two; 34 and 35: all four, nothing to fill.  Sample 1 has an interior zero object as well."""
    v, q, a = inputs(2, 301, 100 + n_rep)
    v[:, n_rep:] = 0
    if n_rep > 4:
        v[1, 3] = 0
    out, plan = check_equal(v, q, a, "n_rep=%d" % n_rep)
    live = -(-(n_rep + 1) * 28 // BM)
    assert plan["live_row_tiles"] == 2 * live and plan["filled_rows"] == 2 * max(0, V * 28 - live * BM)
    for o in range(n_rep + 1, V):
        assert np.array_equal(out[0, o], out[0, n_rep])


@pytest.mark.parametrize("n_rep", [3, 15])
def test_range_starts_on_an_object_boundary(n_rep):
    """Q = 8, G = 2: 16 rows per object, a tile is 16 whole objects: the range starts with object 16, whole."""
    v, q, a = inputs(2, 301, 120 + n_rep, n_q=8)
    v[:, n_rep:] = 0
    v[1, 1] = 0
    _, plan = check_equal(v, q, a, "Q=8 n_rep=%d" % n_rep)
    assert plan["live_row_tiles"] == 2 and plan["filled_rows"] == 2 * (V * 16 - BM)


def test_a_single_object_to_fill():
    """Q = 8, 17 objects: 272 rows, one live tile of 16 objects, and object 16 alone is filled."""
    v, q, a = inputs(2, 301, 130, n_objs=17, n_q=8)
    v[0, 7:] = 0
    v[1, 15:] = 0
    _, plan = check_equal(v, q, a, "V=17")
    assert plan["live_row_tiles"] == 2 and plan["filled_rows"] == 2 * 16


@pytest.mark.parametrize("A", [8, 301, 439])
def test_source_block_against_the_chunk(A):
    """Q * A * G floats per object against the 2 048-float chunk: A = 8 is 224 floats (less than one chunk), A = 301 with its odd last column 8 428 (four chunks and
    59 pieces), A = 439 is 12 292 = six chunks and ONE 16-B piece."""
    obj = 14 * A * G
    assert obj % 4 == 0 and {8: obj < CHUNK_FLOATS, 301: obj % CHUNK_FLOATS not in (0, 4), 439: obj % CHUNK_FLOATS == 4}[A]
    v, q, a = inputs(3, A, 140 + A)
    v[0, 2:] = 0
    v[1, 12:] = 0
    v[2, 20:] = 0
    _, plan = check_equal(v, q, a, "A=%d" % A)
    assert plan["live_row_tiles"] == 1 + 2 + 3


def test_scalar_path_with_two_lengths_in_one_batch():
    """Q * A * G = 630 floats per object (the shape of the sibling's test_shape_that_takes_the_scalar_fill): no multiple of four, the fill copies float by float.
    14 rows per object, 40 objects = 560 rows = three tiles: sample 0 keeps one of them, sample 1 two, sample 2 all."""
    net = net_for(40, 32, 24)
    v, q, a = inputs(3, 45, 150, n_objs=40, n_q=7, v_dim=40, q_dim=32, a_dim=24)
    v[0, 3:] = 0
    v[1, 20:] = 0
    _, plan = check_equal(v, q, a, "scalar fill", net=net)
    assert plan["live_row_tiles"] == 1 + 2 + 3 and plan["filled_rows"] == (560 - 256) + (560 - 512)


@pytest.mark.parametrize("first", [0, 1])
def test_neighbours_with_everything_and_nothing_to_fill(first):
    """B = 9 (no multiple of 8): samples with all objects zero (everything behind the first tile is filled) alternate with samples without a zero object, beginning
    with either kind.  Equality over the whole output: no store crosses a sample's boundary."""
    v, q, a = inputs(9, 301, 160 + first)
    v[first::2] = 0
    n_all = len(range(first, 9, 2))
    _, plan = check_equal(v, q, a, "neighbours, first=%d" % first)
    assert plan["live_row_tiles"] == n_all + 4 * (9 - n_all) and plan["filled_rows"] == n_all * (V * 28 - BM)


def test_one_sample():
    v, q, a = inputs(1, 301, 170)
    v[0, 5:] = 0
    _, plan = check_equal(v, q, a, "B=1")
    assert plan["live_row_tiles"] == 1


def mixed_mask_batch(B, seed):
    """(B, V, VD) `v` in which every fifth sample is all zero, every third has interior zero objects in front of its trailing run, and the runs take every length."""
    v, q, a = inputs(B, 8, seed)
    rs = np.random.RandomState(seed + 1)
    for b in range(B):
        if b % 5 == 0:
            v[b] = 0
            continue
        n_rep = int(rs.randint(0, V + 1))
        v[b, n_rep:] = 0
        if b % 3 == 0 and n_rep > 2:
            v[b, int(rs.randint(0, n_rep - 1))] = 0                # interior: object n_rep - 1 stays live
    return v, q, a


def test_257_samples_and_the_plan_against_the_host_mirror():
    """B = 257 crosses the plan kernel's 256-sample chunk; all-zero mask rows and rows with an interior zero object are mixed.  The plan's fields (live tiles, row
    tiles, filled rows) against tests/mode3_plan_host.py for the same mask, and the output against the full walk."""
    B = 257
    v, q, a = mixed_mask_batch(B, 180)
    mask = zero_object_mask(v)
    assert mask.all(axis=1).sum() >= 52 and (mask[:, :-1] & ~mask[:, 1:]).any()                   # all-zero rows; a zero object followed by a live one
    per_sample = [live_row_tiles(m, 28)[0] for m in mask]
    assert per_sample[256] < 4 and set(per_sample) == {1, 2, 3, 4}                                # the sample behind the chunk boundary has rows to fill
    want = host_plan(mask, 14, G, 8)
    _, plan = check_equal(v, q, a, "B=257")
    assert plan["live_tiles"] == want["live_tiles"] == sum(per_sample)                              # (A = 8: one column tile)
    assert plan["live_row_tiles"] == want["live_row_tiles"] and plan["filled_rows"] == want["filled_rows"] > 0
