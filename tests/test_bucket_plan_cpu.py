"""The host plan of bucketed batching (batch.py: bucket_plan, rank_plan, bucket_widths_for, the host side of DeviceLoader(pad_to='bucket')) on the
synthetic table counts[i] = 10 + (37 * i) % 91, which is uniform on 10 .. 100.  Everything is integer arithmetic: compared exactly.  No GPU."""
import types

import numpy as np
import pytest
import torch

import cti_amd

WIDTHS = (25, 40, 55, 70, 85, 100)


def _counts(N):
    return (10 + (37 * np.arange(N)) % 91).astype(np.int32)


def _order(N, seed=3):
    return torch.randperm(N, generator=torch.Generator().manual_seed(seed))


def _groups(entries, batches):
    return [entries[lo:hi].numpy() for lo, hi, _ in batches]


def _check_consequences(N, counts, entries, batches, SB, widths):
    """The four consequences of the rule for a plan without drop_last; returns the object rows it pads to."""
    assert entries.dtype == torch.int64 and sorted(entries.tolist()) == list(range(N))            # every entry exactly once
    assert [lo for lo, _, _ in batches] == [0] + [hi for _, hi, _ in batches[:-1]] and (not batches or batches[-1][1] == N)
    sizes = [hi - lo for lo, hi, _ in batches]
    assert all(s == SB for s in sizes[:-1]) and 0 < sizes[-1] <= SB                              # full except at most one, which comes last
    assert len(batches) == -(-N // SB)                                                           # as many as the unbucketed rule makes
    for g, (_, _, width) in zip(_groups(entries, batches), batches):
        assert width in widths and counts[g].max() <= width                                      # nothing wider than its batch
    return sum((hi - lo) * width for lo, hi, width in batches)


def test_synthetic_case_pads_to_64000_rows_where_one_width_pads_to_100000():
    N, B = 1000, 50
    counts, order = _counts(N), _order(N)
    assert counts.min() == 10 and counts.max() == 100 and int(counts.sum()) == 54991
    entries, batches = cti_amd.bucket_plan(order, counts, WIDTHS, B)
    rows = _check_consequences(N, counts, entries, batches, B, WIDTHS)
    assert len(batches) == 20 and all(hi - lo == B for lo, hi, _ in batches)                     # no short one
    assert rows == 64000
    assert [w for _, _, w in batches] == sorted(w for _, _, w in batches)                        # the buckets are walked upwards
    one, cuts = cti_amd.bucket_plan(order, counts, (100,), B)
    assert sum((hi - lo) * w for lo, hi, w in cuts) == 100000
    assert torch.equal(one, order)                                                               # one bucket: the order as it came
    # the rule itself, restated as the walk: carry + the bucket's entries in the order of `order`, full groups off the front
    want, carry = [], []
    bucket = np.searchsorted(np.asarray(WIDTHS), counts, side="left")
    for j in range(len(WIDTHS)):
        pool = carry + [int(e) for e in order.tolist() if bucket[e] == j]
        while len(pool) >= B:
            want.append((pool[:B], WIDTHS[j]))
            pool = pool[B:]
        carry = pool
    assert not carry
    assert [(g.tolist(), w) for g, (_, _, w) in zip(_groups(entries, batches), batches)] == want


def test_the_short_batch_comes_last_and_is_as_wide_as_its_largest_count_asks():
    N, B = 257, 50
    counts, order = _counts(N), _order(N)
    entries, batches = cti_amd.bucket_plan(order, counts, WIDTHS, B)
    _check_consequences(N, counts, entries, batches, B, WIDTHS)
    assert [hi - lo for lo, hi, _ in batches] == [50] * 5 + [7]
    last = entries[batches[-1][0]:].numpy()
    assert batches[-1][2] == min(w for w in WIDTHS if w >= counts[last].max())


def test_two_ranks_see_equal_widths_and_partition_the_epoch():
    N, B, world = 257, 25, 2
    counts, order = _counts(N), _order(N)
    entries, batches = cti_amd.bucket_plan(order, counts, WIDTHS, B, world=world)
    _check_consequences(N, counts, entries, batches, B * world, WIDTHS)
    seen, widths = [], []
    for rank in range(world):
        mine, cuts = cti_amd.rank_plan(entries, batches, rank, world)
        assert mine.dtype == torch.int64 and mine.is_contiguous()
        for (lo, hi, width), (glo, ghi, gwidth) in zip(cuts, batches):
            assert width == gwidth and torch.equal(mine[lo:hi], entries[glo:ghi][rank::world])
            assert counts[mine[lo:hi].numpy()].max() <= width
        unbucketed = cti_amd.DeviceLoader(_HostDS(N), B, rank=rank, world=world)
        assert len(cuts) == len(unbucketed) == 6
        seen.append(mine.numpy())
        widths.append([w for _, _, w in cuts])
    assert widths[0] == widths[1]
    assert not set(seen[0]) & set(seen[1]) and sorted(np.concatenate(seen).tolist()) == list(range(N))
    assert [len(s) for s in seen] == [129, 128]
    with pytest.raises(ValueError):
        cti_amd.rank_plan(entries, batches, 2, 2)


def test_batches_per_rank_follow_m_plus_t_above_r():
    N, B, world = 101, 50, 2
    counts = _counts(N)
    m, t = divmod(N, B * world)
    assert (m, t) == (1, 1)
    entries, batches = cti_amd.bucket_plan(torch.arange(N), counts, WIDTHS, B, world=world)
    for rank in range(world):
        mine, cuts = cti_amd.rank_plan(entries, batches, rank, world)
        assert len(cuts) == m + (t > rank)
        assert len(cuts) == len(cti_amd.DeviceLoader(_HostDS(N), B, rank=rank, world=world))                       # today's rule
        assert len(cuts) == len(cti_amd.DeviceLoader(_HostDS(N), B, rank=rank, world=world, pad_to="bucket", bucket_widths=WIDTHS))
        assert len(mine) == m * B + len(range(rank, t, world))


def test_edges():
    N, B = 257, 50
    counts, order = _counts(N), _order(N)
    entries, batches = cti_amd.bucket_plan(order, counts, WIDTHS, B, drop_last=True)              # drop_last: the short group goes
    full, _ = cti_amd.bucket_plan(order, counts, WIDTHS, B)
    assert len(entries) == 250 and len(batches) == 5 and all(hi - lo == B for lo, hi, _ in batches)
    assert torch.equal(entries, full[:250])
    widths = (5, 25, 40, 41, 55, 70, 85, 100, 200)                                                # buckets without entries: first, middle, last
    entries, batches = cti_amd.bucket_plan(order, counts, widths, B)
    _check_consequences(N, counts, entries, batches, B, widths)
    assert not {5, 200} & {w for _, _, w in batches}
    entries, batches = cti_amd.bucket_plan(order, counts, (9, 100, 101), B)                       # everything in one bucket
    assert torch.equal(entries, order) and [w for _, _, w in batches] == [100] * 6
    entries, batches = cti_amd.bucket_plan(torch.arange(N), counts, WIDTHS, B)                    # unshuffled: ascending within a bucket
    bucket = np.searchsorted(np.asarray(WIDTHS), counts[entries.numpy()], side="left")
    assert (np.diff(bucket) >= 0).all() and all((np.diff(entries.numpy()[bucket == j]) > 0).all() for j in range(len(WIDTHS)))
    few, cuts = cti_amd.bucket_plan(torch.arange(3), counts, WIDTHS, B)                           # fewer entries than a batch
    assert few.tolist() == [0, 1, 2] and cuts == [(0, 3, 85)] and counts[:3].tolist() == [10, 47, 84]
    assert cti_amd.bucket_plan(torch.arange(3), counts, WIDTHS, B, drop_last=True)[1] == []
    with pytest.raises(ValueError, match="below the largest"):
        cti_amd.bucket_plan(order, counts, (25, 40, 99), B)
    for bad in ((25, 25, 100), (40, 25, 100), (), (-1, 100)):
        with pytest.raises(ValueError, match="ascending"):
            cti_amd.bucket_plan(order, counts, bad, B)
    with pytest.raises(ValueError):
        cti_amd.bucket_plan(order, counts, WIDTHS, 0)


def test_quantile_widths():
    counts = _counts(1000)
    for K in (1, 4, 6):
        w = cti_amd.bucket_widths_for(counts, K)
        srt = np.sort(counts)
        assert list(w) == sorted(set(int(srt[-(-(j + 1) * 1000 // K) - 1]) for j in range(K)))
        assert len(w) == K and w[-1] == counts.max() and all(a < b for a, b in zip(w, w[1:]))
    assert cti_amd.bucket_widths_for(counts, 1) == (100,)
    few = np.array([3, 7, 7, 3, 7], np.int32)                                                     # more widths asked for than distinct counts
    assert cti_amd.bucket_widths_for(few, 4) == (3, 7) and cti_amd.bucket_widths_for(few, 50) == (3, 7)
    assert cti_amd.bucket_widths_for(_counts(1000), 500)[-1] == 100 and len(cti_amd.bucket_widths_for(_counts(1000), 500)) == 91
    with pytest.raises(ValueError):
        cti_amd.bucket_widths_for(counts, 0)


class _HostDS:
    """What DeviceLoader reads of a DeviceDataset before it assembles."""

    def __init__(self, N):
        self.N, self.packed, self.counts_host = N, types.SimpleNamespace(dataset="the original"), _counts(N)
        self.v_max, self.max_boxes = int(self.counts_host.max()), 100

    def __len__(self):
        return self.N


def test_the_loader_plans_an_epoch_on_the_host():
    N, B = 257, 50
    ds = _HostDS(N)
    loader = cti_amd.DeviceLoader(ds, B, shuffle=True, generator=torch.Generator().manual_seed(3), pad_to="bucket", bucket_widths=WIDTHS)
    assert loader.widths == WIDTHS and len(loader) == 6 and loader.plan_widths is None
    entries, cuts = loader.bucket_epoch()
    g = torch.Generator().manual_seed(3)                                    # what it drew: the epoch's randperm, then the order of the full batches
    order = torch.randperm(N, generator=g)
    visit = torch.randperm(5, generator=g).tolist()
    want, groups = cti_amd.bucket_plan(order, ds.counts_host, WIDTHS, B)
    assert visit != sorted(visit)
    assert [hi - lo for lo, hi, _ in cuts] == [50] * 5 + [7]                 # the short one stays last
    assert [w for _, _, w in cuts] == [groups[k][2] for k in visit] + [groups[5][2]]
    for (lo, hi, _), k in zip(cuts, visit + [5]):
        assert torch.equal(entries[lo:hi], want[groups[k][0]:groups[k][1]])
    again, _ = loader.bucket_epoch()                                        # the generator has moved on
    assert sorted(again.tolist()) == list(range(N)) and not torch.equal(again, entries)
    plain = cti_amd.DeviceLoader(ds, B, pad_to="bucket", bucket_widths=WIDTHS)
    entries, cuts = plain.bucket_epoch()                                    # unshuffled: widths ascending
    assert [w for _, _, w in cuts[:-1]] == sorted(w for _, _, w in cuts[:-1]) and cuts[-1][1] - cuts[-1][0] == 7
    assert len(cti_amd.DeviceLoader(ds, B, drop_last=True, pad_to="bucket", bucket_widths=WIDTHS).bucket_epoch()[1]) == 5
    by_k = cti_amd.DeviceLoader(ds, B, pad_to="bucket", bucket_widths=6)
    assert by_k.widths == cti_amd.bucket_widths_for(ds.counts_host, 6) and by_k.widths[-1] == 100
    # a loader built without the new arguments draws from the generator what it drew before: one randperm
    g1, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    old = cti_amd.DeviceLoader(ds, B, shuffle=True, generator=g1, pad_to="max")
    assert torch.equal(old.epoch_order(), torch.randperm(N, generator=g2)) and torch.equal(g1.get_state(), g2.get_state())
    assert old.widths is None and old.plan_widths is None
    with pytest.raises(ValueError, match="needs bucket_widths"):
        cti_amd.DeviceLoader(ds, B, pad_to="bucket")
    with pytest.raises(ValueError, match="belongs to pad_to='bucket'"):
        cti_amd.DeviceLoader(ds, B, pad_to="max", bucket_widths=WIDTHS)
    with pytest.raises(ValueError, match="below the 100 objects"):
        cti_amd.DeviceLoader(ds, B, pad_to="bucket", bucket_widths=(25, 99))
    with pytest.raises(ValueError, match="ascending"):
        cti_amd.DeviceLoader(ds, B, pad_to="bucket", bucket_widths=(50, 25, 100))
