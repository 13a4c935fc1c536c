"""Batches assembled on the device from tables that stay there: the reference's `Dataset.__getitem__` (src/FFOE/dataset.py:350-376,
src/MC/dataset.py:246-265), `utils.trim_collate` (src/utils.py:120-169) and `.to(device)` on the kernels of csrc/cti_batch.hip.

The reference builds every batch on the host: per question two ragged tables sliced through `pos_boxes` and cut to `max_boxes`, a sparse answer
`scatter_`ed into a zeroed row, a float16 teacher row widened; the collate pads every image to the batch's largest object count; the result is sent from
pageable memory.  Here `pack_dataset` flattens such a data set once on the host, `DeviceDataset` uploads the tables once, and `assemble(idx)` builds the
reference's tuple from a DEVICE vector of entry numbers in a handful of launches: no host copy, no host-to-device copy, no synchronisation, and
nothing that depends on the step as a kernel argument, so an assemble call can be captured and replayed.  `DeviceLoader` stands where the reference
has `DataLoader(dataset, batch_size, collate_fn=utils.trim_collate)`.

`pad_to=None` reproduces trim_collate (the batch's largest object count, which the host has to know: the index vector is needed there too);
`pad_to='max'` or an int pads every batch alike, which keeps ONE captured training graph valid for a whole epoch of adaptive features (the mode-3
product skips the row tiles of the padding objects, csrc/cti_mode3_plan.hip); `pad_to='bucket'` groups the entries of an epoch by object count
(`bucket_plan`) so that every batch has one of a few widths, each of which a Trainer(max_graphs=K) captures once."""
import numpy as np
import torch

from . import _lib as L
from . import ops

_I32 = np.iinfo(np.int32)


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _tokens(x, what, i, shape=None):
    a = _np(x)
    if a.dtype.kind not in "iu":
        raise ValueError("entry %d: %s must hold integers, got %s" % (i, what, a.dtype))
    if a.size and (a.min() < _I32.min or a.max() > _I32.max):
        raise ValueError("entry %d: %s holds a token outside int32" % (i, what))
    if shape is not None and a.shape != shape:
        raise ValueError("entry %d: %s has shape %s, entry 0 has %s" % (i, what, a.shape, shape))
    return a.astype(np.int32)


class PackedDataset:
    """What `pack_dataset` produces: flat numpy arrays on the host.

      kind 'ffoe' or 'mc'; dataset (the original object); num_ans_candidates; adaptive; max_boxes (the cut; a non-adaptive table is never cut)
      features (rows, d) fp32, spatials (rows, ds) fp32, pos (n_img, 2) int64 row spans (synthesised for a non-adaptive (n_img, V0, d) table)
      image (N,) int64, counts (N,) int32 = min(objects of the entry's image, max_boxes), q_token (N, Lq) int32, question_id (N,) int64
      ffoe: ans_token (N, La) int32 or None (TDIUC has none: the tuple then has no `ans` position), ans_off (N + 1,) int64 / ans_labels int32 /
            ans_scores fp32 (CSR), teacher (N, n) float16 or None
      mc:   label (N, 4) fp32, ans_mc (N, 4, La) int32, ans_gt (N, La) int32"""

    def __len__(self):
        return int(self.image.shape[0])


def pack_dataset(dataset):
    """Flatten a reference-shaped data set object (VQAFeatureDataset / TDIUCFeatureDataset / V7WDataset, read by attribute: `features`, `spatials`,
    `pos_boxes` when `adaptive`, `max_boxes` or `max_box`, `num_ans_candidates`, `entries`) into a PackedDataset.  Host only.

    The absent-answer cases of the reference all become zero rows: `answer` None, labels None or empty, `teacher_logit` missing (the reference's
    `except: teacher_logit = 0`); the tuple keeps its positions.  Refused, with the entry named: duplicate labels in one entry (scatter_ would be
    undefined), a label outside the answer candidates, a token outside int32, a teacher row that float16 does not hold exactly, an image index or a
    pos_boxes row outside the table."""
    p = PackedDataset()
    p.dataset = dataset
    entries = dataset.entries
    N = len(entries)
    if N == 0:
        raise ValueError("pack_dataset: the data set has no entries")
    p.kind = "mc" if "ans_mc_token" in entries[0] else "ffoe"
    p.num_ans_candidates = int(dataset.num_ans_candidates)
    p.adaptive = bool(getattr(dataset, "adaptive", False))
    feats, spats = _np(dataset.features), _np(dataset.spatials)
    if feats.dtype != np.float32 or spats.dtype != np.float32:
        raise ValueError("pack_dataset: features %s and spatials %s must be float32" % (feats.dtype, spats.dtype))
    if p.adaptive:
        if feats.ndim != 2 or spats.ndim != 2 or feats.shape[0] != spats.shape[0]:
            raise ValueError("pack_dataset: adaptive features %s and spatials %s must be (rows, d) with the same rows" % (feats.shape, spats.shape))
        pos = _np(dataset.pos_boxes).astype(np.int64).reshape(-1, 2)
        bad = np.flatnonzero((pos[:, 0] < 0) | (pos[:, 1] < pos[:, 0]) | (pos[:, 1] > feats.shape[0]))
        max_boxes = int(dataset.max_boxes if hasattr(dataset, "max_boxes") else dataset.max_box)
        if max_boxes < 0:
            raise ValueError("pack_dataset: max_boxes is %d" % max_boxes)
    else:
        if feats.ndim != 3 or spats.ndim != 3 or feats.shape[:2] != spats.shape[:2]:
            raise ValueError("pack_dataset: non-adaptive features %s and spatials %s must be (n_img, V, d) alike" % (feats.shape, spats.shape))
        n_img, V0 = feats.shape[:2]
        pos = np.stack([np.arange(n_img, dtype=np.int64) * V0, np.arange(1, n_img + 1, dtype=np.int64) * V0], 1)
        feats, spats = feats.reshape(n_img * V0, -1), spats.reshape(n_img * V0, -1)
        bad = np.zeros(0, np.int64)
        max_boxes = int(V0)                                  # the reference indexes a non-adaptive table whole (src/MC/dataset.py:248-250)
    p.features, p.spatials, p.pos, p.max_boxes = np.ascontiguousarray(feats), np.ascontiguousarray(spats), np.ascontiguousarray(pos), max_boxes
    n_img = pos.shape[0]
    bad = set(int(i) for i in bad)

    image = np.zeros(N, np.int64)
    qid = np.zeros(N, np.int64)
    q0 = _tokens(entries[0]["q_token"], "q_token", 0)
    q_token = np.zeros((N,) + q0.shape, np.int32)
    for i, e in enumerate(entries):
        img = int(e["image"])
        if img < 0 or img >= n_img:
            raise ValueError("entry %d: image index %d is outside the %d images of the feature table" % (i, img, n_img))
        if img in bad:
            raise ValueError("entry %d: pos_boxes[%d] = %s is outside the feature table of %d rows" % (i, img, pos[img].tolist(), feats.shape[0]))
        image[i] = img
        qid[i] = int(e["question_id"])
        q_token[i] = _tokens(e["q_token"], "q_token", i, q0.shape)
    p.image, p.question_id, p.q_token = image, qid, q_token
    p.counts = np.minimum(pos[image, 1] - pos[image, 0], max_boxes).astype(np.int32)

    if p.kind == "mc":
        mc0, gt0 = _tokens(entries[0]["ans_mc_token"], "ans_mc_token", 0), _tokens(entries[0]["ans_gt_token"], "ans_gt_token", 0)
        l0 = _np(entries[0]["label"]).astype(np.float32)
        p.ans_mc, p.ans_gt = np.zeros((N,) + mc0.shape, np.int32), np.zeros((N,) + gt0.shape, np.int32)
        p.label = np.zeros((N,) + l0.shape, np.float32)
        for i, e in enumerate(entries):
            p.ans_mc[i] = _tokens(e["ans_mc_token"], "ans_mc_token", i, mc0.shape)
            p.ans_gt[i] = _tokens(e["ans_gt_token"], "ans_gt_token", i, gt0.shape)
            lab = _np(e["label"]).astype(np.float32)
            if lab.shape != l0.shape:
                raise ValueError("entry %d: label has shape %s, entry 0 has %s" % (i, lab.shape, l0.shape))
            p.label[i] = lab
        return p

    n = p.num_ans_candidates
    p.ans_token = None
    if "ans_token" in entries[0]:
        a0 = _tokens(entries[0]["ans_token"], "ans_token", 0)
        p.ans_token = np.zeros((N,) + a0.shape, np.int32)
    off = np.zeros(N + 1, np.int64)
    labels, scores = [], []
    teacher = None
    for i, e in enumerate(entries):
        if p.ans_token is not None:
            p.ans_token[i] = _tokens(e["ans_token"], "ans_token", i, p.ans_token.shape[1:])
        answer = e.get("answer")
        lab = None if answer is None else answer.get("labels")
        if lab is not None and len(lab):
            lab = _np(lab).astype(np.int64).reshape(-1)
            sc = _np(answer["scores"]).astype(np.float32).reshape(-1)
            if sc.shape != lab.shape:
                raise ValueError("entry %d: %d labels and %d scores" % (i, lab.size, sc.size))
            if lab.min() < 0 or lab.max() >= n:
                raise ValueError("entry %d: a label is outside the %d answer candidates" % (i, n))
            if np.unique(lab).size != lab.size:
                raise ValueError("entry %d: duplicate labels %s (the scatter of the target row would be undefined)" % (i, lab.tolist()))
            labels.append(lab.astype(np.int32))
            scores.append(sc)
            off[i + 1] = lab.size
        t = e.get("teacher_logit")
        if t is not None:
            t = _np(t)
            if t.shape != (n,):
                raise ValueError("entry %d: teacher_logit has shape %s, expected (%d,)" % (i, t.shape, n))
            h = t.astype(np.float16)
            if t.dtype != np.float16 and not np.array_equal(h.astype(np.float32), t.astype(np.float32), equal_nan=True):
                raise ValueError("entry %d: teacher_logit holds values that float16 does not hold exactly" % i)
            if teacher is None:
                teacher = np.zeros((N, n), np.float16)
            teacher[i] = h
    p.ans_off = np.cumsum(off)
    p.ans_labels = np.concatenate(labels) if labels else np.zeros(0, np.int32)
    p.ans_scores = np.concatenate(scores) if scores else np.zeros(0, np.float32)
    p.teacher = teacher
    return p


class DeviceDataset:
    """The tables of a PackedDataset on the device, uploaded once.

        ds = cti_amd.DeviceDataset(cti_amd.pack_dataset(dataset), device)            # feature_dtype=torch.bfloat16: the table is rounded at upload
        v, b, q, target, ans, question_id, teacher_logits = ds.assemble(idx)         # FFOE; MC: v, b, q, label, ans_mc, ans_gt
        ds.check()                                                                   # the one synchronisation: raises if an index was out of range

    `assemble(idx, pad_to=None, out=None, counts=None, mask=None)`: `idx` (B,) int64 entry numbers.  With `pad_to=None` the object dimension is the
    batch's largest count, as trim_collate makes it; the host has to know it, so `idx` is a CPU tensor (uploaded here).  With `pad_to` an int or 'max' (=
    min(max_boxes, the largest count in the table); checked against it when first used) every batch has the same shape and `idx` may live on the device:
    nothing is copied or synchronised.  `out` takes the tuple's tensors preallocated (GraphedTrainStep.static_in, say); `counts` (B,) int32 and `mask`
    (B, Vpad) uint8 (1 = padding row) are filled by the feature gather when given.  dtypes and order are the reference's.  An index out of range gives
    a zero sample and sets a sticky word that `check()` reports."""

    def __init__(self, packed, device="cuda", feature_dtype=torch.float32):
        if feature_dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("feature_dtype must be torch.float32 or torch.bfloat16, got %s" % (feature_dtype,))
        self.state = ops.batch_state(device)                 # refuses a CPU device
        self.device = dev = self.state.device
        self.packed, self.kind = packed, packed.kind
        self.n_answers, self.max_boxes = packed.num_ans_candidates, packed.max_boxes
        self.counts_host = packed.counts
        self.v_max = int(packed.counts.max())
        self._pads_checked = set()

        def up(a):
            return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)

        rows, d = packed.features.shape
        self.features = torch.empty(max(rows, 1), d, device=dev, dtype=feature_dtype)[:rows]
        step = max(1, (64 << 20) // max(4 * d, 1))            # rows per upload piece: the fp32 copy of a bf16 table never exists whole on the device
        for a in range(0, rows, step):
            self.features[a:a + step] = torch.from_numpy(packed.features[a:a + step]).to(dev)      # (bf16: round to nearest even in the copy)
        self.spatials, self.pos, self.image = up(packed.spatials), up(packed.pos), up(packed.image)
        self.q_token, self.question_id = up(packed.q_token), up(packed.question_id)
        if self.kind == "mc":
            self.label, self.ans_mc, self.ans_gt = up(packed.label), up(packed.ans_mc), up(packed.ans_gt)
        else:
            self.ans_token, self.teacher = up(packed.ans_token), up(packed.teacher)
            self.ans_off, self.ans_labels, self.ans_scores = up(packed.ans_off), up(packed.ans_labels), up(packed.ans_scores)

    def __len__(self):
        return len(self.packed)

    @property
    def positions(self):
        """How many tensors `assemble` returns."""
        return 6 if self.kind == "mc" or self.ans_token is None else 7

    def pad_for(self, pad_to, host_idx=None):
        """The object dimension of a batch: `pad_to` resolved ('max', an int, or None = the largest count among host_idx)."""
        if pad_to is None:
            if host_idx is None:
                raise ValueError("assemble: pad_to=None pads to the batch's largest object count, which the host must know: pass idx as a CPU tensor "
                                 "(or give pad_to='max' / an int)")
            h = np.asarray(host_idx).reshape(-1)
            h = h[(h >= 0) & (h < len(self))]                 # an index out of range is the device guard's to report
            return int(self.counts_host[h].max()) if h.size else 0
        if isinstance(pad_to, str):
            if pad_to != "max":
                raise ValueError("pad_to is %r, expected None, 'max' or an int" % (pad_to,))
            return self.v_max
        pad_to = int(pad_to)
        if pad_to not in self._pads_checked:
            if pad_to < self.v_max:
                raise ValueError("pad_to=%d is below the %d objects of the largest image (after the cut to max_boxes=%d)" % (pad_to, self.v_max, self.max_boxes))
            self._pads_checked.add(pad_to)
        return pad_to

    def assemble(self, idx, pad_to=None, out=None, counts=None, mask=None):
        if not isinstance(idx, torch.Tensor):
            idx = torch.as_tensor(np.asarray(idx), dtype=torch.int64)
        if idx.dtype != torch.int64 or idx.dim() != 1:
            raise TypeError("idx must be a (B,) int64 tensor, got %s %s" % (idx.dtype, tuple(idx.shape)))
        Vpad = self.pad_for(pad_to, None if idx.is_cuda else idx.numpy())
        if not idx.is_cuda:
            idx = idx.to(self.device)
        return self._assemble(idx.contiguous(), Vpad, out, counts, mask)

    def _assemble(self, idx, Vpad, out=None, counts=None, mask=None):
        n_out = self.positions
        o = [None] * n_out if out is None else list(out)
        if len(o) != n_out:
            raise ValueError("out must hold the %d tensors of the batch tuple, got %d" % (n_out, len(o)))
        st, B = self.state, idx.shape[0]
        if Vpad > 0:
            v = ops.batch_objects(self.features, self.image, self.pos, idx, self.max_boxes, Vpad, st, out=o[0], counts=counts, mask=mask)
            b = ops.batch_objects(self.spatials, self.image, self.pos, idx, self.max_boxes, Vpad, st, out=o[1])
        else:                                                # a batch of images without objects: trim_collate gives (B, 0, d)
            v = torch.empty(B, 0, self.features.shape[1], device=self.device, dtype=self.features.dtype)
            b = torch.empty(B, 0, self.spatials.shape[1], device=self.device)
        q = ops.batch_rows(self.q_token, idx, st, out=o[2])
        if self.kind == "mc":
            return (v, b, q, ops.batch_rows(self.label, idx, st, out=o[3]), ops.batch_rows(self.ans_mc, idx, st, out=o[4]),
                    ops.batch_rows(self.ans_gt, idx, st, out=o[5]))
        target = ops.batch_targets(self.ans_off, self.ans_labels, self.ans_scores, idx, self.n_answers, st, out=o[3])
        qid = ops.batch_rows(self.question_id, idx, st, out=o[-2])
        if self.teacher is not None:
            teacher = ops.batch_rows(self.teacher, idx, st, out=o[-1])
        elif o[-1] is not None:
            teacher = o[-1].zero_()
        else:
            teacher = torch.zeros(B, self.n_answers, device=self.device)
        if self.ans_token is None:
            return v, b, q, target, qid, teacher
        return v, b, q, target, ops.batch_rows(self.ans_token, idx, st, out=o[4]), qid, teacher

    def check(self):
        """Reads the sticky words (the only synchronisation of this class) and raises CtiError naming what was out of range."""
        bad = ops.batch_state_errors(self.state)
        if bad:
            raise L.CtiError("DeviceDataset: %s; those samples were written as zeros" % "; ".join(bad))

    def reset(self):
        self.state.zero_()


def epoch_order(N, shuffle=False, generator=None, rank=0, world=1):
    """The entry numbers one rank visits in one epoch, on the host: torch.randperm(N, generator=generator) when shuffling, else 0 .. N - 1; rank r of
    `world` takes every world-th one from r on, so the ranks partition the epoch."""
    if not 0 <= rank < world:
        raise ValueError("rank %d of world %d" % (rank, world))
    perm = torch.randperm(N, generator=generator) if shuffle else torch.arange(N)
    return perm[rank::world].contiguous()


def bucket_widths_for(counts, K):
    """K quantile widths of a table of object counts: the unique values of sorted(counts)[ceil((j + 1) * N / K) - 1], j = 0 .. K - 1, ascending.  The
    last one is counts.max(); fewer than K come back when the counts have fewer distinct values at those ranks."""
    K = int(K)
    if K < 1:
        raise ValueError("bucket_widths_for: K is %d" % K)
    c = np.sort(_np(counts).reshape(-1))
    N = c.size
    if N == 0:
        raise ValueError("bucket_widths_for: no counts")
    return tuple(int(w) for w in np.unique(c[[-(-(j + 1) * N // K) - 1 for j in range(K)]]))


def _widths(widths):
    w = np.asarray(list(widths), np.int64).reshape(-1)
    if w.size == 0 or w[0] < 0 or (np.diff(w) <= 0).any():
        raise ValueError("bucket widths must be strictly ascending and not negative, got %s" % (w.tolist(),))
    return w


def bucket_plan(order, counts, widths, batch_size, world=1, drop_last=False):
    """One epoch of batches grouped by object count, on the host, O(N).  `order` (int64) is the epoch's global entry order, `counts[e]` the object
    count of entry e, `widths` strictly ascending with widths[-1] >= counts.max().  With SB = batch_size * world:

      an entry's bucket is the smallest j with counts[e] <= widths[j];
      the buckets are walked in ascending order; the pool is the carry followed by the bucket's entries in the order they have in `order`; full
      groups of SB are cut from its front, each a batch of width widths[j]; the rest is the carry into the next bucket;
      after the last bucket a carry that is left is the one short group, as wide as its largest count asks for (dropped with drop_last).

    Returns (entries, batches): `entries` an int64 tensor, the epoch's entries group after group; `batches` a list of (lo, hi, width) over it.  Rank
    r of `world` takes entries[lo:hi][r::world] of every group (`rank_plan`), so all ranks see the same widths in the same order, which the one
    all-reduce per update needs.  With a single width this is order[r::world] cut by batch_size: the unbucketed loader."""
    batch_size, world = int(batch_size), int(world)
    if batch_size < 1 or world < 1:
        raise ValueError("bucket_plan: batch_size %d, world %d" % (batch_size, world))
    w = _widths(widths)
    order = _np(order).astype(np.int64).reshape(-1)
    c = _np(counts).reshape(-1)[order]
    if c.size and int(c.max()) > int(w[-1]):
        raise ValueError("bucket_plan: the last width %d is below the largest object count %d" % (int(w[-1]), int(c.max())))
    bucket = np.searchsorted(w, c, side="left")
    # the carry of a bucket goes in front of the next one, so the walk is a stable sort by bucket cut into groups of SB; a group cut at bucket j
    # holds at least one entry of j and none above it (the carry is shorter than SB), so its last entry names its width
    by_bucket = np.argsort(bucket, kind="stable")
    entries, bucket = order[by_bucket], bucket[by_bucket]
    SB = batch_size * world
    full = entries.size // SB
    end = full * SB if drop_last else entries.size
    batches = [(lo, min(lo + SB, end), int(w[bucket[min(lo + SB, end) - 1]])) for lo in range(0, end, SB)]
    return torch.from_numpy(np.ascontiguousarray(entries[:end])), batches


def rank_plan(entries, batches, rank=0, world=1):
    """What rank r of `world` visits of a bucket_plan: (its entries, its (lo, hi, width) list over them): every world-th entry of each group from r
    on.  A short group with no entry for this rank gives it no batch."""
    if not 0 <= rank < world:
        raise ValueError("rank %d of world %d" % (rank, world))
    mine, cuts, at = [], [], 0
    for lo, hi, width in batches:
        part = entries[lo:hi][rank::world]
        if len(part):
            mine.append(part)
            cuts.append((at, at + len(part), width))
            at += len(part)
    return (torch.cat(mine) if mine else entries[:0]).contiguous(), cuts


class DeviceLoader:
    """Stands where the reference builds `DataLoader(dataset, batch_size, shuffle=..., collate_fn=utils.trim_collate)`: iterable, with `len()` and
    `.dataset` (the ORIGINAL data set object: `len(loader.dataset)`, `num_ans_candidates`, `label2ans`), so `evaluate`, `predict` and the reference's
    loops take it as they take a DataLoader.

    One `torch.randperm(N, generator=generator)` per epoch on the host, uploaded once; the batches are slices of that device vector (rank r of `world`
    takes perm[r::world]: give every rank a generator in the same state), so with `pad_to` set there is no per-batch host-to-device copy and no per-batch synchronisation.  With `pad_to=None` the
    host looks up each batch's largest object count (no copy, no synchronisation either, but every batch has its own shape).

    `pad_to='bucket', bucket_widths=<ascending widths | K>` (K: `bucket_widths_for(counts, K)`, the K quantile widths of the table): once per epoch the
    same randperm is drawn, `bucket_plan` groups it by object count, and the reordered vector is uploaded once; every batch is a slice of it padded to
    its bucket's width, so a `Trainer(max_graphs=len(loader.widths))` replays one captured graph per width and no kernel walks the rows between a
    small image and the table's largest.  When shuffling, the full batches are visited in a second randperm's order (the widths interleave); the one
    short batch stays last.  Unshuffled: widths ascending, entries ascending within a bucket.  `loader.widths` are the resolved widths,
    `loader.plan_widths` the width of each batch of the last epoch started, `loader.plan_entries` that epoch's entry numbers in visiting order (host).
    Rank r takes every world-th entry of each GROUP of batch_size * world, so all ranks see the same widths in the same order; with drop_last the
    short group is dropped whole.

    The ORDER of a shuffled epoch is not that of torch's RandomSampler for the same seed: only the guarantees are the same (every entry once per
    epoch, a new order every epoch, reproducible from the generator's state)."""

    def __init__(self, ds, batch_size, shuffle=False, drop_last=False, pad_to=None, generator=None, rank=0, world=1, bucket_widths=None):
        if batch_size < 1:
            raise ValueError("batch_size is %d" % batch_size)
        if not 0 <= rank < world:
            raise ValueError("rank %d of world %d" % (rank, world))
        self.ds, self.batch_size, self.shuffle, self.drop_last, self.pad_to = ds, int(batch_size), bool(shuffle), bool(drop_last), pad_to
        self.generator, self.rank, self.world = generator, int(rank), int(world)
        self.dataset = ds.packed.dataset
        self.local = len(range(self.rank, len(ds), self.world))          # entries this rank visits per epoch
        self.bucketed = isinstance(pad_to, str) and pad_to == "bucket"
        self.widths, self.plan_widths, self.plan_entries = None, None, None
        if self.bucketed:
            if bucket_widths is None:
                raise ValueError("pad_to='bucket' needs bucket_widths: ascending widths, or the number of quantile widths to take from the table")
            if isinstance(bucket_widths, (int, np.integer)):
                bucket_widths = bucket_widths_for(ds.counts_host, bucket_widths)
            self.widths = tuple(int(w) for w in _widths(bucket_widths))
            if self.widths[-1] < ds.v_max:
                raise ValueError("bucket_widths end at %d, below the %d objects of the largest image (after the cut to max_boxes=%d)"
                                 % (self.widths[-1], ds.v_max, ds.max_boxes))
        elif bucket_widths is not None:
            raise ValueError("bucket_widths belongs to pad_to='bucket', pad_to is %r" % (pad_to,))

    def __len__(self):
        if self.bucketed:                                    # full groups of batch_size * world, then this rank's share of the short one
            m, t = divmod(len(self.ds), self.batch_size * self.world)
            return m if self.drop_last else m + (t > self.rank)
        return self.local // self.batch_size if self.drop_last else (self.local + self.batch_size - 1) // self.batch_size

    def epoch_order(self):
        return epoch_order(len(self.ds), self.shuffle, self.generator, self.rank, self.world)

    def bucket_epoch(self):
        """This rank's plan of one bucketed epoch, on the host: (entries in visiting order, [(lo, hi, width)] over them).  Draws from the generator
        what one epoch draws."""
        N = len(self.ds)
        order = epoch_order(N, self.shuffle, self.generator)
        entries, batches = bucket_plan(order, self.ds.counts_host, self.widths, self.batch_size, self.world, self.drop_last)
        SB = self.batch_size * self.world
        full = [g for g in batches if g[1] - g[0] == SB]
        if self.shuffle and full:
            full = [full[k] for k in torch.randperm(len(full), generator=self.generator).tolist()]
        batches = full + batches[len(full):]
        entries = torch.cat([entries[lo:hi] for lo, hi, _ in batches]) if batches else entries
        at, cuts = 0, []
        for lo, hi, width in batches:
            cuts.append((at, at + hi - lo, width))
            at += hi - lo
        return rank_plan(entries, cuts, self.rank, self.world)

    def __iter__(self):
        if self.bucketed:
            host, cuts = self.bucket_epoch()
            self.plan_entries, self.plan_widths = host, [width for _, _, width in cuts]
            dev = host.to(self.ds.device)
            for lo, hi, width in cuts:
                yield self.ds._assemble(dev[lo:hi], width)
            return
        host = self.epoch_order()
        dev = host.to(self.ds.device)
        bs = self.batch_size
        fixed = None if self.pad_to is None else self.ds.pad_for(self.pad_to)
        for k in range(len(self)):
            lo, hi = k * bs, min((k + 1) * bs, self.local)
            Vpad = fixed if fixed is not None else self.ds.pad_for(None, host[lo:hi].numpy())
            yield self.ds._assemble(dev[lo:hi], Vpad)
