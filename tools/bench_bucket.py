#!/usr/bin/env python3
"""One training epoch over adaptive features, padded two ways (batch.py, trainer.py), at the reference's widths as tools/bench_model.py builds them
(FFOE CTI and FFOE BAN, B = 256, 3129 answers, 2048-wide fp32 features):

    a   DeviceLoader(pad_to='max') + Trainer(): every batch padded to the table's largest object count, ONE captured micro-step
    b   DeviceLoader(pad_to='bucket', bucket_widths=6) + Trainer(max_graphs=6): the same entries grouped by object count, one captured micro-step
        per width

The store is synthetic: `IMAGES` images with 10 + (37 * i) % 91 objects (uniform on 10 .. 100), entry k looks at image k % IMAGES, `EPOCH_BATCHES`
batches per epoch, shuffled, every batch an update.  Each model runs twice: with the store cut at about the most objects its training kernels take
at these widths (CTI 60: the M build of csrc/cti_mbuild.hip holds up to 61 objects in LDS beside 14 question tokens; BAN 64: the logits' backward of
csrc/cti_backward2.hip up to 66; at 100 both refuse), and at the reference's default max_boxes = 50, where more than half the images sit at the cut.
Both cases run in one process on models with the same initial parameters; after the warm-up epochs (until every width is captured, then one more) the timed epochs ALTERNATE a, b, a, b, ..., so a drift of the machine falls on both.  Per case:

    rows                  object rows the epoch's batches hold (exact: sum of batch size x width)
    epoch_ms_runs         host clock around one epoch (the loader's plan and upload, every train_step, the final synchronisation), each timed epoch
    epoch_ms / update_ms  their median, and the median per update; spread = (max - min) / median
    captures, widths      graphs captured, and the widths of the last epoch's batches
    reserved_mb           torch.cuda.memory_reserved() when the case's captures are done (case a is set up first; b's figure includes a's, and
                          both what the run held before its first case: `reserved_mb_at_start`)
`b_over_a` is the ratio of the medians, `rows_b_over_a` the ratio of the rows.  `--cases a` runs the baseline alone (it needs nothing newer than
DeviceLoader(pad_to='max') and Trainer).

    python tools/bench_bucket.py [ffoe_cti ffoe_ban] [--max-boxes M] [--epochs 5] [--cases a,b] [--out profiles/bucket_bench.json]"""
import gc
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_model as bm  # noqa: E402  (puts the package's root on sys.path and imports cti_amd)

cti_amd = bm.cti_amd
DEV = "cuda"
B, D, NTOKEN, IMAGES, EPOCH_BATCHES, K = 256, 2048, 20000, 182, 48, 6
MAX_WARMUP_EPOCHS = 6
MOST_OBJECTS = {"ffoe_cti": 60, "ffoe_ban": 64}             # about what the model's training kernels take at these widths


def synth(num_ans, Q, A, max_boxes, seed=1900):
    """A reference-shaped adaptive data set object (what tensorize() leaves)."""
    rs = np.random.RandomState(seed)
    counts = 10 + (37 * np.arange(IMAGES)) % 91
    ends = np.cumsum(counts)
    ds = types.SimpleNamespace(num_ans_candidates=num_ans, max_boxes=max_boxes, adaptive=True, pos_boxes=np.stack([ends - counts, ends], 1))
    ds.features = torch.from_numpy(np.abs(rs.standard_normal((int(ends[-1]), D))).astype(np.float32))
    ds.spatials = torch.from_numpy(rs.uniform(size=(int(ends[-1]), 6)).astype(np.float32))
    N = EPOCH_BATCHES * B
    ds.entries = []
    for k in range(N):
        lab = rs.choice(num_ans, size=1 + k % 10, replace=False)
        ds.entries.append({"image": k % IMAGES, "question_id": 262148000 + k, "q_token": torch.from_numpy(rs.randint(0, NTOKEN, Q)),
                           "ans_token": torch.from_numpy(rs.randint(0, NTOKEN, max(A, 1))),
                           "answer": {"labels": torch.from_numpy(lab), "scores": torch.from_numpy((rs.randint(1, 11, len(lab)) / 10.0).astype(np.float32))}})
    return ds


class Case:
    def __init__(self, which, name, ds, state):
        builder, gamma, num_ans, Q, A = bm.CASES[name]
        self.which = which
        m = getattr(cti_amd, builder)(bm.args_of(gamma), bm.DS(NTOKEN, D, num_ans)).to(DEV)
        m.load_state_dict(state)
        args = types.SimpleNamespace(device=DEV, model=name.split("_")[1], distillation=False, clip_norm=0.25, gamma=gamma, lr=1e-3)
        g = torch.Generator().manual_seed(77)
        if which == "a":
            self.loader = cti_amd.DeviceLoader(ds, B, shuffle=True, generator=g, pad_to="max")
            self.trainer = cti_amd.Trainer(args, m.train(), cti_amd.BCEWithLogitsSum())
            self.want = 1
        else:
            self.loader = cti_amd.DeviceLoader(ds, B, shuffle=True, generator=g, pad_to="bucket", bucket_widths=K)
            self.trainer = cti_amd.Trainer(args, m.train(), cti_amd.BCEWithLogitsSum(), max_graphs=len(self.loader.widths))
            self.want = len(self.loader.widths)
        self.rows, self.widths, self.runs = 0, [], []

    def epoch(self):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows, widths, loss = 0, [], None
        for v, b, q, a, ans, _, t_logits in self.loader:
            loss = self.trainer.train_step([v, b, q, a, ans, t_logits], update_params=True)[0]
            rows += v.shape[0] * v.shape[1]
            widths.append(v.shape[1])
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if not bool(torch.isfinite(loss)):
            raise RuntimeError("bench_bucket: case %s left a loss that is not finite" % self.which)
        self.rows, self.widths = rows, widths
        return ms

    def warm(self):
        """Epochs until every width of the plan is captured, then one more; returns how many that took."""
        for n in range(1, MAX_WARMUP_EPOCHS + 1):
            self.epoch()
            if self.trainer.captures >= self.want:
                self.epoch()
                self.reserved = torch.cuda.memory_reserved()
                return n + 1
        raise RuntimeError("bench_bucket: case %s captured %d of %d graphs in %d epochs" % (self.which, self.trainer.captures, self.want, MAX_WARMUP_EPOCHS))

    def record(self, warm_epochs):
        med = statistics.median(self.runs)
        return dict(case=self.which, rows=self.rows, updates=len(self.widths), epoch_ms_runs=[round(x, 2) for x in self.runs], epoch_ms=round(med, 2),
                    update_ms=round(med / len(self.widths), 3), spread=round((max(self.runs) - min(self.runs)) / med, 3),
                    captures=self.trainer.captures, widths=self.widths, warmup_epochs=warm_epochs, reserved_mb=round(self.reserved / 2 ** 20, 1))


def one_model(name, max_boxes, which, epochs):
    builder, gamma, num_ans, Q, A = bm.CASES[name]
    gc.collect()
    torch.cuda.empty_cache()                                                # what an earlier run's graphs and models held
    at_start = torch.cuda.memory_reserved()
    host = synth(num_ans, Q, A, max_boxes)
    packed = cti_amd.pack_dataset(host)
    ds = cti_amd.DeviceDataset(packed, DEV)
    torch.manual_seed(1204)
    state = getattr(cti_amd, builder)(bm.args_of(gamma), bm.DS(NTOKEN, D, num_ans)).state_dict()
    cases, warm = [], {}
    for w in which:                                                         # a first: its reserved memory is its own
        c = Case(w, name, ds, state)
        warm[w] = c.warm()
        cases.append(c)
        print("bench_bucket: %s, max_boxes %d, case %s warm after %d epochs, %d captures" % (name, max_boxes, w, warm[w], c.trainer.captures), file=sys.stderr, flush=True)
    for _ in range(epochs):
        for c in cases:                                                     # alternating
            c.runs.append(c.epoch())
    ds.check()
    out = dict(model=name, max_boxes=max_boxes, B=B, entries=len(packed), real_rows=int(packed.counts.sum()), precision=cti_amd.get_precision(),
               reserved_mb_at_start=round(at_start / 2 ** 20, 1), cases=[c.record(warm[c.which]) for c in cases])
    if len(cases) == 2:
        out["b_over_a"] = round(cases[1].record(0)["epoch_ms"] / cases[0].record(0)["epoch_ms"], 3)
        out["rows_b_over_a"] = round(cases[1].rows / cases[0].rows, 3)
    return out


def main(argv):
    def opt(flag, default):
        return argv[argv.index(flag) + 1] if flag in argv else default

    names = [x for x in argv if x in MOST_OBJECTS] or ["ffoe_ban", "ffoe_cti"]
    epochs, which = int(opt("--epochs", 5)), opt("--cases", "a,b").split(",")
    out = opt("--out", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bucket_bench.json"))
    if epochs < 3 or not set(which) <= {"a", "b"}:
        raise SystemExit("bench_bucket: at least three timed epochs, cases out of a,b")
    if not torch.cuda.is_available():
        raise SystemExit("bench_bucket: needs an MI355X")
    cuts = [int(opt("--max-boxes", 0))] if "--max-boxes" in argv else None
    runs = [one_model(n, mb, sorted(which), epochs) for n in names for mb in (cuts or [MOST_OBJECTS[n], 50])]
    line = json.dumps(dict(op="bucketed epoch", epoch_batches=EPOCH_BATCHES, timed_epochs=epochs, runs=runs))
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
