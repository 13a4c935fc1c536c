#!/usr/bin/env python3
"""Batches assembled on the device (batch.py, csrc/cti_batch.hip: DeviceLoader over a resident DeviceDataset) beside the reference's form of the same
input path: `Dataset.__getitem__` per question (slices through pos_boxes, the cut to max_boxes, `scatter_` into a zeroed row, the float16 teacher row
widened), stack-and-pad on the host as utils.trim_collate does, then `.to(device)` from pageable memory -- restated here, in this file.  The
workload's own shape: B = 256, 3129 answers, 2048-wide fp32 features, in two forms: `fixed` (a non-adaptive table, 36 objects per image) and
`adaptive` (10 .. 100 objects per image, every batch padded to the table's largest count with pad_to='max').

    hip_pass_ms / ref_pass_ms     host clock over `batches` batches, the final synchronisation included; three runs each, all recorded
    hip_batch_us / ref_batch_us   device events around the same loop, per batch
    objects_us / copy_us          kernel (a) alone (the feature gather of one batch) against torch's `copy_` of ONE contiguous tensor of the batch's byte
                                  count, cold: both rotate enough operand sets that their total exceeds the 256 MiB Infinity Cache; three runs each
    objects_over_copy             min over min of the two; copy_spread = (max - min) / min of the copy's three runs
Every tensor of a sample of batches is compared between the two forms for equality (`batches_agree`).  The yardsticks are the restatement and the
copy, measured in the same process, never an earlier run of this package.  The pass runs in a child process under a time limit.  One JSON record:

    python tools/bench_batch.py [batches] [--out profiles/batch_bench.json]"""
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N_ANS, D, LQ, LA = 256, 3129, 2048, 14, 3
EPOCH_BATCHES = 25                                     # entries in the synthetic data set: 25 batches' worth; a pass walks it as often as it needs
STEP_TIMEOUT = 1100


def synth(form, seed):
    """A reference-shaped data set object (what tensorize() leaves): torch tables, entries as dicts of tensors."""
    rs = np.random.RandomState(seed)
    n_img = 1500
    ds = types.SimpleNamespace(num_ans_candidates=N_ANS, max_boxes=100)
    if form == "fixed":
        ds.adaptive = False
        ds.features = torch.from_numpy(rs.standard_normal((n_img, 36, D)).astype(np.float32))
        ds.spatials = torch.from_numpy(rs.uniform(size=(n_img, 36, 6)).astype(np.float32))
    else:
        ds.adaptive = True
        counts = rs.randint(10, 101, n_img)
        counts[:2] = (10, 100)
        ends = np.cumsum(counts)
        ds.pos_boxes = np.stack([ends - counts, ends], 1)
        ds.features = torch.from_numpy(rs.standard_normal((int(ends[-1]), D)).astype(np.float32))
        ds.spatials = torch.from_numpy(rs.uniform(size=(int(ends[-1]), 6)).astype(np.float32))
    N = EPOCH_BATCHES * B
    teacher = rs.standard_normal((N, N_ANS)).astype(np.float16)
    ds.entries = []
    for k in range(N):
        lab = rs.choice(N_ANS, size=1 + k % 10, replace=False)
        ds.entries.append({"image": int(rs.randint(n_img)), "question_id": 262148000 + k, "q_token": torch.from_numpy(rs.randint(0, 20000, LQ)),
                           "ans_token": torch.from_numpy(rs.randint(0, 20000, LA)),
                           "answer": {"labels": torch.from_numpy(lab), "scores": torch.from_numpy((rs.randint(1, 11, len(lab)) / 10.0).astype(np.float32))},
                           "teacher_logit": teacher[k]})
    return ds


def ref_item(ds, index):
    """src/FFOE/dataset.py:350-376 (the adaptive form) and src/MC/dataset.py:248-250 (a non-adaptive table is indexed whole), restated."""
    e = ds.entries[index]
    if ds.adaptive:
        s, t = ds.pos_boxes[e["image"]]
        features, spatials = ds.features[s:t, :][:ds.max_boxes], ds.spatials[s:t, :][:ds.max_boxes]
    else:
        features, spatials = ds.features[e["image"]], ds.spatials[e["image"]]
    teacher = torch.from_numpy(np.float32(e["teacher_logit"]))
    target = torch.zeros(ds.num_ans_candidates)
    if e["answer"]["labels"] is not None:
        target.scatter_(0, e["answer"]["labels"], e["answer"]["scores"])
    return features, spatials, e["q_token"], target, e["ans_token"], e["question_id"], teacher


def ref_collate(items):
    """src/utils.py:120-169 restated: images zero-padded to the batch's largest object count and stacked, the rest stacked, ints to a LongTensor."""
    out = []
    for col in zip(*items):
        if torch.is_tensor(col[0]) and col[0].dim() > 1:
            most = max(x.size(0) for x in col)
            out.append(torch.stack([F.pad(x, (0, 0, 0, most - x.size(0))) for x in col], 0))
        elif torch.is_tensor(col[0]):
            out.append(torch.stack(col, 0))
        else:
            out.append(torch.LongTensor(col))
    return out


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    last = fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1), last


def one_form(form, n_batches, cti_amd):
    dev = "cuda"
    host_ds = synth(form, 1800 + len(form))
    packed = cti_amd.pack_dataset(host_ds)
    ds = cti_amd.DeviceDataset(packed, dev)
    N = len(packed)
    Vpad = ds.pad_for("max")
    orders = [torch.randperm(N, generator=torch.Generator().manual_seed(40 + k)) for k in range((n_batches + EPOCH_BATCHES - 1) // EPOCH_BATCHES)]
    cuts = [(o, lo) for o in orders for lo in range(0, N, B)][:n_batches]

    def hip_pass():
        last = None
        dev_orders = {id(o): o.to(dev) for o in orders}                     # one upload per epoch
        for o, lo in cuts:
            last = ds.assemble(dev_orders[id(o)][lo:lo + B], pad_to="max")
        return last

    def ref_pass():
        last = None
        for o, lo in cuts:
            last = [t.to(dev) for t in ref_collate([ref_item(host_ds, int(i)) for i in o[lo:lo + B]])]
        return last

    timed(lambda: [ds.assemble(orders[0][:B].to(dev), pad_to="max") for _ in range(3)])      # warm-up: code objects, the allocator
    hip = [timed(hip_pass)[:2] for _ in range(3)]
    print("bench_batch: %s, this path %s ms" % (form, [round(h[0], 1) for h in hip]), file=sys.stderr, flush=True)
    ref = []
    for _ in range(3):
        ref.append(timed(ref_pass)[:2])
        print("bench_batch: %s, the reference's form %.1f ms" % (form, ref[-1][0]), file=sys.stderr, flush=True)
    ds.check()

    agree = True
    for o, lo in cuts[::max(1, n_batches // 5)]:                            # a sample of batches, every tensor
        idx = o[lo:lo + B]
        mine = ds.assemble(idx.to(dev), pad_to="max")
        theirs = [t.to(dev) for t in ref_collate([ref_item(host_ds, int(i)) for i in idx])]
        vb = theirs[0].shape[1]
        for j, (m, t) in enumerate(zip(mine, theirs)):
            if j < 2:                                                       # the reference pads to the batch's largest count, this path to the table's
                agree = agree and torch.equal(m[:, :vb], t) and not bool(m[:, vb:].any())
            else:
                agree = agree and m.dtype == t.dtype and torch.equal(m, t)

    # kernel (a) alone against a same-bytes copy_, cold: rotate operand sets past the Infinity Cache
    nbytes = B * Vpad * D * 4
    sets = max(2, (300 << 20) // nbytes + 1)
    outs = [torch.empty(B, Vpad, D, device=dev) for _ in range(sets)]
    srcs = [torch.randn(B, Vpad, D, device=dev) for _ in range(sets)]
    idxs = [orders[0][k * B:(k + 1) * B].to(dev) for k in range(sets)]
    ops, reps = cti_amd.ops, 4 * sets

    def objects():
        for r in range(reps):
            ops.batch_objects(ds.features, ds.image, ds.pos, idxs[r % sets], ds.max_boxes, Vpad, ds.state, out=outs[r % sets])

    def copies():
        for r in range(reps):
            outs[r % sets].copy_(srcs[r % sets])

    timed(objects), timed(copies)
    obj_us = [round(timed(objects)[1] * 1e3 / reps, 2) for _ in range(3)]
    cp_us = [round(timed(copies)[1] * 1e3 / reps, 2) for _ in range(3)]
    copied = int(packed.counts[orders[0][:sets * B].numpy()].sum()) * D * 4 // sets          # bytes kernel (a) READS per batch; it writes nbytes
    r3 = lambda xs: [round(x, 2) for x in xs]                               # noqa: E731
    return dict(form=form, batches=n_batches, B=B, Vpad=Vpad, batch_feature_mb=round(nbytes / 1e6, 1),
                hip_pass_ms_runs=r3(h[0] for h in hip), ref_pass_ms_runs=r3(r[0] for r in ref),
                hip_batch_us_runs=r3(h[1] * 1e3 / n_batches for h in hip), ref_batch_us_runs=r3(r[1] * 1e3 / n_batches for r in ref),
                ref_over_hip=round(min(r[0] for r in ref) / min(h[0] for h in hip), 1), batches_agree=bool(agree),
                operand_sets=sets, objects_us_runs=obj_us, copy_us_runs=cp_us, objects_read_mb=round(copied / 1e6, 1),
                objects_over_copy=round(min(obj_us) / min(cp_us), 3), copy_spread=round((max(cp_us) - min(cp_us)) / min(cp_us), 3),
                objects_tb_s=round((copied + nbytes) / min(obj_us) / 1e6, 2), copy_tb_s=round(2 * nbytes / min(cp_us) / 1e6, 2))


def one_pass(n_batches):
    sys.path.insert(0, ROOT)
    import cti_amd
    return dict(op="DeviceLoader pass", n=N_ANS, d=D, forms=[one_form(f, n_batches, cti_amd) for f in ("fixed", "adaptive")])


def main(argv):
    out = os.path.join(ROOT, "profiles", "batch_bench.json")
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    n_batches = int(argv[0]) if argv else 200
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n_batches)], stdout=subprocess.PIPE, text=True, timeout=STEP_TIMEOUT)
    if r.returncode != 0:
        print("bench_batch: the pass ended with status %d" % r.returncode, file=sys.stderr)
        return 1
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    import numpy as np
    import torch
    import torch.nn.functional as F
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print(json.dumps(one_pass(int(sys.argv[2]))), flush=True)
        sys.exit(0)
    sys.exit(main(sys.argv[1:]))
