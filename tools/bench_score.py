#!/usr/bin/env python3
"""ScoreMeter.update / update_mc (csrc/cti_score.hip: one scoring launch + one single-workgroup accumulation) beside a torch restatement of what
the reference's loops do with the same tensors (src/FFOE/train.py:16-21,142-144; src/MC/train.py:14-19,154-156), at the shapes a user runs:
FFOE 256 x 3129 and 1024 x 3129 (batch x answer candidates), MC 1024 x 2 (256 questions x 4 candidate answers).

Per call: events around `reps` back-to-back calls after a warm-up, everything else preallocated -- host issue cost included, as it is in a
training loop.  `torch_us` is the reference's score function and the `.sum()` its callers take; `torch_loop_us` adds the upper bound and the
two running sums of the evaluation loop, which is what one `update` replaces.  The yardstick is the restatement, never an earlier run of this
package.  Each shape runs in a child process of its own under a time limit; the first failure ends the run.  One JSON record per shape:

    python tools/bench_score.py [reps] [--out profiles/score_bench.jsonl]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("ffoe", 256, 3129), ("ffoe", 1024, 3129), ("mc", 1024, 2))
STEP_TIMEOUT = 240


def torch_score_ffoe(logits, labels):
    pred = logits.max(1)[1]
    one_hots = torch.zeros(*labels.size(), device=logits.device)
    one_hots.scatter_(1, pred.view(-1, 1), 1)
    return one_hots * labels


def torch_score_mc(logits, labels):
    prob = torch.softmax(logits, 1)
    picks = [prob[4 * g:4 * g + 4, 0].max(0)[1] + 4 * g for g in range(logits.size(0) // 4)]
    return labels[:, 0].gather(0, torch.stack(picks))


def timeit(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3       # us


def one_shape(rule, rows, n, reps):
    sys.path.insert(0, ROOT)
    import cti_amd
    torch.manual_seed(0)
    dev = "cuda"
    logits = 3.0 * torch.randn(rows, n, device=dev)
    if rule == "ffoe":
        labels = (torch.rand(rows, n, device=dev) < 0.003).float() * torch.rand(rows, n, device=dev)
        score_fn = torch_score_ffoe
        meter = cti_amd.ScoreMeter(dev)
        update = meter.update
        upper_labels = labels
    else:
        a = torch.zeros(rows // 4, 4, device=dev)
        a[torch.arange(rows // 4), torch.randint(0, 4, (rows // 4,))] = 1.0
        a = a.view(rows, 1)
        labels = torch.cat([a, 1 - a], 1)
        score_fn = torch_score_mc
        meter = cti_amd.ScoreMeter(dev)
        update = meter.update_mc
        upper_labels = a
    acc = {"score": torch.zeros((), device=dev), "upper": torch.zeros((), device=dev)}

    def ref_score():
        return score_fn(logits, labels).sum()

    def ref_loop():
        acc["score"] += score_fn(logits, labels).sum()
        acc["upper"] += upper_labels.max(1)[0].sum()

    reps_ref = reps if rule == "ffoe" else max(10, reps // 10)     # the MC restatement issues ~3 torch kernels per GROUP
    hip_us = timeit(lambda: update(logits, labels), reps)
    torch_us = timeit(ref_score, reps_ref)
    torch_loop_us = timeit(ref_loop, reps_ref)
    hip_us2 = timeit(lambda: update(logits, labels), reps)         # again behind the restatement: the spread of this measurement
    meter.reset(); acc["score"].zero_(); acc["upper"].zero_()
    update(logits, labels); ref_loop()
    r = meter.result()
    same = abs(r["score"] - float(acc["score"])) <= 1e-5 * max(1.0, r["score"]) and abs(r["upper_bound"] - float(acc["upper"])) <= 1e-5 * max(1.0, r["upper_bound"])
    return dict(op="ScoreMeter.update" if rule == "ffoe" else "ScoreMeter.update_mc", rows=rows, n=n, hip_us=round(min(hip_us, hip_us2), 2),
                hip_us_runs=[round(hip_us, 2), round(hip_us2, 2)], torch_us=round(torch_us, 2), torch_loop_us=round(torch_loop_us, 2),
                not_slower_than_torch=bool(max(hip_us, hip_us2) <= torch_us), sums_agree=bool(same), reps=reps, reps_torch=reps_ref)


def main(argv):
    out = os.path.join(ROOT, "profiles", "score_bench.jsonl")
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    reps = int(argv[0]) if argv else 200
    records = []
    for rule, rows, n in SHAPES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", rule, str(rows), str(n), str(reps)], stdout=subprocess.PIPE, text=True,
                           timeout=STEP_TIMEOUT)
        if r.returncode != 0:
            print("bench_score: %s %d x %d ended with status %d; stopping" % (rule, rows, n, r.returncode), file=sys.stderr)
            return 1
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        records.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(records) + "\n")
    return 0


if __name__ == "__main__":
    import torch
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print(json.dumps(one_shape(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))), flush=True)
        sys.exit(0)
    sys.exit(main(sys.argv[1:]))
