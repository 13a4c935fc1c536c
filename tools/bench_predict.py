#!/usr/bin/env python3
"""A test pass through PredictionBuffer (csrc/cti_predict.hip: one launch per batch + a one-thread cursor update, one synchronisation and one copy at
the end) beside the reference's form of the same pass (src/FFOE/test.py:78-130): `pred[idx:idx+B].copy_(logits)` into a host tensor per batch, then
one host arg-max and one `np.float16` per question.  The workload's own shape: batches of 256 x 3129 logits, a few hundred of them; the logits
come from a small pool of device tensors standing in for the model's output, so both sides move the same data and neither pays for a model.

    hip_pass_ms       host clock: every append, then result() (the synchronisation and the copies of answers, ids and float16 rows)
    hip_append_us     device events around the appends alone, per batch (host issue cost included, as in a loop)
    ref_copy_ms       host clock: the reference's per-batch copies of logits and question ids
    ref_host_ms       host clock: its per-question arg-max and float16 conversion
The yardstick is the restatement, never an earlier run of this package.  The pass runs in a child process under a time limit.  One JSON record:

    python tools/bench_predict.py [batches] [--out profiles/predict_bench.json]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N_ANS = 256, 3129
STEP_TIMEOUT = 540


def ref_pass(batches, qid_batches, device_sync):
    """get_logits + make_json + make_json_with_logits of the reference, on the same tensors."""
    n = len(batches) * B
    t0 = time.perf_counter()
    pred = torch.FloatTensor(n, N_ANS).zero_()
    qids = torch.IntTensor(n).zero_()
    idx = 0
    for logits, i in zip(batches, qid_batches):
        pred[idx:idx + B, :].copy_(logits.data)
        qids[idx:idx + B].copy_(i)
        idx += B
    device_sync()
    t1 = time.perf_counter()
    answers = np.empty(n, np.int64)
    half = {}
    for r in range(n):
        answers[r] = pred[r].max(0)[1].item()
        half[int(qids[r])] = np.float16(pred[r].detach().numpy())
    t2 = time.perf_counter()
    return answers, qids.numpy(), half, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def one_pass(n_batches):
    sys.path.insert(0, ROOT)
    import cti_amd
    torch.manual_seed(0)
    dev = "cuda"
    pool = [3.0 * torch.randn(B, N_ANS, device=dev) for _ in range(4)]
    batches = [pool[k % 4] for k in range(n_batches)]
    qid_cpu = [torch.arange(k * B, (k + 1) * B, dtype=torch.int32) + 262148000 for k in range(n_batches)]       # what a DataLoader yields
    n = n_batches * B
    buf = cti_amd.PredictionBuffer(n, N_ANS, dev)

    def hip_pass():
        buf.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for logits, i in zip(batches, qid_cpu):
            buf.append(logits, i)
        e1.record()
        p = buf.result()
        t1 = time.perf_counter()
        return p, (t1 - t0) * 1e3, e0.elapsed_time(e1) * 1e3 / n_batches

    hip_pass()                                                              # warm-up: code objects, the pinned staging of the copies
    runs = [hip_pass() for _ in range(3)]
    ref_pass(batches[:4], qid_cpu[:4], torch.cuda.synchronize)
    answers, qids, half, ref_copy_ms, ref_host_ms = ref_pass(batches, qid_cpu, torch.cuda.synchronize)
    p, _, _ = hip_pass()                                                    # again behind the restatement: the spread of this measurement
    same = bool(np.array_equal(p.answers, answers) and np.array_equal(p.question_ids, qids.astype(np.int64)) and
                all(np.array_equal(p.logits[r].view(np.uint16), half[int(qids[r])].view(np.uint16)) for r in range(0, n, 97)))
    hip_ms = [round(r[1], 2) for r in runs]
    return dict(op="PredictionBuffer pass", batches=n_batches, rows=B, n=N_ANS, hip_pass_ms=min(hip_ms), hip_pass_ms_runs=hip_ms,
                hip_append_us=round(min(r[2] for r in runs), 2), ref_copy_ms=round(ref_copy_ms, 2), ref_host_ms=round(ref_host_ms, 2),
                ref_pass_ms=round(ref_copy_ms + ref_host_ms, 2), results_agree=same)


def main(argv):
    out = os.path.join(ROOT, "profiles", "predict_bench.json")
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    n_batches = int(argv[0]) if argv else 200
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n_batches)], stdout=subprocess.PIPE, text=True, timeout=STEP_TIMEOUT)
    if r.returncode != 0:
        print("bench_predict: the pass ended with status %d" % r.returncode, file=sys.stderr)
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
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print(json.dumps(one_pass(int(sys.argv[2]))), flush=True)
        sys.exit(0)
    sys.exit(main(sys.argv[1:]))
