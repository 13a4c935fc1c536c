"""A/B of the mode-3 tile plan (cti_set_tuning key CTI_TUNE_MODE3_SKIP_PADDED) on the BASELINE configs[1] forward, key on vs key 0, alternating in one process.

  python tools/ab_mode3_skip.py                 `v` WITHOUT a zero object: nothing to skip -- what the mask, the plan kernel and the table look-ups cost
  python tools/ab_mode3_skip.py --padded        the benchmark's seeded inputs (nv ~ U[10, 36]): what the skipped tiles save

Prints one JSON line: per key the ms per step of every round, their median and spread, and the plan's totals of the last step with the key on."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench          # noqa: E402
import cti_amd        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--padded", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    ops = cti_amd.ops
    dev = torch.device("cuda:0")
    cti_amd.set_precision("f16f6")
    c = bench.C2
    torch.manual_seed(bench.SEED)
    net = cti_amd.TCNet(c["v_dim"], c["q_dim"], c["a_dim"], c["h_mm"], 1, c["rank"], c["glimpse"]).to(dev).eval()
    v, q, a = bench.synth_inputs(c, c["B"], bench.SEED + 1, dev)
    if not args.padded:
        v = v + (v == 0).all(dim=2, keepdim=True) * 0.5          # every padded object becomes a live one
    ms = {0: [], 1: []}
    plan = None
    with torch.no_grad():
        for rnd in range(args.rounds):
            for key in ((1, 0) if rnd % 2 == 0 else (0, 1)):
                with ops.tuning(mode3_skip_padded=key):
                    for _ in range(args.warmup):
                        net(v, q, a)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        net(v, q, a)
                    torch.cuda.synchronize()
                    ms[key].append((time.perf_counter() - t0) / args.steps * 1e3)
                    if key == 1:
                        ops._debug_keep_mode3_plan = True
                        net(v, q, a)
                        torch.cuda.synchronize()
                        plan = ops.last_mode3_plan()
                        ops._debug_keep_mode3_plan = False
    rec = {"inputs": "bench.synth_inputs(SEED + 1)" + ("" if args.padded else ", no zero object"), "steps": args.steps, "rounds": args.rounds, "plan_key_on": plan}
    for key in (0, 1):
        x = np.array(ms[key])
        rec["key_%d" % key] = {"ms_per_step": [round(float(t), 4) for t in x], "median": round(float(np.median(x)), 4), "spread": round(float(x.max() - x.min()), 4)}
    rec["median_on_minus_off_ms"] = round(rec["key_1"]["median"] - rec["key_0"]["median"], 4)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
