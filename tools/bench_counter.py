#!/usr/bin/env python3
"""cti_counter_fwd / cti_counter_bwd alone (csrc/cti_counter.hip) at the BAN models' shape: rows = 256 samples x 8 glimpses, a (B, G, V, Q) logit
block with Q = 14, objects = 10, V = 36 and V = 100.  Events around `reps` back-to-back launches on preallocated buffers (no allocation, no
reduction of the weight partials inside the timed region); the operands are a few MB and stay cache-resident between launches, as they are in
a model forward, where the attention kernel has just written the logits.  One JSON line per (kernel, V).

    python tools/bench_counter.py [reps]"""
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cti_amd  # noqa: E402
from cti_amd import ops  # noqa: E402

DEV = "cuda"
L = cti_amd.pkg._lib


def timeit(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3       # us


def main(reps=50):
    torch.manual_seed(0)
    B, G, Q, m = 256, 8, 14, 10
    lib = L.lib()
    c = cti_amd.Counter(m).to(DEV)
    with torch.no_grad():
        for f in c.f:
            f.weight.copy_(torch.rand(17, device=DEV) + 0.2)
    ws = [f.weight.detach() for f in c.f]
    wptr = (ctypes.c_void_p * 8)(*[w.data_ptr() for w in ws])
    for V in (36, 100):
        logits = 3.0 * torch.randn(B, G, V, Q, device=DEV)
        xy = torch.rand(B, V, 2, device=DEV) * 0.6
        b = torch.cat([xy, xy + 0.05 + 0.35 * torch.rand(B, V, 2, device=DEV), torch.rand(B, V, 2, device=DEV)], 2)
        boxes = b[:, :, :4].transpose(1, 2)
        out, save = ops.counter_fwd(boxes, logits, ws, m)
        dout = torch.randn_like(out)
        dlogits = torch.empty_like(logits)
        dw_part = torch.empty(B * G, 8 * 17, device=DEV)
        st = ops._stream()
        sL, sB = logits.stride(), boxes.stride()

        def fwd():
            L.check(lib.cti_counter_fwd(logits.data_ptr(), sL[0], sL[1], sL[2], sL[3], boxes.data_ptr(), sB[0], sB[1], sB[2], wptr, 0, out.data_ptr(),
                                        out.stride(0), out.stride(1), save.data_ptr(), save.numel() * 4, B, G, V, Q, m, 16, st), "cti_counter_fwd")

        def bwd():
            L.check(lib.cti_counter_bwd(dout.data_ptr(), boxes.data_ptr(), sB[0], sB[1], sB[2], wptr, 0, save.data_ptr(), save.numel() * 4,
                                        dlogits.data_ptr(), dw_part.data_ptr(), B, G, V, Q, m, 16, st), "cti_counter_bwd")
        for name, fn in (("cti_counter_fwd", fwd), ("cti_counter_bwd", bwd)):
            us = timeit(fn, reps)
            print(json.dumps(dict(kernel=name, rows=B * G, V=V, Q=Q, objects=m, us=round(us, 2), ns_per_row=round(us * 1e3 / (B * G), 1), reps=reps)), flush=True)
        us = timeit(lambda: ops.counter_bwd(dout, boxes, ws, save, m, tuple(logits.shape)), reps)
        print(json.dumps(dict(kernel="ops.counter_bwd (kernel + col_sum of the partials + allocations)", rows=B * G, V=V, us=round(us, 2), reps=reps)), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 50)
