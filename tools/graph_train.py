#!/usr/bin/env python3
"""Training step of the FFOE CTI model (B = 256, the reference's widths) eager vs captured in a hipGraph (cti_amd.GraphedTrainStep):
ms per step and the host-side share.   python tools/graph_train.py [ffoe_cti|ffoe_ban|mc_cti] [steps] [--update-freq K]

--update-freq K: micro-batch accumulation, K micro-batches of B per update.  Three routes on the same model, ms per micro-batch and per update each:
eager autograd accumulation (FlatAdamaxDP(update_freq=K): K backward() calls, one add per parameter from the second on, step()), eager accumulate() /
update(), and the accumulating graphs (GraphedTrainStep(accumulate=True): graph M per micro-batch, graph U per update).  `graph_micro_only_ms` is a
replay of graph M alone."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cti_amd  # noqa: E402
import bench_model as bm  # noqa: E402


def main(name, steps, update_freq=None):
    builder, gamma, num_ans, Q, A = bm.CASES[name]
    B, ntoken = 256, 20000
    torch.manual_seed(1204)
    m = getattr(cti_amd, builder)(bm.args_of(gamma), bm.DS(ntoken, 2048, num_ans)).to("cuda").train()
    g = torch.Generator().manual_seed(7)
    v = torch.randn(B, 36, 2048, generator=g).abs().cuda()
    q = bm.tokens(B, Q, ntoken, g).cuda()
    a = bm.tokens(B, A, ntoken, g).cuda() if A else None
    boxes = torch.rand(B, 36, 6, generator=g).cuda()
    tgt = ((torch.rand(B, num_ans, generator=g) < 0.01).float()).cuda()
    crit = cti_amd.BCEWithLogitsSum()
    opt = cti_amd.FlatAdamaxDP(m, lr=1e-3, clip_norm=0.25, update_freq=update_freq or 1)
    if name == "ffoe_cti":
        inputs, fwd = (v, q, a), (lambda v_, q_, a_: m(v_, q_, a_))
    elif name == "ffoe_ban":
        inputs, fwd = (v, boxes, q), (lambda v_, b_, q_: m(v_, b_, q_, None)[0])
    else:
        inputs, fwd = (v, boxes, q, a), (lambda v_, b_, q_, a_: m(v_, b_, q_, a_)[0])

    class Wrap(torch.nn.Module):
        def forward(self, *xs):
            return fwd(*xs)
    loss_fn = lambda out, t: crit(out, t) / B        # noqa: E731

    def eager():
        opt.zero_grad()
        loss_fn(fwd(*inputs), tgt).backward()
        opt.step()

    def timeit(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        th = time.perf_counter() - t0
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3, th / steps * 1e3
    if update_freq is not None:
        return accumulate_case(name, B, update_freq, m, opt, Wrap(), loss_fn, fwd, inputs, tgt, timeit)
    t_e, h_e = timeit(eager)
    gs = cti_amd.GraphedTrainStep(Wrap(), opt, loss_fn, inputs, tgt, warmup=2)
    t_g, h_g = timeit(lambda: gs(inputs, tgt))
    print(json.dumps({"case": name, "B": B, "eager_ms": round(t_e, 3), "eager_host_ms": round(h_e, 3), "graph_ms": round(t_g, 3), "graph_host_ms": round(h_g, 3),
                      "samples_per_s_graph": round(B / t_g * 1e3, 1), "precision": cti_amd.get_precision(), "steps_done": opt.steps_done()}))


def accumulate_case(name, B, K, m, opt_k, wrap, loss_fn, fwd, inputs, tgt, timeit):
    """One timed call = one UPDATE (K micro-batches)."""
    def autograd_route():                                # what update_freq > 1 meant so far: AccumulateGrad adds per parameter, step() divides by K
        opt_k.zero_grad()
        for _ in range(K):
            loss_fn(fwd(*inputs), tgt).backward()
        opt_k.step()
    t_a, h_a = timeit(autograd_route)
    opt = cti_amd.FlatAdamaxDP(m, lr=1e-3, clip_norm=0.25)        # rebinds the parameters to its own flat buffers
    cti_amd.invalidate_caches()

    def eager_route():
        for _ in range(K):
            opt.zero_grad()
            loss_fn(fwd(*inputs), tgt).backward()
            opt.accumulate()
        opt.update()
    t_e, h_e = timeit(eager_route)
    gs = cti_amd.GraphedTrainStep(wrap, opt, loss_fn, inputs, tgt, warmup=2, accumulate=True)

    def graph_route():
        for j in range(K):
            gs(inputs, tgt, update_params=(j == K - 1))
    t_g, h_g = timeit(graph_route)
    t_m, h_m = timeit(lambda: gs(inputs, tgt, update_params=False))
    gs.update()
    r = lambda x: round(x, 3)        # noqa: E731
    print(json.dumps({"case": name, "B": B, "update_freq": K,
                      "autograd_acc_ms_per_micro_batch": r(t_a / K), "autograd_acc_ms_per_update": r(t_a), "autograd_acc_host_ms_per_update": r(h_a),
                      "eager_ms_per_micro_batch": r(t_e / K), "eager_ms_per_update": r(t_e), "eager_host_ms_per_update": r(h_e),
                      "graph_ms_per_micro_batch": r(t_g / K), "graph_ms_per_update": r(t_g), "graph_host_ms_per_update": r(h_g),
                      "graph_micro_only_ms": r(t_m), "samples_per_s_graph": round(B * K / t_g * 1e3, 1),
                      "precision": cti_amd.get_precision(), "steps_done": opt.steps_done()}))


if __name__ == "__main__":
    argv = list(sys.argv[1:])
    freq = None
    if "--update-freq" in argv:
        i = argv.index("--update-freq")
        freq = int(argv[i + 1])
        if freq < 1:
            sys.exit("--update-freq takes a positive integer")
        del argv[i:i + 2]
    main(argv[0] if argv else "ffoe_cti", int(argv[1]) if len(argv) > 1 else 30, freq)
