#!/usr/bin/env python3
"""Time one mixture-of-experts feed-forward (forward + backward, bf16) three ways on the same inputs:
  (a) dense      every expert over every token through pk_gemm, then the weighted sum — the arithmetic of the reference's `basic`
  (b) per-expert the routed computation as E pk_gemm launches on the slot-ordered buffers, counts read to the host
  (c) grouped    the grouped launches of csrc/moe.hip (no host read)
Shapes: moe_transformer_big (d 1024, F 4096, E 4 / 8 / 16, 8192 and 32768 tokens) and NLLB's (d 1024, F 8192, E 128, 8192 tokens).
Per path: median ms over --repeats timed runs after --warmup (CUDA events around forward + backward), TFLOP/s on the ROUTED
flops (2 experts per token, forward 4 d F, backward 8 d F per pair), and for (c) the share of gate + gather + combine (those
kernels timed alone on the same routing).  Prints one JSON line per shape.   python tools/moe_bench.py [--quick]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pasero_amd import functional as F  # noqa: E402
from pasero_amd.moe import MixtureOfExperts  # noqa: E402

SHAPES = [(1024, 4096, 4, 8192), (1024, 4096, 8, 8192), (1024, 4096, 16, 8192), (1024, 4096, 4, 32768), (1024, 4096, 8, 32768),
          (1024, 4096, 16, 32768), (1024, 8192, 128, 8192)]


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def dense_step(layer, x, dy):
    """(a): every expert over every token; the gate's outputs come from the same kernel, the rest is pk_gemm + torch glue.  It
    leaves out the gate's backward and the backward of the weighted sum (d top_w): its time is a LOWER bound for the dense layer"""
    S, D = x.shape
    logits = F.gemm(x, layer.gate.weight).float()
    r = F.moe_gate(logits, None)
    dense_w = torch.zeros(S, layer.expert_count, dtype=torch.float32, device=x.device).scatter_(1, r.top_idx.long(), r.top_w)
    out = torch.zeros(S, D, dtype=torch.float32, device=x.device)
    for e, ex in enumerate(layer.experts):
        h = F.gemm(x, ex.fc1.weight, bias=ex.fc1.bias, act='relu')
        y = F.gemm(h, ex.fc2.weight, bias=ex.fc2.bias)
        out += dense_w[:, e, None] * y
        dys = (dense_w[:, e, None] * dy).to(x.dtype)
        dh = F.gemm(dys, ex.fc2.weight, b_col=True, act='relu', aux=h, mode=2)
        F.gemm(dys, h, a_col=True, b_col=True)
        F.gemm(dh, ex.fc1.weight, b_col=True)
        F.gemm(dh, x, a_col=True, b_col=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--quick', action='store_true', help='the 8192-token shapes only')
    ap.add_argument('--no-dense', action='store_true')
    args = ap.parse_args()
    bf = torch.bfloat16
    try:
        clock = torch.cuda.clock_rate()
    except Exception:  # (not every build can ask the driver)
        clock = None
    print(json.dumps({'device': torch.cuda.get_device_name(0), 'clock_mhz': clock}))
    for D, Fd, E, S in SHAPES:
        if args.quick and S > 8192:
            continue
        torch.manual_seed(0)
        layer = MixtureOfExperts(D, Fd, E, E).to(bf).cuda()
        x = torch.randn(S, D, device='cuda').to(bf).requires_grad_()
        dy = torch.randn(S, D, device='cuda').to(bf)

        def step():
            y, _, _ = layer(x, None)
            y.backward(dy)
        res = {'d': D, 'F': Fd, 'E': E, 'tokens': S}
        flops = 2 * S * 12 * D * Fd
        for name, on in (('grouped', 1), ('per_expert', 0)):
            prev = F.moe_use_grouped(on)
            med, best = timed(step, args.warmup, args.repeats)
            F.moe_use_grouped(int(prev))
            res[name + '_ms'], res[name + '_min_ms'], res[name + '_tflops'] = round(med, 3), round(best, 3), round(flops / med / 1e9, 1)
        if not args.no_dense:
            with torch.no_grad():
                med, best = timed(lambda: dense_step(layer, x.detach(), dy), args.warmup, args.repeats)
            res['dense_ms'], res['dense_tflops_routed'] = round(med, 3), round(flops / med / 1e9, 1)
        with torch.no_grad():
            logits = F.gemm(x.detach(), layer.gate.weight).float()
            r = F.moe_gate(logits, None)
            ys = F.moe_gather(x.detach(), r)

            def routing():  # forward: gate, gather, combine; backward: scaled gather, dot, combine, gate backward
                rr = F.moe_gate(logits, None)
                F.moe_gather(x.detach(), rr)
                F.moe_combine(ys, rr)
                F.moe_gather(dy, rr, scaled=True)
                d = F.moe_dot(dy, ys, rr)
                F.moe_combine(ys, rr, weighted=False)
                F.moe_gate_bwd(d, rr)
            med, _ = timed(routing, args.warmup, args.repeats)
        res['routing_ms'], res['routing_share'] = round(med, 3), round(med / res['grouped_ms'], 3)
        res['per_expert_over_grouped'] = round(res['per_expert_ms'] / res['grouped_ms'], 3)
        print(json.dumps(res), flush=True)
        del layer, x, dy


if __name__ == '__main__':
    main()
