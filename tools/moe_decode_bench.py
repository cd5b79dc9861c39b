#!/usr/bin/env python3
"""Decoding benchmark of a mixture-of-experts decoder (`moe_transformer`, bf16): ms per incremental decoder call and the
few-rows expert call alone.  Default sizes d = 1024, f = 4096, E = 16; `--nllb` takes the NLLB-MoE layer size d = 2048,
f = 8192, E = 128.  The decoder has `--layers` pre-norm layers, every `--interval`-th a mixture, V = 32 000, 64 encoder positions
(a synthetic encoder output: only the decoder is timed).

  step   per row count, ms per decoder call (one new token per row) on
           perop    the per-op path (`decode.moe_native(False)`): what an MoE decoder runs by default
           grouped  the native step with the grouped route forced (`pk_moerows_few_max(0)`)
           few      the native step with the few-rows kernels (threshold 1024: the route kernel's limit)
         The three alternate inside one process, per row count: 8 warm-up calls, then 5 blocks of 16 calls, one
         synchronisation per block; the median block / 16 is the figure.
  rows   pk_moerows alone over rows in {1, 4, 16, 64, 128, 256, 512}, grouped against few, alternating: 5 warm-up calls, then 5
         windows of 20 calls between device events; the median window / 20.  Per row count the bytes of the ROUTED experts'
         weights (experts with at least one slot x 2 D F elements — what the block has to stream; counted from the routing
         tables of the same input) over that time, as bytes/s and as a share of the HBM roof (8.0 TB/s spec; a float4 copy
         reaches 6.29 TB/s).  The experts' weights of one layer fit the last-level cache at the default size only in part
         (268 MB) and not at the NLLB size (8.6 GB): the figure is a streaming rate, not a cache rate, where it says so.
         `crossover`: the largest row count of the sweep at which the few route is not slower — the measured value for
         pk_moerows_few_max.
One session, one box: compare the columns of one run only.

usage: tools/moe_decode_bench.py [--nllb] [--parts step rows] [--step-rows 1 8 40 80 160] [--layers 4] [--interval 2] [--out F.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
V, S, WARMUP, BLOCKS, BLOCK = 32000, 64, 8, 5, 16
SWEEP = [1, 4, 16, 64, 128, 256, 512]
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
ROUTES = {'grouped': 0, 'few': 1024}


def build(args):
    import torch
    from pasero_amd import config as C, moe  # noqa: F401  (registers the architecture)
    d, f, E = (2048, 8192, 128) if args.nllb else (1024, 4096, 16)
    cfg = C.MOETransformerConfig(embed_dim=d, encoder_ffn_dim=f, decoder_ffn_dim=f, encoder_attention_heads=d // 64,
                                 decoder_attention_heads=d // 64, encoder_layers=1, decoder_layers=args.layers, dropout=0.0,
                                 encoder_prenorm=True, decoder_prenorm=True, encoder_expert_count=2, decoder_expert_count=E,
                                 encoder_expert_interval=0, decoder_expert_interval=args.interval, moe_impl='basic')
    torch.manual_seed(0)
    with torch.device('cuda'):   # (the experts of the NLLB size are 17 GB in fp32: built where they will live)
        model = C.get_architecture(cfg)(cfg, C.DistributedConfig(), C.SyntheticTask(V))
    return cfg, model.to(torch.bfloat16).eval(), (d, f, E)


def bench_step(model, cfg, rows_list):
    import torch
    from pasero_amd import decode, functional as F
    dec, out = model.decoder, []
    for rows in rows_list:
        g = torch.Generator(device='cuda').manual_seed(rows)
        enc_out = torch.randn(rows, S, cfg.embed_dim, device='cuda', generator=g).to(torch.bfloat16)
        enc_mask = torch.zeros(rows, S, dtype=torch.bool, device='cuda')
        tok = torch.randint(4, V, (rows, 1 + WARMUP + BLOCKS * BLOCK), device='cuda', generator=g)
        times = {p: [] for p in ('perop', 'grouped', 'few')}
        states, sums = {}, {}
        with torch.no_grad():
            for path in times:   # set-up and warm-up of every path, then the timed blocks alternate
                decode.moe_native(path != 'perop')
                F.moe_rows_few_max(ROUTES.get(path, 1024))
                st = states[path] = {}
                for t in range(0, 1 + WARMUP):
                    dec(enc_out, enc_mask, tok[:, t:t + 1], state=st, meta={})
                assert (decode.DecodeCache.KEY in st) == (path != 'perop'), path
            for b in range(BLOCKS):
                for path in times:
                    decode.moe_native(path != 'perop')
                    F.moe_rows_few_max(ROUTES.get(path, 1024))
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for t in range(1 + WARMUP + b * BLOCK, 1 + WARMUP + (b + 1) * BLOCK):
                        logits, _ = dec(enc_out, enc_mask, tok[:, t:t + 1], state=states[path], meta={})
                    torch.cuda.synchronize()
                    times[path].append((time.perf_counter() - t0) / BLOCK * 1e3)
                    sums[path] = float(logits.float().abs().sum())
        rec = {'part': 'step', 'rows': rows}
        for path, ts in times.items():
            ts.sort()
            rec[path] = round(ts[len(ts) // 2], 4)
            rec[path + '_min'], rec[path + '_max'] = round(ts[0], 4), round(ts[-1], 4)
        rec['checksums'] = sums
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del states, enc_out
        torch.cuda.empty_cache()
    return out


def bench_rows(model, sizes):
    import torch
    from pasero_amd import functional as F
    d, f, E = sizes
    layer = next(l for l in model.decoder.layers if hasattr(l, 'moe_layer')).moe_layer
    ex = layer.experts
    tabs = layer._tables.get((tuple(e.fc1.weight for e in ex), tuple(e.fc2.weight for e in ex),
                              tuple(e.fc1.bias for e in ex) if layer.has_bias else None,
                              tuple(e.fc2.bias for e in ex) if layer.has_bias else None))
    w1, w2, b1, b2 = tabs
    out = []
    for rows in SWEEP:
        g = torch.Generator(device='cuda').manual_seed(100 + rows)
        x = torch.randn(rows, d, device='cuda', generator=g).to(torch.bfloat16)
        y = torch.empty_like(x)
        offsets = F.moe_gate(F.gemm(x, layer.gate.weight).float(), None).offsets.cpu()
        used = int((offsets[1:] > offsets[:-1]).sum())
        nbytes = used * 2 * d * f * 2
        times = {r: [] for r in ROUTES}
        for route, thr in ROUTES.items():
            F.moe_rows_few_max(thr)
            for _ in range(5):
                F.moe_rows(x, layer.gate.weight, w1, w2, b1, b2, f, layer.act_name, out=y)
        for _ in range(5):
            for route, thr in ROUTES.items():
                F.moe_rows_few_max(thr)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(20):
                    F.moe_rows(x, layer.gate.weight, w1, w2, b1, b2, f, layer.act_name, out=y)
                b.record()
                torch.cuda.synchronize()
                times[route].append(a.elapsed_time(b) / 20)
        rec = {'part': 'rows', 'rows': rows, 'experts_used': used, 'routed_weight_bytes': nbytes}
        for route, ts in times.items():
            ts.sort()
            ms = ts[len(ts) // 2]
            rec[route + '_ms'] = round(ms, 5)
            rec[route + '_TBps'] = round(nbytes / (ms * 1e-3) / 1e12, 3)
            rec[route + '_of_hbm_spec'] = round(nbytes / (ms * 1e-3) / HBM_SPEC, 3)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    F.moe_rows_few_max(256)
    ok = [r['rows'] for r in out if r['few_ms'] <= r['grouped_ms']]
    print(json.dumps({'part': 'rows', 'crossover': max(ok) if ok else 0,
                      'few_not_slower_at': ok, 'hbm_copy_share_of_spec': round(HBM_COPY / HBM_SPEC, 3)}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nllb', action='store_true', help='the NLLB-MoE layer size: d = 2048, f = 8192, E = 128')
    ap.add_argument('--parts', nargs='*', default=['step', 'rows'], choices=['step', 'rows'])
    ap.add_argument('--step-rows', type=int, nargs='*', default=[1, 8, 40, 80, 160])
    ap.add_argument('--layers', type=int, default=4)
    ap.add_argument('--interval', type=int, default=2)
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('moe_decode_bench: needs an MI355X; nothing is measured without one')
    from pasero_amd import decode, functional as F
    cfg, model, sizes = build(args)
    first, thr = decode.moe_native(), F.moe_rows_few_max()
    results = []
    try:
        if 'step' in args.parts:
            results += bench_step(model, cfg, args.step_rows)
        if 'rows' in args.parts:
            results += bench_rows(model, sizes)
    finally:
        decode.moe_native(first)
        F.moe_rows_few_max(thr)
    steps = [r for r in results if r['part'] == 'step']
    if steps:
        print('\n| rows | per-op ms | grouped ms | few ms |\n|---|---|---|---|')
        for r in steps:
            print(f"| {r['rows']} | {r['perop']:.3f} | {r['grouped']:.3f} | {r['few']:.3f} |")
    sweep = [r for r in results if r['part'] == 'rows']
    if sweep:
        print('\n| rows | experts used | grouped ms | few ms | few TB/s | few / HBM spec |\n|---|---|---|---|---|---|')
        for r in sweep:
            print(f"| {r['rows']} | {r['experts_used']} | {r['grouped_ms']:.4f} | {r['few_ms']:.4f} | {r['few_TBps']:.2f} | "
                  f"{r['few_of_hbm_spec']:.2f} |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump({'sizes': sizes, 'layers': args.layers, 'interval': args.interval, 'results': results}, fh, indent=1)


if __name__ == '__main__':
    main()
