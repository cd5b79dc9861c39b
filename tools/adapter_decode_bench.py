#!/usr/bin/env python3
"""Decoding-step benchmark of an adapter decoder at the size of the IWSLT2023 recipe (`adapter_nllb_1b3` decoded with
`--decoder-adapters default`): d = 1024, f = 8192, 24 pre-norm decoder layers, a bottleneck adapter of p = 64 after every
layer, V = 256 206, bf16, 500 encoder positions (a synthetic encoder output: only the decoder is timed).

Reports ms per incremental decoder call (one new token per row) at 1, 8, 40 and 160 rows for
  perop     the per-op path (PASERO_NO_NATIVE_DECODE=1): what a decoder with adapter layers ran before the native step took it
  native3   the native step, every adapter as its three-launch sequence (PK_ADAPTER_FUSED=0; also the step's default route)
  fused     the native step, every adapter as ONE launch (PK_ADAPTER_STEP_FUSED=1), the d columns spread over workgroups
  tile      the same with one workgroup per 32-row tile (PK_ADAPTER_SLICE_BLOCKS=0)
  backbone  the native step of the same decoder without adapters (`decoder_adapters=[]`), for reference
The switches are read when the library is loaded, so every path is a process of its own, started under its own
`timeout`; the first one that fails ends the run.  Per row count: 8 warm-up steps, then 5 blocks of 16 steps, one
synchronisation per block; the median block / 16 is the figure.  One session, one box: compare the columns of one run only.

usage: tools/adapter_decode_bench.py [--rows 1 8 40 160] [--paths perop native3 fused tile backbone] [--out FILE.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = {'perop': {'PASERO_NO_NATIVE_DECODE': '1'}, 'native3': {'PK_ADAPTER_FUSED': '0'}, 'fused': {'PK_ADAPTER_STEP_FUSED': '1'},
         'tile': {'PK_ADAPTER_STEP_FUSED': '1', 'PK_ADAPTER_SLICE_BLOCKS': '0'}, 'backbone': {}}
V, S, WARMUP, BLOCKS, BLOCK = 256206, 500, 8, 5, 16


def child(path, rows_list, layers):
    sys.path.insert(0, ROOT)
    import torch
    from pasero_amd import adapters, config as C, decode  # noqa: F401
    cfg = C.AdapterNLLB1B3Config(encoder_layers=1, decoder_layers=layers, dropout=0.0, encoder_adapters=[],
                                 decoder_adapters=[] if path == 'backbone' else None, decoder_adapter_dim=64)
    assert cfg.embed_dim == 1024 and cfg.decoder_ffn_dim == 8192 and cfg.decoder_prenorm
    torch.manual_seed(0)
    model = C.get_architecture(cfg)(cfg, C.DistributedConfig(), C.SyntheticTask(V)).to(torch.bfloat16).cuda().eval()
    dec = model.decoder
    for rows in rows_list:
        g = torch.Generator(device='cuda').manual_seed(rows)
        enc_out = torch.randn(rows, S, cfg.embed_dim, device='cuda', generator=g).to(torch.bfloat16)
        enc_mask = torch.zeros(rows, S, dtype=torch.bool, device='cuda')
        tok = torch.randint(4, V, (rows, 1 + WARMUP + BLOCKS * BLOCK), device='cuda', generator=g)
        state, times = {}, []
        with torch.no_grad():
            dec(enc_out, enc_mask, tok[:, :1], state=state, meta={})
            for t in range(1, 1 + WARMUP):
                dec(enc_out, enc_mask, tok[:, t:t + 1], state=state, meta={})
            for b in range(BLOCKS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for t in range(1 + WARMUP + b * BLOCK, 1 + WARMUP + (b + 1) * BLOCK):
                    logits, _ = dec(enc_out, enc_mask, tok[:, t:t + 1], state=state, meta={})
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) / BLOCK * 1e3)
        native = decode.DecodeCache.KEY in state
        plan = decode.get_plan(dec)
        assert native == (path != 'perop'), (path, native)
        assert path in ('perop', 'backbone') or plan.c_adapters is not None
        times.sort()
        print(json.dumps({'path': path, 'rows': rows, 'ms_per_step': round(times[len(times) // 2], 4),
                          'min': round(times[0], 4), 'max': round(times[-1], 4), 'native': native,
                          'checksum': float(logits.float().abs().sum())}), flush=True)
        del state, enc_out, logits
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='*', default=[1, 8, 40, 160])
    ap.add_argument('--paths', nargs='*', default=list(PATHS), choices=list(PATHS))
    ap.add_argument('--layers', type=int, default=24)
    ap.add_argument('--timeout', type=int, default=240, help='seconds per path (one process)')
    ap.add_argument('--out')
    ap.add_argument('--child')
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.rows, args.layers)
    results = []
    for path in args.paths:
        env = {k: v for k, v in os.environ.items() if k not in ('PASERO_NO_NATIVE_DECODE', 'PK_ADAPTER_FUSED',
                                                                'PK_ADAPTER_SLICE_BLOCKS', 'PK_ADAPTER_STEP_FUSED')}
        env.update(PATHS[path])
        cmd = ['timeout', '-k', '10', str(args.timeout), sys.executable, os.path.abspath(__file__), '--child', path,
               '--layers', str(args.layers), '--rows'] + [str(r) for r in args.rows]
        run = subprocess.run(cmd, env=env, capture_output=True, text=True)
        sys.stderr.write(run.stderr[-2000:])
        for line in run.stdout.splitlines():
            if line.startswith('{'):
                results.append(json.loads(line))
                print(line, flush=True)
        if run.returncode != 0:
            print(f'path {path} ended with status {run.returncode}: stopping', flush=True)
            sys.exit(run.returncode)
    table = {(r['path'], r['rows']): r['ms_per_step'] for r in results}
    print('\n| rows | ' + ' | '.join(args.paths) + ' |\n|---|' + '---|' * len(args.paths))
    for rows in args.rows:
        print(f'| {rows} | ' + ' | '.join(f'{table[(p, rows)]:.3f}' for p in args.paths) + ' |')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
