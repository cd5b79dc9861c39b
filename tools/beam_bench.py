#!/usr/bin/env python3
"""Beam search micro-benchmark: ms per search step of `pasero_amd.decode.beam_search` and of tests/beam_ref.py (plain torch
around the same decoder: log_softmax, sort, `Decoder.reorder_state` — what a user had before) on synthetic inputs, plus
pk_beam_select alone (median of timed calls, achieved GB/s of its one read of the logits).  Random weights never emit EOS
early, so both run `--steps` full steps with B * K rows.
usage: tools/beam_bench.py [--workload c2|c3|c5] [--sentences 64] [--beam 5] [--steps 32] [--src-len 128]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/beam_bench.py ...` in a run of its own;
synchronising calls per step: `--sync-probe` (torch.cuda.set_sync_debug_mode, as tools/sync_probe.py)."""
import argparse
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
WORKLOADS = {'c2': ('TransformerConfig', 8032), 'c3': ('TransformerBigConfig', 70376), 'c5': ('NLLB1B3Config', 256206)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='c2', choices=list(WORKLOADS))
    ap.add_argument('--sentences', type=int, default=64)
    ap.add_argument('--beam', type=int, default=5)
    ap.add_argument('--steps', type=int, default=32)
    ap.add_argument('--src-len', type=int, default=128)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--sync-probe', action='store_true')
    args = ap.parse_args()
    import paramgen
    from beam_ref import beam_ref
    from pasero_amd import config as C
    from pasero_amd.decode import BeamSelect, beam_search
    from pasero_amd.transformer import Transformer, Decoder
    assert torch.cuda.is_available(), 'beam_bench needs the GPU (no CPU timing stands in for it)'
    name, V = WORKLOADS[args.workload]
    cfg = getattr(C, name)()
    torch.manual_seed(0)
    with torch.device('cuda'):
        model = Transformer(cfg, C.DistributedConfig(), C.SyntheticTask(V))
    model = model.to(torch.bfloat16).cuda().eval()
    B, K = args.sentences, args.beam
    b = paramgen.make_text_batch(1, B, args.src_len, 4, V, ragged=True)
    enc_in, enc_len = torch.from_numpy(b['encoder_input']).cuda(), torch.from_numpy(b['encoder_input_length']).cuda()
    with torch.no_grad():
        enc_out, enc_mask, _ = model.encoder(enc_in, enc_len)
    calls = {'n': 0}
    inner = model.decoder.forward

    def counted(*a, **kw):
        calls['n'] += 1
        return inner(*a, **kw)
    model.decoder.forward = counted

    def ours():
        return beam_search(model.decoder, enc_out, enc_mask, args.steps, K, {})

    def ref():
        box = {'enc': enc_out.repeat_interleave(K, dim=0), 'mask': enc_mask.repeat_interleave(K, dim=0), 'state': {}}

        def reorder(idx):
            box['enc'], box['mask'] = box['enc'].index_select(0, idx), box['mask'].index_select(0, idx)
            Decoder.reorder_state(box['state'], idx)
        with torch.no_grad():
            prompt = torch.full((B, 1), cfg.bos_idx, dtype=torch.long, device='cuda')
            return beam_ref(lambda feed: model.decoder(box['enc'], box['mask'], feed, state=box['state'])[0], reorder, prompt, K,
                            args.steps, cfg.decoder_max_len, cfg.padding_idx, cfg.eos_idx)

    result = {}
    for label, fn in (('beam_search', ours), ('beam_ref', ref)):
        fn()  # warm-up: code objects, plans, allocator
        torch.cuda.synchronize()
        times = []
        for _ in range(args.repeats):
            calls['n'] = 0
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / max(1, calls['n']))
        result[label] = (statistics.median(times), min(times), max(times), calls['n'])
        if args.sync_probe:
            seen = []
            warnings.showwarning = lambda message, *a, **k: seen.append(str(message))
            warnings.simplefilter('always')
            torch.cuda.set_sync_debug_mode(1)
            fn()
            torch.cuda.set_sync_debug_mode(0)
            print(f'{label}: {len(seen) / max(1, calls["n"]):.1f} synchronising calls per decoder call ({len(seen)} in the search)')
    # pk_beam_select alone, on logits the size of a step's
    rows, ld = B * K, (V + 7) // 8 * 8
    logits = (torch.randn(rows, ld, device='cuda') * 3).to(torch.bfloat16)
    hyp = -torch.rand(rows, device='cuda')
    sel = BeamSelect(B, K, V, 'cuda')
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(30)]
    for _ in range(5):
        sel.run(logits[:, :V], B, cfg.eos_idx, cfg.padding_idx, hyp=hyp)
    for s, e in ev:
        s.record()
        sel.run(logits[:, :V], B, cfg.eos_idx, cfg.padding_idx, hyp=hyp)
        e.record()
    torch.cuda.synchronize()
    us = statistics.median(s.elapsed_time(e) for s, e in ev) * 1e3
    nbytes = rows * V * 2
    clock = torch.cuda.clock_rate() if hasattr(torch.cuda, 'clock_rate') else 0
    for label, (med, lo, hi, n) in result.items():
        print(f'{args.workload} bf16 B={B} K={K} S={args.src_len}: {label} {1e3 * med:.3f} ms per step (median of {args.repeats} '
              f'searches, {1e3 * lo:.3f}-{1e3 * hi:.3f}; {n} decoder calls per search; sm clock {clock} MHz)')
    print(f'{args.workload}: speed-up {result["beam_ref"][0] / result["beam_search"][0]:.2f}x; pk_beam_select {us:.1f} us per call '
          f'(median of 30, both launches), {nbytes / 1e6:.1f} MB of logits read once = {nbytes / us / 1e3:.0f} GB/s '
          f'(streaming-read copy rate of the chip: 6290 GB/s)')


if __name__ == '__main__':
    main()
