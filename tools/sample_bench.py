#!/usr/bin/env python3
"""Sampling micro-benchmark.  Part 1: microseconds per decoding step of pk_sample_select (`SampleSelect.run`, both launches)
and of the reference's per-step op chain in plain torch (decoding.py:1143-1190 restated below with stock ops: `.float()
.log_softmax`, the finished-row mask, then argmax + gather / topk + exp + multinomial / exp + sort + cumsum + mask + max()
+ multinomial / exp + multinomial) on the same GPU and the same logits, for greedy+scores, top-k 40, top-p 0.9 and full at
V = 8032, 70 376, 256 206, B = 32, 256, bf16 and fp32.  Both sides are timed in the same process, alternating, `--rounds`
rounds of `--iters` back-to-back calls between two device events (so a launch-bound side pays its enqueue time); medians
over the rounds are compared and the torch side's spread ((max - min) / median over its rounds) is printed as the margin.
Part 2: ms per step of a whole `pasero_amd.decode.sampling` search (top-p 0.9) on Transformer-base against the loop of
tests/sample_ref.py over the same decoder.
usage: tools/sample_bench.py [--rounds 3] [--iters 20] [--skip-search] [--only-search]
Per-kernel times: `rocprofv3 --kernel-trace --stats -- python tools/sample_bench.py ...` in a run of its own."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
MODES = (('greedy+scores', 'greedy', {}), ('top-k 40', 'topk', {'top_k': 40}), ('top-p 0.9', 'topp', {'top_p': 0.9}),
         ('full', 'full', {}))


def torch_chain(logits, mode, finished, pad, top_k=0, top_p=1.0):
    """one step of the reference's single-decoder path after the decoder call (no repeat penalty, empty blacklist)"""
    lp = logits.float().log_softmax(dim=-1)
    pad_prob = lp[:, pad].clone()
    lp.masked_fill_(finished.unsqueeze(1), -torch.inf)
    lp[:, pad] = pad_prob
    if mode == 'greedy':
        tok = lp.argmax(dim=-1)
    elif mode == 'topk':
        values, indices = lp.topk(top_k, dim=-1)
        tok = indices.gather(1, values.exp().multinomial(num_samples=1, replacement=True)).reshape(-1)
    elif mode == 'topp':
        probs, order = lp.exp().sort(dim=-1, descending=True)
        mask = probs.cumsum(dim=-1) <= top_p
        last = mask.cumsum(-1)[:, -1:]
        last.clamp_(0, mask.size(1) - 1)
        mask.scatter_(-1, last, True)
        probs.masked_fill_(~mask, 0)
        width = int(last.max()) + 1  # (the reference's host read)
        tok = order[:, :width].gather(1, probs[:, :width].multinomial(num_samples=1, replacement=True)).reshape(-1)
    else:
        tok = lp.exp().multinomial(num_samples=1, replacement=True).reshape(-1)
    return tok, -lp.gather(1, tok.unsqueeze(1)).squeeze(1)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def kernel_table(args):
    from pasero_amd.decode import SampleSelect
    print('| dtype | V | B | mode | pk_sample_select us | torch chain us | torch spread | ratio |')
    print('|---|---|---|---|---|---|---|---|')
    losses = []
    for dtype in (torch.bfloat16, torch.float32):
        for V in (8032, 70376, 256206):
            for B in (32, 256):
                gen = torch.Generator(device='cuda').manual_seed(V + B)
                ld = (V + 7) // 8 * 8
                logits = (torch.randn(B, ld, device='cuda', generator=gen) * 3.0).to(dtype)[:, :V]
                finished = torch.zeros(B, dtype=torch.bool, device='cuda')
                sel = SampleSelect(B, V, 'cuda')
                for label, mode, kw in MODES:
                    ours = lambda: sel.run(logits, mode, finished=finished.view(torch.uint8), pad=1, seed=1, offset=1, **kw)
                    ref = lambda: torch_chain(logits, mode, finished, 1, **kw)
                    iters = max(3, args.iters // (8 if V * B > 10_000_000 else 1))
                    ours(), ref()
                    torch.cuda.synchronize()
                    a, b = [], []
                    for _ in range(args.rounds):
                        a.append(timed(ours, iters))
                        b.append(timed(ref, iters))
                    ma, mb = statistics.median(a), statistics.median(b)
                    spread = (max(b) - min(b)) / mb
                    if ma > mb * (1 + spread):
                        losses.append((dtype, V, B, label))
                    print(f'| {str(dtype)[6:]} | {V} | {B} | {label} | {ma:.1f} | {mb:.1f} | {100 * spread:.1f} % | {mb / ma:.2f}x |',
                          flush=True)
    clock = torch.cuda.clock_rate() if hasattr(torch.cuda, 'clock_rate') else 0
    print(f'sm clock {clock} MHz; {args.rounds} rounds x {args.iters} calls (1/8 of them on the largest shapes); '
          f'shapes where the kernel is slower than the chain beyond its spread: {losses or "none"}')


def search_row(args):
    import paramgen
    from sample_ref import sample_ref
    from pasero_amd import config as C
    from pasero_amd.decode import sampling
    from pasero_amd.transformer import Transformer
    V, B, S, steps = 8032, 32, 64, 32
    cfg = C.TransformerConfig()
    torch.manual_seed(0)
    model = Transformer(cfg, C.DistributedConfig(), C.SyntheticTask(V)).to(torch.bfloat16).cuda().eval()
    b = paramgen.make_text_batch(1, B, S, 4, V, ragged=True)
    with torch.no_grad():
        enc_out, enc_mask, _ = model.encoder(torch.from_numpy(b['encoder_input']).cuda(),
                                             torch.from_numpy(b['encoder_input_length']).cuda())
    uniforms = torch.rand(steps + 1, B, device='cuda')
    prompt = torch.full((B, 1), cfg.bos_idx, dtype=torch.long, device='cuda')
    calls = {'n': 0}
    inner = model.decoder.forward

    def counted(*a, **kw):
        calls['n'] += 1
        return inner(*a, **kw)
    model.decoder.forward = counted

    def ours():
        return sampling(model.decoder, enc_out, enc_mask, steps, {}, sampling_topp=0.9, uniforms=uniforms)

    def ref():
        state = {}
        with torch.no_grad():
            return sample_ref(lambda feed: model.decoder(enc_out, enc_mask, feed, state=state)[0], prompt, steps,
                              cfg.decoder_max_len, cfg.padding_idx, cfg.eos_idx, sampling_topp=0.9, uniforms=uniforms)
    res = {'sampling': [], 'sample_ref': []}
    ours(), ref()
    for _ in range(args.rounds):
        for label, fn in (('sampling', ours), ('sample_ref', ref)):
            calls['n'] = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            res[label].append(1e3 * (time.perf_counter() - t0) / max(1, calls['n']))
    med = {k: statistics.median(v) for k, v in res.items()}
    print(f'Transformer-base bf16 V={V} B={B} S={S}, top-p 0.9, {steps} steps: sampling {med["sampling"]:.3f} ms per step '
          f'({min(res["sampling"]):.3f}-{max(res["sampling"]):.3f}), sample_ref loop {med["sample_ref"]:.3f} ms per step '
          f'({min(res["sample_ref"]):.3f}-{max(res["sample_ref"]):.3f}), {med["sample_ref"] / med["sampling"]:.2f}x')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--skip-search', action='store_true')
    ap.add_argument('--only-search', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'sample_bench needs the GPU (no CPU timing stands in for it)'
    assert args.rounds >= 3
    if not args.only_search:
        kernel_table(args)
    if not args.skip_search:
        search_row(args)


if __name__ == '__main__':
    main()
