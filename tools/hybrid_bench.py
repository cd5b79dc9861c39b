#!/usr/bin/env python3
"""Benchmark of `hybrid_transformer` (bf16, the preset's sizes: d = 512, hidden 512, 6 encoder and 2 LSTM layers, V = 32 000):

  train   ms per training step (forward + backward) at B = 256, S = T = 128, with the package's kernels (`native`) and with the
          per-op composition in their place (`perop`: per time step one torch matmul and the pointwise cell; the reference's
          four attention lines, which materialise (B, T, S, hidden)); and the recurrence's share of the native step: the
          two LSTM layers' `LSTMFn` forward + backward alone over the step's time.
  decode  ms per incremental decoder call (one new token per row) at B*K = 5, 20, 80 rows, S = 128, native against per-op.

The two alternate inside one process: WARMUP calls each, then 5 blocks between synchronisations; the median block is the
figure.  It sets no threshold and nothing in the code rests on its numbers.  One session, one box: compare the columns of one
run only.

usage: tools/hybrid_bench.py [--parts train decode] [--batch 256] [--len 128] [--rows 5 20 80] [--out F.json]"""
import argparse
import contextlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
V, WARMUP, BLOCKS = 32000, 3, 5


def perop_lstm(gx, w_hh, b_hh, h0=None, c0=None):
    import torch
    B, T, G = gx.shape
    H = G // 4
    h = gx.new_zeros(B, H) if h0 is None else h0
    c = gx.new_zeros(B, H) if c0 is None else c0
    ys = []
    for t in range(T):
        i, f, g, o = (gx[:, t] + (h @ w_hh.t() + b_hh)).split(H, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        ys.append(h)
    return torch.stack(ys, dim=1), h, c


def perop_attention(q, k, w, w_bias, key_pad, value):
    import torch
    scores = torch.tanh(k.unsqueeze(1) + q.unsqueeze(2)) @ w + w_bias
    if key_pad is not None:
        scores = scores.float().masked_fill(key_pad.unsqueeze(1), float('-inf')).type_as(scores)
    probs = torch.softmax(scores, dim=2)
    return torch.bmm(probs, value), probs


@contextlib.contextmanager
def route(name):
    """`perop`: the two autograd functions of pasero_amd.hybrid replaced by the torch compositions above"""
    from pasero_amd import hybrid
    if name == 'native':
        yield
        return
    saved = hybrid.LSTMFn.apply, hybrid.AdditiveAttentionFn.apply
    hybrid.LSTMFn.apply, hybrid.AdditiveAttentionFn.apply = staticmethod(perop_lstm), staticmethod(perop_attention)
    try:
        yield
    finally:
        hybrid.LSTMFn.apply, hybrid.AdditiveAttentionFn.apply = saved


def median_ms(fn, calls_per_block):
    import torch
    for _ in range(WARMUP):
        fn()
    times = []
    for _ in range(BLOCKS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls_per_block):
            fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / calls_per_block * 1e3)
    return sorted(times)[len(times) // 2]


def build():
    import torch
    from pasero_amd import config as C, hybrid  # noqa: F401  (registers the architecture)
    cfg = C.HybridTransformerConfig(dropout=0.0)
    torch.manual_seed(0)
    model = C.get_architecture(cfg)(cfg, C.DistributedConfig(), C.SyntheticTask(V))
    return cfg, model.to(torch.bfloat16).cuda()


def bench_train(cfg, model, B, L):
    import torch
    from pasero_amd.hybrid import LSTMFn
    g = torch.Generator(device='cuda').manual_seed(1)
    batch = {'encoder_input': torch.randint(4, V, (B, L), device='cuda', generator=g),
             'encoder_input_length': torch.full((B,), L, dtype=torch.long, device='cuda'),
             'decoder_input': torch.randint(4, V, (B, L + 1), device='cuda', generator=g)}
    model.train()

    def step():
        model.zero_grad(set_to_none=True)
        loss, _ = model(**batch)
        loss.backward()
    rec = {'part': 'train', 'B': B, 'S': L, 'T': L}
    for name in ('native', 'perop'):
        with route(name):
            rec[name + '_ms'] = round(median_ms(step, 2), 3)
    H = cfg.decoder_hidden_size
    layer = model.decoder.layers[0]
    gx = torch.randn(B, L, 4 * H, device='cuda', generator=g).to(torch.bfloat16).requires_grad_()
    dy = torch.randn(B, L, H, device='cuda', generator=g).to(torch.bfloat16)

    def recurrence():
        gx.grad = layer.weight_hh_l0.grad = layer.bias_hh_l0.grad = None
        LSTMFn.apply(gx, layer.weight_hh_l0, layer.bias_hh_l0)[0].backward(dy)
    one = median_ms(recurrence, 2)
    rec['recurrence_ms'] = round(one * cfg.decoder_layers, 3)
    rec['recurrence_share'] = round(one * cfg.decoder_layers / rec['native_ms'], 3)
    print(json.dumps(rec), flush=True)
    return [rec]


def bench_decode(cfg, model, rows_list, S):
    import torch
    model.eval()
    dec, out = model.decoder, []
    for rows in rows_list:
        g = torch.Generator(device='cuda').manual_seed(rows)
        enc_out = torch.randn(rows, S, cfg.embed_dim, device='cuda', generator=g).to(torch.bfloat16)
        enc_mask = torch.zeros(rows, S, dtype=torch.bool, device='cuda')
        tok = torch.randint(4, V, (rows, 1), device='cuda', generator=g)
        rec = {'part': 'decode', 'rows': rows, 'S': S}
        with torch.no_grad():
            for name in ('native', 'perop'):
                with route(name):
                    state = {}
                    dec(enc_out, enc_mask, tok, state=state, meta={})
                    rec[name + '_ms'] = round(median_ms(lambda: dec(enc_out, enc_mask, tok, state=state, meta={}), 16), 4)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', nargs='*', default=['train', 'decode'], choices=['train', 'decode'])
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--len', type=int, default=128)
    ap.add_argument('--rows', type=int, nargs='*', default=[5, 20, 80])
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('hybrid_bench: needs an MI355X; nothing is measured without one')
    cfg, model = build()
    results = []
    if 'train' in args.parts:
        results += bench_train(cfg, model, args.batch, args.len)
    if 'decode' in args.parts:
        results += bench_decode(cfg, model, args.rows, args.len)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump({'results': results}, fh, indent=1)


if __name__ == '__main__':
    main()
