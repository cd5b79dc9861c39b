#!/usr/bin/env python3
"""tests/golden/beam_search.npz: whole searches of the REAL reference (pasero.decoding.beam_search, CPU fp32) on tiny
models whose weights come from paramgen seeds, for tests/test_beam_search_gpu.py.  Outputs only: every hypothesis of every
n-best list (tokens, score, normalized_score, pos_scores), the rows the decoder saw at every call, and `min_gap`, the
smallest difference between neighbouring finite scores among the best 2K + 1 of any sentence at any step (computed by
tests/beam_ref.py over the reference decoder's logits, which also checks that restatement against the reference).

A seed is usable when min_gap >= 1e-3 * max|logit| of its search — 50 x the project's fp32 decoder-logits bound (2e-5 of the
range), so the project's own logit error cannot re-order candidates.  Seeds are scanned per case until that holds; cases
marked `shrink` also need a sentence to leave the batch on the way.

Runs where the reference tree is importable (oracle/make_golden.py says how):  python tools/make_beam_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import make_golden as MG  # noqa: E402  (imports the reference, stubs its absent third-party modules)
import paramgen  # noqa: E402
from beam_ref import beam_ref  # noqa: E402

torch, decoding, transformer = MG.torch, MG.decoding, MG.transformer
TINY = dict(embed_dim=128, encoder_ffn_dim=128, decoder_ffn_dim=128, encoder_attention_heads=2, decoder_attention_heads=2,
            encoder_layers=1, decoder_layers=2, dropout=0.0)
CASES = {
    'a': dict(V=1003, B=2, S=7, K=5, max_out=4, return_scores=True, len_penalty=0.6, cfg={}),
    'b': dict(V=61, B=2, S=7, K=4, max_out=5, return_scores=True, len_penalty=1.0, cfg={}, prompts=True, blacklist=[1, 5, 6]),
    'c': dict(V=61, B=4, S=6, K=1, max_out=8, return_scores=True, len_penalty=1.0, cfg={}, shrink=True),
    'd': dict(V=61, B=2, S=7, K=3, max_out=5, return_scores=True, len_penalty=1.0,
              cfg=dict(encoder_positional_encoding='rotary', decoder_positional_encoding='rotary')),
}


def prompt_of(case, cfg, seed):
    """(B, 2): BOS + a target-language code on the even rows, BOS + padding on the odd ones"""
    B = case['B']
    p = torch.full((B, 1), cfg.bos_idx, dtype=torch.long)
    if case.get('prompts'):
        rs = np.random.RandomState(seed)
        code = torch.from_numpy(rs.randint(8, case['V'], size=B).astype(np.int64))  # (clear of the blacklist)
        code[1::2] = cfg.padding_idx
        p = torch.cat([p, code[:, None]], dim=1)
    return p


def run(case, seed):
    cfg, model = MG.build_model(case['V'], **TINY, **case['cfg'])
    names_shapes = MG.load_params(model, seed)
    model.eval()
    batch = paramgen.make_text_batch(seed, case['B'], case['S'], 5, case['V'])
    dec, rows, logits = model.decoder, [], []
    inner = dec.forward

    def spy(encoder_out, encoder_mask, decoder_input, **kw):
        out = inner(encoder_out, encoder_mask, decoder_input, **kw)
        rows.append(encoder_out.size(0))
        logits.append(out[0].detach().clone())
        return out
    dec.forward = spy
    try:
        with torch.no_grad():
            enc_out, enc_mask, _ = model.encoder(MG.t(batch['encoder_input']), MG.t(batch['encoder_input_length']))
            prompt = prompt_of(case, cfg, seed)
            hyps = decoding.beam_search(dec, enc_out, enc_mask, case['max_out'], case['K'], {}, decoder_input=prompt,
                                        return_scores=case['return_scores'], len_penalty=case['len_penalty'],
                                        blacklist=case.get('blacklist', []))
    finally:
        dec.forward = inner
    # the restatement over the same logits: must give the same search; its statistics are the fixture's
    feed_log = iter(logits)
    stats = {}
    mine = beam_ref(lambda feed: next(feed_log), lambda idx: None, prompt, case['K'], case['max_out'], cfg.decoder_max_len,
                    cfg.padding_idx, cfg.eos_idx, return_scores=case['return_scores'], len_penalty=case['len_penalty'],
                    blacklist=case.get('blacklist', []), stats=stats)
    same = stats['rows'] == rows and all(
        len(a) == len(b) and all(torch.equal(x['tokens'], y['tokens']) for x, y in zip(a, b)) for a, b in zip(hyps, mine))
    return cfg, names_shapes, hyps, rows, stats, same


def main():
    out = {'cases': np.array(sorted(CASES))}
    for name, case in CASES.items():
        for seed in range(100, 1100):
            cfg, names_shapes, hyps, rows, stats, same = run(case, seed)
            ok = stats['min_gap'] >= 1e-3 * stats['max_logit'] and (len(set(rows)) > 1 or not case.get('shrink'))
            if ok:
                break
        else:
            raise RuntimeError(f'case {name}: no usable seed')
        assert same, f'case {name} seed {seed}: tests/beam_ref.py and the reference disagree'
        print(f'case {name}: seed {seed}, rows per call {rows}, min_gap {stats["min_gap"]:.3e}, max|logit| '
              f'{stats["max_logit"]:.3f} (ratio {stats["min_gap"] / stats["max_logit"]:.2e})')
        p = name + ':'
        out.update({p + 'cfg': MG.cfg_json(cfg), p + 'V': case['V'], p + 'B': case['B'], p + 'S': case['S'], p + 'K': case['K'],
                    p + 'seed': seed, p + 'max_output_len': case['max_out'], p + 'len_penalty': case['len_penalty'],
                    p + 'return_scores': case['return_scores'], p + 'blacklist': np.array(case.get('blacklist', []), dtype=np.int64),
                    p + 'prompt': MG.npy(prompt_of(case, cfg, seed)), p + 'rows': np.array(rows), p + 'min_gap': stats['min_gap'],
                    p + 'max_logit': stats['max_logit'], p + 'n_hyps': np.array([len(nb) for nb in hyps])})
        for b, nbest in enumerate(hyps):
            for i, h in enumerate(nbest):
                q = f'{p}{b}:{i}:'
                out[q + 'tokens'] = MG.npy(h['tokens'])
                out[q + 'score'] = float(h['score'])
                out[q + 'normalized_score'] = float(h['normalized_score'])
                if case['return_scores']:
                    out[q + 'pos_scores'] = MG.npy(h['pos_scores'])
    MG.save('beam_search', **out)


if __name__ == '__main__':
    main()
