#!/usr/bin/env python3
"""tests/golden/adapter_search.npz: whole searches of the REAL reference (pasero.decoding.sampling / beam_search, CPU fp32) on
a tiny `adapter_transformer` (d = 128, 2 heads, 1 encoder and 2 decoder layers, decoder_adapter_dim 8) whose weights come
from paramgen seeds — adapter projections and biases at ordinary scale (paramgen draws every Linear at fan-in scale), not
the 1e-6 initialisation — for tests/test_adapter_decode_gpu.py.  Outputs only: every hypothesis (tokens, score), the rows
the decoder saw at every call, `min_gap` and `max_logit`.

Cases:  g  greedy, B = 3          k  beam K = 4, B = 2          s  beam K = 3, B = 4, a sentence leaves the batch
        l  decoder_adapters_by=['lang'] with the languages de / fr: the same batch searched once per language (beam K = 2)

`min_gap`: for the beam cases the smallest difference between neighbouring finite scores among the best 2K + 1 of any
sentence at any step (tests/beam_ref.py over the reference decoder's logits, which also checks that restatement against the
reference); for the greedy case the smallest top-1 / top-2 logit difference of any row at any call.  A seed is usable when
min_gap >= 1e-3 * max|logit| (50 x the project's fp32 decoder-logits bound), when the same search with the decoder adapters
disabled gives other tokens for at least one sentence (`differs_without_adapters`) and, in case l, when the two languages'
outputs differ (`languages_differ`): a search that never read the adapters would not reproduce the fixture.

Runs where the reference tree is importable (oracle/make_golden.py says how):  python tools/make_adapter_search_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import make_golden as MG  # noqa: E402  (imports the reference, stubs its absent third-party modules)
import paramgen  # noqa: E402
from beam_ref import beam_ref  # noqa: E402

torch, decoding = MG.torch, MG.decoding
TINY = dict(embed_dim=128, encoder_ffn_dim=128, decoder_ffn_dim=128, encoder_attention_heads=2, decoder_attention_heads=2,
            encoder_layers=1, decoder_layers=2, dropout=0.0, decoder_adapter_dim=8)
LANGS = ['de', 'fr']
CASES = {
    'g': dict(V=61, B=3, S=7, K=1, max_out=8, metas=[{}]),
    'k': dict(V=61, B=2, S=7, K=4, max_out=5, metas=[{}]),
    's': dict(V=61, B=4, S=6, K=3, max_out=8, metas=[{}], shrink=True),
    'l': dict(V=61, B=2, S=7, K=2, max_out=6, metas=[{'lang': lang} for lang in LANGS], by=['lang']),
}


class LangTask(MG.FakeTask):
    def get_langs_or_domains(self, key):
        assert key == 'lang'
        return set(LANGS)


def build(case, seed):
    stock = MG.FakeTask
    MG.FakeTask = LangTask  # (build_model instantiates the module's FakeTask)
    try:
        cfg, model = MG.build_model(case['V'], arch='adapter_transformer', decoder_adapters_by=case.get('by', []), **TINY)
    finally:
        MG.FakeTask = stock
    MG.load_params(model, seed)
    model.eval()
    return cfg, model


def one_search(case, cfg, model, batch, meta, adapters_on=True):
    dec, rows, logits = model.decoder, [], []
    for layer in dec.layers:
        for ad in layer.adapters.values():
            ad.enable() if adapters_on else ad.disable()
    inner = dec.forward

    def spy(encoder_out, encoder_mask, decoder_input, **kw):
        out = inner(encoder_out, encoder_mask, decoder_input, **kw)
        rows.append(encoder_out.size(0))
        logits.append(out[0].detach().clone())
        return out
    dec.forward = spy
    prompt = torch.full((case['B'], 1), cfg.bos_idx, dtype=torch.long)
    try:
        with torch.no_grad():
            enc_out, enc_mask, _ = model.encoder(MG.t(batch['encoder_input']), MG.t(batch['encoder_input_length']))
            if case['K'] == 1:
                hyps = decoding.sampling(dec, enc_out, enc_mask, case['max_out'], meta, decoder_input=prompt,
                                         sampling_temperature=0, return_scores=True)
                for nbest in hyps:
                    nbest[0]['score'] = nbest[0]['pos_scores'].sum()
            else:
                hyps = decoding.beam_search(dec, enc_out, enc_mask, case['max_out'], case['K'], meta, decoder_input=prompt)
    finally:
        dec.forward = inner
        for layer in dec.layers:
            for ad in layer.adapters.values():
                ad.enable()
    if case['K'] == 1:
        top2 = torch.cat([x[:, -1].float().topk(2, dim=-1).values for x in logits])
        stats = {'min_gap': float((top2[:, 0] - top2[:, 1]).min()), 'max_logit': float(max(x.abs().max() for x in logits))}
        same = True
    else:
        feed_log, stats = iter(logits), {}
        mine = beam_ref(lambda feed: next(feed_log), lambda idx: None, prompt, case['K'], case['max_out'], cfg.decoder_max_len,
                        cfg.padding_idx, cfg.eos_idx, stats=stats)
        same = stats['rows'] == rows and all(
            len(a) == len(b) and all(torch.equal(x['tokens'], y['tokens']) for x, y in zip(a, b)) for a, b in zip(hyps, mine))
    return hyps, rows, stats, same


def tokens_of(hyps):
    return [[h['tokens'].tolist() for h in nbest] for nbest in hyps]


def main():
    out = {'cases': np.array(sorted(CASES)), 'langs': np.array(LANGS)}
    for name, case in CASES.items():
        for seed in range(100, 1100):
            cfg, model = build(case, seed)
            batch = paramgen.make_text_batch(seed, case['B'], case['S'], 5, case['V'])
            runs = [one_search(case, cfg, model, batch, meta) for meta in case['metas']]
            plain = [one_search(case, cfg, model, batch, meta, adapters_on=False) for meta in case['metas']]
            differs = all(tokens_of(r[0]) != tokens_of(q[0]) for r, q in zip(runs, plain))
            langs_differ = len(runs) < 2 or tokens_of(runs[0][0]) != tokens_of(runs[1][0])
            ok = (all(r[2]['min_gap'] >= 1e-3 * r[2]['max_logit'] and r[3] for r in runs) and differs and langs_differ
                  and (not case.get('shrink') or len(set(runs[0][1])) > 1))
            if ok:
                break
        else:
            raise RuntimeError(f'case {name}: no usable seed')
        p = name + ':'
        out.update({p + 'cfg': MG.cfg_json(cfg), p + 'V': case['V'], p + 'B': case['B'], p + 'S': case['S'], p + 'K': case['K'],
                    p + 'seed': seed, p + 'max_output_len': case['max_out'], p + 'adapters_by': np.array(case.get('by', []), dtype=str),
                    p + 'n_runs': len(runs), p + 'differs_without_adapters': bool(differs),
                    p + 'languages_differ': bool(len(runs) > 1 and langs_differ)})
        for j, (meta, (hyps, rows, stats, _)) in enumerate(zip(case['metas'], runs)):
            print(f'case {name} run {j} {meta}: seed {seed}, rows per call {rows}, min_gap {stats["min_gap"]:.3e}, max|logit| '
                  f'{stats["max_logit"]:.3f}')
            r = f'{p}{j}:'
            out.update({r + 'lang': meta.get('lang', ''), r + 'rows': np.array(rows), r + 'min_gap': stats['min_gap'],
                        r + 'max_logit': stats['max_logit'], r + 'n_hyps': np.array([len(nb) for nb in hyps])})
            for b, nbest in enumerate(hyps):
                for i, h in enumerate(nbest):
                    out[f'{r}{b}:{i}:tokens'] = MG.npy(h['tokens'])
                    out[f'{r}{b}:{i}:score'] = float(h['score'])
    path = os.path.join(MG.OUT, 'adapter_search.npz')
    np.savez_compressed(path, **out)  # (the cfg strings are UTF-32: they shrink tenfold)
    print(f'wrote {path}: {os.path.getsize(path) / 1e3:.1f} kB')


if __name__ == '__main__':
    main()
