#!/usr/bin/env python3
"""tests/golden/sampling_search.npz: whole searches of the REAL reference (pasero.decoding.sampling, CPU fp32) on tiny models
whose weights come from paramgen seeds, for tests/test_sample_ref_cpu.py and tests/test_sampling_search_gpu.py.  Outputs
only: the tokens and pos_scores of every yielded step, the rows the decoder saw at every call, the last-position logits of
every call (what the CPU test replays tests/sample_ref.py from), the uniforms, the margins.

The deterministic cases (greedy with a repeat penalty, a blacklist with prompts of unequal length, a stop sequence,
`sampling_topk=1`) are recorded as they are.  For the stochastic modes `torch.Tensor.multinomial` is replaced, in this
process and for the duration of one search, by the project's draw rule: the weights in the order (weight descending,
position ascending), M their sum, the first position whose inclusive cumulative weight exceeds u * M — with u a 24-bit
uniform from a seeded numpy generator, recorded per step.  For top-k / top-p the reference hands `multinomial` the weights
in descending order already, so position order is (probability descending, token id ascending) provided no two positive
weights are equal: a seed with such a pair is passed over.

A seed is usable when tests/sample_ref.py replays the search token for token from the recorded logits, and every draw
margin (distance of u * M to the nearest cumulative edge, over M) and boundary margin is >= 1e-3, every greedy gap
>= 1e-3 * max|logit| — 50 x the project's fp32 decoder-logits bound (2e-5 of the range), so the project's own logit error
cannot move a choice.

Runs where the reference tree is importable (oracle/make_golden.py says how):  python tools/make_sampling_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import make_golden as MG  # noqa: E402  (imports the reference, stubs its absent third-party modules)
import paramgen  # noqa: E402
from sample_ref import sample_ref  # noqa: E402

torch, decoding = MG.torch, MG.decoding
TINY = dict(embed_dim=128, encoder_ffn_dim=128, decoder_ffn_dim=128, encoder_attention_heads=2, decoder_attention_heads=2,
            encoder_layers=1, decoder_layers=2, dropout=0.0)
OPTS = ('return_scores', 'sampling_temperature', 'sampling_topk', 'sampling_topp', 'repeat_penalty')
CASES = {
    'greedy_penalty': dict(V=61, B=3, S=7, max_out=8, return_scores=True, sampling_temperature=0, repeat_penalty=1.3),
    'greedy_prompts': dict(V=61, B=4, S=6, max_out=6, return_scores=True, sampling_temperature=0, prompts=True,
                           blacklist=[1, 5, 6]),
    'greedy_stop': dict(V=61, B=3, S=7, max_out=8, sampling_temperature=0, stop_from=(0, 2, 4)),
    'topk1': dict(V=61, B=2, S=7, max_out=5, sampling_topk=1),
    'topk': dict(V=251, B=2, S=7, max_out=5, return_scores=True, sampling_topk=5),
    'topp': dict(V=61, B=4, S=6, max_out=6, return_scores=True, sampling_topp=0.8, prompts=True),
    'full': dict(V=61, B=3, S=7, max_out=6, return_scores=True, repeat_penalty=1.2),
}


def prompt_of(case, cfg, seed):
    """(B, 3): BOS + two prompt tokens on the even rows, BOS + padding on the odd ones"""
    B = case['B']
    p = torch.full((B, 1), cfg.bos_idx, dtype=torch.long)
    if case.get('prompts'):
        rs = np.random.RandomState(seed)
        code = torch.from_numpy(rs.randint(8, case['V'], size=(B, 2)).astype(np.int64))  # (clear of the blacklist)
        code[1::2] = cfg.padding_idx
        p = torch.cat([p, code], dim=1)
    return p


class RuleDraws:
    """stands in for torch.Tensor.multinomial during one search"""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)
        self.uniforms, self.equal_weights = [], False

    def __call__(self, probs, num_samples, replacement=False, **kw):
        assert num_samples == 1 and probs.dim() == 2
        u = torch.from_numpy(np.floor(self.rs.random_sample(probs.size(0)) * 2 ** 24) / 2 ** 24)
        self.uniforms.append(u.float())
        w, pos = probs.double().sort(dim=-1, descending=True, stable=True)
        self.equal_weights |= bool(((w[:, 1:] == w[:, :-1]) & (w[:, 1:] > 0)).any())
        cum = w.cumsum(dim=-1)
        idx = (cum <= (u * cum[:, -1])[:, None]).sum(dim=-1).clamp(max=probs.size(1) - 1)
        return pos.gather(1, idx[:, None])


def run(case, seed, stop_sequences=()):
    cfg, model = MG.build_model(case['V'], **TINY)
    MG.load_params(model, seed)
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
    draws = RuleDraws(seed)
    stock = torch.Tensor.multinomial
    torch.Tensor.multinomial = lambda self, *a, **k: draws(self, *a, **k)
    opts = {k: case[k] for k in OPTS if k in case}
    stops = [torch.tensor(s, dtype=torch.long) for s in stop_sequences]
    try:
        with torch.no_grad():
            enc_out, enc_mask, _ = model.encoder(MG.t(batch['encoder_input']), MG.t(batch['encoder_input_length']))
            prompt = prompt_of(case, cfg, seed)
            steps = [{k: v.clone() for k, v in out.items()} for out in decoding.sample_on_the_fly(
                dec, enc_out, enc_mask, case['max_out'], {}, decoder_input=prompt, blacklist=case.get('blacklist', []),
                stop_sequences=stops, **opts)]
    finally:
        dec.forward = inner
        torch.Tensor.multinomial = stock
    uniforms = torch.stack(draws.uniforms) if draws.uniforms else torch.zeros(len(steps), case['B'])
    # the restatement over the same logits: must give the same search; its statistics are the fixture's
    feed_log = iter(logits)
    stats = {}
    mine = sample_ref(lambda feed: next(feed_log), prompt, case['max_out'], cfg.decoder_max_len, cfg.padding_idx, cfg.eos_idx,
                      blacklist=case.get('blacklist', []), stop_sequences=stop_sequences, uniforms=uniforms, stats=stats,
                      **opts)
    same = stats['rows'] == rows and len(mine) == len(steps) and all(torch.equal(a['tokens'], b['tokens'])
                                                                      for a, b in zip(mine, steps))
    last = torch.stack([x[:, -1] for x in logits])
    return cfg, prompt, steps, rows, uniforms, stats, same, draws.equal_weights, last


def main():
    out = {'cases': np.array(sorted(CASES))}
    for name, case in CASES.items():
        for seed in range(100, 1100):
            stop = []
            if 'stop_from' in case:  # a stop sequence that fires: tokens the unstopped search of this seed produced
                row, a, b = case['stop_from']
                plain = run(case, seed)[2]
                stop = [torch.cat([s['tokens'] for s in plain], dim=1)[row, a:b].tolist()]
            cfg, prompt, steps, rows, uniforms, stats, same, equal, last = run(case, seed, stop)
            margins = {k: float(stats[k].min()) for k in ('draw_margin', 'boundary_margin', 'greedy_gap')}
            ok = (same and not equal and margins['draw_margin'] >= 1e-3 and margins['boundary_margin'] >= 1e-3
                  and margins['greedy_gap'] >= 1e-3 * stats['max_logit'])
            if 'stop_from' in case:
                ok = ok and len(steps) < len(plain)
            if ok:
                break
        else:
            raise RuntimeError(f'case {name}: no usable seed')
        print(f'case {name}: seed {seed}, {len(steps)} steps, rows per call {rows}, margins {margins}, max|logit| '
              f'{stats["max_logit"]:.3f}')
        p = name + ':'
        out.update({p + 'cfg': MG.cfg_json(cfg), p + 'V': case['V'], p + 'B': case['B'], p + 'S': case['S'], p + 'seed': seed,
                    p + 'max_output_len': case['max_out'], p + 'prompt': MG.npy(prompt), p + 'rows': np.array(rows),
                    p + 'blacklist': np.array(case.get('blacklist', []), dtype=np.int64),
                    p + 'stop_sequence': np.array(stop[0] if stop else [], dtype=np.int64),
                    p + 'uniforms': MG.npy(uniforms), p + 'logits': MG.npy(last), p + 'max_logit': stats['max_logit'],
                    p + 'widths': np.array([s['tokens'].size(1) for s in steps]),
                    p + 'tokens': MG.npy(torch.cat([s['tokens'] for s in steps], dim=1))})
        out.update({p + k: case.get(k, d) for k, d in (('return_scores', False), ('sampling_temperature', 1.0),
                                                        ('sampling_topk', 0), ('sampling_topp', 1.0), ('repeat_penalty', 1.0))})
        out.update({p + k: v for k, v in margins.items()})
        if case.get('return_scores'):
            out[p + 'pos_scores'] = MG.npy(torch.cat([s['pos_scores'] for s in steps], dim=1))
    path = os.path.join(MG.OUT, 'sampling_search.npz')
    np.savez_compressed(path, **out)  # (the cfg strings are UTF-32: they shrink tenfold)
    print(f'wrote {path}: {os.path.getsize(path) / 1e3:.1f} kB')


if __name__ == '__main__':
    main()
