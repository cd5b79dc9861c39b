#!/usr/bin/env python3
"""tests/golden/moe_decode.npz: INCREMENTAL decoding of the REAL reference's `moe_transformer` (pasero/models/
mixture_of_experts.py, moe_impl='basic', CPU fp32) on the tiny model of moe.npz — d = 128, 2 heads, 2 encoder and 2 decoder
layers, ffn 128, E = 4, V = 61, dropout 0, weights from paramgen seeds — for tests/test_moe_decode_gpu.py.  The searches of
moe.npz end at their first token, so nothing there pins the decoder's incremental path.  Data only.

Two decoder variants:   mix  decoder_expert_interval=2 (a dense and a mixture layer)
                        all  decoder_expert_interval=1 (every layer a mixture: layer 0 has no fc1)
Per variant:
  tf:*      teacher-forced incremental decoding: random tokens in [4, V), B = 4, 7 positions; the first call gets one token,
            then one token per call through `state`.  Recorded: the logits of every call after the first and every mixture
            layer's gate values of those calls (through `return_layers`).
  greedy:*  one greedy search, B = 3;   beam:*  one beam search, K = 3, B = 3; max_output_len 8: every hypothesis and score,
            and the rows the decoder saw at every call.
  shrink:*  one more beam search, K = 3, B = 4, on a model of its own (`shrink:seed`: weights and source batch) — the first
            seed for which a sentence leaves the batch (the rows per call change) and the min_gap and gate_gap rules hold.

Seed rule (checked here, the fields stored): at least two hypotheses per search have >= 4 tokens (native steps actually run);
`min_gap` >= 1e-3 * `max_logit` — greedy: the smallest top-1 / top-2 logit difference of any row at any call; beam: the
smallest difference between neighbouring finite scores among the best 2K + 1 of any sentence at any step (tests/beam_ref.py
over the reference decoder's logits, which also checks that restatement against the reference); `gate_gap` >= 1e-3: the
smallest rank-2 / rank-3 gate-value difference of any row at any mixture call of the decoder (teacher-forced calls and
searches); `experts_used` >= 3 of the 4 experts chosen at rank 1 or 2 during the searches; `differs_with_rolled_gate`: the
same searches with every decoder gate's rows rolled by one expert give other tokens for at least one sentence — a search that
ignored the routing would not reproduce the fixture.  Seeds are scanned until one passes.

Runs where the reference tree is importable (oracle/make_golden.py says how):  python tools/make_moe_decode_golden.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import make_golden as MG  # noqa: E402  (imports the reference, stubs its absent third-party modules)
import paramgen  # noqa: E402
from beam_ref import beam_ref  # noqa: E402

torch, config, decoding = MG.torch, MG.config, MG.decoding
from pasero.models import mixture_of_experts as ref_moe  # noqa: E402

V, S = 61, 7
TINY = dict(embed_dim=128, encoder_ffn_dim=128, decoder_ffn_dim=128, encoder_attention_heads=2, decoder_attention_heads=2,
            encoder_layers=2, decoder_layers=2, dropout=0.0)
MOE = dict(encoder_expert_count=4, decoder_expert_count=4, encoder_expert_interval=2, load_balancing=0.01, moe_impl='basic')
MOE_KEYS = ['encoder_expert_count', 'decoder_expert_count', 'encoder_expert_dim', 'decoder_expert_dim',
            'encoder_expert_layer_ids', 'decoder_expert_layer_ids', 'encoder_expert_interval', 'decoder_expert_interval',
            'moe_impl', 'capacity_factor', 'load_balancing']
VARIANTS = {'mix': 2, 'all': 1}
TF_B, TF_T, SEARCH_B, SHRINK_B, BEAM_K, MAX_OUT = 4, 7, 3, 4, 3, 8


def build(interval, seed):
    cfg = config.MOETransformerConfig(**TINY, **MOE, decoder_expert_interval=interval)
    if cfg.label_smoothing is None:
        cfg.label_smoothing = 0.1
    cfg.model_type = cfg.model_type or 'encoder_decoder'
    cfg.decoder_max_len = cfg.decoder_max_len or 256
    model = ref_moe.MOETransformer(cfg, config.DistributedConfig(), MG.FakeTask(V))
    MG.load_params(model, seed)
    model.eval()
    return cfg, model


class GateSpy:
    """over the decoder's gates while installed: the smallest rank-2 / rank-3 gate-value gap and the experts chosen"""

    def __init__(self, model):
        self.gates = [m for m in model.decoder.modules() if isinstance(m, ref_moe.Top2Gate)]
        self.gap, self.used = float('inf'), set()

    def __enter__(self):
        for g in self.gates:
            g.forward = self.wrap(g.forward)
        return self

    def __exit__(self, *exc):
        for g in self.gates:
            del g.forward

    def wrap(self, inner):
        def forward(input, input_mask=None):
            out = inner(input, input_mask)
            gv = out[2].detach()[~input_mask]
            if gv.size(0):
                top = gv.topk(3)
                self.gap = min(self.gap, float((top.values[:, 1] - top.values[:, 2]).min()))
                self.used |= set(top.indices[:, :2].flatten().tolist())
            return out
        return forward


def encode(model, batch):
    with torch.no_grad():
        enc_out, enc_mask, _ = model.encoder(MG.t(batch['encoder_input']), MG.t(batch['encoder_input_length']))
    return enc_out, enc_mask


def teacher_forced(model, seed):
    dec = model.decoder
    batch = paramgen.make_text_batch(seed, TF_B, S, 5, V)
    tokens = torch.from_numpy(np.random.RandomState(seed).randint(4, V, size=(TF_B, TF_T)).astype(np.int64))
    keys = [layer.gate_key for layer in dec.layers if hasattr(layer, 'gate_key')]
    enc_out, enc_mask = encode(model, batch)
    state, logits, gates = {}, [], {k: [] for k in keys}
    with torch.no_grad(), GateSpy(model) as spy:
        dec(enc_out, enc_mask, tokens[:, :1], state=state)
        for i in range(1, TF_T):
            out, layers = dec(enc_out, enc_mask, tokens[:, i:i + 1], state=state, return_layers=keys)
            logits.append(out[:, -1])
            for k in keys:
                gates[k].append(layers[k][:, -1])
    out = {'tokens': MG.npy(tokens), 'logits': MG.npy(torch.stack(logits)), 'gate_keys': np.array(keys)}
    for k in keys:
        out['gate:' + k] = MG.npy(torch.stack(gates[k]))
    return out, spy.gap


def searches(cfg, model, seed, kinds=('greedy', 'beam'), B=SEARCH_B):
    """-> {kind: (hyps, stats with the rows per call)}, gate gap, experts used, the restatement agrees"""
    dec = model.decoder
    batch = paramgen.make_text_batch(seed, B, S, 5, V)
    enc_out, enc_mask = encode(model, batch)
    prompt = torch.full((B, 1), cfg.bos_idx, dtype=torch.long)
    inner, res, same = dec.forward, {}, True
    with GateSpy(model) as spy:
        for kind in kinds:
            rows, logits = [], []

            def tap(encoder_out, encoder_mask, decoder_input, **kw):
                out = inner(encoder_out, encoder_mask, decoder_input, **kw)
                rows.append(encoder_out.size(0))
                logits.append(out[0].detach().clone())
                return out
            dec.forward = tap
            try:
                with torch.no_grad():
                    if kind == 'greedy':
                        hyps = decoding.sampling(dec, enc_out, enc_mask, MAX_OUT, {}, decoder_input=prompt,
                                                 sampling_temperature=0, return_scores=True)
                        for nbest in hyps:
                            nbest[0]['score'] = nbest[0]['pos_scores'].sum()
                    else:
                        hyps = decoding.beam_search(dec, enc_out, enc_mask, MAX_OUT, BEAM_K, {}, decoder_input=prompt)
            finally:
                dec.forward = inner
            if kind == 'greedy':
                top2 = torch.cat([x[:, -1].float().topk(2, dim=-1).values for x in logits])
                stats = {'min_gap': float((top2[:, 0] - top2[:, 1]).min()), 'max_logit': float(max(x.abs().max() for x in logits))}
            else:
                feed_log, stats = iter(logits), {}
                mine = beam_ref(lambda feed: next(feed_log), lambda idx: None, prompt, BEAM_K, MAX_OUT, cfg.decoder_max_len,
                                cfg.padding_idx, cfg.eos_idx, stats=stats)
                same = stats['rows'] == rows and all(
                    len(a) == len(b) and all(torch.equal(x['tokens'], y['tokens']) for x, y in zip(a, b)) for a, b in zip(hyps, mine))
            stats['rows'] = rows
            res[kind] = (hyps, stats)
    return res, spy.gap, spy.used, same


def tokens_of(res):
    return {kind: [[h['tokens'].tolist() for h in nbest] for nbest in hyps] for kind, (hyps, _) in res.items()}


def roll_gates(model, shift):
    for m in model.decoder.modules():
        if isinstance(m, ref_moe.Top2Gate):
            m.weight.data = m.weight.data.roll(shift, 0)


def main():
    out = {'variants': np.array(sorted(VARIANTS)), 'V': V, 'S': S, 'max_output_len': MAX_OUT, 'beam_size': BEAM_K}
    for name, interval in VARIANTS.items():
        for seed in range(1, 2000):
            cfg, model = build(interval, seed)
            tf, tf_gap = teacher_forced(model, seed)
            res, gap, used, same = searches(cfg, model, seed)
            long_enough = all(sum(len(h['tokens']) >= 4 for nbest in hyps for h in nbest) >= 2 for hyps, _ in res.values())
            gaps_ok = all(st['min_gap'] >= 1e-3 * st['max_logit'] for _, st in res.values())
            ok = same and long_enough and gaps_ok and min(gap, tf_gap) >= 1e-3 and len(used) >= 3
            differs = False
            if ok:
                roll_gates(model, 1)
                rolled = tokens_of(searches(cfg, model, seed)[0])
                roll_gates(model, -1)
                mine = tokens_of(res)
                differs = any(a != b for kind in mine for a, b in zip(mine[kind], rolled[kind]))
            print(f'{name} seed {seed}: restated {same}, long enough {long_enough}, gaps ok {gaps_ok}, gate gap '
                  f'{min(gap, tf_gap):.2e}, experts used {len(used)}, differs with rolled gate {differs}')
            if ok and differs:
                break
        else:
            raise RuntimeError(f'variant {name}: no usable seed')
        for shrink_seed in range(1, 4000):
            cfg_s, model_s = build(interval, shrink_seed)
            extra, gap_s, _, same_s = searches(cfg_s, model_s, shrink_seed, kinds=('beam',), B=SHRINK_B)
            st = extra['beam'][1]
            if same_s and len(set(st['rows'])) > 1 and st['min_gap'] >= 1e-3 * st['max_logit'] and gap_s >= 1e-3:
                break
        else:
            raise RuntimeError(f'variant {name}: no seed whose beam search shrinks its batch')
        print(f'{name}: seed {shrink_seed} shrinks, rows per call {st["rows"]}')
        res['shrink'] = extra['beam']
        p = name + ':'
        out.update({p + 'cfg': MG.cfg_json(cfg), p + 'moe_cfg': np.array(json.dumps({k: getattr(cfg, k) for k in MOE_KEYS})),
                    p + 'seed': seed, p + 'gate_gap': min(gap, tf_gap), p + 'experts_used': len(used),
                    p + 'differs_with_rolled_gate': bool(differs), p + 'tf:B': TF_B, p + 'search:B': SEARCH_B, p + 'shrink:B': SHRINK_B,
                    p + 'shrink:seed': shrink_seed})
        out.update({p + 'tf:' + k: v for k, v in tf.items()})
        for kind, (hyps, stats) in res.items():
            r = f'{p}{kind}:'
            out.update({r + 'min_gap': stats['min_gap'], r + 'max_logit': stats['max_logit'],
                        r + 'n_hyps': np.array([len(nb) for nb in hyps]), r + 'rows': np.array(stats['rows']),
                        r + 'n_long': sum(len(h['tokens']) >= 4 for nbest in hyps for h in nbest)})
            for b, nbest in enumerate(hyps):
                for i, h in enumerate(nbest):
                    out[f'{r}{b}:{i}:tokens'] = MG.npy(h['tokens'])
                    out[f'{r}{b}:{i}:score'] = float(h['score'])
    path = os.path.join(MG.OUT, 'moe_decode.npz')
    np.savez_compressed(path, **out)  # (the cfg strings are UTF-32: they shrink tenfold)
    print(f'wrote {path}: {os.path.getsize(path) / 1e3:.1f} kB')


if __name__ == '__main__':
    main()
