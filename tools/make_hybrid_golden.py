#!/usr/bin/env python3
"""tests/golden/hybrid.npz: the REAL reference's `hybrid_transformer` (pasero/models/hybrid.py, CPU fp32) on a tiny model —
d = 128, 2 encoder heads, 2 encoder layers, 2 LSTM layers of hidden size 64 (so `out_proj` exists), decoder_embed_proj,
V = 61, dropout 0, B = 3 sentences of different source lengths, weights from paramgen seeds.  Data only:

  loss, logs_*, grad_*     one training step: fp64 norms and sums of every gradient, every 16th element of each
  enc_out, enc_mask        the encoder's output for the batch (what the decoder-only replays start from)
  logits                   teacher-forced decoder logits (B, T, V)
  inc_logits               the same positions computed incrementally, one token per call, from an empty state
  attn_probs               `dec_1_cross_attn` of the teacher-forced call (B, T, 1, S)
  state_shapes             shapes of prev_hiddens, prev_cells, attn_key after the first incremental call
  greedy:* / beam:*        a greedy search and a beam search (K = 3) from an explicit BOS prompt: tokens and scores
  param_names / param_shapes (this configuration), `same:` (hidden = d: no out_proj, no embed_proj) and `untied:`
  (untied output projection, unshared embeddings), `cfg` (the fixtures' usual schema), `hybrid_cfg` (the options
  hybrid_transformer adds, as JSON)

Seed rule (checked here, stored as search_min_gap / search_max_logit): at every step of both searches the top-1 / top-2 logit
gap of every row is >= 1e-3 * max|logit|; some greedy output has three tokens or more and some best beam hypothesis more than
one (a tiny random model likes to end at once).

Runs where the reference tree is importable (oracle/make_golden.py says how):  python tools/make_hybrid_golden.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import make_golden as MG  # noqa: E402  (imports the reference, stubs its absent third-party modules)
import paramgen  # noqa: E402

torch, config, decoding = MG.torch, MG.config, MG.decoding
from pasero.models import hybrid as ref_hybrid  # noqa: E402

V, B, S, T = 61, 3, 7, 5
TINY = dict(embed_dim=128, encoder_ffn_dim=128, encoder_attention_heads=2, encoder_layers=2, dropout=0.0)
HYBRID = dict(decoder_layers=2, decoder_hidden_size=64, decoder_embed_proj=True)
HYBRID_KEYS = ['decoder_hidden_size', 'decoder_embed_proj']
MAX_OUT, BEAM, GRAD_STRIDE = 8, 3, 16


def build(seed, **overrides):
    cfg = config.HybridTransformerConfig(**{**TINY, **HYBRID, **overrides})
    if cfg.label_smoothing is None:
        cfg.label_smoothing = 0.1
    cfg.model_type = cfg.model_type or 'encoder_decoder'
    cfg.decoder_max_len = cfg.decoder_max_len or 256
    model = ref_hybrid.HybridTransformer(cfg, config.DistributedConfig(), MG.FakeTask(V))
    names_shapes = MG.load_params(model, seed)
    return cfg, model, names_shapes


class LogitSpy:
    """the logits of every decoder call while it is installed"""

    def __init__(self, dec):
        self.dec, self.logits = dec, []

    def __enter__(self):
        inner = self.inner = self.dec.forward

        def forward(encoder_out, encoder_mask, decoder_input, **kw):
            res = inner(encoder_out, encoder_mask, decoder_input, **kw)
            self.logits.append(res[0].detach().clone())
            return res
        self.dec.forward = forward
        return self

    def __exit__(self, *exc):
        self.dec.forward = self.inner

    def gap(self):
        top2 = torch.cat([x[:, -1].float().topk(2, dim=-1).values for x in self.logits])
        return float((top2[:, 0] - top2[:, 1]).min()), float(max(x.abs().max() for x in self.logits))


def record(cfg, model, seed):
    batch = paramgen.make_text_batch(seed, B, S, T, V)
    tb = {k: MG.t(v) for k, v in batch.items()}
    assert len(set(batch['encoder_input_length'].tolist())) > 1, 'the sentences must differ in source length'
    model.train()
    model.zero_grad(set_to_none=True)
    loss, logs = model(**tb)
    loss.backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert all(g is not None for g in grads.values())
    out = {'loss': MG.npy(loss), **{'logs_' + k: float(v) for k, v in logs.items()},
           'grad_names': np.array(list(grads)),
           'grad_norms': np.array([g.double().norm().item() for g in grads.values()]),
           'grad_sums': np.array([g.double().sum().item() for g in grads.values()]), 'grad_stride': GRAD_STRIDE}
    for k, g in grads.items():
        out['gradsample:' + k] = MG.npy(g.reshape(-1)[::GRAD_STRIDE])
    model.eval()
    dec = model.decoder
    dec_in = tb['decoder_input'][:, :-1]
    with torch.no_grad():
        enc_out, enc_mask, _ = model.encoder(tb['encoder_input'], tb['encoder_input_length'])
        logits, layers = dec(enc_out, enc_mask, dec_in, return_layers=[dec.cross_attn_key])
        state, inc = {}, []
        for t in range(dec_in.size(1)):
            step, _ = dec(enc_out, enc_mask, dec_in[:, t:t + 1], state=state)
            inc.append(step)
            if t == 0:
                shapes = {k: list(v.shape) for k, v in state.items()}
        inc = torch.cat(inc, dim=1)
        prompt = torch.full((B, 1), cfg.bos_idx, dtype=torch.long)
        with LogitSpy(dec) as spy_g:
            greedy = decoding.sampling(dec, enc_out, enc_mask, MAX_OUT, {}, decoder_input=prompt, sampling_temperature=0,
                                       return_scores=True)
        with LogitSpy(dec) as spy_b:
            beam = decoding.beam_search(dec, enc_out, enc_mask, MAX_OUT, BEAM, {}, decoder_input=prompt, return_scores=True)
    out.update({'enc_out': MG.npy(enc_out), 'enc_mask': MG.npy(enc_mask), 'logits': MG.npy(logits), 'inc_logits': MG.npy(inc),
                'attn_probs': MG.npy(layers[dec.cross_attn_key]), 'attn_key_name': dec.cross_attn_key,
                'state_shapes': np.array(json.dumps(shapes)), 'inc_vs_full': float((inc - logits).abs().max()),
                'max_output_len': MAX_OUT, 'beam_size': BEAM})
    (gap_g, max_g), (gap_b, max_b) = spy_g.gap(), spy_b.gap()
    out.update({'search_min_gap': min(gap_g, gap_b), 'search_max_logit': max(max_g, max_b)})
    ok = gap_g >= 1e-3 * max_g and gap_b >= 1e-3 * max_b
    for b, nbest in enumerate(greedy):
        out[f'greedy:{b}:tokens'] = MG.npy(nbest[0]['tokens'])
        out[f'greedy:{b}:score'] = float(nbest[0]['pos_scores'].sum())
    out['beam:n_hyps'] = np.array([len(nb) for nb in beam])
    for b, nbest in enumerate(beam):
        for i, h in enumerate(nbest):
            out[f'beam:{b}:{i}:tokens'] = MG.npy(h['tokens'])
            out[f'beam:{b}:{i}:score'] = float(h['score'])
    # searches worth replaying: a greedy output of three tokens or more, a best beam hypothesis longer than one token
    ok = ok and max(len(nb[0]['tokens']) for nb in greedy) >= 3 and max(len(nb[0]['tokens']) for nb in beam) > 1
    return out, ok


def main():
    for seed in range(1, 400):
        cfg, model, names_shapes = build(seed)
        out, ok = record(cfg, model, seed)
        print(f'seed {seed}: search gap {out["search_min_gap"]:.2e} / max|logit| {out["search_max_logit"]:.2f}, incremental vs '
              f'teacher-forced {out["inc_vs_full"]:.1e}')
        if ok:
            break
    else:
        raise RuntimeError('no usable seed')
    layouts = {}
    for tag, kw in (('same:', dict(decoder_hidden_size=128, decoder_embed_proj=False)),
                    ('untied:', dict(tied_output_projection=False, shared_embeddings=False))):
        _, _, ns = build(seed, **kw)
        layouts.update({tag + k: v for k, v in MG.names_shapes_arrays(ns).items()})
        layouts[tag + 'overrides'] = np.array(json.dumps(kw))
    out = {'cfg': MG.cfg_json(cfg), 'hybrid_cfg': np.array(json.dumps({k: getattr(cfg, k) for k in HYBRID_KEYS})),
           'arch': 'hybrid_transformer', 'V': V, 'B': B, 'S': S, 'T': T, 'seed': seed,
           **MG.names_shapes_arrays(names_shapes), **layouts, **out}
    path = os.path.join(MG.OUT, 'hybrid.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {os.path.getsize(path) / 1e3:.1f} kB (moe.npz: {os.path.getsize(os.path.join(MG.OUT, "moe.npz")) / 1e3:.1f} kB)')


if __name__ == '__main__':
    main()
