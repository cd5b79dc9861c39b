#!/usr/bin/env python3
"""tests/golden/moe.npz: the REAL reference's `moe_transformer` (pasero/models/mixture_of_experts.py, moe_impl='basic', CPU fp32)
on a tiny model — d = 128, 2 heads, 2 encoder and 2 decoder layers, ffn 128, expert interval 2 (one dense and one MoE layer per
stack), E = 4, load_balancing 0.01, dropout 0, V = 61, weights from paramgen seeds.  Data only:

  layer:*   one MoE layer alone (the encoder's) on an input with padding tokens, one sentence tail fully padded from its third
            position: output, gate_value, lb_loss, and the gradients of the input, the gate and every expert parameter of
            sum(y * dy) + lb_weight * lb_loss for a recorded dy
  model:*   one training step (loss, logs, gradients: fp64 norms and sums of all, every 16th element of each) and one greedy
            search (tokens, scores)
  param_names / param_shapes, `cfg` (the fixtures' usual schema) and `moe_cfg` (the options moe_transformer adds, as JSON)

Seed rule (checked here, stored as `min_gap`): in every recorded MoE call each real token's gate values at ranks 1, 2, 3
differ pairwise by >= 1e-3 and every expert receives a token (so the zero-gradient-for-unused-experts difference never
enters); the greedy top-1 / top-2 logit gap is >= 1e-3 * max|logit|.

Runs where the reference tree is importable (oracle/make_golden.py says how):  python tools/make_moe_golden.py"""
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
from pasero.models import mixture_of_experts as ref_moe  # noqa: E402

V, B, S, T = 61, 3, 7, 5
TINY = dict(embed_dim=128, encoder_ffn_dim=128, decoder_ffn_dim=128, encoder_attention_heads=2, decoder_attention_heads=2,
            encoder_layers=2, decoder_layers=2, dropout=0.0)
MOE = dict(encoder_expert_count=4, decoder_expert_count=4, encoder_expert_interval=2, decoder_expert_interval=2,
           load_balancing=0.01, moe_impl='basic')
MOE_KEYS = ['encoder_expert_count', 'decoder_expert_count', 'encoder_expert_dim', 'decoder_expert_dim',
            'encoder_expert_layer_ids', 'decoder_expert_layer_ids', 'encoder_expert_interval', 'decoder_expert_interval',
            'moe_impl', 'capacity_factor', 'load_balancing']
LB_WEIGHT, MAX_OUT, GRAD_STRIDE = 0.7, 8, 16


def build(seed):
    cfg = config.MOETransformerConfig(**TINY, **MOE)
    if cfg.label_smoothing is None:
        cfg.label_smoothing = 0.1
    cfg.model_type = cfg.model_type or 'encoder_decoder'
    cfg.decoder_max_len = cfg.decoder_max_len or 256
    model = ref_moe.MOETransformer(cfg, config.DistributedConfig(), MG.FakeTask(V))
    names_shapes = MG.load_params(model, seed)
    return cfg, model, names_shapes


class GateSpy:
    """rank gaps and expert loads of every MoE call while it is installed"""

    def __init__(self, model):
        self.gates = [m for m in model.modules() if isinstance(m, ref_moe.Top2Gate)]
        self.min_gap, self.all_used = float('inf'), True

    def __enter__(self):
        self.inner = [g.forward for g in self.gates]
        for g, inner in zip(self.gates, self.inner):
            g.forward = self.wrap(inner)
        return self

    def __exit__(self, *exc):
        for g in self.gates:
            del g.forward

    def wrap(self, inner):
        def forward(input, input_mask=None):
            out = inner(input, input_mask)
            gv = out[2].detach()[~input_mask]
            if gv.size(0):
                top = gv.topk(3).values
                gaps = torch.stack([top[:, 0] - top[:, 1], top[:, 1] - top[:, 2]])
                self.min_gap = min(self.min_gap, float(gaps.min()))
                used = torch.zeros(gv.size(1), dtype=torch.bool)
                used[gv.topk(2).indices.flatten()] = True
                self.all_used &= bool(used.all())
            return out
        return forward


def layer_case(model, seed):
    layer = model.encoder.layers[1].moe_layer
    D = TINY['embed_dim']
    x = MG.t(paramgen.make_array(seed, 'moe_layer_x', (B, T, D))).requires_grad_()
    dy = MG.t(paramgen.make_array(seed, 'moe_layer_dy', (B, T, D)))
    pad = torch.zeros(B, T, dtype=torch.bool)
    pad[1, 3:] = True
    pad[2, 2:] = True
    model.zero_grad(set_to_none=True)
    with GateSpy(model) as spy:
        y, gate_value, _ = layer(x, pad)
    ((y * dy).sum() + LB_WEIGHT * layer.lb_loss).backward()
    out = {'x': MG.npy(x), 'dy': MG.npy(dy), 'pad': MG.npy(pad), 'y': MG.npy(y), 'gate_value': MG.npy(gate_value),
           'lb_loss': float(layer.lb_loss.detach()), 'lb_weight': LB_WEIGHT, 'dx': MG.npy(x.grad), 'prefix': 'encoder.layers.1.moe_layer.'}
    for name, p in layer.named_parameters():
        if p.grad is None:  # (an unused expert: the seed is rejected)
            spy.all_used = False
            continue
        out['grad:' + name] = MG.npy(p.grad)
    return {'layer:' + k: v for k, v in out.items()}, spy


def model_case(cfg, model, seed):
    batch = paramgen.make_text_batch(seed, B, S, T, V)
    tb = {k: MG.t(v) for k, v in batch.items()}
    model.train()
    model.zero_grad(set_to_none=True)
    with GateSpy(model) as spy:
        loss, logs = model(**tb)
        loss.backward()
        grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
        complete = len(grads) == len(list(model.named_parameters()))  # (an unused expert keeps .grad None)
        out = {'loss': MG.npy(loss), **{'logs_' + k: float(v) for k, v in logs.items()},
               'grad_names': np.array(list(grads)),
               'grad_norms': np.array([g.double().norm().item() for g in grads.values()]),
               'grad_sums': np.array([g.double().sum().item() for g in grads.values()]), 'grad_stride': GRAD_STRIDE}
        for k, g in grads.items():
            out['gradsample:' + k] = MG.npy(g.reshape(-1)[::GRAD_STRIDE])
        model.eval()
        dec, logits = model.decoder, []
        inner = dec.forward

        def spy_forward(encoder_out, encoder_mask, decoder_input, **kw):
            res = inner(encoder_out, encoder_mask, decoder_input, **kw)
            logits.append(res[0].detach().clone())
            return res
        dec.forward = spy_forward
        prompt = torch.full((B, 1), cfg.bos_idx, dtype=torch.long)
        try:
            with torch.no_grad():
                enc_out, enc_mask, _ = model.encoder(tb['encoder_input'], tb['encoder_input_length'])
                hyps = decoding.sampling(dec, enc_out, enc_mask, MAX_OUT, {}, decoder_input=prompt, sampling_temperature=0,
                                         return_scores=True)
        finally:
            dec.forward = inner
    top2 = torch.cat([x[:, -1].float().topk(2, dim=-1).values for x in logits])
    out.update({'search_min_gap': float((top2[:, 0] - top2[:, 1]).min()),
                'search_max_logit': float(max(x.abs().max() for x in logits)), 'max_output_len': MAX_OUT})
    for b, nbest in enumerate(hyps):
        out[f'search:{b}:tokens'] = MG.npy(nbest[0]['tokens'])
        out[f'search:{b}:score'] = float(nbest[0]['pos_scores'].sum())
    spy.all_used &= complete
    return {'model:' + k: v for k, v in out.items()}, spy


def main():
    for seed in range(1, 400):
        cfg, model, names_shapes = build(seed)
        layer_out, spy_l = layer_case(model, seed)
        model_out, spy_m = model_case(cfg, model, seed)
        min_gap = min(spy_l.min_gap, spy_m.min_gap)
        ok = (min_gap >= 1e-3 and spy_l.all_used and spy_m.all_used
              and model_out['model:search_min_gap'] >= 1e-3 * model_out['model:search_max_logit'])
        print(f'seed {seed}: gate rank gap {min_gap:.2e}, every expert used {spy_l.all_used and spy_m.all_used}, greedy gap '
              f'{model_out["model:search_min_gap"]:.2e} / max|logit| {model_out["model:search_max_logit"]:.2f}')
        if ok:
            break
    else:
        raise RuntimeError('no usable seed')
    out = {'cfg': MG.cfg_json(cfg), 'moe_cfg': np.array(json.dumps({k: getattr(cfg, k) for k in MOE_KEYS})),
           'arch': 'moe_transformer', 'V': V, 'B': B, 'S': S, 'T': T, 'seed': seed, 'min_gap': min_gap,
           **MG.names_shapes_arrays(names_shapes), **layer_out, **model_out}
    path = os.path.join(MG.OUT, 'moe.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {os.path.getsize(path) / 1e3:.1f} kB')


if __name__ == '__main__':
    main()
