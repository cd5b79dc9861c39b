#!/usr/bin/env python3
"""Audit of the drop-in boundary against the reference (naver/pasero):
  1. every `cfg.<attr>` / `dist_cfg.<attr>` pasero_amd reads exists on the reference's configuration classes;
  2. every preset in pasero_amd/config.py has the reference's defaults (pasero/config.py MODEL_CONFIGS);
  3. the model classes the registry resolves to have the reference model's state_dict names / shapes and frozen sets;
  4. remap / update / clean_state_dict (Transformer and AdapterTransformer) turn the same synthetic checkpoints into the
     same keys and values, and the results load strictly.
Every check compares the same `facts()` taken of both implementations.  No forward pass runs (pasero_amd has no CPU
path).  Exit code 0 = clean.

  audit_against_reference.py --reference DIR        facts of the reference tree at DIR, taken now (and, with it on the
                                                    path, its registry must resolve to the pasero_amd classes)
  audit_against_reference.py --fixture FILE         facts of the reference as recorded in FILE (no reference needed:
                                                    tests/golden/reference_boundary.json, what the test suite checks)
  audit_against_reference.py --reference DIR --write FILE   record the reference's facts in FILE
"""
import argparse
import copy
import dataclasses
import glob
import json
import os
import re
import sys
import types
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
TASK_DEFAULTS = ('label_smoothing', 'model_type', 'decoder_max_len')  # set per task (config.py:1146-1153,1241-1272)
# (preset class, overrides, (encoder, decoder) vocabulary, adapter model?)
LAYOUTS = [('TransformerSmallConfig', dict(shared_embeddings=False), (300, 400), False),
           ('MBARTConfig', dict(encoder_layers=2, decoder_layers=2), (1000, 1000), False),
           ('WhisperConfig', dict(encoder_layers=2, decoder_layers=2), (0, 51865), False),
           ('AdapterTransformerConfig', dict(encoder_adapters=['a'], decoder_adapters=['a', 'b']), (500, 500), True),
           ('TransformerConfig', dict(lora_rank=4, encoder_layers=1, decoder_layers=1), (200, 200), False)]


def import_reference(ref_dir):
    # the two third-party imports absent from the image, stubbed as in oracle/make_golden.py
    sb, sbm = types.ModuleType('sacrebleu'), types.ModuleType('sacrebleu.metrics')
    sbm.METRICS = {'BLEU': type('B', (), {'TOKENIZERS': {}})}
    sb.metrics = sbm
    sys.modules['sacrebleu'], sys.modules['sacrebleu.metrics'] = sb, sbm
    names = ['stopes', 'stopes.pipelines', 'stopes.pipelines.monolingual', 'stopes.pipelines.monolingual.utils',
             'stopes.pipelines.monolingual.utils.text_normalizer']
    for n in names:
        sys.modules[n] = types.ModuleType(n)
    sys.modules[names[-1]].remove_non_printing_char = lambda s: s
    sys.modules[names[-1]].replace_unicode_punct = lambda s: s
    sys.path.insert(0, ref_dir)
    from pasero import config as RC
    from pasero.models import transformer as RT, adapters as RA
    return types.SimpleNamespace(C=RC, Transformer=RT.Transformer, AdapterTransformer=RA.AdapterTransformer,
                                 presets=RC.MODEL_CONFIGS)


def ours():
    import pasero_amd.config as MC
    import pasero_amd.transformer as T
    import pasero_amd.adapters as A
    return types.SimpleNamespace(C=MC, Transformer=T.Transformer, AdapterTransformer=A.AdapterTransformer,
                                 presets=MC.CONFIGS)


class FakeTask:
    freeze_encoder_embed_mask = None

    def __init__(self, enc, dec):
        self.encoder_num_embeddings, self.decoder_num_embeddings = enc, dec

    def remap_encoder_embed(self, e): return e * 2
    def remap_decoder_embed(self, e): return e * 3


def _plain(v):
    try:
        return json.loads(json.dumps(v))
    except (TypeError, ValueError):
        return repr(v)


def digest(t):
    """shape, sum, sum of |x| and a position-weighted sum (catches permuted entries), in fp64"""
    import torch
    x = t.detach().double().reshape(-1)
    w = torch.sin(torch.arange(1, x.numel() + 1, dtype=torch.float64))
    return [list(t.shape), float(x.sum()), float(x.abs().sum()), float((x * w).sum())]


def synthetic_state(model):
    """the model's state_dict with every floating-point entry drawn from a generator seeded by its name: the same
    checkpoint for any implementation with the same names and shapes"""
    import torch
    sd = {}
    for k, v in model.state_dict().items():
        if v.is_floating_point():
            sd[k] = torch.randn(v.shape, generator=torch.Generator().manual_seed(zlib.crc32(k.encode()))).to(v.dtype)
        else:
            sd[k] = v.clone()
    return sd


def stale_checkpoint(sd, cfg):
    """what old fairseq / HuggingFace checkpoints look like"""
    import torch
    sd = {k: v.clone() for k, v in sd.items()}
    for layer in ('encoder.layers.0.self_attn', 'decoder.layers.1.encoder_attn'):
        for kind in ('weight', 'bias'):
            parts = [sd.pop(f'{layer}.{p}_proj.{kind}') for p in 'qkv']
            sd[f'{layer}.in_proj_{kind}'] = torch.cat(parts)
    sd['decoder.version'] = torch.tensor([3.0])
    sd['lm_head.weight'] = torch.zeros(3, 3)
    sd.pop('decoder.embed_tokens.weight', None)
    if 'decoder.layer_norm.weight' in sd:
        for kind in ('weight', 'bias'):
            sd[f'decoder.final_layer_norm.{kind}'] = sd.pop(f'decoder.layer_norm.{kind}')
    if cfg.tied_output_projection:
        sd['decoder.output_projection.weight'] = torch.zeros(5, 128)
    sd['encoder.embed_tokens.frozen_embedding.weight'] = torch.zeros(2, 2)
    return sd


def _frozen(m):
    return sorted(k for k, p in m.named_parameters() if not p.requires_grad)


def _strict_load(model, sd):
    try:
        model.load_state_dict(sd, strict=True)
        return None
    except Exception as e:  # noqa: BLE001
        return str(e)[:300]


def state_dict_plumbing(impl):
    """remap_state_dict / update_state_dict / clean_state_dict (transformer.py:382-497,584-592) applied to synthetic
    stale checkpoints -> {case: facts}"""
    import torch

    def small(**kw):
        cfg = impl.C.TransformerConfig(embed_dim=128, encoder_ffn_dim=64, decoder_ffn_dim=64, encoder_attention_heads=2,
                                       decoder_attention_heads=2, encoder_layers=2, decoder_layers=2, **kw)
        cfg.label_smoothing, cfg.model_type, cfg.decoder_max_len = 0.1, 'encoder_decoder', 64
        return cfg

    cases = [('post-norm, training', small(), True), ('pre-norm, inference', small(encoder_prenorm=True,
             decoder_prenorm=True), False), ('untied, unshared', small(tied_output_projection=False,
             shared_embeddings=False), True), ('lora training', small(lora_rank=4), True),
             ('lora inference', small(lora_rank=4), False), ('shifted layers', small(), True)]
    out = {}
    for tag, cfg, training in cases:
        if tag == 'shifted layers':
            cfg.shift_encoder_layers, cfg.shift_decoder_layers = 1, 0
        torch.manual_seed(0)
        model = impl.Transformer(cfg, impl.C.DistributedConfig(), FakeTask(50, 50)).train(training)
        start = synthetic_state(model)
        model.load_state_dict(start)
        sd = stale_checkpoint(start, cfg)
        if tag.startswith('lora') and training:  # a checkpoint of the backbone only: LoRA parameters are new
            sd = {k: v for k, v in sd.items() if '.lora.' not in k}
        model.remap_state_dict(sd)
        model.update_state_dict(sd)
        lora_new = tag == 'lora training'  # (their values are the model's own initialisation: shapes only)
        rec = {'updated': {k: ([list(v.shape)] if lora_new and '.lora.' in k else digest(v)) for k, v in sd.items()}}
        if tag != 'shifted layers':
            rec['strict_load'] = _strict_load(model, sd)
        clean = dict(model.state_dict())
        model.clean_state_dict(clean)
        rec['clean_keys'] = sorted(clean)
        out[tag] = rec
    return out


def adapter_plumbing(impl):
    """AdapterTransformer.update_state_dict / clean_state_dict (adapters.py:144-166): new adapters keep their
    initialisation when training on a backbone checkpoint, adapters the model does not hold are parked in
    `extra_adapters` and written back by clean_state_dict, missing adapters are disabled at inference -> {case: facts}"""
    import torch

    def cfg_for(enc, dec):
        cfg = impl.C.AdapterTransformerConfig(embed_dim=128, encoder_ffn_dim=64, decoder_ffn_dim=64,
                                              encoder_attention_heads=2, decoder_attention_heads=2, encoder_layers=2,
                                              decoder_layers=1, encoder_adapters=enc, decoder_adapters=dec)
        cfg.label_smoothing, cfg.model_type, cfg.decoder_max_len = 0.1, 'encoder_decoder', 64
        return cfg

    torch.manual_seed(1)
    donor = impl.AdapterTransformer(cfg_for(['a', 'x'], ['a', 'x']), impl.C.DistributedConfig(), FakeTask(40, 40))
    full = synthetic_state(donor)
    backbone = {k: v for k, v in full.items() if '.adapters.' not in k}
    out = {}
    for tag, enc, dec, training, ckpt in (('new adapters on a backbone', ['a'], ['a', 'b'], True, backbone),
                                          ('checkpoint holds other adapters', ['a'], ['a'], True, full),
                                          ('inference with a subset', ['a'], ['x', 'zz'], False, full)):
        model = impl.AdapterTransformer(cfg_for(enc, dec), impl.C.DistributedConfig(), FakeTask(40, 40)).train(training)
        model.load_state_dict(synthetic_state(model))
        sd = copy.deepcopy(ckpt)
        model.update_state_dict(sd)
        rec = {'updated': {k: digest(v) for k, v in sd.items()}, 'extra_adapters': sorted(model.extra_adapters),
               'strict_load': _strict_load(model, sd)}
        if rec['strict_load'] is None:
            clean = dict(model.state_dict())
            model.clean_state_dict(clean)
            rec['clean_keys'], rec['frozen'] = sorted(clean), _frozen(model)
        out[tag] = rec
    return out


def facts(impl):
    """everything the checks compare, of one implementation, as JSON-able data"""
    C = impl.C
    f = {'config_attrs': sorted(a for a in dir(C.AdapterTransformerConfig()) if not a.startswith('__')),
         'dist_attrs': sorted(a for a in dir(C.DistributedConfig()) if not a.startswith('__')),
         'presets': {}, 'layouts': {}}
    for name, cls in impl.presets.items():
        r = cls()
        f['presets'][name] = {a: _plain(getattr(r, a)) for a in dir(r)
                              if not a.startswith('_') and not callable(getattr(r, a))}
    for cfg_name, kw, (enc, dec), adapter in LAYOUTS:
        cfg = getattr(C, cfg_name)(**kw)
        cfg.label_smoothing = 0.1 if cfg.label_smoothing is None else cfg.label_smoothing
        cfg.model_type = cfg.model_type or 'encoder_decoder'
        cfg.decoder_max_len = cfg.decoder_max_len or 256
        model = (impl.AdapterTransformer if adapter else impl.Transformer)(cfg, C.DistributedConfig(), FakeTask(enc, dec))
        f['layouts'][cfg_name] = {'state_dict': [[k, list(v.shape)] for k, v in model.state_dict().items()],
                                  'frozen': _frozen(model)}
    f['plumbing'] = state_dict_plumbing(impl)
    f['adapter_plumbing'] = adapter_plumbing(impl)
    return f


def _digests_differ(a, b, exact=False):
    if a[0] != b[0] or len(a) != len(b):
        return True
    if len(a) == 1:  # (shape only)
        return False
    tol = 0.0 if exact else 1e-6 * (1.0 + a[2])
    return any(abs(x - y) > tol for x, y in zip(a[1:], b[1:]))


def compare(ref, mine):
    """-> problems: what `mine` (pasero_amd) does differently from `ref` (the reference)"""
    import pasero_amd.config as MC
    problems = []
    used, dused = set(), set()
    for fn in glob.glob(os.path.join(REPO, 'pasero_amd', '*.py')):
        src = open(fn).read()
        dused |= set(re.findall(r'\bdist_cfg\.(\w+)', src))
        if not fn.endswith('config.py'):
            used |= set(re.findall(r'\bcfg\.(\w+)', src))
    problems += [f'cfg.{a} is read but the reference configuration has no such field' for a in sorted(used)
                 if a not in ref['config_attrs']]
    problems += [f'dist_cfg.{a} is read but the reference has no such field' for a in sorted(dused)
                 if a not in ref['dist_attrs']]
    for name, mine_cls in MC.CONFIGS.items():
        r = ref['presets'].get(name)
        if r is None:
            problems.append(f'preset {name} does not exist in the reference')
            continue
        m = mine_cls()
        for fld in dataclasses.fields(m):
            if fld.name not in TASK_DEFAULTS and r.get(fld.name, '<missing>') != _plain(getattr(m, fld.name)):
                problems.append(f'preset {name}.{fld.name}: {getattr(m, fld.name)!r} here, '
                                f'{r.get(fld.name, "<missing>")!r} in the reference')
    for cfg_name, *_ in LAYOUTS:
        arch = MC.get_architecture(getattr(MC, cfg_name)())
        if not arch.__module__.startswith('pasero_amd'):
            problems.append(f'{cfg_name}: the registry resolves to {arch.__module__}.{arch.__name__}')
        if mine['layouts'][cfg_name]['state_dict'] != ref['layouts'][cfg_name]['state_dict']:
            problems.append(f'{cfg_name}: state_dict names/shapes differ from the reference model')
        if mine['layouts'][cfg_name]['frozen'] != ref['layouts'][cfg_name]['frozen']:
            problems.append(f'{cfg_name}: the set of frozen parameters differs')
    for what, exact in (('plumbing', False), ('adapter_plumbing', True)):
        for tag, r in ref[what].items():
            m = mine[what][tag]
            if set(r['updated']) != set(m['updated']):
                problems.append(f'{what} [{tag}]: keys differ: only reference {sorted(set(r["updated"]) - set(m["updated"]))[:5]}, '
                                f'only ours {sorted(set(m["updated"]) - set(r["updated"]))[:5]}')
                continue
            bad = [k for k in r['updated'] if _digests_differ(r['updated'][k], m['updated'][k], exact)]
            if bad:
                problems.append(f'{what} [{tag}]: values differ for {bad[:5]}')
            if r.get('strict_load', None) is None and m.get('strict_load', None) is not None:
                problems.append(f'{what} [{tag}]: strict load fails: {m["strict_load"]}')
                continue
            for key in ('clean_keys', 'extra_adapters', 'frozen'):
                if key in r and r[key] != m.get(key):
                    problems.append(f'{what} [{tag}]: {key} differ: {sorted(set(r[key]) ^ set(m.get(key) or []))[:6]}')
    return problems, len(used)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', metavar='DIR', help='a checkout of the reference (naver/pasero)')
    ap.add_argument('--fixture', metavar='FILE', help="the reference's facts as recorded by --write")
    ap.add_argument('--write', metavar='FILE', help="record the reference's facts (needs --reference)")
    args = ap.parse_args()
    if bool(args.reference) == bool(args.fixture) or (args.write and not args.reference):
        ap.error('give --reference DIR (optionally with --write FILE) or --fixture FILE')
    sys.path.insert(0, REPO)
    problems = []
    if args.reference:
        impl = import_reference(args.reference)
        ref = facts(impl)
        if args.write:
            with open(args.write, 'w') as f:
                json.dump(ref, f, indent=0, sort_keys=True)
                f.write('\n')
        import pasero_amd.transformer   # noqa: F401  registers 'transformer' in the reference's registry
        import pasero_amd.adapters      # noqa: F401  registers 'adapter_transformer' (after the reference's own import)
        for cfg_name, *_ in LAYOUTS:     # the reference's own registry, with pasero_amd imported, builds our classes
            arch = impl.C.get_architecture(getattr(impl.C, cfg_name)())
            if not arch.__module__.startswith('pasero_amd'):
                problems.append(f'{cfg_name}: the reference registry resolves to {arch.__module__}.{arch.__name__}')
    else:
        with open(args.fixture) as f:
            ref = json.load(f)
    more, nused = compare(ref, facts(ours()))
    problems += more
    for p in problems:
        print('AUDIT:', p)
    print(f'audit_against_reference: {len(problems)} problem(s), {nused} cfg fields, {len(ref["presets"])} reference '
          f'presets, {len(LAYOUTS)} model layouts')
    return 1 if problems else 0


if __name__ == '__main__':
    sys.exit(main())
