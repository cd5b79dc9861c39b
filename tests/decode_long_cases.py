"""Cases shared by tests/test_decode_long_cpu.py and tests/test_decode_long_gpu.py: two tiny encoder-decoders decoded
teacher-forced over 132 target tokens (past the 64th key, where 16-bit self-attention changes kernel and the native step's
caches grow for the first time, and past the 128th, where they grow again), with a 7-token and a 70-token source.

The reference is the CPU oracle (oracle/ref_cpu.py) on the whole prefix, one call, explicit softmax attention, on the
parameters of the model under test (its own `state_dict()`: for a 16-bit model the 16-bit-representable values) widened to
fp64 — the oracle's functions take fp64 unchanged (test_decode_long_cpu.py checks that against its pinned fp32 form).  The
encoder output the decoder reads is the oracle's, rounded once to the model's dtype, on both sides."""
import functools
import json
import types

import torch

import paramgen
from conftest import load_golden
from model_utils import build_model
from oracle import ref_cpu as O

B, T_LEN = 3, 132                      # sentences; target tokens (the first decoder call takes 2, then one step per token)
SOURCES = {'short': 7, 'long': 70}     # cross-attention on the short-sequence kernel / on the long one (S >= 64)
LONG_LENGTHS = [70, 64, 3]             # key padding of the long source
MODELS = ('post', 'pre')
FP32_STEP_TOL = 2e-5                   # the project's bound on step logits (tests/test_model_gpu.py), of the step's logit range
GAP_CAP = 0.02                         # at most this share of the positions may be left out of the argmax comparison


def fixture(model: str) -> dict:
    """what `build_model` reads of a golden fixture.  'post': tiny_encdec_post as it is (post-norm, sinusoidal positions, 2
    layers, V = 101: a padded logit pitch).  'pre': tiny_encdec_pre (pre-norm, learned positions, embedding and final
    LayerNorm, GELU, V = 67) with position tables of 256 rows — the fixture's 32 end before the 64th token."""
    g = load_golden('tiny_encdec_' + model)
    cfg = json.loads(str(g['cfg']))
    if model == 'pre':
        cfg['decoder_max_len'] = cfg['encoder_max_len'] = 256
    return {'cfg': json.dumps(cfg), 'V': int(g['V']), 'seed': int(g['seed'])}


def full_logits(P, cfg, enc_out, enc_mask, tokens, act_dtype=None):
    """(logits (B, T, V), last layer's V projection (B, T, H, hd)) of the oracle's full-prefix decoder; `act_dtype`: with every
    module output rounded to that type (the oracle's 16-bit model)"""
    state = {}
    O.ACT_DTYPE = act_dtype
    try:
        logits = O.decoder(P, cfg, enc_out, enc_mask, tokens, state=state)
    finally:
        O.ACT_DTYPE = None
    return logits, state[f'dec_{cfg.decoder_layers - 1}_self_attn_value']


def incremental_logits(P, cfg, enc_out, enc_mask, tokens):
    """the same, one token per oracle call on top of its incremental state"""
    state, out = {}, []
    for i in range(tokens.size(1)):
        out.append(O.decoder(P, cfg, enc_out, enc_mask, tokens[:, i:i + 1], state=state))
    return torch.cat(out, dim=1), state[f'dec_{cfg.decoder_layers - 1}_self_attn_value']


def checked_positions(logits):
    """(B, T) bool: where the argmax of step logits within FP32_STEP_TOL of `logits` must be the argmax of `logits` — the top
    two are further apart than twice that bound (a step's bound: FP32_STEP_TOL x the largest |logit| of the step, all rows)"""
    top = logits.topk(2, dim=-1).values
    bound = FP32_STEP_TOL * logits.abs().amax(dim=(0, 2))
    return (top[..., 0] - top[..., 1]) > 2 * bound[None, :]


@functools.lru_cache(maxsize=None)
def case(model: str, source: str, dtype=torch.float32, ref_dtype=torch.float64):
    """One (model, source, dtype) case, computed once per session and shared — treat every tensor as read-only.
    Fields: cfg, model (pasero_amd Transformer in `dtype`, on the CPU, eval), P (its parameters in `ref_dtype`), tokens (B, 132),
    enc_out (in `ref_dtype`, `dtype`-representable) / enc_mask, ref / ref_v (oracle logits (B, 132, V) and last-layer V
    projection (B, 132, H, 64)); for the 16-bit types also ref16 / ref16_v (the oracle's 16-bit model) and bracket / bracket_v
    = max |ref16 - ref|."""
    g = fixture(model)
    cfg, m = build_model(g, dtype, 'cpu')
    m.eval()
    P = {k: v.detach().to(ref_dtype) for k, v in m.state_dict().items()}
    S = SOURCES[source]
    b = paramgen.make_text_batch(g['seed'], B, S, T_LEN - 1, g['V'])
    src, src_len = torch.from_numpy(b['encoder_input']), torch.from_numpy(b['encoder_input_length'])
    if source == 'long':
        src_len = torch.tensor(LONG_LENGTHS)
        src = src.clamp(min=4)
        for i, n in enumerate(LONG_LENGTHS):
            src[i, n - 1] = cfg.eos_idx
            src[i, n:] = cfg.padding_idx
    tokens = torch.from_numpy(b['decoder_input']).clamp(min=2)  # no pad tokens inside the prefix
    assert tokens.shape == (B, T_LEN)
    enc_out, enc_mask = O.encoder(P, cfg, src, src_len)
    enc_out = enc_out.to(dtype).to(ref_dtype)
    c = types.SimpleNamespace(cfg=cfg, model=m, P=P, tokens=tokens, enc_out=enc_out, enc_mask=enc_mask, dtype=dtype)
    c.ref, c.ref_v = full_logits(P, cfg, enc_out, enc_mask, tokens)
    if dtype != torch.float32:
        c.ref16, c.ref16_v = full_logits(P, cfg, enc_out, enc_mask, tokens, act_dtype=dtype)
        c.bracket = (c.ref16 - c.ref).abs().max().item()
        c.bracket_v = (c.ref16_v - c.ref_v).abs().max().item()
    return c
