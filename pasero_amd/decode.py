"""Incremental decoding fast path: after the first decoder call of a sentence, every further call with
ONE new token per sentence (`decoder(encoder_out, encoder_mask, tokens[:, t:t+1], state=state)`, pasero/decoding.py:
1119-1221) runs as one native call, `pk_decoder_step` (include/pasero_hip.h), instead of ~90 Python-level op dispatches.

What changes relative to the reference's incremental mode (pasero/models/modules.py:621-641) — the results do not:
  * self-attention K/V live in preallocated (B, cap, D) buffers per layer, the new row is appended in place (the
    reference concatenates a new tensor every step); `state['dec_i_self_attn_key'/'_value']` stay what the reference
    documents — (B, t, H, hd) tensors — as views of those buffers;
  * `k_proj/v_proj(encoder_out)` are computed once per sentence (the reference recomputes them at every step).
The caches ride in the `state` dict under '_pk_decode' (`DecodeCache`); `Decoder.reorder_state` reorders them for beam
search.  Layers the native step does not cover (subclass hooks, gated feed-forward, rotary positions) keep using the
per-op path: `build_plan` returns None for them.  The layers of `adapter_transformer` (`AdapterTransformerDecoderLayer`,
the IWSLT2023 recipes) are covered: the plan carries each layer's stack of adapters in use and the step applies them
with pk_adapter_rows after the layer's feed-forward block (`pk_decoder_step_ex`).  The layers of `moe_transformer`
(`MOETransformerDecoderLayer`, the NLLB-200 MoE checkpoints) are covered when `moe_native()` is on (off by default): the
plan carries each mixture's gate and expert pointer tables and the step runs the feed-forward block as one pk_moerows
call (`pk_decoder_step_moe`).  A native step does not update `moe_layer.lb_loss` (only `compute_loss` reads it).

Beam search (`beam_search`, `BeamSelect`): see the section below.  Sampling search (`search`, `sampling`,
`sample_on_the_fly`, `SampleSelect`): the reference's other decoding arm (decoding.py:906-1221 — greedy, top-k, nucleus and
plain sampling, repeat penalty, blacklist, prompts, stop sequences) with one pk_sample_select call per step and the stop
test on the device; draws are inverse-CDF over (probability descending, token id ascending) from Philox(rng.next_offset()).
"""
import ctypes
import os
import weakref
from typing import Optional

import torch
from torch import Tensor

from . import functional as F
from . import lib
from .lib import ACT, check, dtype_code, ptr, require_gpu, stream_ptr

_P = ctypes.c_void_p
_LAYER_FIELDS = ['qkv_w', 'qkv_b', 'out_w', 'out_b', 'ln1_g', 'ln1_b', 'cq_w', 'cq_b', 'cout_w', 'cout_b', 'ln2_g',
                 'ln2_b', 'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'ln3_g', 'ln3_b']


class PkDecoderLayerWeights(ctypes.Structure):
    _fields_ = [(n, _P) for n in _LAYER_FIELDS]


class PkDecoderPlan(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int) for n in ('n_layers', 'd', 'heads', 'ffn', 'act', 'prenorm', 'dtype', 'scaled_attn')]
                + [('vocab', ctypes.c_longlong), ('eps', ctypes.c_float), ('embed_scale', ctypes.c_float)]
                + [(n, _P) for n in ('embed', 'pos', 'embed_ln_g', 'embed_ln_b', 'final_ln_g', 'final_ln_b', 'out_w')]
                + [('layers', ctypes.POINTER(PkDecoderLayerWeights))])


PK_ADAPTER_STACK_MAX = 4
_ADAPTER_FIELDS = ['ln_g', 'ln_b', 'down_w', 'down_b', 'up_w', 'up_b']


class PkAdapter(ctypes.Structure):
    _fields_ = ([(n, _P) for n in _ADAPTER_FIELDS] + [('p', ctypes.c_int), ('act', ctypes.c_int),
                                                     ('scaling', ctypes.c_float), ('eps', ctypes.c_float)])


class PkAdapterStack(ctypes.Structure):
    _fields_ = [('n', ctypes.c_int), ('a', PkAdapter * PK_ADAPTER_STACK_MAX)]


class PkMoeLayer(ctypes.Structure):
    _fields_ = [('E', ctypes.c_int), ('F', ctypes.c_int)] + [(n, _P) for n in ('gate_w', 'w1', 'b1', 'w2', 'b2')]


class Plan:
    """the PkDecoderPlan of one TransformerDecoder plus what keeps its pointers alive / detects that they went stale;
    `c_adapters`: the PkAdapterStack of every layer when some layer has adapters in use, else None; `c_moe`: the PkMoeLayer
    of every layer when some layer is a mixture of experts, else None"""

    def __init__(self, c_plan, c_layers, keep, fingerprint, cross_w, c_adapters=None, c_moe=None):
        self.c_plan, self.c_layers, self.keep, self.fingerprint, self.cross_w = c_plan, c_layers, keep, fingerprint, cross_w
        self.c_adapters, self.c_moe = c_adapters, c_moe
        self.full = None

    @property
    def adapters_ref(self):
        return None if self.c_adapters is None else ctypes.cast(self.c_adapters, _P)

    @property
    def moe_ref(self):
        return None if self.c_moe is None else ctypes.cast(self.c_moe, _P)


_moe_native = os.environ.get('PASERO_MOE_NATIVE_DECODE', '') not in ('', '0')


def moe_native(on: Optional[bool] = None) -> bool:
    """Native decoding for decoders with mixture-of-experts layers: sets the switch (None only asks) and returns the
    previous setting.  Initial value: the environment variable PASERO_MOE_NATIVE_DECODE at import (unset, empty or 0: off);
    PASERO_NO_NATIVE_DECODE still sends every call to the per-op path.  The switch is part of the plan key of decoders
    with mixture layers: toggling it rebuilds their plan."""
    global _moe_native
    prev = _moe_native
    if on is not None:
        _moe_native = bool(on)
    return prev


def _has_moe(decoder) -> bool:
    return any(hasattr(layer, 'moe_layer') for layer in decoder.layers)


def _moe_spec(layer, D: int):
    """(gate weight, E fc1 weights, E fc2 weights, E fc1 biases | None, E fc2 biases | None, F) of a mixture layer the native
    step can run as pk_moerows — None when it cannot (another mixture class, lora on an expert, non-contiguous tensors)"""
    from .moe import MixtureOfExperts
    mix = getattr(layer, 'moe_layer', None)
    if type(mix) is not MixtureOfExperts or mix.act_name != layer.activation_fn.name or mix.embed_dim != D:
        return None
    E, Fd = mix.expert_count, mix.expert_dim
    if not 2 <= E <= 256 or len(mix.experts) != E:
        return None
    ex = list(mix.experts)
    if any(getattr(m, 'lora', None) is not None for e in ex for m in (e.fc1, e.fc2)):
        return None
    w1, w2 = tuple(e.fc1.weight for e in ex), tuple(e.fc2.weight for e in ex)
    b1 = tuple(e.fc1.bias for e in ex) if mix.has_bias else None
    b2 = tuple(e.fc2.bias for e in ex) if mix.has_bias else None
    gate = mix.gate.weight
    tensors = [gate, *w1, *w2, *(b1 or ()), *(b2 or ())]
    if (any(t is None or not t.is_contiguous() for t in tensors) or tuple(gate.shape) != (E, D)
            or any(tuple(w.shape) != (Fd, D) for w in w1) or any(tuple(w.shape) != (D, Fd) for w in w2)):
        return None
    return gate, w1, w2, b1, b2, Fd


def _adapter_key(decoder):
    """what `AdapterTransformerDecoder.forward` may change between two calls (it rewrites `adapters_in_use` from `meta`,
    adapters.py:112-117) and `enable()` / `disable()`: per adapter layer, the names in use and their disabled flags.
    None for a decoder without adapter layers: its keys stay what they were."""
    key = None
    for layer in decoder.layers:
        names, ads = getattr(layer, 'adapters_in_use', None), getattr(layer, 'adapters', None)
        if names is not None and ads is not None:  # (the decoder writes `adapters_in_use` on its plain layers too)
            flags = tuple(bool(ads[u].disabled or ads[u].permanently_disabled) if u in ads else None for u in names)
            key = (key or ()) + ((tuple(names), flags),)
    return key


def _adapter_stack(layer, D: int):
    """[(tensors in _ADAPTER_FIELDS order, p, act, scaling, eps)] of the adapters `layer` applies, in order — None when the
    native step cannot run them (more than PK_ADAPTER_STACK_MAX, no residual, another output width, an unknown name)"""
    out = []
    for uid in layer.adapters_in_use:
        if uid not in layer.adapters:
            return None  # (the per-op path raises the KeyError)
        ad = layer.adapters[uid]
        if ad.disabled or ad.permanently_disabled:
            continue
        if not ad.residual or ad.output_dim != ad.input_dim or ad.input_dim != D or ad.act_name not in ACT:
            return None
        norm = ad.layer_norm if ad.has_layer_norm else None
        if norm is not None and (type(norm) is not torch.nn.LayerNorm or tuple(norm.normalized_shape) != (D,)
                                 or norm.weight is None):
            return None
        p = ad.down.weight.size(0)
        if tuple(ad.down.weight.shape) != (p, D) or tuple(ad.up.weight.shape) != (D, p):
            return None
        tensors = [getattr(norm, 'weight', None), getattr(norm, 'bias', None), ad.down.weight, ad.down.bias, ad.up.weight,
                   ad.up.bias]
        if any(t is not None and not t.is_contiguous() for t in tensors):
            return None
        out.append((tensors, p, ACT[ad.act_name], float(ad.scaling), float(getattr(norm, 'eps', 1e-5))))
    return out if len(out) <= PK_ADAPTER_STACK_MAX else None


def _fingerprint(decoder):
    w = decoder.embed_tokens.weight
    first = decoder.layers[0]
    fc1 = getattr(first, 'fc1', None)  # (a mixture-of-experts layer has no fc1: its gate serves as the anchor — not the
    # attention projections, which `build_plan` moves into one packed buffer)
    mix = getattr(first, 'moe_layer', None)
    anchor = fc1.weight if fc1 is not None else mix.gate.weight if mix is not None else next(first.parameters())
    return (w.data_ptr(), w.dtype, str(w.device), anchor.data_ptr())


def _full_fingerprint(decoder):
    """every parameter's address and type: the plan holds raw pointers, so a parameter whose storage was replaced
    (`p.data = ...`, a partial `.to()`) must invalidate it.  ~30 us: checked once per sentence batch, the cheap
    fingerprint above at every step."""
    return tuple((p.data_ptr(), p.dtype) for p in decoder.parameters())


def build_plan(decoder) -> Optional[Plan]:
    """PkDecoderPlan for `decoder` (a pasero_amd TransformerDecoder), or None when a layer is not the stock one"""
    from . import modules
    from .adapters import AdapterTransformerDecoderLayer
    from .moe import MOETransformerDecoderLayer
    from .transformer import TransformerDecoderLayer
    cfg = decoder.cfg
    if (decoder.training or not decoder.embed_tokens.weight.is_cuda
            or cfg.embed_dim != 64 * cfg.decoder_attention_heads):  # the native step is built for head_dim 64
        return None
    if getattr(decoder.embed_tokens, 'frozen_embedding', None) is not None:
        # a partially frozen table (modules.py:929-946: lookup and tied projection blend `weight` with
        # `frozen_embedding.weight`; with shared embeddings the decoder carries the encoder's): the plan holds ONE raw
        # table pointer, so these decoders stay on the per-op path, which reads `effective_weight()`
        return None
    pos = decoder.embed_positions
    if not isinstance(pos, (modules.SinusoidalPositionalEmbedding, modules.LearnedPositionalEmbedding)):
        return None  # rotary: positions are applied inside attention — per-op path
    hooks = ('ffn', 'self_attention', 'cross_attention', 'self_attn_residual', 'self_attn_prenorm',
             'self_attn_postnorm', 'cross_attn_residual', 'cross_attn_prenorm', 'cross_attn_postnorm', 'ffn_residual',
             'ffn_prenorm', 'ffn_postnorm', 'forward')

    def ln(m):
        return m if type(m) in (modules.LayerNorm, modules.WrappableLayerNorm, modules.LayerNormWithoutBias) else None

    keep, layers, stacks, mixtures = [], [], [], []
    for layer in decoder.layers:
        if not isinstance(layer, TransformerDecoderLayer):
            return None
        spec = None
        if _moe_native and type(layer) is MOETransformerDecoderLayer:  # exactly, and only with the switch on
            if not layer._hooks_are_base(*[h for h in hooks if h != 'ffn']):
                return None
            spec = _moe_spec(layer, cfg.embed_dim)
            if spec is None:
                return None
            stacks.append([])
        elif type(layer) is AdapterTransformerDecoderLayer:  # exactly: a subclass may do anything around its adapters
            if not layer._hooks_are_base(*hooks[:-1]):
                return None
            stack = _adapter_stack(layer, cfg.embed_dim)
            if stack is None:
                return None
            stacks.append(stack)
        elif not layer._hooks_are_base(*hooks):
            return None
        else:
            stacks.append([])
        mixtures.append(spec)
        if (getattr(layer, '_no_ckpt_forward', None) is not None or layer.fc3 is not None
                or (spec is None and layer.fc1.lora is not None) or layer.self_attn.q_proj.lora is not None):
            return None
        norms = [ln(layer.self_attn_layer_norm), ln(layer.encoder_attn_layer_norm), ln(layer._norm_module(layer.final_layer_norm))]
        sa, ca = layer.self_attn, layer.encoder_attn
        if (None in norms or sa.rotary_embed is not None or ca.rotary_embed is not None or layer.prenorm != cfg.decoder_prenorm
                or layer.activation_fn.name not in ('relu', 'gelu', 'gelu_tanh', 'silu')):
            return None
        w_sa, b_sa = sa._flat()
        w_ca, b_ca = ca._flat()
        D = cfg.embed_dim
        keep += [w_sa, b_sa, w_ca, b_ca]
        vals = [w_sa, b_sa, sa.out_proj.weight, sa.out_proj.bias, norms[0].weight, norms[0].bias,
                w_ca[:D], None if b_ca is None else b_ca[:D], ca.out_proj.weight, ca.out_proj.bias, norms[1].weight,
                norms[1].bias, *((None,) * 4 if spec is not None else (layer.fc1.weight, layer.fc1.bias, layer.fc2.weight,
                                                                      layer.fc2.bias)), norms[2].weight, norms[2].bias]
        layers.append((vals, (w_ca[D:], None if b_ca is None else b_ca[D:])))
    embed_ln = decoder.layernorm_embedding
    final_ln = decoder.layer_norm
    for m in (embed_ln, final_ln):
        if not isinstance(m, modules.Identity) and ln(m) is None:
            return None
    c_layers = (PkDecoderLayerWeights * len(layers))()
    for cl, (vals, _) in zip(c_layers, layers):
        for name, v in zip(_LAYER_FIELDS, vals):
            setattr(cl, name, ptr(v))
    E = decoder.embed_tokens.weight
    out_w = E if decoder.output_projection is None else decoder.output_projection.weight
    table = pos.table()
    keep += [table]
    p = PkDecoderPlan()
    p.n_layers, p.d, p.heads, p.ffn = len(layers), cfg.embed_dim, cfg.decoder_attention_heads, cfg.decoder_ffn_dim
    p.act = ACT[decoder.layers[0].activation_fn.name]
    p.prenorm, p.dtype, p.scaled_attn = int(bool(cfg.decoder_prenorm)), dtype_code(E), int(bool(cfg.scale_attn))
    p.vocab, p.eps, p.embed_scale = E.size(0), float(cfg.norm_eps), float(decoder.embed_scale)
    p.embed, p.pos = ptr(E), ptr(table)
    p.embed_ln_g = None if isinstance(embed_ln, modules.Identity) else ptr(embed_ln.weight)
    p.embed_ln_b = None if isinstance(embed_ln, modules.Identity) else ptr(embed_ln.bias)
    p.final_ln_g = None if isinstance(final_ln, modules.Identity) else ptr(final_ln.weight)
    p.final_ln_b = None if isinstance(final_ln, modules.Identity) else ptr(final_ln.bias)
    p.out_w = ptr(out_w)
    p.layers = ctypes.cast(c_layers, ctypes.POINTER(PkDecoderLayerWeights))
    keep += [t for vals, _ in layers for t in vals if t is not None] + [E, out_w]  # the pointers stay valid
    keep += [t for m in (embed_ln, final_ln) if not isinstance(m, modules.Identity) for t in (m.weight, m.bias)]
    c_adapters = None
    if any(stacks):
        c_adapters = (PkAdapterStack * len(stacks))()
        for cs, stack in zip(c_adapters, stacks):
            cs.n = len(stack)
            for ca, (tensors, rank, act, scaling, eps) in zip(cs.a, stack):
                for name, v in zip(_ADAPTER_FIELDS, tensors):
                    setattr(ca, name, ptr(v))
                ca.p, ca.act, ca.scaling, ca.eps = rank, act, scaling, eps
                keep += [t for t in tensors if t is not None]  # (and under the mixed-dtype rule below)
    c_moe = None
    if any(m is not None for m in mixtures):
        c_moe = (PkMoeLayer * len(mixtures))()
        for cm, layer, spec in zip(c_moe, decoder.layers, mixtures):
            if spec is None:
                continue  # (E == 0: a dense layer)
            gate, w1, w2, b1, b2, Fd = spec
            tables = layer.moe_layer._tables.get((w1, w2, b1, b2))  # the module's own device arrays of expert addresses
            cm.E, cm.F, cm.gate_w = len(w1), Fd, ptr(gate)
            cm.w1, cm.w2, cm.b1, cm.b2 = (ptr(t) for t in tables)
            keep += [gate, *w1, *w2, *(b1 or ()), *(b2 or ())] + [t for t in tables if t is not None]
    dtypes = {t.dtype for t in keep if t is not None and t.is_floating_point()}
    if len(dtypes) != 1:
        return None  # mixed parameter dtypes (e.g. fp32 LayerNorm weights in a bf16 model): per-op path, which refuses loudly
    plan = Plan(p, c_layers, keep, _fingerprint(decoder), [cw for _, cw in layers], c_adapters, c_moe)
    plan.full = _full_fingerprint(decoder)
    return plan


_plans = weakref.WeakKeyDictionary()  # decoder -> (fingerprint, training), Plan | None


def get_plan(decoder) -> Optional[Plan]:
    """the decoder's plan, rebuilt when its parameters moved (`.to()`), changed dtype or it switched train/eval"""
    key = (_fingerprint(decoder), decoder.training)
    ad_key = _adapter_key(decoder)
    if ad_key is not None:  # (decoders without adapter layers keep the two-element key)
        key += (ad_key,)
    if _has_moe(decoder):  # (and decoders without mixture layers theirs)
        key += (('moe_native', _moe_native),)
    cached = _plans.get(decoder)
    if cached is None or cached[0] != key:
        cached = (key, build_plan(decoder))
        _plans[decoder] = cached
    return cached[1]


class DecodeCache:
    """per-sentence-batch decoding state of the native step: self-attention caches, cross-attention K/V, scratch"""

    KEY = '_pk_decode'
    OFF = '_pk_decode_off'  # set once a sentence batch left the native path for good (cache truncation)

    def __init__(self, decoder, plan: Plan, encoder_out: Tensor, encoder_mask: Optional[Tensor], state: dict):
        cfg = decoder.cfg
        self.plan = plan
        self.names = [(f'{layer.self_attn_key}_key', f'{layer.self_attn_key}_value') for layer in decoder.layers]
        first = state[self.names[0][0]]
        B, t = first.size(0), first.size(1)
        self.B, self.t, self.D, self.H = B, t, cfg.embed_dim, cfg.decoder_attention_heads
        self.S = encoder_out.size(1)
        dev, dt = encoder_out.device, encoder_out.dtype
        self.cap = max(64, 1 << (2 * t).bit_length())
        self.k = [torch.empty(B, self.cap, self.D, device=dev, dtype=dt) for _ in self.names]
        self.v = [torch.empty(B, self.cap, self.D, device=dev, dtype=dt) for _ in self.names]
        for (kn, vn), ck, cv in zip(self.names, self.k, self.v):
            ck[:, :t].copy_(state[kn].reshape(B, t, self.D))
            cv[:, :t].copy_(state[vn].reshape(B, t, self.D))
        enc2d = encoder_out.reshape(B * self.S, self.D)
        self.cross = [F.gemm(enc2d, w, bias=b) for w, b in plan.cross_w]  # [k | v] projections, once per sentence
        self.mask = None if encoder_mask is None else encoder_mask.contiguous()
        self.V = decoder.embed_tokens.weight.size(0)
        self.ldl = (self.V + 7) // 8 * 8
        self.scratch = torch.empty(self._scratch_bytes(B), dtype=torch.uint8, device=dev)
        self._tables()
        self._publish(state)

    def _scratch_bytes(self, B: int) -> int:
        L, plan = lib.load(), self.plan
        if plan.c_moe is not None:
            return L.pk_decoder_step_scratch_moe(ctypes.byref(plan.c_plan), B, plan.adapters_ref, plan.moe_ref)
        if plan.c_adapters is None:
            return L.pk_decoder_step_scratch(ctypes.byref(plan.c_plan), B)
        return L.pk_decoder_step_scratch_ex(ctypes.byref(plan.c_plan), B, plan.adapters_ref)

    def _tables(self):
        n = len(self.names)
        self.k_tab = (_P * n)(*[t.data_ptr() for t in self.k])
        self.v_tab = (_P * n)(*[t.data_ptr() for t in self.v])
        self.c_tab = (_P * n)(*[t.data_ptr() for t in self.cross])

    def _publish(self, state: dict):
        """the reference's view of the caches: (B, t, H, hd) tensors per layer"""
        B, t, H = self.B, self.t, self.H
        for (kn, vn), ck, cv in zip(self.names, self.k, self.v):
            state[kn] = ck[:B, :t].view(B, t, H, 64)  # (a buffer of `reorder_beam` may hold more rows than B)
            state[vn] = cv[:B, :t].view(B, t, H, 64)

    def matches(self, state: dict, encoder_out: Tensor) -> bool:
        """still the caches of THIS state (nobody replaced the tensors behind our back)"""
        first = state.get(self.names[0][0])
        return (first is not None and first.data_ptr() == self.k[0].data_ptr() and first.size(1) == self.t
                and first.size(0) == self.B and encoder_out.size(0) == self.B and encoder_out.size(1) == self.S)

    def _grow(self):
        self.cap *= 2
        for lst in (self.k, self.v):
            for i, old in enumerate(lst):
                new = torch.empty(self.B, self.cap, self.D, device=old.device, dtype=old.dtype)
                new[:, :self.t].copy_(old[:self.B, :self.t])
                lst[i] = new
        self._spare = None
        self._tables()

    def step(self, ids: Tensor, pos_start: int, state: dict) -> Tensor:
        if self.t + 1 > self.cap:
            self._grow()
        ids = ids.reshape(-1).contiguous()
        logits = torch.empty(self.B, self.ldl, device=self.scratch.device, dtype=self.k[0].dtype)  # the caller keeps it
        L = lib.load()
        args = (ctypes.byref(self.plan.c_plan), ptr(ids), self.B, self.t, int(pos_start), self.k_tab, self.v_tab, self.cap,
                self.c_tab, ptr(self.mask), self.S, ptr(self.scratch), self.scratch.numel(), ptr(logits), self.ldl)
        if self.plan.c_moe is not None:
            check(L.pk_decoder_step_moe(*args, self.plan.adapters_ref, self.plan.moe_ref, stream_ptr()), 'pk_decoder_step_moe')
        elif self.plan.c_adapters is None:
            check(L.pk_decoder_step(*args, stream_ptr()), 'pk_decoder_step')
        else:
            check(L.pk_decoder_step_ex(*args, self.plan.adapters_ref, stream_ptr()), 'pk_decoder_step_ex')
        self.t += 1
        self._publish(state)
        return logits[:, :self.V].unsqueeze(1)

    def _gather_cross(self, idx: Tensor):
        """select sentences of the cross-attention K|V and of the encoder mask"""
        self.cross = [c.view(-1, self.S, 2 * self.D).index_select(0, idx).view(-1, 2 * self.D) for c in self.cross]
        self.mask = None if self.mask is None else self.mask.index_select(0, idx)

    def reorder(self, indices: Tensor, state: dict):
        """beam search (transformer.py:68-75): select sentences / hypotheses along the batch dimension"""
        idx = indices.to(self.k[0].device)
        self.k = [c[:self.B].index_select(0, idx) for c in self.k]
        self.v = [c[:self.B].index_select(0, idx) for c in self.v]
        self.B = idx.numel()
        self._spare = None
        self._gather_cross(idx)
        nbytes = self._scratch_bytes(self.B)
        if nbytes > self.scratch.numel():
            self.scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.scratch.device)
        self._tables()
        self._publish(state)

    _spare = None  # the second buffer set of `reorder_beam`: (k list, v list), allocated at the first beam re-ordering

    def reorder_beam(self, indices: Tensor, state: dict, shrink: bool):
        """`reorder` for `beam_search`: the same published state, less traffic.  The self-attention caches are gathered
        by ONE pk_beam_reorder launch (rows < t only) into a second buffer set and the two sets swap (an in-place
        gather races); the cross-attention K|V and the mask are left alone unless sentences leave the batch
        (`shrink`) — the rows of one sentence's beams are equal, so selecting among them changes nothing."""
        idx = indices.to(self.k[0].device).contiguous()
        rows_in, rows_out, n = self.B, idx.numel(), len(self.names)
        if self._spare is None:
            self._spare = ([torch.empty_like(c) for c in self.k], [torch.empty_like(c) for c in self.v])
        k2, v2 = self._spare
        assert rows_out <= k2[0].size(0)
        dk = (_P * n)(*[t.data_ptr() for t in k2])
        dv = (_P * n)(*[t.data_ptr() for t in v2])
        check(lib.load().pk_beam_reorder(self.k_tab, self.v_tab, dk, dv, n, ptr(idx), rows_out, rows_in, self.t, self.cap,
                                         self.D, dtype_code(self.k[0]), stream_ptr()), 'pk_beam_reorder')
        self._spare, self.k, self.v = (self.k, self.v), k2, v2
        self.B = rows_out
        if shrink:
            self._gather_cross(idx)
        self._tables()
        self._publish(state)

    def clone(self, state: dict) -> dict:
        """an independent copy of this cache and of the `state` dict it rides in (tests compare two re-orderings)"""
        import copy
        other = copy.copy(self)
        other.k, other.v = [c.clone() for c in self.k], [c.clone() for c in self.v]
        other.cross = [c.clone() for c in self.cross]
        other.mask = None if self.mask is None else self.mask.clone()
        other.scratch = torch.empty_like(self.scratch)
        other._spare = None
        other._tables()
        new_state = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in state.items()}
        new_state[DecodeCache.KEY] = other
        other._publish(new_state)
        return new_state


def try_step(decoder, encoder_out: Tensor, encoder_mask: Optional[Tensor], decoder_input: Tensor, state: Optional[dict],
             return_layers, project: bool) -> Optional[Tensor]:
    """logits (B, 1, V) of one native decoding step, or None when the call is not one (first call of a sentence,
    several new tokens, training, return_layers, non-stock layers)"""
    if (state is None or decoder.training or torch.is_grad_enabled() or return_layers or not project
            or decoder_input.dim() != 2 or decoder_input.size(1) != 1 or not state.get('offset')
            or state.get(DecodeCache.OFF) or os.environ.get('PASERO_NO_NATIVE_DECODE')):
        return None
    plan = get_plan(decoder)
    if plan is None:
        return None
    cache = state.get(DecodeCache.KEY)
    if cache is not None and cache.plan is not plan:
        return None  # a state dict shared by several decoders (decoding.py EnsembleDecoder): per-op path for the others
    if cache is not None and not cache.matches(state, encoder_out):
        cache = None
    first = decoder.layers[0].self_attn_key + '_key'
    if cache is None:
        if first not in state or encoder_out is None or state[first].size(1) != state['offset']:
            return None
        if plan.full != _full_fingerprint(decoder):  # some parameter moved since the plan was built
            _plans.pop(decoder, None)
            plan = get_plan(decoder)
            if plan is None:
                return None
        cache = DecodeCache(decoder, plan, encoder_out, encoder_mask, state)
        state[DecodeCache.KEY] = cache
    max_len = decoder.layers[0].self_attn.max_len
    if max_len is not None and cache.t + 1 > max_len:
        # the reference starts dropping the oldest keys here (modules.py:629-634): per-op path from now on
        state.pop(DecodeCache.KEY, None)
        state[DecodeCache.OFF] = True
        return None
    pos = decoder.embed_positions
    offset = state['offset']
    pos.check_length(1, offset)
    logits = cache.step(decoder_input, pos.shift + offset, state)
    state['offset'] = offset + 1
    return logits


def _select_operands(logits: Tensor, V: int, contiguous=(), strided=()):
    """what BeamSelect.run and SampleSelect.run ask of their operands.  Returns the logits with unit column stride (a
    contiguous copy if they had another) and their row pitch (one row: at least V); asserts of every (tensor | None,
    dtype) pair that it has the dtype and lies on the device, and of the `contiguous` ones that they are contiguous"""
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    ld = logits.stride(0) if logits.size(0) > 1 else max(V, logits.stride(0))
    for t, dt in contiguous:
        assert t is None or (t.dtype == dt and t.is_contiguous() and t.is_cuda)
    for t, dt in strided:
        assert t is None or (t.dtype == dt and t.is_cuda)
    return logits, ld


def _prompt_logprobs(logits: Tensor, next_tokens: Tensor) -> Tensor:
    """log-probabilities of a prompt's tokens under the first decoder call (decoding.py:1395-1402): logits (B, n + 1, V),
    next_tokens (B, n) -> (B, n), plain torch"""
    return logits[:, :-1].float().log_softmax(dim=-1).gather(2, next_tokens.unsqueeze(2)).squeeze(2)


# ---- beam search (pasero/decoding.py:1225-1657) ----------------------------------------------------------------------
class BeamSelect:
    """buffers of pk_beam_select for searches of up to B sentences x K beams over V tokens, and the call itself.
    After `run`: `sel_beam` / `sel_tok` (int64) and `sel_score` (fp32) hold rows [0, B*K) of the continued beams;
    `records()` brings n_eos and the 2K candidates of every sentence to the host in ONE copy."""

    def __init__(self, B: int, K: int, V: int, device):
        L = lib.load()
        self.B, self.K, self.V, self.R = B, K, V, 2 * K
        # K outside [1, 16] is refused by the library (pk_beam_select); size the buffers for any K so that it gets to say so
        self.scratch = torch.empty(max(256, L.pk_beam_select_scratch(B, K, V)), dtype=torch.uint8, device=device)
        n = B * self.R
        self.rec = torch.zeros(B + 4 * n, dtype=torch.int32, device=device)  # n_eos | score bits | beam | token | eos flag
        self.n_eos = self.rec[:B]
        self.cand_score = self.rec[B:B + n].view(torch.float32)
        self.cand_beam, self.cand_tok, self.cand_eos = (self.rec[B + i * n:B + (i + 1) * n] for i in (1, 2, 3))
        self.sel_beam = torch.zeros(B * K, dtype=torch.int64, device=device)
        self.sel_tok = torch.zeros(B * K, dtype=torch.int64, device=device)
        self._scores = [torch.zeros(B * K, dtype=torch.float32, device=device) for _ in range(2)]  # hyp_in of the next step
        self.sel_score = self._scores[0]
        self.lse = torch.zeros(B * K, dtype=torch.float32, device=device)

    def run(self, logits: Tensor, B: int, eos: int, pad: int, hyp: Optional[Tensor] = None, row_bias: Optional[Tensor] = None,
            forced: Optional[Tensor] = None, blacklist: Optional[Tensor] = None, eos_counts: Optional[Tensor] = None):
        """logits (B*K, V), any row stride, fp32 / bf16 / fp16"""
        require_gpu(logits)
        assert logits.dim() == 2 and logits.size(0) == B * self.K and logits.size(1) == self.V and B <= self.B
        logits, ld = _select_operands(logits, self.V, contiguous=(
            (hyp, torch.float32), (row_bias, torch.float32), (forced, torch.int64), (blacklist, torch.int64),
            (eos_counts, torch.uint8)))
        out = self._scores[1] if (hyp is not None and hyp.data_ptr() == self._scores[0].data_ptr()) else self._scores[0]
        check(lib.load().pk_beam_select(
            ptr(logits), ld, self.V, B, self.K, dtype_code(logits), ptr(hyp), ptr(row_bias), ptr(forced), int(pad), int(eos),
            ptr(blacklist), 0 if blacklist is None else blacklist.numel(), ptr(eos_counts), ptr(self.scratch),
            self.scratch.numel(), ptr(self.cand_score), ptr(self.cand_beam), ptr(self.cand_tok), ptr(self.cand_eos),
            ptr(self.n_eos), ptr(self.sel_beam), ptr(self.sel_tok), ptr(out), ptr(self.lse), stream_ptr()), 'pk_beam_select')
        self.sel_score = out

    def records(self, B: int):
        """host copies (numpy): n_eos (B,), score / beam / token / eos flag (B, 2K) — the step's one device->host read"""
        host = self.rec.cpu().numpy()
        n, R = self.B * self.R, self.R
        part = [host[self.B + i * n:self.B + i * n + B * R].reshape(B, R) for i in range(4)]
        return host[:B], part[0].view('float32'), part[1], part[2], part[3]


_warned_repeat_penalty = False


def _uncollate(hyp: dict, padding_idx: int, src_mask: Optional[Tensor]):
    """decoding.py:1660-1705 for the keys a search produces: cut what belongs to padding tokens"""
    tokens = hyp['tokens']
    pad_at = tokens == padding_idx
    hyp['tokens'] = tokens[:int((~pad_at).sum())]
    for k, v in list(hyp.items()):
        if v is None:
            continue
        if k.startswith('enc_'):
            v = v[~src_mask]
            if k.endswith('_self_attn'):
                v = v[..., ~src_mask]
            hyp[k] = v
        elif k == 'pos_scores':
            hyp[k] = v[~pad_at]


def _single(decoder, encoder_outputs, encoder_masks, return_layers, sharded, who):
    """the one decoder / encoder output / mask of a search, or NotImplementedError naming the option"""
    if isinstance(encoder_outputs, (list, tuple)):
        if len(encoder_outputs) > 1:
            raise NotImplementedError(f'pasero_amd {who}: ensembles (several decoders) are not implemented')
        encoder_outputs = encoder_outputs[0] if encoder_outputs else None
    if isinstance(encoder_masks, (list, tuple)):
        encoder_masks = encoder_masks[0] if encoder_masks else None
    if len(getattr(decoder, 'decoders', ())) > 1:
        raise NotImplementedError(f'pasero_amd {who}: ensembles (several decoders) are not implemented')
    if return_layers:
        raise NotImplementedError(f'pasero_amd {who}: return_layers is not implemented')
    if sharded:
        raise NotImplementedError(f'pasero_amd {who}: sharded=True is not implemented')
    if encoder_outputs is None:
        raise NotImplementedError(f'pasero_amd {who}: decoder-only models (empty encoder_outputs) are not implemented')
    if getattr(decoder, 'decoders', None):  # a one-element ensemble wrapper
        decoder = decoder.decoders[0]
    return decoder, encoder_outputs, encoder_masks


def _search_setup(decoder, encoder_outputs, encoder_masks, return_layers, sharded, who, device, decoder_input,
                  max_output_len, blacklist):
    """what both searches start with: the one decoder (in eval mode), the encoder output and mask on the device, B, pad,
    eos, the prompt (`decoder_input`, BOS by default), its lengths `plen` (B,) with their minimum `lo` and maximum `hi`
    (the set-up's one host read), the length limit `max_len` and the blacklist as a tensor (None when empty)"""
    decoder, enc, enc_mask = _single(decoder, encoder_outputs, encoder_masks, return_layers, sharded, who)
    decoder.eval()
    dev = torch.device(device) if device is not None else enc.device
    enc, enc_mask = enc.to(dev), None if enc_mask is None else enc_mask.to(dev)
    require_gpu(enc)
    B = enc.size(0)
    if decoder_input is None:
        decoder_input = torch.full((B, 1), decoder.bos_idx, dtype=torch.long, device=dev)
    decoder_input = decoder_input.to(dev)
    assert decoder_input.dim() == 2 and decoder_input.size(0) == B
    not_pad = decoder_input != decoder.padding_idx
    plen = (not_pad * torch.arange(1, decoder_input.size(1) + 1, device=dev)).amax(dim=1)  # utils.mask_to_len
    lo, hi = (int(x) for x in torch.stack([plen.min(), plen.max()]).tolist())  # (before the loop: not a step's read)
    assert lo > 0
    max_len = min(decoder.max_len, hi + max_output_len)
    assert max_len >= 1
    black = torch.tensor(list(blacklist), dtype=torch.int64, device=dev) if len(blacklist) else None
    return decoder, enc, enc_mask, B, decoder.padding_idx, decoder.eos_idx, decoder_input, plen, lo, hi, max_len, black


def beam_search(decoder, encoder_outputs, encoder_masks, max_output_len: int, beam_size: int, meta: dict, *,
                return_scores: bool = False, decoder_input: Optional[Tensor] = None, return_layers=[],
                sharded: bool = False, enc_layer_outputs: dict = {}, device=None, len_penalty: float = 1.0,
                blacklist=[], **kwargs):
    """Drop-in for pasero.decoding.beam_search (decoding.py:1225-1657): same keyword signature, same return value — a list
    of B n-best lists of dicts ('tokens', 'score', 'normalized_score', 'pos_scores' under `return_scores`), sorted by
    normalized score.  The decoder call is the reference's (`decoder(encoder_out, encoder_mask, tokens, state=state)`: the
    native decoding step when a plan exists, the per-op path otherwise); what surrounds it runs on the device:
      * one pk_beam_select call per step does log-softmax, blacklist, forced prompt tokens, + hypothesis scores, top 2K,
        EOS mask and the choice of the K continued beams, reading the logits once in their own dtype;
      * the native step's self-attention caches are re-ordered by one pk_beam_reorder launch (`DecodeCache.reorder_beam`);
        the cross-attention K|V, the encoder output and its mask are only touched when a sentence leaves the batch;
      * one device->host read per step (n_eos and the candidates); the finished-hypothesis bookkeeping is host Python.
    Among equal scores the candidate with the lower flat index k*V + v comes first (torch.topk leaves it open).
    Not implemented (raise, naming the option): ensembles, `return_layers`, `sharded`, decoder-only models."""
    global _warned_repeat_penalty
    import warnings
    from .transformer import Decoder
    if kwargs.get('repeat_penalty', 1.0) != 1.0 and not _warned_repeat_penalty:
        _warned_repeat_penalty = True
        warnings.warn("'repeat_penalty' is not supported in beam search")
    decoder, enc, enc_mask, B0, pad, eos, decoder_input, plen, lo, hi, max_len, black = _search_setup(
        decoder, encoder_outputs, encoder_masks, return_layers, sharded, 'beam_search', device, decoder_input,
        max_output_len, blacklist)
    K, dev = int(beam_size), enc.device
    tokens = torch.full((B0 * K, max_len), eos, dtype=torch.long, device=dev)  # EOS as filler: a hypothesis ends with it
    width = min(decoder_input.size(1), max_len)
    tokens[:, :width] = decoder_input.repeat_interleave(K, dim=0)[:, :width]
    feed = tokens[:, :lo]
    src_mask = enc_mask
    enc = enc.repeat_interleave(K, dim=0)
    enc_mask = None if enc_mask is None else enc_mask.repeat_interleave(K, dim=0)
    cum = torch.zeros(B0 * K, max_len, dtype=torch.float32, device=dev) if return_scores else None
    select = None
    finished = [[] for _ in range(B0)]
    alive = list(range(B0))      # current batch index -> initial batch index
    plen_alive = plen
    hyp, state, nB = None, {}, B0
    with torch.no_grad():
        for step in range(lo, max_len):
            logits, _ = decoder(enc, enc_mask, feed, state=state, meta=meta)
            if select is None:
                select = BeamSelect(B0, K, logits.size(-1), dev)
            bias = prompt_scores = None
            if logits.size(1) > 1:  # the first call carries the prompt: score its tokens (decoding.py:1395-1402)
                assert step == lo
                nxt = feed[:, 1:]
                prompt_scores = _prompt_logprobs(logits, nxt) * (nxt != pad)
                bias = prompt_scores.sum(dim=1).contiguous()
            forced = tokens[:, step].contiguous() if step < hi else None
            counts = (plen_alive <= step).to(torch.uint8) if step < hi else None  # an EOS inside a prompt is no end
            select.run(logits[:, -1], nB, eos, pad, hyp=hyp, row_bias=bias, forced=forced, blacklist=black, eos_counts=counts)
            n_eos, c_score, c_beam, c_tok, c_eos = select.records(nB)
            keep = None
            if n_eos.any():
                ends = [(b, j) for b in range(nB) for j in range(K) if c_eos[b, j]]
                rows = torch.tensor([b * K + int(c_beam[b, j]) for b, j in ends], dtype=torch.long, device=dev)
                scores = torch.tensor([float(c_score[b, j]) for b, j in ends], dtype=torch.float32, device=dev)
                sents = tokens.index_select(0, rows)[:, 1:step + 1]
                if return_scores:
                    pos = cum.index_select(0, rows)[:, :step]
                    pos[:, step - 1] = scores
                    pos[:, 1:] = pos[:, 1:] - pos[:, :-1]  # cumulative -> per position
                gone = []
                for i, (b, j) in enumerate(ends):
                    hyps = finished[alive[b]]
                    if len(hyps) >= K:
                        continue
                    h = {'tokens': sents[i], 'score': -scores[i]}
                    if return_scores:
                        h['pos_scores'] = -pos[i]
                    hyps.append(h)
                    if len(hyps) == K:
                        gone.append(b)
                if all(len(h) >= K for h in finished):
                    break
                if gone:
                    keep = [b for b in range(nB) if b not in gone]
            idx, new_tok, hyp = select.sel_beam[:nB * K], select.sel_tok[:nB * K], select.sel_score[:nB * K]
            if keep is not None:  # sentences with K finished hypotheses leave the batch
                keep_t = torch.tensor(keep, dtype=torch.long, device=dev)
                idx, new_tok, hyp = (x.view(nB, K).index_select(0, keep_t).reshape(-1) for x in (idx, new_tok, hyp))
                hyp = hyp.contiguous()
                alive = [alive[b] for b in keep]
                plen_alive = plen_alive.index_select(0, keep_t)
                nB = len(keep)
            # `idx` addresses rows of the batch as the decoder just saw it: one gather re-orders and shrinks
            tokens = tokens.index_select(0, idx)
            tokens[:, step] = new_tok
            if return_scores:
                cum = cum.index_select(0, idx)
                if prompt_scores is not None:
                    cum[:, :step - 1] = prompt_scores.cumsum(dim=1).index_select(0, idx)
                cum[:, step - 1] = hyp
            feed = new_tok.unsqueeze(1)
            if keep is not None:  # rows of one sentence are equal: without a departure there is nothing to move
                enc = enc.index_select(0, idx)
                enc_mask = None if enc_mask is None else enc_mask.index_select(0, idx)
            cache = state.get(DecodeCache.KEY)
            if cache is None:
                Decoder.reorder_state(state, idx)
            else:
                cache.reorder_beam(idx, state, keep is not None)
                own = {n for pair in cache.names for n in pair}
                for k, v in state.items():
                    if k not in own and torch.is_tensor(v) and v.dim() > 0:
                        state[k] = v.index_select(0, idx)
        state = None
        if return_scores:
            cum[:, 1:] = cum[:, 1:] - cum[:, :-1]
            cum = -cum
        output = []
        for b0, nbest in enumerate(finished):
            if not nbest:  # the length limit came before an EOS: the first live beam
                i = alive.index(b0)
                h = {'tokens': tokens.view(nB, K, -1)[i, 0, 1:], 'score': -hyp.view(nB, K)[i, 0]}
                if return_scores:
                    h['pos_scores'] = cum.view(nB, K, -1)[i, 0, :-1]
                nbest = [h]
            extra = {k: v[b0] for k, v in enc_layer_outputs.items() if torch.is_tensor(v)}
            nbest = [{**h, **extra, 'normalized_score': h['score'] / (len(h['tokens']) + 1) ** len_penalty} for h in nbest]
            nbest.sort(key=lambda h: h['normalized_score'])
            output.append(nbest)
        for b0, nbest in enumerate(output):
            for h in nbest:
                _uncollate(h, pad, None if src_mask is None else src_mask[b0])
    return output


# ---- sampling search (pasero/decoding.py:906-1221) ---------------------------------------------------------------------
SAMPLE_MODES = {'greedy': 0, 'topk': 1, 'topp': 2, 'full': 3}


class SampleSelect:
    """buffers of pk_sample_select for steps of up to B rows over V tokens, and the call itself.  After `run`:
    `logprob`, `lse`, `kept_mass`, `u` (fp32) and `n_kept` (int32) hold rows [0, B); the tokens are in `token` (int64)
    unless the caller gave a destination of its own (`out`: any int64 view with one element per row, e.g. a column)."""

    def __init__(self, B: int, V: int, device):
        L = lib.load()
        self.B, self.V = B, V
        self.scratch = torch.empty(max(256, L.pk_sample_select_scratch(B, V)), dtype=torch.uint8, device=device)
        self.token = torch.zeros(B, dtype=torch.int64, device=device)
        self.logprob, self.lse, self.kept_mass, self.u = (torch.zeros(B, dtype=torch.float32, device=device) for _ in range(4))
        self.n_kept = torch.zeros(B, dtype=torch.int32, device=device)

    def run(self, logits: Tensor, mode: str, *, top_k: int = 0, top_p: float = 1.0, history: Optional[Tensor] = None,
            penalty: float = 1.0, inv_temperature: float = 1.0, blacklist: Optional[Tensor] = None,
            finished: Optional[Tensor] = None, pad: int = -1, uniforms: Optional[Tensor] = None, seed: int = 0,
            offset: int = 0, forced: Optional[Tensor] = None, out: Optional[Tensor] = None):
        """logits (B, V), any row stride, fp32 / bf16 / fp16; history (B, n) int64 with unit column stride; forced / out:
        int64, one element per row, any stride (they may be the same memory)"""
        require_gpu(logits)
        B = logits.size(0)
        assert logits.dim() == 2 and logits.size(1) == self.V and B <= self.B
        logits, ld = _select_operands(
            logits, self.V, contiguous=((blacklist, torch.int64), (finished, torch.uint8), (uniforms, torch.float32)),
            strided=((history, torch.int64), (forced, torch.int64), (out, torch.int64)))
        n_hist = hist_ld = 0
        if history is not None and history.size(1) > 0:
            assert history.dim() == 2 and history.size(0) == B and history.stride(1) == 1
            n_hist, hist_ld = history.size(1), (history.stride(0) if B > 1 else max(history.size(1), history.stride(0)))
        else:
            history = None

        def strided(t):
            assert t.numel() == B
            return t.stride(0) if t.dim() == 1 else t.stride(0) if t.size(1) == 1 else None
        token = self.token if out is None else out
        check(lib.load().pk_sample_select(
            ptr(logits), ld, self.V, B, dtype_code(logits), ptr(history), hist_ld, n_hist, float(penalty),
            float(inv_temperature), ptr(blacklist), 0 if blacklist is None else blacklist.numel(), ptr(finished), int(pad),
            SAMPLE_MODES[mode], int(top_k), float(top_p), ptr(uniforms), int(seed), int(offset), ptr(forced),
            0 if forced is None else strided(forced), ptr(self.scratch), self.scratch.numel(), ptr(token), strided(token),
            ptr(self.logprob), ptr(self.lse), ptr(self.n_kept), ptr(self.kept_mass), ptr(self.u), stream_ptr()),
            'pk_sample_select')


def sample_on_the_fly(decoder, encoder_outputs, encoder_masks, max_output_len: int, meta: dict, *,
                      return_scores: bool = False, decoder_input: Optional[Tensor] = None,
                      sampling_temperature: float = 1.0, sampling_topk: int = 0, sampling_topp: float = 1.0,
                      return_layers=[], sharded: bool = False, device=None, repeat_penalty: float = 1.0, blacklist=[],
                      stop_sequences=[], uniforms: Optional[Tensor] = None, **kwargs):
    """Drop-in for pasero.decoding.sample_on_the_fly (decoding.py:1005-1221): same keyword signature, a generator that
    yields {'tokens'[, 'pos_scores']} per step (the first yield covers a multi-token prompt).  The decoder call is the
    reference's; between two decoder calls run ONE pk_sample_select (repeat penalty, log-softmax, blacklist, finished
    rows, the choice, the forced prompt token, written straight into `tokens[:, step]`) and the stop test, on the device;
    the only device->host read of a step is the all-finished flag.
    Draws: inverse CDF in the order (probability descending, token id ascending) with one uniform per row and step —
    Philox(seed, offset, row), `(seed, offset) = rng.next_offset()` once per step (seeded by `rng.manual_seed`, or lazily
    from torch's global seed), or `uniforms[i]` (steps, B) for the i-th step when given (replaying a recorded search).
    torch.multinomial's own stream is not reproduced.
    Not implemented (raise, naming the option): ensembles, `return_layers`, `sharded`, decoder-only models."""
    from . import rng
    assert sampling_topk == 0 or sampling_topp == 1, 'combining nucleus sampling and top-k sampling is not allowed'
    decoder, enc, enc_mask, B, pad, eos, decoder_input, plen, lo, hi, max_len, black = _search_setup(
        decoder, encoder_outputs, encoder_masks, return_layers, sharded, 'sample_on_the_fly', device, decoder_input,
        max_output_len, blacklist)
    dev = enc.device
    start = min(lo, max_len - 1)
    tokens = torch.full((B, max_len), pad, dtype=torch.long, device=dev)
    tokens[:, :decoder_input.size(1)] = decoder_input
    stops = [s.to(dev) for s in stop_sequences if len(s) > 0] + [torch.tensor([eos], dtype=torch.long, device=dev)]
    limit = plen + max_output_len
    has_eos = torch.zeros(B, dtype=torch.bool, device=dev)
    if sampling_temperature == 0 or sampling_topk == 1:
        mode = 'greedy'
    elif sampling_topk:
        mode = 'topk'
    elif sampling_topp < 1:
        mode = 'topp'
    else:
        mode = 'full'
    select, prev, state = None, 0, {}
    with torch.no_grad():
        for i, step in enumerate(range(start, max_len)):
            has_eos = has_eos | (limit <= step)
            logits, _ = decoder(enc, enc_mask, tokens[:, prev:step], state=state, meta=meta)
            if select is None:
                select = SampleSelect(B, logits.size(-1), dev)
            seed, offset = rng.next_offset() if (uniforms is None and mode != 'greedy') else (0, 0)
            # inv_temperature stays 1: the reference's single-decoder path never divides by the temperature (`t`,
            # decoding.py:1131, is only used by the ensemble branch); `sampling_temperature` only selects greedy at 0
            col = tokens[:, step:step + 1]  # forced where the prompt reaches this far (pad elsewhere), then the output
            select.run(logits[:, -1], mode, top_k=sampling_topk if mode == 'topk' else 0,
                       top_p=sampling_topp if mode == 'topp' else 1.0, history=tokens[:, :step], penalty=repeat_penalty,
                       blacklist=black, finished=has_eos.view(torch.uint8), pad=pad,
                       uniforms=None if uniforms is None else uniforms[i].to(dev, torch.float32).contiguous(),
                       seed=seed, offset=offset, forced=col if step < hi else None, out=col)
            out = {'tokens': tokens[:, prev + 1:step + 1]}
            if return_scores:
                last = -select.logprob[:B].clone().unsqueeze(1)
                if logits.size(1) > 1:  # the first call carries the prompt: score its tokens with plain torch
                    nxt = tokens[:, prev + 1:step]
                    last = torch.cat([-_prompt_logprobs(logits, nxt), last], dim=1)
                out['pos_scores'] = last
            yield out
            # the stop test (decoding.py:1208-1212) on the device; one host read: the all-finished flag
            for s in stops:
                if step + 1 >= len(s):
                    has_eos = has_eos | (tokens[:, step + 1 - len(s):step + 1] == s).all(dim=1)
            has_eos = has_eos & (plen <= step)  # EOS in the prompt does not count
            prev = step
            if bool(has_eos.all()):
                break


def sampling(decoder, encoder_outputs, encoder_masks, max_output_len: int, meta: dict, *,
             decoder_input: Optional[Tensor] = None, enc_layer_outputs: dict = {}, **kwargs):
    """Drop-in for pasero.decoding.sampling (decoding.py:942-1002): B one-element n-best lists of dicts ('tokens', and
    under `return_scores` 'pos_scores' and 'score' = their sum), cut at the padding as the reference's `uncollate` does."""
    src_mask = encoder_masks[0] if isinstance(encoder_masks, (list, tuple)) and encoder_masks else encoder_masks
    if isinstance(src_mask, (list, tuple)):
        src_mask = None
    hyps = None
    for out in sample_on_the_fly(decoder, encoder_outputs, encoder_masks, max_output_len, meta,
                                 decoder_input=decoder_input, **kwargs):
        for key, values in out.items():
            if hyps is None:
                hyps = [{} for _ in range(len(values))]
            for i, value in enumerate(values):
                hyps[i].setdefault(key, []).append(value)
    pad = getattr(decoder, 'padding_idx')
    for i, hyp in enumerate(hyps):
        for k in hyp:
            hyp[k] = torch.cat(hyp[k])
        hyp.update({k: v[i] for k, v in enc_layer_outputs.items()})
        _uncollate(hyp, pad, None if src_mask is None else src_mask[i])
        if 'pos_scores' in hyp and 'score' not in hyp:
            hyp['score'] = hyp['pos_scores'].sum()
        hyps[i] = [hyp]
    return hyps


def search(*args, **kwargs):
    """Drop-in for pasero.decoding.search (decoding.py:906-916): `sampling` unless beam search was asked for"""
    if not kwargs.pop('sampling', False):
        kwargs['sampling_temperature'] = 0
    if kwargs.get('sampling_temperature', 1.0) > 0 or kwargs.get('beam_size', 1) <= 1:
        return sampling(*args, **kwargs)
    return beam_search(*args, **kwargs)
