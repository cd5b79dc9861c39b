"""The reference of tests/test_decode_long_gpu.py is fit for the job (no GPU needed): the oracle's full-prefix decoder over 132
tokens agrees with its own incremental decoding, in its pinned fp32 form and in the fp64 form the GPU test compares with; the
argmax comparison of the GPU test leaves out at most 2 % of the positions; the 16-bit brackets are real numbers.  And the host
side of the native step's cache growth (`DecodeCache._grow`) on CPU tensors."""
import ctypes

import pytest
import torch

import decode_long_cases as C

CASES = [(m, s) for m in C.MODELS for s in C.SOURCES]


@pytest.mark.parametrize('model,source', CASES)
def test_oracle_incremental_decoding_reproduces_its_full_prefix_logits(model, source):
    """fp32, the oracle's pinned form: 132 one-token calls on the incremental state against one call on the whole prefix, 1e-5
    of the logit range — the GPU test's reference is not an artefact of one evaluation order.  fp64, what the GPU test
    compares with: the same two at 1e-12, and within 1e-5 of the fp32 form (the oracle's functions take fp64 unchanged)."""
    c32 = C.case(model, source, torch.float32, torch.float32)
    assert c32.ref.dtype == torch.float32 and c32.ref.shape == (C.B, C.T_LEN, c32.model.decoder.embed_tokens.weight.size(0))
    inc, inc_v = C.incremental_logits(c32.P, c32.cfg, c32.enc_out, c32.enc_mask, c32.tokens)
    scale = c32.ref.abs().max().item()
    assert torch.isfinite(c32.ref).all() and scale > 1
    assert (inc - c32.ref).abs().max().item() <= 1e-5 * scale
    assert (inc_v - c32.ref_v).abs().max().item() <= 1e-5 * c32.ref_v.abs().max().item()
    c64 = C.case(model, source)
    assert c64.ref.dtype == torch.float64 and c64.ref_v.dtype == torch.float64
    inc, inc_v = C.incremental_logits(c64.P, c64.cfg, c64.enc_out, c64.enc_mask, c64.tokens)
    assert (inc - c64.ref).abs().max().item() <= 1e-12 * scale
    assert (inc_v - c64.ref_v).abs().max().item() <= 1e-12 * c64.ref_v.abs().max().item()
    assert torch.equal(c64.tokens, c32.tokens) and torch.equal(c64.enc_mask, c32.enc_mask)
    assert (c64.ref - c32.ref.double()).abs().max().item() <= 1e-5 * scale
    assert (c64.ref_v - c32.ref_v.double()).abs().max().item() <= 1e-5 * c32.ref_v.abs().max().item()


@pytest.mark.parametrize('model,source', CASES)
def test_argmax_comparison_leaves_out_at_most_two_percent(model, source):
    """positions whose two best logits are closer than 4e-5 of the step's logit range (twice the fp32 bound on step logits)
    say nothing about the argmax: at most 2 % of them, for the seeds the GPU test uses"""
    c = C.case(model, source)
    checked = C.checked_positions(c.ref)
    assert checked.shape == (C.B, C.T_LEN)
    left_out = int((~checked).sum())
    print(f'{model}/{source}: {left_out} of {checked.numel()} positions under the gap rule')
    assert left_out <= C.GAP_CAP * checked.numel()


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('model,source', CASES)
def test_sixteen_bit_brackets_are_finite_and_not_zero(model, source, dtype):
    c = C.case(model, source, dtype)
    print(f'{model}/{source}/{dtype}: bracket logits {c.bracket:.3e} (range {c.ref.abs().max().item():.3f}), '
          f'value cache {c.bracket_v:.3e} (range {c.ref_v.abs().max().item():.3f})')
    assert torch.isfinite(c.ref16).all() and torch.isfinite(c.ref16_v).all()
    for bracket, ref in ((c.bracket, c.ref), (c.bracket_v, c.ref_v)):
        # 16-bit storage moves a result, and by less than the result: neither switched off nor a blow-up
        assert 0 < bracket < 0.25 * ref.abs().max().item()
    assert C.case(model, source, dtype) is c  # computed once, shared


def test_reference_restores_the_oracle_activation_dtype():
    from oracle import ref_cpu as O
    c = C.case('post', 'short', torch.bfloat16)
    assert O.ACT_DTYPE is None
    with pytest.raises(KeyError):
        C.full_logits({}, c.cfg, c.enc_out, c.enc_mask, c.tokens, act_dtype=torch.bfloat16)
    assert O.ACT_DTYPE is None


@pytest.mark.parametrize('spare', [False, True])
def test_cache_growth_keeps_every_row_and_drops_the_spare_set(spare):
    """`DecodeCache._grow` on CPU tensors (it is host code: allocation, a copy, the pointer tables): capacity doubles, rows < t
    of the first B sentences survive bit for bit in buffers of exactly B rows (a buffer of `reorder_beam` may hold more), the
    spare set of `reorder_beam` — sized for the old capacity — is dropped, the tables point at the new buffers"""
    from pasero_amd.decode import DecodeCache
    Bc, rows, t, cap, D, n = 3, 4, 64, 64, 128, 2
    cache = object.__new__(DecodeCache)
    gen = torch.Generator().manual_seed(5)
    cache.B, cache.t, cache.cap, cache.D = Bc, t, cap, D
    cache.names = [(f'dec_{i}_self_attn_key', f'dec_{i}_self_attn_value') for i in range(n)]
    cache.k = [torch.randn(rows, cap, D, generator=gen) for _ in range(n)]
    cache.v = [torch.randn(rows, cap, D, generator=gen) for _ in range(n)]
    cache.cross = [torch.randn(Bc * 5, 2 * D, generator=gen) for _ in range(n)]
    if spare:
        cache._spare = ([torch.empty_like(x) for x in cache.k], [torch.empty_like(x) for x in cache.v])
    old_k, old_v = list(cache.k), list(cache.v)
    cache._grow()
    assert cache.cap == 2 * cap and cache._spare is None
    for new, old in zip(cache.k + cache.v, old_k + old_v):
        assert new.shape == (Bc, 2 * cap, D) and new.is_contiguous() and new.data_ptr() != old.data_ptr()
        assert torch.equal(new[:, :t], old[:Bc, :t])
    for tab, tensors in ((cache.k_tab, cache.k), (cache.v_tab, cache.v), (cache.c_tab, cache.cross)):
        assert [ctypes.cast(tab, ctypes.POINTER(ctypes.c_void_p))[i] for i in range(n)] == [x.data_ptr() for x in tensors]
