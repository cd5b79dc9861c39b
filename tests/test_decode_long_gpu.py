"""The native decoding step (pk_decoder_step, `DecodeCache`) past the lengths every other test stops at, against the CPU oracle
on the whole prefix instead of the per-op incremental path (which runs the same attention kernels and would agree with the
native step on a wrong answer).  132 target tokens cross three things at once:
  * the 64th key: 16-bit self-attention at T = 1 moves from attn_q_kernel to the long-sequence kernel, on operands no
    attention test uses (q: the first D columns of a packed [B][3D] row; K / V: the first t + 1 rows of a [B][cap][D] cache
    whose other rows are unset memory — here NaN, written behind every step, so that a tail row let through shows);
  * t = 64 and t = 128: `DecodeCache._grow`, alone and between `reorder` / `reorder_beam` calls;
  * a source of 70 positions with key padding: cross-attention on the long kernel over the interleaved [B*S][2D] K|V.
The last tests put pk_attn_fwd itself on those two layouts at every length around a tile or capacity boundary, against fp64.

Measured on an MI355X, model / source: worst |native - oracle| over all steps, and for 16 bit the oracle's own bracket
|oracle16 - oracle| it is held to 3 x of (each test prints its figures, and puts them into its failure message):
  fp32 (bound 2e-5 of the step's logit range, 5.8 .. 8.6): post/short 2.4e-6, post/long 2.7e-6, pre/short 3.2e-6, pre/long
        3.2e-6; value cache 1.8e-6 .. 2.2e-6 of a range of 3.8 .. 4.7; argmax positions left out by the gap rule: 1, 0, 0, 0 of 393
  bf16: post/short 2.65e-2 (bracket 2.95e-2), post/long 2.87e-2 (2.48e-2), pre/short 3.32e-2 (3.32e-2), pre/long 2.86e-2 (2.86e-2);
        value cache 2.24e-2 (2.82e-2), 2.45e-2 (2.46e-2), 1.75e-2 (1.75e-2), 1.51e-2 (1.51e-2)
  fp16: post/short 3.42e-3 (3.72e-3), post/long 3.73e-3 (3.50e-3), pre/short 3.73e-3 (3.73e-3), pre/long 2.83e-3 (3.84e-3);
        value cache 3.49e-3 (3.21e-3), 3.03e-3 (3.08e-3), 2.24e-3 (2.24e-3), 1.96e-3 (1.96e-3)
  re-ordered (post/long): fp32 2.7e-6, 0 of 465 positions left out; bf16 2.87e-2 (2.48e-2)
The worst ratio to the bracket is 1.16: the native step is as far from the exact result as the oracle's 16-bit model is."""
import copy

import pytest
import torch

import decode_long_cases as C
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')


def _poison(cache):
    """rows >= t of the self-attention caches are unset memory in production: make them NaN"""
    for buf in cache.k + cache.v:
        buf[:, cache.t:] = float('nan')


def _beam_reorder(state, idx):
    """what `beam_search` does to the incremental state between two steps (pasero_amd/decode.py): the caches by
    `DecodeCache.reorder_beam` — sentences move, so the cross-attention K|V go along — every other tensor by index_select"""
    cache = state['_pk_decode']
    cache.reorder_beam(idx, state, True)
    own = {n for pair in cache.names for n in pair}
    for k, v in state.items():
        if k not in own and torch.is_tensor(v) and v.dim() > 0:
            state[k] = v.index_select(0, idx)


def _decode(c, reorders=None):
    """teacher-forced incremental decoding of case `c` on the GPU: first call 2 tokens, then one native step per token.
    `reorders`: {t: 'state' | 'beam'} — before the token at index t is fed, the batch is re-ordered by IDX through
    `Decoder.reorder_state` / the beam route.  Returns (logits per call [(rows, V) fp64 on the CPU], the row of the case each
    batch row holds at every call, the final state)."""
    from pasero_amd.transformer import Decoder
    dec = copy.deepcopy(c.model).cuda().decoder  # (the case is shared: its model stays where it is)
    enc_out, enc_mask = c.enc_out.to(c.dtype).cuda(), c.enc_mask.cuda()
    tokens = c.tokens.cuda()
    rows = torch.arange(C.B)
    idx = torch.tensor(IDX, device='cuda')
    state, out, held = {}, [], []
    with torch.no_grad():
        lg, _ = dec(enc_out, enc_mask, tokens[:, :2], state=state)
        out.append(lg[:, -1].double().cpu())
        held.append(rows)
        for t in range(2, C.T_LEN):
            how = (reorders or {}).get(t)
            if how is not None:
                assert state['_pk_decode'].t == t
                if how == 'state':
                    Decoder.reorder_state(state, idx)
                else:
                    _beam_reorder(state, idx)
                _poison(state['_pk_decode'])
                enc_out, enc_mask, tokens = enc_out.index_select(0, idx), enc_mask.index_select(0, idx), tokens.index_select(0, idx)
                rows = rows[idx.cpu()]
            lg, _ = dec(enc_out, enc_mask, tokens[:, t:t + 1], state=state)
            assert '_pk_decode' in state, f'the native step did not engage at t = {t}'
            cache = state['_pk_decode']
            assert cache.t == t + 1 and cache.B == rows.numel() and lg.shape[:2] == (rows.numel(), 1)
            _poison(cache)
            out.append(lg[:, -1].double().cpu())
            held.append(rows)
    torch.cuda.synchronize()
    return out, held, state


def _compare(c, out, held, state, what):
    """every step's logits and the published last-layer value cache against the oracle (rows permuted as the batch was):
    fp32 within 2e-5 of the step's range and the same argmax wherever the oracle's two best are further apart than twice that;
    16-bit within 3 x the oracle's own 16-bit bracket"""
    fp32 = c.dtype == torch.float32
    checked = C.checked_positions(c.ref)
    worst, worst_at, left_out, positions, bad = 0.0, None, 0, 0, []
    assert len(out) == C.T_LEN - 1
    for i, (got, rows) in enumerate(zip(out, held), start=1):  # call i - 1 ends at the token of index i
        want = c.ref[rows, i]
        assert got.shape == want.shape
        assert torch.isfinite(got).all(), f'{what}: non-finite logits at t = {i}'
        err = (got - want).abs().max().item()
        if err > worst:
            worst, worst_at = err, i
        if fp32:
            bound = C.FP32_STEP_TOL * want.abs().max().item()
            if err > bound:
                bad.append((i, err, bound))
            ok = checked[rows, i]
            positions += ok.numel()
            left_out += int((~ok).sum())
            same = got.argmax(-1) == want.argmax(-1)
            assert bool(same[ok].all()), f'{what}: argmax differs at t = {i}'
    name = f'dec_{c.cfg.decoder_layers - 1}_self_attn_value'
    got_v, want_v = state[name].double().cpu(), c.ref_v[held[-1]]
    assert got_v.shape == want_v.shape == (held[-1].numel(), C.T_LEN, c.cfg.decoder_attention_heads, 64)
    assert torch.isfinite(got_v).all(), f'{what}: non-finite value cache'
    err_v = (got_v - want_v).abs().max().item()
    if fp32:
        report = (f'{what}: worst |native - oracle| {worst:.3e} at t = {worst_at} (bounds 2e-5 of each step\'s range, range '
                  f'{c.ref.abs().max().item():.3f}); value cache {err_v:.3e} (range {c.ref_v.abs().max().item():.3f}); argmax '
                  f'positions left out by the gap rule: {left_out} of {positions}')
        print(report)
        assert not bad, (report, bad[:5])
        assert err_v <= C.FP32_STEP_TOL * c.ref_v.abs().max().item(), report
        assert left_out <= C.GAP_CAP * positions, report
    else:
        report = (f'{what}: worst |native - oracle| {worst:.3e} at t = {worst_at}, oracle 16-bit bracket {c.bracket:.3e} (ratio '
                  f'{worst / c.bracket:.2f}, bound 3); value cache {err_v:.3e}, bracket {c.bracket_v:.3e} (ratio '
                  f'{err_v / c.bracket_v:.2f}, bound 3)')
        print(report)
        assert worst <= 3 * c.bracket, report
        assert err_v <= 3 * c.bracket_v, report


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('source', list(C.SOURCES))
@pytest.mark.parametrize('model', C.MODELS)
def test_native_step_over_130_tokens_against_the_oracle(model, source, dtype):
    c = C.case(model, source, dtype)
    out, held, state = _decode(c)
    cache = state['_pk_decode']
    assert cache.cap == 256 and cache.t == C.T_LEN and state['offset'] == C.T_LEN  # grew at t = 64 and at t = 128
    _compare(c, out, held, state, f'{model}/{source}/{dtype}')


IDX = [2, 0, 1, 0]  # the batch grows to 4 rows, one is duplicated
# `reorder` while the first buffers are still in use; `reorder_beam` with the cache full (t = cap = 64: the step behind it
# grows with a live spare set), right behind that growth, in the middle, and right behind the second growth (which met the
# spare set of t = 100)
REORDERS = {60: 'state', 64: 'beam', 65: 'beam', 100: 'beam', 129: 'beam'}


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_reordering_around_the_cache_growth(dtype):
    c = C.case('post', 'long', dtype)
    out, held, state = _decode(c, REORDERS)
    cache = state['_pk_decode']
    assert cache.cap == 256 and cache.B == 4 and held[-1].tolist() != list(range(C.B))
    assert sorted(set(held[-1].tolist())) != held[-1].tolist()  # (a row is held twice)
    _compare(c, out, held, state, f'reorder/{dtype}')


# ---- pk_attn_fwd on the decoding step's operand layouts, at the boundary lengths -----------------------------------------
LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1500]
ATTN_TOL = {torch.float32: 1e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}  # test_attention_fwd_bwd (test_kernels_gpu.py)
AB, AH, AD = 3, 2, 128


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _attn_ref(q, k, v, key_pad):
    """softmax(q kᵀ / 8) v per head in fp64: q (B, 1, D), k / v (B, S, D) -> (o (B, 1, D), lse (B, H, 1))"""
    Bq, S = k.size(0), k.size(1)
    qh, kh, vh = (x.double().view(Bq, -1, AH, 64).transpose(1, 2) for x in (q, k, v))
    sc = qh @ kh.transpose(2, 3) / 8.0
    if key_pad is not None:
        sc = sc.masked_fill(key_pad[:, None, None, :], -float('inf'))
    lse = torch.logsumexp(sc, dim=-1)
    o = torch.softmax(sc, dim=-1) @ vh
    return o.transpose(1, 2).reshape(Bq, 1, AD), lse


def _check_attn(F, q, k, v, key_pad, ref, dtype, what):
    o, lse = F.attn_fwd(q, k, v, AH, key_pad, False, 1.0 / 8.0)
    torch.cuda.synchronize()
    assert o.shape == (AB, 1, AD) and lse.shape == (AB, AH, 1)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all(), what
    err = rel_err(o, ref[0])
    assert err < ATTN_TOL[dtype], (what, err)
    # lse = log sum exp of fp32-accumulated scores of O(1): fp32 round-off for every type
    assert (lse.double().cpu() - ref[1]).abs().max().item() < 1e-4, what


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('S', LENGTHS)
def test_attention_on_the_self_attention_layout_of_a_step(S, dtype):
    """q in a packed [B][3D] row, K / V the first S rows of a [B][cap][D] cache whose other rows are NaN"""
    from pasero_amd import functional as F
    cap = max(64, 1 << S.bit_length())  # the next power of two >= max(64, S + 1)
    assert cap >= S + 1 and (cap == 64 or cap // 2 < S + 1)
    gen = torch.Generator().manual_seed(1000 + S)
    qkv = torch.randn(AB, 1, 3 * AD, generator=gen).to(dtype)
    caches = []
    for _ in range(2):
        buf = torch.full((AB, cap, AD), float('nan'), dtype=dtype)
        buf[:, :S] = torch.randn(AB, S, AD, generator=gen).to(dtype)
        caches.append(buf)
    ref = _attn_ref(qkv[..., :AD], caches[0][:, :S], caches[1][:, :S], None)
    qkv, ck, cv = qkv.cuda(), caches[0].cuda(), caches[1].cuda()
    q, k, v = qkv[..., :AD], ck[:, :S], cv[:, :S]
    assert q.stride() == (3 * AD, 3 * AD, 1) and k.stride() == (cap * AD, AD, 1)
    _check_attn(F, q, k, v, None, ref, dtype, f'self S={S} cap={cap} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('S', LENGTHS)
def test_attention_on_the_cross_attention_layout_of_a_step(S, dtype):
    """K and V interleaved in one [B*S][2D] projection, key padding from the lengths [S, max(1, S - 5), 1]"""
    from pasero_amd import functional as F
    gen = torch.Generator().manual_seed(2000 + S)
    q = torch.randn(AB, 1, AD, generator=gen).to(dtype)
    kv = torch.randn(AB, S, 2 * AD, generator=gen).to(dtype)
    key_pad = O.len_to_mask(torch.tensor([S, max(1, S - 5), 1]), S)
    ref = _attn_ref(q, kv[..., :AD], kv[..., AD:], key_pad)
    q, kv = q.cuda(), kv.cuda()
    k, v = kv[..., :AD], kv[..., AD:]
    assert k.stride() == (S * 2 * AD, 2 * AD, 1) and v.data_ptr() == k.data_ptr() + AD * kv.element_size()
    _check_attn(F, q, k, v, key_pad.cuda(), ref, dtype, f'cross S={S} {dtype}')
