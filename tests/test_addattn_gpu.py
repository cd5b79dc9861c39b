"""pk_addattn_fwd / pk_addattn_bwd (csrc/addattn.hip) through `hybrid.AdditiveAttentionFn` against tests/hybrid_ref.py in fp64
over the same storage-type inputs.  The tolerance is measured (the rule of test_adapter_rows_gpu.py): the reference's four
lines run in the same storage type on the GPU on every input, and the kernel may be off by at most twice that path's own
error plus one ulp of the storage type at the output's magnitude.  The kernels write into outputs the test filled with NaN, over
a scratch buffer filled with NaN.  Exact properties: probability 0 at masked keys, two runs
agree bit for bit (no atomics).  Rows of probabilities sum to 1 within: half an ulp of 1 in the storage type (each entry is
rounded once, by at most half an ulp of itself) plus the fp32 arithmetic before it — the normaliser is a sum along a chain of
ceil(S / 64) + 6 additions (a lane's keys, then the wave butterfly), then one reciprocal and one product, 2^-24 each."""
import math

import pytest
import torch

import hybrid_ref as R

pytestmark = pytest.mark.gpu

# (B, T, S, H, D): one query (a decoding step) and fewer keys than lanes; sizes that are no multiple of any tile and H = 96;
# five query tiles, three key passes of a wave, D != H; the `_big` and `_wide` presets' widths (more than 64 KiB of LDS in backward)
SHAPES = [(2, 1, 5, 64, 128), (3, 7, 37, 96, 128), (2, 33, 130, 64, 64), (1, 3, 9, 1024, 1024), (1, 2, 9, 2048, 1024)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
MANT = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}
_cache = {}


def make(B, T, S, H, D, dtype, masked):
    key = (B, T, S, H, D, dtype, masked)
    if key not in _cache:
        g = torch.Generator().manual_seed(T * 1000 + S * 10 + H + D)
        rnd = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()
        pad = None
        if masked:  # padded tails of different lengths; the first sentence keeps every key
            lengths = [S - (b * (S - 1)) // max(B - 1, 1) if b else S for b in range(B)]
            lengths = [max(1, min(S, n)) for n in lengths]
            pad = (torch.arange(S)[None, :] >= torch.tensor(lengths)[:, None]).cuda()
        _cache[key] = {'q': rnd(B, T, H), 'k': rnd(B, S, H), 'w': rnd(H, scale=2 * H ** -0.5), 'value': rnd(B, S, D),
                       'dctx': rnd(B, T, D), 'pad': pad}
    return _cache[key]


def nan_like(*tensors):
    return tuple(torch.full_like(t, float('nan')) for t in tensors)


def direct(t):
    """-> probs, ctx, dq, dk, dw, dvalue through the functional wrappers, every output and the scratch NaN before the call"""
    from pasero_amd import functional as F, lib
    B, T, H = t['q'].shape
    S, D = t['k'].size(1), t['value'].size(2)
    probs, ctx = F.addattn_fwd(t['q'], t['k'], t['w'], t['pad'], t['value'],
                               out=nan_like(t['q'].new_empty(B, T, S), t['q'].new_empty(B, T, D)))
    nbytes = lib.load().pk_addattn_bwd_scratch(B, T, S, H)
    lib.workspace(nbytes, t['q'].device, 'addattn').fill_(0xFF)
    grads = F.addattn_bwd(t['dctx'], t['q'], t['k'], t['w'], t['value'], probs, out=nan_like(t['q'], t['k'], t['w'], t['value']))
    return [probs, ctx, *grads]


def bound_check(what, got, per, want, dtype, worst):
    err_new = (got.double().cpu() - want).abs().max().item()
    err_per = (per.double().cpu() - want).abs().max().item()
    ulp = 2.0 ** (math.floor(math.log2(max(want.abs().max().item(), 1e-30))) - MANT[dtype])
    ratio = err_new / max(2 * err_per + ulp, 1e-300)
    worst[0] = max(worst[0], ratio)
    print(f'  {what}: kernel {err_new:.3e} per-op {err_per:.3e} ulp {ulp:.3e} -> {ratio:.3f} of the bound')
    assert torch.isfinite(got).all(), what
    assert err_new <= 2 * err_per + ulp, what


def run(fn, t, double=False):
    """-> probs, ctx, dq, dk, dw, dvalue of one implementation"""
    conv = (lambda v: v.double().cpu()) if double else (lambda v: v)
    leaves = {k: conv(t[k]).detach().clone().requires_grad_() for k in ('q', 'k', 'w', 'value')}
    pad = t['pad'] if (t['pad'] is None or not double) else t['pad'].cpu()
    probs, ctx = fn(leaves['q'], leaves['k'], leaves['w'], pad, leaves['value'])
    ctx.backward(conv(t['dctx']))
    return [probs.detach(), ctx.detach()] + [leaves[k].grad for k in ('q', 'k', 'w', 'value')]


def kernel(q, k, w, pad, value):
    from pasero_amd.hybrid import AdditiveAttentionFn
    ctx, probs = AdditiveAttentionFn.apply(q, k, w, None, pad, value)
    return probs, ctx


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('masked', [False, True], ids=['no-mask', 'padded-tails'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_forward_and_backward(shape, masked, dtype):
    t = make(*shape, dtype, masked)
    want = run(R.additive_attention, t, double=True)
    per = run(R.additive_attention, t)
    got = direct(t)
    torch.cuda.synchronize()
    worst = [0.0]
    for name, g, p, w in zip(('probs', 'ctx', 'dq', 'dk', 'dw', 'dvalue'), got, per, want):
        bound_check(name, g, p, w, dtype, worst)
    probs = got[0]
    if masked:
        where = t['pad'][:, None, :].expand_as(probs)
        assert (probs[where] == 0).all(), 'a masked key has a probability'
        assert (probs[~where] >= 0).all()
        assert (got[3][t['pad']] == 0).all() and (got[5][t['pad']] == 0).all(), 'a masked key has a gradient'
    chain = (shape[2] + 63) // 64 + 6 + 2
    assert (probs.double().sum(dim=-1) - 1).abs().max().item() <= 2.0 ** -(MANT[dtype] + 1) + chain * 2.0 ** -24
    again = run(kernel, t)   # the same through the autograd function: a second run, bit for bit
    assert all(torch.equal(a, b) for a, b in zip(got, again)), 'two runs differ'
    print(f'{shape} {dtype} masked {masked}: worst {worst[0]:.3f} of the bound')
