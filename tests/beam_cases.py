"""seeded inputs of the pk_beam_select tests, shared by the CPU check of the seeds and the GPU test"""
import math

import torch

DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}


def _case(dtype, V, K, B, variant, seed):
    return dict(dtype=dtype, V=V, K=K, B=B, variant=variant, seed=seed)


SELECT_CASES = []
_seed = 0
for _dtype in ('f32', 'bf16', 'f16'):
    for _V, _K, _B in ((61, 1, 4), (61, 3, 64), (61, 16, 1), (1003, 5, 4), (1003, 16, 64), (8032, 5, 64), (8032, 3, 1),
                       (70376, 5, 64), (70376, 16, 4), (256206, 5, 64), (256206, 1, 4), (256206, 16, 4)):
        _seed += 1
        SELECT_CASES.append(_case(_dtype, _V, _K, _B, 'plain', _seed))
for _i, _variant in enumerate(('first', 'forced', 'blacklist', 'sparse', 'eos_in', 'eos_out', 'eos_nocount')):
    for _dtype, _V, _K, _B in (('f32', 1003, 5, 4), ('bf16', 8032, 3, 4), ('f16', 70376, 5, 4), ('bf16', 61, 16, 4)):
        _seed += 1
        SELECT_CASES.append(_case(_dtype, _V, _K, _B, _variant, _seed))
# rows that end exactly at, one past and one short of a 2048-token chunk (appended: the seeds above stay what they were)
for _dtype in ('f32', 'bf16', 'f16'):
    for _V, _K, _B in ((2048, 16, 4), (2049, 5, 4), (4096, 3, 4), (2047, 16, 1)):
        for _variant in ('plain', 'blacklist', 'forced'):
            _seed += 1
            SELECT_CASES.append(_case(_dtype, _V, _K, _B, _variant, _seed))


def case_id(c):
    return f"{c['dtype']}-V{c['V']}-K{c['K']}-B{c['B']}-{c['variant']}"


def make_select_case(c, device):
    """logits (B*K, ld) with ld != V (the tensor handed out is the [:, :V] view), hyp, and the variant's extras"""
    gen = torch.Generator().manual_seed(1000 + c['seed'])
    V, K, B, variant = c['V'], c['K'], c['B'], c['variant']
    rows, ld = B * K, (V + 7) // 8 * 8 + 8
    x = torch.randn(rows, ld, generator=gen) * 3.0
    eos, pad = 2, 1
    x[:, eos] -= 4.0  # EOS rarely wins unless a variant says so
    hyp = -torch.rand(rows, generator=gen) * 20.0
    forced = eos_counts = None
    blacklist = ()
    if variant == 'first':
        hyp = None
    elif variant == 'forced':
        forced = torch.randint(4, V, (rows,), generator=gen)
        forced[::3] = pad
        forced[1::5] = eos
    elif variant == 'blacklist':
        top = x[:, :V].argmax(dim=1)
        blacklist = tuple(sorted({int(top[0]), int(top[-1]), 5, V - 1}))
    elif variant == 'sparse':  # -inf but for three tokens per row: fewer than 2K finite
        keep = torch.randint(0, V, (rows, 3), generator=gen)
        y = torch.full_like(x, -math.inf)
        y.scatter_(1, keep, x.gather(1, keep))
        x = y
    elif variant == 'eos_in':   # EOS is the best continuation of beam 0 of every sentence
        x[::K, eos] = x[::K, :V].max(dim=1).values + 2.0
        hyp[::K] = hyp.view(B, K).max(dim=1).values + 1.0
    elif variant == 'eos_out':  # EOS lands among the 2K candidates but behind the first K
        order = x[::K, :V].sort(dim=1, descending=True).values
        x[::K, eos] = (order[:, K] + order[:, K + 1]) / 2 if V > K + 2 else order[:, -1]
        hyp[::K] = hyp.view(B, K).max(dim=1).values + 30.0
    elif variant == 'eos_nocount':
        x[::K, eos] = x[::K, :V].max(dim=1).values + 2.0
        hyp[::K] = hyp.view(B, K).max(dim=1).values + 1.0
        eos_counts = torch.zeros(B, dtype=torch.uint8)
        eos_counts[1::2] = 1
    x = x.to(DTYPES[c['dtype']]).to(device)
    mv = lambda t: None if t is None else t.to(device)
    return {'logits': x[:, :V], 'hyp': mv(hyp), 'forced': mv(forced), 'blacklist': blacklist, 'eos_counts': mv(eos_counts),
            'eos': eos, 'pad': pad}


def skipped_share(ref, gap=1e-4):
    """share of the finite candidate positions whose fp64 score is closer than `gap` to a neighbour (index not checked)"""
    return float((~clear_positions(ref, gap) & torch.isfinite(ref['score'])).sum()) / max(1, int(torch.isfinite(ref['score']).sum()))


def clear_positions(ref, gap=1e-4):
    """(B, 2K) bool: finite and more than `gap` away from both neighbours (the (2K+1)-th score counts as a neighbour), or exactly equal to it"""
    s = ref['score']
    nxt = torch.cat([s[:, 1:], (ref['extra'] if ref['extra'] is not None else torch.full_like(s[:, 0], -math.inf))[:, None]], dim=1)
    prv = torch.cat([torch.full_like(s[:, :1], math.inf), s[:, :-1]], dim=1)
    ok = lambda d: (d > gap) | (d == 0)  # an exact tie is decided by the tie rule: checked, not skipped
    return torch.isfinite(s) & ok(s - nxt) & ok(prv - s)
