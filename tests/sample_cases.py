"""seeded inputs of the pk_sample_select tests, shared by the CPU check of the seeds and the GPU test"""
import math

import torch

DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
MODES = {'greedy': {}, 'topk40': {'top_k': 40}, 'topp09': {'top_p': 0.9}, 'full': {}}

SAMPLE_CASES = []
_seed = 0
for _dtype in ('f32', 'bf16', 'f16'):
    for _V, _B in ((61, 1), (61, 256), (1003, 7), (8032, 256), (8032, 1), (70376, 7), (256206, 7), (256206, 256)):
        for _mode in MODES:
            if _V == 256206 and _B == 256 and (_dtype == 'f16' or _mode in ('greedy', 'full')):
                continue  # the largest shape: one stochastic filter per dtype is enough (fp64 comparator memory and time)
            _seed += 1
            SAMPLE_CASES.append(dict(dtype=_dtype, V=_V, B=_B, mode=_mode, variant='plain', seed=_seed))
for _variant in ('blacklist', 'finished', 'forced', 'penalty', 'k1', 'kV', 'p_tiny', 'single', 'equal', 'temperature',
                 'unaligned'):
    for _dtype, _V, _B in (('f32', 1003, 7), ('bf16', 8032, 7), ('f16', 61, 7)):
        for _mode in (('topk40',) if _variant in ('k1', 'kV') else ('topp09',) if _variant == 'p_tiny'
                      else ('greedy', 'topk40', 'topp09', 'full')):
            _seed += 1
            SAMPLE_CASES.append(dict(dtype=_dtype, V=_V, B=_B, mode=_mode, variant=_variant, seed=_seed))

# the rest of the V x B cross product (appended, so that the seeds above stay what they were).  Left out on purpose: at
# (256 206, 256) greedy, full and every f16 case — select_ref's fp64 sort of 65 M elements per case, in memory and time
for _dtype in ('f32', 'bf16', 'f16'):
    for _V, _B in ((61, 7), (1003, 1), (1003, 256), (8032, 7), (70376, 1), (70376, 256), (256206, 1)):
        for _mode in MODES:
            _seed += 1
            SAMPLE_CASES.append(dict(dtype=_dtype, V=_V, B=_B, mode=_mode, variant='plain', seed=_seed))

# rows that end exactly at and one past a 2048-token chunk, and two full chunks (appended, as above)
for _dtype in ('f32', 'bf16', 'f16'):
    for _V, _B in ((2048, 7), (2049, 7), (4096, 7)):
        for _mode in MODES:
            for _variant in ('plain', 'blacklist', 'penalty', 'finished'):
                _seed += 1
                SAMPLE_CASES.append(dict(dtype=_dtype, V=_V, B=_B, mode=_mode, variant=_variant, seed=_seed))


def case_id(c):
    return f"{c['dtype']}-V{c['V']}-B{c['B']}-{c['mode']}-{c['variant']}"


def make_sample_case(c, device):
    """logits (B, V) as a view of (B, ld), ld != V, and the keyword arguments shared by SampleSelect.run and select_ref"""
    gen = torch.Generator().manual_seed(5000 + c['seed'])
    V, B, variant = c['V'], c['B'], c['variant']
    mode = 'greedy' if c['mode'] == 'greedy' else c['mode'].rstrip('0123456789')
    ld = (V + 7) // 8 * 8 + 8
    sigma = 3.0 if V <= 8032 else 6.0  # (a large vocabulary under a flat distribution puts the nucleus' edge among
    x = torch.randn(B, ld, generator=gen) * sigma  # tokens thinner than any cumulative sum resolves)
    pad = 1
    kw = dict(MODES[c['mode']])
    if mode == 'topk':
        kw['top_k'] = min(kw['top_k'], V)
    off = 0
    if variant == 'blacklist':
        kw['blacklist'] = tuple(sorted({int(x[0, :V].argmax()), int(x[-1, :V].argmax()), 5, V - 1}))
    elif variant == 'finished':
        kw['finished'] = (torch.arange(B) % 2 == 0).to(torch.uint8)
    elif variant == 'forced':
        f = torch.randint(4, V, (B,), generator=gen)
        f[::3] = pad
        kw['forced'] = f
        kw['blacklist'] = (int(f[1]),)  # a forced token that is masked: logprob -inf
    elif variant == 'penalty':
        h = torch.randint(0, V, (B, 12), generator=gen)
        h[:, 5] = h[:, 2]  # duplicates apply once
        h[:, 7] = x[:, :V].argmax(dim=1)
        h[:, 11] = pad
        kw.update(history=h, penalty=1.3)
    elif variant == 'k1':
        kw['top_k'] = 1
    elif variant == 'kV':
        kw['top_k'] = V
    elif variant == 'p_tiny':
        kw['top_p'] = 1e-6
    elif variant == 'single':  # one finite logit per row
        keep = torch.randint(0, V, (B, 1), generator=gen)
        y = torch.full_like(x, -math.inf)
        y.scatter_(1, keep, x.gather(1, keep))
        x = y
    elif variant == 'equal':
        x = torch.full_like(x, 0.75)
    elif variant == 'temperature':
        kw['inv_temperature'] = 1.0 / 0.7
    elif variant == 'unaligned':
        ld, off = ld + 1, 1
        x = torch.randn(B, ld, generator=gen) * sigma
    u = torch.floor(torch.rand(B, generator=gen, dtype=torch.float64) * 2 ** 24) / 2 ** 24
    x = x.to(DTYPES[c['dtype']]).to(device)
    for k in ('finished', 'forced', 'history'):
        if k in kw:
            kw[k] = kw[k].to(device)
    return {'logits': x[:, off:off + V], 'mode': mode, 'u': u.float().to(device), 'pad': pad, 'kw': kw}


def reference_tau(ref):
    """tau of the issue: 2 x max |fp32 sort(descending).cumsum - the same in fp64| / M on this input, plus fp32 eps, from
    CPU torch alone (`ref`: select_ref's result)"""
    lp = ref['lp'].cpu()
    p32 = lp.float().exp().sort(dim=-1, descending=True).values.cumsum(dim=-1)
    p64 = lp.exp().sort(dim=-1, descending=True).values.cumsum(dim=-1)
    M = ref['kept_mass'].cpu().clamp(min=1e-300)
    err = ((p32.double() - p64).abs().max(dim=-1).values / M)
    err = err[torch.isfinite(err) & (ref['kept_mass'].cpu() > 0)]
    return 2 * (float(err.max()) if err.numel() else 0.0) + torch.finfo(torch.float32).eps


def boundary_clear(ref, tau):
    """rows whose kept set is checked: boundary margin above tau (relative to M for top-p), or an exact tie"""
    m = ref['boundary_margin']
    return (m > tau * ref['kept_mass'].clamp(min=1e-300)) | (m == 0) | torch.isinf(m)
