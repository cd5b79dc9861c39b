"""pk_sample_select (csrc/sample.hip) against tests/sample_ref.py's fp64 `select_ref` on seeded inputs
(tests/sample_cases.py): values, kept set, the drawn token's cumulative interval, repeatability, the draws, the
distribution of many draws from one row, and the refusals."""
import math

import pytest
import torch

from sample_cases import SAMPLE_CASES, case_id, make_sample_case, reference_tau, boundary_clear
from sample_ref import select_ref

pytestmark = pytest.mark.gpu
OUTS = ('token', 'logprob', 'lse', 'n_kept', 'kept_mass', 'u')


def run_select(inp, uniforms=True, seed=0, offset=0):
    from pasero_amd.decode import SampleSelect
    x = inp['logits']
    sel = SampleSelect(x.size(0), x.size(1), 'cuda')
    kw = dict(inp['kw'])
    bl = kw.pop('blacklist', ())
    sel.run(x, inp['mode'], blacklist=torch.tensor(bl, dtype=torch.int64, device='cuda') if bl else None, pad=inp['pad'],
            uniforms=inp['u'] if uniforms else None, seed=seed, offset=offset, **kw)
    torch.cuda.synchronize()
    return {k: getattr(sel, k).clone() for k in OUTS}


@pytest.mark.parametrize('case', SAMPLE_CASES, ids=case_id)
def test_sample_select_against_fp64(case):
    """lse / logprob: within 2 x torch's own fp32 log_softmax error against fp64 on the same input, plus one ulp.
    Kept set: n_kept equal on every row whose fp64 boundary margin exceeds tau (or is an exact tie), kept_mass within
    tau * M; at most 5 % of the rows skipped.  Token: inside the kept set and u * M within tau * M of its fp64 cumulative
    interval; greedy and forced rows: equal.  tau = 2 x torch's fp32 sort + cumsum error on this input / M + fp32 eps.
    Every case runs twice: all outputs bitwise equal."""
    inp = make_sample_case(case, 'cuda')
    x, mode = inp['logits'], inp['mode']
    B, V = x.shape
    assert x.stride(0) != V  # ld != V
    got = run_select(inp)
    again = run_select(inp)
    for k in OUTS:
        assert torch.equal(got[k].view(torch.int32) if got[k].dtype == torch.float32 else got[k],
                           again[k].view(torch.int32) if again[k].dtype == torch.float32 else again[k]), k
    ref = select_ref(x, mode, u=inp['u'], pad=inp['pad'], **inp['kw'])
    # ---- values: the reference arithmetic's own error on the same (penalised, scaled) input ----
    from sample_ref import penalised_logits
    xs = penalised_logits(x, inp['kw'].get('history'), inp['kw'].get('penalty', 1.0)).float()
    if 'inv_temperature' in inp['kw']:
        xs = xs * torch.tensor(inp['kw']['inv_temperature'], dtype=torch.float32, device='cuda')
    xc = xs.cpu()
    s32, s64 = xc.log_softmax(dim=-1), xc.double().log_softmax(dim=-1)
    both = torch.isfinite(s64)
    err_torch = (s32.double() - s64)[both].abs().max().item()
    lse32 = torch.logsumexp(xc, dim=-1).double() - torch.logsumexp(xc.double(), dim=-1)
    err_lse_torch = max(lse32.abs().max().item(), err_torch)
    del s32, s64, xc
    fin = torch.isfinite(ref['logprob'])
    assert torch.equal(torch.isfinite(got['logprob']), fin)
    eps = torch.finfo(torch.float32).eps
    err_lp = (got['logprob'].double() - ref['logprob'])[fin].abs().max().item() if fin.any() else 0.0
    ulp_lp = eps * ref['logprob'][fin].abs().max().item() if fin.any() else 0.0
    err_lse = (got['lse'].double() - ref['lse']).abs().max().item()
    ulp_lse = eps * ref['lse'].abs().max().item()
    tau = reference_tau(ref)
    clear = boundary_clear(ref, tau)
    skipped = float((~clear).float().mean())
    print(f'{case_id(case)}: logprob err {err_lp:.3e} lse err {err_lse:.3e} (torch fp32 {err_torch:.3e} / {err_lse_torch:.3e}), '
          f'tau {tau:.3e}, skipped rows {skipped:.4f}')
    assert err_lp <= 2 * err_torch + ulp_lp
    assert err_lse <= 2 * err_lse_torch + ulp_lse
    # ---- token ----
    tok = got['token']
    forced = inp['kw'].get('forced')
    is_forced = torch.zeros(B, dtype=torch.bool, device='cuda') if forced is None else forced != inp['pad']
    assert torch.equal(tok[is_forced], ref['token'][is_forced])
    if mode == 'greedy':
        assert torch.equal(tok, ref['token'])
        return
    # ---- kept set ----
    assert skipped <= 0.05
    M = ref['kept_mass']
    assert torch.equal(got['n_kept'].long()[clear], ref['n_kept'][clear])
    assert bool(((got['kept_mass'].double() - M).abs()[clear] <= tau * M[clear] + 1e-300).all())
    assert torch.equal(got['u'], inp['u'])
    # ---- the drawn token's fp64 interval in the rule's order ----
    free = ~is_forced & (M > 0)
    assert bool(((tok >= 0) & (tok < V)).all())
    rank = torch.empty_like(ref['order'])
    rank.scatter_(1, ref['order'], torch.arange(V, device='cuda').expand(B, V))
    r = rank.gather(1, tok[:, None]).squeeze(1)
    hi_c = ref['cum'].gather(1, r[:, None]).squeeze(1)
    lo_c = torch.where(r > 0, ref['cum'].gather(1, (r - 1).clamp(min=0)[:, None]).squeeze(1), torch.zeros_like(hi_c))
    target = inp['u'].double() * M
    inside = (r < ref['n_kept']) | ~clear  # (a skipped row's kept set may be one token longer)
    assert bool(inside[free].all())
    assert bool(((lo_c - tau * M <= target) & (target < hi_c + tau * M))[free].all())
    assert bool(torch.isfinite(ref['lp'].gather(1, tok[:, None]).squeeze(1))[free].all())


def _inp(B, V, mode, dtype=torch.bfloat16, seed=3, **kw):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(1, V, generator=gen) * 3.0).to(dtype).cuda().expand(B, V).contiguous()
    return {'logits': x, 'mode': mode, 'u': torch.zeros(B, device='cuda'), 'pad': 1, 'kw': kw}


def test_draws():
    """u_out lies in [0, 1), is the same for equal (seed, offset, row), differs between offsets and between rows, and
    65 536 draws in 16 equal bins give a Pearson chi-square below the 1 - 1e-4 quantile of chi2(15), 44.3"""
    inp = _inp(65536 // 8, 61, 'full')
    us = [run_select(inp, uniforms=False, seed=1234, offset=o)['u'] for o in range(1, 9)]
    again = run_select(inp, uniforms=False, seed=1234, offset=1)['u']
    assert torch.equal(us[0], again) and not torch.equal(us[0], us[1])
    assert not torch.equal(us[0], run_select(inp, uniforms=False, seed=1235, offset=1)['u'])
    u = torch.cat(us)
    assert bool(((u >= 0) & (u < 1)).all()) and u.unique().numel() > 0.99 * u.numel()
    counts = torch.histc(u.double().cpu(), bins=16, min=0.0, max=1.0)
    expect = u.numel() / 16
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print(f'chi2(15) of 65536 draws: {chi2:.2f}')
    assert chi2 < 44.3


def chi2_quantile(df, z=3.719016485455709):
    """the 1 - 1e-4 quantile of chi2(df): scipy's where it is importable, else Wilson-Hilferty (z = the normal quantile)"""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1 - 1e-4, df))
    except ImportError:
        pass
    return df * (1 - 2 / (9 * df) + z * math.sqrt(2 / (9 * df))) ** 3


@pytest.mark.parametrize('mode,kw', [('topp', {'top_p': 0.9}), ('topk', {'top_k': 40})])
def test_distribution_of_many_draws(mode, kw):
    """one bf16 row at V = 8032 on 16 384 rows, own draw per row: no token outside select_ref's kept set, and the counts
    against select_ref's probabilities (bins merged to an expected count >= 5) pass chi-square at 1 - 1e-4"""
    N, V = 16384, 8032
    inp = _inp(N, V, mode, **kw)
    tok = run_select(inp, uniforms=False, seed=77, offset=5)['token']
    one = {**inp, 'logits': inp['logits'][:1], 'u': torch.zeros(1, device='cuda')}
    ref = select_ref(one['logits'], mode, u=one['u'], pad=1, **kw)
    n = int(ref['n_kept'][0])
    kept = ref['order'][0, :n]
    p = (ref['lp'][0, kept].exp() / ref['kept_mass'][0]).cpu()
    counts = torch.bincount(tok, minlength=V)
    assert int(counts[kept].sum()) == N  # nothing outside the kept set
    obs, exp_ = counts[kept].double().cpu(), p * N
    bins_o, bins_e, o_acc, e_acc = [], [], 0.0, 0.0
    for o, e in zip(obs.tolist(), exp_.tolist()):  # descending probability: merge the tail upwards
        o_acc, e_acc = o_acc + o, e_acc + e
        if e_acc >= 5:
            bins_o.append(o_acc), bins_e.append(e_acc)
            o_acc = e_acc = 0.0
    if e_acc > 0 and bins_e:
        bins_o[-1] += o_acc
        bins_e[-1] += e_acc
    chi2 = sum((o - e) ** 2 / e for o, e in zip(bins_o, bins_e))
    df = len(bins_e) - 1
    print(f'{mode}: kept {n}, {len(bins_e)} bins, chi2 {chi2:.1f}, bound {chi2_quantile(df):.1f}')
    assert df >= 1 and chi2 < chi2_quantile(df)


def test_refusals_name_the_argument():
    from pasero_amd.decode import SampleSelect
    x = torch.randn(4, 61, device='cuda')
    sel = SampleSelect(4, 61, 'cuda')
    with pytest.raises(RuntimeError, match='top_k 5 and top_p 0.5 together'):
        sel.run(x, 'topk', top_k=5, top_p=0.5)
    with pytest.raises(RuntimeError, match='top_k 62'):
        sel.run(x, 'topk', top_k=62)
    with pytest.raises(RuntimeError, match='top_p 1'):
        sel.run(x, 'topp', top_p=1.0)
    from pasero_amd import lib
    L = lib.load()
    args = lambda V, B: (x.data_ptr(), V, V, B, 0, None, 0, 0, 1.0, 1.0, None, 0, None, 1, 0, 0, 1.0, None, 0, 0, None, 0,
                         sel.scratch.data_ptr(), sel.scratch.numel(), sel.token.data_ptr(), 1, sel.logprob.data_ptr(),
                         sel.lse.data_ptr(), sel.n_kept.data_ptr(), sel.kept_mass.data_ptr(), sel.u.data_ptr(), None)
    with pytest.raises(RuntimeError, match='V 134217729'):
        lib.check(L.pk_sample_select(*args((1 << 27) + 1, 4)), 'pk_sample_select')
    with pytest.raises(RuntimeError, match='B 65536'):
        lib.check(L.pk_sample_select(*args(61, 65536)), 'pk_sample_select')
