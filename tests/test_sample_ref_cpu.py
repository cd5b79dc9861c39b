"""tests/sample_ref.py (the plain-torch comparator of the native sampling search) against the reference's own searches:
fed the last-position logits the reference's decoder returned at every call of every recorded search
(tests/golden/sampling_search.npz) and the recorded uniforms, it must yield the recorded tokens step by step."""
import numpy as np
import torch

from conftest import load_golden, golden_cfg
from sample_ref import sample_ref, select_ref


def load_case(g, name):
    p = name + ':'
    return {k[len(p):]: g[k] for k in g.files if k.startswith(p)}


def options(c):
    stop = [c['stop_sequence'].tolist()] if c['stop_sequence'].size else []
    return dict(sampling_temperature=float(c['sampling_temperature']), sampling_topk=int(c['sampling_topk']),
                sampling_topp=float(c['sampling_topp']), repeat_penalty=float(c['repeat_penalty']),
                blacklist=[int(x) for x in c['blacklist']], stop_sequences=stop)


def test_sample_ref_replays_every_recorded_search():
    g = load_golden('sampling_search')
    names = [str(n) for n in g['cases']]
    assert len(names) >= 7
    for name in names:
        c = load_case(g, name)
        cfg = golden_cfg(c)
        calls = []

        def step_fn(feed):
            i = len(calls)
            assert i < len(c['logits']), 'more decoder calls than the reference made'
            calls.append(feed.size(1))
            return torch.from_numpy(c['logits'][i]).unsqueeze(1)  # last position only: tokens do not need the others
        stats = {}
        outs = sample_ref(step_fn, torch.from_numpy(c['prompt']), int(c['max_output_len']), cfg.decoder_max_len,
                          cfg.padding_idx, cfg.eos_idx, uniforms=torch.from_numpy(c['uniforms']), stats=stats, **options(c))
        assert stats['rows'] == [int(r) for r in c['rows']], name
        assert [o['tokens'].size(1) for o in outs] == [int(w) for w in c['widths']], name
        np.testing.assert_array_equal(torch.cat([o['tokens'] for o in outs], dim=1).numpy(), c['tokens'], err_msg=name)
        # the margins the GPU test relies on were computed by this very function
        for k in ('draw_margin', 'boundary_margin'):
            assert float(c[k]) >= 1e-3 and abs(min(float(stats[k].min()), 1e30) - min(float(c[k]), 1e30)) <= 1e-9, (name, k)
        assert float(c['greedy_gap']) >= 1e-3 * float(c['max_logit'])


def test_select_ref_skip_cap_of_the_gpu_test_seeds():
    """the GPU kernel test skips the kept-set check on rows whose fp64 boundary margin is within tau and caps the skipped
    share at 5 % per case: computed here from the comparator alone, on the same seeded inputs (those small enough)"""
    from sample_cases import SAMPLE_CASES, make_sample_case, reference_tau, boundary_clear
    seen = 0
    for case in SAMPLE_CASES:
        if case['B'] * case['V'] > 2_100_000:
            continue  # the large cases are checked on the GPU box, with the same functions
        inp = make_sample_case(case, 'cpu')
        ref = select_ref(inp['logits'], inp['mode'], u=inp['u'], pad=inp['pad'], **inp['kw'])
        tau = reference_tau(ref)
        assert float((~boundary_clear(ref, tau)).float().mean()) <= 0.05, case
        seen += 1
    assert seen >= 100
