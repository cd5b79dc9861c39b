"""CPU tests of the few-rows mixture-of-experts entry points (csrc/moe_rows.hip, pk_decoder_step_moe) and of the switch of
pasero_amd.decode: the route table, the scratch sizes, the argument checks that come before any launch, `moe_native()`."""
import ctypes
import os
import subprocess
import sys
import types

import pytest

F32, BF16, F16 = 0, 1, 2
ROWS_MAX = 1024  # PK_MOE_ROWS_MAX


@pytest.fixture(scope='module')
def L():
    from pasero_amd import lib
    return lib.load()


@pytest.fixture(scope='module')
def a():
    buf = ctypes.create_string_buffer((1 << 16) + 256)   # host memory: every call below must fail before it would be touched
    yield (ctypes.addressof(buf) + 255) // 256 * 256


def _err(L):
    return L.pk_last_error().decode()


def test_initial_threshold_and_set_query(L):
    first = L.pk_moerows_few_max(-1)
    assert first == int(os.environ.get('PK_MOE_ROWS_FEW_MAX', 256))
    try:
        assert L.pk_moerows_few_max(7) == first
        assert L.pk_moerows_few_max(-1) == 7 and L.pk_moerows_few_max(-5) == 7   # negative: only asks
        assert L.pk_moerows_few_max(0) == 7 and L.pk_moerows_few_max(-1) == 0
    finally:
        L.pk_moerows_few_max(first)


def test_few_route_table(L):
    first = L.pk_moerows_few_max(-1)
    try:
        for threshold in (256, 0, 16, 5000):
            L.pk_moerows_few_max(threshold)
            for dtype in (F32, BF16, F16):
                for rows in (1, 16, 17, 256, 257, 1024, 1025):
                    for D, F in ((64, 64), (128, 192), (96, 128), (128, 96), (72, 64), (2048, 8192)):
                        want = dtype != F32 and rows <= min(threshold, ROWS_MAX) and D % 64 == 0 and F % 64 == 0
                        assert L.pk_moerows_few(rows, 4, D, F, dtype) == int(want), (threshold, dtype, rows, D, F)
        L.pk_moerows_few_max(256)
        for bad in ((0, 4, 64, 64, BF16), (8, 1, 64, 64, BF16), (8, 257, 64, 64, BF16), (8, 4, 60, 64, BF16), (8, 4, 64, 64, 7)):
            assert L.pk_moerows_few(*bad) == 0, bad
    finally:
        L.pk_moerows_few_max(first)


def test_scratch_is_positive_and_monotone(L):
    for dtype in (F32, BF16, F16):
        for E, D, F in ((2, 64, 64), (4, 128, 128), (7, 192, 320), (256, 64, 64), (128, 2048, 8192), (4, 72, 40)):
            sizes = [L.pk_moerows_scratch(rows, E, D, F, dtype) for rows in (1, 2, 16, 17, 256, 257, 1024, 1025, 4096)]
            assert all(s > 0 for s in sizes) and all(x <= y for x, y in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
            # the slot-ordered intermediates alone: 2 rows of F and 2 rows of D elements per row
            assert sizes[2] >= 16 * 2 * (D + F) * (4 if dtype == F32 else 2)
    for bad in ((0, 4, 64, 64, BF16), (-3, 4, 64, 64, BF16), (8, 1, 64, 64, BF16), (8, 257, 64, 64, BF16), (8, 4, 60, 64, BF16),
                (8, 4, 64, 12, F32), (8, 4, 64, 64, 3), (1 << 29, 4, 64, 64, BF16)):
        assert L.pk_moerows_scratch(*bad) == 0, bad


def test_every_refusal_comes_before_a_launch(L, a):
    need = L.pk_moerows_scratch(8, 4, 64, 64, BF16)
    assert 0 < need <= (1 << 15)
    x, y, scr = a, a + 4096, a + 8192

    def rows(x=x, y=y, gate=a, w1=a, w2=a, rows=8, E=4, D=64, F=64, act=1, dtype=BF16, scratch=scr, nbytes=1 << 15):
        return L.pk_moerows(x, y, gate, w1, None, w2, None, rows, E, D, F, act, dtype, scratch, nbytes, None)
    for kw, word in ((dict(x=None), 'null'), (dict(y=None), 'null'), (dict(gate=None), 'null'), (dict(w1=None), 'null'),
                     (dict(w2=None), 'null'), (dict(E=1), 'expert count'), (dict(E=257), 'expert count'), (dict(rows=0), 'row count'),
                     (dict(rows=-2), 'row count'), (dict(D=60), 'multiples of 8'), (dict(F=36), 'multiples of 8'),
                     (dict(act=9), 'activation'), (dict(dtype=5), 'dtype'), (dict(scratch=None), 'scratch'),
                     (dict(nbytes=need - 1), 'scratch'), (dict(rows=64, y=x + 16384, nbytes=need), 'scratch'), (dict(y=x), 'overlaps'),
                     (dict(y=x + 512), 'overlaps'), (dict(x=x + 1024 - 16, y=x), 'overlaps'), (dict(x=x + 2), 'aligned')):
        assert rows(**kw) == -1, kw
        assert _err(L).startswith('pk_moerows:') and word in _err(L), (kw, _err(L))

    def route(logits=a, out=a, rows=8, E=4, dtype=BF16):
        return L.pk_moerows_route(logits, rows, E, dtype, out, out, out, out, out, None)
    for kw, word in ((dict(rows=0), 'rows'), (dict(rows=ROWS_MAX + 1), 'rows'), (dict(E=1), 'expert count'), (dict(E=257), 'expert count'),
                     (dict(logits=None), 'null'), (dict(out=None), 'null'), (dict(dtype=4), 'dtype')):
        assert route(**kw) == -1, kw
        assert _err(L).startswith('pk_moerows_route:') and word in _err(L), (kw, _err(L))


def _plan(n_layers=2, d=128, ffn=128, dtype=BF16):
    from pasero_amd.decode import PkDecoderLayerWeights, PkDecoderPlan
    layers = (PkDecoderLayerWeights * n_layers)()
    plan = PkDecoderPlan()
    plan.n_layers, plan.d, plan.heads, plan.ffn, plan.act, plan.dtype, plan.vocab = n_layers, d, d // 64, ffn, 1, dtype, 61
    plan.layers = ctypes.cast(layers, ctypes.POINTER(PkDecoderLayerWeights))
    return plan, layers


def test_step_scratch_and_refusals(L, a):
    from pasero_amd.decode import PkMoeLayer
    plan, keep = _plan()
    for B in (1, 5, 80):
        base = L.pk_decoder_step_scratch_ex(ctypes.byref(plan), B, None)
        assert base > 0 and L.pk_decoder_step_scratch_moe(ctypes.byref(plan), B, None, None) == base
        moe = (PkMoeLayer * 2)()
        assert L.pk_decoder_step_scratch_moe(ctypes.byref(plan), B, None, moe) == base   # E == 0 everywhere: dense layers
        moe[1].E, moe[1].F = 4, 128
        one = L.pk_decoder_step_scratch_moe(ctypes.byref(plan), B, None, moe)
        assert one - base >= L.pk_moerows_scratch(B, 4, 128, 128, BF16) > 0
        moe[0].E, moe[0].F = 16, 256   # the largest among the layers, not the sum
        both = L.pk_decoder_step_scratch_moe(ctypes.byref(plan), B, None, moe)
        assert both - base >= L.pk_moerows_scratch(B, 16, 128, 256, BF16) and both - base < one - base + L.pk_moerows_scratch(B, 16, 128, 256, BF16)
    tabs = (ctypes.c_void_p * 2)(a, a)

    def step(moe):
        return L.pk_decoder_step_moe(ctypes.byref(plan), a, 4, 1, 1, tabs, tabs, 64, tabs, None, 7, a, 256, a, 64, None, moe, None)
    moe = (PkMoeLayer * 2)()
    moe[1].E, moe[1].F = 4, 128   # no gate, no tables
    assert step(moe) == -1 and 'mixture of layer 1 is incomplete' in _err(L)
    moe[1].gate_w = moe[1].w1 = moe[1].w2 = a
    moe[1].E = 300
    assert step(moe) == -1 and 'mixture of layer 1' in _err(L) and 'sizes' in _err(L)
    moe[1].E, moe[1].F = 4, 100
    assert step(moe) == -1 and 'mixture of layer 1' in _err(L)
    moe[1].F = 128   # complete now: the next refusal is the scratch, still before any launch
    assert step(moe) == -1 and 'scratch too small' in _err(L)


def test_moe_native_sets_and_asks():
    from pasero_amd import decode
    first = decode.moe_native()
    try:
        assert decode.moe_native(True) == first and decode.moe_native() is True
        assert decode.moe_native(None) is True
        assert decode.moe_native(False) is True and decode.moe_native() is False
    finally:
        decode.moe_native(first)
    assert decode.moe_native() == first


def test_environment_default_of_the_switch():
    """PASERO_MOE_NATIVE_DECODE is read when pasero_amd.decode is imported: a fresh interpreter per value"""
    from conftest import ROOT
    code = 'import pasero_amd.decode as d; print(int(d.moe_native()))'
    for value, want in ((None, '0'), ('', '0'), ('0', '0'), ('1', '1')):
        env = {k: v for k, v in os.environ.items() if k != 'PASERO_MOE_NATIVE_DECODE'}
        if value is not None:
            env['PASERO_MOE_NATIVE_DECODE'] = value
        out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
        assert out.stdout.strip().splitlines()[-1] == want, (value, out.stdout, out.stderr)


def _cpu_decoder(interval):
    from moe_utils import moe_model
    cfg, model = moe_model(decoder_expert_interval=interval)
    return model.eval().decoder


def test_switch_off_never_reaches_the_mixture_branch(monkeypatch):
    """build_plan over a stand-in that passes the device check (the layers are the real ones, on the CPU: nothing is launched)"""
    from pasero_amd import decode
    real = _cpu_decoder(1)
    stand_in = types.SimpleNamespace(cfg=real.cfg, training=False, layers=real.layers, embed_positions=real.embed_positions,
                                     embed_tokens=types.SimpleNamespace(weight=types.SimpleNamespace(is_cuda=True), frozen_embedding=None))
    reached = []
    monkeypatch.setattr(decode, '_moe_spec', lambda layer, D: reached.append(layer) or None)
    first = decode.moe_native(False)
    try:
        assert decode.build_plan(stand_in) is None and not reached
        decode.moe_native(True)
        assert decode.build_plan(stand_in) is None and reached == [real.layers[0]]
    finally:
        decode.moe_native(first)


def test_plan_key_carries_the_switch_only_for_mixture_decoders():
    from pasero_amd import decode
    from pasero_amd.config import DistributedConfig, SyntheticTask, TransformerConfig
    from pasero_amd.transformer import Transformer
    mixture = _cpu_decoder(2)
    stock = Transformer(TransformerConfig(embed_dim=128, encoder_ffn_dim=128, decoder_ffn_dim=128, encoder_attention_heads=2,
                                          decoder_attention_heads=2, encoder_layers=1, decoder_layers=1, dropout=0.0),
                        DistributedConfig(), SyntheticTask(61)).eval().decoder
    first = decode.moe_native(False)
    try:
        keys = {}
        for on in (False, True, False):
            decode.moe_native(on)
            assert decode.get_plan(mixture) is None and decode.get_plan(stock) is None   # (CPU parameters: no plan either way)
            keys[on] = decode._plans[mixture][0]
            assert keys[on][-1] == ('moe_native', on)
            assert len(decode._plans[stock][0]) == 2   # decoders without mixture layers keep the key they had
        assert keys[True] != keys[False] and keys[True][:-1] == keys[False][:-1]
    finally:
        decode.moe_native(first)
