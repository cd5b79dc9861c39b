"""CPU tests of the mixture-of-experts entry points of the C ABI (csrc/moe.hip): the argument checks that come before any
launch, and the gate's scratch size."""
import ctypes

import pytest

F32, BF16 = 0, 1


@pytest.fixture(scope='module')
def L():
    from pasero_amd import lib
    return lib.load()


@pytest.fixture(scope='module')
def a():
    buf = ctypes.create_string_buffer(1 << 12)   # host memory: every call below must fail before it would be touched
    yield ctypes.addressof(buf)


def _err(L):
    return L.pk_last_error().decode()


def test_gate_scratch_is_monotone(L):
    sizes = [[L.pk_moe_gate_scratch(S, E) for E in (2, 3, 4, 128, 256)] for S in (1, 63, 64, 65, 257, 8192, 32768)]
    assert all(v > 0 for row in sizes for v in row)
    assert all(a <= b for row in sizes for a, b in zip(row, row[1:]))
    assert all(a <= b for r0, r1 in zip(sizes, sizes[1:]) for a, b in zip(r0, r1))
    assert sizes[4][0] > sizes[0][0] and sizes[0][4] > sizes[0][0]
    assert L.pk_moe_gate_scratch(64, 1) == 0 and L.pk_moe_gate_scratch(64, 257) == 0 and L.pk_moe_gate_scratch(0, 4) == 0


def test_gate_argument_checks(L, a):
    def gate(S=8, E=4, logits=a, tables=a, stats=a, scratch=a, nbytes=1 << 12):
        return L.pk_moe_gate(logits, None, S, E, a, a, a, stats, stats, stats, stats, tables, tables, tables, scratch, nbytes, None)
    for kw, word in ((dict(E=1), 'expert count'), (dict(E=257), 'expert count'), (dict(S=0), 'token count'),
                     (dict(logits=None), 'null'), (dict(tables=None), 'null routing table'), (dict(stats=None), 'null'),
                     (dict(scratch=None), 'scratch'), (dict(nbytes=L.pk_moe_gate_scratch(8, 4) - 1), 'scratch'),
                     (dict(S=600, nbytes=L.pk_moe_gate_scratch(512, 4)), 'scratch')):
        assert gate(**kw) == -1, kw
        assert _err(L).startswith('pk_moe_gate:') and word in _err(L), (kw, _err(L))
    for E in (1, 257):
        assert L.pk_moe_gate_bwd(a, a, None, 1.0, a, a, a, 8, E, None) == -1 and 'expert count' in _err(L)
    assert L.pk_moe_gate_bwd(a, a, None, 1.0, None, a, a, 8, 4, None) == -1 and 'null' in _err(L)


def test_row_kernels_argument_checks(L, a):
    assert L.pk_moe_gather(a, a, a, a, a, None, 8, 4, 12, BF16, None) == -1 and 'multiple of 8' in _err(L)
    assert L.pk_moe_gather(a, a, None, a, a, None, 8, 4, 16, BF16, None) == -1 and 'null' in _err(L)
    assert L.pk_moe_gather(a, a, a, a, None, a, 8, 4, 16, BF16, None) == -1 and 'slot_of' in _err(L)
    assert L.pk_moe_gather(a, a, a, a, a, None, 8, 300, 16, BF16, None) == -1 and 'expert count' in _err(L)
    assert L.pk_moe_gather(a, a, a, a, a, None, 8, 4, 16, 9, None) == -1 and 'dtype' in _err(L)
    assert L.pk_moe_combine(a, a, None, a, 8, 16, BF16, None) == -1 and 'null' in _err(L)
    assert L.pk_moe_combine(a, a, a, a, 8, 20, F32, None) == -1 and 'multiple of 8' in _err(L)
    assert L.pk_moe_dot(a, a, a, None, 8, 16, F32, None) == -1 and 'null' in _err(L)
    assert L.pk_moe_dot(a, a, a, a, 8, 4, F32, None) == -1 and 'multiple of 8' in _err(L)


def test_grouped_gemm_argument_checks(L, a):
    def gemm(W=a, offsets=a, rows=16, E=4, N=128, K=128, mode=0, act=1, dtype=BF16, aux=None, bias=None):
        return L.pk_moe_gemm(a, W, bias, a, aux, None, offsets, rows, E, N, K, 0, act, mode, dtype, None)
    for kw, word in ((dict(E=1), 'expert count'), (dict(E=257), 'expert count'), (dict(N=132), 'multiples of 8'),
                     (dict(K=100), 'multiples of 8'), (dict(W=None), 'null'), (dict(offsets=None), 'null'), (dict(rows=0), 'slot rows'),
                     (dict(mode=1), 'mode'), (dict(mode=2), 'mode 2'), (dict(mode=2, aux=a, bias=a), 'mode 2'), (dict(act=7), 'activation'),
                     (dict(dtype=5), 'dtype')):
        assert gemm(**kw) == -1, kw
        assert _err(L).startswith('pk_moe_gemm:') and word in _err(L), (kw, _err(L))

    def wgrad(dW=a, db=a, offsets=a, E=4, M=128, N=128, dtype=BF16, X=a):
        return L.pk_moe_gemm_wgrad(a, X, dW, db, offsets, 16, E, M, N, dtype, None)
    for kw, word in ((dict(E=0), 'expert count'), (dict(E=1000), 'expert count'), (dict(M=4), 'multiples of 8'),
                     (dict(N=130), 'multiples of 8'), (dict(dW=None, db=None), 'null'), (dict(offsets=None), 'null'),
                     (dict(X=None), 'null'), (dict(dtype=3), 'dtype')):
        assert wgrad(**kw) == -1, kw
        assert _err(L).startswith('pk_moe_gemm_wgrad:') and word in _err(L), (kw, _err(L))


def test_header_exports_and_bindings_agree():
    import os
    import re
    from conftest import ROOT
    from pasero_amd import lib
    header = open(os.path.join(ROOT, 'include', 'pasero_hip.h')).read()
    declared = set(re.findall(r'\b(pk_moe_[a-z0-9_]+)\s*\(', header))
    assert declared == {n for n in lib.SIGNATURES if n.startswith('pk_moe_')} and len(declared) == 9
    L = lib.load()
    assert all(hasattr(L, n) for n in declared)
    assert L.pk_moe_use_grouped(-1) in (0, 1)
