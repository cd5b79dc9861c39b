"""CPU tests of the LayerNorm entry points of the C ABI (csrc/layernorm.hip): every argument check answers -1 with a message
naming the entry point before anything is launched (the buffers are host memory: a launch would not get as far as failing
politely), rows == 0 is a no-op, and pk_residual_ln_bwd_workspace is min(ceil(rows / 4), cap) [2][d] fp32 slabs on both sides
of each cap (2048 workgroups from the forward grid, 1024 for d <= 512 and 512 beyond in backward)."""
import ctypes

import pytest

from ln_cases import bwd_workspace_bytes

F32, BF16, F16 = 0, 1, 2
PK_LN_GROUP_MAX = 4


class PkLnParamGrad(ctypes.Structure):
    """include/pasero_hip.h"""
    _fields_ = [('workspace', ctypes.c_void_p), ('dgamma', ctypes.c_void_p), ('dbeta', ctypes.c_void_p)]


@pytest.fixture(scope='module')
def L():
    from pasero_amd import lib
    return lib.load()


@pytest.fixture(scope='module')
def a():
    buf = ctypes.create_string_buffer(1 << 12)   # host memory: every call below must fail before it would be touched
    yield (ctypes.addressof(buf) + 255) // 256 * 256


def _err(L):
    return L.pk_last_error().decode()


def test_workspace_sizes(L):
    for d in (8, 64, 512, 520, 1024, 4096):
        cap = 1024 if d <= 512 else 512
        for rows in (1, 3, 4, 5, 4 * cap - 3, 4 * cap, 4 * cap + 1, 4 * cap + 5, 8192, 8197, 1 << 20):
            blocks = min(-(-rows // 4), cap)
            assert L.pk_residual_ln_bwd_workspace(rows, d) == blocks * 2 * d * 4 == bwd_workspace_bytes(rows, d), (rows, d)
    # the narrow cap lies above the wide one: between them the two differ
    assert L.pk_residual_ln_bwd_workspace(4096, 512) == 1024 * 2 * 512 * 4
    assert L.pk_residual_ln_bwd_workspace(4096, 520) == 512 * 2 * 520 * 4


def test_forward_argument_checks(L, a):
    def fwd(x=a, res=None, gamma=a, beta=a, z=a, y=a, mean=a, rstd=a, rows=2, d=64, p=0.0, dtype=BF16):
        return L.pk_residual_ln_fwd(x, res, gamma, beta, z, y, mean, rstd, rows, d, 1e-5, p, 1, 2, dtype, None)
    for kw, word in ((dict(x=None), 'x is null'), (dict(y=None), 'y/rstd missing'), (dict(rstd=None), 'y/rstd missing'),
                     (dict(mean=None), 'RMSNorm'), (dict(gamma=None, beta=None, z=None), 'nothing to compute'),
                     (dict(p=-0.1), 'bad dropout'), (dict(p=1.0), 'bad dropout'), (dict(p=1.5), 'bad dropout'),
                     (dict(dtype=3), 'dtype'), (dict(dtype=-1), 'dtype'),
                     (dict(d=68), 'unsupported'), (dict(d=68, dtype=F16), 'unsupported'), (dict(d=66, dtype=F32), 'unsupported'),
                     (dict(d=8200), 'unsupported'), (dict(d=8200, dtype=F16), 'unsupported'), (dict(d=4100, dtype=F32), 'unsupported')):
        assert fwd(**kw) == -1, kw
        assert _err(L).startswith('pk_residual_ln_fwd:') and word in _err(L), (kw, _err(L))
    assert fwd(rows=0) == 0 and fwd(rows=0, d=3, x=None) == 0


def test_backward_argument_checks(L, a):
    need = L.pk_residual_ln_bwd_workspace(2, 64)

    def bwd(dy=a, extra=None, z=a, gamma=a, mean=a, rstd=a, dres=a, dx=None, dgamma=a, dbeta=a, ws=a, nbytes=need, rows=2, d=64,
            p=0.0, dtype=BF16):
        return L.pk_residual_ln_bwd(dy, extra, z, gamma, mean, rstd, dres, dx, dgamma, dbeta, ws, nbytes, rows, d, p, 1, 2, dtype, None)
    for kw, word in ((dict(dy=None), 'LN inputs missing'), (dict(z=None), 'LN inputs missing'), (dict(rstd=None), 'LN inputs missing'),
                     (dict(mean=None), 'RMSNorm'), (dict(gamma=None), 'nothing to compute'),
                     (dict(p=-0.5), 'bad dropout'), (dict(p=1.0), 'bad dropout'), (dict(dtype=5), 'dtype'),
                     (dict(d=68), 'unsupported'), (dict(d=66, dtype=F32), 'unsupported'),
                     (dict(d=4104, nbytes=1 << 30), 'unsupported'), (dict(d=2052, dtype=F32, nbytes=1 << 30), 'unsupported'),
                     (dict(nbytes=need - 1), 'workspace too small'), (dict(ws=None), 'workspace too small'),
                     (dict(dbeta=None, nbytes=need - 1), 'workspace too small'),
                     (dict(rows=4097, d=64, nbytes=1024 * 2 * 64 * 4 - 1), 'workspace too small')):
        assert bwd(**kw) == -1, kw
        assert _err(L).startswith('pk_residual_ln_bwd:') and word in _err(L), (kw, _err(L))
    assert bwd(rows=0) == 0


def test_deferred_argument_checks(L, a):
    need = L.pk_residual_ln_bwd_workspace(2, 64)

    def part(dy=a, z=a, gamma=a, rstd=a, ws=a, nbytes=need, rows=2, d=64, p=0.0, dtype=F16):
        return L.pk_residual_ln_bwd_partials(dy, None, z, gamma, a, rstd, a, None, ws, nbytes, rows, d, p, 1, 2, dtype, None)
    for kw, word, who in ((dict(dy=None), 'LN inputs missing', 'pk_residual_ln_bwd_partials:'),
                          (dict(z=None), 'LN inputs missing', 'pk_residual_ln_bwd_partials:'),
                          (dict(gamma=None), 'LN inputs missing', 'pk_residual_ln_bwd_partials:'),
                          (dict(rstd=None), 'LN inputs missing', 'pk_residual_ln_bwd_partials:'),
                          (dict(ws=None), 'LN inputs missing', 'pk_residual_ln_bwd_partials:'),
                          (dict(p=1.0), 'bad dropout', 'pk_residual_ln_bwd_partials:'),
                          (dict(dtype=3), 'dtype', 'pk_residual_ln_bwd_partials:'),
                          # (the shape and workspace checks are the shared launch path's and carry its name)
                          (dict(d=68), 'unsupported', 'pk_residual_ln_bwd'), (dict(d=4104, nbytes=1 << 30), 'unsupported', 'pk_residual_ln_bwd'),
                          (dict(nbytes=need - 1), 'workspace too small', 'pk_residual_ln_bwd')):
        assert part(**kw) == -1, kw
        assert _err(L).startswith(who) and word in _err(L), (kw, _err(L))
    assert part(rows=0) == 0

    items = (PkLnParamGrad * 5)(*[PkLnParamGrad(a, a, a) for _ in range(5)])
    for n in (0, 5, -1):
        assert L.pk_ln_param_grads(items, n, 2, 64, BF16, None) == -1
        assert _err(L).startswith('pk_ln_param_grads:') and 'items' in _err(L)
    assert L.pk_ln_param_grads(None, 1, 2, 64, BF16, None) == -1 and _err(L).startswith('pk_ln_param_grads:')
    items[2].workspace = None
    assert L.pk_ln_param_grads(items, 3, 2, 64, BF16, None) == -1
    assert _err(L).startswith('pk_ln_param_grads:') and 'item 2 has no workspace' in _err(L)
    assert L.pk_ln_param_grads(items, 2, 0, 64, BF16, None) == 0


def test_header_declares_the_struct_the_tests_build():
    import os
    import re
    from conftest import ROOT
    header = open(os.path.join(ROOT, 'include', 'pasero_hip.h')).read()
    assert int(re.search(r'#define PK_LN_GROUP_MAX (\d+)', header).group(1)) == PK_LN_GROUP_MAX
    body = re.search(r'typedef struct PkLnParamGrad \{(.*?)\} PkLnParamGrad;', header, re.S).group(1)
    assert re.findall(r'(\w+);', body) == [n for n, _ in PkLnParamGrad._fields_]
