"""Host-side tests of the time-dependent fused discrete sweep: the C entry point that carries the flag, the ctypes mirror, the engine
cache key and the refusals that need no device.  No GPU needed."""
import ctypes as C
import os

from tfdiffeq_amd import _native as N
from tfdiffeq_amd import discrete as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_exports_the_creation_entry_point_with_the_flag():
    names = ('mi_ode_discrete_create_td',)
    header = open(os.path.join(ROOT, 'include', 'mi_ode.h')).read()
    for name in names:
        assert name in N.EXPORTED_SYMBOLS and name + '(' in header
    lib = N.load()                                           # (binds every prototype: a missing export raises here)
    for name in names:
        assert hasattr(lib, name)
    # the descriptor itself is what it was: existing callers of mi_ode_discrete_create see no change
    assert lib.mi_ode_sizeof(9) == C.sizeof(N.DiscreteDesc)
    assert [f[0] for f in N.DiscreteDesc._fields_] == ['batch', 'dim', 'hidden', 'tableau', 'n_points', 'chunk_tiles']
    assert lib.mi_ode_discrete_create_td.argtypes[1] is C.c_int32 and len(lib.mi_ode_discrete_create_td.argtypes) == 3
    # without a device the entry points refuse with an error code, they do not crash
    h = C.c_void_p()
    assert lib.mi_ode_discrete_create_td(None, 1, C.byref(h)) == N.E_INVALID
    d = N.DiscreteDesc()
    d.batch, d.dim, d.hidden, d.n_points = 8, 16, 16, 3
    assert lib.mi_ode_discrete_create_td(C.byref(d), 2, C.byref(h)) == N.E_INVALID and not h.value
    assert b'time_dependent' in lib.mi_ode_last_error()
    d.dim = 200                                              # outside the tile box, whatever the flag
    assert lib.mi_ode_discrete_create_td(C.byref(d), 1, C.byref(h)) == N.E_INVALID and not h.value


def test_the_engine_cache_key_carries_the_flag(monkeypatch):
    made = []

    class Engine(object):
        def __init__(self, *args):
            made.append(args)

        def close(self):
            pass
    monkeypatch.setattr(D, '_FusedDiscreteEngine', Engine)
    monkeypatch.setattr(D, '_ENGINES', {})
    a = D._cached_engine(33, 3, 5, 'rk4', 5, 'cuda:0', 2, True)
    b = D._cached_engine(33, 3, 5, 'rk4', 5, 'cuda:0', 2, False)
    c = D._cached_engine(33, 3, 5, 'rk4', 5, 'cuda:0', 2)    # the flag defaults to the time-independent network
    assert a is not b and b is c and len(made) == 2
    assert made[0] == (33, 3, 5, 'rk4', 5, 'cuda:0', 2, True) and made[1][-1] is False
    for key in D._ENGINES:                                   # shape first, the chunk last: what the callers that search the cache index
        assert key[:4] == (33, 3, 5, 'rk4') and key[-1] == 2 and isinstance(key[-2], bool)
    assert sorted(k[-2] for k in D._ENGINES) == [False, True]
