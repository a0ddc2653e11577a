"""The plugin kinds (tfdiffeq_amd._plugin_build.KINDS) without a GPU: every derived kind's source, the refusal of a unit of another kind,
the getter names a loaded library gets declared, what the three plugin right-hand sides expose, and the one memo per instance."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import discrete_lowered_cases as DC                        # noqa: E402
import per_trajectory_cases as PC                          # noqa: E402
from tfdiffeq_amd import _plugin_build as PB, lower, rhs   # noqa: E402

F64 = torch.float64
DERIVED = sorted(k.name for k in PB.KINDS.values() if k.base is not None)
STRICT = sorted(k.name for k in PB.KINDS.values() if k.base is not None and k.not_base is not None)


def _base_sources():
    """One translation unit of every kind that is generated as it is (base None)."""
    f, _params, y0 = DC.scalars('cpu', F64)
    tr = lower.trace(f, y0)
    return {'row-local': PC.van_der_pol().source(F64), 'coop': rhs.CustomCoop(40, "k = -y[i];").source(F64),
            'discrete': lower.discrete_source(tr), 'rows-adjoint': lower.adjoint_source(tr)}


BASE = _base_sources()


def test_registry_names_every_kind_once_and_every_base_is_a_generated_kind():
    assert sorted(BASE) == sorted(k.name for k in PB.KINDS.values() if k.base is None)
    assert len(PB.KINDS) == 11 and all(name == k.name for name, k in PB.KINDS.items())
    assert len(set(k.macro for k in PB.KINDS.values())) == 11
    for k in PB.KINDS.values():
        assert k.base is None or PB.KINDS[k.base].base is None
        assert os.path.exists(os.path.join(PB.N.CSRC, k.header)) and k.getter.endswith('_plugin_get')
        text = open(os.path.join(PB.N.CSRC, k.header)).read()
        assert '#define %s(RHS) MI_ODE_DEFINE_PLUGIN_GETTER(%s, ' % (k.macro, k.getter) in text, k.name
    for name, src in BASE.items():
        assert PB._source_roots(src) == (PB.KINDS[name].header,) and src.count(PB.KINDS[name].macro + '(') == 1


@pytest.mark.parametrize('kind', DERIVED)
def test_derive_swaps_the_header_and_the_macro_and_nothing_else(kind):
    k = PB.KINDS[kind]
    base = PB.KINDS[k.base]
    src = PB.derive(kind, BASE[k.base])
    assert PB._source_roots(src) == (k.header,)
    assert src.count(k.macro) == 1 and base.macro not in src
    assert src.replace(k.header, base.header).replace(k.macro + '(', base.macro + '(') == BASE[k.base]


@pytest.mark.parametrize('kind', STRICT)
def test_derive_refuses_a_unit_of_another_kind(kind):
    k = PB.KINDS[kind]
    for name, src in BASE.items():
        if name != k.base:
            with pytest.raises(ValueError) as err:
                PB.derive(kind, src)
            assert str(err.value) == k.not_base and k.not_base.startswith('not a %s plugin translation unit: ' % k.base)


def test_the_lenient_kind_is_hyper_alone_and_returns_a_foreign_unit_unchanged():
    assert [k for k in DERIVED if k not in STRICT] == ['hyper']
    assert PB.derive('hyper', BASE['discrete']) == BASE['discrete']
    coop = PB.derive('hyper', BASE['coop'])                          # (the header is shared with the row-local kind: it is swapped)
    assert 'MI_ODE_DEFINE_COOP_PLUGIN(' in coop and 'MI_ODE_DEFINE_HYPER_PLUGIN' not in coop


def test_public_names_delegate_to_derive():
    for fn, kind in ((rhs.hyper_source_of, 'hyper'), (rhs.rows_source_of, 'rows'), (rhs.rows_t_source_of, 'rows-t'),
                     (rhs.fixed_rows_t_source_of, 'fixed-rows-t'), (rhs.hyper_grad_source_of, 'hyper-grad'),
                     (rhs.discrete_t_source_of, 'discrete-t'), (rhs.rows_adjoint_t_source_of, 'rows-adjoint-t')):
        base = BASE[PB.KINDS[kind].base]
        assert fn(base) == PB.derive(kind, base)


def test_a_loaded_library_gets_the_registrys_getters_declared(monkeypatch):
    class Fn(object):
        restype = argtypes = None

    class Lib(object):                                               # every symbol "exists": what gets declared is what was asked for
        def __init__(self, path):
            self.asked = {}

        def __getattr__(self, name):
            return self.asked.setdefault(name, Fn())

    monkeypatch.setattr(PB, 'build', lambda source: '/nowhere/' + source)
    monkeypatch.setattr(PB.C, 'CDLL', Lib)
    monkeypatch.setattr(PB, '_loaded', {})
    lib = PB.build_and_load('x')
    declared = sorted(name for name, fn in lib.asked.items() if fn.restype is PB.C.c_void_p and fn.argtypes == [PB.C.c_int])
    assert declared == sorted(set(k.getter for k in PB.KINDS.values())) and len(declared) == 10
    assert sorted(PB.getter_names()) == declared


def _kind_names(obj):
    return sorted(n for n in dir(obj) if n.endswith(('_source', '_plugin')) and not n.startswith('_') and callable(getattr(obj, n)))


def test_lowered_and_custom_row_local_expose_the_same_kinds_and_coop_the_base_kind_only():
    low = lower.program_for(lower.trace(PC.time_callable, torch.ones(6, 4, dtype=F64))).rhs
    vdp = PC.van_der_pol()
    want = sorted(k.name.replace('-', '_') + s for k in PB.KINDS.values() if k.base == 'row-local' for s in ('_source', '_plugin'))
    assert type(low).__name__ == '_GeneratedRHS' and _kind_names(low) == _kind_names(vdp) == want and len(want) == 8
    coop = rhs.CustomCoop(40, "k = -y[i];")
    assert _kind_names(coop) == [] and callable(coop._plugin) and coop.plugin_kind == 'coop' and vdp.plugin_kind == low.plugin_kind == 'row-local'
    for k in PB.KINDS.values():
        if k.base == 'row-local':
            assert getattr(low, k.name.replace('-', '_') + '_source')(F64) == PB.derive(k.name, low.source(F64))
            assert getattr(vdp, k.name.replace('-', '_') + '_source')(F64) == PB.derive(k.name, vdp.source(F64))


def test_one_memo_per_instance_and_one_cache_behind_it(monkeypatch):
    built = []

    class Lib(object):
        def __getattr__(self, name):
            return lambda code: 0x1000 + len(built)

    def counted(source):
        built.append(source)
        return Lib()
    monkeypatch.setattr(PB, 'build_and_load', counted)
    monkeypatch.setattr(PB, '_tables', {})
    for f in (PC.van_der_pol(), lower.program_for(lower.trace(PC.time_callable, torch.ones(6, 4, dtype=F64))).rhs):
        monkeypatch.setattr(f, '_plugins', {})
        for kind in ('hyper', 'rows', 'rows_t', 'fixed_rows_t'):
            del built[:]
            one = getattr(f, kind + '_plugin')(F64)
            assert getattr(f, kind + '_plugin')(F64) is one and built == [getattr(f, kind + '_source')(F64)]
            assert isinstance(one[0], Lib) and type(one[1]) is int
        del built[:]
        key = f.cache_key(F64, 'cpu')
        assert f.cache_key(F64, 'cpu') == key and built == [f.source(F64)] and key[-1] == f._plugin(F64)[1]
        assert sorted(f._plugins) == sorted((k, F64) for k in ('row-local', 'hyper', 'rows', 'rows-t', 'fixed-rows-t'))
    coop = rhs.CustomCoop(40, "k = -y[i];")
    del built[:]
    assert coop.cache_key(F64, 'cpu') == coop.cache_key(F64, 'cpu') and built == [coop.source(F64)] and list(coop._plugins) == [('coop', F64)]
    # the module-level loaders share the cache behind the instances: the same (kind, source, dtype) is built once, whoever asks
    del built[:]
    src = BASE['discrete']
    assert rhs.discrete_plugin(src, F64) is rhs.discrete_plugin(src, F64) is PB.load('discrete', src, F64) and built == [src]
    assert PB.load('rows', PC.van_der_pol().rows_source(F64), F64) and built == [src]          # (van der Pol's rows plugin: loaded above)


def test_a_null_table_is_an_error_in_the_kinds_own_words(monkeypatch):
    class Lib(object):
        def __getattr__(self, name):
            return lambda code: None
    monkeypatch.setattr(PB, 'build_and_load', lambda source: Lib())
    monkeypatch.setattr(PB, '_tables', {})
    for kind, words in (('row-local', 'plugin exports no table for'), ('coop', 'plugin exports no table for'), ('rows-t', 'rows-t plugin exports no table for'),
                        ('hyper-grad', 'hyper-grad plugin exports no table for'), ('rows-adjoint', 'rows-adjoint plugin exports no table for')):
        with pytest.raises(PB.N.NativeError) as err:
            PB.load(kind, 'x', F64)
        assert str(err.value) == words + ' torch.float64'
    assert PB._tables == {}
