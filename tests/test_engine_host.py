"""Host-side contract of tfdiffeq_amd/engine.py and _native.status_text: no GPU needed."""
import pytest
import torch

from tfdiffeq_amd import _native as N
from tfdiffeq_amd import adjoint as A
from tfdiffeq_amd import discrete as D
from tfdiffeq_amd import engine as E


def test_status_text_speaks_the_reference_s_words_for_max_steps_and_underflow():
    assert N.status_text(N.ST_MAX_STEPS, max_num_steps=3) == 'max_num_steps exceeded (3>=3)'
    assert N.status_text(N.ST_DT_UNDERFLOW, dt=float('nan')) == 'underflow in dt nan'
    for bits in (N.ST_NONFINITE, N.ST_BAD_T, N.ST_SYNC_TIMEOUT):
        assert N.status_text(bits, max_num_steps=3, dt=float('nan')) == N.status_message(bits)
    # without the caller's figures the library's text stands (the per-row adjoint has no step size to report)
    assert N.status_text(N.ST_MAX_STEPS) == N.status_message(N.ST_MAX_STEPS)
    assert N.status_text(N.ST_DT_UNDERFLOW, max_num_steps=3) == N.status_message(N.ST_DT_UNDERFLOW)


class _FakeLib(object):
    """A library whose segment functions return `bits` and record what they were called with."""

    def __init__(self, bits):
        self.bits, self.calls = bits, []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return self.bits
        return call


def _engine(cls, bits, monkeypatch):
    """An engine of `cls` around the fake library: no handle is created, none is destroyed."""
    eng = cls.__new__(cls)
    eng.lib, eng.h, eng.device = _FakeLib(bits), 1, torch.device('cpu')
    eng.desc, eng.stats = N.AdjointDesc(), N.Stats()
    eng.desc.max_num_steps, eng.stats.dt = 3, float('nan')
    monkeypatch.setattr(N, 'stream_ptr', lambda device: None)
    monkeypatch.setattr(torch.cuda, 'device', lambda device: _NoDevice())
    return eng


class _NoDevice(object):
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


@pytest.mark.parametrize('cls', [A._FusedAdjointEngine, A._LinearAdjointEngine])
def test_an_adjoint_engine_s_run_raises_by_status(cls, monkeypatch):
    eng = _engine(cls, 0, monkeypatch)
    assert eng._run('segment', (1.5, None), 'value') == 'value'
    name, args = eng.lib.calls[0]
    assert name == 'segment' and args[0] == 1 and args[1:3] == (1.5, None) and len(args) == 5        # handle, args, stats, stream
    assert eng._run('dynamics', (2.5,), 'value', stats=False) == 'value' and len(eng.lib.calls[1][1]) == 3   # handle, args, stream
    for bits in (N.ST_SYNC_TIMEOUT, N.ST_SYNC_TIMEOUT | N.ST_MAX_STEPS):
        eng.lib.bits = bits
        with pytest.raises(A.HandoffTimeout) as info:
            eng._run('segment', (), None)
        assert str(info.value) == N.status_message(bits)
    for bits, text in ((N.ST_MAX_STEPS, 'max_num_steps exceeded (3>=3)'), (N.ST_DT_UNDERFLOW, 'underflow in dt nan'),
                       (N.ST_NONFINITE, N.status_message(N.ST_NONFINITE))):
        eng.lib.bits = bits
        with pytest.raises(AssertionError) as info:
            eng._run('segment', (), None)
        assert str(info.value) == text and not isinstance(info.value, A.HandoffTimeout)
    eng.h = None                                             # (nothing to destroy)


def test_the_old_names_are_the_shared_module_s_objects():
    assert A.HandoffTimeout is E.HandoffTimeout
    assert D._SweepEngine is E._SweepEngine
    assert D._cached is E._cached
    assert issubclass(A._FusedAdjointEngine, E._SweepEngine) and issubclass(A._LinearAdjointEngine, E._SweepEngine)
