"""What the Python owners of a one-launch native handle share: the engine base class, the size-4 cache rule and the exception of a
hand-off that timed out.  adjoint.py (the adaptive fused and linear adjoints) and discrete.py (the four discrete sweeps) build on it."""
import ctypes as C

import torch

from . import _native as N


class HandoffTimeout(RuntimeError):
    """A one-launch kernel's in-kernel grid hand-off timed out (the GPU is shared with another persistent kernel).  Nothing
    was committed: the caller may take the generic path.  Every other native failure propagates."""


class _SweepEngine(object):
    """Owns one handle of a one-launch engine: the library, the device, the descriptor, the stats of the last call.  A subclass names its
    create and destroy symbols, fills its descriptor and says what a call passes."""
    _create = _destroy = None

    def _open(self, device, desc, tableau, c_mid, *create_args):
        """The handle of `desc` (its tableau: `tableau` with the dense-output weights `c_mid`, or None) on `device`; create_args go between
        the descriptor and the handle."""
        from .solvers import _fill_tableau
        self.lib = N.load()
        self.device = torch.device(device)
        _fill_tableau(desc.tableau, tableau, c_mid)
        self.desc = desc
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(getattr(self.lib, self._create)(C.byref(desc), *(create_args + (C.byref(h),))), self._create)
        self.h = h
        self.stats = N.Stats()

    def close(self):
        if getattr(self, 'h', None):
            getattr(self.lib, self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _run(self, name, args, value, stats=True):
        """The call `name` of this handle with `args`, the stats (stats=False: the call takes none) and the stream: `value`, or
        HandoffTimeout / AssertionError - what the reference's solver raises (dopri5.py:85-100) - for the status it returned."""
        tail = ((C.byref(self.stats),) if stats else ()) + (N.stream_ptr(self.device),)
        with torch.cuda.device(self.device):
            rc = N.check(getattr(self.lib, name)(self.h, *(tuple(args) + tail)), name)
        if rc & N.ST_SYNC_TIMEOUT:
            raise HandoffTimeout(N.status_message(rc))
        if rc != 0:
            raise AssertionError(N.status_text(rc, getattr(self.desc, 'max_num_steps', None), self.stats.dt))
        return value


def _cached(cache, key, make, close_on_evict):
    """The engine of `key` in `cache`, four cached at most, the oldest evicted - only after a successful make(): a refusal must not cost
    live engines.  close_on_evict: the evicted engine is closed; otherwise only the cache's reference is dropped."""
    eng = cache.get(key)
    if eng is None:
        eng = make()
        while len(cache) >= 4:
            old = cache.pop(next(iter(cache)))
            if close_on_evict:
                old.close()
        cache[key] = eng
    return eng
