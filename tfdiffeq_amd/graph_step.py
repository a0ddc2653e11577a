"""hipGraph capture of one adaptive Runge-Kutta attempt for an arbitrary Python right-hand side.

The generic path (any callable f over torch ops, plane kernels for the state arithmetic) issues ~60 small launches per
attempt and is bound by the host's launch rate.  Nothing in an attempt depends on host values except t0 and dt, and
those can live in device memory (`mi_ode_lincomb_dev` reads dt when it runs; the stage times are 0-d tensors computed
on the device).  So the attempt is recorded ONCE - the S evaluations of f, the stage combinations, y1, the error
estimate and its norms - and replayed per attempt with new (t0, dt); the host only reads back the 4-double norm record
and runs the controller.  Opt-in (`options={'graph': True}`): f must be capture-safe (static shapes, no host
synchronisation, no data-dependent Python control flow), which holds for the usual tensor-expression right-hand sides.
"""
import collections

import torch

from .misc import _error_norms
from .rk_common import _runge_kutta_step


class GraphedAttempt(object):
    def __init__(self, func, y0, f0, tableau):
        self.func = func
        self.tableau = tableau
        dev = y0[0].device
        self.y0 = tuple(torch.empty_like(y).copy_(y) for y in y0)            # static inputs of the graph
        self.f0 = tuple(torch.empty_like(f).copy_(f) for f in f0)
        self.td = torch.zeros(2, dtype=torch.float64, device=dev)            # [t0, dt]
        self.td_host = torch.zeros(2, dtype=torch.float64).pin_memory()
        self._pending = None                                                 # accepted (y1, f1) not yet copied into the inputs
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):                                        # warm-up off the capture (torch.cuda.graphs recipe)
            self.td.fill_(0.0)
            for _ in range(2):
                self._body()
        cur.wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self._body()

    def _body(self):
        y1, f1, err, k = _runge_kutta_step(self.func, self.y0, self.f0, self.td[0], self.td[1], self.tableau)
        recs = torch.stack([_error_norms(e, a, b) for e, a, b in zip(err, self.y0, y1)])
        return y1, f1, err, k, recs

    def matches(self, y0):
        return len(y0) == len(self.y0) and all(a.shape == b.shape and a.dtype == b.dtype and a.device == b.device
                                               for a, b in zip(y0, self.y0))

    def run(self, y0, f0, t0, dt):
        """One attempt from (y0, f0) at t0 with step dt.  Returns (y0_static, y1, f1, err, k, recs): static tensors that
        the NEXT run() overwrites (y1.. by the replay, y0_static by the deferred state copy)."""
        if self._pending is not None:
            y1p, f1p = self._pending
            if all(a is b for a, b in zip(y0, y1p)):                         # the caller advanced to the accepted state
                for dst, src in zip(self.y0, y1p):
                    dst.copy_(src)
                for dst, src in zip(self.f0, f1p):
                    dst.copy_(src)
            self._pending = None
        elif not all(a is b for a, b in zip(y0, self.y0)):                   # first call / foreign state
            for dst, src in zip(self.y0, y0):
                dst.copy_(src)
            for dst, src in zip(self.f0, f0):
                dst.copy_(src)
        self.td_host[0] = float(t0)
        self.td_host[1] = float(dt)
        self.td.copy_(self.td_host, non_blocking=True)
        self.graph.replay()
        y1, f1, err, k, recs = self.out
        return self.y0, y1, f1, err, k, recs

    def accepted(self, y1, f1):
        """The caller keeps (y1, f1) as its state: they move into the graph's inputs at the start of the next run()
        (not now: the dense output of this step still needs the old y0)."""
        self._pending = (y1, f1)


class GraphedFixedStep(object):
    """One step of a fixed-grid solver (solvers.py:94-97: dy = step_func(...); y1 = y0 + dy) as a hipGraph that updates
    the state in place.  The integration is then `for every grid interval: td <- (t0, dt) (device copy); replay; copy
    the state into solution[i+1]` - no host synchronisation anywhere in the loop."""

    def __init__(self, solver, y0):
        from .misc import _lincomb
        self.solver = solver
        dev = y0[0].device
        self.y = tuple(torch.empty_like(y).copy_(y) for y in y0)
        self.td = torch.zeros(2, dtype=torch.float64, device=dev)

        def body():
            dy = solver.step_func(solver.func, self.td[0], self.td[1], self.y)
            y1 = tuple(_lincomb(y_, [1.0], [dy_], 1.0) for y_, dy_ in zip(self.y, dy))      # solvers.py:95
            for y_, y1_ in zip(self.y, y1):
                y_.copy_(y1_)
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(2):
                body()
        cur.wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            body()
        for dst, src in zip(self.y, y0):                     # the warm-up advanced the state
            dst.copy_(src)

    def integrate_pairs(self, t0s, dts, outs):
        """t0s / dts: host float64 arrays (left grid points, interval lengths); outs: per component [T, ...] result tensors
        whose row 0 already holds y0."""
        import numpy as np
        pairs_dev = torch.from_numpy(np.ascontiguousarray(np.stack([t0s, dts], axis=1))).to(self.td.device)
        for i in range(pairs_dev.shape[0]):
            self.td.copy_(pairs_dev[i])
            self.graph.replay()
            for out, y_ in zip(outs, self.y):
                out[i + 1].copy_(y_)


# ---------------------------------------------------------------------------------------------
# adaptive RK for a Python callable with the controller on the device (libmi_ode family C, include/mi_ode.h)
# ---------------------------------------------------------------------------------------------
class _AutogradSeen(object):
    """Context that notices autograd recording inside f (a saved-tensor hook fires): such a right-hand side (the adjoint's
    augmented dynamics, Hamiltonian networks) must never be stream-captured - torch.autograd.grad under capture aborts."""

    def __init__(self):
        self.seen = False
        self._ctx = None

    def __enter__(self):
        def pack(x):
            self.seen = True
            return x
        self._ctx = torch.autograd.graph.saved_tensors_hooks(pack, lambda x: x)
        self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        return self._ctx.__exit__(*exc)


def _credit_nfe(func, missing):
    """Adds `missing` evaluations to an integer `nfe` attribute of the user's callable (unwrapping misc._TupleFunc /
    _ReverseFunc and the adjoint's tuple module), if it keeps one."""
    if missing <= 0:
        return
    base = func
    for _ in range(8):
        nxt = getattr(base, 'base', None)
        if nxt is None:
            nxt = getattr(base, 'base_func', None)
        if nxt is None:
            break
        base = nxt
    cur = getattr(base, 'nfe', None)
    if isinstance(cur, int) and not isinstance(cur, bool):
        try:
            base.nfe = cur + int(missing)
        except Exception:
            pass


_OPQ_FREE = {}                 # descriptor bytes -> idle native handles (a handle is in use by at most one integrate() at a time)
_OPQ_MAX_IDLE = 8


def _opq_handle(lib, key, desc, device):
    import ctypes as C
    from . import _native as N
    free = _OPQ_FREE.get(key)
    if free:
        return free.pop()
    idle = sum(len(v) for v in _OPQ_FREE.values())
    while idle >= _OPQ_MAX_IDLE:                                 # bounded: drop idle handles of other problems
        for k_ in list(_OPQ_FREE):
            if _OPQ_FREE[k_]:
                lib.mi_ode_opq_destroy(_OPQ_FREE[k_].pop())
                idle -= 1
                break
        else:
            break
    h = C.c_void_p()
    with torch.cuda.device(device):
        N.check(lib.mi_ode_opq_create(C.byref(desc), C.byref(h)), 'mi_ode_opq_create')
    return h


def clear_opq_handles():
    from . import _native as N
    lib = N.load()
    clear_recorded_attempts()
    for k_ in list(_OPQ_FREE):
        for h in _OPQ_FREE.pop(k_):
            lib.mi_ode_opq_destroy(h)


# ---- options={'graph': 'reuse'}: the recorded attempt outlives the call ----------------------------------------------------
# Recording an attempt costs two eager attempts, the capture and the instantiation of the graph - 2.5 ms for a 3-op callable, 5 ms
# for a ten-op one, which is most of a call of 40 attempts.  A training loop or a parameter sweep calls odeint with the SAME callable,
# shapes and tolerances again and again: with graph='reuse' the engine (native handle, static state buffers, the graph) is kept and
# later calls only copy y0 / f0 in, reset the controller record and replay.  This is a promise BY THE CALLER that f computes the same
# function of (t, y) every time, up to in-place updates of tensors it reads (optimizer steps): whatever else f depends on - a Python
# float it closes over, a rebound parameter tensor, module.training - is frozen at its value when the attempt was recorded.  Hence
# opt-in.  Keyed on the identity of the user's callable (checked through a weak reference), the wrappers around it, the state's
# shapes / dtype / device and everything the native handle was created with.
_RECORDED = collections.OrderedDict()
_RECORDED_MAX = 4


def _user_callable(func):
    chain = []
    base = func
    for _ in range(8):
        chain.append(type(base).__name__)
        nxt = getattr(base, 'base', None)
        if nxt is None:
            nxt = getattr(base, 'base_func', None)
        if nxt is None:
            break
        base = nxt
    return base, tuple(chain)


def _recorded_key(solver):
    base, chain = _user_callable(solver.func)
    tol = (tuple(float(r) for r in solver.rtol), tuple(float(a) for a in solver.atol)) if not solver.pooled_ratio else \
        (float(solver.rtol), float(solver.atol))
    return (id(base), chain, type(solver).__name__, tuple((tuple(y.shape), y.dtype, str(y.device)) for y in solver.y0), tol,
            float(solver.safety), float(solver.ifactor), float(solver.dfactor), int(solver.max_num_steps)), base


def recorded_engine(solver):
    """The engine an earlier graph='reuse' call with the same callable / shapes / tolerances left behind, or None."""
    key, base = _recorded_key(solver)
    hit = _RECORDED.get(key)
    if hit is None:
        return None
    eng, ref = hit
    if (ref() if ref is not None else None) is not base or eng.graph is None:          # the id was recycled by another object
        _RECORDED.pop(key)
        eng.close()
        return None
    _RECORDED.move_to_end(key)
    return eng


def keep_recorded(solver, eng):
    import weakref
    key, base = _recorded_key(solver)
    try:
        ref = weakref.ref(base)
    except TypeError:                                            # not weak-referenceable (a builtin, a __slots__ object): nothing to pin the id to
        eng.close()
        return
    old = _RECORDED.pop(key, None)
    if old is not None and old[0] is not eng:
        old[0].close()
    _RECORDED[key] = (eng, ref)
    while len(_RECORDED) > _RECORDED_MAX:
        _, (e_, _r) = _RECORDED.popitem(last=False)
        e_.close()


def clear_recorded_attempts():
    while _RECORDED:
        _, (e_, _r) = _RECORDED.popitem()
        e_.close()


class DeviceControlledRK(object):
    """One `integrate()` of an adaptive Runge-Kutta solver (dopri5.py:70-121 and its siblings) for an arbitrary Python
    right-hand side, with the scalar state of the solver on the device.

    An attempt is: S x (stage combination `mi_ode_lincomb_dev`, f), `mi_ode_opq_finish` (error estimate, norms, controller:
    accept test, next step size, output cursor), `mi_ode_opq_commit` (dense output of the requested times inside an accepted
    step, state <- y1 / f1).  It contains no host value, so it runs
      * eagerly - Python calls f every stage, the host reads the `done` flag back once per attempt - or
      * as a hipGraph recorded once (after the eager attempts that served as warm-up) and replayed in chunks, the host
        reading the scalar state back once per chunk.
    `graph`: False never captures, True captures after the first eager attempt, 'auto' (default of the solvers) captures when
    enough attempts remain to pay for the recording and f was not seen to use autograd."""

    EAGER_FIRST = 2            # 'auto': eager attempts before a capture is considered (they are the warm-up of the capture)
    MIN_REMAINING = 12         # 'auto': capture only if about this many attempts are still to come
    _told = False              # the one-time note about what a recorded right-hand side means
    MAX_CHUNK = 64

    def __init__(self, solver, graph='auto'):
        import ctypes as C
        import numpy as np
        from . import _native as N
        from .misc import _DevScalar
        from .rk_common import _is_fsal_shaped
        from .solvers import _fill_tableau
        self.N, self.C = N, C
        self.lib = N.load()
        self.solver = solver
        self.func = solver.func
        self.tableau = solver.tableau
        self.fsal = _is_fsal_shaped(self.tableau)
        self.graph_mode = graph
        if getattr(self.func, '_mi_no_capture', False) and self.graph_mode != 'host':
            self.graph_mode = False                         # (adjoint.py: dynamics that call torch.autograd.grad - never recorded)
        y0 = solver.y0
        self.device = y0[0].device
        self.dtype = y0[0].dtype
        self.ncomp = len(y0)
        d = N.OpqDesc()
        d.dtype = N.dtype_code(self.dtype)
        d.n_comp = self.ncomp
        for c, y in enumerate(y0):
            d.n[c] = int(y.numel())
        _fill_tableau(d.tableau, self.tableau, solver.c_mid)
        d.controller, d.interp, d.order, d.init_order = solver.controller, solver.interp, solver.order, solver.init_order
        if solver.pooled_ratio:
            rt, at = [float(solver.rtol)] * self.ncomp, [float(solver.atol)] * self.ncomp
        else:
            rt, at = [float(r) for r in solver.rtol], [float(a) for a in solver.atol]
        for c in range(self.ncomp):
            d.rtol[c], d.atol[c] = rt[c], at[c]
        d.safety, d.ifactor, d.dfactor = float(solver.safety), float(solver.ifactor), float(solver.dfactor)
        d.max_num_steps = int(solver.max_num_steps)
        self.S = len(self.tableau.alpha)
        # a right-hand side with a fused stage kernel (rhs.Conv2dODE, also behind misc._TupleFunc / _ReverseFunc): one launch per stage
        # forms the stage state and evaluates f; every other callable keeps the lincomb + f path below
        st = getattr(self.func, 'stage_rhs', None)
        y = y0[0]
        self.stage_rhs = st if (st is not None and self.ncomp == 1 and st.supports(y) and not y.requires_grad) else None
        self._stage_note = '' if self.stage_rhs is None else ', fused stage kernel'
        self._key = (bytes(d), str(self.device))
        self.h = _opq_handle(self.lib, self._key, d, self.device)
        h = self.h
        self.dt_dev = _DevScalar(self.lib.mi_ode_opq_dt_dev(h))
        self.ts = torch.zeros(self.S, dtype=self.dtype, device=self.device)
        self.ts_views = [self.ts[s] for s in range(self.S)]      # what f receives as t: 0-d views, rewritten by the controller
        self.stats = N.Stats()
        self.graph = None
        self.py_calls = 0
        self.captured = False
        self._t_cap = 1024                                        # output times the native handle holds without reallocating
        self._np = np

    def close(self):
        """Drops the recorded graph and hands the native handle back to the cache (handles are reused across odeint calls: no
        hipMalloc / hipFree per call)."""
        self.graph = None
        self._keep = None
        if getattr(self, 'h', None):
            _OPQ_FREE.setdefault(self._key, []).append(self.h)
            self.h = None

    # -- one attempt (eager, or under capture) ------------------------------------------------------
    def _ptr_array(self, tensors):
        return (self.C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])

    def _attempt(self):
        from .misc import _contig, _lincomb
        tb = self.tableau
        k = [[f0_] for f0_ in self.F0]
        yi = None
        if self.stage_rhs is not None:                                                               # (py_calls: no Python evaluation)
            last = len(tb.beta) - 1
            for s, beta_i in enumerate(tb.beta):
                k_, y_ = self.stage_rhs.stage(self.ts_views[s], self.Y0[0], k[0], beta_i, self.dt_dev, want_y=self.fsal and s == last)
                k[0].append(k_)
                if y_ is not None:
                    yi = (y_,)
        for s, beta_i in enumerate(tb.beta if self.stage_rhs is None else ()):
            yi = tuple(_lincomb(y0_, beta_i, k_, self.dt_dev) for y0_, k_ in zip(self.Y0, k))      # rk_common.py:51
            self.py_calls += 1
            for k_, f_ in zip(k, self.func(self.ts_views[s], yi)):                                   # rk_common.py:52
                k_.append(_contig(f_))
        if not self.fsal:                                                                            # rk_common.py:54-56
            yi = tuple(_lincomb(y0_, tb.c_sol, k_, self.dt_dev) for y0_, k_ in zip(self.Y0, k))
        st = self.N.stream_ptr(self.device)
        y0p, f0p, y1p = self._ptr_array(self.Y0), self._ptr_array(self.F0), self._ptr_array(yi)
        kp = self._ptr_array([x for k_ in k for x in k_])
        self.N.check(self.lib.mi_ode_opq_finish(self.h, y0p, y1p, kp, st), 'mi_ode_opq_finish')
        self.N.check(self.lib.mi_ode_opq_commit(self.h, y0p, f0p, y1p, kp, st), 'mi_ode_opq_commit')
        return yi, k          # (kept alive by the caller until the stream has consumed them)

    def _poll(self):
        done = self.C.c_int32(0)
        rc = self.N.check(self.lib.mi_ode_opq_poll(self.h, self.C.byref(self.stats), self.C.byref(done), self.N.stream_ptr(self.device)),
                          'mi_ode_opq_poll')
        return bool(done.value), rc

    def _try_capture(self):
        """Record one attempt.  True on success; False (and eager from then on) when f is not capture-safe."""
        try:
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._keep = self._attempt()
            self.graph = g
            self.captured = True
            if self.graph_mode == 'auto' and not DeviceControlledRK._told:
                # (advisor, round 4) a semantic difference from the reference's eager loop, said once: from here on f's PYTHON body does
                # not run again in this call - only the device work it enqueued when it was recorded is replayed
                DeviceControlledRK._told = True
                import warnings
                warnings.warn("tfdiffeq_amd: the right-hand side was recorded as a hipGraph after %d eager attempts and is replayed from "
                              "here on: Python-side effects inside f (logging, counters other than an integer `nfe`, hooks) stop, and f "
                              "received 0-d VIEWS of a device time buffer the controller overwrites (clone t to keep it).  "
                              "options={'graph': False} keeps one Python evaluation per stage." % self.EAGER_FIRST)
            return True
        except Exception as e:                                   # host synchronisation / data-dependent control flow inside f, ...
            import warnings
            self.graph = None
            try:
                torch.cuda.synchronize(self.device)
            except Exception:
                pass
            warnings.warn('tfdiffeq_amd: the right-hand side cannot be recorded as a hipGraph (%s: %s); continuing with one '
                          'Python evaluation per stage' % (type(e).__name__, str(e).split('\n')[0][:200]))
            return False

    def _chunk(self, t_end):
        """Replays to enqueue before the next read-back of the scalar state.  The estimate of the attempts still to come is (t_end - t) / dt
        at the CURRENT step size; a replay past the end is a no-op on the device but still costs the recorded f (round 4: tsit5 with
        graph=True took 87 replays for 64 attempts - the estimate right after the small first step was 64, the next one 23 - 15.5 ms against
        12.2).  So only HALF of the estimate is enqueued blind while it is large: a read-back costs a fraction of one wasted replay."""
        rem = self._remaining(t_end)
        return min(self.MAX_CHUNK, max(2, (rem + 1) // 2 if rem > 4 else rem))

    def _remaining(self, t_end):
        dt = self.stats.dt
        if not (dt > 0):
            return 1
        return max(1, int(min(1e6, self._np.ceil((t_end - self.stats.t) / dt))))

    # -- the whole integrate() ------------------------------------------------------------------------
    def integrate(self, t64, y0, f0, first_dt):
        """t64: increasing float64 numpy array of T >= 1 times; y0 / f0: tuples of device tensors.  Returns the tuple of
        [T, *shape] solutions and fills `self.stats` / `self.info`."""
        N, C = self.N, self.C
        T = int(t64.shape[0])
        outs = tuple(torch.empty((T,) + tuple(y.shape), dtype=y.dtype, device=y.device) for y in y0)
        for o, y in zip(outs, y0):
            o[0].copy_(y)
        self.info = {'engine': 'device-controlled attempts (%s)' % ('fused stage kernel, one launch per stage' if self.stage_rhs is not None
                                                                   else 'one Python evaluation per stage'), 'replays': 0, 'polls': 0}
        self.py_calls = 0
        if T == 1:
            return outs
        n_out = T - 1
        if self.captured and n_out > self._t_cap:                 # opq_begin is about to move the output-time buffer the recorded kernels
            self.graph, self._keep, self.captured = None, None, False      # point to (include/mi_ode.h): record again
        self._t_cap = max(self._t_cap, n_out)
        replay_only = self.captured and self.graph is not None    # graph='reuse': an earlier call recorded the attempt
        if replay_only:
            for dst, src in zip(self.Y0, y0):
                dst.copy_(src)
            for dst, src in zip(self.F0, f0):
                dst.copy_(src)
        else:
            # static state buffers: commit() moves y1 / f1 into them on accept, the stage combinations always read them
            self.Y0 = tuple(torch.empty_like(y, memory_format=torch.contiguous_format).copy_(y) for y in y0)
            self.F0 = tuple(torch.empty_like(f, memory_format=torch.contiguous_format).copy_(f) for f in f0)
        tt = self._np.ascontiguousarray(t64[1:], dtype=self._np.float64)
        rows = (C.c_void_p * self.ncomp)(*[o[1].data_ptr() for o in outs])
        with torch.cuda.device(self.device):
            rc = N.check(self.lib.mi_ode_opq_begin(self.h, float(t64[0]), float(first_dt), tt.ctypes.data_as(C.POINTER(C.c_double)), n_out,
                                                   rows, C.c_void_p(self.ts.data_ptr()), N.stream_ptr(self.device)), 'mi_ode_opq_begin')
            assert rc == 0, N.status_message(rc)
            t_end = float(t64[-1])
            mode = self.graph_mode
            eager = 0
            done = False
            autograd = _AutogradSeen()
            if replay_only:
                self.info['engine'] = 'device-controlled attempts (hipGraph recorded by an earlier call, replayed%s)' % self._stage_note
                chunk = 8                                          # (nothing is known about this call's step sizes yet; replays after `done` are no-ops)
                while not done:
                    for _ in range(chunk):
                        self.graph.replay()
                    self.info['replays'] += chunk
                    done, rc = self._poll()
                    self.info['polls'] += 1
                    chunk = self._chunk(t_end)
            while not done:
                with autograd:
                    keep = self._attempt()
                eager += 1
                done, rc = self._poll()
                del keep
                self.info['polls'] += 1
                if done or mode is False or autograd.seen:
                    continue
                if mode is True or (eager >= self.EAGER_FIRST and self._remaining(t_end) >= self.MIN_REMAINING):
                    if not self._try_capture():
                        mode = False
                        continue
                    self.info['engine'] = 'device-controlled attempts (hipGraph replay, %d eager attempts first%s)' % (eager, self._stage_note)
                    while not done:
                        chunk = self._chunk(t_end)
                        for _ in range(chunk):
                            self.graph.replay()
                        self.info['replays'] += chunk
                        done, rc = self._poll()
                        self.info['polls'] += 1
        self.info['eager_attempts'] = eager
        self.info['python_evaluations'] = self.py_calls          # (0 on the fused stage path: f ran inside the stage kernels)
        self.info['autograd_in_f'] = autograd.seen
        return outs
