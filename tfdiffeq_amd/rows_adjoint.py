"""Gradients for per-trajectory solves: odeint_adjoint(..., options={'per_trajectory': True}).

Forward: the per-trajectory solve itself (k_rows_rowlocal, unchanged).  Backward: row i gets the reference's adjoint algorithm
(adjoint.py:117-178, restated in adjoint.py::_generic_backward) applied to trajectory i ALONE - every interval an adaptive solve of the
row's own tuple state (y, adj_y, adj_t, adj_params) with per-component control - for all rows in ONE launch of k_rows_adjoint
(csrc/mi_ode_rows_adjoint.h), behind the vjp `lower.adjoint_source` generates for the traced module.  The call is planned where it is
made: trace, classify, generate, build.  What the route cannot take is a ValueError with the reason, decided without a device; nothing is
ever answered with shared control.

Per-row inputs: a `t` of shape [batch, T], options['t_lengths'] and [batch] rtol / atol / adjoint_rtol / adjoint_atol take
the forward to k_rows_rowlocal_t and the backward to k_rows_adjoint_t (csrc/mi_ode_rows_adjoint_t.h): row i is the backward above on
(y0[i:i+1], t[i, :len_i]) at the row's own tolerances, the gradient of `t` is [batch, T] - the rows' own, not summed, zero from len_i on.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N
from . import dispatch as D

_REFUSED = "options['per_trajectory'] refused: "


def _tableau(method):
    if method == 'dopri5':
        from .dopri5 import _DORMAND_PRINCE_SHAMPINE_TABLEAU, DPS_C_MID
        return _DORMAND_PRINCE_SHAMPINE_TABLEAU, DPS_C_MID, 5, 4             # dopri5.py:68, 74
    from .bosh3 import _BOGACKI_SHAMPINE_TABLEAU, BS_C_MID
    return _BOGACKI_SHAMPINE_TABLEAU, BS_C_MID, 3, 2                          # bosh3.py:51, 57


class _Plan(object):
    """What ONE call needs: the lowered forward, the trace's parameter layout, the generated source and - on a device - the plugin and a
    copy of the constants the call was bound with (the program's pool buffer is shared: the next odeint of the same program overwrites it)."""

    def __init__(self, low, run_opts, params, targets, n_params, source, cfg):
        self.low, self.run_opts, self.params, self.targets, self.n_params, self.source, self.cfg = low, run_opts, params, targets, n_params, source, cfg
        self.dim = int(low.dim)
        self.lib = self.table = self.pool = None
        self.scalars = []
        self.per_row = False         # per-row times, lengths or tolerances: k_rows_adjoint_t
        self.times = None            # rows_times.RowsTimes of the call (per_row only)

    def kernel(self, dtype):
        S = len(_tableau(self.cfg['adjoint_method'])[0].alpha)
        name, what = ('k_rows_adjoint_t', 'the whole backward of every row over its own times, length and tolerances') if self.per_row else (
            'k_rows_adjoint', 'the whole backward of every row')
        return '%s<%s, %d, ..> (a trajectory per thread: %s, N_aug = %d)' % (
            name, 'double' if dtype == torch.float64 else 'float', S, what, 2 * self.dim + 1 + max(self.n_params, 1))

    def engine(self):
        return ('k_rows_adjoint_t: ' + D.ROWS_ADJOINT_T_WHY) if self.per_row else ('k_rows_adjoint: ' + D.ROWS_ADJOINT_WHY)


def _rows_tol(x):
    """True for a tolerance with one value per row (a tensor or array [batch]); shapes are refused before (_per_row_inputs)."""
    return len(D._shape_of(x) or ()) >= 1


def make_plan(func, y0, method, options, adjoint_method, adjoint_rtol, adjoint_atol, adjoint_options, build=True, per_row=False):
    """The _Plan of odeint_adjoint(func, y0, ..., options={'per_trajectory': True, **options}) or a ValueError with the reason.  options /
    adjoint_options: without the 'per_trajectory' and 't_lengths' keys.  per_row: the call has per-row times, lengths or tolerances
    (adjoint_rtol / adjoint_atol may then be [batch])."""
    from .adjoint import _trainable
    from .odeint import _per_trajectory_target

    def refuse(why):
        raise ValueError(_REFUSED + why)
    if isinstance(y0, (tuple, list)):
        refuse('a tuple state of several components: the per-trajectory adjoint takes one [batch, dim] tensor (its own augmented state is the tuple)')
    low, run_opts = _per_trajectory_target(func, y0, method, options, _adjoint=True)      # (the forward mode's own refusals, but the one for gradients)
    if low is None:
        refuse('a device right-hand side descriptor has no generated vjp: pass the system as a torch.nn.Module the tracer lowers to a row program')
    from . import lower as L
    tr = low.trace
    params = tuple(_trainable(func))
    plist, n_params = L.vjp_params(tr)
    targets = []
    for idx, off, n in plist:
        e = tr.tensors[idx]
        x = e['t']
        if not x.is_leaf:
            refuse('a derived (non-leaf) trainable tensor of shape %s enters the module (W.t(), a slice, a product): the kernel differentiates '
                   'with respect to the tensors the trace reads' % (list(x.shape),))
        if e['lead'] != 0:
            refuse('a trainable tensor of shape %s with batch axes (give every member its own parameters as extra state, or call once per member)'
                   % (list(x.shape),))
        k = [j for j, p_ in enumerate(params) if p_ is x]
        if not k:
            refuse('the trace reads a trainable tensor of shape %s that is not a parameter of the module' % (list(x.shape),))
        targets.append((k[0], off, n))
    for req in tr.tensors:
        if req['t'].requires_grad and not req['t'].dtype.is_floating_point:
            refuse('a trainable tensor of dtype %s' % req['t'].dtype)
    missing = [p_ for j, p_ in enumerate(params) if all(k != j for k, _o, _n in targets)]
    if missing:
        refuse('a parameter of shape %s does not enter the trace as it is (it is used through a derived tensor, or not at all)' % (list(missing[0].shape),))
    why = D.rows_adjoint_refusal(low.dim, n_params, adjoint_method, adjoint_rtol, adjoint_atol, adjoint_options)
    if why:
        refuse(why)
    try:
        source = L.adjoint_source(tr)
    except L.TraceError as e:
        refuse(str(e))
    # (a [batch] tolerance travels as it is; the descriptor's scalar is then a placeholder the kernel never reads)
    cfg = dict(adjoint_method=adjoint_method, adjoint_rtol=D.ROWS_T_RTOL0 if _rows_tol(adjoint_rtol) else float(adjoint_rtol),
               adjoint_atol=D.ROWS_T_ATOL0 if _rows_tol(adjoint_atol) else float(adjoint_atol),
               adjoint_rtol_rows=adjoint_rtol if _rows_tol(adjoint_rtol) else None, adjoint_atol_rows=adjoint_atol if _rows_tol(adjoint_atol) else None,
               max_num_steps=int((adjoint_options or {}).get('max_num_steps', 2 ** 31 - 1)))
    plan = _Plan(low, run_opts, params, targets, n_params, source, cfg)
    plan.per_row = bool(per_row)
    if build and y0.is_cuda:
        from . import rhs as R
        if per_row:
            plan.source = R.rows_adjoint_t_source_of(source)
            plan.lib, plan.table = R.rows_adjoint_t_plugin(plan.source, y0.dtype)
        else:
            plan.lib, plan.table = R.rows_adjoint_plugin(source, y0.dtype)
        bound = low.rhs
        plan.pool = None if bound.pool is None else bound.pool.clone()
        plan.scalars = list(bound.params)
    return plan


def _normalise(method, options, adjoint_method, adjoint_rtol, adjoint_atol, adjoint_options, rtol, atol):
    """adjoint.py:190-197 (the adjoint arguments default to the forward ones), with the 'per_trajectory' key taken out of both option sets."""
    if method is None:
        raise ValueError('cannot supply `options` without specifying `method`')
    if adjoint_options is None:
        adjoint_options = options
    adjoint_options = {k: v for k, v in (adjoint_options or {}).items() if k not in ('per_trajectory', 't_lengths')}
    return (method if adjoint_method is None else adjoint_method, rtol if adjoint_rtol is None else adjoint_rtol,
            atol if adjoint_atol is None else adjoint_atol, adjoint_options)


def _per_row_inputs(y0, t, rtol, atol, options, adjoint_rtol, adjoint_atol):
    """(per_row, options without 't_lengths') from shapes alone: per-row times, lengths and tolerances - the forward's, or
    [batch] adjoint tolerances of their own - take the call to k_rows_rowlocal_t / k_rows_adjoint_t.  ValueError: the shapes do not fit the
    state, with the reason."""
    from . import rows_times
    fwd, why = rows_times.shapes(y0, t, rtol, atol, options)
    bare = {k: v for k, v in (options or {}).items() if k != 't_lengths'}
    adj = False
    if not why:
        adj, why = rows_times.shapes(y0, None, adjoint_rtol, adjoint_atol, bare, names=('adjoint_rtol', 'adjoint_atol'))
    if why:
        raise ValueError(_REFUSED + why)
    return bool(fwd or adj), (bare if fwd or adj else options)


def plan(func, y0, t=None, rtol=1e-6, atol=1e-12, method=None, options=None, adjoint_method=None, adjoint_rtol=None, adjoint_atol=None,
         adjoint_options=None):
    """What odeint_adjoint(..., options={'per_trajectory': True}) will run: the forward's plan (`odeint.plan`) plus `backward`: the adjoint
    kernel, or engine 'refused' with the reason the call raises."""
    method = method or 'dopri5'
    opts, per_row = D.per_trajectory_option(options)
    if not per_row:
        raise ValueError("odeint_adjoint.plan describes the per-trajectory adjoint: pass options={'per_trajectory': True}")
    try:
        per_row_t, bare = _per_row_inputs(y0, t, rtol, atol, opts, adjoint_rtol, adjoint_atol)
        am, art, aat, aopts = _normalise(method, bare, adjoint_method, adjoint_rtol, adjoint_atol, adjoint_options, rtol, atol)
        p = make_plan(func, y0, method, bare, am, art, aat, aopts, build=False, per_row=per_row_t)
    except ValueError as e:
        return {'engine': 'refused', 'kernel': None, 'launches': None, 'per_trajectory': True, 'adjoint': True, 'why': str(e), 'lower': None}
    from .plan import plan_rows
    with torch.no_grad():
        fwd = plan_rows(func, y0, rtol, atol, method, dict(opts or {}), t)
    return {'engine': 'fused', 'kernel': p.kernel(y0.dtype), 'launches': 'one per backward',
            'why': D.ROWS_ADJOINT_T_WHY if per_row_t else D.ROWS_ADJOINT_WHY, 'per_trajectory': True,
            'adjoint': True, 'n_aug': 2 * p.dim + 1 + max(p.n_params, 1), 'n_params': p.n_params, 'forward': fwd, 'lower': fwd.get('lower')}


def _rhs_of(plan_):
    """The mi_ode_rhs of the plan's plugin with the constants the call was bound with."""
    r = N.Rhs()
    r.kind, r.sign, r.plugin = N.RHS_PLUGIN, 1.0, plan_.table
    for i, v in enumerate(plan_.scalars[:8]):
        r.scalars[i] = v
    if plan_.pool is not None:
        r.w[0] = plan_.pool.data_ptr()
    return r


def _check_rows(row_status, batch, cfg):
    """The AssertionError of the lowest failing row, with the count and first indices of the failing rows (reads row_status: waits)."""
    bad = torch.nonzero(row_status).flatten().tolist()
    if bad:
        first = bad[0]
        bits = int(row_status[first])
        msg = N.status_text(bits, cfg['max_num_steps'])          # dopri5.py:85 (a row's step size is not reported: the library's text)
        raise AssertionError('%s [per_trajectory adjoint: %d of %d rows failed; rows %s%s, the message is row %d\'s]' % (
            msg, len(bad), batch, ', '.join(str(i) for i in bad[:8]), ', ...' if len(bad) > 8 else '', first))


def run_backward(plan_, t, ans, grad_ans):
    """(grad_y0 [batch, D], grad_params [P] in the trace's compact order, time_vjps [T], rows dict, n_launches) - ans / grad_ans:
    [T, batch, D], contiguous, on the device."""
    from .solvers import _fill_tableau
    n_t, batch, dim = (int(v) for v in ans.shape)
    dev, dtype = ans.device, ans.dtype
    P, PP = plan_.n_params, max(plan_.n_params, 1)
    cfg = plan_.cfg
    tb, c_mid, order, init_order = _tableau(cfg['adjoint_method'])
    f32 = lambda v: float(np.float32(v))                 # noqa: E731  (misc.py:137-144: python float -> float32 -> float64)
    d = N.AdjointRowsDesc()
    d.dtype, d.n_times, d.batch, d.dim, d.n_params = N.dtype_code(dtype), n_t, batch, dim, P
    d.order, d.init_order = order, init_order
    d.rtol, d.atol = cfg['adjoint_rtol'], cfg['adjoint_atol']
    d.safety, d.ifactor, d.dfactor = f32(0.9), f32(10.0), f32(0.2)
    d.max_num_steps = cfg['max_num_steps']
    _fill_tableau(d.tableau, tb, c_mid)
    groups = (batch + N.ROWS_ADJOINT_THREADS - 1) // N.ROWS_ADJOINT_THREADS
    neg_t = (-torch.as_tensor(t).detach().to(torch.float64)).to(dev).contiguous()
    row_params = torch.empty(batch, PP, dtype=dtype, device=dev)
    row_tvjp = torch.empty(batch, n_t, dtype=dtype, device=dev)
    counts_buf = torch.zeros(batch, 3, max(n_t - 1, 1), dtype=torch.int64, device=dev)       # (never empty: the C side refuses null)
    row_counts = counts_buf[:, :, :n_t - 1]
    row_status = torch.zeros(batch, dtype=torch.int64, device=dev)
    work = torch.zeros(groups * (PP + n_t) + 2, dtype=dtype, device=dev)      # [groups, PP + T] partials, then the ticket word (zeroed)
    d.neg_t_dev, d.row_params_dev, d.row_time_vjps_dev = neg_t.data_ptr(), row_params.data_ptr(), row_tvjp.data_ptr()
    d.row_counts_dev, d.row_status_dev = counts_buf.data_ptr(), row_status.data_ptr()
    d.partials_dev, d.ticket_dev = work.data_ptr(), work.data_ptr() + groups * (PP + n_t) * work.element_size()
    r = _rhs_of(plan_)
    g_y0 = torch.empty(batch, dim, dtype=dtype, device=dev)
    g_th = torch.empty(PP, dtype=dtype, device=dev)
    g_t = torch.empty(n_t, dtype=dtype, device=dev)
    stats = N.Stats()
    with torch.cuda.device(dev):
        N.check(N.load().mi_ode_adjoint_rows(C.byref(d), C.byref(r), ans.data_ptr(), grad_ans.data_ptr(), g_y0.data_ptr(), g_th.data_ptr(),
                                             g_t.data_ptr(), C.byref(stats), N.stream_ptr(dev)), 'mi_ode_adjoint_rows')
    rows = {'grad_params': row_params[:, :P], 'time_vjps': row_tvjp, 'n_attempts': row_counts[:, 0], 'n_accepted': row_counts[:, 1],
            'nfe': row_counts[:, 2], 'status': row_status}
    _check_rows(row_status, batch, cfg)                       # (the one synchronisation of the backward)
    del neg_t, work
    return g_y0, g_th[:P], g_t, rows, int(stats.n_launches)


def run_backward_t(plan_, ans, grad_ans):
    """run_backward with the call's per-row times, lengths and tolerances (plan_.times; k_rows_adjoint_t): time_vjps is [batch, T], every
    row's own, with exact zeros from the row's length on, as the counts of the intervals beyond it are."""
    from .solvers import _fill_tableau
    n_t, batch, dim = (int(v) for v in ans.shape)
    dev, dtype = ans.device, ans.dtype
    P, PP = plan_.n_params, max(plan_.n_params, 1)
    cfg, rt = plan_.cfg, plan_.times
    tb, c_mid, order, init_order = _tableau(cfg['adjoint_method'])
    f32 = lambda v: float(np.float32(v))                 # noqa: E731  (misc.py:137-144: python float -> float32 -> float64)
    d = N.AdjointRowsTDesc()
    d.dtype, d.n_times, d.batch, d.dim, d.n_params = N.dtype_code(dtype), n_t, batch, dim, P
    d.order, d.init_order = order, init_order
    d.rtol, d.atol = cfg['adjoint_rtol'], cfg['adjoint_atol']
    d.safety, d.ifactor, d.dfactor = f32(0.9), f32(10.0), f32(0.2)
    d.max_num_steps = cfg['max_num_steps']
    _fill_tableau(d.tableau, tb, c_mid)
    groups = (batch + N.ROWS_ADJOINT_THREADS - 1) // N.ROWS_ADJOINT_THREADS
    neg_t = (-rt.t).contiguous()                             # [batch, T] float64 on the device (the padding of a short row is never read)
    assert tuple(neg_t.shape) == (batch, n_t) and neg_t.device == dev
    tols = [None if x is None else torch.as_tensor(x).detach().to(device=dev, dtype=torch.float64).contiguous()
            for x in (cfg['adjoint_rtol_rows'], cfg['adjoint_atol_rows'])]
    row_params = torch.empty(batch, PP, dtype=dtype, device=dev)
    row_tvjp = torch.empty(batch, n_t, dtype=dtype, device=dev)
    counts_buf = torch.zeros(batch, 3, max(n_t - 1, 1), dtype=torch.int64, device=dev)       # (never empty: the C side refuses null)
    row_counts = counts_buf[:, :, :n_t - 1]
    row_status = torch.zeros(batch, dtype=torch.int64, device=dev)
    work = torch.zeros(groups * PP + 2, dtype=dtype, device=dev)              # [groups, PP] partials, then the ticket word (zeroed)
    d.neg_t_dev, d.row_params_dev, d.row_time_vjps_dev = neg_t.data_ptr(), row_params.data_ptr(), row_tvjp.data_ptr()
    d.len_dev = None if rt.lengths is None else rt.lengths.data_ptr()
    d.rtol_dev, d.atol_dev = (None if x is None else x.data_ptr() for x in tols)
    d.row_counts_dev, d.row_status_dev = counts_buf.data_ptr(), row_status.data_ptr()
    d.partials_dev, d.ticket_dev = work.data_ptr(), work.data_ptr() + groups * PP * work.element_size()
    r = _rhs_of(plan_)
    g_y0 = torch.empty(batch, dim, dtype=dtype, device=dev)
    g_th = torch.empty(PP, dtype=dtype, device=dev)
    stats = N.Stats()
    with torch.cuda.device(dev):
        N.check(N.load().mi_ode_adjoint_rows_t(C.byref(d), C.byref(r), ans.data_ptr(), grad_ans.data_ptr(), g_y0.data_ptr(), g_th.data_ptr(),
                                               C.byref(stats), N.stream_ptr(dev)), 'mi_ode_adjoint_rows_t')
    rows = {'grad_params': row_params[:, :P], 'time_vjps': row_tvjp, 'n_attempts': row_counts[:, 0], 'n_accepted': row_counts[:, 1],
            'nfe': row_counts[:, 2], 'status': row_status}
    _check_rows(row_status, batch, cfg)                       # (the one synchronisation of the backward)
    del neg_t, work, tols
    return g_y0, g_th[:P], row_tvjp, rows, int(stats.n_launches)


class _OdeintAdjointRows(torch.autograd.Function):

    @staticmethod
    def forward(ctx, plan_, func, call, t, flat_params, y0):
        from .odeint import _run_lowered, odeint
        # (autograd.Function.forward runs with gradients disabled: the marker under which the forward reaches the rows kernel - plain
        # odeint keeps refusing inputs that require grad)
        ans = _run_lowered(plan_.low, func, y0, t, call['rtol'], call['atol'], call['method'], plan_.run_opts)
        fstats = odeint.last_stats if isinstance(odeint.last_stats, dict) else {}
        ctx.forward_info = dict(fstats.get('lower') or {}, engine=fstats.get('engine'), n_launches=fstats.get('n_launches'))
        ctx.plan, ctx.y_shape = plan_, tuple(y0.shape)
        ctx.save_for_backward(t, flat_params, ans)
        return ans

    @staticmethod
    def backward(ctx, grad_output):
        from .adjoint import odeint_adjoint
        plan_ = ctx.plan
        t, flat_params, ans = ctx.saved_tensors
        n_t = int(ans.shape[0])
        with torch.no_grad():
            a = ans.reshape(n_t, -1, plan_.dim).contiguous()
            g = (grad_output if grad_output is not None else torch.zeros_like(ans)).reshape(n_t, -1, plan_.dim).to(ans.dtype).contiguous()
            if plan_.per_row:
                g_y0, g_th, g_t, rows, n_launches = run_backward_t(plan_, a, g)
                if t.dim() == 1:                          # ([batch] tolerances with shared times: the rows' time gradients, summed in row order)
                    g_t = g_t.sum(dim=0)
            else:
                g_y0, g_th, g_t, rows, n_launches = run_backward(plan_, t, a, g)
            grad_params = None
            if flat_params.numel() > 0:
                offs, o = [], 0
                for p_ in plan_.params:
                    offs.append(o)
                    o += p_.numel()
                grad_params = torch.zeros(o, dtype=ans.dtype, device=ans.device)
                for k, off, n in plan_.targets:           # the trace's compact order -> the flat order of the module's parameters
                    grad_params[offs[k]:offs[k] + n] = g_th[off:off + n]
                grad_params = grad_params.to(flat_params.dtype)
            tot = {k: int(rows[k].sum(dim=1).max()) if n_t > 1 else 0 for k in ('n_attempts', 'n_accepted', 'nfe')}
        odeint_adjoint.last_backward_stats = dict(
            tot, engine=plan_.engine(), kernel=plan_.kernel(ans.dtype), n_launches=n_launches, per_trajectory=True,
            rows=rows, forward=ctx.forward_info)
        return None, None, None, g_t.to(dtype=t.dtype, device=t.device), grad_params, g_y0.reshape(ctx.y_shape)


def odeint_adjoint_rows(func, y0, t, rtol, atol, method, options, adjoint_method, adjoint_rtol, adjoint_atol, adjoint_options):
    """odeint_adjoint with options['per_trajectory'] True; `options` without the key."""
    from .adjoint import _FlatParams
    per_row, bare = _per_row_inputs(y0, t, rtol, atol, options, adjoint_rtol, adjoint_atol)
    am, art, aat, aopts = _normalise(method, bare, adjoint_method, adjoint_rtol, adjoint_atol, adjoint_options, rtol, atol)
    plan_ = make_plan(func, y0, method, bare, am, art, aat, aopts, per_row=per_row)      # (refusals first: a ValueError whatever device y0 is on)
    if per_row:
        from . import rows_times
        plan_.times, _ = rows_times.prepare(y0, t, rtol, atol, options)       # (values: lengths in range, rows monotone in one direction)
        if plan_.times is None:                               # (only the adjoint tolerances are per row: the forward is the shared-t call)
            plan_.times, _ = rows_times.prepare(y0, t, art, aat, bare)
        if plan_.times.decreasing:
            raise ValueError(_REFUSED + 'decreasing rows of `t`: the per-row adjoint kernel integrates every row backwards over increasing '
                             'times (solve with plain odeint under torch.no_grad(), or reverse the rows)')
        if 't_lengths' in (options or {}):
            plan_.run_opts = dict(plan_.run_opts, t_lengths=options['t_lengths'])
    N.require_gpu_tensor(y0, 'y0')
    params = plan_.params
    flat_params = _FlatParams.apply({'optional': frozenset()}, *params) if params else torch.zeros(0, device=y0.device, dtype=y0.dtype)
    call = dict(rtol=rtol, atol=atol, method=method)
    return _OdeintAdjointRows.apply(plan_, func, call, torch.as_tensor(t), flat_params, y0)
