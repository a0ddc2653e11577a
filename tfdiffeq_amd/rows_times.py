"""Per-row output times, lengths and tolerances of options={'per_trajectory': True}: what the call's `t` [batch, T],
options['t_lengths'] [batch] and `rtol` / `atol` [batch] become before k_rows_rowlocal_t (csrc/mi_ode_rows_t.h) is launched.

Shapes are refused by the pure functions of dispatch.py; values are checked here with tensor operations on the state's device, behind ONE
host read (as misc._assert_increasing has one): lengths in 1 .. T and every row strictly monotone, all in the same direction, over its
own length.  Only a call that fails looks further, for the row to name."""
import torch

from . import dispatch as D

_REFUSED = "options['per_trajectory'] refused: "


class RowsTimes(object):
    """t: [batch, T] float64 on the state's device, increasing rows (the sign of a decreasing call is taken out, misc._check_inputs);
    lengths: [batch] int32 there, or None (every row T); rtol / atol: [batch] float64 there, or None (the scalar goes to the handle);
    rtol0 / atol0: what the handle is created with (a placeholder where the row's own value replaces it in the kernel)."""
    __slots__ = ('t', 'lengths', 'rtol', 'atol', 'rtol0', 'atol0', 'decreasing', 'T')


def shapes(y0, t, rtol, atol, options, names=('rtol', 'atol')):
    """(wanted, refusal) from shapes and dtypes alone - no tensor is read."""
    y = y0[0] if isinstance(y0, (tuple, list)) and len(y0) == 1 else y0
    lengths = (options or {}).get('t_lengths')
    t_shape, r_shape, a_shape = D._shape_of(t), D._shape_of(rtol), D._shape_of(atol)
    if isinstance(t, (list, tuple)):                         # (times given as nested lists)
        t_shape = tuple(torch.as_tensor(t).shape)
    if not D.rows_t_wanted(t_shape, r_shape, a_shape, lengths is not None):
        return False, ''
    if not isinstance(y, torch.Tensor):
        return True, 'per-row times, lengths or tolerances need one [batch, dim] state tensor'
    l_shape = None if lengths is None else D._shape_of(lengths) or ()
    l_int = lengths is None or (isinstance(lengths, torch.Tensor) and not lengths.is_floating_point() and not lengths.is_complex()
                                and lengths.dtype != torch.bool)
    return True, D.rows_t_refusal(tuple(y.shape), t_shape if t_shape is not None else (1,), l_shape, l_int, r_shape, a_shape, names)


def _per_row(x, batch, device):
    """(tensor [batch] float64 on `device` | None, the scalar for the handle)."""
    shape = D._shape_of(x)
    if shape is None or len(shape) == 0:
        return None, x
    return torch.as_tensor(x).detach().to(device=device, dtype=torch.float64).contiguous(), None


def prepare(y0, t, rtol, atol, options, prefix=_REFUSED):
    """(RowsTimes | None for the shared-t call, options without 't_lengths').  ValueError: a refusal; AssertionError: a row that is not
    strictly monotone (the reference's text, with the row); TypeError: `t` that is not floating point (misc._check_inputs).  prefix: what
    a refusal's message starts with (the fixed-grid route of fixed_rows.py has its own; the default leaves the texts as they are)."""
    opts = dict(options or {})
    wanted, why = shapes(y0, t, rtol, atol, opts)
    if not wanted:
        return None, options
    if why:
        raise ValueError(prefix + why)
    lengths = opts.pop('t_lengths', None)
    y = y0[0] if isinstance(y0, (tuple, list)) else y0
    batch, dev = int(y.shape[0]), y.device
    t = torch.as_tensor(t)
    if not torch.is_floating_point(t):
        raise TypeError('`t` must be a floating point Tensor but is a {}'.format(t.dtype))
    t = t.detach().to(device=dev, dtype=torch.float64)
    if t.dim() == 1:                                         # (per-row tolerances with the shared times: every row gets its copy)
        t = t[None, :].expand(batch, t.shape[0])
    T = int(t.shape[1])
    if T < 1:
        raise ValueError(prefix + '`t` without a time')
    rt = RowsTimes()
    rt.T = T
    rt.lengths = None if lengths is None else lengths.detach().to(device=dev, dtype=torch.int32).contiguous()
    # ---- values: one host read ----
    up, down = t[:, 1:] > t[:, :-1], t[:, 1:] < t[:, :-1]
    flags = [up, down]
    if rt.lengths is not None:
        skip = torch.arange(1, T, device=dev)[None, :] >= rt.lengths[:, None]     # [batch, T - 1]: pairs of times beyond the row's length
        up, down = up | skip, down | skip
        flags = [up, down, (rt.lengths >= 1) & (rt.lengths <= T)]
    all_up, all_down, len_ok = (torch.stack([x.all() for x in flags]).tolist() + [True])[:3]       # (the one host read)
    if not len_ok:
        bad = torch.nonzero((rt.lengths < 1) | (rt.lengths > T)).flatten().tolist()
        raise ValueError(prefix + "options['t_lengths'] must lie in 1 .. T = %d: row %d has %d (%d rows out of range)"
                         % (T, bad[0], int(rt.lengths[bad[0]]), len(bad)))
    if not (all_up or all_down):
        row_up, row_down = up.all(dim=1), down.all(dim=1)
        crooked = torch.nonzero(~(row_up | row_down)).flatten().tolist()
        if crooked:
            raise AssertionError('t must be strictly increasing or decrasing [per_trajectory: row %d of `t` is neither over its own length; '
                                 '%d such rows]' % (crooked[0], len(crooked)))      # misc.py:159 (sic)
        first_down = int(torch.nonzero(~row_up).flatten()[0])
        first_up = int(torch.nonzero(~row_down).flatten()[0])
        raise ValueError(prefix + 'rows of `t` that run in different directions (row %d increases, row %d decreases): the sign of a '
                         'decreasing call goes to the right-hand side once, for every row - call once per direction' % (first_up, first_down))
    rt.decreasing = not all_up
    rt.t = (-t if rt.decreasing else t).contiguous()
    rt.rtol, rt.rtol0 = _per_row(rtol, batch, dev)
    rt.atol, rt.atol0 = _per_row(atol, batch, dev)
    if rt.rtol is not None:
        rt.rtol0 = D.ROWS_T_RTOL0                            # (never read: the kernel takes the row's own)
    if rt.atol is not None:
        rt.atol0 = D.ROWS_T_ATOL0
    return rt, opts
