"""GPU tests of the float64 MLP tile kernels (csrc/mi_ode_mlp64.h: k_persist_mlp64, k_mlp64, k_fixed_mlp64) where tests/test_gpu_mlp64.py
does not look: more than one tile per workgroup (the `tile_i += gridDim.x` loop, the weight stream carried from one tile into the next, a
one-row tile on a later trip, unequal trip counts in front of the grid-wide reduction), the edges of the geometry choice, the per-attempt
schedule for every instantiation, dense output, the fixed-grid options, saturated activations, the status bits and a handle reused
across batch sizes.  Inputs, their numpy restatement and the oracle runs are tests/mlp64_cases.py; tests/test_mlp64_cases_host.py checks on
the CPU that the inputs reject, decide every attempt clearly and put several output times into one step.

The reference is the numpy oracle (oracle/ode_numpy.py) on the same network: identical attempt / accept counts and the project's float64
bars for these kernels - 1e-9 absolute (1e-7 for dopri8) for the adaptive methods, 1e-11 on a fixed grid.  The oracle takes
options['step_size'] and options['eps'], so the fixed-grid options are held to it as well, not to the callable engine.
`odeint.plan` names the kernel, so the width-edge tests assert that (16, 17) and (17, 16) run on the float64 tile kernel."""
import numpy as np
import pytest
import torch

from tests import mlp64_cases as MC

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _solve(case, options=None, batch=None, model=None):
    """(solution on the host as numpy, last_stats) of a case on the device."""
    from tfdiffeq_amd import odeint
    ws, _, y0, t = MC.inputs(case, cus(), batch=batch)
    m = MC.to_mlp(ws, case.act, case.td, dev()) if model is None else model
    opts = dict(case.options or ())
    if case.first_step is not None:
        opts['first_step'] = case.first_step
    opts.update(options or {})
    kw = {} if case.method in ('euler', 'rk4') else dict(rtol=case.rtol, atol=case.atol)
    sol = odeint(m, torch.tensor(y0, device=dev()), torch.tensor(t), method=case.method, options=opts or None, **kw)
    return sol, dict(odeint.last_stats)


def _err(sol, ref):
    return float(np.abs(sol.cpu().numpy() - ref).max())


def _against_the_oracle(case, sol, st, whole=True):
    ref, rst, _ = MC.oracle(case, cus())
    if whole:
        assert st['n_launches'] == 1, st
    assert st['status'] == 0, st
    assert (st['n_attempts'], st['n_accepted']) == (rst.n_attempts, rst.n_accepted), (st, rst.n_attempts, rst.n_accepted)
    err = _err(sol, ref)
    print('%s: max|diff| %.3e (bar %.0e), %d attempts, %d accepted' % (case.name, err, MC.tol_of(case), rst.n_attempts, rst.n_accepted))
    assert err < MC.tol_of(case), err
    return ref


def _second_trip(case, sol, ref):
    """Rows [32 * cus:] on their own: the tiles a workgroup takes on its second and later trips."""
    B = MC.batch_of(case, cus())
    assert MC.n_tiles(B) > cus() and B % MC.TILE == 1, (B, cus())
    tail = _err(sol[:, MC.TILE * cus():], ref[:, MC.TILE * cus():])
    print('%s: rows [%d:] max|diff| %.3e' % (case.name, MC.TILE * cus(), tail))
    assert tail < MC.tol_of(case), 'second trip of the tile loop (rows [%d:]): %.3e' % (MC.TILE * cus(), tail)


# ---- a. more than one tile per workgroup, adaptive ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', MC.MULTI_ADAPTIVE, ids=MC.ids(MC.MULTI_ADAPTIVE))
def test_multi_tile_adaptive_against_the_oracle(case):
    sol, st = _solve(case)
    assert st['n_attempts'] > st['n_accepted'], st           # rejecting inputs (tests/test_mlp64_cases_host.py)
    ref = _against_the_oracle(case, sol, st)
    _second_trip(case, sol, ref)


# ---- b. more than one tile per workgroup, fixed grid -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', MC.MULTI_FIXED, ids=MC.ids(MC.MULTI_FIXED))
def test_multi_tile_fixed_grid_against_the_oracle(case):
    sol, st = _solve(case)
    assert st['n_launches'] == 1, st
    ref, _, _ = MC.oracle(case, cus())
    err = _err(sol, ref)
    print('%s: max|diff| %.3e (bar 1e-11)' % (case.name, err))
    assert err < 1e-11, err
    _second_trip(case, sol, ref)


# ---- c. width edges of the geometry choice ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', MC.WIDTH_EDGES, ids=MC.ids(MC.WIDTH_EDGES))
def test_width_edges_against_the_oracle(case):
    from tfdiffeq_amd import odeint
    sol, st = _solve(case)
    _against_the_oracle(case, sol, st)
    if (case.d, case.h) in ((16, 17), (17, 16)):             # one width past 16: the 64 x 128 float64 tile kernel, not the cooperative one
        ws, _, y0, t = MC.inputs(case)
        p = odeint.plan(MC.to_mlp(ws, case.act, case.td, dev()), torch.tensor(y0, device=dev()), torch.tensor(t), rtol=case.rtol, atol=case.atol,
                        method=case.method)
        assert p['engine'] == 'fused' and p['kernel'].startswith('k_persist_mlp64<') and 'Coop' not in p['kernel'], p
        assert st.get('route') == 'fused', st


# ---- d. the per-attempt schedule is the whole-call kernel, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize('case', MC.SCHEDULES, ids=MC.ids(MC.SCHEDULES))
def test_schedules_are_bit_identical(case):
    whole, wst = _solve(case)
    step, sst = _solve(case, {'fusion': 'step'})
    assert wst['n_launches'] == 1 and sst['n_launches'] > 1, (wst, sst)
    assert sst['status'] == 0 and wst['status'] == 0
    assert (sst['n_attempts'], sst['n_accepted']) == (wst['n_attempts'], wst['n_accepted']), (sst, wst)
    assert torch.equal(step, whole), float((step - whole).abs().max())
    if case.batch == 'B2':
        assert MC.n_tiles(MC.batch_of(case, cus())) > cus()
    _against_the_oracle(case, step, sst, whole=False)        # (with first_step: the oracle with the same first_step)


# ---- e. dense output: many output times inside one step --------------------------------------------------------------------------------------
@pytest.mark.parametrize('fusion', ['whole', 'step'])
@pytest.mark.parametrize('case', MC.DENSE, ids=MC.ids(MC.DENSE))
def test_dense_output_against_the_oracle(case, fusion):
    sol, st = _solve(case, {'fusion': fusion})
    assert sol.shape[0] == 40
    _against_the_oracle(case, sol, st, whole=(fusion == 'whole'))


# ---- f. fixed-grid options: a grid of its own (outputs strictly between its points), eps -------------------------------------------------------
@pytest.mark.parametrize('case', MC.FIXED_OPTIONS, ids=MC.ids(MC.FIXED_OPTIONS))
def test_fixed_grid_options_against_the_oracle(case):
    sol, st = _solve(case)
    assert st['n_launches'] == 1 and st.get('route') == 'fused', st
    ref, _, _ = MC.oracle(case, cus())
    err = _err(sol, ref)
    print('%s: max|diff| %.3e (bar 1e-11)' % (case.name, err))
    assert err < 1e-11, err


# ---- g. saturated activations, one Euler step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', ['tanh', 'relu', 'softplus'])
@pytest.mark.parametrize('d,h', [MC.G64, MC.G16])
def test_saturated_activations_one_euler_step(d, h, act):
    from tfdiffeq_amd import odeint
    ws, y0 = MC.saturated(d, h)
    ref = y0 + MC.np_f(ws, act, False)(0.0, y0)              # t = [0, 1]: y0 + 1.0 * f(0, y0)
    sol = odeint(MC.to_mlp(ws, act, False, dev()), torch.tensor(y0, device=dev()), torch.tensor([0., 1.]), method='euler')
    st = dict(odeint.last_stats)
    assert st['n_launches'] == 1 and st.get('route') == 'fused', st
    got = sol[1].cpu().numpy()
    assert np.isfinite(got).all()
    rel = float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())
    print('saturated %s %dx%d: max|diff| / max(1, |ref|) %.3e (bar 1e-11)' % (act, d, h, rel))
    assert rel < 1e-11, rel


# ---- h. status bits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fusion', ['whole', 'step'])
def test_status_bits_surface_as_the_reference_assertions(fusion):
    with pytest.raises(AssertionError, match='max_num_steps exceeded'):
        _solve(MC.STATUS, {'fusion': fusion, 'max_num_steps': 3})
    from tfdiffeq_amd import odeint
    ws, _, y0, t = MC.inputs(MC.STATUS)
    assert y0.shape[0] == 65
    y0[-1, 3] = np.nan                                       # the single row of the last tile
    m = MC.to_mlp(ws, MC.STATUS.act, MC.STATUS.td, dev())
    for opts in ({'fusion': fusion}, {'fusion': fusion, 'first_step': 0.01}):
        with pytest.raises(AssertionError, match='non-finite'):
            odeint(m, torch.tensor(y0, device=dev()), torch.tensor(t), rtol=MC.STATUS.rtol, atol=MC.STATUS.atol, method='dopri5', options=opts)


# ---- i. one handle, many batches --------------------------------------------------------------------------------------------------------------
def test_one_descriptor_across_batch_sizes_and_a_weight_update():
    case = MC.HANDLE
    assert MC.geometry(case.d, case.h) == (16, 16)
    ws, _, _, _ = MC.inputs(case)
    m = MC.to_mlp(ws, case.act, case.td, dev())
    first, st1 = _solve(case, model=m, batch=33)
    big, st2 = _solve(case, model=m, batch=MC.B2(cus()))
    again, st3 = _solve(case, model=m, batch=33)
    assert st1['n_launches'] == st2['n_launches'] == st3['n_launches'] == 1 and big.shape[1] == MC.B2(cus()) and MC.n_tiles(big.shape[1]) > cus()
    assert torch.equal(again, first)
    _against_the_oracle(case, first, st1)
    ref2, rst2, _ = MC.oracle(case, batch=MC.B2(cus()))
    assert st2['status'] == 0 and (st2['n_attempts'], st2['n_accepted']) == (rst2.n_attempts, rst2.n_accepted), (st2, rst2.n_attempts)
    assert _err(big, ref2) < 1e-9, _err(big, ref2)
    m.Ws[1].mul_(0.5)                                        # in place: the pack is refreshed at the 16 x 16 geometry too
    halved, _ = _solve(case, model=m, batch=33)
    ws2 = list(ws)
    ws2[2] = ws[2] * 0.5
    fresh, _ = _solve(case, model=MC.to_mlp(ws2, case.act, case.td, dev()), batch=33)
    assert torch.equal(halved, fresh)
    assert float((halved - first).abs().max()) > 1e-6
