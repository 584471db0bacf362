"""The CPU reference of the 3D parabolic corrector trajectories (tests/parabolic_enrichment3d_ref.py) checked on itself, the gap
figure the GPU limit test takes its tolerance from, the C surface of ``lrbms3_local_correction_euler`` and the CPU replay of the
enrichment loop of tests/test_parabolic_enrichment3d_gpu.py.  No GPU, no compute call."""
import ctypes
import os
import re

import numpy as np

import common3d as c3
import parabolic_enrichment3d_ref as ref
from parabolic3d_ref import Parabolic3D

NAMES = ('lrbms3_local_correction_euler', 'lrbms3_local_correction_euler_work_size')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_neighbourhood_that_is_the_whole_domain_gives_the_full_order_trajectory():
    """2 x 1 x 1: N(0) is the whole domain and no coupling face has exactly one side inside, so the corrector trajectory is
    ``Parabolic3D.solve`` restricted to subdomain 0 -- two code paths (rows / columns of the neighbourhood against the global
    system), one LU each."""
    p = c3.make_problem('wide_basis')
    o = c3.oracle_of(p)
    T, nt = 0.06, 3
    U = Parabolic3D(o, T, nt).solve(p['mu'])                             # [nt + 1, S, n]
    for ii in range(o.S):
        assert sorted(o.mesh.neighborhood_of(ii)) == [0, 1]
        x = ref.corrector_trajectory(o, ii, p['mu'], T / nt, nt)
        assert ref.max_rel(x, U[1:, ii]) < 1e-12
    assert ref.corrector_trajectories(o, [1, 0], p['mu'], T / nt, nt).shape == (2, o.n, nt)


def test_one_huge_step_approaches_the_stationary_corrector():
    """x_1 = (A + M / dt)^-1 b -> A^-1 b: the gap falls like 1 / dt, and at dt = 1e6 T -- the step of the GPU limit test, on its
    grid -- it is below the figure that test allows for it (measured here: 1.8e-7; LIMIT_GAP = 3e-7)."""
    p = c3.make_problem(ref.LIMIT_GRID)
    o = c3.oracle_of(p)
    T, marked = ref.LOOP['T'], list(range(o.S))
    gaps = [ref.stationary_limit_gap(o, marked, p['mu'], dt) for dt in (1e2 * T, 1e4 * T, 1e6 * T)]
    print('stationary limit gaps at dt = 1e2, 1e4, 1e6 T:', gaps)
    assert gaps[0] > gaps[1] > gaps[2]
    assert 50.0 < gaps[0] / gaps[1] < 200.0            # first order in 1 / dt
    assert gaps[2] < ref.LIMIT_GAP
    # ... while a step of the size the trajectories use is nowhere near the stationary corrector: the two problems differ
    assert ref.stationary_limit_gap(o, marked, p['mu'], T / ref.LOOP['nt']) > 0.1


def test_zero_rows_of_phi_and_linearity():
    p = c3.make_problem('aniso_2x2x1')
    o = c3.oracle_of(p)
    nt, dt, mu = 4, 0.01, p['mu']
    b_K, phi = ref.switching_source(o, nt)
    assert np.all(phi[1:3] == 0.0) and np.all(phi[3:] > 0.0)
    x = ref.corrector_trajectory(o, 2, mu, dt, nt, phi, b_K)
    assert np.abs(x[:2]).max() == 0.0 and np.abs(x[2]).max() > 0.0          # zero right-hand sides from a zero state
    phi2 = phi.copy()
    phi2[0] = -1.0                                                           # row 0 of phi is never read
    phi2[1:] *= 2.0
    assert np.allclose(ref.corrector_trajectory(o, 2, mu, dt, nt, phi2, b_K), 2.0 * x, rtol=1e-12, atol=0.0)
    one = ref.corrector_trajectory(o, 2, mu, dt, nt)
    assert np.array_equal(one, ref.corrector_trajectory(o, 2, mu, dt, nt, np.ones((nt + 1, 1)), o.b[None]))


def _declarations():
    text = open(os.path.join(ROOT, 'include', 'lrbms3d_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return {name: re.search(r'\b(int64_t|int)\s+' + name + r'\s*\(([^;]*?)\)\s*;', text, flags=re.S) for name in NAMES}


def test_the_new_symbols_are_declared_exported_and_bound():
    from pylrbms_amd import _native3d
    from pylrbms_amd._build import build_native
    lib = build_native()
    handle = ctypes.CDLL(lib)
    bound = _native3d.load_library(lib)
    for name, decl in _declarations().items():
        assert decl is not None, name + ' is not declared'
        assert hasattr(handle, name), name + ' is not exported'
        restype, argtypes = _native3d.SIGNATURES3[name]
        assert len(argtypes) == len(decl.group(2).split(',')), name
        assert restype is (_native3d.c_i64 if decl.group(1) == 'int64_t' else ctypes.c_int), name
        assert getattr(bound, name).argtypes == argtypes
    # the trajectory export takes what the stationary one takes plus K, dt, nt and the coefficient table
    assert len(_native3d.SIGNATURES3[NAMES[0]][1]) == len(_native3d.SIGNATURES3['lrbms3_local_correction_solve'][1]) + 4


def test_the_host_layers_reach_the_export():
    import inspect
    from pylrbms_amd import _native3d
    from pylrbms_amd import discretize_parabolic_block_swipdg_3d as par
    from pylrbms_amd.engine3d import Engine3D
    from pylrbms_amd.reductor import LocalBasisSlab, ParabolicLRBMSReductor
    assert callable(_native3d.Native3DContext.local_correction_euler) and callable(Engine3D.local_corrections_euler)
    assert callable(par.InstationaryDiscretization3D.solve_for_local_correction_trajectories)
    assert callable(par.InstationaryReducedDiscretization3D.local_indicators)
    # AdaptiveEnrichment probes ``reductor.reduce`` for ``touched``: the reductor of a discretization made with the keyword is the
    # subclass that has it, chosen in the constructor; the class itself keeps the whole re-reduction
    assert issubclass(par.EnrichingParabolicLRBMSReductor3D, par.ParabolicLRBMSReductor3D)
    assert 'touched' in inspect.signature(par.EnrichingParabolicLRBMSReductor3D.reduce).parameters
    assert 'touched' not in inspect.signature(par.ParabolicLRBMSReductor3D.reduce).parameters
    for flag, cls in ((True, par.EnrichingParabolicLRBMSReductor3D), (False, par.ParabolicLRBMSReductor3D)):
        d = type('D', (), {'online_enrichment': flag})()
        assert type(par.ParabolicLRBMSReductor3D.__new__(par.ParabolicLRBMSReductor3D, d)) is cls
    assert 'online_enrichment' in inspect.signature(par.discretize).parameters
    assert inspect.signature(par.discretize).parameters['online_enrichment'].default is False
    # one POD step for the 2D and the 3D reductor
    assert par.ParabolicLRBMSReductor3D._extend_marked_pod is LocalBasisSlab._extend_marked_pod
    assert ParabolicLRBMSReductor._extend_marked_pod is LocalBasisSlab._extend_marked_pod
    # the refusal without the keyword comes before anything else is read
    for call in (lambda: par.ParabolicLRBMSReductor3D.enrich_local_batch(None, [0], None, 0.5, pod_modes=2),
                 lambda: par.ParabolicLRBMSReductor3D.enrich_local(None, 0, None)):
        try:
            call()
        except NotImplementedError as exc:
            assert 'online_enrichment=True' in str(exc) and 'parabolic 3D path' in str(exc)
        else:
            raise AssertionError('no refusal')


def test_the_enrichment_loop_replayed_on_the_cpu():
    """The loop of the GPU test from LU trajectories, the NumPy local POD and the NumPy reduced model, every subdomain marked in
    every round.  The correctors depend on mu alone, so every round sees the same three snapshots per subdomain: round 1 takes
    their two leading modes, round 2 the third, round 3 finds nothing above the threshold.  Measured: sizes 2, 4, 5, 5 per
    subdomain, error against the full-order trajectory 7.29e-2, 3.28e-2, 3.18e-2, 3.18e-2, smallest factor between a singular
    value and the POD threshold 3.1e2."""
    r = ref.replay()
    S = r['oracle'].S
    print('sizes per round', [sorted(set(s)) for s in r['sizes']], 'errors', r['errors'], 'margin', r['margin'])
    assert r['sizes'][0] == [2] * S and all(len(s) == S for s in r['sizes'])
    for a, b in zip(r['sizes'], r['sizes'][1:]):
        assert all(0 <= y - x <= ref.LOOP['pod_modes'] for x, y in zip(a, b))
    assert sum(r['sizes'][1]) > sum(r['sizes'][0]) and sum(r['sizes'][-1]) > sum(r['sizes'][1])
    assert r['margin'] > 100.0                        # no singular value near the threshold: the sizes do not hinge on round-off
    assert r['errors'][-1] < r['errors'][0]
