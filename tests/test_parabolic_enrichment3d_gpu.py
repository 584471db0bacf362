"""Online enrichment of the parabolic reduced model on the 3D / P2 path on the GPU: the corrector trajectories of
``lrbms3_local_correction_euler`` against the CPU reference tests/parabolic_enrichment3d_ref.py (sparse LU on the oracle's
neighbourhood systems, validated in tests/test_parabolic_enrichment3d_host.py), ``ParabolicLRBMSReductor3D.enrich_local_batch``,
``reduce(touched=)``, ``estimate(decompose=True)`` and the ``AdaptiveEnrichment`` loop against its CPU replay.

Sizes.  interior_3x3x3: n_T = 6 (one partial element chunk), every slot pattern from the 4-slot corners to the 7-slot centre;
aniso_2x2x1: n_T = 48, two element chunks per subdomain; kc_3x1x2: padded side tables; q3_2x1x2: Q = 3; cfg5_template: the
template of config 5 (n_T = 384, 16 chunks) with nt = 2.  Bound of the trajectories: 1e-8 of the largest step, the tolerance of
tests/test_enrichment3d_gpu.py for an iterative solve at rtol 1e-12 against a direct one."""
import ctypes
import functools

import numpy as np
import pytest

import common3d as c3
import parabolic_enrichment3d_ref as ref
from parabolic3d_ref import ParabolicReduced3D

pytestmark = pytest.mark.gpu

T = ref.LOOP['T']
PARTS = ('local_eta_nc', 'local_eta_r', 'local_eta_df', 'time_residual', 'time_deriv_nc')
E_INVALID, E_NOT_CONVERGED = -1, -4


def problem_dict(p, thetas=None):
    return {'grid': p['grid'], 'lambda': {'functions': p['lambdas'], 'coefficients': p['thetas'] if thetas is None else thetas},
            'lambda_bar': p['lambda_bar'], 'lambda_hat': p['lambda_hat'], 'f': p['f'], 'mu_bar': p['mu_bar'], 'mu_hat': p['mu_hat']}


@functools.lru_cache(maxsize=None)
def case(name, nt):
    """(problem, oracle, parabolic discretization with the corrector data) of a common3d problem, built once per module."""
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import discretize
    p = c3.make_problem(name)
    d, _ = discretize(problem_dict(p), T, nt, online_enrichment=True)
    return p, c3.oracle_of(p), d


def _check_trajectories(name, nt, K):
    p, o, d = case(name, nt)
    eng, mu, rtol = d.engine, p['mu'], 1e-12
    every = list(range(o.S))
    if K == 1:
        corr, info = d.solve_for_local_correction_trajectories(every, mu, rtol=rtol, return_info=True)
        want = ref.corrector_trajectories(o, every, mu, T / nt, nt)
        zero = 0
    else:
        b_K, phi = ref.switching_source(o, nt)
        zero = int(np.count_nonzero(~phi[1:].any(axis=1)))
        assert 1 <= zero < nt
        corr, info = eng.local_corrections_euler(d.theta(mu), T / nt, nt, every, b_K=eng.ctx.from_numpy(b_K), phi=phi, rtol=rtol)
        want = ref.corrector_trajectories(o, every, mu, T / nt, nt, phi, b_K)
    corr = corr.cpu().numpy()
    assert corr.shape == (o.S, o.n, nt) and info.shape == (o.S, 2)
    print(name, 'K', K, 'iterations', info[:, 0].min(), info[:, 0].max(), 'worst ratio', info[:, 1].max())
    for ii in every:
        err = ref.max_rel(corr[ii], want[ii])
        print(name, 'K', K, ii, 'relative error', err)
        assert err < ref.CORR_TOL, (ii, err)
    assert np.all(corr[:, :, :zero] == 0.0)                # a zero right-hand side from a zero state: exactly zero, 0 iterations
    assert np.all(info[:, 1] <= rtol) and np.all(info[:, 0] >= nt - zero)


@pytest.mark.parametrize('K', [1, 2])
@pytest.mark.parametrize('name', ['interior_3x3x3', 'aniso_2x2x1', 'kc_3x1x2', 'q3_2x1x2'])
def test_trajectories_of_every_subdomain_in_one_call_match_the_sparse_lu(name, K):
    _check_trajectories(name, 3 if K == 1 else 4, K)


def test_trajectories_on_the_template_of_config_5():
    p, o, d = case('cfg5_template', 2)
    assert d.engine.t.n == 3840
    _check_trajectories('cfg5_template', 2, 1)


def test_a_trajectory_does_not_depend_on_the_batch_the_work_buffer_or_the_call():
    """Bitwise: the centre (all 7 slots) and a corner (4 slots) of the 3 x 3 x 3 grid alone, with all 27, and with all 27 in reversed
    order; a NaN-filled work buffer; a repeated call."""
    import torch
    p, o, d = case('interior_3x3x3', 3)
    mu = p['mu']
    every = list(range(27))
    all_c, all_i = d.solve_for_local_correction_trajectories(every, mu, return_info=True)
    rev_c, rev_i = d.solve_for_local_correction_trajectories(every[::-1], mu, return_info=True)
    for ii in (13, 0):
        assert len(p['grid'].neighborhood_of(ii)) == (7 if ii == 13 else 4)
        one_c, one_i = d.solve_for_local_correction_trajectories([ii], mu, return_info=True)
        assert torch.equal(one_c[0], all_c[ii]) and torch.equal(one_c[0], rev_c[26 - ii])
        assert np.array_equal(one_i[0], all_i[ii]) and np.array_equal(one_i[0], rev_i[26 - ii])
    assert len(set(all_i[:, 0])) > 1            # the problems do stop at different iterations
    again_c, again_i = d.solve_for_local_correction_trajectories(every, mu, return_info=True)
    assert torch.equal(again_c, all_c) and np.array_equal(again_i, all_i)
    eng = d.engine
    ops, marked = eng.ops, [5, 0, 13]
    size = eng.ctx.local_correction_euler_work_size(len(marked), 3)
    assert size == eng.ctx.local_correction_work_size(len(marked)) + 3 * len(marked) * eng.t.n
    out = []
    for fill in (float('nan'), 0.0):
        work = torch.full((size,), fill, dtype=torch.float64, device='cuda')
        out.append(eng.ctx.local_correction_euler(eng.Q, d.theta(mu), T / 3, 3, marked, ops['A_diag'], ops['A_cpl'], ops['D_corr'],
                                                  ops['b'][None].contiguous(), np.ones((4, 1)), rtol=1e-12, work=work))
    assert torch.equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert bool(torch.isfinite(out[0][0]).all())
    for k, ii in enumerate(marked):
        assert torch.equal(out[0][0][k], all_c[ii])


def test_one_huge_step_is_the_stationary_corrector_and_the_stationary_export_keeps_its_bits():
    import torch
    p, o, d = case(ref.LIMIT_GRID, 3)
    eng, mu = d.engine, p['mu']
    every = list(range(o.S))
    stat, stat_i = d.solve_for_local_corrections(every, mu, return_info=True)
    one, _ = eng.local_corrections_euler(d.theta(mu), 1e6 * T, 1, every, rtol=1e-12)
    stat2, stat2_i = d.solve_for_local_corrections(every, mu, return_info=True)
    assert torch.equal(stat, stat2) and np.array_equal(stat_i, stat2_i)
    sh, oh = stat.cpu().numpy(), one.cpu().numpy()[:, :, 0]
    for ii in every:
        gap = float(np.abs(oh[ii] - sh[ii]).max() / np.abs(sh[ii]).max())
        print(ii, 'gap to the stationary corrector', gap)
        assert gap < ref.CORR_TOL + ref.LIMIT_GAP


def _raw_call(d, **over):
    """lrbms3_local_correction_euler through ctypes with a valid argument set varied by ``over``: (rc, message, corr, info)."""
    import torch
    from pylrbms_amd._native3d import _P_DBL, _P_I32
    eng = d.engine
    ctx, ops = eng.ctx, eng.ops
    vp = ctypes.c_void_p
    a = dict(Q=eng.Q, K=1, theta=np.full(8, 0.5), dt=0.01, nt=3, marked=[0, 1], rtol=1e-10, max_iter=200, b_K=True, phi=True, null=())
    a.update(over)
    mk = np.ascontiguousarray(a['marked'], dtype=np.int32)
    nmark = len(mk)
    corr = torch.full((max(nmark, 1), eng.t.n, max(a['nt'], 1)), -7.0, dtype=torch.float64, device='cuda')
    work = ctx.empty(ctx.local_correction_euler_work_size(max(nmark, 1), max(a['nt'], 1)))
    b_K = ops['b'][None].contiguous()
    phi = ctx.from_numpy(np.ones((max(a['nt'], 1) + 1, 1)))
    info = np.full((max(nmark, 1), 2), -7.0)
    def ptr(name, t):
        return vp(None if name in a['null'] else t.data_ptr())
    rc = ctx.lib.lrbms3_local_correction_euler(
        ctx.handle, a['Q'], a['K'], None if 'theta' in a['null'] else a['theta'].ctypes.data_as(_P_DBL), float(a['dt']), a['nt'], nmark,
        None if 'marked' in a['null'] else mk.ctypes.data_as(_P_I32), ptr('A_diag', ops['A_diag']), ptr('A_cpl', ops['A_cpl']),
        ptr('D_corr', ops['D_corr']), vp(b_K.data_ptr() if a['b_K'] else None), vp(phi.data_ptr() if a['phi'] else None),
        ptr('work', work), ptr('corr', corr), a['rtol'], a['max_iter'], info.ctypes.data_as(_P_DBL), ctx._stream())
    torch.cuda.synchronize()
    msg = ctx._fn('last_error')(ctx.handle)
    return rc, (msg.decode() if msg else ''), corr.cpu().numpy(), info


def test_error_paths_are_errors_not_faults():
    from pylrbms_amd._native import NativeError
    p, o, d = case('aniso_2x2x1', 3)
    rc, msg, corr, info = _raw_call(d)
    assert rc == 0 and not (corr == -7.0).any()                          # the call the refusals below vary is a valid one
    cases = {'nmark < 1': dict(marked=[]), 'Q = 0': dict(Q=0), 'Q = 9': dict(Q=9), 'K = 0': dict(K=0), 'K = 65': dict(K=65),
             'nt = 0': dict(nt=0), 'dt = 0': dict(dt=0.0), 'dt < 0': dict(dt=-0.01), 'dt = nan': dict(dt=float('nan')),
             'marked = S': dict(marked=[0, o.S]), 'marked < 0': dict(marked=[-1]), 'marked twice': dict(marked=[1, 1]),
             'max_iter = 0': dict(max_iter=0), 'rtol = 0': dict(rtol=0.0), 'b_K null': dict(b_K=False), 'phi null': dict(phi=False)}
    cases.update({name + ' null': dict(null=(name,)) for name in ('theta', 'marked', 'A_diag', 'A_cpl', 'D_corr', 'work', 'corr')})
    for name, over in cases.items():
        rc, msg, corr, info = _raw_call(d, **over)
        print(name, rc, msg)
        assert rc == E_INVALID and 'local_correction_euler' in msg, name
        assert (corr == -7.0).all() and (info == -7.0).all(), name         # refused before any launch
    # a step that runs out of iterations: an error return that names the subdomain and the step, info filled, the trajectory ends
    # at the iterate as it stands and its later columns repeat it
    rc, msg, corr, info = _raw_call(d, marked=[2, 0], max_iter=1, rtol=1e-12)
    print(rc, msg, info)
    assert rc == E_NOT_CONVERGED and 'subdomain 2, step 1' in msg and 'not converged' in msg
    assert np.all(info[:, 0] == 1.0) and np.all(info[:, 1] > 1e-12) and np.all(np.isfinite(corr))
    assert np.abs(corr[:, :, 0]).max() > 0.0
    assert np.array_equal(corr[:, :, 1], corr[:, :, 0]) and np.array_equal(corr[:, :, 2], corr[:, :, 0])
    with pytest.raises(NativeError, match=r'\(-4\).*subdomain'):
        d.solve_for_local_correction_trajectories([0, 1], p['mu'], max_iter=1)


def test_host_refusals_come_before_any_device_work():
    import torch
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D, discretize
    p, o, d = case('aniso_2x2x1', 3)
    mu = p['mu']
    # the default discretize carries no corrector data
    d0, _ = discretize(problem_dict(p), T, 3)
    assert 'D_corr' not in d0.engine.ops and 'D_corr' in d.engine.ops
    red0 = ParabolicLRBMSReductor3D(d0)
    for call in (lambda: d0.solve_for_local_correction_trajectories([0], mu), lambda: red0.enrich_local_batch([0], None, mu),
                 lambda: red0.enrich_local_batch([], None, mu), lambda: red0.enrich_local(0, None, mu)):
        with pytest.raises(NotImplementedError, match='online_enrichment=True'):
            call()
    # diffusion coefficients of the time
    dtv, _ = discretize(problem_dict(p, thetas=[lambda mu_: 1.0, lambda mu_, t: mu_ * (1.0 + t)]), T, 3, online_enrichment=True)
    assert dtv._tv
    with pytest.raises(NotImplementedError, match='depend on time'):
        dtv.solve_for_local_correction_trajectories([0], mu)
    redtv = ParabolicLRBMSReductor3D(dtv)
    with pytest.raises(NotImplementedError, match='depend on time'):
        redtv.enrich_local_batch([0], None, mu)
    with pytest.raises(NotImplementedError, match='depend on time'):
        redtv.reduce().estimate(None, mu, decompose=True)
    # non-zero initial data
    zero = d.initial_data
    try:
        d.initial_data = torch.ones_like(zero)
        with pytest.raises(NotImplementedError, match='initial data'):
            d.solve_for_local_correction_trajectories([0], mu)
    finally:
        d.initial_data = zero
    assert tuple(d.solve_for_local_correction_trajectories([0], mu).shape) == (1, o.n, 3)


def _model_arrays(rd):
    out = {k: v for k, v in rd.out.items() if v is not None}
    out['M_red'] = rd.M_red
    return out


def test_enrich_local_batch_and_the_ragged_parabolic_model():
    import torch
    import local_pod_ref as pod
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D
    from pylrbms_amd.reductor import ExtensionError
    nt = 4
    p, o, d = case('aniso_2x2x1', nt)
    S, mu0, mu1 = o.S, 0.9, 0.15
    P = ref.local_products(o)
    red = ParabolicLRBMSReductor3D(d)
    U0 = d.solve(mu0)
    red.extend_basis(U0[:, :, [nt]])
    for ii in (1, 3):                                                     # ragged: local sizes 2, 3, 2, 3
        red.extend_basis_local(ii, U0[ii, :, 1])
    assert red.local_sizes() == [2, 3, 2, 3] and red.basis_size() == 3
    red.reserve(6)
    rd0 = red.reduce()
    assert rd0.N == 6
    V_before = red.bases.clone()
    orth0 = pod.orthonormality(V_before.cpu().numpy(), red.local_sizes(), P)

    marked = [0, 1]
    grown = red.enrich_local_batch(marked, None, mu1, pod_modes=2)
    sizes = red.local_sizes()
    assert grown == marked and [sizes[2], sizes[3]] == [2, 3] and red.basis_size() == 6
    assert 2 < sizes[0] <= 4 and 3 < sizes[1] <= 5
    V = red.bases
    for s in range(S):
        if s in marked:                                                   # old columns bitwise, room behind the new ones still zero
            old = [2, 3, 2, 3][s]
            assert torch.equal(V[s, :, :old], V_before[s, :, :old]) and bool((V[s, :, sizes[s]:] == 0).all())
        else:
            assert torch.equal(V[s], V_before[s])
    Vh = V.cpu().numpy()
    orth = pod.orthonormality(Vh, sizes, P)
    print('orthonormality before / after: {:.2e} / {:.2e}'.format(orth0, orth))
    assert orth <= max(10 * orth0, 1e-12)
    # the new vectors span the leading POD modes of the corrector trajectory: far less of it is left outside the grown basis
    traj = ref.corrector_trajectories(o, marked, mu1, T / nt, nt)
    for m, s in enumerate(marked):
        def left(W):
            R = traj[m] - W @ (W.T @ (P[s] @ traj[m]))
            return float(np.sqrt(np.trace(R.T @ P[s] @ R)))
        assert left(Vh[s][:, :sizes[s]]) < 0.2 * left(Vh[s][:, :[2, 3][m]])
    # a single subdomain through the reference API; what is in the span by now adds nothing and says so
    red.enrich_local(3, None, mu1)
    assert red.local_sizes()[3] == 4
    assert red.enrich_local_batch([0], None, mu1, pod_modes=1, rtol=0.5) == []
    with pytest.raises(ExtensionError):
        red.enrich_local(0, None, mu1, rtol=0.5)
    sizes = red.local_sizes()

    # reduce(touched=) in the reserved slab equals a whole pass, bit for bit
    rd1 = red.reduce(touched=marked + [3])
    assert red.last_reduce_info['incremental'] and rd1.out['B_sys'].data_ptr() == rd0.out['B_sys'].data_ptr()
    inc = {k: v.clone() for k, v in _model_arrays(rd1).items()}
    rd2 = red.reduce()
    assert not red.last_reduce_info['incremental']
    whole = _model_arrays(rd2)
    assert set(inc) == set(whole) and 'B_sys' in inc and 'M_red' in inc
    for k in inc:
        assert torch.equal(inc[k], whole[k]), k

    # the ragged model against the NumPy parabolic reference on the compact bases (tolerances of tests/test_parabolic3d_gpu.py)
    u = rd2.solve(mu1)
    uh = u.cpu().numpy()                                                  # [nt + 1, S, N]
    Vh = red.bases.cpu().numpy()
    opr = ParabolicReduced3D(o, [Vh[s][:, :sizes[s]] for s in range(S)], T, nt)
    u_o = opr.solve(mu1)
    assert c3.rel(np.concatenate([uh[:, s, :sizes[s]] for s in range(S)], axis=1), u_o) < 1e-8
    for s in range(S):
        assert (uh[:, s, sizes[s]:] == 0.0).all()                         # padded unknowns stay exactly zero
    est, parts = rd2.estimate(u, mu1)
    est_o, parts_o = opr.estimate(u_o, mu1)
    for nm, a, b in zip(PARTS, parts, parts_o):
        print('reduced', nm, c3.rel(a, b))
        assert c3.rel(a, b) < 1e-6, nm
    assert abs(est - est_o) < 1e-6 * est_o
    # decompose=True: the same value and parts, the indicators are the 2D expression on those parts
    est_d, parts_d, ind = rd2.estimate(u, mu1, decompose=True)
    assert est_d == est and all(np.array_equal(a, b) for a, b in zip(parts_d, parts))
    a_bar, g_bar, a_hat = o.alpha(mu1, o.mu_bar), o.gamma(mu1, o.mu_bar), o.alpha(mu1, o.mu_hat)
    nc, r, df, _, tdn = parts_d
    want = ((2.0 / a_bar) * (g_bar * nc ** 2 + (r + df) ** 2 / a_hat)).sum(axis=1) + (tdn ** 2).sum(axis=1)
    assert ind.shape == (S,) and (ind >= 0).all() and c3.rel(ind, want) < 1e-12


def test_the_slab_grows_to_an_even_width_and_only_when_something_is_gained():
    """No ``reserve`` in front: a round that needs more columns than the slab has widens it to an even width (the wide-load form
    of the pass takes even N), a round that gains nothing leaves the width alone and the next ``reduce(touched=)`` is incremental."""
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import EnrichingParabolicLRBMSReductor3D, ParabolicLRBMSReductor3D
    nt = 4
    p, o, d = case('aniso_2x2x1', nt)
    mu0, mu1 = 0.9, 0.15
    red = ParabolicLRBMSReductor3D(d)
    assert type(red) is EnrichingParabolicLRBMSReductor3D
    red.extend_basis(d.solve(mu0)[:, :, [nt]])
    assert red.local_sizes() == [2] * o.S and red.basis_size() == 2
    assert red.enrich_local_batch([0], None, mu1, pod_modes=2) == [0]
    assert red.local_sizes() == [4, 2, 2, 2] and red.basis_size() == 4
    assert red.enrich_local_batch([0], None, mu1, pod_modes=1) == [0]
    assert red.local_sizes() == [5, 2, 2, 2] and red.basis_size() == 6          # five vectors, an even slab
    red.reduce()
    assert red.enrich_local_batch([0], None, mu1, pod_modes=2, rtol=0.5) == []    # nothing above the threshold: the slab is as it was
    assert red.basis_size() == 6
    red.reduce(touched=[0])
    assert red.last_reduce_info['incremental']


def test_adaptive_enrichment_loop_against_its_cpu_replay():
    """``AdaptiveEnrichment`` on the parabolic 3 x 3 x 3 model from the start of the CPU replay (the constant and the final state of
    one trajectory at mu0, handed in as ready-made bases), every subdomain marked in every round (theta = 1.0), pod_modes = 2, three
    rounds.

    Sizes per subdomain 2, 4, 5, 5 (the replay's); DESIGN.md 9.19 has eta and the error per round.  eta need not fall from round to round (as in 2D: its residual part reacts to the kinks the zero-Dirichlet
    correctors have at the edge of their neighbourhood)."""
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D
    from pylrbms_amd.online_enrichment import AdaptiveEnrichment
    c = ref.LOOP
    r = ref.replay()
    p, o, d = case(c['name'], c['nt'])
    S, mu = o.S, c['mu']
    red = ParabolicLRBMSReductor3D(d, bases=[b.copy() for b in r['start']])
    assert red.local_sizes() == r['sizes'][0]
    Uf = d.solve(mu)                                                      # [S, n, nt + 1]
    assert c3.rel(Uf.permute(2, 0, 1).cpu().numpy(), r['U_fom']) < 1e-8
    history, marks = [], []
    enrich = red.enrich_local_batch

    def recording(subdomains, U_, mu_, **kw):
        marks.append((list(subdomains), kw))
        return enrich(subdomains, U_, mu_, **kw)
    red.enrich_local_batch = recording

    def callback(rd_, U_, mu_, info):
        err = float((red.reconstruct(U_) - Uf).norm() / Uf.norm())
        history.append(dict(info, error=err))
    loop = AdaptiveEnrichment(problem_dict(p), d, d.solution_space, red, red.reduce(), target_error=0.0, marking_doerfler_theta=1.0,
                              marking_max_age=10, pod_modes=c['pod_modes'])
    U, rd, red_out = loop.solve(mu, enrichment_steps=c['rounds'], callback=callback)
    print('eta per round:', [h['eta'] for h in history], 'error per round:', [h['error'] for h in history],
          'replay:', r['errors'], 'sizes:', [sorted(set(h['local RB sizes'])) for h in history])
    assert red_out is red and len(history) == c['rounds'] + 1 and len(marks) == c['rounds']
    for k, h in enumerate(history):
        assert h['local RB sizes'] == r['sizes'][k], k                    # the sizes of the CPU replay, round by round
        assert h['global RB size'] == sum(h['local RB sizes'])
    for k, (marked, kw) in enumerate(marks):
        assert kw == {'pod_modes': c['pod_modes']} and sorted(marked) == list(range(S))
    assert history[-1]['error'] < history[0]['error']
    reserve = 2 + c['rounds'] * c['pod_modes']
    assert red.basis_size() == min(reserve + (reserve & 1), 64 // d.Q)
    assert red.last_reduce_info['incremental']                            # the later rounds re-projected in place
