"""Times the parabolic path with a time-dependent affine source on config 3's problem (T = 0.05, nt = 10, mu = 0.5): full-order and
reduced trajectories through the source entry points (lrbms_fom_implicit_euler_src / lrbms_reduced_implicit_euler_src) with
K = 1, phi = 1 (against the existing entry points on the same data) and with K = 2 and a switching phi, plus
lrbms_project_sources and lrbms_reduced_source_terms with bytes moved / time against 6.3 TB/s.
usage: parabolic_source_time.py [PX PY N NT]   (default: 32 32 40 10, config 3)"""
import sys, time
sys.path.insert(0, '.')
import numpy as np
import torch
from pylrbms_amd import multiscale_problem
from pylrbms_amd.discretize_parabolic_block_swipdg import discretize
from pylrbms_amd.functions import make_expression_function_1x1
from pylrbms_amd.parameters import ExpressionParameterFunctional
from pylrbms_amd.reductor import ParabolicLRBMSReductor

px, py, N, nt = (int(a) for a in (sys.argv[1:5] if len(sys.argv) > 4 else (32, 32, 40, 10)))
T = 0.05
HBM = 6.3e12


def timed(fn, reps=3):
    fn()
    best = 1e9
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(); best = min(best, time.perf_counter() - t0)
    return out, best


p = multiscale_problem.init_grid_and_problem({'num_subdomains': [px, py], 'coarse_per_subdomain': 4})
d1, _ = discretize(p, T, nt)                         # one component, coefficient 1: the existing entry points
f = p['f']
# a second component and a coefficient that switches inside [0, T]: sin(2 pi t / T') > 0 with T' = T / 2
g = make_expression_function_1x1(None, 'x', 'cos(pi*x[0])', order=2, name='g')
p2 = dict(p, f={'functions': [f, g], 'coefficients': [1.0, ExpressionParameterFunctional('sin(2 * pi * _t / {}) > 0'.format(T / 2),
                                                                                          {'_t': ()})]})
d2, _ = discretize(p2, T, nt)
mu = d1.parse_parameter(0.5)
eng, c = d1.engine, d1.engine.ctx
theta, dt = d1.theta(mu), T / nt
ones = torch.ones(nt + 1, 1, dtype=torch.float64, device=eng.b.device)
bK1 = eng.b[None].contiguous()
print('S', eng.S, 'dofs', eng.S * eng.t.n, 'nt', nt, 'N', N)
(U_old, i_old), t_old = timed(lambda: c.fom_implicit_euler(theta, dt, nt, eng.A_diag, eng.A_cpl, eng.b))
(U_new, i_new), t_new = timed(lambda: c.fom_implicit_euler_src(theta, dt, nt, eng.A_diag, eng.A_cpl, bK1, ones))
print('FOM trajectory K=1  existing s {:.4f}  _src s {:.4f}  ratio {:.4f}  equal {}  its {} / {}'.format(
    t_old, t_new, t_new / t_old, bool(torch.equal(U_old, U_new)), i_old['iterations'], i_new['iterations']))
U2, t2 = timed(lambda: d2.solve(mu))
print('FOM trajectory K=2 switching  s {:.4f}  steps/s {:.1f}  phi[:,1] {}  info {}'.format(
    t2, nt / t2, d2.source_coefficients(mu)[:, 1].tolist(), d2.last_solve_info))

rng = np.random.default_rng(0)
red = {}
for name, d, U in (('K=1', d1, U_old), ('K=2', d2, U2.tensor.permute(2, 0, 1))):
    r = ParabolicLRBMSReductor(d, order=0)
    Ut = U.permute(1, 2, 0).contiguous()
    from pylrbms_amd.vectorarrays import BlockVectorArray
    r.extend_basis(BlockVectorArray(Ut[:, :, 1:], d.solution_space))
    while r.basis_size() < N:
        R = d.solution_space.from_data(rng.standard_normal((1, eng.S * eng.t.n)), d.engine.ctx)
        r.extend_basis(R)
    red[name] = (r, r.reduce())
r1, rd1 = red['K=1']
rK = rd1.rhs_red[None].contiguous()
(u_old, _), t_old = timed(lambda: c.reduced_implicit_euler(theta, dt, nt, rd1.B_sys, rd1.M_red, rd1.rhs_red))
(u_new, _), t_new = timed(lambda: c.reduced_implicit_euler_src(theta, dt, nt, rd1.B_sys, rd1.M_red, rK, ones))
print('reduced trajectory K=1  existing s {:.5f}  _src s {:.5f}  ratio {:.4f}  equal {}'.format(
    t_old, t_new, t_new / t_old, bool(torch.equal(u_old, u_new))))
r2, rd2 = red['K=2']
u2, t2 = timed(lambda: rd2.solve(mu))
print('reduced trajectory K=2 switching  s {:.5f}  steps/s {:.1f}'.format(t2, nt / t2))

# the two estimator kernels on the K = 2 reduced model
N2 = rd2.N
V = r2._V.contiguous()
D = c.div_apply(c.flux_reconstruct(eng.F, V), mode=0)
bK = d2._src['b_K']
K, S, n, nT, Q = bK.shape[0], eng.S, eng.t.n, eng.t.n_T, eng.Q
C = 5 * Q * N2
_, t = timed(lambda: c.project_sources(Q, bK, V, D), reps=10)
nbytes = 8 * (S * n * N2 + S * nT * C + K * S * n + K * S * (N2 + C))
print('project_sources  K {} N {} C {}  us {:.1f}  bytes {:.3e}  TB/s {:.2f}  ({:.0f}% of 6.3)'.format(
    K, N2, C, t * 1e6, nbytes, nbytes / t / 1e12, 100 * nbytes / t / HBM))
L = nt + 1
uu = u2.tensor.contiguous()
phi = c.from_numpy(np.ascontiguousarray(d2.source_coefficients(mu)))
_, t = timed(lambda: c.reduced_source_terms(theta, phi, d2._src['F2'], rd2.r_fd_K, uu, eng.ceps, eng.hdiam), reps=10)
nbytes = 8 * (K * S * C + S * N2 * L + S * K * K + S * L)
print('reduced_source_terms  L {}  us {:.1f}  bytes (r_fd_K once) {:.3e}  TB/s {:.2f}  ({:.0f}% of 6.3)'.format(
    L, t * 1e6, nbytes, nbytes / t / 1e12, 100 * nbytes / t / HBM))
(est, _), t = timed(lambda: d2.estimate(U2, mu), reps=1)
print('FOM estimate K=2 s {:.4f} est {:.6e}'.format(t, est))
(est_r, _), t = timed(lambda: rd2.estimate(u2, mu))
print('reduced estimate K=2 s {:.5f} est {:.6e}'.format(t, est_r))
