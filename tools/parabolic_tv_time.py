"""Times the parabolic exports with a diffusion-coefficient row per step on config 3 -- 32 x 32 subdomains,
N = 40, Q = 2, the bench's problem and bases, T = 0.05, nt = 10, 64 parameters; theta_t: a smooth factor of the time times one
10x switch on the second coefficient between the steps 4 and 5 -- and writes profiles/parabolic_tv_time.txt.  Three legs, at the
level of the native context (the calls ``rd.solve_batch`` / ``rd.estimate_batch`` / ``d.solve_batch`` make):
  (a) lrbms_reduced_implicit_euler_batch_tv + lrbms_reduced_parabolic_estimate_batch_tv with the table;
  (b) the only route without them: nt chained lrbms_reduced_implicit_euler_batch calls with nt = 1 at row k + 1, slab k as U0;
  (c) the existing exports at the time mean of the table (a time-independent model), with the iteration counts of (a) and (c).
The same three legs for lrbms_fom_implicit_euler_batch(_tv) at 16 parameters.  Untimed calls first, median of 5, legs alternated.
usage: parabolic_tv_time.py [OUT [PX PY N NT NMU]]"""
import statistics
import sys
import time
sys.path.insert(0, '.')
import numpy as np
import torch
from bench import make_bases_host
from pylrbms_amd import multiscale_problem
from pylrbms_amd.engine import Engine

out_path = sys.argv[1] if len(sys.argv) > 1 else 'profiles/parabolic_tv_time.txt'
px, py, N, nt, nmu = (int(a) for a in (sys.argv[2:7] if len(sys.argv) > 6 else (32, 32, 40, 10, 64)))
T, RTOL, WARM, REPS, NMU_FOM = 0.05, 1e-12, 10, 5, 16

p = multiscale_problem.init_grid_and_problem({'num_subdomains': [px, py], 'coarse_per_subdomain': 4})
lam = p['lambda']
coeffs = lam['coefficients']
theta_bar = np.array([c.evaluate(p['mu_bar']) for c in coeffs])
eng = Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'], theta_bar).assemble()
c = eng.ctx
V = c.from_numpy(make_bases_host(eng.local, eng.t.n, N))
buf = eng.project_and_estimate(V, eng.alloc_reduce_buffers(N))
Lh = np.linalg.cholesky(buf['sys'][2].cpu().numpy())
Vo = torch.bmm(V, c.from_numpy(np.linalg.inv(Lh).transpose(0, 2, 1))).contiguous()
buf = eng.project_and_estimate(Vo, buf)
B, rhs, M, grams = buf['sys'][0], buf['sys'][1], buf['sys'][3], buf['grams']
lo, hi = p['parameter_range']
dt = T / nt


def table(count):
    """theta_t [count, nt + 1, Q]: theta(mu_m) times (1 + 0.2 sin(2 pi t / T)); the second coefficient drops to a tenth after
    t* = 4.5 dt."""
    mus = np.linspace(max(lo, 0.1), hi, count)
    th = np.array([[cf.evaluate(float(m)) for cf in coeffs] for m in mus])
    out = np.empty((count, nt + 1, th.shape[1]))
    t = 0.0
    for k in range(nt + 1):
        if k > 0:
            t += dt
        out[:, k] = th * (1.0 + 0.2 * np.sin(2 * np.pi * t / T))
        if t > 4.5 * dt:
            out[:, k, 1] *= 0.1
    return np.ascontiguousarray(out)


th_t = table(nmu)
th_mean = np.ascontiguousarray(th_t[:, 1:].mean(axis=1))
coef_t = np.ones((nmu, nt + 1, 2))
est_args = (B, M, grams, eng.f2, eng.ceps, eng.hdiam)


def leg_a():
    U, info = c.reduced_implicit_euler_batch_tv(th_t, dt, nt, B, M, rhs, rtol=RTOL)
    c.reduced_parabolic_estimate_batch_tv(th_t, coef_t, dt, nt, U, *est_args)
    return info['iterations']


def leg_a_solve():
    return c.reduced_implicit_euler_batch_tv(th_t, dt, nt, B, M, rhs, rtol=RTOL)[1]['iterations']


def leg_b():
    its, U0 = 0, None
    for k in range(nt):
        U, info = c.reduced_implicit_euler_batch(np.ascontiguousarray(th_t[:, k + 1]), dt, 1, B, M, rhs, U0=U0, rtol=RTOL)
        U0, its = U[1], its + info['iterations']
    return its


def leg_c():
    U, info = c.reduced_implicit_euler_batch(th_mean, dt, nt, B, M, rhs, rtol=RTOL)
    c.reduced_parabolic_estimate_batch(th_mean, coef_t[:, 0], dt, nt, U, *est_args)
    return info['iterations']


def leg_c_solve():
    return c.reduced_implicit_euler_batch(th_mean, dt, nt, B, M, rhs, rtol=RTOL)[1]['iterations']


thf_t = table(NMU_FOM)
thf_mean = np.ascontiguousarray(thf_t[:, 1:].mean(axis=1))
b_K = eng.b.reshape(1, eng.S, eng.t.n).contiguous()
ones = c.from_numpy(np.ones((NMU_FOM, nt + 1, 1)))
ones1 = c.from_numpy(np.ones((NMU_FOM, 2, 1)))


def fom_a():
    return c.fom_implicit_euler_batch_tv(thf_t, dt, nt, eng.A_diag, eng.A_cpl, b_K, ones, rtol=1e-10)[1]['iterations']


def fom_b():
    its, U0 = 0, None
    for k in range(nt):
        U, info = c.fom_implicit_euler_batch(np.ascontiguousarray(thf_t[:, k + 1]), dt, 1, eng.A_diag, eng.A_cpl, b_K, ones1, U0=U0,
                                             rtol=1e-10)
        U0, its = U[1], its + info['iterations']
    return its


def fom_c():
    return c.fom_implicit_euler_batch(thf_mean, dt, nt, eng.A_diag, eng.A_cpl, b_K, ones, rtol=1e-10)[1]['iterations']


def alternated(legs, warm, reps):
    for _ in range(warm):
        for fn in legs.values():
            fn()
    ts, its = {k: [] for k in legs}, {}
    for _ in range(reps):
        for k, fn in legs.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            its[k] = fn()
            torch.cuda.synchronize(); ts[k].append(time.perf_counter() - t0)
    return {k: (statistics.median(v), min(v), its[k]) for k, v in ts.items()}


lines = ['S {} N {} Q {} nt {} T {} rtol {} parameters {} (full order: {}, rtol 1e-10); median of {} after {} untimed rounds, legs alternated'
         .format(eng.S, N, eng.Q, nt, T, RTOL, nmu, NMU_FOM, REPS, WARM)]
red = alternated({'a': leg_a, 'a_solve': leg_a_solve, 'b': leg_b, 'c': leg_c, 'c_solve': leg_c_solve}, WARM, REPS)
names = {'a': '(a) _tv solve + _tv estimate', 'a_solve': '(a) _tv solve alone', 'b': '(b) nt chained nt = 1 solves',
         'c': '(c) existing solve + estimate at the time mean', 'c_solve': '(c) existing solve alone'}
for k, (med, mn, its) in red.items():
    lines.append('reduced  {:48s} median s {:.5f}  min s {:.5f}  iterations (slowest group, summed over the steps) {}'.format(names[k], med, mn, its))
lines.append('reduced  ratio (b) / (a) solve alone {:.3f}   (a) / (c) solve alone {:.3f}   iterations (a) / (c) {:.3f}'.format(
    red['b'][0] / red['a_solve'][0], red['a_solve'][0] / red['c_solve'][0], red['a_solve'][2] / red['c_solve'][2]))
fom = alternated({'a': fom_a, 'b': fom_b, 'c': fom_c}, 2, REPS)
names = {'a': '(a) lrbms_fom_implicit_euler_batch_tv', 'b': '(b) nt chained nt = 1 calls', 'c': '(c) existing export at the time mean'}
for k, (med, mn, its) in fom.items():
    lines.append('full     {:48s} median s {:.5f}  min s {:.5f}  iterations (summed over panels and steps) {}'.format(names[k], med, mn, its))
lines.append('full     ratio (b) / (a) {:.3f}   (a) / (c) {:.3f}   iterations (a) / (c) {:.3f}'.format(
    fom['b'][0] / fom['a'][0], fom['a'][0] / fom['c'][0], fom['a'][2] / fom['c'][2]))
text = '\n'.join(lines) + '\n'
print(text, end='')
with open(out_path, 'w') as fh:
    fh.write(text)
