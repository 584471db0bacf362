"""Times the 3D parabolic exports with a diffusion-coefficient row per step on config 5 -- 8 x 8 x 8 subdomains,
k_c = 4, N = 30, Q = 2, the reduced model of tools/parabolic_batch3d_time.py, T = 0.1, nt = 10, 64 parameters; theta_t: a smooth
factor of the time times one 10x switch on the second coefficient between the steps 4 and 5 -- and writes
profiles/parabolic_tv3d_time.txt.  Legs, at the level of the native context:
  (a) lrbms3_reduced_implicit_euler_batch_tv and lrbms3_reduced_parabolic_estimate_batch_tv with the table;
  (b) the only route without them: nt chained lrbms3_reduced_implicit_euler_batch calls with nt = 1 at row k + 1, slab k as U0;
  (c) the twins at the time mean of the table (a time-independent model), with the iteration counts of (a) and (c);
  (=) a table that is constant in time through the _tv exports against the twins at that theta: the _tv median must not lie above
      the twin's slowest of its five runs.  Every estimate leg follows the solve leg of its own export, and the _tv legs and the
      twin legs change places from round to round, so that neither always runs behind the other.
The same legs for lrbms3_fom_implicit_euler_batch(_tv) (NMU_FOM = 0 leaves them out).  Untimed calls first, median of 5, legs
alternated in one process.
usage: parabolic_tv3d_time.py [OUT [P kc N NT NMU NMU_FOM]]"""
import statistics
import sys
import time
sys.path.insert(0, '.')
import numpy as np
import torch
from pylrbms_amd import multiscale_problem3d
from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D, discretize

out_path = sys.argv[1] if len(sys.argv) > 1 else 'profiles/parabolic_tv3d_time.txt'
P, kc, N, nt, nmu, nmu_fom = (int(a) for a in (sys.argv[2:8] if len(sys.argv) > 7 else (8, 4, 30, 10, 64, 64)))
T, RTOL, RTOL_FOM, WARM, REPS = 0.1, 1e-12, 1e-10, 3, 5

p = multiscale_problem3d.init_grid_and_problem({'num_subdomains': (P, P, P), 'cubes_per_subdomain': kc})
d, _ = discretize(p, T, nt)
eng = d.engine
c, Q = eng.ctx, d.Q
U = d.solve(0.5)
reductor = ParabolicLRBMSReductor3D(d)
reductor.extend_basis(U[:, :, 1:])
g = torch.Generator(device=U.device).manual_seed(0)
while reductor.basis_size() < N:           # fill up with random vectors so that the reduced model has the bench size
    reductor.extend_basis(torch.randn(eng.S, eng.t.n, 1, dtype=torch.float64, device=U.device, generator=g))
rd = reductor.reduce()
N = reductor.basis_size()
B, rhs, M = rd.out['B_sys'], rd.out['rhs_red'], rd.M_red
lo, hi = p['parameter_range']
dt = T / nt


def table(count):
    """theta_t [count, nt + 1, Q]: theta(mu_m) times (1 + 0.2 sin(2 pi t / T)); the second coefficient drops to a tenth after
    t* = 4.5 dt."""
    th = np.stack([d.theta(float(m)) for m in np.linspace(lo, hi, count)])
    out = np.empty((count, nt + 1, Q))
    for k in range(nt + 1):
        out[:, k] = th * (1.0 + 0.2 * np.sin(2 * np.pi * k * dt / T))
        if k * dt > 4.5 * dt:
            out[:, k, 1] *= 0.1
    return np.ascontiguousarray(out)


def const(th):
    return np.ascontiguousarray(np.repeat(th[:, None, :], nt + 1, axis=1))


th_t = table(nmu)
th_mean = np.ascontiguousarray(th_t[:, 1:].mean(axis=1))
coef_t = np.ones((nmu, nt + 1, 2))
coef = np.ascontiguousarray(coef_t[:, 0])
U_tv = c.reduced_implicit_euler_batch_tv(Q, th_t, dt, nt, B, M, rhs, rtol=RTOL)[0]
est = (U_tv, B, M, rd.out, eng.ops, eng.hdiam)

red = {
    'a_solve': lambda: c.reduced_implicit_euler_batch_tv(Q, th_t, dt, nt, B, M, rhs, rtol=RTOL)[1][0],
    'a_estimate': lambda: c.reduced_parabolic_estimate_batch_tv(Q, th_t, coef_t, dt, nt, *est) and 0,
    'c_solve': lambda: c.reduced_implicit_euler_batch(Q, th_mean, dt, nt, B, M, rhs, rtol=RTOL)[1][0],
    'c_estimate': lambda: c.reduced_parabolic_estimate_batch(Q, th_mean, coef, dt, nt, *est) and 0,
    '=_solve_tv': lambda: c.reduced_implicit_euler_batch_tv(Q, const(th_mean), dt, nt, B, M, rhs, rtol=RTOL)[1][0],
    '=_estimate_tv': lambda: c.reduced_parabolic_estimate_batch_tv(Q, const(th_mean), coef_t, dt, nt, *est) and 0,
    '=_solve_twin': lambda: c.reduced_implicit_euler_batch(Q, th_mean, dt, nt, B, M, rhs, rtol=RTOL)[1][0],
    '=_estimate_twin': lambda: c.reduced_parabolic_estimate_batch(Q, th_mean, coef, dt, nt, *est) and 0,
}


def red_b():
    its, U0 = 0, None
    for k in range(nt):
        Uk, info = c.reduced_implicit_euler_batch(Q, np.ascontiguousarray(th_t[:, k + 1]), dt, 1, B, M, rhs, U0=U0, rtol=RTOL)
        U0, its = Uk[1], its + info[0]
    return its


red['b_solve'] = red_b

thf_t = table(max(nmu_fom, 1))
thf_mean = np.ascontiguousarray(thf_t[:, 1:].mean(axis=1))
b_K = eng.ops['b'].reshape(1, eng.S, eng.t.n).contiguous()
ones = c.from_numpy(np.ones((max(nmu_fom, 1), nt + 1, 1)))
ones1 = c.from_numpy(np.ones((max(nmu_fom, 1), 2, 1)))
A = (eng.ops['A_diag'], eng.ops['A_cpl'], b_K)
work_f = c.empty(int(c.lib.lrbms3_fom_implicit_euler_batch_work_size(c.handle, max(nmu_fom, 1))))


def fom_b():
    its, U0 = 0, None
    for k in range(nt):
        Uk, info = c.fom_implicit_euler_batch(np.ascontiguousarray(thf_t[:, k + 1]), dt, 1, *A, ones1, U0=U0, rtol=RTOL_FOM, work=work_f)
        U0, its = Uk[1], its + info['iterations']
    return its


fom = {
    'a_solve': lambda: c.fom_implicit_euler_batch_tv(thf_t, dt, nt, *A, ones, rtol=RTOL_FOM, work=work_f)[1]['iterations'],
    'b_solve': fom_b,
    'c_solve': lambda: c.fom_implicit_euler_batch(thf_mean, dt, nt, *A, ones, rtol=RTOL_FOM, work=work_f)[1]['iterations'],
    '=_solve_tv': lambda: c.fom_implicit_euler_batch_tv(const(thf_mean), dt, nt, *A, ones, rtol=RTOL_FOM, work=work_f)[1]['iterations'],
    '=_solve_twin': lambda: c.fom_implicit_euler_batch(thf_mean, dt, nt, *A, ones, rtol=RTOL_FOM, work=work_f)[1]['iterations'],
}


def alternated(legs, warm, reps):
    for _ in range(warm):
        for fn in legs.values():
            fn()
        print('untimed round done', flush=True)
    ts, its = {k: [] for k in legs}, {}
    for rep in range(reps):
        order = list(legs)
        if rep % 2:                      # the constant-table pairs change places
            for k in [k for k in order if k.endswith('_tv')]:
                i, j = order.index(k), order.index(k[:-3] + '_twin')
                order[i], order[j] = order[j], order[i]
        for k in order:
            fn = legs[k]
            torch.cuda.synchronize(); t0 = time.perf_counter()
            its[k] = fn()
            torch.cuda.synchronize(); ts[k].append(time.perf_counter() - t0)
        print('round', rep, {k: round(v[-1], 5) for k, v in ts.items()}, flush=True)
    return {k: (statistics.median(v), min(v), max(v), its[k]) for k, v in ts.items()}


lines = ['S {} N {} Q {} nt {} T {} parameters {} (rtol {}) / full order {} (rtol {}); median of {} after untimed rounds, legs alternated'
         .format(eng.S, N, Q, nt, T, nmu, RTOL, nmu_fom, RTOL_FOM, REPS)]
for tag, legs, warm in (('reduced', red, WARM), ('full', fom, 1))[:2 if nmu_fom > 0 else 1]:
    r = alternated(legs, warm, REPS)
    for k, (med, mn, mx, its) in r.items():
        lines.append('{:8s} {:16s} median s {:.5f}  min s {:.5f}  max s {:.5f}  iterations {}'.format(tag, k, med, mn, mx, its))
    lines.append('{:8s} solve: (b) / (a) {:.3f}   (a) / (c) {:.3f}   iterations (a) / (c) {:.3f}'.format(
        tag, r['b_solve'][0] / r['a_solve'][0], r['a_solve'][0] / r['c_solve'][0], r['a_solve'][3] / max(r['c_solve'][3], 1)))
    if 'a_estimate' in r:
        lines.append('{:8s} estimate: (a) / (c) {:.3f}'.format(tag, r['a_estimate'][0] / r['c_estimate'][0]))
    for what in ('solve', 'estimate'):
        if '=_{}_tv'.format(what) in r:
            tvm, twin = r['=_{}_tv'.format(what)], r['=_{}_twin'.format(what)]
            lines.append('{:8s} constant table, {}: _tv median {:.5f} against the twin median {:.5f} (its five runs {:.5f} .. {:.5f}): {}'.format(
                tag, what, tvm[0], twin[0], twin[1], twin[2], 'not slower' if tvm[0] <= twin[2] else 'SLOWER'))
    text = '\n'.join(lines) + '\n'
    with open(out_path, 'w') as fh:
        fh.write(text)
print(text, end='')
