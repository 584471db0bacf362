"""Times the batched reduced trajectories of the 3D / P2 path (lrbms3_reduced_implicit_euler_batch) on config 5 -- 8 x 8 x 8
subdomains, k_c = 4, N = 30, Q = 2, the reduced model of tools/parabolic3d_time.py (snapshots of one full-order trajectory filled
up with random vectors), T = 0.1, 10 steps, rtol 1e-12, 64 parameters uniform in the parameter range -- against 64 consecutive
lrbms3_reduced_implicit_euler calls in the same process, and reports from lrbms3_kernel_timing the per-launch time of the
mass-variant panel matvec beside the stationary one (lrbms3_reduced_solve_batch, the same 64 parameters).  Untimed calls first.
usage: parabolic_batch3d_time.py [P kc N NT NMU]   (default: 8 4 30 10 64, config 5)"""
import statistics
import sys
import time
sys.path.insert(0, '.')
import numpy as np
import torch
from pylrbms_amd import multiscale_problem3d
from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D, discretize

P, kc, N, nt, nmu = (int(a) for a in (sys.argv[1:6] if len(sys.argv) > 5 else (8, 4, 30, 10, 64)))
T, RTOL, WARM, REPS = 0.1, 1e-12, 5, 5

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
mus = np.linspace(lo, hi, nmu)
thetas = np.stack([d.theta(float(m)) for m in mus])
dt = T / nt
work = c.empty(int(c.lib.lrbms3_reduced_implicit_euler_batch_work_size(c.handle, N, nmu)))
work1 = c.empty(int(c.lib.lrbms3_reduced_implicit_euler_work_size(c.handle, N)))


def batched():
    return c.reduced_implicit_euler_batch(Q, thetas, dt, nt, B, M, rhs, rtol=RTOL, work=work)


def loop():
    its = 0
    for th in thetas:
        _, info = c.reduced_implicit_euler(Q, th, dt, nt, B, M, rhs, rtol=RTOL, work=work1)
        its += info[0]
    return its


def timed(fn, reps=REPS):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return out, statistics.median(ts), min(ts)


print('S', eng.S, 'N', N, 'Q', Q, 'nt', nt, 'T', T, 'rtol', RTOL, 'parameters', nmu, 'mu', float(mus[0]), '..', float(mus[-1]), flush=True)
for _ in range(WARM):
    batched()
loop()
(Ub, ib), tb, tb_min = timed(batched)
its_loop, tl, tl_min = timed(loop, reps=3)
print('batched call      median s {:.5f}  min s {:.5f}  trajectories/s {:.1f}  iterations (sum over steps, slowest group) {}  worst ratio {:.2e}'
      .format(tb, tb_min, nmu / tb, ib[0], ib[1]))
print('{} single calls   median s {:.5f}  min s {:.5f}  trajectories/s {:.1f}  iterations (sum over calls) {}  per step and call {:.1f}'
      .format(nmu, tl, tl_min, nmu / tl, its_loop, its_loop / (nmu * nt)))
print('ratio single loop / batched call {:.2f}'.format(tl / tb))
print('batched: {:.1f} iterations per step, {:.1f} us per iteration of all {} columns'.format(ib[0] / nt, 1e6 * tb / max(ib[0], 1), nmu))
worst = 0.0
for m in (0, nmu // 2, nmu - 1):
    U1, _ = c.reduced_implicit_euler(Q, thetas[m], dt, nt, B, M, rhs, rtol=RTOL, work=work1)
    worst = max(worst, float((Ub[..., m] - U1).abs().max() / U1.abs().max()))
print('batch columns against the single export (first, middle, last): max relative difference {:.2e}'.format(worst), flush=True)


def per_launch(fn, name):
    c.kernel_timing(True)
    fn()
    rows = [ms for nm, ms in c.kernel_timing_read(cap=4096) if nm == name]
    c.kernel_timing(False)
    return len(rows), 1e3 * statistics.median(rows), 1e3 * min(rows)


# one group alone (16 columns, nothing else on the chip) and the four groups of the call side by side; the stationary twin runs
# with its prebuilt two-level preconditioner, so that both matvecs read the coarse correction and its r.z partials
pc = c.reduced_precond_build(Q, d.theta(0.5 * (lo + hi)), B)
for cols in (16, nmu):
    th = thetas[:cols]
    n1, med1, min1 = per_launch(lambda: c.reduced_implicit_euler_batch(Q, th, dt, 2, B, M, rhs, rtol=RTOL), 'k3b_matvec_mfma<mass>')
    c.reduced_precond_use(pc)
    try:
        for _ in range(2):
            c.reduced_solve_batch(Q, th, B, rhs, rtol=RTOL)
        n0, med0, min0 = per_launch(lambda: c.reduced_solve_batch(Q, th, B, rhs, rtol=RTOL), 'k3b_matvec_mfma')
    finally:
        c.reduced_precond_use(None)
    print('panel matvec per launch, {} columns (lrbms3_kernel_timing, events on the stream):'.format(cols))
    print('  mass variant (step operator)  launches {}  median us {:.1f}  min us {:.1f}'.format(n1, med1, min1))
    print('  stationary                    launches {}  median us {:.1f}  min us {:.1f}'.format(n0, med0, min0))
    print('  ratio mass / stationary (median) {:.3f}  (blocks read per subdomain: {} against {}: {:.3f})'.format(
        med1 / med0, 7 * Q + 1, 7 * Q, (7 * Q + 1) / (7 * Q)))
