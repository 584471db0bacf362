"""Times the batched reduced trajectories (lrbms_reduced_implicit_euler_batch) on config 3 -- 32 x 32 subdomains, N = 40, the
bench's problem and bases (energy-orthonormalised, as its online and parabolic legs use them), T = 0.05, 10 steps, rtol 1e-12,
64 parameters uniform in the parameter range -- against 64 consecutive lrbms_reduced_implicit_euler calls in the same process,
and reports from lrbms_kernel_timing the per-launch time of the mass-variant panel matvec beside the stationary one
(lrbms_reduced_solve_batch, the same 64 parameters).  At least 30 untimed passes first (README: the clock ramp).
usage: parabolic_batch_time.py [PX PY N NT NMU]   (default: 32 32 40 10 64, config 3)"""
import statistics
import sys
import time
sys.path.insert(0, '.')
import numpy as np
import torch
from bench import make_bases_host
from pylrbms_amd import multiscale_problem
from pylrbms_amd.engine import Engine

px, py, N, nt, nmu = (int(a) for a in (sys.argv[1:6] if len(sys.argv) > 5 else (32, 32, 40, 10, 64)))
T, RTOL, WARM, REPS = 0.05, 1e-12, 30, 5

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
B, rhs, M = buf['sys'][0], buf['sys'][1], buf['sys'][3]
lo, hi = p['parameter_range']
mus = np.linspace(max(lo, 0.1), hi, nmu)
thetas = np.array([[cf.evaluate(float(m)) for cf in coeffs] for m in mus])
dt = T / nt
work = c.empty(int(c.lib.lrbms_reduced_implicit_euler_batch_work_size(c.handle, N, nmu)))


def batched():
    return c.reduced_implicit_euler_batch(thetas, dt, nt, B, M, rhs, rtol=RTOL, work=work)


def loop():
    its = 0
    for th in thetas:
        _, info = c.reduced_implicit_euler(th, dt, nt, B, M, rhs, rtol=RTOL)
        its += info['iterations']
    return its


def timed(fn, reps=REPS):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return out, statistics.median(ts), min(ts)


print('S', eng.S, 'N', N, 'Q', eng.Q, 'nt', nt, 'T', T, 'rtol', RTOL, 'parameters', nmu, 'mu', float(mus[0]), '..', float(mus[-1]))
for _ in range(WARM):
    batched()
loop()
(Ub, ib), tb, tb_min = timed(batched)
its_loop, tl, tl_min = timed(loop, reps=3)
print('batched call      median s {:.5f}  min s {:.5f}  trajectories/s {:.1f}  iterations (sum over steps, all columns at once) {}  worst ratio {:.2e}'
      .format(tb, tb_min, nmu / tb, ib['iterations'], ib['relative_residual']))
print('{} single calls   median s {:.5f}  min s {:.5f}  trajectories/s {:.1f}  iterations (sum over calls) {}'.format(
    nmu, tl, tl_min, nmu / tl, its_loop))
print('ratio single loop / batched call {:.2f}'.format(tl / tb))
worst = 0.0
for m in (0, nmu // 2, nmu - 1):
    U1, _ = c.reduced_implicit_euler(thetas[m], dt, nt, B, M, rhs, rtol=RTOL)
    worst = max(worst, float((Ub[..., m] - U1).abs().max() / U1.abs().max()))
print('batch columns against the single export (first, middle, last): max relative difference {:.2e}'.format(worst))


def per_launch(fn, name):
    c.kernel_timing(True)
    fn()
    rows = [ms for nm, ms in c.kernel_timing_read(cap=4096) if nm == name]
    c.kernel_timing(False)
    return len(rows), 1e3 * statistics.median(rows), 1e3 * min(rows)


n1, med1, min1 = per_launch(batched, 'k_bcg_matvec_panel<mass>')
for _ in range(3):
    c.reduced_solve_batch(thetas, B, rhs, rtol=RTOL)
n0, med0, min0 = per_launch(lambda: c.reduced_solve_batch(thetas, B, rhs, rtol=RTOL), 'k_bcg_matvec_panel')
print('panel matvec per launch (lrbms_kernel_timing, events on the stream):')
print('  mass variant (step operator)  launches {}  median us {:.1f}  min us {:.1f}'.format(n1, med1, min1))
print('  stationary                    launches {}  median us {:.1f}  min us {:.1f}'.format(n0, med0, min0))
print('  ratio mass / stationary (median) {:.3f}'.format(med1 / med0))
