"""Times the batched parabolic estimate of the 3D / P2 path (lrbms3_reduced_parabolic_estimate_batch through
``rd.estimate_batch(U, mus, native=True)``) on config 5 -- 8 x 8 x 8 subdomains, k_c = 4, N = 30, Q = 2, the reduced model of
tools/parabolic_batch3d_time.py (snapshots of one full-order trajectory filled up with random vectors), T = 0.1, 10 steps, 64
parameters uniform in the parameter range -- against the loop of 64 ``rd.estimate`` calls in the same process, with the
``rd.solve_batch`` call that made the trajectories beside them for scale, and reports from lrbms3_kernel_timing the time per pass
(16 columns) of the nc-only kernel k3_estimate_nc_batch16 beside the full k3_estimate_batch16.  Untimed calls first, median of 5.
usage: parabolic_estimate_batch3d_time.py [P kc N NT NMU]   (default: 8 4 30 10 64, config 5)"""
import statistics
import sys
import time
sys.path.insert(0, '.')
import numpy as np
import torch
from pylrbms_amd import multiscale_problem3d
from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D, discretize

P, kc, N, nt, nmu = (int(a) for a in (sys.argv[1:6] if len(sys.argv) > 5 else (8, 4, 30, 10, 64)))
T, WARM, REPS = 0.1, 2, 5

p = multiscale_problem3d.init_grid_and_problem({'num_subdomains': (P, P, P), 'cubes_per_subdomain': kc})
d, _ = discretize(p, T, nt)
eng = d.engine
c = eng.ctx
U = d.solve(0.5)
reductor = ParabolicLRBMSReductor3D(d)
reductor.extend_basis(U[:, :, 1:])
g = torch.Generator(device=U.device).manual_seed(0)
while reductor.basis_size() < N:           # fill up with random vectors so that the reduced model has the bench size
    reductor.extend_basis(torch.randn(eng.S, eng.t.n, 1, dtype=torch.float64, device=U.device, generator=g))
rd = reductor.reduce()
N = reductor.basis_size()
lo, hi = p['parameter_range']
mus = [float(m) for m in np.linspace(lo, hi, nmu)]


def timed(fn, reps=REPS):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return out, statistics.median(ts), min(ts)


print('S', eng.S, 'N', N, 'Q', d.Q, 'nt', nt, 'T', T, 'parameters', nmu, 'mu', mus[0], '..', mus[-1], flush=True)
rd.solve_batch(mus)
Ub, ts, ts_min = timed(lambda: rd.solve_batch(mus))
for _ in range(WARM):
    rd.estimate_batch(Ub, mus, native=True)
rd.estimate_batch(Ub, mus)
nat, tn, tn_min = timed(lambda: rd.estimate_batch(Ub, mus, native=True))
loop, tl, tl_min = timed(lambda: rd.estimate_batch(Ub, mus))
print('solve_batch                 median s {:.5f}  min s {:.5f}'.format(ts, ts_min))
print('estimate_batch native       median s {:.5f}  min s {:.5f}  estimates/s {:.1f}'.format(tn, tn_min, nmu / tn))
print('{} rd.estimate calls (loop) median s {:.5f}  min s {:.5f}  estimates/s {:.1f}'.format(nmu, tl, tl_min, nmu / tl))
print('ratio loop / native {:.2f}   (gate from the pass counts alone: 1.5)'.format(tl / tn))
dt = rd.dt
e_est = max(abs(a[0] - b[0]) / abs(b[0]) for a, b in zip(nat, loop))


def sq(parts):
    return (parts[0], parts[1], parts[2], np.asarray(parts[3]) ** 2 * 3.0 / dt, np.asarray(parts[4]) ** 2 * dt)


e_parts = max(float(np.abs(x - y).max() / np.abs(y).max()) for a, b in zip(nat, loop) for x, y in zip(sq(a[1]), sq(b[1])))
print('native against the loop: est {:.2e} relative, squared parts {:.2e} of their largest entry'.format(e_est, e_parts), flush=True)

c.kernel_timing(True)
rd.estimate_batch(Ub, mus, native=True)
rows = c.kernel_timing_read(cap=4096)
c.kernel_timing(False)
for name in ('k3_estimate_batch16', 'k3_estimate_nc_batch16'):
    ms = [v for nm, v in rows if nm == name]
    if ms:
        print('{:24s} passes {:3d}  median us {:.1f}  min us {:.1f}  sum ms {:.2f}'.format(name, len(ms), 1e3 * statistics.median(ms),
                                                                                        1e3 * min(ms), sum(ms)))
full = [v for nm, v in rows if nm == 'k3_estimate_batch16']
nc = [v for nm, v in rows if nm == 'k3_estimate_nc_batch16']
if full and nc:
    print('nc-only pass / full pass (median) {:.3f}'.format(statistics.median(nc) / statistics.median(full)))
