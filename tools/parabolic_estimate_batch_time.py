"""Times the batched parabolic estimate (``InstationaryReducedDiscretization.estimate_batch``: one
lrbms_reduced_parabolic_estimate_batch call) on config 3 -- 32 x 32 subdomains, k_c = 4, N = 40, Q = 2, the bench's problem and
bases (energy-orthonormalised), T = 0.05, 10 steps, 64 parameters uniform in [0.1, 1] -- against 64 consecutive ``rd.estimate``
calls in the same process, beside the ``solve_batch`` call that produced the trajectories, and reports the worst relative
difference between the two estimate paths.  Untimed calls first, then the median of 5.
usage: parabolic_estimate_batch_time.py [OUT [PX PY N NT NMU]]   (default: profiles/parabolic_estimate_batch_time.txt 32 32 40 10 64)"""
import statistics
import sys
import time
sys.path.insert(0, '.')
import numpy as np
import torch
from bench import make_bases_host
from pylrbms_amd import multiscale_problem
from pylrbms_amd.discretize_parabolic_block_swipdg import discretize
from pylrbms_amd.reductor import ParabolicLRBMSReductor

out_path = sys.argv[1] if len(sys.argv) > 1 else 'profiles/parabolic_estimate_batch_time.txt'
px, py, N, nt, nmu = (int(a) for a in (sys.argv[2:7] if len(sys.argv) > 6 else (32, 32, 40, 10, 64)))
T, WARM, REPS = 0.05, 3, 5

p = multiscale_problem.init_grid_and_problem({'num_subdomains': [px, py], 'coarse_per_subdomain': 4})
d, _ = discretize(p, T, nt)
eng = d.engine
c = eng.ctx
V = c.from_numpy(make_bases_host(eng.local, eng.t.n, N))
buf = eng.project_and_estimate(V, eng.alloc_reduce_buffers(N))
Lh = np.linalg.cholesky(buf['sys'][2].cpu().numpy())
Vo = torch.bmm(V, c.from_numpy(np.linalg.inv(Lh).transpose(0, 2, 1))).contiguous()
del buf
reductor = ParabolicLRBMSReductor(d, order=0)
reductor._V, reductor._nloc = Vo, np.full(eng.S, N, dtype=np.int64)     # the bench's bases, as they are
rd = reductor.reduce()
mus = [d.parse_parameter(float(m)) for m in np.linspace(0.1, 1.0, nmu)]


def timed(fn, reps=REPS):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return out, statistics.median(ts), min(ts)


for _ in range(WARM):
    Us = rd.solve_batch(mus)
    rd.estimate_batch(Us, mus)
rd.estimate(Us[0], mus[0])
Us, ts, ts_min = timed(lambda: rd.solve_batch(mus))
batch, tb, tb_min = timed(lambda: rd.estimate_batch(Us, mus))
loop, tl, tl_min = timed(lambda: [rd.estimate(U, mu) for U, mu in zip(Us, mus)])
names = ('local_eta_nc', 'local_eta_r', 'local_eta_df', 'time_residual', 'time_deriv_nc')
worst = {nm: 0.0 for nm in names + ('est',)}
for (e_b, parts_b), (e_l, parts_l) in zip(batch, loop):
    worst['est'] = max(worst['est'], abs(e_b - e_l) / e_l)
    for nm, a, b in zip(names, parts_b, parts_l):
        worst[nm] = max(worst[nm], float(np.abs(a - b).max() / np.abs(b).max()))
lines = [
    'S {} N {} Q {} nt {} T {} parameters {} mu 0.1 .. 1.0  layout {}'.format(eng.S, N, eng.Q, nt, T, nmu,
                                                                             'factored' if len(rd.grams) == 8 else 'dense'),
    'estimate_batch (one native call)  median s {:.5f}  min s {:.5f}  estimates/s {:.1f}'.format(tb, tb_min, nmu / tb),
    '{} rd.estimate calls              median s {:.5f}  min s {:.5f}  estimates/s {:.1f}'.format(nmu, tl, tl_min, nmu / tl),
    'ratio estimate loop / estimate_batch {:.2f}   (gate: >= 2)'.format(tl / tb),
    'solve_batch (the same parameters) median s {:.5f}  min s {:.5f}'.format(ts, ts_min),
    'ratio estimate_batch / solve_batch {:.2f}'.format(tb / ts),
    'worst relative difference estimate_batch vs rd.estimate: ' + '  '.join('{} {:.2e}'.format(k, v) for k, v in worst.items()),
]
with open(out_path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
print('\n'.join(lines))
