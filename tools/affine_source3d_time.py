"""Times the 3D / P2 path with an affine source at config 5 (8 x 8 x 8 subdomains, N = 30, Q = 2): the same problem with f alone
(K = 1, the existing entry points) and with f + c_1 g (K = 2; stationary c_1(mu) = max(0, 2 mu - 1), parabolic c_0(mu, t) =
[sin(4 pi t) > 0], c_1 = -1).  Legs alternate inside one session (rounds), medians and the spread are printed.

* solve loop: 256 parameters in calls of 64 under the prebuilt preconditioner: lrbms3_reduced_solve_batch, the same data through
  lrbms3_reduced_solve_batch_src (K = 1, phi = 1; bits compared), K = 2 through lrbms3_reduced_solve_batch_src -> mu-solves/s;
* lrbms3_project_sources (K = 1, 2, 16): time, and bytes/s against the bytes of one read of V;
* lrbms3_reduced_source_terms for 64 columns beside the batched estimate it accompanies;
* one full-order and one reduced trajectory (nt = 10) with K = 2 against the existing exports with K = 1.
usage: affine_source3d_time.py [ROUNDS] [CONFIG]   (defaults 5, cfg5)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench3d import CONFIGS3D  # noqa: E402
from pylrbms_amd import multiscale_problem3d, sources3d  # noqa: E402
from pylrbms_amd.discretize_parabolic_block_swipdg_3d import discretize  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
cfg = CONFIGS3D[sys.argv[2] if len(sys.argv) > 2 else 'cfg5']
N, NT, T = cfg['N'], 10, 1.0


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def alternate(legs, rounds, warm=1):
    """{name: [seconds per round]}, {name: last result}; the legs take turns inside every round."""
    for _ in range(warm):
        for fn in legs.values():
            fn()
    times, outs = {k: [] for k in legs}, {}
    for _ in range(rounds):
        for k, fn in legs.items():
            outs[k], t = once(fn)
            times[k].append(t)
    return times, outs


def report(title, times, unit=1e3, fmt='{:.3f}', per=None):
    for k, ts in times.items():
        v = np.array(ts) * unit if per is None else per / np.array(ts)
        print('{} {:24s} median {}  min {}  max {}  spread {:.1f} %'.format(title, k, fmt.format(np.median(v)), fmt.format(v.min()),
                                                                         fmt.format(v.max()), 100 * (v.max() - v.min()) / np.median(v)))


def g(x):
    return np.cos(np.pi * x[..., 0]) * (1.0 + x[..., 1] * x[..., 2])


p = multiscale_problem3d.init_grid_and_problem({'num_subdomains': cfg['num_subdomains'], 'cubes_per_subdomain': cfg['cubes_per_subdomain']})
d1, _ = discretize(p, T, NT)
d2, _ = discretize(dict(p, f={'functions': [p['f'], g], 'coefficients': [lambda mu, t: float(np.sin(4 * np.pi * t) > 0), -1.0]}), T, NT)
stat = dict(d2._src, coefficients=[1, lambda mu: max(0.0, 2 * mu - 1)], arity=[0, 1])      # the stationary coefficients on the same components
eng, c, Q = d2.engine, d2.engine.ctx, d2.Q
S, n = eng.S, eng.t.n
print('S', S, 'dofs', S * n, 'N', N, 'Q', Q, 'rounds', rounds)

gen = torch.Generator(device='cuda').manual_seed(0)
V = torch.randn(S, n, N, dtype=torch.float64, device='cuda', generator=gen)
V[:, :, 0] = 1.0
V = torch.linalg.qr(V)[0].contiguous()
work = eng.alloc_work(N)
out = eng.project_and_estimate(V, work=work)
out1 = d1.engine.project_and_estimate(V)
M_red = c.project_mass(V)
src = d2._src

# ---- lrbms3_project_sources
vbytes = 8 * V.numel()
for K in (1, 2, 16):
    b_K = src['b_K'][:1].expand(K, -1, -1).contiguous() if K != 2 else src['b_K']
    bd_K = src['bdiv_K'][:1].expand(K, -1, -1).contiguous() if K != 2 else src['bdiv_K']
    times, _ = alternate({'K = {}'.format(K): lambda: c.project_sources(Q, b_K, bd_K, V, work)}, max(rounds, 5), warm=2)
    ts = np.array(times['K = {}'.format(K)])
    print('project_sources K = {:2d}  ms median {:.3f} min {:.3f} max {:.3f}  bytes of one read of V {:.1f} MB -> {:.2f} TB/s at the median'.format(
        K, np.median(ts) * 1e3, ts.min() * 1e3, ts.max() * 1e3, vbytes / 1e6, vbytes / np.median(ts) / 1e12))
times, _ = alternate({'pass': lambda: eng.project_and_estimate(V, out, work)}, max(rounds, 5), warm=2)
report('project_estimate (ms)', times)
rhs_K, rfd_K = c.project_sources(Q, src['b_K'], src['bdiv_K'], V, work)

# ---- solve loop: 256 parameters in calls of 64
mus = np.random.default_rng(7).uniform(0.1, 1.0, size=256)
thetas = np.array([d2.theta(m) for m in mus])
phis = np.array([sources3d.evaluate_stationary(stat, m) for m in mus])
print('phi[:, 1] == 0 for {} of {} parameters'.format(int((phis[:, 1] == 0).sum()), len(mus)))
c.reduced_precond_use(c.reduced_precond_build(Q, d2.theta(0.55), out['B_sys']))
rhs1 = out1['rhs_red']
rhs1_K = rhs1[None].contiguous()
wk = c.empty(int(c.lib.lrbms3_reduced_solve_batch_work_size(c.handle, N, 64)))


def loop(fn):
    res = [fn(b0) for b0 in range(0, len(mus), 64)]
    return torch.cat([r[0] for r in res], dim=2), max(r[1][0] for r in res)


legs = {'K=1 existing': lambda: loop(lambda b0: c.reduced_solve_batch(Q, thetas[b0:b0 + 64], out['B_sys'], rhs1, work=wk)),
        'K=1 _src phi=1': lambda: loop(lambda b0: c.reduced_solve_batch_src(Q, thetas[b0:b0 + 64], np.ones((64, 1)), out['B_sys'], rhs1_K,
                                                                            work=wk)),
        'K=2 _src': lambda: loop(lambda b0: c.reduced_solve_batch_src(Q, thetas[b0:b0 + 64], phis[b0:b0 + 64], out['B_sys'], rhs_K, work=wk))}
times, outs = alternate(legs, rounds)
report('solve loop (mu-solves/s)', times, fmt='{:.0f}', per=len(mus))
print('iterations', {k: v[1] for k, v in outs.items()})
print('K=1 _src phi=1 equal to the existing export: {}'.format(bool(torch.equal(outs['K=1 existing'][0], outs['K=1 _src phi=1'][0]))))
c.reduced_precond_use(None)

# ---- the f terms of 64 columns beside the batched estimate
u64 = outs['K=2 _src'][0][:, :, :64].contiguous()
out0, ops0 = sources3d.zeroed(eng, out)
th64, ph64 = c.from_numpy(thetas[:64]), c.from_numpy(phis[:64])
legs = {'estimate_batch (f in it)': lambda: c.reduced_estimate_batch(Q, thetas[:64], u64, out, eng.ops, eng.hdiam),
        'estimate_batch (zero f)': lambda: c.reduced_estimate_batch(Q, thetas[:64], u64, out0, ops0, eng.hdiam),
        'reduced_source_terms': lambda: c.reduced_source_terms(Q, th64, ph64, src['F2'], rfd_K, src['bdiv_K'], out['Rb'], u64,
                                                               eng.ops['ceps'], eng.hdiam)}
times, _ = alternate(legs, max(rounds, 5), warm=2)
report('64 columns (ms)', times)

# ---- trajectories, nt = 10
mu = 0.45
legs = {'reduced K=1 existing': lambda: c.reduced_implicit_euler(Q, d1.theta(mu), d1.dt, NT, out1['B_sys'], M_red, out1['rhs_red']),
        'reduced K=2 _src': lambda: c.reduced_implicit_euler_src(Q, d2.theta(mu), d2.dt, NT, out['B_sys'], M_red, rhs_K,
                                                                 d2.source_coefficients(mu))}
times, outs = alternate(legs, rounds)
report('reduced trajectory (ms)', times)
print('iterations', {k: v[1][0] for k, v in outs.items()})
legs = {'full order K=1 existing': lambda: d1.solve(mu, return_info=True), 'full order K=2 _src': lambda: d2.solve(mu, return_info=True)}
times, outs = alternate(legs, min(rounds, 3), warm=1)
report('full-order trajectory (s)', times, unit=1.0, fmt='{:.4f}')
print('iterations', {k: v[1][0] for k, v in outs.items()})
