"""Times the stationary path with a parameter-dependent affine source at config 3 (32 x 32 subdomains, N = 40): the same
problem with f alone (K = 1, the existing entry points) and with f + theta^f_1(mu) g (K = 2, theta^f_1 = (mu > 0.5) (2 mu - 1)).

* solve loop: 256 parameters in calls of 64, under the prebuilt preconditioner, alternated in one session: K = 1 through
  lrbms_reduced_solve_batch, K = 1 data through lrbms_reduced_solve_batch_src (phi = 1; bits compared), K = 2 through
  lrbms_reduced_solve_batch_src -> mu-solves/s per round and the median;
* d.solve(mu) for K = 2 against K = 1 (lrbms_combine_sources + lrbms_fom_solve), ahead of the reduced work, and
  lrbms_combine_sources;
* the reduced estimate of 64 parameters (rd.estimate per mu, and the batched kernel for K = 1 against the batched kernel with
  f2 = 0, r_fd = 0 plus one lrbms_reduced_source_terms launch per mu for K = 2);
* the extra time per enrichment round: lrbms_flux_reconstruct + lrbms_div_apply + lrbms_project_sources on the whole slab,
  next to an incremental reduce(touched=) of 8 subdomains.
usage: affine_source_time.py [ROUNDS]   (default 5)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench import CONFIGS, make_bases_host  # noqa: E402
from pylrbms_amd import multiscale_problem  # noqa: E402
from pylrbms_amd.discretize_elliptic_block_swipdg import discretize  # noqa: E402
from pylrbms_amd.functions import make_expression_function_1x1  # noqa: E402
from pylrbms_amd.parameters import ExpressionParameterFunctional, parse_parameter  # noqa: E402
from pylrbms_amd.reductor import LRBMSReductor  # noqa: E402
from pylrbms_amd.vectorarrays import BlockVectorArray, BlockVectorSpace, ReducedVectorArray  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
cfg = CONFIGS['cfg3']
N = cfg['N']


def timed(fn, reps=3):
    fn()
    best = 1e9
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return out, best


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


p = multiscale_problem.init_grid_and_problem({'num_subdomains': cfg['num_subdomains'], 'coarse_per_subdomain': cfg['coarse_per_subdomain']})
g = make_expression_function_1x1(None, 'x', 'cos(pi*x[0])', order=2, name='g')
switch = ExpressionParameterFunctional('(diffusion > 0.5) * (2 * diffusion - 1)', p['parameter_type'])
d1, _ = discretize(p)
d2, _ = discretize(dict(p, f={'functions': [p['f'], g], 'coefficients': [1, switch]}))
eng, c = d1.engine, d1.engine.ctx
print('S', eng.S, 'dofs', eng.S * eng.t.n, 'N', N, 'K', d2._affine_f['K'])

# ---- full-order solve, d.solve: lrbms_combine_sources + lrbms_fom_solve against lrbms_fom_solve on the plain b.  Run ahead of
# the reduced work: on config 3 a first lrbms_fom_solve that comes after the reduced legs below diverged (profiles/
# cfg3_fom_solve_order.txt), an open finding of its own
bK = d2._affine_f['b_K']
for m in (1.0, 0.3):
    mu = parse_parameter([m], p['parameter_type'])
    _, t1 = timed(lambda: d1.solve(mu), reps=2)
    i1 = d1.last_solve_info
    _, t2 = timed(lambda: d2.solve(mu), reps=2)
    i2 = d2.last_solve_info
    print('d.solve mu {}  K=1 s {:.4f} ({} its)  K=2 s {:.4f} ({} its)  ratio {:.4f}'.format(
        m, t1, i1['iterations'], t2, i2['iterations'], t2 / t1))
_, tc = timed(lambda: c.combine_sources(d2.f_coefficients(parse_parameter([1.0], p['parameter_type'])), bK), reps=20)
nbytes = 8 * (bK.numel() + bK[0].numel())
print('combine_sources (K 2, M {})  us {:.1f}  {:.2f} TB/s'.format(bK[0].numel(), tc * 1e6, nbytes / tc / 1e12))

# the same energy-orthonormal bases in both models
V = c.from_numpy(make_bases_host(eng.local, eng.t.n, N))
E = eng.project_and_estimate(V)['sys'][2].cpu().numpy()
Vo = torch.bmm(V, c.from_numpy(np.linalg.inv(np.linalg.cholesky(E)).transpose(0, 2, 1))).contiguous()
red = {}
for name, d in (('K=1', d1), ('K=2', d2)):
    bases = {'domain_{}'.format(ii): BlockVectorArray(Vo[i:i + 1], BlockVectorSpace([d.solution_space.subspaces[i]]))
             for i, ii in enumerate(eng.local)}
    r = LRBMSReductor(d, bases=bases)
    rd, t = timed(lambda: r.reduce(), reps=2)
    red[name] = (r, rd)
    print('reduce() {}  s {:.4f}'.format(name, t))
r1, rd1 = red['K=1']
r2, rd2 = red['K=2']
assert torch.equal(rd1.B_sys, rd2.B_sys)

# ---- solve loop
mus = np.random.default_rng(7).uniform(0.1, 1.0, size=256)
pmus = [parse_parameter([m], p['parameter_type']) for m in mus]
thetas = np.array([d1.theta(m) for m in pmus])
phis = np.array([d2.f_coefficients(m) for m in pmus])
print('phi[:, 1] == 0 for {} of {} parameters'.format(int((phis[:, 1] == 0).sum()), len(mus)))
pc = c.reduced_precond_build(d1.theta(parse_parameter([0.55], p['parameter_type'])), rd1.B_sys)
c.reduced_precond_use(pc)
rhs1, rhs1_K = rd1.rhs_red, rd1.rhs_red[None].contiguous()
legs = {'K=1 existing': lambda: c.reduced_solve_batches(thetas, rd1.B_sys, rhs1),
        'K=1 _src phi=1': lambda: c.reduced_solve_batches_src(thetas, np.ones((len(mus), 1)), rd1.B_sys, rhs1_K),
        'K=2 _src': lambda: c.reduced_solve_batches_src(thetas, phis, rd2.B_sys, rd2.rhs_red_K)}
for fn in legs.values():
    fn()
rates = {k: [] for k in legs}
outs = {}
for rnd in range(rounds):
    for k, fn in legs.items():
        (u, info), t = once(fn)
        rates[k].append(len(mus) / t)
        outs[k] = (u, info)
    print('round {}  '.format(rnd) + '  '.join('{} {:.0f}'.format(k, rates[k][-1]) for k in legs))
for k in legs:
    print('solve loop {:16s} mu-solves/s median {:.0f}  min {:.0f}  max {:.0f}  iterations {}'.format(
        k, np.median(rates[k]), min(rates[k]), max(rates[k]), outs[k][1]['iterations']))
print('K=1 _src phi=1 equal to the existing export: {}'.format(bool(torch.equal(outs['K=1 existing'][0], outs['K=1 _src phi=1'][0]))))
print('K=2 / K=1 median ratio {:.4f}'.format(np.median(rates['K=2 _src']) / np.median(rates['K=1 existing'])))
c.reduced_precond_use(None)

# ---- reduced estimate of 64 parameters
u64 = outs['K=2 _src'][0][:, :, :64].contiguous()
u64_1 = outs['K=1 existing'][0][:, :, :64].contiguous()


def est_loop(rd, u):
    return [rd.estimate(ReducedVectorArray(u[:, :, m:m + 1].contiguous()), pmus[m]) for m in range(64)]


_, te1 = timed(lambda: est_loop(rd1, u64_1), reps=2)
_, te2 = timed(lambda: est_loop(rd2, u64), reps=2)
print('rd.estimate x 64  K=1 s {:.4f}  K=2 s {:.4f}  ratio {:.3f}'.format(te1, te2, te2 / te1))
zg = list(rd2.grams)
zg[1] = torch.zeros_like(zg[1])
zg = tuple(zg)
zf2 = c.zeros(eng.S)


def est_k2():
    eta = c.reduced_estimate_batch(thetas[:64], u64, zg, zf2, eng.ceps, eng.hdiam)
    for m in range(64):
        eta[1, :, m] += c.reduced_source_terms(thetas[m], phis[m:m + 1], d2._affine_f['F2'], rd2.r_fd_K,
                                               u64[:, :, m:m + 1].contiguous(), eng.ceps, eng.hdiam)[:, 0]
    return eta


_, tb1 = timed(lambda: c.reduced_estimate_batch(thetas[:64], u64_1, rd1.grams, eng.f2, eng.ceps, eng.hdiam))
_, tb2 = timed(est_k2)
print('batched estimate kernel x 64  K=1 ms {:.3f}  K=2 (+64 source-term launches) ms {:.3f}'.format(tb1 * 1e3, tb2 * 1e3))

# ---- enrichment round: what the affine source adds to reduce(touched=)
Vs = r2._V.contiguous()
_, tp = timed(lambda: r2._with_affine_source(rd2, Vs, {}), reps=5)
touched = list(range(0, eng.S, eng.S // 8))[:8]
r1.reserve(N)
r1.reduce()
_, ti = timed(lambda: r1.reduce(touched=touched), reps=3)
print('enrichment round extra (flux_reconstruct + div_apply + project_sources, all {} subdomains) ms {:.3f}  '
      'incremental reduce(touched={} subdomains) ms {:.3f} ({})'.format(eng.S, tp * 1e3, len(touched), ti * 1e3,
                                                                       r1.last_reduce_info))
