"""The call sequence of DESIGN section 5.4.2's finding (tools/affine_source_time.py's order): reduced work on a discretization
d1 (reduce, prebuilt preconditioner, batched solves with it and with their own, batched ``_src`` solves), a ``reduce()`` of a
second discretization d2 with a two-component affine source, then d1's batched solve and estimate.  Shared by
tests/test_call_order_gpu.py and run as a fresh process by its regression test:

    python tests/call_order_seq.py NX MODE OUT      MODE: fresh (d1.solve first) | sequence (d1.solve after the sequence)

writes d1.solve's solution and iteration count at MU to OUT (.npz)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MU = [1.0]
N = 8


def problems(nx):
    """(p, p2): the multiscale problem on nx x nx subdomains (128 elements each, as config 3) and the same problem with the
    source f + theta^f_1(mu) g, g = cos(pi x), theta^f_1 = (mu > 0.5) (2 mu - 1)."""
    from pylrbms_amd import multiscale_problem
    from pylrbms_amd.functions import make_expression_function_1x1
    from pylrbms_amd.parameters import ExpressionParameterFunctional
    p = multiscale_problem.init_grid_and_problem({'num_subdomains': [nx, nx], 'coarse_per_subdomain': 4})
    g = make_expression_function_1x1(None, 'x', 'cos(pi*x[0])', order=2, name='g')
    switch = ExpressionParameterFunctional('(diffusion > 0.5) * (2 * diffusion - 1)', p['parameter_type'])
    return p, dict(p, f={'functions': [p['f'], g], 'coefficients': [1, switch]})


def reductors(d1, d2, N=N):
    """LRBMSReductors of d1 and d2 on the same seeded, energy-orthonormal bases (no full-order solve on either)."""
    import torch
    from bench import make_bases_host
    from pylrbms_amd.reductor import LRBMSReductor
    from pylrbms_amd.vectorarrays import BlockVectorArray, BlockVectorSpace
    eng, c = d1.engine, d1.engine.ctx
    V = c.from_numpy(make_bases_host(eng.local, eng.t.n, N))
    E = eng.project_and_estimate(V)['sys'][2].cpu().numpy()
    Vo = torch.bmm(V, c.from_numpy(np.linalg.inv(np.linalg.cholesky(E)).transpose(0, 2, 1))).contiguous()
    out = []
    for d in (d1, d2):
        bases = {'domain_{}'.format(ii): BlockVectorArray(Vo[i:i + 1], BlockVectorSpace([d.solution_space.subspaces[i]]))
                 for i, ii in enumerate(eng.local)}
        out.append(LRBMSReductor(d, bases=bases))
    return out


def sequence(d1, d2, close_d2=False, nmu=64, N=N):
    """The reduced work of section 5.4.2 on d1 around a reduce() of d2; d2's context is closed after it if ``close_d2``."""
    c = d1.engine.ctx
    r1, r2 = reductors(d1, d2, N)
    rd1 = r1.reduce()
    mus = np.random.default_rng(7).uniform(0.1, 1.0, size=nmu)
    thetas = np.array([d1.theta([m]) for m in mus])
    pc = c.reduced_precond_build(d1.theta([0.55]), rd1.B_sys)
    c.reduced_precond_use(pc)
    c.reduced_solve_batches(thetas, rd1.B_sys, rd1.rhs_red)
    c.reduced_solve_batches_src(thetas, np.ones((nmu, 1)), rd1.B_sys, rd1.rhs_red[None].contiguous())
    c.reduced_precond_use(None)
    c.reduced_solve_batches(thetas, rd1.B_sys, rd1.rhs_red)
    rd2 = r2.reduce()
    assert rd2.rhs_red_K is not None and rd2.rhs_red_K.shape[0] == 2
    if close_d2:
        d2.engine.ctx.close()
    rd1.solve_batch([[m] for m in mus[:17]])
    u = rd1.solve(MU)
    rd1.estimate(u, MU)


def main(nx, mode, out):
    import torch
    from pylrbms_amd.discretize_elliptic_block_swipdg import discretize
    p, p2 = problems(nx)
    d1, _ = discretize(p)
    if mode == 'sequence':
        d2, _ = discretize(p2)
        sequence(d1, d2, N=40)                   # config 3's basis size
    elif mode != 'fresh':
        raise SystemExit('mode: fresh | sequence')
    try:
        x = d1.solve(MU).tensor.cpu().numpy()
        info = d1.last_solve_info
        rc = 0
    except Exception as e:                      # a non-converged CG is reported, not raised past the file
        print('d1.solve:', e)
        x, info, rc = np.zeros(0), {'iterations': -1, 'relative_residual': float('nan')}, 1
    torch.cuda.synchronize()
    np.savez(out, x=x, iterations=info['iterations'], relative_residual=info['relative_residual'])
    print('{} {}x{}: iterations {} relative residual {:.3e}'.format(mode, nx, nx, info['iterations'], info['relative_residual']))
    return rc


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main(int(sys.argv[1]), sys.argv[2], sys.argv[3]))
