"""Every k3_pg tile instantiation of the 3D / P2 pass (BASELINE.json config 5), Q up to 8 and the online forms, against the CPU
oracle (oracle/lrbms3d.py) through the C ABI of include/lrbms3d_hip.h -- runs on the MI355X box (`-m gpu`).

``lrbms3_project_estimate_phase`` (csrc/lrbms3d.hip) launches ``k3_pg<KIND, RT, CT, EVEN>`` through ``dispatch_pg``: tn = ceil(N / 16)
square tiles for AAA / SYS / NC / CPL, (tn, tq) for AB and (tq, tq) for BB with tq = ceil(Q N / 16), the EVEN form when RT, CT and
N are all even.  One cell per (Q, N); together the cells select every instantiation ``dispatch_pg`` lists (pinned on the CPU by
tests/test_dispatch_coverage3d.py, which mirrors the host's choice).  Each cell: the assembled arrays, the projected blocks, the
single estimate and reduced solve against the oracle; forced K-splits and wave counts from NaN-filled buffers; the phased pass;
the batched estimate in both forms and the batched solve with both matvecs, with and without the prebuilt coarse level, at
nmu = 1, 16, 17 and 64; and the shapes the library refuses."""
import numpy as np
import pytest

import common3d as c3

pytestmark = pytest.mark.gpu

TOL = 1e-11
SOLVE_TOL = 1e-10
ASSEMBLED = ('A_diag', 'A_cpl', 'b', 'f2', 'ceps', 'bdiv', 'ebar', 'Aaa', 'Aab', 'Bbb', 'Cf', 'P_diag')
NMUS = (1, 16, 17, 64)
P_DEFAULT = (2, 1, 2)

# (Q, N, subdomains, k_c).  Comments: the k3_pg instantiations the cell selects, as (RT, CT) with "e" for the EVEN form --
# square kinds (AAA, SYS, NC, CPL) at (tn, tn), AB at (tn, tq), BB at (tq, tq).
CELLS = [
    (1, 17, P_DEFAULT, 1),      # square (2,2) odd, AB (2,2) odd, BB (2,2) odd; k3b_matvec_mfma<2>
    (1, 24, P_DEFAULT, 1),      # square (2,2)e, AB (2,2)e, BB (2,2)e
    (1, 33, P_DEFAULT, 1),      # square (3,3), AB (3,3), BB (3,3); batched solve refused
    (1, 48, P_DEFAULT, 1),      # square (3,3), AB (3,3), BB (3,3), even N
    (2, 17, P_DEFAULT, 1),      # square (2,2) odd, AB (2,3), BB (3,3)
    (2, 24, P_DEFAULT, 1),      # square (2,2)e, AB (2,3), BB (3,3)
    (2, 25, P_DEFAULT, 1),      # square (2,2) odd, AB (2,4) odd, BB (4,4) odd
    (2, 32, P_DEFAULT, 1),      # square (2,2)e, AB (2,4)e, BB (4,4)e
    (3, 11, P_DEFAULT, 1),      # square (1,1), AB (1,3), BB (3,3)
    (3, 16, P_DEFAULT, 1),      # square (1,1), AB (1,3), BB (3,3); k3b_matvec_mfma<1> at N = 16
    (3, 21, P_DEFAULT, 1),      # square (2,2) odd, AB (2,4) odd, BB (4,4) odd (Q N = 63)
    (4, 13, P_DEFAULT, 1),      # square (1,1), AB (1,4), BB (4,4) even tiles, odd N: odd form
    (4, 16, P_DEFAULT, 1),      # square (1,1), AB (1,4), BB (4,4)e (Q N = 64)
    (5, 12, P_DEFAULT, 1),      # square (1,1), AB (1,4), BB (4,4)e
    (6, 3, P_DEFAULT, 1),       # square (1,1), AB (1,2), BB (2,2) odd
    (6, 10, P_DEFAULT, 1),      # square (1,1), AB (1,4), BB (4,4)e
    (7, 9, P_DEFAULT, 1),       # square (1,1), AB (1,4), BB (4,4) odd (Q N = 63)
    (8, 8, P_DEFAULT, 1),       # square (1,1), AB (1,4), BB (4,4)e (Q = 8, Q N = 64)
    (8, 1, P_DEFAULT, 1),       # square (1,1), AB (1,1), BB (1,1) (Q = 8, N = 1)
    (1, 49, P_DEFAULT, 2),      # square (4,4) odd, AB (4,4) odd, BB (4,4) odd
    (1, 64, P_DEFAULT, 2),      # square (4,4)e, AB (4,4)e, BB (4,4)e (the largest N)
    (1, 64, P_DEFAULT, 4),      # as above on config 5's template (n_bf = 192, n_b = 386): the batched estimate's largest LDS
]


def _cell_id(c):
    return 'Q{}-N{}-kc{}'.format(c[0], c[1], c[3])


def _basis(d, N):
    return c3.make_bases3d(d.S, d.n, max(N, 2), seed=3)[:, :, -N:].copy()      # N = 1: a non-constant column


@pytest.fixture(scope='module', params=CELLS, ids=_cell_id)
def cell(request):
    import torch
    from pylrbms_amd.engine3d import Engine3D, expand_factored
    Q, N, P, kc = request.param
    p = c3.problem_with_q_components3d(P, kc, Q)
    p['N'] = N
    d = c3.oracle_of(p)
    eng = Engine3D(p['grid'], p['lambdas'], p['f'], p['lambda_bar'], p['lambda_hat'], theta_bar=c3.theta_of(p, p['mu_bar'])).assemble()
    V = _basis(d, N)
    Vd = eng.ctx.from_numpy(V)
    out = eng.project_and_estimate(Vd)
    torch.cuda.synchronize()
    rd = c3.reduce_with_oracle(p, d, V)
    refs = [c3.oracle_dense_blocks(p, d, rd, ii) for ii in range(d.S)]
    yield dict(p=p, d=d, eng=eng, Vd=Vd, out=out, rd=rd, refs=refs, dense=expand_factored(eng, out, Q, N))
    eng.ctx.close()


def _worst_projected(cell, out):
    """Largest relative deviation of the dense blocks of ``out`` from the oracle's, over every subdomain and operator."""
    from pylrbms_amd.engine3d import expand_factored
    d, rd, N = cell['d'], cell['rd'], cell['p']['N']
    got = {k: v.cpu().numpy() for k, v in expand_factored(cell['eng'], out, d.Q, N).items()}
    worst = {}
    for ii, ref in enumerate(cell['refs']):
        for k in ('G_nc', 'G_bb', 'G_rdd', 'r_fd'):
            worst[k] = max(worst.get(k, 0.0), c3.rel(got[k][ii], ref[k]))
        worst['G_ab'] = max(worst.get('G_ab', 0.0), c3.rel(got['G_ab'][:, ii], ref['G_ab']))
        worst['G_aa'] = max(worst.get('G_aa', 0.0), c3.rel(got['G_aa'][:, :, ii], ref['G_aa']))
        worst['B_sys'] = max(worst.get('B_sys', 0.0), c3.rel(got['B_sys'][:, ii], ref['B_sys']))
        worst['rhs_red'] = max(worst.get('rhs_red', 0.0), c3.rel(got['rhs_red'][ii], rd.rhs[ii]))
    return worst


def _forced_pass(cell, option, value):
    """One pass with ``option`` set to ``value``, outputs and work buffer NaN-filled first; the option is reset afterwards."""
    import torch
    eng, N = cell['eng'], cell['p']['N']
    o2, work = eng.alloc_outputs(N), eng.alloc_work(N)
    for v in o2.values():
        v.fill_(float('nan'))
    work.fill_(float('nan'))
    try:
        eng.ctx.set_option(option, value)
        eng.project_and_estimate(cell['Vd'], o2, work)
        torch.cuda.synchronize()
    finally:
        eng.ctx.set_option(option, 0)
    return o2


def test_assembled_operators_match_the_oracle(cell):
    p, d, eng = cell['p'], cell['d'], cell['eng']
    ref = c3.oracle_assembled(p, d)
    for k in ASSEMBLED:
        got = eng.ops[k].cpu().numpy().reshape(ref[k].shape)
        assert c3.rel(got, ref[k]) < TOL, (k, c3.rel(got, ref[k]))


def test_projected_operators_match_the_oracle(cell):
    worst = _worst_projected(cell, cell['out'])
    assert all(v < TOL for v in worst.values()), worst


def test_estimate_matches_the_oracle(cell):
    p, d, eng, rd = cell['p'], cell['d'], cell['eng'], cell['rd']
    u = np.random.default_rng(5).standard_normal((d.S, p['N']))
    eta = eng.reduced_estimate(c3.theta_of(p, p['mu']), eng.ctx.from_numpy(u), cell['out']).cpu().numpy()
    for got, ref, name in zip(eta, rd.local_terms([u[ii] for ii in range(d.S)], p['mu']), ('nc', 'r', 'df')):
        assert c3.rel(got, ref) < SOLVE_TOL, (name, c3.rel(got, ref))


def test_reduced_solve_matches_the_oracle(cell):
    p, eng, rd = cell['p'], cell['eng'], cell['rd']
    u, (it, res) = eng.reduced_solve(c3.theta_of(p, p['mu']), cell['out'], rtol=1e-13)
    ref = np.stack(rd.solve(p['mu']))
    assert res <= 1e-13 and it > 0
    assert c3.rel(u.cpu().numpy(), ref) < SOLVE_TOL, c3.rel(u.cpu().numpy(), ref)


@pytest.mark.parametrize('option,values', [('ksplit', (1, 2, 8)), ('waves', (2, 6, 16))])
def test_forced_launch_shapes_match_the_oracle(cell, option, values):
    """LRBMS3_OPT_KSPLIT (1: the in-kernel epilogues; 2, 8: partial tiles + k3_pg_combine) and LRBMS3_OPT_WAVES (the wave count of
    every k3_pg launch, clamped per kind), each from NaN-filled buffers: the oracle's blocks at the parity tolerance, and the
    automatic choice's outputs to summation-order rounding."""
    out = cell['out']
    for v in values:
        o2 = _forced_pass(cell, option, v)
        for k in out:
            scale = float(out[k].abs().max())
            assert float((out[k] - o2[k]).abs().max()) <= 1e-12 * max(scale, 1e-300), (option, v, k)
        worst = _worst_projected(cell, o2)
        assert all(w < TOL for w in worst.values()), (option, v, worst)


def test_phased_pass_is_bit_identical_to_the_whole_pass(cell):
    import torch
    eng, out, N = cell['eng'], cell['out'], cell['p']['N']
    out2, work = eng.alloc_outputs(N), eng.alloc_work(N)
    for v in out2.values():
        v.fill_(float('nan'))
    work.fill_(float('nan'))
    eng.ctx.project_estimate(eng.Q, cell['Vd'], eng.ops, work, out2, phase=1)
    eng.ctx.project_estimate(eng.Q, cell['Vd'], eng.ops, work, out2, phase=2)
    torch.cuda.synchronize()
    for k in out:
        assert torch.equal(out[k], out2[k]), k


@pytest.mark.parametrize('valu', [0, 1], ids=['estimate_batch16', 'estimate_batch'])
def test_batched_estimate_matches_the_oracle(cell, valu):
    """lrbms3_reduced_estimate_batch: k3_estimate_batch16 in chunks of 16 parameters (LRBMS3_OPT_ESTIMATE_VALU 0, the default;
    the VALU kernel where its LDS would not fit) or k3_estimate_batch in chunks of 8 (1); 1, 16, 17 and 64 parameters put a
    partial, a full, a one-column last and several chunks through each.  Every column against the oracle's local terms."""
    p, d, eng, rd = cell['p'], cell['d'], cell['eng'], cell['rd']
    rng = np.random.default_rng(8)
    try:
        eng.ctx.set_option('estimate_valu', valu)
        for nmu in NMUS:
            mus = rng.uniform(0.1, 1.3, size=nmu)
            U = rng.standard_normal((d.S, p['N'], nmu))
            thetas = np.stack([c3.theta_of(p, mu) for mu in mus])
            eta = eng.ctx.reduced_estimate_batch(d.Q, thetas, eng.ctx.from_numpy(U), cell['out'], eng.ops, eng.hdiam).cpu().numpy()
            for m, mu in enumerate(mus):
                ref = rd.local_terms([U[ii, :, m] for ii in range(d.S)], mu)
                for k in range(3):
                    assert c3.rel(eta[k, :, m], ref[k]) < SOLVE_TOL, (nmu, m, k, c3.rel(eta[k, :, m], ref[k]))
    finally:
        eng.ctx.set_option('estimate_valu', 0)


@pytest.mark.parametrize('valu', [0, 1], ids=['matvec_mfma', 'matvec_valu'])
def test_batched_solve_matches_the_oracle(cell, valu):
    """lrbms3_reduced_solve_batch with k3b_matvec_mfma<1 | 2> (N <= 16 | N > 16; LRBMS3_OPT_SOLVE_VALU 0) or k3b_matvec (1), with
    the inverse diagonal blocks alone and with the prebuilt coarse level, at 1, 16, 17 and 64 parameters: every column against
    the oracle's solution.  Beyond N = 32 the batched solve is refused."""
    from pylrbms_amd._native import NativeError
    p, d, eng, rd, out = cell['p'], cell['d'], cell['eng'], cell['rd'], cell['out']
    if p['N'] > 32:
        with pytest.raises(NativeError):
            eng.ctx.reduced_solve_batch(d.Q, np.stack([c3.theta_of(p, p['mu'])]), out['B_sys'], out['rhs_red'], rtol=1e-13)
        return
    try:
        eng.ctx.set_option('solve_valu', valu)
        for pc in (None, eng.ctx.reduced_precond_build(d.Q, c3.theta_of(p, 0.6), out['B_sys'])):
            eng.ctx.reduced_precond_use(pc)
            for nmu in NMUS:
                mus = np.linspace(0.15, 1.2, nmu)
                thetas = np.stack([c3.theta_of(p, mu) for mu in mus])
                ub, (it, res) = eng.ctx.reduced_solve_batch(d.Q, thetas, out['B_sys'], out['rhs_red'], rtol=1e-13)
                assert tuple(ub.shape) == (eng.S, p['N'], nmu) and res <= 1e-13 and it > 0, (nmu, pc is None, res)
                ub = ub.cpu().numpy()
                for m, mu in enumerate(mus):
                    ref = np.stack(rd.solve(mu))
                    assert c3.rel(ub[:, :, m], ref) < SOLVE_TOL, (nmu, m, pc is None, c3.rel(ub[:, :, m], ref))
    finally:
        eng.ctx.reduced_precond_use(None)
        eng.ctx.set_option('solve_valu', 0)


def test_shapes_beyond_the_limits_are_refused(cell):
    """The pass refuses Q N > 64, the batched solve N = 33 (both with NativeError, before any launch)."""
    from pylrbms_amd._native import NativeError
    d, eng, Q = cell['d'], cell['eng'], cell['d'].Q
    N2 = 64 // Q + 1
    with pytest.raises(NativeError):
        eng.project_and_estimate(eng.ctx.zeros(eng.S_ext, d.n, N2))
    with pytest.raises(NativeError):
        eng.ctx.reduced_solve_batch(Q, np.ones((2, Q)), eng.ctx.zeros(Q, eng.S, 7, 33, 33), eng.ctx.zeros(eng.S, 33))
