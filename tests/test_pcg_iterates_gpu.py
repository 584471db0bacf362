"""The PCG iterates of the 2D solver exports against a NumPy PCG with the same operator and the same preconditioner.

A converged solution does not depend on the preconditioner, so the parity tests cannot see a wrong inverse diagonal block, a
wrong coarse row or a dropped coarse term.  The k-th PCG iterate from x_0 = 0 can: every export stops after exactly
``max_iter`` iterations, returns LRBMS_E_NOT_CONVERGED and leaves x_k and info = (k, |r_k| / |r_0|) behind, and
``tests/pcg_ref.py`` computes the same x_k in NumPy from the operator the product assembled (B_sys of the fused pass, A_diag /
A_cpl of the assembly) and the preconditioner restated from the kernels.  Each cell calls the raw export through ``ctx.lib``
with max_iter = k for k in K_STEPS (while the reference residual ratio is still >= MIN_RATIO), asserts rc, info[0] == k, x_k
within TOL_X of the reference in every column and info[1] within TOL_RES of the reference ratio, then closes with one converged
call against a direct solve.  On every cell with a coarse level, a run with LRBMS_OPT_COARSE 0 is compared against the
two-level reference too and must miss it by more than MUTANT_FLOOR: the cell can tell the two preconditioners apart.

The cell lists are module constants: tests/test_pcg_iterates_host.py mirrors the host's dispatch in online.hip and checks on
the CPU that they reach every instantiation and branch."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve

import pcg_ref

pytestmark = pytest.mark.gpu

E_NOT_CONVERGED = -4
K_STEPS = (1, 2, 3, 6)
MIN_RATIO = 1e-6          # no k whose reference residual ratio is below this (loss of orthogonality)
TOL_X = 1e-10             # x_k per column, relative to its norm
TOL_RES = 1e-8            # info[1] against the reference ratio, relative
MUTANT_FLOOR = 1e4 * TOL_X
KC = 2                    # coarse elements per subdomain and direction of the reduced cells (n_T = 32)

# A. single reduced solve: (grid, N) -- coarse none (S < 4), b = 1, b = 4, both sides of the 64 KB LDS thresholds of k_bt_factor
# (b 51 | 52) and k_bt_inverse (b 56 | 57), b = 64, b = 65 (rocSOLVER), S = 4096 (the limit) and S > 4096 (none)
SINGLE_GRIDS = (((3, 1), 3), ((1, 5), 3), ((4, 3), 3), ((51, 2), 2), ((52, 2), 2), ((56, 2), 2), ((57, 2), 2), ((64, 2), 2),
                ((65, 2), 2), ((64, 64), 2), ((65, 64), 2))
SWEEP_GRID = (4, 3)
SINGLE_N = (1, 2, 15, 16, 17, 33, 40, 63, 64)        # k_cg2_*<true | false>, k_block_inverse at 63 | 64 (its LDS threshold)
Q_COMPONENTS = (1, 2, 4, 8)
# B. batched solve on SWEEP_GRID: (N, nmu) -- panels of 16 (k_bcg_matvec_mfma<16>), 32 and 64 with every ksc_n
BATCH_CELLS = ((5, 1), (40, 16), (3, 17), (16, 32), (24, 17), (40, 32), (48, 17), (64, 32),
               (16, 64), (32, 33), (40, 47), (48, 64), (64, 33))
VALU_CELLS = ((48, 17), (64, 40))                    # LRBMS_OPT_SOLVE_VALU: groups of 16, NM on both sides of 768
SRC_CELL = (6, 20, 3)                                # lrbms_reduced_solve_batch_src: N, nmu, K
# C. full order: (grid, k_c, coarse) -- n_T = 32 (k_fom_restrict), 128 (two waves per subdomain), 512 (eight)
FOM_CELLS = (((3, 1), 2, 1), ((4, 3), 2, 1), ((64, 2), 2, 1), ((4, 3), 2, 0), ((4, 3), 4, 1), ((2, 2), 8, 1))
# On 64 x 2 subdomains of two coarse elements the fine elements are 32 times as long as they are wide, and the SWIPDG operator
# of the multiscale problem is not positive definite there (the oracle's global matrix has an eigenvalue near -578 at
# mu = 0.37): CG has no converged solution to close the cell with.  Its first iterates are still well defined and checked.
FOM_INDEFINITE = ((64, 2),)

_MODELS = {}


def _theta(Q, mu):
    return np.array([1.0, mu]) if Q == 2 else np.linspace(0.3, 1.0, Q) * (0.5 + mu)


def _problem(shape, kc, Q=2):
    from pylrbms_amd import multiscale_problem
    from common import problem_with_q_components
    if Q == 2:
        return multiscale_problem.init_grid_and_problem({'num_subdomains': list(shape), 'coarse_per_subdomain': kc})
    return problem_with_q_components(shape, kc, Q)


def _energy_bases(eng, N, seed=0):
    """Constant + seeded random columns per subdomain, orthonormal in the product's own local energy product (P_diag)."""
    from common import make_bases
    t, S = eng.ctx.t, eng.S
    X = make_bases(S, t.n, N, seed=seed)
    P = pcg_ref.blockell_operator(eng.P_diag.cpu().numpy(), t)
    PX = np.stack([P @ X[:, :, j].ravel() for j in range(N)], axis=-1).reshape(S, t.n, N)
    G = np.einsum('sni,snj->sij', X, PX)
    L = np.linalg.cholesky(G)
    return np.ascontiguousarray(np.linalg.solve(L, X.transpose(0, 2, 1)).transpose(0, 2, 1))


def _model(shape, N, Q=2, kc=KC):
    """Engine on the grid and the reduced system of one pass at basis size N (host copies, kept per (shape, N, Q, kc))."""
    key = (tuple(shape), N, Q, kc)
    if key not in _MODELS:
        from pylrbms_amd.engine import Engine
        from common import theta_bar_of
        p = _problem(shape, kc, Q)
        lam = p['lambda']
        eng = Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'], theta_bar_of(p)).assemble()
        m = {'eng': eng, 'nbr': np.asarray(p['grid'].neighbor_slots), 'Q': len(lam['functions'])}
        if N:
            buf = eng.project_and_estimate(eng.ctx.from_numpy(_energy_bases(eng, N, seed=5)))
            m['B'], m['rhs'] = buf['sys'][0].cpu().numpy(), buf['sys'][1].cpu().numpy()
        _MODELS[key] = m
    return _MODELS[key]


def _raw(ctx, name, *args):
    """One raw export call with caller-owned buffers -> its return code (no exception on LRBMS_E_NOT_CONVERGED)."""
    rc = getattr(ctx.lib, name)(ctx.handle, *args)
    ctx.torch.cuda.synchronize(ctx.device)
    return rc


def _dev(ctx, a):
    return ctx.from_numpy(np.ascontiguousarray(a))


def check_iterates(run, reference, tag, tol_x=TOL_X, tol_res=TOL_RES, steps=K_STEPS):
    """run(k) -> (rc, X [n, m], info); reference(k) -> (X [n, m], ratios [m]).  Asserts the module's contract per k (the
    tolerances and the k are the module's unless a caller with another operator source states its own)."""
    done, cell, worst_res = 0, 0.0, 0.0
    for k in steps:
        X_ref, ratios = reference(k)
        live = ratios[np.linalg.norm(X_ref, axis=0) > 0.0]
        if live.size and live.min() < MIN_RATIO:
            break
        rc, X, info = run(k)
        assert rc == E_NOT_CONVERGED, (tag, k, rc)
        assert int(info[0]) == k, (tag, k, info)
        nrm = np.linalg.norm(X_ref, axis=0)
        err = np.linalg.norm(X - X_ref, axis=0) / np.where(nrm > 0.0, nrm, 1.0)
        assert np.isfinite(err).all() and err.max() < tol_x, (tag, k, float(err.max()))
        res = abs(info[1] - ratios.max()) / ratios.max()
        assert res < tol_res, (tag, k, info[1], float(ratios.max()), res)
        cell = max(cell, float(err.max()))
        worst_res = max(worst_res, float(res))
        done += 1
    assert done >= 1, tag
    print('PCG-ITERATES {}: {} values of k, worst x_k error {:.2e} (tolerance {:.0e}), worst ratio error {:.2e}'.format(
        tag, done, cell, tol_x, worst_res))
    return cell, worst_res


def check_mutant(run, reference, tag):
    """A run of the cell with LRBMS_OPT_COARSE 0 (the caller switched it) against the TWO-LEVEL reference: must miss."""
    k = 2
    X_ref, _ = reference(k)
    rc, X, _ = run(k)
    nrm = np.linalg.norm(X_ref, axis=0)
    err = float((np.linalg.norm(X - X_ref, axis=0) / np.where(nrm > 0.0, nrm, 1.0)).max())
    assert err > MUTANT_FLOOR, (tag, err)
    print('PCG-ITERATES {}: coarse = 0 misses the two-level x_2 by {:.2e} ({:.1e} x the tolerance)'.format(tag, err, err / TOL_X))


# ------------------------------------------------------------------------------------------------------- A. single solve
def _single(m, N, theta, pc_theta=None, coarse=1, B=None, rhs=None, keep=None):
    """(run, reference) of lrbms_reduced_solve on model m at basis size N (leading N columns of its bases)."""
    from pylrbms_amd._native import _dblp, c_vp
    eng = m['eng']
    ctx, S, Q = eng.ctx, eng.S, m['Q']
    B = np.ascontiguousarray(m['B'][..., :N, :N]) if B is None else B
    rhs = np.ascontiguousarray(m['rhs'][:, :N]) if rhs is None else rhs
    A = pcg_ref.reduced_operator(pcg_ref.combine_reduced(B, theta), m['nbr'])
    M = pcg_ref.ReducedPrecond(pcg_ref.combine_reduced(B, theta if pc_theta is None else pc_theta), m['nbr'], coarse)
    Bd, rd = _dev(ctx, B), _dev(ctx, rhs)
    work = ctx.empty(int(ctx.lib.lrbms_reduced_solve_work_size(ctx.handle, N)))
    th = np.ascontiguousarray(theta, dtype=np.float64)

    def run(k, rtol=1e-14):
        u = ctx.empty(S, N)
        info = np.zeros(2)
        rc = _raw(ctx, 'lrbms_reduced_solve', Q, N, _dblp(th), c_vp(Bd.data_ptr()), c_vp(rd.data_ptr()), c_vp(work.data_ptr()),
                  c_vp(u.data_ptr()), float(rtol), int(k), _dblp(info), ctx._stream())
        return rc, u.cpu().numpy().reshape(-1, 1), info

    def reference(k):
        return pcg_ref.pcg_iterate(lambda p: A @ p, M.apply, rhs.reshape(-1, 1), k)

    def converged():
        rc, u, info = run(20000, rtol=1e-13)
        assert rc == 0 and info[1] <= 1e-13, (rc, info)
        pad = 0.0 if keep is None else sp.diags(1.0 - keep.ravel())      # padded unknowns: 1 on the diagonal, as D^-1 has
        ref = spsolve((A + pad).tocsc(), rhs.ravel())
        assert np.linalg.norm(u[:, 0] - ref) < 1e-10 * np.linalg.norm(ref)
    return run, reference, converged, M


def _single_cell(m, N, tag):
    eng = m['eng']
    run, ref, converged, M = _single(m, N, _theta(m['Q'], 0.37))
    check_iterates(run, ref, tag)
    converged()
    if M.has_coarse:
        eng.ctx.set_option('coarse', 0)
        try:
            check_mutant(run, ref, tag)
        finally:
            eng.ctx.set_option('coarse', 1)
    return M


@pytest.mark.parametrize('shape, N', SINGLE_GRIDS)
def test_single_solve_iterates_over_the_coarse_branches(shape, N):
    m = _model(shape, N)
    S = m['eng'].S
    M = _single_cell(m, N, 'single {} N={}'.format(shape, N))
    assert M.has_coarse == (4 <= S <= 4096), (shape, S)
    if S > 1000:
        del _MODELS[(tuple(shape), N, 2, KC)]           # the two large grids are not needed again


@pytest.mark.parametrize('N', SINGLE_N)
def test_single_solve_iterates_over_basis_sizes(N):
    _single_cell(_model(SWEEP_GRID, max(SINGLE_N)), N, 'single {} N={}'.format(SWEEP_GRID, N))


def test_single_solve_iterates_coarse_options_and_prebuilt_preconditioner():
    m = _model(SWEEP_GRID, max(SINGLE_N))
    eng, N = m['eng'], 7
    th, th_pc = np.array([1.0, 0.37]), np.array([1.0, 0.8])
    for coarse in (0, 2):
        eng.ctx.set_option('coarse', coarse)
        try:
            run, ref, converged, M = _single(m, N, th, coarse=coarse)
            assert M.has_coarse == (coarse != 0)
            check_iterates(run, ref, 'single coarse={}'.format(coarse))
            converged()
        finally:
            eng.ctx.set_option('coarse', 1)
    B = np.ascontiguousarray(m['B'][..., :N, :N])
    pc = eng.ctx.reduced_precond_build(th_pc, _dev(eng.ctx, B))
    eng.ctx.reduced_precond_use(pc)
    try:
        run, ref, converged, M = _single(m, N, th, pc_theta=th_pc)
        check_iterates(run, ref, 'single prebuilt at another theta')
        converged()
        eng.ctx.set_option('coarse', 0)
        try:
            check_mutant(run, ref, 'single prebuilt')
        finally:
            eng.ctx.set_option('coarse', 1)
    finally:
        eng.ctx.reduced_precond_use(None)


def _ragged(m, N, seed=3):
    """Leading columns of the model's bases with exact zero columns behind sizes[s] (ragged bases in a slab of width N, as
    online enrichment leaves them): B_sys and rhs_red with the padded rows and columns zeroed."""
    S = m['eng'].S
    rng = np.random.default_rng(seed)
    sizes = rng.integers(max(1, N - 5), N + 1, size=S)
    sizes[0] = N
    keep = (np.arange(N)[None, :] < sizes[:, None]).astype(np.float64)          # [S, N]
    nb = np.where(m['nbr'] >= 0, m['nbr'], 0)
    B = m['B'][..., :N, :N] * keep[None, :, None, :, None] * keep[nb][None, :, :, None, :]
    return np.ascontiguousarray(B), np.ascontiguousarray(m['rhs'][:, :N] * keep), keep


def test_single_solve_iterates_with_zero_padded_ragged_bases():
    m = _model(SWEEP_GRID, max(SINGLE_N))
    B, rhs, keep = _ragged(m, 12)
    assert (keep == 0).any()
    run, ref, converged, M = _single(m, 12, np.array([1.0, 0.37]), B=B, rhs=rhs, keep=keep)
    check_iterates(run, ref, 'single ragged')
    rc, u, _ = run(3)
    assert np.all(u.reshape(keep.shape)[keep == 0] == 0.0)     # the padded unknowns stay exactly 0
    converged()


@pytest.mark.parametrize('Q', Q_COMPONENTS)
def test_single_solve_iterates_over_affine_components(Q):
    m = _model((3, 3), 5, Q=Q)
    _single_cell(m, 5, 'single Q={}'.format(Q))


# ------------------------------------------------------------------------------------------------------ B. batched solve
def _batch(m, N, nmu, pc_theta=None, K=0, seed=0):
    """(run, reference) of lrbms_reduced_solve_batch (K = 0) or _src (K >= 1) with nmu parameters on model m."""
    from pylrbms_amd._native import _dblp, c_vp
    eng = m['eng']
    ctx, S, Q = eng.ctx, eng.S, m['Q']
    B = np.ascontiguousarray(m['B'][..., :N, :N])
    mus = np.linspace(0.1, 1.0, nmu)
    thetas = np.ascontiguousarray(np.stack([_theta(Q, mu) for mu in mus]))
    M = pcg_ref.ReducedPrecond(pcg_ref.combine_reduced(B, thetas.mean(axis=0) if pc_theta is None else pc_theta), m['nbr'])
    As = [pcg_ref.reduced_operator(pcg_ref.combine_reduced(B, th), m['nbr']) for th in thetas]
    if K == 0:
        rhs = np.ascontiguousarray(m['rhs'][:, :N])
        cols = np.repeat(rhs.reshape(-1, 1), nmu, axis=1)
    else:
        rng = np.random.default_rng(seed)
        rhs = np.ascontiguousarray(rng.standard_normal((K, S, N)) * np.abs(m['rhs'][:, :N]).max())
        phi = np.ascontiguousarray(rng.uniform(0.2, 1.0, (nmu, K)))
        cols = np.einsum('mk,kn->nm', phi, rhs.reshape(K, -1))
    Bd, rd = _dev(ctx, B), _dev(ctx, rhs)
    work = ctx.empty(int(ctx.lib.lrbms_reduced_solve_batch_work_size(ctx.handle, N, nmu)))

    def run(k, rtol=1e-14):
        u = ctx.empty(S, N, nmu)
        info = np.zeros(2)
        if K == 0:
            rc = _raw(ctx, 'lrbms_reduced_solve_batch', Q, N, nmu, _dblp(thetas), c_vp(Bd.data_ptr()), c_vp(rd.data_ptr()),
                      c_vp(work.data_ptr()), c_vp(u.data_ptr()), float(rtol), int(k), _dblp(info), ctx._stream())
        else:
            rc = _raw(ctx, 'lrbms_reduced_solve_batch_src', Q, N, K, nmu, _dblp(thetas), _dblp(phi), c_vp(Bd.data_ptr()),
                      c_vp(rd.data_ptr()), c_vp(work.data_ptr()), c_vp(u.data_ptr()), float(rtol), int(k), _dblp(info),
                      ctx._stream())
        return rc, u.cpu().numpy().reshape(-1, nmu), info

    def reference(k):
        out = [pcg_ref.pcg_iterate(lambda p, A=A: A @ p, M.apply, cols[:, j], k) for j, A in enumerate(As)]
        return np.stack([x for x, _ in out], axis=1), np.array([r for _, r in out])

    def converged():
        rc, u, info = run(20000, rtol=1e-13)
        assert rc == 0 and info[1] <= 1e-13, (rc, info)
        for j in sorted({0, nmu // 2, nmu - 1}):
            ref = spsolve(As[j].tocsc(), cols[:, j])
            assert np.linalg.norm(u[:, j] - ref) < 1e-10 * np.linalg.norm(ref), j
    return run, reference, converged, M


@pytest.mark.parametrize('N, nmu', BATCH_CELLS)
def test_batched_solve_iterates_over_the_panel_dispatch(N, nmu):
    m = _model(SWEEP_GRID, max(SINGLE_N))
    eng = m['eng']
    tag = 'batch N={} nmu={}'.format(N, nmu)
    run, ref, converged, M = _batch(m, N, nmu)
    check_iterates(run, ref, tag)
    converged()
    assert M.has_coarse
    eng.ctx.set_option('coarse', 0)
    try:
        check_mutant(run, ref, tag)
    finally:
        eng.ctx.set_option('coarse', 1)


@pytest.mark.parametrize('N, nmu', ((5, 1), (24, 17), (40, 47)))
def test_batched_solve_iterates_with_a_prebuilt_preconditioner(N, nmu):
    m = _model(SWEEP_GRID, max(SINGLE_N))
    eng = m['eng']
    th_pc = np.array([1.0, 0.8])
    pc = eng.ctx.reduced_precond_build(th_pc, _dev(eng.ctx, np.ascontiguousarray(m['B'][..., :N, :N])))
    eng.ctx.reduced_precond_use(pc)
    try:
        run, ref, converged, _ = _batch(m, N, nmu, pc_theta=th_pc)
        check_iterates(run, ref, 'batch prebuilt N={} nmu={}'.format(N, nmu))
        converged()
    finally:
        eng.ctx.reduced_precond_use(None)


@pytest.mark.parametrize('N, nmu', VALU_CELLS)
def test_batched_solve_iterates_valu_form(N, nmu):
    m = _model(SWEEP_GRID, max(SINGLE_N))
    eng = m['eng']
    eng.ctx.set_option('solve_valu', 1)
    try:
        run, ref, converged, _ = _batch(m, N, nmu)
        check_iterates(run, ref, 'batch VALU N={} nmu={}'.format(N, nmu))
        converged()
    finally:
        eng.ctx.set_option('solve_valu', 0)


def test_batched_source_solve_iterates():
    N, nmu, K = SRC_CELL
    m = _model(SWEEP_GRID, max(SINGLE_N))
    run, ref, converged, _ = _batch(m, N, nmu, K=K)
    check_iterates(run, ref, 'batch src N={} nmu={} K={}'.format(N, nmu, K))
    converged()


# ---------------------------------------------------------------------------------------------------------- C. full order
@pytest.mark.parametrize('shape, kc, coarse', FOM_CELLS)
def test_fom_solve_iterates(shape, kc, coarse):
    from pylrbms_amd._native import _dblp, c_vp
    m = _model(shape, 0, kc=kc)
    eng = m['eng']
    ctx, S, t = eng.ctx, eng.S, eng.ctx.t
    th = np.array([1.0, 0.37])
    A_diag, A_cpl, b = eng.A_diag.cpu().numpy(), eng.A_cpl.cpu().numpy(), eng.b.cpu().numpy()
    A = pcg_ref.fom_operator(A_diag, A_cpl, th, t, m['nbr'])
    if S * t.n <= 2000:              # the sparse builder against the dense helpers of the API shim
        from pylrbms_amd.engine import blockell_to_dense, coupling_to_dense
        Ad = A.toarray()
        Amu_d, Amu_c = np.einsum('q,qs...->s...', th, A_diag), np.einsum('q,qs...->s...', th, A_cpl)
        for s in range(S):
            blk = slice(s * t.n, (s + 1) * t.n)
            assert np.array_equal(Ad[blk, blk], blockell_to_dense(t, Amu_d[s]))
            for side, slot in enumerate((0, 1, 3, 4)):
                s2 = int(m['nbr'][s, slot])
                if s2 >= 0:
                    assert np.array_equal(Ad[blk, s2 * t.n:(s2 + 1) * t.n], coupling_to_dense(t, Amu_c[s, side], side))
    M = pcg_ref.FomPrecond(A, S, t.n, coarse)
    assert M.has_coarse == (coarse != 0 and S >= 4)
    work = ctx.empty(int(ctx.lib.lrbms_fom_solve_work_size(ctx.handle)))

    def run(k, rtol=1e-14):
        x = ctx.empty(S, t.n)
        info = np.zeros(2)
        rc = _raw(ctx, 'lrbms_fom_solve', 2, _dblp(th), c_vp(eng.A_diag.data_ptr()), c_vp(eng.A_cpl.data_ptr()),
                  c_vp(eng.b.data_ptr()), c_vp(work.data_ptr()), c_vp(x.data_ptr()), float(rtol), int(k), _dblp(info),
                  ctx._stream())
        return rc, x.cpu().numpy().reshape(-1, 1), info

    def reference(k):
        return pcg_ref.pcg_iterate(lambda p: A @ p, M.apply, b.reshape(-1, 1), k)

    tag = 'fom {} kc={} coarse={}'.format(shape, kc, coarse)
    ctx.set_option('coarse', coarse)
    try:
        check_iterates(run, reference, tag)
        if tuple(shape) not in FOM_INDEFINITE:
            rc, x, info = run(100000, rtol=1e-12)
            assert rc == 0 and info[1] <= 1e-12, (rc, info)
            ref = spsolve(A.tocsc(), b.ravel())
            assert np.abs(x[:, 0] - ref).max() < 1e-8 * np.abs(ref).max()
        if M.has_coarse:
            ctx.set_option('coarse', 0)
            check_mutant(run, reference, tag)
    finally:
        ctx.set_option('coarse', 1)
