"""The PCG iterates of the neighbourhood corrector solvers against a NumPy PCG with the same operator and preconditioner.

Online enrichment solves its corrector problems with a solver of its own on each path: in 2D ``k_hood_pcg`` (csrc/enrich.hip, one
workgroup per marked subdomain), in 3D the batched multi-kernel PCG ``k3l_*`` behind ``lrbms3_local_correction_solve``
(csrc/enrich3d.hip).  Both are plain PCG from x_0 = 0 with a pure block-Jacobi preconditioner.  A converged corrector does not
depend on that preconditioner, so this module does what tests/test_pcg_iterates_gpu.py does for the other solvers: the raw export
is called with max_iter = k, it returns LRBMS_E_NOT_CONVERGED and leaves x_k (its part on the marked subdomain) and
info = (k, |r_k| / |b|) behind, and tests/pcg_ref.py computes the same x_k in NumPy.

2D.  The operator is ``pcg_ref.hood_operator_2d`` on the arrays the product assembled (A_diag, A_cpl, D_corr), the preconditioner the
inverse of its 3 x 3 diagonal blocks, the tolerances TOL_X / TOL_RES of test_pcg_iterates_gpu.py.  ``launch_local_correction`` picks one
of five instantiations of ``k_hood_pcg`` by nel = 5 n_T; a subdomain of kx x ky coarse squares has n_T = 8 kx ky elements (eight
triangles per square, whatever the grid), so nel is a multiple of 40 and CELLS_2D names, per cell, the grid and the global number of
coarse squares per direction that give the wanted (kx, ky): both ends of the range of every instantiation, the edge nel = 640, three
shapes whose dynamic LDS passes 64 KB and the largest template the host accepts (13 x 13 squares: n_T = 1 352, 162 624 B).  One
corner and one interior subdomain are marked: two workgroups, with 3 and 5 present slots.  REFUSED_2D (14 x 14 squares) must come
back as LRBMS_E_INVALID before anything is launched.  tests/test_corrector_iterates_host.py mirrors the dispatch and proves on the CPU
which instantiation each cell reaches.

3D.  The operator is the oracle's ``enrichment3d_ref.hood_system``, the preconditioner the inverse of the 10 x 10 element blocks
of the UNCORRECTED system matrix (the library's documented choice).  Every subdomain of the common3d problem is marked in one
call.  The product's arrays match the oracle's to <= 1e-11 only, so the 3D tolerances are measured, not derived: on an MI355X the
worst deviation over all 3D cells, problems and k in K_STEPS was 3.72e-15 for x_k (relative, l2, own part; interior_3x3x3) and
3.45e-15 for the ratio (q3_2x1x2); TOL_X3 and TOL_RES3 are ten times these.  The freeze test reads iterates 15 .. 19 at ratios just
below 1e-3: x_{j_m} deviated by 1.84e-15 at the worst (TOL_X3 holds), the ratio by 1.41e-13.  The recurrence residual of both
sides carries a rounding error of a few eps |b| whatever |r_k| has become, so the RELATIVE error of |r_k| / |b| grows like
eps / ratio (1.1e-16 / 8.2e-4 = 1.4e-13: one unit in the last place of |b|); the freeze checks compare the ratio with
TOL_RES3_FREEZE, ten times that measured worst and below the 19 eps / 5e-4 = 4e-12 of this estimate.

Freeze.  A problem that reaches rtol keeps its iterate while the rest of the batch goes on (2D: the workgroup leaves its loop; 3D:
state sc[5] / sc[6] of ``k3l_reduce``, honoured by every other kernel).  With an rtol for which the reference problems stop at
different iterations j_m, one call must return x_{j_m} and info[m, 0] = j_m for every problem, and in 3D a call with max_iter
between min j_m and max j_m must hold the stopped problems at x_{j_m} and the others at x_{max_iter}.  The host module asserts
that no reference ratio lies within 1e-6 (relative) of rtol, so the stopping decision cannot flip."""
import functools

import numpy as np
import pytest

import pcg_ref
from test_pcg_iterates_gpu import E_NOT_CONVERGED, K_STEPS, TOL_RES, TOL_X, check_iterates

pytestmark = pytest.mark.gpu

E_INVALID = -1
MU_2D = 0.1
# (num_subdomains, global coarse squares per direction, marked subdomains): kx = squares / Px, ky = squares / Py
CELLS_2D = (
    ((3, 3), 12, (0, 4)),       # 4 x 4:   n_T =   128, nel =   640: <1,640>, the edge
    ((6, 3), 18, (0, 7)),       # 3 x 6:   n_T =   144, nel =   720: <1,1024> just above the threshold, 304 idle threads
    ((3, 3), 15, (0, 4)),       # 5 x 5:   n_T =   200, nel = 1 000: <1,1024>, 24 idle threads
    ((9, 3), 27, (0, 10)),      # 3 x 9:   n_T =   216, nel = 1 080: <2,1024>, the second element active in 56 threads only
    ((3, 3), 21, (0, 4)),       # 7 x 7:   n_T =   392, nel = 1 960: <2,1024> near its upper threshold
    ((6, 4), 36, (0, 7)),       # 6 x 9:   n_T =   432, nel = 2 160: <4,1024> just above the threshold
    ((3, 3), 30, (0, 4)),       # 10 x 10: n_T =   800, nel = 4 000: <4,1024> near its upper threshold, LDS 96 384 B
    ((4, 3), 36, (0, 5)),       # 9 x 12:  n_T =   864, nel = 4 320: <8,1024> just above the threshold, LDS 104 064 B
    ((3, 3), 39, (0, 4)),       # 13 x 13: n_T = 1 352, nel = 6 760: <8,1024>, LDS 162 624 B: the largest shape the host accepts
)
REFUSED_2D = ((2, 2), 28)       # 14 x 14: n_T = 1 568, 5 n doubles = 188 160 B: "does not fit in LDS"
FREEZE_2D = ((3, 3), 12, (0, 1, 4), 1e-3)             # grid, squares, marked (corner, edge, interior), rtol

# common3d problem -> the k it is checked at
CELLS_3D = {
    'interior_3x3x3': K_STEPS,      # 4, 5, 6 and 7 present slots; all 27 subdomains in one call
    'kc_3x1x2': K_STEPS,            # n_T = 36: the last chunk of FOM_EPB = 24 elements is partial
    'aniso_2x2x1': K_STEPS,         # n_T = 48: exactly two full chunks, anisotropic kappa
    'q3_2x1x2': K_STEPS,            # Q = 3
    'cfg5_template': (1, 2),        # n_T = 384, nbx = 16
}
FREEZE_3D = ('interior_3x3x3', 1e-3)
TOL_X3 = 3.7e-14             # ten times the measured worst (module docstring); never above 1e-8
TOL_RES3 = 3.5e-14
TOL_RES3_FREEZE = 1.4e-12      # the ratio of the iterates 15 .. 19 of the freeze test (module docstring)


# ------------------------------------------------------------------------------------------------------------- 2D
def problem_2d(shape, squares):
    from pylrbms_amd import OS2015_academic_problem
    return OS2015_academic_problem.init_grid_and_problem({'num_subdomains': list(shape),
                                                          'half_num_fine_elements_per_subdomain_and_dim': squares})


def reference_2d(A_diag, A_cpl, D_corr, b, theta, template, nbr, ii):
    """``pcg_ref.CorrectorRef`` of subdomain ii from assembled arrays (the product's on the GPU, the oracle's in the host tests)."""
    A, dofs = pcg_ref.hood_operator_2d(A_diag, A_cpl, D_corr, theta, template, nbr, ii)
    own = np.nonzero(dofs // template.n == ii)[0]
    return pcg_ref.CorrectorRef(A, np.asarray(b).reshape(-1)[dofs], own, pcg_ref.hood_block_jacobi_2d(A))


class _Model2D:
    """Engine of the cell with the arrays the corrector reads, and nothing else assembled."""

    def __init__(self, shape, squares):
        from pylrbms_amd.engine import Engine
        from common import theta_bar_of, theta_of
        p = problem_2d(shape, squares)
        lam = p['lambda']
        eng = Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'], theta_bar_of(p))
        c = eng.ctx
        self.ctx, self.t, self.nbr, self.Q = c, eng.t, np.asarray(p['grid'].neighbor_slots), eng.Q
        self.theta = np.ascontiguousarray(theta_of(p, MU_2D), dtype=np.float64)
        self.A_diag, self.A_cpl = c.assemble_swipdg(eng.lam)
        self.b = c.assemble_rhs(eng.f_smp, eng.lhat)[0]
        self.D_corr = c.assemble_dirichlet_correction(eng.lam)
        self.host = [x.cpu().numpy() for x in (self.A_diag, self.A_cpl, self.D_corr, self.b)]

    def reference(self, ii):
        return reference_2d(*self.host, self.theta, self.t, self.nbr, ii)

    def solve(self, marked, max_iter, rtol=1e-14):
        """One raw call -> (rc, corr [nmark, n], info [nmark, 2])."""
        from pylrbms_amd._native import _P_I32, _dblp, c_vp
        c = self.ctx
        mk = np.ascontiguousarray(marked, dtype=np.int32)
        work = c.empty(int(c.lib.lrbms_local_correction_work_size(c.handle, len(mk))))
        corr = c.zeros(len(mk), self.t.n)
        info = np.zeros((len(mk), 2))
        rc = c.lib.lrbms_local_correction_solve(c.handle, self.Q, _dblp(self.theta), len(mk), mk.ctypes.data_as(_P_I32),
                                                c_vp(self.A_diag.data_ptr()), c_vp(self.A_cpl.data_ptr()),
                                                c_vp(self.D_corr.data_ptr()), c_vp(self.b.data_ptr()), c_vp(work.data_ptr()),
                                                c_vp(corr.data_ptr()), float(rtol), int(max_iter), _dblp(info), c._stream())
        c.torch.cuda.synchronize(c.device)
        return rc, corr.cpu().numpy(), info


def _per_problem(solve, marked):
    """run(k) of ``check_iterates`` for problem j of the batch, one batched call per k."""
    calls = {}

    def column(j):
        def run(k):
            if k not in calls:
                calls[k] = solve(marked, k)
            rc, corr, info = calls[k]
            return rc, corr[j][:, None], info[j]
        return run
    return column


def _check_converged(solve, marked, refs, tag):
    rc, corr, info = solve(marked, 100000, rtol=1e-12)
    assert rc == 0 and (info[:, 1] <= 1e-12).all() and (info[:, 0] >= 1).all(), (tag, rc, info)
    for j, ref in enumerate(refs):
        want = ref.solve()
        assert np.abs(corr[j] - want).max() < 1e-8 * np.abs(want).max(), (tag, marked[j])


def _check_freeze(solve, marked, refs, rtol, tol_x, tol_res, tag):
    """One call with ample max_iter: every problem stops at its own j_m and holds x_{j_m}.  -> the j_m."""
    stops = [ref.stop(rtol)[0] for ref in refs]
    assert len(set(stops)) > 1, (tag, stops)
    rc, corr, info = solve(marked, 100000, rtol=rtol)
    assert rc == 0, (tag, rc)
    assert [int(v) for v in info[:, 0]] == stops, (tag, info[:, 0], stops)
    figures = []
    for j, (ref, jm) in enumerate(zip(refs, stops)):
        X, ratios = ref.history(jm + 1)
        err = np.linalg.norm(corr[j] - X[jm - 1]) / np.linalg.norm(X[jm - 1])
        later = np.linalg.norm(X[jm] - X[jm - 1]) / np.linalg.norm(X[jm - 1])
        res = abs(info[j, 1] - ratios[jm - 1]) / ratios[jm - 1]
        figures.append((marked[j], jm, err, res, later))
        print('CORRECTOR-FREEZE {} problem {}: j = {}, x_j error {:.2e}, ratio error {:.2e}, the next iterate is {:.2e} away'.format(
            tag, *figures[-1]))
    print('CORRECTOR-FREEZE {}: worst x_j error {:.2e}, worst ratio error {:.2e}'.format(tag, max(f[2] for f in figures),
                                                                                      max(f[3] for f in figures)))
    for ii, jm, err, res, later in figures:
        assert later > 1e3 * tol_x, (tag, ii, later)                        # the test can tell x_j from x_{j+1}
        assert err < tol_x and res < tol_res, (tag, ii, jm, err, res)
    return stops


@pytest.mark.parametrize('shape, squares, marked', CELLS_2D)
def test_hood_pcg_iterates_at_every_launch_form(shape, squares, marked):
    m = _Model2D(shape, squares)
    refs = [m.reference(ii) for ii in marked]
    assert sorted(len(r.b) // m.t.n for r in refs) == [3, 5]             # a corner and an interior neighbourhood
    column = _per_problem(m.solve, marked)
    for j, ii in enumerate(marked):
        check_iterates(column(j), refs[j].iterate, '2D {} x {} squares, subdomain {}'.format(m.t.kx, m.t.ky, ii))
    _check_converged(m.solve, marked, refs, (shape, squares))


def test_a_template_beyond_the_lds_limit_is_refused_before_any_launch():
    """Only the mesh is on the device: the call must not read an operator array, so it gets four doubles for each."""
    from pylrbms_amd._native import NativeContext, _P_I32, _dblp, c_vp
    shape, squares = REFUSED_2D
    grid = problem_2d(shape, squares)['grid']
    nbr = np.asarray(grid.neighbor_slots, dtype=np.int32)
    S = grid.num_subdomains
    c = NativeContext(0)
    c.mesh_upload(grid.template, np.eye(2), nbr, S, S)
    dummy, corr = c.zeros(4), c.zeros(4)
    mk, th, info = np.zeros(1, dtype=np.int32), np.ones(2), np.full((1, 2), -7.0)
    rc = c.lib.lrbms_local_correction_solve(c.handle, 2, _dblp(th), 1, mk.ctypes.data_as(_P_I32), c_vp(dummy.data_ptr()),
                                            c_vp(dummy.data_ptr()), c_vp(dummy.data_ptr()), c_vp(dummy.data_ptr()),
                                            c_vp(dummy.data_ptr()), c_vp(corr.data_ptr()), 1e-12, 10, _dblp(info), c._stream())
    c.torch.cuda.synchronize(c.device)
    assert rc == E_INVALID
    assert 'does not fit in LDS' in c.lib.lrbms_last_error(c.handle).decode()
    assert (info == -7.0).all() and not corr.cpu().numpy().any() and not dummy.cpu().numpy().any()


def test_hood_pcg_stops_every_problem_at_its_own_iteration():
    shape, squares, marked, rtol = FREEZE_2D
    m = _Model2D(shape, squares)
    _check_freeze(m.solve, marked, [m.reference(ii) for ii in marked], rtol, TOL_X, TOL_RES, '2D')


# ------------------------------------------------------------------------------------------------------------- 3D
def reference_3d(o, ii, mu, b=None):
    """``pcg_ref.CorrectorRef`` of subdomain ii of the oracle ``o``: hood_system, and block-Jacobi from the uncorrected blocks."""
    import enrichment3d_ref as ref
    dofs = ref.hood_dofs(o, ii)
    k = o.mesh.neighborhood_of(ii).index(ii)
    b = o.b if b is None else b
    return pcg_ref.CorrectorRef(ref.hood_system(o, ii, mu), b[dofs], np.arange(k * o.n, (k + 1) * o.n),
                                pcg_ref.hood_block_jacobi_3d(o.system_matrix(mu), dofs))


@functools.lru_cache(maxsize=None)
def _refs_3d(name):
    from test_enrichment3d_gpu import case
    p, o, _ = case(name)
    return [reference_3d(o, ii, p['mu']) for ii in range(o.S)]


def _solver_3d(name):
    from pylrbms_amd._native import _P_DBL, _P_I32, c_vp
    from test_enrichment3d_gpu import case
    p, o, d = case(name)
    eng = d.engine
    c, ops = eng.ctx, eng.ops
    theta = np.ascontiguousarray(d.theta(p['mu']), dtype=np.float64)

    def solve(marked, max_iter, rtol=1e-14):
        mk = np.ascontiguousarray(marked, dtype=np.int32)
        work = c.empty(c.local_correction_work_size(len(mk)))
        corr = c.zeros(len(mk), c.n)
        info = np.zeros((len(mk), 2))
        rc = c.lib.lrbms3_local_correction_solve(c.handle, eng.Q, theta.ctypes.data_as(_P_DBL), len(mk), mk.ctypes.data_as(_P_I32),
                                                 c_vp(ops['A_diag'].data_ptr()), c_vp(ops['A_cpl'].data_ptr()),
                                                 c_vp(ops['D_corr'].data_ptr()), c_vp(ops['b'].data_ptr()), c_vp(work.data_ptr()),
                                                 c_vp(corr.data_ptr()), float(rtol), int(max_iter), info.ctypes.data_as(_P_DBL),
                                                 c._stream())
        c.torch.cuda.synchronize(c.device)
        return rc, corr.cpu().numpy(), info
    return solve, list(range(o.S))


@pytest.mark.parametrize('name', sorted(CELLS_3D))
def test_batched_corrector_iterates_in_3d(name):
    solve, marked = _solver_3d(name)
    refs = _refs_3d(name)
    column = _per_problem(solve, marked)
    worst = np.zeros(2)
    for j, ii in enumerate(marked):
        worst = np.maximum(worst, check_iterates(column(j), refs[j].iterate, '3D {} subdomain {}'.format(name, ii), tol_x=TOL_X3,
                                                 tol_res=TOL_RES3, steps=CELLS_3D[name]))
    print('CORRECTOR-ITERATES 3D {}: worst x_k error {:.2e} (tolerance {:.1e}), worst ratio error {:.2e} (tolerance {:.1e})'.format(
        name, worst[0], TOL_X3, worst[1], TOL_RES3))
    _check_converged(solve, marked, refs, name)


def test_batched_corrector_freezes_every_problem_at_its_own_iteration():
    name, rtol = FREEZE_3D
    solve, marked = _solver_3d(name)
    refs = _refs_3d(name)
    stops = _check_freeze(solve, marked, refs, rtol, TOL_X3, TOL_RES3_FREEZE, '3D')
    # a call that ends between the first and the last stop: the stopped problems hold x_{j_m}, the others x_{max_iter}
    mid = (min(stops) + max(stops)) // 2
    assert min(stops) < mid < max(stops), stops
    rc, corr, info = solve(marked, mid, rtol=rtol)
    assert rc == E_NOT_CONVERGED
    frozen, figures = 0, []
    for j, (ref, jm) in enumerate(zip(refs, stops)):
        at = min(jm, mid)
        frozen += jm <= mid
        X, ratios = ref.history(at)
        assert int(info[j, 0]) == at, (marked[j], info[j], jm, mid)
        figures.append((marked[j], at, np.linalg.norm(corr[j] - X[at - 1]) / np.linalg.norm(X[at - 1]),
                        abs(info[j, 1] - ratios[at - 1]) / ratios[at - 1]))
    print('CORRECTOR-FREEZE 3D max_iter = {}: worst x error {:.2e}, worst ratio error {:.2e}'.format(
        mid, max(f[2] for f in figures), max(f[3] for f in figures)))
    for ii, at, err, res in figures:
        assert err < TOL_X3 and res < TOL_RES3_FREEZE, (ii, at, mid, err, res)
    assert 0 < frozen < len(marked)
