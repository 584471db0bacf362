"""The cells of tests/test_corrector_iterates_gpu.py and the corrector pieces of tests/pcg_ref.py, on the CPU.

- A mirror of ``launch_local_correction`` (csrc/enrich.hip; the internal one both exports go through): the nel ladder, the LDS byte count of ``launch_hood`` and the 160 KB
  refusal, read from the source.  The 2D cells must reach all five instantiations of ``k_hood_pcg``, both ends of the range of
  every instantiation above <1,640>, at least two shapes above 64 KB of LDS, the largest accepted template and a refused one.
- ``pcg_ref.hood_operator_2d`` on the oracle's blocks in the product's layouts equals the oracle's own neighbourhood system
  (``OracleDiscretization.local_correction_system``, assembled from scratch on the faces of the neighbourhood).
- Every reference operator is SPD (dense check where the neighbourhood is small enough) and every reference preconditioner
  symmetric.
- The cells can tell preconditioners apart: the reference iterate with the right M^-1 against the identity, block-Jacobi from the
  other set of blocks (3D: corrected, 2D: uncorrected) and the inverses of the centre subdomain in every slot.
- The rtol of the freeze tests is no knife edge: no reference ratio up to the last stop lies within 1e-6 (relative) of it."""
import functools
import os
import re

import numpy as np
import pytest

import common3d as c3
import pcg_ref
import test_corrector_iterates_gpu as cells
from test_enrichment3d_host import oracle as oracle_3d
from test_pcg_iterates_gpu import K_STEPS, MIN_RATIO, TOL_X

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pylrbms_amd', 'csrc', 'enrich.hip')
LDS_DEFAULT = 64 * 1024
SEPARATION = 1e3              # a mutant must move some x_k by more than this many iterate tolerances
DENSE_LIMIT = 2000            # unknowns up to which the SPD check is a dense eigenvalue computation


# ------------------------------------------------------------------------------------------------ the dispatch mirror
def _src():
    with open(SRC) as fh:
        return fh.read()


def ladder(src=None):
    """[(nel bound, EPT, BT), ...] of ``launch_local_correction``, in source order."""
    body = re.search(r'int launch_local_correction\(.*?\n}\n', src or _src(), re.S).group(0)
    return [(int(a), int(b), int(c)) for a, b, c in re.findall(r'if \(nel <= (\d+)\)\s*launch_hood<(\d+), (\d+)>', body)]


def form_of(n_T, src=None):
    """(EPT, BT) the host launches for a template of n_T elements, None if it refuses it as too large."""
    return next(((ept, bt) for bound, ept, bt in ladder(src) if 5 * n_T <= bound), None)


def lds_bytes(n_T, bt, src=None):
    """Dynamic LDS of ``launch_hood<EPT, BT>`` from its size expression."""
    expr = re.search(r'void launch_hood\(.*?const size_t lds = ([^;]*);', src or _src(), re.S).group(1)
    py = expr.replace('sizeof(double)', '8').replace('(size_t)', '').replace('ctx->t.n', 'n').replace('/', '//')
    return int(eval(py, {}, {'n': 3 * n_T, 'BT': bt}))


def refused(n_T, src=None):
    """The "does not fit in LDS" test of the host."""
    cond = re.search(r'if \(([^\n]*)\)\n\s*return lrbms_fail\(ctx, LRBMS_E_INVALID, "local_correction_solve: neighbourhood does not fit in LDS"\)',
                     src or _src()).group(1)
    py = cond.replace('sizeof(double)', '8').replace('(size_t)', '').replace('ctx->t.n', 'n')
    return bool(eval(py, {}, {'n': 3 * n_T}))


def n_T_of(shape, squares):
    assert squares % shape[0] == 0 and squares % shape[1] == 0
    return 8 * (squares // shape[0]) * (squares // shape[1])


def test_the_mirror_reads_the_ladder_of_the_source():
    lad = ladder()
    assert lad == [(640, 1, 640), (1024, 1, 1024), (2048, 2, 1024), (4096, 4, 1024), (8192, 8, 1024)]
    for bound, ept, bt in lad:
        assert ept * bt >= bound                             # every element of the largest template of a form has a thread
    assert lds_bytes(128, 640) == 8 * (5 * 384 + 30) and not refused(1352) and refused(1360)


def test_both_exports_reach_their_kernels_through_the_one_ladder():
    """The ladder is in the source once, in the internal ``launch_local_correction`` that ``ladder()`` reads; every kernel launch lies
    behind it, and each export calls that function exactly once."""
    src = _src()
    rungs = re.findall(r'if \(nel <= \d+\)\s*(\w+)<\d+, \d+>', src)
    assert rungs == ['launch_hood'] * len(ladder()) and len(rungs) == 5          # no rung outside the function ladder() reads
    assert len(re.findall(r'\blaunch_hood<', src)) == len(rungs)                 # and no instantiation beside the rungs
    launcher = re.search(r'void launch_hood\(.*?\n}\n', src, re.S).group(0)
    outside = src.replace(launcher, '')
    for kernel in ('k_hood_pcg', 'k_hood_euler'):
        assert len(re.findall(r'hipLaunchKernelGGL\(\(%s<EPT, BT>\)' % kernel, launcher)) == 1
        assert 'hipLaunchKernelGGL((%s' % kernel not in outside and '%s<<<' % kernel not in src
    assert src.count('const size_t lds =') == 1
    bodies = re.findall(r'\nint launch_local_correction(?:_euler)?\(.*?\n}\n', src, re.S)
    assert len(bodies) == 3 and 'launch_hood<' in bodies[0]                      # the shared function, then the two exports
    for body in bodies[1:]:
        calls = re.findall(r'\blaunch_local_correction\(', body[body.index('{'):])
        assert len(calls) == 1 and 'launch_hood' not in body and 'hipLaunchKernelGGL' not in body and 'nel' not in body


def test_2d_cells_reach_every_launch_form_on_both_sides():
    lad = ladder()
    hit = {}
    for shape, squares, marked in cells.CELLS_2D:
        n_T = n_T_of(shape, squares)
        assert not refused(n_T), (shape, squares)
        hit.setdefault(form_of(n_T), []).append(5 * n_T)
    assert set(hit) == {(ept, bt) for _, ept, bt in lad}, sorted(hit)
    assert 640 in hit[(1, 640)]                               # the edge of the first form
    # the largest template the host accepts ends the range of the last form (the LDS refusal comes before the element count)
    largest = max(n for n in range(8, 8192 // 5 + 1, 8) if not refused(n) and form_of(n))
    lower = 640
    for bound, ept, bt in lad[1:]:
        # nel is a multiple of 40 (n_T = 8 kx ky): a cell within the first and one within the last quarter of the range
        upper = min(bound, 5 * largest)
        nels, quarter = hit[(ept, bt)], (upper - lower) / 4.0
        assert any(n <= lower + quarter for n in nels) and any(n >= upper - quarter for n in nels), ((ept, bt), nels)
        lower = bound
    # the largest accepted template itself is a cell, and so is the idle-thread tail of <1,1024>
    assert 5 * largest in hit[(8, 1024)]
    assert any(0 < 1024 - n < 64 for n in hit[(1, 1024)])
    big = [n_T_of(s, q) for s, q, _ in cells.CELLS_2D if lds_bytes(n_T_of(s, q), form_of(n_T_of(s, q))[1]) > LDS_DEFAULT]
    assert len(big) >= 2 and {form_of(n) for n in big} >= {(4, 1024), (8, 1024)}, big
    assert lds_bytes(largest, 1024) == 162624
    n_T = n_T_of(*cells.REFUSED_2D)
    assert refused(n_T) and form_of(n_T) is not None         # refused for its LDS, not for its element count


def test_2d_cells_mark_a_corner_and_an_interior_subdomain():
    for shape, squares, marked in cells.CELLS_2D:
        nbr = np.asarray(cells.problem_2d(shape, squares)['grid'].neighbor_slots)
        assert sorted(int((nbr[ii] >= 0).sum()) for ii in marked) == [3, 5], (shape, marked)


def test_mirror_fails_on_a_new_launch_form():
    """A scratch copy of the source with one more instantiation: the cells do not reach it, and the check says so."""
    src = _src()
    new = src.replace('else if (nel <= 8192)', 'else if (nel <= 4200)\n    launch_hood<5, 1024>(ctx);\n  else if (nel <= 8192)', 1)
    assert new != src and (4200, 5, 1024) in ladder(new)
    hit = {form_of(n_T_of(s, q), new) for s, q, _ in cells.CELLS_2D}
    assert {(e, b) for _, e, b in ladder(new)} - hit == {(5, 1024)}


# ------------------------------------------------------------------------------------------------ 2D references on the CPU
def oracle_arrays_2d(p, o):
    """The oracle's SWIPDG blocks, the Dirichlet corrections of its coupling faces and its load vector in the product's layouts:
    A_diag [Q, S, n_T, 4, 9], A_cpl / D_corr [Q, S, 4, ncf, 9], b [S, n].  D_corr of a coupling face seen from an element is the
    Dirichlet-face block of that element minus the own / own block of the inner-face form that A_diag holds."""
    from pylrbms_amd.grid import SLOT_TO_SIDE
    grid, t, m, qd = p['grid'], p['grid'].template, o.mesh, o.quad
    S, nT, Q = o.S, t.n_T, o.Q
    nbr = np.asarray(grid.neighbor_slots)
    A_diag, A_cpl, D_corr = np.zeros((Q, S, nT, 4, 9)), np.zeros((Q, S, 4, t.ncf, 9)), np.zeros((Q, S, 4, t.ncf, 9))
    faces = np.nonzero(m.face_kind == 1)[0]
    for q, fn in enumerate(o.lambda_funcs):
        for s in range(S):
            own = o.block(o.A[q], s, s).toarray().reshape(nT, 3, nT, 3)
            A_diag[q, s, :, 0] = own[np.arange(nT), :, np.arange(nT), :].reshape(nT, 9)
            for f in range(3):
                nb = t.nb_elem[:, f]
                ok = np.nonzero(nb >= 0)[0]
                A_diag[q, s, ok, 1 + f] = own[ok, :, nb[ok], :].reshape(-1, 9)
            for side, slot in enumerate((0, 1, 3, 4)):
                s2, cnt = int(nbr[s, slot]), int(t.side_count[side])
                if s2 >= 0:
                    blk = o.block(o.A[q], s, s2).toarray().reshape(nT, 3, nT, 3)
                    A_cpl[q, s, side, :cnt] = blk[t.side_elem[side, :cnt], :, t.side_elem_out[side, :cnt], :].reshape(cnt, 9)
        mm, _, _, pp = o._swipdg_face_blocks(fn, qd.system_coupling_face, faces)
        for which, inner, (E, fl), (E2, _) in (('minus', mm, m.face_minus[faces].T, m.face_plus[faces].T),
                                               ('plus', pp, m.face_plus[faces].T, m.face_minus[faces].T)):
            corr = o._swipdg_boundary_block(fn, qd.system_boundary_face, faces, which) - inner
            for k in range(len(faces)):
                s, e, s2 = int(m.elem_subdomain[E[k]]), int(m.elem_local[E[k]]), int(m.elem_subdomain[E2[k]])
                side = SLOT_TO_SIDE[int(np.nonzero(nbr[s] == s2)[0][0])]
                f = int(np.nonzero(t.nb_elem[e] == -(1 + side))[0][0])
                D_corr[q, s, side, t.elem_side_pos[e, f]] = corr[k].ravel()
    return A_diag, A_cpl, D_corr, o.b.reshape(S, t.n)


@functools.lru_cache(maxsize=None)
def model_2d(shape, squares):
    from common import oracle_from_problem, theta_of
    p = cells.problem_2d(shape, squares)
    o = oracle_from_problem(p)
    return p, o, oracle_arrays_2d(p, o), theta_of(p, cells.MU_2D)


@functools.lru_cache(maxsize=None)
def refs_2d(shape, squares, marked):
    p, o, arrays, theta = model_2d(shape, squares)
    nbr = np.asarray(p['grid'].neighbor_slots)
    return [cells.reference_2d(*arrays, theta, p['grid'].template, nbr, ii) for ii in marked]


@functools.lru_cache(maxsize=None)
def refs_3d(name):
    o = oracle_3d(name)                      # the cache of tests/test_enrichment3d_host.py: one oracle per problem and session
    return [cells.reference_3d(o, ii, c3.PROBLEMS[name][6]) for ii in range(o.S)]


CELLS_2D_AND_FREEZE = cells.CELLS_2D + (cells.FREEZE_2D[:3],)


@pytest.mark.parametrize('shape, squares, marked', [cells.CELLS_2D[0], cells.CELLS_2D[1], cells.CELLS_2D[5]])
def test_hood_operator_2d_is_the_oracle_neighbourhood_system(shape, squares, marked):
    """Square and oblong subdomains, every subdomain of the grid: corner, edge and interior neighbourhoods."""
    p, o, arrays, theta = model_2d(shape, squares)
    t, nbr = p['grid'].template, np.asarray(p['grid'].neighbor_slots)
    assert np.abs(arrays[2]).max() > 1e-3 * np.abs(arrays[0]).max()          # the correction is not negligible
    for ii in range(o.S):
        A, dofs = pcg_ref.hood_operator_2d(*arrays[:3], theta, t, nbr, ii)
        want, b, hood, want_dofs = o.local_correction_system(ii, cells.MU_2D)
        assert np.array_equal(dofs, want_dofs) and hood == [int(k) for k in nbr[ii] if k >= 0]
        assert abs(A - want).max() <= 1e-13 * abs(want).max(), ii
    # without D_corr the operator is another one: the uncorrected mutant below is a real mutant
    A0, _ = pcg_ref.hood_operator_2d(arrays[0], arrays[1], 0.0 * arrays[2], theta, t, nbr, marked[1])
    A1, _ = pcg_ref.hood_operator_2d(*arrays[:3], theta, t, nbr, marked[1])
    assert abs(A1 - A0).max() > 1e-3 * abs(A1).max()


def _check_spd(ref, tag):
    assert abs(ref.A - ref.A.T).max() <= 1e-12 * abs(ref.A).max(), tag
    assert np.abs(ref.Minv - ref.Minv.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(ref.Minv).max(), tag
    assert np.linalg.eigvalsh(ref.Minv).min() > 0.0, tag
    if ref.A.shape[0] <= DENSE_LIMIT:
        lo, asym = pcg_ref.spd_check(ref.A.toarray())
        assert lo > 0.0 and asym <= 1e-12, (tag, lo, asym)
        return 1
    return 0


def test_2d_reference_operators_are_spd_and_their_preconditioners_symmetric():
    dense = sum(_check_spd(ref, (shape, squares, ii)) for shape, squares, marked in CELLS_2D_AND_FREEZE
                for ii, ref in zip(marked, refs_2d(shape, squares, marked)))
    assert dense >= 3


@pytest.mark.parametrize('name', sorted(cells.CELLS_3D))
def test_3d_reference_operators_are_spd_and_their_preconditioners_symmetric(name):
    refs = refs_3d(name)
    # cfg5_template: 2 x 3 840 unknowns per neighbourhood -- one dense check, of the first subdomain, on the Cholesky factor
    for ii, ref in enumerate(refs):
        if not _check_spd(ref, (name, ii)) and ii == 0:
            np.linalg.cholesky(ref.A.toarray())


# ------------------------------------------------------------------------------------------------ the cells see the preconditioner
def _separation(ref, mutant, steps):
    """Largest relative distance over ``steps`` between the own part of x_k with the cell's preconditioner and with ``mutant``."""
    X, _ = ref.history(max(steps))
    Y, _ = ref.history(max(steps), Minv=mutant)
    return max(float(np.linalg.norm(Y[k - 1] - X[k - 1]) / np.linalg.norm(X[k - 1])) for k in steps)


def _centre_everywhere(ref, block):
    """The inverse blocks of the marked subdomain in every slot (members are consecutive, equally long)."""
    centre = ref.Minv[ref.own[0] // block:ref.own[-1] // block + 1]
    return np.concatenate([centre] * (ref.Minv.shape[0] // centre.shape[0]))


@pytest.mark.parametrize('shape, squares, marked', cells.CELLS_2D)
def test_2d_cells_tell_preconditioners_apart(shape, squares, marked):
    p, o, arrays, theta = model_2d(shape, squares)
    t, nbr = p['grid'].template, np.asarray(p['grid'].neighbor_slots)
    for ii, ref in zip(marked, refs_2d(shape, squares, marked)):
        A0, _ = pcg_ref.hood_operator_2d(arrays[0], arrays[1], 0.0 * arrays[2], theta, t, nbr, ii)
        mutants = {'identity': (None,), 'uncorrected blocks': pcg_ref.hood_block_jacobi_2d(A0),
                   'centre inverses in every slot': _centre_everywhere(ref, 3)}
        for what, mutant in mutants.items():
            sep = _separation(ref, mutant, K_STEPS)
            assert sep > SEPARATION * TOL_X, (shape, squares, ii, what, sep)


@pytest.mark.parametrize('name', sorted(cells.CELLS_3D))
def test_3d_cells_tell_preconditioners_apart(name):
    for ii, ref in enumerate(refs_3d(name)):
        mutants = {'identity': (None,), 'corrected blocks': np.linalg.inv(pcg_ref.diagonal_blocks(ref.A, 10)),
                   'centre inverses in every slot': _centre_everywhere(ref, 10)}
        for what, mutant in mutants.items():
            sep = _separation(ref, mutant, cells.CELLS_3D[name])
            assert sep > SEPARATION * cells.TOL_X3, (name, ii, what, sep)


def test_3d_tolerances_respect_their_cap():
    assert 0.0 < cells.TOL_X3 <= 1e-8 and 0.0 < cells.TOL_RES3 <= cells.TOL_RES3_FREEZE <= 1e-8


def test_every_k_of_every_cell_is_checked():
    """``check_iterates`` stops at the first k whose reference ratio is below MIN_RATIO: no cell loses a k to that."""
    for shape, squares, marked in cells.CELLS_2D:
        for ref in refs_2d(shape, squares, marked):
            assert ref.history(max(K_STEPS))[1].min() >= MIN_RATIO, (shape, squares)
    for name, steps in cells.CELLS_3D.items():
        for ref in refs_3d(name):
            assert ref.history(max(steps))[1].min() >= MIN_RATIO, name


# ------------------------------------------------------------------------------------------------ the freeze tests' rtol
def _check_gap(refs, rtol, tag):
    stops = [ref.stop(rtol)[0] for ref in refs]
    assert len(set(stops)) > 1, (tag, stops)
    assert 1e-4 <= rtol <= 1e-2
    for ref in refs:
        _, ratios = ref.history(max(stops))
        gap = np.abs(ratios / rtol - 1.0).min()
        assert gap > 1e-6, (tag, gap)
    return stops


def test_the_rtol_of_the_freeze_tests_is_no_knife_edge():
    shape, squares, marked, rtol = cells.FREEZE_2D
    stops = _check_gap(refs_2d(shape, squares, marked), rtol, '2D')
    print('2D stops', stops)
    name, rtol = cells.FREEZE_3D
    stops = _check_gap(refs_3d(name), rtol, '3D')
    print('3D stops', stops)
    assert max(stops) - min(stops) >= 2                       # room for a max_iter strictly between the first and the last stop
