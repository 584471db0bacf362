"""The NumPy PCG of tests/pcg_ref.py and the cells of tests/test_pcg_iterates_gpu.py, on the CPU.

- ``pcg_iterate`` equals the A-norm minimiser over K_k(M^-1 A, M^-1 b), computed independently in mpmath at 40 digits.
- The iterates see what a converged solution absorbs: an inverse diagonal block off by 1e-6, or a dropped coarse term.
- The restated preconditioners are SPD on a small oracle problem; the full-order one built blockwise equals the one built from
  the oracle's global sparse matrix.
- A mirror of the solver dispatch of csrc/online.hip (the ksc_n ladder, LRBMS_PANEL_DISPATCH, reduced_batch_group_width, the
  NM split of the VALU matvec, the LDS thresholds of k_bt_factor / k_bt_inverse / k_block_inverse, the coarse branches):
  the GPU file's cells must reach every instantiation and branch, so a new one without a cell fails here."""
import os
import re

import numpy as np
import pytest

import pcg_ref
import test_pcg_iterates_gpu as cells

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pylrbms_amd', 'csrc', 'online.hip')
LDS_DEFAULT = 64 * 1024


# ------------------------------------------------------------------------------------------------ the reference itself
def _random_spd(rng, n, cond):
    Qm, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (Qm * np.geomspace(1.0, cond, n)) @ Qm.T


def _krylov_minimiser_mp(A, Minv, b, k):
    """x_k = K (K^T A K)^-1 K^T b with K = [M^-1 b, (M^-1 A) M^-1 b, ...] (k columns), all in mpmath at 40 digits."""
    import mpmath
    mpmath.mp.dps = 40
    Am, Mm, bm = mpmath.matrix(A.tolist()), mpmath.matrix(Minv.tolist()), mpmath.matrix(b.tolist())
    cols = [Mm * bm]
    for _ in range(k - 1):
        cols.append(Mm * (Am * cols[-1]))
    n = len(b)
    K = mpmath.matrix(n, k)
    for j, c in enumerate(cols):
        for i in range(n):
            K[i, j] = c[i]
    y = mpmath.lu_solve(K.T * Am * K, K.T * bm)
    return np.array([float(v) for v in K * y])


@pytest.mark.parametrize('n, m', [(6, 1), (23, 2), (60, 1)])
def test_pcg_iterate_is_the_krylov_a_norm_minimiser(n, m):
    rng = np.random.default_rng(n)
    A = _random_spd(rng, n, 50.0)
    Minv = _random_spd(rng, n, 10.0)
    B = rng.standard_normal((n, m))
    for k in range(1, min(8, n - 1) + 1):
        X, rel = pcg_ref.pcg_iterate(lambda p: A @ p, lambda r: Minv @ r, B, k)
        for j in range(m):
            ref = _krylov_minimiser_mp(A, Minv, B[:, j], k)
            assert np.linalg.norm(X[:, j] - ref) < 1e-12 * np.linalg.norm(ref), (n, k, j)
            assert abs(rel[j] - np.linalg.norm(B[:, j] - A @ ref) / np.linalg.norm(B[:, j])) < 1e-10 * rel[j] + 1e-15
    x1, r1 = pcg_ref.pcg_iterate(lambda p: A @ p, lambda r: Minv @ r, B[:, 0], 3)      # a 1-D right-hand side
    assert x1.shape == (n,) and isinstance(r1, float) and np.allclose(x1, pcg_ref.pcg_iterate(
        lambda p: A @ p, lambda r: Minv @ r, B[:, :1], 3)[0][:, 0], rtol=0, atol=0)
    Z = np.zeros((n, 2))
    Z[:, 1] = B[:, 0]
    X, rel = pcg_ref.pcg_iterate(lambda p: A @ p, lambda r: Minv @ r, Z, 2)              # a zero column stays zero
    assert not X[:, 0].any() and rel[0] == 0.0 and rel[1] > 0.0


# ------------------------------------------------------------------------------------------------ small oracle problem
_ORACLE = {}


def _oracle_model(N=3):
    """(p, d, B_sys [Q, S, 5, N, N], rhs [S, N]) of the multiscale problem on 3 x 2 subdomains with energy-orthonormal bases."""
    if N not in _ORACLE:
        from pylrbms_amd import multiscale_problem
        from common import energy_orthonormalize, make_bases, oracle_from_problem
        from oracle.lrbms import OracleReductor
        p = multiscale_problem.init_grid_and_problem({'num_subdomains': [3, 2], 'coarse_per_subdomain': 2})
        d = oracle_from_problem(p)
        V = energy_orthonormalize(make_bases(d.S, d.n, N, seed=2), d)
        rd = OracleReductor(d, [V[ii] for ii in range(d.S)]).reduce()
        nbr = np.asarray(p['grid'].neighbor_slots)
        B = np.zeros((d.Q, d.S, 5, N, N))
        for s in range(d.S):
            for slot, t in enumerate(nbr[s]):
                if t >= 0:
                    for q in range(d.Q):
                        B[q, s, slot] = rd.op[s][int(t)][q]
        _ORACLE[N] = (p, d, B, np.stack(rd.rhs), nbr, rd)
    return _ORACLE[N]


def test_reduced_operator_is_the_oracle_reduced_system():
    p, d, B, rhs, nbr, rd = _oracle_model()
    A = pcg_ref.reduced_operator(pcg_ref.combine_reduced(B, d.theta(0.37)), nbr).toarray()
    Aref, bref, _ = rd.assemble(0.37)
    assert np.abs(A - Aref).max() <= 1e-14 * np.abs(Aref).max()
    assert np.array_equal(rhs.ravel(), bref)


def test_restated_preconditioners_are_spd():
    p, d, B, rhs, nbr, rd = _oracle_model()
    Amu = pcg_ref.combine_reduced(B, d.theta(0.37))
    for coarse in (0, 1):
        M = pcg_ref.ReducedPrecond(Amu, nbr, coarse)
        assert M.has_coarse == (coarse == 1)
        lo, asym = pcg_ref.spd_check(pcg_ref.precond_matrix(M.apply, rhs.size))
        assert lo > 0.0 and asym < 1e-12, (coarse, lo, asym)
    A = d.assemble_global(0.37)
    for coarse in (0, 1):
        F = pcg_ref.FomPrecond(A, d.S, d.n, coarse)
        lo, asym = pcg_ref.spd_check(pcg_ref.precond_matrix(F.apply, d.S * d.n))
        assert lo > 0.0 and asym < 1e-12, (coarse, lo, asym)


def test_full_order_preconditioner_blockwise_equals_global():
    """Minv from the 3 x 3 diagonal element blocks of the oracle's local matrices and A0[s, t] = 1^T A_st 1 from its
    subdomain blocks (the rule of k_fom_combine / k_fom_coarse_entries) against FomPrecond on the global sparse matrix."""
    p, d, B, rhs, nbr, rd = _oracle_model()
    th = d.theta(0.37)
    A = d.assemble_global(0.37)
    F = pcg_ref.FomPrecond(A, d.S, d.n)
    Minv, A0 = [], np.zeros((d.S, d.S))
    for s in range(d.S):
        Ass = sum(th[q] * d.block(d.A[q], s, s) for q in range(d.Q)).toarray()
        Minv += [np.linalg.inv(Ass[3 * e:3 * e + 3, 3 * e:3 * e + 3]) for e in range(d.n // 3)]
        for t in nbr[s]:
            if t >= 0:
                A0[s, int(t)] = sum(th[q] * d.block(d.A[q], s, int(t)) for q in range(d.Q)).sum()
    assert np.abs(np.stack(Minv) - F.Minv).max() <= 1e-12 * np.abs(F.Minv).max()
    assert np.abs(A0 - F.A0).max() <= 1e-12 * np.abs(A0).max()


def test_iterates_see_a_small_preconditioner_error():
    """x_1 .. x_3 move by more than 1e-8 (relative, on the subdomain of the fault; 10 x the GPU tolerance overall) when one D^-1 entry moves by 1e-6, and
    by more than 1e-3 when the coarse term is dropped: the GPU tolerance of 1e-10 sees both; the converged solution does not."""
    p, d, B, rhs, nbr, rd = _oracle_model()
    Amu = pcg_ref.combine_reduced(B, d.theta(0.37))
    A = pcg_ref.reduced_operator(Amu, nbr)
    M = pcg_ref.ReducedPrecond(Amu, nbr)
    assert M.has_coarse
    bad = pcg_ref.ReducedPrecond(Amu, nbr)
    bad.Dinv = bad.Dinv.copy()
    bad.Dinv[2, 0, 0] *= 1.0 + 1e-6                      # one entry of one inverse diagonal block, off by 1e-6
    no_coarse = pcg_ref.ReducedPrecond(Amu, nbr, coarse=0)
    b = rhs.ravel()
    own = slice(2 * rhs.shape[1], 3 * rhs.shape[1])
    for k in (1, 2, 3):
        x, _ = pcg_ref.pcg_iterate(lambda v: A @ v, M.apply, b, k)
        y, _ = pcg_ref.pcg_iterate(lambda v: A @ v, bad.apply, b, k)
        assert np.linalg.norm(y[own] - x[own]) > 1e-8 * np.linalg.norm(x[own]), k
        assert np.linalg.norm(y - x) > 10 * cells.TOL_X * np.linalg.norm(x), k
        y, _ = pcg_ref.pcg_iterate(lambda v: A @ v, no_coarse.apply, b, k)
        assert np.linalg.norm(y - x) > 1e-3 * np.linalg.norm(x), k
    # converged: the same solution whatever the (SPD) preconditioner
    x, _ = pcg_ref.pcg_iterate(lambda v: A @ v, M.apply, b, b.size)
    y, _ = pcg_ref.pcg_iterate(lambda v: A @ v, no_coarse.apply, b, b.size)
    assert np.linalg.norm(y - x) < 1e-9 * np.linalg.norm(x)


def test_zero_padded_column_decouples():
    p, d, B, rhs, nbr, rd = _oracle_model()
    Bp = B.copy()
    Bp[:, 1, :, 2, :] = 0.0                                  # subdomain 1 pads its last column
    for s in range(d.S):
        for slot, t in enumerate(nbr[s]):
            if t == 1:
                Bp[:, s, slot, :, 2] = 0.0
    Amu = pcg_ref.combine_reduced(Bp, d.theta(0.37))
    M = pcg_ref.ReducedPrecond(Amu, nbr)
    assert M.Dinv[1, 2, 2] == 1.0 and not M.Dinv[1, 2, :2].any()
    b = rhs.copy()
    b[1, 2] = 0.0
    x, _ = pcg_ref.pcg_iterate(lambda v: pcg_ref.reduced_operator(Amu, nbr) @ v, M.apply, b.ravel(), 3)
    assert x.reshape(b.shape)[1, 2] == 0.0


# ------------------------------------------------------------------------------------------------ the dispatch mirror
def _src():
    return open(SRC).read()


def ksc_ladder(src=None):
    """[(N bound, ksc_n), ...], default of ``const int ksc_n = N <= 16 ? 4 : ... : 16;``."""
    src = src or _src()
    expr = re.search(r'const int ksc_n = ([^;]*);', src).group(1)
    steps = [(int(a), int(b)) for a, b in re.findall(r'N <= (\d+) \? (\d+)', expr)]
    return steps, int(re.search(r': (\d+)\s*$', expr).group(1))


def ksc_of(N, src=None):
    steps, last = ksc_ladder(src)
    return next((v for bound, v in steps if N <= bound), last)


def panel_instantiations(src=None):
    """{(GW, ksc, CT)} that LRBMS_PANEL_DISPATCH launches, with the ksc_n each is chosen for (per GW branch)."""
    src = src or _src()
    body = re.search(r'#define LRBMS_PANEL_DISPATCH\(X\)(.*?)while \(0\)', src, re.S).group(1)
    branches = re.findall(r'if \(ksc_n == (\d+)\) X\((\d+), (\d+), (\d+)\)|else X\((\d+), (\d+), (\d+)\)', body)
    out = set()
    for a, g1, k1, c1, g2, k2, c2 in branches:
        if a:
            assert int(a) == int(k1), 'LRBMS_PANEL_DISPATCH: ksc_n == {} launches KSC = {}'.format(a, k1)
            out.add((int(g1), int(k1), int(c1)))
        else:
            out.add((int(g2), int(k2), int(c2)))
    return out


def group_width(nmu, valu, src=None):
    src = src or _src()
    body = re.search(r'static int reduced_batch_group_width\(.*?\n}\n', src, re.S).group(0)
    a, w16 = map(int, re.search(r'nmu <= (\d+)\) return (\d+);', body).groups())
    b, w32, w64 = map(int, re.search(r'return nmu <= (\d+) \? (\d+) : (\d+);', body).groups())
    if valu or nmu <= a:
        return w16
    return w32 if nmu <= b else w64


def valu_split(src=None):
    return int(re.search(r'else if \(NM <= (\d+)\)', src or _src()).group(1))


def _lds(expr, **var):
    """Bytes of an LDS size expression of the source (``sizeof(double) * (...)``) at the given variable values."""
    py = expr.replace('sizeof(double)', '8').replace('(size_t)', '')
    return int(eval(py, {}, var))


def lds_formulas(src=None):
    src = src or _src()
    f = re.search(r'lds_f = ([^,]*), lds_i = ([^;]*);', src)
    blk = re.search(r'static int launch_block_inverse\(.*?const size_t lds = ([^;]*);', src, re.S).group(1)
    return f.group(1), f.group(2), blk


def coarse_limits(src=None):
    src = src or _src()
    lo, hi = map(int, re.search(r'opt_coarse == 0 \|\| S < (\d+) \|\| S > (\d+)\) return LRBMS_OK', src).groups())
    band = int(re.search(r'if \(bw <= (\d+) && ctx->opt_coarse != 2\)', src).group(1))
    return lo, hi, band


def band_of(shape):
    """Largest distance between neighbours in the row-by-row subdomain numbering (coarse_finish)."""
    nx, ny = shape
    return nx if ny > 1 else (1 if nx > 1 else 1)


def coarse_branch(shape, coarse=1, src=None):
    lo, hi, band = coarse_limits(src)
    S = shape[0] * shape[1]
    if coarse == 0 or S < lo or S > hi:
        return ('none', S < lo, S > hi)
    b = band_of(shape)
    if b > band or coarse == 2:
        return ('rocsolver',)
    ff, fi, _ = lds_formulas(src)
    return ('bt', b == 1, _lds(ff, b=b) > LDS_DEFAULT, _lds(fi, b=b) > LDS_DEFAULT, b == band)


def batch_kernels(N, nmu, valu, Q=2, src=None):
    """Kernel instances one batched call launches (per group)."""
    GW = group_width(nmu, valu, src)
    out = set()
    groups = [min(GW, nmu - g) for g in range(0, nmu, GW)]
    if valu:
        out |= {('k_bcg_matvec', 3 if N * nm <= valu_split(src) else 'BCG_KMAX') for nm in groups}
        out.add(('k_bcg_update',))
    elif GW == 16:
        out |= {('k_bcg_matvec_mfma', 16), ('k_bcg_update_mfma', 16)}
    else:
        out |= {('k_bcg_matvec_panel', GW, ksc_of(N, src), 1), ('k_bcg_update_mfma', GW)}
    out |= {('k_coarse_apply', (nm + 15) // 16) for nm in groups}
    if len(groups) > 1:
        out.add(('k_bcg_scatter',))
    return out


def _batch_cells():
    yield from ((N, nmu, False) for N, nmu in cells.BATCH_CELLS)
    yield from ((N, nmu, True) for N, nmu in cells.VALU_CELLS)
    N, nmu, _ = cells.SRC_CELL
    yield N, nmu, False


def test_ladder_and_dispatch_agree():
    insts = panel_instantiations()
    steps, last = ksc_ladder()
    kscs = {v for _, v in steps} | {last}
    assert insts == {(gw, k, 1) for gw in (32, 64) for k in kscs}, sorted(insts)
    assert group_width(1, False) == 16 and group_width(17, True) == 16


def test_cells_reach_every_panel_instantiation_and_update():
    hit = set().union(*(batch_kernels(N, nmu, valu) for N, nmu, valu in _batch_cells()))
    for N, nmu, _ in _batch_cells():
        assert 1 <= N <= 64 and 1 <= nmu <= 64
    panels = {('k_bcg_matvec_panel',) + i for i in panel_instantiations()}
    want = panels | {('k_bcg_matvec_mfma', 16), ('k_bcg_matvec', 3), ('k_bcg_matvec', 'BCG_KMAX'), ('k_bcg_update',),
                     ('k_bcg_scatter',)} | {('k_bcg_update_mfma', w) for w in (16, 32, 64)} | \
        {('k_coarse_apply', y) for y in (1, 2, 3, 4)}
    missed = want - hit
    assert not missed, 'no cell of test_pcg_iterates_gpu.py launches: {}'.format(sorted(missed))
    # the nmu the issue of this file names: 1, 16, 17, 32, 33, 47, 64 and a partly filled 64-wide panel
    nmus = {nmu for _, nmu, _ in _batch_cells()}
    assert {1, 16, 17, 32, 33, 47, 64} <= nmus
    # the panels of 64 at every ksc (17 <= N <= 32 and 41 <= N <= 48 included), NM on both sides of the VALU split
    assert {ksc_of(N) for N, nmu, v in _batch_cells() if not v and group_width(nmu, v) == 64} == \
        {k for g, k, _ in panel_instantiations() if g == 64}
    split = valu_split()
    nms = {N * min(16, nmu - g) for N, nmu, v in _batch_cells() if v for g in range(0, nmu, 16)}
    assert any(x <= split for x in nms) and any(x > split for x in nms) and split in nms


def test_cells_reach_every_coarse_branch():
    lo, hi, band = coarse_limits()
    ff, fi, _ = lds_formulas()
    single = [shape for shape, _ in cells.SINGLE_GRIDS]
    hit = {coarse_branch(s) for s in single} | {coarse_branch(cells.SWEEP_GRID, c) for c in (0, 2)}
    kinds = {h[0] for h in hit}
    assert kinds == {'none', 'bt', 'rocsolver'}
    assert ('none', True, False) in hit and ('none', False, True) in hit, 'S < {} and S > {}'.format(lo, hi)
    assert any(shape[0] * shape[1] == hi for shape in single), 'S = {} (the limit)'.format(hi)
    bt = [h for h in hit if h[0] == 'bt']
    assert any(h[1] for h in bt), 'b = 1'
    assert any(h[4] for h in bt), 'b = {}'.format(band)
    assert any(band_of(s) == band + 1 and lo <= s[0] * s[1] <= hi for s in single), 'b = {} (rocSOLVER)'.format(band + 1)
    # each side of each LDS threshold: the largest b below and the smallest b above are both cells
    bands = {band_of(s) for s in single}
    for expr in (ff, fi):
        first = next(b for b in range(1, band + 1) if _lds(expr, b=b) > LDS_DEFAULT)
        assert {first - 1, first} <= bands, (expr, first)


def test_cells_reach_block_inverse_threshold_and_both_parities():
    _, _, blk = lds_formulas()
    first = next(N for N in range(1, 65) if _lds(blk, N=N) > LDS_DEFAULT)
    Ns = set(cells.SINGLE_N)
    assert {first - 1, first} <= Ns
    assert any(N % 2 for N in Ns) and any(N % 2 == 0 for N in Ns)
    assert {2, 3} & {N for _, N in cells.SINGLE_GRIDS}


def test_mirror_fails_on_a_new_dispatch_line():
    """A scratch copy of the source with one more panel instantiation makes the coverage check fail."""
    src = _src()
    new = src.replace('else X(64, 16, 1);', 'else if (ksc_n == 14) X(64, 14, 1); else X(64, 16, 1);', 1)
    new = new.replace('N <= 48 ? 12 :', 'N <= 48 ? 12 : N <= 56 ? 14 :', 1)
    assert new != src
    hit = set().union(*({('k_bcg_matvec_panel', group_width(nmu, v), ksc_of(N), 1)} for N, nmu, v in _batch_cells()
                        if not v and group_width(nmu, v) > 16))
    insts = {('k_bcg_matvec_panel',) + i for i in panel_instantiations(new)}
    assert insts - hit == {('k_bcg_matvec_panel', 64, 14, 1)}


def test_full_order_cells():
    """n_T = 8 k_c^2: 32 (no whole wave per subdomain: k_fom_restrict), 128 and 512 (wave sums: k_fom_coarse1 with 2 and 8
    waves); a grid without a coarse level, a band of 64, and the coarse level switched off."""
    nTs = {8 * kc * kc for _, kc, _ in cells.FOM_CELLS}
    assert any(n % 64 for n in nTs) and {n // 64 for n in nTs if n % 64 == 0} >= {2, 8}
    assert any(s[0] * s[1] < 4 for s, _, _ in cells.FOM_CELLS)
    assert any(c == 0 for _, _, c in cells.FOM_CELLS) and any(band_of(s) == 64 for s, _, _ in cells.FOM_CELLS)
