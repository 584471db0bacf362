"""Shared helpers of the quadrature rule-set tests (tests/test_quadrature_cases_host.py, tests/test_assembly_rules_gpu.py,
tests/test_assembly_rules3d_gpu.py).  Test infrastructure only.

The data functions here oscillate inside every element, so the samples of one record all differ: a wrong offset, point order or
rule length in a sample record changes the assembled array far beyond the parity tolerance.  The host tests assert that property
of the data on the oracle (``separation``), the GPU tests then compare the product with the oracle per rule set / degree.

2D rule sets (``RULE_SETS_2D``; ``spec_2d(name, cls)`` builds one with the product's or the oracle's ``QuadratureSpec``), 3D
degrees (``DEGREES_3D``), and the sample-record layouts with gaps that the C ABI admits (``padded_quadrature`` /
``PaddedSpec3D``)."""
import ctypes
import functools

import numpy as np

import common3d as c3

TOL = 1e-11                    # the parity tolerance of tests/test_parity_gpu.py and tests/test_parity3d_gpu.py
SEPARATION = 1e3               # two rule sets must move an array by at least SEPARATION * TOL for the parity test to tell them apart

# ----------------------------------------------------------------------------------------------------------------- 2D
CONTROL_2D = 'control'
RULE_SETS_2D = {
    'control': lambda S: S.dune(2, 2, 2, 2),
    'uniform5': lambda S: S.uniform(5),
    # odd orders: the order-3 rule with a negative weight, one-point energy_volume / elliptic_bar / ceps
    'odd': lambda S: S.dune(1, 1, 1, 1),
    # the lambda and lambda_hat records change length in opposite directions
    'lam0_hat2': lambda S: S.dune(0, 2, 0, 2),
    'lam2_hat0': lambda S: S.dune(2, 0, 2, 0),
    # every rule but df_bb has one point, nfs = 1
    'one_point': lambda S: S.uniform(1).with_(df_bb=2),
    # 16 points = LRBMS_MAXQV per triangle rule, 4 points = LRBMS_MAXQF per edge rule
    'max_points': lambda S: S.uniform(8).with_(system_inner_face=7, system_coupling_face=7, system_boundary_face=7,
                                               energy_face=7, flux_face=7),
    # nfs comes from the coupling rule: inner faces fill fewer than nfs slots (dune() never produces this)
    'coupling_gt_inner': lambda S: S.dune(2, 2, 2, 2).with_(system_inner_face=2, system_coupling_face=6, system_boundary_face=6),
}
DCORR_AND_SOURCE_SETS_2D = ('uniform5', 'max_points')
PADDED_SETS_2D = ('control', 'coupling_gt_inner')
N_2D, MU_2D = 6, 0.45


def spec_2d(name, cls=None):
    """The rule set ``name`` as a ``QuadratureSpec`` of ``cls`` (default: the product's; the oracle's has the same constructors)."""
    if cls is None:
        from pylrbms_amd.quadrature import QuadratureSpec as cls
    return RULE_SETS_2D[name](cls)


def oracle_spec_2d(name):
    from oracle.quadrature import QuadratureSpec
    return spec_2d(name, QuadratureSpec)


LAMBDAS_2D = ('1+0.6*sin(7*x[0])*cos(5*x[1])', '0.7+0.5*cos(6*x[0]+4*x[1])')
F_2D = 'exp(x[0])*cos(9*x[1])'
F_SECOND_2D = 'sin(8*x[0]-3*x[1])+0.5*x[0]*x[1]'          # second source component of the affine-source checks


def problem_2d():
    """6 subdomains of 2 x 2 coarse squares (n_T = 32) on [0, 3] x [0, 2], anisotropic constant tensor, Q = 2; every data function
    smooth and oscillating inside every element."""
    from pylrbms_amd.functions import make_constant_function_2x2, make_expression_function_1x1
    from pylrbms_amd.grid import DDSubdomainsGrid, make_boundary_info
    from pylrbms_amd.parameters import ExpressionParameterFunctional
    grid = DDSubdomainsGrid([0, 0], [3, 2], (6, 4), (3, 2))
    pt = {'diffusion': (1,)}
    total = '+'.join(LAMBDAS_2D)
    return {'grid': grid, 'boundary_info': make_boundary_info(grid, {'type': 'xt.grid.boundaryinfo.alldirichlet'}),
            'lambda': {'functions': [make_expression_function_1x1(grid, 'x', e, name='lambda_{}'.format(q))
                                     for q, e in enumerate(LAMBDAS_2D)],
                       'coefficients': [ExpressionParameterFunctional('1.', pt), ExpressionParameterFunctional('diffusion', pt)]},
            'lambda_bar': make_expression_function_1x1(grid, 'x', total, name='lambda_bar'),
            'lambda_hat': make_expression_function_1x1(grid, 'x', total, name='lambda_hat'),
            'kappa': make_constant_function_2x2(grid, [[2., 0.5], [0.5, 1.]]),
            'f': make_expression_function_1x1(grid, 'x', F_2D, name='f'),
            'parameter_type': pt, 'mu_bar': (1.,), 'mu_hat': (1.,), 'mu_min': (0.1,), 'mu_max': (1.,), 'parameter_range': (0.1, 1.)}


@functools.lru_cache(maxsize=None)
def oracle_2d(name):
    """(problem, oracle at the rule set ``name``), once per session."""
    from common import oracle_from_problem
    p = problem_2d()
    return p, oracle_from_problem(p, quad=oracle_spec_2d(name))


# assembled array of the 2D oracle -> the spec fields whose rules it is integrated with
ARRAY_RULES_2D = {
    'A_diag': ('system_volume', 'system_inner_face', 'system_coupling_face', 'system_boundary_face'),
    'A_cpl': ('system_coupling_face',),
    'b': ('rhs',), 'f2': ('f2',), 'ceps': ('ceps',),
    'P_diag': ('energy_volume', 'energy_face'), 'ebar': ('elliptic_bar',), 'F': ('flux_face',),
    'caa': ('df_aa',), 'Aab': ('df_ab',), 'Bbb': ('df_bb',),
}
EDGE_FIELDS_2D = ('system_inner_face', 'system_coupling_face', 'system_boundary_face', 'energy_face', 'flux_face')


def oracle_arrays_2d(p, d):
    """Every assembled array of the 2D oracle (dict of dense numpy arrays, one per key of ``ARRAY_RULES_2D``)."""
    grid, S, Q = p['grid'], d.S, d.Q
    nbr = np.asarray(grid.neighbor_slots)
    out = {'A_diag': np.stack([np.stack([d.block(d.A[q], ii, ii).toarray() for ii in range(S)]) for q in range(Q)]),
           'A_cpl': np.stack([np.stack([d.block(d.A[q], ii, int(jj)).toarray() for ii in range(S) for jj in nbr[ii] if jj >= 0 and jj != ii])
                              for q in range(Q)]),
           'b': np.asarray(d.b), 'f2': np.asarray(d.local_eta_rf_squared), 'ceps': np.asarray(d.min_diffusion_evs),
           'P_diag': np.stack([d.block(d.energy_product, ii, ii).toarray() for ii in range(S)]),
           'ebar': np.stack([d.block(d.elliptic_bar, ii, ii).toarray() for ii in range(S)]),
           'F': np.stack([d.F[q].toarray() for q in range(Q)]),
           'caa': np.stack([np.stack([d.caa[q][q2].toarray() for q2 in range(Q)]) for q in range(Q)]),
           'Aab': np.stack([np.asarray(d.ab_blocks[q]) for q in range(Q)]), 'Bbb': np.asarray(d.bb_blocks)}
    assert set(out) == set(ARRAY_RULES_2D)
    return out


def points_of_rule_2d(field, order):
    """The point set a requested order stands for (orders 0 / 1 and 6 / 7 share a triangle rule, edge rules go by point count)."""
    from oracle.quadrature import edge_rule, triangle_rule
    pts = edge_rule(order)[0] if field in EDGE_FIELDS_2D else triangle_rule(order)[0]
    return np.asarray(pts, dtype=np.float64)


def same_points_2d(field, a, b):
    pa, pb = points_of_rule_2d(field, a), points_of_rule_2d(field, b)
    return pa.shape == pb.shape and np.array_equal(pa, pb)


def flux_rows_dense(p, eng_F, m):
    """The product's flux coefficient rows F [Q, S, n_rt, 6] as dense [Q, S, n_rt, ndof] rows in the oracle's DoF numbering (``m``:
    the oracle mesh): row r of subdomain s holds F[..., :3] in the columns of element e0 of s and F[..., 3:] in those of element e1
    of s itself (inner face) or of the neighbour behind the side (coupling face); nothing on a physical side."""
    from pylrbms_amd.grid import SIDE_TO_SLOT
    grid, t = p['grid'], p['grid'].template
    F = np.asarray(eng_F, dtype=np.float64)
    Q, S = F.shape[:2]
    n, ndof = t.n, S * t.n
    nbr = np.asarray(grid.neighbor_slots)
    out = np.zeros((Q, S, t.n_rt, ndof))
    dropped = 0.0
    for s in range(S):
        for r in range(t.n_rt):
            e0, e1, side = int(t.rt_e0[r]), int(t.rt_e1[r]), int(t.rt_side[r])
            out[:, s, r, s * n + 3 * e0:s * n + 3 * e0 + 3] += F[:, s, r, :3]
            s1 = s if side < 0 else int(nbr[s, SIDE_TO_SLOT[side]])
            if s1 >= 0:
                out[:, s, r, s1 * n + 3 * e1:s1 * n + 3 * e1 + 3] += F[:, s, r, 3:]
            else:
                dropped = max(dropped, float(np.abs(F[:, s, r, 3:]).max()))
    return out, dropped


def oracle_flux_rows(d):
    """[Q, S, n_rt, ndof]: the oracle's flux rows of the RT faces of every subdomain, in its order of them."""
    return np.stack([np.stack([d.F[q][d.mesh.rt_faces[ii]].toarray() for ii in range(d.S)]) for q in range(d.Q)])


# ---- sample-record layouts with gaps (lrbms_set_quadrature validates every offset and stride with >=)
LAM_SEGMENTS = (('o_sysv', lambda q: q.system_volume.n), ('o_sysf', lambda q: 3 * q.nfs), ('o_enf', lambda q: 3 * q.energy_face.n),
                ('o_flf', lambda q: 3 * q.flux_face.n), ('o_env', lambda q: q.energy_volume.n))
LAMDF_SEGMENTS = (('o_aa', lambda q: q.df_aa.n), ('o_ab', lambda q: q.df_ab.n))
LHAT_SEGMENTS = (('o_haa', lambda q: q.df_aa.n), ('o_hab', lambda q: q.df_ab.n), ('o_hbb', lambda q: q.df_bb.n),
                 ('o_hceps', lambda q: q.ceps.n))
F_SEGMENTS = (('o_frhs', lambda q: q.rhs.n), ('o_ff2', lambda q: q.f2.n))
RECORDS_2D = {'lam': ('lam_stride', LAM_SEGMENTS), 'lam_df': ('lamdf_stride', LAMDF_SEGMENTS), 'lhat': ('lhat_stride', LHAT_SEGMENTS),
              'f_smp': ('f_stride', F_SEGMENTS), 'lbar': ('lbar_stride', ())}


def clone_quadrature(q):
    from pylrbms_amd.quadrature import NativeQuadrature
    out = NativeQuadrature()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(q), ctypes.sizeof(NativeQuadrature))
    return out


def padded_quadrature(q):
    """A copy of the packed ``NativeQuadrature`` q with the same rules and gaps in every record: segment k of a record starts
    1 + (k % 3) slots after the end of the one before (the first one after slot 0), every stride grows past the last segment;
    ``pad`` / ``pad_`` are left alone."""
    out = clone_quadrature(q)
    for stride, segments in RECORDS_2D.values():
        end = 0
        for k, (name, size) in enumerate(segments):
            setattr(out, name, end + 1 + (k % 3))
            end = getattr(out, name) + size(q)
        setattr(out, stride, (end if segments else getattr(q, stride)) + 2)
    return out


def relayout_record(x, q_from, q_to, record):
    """The samples x [..., stride of q_from] of ``record`` moved to the layout of q_to, NaN in every slot no segment covers."""
    stride, segments = RECORDS_2D[record]
    x = np.asarray(x, dtype=np.float64)
    assert x.shape[-1] == getattr(q_from, stride)
    out = np.full(x.shape[:-1] + (getattr(q_to, stride),), np.nan)
    if not segments:                                   # lambda_bar: one segment at slot 0
        out[..., :q_from.elliptic_bar.n] = x[..., :q_from.elliptic_bar.n]
    for name, size in segments:
        a, b, k = getattr(q_from, name), getattr(q_to, name), size(q_from)
        out[..., b:b + k] = x[..., a:a + k]
    return out


# ----------------------------------------------------------------------------------------------------------------- 3D
CONTROL_3D = 2
DEGREES_3D = (0, 1, 3, 4)
DEGREES_SECOND_GRID_3D = (1, 3)
DEGREES_EXPORTS_3D = (0, 4)
DEGREE_PADDED_3D = 1
ARRAYS_3D = ('A_diag', 'A_cpl', 'Cf', 'ebar', 'Aaa', 'Aab', 'Bbb', 'P_diag', 'b', 'f2', 'ceps', 'bdiv')
# assembled array -> the rules (fields of QuadratureSpec3D) it is integrated with
ARRAY_RULES_3D = {'A_diag': ('system_volume', 'system_face'), 'A_cpl': ('system_face',), 'P_diag': ('system_volume', 'system_face'),
                  'Cf': ('flux_face',), 'ebar': ('product_volume',), 'b': ('product_volume',), 'f2': ('product_volume',),
                  'ceps': ('product_volume',), 'Aaa': ('estimator_volume',), 'Aab': ('estimator_volume',),
                  'Bbb': ('estimator_volume',), 'bdiv': ('estimator_volume',)}


def _lam1_3d(x):
    return 1.0 + 0.6 * np.sin(9.0 * x[..., 0] + 4.0 * x[..., 1]) * np.cos(7.0 * x[..., 2])


def _lam2_3d(x):
    return 0.7 + 0.5 * np.cos(8.0 * x[..., 0] - 5.0 * x[..., 2] + 3.0 * x[..., 1])


def _lbar_3d(x):
    return 1.0 + 0.5 * (c3._one(x) + _lam1_3d(x) + _lam2_3d(x))


def _f_3d(x):
    """1 + sin 9z + cos 8x plus a rougher term: without it the 216-, 343- and 729-point rules of degrees 2, 3 and 4 integrate f to
    the same 4e-10, and ``bdiv`` could not tell those degrees apart."""
    return 1.0 + np.sin(9.0 * x[..., 2]) + np.cos(8.0 * x[..., 0]) + 0.5 * np.sin(12.0 * (x[..., 0] + x[..., 1]) - 3.0 * x[..., 2])


def f_second_3d(x):
    return np.sin(7.0 * x[..., 0] + 5.0 * x[..., 1]) + 0.5 * np.cos(6.0 * x[..., 2]) * x[..., 1]


_THETAS_3D = [lambda mu: 1.0, lambda mu: mu, lambda mu: mu * mu]
GRIDS_3D = {'first': ([2, 1, 2], 1), 'second': ([2, 2, 1], (2, 1, 1))}
N_3D, MU_3D = 6, 0.6


def problem_3d(grid, degree):
    """The common3d problem dict on ``GRIDS_3D[grid]`` with Q = 3 oscillating components at quadrature degree ``degree``."""
    P, kc = GRIDS_3D[grid]
    p = c3.make_problem('rules_{}_deg{}'.format(grid, degree), data_degree=degree,
                        spec=(P, kc, [c3._one, _lam1_3d, _lam2_3d], _THETAS_3D, c3.KAPPA_ANISO, N_3D, MU_3D))
    p.update(f=_f_3d, lambda_bar=_lbar_3d, lambda_hat=_lbar_3d)
    return p


@functools.lru_cache(maxsize=None)
def oracle_3d(grid, degree):
    """(problem, oracle, its assembled arrays in the product's layouts), once per session."""
    p = problem_3d(grid, degree)
    d = c3.oracle_of(p)
    return p, d, c3.oracle_assembled(p, d)


def points_of_rule_3d(field, degree):
    from pylrbms_amd.grid3d import QuadratureSpec3D, tet_rule, tri_rule
    order = getattr(QuadratureSpec3D(degree), field)
    return (tri_rule if field.endswith('_face') else tet_rule)(order)[0]


def same_points_3d(field, a, b):
    pa, pb = points_of_rule_3d(field, a), points_of_rule_3d(field, b)
    return pa.shape == pb.shape and np.array_equal(pa, pb)


def asm_reduction_lengths(degree):
    """The reduction length of every operator class of k3_asm at a degree: nB (ebar, b), nC (A_aa, A_ab, B_bb, int f), nFs (blocks
    across a face), nA + 8 nFs (diagonal blocks: volume rule + 4 faces x (inner-face table | Dirichlet table))."""
    from pylrbms_amd.grid3d import QuadratureSpec3D
    s = QuadratureSpec3D(degree)
    return {'nB': s.nB, 'nC': s.nC, 'nFs': s.nFs, 'nA+8nFs': s.nA + 8 * s.nFs}


class PaddedSpec3D:
    """The sample-record layout of ``QuadratureSpec3D(degree)`` with gaps: o_fs, o_ff, o_c and lam_stride enlarged (the volume-A
    samples stay at slot 0), hat_stride and f_stride enlarged (their segments stay at 0 and nB).  The rules are unchanged."""

    def __init__(self, degree):
        from pylrbms_amd.grid3d import QuadratureSpec3D
        s = QuadratureSpec3D(degree)
        self.__dict__.update(s.__dict__)
        self.packed = s
        self.o_fs = s.o_fs + 1
        self.o_ff = self.o_fs + 4 * s.nFs + 2
        self.o_c = self.o_ff + 4 * s.nFf + 3
        self.lam_stride = self.o_c + s.nC + 2
        self.hat_stride, self.f_stride = s.hat_stride + 3, s.f_stride + 1

    def relayout_lam(self, x):
        s = self.packed
        out = np.full(x.shape[:-1] + (self.lam_stride,), np.nan)
        out[..., :s.nA] = x[..., :s.nA]
        for a, b, k in ((s.o_fs, self.o_fs, 4 * s.nFs), (s.o_ff, self.o_ff, 4 * s.nFf), (s.o_c, self.o_c, s.nC)):
            out[..., b:b + k] = x[..., a:a + k]
        return out

    def relayout_tail(self, x, stride):
        out = np.full(x.shape[:-1] + (stride,), np.nan)
        out[..., :x.shape[-1]] = x
        return out


# ----------------------------------------------------------------------------------------------------------------- both
def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
