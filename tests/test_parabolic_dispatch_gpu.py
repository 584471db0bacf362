"""The side kernels and the single-parameter exports of the 2D parabolic path over their own dispatch, on the GPU:

  A  lrbms_mass_inverse_norm2, lrbms_div_apply (modes 0 and 1), lrbms_div_pairing as raw ``ctx`` calls: every slot-presence pattern
     (4 x 3 with interior subdomains, the strips 3 x 1 and 1 x 5), n_T = 8 | 32 | 128, 1 .. 33 columns, Q = 1 | 2 | 8
  B  ``d._time_residual_norm2`` and ``d._reconstruction_terms``: the 16-column chunk loop with full chunks and a one-column tail,
     term by term and summed
  C  lrbms_reduced_time_residual and lrbms_reduced_reconstruction_terms as raw exports at N up to 64 (both parities, the LDS opt-in
     of k_block_inverse on M_red), Q = 1 .. 8 (C = 5 Q N up to 2560), a zero-padded subdomain, their refusals; the projection of r_ud
     (lrbms_div_apply mode 1 -> lrbms_gemm_tn with Mx = N odd)
  D  lrbms_reduced_implicit_euler(_src): trajectories at N = 1 .. 64 with initial data, K = 3 sources, a zero step, a ragged
     basis; the first-step PCG iterates from a non-zero start (k_cg2_matvec<false> in its warm-start form, k_assemble_mu_mass,
     k_block_inverse on M_red + dt A)
  E  lrbms_fom_implicit_euler(_src) with initial data
  F  discretize -> ParabolicLRBMSReductor -> reduce -> rd.solve -> rd.estimate and d.estimate at N = 33 given bases, both settings
     of ``estimator.elliptic_reconstruction``, every part

against the restatements of tests/parabolic_ref.py (sparse LU / dense NumPy on oracle objects), tests/parabolic_batch_ref.py,
tests/fom_euler_batch_ref.py and oracle/parabolic.py.  Every call runs under ``poisoned`` of tests/test_work_poison_gpu.py; the
inputs a stray lane could over-read sit between NaN bands.  tests/test_parabolic_dispatch_host.py shows without a GPU that the
cells reach every branch and that a kernel with one of the faults of ``parabolic_ref.FAULTS`` could not pass them.

Tolerances (the project's): mass_inverse_norm2 1e-12 (tests/test_parabolic_gpu.py); arrays against the oracle 1e-11 of the largest
entry ("Stated parity tolerance"); estimate columns, time residual, div_pairing 1e-10
(tests/test_parabolic_estimate_batch_gpu.py); trajectories TOL_TRAJ; iterates TOL_X / TOL_RES / MUTANT_FLOOR.  The summed
reconstruction terms t1 - t2 - 2 t3 are compared relative to |t1| + |t2| + 2 |t3| of the reference."""
import ctypes

import numpy as np
import pytest

import parabolic_ref as ref
import pcg_ref
from common import expand_cols, oracle_from_problem, problem_with_q_components
from parabolic_batch_ref import column_errors, dense_euler, mass_operator
from test_parabolic_batch_gpu import T_END, TOL_TRAJ, _cut, _system
from test_pcg_iterates_gpu import (K_STEPS, KC, MUTANT_FLOOR, Q_COMPONENTS, SWEEP_GRID, _dev, _energy_bases, _model, _raw,
                                   check_iterates, check_mutant)
from test_work_poison_gpu import SENTINEL, Guard, poisoned

pytestmark = pytest.mark.gpu

TOL_MASS, TOL_ARRAY, TOL_EST = 1e-12, 1e-11, 1e-10
MISS = 1e-6                                  # a faulty reference is at least this far from the product (1e4 x TOL_EST)
BAND = 256                                   # doubles of NaN around an input
THETA = np.array([1.0, 0.37])                # the parameter of the Q = 2 cells (the one of the iterate tests)
PARTS = ('local_eta_nc', 'local_eta_r', 'local_eta_df', 'time_residual', 'time_deriv_nc')

# ------------------------------------------------------------------------------------------------------------------ cells
# A: (grid, k_c); columns per cell
A_GRIDS = (((4, 3), 2), ((3, 1), 2), ((1, 5), 2), ((2, 2), 1), ((2, 2), 4))
A_COLS = (1, 7, 16, 17, 33)
FLUX_CELL = ((4, 3), 2, 7)                   # (grid, k_c, N): lrbms_flux_reconstruct's own output as Rt
PAIRING_CELLS = ([((4, 3), 2, 1, L) for L in A_COLS] + [((4, 3), 2, 2, L) for L in A_COLS]
                 + [((4, 3), 2, 8, L) for L in (1, 7, 16, 17)]                             # C = 5 Q L up to 680
                 + [(g, kc, 2, L) for g, kc in A_GRIDS[1:] for L in (7, 17)])              # (grid, k_c, Q, L)
# B: (grid, Q); len(U) per cell
B_CELLS = (((4, 3), 2), ((3, 1), 8))
B_LENGTHS = (1, 16, 17, 33)
B_SCALE = 2e-4
# C: (N, Q, L) on the slot table of SWEEP_GRID
C_CELLS = ((1, 1, 1), (17, 8, 3), (33, 2, 5), (63, 1, 2), (64, 3, 2), (64, 8, 1))
C_INTERIOR, C_RAGGED = 5, 6                  # an interior subdomain of 4 x 3 and its right neighbour (zero-padded)
C_REFUSALS = ((65, 1, 1), (1, 1, 0), (1, 9, 1))
R_UD_CELLS = (((4, 3), 2, 5), ((4, 3), 2, 33), ((3, 1), 8, 5))                            # (grid, Q, N)
# D
D_SIZES = (1, 5, 17, 33, 40, 63, 64)
D_EXTRA = (5, 33, 64)
D_RAGGED = 12
D_ITERATES = (33, 64)
# E: (grid, k_c)
E_CELLS = (((4, 3), 2), ((4, 3), 4))
# F: (grid, Q, N)
F_CELLS = (((4, 3), 2, 33), ((3, 1), 8, 5))
F_T, F_NT = 0.05, 2

_PROBLEMS, _ORACLES, _DISC = {}, {}, {}


def problem(shape, kc=KC, Q=2):
    key = (tuple(shape), kc, Q)
    if key not in _PROBLEMS:
        from pylrbms_amd import multiscale_problem
        _PROBLEMS[key] = (multiscale_problem.init_grid_and_problem({'num_subdomains': list(shape), 'coarse_per_subdomain': kc})
                          if Q == 2 else problem_with_q_components(shape, kc, Q))
    return _PROBLEMS[key]


def oracle(shape, kc=KC, Q=2):
    key = (tuple(shape), kc, Q)
    if key not in _ORACLES:
        _ORACLES[key] = oracle_from_problem(problem(shape, kc, Q))
    return _ORACLES[key]


def slot_table(shape):
    return np.asarray(problem(shape)['grid'].neighbor_slots).reshape(-1, 5)


def theta_of(Q):
    return THETA if Q == 2 else np.linspace(0.3, 1.0, Q) * 0.87


def mu_of(Q):
    """The parameter of a discretization with Q components (theta(mu) == theta_of(Q))."""
    return float(THETA[1]) if Q == 2 else {'diffusion': theta_of(Q)}


def full_inputs(shape, kc, Q, C, seed=0):
    """Seeded random Rt [S, n_rt, C], Y = G [S, n, C'] of a cell of A (C' = C for the norm, L for the pairing)."""
    o = oracle(shape, kc, Q)
    rng = np.random.default_rng(1000 * C + 10 * kc + Q + seed)
    return rng.standard_normal((o.S, o.n_rt[0], C)), rng


def reduced_cell(N, Q, L, system=None):
    """Inputs of a cell of C on the slot table of SWEEP_GRID -> dict B [Q, S, 5, N, N], M [S, N, N], rhs [S, N], G_ud [S, N, 5 Q N],
    U [L, S, N], theta [Q], keep [S, N].  ``system`` = (B, M, rhs) of the projected Q = 2 problem (``_cut(N)``), else synthetic: B
    random, M[s] = W^T W + I.  Subdomain C_RAGGED is zero-padded by min(3, N - 1) unknowns in every operator and input."""
    nbr = slot_table(SWEEP_GRID)
    S = nbr.shape[0]
    rng = np.random.default_rng(1000 * N + 10 * Q + L)
    if system is None:
        B = rng.standard_normal((Q, S, 5, N, N))
        B[:, nbr < 0] = 0.0
        W = rng.standard_normal((S, N, N))
        M = np.einsum('ski,skj->sij', W, W) + np.eye(N)
        rhs = rng.standard_normal((S, N))
    else:
        assert Q == 2
        B, M, rhs = (np.array(x, dtype=np.float64) for x in system)
    G_ud = rng.standard_normal((S, N, 5 * Q * N))          # (random in the columns of an absent slot too: they meet ur = 0)
    U =rng.standard_normal((L, S, N)) * (1.0 if system is None else np.abs(rhs).max())
    keep = np.ones((S, N), dtype=bool)
    k = min(3, N - 1)
    if k:
        keep[C_RAGGED, N - k:] = False
    B, M, rhs, G_ud, U = pad(B, M, rhs, G_ud, U, nbr, keep)
    return dict(B=B, M=M, rhs=rhs, G_ud=G_ud, U=U, theta=theta_of(Q), keep=keep, nbr=nbr)


def pad(B, M, rhs, G_ud, U, nbr, keep):
    """Zero the rows and columns of the unknowns with keep == False: in M, in the blocks of B (rows of the subdomain's own blocks,
    columns of every block that multiplies it), in rhs, in G_ud (rows, and the columns of its slots) and in U."""
    kf = keep.astype(np.float64)
    nb = np.where(nbr >= 0, nbr, 0)
    B = B * kf[None, :, None, :, None] * kf[nb][None, :, :, None, :]
    M = M * kf[:, :, None] * kf[:, None, :]
    rhs = rhs * kf
    if G_ud is not None:
        S, N = kf.shape
        Q = G_ud.shape[2] // (5 * N)
        G_ud = (G_ud.reshape(S, N, 5, Q, N) * kf[:, :, None, None, None] * kf[nb][:, None, :, None, :]).reshape(S, N, 5 * Q * N)
    if U is not None:
        U = U * kf[None]
    return tuple(None if x is None else np.ascontiguousarray(x) for x in (B, M, rhs, G_ud, U))


def start_value(S, N, scale, seed):
    return np.random.default_rng(seed).standard_normal((S, N)) * scale


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _banded(ctx, a):
    """``a`` on the device as a contiguous view between two NaN-filled bands of BAND doubles in one allocation."""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float64)
    big = torch.full((a.size + 2 * BAND,), float('nan'), dtype=torch.float64, device=ctx.device)
    view = big[BAND:BAND + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def _engine(shape, kc=KC, Q=2):
    return _model(shape, 0, Q=Q, kc=kc)['eng']


def _disc(shape, Q):
    """The parabolic discretization of a cell of B / F (T = F_T, nt = F_NT) and its oracle."""
    key = (tuple(shape), Q)
    if key not in _DISC:
        from pylrbms_amd.discretize_parabolic_block_swipdg import discretize
        _DISC[key] = discretize(problem(shape, KC, Q), F_T, F_NT)[0]
    return _DISC[key], oracle(shape, KC, Q)


# ----------------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize('shape,kc', A_GRIDS)
def test_mass_inverse_norm2_over_grids_and_column_counts(shape, kc):
    ctx, o = _engine(shape, kc).ctx, oracle(shape, kc)
    worst = 0.0
    for L in A_COLS:
        Y = np.random.default_rng(L).standard_normal((o.S, o.n, L))
        Yt = _banded(ctx, Y)
        out = poisoned(ctx, lambda: ctx.mass_inverse_norm2(Yt)).cpu().numpy()
        assert out.shape == (o.S, L)
        want = ref.mass_inverse_norm2(o, Y)
        err = max(_rel(out[:, l], want[:, l]) for l in range(L))
        worst = max(worst, err)
        assert err < TOL_MASS, (L, err)
        assert min(_rel(out[:, l], ref.mass_inverse_norm2(o, Y, 'mass_not_inverse')[:, l]) for l in range(L)) > MISS
        if o.n > 64:
            assert min(_rel(out[:, l], ref.mass_inverse_norm2(o, Y, 'first_64')[:, l]) for l in range(L)) > MISS
    print('PARABOLIC-DISPATCH A mass_inverse_norm2 {} kc={}: worst relative deviation {:.2e}'.format(shape, kc, worst))


@pytest.mark.parametrize('mode', (0, 1))
@pytest.mark.parametrize('shape,kc', A_GRIDS)
def test_div_apply_over_grids_and_column_counts(shape, kc, mode):
    ctx, o = _engine(shape, kc).ctx, oracle(shape, kc)
    worst = 0.0
    for C in A_COLS:
        Rt, _ = full_inputs(shape, kc, 2, C)
        Rtt = _banded(ctx, Rt)
        out = poisoned(ctx, lambda: ctx.div_apply(Rtt, mode=mode)).cpu().numpy()
        want = ref.div_rows(o, Rt, mode)
        assert out.shape == want.shape == (o.S, o.n // 3 if mode == 0 else o.n, C)
        err = _rel(out, want)
        worst = max(worst, err)
        assert err < TOL_ARRAY, (C, err)
        assert _rel(out, ref.div_rows(o, Rt, mode, 'boundary_sign')) > MISS          # every subdomain of these grids has such faces
    print('PARABOLIC-DISPATCH A div_apply mode {} {} kc={}: worst relative deviation {:.2e}'.format(mode, shape, kc, worst))


def test_div_apply_on_the_flux_reconstruction_of_a_basis():
    shape, kc, N = FLUX_CELL
    eng, o = _engine(shape, kc), oracle(shape, kc)
    ctx = eng.ctx
    V = _dev(ctx, _energy_bases(eng, N, seed=3))
    Rtt = ctx.flux_reconstruct(eng.F, V)
    Rt = Rtt.cpu().numpy()
    assert Rt.shape == (o.S, o.n_rt[0], 5 * 2 * N) and np.abs(Rt).max() > 0.0
    for mode in (0, 1):
        out = poisoned(ctx, lambda: ctx.div_apply(Rtt, mode=mode)).cpu().numpy()
        err = _rel(out, ref.div_rows(o, Rt, mode))
        print('PARABOLIC-DISPATCH A div_apply mode {} on a flux image: relative deviation {:.2e}'.format(mode, err))
        assert err < TOL_ARRAY


@pytest.mark.parametrize('shape,kc,Q,L', PAIRING_CELLS)
def test_div_pairing_over_grids_components_and_column_counts(shape, kc, Q, L):
    ctx, o = _engine(shape, kc, Q).ctx, oracle(shape, kc, Q)
    th = theta_of(Q)
    Rt, rng = full_inputs(shape, kc, Q, 5 * Q * L)
    G = rng.standard_normal((o.S, o.n, L))
    Dt = ctx.div_apply(_dev(ctx, Rt), mode=0)
    D = Dt.cpu().numpy()
    assert _rel(D, ref.div_rows(o, Rt, 0)) < TOL_ARRAY
    Db, Gt = _banded(ctx, D), _banded(ctx, G)
    out = poisoned(ctx, lambda: ctx.div_pairing(th, Db, Gt)).cpu().numpy()
    want = ref.div_pairing(o, th, Rt, G)
    assert out.shape == want.shape == (o.S, L)
    err = _rel(out, want)
    print('PARABOLIC-DISPATCH A div_pairing {} kc={} Q={} L={}: relative deviation {:.2e}'.format(shape, kc, Q, L, err))
    assert err < TOL_EST
    assert _rel(out, ref.div_pairing(o, th, Rt, G, 'boundary_sign')) > MISS
    if Q > 2:
        assert _rel(out, ref.div_pairing(o, th, Rt, G, 'theta_q2')) > MISS


# ----------------------------------------------------------------------------------------------------------------------- B
_B_REF = {}


def full_vectors(shape, Q):
    """The 33 vectors of a cell of B [33, S, n]: seeded random, scaled so that r_l2(BU_R, BU_R) has the size of r_l2(F_R, F_R)
    (tests/test_parabolic_dispatch_host.py: no term is below 1e-2 of the largest)."""
    o = oracle(shape, KC, Q)
    return np.random.default_rng(7 + Q).standard_normal((max(B_LENGTHS), o.S, o.n)) * B_SCALE


def _b_reference(shape, Q):
    key = (tuple(shape), Q)
    if key not in _B_REF:
        o = oracle(shape, KC, Q)
        U = full_vectors(shape, Q)
        terms = ref.reconstruction_terms_full(o, U, mu_of(Q))
        A = o.assemble_global(mu_of(Q))
        Y = (A @ U.reshape(U.shape[0], -1).T).reshape(o.S, o.n, U.shape[0])
        _B_REF[key] = (terms, ref.mass_inverse_norm2(o, Y).sum(axis=0))
        for x in _B_REF[key]:
            x.setflags(write=False)
    return _B_REF[key]


@pytest.mark.parametrize('L', B_LENGTHS)
@pytest.mark.parametrize('shape,Q', B_CELLS)
def test_full_order_time_residual_and_reconstruction_terms(shape, Q, L):
    import torch
    from pylrbms_amd.vectorarrays import BlockVectorArray
    d, o = _disc(shape, Q)
    eng = d.engine
    c = eng.ctx
    mu = d.parse_parameter(mu_of(Q))
    assert np.allclose(d.theta(mu), theta_of(Q), rtol=0, atol=0)
    Uh = full_vectors(shape, Q)[:L]
    U = BlockVectorArray(_dev(c, Uh.transpose(1, 2, 0)), d.solution_space)
    assert len(U) == L
    terms, tr2 = _b_reference(shape, Q)
    terms = terms[:, :, :L]
    # the time residual
    got = poisoned(c, lambda: d._time_residual_norm2(U, mu))
    e_tr = _rel(got, tr2[:L])
    assert got.shape == (L,) and e_tr < TOL_EST, e_tr
    # the three terms, by the calls of the method on its own chunks
    theta = d.theta(mu)

    def three():
        t2 = c.mass_inverse_norm2(eng.b.reshape(eng.S, eng.t.n, 1).contiguous())
        t1s, t3s = [], []
        for c0 in range(0, L, 16):
            V = U.tensor[:, :, c0:c0 + 16].contiguous()
            BU = c.fom_apply(theta, eng.A_diag, eng.A_cpl, V)
            t1s.append(c.mass_inverse_norm2(BU))
            D = c.div_apply(c.flux_reconstruct(eng.F, V), mode=0)
            t3s.append(c.div_pairing(theta, D, (BU - eng.b.reshape(eng.S, eng.t.n, 1)).contiguous()))
        return torch.cat(t1s, dim=1), t2, torch.cat(t3s, dim=1)
    t1, t2, t3 = (x.cpu().numpy() for x in poisoned(c, three))
    errs = (_rel(t1, terms[0]), _rel(t2[:, 0], terms[1][:, 0]), _rel(t3, terms[2]))
    assert errs[0] < TOL_EST and errs[1] < TOL_MASS and errs[2] < TOL_EST, errs
    # the method's sum against the sum of the reference terms, relative to |t1| + |t2| + 2 |t3|
    out = poisoned(c, lambda: d._reconstruction_terms(U, mu)).cpu().numpy()
    assert out.shape == (o.S, L)
    e_sum = float((np.abs(out - ref.summed(terms)) / ref.magnitude(terms)).max())
    print('PARABOLIC-DISPATCH B {} Q={} len(U)={}: time residual {:.2e}, terms {:.2e} {:.2e} {:.2e}, sum {:.2e}'.format(
        shape, Q, L, e_tr, errs[0], errs[1], errs[2], e_sum))
    assert e_sum < TOL_EST
    assert float((np.abs(out - ref.summed(terms, 'drop_r_ud')) / ref.magnitude(terms)).max()) > MISS
    tail = slice(ref.CHUNK * ((L - 1) // ref.CHUNK), L)       # the last chunk (one column at 17 and 33): not left out
    assert float((np.abs(out[:, tail]) / ref.magnitude(terms)[:, tail]).min()) > MISS


# ----------------------------------------------------------------------------------------------------------------------- C
def _c_cell(N, Q, L):
    return reduced_cell(N, Q, L, _cut(N) if Q == 2 else None)


@pytest.mark.parametrize('N,Q,L', C_CELLS)
def test_reduced_time_residual_over_its_argument_range(N, Q, L):
    ctx = _system()['eng'].ctx
    c = _c_cell(N, Q, L)
    assert np.array_equal(c['nbr'], _system()['nbr']) and (c['nbr'][C_INTERIOR] >= 0).all() and C_RAGGED in c['nbr'][C_INTERIOR]
    Bt, Mt, Ut = _banded(ctx, c['B']), _banded(ctx, c['M']), _banded(ctx, c['U'])
    out = poisoned(ctx, lambda: ctx.reduced_time_residual(c['theta'], Bt, Mt, Ut)).cpu().numpy()
    assert out.shape == (L, ctx.S)
    want = ref.reduced_time_residual(c['B'], c['M'], c['nbr'], c['theta'], c['U'])
    err = float((np.abs(out - want) / np.abs(want)).max())
    print('PARABOLIC-DISPATCH C reduced_time_residual N={} Q={} L={}: worst relative deviation {:.2e}'.format(N, Q, L, err))
    assert err < TOL_EST
    if N > 1:
        assert _rel(out, ref.reduced_time_residual(c['B'], c['M'], c['nbr'], c['theta'], c['U'], 'mass_not_inverse')) > MISS
    if Q > 2:
        assert _rel(out, ref.reduced_time_residual(c['B'], c['M'], c['nbr'], c['theta'], c['U'], 'theta_q2')) > MISS


@pytest.mark.parametrize('N,Q,L', C_CELLS)
def test_reduced_reconstruction_terms_over_their_argument_range(N, Q, L):
    ctx = _system()['eng'].ctx
    c = _c_cell(N, Q, L)
    Bt, Mt, rt, Gt, Ut = (_banded(ctx, c[k]) for k in ('B', 'M', 'rhs', 'G_ud', 'U'))
    out = poisoned(ctx, lambda: ctx.reduced_reconstruction_terms(c['theta'], Bt, Mt, rt, Gt, Ut)).cpu().numpy()
    assert out.shape == (L, ctx.S)
    args = (c['B'], c['M'], c['rhs'], c['G_ud'], c['nbr'], c['theta'], c['U'])
    terms = ref.reduced_reconstruction_terms(*args)
    err = float((np.abs(out - ref.summed(terms)) / ref.magnitude(terms)).max())
    print('PARABOLIC-DISPATCH C reduced_reconstruction_terms N={} Q={} L={} (C = {}): worst deviation {:.2e} of |t1| + |t2| + 2 |t3|'
          .format(N, Q, L, 5 * Q * N, err))
    assert err < TOL_EST
    miss = lambda t, f=None: float((np.abs(out - ref.summed(t, f)) / ref.magnitude(terms)).max())          # noqa: E731
    assert miss(terms, 'drop_r_ud') > MISS
    if N > 1:
        assert miss(ref.reduced_reconstruction_terms(*args, fault='mass_not_inverse')) > MISS
    if 5 * Q * N > 64:
        assert miss(ref.reduced_reconstruction_terms(*args, fault='first_64')) > MISS
    if Q > 2:
        assert miss(ref.reduced_reconstruction_terms(*args, fault='theta_q2')) > MISS


@pytest.mark.parametrize('name', ('lrbms_reduced_time_residual', 'lrbms_reduced_reconstruction_terms'))
@pytest.mark.parametrize('N,Q,L', C_REFUSALS)
def test_reduced_side_exports_refuse_before_any_launch(N, Q, L, name):
    """Every buffer has the size the call names, so a kernel launched in spite of the limits would stay inside it; ``out`` and
    ``work`` keep the sentinel, bit for bit."""
    import torch
    from pylrbms_amd._native import NativeError, _dblp
    ctx = _system()['eng'].ctx
    S = ctx.S
    vp = ctypes.c_void_p
    B, M, U = ctx.zeros(Q, S, 5, N, N), ctx.zeros(S, N, N), ctx.zeros(max(L, 1), S, N)
    rhs, G_ud = ctx.zeros(S, N), ctx.zeros(S, N, 5 * Q * N)
    M += torch.eye(N, dtype=torch.float64, device=ctx.device)
    g = Guard(ctx, 0.0)
    work = g.alloc((int(ctx.lib.lrbms_reduced_time_residual_work_size(ctx.handle, N)),), 0.0)
    out = g.alloc((max(L, 1), S), 0.0)
    for t in (work, out):
        t.view(torch.int64).fill_(SENTINEL)
    th = np.ones(Q)
    if name == 'lrbms_reduced_time_residual':
        rc = _raw(ctx, name, Q, N, L, _dblp(th), vp(B.data_ptr()), vp(M.data_ptr()), vp(U.data_ptr()), vp(work.data_ptr()),
                  vp(out.data_ptr()), ctx._stream())
    else:
        rc = _raw(ctx, name, Q, N, L, _dblp(th), vp(B.data_ptr()), vp(M.data_ptr()), vp(rhs.data_ptr()), vp(G_ud.data_ptr()),
                  vp(U.data_ptr()), vp(work.data_ptr()), vp(out.data_ptr()), ctx._stream())
    assert rc != 0
    with pytest.raises(NativeError):
        ctx._check(rc, name)
    g.check()
    assert bool((out.view(torch.int64) == SENTINEL).all()) and bool((work.view(torch.int64) == SENTINEL).all())


_REDUCED = {}


def given_bases(shape, Q, N):
    """[S, n, N]: a constant and N - 1 seeded columns per subdomain, orthonormal in the product's local energy product."""
    d, o = _disc(shape, Q)
    return _energy_bases(d.engine, N, seed=N)


def _reduced(shape, Q, N):
    """(d, o, reductor, rd, V, oracle reductor, oracle reduced model) of given bases of N columns."""
    key = (tuple(shape), Q, N)
    if key not in _REDUCED:
        from oracle.lrbms import OracleReductor
        from pylrbms_amd.reductor import ParabolicLRBMSReductor
        d, o = _disc(shape, Q)
        V = given_bases(shape, Q, N)
        reductor = ParabolicLRBMSReductor(d, bases={'domain_{}'.format(ii): V[ii].T for ii in range(o.S)})
        assert reductor.basis_size() == N
        rd = reductor.reduce()
        assert rd.N == N
        ored = OracleReductor(o, [V[ii] for ii in range(o.S)])
        _REDUCED[key] = (d, o, reductor, rd, V, ored, ored.reduce())
    return _REDUCED[key]


@pytest.mark.parametrize('shape,Q,N', R_UD_CELLS)
def test_projected_r_ud(shape, Q, N):
    from oracle.parabolic import OracleParabolicReduced
    d, o, reductor, rd, V, ored, ord_ = _reduced(shape, Q, N)
    rd._G_ud = None
    G = poisoned(d.engine.ctx, lambda: setattr(rd, '_G_ud', None) or rd._projected_r_ud()).cpu().numpy()
    assert G.shape == (o.S, N, 5 * Q * N)
    compact = OracleParabolicReduced(ored, ord_, F_T, F_NT)._projected_r_ud()
    want = np.stack([expand_cols(compact[ii], problem(shape, KC, Q)['grid'], ii, Q * N) for ii in range(o.S)])
    err = _rel(G, want)
    print('PARABOLIC-DISPATCH C projected r_ud {} Q={} N={} (My = {}): relative deviation {:.2e}'.format(shape, Q, N, 5 * Q * N, err))
    assert err < TOL_ARRAY


# ----------------------------------------------------------------------------------------------------------------------- D
NT = 2


def _euler(ctx, N, B, M, rhs, U0=None, phi=None):
    """The single export on host arrays under ``poisoned`` -> (U [NT + 1, S, N] host, info); rhs [S, N], or [K, S, N] with phi."""
    Bd, Md, rd = _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs)
    U0d = None if U0 is None else _dev(ctx, U0)
    if phi is None:
        U, info = poisoned(ctx, lambda: ctx.reduced_implicit_euler(THETA, T_END / NT, NT, Bd, Md, rd, U0=U0d))
    else:
        phid = _dev(ctx, phi)
        U, info = poisoned(ctx, lambda: ctx.reduced_implicit_euler_src(THETA, T_END / NT, NT, Bd, Md, rd, phid, U0=U0d))
    assert info['relative_residual'] <= 1e-13
    return U.cpu().numpy(), info


def _traj_error(U, want):
    return float(column_errors(U[..., None], want[..., None]).max())


@pytest.mark.parametrize('N', D_SIZES)
def test_single_reduced_trajectory_over_basis_sizes(N):
    s = _system()
    B, M, rhs = _cut(N)
    U, info = _euler(s['eng'].ctx, N, B, M, rhs)
    assert np.all(U[0] == 0.0) and info['iterations'] >= NT
    err = _traj_error(U, dense_euler(B, M, s['nbr'], THETA, T_END / NT, NT, rhs=rhs))
    print('PARABOLIC-DISPATCH D single trajectory N={}: {} iterations, error {:.2e} (tolerance {:.0e})'.format(
        N, info['iterations'], err, TOL_TRAJ))
    assert err < TOL_TRAJ


def source_of(S, N, rhs, zero_first=False):
    """rhs_K [3, S, N] and phi [NT + 1, 3] of the _src cells; ``zero_first``: the row of the first step is zero."""
    rng = np.random.default_rng(N)
    rhs_K = np.ascontiguousarray(np.concatenate([rhs[None], rng.standard_normal((2, S, N)) * np.abs(rhs).max()]))
    phi = rng.uniform(0.2, 1.0, (NT + 1, 3))
    if zero_first:
        phi[1] = 0.0
    return rhs_K, phi


@pytest.mark.parametrize('N', D_EXTRA)
def test_single_reduced_trajectory_with_initial_data_and_sources(N):
    s = _system()
    ctx, S, nbr, dt = s['eng'].ctx, s['eng'].S, s['nbr'], T_END / NT
    B, M, rhs = _cut(N)
    plain = dense_euler(B, M, nbr, THETA, dt, NT, rhs=rhs)
    U0 = start_value(S, N, np.abs(plain).max(), seed=N)
    U, _ = _euler(ctx, N, B, M, rhs, U0=U0)
    assert np.array_equal(U[0], U0)
    e_u0 = _traj_error(U, dense_euler(B, M, nbr, THETA, dt, NT, rhs=rhs, U0=U0))
    assert _traj_error(U, plain) > 1e-2                          # the start value is not lost on the way
    rhs_K, phi = source_of(S, N, rhs)
    U, _ = _euler(ctx, N, B, M, rhs_K, U0=U0, phi=phi)
    e_src = _traj_error(U, dense_euler(B, M, nbr, THETA, dt, NT, rhs_K=rhs_K, phi=phi, U0=U0))
    rhs_K, phi = source_of(S, N, rhs, zero_first=True)
    U, info = _euler(ctx, N, B, M, rhs_K, phi=phi)
    assert np.all(U[1] == 0.0) and np.abs(U[2]).max() > 0.0     # the zero step is skipped, the next one is not
    e_zero = _traj_error(U, dense_euler(B, M, nbr, THETA, dt, NT, rhs_K=rhs_K, phi=phi))
    print('PARABOLIC-DISPATCH D N={}: error with U0 {:.2e}, _src K=3 with U0 {:.2e}, _src after a zero step {:.2e}'.format(
        N, e_u0, e_src, e_zero))
    assert e_u0 < TOL_TRAJ and e_src < TOL_TRAJ and e_zero < TOL_TRAJ


def ragged_keep(S, N):
    """[S, N] bool: subdomain s keeps N - (s % 4) unknowns (the first all of them)."""
    return np.arange(N)[None, :] < (N - np.arange(S) % 4)[:, None]


def test_single_reduced_trajectory_with_a_ragged_basis():
    s = _system()
    ctx, S, nbr, N = s['eng'].ctx, s['eng'].S, s['nbr'], D_RAGGED
    keep = ragged_keep(S, N)
    B, M, rhs = _cut(N)
    B, M, rhs, _, _ = pad(B, M, rhs, None, None, nbr, keep)
    U0 = start_value(S, N, 1e-3, seed=1) * keep
    U, _ = _euler(ctx, N, B, M, rhs, U0=U0)
    assert np.all(U[:, ~keep] == 0.0)
    err = _traj_error(U, dense_euler(B, M, nbr, THETA, T_END / NT, NT, rhs=rhs, U0=U0, keep=keep))
    print('PARABOLIC-DISPATCH D ragged N={}: error {:.2e}'.format(N, err))
    assert err < TOL_TRAJ


def iterate_system(B, M, rhs, nbr, U0, dt):
    """-> (A sparse, r0 = M u0 + dt b - (M + dt A) u0, |r0| / |M u0 + dt b|): the first step from the start value U0."""
    S, N = rhs.shape
    A = pcg_ref.reduced_operator(ref.step_blocks(B, M, THETA, dt), nbr)
    u0 = U0.reshape(S * N)
    full = mass_operator(M) @ u0 + dt * rhs.reshape(S * N)
    r0 = full - A @ u0
    return A, r0, float(np.linalg.norm(r0) / np.linalg.norm(full))


def iterate_reference(A, r0, scale, P):
    def reference(k):
        x, r = pcg_ref.pcg_iterate(lambda p: A @ p, P.apply, r0[:, None], k)
        return x, r * scale
    return reference


def iterate_start(B, M, rhs, nbr, N, dt):
    S = rhs.shape[0]
    return start_value(S, N, np.abs(dense_euler(B, M, nbr, THETA, dt, 1, rhs=rhs)).max(), seed=100 + N)


@pytest.mark.parametrize('N', D_ITERATES)
def test_single_export_first_step_iterates_from_a_start_value(N):
    from pylrbms_amd._native import _dblp, c_vp
    s = _system()
    ctx, S, nbr, dt = s['eng'].ctx, s['eng'].S, s['nbr'], T_END
    B, M, rhs = _cut(N)
    U0 = iterate_start(B, M, rhs, nbr, N, dt)
    A, r0, scale = iterate_system(B, M, rhs, nbr, U0, dt)
    Bd, Md, rd, U0d = _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs), _dev(ctx, U0)
    size = int(ctx.lib.lrbms_reduced_solve_work_size(ctx.handle, N))

    def raw(k):
        work = ctx.empty(size)
        U = ctx.zeros(2, S, N)
        U[0] = U0d
        info = np.zeros(2)
        rc = _raw(ctx, 'lrbms_reduced_implicit_euler', 2, N, _dblp(THETA), dt, 1, c_vp(Bd.data_ptr()), c_vp(Md.data_ptr()),
                  c_vp(rd.data_ptr()), c_vp(work.data_ptr()), c_vp(U.data_ptr()), 1e-14, int(k), _dblp(info), ctx._stream())
        return rc, U, info

    def run(k):
        rc, U, info = poisoned(ctx, lambda: raw(k))
        Uh = U.cpu().numpy().reshape(2, S * N)
        return rc, (Uh[1] - Uh[0])[:, None], info

    P = ref.mass_preconditioner(B, M, nbr, THETA, dt)
    assert P.has_coarse
    reference = iterate_reference(A, r0, scale, P)
    tag = 'single euler U0 N={}'.format(N)
    check_iterates(run, reference, tag)
    # a reference whose inverse blocks lack the mass, and the mass on every slot: the product is far from both
    for fault in ('no_mass', 'mass_every_slot'):
        check_mutant(run, iterate_reference(A, r0, scale, ref.mass_preconditioner(B, M, nbr, THETA, dt, fault)), tag + ' ' + fault)
    ctx.set_option('coarse', 0)
    try:
        check_mutant(run, reference, tag)
    finally:
        ctx.set_option('coarse', 1)


# ----------------------------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize('shape,kc', E_CELLS)
def test_single_full_order_trajectory_with_initial_data(shape, kc):
    import fom_euler_batch_ref
    m = _model(shape, 0, kc=kc)
    eng = m['eng']
    ctx, S, t, dt = eng.ctx, eng.S, eng.ctx.t, T_END / NT
    A_diag, A_cpl, b = eng.A_diag.cpu().numpy(), eng.A_cpl.cpu().numpy(), eng.b.cpu().numpy()
    rng = np.random.default_rng(kc)
    b_K = np.ascontiguousarray(np.concatenate([b[None], rng.standard_normal((2, S, t.n)) * np.abs(b).max()]))
    phi = rng.uniform(0.2, 1.0, (NT + 1, 3))
    parts = (fom_euler_batch_ref.component_operators(A_diag, A_cpl, t, m['nbr']), fom_euler_batch_ref.p1_mass(t.area, S))

    def want(U0, b_K, phi):
        r = fom_euler_batch_ref.BatchFomEulerRef(parts[0], parts[1], S, t.n, THETA[None], dt, NT, phi[None], b_K, U0=U0)
        return r.trajectories()[:, :, 0].reshape(NT + 1, S, t.n)
    plain = want(None, b[None], np.ones((NT + 1, 1)))
    U0 = start_value(S, t.n, np.abs(plain).max(), seed=kc)
    U0d, b_Kd, phid = _dev(ctx, U0), _dev(ctx, b_K), _dev(ctx, phi)
    U, info = poisoned(ctx, lambda: ctx.fom_implicit_euler(THETA, dt, NT, eng.A_diag, eng.A_cpl, eng.b, U0=U0d, rtol=1e-13))
    U = U.cpu().numpy()
    assert np.array_equal(U[0], U0) and info['relative_residual'] <= 1e-13
    e_u0 = _traj_error(U, want(U0.reshape(-1, 1), b[None], np.ones((NT + 1, 1))))
    assert _traj_error(U, plain) > 1e-2
    U, info = poisoned(ctx, lambda: ctx.fom_implicit_euler_src(THETA, dt, NT, eng.A_diag, eng.A_cpl, b_Kd, phid, U0=U0d, rtol=1e-13))
    e_src = _traj_error(U.cpu().numpy(), want(U0.reshape(-1, 1), b_K, phi))
    print('PARABOLIC-DISPATCH E {} kc={}: error with U0 {:.2e}, _src K=3 with U0 {:.2e} (tolerance {:.0e})'.format(
        shape, kc, e_u0, e_src, TOL_TRAJ))
    assert e_u0 < TOL_TRAJ and e_src < TOL_TRAJ


# ----------------------------------------------------------------------------------------------------------------------- F
@pytest.mark.parametrize('shape,Q,N', F_CELLS)
def test_estimator_surface_from_given_bases(shape, Q, N):
    from oracle.parabolic import OracleParabolic, OracleParabolicReduced
    from pylrbms_amd.reductor import ReducedVectorArray
    d, o, reductor, rd, V, ored, ord_ = _reduced(shape, Q, N)
    ctx = d.engine.ctx
    mu_o = mu_of(Q)
    mu = d.parse_parameter(mu_o)
    op, opr = OracleParabolic(o, F_T, F_NT), OracleParabolicReduced(ored, ord_, F_T, F_NT)
    # the reduced trajectory
    u = poisoned(ctx, lambda: rd.solve(mu).tensor)
    uh = u.cpu().numpy().transpose(2, 0, 1).reshape(F_NT + 1, o.S * N)
    e_u = _traj_error(uh.reshape(F_NT + 1, o.S, N), opr.solve(mu_o).reshape(F_NT + 1, o.S, N))
    assert e_u < TOL_TRAJ, e_u
    u = ReducedVectorArray(u)
    UU = reductor.reconstruct(u)
    UUh = UU.tensor.cpu().numpy().transpose(2, 0, 1)
    assert _rel(UUh, np.einsum('sni,ksi->ksn', V, uh.reshape(F_NT + 1, o.S, N))) < 1e-12
    # every part, reduced and full order, on the product's own coefficients, for both settings of the flag
    got, want = {}, {}
    try:
        for flag in (False, True):
            d.estimator.elliptic_reconstruction = flag
            assert rd.estimator is d.estimator
            got['rd', flag] = poisoned(ctx, lambda: rd.estimate(u, mu))
            got['d', flag] = poisoned(ctx, lambda: d.estimate(UU, mu))
            want['rd', flag] = opr.estimate(uh, mu_o, elliptic_reconstruction=flag)
            want['d', flag] = op.estimate(UUh, mu_o, elliptic_reconstruction=flag)
    finally:
        d.estimator.elliptic_reconstruction = False
    worst = {}
    for key in got:
        (est, parts), (est_o, parts_o) = got[key], want[key]
        for nm, a, b in zip(PARTS, parts, parts_o):
            worst[key + (nm,)] = _rel(a, b)
        worst[key + ('est',)] = abs(est - est_o) / est_o
    # the True-minus-False difference of local_eta_r: the reconstruction terms alone, relative to local_eta_r itself
    for who in ('rd', 'd'):
        a = got[who, True][1][1] - got[who, False][1][1]
        b = want[who, True][1][1] - want[who, False][1][1]
        assert np.abs(b).max() > 1e-3 * np.abs(want[who, True][1][1]).max()                     # they are a visible part of it
        worst[who, 'terms'] = float(np.abs(a - b).max() / np.abs(want[who, True][1][1]).max())
    for key in sorted(worst, key=str):
        print('PARABOLIC-DISPATCH F {} Q={} N={} {}: relative deviation {:.2e}'.format(shape, Q, N, key, worst[key]))
    bad = {k: v for k, v in worst.items() if not v < TOL_EST}
    assert not bad, bad


assert set(Q_COMPONENTS) >= {Q for _, _, Q, _ in PAIRING_CELLS}
