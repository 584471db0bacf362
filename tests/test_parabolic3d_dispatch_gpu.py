"""The side kernels of the parabolic 3D / P2 path over their own dispatch, on the GPU:

  A  lrbms3_project_mass            k3p_project_mass<T>, T = ceil(N / 16) = 1..4: cross tiles, masked tile edges (N = 16 k, 16 k +- 1),
                                    n_T % 8 != 0, fewer elements than waves
  B  lrbms3_mass_inverse_norm2      k3p_mass_inv_norm2: G = 1, G > 1 dividing n_T or not, idle tail threads, L > 256 (the l0 loop's
                                    second and third trip)
  C  lrbms3_reduced_time_residual   the raw export on synthetic operators at N up to 64, Q = 1 and 8, a subdomain with all seven
                                    slots, and its refusals
  D  lrbms3_reduced_implicit_euler  and the Python surface (rd.solve, rd.solve_batch's loop, rd.estimate) at N > 32

against the restatements of tests/parabolic3d_ref.py (np.longdouble / sparse LU / dense NumPy).  Every call runs under
``poisoned`` of tests/test_work_poison_gpu.py: zero- and NaN-filled outputs and work between sentinel bands.
tests/test_parabolic3d_dispatch_host.py shows without a GPU that these cells reach every branch and that a kernel with one of the
faults the reference can be switched to could not pass them."""
import ctypes

import numpy as np
import pytest

import common3d as c3
import parabolic3d_ref as ref
from test_work_poison_gpu import SENTINEL, Guard, poisoned

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------------------ cells
A_CELLS = ([('kc_3x1x2', N) for N in (15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)] + [('aniso_2x2x1', N) for N in (33, 64)]
           + [('interior_3x3x3', N) for N in (17, 33, 49)])
ZERO_TILE_CELL = ('kc_3x1x2', 48)          # columns 32..47 of subdomain 1 zero: a whole tile of zero-padded columns
B_CELLS = ([('kc_3x1x2', L) for L in (2, 3, 100, 128, 129, 255, 256, 257, 300, 513)] + [('interior_3x3x3', L) for L in (129, 257)])
C_PROBLEM = 'interior_3x3x3'
C_CELLS = [(1, 1, 1), (17, 8, 3), (33, 2, 5), (63, 1, 2), (64, 3, 2), (64, 8, 1)]          # (N, Q, L)
C_RAGGED = 14                              # a face neighbour of the centre subdomain 13: zero-padded by min(3, N - 1) unknowns
D_PROBLEM = 'q1_strip'
D_CELLS = [33, 64]
BAND = 256                                 # doubles of NaN around an input: more than the two rows (2 N) a lane with r >= 10 would reach

_ORACLES, _DISC = {}, {}


def oracle(name):
    if name not in _ORACLES:
        p = c3.make_problem(name)
        _ORACLES[name] = (p, c3.oracle_of(p))
    return _ORACLES[name]


def bases_of(name, N):
    """The basis of a cell of A: ``make_bases3d(seed=N)``, the last column of subdomain 0 zeroed (a ragged basis); in
    ZERO_TILE_CELL also the whole last tile of subdomain 1."""
    p, o = oracle(name)
    V = c3.make_bases3d(o.S, o.n, N, seed=N)
    if N > 1:
        V[0, :, N - 1] = 0.0
    if (name, N) == ZERO_TILE_CELL:
        V[1, :, 32:48] = 0.0
    return V


def vectors_of(name, L):
    p, o = oracle(name)
    return np.random.default_rng(L).standard_normal((o.S, o.n, L))


def synthetic_operators(nbr, N, Q, L, seed=0):
    """Inputs of a cell of C on the slot table ``nbr`` [S, 7]: random B_sys [Q, S, 7, N, N], SPD M_red[s] = W^T W + I, random
    dU [L, S, N], theta [Q]; subdomain C_RAGGED zero-padded by k = min(3, N - 1) unknowns (rows and columns of M_red and of its
    B_sys blocks zero, the columns of the blocks that multiply it too, its dU entries zero).  -> B, M_red, dU, theta, keep [S, N]."""
    nbr = np.asarray(nbr).reshape(-1, 7)
    S = nbr.shape[0]
    rng = np.random.default_rng(1000 * N + 10 * Q + L + seed)
    B = rng.standard_normal((Q, S, 7, N, N))
    W = rng.standard_normal((S, N, N))
    M_red = np.einsum('ski,skj->sij', W, W) + np.eye(N)
    dU = rng.standard_normal((L, S, N))
    theta = rng.uniform(0.5, 1.5, size=Q)
    keep = np.ones((S, N), dtype=bool)
    k = min(3, N - 1)
    if k:
        r = C_RAGGED
        keep[r, N - k:] = False
        M_red[r, N - k:, :] = 0.0
        M_red[r, :, N - k:] = 0.0
        dU[:, r, N - k:] = 0.0
        B[:, r, :, N - k:, :] = 0.0
        for s in range(S):
            for slot in range(7):
                if nbr[s, slot] == r:
                    B[:, s, slot, :, N - k:] = 0.0
    return B, M_red, dU, theta, keep


def _pd(p):
    return {'grid': p['grid'], 'lambda': {'functions': p['lambdas'], 'coefficients': p['thetas']}, 'lambda_bar': p['lambda_bar'],
            'lambda_hat': p['lambda_hat'], 'f': p['f'], 'mu_bar': p['mu_bar'], 'mu_hat': p['mu_hat']}


def _disc(name, T=0.15, nt=3):
    if name not in _DISC:
        from pylrbms_amd.discretize_parabolic_block_swipdg_3d import discretize
        p, o = oracle(name)
        _DISC[name] = discretize(_pd(p), T, nt)[0]
    p, o = oracle(name)
    return p, o, _DISC[name]


def _banded(ctx, a):
    """``a`` on the device as a contiguous view between two NaN-filled bands of BAND doubles in one allocation: a read past
    either end of the input poisons whatever it feeds."""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float64)
    big = torch.full((a.size + 2 * BAND,), float('nan'), dtype=torch.float64, device=ctx.device)
    view = big[BAND:BAND + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


# ----------------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize('name,N', A_CELLS)
def test_project_mass_over_the_tile_dispatch(name, N):
    p, o, d = _disc(name)
    ctx = d.engine.ctx
    V = bases_of(name, N)
    Vt = _banded(ctx, V)
    M_red = poisoned(ctx, lambda: ctx.project_mass(Vt)).cpu().numpy()
    assert M_red.shape == (o.S, N, N)
    want = ref.project_mass(o, V).astype(np.float64)
    worst = max(c3.rel(M_red[s], want[s]) for s in range(o.S))
    print('project_mass {} N = {}: worst relative deviation {:.3e}'.format(name, N, worst))
    assert worst < 1e-12
    for s in range(o.S):
        assert c3.rel(M_red[s], M_red[s].T) < 1e-13
    assert np.all(M_red[0, N - 1, :] == 0.0) and np.all(M_red[0, :, N - 1] == 0.0)
    if (name, N) == ZERO_TILE_CELL:
        assert np.all(M_red[1, 32:48, :] == 0.0) and np.all(M_red[1, :, 32:48] == 0.0)
    # the reference's switches: the result is far from every wrong variant that exists at this cell
    nT = p['grid'].template.n_T
    # (the six element types share one mass block, tests/test_parabolic3d_dispatch_host.py: no variant with the types swapped)
    if nT % ref.WAVES:
        wrong = ref.project_mass(o, V, drop_tail=True).astype(np.float64)
        assert min(c3.rel(M_red[s], wrong[s]) for s in range(o.S)) > 1e-6
    if N > 16:                             # subdomain 0 apart: its zeroed last column is the whole second tile at N = 17
        wrong = ref.project_mass(o, V, drop_cross=True).astype(np.float64)
        assert min(c3.rel(M_red[s], wrong[s]) for s in range(1, o.S)) > 1e-6


# ----------------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize('name,L', B_CELLS)
def test_mass_inverse_norm2_over_the_chunk_classes(name, L):
    p, o, d = _disc(name)
    ctx = d.engine.ctx
    Y = vectors_of(name, L)
    Yt = _banded(ctx, Y)
    out = poisoned(ctx, lambda: ctx.mass_inverse_norm2(Yt)).cpu().numpy()
    assert out.shape == (o.S, L)
    want = ref.mass_inverse_norm2(o, Y)
    worst = max(c3.rel(out[:, l], want[:, l]) for l in range(L))
    print('mass_inverse_norm2 {} L = {}: worst relative deviation {:.3e}'.format(name, L, worst))
    assert worst < 1e-12
    nT = p['grid'].template.n_T
    if L > ref.CHUNK:
        wrong = ref.mass_inverse_norm2(o, Y, first_trip_only=True)
        assert min(c3.rel(out[:, l], wrong[:, l]) for l in range(ref.CHUNK, L)) > 1e-6
    hit = [l for l in range(L) if ref.chunk_of(L, l)[1] > 1 and nT % ref.chunk_of(L, l)[1]]       # G does not divide n_T
    if hit:
        wrong = ref.mass_inverse_norm2(o, Y, drop_group_tail=True)
        assert min(c3.rel(out[:, l], wrong[:, l]) for l in hit) > 1e-6


# ----------------------------------------------------------------------------------------------------------------------- C
def _raw_time_residual(ctx, Q, N, L, theta, B, M_red, dU, work, out):
    """The export itself, without the wrapper's shape checks -> its return code."""
    from pylrbms_amd._native3d import _P_DBL
    th = np.ascontiguousarray(theta, dtype=np.float64)
    vp = ctypes.c_void_p
    return ctx.lib.lrbms3_reduced_time_residual(ctx.handle, Q, N, L, th.ctypes.data_as(_P_DBL), vp(B.data_ptr()), vp(M_red.data_ptr()),
                                                vp(dU.data_ptr()), vp(work.data_ptr()), vp(out.data_ptr()), ctx._stream())


@pytest.mark.parametrize('N,Q,L', C_CELLS)
def test_reduced_time_residual_at_its_argument_limits(N, Q, L):
    p, o, d = _disc(C_PROBLEM)
    ctx = d.engine.ctx
    nbr = np.asarray(p['grid'].neighbor_slots).reshape(o.S, 7)
    assert (nbr[13] >= 0).all() and C_RAGGED in nbr[13]
    B, M_red, dU, theta, keep = synthetic_operators(nbr, N, Q, L)
    Bt, Mt, dUt = _banded(ctx, B), _banded(ctx, M_red), _banded(ctx, dU)
    out = poisoned(ctx, lambda: ctx.reduced_time_residual(Q, theta, Bt, Mt, dUt)).cpu().numpy()      # work and out: the wrapper's
    assert out.shape == (L, o.S)
    want = ref.reduced_time_residual(B, M_red, nbr, theta, dU, keep)
    err = np.abs(out - want) / np.abs(out)
    print('reduced_time_residual N = {} Q = {} L = {}: worst relative deviation {:.3e}'.format(N, Q, L, err.max()))
    assert np.all(np.abs(out - want) < 1e-10 * np.abs(out))
    if N > 1:                              # (N = 1: the inverse of a 1 x 1 block is the inverse of its diagonal)
        wrong = ref.reduced_time_residual(B, M_red, nbr, theta, dU, keep, diagonal_inverse=True)
        assert np.abs(out - wrong).max() > 1e-6 * np.abs(out).max()
    for slot in range(7):                  # the centre subdomain has all seven
        wrong = ref.reduced_time_residual(B, M_red, nbr, theta, dU, keep, drop_slot=slot)
        assert np.abs(out[:, 13] - wrong[:, 13]).max() > 1e-6 * np.abs(out[:, 13]).max(), slot


@pytest.mark.parametrize('N,Q,L', [(65, 1, 1), (1, 9, 1), (1, 1, 0), (1, 1, 65536)])
def test_reduced_time_residual_refuses_before_any_launch(N, Q, L):
    """Every buffer has the size the call names, so a kernel launched in spite of the limits would stay inside it; ``out`` and
    ``work`` keep the sentinel, bit for bit."""
    import torch
    from pylrbms_amd._native import NativeError
    p, o, d = _disc(C_PROBLEM)
    ctx, S = d.engine.ctx, o.S
    B, M_red, dU = ctx.zeros(Q, S, 7, N, N), ctx.zeros(S, N, N), ctx.zeros(max(L, 1), S, N)
    M_red += torch.eye(N, dtype=torch.float64, device=ctx.device)
    g = Guard(ctx, 0.0)
    work = g.alloc((S * 8 * N * N,), 0.0)
    out = g.alloc((max(L, 1), S), 0.0)
    for t in (work, out):
        t.view(torch.int64).fill_(SENTINEL)
    rc = _raw_time_residual(ctx, Q, N, L, np.ones(Q), B, M_red, dU, work, out)
    assert rc != 0
    with pytest.raises(NativeError):
        ctx._check(rc, 'lrbms3_reduced_time_residual')
    g.check()
    assert bool((out.view(torch.int64) == SENTINEL).all()) and bool((work.view(torch.int64) == SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------------------- D
_D = {}


def _projected(N):
    """q1_strip at basis size N (subdomain 1 zero-padded by two vectors): the pass's outputs and the projected mass."""
    if N not in _D:
        p, o, d = _disc(D_PROBLEM)
        eng = d.engine
        V = c3.make_bases3d(o.S, o.n, N, seed=N)
        V[1, :, N - 2:] = 0.0
        Vt = eng.ctx.from_numpy(V)
        _D[N] = (eng.project_and_estimate(Vt), eng.ctx.project_mass(Vt))
    return _D[N]


@pytest.mark.parametrize('N', D_CELLS)
def test_reduced_implicit_euler_beyond_the_batched_width(N):
    from test_parabolic3d_gpu import _dense_reduced
    p, o, d = _disc(D_PROBLEM)
    eng, mu = d.engine, p['mu']
    assert d.Q == 1 and N > 32
    out, M_red = _projected(N)
    th, dt, nt = d.theta(mu), 0.05, 3
    u, (it, res) = poisoned(eng.ctx, lambda: eng.ctx.reduced_implicit_euler(d.Q, th, dt, nt, out['B_sys'], M_red, out['rhs_red']))
    assert res <= 1e-12 and it > 0
    u = u.cpu().numpy()
    nbr = np.asarray(p['grid'].neighbor_slots).reshape(o.S, 7)
    B, Mr, rhs = out['B_sys'].cpu().numpy(), M_red.cpu().numpy(), out['rhs_red'].cpu().numpy()
    keep = np.ones((o.S, N), dtype=bool)
    keep[1, N - 2:] = False
    assert np.all(u[:, 1, N - 2:] == 0.0)                                # padded unknowns stay exactly 0
    A = _dense_reduced(o.S, N, nbr, B, th)
    want = ref.reduced_stepping(A, Mr, rhs, dt, nt, keep)
    worst = c3.rel(u.reshape(nt + 1, -1), want)
    print('reduced_implicit_euler N = {}: relative deviation {:.3e} after {} iterations'.format(N, worst, it))
    assert worst < 1e-9
    assert c3.rel(u.reshape(nt + 1, -1), ref.reduced_stepping(A, Mr, rhs, dt, nt, keep, mass_in_rhs=False)) > 1e-6


def test_reductor_surface_beyond_the_batched_width():
    """rd.solve, the loop rd.solve_batch falls back to at N > 32 and rd.estimate, from a ready-made basis of 33 vectors."""
    import torch
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D
    from test_parabolic3d_gpu import PARTS
    N = 33
    p, o, d = _disc(D_PROBLEM)
    T, nt = d.T, d.time_stepper.nt
    V = c3.make_bases3d(o.S, o.n, N, seed=N)
    reductor = ParabolicLRBMSReductor3D(d, bases=d.engine.ctx.from_numpy(V))
    assert reductor.basis_size() == N
    rd = reductor.reduce()
    assert rd.N == N
    mus = [p['mu'], 0.4]
    Ub = rd.solve_batch(mus)
    assert tuple(Ub.shape) == (2, nt + 1, o.S, N)
    for m, mu in enumerate(mus):
        assert torch.equal(Ub[m], rd.solve(mu))                         # the N > 32 fallback: bit for bit
    red = ref.ParabolicReduced3D(o, [V[ii] for ii in range(o.S)], T, nt)
    mu = mus[0]
    u_o = red.solve(mu)
    assert c3.rel(Ub[0].cpu().numpy().reshape(nt + 1, -1), u_o) < 1e-8
    est, parts = rd.estimate(Ub[0], mu)
    est_o, parts_o = red.estimate(u_o, mu)
    for nm, a, b in zip(PARTS, parts, parts_o):
        print('estimate N = 33, {}: relative deviation {:.3e}'.format(nm, c3.rel(a, b)))
        assert c3.rel(a, b) < 1e-6, nm
    assert abs(est - est_o) < 1e-6 * est_o
