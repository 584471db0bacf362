"""NumPy restatement of lrbms3_reduced_parabolic_estimate_batch: the five outputs of the export from DENSE reduced
operators in the neighbourhood formulation -- the layout of ``common3d.oracle_dense_blocks`` (from the CPU oracle) and of
``pylrbms_amd.engine3d.expand_factored`` (from the factored arrays of a pass), columns slot-major, then q, then basis index.
Test infrastructure only.

    model = dict(nbr [S, 7], B_sys [Q, S, 7, N, N], M_red [S, N, N], G_nc [S, 7N, 7N], G_bb / G_rdd [S, 7QN, 7QN], r_fd [S, 7QN],
                 G_ab [Q, S, N, 7QN], G_aa [Q, Q, S, N, N], f2 [S], ceps [S], hdiam)
    source = dict(F2 [S, K, K], r_fd_K [K, S, 7QN])            # with it the model's f2 / r_fd are not read

Every switch of ``estimate_outputs`` throws one fault into the restatement ("mutant"); tests/test_parabolic_estimate_batch3d_host.py
shows each of them to be more than 1e-6 away from the right one on the inputs of the GPU cells, so an export with that fault could
not pass there."""
import numpy as np

SELF = 3
DT = 0.05
# (problem of common3d.PROBLEMS, N, nmu, nt) of the export-level GPU tests: nmu in {1, 15, 16, 17, 33, 64} (one column, a partial
# pass, a full one, a second pass of one column, three passes, four full ones), nt in {1, 3}, N odd and even on one and two row
# tiles of the panel matvec; a subdomain with all seven slots (interior_3x3x3), an anisotropic kappa, Q = 1 and Q = 3, padded side
# rows (kc_3x1x2) and the template of config 5 (dynamic LDS above 64 KB)
CELLS = (('interior_3x3x3', 5, 17, 3), ('interior_3x3x3', 15, 1, 1), ('interior_3x3x3', 16, 15, 3), ('interior_3x3x3', 17, 33, 1),
         ('interior_3x3x3', 32, 64, 3), ('aniso_2x2x1', 4, 16, 3), ('q1_strip', 3, 17, 1), ('q3_2x1x2', 6, 33, 3), ('kc_3x1x2', 4, 15, 1),
         ('cfg5_template', 30, 17, 1))
BASIS_SEED = 3


def cell_thetas(p, nmu):
    import common3d as c3
    return np.ascontiguousarray(np.stack([c3.theta_of(p, mu) for mu in np.linspace(0.15, 1.2, nmu)]))


def panel(S, N, nmu, nt, seed=11):
    """The trajectories U [nt + 1, S, N, nmu] of the GPU cells: a start plus steps of comparable size, seeded; every difference
    U[k + 1] - U[k] is a full random vector (its nc form is far from zero)."""
    rng = np.random.default_rng(seed + 1000 * N + 10 * nmu + nt)
    steps = rng.standard_normal((nt + 1, S, N, nmu)) * (0.5 ** np.arange(nt + 1))[:, None, None, None]
    return np.ascontiguousarray(np.cumsum(steps, axis=0))


def coefficients(nmu, seed=3):
    """coef [nmu, 2]: positive, distinct per column and per entry (a swap of the two columns is visible)."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([0.6 + rng.random(nmu), 1.7 + rng.random(nmu)], axis=1))


def model_from_oracle(p, o, rd, M_blocks, N):
    """The model dict from the oracle's reduced model ``rd`` (Reductor3D.reduce) and the projected mass blocks."""
    import common3d as c3
    S, Q = o.S, o.Q
    blocks = [c3.oracle_dense_blocks(dict(p, N=N), o, rd, ii) for ii in range(S)]
    m = {k: np.stack([b[k] for b in blocks]) for k in ('G_nc', 'G_bb', 'G_rdd', 'r_fd')}
    m['G_ab'] = np.stack([b['G_ab'] for b in blocks], axis=1)
    m['G_aa'] = np.stack([b['G_aa'] for b in blocks], axis=2)
    m['B_sys'] = np.stack([b['B_sys'] for b in blocks], axis=1)
    m.update(nbr=np.asarray(p['grid'].neighbor_slots).reshape(S, 7), M_red=np.stack(M_blocks), f2=np.asarray(o.f2), ceps=np.asarray(o.ceps),
             hdiam=float(o.hdiam))
    assert m['B_sys'].shape == (Q, S, 7, N, N)
    return m


def neighbourhood(nbr, s, X):
    """X [S, N, L] -> the coefficients on the 7 slots of s, [7, N, L], zero where there is no neighbour."""
    out = np.zeros((7,) + X.shape[1:])
    for slot in range(7):
        t = int(nbr[s, slot])
        if t >= 0:
            out[slot] = X[t]
    return out


def quad(x, G, y):
    """x_l^T G y_l per column l."""
    return np.einsum('il,il->l', x, G @ y)


def elliptic_rows(model, thetas, X, phi=None, source=None, drop_boundary_elements=False, drop_cross=False):
    """nc, r, df [S, L] of the columns X [S, N, L] with thetas [L, Q] (and phi [L, K] with a source): the raw rows of
    lrbms3_reduced_estimate_batch (+ lrbms3_reduced_source_terms).  Mutants: ``drop_boundary_elements`` -- the neighbour x
    neighbour blocks of G_nc (the term sum_e ze^T E ze of the factored form) are left out; ``drop_cross`` -- its self x neighbour
    blocks (the term 2 (Cn u) . z)."""
    nbr = model['nbr']
    S, N, L = X.shape
    Q = thetas.shape[1]
    c = (1.0 / np.pi ** 2) * model['hdiam'] ** 2
    nc, r, df = np.zeros((S, L)), np.zeros((S, L)), np.zeros((S, L))
    own = np.zeros(7 * N, dtype=bool)
    own[SELF * N:(SELF + 1) * N] = True
    for s in range(S):
        u7 = neighbourhood(nbr, s, X)                                           # [7, N, L]
        uo = u7.reshape(7 * N, L)
        ur = (thetas.T[None, :, None, :] * u7[:, None, :, :]).reshape(7 * Q * N, L)      # slot, q, j
        G = model['G_nc'][s].copy()
        if drop_boundary_elements:
            G[np.ix_(~own, ~own)] = 0.0
        if drop_cross:
            G[np.ix_(own, ~own)] = 0.0
            G[np.ix_(~own, own)] = 0.0
        nc[s] = quad(uo, G, uo)
        dd = quad(ur, model['G_rdd'][s], ur)
        if source is None:
            ff, fd = model['f2'][s], model['r_fd'][s] @ ur
        else:
            ff = np.einsum('lj,jk,lk->l', phi, source['F2'][s], phi)
            fd = np.einsum('lj,ji,il->l', phi, source['r_fd_K'][:, s], ur)
        r[s] = (ff - 2.0 * fd + dd) * c / model['ceps'][s]
        val = quad(ur, model['G_bb'][s], ur)
        us = u7[SELF]
        for q in range(Q):
            val += 2.0 * thetas[:, q] * quad(us, model['G_ab'][q, s], ur)
            for q2 in range(Q):
                val += thetas[:, q] * thetas[:, q2] * quad(us, model['G_aa'][q, q2, s], us)
        df[s] = val
    return nc, r, df


def time_residual2(model, thetas, dU, keep=None, drop_slot=None, diagonal_inverse=False):
    """[nt, S, nmu] = y^T M_red[s]^-1 y, y = (sum_q theta_qm B_q dU[k])_s, on the kept unknowns (``keep`` [S, N]: False on zero-padded
    basis columns).  Mutants: ``drop_slot`` (one neighbour slot left out of y), ``diagonal_inverse`` (diag(M_red)^-1)."""
    nbr, B, M_red = model['nbr'], model['B_sys'], model['M_red']
    nt, S, N, nmu = dU.shape
    keep = np.ones((S, N), dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    out = np.zeros((nt, S, nmu))
    for s in range(S):
        y = np.zeros((nt, N, nmu))
        for slot in range(7):
            t = int(nbr[s, slot])
            if t < 0 or slot == drop_slot:
                continue
            y += np.einsum('mq,qij,kjm->kim', thetas, B[:, s, slot], dU[:, t])
        ks = keep[s]
        yk = y[:, ks]
        Ms = M_red[s][np.ix_(ks, ks)]
        z = yk / np.diag(Ms)[None, :, None] if diagonal_inverse else np.einsum('ij,kjm->kim', np.linalg.inv(Ms), yk)
        out[:, s] = np.einsum('kim,kim->km', yk, z)
    return out


def estimate_outputs(model, thetas, coef, dt, U, keep=None, phi=None, source=None, drop_slot=None, diagonal_inverse=False,
                     drop_boundary_elements=False, drop_cross=False, shift_source=False, swap_coef=False):
    """The five outputs of the export as a dict (eta_loc [3, nt + 1, S, nmu], time_deriv_nc [nt, S, nmu], time_residual [nt, nmu],
    eta [nt + 1, nmu], est [nmu]) plus the squared parts ``nc_dU`` [nt, S, nmu] (before the clamp) and ``tr2`` [nt, S, nmu].
    U [nt + 1, S, N, nmu]; thetas [nmu, Q]; coef [nmu, 2]; phi [nmu, nt + 1, K] with ``source``.  Further mutants: ``shift_source``
    (U[k] takes the source row k + 1, the last one its own), ``swap_coef`` (the two columns of coef exchanged)."""
    thetas, coef, U = np.asarray(thetas, dtype=np.float64), np.asarray(coef, dtype=np.float64), np.asarray(U, dtype=np.float64)
    L, S, N, nmu = U.shape
    nt = L - 1
    X = np.ascontiguousarray(U.transpose(1, 2, 0, 3)).reshape(S, N, L * nmu)              # column (k, m)
    th = np.tile(thetas, (L, 1))
    ph = None
    if source is not None:
        rows = np.minimum(np.arange(L) + 1, nt) if shift_source else np.arange(L)
        ph = np.asarray(phi, dtype=np.float64)[:, rows].transpose(1, 0, 2).reshape(L * nmu, -1)
    nc, r, df = (x.reshape(S, L, nmu).transpose(1, 0, 2) for x in
                 elliptic_rows(model, th, X, ph, source, drop_boundary_elements, drop_cross))        # [nt + 1, S, nmu]
    dU = U[1:] - U[:-1]
    Xd = np.ascontiguousarray(dU.transpose(1, 2, 0, 3)).reshape(S, N, nt * nmu)
    nc_dU = elliptic_rows(model, np.tile(thetas, (nt, 1)), Xd, None, None, drop_boundary_elements, drop_cross)[0]
    nc_dU = nc_dU.reshape(S, nt, nmu).transpose(1, 0, 2)
    tr2 = time_residual2(model, thetas, dU, keep, drop_slot, diagonal_inverse)
    c0, c1 = (coef[:, 1], coef[:, 0]) if swap_coef else (coef[:, 0], coef[:, 1])
    sc = 2.0 * np.sqrt(dt / 3.0)
    eta = sc * (c0[None] * np.linalg.norm(nc, axis=1) + c1[None] * np.linalg.norm(r + df, axis=1))
    time_residual = np.sqrt(dt / 3.0 * tr2.sum(axis=1))
    time_deriv_nc = np.sqrt(np.maximum(nc_dU, 0.0) / dt)
    est = np.linalg.norm(eta, axis=0) + np.linalg.norm(time_residual, axis=0) + np.sqrt((time_deriv_nc ** 2).sum(axis=(0, 1)))
    return dict(eta_loc=np.stack([nc, r, df]) * sc, time_deriv_nc=time_deriv_nc, time_residual=time_residual, eta=eta, est=est,
                nc_dU=nc_dU, tr2=tr2)


def squared(out, dt):
    """The comparable forms of the outputs: the square roots amplify round-off near zero, so time_deriv_nc and time_residual are
    compared as time_deriv_nc^2 dt and time_residual^2 3 / dt."""
    return dict(eta_loc=np.asarray(out['eta_loc']), tdnc2=np.asarray(out['time_deriv_nc']) ** 2 * dt,
                tr2=np.asarray(out['time_residual']) ** 2 * 3.0 / dt, eta=np.asarray(out['eta']), est=np.asarray(out['est']))


def worst(got, ref, dt):
    """Per output, max |got - ref| / max |ref| of the comparable forms."""
    g, r = squared(got, dt), squared(ref, dt)
    return {k: float(np.abs(g[k] - r[k]).max() / max(np.abs(r[k]).max(), 1e-300)) for k in r}
