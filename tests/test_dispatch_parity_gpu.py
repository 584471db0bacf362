"""Every branch of the fused project+estimate pass's (Q, N) dispatch against the CPU oracle -- runs on the MI355X box (`-m gpu`).

``launch_project_estimate_fused`` (csrc/fused.hip) picks its projection kernel by the number of affine components Q and the basis
width N (k_f1w, k_f1v, k_f1u<ntx, Q>, the producer / consumer k_f1<ntx, 7, Q|0> in 1 .. 3 slices of column groups), k_f2<NR> by
NR = ceil(QN / 16), k_f3 / k_coupling / the thin kernels by ntx = ceil(N / 16), and falls back to the unfused kernels where
``fused_supported`` says no (Q N > 128, Q > 4).  One cell per branch: every assembled, projected and estimated array against the
oracle (1e-11 relative), the reduced solve (1e-10), fused against unfused in both output layouts, the timing name of the
projection kernel that ran, forced K-splits from NaN-poisoned buffers, and the batched panel solve of 16 / 17 parameters.

Then zero-padded ragged bases (what ``LRBMSReductor.reserve`` leaves behind): the padded rows and columns of every output are
exactly 0, and the reduced solves and estimates agree with the oracle on the UNPADDED bases."""
import numpy as np
import pytest

from common import (compare_all, energy_orthonormalize, make_bases, oracle_from_problem, problem_with_q_components,
                    ragged_padded_bases, theta_bar_of, theta_of)

pytestmark = pytest.mark.gpu

TOL = 1e-11
SOLVE_TOL = 1e-10
FORMS = ('k_f1w', 'k_f1v', 'k_f1u', 'k_f1')
NAMES = ('B_sys', 'rhs_red', 'E_red', 'M_red', 'G_nc', 'r_fd', 'G_rdd', 'G_bb', 'G_ab', 'G_aa')

# (Q, N, subdomains, k_c, timing name of the projection kernel -- None: fused_supported is false, the unfused kernels run).
# Comments: the instantiation the launcher selects; "slices": column-group slices of k_f1 in grid.y (Q + 2 + Q (Q + 1) / 2 + Q^2
# groups, at most min(12, 448 / N) per slice); NR: the k_f2<NR> instantiation.
CELLS = [
    (1, 1, (3, 2), 2, 'k_f1u'),       # k_f1u<1, 1>, NR 1
    (1, 16, (3, 2), 2, 'k_f1u'),      # k_f1u<1, 1>, NR 1 (one full column tile)
    (1, 17, (3, 2), 2, 'k_f1u'),      # k_f1u<2, 1>, NR 2
    (1, 32, (3, 2), 2, 'k_f1u'),      # k_f1u<2, 1>, NR 2
    (1, 40, (3, 2), 2, 'k_f1u'),      # k_f1u<3, 1>, NR 3
    (1, 48, (3, 2), 2, 'k_f1u'),      # k_f1u<3, 1>, NR 3
    (1, 49, (3, 2), 2, 'k_f1'),       # k_f1<4, 7, 1>, one slice, NR 4
    (1, 64, (3, 2), 2, 'k_f1'),       # k_f1<4, 7, 1>, NR 4
    (2, 22, (3, 2), 2, 'k_f1v'),      # k_f1v<2, 2, 1, 3, 0>, NR 3
    (2, 26, (3, 2), 2, 'k_f1u'),      # k_f1u<2, 2> (no k_f1v instantiation for its levels), NR 4
    (2, 32, (3, 2), 2, 'k_f1u'),      # k_f1u<2, 2>, full second tile, NR 4
    (2, 33, (3, 2), 2, 'k_f1u'),      # k_f1u<3, 2>, odd N, NR 5
    (2, 39, (3, 2), 2, 'k_f1u'),      # k_f1u<3, 2>, odd N, NR 5
    (2, 41, (3, 3), 4, 'k_f1'),       # k_f1<3, 7, 0>, 2 slices, NR 6 (config 3's template after one enrichment round)
    (2, 42, (3, 3), 4, 'k_f1'),       # k_f1<3, 7, 0>, 2 slices, NR 6
    (2, 48, (3, 3), 4, 'k_f1'),       # k_f1<3, 7, 0>, 2 slices, NR 6
    (2, 50, (3, 3), 4, 'k_f1'),       # k_f1<4, 7, 0>, 2 slices, NR 7
    (2, 56, (3, 2), 2, 'k_f1'),       # k_f1<4, 7, 0>, 2 slices, NR 7
    (2, 63, (3, 2), 2, 'k_f1'),       # k_f1<4, 7, 0>, odd N, 2 slices, NR 8
    (3, 1, (3, 2), 2, 'k_f1'),        # runtime-Q producer k_f1<1, 7, 0>, 2 slices, NR 1
    (3, 5, (3, 2), 2, 'k_f1'),        # k_f1<1, 7, 0>, NR 1
    (3, 16, (3, 2), 2, 'k_f1'),       # k_f1<1, 7, 0>, NR 3
    (3, 21, (3, 2), 2, 'k_f1'),       # k_f1<2, 7, 0>, NR 4
    (3, 32, (3, 2), 2, 'k_f1'),       # k_f1<2, 7, 0>, NR 6
    (3, 37, (3, 2), 2, 'k_f1'),       # k_f1<3, 7, 0>, NR 7
    (3, 42, (3, 2), 2, 'k_f1'),       # k_f1<3, 7, 0>, NR 8 (QN = 126)
    (3, 43, (3, 2), 2, None),         # QN = 129
    (4, 2, (3, 2), 2, 'k_f1'),        # k_f1<1, 7, 0>, 3 slices, NR 1
    (4, 8, (3, 2), 2, 'k_f1'),        # k_f1<1, 7, 0>, 3 slices, NR 2
    (4, 17, (3, 2), 2, 'k_f1'),       # k_f1<2, 7, 0>, 3 slices, NR 5
    (4, 24, (3, 2), 2, 'k_f1'),       # k_f1<2, 7, 0>, 3 slices, NR 6
    (4, 28, (3, 2), 2, 'k_f1'),       # k_f1<2, 7, 0>, 3 slices, NR 7
    (4, 32, (3, 2), 2, 'k_f1'),       # k_f1<2, 7, 0>, 3 slices, NR 8 (QN = 128, the largest fused shape)
    (4, 33, (3, 2), 2, None),         # QN = 132
    (6, 10, (3, 2), 2, None),         # Q > 4: unfused projection, online kernels at Q = 6
    (8, 16, (3, 2), 2, None),         # Q = 8, QN = 128
]


def _engine(p):
    from pylrbms_amd.engine import Engine
    lam = p['lambda']
    return Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'],
                  theta_bar_of(p)).assemble()


def _problem(Q, shape, kc):
    """Q = 2: the multiscale problem itself (config 3's data); any other Q: the same grid with Q seeded lognormal components."""
    if Q == 2:
        from pylrbms_amd import multiscale_problem
        return multiscale_problem.init_grid_and_problem({'num_subdomains': list(shape), 'coarse_per_subdomain': kc})
    return problem_with_q_components(shape, kc, Q)


def _mus(p, count, seed):
    size = p['parameter_type']['diffusion'][0]
    return [tuple(row) for row in np.random.default_rng(seed).uniform(0.1, 1.0, size=(count, size))]


def _host(x):
    return x.detach().cpu().numpy()


def _outputs(buf):
    from pylrbms_amd.engine import expand_factored_grams
    return list(buf['sys']) + list(expand_factored_grams(buf['grams']))


def _poison(buf):
    for x in list(buf['sys']) + list(buf['grams']) + [buf['work']]:
        x.fill_(float('nan'))


def _ran(eng, fn):
    eng.ctx.kernel_timing(True)
    try:
        fn()
        return {k for k, _ in eng.ctx.kernel_timing_read()}
    finally:
        eng.ctx.kernel_timing(False)


def _check_batch_solve(eng, p, rd, B_sys, rhs_red, seed):
    """reduced_solve_batch: 17 parameters (one-column last group) for Q <= 4, 16 for Q > 4 -- every column against the oracle's
    dense solve; 17 at Q > 4 is refused by the host-side check."""
    from pylrbms_amd._native import NativeError
    Q = eng.Q
    nmu = 17 if Q <= 4 else 16
    mus = _mus(p, nmu, seed)
    thetas = np.stack([theta_of(p, mu) for mu in mus])
    ub, info = eng.ctx.reduced_solve_batch(thetas, B_sys, rhs_red)
    assert info['relative_residual'] <= 1e-13
    ub = _host(ub)
    for m, mu in enumerate(mus):
        ref = np.stack(rd.solve(mu))
        assert np.linalg.norm(ub[:, :, m] - ref) < SOLVE_TOL * np.linalg.norm(ref), m
    if Q > 4:
        more = np.concatenate([thetas, thetas[:1]])
        with pytest.raises(NativeError, match='Q <= 4'):
            eng.ctx.reduced_solve_batch(more, B_sys, rhs_red)


@pytest.mark.parametrize('Q, N, shape, kc, form', CELLS, ids=['Q{}-N{}'.format(c[0], c[1]) for c in CELLS])
def test_dispatch_cell_matches_the_oracle(Q, N, shape, kc, form):
    from oracle.lrbms import OracleReductor
    p = _problem(Q, shape, kc)
    eng = _engine(p)
    d = oracle_from_problem(p)
    assert eng.Q == Q and d.Q == Q
    fused = form is not None
    assert eng.ctx.fused_supported(Q, N) == fused and eng.ctx.fused_supported(Q, N, factored=True) == fused
    V = energy_orthonormalize(make_bases(d.S, d.n, N, seed=3), d)
    mu = _mus(p, 1, seed=1000 + N)[0]
    res = compare_all(p, eng, V, mu, oracle=d)
    assert res.pop('cg_iterations') > 0
    assert fused == ('fused_B_sys' in res) == ('fused_dense_B_sys' in res) == ('eta_batch_factored' in res)
    bad = {k: v for k, v in res.items() if not (v < (SOLVE_TOL if k == 'u_solve' else TOL))}
    assert not bad, bad
    rd = OracleReductor(d, [V[ii] for ii in range(d.S)]).reduce()
    Vd = eng.ctx.from_numpy(V)
    ref = eng.project_and_estimate(Vd, fused=False)                   # the unfused kernels compare_all has just checked
    if not fused:
        assert eng.project_and_estimate(Vd)['Wt'] is not None         # the default path is the unfused one (image bases formed)
        _check_batch_solve(eng, p, rd, ref['sys'][0], ref['sys'][1], seed=N)
        return
    ref = [x.clone() for x in _outputs(ref)]
    floor = float(np.abs(V).max()) ** 2 * 1e-3                        # as compare_all: N = 1 has exactly-zero gradient blocks
    scale = [max(float(x.abs().max()), floor) for x in ref]
    nch = p['grid'].template.n_T // 4                                  # K-chunks of four elements
    splits = (1, 2, 4) if nch % 16 == 0 else (1, 2)
    other = set(FORMS) - {form}
    bufs = {True: eng.alloc_reduce_buffers(N, factored=True), False: eng.alloc_reduce_buffers(N, factored=False)}
    failures = []
    try:
        for factored in (True, False):
            # factored: the default launch policy (k_thin3); dense: serial launches and the LDS preparation without the G_nc fold,
            # so that k_f3, k_coupling and the separate thin kernels run as well
            eng.ctx.set_option('streams', -1 if factored else 0)
            eng.ctx.set_option('prep_lds', 1 if factored else 2)
            buf = bufs[factored]
            for ks in splits:
                eng.ctx.set_option('f1_ksplit', ks)
                _poison(buf)
                ran = _ran(eng, lambda: eng.project_and_estimate(Vd, buf, fused=True))
                assert form in ran and not (other & ran), (factored, ks, sorted(ran))
                want = {'k_f2', 'k_thin3'} if factored else {'k_f2', 'k_f3', 'k_coupling', 'k_thin_nc', 'k_thin_rt', 'k_thin_expand'}
                assert want <= ran, (factored, ks, sorted(ran))
                for name, a, b, s in zip(NAMES, _outputs(buf), ref, scale):
                    err = float((a - b).abs().max()) / s
                    if not err <= TOL:                                 # (NaN fails too)
                        failures.append((factored, ks, name, err))
    finally:
        for k, v in (('f1_ksplit', 0), ('streams', -1), ('prep_lds', 1)):
            eng.ctx.set_option(k, v)
    assert not failures, failures
    buf = eng.project_and_estimate(Vd)
    _check_batch_solve(eng, p, rd, buf['sys'][0], buf['sys'][1], seed=N)


def test_nine_affine_components_are_refused():
    """The C ABI takes Q in 1 .. 8: a ninth component is refused by the argument check of the first assembly call."""
    from pylrbms_amd._native import NativeError
    p = problem_with_q_components((2, 2), 2, 9)
    with pytest.raises(NativeError, match='Q must be in 1..8'):
        _engine(p)


# ---------------------------------------------------------------------- zero-padded ragged bases

def _pad_masks(grid, sizes, Q, N):
    """Per output (dense layout, as expand_factored_grams returns it): True where a row or column belongs to a zero column of the
    slab -- of the subdomain itself or of the neighbour in that slot.  Slots without a neighbour are not padding and stay False."""
    S = len(sizes)
    pad = [np.arange(N) >= sizes[s] for s in range(S)]
    slots = np.asarray(grid.neighbor_slots)

    def slot_pad(s, k):
        j = int(slots[s, k])
        return pad[j] if j >= 0 else np.zeros(N, dtype=bool)
    m = {name: None for name in NAMES}
    m['B_sys'] = np.zeros((Q, S, 5, N, N), dtype=bool)
    m['rhs_red'] = np.stack(pad)
    m['E_red'] = m['M_red'] = np.stack([pad[s][:, None] | pad[s][None, :] for s in range(S)])
    m['G_nc'] = np.zeros((S, 5 * N, 5 * N), dtype=bool)
    m['r_fd'] = np.zeros((S, 5 * Q * N), dtype=bool)
    for key in ('G_rdd', 'G_bb'):
        m[key] = np.zeros((S, 9, Q * N, Q * N), dtype=bool)
    m['G_ab'] = np.zeros((Q, S, N, 5 * Q * N), dtype=bool)
    m['G_aa'] = np.broadcast_to(m['E_red'][None, None], (Q, Q, S, N, N)).copy()
    for s in range(S):
        hood = [slot_pad(s, k) if slots[s, k] >= 0 else None for k in range(5)]
        assert int(slots[s, 2]) == s
        for k in range(5):
            if hood[k] is None:
                continue
            m['B_sys'][:, s, k] = pad[s][:, None] | hood[k][None, :]
            m['r_fd'][s, k * Q * N:(k + 1) * Q * N] = np.tile(hood[k], Q)
            m['G_ab'][:, s, :, k * Q * N:(k + 1) * Q * N] = pad[s][:, None] | np.tile(hood[k], Q)[None, :]
            for k2 in range(5):
                if hood[k2] is not None:
                    m['G_nc'][s, k * N:(k + 1) * N, k2 * N:(k2 + 1) * N] = hood[k][:, None] | hood[k2][None, :]
        selfq = np.tile(pad[s], Q)
        for key in ('G_rdd', 'G_bb'):
            m[key][s, 0] = selfq[:, None] | selfq[None, :]
            for side, k in enumerate((0, 1, 3, 4)):
                if hood[k] is not None:
                    aq = np.tile(hood[k], Q)
                    m[key][s, 1 + side] = aq[:, None] | selfq[None, :]
                    m[key][s, 5 + side] = aq[:, None] | aq[None, :]
    return m


RAGGED = [
    (2, 7, (3, 2), 2, 'k_f1u'),
    (2, 22, (3, 2), 2, 'k_f1v'),
    (2, 38, (3, 2), 2, 'k_f1w'),      # zeros inside k_f1w's packed tails of the symmetric groups
    (2, 40, (3, 3), 4, 'k_f1w'),      # config 3's width and template
    (2, 42, (3, 3), 4, 'k_f1'),       # ... after one enrichment round: the two-slice producer
    (2, 50, (3, 2), 2, 'k_f1'),
    (2, 64, (3, 2), 2, 'k_f1'),
    (1, 49, (3, 2), 2, 'k_f1'),
    (4, 32, (3, 2), 2, 'k_f1'),       # three slices, k_f2<8>
]


@pytest.mark.parametrize('Q, N, shape, kc, form', RAGGED, ids=['Q{}-N{}'.format(c[0], c[1]) for c in RAGGED])
def test_zero_padded_ragged_bases(Q, N, shape, kc, form):
    """``reserve`` rests on "zero columns project to zero rows / columns": the oracle on the padded slab, exact zeros in every padded
    row and column of every output (both layouts, from NaN-poisoned buffers), the padded unknowns of the single and the batched
    reduced solve exactly 0 with their real entries equal to the oracle's solve on the unpadded bases, and the estimates of the
    padded model equal to the oracle's on the unpadded bases."""
    import torch
    from oracle.lrbms import OracleReductor
    p = _problem(Q, shape, kc)
    eng = _engine(p)
    d = oracle_from_problem(p)
    assert eng.ctx.fused_supported(Q, N) and eng.ctx.fused_supported(Q, N, factored=True)
    V, sizes = ragged_padded_bases(d, N, seed=40 + N)
    assert max(sizes) == N and min(sizes) < N
    mu = _mus(p, 1, seed=2000 + N)[0]
    res = compare_all(p, eng, V, mu, do_solve=False, oracle=d)
    bad = {k: v for k, v in res.items() if not v < TOL}
    assert not bad, bad
    Vd = eng.ctx.from_numpy(V)
    masks = _pad_masks(p['grid'], sizes, Q, N)
    for factored in (True, False):
        buf = eng.alloc_reduce_buffers(N, factored=factored)
        _poison(buf)
        ran = _ran(eng, lambda: eng.project_and_estimate(Vd, buf, fused=True))
        assert form in ran, sorted(ran)
        for name, x in zip(NAMES, _outputs(buf)):
            mk = torch.as_tensor(masks[name], device=x.device)
            assert mk.shape == x.shape, (name, mk.shape, x.shape)
            assert bool((x[mk] == 0.0).all()), (factored, name, int((x[mk] != 0.0).sum()))
    # online: against the oracle on the UNPADDED ragged bases
    rd = OracleReductor(d, [V[ii][:, :sizes[ii]] for ii in range(d.S)]).reduce()
    buf = eng.project_and_estimate(Vd)
    B_sys, rhs_red = buf['sys'][0], buf['sys'][1]
    mus = _mus(p, 17, seed=3000 + N)
    thetas = np.stack([theta_of(p, m) for m in mus])
    refs = [rd.solve(m) for m in mus]

    def check(u, ref, tag):
        for ii in range(d.S):
            assert (u[ii, sizes[ii]:] == 0.0).all(), (tag, ii)       # padded unknowns: exactly zero
        got = np.concatenate([u[ii, :sizes[ii]] for ii in range(d.S)])
        want = np.concatenate(ref)
        assert np.linalg.norm(got - want) < SOLVE_TOL * np.linalg.norm(want), tag
    u1, _ = eng.reduced_solve(thetas[0], B_sys, rhs_red)
    check(_host(u1), refs[0], 'single')
    ub, info = eng.ctx.reduced_solve_batch(thetas, B_sys, rhs_red)
    ub = _host(ub)
    for m in range(len(mus)):
        check(ub[:, :, m], refs[m], ('batch', m))
    # estimates of the oracle's solutions, zero-padded into the slab: single-parameter kernel and the batched one
    U = np.zeros((d.S, N, len(mus)))
    for m in range(len(mus)):
        for ii in range(d.S):
            U[ii, :sizes[ii], m] = refs[m][ii]
    eta_b = _host(eng.ctx.reduced_estimate_batch(thetas, eng.ctx.from_numpy(U), buf['grams'], eng.f2, eng.ceps, eng.hdiam))
    for m in (0, 16):
        _, (nc, r, df), _ = rd.estimate(refs[m], mus[m], decompose=True)
        eta_s = _host(eng.reduced_estimate(thetas[m], eng.ctx.from_numpy(np.ascontiguousarray(U[:, :, m])), buf['grams']))
        for row, want in enumerate((nc, r, df)):
            tol = SOLVE_TOL * max(np.abs(want).max(), 1e-300)
            assert np.abs(eta_s[row] - want).max() < tol, (m, row)
            assert np.abs(eta_b[row, :, m] - want).max() < tol, (m, row)
