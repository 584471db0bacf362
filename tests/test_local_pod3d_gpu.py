"""Local POD basis extension on the GPU, 3D / P2 path: ``lrbms3_local_pod`` (the kernels of the 2D export with the local energy
product of ``lrbms3_energy_product_apply``) against the NumPy reference of tests/local_pod_ref.py on 2 x 1 x 2 subdomains with
n = 60 DoFs (no multiple of 16), and ``extend_basis(method='pod')`` on the 3D reductors end to end.  The bounds are those of
tests/test_local_pod_gpu.py (its module docstring says where each comes from)."""
import numpy as np
import pytest

import common3d as c3
import local_pod_ref as ref
from test_local_pod_gpu import SPAN_TOL

pytestmark = pytest.mark.gpu

NAME, NW = 'q3_2x1x2', 8
_cache = {}


def _setup():
    """(p, d, eng, dense P [S, n, n], mu, full-order trajectory [S, n, nt + 1]) once per module."""
    if not _cache:
        import torch
        from pylrbms_amd.discretize_parabolic_block_swipdg_3d import discretize
        p = c3.make_problem(NAME)
        pd = {'grid': p['grid'], 'lambda': {'functions': p['lambdas'], 'coefficients': p['thetas']}, 'lambda_bar': p['lambda_bar'],
              'lambda_hat': p['lambda_hat'], 'f': p['f'], 'mu_bar': p['mu_bar'], 'mu_hat': p['mu_hat']}
        d, _ = discretize(pd, 0.2, 12)
        eng = d.engine
        assert eng.S == 4 and eng.t.n == 60
        eye = torch.eye(eng.t.n, dtype=torch.float64, device=eng.ctx.device)[None].expand(eng.S, -1, -1).contiguous()
        P = np.stack([ref.sym(x) for x in eng.ctx.energy_product_apply(eng.ops['P_diag'], eye).cpu().numpy()])
        _cache['x'] = (p, d, eng, P, p['mu'], d.solve(p['mu']))
    return _cache['x']


def _run(eng, U, V, nloc, modes, halo=0, **kw):
    import torch
    ctx = eng.ctx
    Vh = np.concatenate([V, np.random.default_rng(99).standard_normal((halo,) + V.shape[1:])]) if halo else V
    Ud, Vd = ctx.from_numpy(U), ctx.from_numpy(Vh)
    nd = torch.as_tensor(np.asarray(nloc, dtype=np.int32)).to(ctx.device)
    sv, ai = ctx.local_pod(eng.ops['P_diag'], Ud, Vd, nd, modes, **kw)
    ai = ai.cpu().numpy()
    return dict(V=Vd.cpu().numpy(), nloc=nd.cpu().numpy().astype(np.int64), sv=sv.cpu().numpy(), added=ai[0].astype(np.int64),
                info=ai[1], U=Ud.cpu().numpy(), V_in=Vh)


def _gram_schmidt_orthonormality(d, U, V, nloc, P):
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D
    from pylrbms_amd.reductor import ExtensionError
    red = ParabolicLRBMSReductor3D(d, bases=[V[s][:, :int(nloc[s])] for s in range(len(nloc))])
    try:
        red.extend_basis(U)
    except ExtensionError:
        pass
    return ref.orthonormality(red.bases.cpu().numpy(), red._nloc, P)


@pytest.mark.parametrize('L', ref.L_VALUES)
def test_against_the_reference(L):
    import torch
    p, d, eng, P, mu, traj = _setup()
    S = eng.S
    U, V, nloc, _ = ref.make_case(P, L, NW, seed=L)
    assert nloc.tolist() == [0, 1, 3, NW] and ref.threshold_margin(U, V, nloc, P) >= 10.0
    P_before = eng.ops['P_diag'].clone()
    out = _run(eng, U, V, nloc, modes=6, halo=1)
    Vr, nloc_r, sv_r, added_r = ref.local_pod_ref(U, V, nloc, P, modes=6)
    assert not out['info'].any()
    assert np.array_equal(out['added'], added_r) and np.array_equal(out['nloc'], nloc_r) and added_r[3] == 0
    worst_sigma = worst_span = 0.0
    for s in range(S):
        sig, W = ref.product_svd(ref.deflate(U[s], V[s], P[s]), P[s])
        resolved, noise = ref.sigma_error(out['sv'][s], sig)
        assert noise <= ref.NOISE
        worst_sigma = max(worst_sigma, resolved)
        k, n0 = int(added_r[s]), int(nloc[s])
        lead = int(np.count_nonzero(sv_r[s, :k] >= 1e-3 * sv_r[s, 0]))
        worst_span = max(worst_span, ref.span_defect(Vr[s][:, n0:n0 + lead], out['V'][s][:, n0:n0 + k], P[s]))
        assert np.array_equal(out['V'][s][:, :n0], V[s][:, :n0]) and np.all(out['V'][s][:, n0 + k:] == 0.0)
    orth = ref.orthonormality(out['V'], out['nloc'], P)
    orth_gs = _gram_schmidt_orthonormality(d, U, V, nloc, P)
    print('local_pod 3D L={}: sigma {:.2e} sigma_1, span {:.2e}, orthonormality {:.2e} (Gram-Schmidt {:.2e})'.format(
        L, worst_sigma, worst_span, orth, orth_gs))
    assert worst_sigma <= ref.SIGMA_TOL
    assert worst_span <= SPAN_TOL
    assert orth <= max(10 * orth_gs, 1e-12)
    assert np.array_equal(out['V'][S], out['V_in'][S]) and np.array_equal(out['U'], U)
    assert torch.equal(eng.ops['P_diag'], P_before)


def test_exactness_and_repeatability():
    import torch
    from pylrbms_amd._native import NativeError
    p, d, eng, P, mu, traj = _setup()
    S, n = eng.S, eng.t.n
    U, V, nloc, _ = ref.make_case(P, 17, NW, seed=2)
    size = eng.ctx.local_pod_work_size(17, NW)
    first = _run(eng, U, V, nloc, 5, work=torch.full((size,), float('nan'), dtype=torch.float64, device=eng.ctx.device))
    again = _run(eng, U, V, nloc, 5)
    for k in ('V', 'sv', 'added', 'nloc', 'info'):
        assert np.array_equal(first[k], again[k]), k
    assert first['added'].tolist() == [5, 5, 5, 0]                # modes truncates, the full slab has no room
    # in the span, a zero column, duplicates: nothing is added, V keeps its bits
    rng = np.random.default_rng(3)
    W = np.stack([V[s][:, :nloc[s]] @ rng.standard_normal((int(nloc[s]), 4)) for s in range(S)])
    W[:, :, 1] = 0.0
    W[:, :, 3] = W[:, :, 0]
    out = _run(eng, W, V, nloc, 4)
    assert not out['added'].any() and np.array_equal(out['V'], V) and np.all(out['sv'][0] == 0.0)
    # subdomains are independent
    U2 = U.copy()
    U2[1] = U[1][:, rng.permutation(17)]
    perm = _run(eng, U2, V, nloc, 5)
    for k in ('V', 'sv', 'added'):
        assert np.array_equal(first[k][[0, 2, 3]], perm[k][[0, 2, 3]]), k
    nd = torch.zeros(S, dtype=torch.int32, device=eng.ctx.device)
    with pytest.raises(NativeError, match='rtol < 1e-7'):
        eng.ctx.local_pod(eng.ops['P_diag'], eng.ctx.zeros(S, n, 4), eng.ctx.zeros(S, n, 4), nd, 2, rtol=1e-8)
    with pytest.raises(NativeError, match=r'L must be in \[1, 128\]'):
        eng.ctx.local_pod(eng.ops['P_diag'], eng.ctx.zeros(S, n, 129), eng.ctx.zeros(S, n, 4), nd, 2)


def test_reduction_over_n_in_pieces_on_the_config5_template():
    """n = 3840 > 512: V^T P R and R^T P R are reduced in 8 pieces that are summed in their order (the work formula's last term).
    No dense product at this size: P is applied by ``lrbms3_energy_product_apply``, the small Gram matrices go to NumPy."""
    import torch
    p = c3.make_problem('cfg5_template')
    eng = c3.engine_of(p).assemble()
    ctx, S, n = eng.ctx, eng.S, eng.t.n
    assert n == 3840
    L, Nw, nl = 17, 6, [0, 1, 3, 6]
    P_diag = eng.ops['P_diag']

    def gram(X, Y):
        return torch.einsum('snk,snl->skl', X, ctx.energy_product_apply(P_diag, Y.contiguous())).cpu().numpy()
    rng = np.random.default_rng(5)
    x = np.linspace(0.0, 1.0, n)
    smooth = np.stack([np.cos(np.pi * j * x) for j in range(Nw + L)], axis=1)                 # well-conditioned, cheap
    B = ctx.from_numpy(np.stack([smooth + 0.01 * rng.standard_normal(smooth.shape) for _ in range(S)]))
    C = np.linalg.cholesky(np.stack([ref.sym(g) for g in gram(B, B)]))
    B = torch.einsum('snk,skl->snl', B, ctx.from_numpy(np.linalg.inv(C).transpose(0, 2, 1)))  # P-orthonormal columns
    V = ctx.zeros(S, n, Nw)
    U = ctx.zeros(S, n, L)
    decay = 10.0 ** (-0.3 * np.arange(L))
    for s in range(S):
        V[s, :, :nl[s]] = B[s, :, :nl[s]]
        O = np.linalg.qr(rng.standard_normal((L, L)))[0]
        U[s] = B[s, :, Nw:] @ ctx.from_numpy(decay[:, None] * O)
        if nl[s]:
            U[s] += B[s, :, :nl[s]] @ ctx.from_numpy(rng.uniform(0.5, 1.5, (nl[s], L)))
    nd = torch.as_tensor(np.array(nl, dtype=np.int32)).to(ctx.device)
    V0 = V.clone()
    size = ctx.local_pod_work_size(L, Nw)
    assert size == S * (2 * n * L + n * 6 + 6 * L + 2 * L * L + 18 * 18 + L + L * 6 + 4 + 8 * 17 * L)
    sv, ai = ctx.local_pod(P_diag, U, V, nd, 4, work=torch.full((size,), float('nan'), dtype=torch.float64, device=ctx.device))
    added, info = ai.cpu().numpy()
    assert not info.any() and added.tolist() == [4, 4, 3, 0] and nd.cpu().tolist() == [4, 5, 6, 6]
    Vh = V.cpu().numpy()
    G = gram(V, V)
    for s in range(S):
        k = nl[s] + int(added[s])
        assert np.abs(G[s][:k, :k] - np.eye(k)).max() <= 1e-12 and np.all(Vh[s][:, k:] == 0.0)
        assert np.array_equal(Vh[s][:, :nl[s]], V0[s, :, :nl[s]].cpu().numpy())
    # the singular values: those of the deflated snapshots, by an eigen-decomposition of their Gram matrix in NumPy
    R = U.clone()
    for _ in range(2):
        R = R - torch.einsum('snk,skl->snl', V0, ctx.from_numpy(gram(V0, R)))
    lam = np.stack([np.linalg.eigvalsh(ref.sym(g))[::-1] for g in gram(R, R)])
    sig = np.sqrt(np.maximum(lam, 0.0))
    svh = sv.cpu().numpy()
    for s in range(S):
        assert ref.sigma_error(svh[s], sig[s])[0] <= ref.SIGMA_TOL
    sv2, ai2 = ctx.local_pod(P_diag, U, V0.clone(), torch.as_tensor(np.array(nl, dtype=np.int32)).to(ctx.device), 4)
    assert torch.equal(sv2, sv) and torch.equal(ai2, ai)


def _reductor(d, empty=False):
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D
    red = ParabolicLRBMSReductor3D(d)                             # order 0: the constant
    if empty:
        eng = d.engine
        red._V, red._nloc = eng.ctx.zeros(eng.S, eng.t.n, 0), np.zeros(eng.S, dtype=np.int64)
    return red


def test_pod_of_a_trajectory_is_optimal():
    p, d, eng, P, mu, traj = _setup()
    Uh = traj.cpu().numpy()
    k = 4
    pod = _reductor(d, empty=True)
    sv, added = pod.extend_basis(traj, method='pod', pod_modes=k)
    gs = _reductor(d, empty=True)
    gs.extend_basis(traj, max_vectors=k)
    assert added.tolist() == [k] * eng.S and gs.local_sizes() == [k] * eng.S and pod.basis_size() == k
    Vp, Vg = pod.bases.cpu().numpy(), gs.bases.cpu().numpy()
    for s in range(eng.S):
        e_pod, e_gs = ref.projection_error2(Uh[s], Vp[s], P[s]), ref.projection_error2(Uh[s], Vg[s], P[s])
        assert e_pod <= e_gs * (1 + 1e-8), s
        assert abs(e_pod - (sv[s, k:] ** 2).sum()) <= 1e-8 * (sv[s] ** 2).sum(), s


def test_end_to_end_reduced_error_is_no_larger_than_with_gram_schmidt():
    from pylrbms_amd.reductor import ExtensionError
    p, d, eng, P, mu, traj = _setup()
    Uh = traj.cpu().numpy()
    k = 3
    errs = {}
    for method in ('pod', 'gram_schmidt'):
        red = _reductor(d)
        if method == 'pod':
            sv, added = red.extend_basis(traj, method='pod', pod_modes=k)
            assert added.tolist() == [k] * eng.S
        else:
            red.extend_basis(traj, max_vectors=1 + k)
        assert red.local_sizes() == [1 + k] * eng.S
        rd = red.reduce()
        u = rd.solve(mu)
        est, parts = rd.estimate(u, mu)
        assert np.isfinite(est) and est > 0
        E = red.reconstruct(u).cpu().numpy() - Uh
        errs[method] = np.sqrt(sum(np.einsum('ij,ij->', E[s], P[s] @ E[s]) for s in range(eng.S)))
        if method == 'pod':
            with pytest.raises(ExtensionError):
                red.extend_basis(red.reconstruct(u), method='pod')
    print('local_pod 3D end to end: energy error of the reduced trajectory, POD {:.3e}, Gram-Schmidt {:.3e}'.format(
        errs['pod'], errs['gram_schmidt']))
    assert errs['pod'] <= errs['gram_schmidt']


def test_reduce_touched_after_a_pod_extension_into_reserved_columns_is_bitwise_the_whole_pass():
    import torch
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D
    p, d, eng, P, mu, traj = _setup()
    red = LRBMSReductor3D(d, order=0)
    red.extend_basis(traj[:, :, 1])
    assert red.reserve(6) == 6
    rd0 = red.reduce()
    slab = red._V
    Ut = traj.clone()
    Ut[[0, 1, 3]] = 0.0                                           # only subdomain 2 sees snapshots
    sv, added = red.extend_basis(Ut, method='pod', pod_modes=3)
    assert added.tolist() == [0, 0, 3, 0] and red._V is slab and red.local_sizes() == [2, 2, 5, 2]
    rd1 = red.reduce(touched=[])                                  # the reductor knows what changed
    assert red.last_reduce_info['incremental'] and red.last_reduce_info['own'] == 1
    assert rd1.out['B_sys'] is rd0.out['B_sys']
    fresh = LRBMSReductor3D(d, red.bases.clone()).reduce()
    for k in eng.ctx.OUT_NAMES:
        assert torch.equal(rd1.out[k], fresh.out[k]), k
