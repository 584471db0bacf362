"""Streamed local POD (incremental HAPOD) on the GPU, 3D / P2 path: ``lrbms3_local_pod_stream_begin / _push / _finish`` (the kernels
of the 2D exports with the local energy product of ``lrbms3_energy_product_apply``) on 2 x 1 x 2 subdomains with n = 60 DoFs (no
multiple of 16, less than two row tiles of the rotate kernel), and ``extend_basis(method='hapod')`` on
``solve_batch(as_snapshots='slabs')`` with the 3D reductors end to end.  The bounds are those of tests/test_local_pod_stream_gpu.py
(its module docstring says where each comes from)."""
import numpy as np
import pytest

import local_pod_stream_ref as sref
from test_local_pod3d_gpu import NW, _gram_schmidt_orthonormality, _reductor, _setup
from test_local_pod_gpu import SPAN_TOL
from test_local_pod_stream_gpu import _run as _run2d
from test_local_pod_stream_gpu import _views

pytestmark = pytest.mark.gpu

_cache = {}


def _run(eng, U, V, nloc, keep, cmax, modes, **kw):
    return _run2d(eng, U, V, nloc, keep, cmax, modes, P_diag=eng.ops['P_diag'], **kw)


@pytest.mark.parametrize('chunking', sref.EXACT_CHUNKINGS)
def test_exact_inputs_against_the_svd_in_the_product(chunking):
    L, cmax, keep = chunking
    p, d, eng, P, mu, traj = _setup()
    S, n = eng.S, eng.t.n
    U, V, nloc, _ = sref.make_case(P, L, NW, seed=n)
    assert nloc.tolist() == [0, 1, 3, NW] and sref.final_margin(U, V, nloc, P) >= 10.0
    out = _run(eng, U, V, nloc, keep, cmax, modes=6, halo=1)
    nodes = len(sref.chunks(L, cmax))
    assert not out['info'].any() and out['kb'].max() <= keep
    worst_sigma = worst_span = 0.0
    for s in range(S):
        R = sref.deflate(U[s], V[s], P[s])
        sig, W = sref.product_svd(R, P[s])
        norm0 = np.sqrt(np.einsum('ij,ij->j', U[s], P[s] @ U[s]).max())
        k, n0 = min(int(np.count_nonzero(sig > 1e-6 * norm0)), 6, NW - int(nloc[s])), int(nloc[s])
        assert out['added'][s] == k and out['nloc'][s] == n0 + k
        worst_sigma = max(worst_sigma, sref.sigma_error(out['sv'][s], sig)[0])
        lead = int(np.count_nonzero(sig[:k] >= 1e-3 * sig[0]))
        new = out['V'][s][:, n0:n0 + k]
        worst_span = max(worst_span, sref.span_defect(W[:, :lead], new, P[s]))
        e = sref.projection_error2(R, new, P[s])
        assert abs(e - (sig[k:] ** 2).sum()) <= 1e-8 * (sig ** 2).sum()
        assert e <= out['lost'][s] * (1 + 1e-8)
        assert np.array_equal(out['V'][s][:, :n0], V[s][:, :n0]) and np.all(out['V'][s][:, n0 + k:] == 0.0)
    assert out['added'][3] == 0 and np.array_equal(out['V'][3], V[3])      # the full subdomain: its slab bits unchanged
    orth = sref.orthonormality(out['V'], out['nloc'], P)
    orth_gs = _gram_schmidt_orthonormality(d, U[:, :, :min(L, 64)], V, nloc, P)
    print('local_pod_stream 3D L={} cmax={} keep={}: sigma {:.2e} sigma_1, span {:.2e}, orthonormality {:.2e} (Gram-Schmidt {:.2e})'.format(
        L, cmax, keep, worst_sigma, worst_span, orth, orth_gs))
    assert worst_sigma <= sref.SIGMA_TOL * (nodes + 1)
    assert worst_span <= SPAN_TOL
    assert orth <= max(10 * orth_gs, 1e-12)
    assert np.array_equal(out['V'][S], out['V_in'][S]) and np.array_equal(out['U'], U)


def test_truncating_inputs_against_the_restatement():
    n, keep, L, cmax = case = (60, 5, 130, 7)
    assert case in sref.TRUNCATING_CASES
    p, d, eng, P, mu, traj = _setup()
    U, V, nloc, _ = sref.make_truncating_case(P, L, NW, seed=sref.TRUNCATING_SEED)
    want = sref.stream_ref(U, V, nloc, P, keep, cmax, modes=keep)
    assert sref.node_gap(want['streams'], keep) >= sref.GAP_MIN      # the condition the tolerance rests on
    out = _run(eng, U, V, nloc, keep, cmax, modes=keep)
    assert not out['info'].any()
    pushed = np.minimum(np.cumsum([c1 - c0 for c0, c1 in sref.chunks(L, cmax)]), keep)
    assert np.array_equal(out['kb'], want['kb']) and np.array_equal(out['kb'], np.repeat(pushed[:, None], eng.S, axis=1))
    assert np.array_equal(out['added'], want['added']) and out['added'].max() == keep
    s1 = want['sv'].max(axis=1)
    dsv = (np.abs(out['sv'] - want['sv']).max(axis=1) / s1).max()
    dlost = (np.abs(out['lost'] - want['lost']) / s1 ** 2).max()
    print('local_pod_stream 3D truncating {}: sv {:.2e} sigma_1, lost {:.2e} sigma_1^2'.format(case, dsv, dlost))
    assert dsv <= 1e-9 and dlost <= 1e-9
    for s in range(eng.S):
        R = sref.deflate(U[s], V[s], P[s])
        n0, k = int(nloc[s]), int(out['added'][s])
        assert sref.projection_error2(R, out['V'][s][:, n0:n0 + k], P[s]) <= out['lost'][s] * (1 + 1e-8)
    # both routes of the rotation, the same basis (row tail: 60 = 32 + 28)
    eng.ctx.set_option('pod_rotate_valu', 1)
    try:
        valu = _run(eng, U, V, nloc, keep, cmax, modes=keep)
    finally:
        eng.ctx.set_option('pod_rotate_valu', 0)
    assert np.array_equal(valu['kb'], out['kb']) and np.array_equal(valu['added'], out['added'])
    assert np.abs(valu['sv'] - out['sv']).max() <= 1e-12 * out['sv'].max()


def test_bits_and_refusals():
    import torch
    from pylrbms_amd._native import NativeError
    p, d, eng, P, mu, traj = _setup()
    S, n = eng.S, eng.t.n
    ctx = eng.ctx
    U, V, nloc, _ = sref.make_truncating_case(P, 50, NW, seed=2)
    assert ctx.lib.lrbms3_local_pod_stream_state_size(ctx.handle, 8, 17) == S * (2 * n * 25 + 3)
    assert ctx.lib.lrbms3_local_pod_stream_work_size(ctx.handle, 8, 17, NW) == S * (
        2 * n * 17 + 2 * n * 8 + NW * 17 + 2 * 25 * 25 + 26 * 26 + 25 + 25 * 8 + 4)
    first = _run(eng, U, V, nloc, 8, 17, 5, halo=1)
    again = _run(eng, U, V, nloc, 8, 17, 5, halo=1, poison=True)
    for k in ('V', 'sv', 'added', 'nloc', 'info', 'lost', 'kb'):
        assert np.array_equal(first[k], again[k]), k
    assert first['added'].tolist() == [5, 5, 5, 0] and np.array_equal(first['V'][S], first['V_in'][S])
    stream = again['stream']
    stream.begin()
    v = _views(stream)
    assert not v['X'].any() and not v['PX'].any() and not v['kb'].any() and not v['lost'].any()
    nd = torch.zeros(S, dtype=torch.int32, device=ctx.device)
    with pytest.raises(NativeError, match='keep must be in'):
        ctx.local_pod_stream(eng.ops['P_diag'], ctx.zeros(S, n, 4), nd, keep=65, cmax=8)
    with pytest.raises(NativeError, match='keep \\+ cmax must be <= 128'):
        ctx.local_pod_stream(eng.ops['P_diag'], ctx.zeros(S, n, 4), nd, keep=64, cmax=65)
    ok = ctx.local_pod_stream(eng.ops['P_diag'], ctx.zeros(S, n, 4), nd, keep=8, cmax=8)
    ok.push(ctx.zeros(S, n, 3))
    with pytest.raises(NativeError, match='rtol < 1e-7'):
        ok.finish(2, rtol=1e-8)
    with pytest.raises(NativeError, match='modes must be >= 1'):
        ok.finish(0)


def test_stream_on_the_config5_template_with_the_reduction_over_n_in_pieces():
    """n = 3840 > 512: the Gram matrices are reduced in 8 pieces (the work formula's last term) and the rotate kernel walks 120 row
    tiles per panel.  No dense product at this size: the inputs of the single-call test of this shape, pushed in three pieces, give
    the singular values of all deflated columns (nothing truncates: 17 directions <= keep) and a P-orthonormal extension."""
    import torch
    import common3d as c3
    p = c3.make_problem('cfg5_template')
    eng = c3.engine_of(p).assemble()
    ctx, S, n = eng.ctx, eng.S, eng.t.n
    assert n == 3840
    L, Nw, nl, keep, cmax = 17, 6, [0, 1, 3, 6], 20, 7
    P_diag = eng.ops['P_diag']

    def gram(X, Y):
        return torch.einsum('snk,snl->skl', X, ctx.energy_product_apply(P_diag, Y.contiguous())).cpu().numpy()
    rng = np.random.default_rng(5)
    x = np.linspace(0.0, 1.0, n)
    smooth = np.stack([np.cos(np.pi * j * x) for j in range(Nw + L)], axis=1)
    B = ctx.from_numpy(np.stack([smooth + 0.01 * rng.standard_normal(smooth.shape) for _ in range(S)]))
    C = np.linalg.cholesky(np.stack([sref.sym(g) for g in gram(B, B)]))
    B = torch.einsum('snk,skl->snl', B, ctx.from_numpy(np.linalg.inv(C).transpose(0, 2, 1)))  # P-orthonormal columns
    V, U = ctx.zeros(S, n, Nw), ctx.zeros(S, n, L)
    decay = 10.0 ** (-0.3 * np.arange(L))
    for s in range(S):
        V[s, :, :nl[s]] = B[s, :, :nl[s]]
        U[s] = B[s, :, Nw:] @ ctx.from_numpy(decay[:, None] * np.linalg.qr(rng.standard_normal((L, L)))[0])
        if nl[s]:
            U[s] += B[s, :, :nl[s]] @ ctx.from_numpy(rng.uniform(0.5, 1.5, (nl[s], L)))
    V0 = V.clone()
    Lx = keep + cmax
    assert ctx.lib.lrbms3_local_pod_stream_work_size(ctx.handle, keep, cmax, Nw) == S * (
        2 * n * 20 + 2 * n * keep + Nw * 20 + 2 * Lx * Lx + 28 * 28 + Lx + Lx * keep + 4 + 8 * Lx * Lx)
    results = []
    for route in (0, 1, 0):
        ctx.set_option('pod_rotate_valu', route)
        try:
            Vr = V0.clone()
            nd = torch.as_tensor(np.array(nl, dtype=np.int32)).to(ctx.device)
            stream = ctx.local_pod_stream(P_diag, Vr, nd, keep=keep, cmax=cmax)
            stream.work.fill_(float('nan'))
            stream.push(U)                                            # 17 columns: pieces of 7, 7, 3
            sv, ai, lost = stream.finish(4)
        finally:
            ctx.set_option('pod_rotate_valu', 0)
        assert stream.nodes == 3 and stream.columns == L
        results.append((Vr, sv, ai, lost, nd))
    Vr, sv, ai, lost, nd = results[0]
    assert all(torch.equal(a, b) for a, b in zip(results[0], results[2]))                     # the same bits again
    added, info = ai.cpu().numpy()
    assert not info.any() and added.tolist() == [4, 4, 3, 0] and nd.cpu().tolist() == [4, 5, 6, 6]
    assert torch.equal(results[1][2], ai) and float((results[1][1] - sv).abs().max()) <= 1e-12 * float(sv.max())
    Vh, G = Vr.cpu().numpy(), gram(Vr, Vr)
    for s in range(S):
        k = nl[s] + int(added[s])
        assert np.abs(G[s][:k, :k] - np.eye(k)).max() <= 1e-12 and np.all(Vh[s][:, k:] == 0.0)
        assert np.array_equal(Vh[s][:, :nl[s]], V0[s, :, :nl[s]].cpu().numpy())
    R = U.clone()
    for _ in range(2):
        R = R - torch.einsum('snk,skl->snl', V0, ctx.from_numpy(gram(V0, R)))
    lam = np.stack([np.linalg.eigvalsh(sref.sym(g))[::-1] for g in gram(R, R)])
    sig = np.sqrt(np.maximum(lam, 0.0))
    svh, losth = sv.cpu().numpy(), lost.cpu().numpy()
    for s in range(S):
        assert sref.sigma_error(svh[s], sig[s])[0] <= sref.SIGMA_TOL * 4
        tail = (sig[s][int(added[s]):] ** 2).sum()
        assert abs(losth[s] - tail) <= 1e-8 * (sig[s] ** 2).sum()                               # exact: lost is the tail of the spectrum


def _training_set():
    if 'training' not in _cache:
        p, d, eng, P, mu, traj = _setup()
        mus = [float(v) for v in np.linspace(0.3, 0.9, 11)]
        slabs = d.solve_batch(mus, as_snapshots='slabs')
        nt = d.time_stepper.nt
        assert len(mus) * nt > 128 and len(slabs) == nt and all(tuple(u.shape) == (eng.S, eng.t.n, len(mus)) for u in slabs)
        assert all(u.is_contiguous() for u in slabs)
        with pytest.raises(ValueError):
            d.solve_batch(mus, as_snapshots=True)
        _cache['training'] = (mus, slabs, np.concatenate([u.cpu().numpy() for u in slabs], axis=2))
    return _cache['training']


def test_hapod_of_a_training_set_end_to_end():
    """n = 60 <= keep = 64: nothing is truncated on the way, so the k modes of the 132 columns are THE k POD modes."""
    import torch
    p, d, eng, P, mu, traj = _setup()
    mus, slabs, allcols = _training_set()
    k = 4
    red = _reductor(d, empty=True)
    sv, added = red.extend_basis(slabs, method='hapod', pod_modes=k)
    assert added.tolist() == [k] * eng.S and red.basis_size() == k
    info = red.last_pod_info
    assert info['columns'] == allcols.shape[2] and info['nodes'] == len(slabs)
    pod = _reductor(d, empty=True)
    pod.extend_basis(torch.cat(list(slabs), dim=2), method='pod', pod_modes=k)
    Vh, Vp = red.bases.cpu().numpy(), pod.bases.cpu().numpy()
    for s in range(eng.S):
        sig, _ = sref.product_svd(allcols[s], P[s])
        e = sref.projection_error2(allcols[s], Vh[s], P[s])
        assert e <= sref.projection_error2(allcols[s], Vp[s][:, :k], P[s]) * (1 + 1e-8), s
        assert abs(e - (sig[k:] ** 2).sum()) <= 1e-8 * (sig ** 2).sum(), s
        assert e <= info['lost'][s] * (1 + 1e-8), s
    # on the order-0 basis: reduce and solve run on the result
    red = _reductor(d)
    sv, added = red.extend_basis(slabs, method='hapod', pod_modes=3)
    assert added.tolist() == [3] * eng.S and red.local_sizes() == [4] * eng.S
    rd = red.reduce()
    u = rd.solve(mu)
    est, parts = rd.estimate(u, mu)
    assert np.isfinite(est) and est > 0


def test_reduce_touched_after_a_hapod_extension_into_reserved_columns_is_bitwise_the_whole_pass():
    import torch
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D
    p, d, eng, P, mu, traj = _setup()
    mus, slabs, allcols = _training_set()
    red = LRBMSReductor3D(d, order=0)
    red.extend_basis(traj[:, :, 1])
    assert red.reserve(6) == 6
    rd0 = red.reduce()
    slab = red._V
    masked = []
    for u in slabs:
        u = u.clone()
        u[[0, 1, 3]] = 0.0                                        # only subdomain 2 sees snapshots
        masked.append(u)
    sv, added = red.extend_basis(masked, method='hapod', pod_modes=3)
    assert added.tolist() == [0, 0, 3, 0] and red._V is slab and red.local_sizes() == [2, 2, 5, 2]
    rd1 = red.reduce(touched=[])
    assert red.last_reduce_info['incremental'] and red.last_reduce_info['own'] == 1
    assert rd1.out['B_sys'] is rd0.out['B_sys']
    fresh = LRBMSReductor3D(d, red.bases.clone()).reduce()
    for k in eng.ctx.OUT_NAMES:
        assert torch.equal(rd1.out[k], fresh.out[k]), k
