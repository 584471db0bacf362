"""Streamed local POD (incremental HAPOD) on the GPU, 2D path: ``lrbms_local_pod_stream_begin / _push / _finish`` against the SVD in
the product of ALL pushed columns (exact inputs) and against the NumPy restatement of tests/local_pod_stream_ref.py (truncating
inputs), the rotate kernel alone, bits, degenerate pushes, refusals, and ``extend_basis(method='hapod')`` on
``solve_batch(as_snapshots='slabs')`` end to end.  Meshes and the dense product as in tests/test_local_pod_gpu.py.

Bounds.  Exact inputs: sigma within SIGMA_TOL sigma_1 (nodes + 1) over the resolved values (the Gram route's error once per node),
span within SPAN_TOL of test_local_pod_gpu (100 x the reference-against-SVD defect), orthonormality max(10 x Gram-Schmidt, 1e-12).
Truncating inputs: sv within 1e-9 sigma_1 and lost within 1e-9 sigma_1^2 of the restatement: under the gap condition a Gram
perturbation of 1e-15 moves them by 1.2e-13 at most on the CPU (tests/test_local_pod_stream_host.py), plus the Jacobi tolerance.
Rotate kernel: 8 eps Lx max|X| max|T|."""
import ctypes
import types

import numpy as np
import pytest

import local_pod_stream_ref as sref
from test_local_pod_gpu import CONFIGS, NW, SPAN_TOL, _engine, _gram_schmidt_orthonormality

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MESH_OF_N = {24: '2x2_n24', 96: '3x3_n96'}
_ref_cache = {}


def _views(stream):
    """Views of the state of a stream: X, PX [S, n, Lx], norm0sq, lost [S], kb, flags int32 [S] (the layout of the C header)."""
    import torch
    ctx = stream.ctx
    S, n, Lx = ctx.S, ctx.n, stream.keep + stream.cmax
    st = stream.state
    assert st.numel() == S * (2 * n * Lx + 3)
    m = S * n * Lx
    ints = st[2 * m + 2 * S:].view(torch.int32)
    return dict(X=st[:m].view(S, n, Lx), PX=st[m:2 * m].view(S, n, Lx), norm0sq=st[2 * m:2 * m + S], lost=st[2 * m + S:2 * m + 2 * S],
                kb=ints[:S], flags=ints[S:])


def _T(stream):
    """T [S, Lx, keep] of the last push, in ``work`` at the offset the C header states."""
    ctx = stream.ctx
    S, n, keep, cmax, Nw = ctx.S, ctx.n, stream.keep, stream.cmax, stream.Nw
    Lx = keep + cmax
    Lp, M1 = Lx + (Lx & 1), max(cmax, keep)
    off = S * (2 * n * M1 + 2 * n * keep + Nw * M1 + 2 * Lx * Lx + Lp * Lp + Lx)
    return stream.work[off:off + S * Lx * keep].view(S, Lx, keep)


def _run(eng, U, V, nloc, keep, cmax, modes, halo=0, poison=False, P_diag=None, **kw):
    """begin, the columns of U in pieces of cmax, finish -- on host arrays; ``halo`` extra rows of noise behind V; ``poison``: state
    NaN-filled before a second begin, work NaN-filled.  Returns host arrays (kb [pushes, S] read back after every push)."""
    import torch
    ctx = eng.ctx
    rng = np.random.default_rng(99)
    Vh = np.concatenate([V, rng.standard_normal((halo,) + V.shape[1:])]) if halo else V
    Ud, Vd = ctx.from_numpy(U), ctx.from_numpy(Vh)
    nd = torch.as_tensor(np.asarray(nloc, dtype=np.int32)).to(ctx.device)
    stream = ctx.local_pod_stream(eng.P_diag if P_diag is None else P_diag, Vd, nd, keep=keep, cmax=cmax)
    if poison:
        stream.state.fill_(float('nan'))
        stream.work.fill_(float('nan'))
        stream.begin()
    kb = []
    for c0, c1 in sref.chunks(U.shape[2], cmax):
        stream.push(Ud[:, :, c0:c1])
        kb.append(_views(stream)['kb'].cpu().numpy().copy())
    sv, ai, lost = stream.finish(modes, **kw)
    ai = ai.cpu().numpy()
    return dict(V=Vd.cpu().numpy(), nloc=nd.cpu().numpy().astype(np.int64), sv=sv.cpu().numpy(), added=ai[0].astype(np.int64),
                info=ai[1], lost=lost.cpu().numpy(), kb=np.array(kb), U=Ud.cpu().numpy(), V_in=Vh, stream=stream)


# ------------------------------------------------------------------------------------------------------------- 1: exact inputs
@pytest.mark.parametrize('chunking', sref.EXACT_CHUNKINGS)
@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_exact_inputs_against_the_svd_in_the_product(name, chunking):
    L, cmax, keep = chunking
    d, eng, P = _engine(name)
    S, n = eng.S, eng.t.n
    U, V, nloc, _ = sref.make_case(P, L, NW, seed=n)
    assert {0, 1, 3, NW} <= set(nloc.tolist())                    # ragged: empty, one, odd, full
    assert sref.final_margin(U, V, nloc, P) >= 10.0
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
        resolved, noise = sref.sigma_error(out['sv'][s], sig)
        worst_sigma = max(worst_sigma, resolved)
        lead = int(np.count_nonzero(sig[:k] >= 1e-3 * sig[0]))
        new = out['V'][s][:, n0:n0 + k]
        worst_span = max(worst_span, sref.span_defect(W[:, :lead], new, P[s]))
        e = sref.projection_error2(R, new, P[s])
        assert abs(e - (sig[k:] ** 2).sum()) <= 1e-8 * (sig ** 2).sum()
        assert e <= out['lost'][s] * (1 + 1e-8)
        # old columns bitwise, columns past the new nloc exactly zero; a full subdomain: nothing added, its slab bits unchanged
        assert np.array_equal(out['V'][s][:, :n0], V[s][:, :n0]) and np.all(out['V'][s][:, n0 + k:] == 0.0)
        if n0 == NW:
            assert k == 0 and np.array_equal(out['V'][s], V[s])
    orth = sref.orthonormality(out['V'], out['nloc'], P)
    orth_gs = _gram_schmidt_orthonormality(eng, U[:, :, :min(L, 64)], V, nloc, P)
    print('local_pod_stream {} L={} cmax={} keep={}: sigma {:.2e} sigma_1, span {:.2e}, orthonormality {:.2e} (Gram-Schmidt {:.2e})'.format(
        name, L, cmax, keep, worst_sigma, worst_span, orth, orth_gs))
    assert worst_sigma <= sref.SIGMA_TOL * (nodes + 1)
    assert worst_span <= SPAN_TOL
    assert orth <= max(10 * orth_gs, 1e-12)
    assert np.array_equal(out['V'][S], out['V_in'][S]) and np.array_equal(out['U'], U)      # the halo row and the snapshots


# ------------------------------------------------------------------------------------------------------------- 2: truncating inputs
def _truncating(case):
    """(eng, P, U, V, nloc, restatement) of a truncating case on the mesh with its n, built once."""
    if case not in _ref_cache:
        n, keep, L, cmax = case
        d, eng, P = _engine(MESH_OF_N[n])
        U, V, nloc, _ = sref.make_truncating_case(P, L, NW, seed=sref.TRUNCATING_SEED)
        want = sref.stream_ref(U, V, nloc, P, keep, cmax, modes=keep)
        _ref_cache[case] = (eng, P, U, V, nloc, want)
    return _ref_cache[case]


@pytest.mark.parametrize('case', [c for c in sref.TRUNCATING_CASES if c[0] in MESH_OF_N])
def test_truncating_inputs_against_the_restatement(case):
    n, keep, L, cmax = case
    eng, P, U, V, nloc, want = _truncating(case)
    assert sref.node_gap(want['streams'], keep) >= sref.GAP_MIN      # the condition the tolerance rests on
    out = _run(eng, U, V, nloc, keep, cmax, modes=keep)
    assert not out['info'].any()
    pushed = np.minimum(np.cumsum([c1 - c0 for c0, c1 in sref.chunks(L, cmax)]), keep)
    assert np.array_equal(out['kb'], want['kb']) and np.array_equal(out['kb'], np.repeat(pushed[:, None], eng.S, axis=1))
    assert np.array_equal(out['added'], want['added']) and out['added'].max() == keep
    s1 = want['sv'].max(axis=1)
    dsv = (np.abs(out['sv'] - want['sv']).max(axis=1) / s1).max()
    dlost = (np.abs(out['lost'] - want['lost']) / s1 ** 2).max()
    print('local_pod_stream truncating {}: sv {:.2e} sigma_1, lost {:.2e} sigma_1^2'.format(case, dsv, dlost))
    assert dsv <= 1e-9 and dlost <= 1e-9
    for s in range(eng.S):                                          # the bound on the device result itself
        R = sref.deflate(U[s], V[s], P[s])
        n0, k = int(nloc[s]), int(out['added'][s])
        assert sref.projection_error2(R, out['V'][s][:, n0:n0 + k], P[s]) <= out['lost'][s] * (1 + 1e-8)
    assert sref.orthonormality(out['V'], out['nloc'], P) <= 1e-12


# ------------------------------------------------------------------------------------------------------------- 3: the rotate kernel
@pytest.mark.parametrize('keep,cmax,C', [(3, 4, 3), (64, 1, 1), (32, 64, 64), (64, 64, 64)])
def test_rotate_kernel_alone_and_against_the_xt_route(keep, cmax, C):
    """A crafted state [B | .] (ragged widths of B: none, a few, full), one push: the new B, PB are [B | R | 0] T with the T and R the
    push left behind, columns >= kb exactly zero -- on the MFMA kernel and on the k_pod_xt route."""
    import torch
    d, eng, P = _engine('3x3_n96')
    ctx, S, n = eng.ctx, eng.S, eng.t.n
    Lx = keep + cmax
    rng = np.random.default_rng(Lx)
    widths = [0, min(2, keep), keep, keep, min(5, keep), keep, 1, keep, 0][:S]
    B = np.zeros((S, n, keep))
    for s in range(S):
        B[s][:, :widths[s]] = rng.standard_normal((n, widths[s])) * 10.0 ** rng.uniform(-2, 0, widths[s])
    U = rng.standard_normal((S, n, C))
    U[0] = 0.0                                                      # subdomain 0: no carried modes and a zero chunk -> kb = 0
    V = np.zeros((S, n, NW))
    nd = torch.zeros(S, dtype=torch.int32, device=ctx.device)
    PB = np.einsum('sij,sjk->sik', P, B)
    results = {}
    for route in (0, 1):
        ctx.set_option('pod_rotate_valu', route)
        try:
            stream = ctx.local_pod_stream(eng.P_diag, ctx.from_numpy(V), nd, keep=keep, cmax=cmax)
            v = _views(stream)
            v['X'][:, :, :keep], v['PX'][:, :, :keep] = ctx.from_numpy(B), ctx.from_numpy(PB)
            v['kb'][:] = torch.as_tensor(np.array(widths, dtype=np.int32)).to(ctx.device)
            stream.push(ctx.from_numpy(U))
        finally:
            ctx.set_option('pod_rotate_valu', 0)
        X, PX, T, kb = (x.cpu().numpy() for x in (v['X'], v['PX'], _T(stream), v['kb']))
        results[route] = (X, PX, T, kb)
        for A, A0 in ((X, B), (PX, PB)):
            before = np.concatenate([A0, A[:, :, keep:]], axis=2)  # [B | R | 0]: the rotation leaves the columns from keep on alone
            assert np.all(before[:, :, keep + C:] == 0.0)
            want = np.einsum('sik,skj->sij', before, T)
            for s in range(S):
                tol = 8 * EPS * Lx * np.abs(before[s]).max() * np.abs(T[s]).max()
                assert np.abs(A[s][:, :keep] - want[s]).max() <= tol, (route, s)
                assert np.all(A[s][:, kb[s]:keep] == 0.0) and np.all(T[s][:, kb[s]:] == 0.0)
        assert kb[0] == 0 and kb.max() == min(keep, Lx) and len(set(kb.tolist())) >= 2      # ragged, 0 and keep among them
    assert np.array_equal(results[0][2], results[1][2]) and np.array_equal(results[0][3], results[1][3])      # the same T and kb
    for i in (0, 1):
        for s in range(S):
            before = np.abs(np.concatenate([(B, PB)[i][s], results[0][i][s][:, keep:]], axis=1)).max()
            tol = 8 * EPS * Lx * before * np.abs(results[0][2][s]).max()
            assert np.abs(results[0][i][s][:, :keep] - results[1][i][s][:, :keep]).max() <= tol


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_both_rotate_routes_give_the_same_basis(name):
    """Row tails (n = 24 is less than a tile) through a whole stream, on both routes."""
    d, eng, P = _engine(name)
    U, V, nloc, _ = sref.make_truncating_case(P, 40, NW, seed=3)
    out = {}
    for route in (0, 1):
        eng.ctx.set_option('pod_rotate_valu', route)
        try:
            out[route] = _run(eng, U, V, nloc, 5, 7, modes=5)
        finally:
            eng.ctx.set_option('pod_rotate_valu', 0)
    assert np.array_equal(out[0]['added'], out[1]['added']) and np.array_equal(out[0]['kb'], out[1]['kb'])
    assert np.abs(out[0]['sv'] - out[1]['sv']).max() <= 1e-12 * out[0]['sv'].max()
    for s in range(eng.S):
        n0, k = int(nloc[s]), int(out[0]['added'][s])
        assert sref.span_defect(out[0]['V'][s][:, n0:n0 + k], out[1]['V'][s][:, n0:n0 + k], P[s]) <= 1e-9


# ------------------------------------------------------------------------------------------------------------- 4: bits
def test_repeats_poisoned_work_and_a_poisoned_state_give_the_same_bits():
    d, eng, P = _engine('3x3_n96')
    n, S = eng.t.n, eng.S
    U, V, nloc, _ = sref.make_truncating_case(P, 50, NW, seed=2)
    assert eng.ctx.lib.lrbms_local_pod_stream_state_size(eng.ctx.handle, 8, 17) == S * (2 * n * 25 + 3)      # the header's formulas
    assert eng.ctx.lib.lrbms_local_pod_stream_work_size(eng.ctx.handle, 8, 17, NW) == S * (
        2 * n * 17 + 2 * n * 8 + NW * 17 + 2 * 25 * 25 + 26 * 26 + 25 + 25 * 8 + 4)
    first = _run(eng, U, V, nloc, 8, 17, 5, halo=1)
    again = _run(eng, U, V, nloc, 8, 17, 5, halo=1, poison=True)
    for k in ('V', 'sv', 'added', 'nloc', 'info', 'lost', 'kb'):
        assert np.array_equal(first[k], again[k]), k
    assert first['added'].max() == 5 and np.array_equal(first['V'][S], first['V_in'][S])
    # the same stream object, begun again
    stream = again['stream']
    stream.work.fill_(float('nan'))
    stream.begin()
    v = _views(stream)
    assert not v['X'].any() and not v['PX'].any() and not v['kb'].any() and not v['lost'].any() and not v['norm0sq'].any()


def test_subdomains_are_independent():
    d, eng, P = _engine('3x3_n96')
    S = eng.S
    nloc = np.full(S, 2)
    U, V, _, _ = sref.make_truncating_case(P, 40, NW, seed=4, nloc=nloc)
    base = _run(eng, U, V, nloc, 8, 17, 4)
    # the dense products differ from subdomain to subdomain, so "permuting subdomains" is changing one and watching the others
    U2 = U.copy()
    U2[4] = U[4][:, np.random.default_rng(0).permutation(40)]
    perm = _run(eng, U2, V, nloc, 8, 17, 4)
    others = [s for s in range(S) if s != 4]
    for k in ('V', 'sv', 'added', 'lost'):
        assert np.array_equal(base[k][others], perm[k][others]), k
    assert not np.array_equal(base['V'][4], perm['V'][4])


# ------------------------------------------------------------------------------------------------------------- 5: degenerate pushes
def test_degenerate_pushes_leave_kb_where_the_restatement_says():
    import torch
    from pylrbms_amd.reductor import ExtensionError, LRBMSReductor
    d, eng, P = _engine('2x2_n24')
    S, n = eng.S, eng.t.n
    rng = np.random.default_rng(6)
    V = np.zeros((S, n, NW))
    nloc = np.array([3, 0, 4, NW])
    for s in range(S):
        V[s][:, :nloc[s]] = sref.p_orthonormal(rng.standard_normal((n, int(nloc[s]))), P[s]) if nloc[s] else 0.0
    inspan = np.stack([V[s][:, :nloc[s]] @ rng.standard_normal((int(nloc[s]), 5)) if nloc[s] else np.zeros((n, 5)) for s in range(S)])
    fresh = rng.standard_normal((S, n, 5))
    U = np.concatenate([fresh, np.zeros((S, n, 5)), inspan, fresh], axis=2)     # a chunk, a zero one, one in span(V), the first again
    out = _run(eng, U, V, nloc, 6, 5, modes=6)
    want = sref.stream_ref(U, V, nloc, P, 6, 5, modes=6)
    assert np.array_equal(out['kb'], want['kb']) and np.array_equal(out['kb'], np.full((4, S), 5))
    assert np.array_equal(out['added'], want['added']) and out['added'].tolist() == [5, 5, 4, 0]
    assert np.abs(out['sv'] - want['sv']).max() <= 1e-9 * want['sv'].max()
    # only such chunks: nothing is added anywhere, the slab is untouched
    only = np.concatenate([np.zeros((S, n, 5)), inspan, inspan], axis=2)
    out = _run(eng, only, V, nloc, 6, 5, modes=6)
    # (a node of rounding noise alone keeps noise columns, its floor is relative to its own lam_1: kb is exact only where the chunks
    # are exact zeros, subdomain 1; the threshold of finish is relative to the undeflated snapshots and drops them all)
    assert not out['kb'][:, 1].any() and not out['added'].any() and np.array_equal(out['V'], V) and np.array_equal(out['nloc'], nloc)
    assert out['sv'].max() <= 1e-12
    red = LRBMSReductor.__new__(LRBMSReductor)
    red.d = types.SimpleNamespace(engine=eng)
    red._V, red._nloc = eng.ctx.from_numpy(V), nloc.astype(np.int64).copy()
    V0 = red._V.clone()
    with pytest.raises(ExtensionError):
        red.extend_basis_hapod([eng.ctx.from_numpy(only[:, :, :5]), eng.ctx.from_numpy(only[:, :, 5:])], keep=6)
    assert torch.equal(red._V, V0) and np.array_equal(red._nloc, nloc) and not getattr(red, '_dirty', set())


# ------------------------------------------------------------------------------------------------------------- 6: refusals
def test_refusals_carry_a_message_and_touch_nothing():
    import torch
    d, eng, P = _engine('2x2_n24')
    ctx, S, n = eng.ctx, eng.S, eng.t.n
    lib, h = ctx.lib, ctx.handle
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    nan = float('nan')
    state = torch.full((S * (2 * n * 128 + 3),), nan, dtype=torch.float64, device=ctx.device)
    work = torch.full((max(int(lib.lrbms_local_pod_stream_work_size(h, 64, 64, 8)), 1),), nan, dtype=torch.float64, device=ctx.device)
    V = ctx.from_numpy(np.random.default_rng(1).standard_normal((S, n, 8)))
    V0 = V.clone()
    U = ctx.zeros(S, n, 64)
    nd = torch.zeros(S, dtype=torch.int32, device=ctx.device)
    sv, lost = ctx.zeros(S, 64), ctx.zeros(S)
    ai = torch.zeros(2, S, dtype=torch.int32, device=ctx.device)
    Pd = p(eng.P_diag)

    def begin(keep, cmax, st=state):
        return lib.lrbms_local_pod_stream_begin(h, keep, cmax, p(st) if st is not None else None, None)

    def push(keep=8, cmax=8, C=4, Nw=8, Pp=Pd, Up=p(U), Vp=p(V), np_=p(nd), sp=p(state), wp=p(work)):
        return lib.lrbms_local_pod_stream_push(h, keep, cmax, C, Nw, Pp, Up, Vp, np_, sp, wp, None)

    def finish(keep=8, cmax=8, Nw=8, modes=2, rtol=1e-6, atol=0.0, ptrs=None):
        ptrs = ptrs or [Pd, p(V), p(nd), p(state), p(sv), p(ai[0]), p(ai[1]), p(lost), p(work)]
        return lib.lrbms_local_pod_stream_finish(h, keep, cmax, Nw, modes, rtol, atol, *ptrs, None)

    def refused(rc, text):
        assert rc == -1 and text in lib.lrbms_last_error(h).decode(), (rc, lib.lrbms_last_error(h))      # LRBMS_E_INVALID

    for keep, cmax, text in ((0, 8, 'keep must be in [1, 64]'), (65, 8, 'keep must be in [1, 64]'), (8, 0, 'cmax must be >= 1'),
                             (64, 65, 'keep + cmax must be <= 128'), (100, 100, 'keep must be in [1, 64]')):
        refused(begin(keep, cmax), text)
        refused(push(keep=keep, cmax=cmax), text)
        refused(finish(keep=keep, cmax=cmax), text)
        assert lib.lrbms_local_pod_stream_state_size(h, keep, cmax) == -1 and lib.lrbms_local_pod_stream_work_size(h, keep, cmax, 8) == -1
    refused(begin(8, 8, None), 'null pointer')
    for C in (0, 9):
        refused(push(C=C), 'C must be in [1, cmax]')
    for Nw in (0, 65):
        refused(push(Nw=Nw), 'Nw must be in [1, 64]')
        refused(finish(Nw=Nw), 'Nw must be in [1, 64]')
        assert lib.lrbms_local_pod_stream_work_size(h, 8, 8, Nw) == -1
    for kw in ({'Pp': None}, {'Up': None}, {'Vp': None}, {'np_': None}, {'sp': None}, {'wp': None}):
        refused(push(**kw), 'null pointer')
    refused(finish(modes=0), 'modes must be >= 1')
    refused(finish(rtol=9e-8), 'rtol < 1e-7')
    refused(finish(atol=-1.0), 'atol must be >= 0')
    full = [Pd, p(V), p(nd), p(state), p(sv), p(ai[0]), p(ai[1]), p(lost), p(work)]
    for i in range(len(full)):
        refused(finish(ptrs=full[:i] + [None] + full[i + 1:]), 'null pointer')
    torch.cuda.synchronize()
    assert bool(torch.isnan(state).all()) and bool(torch.isnan(work).all()) and torch.equal(V, V0) and not nd.any()


# ------------------------------------------------------------------------------------------------------------- 7: end to end
def _reductor(name, empty=False):
    from test_local_pod_gpu import _reductor as make
    return make(name, empty=empty)


def _training_set(name):
    """(mus, slabs of solve_batch(as_snapshots='slabs'), all snapshots [S, n, len(mus) nt] on the host), once per mesh."""
    key = ('training', name)
    if key not in _ref_cache:
        d, eng, P = _engine(name)
        mus = [d.parse_parameter(v) for v in (0.15, 0.3, 0.45, 0.7, 0.95, 1.0)]
        slabs = d.solve_batch(mus, as_snapshots='slabs')
        nt = d.time_stepper.nt
        assert len(mus) * nt > 128 and len(slabs) == nt and all(tuple(u.shape) == (eng.S, eng.t.n, len(mus)) for u in slabs)
        assert all(u.is_contiguous() for u in slabs)
        with pytest.raises(ValueError):
            d.solve_batch(mus, as_snapshots=True)                 # as before: more than 128 vectors
        allcols = np.concatenate([u.cpu().numpy() for u in slabs], axis=2)
        _ref_cache[key] = (mus, slabs, allcols)
    return _ref_cache[key]


def test_hapod_of_a_training_set_is_the_pod_of_all_its_columns():
    """n = 24 <= keep: nothing is truncated on the way, so k modes of 144 columns are THE k POD modes -- no worse than the first k
    of what method='pod' appends for the same columns (optimality), and what they leave is the tail of the spectrum."""
    name, k = '2x2_n24', 4
    d, eng, P = _engine(name)
    mus, slabs, allcols = _training_set(name)
    red = _reductor(name, empty=True)
    sv, added = red.extend_basis(slabs, method='hapod', pod_modes=k)
    assert added.max() <= k and added.tolist() == [k] * eng.S and red.basis_size() == k
    info = red.last_pod_info
    assert info['columns'] == allcols.shape[2] and info['nodes'] == len(slabs) and info['lost'].shape == (eng.S,)
    pod = _reductor(name, empty=True)
    import torch
    pod.extend_basis(torch.cat(list(slabs), dim=2), method='pod', pod_modes=k)      # consecutive calls of 128 columns, k modes each
    assert min(pod.local_sizes()) >= k
    Vh, Vp = red._V.cpu().numpy(), pod._V.cpu().numpy()
    for s in range(eng.S):
        sig, _ = sref.product_svd(allcols[s], P[s])
        e = sref.projection_error2(allcols[s], Vh[s], P[s])
        assert e <= sref.projection_error2(allcols[s], Vp[s][:, :k], P[s]) * (1 + 1e-8), s
        assert abs(e - (sig[k:] ** 2).sum()) <= 1e-8 * (sig ** 2).sum(), s
        assert e <= info['lost'][s] * (1 + 1e-8), s
    assert sref.orthonormality(Vh, red._nloc, P) <= 1e-12


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_end_to_end_reduce_and_solve_on_a_hapod_basis(name):
    d, eng, P = _engine(name)
    mus, slabs, allcols = _training_set(name)
    k = 3
    red = _reductor(name)                                          # order 0: the constant, then at most k vectors
    sv, added = red.extend_basis(slabs, method='hapod', pod_modes=k)
    assert added.max() <= k and added.tolist() == [k] * eng.S and red.local_sizes() == [1 + k] * eng.S
    Vh = red._V.cpu().numpy()
    for s in range(eng.S):
        R = sref.deflate(allcols[s], Vh[s][:, :1], P[s])
        assert sref.projection_error2(R, Vh[s][:, 1:1 + k], P[s]) <= red.last_pod_info['lost'][s] * (1 + 1e-8)
    rd = red.reduce()
    u = rd.solve(mus[2])
    est, parts = rd.estimate(u, mus[2])
    assert np.isfinite(est) and est > 0
    full = d.solve(mus[2]).tensor.cpu().numpy()
    E = red.reconstruct(u).tensor.cpu().numpy() - full
    err = np.sqrt(sum(np.einsum('ij,ij->', E[s], P[s] @ E[s]) for s in range(eng.S)))
    norm = np.sqrt(sum(np.einsum('ij,ij->', full[s], P[s] @ full[s]) for s in range(eng.S)))
    print('local_pod_stream end to end {}: energy error of the reduced trajectory {:.3e} of {:.3e}'.format(name, err, norm))
    assert np.isfinite(err) and err < norm


def test_reduce_touched_after_a_hapod_extension_into_reserved_columns_is_bitwise_the_whole_pass():
    import torch
    name = '3x3_n96'
    d, eng, P = _engine(name)
    mus, slabs, allcols = _training_set(name)
    red = _reductor(name)
    red.extend_basis(d.solve(mus[0]), max_vectors=2)
    width = red.reserve(6)
    rd0 = red.reduce()
    slab = red._V
    masked = []
    for u in slabs:
        u = u.clone()
        u[[1, 2, 3, 5, 6, 7, 8]] = 0.0                            # only subdomains 0 and 4 see snapshots
        masked.append(u)
    sv, added = red.extend_basis(masked, method='hapod', pod_modes=3)
    assert added.tolist() == [3, 0, 0, 0, 3, 0, 0, 0, 0] and red._V is slab and red.basis_size() == width
    rd1 = red.reduce(touched=[])                                  # the reductor knows what changed
    assert red.last_reduce_info['incremental'] and 0 < red.last_reduce_info['subdomains'] < eng.S
    assert rd1.B_sys.data_ptr() == rd0.B_sys.data_ptr()
    inc = [x.clone() for x in (rd1.B_sys, rd1.rhs_red, rd1.E_red, rd1.M_red) + rd1.grams]
    rd2 = red.reduce()
    assert not red.last_reduce_info['incremental']
    for a, b in zip(inc, (rd2.B_sys, rd2.rhs_red, rd2.E_red, rd2.M_red) + rd2.grams):
        assert torch.equal(a, b)
