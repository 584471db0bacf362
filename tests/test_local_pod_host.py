"""Local POD basis extension, the parts that need no GPU: the NumPy reference of tests/local_pod_ref.py pinned against an SVD in
the product, the margins of the inputs the GPU tests share, the Jacobi iteration of the eigen kernel restated in NumPy, and the host
logic of ``extend_basis_pod`` / ``extend_basis(method='pod')`` on a fake context that runs the reference."""
import inspect
import os
import re
import types

import numpy as np
import pytest

import local_pod_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS2 = ('lrbms_local_pod_work_size', 'lrbms_local_pod', 'lrbms_pod_gram', 'lrbms_pod_eigh_work_size', 'lrbms_pod_eigh')
EXPORTS3 = ('lrbms3_local_pod_work_size', 'lrbms3_local_pod')


# ------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize('L', ref.L_VALUES)
@pytest.mark.parametrize('n', [24, 96])
def test_reference_matches_the_svd_in_the_product(n, L):
    S, Nw = 6, 8
    P = ref.spd_products(S, n, seed=n)
    U, V, nloc, _ = ref.make_case(P, L, Nw, seed=n)
    assert ref.threshold_margin(U, V, nloc, P) >= 10.0
    Vn, nloc_new, sv, added = ref.local_pod_ref(U, V, nloc, P, modes=6)
    for s in range(S):
        R = ref.deflate(U[s], V[s], P[s])
        sig, W = ref.product_svd(R, P[s])
        resolved, noise = ref.sigma_error(sv[s], sig)                # (what the two bounds are: local_pod_ref.SIGMA_TOL)
        assert resolved <= ref.SIGMA_TOL and noise <= ref.NOISE
        norm0 = np.sqrt(np.einsum('ij,ij->j', U[s], P[s] @ U[s]).max())
        k = min(int(np.count_nonzero(sig > 1e-6 * norm0)), 6, Nw - int(nloc[s]))
        assert added[s] == k
        assert np.array_equal(Vn[s][:, :nloc[s]], V[s][:, :nloc[s]]) and np.all(Vn[s][:, nloc_new[s]:] == 0.0)
        lead = int(np.count_nonzero(sig[:k] >= 1e-3 * sig[0]))
        assert ref.span_defect(W[:, :lead], Vn[s][:, nloc[s]:nloc_new[s]], P[s]) <= 1e-6
    assert ref.orthonormality(Vn, nloc_new, P) <= 1e-13
    assert (nloc == Nw).any() and added[nloc == Nw].max() == 0 and (added > 0).any()


def test_reference_is_optimal_and_its_error_is_the_tail_of_the_spectrum():
    n, L, k = 60, 20, 5
    P = ref.spd_products(1, n, seed=5)[0]
    rng = np.random.default_rng(2)
    U = np.cumsum(rng.standard_normal((n, L)) * 0.7 ** np.arange(L), axis=1)
    V0 = np.zeros((n, k))
    Vn, sv, added = ref.local_pod_one(U, V0, 0, P, modes=k)
    assert added == k
    gs = ref.p_orthonormal(U[:, :k], P)
    e_pod, e_gs = ref.projection_error2(U, Vn, P), ref.projection_error2(U, gs, P)
    assert e_pod <= e_gs * (1 + 1e-8)
    assert abs(e_pod - (sv[k:] ** 2).sum()) <= 1e-8 * (sv ** 2).sum()


@pytest.mark.parametrize('L', ref.L_VALUES)
def test_jacobi_iteration_of_the_eigen_kernel(L):
    """The kernel's iteration (ordering, exact zeroing, skip threshold, stopping test) restated in NumPy converges well inside
    the sweep cap on clustered, repeated and zero spectra, and keeps a zero row / column exactly zero."""
    for name, (G, lam) in ref.eigen_matrices(L).items():
        got, Z, sweeps, converged = ref.jacobi_eigh(G)
        assert converged and sweeps <= 30, (name, sweeps)
        scale = max(np.abs(G).max(), 1e-300) * L
        assert np.abs(G @ Z.T - Z.T * got).max() <= 8 * ref.EPS * scale, name
        assert np.abs(Z @ Z.T - np.eye(L)).max() <= 8 * ref.EPS * L, name
        assert np.all(np.diff(got) <= 0.0)
        if lam is not None:
            assert np.abs(got - lam).max() <= 8 * ref.EPS * scale, name
        else:
            j = int(np.where(got == 0.0)[0][0])                      # the zero snapshot: an exact zero, its vector a unit vector
            assert np.array_equal(np.abs(Z[j]), np.eye(L)[0])


def test_exports_are_declared_and_bound():
    from pylrbms_amd._build import SOURCES
    from pylrbms_amd._native import SIGNATURES, NativeContext
    from pylrbms_amd._native3d import SIGNATURES3, Native3DContext
    assert 'pod.hip' in SOURCES
    for header, names, table, cls, prefix in (('lrbms_hip.h', EXPORTS2, SIGNATURES, NativeContext, 'lrbms_'),
                                              ('lrbms3d_hip.h', EXPORTS3, SIGNATURES3, Native3DContext, 'lrbms3_')):
        with open(os.path.join(ROOT, 'include', header)) as fh:
            text = fh.read()
        for name in names:
            m = re.search(r'\b(?:int|int64_t) {}\(([^;]*)\);'.format(name), text)
            assert m, '{} is not declared in include/{}'.format(name, header)
            assert name in table and len(table[name][1]) == m.group(1).count(',') + 1, name
            if not name.endswith('_work_size'):
                assert hasattr(cls, name[len(prefix):]), name
    assert 'rtol < 1e-7' in open(os.path.join(ROOT, 'include', 'lrbms_hip.h')).read()


# ------------------------------------------------------------------------------------------------------------- host logic
class FakeContext:
    """``local_pod`` by the NumPy reference on CPU tensors; records every call."""

    def __init__(self, P):
        import torch
        self.torch, self.P, self.calls = torch, P, []

    def zeros(self, *shape):
        return self.torch.zeros(*shape, dtype=self.torch.float64)

    def local_pod(self, P_diag, U, V, nloc, modes, rtol=1e-6, atol=0.0):
        torch = self.torch
        assert P_diag is self.P and nloc.dtype == torch.int32 and U.is_contiguous() and V.is_contiguous()
        S = U.shape[0]
        self.calls.append(dict(U=U.numpy().copy(), width=int(V.shape[2]), nloc=nloc.numpy().copy(), modes=int(modes), rtol=rtol))
        Vn, nloc_new, sv, added = ref.local_pod_ref(U.numpy(), V.numpy(), nloc.numpy(), self.P, modes, rtol, atol)
        V[:S] = torch.from_numpy(Vn[:S])
        nloc += torch.from_numpy(added.astype(np.int32))
        return torch.from_numpy(sv), torch.stack([torch.from_numpy(added.astype(np.int32)), torch.zeros(S, dtype=torch.int32)])


def _fake_reductor(cls, S=3, n=40, width=1, local=None, seed=0):
    """An instance of ``cls`` around a fake engine: order-0-like bases of ``width`` P-orthonormal columns."""
    import torch
    P = ref.spd_products(S, n, seed=seed)
    red = cls.__new__(cls)
    eng = types.SimpleNamespace(S=S, S_ext=S, t=types.SimpleNamespace(n=n), ctx=FakeContext(P), P_diag=P, ops={'P_diag': P},
                                local=list(local if local is not None else range(S)))
    red.d = types.SimpleNamespace(engine=eng, Q=1)
    red.euclidean = False
    red._torch = torch
    rng = np.random.default_rng(seed)
    V = np.stack([ref.p_orthonormal(rng.standard_normal((n, width)), P[s]) for s in range(S)]) if width else np.zeros((S, n, 0))
    red._V = torch.from_numpy(V).contiguous()
    red._nloc = np.full(S, width, dtype=np.int64)
    return red, P


def _snapshots(S, n, L, seed=1, decay=0.6):
    import torch
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.standard_normal((S, n, L)) * decay ** np.arange(L))


def _classes():
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D
    from pylrbms_amd.reductor import LRBMSReductor, ParabolicLRBMSReductor
    return LRBMSReductor, ParabolicLRBMSReductor, LRBMSReductor3D, ParabolicLRBMSReductor3D


def test_a_list_is_stacked_along_the_columns_and_the_result_is_the_reference():
    from pylrbms_amd.reductor import LRBMSReductor
    red, P = _fake_reductor(LRBMSReductor, local=[4, 7, 9])
    V0 = red._V.numpy().copy()
    A, B = _snapshots(3, 40, 5, seed=1), _snapshots(3, 40, 3, seed=2)
    wrapped = types.SimpleNamespace(tensor=B)                          # a block array: its slab is .tensor
    sv, added = red.extend_basis_pod([A, wrapped], modes=4)
    call, = red.d.engine.ctx.calls
    assert np.array_equal(call['U'], np.concatenate([A.numpy(), B.numpy()], axis=2)) and call['modes'] == 4
    assert call['width'] == 6                                          # 1 + 4 = 5 vectors -> the even width 6
    Vn, nloc_new, sv_ref, added_ref = ref.local_pod_ref(call['U'], np.pad(V0, ((0, 0), (0, 0), (0, 5))), [1, 1, 1], P, 4)
    assert np.array_equal(added, added_ref) and np.array_equal(added, [4, 4, 4]) and np.array_equal(sv, sv_ref)
    assert red.basis_size() == 6 and red.local_sizes() == [5, 5, 5]
    assert np.array_equal(red._V.numpy(), Vn) and np.all(red._V.numpy()[:, :, 5] == 0.0)
    assert red._dirty == {4, 7, 9}                                     # global ids, as the Gram-Schmidt path records them
    assert ref.orthonormality(red._V.numpy(), red._nloc, P) <= 1e-13


def test_more_than_128_columns_run_as_consecutive_calls_on_the_grown_basis():
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D
    red, P = _fake_reductor(LRBMSReductor3D, S=2, n=50, width=0)
    U = _snapshots(2, 50, 300, seed=3, decay=0.97)
    sv, added = red.extend_basis_pod(U, modes=3)
    calls = red.d.engine.ctx.calls
    assert [c['U'].shape[2] for c in calls] == [128, 128, 44]
    assert np.array_equal(np.concatenate([c['U'] for c in calls], axis=2), U.numpy())
    assert [c['nloc'].tolist() for c in calls] == [[0, 0], [3, 3], [6, 6]] and [c['width'] for c in calls] == [3, 6, 9]
    assert sv.shape == (2, 300) and np.array_equal(added, [9, 9]) and red.basis_size() == 9      # (3D: no even rule)
    assert red._dirty == {0, 1}                                        # local indices on the 3D path
    assert ref.orthonormality(red._V.numpy(), red._nloc, P) <= 1e-13


def test_padding_is_cut_back_and_reserved_columns_are_filled_in_place():
    from pylrbms_amd.reductor import LRBMSReductor
    red, P = _fake_reductor(LRBMSReductor, S=2, n=40, width=1)
    U = _snapshots(2, 40, 6, seed=4)
    U[1] = red._V[1] @ _snapshots(1, 1, 6, seed=5)[0]                   # subdomain 1: wholly in the span of its basis
    sv, added = red.extend_basis_pod(U)                                # modes=None: as many as pass the threshold
    assert red.d.engine.ctx.calls[0]['width'] == 8 and red.d.engine.ctx.calls[0]['modes'] == 6
    assert np.array_equal(added, [6, 0]) and red.basis_size() == 8 and red._dirty == {0}
    # reserved columns: the slab keeps its width (what reduce(touched=) needs)
    red, P = _fake_reductor(LRBMSReductor, S=2, n=40, width=1)
    assert red.reserve(10) == 10
    slab = red._V
    red.extend_basis_pod(_snapshots(2, 40, 6, seed=6), modes=3)
    assert red._V is slab and red.basis_size() == 10 and red.local_sizes() == [4, 4]
    # the width never passes 64
    red, P = _fake_reductor(LRBMSReductor, S=1, n=80, width=1)
    sv, added = red.extend_basis_pod(_snapshots(1, 80, 100, seed=7, decay=0.99))
    assert red.d.engine.ctx.calls[0]['width'] == 64 and added[0] == 63 and red.basis_size() == 64


def test_refusals():
    from pylrbms_amd.reductor import ExtensionError, LRBMSReductor
    red, P = _fake_reductor(LRBMSReductor)
    U = _snapshots(3, 40, 4)
    with pytest.raises(ValueError, match='1e-7'):
        red.extend_basis_pod(U, rtol=1e-8)
    with pytest.raises(ValueError):
        red.extend_basis_pod(U, modes=0)
    with pytest.raises(ValueError):
        red.extend_basis_pod(U, atol=-1.0)
    with pytest.raises(ValueError):
        red.extend_basis_pod(U[:, :30])
    with pytest.raises(ValueError):
        red.extend_basis_pod([])
    with pytest.raises(ValueError, match='gram_schmidt'):
        red.extend_basis(types.SimpleNamespace(tensor=U), method='svd')
    assert red.d.engine.ctx.calls == []
    V0 = red._V.clone()
    inside = red._V @ _snapshots(3, 1, 4)                               # in the span everywhere, and a zero column
    inside[:, :, 2] = 0.0
    with pytest.raises(ExtensionError):
        red.extend_basis_pod(inside)
    assert np.array_equal(red._V.numpy(), V0.numpy()) and red.local_sizes() == [1, 1, 1] and not getattr(red, '_dirty', set())


def test_method_dispatch_on_the_four_reductors():
    from pylrbms_amd.reductor import ExtensionError
    for cls in _classes():
        params = inspect.signature(cls.extend_basis).parameters
        assert params['method'].default == 'gram_schmidt' and params['pod_modes'].default is None, cls
        assert hasattr(cls, 'extend_basis_pod')
        red, P = _fake_reductor(cls, S=2, n=40, width=1)
        U = _snapshots(2, 40, 12, seed=8)
        out = red.extend_basis(U, method='pod', pod_modes=3)
        assert np.array_equal(out[1], [3, 3]) and red.local_sizes() == [4, 4], cls
        if 'max_vectors' in params:                                    # the parabolic reductors: no basis grows past max_vectors
            red.extend_basis(U, max_vectors=6, method='pod')
            assert red.local_sizes() == [6, 6] and red.d.engine.ctx.calls[-1]['modes'] == 2
            with pytest.raises(ExtensionError):
                red.extend_basis(U, max_vectors=6, method='pod', pod_modes=4)
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D
    red, P = _fake_reductor(LRBMSReductor3D)
    red.euclidean = True
    with pytest.raises(NotImplementedError):
        red.extend_basis(_snapshots(3, 40, 2), method='pod')


def test_halo_rows_of_a_slab_are_left_alone():
    import torch
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D
    red, P = _fake_reductor(LRBMSReductor3D, S=2, n=40, width=4)
    halo = torch.from_numpy(np.random.default_rng(9).standard_normal((1, 40, 4)))
    red._V = torch.cat([red._V, halo]).contiguous()                    # [S_ext = 3, n, 4]: a halo row behind the local ones
    red._nloc = np.array([2, 4, 4])
    red._V[0, :, 2:] = 0.0
    sv, added = red.extend_basis_pod(_snapshots(2, 40, 5, seed=10), modes=2)
    assert np.array_equal(added, [2, 2]) and red._nloc.tolist() == [4, 6, 4] and red.basis_size() == 6
    assert np.array_equal(red._V[2, :, :4].numpy(), halo[0].numpy()) and np.all(red._V[2, :, 4:].numpy() == 0.0)
    assert red.d.engine.ctx.calls[0]['nloc'].tolist() == [2, 4]
