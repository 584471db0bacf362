"""Streamed local POD (incremental HAPOD), the parts that need no GPU: the NumPy restatement of tests/local_pod_stream_ref.py pinned
against an SVD in the product of ALL pushed columns, the margins of the inputs the GPU tests share (conditions on the inputs, not
measurements: if a seed breaks one, the input changes, not the margin), the gap condition and the sensitivity behind the device
tolerance of the truncating cases, the host logic of ``extend_basis_hapod`` / ``extend_basis(method='hapod')`` on a fake context
that runs the restatement, and ``solve_batch(as_snapshots='slabs')`` on the fakes of the fom-euler-batch host tests.

Measured on the CPU with these inputs: sigma against the SVD <= 1.7e-14 sigma_1, node margin >= 11.0, final margin >= 66,
gap >= 3.3e-3, and a Gram perturbation of 1e-15 max|G| moves sv by <= 1.2e-14 sigma_1 and lost by <= 1.2e-13 sigma_1^2."""
import inspect
import os
import re
import types

import numpy as np
import pytest

import local_pod_stream_ref as sref
from test_local_pod_host import FakeContext, _classes, _fake_reductor, _snapshots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NW, S_HOST = 8, 6
EXPORTS = ('local_pod_stream_state_size', 'local_pod_stream_work_size', 'local_pod_stream_begin', 'local_pod_stream_push',
           'local_pod_stream_finish')
_cache = {}


def _exact(n, L):
    """The exact inputs for (n, L_total) and their SVD data, shared by the chunkings."""
    if (n, L) not in _cache:
        P = sref.spd_products(S_HOST, n, seed=n)
        U, V, nloc, _ = sref.make_case(P, L, NW, seed=n)
        svd = []
        for s in range(S_HOST):
            R = sref.deflate(U[s], V[s], P[s])
            sig, W = sref.product_svd(R, P[s])
            norm0 = np.sqrt(np.einsum('ij,ij->j', U[s], P[s] @ U[s]).max())
            svd.append((R, sig, W, min(int(np.count_nonzero(sig > 1e-6 * norm0)), 6, NW - int(nloc[s]))))
        _cache[(n, L)] = (P, U, V, nloc, svd, {})
    return _cache[(n, L)]


# ------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('chunking', sref.EXACT_CHUNKINGS)
@pytest.mark.parametrize('n', [24, 60, 96])
def test_exact_inputs_give_the_pod_of_all_columns_whatever_the_chunking(n, chunking):
    L, cmax, keep = chunking
    P, U, V, nloc, svd, spans = _exact(n, L)
    out = sref.stream_ref(U, V, nloc, P, keep, cmax, modes=6)
    assert sref.node_margin(out['streams']) >= 10.0           # no node eigenvalue within a factor 10 of the floor
    assert sref.final_margin(U, V, nloc, P) >= 10.0           # no final sigma within a factor 10 of the threshold
    assert out['kb'].max() <= keep and (nloc == NW).any()
    for s in range(S_HOST):
        R, sig, W, k = svd[s]
        resolved, noise = sref.sigma_error(out['sv'][s], sig)
        assert resolved <= sref.SIGMA_TOL and noise <= sref.NOISE
        assert out['added'][s] == k
        n0 = int(nloc[s])
        new = out['V'][s][:, n0:n0 + k]
        e = sref.projection_error2(R, new, P[s])
        assert abs(e - (sig[k:] ** 2).sum()) <= 1e-8 * (sig ** 2).sum()
        assert e <= out['lost'][s] * (1 + 1e-8)
        assert np.array_equal(out['V'][s][:, :n0], V[s][:, :n0]) and np.all(out['V'][s][:, n0 + k:] == 0.0)
        # chunkings of the same columns span the same space: against the first chunking seen, 100 x its defect against the SVD
        lead = int(np.count_nonzero(sig[:k] >= 1e-3 * sig[0]))
        defect = sref.span_defect(W[:, :lead], new, P[s])
        first = spans.setdefault(s, (new, defect, chunking))
        if first[2] != chunking:
            other = sref.span_defect(first[0][:, :lead], new, P[s])
            assert other <= 100 * max(first[1], defect), (s, other, first[1], defect)
    assert sref.orthonormality(out['V'], out['nloc'], P) <= 1e-13
    assert out['added'][nloc == NW].max() == 0 and (out['added'] > 0).any()


def test_exact_inputs_were_compared_across_chunkings():
    """The span comparison above needs at least two chunkings per column set: the three chunkings of 200 columns."""
    assert sum(1 for c in sref.EXACT_CHUNKINGS if c[0] == 200) == 3


@pytest.mark.parametrize('case', sref.TRUNCATING_CASES)
def test_truncating_inputs_meet_the_bound_the_gap_condition_and_the_sensitivity(case):
    n, keep, L, cmax = case
    P = sref.spd_products(S_HOST, n, seed=n)
    U, V, nloc, _ = sref.make_truncating_case(P, L, NW, seed=sref.TRUNCATING_SEED)
    out = sref.stream_ref(U, V, nloc, P, keep, cmax, modes=keep)
    pushed = np.minimum(np.cumsum([c1 - c0 for c0, c1 in sref.chunks(L, cmax)]), keep)
    assert np.array_equal(out['kb'], np.repeat(pushed[:, None], S_HOST, axis=1))      # every node is full as soon as it can be
    assert sref.node_gap(out['streams'], keep) >= sref.GAP_MIN
    for s in range(S_HOST):
        R = sref.deflate(U[s], V[s], P[s])
        sig, _ = sref.product_svd(R, P[s])
        n0, k = int(nloc[s]), int(out['added'][s])
        e = sref.projection_error2(R, out['V'][s][:, n0:n0 + k], P[s])
        assert e <= out['lost'][s] * (1 + 1e-8)
        assert e >= (sig[k:] ** 2).sum() * (1 - 1e-12)
    assert out['added'].max() == keep
    # a Gram perturbation of 1e-15: three orders inside the device tolerance (1e-9 sigma_1, 1e-9 sigma_1^2) of the GPU tests
    noisy = sref.stream_ref(U, V, nloc, P, keep, cmax, modes=keep, noise=(np.random.default_rng(0), 1e-15))
    s1 = out['sv'].max(axis=1)
    assert np.array_equal(noisy['kb'], out['kb']) and np.array_equal(noisy['added'], out['added'])
    assert (np.abs(noisy['sv'] - out['sv']).max(axis=1) / s1).max() <= 1e-12
    assert (np.abs(noisy['lost'] - out['lost']) / s1 ** 2).max() <= 1e-12


def test_begin_resets_and_finish_leaves_the_state():
    P = sref.spd_products(1, 24, seed=1)
    U, V, nloc, _ = sref.make_truncating_case(P, 20, NW, seed=1, nloc=[2])
    st = sref.StreamOne(V[0], 2, P[0], 5, 7)
    for c0, c1 in sref.chunks(20, 7):
        st.push(U[0][:, c0:c1])
    first = st.finish(4)
    again = st.finish(4)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    st.begin()
    assert st.kb == 0 and st.lost == 0.0 and st.norm0sq == 0.0 and not st.X.any() and not st.PX.any()
    for c0, c1 in sref.chunks(20, 7):
        st.push(U[0][:, c0:c1])
    assert all(np.array_equal(a, b) for a, b in zip(first, st.finish(4)))


def test_exports_are_declared_and_bound():
    from pylrbms_amd._native import SIGNATURES, ContextBase, LocalPodStream
    from pylrbms_amd._native3d import SIGNATURES3
    for header, table, prefix in (('lrbms_hip.h', SIGNATURES, 'lrbms_'), ('lrbms3d_hip.h', SIGNATURES3, 'lrbms3_')):
        with open(os.path.join(ROOT, 'include', header)) as fh:
            text = fh.read()
        for name in EXPORTS:
            m = re.search(r'\b(?:int|int64_t) {}\(([^;]*)\);'.format(prefix + name), text)
            assert m, '{} is not declared in include/{}'.format(prefix + name, header)
            assert prefix + name in table and len(table[prefix + name][1]) == m.group(1).count(',') + 1, name
    assert hasattr(ContextBase, 'local_pod_stream') and all(hasattr(LocalPodStream, k) for k in ('begin', 'push', 'finish'))
    text = open(os.path.join(ROOT, 'include', 'lrbms_hip.h')).read()
    assert 'S (2 n Lx + 3)' in text and '2 n M1 + 2 n keep' in text          # the formulas of the two sizes


# ------------------------------------------------------------------------------------------------------------- host logic
class FakeStreamContext(FakeContext):
    """``FakeContext`` plus ``local_pod_stream`` by the restatement; records every stream."""

    def __init__(self, P):
        super().__init__(P)
        self.streams = []

    def local_pod_stream(self, P_diag, V, nloc, keep=64, cmax=64):
        assert P_diag is self.P and nloc.dtype == self.torch.int32 and V.is_contiguous() and keep + cmax <= 128
        self.streams.append(sref.FakeStream(self, self.P, V, nloc, keep, cmax))
        return self.streams[-1]


def _reductor(cls, **kw):
    red, P = _fake_reductor(cls, **kw)
    red.d.engine.ctx = FakeStreamContext(P)
    return red, P


def test_a_list_is_pushed_item_by_item_and_wide_items_are_split():
    import torch
    from pylrbms_amd.reductor import LRBMSReductor
    red, P = _reductor(LRBMSReductor, local=[4, 7, 9])
    V0 = red._V.numpy().copy()
    A, B, C = _snapshots(3, 40, 5, seed=1), _snapshots(3, 40, 3, seed=2), _snapshots(3, 40, 150, seed=3, decay=0.97)
    wrapped = types.SimpleNamespace(tensor=B)                          # a block array: its slab is .tensor
    sv, added = red.extend_basis_hapod(iter([A, [wrapped], C]), modes=4)
    stream, = red.d.engine.ctx.streams
    assert (stream.keep, stream.cmax) == (64, 64)
    assert [u.shape[2] for u in stream.pushed] == [5, 3, 64, 64, 22]   # never concatenated; the wide item split at cmax
    assert np.array_equal(np.concatenate(stream.pushed, axis=2), np.concatenate([A.numpy(), B.numpy(), C.numpy()], axis=2))
    assert stream.finishes == [dict(modes=4, rtol=1e-6, atol=0.0)]     # exactly one finish
    assert stream.width == 6                                           # 1 + 4 = 5 vectors -> the even width 6
    allcols = np.concatenate(stream.pushed, axis=2)
    want = sref.stream_ref(allcols, np.pad(V0, ((0, 0), (0, 0), (0, 5))), [1, 1, 1], P, 64, 64, 4)      # (pieces of 64: other nodes)
    assert np.array_equal(added, want['added']) and np.array_equal(added, [4, 4, 4]) and sv.shape == (3, 64)
    assert np.abs(sv - want['sv']).max() <= 1e-12 * sv.max()
    assert red.basis_size() == 6 and red.local_sizes() == [5, 5, 5] and np.all(red._V.numpy()[:, :, 5] == 0.0)
    assert red._dirty == {4, 7, 9}
    info = red.last_pod_info
    assert info['columns'] == 158 and info['nodes'] == 5 and isinstance(info['lost'], np.ndarray) and info['lost'].shape == (3,)
    assert sref.orthonormality(red._V.numpy(), red._nloc, P) <= 1e-13
    # keep = 32: pieces of 96 columns; its nodes truncate (39 directions), the bound holds all the same
    red2, _ = _reductor(LRBMSReductor, local=[4, 7, 9])
    sv2, added2 = red2.extend_basis_hapod(torch.from_numpy(allcols), modes=4, keep=32)
    stream2, = red2.d.engine.ctx.streams
    assert stream2.cmax == 96 and [u.shape[2] for u in stream2.pushed] == [96, 62] and sv2.shape == (3, 32)
    for s in range(3):
        R = sref.deflate(allcols[s], V0[s], P[s])
        assert sref.projection_error2(R, red2._V.numpy()[s][:, 1:5], P[s]) <= red2.last_pod_info['lost'][s] * (1 + 1e-8)


def test_300_columns_with_three_modes_add_exactly_three():
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D
    red, P = _reductor(LRBMSReductor3D, S=2, n=50, width=0)
    U = _snapshots(2, 50, 300, seed=3, decay=0.97)                     # the inputs of the consecutive-calls test: 'pod' adds 9
    sv, added = red.extend_basis(U, method='hapod', pod_modes=3)
    assert np.array_equal(added, [3, 3]) and red.basis_size() == 3 and red._dirty == {0, 1}
    stream, = red.d.engine.ctx.streams
    assert [u.shape[2] for u in stream.pushed] == [64, 64, 64, 64, 44] and stream.width == 3
    pod, _ = _reductor(LRBMSReductor3D, S=2, n=50, width=0)
    assert np.array_equal(pod.extend_basis(U, method='pod', pod_modes=3)[1], [9, 9])
    # ... and they are the POD modes of all 300 columns (n = 50 <= keep: nothing is truncated on the way)
    for s in range(2):
        sig, W = sref.product_svd(U[s].numpy(), P[s])
        e = sref.projection_error2(U[s].numpy(), red._V.numpy()[s], P[s])
        assert abs(e - (sig[3:] ** 2).sum()) <= 1e-8 * (sig ** 2).sum()
        assert e <= red.last_pod_info['lost'][s] * (1 + 1e-8)


def test_padding_is_cut_back_and_reserved_columns_are_filled_in_place():
    from pylrbms_amd.reductor import LRBMSReductor
    red, P = _reductor(LRBMSReductor, S=2, n=40, width=1)
    U = _snapshots(2, 40, 6, seed=4)
    U[1] = red._V[1] @ _snapshots(1, 1, 6, seed=5)[0]                   # subdomain 1: wholly in the span of its basis
    sv, added = red.extend_basis_hapod(U)                              # modes=None: as many as pass the threshold and fit
    stream = red.d.engine.ctx.streams[0]
    assert stream.width == 64 and stream.finishes[0]['modes'] == 64
    assert np.array_equal(added, [6, 0]) and red.basis_size() == 8 and red._dirty == {0}
    red, P = _reductor(LRBMSReductor, S=2, n=40, width=1)
    assert red.reserve(10) == 10
    slab = red._V
    red.extend_basis_hapod([_snapshots(2, 40, 6, seed=6)], modes=3)
    assert red._V is slab and red.basis_size() == 10 and red.local_sizes() == [4, 4]


def test_refusals_and_an_extension_error_leave_the_slab_untouched():
    import torch
    from pylrbms_amd.reductor import ExtensionError, LRBMSReductor
    red, P = _reductor(LRBMSReductor)
    U = _snapshots(3, 40, 4)
    with pytest.raises(ValueError, match='1e-7'):
        red.extend_basis_hapod(U, rtol=1e-8)
    with pytest.raises(ValueError):
        red.extend_basis_hapod(U, modes=0)
    with pytest.raises(ValueError):
        red.extend_basis_hapod(U, atol=-1.0)
    with pytest.raises(ValueError):
        red.extend_basis_hapod(U, keep=65)
    with pytest.raises(ValueError):
        red.extend_basis_hapod(U, keep=0)
    with pytest.raises(ValueError):
        red.extend_basis_hapod([])
    with pytest.raises(ValueError):
        red.extend_basis_hapod(iter([]))
    assert red.d.engine.ctx.streams == []
    V0 = red._V.clone()
    with pytest.raises(ValueError):
        red.extend_basis_hapod([U, U[:, :30]])                          # a malformed item after a good one
    assert torch.equal(red._V, V0) and red.local_sizes() == [1, 1, 1]
    with pytest.raises(ValueError, match='gram_schmidt'):
        red.extend_basis(types.SimpleNamespace(tensor=U), method='svd')
    inside = red._V @ _snapshots(3, 1, 4)                               # in the span everywhere, a zero column, a duplicate
    inside[:, :, 2] = 0.0
    with pytest.raises(ExtensionError):
        red.extend_basis_hapod([inside, inside, torch.zeros(3, 40, 2, dtype=torch.float64)])
    assert np.array_equal(red._V.numpy(), V0.numpy()) and red.local_sizes() == [1, 1, 1] and not getattr(red, '_dirty', set())
    assert red.d.engine.ctx.streams[-1].finishes and red.last_pod_info['columns'] == 10


def test_method_dispatch_on_the_four_reductors():
    from pylrbms_amd.reductor import ExtensionError
    for cls in _classes():
        params = inspect.signature(cls.extend_basis).parameters
        assert params['method'].default == 'gram_schmidt' and params['pod_modes'].default is None, cls
        assert hasattr(cls, 'extend_basis_hapod')
        red, P = _reductor(cls, S=2, n=40, width=1)
        U = _snapshots(2, 40, 12, seed=8)
        out = red.extend_basis([U[:, :, :5], U[:, :, 5:]], method='hapod', pod_modes=3)
        assert np.array_equal(out[1], [3, 3]) and red.local_sizes() == [4, 4], cls
        assert red.d.engine.ctx.calls == []                            # not the single-call POD
        if 'max_vectors' in params:                                    # the parabolic reductors: no basis grows past max_vectors
            red.extend_basis(U, max_vectors=6, method='hapod')
            assert red.local_sizes() == [6, 6] and red.d.engine.ctx.streams[-1].finishes[-1]['modes'] == 2
            with pytest.raises(ExtensionError):
                red.extend_basis(U, max_vectors=6, method='hapod', pod_modes=4)
        red.extend_basis(U, method='pod', pod_modes=1)                 # 'pod' is what it was
        assert len(red.d.engine.ctx.calls) == 1
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D
    red, P = _reductor(LRBMSReductor3D)
    red.euclidean = True
    with pytest.raises(NotImplementedError):
        red.extend_basis(_snapshots(3, 40, 2), method='hapod')


def test_halo_rows_of_a_slab_are_left_alone():
    import torch
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D
    red, P = _reductor(LRBMSReductor3D, S=2, n=40, width=4)
    halo = torch.from_numpy(np.random.default_rng(9).standard_normal((1, 40, 4)))
    red._V = torch.cat([red._V, halo]).contiguous()
    red._nloc = np.array([2, 4, 4])
    red._V[0, :, 2:] = 0.0
    sv, added = red.extend_basis_hapod(_snapshots(2, 40, 5, seed=10), modes=2)
    assert np.array_equal(added, [2, 2]) and red._nloc.tolist() == [4, 6, 4] and red.basis_size() == 6
    assert np.array_equal(red._V[2, :, :4].numpy(), halo[0].numpy()) and np.all(red._V[2, :, 4:].numpy() == 0.0)


# ------------------------------------------------------------------------------------------------------------- solve_batch
def test_solve_batch_slabs_are_views_of_the_panels_in_order_2d():
    from test_fom_euler_batch_host import _fake_discretization
    nt = 3
    d = _fake_discretization(False, nt)
    mus = [float(v) for v in np.linspace(0.1, 1.0, 70)]                 # 70 x 3 = 210 vectors: more than 128
    slabs = d.solve_batch(mus, as_snapshots='slabs')
    assert isinstance(slabs, list) and [tuple(u.shape) for u in slabs] == [(3, 12, 64)] * nt + [(3, 12, 6)] * nt
    assert all(u.is_contiguous() for u in slabs)
    for i, u in enumerate(slabs):                                      # step k = 1 .. nt of every call, the columns in order
        k, m0 = i % nt + 1, 64 * (i // nt)
        assert np.array_equal(u[1, 5].numpy(), 100.0 * np.array(mus[m0:m0 + 64]) + k)
    panel = d.engine.ctx.panel                                         # (the last call's)
    assert slabs[nt].data_ptr() == panel[1].data_ptr() and slabs[-1].data_ptr() == panel[nt].data_ptr()
    panel[2, 1, 3, 4] = -7.0
    assert float(slabs[nt + 1][1, 3, 4]) == -7.0
    assert d.last_solve_info == {'iterations': 30, 'relative_residual': 2e-11}
    with pytest.raises(ValueError):
        d.solve_batch(mus, as_snapshots=True)                          # as before: at most 128 vectors
    assert len(d.solve_batch(mus)) == 70 and len(d.solve_batch(mus, as_snapshots=False)) == 70


def test_solve_batch_slabs_are_views_of_the_panels_in_order_3d():
    from test_fom_euler_batch3d_host import _fake_discretization
    nt = 3
    d = _fake_discretization(False, nt)
    mus = [float(v) for v in np.linspace(0.1, 1.0, 70)]
    slabs, info = d.solve_batch(mus, as_snapshots='slabs', return_info=True)
    assert isinstance(slabs, list) and [tuple(u.shape) for u in slabs] == [(3, 20, 64)] * nt + [(3, 20, 6)] * nt
    assert all(u.is_contiguous() for u in slabs) and info == (30, 2e-11)
    for i, u in enumerate(slabs):
        k, m0 = i % nt + 1, 64 * (i // nt)
        assert np.array_equal(u[1, 5].numpy(), 100.0 * np.array(mus[m0:m0 + 64]) + k)
    panel = d.engine.ctx.panel
    assert slabs[nt].data_ptr() == panel[1].data_ptr() and slabs[-1].data_ptr() == panel[nt].data_ptr()
    with pytest.raises(ValueError):
        d.solve_batch(mus, as_snapshots=True)
    assert len(d.solve_batch(mus)) == 70
