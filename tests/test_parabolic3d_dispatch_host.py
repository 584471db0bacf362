"""What tests/test_parabolic3d_dispatch_gpu.py relies on, shown without a GPU: the restatements of tests/parabolic3d_ref.py agree
with the oracle on a small problem; each of their wrong ("mutant") variants is more than 1e-6 away from the right one at the cells
it applies to, so a kernel with that fault could not pass there; and the cells reach every branch of the kernels' dispatch, whose
arithmetic (T = (N + 15) / 16; Lc, G = 256 / Lc; the limits of the time residual) is restated from the source."""
import re

import numpy as np
import pytest

import common3d as c3
import parabolic3d_ref as ref
from test_parabolic3d_dispatch_gpu import (A_CELLS, B_CELLS, C_CELLS, C_PROBLEM, C_RAGGED, D_CELLS, D_PROBLEM, ZERO_TILE_CELL, bases_of,
                                           oracle, synthetic_operators, vectors_of)


def _miss(a, b):
    """Largest relative distance of a block (or column set) of a from b."""
    return c3.rel(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))


# ------------------------------------------------------------------------------------------- the references and the oracle
def test_the_restatements_agree_with_the_oracle():
    p, o = oracle('aniso_2x2x1')
    mu, T, nt, N = p['mu'], 0.2, 3, p['N']
    V = c3.make_bases3d(o.S, o.n, N, seed=5)
    red = ref.ParabolicReduced3D(o, [V[ii] for ii in range(o.S)], T, nt)
    # A: the projected mass
    M_red = ref.project_mass(o, V).astype(np.float64)
    for s in range(o.S):
        assert _miss(M_red[s], red.M_blocks[s]) < 1e-13
    # B: the full-order time residual, summed over the subdomains
    full = ref.Parabolic3D(o, T, nt)
    dU = np.random.default_rng(4).standard_normal((3, o.S, o.n))
    Y = (o.system_matrix(mu) @ dU.reshape(3, -1).T).reshape(o.S, o.n, 3)
    assert _miss(ref.mass_inverse_norm2(o, Y).sum(axis=0), full.time_residual2(dU, mu)) < 1e-12
    # C: the reduced time residual on the 7-slot layout of the oracle's projected operators
    rd = c3.reduce_with_oracle(p, o, V)
    B = np.stack([c3.oracle_dense_blocks(p, o, rd, s)['B_sys'] for s in range(o.S)], axis=1)            # [Q, S, 7, N, N]
    nbr = np.asarray(p['grid'].neighbor_slots).reshape(o.S, 7)
    th = c3.theta_of(p, mu)
    du = np.random.default_rng(1).standard_normal((3, o.S, N))
    A, M, b = red.matrices(mu)
    want = np.array([np.linalg.solve(M, A @ v) @ (A @ v) for v in du.reshape(3, -1)])
    assert _miss(ref.reduced_time_residual(B, M_red, nbr, th, du).sum(axis=1), want) < 1e-11
    # D: the reduced stepping
    A7 = np.zeros_like(A)
    y = ref.reduced_operator_rows(B, nbr, th, np.eye(o.S * N).reshape(o.S * N, o.S, N))
    A7[:] = y.reshape(o.S * N, o.S * N).T
    assert _miss(A7, A) < 1e-13
    assert _miss(ref.reduced_stepping(A7, M_red, b, T / nt, nt), red.solve(mu)) < 1e-10


# ----------------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize('name,N', A_CELLS)
def test_project_mass_mutants_miss(name, N):
    p, o = oracle(name)
    t = p['grid'].template
    V = bases_of(name, N)
    want = ref.project_mass(o, V)
    # the reference's own accuracy against float64, and the conditioning the GPU test's 1e-12 rests on
    Mt = o.M.tocsr()
    for s in range(o.S):
        dofs = o.dofs_of(s)
        assert _miss(V[s].T @ (Mt[dofs][:, dofs] @ V[s]), want[s]) < 5e-14
    full = ref.project_mass(o, c3.make_bases3d(o.S, o.n, N, seed=N)).astype(np.float64)
    assert max(np.linalg.cond(full[s]) for s in range(o.S)) < (40.0 if name == 'interior_3x3x3' else 10.0)
    if t.n_T % ref.WAVES:
        wrong = ref.project_mass(o, V, drop_tail=True)
        assert min(_miss(wrong[s], want[s]) for s in range(o.S)) > 1e-6
    if N > 16:
        wrong = ref.project_mass(o, V, drop_cross=True)
        # (subdomain 0 apart: its zeroed last column is the whole second tile at N = 17)
        assert min(_miss(wrong[s], want[s]) for s in range(1, o.S)) > 1e-6
    else:
        assert np.array_equal(ref.project_mass(o, V, drop_cross=True), want)


def test_the_element_types_share_one_mass_block():
    """The mutant 'one element type's TM replaced by another type's' does not exist on these meshes: the six Kuhn tetrahedra of a
    cube have the same volume and the P2 mass block of an affine element is |K| times the reference block, so all n_T blocks of a
    subdomain are one matrix (and lrbms3's TM [6][100] holds it six times).  The swap is the identity at every cell of A; no test
    can tell the types apart through the mass.  Should a mesh with unequal element volumes arrive, this test fails and the swap
    becomes a mutant to separate."""
    for name in sorted({name for name, _ in A_CELLS}):
        p, o = oracle(name)
        t = p['grid'].template
        assert set(np.unique(t.elem_type)) == set(range(6))
        V = bases_of(name, 17)
        for s in (0, o.S - 1):
            blocks = ref.element_mass_blocks(o, s)
            assert np.abs(blocks - blocks[0]).max() <= 1e-15 * np.abs(blocks[0]).max()
        wrong = ref.project_mass(o, V, elem_type=t.elem_type, swap_types=(0, 3))
        assert _miss(wrong, ref.project_mass(o, V)) < 1e-15


# ----------------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize('name,L', B_CELLS)
def test_mass_inverse_norm2_mutants_miss(name, L):
    p, o = oracle(name)
    nT = p['grid'].template.n_T
    Y = vectors_of(name, L)
    want = ref.mass_inverse_norm2(o, Y)
    assert np.all(want > 0.0)
    if L > ref.CHUNK:
        wrong = ref.mass_inverse_norm2(o, Y, first_trip_only=True)
        assert np.array_equal(wrong[:, :ref.CHUNK], want[:, :ref.CHUNK]) and _miss(wrong, want) > 1e-6
    hit = [l for l in range(L) if ref.chunk_of(L, l)[1] > 1 and nT % ref.chunk_of(L, l)[1]]
    wrong = ref.mass_inverse_norm2(o, Y, drop_group_tail=True)
    for l in range(L):
        if l in hit:
            assert _miss(wrong[:, l], want[:, l]) > 1e-6
        else:
            assert np.array_equal(wrong[:, l], want[:, l])


# ----------------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize('N,Q,L', C_CELLS)
def test_time_residual_mutants_miss(N, Q, L):
    p, _ = oracle(C_PROBLEM)
    nbr = np.asarray(p['grid'].neighbor_slots).reshape(-1, 7)
    B, M_red, dU, theta, keep = synthetic_operators(nbr, N, Q, L)
    for s in range(nbr.shape[0]):          # the 1e-10 of the GPU test is the reference's to give
        assert np.linalg.cond(M_red[s][np.ix_(keep[s], keep[s])]) < 1e3
    assert int((~keep).sum()) == min(3, N - 1) and (N == 1 or not keep[C_RAGGED, -1])
    want = ref.reduced_time_residual(B, M_red, nbr, theta, dU, keep)
    assert np.all(want > 0.0)
    if N > 1:
        wrong = ref.reduced_time_residual(B, M_red, nbr, theta, dU, keep, diagonal_inverse=True)
        assert min(_miss(wrong[:, s], want[:, s]) for s in range(nbr.shape[0])) > 1e-6
    for slot in range(7):
        wrong = ref.reduced_time_residual(B, M_red, nbr, theta, dU, keep, drop_slot=slot)
        for s in range(nbr.shape[0]):
            if nbr[s, slot] >= 0:
                assert _miss(wrong[:, s], want[:, s]) > 1e-6, (slot, s)
            else:
                assert np.array_equal(wrong[:, s], want[:, s])


# ------------------------------------------------------------------------------------------------------ branch coverage
def _body(src, name):
    m = re.search(r'\n[^\n]*\b' + re.escape(name) + r'\([^;{]*\{.*?\n\}\n', src, re.S)
    assert m, name
    return m.group(0)


def test_the_cells_reach_every_branch():
    src = c3.source3d()
    # A: T = (N + 15) / 16 selects k3p_project_mass<1..4>; a wave takes the elements wave, wave + 8, ...
    host = _body(src, 'int lrbms3_project_mass')
    assert 'const int T = (N + 15) / 16;' in host and 'N > 64' in host
    assert sorted(int(v) for v in re.findall(r'k3p_project_mass<(\d+)>', host)) == [1, 2, 3, 4]
    kernel = _body(src, 'void k3p_project_mass')
    assert 'for (int e = wave; e < t.nT; e += 8)' in kernel and ref.WAVES == 8
    nT = {name: oracle(name)[0]['grid'].template.n_T for name in {c[0] for c in A_CELLS + B_CELLS} | {C_PROBLEM, D_PROBLEM}}
    assert {k: nT[k] for k in ('aniso_2x2x1', 'q1_strip', 'kc_3x1x2', 'interior_3x3x3')} == \
        {'aniso_2x2x1': 48, 'q1_strip': 48, 'kc_3x1x2': 36, 'interior_3x3x3': 6}
    for T in (1, 2, 3, 4):                  # every instantiation with n_T % 8 != 0; the edges 16 k - 1, 16 k, 16 k + 1
        assert any((N + 15) // 16 == T and nT[name] % 8 for name, N in A_CELLS)
    on_kc = {N for name, N in A_CELLS if name == 'kc_3x1x2'}
    assert all({16 * k - 1, 16 * k} <= on_kc for k in (1, 2, 3, 4)) and all(16 * k + 1 in on_kc for k in (1, 2, 3))
    assert any(nT[name] < 8 and N > 32 for name, N in A_CELLS)          # fewer elements than waves, beyond T = 2
    assert ZERO_TILE_CELL in A_CELLS
    # B: Lc, G per trip of the l0 loop
    kernel = _body(src, 'void k3p_mass_inv_norm2')
    assert 'for (int l0 = 0; l0 < L; l0 += 256)' in kernel and ref.CHUNK == 256
    assert 'Lc = L - l0 < 256 ? L - l0 : 256, G = 256 / Lc, g = tid / Lc' in kernel
    assert 'for (int e = g; e < t.nT; e += G)' in kernel
    classes = set()
    for name, L in B_CELLS:
        trips = sorted({l // 256 for l in range(L)})
        for trip in trips:
            Lc, G = ref.chunk_of(L, 256 * trip)
            assert Lc == min(L - 256 * trip, 256) and G == 256 // Lc
            classes.add(('G = 1' if G == 1 else 'G | n_T' if nT[name] % G == 0 else 'G > n_T' if G > nT[name] else 'G !| n_T',
                         'idle' if 256 % Lc else 'full', 'trip {}'.format(min(trip, 1))))
    kinds = {c[0] for c in classes}
    assert kinds == {'G = 1', 'G | n_T', 'G > n_T', 'G !| n_T'}
    assert {c[1] for c in classes if c[0] == 'G = 1'} == {'idle', 'full'} and ('G | n_T', 'idle', 'trip 0') in classes
    assert any(c[2] == 'trip 1' for c in classes) and any(L > 512 for _, L in B_CELLS)
    # C: the limits of the export and the slots of the mesh
    host = _body(src, 'int lrbms3_reduced_time_residual')
    assert 'Q < 1 || Q > 8 || N < 1 || N > 64 || L < 1 || L > 65535' in host
    assert 'sizeof(double) * N * (2 * N + 1)' in host and 8 * 64 * (2 * 64 + 1) == 66048
    assert {N for N, _, _ in C_CELLS} >= {1, 33, 64} and {Q for _, Q, _ in C_CELLS} >= {1, 8}
    nbr = np.asarray(oracle(C_PROBLEM)[0]['grid'].neighbor_slots).reshape(-1, 7)
    present = (nbr >= 0).sum(axis=1)
    assert present.max() == 7 and present.min() < 7 and present[13] == 7 and C_RAGGED in nbr[13]
    # D: beyond the batched exports' width, at Q = 1 (the pass takes Q N <= 64)
    assert all(32 < N <= 64 for N in D_CELLS) and len(oracle(D_PROBLEM)[0]['lambdas']) == 1
    assert 'needs N <= 32 and nmu <= 64' in src
