"""The inputs of the quadrature rule-set tests (tests/quadrature_cases.py), checked on the CPU oracle alone:

* separation: the data can tell two rule sets apart.  Every assembled array of the oracle whose rule's point set differs from the
  control's differs from the control's array by at least ``SEPARATION`` x the parity tolerance it is compared at on the GPU; an
  array whose rules are unchanged is the same bits.  A condition on the inputs, not a measurement of the product;
* the sample-record layouts of ``native_quadrature`` / ``QuadratureSpec3D`` are ascending, packed and within MAXQV / MAXQF, and
  the case lists reach the sizes they claim (1 point, 16 points, 4 edge points, coupling > inner);
* the 3D degrees give the reductions of k3_asm a length shorter than one staged chunk, an exact multiple of it and several
  chunks with a tail."""
import re

import numpy as np
import pytest

import quadrature_cases as qc


# ------------------------------------------------------------------------------------------------------------ separation
@pytest.mark.parametrize('name', [n for n in qc.RULE_SETS_2D if n != qc.CONTROL_2D])
def test_2d_rule_sets_are_separated_from_the_control(name):
    p, d0 = qc.oracle_2d(qc.CONTROL_2D)
    _, d = qc.oracle_2d(name)
    s0, s = qc.oracle_spec_2d(qc.CONTROL_2D), qc.oracle_spec_2d(name)
    a0, a = qc.oracle_arrays_2d(p, d0), qc.oracle_arrays_2d(p, d)
    changed = 0
    for key, fields in qc.ARRAY_RULES_2D.items():
        if all(qc.same_points_2d(f, getattr(s0, f), getattr(s, f)) for f in fields):
            assert np.array_equal(a[key], a0[key]), (name, key)
        else:
            sep = qc.rel(a[key], a0[key])
            print(name, key, 'separation', sep)
            assert sep >= qc.SEPARATION * qc.TOL, (name, key, sep)
            changed += 1
    assert changed > 0, name


@pytest.mark.parametrize('grid,degree', [('first', d) for d in qc.DEGREES_3D] + [('second', d) for d in qc.DEGREES_SECOND_GRID_3D])
def test_3d_degrees_are_separated_from_the_control(grid, degree):
    _, _, a0 = qc.oracle_3d(grid, qc.CONTROL_3D)
    _, _, a = qc.oracle_3d(grid, degree)
    assert set(qc.ARRAYS_3D) == set(qc.ARRAY_RULES_3D) and set(qc.ARRAYS_3D) <= set(a)
    changed = 0
    for key, fields in qc.ARRAY_RULES_3D.items():
        if all(qc.same_points_3d(f, qc.CONTROL_3D, degree) for f in fields):
            assert np.array_equal(a[key], a0[key]), (grid, degree, key)
        else:
            sep = qc.rel(a[key], a0[key])
            print(grid, degree, key, 'separation', sep)
            assert sep >= qc.SEPARATION * qc.TOL, (grid, degree, key, sep)
            changed += 1
    assert changed > 0


# ---------------------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize('name', list(qc.RULE_SETS_2D) + ['uniform1'])
def test_native_quadrature_layout(name):
    from pylrbms_amd.quadrature import EDGE_FIELDS, MAXQF, MAXQV, TRI_FIELDS, QuadratureSpec, native_quadrature
    q = native_quadrature(QuadratureSpec.uniform(1) if name == 'uniform1' else qc.spec_2d(name))
    assert all(1 <= getattr(q, k).n <= MAXQV for k in TRI_FIELDS) and all(1 <= getattr(q, k).n <= MAXQF for k in EDGE_FIELDS)
    assert q.nfs == max(q.system_inner_face.n, q.system_coupling_face.n)
    for stride, segments in qc.RECORDS_2D.values():
        end = 0
        for field, size in segments:                     # ascending and packed: every segment starts where the one before ends
            assert getattr(q, field) == end, (name, field)
            end += size(q)
        assert getattr(q, stride) == (end if segments else q.elliptic_bar.n), (name, stride)


def test_2d_case_list_reaches_the_sizes_it_claims():
    from pylrbms_amd.quadrature import EDGE_FIELDS, MAXQF, MAXQV, TRI_FIELDS, native_quadrature
    qs = {name: native_quadrature(qc.spec_2d(name)) for name in qc.RULE_SETS_2D}
    tri = {getattr(q, k).n for q in qs.values() for k in TRI_FIELDS}
    edge = {getattr(q, k).n for q in qs.values() for k in EDGE_FIELDS}
    assert 1 in tri and MAXQV in tri and 1 in edge and MAXQF in edge
    assert any(q.system_coupling_face.n > q.system_inner_face.n for q in qs.values())
    assert any(q.system_coupling_face.n < q.system_inner_face.n for q in qs.values())
    assert any(w < 0.0 for q in qs.values() for k in TRI_FIELDS for w in getattr(q, k).w[:getattr(q, k).n])      # order 3
    one = qs['one_point']
    assert one.nfs == 1 and all(getattr(one, k).n == 1 for k in TRI_FIELDS if k != 'df_bb') and one.df_bb.n == 3


def test_padded_layouts_pass_the_validation_and_have_gaps():
    """``padded_quadrature`` moves every offset up and enlarges every stride, keeps the rules; ``relayout_record`` puts every sample
    where the new layout reads it and NaN everywhere else."""
    from pylrbms_amd.quadrature import native_quadrature
    for name in qc.PADDED_SETS_2D:
        q = native_quadrature(qc.spec_2d(name))
        g = qc.padded_quadrature(q)
        assert g.nfs == q.nfs and g.pad_ == q.pad_ and g.system_volume.pad == q.system_volume.pad
        for record, (stride, segments) in qc.RECORDS_2D.items():
            assert getattr(g, stride) > getattr(q, stride)
            x = np.arange(1.0, 1.0 + 2 * getattr(q, stride)).reshape(2, -1)
            y = qc.relayout_record(x, q, g, record)
            for field, size in segments:
                assert 1 <= getattr(g, field) - getattr(q, field)
                assert np.array_equal(y[:, getattr(g, field):getattr(g, field) + size(q)], x[:, getattr(q, field):getattr(q, field) + size(q)])
            assert np.isnan(y).sum() == 2 * (getattr(g, stride) - getattr(q, stride))
            assert np.array_equal(qc.relayout_record(y, g, q, record), x)


@pytest.mark.parametrize('degree', (qc.CONTROL_3D,) + qc.DEGREES_3D)
def test_spec3d_layout(degree):
    from pylrbms_amd.grid3d import QuadratureSpec3D, rule_size, tet_rule, tri_rule
    s = QuadratureSpec3D(degree)
    assert (s.nA, s.nB, s.nC) == tuple(len(tet_rule(x)[1]) for x in (s.system_volume, s.product_volume, s.estimator_volume))
    assert (s.nFs, s.nFf) == tuple(len(tri_rule(x)[1]) for x in (s.system_face, s.flux_face))
    assert s.nA == rule_size(degree + 2) ** 3 and s.nC == rule_size(3 * degree + 4) ** 3
    assert s.o_fs == s.nA and s.o_ff == s.o_fs + 4 * s.nFs and s.o_c == s.o_ff + 4 * s.nFf and s.lam_stride == s.o_c + s.nC
    assert s.hat_stride == s.nB + s.nC and s.f_stride == s.nB + s.nC
    g = qc.PaddedSpec3D(degree)
    assert g.o_fs > s.o_fs and g.o_ff - g.o_fs > 4 * s.nFs and g.o_c - g.o_ff > 4 * s.nFf and g.lam_stride > g.o_c + s.nC
    assert g.hat_stride > s.hat_stride and g.f_stride > s.f_stride and (g.nA, g.nB, g.nC, g.nFs, g.nFf) == (s.nA, s.nB, s.nC, s.nFs, s.nFf)
    x = np.arange(1.0, 1.0 + s.lam_stride)[None]
    y = g.relayout_lam(x)
    assert np.isnan(y).sum() == g.lam_stride - s.lam_stride and np.array_equal(y[0, g.o_c:g.o_c + s.nC], x[0, s.o_c:])


# -------------------------------------------------------------------------------------------------------------- chunking
def _asm_kc():
    from common3d import source3d
    return int(re.search(r'constexpr int ASM_KC = (\d+);', source3d()).group(1))


def test_degrees_cover_the_chunk_forms_of_k3_asm():
    """k3_asm stages its table ASM_KC quadrature points at a time.  Over the degrees under test (control included) its reductions
    meet all three forms -- shorter than one chunk, an exact multiple of the chunk, several chunks with a tail -- and the operator
    classes of length nB and nC meet each of them; nFs and nA + 8 nFs have one form at every degree (asserted below, with the
    reason)."""
    kc = _asm_kc()
    assert kc == 32
    lengths = {deg: qc.asm_reduction_lengths(deg) for deg in (qc.CONTROL_3D,) + qc.DEGREES_3D}
    assert lengths[0] == {'nB': 27, 'nC': 27, 'nFs': 9, 'nA+8nFs': 80} and lengths[1] == {'nB': 27, 'nC': 64, 'nFs': 9, 'nA+8nFs': 80}
    assert lengths[3] == {'nB': 64, 'nC': 343, 'nFs': 16, 'nA+8nFs': 155} and lengths[4] == {'nB': 125, 'nC': 729, 'nFs': 25, 'nA+8nFs': 264}
    allk = [k for v in lengths.values() for k in v.values()]
    assert any(k < kc for k in allk) and any(k % kc == 0 for k in allk) and any(k > 2 * kc and k % kc for k in allk)
    assert max(-(-k // kc) for k in allk) == 23
    forms = {'below': lambda k: k < kc, 'multiple': lambda k: k % kc == 0, 'chunks_and_tail': lambda k: k > 2 * kc and k % kc != 0}
    reach = {op: {f for f, hit in forms.items() for deg in lengths if hit(lengths[deg][op])} for op in ('nB', 'nC', 'nFs', 'nA+8nFs')}
    # nB: 27 | 64 | 125;  nC: 27 | 64 | 216, 343, 729;  nA + 8 nFs: 80, 155 (tails) and 264 (tail) -- never below one chunk or a multiple:
    # the volume rule alone has 8 points and the four faces add 8 nFs >= 72; nFs: 9, 16, 25 -- a face rule never fills a chunk
    assert reach['nB'] == set(forms) and reach['nC'] == set(forms)
    assert reach['nFs'] == {'below'} and reach['nA+8nFs'] == {'chunks_and_tail'}
