"""Call history and cross-context independence of the full-order solve, on the GPU.

A discretization's ``d.solve(mu)`` must not depend on what ran before it in the process: reduced work on the same context
(prebuilt preconditioner, batched solves on the library's side streams), a ``reduce()`` of a second discretization with a
two-component affine source (fused pass, flux reconstruction, divergence, source projection on another context), that
context being closed.  The reference answer is the first thing d1 does; after the sequence, d1's solve and the first solve
of a second, untouched discretization of the same problem must give the same bits and the same iteration count.  The
sequence is tests/call_order_seq.py; the regression test runs it in a fresh process, where the caching allocator's state is
that of the recorded finding."""
import os
import subprocess
import sys

import numpy as np
import pytest

import call_order_seq as seq

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NX = 4                       # 16 subdomains of 128 elements: the residual sums per wave of the full-order CG (r0w) run


def _discretize(p):
    from pylrbms_amd.discretize_elliptic_block_swipdg import discretize
    return discretize(p)[0]


@pytest.mark.parametrize('close_d2', [False, True])
def test_fom_solve_is_independent_of_the_call_history(close_d2):
    import torch
    p, p2 = seq.problems(NX)
    d1 = _discretize(p)
    ref = d1.solve(seq.MU).tensor.clone()
    ref_info = dict(d1.last_solve_info)
    assert ref_info['relative_residual'] <= 1e-12
    d1b = _discretize(p)                   # built before the sequence, first solved after it
    d2 = _discretize(p2)
    seq.sequence(d1, d2, close_d2=close_d2)
    x = d1.solve(seq.MU).tensor
    assert d1.last_solve_info == ref_info
    assert torch.equal(x, ref)
    xb = d1b.solve(seq.MU).tensor
    assert d1b.last_solve_info == ref_info
    assert torch.equal(xb, ref)
    d1c = _discretize(p)                   # built after the sequence, beside d1b
    assert torch.equal(d1c.solve(seq.MU).tensor, ref) and d1c.last_solve_info == ref_info


def _child(nx, mode, out):
    r = subprocess.run([sys.executable, os.path.join(HERE, 'call_order_seq.py'), str(nx), mode, str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, 'child {} exited {}:\n{}\n{}'.format(mode, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return np.load(out)


def test_first_fom_solve_after_the_recorded_sequence_in_a_fresh_process(tmp_path):
    """Section 5.4.2's stage 7 in a process of its own: d1's first solve comes after the reduced work and d2's reduce()
    with its source.  It must converge in the iterations of a fresh process and give its bits."""
    nx = 32                                # config 3's grid: 1 024 subdomains of 128 elements
    fresh = _child(nx, 'fresh', tmp_path / 'fresh.npz')
    after = _child(nx, 'sequence', tmp_path / 'sequence.npz')
    assert float(after['relative_residual']) <= 1e-12
    assert int(after['iterations']) == int(fresh['iterations'])
    assert np.array_equal(after['x'], fresh['x'])
