"""The C surface of the parabolic enrichment (``lrbms_local_correction_euler`` and its work size): declared in
include/lrbms_hip.h, exported by the library, bound by the ctypes table with the declared argument count -- and the product does
not import the oracle.  No GPU, no compute call."""
import ctypes
import os
import re

NAMES = ('lrbms_local_correction_euler', 'lrbms_local_correction_euler_work_size')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declarations():
    text = open(os.path.join(ROOT, 'include', 'lrbms_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return {name: re.search(r'\b(int64_t|int)\s+' + name + r'\s*\(([^;]*?)\)\s*;', text, flags=re.S) for name in NAMES}


def test_the_new_symbols_are_declared_exported_and_bound():
    from pylrbms_amd import _native
    from pylrbms_amd._build import build_native
    lib = build_native()
    handle = ctypes.CDLL(lib)
    bound = _native.load_library(lib)
    for name, decl in _declarations().items():
        assert decl is not None, name + ' is not declared'
        assert hasattr(handle, name), name + ' is not exported'
        restype, argtypes = _native.SIGNATURES[name]
        assert len(argtypes) == len(decl.group(2).split(',')), name
        assert restype is (_native.c_i64 if decl.group(1) == 'int64_t' else ctypes.c_int), name
        assert getattr(bound, name).argtypes == argtypes
    # the trajectory export takes what the stationary one takes plus K, dt, nt and the coefficient table
    assert len(_native.SIGNATURES[NAMES[0]][1]) == len(_native.SIGNATURES['lrbms_local_correction_solve'][1]) + 4


def test_the_host_layers_reach_the_export():
    from pylrbms_amd import _native
    from pylrbms_amd.discretize_parabolic_block_swipdg import InstationaryDuneDiscretization
    from pylrbms_amd.engine import Engine
    from pylrbms_amd.reductor import InstationaryReducedDiscretization, ParabolicLRBMSReductor
    assert callable(_native.NativeContext.local_correction_euler) and callable(Engine.local_corrections_euler)
    assert callable(InstationaryDuneDiscretization.solve_for_local_correction_trajectories)
    assert ParabolicLRBMSReductor.enrich_local_batch is not ParabolicLRBMSReductor.__mro__[1].enrich_local_batch
    assert callable(InstationaryReducedDiscretization.local_indicators)


def test_the_product_imports_nothing_from_the_oracle():
    pkg = os.path.join(ROOT, 'pylrbms_amd')
    seen = 0
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                seen += 1
                assert not re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M), f
                assert not re.search(r'\b(parabolic_enrichment_ref|import_module\(\s*[\'"]oracle)', src), f
    assert seen > 20
