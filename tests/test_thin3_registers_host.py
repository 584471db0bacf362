"""The build-time guard of the thin kernels' register count (pylrbms_amd._isa_check.check_thin_registers), on the CPU box.

k_thin3<1..3> and k_thin_ncf run five 256-thread workgroups per CU only while a wave takes at most 96 registers of the unified
file and no scratch; the guard reads exactly that from the kernel descriptors of the product build's gfx950 assembly and fails
the build otherwise.  Here: the tree passes, and synthetic descriptors one register over the line, with scratch, or with a kernel
missing are refused."""
import re

import pytest

from pylrbms_amd._isa_check import THIN_KERNELS, THIN_VGPR_LIMIT, IsaCheckError, check_thin_registers

SYMBOLS = {
    'k_thin3<1>': '_ZN12_GLOBAL__N_17k_thin3ILi1EEEv4TmplNS_10ThinRtArgsENS_11ThinNcfArgsEPKdPd',
    'k_thin3<2>': '_ZN12_GLOBAL__N_17k_thin3ILi2EEEv4TmplNS_10ThinRtArgsENS_11ThinNcfArgsEPKdPd',
    'k_thin3<3>': '_ZN12_GLOBAL__N_17k_thin3ILi3EEEv4TmplNS_10ThinRtArgsENS_11ThinNcfArgsEPKdPd',
    'k_thin3<4>': '_ZN12_GLOBAL__N_17k_thin3ILi4EEEv4TmplNS_10ThinRtArgsENS_11ThinNcfArgsEPKdPd',
    'k_thin_ncf': '_ZN12_GLOBAL__N_110k_thin_ncfE4TmplNS_11ThinNcfArgsE',
    'k_thin_rt': '_ZN12_GLOBAL__N_19k_thin_rtE4TmplNS_10ThinRtArgsE',
}


def _descriptor(symbol, next_free_vgpr, scratch=0, accum_offset=None):
    accum_offset = accum_offset if accum_offset is not None else (next_free_vgpr + 3) // 4 * 4
    return ('\t.section\t.rodata,"a",@progbits\n\t.p2align\t6, 0x0\n'
            '\t.amdhsa_kernel {}\n'
            '\t\t.amdhsa_group_segment_fixed_size 0\n'
            '\t\t.amdhsa_private_segment_fixed_size {}\n'
            '\t\t.amdhsa_kernarg_size 616\n'
            '\t\t.amdhsa_next_free_vgpr {}\n'
            '\t\t.amdhsa_next_free_sgpr 100\n'
            '\t\t.amdhsa_accum_offset {}\n'
            '\t\t.amdhsa_reserve_vcc 1\n'
            '\t.end_amdhsa_kernel\n').format(symbol, scratch, next_free_vgpr, accum_offset)


def _text(**over):
    """Descriptors of the six thin kernels: the guarded four at the limit unless ``over`` says otherwise (kernel name with '<', '>'
    and '_' spelled k_thin3_1 ... -> (next_free_vgpr, scratch) or None to leave the kernel out)."""
    spec = {k: (THIN_VGPR_LIMIT, 0) for k in THIN_KERNELS}
    spec['k_thin3<4>'] = (112, 0)         # N in 49 .. 64: three workgroups by LDS, not guarded
    spec['k_thin_rt'] = (88, 0)
    for key, val in over.items():
        name = re.sub(r'^k_thin3_(\d)$', r'k_thin3<\1>', key)
        assert name in spec, key
        spec[name] = val
    return ''.join(_descriptor(SYMBOLS[k], *v) for k, v in spec.items() if v is not None)


def test_the_tree_keeps_five_workgroups_per_cu():
    from pylrbms_amd._build import fused_assembly
    with open(fused_assembly()) as fh:
        report = check_thin_registers(fh.read())
    assert len(report) == len(THIN_KERNELS), report
    for kernel in THIN_KERNELS:
        line = [r for r in report if r.startswith(kernel + ':')]
        assert len(line) == 1, (kernel, report)
        regs, scratch = re.search(r'next free VGPR (\d+), accum_offset \d+, scratch (\d+)', line[0]).groups()
        assert int(regs) <= 96 and int(scratch) == 0, line


def test_the_build_runs_the_guard():
    """check_isa (run by build_native beside the compiles) reports the four kernels."""
    from pylrbms_amd._build import check_isa
    report = check_isa()
    for kernel in THIN_KERNELS:
        assert any(r.startswith(kernel + ': next free VGPR') for r in report), (kernel, report)


def test_descriptors_at_the_limit_pass():
    report = check_thin_registers(_text())
    assert len(report) == 4 and all('next free VGPR 96' in r for r in report), report


@pytest.mark.parametrize('kernel', ['k_thin3_1', 'k_thin3_2', 'k_thin3_3', 'k_thin_ncf'])
def test_one_register_over_the_line_is_refused(kernel):
    with pytest.raises(IsaCheckError, match=r'next free VGPR 97 > 96'):
        check_thin_registers(_text(**{kernel: (97, 0)}))


def test_accumulation_registers_count():
    """88 architectural registers and 16 behind accum_offset are 104 of the unified file: four workgroups."""
    text = _text(k_thin3_3=None) + _descriptor(SYMBOLS['k_thin3<3>'], 104, accum_offset=88)
    with pytest.raises(IsaCheckError, match=r'k_thin3<3>: next free VGPR 104 > 96 \(accum_offset 88\)'):
        check_thin_registers(text)


def test_scratch_is_refused():
    with pytest.raises(IsaCheckError, match=r'k_thin_ncf: 20 bytes of scratch'):
        check_thin_registers(_text(k_thin_ncf=(95, 20)))


def test_a_missing_kernel_is_refused():
    with pytest.raises(IsaCheckError, match=r'no kernel descriptor of k_thin3<2>'):
        check_thin_registers(_text(k_thin3_2=None))


def test_the_wide_instantiation_is_not_guarded():
    check_thin_registers(_text())         # k_thin3<4> stands at 112 in every synthetic text
