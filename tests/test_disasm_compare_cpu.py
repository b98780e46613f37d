"""CPU tests of scripts/disasm_kernel.py's compare mode: the metadata note is
parsed kernel by kernel and fails loudly on a layout it does not know, the
instruction classes are counted as the acceptance rule needs them, and a
kernel that differs is refused exactly when scratch appears, LDS bytes or a
memory / LDS-DMA / atomic count move, or the VGPR count crosses a wave step."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("disasm_kernel", os.path.join(ROOT, "scripts", "disasm_kernel.py"))
dk = importlib.util.module_from_spec(spec)
spec.loader.exec_module(dk)

NOTE = """Displaying notes found in: .note
  Owner                Data size \tDescription
  AMDGPU               0x000037da\tNT_AMDGPU_METADATA (AMDGPU Metadata)
    AMDGPU Metadata:
        ---
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           208
        .value_kind:     by_value
    .group_segment_fixed_size: 8
    .name:           _ZN3nbx1aE
    .private_segment_fixed_size: 0
    .sgpr_spill_count: 3
    .vgpr_count:     93
  - .args:
      - .name:           hidden
        .offset:         0
    .group_segment_fixed_size: 16640
    .name:           '_ZN3nbx1bE'
    .private_segment_fixed_size: 0
    .sgpr_spill_count: 0
    .vgpr_count:     44
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
amdhsa.version:
  - 1
  - 2
...
"""


def test_metadata_note_is_parsed_per_kernel():
    meta = dk.parse_kernel_meta(NOTE)
    assert meta == {"_ZN3nbx1aE": {"vgpr": 93, "sgpr_spill": 3, "lds_bytes": 8, "scratch": 0},
                    "_ZN3nbx1bE": {"vgpr": 44, "sgpr_spill": 0, "lds_bytes": 16640, "scratch": 0}}


@pytest.mark.parametrize("broken", [
    NOTE.replace("amdhsa.kernels:", "amdhsa.kernelz:"),                    # no kernel list
    NOTE.replace("    .vgpr_count:     44\n", ""),                         # a field gone
    NOTE.replace("amdhsa.kernels:\n", "amdhsa.kernels:\n    .odd: 1\n"),   # not a list
])
def test_unknown_note_layout_fails(broken):
    with pytest.raises(SystemExit):
        dk.parse_kernel_meta(broken)


def test_instruction_classes():
    ins = ["global_load_dwordx4 v[0:3], v[4:5], off nt", "global_store_dwordx4 v[4:5], v[0:3], off",
           "global_load_lds_dwordx4 v[2:3], off nt", "ds_read_b32 v1, v2", "ds_read2_b32 v[1:2], v3 offset1:1",
           "global_atomic_add v1, v[2:3], v4, off sc0", "s_waitcnt vmcnt(0)", "s_waitcnt lgkmcnt(0)", "s_barrier",
           "v_add_u32_e32 v1, v2, v3", "flat_load_dword v1, v[2:3]"]
    assert dk.count_classes(ins) == {"mem": 3, "dma": 1, "lds": 2, "atomic": 1, "wait": 2, "barrier": 1}


def test_wave_step():
    assert [dk.waves(v) for v in (24, 40, 41, 64, 65, 72, 73, 96, 97, 128, 129, 256, 257, 512)] == \
        [8, 8, 8, 8, 7, 7, 6, 5, 4, 4, 3, 2, 1, 1]


def test_acceptance_rule():
    base = {"vgpr": 76, "sgpr_spill": 4, "lds_bytes": 16640, "scratch": 0, "mem": 41, "dma": 20, "lds": 12,
            "atomic": 2, "wait": 14, "barrier": 0, "n": 430}
    ok = dict(base, n=425, sgpr_spill=9, wait=16, lds=13, vgpr=74)   # free to move
    assert dk.refusal(base, ok, True) == []
    assert dk.refusal(base, ok, False) == ["control kernel differs"]
    assert dk.refusal(base, dict(base, scratch=16), True) == ["scratch"]
    assert dk.refusal(base, dict(base, lds_bytes=8320), True) == ["lds_bytes"]
    assert dk.refusal(base, dict(base, mem=40), True) == ["mem"]
    assert dk.refusal(base, dict(base, dma=24), True) == ["dma"]
    assert dk.refusal(base, dict(base, atomic=3), True) == ["atomic"]
    assert dk.refusal(base, dict(base, vgpr=72), True) == ["waves/SIMD"]   # a gain is a change too
    assert dk.refusal(base, dict(base, vgpr=81), True) == ["waves/SIMD"]
    assert dk.refusal(dict(base, vgpr=41), dict(base, vgpr=40), True) == []   # both at the 8-wave cap
