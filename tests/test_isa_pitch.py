"""What hipcc makes of csrc/pitch.hip for gfx950 (no GPU: it cross-compiles): the persistent WSOLA workgroup and the resampler keep
everything in registers -- 0 spilled vector registers, 0 bytes of scratch memory, no scratch instruction -- and the 1024-thread
WSOLA kernel fits the 128 vector registers that four waves per SIMD leave it."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc (cross-compiles without a GPU)")
def test_pitch_kernels_keep_everything_in_registers():
    import isa_check
    text = isa_check.compile_asm(os.path.join(isa_check.CSRC, "pitch.hip"))
    assert not re.search(r"^\s*scratch_", text, flags=re.M)
    found = {}
    for m in re.finditer(r"\.name:\s+(\S*(?:tempo_wsola_kernel|resample_ratio_kernel)\S*)\n(.*?)\.wavefront_size", text, flags=re.S):
        found[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_count|vgpr_spill_count):\s+(\d+)", m.group(2))}
    assert len(found) == 4, list(found)
    for k, v in found.items():
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        assert v["vgpr_count"] <= 128, (k, v)
