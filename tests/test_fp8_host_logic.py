"""Static checks of the fp8 decode-GEMM kernels in the built gfx950 code objects (no GPU): the batch <= 8 form keeps skinny8_kernel's
rule -- every request of the launch is issued before the first `s_waitcnt vmcnt` -- and there is one fp8 instantiation per bf16 one."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fp8_batch8_kernels_issue_their_requests_back_to_back(libqtts):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_waits
    ks = isa_waits.kernels(libqtts)
    inst = lambda key: {re.search(key + r"<([^>]*)>", n).group(1) for n in ks if key + "<" in n}
    s8, b8 = inst("skinny8_fp8_kernel"), inst("skinny8_kernel")
    assert s8 == b8 and len(s8) >= 30, (len(s8), len(b8))
    for n, ins in ks.items():
        if "skinny8_fp8_kernel<" not in n:
            continue
        n_loads = sum(isa_waits.is_load(i) for i in ins)
        assert n_loads >= 5, (n, n_loads)
        assert isa_waits.waits_inside_burst(ins, n_loads) == [], (n, "a wait between the requests of the launch")
        assert any("cvt_scalef32_pk_bf16_fp8" in str(i) for i in ins), (n, "no hardware fp8 -> bf16 conversion")
