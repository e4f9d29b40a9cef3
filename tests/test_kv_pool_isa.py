"""CPU, from the gfx950 code objects of the built library: the pooled (page-table) forms of the talker's two decode attentions issue
their first request burst back to back, as the contiguous forms do (tests/test_host_logic.py::
test_frame_step_kernels_issue_their_requests_back_to_back pins those).  The page ids of the register window are wave-uniform -- key
g + 16 pg lies in page pg for every lane, the row comes from blockIdx -- and are fetched by scalar loads, which count on lgkmcnt: no
`s_waitcnt vmcnt` sits between this step's row, the norm weights and the speculative K / V requests, and the burst is exactly as long as
the contiguous form's (no id travels as a vector load)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the contiguous forms' bursts as tests/test_host_logic.py pins them: 8 / 6 row + 5 norm / rope + 16 speculative K / V chunk requests
PINNED = {"attn_tk_kernel<unsigned short, 2, {ct}>": 29, "attn_tk_kernel<unsigned short, 1, {ct}>": 27}
# ... and the instantiations that test does not name: their burst is read from the contiguous form of the same library
OTHERS = ["attn_tk_kernel<float, 2, {ct}>", "attn_tk_kernel<float, 1, {ct}>", "attn_tk16_kernel<2, {ct}>", "attn_tk16_kernel<1, {ct}>"]


def test_pooled_decode_attentions_issue_their_first_burst_back_to_back(libqtts):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_waits
    ks = isa_waits.kernels(libqtts)

    def one(key):
        hit = [ins for n, ins in ks.items() if key in n]
        assert len(hit) == 1, key
        return hit[0]
    for key in list(PINNED) + OTHERS:
        contig, pooled = one(key.format(ct="true")), one(key.format(ct="false"))
        n_first = PINNED.get(key, isa_waits.first_burst(contig))
        assert n_first >= 27 and isa_waits.waits_inside_burst(contig, n_first) == [], key
        assert isa_waits.waits_inside_burst(pooled, n_first) == [], (key, "a wait inside the pooled form's first request burst")
        assert isa_waits.first_burst(pooled) == isa_waits.first_burst(contig), (key, isa_waits.first_burst(pooled), isa_waits.first_burst(contig))
        # the ids are there, and they are scalar: more scalar loads in front of the burst's end than the contiguous form has
        assert isa_waits.scalar_loads_before(pooled, n_first) > isa_waits.scalar_loads_before(contig, n_first), key
