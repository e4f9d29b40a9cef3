"""CPU, emulator only: the pooled (page-table) forms of the talker's decode attentions -- `attn_tk_kernel<.., false>` on bf16 and fp32
caches, `attn_tk16_kernel<.., false>` on a bf16 cache with transposed V pages -- from their real source, against the CONTIGUOUS forms on
the same keys.  The pooled forms fetch the page ids of a chunk through a wave-uniform table index; the address arithmetic, the key
ownership and the combine order are the contiguous form's, so output and appended K / V must be BIT-identical.

The table is what the engine's allocator produces: every row holds ceil((S0 + 1) / 16) pages drawn from a random permutation of the
pool, every other entry names the sink page.  Never-written slots of the contiguous pool hold NaN, the sink holds zeros (as after
finalize), every page nobody was granted holds a sentinel: nothing outside the rows' granted pages and the sink may be written.
Lengths sit at every page and register-window edge; rows carry left pads; 1 and 3 splits; three wave orders of the emulator."""
import ctypes as C

import numpy as np
import pytest

from test_hostemu import _bf16_round, _ptr, emu  # noqa: F401  (`emu` is a fixture)

HD, EPS = 128, 1e-6
LENGTHS = [15, 16, 17, 63, 64, 65, 255, 256, 257]
SENTINEL16, SENTINEL32 = 0x1234, np.float32(-77.25)


def _case(emu, g, form, B, nh, nkv, S0, npads, nsplit_orders):
    bf16 = form != "tk_f32"
    vt = form == "tk16"
    inv_freq = (1.0 / (10000.0 ** (np.arange(64) / 64.0))).astype(np.float32)
    qw = (1 + 0.1 * g.standard_normal(HD)).astype(np.float32)
    kw = (1 + 0.1 * g.standard_normal(HD)).astype(np.float32)
    need = (S0 + 1 + 15) // 16                  # pages that hold the cached keys and the appended one
    pps = need + 1                              # one entry more: the speculative loads and the clamp reach it
    n_pages = B * pps
    sink = n_pages - 1
    perm = g.permutation(n_pages - 1)
    table = np.full((B, pps), sink, np.int32)
    for b in range(B):
        table[b, :need] = perm[b * need:(b + 1) * need]
    granted = set(int(x) for x in table[:, :need].reshape(-1))
    assert len(granted) == B * need and sink not in granted
    ld = (nh + 2 * nkv) * HD
    qkv = g.standard_normal((B, ld)).astype(np.float32)
    npad = np.asarray(npads, np.int32)
    kshape, vshape = (n_pages, nkv, 16, HD), ((n_pages, nkv, HD, 16) if vt else (n_pages, nkv, 16, HD))
    K = (g.standard_normal((B, nkv, S0, HD)) * 0.7).astype(np.float32)
    V = g.standard_normal((B, nkv, S0, HD)).astype(np.float32)
    if bf16:
        K, V = _bf16_round(K)[1], _bf16_round(V)[1]
        dt, hole, zero, sentinel = np.uint16, 0x7FC0, 0, SENTINEL16
    else:
        dt, hole, zero, sentinel = np.float32, np.float32(np.nan), np.float32(0), SENTINEL32
    kc, vc = np.full(kshape, hole, dt), np.full(vshape, hole, dt)              # contiguous: never-written slots hold NaN
    kp, vp_ = np.full(kshape, sentinel, dt), np.full(vshape, sentinel, dt)    # pooled: pages nobody holds keep the sentinel
    kp[sink], vp_[sink] = zero, zero
    for b in range(B):
        for i in range(need):
            kp[table[b, i]], vp_[table[b, i]] = hole, hole
        for s in range(int(npad[b]), S0):
            for pool_k, pool_v, page in ((kc, vc, b * pps + s // 16), (kp, vp_, table[b, s // 16])):
                pool_k[page, :, s % 16] = K[b, :, s]
                if vt:
                    pool_v[page, :, :, s % 16] = V[b, :, s]
                else:
                    pool_v[page, :, s % 16] = V[b, :, s]
    bits = lambda a: a.view(np.uint32) if a.dtype == np.float32 else a
    contiguous_out = []
    for nsplit, order in nsplit_orders:
        outs = []
        for tab, k0, v0 in ((None, kc, vc), (table, kp, vp_)):
            kk, vv = k0.copy(), v0.copy()
            out = np.full((B, nh * HD + 4), 5.0, np.float32)
            emu.hostemu_set_fiber_order(order)
            try:
                rc = emu.hostemu_attn_decode(_ptr(qkv), ld, B, 1, nh, nkv, _ptr(qw), _ptr(kw), EPS, _ptr(inv_freq), _ptr(npad), S0,
                                             _ptr(kk), _ptr(vv), _ptr(tab) if tab is not None else None, pps, 1 if bf16 else 0, _ptr(out),
                                             nh * HD + 4, S0 + 4)
            finally:
                emu.hostemu_set_fiber_order(0)
            assert rc == 0, (form, S0, (emu.qtts_last_error() or b"").decode())
            outs.append((out, kk, vv))
        (oc, kc1, vc1), (op, kp1, vp1) = outs
        tag = (form, B, nh, S0, nsplit, order)
        assert np.isfinite(op).all() and np.all(op[:, nh * HD:] == 5.0), tag
        assert np.array_equal(bits(oc), bits(op)), (tag, "output differs from the contiguous form")
        for b in range(B):
            for i in range(need):       # the row's pages, the appended key included, are the contiguous row's -- bit for bit
                assert np.array_equal(bits(kp1[table[b, i]]), bits(kc1[b * pps + i])), (tag, b, i)
                assert np.array_equal(bits(vp1[table[b, i]]), bits(vc1[b * pps + i])), (tag, b, i)
            # ... and the append happened: slot S0 of the row's last page differs from the hole it held
            page, slot = table[b, S0 // 16], S0 % 16
            assert not np.array_equal(bits(kp1[page, :, slot]), bits(kp[page, :, slot])), (tag, b)
        for page in range(n_pages):     # nothing else was written: not the sink (no row idles here), not a page nobody holds
            if page not in granted:
                assert np.array_equal(bits(kp1[page]), bits(kp[page])) and np.array_equal(bits(vp1[page]), bits(vp_[page])), (tag, page)
        contiguous_out.append(oc[:, :nh * HD].copy())
    return contiguous_out


ORDERS = (0, 1, 2)


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("form", ["tk_bf16", "tk_f32", "tk16"])
def test_pooled_decode_attention_is_bit_identical_to_the_contiguous_form(emu, qopt, form, nsplit):
    """Every length under all three wave orders.  With 3 splits the split path must really have run: from 129 cached keys on (three
    chunks of 64 keys: at least two workgroups hold keys, and their partial results go through the merge kernel) the contiguous form's
    output is the one-workgroup output to rounding, not bit for bit."""
    qopt(emu, "QTTS_DEBUG_ATTN_VT", "1" if form == "tk16" else "0")
    split = lambda n: qopt(emu, "QTTS_DEBUG_ATTN_NSPLIT", str(n))
    split(nsplit)
    g = np.random.default_rng(4100 + nsplit + len(form))
    took_the_split_path = 0
    for n, S0 in enumerate(LENGTHS):
        pads = [0, min(S0 - 1, 5 + n)]                                               # GQA 2:1, a pad in row 1
        state = g.bit_generator.state
        outs = _case(emu, g, form, 2, 4, 2, S0, pads, [(nsplit, o) for o in ORDERS])
        assert all(np.array_equal(outs[0].view(np.uint32), o.view(np.uint32)) for o in outs[1:]), (form, S0, "the wave order changed the output")
        if nsplit > 1 and S0 >= 255:
            g.bit_generator.state = state                                            # the same case once more, in one workgroup
            split(1)
            one = _case(emu, g, form, 2, 4, 2, S0, pads, [(1, 0)])[0]
            split(nsplit)
            # (a sanity bound, not the property: fp32 sums of <= 257 terms of order 1; tk16 rounds every probability to bf16 against a
            # maximum that differs between the two runs -- 2^-8 of a V of order 1)
            assert np.allclose(one, outs[0], rtol=0, atol=2.0 ** -8 if form == "tk16" else 1e-4), (form, S0)
            took_the_split_path += not np.array_equal(one.view(np.uint32), outs[0].view(np.uint32))
    assert took_the_split_path == (3 if nsplit > 1 else 0), took_the_split_path
    for S0 in (17, 257):
        _case(emu, g, form, 2, 2, 2, S0, [3, 0], [(nsplit, o) for o in ORDERS])     # 1:1
