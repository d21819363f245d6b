"""mrl_gemm (csrc/gemm.hip) per entry at every tile edge, orientation, compute mode, epilogue
and layout (cases, float64 references, per-entry scales and the bound: tests/gemm_cases.py;
the CPU side: tests/test_gemm_host.py).

Every operand is a view into an allocation whose padding columns, guard rows and, for a
shifted base, leading float are NaN; C and the slabs start as a sentinel bit pattern.  After
each launch ``within`` holds (a) every entry to tol x its scale, scale-0 entries exactly, (b)
the sentinel bit for bit outside the valid entries and (c) the valid entries free of NaN; (d)
a second launch must give the same bits.  The largest error per (mode, epilogue) in scale
units is printed, against TOL."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gemm_cases as C

pytestmark = pytest.mark.gpu

MODE_ID = {"f32": 0, "bf16": 1, "split": 2}
EPI_ID = {"store": 0, "tanh": 1, "dtanh": 2, "slab": 3}
GROUPS = {
    "narrow-cover": C.NARROW_COVER,
    "wide-20353x70x40": [c for c in C.WIDE if c.m == 20353],
    "wide-20352x70x40": [c for c in C.WIDE if c.m == 20352],
    "wide-6785x300x33": [c for c in C.WIDE if c.m == 6785],
    "wide-7117x257x36": [c for c in C.WIDE if c.m == 7117 and not c.shift],
    "wide-7117x257x36-shifted": [c for c in C.WIDE if c.m == 7117 and c.shift],
    "slabs-wide": [c for c in C.SLABS if c.k == 1287],
    "slabs-narrow": [c for c in C.SLABS if c.k != 1287],
}
for _m, _n, _k, _pad in C.PRODUCT_SHAPES:
    for _o in C.ORIENTS:
        GROUPS["product-%dx%dx%d-%s%s" % (_m, _n, _k, "NT"[_o[0]], "NT"[_o[1]])] = [
            c for c in C.NARROW_PRODUCT if (c.m, c.at, c.bt) == (_m, *_o)]
assert sorted(c for g in GROUPS.values() for c in g) == sorted(C.CASES)


class Launch:
    """The device buffers and descriptor of one case."""

    def __init__(self, c):
        from modular_rl_amd import _lib
        self.c, L = c, C.layout(c)
        self.keep = {}

        def dev(name, off=0):
            host = getattr(L, name)
            if host is None:
                return None
            t = torch.from_numpy(host).cuda()
            assert t.data_ptr() % 256 == 0
            self.keep[name] = t
            return ctypes.c_void_p(t.data_ptr() + 4 * off)

        self.out = torch.empty(L.c_size, dtype=torch.int32, device="cuda")
        self.desc = _lib.GemmDesc(m=c.m, n=c.n, k=c.k, a=dev("A", L.offa), lda=L.lda, a_trans=c.at, ones_row=c.ones,
                                  b=dev("B", L.offb), ldb=L.ldb, b_trans=c.bt, epilogue=EPI_ID[c.epi], a2=dev("A2", L.offa),
                                  b2=dev("B2", L.offb), c=ctypes.c_void_p(self.out.data_ptr()), ldc=L.ldc, bias=dev("bias"),
                                  h=dev("H"), ldh=L.ldh, splits=c.splits, compute=MODE_ID[c.mode],
                                  slab_stride=L.slab_stride)

    def run(self, skip=None):
        """Launch into a C of sentinels; the buffer as uint32 on the host."""
        from modular_rl_amd._lib import call, stream
        self.out.fill_(int(C.SENT_BITS) - (1 << 32))
        call("mrl_gemm", ctypes.byref(self.desc), None if skip is None else ctypes.c_void_p(skip.data_ptr()), stream())
        torch.cuda.synchronize()
        return self.out.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("group", list(GROUPS))
def test_gemm_per_entry(group):
    """Every case of the group: the tile width the library reports is the restated one, the
    launch is ``within`` the bound with sentinels and padding untouched, and a second launch
    gives the same bits."""
    from modular_rl_amd import _lib
    lib = _lib.load(require_gpu=True)
    worst = {}
    for c in GROUPS[group]:
        run = Launch(c)
        assert lib.mrl_gemm_tile_n(ctypes.byref(run.desc)) == C.tile_n(c), c
        bits = run.run()
        assert C.within(c, bits.view(np.float32)) == [], C.case_id(c)
        assert np.array_equal(run.run(), bits), ("a second launch gave other bits", C.case_id(c))
        d = float(C.distance(bits.view(np.float32)[C.valid_index(c)], *C.reference(c)).max())
        worst[(c.mode, c.epi)] = max(worst.get((c.mode, c.epi), 0.0), d)
    for key in sorted(worst):
        print("mrl_gemm %-26s %-5s %-5s  largest error %.3g scale units  (TOL %.3g)" % (group, *key, worst[key], C.TOL[key]))


SKIP_CASES = [next(c for c in C.WIDE if (c.at, c.bt) == o and c.m == m and c.mode == "f32") for o in C.ORIENTS
              for m in (6785, 20352)] + [next(c for c in C.SLABS if c.m == 130 and c.ones and c.mode == "f32")]


@pytest.mark.parametrize("c", SKIP_CASES, ids=C.case_id)
def test_device_skip_flag(c):
    """A device ``skip`` of 1 leaves C untouched; a device 0 gives the bits of skip = NULL:
    once per orientation and tile width, and on the slab path."""
    from modular_rl_amd import _lib
    _lib.load(require_gpu=True)
    assert C.tile_n(c) == (32 if c.m == 20352 else 128)
    run = Launch(c)
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    assert np.all(run.run(skip=flag) == C.SENT_BITS)
    plain = run.run()
    assert C.within(c, plain.view(np.float32)) == []
    flag.zero_()
    assert np.array_equal(run.run(skip=flag), plain)
