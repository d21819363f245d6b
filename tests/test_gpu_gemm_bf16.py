"""mrl_gemm_bf16 / mrl_gemm_bf16_tn (csrc/gemm_bf16*.hip) per entry at every kernel's tile edges,
layouts and epilogues, and mrl_cast_rows_bf16 / mrl_pack_w_bf16 bit for bit (cases, float64
references, scales and the bound: tests/gemm_bf16_cases.py; the CPU side:
tests/test_gemm_bf16_host.py).

Every operand is a view into an allocation whose guard rows, and whatever else the contract does
not promise, are NaN; C and the slabs start as a sentinel.  Per case: (a) the library's route
query equals the restated route at the device's CU count -- a case whose kernel the device cannot
run fails, it does not fall to the tiled kernel unnoticed; (b) ``within`` holds every entry to
its bound, the sentinel bit for bit and the valid entries free of NaN; (c) a second launch gives
the same bits; (d) every non-tiled kernel equals the tiled one bit for bit on the valid entries
(the TN 256 x 256 kernel: on the rows above the ones-row, slab by slab); (e) the largest error
per (kernel, epilogue, output type) is printed against TOL."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gemm_bf16_cases as C

pytestmark = pytest.mark.gpu


def _ncu(lib):
    n = ctypes.c_int32(0)
    assert lib.mrl_device_cu_count(ctypes.byref(n)) == 0
    return n.value


def _dev(host):
    if host is None:
        return None
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(host.dtype)
    t = torch.from_numpy(host.view(signed) if signed else host).cuda()
    assert t.data_ptr() % 256 == 0
    return t


def _set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


class Launch:
    """The device buffers and descriptor of one case."""

    def __init__(self, c):
        from modular_rl_amd import _lib
        self.c, L = c, C.layout(c)
        self.L, self.esz = L, 2 if c.bf else 4
        self.t = {name: _dev(getattr(L, name)) for name in ("A", "B", "A2", "B2", "bias", "H")}
        self.init = _dev(L.C)
        self.out = torch.empty_like(self.init)

        def p(name, off, size):
            return None if self.t[name] is None else ctypes.c_void_p(self.t[name].data_ptr() + size * off)

        cp = ctypes.c_void_p(self.out.data_ptr() + self.esz * L.c_off)
        if c.kind == "nn":
            self.entry = "mrl_gemm_bf16"
            self.desc = _lib.GemmBf16Desc(m=c.m, n=c.n, k=c.k, a=p("A", L.a_off, 2), lda=L.lda, bt=p("B", L.b_off, 2),
                                          ldb=L.ldb, a2=p("A2", L.a_off, 2), bt2=p("B2", L.b_off, 2), c=cp, ldc=L.ldc,
                                          c_bf16=c.bf, epilogue=C.EPIS.index(c.epi), bias=p("bias", L.bias_off, 4),
                                          h=p("H", L.h_off, 2), ldh=L.ldh, lds_limit=c.lds)
        else:
            self.entry = "mrl_gemm_bf16_tn"
            self.desc = _lib.GemmBf16TnDesc(m=c.m, n=c.n, k=c.k, a=p("A", L.a_off, 2), lda=L.lda, b=p("B", L.b_off, 2),
                                            ldb=L.ldb, ones_row=c.ones, splits=c.splits, slab=cp,
                                            slab_stride=L.slab_stride, ldc=L.ldc, lds_limit=c.lds)

    def route(self, lib):
        return getattr(lib, self.entry + "_route")(ctypes.byref(self.desc))

    def run(self, skip=None):
        """Launch into a C of sentinels; the buffer's bits on the host."""
        from modular_rl_amd._lib import call, stream
        self.out.copy_(self.init)
        call(self.entry, ctypes.byref(self.desc), None if skip is None else ctypes.c_void_p(skip.data_ptr()), stream())
        torch.cuda.synchronize()
        return self.out.cpu().numpy().view(np.uint16 if self.c.bf else np.uint32)


@pytest.mark.parametrize("group", list(C.GROUPS))
def test_gemm_bf16_per_entry(group, monkeypatch):
    from modular_rl_amd import _lib
    lib = _lib.load(require_gpu=True)
    ncu = _ncu(lib)
    worst = {}
    for c in C.GROUPS[group]:
        run, env = Launch(c), C.env_of(c)
        _set_env(monkeypatch, env)
        want = C.route(c, ncu, env)
        assert C.ROUTES[run.route(lib)] == want, (C.case_id(c), "the library routes the case elsewhere")
        assert C.family(want) == c.kernel or (c.kernel == "stream" and C.family(C.route(c, C.NCU, env)) == "tiled"), (
            C.case_id(c), "this device (%d CUs) cannot run the kernel the case was written for" % ncu)
        bits = run.run()
        assert C.within(c, bits) == [], C.case_id(c)
        assert np.array_equal(run.run(), bits), ("a second launch gave other bits", C.case_id(c))
        idx = C.valid_index(c)
        if C.family(want) != "tiled" and C.family(want) != "tn_tiled":
            _set_env(monkeypatch, C.TILED_ENV)
            assert C.family(C.ROUTES[run.route(lib)]) in ("tiled", "tn_tiled"), C.case_id(c)
            tiled = run.run()
            rows = slice(0, c.m - c.ones)  # the TN big kernel's ones-row sums in another order
            assert np.array_equal(tiled[idx][:, rows], bits[idx][:, rows]), ("not the tiled kernel's bits", C.case_id(c))
            assert C.within(c, tiled) == [], C.case_id(c)
        d = float(C.case_distance(c, C.to_values(c, bits[idx])).max())
        key = (c.kernel, c.epi, "bf16" if c.bf else "f32")
        worst[key] = max(worst.get(key, 0.0), d)
    for key in sorted(worst):
        print("mrl_gemm_bf16 %-14s %-8s %-5s %-4s largest error %.3g scale units  (TOL %.3g, 0: a-priori)" % (
            group, *key, worst[key], C.TOL[key[:2]]))


def test_k0_never_reaches_the_persistent_kernels(monkeypatch):
    """K = 0 (no K stage at all: 0 % 4 == 0) must not pass the 256 x 256 launcher's stage-count
    check; asserted on the route, not with a launch."""
    from modular_rl_amd import _lib
    lib = _lib.load(require_gpu=True)
    _set_env(monkeypatch, dict(C.TILED_ENV, MRL_GEMM_BIG_MIN_M=1, MRL_GEMM_STREAM_MIN_M=1))
    for dual in (0, 1):
        d = _lib.GemmBf16Desc(m=300, n=300, k=0, a=0x1000, lda=0, bt=0x1000, ldb=0, a2=0x1000 if dual else None,
                              bt2=0x1000 if dual else None, c=0x1000, ldc=300)
        assert C.ROUTES[lib.mrl_gemm_bf16_route(ctypes.byref(d))] == "tiled128_bk64"
        d.k = 128
        assert C.ROUTES[lib.mrl_gemm_bf16_route(ctypes.byref(d))] == "big"


def test_production_shapes_keep_streaming(monkeypatch):
    """The layered path's tall single products at Humanoid widths (K = 376 and 512 with lda =
    ld8(K)) still stream under the default thresholds; a hidden width of 300 runs tiled."""
    from modular_rl_amd import _lib
    lib = _lib.load(require_gpu=True)
    for k in C.DEFAULT_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, want in ((376, "stream384"), (512, "stream512"), (300, "tiled128_bk64"), (440, "tiled128_bk64")):
        d = _lib.GemmBf16Desc(m=40000, n=512, k=k, a=0x1000, lda=C.ld8(k), bt=0x1000, ldb=C.ld8(k), c=0x1000, ldc=512)
        assert C.ROUTES[lib.mrl_gemm_bf16_route(ctypes.byref(d))] == want, k


SKIP_CASES = [next(c for c in cases if c.bf == bf and c.k > 0 and C.family(C.route(c)) == c.kernel)
              for cases in (C.TILED, C.SMALL, C.STREAM, C.BIG) for bf in (0, 1)] + [C.TN_TILED[4], C.TN_BIG[2]]


@pytest.mark.parametrize("c", SKIP_CASES, ids=C.case_id)
def test_device_skip_flag(c, monkeypatch):
    """A device ``skip`` of 1 leaves every byte; a device 0 gives the bits of skip = NULL: once per
    kernel and output type."""
    from modular_rl_amd import _lib
    lib = _lib.load(require_gpu=True)
    _set_env(monkeypatch, C.env_of(c))
    run = Launch(c)
    assert C.family(C.ROUTES[run.route(lib)]) == c.kernel
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    assert np.array_equal(run.run(skip=flag), run.L.C)
    plain = run.run()
    assert C.within(c, plain) == []
    flag.zero_()
    assert np.array_equal(run.run(skip=flag), plain)


@pytest.mark.parametrize("big", [0, 1])
def test_tn_slabs_in_a_flat_parameter_slab(big, monkeypatch):
    """Two TN launches into one flat slab the way the layered VJP writes its weight gradients:
    slab_stride = P, layer l's [din + 1, dout] block (ldc = dout) at w_off[l], the next layer's
    block right behind its ones-row and a NaN gap between the slabs.  After both launches each
    block holds only its own layer's values, per slab, and the gap is untouched."""
    from modular_rl_amd import _lib
    from modular_rl_amd._lib import call, stream
    lib = _lib.load(require_gpu=True)
    monkeypatch.setenv("MRL_GEMM_TN_BIG", str(big))
    layers = [(256, 264), (264, 256)] if big else [(40, 33), (33, 9)]  # (din, dout)
    K, splits, gap = 100, 4, 5
    w_off = [0, (layers[0][0] + 1) * layers[0][1]]
    P = w_off[1] + (layers[1][0] + 1) * layers[1][1] + gap
    cases = [C.Case("tn", "tn_big" if big else "tn_tiled", din + 1, dout, K, 0, 0, "slab", 0, 1, splits, "tight", 0, 0)
             for din, dout in layers]
    S = C.dims(cases[0]).S
    flat = torch.full((S * P,), float("nan"), dtype=torch.float32, device="cuda")
    keep = []
    for c, off in zip(cases, w_off):
        L = C.layout(c)
        a, b = _dev(L.A), _dev(L.B)
        keep += [a, b]
        d = _lib.GemmBf16TnDesc(m=c.m, n=c.n, k=c.k, a=ctypes.c_void_p(a.data_ptr() + 2 * L.a_off), lda=L.lda,
                                b=ctypes.c_void_p(b.data_ptr() + 2 * L.b_off), ldb=L.ldb, ones_row=1, splits=splits,
                                slab=ctypes.c_void_p(flat.data_ptr() + 4 * off), slab_stride=P, ldc=c.n)
        assert C.ROUTES[lib.mrl_gemm_bf16_tn_route(ctypes.byref(d))] == ("tn_big" if big else C.route(c))
        call("mrl_gemm_bf16_tn", ctypes.byref(d), None, stream())
    torch.cuda.synchronize()
    got = flat.cpu().numpy().reshape(S, P)
    assert np.isnan(got[:, P - gap:]).all(), "the gap behind the last layer was written"
    for c, off in zip(cases, w_off):
        block = got[:, off:off + c.m * c.n].reshape(S, c.m, c.n)
        dist = C.distance(block, *C.reference(c))
        assert np.all(dist <= C.tol(c)), (C.case_id(c), dist.reshape(-1), C.tol(c).reshape(-1))


# ------------------------------------------------------------------ casts and packs
def _special_table():
    """float32 bit patterns at every rounding edge of the bf16 conversion."""
    u = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # exact ties: to even downwards, upwards, both signs
         0x3F808001, 0x3F807FFF, 0x3F817FFF, 0x3F818001,  # just off the ties
         0x00000000, 0x80000000,                          # +-0
         0x00000001, 0x80000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x00010000,  # f32 subnormals, ties among them
         0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,  # the largest finite values: the first three round to inf
         0x7F800000, 0xFF800000,                          # +-inf
         0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FBFFFFF, 0x7F80FFFF]  # NaNs, quiet and signalling, payload in the low half
    return np.array(u, dtype=np.uint32).view(np.float32)


def _same_bf16(got, want):
    """Bit for bit, except that a NaN need only be a NaN."""
    gn, wn = (got & 0x7FFF) > 0x7F80, (want & 0x7FFF) > 0x7F80
    return np.array_equal(gn, wn) and np.array_equal(got[~wn], want[~wn])


def test_rne_restatement_on_the_special_table():
    """The numpy restatement itself, against values worked by hand."""
    t = _special_table()
    want = [0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F80, 0x3F81, 0x3F82, 0x0000, 0x8000, 0x0000, 0x8000, 0x0080, 0x0000,
            0x0002, 0x0001, 0x7F80, 0xFF80, 0x7F80, 0x7F7F, 0x7F80, 0xFF80]
    got = C.rne_bits(t)
    assert list(got[:22]) == want
    assert np.all((got[22:] & 0x7FFF) > 0x7F80)


CAST_SHAPES = [(1, 1, 1, 1), (3, 27, 27, 32), (5, 27, 40, 27), (37, 130, 133, 136), (4100, 513, 515, 520)]


@pytest.mark.parametrize("rows,cols,ldx,ldy", CAST_SHAPES)
def test_cast_rows_bf16_bit_for_bit(rows, cols, ldx, ldy):
    """mrl_cast_rows_bf16 == RNE bit for bit on the special table and random values: ldx > cols,
    the padding cols..ldy written as zeros, the guard rows around y untouched, NaN input padding
    never copied; a single element and a size past the grid cap (rows ldy > 8192 x 256)."""
    from modular_rl_amd import _lib
    from modular_rl_amd._lib import call, stream
    _lib.load(require_gpu=True)
    rng = np.random.default_rng([rows, cols])
    x = np.full((rows + 2 * C.GUARD, ldx), np.nan, dtype=np.float32)
    v = (rng.standard_normal((rows, cols)) * 2.0 ** rng.integers(-20, 20, (rows, cols))).astype(np.float32)
    t = _special_table()
    v.reshape(-1)[:min(t.size, v.size)] = t[:min(t.size, v.size)]
    v.reshape(-1)[-min(t.size, v.size):] = t[:min(t.size, v.size)]  # the grid-stride tail too
    x[C.GUARD:C.GUARD + rows, :cols] = v
    dx = torch.from_numpy(x).cuda()
    y0 = np.full((rows + 2 * C.GUARD, ldy), C.SENT16, dtype=np.uint16)
    dy = torch.from_numpy(y0.view(np.int16)).cuda()
    call("mrl_cast_rows_bf16", ctypes.c_void_p(dx.data_ptr() + 4 * C.GUARD * ldx), rows, cols, ldx,
         ctypes.c_void_p(dy.data_ptr() + 2 * C.GUARD * ldy), ldy, stream())
    torch.cuda.synchronize()
    got = dy.cpu().numpy().view(np.uint16)
    want = y0.copy()
    want[C.GUARD:C.GUARD + rows, :cols] = C.rne_bits(v)
    want[C.GUARD:C.GUARD + rows, cols:] = 0
    assert _same_bf16(got, want)
    if rows * ldy > 8192 * 256:
        assert rows * ldy > 8192 * 256 + 256  # more than one grid-stride pass


@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("din,dout,pad", [(1, 1, 0), (27, 33, 5), (130, 17, 8), (2100, 520, 8)])
def test_pack_w_bf16_bit_for_bit(din, dout, pad, transpose):
    """mrl_pack_w_bf16, both transposes == RNE bit for bit: zero padding columns, guard rows
    untouched; one element, and a size past the grid cap (rows ld > 4096 x 256)."""
    from modular_rl_amd import _lib
    from modular_rl_amd._lib import call, stream
    _lib.load(require_gpu=True)
    rng = np.random.default_rng([din, dout, transpose])
    w = (rng.standard_normal((din, dout)) * 2.0 ** rng.integers(-20, 20, (din, dout))).astype(np.float32)
    t = _special_table()
    w.reshape(-1)[:min(t.size, w.size)] = t[:min(t.size, w.size)]
    w.reshape(-1)[-min(t.size, w.size):] = t[:min(t.size, w.size)]
    rows, cols = (dout, din) if transpose else (din, dout)
    ld = cols + pad
    wbuf = np.concatenate([np.full(4, np.nan, dtype=np.float32), w.reshape(-1), np.full(4, np.nan, dtype=np.float32)])
    dw = torch.from_numpy(wbuf).cuda()
    y0 = np.full((rows + 2 * C.GUARD, ld), C.SENT16, dtype=np.uint16)
    dy = torch.from_numpy(y0.view(np.int16)).cuda()
    call("mrl_pack_w_bf16", ctypes.c_void_p(dw.data_ptr() + 16), din, dout, transpose,
         ctypes.c_void_p(dy.data_ptr() + 2 * C.GUARD * ld), ld, stream())
    torch.cuda.synchronize()
    got = dy.cpu().numpy().view(np.uint16)
    want = y0.copy()
    want[C.GUARD:C.GUARD + rows, :cols] = C.rne_bits(w.T if transpose else w)
    want[C.GUARD:C.GUARD + rows, cols:] = 0
    assert _same_bf16(got, want)
