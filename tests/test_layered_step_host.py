"""The CPU half of the layered rollout's step tests (tests/layered_step_cases.py,
tests/layered_step_np.py): the case tables reach every branch named here, the float32
restatement of every head route is inside the head bound and every wrong head outside it, the
merge restated in the device's chunked order agrees with the oracle's and every wrong merge does
not.  Nothing here runs on a device."""
import numpy as np
import pytest

from tests import layered_step_cases as C
from tests import layered_step_np as R

REQUIRED = {
    # every head route x operand mode, both alignment fallbacks, the second instantiation
    "head:runs8:f32", "head:runs8:bf", "head:runs8:b16", "head:runs4:f32", "head:runs4:bf", "head:runs4:b16",
    "head:strided:f32", "head:strided:bf", "head:strided:b16", "head:uint2_tail", "head:fallback_woff",
    "head:fallback_hoff", "head:whole_strides", "head:ragged_stride", "head:idle_lanes", "head:one_unit", "head:wpb1",
    "head:wpb4", "head:ragged_block", "head:blocks>1", "head:eval:runs8:f32", "head:eval:runs4:b16",
    "head:eval:strided:f32", "head:t0", "head:t1",
    # the record merge
    "merge:nb<=16", "merge:nb==16", "merge:nb>16", "merge:partial_last_chunk", "merge:one_block_last_chunk",
    "merge:state_empty", "merge:state_running", "merge:zero_count_reward", "merge:zero_count_block",
    # the obs kernel
    "obs:nvalid1", "obs:nvalid64", "obs:nvalid_ragged", "obs:blocks1", "obs:blocks>1", "obs:col_chunks1",
    "obs:col_chunks>1", "obs:reward_chunk_with_obs", "obs:ragged_last_chunk", "obs:parity0", "obs:parity1", "obs:t0",
    "obs:t1", "obs:t_last", "obs:var_n<=1", "obs:zero_variance", "obs:clip", "obs:filter0", "obs:filter1", "obs:twin",
    "obs:notwin", "obs:twin_padded", "obs:eval", "obs:eval:n>=2", "obs:eval:n<2",
    # the partials
    "rec:nvalid1", "rec:nvalid64", "rec:nvalid_ragged", "rec:blocks1", "rec:blocks>1", "rec:col_chunks1",
    "rec:col_chunks>1", "rec:reward_chunk_with_obs", "rec:reset", "rec:with_reward", "rec:m2_exact_zero",
    # the thread-per-env act
    "act:categorical", "act:gauss", "act:blocks1", "act:blocks>1", "act:full_block", "act:ragged_block",
}


def test_case_tables_reach_every_branch():
    seen = set()
    for c in C.HEAD + C.OBS + C.REC + C.ACT:
        seen |= C.branches(c)
    assert REQUIRED <= seen, sorted(REQUIRED - seen)
    for table in (C.HEAD, C.OBS, C.REC, C.ACT):
        assert len(set(table)) == len(table)
    # the issue's shapes, unpruned where it says so
    for nh in (256, 512):
        for mode in C.MODES:
            got = {(c.E, c.wpb) for c in C.HEAD if (c.nh, c.mode, c.align, c.ev) == (nh, mode, "al", 0)}
            assert got == {(E, w) for E in C.HEAD_E for w in (1, 4)}
            assert any((c.nh, c.mode, c.align) == (nh, mode, "mis") for c in C.HEAD)
    assert {c.nh for c in C.HEAD} == {512, 256, 128, 64, 200, 30, 1}
    assert {(c.nh, c.mode) for c in C.HEAD} == {(nh, m) for nh in (512, 256, 128, 64, 200, 30, 1) for m in C.MODES}
    assert all(c.align == "al" or c.nh in (256, 512) for c in C.HEAD)
    for env in C.ENVS:
        want = set(C.OBS_E) | (set(C.OBS_E_BIG) if env in ("CartPole-v0", "Humanoid-v2") else set())
        assert {c.E for c in C.OBS if c.env == env and not c.ev} == want
    # the geometry the names stand for
    assert [C.n_blocks(E) for E in C.OBS_E_BIG] == [16, 17, 33]
    assert {C.ENVS[e][0] + 1 for e in C.ENVS} == {5, 12, 18, 377} and 377 == 11 * 32 + 24 + 1
    assert max(c.t for c in C.HEAD) < C.HEAD_T <= 2 and max(c.t for c in C.OBS) == C.OBS_T - 1


def test_head_bound_is_from_the_operation_count():
    assert [R.head_chain(nh) for nh in (1, 30, 64, 128, 200, 256, 512)] == [8, 8, 8, 9, 11, 11, 15]
    assert R.gamma(15) == pytest.approx(15 * 2.0 ** -24, rel=1e-6)


def test_exact_fma():
    """fma32 rounds a b + c once: cases where rounding the float64 sum again would differ."""
    f = np.float32
    one = np.array([1.0], dtype=np.float32)
    tie = R.fma32(np.array([f(2.0 ** -12)]), np.array([f(2.0 ** -12)]), one)  # exactly 1 + 2**-24: ties to even
    assert tie[0] == f(1.0)
    # c + 2**-14 - 2**-50 with c = 2**10 + 2**-13 (odd): below the tie, so c; the float64 sum alone
    # lands on the tie c + 2**-14 and would then go to even, c + 2**-13
    c = np.array([2.0 ** 10 + 2.0 ** -13], dtype=np.float32)
    a, b = np.array([2.0 ** -7 * (1 + 2.0 ** -18)], dtype=np.float32), np.array([2.0 ** -7 * (1 - 2.0 ** -18)], dtype=np.float32)
    assert np.float32(a.astype(np.float64) * b + c)[0] != c[0]
    dn = R.fma32(a, b, c)
    assert dn.dtype == np.float32 and dn[0] == c[0]
    rng = np.random.default_rng(0)
    x, y, z = (rng.standard_normal(1000).astype(np.float32) for _ in range(3))
    from fractions import Fraction
    got = R.fma32(x, y, z)
    for i in range(0, 1000, 7):
        exact = Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i]))
        lo, hi = np.nextafter(got[i], f(-np.inf)), np.nextafter(got[i], f(np.inf))
        assert abs(Fraction(float(got[i])) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))


@pytest.mark.parametrize("nh", (512, 256, 128, 64, 200, 30, 1))
def test_head_restatement_inside_and_twins_outside(nh):
    """Per head case: the float32 restatement of each route the case takes is inside the bound
    (its worst error / bound ratio is printed); every wrong twin that applies is outside it."""
    worst, names = {}, set()
    for c in [c for c in C.HEAD if c.nh == nh]:
        want, bound = R.head_reference(c)
        for _, woff, hoff in C.head_variants(c):
            route = C.head_route(c.nh, woff == 0 and hoff == 0)
            z = R.head_restated(c, route)
            assert z.dtype == np.float32 and not R.head_outside(c, z), C.case_id(c)
            key = (route, c.mode)
            worst[key] = max(worst.get(key, 0.0), float((np.abs(z - want) / bound).max()))
        for name, z in R.head_twins(c):
            names.add(name)
            assert R.head_outside(c, z), (C.case_id(c), name)
    print("head restatement, worst error / bound:", {k: round(v, 3) for k, v in sorted(worst.items())})
    assert all(v < 1.0 for v in worst.values())
    want = {"last unit dropped", "a unit counted twice", "bias omitted", "row E - 1 used for every env",
            "operands not rounded", "truncation instead of round-to-nearest-even", "only the rows rounded",
            "only the head kernel rounded"} | ({"head kernel read as [A, nh]"} if nh > 1 else set())
    assert names == want, names ^ want


def test_routes_differ_in_bits():
    """The two routes of one width sum in different orders: their float32 results differ
    somewhere, which is what lets the GPU test tell the alignment fallback from the runs."""
    for c in C.HEAD:
        if c.align == "mis":
            a = R.head_restated(c, C.head_route(c.nh, True))
            b = R.head_restated(c, "strided")
            assert not np.array_equal(a.view(np.uint32), b.view(np.uint32)), C.case_id(c)


@pytest.mark.parametrize("i", range(len(C.OBS)), ids=[C.case_id(c) for c in C.OBS])
def test_merge_restatement_passes_and_twins_fail(i):
    c = C.OBS[i]
    o = R.obs_operands(c)
    fs, rows = R.obs_reference(c, o)
    assert rows.shape == (c.E, o.O) and np.isfinite(rows).all()
    if c.filt:
        assert rows.max() == 5.0 and (c.E == 1 or rows.min() == -5.0)
    if c.ev:
        assert fs is None
        return
    assert R.state_close(R.merge_restated(c, o), fs)
    for twin in R.MERGE_TWINS:
        if R.merge_twin_applies(c, twin):
            assert not R.state_close(R.merge_restated(c, o, twin), fs), twin
    D, kc = o.D, C.const_column(c.env)
    if kc is not None:  # the zero-variance column: S exactly 0, the row two denominators out
        assert fs[2 + D + kc] == 0.0 and fs[2 + kc] == R.CONST
        if c.filt and not (c.state == "empty" and c.E == 1):
            assert abs(rows[0, kc] - 2.0) < 1e-6
    if c.t == 0:  # the reward column did not merge
        assert fs[1] == o.fs[o.rd, 1] and fs[2 + o.O] == o.fs[o.rd, 2 + o.O]
    assert fs[0] == o.fs[o.rd, 0] + c.E - (C.BLOCK if C.zero_block(c.E) is not None else 0)


def test_every_merge_twin_applies_somewhere():
    for twin in R.MERGE_TWINS:
        assert any(R.merge_twin_applies(c, twin) for c in C.OBS), twin


def test_block_records_and_categorical_rule():
    rng = np.random.default_rng(3)
    raw = rng.standard_normal((130, 5))
    rec = R.block_records(raw, True)
    assert rec.shape == (3, 12) and list(rec[:, 0]) == [64, 64, 2] and list(rec[:, 1]) == [64, 64, 2]
    np.testing.assert_allclose(rec[2, 2:7], raw[128:].mean(0), rtol=1e-14)
    np.testing.assert_allclose(rec[0, 7:], ((raw[:64] - raw[:64].mean(0)) ** 2).sum(0), rtol=1e-13)
    assert np.all(R.block_records(raw[:1], False)[0, 7:] == 0.0) and R.block_records(raw[:1], False)[0, 1] == 0
    p = np.array([[0.25, 0.75], [0.5, 0.5], [0.1, 0.9], [0.3, 0.7]] * 2, dtype=np.float32)
    u = R.edge_uniforms(p)
    act = R.categorical_action(p, u)
    # below p0 -> 0; above p0 -> 1; u = 0 -> 0; 1 - 2**-53 -> 1 (the sum is 1.0); then the same
    # edges on the second running sum: below 1 -> 1, above 1 -> none exceeds -> 0
    assert list(act) == [0, 1, 0, 1, 1, 0, 0, 1]
