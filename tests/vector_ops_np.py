"""float64 / exact restatements of the flat-vector layer of the C ABI (test helper, not
collected): the slab reductions, the moments, the standardisation and the elementwise
update kernels of `include/mrl_hip.h`, each with the error bound its GPU test uses and
the input generators the GPU tests and the CPU separation checks share.

Every bound is derived from the arithmetic the header promises, never from what the
device returns.  Notation: u = 2^-53 (fp64 unit roundoff), u32 = 2^-24 (float32 unit
roundoff), gamma_k(u) = k u / (1 - k u) >= (1 + u)^k - 1 (Higham, Accuracy and Stability
of Numerical Algorithms, Lemma 3.1).

The library is compiled with the compiler's default contraction, so a device expression
`a + f * b` may be one fused operation: where that changes the result the reference lists
every admissible evaluation (`oracle.fma.fma` is a correctly rounded fma).
"""
import math

import numpy as np

from oracle import fma as F

U64 = 2.0 ** -53
U32 = 2.0 ** -24


def gamma(k, u=U64):
    return k * u / (1.0 - k * u)


# ------------------------------------------------------------------ inputs
def cancel_rows(rng, rows, cols):
    """Cancellation-heavy float32 slab [rows, cols]: per column rows//2 magnitudes drawn
    from U(0.5e6, 2e6), each present once with either sign and at shuffled positions,
    plus unit normal noise on every element (an odd row out holds noise only).  The
    running sums wander at 1e6 .. 1e7 while the column sum is O(sqrt(rows)): float32
    accumulation (ulp 0.06 .. 1 at those magnitudes) loses the result, fp64 does not.
    Every value is a multiple of 2^-10 (moments_ref relies on it)."""
    half = rows // 2
    mag = rng.uniform(0.5e6, 2e6, (half, cols))
    x = np.zeros((rows, cols))
    x[:half] = mag
    x[half:2 * half] = -mag
    x = rng.permuted(x, axis=0)
    return (x + unit_noise(rng, (rows, cols))).astype(np.float32)


def unit_noise(rng, shape):
    """Unit normal noise on the 2^-10 grid, float32."""
    return (np.rint(rng.standard_normal(shape) * 1024.0) / 1024.0).astype(np.float32)


def cancel_vec(rng, n):
    return cancel_rows(rng, n, 1)[:, 0].copy()


def shifted_normal(rng, n, mean):
    """float32 data of the given mean and unit standard deviation."""
    return (mean + rng.standard_normal(n)).astype(np.float32)


# ------------------------------------------------------------------ sums
def half_ulp32(v):
    """Half a float32 ulp at |v| (elementwise; normal range)."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    _, e = np.frexp(np.maximum(v, 2.0 ** -126))  # v = m 2^e, m in [0.5, 1): ulp = 2^(e-24)
    return np.ldexp(1.0, e - 25)


def fsum_cols(x):
    """Exact column sums of x [rows, cols] (math.fsum: one rounding of the exact sum)."""
    x = np.asarray(x, dtype=np.float64)
    return np.array([math.fsum(x[:, c]) for c in range(x.shape[1])])


def sum_bound(terms, abs_sum, exact=None):
    """|device - fsum| for a sum of `terms` exactly known fp64 values accumulated in fp64 in
    any fixed order: every partial sum is rounded once and each input passes through at most
    terms - 1 additions, so the error is at most gamma_{terms-1}(u) sum|x_i| <=
    terms 2^-53 sum|x_i| =: B (Higham, eq. 4.4 -- valid for every summation order, which is
    what lets one bound serve the 4-group, 16-group, narrow and grid-stride kernels).
    fsum's own rounding (u |s| <= u sum|x_i|) is covered by the slack between terms - 1 and
    terms.  exact given: the device then casts its fp64 sum d to float32, adding half a
    float32 ulp of d; |d| <= |exact| + B, so the half ulp is taken there (it equals half an
    ulp of the exact sum unless a power of two lies within B of it)."""
    b = terms * U64 * np.asarray(abs_sum, dtype=np.float64)
    if exact is not None:
        b = b + half_ulp32(np.abs(exact) + b)
    return b


def reduce_rows_ref(slab):
    """mrl_reduce_rows_*: out[c] = sum_r slab[r, c].  Returns (exact sums, sum |.|)."""
    s = np.asarray(slab, dtype=np.float64)
    return fsum_cols(s), np.abs(s).sum(axis=0)


def reduce_rows_bound(slab, cast32):
    s, a = reduce_rows_ref(slab)
    return sum_bound(np.asarray(slab).shape[0], a, s if cast32 else None)


def sum_rows_f32(slab):
    """The wrong twin: the same sums accumulated in float32, row after row."""
    acc = np.zeros(np.asarray(slab).shape[1], dtype=np.float32)
    for row in np.asarray(slab, dtype=np.float32):
        acc = acc + row
    return acc.astype(np.float64)


def sum_rows_pairwise(slab):
    """A right twin: fp64, adjacent pairs added level by level (not the device's order)."""
    s = [r for r in np.asarray(slab, dtype=np.float64)]
    while len(s) > 1:
        s = [s[i] + s[i + 1] if i + 1 < len(s) else s[i] for i in range(0, len(s), 2)]
    return s[0]


# ------------------------------------------------------------------ moments
def moments_ref(a, b=None, shift=0.0):
    """mrl_moments / mrl_moments_centered: (sum d, sum d^2, n) of d = a - b - shift, EXACT.
    a, b float32 multiples of 2^-10 below 2^23 (the generators above; checked): a - b is
    then exact in fp64; with b None any float32 a is (no difference is formed), so nothing
    is asked of it.  d = (a - b) - shift is held as the unevaluated
    pair hi + lo (TwoSum), d^2 = hi^2 + 2 hi lo + lo^2 with every product split exactly
    (Dekker), and math.fsum adds all the pieces with one rounding.
    Returns (s1, s2, sum |d|, sum d^2)."""
    d0 = np.asarray(a, dtype=np.float64) - (0.0 if b is None else np.asarray(b, dtype=np.float64))
    assert b is None or (np.all(np.rint(d0 * 1024.0) == d0 * 1024.0) and np.all(np.abs(d0) < 2.0 ** 24))
    hi, lo = F.two_sum(d0, np.full_like(d0, -float(shift)))
    s1 = math.fsum(np.concatenate([hi, lo]))
    pieces = []
    for (p, q) in ((hi, hi), (2.0 * hi, lo), (lo, lo)):
        pr, er = F.two_prod(p, q)
        pieces += [pr, er]
    s2 = math.fsum(np.concatenate(pieces))
    return s1, s2, float(np.abs(hi).sum()), s2


def moments_bounds(n, abs_sum, sq_sum):
    """Bounds of the two sums.  The device evaluates d in fp64 with at most two roundings
    ((a - b), then - shift) and d^2 with one more (or none: fused into the accumulation),
    so each term of the first sum carries (1 + u)^2 and of the second (1 + u)^5 before the
    n - 1 additions: gamma_{n+1}(u) sum|d| and gamma_{n+4}(u) sum d^2."""
    return gamma(n + 1) * abs_sum, gamma(n + 4) * sq_sum


def moments_f32(a, b=None, shift=0.0):
    """The wrong twin: float32 differences, squares and accumulators."""
    d = np.asarray(a, dtype=np.float32) - (np.float32(0) if b is None else np.asarray(b, dtype=np.float32))
    d = d - np.float32(shift)
    s1 = np.cumsum(d, dtype=np.float32)[-1]  # one running float32 sum each
    s2 = np.cumsum(d * d, dtype=np.float32)[-1]
    return float(s1), float(s2)


def moments_f64(a, b=None, shift=0.0):
    """A right twin: the header's expression in fp64 with numpy's (pairwise) sums."""
    d = np.asarray(a, dtype=np.float64) - (0.0 if b is None else np.asarray(b, dtype=np.float64)) - shift
    return float(np.sum(d)), float(np.sum(d * d))


# ------------------------------------------------------------------ standardize
def standardize_ref(x):
    """numpy's float64 (x - x.mean()) / x.std() on the float32 inputs (core.py:100-105)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (x - x.mean()) / x.std()


def standardize_two_pass(x, sum_fn=np.sum):
    """The device's two-pass form (standardize_kernel with cmoments) in fp64."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    mean0 = sum_fn(x) / n
    c = x - mean0
    d = sum_fn(c) / n
    var = max(sum_fn(c * c) / n - d * d, 0.0)
    return (x - (mean0 + d)) / np.sqrt(var)


def standardize_single_pass(x, sum_fn=np.sum):
    """The single-pass form E[x^2] - mean^2 from fp64 sums (cmoments == NULL)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    mean = sum_fn(x) / n
    var = max(sum_fn(x * x) / n - mean * mean, 0.0)
    return (x - mean) / np.sqrt(var)


def standardize_slack(x, two_pass=True):
    """fp64 part of the tolerance: how far the device's fp64 z = (x - mean) / std and
    numpy's may sit from the exact value, elementwise.  With m, s the exact mean and
    standard deviation and E|.| a mean absolute value:

    two-pass: mean = mean0 + d where mean0 is ANY shift near the mean (its own error only
      moves the centre) and d = sum(x - mean0) / n: per term one rounding, n - 1 additions,
      the division and the final sum -> |dmean| <= gamma_{n+1} E|x - mean0| + u |m|.
      var = sum (x - mean0)^2 / n - d^2 has no cancellation (d^2 <= var 1e-20 here):
      |dvar| / var <= gamma_{n+6}; the square root halves it and adds u.
    single-pass: |dmean| <= gamma_n E|x|; var = E[x^2] - mean^2 carries gamma_{n+1} E[x^2]
      + 2 |m| |dmean| + 2 u m^2 of absolute error -- small only while |m| <~ s (the
      cancellation the header documents).
    z: the subtraction and the division round once each (2 u |z|).
    numpy's reference: pairwise sums, at most 8-way unrolled blocks of 128 then a binary
      tree: fewer than 16 + 3 + log2(n / 128 + 1) + 2 roundings per term, i.e. gamma_k with
      k = 24 + log2(n) in place of gamma_n above, and two-pass.
    The returned slack is the device's bound plus the reference's."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    m = math.fsum(x) / n
    c = x - m
    var = math.fsum(c * c) / n
    s = math.sqrt(var)
    z = np.abs(c) / s
    eabs_c = math.fsum(np.abs(c)) / n

    def part(gn, single):
        if single:
            ex2 = math.fsum(x * x) / n
            dmean = gn(0) * math.fsum(np.abs(x)) / n
            dvar = gn(1) * ex2 + 2.0 * abs(m) * dmean + 2.0 * U64 * m * m
        else:
            dmean = gn(1) * eabs_c + U64 * abs(m)
            dvar = gn(6) * var
        rel_s = 0.5 * dvar / var + U64
        return dmean / s + z * (rel_s + 2.0 * U64)

    dev = part(lambda k: gamma(n + k), not two_pass)
    ref = part(lambda k: gamma(24 + math.ceil(math.log2(n)) + k), False)
    return 1.01 * (dev + ref)  # 1.01: the second-order terms dropped above


def standardize_bound(x, two_pass=True):
    """Tolerance of mrl_standardize against standardize_ref, elementwise.  Two roundings
    separate the device's float32 output from the exact standardized value z:
      1. the cast of its fp64 result to float32: half a float32 ulp of that result, i.e. at
         most (1/2) eps32 |z| with eps32 = 2^-23 -- the multiple is 1/2, taken on the
         binade of z (half_ulp32), not rounded up to the next power of two;
      2. the fp64 evaluation before the cast (standardize_slack, ~1e-10 for the two-pass
         form at n = 5e5): it shifts the value that is cast, so it is added once outside
         and once inside the half ulp.
    Nothing looser separates the two forms: with fp64 sums the single-pass form at
    |mean| / std = 1e4 is off by ~1e-8 |z|, a twelfth of eps32 -- it shows only as casts
    that land one float32 apart from the right one, which a half-ulp tolerance rejects and
    a whole-eps32 one would not."""
    z = standardize_ref(x)
    sl = standardize_slack(x, two_pass)
    return half_ulp32(np.abs(z) + sl) + sl


# ------------------------------------------------------------------ elementwise
def cast_scale_ref(a, scale):
    """mrl_cast_scale_f32_f64: one fp64 product -- bit for bit."""
    return float(scale) * np.asarray(a, dtype=np.float32).astype(np.float64)


def gather_rows_ref(src_rows, idx):
    """mrl_gather_rows: a copy -- bit for bit."""
    return np.asarray(src_rows)[np.asarray(idx)]


def linesearch_ref(a, b, k0, K):
    """mrl_linesearch_candidates: out[k] = (float)(a + 2^-(k0+k) b).  The factor is a power
    of two, so the product is exact (no underflow: |b| >= 2^-900 or zero) and the fused and
    unfused forms are the same single rounding of the sum -- bit for bit."""
    a64 = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.stack([np.float32(a64 + 2.0 ** -(k0 + k) * b) for k in range(K)])


def axpy_cast_refs(a, b, frac):
    """mrl_axpy_cast: the float32 casts of the two admissible fp64 evaluations of
    a + frac * b (unfused, fused)."""
    a64 = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float64)
    return [np.float32(a64 + frac * b), np.float32(F.fma(np.full_like(b, frac), b, a64))]


def vf_target_refs(ret, vp, mixfrac):
    """mrl_vf_target: y = (float)(ret * mixfrac + vp * (1 - mixfrac)) in fp64: unfused, or
    either product fused into the sum (the other one rounded first)."""
    r = np.asarray(ret, dtype=np.float32).astype(np.float64)
    v = np.asarray(vp, dtype=np.float32).astype(np.float64)
    w = np.full_like(r, float(mixfrac))
    w1 = np.full_like(r, 1.0 - float(mixfrac))
    return [np.float32(r * w + v * w1), np.float32(F.fma(r, w, v * w1)), np.float32(F.fma(v, w1, r * w))]


def matches_one_of(out, refs):
    """Elementwise: out equals (bit for bit; float32 arrays of finite values) one of refs."""
    out = np.asarray(out, dtype=np.float32).view(np.uint32)
    ok = np.zeros(out.shape, dtype=bool)
    for r in refs:
        ok |= out == np.asarray(r, dtype=np.float32).view(np.uint32)
    return ok


def adam_ref(theta, g, m, v, a_t, beta1, beta2, eps):
    """mrl_adam_step (ppo.py:231-258) in fp64 on the float32 inputs and the float32-cast
    scalars: m' = b1 m + (1 - b1) g; v' = b2 v + (1 - b2) g^2;
    theta' = theta - a_t m' / (sqrt(v') + eps).  Returns (theta', m', v', bounds) with the
    bounds (dtheta, dm, dv) counting the float32 roundings (u32 = 2^-24 each, gamma_k(u32)
    for k of them) of the device's float32 evaluation, with or without contraction:

    m': (1 - b1) [1], b1 m [1], (1 - b1) g [1], the sum [1].  The second term carries 3, the
        first 2: dm <= gamma_3 (|b1 m| + |(1 - b1) g|) =: gamma_3 M.
    v': g g [1], (1 - b2) [1], their product [1], b2 v [1], the sum [1]: the second term
        carries 4, the first 2: dv <= gamma_4 (|b2 v| + |(1 - b2) g^2|) = gamma_4 v'
        (both terms are non-negative: no cancellation).
    theta': with den = sqrt(v') + eps and w = a_t m' / den: sqrtf halves v's relative error
        (2) and rounds [1], + eps [1]: den carries 4; a_t m' [1] and the division [1] (both
        correctly rounded: the compiler's default for float32 sqrt and division), and m'
        enters with its absolute error dm: dw <= a_t dm / den + gamma_6 |w|; the final
        subtraction rounds once, at most u32 (|theta| + |w|) to first order:
        dtheta <= gamma_1 |theta| + gamma_7 |w| + gamma_3 a_t M / den."""
    f = lambda t: np.asarray(t, dtype=np.float32).astype(np.float64)  # noqa: E731
    th, g, m, v = f(theta), f(g), f(m), f(v)
    a, b1, b2, e = (float(np.float32(s)) for s in (a_t, beta1, beta2, eps))
    t1, t2 = b1 * m, (1.0 - b1) * g
    m1 = t1 + t2
    v1 = b2 * v + (1.0 - b2) * (g * g)
    den = np.sqrt(v1) + e
    w = a * m1 / den
    M = np.abs(t1) + np.abs(t2)
    dm = gamma(3, U32) * M
    dv = gamma(4, U32) * v1
    dth = gamma(1, U32) * np.abs(th) + gamma(7, U32) * np.abs(w) + gamma(3, U32) * a * M / den
    return th - w, m1, v1, (dth, dm, dv)


# ------------------------------------------------------------------ CG early exit
def three_eigen_system(n, seed):
    """Diagonal operator with exactly three distinct eigenvalues (1, 2, 4 by index mod 3;
    powers of two, so the float32 product d * p32 is exact) and b with unit-scale normal
    weight on every coordinate, hence comparable weight on each eigenspace (n >= 3).  In
    exact arithmetic CG on (A + damping I) stops after three iterations; the float32
    hand-off of p leaves rdotr at ~(2^-24)^2 of its start.  tol = 1e-8 b.b sits between
    rdotr after two iterations (>~ 1e-3 b.b) and after three (<~ 1e-13 b.b)."""
    rng = np.random.default_rng(seed)
    d = np.array([1.0, 2.0, 4.0])[np.arange(n) % 3]
    g = rng.standard_normal(n).astype(np.float32)
    b = -g.astype(np.float64)
    return d, g, b, 1e-8 * float(b.dot(b))
