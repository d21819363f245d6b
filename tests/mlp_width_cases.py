"""Cases, float64 references, per-entry scales and bounds of the fused 64-wide MLP kernels
along their WIDTH axes (tests/test_mlp_widths_host.py on the CPU, tests/test_gpu_mlp_widths.py
on the device): the input width O = n_in at every step of the input layer's k-steps and of
the cached VJP's dispatch, the head width A at the head's k-step and at MAX_OUT, and the
time-feature form (n_obs = n_in - 1 observation columns, the time feature at column n_obs).

The helper functions restate the host dispatch (csrc/mlp_layout.h, mlp_kernels.hip,
mlp_vjp16.hip, mlp_fisher.hip) so the host test can prove the case list reaches every
branch.  Every reference is float64 (oracle.trpo_np) and every output entry has a scale of
its own, computed from the reference alone: the sum of the absolute terms the entry is formed
from (|X|^T |ga1| for gW0), the absolute values carried through the chain, plus what the
entry inherits from the rounding of its factors h and 1 - h^2 (see S(q) below), so an entry
that is small by cancellation is still held to the size of its terms.

Bound.  ``f32_outputs`` restates the same computation in numpy float32 (f32 matmuls, the two
branches of ``tanh_fast``, csrc/mlp_device.h); FLOOR[output] is its largest distance from the
float64 reference in scale units over every case below, and the kernels are allowed
TOL = 4 x FLOOR: ulp-level differences of the device's v_exp_f32 / v_rcp_f32, FMA
contraction and another summation order (the margin of tests/test_gpu_head_rows.py).  An
entry whose scale is 0 must be exact.  Nothing here reads a device result."""
import functools
import math
from types import SimpleNamespace

import numpy as np

from oracle import trpo_np as T

F = np.float32
HEAD_IDS = {"linear": 0, "softmax": 1, "gauss": 2}
MAX_IN, MAX_OUT = 32, 8

O_EDGES = [1, 2, 3, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32]
A_EDGES = [1, 2, 4, 5, 7, 8]
EPT_NIN = [2, 5, 16, 17, 32]
NS = [1, 15, 16, 17, 31, 32, 33, 127, 128, 129]  # the 16-row tile, the 32-row tile, the 128-row block
GRID_N = 77                                      # two 32-row tiles and 13 rows; four 16-row tiles and 13
CORNERS = [(1, 1), (15, 4), (16, 5), (17, 8), (31, 8), (32, 8)]
BF16_N = 3001
EPT_LIMIT = 200.0
STATIC_POLICY = {(11, 3, "gauss"), (4, 2, "softmax")}  # csrc/mlp_layout.h STATIC_SHAPES 1 and 2


# ------------------------------------------------------------------ the host dispatch, restated
def ks0p(O):
    """mlp_dims: input-layer k-steps ceil(O / 2), rounded up to a multiple of 4."""
    return (((O + 1) // 2) + 3) & ~3


def vjp_kernel(O, cached):
    """mrl_mlp_vjp / launch_vjp16: the kernel a VJP of input width O takes."""
    if not cached or O % 16 == 0:
        return "vjp32"
    return "vjp16_wide" if O > 16 else "vjp16"


def ks2(A):
    """head k-steps of the VJP kernels: (A + 3) >> 2."""
    return (A + 3) >> 2


def fisher_hyb_fits(O, A, head):
    """mrl_mlp_fisher_hyb_fits: the static policy shapes only."""
    return (O, A, head) in STATIC_POLICY


def gh_of(A, head):
    return 2 * A if head == "gauss" else A


def grid_rows(n):
    """mrl_mlp_partial_rows / mrl_mlp_slab_rows below their caps: four per block of 128 rows."""
    return 4 * max(1, -(-(-(-n // 32)) // 4))


# ------------------------------------------------------------------ the case list
def heads_of(A):
    return ("gauss", "softmax", "linear") if A == 1 else ("gauss", "softmax")


GRID = [(head, O, A, GRID_N, False) for O in O_EDGES for A in A_EDGES for head in ("gauss", "softmax")]
CORNER_SHAPES = [(head, O, A) for O, A in CORNERS for head in heads_of(A)]
CORNER = [(head, O, A, n, False) for head, O, A in CORNER_SHAPES for n in NS]
EPT = [("linear", O, 1, n, True) for O in EPT_NIN for n in NS]
CASES = GRID + CORNER + EPT
# shapes (head, O, A, ept) -> the row counts they run at
SHAPES = {}
for _h, _O, _A, _n, _e in CASES:
    SHAPES.setdefault((_h, _O, _A, _e), []).append(_n)
BF16_SHAPES = [(head, O, A) for head, O, A in CORNER_SHAPES if head != "linear"]


def shape_id(s):
    return "-".join(str(int(v) if isinstance(v, bool) else v) for v in s)


BLOCKS = ("W0", "b0", "W1", "b1", "W2", "b2", "ls")


def block_slices(O, A, head):
    """name -> slice of the flat theta (Keras order: W0, b0, W1, b1, W2, b2, [logstd])."""
    sizes = [O * 64, 64, 64 * 64, 64, 64 * A, A, A if head == "gauss" else 0]
    out, off = {}, 0
    for name, s in zip(BLOCKS, sizes):
        if s:
            out[name] = slice(off, off + s)
        off += s
    return out


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def make_case(head, O, A, N, ept):
    """fp32 inputs of one case, keyed by the case.  theta: T.mlp_init plus noise (as
    tests/test_gpu_mlp._setup); G: the head-gradient rows the VJP is given, dense and
    structured (only row N - 1, only column A - 1 and, for gauss, column gh - 1); v: the
    Fisher product's tangent."""
    rng = np.random.default_rng([HEAD_IDS[head], O, A, N, int(ept)])
    spec = T.Spec(O, [64, 64], A, head)
    th = T.mlp_init(rng, spec.shapes, head == "gauss") + 0.05 * rng.standard_normal(spec.P)
    if head == "gauss":
        th[-A:] = 0.3 * rng.standard_normal(A)
    c = SimpleNamespace(head=head, O=O, A=A, N=N, ept=None, spec=spec, gh=gh_of(A, head), P=spec.P)
    c.th = _f32(th)
    n_obs = O - 1 if ept else O
    c.obs = _f32(rng.standard_normal((N, n_obs)))
    X = c.obs.astype(np.float64)
    if ept:
        c.ept = rng.integers(0, int(EPT_LIMIT), size=N).astype(np.int32)
        c.ept[N - 1] = int(EPT_LIMIT) - 1  # a time feature of the last row that is not small
        tf = (c.ept / EPT_LIMIT).astype(np.float32).astype(np.float64)  # the kernels' f32 time feature
        X = np.concatenate([X, tf[:, None]], axis=1)
    c.X = X
    c.G = {"dense": _f32(rng.standard_normal((N, c.gh)))}
    g = np.zeros((N, c.gh))
    g[N - 1, A - 1] = 1.0 + rng.random()
    if head == "gauss":
        g[N - 1, c.gh - 1] = -1.0 - rng.random()
    c.G["struct"] = _f32(g)
    c.v = _f32(rng.standard_normal(spec.P))
    for a in (c.th, c.obs, c.X, c.v, c.G["dense"], c.G["struct"]):
        a.setflags(write=False)
    return c


# ------------------------------------------------------------------ float64 reference and scales
# S(q) below: the size of the terms q is formed from, |q| included, such that a float32
# evaluation of q is off by a few ulp of S(q).  Its leading term is the sum of |terms| of the
# entry itself (|X|^T |ga1| for gW0); the rest is what the entry inherits from the rounding of
# its factors: a hidden unit h = tanh(a) near 0 by cancellation in a carries a's error
# (S(h) = |h| + (1 - h^2) S(a)), and the factor 1 - h^2 of a saturated unit carries h's
# (S(1 - h^2) = 1 + 2 |h| S(h)).  Without these a gW2 entry h2 * g of one row would be held
# to |h2| |g| although h2 itself is only known to ulp(S(a2)).
def _forward_scales(Ws, bs, acts):
    x, h1, h2 = acts
    Sh1 = np.abs(h1) + (1 - h1 ** 2) * (np.abs(x) @ np.abs(Ws[0]) + np.abs(bs[0]))
    Sh2 = np.abs(h2) + (1 - h2 ** 2) * (Sh1 @ np.abs(Ws[1]) + np.abs(bs[1]))
    Sd1, Sd2 = 1 + 2 * np.abs(h1) * Sh1, 1 + 2 * np.abs(h2) * Sh2
    return Sh1, Sh2, Sd1, Sd2


def _vjp_scale(Ws, bs, acts, Gz, SG):
    """S of every entry of T.mlp_vjp(acts, Gz), the rows Gz known to ulp(SG)."""
    x, h1, h2 = acts
    Sh1, Sh2, Sd1, Sd2 = _forward_scales(Ws, bs, acts)
    d1, d2 = 1 - h1 ** 2, 1 - h2 ** 2
    gh2 = Gz @ Ws[2].T
    Sa2 = (SG @ np.abs(Ws[2]).T) * d2 + np.abs(gh2) * Sd2
    gh1 = (gh2 * d2) @ Ws[1].T
    Sa1 = (Sa2 @ np.abs(Ws[1]).T) * d1 + np.abs(gh1) * Sd1
    return [np.abs(x).T @ Sa1, Sa1.sum(0), Sh1.T @ Sa2, Sa2.sum(0), Sh2.T @ SG, SG.sum(0)]


def vjp_reference(c, G):
    """(value [P], scale [P]) of sum_rows J^T G for head rows G [N, gh] (float64); the
    log-std slots are the column sums of G[:, A:]."""
    th = c.th.astype(np.float64)
    Ws, bs, _ = c.spec.split(th)
    _, acts = T.mlp_forward(c.spec, th, c.X)
    A = c.A
    val = T.mlp_vjp(c.spec, th, acts, G[:, :A])
    sc = _vjp_scale(Ws, bs, acts, G[:, :A], np.abs(G[:, :A]))
    if c.head == "gauss":
        val, sc = val + [G[:, A:].sum(0)], sc + [np.abs(G[:, A:]).sum(0)]
    return T.flatten(val), T.flatten(sc)


def _metric_rows(c, th, z, acts):
    """(gz, S(gz)) [N, A]: the KL-metric rows of T.fisher_vector_product along c.v."""
    N = c.N
    Ws, bs, logstd = c.spec.split(th)
    dWs, dbs, _ = c.spec.split(c.v.astype(np.float64))
    x, h1, h2 = acts
    Sh1, Sh2, Sd1, Sd2 = _forward_scales(Ws, bs, acts)
    d1, d2 = 1 - h1 ** 2, 1 - h2 ** 2
    da1 = x @ dWs[0] + dbs[0]
    Sdh1 = (np.abs(x) @ np.abs(dWs[0]) + np.abs(dbs[0])) * d1 + np.abs(da1) * Sd1
    dh1 = da1 * d1
    da2 = dh1 @ Ws[1] + h1 @ dWs[1] + dbs[1]
    Sdh2 = (Sdh1 @ np.abs(Ws[1]) + Sh1 @ np.abs(dWs[1]) + np.abs(dbs[1])) * d2 + np.abs(da2) * Sd2
    dz = (da2 * d2) @ Ws[2] + h2 @ dWs[2] + dbs[2]
    Sdz = Sdh2 @ np.abs(Ws[2]) + Sh2 @ np.abs(dWs[2]) + np.abs(dbs[2])
    if c.head == "gauss":
        w = 1.0 / np.exp(2 * logstd)[None, :] / N
        return dz * w, Sdz * w * (1 + 2 * np.abs(logstd))[None, :]
    Sz = Sh2 @ np.abs(Ws[2]) + np.abs(bs[2])
    p = T.softmax(z)
    Sp = p * (Sz + (p * Sz).sum(1, keepdims=True) + np.maximum(1.0, np.abs(np.log(p))))
    m = (p * dz).sum(1, keepdims=True)
    Sm = (p * Sdz + Sp * np.abs(dz)).sum(1, keepdims=True)
    return p * (dz - m) / N, (p * (Sdz + Sm) + Sp * np.abs(dz - m)) / N


@functools.lru_cache(maxsize=None)
def reference(head, O, A, N, ept):
    """name -> (float64 value, scale) of every output of the case: "z" [N, A], "prob"
    [N, A] (softmax), "vjp.dense" / "vjp.struct" [P], "fvp" [P] (policy heads)."""
    c = make_case(head, O, A, N, ept)
    th = c.th.astype(np.float64)
    Ws, bs, logstd = c.spec.split(th)
    z, acts = T.mlp_forward(c.spec, th, c.X)
    zs = np.abs(acts[2]) @ np.abs(Ws[2]) + np.abs(bs[2])  # sum_k |h2_k W2_ko| + |b2_o|
    r = {"z": (z, zs)}
    if head == "softmax":
        p = T.policy_prob(c.spec, th, c.X)
        # dp_i = p_i (dz_i - sum_j p_j dz_j), and the rounding of the exponent and the division
        r["prob"] = (p, p * (zs + (p * zs).sum(1, keepdims=True) + np.maximum(1.0, np.abs(np.log(p)))))
    for k, G in c.G.items():
        r["vjp." + k] = vjp_reference(c, G.astype(np.float64))
    if head != "linear":
        v = c.v.astype(np.float64)
        gz, Sg = _metric_rows(c, th, z, acts)
        sc = _vjp_scale(Ws, bs, acts, gz, Sg)
        if head == "gauss":
            sc.append(2.0 * np.abs(c.spec.split(v)[2]))
        r["fvp"] = (T.fisher_vector_product(c.spec, th, v, c.X), T.flatten(sc))
    for val, sc in r.values():
        val.setflags(write=False)
        sc.setflags(write=False)
    return r


# ------------------------------------------------------------------ float32 restatement
def tanh_fast_f32(x):
    """tanh_fast of csrc/mlp_device.h in numpy float32: the odd polynomial below 0.125, else
    1 - 2 / (exp(2|x|) + 1) with float32 exp and division (the fused multiply-adds as a
    multiply and an add)."""
    x = np.asarray(x, dtype=np.float32)
    ax, x2 = np.abs(x), x * x
    q = x2 * F(-0.0539682545) + F(0.133333340)
    q = x2 * q + F(-0.333333343)
    q = x2 * q + F(1.0)
    with np.errstate(over="ignore"):
        e = np.exp(F(2.0) * ax)
    t = F(1.0) - F(2.0) * (F(1.0) / (e + F(1.0)))
    return np.where(ax < F(0.125), x * q, np.copysign(t, x)).astype(np.float32)


def _softmax_f32(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _vjp_f32(Ws, acts, G, A, gauss):
    x, h1, h2 = acts
    Gz = np.ascontiguousarray(G[:, :A])
    ga2 = (Gz @ Ws[2].T) * (F(1) - h2 * h2)
    ga1 = (ga2 @ Ws[1].T) * (F(1) - h1 * h1)
    out = [x.T @ ga1, ga1.sum(0), h1.T @ ga2, ga2.sum(0), h2.T @ Gz, Gz.sum(0)]
    if gauss:
        out.append(G[:, A:].sum(0))
    return T.flatten(out)


def f32_outputs(c):
    """The outputs of ``reference`` computed in float32 throughout."""
    Ws, bs, logstd = c.spec.split(c.th)
    x = _f32(c.X)
    h1 = tanh_fast_f32(x @ Ws[0] + bs[0])
    h2 = tanh_fast_f32(h1 @ Ws[1] + bs[1])
    z = h2 @ Ws[2] + bs[2]
    acts, A, N, gauss = (x, h1, h2), c.A, c.N, c.head == "gauss"
    r = {"z": z}
    if c.head == "softmax":
        r["prob"] = _softmax_f32(z)
    for k, G in c.G.items():
        r["vjp." + k] = _vjp_f32(Ws, acts, G, A, gauss)
    if c.head != "linear":
        dWs, dbs, dls = c.spec.split(c.v)
        dh1 = (x @ dWs[0] + dbs[0]) * (F(1) - h1 * h1)
        dh2 = (dh1 @ Ws[1] + h1 @ dWs[1] + dbs[1]) * (F(1) - h2 * h2)
        dz = dh2 @ Ws[2] + h2 @ dWs[2] + dbs[2]
        inv_n = F(1.0 / N)
        if gauss:
            sd = np.exp(logstd)
            G = np.concatenate([dz / (sd * sd)[None, :] * inv_n, np.repeat((F(2) * dls * inv_n)[None, :], N, axis=0)],
                               axis=1)
        else:
            p = _softmax_f32(z)
            G = p * (dz - (p * dz).sum(1, keepdims=True)) * inv_n
        r["fvp"] = _vjp_f32(Ws, acts, _f32(G), A, gauss)
    return r


# ------------------------------------------------------------------ distances and bounds
def distance(got, want, scale):
    """The largest |got - want| / scale over the entries; inf where an entry of scale 0 is
    not exact or a value is not finite."""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != want.shape or not np.isfinite(got).all():
        return math.inf
    err = np.abs(got - want)
    pos = scale > 0
    if np.any(err[~pos] != 0):
        return math.inf
    return float(np.max(err[pos] / scale[pos])) if pos.any() else 0.0


def distances(c, name, got, ref):
    """FLOOR key -> distance of output ``name`` ("z", "prob", "fvp", "vjp.dense" ...): the
    flat gradients per parameter block."""
    want, scale = ref[name]
    kind = name.split(".")[0]
    if kind in ("z", "prob"):
        return {kind: distance(got, want, scale)}
    got = np.asarray(got, dtype=np.float64)
    return {f"{kind}.{b}": distance(got[s], want[s], scale[s]) for b, s in block_slices(c.O, c.A, c.head).items()}


def round_up2(v):
    """v rounded up to two significant digits."""
    if v <= 0:
        return 0.0
    e = math.floor(math.log10(v)) - 1
    return float(f"{math.ceil(v / 10 ** e - 1e-9) * 10 ** e:.1e}")


def measure_floors():
    """FLOOR recomputed: the float32 restatement against the float64 reference over CASES."""
    worst = {}
    for key in CASES:
        c, ref = make_case(*key), reference(*key)
        for name, got in f32_outputs(c).items():
            for k, d in distances(c, name, got, ref).items():
                worst[k] = max(worst.get(k, 0.0), d)
    return worst


# measure_floors() on the CPU, rounded up to two digits (numpy 2.2)
FLOOR = {
    "z": 2.1e-07, "prob": 9.3e-08,
    "vjp.W0": 8.7e-08, "vjp.b0": 8.6e-08, "vjp.W1": 2.5e-07, "vjp.b1": 6.4e-08, "vjp.W2": 1.1e-07, "vjp.b2": 1.1e-07,
    "vjp.ls": 1.4e-07,
    # the Fisher product's scale carries the JVP's absolute terms through the metric and the
    # VJP: about 100 x the entries' own size, and the floors are as much lower
    "fvp.W0": 7.9e-10, "fvp.b0": 7.9e-10, "fvp.W1": 3.8e-09, "fvp.b1": 2.5e-09, "fvp.W2": 5.8e-10, "fvp.b2": 2.0e-09,
    "fvp.ls": 1.9e-06,
}
TOL = {k: 4.0 * v for k, v in FLOOR.items()}
STD_RTOL = 2e-5  # the DiagGauss std columns exp(logstd): the bound of test_gpu_mlp.test_forward_prob


def within(c, name, got, ref):
    """[] or the (key, distance, bound) of every block of ``got`` beyond TOL."""
    return [(k, d, TOL[k]) for k, d in distances(c, name, got, ref).items() if not d <= TOL[k]]
