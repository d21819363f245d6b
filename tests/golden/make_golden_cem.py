"""Generate tests/golden/cem.npz from the REFERENCE's own ``cem`` generator.

Runs only where the reference checkout exists.  ``modular_rl/cem.py`` cannot be imported
(its ``from .core import *`` pulls Theano / Keras), so the ``cem`` function and the
``CEM_OPTIONS`` table are AST-extracted from the file at run time and executed with numpy
alone, as make_golden.py does.  The reference's ``map`` path (``np.array(map(f, ths))``)
does not work on Python 3, so the function runs with a stand-in pool whose ``map`` is a list
comprehension -- the reference's own ``pool.map`` branch.

Objective: a fixed quadratic; ``np.random.seed`` fixed.  Two configurations, P = 7, batch 24,
6 iterations, elite_frac 0.25: extra_std 0, and extra_std 0.5 with std_decay_time 3.  Stored
per iteration: the population (the objective's recorded arguments), ys, th, std, ymean; and
the option table's names and defaults.

Usage:  python tests/golden/make_golden_cem.py
"""
import ast
import contextlib
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/modular_rl/cem.py"


def extract():
    tree = ast.parse(open(REF).read())
    keep = [n for n in tree.body
            if (isinstance(n, ast.FunctionDef) and n.name == "cem")
            or (isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "CEM_OPTIONS")]
    assert len(keep) == 2
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), REF, "exec"), ns)
    return ns["cem"], ns["CEM_OPTIONS"]


class Pool:
    def map(self, f, xs):
        return [f(x) for x in xs]


def run(cem, seed, P, batch, n_iter, elite_frac, initial_std, extra_std, std_decay_time):
    rng = np.random.RandomState(1234)
    target = rng.randn(P)
    scale = 0.5 + rng.rand(P)
    calls = []

    def f(th):
        calls.append(np.array(th, dtype=np.float64))
        return -float(np.sum(scale * np.square(th - target)))

    th0 = np.zeros(P)
    np.random.seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        infos = list(cem(f, th0, batch, n_iter, elite_frac, initial_std, extra_std, std_decay_time, pool=Pool()))
    pops = np.array(calls).reshape(n_iter, batch, P)
    ys = np.array([i["ys"] for i in infos])
    for g in range(n_iter):
        assert len(np.unique(ys[g])) == batch, "tied ys: the reference's tie order is unspecified"
    return dict(pops=pops, ys=ys, th=np.array([i["th"] for i in infos]), std=np.array([i["std"] for i in infos]),
                ymean=np.array([i["ymean"] for i in infos]), th0=th0,
                cfg=np.array([batch, n_iter, elite_frac, initial_std, extra_std, std_decay_time], dtype=np.float64))


def main():
    cem, options = extract()
    out = {}
    for tag, extra_std, decay in (("a", 0.0, 1.0), ("b", 0.5, 3.0)):
        for k, v in run(cem, 7, 7, 24, 6, 0.25, 1.0, extra_std, decay).items():
            out[f"{tag}_{k}"] = v
    out["option_names"] = np.array([o[0] for o in options])
    out["option_types"] = np.array([o[1].__name__ for o in options])
    out["option_defaults"] = np.array([float(o[2]) for o in options])
    np.savez(os.path.join(HERE, "cem.npz"), **out)
    print("wrote cem.npz:", {k: np.shape(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
