"""Plain-Python, sequential restatement of the global regression that include/jda.h defines under "a stage's global
regression" (test infrastructure, not product; nothing under jda_amd/ imports it), written from that text: the shuffle on
the counter-based SplitMix64 generator, the 64 strided partial sums of dot with their six pairing steps, and the dual
coordinate descent of one coordinate.  Python floats are IEEE doubles and Python evaluates one operation at a time: this
is the bit-level yardstick.  sequential_dot=True adds the K terms one after the other instead (liblinear's order) -- used
only by the control that the pinned order is visible in the bits."""
import math

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


def splitmix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def shuffle(index, seed, it):
    """jdaFitShuffleCpp, in place: for s = 0 .. n-1: t = s + r(it, s) % (n - s), swap."""
    n = len(index)
    base = splitmix64(seed + (it + 1) * G)
    for s in range(n):
        t = s + splitmix64(base + (s + 1) * G) % (n - s)
        index[s], index[t] = index[t], index[s]
    return index


def dot(w, row, sequential=False):
    if sequential:
        acc = 0.
        for k in row:
            acc = acc + w[k]
        return acc
    p = [0.] * 64
    for k, at in enumerate(row):                      # p[c]: k = c, c + 64, .. ascending
        p[k & 63] = p[k & 63] + w[at]
    h = 32
    while h >= 1:
        for c in range(h):
            p[c] = p[c] + p[c + h]
        h >>= 1
    return p[0]


def fit(lbf, residual, leaf_n, rows=None, C=0., eps=0., max_iter=0, seed=0, sequential_dot=False):
    """lbf [n][K] ints, residual [n][dim] floats (lists or arrays) -> (w [K * leaf_n][dim], iters [dim], gnorm1 [2][dim])."""
    n = len(lbf)
    rows = list(range(n)) if rows is None else [int(r) for r in rows]
    nr = len(rows)
    K = len(lbf[0]) if n else 0
    dim = len(residual[0]) if n else 0
    f = K * leaf_n
    w = [[0.] * dim for _ in range(f)]
    iters = [0] * dim
    gn = [[0.] * dim, [0.] * dim]
    if nr == 0:
        return w, iters, gn
    C = C if C > 0 else 1. / nr
    eps = eps if eps > 0 else 0.0001
    max_iter = max_iter if max_iter > 0 else 1000
    lam = 0.5 / C
    H = float(K) + lam
    X = [[int(v) for v in lbf[r]] for r in rows]
    # ONE index array shared by the coordinates: epoch e's order does not depend on the coordinate
    orders, index = [], list(range(nr))
    for j in range(dim):
        y = [float(residual[r][j]) for r in rows]
        beta = [0.] * nr
        wj = [0.] * f
        it = 0
        init = last = 0.
        while it < max_iter:
            if it == len(orders):
                orders.append(list(shuffle(index, seed, it)))
            gnorm = 0.
            for i in orders[it]:
                b = beta[i]
                Gv = -y[i] + lam * b
                Gv = Gv + dot(wj, X[i], sequential_dot)
                if b == 0:
                    viol = -Gv if Gv < 0 else (Gv if Gv > 0 else 0.)
                else:
                    viol = math.fabs(Gv)
                gnorm += viol
                Hb = H * b
                if Gv < Hb:
                    d = -Gv / H
                elif Gv > Hb:
                    d = -Gv / H
                else:
                    d = -b
                if math.fabs(d) < 1.0e-12:
                    continue
                nb = b + d
                d = nb - b
                beta[i] = nb
                if d != 0:
                    for at in X[i]:
                        wj[at] = wj[at] + d
            if it == 0:
                init = gnorm
            last = gnorm
            it += 1
            if gnorm <= eps * init:
                break
        iters[j] = it
        gn[0][j], gn[1][j] = init, last
        for k in range(f):
            w[k][j] = wj[k]
    return w, iters, gn


# ---- test data (shared by the host and the GPU tests) --------------------------------------------------------------------

def make_problem(seed, n, K, leaf_n, dim, noise=0.01):
    """Random leaves and y = X w* + noise: (lbf [n, K] int32, residual [n, dim] float64)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    lbf = (np.arange(K, dtype=np.int64)[None, :] * leaf_n + rng.integers(0, leaf_n, (n, K))).astype(np.int32)
    w_star = rng.standard_normal((K * leaf_n, dim)) * 0.05
    res = w_star[lbf].sum(1) + noise * rng.standard_normal((n, dim))
    return lbf, np.ascontiguousarray(res, np.float64)


def fit_arrays(lbf, residual, leaf_n, **kw):
    """fit() on numpy arrays -> numpy arrays in the dtypes and shapes Cascador.global_regression_cpp returns."""
    import numpy as np
    K, dim = lbf.shape[1], residual.shape[1]
    w, iters, gn = fit(lbf.tolist(), residual.tolist(), leaf_n, **kw)
    return (np.array(w, np.float64).reshape(K * leaf_n, dim), np.array(iters, np.int32), np.array(gn, np.float64).reshape(2, dim))


# the control case of tests/test_fit_host.py: (seed, n, K, depth, L) -- one of tests/test_fit.py's own cases
ORDER_CASE = (130, 24, 130, 3, 1)


# the end-to-end case of tests/test_fit.py; tests/test_fit_host.py checks on the CPU that the restated chain alone lowers the error
def e2e_inputs(seed=31, n=60, L=5):
    """The sample set of the end-to-end test of tests/test_fit.py: current shapes and ground truth a structured step away."""
    import numpy as np
    import train_ref
    d = train_ref.make_samples(seed, n, L, outside=0.0)
    rng = np.random.default_rng(seed)
    gt = d["shapes"] + rng.normal(0, 0.04, d["shapes"].shape) + 0.03
    return d, gt


def e2e_reference(d, gt, D, carts, L, Cv=10.0, max_iter=40, seed=9):
    import stage_ref
    import train_ref
    s = train_ref.ref_set(d)
    lbf = [stage_ref.gen_lbf(D, carts, s.patches[i], s.shapes[i]) for i in range(s.n)]
    res = (gt - d["shapes"]).tolist()
    w, iters, gn = fit(lbf, res, 1 << (D - 1), C=Cv, max_iter=max_iter, seed=seed)
    shapes, _ = stage_ref.stage_update(D, None, s, w, lbf=lbf)
    before = stage_ref.mean_error(gt.tolist(), d["shapes"].tolist(), L, [0], [1])
    after = stage_ref.mean_error(gt.tolist(), shapes, L, [0], [1])
    return lbf, w, iters, gn, shapes, before, after
