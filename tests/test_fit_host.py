"""CPU-side checks of the global regression (include/jda.h, "Dialect CPP: a stage's global regression"): the host-only
shuffle against tests/fit_ref.py, every refusal that must come before the device is touched (with w under a canary),
n_rows == 0, and the CONTROLS of the yardstick of tests/test_fit.py -- the restated solver solves the problem it claims to
(against numpy's closed form of the primal), and on that test's own inputs a sequential dot changes bits of w, so "bit-exact
with the pinned dot" tests something."""
import ctypes as C

import numpy as np
import pytest

from conftest import same
import fit_ref
import stage_ref
import train_ref


def _cascador(model_file, L=5, D=3):
    from jda_amd import api
    p, _ = model_file((1, 2, L, D))
    return api.Cascador(p, "double")


def test_the_two_symbols_are_exported(built):
    from jda_amd import api
    for name in ("jdaGlobalRegressionCpp", "jdaFitShuffleCpp"):
        assert hasattr(api.lib, name), name


# ---- the shuffle -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 2, 64, 1000])
def test_shuffle_equals_the_restatement(built, n):
    from jda_amd import api
    seen = set()
    for seed in (0, 1, 0x9E3779B97F4A7C15, 2 ** 64 - 1):
        got = np.arange(n, dtype=np.int32)
        want = list(range(n))
        for it in range(4):                                                   # epochs chained on one array
            got = api.fit_shuffle_cpp(got, seed, it)
            fit_ref.shuffle(want, seed, it)
            assert same(got, np.array(want, np.int32))
            assert sorted(got.tolist()) == list(range(n))                     # a permutation
            seen.add((seed, it, tuple(got.tolist())))
    if n >= 64:
        assert len({p for _, _, p in seen}) == len(seen)                      # (seed, iter) changes it
        a = api.fit_shuffle_cpp(np.arange(n, dtype=np.int32), 5, 0)
        b = api.fit_shuffle_cpp(np.arange(n, dtype=np.int32), 5, 1)
        c = api.fit_shuffle_cpp(np.arange(n, dtype=np.int32), 6, 0)
        assert not same(a, b) and not same(a, c)


def test_shuffle_refuses_bad_arguments(built):
    from jda_amd import api
    ip = C.POINTER(C.c_int)
    a = np.arange(4, dtype=np.int32)
    assert api.lib.jdaFitShuffleCpp(None, 4, 0, 0) == -1 and api.last_error()
    assert api.lib.jdaFitShuffleCpp(a.ctypes.data_as(ip), -1, 0, 0) == -1
    assert api.lib.jdaFitShuffleCpp(a.ctypes.data_as(ip), 4, 0, -1) == -1
    assert same(a, np.arange(4, dtype=np.int32))
    assert api.lib.jdaFitShuffleCpp(None, 0, 0, 0) == 0


# ---- refusals and the empty problem ------------------------------------------------------------------------------------

def test_refusals_that_need_no_device(built, model_file):
    from jda_amd import api
    L, D, K, n = 5, 3, 4, 9
    leaf_n, dim = 1 << (D - 1), 2 * L
    c = _cascador(model_file, L, D)
    lbf, res = fit_ref.make_problem(1, n, K, leaf_n, dim)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)

    def refused(what, h=c.h, lbf=lbf, res=res, n=n, K=K, rows=None, n_rows=None, null_w=False):
        w = np.full((K * leaf_n if K > 0 else 1, dim), 7.25)
        it = np.full(dim, -3, np.int32)
        ra = None if rows is None else np.ascontiguousarray(rows, np.int32)
        rc = api.lib.jdaGlobalRegressionCpp(h, None if lbf is None else lbf.ctypes.data_as(ip), None if res is None else res.ctypes.data_as(dp),
                                            n, K, None if ra is None else ra.ctypes.data_as(ip), (n if ra is None else ra.size) if n_rows is None else n_rows,
                                            None, None if null_w else w.ctypes.data_as(dp), it.ctypes.data_as(ip), None, None)
        assert rc == -1 and what in api.last_error(), (rc, api.last_error())
        assert (w == 7.25).all() and (it == -3).all()                         # nothing was written

    refused("bad arguments", h=None)
    refused("K must be positive", K=0)
    refused("K must be positive", K=-2)
    refused("must not be negative", n=-1)
    refused("must not be negative", rows=[0, 1], n_rows=-1)
    refused("w must be given", null_w=True)
    refused("lbf and residual", lbf=None)
    refused("lbf and residual", res=None)
    refused("rows[2] is outside", rows=[0, 1, n])
    refused("rows[0] is outside", rows=[-1, 1])
    for i, k, v in ((0, 0, -1), (8, 3, 4 * leaf_n), (4, 1, 0), (4, 2, 3 * leaf_n)):
        bad = lbf.copy(); bad[i, k] = v
        refused("lbf[%d] is not a leaf of cart %d" % (i * K + k, k), lbf=bad)
        refused("lbf[%d] is not a leaf of cart %d" % (i * K + k, k), lbf=bad, rows=[8, i, 0])
    for v in (np.nan, np.inf, -np.inf):
        bad = res.copy(); bad[3, 7] = v
        refused("residual[%d] is not finite" % (3 * dim + 7), res=bad)
        refused("residual[%d] is not finite" % (3 * dim + 7), res=bad, rows=[3])
    # the used rows of lbf must fit the workspace: one serial pass, nothing to chunk
    big_lbf, big_res = fit_ref.make_problem(2, 3000, 100, leaf_n, dim)
    c.set_option("workspace_mb", 1)
    refused("workspace_mb", lbf=big_lbf, res=big_res, n=3000, K=100)
    for key in ("fit_lds_kb", "fit_ahead"):
        with pytest.raises(api.JdaError):
            c.set_option(key, -1)
    c.close()


def test_empty_problem_returns_zeros(built, model_file):
    L, D, K = 5, 3, 4
    c = _cascador(model_file, L, D)
    lbf, res = fit_ref.make_problem(1, 6, K, 1 << (D - 1), 2 * L)
    for args in ((lbf, res, []), (lbf[:0], res[:0], None)):
        w, iters, gn, st = c.global_regression_cpp(args[0], args[1], rows=args[2])
        assert w.shape == (K * 4, 2 * L) and not w.any() and not iters.any() and not gn.any() and st["epochs_launched"] == 0
    # rows == NULL: n_rows is not read -- n = 0 with a negative n_rows is the empty problem, not a refusal
    from jda_amd import api
    w = np.full((K * 4, 2 * L), 7.25)
    assert api.lib.jdaGlobalRegressionCpp(c.h, None, None, 0, K, None, -5, None, w.ctypes.data_as(C.POINTER(C.c_double)), None, None, None) == 0
    assert not w.any()
    c.close()


# ---- control 1: the restated solver is a solver ------------------------------------------------------------------------

# largest |w_ref - w_numpy| measured for this case (n = 60, K = 6, leafNum = 4, C = 1, eps = 1e-10): 4.16e-12; the stop rule
# is relative to the first epoch's gradient norm, so the residual depends on the data -- the bound is 10 x the measurement
CONTROL_1_MEASURED = 4.16e-12


def test_control_restated_solver_solves_the_primal():
    n, K, leaf_n, dim, Cv = 60, 6, 4, 2, 1.0
    lbf, res = fit_ref.make_problem(7, n, K, leaf_n, dim, noise=0.05)
    w, iters, gn = fit_ref.fit_arrays(lbf, res, leaf_n, C=Cv, eps=1e-10, max_iter=100000, seed=3)
    X = np.zeros((n, K * leaf_n))
    X[np.arange(n)[:, None], lbf] = 1.
    want = np.linalg.solve(np.eye(K * leaf_n) + 2 * Cv * X.T @ X, 2 * Cv * X.T @ res)   # the primal of L2-loss SVR at p = 0
    err = float(np.abs(w - want).max())
    print("fit_ref against the closed form: max |diff| = %.3e after %s epochs (|w| up to %.3f)" % (err, iters.tolist(), np.abs(want).max()))
    assert (iters < 100000).all() and (gn[1] <= 1e-10 * gn[0]).all()
    assert np.abs(want).max() > 0.01
    assert err <= 10 * CONTROL_1_MEASURED


# ---- control 2: the pinned order of dot is visible ---------------------------------------------------------------------

def test_control_sequential_dot_changes_the_weights():
    seed, n, K, D, L = fit_ref.ORDER_CASE
    leaf_n = 1 << (D - 1)
    lbf, res = fit_ref.make_problem(seed, n, K, leaf_n, 2 * L)
    w, _, _ = fit_ref.fit_arrays(lbf, res, leaf_n, max_iter=12, seed=1)
    ws, _, _ = fit_ref.fit_arrays(lbf, res, leaf_n, max_iter=12, seed=1, sequential_dot=True)
    changed = int((w.view(np.uint64) != ws.view(np.uint64)).sum())
    print("weights whose bits change under a sequential dot: %d of %d" % (changed, w.size))
    assert changed >= 1
    assert np.abs(w - ws).max() < 1e-12                                       # ... and nothing but the order changed


# ---- the end-to-end inputs: the reference chain alone lowers the stage's error ------------------------------------------

def test_reference_chain_lowers_the_mean_error():
    D, L, K = 3, 5, 6
    d, gt = fit_ref.e2e_inputs()
    rows, th = stage_ref.make_carts(31, K, D, L, True)
    _, w, iters, _, _, before, after = fit_ref.e2e_reference(d, gt, D, stage_ref.carts_of(D, rows, th), L)
    print("mean error %.5f -> %.5f, epochs %s" % (before, after, iters))
    assert after < before
