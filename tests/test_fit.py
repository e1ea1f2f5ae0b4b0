"""A stage's global regression on the device (jdaGlobalRegressionCpp, k_fit.hip) against the sequential restatement
tests/fit_ref.py, bit for bit: w, iters and both gnorm1 rows are compared exactly (`same`), there is no tolerance anywhere.
tests/test_fit_host.py holds the controls: the restatement solves the primal it claims to, and the pinned shape of dot is
visible in the bits of these tests' own inputs.  Dialect CPP is parity-unpinned: bit-exact against this repo's restatement
of include/jda.h, not against the reference."""
import numpy as np
import pytest

from conftest import same
import fit_ref
import stage_ref
import train_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _cascador(model_file, L, D):
    from jda_amd import api
    p, _ = model_file((1, 2, L, D))
    return api.Cascador(p, "double", device=0)


def _check(c, lbf, res, D, want=None, **kw):
    """One call against the restatement (or a result computed before): everything it returns, bit for bit."""
    kw.setdefault("max_iter", 25)
    if want is None:
        want = fit_ref.fit_arrays(lbf, res, 1 << (D - 1), **kw)
    w, iters, gn, st = c.global_regression_cpp(lbf, res, **kw)
    assert same(iters, want[1]), (iters, want[1])
    assert same(gn, want[2])
    assert same(w, want[0])
    assert st["epochs_launched"] >= int(iters.max())
    return want, st


def test_smallest_case(built, gpu, model_file):
    """K = 1, n = 1, L = 1 on the shallowest cascador there is: the model loader refuses tree_depth < 2 ("implausible
    dimensions"), so a cascador of depth 1 (leafNum 1) cannot be made; depth 2 has leafNum 2, the sample sits in leaf 1."""
    c = _cascador(model_file, 1, 2)
    lbf, res = np.ones((1, 1), np.int32), np.array([[0.25, -0.5]])
    want, st = _check(c, lbf, res, 2)
    assert st["lds_path"] == 1 and np.abs(want[0]).max() > 0
    c.close()


@pytest.mark.parametrize("K,L", [(1, 1), (63, 1), (64, 2), (65, 1), (130, 1)])
def test_lane_edges_of_the_strided_sums(built, gpu, model_file, K, L):
    D = 3
    c = _cascador(model_file, L, D)
    seed, n = (fit_ref.ORDER_CASE[0], fit_ref.ORDER_CASE[1]) if K == 130 else (K, 24)
    lbf, res = fit_ref.make_problem(seed, n, K, 1 << (D - 1), 2 * L)
    _check(c, lbf, res, D, max_iter=12, seed=1)
    c.close()


@pytest.mark.parametrize("K", [540, 700, 1030])
def test_wide_stages_on_both_paths(built, gpu, model_file, K):
    """The instantiations that keep 9 and 16 rounds of 64 carts in registers (K = 540, the shipped size, and K = 700) and the
    generic one for K above 1024, which reads the row where it uses it: each with the column in LDS and in global memory."""
    D, L, n = 2, 1, 12
    c = _cascador(model_file, L, D)
    lbf, res = fit_ref.make_problem(K, n, K, 1 << (D - 1), 2 * L)
    want, st = _check(c, lbf, res, D, max_iter=4, C=1.0, seed=K)
    assert st["lds_path"] == 1 and (want[1] == 4).all() and np.abs(want[0]).max() > 1e-3
    c.set_option("fit_lds_kb", 0)
    assert _check(c, lbf, res, D, want, max_iter=4, C=1.0, seed=K)[1]["lds_path"] == 0
    c.close()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 67, 200])
def test_index_batch_and_prefetch_edges(built, gpu, model_file, n):
    D, L, K = 3, 1, 5
    c = _cascador(model_file, L, D)
    lbf, res = fit_ref.make_problem(n, n, K, 1 << (D - 1), 2 * L)
    _check(c, lbf, res, D, max_iter=10, seed=n)
    c.close()


@pytest.mark.parametrize("L", [1, 27, 68])
def test_coordinates(built, gpu, model_file, L):
    D = 3
    c = _cascador(model_file, L, D)
    lbf, res = fit_ref.make_problem(L, 40, 3, 1 << (D - 1), 2 * L)
    _check(c, lbf, res, D, max_iter=8)
    c.close()


@pytest.mark.parametrize("D", [2, 4, 6])
def test_depths(built, gpu, model_file, D):
    c = _cascador(model_file, 2, D)
    lbf, res = fit_ref.make_problem(D, 50, 7, 1 << (D - 1), 4)
    assert len(set((lbf % (1 << (D - 1))).reshape(-1).tolist())) == 1 << (D - 1) or D == 6
    _check(c, lbf, res, D, max_iter=10)
    c.close()


def test_coordinates_stop_at_different_epochs(built, gpu, model_file):
    D, L, K, n = 3, 2, 4, 40
    leaf_n = 1 << (D - 1)
    c = _cascador(model_file, L, D)
    lbf, res = fit_ref.make_problem(3, n, K, leaf_n, 4, noise=0.05)
    clean, _ = fit_ref.make_problem(3, n, K, leaf_n, 4, noise=0.0)[1], None
    res[:, 0] = 0.                                                            # stops after epoch 1 with w = 0 (d = -beta, |d| < 1e-12)
    res[:, 1] = 1e-14                                                         # every step below the 1e-12 cut: nothing moves, Gnorm1
    res[:, 2] = clean[:, 2]                                                   # never falls, the coordinate runs to max_iter; noiseless
    want, _ = _check(c, lbf, res, D, max_iter=60, C=1.0, eps=1e-3, seed=4)    # column 3: noisy
    w, iters, gn = want
    assert iters[0] == 1 and not w[:, 0].any() and gn[0][0] == 0.
    assert iters[1] == 60 and not w[:, 1].any() and gn[1][1] == gn[0][1] > 0.
    assert 1 < iters[2] < 60 and 1 < iters[3] < 60 and iters[2] != iters[3]
    c.close()


def test_max_iter_reached(built, gpu, model_file):
    D, L = 3, 1
    c = _cascador(model_file, L, D)
    lbf, res = fit_ref.make_problem(8, 50, 6, 4, 2, noise=0.05)
    want, st = _check(c, lbf, res, D, max_iter=3, eps=1e-12, C=1.0)
    assert (want[1] == 3).all() and (want[2][1] > 1e-12 * want[2][0]).all() and st["epochs_launched"] == 3
    c.close()


def test_lds_path_equals_global_path(built, gpu, model_file):
    D, L = 4, 1
    c = _cascador(model_file, L, D)
    lbf, res = fit_ref.make_problem(9, 40, 70, 8, 2)                          # a column is 70 * 8 doubles = 4,480 B: four granules
    want, st = _check(c, lbf, res, D, max_iter=6)
    assert (st["lds_path"], st["lds_bytes"]) == (1, 4480)
    c.set_option("fit_lds_kb", 5)                                             # 5 KB = exactly four granules: still fits
    assert _check(c, lbf, res, D, want, max_iter=6)[1]["lds_path"] == 1
    c.set_option("fit_lds_kb", 4)                                             # three granules: does not
    assert _check(c, lbf, res, D, want, max_iter=6)[1]["lds_path"] == 0
    c.set_option("fit_lds_kb", 0)
    _, st = _check(c, lbf, res, D, want, max_iter=6)
    assert (st["lds_path"], st["lds_bytes"]) == (0, 0)
    c.close()


def test_fit_ahead_does_not_change_results(built, gpu, model_file):
    D, L = 3, 2
    c = _cascador(model_file, L, D)
    lbf, res = fit_ref.make_problem(10, 45, 5, 4, 4)
    res[:, 1] = 0.
    kw = dict(max_iter=60, C=1.0, eps=1e-2)
    c.set_option("fit_ahead", 0)
    want, st0 = _check(c, lbf, res, D, **kw)
    assert st0["epochs_launched"] == int(want[1].max()) < 60                  # synchronous: not one launch past the last stop
    c.set_option("fit_ahead", 4)
    _, st4 = _check(c, lbf, res, D, want, **kw)
    assert int(want[1].max()) <= st4["epochs_launched"] <= int(want[1].max()) + 4
    c.close()


def test_rows_subset_equals_the_gathered_problem(built, gpu, model_file):
    D, L = 3, 1
    c = _cascador(model_file, L, D)
    lbf, res = fit_ref.make_problem(11, 90, 5, 4, 2)
    rows = np.random.default_rng(11).permutation(90)[:70].astype(np.int32)
    rows[5] = rows[40]                                                        # a row named twice is two samples
    lbf2, res2 = lbf.copy(), res.copy()
    unused = np.setdiff1d(np.arange(90), rows)
    lbf2[unused] = -7; res2[unused] = np.nan                                  # rows that are not used are not looked at
    want = fit_ref.fit_arrays(lbf[rows], res[rows], 4, max_iter=10, seed=2)
    w, iters, gn, _ = c.global_regression_cpp(lbf2, res2, rows=rows, max_iter=10, seed=2)
    assert same(w, want[0]) and same(iters, want[1]) and same(gn, want[2])
    w, iters, gn, _ = c.global_regression_cpp(lbf[rows], res[rows], max_iter=10, seed=2)      # the dense call on the gathered arrays
    assert same(w, want[0]) and same(iters, want[1]) and same(gn, want[2])
    c.close()


def test_parameters_and_repeatability(built, gpu, model_file):
    D, L = 3, 1
    c = _cascador(model_file, L, D)
    lbf, res = fit_ref.make_problem(12, 60, 6, 4, 2)
    a, _ = _check(c, lbf, res, D, C=0.7, max_iter=9, seed=1)
    b, _ = _check(c, lbf, res, D, C=0.7, max_iter=9, seed=2)
    d, _ = _check(c, lbf, res, D, max_iter=9, seed=1)                         # C <= 0: 1 / n_rows
    assert not same(a[0], b[0]) and not same(a[0], d[0])
    _check(c, lbf, res, D, a, C=0.7, max_iter=9, seed=1)                      # again on the same cascador: no state leaks
    c.close()


def test_end_to_end_stage(built, gpu, model_file):
    from jda_amd import api
    D, L, F, K = 3, 5, 24, 6
    c = _cascador(model_file, L, D)
    d, gt = fit_ref.e2e_inputs()
    nd = train_ref.make_samples(131, 60, L)
    pd = dict(d, residual=api.shape_residual_cpp(gt, d["shapes"], landmark_id=0))
    feats, ths = [], []
    for k in range(K):
        pools = [train_ref.gen_feature_pool(F, L, train_ref.RADIUS, True, 31 + k, node) for node in range(1, 4)]
        flat = stage_ref.pool_array([r for p, _ in pools for r in p])
        got = c.train_cart_cpp(pd, nd, flat, [1, 0, 1], np.array([u for _, u in pools]))
        feats.append(got["features"]); ths.append(got["thresholds"])
    feats, ths = np.concatenate(feats), np.concatenate(ths)
    lbf = c.gen_lbf_cpp(d, feats, ths)
    res = api.shape_residual_cpp(gt, d["shapes"])
    w, iters, gn, _ = c.global_regression_cpp(lbf, res, C=10.0, max_iter=40, seed=9)
    shapes = c.stage_update_shapes_cpp(d, None, None, w, lbf)
    before = api.mean_error_cpp(gt, d["shapes"], [0], [1])
    after = api.mean_error_cpp(gt, shapes, [0], [1])
    # the same chain in the restatements
    rows = [(f["scale"], f["landmark_id1"], f["landmark_id2"], f["offset1_x"], f["offset1_y"], f["offset2_x"], f["offset2_y"]) for f in feats]
    r_lbf, r_w, r_iters, r_gn, r_shapes, r_before, r_after = fit_ref.e2e_reference(d, gt, D, stage_ref.carts_of(D, rows, ths), L)
    assert same(lbf, np.array(r_lbf, np.int32)) and same(res, gt - d["shapes"])
    assert same(w, np.array(r_w)) and same(iters, np.array(r_iters, np.int32)) and same(gn, np.array(r_gn))
    assert same(shapes, np.array(r_shapes)) and same(np.float64(after), np.float64(r_after)) and same(np.float64(before), np.float64(r_before))
    print("mean error %.5f -> %.5f" % (before, after))
    assert r_after < r_before and after < before
    c.close()
