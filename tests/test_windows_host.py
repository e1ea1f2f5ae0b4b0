"""tests/windows_ref.py -- the numpy-fp32 restatement of the reference's window loop that tests/test_windows.py holds the GPU
entry jdaValidateWindows against -- pinned to the CPU oracle (itself pinned to the compiled reference,
tests/test_oracle_vs_reference.py): for EVERY window of the reference's grid on small frames, carts_n, score, path_hash and
shapes bit for bit; the grid enumeration too.  No GPU.  These tests pass without the feature: they vouch for the yardstick."""
import numpy as np
import pytest

import windows_ref
from conftest import same

# (T, K, L, D), frame size, seed, tau of the calibration: chosen on the CPU so that the precondition below holds
CASES = [((2, 8, 5, 3), (64, 48), 4, 5.0), ((3, 20, 5, 4), (80, 64), 5, 9.0)]
SCAN = dict(scale=1.25, min_size=24, max_size=-1)


def make_case(dims, size, seed, tau, multi):
    """A synthetic model in the cascade regime and two frames.  calibrate_thresholds walks scale-0 nodes only, so the
    multi-scale model is calibrated with its scales set aside and gets them back: its thresholds are then merely plausible,
    which the precondition checks."""
    from jda_amd import synth
    m = synth.make_model(*dims, seed=seed, multi_scale=multi, norm_every=3)
    frames = synth.make_frames(2, size[0], size[1], seed=seed + 100)
    scale = m.scale.copy()
    m.scale[:] = 0
    synth.calibrate_thresholds(m, synth.make_frames(4, size[0], size[1], seed=seed + 200), tau=tau, p_final=0.05, min_size=24)
    m.scale = scale
    return m, frames


@pytest.mark.parametrize("multi", [False, True], ids=["scale0", "multiscale"])
@pytest.mark.parametrize("dims,size,seed,tau", CASES)
def test_restatement_equals_oracle_on_the_grid(built, tmp_path, dims, size, seed, tau, multi):
    from oracle.pyoracle import Oracle
    m, frames = make_case(dims, size, seed, tau, multi)
    p = str(tmp_path / "m.model")
    m.save(p, 8)
    orc = Oracle(p)
    rm = windows_ref.RefModel(m)
    assert rm.multi == multi
    g = windows_ref.grid(size[0], size[1], **SCAN)
    carts_all = []
    for f in range(len(frames)):
        want = orc.trace(frames[f], **SCAN)
        assert len(g) == len(want["carts_n"]) == orc.count_windows(size[0], size[1], **SCAN)[0]
        got = windows_ref.validate(rm, frames, [(f, x, y, s) for x, y, s in g])
        for k in ("carts_n", "score", "path_hash", "shapes"):
            assert same(got[k], want[k]), (f, k, int((np.asarray(got[k]) != np.asarray(want[k])).sum()))
        carts_all.append(got["carts_n"])
    # what the GPU tests rely on: the walk ends in each of the three places
    c = np.concatenate(carts_all)
    T, K = dims[0], dims[1]
    assert (c == 1).any(), "no window rejects at cart 0"
    assert ((c > K) & (c < T * K)).any(), "no window rejects in a later stage"
    assert (c == T * K).any(), "no window walks all T*K carts"


def test_grid_is_the_projects_enumeration():
    from jda_amd import synth
    for w, h, kw in [(64, 48, SCAN), (80, 64, SCAN), (200, 150, dict(scale=1.2, min_size=30, max_size=100)), (23, 50, SCAN)]:
        xs, ys, ws = synth.window_table(w, h, **kw)
        g = np.array(windows_ref.grid(w, h, **kw), np.int32).reshape(-1, 3)
        assert np.array_equal(g[:, 0], xs) and np.array_equal(g[:, 1], ys) and np.array_equal(g[:, 2], ws)


def test_pyramid_equals_oracle_resize(built, tmp_path):
    from jda_amd import synth
    from oracle.pyoracle import Oracle
    p = str(tmp_path / "m.model")
    synth.make_model(1, 4, 3, 2, seed=1).save(p, 8)
    orc = Oracle(p)
    for w, h in [(64, 48), (80, 64), (37, 29)]:
        fr = synth.make_frames(1, w, h, seed=9)[0]
        half, quarter = windows_ref.pyramid(fr)
        hw, hh, qw, qh = orc.pyramid_dims(w, h)
        assert np.array_equal(half, orc.resize(fr, hw, hh)) and np.array_equal(quarter, orc.resize(fr, qw, qh))
