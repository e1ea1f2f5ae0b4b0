"""The mining enumeration without a GPU: jdaMineWindows / jdaMineWindowList against NextImage's walk restated in Python
(reference src/jda/data.cpp:885-967; tests/mining_ref.py)."""
import numpy as np
import pytest

import mining_ref


def _sweep():
    rng = np.random.default_rng(11)
    cases = [(48, 48, 48, 5, 1.2), (48, 100, 48, 5, 1.2), (100, 48, 48, 5, 1.2), (49, 49, 48, 2, 1.1),   # not > origin_size
             (24, 30, 24, 3, 1.25), (60, 100, 48, 7, 1.25),     # 48 * 1.25 = 60 lands on W exactly: no second level
             (101, 75, 48, 7, 1.5625), (75, 101, 48, 2, 1.5625),  # 48 -> 75 lands on H (resp. W)
             (640, 480, 48, 13, 1.3), (481, 641, 48, 23, 1.49)]
    for _ in range(60):
        w, h = int(rng.integers(20, 400)), int(rng.integers(20, 400))
        cases.append((w, h, int(rng.choice([24, 36, 48])), int(rng.integers(2, 24)), float(rng.uniform(1.1, 1.5))))
    return cases


@pytest.mark.parametrize("w,h,os_,step,factor", _sweep())
def test_mine_windows_count_and_listing_equal_next_image(built, w, h, os_, step, factor):
    from jda_amd import api
    want = mining_ref.windows(w, h, os_, step, factor)
    n, nl = api.mine_windows(w, h, os_, step, factor)
    assert (n, nl) == (len(want), len(mining_ref.levels(w, h, os_, step, factor)))
    got = api.mine_windows(w, h, os_, step, factor, listing=True)
    assert got.shape == (len(want), 3)
    assert np.array_equal(got, np.array(want, np.int32).reshape(-1, 3))


def test_mine_windows_edges(built):
    from jda_amd import api
    assert api.mine_windows(48, 480, 48, 5, 1.2) == (0, 0)                 # data.cpp:921: W must exceed origin_size
    assert api.mine_windows(60, 100, 48, 7, 1.25) == (((60 - 48) // 7 + 1) * ((100 - 48) // 7 + 1), 1)   # int(48 * 1.25) = 60 >= W
    with pytest.raises(api.JdaError):
        api.mine_windows(640, 480, 48, 0, 1.2)                            # step must be positive
    with pytest.raises(api.JdaError):
        api.mine_windows(640, 480, 48, 5, 1.01)                           # int(48 * 1.01) = 48: the walk would not end


def test_transforms_restatement_shapes():
    img = np.arange(12, dtype=np.uint8).reshape(3, 4)
    for t in range(8):
        got = mining_ref.transform(img, t)
        assert got.shape == ((4, 3) if t in (1, 3, 5, 7) else (3, 4))
    assert np.array_equal(mining_ref.transform(img, 7), img.T)            # flip(0), transpose, flip(1) = transpose
    assert np.array_equal(mining_ref.transform(img, 6), np.flipud(img))   # flip(-1) then flip(1) = flip(0)
