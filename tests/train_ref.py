"""Plain-Python, sequential restatement of the reference's CART training that the training tests compare the product
with (test infrastructure, not product; nothing under jda_amd/ imports it), written from the reference's source:
DataSet::CalcFeatureValues (src/jda/data.cpp:148-173) on oracle.cpp_reading2's split-node evaluation, Cart::SplitNode's
recursion and leaf scores (src/jda/cart.cpp:57-162), SplitNodeWithClassification (cart.cpp:176-252),
SplitNodeWithRegression (cart.cpp:288-350), Cart::GenFeaturePool (cart.cpp:352-390) on include/jda.h's generator.
Python floats are IEEE doubles and math.log is the host C library's log: this is the bit-level yardstick.  Dialect CPP is
parity-unpinned: the reference itself needs OpenCV and cannot be built here."""
import math

from oracle import cpp_reading2 as r2

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
ESP = 2.2e-16                       # Config::esp, common.cpp:143
DBL_MAX = 1.7976931348623157e308    # numeric_limits<double>::max()


# ---- IEEE helpers (C++ doubles do not raise) ---------------------------------------------------------------------------

def fdiv(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def clog(x):
    if x != x or x < 0:
        return math.nan
    if x == 0:
        return -math.inf
    return math.log(x)


def is_zero(v):                     # cart.cpp:18-21
    return abs(v) < 1e-9


def calc_entropy(p):                # cart.cpp:169-174
    if is_zero(p) or is_zero(1. - p):
        return 0.
    e = -(p) * clog(p) - (1. - p) * clog(1. - p)
    e /= math.log(2.)
    return e


# ---- the pool ----------------------------------------------------------------------------------------------------------

def splitmix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


class PoolRng:
    """include/jda.h: draw d = 1, 2, ... of feature i under (seed, key)."""

    def __init__(self, seed, key, i):
        self.base = splitmix64((splitmix64((seed + (key + 1) * G) & M64) + (i + 1) * G) & M64)
        self.d = 0

    def next(self):
        self.d += 1
        return splitmix64((self.base + self.d * G) & M64)

    def unit(self):
        return float(self.next() >> 11) * 2.0 ** -53

    def uniform(self, a, b):
        return a + (b - a) * self.unit()


def gen_feature_pool(F, L, radius, multi_scale, seed, key):
    """Cart::GenFeaturePool (cart.cpp:352-390) in include/jda.h's draw order -> ([(scale, lm1, lm2, o1x, o1y, o2x, o2y)], [u])."""
    feats, us = [], []
    for i in range(F):
        rng = PoolRng(seed, key, i)
        x1 = y1 = x2 = y2 = 1.
        while x1 * x1 + y1 * y1 > 1. or x2 * x2 + y2 * y2 > 1.:     # cart.cpp:364-367
            x1 = rng.uniform(-1., 1.); y1 = rng.uniform(-1., 1.)
            x2 = rng.uniform(-1., 1.); y2 = rng.uniform(-1., 1.)
        scale = rng.next() % 3                                       # cart.cpp:369-378
        if not multi_scale:
            scale = 0                                                # cart.cpp:381
        lm1 = rng.next() % L
        lm2 = rng.next() % L
        feats.append((scale, lm1, lm2, x1 * radius, y1 * radius, x2 * radius, y2 * radius))
        us.append(rng.uniform(0.1, 0.9))                             # cart.cpp:320
    return feats, us


def pool_of(features):
    """Rows of (scale, lm1, lm2, o1x, o1y, o2x, o2y) (tuples or jda_amd.api.FEATURE_DTYPE records) as the object
    cpp_reading2.feature_value reads its node fields from."""
    c = r2.Cart2()
    rows = [(int(f["scale"]), int(f["landmark_id1"]), int(f["landmark_id2"]), float(f["offset1_x"]), float(f["offset1_y"]),
             float(f["offset2_x"]), float(f["offset2_y"])) if not isinstance(f, tuple) else f for f in features]
    c.scale = [r[0] for r in rows]; c.lm1 = [r[1] for r in rows]; c.lm2 = [r[2] for r in rows]
    c.o1x = [r[3] for r in rows]; c.o1y = [r[4] for r in rows]; c.o2x = [r[5] for r in rows]; c.o2y = [r[6] for r in rows]
    return c


class SampleSet:
    """patches: per sample a tuple (o, h, q) of 2-D uint8 arrays; shapes: per sample a list of 2L floats."""

    def __init__(self, patches, shapes, weights, residual=None, has_gt=None):
        self.patches = [tuple((p.tolist(), 0, 0, p.shape[1], p.shape[0]) for p in t) for t in patches]
        self.shapes = [[float(v) for v in s] for s in shapes]
        self.weights = [float(w) for w in weights]
        self.residual = None if residual is None else [(float(r[0]), float(r[1])) for r in residual]
        self.has_gt = None if has_gt is None else [int(g) for g in has_gt]
        self.n = len(self.shapes)


def calc_feature_values(s, pool, idx):
    """DataSet::CalcFeatureValues (data.cpp:148-173) with the identity STParameter: [feature][position in idx]."""
    n = len(pool.scale)
    out = [[0] * len(idx) for _ in range(n)]
    for j, sid in enumerate(idx):
        pt, shape = s.patches[sid], s.shapes[sid]
        for i in range(n):
            out[i][j] = r2.feature_value(pool, i, pt, shape, r2.IDENTITY)
    return out


# ---- the two criteria --------------------------------------------------------------------------------------------------

def split_classification(pos, pos_idx, neg, neg_idx, pf, nf, reverse=False, detail=None):
    """SplitNodeWithClassification (cart.cpp:176-252) -> (feature_idx, threshold, es_, ths_).  reverse=True adds every bin
    and both totals in REVERSED sample order: the control that summation order is visible in the criterion.  detail: a dict
    that receives the intermediates as they stood before the sweep -- wp / wn (weighted histograms [F][511]) and p_n / n_n
    (count histograms)."""
    feature_n, pos_n, neg_n = len(pf), len(pos_idx), len(neg_idx)
    feature_idx, threshold = 0, -256
    es_, ths_ = [0.] * feature_n, [0] * feature_n
    pj = range(pos_n - 1, -1, -1) if reverse else range(pos_n)
    nj = range(neg_n - 1, -1, -1) if reverse else range(neg_n)
    for i in range(feature_n):
        wp_l = wp_r = wn_l = wn_r = 0.
        wp, wn = [0.] * 511, [0.] * 511
        p_n, n_n = [0] * 511, [0] * 511
        for j in pj:                                                 # cart.cpp:199-203
            wp[pf[i][j] + 255] += pos.weights[pos_idx[j]]
            wp_r += pos.weights[pos_idx[j]]
            p_n[pf[i][j] + 255] += 1
        for j in nj:                                                 # cart.cpp:204-208
            wn[nf[i][j] + 255] += neg.weights[neg_idx[j]]
            wn_r += neg.weights[neg_idx[j]]
            n_n[nf[i][j] + 255] += 1
        if detail is not None:
            for k, v in (("wp", wp), ("wn", wn), ("p_n", p_n), ("n_n", n_n)):
                detail.setdefault(k, []).append(v)
        current_p = current_n = 0
        w = wp_r + wn_r
        threshold_ = -256
        entropy = calc_entropy(fdiv(wp_r, w))
        for th in range(-255, 256):                                  # cart.cpp:216-238
            idx = th + 255
            wp_l += wp[idx]; wn_l += wn[idx]
            wp_r -= wp[idx]; wn_r -= wn[idx]
            current_p += p_n[idx]; current_n += n_n[idx]
            p_ratio = fdiv(float(current_p), float(pos_n))
            n_ratio = fdiv(float(current_n), float(neg_n))
            if p_ratio < 0.1 or p_ratio > 0.9:
                continue
            if n_ratio < 0.1 or n_ratio > 0.9:
                continue
            w_l = wp_l + wn_l
            w_r = wp_r + wn_r
            e = fdiv(w_l, w) * calc_entropy(fdiv(wp_l, w_l)) + fdiv(w_r, w) * calc_entropy(fdiv(wp_r, w_r))
            if e < entropy:
                entropy = e
                threshold_ = th
        es_[i] = entropy
        ths_[i] = threshold_
    entropy_min = DBL_MAX                                            # cart.cpp:243-250
    for i in range(feature_n):
        if es_[i] < entropy_min:
            entropy_min = es_[i]
            threshold = ths_[i]
            feature_idx = i
    return feature_idx, threshold, es_, ths_


def calc_variance(vec):
    """calcVariance (cart.cpp:259-266).  cv::mean and Mat::mul are OpenCV's: DEFINED in include/jda.h as sums in sample
    order times the reciprocal of the count (from memory of cv::mean, unchecked)."""
    if len(vec) == 0:
        return 0.
    inv = 1. / float(len(vec))
    s1 = s2 = 0.
    for v in vec:
        s1 += v
        s2 += v * v
    m1, m2 = s1 * inv, s2 * inv
    return m2 - m1 * m1


def ordered_sums(vec):
    """calc_variance's two sums of vec, in its order -> (sum v, sum v * v)."""
    s1 = s2 = 0.
    for v in vec:
        s1 += v
        s2 += v * v
    return s1, s2


def split_regression(pos, pos_idx, pf, u, detail=None):
    """SplitNodeWithRegression (cart.cpp:288-350) -> (feature_idx, threshold, vs_, ths_); pos.residual[s] is
    CalcShapeResidual(idx, landmark_id)'s row of sample s.  detail: a dict that receives the intermediates -- kidx (the index
    into the sorted values), th, counts (the values' count histogram [F][511]), sums ([F][8]: calc_variance's sums of lx, ly,
    rx, ry as left x, x*x, y, y*y, right x, x*x, y, y*y), n_left, n_right."""
    feature_n, pos_n = len(pf), len(pos_idx)
    feature_idx, threshold = 0, -256
    if pos_n == 0:                                                   # cart.cpp:299-301 (include/jda.h: 0 / -256 reported)
        return feature_idx, threshold, [0.] * feature_n, [-256] * feature_n
    vs_, ths_ = [0.] * feature_n, [0] * feature_n
    for i in range(feature_n):
        srt = sorted(pf[i])                                          # cart.cpp:314-315
        threshold_ = srt[min(pos_n - 1, int(pos_n * u[i]))]          # cart.cpp:320
        lx, ly, rx, ry = [], [], [], []
        for j in range(pos_n):
            if pos.has_gt is not None and not pos.has_gt[pos_idx[j]]:
                continue                                             # cart.cpp:323-325
            r = pos.residual[pos_idx[j]]
            if pf[i][j] <= threshold_:
                lx.append(r[0]); ly.append(r[1])
            else:
                rx.append(r[0]); ry.append(r[1])
        vs_[i] = (calc_variance(lx) + calc_variance(ly)) * float(len(lx)) + \
                 (calc_variance(rx) + calc_variance(ry)) * float(len(rx))
        ths_[i] = threshold_
        if detail is not None:
            counts = [0] * 511
            for v in pf[i]:
                counts[v + 255] += 1
            detail.setdefault("kidx", []).append(min(pos_n - 1, int(pos_n * u[i])))
            detail.setdefault("th", []).append(threshold_)
            detail.setdefault("counts", []).append(counts)
            detail.setdefault("sums", []).append(list(ordered_sums(lx) + ordered_sums(ly) + ordered_sums(rx) + ordered_sums(ry)))
            detail.setdefault("n_left", []).append(len(lx))
            detail.setdefault("n_right", []).append(len(rx))
    variance_min = DBL_MAX                                           # cart.cpp:341-348
    for i in range(feature_n):
        if vs_[i] < variance_min:
            variance_min = vs_[i]
            threshold = ths_[i]
            feature_idx = i
    return feature_idx, threshold, vs_, ths_


def ordered_histogram(values, idx, weights):
    """The ordered histogram of cart.cpp:199-203 said once more, by brute force: the second opinion on split_classification's
    wp / wn for the crafted inputs of tests/test_train_limits_host.py."""
    bins = [0.] * 511
    for j, s in enumerate(idx):
        bins[values[j] + 255] += weights[s]
    return bins


def split_node(pos, pos_idx, neg, neg_idx, pool, mode, u, detail=None):
    """The choice of cart.cpp:93-115 -> (feature_idx, threshold, criteria, thresholds, pos_feature, neg_feature)."""
    pf = calc_feature_values(pos, pool, pos_idx)
    nf = calc_feature_values(neg, pool, neg_idx)
    if mode == 1:
        fi, th, es, ths = split_classification(pos, pos_idx, neg, neg_idx, pf, nf, detail=detail)
    else:
        fi, th, es, ths = split_regression(pos, pos_idx, pf, u, detail=detail)
    return fi, th, es, ths, pf, nf


def train_cart(D, pos, neg, pools, modes, us):
    """Cart::Train / SplitNode (cart.cpp:41-162).  pools[i - 1] (a pool_of object), modes[i - 1], us[i - 1] belong to node
    i = 1 .. nodes_n/2 - 1.  -> dict(features (pool index per node), thresholds, scores, pos_leaf, neg_leaf, nodes)."""
    nodes_n = 1 << D
    half = nodes_n // 2
    out = dict(features=[0] * (half - 1), thresholds=[0] * (half - 1), scores=[0.] * half, pos_leaf=[0] * pos.n,
               neg_leaf=[0] * neg.n, nodes=[None] * (half - 1))

    def rec(pos_idx, neg_idx, node_idx):
        if node_idx >= half:                                         # cart.cpp:63-89
            idx = node_idx - half
            pos_w = neg_w = ESP
            for i in pos_idx:
                pos_w += pos.weights[i]
                out["pos_leaf"][i] = idx
            for i in neg_idx:
                neg_w += neg.weights[i]
                out["neg_leaf"][i] = idx
            out["scores"][idx] = 0.5 * (clog(pos_w) - clog(neg_w))
            return
        pool = pools[node_idx - 1]
        fi, th, es, _ths, pf, nf = split_node(pos, pos_idx, neg, neg_idx, pool, modes[node_idx - 1],
                                              None if us is None else us[node_idx - 1])
        lp = [s for j, s in enumerate(pos_idx) if pf[fi][j] <= th] if pos_idx else []       # cart.cpp:120-150
        rp = [s for j, s in enumerate(pos_idx) if not pf[fi][j] <= th] if pos_idx else []
        ln = [s for j, s in enumerate(neg_idx) if nf[fi][j] <= th] if neg_idx else []
        rn = [s for j, s in enumerate(neg_idx) if not nf[fi][j] <= th] if neg_idx else []
        out["features"][node_idx - 1] = fi
        out["thresholds"][node_idx - 1] = th
        out["nodes"][node_idx - 1] = (len(pos_idx), len(neg_idx), fi, es[fi])
        rec(lp, ln, 2 * node_idx)                                    # cart.cpp:160-161
        rec(rp, rn, 2 * node_idx + 1)
    rec(list(range(pos.n)), list(range(neg.n)), 1)
    return out


class _Depth:
    def __init__(self, D):
        self.D = D


def forward(D, rows, thresholds, patches, shape):
    """The existing dialect-CPP walk, oracle.cpp_reading2.forward (Cart::Forward, cart.cpp:392-404), on a trained cart
    given as per-node feature rows and thresholds (node i at index i - 1)."""
    c = pool_of([rows[0]] + list(rows))             # cpp_reading2's carts are indexed by node, from 1
    c.nth = [0] + [int(t) for t in thresholds]
    return r2.forward(_Depth(D), c, patches, shape, r2.IDENTITY)


# ---- test data (shared by the host and the GPU tests, so that the host-side control speaks about the GPU cases) --------

def make_samples(seed, n, L, sizes=(48, 36, 24), outside=0.15, flat=False, equal_weights=False, gt_drop=0.0):
    """A random sample set as the dict jda_amd.api takes.  Weights exp(-score) normalised with scores spread over +-8
    (wide dynamic range: the order of a sum is visible in its bits); a share of the shapes is pushed outside the patch
    (clamping); flat: every pixel equal (every feature value 0)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    pb = sum(v * v for v in sizes)
    patches = np.full((n, pb), 77, np.uint8) if flat else rng.integers(0, 256, (n, pb), dtype=np.uint8)
    shapes = rng.uniform(0.15, 0.85, (1, 2 * L)) + rng.normal(0, 0.05, (n, 2 * L))
    far = rng.random(n) < outside
    shapes[far] += rng.uniform(-0.9, 0.9, (int(far.sum()), 2 * L))
    score = rng.uniform(-8, 8, n)
    w = np.ones(n) if equal_weights else np.exp(-score)
    w = w / w.sum() if n else w
    residual = rng.normal(0, 0.05, (n, 2))
    has_gt = (rng.random(n) >= gt_drop).astype(np.uint8)
    return dict(patches=patches, shapes=shapes, weights=w, residual=residual, has_gt=has_gt, sizes=sizes)


def ref_set(d):
    """make_samples' dict -> SampleSet."""
    o, h, q = d["sizes"]
    pats = [(row[:o * o].reshape(o, o), row[o * o:o * o + h * h].reshape(h, h), row[o * o + h * h:].reshape(q, q))
            for row in d["patches"]]
    return SampleSet(pats, d["shapes"], d["weights"], d["residual"], d["has_gt"])


# classification cases of tests/test_train.py: (seed, pos_n, neg_n, L, multi_scale, F); tests/test_train_host.py checks
# on the CPU that reversed summation order changes bits of their criteria
CLS_CASES = [(11, 500, 400, 5, False, 48), (12, 450, 520, 27, True, 48)]
RADIUS = 0.3


# ---- crafted sample sets of tests/test_train_limits*.py (the host file proves each property on this restatement alone) --

FEW_LEVELS, FEW_PROBS = (40, 120, 200), (0.7, 0.2, 0.1)


def make_few_valued(seed, n, L, sizes=(48, 36, 24), outside=0.15, gt_drop=0.0):
    """make_samples with every pixel drawn from three equally spaced gray levels (shares 0.7 / 0.2 / 0.1): a feature takes
    at most the five values 0, +-80, +-160, about half of a list falls into bin 255, and the weights keep make_samples'
    score spread of +-8."""
    import numpy as np
    d = make_samples(seed, n, L, sizes, outside=outside, gt_drop=gt_drop)
    rng = np.random.default_rng(seed + 5000)
    d["patches"] = np.array(FEW_LEVELS, np.uint8)[rng.choice(3, size=d["patches"].shape, p=FEW_PROBS)]
    return d


def make_extreme(seed, n, L, sizes=(48, 36, 24), outside=0.3, gt_drop=0.0):
    """make_samples with every pixel 0 or 255 (so also every pixel a pool reads, and every border pixel a shape pushed
    outside the patch is clamped to): a feature takes the values -255, 0 and 255."""
    import numpy as np
    d = make_samples(seed, n, L, sizes, outside=outside, gt_drop=gt_drop)
    rng = np.random.default_rng(seed + 6000)
    d["patches"] = (rng.integers(0, 2, d["patches"].shape, dtype=np.uint8) * 255).astype(np.uint8)
    return d


def deepest_rank(values, count):
    """Over the FULL 64-entry batches of every feature's row (k_train_hist's batches of the list), the smallest and the
    largest number of entries the most-hit bin of a batch receives -> (min, max); a bin hit m times is added to in ranks
    0 .. m - 1.  count < 64 has no full batch: (0, 0)."""
    lo, hi = None, 0
    for row in values:
        for j0 in range(0, count - 63, 64):
            seen = {}
            for v in row[j0:j0 + 64]:
                seen[v] = seen.get(v, 0) + 1
            m = max(seen.values())
            lo = m if lo is None else min(lo, m)
            hi = max(hi, m)
    return (lo or 0), hi


def pairwise_cover(factors, allowed=lambda row: True):
    """Rows (one value per factor) in which every pair of values of two different factors occurs at least once, except pairs
    that `allowed` (called with a dict factor index -> value, partial rows included) rules out.  Greedy and deterministic:
    the first uncovered pair opens a row, every other factor takes the value that covers most of what is still uncovered."""
    todo = [(i, a, j, b) for i in range(len(factors)) for j in range(i + 1, len(factors)) for a in range(len(factors[i]))
            for b in range(len(factors[j])) if allowed({i: factors[i][a], j: factors[j][b]})]
    left = set(todo)
    rows = []
    for pair in todo:
        if pair not in left:
            continue
        i, a, j, b = pair
        row = {i: a, j: b}
        for k in range(len(factors)):
            if k in row:
                continue
            def gain(v):
                return sum(((k, v, m, row[m]) if k < m else (m, row[m], k, v)) in left for m in row)
            ok = [v for v in range(len(factors[k])) if allowed({**{m: factors[m][row[m]] for m in row}, k: factors[k][v]})]
            row[k] = max(ok, key=lambda v: (gain(v), -((v + len(rows)) % len(factors[k]))))
        for m in row:
            for q in row:
                if m < q:
                    left.discard((m, row[m], q, row[q]))
        rows.append(tuple(factors[k][row[k]] for k in range(len(factors))))
    return rows
