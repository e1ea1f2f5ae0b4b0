"""Plain-Python, sequential restatement of the trainer pieces under the similarity transform as include/jda.h defines them
with the option "train_similarity" (test infrastructure, not product; nothing under jda_amd/ imports it): every sample runs
under its own stp_mc = STParameter::Calc(its shape, mean_shape).  Nothing is restated twice: STParameter::Calc / Apply, the
split-node evaluation and Cart::Forward are oracle.cpp_reading2's (st_calc, st_apply, feature_value, forward); the two split
criteria are train_ref's, GenDeltaShape's sum is stage_ref's, the model file is model_ref's.  What is written here is only
how they compose: DataSet::CalcSTParameters (data.cpp:131-146), CalcFeatureValues with stp_mc[idx[j]] (jda.h's reading of
data.cpp:168), Cart::Train's recursion on it (cart.cpp:57-162), GenLBF / GenDeltaShape with the sample's parameter
(btcart.cpp:399, 422), CalcShapeResidual with stp_cm (data.cpp:185, 203) and Validate from a start shape (cascador.cpp:166-211).
Python floats are IEEE doubles: this is the bit-level yardstick.  Dialect CPP is parity-unpinned."""
import math

import numpy as np

from oracle import cpp_reading2 as r2

import stage_ref
import train_ref


class _Depth:
    def __init__(self, D):
        self.D = D


# ---- the parameters --------------------------------------------------------------------------------------------------------

def st_parameters(shapes, mean_shape):
    """DataSet::CalcSTParameters (data.cpp:131-146) -> (stp_mc, stp_cm), each a list of 5-tuples (scale, rot00, rot01, rot10, rot11)."""
    mean = [float(v) for v in mean_shape]
    L = len(mean) // 2
    mc = [r2.st_calc([float(v) for v in s], mean, L) for s in shapes]
    cm = [r2.st_calc(mean, [float(v) for v in s], L) for s in shapes]
    return mc, cm


def derive_cm(mc, scale_cm):
    """The shortcut the issue proposes for stp_cm: the same cosine, the sine negated (scale2 / scale1 computed apart)."""
    _, cs, msn, sn, _ = mc
    return (scale_cm, cs, sn, -sn, cs)


# ---- feature values, one node, one cart ---------------------------------------------------------------------------------------

def calc_feature_values(s, pool, idx, stp_mc):
    """CalcFeatureValues with the sample's own parameter, stp_mc[idx[j]]: [feature][position in idx]."""
    n = len(pool.scale)
    out = [[0] * len(idx) for _ in range(n)]
    for j, sid in enumerate(idx):
        for i in range(n):
            out[i][j] = r2.feature_value(pool, i, s.patches[sid], s.shapes[sid], stp_mc[sid])
    return out


def split_node(pos, pos_idx, neg, neg_idx, pool, mode, u, pos_mc, neg_mc):
    """train_ref.split_node on these values -> (feature_idx, threshold, criteria, thresholds, pos_feature, neg_feature)."""
    pf = calc_feature_values(pos, pool, pos_idx, pos_mc)
    nf = calc_feature_values(neg, pool, neg_idx, neg_mc)
    if mode == 1:
        fi, th, es, ths = train_ref.split_classification(pos, pos_idx, neg, neg_idx, pf, nf)
    else:
        fi, th, es, ths = train_ref.split_regression(pos, pos_idx, pf, u)
    return fi, th, es, ths, pf, nf


def train_cart(D, pos, neg, pools, modes, us, pos_mc, neg_mc):
    """Cart::Train / SplitNode (cart.cpp:41-162), train_ref.train_cart's recursion on split_node above."""
    half = (1 << D) // 2
    out = dict(features=[0] * (half - 1), thresholds=[0] * (half - 1), scores=[0.] * half, pos_leaf=[0] * pos.n, neg_leaf=[0] * neg.n)

    def rec(pos_idx, neg_idx, node_idx):
        if node_idx >= half:                                         # cart.cpp:63-89
            idx = node_idx - half
            pos_w = neg_w = train_ref.ESP
            for i in pos_idx:
                pos_w += pos.weights[i]
                out["pos_leaf"][i] = idx
            for i in neg_idx:
                neg_w += neg.weights[i]
                out["neg_leaf"][i] = idx
            out["scores"][idx] = 0.5 * (train_ref.clog(pos_w) - train_ref.clog(neg_w))
            return
        fi, th, _es, _ths, pf, nf = split_node(pos, pos_idx, neg, neg_idx, pools[node_idx - 1], modes[node_idx - 1],
                                               None if us is None else us[node_idx - 1], pos_mc, neg_mc)
        out["features"][node_idx - 1] = fi
        out["thresholds"][node_idx - 1] = th
        rec([s for j, s in enumerate(pos_idx) if pf[fi][j] <= th], [s for j, s in enumerate(neg_idx) if nf[fi][j] <= th], 2 * node_idx)
        rec([s for j, s in enumerate(pos_idx) if not pf[fi][j] <= th], [s for j, s in enumerate(neg_idx) if not nf[fi][j] <= th], 2 * node_idx + 1)
    rec(list(range(pos.n)), list(range(neg.n)), 1)
    return out


def forward(D, rows, thresholds, patches, shape, stp):
    """Cart::Forward of a trained cart (per-node feature rows and thresholds, node i at index i - 1) under stp."""
    c = stage_ref.carts_of(D, list(rows), list(thresholds))[0]
    return r2.forward(_Depth(D), c, patches, shape, stp)


# ---- closing a stage -----------------------------------------------------------------------------------------------------------

def apply_delta(stp, delta):
    """STParameter::Apply(delta, delta) (data.cpp:116-126)."""
    out = list(delta)
    for i in range(len(delta) // 2):
        out[2 * i], out[2 * i + 1] = r2.st_apply(stp, delta[2 * i], delta[2 * i + 1])
    return out


def stage_update(D, carts, sample_set, w, mean_shape, lbf=None):
    """btcart.cpp:285-292 with GenLBF's and GenDeltaShape's parameter (btcart.cpp:399, 422) -> (new shapes [n][2L], lbf [n][K])."""
    mc, _ = st_parameters(sample_set.shapes, mean_shape)
    base = 1 << (D - 1)
    shapes, lbfs = [], []
    for i in range(sample_set.n):
        if lbf is None:
            row = [k * base + r2.forward(_Depth(D), c, sample_set.patches[i], sample_set.shapes[i], mc[i]) for k, c in enumerate(carts)]
        else:
            row = [int(v) for v in lbf[i]]
        delta = apply_delta(mc[i], stage_ref.gen_delta_shape(row, w))
        shapes.append([s + d for s, d in zip(sample_set.shapes[i], delta)])
        lbfs.append(row)
    return shapes, lbfs


def shape_residual(gt, cur, idx, stp_cm, landmark_id=None):
    """Both DataSet::CalcShapeResidual overloads (data.cpp:175-208) with stp_cm[idx[i]] applied."""
    out = []
    for i in idx:
        d = [float(g) - float(c) for g, c in zip(gt[i], cur[i])]
        if landmark_id is None:
            out.append(apply_delta(stp_cm[i], d))
        else:
            out.append(list(r2.st_apply(stp_cm[i], d[2 * landmark_id], d[2 * landmark_id + 1])))
    return out


# ---- Validate from a start shape ---------------------------------------------------------------------------------------------

def validate_record(m2, o, h, q, start_shape):
    """model_ref.validate_record under the transform: every full stage starts with Calc(shape as it stands, mean_shape)
    (cascador.cpp:180); the partial stage keeps the stage before's parameter, the default when it is stage 0 -> (is_face, score,
    shape, n)."""
    patches = tuple((p, 0, 0, p.shape[1], p.shape[0]) for p in (o, h, q))
    shape = [float(v) for v in start_shape]
    score, n = 0.0, 0
    base = 1 << (m2.D - 1)
    stp = r2.IDENTITY
    for t in range(min(m2.stage_idx, m2.T)):
        stp = r2.st_calc(shape, m2.mean_shape, m2.L)
        lbf = []
        for k in range(m2.K):
            c = m2.carts[t][k]
            idx = r2.forward(m2, c, patches, shape, stp)
            score += c.scores[idx]
            score = (score - c.mean) / c.std
            n += 1
            if score < c.th:
                return False, score, shape, n
            lbf.append(k * base + idx)
        delta = apply_delta(stp, stage_ref.gen_delta_shape(lbf, m2.w[t]))
        shape = [shape[j] + delta[j] for j in range(2 * m2.L)]
    if m2.stage_idx < m2.T:
        for k in range(m2.cart_idx + 1):
            c = m2.carts[m2.stage_idx][k]
            idx = r2.forward(m2, c, patches, shape, stp)
            score += c.scores[idx]
            score = (score - c.mean) / c.std
            n += 1
            if score < c.th:
                return False, score, shape, n
    return True, score, shape, n


# ---- test data (shared by the host and the GPU tests) -------------------------------------------------------------------------

ODD = (9, 7, 5)                     # 81 + 49 + 25 = 155 bytes a record: no alignment at all
ROT_DEG, SCALES, NOISE = 30.0, (0.8, 1.25), 0.01


def make_shapes(seed, n, mean_shape, rot_deg=ROT_DEG, scales=SCALES, noise=NOISE):
    """Each sample's shape is the mean shape under its own rotation (+-rot_deg) and scale about the mean shape's centre, plus
    noise: the transform matters for every sample."""
    rng = np.random.default_rng(seed)
    pts = np.asarray(mean_shape, np.float64).reshape(-1, 2)
    ctr = pts.mean(0)
    out = np.zeros((n, pts.size))
    for i in range(n):
        a = math.radians(rng.uniform(-rot_deg, rot_deg))
        s = rng.uniform(*scales)
        R = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
        out[i] = (ctr + s * (pts - ctr) @ R.T + rng.normal(0, noise, pts.shape)).reshape(-1)
    return out


def make_samples(seed, n, mean_shape, sizes=ODD, **kw):
    """train_ref.make_samples' dict with make_shapes' shapes."""
    d = train_ref.make_samples(seed, n, len(mean_shape) // 2, sizes, **kw)
    d["shapes"] = make_shapes(seed + 1000, n, mean_shape)
    return d


def differing_share(s, pool, stp_mc):
    """Share of the (feature, sample) values that differ from the identity reading: the tests assert it above one half, on
    this restatement alone, so that they cannot pass vacuously."""
    idx = list(range(s.n))
    a = np.array(calc_feature_values(s, pool, idx, stp_mc))
    b = np.array(train_ref.calc_feature_values(s, pool, idx))
    return float((a != b).mean())
