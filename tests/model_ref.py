"""The model in training, restated in plain Python: what jdaCascadorCreateTrainingCpp / jdaModelPutCartCpp /
jdaModelCloseStageCpp keep and what jdaCascadorSerializeToCpp writes (include/jda.h, "Dialect CPP: the model in training").
The file goes through jda_amd.synth.Model.tobytes, which was written from the reference's layout (cascador.cpp:79-124,
cart.cpp:429-450) independently of the library's writer.  validate_record is JoinCascador::Validate (cascador.cpp:166-211)
on a sample record's three patches from a given start shape, sequentially, on oracle/cpp_reading2.py's forward."""
import os
import tempfile

import numpy as np

from jda_amd import synth


class GrowModel:
    """JoinCascador::JoinCascador()'s model (cascador.cpp:17-29; cart.cpp:23-37, btcart.cpp:104-116: everything zero, std 1;
    Cart::th, which the reference leaves uninitialised, 0) with put / close / status."""

    def __init__(self, T, K, L, D, mean_shape):
        self.m = synth.Model(T, K, L, D)
        self.m.mean_shape = np.array(mean_shape, np.float64).reshape(2 * L)
        self.stage, self.cart = 0, -1

    def status(self):
        return self.stage, self.cart

    def put(self, k, features, thresholds, leaf_scores, th, mean=0., std=1.):
        m, t = self.m, self.stage
        assert t < m.T and (k == self.cart + 1 and k < m.K or k == self.cart and k >= 0)
        f = np.asarray(features)
        # slot i - 1 is node i = 1 .. nodes_n/2 - 1: Cart::SerializeTo's loop (cart.cpp:431-441)
        m.scale[t, k] = f["scale"]; m.lm1[t, k] = f["landmark_id1"]; m.lm2[t, k] = f["landmark_id2"]
        m.off[t, k, :, 0] = f["offset1_x"]; m.off[t, k, :, 1] = f["offset1_y"]
        m.off[t, k, :, 2] = f["offset2_x"]; m.off[t, k, :, 3] = f["offset2_y"]
        m.nth[t, k] = thresholds
        m.leaf[t, k] = leaf_scores
        m.cth[t, k], m.cmean[t, k], m.cstd[t, k] = th, mean, std
        self.cart = k

    def close(self, w):
        m = self.m
        assert self.stage < m.T and self.cart == m.K - 1
        m.w[self.stage] = np.asarray(w, np.float64).reshape(m.K * m.leaf_n, m.dim)
        self.stage, self.cart = self.stage + 1, -1

    def tobytes(self):
        return self.m.tobytes(8, self.stage, self.cart)

    def save(self, path):
        with open(path, "wb") as f:
            f.write(self.tobytes())
        return path


def cart_of(model, t, k):
    """Cart (t, k) of a synth.Model as put_cart_cpp's arguments: (features, thresholds, leaf_scores, th, mean, std)."""
    from jda_amd import api
    f = np.zeros(model.node_n, api.FEATURE_DTYPE)
    f["scale"], f["landmark_id1"], f["landmark_id2"] = model.scale[t, k], model.lm1[t, k], model.lm2[t, k]
    f["offset1_x"], f["offset1_y"] = model.off[t, k, :, 0], model.off[t, k, :, 1]
    f["offset2_x"], f["offset2_y"] = model.off[t, k, :, 2], model.off[t, k, :, 3]
    return f, model.nth[t, k].copy(), model.leaf[t, k].copy(), float(model.cth[t, k]), float(model.cmean[t, k]), float(model.cstd[t, k])


def model2_of(blob):
    """oracle.cpp_reading2.Model2 of a model's bytes."""
    from oracle import cpp_reading2 as r2
    fd, p = tempfile.mkstemp(suffix=".model")
    try:
        with os.fdopen(fd, "wb") as f:
            f.write(blob)
        return r2.Model2(p)
    finally:
        os.unlink(p)


def validate_record(m2, o, h, q, start_shape):
    """Validate on one record (o, h, q: 2-D uint8 patches as stored) from start_shape, the similarity transform off ->
    (is_face, score, shape, n)."""
    from oracle import cpp_reading2 as r2
    patches = tuple((p, 0, 0, p.shape[1], p.shape[0]) for p in (o, h, q))
    shape = [float(v) for v in start_shape]
    score, n = 0.0, 0
    base = 1 << (m2.D - 1)
    for t in range(min(m2.stage_idx, m2.T)):
        lbf = []
        for k in range(m2.K):
            c = m2.carts[t][k]
            idx = r2.forward(m2, c, patches, shape, r2.IDENTITY)
            score += c.scores[idx]
            score = (score - c.mean) / c.std
            n += 1
            if score < c.th:
                return False, score, shape, n
            lbf.append(k * base + idx)
        delta = [0.0] * (2 * m2.L)
        for k in range(m2.K):
            row = m2.w[t][lbf[k]]
            for j in range(2 * m2.L):
                delta[j] += row[j]
        shape = [shape[j] + delta[j] for j in range(2 * m2.L)]
    if m2.stage_idx < m2.T:
        for k in range(m2.cart_idx + 1):
            c = m2.carts[m2.stage_idx][k]
            idx = r2.forward(m2, c, patches, shape, r2.IDENTITY)
            score += c.scores[idx]
            score = (score - c.mean) / c.std
            n += 1
            if score < c.th:
                return False, score, shape, n
    return True, score, shape, n
