"""Plain-Python, sequential restatement of what the reference's boosting loop does between two carts, the yardstick of
tests/test_boost_host.py and tests/test_boost_gpu.py (test infrastructure, not product; nothing under jda_amd/ imports
it), written from the reference's source: BoostCart::Train's loop body without the restart branch (src/jda/btcart.cpp:154-253)
and DataSet::UpdateWeights, UpdateScores, Swap, CalcThresholdByNumber, Remove, PreRemove, QSort / _QSort_, CalcMeanAndStd,
ApplyMeanAndStd (src/jda/data.cpp:255-448).  The cart itself is tests/train_ref.py's.  Python floats are IEEE doubles and
math.exp / math.sqrt are the host C library's: this is the bit-level yardstick.  Dialect CPP is parity-unpinned: the
reference itself needs OpenCV and cannot be built here."""
import math

import train_ref
from train_ref import fdiv


def cexp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def csqrt(x):
    return math.sqrt(x) if x >= 0 else math.nan


# ---- data.cpp, function by function (on plain lists) ------------------------------------------------------------------

def update_scores(scores, leaf, cart_scores):
    """DataSet::UpdateScores (data.cpp:305-317) -> (scores, last_scores)."""
    last = list(scores)
    return [s + cart_scores[l] for s, l in zip(scores, leaf)], last


def calc_mean_and_std(pos_scores, neg_scores):
    """DataSet::CalcMeanAndStd (data.cpp:420-441); std::pow(v, 2) as v * v (include/jda.h)."""
    n = len(pos_scores) + len(neg_scores)
    mean = 0.
    for s in pos_scores:
        mean += s
    for s in neg_scores:
        mean += s
    mean = fdiv(mean, float(n))
    var = 0.
    for s in pos_scores:
        v = s - mean
        var += v * v
    for s in neg_scores:
        v = s - mean
        var += v * v
    var = fdiv(var, float(n))
    return mean, csqrt(var)


def apply_mean_and_std(scores, mean, std):
    """DataSet::ApplyMeanAndStd (data.cpp:443-448)."""
    return [fdiv(s - mean, std) for s in scores]


def qsort(scores, swap=None):
    """DataSet::_QSort_ (data.cpp:385-410), recursion and all, on a copy of the scores and an index list (swap(i, j), if
    given, is called for every exchange: DataSet::Swap) -> (order, sorted scores)."""
    sc = list(scores)
    order = list(range(len(sc)))

    def rec(left, right):
        i, j = left, right
        t = sc[(left + right) // 2]
        while True:
            while sc[i] > t:
                i += 1
            while sc[j] < t:
                j -= 1
            if i <= j:
                sc[i], sc[j] = sc[j], sc[i]
                order[i], order[j] = order[j], order[i]
                if swap is not None:
                    swap(i, j)
                i += 1
                j -= 1
            if not i <= j:
                break
        if left < j:
            rec(left, j)
        if i < right:
            rec(i, right)
    if sc:
        rec(0, len(sc) - 1)
    return order, sc


def threshold_by_number(sorted_scores, remove):
    """DataSet::CalcThresholdByNumber (data.cpp:340-345)."""
    offset = len(sorted_scores) - 1 - remove
    if offset < 0:
        offset = 0
    return sorted_scores[offset]


def pre_remove(sorted_scores, th):
    """DataSet::PreRemove (data.cpp:371-378) -> the number of samples that Remove(th) would drop."""
    size = len(sorted_scores)
    offset = size - 1
    while offset >= 0 and sorted_scores[offset] < th:
        offset -= 1
    return size - 1 - offset


def remove(sorted_scores, th):
    """DataSet::Remove (data.cpp:347-369) -> the new size."""
    offset = len(sorted_scores) - 1
    while offset >= 0 and sorted_scores[offset] < th:
        offset -= 1
    return offset + 1


def update_weights(pos_scores, neg_scores, reverse=False):
    """DataSet::UpdateWeights(pos, neg) (data.cpp:255-303) -> (pos weights, neg weights, r = 1. / sum_w).  reverse=True adds
    both sums in REVERSED sample order: the control that summation order is visible in the bits."""
    pw = [cexp(-1. * s) for s in pos_scores]
    nw = [cexp(1. * s) for s in neg_scores]
    sum_pos_w = sum_neg_w = 0.
    for w in (reversed(pw) if reverse else pw):
        sum_pos_w += w
    for w in (reversed(nw) if reverse else nw):
        sum_neg_w += w
    sum_w = sum_pos_w + sum_neg_w
    r = fdiv(1., sum_w)
    return [w * r for w in pw], [w * r for w in nw], r


# ---- the loop ----------------------------------------------------------------------------------------------------------

class RefSet:
    """One DataSet as the loop sees it: per sample its patch bytes (a row of a numpy array), shape, optional residual row,
    score, last score and weight, and the is_sorted flag that makes QSort a no-op on a set nobody touched."""

    def __init__(self, patches, shapes, scores, residual=None):
        self.patches = [p for p in patches]
        self.shapes = [list(map(float, s)) for s in shapes]
        self.residual = None if residual is None else [tuple(map(float, r)) for r in residual]
        self.scores = [float(s) for s in scores]
        self.last = list(self.scores)
        self.weights = [0.] * len(self.scores)
        self.is_sorted = False
        self.orders = []                   # the order of every real sort, for the test's preconditions

    @property
    def size(self):
        return len(self.scores)

    def cols(self):
        return [c for c in (self.patches, self.shapes, self.residual, self.last, self.weights) if c is not None]

    def qsort(self):                       # DataSet::QSort, data.cpp:380-384
        if self.is_sorted or not self.size:
            self.is_sorted = True
            return

        def swap(i, j):                    # DataSet::Swap, data.cpp:319-333 (scores are exchanged by qsort itself)
            for c in self.cols():
                c[i], c[j] = c[j], c[i]
        before = list(self.scores)
        order, self.scores = qsort(self.scores, swap)
        self.orders.append((before, order))
        self.is_sorted = True

    def resize(self, n):                   # DataSet::Remove's resizes
        for c in self.cols() + [self.scores]:
            del c[n:]

    def append(self, patches, shapes, scores):          # what MoreNegSamples leaves: new samples at the end, unsorted
        self.patches += [p for p in patches]
        self.shapes += [list(map(float, s)) for s in shapes]
        self.scores += [float(s) for s in scores]
        self.last += [float(s) for s in scores]
        self.weights += [0.] * len(scores)
        self.is_sorted = False

    def sample_set(self, sizes):
        import numpy as np
        d = dict(patches=np.stack(self.patches), shapes=np.array(self.shapes), weights=np.array(self.weights),
                 residual=None if self.residual is None else np.array(self.residual), has_gt=None, sizes=sizes)
        if d["residual"] is None:
            d["residual"] = np.zeros((self.size, 2))
        return train_ref.ref_set(d)


def boost_loop(D, sizes, pos, neg, carts, drop_n, normalization_step, more_neg=None):
    """btcart.cpp:146-253 without the restart branch, K = len(carts) iterations.  carts[k] = (pools, modes, us) as
    train_ref.train_cart takes them; more_neg = {k: (patches, shapes, scores)}: the negatives that arrive at the top of
    iteration k (MoreNegSamples, btcart.cpp:149-152).  -> one dict per cart (everything the loop decided and the state of
    both sets after it), and the weights a further cart would start from."""
    out = []
    for k, (pools, modes, us) in enumerate(carts):
        kk = k + 1
        if more_neg and k in more_neg:
            neg.append(*more_neg[k])
        pos.qsort(); neg.qsort()                                               # btcart.cpp:154
        pos.weights, neg.weights, _ = update_weights(pos.scores, neg.scores)  # btcart.cpp:160
        start = dict(pos_weights=list(pos.weights), neg_weights=list(neg.weights), pos_patches=list(pos.patches),
                     neg_patches=list(neg.patches), pos_n=pos.size, neg_n=neg.size)
        cart = train_ref.train_cart(D, pos.sample_set(sizes), neg.sample_set(sizes), pools, modes, us)      # btcart.cpp:166
        pos.scores, pos.last = update_scores(pos.scores, cart["pos_leaf"], cart["scores"])                  # btcart.cpp:171-172
        neg.scores, neg.last = update_scores(neg.scores, cart["neg_leaf"], cart["scores"])
        pos.is_sorted = neg.is_sorted = False
        if kk % normalization_step == 0:                                       # btcart.cpp:173-181
            mean, std = calc_mean_and_std(pos.scores, neg.scores)
            pos.scores = apply_mean_and_std(pos.scores, mean, std)
            neg.scores = apply_mean_and_std(neg.scores, mean, std)
        else:
            mean, std = 0., 1.
        pos.qsort(); neg.qsort()                                               # btcart.cpp:183-184
        th = threshold_by_number(pos.scores, drop_n)                           # btcart.cpp:185
        pos_n, neg_n = pos.size, neg.size
        will_removed = pre_remove(neg.scores, th)                              # btcart.cpp:188
        pos.resize(remove(pos.scores, th))                                     # btcart.cpp:238-239
        neg.resize(remove(neg.scores, th))
        out.append(dict(start=start, cart=cart, th=th, mean=mean, std=std, will_removed=will_removed,
                        pos_drop=pos_n - pos.size, neg_drop=neg_n - neg.size,
                        pos=dict(patches=list(pos.patches), shapes=[list(s) for s in pos.shapes], scores=list(pos.scores),
                                 last=list(pos.last), residual=list(pos.residual)),
                        neg=dict(patches=list(neg.patches), shapes=[list(s) for s in neg.shapes], scores=list(neg.scores),
                                 last=list(neg.last))))
    final = update_weights(pos.scores, neg.scores)
    return out, final[:2]


# ---- test data ---------------------------------------------------------------------------------------------------------

TIES_4 = ([3., 2., 2., 1.], [0, 2, 1, 3])
TIES_8 = ([1.] * 8, [5, 4, 7, 6, 1, 0, 3, 2])


def sort_input(seed, n, halves):
    """Random normals, or -- halves -- normals rounded to halves (many ties).  For n >= 3 the rounded input is the first of
    the seeds seed, seed + 1, ... on which the quicksort above orders the ties differently from a stable sort, so that a
    test on it can tell the two apart (decided on this restatement alone)."""
    import numpy as np
    while True:
        s = np.random.default_rng(seed).normal(0, 1.5, n)
        if not halves:
            return s
        s = np.round(s * 2) / 2
        if n < 3 or qsort(s.tolist())[0] != np.argsort(-s, kind="stable").tolist():
            return s
        seed += 1
