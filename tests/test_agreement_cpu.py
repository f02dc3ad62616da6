"""The agreement of two label images (csrc/agreement.hip, ops.label_contingency / label_agreement) restated in numpy and
Python integers, checked against scikit-image 0.18.3's contingency_table, adapted_rand_error and variation_of_information
(tests/golden/agreement.npz).  The GPU tests import the restatement.  No GPU here."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

from conftest import load_golden

THRESHOLDS = (0.5, 0.75, 0.9)
SCORES = ("tp", "fp", "fn", "precision", "recall", "f1", "ap", "mean_matched_iou")
NAN = np.float64(np.nan)


# ---- the restatement
def pair_rows(T, S, cap_t, cap_s):
    """One frame: the pairs (t, s, n) with n > 0 except (0, 0), sorted by (t, s), and the overflow bits a value can raise.
    A value outside 0 .. cap is read as 0; one above the cap raises bit 2 (value 2)."""
    T, S = np.asarray(T).astype(np.int64), np.asarray(S).astype(np.int64)
    over = 2 if (T > cap_t).any() or (S > cap_s).any() else 0
    t = np.where((T < 0) | (T > cap_t), 0, T)
    s = np.where((S < 0) | (S > cap_s), 0, S)
    code, n = np.unique(t * (cap_s + 1) + s, return_counts=True)
    keep = code != 0
    return code[keep] // (cap_s + 1), code[keep] % (cap_s + 1), n[keep].astype(np.int64), over


def better(n1, u1, p1, n2, u2, p2):
    """Is partner p1 (overlap n1, union u1) a better partner than p2?  The larger n / u, exactly; then the smaller label."""
    a, c = int(n1) * int(u2), int(n2) * int(u1)
    return a > c or (a == c and p1 < p2)


def match_rows(t, s, n, cap_t, cap_s, thresholds=THRESHOLDS):
    """One frame's arrays of pcseg_agreement_match from its pair rows (include/pcseg.h)."""
    t, s, n = (np.asarray(v).astype(np.int64) for v in (t, s, n))
    A, Bs = np.zeros(cap_t + 1, np.int64), np.zeros(cap_s + 1, np.int64)
    np.add.at(A, t, n)
    np.add.at(Bs, s, n)
    K = len(thresholds)
    out = {"area_t": A[1:].copy(), "area_s": Bs[1:].copy(),
           "best_t": np.zeros((cap_t, 3), np.int32), "best_s": np.zeros((cap_s, 3), np.int32),
           "iou_t": np.full(cap_t, NAN), "iou_s": np.full(cap_s, NAN),
           "match_t": np.zeros(cap_t, np.uint8), "match_s": np.zeros(cap_s, np.uint8)}
    cand_t, cand_s = {}, {}
    for ti, si, ni in zip(t.tolist(), s.tolist(), n.tolist()):
        if ti >= 1 and si >= 1:
            u = int(A[ti] + Bs[si] - ni)
            for cand, own, partner in ((cand_t, ti, si), (cand_s, si, ti)):
                cur = cand.get(own)
                if cur is None:
                    cand[own] = [ni, u, partner, 1]
                else:
                    cur[3] += 1
                    if better(ni, u, partner, cur[0], cur[1], cur[2]):
                        cur[:3] = [ni, u, partner]
    tp = [0] * K
    for side, cand in (("t", cand_t), ("s", cand_s)):
        for own, (ni, u, partner, count) in cand.items():
            out["best_" + side][own - 1] = (partner, ni, count)
            iou = np.float64(ni) / np.float64(u)
            out["iou_" + side][own - 1] = iou
            bits = 0
            for k, tau in enumerate(thresholds):
                if 2 * ni > u and iou >= tau:
                    bits |= 1 << k
                    tp[k] += side == "t"
            out["match_" + side][own - 1] = bits
    fg = t >= 1
    col = np.zeros(cap_s + 1, np.int64)  # the sum over t >= 1 of n(t, s)
    np.add.at(col, s[fg], n[fg])
    out["frame_ints"] = np.array([int((A[1:] > 0).sum()), int((Bs[1:] > 0).sum()), int(A[1:].sum()), int((n[fg] ** 2).sum()),
                                  int((A[1:] ** 2).sum()), int((col ** 2).sum())] + tp, np.int64)
    return out


def frame_scores(m, t, s, n, n_px, thresholds=THRESHOLDS):
    """One frame's scores from the integers, float64, a zero denominator giving what IEEE gives."""
    f64 = np.float64
    n_truth, n_rois, N1, S_pp, S_a, S_b = (int(v) for v in m["frame_ints"][:6])
    out = {k: np.zeros(len(thresholds)) for k in SCORES}
    with np.errstate(all="ignore"):
        for k in range(len(thresholds)):
            tp = int(m["frame_ints"][6 + k])
            ious = [float(v) for v, bits in zip(m["iou_t"], m["match_t"]) if (bits >> k) & 1]
            assert len(ious) == tp
            out["tp"][k], out["fp"][k], out["fn"][k] = tp, n_rois - tp, n_truth - tp
            out["precision"][k] = f64(tp) / f64(n_rois)
            out["recall"][k] = f64(tp) / f64(n_truth)
            out["f1"][k] = f64(2 * tp) / f64(n_truth + n_rois)
            out["ap"][k] = f64(tp) / f64(n_truth + n_rois - tp)
            out["mean_matched_iou"][k] = f64(math.fsum(ious)) / f64(tp)
        p2 = S_pp - N1
        prec = f64(p2) / f64(S_a - N1)
        rec = f64(p2) / f64(S_b - N1)
        f = 2. * prec * rec / (prec + rec)
        out["are"], out["are_precision"], out["are_recall"] = 1. - f, prec, rec
    # variation of information: every pair, label 0 on both sides and n(0, 0) included
    pairs = [(int(a), int(b), int(c)) for a, b, c in zip(t, s, n)]
    n00 = n_px - sum(c for _, _, c in pairs)
    if n00 > 0:
        pairs.append((0, 0, n00))
    At, Bs = {}, {}
    for a, b, c in pairs:
        At[a] = At.get(a, 0) + c
        Bs[b] = Bs.get(b, 0) + c
    out["vi_split"] = f64(-math.fsum((c / n_px) * math.log2(c / At[a]) for a, b, c in pairs))
    out["vi_merge"] = f64(-math.fsum((c / n_px) * math.log2(c / Bs[b]) for a, b, c in pairs))
    out["n_pairs"] = len(pairs)
    return out


def agreement(T, S, thresholds=THRESHOLDS, cap_t=None, cap_s=None):
    """ops.label_agreement restated for a batch (B, H, W): the same keys, numpy arrays, ``scores`` stacked over the frames."""
    T, S = np.asarray(T), np.asarray(S)
    B, H, W = T.shape
    cap_t = max(int(T.max()), 1) if cap_t is None else cap_t
    cap_s = max(int(S.max()), 1) if cap_s is None else cap_s
    per, rows, scores, over = [], [], [], []
    for b in range(B):
        t, s, n, o = pair_rows(T[b], S[b], cap_t, cap_s)
        m = match_rows(t, s, n, cap_t, cap_s, thresholds)
        per.append(m)
        rows.append((np.full(len(t), b, np.int64), t, s, n))
        scores.append(frame_scores(m, t, s, n, H * W, thresholds))
        over.append(o)
    out = {k: np.stack([m[k] for m in per]) for k in per[0]}
    for i, k in enumerate(("frame", "t", "s", "n")):
        out[k] = np.concatenate([r[i] for r in rows])
    out["scores"] = {k: np.stack([np.asarray(sc[k]) for sc in scores]) for k in scores[0]}
    out["overflow"] = np.array(over, np.int32)
    out["pairs_per_frame"] = np.array([len(r[1]) for r in rows])
    return out


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def same_floats(a, b):
    """Equal by their bits, any NaN equal to any NaN (a NaN carries no value; its sign depends on the operation that made it)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


# ---- against the library
@pytest.fixture(scope="module")
def golden():
    return load_golden("agreement")


def golden_names(g):
    return [str(n) for n in g["names"]]


def test_fixture_covers_the_listed_situations(golden):
    names = golden_names(golden)
    assert len(names) >= 12
    for want in ("identical", "disjoint", "empty_test", "empty_truth", "over", "under", "shift", "random"):
        assert want in names
    for n in names:
        assert golden["t_" + n].shape == golden["s_" + n].shape and golden["t_" + n].shape[0] <= 96 and golden["t_" + n].shape[1] <= 80


def test_table_equals_the_librarys(golden):
    for name in golden_names(golden):
        T, S, ct = golden["t_" + name], golden["s_" + name], golden["ct_" + name]
        cap_t, cap_s = ct.shape[0] - 1, ct.shape[1] - 1
        t, s, n, over = pair_rows(T, S, max(cap_t, 1), max(cap_s, 1))
        assert over == 0
        dense = np.zeros_like(ct)
        dense[t, s] = n
        dense[0, 0] = T.size - n.sum()
        assert np.array_equal(dense, ct), name
        m = match_rows(t, s, n, max(cap_t, 1), max(cap_s, 1))
        assert np.array_equal(m["area_t"][:cap_t], ct.sum(axis=1)[1:]) and np.array_equal(m["area_s"][:cap_s], ct.sum(axis=0)[1:]), name


def test_adapted_rand_error_by_its_bits(golden):
    for name in golden_names(golden):
        T, S = golden["t_" + name], golden["s_" + name]
        r = agreement(T[None], S[None])["scores"]
        got = np.array([r["are"][0], r["are_precision"][0], r["are_recall"][0]])
        assert same_floats(got, golden["are_" + name]), (name, got, golden["are_" + name])


def test_variation_of_information_within_the_derived_bound(golden):
    """|delta| <= 2^-52 (16 + 2 P max(1, value)), P = pairs with n > 0: every term is >= 0, a term's absolute error is a few
    eps times its weight n / HW and the weights sum to 1; the library's own unsorted sum over P terms adds at most P eps value."""
    for name in golden_names(golden):
        T, S = golden["t_" + name], golden["s_" + name]
        r = agreement(T[None], S[None])["scores"]
        P = int(r["n_pairs"][0])
        assert P == int((golden["ct_" + name] > 0).sum())
        for got, want in zip((r["vi_split"][0], r["vi_merge"][0]), golden["vi_" + name]):
            bound = 2.0 ** -52 * (16 + 2 * P * max(1.0, float(want)))
            assert abs(float(got) - float(want)) <= bound, (name, got, want, bound)


# ---- best partner and match
def near_tie_rows():
    """Truth label 1 with two partners whose IoUs are different fractions and the same float64: n(1, 1) / U_1 < n(1, 2) / U_2,
    so the right partner is 2, while float IoUs with the smaller-label rule would say 1.  Areas of some 2^28 pixels: rows only,
    no image.  U_s = A_1 + n(0, s)."""
    # n11 / U1 = m / (3 m + 1) and n12 / U2 = (m + 1) / (3 m + 4): the cross products differ by exactly 1
    m, n10 = 250000000, 5
    n11, n12 = m, m + 1
    U1, U2 = 3 * m + 1, 3 * m + 4
    assert n12 * U1 - n11 * U2 == 1
    A1 = n11 + n12 + n10
    x1, x2 = U1 - A1, U2 - A1
    assert x1 > 0
    t = np.array([0, 0, 1, 1, 1])
    s = np.array([1, 2, 0, 1, 2])
    n = np.array([x1, x2, n10, n11, n12])
    return t, s, n, (n11, U1), (n12, U2)


def test_cross_multiplication_agrees_with_fractions_on_a_near_tie():
    t, s, n, (n1, U1), (n2, U2) = near_tie_rows()
    assert np.float64(n1) / np.float64(U1) == np.float64(n2) / np.float64(U2)  # the floats cannot tell them apart
    assert Fraction(n1, U1) < Fraction(n2, U2)
    assert int(n.sum()) < 2 ** 30
    m = match_rows(t, s, n, 1, 2)
    assert m["best_t"][0].tolist() == [2, n2, 2]
    assert better(n2, U2, 2, n1, U1, 1) and not better(n1, U1, 1, n2, U2, 2)
    # and on random rows: the partner chosen is the maximum of (Fraction, -label)
    rng = np.random.default_rng(5)
    for _ in range(20):
        T, S = rng.integers(0, 7, (12, 9)), rng.integers(0, 6, (12, 9))
        t, s, n, _ = pair_rows(T, S, 6, 5)
        m = match_rows(t, s, n, 6, 5)
        A, Bs = np.bincount(T.ravel(), minlength=7), np.bincount(S.ravel(), minlength=6)
        for l in range(1, 7):
            cands = [(Fraction(int(c), int(A[l] + Bs[b] - c)), -int(b), int(c)) for a, b, c in zip(t, s, n) if a == l and b >= 1]
            want = [-max(cands)[1], max(cands)[2], len(cands)] if cands else [0, 0, 0]
            assert m["best_t"][l - 1].tolist() == want


def test_match_is_best_partner_with_majority_overlap_and_iou(golden):
    for name in golden_names(golden):
        T, S = golden["t_" + name].astype(np.int64), golden["s_" + name].astype(np.int64)
        r = agreement(T[None], S[None])
        A, Bs = np.bincount(T.ravel()), np.bincount(S.ravel())
        tp = [0] * len(THRESHOLDS)
        for l in range(1, len(A)):
            # every partner that qualifies, found without reference to "best": there is at most one, and it is the best
            for k, tau in enumerate(THRESHOLDS):
                hits = []
                for p in range(1, len(Bs)):
                    c = int(((T == l) & (S == p)).sum())
                    u = int(A[l] + Bs[p] - c)
                    if c and 2 * c > u and np.float64(c) / np.float64(u) >= tau:
                        hits.append(p)
                assert len(hits) <= 1
                matched = (int(r["match_t"][0, l - 1]) >> k) & 1
                assert matched == len(hits), (name, l, k)
                if hits:
                    assert r["best_t"][0, l - 1, 0] == hits[0]
                    assert (int(r["match_s"][0, hits[0] - 1]) >> k) & 1 and r["best_s"][0, hits[0] - 1, 0] == l
                    tp[k] += 1
        assert r["frame_ints"][0, 6:].tolist() == tp, name
        assert int(r["match_s"].astype(bool).sum()) == int(r["match_t"].astype(bool).sum())


def test_scores_of_identical_and_empty_frames(golden):
    T = golden["t_identical"]
    sc = agreement(T[None], T[None])["scores"]
    assert np.all(sc["ap"] == 1.0) and np.all(sc["f1"] == 1.0) and np.all(sc["mean_matched_iou"] == 1.0)
    assert sc["are"][0] == 0.0 and sc["vi_split"][0] == 0.0 and sc["vi_merge"][0] == 0.0
    Z = np.zeros((1, 5, 7), np.int32)
    sc = agreement(Z, Z)["scores"]
    assert np.all(np.isnan(sc["precision"])) and np.all(np.isnan(sc["ap"])) and np.isnan(sc["are"][0]) and sc["vi_split"][0] == 0.0


# ---- the C ABI (fails without the feature)
def test_contingency_workspace_query_and_argument_checks():
    """Argument and workspace checks come before the first device call: nothing here touches a device."""
    from particle_col_image_segmentation_amd import build
    build.build()
    from particle_col_image_segmentation_amd import _lib
    lib = _lib.load()
    need = lib.pcseg_contingency_workspace_bytes(2, 1024)
    assert need > 0 and need % 256 == 0
    assert need >= 2 * 1024 * (8 + 4)
    assert lib.pcseg_contingency_workspace_bytes(0, 1024) == 0 and lib.pcseg_contingency_workspace_bytes(2, 0) == 0
    p = ctypes.c_void_p(4096)
    B, H, W = 2, 96, 80
    rc = lib.pcseg_label_contingency(p, p, 16, 16, 1024, p, p, p, B, H, W, p, need - 1, None)
    assert rc == -3 and b"workspace too small" in lib.pcseg_last_error()
    rc = lib.pcseg_label_contingency(None, None, 16, 16, 1024, p, p, p, B, H, W, p, need, None)
    assert rc == -1 and b"bad arguments" in lib.pcseg_last_error()
    assert lib.pcseg_contingency_write(1024, p, p, p, p, B, p, need - 1, None) == -3
    assert lib.pcseg_contingency_write(1024, None, p, p, p, B, p, need, None) == -1
    thr = (ctypes.c_double * 1)(0.25)  # a threshold below 0.5 would let a label have two matches
    rc = lib.pcseg_agreement_match(p, p, p, 1, 4, 4, ctypes.cast(thr, ctypes.c_void_p), 1, p, p, p, p, p, p, p, p, p, 1, None)
    assert rc == -1 and b"threshold" in lib.pcseg_last_error()
