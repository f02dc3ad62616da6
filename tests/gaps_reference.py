"""The nearest OTHER label and the gap table restated in numpy, two ways (no tests in here).

Definitions (include/pcseg_gaps.h): a site is a pixel whose label lies in 1 .. cap and is selected; for a pixel p, D2(p) is the
smallest squared distance to a site whose label differs from p's (raw integers), N(p) the smallest label among those sites at
that distance; -1 / 0 where there is none, or none with D2 <= r2 (r2 >= 0).  The gap of a live label l to type slot t is the
smallest D2 over the pixels of l with the live labels of slot t as the sites, its partner the smallest N at that minimum.

``nearest_other_label`` is brute force: every pixel against every site, the own label masked out -- no column candidates.
``nearest_other_label_by_zeroing`` goes through the existing restatement ``test_territory_cpu.nearest_label``: on a pixel that
carries no site's label the transform IS the nearest-label transform, and on the pixels of a site label l it is the
nearest-label transform of the image with l zeroed."""
import numpy as np

from test_territory_cpu import nearest_label, site_mask

BIG = np.int64(1) << 40


def nearest_other_label(lab, sel=None, cap=None, r2=-1):
    """(D2, N) of one (H, W) label image, int64"""
    lab = np.asarray(lab).astype(np.int64)
    H, W = lab.shape
    d2 = np.full((H, W), -1, np.int64)
    near = np.zeros((H, W), np.int64)
    qr, qc = np.nonzero(site_mask(lab, sel, cap))
    if qr.size == 0:
        return d2, near
    ql = lab[qr, qc]
    for r in range(H):
        d = (r - qr[None, :]) ** 2 + (np.arange(W)[:, None] - qc[None, :]) ** 2          # (W, sites)
        d = np.where(ql[None, :] != lab[r][:, None], d, BIG)
        if r2 >= 0:
            d = np.where(d <= r2, d, BIG)
        best = d.min(axis=1)
        who = np.where(d == best[:, None], ql[None, :], BIG).min(axis=1)
        ok = best < BIG
        d2[r], near[r] = np.where(ok, best, -1), np.where(ok, who, 0)
    return d2, near


def nearest_other_label_by_zeroing(lab, sel=None, cap=None, r2=-1):
    """the same through ``test_territory_cpu.nearest_label``"""
    lab = np.asarray(lab).astype(np.int64)
    sites = site_mask(lab, sel, cap)
    d2, near, _ = nearest_label(lab, sel, cap)  # right wherever the pixel carries no site's label
    for l in np.unique(lab[sites]):
        dl, nl, _ = nearest_label(np.where(lab == l, 0, lab), sel, cap)
        d2, near = np.where(lab == l, dl, d2), np.where(lab == l, nl, near)
    if r2 >= 0:
        far = d2 > r2
        d2, near = np.where(far, -1, d2), np.where(far, 0, near)
    return d2, near


def pair_gaps(lab, cap):
    """int64 (cap, cap): the smallest squared distance between a pixel of label i + 1 and one of label j + 1; -1 where one of
    them has no pixel, and on the diagonal"""
    lab = np.asarray(lab).astype(np.int64)
    out = np.full((cap, cap), -1, np.int64)
    px = {l: np.argwhere(lab == l) for l in range(1, cap + 1)}
    for i in range(1, cap + 1):
        for j in range(i + 1, cap + 1):
            if len(px[i]) and len(px[j]):
                d = ((px[i][:, None, :] - px[j][None, :, :]) ** 2).sum(axis=2)
                out[i - 1, j - 1] = out[j - 1, i - 1] = d.min()
    return out


def label_gaps(lab, live, slot_of, K, r2=-1):
    """(gap2, partner) int64 (cap, K) of one frame from the pairwise gaps: no transform at all"""
    live, slot_of = np.asarray(live).astype(bool), np.asarray(slot_of).astype(np.int64)
    cap = live.shape[0]
    pg = pair_gaps(lab, cap)
    gap2, partner = np.full((cap, K), -1, np.int64), np.zeros((cap, K), np.int64)
    for l in range(cap):
        if not live[l]:
            continue
        for t in range(K):
            cand = [(pg[l, m], m + 1) for m in range(cap)
                    if m != l and live[m] and slot_of[m] == t and pg[l, m] >= 0 and (r2 < 0 or pg[l, m] <= r2)]
            if cand:
                gap2[l, t], partner[l, t] = min(cand)
    return gap2, partner


def label_gaps_by_transform(lab, live, slot_of, K, r2=-1):
    """the same as the header states it: per slot the transform with that slot's live labels as the sites, then the
    lexicographic minimum of (D2, N) over the pixels of every live label"""
    lab = np.asarray(lab).astype(np.int64)
    live, slot_of = np.asarray(live).astype(bool), np.asarray(slot_of).astype(np.int64)
    cap = live.shape[0]
    gap2, partner = np.full((cap, K), -1, np.int64), np.zeros((cap, K), np.int64)
    for t in range(K):
        d2, near = nearest_other_label(lab, live & (slot_of == t), cap, r2)
        for l in np.nonzero(live)[0]:
            m = (lab == l + 1) & (d2 >= 0)
            if m.any():
                gap2[l, t], partner[l, t] = min(zip(d2[m].tolist(), near[m].tolist()))
    return gap2, partner


def gap_rows(frame_ids, labs, live, slot_of, K, scale, r2=-1, table=None):
    """float64 rows [frame, label, slot, gap_um.., gap_label.., gap_px2..] over the live rows in (frame, label) order;
    ``table``: the restatement of the table to go through (default: ``label_gaps``)"""
    rows = []
    for b in range(len(labs)):
        gap2, partner = (table or label_gaps)(labs[b], live[b], slot_of[b], max(K, 1), r2)
        for l in np.nonzero(np.asarray(live[b]).astype(bool))[0]:
            g = gap2[l, :K].astype(np.float64)
            some = g >= 0
            um = np.where(some, np.sqrt(np.where(some, g, 0.0)) / np.float64(scale), np.nan)
            s = int(slot_of[b][l])
            rows.append([float(frame_ids[b]), float(l + 1), float(s) if s < 4 else -1.0] + list(um)
                        + list(np.where(some, partner[l, :K], -1).astype(np.float64)) + list(g))
    return np.array(rows, np.float64).reshape(len(rows), 3 + 3 * K)


def check_symmetry(gap2, partner, live, slot_of, K):
    """the table against itself: with m = partner[l, t] and s = slot_of[l] < K, gap2[m, s] <= gap2[l, t] (the pair (m, l) is a
    candidate of m's), equal where m's partner of slot s is l, and where equal m's partner is not larger than l"""
    gap2, partner = np.asarray(gap2), np.asarray(partner)
    n = 0
    for l in np.nonzero(np.asarray(live).astype(bool))[0]:
        s = int(slot_of[l])
        for t in range(K):
            m = int(partner[l, t])
            if m == 0:
                assert gap2[l, t] == -1
                continue
            assert m != l + 1 and live[m - 1] and slot_of[m - 1] == t and gap2[l, t] >= 1, (l, t, m)
            if s < K:
                assert 1 <= gap2[m - 1, s] <= gap2[l, t], (l, t, m)
                if partner[m - 1, s] == l + 1:
                    assert gap2[m - 1, s] == gap2[l, t], (l, t, m)
                if gap2[m - 1, s] == gap2[l, t]:
                    assert partner[m - 1, s] <= l + 1, (l, t, m)
                n += 1
    return n
