"""The crafted class maps of class_map_patterns.py are what they are meant to be: the preconditions of
test_gpu_classify_tables.py, checked with the oracle alone (no GPU)."""
import itertools

import numpy as np
import pytest

import class_map_patterns as cmp_
from oracle import oracle as orc

CLS_CHUNK = 1024   # regions per round of the placement loop of classify_regions_kernel (csrc/reduce.hip)
TABLE_CHUNK = 256  # rows per round of the writers of table_write_kernel (csrc/tables.hip)


def all_frames():
    out = list(cmp_.frames3().values()) + list(cmp_.frames4().values())
    return out + [cmp_.frame_nan(), cmp_.frame_nan(sibling=True)]


@pytest.mark.parametrize("frame", all_frames(), ids=lambda f: f.name)
def test_regions_are_as_asked(frame):
    """One component per item, in raster order after the background, of exactly the item's class and area, and no two
    of them 8-connected (the components of "not background" are as many as the items)."""
    lab, n = orc.label(frame.cm, return_num=True)
    assert n == len(frame.items) + 1
    tab = orc.region_table(lab, n)
    assert lab[0, 0] == 1 and frame.cm[0, 0] == cmp_.BACKGROUND
    assert tab[0, 0] == frame.cm.size - sum(a for _, a in frame.items)
    np.testing.assert_array_equal(tab[1:, 0], [a for _, a in frame.items])
    np.testing.assert_array_equal(frame.cm.ravel()[tab[1:, 7]], [v for v, _ in frame.items])
    assert (np.diff(tab[1:, 7]) > 0).all()
    assert orc.label(frame.cm != cmp_.BACKGROUND, return_num=True)[1] == len(frame.items)


def test_strip_map_gaps():
    """A gap of up to 4 columns joins two neighbours under the disk(2) dilation of the merges, 5 do not."""
    assert orc.CELL_CLUSTER_DISTANCE_THRESHOLD // 2 == 2
    for gap, joined in ((1, True), (4, True), (5, False), (6, False)):
        cm, bg = cmp_.strip_map([(1, 21), (1, 30)], 5, (16, 64), gaps=[6, gap])
        assert bg == 1
        n = orc.label(orc.binary_dilation_disk(cm == 1, 2), return_num=True)[1]
        assert n == (1 if joined else 2), gap
    with pytest.raises(ValueError):
        cmp_.strip_map([(1, 400)], 5, (16, 64))


def test_oracle_returns_or_raises():
    for name, e in itertools.chain(cmp_.expectations3().items(), cmp_.expectations4().items()):
        assert not e["nan"], name
    nan = cmp_.frame_nan()
    with pytest.raises(ValueError, match="cannot convert float NaN to integer"):
        orc.get_cell_positions_and_areas(nan.cm, nan.cell_types, merged=True)
    e = cmp_.expectation_nan(nan, cmp_.frame_nan(sibling=True))
    assert e["names"][e["nan_slot"]] == "6B07" and (~e["mean_free"]).sum() == 2
    for s in (0, 2):
        assert e["type_stats"][s, 0] > 0 and e["type_stats"][s, 1] > 0


def test_thresholds_frame():
    e = cmp_.expectations3()["a_thresholds"]
    items = cmp_.frames3()["a_thresholds"].items
    kind = e["classes"]["kind"]
    for v, name in ((1, "3D05"), (2, "6B07"), (4, "C3M10")):
        mc, mk = cmp_.thresholds(name)
        got = {a: int(kind[k + 1]) for k, (val, a) in enumerate(items) if val == v}
        assert got == {mc - 1: 0, mc: 1, mk - 1: 1, mk: 2, mk + 1: 2}
    assert sum(1 for v, _ in items if v == 3) == 2 and e["particle_area"] == sum(a for v, a in items if v == 3)
    # the type that is present only below the minimum cell area: listed, count 0
    e = cmp_.expectations3()["a_absent"]
    assert e["order"] == ["6B07", "3D05"] and e["counts"][0]["6B07"] == 0 and e["type_stats"][1, :3].tolist() == [0, 0, 0]
    assert e["type_stats"][1, 3] == 1 and e["type_stats"][2, 3] == cmp_.NO_REGION
    e = cmp_.expectations3()["no_cells_particles"]
    assert e["order"] == ["3D05"] and not e["classes"]["kind"].any()
    assert not cmp_.expectations3()["no_cells_background"]["classes"]["kind"].any()


def floor_division_tally():
    """(exact, one less) over the clusters of frame (b) that are an exact multiple of their type's mean cell area, from
    the oracle's ``cells``"""
    fr, e = cmp_.frames3()["b_floor_division"], cmp_.expectations3()["b_floor_division"]
    exact = less = 0
    for v, (cells, mult) in cmp_.floor_division_sets().items():
        name = fr.cell_types[v]
        assert sorted(r.area for r in e["cell_pos"][name]) == sorted(cells)
        got = {r.area: r.cells for r in e["cell_clusters"][name]}
        S, n = sum(cells), len(cells)
        for C, q, f in mult:
            assert C * n == q * S and got[C] == f and f in (q, q - 1)
            exact += f == q
            less += f == q - 1
        # one pixel below / above a multiple: the quotient of the lower multiple (or of the one before it)
        assert len(got) == len(mult) + 2
    return exact, less


def test_floor_division_kinds():
    exact, less = floor_division_tally()
    assert exact >= 8 and less >= 8, (exact, less)
    # the issue's own examples
    assert np.float64(248) // (np.float64(62) / np.float64(3)) == 11 and np.float64(300) // np.float64(30) == 10
    sets = cmp_.floor_division_sets()
    assert len({cells for cells, _ in sets.values()}) == 3
    # floor(a / b) would say otherwise for every "one less" cluster
    cells, mult = sets[1]
    avg = np.float64(sum(cells)) / np.float64(len(cells))
    assert all(np.floor(np.float64(C) / avg) == q for C, q, _ in mult)


def test_type_orders():
    orders = []
    below = 0
    for name, e in cmp_.expectations3().items():
        if not name.startswith("c_order_"):
            continue
        orders.append(tuple(e["order"]))
        first = e["type_stats"][:3, 3]
        assert [e["names"][s] for s in np.argsort(first)] == e["order"]
        below += int((e["classes"]["kind"][first] == 0).sum())
        # the combined list follows the order of first appearance, not the slot order
        assert e["lists"][4].tolist() == [r for n in e["order"] for r in e["lists"][e["names"].index(n)].tolist()]
    assert sorted(orders) == sorted(itertools.permutations(["3D05", "6B07", "C3M10"]))
    assert below == 9  # (half of the 18 first regions are below the minimum cell area)


@pytest.mark.parametrize("name,slots", [("e_many", 3), ("e_many_four", 4)])
def test_many_regions(name, slots):
    e = (cmp_.expectations3() if slots == 3 else cmp_.expectations4())[name]
    kind, slot_of = e["classes"]["kind"], e["classes"]["slot_of"]
    assert len(e["lists"][4]) > 2048 and e["n"] > 2 * CLS_CHUNK
    rows = np.nonzero(kind)[0]
    assert len(rows) > TABLE_CHUNK * 8
    # every (slot, kind) list has members in each of the three rounds of the placement loop
    for s in range(slots):
        for k in (1, 2):
            r = np.nonzero((kind == k) & (slot_of == s))[0]
            assert set(r // CLS_CHUNK) == {0, 1, 2}, (s, k)
    # ... and the cell rows of every 256-region round of the writer are some, not all (the compaction has work)
    per_round = np.bincount(rows // TABLE_CHUNK, minlength=-(-e["n"] // TABLE_CHUNK))
    assert (per_round > 0).all() and (per_round[:-1] < TABLE_CHUNK).all()
    assert (e["classes"]["kind"] == 0).sum() > 100 and e["particle_area"] > 0


def group_kinds(e):
    """(groups of "combined" with members of two types, groups with a cell and a cluster, regions alone in their group)"""
    kind, slot_of = e["classes"]["kind"], e["classes"]["slot_of"]
    two = mixed = alone = 0
    for s, g in e["groups"].items():
        for i in range(len(g["area"])):
            mem = g["members"][g["offsets"][i]:g["offsets"][i + 1]] - 1
            two += s == 4 and len(set(slot_of[mem])) > 1
            mixed += len(set(kind[mem])) > 1
            alone += len(mem) == 1
    return two, mixed, alone


def test_groups_are_not_trivial():
    two, mixed, alone = group_kinds(cmp_.expectations3()["a_thresholds"])
    assert two >= 1 and mixed >= 1 and alone >= 1
    for name, e in cmp_.expectations3().items():
        if name.startswith("c_order_") or name == "e_many":
            two, mixed, alone = group_kinds(e)
            assert two >= 1 and mixed >= 1, name
    e = cmp_.expectations4()["f_four_slots"]
    two, mixed, alone = group_kinds(e)
    assert two >= 1 and mixed >= 1 and alone >= 1 and len(e["names"]) == 4 and all(len(l) for l in e["lists"])
    # a region of the second class value of 6B07 is listed but not in the type's mask: dropped unless a neighbour's
    # dilation covers its centroid
    listed = len(e["lists"][1])
    grouped = len(e["groups"][1]["members"])
    assert grouped < listed
