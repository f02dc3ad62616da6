"""The argument contract of ``ops``: one valid call of every public function that takes a tensor, and the refused calls that
are generated from it (no tests in here; ``test_ops_contract_cpu.py`` runs the table on CPU tensors with the device predicate
replaced, ``test_gpu_ops_contract.py`` on device tensors with the predicate as it is).

No call of this table ever enters the library: :func:`install` replaces ``ops._call`` and ``ops._workspace`` -- the only two
ways into it -- by a hook that raises :class:`Reached`.  The valid call must raise ``Reached`` (the checks do not over-refuse);
a mutated call must raise its ``TypeError`` / ``ValueError`` first.  Only dtypes and shapes matter: every tensor is zeros.

An entry states the tensor arguments of its call with SYMBOLIC shapes (``"B", "H", "W"``, an int for a fixed size).  Two
arguments that use one symbol must agree on it, and so must an argument and whatever the entry lists under ``bound`` (a size
that is also passed as a number, or derived: ``H32`` = ceil(H / 32), ``B1`` = B + 1).  From that the mutations follow, one
argument changed at a time:

- ``foreign``: the tensor on another device (a CPU tensor in the GPU run, a ``meta`` tensor in the CPU run): TypeError
- ``numpy``: a numpy array in its place: TypeError
- ``dtype:<d>``: the neighbouring dtype(s) (int32 <-> int64, uint8 <-> int32, float32 <-> float64) the entry does not list as
  accepted -- where it accepts them all, the nearest dtype it does not: TypeError
- ``rank+`` / ``rank-``: one dimension more (a leading one) or one fewer (the first frame): ValueError, or TypeError where the
  argument is stated with ``rank=TypeError`` (``_label_batch``, ``_plane_view``, ``_h_extrema`` and ``peel`` have always raised
  that); left out where the entry accepts that rank
- ``axis<i>``: every axis whose size is bound, one larger (the last axis of a 2-D or 3-D.. argument: one smaller -- "one more
  frame, one more row, one fewer column"): ValueError
- ``strided`` (in/out arguments only): the same shape as a non-contiguous view: ValueError -- never copied, never written
  through as if dense."""
import collections
import inspect

import numpy as np
import torch

DIMS = dict(B=2, H=9, W=12, C=3, cap=5, cap1=6, capa=6, n=7, m=4, M=2, S=3, L=4, H32=1, W32=1, B1=3)

Arg = collections.namedtuple("Arg", "dtype shape rank")


def T(dtype, *shape, rank=ValueError):
    return Arg(dtype, shape, rank)


def u8(*shape):
    return T(torch.uint8, *shape)


def i32(*shape):
    return T(torch.int32, *shape)


def i64(*shape):
    return T(torch.int64, *shape)


def f32(*shape):
    return T(torch.float32, *shape)


def f64(*shape):
    return T(torch.float64, *shape)


def labels3(dtype=torch.int32):
    """a (B, H, W) argument of a check that answers a wrong rank with TypeError"""
    return T(dtype, "B", "H", "W", rank=TypeError)


IMG = ("B", "H", "W")
STATS = ("B", "cap", 8)

Entry = collections.namedtuple("Entry", "name fn args extra bound inout accepts accepts_rank call")


def entry(fn, args, extra=None, bound=(), inout=(), accepts=None, accepts_rank=None, variant="", call=None):
    """``fn``: the function's name; ``args``: tensor arguments by keyword; ``extra(d, be)`` -> the other keywords (``d``: the
    sizes, ``be``: the backend that makes tensors); ``bound``: symbols tied to something that is no second tensor;
    ``inout``: the arguments written in place; ``accepts``: argument -> further dtypes documented as accepted for it alone;
    ``accepts_rank``: argument -> further ranks accepted; ``call(ops, kw)``: how the call is made (default: by keyword)."""
    return Entry(fn + ("-" + variant if variant else ""), fn, dict(args), extra or (lambda d, be: {}), frozenset(bound), tuple(inout),
                 dict(accepts or {}), dict(accepts_rank or {}), call)


def _class_tables(ops):
    return ops.ClassTables({1: "A", 2: "B", 3: "Particle", 5: "Background"}, ["A", "B"], {"A": 1, "B": 1}, {"A": 2, "B": 2})


def _surface(d, be):
    return {"bits": be.tensor(torch.int32, (d["B"], d["H"], d["W32"])), "counts": be.tensor(torch.int64, (d["B"],)),
            "shape": (d["B"], d["H"], d["W"])}


EDGES = (0.0, 1.0, 2.0)
_POINTS = dict(xy=f64("n", 2), slot=i32("n"), frame_offsets=i64("B1"))
_RUNS = dict(bits=i32("B", "H32", "W"), run_parent=i32(*IMG), stats=i64(*STATS))
_NEAR = dict(near=labels3(), d2=labels3())


def _mixing_by_points(ops, kw):
    kw = dict(kw)
    pts = ops.Points(kw.pop("xy"), kw.pop("slot"), None, kw.pop("frame_offsets"))
    return ops.pair_label_mixing(pts, None, None, **kw)


ENTRIES = (
    entry("argmax_planes", dict(stack=f32("B", "C", "H", "W"))),
    entry("median5", dict(x=u8(*IMG))),
    entry("classmap_label", dict(stack=f32("B", "C", "H", "W"))),
    entry("label_equal8", dict(x=u8(*IMG))),
    entry("label_bool8", dict(x=u8(*IMG))),
    entry("label_bool4", dict(x=u8(*IMG))),
    entry("compact_labels", dict(roots=i32(*IMG))),
    entry("region_init", dict(counts=i32("B")), lambda d, be: dict(cap=d["cap"], C=d["C"], shape=(d["B"], d["H"], d["W"]), device=be.device),
          bound=("B",)),
    entry("region_sums2", dict(labels_a=i32(*IMG), cls=u8(*IMG), sums_a=f64("B", "capa", "C"), labels_b=i32(*IMG), sums_b=f64("B", "cap", "C"),
                               planes=f32("B", "C", "H", "W"), stats_b=i64(*STATS), overflow_b=i32("B")),
          lambda d, be: dict(sum_classes=6), inout=("sums_a", "sums_b", "stats_b", "overflow_b")),
    entry("region_reduce", dict(labels=i32(*IMG), counts=i32("B"), cls=u8(*IMG), planes=f32("B", "C", "H", "W")),
          lambda d, be: dict(cap=d["cap"])),
    entry("region_shape", dict(labels=labels3(), counts=i32("B")), lambda d, be: dict(cap=d["cap"])),
    entry("shape_properties", dict(stats=i64(*STATS), shape=i64("B", "cap", 8), counts=i32("B"))),
    entry("region_hull", dict(labels=labels3(), counts=i32("B"), stats=i64(*STATS)), lambda d, be: dict(cap=d["cap"]), bound=("cap",)),
    entry("hull_properties", dict(stats=i64(*STATS), hull=i64("B", "cap", 4), counts=i32("B"))),
    entry("thin_labels", dict(labels=labels3())),
    entry("thin", dict(image=labels3(torch.uint8)), accepts=dict(image=(torch.bool, torch.int32))),
    entry("region_skeleton", dict(labels=labels3(), peel=labels3(torch.uint16), counts=i32("B")), lambda d, be: dict(cap=d["cap"])),
    entry("skeleton_properties", dict(stats=i64(*STATS), table=i64("B", "cap", 6), counts=i32("B"))),
    entry("threshold_lt", dict(img=f32(*IMG)), lambda d, be: dict(threshold=0.5)),
    entry("edt_sq", dict(mask=u8(*IMG))),
    entry("edt_sq_lt", dict(img=labels3(torch.float32)), lambda d, be: dict(threshold=0.5)),
    entry("dilate_disk", dict(x=u8(*IMG)), lambda d, be: dict(value_bits=2, radius=2)),
    entry("fill_particle", dict(ds=u8(*IMG), overlap_area=i64("B")),
          lambda d, be: dict(particle_label=3, cell_label=1, overlap_label=3, dilation_radius=2, dist_threshold=2), inout=("overlap_area",)),
    entry("fill_holes", dict(mask=u8(*IMG))),
    entry("local_maxima", dict(img=i32(*IMG))),
    entry("reconstruct", dict(seed=i32(*IMG), mask=i32(*IMG)), variant="i32"),
    entry("reconstruct", dict(seed=f64(*IMG), mask=f64(*IMG)), variant="f64", accepts=dict(seed=(torch.float32,), mask=(torch.float32,))),
    entry("h_maxima", dict(image=labels3()), lambda d, be: dict(h=1)),
    entry("h_minima", dict(image=labels3(torch.float64)), lambda d, be: dict(h=0.5)),
    entry("edt_maxima", dict(d2=i32(*IMG)), lambda d, be: dict(h=1.0)),
    entry("watershed", dict(img=labels3(torch.float32), markers=i32(*IMG), mask=u8(*IMG))),
    entry("dilated_roots", dict(x=u8(*IMG)), lambda d, be: dict(value_bits=2, radius=2)),
    entry("dilated_runs", dict(x=u8(*IMG), run_parent=i32(*IMG)), lambda d, be: dict(value_bits=2, radius=2), inout=("run_parent",)),
    entry("merge_groups_runs", dict(_RUNS, region_list=i32("B", "L"), n_list=i32("B")), bound=("H32",)),
    entry("dilated_runs_multi", dict(x=u8(*IMG)), lambda d, be: dict(value_bits_list=(2, 4), radius=2)),
    entry("merge_groups_fused_multi", dict(bits=i32("M", "B", "H32", "W"), run_parent=i32("M", "B", "H", "W"), stats=i64(*STATS),
                                           region_lists=i32("B", "S", "cap"), n_lists=i32("B", "S")),
          lambda d, be: dict(slots=(0, 1)), bound=("H32", "M")),
    entry("merge_groups_fused", dict(_RUNS, region_lists=i32("B", "S", "cap"), n_lists=i32("B", "S")), lambda d, be: dict(slot=1),
          bound=("H32",)),
    entry("merge_groups", dict(dilated_labels=i32(*IMG), stats=i64(*STATS), region_list=i32("B", "L"), n_list=i32("B"))),
    entry("group_reduce", dict(stats=i64(*STATS), region_list=i32("B", "L"), n_list=i32("B"), group_of=i32("B", "L"), n_groups=i32("B")),
          lambda d, be: dict(H=d["H"], W=d["W"])),
    entry("classify_regions", dict(stats=i64(*STATS), cls_out=u8("B", "cap"), counts=i32("B")),
          lambda d, be: dict(tables=_class_tables(be.ops))),
    entry("label_parent", dict(labels_a=i32(*IMG), labels_r=i32(*IMG), counts_r=i32("B"), cls_a=u8("B", "cap"), stats_r=i64(*STATS)),
          lambda d, be: dict(cap=d["cap"])),
    entry("label_contingency", dict(labels_t=labels3(), labels_s=labels3()), lambda d, be: dict(cap_t=d["cap"], cap_s=d["cap"])),
    entry("label_agreement", dict(labels_t=labels3(), labels_s=labels3()), lambda d, be: dict(cap_t=d["cap"], cap_s=d["cap"])),
    entry("label_borders", dict(labels=labels3(), strength=labels3(torch.float32)), lambda d, be: dict(cap=d["cap"])),
    entry("relabel_map", dict(labels=labels3(), label_map=i32("B", "cap1"))),
    entry("merge_by_border", dict(labels=labels3(), strength=labels3(torch.float32), counts=i32("B")),
          lambda d, be: dict(below=0.5, cap=d["cap"])),
    entry("point_neighbours", dict(_POINTS, ids=i32("n")), lambda d, be: dict(K=2, scale=1.0, edges=EDGES)),
    entry("pair_label_mixing", dict(_POINTS, frame_keys=i64("B")), lambda d, be: dict(K=2, scale=1.0, edges=EDGES, permutations=3),
          bound=("B", "B1")),
    entry("pair_label_mixing", dict(_POINTS, frame_keys=i64("B")), lambda d, be: dict(K=2, scale=1.0, edges=EDGES, permutations=3),
          bound=("B", "B1"), variant="points", call=_mixing_by_points),
    entry("surface_points", dict(x=u8(*IMG)), lambda d, be: dict(value_bits=2)),
    entry("surface_distances", dict(points_rc=f64("n", 2), frame_offsets=i64("B1"), mask=u8(*IMG), slot=i32("n")),
          lambda d, be: dict(surface=_surface(d, be), scale=1.0, n_types=2, edges=EDGES), bound=("B", "H", "W", "B1")),
    entry("surface_shells", dict(mask=u8(*IMG)), lambda d, be: dict(surface=_surface(d, be), edges=EDGES, scale=1.0),
          bound=("B", "H", "W")),
    entry("particle_mask", dict(recreated=u8(*IMG)), lambda d, be: dict(particle_value=3)),
    entry("particle_surface", dict(recreated=u8(*IMG)), lambda d, be: dict(particle_value=3)),
    entry("particle_surface", dict(mask=u8(*IMG)), lambda d, be: dict(recreated=None, particle_value=3), variant="mask"),
    entry("nearest_label", dict(labels=labels3(), sel=u8("B", "cap")), lambda d, be: dict(cap=d["cap"], want_site=True), bound=("cap",)),
    entry("territory_labels", _NEAR, lambda d, be: dict(r2=4)),
    entry("expand_labels", dict(labels=labels3()), lambda d, be: dict(distance=1), accepts_rank=dict(labels=(2,))),
    entry("territory_reduce", dict(_NEAR, mask=u8(*IMG)), lambda d, be: dict(r2=4, cap=d["cap"])),
    entry("territory_pairs", dict(_NEAR, slot_of=u8("B", "cap")), lambda d, be: dict(r2=4, pair_cap=16, n_types=2)),
    entry("remove_overlapping", dict(dapi=u8(*IMG), other=u8(*IMG)), lambda d, be: dict(threshold=0.1)),
    entry("otsu_hist", dict(img=f32(*IMG))),
    entry("morph3x3", dict(mask=u8(*IMG)), lambda d, be: dict(erode=True)),
    entry("nearest_dist", dict(a=f64("n", 2), b=f64("m", 2))),
    entry("threshold_otsu", dict(img=f32(*IMG))),
)

# the public functions of ops that take no device tensor, and why
HOST_ONLY = {
    "agreement_scores": "numpy arrays in, numpy arrays out: the per-frame scores from the integers of the match step",
    "agreement_columns": "column names",
    "agreement_tables": "reads label_agreement's result dict back and assembles numpy tables: no library call",
    "check_agreement_overflow": "reads the flags of label_agreement's result",
    "check_border_flags": "reads the flags merge_by_border returned",
    "border_block": "three constants of the library",
    "mixing_tile": "one constant of the library",
    "surface_thresholds": "numpy in, numpy out (the entry takes no stream)",
    "reach_r2": "a bisection on the host",
    "reach_um_r2": "surface_thresholds and arithmetic",
}
# ... and those that take the pipeline's own result, not a caller's tensors: what they hand to the library goes through the
# wrappers of the table or through ops._addr (``_req`` and an exact shape for every field)
COMPOSED = {
    "class_rows": "indexing of a result dict with torch: no library call",
    "refined_rows": "indexing of a result dict with torch: no library call",
    "build_tables": "the pipeline's result dict: every field through ops._addr, every stage through a wrapper of the table",
    "refined_inputs": "the pipeline's result dict: every field through ops._addr",
    "refined_tables": "label_parent and classify_regions (in the table), then refined_inputs",
    "territory_rows": "nearest_label, territory_reduce and territory_pairs (in the table) and torch indexing",
}


def public_functions(ops):
    """the names of the functions ``ops`` defines for its callers (classes and named tuples apart)"""
    return sorted(name for name, obj in vars(ops).items()
                  if not name.startswith("_") and callable(obj) and not inspect.isclass(obj) and getattr(obj, "__module__", None) == ops.__name__)


# ------------------------------------------------------------------ the hook
class Reached(Exception):
    """raised in the place of a library call: the arguments passed every check in front of it"""

    def __init__(self, entry):
        super().__init__(entry)
        self.entry = entry


def install(ops, monkeypatch):
    """``ops._call`` and ``ops._workspace`` raise :class:`Reached`: from here on no wrapper enters the library"""
    def hook(entry, *args, **kwargs):
        raise Reached(entry)
    monkeypatch.setattr(ops, "_call", hook)
    monkeypatch.setattr(ops, "_workspace", hook)


# ------------------------------------------------------------------ tensors
NUMPY = {torch.uint8: np.uint8, torch.uint16: np.uint16, torch.int32: np.int32, torch.int64: np.int64, torch.float32: np.float32,
         torch.float64: np.float64}
NEIGHBOURS = {torch.int32: (torch.int64, torch.uint8), torch.int64: (torch.int32,), torch.uint8: (torch.int32,),
              torch.float32: (torch.float64,), torch.float64: (torch.float32,), torch.uint16: (torch.int32,)}
_FURTHER = (torch.int32, torch.int64, torch.int16)  # where every neighbour is accepted: the first of these that is not


class Backend:
    """Where the valid tensors live (``home``) and where a foreign one does."""

    def __init__(self, ops, home, foreign):
        self.ops, self.device, self.foreign_device = ops, home, foreign

    def tensor(self, dtype, shape):
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def foreign(self, dtype, shape):
        return torch.zeros(shape, dtype=dtype, device=self.foreign_device)

    def strided(self, dtype, shape):
        """``shape`` as a view of every second element of the last dimension: same sizes, not contiguous"""
        big = torch.zeros(tuple(shape[:-1]) + (2 * shape[-1],), dtype=dtype, device=self.device)
        t = big[..., ::2]
        assert tuple(t.shape) == tuple(shape) and not t.is_contiguous()
        return t


def sizes(shape, dims=DIMS):
    return tuple(dims[s] if isinstance(s, str) else s for s in shape)


# ------------------------------------------------------------------ mutations
Mutation = collections.namedtuple("Mutation", "arg kind raises detail")


def _bound_symbols(e):
    seen = collections.Counter(s for a in e.args.values() for s in set(a.shape) if isinstance(s, str))
    return {s for s, k in seen.items() if k >= 2} | set(e.bound)


def wrong_dtypes(e, name):
    arg = e.args[name]
    ok = (arg.dtype,) + tuple(e.accepts.get(name, ()))
    out = [d for d in NEIGHBOURS[arg.dtype] if d not in ok]
    return out or [d for d in _FURTHER if d not in ok][:1]


def mutations(e):
    """every refused call of entry ``e``"""
    out = []
    bound = _bound_symbols(e)
    for name, arg in e.args.items():
        out.append(Mutation(name, "foreign", TypeError, None))
        out.append(Mutation(name, "numpy", TypeError, None))
        out += [Mutation(name, "dtype:%s" % str(d)[6:], TypeError, d) for d in wrong_dtypes(e, name)]
        ok_ranks = e.accepts_rank.get(name, ())
        rank_error = ValueError if name in e.inout else arg.rank
        for kind, delta in (("rank+", 1), ("rank-", -1)):
            if len(arg.shape) + delta not in ok_ranks:
                out.append(Mutation(name, kind, rank_error, delta))
        nd = len(arg.shape)
        for i, s in enumerate(arg.shape):
            if not isinstance(s, str) or s in bound:
                out.append(Mutation(name, "axis%d" % i, ValueError, (i, -1 if (i == nd - 1 and nd >= 2) else 1)))
        if name in e.inout:
            out.append(Mutation(name, "strided", ValueError, None))
    return out


def arguments(e, be, mutation=None):
    """the keywords of entry ``e``'s call, valid or with one argument mutated"""
    kw = {name: be.tensor(a.dtype, sizes(a.shape)) for name, a in e.args.items()}
    kw.update(e.extra(DIMS, be))
    if mutation is not None:
        a = e.args[mutation.arg]
        shape, kind = sizes(a.shape), mutation.kind
        if kind == "foreign":
            t = be.foreign(a.dtype, shape)
        elif kind == "numpy":
            t = np.zeros(shape, NUMPY[a.dtype])
        elif kind.startswith("dtype:"):
            t = be.tensor(mutation.detail, shape)
        elif kind == "rank+":
            t = be.tensor(a.dtype, (1,) + shape)
        elif kind == "rank-":
            t = be.tensor(a.dtype, shape[1:])
        elif kind.startswith("axis"):
            i, delta = mutation.detail
            t = be.tensor(a.dtype, shape[:i] + (shape[i] + delta,) + shape[i + 1:])
        elif kind == "strided":
            t = be.strided(a.dtype, shape)
        else:
            raise ValueError(kind)
        kw[mutation.arg] = t
    return kw


def invoke(e, ops, kw):
    if e.call is not None:
        return e.call(ops, kw)
    return getattr(ops, e.fn)(**kw)


def valid_params():
    return [(e.name, e) for e in ENTRIES]


def mutation_params():
    return [("%s-%s-%s" % (e.name, m.arg, m.kind), e, m) for e in ENTRIES for m in mutations(e)]
