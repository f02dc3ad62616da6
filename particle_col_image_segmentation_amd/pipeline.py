"""Batched per-frame hot path on one GPU: frames (B,5,H,W) -> label masks + ROI tables.

One ``FramePipeline.run`` is the full chain of SURVEY.md section 8a for a batch
that is already resident in HBM:

    class map (argmax+1) -> median5 (A1) -> label (A2) -> region table + isotope sums (A3, M1)
    -> classification / cluster cell counts (A3 tail, A4) -> proximity merge per type + combined (A5, A6)
    -> particle-area reconstruction per cell class (A8) -> [counts / densities: host epilogue (A9)]
    -> boundary refinement: threshold + EDT + local maxima + markers + watershed (R1-R4, W1)
    -> per-ROI isotope sums of the refined ROIs (M1)

Everything stays on the device and no kernel chain waits for the host (the watershed's fixed points finish in
device-side tail kernels), so the whole chain of a batch can be captured once as a hipGraph and replayed
(``FramePipeline(graph=True)``).  ``tables()`` downloads the result as plain numpy tables (the per-ROI table format of
this build; the reference's CSV writers take the per-frame drop-in objects instead, see ``tiff_analysis``).
"""
import collections

import numpy as np
import torch

from . import gaps, local, ops, spatial
from . import tiff_analysis as ta
from .synth import BOUNDARY_PLANE, CELL_TYPES_5

# ratio presets for the isotope planes: (name, numerator plane, denominator planes) -- .m:136-139
RATIOS_7 = (("C13act", 1, (1, 0)), ("N15act", 3, (2, 3)), ("O17act", 5, (6, 5, 4)), ("O18act", 6, (6, 5, 4)))
RATIOS_5 = (("C13act", 1, (1, 0)), ("N15act", 3, (2, 3)))


class BatchResult(dict):
    """Device tensors of one batch (see FramePipeline.run for the keys).

    ``FramePipeline.run`` returns as soon as both kernel chains are enqueued; reading any entry waits (once) for the two
    events that close them, so callers never see unfinished tensors, while a loop that only calls ``run`` keeps the
    next batch's class-map chain running under this batch's watershed tail."""

    _pending = None
    _slot = None   # graph mode: the capture slot whose static tensors this result aliases ...
    _gen = 0       # ... and the slot's replay count when this result was handed out
    _stack = None  # the input of the run (FramePipeline.borders reads its boundary plane); not an entry: run()'s keys stay

    def _check_alive(self):
        if self._slot is not None and self._slot.gen != self._gen:
            raise RuntimeError("this graph-mode result has been overwritten: its lane has replayed a later batch "
                               "(results stay valid until `lanes` further batches have been handed to run())")

    def done_events(self):
        """The events that close this batch's kernel chains (waits for the lane thread to have enqueued them)."""
        pending = self._pending
        if pending is None:
            return []
        if hasattr(pending, "result"):
            return list(pending.result()[1])
        return list(pending)

    def ready(self):
        """True once the batch's kernel chains have finished (never blocks: a batch whose lane has not even enqueued it
        yet is not ready)."""
        pending = self._pending
        if pending is None:
            return True
        if hasattr(pending, "result"):
            if not pending.done():
                return False
            events = pending.result()[1]
        else:
            events = pending
        return all(ev.query() for ev in events)

    def synchronize(self):
        self._check_alive()
        pending = self._pending
        if pending is None:
            return self
        events = pending
        if hasattr(pending, "result"):  # a lane's future: (entries, closing events)
            # a lane that raised keeps raising here on every read: _pending is only cleared after a clean hand-over
            entries, events = pending.result()
            dict.update(self, entries)
        for ev in events:
            ev.synchronize()
        # the tensors were allocated on the lane's streams: tell the caching allocator that the caller's stream uses
        # them too, so that dropping this result cannot hand their blocks to the lane's next batch while a kernel the
        # caller enqueued is still reading them
        if self._slot is None:  # (a graph slot's tensors live in the graph's private pool: nothing to announce)
            cur = torch.cuda.current_stream()
            for t in _tensors(dict.values(self)):
                if t.is_cuda:
                    t.record_stream(cur)
        self._pending = None
        return self

    def __getitem__(self, key):
        self._settle()
        return dict.__getitem__(self, key)

    def _settle(self):
        """every accessor: wait for the batch once, and refuse a graph-mode result whose lane has replayed since"""
        if self._pending:
            self.synchronize()
        elif self._slot is not None:
            self._check_alive()

    def get(self, key, default=None):
        self._settle()
        return dict.get(self, key, default)

    def items(self):
        self._settle()
        return dict.items(self)

    def values(self):
        self._settle()
        return dict.values(self)

    def keys(self):
        self._settle()
        return dict.keys(self)

    def __iter__(self):
        self._settle()
        return dict.__iter__(self)

    def __contains__(self, key):
        self._settle()
        return dict.__contains__(self, key)

    def __len__(self):
        self._settle()
        return dict.__len__(self)

    def check(self):
        """Raise for the conditions the reference raises for / the tables cannot hold."""
        if int(self["overflow"].sum().item()) or int(self["ws_overflow"].sum().item()):
            raise RuntimeError("region table capacity exceeded: raise FramePipeline(cap=...)")
        if int((self["counts"] < 0).sum().item()):
            # a label pass found a union-find entry outside its fence (csrc/union_find.h, walk_ok) and reported -1 components:
            # the workspace was overwritten while the chain ran (e.g. one captured graph replayed on two streams at once)
            raise RuntimeError("corrupt union-find image in the class-map labelling (counts < 0)")
        if int(self["nan_flag"].sum().item()):
            # tiff_analysis.py:776-781: clusters of a type without any single cell -> int(NaN)
            raise ValueError("cannot convert float NaN to integer")
        if dict.__contains__(self, "border_flags"):
            ops.check_border_flags(self["border_flags"])
        return self


def _tensors(values):
    for v in values:
        if isinstance(v, torch.Tensor):
            yield v
        elif isinstance(v, dict):
            yield from _tensors(v.values())


_LANES = {}  # (device index, lanes) -> (executors, stream sets): shared by every pipeline of the process
N_STREAMS = 5  # per lane: class chain, refinement chain (high priority), particle fill, two more merge slots


def _lanes_for(device, lanes):
    key = (device.index, lanes)
    if key not in _LANES:
        from concurrent.futures import ThreadPoolExecutor
        pools = [ThreadPoolExecutor(max_workers=1, thread_name_prefix="pcseg-lane%d" % i) for i in range(lanes)]
        streams = [tuple(torch.cuda.Stream(device=device, priority=-1 if k == 1 else 0) for k in range(N_STREAMS))
                   for _ in range(lanes)]
        _LANES[key] = (pools, streams)
    return _LANES[key]


TableSwitches = ops.TableSwitches  # the switches of the optional tables and their defaults, described in tables_device

# THE schema of the optional tables, in the order table_columns names them: name, on(switches), columns(type names,
# switches), key columns of the gather's sort (distributed._SORT_COLS) and rows(pipeline, frame ids, ops.build_tables
# result) -> the device table.  The refined_* tables are their namesakes over the refined rows of kind >= 1.
_Table = collections.namedtuple("_Table", "name on columns key rows")
_bins = lambda edges: ["bin_%d" % k for k in range(len(edges) - 1)] + ["over"]
_per_type = lambda names, *fmts: [f % n for n in names for f in fmts]
_nn_cols = lambda names, o: ["frame", "label", "slot"] + _per_type(names, "nn_um_%s") + _per_type(names, "nn_label_%s")
_pair_cols = lambda names, o: ["frame", "slot_a", "slot_b", "n_pairs"] + _bins(o.pair_edges)
_sf_cols = lambda names, o: ["frame", "label", "slot", "inside", "surface_um", "nearest_row", "nearest_col"]
_sf_hist_cols = lambda names, o: ["frame", "side", "slot", "n"] + _bins(o.surface_edges)
_sf_rows = lambda p, fid, sf: p._point_rows(fid, sf["points"], sf["inside"], sf["dist"], sf["nearest"])
_shape_cols = lambda names, o: ["frame", "label", "slot", "n_border", "n_1", "n_sqrt2", "n_mid", "mu_rr", "mu_rc", "mu_cc", "major_um",
                               "minor_um", "eccentricity", "orientation", "equivalent_diameter_um", "extent", "perimeter_um"]
_hull_cols = lambda names, o: ["frame", "label", "slot", "convex_area", "solidity", "feret_um", "euler_number", "convex_area_um2"]
_skel_cols = lambda names, o: ["frame", "label", "slot", "skel_px", "n_orth", "n_diag", "n_end", "n_junction", "passes", "length_um",
                              "width_um"]
_terr_cols = lambda names, o: (["frame", "label", "slot", "territory_px", "territory_on_px", "reach2_max", "clipped"]
                               + _per_type(names, "n_adj_%s") + _per_type(names, "n_contact_%s") + ["territory_um2", "territory_on_um2"])
_adj_cols = lambda names, o: ["frame", "label_a", "label_b", "slot_a", "slot_b", "border_px", "contact_px"]
_mix_cols = lambda names, o: list(ta.MIXING_COLUMNS)
_pairs, _shells = (lambda o: o.pair_edges is not None), (lambda o: o.surface_edges is not None)
_mixes = lambda o: bool(o.mixing) and _pairs(o)
OPTIONAL_TABLES = (
    _Table("neighbours", lambda o: o.neighbours, _nn_cols, (0, 1),
           lambda p, fid, raw: p._neighbour_rows(raw["cells"], raw["cell_nn"]["dist"], raw["cell_nn"]["nn_id"])),
    _Table("pair_hist", _pairs, _pair_cols, (0, 1, 2), lambda p, fid, raw: p._pair_rows(fid, raw["cell_nn"]["hist"])),
    _Table("mixing", _mixes, _mix_cols, (0, 1, 2, 3), lambda p, fid, raw: p._mixing_rows(fid, raw["cell_mix"], raw["mixing_args"])),
    _Table("refined", lambda o: o.refined, lambda names, o: ["frame", "label", "parent", "parent_px", "n_overlap", "class", "kind",
                                                             "cells", "area", "centroid_row", "centroid_col"], (0, 1),
           lambda p, fid, raw: raw["refined"]),
    _Table("cell_resolution", lambda o: o.refined, lambda names, o: ["frame", "label", "children", "resolved", "cells_integrated"],
           (0, 1), lambda p, fid, raw: raw["cell_resolution"]),
    _Table("frames_refined", lambda o: o.refined,
           lambda names, o: ["frame", "refined_nan_flag"] + _per_type(names, "%s_refined_cells", "%s_refined_clusters", "%s_resolved",
                                                                      "%s_residual", "%s_count_integrated"),
           (0, 1), lambda p, fid, raw: raw["frames_refined"]),
    _Table("refined_neighbours", lambda o: o.refined and o.neighbours, _nn_cols, (0, 1),
           lambda p, fid, raw: p._point_rows(fid, raw["refined_nn"]["points"], raw["refined_nn"]["dist"], raw["refined_nn"]["nn_id"])),
    _Table("refined_pair_hist", lambda o: o.refined and _pairs(o), _pair_cols, (0, 1, 2),
           lambda p, fid, raw: p._pair_rows(fid, raw["refined_nn"]["hist"])),
    _Table("refined_mixing", lambda o: o.refined and _mixes(o), _mix_cols, (0, 1, 2, 3),
           lambda p, fid, raw: p._mixing_rows(fid, raw["refined_mix"], raw["mixing_args"])),
    _Table("surface", lambda o: o.surface, _sf_cols, (0, 1), lambda p, fid, raw: _sf_rows(p, fid, raw["cell_sf"])),
    _Table("frames_surface", lambda o: o.surface, lambda names, o: ["frame", "surface_px", "filled_area"], (0,),
           lambda p, fid, raw: torch.stack([fid, raw["cell_sf"]["surface_px"], raw["cell_sf"]["filled_area"]], dim=1).to(torch.float64)),
    _Table("surface_hist", _shells, _sf_hist_cols, (0, 1, 2), lambda p, fid, raw: p._side_rows(fid, raw["cell_sf"]["hist"])),
    _Table("surface_shells", _shells, lambda names, o: ["frame", "side", "n_px"] + _bins(o.surface_edges), (0, 1),
           lambda p, fid, raw: p._side_rows(fid, raw["cell_sf"]["shells"])),
    _Table("refined_surface", lambda o: o.refined and o.surface, _sf_cols, (0, 1),
           lambda p, fid, raw: _sf_rows(p, fid, raw["refined_sf"])),
    _Table("refined_surface_hist", lambda o: o.refined and _shells(o), _sf_hist_cols, (0, 1, 2),
           lambda p, fid, raw: p._side_rows(fid, raw["refined_sf"]["hist"])),
    _Table("territories", lambda o: o.territory, _terr_cols, (0, 1), lambda p, fid, raw: raw["territories"]),
    _Table("adjacency", lambda o: o.territory, _adj_cols, (0, 1, 2), lambda p, fid, raw: raw["adjacency"]),
    _Table("refined_territories", lambda o: o.refined and o.territory, _terr_cols, (0, 1), lambda p, fid, raw: raw["refined_territories"]),
    _Table("refined_adjacency", lambda o: o.refined and o.territory, _adj_cols, (0, 1, 2), lambda p, fid, raw: raw["refined_adjacency"]),
    _Table("skeletons", lambda o: o.skeleton, _skel_cols, (0, 1), lambda p, fid, raw: raw["skeletons"]),
    _Table("refined_skeletons", lambda o: o.refined and o.skeleton, _skel_cols, (0, 1), lambda p, fid, raw: raw["refined_skeletons"]),
    _Table("convexity", lambda o: o.convex, _hull_cols, (0, 1), lambda p, fid, raw: raw["convexity"]),
    _Table("refined_convexity", lambda o: o.refined and o.convex, _hull_cols, (0, 1), lambda p, fid, raw: raw["refined_convexity"]),
    _Table("shapes", lambda o: o.shape, _shape_cols, (0, 1), lambda p, fid, raw: raw["shapes"]),
    _Table("refined_shapes", lambda o: o.refined and o.shape, _shape_cols, (0, 1), lambda p, fid, raw: raw["refined_shapes"]),
)
_EXTRA_TABLES = tuple(t.name for t in OPTIONAL_TABLES)


def _download(tables):
    """device tensors -> numpy through PINNED staging buffers (torch caches them): all copies are enqueued, then one
    wait.  A pageable ``.cpu()`` of the ~100 MB ROI table of a dataset costs more than the kernels of a batch."""
    out, staged = {}, []
    for k, v in tables.items():
        if isinstance(v, torch.Tensor) and v.is_cuda:
            buf = torch.empty(tuple(v.shape), dtype=v.dtype, pin_memory=True)
            buf.copy_(v, non_blocking=True)
            staged.append((k, buf))
        elif isinstance(v, torch.Tensor):
            out[k] = v.numpy()
        else:
            out[k] = np.asarray(v)
    if staged:
        torch.cuda.current_stream().synchronize()
        for k, buf in staged:
            out[k] = buf.numpy()
    return out


def _on(stream, *tensors):
    """Tensors made on another stream are about to be read by kernels on ``stream``: tell the caching allocator, so
    that freeing them cannot hand their memory to new work of the producing stream while ``stream`` still reads."""
    for t in tensors:
        if t is not None:
            t.record_stream(stream)


class _GraphSlot:
    """One captured chain: the hipGraph of a lane for one input buffer, the static result tensors it writes (they live in
    the graph's private memory pool) and the stream it is replayed on."""
    __slots__ = ("graph", "entries", "stream", "release", "gen", "stack")

    def __init__(self, stream):
        self.graph, self.entries, self.stream, self.release, self.gen, self.stack = None, None, stream, None, 0, None


class FramePipeline:
    def __init__(self, cell_types=None, threshold=0.5, boundary_plane=BOUNDARY_PLANE, cap=None, merged=True,
                 watershed_mode=0, overlap=True, lanes=None, multi_stream=True, graph=False, max_graphs=None, marker_h=None,
                 merge_below=None, merge_by="mean"):
        """``graph=True``: the chain of a batch (about a hundred launches on five streams) is captured ONCE per input
        buffer as a hipGraph and replayed for every later batch in that buffer -- one host call per batch instead of a
        hundred, no host thread per lane.  Inputs must then live in a small set of reused device buffers (the graph is
        keyed on the buffer's address and shape; ``max_graphs`` bounds the cache), and a result's tensors are the
        graph's static outputs: they stay valid until ``lanes`` further batches have been handed to :meth:`run`.
        ``lanes``: batches in flight (default 8 host threads in eager mode, 2 replay streams in graph mode).
        ``marker_h`` (pixels of the distance map; None: every local maximum): the watershed's markers are the h-maxima of the
        distance map (``ops.edt_maxima``) and the result gains ``marker_flags``.
        ``merge_below`` (a boundary probability in [0, 1]; None: no merge, nothing more is launched) / ``merge_by`` ("mean" or
        "saddle"): after the flood, touching refined ROIs whose border in the boundary plane is weaker than ``merge_below``
        are joined (``ops.merge_by_border``, 8-neighbour links; eagerly and in the captured graph alike, nothing is read
        back).  ``ws_labels`` and ``n_markers`` of the result are then the MERGED image and its counts, so the sums stage,
        the refined tables, the shapes and :meth:`agreement` see the merged ROIs; the result gains ``ws_labels_unmerged``,
        ``n_unmerged``, ``merge_map`` and ``border_flags``.  ``markers`` stays the flood's marker image, numbered as
        ``ws_labels_unmerged``."""
        if lanes is None:
            lanes = 2 if graph else 8
        self.cell_types = dict(cell_types or CELL_TYPES_5)
        self.tables_ = ops.ClassTables(self.cell_types, ta.CELL_TYPES, ta.MIN_CELL_AREA, ta.MIN_CLUSTER_AREA)
        self.threshold = float(threshold)
        self.boundary_plane = int(boundary_plane)
        self.cap = cap
        self.merged = merged
        self.watershed_mode = watershed_mode
        self.marker_h = None if marker_h is None else float(marker_h)
        self.merge_below = None if merge_below is None else float(merge_below)
        if merge_by not in ("mean", "saddle") or (self.merge_below is not None and not 0.0 <= self.merge_below <= 1.0):
            raise ValueError('merge_by must be "mean" or "saddle" and merge_below a probability in [0, 1]')
        self.merge_by = merge_by
        self.overlap = overlap
        self.lanes = max(1, int(lanes))
        self.multi_stream = bool(multi_stream)  # False: the class-map chain (incl. merges and fill) on ONE stream
        self.graph = bool(graph)
        self.max_graphs = int(max_graphs or 4 * self.lanes)
        self._graphs = {}  # (lane, input address, shape) -> _GraphSlot, in insertion order (oldest first)
        self._table_stream = None
        self._lane_pool = None  # one single-thread executor + stream set per lane, made on first use
        self._lane_streams = None
        self._step = 0

    def run(self, stack):
        """Enqueue the full chain for one batch and return at once; reading any entry of the result waits for it.
        ``stack`` must not be modified (or refilled in place) before the result has been read or
        ``result.synchronize()`` has returned: the kernels read it asynchronously."""
        if stack.dim() != 4 or stack.dtype != torch.float32 or not stack.is_cuda:
            raise TypeError("stack must be a (B, C, H, W) float32 CUDA tensor")
        if self.graph:
            return self._run_graph(stack)
        stack = stack.contiguous()
        res = BatchResult()
        res._stack = stack
        res["shape"] = tuple(stack.shape)
        if not self.overlap:
            self._class_stage(stack, res)
            self._merge_all(stack, res)
            self._fill_stage(stack, res)
            self._refine_chain(stack, res)
            self._sums_stage(stack, res)
            return res
        # The chain is a small graph, not a line: the class-map stage (front end, region table, classification), the
        # merge of each cell type and of all types together (they only need the classification), the particle fill (it
        # only needs the denoised map) and the boundary refinement (it only needs the input) run on streams of their
        # own, ordered by events.  Nothing in the chain waits for the host, so one host thread can keep them all fed;
        # consecutive batches still alternate between `lanes` host threads (a stream set each) so that the launch
        # overhead of one batch runs under the kernels of the other.  `run` returns at once; the result object waits
        # for its lane and its closing events the first time an entry is read.
        if self._lane_pool is None or self._lane_streams[0][0].device != stack.device:
            self._lane_pool, self._lane_streams = _lanes_for(stack.device, self.lanes)
        lane = self._step % self.lanes
        self._step += 1
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream())
        res._pending = self._lane_pool[lane].submit(self._run_lane, lane, stack, ready, dict(res))
        return res

    def synchronize(self):
        """Wait until every batch handed to ``run`` so far is finished (lanes drained, device idle)."""
        for pool in self._lane_pool or ():
            pool.submit(lambda: None).result()
        torch.cuda.synchronize()

    # ------------------------------------------------------------------ hipGraph capture / replay
    def _run_graph(self, stack):
        if not stack.is_contiguous():
            raise ValueError("graph mode needs a contiguous input buffer (the graph is keyed on its address)")
        dev = stack.device
        lane = self._step % self.lanes
        self._step += 1
        key = (lane, stack.data_ptr(), tuple(stack.shape))
        slot = self._graphs.get(key)
        if slot is None:
            slot = self._capture(lane, stack, key)
        cur = torch.cuda.current_stream(dev)
        slot.stream.wait_stream(cur)  # whatever the caller's stream wrote into the buffer
        if slot.release is not None:  # ... and whoever still reads the slot's previous result (tables_device)
            slot.stream.wait_event(slot.release)
            slot.release = None
        done = torch.cuda.Event()
        with torch.cuda.stream(slot.stream):
            # ONE instance of a captured chain at a time: a slot owns one workspace (union-find parents, overflow tables,
            # dirty-tile lists) and one set of static outputs, so two replays of it must never overlap.  Replaying on
            # slot.stream -- and nowhere else -- serialises them; profiles/r03/exp_graph_r3a.log is what the other way
            # round looks like (one graph replayed on 4 streams at once: a memory-access fault).
            if torch.cuda.current_stream(dev) != slot.stream:
                raise RuntimeError("a graph slot may only be replayed on its own stream")
            slot.graph.replay()
            done.record(slot.stream)
        slot.gen += 1
        res = BatchResult(slot.entries)
        res._stack = stack
        res._pending, res._slot, res._gen = [done], slot, slot.gen
        return res

    def _capture(self, lane, stack, key):
        """Capture the lane's five-stream chain for this input buffer (once).  A plain run comes first: one-time work
        inside the library (function attributes, the tile counter's allocation) must not fall into the capture."""
        dev = stack.device
        while len(self._graphs) >= self.max_graphs:
            old = self._graphs.pop(next(iter(self._graphs)))  # oldest first; its memory pool goes with it ...
            old.stream.synchronize()  # ... so no replay of it may still be running (a caller may have dropped its result unread)
            old.gen += 1              # results that still alias its static tensors refuse to be read from now on
        _, lane_streams = _lanes_for(dev, self.lanes)
        streams = lane_streams[lane]
        slot = _GraphSlot(torch.cuda.Stream(device=dev))
        entries = {"shape": tuple(stack.shape)}

        def chain(s_main):
            ready = torch.cuda.Event()
            ready.record(s_main)
            if self.overlap:
                out, done = self._run_streams(streams, stack, ready, dict(entries))
                for ev in done:
                    s_main.wait_event(ev)
                return out
            out = BatchResult(entries)
            self._class_stage(stack, out)
            self._merge_all(stack, out)
            self._fill_stage(stack, out)
            self._refine_chain(stack, out)
            self._sums_stage(stack, out)
            return dict(out)

        slot.stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(slot.stream):
            chain(slot.stream)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=slot.stream, capture_error_mode="thread_local"):
            slot.entries = chain(slot.stream)
        slot.graph, slot.stack = graph, stack  # (the buffer stays alive as long as a graph reads it)
        self._graphs[key] = slot
        return slot

    def _merge_slots(self):
        if not self.merged:
            return []
        return [s for s in range(len(self.tables_.slot_names))] + [4]

    def _run_lane(self, lane, stack, ready, entries):
        torch.cuda.set_device(stack.device)
        return self._run_streams(self._lane_streams[lane], stack, ready, entries)

    def _run_streams(self, streams, stack, ready, entries):
        out = BatchResult(entries)  # built privately: the caller's object only receives it on synchronize()
        s_class, s_refine, s_fill, s_m1, s_m2 = streams
        if not self.multi_stream:
            s_fill = s_m1 = s_m2 = s_class
        for st in streams:
            st.wait_event(ready)
            stack.record_stream(st)
        with torch.cuda.stream(s_refine):
            self._refine_chain(stack, out)
        with torch.cuda.stream(s_class):
            self._class_stage(stack, out, denoised_ready=(ev_z := torch.cuda.Event()))
            ev_c = torch.cuda.Event()
            ev_c.record(s_class)
        with torch.cuda.stream(s_refine):
            # the isotope sums of BOTH label images in one pass over the planes, once both are final
            s_refine.wait_event(ev_c)
            _on(s_refine, out["labels"], out["denoised"], out["cc_sums"])
            self._sums_stage(stack, out)
        with torch.cuda.stream(s_fill):
            if s_fill is not s_class:
                s_fill.wait_event(ev_z)
                _on(s_fill, out["denoised"])
            self._fill_stage(stack, out)
        with torch.cuda.stream(s_class):  # (the class-map stream is idle after the classification)
            self._merge_all(stack, out)
        done = []
        for st in streams:
            ev = torch.cuda.Event()
            ev.record(st)
            done.append(ev)
        return dict(out), done

    def _class_stage(self, stack, res, denoised_ready=None):
        B, C, H, W = stack.shape
        cap = self.cap or max(1024, (H * W) // 64)
        tb = self.tables_
        # ---- class map + denoise + label in one fused front end (ingest, A1, A2)
        z, labels, counts = ops.classmap_label(stack)
        res["denoised"] = z
        if denoised_ready is not None:
            denoised_ready.record(torch.cuda.current_stream())
        # ---- region table (A3): the integer columns only (4 bytes per pixel); the isotope sums of the class components
        # come from the fused plane pass at the end of the batch (_sums_stage), into the zeroed table made here
        stats, cls_out, cc_sums, overflow = ops.region_reduce(labels, counts, cls=z, cap=cap, zero_sums=C)
        res.update(labels=labels, counts=counts, stats=stats, cls_out=cls_out, cc_sums=cc_sums, overflow=overflow)
        # ---- classification, cluster cell counts, region lists (A3 tail, A4)
        res.update(ops.classify_regions(stats, cls_out, counts, tb))
        res["groups"] = {}

    def _merge_all(self, stack, res):
        """every proximity merge of the batch (one mask per cell type + the union of all types, A5 / A6) in five launches:
        the class map is read once for all masks, dilation / run components / cross-tile links / grouping each run once over
        masks x frames"""
        slots = self._merge_slots()
        if not slots:
            return
        B, C, H, W = stack.shape
        tb = self.tables_
        masks = []
        for s in slots:
            bits = 0
            for v in ([tb.slot_value[s]] if s < 4 else tb.slot_value):
                bits |= 1 << v
            masks.append(bits)
        keep = [k for k, m in enumerate(masks) if m]
        if not keep:
            return
        # the batched kernels take up to four masks a call (MaskSet / MergeSlots are four wide): a four-type table has five
        for lo in range(0, len(keep), 4):
            part = keep[lo:lo + 4]
            dbits, run_par = ops.dilated_runs_multi(res["denoised"], [masks[k] for k in part], ta.CELL_CLUSTER_DISTANCE_THRESHOLD // 2)
            gof, ng, gst = ops.merge_groups_fused_multi(dbits, run_par, res["stats"], res["region_list"], res["n_list"], [slots[k] for k in part])
            for m, k in enumerate(part):
                res["groups"][slots[k]] = {"group_of": gof[m], "n_groups": ng[m], "group_stats": gst[m]}

    def _fill_stage(self, stack, res):
        """particle-area reconstruction, one fill per cell class on the previous output (A8)"""
        B = stack.shape[0]
        tb = self.tables_
        ds = res["denoised"]
        overlap = torch.zeros((B,), dtype=torch.int64, device=stack.device)
        if tb.particle_value is not None:
            for v in tb.cell_values:
                ds, overlap = ops.fill_particle(ds, tb.particle_value, v, tb.particle_value, ta.DILATION_RADIUS,
                                                ta.DISTANCE_THRESHOLD, overlap)
        res["recreated"] = ds
        res["overlap_area"] = overlap

    def _refine_chain(self, stack, res):
        B, C, H, W = stack.shape
        cap = self.cap or max(1024, (H * W) // 64)
        # ---- boundary refinement (R1-R4, W1) on the boundary plane, read in place
        bm = stack[:, self.boundary_plane]
        d2, mask = ops.edt_sq_lt(bm, self.threshold)
        if self.marker_h is None:
            _, markers, n_markers = ops.local_maxima(d2, want_mask=False)
        else:
            _, markers, n_markers, res["marker_flags"] = ops.edt_maxima(d2, self.marker_h, want_mask=False)
        ws_labels, tie_flags = ops.watershed(bm, markers, mask, mode=self.watershed_mode)
        if self.merge_below is not None:
            # ---- over-segmentation: dissolve the borders the classifier did not see (fill -> merge -> relabel, no host read)
            res.update(ws_labels_unmerged=ws_labels, n_unmerged=n_markers)
            ws_labels, n_markers, res["merge_map"], res["border_flags"] = ops.merge_by_border(
                ws_labels, bm, self.merge_below, by=self.merge_by, counts=n_markers, cap=cap)
        res.update(mask=mask, markers=markers, n_markers=n_markers, ws_labels=ws_labels, tie_flags=tie_flags)
        # ---- area / centroid sums of the refined ROIs (plane-free pass); their isotope sums: _sums_stage.  (The sums pass
        # does not take the integer columns along: that form was built and removed -- the refined ROIs are small, every lane
        # ends a run or two per 32-row block, and eight 64-bit LDS atomics per run end cost more there (614 us against
        # 407 + 191).)
        ws_stats, _, ws_sums, ws_overflow = ops.region_reduce(ws_labels, n_markers, cap=cap, zero_sums=C)
        res.update(ws_stats=ws_stats, ws_sums=ws_sums, ws_overflow=ws_overflow)

    def _sums_stage(self, stack, res):
        """per-ROI isotope sums (M1, .m:122-135) of the class-map components AND of the refined ROIs in one pass over
        the planes.  Sums of class components are only ever reported for cell / cluster regions (tiff_analysis.py:1041-1044):
        that image is summed under the cell classes only."""
        cell_bits = 0
        for v in self.tables_.cell_values:
            cell_bits |= 1 << int(v)
        B, C, H, W = stack.shape
        # the fused pass reads labels and planes as 16-byte quads: a contiguous view at an odd storage offset (legal for run())
        # takes the per-image kernels below like a ragged width does
        aligned = all(t.data_ptr() % 16 == 0 for t in (res["labels"], res["ws_labels"], stack)) and res["denoised"].data_ptr() % 4 == 0
        if W % 4 == 0 and aligned:
            ops.region_sums2(res["labels"], res["denoised"], cell_bits, res["cc_sums"], res["ws_labels"], res["ws_sums"], stack)
            return
        # ragged widths: region_reduce per image (the row sums kernel; the integer columns it returns are those _class_stage
        # and _refine_chain already have)
        cap = res["stats"].shape[1]
        _, _, res["cc_sums"], _ = ops.region_reduce(res["labels"], res["counts"], cls=res["denoised"], planes=stack, cap=cap,
                                                    sum_classes=cell_bits)
        _, _, res["ws_sums"], _ = ops.region_reduce(res["ws_labels"], res["n_markers"], planes=stack, cap=cap)

    # ------------------------------------------------------------------ table output
    def table_columns(self, C, ratios=RATIOS_5, **switches):
        """Column names of every table of :meth:`tables` (known without any data: ranks that own no frame of a
        dataset still agree on the schema, see ``distributed.run_sharded``).  ``switches``: the optional tables, as
        :meth:`tables_device` takes and describes them."""
        return self._columns(C, ratios, TableSwitches(**switches))

    @staticmethod
    def _check_switches(o):
        if o.mixing and o.pair_edges is None:
            raise ValueError("mixing needs pair_edges: the envelopes are those of the pair_hist bins")
        if o.mixing and not 0 < int(o.mixing) <= 65535:
            raise ValueError("mixing: 1 .. 65535 permutations (0 or None: off)")

    def _columns(self, C, ratios, switches):
        self._check_switches(switches)
        tb = self.tables_
        rn = [r[0] for r in ratios]
        cols = {
            "cells": ["frame", "label", "class", "kind", "area", "centroid_row", "centroid_col", "min_row", "min_col",
                      "max_row1", "max_col1", "cells", "group", "group_combined"] + ["S%d" % k for k in range(C)] + rn,
            "rois": ["frame", "label", "area", "centroid_row", "centroid_col"] + ["S%d" % k for k in range(C)] + rn,
            "frames": ["frame", "n_labels", "n_rois", "particle_area", "particle_area_recreated", "tie_flag"]
                      + _per_type(tb.slot_names, "%s_present", "%s_count", "%s_density", "%s_area_ratio"),
            "distances": ["frame", "label", "nearest_other_type_um"],
            "groups": ["frame", "slot", "group", "area", "centroid_row", "centroid_col", "min_row", "min_col",
                       "max_row1", "max_col1", "members"],
        }
        cols.update((t.name, t.columns(tb.slot_names, switches)) for t in OPTIONAL_TABLES if t.on(switches))
        return cols

    # which of run_sharded's table keywords each method takes
    _TABLE_KEYWORDS = {"tables_device": ("ratios", "distances", "raster") + TableSwitches._fields,
                       "host_tables": ("ratios", "distances", "raster") + TableSwitches._fields,
                       "empty_device_tables": ("ratios",) + TableSwitches._fields}

    @classmethod
    def table_kwargs(cls, method, given):
        """The entries of ``given`` (a caller's table keywords) that ``method`` takes: each keyword only when given."""
        unknown = set(given) - set(cls._TABLE_KEYWORDS["tables_device"])
        if unknown:
            raise TypeError("unknown table keyword(s): %s" % ", ".join(sorted(unknown)))
        return {k: given[k] for k in cls._TABLE_KEYWORDS[method] if k in given}

    def tables_device(self, res, frame_ids=None, ratios=RATIOS_5, check=True, distances=False, raster=19.0, **switches):
        """The batch as dense row tables, assembled ON THE DEVICE (``csrc/tables.hip``): float64 CUDA tensors ``rois``,
        ``cells``, ``groups`` and ``frames_rec`` (one row per frame: frame id + the int64 record of
        ``pcseg_table_write``, see include/pcseg.h).  One small device-to-host copy (three row totals) sizes the
        outputs; nothing else leaves the GPU, so the tables can go straight into the all-gather.  ``distances``: also the
        nearest-other-type table of BASELINE config 5 (.m:260-268) as ``distances`` = ``[frame, label, distance]`` -- one
        batched launch over the cell rows of every frame (rows of type slot 0, then of slot 1, inside each frame); always
        present (empty unless requested) so that every rank gathers the same set of tables.

        ``switches`` are the fields of :class:`TableSwitches`, all off by default and keyword only (an unknown name is a
        ``TypeError``); :meth:`tables`, :meth:`host_tables`, :meth:`table_columns` and :meth:`empty_device_tables` take the same
        ones, and ``OPTIONAL_TABLES`` is the schema of what they add:

        ``neighbours``: also ``neighbours`` = ``[frame, label, slot, nn_um_<type>.., nn_label_<type>..]``, one row per row
        of ``cells`` in its order: the distance (same scale as ``distances``) to the nearest OTHER row of every cell type
        of the frame, NaN / -1 when there is none, and its label (refine_boundaries.py:8-12, goal 3).  ``pair_edges``
        (m + 1 increasing values from 0, in um): also ``pair_hist`` = ``[frame, slot_a, slot_b, n_pairs, bin_0..
        bin_m-1, over]``, K (K + 1) / 2 rows per frame (slot_a <= slot_b, all-zero rows included): the pairs of rows of
        the two types whose distance d lies in ``[edges[k], edges[k + 1])``, and those at ``d >= edges[m]``.

        ``mixing`` (P permutations, an int; 0 / None: off; needs ``pair_edges``, else ``ValueError``; csrc/mixing.hip): are
        two strains closer together or further apart than chance?  The random-labelling test of ``pair_hist``: the rows
        stay where they are, the slots of a frame's typed rows are shuffled P times (``mixing_seed`` and the frame's id
        set the shuffles, see ``ops.pair_label_mixing``: a frame's rows do not depend on its batch or shard).  ``mixing`` =
        ``[frame, slot_a, slot_b, bin, r_lo_um, r_hi_um, n_perm, obs, mean, lo, hi, n_le, n_ge, cum_obs, cum_mean, cum_lo,
        cum_hi, cum_n_le, cum_n_ge]``, one row per (frame, slot pair, bin), B Q m rows: the observed count of the bin, mean
        (``sum / P``), minimum and maximum of the shuffled counts, how many shuffles gave ``<= obs`` and ``>= obs``, and the
        same of the counts summed over the bins 0 .. k (the K-function form).  The one-sided Monte Carlo p-values are
        ``(1 + n_ge) / (1 + n_perm)`` for attraction and ``(1 + n_le) / (1 + n_perm)`` for segregation; they are not in the
        table.  With ``refined`` also ``refined_mixing``, over the refined rows of kind >= 1.

        ``refined`` (refine_boundaries.py:1-12, goal 2): the refined ROIs classified by their parent class-map
        component (``ops.refined_tables``).  ``refined`` = one row per row of ``rois`` (its parent, overlap, class, kind
        and cells), ``cell_resolution`` = one row per row of ``cells`` (children, resolved, cells_integrated) and
        ``frames_refined`` = one row per frame (per-type refined counts, resolved / residual clusters,
        count_integrated); with ``neighbours`` / ``pair_edges`` also ``refined_neighbours`` / ``refined_pair_hist``,
        the same tables over the refined rows of kind >= 1.  ``check`` also raises where a parent label exceeds cap, and
        ``RuntimeError`` where the h-maxima markers of a frame (``marker_h``) did not converge.

        ``surface`` (HCN_nanosims_rois_activity_distance_5iso_YG.m:271-309, the distance of every ROI to the aggregate
        boundary): where the cells sit relative to the particle.  The surface mask is ``binary_fill_holes(recreated ==
        Particle)``, its surface the mask pixels with a 4-neighbour outside it (or outside the image).  ``surface`` =
        ``[frame, label, slot, inside, surface_um, nearest_row, nearest_col]``, one row per row of ``cells`` in its
        order: whether the centroid's pixel lies in the mask, the distance (scale of ``distances``) from the centroid to
        the nearest surface pixel and that pixel (the smallest raster index among equally near ones); NaN, -1, -1 and
        inside 0 in a frame without particle.  ``frames_surface`` = ``[frame, surface_px, filled_area]``.
        ``surface_edges`` (m + 1 increasing values from 0, in um): ``surface_hist`` = ``[frame, side, slot, n, bin_0..
        bin_m-1, over]``, 2 K rows per frame in (side, slot) order (side 0 outside, 1 inside): the rows of ``surface`` by
        distance, and ``surface_shells`` = ``[frame, side, n_px, bin_0.., over]``, 2 rows per frame: the frame's pixels
        by their distance to the surface in the same bins -- ``surface_hist`` over ``surface_shells`` is the
        colonisation profile.  With ``refined`` also ``refined_surface`` / ``refined_surface_hist``: the same over the
        refined rows of kind >= 1, in the order of ``refined_neighbours``.

        ``shape``: what a ROI looks like (scikit-image 0.18.3 ``regionprops`` conventions; csrc/shape.hip).  ``shapes`` =
        ``[frame, label, slot, n_border, n_1, n_sqrt2, n_mid, mu_rr, mu_rc, mu_cc, major_um, minor_um, eccentricity,
        orientation, equivalent_diameter_um, extent, perimeter_um]``, one row per row of ``cells`` in its order: the
        border-pixel counts of ``perimeter`` (all, and by weight class 1, sqrt 2, (1 + sqrt 2) / 2), the second central
        moments per pixel (in pixels^2), the axis lengths, the equivalent diameter and the perimeter at the scale of
        ``distances``.  With ``refined`` also ``refined_shapes``: the same over the refined rows of kind >= 1.  The pass
        runs here, on the table stream; :meth:`run` does not change.

        ``convex``: one cell or a clump (csrc/hull.hip; exact, equal to scikit-image 0.18.3).  ``convexity`` = ``[frame,
        label, slot, convex_area, solidity, feret_um, euler_number, convex_area_um2]``, one row per row of ``cells`` in
        its order: the pixels of the convex hull image, area / convex_area, ``feret_diameter_max`` at the scale of
        ``distances``, the Euler number (8-connectivity: 1 - holes for a connected ROI) and the convex area / scale^2.
        With ``refined`` also ``refined_convexity``: the same over the refined rows of kind >= 1.  Runs in the table
        stage as well.

        ``territory`` (csrc/voronoi.hip; exact integers): how much of the frame a ROI has to itself and which ROIs are its
        neighbours.  The labels of kind >= 1 are the sites of the nearest-label transform; a pixel belongs to the nearest
        of them (the smallest label among equally near ones) if ``sqrt(d2) / scale < territory_reach`` (um, the scale of
        ``distances``; None: unbounded).  ``territories`` = ``[frame, label, slot, territory_px, territory_on_px,
        reach2_max, clipped, n_adj_<type>.., n_contact_<type>.., territory_um2, territory_on_um2]``, one row per row of
        ``cells`` in its order: the pixels of the territory, those on the surface mask of ``surface``, the largest squared
        distance among them, 1 if one lies on the frame's outer row or column, the partners of every type whose territory
        shares a border with this one and those the ROI touches itself, and the two areas / scale^2.  ``adjacency`` =
        ``[frame, label_a, label_b, slot_a, slot_b, border_px, contact_px]`` sorted by (frame, a, b), a < b: the
        4-neighbour pixel pairs between the two territories, and those between the two ROIs themselves.  With ``refined``
        also ``refined_territories`` / ``refined_adjacency``: the same over the refined rows of kind >= 1 on the watershed
        labels.  ``check`` also raises where a frame has more than 8 cap pairs.

        ``skeleton``: how long and how wide (csrc/skeleton.hip; exact, equal to scikit-image 0.18.3's ``morphology.thin`` of
        every ROI on its own).  ``skeletons`` = ``[frame, label, slot, skel_px, n_orth, n_diag, n_end, n_junction, passes,
        length_um, width_um]``, one row per row of ``cells`` in its order: the pixels of the ROI's skeleton, its orthogonal
        and diagonal links, the pixels with one link and with three or more (two ends and no junction: one rod; a
        junction: a clump), the full iterations the thinning took, ``(n_orth + n_diag sqrt 2)`` and ``area / length`` at the
        scale of ``distances``.  With ``refined`` also ``refined_skeletons``: the same over the refined rows of kind >= 1.
        Runs in the table stage and waits for the device between its launches."""
        o = TableSwitches(**switches)
        self._check_switches(o)
        res.synchronize()
        B, C, H, W = res["shape"]
        dev = res["stats"].device
        if check and "marker_flags" in res and int((res["marker_flags"] != 0).sum().item()):
            raise RuntimeError("the h-maxima markers of this batch did not converge (marker_flags): its refined ROIs are no result")
        if check:
            ops.check_border_flags(res.get("border_flags"))
        # a stream of its own, at high priority: the handful of small kernels here must not queue behind the next
        # batch's big ones on a saturated GPU
        if self._table_stream is None or self._table_stream.device != dev:
            self._table_stream = torch.cuda.Stream(device=dev, priority=-1)
        ts = self._table_stream
        ts.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(ts):
            ids = list(range(B)) if frame_ids is None else [int(v) for v in frame_ids]
            step = ids[1] - ids[0] if B > 1 else 1
            if all(ids[k] == ids[0] + k * step for k in range(B)):  # arithmetic progression (shards are): no upload
                fid = torch.arange(B, dtype=torch.int64, device=dev) * step + ids[0]
            else:
                fid = torch.tensor(ids, dtype=torch.int64).to(dev)
            groups = (res.get("groups") or {}) if self.merged else {}
            raw = ops.build_tables(res, groups, fid, C, ratios, check=check,  # raises what BatchResult.check() raises
                                   distance_slots=self.tables_.slot if distances else None, raster=raster, tables=self.tables_,
                                   switches=o)
            dt = {k: raw[k] for k in ("rois", "cells", "groups")}
            dt["frames_rec"] = torch.cat([fid[:, None].to(torch.float64), raw["frames"].to(torch.float64)], dim=1)
            dt["distances"] = self._distance_rows(dt["cells"], raw.get("cell_dist"))
            dt.update((t.name, t.rows(self, fid, raw)) for t in OPTIONAL_TABLES if t.on(o))
            if res._slot is not None:  # graph mode: the lane may overwrite this result once the tables are out
                res._check_alive()
                res._slot.release = torch.cuda.Event()
                res._slot.release.record(ts)
        torch.cuda.current_stream(dev).wait_stream(ts)
        for t in dt.values():
            t.record_stream(torch.cuda.current_stream(dev))
        return dt

    def _distance_rows(self, cells, cell_dist):
        """``[frame, label, distance]`` for the rows of ``cells`` that have a distance, frame by frame the rows of type
        slot 0, then those of slot 1 (the order in which the script concatenates its two ROI classes, .m:264-268)."""
        if cell_dist is None or cells.shape[0] == 0:
            return torch.zeros((0, 3), dtype=torch.float64, device=cells.device)
        keep = torch.nonzero(~torch.isnan(cell_dist))[:, 0]
        if keep.numel() == 0:
            return torch.zeros((0, 3), dtype=torch.float64, device=cells.device)
        rows = cells[keep]
        lut = torch.from_numpy(self.tables_.slot.astype("int64")).to(cells.device)
        slot = lut[rows[:, 2].to(torch.int64)]
        # rows are in (frame position, label) order already: a STABLE sort by slot inside each frame keeps labels ascending
        pos = torch.cumsum(torch.cat([rows.new_zeros(1), (rows[1:, 0] != rows[:-1, 0]).to(rows.dtype)]), 0).to(torch.int64)
        order = torch.sort(pos * 2 + slot, stable=True)[1]
        return torch.stack([rows[order, 0], rows[order, 1], cell_dist[keep][order]], dim=1)

    def _neighbour_rows(self, cells, dist, nn_id):
        """``[frame, label, slot, nn_um_<type>.., nn_label_<type>..]`` for every row of ``cells``."""
        lut = torch.from_numpy(self.tables_.slot.astype("int64")).to(cells.device)
        slot = lut[cells[:, 2].to(torch.int64)].to(torch.float64)
        return torch.cat([cells[:, :2], slot[:, None], dist, nn_id.to(torch.float64)], dim=1)

    def _pair_rows(self, fid, hist):
        """``[frame, slot_a, slot_b, n_pairs, bins.., over]``: K (K + 1) / 2 rows per frame, slot pairs in (a <= b) order."""
        B, P = hist.shape[0], hist.shape[1]
        K = len(self.tables_.slot_names)
        ab = torch.tensor([(a, b) for a in range(K) for b in range(a, K)], dtype=torch.float64, device=hist.device)
        return torch.cat([fid.to(torch.float64)[:, None, None].expand(B, P, 1), ab[None].expand(B, P, 2),
                          hist.to(torch.float64)], dim=2).reshape(B * P, -1)

    def _mixing_rows(self, fid, mix, args):
        """``[frame, slot_a, slot_b, bin, r_lo_um, r_hi_um, n_perm, obs, mean, lo, hi, n_le, n_ge, cum_..]``: one row per
        (frame, slot pair, bin) of ``ops.pair_label_mixing``'s tensors; ``args`` = (edges, P)."""
        edges, P = args
        B, Q, m = mix["obs"].shape
        K = len(self.tables_.slot_names)
        dev = mix["obs"].device
        ab = torch.tensor([(a, b) for a in range(K) for b in range(a, K)], dtype=torch.float64, device=dev)
        e = torch.as_tensor(np.asarray(edges, np.float64).reshape(-1)).to(dev)
        bins = torch.stack([torch.arange(m, dtype=torch.float64, device=dev), e[:-1], e[1:]], dim=1)
        f64 = lambda k: mix[k].to(torch.float64)[:, :, :, None]
        per = torch.full((B, Q, m, 1), float(P), dtype=torch.float64, device=dev)  # tensor divisor: a correctly rounded division
        half = lambda c: [f64(c + "obs"), f64(c + "sum") / per, f64(c + "lo"), f64(c + "hi"), f64(c + "n_le"), f64(c + "n_ge")]
        return torch.cat([fid.to(torch.float64)[:, None, None, None].expand(B, Q, m, 1), ab[None, :, None, :].expand(B, Q, m, 2),
                          bins[None, None].expand(B, Q, m, 3), per] + half("") + half("cum_"), dim=3).reshape(B * Q * m, -1)

    def _point_rows(self, fid, points, *columns):
        """``[frame, label, slot, columns..]`` for every point of a packed point set (``ops.Points``)."""
        foff, ids = points.frame_offsets, points.ids
        frame = torch.repeat_interleave(fid.to(torch.float64), foff[1:] - foff[:-1], output_size=ids.shape[0])
        f64 = lambda t: t.to(torch.float64) if t.dim() == 2 else t.to(torch.float64)[:, None]
        return torch.cat([f64(frame), f64(ids), f64(points.slot)] + [f64(c) for c in columns], dim=1)

    def _side_rows(self, fid, hist):
        """(B, 2, m + 2) or (B, 2, K, m + 2) counts -> ``[frame, side, (slot,) n, bins.., over]`` rows, (side, slot) order."""
        B = hist.shape[0]
        keys = [(s,) for s in range(2)] if hist.dim() == 3 else [(s, t) for s in range(2) for t in range(hist.shape[2])]
        key = torch.tensor(keys, dtype=torch.float64, device=hist.device)
        R = len(keys)
        return torch.cat([fid.to(torch.float64)[:, None, None].expand(B, R, 1), key[None].expand(B, R, key.shape[1]),
                          hist.reshape(B, R, -1).to(torch.float64)], dim=2).reshape(B * R, -1)

    def empty_device_tables(self, C, ratios=RATIOS_5, device=None, **switches):
        """What :meth:`tables_device` returns for zero frames (a rank that owns no frame of a dataset), with its ``switches``."""
        cols = self._columns(C, ratios, TableSwitches(**switches))
        mk = lambda n: torch.zeros((0, n), dtype=torch.float64, device=device)
        out = {"rois": mk(len(cols["rois"])), "cells": mk(len(cols["cells"])), "groups": mk(len(cols["groups"])),
               "frames_rec": mk(18), "distances": mk(3)}
        for k in _EXTRA_TABLES:
            if k in cols:
                out[k] = mk(len(cols[k]))
        return out

    def host_tables(self, dt, C, ratios=RATIOS_5, distances=False, raster=19.0, **switches):
        """numpy tables from (downloaded or gathered) :meth:`tables_device` output: ``cells`` / ``rois`` / ``groups`` /
        ``distances`` as they are, ``frames`` after the two ``round(x, 5)`` of get_cell_counts_and_densities
        (tiff_analysis.py:1018-1038; Python's decimal rounding, a handful of numbers per frame).  Every table's width
        must be the one :meth:`table_columns` names for ``C`` planes, these ``ratios`` and the ``switches`` the tables were
        made with (those of :meth:`tables_device`)."""
        cols = self._columns(C, ratios, TableSwitches(**switches))
        host = _download(dt)
        tb = self.tables_
        out = {k: host[k] for k in ("cells", "rois", "groups")}
        for k in out:
            if out[k].shape[1] != len(cols[k]):
                raise ValueError("table %r has %d columns, the schema for %d planes names %d" % (k, out[k].shape[1], C, len(cols[k])))
        rec = host["frames_rec"]
        px2 = ta.PX_TO_UM_CONV ** 2
        frame_rows = []
        n_slots = len(tb.slot_names)
        nan = float("nan")
        for row_rec in rec.tolist():  # plain Python floats: indexing numpy scalars one by one cost 50 us per frame
            row = row_rec[:6]
            pa_um = row_rec[3] / px2
            for s in range(n_slots):
                present, count, area_px = int(row_rec[6 + 3 * s]), int(row_rec[7 + 3 * s]), int(row_rec[8 + 3 * s])
                ok = present and pa_um
                row += [float(present), float(count), round(count / pa_um, 5) if ok else nan,
                        round((area_px / px2) / pa_um, 5) if ok else nan]
            frame_rows.append(row)
        out["frames"] = np.array(frame_rows, np.float64).reshape(len(frame_rows), len(cols["frames"]))
        # the nearest-other-type table comes from the device (tables_device(distances=True)); without it an empty table
        if distances and "distances" not in host:
            raise ValueError("host_tables(distances=True) needs tables made by tables_device(..., distances=True)")
        out["distances"] = host["distances"].reshape(-1, 3) if distances and "distances" in host else np.zeros((0, 3), np.float64)
        for k in _EXTRA_TABLES:
            if k in cols:
                if k not in host:
                    raise ValueError("host_tables(%s) needs tables made by tables_device with it" % k)
                out[k] = host[k].reshape(-1, len(cols[k]))
        for k, v in cols.items():
            out[k + "_columns"] = v
        return out

    def agreement(self, res, truth, of="refined", thresholds=(0.5, 0.75, 0.9), frame_ids=None, truth_cap=None, pair_cap=None):
        """Score one batch's segmentation against a truth label image: ``truth`` int32 (B, H, W) CUDA tensor (0: background),
        ``of`` = "refined" (``res["ws_labels"]``, labels 1 .. ``res["n_markers"]``) or "components" (``res["labels"]``,
        labels 1 .. ``res["counts"]``).  Returns numpy tables with ``<name>_columns`` lists (``ops.agreement_tables``):
        ``agreement_pairs`` -- frame, truth, label, px, truth_area, area, iou for every pair of a truth label and a ROI that
        share pixels --, ``agreement_rois`` (one row per ROI with pixels: its best truth label, the overlap, the IoU, the
        number of partners and ``matched_<tau>`` per IoU threshold), ``agreement_truth`` (the mirror image) and
        ``frames_agreement`` (per frame n_truth, n_rois; tp, fp, fn, precision, recall, f1, ap and mean_matched_iou per
        threshold; adapted Rand error with its precision and recall; the two halves of the variation of information).  A
        label is matched at tau when its best partner covers more than half of their union and ``iou >= tau``
        (``ops.label_agreement``).  ``truth_cap``: the largest truth label (default: read back).  RuntimeError where a frame
        has more pairs than ``pair_cap`` (default: 4 x the label caps).  ``res`` is only read."""
        if of not in ("refined", "components"):
            raise ValueError('of must be "refined" or "components"')
        labels, counts = (res["ws_labels"], res["n_markers"]) if of == "refined" else (res["labels"], res["counts"])
        if not isinstance(truth, torch.Tensor) or truth.dtype != torch.int32 or tuple(truth.shape) != tuple(labels.shape):
            raise TypeError("truth must be an int32 CUDA tensor of the batch's (B, H, W)")
        cap_s = max(int(counts.max().item()), 1)
        ag = ops.label_agreement(truth, labels, thresholds, cap_t=truth_cap, cap_s=cap_s, pair_cap=pair_cap)
        ops.check_agreement_overflow(ag)
        return ops.agreement_tables(ag, frame_ids)

    def borders(self, res, frame_ids=None, conn=8, raster=19.0, pair_cap=None):
        """The borders between the refined ROIs of one batch, weighed by the boundary plane (``ops.label_borders`` on
        ``res["ws_labels"]`` and the boundary plane of the input ``res`` was run on (the result keeps a reference to it) -- with ``merge_below`` these are the borders that survived
        the merge).  Returns ``{"borders": float64 numpy rows, "borders_columns": [...]}``, one row per pair of touching ROIs
        sorted by (frame, roi_a, roi_b): the frame's id (``frame_ids``; default: its position), ``roi_a`` < ``roi_b``,
        ``links`` (4- or 8-neighbour pixel pairs across the border, ``conn``), ``mean`` and ``saddle`` (the mean and the
        smallest boundary probability along it) and ``length_um`` = ``links`` at ``512 / raster`` pixels per um (the
        scale of ``distances``).
        RuntimeError where a frame has more pairs than ``pair_cap`` (default: 4 x the largest ROI count).  ``res`` is only
        read."""
        stack = getattr(res, "_stack", None)
        if stack is None:
            raise TypeError("borders needs a result of run(): it reads the boundary plane of the run's input")
        labels = res["ws_labels"]
        B = labels.shape[0]
        fid = np.arange(B, dtype=np.float64) if frame_ids is None else np.asarray(frame_ids, np.float64)
        if fid.shape != (B,):
            raise ValueError("frame_ids must name every frame of the batch")
        bd = ops.label_borders(labels, stack[:, self.boundary_plane], conn=conn, cap=max(int(res["n_markers"].max().item()), 1), pair_cap=pair_cap)
        if bd["n_overflow"]:
            raise RuntimeError("the border table of frame(s) %s is full: pair_cap = %d is too small"
                               % ([int(b) for b in torch.nonzero((bd["overflow"] & 1).cpu())[:, 0]], bd["pair_cap"]))
        host = {k: bd[k].cpu().numpy() for k in ("frame", "a", "b", "links", "mean", "saddle")}
        rows = np.stack([fid[host["frame"]], host["a"], host["b"], host["links"], host["mean"], host["saddle"].astype(np.float64),
                         host["links"] / (512.0 / float(raster))], axis=1).astype(np.float64).reshape(-1, 7)
        return {"borders": rows, "borders_columns": ["frame", "roi_a", "roi_b", "links", "mean", "saddle", "length_um"]}

    def _window_points(self, res, edges, window, of, frame_ids, raster):
        """What :meth:`clustering` and :meth:`neighbourhoods` are made from, after their refusals: ``(fid, window, points, rc)``
        -- the frames' ids (numpy float64), the window as a uint8 (B, H, W) tensor, the points of ``pair_hist`` /
        ``refined_pair_hist`` (:class:`ops.Points`) and their (row, col) centroids."""
        if of not in ("cells", "refined"):
            raise ValueError('of must be "cells" or "refined"')
        if isinstance(window, str) and window not in ("particle", "frame"):
            raise ValueError('window must be "particle", "frame" or a uint8 (B, H, W) CUDA tensor')
        B, C, H, W = res["shape"]
        fid = np.arange(B, dtype=np.float64) if frame_ids is None else np.asarray(frame_ids, np.float64)
        if fid.shape != (B,):
            raise ValueError("frame_ids must name every frame of the batch")
        if not isinstance(window, str):
            window = ops._req(window, torch.uint8, 3)
            if tuple(window.shape) != (B, H, W):
                raise ValueError("window must have the batch's (B, H, W)")
        spatial._reach_within_limit(edges, 512.0 / float(raster))  # edges the library refuses: ValueError before any launch
        tb = self.tables_
        dev = res["stats"].device
        if isinstance(window, str):
            window = (ops.particle_mask(res["recreated"], tb.particle_value) if window == "particle"
                      else torch.ones((B, H, W), dtype=torch.uint8, device=dev))
        pos = torch.arange(B, dtype=torch.int64, device=dev)
        groups = (res.get("groups") or {}) if self.merged else {}
        _, d = ops._dense_tables(res, groups, pos, C, (), True)
        if of == "cells":
            points = ops._pack_cells("neighbours_pack_cells", d, tb.slot)
            rc = ops._pack_cells("surface_pack_cells", d, tb.slot).coords
        else:
            points = ops.refined_tables(res, pos, tb, d.ws, (d.n_roi, d.n_cell), check=True, points=True)["points"]
            rc = ops._refined_centroids(res, points)
        return fid, window, points, rc

    def clustering(self, res, edges, window="particle", of="cells", frame_ids=None, raster=19.0):
        """Are the cells of one batch clumped or spread evenly over the window they can sit in?  Observed pair counts against
        complete spatial randomness on that window, exactly (``spatial.window_pair_counts``, csrc/window_pairs.hip): no edge
        correction, no simulation.  ``edges``: m + 1 increasing values from 0, in um at ``512 / raster`` pixels per um (the
        scale of ``distances``).  ``window``: "particle" (``ops.particle_mask(res["recreated"], <Particle value>)``, the mask of
        the surface tables), "frame" (every pixel) or a uint8 (B, H, W) CUDA tensor (non-zero: in the window).  ``of``:
        "cells" (the rows of ``cells``) or "refined" (the refined rows of kind >= 1): the points, slots and order of
        ``pair_hist`` / ``refined_pair_hist``.  A point is in the window when the mask is set at pixel ``(floor(row + 0.5),
        floor(col + 0.5))`` of its centroid (the rule of ``surface``'s ``inside``); the others are left out of the observed
        counts, which are ``ops.point_neighbours``' histogram of the rest.  Returns numpy tables with ``<name>_columns`` lists:
        ``window_pairs`` = ``[frame, n_px, bin_0 .. bin_m-1, over]``, one row per frame: the window's pixels A and the ordered
        pairs of window pixels (self pairs included) per distance bin, ``over`` the rest of the A^2 pairs -- exact integers,
        stored as float64 like every table: exact up to 2^53; ``clustering`` = ``[frame, slot_a, slot_b, bin, r_lo_um, r_hi_um,
        n_a, n_b, n_out_a, n_out_b, obs, window_pairs, expected, ratio, cum_obs, cum_window_pairs, cum_expected, cum_ratio]``,
        one row per (frame, slot pair a <= b, bin): the points of the two slots in the window and left out, the observed
        pairs, the window's count G of the bin, ``expected = (npairs * G) / (A * A)`` with ``npairs = n_a (n_a - 1) / 2`` (a ==
        b) or ``n_a n_b`` -- the expectation for points placed independently and uniformly on the window's pixels --, ``ratio =
        obs / expected`` (above 1: clustering at that range, below 1: spacing) and the same of the counts summed over the
        bins 0 .. k (the K-function form); NaN where A == 0 or expected == 0.  ``frame_ids`` as in :meth:`borders`.
        ``res`` is only read."""
        fid, window, points, rc = self._window_points(res, edges, window, of, frame_ids, raster)
        tb = self.tables_
        out = _download(spatial._clustering_tables(points, rc, window, edges, 512.0 / float(raster), len(tb.slot_names), fid))
        out.update((k + "_columns", v) for k, v in spatial.clustering_columns(edges).items())
        return out

    def neighbourhoods(self, res, edges, window="particle", of="cells", frame_ids=None, raster=19.0):
        """What lies around ONE cell of a batch: for every typed point and every distance bin the cells of each strain, the
        pixels of each strain and the pixels of the window in that ring around it (``local.point_counts``, ``local.disk_counts``,
        csrc/local_counts.hip) -- the per-cell marks of :meth:`clustering`: the local K-function with its edge-correction term
        and a segregation index per cell.  ``edges``, ``window``, ``of``, ``frame_ids`` and ``raster`` mean what they mean in
        :meth:`clustering`; the points, slots and row order are those of ``pair_hist`` / ``refined_pair_hist``, and a point is in
        the window by the same ``(floor(row + 0.5), floor(col + 0.5))`` rule.  A point outside the window counts for nobody
        (``clustering`` leaves it out of ``obs`` in the same way).  The pixel sets are the window and, per type slot, the pixels
        of ``res["denoised"]`` whose class value maps to the slot -- no resolved cells are needed, so the pixel columns also
        describe unresolved clusters; the query pixel of a point is its rounded centroid.
        Returns ``{"neighbourhoods": float64 numpy rows, "neighbourhoods_columns": [...]}`` (``local.neighbourhood_columns``), one
        row per (typed point, bin) in point order then bin order: ``frame``, ``label``, ``slot``, ``in_window``, ``bin``,
        ``r_lo_um``, ``r_hi_um``; ``win_px`` / ``cum_win_px``, the window's pixels in the ring and in the disk up to the bin (how
        much of the particle lies within that distance: a cell at the rim has less of it, and looks lonely for that reason
        alone); per type slot ``n_<t>`` / ``cum_n_<t>`` (the OTHER in-window points of the slot), ``px_<t>`` / ``cum_px_<t>`` (the
        strain's pixels, the cell's own included) and ``expected_<t>`` / ``cum_expected_<t>`` = ``(N_t * win_px) / A`` with ``N_t``
        the slot's in-window points, less one for the row's own slot, and ``A`` the window's area -- the count expected around
        this cell for points placed uniformly on the window; NaN where A == 0; then ``own_frac = cum_n_own / sum_t cum_n_t`` and
        ``own_px_frac = cum_px_own / sum_t cum_px_t``, NaN where the denominator is 0.  The row of a point outside the window has
        ``in_window = 0`` and NaN in every count column.  For every frame, slot pair a <= b and bin the sum of ``n_<b>`` over the
        in-window rows of slot a is ``clustering``'s ``obs`` (twice it when a == b).
        The lattice caveat of DESIGN section 22 holds here too: the window and the pixel sets are counted from the ROUNDED
        centroid on the pixel lattice, while the point counts use the unrounded centroids -- below a few pixels ``expected``
        carries the lattice's steps, and bins narrower than a pixel are better merged.  ``res`` is only read."""
        fid, window, points, rc = self._window_points(res, edges, window, of, frame_ids, raster)
        tb = self.tables_
        K = len(tb.slot_names)
        planes = local.set_planes(window, res["denoised"], tb.slot)
        out = _download(local.neighbourhood_tables(points, rc, planes, edges, 512.0 / float(raster), K, fid))
        out["neighbourhoods_columns"] = local.neighbourhood_columns(list(tb.slot_names), edges)
        return out

    def gaps(self, res, of="cells", reach=None, frame_ids=None, raster=19.0):
        """How far is every ROI of one batch from the nearest OTHER ROI of each strain, rim to rim?  The gap of two ROIs is the
        smallest distance between a pixel of one and a pixel of the other (``gaps.label_gaps``, csrc/gaps.hip): exact, where
        ``neighbours`` measures between centroids -- which for rods and for unresolved clusters can lie many pixels from the
        rim.  ``of``: "cells" (the class-map components of kind >= 1: one row per row of ``cells``) or "refined" (the refined
        rows of kind >= 1): the rows, slots and order of ``neighbours`` / ``refined_neighbours``.  ``reach``: in um at ``512 /
        raster`` pixels per um (the scale of ``distances``), gaps of ``reach`` and more count as none; None: unbounded.
        Returns ``{"gaps": float64 numpy rows, "gaps_columns": [...]}`` (``gaps.gap_columns``): ``frame`` (``frame_ids`` as in
        :meth:`borders`), ``label``, ``slot``, then per type slot ``gap_um_<type>`` (``sqrt(gap_px2) / scale``; NaN where there
        is no other ROI of that type), ``gap_label_<type>`` (the nearest one, the smallest label among equally near ones; -1
        for none) and ``gap_px2_<type>`` (the squared gap in pixels; -1 for none).  Refined ROIs flooded against each other
        have ``gap_px2 == 1`` (or 2 where they meet only diagonally); components of one class are never closer than
        ``gap_px2 == 4`` (they are 8-connected components: two of them cannot have neighbouring pixels), components of
        different classes can touch.  ``gap_px2_<t> == 1`` exactly where ``territories`` reports ``n_contact_<t> > 0``.
        ``res`` is only read."""
        if of not in ("cells", "refined"):
            raise ValueError('of must be "cells" or "refined"')
        B, C, H, W = res["shape"]
        fid = np.arange(B, dtype=np.float64) if frame_ids is None else np.asarray(frame_ids, np.float64)
        if fid.shape != (B,):
            raise ValueError("frame_ids must name every frame of the batch")
        scale = 512.0 / float(raster)
        r2 = ops.reach_um_r2(reach, scale)
        tb = self.tables_
        names = list(tb.slot_names)
        dev = res["stats"].device
        if of == "cells":
            rows = ops.class_rows(res)
        else:
            pos = torch.arange(B, dtype=torch.int64, device=dev)
            groups = (res.get("groups") or {}) if self.merged else {}
            _, d = ops._dense_tables(res, groups, pos, C, (), True)
            rt = ops.refined_tables(res, pos, tb, d.ws, (d.n_roi, d.n_cell), check=True)
            rows = ops.refined_rows(res, rt["kind_r"], rt["slot_r"])
        table = gaps.gap_rows(rows.labels, rows.live, rows.slot_of, torch.from_numpy(fid).to(dev), scale, names, r2)
        return {"gaps": table.cpu().numpy().reshape(-1, 3 + 3 * len(names)), "gaps_columns": gaps.gap_columns(names)}

    def tables(self, res, frame_ids=None, ratios=RATIOS_5, distances=False, raster=19.0, check=True, **switches):
        """Download one batch as numpy tables: ``cells`` (one row per cell / cluster region), ``rois`` (one row per
        refined ROI), ``frames`` (one row per frame) and ``groups`` (one row per merged group): :meth:`tables_device`
        followed by :meth:`host_tables`.  ``check=False`` skips ``BatchResult.check`` (a caller that has looked at the
        flags itself, e.g. to keep the ROI rows of a batch in which the reference would have raised on one frame's
        cluster statistics).  ``switches``: the optional tables, as :meth:`tables_device` takes and describes them."""
        dt = self.tables_device(res, frame_ids, ratios, check, distances, raster, **switches)
        return self.host_tables(dt, res["shape"][1], ratios, distances, raster, **switches)
