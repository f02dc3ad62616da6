// Union-find over "parent images": the fenced walks, finds and unions of the CCL family (ccl.hip), the proximity merges
// (reduce.hip), the border merges (borders.hip) and the watershed's label assignment (watershed.hip) -- the only copies.
#pragma once
#include "common.h"

namespace pcseg {

// ---- node policies: which slot of the image stores a node's parent, and the fence that holds a walk over it
//
// WALKS ARE FENCED.  In a well-formed union-find image the entry stored at index x is a smaller-or-equal index of the same
// set and never negative (roots are minima; unions only ever lower an entry), so a walk is strictly decreasing: finite and
// inside [0, x].  `walk_ok` is ONE unsigned compare that holds a walk to exactly that, whatever the array contains -- an
// image that is being rewritten by another instance of the same chain (one captured graph replayed on several streams at
// once: profiles/r03/exp_graph_r3a.log) or roots handed in by a caller (pcseg_compact_labels) then
// ends in an error flag (`corrupt`, may be null: the walk just stops) instead of a load from a wild address or a loop
// that never ends.
__device__ __forceinline__ bool walk_ok(int x, int p) { return (unsigned)p <= (unsigned)x; }
__device__ __forceinline__ void walk_corrupt(int *corrupt)
{
    if (corrupt) __hip_atomic_store(corrupt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// plain nodes: a node is the index its parent is stored at
struct PlainNodes {
    __device__ __forceinline__ int slot(int x) const { return x; }
    __device__ __forceinline__ bool ok(int x, int p) const { return walk_ok(x, p); }
};

// VIRTUAL nodes (the watershed's label assignment): a seed has node `index`, a non-seed `index + NS` (NS a power of two
// above every index), so that every seed precedes every other pixel and the root of a component that holds a seed IS a seed.
// The walks over the frame-wide parent image are FENCED like the plain ones (walk_ok): an entry stored for the node
// with virtual index x is a virtual index <= x (roots are minima of the virtual order, unions only lower entries) whose
// pixel lies inside the frame.  Anything else -- the image being rewritten by a second instance of the same captured chain
// (profiles/r03/exp_graph_r3a.log), a stale workspace -- stops the walk and raises the frame's tie flag (the exact flood
// then recomputes the frame in mode 0, mode 2 reports it) instead of loading from a wild address or walking for ever.
// (n: pixels of the frame; the LDS finds and unions are not fenced and need none)
template <int NS>
struct VirtualNodes {
    int n = 0;
    __device__ __forceinline__ int slot(int x) const { return x & (NS - 1); }
    __device__ __forceinline__ bool ok(int x, int p) const { return walk_ok(x, p) && slot(p) < n; }
};

// ---- LDS union-find
// (relaxed workgroup-scope atomic accesses, not `volatile`: the compiler keeps a volatile access through a pointer
// argument in the generic address space -- flat_load / flat_store instead of ds_read / ds_write, 68 of them in the
// watershed tile pass -- while it does infer LDS for these)
__device__ __forceinline__ int ld_lds(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st_lds(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// find_lds<UF_HALVING>, unite_lds<UF_HALVING>: with path halving (long chains: the lake components of the watershed's second
// level wind through a tile)
constexpr bool UF_HALVING = true;
template <bool HALVING = false, typename Nodes = PlainNodes>
__device__ __forceinline__ int find_lds(int *par, int x, Nodes nodes = Nodes())
{
    int p;
    while ((p = ld_lds(par + nodes.slot(x))) != x) {
        if (HALVING) {
            const int g = ld_lds(par + nodes.slot(p));
            if (g != p) st_lds(par + nodes.slot(x), g);  // re-pointing x at its grandparent keeps it in its set (parents only ever decrease)
            p = g;
        }
        x = p;
    }
    return x;
}
template <bool HALVING = false, typename Nodes = PlainNodes>
__device__ __forceinline__ void unite_lds(int *par, int a, int b, Nodes nodes = Nodes())
{
    for (;;) {
        a = find_lds<HALVING>(par, a, nodes);
        b = find_lds<HALVING>(par, b, nodes);
        if (a == b) return;
        if (a < b) { int t = a; a = b; b = t; }
        int old = atomicMin(&par[nodes.slot(a)], b);
        if (old == a) return;
        a = old;
    }
}
// the same with both walks in lockstep (two independent LDS reads per step).  Pays in the class-map tile pass (451 -> 434
// us); the run-based tile pass got slower with it (155 -> 168 us) and so did the watershed's, which is bound by its
// vector instructions, not by LDS latency (360 -> 424 us): they keep the plain form.
__device__ __forceinline__ void unite_lds_pair(int *par, int a, int b)
{
    for (;;) {
        for (;;) {
            if (a == b) return;
            const int pa = ld_lds(par + a), pb = ld_lds(par + b);
            if (pa == a && pb == b) break;
            a = pa;
            b = pb;
        }
        if (a < b) { int t = a; a = b; b = t; }
        int old = atomicMin(&par[a], b);
        if (old == a) return;
        a = old;
    }
}

// ---- global union-find (parents only ever decrease; stale reads cost iterations, never correctness)

// plain (read-only) walk to the root of x; x must be a valid node (its slot inside the image)
template <typename Nodes = PlainNodes>
__device__ __forceinline__ int walk_root(const int *par, int x, int *corrupt = nullptr, Nodes nodes = Nodes())
{
    int q;
    while ((q = par[nodes.slot(x)]) != x) {
        if (!nodes.ok(x, q)) {
            walk_corrupt(corrupt);
            break;
        }
        x = q;
    }
    return x;
}

template <typename Nodes = PlainNodes>
__device__ __forceinline__ int find_glb(int *par, int x, int *corrupt = nullptr, Nodes nodes = Nodes())
{
    // path halving: re-pointing x at its grandparent is always valid (any ancestor is) and races are benign
    int p;
    while ((p = ld_agent(par + nodes.slot(x))) != x) {
        if (!nodes.ok(x, p)) { walk_corrupt(corrupt); return x; }
        int g = ld_agent(par + nodes.slot(p));
        if (!nodes.ok(p, g)) { walk_corrupt(corrupt); return p; }
        if (g != p) __hip_atomic_store(par + nodes.slot(x), g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;
    }
    return x;
}
// the two walks to the roots advance in LOCKSTEP (path halving on both, as in find_glb): a step of the pair is two
// independent loads in flight instead of one, and the border passes are nothing but these dependent walks.
// Returns false (and raises `corrupt`) when an entry breaks the fence: the caller must not link anything then.
template <typename Nodes = PlainNodes>
__device__ __forceinline__ bool find2_glb(int *par, int &a, int &b, int *corrupt = nullptr, Nodes nodes = Nodes())
{
    for (;;) {
        if (a == b) return true;
        const int pa = ld_agent(par + nodes.slot(a)), pb = ld_agent(par + nodes.slot(b));
        if (pa == a && pb == b) return true;
        if (!nodes.ok(a, pa) || !nodes.ok(b, pb)) break;
        const int ga = ld_agent(par + nodes.slot(pa)), gb = ld_agent(par + nodes.slot(pb));
        if (!nodes.ok(pa, ga) || !nodes.ok(pb, gb)) break;
        if (pa != a) {
            if (ga != pa) __hip_atomic_store(par + nodes.slot(a), ga, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a = ga;
        }
        if (pb != b) {
            if (gb != pb) __hip_atomic_store(par + nodes.slot(b), gb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            b = gb;
        }
    }
    walk_corrupt(corrupt);
    return false;
}
template <typename Nodes = PlainNodes>
__device__ __forceinline__ void unite_glb(int *par, int a, int b, int *corrupt = nullptr, Nodes nodes = Nodes())
{
    for (;;) {
        if (!find2_glb(par, a, b, corrupt, nodes)) return;
        if (a == b) return;
        if (a < b) { int t = a; a = b; b = t; }
        int old = atomicMin(par + nodes.slot(a), b);
        if (old == a) return;
        if (!nodes.ok(a, old)) { walk_corrupt(corrupt); return; }
        a = old;
    }
}

// ---- the election of a quad label pass (ccl_relabel_quads_kernel, ws_uf_label4_kernel): a lane holds the parent entries
// of four adjacent pixels (-1 = none) and walks a chain for its first one, the `lead` -- but neighbouring lanes mostly carry
// the same lead: only the first lane of each run of equal leads walks (the return value: this lane heads a run), the others
// read its answer from `head_lane`.  A quad that straddles a component border holds a second entry (`lead2`, -1 = none);
// `third` is raised (never cleared) where it holds a further one still.  Every lane of the wave must call.
// (outputs by reference and the third entry found in a loop of its own: returned as a struct, or with the two loops as one,
// ccl_relabel_quads_kernel goes from 60 vector registers to 64 and 12 bytes of scratch)
__device__ __forceinline__ bool elect_quad(const int4 &p4, int &lead, int &lead2, int &head_lane, bool &third)
{
    const int pv[4] = {p4.x, p4.y, p4.z, p4.w};
    const int lane = lane_id();
    lead = pv[0] >= 0 ? pv[0] : (pv[1] >= 0 ? pv[1] : (pv[2] >= 0 ? pv[2] : pv[3]));
    const int left = __shfl_up(lead, 1);
    const bool head = lane == 0 || lead != left;
    const unsigned long long heads = __ballot(head);
    head_lane = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
    lead2 = -1;
#pragma unroll
    for (int j = 1; j < 4; ++j)
        if (pv[j] >= 0 && pv[j] != lead && lead2 < 0) lead2 = pv[j];
#pragma unroll
    for (int j = 2; j < 4; ++j)
        if (pv[j] >= 0 && pv[j] != lead && pv[j] != lead2) third = true;
    return head;
}

}  // namespace pcseg
