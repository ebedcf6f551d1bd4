// pt_sweep_skip.h — the box sweep's skip table: the leaf tests a bounce need not issue because it starts on their plane.
//
// A diffuse bounce starts on the triangle it just hit.  Where that triangle's group has a box that is flat on axis a at
// coordinate c, every triangle of the group has p0.a == p1.a == p2.a == c, and so has every triangle of every other group whose
// box is flat on a at the same c (a wall split in two, a light set into a ceiling).  For an origin with o.a == c, exactly, the
// leaf test of such a triangle (pt_trace.h: leaf_test_slot) keeps nothing, whatever the direction:
//   - e1.a and e2.a are c - c = +0, and s.a = o.a - p0.a is +-0;
//   - of s2 = s x e1 the two components other than a are (+-0 * x) - (y * +-0): +-0, or NaN where an operand is infinite;
//   - dot(e2, s2) adds e2.a * s2.a = +-0 * s2.a to two products with those components: +-0, or NaN;
//   - tt = that * inv_divisor is +-0 or NaN, and `tt > ray.tnear` fails for tnear = 1e-4 and for tnear = 0.
// The test writes nothing and never reaches the tie branch, so leaving it out changes no state.  The sweep finds such a group
// all the same (on axis a its slab gives (c - o.a) * inv = +-0 for near and far, on the other axes the origin lies inside), so
// today every bounce off a wall tests the wall it left.
//
// The table has one entry per PRIMITIVE, indexed by the primitive a segment ended on: the flat axis of its group, c, and a mask
// in the bit order of the lane's hit word (group k = bit 31 - k, k in the order of the table the launch sweeps) of every group
// that is flat on that axis at a float-equal c (-0.0 == +0.0: the subtraction above gives +-0 either way).  A group whose box is
// not flat has mask 0.  The kernel compares the new origin's coordinate with c and clears the mask out of the hit word when they
// are equal (pt_trace_sweep_body.h); equality is required — one ulp off the plane the test can keep a hit.
//
// A box flat on two axes uses the lower one.  "Flat" is asked of the box AND of the nine vertex coordinates it stands for: the
// argument above is about vertices, and a box that did not contain them would not carry it.
//
// The header needs no HIP header, so the CPU test tests/native/sweep_skip_check.cpp runs the same code.
#pragma once
#include <stdint.h>
#include <string.h>

#include "pt_sweep_layout.h"

namespace ptl {

// option "sweep_self_skip"
constexpr int kSweepSelfSkipOff = 0, kSweepSelfSkipOn = 1;

struct SweepSkipEntry {
    float c;             // the plane's coordinate on `axis`
    uint32_t mask;       // groups flat on `axis` at c, group k = bit 31 - k; 0: the primitive's group is not flat
    uint32_t axis;       // 0 .. 2; 0 where mask is 0
};
static_assert(sizeof(SweepSkipEntry) == 12, "12 bytes per primitive");

// Bytes a block stages: one entry per primitive, rounded up to the 16 bytes stage_to_lds copies at a time.
PT_SWEEP_HD uint32_t sweep_skip_bytes(uint32_t num_prims) { return (num_prims * (uint32_t)sizeof(SweepSkipEntry) + 15u) & ~15u; }
// A table as the handle keeps it: room for kSweepMaxPrims entries whatever the scene, so that the rounded-up read stays inside.
constexpr uint32_t kSweepSkipTableBytes = kSweepMaxPrims * (uint32_t)sizeof(SweepSkipEntry);
static_assert(kSweepSkipTableBytes % 16u == 0, "sweep_skip_bytes(kSweepMaxPrims) is the table");
// The entries are staged behind the slot records, inside the region the octant node tables of the tree kernel would take.
// For a binary tree it always fits: 192 G + 64 + 48 N + 12 N + 12 <= 252 N + 76 against 512 (N - 1) + 128 for N >= 2.
PT_SWEEP_HD uint32_t sweep_skip_off(uint32_t groups, uint32_t num_prims) { return sweep_layout_bytes(groups, num_prims); }
PT_SWEEP_HD bool sweep_skip_fits(uint32_t groups, uint32_t num_prims, uint32_t num_nodes, uint32_t node_stride) {
    return sweep_skip_off(groups, num_prims) + sweep_skip_bytes(num_prims) <= 8u * oct_table_pitch(num_nodes, node_stride);
}

// What the info keys "sweep_skip_groups" and "sweep_skip_planes" report.
struct SweepSkipInfo {
    uint32_t groups;     // groups with a non-zero mask
    uint32_t planes;     // distinct (axis, c) among them
};

// The flat axis of group g (the lowest), or -1: its box is flat there and all its primitives are triangles with every vertex
// on that plane.
inline int sweep_group_flat_axis(const SweepGroup& g, const DNode* nodes, int num_nodes, uint32_t node_stride, const DPrim* prims,
                                 int num_prims, float* c) {
    const uint32_t node = g.box_off / node_stride, rest = g.box_off % node_stride;
    if (node >= (uint32_t)num_nodes || (rest != 0 && rest != kSweepBoxBytes)) return -1;
    const float* box = rest ? nodes[node].rmin : nodes[node].lmin;
    for (int a = 0; a < 3; a++) {
        if (!(box[a] == box[3 + a])) continue;
        bool on_plane = true;
        for (uint64_t m = sweep_group_mask(g); m && on_plane; m = sweep_clear_lowest(m)) {
            const int32_t prim = sweep_lowest(m);
            if (prim >= num_prims || prims[prim].info < 0) { on_plane = false; break; }
            for (int v = 0; v < 3; v++) on_plane = on_plane && prims[prim].v[3 * v + a] == box[a];
        }
        if (on_plane) { *c = box[a]; return a; }
    }
    return -1;
}

// Is group g flat on `axis` at a coordinate equal to c, vertices included?  (Its own lowest flat axis may be another.)
inline bool sweep_group_on_plane(const SweepGroup& g, int axis, float c, const DNode* nodes, int num_nodes, uint32_t node_stride,
                                 const DPrim* prims, int num_prims) {
    const uint32_t node = g.box_off / node_stride, rest = g.box_off % node_stride;
    if (node >= (uint32_t)num_nodes || (rest != 0 && rest != kSweepBoxBytes)) return false;
    const float* box = rest ? nodes[node].rmin : nodes[node].lmin;
    if (!(box[axis] == c && box[3 + axis] == c)) return false;
    for (uint64_t m = sweep_group_mask(g); m; m = sweep_clear_lowest(m)) {
        const int32_t prim = sweep_lowest(m);
        if (prim >= num_prims || prims[prim].info < 0) return false;
        for (int v = 0; v < 3; v++)
            if (!(prims[prim].v[3 * v + axis] == c)) return false;
    }
    return true;
}

// Fills out[0 .. num_prims) (and zeroes the rest of the kSweepSkipTableBytes) for `groups` in the order of the table a launch
// sweeps: the order build_sweep_layout was given.  Returns false where the arguments cannot be a sweep's.
inline bool build_sweep_skip(const SweepGroup* groups, int count, const DNode* nodes, int num_nodes, uint32_t node_stride, const DPrim* prims,
                             int num_prims, unsigned char* out, SweepSkipInfo* info) {
    if (count < 1 || count > kSweepMaxBoxes || num_prims < count || num_prims > kSweepMaxPrims || num_nodes < 1) return false;
    memset(out, 0, kSweepSkipTableBytes);
    SweepSkipInfo si{0, 0};
    for (int k = 0; k < count; k++) {
        float c = 0.0f;
        const int axis = sweep_group_flat_axis(groups[k], nodes, num_nodes, node_stride, prims, num_prims, &c);
        if (axis < 0) continue;
        uint32_t mask = 0;
        for (int j = 0; j < count; j++)
            if (j == k || sweep_group_on_plane(groups[j], axis, c, nodes, num_nodes, node_stride, prims, num_prims)) mask |= 0x80000000u >> j;
        si.groups++;
        // a plane counts once, at its lowest group that has this axis as its own
        bool first = true;
        for (int j = 0; j < k && first; j++) {
            float cj = 0.0f;
            if (sweep_group_flat_axis(groups[j], nodes, num_nodes, node_stride, prims, num_prims, &cj) == axis && cj == c) first = false;
        }
        if (first) si.planes++;
        const SweepSkipEntry e{c, mask, (uint32_t)axis};
        for (uint64_t m = sweep_group_mask(groups[k]); m; m = sweep_clear_lowest(m)) {
            const int32_t prim = sweep_lowest(m);
            if (prim >= num_prims) return false;
            memcpy(out + (size_t)prim * sizeof(SweepSkipEntry), &e, sizeof(e));
        }
    }
    if (info) *info = si;
    return true;
}

// The kernel's rule: the skip word of a lane whose segment ended on `prim` and whose next segment starts at `org`.
PT_SWEEP_HD uint32_t sweep_skip_word(const SweepSkipEntry& e, const float org[3]) {
    const float oa = e.axis == 0u ? org[0] : e.axis == 1u ? org[1] : org[2];
    return oa == e.c ? e.mask : 0u;
}

}  // namespace ptl
