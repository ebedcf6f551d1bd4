// pt_sweep_layout.h — what trace_kernel_v2_sweep stages in place of the 8 octant node tables: the leaf sweep's own tables.
//
// The sweep (pt_leaf_sweep.h) never walks the tree, so the block needs of it only the group boxes, and of the primitives only
// what a leaf test reads.  Made once at scene creation from the groups of build_sweep_groups:
//
//   box tables    8 octants x G groups x 24 B.  Group k of octant o is (near.xyz, far.xyz) of the group's box for that octant: the
//                 six floats the octant node table holds at SweepGroup::box_off, bit for bit.  A lane reads its octant's table
//                 front to back through a pointer, two groups per iteration, and keeps ONE hit bit per group.
//   slot records  one 48-B record per primitive, a DPrim whose spare word is a link: prim | next_slot << 8.
//                 Slot k < G is the first (lowest) primitive of group k; the other primitives of a group follow from slot G
//                 upwards, chained through next_slot; next_slot == 0 means "none" (slot 0 is never a successor).
//                 A set hit bit k names slot k, and the chain from there is the group.
//
// The global table keeps p0, p1, p2; the block that stages a record into LDS replaces p1, p2 by the edges p1 - p0, p2 - p0
// (sweep_stage_record), so the subtraction of the triangle test runs once per block instead of once per test: same operands,
// same operation, same bits.
//
// The header needs no HIP header, so the CPU test tests/native/sweep_layout_check.cpp runs the same code.
#pragma once
#include <stdint.h>
#include <string.h>

#include "pt_layout.h"
#include "pt_leaf_sweep.h"

namespace ptl {

static_assert(kSweepMaxBoxes <= 32, "one hit bit per group in a 32-bit register");
static_assert(kSweepMaxPrims <= 256, "a link word holds a primitive and a slot in a byte each");

// Bytes between the 8 box tables.  G boxes are 3 G units of 8 B; like oct_table_pitch the pitch is made an ODD number of the
// unit the reads are aligned to (here 8 B: a box is read as three 8-B pairs), so that o * pitch for o = 0 .. 7 are 8 different
// positions among the 32 that 8-B units have in LDS's 64 banks.
PT_SWEEP_HD uint32_t sweep_box_pitch(uint32_t groups) {
    const uint32_t bytes = groups * kSweepBoxBytes;
    return bytes + (((bytes / 8u) & 1u) ? 0u : 8u);
}
// Byte offset of the slot records behind the box tables (8 * pitch is a multiple of 64), and of the end of the layout.
PT_SWEEP_HD uint32_t sweep_slots_off(uint32_t groups) { return 8u * sweep_box_pitch(groups); }
PT_SWEEP_HD uint32_t sweep_layout_bytes(uint32_t groups, uint32_t num_prims) {
    return sweep_slots_off(groups) + num_prims * (uint32_t)sizeof(DPrim);
}
// Does the layout fit where the octant node tables of `num_nodes` nodes would be staged (LdsPlan: the node region)?  For a
// binary tree over N >= 3 primitives it does: at most 192 G + 64 + 48 N <= 240 N + 128 bytes against 512 (N - 1) and more.
PT_SWEEP_HD bool sweep_layout_fits(uint32_t groups, uint32_t num_prims, uint32_t num_nodes, uint32_t node_stride) {
    return sweep_layout_bytes(groups, num_prims) <= 8u * oct_table_pitch(num_nodes, node_stride);
}

// The link word of a slot record.
PT_SWEEP_HD uint32_t sweep_link(uint32_t prim, uint32_t next_slot) { return prim | next_slot << 8; }
PT_SWEEP_HD uint32_t sweep_link_prim(uint32_t link) { return link & 0xffu; }
PT_SWEEP_HD uint32_t sweep_link_next(uint32_t link) { return link >> 8; }

// The hit word of a lane: group k is bit 31 - k, so that the groups come out in their order, lowest group first.
// The sweep loop shifts a bit in per group (hits = 2 * hits + hit); after G groups sweep_hits_align moves group 0 to bit 31.
PT_SWEEP_HD uint32_t sweep_hits_align(uint32_t hits, uint32_t groups) { return hits << (32u - groups); }      // 1 <= groups <= 32
PT_SWEEP_HD uint32_t sweep_first_group(uint32_t hits) { return (uint32_t)__builtin_clz(hits); }               // hits != 0
PT_SWEEP_HD uint32_t sweep_clear_group(uint32_t hits, uint32_t k) { return hits & ~(0x80000000u >> k); }

// Fills `out` (sweep_layout_bytes(count, num_prims) bytes, zeroed here) from the groups build_sweep_groups made of `nodes`
// (plain layout, the same node_stride) and the primitive records.  Returns false where the arguments cannot be laid out.
inline bool build_sweep_layout(const SweepGroup* groups, int count, const DNode* nodes, int num_nodes, uint32_t node_stride,
                               const DPrim* prims, int num_prims, unsigned char* out) {
    if (count < 1 || count > kSweepMaxBoxes || num_prims < count || num_prims > kSweepMaxPrims || num_nodes < 1) return false;
    memset(out, 0, sweep_layout_bytes((uint32_t)count, (uint32_t)num_prims));
    const uint32_t pitch = sweep_box_pitch((uint32_t)count);
    for (int k = 0; k < count; k++) {
        const uint32_t node = groups[k].box_off / node_stride, rest = groups[k].box_off % node_stride;
        if (node >= (uint32_t)num_nodes || (rest != 0 && rest != kSweepBoxBytes)) return false;
        const float* box = rest ? nodes[node].rmin : nodes[node].lmin;             // min[3] then max[3], contiguous
        for (uint32_t o = 0; o < 8; o++) {
            // octant bit a set <=> 1/d[a] < 0: the near plane of axis a is the box's max (pt_scene_life.hip: upload_tree)
            float nf[6];
            for (int a = 0; a < 3; a++) {
                const bool neg = (o >> a) & 1u;
                nf[a] = box[neg ? 3 + a : a];
                nf[3 + a] = box[neg ? a : 3 + a];
            }
            memcpy(out + o * pitch + (uint32_t)k * kSweepBoxBytes, nf, kSweepBoxBytes);
        }
    }
    DPrim* slots = reinterpret_cast<DPrim*>(out + sweep_slots_off((uint32_t)count));
    int next_free = count;
    for (int k = 0; k < count; k++) {
        uint64_t m = sweep_group_mask(groups[k]);
        if (m == 0) return false;
        int slot = k;
        while (m) {
            const int32_t prim = sweep_lowest(m);
            m = sweep_clear_lowest(m);
            if (prim >= num_prims || (m && next_free >= num_prims)) return false;
            const int next = m ? next_free++ : 0;
            slots[slot] = prims[prim];
            slots[slot].pad = (int32_t)sweep_link((uint32_t)prim, (uint32_t)next);
            slot = next;
        }
    }
    return next_free == num_prims;
}

// A slot record as the kernel keeps it in LDS: p0, e1 = p1 - p0, e2 = p2 - p0 in place of p0, p1, p2 (triangles only; the
// sweep kernel is compiled for triangles).  Plain fp32 subtractions, the ones Möller–Trumbore starts with (shape.cuh:190-191).
PT_SWEEP_HD DPrim sweep_stage_record(const DPrim& g) {
    DPrim r = g;
    for (int a = 0; a < 3; a++) {
        r.v[3 + a] = g.v[3 + a] - g.v[a];
        r.v[6 + a] = g.v[6 + a] - g.v[a];
    }
    return r;
}

}  // namespace ptl
