// pt_sweep_pairs.h — the box sweep's groups paired up by what their boxes share, and the box tables in that order.
//
// The sweep loop of trace_kernel_v2_sweep (pt_trace_sweep_body.h, step (3)) tests two groups per iteration.  Two boxes with the
// same interval on an axis — both floats equal BIT FOR BIT, so -0.0 and +0.0 are different planes — get the same two slab
// products (plane - o) * 1/d from the same operands, and an interval with min == max gets the same product twice.  Axis-aligned
// walls, floors and block faces are what small scenes are made of: cbox's 25 boxes have 8 distinct y intervals, 12 of them flat.
// So the host pairs the groups and the kernel computes a shared axis once, inside ONE iteration; nothing is carried from one
// iteration to the next.  Classes, in table order, with the VALU a pair saves of the general pair's 35:
//
//   SHARE_FLAT_x, _y, _z   both boxes flat on the axis in the same plane: one sub and one mul where eight stood        -6
//   SHARE_x, _y, _z        both boxes have the same (min, max) on the axis: the axis once                               -4
//   general pairs          two leftover groups, the pair loop as it was
//   single                 at most one: an odd count's last group, the tail as it was
//
// Pairs are picked greedily by saving, ties by the lowest group index, then the lowest axis: deterministic.  The result is a
// permutation of the groups; build_sweep_layout (pt_sweep_layout.h) runs UNCHANGED on the permuted array, so hit bit k still
// names slot k and the chains need no new code.  build_sweep_pair_tables then overwrites the 8 octant box tables with records
// in class order:
//
//   general pair   12 floats   A near.xyz far.xyz, B near.xyz far.xyz (what build_sweep_layout wrote)
//   SHARE_a pair   10 floats   near_a far_a | A near_b near_c | A far_b far_c | B near_b near_c | B far_b far_c   (b < c, the other axes)
//   FLAT_a pair    10 floats   plane_a 0    | the same eight.  9 floats padded to 10: every record is read as 8-byte pairs
//   single          6 floats   near.xyz far.xyz
//
// The tables are never larger than build_sweep_layout's (a record is at most 24 B per group), so they are staged where those
// are, under the same fit predicate, and the slot records stay at sweep_slots_off(groups).  The pitch follows the same rule: an
// odd number of 8-byte units.  With every pair general the tables are build_sweep_layout's own, byte for byte.
// A flat axis of a box that shares it with no partner is left alone: it would take a loop body per axis and class on top of these.
//
// The header needs no HIP header, so the CPU test tests/native/sweep_pairs_check.cpp runs the same code.
#pragma once
#include <stdint.h>
#include <string.h>

#include "pt_sweep_layout.h"

namespace ptl {

constexpr uint32_t kSweepPairFloats = 12, kSweepSharedPairFloats = 10, kSweepSingleFloats = 6;
constexpr int kSweepSavingFlat = 6, kSweepSavingShare = 4;

// Pairs per class, in table order; 2 * (every pair) + single = the group count.
struct SweepPairClasses {
    uint8_t flat[3];      // SHARE_FLAT_x, _y, _z
    uint8_t share[3];     // SHARE_x, _y, _z
    uint8_t general;
    uint8_t single;       // 0 or 1
};
static_assert(sizeof(SweepPairClasses) == 8, "SweepPairClasses travels as two scalar words");

PT_SWEEP_HD uint32_t sweep_pairs_shared(const SweepPairClasses& c) { return (uint32_t)c.share[0] + c.share[1] + c.share[2]; }
PT_SWEEP_HD uint32_t sweep_pairs_flat(const SweepPairClasses& c) { return (uint32_t)c.flat[0] + c.flat[1] + c.flat[2]; }
PT_SWEEP_HD uint32_t sweep_pairs_groups(const SweepPairClasses& c) {
    return 2u * (sweep_pairs_shared(c) + sweep_pairs_flat(c) + c.general) + c.single;
}
// Every pair general: the order and the tables of build_sweep_layout.
PT_SWEEP_HD SweepPairClasses sweep_pairs_none(uint32_t groups) {
    SweepPairClasses c{};
    c.general = (uint8_t)(groups >> 1);
    c.single = (uint8_t)(groups & 1u);
    return c;
}
// Bytes between the 8 box tables in class order: an odd number of 8-byte units, like sweep_box_pitch, and never more than it.
PT_SWEEP_HD uint32_t sweep_pairs_pitch(const SweepPairClasses& c) {
    const uint32_t bytes = 4u * (kSweepSharedPairFloats * (sweep_pairs_shared(c) + sweep_pairs_flat(c)) + kSweepPairFloats * c.general +
                                 kSweepSingleFloats * c.single);
    return bytes + (((bytes / 8u) & 1u) ? 0u : 8u);
}

// The box (min[3] then max[3]) a group names inside the plain node table, or null where it names none.
inline const float* sweep_group_box(const SweepGroup& g, const DNode* nodes, int num_nodes, uint32_t node_stride) {
    const uint32_t node = g.box_off / node_stride, rest = g.box_off % node_stride;
    if (node >= (uint32_t)num_nodes || (rest != 0 && rest != kSweepBoxBytes)) return nullptr;
    return rest ? nodes[node].rmin : nodes[node].lmin;
}

// What pairing two boxes saves, and on which axis (the lowest among the best): both flat in one plane, or the same interval.
inline int sweep_pair_saving(const float* a, const float* b, int* axis) {
    int best = 0;
    *axis = -1;
    for (int x = 0; x < 3; x++) {
        if (memcmp(a + x, b + x, 4) != 0 || memcmp(a + 3 + x, b + 3 + x, 4) != 0) continue;      // bits: -0.0 is not +0.0
        const int s = memcmp(a + x, a + 3 + x, 4) == 0 ? kSweepSavingFlat : kSweepSavingShare;
        if (s > best) { best = s; *axis = x; }
    }
    return best;
}

// Pairs `count` groups (1 .. kSweepMaxBoxes) greedily by saving.  out[k] = groups[perm[k]] in class order, classes = the counts.
// Returns false where a group names no box.
inline bool build_sweep_pairs(const SweepGroup* groups, int count, const DNode* nodes, int num_nodes, uint32_t node_stride,
                              SweepGroup* out, int* perm, SweepPairClasses* classes) {
    if (count < 1 || count > kSweepMaxBoxes) return false;
    const float* box[kSweepMaxBoxes];
    for (int k = 0; k < count; k++)
        if (!(box[k] = sweep_group_box(groups[k], nodes, num_nodes, node_stride))) return false;
    bool used[kSweepMaxBoxes] = {};
    int pair_of[6][kSweepMaxBoxes];                  // per class: the groups of its pairs, two by two, in the order picked
    int n_of[6] = {0, 0, 0, 0, 0, 0};
    for (;;) {
        int best = 0, bi = -1, bj = -1, ba = -1;
        for (int i = 0; i < count; i++) {
            if (used[i]) continue;
            for (int j = i + 1; j < count; j++) {
                if (used[j]) continue;
                int axis;
                const int s = sweep_pair_saving(box[i], box[j], &axis);
                if (s > best) { best = s; bi = i; bj = j; ba = axis; }            // strictly more: the lowest (i, j) keeps a tie
            }
        }
        if (best == 0) break;
        const int cls = (best == kSweepSavingFlat ? 0 : 3) + ba;
        pair_of[cls][n_of[cls]++] = bi;
        pair_of[cls][n_of[cls]++] = bj;
        used[bi] = used[bj] = true;
    }
    int n = 0;
    SweepPairClasses c{};
    for (int cls = 0; cls < 6; cls++) {
        for (int k = 0; k < n_of[cls]; k++) perm[n++] = pair_of[cls][k];
        (cls < 3 ? c.flat[cls] : c.share[cls - 3]) = (uint8_t)(n_of[cls] / 2);
    }
    const int paired = n;
    for (int k = 0; k < count; k++)
        if (!used[k]) perm[n++] = k;
    c.general = (uint8_t)((count - paired) / 2);
    c.single = (uint8_t)((count - paired) & 1);
    for (int k = 0; k < count; k++) out[k] = groups[perm[k]];
    *classes = c;
    return true;
}

// Overwrites the box tables at the head of `out` (a layout build_sweep_layout made of the SAME permuted groups: the first
// sweep_slots_off(count) bytes) with the 8 tables in class order at sweep_pairs_pitch; what is left of the region is zero.
// Returns false where the classes do not add up to `count`, a group names no box or a sharing pair does not share.
inline bool build_sweep_pair_tables(const SweepGroup* groups, int count, const SweepPairClasses& classes, const DNode* nodes,
                                    int num_nodes, uint32_t node_stride, unsigned char* out) {
    if (count < 1 || count > kSweepMaxBoxes || sweep_pairs_groups(classes) != (uint32_t)count || classes.single > 1) return false;
    const uint32_t pitch = sweep_pairs_pitch(classes);
    if (8u * pitch > sweep_slots_off((uint32_t)count)) return false;
    memset(out, 0, sweep_slots_off((uint32_t)count));
    for (uint32_t o = 0; o < 8; o++) {
        float* w = reinterpret_cast<float*>(out + o * pitch);
        int k = 0;
        // near and far planes of group g for this octant: bit a set <=> 1/d[a] < 0, the near plane of axis a is the box's max
        auto planes = [&](int g, float* nf) {
            const float* box = sweep_group_box(groups[g], nodes, num_nodes, node_stride);
            if (!box) return false;
            for (int a = 0; a < 3; a++) {
                const bool neg = (o >> a) & 1u;
                nf[a] = box[neg ? 3 + a : a];
                nf[3 + a] = box[neg ? a : 3 + a];
            }
            return true;
        };
        for (int cls = 0; cls < 6; cls++) {
            const int ax = cls % 3, b = ax == 0 ? 1 : 0, c = ax == 2 ? 1 : 2;
            const bool flat = cls < 3;
            for (int p = 0; p < (flat ? classes.flat[ax] : classes.share[ax]); p++, k += 2) {
                float A[6], B[6];
                if (!planes(k, A) || !planes(k + 1, B)) return false;
                if (memcmp(&A[ax], &B[ax], 4) != 0 || memcmp(&A[3 + ax], &B[3 + ax], 4) != 0) return false;
                if (flat && memcmp(&A[ax], &A[3 + ax], 4) != 0) return false;
                const float rec[kSweepSharedPairFloats] = {A[ax], flat ? 0.0f : A[3 + ax], A[b], A[c], A[3 + b], A[3 + c], B[b], B[c], B[3 + b], B[3 + c]};
                memcpy(w, rec, sizeof(rec));
                w += kSweepSharedPairFloats;
            }
        }
        for (int p = 0; p < 2 * classes.general + classes.single; p++, k++) {
            float A[6];
            if (!planes(k, A)) return false;
            memcpy(w, A, sizeof(A));
            w += kSweepSingleFloats;
        }
    }
    return true;
}

}  // namespace ptl
