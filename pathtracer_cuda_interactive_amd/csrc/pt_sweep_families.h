// pt_sweep_families.h — the box sweep's PAIR2 records in front of the pair classes of pt_sweep_pairs.h.
//
// pt_sweep_pairs.h lets a pair of groups share ONE axis interval.  Small scenes share more: two faces of a block, or two
// halves of a wall, have the same interval on two axes.  One more record family, a loop of its own in the kernel
// (pt_kernels.h: sweep_pair2), each record self-contained like a pair's:
//
//   PAIR2_u(fb, fc)   two groups with bit-equal intervals on BOTH axes other than u (b < c); each of them flat or not
//
// "Bit-equal" as in pt_sweep_pairs.h: -0.0 and +0.0 are different planes.  Table order: PAIR2 (u = x, y, z; per u the four
// flatness combinations fb + 2 fc), then the classes of pt_sweep_pairs.h.  The group order stays a permutation, so
// build_sweep_layout runs unchanged on it, hit bit k names slot k and the chains need nothing new.
//
// The count model (VALU of the sweep loops): a record costs 1 for its pointer, a box 5 (max, max3, min3, compare, add with
// carry), a shared axis 4 per record, 2 where flat, an axis that is not shared 4 per box; the single has no pointer.
//
//   general pair 35   SHARE 31   SHARE_FLAT 29   single 17   PAIR2 27 / 25 / 23 (0 / 1 / 2 flat)
//
// build_sweep_families picks the records that make the model's sum smallest: a depth-first search over the lowest group not yet
// placed (a pair with it, or leave it to the general pairs), bounded by what each remaining group could save at most, started
// from the greedy pairing of build_sweep_pairs and replacing it only by a strictly smaller sum.  So the sum is never above that
// pairing's, a scene with nothing more to share keeps that pairing's order and tables byte for byte, and ties go to the lowest
// group index, then the lowest axis.  The search gives up after kSweepSearchNodes nodes and keeps the best it has
// (deterministic all the same).
//
// A QUAD family (four groups with one shared interval, that axis once for the four: 57 / 55 VALU) was built with it, matched
// the model instruction for instruction and brought cbox's sum from 353 to 342, but did not show against PAIR2 alone on the
// GPU (profiles/r16_sweep_families.log §3), so it is not here: a class stays only if it pays.
//
// Records, read as 8-byte pairs (u: the axis not shared; b < c: the other two):
//
//   PAIR2   8 floats    near_b far_b | near_c far_c | A near_u far_u | B near_u far_u      (a flat axis: plane 0)
//
// 16 B per group against build_sweep_layout's 24: the tables are never larger, the fit predicate and sweep_slots_off are
// unchanged, the pitch is an odd number of 8-byte units.
//
// The header needs no HIP header, so the CPU test tests/native/sweep_families_check.cpp runs the same code.
#pragma once
#include <stdint.h>
#include <string.h>

#include "pt_sweep_pairs.h"

namespace ptl {

constexpr uint32_t kSweepPair2Floats = 8;
constexpr uint32_t kSweepSearchNodes = 400000;
// option "sweep_families"
constexpr int kSweepFamiliesOff = 0, kSweepFamiliesOn = 1;

// Records per class of the family, in table order: three scalar words.
struct SweepFamilyClasses {
    uint8_t pair2[3][4];      // [u][fb + 2 * fc]: u the axis not shared, fb / fc: the lower / upper shared axis is flat
};
static_assert(sizeof(SweepFamilyClasses) == 12, "SweepFamilyClasses travels as three scalar words");

// Every class of a launch: the families, then the pair classes.
struct SweepClasses {
    SweepFamilyClasses fam;
    SweepPairClasses pairs;
};

PT_SWEEP_HD uint32_t sweep_pair2_records(const SweepFamilyClasses& f) {
    uint32_t n = 0;
    for (int u = 0; u < 3; u++)
        for (int k = 0; k < 4; k++) n += f.pair2[u][k];
    return n;
}
PT_SWEEP_HD uint32_t sweep_classes_groups(const SweepClasses& c) {
    return 2u * sweep_pair2_records(c.fam) + sweep_pairs_groups(c.pairs);
}
PT_SWEEP_HD SweepClasses sweep_classes_of_pairs(const SweepPairClasses& p) {
    SweepClasses c{};
    c.pairs = p;
    return c;
}
// Bytes between the 8 box tables: an odd number of 8-byte units, never more than sweep_box_pitch.
PT_SWEEP_HD uint32_t sweep_classes_pitch(const SweepClasses& c) {
    const uint32_t bytes = 4u * (kSweepPair2Floats * sweep_pair2_records(c.fam) +
                                 kSweepSharedPairFloats * (sweep_pairs_shared(c.pairs) + sweep_pairs_flat(c.pairs)) +
                                 kSweepPairFloats * c.pairs.general + kSweepSingleFloats * c.pairs.single);
    return bytes + (((bytes / 8u) & 1u) ? 0u : 8u);
}
// The end of what the kernel's record stream reads (pt_kernels.h: SweepWindow), as an offset into the staged sweep region: one
// past the furthest byte.  The stream reads a window of kSweepWindowBytes at the start of a table and behind every record but
// the single, whether a record follows or not, so the furthest read is octant 7's, behind its last pair record: into the single
// and 8 bytes past it, or 32 bytes past the table's records.  Those bytes are the table's padding and the head of the slot
// records staged behind the tables (sweep_slots_off); nothing uses them.  sweep_stream_fits is the checked property.
constexpr uint32_t kSweepWindowBytes = 32;
PT_SWEEP_HD uint32_t sweep_stream_end(const SweepClasses& c) {
    const uint32_t pair_bytes = 4u * (kSweepPair2Floats * sweep_pair2_records(c.fam) +
                                      kSweepSharedPairFloats * (sweep_pairs_shared(c.pairs) + sweep_pairs_flat(c.pairs)) +
                                      kSweepPairFloats * c.pairs.general);
    return 7u * sweep_classes_pitch(c) + pair_bytes + kSweepWindowBytes;
}
// The stream stays inside the region a block stages for `groups` groups and `num_prims` slot records.
PT_SWEEP_HD bool sweep_stream_fits(const SweepClasses& c, uint32_t groups, uint32_t num_prims) {
    return sweep_stream_end(c) <= sweep_layout_bytes(groups, num_prims);
}
// The count model: VALU instructions of the sweep loops over these classes.
PT_SWEEP_HD uint32_t sweep_valu_model(const SweepClasses& c) {
    uint32_t n = 0;
    for (int u = 0; u < 3; u++)
        for (int k = 0; k < 4; k++) n += c.fam.pair2[u][k] * (1u + 10u + 8u + ((k & 1) ? 2u : 4u) + ((k & 2) ? 2u : 4u));
    return n + 29u * sweep_pairs_flat(c.pairs) + 31u * sweep_pairs_shared(c.pairs) + 35u * c.pairs.general + 17u * c.pairs.single;
}
// Pairs that share axis `axis` (-1: any) flat / not flat: what the info keys "sweep_flat_pairs", "sweep_share_pairs"
// report.  Without an axis a PAIR2 counts once, as flat where one of its axes is; with one it counts under each axis it shares.
PT_SWEEP_HD uint32_t sweep_classes_sharing(const SweepClasses& c, bool flat, int axis) {
    uint32_t n = 0;
    for (int u = 0; u < 3; u++)
        for (int k = 0; k < 4; k++) {
            const int b = u == 0 ? 1 : 0, cc = u == 2 ? 1 : 2;
            if (axis < 0) n += ((k != 0) == flat) ? c.fam.pair2[u][k] : 0u;
            else n += (axis == b && ((k & 1) != 0) == flat) || (axis == cc && ((k & 2) != 0) == flat) ? c.fam.pair2[u][k] : 0u;
        }
    for (int a = 0; a < 3; a++)
        if (axis < 0 || axis == a) n += flat ? c.pairs.flat[a] : c.pairs.share[a];
    return n;
}

// Which axes two boxes share bit for bit, and which of those are flat.
inline void sweep_shared_axes(const float* a, const float* b, uint32_t* shared, uint32_t* flat) {
    *shared = *flat = 0;
    for (int x = 0; x < 3; x++) {
        if (memcmp(a + x, b + x, 4) != 0 || memcmp(a + 3 + x, b + 3 + x, 4) != 0) continue;
        *shared |= 1u << x;
        if (memcmp(a + x, a + 3 + x, 4) == 0) *flat |= 1u << x;
    }
}

namespace sweep_search {

// class numbers in table order: 0 .. 11 PAIR2 (4 u + fb + 2 fc), 12 .. 17 the pair classes (flat x y z, share x y z)
constexpr int kClasses = 18;
struct Record { uint8_t cls, g[2]; };
struct Pairing { Record rec[kSweepMaxBoxes / 2]; int n; int saving; };

struct State {
    int count;
    uint8_t shared[kSweepMaxBoxes][kSweepMaxBoxes], flat[kSweepMaxBoxes][kSweepMaxBoxes];
    int bound4[kSweepMaxBoxes];                  // 4 x the most a group can save as its share of a record
    uint32_t nodes;
    Pairing cur, best;
};

inline int axis_saving(bool flat) { return flat ? kSweepSavingFlat : kSweepSavingShare; }

// The pair record of i < j: class and saving (0: they share nothing).  Two boxes of different groups never share all three axes;
// should they, the record shares the lower two.
inline int pair_record(const State& s, int i, int j, int* cls) {
    uint32_t sh = s.shared[i][j];
    const uint32_t fl = s.flat[i][j];
    if (sh == 7u) sh = 3u;
    if (sh == 0) return 0;
    if ((sh & (sh - 1u)) == 0) {
        const int ax = sh == 1u ? 0 : sh == 2u ? 1 : 2;
        *cls = 12 + ((fl >> ax) & 1u ? 0 : 3) + ax;
        return axis_saving((fl >> ax) & 1u);
    }
    const int u = sh == 6u ? 0 : sh == 5u ? 1 : 2, b = u == 0 ? 1 : 0, c = u == 2 ? 1 : 2;
    const bool fb = (fl >> b) & 1u, fc = (fl >> c) & 1u;
    *cls = 4 * u + (fb ? 1 : 0) + (fc ? 2 : 0);
    return axis_saving(fb) + axis_saving(fc);
}
inline void descend(State& s, uint32_t used, int saving) {
    if (s.nodes >= kSweepSearchNodes) return;
    s.nodes++;
    int i = 0, rest4 = 0;
    while (i < s.count && ((used >> i) & 1u)) i++;
    if (i == s.count) {
        if (saving > s.best.saving) { s.best = s.cur; s.best.saving = saving; }
        return;
    }
    for (int k = i; k < s.count; k++)
        if (!((used >> k) & 1u)) rest4 += s.bound4[k];
    if (4 * saving + rest4 <= 4 * s.best.saving) return;
    const uint32_t with_i = used | 1u << i;
    for (int j = i + 1; j < s.count; j++) {
        int cls = 0;
        if (((used >> j) & 1u)) continue;
        const int w = pair_record(s, i, j, &cls);
        if (w == 0) continue;
        s.cur.rec[s.cur.n++] = Record{(uint8_t)cls, {(uint8_t)i, (uint8_t)j}};
        descend(s, with_i | 1u << j, saving + w);
        s.cur.n--;
    }
    descend(s, with_i, saving);
}

}  // namespace sweep_search

// Places `count` groups (1 .. kSweepMaxBoxes) in PAIR2 records and the pair classes so that sweep_valu_model is smallest.
// mode: kSweepFamiliesOn, or kSweepFamiliesOff (build_sweep_pairs' pairing as it is).
// out[k] = groups[perm[k]] in class order.  Returns false where a group names no box.
inline bool build_sweep_families(const SweepGroup* groups, int count, const DNode* nodes, int num_nodes, uint32_t node_stride, int mode,
                                 SweepGroup* out, int* perm, SweepClasses* classes) {
    using namespace sweep_search;
    SweepPairClasses greedy{};
    if (!build_sweep_pairs(groups, count, nodes, num_nodes, node_stride, out, perm, &greedy)) return false;
    *classes = sweep_classes_of_pairs(greedy);
    if (mode == kSweepFamiliesOff) return true;
    State st;
    State* s = &st;
    s->count = count;
    s->nodes = 0;
    s->cur.n = 0; s->cur.saving = 0;
    s->best.n = 0;
    s->best.saving = kSweepSavingFlat * (int)sweep_pairs_flat(greedy) + kSweepSavingShare * (int)sweep_pairs_shared(greedy);
    for (int i = 0; i < count; i++) {
        s->bound4[i] = 0;
        for (int j = 0; j < count; j++) {
            uint32_t sh = 0, fl = 0;
            if (i != j)
                sweep_shared_axes(sweep_group_box(groups[i], nodes, num_nodes, node_stride), sweep_group_box(groups[j], nodes, num_nodes, node_stride), &sh, &fl);
            s->shared[i][j] = (uint8_t)sh;
            s->flat[i][j] = (uint8_t)fl;
        }
    }
    for (int i = 0; i < count; i++) {
        for (int j = 0; j < count; j++) {
            if (i == j) continue;
            int cls;
            const int w = pair_record(*s, i < j ? i : j, i < j ? j : i, &cls);
            if (2 * w > s->bound4[i]) s->bound4[i] = 2 * w;
        }
    }
    descend(*s, 0u, 0);
    if (s->best.n == 0) return true;            // nothing beats the greedy pairing: its order, its tables
    // class order; inside a class the order the search placed the records in (ascending lowest group)
    SweepClasses c{};
    bool placed[kSweepMaxBoxes] = {};
    int n = 0;
    for (int cls = 0; cls < kClasses; cls++)
        for (int r = 0; r < s->best.n; r++) {
            const Record& rec = s->best.rec[r];
            if (rec.cls != cls) continue;
            for (int k = 0; k < 2; k++) { perm[n++] = rec.g[k]; placed[rec.g[k]] = true; }
            if (cls < 12) c.fam.pair2[cls / 4][cls % 4]++;
            else if (cls < 15) c.pairs.flat[cls - 12]++;
            else c.pairs.share[cls - 15]++;
        }
    const int in_records = n;
    for (int k = 0; k < count; k++)
        if (!placed[k]) perm[n++] = k;
    c.pairs.general = (uint8_t)((count - in_records) / 2);
    c.pairs.single = (uint8_t)((count - in_records) & 1);
    for (int k = 0; k < count; k++) out[k] = groups[perm[k]];
    *classes = c;
    return true;
}

// build_sweep_pair_tables with the PAIR2 records in front: overwrites the box tables at the head of `out` (a layout build_sweep_layout
// made of the SAME permuted groups) with the 8 tables in class order at sweep_classes_pitch; what is left of the region is zero.
// Returns false where the classes do not add up to `count`, a group names no box or a record does not share what its class says.
inline bool build_sweep_family_tables(const SweepGroup* groups, int count, const SweepClasses& classes, const DNode* nodes, int num_nodes,
                                      uint32_t node_stride, unsigned char* out) {
    if (count < 1 || count > kSweepMaxBoxes || sweep_classes_groups(classes) != (uint32_t)count || classes.pairs.single > 1) return false;
    const uint32_t fam_groups = 2u * sweep_pair2_records(classes.fam);
    if (fam_groups == 0) return build_sweep_pair_tables(groups, count, classes.pairs, nodes, num_nodes, node_stride, out);
    const uint32_t pitch = sweep_classes_pitch(classes);
    if (8u * pitch > sweep_slots_off((uint32_t)count)) return false;
    // the pair classes behind the families: build_sweep_pair_tables on the groups they own, at its own pitch, then moved into place
    const int rest = count - (int)fam_groups;
    unsigned char tail[8u * (kSweepMaxBoxes * kSweepBoxBytes + 8u)];
    const uint32_t tail_pitch = rest ? sweep_pairs_pitch(classes.pairs) : 0;
    const uint32_t tail_bytes = 4u * (kSweepSharedPairFloats * (sweep_pairs_shared(classes.pairs) + sweep_pairs_flat(classes.pairs)) +
                                      kSweepPairFloats * classes.pairs.general + kSweepSingleFloats * classes.pairs.single);
    if (rest && !build_sweep_pair_tables(groups + fam_groups, rest, classes.pairs, nodes, num_nodes, node_stride, tail)) return false;
    memset(out, 0, sweep_slots_off((uint32_t)count));
    for (uint32_t o = 0; o < 8; o++) {
        float* w = reinterpret_cast<float*>(out + o * pitch);
        int k = 0;
        bool ok = true;
        // near and far plane of group g on axis a for this octant: bit a set <=> 1/d[a] < 0, the near plane is the box's max
        auto plane = [&](int g, int a, bool far) {
            const float* box = sweep_group_box(groups[g], nodes, num_nodes, node_stride);
            if (!box) { ok = false; return 0.0f; }
            const bool neg = (o >> a) & 1u;
            return box[(neg != far) ? 3 + a : a];
        };
        auto shares = [&](int g, int h, int a, bool flat) {
            const float n0 = plane(g, a, false), n1 = plane(h, a, false), f0 = plane(g, a, true), f1 = plane(h, a, true);
            return ok && memcmp(&n0, &n1, 4) == 0 && memcmp(&f0, &f1, 4) == 0 && (memcmp(&n0, &f0, 4) == 0) == flat;
        };
        for (int u = 0; u < 3; u++)
            for (int f = 0; f < 4; f++)
                for (int p = 0; p < classes.fam.pair2[u][f]; p++, k += 2) {
                    const int b = u == 0 ? 1 : 0, c = u == 2 ? 1 : 2;
                    const bool fb = f & 1, fc = f & 2;
                    if (!shares(k, k + 1, b, fb) || !shares(k, k + 1, c, fc)) return false;
                    const float rec[kSweepPair2Floats] = {plane(k, b, false), fb ? 0.0f : plane(k, b, true), plane(k, c, false), fc ? 0.0f : plane(k, c, true),
                                                          plane(k, u, false), plane(k, u, true), plane(k + 1, u, false), plane(k + 1, u, true)};
                    memcpy(w, rec, sizeof(rec));
                    w += kSweepPair2Floats;
                }
        if (!ok) return false;
        if (rest) memcpy(w, tail + o * tail_pitch, tail_bytes);
    }
    return true;
}

}  // namespace ptl
